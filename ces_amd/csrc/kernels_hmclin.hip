// The leapfrog step of MCMC.model_mh(chains=M, update='hmc') for the LINEAR maps (lineal, lineal_log) at any p
// (include/cesx.h, cesx_mh_hmc_lineal_*): the GEMM form of kernels_hmc.hip's step, on the launches of the Langevin step of
// kernels_lvlin.hip.  With S the scale, g = S^T grad phi, e the multiplier of an armed handle (1 otherwise) and L leapfrogs,
//
//     begin    r = xi - (e / 2) g(U)                          hl_kick_kernel (unarmed: lvlin_z_kernel itself, its bits)
//              Q = U + S z,  z = e r                          the random walk's triangular update launch
//     leap     g(Q)                                           lin_grad of engine.hip: one or two update launches (+ lvlin_exph_kernel)
//              r = r - e g(Q),  z = e r                       hl_kick_kernel
//              Qnext = Q + S z                                the triangular launch again, into the OTHER position buffer
//     accept   g(Q), phi(Q), |xi|^2, |r - (e / 2) g(Q)|^2     lin_grad, then hl_accept_kernel: the test and the masked copies
//
// so what is not a GEMM is two kernels.  The momentum r is a [p][J] block of the engine dtype between the launches (mh.lin_z;
// armed: mh.lin_r, with z = e r in mh.lin_z, so that nothing stored is rescaled).  phi is formed at the last position only.
//
// hl_accept_kernel is lvlin_accept_kernel with another second norm: V chains per lane through 16-byte loads, the rows of a
// column split over the 16 waves of a workgroup (row r to wave r % 16), every sum in fp64 in a fixed order -- each wave its
// rows ascending, then the waves' partials through ONE LDS block in wave order, one sum at a time (32 KiB for fp32, 16 KiB
// for fp64: three blocks at once halved the workgroups per CU) --, thread c < 64 V tests chain c.  The data and prior sums
// are mh_accept_kernel's in its order, so phi equals cesx_mh_start's bit for bit.  No atomics; a NaN anywhere in a chain's
// sums rejects that chain alone (the test is a `<`).  ADAPT: alpha_j = min(1, exp d), 0 for a NaN, for ad_update_kernel.
// Bound: HBM (G, the prior rows, xi, r, g(Q) once; Q and g(Q) again, U and g(U) written, for the accepted columns).
#include "cesx_internal.h"

namespace cesx {

constexpr int HL_NW = 16;                 // waves per workgroup (LL_NW of kernels_lvlin.hip)
constexpr int HL_THREADS = HL_NW * 64;
constexpr int HL_EW_THREADS = 256;        // the element-wise kernel

template <typename T> struct HlVec;
template <> struct HlVec<float> { static constexpr int V = 4; };
template <> struct HlVec<double> { static constexpr int V = 2; };

template <typename T>
struct HlArgs {
    const T* G; const double* y; const double* gw; int n;      // data rows (whitened for a dense Gamma)
    const T* X; const double* mu; const double* sw; int nx;    // prior rows: the states with mu, 1 / Sigma_rr, or w with nullptr, nullptr
    const T* xi; const T* r; const T* gq;                      // the step's noise block, the momentum before the last half kick, g(Q)
    const T* Q; T* U; T* gU; int p;                            // accepted columns of Q into U and of gq into gU
    long long J;
    const double* e;                                           // ADAPT: the step multiplier (mh.ad_state[0])
    double* alpha;                                             // ADAPT: [J] the chains' acceptance probabilities of this step
    MhChains c;
};

// V consecutive values of one row from column j0 on, in fp64 (VEC: j0 + V <= J and 16-byte aligned)
template <typename T, bool VEC>
__device__ __forceinline__ void hl_load(const T* __restrict__ row, long long j0, long long J, double out[]) {
    constexpr int V = HlVec<T>::V;
    if (VEC) {
        typedef T vt __attribute__((ext_vector_type(V)));
        const vt v = *reinterpret_cast<const vt*>(row + j0);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = (double)v[e];
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = j0 + e < J ? (double)row[j0 + e] : 0.0;
    }
}

template <typename T, bool VEC, bool ADAPT>
__global__ __launch_bounds__(HL_THREADS)
void hl_accept_kernel(const HlArgs<T> a) {
    constexpr int V = HlVec<T>::V;
    constexpr int BN = 64 * V;                 // chains per workgroup
    __shared__ double part[HL_NW][BN];         // one sum at a time: phi's, then |xi|^2, then |r - (e / 2) g_Q|^2
    __shared__ int take[BN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long j0 = (long long)blockIdx.x * BN + (long long)lane * V;
    const bool vec = VEC && j0 + V <= a.J;
    double he = 0.5;
    if constexpr (ADAPT) he = 0.5 * *a.e;      // (a uniform load)
    double s[V], n1[V], n2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s[e] = 0.0; n1[e] = 0.0; n2[e] = 0.0; }
    if (j0 < a.J) {
#pragma unroll 4
        for (int i = wave; i < a.n; i += HL_NW) {
            double g[V];
            if (vec) hl_load<T, true>(a.G + (size_t)i * a.J, j0, a.J, g);
            else hl_load<T, false>(a.G + (size_t)i * a.J, j0, a.J, g);
            const double yi = a.y[i], wi = a.gw[i];
#pragma unroll
            for (int e = 0; e < V; ++e) { const double d = g[e] - yi; s[e] += wi * (d * d); }
        }
#pragma unroll 4
        for (int r = wave; r < a.nx; r += HL_NW) {
            double x[V];
            if (vec) hl_load<T, true>(a.X + (size_t)r * a.J, j0, a.J, x);
            else hl_load<T, false>(a.X + (size_t)r * a.J, j0, a.J, x);
            const double m = a.mu ? a.mu[r] : 0.0, wr = a.sw ? a.sw[r] : 1.0;
#pragma unroll
            for (int e = 0; e < V; ++e) { const double d = x[e] - m; s[e] += wr * (d * d); }
        }
#pragma unroll 2
        for (int r = wave; r < a.p; r += HL_NW) {
            double x[V], mo[V], gq[V];
            const size_t o = (size_t)r * a.J;
            if (vec) { hl_load<T, true>(a.xi + o, j0, a.J, x); hl_load<T, true>(a.r + o, j0, a.J, mo); hl_load<T, true>(a.gq + o, j0, a.J, gq); }
            else { hl_load<T, false>(a.xi + o, j0, a.J, x); hl_load<T, false>(a.r + o, j0, a.J, mo); hl_load<T, false>(a.gq + o, j0, a.J, gq); }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double d = mo[e] - he * gq[e];
                n1[e] = fma(x[e], x[e], n1[e]);
                n2[e] = fma(d, d, n2[e]);
            }
        }
    }
    // the waves' partials in wave order, one sum at a time through the one LDS block; thread c < BN sums chain c of the workgroup
    const int tid = threadIdx.x;
    double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (q > 0) __syncthreads();
#pragma unroll
        for (int e = 0; e < V; ++e) part[wave][lane * V + e] = q == 0 ? s[e] : q == 1 ? n1[e] : n2[e];
        __syncthreads();
        if (tid < BN) {
            double acc = 0.0;
#pragma unroll
            for (int w = 0; w < HL_NW; ++w) acc += part[w][tid];
            t[q] = acc;
        }
    }
    if (tid < BN) {
        const long long j = (long long)blockIdx.x * BN + tid;
        int acc = 0;
        if (j < a.J) {
            const double ph = 0.5 * t[0];
            const double lu = a.c.logu ? a.c.logu[j]
                                       : mh_log_uniform((unsigned long long)(a.c.j_offset + j), a.c.step, a.c.seed_lo, a.c.seed_hi);
            const double d = a.c.phi[j] - ph + (0.5 * t[1] - 0.5 * t[2]);
            if constexpr (ADAPT) a.alpha[j] = d >= 0.0 ? 1.0 : d < 0.0 ? exp(d) : 0.0;      // (NaN: neither comparison holds)
            if (lu < d) {
                a.c.phi[j] = ph;
                a.c.cnt[j] += 1ull;
                acc = 1;
            }
        }
        take[tid] = acc;
    }
    __syncthreads();
    // the accepted columns: U := Q and g(U) := g(Q) (every wave its rows)
    int tk[V];
    bool any = false, all = true;
#pragma unroll
    for (int e = 0; e < V; ++e) { tk[e] = take[lane * V + e]; any = any || tk[e]; all = all && tk[e]; }
    if (!any) return;
    typedef T vt __attribute__((ext_vector_type(V)));
    for (int r = wave; r < a.p; r += HL_NW) {
        const size_t o = (size_t)r * a.J + j0;
        if (vec && all) {
            *reinterpret_cast<vt*>(a.U + o) = *reinterpret_cast<const vt*>(a.Q + o);
            *reinterpret_cast<vt*>(a.gU + o) = *reinterpret_cast<const vt*>(a.gq + o);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (tk[e]) { a.U[o + e] = a.Q[o + e]; a.gU[o + e] = a.gq[o + e]; }      // (tk[e] != 0 only for j0 + e < J)
        }
    }
}

// The kick over the len = p J elements of the engine's own blocks (16-byte aligned: whole vectors, then the tail).
//   ADAPT false   r = r - g                            (mid-trajectory; the begin form is lvlin_z_kernel)
//   ADAPT true    r = src - c g,  z = e r              begin: src = xi, c = e / 2;  mid-trajectory: src = r, c = e
template <typename T, bool ADAPT>
__global__ __launch_bounds__(HL_EW_THREADS)
void hl_kick_kernel(const T* src, const T* __restrict__ g, T* r, T* __restrict__ z, const double* __restrict__ ep, size_t len,
                    int begin) {
    constexpr int V = HlVec<T>::V;
    typedef T vt __attribute__((ext_vector_type(V)));
    T e = (T)1, c = (T)1;
    if constexpr (ADAPT) {
        const double ed = *ep;                 // (a uniform load: ad_update_kernel stored it behind the last accept)
        e = (T)ed;
        c = begin ? (T)(0.5 * ed) : e;
    }
    const size_t nv = len / V, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        const vt x = reinterpret_cast<const vt*>(src)[i], q = reinterpret_cast<const vt*>(g)[i];
        vt o, w;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if constexpr (ADAPT) { o[k] = x[k] - c * q[k]; w[k] = e * o[k]; }
            else o[k] = x[k] - q[k];
        }
        reinterpret_cast<vt*>(r)[i] = o;
        if constexpr (ADAPT) reinterpret_cast<vt*>(z)[i] = w;
    }
    const size_t k = nv * V + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < len) {
        if constexpr (ADAPT) { const T o = src[k] - c * g[k]; r[k] = o; z[k] = e * o; }
        else r[k] = src[k] - g[k];
    }
}

static unsigned hl_ew_grid(const Engine& e, size_t work) {
    const size_t want = (work + HL_EW_THREADS - 1) / HL_EW_THREADS;
    const size_t cap = (size_t)e.num_cus * 16;
    return (unsigned)std::max<size_t>(1, std::min(want, cap));
}

template <typename T>
static int hl_kick_t(Engine& e, bool begin, hipStream_t s) {
    const size_t len = (size_t)e.p * (size_t)e.J;
    constexpr int V = HlVec<T>::V;
    const size_t work = len / V + V;          // (whole vectors; the tail of fewer than V elements rides in the first threads)
    const dim3 grid(hl_ew_grid(e, work)), block(HL_EW_THREADS);
    if (e.mh.ad_armed) {
        T* r = (T*)e.mh.lin_r.get();
        hipLaunchKernelGGL((hl_kick_kernel<T, true>), grid, block, 0, s, begin ? (const T*)e.mh.xi.get() : (const T*)r,
                           (const T*)(begin ? e.mh.lin_g.get() : e.mh.lin_gp.get()), r, (T*)e.mh.lin_z.get(),
                           (const double*)e.mh.ad_state.get(), len, begin ? 1 : 0);
    } else {
        T* r = (T*)e.mh.lin_z.get();
        hipLaunchKernelGGL((hl_kick_kernel<T, false>), grid, block, 0, s, (const T*)r, (const T*)e.mh.lin_gp.get(), r, (T*)nullptr,
                           (const double*)nullptr, len, 0);
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

// begin: r = xi - (e / 2) g(U); otherwise r -= e g(Q) (mh.lin_gp).  Unarmed r lives in mh.lin_z and the begin form is
// lvlin_z_kernel's launch; armed r lives in mh.lin_r (the caller has allocated it) and z = e r goes to mh.lin_z
int launch_hl_kick(Engine& e, bool begin, hipStream_t s) {
    if (begin && !e.mh.ad_armed) return launch_lvlin_z(e, s);
    return e.cfg.dtype == CESX_F32 ? hl_kick_t<float>(e, begin, s) : hl_kick_t<double>(e, begin, s);
}

template <typename T>
static int hl_accept_t(Engine& e, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    constexpr int V = HlVec<T>::V, BN = 64 * V;
    const bool dense = !e.diag_sigma;
    HlArgs<T> a{};
    a.G = (const T*)G; a.y = e.d_y; a.gw = e.d_gw; a.n = e.n;
    a.X = (const T*)(dense ? e.mh.w.get() : X);
    a.mu = dense ? nullptr : e.d_mu;
    a.sw = dense ? nullptr : e.d_sw;
    a.nx = e.p;
    a.xi = (const T*)e.mh.xi.get(); a.gq = (const T*)e.mh.lin_gp.get();
    a.r = (const T*)(e.mh.ad_armed ? e.mh.lin_r.get() : e.mh.lin_z.get());
    a.Q = (const T*)X; a.U = (T*)U; a.gU = (T*)e.mh.lin_g.get(); a.p = e.p;
    a.J = e.J; a.c = mh_chains(e, false, logu, step);
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    // (xi, r, g, g_Q and w are the engine's own blocks: aligned)
    const bool vec = e.J % V == 0 && al16(a.G) && al16(a.X) && al16(a.Q) && al16(a.U);
    const dim3 grid((unsigned)((e.J + BN - 1) / BN)), block(HL_THREADS);
    if (e.mh.ad_armed) {
        a.e = e.mh.ad_state.get(); a.alpha = e.mh.ad_alpha.get();
        if (vec) hipLaunchKernelGGL((hl_accept_kernel<T, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hl_accept_kernel<T, false, true>), grid, block, 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((hl_accept_kernel<T, true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hl_accept_kernel<T, false, false>), grid, block, 0, s, a);
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_hl_accept(Engine& e, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? hl_accept_t<float>(e, X, G, U, logu, step, s) : hl_accept_t<double>(e, X, G, U, logu, step, s);
}

}  // namespace cesx
