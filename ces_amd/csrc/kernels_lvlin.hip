// The Metropolis-adjusted Langevin step of MCMC.model_mh(chains=M, update='langevin') for the LINEAR maps (lineal: G = A X + b;
// lineal_log: G = A exp(X) + b) at any p: the vector-Jacobian product DG^T r is a GEMM, so the step needs no [n][p][J]
// Jacobian image and no chain-per-lane triangular loops (kernels_gpgrad.hip: right for p = 2, hopeless for p = 256).
//
//     g = S^T grad phi,   grad phi = t + Sigma^{-1} (X - mu),   t = A^T Gamma^{-1} (G - y)   [lineal_log: exp(X) (.) t]
//
// The products are update launches (launch_update: one descriptor, one picker) over images the engine forms on the host in
// fp64 at cesx_mh_langevin_lineal_set (engine.hip):
//     lineal       ONE launch      g  = [S^T A^T M | S^T Sigma^{-1}] . [G~ ; X] + bias
//     lineal_log   two launches    t0 = (A^T M) . G~ - A^T M y~;   h = exp(X) (.) t0 (lvlin_exph_kernel);
//                                  g  = [S^T | S^T Sigma^{-1}] . [h ; X] + bias
// with G~ the data rows the score kernel reads (G, or the whitened copy L_Gamma^{-1} G of a dense Gamma) and M = Gamma^{-1} /
// L_Gamma^{-T} accordingly, so the product is A^T Gamma^{-1} (G - y) either way.  This file holds what is not a GEMM:
//
//     lvlin_exph_kernel     h = exp(X) (.) t0, in place over t0
//     lvlin_z_kernel        z = xi - g / 2; the proposal P = U + S z is then the triangular update launch of cesx_mh_propose
//     lvlin_accept_kernel   phi(P), the test with the Langevin correction, and the masked copies P -> U and g(P) -> g(U)
//
// lvlin_accept_kernel is mh_accept_kernel (kernels_mh.hip) with two more sums: V chains per lane through 16-byte loads, the
// rows of a column split over the 16 waves of a workgroup (row r to wave r % 16), every sum in fp64 in a fixed order -- each
// wave its rows in increasing order, then the waves' partials through LDS in wave order.  The data and prior sums are
// mh_accept_kernel's in its order, so phi equals cesx_mh_start's bit for bit.  No atomics; NaN anywhere rejects (the test is
// a `<`).  Bound: HBM (G, the prior rows, xi, g(U), g(P) once; P and g(P) again, U and g(U) written, for the accepted columns).
#include "cesx_internal.h"

namespace cesx {

constexpr int LL_NW = 16;                 // waves per workgroup (MH_NW of kernels_mh.hip)
constexpr int LL_THREADS = LL_NW * 64;
constexpr int LL_EW_THREADS = 256;        // the element-wise kernels

template <typename T> struct LlVec;
template <> struct LlVec<float> { static constexpr int V = 4; };
template <> struct LlVec<double> { static constexpr int V = 2; };

template <typename T>
struct LvlinArgs {
    const T* G; const double* y; const double* gw; int n;      // data rows (whitened for a dense Gamma)
    const T* X; const double* mu; const double* sw; int nx;    // prior rows: the states with mu, 1 / Sigma_rr, or w with nullptr, nullptr
    const T* xi; const T* gu; const T* gp;                     // the step's noise block, g of the chains' states and of the proposals
    const T* P; T* U; T* gU; int p;                            // accept: accepted columns of P into U and of gp into gU
    long long J;
    MhChains c;
};

// V consecutive values of one row from column j0 on, in fp64 (VEC: j0 + V <= J and 16-byte aligned)
template <typename T, bool VEC>
__device__ __forceinline__ void ll_load(const T* __restrict__ row, long long j0, long long J, double out[]) {
    constexpr int V = LlVec<T>::V;
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

template <typename T, bool VEC>
__global__ __launch_bounds__(LL_THREADS)
void lvlin_accept_kernel(const LvlinArgs<T> a) {
    constexpr int V = LlVec<T>::V;
    constexpr int BN = 64 * V;                 // chains per workgroup
    __shared__ double part[LL_NW][BN];         // one sum at a time: phi's, then |xi|^2, then |xi - (g_U + g_P) / 2|^2
    __shared__ int take[BN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long j0 = (long long)blockIdx.x * BN + (long long)lane * V;
    const bool vec = VEC && j0 + V <= a.J;
    const bool corr = !a.c.start;
    double s[V], n1[V], n2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s[e] = 0.0; n1[e] = 0.0; n2[e] = 0.0; }
    if (j0 < a.J) {
#pragma unroll 4
        for (int i = wave; i < a.n; i += LL_NW) {
            double g[V];
            if (vec) ll_load<T, true>(a.G + (size_t)i * a.J, j0, a.J, g);
            else ll_load<T, false>(a.G + (size_t)i * a.J, j0, a.J, g);
            const double yi = a.y[i], wi = a.gw[i];
#pragma unroll
            for (int e = 0; e < V; ++e) { const double d = g[e] - yi; s[e] += wi * (d * d); }
        }
#pragma unroll 4
        for (int r = wave; r < a.nx; r += LL_NW) {
            double x[V];
            if (vec) ll_load<T, true>(a.X + (size_t)r * a.J, j0, a.J, x);
            else ll_load<T, false>(a.X + (size_t)r * a.J, j0, a.J, x);
            const double m = a.mu ? a.mu[r] : 0.0, wr = a.sw ? a.sw[r] : 1.0;
#pragma unroll
            for (int e = 0; e < V; ++e) { const double d = x[e] - m; s[e] += wr * (d * d); }
        }
        if (corr) {
#pragma unroll 2
            for (int r = wave; r < a.p; r += LL_NW) {
                double x[V], gu[V], gp[V];
                const size_t o = (size_t)r * a.J;
                if (vec) { ll_load<T, true>(a.xi + o, j0, a.J, x); ll_load<T, true>(a.gu + o, j0, a.J, gu); ll_load<T, true>(a.gp + o, j0, a.J, gp); }
                else { ll_load<T, false>(a.xi + o, j0, a.J, x); ll_load<T, false>(a.gu + o, j0, a.J, gu); ll_load<T, false>(a.gp + o, j0, a.J, gp); }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const double d = x[e] - 0.5 * (gu[e] + gp[e]);
                    n1[e] = fma(x[e], x[e], n1[e]);
                    n2[e] = fma(d, d, n2[e]);
                }
            }
        }
    }
    // the waves' partials in wave order, one sum at a time through the one LDS block; thread c < BN sums chain c of the workgroup
    const int tid = threadIdx.x;
    double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (q > 0 && !corr) continue;
        if (q > 0) __syncthreads();
#pragma unroll
        for (int e = 0; e < V; ++e) part[wave][lane * V + e] = q == 0 ? s[e] : q == 1 ? n1[e] : n2[e];
        __syncthreads();
        if (tid < BN) {
            double acc = 0.0;
#pragma unroll
            for (int w = 0; w < LL_NW; ++w) acc += part[w][tid];
            t[q] = acc;
        }
    }
    if (tid < BN) {
        const long long j = (long long)blockIdx.x * BN + tid;
        int acc = 0;
        if (j < a.J) {
            const double ph = 0.5 * t[0];
            if (a.c.start) {
                a.c.phi[j] = ph;
                a.c.cnt[j] = 0ull;
            } else {
                const double lu = a.c.logu ? a.c.logu[j]
                                           : mh_log_uniform((unsigned long long)(a.c.j_offset + j), a.c.step, a.c.seed_lo, a.c.seed_hi);
                if (lu < a.c.phi[j] - ph + (0.5 * t[1] - 0.5 * t[2])) {
                    a.c.phi[j] = ph;
                    a.c.cnt[j] += 1ull;
                    acc = 1;
                }
            }
        }
        take[tid] = acc;
    }
    if (a.c.start) return;
    __syncthreads();
    // the accepted columns: U := P and g(U) := g(P) (every wave its rows)
    int tk[V];
    bool any = false, all = true;
#pragma unroll
    for (int e = 0; e < V; ++e) { tk[e] = take[lane * V + e]; any = any || tk[e]; all = all && tk[e]; }
    if (!any) return;
    typedef T vt __attribute__((ext_vector_type(V)));
    for (int r = wave; r < a.p; r += LL_NW) {
        const size_t o = (size_t)r * a.J + j0;
        if (vec && all) {
            *reinterpret_cast<vt*>(a.U + o) = *reinterpret_cast<const vt*>(a.P + o);
            *reinterpret_cast<vt*>(a.gU + o) = *reinterpret_cast<const vt*>(a.gp + o);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (tk[e]) { a.U[o + e] = a.P[o + e]; a.gU[o + e] = a.gp[o + e]; }      // (tk[e] != 0 only for j0 + e < J)
        }
    }
}

// z = xi - g / 2 over the len = p J elements of the engine's own blocks (16-byte aligned: whole vectors, then the tail)
template <typename T>
__global__ __launch_bounds__(LL_EW_THREADS)
void lvlin_z_kernel(const T* __restrict__ xi, const T* __restrict__ g, T* __restrict__ z, size_t len) {
    constexpr int V = LlVec<T>::V;
    typedef T vt __attribute__((ext_vector_type(V)));
    const size_t nv = len / V, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        const vt x = reinterpret_cast<const vt*>(xi)[i], q = reinterpret_cast<const vt*>(g)[i];
        vt o;
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = x[e] - (T)0.5 * q[e];
        reinterpret_cast<vt*>(z)[i] = o;
    }
    const size_t k = nv * V + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < len) z[k] = xi[k] - (T)0.5 * g[k];
}

__device__ __forceinline__ float ll_exp(float x) { return expf(x); }
__device__ __forceinline__ double ll_exp(double x) { return exp(x); }

// h = exp(X) (.) t0 in place over t0 (the engine's block); X is the caller's: vectors only when `vec` says it is 16-byte aligned
template <typename T>
__global__ __launch_bounds__(LL_EW_THREADS)
void lvlin_exph_kernel(const T* __restrict__ X, T* __restrict__ t0, size_t len, int vec) {
    constexpr int V = LlVec<T>::V;
    typedef T vt __attribute__((ext_vector_type(V)));
    const size_t nv = vec ? len / V : 0, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        const vt x = reinterpret_cast<const vt*>(X)[i];
        vt o = reinterpret_cast<vt*>(t0)[i];
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = ll_exp(x[e]) * o[e];
        reinterpret_cast<vt*>(t0)[i] = o;
    }
    for (size_t k = nv * V + (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < len; k += stride) t0[k] = ll_exp(X[k]) * t0[k];
}

static unsigned ll_ew_grid(const Engine& e, size_t len) {
    const size_t want = (len + LL_EW_THREADS - 1) / LL_EW_THREADS;
    const size_t cap = (size_t)e.num_cus * 16;
    return (unsigned)std::max<size_t>(1, std::min(want, cap));
}

template <typename T>
static int lvlin_z_t(Engine& e, hipStream_t s) {
    const size_t len = (size_t)e.p * (size_t)e.J;
    constexpr int V = LlVec<T>::V;
    const size_t work = len / V + V;          // (whole vectors; the tail of fewer than V elements rides in the first threads)
    hipLaunchKernelGGL((lvlin_z_kernel<T>), dim3(ll_ew_grid(e, work)), dim3(LL_EW_THREADS), 0, s, (const T*)e.mh.xi.get(),
                       (const T*)e.mh.lin_g.get(), (T*)e.mh.lin_z.get(), len);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_lvlin_z(Engine& e, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? lvlin_z_t<float>(e, s) : lvlin_z_t<double>(e, s);
}

template <typename T>
static int lvlin_exph_t(Engine& e, const void* X, void* t0, hipStream_t s) {
    const size_t len = (size_t)e.p * (size_t)e.J;
    const int vec = ((uintptr_t)X & 15) == 0 && ((uintptr_t)t0 & 15) == 0;
    hipLaunchKernelGGL((lvlin_exph_kernel<T>), dim3(ll_ew_grid(e, len / (vec ? LlVec<T>::V : 1) + LL_EW_THREADS)), dim3(LL_EW_THREADS), 0, s,
                       (const T*)X, (T*)t0, len, vec);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_lvlin_exph(Engine& e, const void* X, void* t0, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? lvlin_exph_t<float>(e, X, t0, s) : lvlin_exph_t<double>(e, X, t0, s);
}

template <typename T>
static int lvlin_score_t(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    constexpr int V = LlVec<T>::V, BN = 64 * V;
    const bool dense = !e.diag_sigma;
    LvlinArgs<T> a{};
    a.G = (const T*)G; a.y = e.d_y; a.gw = e.d_gw; a.n = e.n;
    a.X = (const T*)(dense ? e.mh.w.get() : X);
    a.mu = dense ? nullptr : e.d_mu;
    a.sw = dense ? nullptr : e.d_sw;
    a.nx = e.p;
    a.xi = (const T*)e.mh.xi.get(); a.gu = (const T*)e.mh.lin_g.get(); a.gp = (const T*)e.mh.lin_gp.get();
    a.P = (const T*)X; a.U = (T*)U; a.gU = (T*)e.mh.lin_g.get(); a.p = e.p;
    a.J = e.J; a.c = mh_chains(e, start, logu, step);
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    // (xi, g, g_P and w are the engine's own blocks: aligned)
    const bool vec = e.J % V == 0 && al16(a.G) && al16(a.X) && (start || (al16(a.P) && al16(a.U)));
    const dim3 grid((unsigned)((e.J + BN - 1) / BN));
    if (vec) hipLaunchKernelGGL((lvlin_accept_kernel<T, true>), grid, dim3(LL_THREADS), 0, s, a);
    else hipLaunchKernelGGL((lvlin_accept_kernel<T, false>), grid, dim3(LL_THREADS), 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_lvlin_score(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? lvlin_score_t<float>(e, start, X, G, U, logu, step, s)
                                   : lvlin_score_t<double>(e, start, X, G, U, logu, step, s);
}

}  // namespace cesx
