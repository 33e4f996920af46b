// Metropolis-Hastings over the columns of the (p, J) layout: the score and the accept step of MCMC.model_mh
// (ces/sample.py:121-196), one independent chain per column.  The proposal P = a U + b S xi is an update launch
// (engine.hip, cesx_mh_propose); this file holds what follows the forward map:
//
//     phi(x) = 1/2 sum_i gw_i (g_i - y_i)^2  +  1/2 sum_r sw_r (x_r - mu_r)^2                  (:141-152 / :170-180)
//     accept  log u < phi(U) - phi(P)   ->   U := P, phi := phi(P), counter + 1                (:188-191)
//
// The test itself, with the uniform of the chain, is mh_test (cesx_internal.h), which gp_score_kernel shares.
//
// (the prior rows: the state itself with mu, 1 / Sigma_rr for a diagonal Sigma; w = L_Sigma^{-1} (x - mu) with unit
// weights for a dense one; none for pCN.)  V chains per lane (one 16-byte load: 4 floats / 2 doubles; a wave reads 1 KiB
// of a row per instruction) and the rows of a column split over the MH_NW waves of a workgroup (row r to wave r % MH_NW),
// so that J = 65 536 keeps 16 waves per CU in flight instead of one wave per SIMD.  Every sum runs in fp64 in a fixed
// order -- each wave its rows in increasing order, then the waves' partials through LDS in wave order -- so that runs are
// bit-reproducible.  Bound: HBM (G and the prior rows once, P again and U for the accepted columns).
#include "cesx_internal.h"

namespace cesx {

constexpr int MH_NW = 16;                 // waves per workgroup
constexpr int MH_THREADS = MH_NW * 64;

template <typename T> struct MhVec;
template <> struct MhVec<float> { static constexpr int V = 4; };
template <> struct MhVec<double> { static constexpr int V = 2; };

template <typename T>
struct MhArgs {
    const T* G; const double* y; const double* gw; int n;      // data rows
    const T* X; const double* mu; const double* sw; int nx;    // prior rows (mu / sw nullptr: 0 / 1; nx = 0: no prior term)
    const T* P; T* U; int p;                                   // accept: accepted columns of P copied into U
    long long J;
    MhChains c;                                                // (last: the tail it shares with GpScoreArgs)
};

// V consecutive values of one row from column j0 on, in fp64 (VEC: j0 + V <= J and 16-byte aligned)
template <typename T, bool VEC>
__device__ __forceinline__ void mh_load(const T* __restrict__ row, long long j0, long long J, double out[]) {
    constexpr int V = MhVec<T>::V;
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
__global__ __launch_bounds__(MH_THREADS)
void mh_accept_kernel(const MhArgs<T> a) {
    constexpr int V = MhVec<T>::V;
    constexpr int BN = 64 * V;                 // chains per workgroup
    __shared__ double part[MH_NW][BN];
    __shared__ int take[BN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long j0 = (long long)blockIdx.x * BN + (long long)lane * V;
    const bool vec = VEC && j0 + V <= a.J;
    double s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.0;
    if (j0 < a.J) {
#pragma unroll 4
        for (int i = wave; i < a.n; i += MH_NW) {
            double g[V];
            if (vec) mh_load<T, true>(a.G + (size_t)i * a.J, j0, a.J, g);
            else mh_load<T, false>(a.G + (size_t)i * a.J, j0, a.J, g);
            const double yi = a.y[i], wi = a.gw[i];
#pragma unroll
            for (int e = 0; e < V; ++e) { const double d = g[e] - yi; s[e] += wi * (d * d); }
        }
#pragma unroll 4
        for (int r = wave; r < a.nx; r += MH_NW) {
            double x[V];
            if (vec) mh_load<T, true>(a.X + (size_t)r * a.J, j0, a.J, x);
            else mh_load<T, false>(a.X + (size_t)r * a.J, j0, a.J, x);
            const double m = a.mu ? a.mu[r] : 0.0, wr = a.sw ? a.sw[r] : 1.0;
#pragma unroll
            for (int e = 0; e < V; ++e) { const double d = x[e] - m; s[e] += wr * (d * d); }
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) part[wave][lane * V + e] = s[e];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const long long j = j0 + e;
            int acc = 0;
            if (j < a.J) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < MH_NW; ++w) t += part[w][lane * V + e];
                acc = mh_test(a.c, j, 0.5 * t);
            }
            take[lane * V + e] = acc;
        }
    }
    if (a.c.start) return;
    __syncthreads();
    // the accepted columns: U := P (every wave its rows)
    int tk[V];
    bool any = false, all = true;
#pragma unroll
    for (int e = 0; e < V; ++e) { tk[e] = take[lane * V + e]; any = any || tk[e]; all = all && tk[e]; }
    if (!any) return;
    typedef T vt __attribute__((ext_vector_type(V)));
    for (int r = wave; r < a.p; r += MH_NW) {
        const T* src = a.P + (size_t)r * a.J + j0;
        T* dst = a.U + (size_t)r * a.J + j0;
        if (vec && all) {
            *reinterpret_cast<vt*>(dst) = *reinterpret_cast<const vt*>(src);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (tk[e]) dst[e] = src[e];          // (tk[e] != 0 only for j0 + e < J)
        }
    }
}

template <typename T>
static int mh_score_t(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step,
                      hipStream_t s) {
    constexpr int V = MhVec<T>::V, BN = 64 * V;
    const bool rw = e.mh.kind == CESX_MH_RW;
    MhArgs<T> a{};
    a.G = (const T*)G; a.y = e.d_y; a.gw = e.d_gw; a.n = e.n;
    a.X = (const T*)(e.mh.dense_prior ? e.mh.w.get() : X);
    a.mu = rw && !e.mh.dense_prior ? e.d_mu : nullptr;
    a.sw = rw && !e.mh.dense_prior ? e.d_sw : nullptr;
    a.nx = rw ? e.p : 0;
    a.P = (const T*)X; a.U = (T*)U; a.p = e.p;
    a.J = e.J; a.c = mh_chains(e, start, logu, step);
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    const bool vec = e.J % V == 0 && al16(a.G) && al16(a.X) && (start || (al16(a.P) && al16(a.U)));
    const dim3 grid((unsigned)((e.J + BN - 1) / BN));
    if (vec) hipLaunchKernelGGL((mh_accept_kernel<T, true>), grid, dim3(MH_THREADS), 0, s, a);
    else hipLaunchKernelGGL((mh_accept_kernel<T, false>), grid, dim3(MH_THREADS), 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_mh_score(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? mh_score_t<float>(e, start, X, G, U, logu, step, s)
                                   : mh_score_t<double>(e, start, X, G, U, logu, step, s);
}

}  // namespace cesx
