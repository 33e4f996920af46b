// The dense per-chain likelihood of MCMC.gp_mh with pca_tools (ces/sample.py:52-53, :91-92; ces/emulate.py:74-77): k GPs
// on PCA-decorrelated outputs, the data space rebuilt per state as
//     d     = B m + g0 - y                       (B = VD_k [n][k], m the k GP means, g0 = mG)
//     Sigma = Gamma + B diag(v) B^T              (v the k GP variances; Gamma and y UNWHITENED)
//     phi   = 1/2 d^T Sigma^{-1} d [+ 1/2 log det Sigma] + the prior term of gp_score_kernel
// followed by the test (mh_test, cesx_internal.h) and the copy U := P of an accepted column.  Sigma changes with every
// state of every chain: one n x n Cholesky factorisation per chain and step.  All arithmetic fp64 whatever the engine dtype.
//
// gp_score_dense_kernel: one chain per wave, one wave per workgroup.  The factor lives in LDS, its lower triangle packed
// by columns -- element (i, c), i >= c, at c n - c (c - 1) / 2 + (i - c) -- and row i belongs to lane i % 64 (slot i / 64,
// n <= 128: two slots), so that the lanes of a wave read and write consecutive addresses of one column.  Left-looking:
// column c of Sigma is formed in registers right before it is factored (the unfactored matrix is never stored),
//     s_i = Gamma_ic + sum_t Bt[t][i] (v_t B[c][t])  -  sum_{c' < c} L_ic' L_cc'          (t and c' in increasing order)
// the pivot s_c goes to every lane (one shuffle), L_cc = sqrt(s_c), L_ic = s_i / L_cc, the column is written once.  The
// forward substitution rides along: z_c = d_c / L_cc, d_i -= L_ic z_c from the registers that hold the column, and
// z_c^2 and log L_cc are summed in column order in every lane -- no reduction, no atomics, one fixed order: two calls are
// bit-identical and a chain's phi does not depend on M, on its column or on its neighbours.  B is read in both layouts
// from L2 (shared by all chains): Bt [k][n] for the lanes' rows, B [n][k] for the wave-uniform row c.
// A pivot that is not > 0 or not finite makes phi NaN: the test rejects, a start state stays stuck (what the variance
// modes of gp_score_kernel do with a non-positive variance).  No trap, no assert.
// The wave's LDS accesses execute in program order; the barrier after a column (one wave: no wait) is there for the
// compiler, which must not move the next column's reads of L above the lanes' stores.
// LDS: (n (n + 1) / 2 + 2 k) doubles -- 66 KiB + 2 KiB at n = k = 128, two workgroups per CU; 10 KiB at n = 50.
#include "cesx_internal.h"

namespace cesx {

constexpr int GPD_THREADS = 64;

template <typename T>
struct GpDenseArgs {
    const double *mean, *var; int n, k; long long M;      // the GP rows (k x M)
    const double *B, *Bt, *g0;                            // [n][k], [k][n], [n]
    const double *y, *Gam;                                // unwhitened: [n], [n][n] symmetric
    int logdet;
    const T* X; const double *mu, *sw, *LSi; int p;       // prior: diagonal (sw) or dense (LSi = L_Sigma^{-1})
    T* U;
    MhChains c;
};

size_t gp_dense_lds(int n, int k) { return ((size_t)n * (n + 1) / 2 + 2 * (size_t)k) * 8; }

template <typename T>
__global__ __launch_bounds__(GPD_THREADS)
void gp_score_dense_kernel(const GpDenseArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double gpd_smem[];
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;
    const int n = a.n, k = a.k, p = a.p;
    double* Lp = gpd_smem;                                // the packed factor
    double* vv = Lp + n * (n + 1) / 2;                    // [k] the chain's variances
    double* mm = vv + k;                                  // [k] the chain's means
    for (int t = lane; t < k; t += GPD_THREADS) {
        vv[t] = a.var[(size_t)t * a.M + j];
        mm[t] = a.mean[(size_t)t * a.M + j];
    }
    __syncthreads();
    const int i0 = lane, i1 = lane + GPD_THREADS;         // this lane's rows
    const bool in0 = i0 < n, in1 = i1 < n;
    double d0 = 0.0, d1 = 0.0;
    for (int t = 0; t < k; ++t) {
        const double m = mm[t];
        if (in0) d0 = fma(a.Bt[(size_t)t * n + i0], m, d0);
        if (in1) d1 = fma(a.Bt[(size_t)t * n + i1], m, d1);
    }
    if (in0) d0 = d0 + a.g0[i0] - a.y[i0];
    if (in1) d1 = d1 + a.g0[i1] - a.y[i1];
    double q = 0.0, ld = 0.0;
    bool bad = false;
    for (int c = 0; c < n; ++c) {
        const bool on0 = in0 && i0 >= c, on1 = in1 && i1 >= c;
        const double* Bc = a.B + (size_t)c * k;
        double s0 = 0.0, s1 = 0.0;
        for (int t = 0; t < k; ++t) {
            const double w = vv[t] * Bc[t];
            if (on0) s0 = fma(a.Bt[(size_t)t * n + i0], w, s0);
            if (on1) s1 = fma(a.Bt[(size_t)t * n + i1], w, s1);
        }
        if (on0) s0 = a.Gam[(size_t)c * n + i0] + s0;
        if (on1) s1 = a.Gam[(size_t)c * n + i1] + s1;
        int base = 0;                                     // element (i, c') at Lp[base + i]
        for (int cc = 0; cc < c; ++cc) {
            const double lc = Lp[base + c];               // L[c][c']: one address, broadcast
            if (on0) s0 = fma(-Lp[base + i0], lc, s0);
            if (on1) s1 = fma(-Lp[base + i1], lc, s1);
            base += n - cc - 1;
        }
        // (c is wave-uniform: the slot is picked before the shuffle)
        const double piv = __shfl(c < GPD_THREADS ? s0 : s1, c & (GPD_THREADS - 1), GPD_THREADS);
        const double dc = __shfl(c < GPD_THREADS ? d0 : d1, c & (GPD_THREADS - 1), GPD_THREADS);
        if (!(piv > 0.0 && piv < __builtin_inf())) bad = true;
        const double l = sqrt(piv);
        const double x0 = i0 == c ? l : s0 / l, x1 = i1 == c ? l : s1 / l;
        if (on0) Lp[base + i0] = x0;
        if (on1) Lp[base + i1] = x1;
        const double zc = dc / l;
        q = fma(zc, zc, q);
        if (a.logdet) ld += log(l);
        if (in0 && i0 > c) d0 = fma(-x0, zc, d0);
        if (in1 && i1 > c) d1 = fma(-x1, zc, d1);
        __syncthreads();
    }
    // the prior term: gp_score_kernel's sums (every lane the same values)
    double s = 0.0;
    if (a.LSi) {
        for (int r = 0; r < p; ++r) {
            double w = 0.0;
            for (int t = 0; t <= r; ++t) w = fma(a.LSi[(size_t)r * p + t], (double)a.X[(size_t)t * a.M + j] - a.mu[t], w);
            s = fma(w, w, s);
        }
    } else {
        for (int r = 0; r < p; ++r) { const double d = (double)a.X[(size_t)r * a.M + j] - a.mu[r]; s = fma(a.sw[r], d * d, s); }
    }
    double ph = 0.5 * q + ld + 0.5 * s;
    if (bad) ph = __longlong_as_double(0x7ff8000000000000ll);
    int take = 0;
    if (lane == 0) take = mh_test(a.c, j, ph) ? 1 : 0;
    take = __shfl(take, 0, GPD_THREADS);
    if (take)
        for (int r = lane; r < p; r += GPD_THREADS) a.U[(size_t)r * a.M + j] = a.X[(size_t)r * a.M + j];
}

// once per installed descriptor (cesx_gp_dense_set): both instantiations may take the dynamic LDS of this shape
int gp_dense_prepare(Engine& e, int n, int k) {
    const int lds = (int)gp_dense_lds(n, k);
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gp_score_dense_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gp_score_dense_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return CESX_OK;
}

template <typename T>
static int gp_score_dense_t(Engine& e, bool start, const void* X, const double* mean, const double* var, void* U,
                            const double* logu, unsigned step, hipStream_t s) {
    GpDenseArgs<T> a{};
    a.mean = mean; a.var = var; a.n = e.n; a.k = e.gpd.k; a.M = e.J;
    a.B = e.gpd.B; a.Bt = e.gpd.Bt; a.g0 = e.gpd.g0; a.y = e.gpd.y; a.Gam = e.gpd.Gam;
    a.logdet = e.gpd.logdet;
    a.X = (const T*)X; a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get(); a.p = e.p;
    a.U = (T*)U; a.c = mh_chains(e, start, logu, step);
    if (e.J >= (1LL << 31)) { e.err = "cesx_gp: too many chains for one dense launch"; return CESX_EUNSUPPORTED; }
    hipLaunchKernelGGL((gp_score_dense_kernel<T>), dim3((unsigned)e.J), dim3(GPD_THREADS), gp_dense_lds(e.n, e.gpd.k), s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_gp_score_dense(Engine& e, bool start, const void* X, const double* mean, const double* var, void* U,
                          const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? gp_score_dense_t<float>(e, start, X, mean, var, U, logu, step, s)
                                   : gp_score_dense_t<double>(e, start, X, mean, var, U, logu, step, s);
}

}  // namespace cesx
