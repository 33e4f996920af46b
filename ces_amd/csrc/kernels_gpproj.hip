// The per-chain likelihood of MCMC.gp_mh with pca_tools, Sigma projected to k x k (CESX_GP_PROJ; include/cesx.h has the
// algebra, ces_amd.emulate.project_sigma the host reduction).  Per chain j, from the k GP means m and variances v:
//     a   = a0 + R m                              (R k x k upper triangular)
//     A   = I_k + R diag(v) R^T                   (symmetric, eigenvalues >= 1 for v >= 0)
//     phi = 1/2 (c_perp + a^T A^{-1} a) [+ half_logdet_gamma + 1/2 log det A] + the prior term of gp_score_kernel
// followed by the test (mh_test, cesx_internal.h) and the copy U := P of an accepted column.  n_obs does not appear: what
// depends on the chain is k-dimensional.  All arithmetic fp64 whatever the engine dtype.
//
// gp_score_proj_kernel<T, G, SLOTS>: one wave per workgroup, 64 / G chains per wave.  A chain belongs to a group of G
// consecutive lanes, G the smallest of 16, 32, 64 that is >= k; for 64 < k <= 128 one chain has the wave and every lane two
// rows (SLOTS = 2), as in gp_score_dense_kernel.  Row i belongs to group lane i % G (slot i / G).  Each group has its own
// slice of the dynamic LDS: the factor's lower triangle packed by columns -- element (i, c), i >= c, at
// c k - c (c - 1) / 2 + (i - c) -- then the chain's k variances and k means.  Left-looking: column c of A is formed in
// registers right before it is factored (A is never stored),
//     s_i = [i == c] + sum_{t >= c} Rt[t][i] (v_t R[c][t])  -  sum_{c' < c} L_ic' L_cc'      (t and c' in increasing order)
// (R[c][t] = 0 for t < c: the sum starts at c for every lane; Rt[t][i] = R[i][t] is stored with its zeros, t < i, and a
// zero times a finite number adds nothing: one order whatever the row).  The pivot s_c goes to the group's lanes (one
// shuffle of width G), L_cc = sqrt(s_c), L_ic = s_i / L_cc, the column is written once.  The forward substitution rides
// along: z_c = a_c / L_cc, a_i -= L_ic z_c from the registers that hold the column; q = c_perp + sum z_c^2 and
// half_logdet_gamma + sum log L_cc are summed in column order in every lane -- no reduction, no atomics, one fixed order:
// two calls are bit-identical and a chain's phi does not depend on M, on its column, on its group or on its neighbours
// (nothing crosses a group: the shuffles have width G, the LDS slices are disjoint).  R and Rt are read from L2 (shared by
// all chains); c and t are wave-uniform, so R[c][t] is one address for the wave.
// A pivot that is not > 0 or not finite makes phi NaN: the test rejects, a start state stays stuck.  No trap, no assert.
// The ragged last wave: a group past the last chain loads nothing from the chains' arrays and stores nothing; it factors
// I_k (v = 0, m = 0) and reaches every barrier.
// The wave's LDS accesses execute in program order; the barrier after a column (one wave: no wait) is there for the
// compiler, which must not move the next column's reads of L above the lanes' stores.
// LDS: (64 / G) (k (k + 1) / 2 + 2 k) doubles -- 5.3 KiB at k = 16, 17.3 KiB at k = 64, 66.5 KiB at k = 128.
#include "cesx_internal.h"

namespace cesx {

constexpr int GPP_THREADS = 64;

template <typename T>
struct GpProjArgs {
    const double *mean, *var; int k; long long M;         // the GP rows (k x M)
    const double *R, *Rt, *a0;                            // [k][k] zero below the diagonal, its transpose, [k]
    double c_perp, hld; int logdet;
    const T* X; const double *mu, *sw, *LSi; int p;       // prior: diagonal (sw) or dense (LSi = L_Sigma^{-1})
    T* U;
    MhChains c;
};

int gp_proj_group(int k) { return k <= 16 ? 16 : k <= 32 ? 32 : 64; }
size_t gp_proj_lds(int k) {
    return (size_t)(GPP_THREADS / gp_proj_group(k)) * ((size_t)k * (k + 1) / 2 + 2 * (size_t)k) * 8;
}

template <typename T, int G, int SLOTS>
__global__ __launch_bounds__(GPP_THREADS)
void gp_score_proj_kernel(const GpProjArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double gpp_smem[];
    constexpr int CH = GPP_THREADS / G;                   // chains per wave
    const int lane = threadIdx.x, g = lane / G, gl = lane % G;
    const long long j = (long long)blockIdx.x * CH + g;
    const bool live = j < a.M;
    const int k = a.k, p = a.p;
    double* Lp = gpp_smem + (size_t)g * (k * (k + 1) / 2 + 2 * k);      // this group's packed factor
    double* vv = Lp + k * (k + 1) / 2;                    // [k] the chain's variances
    double* mm = vv + k;                                  // [k] the chain's means
    for (int t = gl; t < k; t += G) {
        vv[t] = live ? a.var[(size_t)t * a.M + j] : 0.0;
        mm[t] = live ? a.mean[(size_t)t * a.M + j] : 0.0;
    }
    __syncthreads();
    const int i0 = gl, i1 = gl + G;                       // this lane's rows
    const bool in0 = i0 < k, in1 = SLOTS == 2 && i1 < k;
    double d0 = 0.0, d1 = 0.0;
    for (int t = 0; t < k; ++t) {
        const double m = mm[t];
        if (in0) d0 = fma(a.Rt[(size_t)t * k + i0], m, d0);
        if (SLOTS == 2) { if (in1) d1 = fma(a.Rt[(size_t)t * k + i1], m, d1); }
    }
    if (in0) d0 = d0 + a.a0[i0];
    if (SLOTS == 2) { if (in1) d1 = d1 + a.a0[i1]; }
    double q = a.c_perp, ld = a.logdet ? a.hld : 0.0;
    bool bad = false;
    int base = 0;                                         // element (i, c) at Lp[base + i]
    for (int c = 0; c < k; ++c) {
        const bool on0 = in0 && i0 >= c, on1 = in1 && i1 >= c;
        const double* Rc = a.R + (size_t)c * k;
        double s0 = 0.0, s1 = 0.0;
        for (int t = c; t < k; ++t) {
            const double w = vv[t] * Rc[t];
            if (on0) s0 = fma(a.Rt[(size_t)t * k + i0], w, s0);
            if (SLOTS == 2) { if (on1) s1 = fma(a.Rt[(size_t)t * k + i1], w, s1); }
        }
        if (i0 == c) s0 = 1.0 + s0;
        if (SLOTS == 2) { if (i1 == c) s1 = 1.0 + s1; }
        int bb = 0;                                       // element (i, c') at Lp[bb + i]
        for (int cc = 0; cc < c; ++cc) {
            const double lc = Lp[bb + c];                 // L[c][c']: one address per group, broadcast
            if (on0) s0 = fma(-Lp[bb + i0], lc, s0);
            if (SLOTS == 2) { if (on1) s1 = fma(-Lp[bb + i1], lc, s1); }
            bb += k - cc - 1;
        }
        // (c is wave-uniform: the slot is picked before the shuffle; the shuffle stays inside the group)
        const double piv = __shfl(SLOTS == 2 && c >= G ? s1 : s0, c & (G - 1), G);
        const double dc = __shfl(SLOTS == 2 && c >= G ? d1 : d0, c & (G - 1), G);
        if (!(piv > 0.0 && piv < __builtin_inf())) bad = true;
        const double l = sqrt(piv);
        const double x0 = i0 == c ? l : s0 / l, x1 = i1 == c ? l : s1 / l;
        if (on0) Lp[base + i0] = x0;
        if (SLOTS == 2) { if (on1) Lp[base + i1] = x1; }
        const double zc = dc / l;
        q = fma(zc, zc, q);
        if (a.logdet) ld += log(l);
        if (in0 && i0 > c) d0 = fma(-x0, zc, d0);
        if (SLOTS == 2) { if (in1 && i1 > c) d1 = fma(-x1, zc, d1); }
        base += k - c - 1;
        __syncthreads();
    }
    if (!live) return;                                    // (behind the last barrier)
    // the prior term: gp_score_kernel's sums (every lane of the group the same values)
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
    if (gl == 0) take = mh_test(a.c, j, ph) ? 1 : 0;
    take = __shfl(take, 0, G);
    if (take)
        for (int r = gl; r < p; r += G) a.U[(size_t)r * a.M + j] = a.X[(size_t)r * a.M + j];
}

// the instantiation for k: f(kernel, chains per wave)
template <typename T, typename F>
static int gp_proj_pick(int k, F f) {
    if (k <= 16) return f(gp_score_proj_kernel<T, 16, 1>, 4);
    if (k <= 32) return f(gp_score_proj_kernel<T, 32, 1>, 2);
    if (k <= 64) return f(gp_score_proj_kernel<T, 64, 1>, 1);
    return f(gp_score_proj_kernel<T, 64, 2>, 1);
}

// once per installed descriptor (cesx_gp_proj_set): both instantiations for this k may take its dynamic LDS
int gp_proj_prepare(Engine& e, int k) {
    const int lds = (int)gp_proj_lds(k);
    auto raise = [&](auto kern, int) -> int {
        CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        return CESX_OK;
    };
    if (const int rc = gp_proj_pick<float>(k, raise)) return rc;
    return gp_proj_pick<double>(k, raise);
}

template <typename T>
static int gp_score_proj_t(Engine& e, bool start, const void* X, const double* mean, const double* var, void* U,
                           const double* logu, unsigned step, hipStream_t s) {
    GpProjArgs<T> a{};
    a.mean = mean; a.var = var; a.k = e.gpp.k; a.M = e.J;
    a.R = e.gpp.R; a.Rt = e.gpp.Rt; a.a0 = e.gpp.a0;
    a.c_perp = e.gpp.c_perp; a.hld = e.gpp.half_logdet_gamma; a.logdet = e.gpp.logdet;
    a.X = (const T*)X; a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get(); a.p = e.p;
    a.U = (T*)U; a.c = mh_chains(e, start, logu, step);
    if (e.J >= (1LL << 31)) { e.err = "cesx_gp: too many chains for one projected launch"; return CESX_EUNSUPPORTED; }
    return gp_proj_pick<T>(a.k, [&](auto kern, int ch) -> int {
        hipLaunchKernelGGL(kern, dim3((unsigned)((e.J + ch - 1) / ch)), dim3(GPP_THREADS), gp_proj_lds(a.k), s, a);
        CESX_HIP(hipGetLastError());
        return CESX_OK;
    });
}

int launch_gp_score_proj(Engine& e, bool start, const void* X, const double* mean, const double* var, void* U,
                         const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? gp_score_proj_t<float>(e, start, X, mean, var, U, logu, step, s)
                                   : gp_score_proj_t<double>(e, start, X, mean, var, U, logu, step, s);
}

}  // namespace cesx
