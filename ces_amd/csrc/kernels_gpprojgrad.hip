// The gradient coefficients of the projected per-chain likelihood (CESX_GP_PROJ; kernels_gpproj.hip has the score, include/cesx.h
// the algebra): what MCMC.gp_mh(chains=M, pca_tools=, sigma_form='projected', update='langevin' / 'hmc') needs of Sigma_j before
// lv_score (lv_score.h) can form grad phi.  Per chain j, with a = a0 + R m, A = I_k + R diag(v) R^T = L L^T and z = L^{-1} a:
//     phi_data = 1/2 (c_perp + |z|^2) [+ half_logdet_gamma + sum log L_cc]          (gp_score_proj_kernel's 1/2 q + ld, its bits)
//     w   = L^{-T} z = A^{-1} a
//     e_t = (R^T w)_t                                      = d phi / d m_t
//     h_t = |L^{-1} R[:, t]|^2 = (R^T A^{-1} R)_tt
//     a_t = e_t,   b_t = 1/2 ([logdet] h_t - e_t^2)        = d phi / d v_t
// The h term belongs to the log det: without the flag it is absent from b (the gradient is the gradient of the phi that is
// scored), and the two phases that only it needs (4 and 5) are not run.
//
// gp_proj_coef_kernel<G, SLOTS>: placement, group width, row ownership and LDS slice of gp_score_proj_kernel -- one wave per
// workgroup, 64 / G chains per wave, G the smallest of 16, 32, 64 that is >= k, two row slots for 64 < k <= 128; the group's
// slice holds the packed factor (element (i, c), i >= c, at c k - c (c + 1) / 2 + i), the k variances and the k means:
// gp_proj_lds(k) bytes, nothing more.  Not templated on the engine dtype: only the fp64 GP rows are read (the prior term stays
// in lv_score).  Phases, every sum in one fixed order:
//     1. the factor and the forward substitution: gp_score_proj_kernel's statements; lane c keeps its own z_c
//     2. back substitution, c = k - 1 .. 0: w_c = z_c / L_cc to the group (one shuffle of width G), lanes i < c take
//        z_i -= L_ci w_c from their own column; w_c over the means' slice (the means are dead once a exists)
//     3. e_t = sum_i R[i][t] w_i in lane t (and t + G), i increasing; R read row-wise (the lanes' loads coalesce), its zeros
//        below the diagonal add nothing
//     4. L^{-1} =: X in place over L, columns right to left: row owner i forms sum_{s = j + 1 .. i} X_is L_sj (s increasing) from
//        its own row of the inverted trailing block and the original column j (one address per group), then X_ij = -(...) / L_jj,
//        X_jj = 1 / L_jj
//     5. h_t = sum_i (sum_{s <= i} X_is R[s][t])^2 in lane t (R[s][t] = 0 for s > t: the inner sum ends at min(i, t) by value);
//        no per-lane vector is kept
// No atomics, nothing crosses a group (shuffles of width G, disjoint LDS slices): two calls are bit-identical and a chain's
// outputs do not depend on M, on its column, on its group or on its neighbours.  A pivot that is not > 0 or not finite makes
// phi_data, a and b of that chain NaN; its wave-mates keep their bits.  The ragged last wave: a group past the last chain
// factors I_k, reaches every barrier and stores nothing.  The barriers (one wave: no wait) are there for the compiler, as in
// gp_score_proj_kernel.  By flop count about 4 x the score launch (factor k^3 / 6, inverse k^3 / 6, product k^3 / 3).
#include "cesx_internal.h"

namespace cesx {

constexpr int GPC_THREADS = 64;

struct GpProjCoefArgs {
    const double *mean, *var; int k; long long M;         // the GP rows (k x M)
    const double *R, *Rt, *a0;                            // the descriptor's images (kernels_gpproj.hip)
    double c_perp, hld; int logdet;
    double *phid, *ca, *cb;                               // [M], [k][M], [k][M]
};

template <int G, int SLOTS>
__global__ __launch_bounds__(GPC_THREADS)
void gp_proj_coef_kernel(const GpProjCoefArgs a) {
    extern __shared__ __attribute__((aligned(16))) double gpc_smem[];
    constexpr int CH = GPC_THREADS / G;                   // chains per wave
    const int lane = threadIdx.x, g = lane / G, gl = lane % G;
    const long long j = (long long)blockIdx.x * CH + g;
    const bool live = j < a.M;
    const int k = a.k;
    double* Lp = gpc_smem + (size_t)g * (k * (k + 1) / 2 + 2 * k);      // this group's packed factor
    double* vv = Lp + k * (k + 1) / 2;                    // [k] the chain's variances
    double* mm = vv + k;                                  // [k] the chain's means, then w
    for (int t = gl; t < k; t += G) {
        vv[t] = live ? a.var[(size_t)t * a.M + j] : 0.0;
        mm[t] = live ? a.mean[(size_t)t * a.M + j] : 0.0;
    }
    __syncthreads();
    const int i0 = gl, i1 = gl + G;                       // this lane's rows
    const bool in0 = i0 < k, in1 = SLOTS == 2 && i1 < k;
    // ---- 1. gp_score_proj_kernel's factor and forward substitution ----
    double d0 = 0.0, d1 = 0.0;
    for (int t = 0; t < k; ++t) {
        const double m = mm[t];
        if (in0) d0 = fma(a.Rt[(size_t)t * k + i0], m, d0);
        if (SLOTS == 2) { if (in1) d1 = fma(a.Rt[(size_t)t * k + i1], m, d1); }
    }
    if (in0) d0 = d0 + a.a0[i0];
    if (SLOTS == 2) { if (in1) d1 = d1 + a.a0[i1]; }
    double q = a.c_perp, ld = a.logdet ? a.hld : 0.0;
    double z0 = 0.0, z1 = 0.0;                            // z of this lane's rows
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
        if (i0 == c) z0 = zc;
        if (SLOTS == 2) { if (i1 == c) z1 = zc; }
        base += k - c - 1;
        __syncthreads();
    }
    // ---- 2. w = L^{-T} z; column i of the packed factor starts at Lp[b + i] with b = i k - i (i + 1) / 2 ----
    const int b0 = in0 ? i0 * k - i0 * (i0 + 1) / 2 : 0, b1 = in1 ? i1 * k - i1 * (i1 + 1) / 2 : 0;
    for (int c = k - 1; c >= 0; --c) {
        const double zc = __shfl(SLOTS == 2 && c >= G ? z1 : z0, c & (G - 1), G);
        const double wc = zc / Lp[c * k - c * (c + 1) / 2 + c];
        if (in0 && i0 < c) z0 = fma(-Lp[b0 + c], wc, z0);
        if (SLOTS == 2) { if (in1 && i1 < c) z1 = fma(-Lp[b1 + c], wc, z1); }
        if (i0 == c) mm[c] = wc;
        if (SLOTS == 2) { if (i1 == c) mm[c] = wc; }
    }
    __syncthreads();
    // ---- 3. e = R^T w ----
    double e0 = 0.0, e1 = 0.0;
    for (int i = 0; i < k; ++i) {
        const double wi = mm[i];
        if (in0) e0 = fma(a.R[(size_t)i * k + i0], wi, e0);
        if (SLOTS == 2) { if (in1) e1 = fma(a.R[(size_t)i * k + i1], wi, e1); }
    }
    double h0 = 0.0, h1 = 0.0;
    if (a.logdet) {                                       // (wave-uniform)
        // ---- 4. X = L^{-1} over L, columns right to left ----
        for (int c = k - 1; c >= 0; --c) {
            const int bc = c * k - c * (c + 1) / 2;       // element (i, c) at Lp[bc + i]
            const double lcc = Lp[bc + c];
            double s0 = 0.0, s1 = 0.0;
            int bs = bc + k - c - 1;                      // element (i, s) at Lp[bs + i]
            for (int s = c + 1; s < k; ++s) {
                const double lsc = Lp[bc + s];            // the original L[s][c]: one address per group
                if (in0 && i0 >= s) s0 = fma(Lp[bs + i0], lsc, s0);
                if (SLOTS == 2) { if (in1 && i1 >= s) s1 = fma(Lp[bs + i1], lsc, s1); }
                bs += k - s - 1;
            }
            if (in0 && i0 >= c) Lp[bc + i0] = i0 == c ? 1.0 / lcc : -s0 / lcc;
            if (SLOTS == 2) { if (in1 && i1 >= c) Lp[bc + i1] = i1 == c ? 1.0 / lcc : -s1 / lcc; }
            __syncthreads();
        }
        // ---- 5. h_t = sum_i (X R)_it^2 ----
        for (int i = 0; i < k; ++i) {
            double y0 = 0.0, y1 = 0.0;
            int bs = 0;
            for (int s = 0; s <= i; ++s) {
                const double x = Lp[bs + i];              // X[i][s]: one address per group
                if (in0) y0 = fma(x, a.R[(size_t)s * k + i0], y0);
                if (SLOTS == 2) { if (in1) y1 = fma(x, a.R[(size_t)s * k + i1], y1); }
                bs += k - s - 1;
            }
            h0 = fma(y0, y0, h0);
            if (SLOTS == 2) h1 = fma(y1, y1, h1);
        }
    }
    if (!live) return;                                    // (behind the last barrier)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double ph = 0.5 * q + ld;
    if (bad) ph = nan;
    if (gl == 0) a.phid[j] = ph;
    if (in0) {
        a.ca[(size_t)i0 * a.M + j] = bad ? nan : e0;
        a.cb[(size_t)i0 * a.M + j] = bad ? nan : 0.5 * (h0 - e0 * e0);
    }
    if (SLOTS == 2) {
        if (in1) {
            a.ca[(size_t)i1 * a.M + j] = bad ? nan : e1;
            a.cb[(size_t)i1 * a.M + j] = bad ? nan : 0.5 * (h1 - e1 * e1);
        }
    }
}

// the instantiation for k: f(kernel, chains per wave)
template <typename F>
static int gp_proj_coef_pick(int k, F f) {
    if (k <= 16) return f(gp_proj_coef_kernel<16, 1>, 4);
    if (k <= 32) return f(gp_proj_coef_kernel<32, 1>, 2);
    if (k <= 64) return f(gp_proj_coef_kernel<64, 1>, 1);
    return f(gp_proj_coef_kernel<64, 2>, 1);
}

// once per installed descriptor (cesx_gp_proj_set): the instantiation for this k may take its dynamic LDS
int gp_proj_coef_prepare(Engine& e, int k) {
    const int lds = (int)gp_proj_lds(k);
    return gp_proj_coef_pick(k, [&](auto kern, int) -> int {
        CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        return CESX_OK;
    });
}

int launch_gp_proj_coef(Engine& e, const double* mean, const double* var, double* phid, double* ca, double* cb, hipStream_t s) {
    GpProjCoefArgs a{};
    a.mean = mean; a.var = var; a.k = e.gpp.k; a.M = e.J;
    a.R = e.gpp.R; a.Rt = e.gpp.Rt; a.a0 = e.gpp.a0;
    a.c_perp = e.gpp.c_perp; a.hld = e.gpp.half_logdet_gamma; a.logdet = e.gpp.logdet;
    a.phid = phid; a.ca = ca; a.cb = cb;
    if (e.J >= (1LL << 31)) { e.err = "cesx_gp_proj: too many chains for one projected launch"; return CESX_EUNSUPPORTED; }
    return gp_proj_coef_pick(a.k, [&](auto kern, int ch) -> int {
        hipLaunchKernelGGL(kern, dim3((unsigned)((e.J + ch - 1) / ch)), dim3(GPC_THREADS), gp_proj_lds(a.k), s, a);
        CESX_HIP(hipGetLastError());
        return CESX_OK;
    });
}

}  // namespace cesx
