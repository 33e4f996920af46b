// What the one-thread-per-chain kernels of the gradient samplers share: the Langevin step (lv_* kernels, kernels_gpgrad.hip)
// and the leapfrog step (hm_* kernels, kernels_hmc.hip) score a chain with the SAME function, so phi and g = S^T grad phi of a
// state are the same bits whichever sampler left them -- single Langevin steps and HMC steps alternate on one handle.
#pragma once
#include "cesx_internal.h"

namespace cesx {

template <typename T>
struct LvArgs {
    const double *mean, *var, *dmean, *dvar;        // the GP rows [n][M] and their gradients [n][p][M] at X
    const double* phid;                             // CESX_GP_PROJ: [M] the data term of phi at X (gp_proj_coef_kernel)
    int n, p, mode; long long M;                    // (CESX_GP_PROJ: n is the descriptor's k)
    const double *y, *gw, *gam, *Lg;                // gp_score_kernel's data: y (whitened when Lg != nullptr), 1 / Gamma_ii, Gamma, L_Gamma^{-1}
    const T* X; const double *mu, *sw, *LSi;        // and its prior: diagonal (sw) or dense (LSi = L_Sigma^{-1})
    const double* S;                                // [p][p] the lower-triangular scale
    double *ca, *cb, *gphi;                         // engine scratch [n][M], [n][M], [p][M]: a_i, b_i, grad phi
    double* gx;                                     // [p][M] g = S^T grad phi at X (lv_score writes it)
    double* gu;                                     // [p][M] g at the chains' states U
    const T* xi;                                    // [p][M] the step's noise block
    T *U, *P;
    MhChains c;
};

constexpr int LV_THREADS = 256;

// phi of chain j at X (gp_score_kernel's sums in its order) and g = S^T grad phi into a.gx
template <typename T>
__device__ __forceinline__ double lv_score(const LvArgs<T>& a, long long j) {
    const int n = a.n, p = a.p;
    const size_t M = (size_t)a.M;
    double s = 0.0;
    if (a.mode == CESX_GP_PROJ) {
        // ca and cb are filled: a_t = e_t, b_t = 1/2 ([logdet] h_t - e_t^2) of gp_proj_coef_kernel (kernels_gpprojgrad.hip), which
        // factored I_k + R diag(v) R^T of this chain; the data term of phi is a.phid[j] and s sums the prior term alone
    } else if (a.mode == CESX_GP_GAMMA) {
        if (a.Lg) {
            for (int i = 0; i < n; ++i) {
                double w = 0.0;
                for (int k = 0; k <= i; ++k) w = fma(a.Lg[(size_t)i * n + k], a.mean[k * M + j], w);
                const double d = w - a.y[i];
                s = fma(d, d, s);
                a.ca[i * M + j] = d;
            }
            // a = L_Gamma^{-T} d in place: a_k reads d_i, i >= k, and overwrites d_k, which no later a needs
            for (int k = 0; k < n; ++k) {
                double acc = 0.0;
                for (int i = k; i < n; ++i) acc = fma(a.Lg[(size_t)i * n + k], a.ca[i * M + j], acc);
                a.ca[k * M + j] = acc;
            }
        } else {
            for (int i = 0; i < n; ++i) {
                const double d = a.mean[i * M + j] - a.y[i];
                s = fma(a.gw[i], d * d, s);
                a.ca[i * M + j] = a.gw[i] * d;
            }
        }
    } else {
        for (int i = 0; i < n; ++i) {
            double v = a.var[i * M + j];
            if (a.mode == CESX_GP_GAMMA_VAR) v = a.gam[(size_t)i * (n + 1)] + v;
            const double d = a.mean[i * M + j] - a.y[i];
            s += d * d / v + log(v);                 // (v <= 0: NaN or inf - inf, the test then rejects)
            a.ca[i * M + j] = d / v;
            a.cb[i * M + j] = 0.5 * (1.0 / v - d * d / (v * v));
        }
    }
    // the prior: Sigma^{-1} (x - mu)
    if (a.LSi) {
        for (int r = 0; r < p; ++r) {
            double w = 0.0;
            for (int k = 0; k <= r; ++k) w = fma(a.LSi[(size_t)r * p + k], (double)a.X[k * M + j] - a.mu[k], w);
            s = fma(w, w, s);
            a.gx[r * M + j] = w;
        }
        for (int q = 0; q < p; ++q) {
            double acc = 0.0;
            for (int r = q; r < p; ++r) acc = fma(a.LSi[(size_t)r * p + q], a.gx[r * M + j], acc);
            a.gphi[q * M + j] = acc;
        }
    } else {
        for (int r = 0; r < p; ++r) {
            const double d = (double)a.X[r * M + j] - a.mu[r];
            s = fma(a.sw[r], d * d, s);
            a.gphi[r * M + j] = a.sw[r] * d;
        }
    }
    // the data term: sum_i a_i grad mean_i + b_i grad var_i
    for (int q = 0; q < p; ++q) {
        double acc = a.gphi[q * M + j];
        for (int i = 0; i < n; ++i) {
            acc = fma(a.ca[i * M + j], a.dmean[((size_t)i * p + q) * M + j], acc);
            if (a.mode != CESX_GP_GAMMA) acc = fma(a.cb[i * M + j], a.dvar[((size_t)i * p + q) * M + j], acc);
        }
        a.gphi[q * M + j] = acc;
    }
    for (int r = 0; r < p; ++r) {
        double acc = 0.0;
        for (int q = r; q < p; ++q) acc = fma(a.S[(size_t)q * p + r], a.gphi[q * M + j], acc);
        a.gx[r * M + j] = acc;
    }
    // (CESX_GP_PROJ: gp_score_proj_kernel's final expression, 1/2 q + ld + 1/2 s, so a start here leaves cesx_gp_start's bits)
    if (a.mode == CESX_GP_PROJ) return a.phid[j] + 0.5 * s;
    return 0.5 * s;
}

}  // namespace cesx
