// The leapfrog step of MCMC.model_mh / gp_mh(chains=M, update='hmc') on the step path (include/cesx.h, cesx_mh_hmc_* and
// cesx_gp_hmc_*): one thread per chain beside the lv_* kernels (kernels_gpgrad.hip), scoring with their lv_score
// (lv_score.h), so the same three kernels serve the closed-form maps (mode CESX_GP_GAMMA on G, DG of cesx_map_jac) and the
// emulator (the rows of cesx_gp_predict_grad in the three likelihood modes).  All arithmetic is fp64 whatever the engine
// dtype; an fp32 engine stores Q rounded after every leapfrog, because the forward map reads that array.
//
// With S the scale, g = S^T grad phi and L leapfrogs, one step of a chain at U is
//     hm_begin_kernel    r = xi - g(U) / 2,  Q = U + S r                          (l = 1: lv_propose_kernel's sums, its bits)
//     hm_leap_kernel     phi(Q), g(Q);  r = r - g(Q);  Q = Q + S r                (L - 1 times, Q in place)
//     hm_accept_kernel   phi(Q), g(Q);  r = r - g(Q) / 2;
//                        log u < phi(U) - phi(Q) + (|xi|^2 / 2 - |r|^2 / 2)  ->  U := Q, phi := phi(Q), g := g(Q), counter + 1
// r lives in an engine-owned [p][M] fp64 block (mh.hm_r), the noise block in mh.xi as the Langevin step keeps it, g(Q) in the
// proposal's g buffer (mh.lv_gp).  Every sum runs in a fixed order (rows ascending), so runs are bit-identical; the fused
// kernel (mh_hmc_map_kernel, kernels_maps.hip) restates these sums in this order.
// A non-finite phi(Q) in mid-trajectory poisons r (NaN): with a NaN or an infinity in g, r or Q -- which stay in r by
// r - g and Q + S r -- the test's right-hand side is NaN or -inf and the comparison false.  The chain stays, its phi and g
// untouched: plain IEEE comparison semantics, as lv_accept_kernel has them.
//
// ADAPT (cesx_mh_adapt_set armed the handle, include/cesx.h): the same step with e S in place of S, e one fp64 multiplier shared
// by all chains and read from device memory (a uniform load: ad_update_kernel of kernels_adapt.hip stored it behind the last
// accept, and stream order hands it over), written without rescaling anything stored:
//     begin   r = xi - (e / 2) g(U),  Q = U + e S r        leap   r = r - e g(Q),  Q = Q + e S r
//     accept  r = r - (e / 2) g(Q);  d = phi(U) - phi(Q) + (|xi|^2 / 2 - |r|^2 / 2);  log u < d accepts;
//             alpha[j] = 1 (d >= 0), exp(d) (d < 0), 0 (d NaN): the chain's acceptance probability, for ad_update_kernel
// The ADAPT = false instantiations are the expressions above, untouched.
#include "cesx_internal.h"
#include "lv_score.h"

namespace cesx {

template <typename T>
struct HmArgs {
    LvArgs<T> lv;                                   // lv.X = lv.P = Q: lv_score reads the leapfrog position
    double* r;                                      // [p][M] the momentum
    const double* e;                                // ADAPT: the step multiplier (mh.ad_state[0])
    double* alpha;                                  // ADAPT: [M] the chains' acceptance probabilities of this step
};

// r = xi - g(U) / 2 and the first position Q = U + S r: lv_propose_kernel's expression in its loop order
template <typename T, bool ADAPT>
__global__ __launch_bounds__(LV_THREADS)
void hm_begin_kernel(const HmArgs<T> h) {
    const LvArgs<T>& a = h.lv;
    const long long j = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (j >= a.M) return;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    if constexpr (ADAPT) {
        const double e = *h.e, he = 0.5 * e;
        for (int s = 0; s < p; ++s) {
            double acc = 0.0;
            for (int r = 0; r <= s; ++r) acc = fma(a.S[(size_t)s * p + r], (double)a.xi[r * M + j] - he * a.gu[r * M + j], acc);
            a.P[s * M + j] = (T)((double)a.U[s * M + j] + e * acc);
            h.r[s * M + j] = (double)a.xi[s * M + j] - he * a.gu[s * M + j];
        }
        return;
    }
    for (int s = 0; s < p; ++s) {
        double acc = 0.0;
        for (int r = 0; r <= s; ++r) acc = fma(a.S[(size_t)s * p + r], (double)a.xi[r * M + j] - 0.5 * a.gu[r * M + j], acc);
        a.P[s * M + j] = (T)((double)a.U[s * M + j] + acc);
        h.r[s * M + j] = (double)a.xi[s * M + j] - 0.5 * a.gu[s * M + j];
    }
}

// phi(Q) and g(Q), the full kick r = r - g(Q), the next position Q = Q + S r in place: row s of Q is read once, by its own
// update, after every r of the chain is final
template <typename T, bool ADAPT>
__global__ __launch_bounds__(LV_THREADS)
void hm_leap_kernel(const HmArgs<T> h) {
    const LvArgs<T>& a = h.lv;
    const long long j = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (j >= a.M) return;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    const double ph = lv_score(a, j);
    if constexpr (ADAPT) {
        const double e = *h.e;
        for (int r = 0; r < p; ++r) h.r[r * M + j] = h.r[r * M + j] - e * a.gx[r * M + j];
        if (!(ph - ph == 0.0)) h.r[j] = __builtin_nan("");
        for (int s = 0; s < p; ++s) {
            double acc = 0.0;
            for (int r = 0; r <= s; ++r) acc = fma(a.S[(size_t)s * p + r], h.r[r * M + j], acc);
            a.P[s * M + j] = (T)((double)a.P[s * M + j] + e * acc);
        }
        return;
    }
    for (int r = 0; r < p; ++r) h.r[r * M + j] = h.r[r * M + j] - a.gx[r * M + j];
    if (!(ph - ph == 0.0)) h.r[j] = __builtin_nan("");       // (an infinite or NaN phi whose g is finite all the same)
    for (int s = 0; s < p; ++s) {
        double acc = 0.0;
        for (int r = 0; r <= s; ++r) acc = fma(a.S[(size_t)s * p + r], h.r[r * M + j], acc);
        a.P[s * M + j] = (T)((double)a.P[s * M + j] + acc);
    }
}

// phi(Q) and g(Q) at the last position, the half kick, the two norms and the test; an accepted chain takes Q, phi and g
template <typename T, bool ADAPT>
__global__ __launch_bounds__(LV_THREADS)
void hm_accept_kernel(const HmArgs<T> h) {
    const LvArgs<T>& a = h.lv;
    const long long j = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (j >= a.M) return;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    const double ph = lv_score(a, j);
    if constexpr (ADAPT) {
        const double he = 0.5 * *h.e;
        double n1 = 0.0, n2 = 0.0;
        for (int r = 0; r < p; ++r) {
            const double x = (double)a.xi[r * M + j];
            const double d = h.r[r * M + j] - he * a.gx[r * M + j];
            n1 = fma(x, x, n1);
            n2 = fma(d, d, n2);
        }
        const double lu = a.c.logu ? a.c.logu[j] : mh_log_uniform((unsigned long long)(a.c.j_offset + j), a.c.step, a.c.seed_lo, a.c.seed_hi);
        const double d = a.c.phi[j] - ph + (0.5 * n1 - 0.5 * n2);
        h.alpha[j] = d >= 0.0 ? 1.0 : d < 0.0 ? exp(d) : 0.0;      // (NaN: neither comparison holds)
        if (lu < d) {
            a.c.phi[j] = ph;
            a.c.cnt[j] += 1ull;
            for (int r = 0; r < p; ++r) {
                a.U[r * M + j] = a.X[r * M + j];
                a.gu[r * M + j] = a.gx[r * M + j];
            }
        }
        return;
    }
    double n1 = 0.0, n2 = 0.0;
    for (int r = 0; r < p; ++r) {
        const double x = (double)a.xi[r * M + j];
        const double d = h.r[r * M + j] - 0.5 * a.gx[r * M + j];
        n1 = fma(x, x, n1);
        n2 = fma(d, d, n2);
    }
    const double lu = a.c.logu ? a.c.logu[j] : mh_log_uniform((unsigned long long)(a.c.j_offset + j), a.c.step, a.c.seed_lo, a.c.seed_hi);
    if (lu < a.c.phi[j] - ph + (0.5 * n1 - 0.5 * n2)) {
        a.c.phi[j] = ph;
        a.c.cnt[j] += 1ull;
        for (int r = 0; r < p; ++r) {
            a.U[r * M + j] = a.X[r * M + j];
            a.gu[r * M + j] = a.gx[r * M + j];
        }
    }
}

template <typename T>
static int hm_t(Engine& e, int what, int mode, void* Q, const double* mean, const double* var, const double* dmean,
                const double* dvar, void* U, const double* logu, unsigned step, hipStream_t s) {
    HmArgs<T> h{};
    LvArgs<T>& a = h.lv;                            // (filled as lv_t of kernels_gpgrad.hip fills it for a proposal)
    a.mean = mean; a.var = var; a.dmean = dmean; a.dvar = dvar;
    a.n = mode == CESX_GP_PROJ ? e.gpp.k : e.n; a.p = e.p; a.mode = mode; a.M = e.J;
    a.phid = e.mh.phi_data;
    a.y = e.d_y; a.gw = e.d_gw; a.gam = e.d_Gamma; a.Lg = e.whiten ? e.d_Wh : nullptr;
    a.X = (const T*)Q; a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get();
    a.S = e.mh.bS;
    a.ca = e.mh.lv_a; a.cb = e.mh.lv_b; a.gphi = e.mh.lv_gphi;
    a.gu = e.mh.lv_g; a.gx = e.mh.lv_gp.get();
    a.xi = (const T*)e.mh.xi.get(); a.U = (T*)U; a.P = (T*)Q;
    a.c = mh_chains(e, false, logu, step);
    h.r = e.mh.hm_r;
    const dim3 grid((unsigned)((e.J + LV_THREADS - 1) / LV_THREADS)), block(LV_THREADS);
    if (e.mh.ad_armed) {                            // cesx_mh_adapt_set: the step at e S, alpha for ad_update_kernel
        h.e = e.mh.ad_state.get(); h.alpha = e.mh.ad_alpha.get();
        if (what == 0) hipLaunchKernelGGL((hm_begin_kernel<T, true>), grid, block, 0, s, h);
        else if (what == 1) hipLaunchKernelGGL((hm_leap_kernel<T, true>), grid, block, 0, s, h);
        else hipLaunchKernelGGL((hm_accept_kernel<T, true>), grid, block, 0, s, h);
        CESX_HIP(hipGetLastError());
        return CESX_OK;
    }
    if (what == 0) hipLaunchKernelGGL((hm_begin_kernel<T, false>), grid, block, 0, s, h);
    else if (what == 1) hipLaunchKernelGGL((hm_leap_kernel<T, false>), grid, block, 0, s, h);
    else hipLaunchKernelGGL((hm_accept_kernel<T, false>), grid, block, 0, s, h);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

// what: 0 begin (r and the first Q from U, the noise block in mh.xi and the chains' g), 1 leap (the rows and gradients at Q;
// Q advances in place), 2 accept (the rows and gradients at the last Q; U takes the accepted columns)
int launch_hmc(Engine& e, int what, int mode, void* Q, const double* mean, const double* var, const double* dmean,
               const double* dvar, void* U, const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? hm_t<float>(e, what, mode, Q, mean, var, dmean, dvar, U, logu, step, s)
                                   : hm_t<double>(e, what, mode, Q, mean, var, dmean, dvar, U, logu, step, s);
}

}  // namespace cesx
