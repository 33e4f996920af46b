// The state of the stages behind Calibrate, one struct per stage (Engine members mh, gp, gpd, gpp, gf, dc, l9, l6, mp, cs, ch, ca).  Each owns its
// device memory (DevBuf: freed with the struct), says what "nothing installed" is, and has one drop() that establishes it.
// drop() releases the buffers whose size comes from the installed descriptor and keeps the ones sized by the engine's
// shape alone (allocated on first use, reused by every later install).  No hip/ header: tools/devbuf_check.cpp runs these
// structs on the host.
#pragma once
#include <vector>
#include "devbuf.h"
#include "../../include/cesx.h"

namespace cesx {

// ---- Metropolis-Hastings over the columns (cesx_mh_*, kernels_mh.hip); the chains of cesx_gp_* are these too ----
struct MhState {
    int kind = -1;                     // CESX_MH_RW / CESX_MH_PCN / CESX_MH_LANGEVIN after cesx_mh_set_proposal, -1: none (cesx_set_problem drops it)
    double a = 1.0;                    // P = a U + (b S) xi
    bool dense_prior = false;          // RW with a dense Sigma: the prior term is scored through w = L_Sigma^{-1} (u - mu)
    bool started = false;
    bool lv_proposed = false;          // Langevin: a cesx_gp_langevin_propose since the start or the last accept (its block is in xi)
    unsigned long long steps = 0;      // cesx_mh_accept calls since cesx_mh_start
    DevBuf<void> W, Wf;                // b S zero padded [rpad][kp], row-major and in the LDS-DMA kernels' order
    DevBuf<void> Li, Li_f;             // dense prior: L_Sigma^{-1} in the same two layouts
    DevBuf<void> lb;                   // dense prior: -L_Sigma^{-1} mu [rpad] (the bias of the w launch)
    DevBuf<void> w;                    // dense prior: [p][J] w of the states being scored
    DevBuf<void> xi;                   // fp64: [p][J] the step's noise block (update3_kernel reads segments from memory); Langevin: either dtype, kept from propose to accept
    DevBuf<double> phi;                // [J] phi of the chains' current states
    DevBuf<unsigned long long> cnt;    // [J] accepted proposals per chain
    DevBuf<double> LSi;                // [p][p] L_Sigma^{-1} of a dense Sigma, fp64: the dense prior's factor as gp_score_kernel reads it
    DevBuf<double> bS;                 // [p][p] b S, fp64 row-major: the proposal as gp_chain_kernel reads it (cesx_gp_run)
    std::vector<double> h_bS;          // [p][p] b S on the host: cesx_mh_run_map passes it by value
    DevBuf<double> lv_g, lv_gp;        // Langevin: [p][J] g = S^T grad phi of the chains' states and of the proposals (kernels_gpgrad.hip)
    DevBuf<double> lv_a, lv_b, lv_gphi; // Langevin: [max(n, k)][J] twice, [p][J] what lv_score keeps per chain: a_i, b_i, grad phi (k: CESX_GP_PROJ's rows)
    DevBuf<double> phi_data;           // Langevin, CESX_GP_PROJ: [J] the data term of phi of the states being scored (kernels_gpprojgrad.hip)
    // HMC under a Langevin proposal (cesx_mh_hmc_* / cesx_gp_hmc_*, kernels_hmc.hip): the chains' phi, g and noise block are the Langevin step's
    bool hm_begun = false;             // a cesx_mh_hmc_begin since the start or the last accept: xi and hm_r belong to a trajectory in flight
    DevBuf<double> hm_r;               // [p][J] the momentum r of the trajectory in flight
    // Langevin on a linear map (cesx_mh_langevin_lineal_*, kernels_lvlin.hip): the gradient is an update launch over these images
    int lin = 0;                       // 0: no cesx_mh_langevin_lineal_set; 1: lineal (one launch); 2: lineal_log (two launches and exp)
    bool lin_started = false;          // the LAST start was cesx_mh_langevin_lineal_start: g lives in lin_g, not in lv_g
    DevBuf<void> lin_Wa, lin_Wa_f;     // lineal: S^T [A^T M | Sigma^{-1}] [rpad][kn + kp]; lineal_log: A^T M [rpad][kn]; both layouts, as W / Wf
    DevBuf<void> lin_Wb, lin_Wb_f;     // lineal_log: [S^T | S^T Sigma^{-1}] [rpad][2 kp]
    DevBuf<void> lin_ba, lin_bb;       // [rpad] the biases of the two launches
    DevBuf<void> lin_g, lin_gp, lin_z; // [p][J] engine dtype: g of the chains' states, of the proposals, and z = xi - g / 2
    DevBuf<void> lin_t;                // lineal_log: [p][J] t0, then h = exp(X) (.) t0
    // leapfrog on a linear map (cesx_mh_hmc_lineal_*, kernels_hmclin.hip): the momentum r lives in lin_z; armed, r in lin_r and z = e r in lin_z
    DevBuf<void> lin_r;                // [p][J] engine dtype: the momentum of an armed handle's trajectory (allocated by its first begin)
    int hl_leaps = 0;                  // cesx_mh_hmc_lineal_leap calls since the begin
    // pooled step-size adaptation (cesx_mh_adapt_*, kernels_adapt.hip): while armed the hm_* launches take e S for S
    bool ad_armed = false;             // a cesx_mh_adapt_set since the last cesx_mh_set_proposal / cesx_set_problem
    int ad_n = 0, ad_done = 0;         // adaptation steps asked for, and accepts made (each followed by ad_update_kernel)
    double ad_target = 0.0, ad_gain = 0.0, ad_kappa = 0.0;
    DevBuf<double> ad_alpha;           // [J] the chains' acceptance probabilities of the step in hand
    DevBuf<double> ad_state;           // [4] e, log e, log ebar, t
    DevBuf<double> ad_hist;            // [ad_n][2] row t - 1: e_t, abar_t
    // where the Langevin / leapfrog entry points take the data term of grad phi from (cesx_mh_grad_source): the Jacobian image, or ready-made
    int grad_source = 0;               // CESX_MH_GRAD_JACOBIAN; CESX_MH_GRAD_READY: the dc_* kernels (kernels_darcy_chain.hip)
    bool none() const { return kind < 0; }
    // every buffer is sized by the engine: kept -- but the adaptation's history, which its step count sizes
    void drop() { kind = -1; grad_source = 0; started = false; lv_proposed = false; hm_begun = false; lin = 0; lin_started = false; ad_armed = false; ad_n = 0; ad_done = 0; ad_hist.reset(); }
};

// ---- GP emulator over the columns (cesx_gp_*, kernels_gp.hip) ----
struct GpState {
    int n = 0, Jt = 0, Jp = 0;         // GPs, training points, training points rounded up to 16 (n 0: no emulator)
    size_t li_len = 0;                 // doubles of one GP's packed L^{-1} (Jp/16 (Jp/16 + 1)/2 blocks of 256)
    bool matern12 = false;             // a GP of family 1: no gradient (cesx_gp_predict_grad refuses)
    DevBuf<double> A;                  // [n][p][p] the input maps A_i (lower triangular)
    DevBuf<double> c;                  // [p] the input shift c
    DevBuf<double> Z;                  // [n][Jt][p] the mapped training points
    DevBuf<double> par;                // [n][4] sigma^2, sn^2, mean bias, kernel family
    DevBuf<double> mw;                 // [n][p] the affine mean's weights over z
    DevBuf<double> alpha;              // [n][Jp] alpha, zero padded
    DevBuf<double> Li;                 // [n][li_len] L^{-1} in v_mfma_f64_16x16x4 A-operand order
    DevBuf<double> ws;                 // the K* panels of the launches that do not fit in LDS (grown by launch_gp_predict)
    bool none() const { return n == 0; }
    void drop() {                      // the image goes, ws stays
        n = 0;
        A.reset(); c.reset(); Z.reset(); par.reset(); mw.reset(); alpha.reset(); Li.reset();
    }
};

// ---- the dense per-chain Sigma of CESX_GP_DENSE (cesx_gp_dense_set, kernels_gpdense.hip) ----
struct GpDenseState {
    int k = 0, logdet = 0;             // columns of B (0: no descriptor; cesx_set_problem drops it), the log det term
    DevBuf<double> B, Bt;              // B [n][k] and its transpose [k][n]; both [n][n]: the largest k fits
    DevBuf<double> g0;                 // [n] the mean shift (zeros for a NULL g0)
    DevBuf<double> y, Gam;             // [n], [n][n] the unwhitened problem on the device
    bool none() const { return k == 0; }
    void drop() { k = 0; }             // every buffer is sized by the engine: kept
};

// ---- Sigma projected to k x k of CESX_GP_PROJ (cesx_gp_proj_set, kernels_gpproj.hip) ----
struct GpProjState {
    int k = 0, logdet = 0;             // the order of R (0: no descriptor; cesx_set_problem drops it), the log det term
    double c_perp = 0.0;               // |(I - Q Q^T) r0|^2, the part of the quadratic form no chain changes
    double half_logdet_gamma = 0.0;    // sum log diag(L_Gamma)
    DevBuf<double> R, Rt;              // R [k][k] (zero below the diagonal) and its transpose; both KMAX x KMAX: every k fits
    DevBuf<double> a0;                 // [k] Q^T r0
    bool none() const { return k == 0; }
    void drop() { k = 0; }             // every buffer is sized by CESX_GP_PROJ_KMAX: kept
};

// ---- GP training: batched likelihood and gradient (cesx_gpfit_*, kernels_gpfit.hip) ----
struct GpFitState {
    int n = 0, Jt = 0, Jp = 0;         // GPs, training points, training points rounded up to 16 (n 0: no fit problem)
    int family = 0, ard = 0, mean = 0; // kernel family, ARD, mean kind (CESX_GPFIT_MEAN_*): one of each per problem
    int nl = 0, ntheta = 0, ntile = 0; // lengthscales (p or 1), parameters per GP, 64 x 64 tiles of the lower triangle
    DevBuf<double> X, Y;               // [Jt][p], [n][Jt]
    DevBuf<double> Xs;                 // [n][Jp][p] X / l of the last evaluation
    DevBuf<double> r, t, alpha;        // [n][Jp]: y - m(X), L^{-1} r, alpha
    DevBuf<double> A, W, Ki;           // [n][Jp][Jp]: Ky -> L, L^{-T}, K^{-1}
    DevBuf<double> Ld;                 // [n][Jp][16] the diagonal blocks of L (Ky's stay in A: every workgroup of a launch reads them)
    DevBuf<double> part;               // [n][ntile][nl + 2] the gradient pass's partial sums
    DevBuf<double> theta, out;         // [n][ntheta], [n][2 + ntheta] of the evaluation in flight
    DevBuf<int> idx, status;           // [n]
    std::vector<double> h_out;
    bool none() const { return n == 0; }
    void drop() {                      // everything is sized by the descriptor
        n = 0;
        X.reset(); Y.reset(); Xs.reset(); r.reset(); t.reset(); alpha.reset(); A.reset(); W.reset(); Ki.reset(); Ld.reset();
        part.reset(); theta.reset(); out.reset(); idx.reset(); status.reset();
    }
};

// ---- Darcy forward map over the columns (cesx_darcy_*, kernels_darcy.hip, kernels_darcy_stream.hip); state of its own: the lineal map is untouched ----
struct DarcyState {
    int K = 0;                         // Nmesh of the installed map (0: none)
    bool streamed = false;             // installed by cesx_darcy_set_streamed: cesx_darcy_apply launches kernels_darcy_stream.hip
    int slots = 0;                     // streamed: workspace slots = the largest grid an apply launches (0: resident)
    DevBuf<double> mat;                // [4][K][K] coef (K folded in, entry 0 zero), D, S, R, row-major
    DevBuf<int> idx;                   // [p] scatter, then [n] obs_index
    DevBuf<double> ws;                 // streamed: [slots][n][2 m + 1] the finished rows of U, one slot per workgroup in flight
    DevBuf<double> gscr;               // cesx_darcy_grad: [J][2 n_obs] r and c of each particle (kernels_darcy_grad.hip); sized by the engine: kept
    bool none() const { return K == 0; }
    void drop() { K = 0; streamed = false; slots = 0; mat.reset(); idx.reset(); ws.reset(); }
};

// ---- Lorenz '96 forward map over the columns (cesx_lorenz_*, kernels_l96.hip); state of its own, as the Darcy map's ----
struct L96State {
    cesx_l96_desc desc{};              // the installed descriptor (n_slow 0: none; its t points nowhere: the member t)
    DevBuf<double> t;                  // [n_t] the sample times
    bool none() const { return desc.n_slow == 0; }
    void drop() { desc = cesx_l96_desc{}; t.reset(); }
};

// ---- Lorenz '63 forward map over the columns (cesx_lorenz_three_*, kernels_l63.hip); state of its own, as the Lorenz '96 map's ----
struct L63State {
    cesx_l63_desc desc{};              // the installed descriptor (n_t 0: none; its t points nowhere: the member t)
    DevBuf<double> t;                  // [n_t] the sample times
    bool none() const { return desc.n_t == 0; }
    void drop() { desc = cesx_l63_desc{}; t.reset(); }
};

// ---- closed-form maps over the columns (cesx_map_*, cesx_mh_run_map, kernels_maps.hip); state of its own, as the Lorenz maps' ----
struct MapState {
    cesx_map_desc desc{};              // the installed descriptor (kind 0: none); passed to the kernels by value: no device memory
    bool none() const { return desc.kind == 0; }
    bool fused() const { return desc.kind == CESX_MAP_ELLIPTIC || desc.kind == CESX_MAP_BANANA; }   // cesx_mh_run_map has it
    void drop() { desc = cesx_map_desc{}; }
};

// ---- streaming summaries of the chains' draws (cesx_chain_summary_*, kernels_chainsum.hip); state of its own: cesx_set_problem does not touch it ----
struct ChainSumState {
    long long N = 0, added = 0;        // draws of the run in hand (0: no cesx_chain_summary_begin), draws added so far
    int slabs = 0;                     // column slabs of the pooled launch (kernels_chainsum.hip, cs_slab_cols): the rows of `part`
    DevBuf<double> shift;              // [p][J] every chain's first draw: the shift of its half sums
    DevBuf<double> S;                  // [2 halves][2: S1, S2][p][J] sum (x - shift), sum (x - shift)^2
    DevBuf<double> c;                  // [p] the pooled shift: the row mean of the first draw
    DevBuf<double> cpart;              // [p][slices] the row sums behind c
    DevBuf<double> tot;                // [p][p] sum (x - c)(x - c)^T, lower triangle, then [p] sum (x - c): the run's totals
    DevBuf<double> part;               // [slabs][pairs][64][64] a launch's cross moments per slab, then [slabs][pp] its row sums
    DevBuf<double> hpart;              // [p][blocks][3] the half-chain reduce's partials, then [p][3] sum (m - c), sum (m - c)^2, sum s^2
    DevBuf<double> half;               // [2: m, s^2][2 halves][p][J], only while a cesx_chain_summary_read that asks for them runs
    bool none() const { return N == 0; }
    void drop() { N = 0; added = 0; half.reset(); }       // every other buffer is sized by the engine: kept
};

// ---- streaming 1-D and 2-D marginals of the chains' draws (cesx_chain_hist_*, kernels_chainhist.hip); state of its own: cesx_set_problem does not touch it ----
struct ChainHistState {
    int bins = 0, bins2 = 0, n_pairs = 0;      // of the run in hand (bins 0: no cesx_chain_hist_begin)
    long long added = 0;                       // draws added so far
    // every buffer is sized by the engine's p and the caps of include/cesx.h (CESX_CHAIN_HIST_*_MAX): allocated by the first begin
    DevBuf<double> edges1;                     // [p][bins + 1]
    DevBuf<double> edges2;                     // [n_pairs][2][bins2 + 1] the edges of each pair's first and second row
    DevBuf<int> pairs;                         // [n_pairs][2]
    DevBuf<unsigned long long> tot1;           // [p][bins + 2] the run's counts: the bins, below, above
    DevBuf<unsigned long long> tot2;           // [n_pairs][bins2][bins2], then [n_pairs] outside
    bool none() const { return bins == 0; }
    void drop() { bins = 0; bins2 = 0; n_pairs = 0; added = 0; }      // every buffer is sized by the engine: kept
};

// ---- streaming lagged sums of the chains' draws (cesx_chain_acf_*, kernels_chainacf.hip); state of its own: cesx_set_problem does not touch it ----
struct ChainAcfState {
    long long N = 0, added = 0, done = 0;      // draws of the run in hand (0: no cesx_chain_acf_begin), draws added, draws in the sums
    int L = 0, LT = 0, C = 0;                  // lags, the ring's slots (kernels_chainacf.hip, acf_lt), chains followed
    int pend = 0;                              // draws waiting in `pending`: added - done
    // every buffer is [..][p][C]: sized by the run, grown by a begin that needs more and kept otherwise
    DevBuf<double> c, S1;                      // every chain's first draw (the shift) and sum a
    DevBuf<double> P;                          // [LT + 1] the lagged sums P_k
    DevBuf<double> ring;                       // [LT] a_t in slot t mod LT: the last LT values
    DevBuf<double> head;                       // [L] a_0 .. a_{L-1}
    DevBuf<void> pending;                      // [ACF_BLOCK] draws of the C chains in the engine dtype
    DevBuf<double> out;                        // [L + 1][p] sum G_k, then [p] each: cbar, sum (m - cbar), sum (m - cbar)^2
    DevBuf<double> gamma, mean;                // [L + 1][p][C], [p][C]: only while a cesx_chain_acf_read runs
    bool none() const { return N == 0; }
    void drop() { N = 0; added = 0; done = 0; L = 0; LT = 0; C = 0; pend = 0; gamma.reset(); mean.reset(); }
};

}  // namespace cesx
