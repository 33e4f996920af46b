// Closed-form forward maps over the columns (ces/utils.py:33-122: elliptic, banana, the exp prologue of lineal_log) and the
// fused chain kernel of MCMC.model_mh for them.
//
//   map_apply_kernel     G = map(U), one column per lane, fp64 whatever the engine dtype, rounded on the store.
//   mh_run_map_kernel    n_steps Metropolis steps of every chain in ONE launch, one chain per lane.  Per step what
//                        cesx_mh_propose / cesx_map_apply / cesx_mh_accept do in three launches (five with the device noise
//                        of an fp64 engine and a dense prior):
//                            P   = a U + (b S) xi                                       (engine.hip, cesx_mh_propose)
//                            phi = 1/2 |L_Gamma^{-1} (map(P) - y)|^2 + 1/2 |L_Sigma^{-1} (P - mu)|^2   (kernels_mh.hip)
//                            log u < phi(U) - phi(P)  ->  U := P, phi := phi(P), counter + 1          (mh_test)
//                        The chain (P values, phi, its counter) lives in the lane's registers for the whole launch; the problem
//                        (y, the factors of Gamma and Sigma, b S: a handful of doubles at P = N = 2) arrives by value in the
//                        kernel arguments.  No LDS, no exchange between lanes, a plain 1-D grid: a chain's result does not
//                        depend on J_local, on its column or on the other chains.  At p = n = 2 the step path is launch latency
//                        and nothing else; here a step costs its arithmetic (two Philox blocks, the fp64 Box-Muller pair, exp,
//                        log).  All arithmetic is fp64; an fp32 engine rounds where it stores (the trace, U at the end).
//   map_jac_kernel       G = map(U) and DG[i][q] = dG_i / du_q, both fp64 whatever the engine dtype, one column per lane: the
//                        rows [n][J] and gradients [n][p][J] that lv_score (kernels_gpgrad.hip) takes in mode CESX_GP_GAMMA.
//   mh_langevin_map_kernel   mh_run_map_kernel's launch for the preconditioned Metropolis-adjusted Langevin step of
//                        MCMC.model_mh(chains=M, update='langevin') (include/cesx.h, cesx_mh_langevin_*): next to its state,
//                        phi and counter the lane keeps g = S^T grad phi of its state, and per step it forms
//                            P        = U + S (xi - g(U) / 2)
//                            phi(P), grad phi(P) = DG^T Gamma^{-1} (map(P) - y) + Sigma^{-1} (P - mu)     (lv_score's sums)
//                            g(P)     = S^T grad phi(P)
//                            log u < phi(U) - phi(P) + |xi|^2 / 2 - |xi - (g(U) + g(P)) / 2|^2 / 2  ->  U, phi, g := those of P
//                        The chains' g comes from and goes back to mh.lv_g, where the lv_* kernels keep it: fused launches and
//                        single Langevin steps alternate.
//   mh_hmc_map_kernel    mh_langevin_map_kernel with the leapfrog loop inside (MCMC.model_mh(chains=M, update='hmc'), include/cesx.h,
//                        cesx_mh_hmc_run_map): per step r = xi - g(U) / 2, then `leapfrog` times x = x + S r, phi(x), g(x),
//                        r = r - g(x) (half at the last), and the test with both kinetic energies.  It shares phi, g and the
//                        counters with the kernel above and with the hm_* step kernels (kernels_hmc.hip).
//
// The noise is the step path's: xi row r of global chain gj at MH step s from philox(gj, r / 4, s | 2^31) through normal4 in
// fp64 (what noise_kernel<double> draws for an fp64 engine -- for EITHER engine dtype here, so that an fp32 engine's launch is
// the fp64 engine's rounded on the store), the uniform from mh_log_uniform.
#include "cesx_internal.h"

namespace cesx {

constexpr int MAP_THREADS = 64;            // one wave per workgroup: the chains spread over as many CUs as there are waves

// ---- the maps: P parameters -> N observables, fp64 ----
struct MapElliptic {
    static constexpr int P = 2, N = 2;
    double x1, x2;                         // (two doubles: the fused kernel keeps its arguments in scalar registers)
    __host__ explicit MapElliptic(const double* prm) : x1(prm[0]), x2(prm[1]) {}
    __device__ __forceinline__ void operator()(const double u[2], double g[2]) const {
        const double em = exp(-u[0]);
        g[0] = u[1] * x1 + em * (-x1 * x1 + x1) * 0.5;      // ces/utils.py:77-78
        g[1] = u[1] * x2 + em * (-x2 * x2 + x2) * 0.5;
    }
    // DG[i][q] = dg_i / du_q                               ces/utils.py:85-86
    __device__ __forceinline__ void jac(const double u[2], double DG[2][2]) const {
        const double em = exp(-u[0]);
        DG[0][0] = -em * (-x1 * x1 + x1) * 0.5; DG[0][1] = x1;
        DG[1][0] = -em * (-x2 * x2 + x2) * 0.5; DG[1][1] = x2;
    }
    // map and Jacobian together, for the kernels that must agree bit for bit (map_jac_kernel, mh_langevin_map_kernel)
    __device__ __forceinline__ void map_jac(const double u[2], double g[2], double DG[2][2]) const {
        (*this)(u, g);
        jac(u, DG);
    }
};
struct MapBanana {
    static constexpr int P = 2, N = 2;
    double a, b;
    __host__ explicit MapBanana(const double* prm) : a(prm[0]), b(prm[1]) {}
    __device__ __forceinline__ void operator()(const double u[2], double g[2]) const {
        g[0] = u[0] * a;                   // ces/utils.py:120-121
        g[1] = u[1] / a - b * (u[0] * u[0] + a * a);
    }
    __device__ __forceinline__ void jac(const double u[2], double DG[2][2]) const {
        DG[0][0] = a; DG[0][1] = 0.0;
        DG[1][0] = -2.0 * b * u[0]; DG[1][1] = 1.0 / a;
    }
    // map and Jacobian together, for the kernels that must agree bit for bit (map_jac_kernel, mh_langevin_map_kernel): every
    // rounding of operator() spelled out as map_apply_kernel contracts it -- left to the compiler, u1^2 + a^2 is
    // fma(a, a, u1 u1) in a kernel that evaluates it once and fma(u1, u1, a a) in a loop that a a is hoisted out of
    __device__ __forceinline__ void map_jac(const double u[2], double g[2], double DG[2][2]) const {
#pragma clang fp contract(off)
        g[0] = u[0] * a;
        g[1] = fma(-b, fma(a, a, u[0] * u[0]), u[1] / a);
        jac(u, DG);
    }
};

template <typename T, typename Map>
__global__ __launch_bounds__(MAP_THREADS)
void map_apply_kernel(const Map map, const T* __restrict__ U, T* __restrict__ G, long long J) {
    const long long j = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    if (j >= J) return;
    double u[Map::P], g[Map::N];
#pragma unroll
    for (int r = 0; r < Map::P; ++r) u[r] = (double)U[(size_t)r * J + j];
    map(u, g);
#pragma unroll
    for (int i = 0; i < Map::N; ++i) G[(size_t)i * J + j] = (T)g[i];
}

// exp over all p J entries (G may be U)
template <typename T>
__global__ __launch_bounds__(256)
void map_exp_kernel(const T* U, T* G, long long len) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < len) G[i] = (T)exp((double)U[i]);
}

template <typename T, typename Map>
static int map_apply_t(Engine& e, const void* U, void* G, hipStream_t s) {
    const long long blocks = (e.J + MAP_THREADS - 1) / MAP_THREADS;
    if (blocks >= (1LL << 31)) { e.err = "cesx_map_apply: too many columns for one launch"; return CESX_EUNSUPPORTED; }
    hipLaunchKernelGGL((map_apply_kernel<T, Map>), dim3((unsigned)blocks), dim3(MAP_THREADS), 0, s, Map(e.mp.desc.prm),
                       (const T*)U, (T*)G, (long long)e.J);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_map_apply(Engine& e, const void* U, void* G, hipStream_t s) {
    const bool f32 = e.cfg.dtype == CESX_F32;
    switch (e.mp.desc.kind) {
    case CESX_MAP_ELLIPTIC: return f32 ? map_apply_t<float, MapElliptic>(e, U, G, s) : map_apply_t<double, MapElliptic>(e, U, G, s);
    case CESX_MAP_BANANA: return f32 ? map_apply_t<float, MapBanana>(e, U, G, s) : map_apply_t<double, MapBanana>(e, U, G, s);
    case CESX_MAP_EXP: {
        const long long len = (long long)e.p * e.J, blocks = (len + 255) / 256;
        if (blocks >= (1LL << 31)) { e.err = "cesx_map_apply: too many entries for one launch"; return CESX_EUNSUPPORTED; }
        if (f32) hipLaunchKernelGGL((map_exp_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)U, (float*)G, len);
        else hipLaunchKernelGGL((map_exp_kernel<double>), dim3((unsigned)blocks), dim3(256), 0, s, (const double*)U, (double*)G, len);
        CESX_HIP(hipGetLastError());
        return CESX_OK;
    }
    default: e.err = "cesx_map_apply: no map installed"; return CESX_ESTATE;
    }
}

// G and DG of the columns, fp64 both: [n][J] and [n][p][J] (the layout of cesx_gp_predict_grad's mean / dmean)
template <typename T, typename Map>
__global__ __launch_bounds__(MAP_THREADS)
void map_jac_kernel(const Map map, const T* __restrict__ U, double* __restrict__ G, double* __restrict__ DG, long long J) {
    const long long j = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    if (j >= J) return;
    double u[Map::P], g[Map::N], dg[Map::N][Map::P];
#pragma unroll
    for (int r = 0; r < Map::P; ++r) u[r] = (double)U[(size_t)r * J + j];
    map.map_jac(u, g, dg);
#pragma unroll
    for (int i = 0; i < Map::N; ++i) {
        G[(size_t)i * J + j] = g[i];
#pragma unroll
        for (int q = 0; q < Map::P; ++q) DG[((size_t)i * Map::P + q) * J + j] = dg[i][q];
    }
}

template <typename T, typename Map>
static int map_jac_t(Engine& e, const void* U, double* G, double* DG, hipStream_t s) {
    const long long blocks = (e.J + MAP_THREADS - 1) / MAP_THREADS;
    if (blocks >= (1LL << 31)) { e.err = "cesx_map_jac: too many columns for one launch"; return CESX_EUNSUPPORTED; }
    hipLaunchKernelGGL((map_jac_kernel<T, Map>), dim3((unsigned)blocks), dim3(MAP_THREADS), 0, s, Map(e.mp.desc.prm),
                       (const T*)U, G, DG, (long long)e.J);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_map_jac(Engine& e, const void* U, double* G, double* DG, hipStream_t s) {
    const bool f32 = e.cfg.dtype == CESX_F32;
    switch (e.mp.desc.kind) {
    case CESX_MAP_ELLIPTIC: return f32 ? map_jac_t<float, MapElliptic>(e, U, G, DG, s) : map_jac_t<double, MapElliptic>(e, U, G, DG, s);
    case CESX_MAP_BANANA: return f32 ? map_jac_t<float, MapBanana>(e, U, G, DG, s) : map_jac_t<double, MapBanana>(e, U, G, DG, s);
    case CESX_MAP_EXP: e.err = "cesx_map_jac: CESX_MAP_EXP has no Jacobian launch (lineal_log's gradient is an A^T product)"; return CESX_EUNSUPPORTED;
    default: e.err = "cesx_map_jac: no map installed"; return CESX_ESTATE;
    }
}

// ---- the fused chain kernels ----

// The problem and the proposal as one lane needs them, by value: every triangular factor packed (row r at r (r + 1) / 2), both
// quadratic forms through their factors -- a diagonal Gamma or Sigma is the factor diag(1 / sqrt(.)) -- so that the kernel
// arguments stay in scalar registers for the whole launch (P = N = 2: 14 doubles).
template <int P, int N>
struct MapRunProblem {
    double a;                          // P = a U + W xi
    double W[P * (P + 1) / 2];         // b S
    double Lg[N * (N + 1) / 2];        // L_Gamma^{-1}
    double yw[N];                      // L_Gamma^{-1} y
    double Ls[P * (P + 1) / 2];        // L_Sigma^{-1}
    double lb[P];                      // -L_Sigma^{-1} mu  (w = L_Sigma^{-1} x + lb)
    int prior;                         // 0: no prior term (pCN), 1: the prior term (random walk)
};

struct MapRunArgs {
    void* U; void* trace; const void* xi; const double* logu;
    double* phi; unsigned long long* cnt;
    long long J, j_offset;
    unsigned seed_lo, seed_hi, step0;      // step0: the Philox step word of the first step (index | 2^31)
    int n_steps, stride;
};

// phi(x) = 1/2 |L_Gamma^{-1} g - y~|^2 [+ 1/2 |L_Sigma^{-1} x + lb|^2] with g = map(x), every sum in row order
template <int P, int N>
__device__ __forceinline__ double map_phi(const MapRunProblem<P, N>& q, const double x[P], const double g[N]) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double acc = -q.yw[r];
#pragma unroll
        for (int k = 0; k <= r; ++k) acc += q.Lg[r * (r + 1) / 2 + k] * g[k];
        t += acc * acc;
    }
    if (q.prior) {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            double acc = q.lb[r];
#pragma unroll
            for (int k = 0; k <= r; ++k) acc += q.Ls[r * (r + 1) / 2 + k] * x[k];
            t += acc * acc;
        }
    }
    return 0.5 * t;
}

template <typename T, typename Map>
__global__ __launch_bounds__(MAP_THREADS)
void mh_run_map_kernel(const Map map, const MapRunProblem<Map::P, Map::N> q, const MapRunArgs a) {
    constexpr int P = Map::P, N = Map::N, NQ = (P + 3) / 4;
    const long long j = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    if (j >= a.J) return;
    // the lane's own addresses, advanced as the steps go (vector registers: the scalar ones hold the problem and the constants)
    T* __restrict__ Uj = (T*)a.U + j;
    T* __restrict__ tp = a.trace ? (T*)a.trace + j : nullptr;
    const T* __restrict__ xp = a.xi ? (const T*)a.xi + j : nullptr;
    const double* __restrict__ lp = a.logu ? a.logu + j : nullptr;
    const unsigned long long gj = (unsigned long long)(a.j_offset + j);
    double u[P];
#pragma unroll
    for (int r = 0; r < P; ++r) u[r] = (double)Uj[(size_t)r * a.J];
    double ph = a.phi[j];
    unsigned long long cnt = a.cnt[j];
    int since = 0;
    for (int k = 0; k < a.n_steps; ++k) {
        const unsigned step = a.step0 + (unsigned)k;          // (step0 carries the MH domain bit)
        // ---- propose ----
        double z[4 * NQ];
        if (xp) {
#pragma unroll
            for (int r = 0; r < P; ++r) z[r] = (double)xp[(size_t)r * a.J];
            xp += (size_t)P * a.J;
        } else {
#pragma unroll
            for (int c = 0; c < NQ; ++c)
                normal4(philox4x32_10((uint32_t)gj, (uint32_t)(gj >> 32), (uint32_t)c, step, a.seed_lo, a.seed_hi), z + 4 * c);
        }
        double x[P], g[N];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c <= r; ++c) acc += q.W[r * (r + 1) / 2 + c] * z[c];
            x[r] = q.a * u[r] + acc;
        }
        // ---- score and test (a NaN phi(P) compares false: rejected, as mh_test does) ----
        map(x, g);
        const double php = map_phi<P, N>(q, x, g);
        double lu;
        if (lp) { lu = *lp; lp += a.J; }
        else lu = mh_log_uniform(gj, step, a.seed_lo, a.seed_hi);
        if (lu < ph - php) {
#pragma unroll
            for (int r = 0; r < P; ++r) u[r] = x[r];
            ph = php;
            cnt += 1ull;
        }
        if (tp && ++since == a.stride) {
            since = 0;
#pragma unroll
            for (int r = 0; r < P; ++r) tp[(size_t)r * a.J] = (T)u[r];
            tp += (size_t)P * a.J;
        }
    }
#pragma unroll
    for (int r = 0; r < P; ++r) Uj[(size_t)r * a.J] = (T)u[r];
    a.phi[j] = ph;
    a.cnt[j] = cnt;
}

template <typename T, typename Map>
static int mh_run_map_t(Engine& e, const MapRunArgs& a, hipStream_t s) {
    constexpr int P = Map::P, N = Map::N;
    MapRunProblem<P, N> q{};
    q.a = e.mh.a;
    q.prior = e.mh.kind == CESX_MH_RW ? 1 : 0;
    // L_Gamma^{-1}: the engine's factor of a dense Gamma (y~ = h_yw is whitened with it), diag(1 / sqrt(Gamma_ii)) otherwise
    for (int r = 0; r < N; ++r) {
        double acc = 0.0;
        for (int k = 0; k <= r; ++k) {
            const double v = e.whiten ? e.h_Li[(size_t)r * N + k] : k == r ? std::sqrt(e.h_gw[r]) : 0.0;
            q.Lg[r * (r + 1) / 2 + k] = v;
            acc += v * e.h_y_raw[k];
        }
        q.yw[r] = e.whiten ? e.h_yw[r] : acc;
    }
    for (int r = 0; r < P; ++r) {
        double acc = 0.0;                  // (cesx_mh_set_proposal's lb)
        for (int k = 0; k <= r; ++k) {
            q.W[r * (r + 1) / 2 + k] = e.mh.h_bS[(size_t)r * P + k];
            q.Ls[r * (r + 1) / 2 + k] = e.h_LSi[(size_t)r * P + k];
            acc += e.h_LSi[(size_t)r * P + k] * e.h_mu[k];
        }
        q.lb[r] = -acc;
    }
    const long long blocks = (e.J + MAP_THREADS - 1) / MAP_THREADS;
    if (blocks >= (1LL << 31)) { e.err = "cesx_mh_run_map: too many chains for one launch"; return CESX_EUNSUPPORTED; }
    hipLaunchKernelGGL((mh_run_map_kernel<T, Map>), dim3((unsigned)blocks), dim3(MAP_THREADS), 0, s, Map(e.mp.desc.prm), q, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

static MapRunArgs map_run_args(Engine& e, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                               const double* logu) {
    MapRunArgs a{};
    a.U = U; a.trace = trace; a.xi = xi; a.logu = logu;
    a.phi = e.mh.phi; a.cnt = e.mh.cnt;
    a.J = e.J; a.j_offset = e.cfg.j_offset;
    a.seed_lo = (unsigned)e.cfg.seed; a.seed_hi = (unsigned)(e.cfg.seed >> 32);
    a.step0 = (unsigned)(step_index | 0x80000000ull); a.n_steps = n_steps; a.stride = stride;
    return a;
}

int launch_mh_run_map(Engine& e, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                      const double* logu, hipStream_t s) {
    const MapRunArgs a = map_run_args(e, step_index, n_steps, stride, U, trace, xi, logu);
    const bool f32 = e.cfg.dtype == CESX_F32;
    switch (e.mp.desc.kind) {
    case CESX_MAP_ELLIPTIC: return f32 ? mh_run_map_t<float, MapElliptic>(e, a, s) : mh_run_map_t<double, MapElliptic>(e, a, s);
    case CESX_MAP_BANANA: return f32 ? mh_run_map_t<float, MapBanana>(e, a, s) : mh_run_map_t<double, MapBanana>(e, a, s);
    default: e.err = "cesx_mh_run_map: the installed map has no fused kernel"; return CESX_ESTATE;
    }
}

// ---- the fused Langevin kernel ----

// The problem and the scale as lv_score (kernels_gpgrad.hip) reads them, by value: the same numbers in the same sums, so that a
// fused launch leaves the phi and g that single Langevin steps leave BIT FOR BIT on an fp64 engine -- g enters the next
// proposal, so a resume that scores the resumed states with lv_start_kernel continues a fused run exactly.  (map_phi's
// factored forms, sqrt(1 / Gamma_ii) twice and L_Sigma^{-1} x + lb, would differ from lv_score's in the last bits.)
// Triangular factors packed as in MapRunProblem; a diagonal Gamma or Sigma keeps its weights on the diagonal slots.
// P = N = 2: 13 doubles.  Which of the two forms each is (DENSE bit 0: a dense Gamma, bit 1: a dense Sigma) is a template
// parameter of the kernel: with both forms of both terms behind run-time branches the elliptic instantiation is out of scalar
// registers (1 SGPR spilled) and at 137 VGPRs (3 waves per SIMD, not 4).
template <int P, int N>
struct MapLangevinProblem {
    double S[P * (P + 1) / 2];         // the scale: P = U + S (xi - g / 2), g = S^T grad phi
    double Lg[N * (N + 1) / 2];        // dense Gamma: L_Gamma^{-1}; diagonal: 1 / Gamma_ii at (i, i)
    double y[N];                       // y, whitened for a dense Gamma
    double Ls[P * (P + 1) / 2];        // dense Sigma: L_Sigma^{-1}; diagonal: 1 / Sigma_rr at (r, r)
    double mu[P];
};

// phi(x) and gx = S^T grad phi(x) from g = map(x) and DG: lv_score in mode CESX_GP_GAMMA, statement by statement
template <int P, int N, int DENSE>
__device__ __forceinline__ double map_lv_score(const MapLangevinProblem<P, N>& q, const double x[P], const double g[N],
                                               const double DG[N][P], double gx[P]) {
    double s = 0.0, ca[N], gphi[P];
    if (DENSE & 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double w = 0.0;
#pragma unroll
            for (int k = 0; k <= i; ++k) w = fma(q.Lg[i * (i + 1) / 2 + k], g[k], w);
            const double d = w - q.y[i];
            s = fma(d, d, s);
            ca[i] = d;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int i = k; i < N; ++i) acc = fma(q.Lg[i * (i + 1) / 2 + k], ca[i], acc);
            ca[k] = acc;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double gw = q.Lg[i * (i + 1) / 2 + i];
            const double d = g[i] - q.y[i];
            s = fma(gw, d * d, s);
            ca[i] = gw * d;
        }
    }
    if (DENSE & 2) {
        double w[P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k <= r; ++k) acc = fma(q.Ls[r * (r + 1) / 2 + k], x[k] - q.mu[k], acc);
            s = fma(acc, acc, s);
            w[r] = acc;
        }
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int r = c; r < P; ++r) acc = fma(q.Ls[r * (r + 1) / 2 + c], w[r], acc);
            gphi[c] = acc;
        }
    } else {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const double sw = q.Ls[r * (r + 1) / 2 + r];
            const double d = x[r] - q.mu[r];
            s = fma(sw, d * d, s);
            gphi[r] = sw * d;
        }
    }
#pragma unroll
    for (int c = 0; c < P; ++c) {
        double acc = gphi[c];
#pragma unroll
        for (int i = 0; i < N; ++i) acc = fma(ca[i], DG[i][c], acc);
        gphi[c] = acc;
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int c = r; c < P; ++c) acc = fma(q.S[c * (c + 1) / 2 + r], gphi[c], acc);
        gx[r] = acc;
    }
    return 0.5 * s;
}

template <typename T, typename Map, int DENSE>
__global__ __launch_bounds__(MAP_THREADS)
void mh_langevin_map_kernel(const Map map, const MapLangevinProblem<Map::P, Map::N> q, const MapRunArgs a, double* __restrict__ lv_g) {
    constexpr int P = Map::P, N = Map::N, NQ = (P + 3) / 4;
    const long long j = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    if (j >= a.J) return;
    // the lane's own addresses in vector registers, as in mh_run_map_kernel
    T* __restrict__ Uj = (T*)a.U + j;
    double* __restrict__ gj_p = lv_g + j;
    T* __restrict__ tp = a.trace ? (T*)a.trace + j : nullptr;
    const T* __restrict__ xp = a.xi ? (const T*)a.xi + j : nullptr;
    const double* __restrict__ lp = a.logu ? a.logu + j : nullptr;
    const unsigned long long gj = (unsigned long long)(a.j_offset + j);
    double u[P], gu[P];
#pragma unroll
    for (int r = 0; r < P; ++r) { u[r] = (double)Uj[(size_t)r * a.J]; gu[r] = gj_p[(size_t)r * a.J]; }
    double ph = a.phi[j];
    unsigned long long cnt = a.cnt[j];
    int since = 0;
    for (int k = 0; k < a.n_steps; ++k) {
        const unsigned step = a.step0 + (unsigned)k;          // (step0 carries the MH domain bit)
        // ---- propose: P = U + S (xi - g(U) / 2), lv_propose_kernel's sums ----
        double z[4 * NQ];
        if (xp) {
#pragma unroll
            for (int r = 0; r < P; ++r) z[r] = (double)xp[(size_t)r * a.J];
            xp += (size_t)P * a.J;
        } else {
#pragma unroll
            for (int c = 0; c < NQ; ++c)
                normal4(philox4x32_10((uint32_t)gj, (uint32_t)(gj >> 32), (uint32_t)c, step, a.seed_lo, a.seed_hi), z + 4 * c);
        }
        double x[P], g[N], DG[N][P], gx[P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c <= r; ++c) acc = fma(q.S[r * (r + 1) / 2 + c], z[c] - 0.5 * gu[c], acc);
            x[r] = u[r] + acc;
        }
        // ---- score and test (any NaN compares false: rejected, as lv_accept_kernel does) ----
        map.map_jac(x, g, DG);
        const double php = map_lv_score<P, N, DENSE>(q, x, g, DG, gx);
        double n1 = 0.0, n2 = 0.0;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const double d = z[r] - 0.5 * (gu[r] + gx[r]);
            n1 = fma(z[r], z[r], n1);
            n2 = fma(d, d, n2);
        }
        double lu;
        if (lp) { lu = *lp; lp += a.J; }
        else lu = mh_log_uniform(gj, step, a.seed_lo, a.seed_hi);
        if (lu < ph - php + (0.5 * n1 - 0.5 * n2)) {
#pragma unroll
            for (int r = 0; r < P; ++r) { u[r] = x[r]; gu[r] = gx[r]; }
            ph = php;
            cnt += 1ull;
        }
        if (tp && ++since == a.stride) {
            since = 0;
#pragma unroll
            for (int r = 0; r < P; ++r) tp[(size_t)r * a.J] = (T)u[r];
            tp += (size_t)P * a.J;
        }
    }
#pragma unroll
    for (int r = 0; r < P; ++r) { Uj[(size_t)r * a.J] = (T)u[r]; gj_p[(size_t)r * a.J] = gu[r]; }
    a.phi[j] = ph;
    a.cnt[j] = cnt;
}

template <typename T, typename Map>
static int mh_langevin_map_t(Engine& e, const MapRunArgs& a, hipStream_t s) {
    constexpr int P = Map::P, N = Map::N;
    MapLangevinProblem<P, N> q{};
    for (int r = 0; r < N; ++r) {
        for (int k = 0; k <= r; ++k) q.Lg[r * (r + 1) / 2 + k] = e.whiten ? e.h_Li[(size_t)r * N + k] : k == r ? e.h_gw[r] : 0.0;
        q.y[r] = e.h_yw[r];
    }
    for (int r = 0; r < P; ++r) {
        for (int k = 0; k <= r; ++k) {
            q.S[r * (r + 1) / 2 + k] = e.mh.h_bS[(size_t)r * P + k];
            q.Ls[r * (r + 1) / 2 + k] = e.diag_sigma ? (k == r ? e.h_sw[r] : 0.0) : e.h_LSi[(size_t)r * P + k];
        }
        q.mu[r] = e.h_mu[r];
    }
    const long long blocks = (e.J + MAP_THREADS - 1) / MAP_THREADS;
    if (blocks >= (1LL << 31)) { e.err = "cesx_mh_langevin_run_map: too many chains for one launch"; return CESX_EUNSUPPORTED; }
    double* lv_g = e.mh.lv_g.get();
    auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(MAP_THREADS), 0, s, Map(e.mp.desc.prm), q, a, lv_g); };
    switch ((e.whiten ? 1 : 0) | (e.diag_sigma ? 0 : 2)) {
    case 0: launch(mh_langevin_map_kernel<T, Map, 0>); break;
    case 1: launch(mh_langevin_map_kernel<T, Map, 1>); break;
    case 2: launch(mh_langevin_map_kernel<T, Map, 2>); break;
    default: launch(mh_langevin_map_kernel<T, Map, 3>); break;
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_mh_langevin_run_map(Engine& e, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                               const double* logu, hipStream_t s) {
    const MapRunArgs a = map_run_args(e, step_index, n_steps, stride, U, trace, xi, logu);
    const bool f32 = e.cfg.dtype == CESX_F32;
    switch (e.mp.desc.kind) {
    case CESX_MAP_ELLIPTIC: return f32 ? mh_langevin_map_t<float, MapElliptic>(e, a, s) : mh_langevin_map_t<double, MapElliptic>(e, a, s);
    case CESX_MAP_BANANA: return f32 ? mh_langevin_map_t<float, MapBanana>(e, a, s) : mh_langevin_map_t<double, MapBanana>(e, a, s);
    default: e.err = "cesx_mh_langevin_run_map: the installed map has no fused kernel"; return CESX_ESTATE;
    }
}

// ---- the fused HMC kernel ----

// mh_langevin_map_kernel with the leapfrog loop inside (include/cesx.h, cesx_mh_hmc_run_map): per step the lane draws xi, forms
// r = xi - g(U) / 2 and walks `leapfrog` positions x = x + S r, scoring each with map_lv_score and kicking r by g(x) (by
// g(x) / 2 at the last), then tests log u < phi(U) - phi(x) + (|xi|^2 / 2 - |r|^2 / 2).  The sums are the hm_* kernels'
// (kernels_hmc.hip) in their order, so on an fp64 engine the launch leaves the step path's U, phi and g bit for bit; the chain,
// phi, g, r, xi's norm and the Jacobian stay in the lane's registers, and the trajectory is fp64 whatever the engine dtype
// (the step path of an fp32 engine rounds Q after every leapfrog; this kernel rounds on the stores alone).
template <typename T, typename Map, int DENSE>
__global__ __launch_bounds__(MAP_THREADS)
void mh_hmc_map_kernel(const Map map, const MapLangevinProblem<Map::P, Map::N> q, const MapRunArgs a, double* __restrict__ lv_g,
                       const int leapfrog) {
    constexpr int P = Map::P, N = Map::N, NQ = (P + 3) / 4;
    const long long j = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    if (j >= a.J) return;
    // the lane's own addresses in vector registers, as in mh_run_map_kernel
    T* __restrict__ Uj = (T*)a.U + j;
    double* __restrict__ gj_p = lv_g + j;
    T* __restrict__ tp = a.trace ? (T*)a.trace + j : nullptr;
    const T* __restrict__ xp = a.xi ? (const T*)a.xi + j : nullptr;
    const double* __restrict__ lp = a.logu ? a.logu + j : nullptr;
    const unsigned long long gj = (unsigned long long)(a.j_offset + j);
    double u[P], gu[P];
#pragma unroll
    for (int r = 0; r < P; ++r) { u[r] = (double)Uj[(size_t)r * a.J]; gu[r] = gj_p[(size_t)r * a.J]; }
    double ph = a.phi[j];
    unsigned long long cnt = a.cnt[j];
    int since = 0;
    for (int k = 0; k < a.n_steps; ++k) {
        const unsigned step = a.step0 + (unsigned)k;          // (step0 carries the MH domain bit): ONE step index whatever leapfrog is
        double x[P], rm[P], gx[P], n1 = 0.0;
        {   // ---- begin: r = xi - g(U) / 2 and |xi|^2, hm_begin_kernel's and hm_accept_kernel's sums ----
            double z[4 * NQ];
            if (xp) {
#pragma unroll
                for (int r = 0; r < P; ++r) z[r] = (double)xp[(size_t)r * a.J];
                xp += (size_t)P * a.J;
            } else {
#pragma unroll
                for (int c = 0; c < NQ; ++c)
                    normal4(philox4x32_10((uint32_t)gj, (uint32_t)(gj >> 32), (uint32_t)c, step, a.seed_lo, a.seed_hi), z + 4 * c);
            }
#pragma unroll
            for (int r = 0; r < P; ++r) { rm[r] = z[r] - 0.5 * gu[r]; n1 = fma(z[r], z[r], n1); x[r] = u[r]; }
        }
        // ---- the trajectory (any NaN or infinity ends in a false comparison, as on the step path) ----
        double php = 0.0;
        for (int l = 1; l <= leapfrog; ++l) {
#pragma unroll
            for (int r = 0; r < P; ++r) {
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c <= r; ++c) acc = fma(q.S[r * (r + 1) / 2 + c], rm[c], acc);
                x[r] = x[r] + acc;
            }
            double g[N], DG[N][P];
            map.map_jac(x, g, DG);
            php = map_lv_score<P, N, DENSE>(q, x, g, DG, gx);
            if (l < leapfrog) {
#pragma unroll
                for (int r = 0; r < P; ++r) rm[r] = rm[r] - gx[r];
                if (!(php - php == 0.0)) rm[0] = __builtin_nan("");
            }
        }
        double n2 = 0.0;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const double d = rm[r] - 0.5 * gx[r];
            n2 = fma(d, d, n2);
        }
        double lu;
        if (lp) { lu = *lp; lp += a.J; }
        else lu = mh_log_uniform(gj, step, a.seed_lo, a.seed_hi);
        if (lu < ph - php + (0.5 * n1 - 0.5 * n2)) {
#pragma unroll
            for (int r = 0; r < P; ++r) { u[r] = x[r]; gu[r] = gx[r]; }
            ph = php;
            cnt += 1ull;
        }
        if (tp && ++since == a.stride) {
            since = 0;
#pragma unroll
            for (int r = 0; r < P; ++r) tp[(size_t)r * a.J] = (T)u[r];
            tp += (size_t)P * a.J;
        }
    }
#pragma unroll
    for (int r = 0; r < P; ++r) { Uj[(size_t)r * a.J] = (T)u[r]; gj_p[(size_t)r * a.J] = gu[r]; }
    a.phi[j] = ph;
    a.cnt[j] = cnt;
}

template <typename T, typename Map>
static int mh_hmc_map_t(Engine& e, const MapRunArgs& a, int leapfrog, hipStream_t s) {
    constexpr int P = Map::P, N = Map::N;
    MapLangevinProblem<P, N> q{};                   // (filled as mh_langevin_map_t fills it: lv_score's numbers)
    for (int r = 0; r < N; ++r) {
        for (int k = 0; k <= r; ++k) q.Lg[r * (r + 1) / 2 + k] = e.whiten ? e.h_Li[(size_t)r * N + k] : k == r ? e.h_gw[r] : 0.0;
        q.y[r] = e.h_yw[r];
    }
    for (int r = 0; r < P; ++r) {
        for (int k = 0; k <= r; ++k) {
            q.S[r * (r + 1) / 2 + k] = e.mh.h_bS[(size_t)r * P + k];
            q.Ls[r * (r + 1) / 2 + k] = e.diag_sigma ? (k == r ? e.h_sw[r] : 0.0) : e.h_LSi[(size_t)r * P + k];
        }
        q.mu[r] = e.h_mu[r];
    }
    const long long blocks = (e.J + MAP_THREADS - 1) / MAP_THREADS;
    if (blocks >= (1LL << 31)) { e.err = "cesx_mh_hmc_run_map: too many chains for one launch"; return CESX_EUNSUPPORTED; }
    double* lv_g = e.mh.lv_g.get();
    auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(MAP_THREADS), 0, s, Map(e.mp.desc.prm), q, a, lv_g, leapfrog); };
    switch ((e.whiten ? 1 : 0) | (e.diag_sigma ? 0 : 2)) {
    case 0: launch(mh_hmc_map_kernel<T, Map, 0>); break;
    case 1: launch(mh_hmc_map_kernel<T, Map, 1>); break;
    case 2: launch(mh_hmc_map_kernel<T, Map, 2>); break;
    default: launch(mh_hmc_map_kernel<T, Map, 3>); break;
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_mh_hmc_run_map(Engine& e, uint64_t step_index, int n_steps, int leapfrog, int stride, void* U, void* trace,
                          const void* xi, const double* logu, hipStream_t s) {
    const MapRunArgs a = map_run_args(e, step_index, n_steps, stride, U, trace, xi, logu);
    const bool f32 = e.cfg.dtype == CESX_F32;
    switch (e.mp.desc.kind) {
    case CESX_MAP_ELLIPTIC: return f32 ? mh_hmc_map_t<float, MapElliptic>(e, a, leapfrog, s) : mh_hmc_map_t<double, MapElliptic>(e, a, leapfrog, s);
    case CESX_MAP_BANANA: return f32 ? mh_hmc_map_t<float, MapBanana>(e, a, leapfrog, s) : mh_hmc_map_t<double, MapBanana>(e, a, leapfrog, s);
    default: e.err = "cesx_mh_hmc_run_map: the installed map has no fused kernel"; return CESX_ESTATE;
    }
}

}  // namespace cesx
