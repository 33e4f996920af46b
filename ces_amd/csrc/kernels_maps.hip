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
};
struct MapBanana {
    static constexpr int P = 2, N = 2;
    double a, b;
    __host__ explicit MapBanana(const double* prm) : a(prm[0]), b(prm[1]) {}
    __device__ __forceinline__ void operator()(const double u[2], double g[2]) const {
        g[0] = u[0] * a;                   // ces/utils.py:120-121
        g[1] = u[1] / a - b * (u[0] * u[0] + a * a);
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

// ---- the fused chain kernel ----

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

int launch_mh_run_map(Engine& e, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                      const double* logu, hipStream_t s) {
    MapRunArgs a{};
    a.U = U; a.trace = trace; a.xi = xi; a.logu = logu;
    a.phi = e.mh.phi; a.cnt = e.mh.cnt;
    a.J = e.J; a.j_offset = e.cfg.j_offset;
    a.seed_lo = (unsigned)e.cfg.seed; a.seed_hi = (unsigned)(e.cfg.seed >> 32);
    a.step0 = (unsigned)(step_index | 0x80000000ull); a.n_steps = n_steps; a.stride = stride;
    const bool f32 = e.cfg.dtype == CESX_F32;
    switch (e.mp.desc.kind) {
    case CESX_MAP_ELLIPTIC: return f32 ? mh_run_map_t<float, MapElliptic>(e, a, s) : mh_run_map_t<double, MapElliptic>(e, a, s);
    case CESX_MAP_BANANA: return f32 ? mh_run_map_t<float, MapBanana>(e, a, s) : mh_run_map_t<double, MapBanana>(e, a, s);
    default: e.err = "cesx_mh_run_map: the installed map has no fused kernel"; return CESX_ESTATE;
    }
}

}  // namespace cesx
