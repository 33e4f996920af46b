// The Langevin and leapfrog steps of MCMC.model_mh(chains=M, update='langevin' / 'hmc') for a map whose gradient of the data
// misfit arrives READY-MADE (include/cesx.h, cesx_mh_grad_source with CESX_MH_GRAD_READY): G [n][M] and d = d phi_d / du [p][M]
// of cesx_darcy_grad stand where the lv_* / hm_* kernels (kernels_gpgrad.hip, kernels_hmc.hip) take G and the [n][p][M] Jacobian
// image.  The four kernels are what cesx_mh_langevin_start / _accept and cesx_mh_hmc_leap / _accept launch under that source;
// cesx_mh_langevin_propose and cesx_mh_hmc_begin read the chains' g alone and stay lv_propose_kernel / hm_begin_kernel.
//
// Arithmetic: lv_score's mode CESX_GP_GAMMA (lv_score.h) term for term and in its order, but
//     grad phi[q] = prior[q] + d[q]
// where lv_score sums a_i dG_i / du_q on top of prior[q]; the kick, the two norms, the test, the NaN rule and the masked copies
// are lv_accept_kernel's and hm_*_kernel<ADAPT>'s expressions in their row order.  All of it is fp64 whatever the engine dtype.
//
// Grid: ONE WAVE PER CHAIN (a workgroup of 64 lanes, darcy_grad_kernel's grid), not lv_score's one thread per chain.  A Darcy run
// has few, expensive chains: at M = 1 024 one thread per chain is four workgroups, and a chain's two triangular products with S
// and its dense prior's two are p^2 dependent FMAs in one lane.  Here the ROWS of a triangular product go across the lanes -- a
// row's inner sum still runs in lv_score's index order, so the row is the same bits -- and the depth is p^2 / 64:
//     forward products (L v: L_Sigma^{-1} (x - mu), L_Gamma^{-1} G, S r)   a 64 x 16 tile of L is staged in LDS by row reads
//                       (16 lanes contiguous on a row), then lane l sums row l of the tile over k ascending
//     transposed products (L^T v: the prior's second loop, S^T grad phi)   lane l owns column l and walks the rows downwards: row
//                       r of L is read along the row, lanes contiguous
//     scalar sums (s, |xi|^2, |r|^2)                                        the addends go to LDS and EVERY lane sums them in
//                       ascending order (broadcast reads): one fixed order whatever p is, no butterfly, and the sum is in every lane
// No atomics, plain stores only: two runs are bit-identical.  The p-vectors of a chain (strided by M in memory) are loaded into
// LDS once and written back once; n_obs is streamed through 64-entry chunks.  p <= DC_PMAX = 256 (what a Darcy descriptor
// allows: p <= K^2 <= 256; cesx_mh_grad_source refuses a larger engine), n_obs is not bounded.
#include "cesx_internal.h"

namespace cesx {

constexpr int DC_PMAX = 256;
constexpr int DC_W = 64;                   // lanes of the one wave
constexpr int DC_KT = 16;                  // columns of a staged tile: 64 rows x 16 columns, 128-byte row pieces
constexpr int DC_LD = DC_KT + 1;           // tile rows padded by one double: lane l reads row l, 32 lanes on 32 bank pairs

template <typename T>
struct DcArgs {
    const double *G, *d;                   // [n][M] the map, [p][M] the data term of grad phi, at X
    int n, p; long long M;
    const double *y, *gw, *Lg;             // y (whitened when Lg != nullptr), 1 / Gamma_ii, L_Gamma^{-1}
    const T* X; const double *mu, *sw, *LSi;
    const double* S;                       // [p][p] the lower-triangular scale
    double* gu;                            // [p][M] g = S^T grad phi of the chains' states (mh.lv_g)
    const T* xi;                           // [p][M] the step's noise block
    T *U, *P;                              // accept: the chains' states; leap: the position, advanced in place
    MhChains c;
    double* r;                             // [p][M] the momentum (mh.hm_r)
    const double* e;                       // ADAPT: the step multiplier (mh.ad_state[0])
    double* alpha;                         // ADAPT: [M] the chains' acceptance probabilities of this step
};

struct DcLds {
    double x[DC_PMAX];                     // X of the chain, as doubles
    double w[DC_PMAX], v[DC_PMAX];         // the prior's w and addends; then xi and the momentum
    double gphi[DC_PMAX], g[DC_PMAX];      // d, then grad phi; g = S^T grad phi
    double tile[DC_W * DC_LD];             // 64 rows x 16 columns of a forward product's matrix
    double c1[DC_W], c2[DC_W];             // a chunk of a streamed vector / of a scalar sum's addends
};

// rows r0 .. r0 + 63 of L v, L [m][m] lower triangular and row-major, v through vec(k): lane l returns row r0 + l (0 past m), its
// sum over k = 0 .. row ascending.  r0 is a multiple of 64; every lane of the wave calls it
template <typename V>
__device__ __forceinline__ double dc_forward(const double* L, int m, int r0, V vec, DcLds& s, int lane) {
    const int row = r0 + lane;
    const int rn = min(DC_W, m - r0);
    double acc = 0.0;
    const int kend = min(r0 + DC_W, m);                              // (the chunk's last row ends at column kend - 1)
    const int c = lane & (DC_KT - 1);
    for (int k0 = 0; k0 < kend; k0 += DC_KT) {
        const int kn = min(DC_KT, m - k0);
        __syncthreads();                                             // (the tile and the chunk of the last round are read)
        for (int rr = lane / DC_KT; rr < rn; rr += DC_W / DC_KT) s.tile[rr * DC_LD + c] = c < kn ? L[(size_t)(r0 + rr) * m + k0 + c] : 0.0;
        if (lane < DC_KT) s.c1[lane] = lane < kn ? vec(k0 + lane) : 0.0;
        __syncthreads();
        if (row < m) {
            const int ke = min(kn, row - k0 + 1);                    // (<= 0: the row ended before this tile)
            for (int kk = 0; kk < ke; ++kk) acc = fma(s.tile[lane * DC_LD + kk], s.c1[kk], acc);
        }
    }
    return acc;
}

// columns c0 .. c0 + 63 of L^T v, v [m] in LDS: lane l returns column c0 + l (0 past m), its sum over r = col .. m - 1 ascending
__device__ __forceinline__ double dc_transposed(const double* L, int m, int c0, const double* v, int lane) {
    const int col = c0 + lane;
    double acc = 0.0;
    for (int r = c0; r < m; ++r)
        if (col <= r) acc = fma(L[(size_t)r * m + col], v[r], acc);
    return acc;
}

// phi of chain j at X = a.X (lv_score's sums in its order) and g = S^T grad phi into s.g; s.x keeps X.  The value is in every lane
template <typename T>
__device__ __forceinline__ double dc_score(const DcArgs<T>& a, long long j, DcLds& s, int lane) {
    const int n = a.n, p = a.p;
    const size_t M = (size_t)a.M;
    for (int r = lane; r < p; r += DC_W) {
        s.x[r] = (double)a.X[r * M + j];
        s.gphi[r] = a.d[r * M + j];
    }
    double sum = 0.0;
    if (a.Lg) {
        for (int i0 = 0; i0 < n; i0 += DC_W) {
            const double w = dc_forward(a.Lg, n, i0, [&](int k) { return a.G[k * M + j]; }, s, lane);
            s.c2[lane] = i0 + lane < n ? w - a.y[i0 + lane] : 0.0;
            __syncthreads();
            const int in = min(DC_W, n - i0);
            for (int ii = 0; ii < in; ++ii) sum = fma(s.c2[ii], s.c2[ii], sum);
        }
        // (a = L_Gamma^{-T} d of lv_score weighs the Jacobian's rows: the ready-made gradient has them summed)
    } else {
        for (int i0 = 0; i0 < n; i0 += DC_W) {
            const int i = i0 + lane;
            __syncthreads();                                         // (the last chunk is summed)
            if (i < n) {
                const double d = a.G[i * M + j] - a.y[i];
                s.c1[lane] = a.gw[i];
                s.c2[lane] = d * d;
            }
            __syncthreads();
            const int in = min(DC_W, n - i0);
            for (int ii = 0; ii < in; ++ii) sum = fma(s.c1[ii], s.c2[ii], sum);
        }
    }
    __syncthreads();                                                 // (s.x and s.gphi are written)
    if (a.LSi) {
        for (int r0 = 0; r0 < p; r0 += DC_W) {
            const double w = dc_forward(a.LSi, p, r0, [&](int k) { return s.x[k] - a.mu[k]; }, s, lane);
            if (r0 + lane < p) s.w[r0 + lane] = w;
        }
        __syncthreads();
        for (int r = 0; r < p; ++r) sum = fma(s.w[r], s.w[r], sum);
        for (int q0 = 0; q0 < p; q0 += DC_W) {
            const double acc = dc_transposed(a.LSi, p, q0, s.w, lane);
            if (q0 + lane < p) s.gphi[q0 + lane] = __dadd_rn(acc, s.gphi[q0 + lane]);
        }
    } else {
        for (int r = lane; r < p; r += DC_W) {
            const double d = s.x[r] - a.mu[r];
            s.w[r] = a.sw[r];
            s.v[r] = d * d;
            s.gphi[r] = __dadd_rn(__dmul_rn(a.sw[r], d), s.gphi[r]);
        }
        __syncthreads();
        for (int r = 0; r < p; ++r) sum = fma(s.w[r], s.v[r], sum);
    }
    __syncthreads();                                                 // (every grad phi is in LDS)
    for (int r0 = 0; r0 < p; r0 += DC_W) {
        const double acc = dc_transposed(a.S, p, r0, s.gphi, lane);
        if (r0 + lane < p) s.g[r0 + lane] = acc;
    }
    __syncthreads();
    return 0.5 * sum;
}

// phi and g of the start states: lv_start_kernel
template <typename T>
__global__ __launch_bounds__(DC_W)
void dc_start_kernel(const DcArgs<T> a) {
    __shared__ DcLds s;
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;
    const size_t M = (size_t)a.M;
    const double ph = dc_score(a, j, s, lane);
    if (lane == 0) {
        a.c.phi[j] = ph;
        a.c.cnt[j] = 0ull;
    }
    for (int r = lane; r < a.p; r += DC_W) a.gu[r * M + j] = s.g[r];
}

// phi(P), g(P), the two norms and the test of lv_accept_kernel; an accepted chain takes P, phi and g
template <typename T>
__global__ __launch_bounds__(DC_W)
void dc_lv_accept_kernel(const DcArgs<T> a) {
    __shared__ DcLds s;
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    const double phu = a.c.phi[j];
    const double ph = dc_score(a, j, s, lane);
    for (int r = lane; r < p; r += DC_W) {
        const double x = (double)a.xi[r * M + j];
        s.w[r] = x;
        s.v[r] = x - 0.5 * (a.gu[r * M + j] + s.g[r]);
    }
    __syncthreads();
    double n1 = 0.0, n2 = 0.0;
    for (int r = 0; r < p; ++r) {
        n1 = fma(s.w[r], s.w[r], n1);
        n2 = fma(s.v[r], s.v[r], n2);
    }
    const double lu = a.c.logu ? a.c.logu[j] : mh_log_uniform((unsigned long long)(a.c.j_offset + j), a.c.step, a.c.seed_lo, a.c.seed_hi);
    if (lu < phu - ph + (0.5 * n1 - 0.5 * n2)) {
        if (lane == 0) {
            a.c.phi[j] = ph;
            a.c.cnt[j] += 1ull;
        }
        for (int r = lane; r < p; r += DC_W) {
            a.U[r * M + j] = (T)s.x[r];
            a.gu[r * M + j] = s.g[r];
        }
    }
}

// phi(Q) and g(Q), the full kick r = r - g(Q), the next position Q = Q + S r in place: hm_leap_kernel
template <typename T, bool ADAPT>
__global__ __launch_bounds__(DC_W)
void dc_hm_leap_kernel(const DcArgs<T> a) {
    __shared__ DcLds s;
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    const double ph = dc_score(a, j, s, lane);
    double e = 1.0;
    if constexpr (ADAPT) e = *a.e;
    for (int r = lane; r < p; r += DC_W) {
        double rv;
        if constexpr (ADAPT) rv = a.r[r * M + j] - e * s.g[r];
        else rv = a.r[r * M + j] - s.g[r];
        if (r == 0 && !(ph - ph == 0.0)) rv = __builtin_nan("");     // (an infinite or NaN phi whose g is finite all the same)
        s.v[r] = rv;
        a.r[r * M + j] = rv;
    }
    for (int s0 = 0; s0 < p; s0 += DC_W) {                           // (dc_forward synchronises before it reads s.v)
        const double acc = dc_forward(a.S, p, s0, [&](int k) { return s.v[k]; }, s, lane);
        const int row = s0 + lane;
        if (row < p) {
            if constexpr (ADAPT) a.P[row * M + j] = (T)(s.x[row] + e * acc);
            else a.P[row * M + j] = (T)(s.x[row] + acc);
        }
    }
}

// phi(Q) and g(Q) at the last position, the half kick, the two norms and the test: hm_accept_kernel
template <typename T, bool ADAPT>
__global__ __launch_bounds__(DC_W)
void dc_hm_accept_kernel(const DcArgs<T> a) {
    __shared__ DcLds s;
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    const double phu = a.c.phi[j];
    const double ph = dc_score(a, j, s, lane);
    double he = 0.5;
    if constexpr (ADAPT) he = 0.5 * *a.e;
    for (int r = lane; r < p; r += DC_W) {
        s.w[r] = (double)a.xi[r * M + j];
        if constexpr (ADAPT) s.v[r] = a.r[r * M + j] - he * s.g[r];
        else s.v[r] = a.r[r * M + j] - 0.5 * s.g[r];
    }
    __syncthreads();
    double n1 = 0.0, n2 = 0.0;
    for (int r = 0; r < p; ++r) {
        n1 = fma(s.w[r], s.w[r], n1);
        n2 = fma(s.v[r], s.v[r], n2);
    }
    const double lu = a.c.logu ? a.c.logu[j] : mh_log_uniform((unsigned long long)(a.c.j_offset + j), a.c.step, a.c.seed_lo, a.c.seed_hi);
    const double d = phu - ph + (0.5 * n1 - 0.5 * n2);
    if constexpr (ADAPT) {
        if (lane == 0) a.alpha[j] = d >= 0.0 ? 1.0 : d < 0.0 ? exp(d) : 0.0;      // (NaN: neither comparison holds)
    }
    if (lu < d) {
        if (lane == 0) {
            a.c.phi[j] = ph;
            a.c.cnt[j] += 1ull;
        }
        for (int r = lane; r < p; r += DC_W) {
            a.U[r * M + j] = (T)s.x[r];
            a.gu[r * M + j] = s.g[r];
        }
    }
}

template <typename T>
static int dc_t(Engine& e, int what, const void* X, const double* G, const double* d, void* U, const double* logu, unsigned step,
                hipStream_t s) {
    if (e.p > DC_PMAX || e.J >= (1LL << 31)) { e.err = "cesx_mh_grad_source: CESX_MH_GRAD_READY serves p <= 256 and J_local < 2^31"; return CESX_EUNSUPPORTED; }
    DcArgs<T> a{};
    a.G = G; a.d = d; a.n = e.n; a.p = e.p; a.M = e.J;
    a.y = e.d_y; a.gw = e.d_gw; a.Lg = e.whiten ? e.d_Wh : nullptr;
    a.X = (const T*)X; a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get();
    a.S = e.mh.bS;
    a.gu = e.mh.lv_g;
    a.xi = (const T*)e.mh.xi.get(); a.U = (T*)U; a.P = (T*)const_cast<void*>(X);
    a.c = mh_chains(e, what == 0, logu, step);
    a.r = e.mh.hm_r;
    const bool armed = e.mh.ad_armed && what >= 2;                   // cesx_mh_adapt_set: the step at e S, alpha for ad_update_kernel
    if (armed) { a.e = e.mh.ad_state.get(); a.alpha = e.mh.ad_alpha.get(); }
    const dim3 grid((unsigned)e.J), block(DC_W);
    if (what == 0) hipLaunchKernelGGL((dc_start_kernel<T>), grid, block, 0, s, a);
    else if (what == 1) hipLaunchKernelGGL((dc_lv_accept_kernel<T>), grid, block, 0, s, a);
    else if (what == 2 && armed) hipLaunchKernelGGL((dc_hm_leap_kernel<T, true>), grid, block, 0, s, a);
    else if (what == 2) hipLaunchKernelGGL((dc_hm_leap_kernel<T, false>), grid, block, 0, s, a);
    else if (armed) hipLaunchKernelGGL((dc_hm_accept_kernel<T, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dc_hm_accept_kernel<T, false>), grid, block, 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

// what: 0 start (phi and g of the states X), 1 the Langevin accept (X = the proposal; U takes the accepted columns), 2 leap (X = Q,
// advanced in place), 3 the leapfrog accept (X = the last Q); G and d = cesx_darcy_grad's G_dev and dphi_dev at X
int launch_darcy_chain(Engine& e, int what, const void* X, const double* G, const double* d, void* U, const double* logu,
                       unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? dc_t<float>(e, what, X, G, d, U, logu, step, s) : dc_t<double>(e, what, X, G, d, U, logu, step, s);
}

}  // namespace cesx
