// The gradients of the GP emulator over the columns of the (p, J) layout, and the preconditioned Metropolis-adjusted
// Langevin step of MCMC.gp_mh(chains=M, update='langevin') that uses them (include/cesx.h, cesx_gp_predict_grad and
// cesx_gp_langevin_*).  All arithmetic is fp64 whatever the engine dtype.
//
// gp_grad_kernel: the tile of gp_predict_kernel -- one workgroup per (GP i, tile of GP_T = 32 chains), 8 waves -- and its
// first three phases restated: they MUST stay in step with kernels_gp.hip:64-136 and gp_kern (kernels_gp.hip:40-46), the same
// products in the same order, because mean and var of this launch equal cesx_gp_predict's bit for bit.  With
// h(r) = f'(r) / r and dk_t = sigma^2 h(r_t) (z - Z_t):
//     1-3. z, K* (panel P0), mean, W = L^{-1} K* on the matrix pipe, var -- and W kept (panel P1)
//     4.   beta = L^{-T} W                      (v_mfma_f64_16x16x4_f64 again: A = the blocks of the same packed L^{-1} image
//                                                read transposed, B = W from P1; beta over K* in P0, which is dead by now)
//     5.   cm_t = alpha_t sigma^2 h(r_t) (over W in P1), cv_t = beta_t sigma^2 h(r_t) (in place in P0), then row by row of z
//              d mean / dz_r = sum_t cm_t (z_r - Z_tr) + w_r,      d var / dz_r = -2 sum_t cv_t (z_r - Z_tr)
//          on the vector ALU: 16 thread groups take every 16th t in increasing order, their partials are summed in group
//          order through LDS -- fixed orders, no atomics: runs are bit-identical
//     6.   d / dx = A_i^T d / dz                (A_i lower triangular; rows summed in increasing order)
// The mean-only mode (var and dvar NULL) has no triangular product at all: one panel, cm over K*.
// A tile holds z [p][32], the two z-gradients [2 p][32] and the panels [J_p][32] each: (2 J_p + 3 p) 256 bytes (J_p + 3 p in
// the mean-only mode) next to the 8 KiB partial-sum buffer.  Up to 2 J_p + 3 p <= 608 that is LDS; beyond it the tile lives in
// the global workspace of gp_predict_kernel<T, false>, one slot per workgroup, and the (GP, tile) pairs go in as many launches
// as the slots need (a loop over tiles inside the kernel keeps the launch's scalars live around it: they spill).
//
// lv_* kernels: one thread per chain, like gp_score_kernel.  lv_score forms phi (gp_score_kernel's terms in its order) and
// g = S^T grad phi from the GP rows and their gradients; the vectors a chain needs in between live in engine memory
// ([n][J] and [p][J] fp64 rows, coalesced over the chains), so p and n are not bounded by registers.
#include "cesx_internal.h"
#include "lv_score.h"

namespace cesx {

constexpr int GP_T = 32;                  // chains per tile (two 16-column MFMA groups)
constexpr int GP_NW = 8;                   // waves per workgroup
constexpr int GP_THREADS = GP_NW * 64;
constexpr int GP_NG = GP_THREADS / GP_T;   // thread groups of one chain column each
constexpr int GP_RED = GP_NW * 4 * GP_T;   // doubles of the partial-sum buffer (= 2 GP_NG GP_T: both gradients' partials)
constexpr size_t GP_LDS_MAX = 160 * 1024 - GP_RED * 8;
using gp_d4 = double __attribute__((ext_vector_type(4)));

template <typename T>
struct GpGradArgs {
    const T* X; long long M; int p;
    int Jt, Jp; size_t li_len;
    const double *A, *c, *Z, *par, *mw, *alpha, *Li;
    double *mean, *var, *dmean, *dvar; int nugget;
    double* ws; size_t slot;               // nullptr: the tile in LDS; else doubles per workgroup slot
    int ntiles, w0;                        // tiles per GP; the first (GP, tile) pair of this launch
};

// sigma^2 f(r): gp_kern of kernels_gp.hip, restated (a __device__ function is private to its translation unit)
static __device__ __noinline__ double gpg_kern(int fam, double s2, double d2) {
    const double r = sqrt(d2);
    const double s = fam == 1 ? r : (fam == 2 ? 1.7320508075688772 : 2.23606797749979) * r;
    const double e = exp(fam == 0 ? -0.5 * d2 : -s);
    const double poly = fam <= 1 ? 1.0 : (fam == 2 ? 1.0 + s : 1.0 + s + s * s / 3.0);
    return s2 * (poly * e);
}

// sigma^2 h(r), h = f'(r) / r, of family 0 RBF, 2 Matern32, 3 Matern52: finite at r = 0.  (Matern12 has no gradient at a
// training point and never gets here: cesx_gp_predict_grad refuses it.)
static __device__ __noinline__ double gpg_dkern(int fam, double s2, double d2) {
    const double s = (fam == 2 ? 1.7320508075688772 : 2.23606797749979) * sqrt(d2);
    const double e = exp(fam == 0 ? -0.5 * d2 : -s);
    const double poly = fam == 0 ? -1.0 : (fam == 2 ? -3.0 : (-5.0 / 3.0) * (1.0 + s));
    return s2 * (poly * e);
}

template <typename T, bool LDSP>
__global__ __launch_bounds__(GP_THREADS)
void gp_grad_kernel(const GpGradArgs<T> a) {
    extern __shared__ double gpg_smem[];
    __shared__ double red[GP_RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int p = a.p;
    const bool full = a.var != nullptr;
    double* zq = LDSP ? gpg_smem : a.ws + (size_t)blockIdx.x * a.slot;      // [p][32]
    double* gz = zq + (size_t)p * GP_T;                                      // [2][p][32] d mean / dz, d var / dz
    double* P0 = gz + (size_t)2 * p * GP_T;                                  // [Jp][32] K*, then beta, then cv
    double* P1 = P0 + (size_t)a.Jp * GP_T;                                   // [Jp][32] W, then cm (full mode only)
    double* cm = full ? P1 : P0;
    const int NB = a.Jp >> 4;
    {   // (one tile per workgroup and no loop over tiles: with one, the launch's scalars are live around it and spill)
        const int w = a.w0 + (int)blockIdx.x;
        const int g = w / a.ntiles;
        const long long j0 = (long long)(w - g * a.ntiles) * GP_T;
        const double* A = a.A + (size_t)g * p * p;
        // 1. the mapped queries
        for (int idx = tid; idx < p * GP_T; idx += GP_THREADS) {
            const int r = idx / GP_T, cc = idx % GP_T;
            const long long j = j0 + cc;
            double z = 0.0;
            if (j < a.M)
                for (int s = 0; s <= r; ++s) z = fma(A[(size_t)r * p + s], (double)a.X[(size_t)s * a.M + j] - a.c[s], z);
            zq[idx] = z;
        }
        __syncthreads();
        // 2. the K* panel (zero rows past Jt) and the mean's partial sums
        const double s2 = a.par[4 * g], sn2 = a.par[4 * g + 1];
        const int fam = (int)a.par[4 * g + 3];
        const int cc = tid & (GP_T - 1), grp = tid / GP_T;
        const double* Zg = a.Z + (size_t)g * a.Jt * p;
        const double* al = a.alpha + (size_t)g * a.Jp;
        const double* mw = a.mw + (size_t)g * p;
        double macc = 0.0;
        for (int t = grp; t < a.Jp; t += GP_NG) {
            double k = 0.0;
            if (t < a.Jt) {
                double d2 = 0.0;
                for (int r = 0; r < p; ++r) { const double d = zq[r * GP_T + cc] - Zg[(size_t)t * p + r]; d2 = fma(d, d, d2); }
                k = gpg_kern(fam, s2, d2);
                macc = fma(al[t], k, macc);
            }
            P0[(size_t)t * GP_T + cc] = k;
        }
        red[grp * GP_T + cc] = macc;
        __syncthreads();
        if (tid < GP_T) {
            double m = 0.0;
            for (int q = 0; q < GP_NG; ++q) m += red[q * GP_T + tid];
            double lin = a.par[4 * g + 2];
            for (int r = 0; r < p; ++r) lin = fma(mw[r], zq[r * GP_T + tid], lin);
            const long long j = j0 + tid;
            if (j < a.M) a.mean[(size_t)g * a.M + j] = m + lin;
        }
        if (full) {
            __syncthreads();                                         // (red is read above)
            // 3. W = L^{-1} K* on the matrix pipe, the squares summed per column; W stays in P1
            const int col = lane & 15, kq = lane >> 4;
            const double* Lg = a.Li + (size_t)g * a.li_len;
            double ss0 = 0.0, ss1 = 0.0;
            for (int rr = 0; rr * GP_NW < NB; ++rr) {
                const int b = rr * GP_NW + ((rr & 1) ? GP_NW - 1 - wave : wave);
                if (b >= NB) continue;
                const double* Lb = Lg + (size_t)b * (b + 1) / 2 * 256;   // block row b: (b + 1) 4 k-steps of 64 values
                gp_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
                const int nk = (b + 1) * 4;
#pragma unroll 4
                for (int k4 = 0; k4 < nk; ++k4) {
                    const double av = Lb[(size_t)k4 * 64 + lane];           // L^{-1}[16 b + col][4 k4 + kq]
                    const double* kr = P0 + (size_t)(4 * k4 + kq) * GP_T + col;
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kr[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kr[16], acc1, 0, 0, 0);
                }
                // C/D map of the f64 form: column lane & 15, row kq + 4 reg
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ss0 = fma(acc0[q], acc0[q], ss0); ss1 = fma(acc1[q], acc1[q], ss1);
                    double* wr = P1 + (size_t)(16 * b + kq + 4 * q) * GP_T + col;
                    wr[0] = acc0[q]; wr[16] = acc1[q];
                }
            }
            red[(wave * 4 + kq) * GP_T + col] = ss0;
            red[(wave * 4 + kq) * GP_T + 16 + col] = ss1;
            __syncthreads();                                         // (and: every row of W is in P1, K* is dead)
            if (tid < GP_T) {
                double s = 0.0;
                for (int q = 0; q < GP_NW * 4; ++q) s += red[q * GP_T + tid];
                double v = s2 - s;
                if (a.nugget) v += sn2;
                const long long j = j0 + tid;
                if (j < a.M) a.var[(size_t)g * a.M + j] = v;
            }
            // 4. beta = L^{-T} W: block row c of beta sums the blocks (b, c), b >= c, of the packed image, each read
            //    transposed -- k-step j of block (b, c) gives lane (i = col, k = kq) the value L^{-1}[16 b + 4 j + k][16 c + i],
            //    which the image holds at k-step 4 c + (i >> 2), lane (i & 3) 16 + 4 j + k of block row b
            for (int rr = 0; rr * GP_NW < NB; ++rr) {
                const int c = rr * GP_NW + ((rr & 1) ? GP_NW - 1 - wave : wave);
                if (c >= NB) continue;
                gp_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
                const int at = (4 * c + (col >> 2)) * 64 + (col & 3) * 16 + kq;
                for (int b = c; b < NB; ++b) {
                    const double* Lb = Lg + (size_t)b * (b + 1) / 2 * 256 + at;
                    const double* wr = P1 + (size_t)(16 * b + kq) * GP_T + col;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double av = Lb[4 * j];
                        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, wr[(size_t)4 * j * GP_T], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, wr[(size_t)4 * j * GP_T + 16], acc1, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    double* br = P0 + (size_t)(16 * c + kq + 4 * q) * GP_T + col;
                    br[0] = acc0[q]; br[16] = acc1[q];
                }
            }
        }
        __syncthreads();                                             // (beta is in P0; mean-only: red and K* are read above)
        // 5. the coefficients of dk_t, each thread the (t, chain) pairs it sums below
        for (int t = grp; t < a.Jt; t += GP_NG) {
            double d2 = 0.0;
            for (int r = 0; r < p; ++r) { const double d = zq[r * GP_T + cc] - Zg[(size_t)t * p + r]; d2 = fma(d, d, d2); }
            const double hh = gpg_dkern(fam, s2, d2);
            if (full) P0[(size_t)t * GP_T + cc] *= hh;
            cm[(size_t)t * GP_T + cc] = al[t] * hh;
        }
        for (int r = 0; r < p; ++r) {
            const double zr = zq[r * GP_T + cc];
            double am = 0.0, av = 0.0;
            for (int t = grp; t < a.Jt; t += GP_NG) {
                const double d = zr - Zg[(size_t)t * p + r];
                am = fma(cm[(size_t)t * GP_T + cc], d, am);
                if (full) av = fma(P0[(size_t)t * GP_T + cc], d, av);
            }
            red[grp * GP_T + cc] = am;
            red[(GP_NG + grp) * GP_T + cc] = av;
            __syncthreads();
            if (tid < (full ? 2 : 1) * GP_T) {
                const int which = tid / GP_T;
                double s = 0.0;
                for (int q = 0; q < GP_NG; ++q) s += red[(which * GP_NG + q) * GP_T + cc];
                gz[((size_t)which * p + r) * GP_T + cc] = which ? -2.0 * s : s + mw[r];
            }
            __syncthreads();
        }
        // 6. d / dx = A^T d / dz
        for (int idx = tid; idx < (full ? 2 : 1) * p * GP_T; idx += GP_THREADS) {
            const int which = idx / (p * GP_T), s = idx / GP_T - which * p, c2 = idx % GP_T;
            const long long j = j0 + c2;
            double acc = 0.0;
            for (int r = s; r < p; ++r) acc = fma(A[(size_t)r * p + s], gz[((size_t)which * p + r) * GP_T + c2], acc);
            if (j < a.M) (which ? a.dvar : a.dmean)[((size_t)g * p + s) * a.M + j] = acc;
        }
    }
}

template <typename T>
static int gp_grad_t(Engine& e, const void* X, double* mean, double* var, double* dmean, double* dvar, bool nugget, hipStream_t s) {
    GpGradArgs<T> a{};
    a.X = (const T*)X; a.M = e.J; a.p = e.p;
    a.Jt = e.gp.Jt; a.Jp = e.gp.Jp; a.li_len = e.gp.li_len;
    a.A = e.gp.A; a.c = e.gp.c; a.Z = e.gp.Z; a.par = e.gp.par; a.mw = e.gp.mw; a.alpha = e.gp.alpha; a.Li = e.gp.Li;
    a.mean = mean; a.var = var; a.dmean = dmean; a.dvar = dvar; a.nugget = nugget ? 1 : 0;
    if ((e.J + GP_T - 1) / GP_T * (long long)e.gp.n >= (1LL << 31)) { e.err = "cesx_gp_predict_grad: too many (GP, tile) pairs"; return CESX_EUNSUPPORTED; }
    a.ntiles = (int)((e.J + GP_T - 1) / GP_T);
    const int nwork = a.ntiles * e.gp.n;
    const size_t tile = (size_t)(3 * e.p + (var ? 2 : 1) * e.gp.Jp) * GP_T;      // doubles
    a.slot = tile;
    if (tile * 8 <= GP_LDS_MAX) {
        auto kern = gp_grad_kernel<T, true>;
        CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(tile * 8)));
        hipLaunchKernelGGL(kern, dim3((unsigned)nwork), dim3(GP_THREADS), tile * 8, s, a);
    } else {
        // the tiles in global memory (the workspace of cesx_gp_predict): at most 256 MiB of them, one slot per workgroup, and
        // the (GP, tile) pairs in launches of that many workgroups -- the stream orders the launches, so a slot is free again
        const long long slots = std::max(1LL, std::min<long long>((long long)nwork, std::min<long long>(1024, (32LL << 20) / (long long)tile)));
        const size_t need = (size_t)slots * tile;
        if (e.gp.ws.bytes < need * 8) {
            if (e.gp.ws) CESX_HIP(hipStreamSynchronize(s));      // (a launch of this stream may still read the old one)
            TRY_BUF(e.gp.ws.alloc(need * 8, false));
        }
        a.ws = e.gp.ws;
        for (a.w0 = 0; a.w0 < nwork; a.w0 += (int)slots)
            hipLaunchKernelGGL((gp_grad_kernel<T, false>), dim3((unsigned)std::min<long long>(slots, nwork - a.w0)), dim3(GP_THREADS), 0, s, a);
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_gp_predict_grad(Engine& e, const void* X, double* mean, double* var, double* dmean, double* dvar, bool nugget,
                           hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? gp_grad_t<float>(e, X, mean, var, dmean, dvar, nugget, s)
                                   : gp_grad_t<double>(e, X, mean, var, dmean, dvar, nugget, s);
}

// ---- the Langevin step: one thread per chain ----

// LvArgs, LV_THREADS and lv_score (phi of chain j at X, gp_score_kernel's sums in its order, and g = S^T grad phi into a.gx):
// lv_score.h, shared with kernels_hmc.hip

// phi and g of the start states: a.gx is the chains' own g
template <typename T>
__global__ __launch_bounds__(LV_THREADS)
void lv_start_kernel(const LvArgs<T> a) {
    const long long j = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (j >= a.M) return;
    a.c.phi[j] = lv_score(a, j);
    a.c.cnt[j] = 0ull;
}

// P = U + S (xi - g(U) / 2)
template <typename T>
__global__ __launch_bounds__(LV_THREADS)
void lv_propose_kernel(const LvArgs<T> a) {
    const long long j = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (j >= a.M) return;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    for (int s = 0; s < p; ++s) {
        double acc = 0.0;
        for (int r = 0; r <= s; ++r) acc = fma(a.S[(size_t)s * p + r], (double)a.xi[r * M + j] - 0.5 * a.gu[r * M + j], acc);
        a.P[s * M + j] = (T)((double)a.U[s * M + j] + acc);
    }
}

// phi(P), g(P), the test log u < phi(U) - phi(P) + |xi|^2 / 2 - |xi - (g(U) + g(P)) / 2|^2 / 2; an accepted chain takes P, phi
// and g.  Any NaN makes the comparison false: the proposal is rejected, a chain whose own phi or g is NaN stays.
template <typename T>
__global__ __launch_bounds__(LV_THREADS)
void lv_accept_kernel(const LvArgs<T> a) {
    const long long j = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (j >= a.M) return;
    const int p = a.p;
    const size_t M = (size_t)a.M;
    const double ph = lv_score(a, j);
    double n1 = 0.0, n2 = 0.0;
    for (int r = 0; r < p; ++r) {
        const double x = (double)a.xi[r * M + j];
        const double d = x - 0.5 * (a.gu[r * M + j] + a.gx[r * M + j]);
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
static int lv_t(Engine& e, int what, int mode, const void* X, const double* mean, const double* var, const double* dmean,
                const double* dvar, void* U, void* P, const double* logu, unsigned step, hipStream_t s) {
    LvArgs<T> a{};
    a.mean = mean; a.var = var; a.dmean = dmean; a.dvar = dvar;
    a.n = mode == CESX_GP_PROJ ? e.gpp.k : e.n; a.p = e.p; a.mode = mode; a.M = e.J;
    a.phid = e.mh.phi_data;
    a.y = e.d_y; a.gw = e.d_gw; a.gam = e.d_Gamma; a.Lg = e.whiten ? e.d_Wh : nullptr;
    a.X = (const T*)X; a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get();
    a.S = e.mh.bS;
    a.ca = e.mh.lv_a; a.cb = e.mh.lv_b; a.gphi = e.mh.lv_gphi;
    a.gu = e.mh.lv_g; a.gx = what == 0 ? e.mh.lv_g.get() : e.mh.lv_gp.get();
    a.xi = (const T*)e.mh.xi.get(); a.U = (T*)U; a.P = (T*)P;
    a.c = mh_chains(e, what == 0, logu, step);
    const dim3 grid((unsigned)((e.J + LV_THREADS - 1) / LV_THREADS)), block(LV_THREADS);
    if (what == 0) hipLaunchKernelGGL((lv_start_kernel<T>), grid, block, 0, s, a);
    else if (what == 1) hipLaunchKernelGGL((lv_propose_kernel<T>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((lv_accept_kernel<T>), grid, block, 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

// what: 0 start (phi and g of the states X), 1 propose (P from U, the noise block in mh.xi and the chains' g), 2 accept (the
// proposal X = P with its GP rows and gradients; U takes the accepted columns)
int launch_gp_langevin(Engine& e, int what, int mode, const void* X, const double* mean, const double* var, const double* dmean,
                       const double* dvar, void* U, void* P, const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? lv_t<float>(e, what, mode, X, mean, var, dmean, dvar, U, P, logu, step, s)
                                   : lv_t<double>(e, what, mode, X, mean, var, dmean, dvar, U, P, logu, step, s);
}

}  // namespace cesx
