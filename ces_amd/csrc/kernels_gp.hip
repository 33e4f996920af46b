// The GP emulator over the columns of the (p, J) layout: the batched prediction of ces/emulate.py predict_gps and the score
// and accept step of MCMC.gp_mh (ces/sample.py:17-119), one independent chain per column.  All GP arithmetic is fp64
// whatever the engine dtype (the optimiser drives sn^2 to ~1e-6 sigma^2; fp32 errors in L^{-1} k* would swamp the variance).
//
// gp_predict_kernel: one workgroup per (GP i, tile of GP_T = 32 chains), the grid output-major so that the workgroups in flight
// share one L_i^{-1} in L2.  Per tile:
//     z_c  = A_i (x_c - c)                                       (the input map: ARD lengthscales and enka.scale in one)
//     K*   = sigma_i^2 f(|z_c - Z_t|)   [Jp x 32] in LDS          (vector ALU; r from direct differences: 0 on a training point)
//     mean = K*^T alpha_i + w_i^T z_c + b_i
//     W    = L_i^{-1} K*                                          (v_mfma_f64_16x16x4_f64: A = L^{-1} from L2, B = K* from LDS)
//     var  = sigma_i^2 - sum_t W_tc^2 (+ sn_i^2 with the nugget)
// The 8 waves take the 16-row block rows of W in zig-zag order (block b to wave b % 8, reversed every other round) so that
// the triangle's work splits evenly.  Every sum has a fixed order (no atomics): runs are bit-identical.  A panel that does
// not fit in LDS (Jp + p > 608) lives in a global workspace per workgroup slot and the grid strides over the tiles.
//
// gp_score_kernel: one thread per chain, phi from the fp64 GP rows in the likelihood mode of include/cesx.h, the prior term
// for RW and pCN alike (ces/sample.py subtracts prior.logpdf for both), the test (mh_test, cesx_internal.h: mh_accept_kernel's) and the copy U := P of the accepted columns.
#include "cesx_internal.h"

namespace cesx {

constexpr int GP_T = 32;                   // chains per tile (two 16-column MFMA groups)
constexpr int GP_NW = 8;                   // waves per workgroup
constexpr int GP_THREADS = GP_NW * 64;
constexpr int GP_RED = GP_NW * 4 * GP_T;   // doubles of the partial-sum buffer
constexpr size_t GP_LDS_MAX = 160 * 1024 - GP_RED * 8;
using gp_d4 = double __attribute__((ext_vector_type(4)));

template <typename T>
struct GpArgs {
    const T* X; long long M; int p;
    int Jt, Jp; size_t li_len;
    const double *A, *c, *Z, *par, *mw, *alpha, *Li;
    double* mean; double* var; int nugget;
    double* ws;                            // nullptr: the panel in LDS
    int ntiles, nwork;
};

// sigma^2 f(r) of kernel family fam (0 RBF, 1 Matern12, 2 Matern32, 3 Matern52); d2 = r^2
__device__ __noinline__ double gp_kern(int fam, double s2, double d2) {
    const double r = sqrt(d2);
    const double s = fam == 1 ? r : (fam == 2 ? 1.7320508075688772 : 2.23606797749979) * r;
    const double e = exp(fam == 0 ? -0.5 * d2 : -s);            // (one exp: its constants are SGPR pairs)
    const double poly = fam <= 1 ? 1.0 : (fam == 2 ? 1.0 + s : 1.0 + s + s * s / 3.0);
    return s2 * (poly * e);
}

template <typename T, bool LDSP>
__global__ __launch_bounds__(GP_THREADS)
void gp_predict_kernel(const GpArgs<T> a) {
    extern __shared__ double gp_smem[];
    __shared__ double red[GP_RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int p = a.p;
    double* zq = LDSP ? gp_smem : a.ws + (size_t)blockIdx.x * (size_t)(p + a.Jp) * GP_T;     // [p][32]
    double* Kp = zq + (size_t)p * GP_T;                                                          // [Jp][32]
    const int NB = a.Jp >> 4;
    // (the LDS path has one tile per workgroup: no loop, fewer live scalars)
    for (int w = blockIdx.x; w < a.nwork; w += LDSP ? a.nwork : (int)gridDim.x) {
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
        const int cc = tid & (GP_T - 1), grp = tid / GP_T;          // 16 groups of 32 threads
        const double* Zg = a.Z + (size_t)g * a.Jt * p;
        const double* al = a.alpha + (size_t)g * a.Jp;
        double macc = 0.0;
        for (int t = grp; t < a.Jp; t += GP_THREADS / GP_T) {
            double k = 0.0;
            if (t < a.Jt) {
                double d2 = 0.0;
                for (int r = 0; r < p; ++r) { const double d = zq[r * GP_T + cc] - Zg[(size_t)t * p + r]; d2 = fma(d, d, d2); }
                k = gp_kern(fam, s2, d2);
                macc = fma(al[t], k, macc);
            }
            Kp[(size_t)t * GP_T + cc] = k;
        }
        red[grp * GP_T + cc] = macc;
        __syncthreads();
        if (tid < GP_T) {
            double m = 0.0;
            for (int q = 0; q < GP_THREADS / GP_T; ++q) m += red[q * GP_T + tid];
            double lin = a.par[4 * g + 2];
            const double* mw = a.mw + (size_t)g * p;
            for (int r = 0; r < p; ++r) lin = fma(mw[r], zq[r * GP_T + tid], lin);
            const long long j = j0 + tid;
            if (j < a.M) a.mean[(size_t)g * a.M + j] = m + lin;
        }
        if (a.var) {
            __syncthreads();                                         // (red is read above)
            // 3. W = L^{-1} K* on the matrix pipe, the squares summed per column
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
                    const double* kr = Kp + (size_t)(4 * k4 + kq) * GP_T + col;
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kr[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kr[16], acc1, 0, 0, 0);
                }
                // C/D map: column lane & 15, row kq + 4 reg
#pragma unroll
                for (int q = 0; q < 4; ++q) { ss0 = fma(acc0[q], acc0[q], ss0); ss1 = fma(acc1[q], acc1[q], ss1); }
            }
            red[(wave * 4 + kq) * GP_T + col] = ss0;
            red[(wave * 4 + kq) * GP_T + 16 + col] = ss1;
            __syncthreads();
            if (tid < GP_T) {
                double s = 0.0;
                for (int q = 0; q < GP_NW * 4; ++q) s += red[q * GP_T + tid];
                double v = s2 - s;
                if (a.nugget) v += sn2;
                const long long j = j0 + tid;
                if (j < a.M) a.var[(size_t)g * a.M + j] = v;
            }
        }
        __syncthreads();                                             // (zq, Kp and red are rewritten by the next tile)
    }
}

template <typename T>
static int gp_predict_t(Engine& e, const void* X, double* mean, double* var, bool nugget, hipStream_t s) {
    GpArgs<T> a{};
    a.X = (const T*)X; a.M = e.J; a.p = e.p;
    a.Jt = e.gp.Jt; a.Jp = e.gp.Jp; a.li_len = e.gp.li_len;
    a.A = e.gp.A; a.c = e.gp.c; a.Z = e.gp.Z; a.par = e.gp.par; a.mw = e.gp.mw; a.alpha = e.gp.alpha; a.Li = e.gp.Li;
    a.mean = mean; a.var = var; a.nugget = nugget ? 1 : 0;
    if ((e.J + GP_T - 1) / GP_T * (long long)e.gp.n >= (1LL << 31)) { e.err = "cesx_gp_predict: too many (GP, tile) pairs"; return CESX_EUNSUPPORTED; }
    a.ntiles = (int)((e.J + GP_T - 1) / GP_T);
    a.nwork = a.ntiles * e.gp.n;
    const size_t panel = (size_t)(e.p + e.gp.Jp) * GP_T;                  // doubles
    if (panel * 8 <= GP_LDS_MAX) {
        auto kern = gp_predict_kernel<T, true>;
        CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(panel * 8)));
        hipLaunchKernelGGL(kern, dim3((unsigned)a.nwork), dim3(GP_THREADS), panel * 8, s, a);
    } else {
        // the panels in global memory: at most 256 MiB of them, the grid strides over the tiles
        const long long slots = std::max(1LL, std::min<long long>((long long)a.nwork, std::min<long long>(1024, (32LL << 20) / (long long)panel)));
        const size_t need = (size_t)slots * panel;
        if (e.gp.ws.bytes < need * 8) {
            if (e.gp.ws) CESX_HIP(hipStreamSynchronize(s));      // (a launch of this stream may still read the old one)
            TRY_BUF(e.gp.ws.alloc(need * 8, false));
        }
        a.ws = e.gp.ws;
        hipLaunchKernelGGL((gp_predict_kernel<T, false>), dim3((unsigned)slots), dim3(GP_THREADS), 0, s, a);
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_gp_predict(Engine& e, const void* X, double* mean, double* var, bool nugget, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? gp_predict_t<float>(e, X, mean, var, nugget, s)
                                   : gp_predict_t<double>(e, X, mean, var, nugget, s);
}

template <typename T>
struct GpScoreArgs {
    const double *mean, *var; int n; long long M;
    const double *y, *gw, *gam, *Lg;       // data: y (whitened when Lg != nullptr), diag(Gamma^{-1}), diag(Gamma) (stride n + 1), L_Gamma^{-1}
    int mode;
    const T* X; const double *mu, *sw, *LSi; int p;      // prior: diagonal (sw) or dense (LSi = L_Sigma^{-1})
    T* U;
    MhChains c;                            // (last: the tail it shares with MhArgs)
};

constexpr int GPS_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(GPS_THREADS)
void gp_score_kernel(const GpScoreArgs<T> a) {
    const long long j = (long long)blockIdx.x * GPS_THREADS + threadIdx.x;
    if (j >= a.M) return;
    const int n = a.n, p = a.p;
    double s = 0.0;
    if (a.mode == CESX_GP_GAMMA) {
        if (a.Lg) {
            for (int i = 0; i < n; ++i) {
                double w = 0.0;
                for (int k = 0; k <= i; ++k) w = fma(a.Lg[(size_t)i * n + k], a.mean[(size_t)k * a.M + j], w);
                const double d = w - a.y[i];
                s = fma(d, d, s);
            }
        } else {
            for (int i = 0; i < n; ++i) { const double d = a.mean[(size_t)i * a.M + j] - a.y[i]; s = fma(a.gw[i], d * d, s); }
        }
    } else {
        for (int i = 0; i < n; ++i) {
            double v = a.var[(size_t)i * a.M + j];
            if (a.mode == CESX_GP_GAMMA_VAR) v = a.gam[(size_t)i * (n + 1)] + v;
            const double d = a.mean[(size_t)i * a.M + j] - a.y[i];
            s += d * d / v + log(v);                 // (v <= 0: NaN or inf - inf, the test below then rejects)
        }
    }
    if (a.LSi) {
        for (int r = 0; r < p; ++r) {
            double w = 0.0;
            for (int k = 0; k <= r; ++k) w = fma(a.LSi[(size_t)r * p + k], (double)a.X[(size_t)k * a.M + j] - a.mu[k], w);
            s = fma(w, w, s);
        }
    } else {
        for (int r = 0; r < p; ++r) { const double d = (double)a.X[(size_t)r * a.M + j] - a.mu[r]; s = fma(a.sw[r], d * d, s); }
    }
    if (mh_test(a.c, j, 0.5 * s))
        for (int r = 0; r < p; ++r) a.U[(size_t)r * a.M + j] = a.X[(size_t)r * a.M + j];
}

template <typename T>
static int gp_score_t(Engine& e, int mode, bool start, const void* X, const double* mean, const double* var, void* U,
                      const double* logu, unsigned step, hipStream_t s) {
    GpScoreArgs<T> a{};
    a.mean = mean; a.var = var; a.n = e.n; a.M = e.J;
    a.y = e.d_y; a.gw = e.d_gw; a.gam = e.d_Gamma; a.Lg = e.whiten ? e.d_Wh : nullptr;
    a.mode = mode;
    a.X = (const T*)X; a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get(); a.p = e.p;
    a.U = (T*)U; a.c = mh_chains(e, start, logu, step);
    hipLaunchKernelGGL((gp_score_kernel<T>), dim3((unsigned)((e.J + GPS_THREADS - 1) / GPS_THREADS)), dim3(GPS_THREADS), 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int launch_gp_score(Engine& e, int mode, bool start, const void* X, const double* mean, const double* var, void* U,
                    const double* logu, unsigned step, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? gp_score_t<float>(e, mode, start, X, mean, var, U, logu, step, s)
                                   : gp_score_t<double>(e, mode, start, X, mean, var, U, logu, step, s);
}

}  // namespace cesx
