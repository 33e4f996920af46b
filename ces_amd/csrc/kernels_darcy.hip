// The Darcy forward map (ces_amd/darcy.py: gaussrnd_coarse + solve_gwf restated) over the columns of the (p, J) layout: one
// particle per workgroup of ONE wave, everything of that particle resident in LDS, all arithmetic fp64 whatever the engine
// dtype (the systems reach cond 1e8 and beyond on legitimate inputs; the engine dtype governs only how U is read and G written).
//
// Per particle xi (K = Nmesh, m = K - 2, n = m^2 unknowns):
//     L     = coef o Xi (xi scattered to its K^2 slots), L[0][0] = 0          (gaussrnd_coarse.m:6-23; coef holds the factor K)
//     theta = D L D^T                                                         (idct2: D the orthonormal inverse DCT-II matrix)
//     a     = S exp(theta) S^T                                                (interp2 'spline' centres -> nodes)
//     A     = 5-point operator, arithmetic-mean faces, (K-1)^2, column-major unknowns, half-bandwidth m   (solve_gwf.m:19-35)
//     A x   = 1       banded LU with partial pivoting (LAPACK gbtf2 / gbtrs: kl = ku = m, fill above the band, row swaps)
//     g_k   = (R' X R'^T)[obs_k],  R' = R[:, 1:-1], X = x as m x m column-major (only the n_obs picked centres are formed)
// The spline of exp(theta) overshoots below zero on ordinary inputs (the example's U0 = 10 N(0, 1) does in most draws): A is
// then symmetric INDEFINITE, which is why this is a pivoting LU and not a Cholesky.
//
// Placement.  The working band is (S + 1) n doubles; with the pad below 78 400 B at K = 16, plus one K x K scratch tile:
// 80 448 B per workgroup, two workgroups per CU (163 840 B of LDS).  A CU therefore holds two particles whatever the workgroup
// shape, and a column step is a dependent chain (pivot search -> swap -> multipliers -> rank-1 update) of at most m x 2m = 392
// entries: one wave does it in 7 passes without a single cross-wave barrier.
// Stages 1, 2 and 5 run here too, as K x K separable products on the resident particle: together 4 K^3 = 16 k FMAs beside
// the LU's ~77 k on a longer dependent chain, and theta / a never travel through HBM (a batched MFMA form would write and
// re-read K^2 J doubles per stage and add launches).  D, S, R come from L2 (a few KiB shared by every workgroup).
//
// Band layout.  A(r, c) lives at band[kv + r + c S], kv = 2 m: LAPACK's AB(kv + r - c, c) with leading dimension S + 1, where
// S >= 3 m is padded to S = 17 (mod 32).  Down a column of A the address step is 1, along a row it is S:
//     pivot search  lanes over <= m + 1 consecutive rows of one column              -> consecutive banks
//     row swap      lanes over <= 2 m + 1 columns of two rows: stride 17 (mod 32)   -> distinct banks for 32 consecutive columns
//     rank-1 update lane = 16 g + t: row t (1..m <= 14) of column g of the pass     -> group g covers banks 17 g + 1 .. 17 g + 14,
//                   its row-j operand bank 17 g: a 32-lane half (g = 0, 1 / 2, 3) touches each fp64 bank once
// The multipliers are applied to the right-hand side as they are formed and are not stored.
//
// Status.  A pivot that is exactly zero ends the particle: its status word is the 1-based column, its outputs NaN.  A pivot
// column that holds a NaN or an infinity (exp(theta) overflowed) ends it too, with MINUS the 1-based column: nothing is
// singular there, the input left fp64's range.  No trap, no assert.  Every sum has a fixed order: runs are bit-identical.
//
// ONE WAVE PER WORKGROUP is load-bearing (DARCY_THREADS == 64): the LDS accesses of one wave execute in program order, so a
// step may read a word in all lanes and overwrite it from one lane in the next statement, and lanes may touch the band and
// the right-hand side side by side, without a barrier in between; the __syncthreads() below only keep the compiler from
// moving LDS accesses across them.  The sites that rely on it are marked (one wave).  A version with more waves per particle
// needs real barriers at each of them.
#include "cesx_internal.h"

#include <limits>

namespace cesx {

constexpr int DARCY_KMAX = 16;
constexpr int DARCY_TILE = DARCY_KMAX * DARCY_KMAX;      // doubles of the K x K scratch tile in front of the band
constexpr int DARCY_THREADS = 64;                        // one wave: see the header
static_assert(DARCY_THREADS == 64, "darcy_kernel orders its LDS accesses by the program order of ONE wave");

struct DarcyArgs {
    const void* U; void* G; int* status; long long J;
    int K, p, n_obs, S;
    const double *coef, *D, *Sm, *R;
    const int *scatter, *obs;
};

// row stride of the band: the smallest S >= 3 m with S = 17 (mod 32)
inline int darcy_stride(int K) { const int m = K - 2; return 3 * m <= 17 ? 17 : 49; }
inline size_t darcy_lds(int K) { const int m = K - 2; return ((size_t)(darcy_stride(K) + 1) * m * m + DARCY_TILE) * 8; }

// out = M in (K x K, row-major), one entry per lane and pass
__device__ inline void darcy_left(double* out, const double* __restrict__ M, const double* in, int K, int lane) {
    for (int e = lane; e < K * K; e += DARCY_THREADS) {
        const int i = e / K, c = e - i * K;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(M[i * K + k], in[k * K + c], s);
        out[e] = s;
    }
}

// out = f(in M^T)
template <bool EXP>
__device__ inline void darcy_right(double* out, const double* in, const double* __restrict__ M, int K, int lane) {
    for (int e = lane; e < K * K; e += DARCY_THREADS) {
        const int i = e / K, c = e - i * K;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(in[i * K + k], M[c * K + k], s);
        out[e] = EXP ? exp(s) : s;
    }
}

template <typename T>
__global__ __launch_bounds__(DARCY_THREADS)
void darcy_kernel(const DarcyArgs a) {
    extern __shared__ double darcy_smem[];
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;                       // the particle
    const int K = a.K, m = K - 2, n = m * m, kv = 2 * m, S = a.S, KK = K * K;
    double* t0 = darcy_smem;                              // K x K tile: L, exp(theta), a; then the right-hand side / x
    double* band = darcy_smem + DARCY_TILE;               // (S + 1) n doubles
    double* t1 = band;                                    // the second K x K tile of stages 1-2 and W of stage 5 alias the band
    const T* U = (const T*)a.U;
    T* G = (T*)a.G;

    // ---- 1: KL synthesis ----
    for (int e = lane; e < KK; e += DARCY_THREADS) t0[e] = 0.0;
    __syncthreads();
    for (int q = lane; q < a.p; q += DARCY_THREADS) {
        const int s = a.scatter[q];
        t0[s] = a.coef[s] * (double)U[(size_t)q * a.J + j];
    }
    __syncthreads();
    if (lane == 0) t0[0] = 0.0;                           // the constant mode is removed (gaussrnd_coarse.m:21)
    __syncthreads();
    darcy_left(t1, a.D, t0, K, lane);
    __syncthreads();
    darcy_right<true>(t0, t1, a.D, K, lane);              // exp(theta)
    __syncthreads();
    // ---- 2: to the nodes ----
    darcy_left(t1, a.Sm, t0, K, lane);
    __syncthreads();
    darcy_right<false>(t0, t1, a.Sm, K, lane);            // a (K x K) at the nodes
    __syncthreads();
    // ---- 3: assembly into the zeroed band ----
    for (int e = lane; e < (S + 1) * n; e += DARCY_THREADS) band[e] = 0.0;
    __syncthreads();
    const double h2 = (double)((K - 1) * (K - 1));
    for (int q = lane; q < n; q += DARCY_THREADS) {
        const int jj = q / m + 1, i = q - (jj - 1) * m + 1;      // interior node (i, jj), unknowns column by column
        const double cc = t0[i * K + jj];
        const double w = (t0[(i - 1) * K + jj] + cc) / 2, e = (t0[(i + 1) * K + jj] + cc) / 2;
        const double s = (t0[i * K + jj - 1] + cc) / 2, nn = (t0[i * K + jj + 1] + cc) / 2;
        double* row = band + kv + q;                      // A(q, c) = row[c S]
        row[q * S] = (w + e + s + nn) * h2;
        if (i > 1) row[(q - 1) * S] = -w * h2;
        if (i < m) row[(q + 1) * S] = -e * h2;
        if (jj > 1) row[(q - m) * S] = -s * h2;
        if (jj < m) row[(q + m) * S] = -nn * h2;
    }
    __syncthreads();
    for (int q = lane; q < n; q += DARCY_THREADS) t0[q] = 1.0;       // the right-hand side (the spline of the constant 1 is 1)
    __syncthreads();

    // ---- 4: banded LU with partial pivoting, the right-hand side eliminated along ----
    const int t = lane & 15, grp = lane >> 4;
    int ju = 0, info = 0;
    for (int col = 0; col < n; ++col) {
        const int km = min(m, n - 1 - col);
        double* cj = band + kv + col + col * S;           // A(col + t, col) = cj[t]
        const bool in_col = t <= km;
        const double av = in_col ? fabs(cj[t]) : -1.0;
        double mx = av;
        for (int o = 8; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 16));
        const unsigned long long hit = __ballot(in_col && av == mx) & 0xffffull;     // (the 16-lane groups hold copies: group 0 speaks)
        // a NaN never wins fmax and an infinity is no pivot to divide by: any non-finite entry of the pivot column ends the particle
        const unsigned long long nonfin = __ballot(in_col && !(av <= 1.7976931348623157e308)) & 0xffffull;
        if (nonfin != 0ull || hit == 0ull) { info = -(col + 1); break; }
        if (!(mx > 0.0)) { info = col + 1; break; }
        const int jp = __ffsll((long long)hit) - 1;       // the first largest entry, as idamax
        ju = max(ju, min(col + m + jp, n - 1));
        const int nc = ju - col;                          // columns right of col this step touches (<= 2 m)
        if (jp != 0) {                                    // rows col and col + jp over the columns col .. ju, and in the right-hand side
            if (lane <= nc) {
                double* p0 = band + kv + col + (col + lane) * S;
                const double x0 = p0[0], x1 = p0[jp];
                p0[0] = x1; p0[jp] = x0;
            } else if (lane == DARCY_THREADS - 1) {       // (one wave: the right-hand side beside the band, nc <= 2 m < 63)
                const double x0 = t0[col], x1 = t0[col + jp];
                t0[col] = x1; t0[col + jp] = x0;
            }
            __syncthreads();
        }
        if (km > 0) {
            const bool row_on = t >= 1 && t <= km;
            const double l = row_on ? cj[t] / cj[0] : 0.0;        // the multipliers: used here, not stored
            if (row_on && grp == 0) t0[col + t] -= l * t0[col];
            for (int c0 = 1; c0 <= nc; c0 += 4) {
                const int c = c0 + grp;
                if (row_on && c <= nc) {
                    double* pc = band + kv + col + (col + c) * S;
                    pc[t] -= l * pc[0];
                }
            }
        }
        __syncthreads();
    }
    // back substitution with U (bandwidth kv above the diagonal)
    if (!info) {
        for (int col = n - 1; col >= 0; --col) {
            const double* cj = band + kv + col + col * S;         // A(col - t, col) = cj[-t]
            const double xj = t0[col] / cj[0];                    // (one wave: every lane reads t0[col] before lane 0 overwrites it)
            if (lane >= 1 && lane <= min(kv, col)) t0[col - lane] -= xj * cj[-lane];
            if (lane == 0) t0[col] = xj;
            __syncthreads();
        }
        // ---- 5: back to the picked centres ----
        for (int e = lane; e < K * m; e += DARCY_THREADS) {          // W = R[:, 1:-1] X, X[i][jx] = x[jx m + i]
            const int r = e / m, jx = e - r * m;
            double s = 0.0;
            for (int i = 0; i < m; ++i) s = fma(a.R[r * K + 1 + i], t0[jx * m + i], s);
            t1[e] = s;
        }
        __syncthreads();
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int k = lane; k < a.n_obs; k += DARCY_THREADS) {
        double g = qnan;
        if (!info) {
            const int o = a.obs[k], r = o / K, c = o - r * K;     // row-major flatten of the K x K centres
            g = 0.0;
            for (int jx = 0; jx < m; ++jx) g = fma(t1[r * m + jx], a.R[c * K + 1 + jx], g);
        }
        G[(size_t)k * a.J + j] = (T)g;
    }
    if (a.status && lane == 0) a.status[j] = info;
}

// once per installed map (cesx_darcy_set): both instantiations may take the dynamic LDS of this K
int darcy_prepare(Engine& e, int K) {
    const int lds = (int)darcy_lds(K);
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(darcy_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(darcy_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return CESX_OK;
}

int launch_darcy(Engine& e, const void* U, void* G, int* status, hipStream_t s) {
    DarcyArgs a{};
    a.U = U; a.G = G; a.status = status; a.J = e.J;
    a.K = e.dc.K; a.p = e.p; a.n_obs = e.n; a.S = darcy_stride(e.dc.K);
    const int KK = e.dc.K * e.dc.K;
    a.coef = e.dc.mat; a.D = e.dc.mat + KK; a.Sm = e.dc.mat + 2 * KK; a.R = e.dc.mat + 3 * KK;
    a.scatter = e.dc.idx; a.obs = e.dc.idx + e.p;
    if (e.J >= (1LL << 31)) { e.err = "cesx_darcy_apply: too many particles for one launch"; return CESX_EUNSUPPORTED; }
    const size_t lds = darcy_lds(e.dc.K);
    auto kern = e.cfg.dtype == CESX_F32 ? darcy_kernel<float> : darcy_kernel<double>;
    hipLaunchKernelGGL(kern, dim3((unsigned)e.J), dim3(DARCY_THREADS), lds, s, a);      // (J >= 1: cesx_create)
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

}  // namespace cesx
