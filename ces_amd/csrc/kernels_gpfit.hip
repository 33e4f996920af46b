// Training the GP emulators: the log marginal likelihood of n_gp exact GPs on shared training inputs and its gradient in
// the natural parameters (ces_amd/emulate.py, GPR.log_marginal_likelihood_and_grad), all GPs of a batch in every launch
// (the batch index is grid.y; the launch count depends on J_t alone).  All arithmetic fp64 whatever the engine dtype.
//
// Per GP i with theta_i = (sigma^2, l (p values with ARD, else 1), sn^2, mean parameters), Jp = J_t rounded up to 16,
// the padding rows and columns those of the identity (the factor, its inverse and K^{-1} are the identity there):
//   gpfit_prep_kernel    Xs = X / l (the division of Stationary._scaled_diff), r = y - m(X), status := CESX_OK
//   gpfit_build_kernel   Ky = sigma^2 f(|Xs_a - Xs_b|) + sn^2 I, lower triangle, r from direct differences (0 on the diagonal)
//   gpfit_chol_kernel    one launch per block column k of 16 (left-looking): every workgroup forms and factors the diagonal
//                        block T_kk = Ky_kk - sum_j L_kj L_kj^T in LDS (its four waves split j; the partial sums are added in
//                        a fixed order), then each wave takes one 16-row block of the augmented matrix [Ky; I]:
//                            L_ik = (Ky_ik - sum_{j<k} L_ij L_kj^T) L_kk^{-T}             (i > k)
//                            W_ik = (I_ik  - sum_{i<=j<k} W_ij L_kj^T) L_kk^{-T}          (i <= k),   W = L^{-T},
//                        the sums on v_mfma_f64_16x16x4_f64, the 16 x 16 solve by substitution (16 lanes, a row each).
//                        So the triangular inverse comes out of the factorisation's own launches.  A pivot that is not > 0
//                        sets the GP's status word; the other GPs of the batch never see it.  Every workgroup of launch k
//                        READS Ky_kk, so no workgroup may overwrite it in that launch (workgroups of one grid are not
//                        ordered, and a grid can be larger than what is resident at once): L_kk goes to a buffer of its own
//                        (Ld), Ky's diagonal blocks stay in place, and nothing a launch writes is read before the next.
//   gpfit_kinv_kernel    K^{-1} = W W^T, lower block triangle, one wave per 16 x 16 block (MFMA)
//   gpfit_tvec_kernel    t = W^T r = L^{-1} r;   gpfit_alpha_kernel   alpha = W t = L^{-T} t
//   gpfit_grad_kernel    one pass over the lower triangle in 64 x 64 tiles: the differences and g = sigma^2 f'(r) / r again,
//                        Q = alpha alpha^T - K^{-1}; per tile the sums of Q f, Q g D_d^2 (per d with ARD, else Q g r^2) and
//                        tr Q, off-diagonal entries twice.  The p derivative matrices of the host are never stored.
//   gpfit_final_kernel   the tiles' partial sums in a fixed order, sum log L_aa, r^T alpha, the mean's gradient; lml, the
//                        gradient in GPR._get() order and the status into the output rows.
// No atomics: every sum has one order (lane-strided partials, a butterfly over the wave, the waves in sequence), so two
// evaluations are bit-identical.
//
// MFMA operands: lane (m = lane & 15, q = lane >> 4) supplies A[m][k] and B[k][m] of one k in four.  Both operands here are
// rows of row-major matrices read along k, so a lane loads the FOUR consecutive k's 16 kb + 4 q .. + 3 of its row in one
// 32-byte load and feeds them to four successive instructions: instruction s sums over k = 16 kb + 4 q' + s, q' = 0..3 --
// a permutation of k, the same for A and B.  C/D: column lane & 15, row q + 4 reg.
#include "cesx_internal.h"

namespace cesx {

constexpr int GF_NW = 4;                   // waves per workgroup
constexpr int GF_THREADS = GF_NW * 64;
constexpr int GF_TILE = 64;                // the build / gradient pass works in 64 x 64 tiles of the lower triangle
constexpr int GF_DC = 8;                   // lengthscale sums a thread carries at a time (p > 8: more passes over the tile)
using gf_d4 = double __attribute__((ext_vector_type(4)));

struct GpFitArgs {
    int Jt, Jp, NB, p, family, ard, mean, nl, ntheta, ntile, nacc;
    const int* idx;                        // [n_active] the GPs of this evaluation
    const double* theta;                   // [n_active][ntheta]
    const double *X, *Y;                   // [Jt][p], [n_gp][Jt]
    double *Xs, *res, *tv, *alpha;         // [n_gp][Jp][p], [n_gp][Jp] each
    double *A, *W, *Ki;                    // [n_gp][Jp][Jp]: Ky -> L (strictly lower blocks; the diagonal blocks stay Ky's), L^{-T} (upper), K^{-1} (lower)
    double* Ld;                            // [n_gp][Jp][16] the diagonal blocks L_kk (row 16 k + r, column c)
    double* part;                          // [n_gp][ntile][nacc]
    int* status;                           // [n_gp]
    double* out;                           // [n_active][2 + ntheta]: lml, status, gradient
};

// f(r) and f'(r) / r of kernel family fam (0 RBF, 1 Matern12, 2 Matern32, 3 Matern52); d2 = r^2.  (f'(r) / r is finite at
// r = 0 but for Matern12, whose factor D_d^2 is 0 there: 0, as the host's dfr_over_r.)
__device__ __forceinline__ void gf_kern(int fam, double d2, double& f, double& g) {
    const double r = sqrt(d2);
    const double s = fam == 1 ? r : (fam == 2 ? 1.7320508075688772 : 2.23606797749979) * r;
    const double e = exp(fam == 0 ? -0.5 * r * r : -s);            // (one exp: its constants are SGPR pairs)
    if (fam == 0) { f = e; g = -e; }
    else if (fam == 1) { f = e; g = r > 0.0 ? -e / r : 0.0; }
    else if (fam == 2) { f = (1.0 + s) * e; g = -3.0 * e; }
    else { f = (1.0 + s + s * s / 3.0) * e; g = -(5.0 / 3.0) * (1.0 + s) * e; }
}

// tile t of the lower triangle, row-major: (ta, tb), tb <= ta
__device__ __forceinline__ void gf_tile(int t, int& ta, int& tb) {
    int a = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= t) ++a;
    while (a * (a + 1) / 2 > t) --a;
    ta = a; tb = t - a * (a + 1) / 2;
}

// the wave's sum in one order (butterfly), in every lane
__device__ __forceinline__ double gf_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sum (waves added in sequence), in every thread; red: GF_NW doubles
__device__ __forceinline__ double gf_block_sum(double v, double* red) {
    v = gf_wave_sum(v);
    __syncthreads();                                        // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < GF_NW; ++w) s += red[w];
    return s;
}

// acc0 + acc1 += sum over the 16-wide k blocks j0 .. j1-1 of rows ra x rows rb (each pointer at the lane's row, + 4 q):
// four blocks' loads are issued before their sixteen instructions -- the loop is bound by the latency of L2, not by the pipe
__device__ __forceinline__ void gf_mac_blocks(const double* ra, const double* rb, int j0, int j1, gf_d4& acc0, gf_d4& acc1) {
    int j = j0;
    for (; j + 4 <= j1; j += 4) {
        gf_d4 va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            va[u] = *reinterpret_cast<const gf_d4*>(ra + 16 * (j + u));
            vb[u] = *reinterpret_cast<const gf_d4*>(rb + 16 * (j + u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][0], vb[u][0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][1], vb[u][1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][2], vb[u][2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][3], vb[u][3], acc1, 0, 0, 0);
        }
    }
    for (; j < j1; ++j) {
        const gf_d4 va = *reinterpret_cast<const gf_d4*>(ra + 16 * j);
        const gf_d4 vb = *reinterpret_cast<const gf_d4*>(rb + 16 * j);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[0], vb[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[1], vb[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[2], vb[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[3], vb[3], acc1, 0, 0, 0);
    }
}

__global__ __launch_bounds__(GF_THREADS)
void gpfit_prep_kernel(const GpFitArgs a) {
    const int g = a.idx[blockIdx.y];
    const double* th = a.theta + (size_t)blockIdx.y * a.ntheta;
    const int row = blockIdx.x * GF_THREADS + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[g] = CESX_OK;
    if (row >= a.Jp) return;
    const int p = a.p;
    double* xs = a.Xs + ((size_t)g * a.Jp + row) * p;
    double r = 0.0;
    if (row < a.Jt) {
        const double* x = a.X + (size_t)row * p;
        const double* mp = th + a.nl + 2;
        double m = 0.0;
        if (a.mean == 1) m = mp[0];
        for (int d = 0; d < p; ++d) {
            xs[d] = x[d] / th[1 + (a.ard ? d : 0)];
            if (a.mean == 2) m = fma(x[d], mp[d], m);
        }
        if (a.mean == 2) m += mp[p];
        r = a.Y[(size_t)g * a.Jt + row] - m;
    } else {
        for (int d = 0; d < p; ++d) xs[d] = 0.0;
    }
    a.res[(size_t)g * a.Jp + row] = r;
}

__global__ __launch_bounds__(GF_THREADS)
void gpfit_build_kernel(const GpFitArgs a) {
    const int g = a.idx[blockIdx.y];
    const double* th = a.theta + (size_t)blockIdx.y * a.ntheta;
    const double s2 = th[0], sn2 = th[1 + a.nl];
    int ta, tb;
    gf_tile((int)blockIdx.x, ta, tb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, p = a.p, Jp = a.Jp;
    const double* Xs = a.Xs + (size_t)g * Jp * p;
    double* A = a.A + (size_t)g * Jp * Jp;
    for (int ii = 0; ii < 4; ++ii) {
        const int ra = ta * GF_TILE + ty + 16 * ii;
        if (ra >= Jp) continue;
        for (int jj = 0; jj < 4; ++jj) {
            const int cb = tb * GF_TILE + tx + 16 * jj;
            if (cb > ra) continue;
            double v;
            if (ra >= a.Jt) {
                v = ra == cb ? 1.0 : 0.0;
            } else {
                double d2 = 0.0;
                for (int d = 0; d < p; ++d) { const double df = Xs[(size_t)ra * p + d] - Xs[(size_t)cb * p + d]; d2 = fma(df, df, d2); }
                double f, gq;
                gf_kern(a.family, d2, f, gq);
                v = s2 * f;
                if (ra == cb) v += sn2;
            }
            A[(size_t)ra * Jp + cb] = v;
        }
    }
}

__global__ __launch_bounds__(GF_THREADS)
void gpfit_chol_kernel(const GpFitArgs a, const int k) {
    __shared__ double S[GF_NW][16][17];
    __shared__ double D[16][17];
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int g = a.idx[blockIdx.y];
    const int Jp = a.Jp, NB = a.NB;
    double* A = a.A + (size_t)g * Jp * Jp;
    double* W = a.W + (size_t)g * Jp * Jp;
    const double* rowk = A + (size_t)(16 * k + m) * Jp + 4 * q;
    // 1. the diagonal block: the waves split the sum over j
    {
        gf_d4 acc = {0.0, 0.0, 0.0, 0.0};
        int j = wave;
        for (; j + GF_NW < k; j += 2 * GF_NW) {                      // (two blocks' loads in flight)
            const gf_d4 v = *reinterpret_cast<const gf_d4*>(rowk + 16 * j);
            const gf_d4 w = *reinterpret_cast<const gf_d4*>(rowk + 16 * (j + GF_NW));
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[s], v[s], acc, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w[s], w[s], acc, 0, 0, 0);
        }
        if (j < k) {
            const gf_d4 v = *reinterpret_cast<const gf_d4*>(rowk + 16 * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[s], v[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S[wave][q + 4 * r][m] = acc[r];
    }
    __syncthreads();
    const int dr = tid >> 4, dc = tid & 15;
    {
        double v = 0.0;
        if (dc <= dr) v = A[(size_t)(16 * k + dr) * Jp + 16 * k + dc] - (((S[0][dr][dc] + S[1][dr][dc]) + S[2][dr][dc]) + S[3][dr][dc]);
        D[dr][dc] = v;
    }
    __syncthreads();
    bool bad = false;
    for (int c = 0; c < 16; ++c) {
        double d = D[c][c];
        if (!(d > 0.0)) { bad = true; d = 1.0; }
        const double piv = sqrt(d);
        __syncthreads();
        if (dc == c && dr >= c) D[dr][c] = dr == c ? piv : D[dr][c] / piv;
        __syncthreads();
        if (dr > c && dc > c && dc <= dr) D[dr][dc] = fma(-D[dr][c], D[dc][c], D[dr][dc]);
        __syncthreads();
    }
    if (bad && tid == 0) a.status[g] = CESX_ENOTPD;
    // 2. one 16-row block per wave: item 0 is the diagonal block itself, 1 .. NB-k-1 the rows k + item of Ky, then the rows
    //    0 .. k of the identity underneath
    const int item = (int)blockIdx.x * GF_NW + wave;
    const bool isA = item < NB - k;
    const int i = isA ? k + item : item - (NB - k);
    const bool work = item >= 1 && item <= NB;
    double* M = isA ? A : W;
    if (item == 0) {
        for (int e = lane; e < 256; e += 64) {
            const int r = e >> 4, c = e & 15;
            a.Ld[((size_t)g * Jp + 16 * k + r) * 16 + c] = c <= r ? D[r][c] : 0.0;
        }
    }
    if (work) {
        gf_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        const double* rowi = M + (size_t)(16 * i + m) * Jp + 4 * q;
        gf_mac_blocks(rowi, rowk, isA ? 0 : i, k, acc0, acc1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = q + 4 * r;
            const double base = isA ? A[(size_t)(16 * i + row) * Jp + 16 * k + m] : (i == k && row == m ? 1.0 : 0.0);
            S[wave][row][m] = base - (acc0[r] + acc1[r]);
        }
    }
    __syncthreads();
    if (work && lane < 16) {
        // X L_kk^T = T, row `lane` of it: x_c = (t_c - sum_{c' < c} x_c' L_kk[c][c']) / L_kk[c][c]
        double x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            double t = S[wave][lane][c];
#pragma unroll
            for (int cc = 0; cc < c; ++cc) t = fma(-x[cc], D[c][cc], t);
            x[c] = t / D[c][c];
        }
        double* dst = M + (size_t)(16 * i + lane) * Jp + 16 * k;
#pragma unroll
        for (int c = 0; c < 16; c += 4) {
            const gf_d4 v = {x[c], x[c + 1], x[c + 2], x[c + 3]};
            *reinterpret_cast<gf_d4*>(dst + c) = v;
        }
    }
}

__global__ __launch_bounds__(GF_THREADS)
void gpfit_kinv_kernel(const GpFitArgs a) {
    const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = a.idx[blockIdx.y];
    const int Jp = a.Jp, NB = a.NB;
    const int item = (int)blockIdx.x * GF_NW + wave;
    if (item >= NB * (NB + 1) / 2) return;
    int ba, bb;
    gf_tile(item, ba, bb);
    const double* W = a.W + (size_t)g * Jp * Jp;
    const double* ra = W + (size_t)(16 * ba + m) * Jp + 4 * q;
    const double* rb = W + (size_t)(16 * bb + m) * Jp + 4 * q;
    gf_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    gf_mac_blocks(ra, rb, ba, NB, acc0, acc1);
    double* Ki = a.Ki + (size_t)g * Jp * Jp;
#pragma unroll
    for (int r = 0; r < 4; ++r) Ki[(size_t)(16 * ba + q + 4 * r) * Jp + 16 * bb + m] = acc0[r] + acc1[r];
}

// t_k = sum_{a <= k} W[a][k] r_a, one thread per k (a serial chain of up to Jp fmas per thread: nothing at the tuned sizes,
// J_t <= 1024, where it is a few us of the evaluation; at the largest J_t cesx_gpfit_set accepts it is the slow way to do it)
__global__ __launch_bounds__(GF_THREADS)
void gpfit_tvec_kernel(const GpFitArgs a) {
    const int g = a.idx[blockIdx.y];
    const int k = blockIdx.x * GF_THREADS + threadIdx.x, Jp = a.Jp;
    if (k >= Jp) return;
    const double* W = a.W + (size_t)g * Jp * Jp;
    const double* r = a.res + (size_t)g * Jp;
    double t = 0.0;
#pragma unroll 8
    for (int i = 0; i <= k; ++i) t = fma(W[(size_t)i * Jp + k], r[i], t);
    a.tv[(size_t)g * Jp + k] = t;
}

// alpha_a = sum_{k >= a} W[a][k] t_k, one wave per row
__global__ __launch_bounds__(GF_THREADS)
void gpfit_alpha_kernel(const GpFitArgs a) {
    const int g = a.idx[blockIdx.y];
    const int lane = threadIdx.x & 63, Jp = a.Jp;
    const int row = blockIdx.x * GF_NW + (threadIdx.x >> 6);
    if (row >= Jp) return;
    const double* w = a.W + (size_t)g * Jp * Jp + (size_t)row * Jp;
    const double* t = a.tv + (size_t)g * Jp;
    double s = 0.0;
    for (int k = (row & ~63) + lane; k < Jp; k += 64)
        if (k >= row) s = fma(w[k], t[k], s);
    s = gf_wave_sum(s);
    if (lane == 0) a.alpha[(size_t)g * Jp + row] = s;
}

__global__ __launch_bounds__(GF_THREADS)
void gpfit_grad_kernel(const GpFitArgs a) {
    __shared__ double red[GF_NW];
    const int g = a.idx[blockIdx.y];
    const double* th = a.theta + (size_t)blockIdx.y * a.ntheta;
    const double s2 = th[0];
    int ta, tb;
    gf_tile((int)blockIdx.x, ta, tb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, p = a.p, Jp = a.Jp, Jt = a.Jt;
    const double* Xs = a.Xs + (size_t)g * Jp * p;
    const double* Ki = a.Ki + (size_t)g * Jp * Jp;
    const double* al = a.alpha + (size_t)g * Jp;
    double* out = a.part + ((size_t)g * a.ntile + blockIdx.x) * a.nacc;
    for (int c0 = 0; c0 < a.nl; c0 += GF_DC) {
        double acc[GF_DC];
#pragma unroll
        for (int u = 0; u < GF_DC; ++u) acc[u] = 0.0;
        double sf = 0.0, tr = 0.0;
#pragma unroll 1
        for (int ii = 0; ii < 4; ++ii) {
            const int ra = ta * GF_TILE + ty + 16 * ii;
            if (ra >= Jt) continue;
            const double* xa = Xs + (size_t)ra * p;
            const double ala = al[ra];
#pragma unroll 1
            for (int jj = 0; jj < 4; ++jj) {
                const int cb = tb * GF_TILE + tx + 16 * jj;
                if (cb > ra) continue;
                const double* xb = Xs + (size_t)cb * p;
                double d2 = 0.0;
                for (int d = 0; d < p; ++d) { const double df = xa[d] - xb[d]; d2 = fma(df, df, d2); }
                double f, gq;
                gf_kern(a.family, d2, f, gq);
                const double Q = ala * al[cb] - Ki[(size_t)ra * Jp + cb];
                const double wQ = ra == cb ? Q : 2.0 * Q;
                if (c0 == 0) {
                    sf = fma(wQ, f, sf);
                    if (ra == cb) tr += Q;
                }
                const double wg = wQ * (s2 * gq);
                if (a.ard) {
#pragma unroll
                    for (int u = 0; u < GF_DC; ++u)
                        if (c0 + u < p) { const double df = xa[c0 + u] - xb[c0 + u]; acc[u] = fma(wg, df * df, acc[u]); }
                } else {
                    acc[0] = fma(wg, d2, acc[0]);
                }
            }
        }
        if (c0 == 0) {
            sf = gf_block_sum(sf, red);
            tr = gf_block_sum(tr, red);
            if (threadIdx.x == 0) { out[0] = sf; out[1 + a.nl] = tr; }
        }
#pragma unroll
        for (int u = 0; u < GF_DC; ++u) {
            if (c0 + u < a.nl) {                                    // (uniform: the barriers inside are safe)
                const double s = gf_block_sum(acc[u], red);
                if (threadIdx.x == 0) out[1 + c0 + u] = s;
            }
        }
    }
}

// one workgroup per GP of the batch; wave w takes the sums w, w + 4, ...:
//   0 sum log L_aa, 1 r^T alpha, 2 .. 2 + nm: the mean's gradient, then the nacc sums of the gradient pass over the tiles
__global__ __launch_bounds__(GF_THREADS)
void gpfit_final_kernel(const GpFitArgs a) {
    __shared__ double lm[2];
    const int g = a.idx[blockIdx.y];
    const double* th = a.theta + (size_t)blockIdx.y * a.ntheta;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Jp = a.Jp, Jt = a.Jt, p = a.p, nl = a.nl;
    const int nm = a.ntheta - nl - 2;
    const double* A = a.A + (size_t)g * Jp * Jp;
    const double* al = a.alpha + (size_t)g * Jp;
    const double* r = a.res + (size_t)g * Jp;
    const double* part = a.part + (size_t)g * a.ntile * a.nacc;
    double* out = a.out + (size_t)blockIdx.y * (2 + a.ntheta);
    for (int s = wave; s < 2 + nm + a.nacc; s += GF_NW) {
        double v = 0.0;
        if (s == 0) {
            for (int i = lane; i < Jt; i += 64) v += log(a.Ld[((size_t)g * Jp + i) * 16 + (i & 15)]);
        } else if (s == 1) {
            for (int i = lane; i < Jt; i += 64) v = fma(r[i], al[i], v);
        } else if (s < 2 + nm) {
            const int d = s - 2;                                   // Linear: A_0 .. A_{p-1}, b; Constant: c
            if (a.mean == 2 && d < p) { for (int i = lane; i < Jt; i += 64) v = fma(a.X[(size_t)i * p + d], al[i], v); }
            else { for (int i = lane; i < Jt; i += 64) v += al[i]; }
        } else {
            const int u = s - 2 - nm;
            for (int t = lane; t < a.ntile; t += 64) v += part[(size_t)t * a.nacc + u];
        }
        v = gf_wave_sum(v);
        if (lane == 0) {
            if (s < 2) lm[s] = v;
            else if (s < 2 + nm) out[2 + nl + 2 + (s - 2)] = v;
            else {
                const int u = s - 2 - nm;
                if (u == 0 || u == 1 + nl) out[2 + u] = 0.5 * v;
                else out[2 + u] = -0.5 * v / th[1 + (u - 1)];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = -0.5 * lm[1] - lm[0] - 0.5 * (double)Jt * 1.8378770664093453;      // log 2 pi
        out[1] = (double)a.status[g];
    }
}

int launch_gpfit_eval(Engine& e, int n_active, hipStream_t s) {
    GpFitArgs a{};
    a.Jt = e.gf.Jt; a.Jp = e.gf.Jp; a.NB = e.gf.Jp / 16; a.p = e.p;
    a.family = e.gf.family; a.ard = e.gf.ard; a.mean = e.gf.mean; a.nl = e.gf.nl; a.ntheta = e.gf.ntheta;
    a.ntile = e.gf.ntile; a.nacc = e.gf.nl + 2;
    a.idx = e.gf.idx; a.theta = e.gf.theta; a.X = e.gf.X; a.Y = e.gf.Y;
    a.Xs = e.gf.Xs; a.res = e.gf.r; a.tv = e.gf.t; a.alpha = e.gf.alpha;
    a.A = e.gf.A; a.W = e.gf.W; a.Ki = e.gf.Ki; a.Ld = e.gf.Ld; a.part = e.gf.part; a.status = e.gf.status; a.out = e.gf.out;
    const unsigned ny = (unsigned)n_active, NB = (unsigned)a.NB;
    const dim3 blk(GF_THREADS);
    hipLaunchKernelGGL(gpfit_prep_kernel, dim3((a.Jp + GF_THREADS - 1) / GF_THREADS, ny), blk, 0, s, a);
    hipLaunchKernelGGL(gpfit_build_kernel, dim3((unsigned)a.ntile, ny), blk, 0, s, a);
    for (int k = 0; k < a.NB; ++k)
        hipLaunchKernelGGL(gpfit_chol_kernel, dim3((NB + GF_NW) / GF_NW, ny), blk, 0, s, a, k);
    hipLaunchKernelGGL(gpfit_kinv_kernel, dim3((NB * (NB + 1) / 2 + GF_NW - 1) / GF_NW, ny), blk, 0, s, a);
    hipLaunchKernelGGL(gpfit_tvec_kernel, dim3((a.Jp + GF_THREADS - 1) / GF_THREADS, ny), blk, 0, s, a);
    hipLaunchKernelGGL(gpfit_alpha_kernel, dim3((a.Jp + GF_NW - 1) / GF_NW, ny), blk, 0, s, a);
    hipLaunchKernelGGL(gpfit_grad_kernel, dim3((unsigned)a.ntile, ny), blk, 0, s, a);
    hipLaunchKernelGGL(gpfit_final_kernel, dim3(1, ny), blk, 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

int gpfit_tiles(int Jp) {
    const int nt = (Jp + GF_TILE - 1) / GF_TILE;
    return nt * (nt + 1) / 2;
}

}  // namespace cesx
