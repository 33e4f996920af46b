// The Darcy forward map of kernels_darcy.hip for meshes whose working band no longer fits in LDS (Nmesh up to 64): the same
// five stages and the same arithmetic contract (all fp64, the engine dtype governs only how U is read and G written; gbtf2's
// pivot rule; multipliers applied to the right-hand side as they are formed and never stored; the same status words; no
// trap, no assert), with the banded LU STREAMED: only the rows and columns a column step can touch are resident, every
// finished row of U goes to an HBM workspace slot and comes back for the back substitution.
//
// Live window.  At column step col (m = K - 2, n = m^2) the elimination reads and writes rows col .. col + m and columns
// col .. col + 2 m (kl = m, ku = 2 m after the row swaps) and nothing else.  Row col is final once the step is over.
//
// Ring.  The window lives in LDS as a ring of H = m + 2 row slots and W = 2 m + 2 column slots: A(r, c) at
// win[(c mod W) RS + (r mod H)], RS = H | 1.  That is ONE row slot and ONE column slot more than the live window needs,
// and it is what keeps the step at one barrier: row col + m + 1 and column col + 2 m + 1, which enter the window for step
// col + 1, land on the slots that row col - 1 and column col - 1 left a whole step ago, so they are generated (from the nodal
// field a, straight into the ring) DURING step col, beside the rank-1 update, and not behind a barrier of their own.  The
// entering row is written over all 2 m + 1 columns of the next window, zeros included, and the entering column is zeroed over
// the rows above it: every ring word a step reads was written earlier for THIS particle -- nothing survives the many wraps
// (n >> W), the previous particle of the workgroup or an early exit on a bad pivot.
// Down a column the address step is 1 (pivot search, the rank-1 update's lanes: consecutive banks); along a row it is RS, odd
// (row swap, the finished row on its way out, the entering row: distinct fp64 banks for 32 consecutive columns).
//
// Column step (DARCY_STREAM_THREADS threads = several waves; every barrier below is a real one):
//     pivot search   EVERY wave reads the m + 1 entries of column col, lane = row, and reduces in registers: all waves get the
//                    same pivot row jp and the same verdict without exchanging a word.  The column stays in registers: its
//                    swap, the pivot and the multipliers never go back to LDS (column col is dead after the step).
//     row swap       rows col and col + jp over the columns col + 1 .. ju and in the right-hand side; then a barrier (only
//                    when jp != 0: nothing else has touched those rows since the last barrier)
//     multipliers    l(t) = A(col + t, col) / pivot, each thread its own row's, applied to the right-hand side by one group
//     rank-1 update  lane = g RG + t: row t of column g of the pass, RG the power of two >= m (64 at K = 64, 16 at K = 17)
//     beside it      the finished row col (read-only in this step) goes to the workspace as one contiguous row of 2 m + 1
//                    doubles, diagonal first; the entering row and column are generated
//     barrier
//
// Back substitution.  Row form, last row first: x(r) = (b(r) - sum_k U(r, r + k) x(r + k)) / U(r, r).  The finished rows come
// back in chunks of as many whole rows as the ring's LDS holds, prefetched into registers by all waves while wave 0 solves
// the chunk before; a row's sum is lane-strided partial sums (k = 1 + lane, + 64) folded by an xor butterfly: the order is a
// function of (m, n) alone, so a particle's result depends neither on the grid nor on the slot nor on the chunking.
// The workspace words were written by other waves of the same workgroup: every storing wave waits for its stores
// (s_waitcnt vmcnt(0)) and the workgroup meets at a barrier before the first of them is loaded.  A slot belongs to ONE
// workgroup for the whole launch (slot = blockIdx.x), so no word ever crosses to another compute unit inside a launch; the
// loads are L2-served all the same (ds_ws_load), so that nothing rests on what the L1 does with a line its own compute unit
// rewrites -- the slot is rewritten by every particle the workgroup takes.
//
// LDS per workgroup (doubles): a K^2 | right-hand side / x n (+ pad) | ring max(RS W, K^2); the second K x K tile of stages
// 1, 2 and 5 aliases the ring.  K = 64: 32 768 + 30 752 + 65 520 = 129 040 B of the 163 840 a workgroup may take; K = 32:
// 31 760 B.  The mesh limit follows from these sizes and from the pivot search (the ring's H row slots fit one wave's lanes).
#include "cesx_internal.h"

namespace cesx {

#ifndef DARCY_STREAM_THREADS
#define DARCY_STREAM_THREADS 512
#endif
constexpr int DS_THREADS = DARCY_STREAM_THREADS;
constexpr int DS_WAVES = DS_THREADS / 64;
static_assert(DS_THREADS % 64 == 0 && DS_THREADS >= 256 && DS_THREADS <= 1024, "whole waves; the entering row and column take 3 m + 1 <= 187 threads of one pass");
constexpr size_t DS_LDS_MAX = 163840;                    // what one workgroup may take on gfx950

constexpr int ds_H(int K) { return K; }                                  // m + 2 row slots
constexpr int ds_RS(int K) { return K | 1; }
constexpr int ds_W(int K) { return 2 * K - 2; }                          // 2 m + 2 column slots
constexpr int ds_win(int K) { return ds_RS(K) * ds_W(K) > K * K ? ds_RS(K) * ds_W(K) : K * K; }
constexpr int ds_npad(int K) { return ((K - 2) * (K - 2) + 1) & ~1; }
constexpr size_t ds_lds(int K) { return (size_t)(K * K + ds_npad(K) + ds_win(K)) * 8; }
constexpr int ds_kmax() {
    int K = 4;
    while (ds_lds(K + 1) <= DS_LDS_MAX && ds_H(K + 1) <= 64) ++K;         // LDS; the ring's row slots within one wave's lanes
    return K;
}
constexpr int DS_KMAX = ds_kmax();
static_assert(DS_KMAX == CESX_DARCY_STREAM_KMAX, "include/cesx.h documents the limit this file derives");
constexpr int DS_PF = (ds_win(DS_KMAX) + DS_THREADS - 1) / DS_THREADS;   // doubles of a back-substitution chunk per thread

size_t darcy_stream_lds(int K) { return ds_lds(K); }
int darcy_stream_kmax() { return DS_KMAX; }
size_t darcy_stream_slot_bytes(int K) { const size_t m = K - 2; return m * m * (2 * m + 1) * 8; }

// A finished row on its way back: an L2-served load (global_load ... sc1), so that what the back substitution reads never
// depends on what this compute unit's L1 kept of the slot's previous tenant (the particle this workgroup solved before).
__device__ inline double ds_ws_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct DarcyStreamArgs {
    const void* U; void* G; int* status; int J;
    int K, p, n_obs, rg_log2;
    const double* mat;                                    // [4][K][K] coef, D, S, R (DarcyState::mat)
    const int* idx;                                       // [p] scatter, [n_obs] obs_index (DarcyState::idx)
    double* ws;                                           // gridDim.x slots of n (2 m + 1) doubles
};

__device__ inline void ds_left(double* out, const double* __restrict__ M, const double* in, int K, int tid) {
    for (int e = tid; e < K * K; e += DS_THREADS) {
        const int i = e / K, c = e - i * K;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(M[i * K + k], in[k * K + c], s);
        out[e] = s;
    }
}

template <bool EXP>
__device__ inline void ds_right(double* out, const double* in, const double* __restrict__ M, int K, int tid) {
    for (int e = tid; e < K * K; e += DS_THREADS) {
        const int i = e / K, c = e - i * K;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(in[i * K + k], M[c * K + k], s);
        out[e] = EXP ? exp(s) : s;
    }
}

// A(r, c) of the 5-point operator from the nodal field (row r = interior node (i, jj), unknowns column by column)
__device__ inline double ds_entry(const double* a, int K, int m, double h2, int i, int jj, int d) {
    const double cc = a[i * K + jj];
    const double w = (a[(i - 1) * K + jj] + cc) / 2, e = (a[(i + 1) * K + jj] + cc) / 2;
    const double s = (a[i * K + jj - 1] + cc) / 2, nn = (a[i * K + jj + 1] + cc) / 2;
    if (d == 0) return (w + e + s + nn) * h2;
    if (d == -1 && i > 1) return -w * h2;
    if (d == 1 && i < m) return -e * h2;
    if (d == -m && jj > 1) return -s * h2;
    if (d == m && jj < m) return -nn * h2;
    return 0.0;
}

// The geometry of one phase, from K read behind an empty asm.  Each phase of a particle derives its own copy: the compiler
// otherwise forms every loop-invariant scalar of every phase (division constants, byte offsets, "tid < ..." masks) once, in
// front of the persistent loop, and keeps them all live through the LU -- 72 scalar registers spilled that way.
#define DS_GEOMETRY                                                                                                      \
    int K = a.K, tid = threadIdx.x;                                                                                      \
    asm volatile("" : "+s"(K), "+v"(tid));                                                                               \
    [[maybe_unused]] const int m = K - 2, n = m * m, kv = 2 * m, KK = K * K;                                             \
    [[maybe_unused]] const int H = m + 2, RS = H | 1, W = 2 * m + 2, W0 = 2 * m + 1;                                     \
    [[maybe_unused]] double* t0 = ds_smem;            /* K x K: L, exp(theta), then the nodal field a (kept through the LU) */ \
    [[maybe_unused]] double* rhs = ds_smem + KK;      /* n: the right-hand side, then x */                                \
    [[maybe_unused]] double* win = rhs + ((n + 1) & ~1);      /* the ring; the second K x K tile and the chunk buffer alias it */ \
    [[maybe_unused]] double* t1 = win;                                                                                   \
    [[maybe_unused]] const double h2 = (double)((K - 1) * (K - 1))

template <typename T>
__global__ __launch_bounds__(DS_THREADS)
void darcy_stream_lu(const DarcyStreamArgs a) {
    extern __shared__ double ds_smem[];
    const T* U = (const T*)a.U;
    T* G = (T*)a.G;

    for (int j = blockIdx.x; j < a.J; j += gridDim.x) {
        int info = 0;
        {
        DS_GEOMETRY;
        // ---- 1: KL synthesis ----
        for (int e = tid; e < KK; e += DS_THREADS) t0[e] = 0.0;
        __syncthreads();
        for (int q = tid; q < a.p; q += DS_THREADS) {
            const int s = a.idx[q];
            t0[s] = a.mat[s] * (double)U[(size_t)q * a.J + j];
        }
        __syncthreads();
        if (tid == 0) t0[0] = 0.0;                        // the constant mode is removed (gaussrnd_coarse.m:21)
        __syncthreads();
        ds_left(t1, a.mat + KK, t0, K, tid);
        __syncthreads();
        ds_right<true>(t0, t1, a.mat + KK, K, tid);              // exp(theta)
        __syncthreads();
        // ---- 2: to the nodes ----
        ds_left(t1, a.mat + 2 * KK, t0, K, tid);
        __syncthreads();
        ds_right<false>(t0, t1, a.mat + 2 * KK, K, tid);            // a (K x K) at the nodes
        __syncthreads();
        // ---- 3: the first window, rows 0 .. m and columns 0 .. 2 m, zeros included; the right-hand side ----
        {
            const int nr = min(m + 1, n), ncw = min(W0, n);
            for (int e = tid; e < nr * ncw; e += DS_THREADS) {
                const int c = e / nr, r = e - c * nr;     // (r < H, c < W: the slots are r and c themselves)
                const int jj = r / m + 1, i = r - (jj - 1) * m + 1;
                win[c * RS + r] = ds_entry(t0, K, m, h2, i, jj, c - r);
            }
            for (int q = tid; q < n; q += DS_THREADS) rhs[q] = 1.0;      // (the spline of the constant 1 is 1)
        }
        __syncthreads();
        }
        {
        // ---- 4: banded LU with partial pivoting over the ring, the right-hand side eliminated along ----
        DS_GEOMETRY;
        double* wsp = a.ws + (size_t)blockIdx.x * (size_t)n * W0;
        const int RG = 1 << a.rg_log2, CP = DS_THREADS >> a.rg_log2;
        const int lane = tid & 63, tu = (tid & (RG - 1)) + 1, gu = tid >> a.rg_log2;
        int ju = 0;
        int rs0 = 0, cs0 = 0;                             // ring slots of row col and of column col
        int ei = 0, ejj = 0;                              // the entering row r = col + m + 1 as interior node (ei, ejj)
        { const int r = m + 1; ejj = r / m + 1; ei = r - (ejj - 1) * m + 1; }
        for (int col = 0; col < n; ++col) {
            const int km = min(m, n - 1 - col);
            // pivot search, in every wave alike: lane = row offset
            const bool in_col = lane <= km;
            int rsl = rs0 + lane; if (rsl >= H) rsl -= H;
            const double cv = in_col ? win[cs0 * RS + rsl] : 0.0;
            const double av = in_col ? fabs(cv) : -1.0;
            double mx = av;
            for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
            const unsigned long long hit = __ballot(in_col && av == mx);
            // a NaN never wins fmax and an infinity is no pivot to divide by: any non-finite entry of the pivot column ends the particle
            const unsigned long long nonfin = __ballot(in_col && !(av <= 1.7976931348623157e308));
            if (nonfin != 0ull || hit == 0ull) { info = -(col + 1); break; }
            if (!(mx > 0.0)) { info = col + 1; break; }
            const int jp = __ffsll((long long)hit) - 1;   // the first largest entry, as idamax
            ju = max(ju, min(col + m + jp, n - 1));
            const int nc = ju - col;                      // columns right of col this step touches (<= 2 m)
            const double piv = __shfl(cv, jp, 64);
            const double top = __shfl(cv, 0, 64);
            const double cvs = (lane == jp) ? top : cv;   // column col below the diagonal after the swap, in registers
            const double lsrc = __shfl(cvs, tu & 63, 64); // this thread's update row
            if (jp != 0) {                                // rows col and col + jp over the columns col + 1 .. ju, and in the right-hand side
                int rsp = rs0 + jp; if (rsp >= H) rsp -= H;
                if (tid < nc) {
                    int cs = cs0 + 1 + tid; if (cs >= W) cs -= W;
                    double* pc = win + cs * RS;
                    const double x0 = pc[rs0], x1 = pc[rsp];
                    pc[rs0] = x1; pc[rsp] = x0;
                } else if (tid == DS_THREADS - 1) {       // (nc <= 2 m < DS_THREADS - 1)
                    const double x0 = rhs[col], x1 = rhs[col + jp];
                    rhs[col] = x1; rhs[col + jp] = x0;
                }
                __syncthreads();
            }
            // the finished row col leaves for the workspace: the diagonal, then the columns col + 1 .. col + 2 m
            if (tid < W0) {
                double v = piv;
                if (tid > 0) {
                    int cs = cs0 + tid; if (cs >= W) cs -= W;
                    v = col + tid < n ? win[cs * RS + rs0] : 0.0;
                }
                wsp[(size_t)col * W0 + tid] = v;
            }
            // the row and the column that enter the window for step col + 1, on the slots row col - 1 and column col - 1 left
            {
                const int r = col + m + 1, cnew = col + W0;
                int rsn = rs0 + m + 1; if (rsn >= H) rsn -= H;
                int csn = cs0 + W0; if (csn >= W) csn -= W;
                const int back = DS_THREADS - 1 - tid;    // (from the far end of the workgroup: the front writes the row above)
                if (r < n && back < W0) {                 // A(r, col + 1 + back)
                    const int c = col + 1 + back;
                    int cs = cs0 + 1 + back; if (cs >= W) cs -= W;
                    if (c < n) win[cs * RS + rsn] = ds_entry(t0, K, m, h2, ei, ejj, c - r);
                } else if (cnew < n && back >= W0 && back < W0 + m) {    // A(col + 1 + q, cnew) = 0, q < m: outside the band
                    int rz = rs0 + 1 + (back - W0); if (rz >= H) rz -= H;
                    win[csn * RS + rz] = 0.0;
                }
            }
            if (km > 0) {
                const bool row_on = tu <= km;
                const double l = row_on ? lsrc / piv : 0.0;       // the multipliers: used here, not stored
                int rsu = rs0 + tu; if (rsu >= H) rsu -= H;
                if (row_on && gu == 0) rhs[col + tu] -= l * rhs[col];
                for (int c0 = 1; c0 <= nc; c0 += CP) {
                    const int c = c0 + gu;
                    if (row_on && c <= nc) {
                        int cs = cs0 + c; if (cs >= W) cs -= W;
                        double* pc = win + cs * RS;
                        pc[rsu] -= l * pc[rs0];
                    }
                }
            }
            if (++rs0 == H) rs0 = 0;
            if (++cs0 == W) cs0 = 0;
            if (++ei > m) { ei = 1; ++ejj; }
            __syncthreads();
        }
        }
        // the workspace rows were stored by other waves of this workgroup: each wave waits for its own stores, then the barrier
        __threadfence_block();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        {
        DS_GEOMETRY;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        if (!info) {
            // back substitution, last row first, in chunks of bs_rows whole rows
            const double* wsp = a.ws + (size_t)blockIdx.x * (size_t)n * W0;
            const int bs_rows = max(RS * W, KK) / W0;     // whole rows of U in the ring's LDS
            const int lane = tid & 63, wave = tid >> 6;
            double pre[DS_PF];
            int hi = n - 1, lo = max(0, hi - bs_rows + 1);
#pragma unroll
            for (int q = 0; q < DS_PF; ++q) {
                const int e = tid + q * DS_THREADS;
                pre[q] = ds_ws_load(wsp + (size_t)lo * W0 + min(e, (hi - lo + 1) * W0 - 1));      // (clamped, not predicated)
            }
            while (hi >= 0) {
                const int cnt = (hi - lo + 1) * W0;
#pragma unroll
                for (int q = 0; q < DS_PF; ++q) {
                    const int e = tid + q * DS_THREADS;
                    if (e < cnt) win[e] = pre[q];
                }
                __syncthreads();
                const int nhi = lo - 1, nlo = max(0, nhi - bs_rows + 1);
                if (nhi >= 0) {
#pragma unroll
                    for (int q = 0; q < DS_PF; ++q) {
                        const int e = tid + q * DS_THREADS;
                        pre[q] = ds_ws_load(wsp + (size_t)nlo * W0 + min(e, (nhi - nlo + 1) * W0 - 1));
                    }
                }
                if (wave == 0) {                          // one wave: its LDS accesses execute in program order
                    for (int row = hi; row >= lo; --row) {
                        const double* ur = win + (row - lo) * W0;
                        const int len = min(kv, n - 1 - row);
                        double s = 0.0;
                        for (int k = 1 + lane; k <= len; k += 64) s = fma(ur[k], rhs[row + k], s);
                        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                        if (lane == 0) rhs[row] = (rhs[row] - s) / ur[0];
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                __syncthreads();
                hi = nhi; lo = nlo;
            }
            // ---- 5: back to the picked centres ----
            const double* R = a.mat + 3 * KK;
            for (int e = tid; e < K * m; e += DS_THREADS) {          // W = R[:, 1:-1] X, X[i][jx] = x[jx m + i]
                const int r = e / m, jx = e - r * m;
                double s = 0.0;
                for (int i = 0; i < m; ++i) s = fma(R[r * K + 1 + i], rhs[jx * m + i], s);
                t1[e] = s;
            }
            __syncthreads();
        }
        for (int k = tid; k < a.n_obs; k += DS_THREADS) {
            double g = qnan;
            if (!info) {
                const int o = a.idx[a.p + k], r = o / K, c = o - r * K;     // row-major flatten of the K x K centres
                g = 0.0;
                for (int jx = 0; jx < m; ++jx) g = fma(t1[r * m + jx], a.mat[3 * KK + c * K + 1 + jx], g);
            }
            G[(size_t)k * a.J + j] = (T)g;
        }
        if (a.status && tid == 0) a.status[j] = info;
        }
        __syncthreads();                                  // the next particle's stage 1 overwrites what the outputs read
    }
}

// once per installed map (cesx_darcy_set_streamed): the dynamic LDS limit of both instantiations, and the automatic grid
// (what the occupancy of this K lets run at once; the apply launches min(J, slots) workgroups)
int darcy_stream_prepare(Engine& e, int K, int* auto_grid) {
    const int lds = (int)ds_lds(K);
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(darcy_stream_lu<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(darcy_stream_lu<double>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int per_cu = 0;
    auto kern = e.cfg.dtype == CESX_F32 ? darcy_stream_lu<float> : darcy_stream_lu<double>;
    CESX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, DS_THREADS, (size_t)lds));
    *auto_grid = std::max(1, per_cu) * std::max(1, e.num_cus);
    return CESX_OK;
}

int launch_darcy_stream(Engine& e, const void* U, void* G, int* status, hipStream_t s) {
    DarcyStreamArgs a{};
    const int K = e.dc.K, m = K - 2;
    a.U = U; a.G = G; a.status = status; a.J = (int)e.J;
    a.K = K; a.p = e.p; a.n_obs = e.n;
    a.rg_log2 = 1;
    while ((1 << a.rg_log2) < m) ++a.rg_log2;             // the update's row group: the power of two >= m (<= 64)
    a.mat = e.dc.mat; a.idx = e.dc.idx; a.ws = e.dc.ws;
    const long long grid = std::min<long long>(e.J, e.dc.slots);
    if (e.J + grid >= (1LL << 31)) { e.err = "cesx_darcy_apply: too many particles for one launch"; return CESX_EUNSUPPORTED; }
    if (grid < 1 || e.dc.ws.bytes < (size_t)grid * darcy_stream_slot_bytes(K)) { e.err = "cesx_darcy_apply: the streamed map has no workspace"; return CESX_ESTATE; }
    auto kern = e.cfg.dtype == CESX_F32 ? darcy_stream_lu<float> : darcy_stream_lu<double>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(DS_THREADS), ds_lds(K), s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

}  // namespace cesx
