// Streaming marginals of the chains' draws (cesx_chain_hist_*, include/cesx.h): a histogram of every row and a 2-D histogram
// of chosen pairs of rows of MCMC(..., chains=M, summary=True, marginals=...), counted from a launch's trace while it is in
// device memory -- the input of kernels_chainsum.hip.  The bin rule is fp64 (an fp32 draw converts exactly) and the edge
// array has the last word (ch_bin), so the counts are numpy.histogram's; counts are integers, so they are exact however the
// run is cut into launches and in whatever order the workgroups finish.
//
//   chain_hist1_kernel   grid (slabs of chains, groups of CH_RB rows, chunks of draws).  A lane takes a chain of the slab and
//                        walks the chunk's draws, CH_DU draws of CH_RB rows in flight; a wave's loads are contiguous along J.
//                        Counts go to the workgroup's LDS histogram, B + 2 uint32 per row (the bins, below, above), the rows'
//                        edges beside it.  A lane keeps the bin of its last draw and the length of the run in registers and
//                        adds to LDS when the bin changes: a chain that rejects repeats its state, and a concentrated
//                        posterior costs one LDS atomic per run, not per draw.
//   chain_hist2_kernel   grid (slabs, pairs, chunks of draws): the same over the two rows of a pair, B2 x B2 uint32 in LDS
//                        (16 KiB at B2 = 64) and the pair's two edge rows; the outside count stays in registers.
// Both flush once: every non-zero LDS counter is added to the run's unsigned long long totals with a global 64-bit integer
// atomic.  A launch's 32-bit counters cannot overflow: a workgroup sees at most slab_cols x the launch's draws, and
// chainhist_add cuts a trace into launches of at most CH_LAUNCH_DRAWS draws.
#include "cesx_internal.h"

namespace cesx {

constexpr int CH_THREADS = 256;
constexpr int CH_RB = 4;               // rows per workgroup of chain_hist1_kernel
constexpr int CH_DU = 4;               // draws in flight per lane and row
constexpr int CH_SLAB = 4096;          // most chains per slab
constexpr int CH_WGS = 1024;           // the workgroups a launch aims at
constexpr int CH_DMIN = 32;            // fewest draws of a chunk, where the draws are cut to reach CH_WGS
constexpr int CH_B = CESX_CHAIN_HIST_BINS_MAX, CH_B2 = CESX_CHAIN_HIST_BINS2D_MAX;
constexpr long long CH_LAUNCH_DRAWS = 0xffffffffll / CH_SLAB;     // slab_cols x draws stays below 2^32

// The bin of x among the strictly increasing edges e[0 .. B] (LDS): 0 .. B - 1 inside, B below, B + 1 above.  e[k] <= x <
// e[k + 1], x == e[B] in bin B - 1; x < e[0] and -inf below; x > e[B], +inf and NaN above.  The guess is that of uniform
// edges; it stands only where the edge array confirms it, otherwise a bisection of the edges finds the bin.
__device__ __forceinline__ int ch_bin(double x, const double* e, int B, double e0, double eB, double scale) {
    if (x < e0) return B;
    if (!(x <= eB)) return B + 1;
    const double t = fmin(fmax((x - e0) * scale, 0.0), (double)(B - 1));      // (fmax drops a NaN of 0 x inf)
    int k = (int)t;
    if (!(e[k] <= x && x < e[k + 1])) {
        int lo = 0, hi = B - 1;                                               // the largest k <= B - 1 with e[k] <= x (e[0] <= x)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (e[mid] <= x) lo = mid; else hi = mid - 1;
        }
        k = lo;
    }
    return k;
}

// edges [p][B + 1]; tot [p][B + 2]
template <typename T>
__global__ __launch_bounds__(CH_THREADS)
void chain_hist1_kernel(const T* __restrict__ trace, int kept, int p, long long J, int slab_cols, int dchunk, int B,
                        const double* __restrict__ edges, unsigned long long* __restrict__ tot) {
    __shared__ double ed[CH_RB * (CH_B + 1)];
    __shared__ unsigned cnt[CH_RB * (CH_B + 2)];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * CH_RB;
    const int nr = p - r0 < CH_RB ? p - r0 : CH_RB;
    const int E = B + 1, C = B + 2;                       // the rows of a group lie back to back in both arrays, as in memory
    for (int i = tid; i < nr * E; i += CH_THREADS) ed[i] = edges[(size_t)r0 * E + i];
    for (int i = tid; i < nr * C; i += CH_THREADS) cnt[i] = 0u;
    __syncthreads();
    double e0[CH_RB], eB[CH_RB], sc[CH_RB];
#pragma unroll
    for (int q = 0; q < CH_RB; ++q) {
        const int qq = q < nr ? q : 0;
        e0[q] = ed[qq * E]; eB[q] = ed[qq * E + B];
        sc[q] = (double)B / (eB[q] - e0[q]);
    }
    const long long j0 = (long long)blockIdx.x * slab_cols;
    const long long j1 = j0 + slab_cols < J ? j0 + slab_cols : J;
    const int d_lo = blockIdx.z * dchunk;
    const int d_hi = d_lo + dchunk < kept ? d_lo + dchunk : kept;
    const size_t sJ = (size_t)J, pJ = (size_t)p * sJ;
    for (long long j = j0 + tid; j < j1; j += CH_THREADS) {
        int last[CH_RB];
        unsigned run[CH_RB];
#pragma unroll
        for (int q = 0; q < CH_RB; ++q) { last[q] = 0; run[q] = 0u; }
        for (int d = d_lo; d < d_hi; d += CH_DU) {
            T v[CH_DU][CH_RB];
#pragma unroll
            for (int u = 0; u < CH_DU; ++u)
#pragma unroll
                for (int q = 0; q < CH_RB; ++q)
                    v[u][q] = (q < nr && d + u < d_hi) ? trace[(size_t)(d + u) * pJ + (size_t)(r0 + q) * sJ + (size_t)j] : (T)0;
#pragma unroll
            for (int u = 0; u < CH_DU; ++u)
#pragma unroll
                for (int q = 0; q < CH_RB; ++q)
                    if (q < nr && d + u < d_hi) {
                        const int k = ch_bin((double)v[u][q], ed + q * E, B, e0[q], eB[q], sc[q]);
                        if (k == last[q]) {
                            ++run[q];
                        } else {
                            if (run[q]) atomicAdd(&cnt[q * C + last[q]], run[q]);
                            last[q] = k; run[q] = 1u;
                        }
                    }
        }
#pragma unroll
        for (int q = 0; q < CH_RB; ++q)
            if (q < nr && run[q]) atomicAdd(&cnt[q * C + last[q]], run[q]);
    }
    __syncthreads();
    for (int i = tid; i < nr * C; i += CH_THREADS) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(&tot[(size_t)r0 * C + i], (unsigned long long)c);
    }
}

// edges2 [pair][2][B + 1]; pairs [pair][2]; tot2 [pair][B][B], row = the bin of the pair's first row; out2 [pair]
template <typename T>
__global__ __launch_bounds__(CH_THREADS)
void chain_hist2_kernel(const T* __restrict__ trace, int kept, int p, long long J, int slab_cols, int dchunk, int B,
                        const double* __restrict__ edges2, const int* __restrict__ pairs, unsigned long long* __restrict__ tot2,
                        unsigned long long* __restrict__ out2) {
    __shared__ double ed[2 * (CH_B2 + 1)];
    __shared__ unsigned cnt[CH_B2 * CH_B2];
    const int tid = threadIdx.x, pair = blockIdx.y;
    const int E = B + 1, cells = B * B;
    const size_t ra = (size_t)pairs[2 * pair], rb = (size_t)pairs[2 * pair + 1];
    for (int i = tid; i < 2 * E; i += CH_THREADS) ed[i] = edges2[(size_t)pair * 2 * E + i];
    for (int i = tid; i < cells; i += CH_THREADS) cnt[i] = 0u;
    __syncthreads();
    const double a0 = ed[0], aB = ed[B], as = (double)B / (aB - a0);
    const double b0 = ed[E], bB = ed[E + B], bs = (double)B / (bB - b0);
    const long long j0 = (long long)blockIdx.x * slab_cols;
    const long long j1 = j0 + slab_cols < J ? j0 + slab_cols : J;
    const int d_lo = blockIdx.z * dchunk;
    const int d_hi = d_lo + dchunk < kept ? d_lo + dchunk : kept;
    const size_t sJ = (size_t)J, pJ = (size_t)p * sJ;
    unsigned long long outside = 0ull;
    for (long long j = j0 + tid; j < j1; j += CH_THREADS) {
        int last = -1;                                    // a cell, or -1: outside
        unsigned run = 0u;
        for (int d = d_lo; d < d_hi; d += CH_DU) {
            T va[CH_DU], vb[CH_DU];
#pragma unroll
            for (int u = 0; u < CH_DU; ++u) {
                const bool ok = d + u < d_hi;
                va[u] = ok ? trace[(size_t)(d + u) * pJ + ra * sJ + (size_t)j] : (T)0;
                vb[u] = ok ? trace[(size_t)(d + u) * pJ + rb * sJ + (size_t)j] : (T)0;
            }
#pragma unroll
            for (int u = 0; u < CH_DU; ++u)
                if (d + u < d_hi) {
                    const int ka = ch_bin((double)va[u], ed, B, a0, aB, as);
                    const int kb = ch_bin((double)vb[u], ed + E, B, b0, bB, bs);
                    const int cell = (ka < B && kb < B) ? ka * B + kb : -1;
                    if (cell == last) {
                        ++run;
                    } else {
                        if (last >= 0) atomicAdd(&cnt[last], run); else outside += run;
                        last = cell; run = 1u;
                    }
                }
        }
        if (last >= 0) atomicAdd(&cnt[last], run); else outside += run;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) outside += __shfl_down(outside, o, 64);
    if ((tid & 63) == 0 && outside) atomicAdd(&out2[pair], outside);
    __syncthreads();
    for (int i = tid; i < cells; i += CH_THREADS) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(&tot2[(size_t)pair * cells + i], (unsigned long long)c);
    }
}

// ---------------------------------------------------------------------------
// The launch plan, from the shape alone: slabs of whole workgroup passes (multiples of CH_THREADS chains, at most CH_SLAB) that
// bring the launch to CH_WGS workgroups; where the slabs and groups alone fall short, the draws are cut into chunks of no
// fewer than CH_DMIN (a multiple of CH_DU).
struct ChPlan { int slab_cols, slabs, dchunk, nz; };
static ChPlan ch_plan(long long J, int groups, int kept) {
    const long long most = (J + CH_THREADS - 1) / CH_THREADS, least = (J + CH_SLAB - 1) / CH_SLAB;
    long long want = (CH_WGS + groups - 1) / groups;
    want = want < least ? least : (want > most ? most : want);
    long long cols = ((J + want - 1) / want + CH_THREADS - 1) / CH_THREADS * CH_THREADS;
    if (cols > CH_SLAB) cols = CH_SLAB;
    ChPlan pl;
    pl.slab_cols = (int)cols;
    pl.slabs = (int)((J + cols - 1) / cols);
    long long nz = CH_WGS / ((long long)pl.slabs * groups);
    const long long zmax = (kept + CH_DMIN - 1) / CH_DMIN;
    nz = nz < 1 ? 1 : (nz > zmax ? zmax : nz);
    pl.dchunk = (int)(((kept + nz - 1) / nz + CH_DU - 1) / CH_DU * CH_DU);
    pl.nz = (kept + pl.dchunk - 1) / pl.dchunk;
    return pl;
}

// the descriptor has been checked (cesx_chain_hist_begin): from here on only a device call can fail
int chainhist_begin(Engine& e, const cesx_chain_hist_desc* d, hipStream_t s) {
    ChainHistState& ch = e.ch;
    const size_t p = (size_t)e.p, B = (size_t)d->bins, B2 = (size_t)d->bins2d, np = (size_t)d->n_pairs;
    TRY_BUF(ch.edges1.ensure(p * (CH_B + 1) * 8, false));
    TRY_BUF(ch.tot1.ensure(p * (CH_B + 2) * 8, false));
    TRY_BUF(ch.edges2.ensure((size_t)CESX_CHAIN_HIST_PAIRS_MAX * 2 * (CH_B2 + 1) * 8, false));
    TRY_BUF(ch.pairs.ensure((size_t)CESX_CHAIN_HIST_PAIRS_MAX * 2 * 4, false));
    TRY_BUF(ch.tot2.ensure((size_t)CESX_CHAIN_HIST_PAIRS_MAX * (CH_B2 * CH_B2 + 1) * 8, false));
    CESX_HIP(hipStreamSynchronize(s));                    // an earlier run's adds read the edges and add to the totals
    // Only a device error can fail from here on (CESX_EHIP, not one of the refusals the header lists); the earlier run is
    // dropped first, so after such an error no run is in hand: add and read return CESX_ESTATE until the next begin.
    ch.drop();
    CESX_HIP(hipMemcpy(ch.edges1, d->edges1, p * (B + 1) * 8, hipMemcpyHostToDevice));
    CESX_HIP(hipMemsetAsync(ch.tot1, 0, p * (B + 2) * 8, s));
    if (np) {
        std::vector<double> e2(np * 2 * (B2 + 1));
        for (size_t k = 0; k < np; ++k)
            for (int h = 0; h < 2; ++h)
                for (size_t i = 0; i <= B2; ++i) e2[(k * 2 + h) * (B2 + 1) + i] = d->edges2[(size_t)d->pairs[2 * k + h] * (B2 + 1) + i];
        CESX_HIP(hipMemcpy(ch.edges2, e2.data(), e2.size() * 8, hipMemcpyHostToDevice));
        CESX_HIP(hipMemcpy(ch.pairs, d->pairs, np * 2 * 4, hipMemcpyHostToDevice));
        CESX_HIP(hipMemsetAsync(ch.tot2, 0, np * (B2 * B2 + 1) * 8, s));
    }
    ch.bins = d->bins; ch.bins2 = d->bins2d; ch.n_pairs = d->n_pairs;
    return CESX_OK;
}

template <typename T>
static int chainhist_add_t(Engine& e, const void* trace, int kept, hipStream_t s) {
    ChainHistState& ch = e.ch;
    const int p = e.p, groups = (p + CH_RB - 1) / CH_RB;
    const long long J = e.J;
    const size_t B2 = (size_t)ch.bins2;
    for (long long d0 = 0; d0 < kept; d0 += CH_LAUNCH_DRAWS) {
        const int k = (int)(kept - d0 < CH_LAUNCH_DRAWS ? kept - d0 : CH_LAUNCH_DRAWS);
        const T* t = (const T*)trace + (size_t)d0 * (size_t)p * (size_t)J;
        const ChPlan a = ch_plan(J, groups, k);
        hipLaunchKernelGGL(chain_hist1_kernel<T>, dim3(a.slabs, groups, a.nz), dim3(CH_THREADS), 0, s, t, k, p, J, a.slab_cols, a.dchunk,
                           ch.bins, (const double*)ch.edges1, ch.tot1.get());
        CESX_HIP(hipGetLastError());
        if (ch.n_pairs) {
            const ChPlan b = ch_plan(J, ch.n_pairs, k);
            hipLaunchKernelGGL(chain_hist2_kernel<T>, dim3(b.slabs, ch.n_pairs, b.nz), dim3(CH_THREADS), 0, s, t, k, p, J, b.slab_cols,
                               b.dchunk, ch.bins2, (const double*)ch.edges2, (const int*)ch.pairs, ch.tot2.get(),
                               ch.tot2.get() + (size_t)ch.n_pairs * B2 * B2);
            CESX_HIP(hipGetLastError());
        }
    }
    ch.added += kept;
    return CESX_OK;
}

int chainhist_add(Engine& e, const void* trace, int kept, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? chainhist_add_t<float>(e, trace, kept, s) : chainhist_add_t<double>(e, trace, kept, s);
}

int chainhist_read(Engine& e, unsigned long long* hist1, unsigned long long* out1, unsigned long long* hist2,
                   unsigned long long* out2, hipStream_t s) {
    ChainHistState& ch = e.ch;
    const size_t p = (size_t)e.p, B = (size_t)ch.bins, B2 = (size_t)ch.bins2, np = (size_t)ch.n_pairs;
    CESX_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> t1(p * (B + 2));
    CESX_HIP(hipMemcpy(t1.data(), ch.tot1, t1.size() * 8, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < p; ++r) {
        for (size_t k = 0; k < B; ++k) hist1[r * B + k] = t1[r * (B + 2) + k];
        out1[2 * r] = t1[r * (B + 2) + B];
        out1[2 * r + 1] = t1[r * (B + 2) + B + 1];
    }
    if (np) {
        CESX_HIP(hipMemcpy(hist2, ch.tot2, np * B2 * B2 * 8, hipMemcpyDeviceToHost));
        CESX_HIP(hipMemcpy(out2, ch.tot2.get() + np * B2 * B2, np * 8, hipMemcpyDeviceToHost));
    }
    return CESX_OK;
}

}  // namespace cesx
