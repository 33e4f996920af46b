// Streaming summaries of the chains' draws (cesx_chain_summary_*, include/cesx.h): the sums behind the pooled mean and
// covariance, the split R-hat and the effective sample size of MCMC(..., chains=M, summary=True), taken from a launch's
// trace while it is still in device memory.  All arithmetic is fp64 (an fp32 draw converts exactly), every sum runs in a
// fixed order and nothing is added atomically: runs are bit-reproducible.
//
//   chain_half_kernel         one lane per chain, CS_RB rows per workgroup.  Per (row, chain) and half -- the chain's first
//                             n = N / 2 and last n draws -- S1 = sum (x - shift), S2 = sum (x - shift)^2 with shift = the
//                             chain's first draw: the cancellation of the variance is bounded by the chain's own spread.
//                             The sums are loaded from the state, carried in registers through the launch's draws in order
//                             and stored once: however a run is cut into launches, a chain's sums are the same bits.
//   chain_pool_kernel         sum over draws and chains of (x - c)(x - c)^T, c = the row means of the first draw
//                             (rowsum_kernel of kernels_stats.hip).  A workgroup takes a slab of chains (cs_slab_cols) and one 64 x 64
//                             super tile of the lower triangle: tiles of 64 rows x CS_TC chains go through registers (the
//                             next tile's loads fly under this tile's MFMAs) into LDS as x - c, zero past p and past J; wave w
//                             owns block row w of the super tile, up to four 16 x 16 accumulators on v_mfma_f64_16x16x4_f64
//                             (A: lane l holds row l & 15, chain l >> 4; C/D: column l & 15, row (l >> 4) + 4 reg).  Blocks
//                             past p or above the diagonal are not computed.  The diagonal super tiles also sum the rows.
//   chain_pool_reduce_kernel  the slabs' partials in a fixed order, then the earlier launches' total: added last.
//   chain_half_reduce_kernel  per row over the 2 M half-chains: m = shift + S1 / n, s^2 = (S2 - S1^2 / n) / (n - 1), then
//   chain_half_final_kernel   sum (m - c), sum (m - c)^2, sum s^2: CS_CH chains per workgroup, the workgroups in order.
#include "cesx_internal.h"

namespace cesx {

constexpr int CS_THREADS = 256;
constexpr int CS_RB = 4;           // rows per workgroup of chain_half_kernel
constexpr int CS_SLAB = 2048;      // most chains per slab of chain_pool_kernel
constexpr int CS_WGS = 1024;       // the workgroups a pooled launch aims at: narrower slabs where the lower triangle has few super tiles
constexpr int CS_TC = 32;          // chains per staged tile
constexpr int CS_RS = 36;          // doubles per LDS row: 72 words, so rows r and r + 8 meet in a bank and nothing else does
constexpr int CS_CH = 1024;        // chains per workgroup of chain_half_reduce_kernel
constexpr int CS_SLICES = 64;      // most slices of the row sums behind c
constexpr int CS_RE = 8, CS_RL = 32;   // chain_pool_reduce_kernel: entries per workgroup, lanes per entry (CS_RE * CS_RL = CS_THREADS)

typedef double cs_d4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(CS_THREADS)
void chain_half_kernel(const T* __restrict__ trace, int kept, int p, long long J, long long d0, long long N, long long n,
                       double* __restrict__ shift, double* __restrict__ S) {
    const long long j = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (j >= J) return;
    const int r0 = blockIdx.y * CS_RB;
    const int nr = p - r0 < CS_RB ? p - r0 : CS_RB;
    const size_t pj = (size_t)p * (size_t)J;
    // the halves this launch's draws d0 .. d0 + kept - 1 fall into: only their sums are loaded and stored (a run's first
    // launch stores both: the other half's zeros)
    const bool in0 = d0 < n, in1 = d0 + kept > N - n;
    double sh[CS_RB], a[CS_RB][4];
#pragma unroll
    for (int q = 0; q < CS_RB; ++q) {
        sh[q] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) a[q][k] = 0.0;
        if (q < nr) {
            const size_t idx = (size_t)(r0 + q) * (size_t)J + (size_t)j;
            if (d0 == 0) {
                sh[q] = (double)trace[idx];
            } else {
                sh[q] = shift[idx];
                if (in0) { a[q][0] = S[idx]; a[q][1] = S[pj + idx]; }
                if (in1) { a[q][2] = S[2 * pj + idx]; a[q][3] = S[3 * pj + idx]; }
            }
        }
    }
#pragma unroll 4
    for (int d = 0; d < kept; ++d) {
        const long long g = d0 + d;
        const bool h0 = g < n, h1 = g >= N - n;
        if (!h0 && !h1) continue;                       // the middle draw of an odd N
#pragma unroll
        for (int q = 0; q < CS_RB; ++q) {
            if (q < nr) {
                const double v = (double)trace[((size_t)d * p + (size_t)(r0 + q)) * (size_t)J + (size_t)j] - sh[q];
                if (h0) { a[q][0] += v; a[q][1] = fma(v, v, a[q][1]); }
                else    { a[q][2] += v; a[q][3] = fma(v, v, a[q][3]); }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CS_RB; ++q) {
        if (q < nr) {
            const size_t idx = (size_t)(r0 + q) * (size_t)J + (size_t)j;
            if (d0 == 0) shift[idx] = sh[q];
            if (in0 || d0 == 0) { S[idx] = a[q][0]; S[pj + idx] = a[q][1]; }
            if (in1 || d0 == 0) { S[2 * pj + idx] = a[q][2]; S[3 * pj + idx] = a[q][3]; }
        }
    }
}

// c[row] = (sum of the row's slices) / J
__global__ void chain_c_final_kernel(const double* __restrict__ part, int p, int nslices, long long J, double* __restrict__ c) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= p) return;
    double s = 0.0;
    for (int k = 0; k < nslices; ++k) s += part[(size_t)row * nslices + k];
    c[row] = s / (double)J;
}

// grid = (slabs, pairs); pair = si (si + 1) / 2 + sj, sj <= si: super tile (si, sj) of the lower triangle.
// part [slab][pair][64][64]: the blocks this workgroup computes (the rest is never read); part1 [slab][pp]: row sums.
template <typename T>
__global__ __launch_bounds__(CS_THREADS)
void chain_pool_kernel(const T* __restrict__ trace, int kept, int p, long long J, int slab_cols, const double* __restrict__ c, int pairs, int pp,
                       double* __restrict__ part, double* __restrict__ part1) {
    __shared__ double As[64 * CS_RS], Bs[64 * CS_RS];
    const int slab = blockIdx.x, pair = blockIdx.y;
    int si = 0;
    while ((si + 1) * (si + 2) / 2 <= pair) ++si;
    const int sj = pair - si * (si + 1) / 2;
    const bool diag = si == sj;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int lc = tid & (CS_TC - 1), lr = tid / CS_TC;                  // this thread stages rows lr + 8 i of column lc
    const long long j0 = (long long)slab * slab_cols;
    const long long j1 = j0 + slab_cols < J ? j0 + slab_cols : J;
    const int ntile = (int)((j1 - j0 + CS_TC - 1) / CS_TC);
    const long long total = (long long)kept * ntile;
    // rows of A (super tile si) and B (sj) this thread stages: how many of the 8 are below p, and their c
    const int ra0 = 64 * si + lr, rb0 = 64 * sj + lr;
    const int na = ra0 < p ? (p - ra0 + 7) / 8 : 0, nb = diag ? 0 : (rb0 < p ? (p - rb0 + 7) / 8 : 0);
    double ca[8], cb[8], va[8], vb[8], rs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ca[i] = i < na ? c[ra0 + 8 * i] : 0.0;
        cb[i] = i < nb ? c[rb0 + 8 * i] : 0.0;
        va[i] = 0.0; vb[i] = 0.0; rs[i] = 0.0;
    }
    // wave w owns block row w; nq: the blocks of that row it computes (below p, and not above the diagonal)
    const bool active = 64 * si + 16 * w < p;
    int nq = (p - 64 * sj + 15) / 16;
    if (nq > 4) nq = 4;
    if (diag && nq > w + 1) nq = w + 1;
    if (!active) nq = 0;
    cs_d4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = cs_d4{0.0, 0.0, 0.0, 0.0};

    auto load = [&](long long it) {
        const long long d = it / ntile;
        const int t = (int)(it - d * ntile);
        const long long col = j0 + (long long)t * CS_TC + lc;
        const bool ok = col < j1;
        const size_t base = (size_t)d * (size_t)p * (size_t)J + (size_t)col;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            va[i] = (ok && i < na) ? (double)trace[base + (size_t)(ra0 + 8 * i) * (size_t)J] - ca[i] : 0.0;
            vb[i] = (ok && i < nb) ? (double)trace[base + (size_t)(rb0 + 8 * i) * (size_t)J] - cb[i] : 0.0;
        }
    };

    const double* Bt = diag ? As : Bs;
    if (total > 0) load(0);
    for (long long it = 0; it < total; ++it) {
        __syncthreads();                                   // the last tile's reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[(lr + 8 * i) * CS_RS + lc] = va[i];
            if (!diag) Bs[(lr + 8 * i) * CS_RS + lc] = vb[i];
            else rs[i] += va[i];
        }
        __syncthreads();
        if (it + 1 < total) load(it + 1);                  // in flight under the MFMAs below
        if (nq > 0) {
#pragma unroll
            for (int t = 0; t < CS_TC / 4; ++t) {
                const double av = As[(16 * w + r) * CS_RS + 4 * t + kq];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nq) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bt[(16 * q + r) * CS_RS + 4 * t + kq], acc[q], 0, 0, 0);
            }
        }
    }
    double* out = part + ((size_t)slab * pairs + pair) * 4096;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < nq) {
#pragma unroll
            for (int g = 0; g < 4; ++g) out[(size_t)(16 * w + kq + 4 * g) * 64 + 16 * q + r] = acc[q][g];
        }
    if (diag) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double v = rs[i];
#pragma unroll
            for (int o = CS_TC / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lc == 0 && i < na) part1[(size_t)slab * pp + ra0 + 8 * i] = v;
        }
    }
}

// tot [p][p] (lower triangle; zero above) then [p]: tot = (the slabs' sum) + tot, or the slabs' sum alone for a run's first
// launch.  A workgroup takes CS_RE entries; CS_RL lanes per entry take every CS_RL-th slab in order (one lane alone would
// walk up to a thousand slabs at a load latency each), then the lanes' partials are added in lane order.
__global__ __launch_bounds__(CS_THREADS)
void chain_pool_reduce_kernel(const double* __restrict__ part, const double* __restrict__ part1, int slabs, int pairs,
                              int p, int pp, int first, double* __restrict__ tot) {
    __shared__ double red[CS_RL][CS_RE];
    const int e = threadIdx.x % CS_RE, sl = threadIdx.x / CS_RE;
    const int idx = blockIdx.x * CS_RE + e;
    const int pp2 = p * p;
    const bool valid = idx < pp2 + p;
    bool upper = false;
    const double* src = part;
    size_t stride = 0;
    if (valid) {
        if (idx < pp2) {
            const int i = idx / p, j = idx - i * p;
            upper = j > i;
            const int si = i >> 6, sj = j >> 6;
            src = part + ((size_t)(si * (si + 1) / 2 + sj) * 64 + (i & 63)) * 64 + (j & 63);
            stride = (size_t)pairs * 4096;
        } else {
            src = part1 + (idx - pp2);
            stride = (size_t)pp;
        }
    }
    double s = 0.0;
    if (valid && !upper)
        for (int k = sl; k < slabs; k += CS_RL) s += src[(size_t)k * stride];
    red[sl][e] = s;
    __syncthreads();
    if (sl != 0 || !valid) return;
    if (upper) { if (first) tot[idx] = 0.0; return; }
    double t = 0.0;
    for (int l = 0; l < CS_RL; ++l) t += red[l][e];
    tot[idx] = first ? t : t + tot[idx];
}

// grid = (blocks, p).  hpart [p][blocks][3].  half (may be null): [2: m, s^2][2 halves][p][J]
__global__ __launch_bounds__(CS_THREADS)
void chain_half_reduce_kernel(const double* __restrict__ shift, const double* __restrict__ S, const double* __restrict__ c, int p,
                              long long J, long long n, int blocks, double* __restrict__ hpart, double* __restrict__ half) {
    __shared__ double red[3][CS_THREADS / 64];
    const int row = blockIdx.y, b = blockIdx.x;
    const double cr = c[row], dn = (double)n, dn1 = (double)(n - 1);
    const size_t pj = (size_t)p * (size_t)J;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int h = 0; h < 2; ++h)
        for (int u = 0; u < CS_CH / CS_THREADS; ++u) {
            const long long j = (long long)b * CS_CH + u * CS_THREADS + threadIdx.x;
            if (j < J) {
                const size_t idx = (size_t)row * (size_t)J + (size_t)j;
                const double s1 = S[(size_t)(2 * h) * pj + idx], s2 = S[(size_t)(2 * h + 1) * pj + idx];
                const double m = shift[idx] + s1 / dn;
                const double v = (s2 - s1 * s1 / dn) / dn1;
                const double dm = m - cr;
                a0 += dm; a1 = fma(dm, dm, a1); a2 += v;
                if (half) {
                    half[(size_t)h * pj + idx] = m;
                    half[(size_t)(2 + h) * pj + idx] = v;
                }
            }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_down(a0, o, 64); a1 += __shfl_down(a1, o, 64); a2 += __shfl_down(a2, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[0][w] = a0; red[1][w] = a1; red[2][w] = a2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int i = 0; i < CS_THREADS / 64; ++i) s += red[threadIdx.x][i];
        hpart[((size_t)row * blocks + b) * 3 + threadIdx.x] = s;
    }
}

__global__ void chain_half_final_kernel(const double* __restrict__ hpart, int p, int blocks, double* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * p) return;
    const int row = idx / 3, k = idx - 3 * row;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += hpart[((size_t)row * blocks + b) * 3 + k];
    out[idx] = s;
}

// ---------------------------------------------------------------------------
static int cs_pp(const Engine& e) { return (e.p + 63) / 64 * 64; }
static int cs_pairs(const Engine& e) { const int t = cs_pp(e) / 64; return t * (t + 1) / 2; }
// The slab plan, from the engine's shape alone (tests/chain_summary_cases.py restates it): as many slabs as bring the launch
// to CS_WGS workgroups, of no more than CS_SLAB chains and no fewer than one tile, whole tiles each.
static int cs_slab_cols(const Engine& e) {
    const long long lo = (e.J + CS_SLAB - 1) / CS_SLAB, hi = (e.J + CS_TC - 1) / CS_TC;
    long long want = (CS_WGS + cs_pairs(e) - 1) / cs_pairs(e);
    want = want < lo ? lo : (want > hi ? hi : want);
    const long long cols = (e.J + want - 1) / want;
    return (int)((cols + CS_TC - 1) / CS_TC * CS_TC);
}
static int cs_slabs(const Engine& e) { const int w = cs_slab_cols(e); return (int)((e.J + w - 1) / w); }
static int cs_blocks(const Engine& e) { return (int)((e.J + CS_CH - 1) / CS_CH); }
static int cs_slices(const Engine& e) { const long long s = (e.J + 1023) / 1024; return (int)(s < 1 ? 1 : (s > CS_SLICES ? CS_SLICES : s)); }

// the stage's buffers, sized by the engine's shape alone: allocated by the first begin, kept by drop()
int chainsum_begin(Engine& e, long long n_draws) {
    ChainSumState& cs = e.cs;
    const size_t pj = (size_t)e.p * (size_t)e.J, p = (size_t)e.p;
    cs.drop();
    cs.slabs = cs_slabs(e);
    TRY_BUF(cs.shift.ensure(pj * 8, false));
    TRY_BUF(cs.S.ensure(4 * pj * 8, false));
    TRY_BUF(cs.c.ensure(p * 8, false));
    TRY_BUF(cs.cpart.ensure(p * CS_SLICES * 8, false));
    TRY_BUF(cs.tot.ensure((p * p + p) * 8, false));
    TRY_BUF(cs.part.ensure(((size_t)cs.slabs * cs_pairs(e) * 4096 + (size_t)cs.slabs * cs_pp(e)) * 8, false));
    TRY_BUF(cs.hpart.ensure(((size_t)cs_blocks(e) * 3 * p + 3 * p) * 8, false));
    cs.N = n_draws;
    return CESX_OK;
}

template <typename T>
static int chainsum_add_t(Engine& e, const void* trace, int kept, hipStream_t s) {
    ChainSumState& cs = e.cs;
    const int p = e.p, pp = cs_pp(e), pairs = cs_pairs(e), slabs = cs.slabs;
    const long long J = e.J, n = cs.N / 2;
    const int first = cs.added == 0;
    if (first) {                                          // c: the row means of the run's first draw
        const int nsl = cs_slices(e);
        if (const int rc = launch_rowsum(e, trace, p, nsl, cs.cpart, s)) return rc;
        hipLaunchKernelGGL(chain_c_final_kernel, dim3((p + 255) / 256), dim3(256), 0, s, (const double*)cs.cpart, p, nsl, J, cs.c.get());
        CESX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(chain_half_kernel<T>, dim3((unsigned)((J + CS_THREADS - 1) / CS_THREADS), (p + CS_RB - 1) / CS_RB), dim3(CS_THREADS), 0, s,
                       (const T*)trace, kept, p, J, cs.added, cs.N, n, cs.shift.get(), cs.S.get());
    CESX_HIP(hipGetLastError());
    double* part1 = cs.part.get() + (size_t)slabs * pairs * 4096;
    hipLaunchKernelGGL(chain_pool_kernel<T>, dim3(slabs, pairs), dim3(CS_THREADS), 0, s, (const T*)trace, kept, p, J, cs_slab_cols(e),
                       (const double*)cs.c, pairs, pp, cs.part.get(), part1);
    CESX_HIP(hipGetLastError());
    hipLaunchKernelGGL(chain_pool_reduce_kernel, dim3((p * p + p + CS_RE - 1) / CS_RE), dim3(CS_THREADS), 0, s, (const double*)cs.part, (const double*)part1,
                       slabs, pairs, p, pp, first, cs.tot.get());
    CESX_HIP(hipGetLastError());
    cs.added += kept;
    return CESX_OK;
}

int chainsum_add(Engine& e, const void* trace, int kept, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? chainsum_add_t<float>(e, trace, kept, s) : chainsum_add_t<double>(e, trace, kept, s);
}

int chainsum_read(Engine& e, double* c, double* s1, double* cc, double* within, double* between, double* half_mean,
                  double* half_var, hipStream_t s) {
    ChainSumState& cs = e.cs;
    const int p = e.p, blocks = cs_blocks(e);
    const size_t pj = (size_t)p * (size_t)e.J;
    const bool want_half = half_mean || half_var;
    if (want_half) TRY_BUF(cs.half.ensure(4 * pj * 8, false));
    double* out3 = cs.hpart.get() + (size_t)blocks * 3 * p;
    hipLaunchKernelGGL(chain_half_reduce_kernel, dim3(blocks, p), dim3(CS_THREADS), 0, s, (const double*)cs.shift, (const double*)cs.S,
                       (const double*)cs.c, p, (long long)e.J, cs.N / 2, blocks, cs.hpart.get(), want_half ? cs.half.get() : (double*)nullptr);
    CESX_HIP(hipGetLastError());
    hipLaunchKernelGGL(chain_half_final_kernel, dim3((3 * p + 255) / 256), dim3(256), 0, s, (const double*)cs.hpart, p, blocks, out3);
    CESX_HIP(hipGetLastError());
    CESX_HIP(hipStreamSynchronize(s));
    std::vector<double> o3((size_t)3 * p);
    CESX_HIP(hipMemcpy(o3.data(), out3, o3.size() * 8, hipMemcpyDeviceToHost));
    CESX_HIP(hipMemcpy(c, cs.c, (size_t)p * 8, hipMemcpyDeviceToHost));
    CESX_HIP(hipMemcpy(cc, cs.tot, (size_t)p * p * 8, hipMemcpyDeviceToHost));
    CESX_HIP(hipMemcpy(s1, cs.tot.get() + (size_t)p * p, (size_t)p * 8, hipMemcpyDeviceToHost));
    if (half_mean) CESX_HIP(hipMemcpy(half_mean, cs.half, 2 * pj * 8, hipMemcpyDeviceToHost));
    if (half_var) CESX_HIP(hipMemcpy(half_var, cs.half.get() + 2 * pj, 2 * pj * 8, hipMemcpyDeviceToHost));
    cs.half.reset();
    const double h = 2.0 * (double)e.J;                  // half-chains
    for (int r = 0; r < p; ++r) {
        const double a0 = o3[(size_t)3 * r], a1 = o3[(size_t)3 * r + 1], a2 = o3[(size_t)3 * r + 2];
        within[r] = a2 / h;
        between[r] = (a1 - a0 * a0 / h) / (h - 1.0);
    }
    return CESX_OK;
}

}  // namespace cesx
