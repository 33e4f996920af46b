// Streaming lagged sums of the chains' draws (cesx_chain_acf_*, include/cesx.h): what the autocorrelation ESS of
// MCMC(..., chains=M, summary=True, autocorr=...) is made of, taken from the draws cesx_chain_summary_add reads while they are
// in device memory.  All state is fp64 (an fp32 draw converts exactly), every sum runs in a fixed order and nothing is added
// atomically.  For row r, chain j < C and draws x_0 .. x_{N-1}, with the shift c = x_0 and a_t = x_t - c:
//   S1 = sum a_t,   P_k = sum_{t >= k} a_{t-k} a_t  (k = 0 .. L),   the first L and the last L of the a_t.
//
//   chain_acf_pack_kernel   the step path adds one draw at a time: up to ACF_BLOCK draws of the C chains wait in the stage's
//                           own memory ([draw][p][C], engine dtype), so that the sums below move once per block.
//   chain_acf_kernel        one lane per chain, one row per workgroup: c, S1, P_0 .. P_LT and a ring of the last LT values of
//                           a (slot t mod LT) are loaded, carried through the block's draws in order -- per draw one
//                           P_k = fma(a_{t-k}, a_t, P_k) for every k, the ring being zero before the first draw -- and
//                           stored once.  Each P_k is one running sum in increasing t whatever the cut into launches: the
//                           same bits.  LT = 8 and 32: the ring in registers, the draws unrolled by LT so that every slot
//                           is a register known at compile time; LT = 64: the ring in LDS ([slot][lane]: conflict-free
//                           ds_read_b64, each lane its own column, no barrier).  Lags past L up to LT are summed and never read.
//   chain_acf_final_kernel  per (row, chain): d = S1 / N, Hd_k = S1 - (the last k of a), Tl_k = S1 - (the first k of a),
//                           G_k = P_k - d (Hd_k + Tl_k) + (N - k) d^2 = sum (x_t - m)(x_{t+k} - m), m = c + d.
//   chain_acf_reduce_kernel one workgroup per output over the C chains: every ACF_RT-th chain in order per thread, then
//                           a tree over the threads; cbar = mean c, then sum G_k, sum (m - cbar), sum (m - cbar)^2.
#include "cesx_internal.h"

namespace cesx {

constexpr int ACF_THREADS = 64;    // chain_acf_kernel: one wave per workgroup (the LDS ring is 32 KiB per wave)
constexpr int ACF_BLOCK = 64;      // draws the stage holds back before the lag kernel runs on them
constexpr int ACF_PF = 8;          // draws loaded ahead of their sums
constexpr int ACF_RT = 256;        // threads of chain_acf_reduce_kernel

static int acf_lt(int L) { return L <= 8 ? 8 : (L <= 32 ? 32 : 64); }

// dst [take][p][C] <- the first C chains of src [take][p][J]
template <typename T>
__global__ __launch_bounds__(256)
void chain_acf_pack_kernel(const T* __restrict__ src, int p, long long J, int C, T* __restrict__ dst) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    const size_t row = (size_t)blockIdx.z * p + blockIdx.y;
    dst[row * (size_t)C + j] = src[row * (size_t)J + j];
}

// grid = (ceil(C / ACF_THREADS), p).  src: draw t0 + i of row r and chain j at src[i * ld_draw + r * ldj + j], i < nd.
// State, all [..][p][C]: c, S1, P [LT + 1], ring [LT] (slot t mod LT), head [L] (a_0 .. a_{L-1}).
template <typename T, int LT, bool LDS>
__global__ __launch_bounds__(ACF_THREADS)
void chain_acf_kernel(const T* __restrict__ src, size_t ld_draw, size_t ldj, int p, int C, long long t0, int nd, int L,
                      double* __restrict__ c, double* __restrict__ S1, double* __restrict__ P, double* __restrict__ ring,
                      double* __restrict__ head) {
    __shared__ double lring[LDS ? LT * ACF_THREADS : 1];
    const int lane = threadIdx.x;
    const int j = blockIdx.x * ACF_THREADS + lane;
    if (j >= C) return;
    const int r = blockIdx.y;
    const size_t pc = (size_t)p * (size_t)C, idx = (size_t)r * (size_t)C + (size_t)j;
    const T* x = src + (size_t)r * ldj + (size_t)j;
    const long long t1 = t0 + nd;
    const bool first = t0 == 0;
    double cc, s1, Pk[LT + 1], h[LDS ? 1 : LT];
    cc = first ? (double)x[0] : c[idx];
    s1 = first ? 0.0 : S1[idx];
#pragma unroll
    for (int k = 0; k <= LT; ++k) Pk[k] = first ? 0.0 : P[(size_t)k * pc + idx];
#pragma unroll
    for (int k = 0; k < LT; ++k) {
        const double v = first ? 0.0 : ring[(size_t)k * pc + idx];
        if constexpr (LDS) lring[k * ACF_THREADS + lane] = v; else h[k] = v;
    }

    if constexpr (LDS) {
        for (long long tb = t0; tb < t1; tb += ACF_PF) {
            double xv[ACF_PF];
#pragma unroll
            for (int u = 0; u < ACF_PF; ++u) {           // past the block: the block's last draw again, not used
                const long long t = tb + u < t1 ? tb + u : t1 - 1;
                xv[u] = (double)x[(size_t)(t - t0) * ld_draw];
            }
#pragma unroll
            for (int u = 0; u < ACF_PF; ++u) {
                const long long t = tb + u;
                if (t < t1) {
                    const double a = xv[u] - cc;
                    const int s = (int)(t & (LT - 1));
                    s1 += a;
                    if (t < L) head[(size_t)t * pc + idx] = a;
                    Pk[0] = fma(a, a, Pk[0]);
#pragma unroll
                    for (int k = 1; k <= LT; ++k) Pk[k] = fma(lring[((s - k) & (LT - 1)) * ACF_THREADS + lane], a, Pk[k]);
                    lring[s * ACF_THREADS + lane] = a;
                }
            }
        }
    } else {
        static_assert(LT % ACF_PF == 0, "a group is whole prefetch blocks");
        // i = t - t0; the next load and the next head store go through pointers that move one draw at a time (the
        // 2 LT products s * ld_draw and s * pc as loop constants would not fit the scalar registers)
        const T* xq = x;
        double* hq = head + (size_t)t0 * pc + idx;
        const int hl = t0 < L ? (int)(L - t0) : 0;       // draws of this block that belong to the head
        for (int ib = -(int)(t0 % LT); ib < nd; ib += LT) {
#pragma unroll
            for (int s8 = 0; s8 < LT; s8 += ACF_PF) {
                if (ib + s8 + ACF_PF <= 0 || ib + s8 >= nd) continue;
                double xv[ACF_PF];
#pragma unroll
                for (int u = 0; u < ACF_PF; ++u) {       // outside the block: its nearest draw, not used
                    const int i = ib + s8 + u;
                    xv[u] = (double)*xq;
                    if (i >= 0 && i + 1 < nd) xq += ld_draw;
                }
#pragma unroll
                for (int u = 0; u < ACF_PF; ++u) {
                    const int s = s8 + u;                // the slot of a_t: known at compile time
                    const int i = ib + s;
                    if (i >= 0 && i < nd) {
                        const double a = xv[u] - cc;
                        s1 += a;
                        if (i < hl) { *hq = a; hq += pc; }
                        Pk[0] = fma(a, a, Pk[0]);
#pragma unroll
                        for (int k = 1; k <= LT; ++k) Pk[k] = fma(h[(s - k + LT) % LT], a, Pk[k]);
                        h[s] = a;
                    }
                }
            }
        }
    }

    if (first) c[idx] = cc;
    S1[idx] = s1;
#pragma unroll
    for (int k = 0; k <= LT; ++k) P[(size_t)k * pc + idx] = Pk[k];
#pragma unroll
    for (int k = 0; k < LT; ++k) {
        double v;
        if constexpr (LDS) v = lring[k * ACF_THREADS + lane]; else v = h[k];
        ring[(size_t)k * pc + idx] = v;
    }
}

// one thread per (row, chain): gamma [L + 1][p][C], mean [p][C]
__global__ __launch_bounds__(256)
void chain_acf_final_kernel(const double* __restrict__ c, const double* __restrict__ S1, const double* __restrict__ P,
                            const double* __restrict__ ring, const double* __restrict__ head, size_t pc, long long N, int L, int LT,
                            double* __restrict__ gamma, double* __restrict__ mean) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pc) return;
    const double s1 = S1[idx], d = s1 / (double)N;
    double hs = 0.0, ts = 0.0;                             // the last k and the first k of a
    for (int k = 0; k <= L; ++k) {
        if (k > 0) {
            hs += ring[(size_t)((N - k) % LT) * pc + idx];
            ts += head[(size_t)(k - 1) * pc + idx];
        }
        const double hd = s1 - hs, tl = s1 - ts;
        gamma[(size_t)k * pc + idx] = P[(size_t)k * pc + idx] - d * (hd + tl) + (double)(N - k) * (d * d);
    }
    mean[idx] = c[idx] + d;
}

// out[e] = (sum over j < C of f(src[e * C + j])) / div; mode 0: f(v) = v, 1: v - cbar[e % p], 2: (v - cbar[e % p])^2
__global__ __launch_bounds__(ACF_RT)
void chain_acf_reduce_kernel(const double* __restrict__ src, int C, int p, int mode, const double* __restrict__ cbar, double div,
                             double* __restrict__ out) {
    __shared__ double red[ACF_RT];
    const int e = blockIdx.x, tid = threadIdx.x;
    const double cb = mode ? cbar[e % p] : 0.0;
    double s = 0.0;
    for (int j = tid; j < C; j += ACF_RT) {
        double v = src[(size_t)e * (size_t)C + j] - cb;
        if (mode == 2) v = v * v;
        s += v;
    }
    red[tid] = s;
    __syncthreads();
    for (int o = ACF_RT / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[e] = red[0] / div;
}

// ---------------------------------------------------------------------------
int chainacf_begin(Engine& e, long long n_draws, int lags, int n_chains) {
    ChainAcfState& ca = e.ca;
    const int LT = acf_lt(lags);
    const size_t pc = (size_t)e.p * (size_t)n_chains, esz = e.cfg.dtype == CESX_F32 ? 4 : 8;
    ca.drop();
    TRY_BUF(ca.c.ensure(pc * 8, false));
    TRY_BUF(ca.S1.ensure(pc * 8, false));
    TRY_BUF(ca.P.ensure((size_t)(LT + 1) * pc * 8, false));
    TRY_BUF(ca.ring.ensure((size_t)LT * pc * 8, false));
    TRY_BUF(ca.head.ensure((size_t)lags * pc * 8, false));
    TRY_BUF(ca.pending.ensure((size_t)ACF_BLOCK * pc * esz, false));
    TRY_BUF(ca.out.ensure(((size_t)(lags + 1) * e.p + 3 * (size_t)e.p) * 8, false));
    ca.N = n_draws; ca.L = lags; ca.LT = LT; ca.C = n_chains;
    return CESX_OK;
}

// the lag kernel over nd draws at src (chains ldj apart in a row): draws ca.done .. ca.done + nd - 1
template <typename T>
static int acf_run(Engine& e, const T* src, size_t ldj, int nd, hipStream_t s) {
    ChainAcfState& ca = e.ca;
    const dim3 grid((ca.C + ACF_THREADS - 1) / ACF_THREADS, e.p), block(ACF_THREADS);
    const size_t ld_draw = (size_t)e.p * ldj;
#define ACF_LAUNCH(LT, LDS)                                                                                                   \
    hipLaunchKernelGGL((chain_acf_kernel<T, LT, LDS>), grid, block, 0, s, src, ld_draw, ldj, e.p, ca.C, ca.done, nd, ca.L,    \
                       ca.c.get(), ca.S1.get(), ca.P.get(), ca.ring.get(), ca.head.get())
    if (ca.LT == 8) ACF_LAUNCH(8, false);
    else if (ca.LT == 32) ACF_LAUNCH(32, false);
    else ACF_LAUNCH(64, true);
#undef ACF_LAUNCH
    CESX_HIP(hipGetLastError());
    ca.done += nd;
    return CESX_OK;
}

template <typename T>
static int acf_flush(Engine& e, hipStream_t s) {
    ChainAcfState& ca = e.ca;
    if (ca.pend == 0) return CESX_OK;
    const int nd = ca.pend;
    ca.pend = 0;
    return acf_run<T>(e, (const T*)ca.pending.get(), (size_t)ca.C, nd, s);
}

template <typename T>
static int chainacf_add_t(Engine& e, const void* trace, int kept, hipStream_t s) {
    ChainAcfState& ca = e.ca;
    const T* src = (const T*)trace;
    const size_t pj = (size_t)e.p * (size_t)e.J, pc = (size_t)e.p * (size_t)ca.C;
    ca.added += kept;
    while (kept > 0) {
        if (ca.pend == 0 && kept >= ACF_BLOCK) return acf_run<T>(e, src, (size_t)e.J, kept, s);
        const int take = kept < ACF_BLOCK - ca.pend ? kept : ACF_BLOCK - ca.pend;
        hipLaunchKernelGGL(chain_acf_pack_kernel<T>, dim3((ca.C + 255) / 256, e.p, take), dim3(256), 0, s, src, e.p, (long long)e.J, ca.C,
                           (T*)ca.pending.get() + (size_t)ca.pend * pc);
        CESX_HIP(hipGetLastError());
        ca.pend += take; kept -= take; src += (size_t)take * pj;
        if (ca.pend == ACF_BLOCK) if (const int rc = acf_flush<T>(e, s)) return rc;
    }
    return CESX_OK;
}

int chainacf_add(Engine& e, const void* trace, int kept, hipStream_t s) {
    return e.cfg.dtype == CESX_F32 ? chainacf_add_t<float>(e, trace, kept, s) : chainacf_add_t<double>(e, trace, kept, s);
}

int chainacf_read(Engine& e, double* gsum, double* msum, double* m2sum, double* chain_gamma, double* chain_mean, hipStream_t s) {
    ChainAcfState& ca = e.ca;
    const int p = e.p, L = ca.L, C = ca.C;
    const size_t pc = (size_t)p * (size_t)C, ng = (size_t)(L + 1) * p;
    if (const int rc = e.cfg.dtype == CESX_F32 ? acf_flush<float>(e, s) : acf_flush<double>(e, s)) return rc;
    TRY_BUF(ca.gamma.ensure((size_t)(L + 1) * pc * 8, false));
    TRY_BUF(ca.mean.ensure(pc * 8, false));
    hipLaunchKernelGGL(chain_acf_final_kernel, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, s, (const double*)ca.c, (const double*)ca.S1,
                       (const double*)ca.P, (const double*)ca.ring, (const double*)ca.head, pc, ca.N, L, ca.LT, ca.gamma.get(), ca.mean.get());
    CESX_HIP(hipGetLastError());
    double* out = ca.out.get();                            // [L + 1][p] sum G, then [p] cbar, [p] sum (m - cbar), [p] sum (m - cbar)^2
    double* cbar = out + ng;
    hipLaunchKernelGGL(chain_acf_reduce_kernel, dim3(p), dim3(ACF_RT), 0, s, (const double*)ca.c, C, p, 0, (const double*)nullptr, (double)C, cbar);
    CESX_HIP(hipGetLastError());
    hipLaunchKernelGGL(chain_acf_reduce_kernel, dim3((unsigned)ng), dim3(ACF_RT), 0, s, (const double*)ca.gamma, C, p, 0, (const double*)nullptr, 1.0, out);
    CESX_HIP(hipGetLastError());
    hipLaunchKernelGGL(chain_acf_reduce_kernel, dim3(p), dim3(ACF_RT), 0, s, (const double*)ca.mean, C, p, 1, (const double*)cbar, 1.0, cbar + p);
    CESX_HIP(hipGetLastError());
    hipLaunchKernelGGL(chain_acf_reduce_kernel, dim3(p), dim3(ACF_RT), 0, s, (const double*)ca.mean, C, p, 2, (const double*)cbar, 1.0, cbar + 2 * p);
    CESX_HIP(hipGetLastError());
    CESX_HIP(hipStreamSynchronize(s));
    std::vector<double> o(ng + 3 * (size_t)p);
    CESX_HIP(hipMemcpy(o.data(), out, o.size() * 8, hipMemcpyDeviceToHost));
    for (int r = 0; r < p; ++r) {
        for (int k = 0; k <= L; ++k) gsum[(size_t)r * (L + 1) + k] = o[(size_t)k * p + r];
        msum[r] = o[ng + p + r];
        m2sum[r] = o[ng + 2 * (size_t)p + r];
    }
    if (chain_gamma) CESX_HIP(hipMemcpy(chain_gamma, ca.gamma, (size_t)(L + 1) * pc * 8, hipMemcpyDeviceToHost));
    if (chain_mean) CESX_HIP(hipMemcpy(chain_mean, ca.mean, pc * 8, hipMemcpyDeviceToHost));
    ca.gamma.reset(); ca.mean.reset();
    return CESX_OK;
}

}  // namespace cesx
