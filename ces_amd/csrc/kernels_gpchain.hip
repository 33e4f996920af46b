// The fused chain kernel of MCMC.gp_mh(chains=M): n_steps Metropolis steps of every chain on the GP emulator in ONE launch
// (cesx_gp_run, include/cesx.h).  Per step what cesx_mh_propose / cesx_gp_predict / cesx_gp_accept do in three launches (four
// with the device noise of an fp64 engine):
//     P    = a U + (b S) xi                                                       (engine.hip, cesx_mh_propose)
//     mean, var of every GP at P                                                   (kernels_gp.hip, gp_predict_kernel)
//     phi  = the likelihood mode's term + 1/2 |L_Sigma^{-1} (P - mu)|^2            (kernels_gp.hip, gp_score_kernel)
//     log u < phi(U) - phi(P)  ->  U := P, phi := phi(P), counter + 1              (mh_test)
//
// gp_chain_kernel: one workgroup per tile of GPC_T = 32 chains, 8 waves, as gp_predict_kernel; chains are independent, so
// nothing crosses workgroups.  The tile's state -- U as fp64 [p][32] in LDS, phi and the accept counter in the registers of
// thread cc < 32 for chain cc -- is loaded once, lives on chip for the whole launch and is stored once.  The GPs run in turn
// through ONE K* panel; their means and variances stay in LDS ([n_gp][32] each) and never reach HBM.  All arithmetic is fp64
// for either engine dtype; an fp32 engine rounds where it stores (the trace, U at the end).
//
// The prediction restates the tile body of gp_predict_kernel and MUST stay in step with kernels_gp.hip:64-136 (the mapped
// queries, the K* panel and the 16 group partials of the mean, the zig-zag block rows of W = L^{-1} K* on
// v_mfma_f64_16x16x4_f64, the 32 partials of the variance) and with gp_kern (kernels_gp.hip:40-46): the same products in
// the same order, so that mean and var of an fp64 query column are bit-identical to cesx_gp_predict's.  The score restates
// gp_score_kernel (kernels_gp.hip:194-222) term by term.  The proposal's rows are summed in column order as
// mh_run_map_kernel does (kernels_maps.hip:175-181); the noise is the step path's: xi row r of global chain gj at MH step s
// from philox(gj, r / 4, s | 2^31) through the fp64 normal4 for either engine dtype, the uniform from mh_log_uniform.
// No atomics: every sum has a fixed order and runs are bit-identical.
#include "cesx_internal.h"

namespace cesx {

constexpr int GPC_T = 32;                    // chains per tile (two 16-column MFMA groups)
constexpr int GPC_NW = 8;                    // waves per workgroup
constexpr int GPC_THREADS = GPC_NW * 64;
constexpr int GPC_RED = GPC_NW * 4 * GPC_T;  // doubles of the partial-sum buffer (static LDS)
constexpr size_t GPC_LDS_BUDGET = 160 * 1024;
using gpc_d4 = double __attribute__((ext_vector_type(4)));

template <typename T>
struct GpChainArgs {
    T* U; T* trace; const T* xi; const double* logu;
    double* phi; unsigned long long* cnt;
    long long M, j_offset;
    unsigned seed_lo, seed_hi, step0;      // step0: the Philox step word of the first step (index | 2^31)
    int n_steps, stride;
    int p, n, Jt, Jp; size_t li_len;       // the emulator (GpState)
    const double *A, *c, *Z, *par, *mw, *alpha, *Li;
    int mode, nugget;
    const double *y, *gw, *gam, *Lg;       // data, as GpScoreArgs
    const double *mu, *sw, *LSi;           // prior: diagonal (sw) or dense (LSi = L_Sigma^{-1})
    double a; const double* bS;            // P = a U + (b S) xi, b S [p][p] row-major
};

// sigma^2 f(r): gp_kern of kernels_gp.hip, restated (a __device__ function is private to its translation unit)
__device__ __noinline__ static double gpc_kern(int fam, double s2, double d2) {
    const double r = sqrt(d2);
    const double s = fam == 1 ? r : (fam == 2 ? 1.7320508075688772 : 2.23606797749979) * r;
    const double e = exp(fam == 0 ? -0.5 * d2 : -s);
    const double poly = fam <= 1 ? 1.0 : (fam == 2 ? 1.0 + s : 1.0 + s + s * s / 3.0);
    return s2 * (poly * e);
}

// The step's draws as calls: the constants of the fp64 log, sincos and of Philox stay inside the callee instead of being
// hoisted out of the step loop into scalar registers the loop has no room for (as gp_kern's exp constants do).
// xi rows 4 q .. 4 q + 3 of global chain gj at step word `step`: the words and the normals of mh_run_map_kernel
__device__ __noinline__ static gpc_d4 gpc_normal4(unsigned long long gj, unsigned q, unsigned step, unsigned seed_lo, unsigned seed_hi) {
    double z[4];
    normal4(philox4x32_10((uint32_t)gj, (uint32_t)(gj >> 32), q, step, seed_lo, seed_hi), z);
    return gpc_d4{z[0], z[1], z[2], z[3]};
}
__device__ __noinline__ static double gpc_log(double v) { return log(v); }
__device__ __noinline__ static double gpc_log_uniform(unsigned long long gj, unsigned step, unsigned seed_lo, unsigned seed_hi) {
    return mh_log_uniform(gj, step, seed_lo, seed_hi);
}

// A uniform value as a per-lane one in vector registers.  The scalar registers hold the loop state and what the matrix pipe's
// loop addresses; everything a thread reads through an address of its own anyway (the problem's vectors, which only the one
// thread per chain reads; the proposal's and the input maps' entries; the training points of the thread's group) goes through
// per-lane values, or the kernel's scalars would not fit and spill inside the step loop (profiles/gp_chain_isa_audit.txt).
template <typename V>
__device__ __forceinline__ V gpc_v(V x) { asm volatile("" : "+v"(x)); return x; }

// dynamic LDS of one tile in doubles: zq [p][32], K* [Jp][32], mean and var [n_gp][32] each, U and P [p][32] each
static size_t gpc_lds_doubles(int p, int Jp, int n_gp) { return (size_t)GPC_T * ((size_t)3 * p + Jp + (size_t)2 * n_gp); }

// (4 waves per SIMD = at most 128 VGPRs: two workgroups per CU where LDS allows, so that one tile's waits on L2 are
// covered by another's arithmetic)
template <typename T>
__global__ __launch_bounds__(GPC_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void gp_chain_kernel(const GpChainArgs<T> a) {
    extern __shared__ double gpc_smem[];
    __shared__ double red[GPC_RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int p = a.p, n = a.n;
    double* zq = gpc_smem;                                   // [p][32] the step's xi, then each GP's mapped queries
    double* Kp = zq + (size_t)p * GPC_T;                     // [Jp][32]
    double* gm = Kp + (size_t)a.Jp * GPC_T;                  // [n][32] the GP means at P
    double* gv = gm + (size_t)n * GPC_T;                     // [n][32] the GP variances at P
    double* Uc = gv + (size_t)n * GPC_T;                     // [p][32] the chains' states
    double* Pp = Uc + (size_t)p * GPC_T;                     // [p][32] the proposals
    const int NB = a.Jp >> 4;
    const int NQ = (p + 3) >> 2;
    const bool want_var = a.mode != CESX_GP_GAMMA;
    const int cc = tid & (GPC_T - 1), grp = tid / GPC_T;     // 16 groups of 32 threads (512 % 32 == 0: a thread keeps its column cc)
    const int col = lane & 15, kq = lane >> 4;

    // ---- per-lane values (gpc_v) ----
    const long long Mv = gpc_v(a.M);
    const long long jc = gpc_v((long long)blockIdx.x * GPC_T) + cc;      // the thread's column: chain jc of this engine
    const unsigned long long gjc = (unsigned long long)(gpc_v(a.j_offset) + jc);
    // flags: 1 the thread is the one of chain jc (tid < 32, jc < M), 2 jc < M, 4 dense Gamma, 8 dense prior, 16 the nugget
    const int fl = gpc_v((tid < GPC_T && jc < Mv ? 1 : 0) | (jc < Mv ? 2 : 0) | (a.Lg ? 4 : 0) | (a.LSi ? 8 : 0) | (a.nugget ? 16 : 0));
    // (a test of fl or mode_v inside the step loop goes through gpc_v again: the compiler then leaves it where it is
    // instead of keeping one mask pair per test in scalar registers for the whole launch)
    const int mode_v = gpc_v(a.mode), stride_v = gpc_v(a.stride);
    const unsigned seed_lo = gpc_v(a.seed_lo), seed_hi = gpc_v(a.seed_hi);
    const double a_v = gpc_v(a.a);
    const double* const bS_v = gpc_v(a.bS);
    const double* const A_v = gpc_v(a.A);
    const double* const c_v = gpc_v(a.c);
    const double* const Z_v = gpc_v(a.Z);
    const double* const par_v = gpc_v(a.par);
    const double* const mw_v = gpc_v(a.mw);
    const double* const al_v = gpc_v(a.alpha);
    const double* const y_v = gpc_v(a.y);
    // (one address per role: the likelihood reads L_Gamma^{-1}, diag(Gamma^{-1}) or Gamma, the prior L_Sigma^{-1} or diag(Sigma^{-1}))
    const double* const gx_v = gpc_v(a.Lg ? a.Lg : a.mode == CESX_GP_GAMMA ? a.gw : a.gam);
    const double* const mu_v = gpc_v(a.mu);
    const double* const pr_v = gpc_v(a.LSi ? a.LSi : a.sw);
    double* const phi_j = gpc_v(a.phi) + jc;
    unsigned long long* const cnt_j = gpc_v(a.cnt) + jc;
    T* const U_j = gpc_v(a.U) + jc;
    T* tp = a.trace ? gpc_v(a.trace) + jc : nullptr;
    const double* lp = a.logu ? gpc_v(a.logu) + jc : nullptr;
    const T* xp = a.xi ? gpc_v(a.xi) + jc : nullptr;

#pragma unroll 1
    for (int idx = tid; idx < p * GPC_T; idx += GPC_THREADS)
        Uc[idx] = (fl & 2) ? (double)U_j[(size_t)(idx / GPC_T) * Mv] : 0.0;
    // the thread of chain jc keeps its phi and its counter
    double ph = 0.0;
    unsigned long long cnt = 0ull;
    if (fl & 1) { ph = *phi_j; cnt = *cnt_j; }
    int since = 0;
    __syncthreads();

    for (int k = 0; k < a.n_steps; ++k) {
        const unsigned step = a.step0 + (unsigned)k;         // (step0 carries the MH domain bit)
        // ---- propose: xi into zq, then P = a U + (b S) xi ----
        if (xp) {
#pragma unroll 1
            for (int idx = gpc_v(tid); idx < p * GPC_T; idx += GPC_THREADS)
                zq[idx] = (gpc_v(fl) & 2) ? (double)xp[(size_t)(idx / GPC_T) * Mv] : 0.0;
            xp += (size_t)p * Mv;
        } else {
#pragma unroll 1
            for (int idx = gpc_v(tid); idx < NQ * GPC_T; idx += GPC_THREADS) {
                const int q = idx / GPC_T;
                const gpc_d4 z = gpc_normal4(gjc, (unsigned)q, step, seed_lo, seed_hi);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < p) zq[(4 * q + e) * GPC_T + cc] = z[e];
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int idx = gpc_v(tid); idx < p * GPC_T; idx += GPC_THREADS) {
            const int r = idx / GPC_T;
            double acc = 0.0;
#pragma unroll 1
            for (int c = 0; c <= r; ++c) acc += bS_v[(size_t)r * p + c] * zq[c * GPC_T + cc];
            Pp[idx] = a_v * Uc[idx] + acc;
        }
        __syncthreads();

        // ---- predict: the GPs in turn (kernels_gp.hip:64-136) ----
        int g = 0;
        do {                                                 // (n >= 1: cesx_gp_set)
            const double* A = A_v + (size_t)g * p * p;
            // 1. the mapped queries
#pragma unroll 1
            for (int idx = gpc_v(tid); idx < p * GPC_T; idx += GPC_THREADS) {
                const int r = idx / GPC_T;
                double z = 0.0;
                if (gpc_v(fl) & 2) {
#pragma unroll 1
                    for (int s = 0; s <= r; ++s) z = fma(A[(size_t)r * p + s], Pp[s * GPC_T + cc] - c_v[s], z);
                }
                zq[idx] = z;
            }
            __syncthreads();
            // 2. the K* panel (zero rows past Jt) and the mean's partial sums
            const double s2 = par_v[4 * g];
            const int fam = (int)par_v[4 * g + 3];
            const double* Zg = Z_v + (size_t)g * a.Jt * p;
            const double* al = al_v + (size_t)g * a.Jp;
            double macc = 0.0;
#pragma unroll 1
            for (int t = grp; t < a.Jp; t += GPC_THREADS / GPC_T) {
                double kv = 0.0;
                if (t < a.Jt) {
                    double d2 = 0.0;
                    const int pl = gpc_v(p);                  // (a per-lane bound: the unrolled loop's control stays out of the scalars)
#pragma unroll 4
                    for (int r = 0; r < pl; ++r) { const double d = zq[r * GPC_T + cc] - Zg[(size_t)t * pl + r]; d2 = fma(d, d, d2); }
                    kv = gpc_kern(fam, s2, d2);
                    macc = fma(al[t], kv, macc);
                }
                Kp[(size_t)t * GPC_T + cc] = kv;
            }
            red[grp * GPC_T + cc] = macc;
            __syncthreads();
            if (gpc_v(tid) < GPC_T) {
                double m = 0.0;
#pragma unroll 1
                for (int q = 0; q < GPC_THREADS / GPC_T; ++q) m += red[q * GPC_T + tid];
                double lin = par_v[4 * g + 2];
                const double* mw = mw_v + (size_t)g * p;
#pragma unroll 1
                for (int r = 0; r < p; ++r) lin = fma(mw[r], zq[r * GPC_T + tid], lin);
                gm[g * GPC_T + tid] = m + lin;
            }
            if (want_var) {
                __syncthreads();                                     // (red is read above)
                // 3. W = L^{-1} K* on the matrix pipe, the squares summed per column
                const double* Lg = a.Li + (size_t)g * a.li_len;
                double ss0 = 0.0, ss1 = 0.0;
                for (int rr = 0; rr * GPC_NW < NB; ++rr) {
                    const int b = rr * GPC_NW + ((rr & 1) ? GPC_NW - 1 - wave : wave);
                    if (b >= NB) continue;
                    const double* Lb = Lg + (size_t)b * (b + 1) / 2 * 256;   // block row b: (b + 1) 4 k-steps of 64 values
                    gpc_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
                    const int nk = (b + 1) * 4;
#pragma unroll 4
                    for (int k4 = 0; k4 < nk; ++k4) {
                        const double av = Lb[(size_t)k4 * 64 + lane];           // L^{-1}[16 b + col][4 k4 + kq]
                        const double* kr = Kp + (size_t)(4 * k4 + kq) * GPC_T + col;
                        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kr[0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kr[16], acc1, 0, 0, 0);
                    }
                    // C/D map: column lane & 15, row kq + 4 reg
#pragma unroll
                    for (int q = 0; q < 4; ++q) { ss0 = fma(acc0[q], acc0[q], ss0); ss1 = fma(acc1[q], acc1[q], ss1); }
                }
                red[(wave * 4 + kq) * GPC_T + col] = ss0;
                red[(wave * 4 + kq) * GPC_T + 16 + col] = ss1;
                __syncthreads();
                if (gpc_v(tid) < GPC_T) {
                    double s = 0.0;
#pragma unroll 1
                    for (int q = 0; q < GPC_NW * 4; ++q) s += red[q * GPC_T + tid];
                    double v = s2 - s;
                    if (gpc_v(fl) & 16) v += par_v[4 * g + 1];
                    gv[g * GPC_T + tid] = v;
                }
            }
            __syncthreads();                                         // (zq, Kp and red are rewritten by the next GP)
        } while (++g < n);

        // ---- score, test, trace: the thread of chain jc (kernels_gp.hip:194-222, mh_test) ----
        if (gpc_v(fl) & 1) {
            const int nn = gpc_v(n), pq = gpc_v(p);          // (per-lane bounds: no loop guard kept in scalar registers)
            double s = 0.0;
            if (gpc_v(mode_v) == CESX_GP_GAMMA) {
                if (gpc_v(fl) & 4) {
#pragma unroll 1
                    for (int i = 0; i < nn; ++i) {
                        double w = 0.0;
#pragma unroll 1
                        for (int q = 0; q <= i; ++q) w = fma(gx_v[(size_t)i * nn + q], gm[q * GPC_T + tid], w);
                        const double d = w - y_v[i];
                        s = fma(d, d, s);
                    }
                } else {
#pragma unroll 1
                    for (int i = 0; i < nn; ++i) { const double d = gm[i * GPC_T + tid] - y_v[i]; s = fma(gx_v[i], d * d, s); }
                }
            } else {
#pragma unroll 1
                for (int i = 0; i < nn; ++i) {
                    double v = gv[i * GPC_T + tid];
                    if (gpc_v(mode_v) == CESX_GP_GAMMA_VAR) v = gx_v[(size_t)i * nn + i] + v;
                    const double d = gm[i * GPC_T + tid] - y_v[i];
                    s += d * d / v + gpc_log(v);                 // (v <= 0: NaN or inf - inf, the test below then rejects)
                }
            }
            if (gpc_v(fl) & 8) {
#pragma unroll 1
                for (int r = 0; r < pq; ++r) {
                    double w = 0.0;
#pragma unroll 1
                    for (int q = 0; q <= r; ++q) w = fma(pr_v[(size_t)r * pq + q], Pp[q * GPC_T + tid] - mu_v[q], w);
                    s = fma(w, w, s);
                }
            } else {
#pragma unroll 1
                for (int r = 0; r < pq; ++r) { const double d = Pp[r * GPC_T + tid] - mu_v[r]; s = fma(pr_v[r], d * d, s); }
            }
            const double php = 0.5 * s;
            double lu;
            if (lp) { lu = *lp; lp += Mv; }
            else lu = gpc_log_uniform(gjc, step, seed_lo, seed_hi);
            if (lu < ph - php) {                             // (a NaN phi(P) compares false; a NaN phi(U) stays stuck)
#pragma unroll 1
                for (int r = 0; r < pq; ++r) Uc[r * GPC_T + tid] = Pp[r * GPC_T + tid];
                ph = php;
                cnt += 1ull;
            }
            if (tp && ++since == stride_v) {
                since = 0;
#pragma unroll 1
                for (int r = 0; r < pq; ++r) tp[(size_t)r * Mv] = (T)Uc[r * GPC_T + tid];
                tp += (size_t)pq * Mv;
            }
        }
        // (the next step's xi goes to zq, which nobody reads here; the barrier behind it orders Uc and Pp)
    }

    if (gpc_v(fl) & 1) {
#pragma unroll 1
        for (int r = 0; r < p; ++r) U_j[(size_t)r * Mv] = (T)Uc[r * GPC_T + tid];
        *phi_j = ph;
        *cnt_j = cnt;
    }
}

template <typename T>
static int gp_run_t(Engine& e, int mode, uint64_t step_index, int n_steps, int stride, bool nugget, void* U, void* trace,
                    const void* xi, const double* logu, hipStream_t s) {
    GpChainArgs<T> a{};
    a.U = (T*)U; a.trace = (T*)trace; a.xi = (const T*)xi; a.logu = logu;
    a.phi = e.mh.phi; a.cnt = e.mh.cnt;
    a.M = e.J; a.j_offset = e.cfg.j_offset;
    a.seed_lo = (unsigned)e.cfg.seed; a.seed_hi = (unsigned)(e.cfg.seed >> 32);
    a.step0 = (unsigned)(step_index | 0x80000000ull); a.n_steps = n_steps; a.stride = stride;
    a.p = e.p; a.n = e.gp.n; a.Jt = e.gp.Jt; a.Jp = e.gp.Jp; a.li_len = e.gp.li_len;
    a.A = e.gp.A; a.c = e.gp.c; a.Z = e.gp.Z; a.par = e.gp.par; a.mw = e.gp.mw; a.alpha = e.gp.alpha; a.Li = e.gp.Li;
    a.mode = mode; a.nugget = nugget ? 1 : 0;
    a.y = e.d_y; a.gw = e.d_gw; a.gam = e.d_Gamma; a.Lg = e.whiten ? e.d_Wh : nullptr;
    a.mu = e.d_mu; a.sw = e.d_sw; a.LSi = e.diag_sigma ? nullptr : e.mh.LSi.get();
    a.a = e.mh.a; a.bS = e.mh.bS;
    const size_t lds = gpc_lds_doubles(e.p, e.gp.Jp, e.gp.n) * 8;
    auto kern = gp_chain_kernel<T>;
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((e.J + GPC_T - 1) / GPC_T)), dim3(GPC_THREADS), lds, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

bool gp_run_fits(int p, int Jp, int n_gp) { return gpc_lds_doubles(p, Jp, n_gp) * 8 + (size_t)GPC_RED * 8 <= GPC_LDS_BUDGET; }

int launch_gp_run(Engine& e, int mode, uint64_t step_index, int n_steps, int stride, bool nugget, void* U, void* trace,
                  const void* xi, const double* logu, hipStream_t s) {
    if ((e.J + GPC_T - 1) / GPC_T >= (1LL << 31)) { e.err = "cesx_gp_run: too many tiles of chains for one launch"; return CESX_EUNSUPPORTED; }
    return e.cfg.dtype == CESX_F32 ? gp_run_t<float>(e, mode, step_index, n_steps, stride, nugget, U, trace, xi, logu, s)
                                   : gp_run_t<double>(e, mode, step_index, n_steps, stride, nugget, U, trace, xi, logu, s);
}

}  // namespace cesx
