// Internal declarations shared by the HIP translation units of libcesx.so.
// gfx950 (MI355X / CDNA4) only.
#pragma once
#include <array>
#include <cstddef>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/cesx.h"
#include "cesx_stages.h"

namespace cesx {

constexpr int WAVE = 64;

// ---------------------------------------------------------------------------
// MFMA traits.  A/B operand lane map for both shapes: index within the tile =
// lane % TILE, k within the instruction = lane / TILE (one element per lane).
// ---------------------------------------------------------------------------
template <typename T> struct Mfma;

template <> struct Mfma<float> {
    static constexpr int TILE = 32;   // v_mfma_f32_32x32x2_f32
    static constexpr int KSTEP = 2;   // k values consumed per instruction
    static constexpr int NACC = 16;   // accumulator elements per lane
    static constexpr int VEC = 4;     // elements per 16-byte LDS read
    using acc_t = float __attribute__((ext_vector_type(16)));
    using vec_t = float __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
    // C/D map: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    static __device__ __forceinline__ int crow(int lane, int reg) {
        return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    }
    static __device__ __forceinline__ int ccol(int lane) { return lane & 31; }
};

template <> struct Mfma<double> {
    static constexpr int TILE = 16;   // v_mfma_f64_16x16x4_f64
    static constexpr int KSTEP = 4;
    static constexpr int NACC = 4;
    static constexpr int VEC = 2;
    using acc_t = double __attribute__((ext_vector_type(4)));
    using vec_t = double __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // f64 C/D map differs from the f32 family: col = lane & 15, row = (lane >> 4) + 4 * reg
    static __device__ __forceinline__ int crow(int lane, int reg) { return (lane >> 4) + 4 * reg; }
    static __device__ __forceinline__ int ccol(int lane) { return lane & 15; }
};

// Gram kernels: blocks per wave (accumulator budget: 5 x 16 / 9 x 8 VGPRs of the 128 a wave has at
// 4 waves per SIMD); the host's work partition and both Gram kernels use the same constant.
template <typename T> struct GramCfg;
template <> struct GramCfg<float>  { static constexpr int NBW = 4; };
template <> struct GramCfg<double> { static constexpr int NBW = 8; };

// one LDS-DMA piece: 64 lanes x 16 B from per-lane global addresses to lds_dst + 16 lane (M0 = the
// wave-uniform LDS byte address; hipcc keeps nothing live in M0 across a statement).  The compiler's
// s_waitcnt bookkeeping does not see these loads: callers wait with an explicit vmcnt.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(gsrc), "s"(lds_dst) : "memory");
}

// The same piece from a wave-uniform 64-bit base (an SGPR pair) plus a 32-bit per-lane byte offset: the address
// arithmetic of a piece is scalar, no vector ALU instruction is spent on it (on gfx950 every VALU instruction in an
// f32 MFMA loop costs the matrix pipe ~4 cycles, a 64-bit v_mul four times that).
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" :: "s"(sbase), "v"(voff), "s"(lds_dst) : "memory");
}

// Slab layout of one partial Gram block ("accumulator-major"): element ((q * 64 + lane) * VEC + e)
// is accumulator register VEC * q + e of lane `lane`, so a wave stores a block with 16-byte stores
// of consecutive lanes (1 KiB per instruction).  (row, col) of the first element of group `grp`
// (= q * 64 + lane); the VEC elements of a group are rows row0 + e (f32) / row0 + 4 e (f64).
template <typename T> __host__ __device__ inline void slab_group_rc(int grp, int& row0, int& col, int& rstep);
template <> __host__ __device__ inline void slab_group_rc<float>(int grp, int& row0, int& col, int& rstep) {
    const int q = grp >> 6, lane = grp & 63;
    row0 = 8 * q + 4 * (lane >> 5); col = lane & 31; rstep = 1;          // reg = 4 q + e: (reg & 3) + 8 (reg >> 2) + 4 lh
}
template <> __host__ __device__ inline void slab_group_rc<double>(int grp, int& row0, int& col, int& rstep) {
    const int q = grp >> 6, lane = grp & 63;
    row0 = (lane >> 4) + 8 * q; col = lane & 15; rstep = 4;              // reg = 2 q + e: (lane >> 4) + 4 reg
}

// j (or k) values covered by one 16-byte fragment read of every lane: the
// KSTEP lane groups each take VEC consecutive values -> KSTEP * VEC = 8.
constexpr int GROUP = 8;

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011).  counter = (particle_lo, particle_hi,
// row_quad, step), key = seed.  oracle/philox.py restates this in numpy.
// ---------------------------------------------------------------------------
struct uint4x { uint32_t x, y, z, w; };

__host__ __device__ __forceinline__ uint4x philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                         uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return {c0, c1, c2, c3};
}

// ---- the Metropolis test of the chain samplers (mh_accept_kernel, gp_score_kernel): one copy, because the two stages and
// oracle/philox.py / oracle/stage_ref.py have to agree on it bit for bit ----

// log of the uniform of global chain gj at step word `step`: row-quad word 0xffffffff, which no xi row uses (include/cesx.h)
__device__ __forceinline__ double mh_log_uniform(unsigned long long gj, unsigned step, unsigned seed_lo, unsigned seed_hi) {
    const uint4x r = philox4x32_10((uint32_t)gj, (uint32_t)(gj >> 32), 0xffffffffu, step, seed_lo, seed_hi);
    const unsigned long long m53 = ((unsigned long long)(r.x >> 5) << 26) | (unsigned long long)(r.y >> 6);
    return log(((double)m53 + 0.5) * 1.1102230246251565404e-16);      // 2^-53
}

// The chains' state as a score kernel sees it: the tail of MhArgs and GpScoreArgs, filled by mh_chains (below Engine)
struct MhChains {
    long long j_offset;
    double* phi; unsigned long long* cnt;
    const double* logu;                    // nullptr: the device uniform of `step`
    unsigned seed_lo, seed_hi, step;
    int start;                             // 1: phi := phi(X), counters cleared, no test
};

// Chain j with phi(X_j) = ph.  start: the chain's phi and counter are set.  Otherwise the test
// log u < phi(U_j) - ph (ces/sample.py:188-191, :98-101), phi and the counter follow; true: the chain takes X_j.
// (c by value: both kernels then compile to the instructions they had with the test written out in each; through a
// reference mh_accept_kernel comes out in another block order.)
__device__ __forceinline__ bool mh_test(const MhChains c, long long j, double ph) {
    if (c.start) {
        c.phi[j] = ph;
        c.cnt[j] = 0ull;
        return false;
    }
    const double lu = c.logu ? c.logu[j] : mh_log_uniform((unsigned long long)(c.j_offset + j), c.step, c.seed_lo, c.seed_hi);
    if (lu < c.phi[j] - ph) {
        c.phi[j] = ph;
        c.cnt[j] += 1ull;
        return true;
    }
    return false;
}

// Box-Muller radius sqrt(-2 ln u), u in [2^-25, 1): the bare v_log_f32 / v_sqrt_f32 (1 ulp each; no denormal scaling,
// no Newton step around the square root -- the library forms cost 14 % of the noise draw's vector instructions, and the
// draw is paid for in full wherever it runs: round 4).  Shared by normal4 and the in-kernel draw of kernels_update2.hip.
__device__ __forceinline__ float bm_radius(float u) {
    return __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u));      // -2 ln 2 * log2(u)
}

// Four N(0,1) draws for rows 4q..4q+3 of one particle (Box-Muller on two pairs).
__device__ __forceinline__ void normal4(uint4x r, float out[4]) {
    const float s = 5.9604644775390625e-08f;   // 2^-24
    float u0 = ((float)(r.x >> 8) + 0.5f) * s, u1 = ((float)(r.y >> 8) + 0.5f) * s;
    float u2 = ((float)(r.z >> 8) + 0.5f) * s, u3 = ((float)(r.w >> 8) + 0.5f) * s;
    float ra = bm_radius(u0), rb = bm_radius(u2);
    // v_sin_f32 / v_cos_f32 take their argument in revolutions
    out[0] = ra * __builtin_amdgcn_cosf(u1);
    out[1] = ra * __builtin_amdgcn_sinf(u1);
    out[2] = rb * __builtin_amdgcn_cosf(u3);
    out[3] = rb * __builtin_amdgcn_sinf(u3);
}
__device__ __forceinline__ void normal4(uint4x r, double out[4]) {
    const double s = 2.3283064365386963e-10;   // 2^-32
    const double twopi = 6.283185307179586476925286766559;
    double u0 = ((double)r.x + 0.5) * s, u1 = ((double)r.y + 0.5) * s;
    double u2 = ((double)r.z + 0.5) * s, u3 = ((double)r.w + 0.5) * s;
    double ra = sqrt(-2.0 * log(u0)), rb = sqrt(-2.0 * log(u2));
    double sa, ca, sb, cb;
    sincos(twopi * u1, &sa, &ca);
    sincos(twopi * u3, &sb, &cb);
    out[0] = ra * ca; out[1] = ra * sa; out[2] = rb * cb; out[3] = rb * sb;
}

// One workgroup's share of a noise block xi[p][J] (256 threads; thread = rows 4 by .. 4 by + 3 of NP consecutive
// particles of column block bx): the body of noise_kernel (kernels_update.hip).
template <typename T, bool VEC4>
__device__ __forceinline__ void noise_body(T* __restrict__ xi, int p, long long J, long long j_offset, unsigned seed_lo,
                                           unsigned seed_hi, unsigned step, unsigned bx, unsigned by) {
    constexpr int NP = VEC4 ? 4 : 1;
    const long long j0 = ((long long)bx * 256 + threadIdx.x) * NP;
    const int q = (int)by;
    if (j0 >= J) return;
    T z[NP][4];
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const unsigned long long gj = (unsigned long long)(j_offset + j0 + c);
        const uint4x r = philox4x32_10((uint32_t)gj, (uint32_t)(gj >> 32), (uint32_t)q, step, seed_lo, seed_hi);
        normal4(r, z[c]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (4 * q + e >= p) break;
        T* dst = xi + (size_t)(4 * q + e) * J + j0;
        if (VEC4) {
            typedef T v4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<v4*>(dst) = v4{z[0][e], z[NP > 1 ? 1 : 0][e], z[NP > 2 ? 2 : 0][e], z[NP > 3 ? 3 : 0][e]};
        } else {
            dst[0] = z[0][e];
        }
    }
}

// ---------------------------------------------------------------------------
// Packed fp64 moment buffer (the only data that crosses GPUs).  The part that
// depends on U alone comes first and is contiguous, so that it can be reduced
// (and chol(C) started) before the rest of the Gram is finished:
//   [ N | sum a (p) | S_aa (p x p) ][ sum b (n) | S_ab (p x n) | S_bb (n x n) | lagged q sums (2) ]
// ---------------------------------------------------------------------------
struct MomLayout {
    int p, n;
    __host__ __device__ size_t sa() const { return 1; }
    __host__ __device__ size_t Saa() const { return 1 + (size_t)p; }
    __host__ __device__ size_t uu_len() const { return 1 + (size_t)p + (size_t)p * p; }
    __host__ __device__ size_t sb() const { return uu_len(); }
    __host__ __device__ size_t Sab() const { return sb() + n; }
    __host__ __device__ size_t Sbb() const { return Sab() + (size_t)p * n; }
    __host__ __device__ size_t tail() const { return Sbb() + (size_t)n * n; }
    __host__ __device__ size_t len() const { return tail() + 2; }
};

// ---------------------------------------------------------------------------
// Gram work partition (host builds it once per engine).
// ---------------------------------------------------------------------------
struct GramPlan {
    int tile;            // Mfma<T>::TILE
    int nbr;             // block rows = ceil((p+n)/tile)
    int nblocks;         // lower-triangular blocks
    int ntypes;          // workgroup types
    int max_rb;          // max staged row blocks over types
    int nbw;             // per-wave block capacity (compile-time constant of the kernel)
    // Every type gets a number of J-slices (workgroups) proportional to its block count, so that
    // all workgroups of a launch carry the same amount of MFMA work whatever the shape of the types.
    // flattened tables uploaded to the device:
    //  type_hdr[type*8 + {0: nrb, 1: rows_off, 2: blocks_off, 3: blocks of the type, 4: first workgroup,
    //                     5: slices, 6: first slab (in blocks), 7: first row-sum slot}]
    //  rows[rows_off + i]            = global block row of compact row i (| 1<<16: this type reports its sums)
    //  wblk[(blocks_off + wave*nbw + b)*3 + {0,1,2}] = {ia, ib, block index inside the type} or ia = -1
    //  blk_rc[out*5 + {0..4}] = (R, C) of output block, its first slab, slab stride (blocks), slices
    //  row_own[br*2 + {0,1}]  = first row-sum slot and slices of the type that owns block row br (slices 0: not owned)
    std::vector<int> type_hdr, rows, wblk, blk_rc, row_own;
    int total_wgs = 0, total_slabs = 0, total_rs = 0;
    int own_lo = 0, own_hi = 0;   // block rows [own_lo, own_hi) whose row sums this plan reports
};
// subset: 0 = all lower-triangular blocks, 1 = the blocks that only involve the first pbU
// block rows (U x U: everything chol(C) needs), 2 = all the others
GramPlan make_gram_plan(int P, int tile, int nbw, int max_rows_lds, int subset = 0, int pbU = 0, int min_types = 1,
                        int wg_budget = 256, long long ntiles = 1 << 30);

// one Gram launch: plan + its device tables and partial-result buffers
struct GramPart {
    GramPlan plan;
    int *d_type_hdr = nullptr, *d_rows = nullptr, *d_wblk = nullptr, *d_blk_rc = nullptr, *d_row_own = nullptr;
    void* d_slabs = nullptr;            // per type [slices][blocks of the type][tile*tile] engine dtype
    double* d_rowsum_part = nullptr;    // [row-sum slots][p+n]
    // the plan's flattened tables: allocated and uploaded from this one list (gram_part_alloc); Engine::core owns the memory
    struct Table { int** dev; const std::vector<int>* host; };
    std::array<Table, 5> tables() {
        return {{{&d_type_hdr, &plan.type_hdr}, {&d_rows, &plan.rows}, {&d_wblk, &plan.wblk}, {&d_blk_rc, &plan.blk_rc},
                 {&d_row_own, &plan.row_own}}};
    }
};

// ---------------------------------------------------------------------------
// Engine state
// ---------------------------------------------------------------------------
struct Scalars {              // device-resident fp64 scalars written by K2
    double hk, t_new, sqrt2hk, alpha;
    double self_bias, self_bias_data, bias_data, bias;
    double radspec, frob2, tr_suu, absmax;
    double spare[4];
    int    status, pad;
    unsigned long long seq;   // host copy only: step counter written last by publish_kernel
};

// Finalisation of a step's data metrics and publication of its scalars to the host: the fixed-order fp64 sum of the
// update kernel's per-workgroup partials (sums[0..1] = sum over workgroups of {q_r^2, q_e^2}), this shard's
// contribution to the two data metrics (divided by the GLOBAL ensemble size), from the tail of the all-reduced moment
// buffer the previous step's global values (multi-device runs), then -- host != nullptr -- the copy of the scalars
// into the host-mapped result block, its sequence number last.  Run by ONE workgroup of 256 threads: the
// metric_final kernel, or (single-device fast path) an extra workgroup of the NEXT step's U x U reduce launch, so
// that no one-workgroup kernel sits between the update kernel and the next Gram launch.
struct MetricFin {
    const double* part; int nparts; const double* mom; size_t tail_off; double* sums; Scalars* sc;
    Scalars* host; unsigned long long seq;
    double N;            // > 0: the global ensemble size (else read from mom[0])
};
__device__ __forceinline__ void metric_final_body(const MetricFin& f) {
    __shared__ double mf_red[2][4];
    __shared__ double mf_out[4];
    constexpr int ND = offsetof(Scalars, seq) / 8;
    // 256 threads do the work whatever the launch's block size is (the summation order is part of the result);
    // the other waves of a larger block leave (a finished wave does not hold up the barriers below)
    constexpr unsigned MF_THREADS = 256;
    if (threadIdx.x >= MF_THREADS) return;
    // the scalars earlier kernels of the step wrote (hk, t, bias ...): read FIRST, beside the partial sums -- the
    // chain of dependent round trips of this one workgroup is what a launch that carries it waits for
    double mine = 0.0;
    if (f.host != nullptr && threadIdx.x < ND)
        mine = __hip_atomic_load(reinterpret_cast<const double*>(f.sc) + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double lag0 = 0.0, lag1 = 0.0, Nm = f.N;          // (thread 0's inputs from the moment buffer: also up front)
    if (threadIdx.x == 0) {
        lag0 = f.mom[f.tail_off]; lag1 = f.mom[f.tail_off + 1];
        if (!(Nm > 0.0)) Nm = f.mom[0];
    }
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < f.nparts; i += MF_THREADS) { a += f.part[(size_t)i * 2]; b += f.part[(size_t)i * 2 + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
    if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 4) { mf_red[0][threadIdx.x >> 6] = a; mf_red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0;
        for (int i = 0; i < (int)(MF_THREADS >> 6); ++i) { a += mf_red[0][i]; b += mf_red[1][i]; }
        const double N = Nm;
        f.sums[0] = a; f.sums[1] = b;
        mf_out[0] = f.sc->bias_data = a / N;
        mf_out[1] = f.sc->self_bias_data = b / N;
        mf_out[2] = f.sc->spare[1] = lag0 / N;          // lagged global bias-data
        mf_out[3] = f.sc->spare[2] = lag1 / N;          // lagged global self-bias-data
    }
    if (f.host == nullptr) return;
    // last kernel of an eks / aldi step: publish the results (see publish_kernel)
    __syncthreads();
    if (threadIdx.x < ND) {
        const int i = threadIdx.x;
        const double v = i == (int)(offsetof(Scalars, bias_data) / 8) ? mf_out[0]
                       : i == (int)(offsetof(Scalars, self_bias_data) / 8) ? mf_out[1]
                       : i == (int)(offsetof(Scalars, spare) / 8) + 1 ? mf_out[2]
                       : i == (int)(offsetof(Scalars, spare) / 8) + 2 ? mf_out[3] : mine;
        reinterpret_cast<double*>(f.host)[i] = v;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&f.host->seq, f.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Engine {
    cesx_config cfg{};
    std::string err;
    bool problem_set = false, shift_valid = false;
    struct Factor {                     // chol(C) of the current moments (kernels_dense.hip: launch_chol_async, factor_C, join_side)
        bool inflight = false;          // cesx_chol_async ran for the current moments and launch_dense has not joined the side stream yet
        bool fused_center = false;      // the last cesx_chol_async fused the centring into the factorisation's load (no U-only centring launch)
        bool img = false;               // the last cesx_chol_async stores L into d_Wq (image_ok for its update rule)
        bool signals = false;           // the last cesx_chol_async stores seq into d_cholflag (its last kernel does)
        unsigned long long seq = 0;     // cesx_chol_async calls so far: the sequence number of the last one
        unsigned long long waited_seq = 0; hipStream_t waited_stream = nullptr;      // the last one launch_dense joined, and on which stream
        bool polled = false;            // the last launch_dense (Step / Drift) joined through the polled word, not the event
        bool image_only = false;        // the last factorisation into d_L wrote the chained image only: d_L does not hold it (ensure_factor)
    } fac;
    bool fuse_center_auto = true;     // no CESX_FUSE_CENTER given: fused where the step takes the hk-free form AND the second Gram launch is
                                      // short (Engine::gram_b_short: small ensembles -- the side chain is then the step's critical path and
                                      // the host's launches its floor; C4 0.0790 -> 0.0728 ms/step, round 4), not at C2 (see below)
    bool gram_b_short = false;        // the second Gram launch's MFMA time is below ~60 us (plan_gram_parts)
    bool fuse_center_ok = false;      // CESX_FUSE_CENTER=1 switches that on (round 4: also with the hk-free form -- the tail launch then forms C, M, ubar
                                      // and the trace / bias sums itself; measured 0.3988 against 0.3952 ms/step at C2: the side chain ends 15 us
                                      // earlier, the noise draw behind it meets the end of the second Gram launch, and the tail launch is longer).  Measured at C2 (round 3, row sums staged through LDS): the factorisation
                                      // takes 107 us instead of 13 + 99, the side chain ends 4.5 us earlier, the step gains 0.2-1 % over 400 steps and
                                      // nothing in the 20-step line (the caller's stream -- second Gram launch, reduce, centring -- is the critical path)
    bool overlap_chol = true;      // run chol(C) on the side stream beside the second (non U x U) part of the Gram
                                   // (CESX_OVERLAP=0 disables)
    int p = 0, n = 0, P = 0;
    int64_t J = 0, Jg = 0;
    size_t esz = 4;               // sizeof(T)
    bool diag_sigma = false;
    // Dense Gamma (the reference's pde examples use a sample covariance, examples/notebooks/lorenz63.ipynb): the engine
    // WHITENS the data once per step -- G~ = L_Gamma^{-1} G with Gamma = L L^T (one triangular n x n x J product on the matrix
    // pipe, the update kernel's own code, ~4 GFLOP at C2), y~ = L^{-1} y, Gamma~ = I -- and every kernel behind it runs the
    // diagonal-Gamma path: D = (1/J) E^T Gamma^{-1} R = (1/J) E~^T R~ (ces/calibrate.py:429/:461/:503), the data metrics
    // (:434-435), the recomputed gain C_ug (hk C_gg + Gamma)^{-1} (g - y) (:440-441/:472-473) and K (g - y) are all invariant.
    // (Round 4 kept Gamma^{-1} in the small algebra -- fp64 GEMMs for the Frobenius term and K -- and ran a VALU pass over G for
    //  the per-particle metrics: 1.23 ms per step against 0.39 for diagonal Gamma.)
    bool whiten = false;
    void *d_Wwh = nullptr, *d_Wwh_f = nullptr;   // L_Gamma^{-1} zero padded [rpad][kn], row-major and in the update kernels' fragment-major order
    void* d_Gw = nullptr;                        // [n][J] the whitened data of the current step (allocated with the first dense problem)
    const void* gw_src = nullptr;                // ... of this caller array, whitened on gw_stream
    hipStream_t gw_stream = nullptr;
    unsigned long long gw_calls = 0;             // Engine::moments_calls when it was whitened
    std::vector<double> h_LG, h_Li;              // host copies of L_Gamma and its inverse (cesx_debug_dense reports in the caller's coordinates)

    // problem data (fp64) on device
    double *d_y = nullptr, *d_mu = nullptr, *d_ustar = nullptr;
    double *d_Gamma = nullptr, *d_gw = nullptr;    // the engine's (diagonal, or whitened: identity) Gamma and gw = diag(Gamma^{-1})
    double *d_Sigma = nullptr, *d_Sinv = nullptr, *d_sw = nullptr;
    // centring shift
    double* d_shift64 = nullptr;   // [p+n]
    void*   d_shiftT = nullptr;    // [p+n] engine dtype
    void*   d_yT = nullptr;        // y in engine dtype
    void*   d_gwT = nullptr;       // diag(Gamma^{-1}) in engine dtype
    // gram: part 0 = U x U blocks (all chol(C) needs), part 1 = the rest
    GramPart gram[2];
    MomLayout ml{};
    // stats partials
    int colsum_slices = 0;
    double* d_colsum_part = nullptr;
    // moments
    size_t mom_len = 0;
    double* d_mom = nullptr;
    double* d_sums = nullptr;      // [1+p+n]
    double* d_sums_w = nullptr;    // [1+p+n] the same with the G part whitened (dense Gamma)
    // dense workspace (fp64)
    double *d_ubar = nullptr, *d_gbar = nullptr, *d_m = nullptr;
    double *d_C = nullptr, *d_L = nullptr, *d_Cug = nullptr, *d_See = nullptr, *d_Srr = nullptr;
    double *d_dg = nullptr;
    double *d_K = nullptr, *d_Kp = nullptr, *d_M = nullptr, *d_P = nullptr, *d_PK = nullptr;
    double *d_t1 = nullptr, *d_t2 = nullptr, *d_t3 = nullptr, *d_t4 = nullptr;   // max(p,n)^2 each
    double *d_Wh = nullptr;        // L_Gamma^{-1} in fp64 (dense Gamma: the centring sums of a fresh ensemble are whitened with it)
    // warm-started SPD inverses of K2 (kernels_dense.hip, spd_inverse): the previous step's inverse of the gain matrix (0, n x n) and
    // of the EKS matrix (1, p x p), three n_max^2 scratch matrices, 2 x ceil(n_max/16)^2 residual partials, the verdict word
    double *d_ns_x[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // [which][ns_cur[which]]: the previous inverse; the other one: this step's
    int ns_cur[2] = {0, 0};
    double *d_ns_r[3] = {nullptr, nullptr, nullptr}, *d_ns_parts = nullptr;
    int* d_ns_skip = nullptr;
    bool ns_ok = true;             // CESX_NS_WARM=0: always the factorisation
    double ns_r0_last = 1e300;     // ||I - A X_prev||_F^2 of the last step's warm-start attempt (cesx_result reads it from the result block)
    double *d_spec = nullptr;      // spectral rule: {sum 2^-k log N_k, 2^-k, degenerate flag, pad} + 2 x ceil(n/16)^2 partial sums of squares
    double *d_absmax = nullptr;    // [1]
    void   *d_rowc = nullptr;        // [kn][4] {gbar_i, y_i, 1/Gamma_ii, 0} engine dtype (K3 data metrics)
    double *d_metric_part = nullptr; // [blocks][2] per-workgroup {sum q_r^2, sum q_e^2}
    double *d_metric_sums = nullptr; // [2] this shard's sums of the last apply
    double *d_mv = nullptr;        // matvec results [6][max(p,n)]
    double *d_part = nullptr;      // reduction partials
    Scalars* d_scal = nullptr;
    double* d_absmax_part = nullptr;
    // update coefficients (engine dtype)
    int bk = 16, kp = 0, kn = 0, ktot = 0, rpad = 0;
    double* d_Lwork = nullptr;     // p > 256: work copy of C for the blocked Cholesky [potrf_ld(p)]^2
    void* d_W = nullptr;           // [rpad][ktot]
    void* d_Wf = nullptr;          // the same matrix in the fragment-major order of kernels_update2.hip (fp32) / kernels_update3.hip (fp64)
    bool update_v2 = true;         // fp32 K3 through the LDS-DMA kernel (CESX_UPDATE_V1=1 switches back)
    int  center_u_wgs = 256;       // workgroups of the U-only centring on the side stream (see plan_gram_parts)
    bool gram_v2 = true;           // K1 through the LDS-DMA kernel when the shapes allow (CESX_GRAM_V1=1 switches back)
    int num_cus = 256;
    void* d_bias = nullptr;        // [rpad]
    // ---- ALDI with the time step kept OUT of the update coefficients (round 4; launch_dense, "hk-free") ----
    // U_next = hk ( sqrt(2/hk) L xi + (a I - M + I/hk) U - K G + b' ),  b' = K y + M mu - a ubar: the image
    // Wq = [ L | a I - M (+ 1/hk on the diagonal) | -K ] needs hk in p diagonal entries only.  L is written by the
    // factorisation itself (it stores its panels into the image as it finishes them, on the side stream), everything else
    // by ONE launch of the caller's stream behind the second reduce (tail_aldi_kernel: -K and a I - M rows straight from the
    // moments, the four matvecs, the Frobenius partials; its last workgroup, by ticket, joins the side stream, sums the
    // partials and writes hk, b', the diagonal and the next shift), and K3 takes hk and sqrt(2hk) from the scalar block at
    // run time: xi segment first, accumulators rescaled once by sqrt(2/hk), the result times hk in the epilogue.
    void* d_Wq = nullptr;          // [rpad][ktot] fragment-major (wf_index), fp32; zero outside what the kernels above write
    unsigned* d_ticket = nullptr;  // arrival counter of tail_aldi_kernel
    bool hkfree_ok = true;         // CESX_HKFREE=0 switches the path off
    bool update_small = true;      // CESX_UPDATE_SMALL=0: update2_kernel also for out_rows <= 64 (dev A/B)
    bool last_hkfree = false;      // the last launch_dense took the path: the update launch reads d_Wq in the order [xi; U; G]
    // ---- K3 through the Cholesky factor (round 6; kernels_update4.hip) ----
    // With a diagonal Sigma, C Sigma^{-1} (U - mu) = L (L^T Sigma^{-1} U) - M mu: two triangular products instead of the dense M U.
    // d_Wq then holds the CHAINED image (wc_index_L / _Lt / _K): the factorisation stores every panel twice (L, and transposed and
    // scaled), the tail launch stores -K, nothing stores a I - M.  Decided by the problem and the shape alone (cesx_set_problem):
    // every call flow of a problem runs the same kernels.
    bool chain = false;            // d_Wq is in the chained layout and the hk-free step launches update4_kernel
    bool chain_ok = true;          // CESX_CHAIN=0: the hk-free form of round 4 (update2_kernel<., true>) also where the chained one qualifies
    void* d_xi_tmp = nullptr;      // [p][J] a noise block drawn right in front of update4_kernel when none was prefetched or injected
    void* d_Wfwd = nullptr;        // forward-map staging [npad][kp]
    void* d_Wfwd_f = nullptr;      // the same map in the fragment-major order of the LDS-DMA update kernels (cesx_forward_set_lineal)
    void* d_bfwd = nullptr;        // [rpad] its offset b
    bool  fwd_set = false, fwd_has_b = false;
    double *d_A64 = nullptr, *d_b64 = nullptr;   // the installed map in fp64 (n x p, n): cesx_moments_rest_lineal
    double *d_lvec = nullptr;                    // [2][n] c = A s_u + b - s_g and A sa
    // ---- the stages behind Calibrate: each struct owns its device memory and has one drop() (cesx_stages.h) ----
    std::vector<double> h_LSi, h_mu;   // L_Sigma^{-1} and mu of the problem (cesx_set_problem): the dense prior's image
    std::vector<double> h_y_raw, h_Gamma_raw;       // y and Gamma as cesx_set_problem got them (UNWHITENED; Gamma symmetric from its lower triangle)
    std::vector<double> h_yw, h_gw;                 // host copies of d_y (whitened for a dense Gamma) and d_gw: cesx_mh_run_map passes the problem by value
    std::vector<double> h_sw;                       // host copy of d_sw (1 / Sigma_rr): cesx_mh_langevin_run_map passes lv_score's numbers by value
    MhState mh;                        // Metropolis-Hastings over the columns (cesx_mh_*, kernels_mh.hip)
    GpState gp;                        // GP emulator over the columns (cesx_gp_*, kernels_gp.hip)
    GpDenseState gpd;                  // the dense per-chain Sigma of CESX_GP_DENSE (cesx_gp_dense_set, kernels_gpdense.hip)
    GpProjState gpp;                   // Sigma projected to k x k of CESX_GP_PROJ (cesx_gp_proj_set, kernels_gpproj.hip)
    GpFitState gf;                     // GP training (cesx_gpfit_*, kernels_gpfit.hip)
    DarcyState dc;                     // Darcy forward map (cesx_darcy_*, kernels_darcy.hip)
    L96State l9;                       // Lorenz '96 forward map (cesx_lorenz_*, kernels_l96.hip)
    L63State l6;                       // Lorenz '63 forward map (cesx_lorenz_three_*, kernels_l63.hip)
    MapState mp;                       // closed-form maps and their fused chain kernel (cesx_map_*, cesx_mh_run_map, kernels_maps.hip)
    ChainSumState cs;                  // streaming summaries of the chains' draws (cesx_chain_summary_*, kernels_chainsum.hip)
    ChainHistState ch;                 // streaming marginals of the chains' draws (cesx_chain_hist_*, kernels_chainhist.hip)
    ChainAcfState ca;                  // streaming lagged sums of the chains' draws (cesx_chain_acf_*, kernels_chainacf.hip)
    // per-kernel profiling (cesx_profile_*)
    int prof_part = 0;                 // which moments launch (0: U x U, 1: the rest) the next profiled Gram launch is
    unsigned long long prof_step = 0;  // bumped by every first-half entry point (cesx_moments_uu*): the step the next profiled launches belong to
    bool profile = false;
    int  profile_only = -1;            // cesx_profile_enable(h, 3 / 4): only the update (1) / the moments (0) launches carry events
    bool profile_gap_only = false;     // cesx_profile_enable(h, 2): bind ONLY the stop of the second moments launch and the start of the
                                       // update launch (the gap between them, cesx_profile_gap): a step whose launches carry start AND stop
                                       // events runs ~70 us longer and its gap reads anywhere between 40 and 150 us
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[2];
    std::vector<unsigned long long> prof_tag[2];       // the step (Engine::moments_calls at the launch) each pair belongs to: cesx_profile_gap pairs events of ONE step
    std::vector<hipEvent_t> prof_pool;
    long long* d_clk = nullptr;    // [4] {s_memtime, s_memrealtime} ticks of the last PROFILED update launch (workgroup 0, wave 0)
    // results
    Scalars* h_scal = nullptr;           // pinned, device-mapped: the GPU writes results straight into it
    Scalars* h_scal_dev = nullptr;       // device address of h_scal
    unsigned long long seq = 0;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;      // hand-over main -> side (U x U moments reduced) / side -> main (chol(C) done)
    hipStream_t side = nullptr;      // side stream (high priority): U x U Gram, chol(C), the step's last small kernel
    hipEvent_t ev_x[2] = {nullptr, nullptr};   // prefetched noise block b is complete (side stream)
    // Noise blocks drawn ahead by cesx_prefetch_noise, [p][J] engine dtype each.  Two of them: behind chol(C) of the
    // step that asked for block s the side stream draws block s (unless an earlier step already did) AND block s + 1
    // (the lookahead), so that from the second step on the update kernel finds its block complete -- ordered before
    // this step's chol(C) on the side stream, whose event the caller's stream waits for anyway -- and the draw of the
    // next one runs beside K2's latency-bound kernels with nothing waiting for it.
    void* d_xi[2] = {nullptr, nullptr};
    long long xi_step[2] = {-1, -1};                 // step index block b holds (-1: none)
    unsigned long long xi_seq[2] = {0, 0};           // Factor::seq of the cesx_chol_async call that drew block b
    long long xi_want = -1;          // step index asked for by cesx_prefetch_noise, drawn behind the next chol(C)
    bool xi_lookahead = true;        // CESX_NOISE_LOOKAHEAD=0 switches the second draw off
    // ---- the side stream joined through a polled word instead of a barrier packet (round 3, launch_dense) ----
    bool poll_join_ok = true;                     // CESX_POLL_JOIN=0: always join the side stream with the event
    unsigned long long* d_cholflag = nullptr;     // Factor::seq of the last factorisation that completed on the side stream, stored by the kernel itself
    // ---- the polled join made safe (round 4) ----
    int side_prio = 0; bool side_has_prio = false;   // priority of the side stream (cesx_create)
    unsigned long long poll_ticks = 200000000ull; // bound of the poll in 100-MHz wall-clock ticks (2 s; CESX_POLL_TIMEOUT_MS)
    unsigned long long poll_recoveries = 0;       // steps whose poll ran out and that cesx_result re-ran with chol(C) in line
    bool in_retry = false;
    unsigned long long test_drop_signal_at = 0;   // CESX_TEST_DROP_CHOL_SIGNAL (tests): that factorisation does not store its word
    unsigned long long moments_calls = 0;         // cesx_moments* calls so far (a re-run step tells whether a later one read an unwritten ensemble)
    struct LastApply { bool valid = false; cesx_step_params prm{}; const double* mom = nullptr; const void *U = nullptr, *G = nullptr, *xi = nullptr;
                       void* Unext = nullptr; hipStream_t s = nullptr; unsigned long long moments_calls = 0;
                       bool mom_reused = false;      // a later cesx_moments* call was given the same buffer before the result was read: no re-run
                     } last_apply;
    // ---- RCCL communicator of a sharded ensemble (comm.hip; nullptr: none) ----
    void* comm = nullptr;
    void* comm_side = nullptr;     // the side stream's own communicator (ncclCommSplit of `comm`; nullptr: both streams share `comm`)
    int comm_nranks = 0, comm_rank = 0;
    unsigned long long comm_calls = 0, comm_doubles = 0;
    int last_update_grid_x = 0, last_update_grid = 0, last_metric_parts = 0;
    bool pending = false;
    // single-device fast path: the metric finalisation + publication of the last update rides on the next
    // U x U reduce launch (cesx_moments_uu_chol); every other entry point flushes it as a kernel of its own first
    bool met_deferred = false;
    hipStream_t met_stream = nullptr;
    double* d_lag = nullptr;       // [3] {N, lagged sum q_r^2, lagged sum q_e^2} of the moment buffer of the last cesx_apply (K2 copies
                                   // them here: the deferred finalisation reads engine-owned memory, not the caller's buffer)
    cesx_step_params last_prm{};
    // Every d_ pointer above (the GramParts' and d_xi included) points into one of these: allocated through core_alloc, never
    // released before the engine is.  An engine that never allocated (tools/plan_dump.hip) destructs without a dev_free call.
    std::vector<DevBuf<void>> core;
};

// ---------------------------------------------------------------------------
// kernel launchers (defined in the .hip files)
// ---------------------------------------------------------------------------
int launch_colsum(Engine& e, const void* U, const void* G, double* sums, hipStream_t s);
// rowsum_kernel over the `rows` rows of X alone: part[row * nslices + slice], the caller's own buffer
int launch_rowsum(Engine& e, const void* X, int rows, int nslices, double* part, hipStream_t s);
int launch_set_shift(Engine& e, const double* sums, hipStream_t s);
// ---- K1: the moments launches (kernels_gram.hip, kernels_gram2.hip) ----
// The plans of both launches of this engine (Engine::gram[.].plan), with center_u_wgs and gram_b_short; needs p, n, J, Jg, the
// dtype and num_cus, no device.  CESX_EINVAL (Engine::err) when a plan does not fit in LDS.
int plan_gram_parts(Engine& e);
int gram_part_alloc(Engine& e, GramPart& gp);      // the plan's tables (uploaded), its slabs and row-sum slots (zeroed): Engine::core
// One moments launch: the Gram kernel of a part and the fp64 reduce of its slabs into `mom`; call sites name the fields they use.
struct GramLaunch {
    int part = 0;                     // 0: the U x U blocks, 1: the rest
    const void *U = nullptr, *G = nullptr;
    double* mom = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t bound_stop = nullptr;  // != nullptr: bound to the reduce kernel's own completion signal (no marker packet behind it)
    MetricFin fin{};                  // fin.part != nullptr: the previous update's metric finalisation rides on the reduce launch
};
enum class GramKernel {
    None,                                     // the part has no block (the reduce still runs)
    Gram2, Gram2Imm, Gram2Sg, Gram2SgImm,     // gram2_kernel<T, sg, imm>: the LDS-DMA kernel
    Gram1Aligned, Gram1Scalar                 // gram_kernel<T, aligned>: the register-staged kernel
};
// the kernel launch_moments runs for this part of these arrays
GramKernel pick_gram_kernel(const Engine& e, int part, const void* U, const void* G);
int launch_moments(Engine& e, const GramLaunch& L);
// kernels_gram2.hip: the staged rows gram2_kernel takes, and (imm) whether its ds_read offsets reach both slots
bool gram2_rows_ok(int nrows, bool* imm);
int launch_gram2(Engine& e, const GramLaunch& L, GramKernel k);      // k: one of the Gram2 arms
// ---- K2: the dense algebra between the moments and the update (kernels_dense.hip) ----
enum class DensePhase { Step, Drift, Noise };      // everything for eks / aldi; aldi_constant: the drift coefficients, the noise
                                                   // coefficients once hk is known
// One K2 launch; call sites name the fields they use.
struct DenseLaunch {
    const cesx_step_params* prm = nullptr;
    const double* mom = nullptr;      // (Noise: none)
    DensePhase phase = DensePhase::Step;
    hipStream_t s = nullptr;
    bool upd_ok = false;              // an update kernel takes the hk-free image of this step (pick_update_kernel)
};
// center_kernel's `what`
constexpr int CENTER_U = 1;           // the part that depends on U alone (C, M, ubar, the trace / bias partials)
constexpr int CENTER_G = 2;           // the part that involves G
constexpr int CENTER_KEEP_STATUS = 4; // the status word stays: a factorisation with the centring fused into its load already ran
enum class AssembleMode { Aldi, Eks, ConstDrift, ConstNoise };      // assemble_kernel's `mode`, in its order
enum class DenseRoute {
    NoiseOnly,      // hk from the drift's absmax, then the noise coefficients
    Tail,           // hk-free: one launch behind the factorisation writes the rest of the image (tail_aldi_kernel)
    Finish,         // aldi, default / spectral time step: scalars, matvecs and W in one launch (finish_aldi_kernel)
    General         // scalars, the recomputed gain, the EKS inverse, assemble_kernel
};
enum class TailArm { None, DenseSigma, Chained, Plain };      // tail_aldi_kernel<DSIG, CHAIN>
enum class SideJoin { None, Event, Polled };        // nothing in flight; ev_b; the word chol(C) stores, polled by a launch of this stream
enum class UPart {
    Side,           // the side stream formed it (centring launch in front of its factorisation)
    Center,         // a centring launch of this stream forms it
    FusedLoad       // the factorisation formed C while it loaded S_aa, the tail launch forms the rest (its self_u)
};
enum class InlineFactor { None, Image, Fp64 };      // chol(C) on this stream: into the hk-free image (and d_L unless chained), into d_L
// Everything launch_dense decides, as plain data (plan_dense); a field its route does not use holds its zero value.
struct DensePlan {
    DenseRoute route = DenseRoute::General;
    TailArm tail = TailArm::None;
    SideJoin join = SideJoin::None;
    UPart upart = UPart::Side;
    int center = 0;                   // CENTER_* parts of the centring launch of this stream, 0: none
    InlineFactor factor = InlineFactor::None;
    bool refactor = false;            // d_L is wanted and the factor at hand is in the chained image only: ensure_factor factors C again
    bool gemm_M = false;              // M = C Sigma^{-1} by GEMM (dense Sigma)
    bool spectral = false;            // lambda_max of the whitened residual covariance (spectral time step)
    bool gain_inverse = false;        // K' = C_ug (hk C_gg + Gamma)^{-1}
    bool eks_inverse = false;         // P = Sigma (Sigma + hk C)^{-1}
    AssembleMode mode = AssembleMode::Aldi;
    int ktot = 0;                     // columns of the W assemble_kernel writes, 0: it does not run
};
// The K2 of this launch for the engine as it stands.  Pure: no HIP call, no write.  below_side: stream_below_side(e, L.s),
// which a caller asks only where poll_join_open holds -- nothing else hinges on it.
DensePlan plan_dense(const Engine& e, const DenseLaunch& L, bool below_side);
// what every polled join asks besides the stream priorities: a signalling factorisation in flight, one device, two streams
bool poll_join_open(const Engine& e, hipStream_t s);
// runs a plan: no decision of its own.  The one writer of Engine::last_hkfree and, through join_side, of what Factor keeps of the join.
int launch_dense(Engine& e, const DenseLaunch& L, const DensePlan& plan);
// Kernels of the caller's stream and of the side stream may WAIT for each other inside a launch (the polled join of
// launch_dense) only when the two streams cannot share a hardware queue: HIP maps the streams of one priority level
// onto a few queues, and a waiter in front of what it waits for in one in-order queue never ends.  True when `s` has a
// strictly lower priority than the side stream (a numerically greater one).
bool stream_below_side(Engine& e, hipStream_t s);
int launch_chol_async(Engine& e, int update, const double* mom, hipStream_t s, bool ev_a_bound = false);
int ensure_factor(Engine& e, hipStream_t s);      // d_L for a host reader: re-factors C in line when it is in the chained image only
struct UpdateSrc {            // one K-segment of the update GEMM
    const void* ptr;          // (rows x J) array, or nullptr for on-device noise
    int rows;                 // real rows
    int kind;                 // 0 = memory, 1 = philox noise
    int tri;                  // 1: the W columns of this segment are lower triangular (sqrt(2hk) L)
};
struct UpdateAdd {            // an optional epilogue term  + c * ptr  (out_rows x J), c = *cp * imm, or imm when cp == nullptr
    const void* ptr = nullptr;
    const double* cp = nullptr;
    double imm = 0.0;
};
// One update launch  out = W . [segments] + bias (+ add1 + add2)  (kernels_update*.hip); call sites name the fields they use.
struct UpdateLaunch {
    int out_rows = 0;
    const void* W = nullptr;       // [rpad][ktot] row-major (update_kernel)
    const void* Wf = nullptr;      // the same W in the fragment-major order of the LDS-DMA kernels (wf_index / wd_index), or the hk-free
                                   // image Engine::d_Wq; nullptr: update_kernel only
    int ktot = 0;
    const void* bias = nullptr;    // [rpad] or nullptr
    UpdateSrc src[3] = {};
    int nsrc = 0;
    UpdateAdd add1, add2;
    void* out = nullptr;
    double* absmax_part = nullptr; // per-workgroup max |out|, or nullptr
    uint64_t step_index = 0;       // Philox counter of in-kernel noise
    bool metrics = false;          // data metrics over the K-segment metric_seg (it holds G)
    int metric_seg = 1;
    const double* hkp = nullptr;   // != nullptr: Wf is the hk-free image, segments [xi | U | G] with the triangular one first; the
    const double* s2p = nullptr;   // accumulators are scaled by *s2p / *hkp behind the first segment and the result (+ bias) by *hkp
    const unsigned long long* fault = nullptr;   // != nullptr: the launch leaves `out` untouched when *fault == fault_seq (a polled join that ran out)
    unsigned long long fault_seq = 0;
    int prof = -1;                 // profiling slot (1 = K3) or -1
};
// the K-segments of a launch, resolved once for every kernel (k-tiles of 16; every segment is padded to whole tiles)
struct UpdateSegs {
    int kt[3];        // first k-tile of each segment (0x7fffffff: absent)
    int tri_seg;      // segment with lower-triangular W columns, -1: none
    bool noise;       // a segment is drawn in-kernel
    bool al16;        // every segment read from memory is non-null and 16-byte aligned
    bool ok;          // 1 to 3 segments that add up to ktot
};
UpdateSegs update_segments(const UpdateLaunch& L);
enum class UpdateKernel {
    None,             // an hk-free image that no kernel takes
    Update4,          // update4_kernel: the chained hk-free image (K3 through the Cholesky factor)
    Update2s, Update2, Update3s, Update3,   // the LDS-DMA kernels, fp32 / fp64, small (out_rows <= 64) or tiled
    Generic           // update_kernel
};
// the kernel launch_update runs for L; cesx_apply asks it before launch_dense commits the step to the hk-free image
UpdateKernel pick_update_kernel(const Engine& e, const UpdateLaunch& L);
int launch_update(Engine& e, const UpdateLaunch& L, hipStream_t s);
int update_grid_blocks(Engine& e, int out_rows);
// the kernels behind launch_update (L checked, g = update_segments(L)); small: update2s_kernel / update3s_kernel
int launch_update2(Engine& e, const UpdateLaunch& L, const UpdateSegs& g, bool small, hipStream_t s);
int launch_update3(Engine& e, const UpdateLaunch& L, const UpdateSegs& g, bool small, hipStream_t s);
int launch_update4(Engine& e, const UpdateLaunch& L, hipStream_t s);     // the noise segment from memory
int update2_lds(const Engine& e);     // dynamic LDS of one update2_kernel / update3_kernel workgroup
int update3_lds(const Engine& e);
constexpr int U2S_MAX_KT = 12;        // update2s_kernel / update3s_kernel: ktot <= 192
constexpr int U3S_MAX_KT = 12;
// the shapes the chained form takes (decided once per problem, cesx_set_problem)
bool update4_shape_ok(const Engine& e);
// index of W[i][k] (row i of the zero-padded rpad x ktot matrix, nkt = ktot / 16) in the fragment-major
// image: for every 256-row chunk y and k-tile kt, 16 pieces (g, rb) of 64 lanes x 4 floats; lane
// (lh, li) of piece (g, rb) holds W[256 y + 32 rb + li][16 kt + 2 (4 g + v) + lh], v = 0..3
__host__ __device__ inline size_t wf_index(int i, int k, int nkt) {
    const int y = i >> 8, rb = (i >> 5) & 7, li = i & 31;
    const int kt = k >> 4, kk = k & 15, m = kk >> 1, lh = kk & 1, g = m >> 2, v = m & 3;
    return ((((size_t)y * nkt + kt) * 16 + g * 8 + rb) * 64 + lh * 32 + li) * 4 + v;
}
// ---- the "chained" coefficient image of kernels_update4.hip (K3 through the Cholesky factor) ----
// (18 + ng) tiles of 16 pieces (g, b) of 64 lanes x 4 floats.  k order inside a 16-column tile: lane (lh, m) of piece (g, b)
// holds columns 8 g + 4 lh + v, v = 0..3 -- the accumulator row order of v_mfma_f32_32x32x2_f32 (wf_index keeps 2 (4 g + v) + lh).
__host__ __device__ inline size_t wc_slot(int t, int b, int m, int kl) {          // tile t, row block b, row m of it, column kl (0..15) of the tile
    const int g = kl >> 3, lh = (kl >> 2) & 1, v = kl & 3;
    return ((((size_t)t * 16 + g * 8 + b) * 64) + lh * 32 + m) * 4 + v;
}
// L[i][j], i >= j: column block cb = j / 32 of the lower factor sits in tiles 2 (8 - cb) + h, rows b >= cb
__host__ __device__ inline size_t wc_index_L(int i, int j) {
    return wc_slot(2 * (8 - (j >> 5)) + ((j >> 4) & 1), i >> 5, i & 31, j & 15);
}
// -(L^T Sigma^{-1})[r][k] = -L[k][r] / Sigma_kk, k >= r: column block kb = k / 32 sits in tiles 2 (7 - kb) + h, rows b <= kb
__host__ __device__ inline size_t wc_index_Lt(int r, int k) {
    return wc_slot(2 * (7 - (k >> 5)) + ((k >> 4) & 1), r >> 5, r & 31, k & 15);
}
// -K[i][c]: tiles 18 + c / 16
__host__ __device__ inline size_t wc_index_K(int i, int c) {
    return wc_slot(18 + (c >> 4), i >> 5, i & 31, c & 15);
}
// index of W[i][k] in the fp64 fragment-major image read by update3_kernel: for every 256-row chunk y, k-tile kt
// and 16-row block rb two pieces (sp) of 64 lanes x 2 doubles; lane (lr, li) = 16 lr + li of piece sp holds
// W[256 y + 16 rb + li][16 kt + 4 (2 sp + e) + lr], e = 0, 1
__host__ __device__ inline size_t wd_index(int i, int k, int nkt) {
    const int y = i >> 8, rb = (i >> 4) & 15, li = i & 15;
    const int kt = k >> 4, kk = k & 15, s = kk >> 2, lr = kk & 3, sp = s >> 1, e = s & 1;
    return ((((size_t)y * nkt + kt) * 16 + rb) * 2 + sp) * 128 + (size_t)(lr * 16 + li) * 2 + e;
}
// dense Gamma: the whitened copy of G this step's kernels read (G itself when Gamma is diagonal); force: whiten again even
// when the same array was whitened last (the first moments call of a step: its contents may be new)
const void* whitened_G(Engine& e, const void* G, hipStream_t s, bool force, int* rc);
int launch_metric_final(Engine& e, const double* mom, bool publish, hipStream_t s);
MetricFin metric_fin_args(Engine& e, const double* mom, bool publish);     // (publish: takes the next sequence number; mom == nullptr: the engine's own copy d_lag)
int launch_publish(Engine& e, hipStream_t s);
int launch_absmax_final(Engine& e, int nparts, double* absmax_out, hipStream_t s);
constexpr int PNB = 32;    // leading dimensions of Cholesky factors are rounded up to this
inline int potrf_ld(int n) { return (n + PNB - 1) / PNB * PNB; }
int gram_nbw(int dtype);
int gram_tile(int dtype);
int gram_kt(int dtype);
int gram_max_stage_rows();
int launch_noise(Engine& e, uint64_t step_index, void* xi, hipStream_t s);
int launch_stage_forward(Engine& e, const void* A, const void* b, hipStream_t s);   // A, b -> d_Wfwd, d_Wfwd_f, d_bfwd
int launch_moments_lineal(Engine& e, double* mom, hipStream_t s);                   // G part of the moments from the head + the installed linear map
int launch_calibrate(Engine& e, double target_ms, double* tflops, double* clock_ghz, hipStream_t s);   // kernels_calib.hip
// the chains' state of a score launch (launch_mh_score, launch_gp_score)
inline MhChains mh_chains(const Engine& e, bool start, const double* logu, unsigned step) {
    return {e.cfg.j_offset, e.mh.phi, e.mh.cnt, logu, (unsigned)e.cfg.seed, (unsigned)(e.cfg.seed >> 32), step, start ? 1 : 0};
}
// kernels_mh.hip: phi of the states X (with their forward map G, whitened when Gamma is dense) of every chain; start: into
// Engine::mh.phi, counters cleared; otherwise the accept test of step word `step` and the masked copy X -> U
int launch_mh_score(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s);
// kernels_gp.hip: the GP means (and variances, var_out != nullptr) of the states X (p x J, engine dtype) into fp64 (gp.n x J)
int launch_gp_predict(Engine& e, const void* X, double* mean, double* var, bool nugget, hipStream_t s);
// kernels_gpgrad.hip: launch_gp_predict with the gradients of the rows with respect to x, fp64 (gp.n x p x J); var and dvar
// nullptr: the mean-only mode
int launch_gp_predict_grad(Engine& e, const void* X, double* mean, double* var, double* dmean, double* dvar, bool nugget,
                           hipStream_t s);
// kernels_gpgrad.hip: the Langevin step on the GP rows and gradients.  what 0: phi and g = S^T grad phi of the states X into
// mh.phi / mh.lv_g, counters cleared; 1: P = U + S (xi - g / 2) with the block in mh.xi; 2: the proposal X with its rows, the
// test with the Langevin correction, U := X, phi and g on the accepted columns
int launch_gp_langevin(Engine& e, int what, int mode, const void* X, const double* mean, const double* var, const double* dmean,
                       const double* dvar, void* U, void* P, const double* logu, unsigned step, hipStream_t s);
// kernels_lvlin.hip: the Langevin step on a linear map (cesx_mh_langevin_lineal_*).  launch_lvlin_score is launch_mh_score with
// the prior term whatever the proposal kind, the Langevin correction from mh.xi / mh.lin_g / mh.lin_gp in the test, and the
// masked copy of g(P) beside the one of P; launch_lvlin_z: mh.lin_z = mh.xi - mh.lin_g / 2; launch_lvlin_exph: t0 := exp(X) (.) t0
int launch_lvlin_score(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s);
int launch_lvlin_z(Engine& e, hipStream_t s);
int launch_lvlin_exph(Engine& e, const void* X, void* t0, hipStream_t s);
// kernels_hmclin.hip: the leapfrog step on a linear map (cesx_mh_hmc_lineal_*).  launch_hl_kick: begin -- r = mh.xi - (e / 2) mh.lin_g
// (unarmed: launch_lvlin_z, r in mh.lin_z) --, otherwise r -= e mh.lin_gp; armed: r in mh.lin_r and z = e r into mh.lin_z.
// launch_hl_accept: launch_lvlin_score's accept with |r - (e / 2) g_Q|^2 from the momentum block as the second norm, and alpha armed
int launch_hl_kick(Engine& e, bool begin, hipStream_t s);
int launch_hl_accept(Engine& e, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s);
// kernels_gp.hip: phi of the states X from the GP rows (mode CESX_GP_GAMMA / _VAR / _GAMMA_VAR); start: into mh.phi,
// counters cleared; otherwise the accept test of step word `step` and the masked copy X -> U
int launch_gp_score(Engine& e, int mode, bool start, const void* X, const double* mean, const double* var, void* U,
                    const double* logu, unsigned step, hipStream_t s);
// kernels_gpchain.hip: n_steps Metropolis steps of every chain on the emulator in one launch (mode CESX_GP_GAMMA / _VAR /
// _GAMMA_VAR; include/cesx.h, cesx_gp_run).  gp_run_fits: the tile's LDS need is within the workgroup budget
bool gp_run_fits(int p, int Jp, int n_gp);
int launch_gp_run(Engine& e, int mode, uint64_t step_index, int n_steps, int stride, bool nugget, void* U, void* trace,
                  const void* xi, const double* logu, hipStream_t s);
// kernels_gpdense.hip: the same for CESX_GP_DENSE -- Sigma_j = Gamma + B diag(var_j) B^T factored per chain; mean and var
// are (gpd.k x J).  gp_dense_prepare: once per installed descriptor (the kernels' dynamic LDS limit for n and k)
int gp_dense_prepare(Engine& e, int n, int k);
int launch_gp_score_dense(Engine& e, bool start, const void* X, const double* mean, const double* var, void* U,
                          const double* logu, unsigned step, hipStream_t s);
// kernels_gpproj.hip: the same for CESX_GP_PROJ -- I_k + R diag(var_j) R^T factored per chain by a sub-wave group of lanes;
// mean and var are (gpp.k x J).  gp_proj_prepare: once per installed descriptor (the kernels' dynamic LDS limit for k)
int gp_proj_prepare(Engine& e, int k);
int launch_gp_score_proj(Engine& e, bool start, const void* X, const double* mean, const double* var, void* U,
                         const double* logu, unsigned step, hipStream_t s);
// gp_proj_group: the lanes of one chain's group (16, 32 or 64) for k; gp_proj_lds: the dynamic LDS of a workgroup of either kernel
int gp_proj_group(int k);
size_t gp_proj_lds(int k);
// kernels_gpprojgrad.hip: the gradient coefficients of CESX_GP_PROJ from the rows (gpp.k x J): phid [J] the data term of phi
// (launch_gp_score_proj's bits), ca and cb [gpp.k][J] the a_t and b_t lv_score reads in mode CESX_GP_PROJ
int gp_proj_coef_prepare(Engine& e, int k);
int launch_gp_proj_coef(Engine& e, const double* mean, const double* var, double* phid, double* ca, double* cb, hipStream_t s);

// kernels_darcy.hip: G = the installed Darcy map of the columns of U (engine dtype in and out, fp64 inside); status (J int32,
// or nullptr): 0, the 1-based column of the zero pivot of a particle whose outputs are NaN, or minus the column that held a
// non-finite entry.  darcy_prepare: once per installed map (the kernels' dynamic LDS limit for this K)
int darcy_prepare(Engine& e, int K);
int launch_darcy(Engine& e, const void* U, void* G, int* status, hipStream_t s);
// kernels_darcy_grad.hip: the resident map with the gradient of the data misfit by one adjoint solve (cesx_darcy_grad): G [n][J],
// phid [J], dphi [p][J], all fp64; reads the problem's y, gw / Wh and DarcyState::gscr ([J][2 n] doubles)
size_t darcy_grad_lds_bytes(int K);
int darcy_grad_prepare(Engine& e, int K);
int launch_darcy_grad(Engine& e, const void* U, double* G, double* phid, double* dphi, int* status, hipStream_t s);
// kernels_darcy_stream.hip: the same map with the banded LU streamed through a live window in LDS and an HBM workspace
// (DarcyState::ws, one slot per workgroup in flight), for Nmesh up to darcy_stream_kmax().  darcy_stream_prepare: once per
// installed map (the dynamic LDS limit for this K; auto_grid = the workgroups the device holds at once)
int darcy_stream_kmax();
size_t darcy_stream_lds(int K);
size_t darcy_stream_slot_bytes(int K);
int darcy_stream_prepare(Engine& e, int K, int* auto_grid);
int launch_darcy_stream(Engine& e, const void* U, void* G, int* status, hipStream_t s);

// kernels_l96.hip: per column, RK45 of the installed two-scale Lorenz '96 model from W_in (n_state x J fp64) with the
// parameters the descriptor's map takes from U; G = the last window's statistics (engine dtype), W_out = the state at t[-1]
// (may be W_in), info ([4][J] int32 or nullptr) = status, accepted steps, attempted steps, 0
int launch_l96(Engine& e, const void* U, const double* W_in, void* G, double* W_out, int* info, hipStream_t s);

// kernels_l63.hip: per column, RK45 of the installed Lorenz '63 model from W_in (3 x J fp64), one particle per lane; G = the
// nine means of the last window (engine dtype), W_out = the state at t[-1] (may be W_in), info as launch_l96 writes it
int launch_l63(Engine& e, const void* U, const double* W_in, void* G, double* W_out, int* info, hipStream_t s);
// kernels_maps.hip: G = the installed closed-form map of every column of U, one column per lane (fp64, rounded on the store);
// and n_steps Metropolis steps of every chain in one launch for the installed map of a fused kind (include/cesx.h)
int launch_map_apply(Engine& e, const void* U, void* G, hipStream_t s);
int launch_mh_run_map(Engine& e, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                      const double* logu, hipStream_t s);
// kernels_maps.hip: G [n][J] and the Jacobian DG [n][p][J] of the installed map, fp64 whatever the engine dtype; and
// launch_mh_run_map under a Langevin proposal (the chains' g in mh.lv_g is read and written back)
int launch_map_jac(Engine& e, const void* U, double* G, double* DG, hipStream_t s);
int launch_mh_langevin_run_map(Engine& e, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                               const double* logu, hipStream_t s);
// kernels_hmc.hip: the leapfrog step on the rows and gradients lv_score reads (cesx_mh_hmc_* / cesx_gp_hmc_*).  what 0: r (mh.hm_r)
// and the first Q from U, the block in mh.xi and mh.lv_g; 1: phi(Q), g(Q), the full kick, Q advanced in place; 2: the last Q
// with its rows, the half kick, the test, U := Q, phi and g on the accepted columns.  kernels_maps.hip: n_steps such steps of
// `leapfrog` positions each in one launch for the installed map of a fused kind
int launch_hmc(Engine& e, int what, int mode, void* Q, const double* mean, const double* var, const double* dmean,
               const double* dvar, void* U, const double* logu, unsigned step, hipStream_t s);
int launch_mh_hmc_run_map(Engine& e, uint64_t step_index, int n_steps, int leapfrog, int stride, void* U, void* trace,
                          const void* xi, const double* logu, hipStream_t s);
// kernels_darcy_chain.hip: the same steps on a READY-MADE gradient (cesx_mh_grad_source, CESX_MH_GRAD_READY): G [n][J] and d [p][J] =
// the data term of grad phi at X (cesx_darcy_grad), one wave per chain.  what 0: phi and g of the states X into mh.phi / mh.lv_g,
// counters cleared; 1: the Langevin accept of the proposal X; 2: the leap at X = Q, advanced in place; 3: the leapfrog accept at X
int launch_darcy_chain(Engine& e, int what, const void* X, const double* G, const double* d, void* U, const double* logu,
                       unsigned step, hipStream_t s);
// kernels_adapt.hip: the step-size recursion behind an armed handle's accept (cesx_mh_adapt_*): mh.ad_alpha -> mh.ad_state, a
// row of mh.ad_hist.  While mh.ad_armed, launch_hmc launches the ADAPT instantiations, which read mh.ad_state[0]
int launch_adapt_update(Engine& e, hipStream_t s);

// kernels_chainsum.hip: the stage behind cesx_chain_summary_* (include/cesx.h); the entry points have checked the state
int chainsum_begin(Engine& e, long long n_draws);
int chainsum_add(Engine& e, const void* trace, int kept, hipStream_t s);
int chainsum_read(Engine& e, double* c, double* s1, double* cc, double* within, double* between, double* half_mean,
                  double* half_var, hipStream_t s);

// kernels_chainhist.hip: the stage behind cesx_chain_hist_* (include/cesx.h); the entry points have checked the arguments
int chainhist_begin(Engine& e, const cesx_chain_hist_desc* d, hipStream_t s);
int chainhist_add(Engine& e, const void* trace, int kept, hipStream_t s);
int chainhist_read(Engine& e, unsigned long long* hist1, unsigned long long* out1, unsigned long long* hist2,
                   unsigned long long* out2, hipStream_t s);

// kernels_chainacf.hip: the stage behind cesx_chain_acf_* (include/cesx.h); the entry points have checked the arguments and the state
int chainacf_begin(Engine& e, long long n_draws, int lags, int n_chains);
int chainacf_add(Engine& e, const void* trace, int kept, hipStream_t s);
int chainacf_read(Engine& e, double* gsum, double* msum, double* m2sum, double* chain_gamma, double* chain_mean, hipStream_t s);

// kernels_gpfit.hip: lml, gradient and status of the GPs gf.idx[0 .. n_active) at gf.theta into gf.out
int launch_gpfit_eval(Engine& e, int n_active, hipStream_t s);
int gpfit_tiles(int Jp);                            // 64 x 64 tiles of the lower triangle of a Jp x Jp matrix

// Event pair for one profiled launch (cesx_profile_*).  bound = false: the pair is RECORDED around the launch (two
// marker packets: they delay the stream by ~6 us each and the interval includes that).  bound = true: the caller
// passes a / b to hipExtLaunchKernel, which ties them to the kernel's own start / end time stamps -- the interval
// is the kernel's duration as rocprofv3 reports it, and no marker sits in front of the next launch.
struct ProfScope {
    Engine& e; int which; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; bool bound;
    ProfScope(Engine& e_, int which_, hipStream_t s_, bool bound_ = false) : e(e_), which(which_), s(s_), bound(bound_) {
        if (!e.profile || which < 0) return;
        if (e.profile_only >= 0 && which != e.profile_only) return;
        if (e.profile_gap_only && !bound) return;         // (recorded pairs are markers on the stream: not in a gap-only step)
        auto get = [&]() { hipEvent_t ev = nullptr; if (!e.prof_pool.empty()) { ev = e.prof_pool.back(); e.prof_pool.pop_back(); } else (void)hipEventCreate(&ev); return ev; };
        // gap-only: the moments launch binds its stop alone, the update launch its start alone (the other stays null)
        if (!e.profile_gap_only || which == 1) a = get();
        if (!e.profile_gap_only || which == 0) b = get();
        if (!bound) (void)hipEventRecord(a, s);
    }
    bool on() const { return a != nullptr || b != nullptr; }
    ~ProfScope() {
        if (!on()) return;
        if (!bound) (void)hipEventRecord(b, s);
        e.prof_ev[which].push_back({a, b});
        e.prof_tag[which].push_back(e.prof_step * 2 + (which == 0 ? (unsigned long long)e.prof_part : 1ull));
    }
};

// the message cesx_last_error(NULL) returns (per thread): entry points that have no handle (cesx_create, cesx_comm_unique_id)
void set_global_error(const std::string& msg);

#define CESX_HIP(call)                                                              \
    do {                                                                            \
        hipError_t _e = (call);                                                     \
        if (_e != hipSuccess) {                                                     \
            e.err = std::string(#call) + ": " + hipGetErrorString(_e);              \
            return CESX_EHIP;                                                       \
        }                                                                           \
    } while (0)

// a failed DevBuf::alloc / ensure (dev_alloc's code: the hipError_t of its allocation, or of its memset) as an entry point's error
inline int buf_fail(Engine& e, int rc) {
    e.err = std::string("device allocation: ") + hipGetErrorString((hipError_t)rc);
    return CESX_EHIP;
}
#define TRY_BUF(x) do { if (const int _b = (x)) return buf_fail(e, _b); } while (0)

// a core buffer (Engine::core owns it; freed with the engine), its pointer handed out into the engine's own field
template <typename P> int core_alloc(Engine& e, P** ptr, size_t bytes, bool zero = true) {
    DevBuf<void> b;
    TRY_BUF(b.alloc(bytes, zero));
    *ptr = static_cast<P*>(b.get());
    e.core.push_back(std::move(b));
    return CESX_OK;
}

// the argument fields every update kernel but update4_kernel shares (UpdArgs<T>, Upd2Args, Upd3Args)
template <typename T, typename A>
inline void pack_update_common(A& a, const Engine& e, const UpdateLaunch& L, const UpdateSegs& g) {
    a.out_rows = L.out_rows; a.bias = (const T*)L.bias;
    a.J = e.J;
    a.out = (T*)L.out;
    a.add1 = (const T*)L.add1.ptr; a.c1p = L.add1.cp; a.c1i = L.add1.imm;
    a.add2 = (const T*)L.add2.ptr; a.c2p = L.add2.cp; a.c2i = L.add2.imm;
    a.absmax_part = L.absmax_part;
    a.rowc = (const T*)e.d_rowc;
    a.metric_part = L.metrics ? e.d_metric_part : nullptr;
    a.metric_seg = L.metric_seg;
    a.tri_seg = g.tri_seg;
    a.fault = L.fault; a.fault_seq = L.fault_seq;
}

// One launch of an LDS-DMA update kernel (256 threads): its dynamic LDS, the grid (Engine::last_update_grid*: the partial
// results it leaves), and the profiling events bound to the kernel's own start / end; a launch with both events also has
// wave 0 of workgroup 0 store its clocks (a.clk = Engine::d_clk, cesx_profile_clock).
template <typename K, typename A>
int launch_update_bound(Engine& e, K kern, dim3 grid, int lds, A& a, int prof_which, hipStream_t s) {
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    e.last_update_grid_x = (int)grid.x;
    e.last_update_grid = (int)(grid.x * grid.y);
    {
        ProfScope prof(e, prof_which, s, true);
        a.clk = (prof.a && prof.b) ? e.d_clk : nullptr;
        if (prof.on()) hipExtLaunchKernelGGL(kern, grid, dim3(256), (unsigned)lds, s, prof.a, prof.b, 0, a);
        else hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

// One launch of a Gram kernel over the workgroups of the part's plan (gram_kernel and gram2_kernel take the same arguments).
// bound: the profiling events are tied to the kernel's own start / end (ProfScope); otherwise they are recorded around it.
template <typename T, typename K>
int launch_gram_kernel(Engine& e, const GramLaunch& L, K kern, int threads, int lds, bool bound) {
    GramPart& gp = e.gram[L.part];
    const dim3 grid(gp.plan.total_wgs), block(threads);
    CESX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    {
        ProfScope prof(e, (e.profile_gap_only && L.part == 0) ? -1 : 0, L.s, bound);      // (gap-only: the second launch's stop, nothing else)
        auto launch = [&](auto... args) {
            if (bound && prof.on()) hipExtLaunchKernelGGL(kern, grid, block, (unsigned)lds, L.s, prof.a, prof.b, 0, args...);
            else hipLaunchKernelGGL(kern, grid, block, lds, L.s, args...);
        };
        launch((const T*)L.U, (const T*)L.G, (const T*)e.d_shiftT, e.p, e.n, (long long)e.J, (const int*)gp.d_type_hdr, gp.plan.ntypes,
               (const int*)gp.d_rows, (const int*)gp.d_wblk, (T*)gp.d_slabs, gp.d_rowsum_part);
    }
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

}  // namespace cesx
