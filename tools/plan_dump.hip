// dev tool (host only, runs without a GPU): the Gram work partition of a shape, and the K2 plan of an engine state.
//   plan_dump p n J f64(0|1) [workgroup budget of the second launch]
//       types, staged block rows, slices, the row traffic the plan implies and the busiest SIMD against the mean
//   plan_dump engine p n J f64(0|1) [shards] [CUs]
//       both parts as an engine of that shape plans them (plan_gram_parts: the budgets of `CUs` compute units -- 256 --, the
//       slim or the blocked factorisation beside the second launch, J the local share of `shards` x J, the re-plan): the
//       totals and every integer of the five device tables.  Two trees that print the same plan the same sums.
//   plan_dump dense f0 .. f22 | plan_dump dense bench | plan_dump dense sweep      [CESX_LIB=path of libcesx.so]
//       the K2 plan (plan_dense through cesx_debug_dense_plan, include/cesx.h: 23 facts -> 13 fields) of one vector of facts,
//       by name; of the benchmark's engine state under the 16 valid (update, phase, time step) combinations; of the sweep of
//       tests/test_dense_plans_host.py, one line `facts : plan` per case (the input of tools/make_golden_dense_plans.py)
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tools/plan_dump tools/plan_dump.hip -ldl
#include "../ces_amd/csrc/kernels_gram.hip"
#include "../ces_amd/csrc/kernels_gram2.hip"
#include <cstdio>
#include <dlfcn.h>
using namespace cesx;
namespace cesx {      // devbuf.h's seam: this tool has no device and never allocates (gram_part_alloc is linked in, not called)
int dev_alloc(void**, size_t, bool) { return 1; }
void dev_free(void*) {}
}
#ifndef DENSE_PLAN_FN      // (a tree without the export: a stand-in of this signature, defined in front of this file)
static int dense_plan_fn(const int32_t* facts, int32_t* plan) {
    static int (*fn)(const int32_t*, int32_t*) = nullptr;
    if (!fn) {
        void* lib = dlopen(getenv("CESX_LIB") ? getenv("CESX_LIB") : "ces_amd/libcesx.so", RTLD_NOW);
        if (lib) fn = (int (*)(const int32_t*, int32_t*))dlsym(lib, "cesx_debug_dense_plan");
        if (!fn) { fprintf(stderr, "plan_dump dense: no cesx_debug_dense_plan (CESX_LIB, or run from the repository root)\n"); exit(2); }
    }
    return fn(facts, plan);
}
#endif
namespace dense {
constexpr int NF = 23, NP = 13;
enum Fact { UPDATE, TIME_STEP, PHASE, UPD_OK, F64, P_SLIM, DIAG_SIGMA, CHAIN, HKFREE_OK, UPDATE_V2, HAS_WQ, INFLIGHT, FUSED_CENTER,
            IMG, SIGNALS, IMAGE_ONLY, POLL_JOIN_OK, SHARDED, ON_SIDE, BELOW_SIDE, FUSE_OK, FUSE_AUTO, GRAM_B_SHORT };
// the 16 valid (update, phase, time step) combinations: eks / aldi as a step, aldi_constant as drift and noise
static const int COMBOS[4][2] = {{0, 0}, {1, 0}, {2, 1}, {2, 2}}, TIME_STEPS[4] = {0, 1, 2, 4};
// the ten booleans the routes branch on directly, bit i of the case number
static const int FACTORIAL[10] = {INFLIGHT, FUSED_CENTER, IMG, SIGNALS, IMAGE_ONLY, POLL_JOIN_OK, SHARDED, ON_SIDE, BELOW_SIDE, UPD_OK};
// single switches away from the base state, over the five booleans they meet (bit i of the case number)
static const int SWITCHES[6] = {HKFREE_OK, UPDATE_V2, HAS_WQ, FUSE_OK, FUSE_AUTO, GRAM_B_SHORT};
static const int SWITCH_OVER[5] = {INFLIGHT, FUSED_CENTER, IMG, IMAGE_ONLY, UPD_OK};
static void base(int32_t* f) {      // everything allowed, nothing in flight, no switch given
    for (int i = 0; i < NF; ++i) f[i] = 0;
    f[P_SLIM] = f[DIAG_SIGMA] = f[CHAIN] = f[HKFREE_OK] = f[UPDATE_V2] = f[HAS_WQ] = f[SIGNALS] = f[POLL_JOIN_OK] = f[BELOW_SIDE] = f[FUSE_AUTO] = 1;
}
static void line(const int32_t* f) {
    int32_t pl[NP];
    if (dense_plan_fn(f, pl) != 0) { fprintf(stderr, "plan_dump dense: bad facts\n"); exit(2); }
    for (int i = 0; i < NF; ++i) printf("%d ", f[i]);
    printf(":");
    for (int i = 0; i < NP; ++i) printf(" %d", pl[i]);
    printf("\n");
}
static void named(const int32_t* f) {
    static const char* const UPD[] = {"eks", "aldi", "aldi_constant"}, * const TS[] = {"default", "spectral", "constant", "adaptive", "mix"},
        * const PH[] = {"step", "drift", "noise"}, * const ROUTE[] = {"NoiseOnly", "Tail", "Finish", "General"},
        * const TAIL[] = {"-", "DenseSigma", "Chained", "Plain"}, * const JOIN[] = {"None", "Event", "Polled"},
        * const UP[] = {"Side", "Center", "FusedLoad"}, * const FAC[] = {"None", "Image", "Fp64"},
        * const MODE[] = {"Aldi", "Eks", "ConstDrift", "ConstNoise"};
    int32_t pl[NP];
    if (dense_plan_fn(f, pl) != 0) { fprintf(stderr, "plan_dump dense: bad facts\n"); exit(2); }
    printf("%s/%s/%s: route %s tail %s join %s upart %s center %d factor %s refactor %d gemm_M %d spectral %d gain_inverse %d "
           "eks_inverse %d mode %s ktot %d\n", UPD[f[UPDATE]], PH[f[PHASE]], TS[f[TIME_STEP]], ROUTE[pl[0]], TAIL[pl[1]], JOIN[pl[2]],
           UP[pl[3]], pl[4], FAC[pl[5]], pl[6], pl[7], pl[8], pl[9], pl[10], MODE[pl[11]], pl[12]);
}
// the benchmark's engine in its steady state: fp32, p = 256, diagonal Sigma, chained; chol(C) in flight on the side stream with its
// own centring launch, L into the image for aldi, d_L left out when the step before was a tail step (the same rule repeated)
static void bench_state(int32_t* f, int c, int t) {
    base(f);
    f[UPDATE] = COMBOS[c][0]; f[PHASE] = COMBOS[c][1]; f[TIME_STEP] = TIME_STEPS[t];
    f[UPD_OK] = 1;
    f[INFLIGHT] = f[PHASE] != 2;      // (the drift launch joined it)
    f[IMG] = f[UPDATE] == 1;
    f[IMAGE_ONLY] = f[IMG] && f[TIME_STEP] == 0;
}
static int run(int argc, char** argv) {
    int32_t f[NF];
    if (argc == 3 && !strcmp(argv[2], "bench")) {
        for (int c = 0; c < 4; ++c)
            for (int t = 0; t < 4; ++t) { bench_state(f, c, t); named(f); }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[2], "sweep")) {
        // 256 groups (combination, time step, dtype, diag_sigma, chain, p class) of 1024 cases, then the six switches over the groups
        for (int sw = -1; sw < 6; ++sw)
            for (int g = 0; g < 256; ++g) {
                base(f);
                f[UPDATE] = COMBOS[g >> 6][0]; f[PHASE] = COMBOS[g >> 6][1]; f[TIME_STEP] = TIME_STEPS[(g >> 4) & 3];
                f[F64] = (g >> 3) & 1; f[DIAG_SIGMA] = (g >> 2) & 1; f[CHAIN] = (g >> 1) & 1; f[P_SLIM] = g & 1;
                if (sw >= 0) f[SWITCHES[sw]] ^= 1;
                for (int k = 0; k < (sw < 0 ? 1024 : 32); ++k) {
                    for (int b = 0; b < (sw < 0 ? 10 : 5); ++b) f[sw < 0 ? FACTORIAL[b] : SWITCH_OVER[b]] = (k >> b) & 1;
                    line(f);
                }
            }
        return 0;
    }
    if (argc != 2 + NF) return 2;
    for (int i = 0; i < NF; ++i) f[i] = atoi(argv[2 + i]);
    named(f);
    return 0;
}
}  // namespace dense
static void table(const char* name, const std::vector<int>& v) {
    printf("  %s[%zu]:", name, v.size());
    for (int q : v) printf(" %d", q);
    printf("\n");
}
static int dump_engine(int argc, char** argv) {
    if (argc < 6) return 2;
    Engine e;
    e.p = atoi(argv[2]); e.n = atoi(argv[3]); e.P = e.p + e.n; e.J = atoll(argv[4]);
    e.cfg.dtype = atoi(argv[5]) ? CESX_F64 : CESX_F32;
    e.esz = e.cfg.dtype == CESX_F32 ? 4 : 8;
    e.Jg = e.J * (argc > 6 ? atoi(argv[6]) : 1);
    e.num_cus = argc > 7 ? atoi(argv[7]) : 256;
    const int rc = plan_gram_parts(e);
    printf("engine p %d n %d J %lld Jg %lld f64 %d cus %d: rc %d center_u_wgs %d gram_b_short %d\n", e.p, e.n, (long long)e.J,
           (long long)e.Jg, e.cfg.dtype == CESX_F64, e.num_cus, rc, e.center_u_wgs, (int)e.gram_b_short);
    for (int part = 0; part < 2; ++part) {
        const GramPlan& pl = e.gram[part].plan;
        printf(" part %d: tile %d nbr %d nblocks %d ntypes %d max_rb %d nbw %d wgs %d slabs %d rs %d own [%d, %d)\n", part, pl.tile,
               pl.nbr, pl.nblocks, pl.ntypes, pl.max_rb, pl.nbw, pl.total_wgs, pl.total_slabs, pl.total_rs, pl.own_lo, pl.own_hi);
        table("type_hdr", pl.type_hdr); table("rows", pl.rows); table("wblk", pl.wblk); table("blk_rc", pl.blk_rc);
        table("row_own", pl.row_own);
    }
    return rc;
}
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "engine")) return dump_engine(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "dense")) return dense::run(argc, argv);
    if (argc < 5) return 2;
    int p = atoi(argv[1]), n = atoi(argv[2]); long long J = atoll(argv[3]); int f64 = atoi(argv[4]); int budget_b = argc > 5 ? atoi(argv[5]) : 248;
    int tile = f64 ? 16 : 32, nbw = f64 ? 8 : 4, kt = f64 ? 16 : 32, esz = f64 ? 8 : 4;
    int P = p + n, pbU = (p + tile - 1) / tile;
    for (int part = 0; part < 2; ++part) {
        GramPlan pl = make_gram_plan(P, tile, nbw, MAX_STAGE_ROWS, part + 1, pbU, 1, part == 0 ? 256 : budget_b, J / kt);
        double traffic = 0, slabs = 0; long long worst = 0, sum = 0;
        printf("part %d: %d types, %d wgs, %d blocks, max_rb %d\n", part, pl.ntypes, pl.total_wgs, pl.nblocks, pl.max_rb);
        for (int t = 0; t < pl.ntypes; ++t) {
            const int* h = &pl.type_hdr[t * 8];
            printf("  type %2d: nrb %2d blocks %3d slices %3d  (blocks/rowblock %.2f)\n", t, h[0], h[3], h[5], (double)h[3] / h[0]);
            traffic += (double)h[0] * tile * J * esz;
            { long long nt_ = J / kt, tps = (nt_ + h[5] - 1) / h[5]; int mxs = (h[3] + 15) / 16 * 4; /* approx per-SIMD blocks */
              int per_simd = (h[3] + 3) / 4; worst = std::max(worst, tps * per_simd); sum += (long long)h[3] * nt_; (void)mxs; }
            slabs += (double)h[5] * h[3] * tile * tile * esz;
        }
        printf("  busiest SIMD %lld block-tiles, mean %.0f (per SIMD over %d WGs) -> efficiency %.3f\n", worst, (double)sum / 4 / pl.total_wgs, pl.total_wgs, (double)sum / 4 / pl.total_wgs / worst);
        printf("  row traffic %.1f MB (algorithmic %.1f MB), slabs %.1f MB\n", traffic / 1e6, (double)P * J * esz / 1e6, slabs / 1e6);
    }
}
