// dev tool (host only, runs without a GPU): the Gram work partition of a shape.
//   plan_dump p n J f64(0|1) [workgroup budget of the second launch]
//       types, staged block rows, slices, the row traffic the plan implies and the busiest SIMD against the mean
//   plan_dump engine p n J f64(0|1) [shards] [CUs]
//       both parts as an engine of that shape plans them (plan_gram_parts: the budgets of `CUs` compute units -- 256 --, the
//       slim or the blocked factorisation beside the second launch, J the local share of `shards` x J, the re-plan): the
//       totals and every integer of the five device tables.  Two trees that print the same plan the same sums.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tools/plan_dump tools/plan_dump.hip
#include "../ces_amd/csrc/kernels_gram.hip"
#include "../ces_amd/csrc/kernels_gram2.hip"
#include <cstdio>
using namespace cesx;
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
        const GramPlan& pl = e.gp[part].plan;
        printf(" part %d: tile %d nbr %d nblocks %d ntypes %d max_rb %d nbw %d wgs %d slabs %d rs %d own [%d, %d)\n", part, pl.tile,
               pl.nbr, pl.nblocks, pl.ntypes, pl.max_rb, pl.nbw, pl.total_wgs, pl.total_slabs, pl.total_rs, pl.own_lo, pl.own_hi);
        table("type_hdr", pl.type_hdr); table("rows", pl.rows); table("wblk", pl.wblk); table("blk_rc", pl.blk_rc);
        table("row_own", pl.row_own);
    }
    return rc;
}
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "engine")) return dump_engine(argc, argv);
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
