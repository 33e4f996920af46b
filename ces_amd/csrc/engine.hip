// C ABI of libcesx.so (include/cesx.h): handle lifetime, problem set-up and
// the host-side sequencing of K1 (moments) -> K2 (dense) -> K3 (update).
#include "cesx_internal.h"
#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <sched.h>
#include <stdexcept>
#include <thread>

using namespace cesx;

namespace {

thread_local std::string g_create_err;      // per-thread: cesx_create has no handle to hang the message on

// ---- tiny host-side dense helpers (set-up only: Gamma and Sigma are factorised once) ----
bool host_chol(int n, const double* A, std::vector<double>& L) {
    L.assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0)) return false;
        const double ljj = std::sqrt(d);
        L[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = s / ljj;
        }
    }
    return true;
}
void host_tri_inverse(int n, const std::vector<double>& L, std::vector<double>& Li) {
    Li.assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= L[(size_t)i * n + k] * Li[(size_t)k * n + j];
            Li[(size_t)i * n + j] = s / L[(size_t)i * n + i];
        }
}
// Ainv = Li^T Li
void host_spd_inverse(int n, const std::vector<double>& Li, std::vector<double>& Ainv) {
    Ainv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = i; k < n; ++k) s += Li[(size_t)k * n + i] * Li[(size_t)k * n + j];
            Ainv[(size_t)i * n + j] = Ainv[(size_t)j * n + i] = s;
        }
}
bool is_diagonal(int n, const double* A) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (i != j && A[(size_t)i * n + j] != 0.0) return false;
    return true;
}

int upload(Engine& e, void* dst, const void* src, size_t bytes) {
    CESX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return CESX_OK;
}
// fp64 host vector -> engine dtype on device
int upload_T(Engine& e, void* dst, const double* src, size_t len) {
    if (e.cfg.dtype == CESX_F64) return upload(e, dst, src, len * 8);
    std::vector<float> tmp(len);
    for (size_t i = 0; i < len; ++i) tmp[i] = (float)src[i];
    return upload(e, dst, tmp.data(), len * 4);
}

#define TRY(x) do { int _rc = (x); if (_rc != CESX_OK) return _rc; } while (0)

// Every entry point runs on the engine's device and gives the calling thread its own device
// back on return (a process may hold engines on several devices; cesx_destroy runs from GC).
struct DeviceGuard {
    int prev = -1, dev;
    hipError_t st = hipSuccess;
    explicit DeviceGuard(int device) : dev(device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) st = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};
#define SET_DEVICE(e)                                                               \
    DeviceGuard _dg((e).cfg.device);                                                \
    if (_dg.st != hipSuccess) {                                                     \
        (e).err = std::string("hipSetDevice: ") + hipGetErrorString(_dg.st);        \
        return CESX_EHIP;                                                           \
    }

int check_prm(Engine& e, const cesx_step_params* prm) {
    if (!prm || prm->struct_bytes != sizeof(cesx_step_params)) { e.err = "bad cesx_step_params"; return CESX_EINVAL; }
    if (prm->update < 0 || prm->update > 2) { e.err = "unknown update rule"; return CESX_EINVAL; }
    if (prm->update != CESX_UPDATE_ALDI_CONSTANT) {
        if (prm->time_step == CESX_TS_ADAPTIVE) {
            e.err = "time_step='adaptive' needs LM_procedure, which the reference never defines (ces/calibrate.py:255)";
            return CESX_EUNSUPPORTED;
        }
        if (prm->time_step < 0 || prm->time_step > 4) { e.err = "unknown time_step rule"; return CESX_EINVAL; }
    }
    if (!e.problem_set) { e.err = "cesx_set_problem has not been called"; return CESX_ESTATE; }
    return CESX_OK;
}

int finish_step(Engine& e, const cesx_step_params& prm) {
    e.pending = true;
    e.last_prm = prm;
    return CESX_OK;
}

// the buffer of cesx_prefetch_noise that holds this step's noise block (-1: none)
int prefetched_block(const Engine& e, uint64_t step_index) {
    for (int b = 0; b < 2; ++b)
        if (e.d_xi[b] && e.xi_step[b] == (long long)step_index) return b;
    return -1;
}

// the noise block of this step drawn ahead by cesx_prefetch_noise (nullptr: draw inside the update kernel)
const void* prefetched_noise(Engine& e, const cesx_step_params& prm, hipStream_t s) {
    // drawn on the side stream behind chol(C); its own event, waited for HERE (right before the update kernel):
    // K2's scalar and assemble kernels do not need the block and run beside the draw
    const int b = prefetched_block(e, prm.step_index);
    if (b < 0) return nullptr;
    // a block drawn behind an EARLIER chol(C) precedes this step's chol(C) on the side stream: a stream that has
    // waited for this step's ev_b is already ordered behind the draw
    const bool ordered = e.xi_seq[b] < e.fac.waited_seq && s == e.fac.waited_stream;
    if (!ordered && hipStreamWaitEvent(s, e.ev_x[b], 0) != hipSuccess) return nullptr;
    return e.d_xi[b];
}

// the update launch of an eks / aldi step: W [U; G; xi] + b, or (hkfree) the coefficient image without the time step
// (launch_dense): [L | a I - M + I/hk | -K] against [xi; U; G] -- through the Cholesky factor where it is the chained one
UpdateLaunch main_update(Engine& e, const cesx_step_params& prm, const void* U, const void* G, const void* xi, void* Unext,
                         bool hkfree) {
    const UpdateSrc su{U, e.p, 0, 0}, sg{G, e.n, 0, 0}, sx{xi, e.p, xi ? 0 : 1, 1};
    UpdateLaunch L{.out_rows = e.p, .W = e.d_W, .Wf = e.d_Wf, .ktot = e.ktot, .bias = e.d_bias, .src = {su, sg, sx}, .nsrc = 3,
                   .out = Unext, .step_index = prm.step_index, .metrics = true, .prof = 1};
    if (e.fac.polled) { L.fault = e.d_cholflag + 1; L.fault_seq = e.fac.seq; }
    if (hkfree) {
        L.Wf = e.d_Wq;
        L.src[0] = sx; L.src[1] = su; L.src[2] = sg;
        L.metric_seg = 2;
        L.hkp = &e.d_scal->hk;
        L.s2p = &e.d_scal->sqrt2hk;
    }
    return L;
}

int run_update_main(Engine& e, const cesx_step_params& prm, const void* U, const void* G, const void* xi,
                    void* Unext, hipStream_t s) {
    if (!xi) xi = prefetched_noise(e, prm, s);
    const int rc = launch_update(e, main_update(e, prm, U, G, xi, Unext, e.last_hkfree), s);
    e.last_metric_parts = e.last_update_grid_x;
    return rc;
}

}  // namespace
namespace cesx {
void set_global_error(const std::string& msg) { try { g_create_err = msg; } catch (...) {} }

// devbuf.h over HIP: the engine allocates and frees device memory here and nowhere else (kernels_calib.hip: the scratch of its one call)
int dev_alloc(void** p, size_t bytes, bool zero) {
    const size_t len = bytes ? bytes : 8;
    hipError_t st = hipMalloc(p, len);
    if (st != hipSuccess) { *p = nullptr; return (int)st; }
    if (zero && (st = hipMemset(*p, 0, len)) != hipSuccess) { (void)hipFree(*p); *p = nullptr; return (int)st; }
    return 0;
}
void dev_free(void* p) { (void)hipFree(p); }

const void* whitened_G(Engine& e, const void* G, hipStream_t s, bool force, int* rc) {
    *rc = CESX_OK;
    if (!e.whiten) return G;
    // (reused only inside the step that whitened it: the same array, the same stream, no cesx_moments* call since)
    if (!force && e.gw_src == G && e.gw_stream == s && e.gw_calls == e.moments_calls) return e.d_Gw;
    // G~ = L_Gamma^{-1} G: one K segment with lower-triangular coefficients (the kernel skips the zero blocks), no bias
    *rc = launch_update(e, UpdateLaunch{.out_rows = e.n, .W = e.d_Wwh, .Wf = e.d_Wwh_f, .ktot = e.kn, .src = {{G, e.n, 0, 1}}, .nsrc = 1,
                                        .out = e.d_Gw}, s);
    if (*rc != CESX_OK) return nullptr;
    e.gw_src = G; e.gw_stream = s; e.gw_calls = e.moments_calls;
    return e.d_Gw;
}
}  // namespace cesx
namespace {
// the deferred metric finalisation + publication of the last update (Engine::met_deferred), as a kernel of its own
int flush_metrics(Engine& e) {
    if (!e.met_deferred) return CESX_OK;
    e.met_deferred = false;
    return launch_metric_final(e, nullptr, true, e.met_stream);
}
#define FLUSH(e) TRY(flush_metrics(e))
// dense Gamma: from here on G is the engine's whitened copy of the caller's array (whitened_G)
#define WHITEN(e, G, stream, force) do { int _wrc; G = whitened_G(e, G, (hipStream_t)(stream), force, &_wrc); if (_wrc != CESX_OK) return _wrc; } while (0)
// (the U x U launch reads G rows only when p is not a multiple of the MFMA tile: whiten there only then)
#define WHITEN_UU(e, G, stream) do { if ((e).whiten && (e).p % gram_tile((e).cfg.dtype) != 0) WHITEN(e, G, stream, true); } while (0)

}  // namespace

extern "C" {

int cesx_abi_version(void) { return CESX_ABI_VERSION; }

const char* cesx_last_error(cesx_handle h) {
    if (!h) return g_create_err.c_str();
    return reinterpret_cast<Engine*>(h)->err.c_str();
}

// The side stream carries the one-workgroup Cholesky beside the second Gram launch.  It is a
// HIGH-PRIORITY stream: HIP multiplexes the streams of a priority level onto a few hardware
// queues (4 by default), and once a communicator library has created its own streams the side
// stream would share a queue with the caller's stream -- two streams on one queue run one after
// the other.  Priority levels have their own queues.
static hipError_t create_side_stream(Engine& e) {
    int lo = 0, hi = 0;
    const bool prio = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi < lo;
    if (prio && hipStreamCreateWithPriority(&e.side, hipStreamNonBlocking, hi) == hipSuccess) {
        e.side_prio = hi; e.side_has_prio = true;
        return hipSuccess;
    }
    return hipStreamCreateWithFlags(&e.side, hipStreamNonBlocking);
}

static int create_impl(const cesx_config* cfg, cesx_handle* out) {
    if (out) *out = nullptr;
    if (!cfg || !out || cfg->struct_bytes != sizeof(cesx_config)) { g_create_err = "bad cesx_config"; return CESX_EINVAL; }
    if (cfg->p < 1 || cfg->n_obs < 1 || cfg->J_local < 1 || cfg->J_global < cfg->J_local || cfg->j_offset < 0 ||
        (cfg->dtype != CESX_F32 && cfg->dtype != CESX_F64)) {
        g_create_err = "cesx_create: invalid shape or dtype";
        return CESX_EINVAL;
    }
    if (cfg->p > 16384 || cfg->n_obs > 16384) {     // K2 is dense in (p + n)^2 and indexes it with 32 bits
        g_create_err = "cesx_create: p and n_obs are limited to 16384";
        return CESX_EINVAL;
    }
    Engine* ep = new (std::nothrow) Engine();
    if (!ep) { g_create_err = "out of host memory"; return CESX_EINVAL; }
    Engine& e = *ep;
    e.cfg = *cfg;
    e.p = cfg->p; e.n = cfg->n_obs; e.P = e.p + e.n;
    e.J = cfg->J_local; e.Jg = cfg->J_global;
    e.esz = cfg->dtype == CESX_F32 ? 4 : 8;
    if (const char* ov = std::getenv("CESX_OVERLAP")) e.overlap_chol = ov[0] != '0';
    if (const char* uv = std::getenv("CESX_UPDATE_V1")) e.update_v2 = uv[0] == '0';
    if (const char* gv = std::getenv("CESX_GRAM_V1")) e.gram_v2 = gv[0] == '0';
    if (const char* fv = std::getenv("CESX_FUSE_CENTER")) { e.fuse_center_ok = fv[0] != '0'; e.fuse_center_auto = false; }
    if (const char* pv = std::getenv("CESX_POLL_JOIN")) e.poll_join_ok = pv[0] != '0';
    if (const char* hv = std::getenv("CESX_HKFREE")) e.hkfree_ok = hv[0] != '0';
    if (const char* cv = std::getenv("CESX_CHAIN")) e.chain_ok = cv[0] != '0';
    if (const char* sv = std::getenv("CESX_UPDATE_SMALL")) e.update_small = sv[0] != '0';
    if (const char* dv = std::getenv("CESX_TEST_DROP_CHOL_SIGNAL")) e.test_drop_signal_at = (unsigned long long)std::max(0, std::atoi(dv));
    if (const char* tv = std::getenv("CESX_POLL_TIMEOUT_MS")) e.poll_ticks = (unsigned long long)std::max(1, std::atoi(tv)) * 100000ull;
    auto fail = [&](int rc) { g_create_err = e.err; cesx_destroy(reinterpret_cast<cesx_handle>(ep)); return rc; };
    int rc;
    DeviceGuard dg(cfg->device);
    if (dg.st != hipSuccess) { e.err = std::string("hipSetDevice: ") + hipGetErrorString(dg.st); return fail(CESX_EHIP); }
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && ncu > 0) e.num_cus = ncu;
    }
    const int p = e.p, n = e.n, P = e.P, mx = p > n ? p : n;
    const size_t pp = (size_t)p * p, pn = (size_t)p * n, nn = (size_t)n * n;
    const size_t mm = (size_t)potrf_ld(mx) * potrf_ld(mx);     // temporaries also hold padded Cholesky factors

    e.ml = MomLayout{p, n};
    if ((rc = plan_gram_parts(e))) return fail(rc);      // (kernels_gram.hip)
    e.colsum_slices = (int)std::min<long long>(16, (e.J + 1023) / 1024);
    if (e.colsum_slices < 1) e.colsum_slices = 1;
    e.kp = (p + 15) / 16 * 16; e.kn = (n + 15) / 16 * 16; e.ktot = 2 * e.kp + e.kn;
    e.rpad = (mx + 255) / 256 * 256;
    e.mom_len = e.ml.len();                      // incl. lagged {sum q_r^2, sum q_e^2} of the previous apply

#define DM(ptr, bytes) if ((rc = core_alloc(e, &ptr, (bytes)))) return fail(rc)
    DM(e.d_y, n * 8); DM(e.d_mu, p * 8); DM(e.d_ustar, p * 8);
    DM(e.d_Gamma, nn * 8); DM(e.d_gw, n * 8); DM(e.d_Wh, nn * 8);
    DM(e.d_Sigma, pp * 8); DM(e.d_Sinv, pp * 8); DM(e.d_sw, p * 8);
    DM(e.d_shift64, P * 8);
    DM(e.d_shiftT, P * e.esz); DM(e.d_yT, n * e.esz); DM(e.d_gwT, n * e.esz);
    DM(e.d_rowc, (size_t)e.kn * 4 * e.esz);
    DM(e.d_W, (size_t)e.rpad * e.ktot * e.esz); DM(e.d_Wf, (size_t)e.rpad * e.ktot * e.esz);
    DM(e.d_bias, (size_t)e.rpad * e.esz);
    if (cfg->dtype == CESX_F32)          // (the chained layout of kernels_update4.hip: 18 + kn / 16 tiles of 16 KiB)
        DM(e.d_Wq, std::max((size_t)e.rpad * e.ktot * 4, (size_t)(18 + e.kn / 16) * 16384));
    DM(e.d_Wfwd, (size_t)e.rpad * e.kp * e.esz); DM(e.d_Wfwd_f, (size_t)e.rpad * e.kp * e.esz);
    DM(e.d_bfwd, (size_t)e.rpad * e.esz);
    for (GramPart& gp : e.gram)
        if ((rc = gram_part_alloc(e, gp))) return fail(rc);
    DM(e.d_metric_part, ((size_t)((e.J + 31) / 32) + 8) * 2 * 8);
    DM(e.d_metric_sums, 2 * 8);
    DM(e.d_colsum_part, (size_t)P * e.colsum_slices * 8);
    DM(e.d_mom, e.mom_len * 8); DM(e.d_sums, (1 + P) * 8); DM(e.d_sums_w, (1 + P) * 8);
    DM(e.d_ubar, p * 8); DM(e.d_gbar, n * 8); DM(e.d_m, n * 8); DM(e.d_dg, n * 8);
    DM(e.d_C, pp * 8); DM(e.d_L, (size_t)potrf_ld(p) * potrf_ld(p) * 8); DM(e.d_Cug, pn * 8); DM(e.d_See, nn * 8); DM(e.d_Srr, nn * 8);
    DM(e.d_K, pn * 8); DM(e.d_Kp, pn * 8); DM(e.d_M, pp * 8); DM(e.d_P, pp * 8); DM(e.d_PK, pn * 8);
    if (potrf_ld(mx) > 256) DM(e.d_Lwork, (size_t)potrf_ld(mx) * potrf_ld(mx) * 8);
    DM(e.d_t1, mm * 8); DM(e.d_t2, mm * 8); DM(e.d_t3, mm * 8); DM(e.d_t4, mm * 8);
    if (potrf_ld(mx) <= 256) {          // warm-started SPD inverses (kernels_dense.hip, spd_inverse); zeroed: X_prev = 0 is a cold start
        if (const char* nv = std::getenv("CESX_NS_WARM")) e.ns_ok = nv[0] != '0';
        const size_t nb16 = ((size_t)mx + 15) / 16;
        for (int k = 0; k < 2; ++k) { DM(e.d_ns_x[0][k], nn * 8); DM(e.d_ns_x[1][k], pp * 8); }
        for (int k = 0; k < 3; ++k) DM(e.d_ns_r[k], (size_t)mx * mx * 8);
        DM(e.d_ns_parts, 2 * nb16 * nb16 * 8);
        DM(e.d_ns_skip, 64);
    }
    {   // spectral rule (kernels_dense.hip, spec_square_kernel): {log accumulator, weight, flag, pad} + 2 x per-workgroup partial sums
        const size_t nb16 = ((size_t)n + 15) / 16;
        DM(e.d_spec, (4 + 2 * nb16 * nb16) * 8);
    }
    DM(e.d_mv, (size_t)6 * mx * 8); DM(e.d_part, 256 * 4 * 8);
    DM(e.d_scal, sizeof(Scalars)); DM(e.d_absmax, 8);
    DM(e.d_absmax_part, (size_t)update_grid_blocks(e, p) * 8);
    DM(e.d_clk, 4 * 8);
    DM(e.d_cholflag, 128);
    DM(e.d_ticket, 64);
    DM(e.d_lag, 3 * 8);
    DM(e.d_A64, (size_t)n * p * 8); DM(e.d_b64, n * 8); DM(e.d_lvec, 2 * n * 8);
#undef DM
    if (hipHostMalloc(reinterpret_cast<void**>(&e.h_scal), sizeof(Scalars), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&e.h_scal_dev), e.h_scal, 0) != hipSuccess ||
        hipEventCreateWithFlags(&e.ev_a, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e.ev_b, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e.ev_x[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e.ev_x[1], hipEventDisableTiming) != hipSuccess ||
        create_side_stream(e) != hipSuccess) {
        e.err = "pinned host buffer / event creation failed";
        return fail(CESX_EHIP);
    }
    std::memset(e.h_scal, 0, sizeof(Scalars));
    *out = reinterpret_cast<cesx_handle>(ep);
    return CESX_OK;
}

int cesx_create(const cesx_config* cfg, cesx_handle* out) {
    // no C++ exception may cross the C boundary (std::vector growth in the Gram plan, std::string)
    try {
        return create_impl(cfg, out);
    } catch (const std::exception& ex) {
        try { g_create_err = std::string("cesx_create: ") + ex.what(); } catch (...) {}
    } catch (...) {
        try { g_create_err = "cesx_create: unknown C++ exception"; } catch (...) {}
    }
    if (out) *out = nullptr;      // (a half-built engine is leaked rather than destroyed twice)
    return CESX_EINVAL;
}

void cesx_destroy(cesx_handle h) {
    if (!h) return;
    Engine& e = *reinterpret_cast<Engine*>(h);
    DeviceGuard dg(e.cfg.device);
    for (int w = 0; w < 2; ++w)
        for (auto& pr : e.prof_ev[w]) { if (pr.first) (void)hipEventDestroy(pr.first); if (pr.second) (void)hipEventDestroy(pr.second); }
    for (auto ev : e.prof_pool) (void)hipEventDestroy(ev);
    if (e.h_scal) (void)hipHostFree(e.h_scal);
    if (e.ev_a) (void)hipEventDestroy(e.ev_a);
    if (e.ev_b) (void)hipEventDestroy(e.ev_b);
    for (hipEvent_t ev : {e.ev_x[0], e.ev_x[1]})
        if (ev) (void)hipEventDestroy(ev);
    if (e.side) (void)hipStreamDestroy(e.side);
    if (e.comm) (void)cesx_comm_destroy(h);
    delete &e;      // (the device memory: Engine::core and the stage structs free theirs, on the engine's device)
}

int cesx_set_problem(cesx_handle h, const double* y, const double* Gamma, const double* mu,
                     const double* Sigma, const double* ustar) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!y || !Gamma || !mu || !Sigma || !ustar) { e.err = "cesx_set_problem: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    const int p = e.p, n = e.n;
    std::vector<double> L, Li, inv;
    if (!host_chol(n, Gamma, L)) { e.err = "Gamma is not symmetric positive definite"; return CESX_ENOTPD; }
    host_tri_inverse(n, L, Li);
    host_spd_inverse(n, Li, inv);
    // Dense Gamma: the engine works in whitened data coordinates (cesx_internal.h, Engine::whiten) -- y~ = L^{-1} y,
    // Gamma~ = I, and G~ = L^{-1} G formed once per step by the update kernel's own code (whitened_G below)
    // (nothing of the engine's state is committed before every allocation and upload below has succeeded: a failure leaves
    //  the handle WITHOUT a problem -- cesx_moments* / cesx_apply then return CESX_ESTATE -- instead of half of the new one)
    const bool whiten = !is_diagonal(n, Gamma);
    e.problem_set = false;
    // a new problem drops the MH proposal (include/cesx.h) and the descriptors of CESX_GP_DENSE and CESX_GP_PROJ: all are images
    // of the problem.  The GP image, the fit problem and the four forward maps (lineal, Darcy, Lorenz '96, Lorenz '63) stay installed.
    e.mh.drop(); e.gpd.drop(); e.gpp.drop();
    e.whiten = false;
    e.gw_src = nullptr;
    // the problem as given, for the one mode that factors Sigma_j = Gamma + B diag(v_j) B^T itself (kernels_gpdense.hip)
    e.h_y_raw.assign(y, y + n);
    e.h_Gamma_raw.resize((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k <= i; ++k) e.h_Gamma_raw[(size_t)i * n + k] = e.h_Gamma_raw[(size_t)k * n + i] = Gamma[(size_t)i * n + k];
    std::vector<double> gw(n), yi(y, y + n), Gi(Gamma, Gamma + (size_t)n * n);
    for (int i = 0; i < n; ++i) gw[i] = 1.0 / Gamma[(size_t)i * n + i];
    if (whiten) {
        e.h_LG = L; e.h_Li = Li;
        for (int i = 0; i < n; ++i) {
            double t = 0.0;
            for (int k = 0; k <= i; ++k) t += Li[(size_t)i * n + k] * y[k];
            yi[i] = t;
            gw[i] = 1.0;
            for (int k = 0; k < n; ++k) Gi[(size_t)i * n + k] = i == k ? 1.0 : 0.0;
        }
        // L^{-1} (lower triangular), zero padded to the update kernels' [rpad][kn] layout, row-major and fragment-major
        const size_t len = (size_t)e.rpad * e.kn;
        std::vector<double> rm(len, 0.0), fm(len, 0.0);
        const int nkt = e.kn / 16;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k <= i; ++k) {
                const double v = Li[(size_t)i * n + k];
                rm[(size_t)i * e.kn + k] = v;
                fm[e.cfg.dtype == CESX_F32 ? wf_index(i, k, nkt) : wd_index(i, k, nkt)] = v;
            }
        // (each buffer checked on its own: a second call finds what an earlier, failed one did allocate)
        if (!e.d_Wwh) TRY(core_alloc(e, &e.d_Wwh, len * e.esz));
        if (!e.d_Wwh_f) TRY(core_alloc(e, &e.d_Wwh_f, len * e.esz));
        if (!e.d_Gw) TRY(core_alloc(e, &e.d_Gw, (size_t)n * (size_t)e.J * e.esz, false));
        TRY(upload_T(e, e.d_Wwh, rm.data(), len)); TRY(upload_T(e, e.d_Wwh_f, fm.data(), len));
    }
    TRY(upload(e, e.d_y, yi.data(), n * 8)); TRY(upload(e, e.d_Gamma, Gi.data(), (size_t)n * n * 8));
    TRY(upload(e, e.d_gw, gw.data(), n * 8));
    TRY(upload(e, e.d_Wh, Li.data(), (size_t)n * n * 8));
    TRY(upload_T(e, e.d_yT, yi.data(), n)); TRY(upload_T(e, e.d_gwT, gw.data(), n));
    if (!host_chol(p, Sigma, L)) { e.err = "Sigma is not symmetric positive definite"; return CESX_ENOTPD; }
    host_tri_inverse(p, L, Li);
    host_spd_inverse(p, Li, inv);
    e.h_LSi = Li;
    e.h_mu.assign(mu, mu + p);
    e.diag_sigma = is_diagonal(p, Sigma);
    std::vector<double> sw(p);
    for (int i = 0; i < p; ++i) sw[i] = 1.0 / Sigma[(size_t)i * p + i];
    TRY(upload(e, e.d_mu, mu, p * 8)); TRY(upload(e, e.d_ustar, ustar, p * 8));
    TRY(upload(e, e.d_Sigma, Sigma, (size_t)p * p * 8)); TRY(upload(e, e.d_Sinv, inv.data(), (size_t)p * p * 8));
    TRY(upload(e, e.d_sw, sw.data(), p * 8));
    e.h_yw = yi; e.h_gw = gw; e.h_sw = sw;
    {
        // K3 through the Cholesky factor where the problem and the shape allow (cesx_internal.h, Engine::chain).  The two layouts
        // of d_Wq share no writer's footprint: a change of layout starts from a zeroed image, with nothing of the engine in flight
        const bool chain = e.chain_ok && e.hkfree_ok && e.diag_sigma && update4_shape_ok(e);
        if (chain != e.chain && e.d_Wq) {
            CESX_HIP(hipDeviceSynchronize());
            CESX_HIP(hipMemset(e.d_Wq, 0, std::max((size_t)e.rpad * e.ktot * 4, (size_t)(18 + e.kn / 16) * 16384)));
        }
        e.chain = chain;
    }
    // a new problem: the warm starts of K2's SPD inverses (kernels_dense.hip, spd_inverse) start cold
    if (e.d_ns_x[0][0]) {
        for (int k = 0; k < 2; ++k) { CESX_HIP(hipMemset(e.d_ns_x[0][k], 0, (size_t)n * n * 8)); CESX_HIP(hipMemset(e.d_ns_x[1][k], 0, (size_t)p * p * 8)); }
    }
    e.whiten = whiten;
    e.ns_r0_last = 1e300;          // (the first warm start of the new problem is sized like a cold one)
    e.problem_set = true;
    e.shift_valid = false;
    return CESX_OK;
}

size_t cesx_moments_len(cesx_handle h) { return h ? reinterpret_cast<Engine*>(h)->mom_len : 0; }
size_t cesx_moments_uu_len(cesx_handle h) { return h ? reinterpret_cast<Engine*>(h)->ml.uu_len() : 0; }

void* cesx_side_stream(cesx_handle h) { return h ? (void*)reinterpret_cast<Engine*>(h)->side : nullptr; }

int cesx_colsum(cesx_handle h, const void* U, const void* G, double* sums, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G || !sums) { e.err = "cesx_colsum: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_colsum(e, U, G, sums, (hipStream_t)stream);
}

int cesx_set_shift(cesx_handle h, const double* sums, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!sums) { e.err = "cesx_set_shift: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_set_shift(e, sums, (hipStream_t)stream);
}

static int moments_check(Engine& e, const void* U, const void* G, double* mom) {
    ++e.moments_calls;
    // A step whose polled join runs out is re-run by cesx_result FROM ITS OWN moment buffer (include/cesx.h, lifetime
    // rules).  A caller that hands the same buffer to the next step's moments before it has read that result gives the
    // buffer up: the re-run is then not attempted (cesx_result reports CESX_EHIP for such a step instead of computing it
    // from the next step's moments).
    if (e.last_apply.valid && e.pending && mom != nullptr && mom == e.last_apply.mom) e.last_apply.mom_reused = true;
    if (!U || !G || !mom) { e.err = "cesx_moments: null pointer"; return CESX_EINVAL; }
    if (!e.problem_set) { e.err = "cesx_set_problem has not been called"; return CESX_ESTATE; }
    if (!e.shift_valid) { e.err = "no centring shift: call cesx_colsum + cesx_set_shift (or cesx_step with recenter) first"; return CESX_ESTATE; }
    return CESX_OK;
}

// The first half of a step (cesx_moments_uu*): the U x U launch and its reduce on the caller's stream, then
//   Plain:        nothing;
//   Handover:     the side stream is made to wait for the reduce -- the hand-over event (ev_a) bound to the reduce kernel's own
//                 completion signal, no marker packet in front of whatever the caller's stream runs next -- and, when the
//                 previous update's metric finalisation is still pending on this stream, that too as the reduce launch's
//                 first workgroup;
//   HandoverChol: the same and the factorisation behind it (nothing can sit between the reduce and the hand-over).
// A caller already on the side stream has nothing to hand over: its own ordering applies.
enum class UuThen { Plain, Handover, HandoverChol };
static int moments_uu(cesx_handle h, const void* U, const void* G, double* mom, void* stream, UuThen then, int update = 0) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(moments_check(e, U, G, mom));
    if (update < 0 || update > 2) { e.err = "cesx_moments_uu_chol: bad argument"; return CESX_EINVAL; }
    SET_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const bool hand = then != UuThen::Plain && s != e.side;
    ++e.prof_step;
    if (!hand || e.met_stream != s) FLUSH(e);      // (a hand-over on the deferred finalisation's own stream carries it)
    WHITEN_UU(e, G, s);
    GramLaunch L{.part = 0, .U = U, .G = G, .mom = mom, .s = s};
    if (hand) {
        L.bound_stop = e.ev_a;
        if (e.met_deferred) {
            L.fin = metric_fin_args(e, nullptr, true);
            L.fin.N = (double)e.Jg;
            e.met_deferred = false;
        }
    }
    TRY(launch_moments(e, L));
    if (hand) CESX_HIP(hipStreamWaitEvent(e.side, e.ev_a, 0));
    return then == UuThen::HandoverChol ? launch_chol_async(e, update, mom, s, hand) : CESX_OK;
}

int cesx_moments_uu(cesx_handle h, const void* U, const void* G, double* mom, void* stream) {
    return moments_uu(h, U, G, mom, stream, UuThen::Plain);
}
int cesx_moments_uu_handover(cesx_handle h, const void* U, const void* G, double* mom, void* stream) {
    return moments_uu(h, U, G, mom, stream, UuThen::Handover);
}
int cesx_moments_uu_chol(cesx_handle h, int update, const void* U, const void* G, double* mom, void* stream) {
    return moments_uu(h, U, G, mom, stream, UuThen::HandoverChol, update);
}

int cesx_chol_async(cesx_handle h, int update, const double* mom, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!mom || update < 0 || update > 2) { e.err = "cesx_chol_async: bad argument"; return CESX_EINVAL; }
    if (!e.problem_set) { e.err = "cesx_set_problem has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_chol_async(e, update, mom, (hipStream_t)stream);
}

int cesx_moments_rest(cesx_handle h, const void* U, const void* G, double* mom, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(moments_check(e, U, G, mom));
    SET_DEVICE(e);
    FLUSH(e);
    // (the reduce kernel of this launch also copies this shard's data-metric sums of the PREVIOUS
    //  apply to the tail of the buffer: they ride on this step's all-reduce)
    WHITEN(e, G, stream, true);
    return launch_moments(e, GramLaunch{.part = 1, .U = U, .G = G, .mom = mom, .s = (hipStream_t)stream});
}

int cesx_moments_rest_lineal(cesx_handle h, double* mom, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!mom) { e.err = "cesx_moments_rest_lineal: null pointer"; return CESX_EINVAL; }
    if (!e.problem_set) { e.err = "cesx_set_problem has not been called"; return CESX_ESTATE; }
    if (!e.shift_valid) { e.err = "no centring shift: call cesx_colsum + cesx_set_shift (or cesx_step with recenter) first"; return CESX_ESTATE; }
    if (!e.fwd_set) { e.err = "cesx_moments_rest_lineal: cesx_forward_set_lineal has not been called"; return CESX_ESTATE; }
    if (e.whiten) { e.err = "cesx_moments_rest_lineal: dense Gamma (the engine works on whitened data: take cesx_moments_rest)"; return CESX_EUNSUPPORTED; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_moments_lineal(e, mom, (hipStream_t)stream);
}

int cesx_moments(cesx_handle h, const void* U, const void* G, double* mom, void* stream) {
    int rc = cesx_moments_uu(h, U, G, mom, stream);
    return rc ? rc : cesx_moments_rest(h, U, G, mom, stream);
}

int cesx_apply_drift(cesx_handle h, const cesx_step_params* prm, const double* mom, const void* U,
                     const void* G, void* Unext, double* absmax, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(check_prm(e, prm));
    if (!mom || !U || !G || !Unext || !absmax) { e.err = "cesx_apply_drift: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    WHITEN(e, G, s, false);
    const DenseLaunch K2{.prm = prm, .mom = mom, .phase = DensePhase::Drift, .s = s};
    TRY(launch_dense(e, K2, plan_dense(e, K2, poll_join_open(e, s) && stream_below_side(e, s))));
    TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.d_W, .Wf = e.d_Wf, .ktot = e.kp + e.kn, .bias = e.d_bias,
                                      .src = {{U, e.p, 0, 0}, {G, e.n, 0, 0}}, .nsrc = 2, .out = Unext,
                                      .absmax_part = e.d_absmax_part, .step_index = prm->step_index, .metrics = true}, s));
    e.last_metric_parts = e.last_update_grid_x;
    const int nparts = e.last_update_grid;
    TRY(launch_metric_final(e, mom, false, s));      // data metrics: K3 accumulated them while the (whitened) G rows streamed by
    return launch_absmax_final(e, nparts, absmax, s);
}

int cesx_apply_finish(cesx_handle h, const cesx_step_params* prm, const double* absmax, const void* U,
                      const void* xi, void* Unext, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(check_prm(e, prm));
    if (!absmax || !U || !Unext) { e.err = "cesx_apply_finish: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    if (absmax != e.d_absmax) CESX_HIP(hipMemcpyAsync(e.d_absmax, absmax, 8, hipMemcpyDeviceToDevice, s));
    const DenseLaunch K2{.prm = prm, .phase = DensePhase::Noise, .s = s};
    TRY(launch_dense(e, K2, plan_dense(e, K2, false)));
    // U_next = sqrt(2hk) L xi + 1 * U + hk * drift   (drift currently lives in U_next)
    if (!xi) xi = prefetched_noise(e, *prm, s);
    TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.d_W, .Wf = e.d_Wf, .ktot = e.kp, .src = {{xi, e.p, xi ? 0 : 1, 1}},
                                      .nsrc = 1, .add1 = {U, nullptr, 1.0}, .add2 = {Unext, &e.d_scal->hk, 1.0}, .out = Unext,
                                      .step_index = prm->step_index}, s));
    TRY(launch_publish(e, s));
    return finish_step(e, *prm);
}

int cesx_apply(cesx_handle h, const cesx_step_params* prm, const double* mom, const void* U, const void* G,
               const void* xi, void* Unext, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(check_prm(e, prm));
    if (!mom || !U || !G || !Unext) { e.err = "cesx_apply: null pointer"; return CESX_EINVAL; }
    if (U == Unext) { e.err = "U_next must not alias U (ces/calibrate.py:357 keeps U0 in the trace)"; return CESX_EINVAL; }
    if (prm->update == CESX_UPDATE_ALDI_CONSTANT) {
        TRY(cesx_apply_drift(h, prm, mom, U, G, Unext, e.d_absmax, stream));
        return cesx_apply_finish(h, prm, e.d_absmax, U, xi, Unext, stream);
    }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    e.last_apply = Engine::LastApply{true, *prm, mom, U, G, xi, Unext, s, e.moments_calls};     // (the caller's G: a re-run whitens it again if need be)
    WHITEN(e, G, s, false);
    // (the kernel that would take this step's hk-free image is known here: the hk-free K2 has no other consumer)
    const UpdateKernel hk = pick_update_kernel(e, main_update(e, *prm, U, G, xi, Unext, true));
    const DenseLaunch K2{.prm = prm, .mom = mom, .phase = DensePhase::Step, .s = s, .upd_ok = hk != UpdateKernel::None};
    const DensePlan plan = plan_dense(e, K2, poll_join_open(e, s) && stream_below_side(e, s));
    // the chained form reads its noise from memory: a block neither injected nor drawn ahead goes into an engine buffer,
    // allocated here -- nothing is allocated once K2 is enqueued
    if (hk == UpdateKernel::Update4 && !xi && prefetched_block(e, prm->step_index) < 0 && plan.route == DenseRoute::Tail && !e.d_xi_tmp)
        TRY(core_alloc(e, &e.d_xi_tmp, (size_t)e.p * (size_t)e.J * e.esz, false));
    TRY(launch_dense(e, K2, plan));
    TRY(run_update_main(e, *prm, U, G, xi, Unext, s));
    // (Moving this last small kernel to the side stream was tried: the event record + wait pair costs
    //  as much GPU idle time as the 7 us kernel itself.)
    if (e.overlap_chol) {
        // the finalisation rides on the next step's U x U reduce launch (cesx_moments_uu_chol / _handover on this
        // stream) -- no one-workgroup kernel (7 us) between this update and the next Gram launch; anything else flushes it
        e.met_deferred = true; e.met_stream = s;      // (reads the engine's own d_lag, not `mom`)
    } else {
        TRY(launch_metric_final(e, mom, true, s));     // also publishes the step result to the host
    }
    return finish_step(e, *prm);
}

int cesx_step(cesx_handle h, const cesx_step_params* prm, const void* U, const void* G, const void* xi,
              void* Unext, int recenter, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(check_prm(e, prm));
    if (!U || !G || !Unext) { e.err = "cesx_step: null pointer"; return CESX_EINVAL; }
    if (e.J != e.Jg) { e.err = "cesx_step is single-device: use cesx_moments / all-reduce / cesx_apply for a sharded ensemble"; return CESX_ESTATE; }
    if (U == Unext) { e.err = "U_next must not alias U (ces/calibrate.py:357 keeps U0 in the trace)"; return CESX_EINVAL; }
    if (recenter || !e.shift_valid) {
        TRY(cesx_colsum(h, U, G, e.d_sums, stream));
        TRY(cesx_set_shift(h, e.d_sums, stream));
    }
    if (!xi && e.overlap_chol) TRY(cesx_prefetch_noise(h, prm->step_index, stream));
    // U x U moments -> chol(C) on the side stream, beside the rest of the Gram -> apply.  (Putting the
    // U x U launch itself on the side stream too was measured slower: see ces_amd/dist.py.)
    if (e.overlap_chol) TRY(cesx_moments_uu_chol(h, prm->update, U, G, e.d_mom, stream));
    else TRY(cesx_moments_uu(h, U, G, e.d_mom, stream));
    TRY(cesx_moments_rest(h, U, G, e.d_mom, stream));
    return cesx_apply(h, prm, e.d_mom, U, G, xi, Unext, stream);
}

int cesx_result(cesx_handle h, cesx_step_result* out) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!out) { e.err = "cesx_result: null pointer"; return CESX_EINVAL; }
    if (!e.pending) { e.err = "cesx_result: no step has been enqueued"; return CESX_ESTATE; }
    if (e.met_deferred) {
        SET_DEVICE(e);
        FLUSH(e);
    }
    // Wait for the sequence number the GPU writes last into pinned memory.  A step is a few
    // hundred microseconds, so the first 100 us are a pause-spin (lowest latency); after that the
    // thread yields its core, and from 2 ms on it sleeps in 100 us slices -- a long wait (large
    // shards, a stalled collective) does not burn a host core.
    {
        volatile unsigned long long* seq = &e.h_scal->seq;
        const auto t0 = std::chrono::steady_clock::now();
        unsigned spins = 0;
        while (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != e.seq) {
            __builtin_ia32_pause();
            if ((++spins & 0x3ff) != 0) continue;
            const auto waited = std::chrono::steady_clock::now() - t0;
            if (waited < std::chrono::microseconds(100)) continue;
            if (waited < std::chrono::milliseconds(2)) { sched_yield(); continue; }
            if (hipPeekAtLastError() != hipSuccess) { e.err = "HIP error while waiting for the step"; return CESX_EHIP; }
            if (waited > std::chrono::seconds(120)) { e.err = "timed out waiting for the step result"; return CESX_EHIP; }
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    }
    const Scalars& sc = *e.h_scal;
    out->hk = sc.hk; out->t_new = sc.t_new;
    out->self_bias = sc.self_bias; out->self_bias_data = sc.self_bias_data;
    out->bias_data = sc.bias_data; out->bias = sc.bias;
    out->radspec = sc.radspec; out->status = sc.status; out->reserved = 0;
    out->lag_bias_data = sc.spare[1]; out->lag_self_bias_data = sc.spare[2];
    e.ns_r0_last = sc.spare[3] > 0.0 ? sc.spare[3] : 1e300;      // (kernels_dense.hip, spd_inverse: sizes the next warm start's sweeps)
    if (sc.status == CESX_ENOTPD) {
        e.err = "ensemble covariance is not positive definite (Cholesky failed)";
        return CESX_ENOTPD;
    }
    if (sc.status == CESX_EHIP) {
        // The polled join ran out (kernels_dense.hip): the step wrote NOTHING (no W, no centring shift, U_next untouched).
        // From here on this engine joins its side stream with the event, and the step is re-run once with chol(C)
        // in line on the caller's stream (correct whatever the side stream is doing).
        e.poll_join_ok = false;
        if (e.last_apply.valid && !e.in_retry && e.fac.polled && !e.last_apply.mom_reused) {
            const Engine::LastApply la = e.last_apply;
            e.in_retry = true;
            // whatever a pipelined driver put on the side stream behind the failed step (the centring + chol(C) of moments of
            // an unwritten ensemble: it may well report "not positive definite") ends BEFORE the re-run resets the status word
            {
                SET_DEVICE(e);
                CESX_HIP(hipStreamSynchronize(e.side));
            }
            e.fac.inflight = false;
            int rc = cesx_apply(h, &la.prm, la.mom, la.U, la.G, la.xi, la.Unext, (void*)la.s);
            if (rc == CESX_OK) rc = cesx_result(h, out);
            e.in_retry = false;
            if (rc != CESX_OK) return rc;
            ++e.poll_recoveries;
            if (e.moments_calls != la.moments_calls) {
                e.err = "the polled join of the side stream timed out; the step was re-run and its result is valid, but moments "
                        "enqueued after it were taken of an ensemble that had not been written yet: redo them";
                return CESX_ESTATE;
            }
            return CESX_OK;
        }
        e.err = e.last_apply.valid && e.last_apply.mom_reused
            ? "the side stream's factorisation never signalled its completion (the polled join timed out), and the step's moment "
              "buffer had already been handed to a later cesx_moments* call: not re-run (include/cesx.h, lifetime rules)"
            : "the side stream's factorisation never signalled its completion (the polled join timed out)";
        return CESX_EHIP;
    }
    return CESX_OK;
}

unsigned long long cesx_debug_poll_recoveries(cesx_handle h) { return h ? reinterpret_cast<Engine*>(h)->poll_recoveries : 0; }

int cesx_debug_update_form(cesx_handle h) {
    if (!h) return -1;
    const Engine& e = *reinterpret_cast<Engine*>(h);
    return !e.last_hkfree ? 0 : e.chain ? 2 : 1;
}

int cesx_debug_warm_inverse(cesx_handle h) {
    if (!h) return -1;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!e.d_ns_skip) return 0;
    DeviceGuard dg(e.cfg.device);
    int v = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, e.d_ns_skip, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

int cesx_draw_noise(cesx_handle h, uint64_t step_index, void* xi, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!xi) { e.err = "cesx_draw_noise: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    return launch_noise(e, step_index, xi, (hipStream_t)stream);
}

int cesx_prefetch_noise(cesx_handle h, uint64_t step_index, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    SET_DEVICE(e);
    (void)stream;
    if (std::getenv("CESX_NO_NOISE_PREFETCH")) return CESX_OK;
    e.xi_lookahead = !(std::getenv("CESX_NOISE_LOOKAHEAD") && std::atoi(std::getenv("CESX_NOISE_LOOKAHEAD")) == 0);
    for (int b = 0; b < (e.xi_lookahead ? 2 : 1); ++b)
        if (!e.d_xi[b]) TRY(core_alloc(e, &e.d_xi[b], (size_t)e.p * (size_t)e.J * e.esz, false));
    // The draw itself is enqueued by cesx_chol_async on the side stream, behind chol(C): no extra
    // cross-stream event (each costs ~6 us of GPU idle time), and it runs while the caller's stream
    // is in the tail of the second Gram launch and the latency-bound start of K2.
    e.xi_want = (long long)step_index;
    return CESX_OK;
}

int cesx_forward_lineal(cesx_handle h, const void* A, const void* b, const void* U, void* G, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!A || !U || !G) { e.err = "cesx_forward_lineal: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    // stage A (n x p) into the zero-padded (rpad x kp) layout the update kernel reads
    CESX_HIP(hipMemsetAsync(e.d_Wfwd, 0, (size_t)e.rpad * e.kp * e.esz, s));
    CESX_HIP(hipMemcpy2DAsync(e.d_Wfwd, (size_t)e.kp * e.esz, A, (size_t)e.p * e.esz, (size_t)e.p * e.esz, e.n,
                              hipMemcpyDeviceToDevice, s));
    return launch_update(e, UpdateLaunch{.out_rows = e.n, .W = e.d_Wfwd, .ktot = e.kp, .bias = b, .src = {{U, e.p, 0, 0}}, .nsrc = 1,
                                         .out = G}, s);
}

int cesx_forward_set_lineal(cesx_handle h, const void* A, const void* b, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!A) { e.err = "cesx_forward_set_lineal: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    TRY(launch_stage_forward(e, A, b, (hipStream_t)stream));
    e.fwd_set = true;
    e.fwd_has_b = b != nullptr;
    return CESX_OK;
}

int cesx_forward_apply(cesx_handle h, const void* U, void* G, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G) { e.err = "cesx_forward_apply: null pointer"; return CESX_EINVAL; }
    if (!e.fwd_set) { e.err = "cesx_forward_apply: cesx_forward_set_lineal has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return launch_update(e, UpdateLaunch{.out_rows = e.n, .W = e.d_Wfwd, .Wf = e.d_Wfwd_f, .ktot = e.kp,
                                         .bias = e.fwd_has_b ? e.d_bfwd : nullptr, .src = {{U, e.p, 0, 0}}, .nsrc = 1, .out = G},
                         (hipStream_t)stream);
}

// ---- Sample: Metropolis-Hastings over the columns (ces/sample.py; kernels_mh.hip) ----

// the Philox step word of an MH draw: a counter domain of its own (include/cesx.h)
static unsigned mh_step_word(uint64_t step_index) { return (unsigned)(step_index | 0x80000000ull); }

// a lower-triangular p x p fp64 matrix (row-major), zero padded into the update kernels' [rpad][kp] layouts, engine dtype
static int mh_upload_tri(Engine& e, const double* M, DevBuf<void>& rm_dev, DevBuf<void>& fm_dev) {
    const size_t len = (size_t)e.rpad * e.kp;
    std::vector<double> rm(len, 0.0), fm(len, 0.0);
    const int nkt = e.kp / 16;
    for (int i = 0; i < e.p; ++i)
        for (int k = 0; k <= i; ++k) {
            const double v = M[(size_t)i * e.p + k];
            rm[(size_t)i * e.kp + k] = v;
            fm[e.cfg.dtype == CESX_F32 ? wf_index(i, k, nkt) : wd_index(i, k, nkt)] = v;
        }
    TRY_BUF(rm_dev.ensure(len * e.esz)); TRY_BUF(fm_dev.ensure(len * e.esz));
    TRY(upload_T(e, rm_dev, rm.data(), len));
    return upload_T(e, fm_dev, fm.data(), len);
}

// phi of the states X with their forward map G (cesx_mh_start: into the engine's phi; cesx_mh_accept: the test and U := X)
static int mh_score(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    WHITEN(e, G, s, true);
    // a dense prior: w = L_Sigma^{-1} X - L_Sigma^{-1} mu, one triangular product (the kernel skips the zero blocks)
    if (e.mh.dense_prior)
        TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.Li, .Wf = e.mh.Li_f, .ktot = e.kp, .bias = e.mh.lb,
                                          .src = {{X, e.p, 0, 1}}, .nsrc = 1, .out = e.mh.w}, s));
    return launch_mh_score(e, start, X, G, U, logu, step, s);
}

// Failure rule: from the synchronise until the last upload the handle has NO proposal; a failure leaves it so.  The buffers are kept.
int cesx_mh_set_proposal(cesx_handle h, int kind, const double* S, double beta) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!S) { e.err = "cesx_mh_set_proposal: null pointer"; return CESX_EINVAL; }
    if (kind != CESX_MH_RW && kind != CESX_MH_PCN && kind != CESX_MH_LANGEVIN) { e.err = "cesx_mh_set_proposal: unknown proposal kind"; return CESX_EINVAL; }
    if (kind == CESX_MH_PCN && !(beta > 0.0 && beta <= 1.0)) { e.err = "cesx_mh_set_proposal: pCN needs 0 < beta <= 1"; return CESX_EINVAL; }
    if (!e.problem_set) { e.err = "cesx_set_problem has not been called"; return CESX_ESTATE; }
    const int p = e.p;
    for (int i = 0; i < p; ++i)
        for (int k = i + 1; k < p; ++k)
            if (S[(size_t)i * p + k] != 0.0) { e.err = "cesx_mh_set_proposal: S is not lower triangular"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (the images below may be read by launches still in flight)
    e.mh.drop();
    const double b = kind == CESX_MH_PCN ? std::sqrt(beta) : 1.0;          // ces/sample.py:202: sqrt(beta), not beta
    std::vector<double> bS(S, S + (size_t)p * p);
    for (double& v : bS) v *= b;
    TRY(mh_upload_tri(e, bS.data(), e.mh.W, e.mh.Wf));
    e.mh.h_bS = bS;
    TRY_BUF(e.mh.bS.ensure((size_t)p * p * 8));
    TRY(upload(e, e.mh.bS, bS.data(), (size_t)p * p * 8));
    e.mh.dense_prior = kind == CESX_MH_RW && !e.diag_sigma;
    if (!e.diag_sigma) {                       // gp_score_kernel's fp64 L_Sigma^{-1} (RW and pCN: ces/sample.py:57 / :96)
        TRY_BUF(e.mh.LSi.ensure((size_t)p * p * 8));
        TRY(upload(e, e.mh.LSi, e.h_LSi.data(), (size_t)p * p * 8));
    }
    if (e.mh.dense_prior) {
        TRY(mh_upload_tri(e, e.h_LSi.data(), e.mh.Li, e.mh.Li_f));
        std::vector<double> lb(e.rpad, 0.0);
        for (int i = 0; i < p; ++i) {
            double acc = 0.0;
            for (int k = 0; k <= i; ++k) acc += e.h_LSi[(size_t)i * p + k] * e.h_mu[k];
            lb[i] = -acc;
        }
        TRY_BUF(e.mh.lb.ensure((size_t)e.rpad * e.esz));
        TRY(upload_T(e, e.mh.lb, lb.data(), e.rpad));
        TRY_BUF(e.mh.w.ensure((size_t)p * (size_t)e.J * e.esz));
    }
    if (e.cfg.dtype == CESX_F64 || kind == CESX_MH_LANGEVIN) TRY_BUF(e.mh.xi.ensure((size_t)p * (size_t)e.J * e.esz));
    if (kind == CESX_MH_LANGEVIN) {            // what the lv_* kernels keep per chain (kernels_gpgrad.hip)
        TRY_BUF(e.mh.lv_g.ensure((size_t)p * (size_t)e.J * 8)); TRY_BUF(e.mh.lv_gp.ensure((size_t)p * (size_t)e.J * 8));
        TRY_BUF(e.mh.lv_gphi.ensure((size_t)p * (size_t)e.J * 8)); TRY_BUF(e.mh.hm_r.ensure((size_t)p * (size_t)e.J * 8));
        // (rows for max(n, k): CESX_GP_PROJ's coefficients are k-dimensional; a descriptor installed later grows them, proj_rows)
        const size_t rows = (size_t)std::max(e.n, e.gpp.k);
        TRY_BUF(e.mh.lv_a.ensure(rows * (size_t)e.J * 8)); TRY_BUF(e.mh.lv_b.ensure(rows * (size_t)e.J * 8));
        TRY_BUF(e.mh.phi_data.ensure((size_t)e.J * 8));
    }
    TRY_BUF(e.mh.phi.ensure((size_t)e.J * 8)); TRY_BUF(e.mh.cnt.ensure((size_t)e.J * 8));
    e.mh.a = kind == CESX_MH_PCN ? std::sqrt(1.0 - beta * beta) : 1.0;
    e.mh.kind = kind;
    return CESX_OK;
}

int cesx_mh_start(cesx_handle h, const void* U, const void* G, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G) { e.err = "cesx_mh_start: null pointer"; return CESX_EINVAL; }
    if (e.mh.none() || !e.problem_set) { e.err = "cesx_mh_start: no proposal (cesx_mh_set_proposal after cesx_set_problem)"; return CESX_ESTATE; }
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_mh_start: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(mh_score(e, true, U, G, nullptr, nullptr, 0u, (hipStream_t)stream));
    e.mh.started = true;
    e.mh.steps = 0;
    return CESX_OK;
}

int cesx_mh_propose(cesx_handle h, uint64_t step_index, const void* U, const void* xi, void* P, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !P) { e.err = "cesx_mh_propose: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_mh_propose: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_propose: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    if (e.mh.none()) { e.err = "cesx_mh_propose: cesx_mh_set_proposal has not been called"; return CESX_ESTATE; }
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_mh_propose: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    const unsigned sw = mh_step_word(step_index);
    // fp64: the block is drawn into the engine's buffer first (update3_kernel reads every segment from memory)
    if (!xi && e.cfg.dtype == CESX_F64) {
        TRY(launch_noise(e, sw, e.mh.xi, s));
        xi = e.mh.xi;
    }
    return launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.W, .Wf = e.mh.Wf, .ktot = e.kp,
                                         .src = {{xi, e.p, xi ? 0 : 1, 1}}, .nsrc = 1, .add1 = {U, nullptr, e.mh.a}, .out = P,
                                         .step_index = sw}, s);
}

int cesx_mh_accept(cesx_handle h, uint64_t step_index, void* U, const void* P, const void* GP, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !P || !GP) { e.err = "cesx_mh_accept: null pointer"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    // (the kind first, as cesx_mh_start, cesx_mh_propose, cesx_mh_run_map and cesx_gp_run answer: under a Langevin proposal the call is
    //  refused as such, whether or not one of the Langevin starts has run)
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_mh_accept: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }
    if (e.mh.none() || !e.mh.started) { e.err = "cesx_mh_accept: cesx_mh_start has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(mh_score(e, false, P, GP, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_mh_stats(cesx_handle h, unsigned long long* steps, double* rate, unsigned long long* per_chain) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!steps || !rate) { e.err = "cesx_mh_stats: null pointer"; return CESX_EINVAL; }
    if (!e.mh.started) { e.err = "cesx_mh_stats: cesx_mh_start has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    std::vector<unsigned long long> c((size_t)e.J);
    CESX_HIP(hipDeviceSynchronize());
    CESX_HIP(hipMemcpy(c.data(), e.mh.cnt, (size_t)e.J * 8, hipMemcpyDeviceToHost));
    unsigned long long sum = 0;
    for (unsigned long long v : c) sum += v;
    *steps = e.mh.steps;
    *rate = e.mh.steps ? (double)sum / ((double)e.mh.steps * (double)e.J) : 0.0;
    if (per_chain) std::memcpy(per_chain, c.data(), (size_t)e.J * 8);
    return CESX_OK;
}

// ---- Emulate: GP prediction and the GP sampler over the columns (ces/emulate.py, ces/sample.py:17-119; kernels_gp.hip) ----

// Failure rule: an argument error leaves the OLD image; behind the synchronise the old image is dropped, and a failure then leaves none.
int cesx_gp_set(cesx_handle h, const cesx_gp_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != sizeof(cesx_gp_desc)) { e.err = "cesx_gp_set: bad cesx_gp_desc"; return CESX_EINVAL; }
    if (!d->A || !d->c || !d->Z || !d->family || !d->par || !d->mw || !d->alpha || !d->Li) { e.err = "cesx_gp_set: null pointer"; return CESX_EINVAL; }
    if (d->n_gp < 1 || d->J_t < 1) { e.err = "cesx_gp_set: n_gp and J_t must be >= 1"; return CESX_EINVAL; }
    const int n = d->n_gp, Jt = d->J_t, p = e.p, Jp = (Jt + 15) / 16 * 16, NB = Jp / 16;
    for (int i = 0; i < n; ++i)
        if (d->family[i] < 0 || d->family[i] > 3) { e.err = "cesx_gp_set: unknown kernel family"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (the old image may be read by launches still in flight)
    e.gp.drop();
    const size_t li_len = (size_t)NB * (NB + 1) / 2 * 256;
    std::vector<double> par((size_t)n * 4), alpha((size_t)n * Jp, 0.0), Li((size_t)n * li_len, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) par[(size_t)i * 4 + k] = d->par[(size_t)i * 3 + k];
        par[(size_t)i * 4 + 3] = (double)d->family[i];
        for (int t = 0; t < Jt; ++t) alpha[(size_t)i * Jp + t] = d->alpha[(size_t)i * Jt + t];
        // L^{-1} in the A-operand order of v_mfma_f64_16x16x4_f64: block row b, k-step k4, lane l holds
        // L^{-1}[16 b + (l & 15)][4 k4 + (l >> 4)] (zero above the diagonal and past J_t)
        const double* L = d->Li + (size_t)i * Jt * Jt;
        double* o = Li.data() + (size_t)i * li_len;
        for (int b = 0; b < NB; ++b)
            for (int k4 = 0; k4 < (b + 1) * 4; ++k4)
                for (int l = 0; l < 64; ++l) {
                    const int row = 16 * b + (l & 15), col = 4 * k4 + (l >> 4);
                    *o++ = row < Jt && col <= row ? L[(size_t)row * Jt + col] : 0.0;
                }
    }
    TRY_BUF(e.gp.A.alloc((size_t)n * p * p * 8)); TRY(upload(e, e.gp.A, d->A, (size_t)n * p * p * 8));
    TRY_BUF(e.gp.c.alloc((size_t)p * 8)); TRY(upload(e, e.gp.c, d->c, (size_t)p * 8));
    TRY_BUF(e.gp.Z.alloc((size_t)n * Jt * p * 8)); TRY(upload(e, e.gp.Z, d->Z, (size_t)n * Jt * p * 8));
    TRY_BUF(e.gp.par.alloc(par.size() * 8)); TRY(upload(e, e.gp.par, par.data(), par.size() * 8));
    TRY_BUF(e.gp.mw.alloc((size_t)n * p * 8)); TRY(upload(e, e.gp.mw, d->mw, (size_t)n * p * 8));
    TRY_BUF(e.gp.alpha.alloc(alpha.size() * 8)); TRY(upload(e, e.gp.alpha, alpha.data(), alpha.size() * 8));
    TRY_BUF(e.gp.Li.alloc(Li.size() * 8)); TRY(upload(e, e.gp.Li, Li.data(), Li.size() * 8));
    e.gp.Jt = Jt; e.gp.Jp = Jp; e.gp.li_len = li_len;
    e.gp.matern12 = false;
    for (int i = 0; i < n; ++i) e.gp.matern12 = e.gp.matern12 || d->family[i] == 1;
    e.gp.n = n;
    return CESX_OK;
}

int cesx_gp_predict(cesx_handle h, const void* X, double* mean, double* var, int nugget, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!X || !mean) { e.err = "cesx_gp_predict: null pointer"; return CESX_EINVAL; }
    if (e.gp.none()) { e.err = "cesx_gp_predict: cesx_gp_set has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_gp_predict(e, X, mean, var, nugget != 0, (hipStream_t)stream);
}

// Failure rule: from the synchronise until the last upload the handle has NO descriptor; a failure leaves it so.  The buffers are kept.
int cesx_gp_dense_set(cesx_handle h, const cesx_gp_dense_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != sizeof(cesx_gp_dense_desc)) { e.err = "cesx_gp_dense_set: bad cesx_gp_dense_desc"; return CESX_EINVAL; }
    if (e.n > CESX_GP_DENSE_NMAX) { e.err = "cesx_gp_dense_set: n_obs is limited to 128 (the factor of Sigma lives in LDS)"; return CESX_EINVAL; }
    if (d->k < 1 || d->k > e.n) { e.err = "cesx_gp_dense_set: k must be in 1 .. n_obs"; return CESX_EINVAL; }
    if (!d->B) { e.err = "cesx_gp_dense_set: null pointer"; return CESX_EINVAL; }
    if (!e.problem_set) { e.err = "cesx_gp_dense_set: cesx_set_problem has not been called"; return CESX_ESTATE; }
    const int n = e.n, k = d->k;
    std::vector<double> B(d->B, d->B + (size_t)n * k), Bt((size_t)n * k), g0(n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < k; ++t) Bt[(size_t)t * n + i] = B[(size_t)i * k + t];
    if (d->g0) g0.assign(d->g0, d->g0 + n);
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (the old image may be read by launches still in flight)
    e.gpd.drop();
    // B for the largest k once: a later descriptor of the same engine fits
    TRY_BUF(e.gpd.B.ensure((size_t)n * n * 8));
    TRY_BUF(e.gpd.Bt.ensure((size_t)n * n * 8));
    TRY_BUF(e.gpd.g0.ensure((size_t)n * 8));
    TRY_BUF(e.gpd.y.ensure((size_t)n * 8));
    TRY_BUF(e.gpd.Gam.ensure((size_t)n * n * 8));
    TRY(upload(e, e.gpd.B, B.data(), B.size() * 8)); TRY(upload(e, e.gpd.Bt, Bt.data(), Bt.size() * 8));
    TRY(upload(e, e.gpd.g0, g0.data(), (size_t)n * 8));
    TRY(upload(e, e.gpd.y, e.h_y_raw.data(), (size_t)n * 8));
    TRY(upload(e, e.gpd.Gam, e.h_Gamma_raw.data(), (size_t)n * n * 8));
    TRY(gp_dense_prepare(e, n, k));
    e.gpd.logdet = d->logdet ? 1 : 0;
    e.gpd.k = k;
    return CESX_OK;
}

// Failure rule: as cesx_gp_dense_set's.
int cesx_gp_proj_set(cesx_handle h, const cesx_gp_proj_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != sizeof(cesx_gp_proj_desc)) { e.err = "cesx_gp_proj_set: bad cesx_gp_proj_desc"; return CESX_EINVAL; }
    if (d->k < 1 || d->k > CESX_GP_PROJ_KMAX) { e.err = "cesx_gp_proj_set: k must be in 1 .. 128 (the factor of I + S lives in LDS)"; return CESX_EINVAL; }
    if (!d->R || !d->a0) { e.err = "cesx_gp_proj_set: null pointer"; return CESX_EINVAL; }
    const int k = d->k;
    // R with its zeros below the diagonal (only the upper triangle is read) and its transpose
    std::vector<double> R((size_t)k * k, 0.0), Rt((size_t)k * k, 0.0);
    bool finite = std::isfinite(d->c_perp) && std::isfinite(d->half_logdet_gamma);
    for (int i = 0; i < k; ++i) {
        finite = finite && std::isfinite(d->a0[i]);
        for (int t = i; t < k; ++t) {
            const double r = d->R[(size_t)i * k + t];
            finite = finite && std::isfinite(r);
            R[(size_t)i * k + t] = Rt[(size_t)t * k + i] = r;
        }
    }
    if (!finite) { e.err = "cesx_gp_proj_set: a non-finite entry in R, a0, c_perp or half_logdet_gamma"; return CESX_EINVAL; }
    if (d->c_perp < 0.0) { e.err = "cesx_gp_proj_set: c_perp must be >= 0"; return CESX_EINVAL; }
    if (!e.problem_set) { e.err = "cesx_gp_proj_set: cesx_set_problem has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (the old image may be read by launches still in flight)
    e.gpp.drop();
    // for the largest k once: a later descriptor fits
    const size_t kmax = CESX_GP_PROJ_KMAX;
    TRY_BUF(e.gpp.R.ensure(kmax * kmax * 8));
    TRY_BUF(e.gpp.Rt.ensure(kmax * kmax * 8));
    TRY_BUF(e.gpp.a0.ensure(kmax * 8));
    TRY(upload(e, e.gpp.R, R.data(), R.size() * 8)); TRY(upload(e, e.gpp.Rt, Rt.data(), Rt.size() * 8));
    TRY(upload(e, e.gpp.a0, d->a0, (size_t)k * 8));
    TRY(gp_proj_prepare(e, k));
    TRY(gp_proj_coef_prepare(e, k));
    e.gpp.c_perp = d->c_perp; e.gpp.half_logdet_gamma = d->half_logdet_gamma;
    e.gpp.logdet = d->logdet ? 1 : 0;
    e.gpp.k = k;
    return CESX_OK;
}

int cesx_mh_phi(cesx_handle h, double* phi_host) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!phi_host) { e.err = "cesx_mh_phi: null pointer"; return CESX_EINVAL; }
    if (!e.mh.started) { e.err = "cesx_mh_phi: no start (cesx_mh_start / cesx_gp_start) has been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    CESX_HIP(hipDeviceSynchronize());
    CESX_HIP(hipMemcpy(phi_host, e.mh.phi, (size_t)e.J * 8, hipMemcpyDeviceToHost));
    return CESX_OK;
}

static int gp_check_mode(Engine& e, int mode, const double* mean, const double* var) {
    if (mode == CESX_GP_DENSE) {
        if (e.gpd.none()) { e.err = "cesx_gp: CESX_GP_DENSE needs a descriptor (cesx_gp_dense_set after cesx_set_problem)"; return CESX_ESTATE; }
        if (!mean || !var) { e.err = "cesx_gp: null pointer"; return CESX_EINVAL; }
        if (e.gp.n != e.gpd.k) { e.err = "cesx_gp: the emulator's n_gp differs from the descriptor's k"; return CESX_EINVAL; }
        return CESX_OK;
    }
    if (mode == CESX_GP_PROJ) {
        if (e.gpp.none()) { e.err = "cesx_gp: CESX_GP_PROJ needs a descriptor (cesx_gp_proj_set after cesx_set_problem)"; return CESX_ESTATE; }
        if (!mean || !var) { e.err = "cesx_gp: null pointer"; return CESX_EINVAL; }
        if (e.gp.n != e.gpp.k) { e.err = "cesx_gp: the emulator's n_gp differs from the descriptor's k"; return CESX_EINVAL; }
        return CESX_OK;
    }
    if (mode != CESX_GP_GAMMA && mode != CESX_GP_VAR && mode != CESX_GP_GAMMA_VAR) { e.err = "cesx_gp: unknown likelihood mode"; return CESX_EINVAL; }
    if (!mean || (mode != CESX_GP_GAMMA && !var)) { e.err = "cesx_gp: null pointer"; return CESX_EINVAL; }
    if (mode != CESX_GP_GAMMA && e.whiten) { e.err = "cesx_gp: the variance modes need a diagonal Gamma"; return CESX_EINVAL; }
    if (e.gp.n != e.n) { e.err = "cesx_gp: the emulator's n_gp differs from n_obs"; return CESX_EINVAL; }
    return CESX_OK;
}

int cesx_gp_start(cesx_handle h, int mode, const void* U, const double* mean, const double* var, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U) { e.err = "cesx_gp_start: null pointer"; return CESX_EINVAL; }
    if (e.mh.none() || !e.problem_set) { e.err = "cesx_gp_start: no proposal (cesx_mh_set_proposal after cesx_set_problem)"; return CESX_ESTATE; }
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_gp_start: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }
    TRY(gp_check_mode(e, mode, mean, var));
    SET_DEVICE(e);
    FLUSH(e);
    if (mode == CESX_GP_DENSE) TRY(launch_gp_score_dense(e, true, U, mean, var, nullptr, nullptr, 0u, (hipStream_t)stream));
    else if (mode == CESX_GP_PROJ) TRY(launch_gp_score_proj(e, true, U, mean, var, nullptr, nullptr, 0u, (hipStream_t)stream));
    else TRY(launch_gp_score(e, mode, true, U, mean, var, nullptr, nullptr, 0u, (hipStream_t)stream));
    e.mh.started = true;
    e.mh.steps = 0;
    return CESX_OK;
}

int cesx_gp_accept(cesx_handle h, int mode, uint64_t step_index, void* U, const void* P, const double* mean, const double* var,
                   const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !P) { e.err = "cesx_gp_accept: null pointer"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_gp_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_gp_accept: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }      // (the kind first: cesx_mh_accept)
    if (e.mh.none() || !e.mh.started) { e.err = "cesx_gp_accept: cesx_gp_start has not been called"; return CESX_ESTATE; }
    TRY(gp_check_mode(e, mode, mean, var));
    SET_DEVICE(e);
    FLUSH(e);
    if (mode == CESX_GP_DENSE) TRY(launch_gp_score_dense(e, false, P, mean, var, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    else if (mode == CESX_GP_PROJ) TRY(launch_gp_score_proj(e, false, P, mean, var, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    else TRY(launch_gp_score(e, mode, false, P, mean, var, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_gp_run(cesx_handle h, int mode, uint64_t step_index, int n_steps, int stride, int nugget, void* U, void* trace,
                const void* xi, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U) { e.err = "cesx_gp_run: null pointer"; return CESX_EINVAL; }
    if (n_steps < 1 || stride < 1) { e.err = "cesx_gp_run: n_steps and stride must be >= 1"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull || step_index + (uint64_t)n_steps > 0x80000000ull) { e.err = "cesx_gp_run: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    if (mode == CESX_GP_DENSE || mode == CESX_GP_PROJ) { e.err = "cesx_gp_run: CESX_GP_DENSE and CESX_GP_PROJ stay on the step path (cesx_mh_propose / cesx_gp_predict / cesx_gp_accept)"; return CESX_EINVAL; }
    if (mode != CESX_GP_GAMMA && mode != CESX_GP_VAR && mode != CESX_GP_GAMMA_VAR) { e.err = "cesx_gp_run: unknown likelihood mode"; return CESX_EINVAL; }
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_gp_run: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }
    if (!e.problem_set || e.mh.none() || e.gp.none() || !e.mh.started) { e.err = "cesx_gp_run: needs cesx_set_problem, cesx_mh_set_proposal, cesx_gp_set and a start (cesx_gp_start / cesx_mh_start)"; return CESX_ESTATE; }
    if (mode != CESX_GP_GAMMA && e.whiten) { e.err = "cesx_gp_run: the variance modes need a diagonal Gamma"; return CESX_EINVAL; }
    if (e.gp.n != e.n) { e.err = "cesx_gp_run: the emulator's n_gp differs from n_obs"; return CESX_EINVAL; }
    if (!gp_run_fits(e.p, e.gp.Jp, e.gp.n)) { e.err = "cesx_gp_run: the tile does not fit in LDS (256 (3 p + J_p + 2 n_gp) + 8192 bytes > 160 KiB); take the step path"; return CESX_EUNSUPPORTED; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_gp_run(e, mode, step_index, n_steps, stride, nugget != 0, U, trace, xi, logu, (hipStream_t)stream));
    e.mh.steps += (unsigned long long)n_steps;
    return CESX_OK;
}

int cesx_gp_predict_grad(cesx_handle h, const void* X, double* mean, double* var, double* dmean, double* dvar, int nugget,
                         void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!X || !mean || !dmean || (var == nullptr) != (dvar == nullptr)) { e.err = "cesx_gp_predict_grad: null pointer (var_dev and dvar_dev go together)"; return CESX_EINVAL; }
    if (e.gp.none()) { e.err = "cesx_gp_predict_grad: cesx_gp_set has not been called"; return CESX_ESTATE; }
    if (e.gp.matern12) { e.err = "cesx_gp_predict_grad: a Matern12 kernel is not differentiable at its training points"; return CESX_EUNSUPPORTED; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_gp_predict_grad(e, X, mean, var, dmean, dvar, nugget != 0, (hipStream_t)stream);
}

// ---- the Langevin step of gp_mh(chains=, update='langevin') (kernels_gpgrad.hip) ----

// an armed handle (cesx_mh_adapt_set) runs adaptation steps through cesx_mh_hmc_begin / _leap / _accept and cesx_gp_hmc_leap /
// _accept alone: every other step of the Langevin family would move the chains at a step the recursion does not see
static int adapt_refuses(Engine& e) {
    if (e.mh.ad_armed) { e.err = "the handle is armed for step-size adaptation (cesx_mh_adapt_set): its steps are cesx_mh_hmc_begin / _leap / _accept and cesx_gp_hmc_leap / _accept (cesx_gp_proj_hmc_leap / _accept); cesx_mh_adapt_read, then cesx_mh_set_proposal, ends the phase"; return CESX_ESTATE; }
    return CESX_OK;
}

// what every cesx_gp_langevin_* call needs before it looks at its own arguments; `started`: a cesx_gp_langevin_start too
static int langevin_check_state(Engine& e, bool started) {
    if (started) TRY(adapt_refuses(e));
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN) { e.err = "cesx_gp_langevin: no Langevin proposal (cesx_mh_set_proposal with CESX_MH_LANGEVIN after cesx_set_problem)"; return CESX_ESTATE; }
    if (e.gp.none()) { e.err = "cesx_gp_langevin: cesx_gp_set has not been called"; return CESX_ESTATE; }
    if (started && (!e.mh.started || e.mh.lin_started)) { e.err = "cesx_gp_langevin: cesx_gp_langevin_start has not been called"; return CESX_ESTATE; }
    return CESX_OK;
}

static int langevin_check_mode(Engine& e, int mode, const double* mean, const double* var, const double* dmean, const double* dvar) {
    if (mode == CESX_GP_DENSE || mode == CESX_GP_PROJ) { e.err = "cesx_gp_langevin: CESX_GP_DENSE and CESX_GP_PROJ have no gradient on the device"; return CESX_EINVAL; }
    if (mode != CESX_GP_GAMMA && mode != CESX_GP_VAR && mode != CESX_GP_GAMMA_VAR) { e.err = "cesx_gp_langevin: unknown likelihood mode"; return CESX_EINVAL; }
    if (!mean || !dmean || (mode != CESX_GP_GAMMA && (!var || !dvar))) { e.err = "cesx_gp_langevin: null pointer"; return CESX_EINVAL; }
    if (mode != CESX_GP_GAMMA && e.whiten) { e.err = "cesx_gp_langevin: the variance modes need a diagonal Gamma"; return CESX_EINVAL; }
    if (e.gp.n != e.n) { e.err = "cesx_gp_langevin: the emulator's n_gp differs from n_obs"; return CESX_EINVAL; }
    return CESX_OK;
}

int cesx_gp_langevin_start(cesx_handle h, int mode, const void* U, const double* mean, const double* var, const double* dmean,
                           const double* dvar, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(langevin_check_state(e, false));
    if (!U) { e.err = "cesx_gp_langevin_start: null pointer"; return CESX_EINVAL; }
    TRY(langevin_check_mode(e, mode, mean, var, dmean, dvar));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_gp_langevin(e, 0, mode, U, mean, var, dmean, dvar, nullptr, nullptr, nullptr, 0u, (hipStream_t)stream));
    e.mh.started = true;
    e.mh.lin_started = false;
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    e.mh.steps = 0;
    return CESX_OK;
}

int cesx_gp_langevin_propose(cesx_handle h, uint64_t step_index, const void* U, const void* xi, void* P, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(langevin_check_state(e, true));
    if (!U || !P) { e.err = "cesx_gp_langevin_propose: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_gp_langevin_propose: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_gp_langevin_propose: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    // the block stays in engine memory: the accept step needs it again
    if (xi) CESX_HIP(hipMemcpyAsync(e.mh.xi, xi, (size_t)e.p * (size_t)e.J * e.esz, hipMemcpyDeviceToDevice, s));
    else TRY(launch_noise(e, mh_step_word(step_index), e.mh.xi, s));
    TRY(launch_gp_langevin(e, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, const_cast<void*>(U), P, nullptr, 0u, s));
    e.mh.lv_proposed = true; e.mh.hm_begun = false;      // (the block of a trajectory in flight is overwritten)
    return CESX_OK;
}

int cesx_gp_langevin_accept(cesx_handle h, int mode, uint64_t step_index, void* U, const void* P, const double* mean,
                            const double* var, const double* dmean, const double* dvar, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(langevin_check_state(e, true));
    if (!e.mh.lv_proposed) { e.err = "cesx_gp_langevin_accept: no cesx_gp_langevin_propose since the start or the last accept"; return CESX_ESTATE; }
    if (!U || !P) { e.err = "cesx_gp_langevin_accept: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_gp_langevin_accept: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_gp_langevin_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    TRY(langevin_check_mode(e, mode, mean, var, dmean, dvar));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_gp_langevin(e, 2, mode, P, mean, var, dmean, dvar, U, nullptr, logu, mh_step_word(step_index), (hipStream_t)stream));
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_profile_enable(cesx_handle h, int on) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (on < 0 || on > 4) { e.err = "cesx_profile_enable: bad mode"; return CESX_EINVAL; }
    e.profile = on != 0;
    e.profile_gap_only = on == 2;
    e.profile_only = on == 3 ? 1 : on == 4 ? 0 : -1;      // 3: the update launches alone, 4: the moments launches alone
    if (e.profile) {
        SET_DEVICE(e);
        while (e.prof_pool.size() < 512) {        // created up front: no event creation in a timed region
            hipEvent_t ev = nullptr;
            CESX_HIP(hipEventCreate(&ev));
            e.prof_pool.push_back(ev);
        }
    }
    return CESX_OK;
}

int cesx_profile_read(cesx_handle h, int which, double* total_ms, int* launches) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (which < 0 || which > 1 || !total_ms || !launches) { e.err = "cesx_profile_read: bad argument"; return CESX_EINVAL; }
    SET_DEVICE(e);
    double tot = 0.0;
    int cnt = 0;
    for (auto& pr : e.prof_ev[which]) {
        float ms = 0.f;
        if (pr.first && pr.second) {               // (a pair of a gap-only step has one event only: recycled, not counted)
            CESX_HIP(hipEventSynchronize(pr.second));
            CESX_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
            tot += ms;
            ++cnt;
        }
        if (pr.first) e.prof_pool.push_back(pr.first);
        if (pr.second) e.prof_pool.push_back(pr.second);
    }
    e.prof_ev[which].clear();
    e.prof_tag[which].clear();
    *total_ms = tot;
    *launches = cnt;
    return CESX_OK;
}

int cesx_copy_cols_async(cesx_handle h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                      size_t height, int to_device, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!dst || !src || width_bytes == 0 || height == 0 || dpitch < width_bytes || spitch < width_bytes) {
        e.err = "cesx_copy_cols_async: bad argument";
        return CESX_EINVAL;
    }
    SET_DEVICE(e);
    CESX_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height,
                              to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, (hipStream_t)stream));
    return CESX_OK;
}

int cesx_profile_gap(cesx_handle h, double* gap_ms) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!gap_ms) { e.err = "cesx_profile_gap: null pointer"; return CESX_EINVAL; }
    *gap_ms = -1.0;
    if (e.prof_ev[0].empty() || e.prof_ev[1].empty()) return CESX_OK;
    SET_DEVICE(e);
    hipEvent_t gram_end = e.prof_ev[0].back().second, upd_start = e.prof_ev[1].back().first;
    if (!gram_end || !upd_start) return CESX_OK;
    // both events must belong to ONE step: a step without a second moments launch (the linear-map fast path, a shard
    // whose second part is empty) leaves an older Gram event at the back -- no gap then (-1)
    if (e.prof_tag[0].empty() || e.prof_tag[1].empty() || e.prof_tag[0].back() != e.prof_tag[1].back()) return CESX_OK;
    CESX_HIP(hipEventSynchronize(upd_start));
    float ms = 0.f;
    CESX_HIP(hipEventElapsedTime(&ms, gram_end, upd_start));
    *gap_ms = ms;
    return CESX_OK;
}

int cesx_profile_clock(cesx_handle h, double* clock_ghz) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!clock_ghz) { e.err = "cesx_profile_clock: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    CESX_HIP(hipDeviceSynchronize());
    long long t[4] = {0, 0, 0, 0};         // {s_memtime, s_memrealtime} at the start, then at the end, of one wave
    CESX_HIP(hipMemcpy(t, e.d_clk, 32, hipMemcpyDeviceToHost));
    *clock_ghz = t[3] > t[1] ? (double)(t[2] - t[0]) / (double)(t[3] - t[1]) * 0.1 : 0.0;      // s_memrealtime ticks at 100 MHz
    return CESX_OK;
}

int cesx_calibrate_mfma(cesx_handle h, double target_ms, double* tflops, double* clock_ghz, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!(target_ms > 0.0) || target_ms > 1000.0 || !tflops) { e.err = "cesx_calibrate_mfma: bad argument"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_calibrate(e, target_ms, tflops, clock_ghz, (hipStream_t)stream);
}

// Host-only: plan_dense for an engine state and a launch given as 23 facts (include/cesx.h), the plan's 13 fields as integers.
int cesx_debug_dense_plan(const int32_t* f, int32_t* plan) {
    if (!f || !plan || f[0] < CESX_UPDATE_EKS || f[0] > CESX_UPDATE_ALDI_CONSTANT || f[1] < CESX_TS_DEFAULT || f[1] > CESX_TS_MIX ||
        f[2] < 0 || f[2] > 2) return -1;
    try {
        Engine e;
        cesx_step_params prm{};
        prm.update = f[0]; prm.time_step = f[1];
        e.cfg.dtype = f[4] ? CESX_F64 : CESX_F32;
        e.p = f[5] ? 256 : 257;                          // potrf_ld(p) <= 256 or not
        e.kp = 16; e.kn = 32; e.ktot = 64;               // (any three that tell kp, kp + kn and ktot apart)
        e.diag_sigma = f[6]; e.chain = f[7]; e.hkfree_ok = f[8]; e.update_v2 = f[9];
        e.d_Wq = f[10] ? &e : nullptr;                   // (never dereferenced)
        e.fac.inflight = f[11]; e.fac.fused_center = f[12]; e.fac.img = f[13]; e.fac.signals = f[14]; e.fac.image_only = f[15];
        e.poll_join_ok = f[16];
        e.J = 1; e.Jg = f[17] ? 2 : 1;
        e.side = reinterpret_cast<hipStream_t>(&e.side);
        e.fuse_center_ok = f[20]; e.fuse_center_auto = f[21]; e.gram_b_short = f[22];
        const DenseLaunch L{.prm = &prm, .phase = (DensePhase)f[2], .s = f[18] ? e.side : nullptr, .upd_ok = f[3] != 0};
        const DensePlan P = plan_dense(e, L, f[19] != 0);
        const int32_t out[13] = {(int)P.route, (int)P.tail, (int)P.join, (int)P.upart, P.center, (int)P.factor, P.refactor, P.gemm_M,
                                 P.spectral, P.gain_inverse, P.eks_inverse, (int)P.mode, P.ktot};
        std::copy(out, out + 13, plan);
        return 0;
    } catch (...) { return -2; }
}

// Host-only: builds the Gram work partition a handle of this shape would use (no device needed) and checks its
// invariants.  Returns the number of violations; info[0..5] = {types, workgroups, blocks, busiest workgroup's
// tiles x blocks-per-SIMD, max staged row blocks, slabs}.
int cesx_debug_gram_plan(int p, int n_obs, int dtype, int part, int wg_budget, long long J_local, int* info) {
    if (p < 1 || n_obs < 1 || (dtype != CESX_F32 && dtype != CESX_F64) || part < 0 || part > 1 || J_local < 1) return -1;
    try {
        const int P = p + n_obs, tile = gram_tile(dtype), kt = gram_kt(dtype), nbw = gram_nbw(dtype);
        const int pbU = (p + tile - 1) / tile;
        const long long ntiles = (J_local + kt - 1) / kt;
        const GramPlan pl = make_gram_plan(P, tile, nbw, gram_max_stage_rows(), part + 1, pbU, 1, wg_budget, ntiles);
        const int nbr = (P + tile - 1) / tile;
        int bad = 0;
        std::vector<int> seen((size_t)nbr * nbr, 0);
        long long wgs = 0, slabs = 0, worst = 0;
        if ((int)pl.type_hdr.size() != pl.ntypes * 8) ++bad;
        for (int t = 0; t < pl.ntypes && !bad; ++t) {
            const int* h = &pl.type_hdr[(size_t)t * 8];
            const int nrb = h[0], rows_off = h[1], blocks_off = h[2], nblk = h[3], wg0 = h[4], nsl = h[5];
            if (nrb < 1 || nrb * tile > gram_max_stage_rows() || nrb > pl.max_rb) ++bad;
            if (nsl < 1 || (long long)nsl > std::max<long long>(1, ntiles)) ++bad;
            if (wg0 != wgs || h[6] != slabs) ++bad;
            wgs += nsl; slabs += (long long)nsl * nblk;
            const long long tps = (ntiles + nsl - 1) / nsl;
            if (tps * nsl < ntiles) ++bad;
            int per_simd[4] = {0, 0, 0, 0}, cnt = 0;
            for (int w = 0; w < 16; ++w)
                for (int b = 0; b < nbw; ++b) {
                    const int* e3 = &pl.wblk[((size_t)blocks_off + (size_t)w * nbw + b) * 3];
                    if (e3[0] < 0) continue;
                    if (e3[0] >= nrb || e3[1] >= nrb || e3[2] < 0 || e3[2] >= nblk) { ++bad; continue; }
                    const int R = pl.rows[rows_off + e3[0]] & 0xffff, C = pl.rows[rows_off + e3[1]] & 0xffff;
                    if (R >= nbr || C > R) { ++bad; continue; }
                    ++seen[(size_t)R * nbr + C];
                    ++per_simd[w & 3]; ++cnt;
                }
            if (cnt != nblk) ++bad;
            const int mx = std::max(std::max(per_simd[0], per_simd[1]), std::max(per_simd[2], per_simd[3]));
            worst = std::max(worst, tps * mx);
        }
        int nwant = 0;
        for (int R = 0; R < nbr; ++R)
            for (int C = 0; C <= R; ++C) {
                const bool uu = R < pbU && C < pbU;
                const bool wanted = part == 0 ? uu : !uu;
                nwant += wanted ? 1 : 0;
                if (seen[(size_t)R * nbr + C] != (wanted ? 1 : 0)) ++bad;      // every wanted block exactly once, no other
            }
        if (nwant != pl.nblocks) ++bad;
        if (wgs != pl.total_wgs || slabs != pl.total_slabs) ++bad;
        if (pl.nblocks > 0 && pl.total_wgs > std::max(wg_budget, pl.ntypes)) ++bad;
        if (info) { info[0] = pl.ntypes; info[1] = pl.total_wgs; info[2] = pl.nblocks; info[3] = (int)worst; info[4] = pl.max_rb; info[5] = pl.total_slabs; }
        return bad;
    } catch (...) {
        return -2;
    }
}

int cesx_debug_dense(cesx_handle h, double* ubar, double* gbar, double* C, double* L, double* K, double* M) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());
    if (L) {          // (K3 through the Cholesky factor: a step that kept L in its coefficient image only -- factored again here)
        TRY(ensure_factor(e, nullptr));
        CESX_HIP(hipDeviceSynchronize());
    }
    const size_t p = e.p, n = e.n;
    if (ubar) CESX_HIP(hipMemcpy(ubar, e.d_ubar, p * 8, hipMemcpyDeviceToHost));
    if (gbar) {
        CESX_HIP(hipMemcpy(gbar, e.d_gbar, n * 8, hipMemcpyDeviceToHost));
        if (e.whiten) {          // the engine holds the mean of the WHITENED data: gbar = L_Gamma gbar~
            std::vector<double> t(gbar, gbar + n);
            for (size_t i = 0; i < n; ++i) {
                double a = 0.0;
                for (size_t k = 0; k <= i; ++k) a += e.h_LG[i * n + k] * t[k];
                gbar[i] = a;
            }
        }
    }
    if (C) CESX_HIP(hipMemcpy(C, e.d_C, p * p * 8, hipMemcpyDeviceToHost));
    if (L) {
        const size_t ld = potrf_ld(e.p);
        CESX_HIP(hipMemcpy2D(L, p * 8, e.d_L, ld * 8, p * 8, p, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < p; ++i)
            for (size_t j = i + 1; j < p; ++j) L[i * p + j] = 0.0;     // the factor's upper triangle is not stored
    }
    if (K) {
        CESX_HIP(hipMemcpy(K, e.d_K, p * n * 8, hipMemcpyDeviceToHost));
        if (e.whiten) {          // K~ = C_ug~ = C_ug L^{-T}; the reference's gain C_ug Gamma^{-1} = K~ L^{-1}
            std::vector<double> t(K, K + p * n);
            for (size_t i = 0; i < p; ++i)
                for (size_t j = 0; j < n; ++j) {
                    double a = 0.0;
                    for (size_t k = j; k < n; ++k) a += t[i * n + k] * e.h_Li[k * n + j];
                    K[i * n + j] = a;
                }
        }
    }
    if (M) CESX_HIP(hipMemcpy(M, e.d_M, p * p * 8, hipMemcpyDeviceToHost));
    return CESX_OK;
}


// ---- Emulate: training the GPs, batched likelihood and gradient (ces_amd/emulate.py train_gps(device=True); kernels_gpfit.hip) ----

static int gpfit_alloc(Engine& e, const cesx_gpfit_desc* d, int Jp, int nl, int ntheta, int ntile) {
    const size_t n = (size_t)d->n_gp, Jt = (size_t)d->J_t, p = (size_t)e.p, J2 = (size_t)Jp * Jp;
    TRY_BUF(e.gf.X.alloc(Jt * p * 8)); TRY(upload(e, e.gf.X, d->X, Jt * p * 8));
    TRY_BUF(e.gf.Y.alloc(n * Jt * 8)); TRY(upload(e, e.gf.Y, d->Y, n * Jt * 8));
    TRY_BUF(e.gf.Xs.alloc(n * Jp * p * 8));
    TRY_BUF(e.gf.r.alloc(n * Jp * 8)); TRY_BUF(e.gf.t.alloc(n * Jp * 8)); TRY_BUF(e.gf.alpha.alloc(n * Jp * 8));
    TRY_BUF(e.gf.A.alloc(n * J2 * 8)); TRY_BUF(e.gf.W.alloc(n * J2 * 8)); TRY_BUF(e.gf.Ki.alloc(n * J2 * 8));
    TRY_BUF(e.gf.Ld.alloc(n * Jp * 16 * 8));
    TRY_BUF(e.gf.part.alloc(n * ntile * (size_t)(nl + 2) * 8));
    TRY_BUF(e.gf.theta.alloc(n * ntheta * 8)); TRY_BUF(e.gf.out.alloc(n * (size_t)(2 + ntheta) * 8));
    TRY_BUF(e.gf.idx.alloc(n * 4)); TRY_BUF(e.gf.status.alloc(n * 4));
    return CESX_OK;
}

// Failure rule: the old fit problem is dropped before the arguments are looked at (a bad descriptor drops it too); a failed
// allocation or upload leaves none and nothing allocated.
int cesx_gpfit_set(cesx_handle h, const cesx_gpfit_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    e.gf.n = 0;                                // whatever fails below, the handle is left without a fit problem
    if (!d || d->struct_bytes != sizeof(cesx_gpfit_desc)) { e.err = "cesx_gpfit_set: bad cesx_gpfit_desc"; return CESX_EINVAL; }
    if (!d->X || !d->Y) { e.err = "cesx_gpfit_set: null pointer"; return CESX_EINVAL; }
    if (d->n_gp < 1 || d->n_gp > 65535 || d->J_t < 1 || d->J_t > 16384) { e.err = "cesx_gpfit_set: 1 <= n_gp <= 65535 and 1 <= J_t <= 16384"; return CESX_EINVAL; }
    if (d->family < 0 || d->family > 3) { e.err = "cesx_gpfit_set: unknown kernel family"; return CESX_EINVAL; }
    if (d->mean < CESX_GPFIT_MEAN_ZERO || d->mean > CESX_GPFIT_MEAN_LINEAR) { e.err = "cesx_gpfit_set: unknown mean kind"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (an evaluation of the old problem may still be in flight)
    e.gf.drop();
    const int Jp = (d->J_t + 15) / 16 * 16, nl = d->ard ? e.p : 1;
    const int ntheta = nl + 2 + (d->mean == CESX_GPFIT_MEAN_ZERO ? 0 : d->mean == CESX_GPFIT_MEAN_CONSTANT ? 1 : e.p + 1);
    const int ntile = gpfit_tiles(Jp);
    const int rc = gpfit_alloc(e, d, Jp, nl, ntheta, ntile);
    if (rc != CESX_OK) { e.gf.drop(); return rc; }          // nothing is committed before everything is
    e.gf.Jt = d->J_t; e.gf.Jp = Jp; e.gf.family = d->family; e.gf.ard = d->ard ? 1 : 0; e.gf.mean = d->mean;
    e.gf.nl = nl; e.gf.ntheta = ntheta; e.gf.ntile = ntile;
    e.gf.h_out.assign((size_t)d->n_gp * (2 + ntheta), 0.0);
    e.gf.n = d->n_gp;
    return CESX_OK;
}

int cesx_gpfit_ntheta(cesx_handle h) {
    if (!h) return -1;
    Engine& e = *reinterpret_cast<Engine*>(h);
    return e.gf.none() ? -1 : e.gf.ntheta;
}

int cesx_gpfit_eval(cesx_handle h, int n_active, const int32_t* idx, const double* theta, double* lml, double* grad,
                    int32_t* status, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.gf.none()) { e.err = "cesx_gpfit_eval: cesx_gpfit_set has not been called"; return CESX_ESTATE; }
    if (!idx || !theta || !lml || !grad || !status) { e.err = "cesx_gpfit_eval: null pointer"; return CESX_EINVAL; }
    if (n_active < 1 || n_active > e.gf.n) { e.err = "cesx_gpfit_eval: 1 <= n_active <= n_gp"; return CESX_EINVAL; }
    {
        std::vector<char> seen((size_t)e.gf.n, 0);          // (two entries for one GP would share its workspace)
        for (int i = 0; i < n_active; ++i) {
            if (idx[i] < 0 || idx[i] >= e.gf.n || seen[(size_t)idx[i]]) { e.err = "cesx_gpfit_eval: idx out of range or repeated"; return CESX_EINVAL; }
            seen[(size_t)idx[i]] = 1;
        }
    }
    SET_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t nt = (size_t)e.gf.ntheta, no = 2 + nt;
    CESX_HIP(hipMemcpyAsync(e.gf.idx, idx, (size_t)n_active * 4, hipMemcpyHostToDevice, s));
    CESX_HIP(hipMemcpyAsync(e.gf.theta, theta, (size_t)n_active * nt * 8, hipMemcpyHostToDevice, s));
    TRY(launch_gpfit_eval(e, n_active, s));
    CESX_HIP(hipMemcpyAsync(e.gf.h_out.data(), e.gf.out, (size_t)n_active * no * 8, hipMemcpyDeviceToHost, s));
    CESX_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n_active; ++i) {
        const double* o = e.gf.h_out.data() + (size_t)i * no;
        lml[i] = o[0];
        status[i] = o[1] == 0.0 ? CESX_OK : CESX_ENOTPD;
        std::memcpy(grad + (size_t)i * nt, o + 2, nt * 8);
    }
    return CESX_OK;
}

int cesx_gpfit_factors(cesx_handle h, int i, double* alpha, double* Li) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.gf.none()) { e.err = "cesx_gpfit_factors: cesx_gpfit_set has not been called"; return CESX_ESTATE; }
    if (i < 0 || i >= e.gf.n || !alpha || !Li) { e.err = "cesx_gpfit_factors: bad GP index or null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    const size_t Jt = (size_t)e.gf.Jt, Jp = (size_t)e.gf.Jp;
    std::vector<double> W(Jp * Jp);
    CESX_HIP(hipDeviceSynchronize());
    CESX_HIP(hipMemcpy(alpha, e.gf.alpha + (size_t)i * Jp, Jt * 8, hipMemcpyDeviceToHost));
    CESX_HIP(hipMemcpy(W.data(), e.gf.W + (size_t)i * Jp * Jp, Jp * Jp * 8, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < Jt; ++r)                         // L^{-1} = W^T: the engine keeps the upper-triangular L^{-T}
        for (size_t c = 0; c < Jt; ++c) Li[r * Jt + c] = c <= r ? W[c * Jp + r] : 0.0;
    return CESX_OK;
}

// ---- Darcy forward map over the columns (ces_amd/darcy.py; kernels_darcy.hip, kernels_darcy_stream.hip) ----

// Failure rule: an argument error leaves the OLD map; behind the synchronise there is none until everything is uploaded.
// One body for both kinds: `who` names the entry point in the messages; only the K limit and the workspace differ.
static int darcy_install(Engine& e, const cesx_darcy_desc* d, const char* who, bool streamed, int max_workgroups) {
    auto fail = [&](const char* what) { e.err = std::string(who) + ": " + what; return CESX_EINVAL; };
    if (!d || d->struct_bytes != sizeof(cesx_darcy_desc)) return fail("bad cesx_darcy_desc");
    if (!d->coef || !d->scatter || !d->D || !d->S || !d->R || !d->obs_index) return fail("null pointer");
    if (d->K < 4) return fail("K < 4 (a not-a-knot spline needs four points)");
    if (!streamed && d->K > 16) return fail("K > 16 (the working band of one particle no longer fits in LDS)");
    if (streamed && d->K > darcy_stream_kmax())
        return fail(("K > " + std::to_string(darcy_stream_kmax()) + " (the live window of one particle no longer fits in LDS)").c_str());
    if (streamed && max_workgroups < 0) return fail("max_workgroups < 0");
    const int K = d->K, KK = K * K, p = e.p, n = e.n;
    if (d->p != p || d->n_obs != n) return fail("p / n_obs differ from the handle's");
    if (p > KK) return fail("p exceeds K^2");
    std::vector<int> idx((size_t)p + n);
    std::vector<char> seen((size_t)KK, 0);
    for (int q = 0; q < p; ++q) {
        const int s = d->scatter[q];
        if (s < 0 || s >= KK || seen[s]) return fail("scatter index out of range or repeated");
        seen[s] = 1; idx[q] = s;
    }
    for (int k = 0; k < n; ++k) {
        const int o = d->obs_index[k];
        if (o < 0 || o >= KK) return fail("obs_index out of range");
        idx[(size_t)p + k] = o;
    }
    SET_DEVICE(e);
    CESX_HIP(hipDeviceSynchronize());          // (the old image may be read by launches still in flight)
    e.dc.drop();
    int slots = 0;
    if (streamed) {
        // slots = min(J, max_workgroups or the automatic grid, CESX_DARCY_WS_CAP / bytes per slot), at least one
        int auto_grid = 0;
        TRY(darcy_stream_prepare(e, K, &auto_grid));
        const size_t per = darcy_stream_slot_bytes(K);
        long long s = std::min<long long>(e.J, max_workgroups > 0 ? max_workgroups : auto_grid);
        s = std::min<long long>(s, (long long)(CESX_DARCY_WS_CAP / per));
        slots = (int)std::max<long long>(s, 1);
        TRY_BUF(e.dc.ws.alloc((size_t)slots * per, false));
    } else {
        TRY(darcy_prepare(e, K));
        TRY(darcy_grad_prepare(e, K));
    }
    TRY_BUF(e.dc.mat.alloc((size_t)4 * KK * 8));
    TRY_BUF(e.dc.idx.alloc(idx.size() * 4));
    const double* mats[4] = {d->coef, d->D, d->S, d->R};
    for (int k = 0; k < 4; ++k) TRY(upload(e, e.dc.mat + (size_t)k * KK, mats[k], (size_t)KK * 8));
    TRY(upload(e, e.dc.idx, idx.data(), idx.size() * 4));
    e.dc.streamed = streamed; e.dc.slots = slots;
    e.dc.K = K;
    return CESX_OK;
}

int cesx_darcy_set(cesx_handle h, const cesx_darcy_desc* d) {
    if (!h) return CESX_EINVAL;
    return darcy_install(*reinterpret_cast<Engine*>(h), d, "cesx_darcy_set", false, 0);
}

int cesx_darcy_set_streamed(cesx_handle h, const cesx_darcy_desc* d, int max_workgroups) {
    if (!h) return CESX_EINVAL;
    return darcy_install(*reinterpret_cast<Engine*>(h), d, "cesx_darcy_set_streamed", true, max_workgroups);
}

size_t cesx_darcy_workspace_bytes(cesx_handle h) {
    if (!h) return 0;
    const Engine& e = *reinterpret_cast<Engine*>(h);
    return e.dc.none() || !e.dc.streamed ? 0 : e.dc.ws.bytes;
}

int cesx_darcy_apply(cesx_handle h, const void* U, void* G, int32_t* status, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G) { e.err = "cesx_darcy_apply: null pointer"; return CESX_EINVAL; }
    if (e.dc.none()) { e.err = "cesx_darcy_apply: cesx_darcy_set has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    if (e.dc.streamed) return launch_darcy_stream(e, U, G, status, (hipStream_t)stream);
    return launch_darcy(e, U, G, status, (hipStream_t)stream);
}

size_t cesx_darcy_grad_lds_bytes(int K) { return K < 4 || K > 16 ? 0 : darcy_grad_lds_bytes(K); }

int cesx_darcy_grad(cesx_handle h, const void* U, double* G, double* phid, double* dphi, int32_t* status, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G || !phid || !dphi) { e.err = "cesx_darcy_grad: null pointer"; return CESX_EINVAL; }
    if (e.dc.none()) { e.err = "cesx_darcy_grad: cesx_darcy_set has not been called"; return CESX_ESTATE; }
    if (!e.problem_set) { e.err = "cesx_darcy_grad: cesx_set_problem has not been called (the misfit needs y and Gamma)"; return CESX_ESTATE; }
    if (e.dc.streamed) { e.err = "cesx_darcy_grad: the installed map is a streamed one (cesx_darcy_set_streamed keeps no multipliers); install it with cesx_darcy_set"; return CESX_EUNSUPPORTED; }
    SET_DEVICE(e);
    TRY_BUF(e.dc.gscr.ensure((size_t)e.J * 2 * (size_t)e.n * 8));
    return launch_darcy_grad(e, U, G, phid, dphi, status, (hipStream_t)stream);
}

// ---- Lorenz '96 forward map over the columns (ces_amd/models.py; kernels_l96.hip) ----

// Failure rule: ANY failure leaves the OLD map installed -- the new sample times are allocated and uploaded before the old are released.
int cesx_lorenz_set(cesx_handle h, const cesx_l96_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != sizeof(cesx_l96_desc)) { e.err = "cesx_lorenz_set: bad cesx_l96_desc"; return CESX_EINVAL; }
    if (d->n_slow < 4) { e.err = "cesx_lorenz_set: n_slow < 4 (the slow tendencies reach from k - 2 to k + 1)"; return CESX_EINVAL; }
    if (d->n_fast < 1) { e.err = "cesx_lorenz_set: n_fast < 1"; return CESX_EINVAL; }
    if ((long long)d->n_slow * ((long long)d->n_fast + 1) > 448) { e.err = "cesx_lorenz_set: n_state = n_slow (n_fast + 1) > 448"; return CESX_EINVAL; }
    if (d->p != e.p || d->n_obs != e.n) { e.err = "cesx_lorenz_set: p / n_obs differ from the handle's"; return CESX_EINVAL; }
    if (d->stat_mode < 0 || d->stat_mode > 2) { e.err = "cesx_lorenz_set: stat_mode is not 0, 1 or 2"; return CESX_EINVAL; }
    if (d->n_obs != (d->stat_mode == 0 ? 5 * d->n_slow : 5)) { e.err = "cesx_lorenz_set: n_obs is not 5 n_slow (stat_mode 0) / 5 (stat_mode 1, 2)"; return CESX_EINVAL; }
    if (d->stat_mode == 2 && d->n_slow < 8) { e.err = "cesx_lorenz_set: stat_mode 2 reads slow index 7, n_slow < 8"; return CESX_EINVAL; }
    for (int k = 0; k < 4; ++k) {
        if (d->par_row[k] < -1 || d->par_row[k] >= e.p) { e.err = "cesx_lorenz_set: par_row out of range"; return CESX_EINVAL; }
        for (int m = 0; m < k; ++m)
            if (d->par_row[k] >= 0 && d->par_row[k] == d->par_row[m]) { e.err = "cesx_lorenz_set: par_row repeated"; return CESX_EINVAL; }
        if (d->par_row[k] < 0 && !std::isfinite(d->par_fixed[k])) { e.err = "cesx_lorenz_set: a fixed parameter is not finite"; return CESX_EINVAL; }
    }
    if (!(d->T > 0.0) || !(d->max_step > 0.0) || !(d->rtol > 0.0) || !(d->atol > 0.0) || !std::isfinite(d->T) || !std::isfinite(d->rtol)
        || !std::isfinite(d->atol)) {
        e.err = "cesx_lorenz_set: T, max_step, rtol and atol must be positive"; return CESX_EINVAL;
    }
    if (d->n_t < 2 || !d->t) { e.err = "cesx_lorenz_set: no sample times"; return CESX_EINVAL; }
    for (int k = 0; k < d->n_t; ++k)
        if (!(d->t[k] >= 0.0 && d->t[k] <= d->T) || (k && d->t[k] < d->t[k - 1])) {
            e.err = "cesx_lorenz_set: t is not non-decreasing within [0, T]"; return CESX_EINVAL;
        }
    if (d->spinup_samples < 0 || d->window_samples < 1 || d->n_t - 1 - d->spinup_samples < d->window_samples
        || (d->n_t - 1 - d->spinup_samples) % d->window_samples != 0) {
        e.err = "cesx_lorenz_set: n_t - 1 - spinup_samples is not a positive multiple of window_samples"; return CESX_EINVAL;
    }
    if (d->max_attempts < 1) { e.err = "cesx_lorenz_set: max_attempts < 1"; return CESX_EINVAL; }
    SET_DEVICE(e);
    CESX_HIP(hipDeviceSynchronize());          // (the old sample times may be read by launches still in flight)
    DevBuf<double> tnew;
    TRY_BUF(tnew.alloc((size_t)d->n_t * 8));
    TRY(upload(e, tnew, d->t, (size_t)d->n_t * 8));
    e.l9.t = std::move(tnew);
    e.l9.desc = *d;
    e.l9.desc.t = nullptr;
    return CESX_OK;
}

int cesx_lorenz_apply(cesx_handle h, const void* U, const double* W_in, void* G, double* W_out, int32_t* info, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !W_in || !G || !W_out) { e.err = "cesx_lorenz_apply: null pointer"; return CESX_EINVAL; }
    if (G == U) { e.err = "cesx_lorenz_apply: G must not alias U"; return CESX_EINVAL; }
    if (e.l9.none()) { e.err = "cesx_lorenz_apply: cesx_lorenz_set has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return launch_l96(e, U, W_in, G, W_out, info, (hipStream_t)stream);
}

// ---- Lorenz '63 forward map over the columns (ces_amd/models.py; kernels_l63.hip) ----

// Failure rule as cesx_lorenz_set's: ANY failure leaves the OLD map installed.
int cesx_lorenz_three_set(cesx_handle h, const cesx_l63_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != sizeof(cesx_l63_desc)) { e.err = "cesx_lorenz_three_set: bad cesx_l63_desc"; return CESX_EINVAL; }
    if (e.n != 9) { e.err = "cesx_lorenz_three_set: the handle's n_obs is not 9 (x, y, z, x^2, y^2, z^2, xy, xz, yz)"; return CESX_EINVAL; }
    for (int k = 0; k < 3; ++k) {
        if (d->par_row[k] < -1 || d->par_row[k] >= e.p) { e.err = "cesx_lorenz_three_set: par_row out of range"; return CESX_EINVAL; }
        for (int m = 0; m < k; ++m)
            if (d->par_row[k] >= 0 && d->par_row[k] == d->par_row[m]) { e.err = "cesx_lorenz_three_set: par_row repeated"; return CESX_EINVAL; }
        if (d->par_row[k] < 0 && !std::isfinite(d->par_fixed[k])) { e.err = "cesx_lorenz_three_set: a fixed parameter is not finite"; return CESX_EINVAL; }
    }
    if (!std::isfinite(d->t0) || !std::isfinite(d->T) || !(d->t0 < d->T)) { e.err = "cesx_lorenz_three_set: t0 < T must be finite"; return CESX_EINVAL; }
    if (!(d->max_step > 0.0) || !(d->rtol > 0.0) || !(d->atol > 0.0) || !std::isfinite(d->rtol) || !std::isfinite(d->atol)) {
        e.err = "cesx_lorenz_three_set: max_step, rtol and atol must be positive"; return CESX_EINVAL;
    }
    if (d->n_t < 2 || !d->t) { e.err = "cesx_lorenz_three_set: no sample times"; return CESX_EINVAL; }
    for (int k = 0; k < d->n_t; ++k)
        if (!(d->t[k] >= d->t0 && d->t[k] <= d->T) || (k && d->t[k] < d->t[k - 1])) {
            e.err = "cesx_lorenz_three_set: t is not non-decreasing within [t0, T]"; return CESX_EINVAL;
        }
    if (d->window_samples < 1 || (d->n_t - 1) % d->window_samples != 0) {
        e.err = "cesx_lorenz_three_set: n_t - 1 is not a positive multiple of window_samples"; return CESX_EINVAL;
    }
    if (d->max_attempts < 1) { e.err = "cesx_lorenz_three_set: max_attempts < 1"; return CESX_EINVAL; }
    SET_DEVICE(e);
    CESX_HIP(hipDeviceSynchronize());          // (the old sample times may be read by launches still in flight)
    DevBuf<double> tnew;
    TRY_BUF(tnew.alloc((size_t)d->n_t * 8));
    TRY(upload(e, tnew, d->t, (size_t)d->n_t * 8));
    e.l6.t = std::move(tnew);
    e.l6.desc = *d;
    e.l6.desc.t = nullptr;
    return CESX_OK;
}

int cesx_lorenz_three_apply(cesx_handle h, const void* U, const double* W_in, void* G, double* W_out, int32_t* info, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !W_in || !G || !W_out) { e.err = "cesx_lorenz_three_apply: null pointer"; return CESX_EINVAL; }
    if (G == U) { e.err = "cesx_lorenz_three_apply: G must not alias U"; return CESX_EINVAL; }
    if (e.l6.none()) { e.err = "cesx_lorenz_three_apply: cesx_lorenz_three_set has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return launch_l63(e, U, W_in, G, W_out, info, (hipStream_t)stream);
}

// ---- Closed-form maps over the columns and their fused chain kernel (ces_amd/utils.py; kernels_maps.hip) ----

// Failure rule: ANY failure leaves the OLD map installed.  The descriptor travels by value: nothing in flight reads it.
int cesx_map_set(cesx_handle h, const cesx_map_desc* d) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != (int)sizeof(cesx_map_desc)) { e.err = "cesx_map_set: bad cesx_map_desc"; return CESX_EINVAL; }
    if (d->kind != CESX_MAP_ELLIPTIC && d->kind != CESX_MAP_BANANA && d->kind != CESX_MAP_EXP) { e.err = "cesx_map_set: unknown map kind"; return CESX_EINVAL; }
    if (d->kind != CESX_MAP_EXP) {
        if (e.p != 2 || e.n != 2) { e.err = "cesx_map_set: the elliptic and the banana map need p = n_obs = 2"; return CESX_EINVAL; }
        if (!std::isfinite(d->prm[0]) || !std::isfinite(d->prm[1])) { e.err = "cesx_map_set: a parameter is not finite"; return CESX_EINVAL; }
        if (d->kind == CESX_MAP_BANANA && d->prm[0] == 0.0) { e.err = "cesx_map_set: banana needs a != 0"; return CESX_EINVAL; }
    }
    e.mp.desc = *d;
    return CESX_OK;
}

int cesx_map_apply(cesx_handle h, const void* U, void* G, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G) { e.err = "cesx_map_apply: null pointer"; return CESX_EINVAL; }
    if (e.mp.none()) { e.err = "cesx_map_apply: cesx_map_set has not been called"; return CESX_ESTATE; }
    if (G == U && e.mp.desc.kind != CESX_MAP_EXP) { e.err = "cesx_map_apply: G must not alias U"; return CESX_EINVAL; }
    SET_DEVICE(e);
    return launch_map_apply(e, U, G, (hipStream_t)stream);
}

int cesx_mh_run_map(cesx_handle h, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                    const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U) { e.err = "cesx_mh_run_map: null pointer"; return CESX_EINVAL; }
    if (n_steps < 1 || stride < 1) { e.err = "cesx_mh_run_map: n_steps and stride must be >= 1"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull || step_index + (uint64_t)n_steps > 0x80000000ull) { e.err = "cesx_mh_run_map: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    if (e.mh.kind == CESX_MH_LANGEVIN) { e.err = "cesx_mh_run_map: the proposal is CESX_MH_LANGEVIN (cesx_gp_langevin_*)"; return CESX_EINVAL; }
    if (!e.problem_set || e.mh.none() || !e.mh.started) { e.err = "cesx_mh_run_map: cesx_mh_start has not been called (after cesx_set_problem and cesx_mh_set_proposal)"; return CESX_ESTATE; }
    if (!e.mp.fused()) { e.err = "cesx_mh_run_map: no map of a fused kind is installed (cesx_map_set: CESX_MAP_ELLIPTIC or CESX_MAP_BANANA)"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_mh_run_map(e, step_index, n_steps, stride, U, trace, xi, logu, (hipStream_t)stream));
    e.mh.steps += (unsigned long long)n_steps;
    return CESX_OK;
}

// ---- The Langevin step of model_mh(chains=, update='langevin'): launch_gp_langevin on a map's G and Jacobian (kernels_gpgrad.hip,
// lv_* in mode CESX_GP_GAMMA: mean := G, dmean := DG, no variances), and its fused kernel (kernels_maps.hip) ----

int cesx_map_jac(cesx_handle h, const void* U, double* G, double* DG, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U || !G || !DG) { e.err = "cesx_map_jac: null pointer"; return CESX_EINVAL; }
    if (e.mp.none()) { e.err = "cesx_map_jac: cesx_map_set has not been called"; return CESX_ESTATE; }
    if (e.mp.desc.kind == CESX_MAP_EXP) { e.err = "cesx_map_jac: CESX_MAP_EXP has no Jacobian launch (lineal_log's gradient is an A^T product)"; return CESX_EUNSUPPORTED; }
    SET_DEVICE(e);
    return launch_map_jac(e, U, G, DG, (hipStream_t)stream);
}

// what every cesx_mh_langevin_* call needs before it looks at its own arguments; `started`: a cesx_mh_langevin_start too
static int mh_langevin_check_state(Engine& e, bool started) {
    if (started) TRY(adapt_refuses(e));
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN) { e.err = "cesx_mh_langevin: no Langevin proposal (cesx_mh_set_proposal with CESX_MH_LANGEVIN after cesx_set_problem)"; return CESX_ESTATE; }
    if (started && (!e.mh.started || e.mh.lin_started)) { e.err = "cesx_mh_langevin: cesx_mh_langevin_start has not been called (the last start was not it)"; return CESX_ESTATE; }
    return CESX_OK;
}

int cesx_mh_langevin_start(cesx_handle h, const void* U, const double* G, const double* DG, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(mh_langevin_check_state(e, false));
    if (!U || !G || !DG) { e.err = "cesx_mh_langevin_start: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    if (e.mh.grad_source == CESX_MH_GRAD_READY) TRY(launch_darcy_chain(e, 0, U, G, DG, nullptr, nullptr, 0u, (hipStream_t)stream));      // (DG: [p][J] ready-made)
    else TRY(launch_gp_langevin(e, 0, CESX_GP_GAMMA, U, G, nullptr, DG, nullptr, nullptr, nullptr, nullptr, 0u, (hipStream_t)stream));
    e.mh.started = true;
    e.mh.lin_started = false;
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    e.mh.steps = 0;
    return CESX_OK;
}

int cesx_mh_langevin_propose(cesx_handle h, uint64_t step_index, const void* U, const void* xi, void* P, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(mh_langevin_check_state(e, true));
    if (!U || !P) { e.err = "cesx_mh_langevin_propose: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_mh_langevin_propose: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_langevin_propose: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    // the block stays in engine memory: the accept step needs it again
    if (xi) CESX_HIP(hipMemcpyAsync(e.mh.xi, xi, (size_t)e.p * (size_t)e.J * e.esz, hipMemcpyDeviceToDevice, s));
    else TRY(launch_noise(e, mh_step_word(step_index), e.mh.xi, s));
    TRY(launch_gp_langevin(e, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, const_cast<void*>(U), P, nullptr, 0u, s));
    e.mh.lv_proposed = true; e.mh.hm_begun = false;      // (the block of a trajectory in flight is overwritten)
    return CESX_OK;
}

int cesx_mh_langevin_accept(cesx_handle h, uint64_t step_index, void* U, const void* P, const double* G, const double* DG,
                            const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(mh_langevin_check_state(e, true));
    if (!e.mh.lv_proposed) { e.err = "cesx_mh_langevin_accept: no cesx_mh_langevin_propose since the start or the last accept"; return CESX_ESTATE; }
    if (!U || !P || !G || !DG) { e.err = "cesx_mh_langevin_accept: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_mh_langevin_accept: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_langevin_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    if (e.mh.grad_source == CESX_MH_GRAD_READY) TRY(launch_darcy_chain(e, 1, P, G, DG, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    else TRY(launch_gp_langevin(e, 2, CESX_GP_GAMMA, P, G, nullptr, DG, nullptr, U, nullptr, logu, mh_step_word(step_index), (hipStream_t)stream));
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_mh_langevin_run_map(cesx_handle h, uint64_t step_index, int n_steps, int stride, void* U, void* trace, const void* xi,
                             const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U) { e.err = "cesx_mh_langevin_run_map: null pointer"; return CESX_EINVAL; }
    if (n_steps < 1 || stride < 1) { e.err = "cesx_mh_langevin_run_map: n_steps and stride must be >= 1"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull || step_index + (uint64_t)n_steps > 0x80000000ull) { e.err = "cesx_mh_langevin_run_map: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    TRY(mh_langevin_check_state(e, true));
    if (!e.mp.fused()) { e.err = "cesx_mh_langevin_run_map: no map of a fused kind is installed (cesx_map_set: CESX_MAP_ELLIPTIC or CESX_MAP_BANANA)"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_mh_langevin_run_map(e, step_index, n_steps, stride, U, trace, xi, logu, (hipStream_t)stream));
    e.mh.lv_proposed = false; e.mh.hm_begun = false;              // (a block proposed before the launch belongs to a state the chains have left)
    e.mh.steps += (unsigned long long)n_steps;
    return CESX_OK;
}

// ---- leapfrog HMC under a Langevin proposal (include/cesx.h; kernels_hmc.hip, mh_hmc_map_kernel of kernels_maps.hip) ----

// what every cesx_mh_hmc_* / cesx_gp_hmc_* call needs before it looks at its own arguments; `begun`: a cesx_mh_hmc_begin too
static int hmc_check_state(Engine& e, bool begun) {
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN) { e.err = "cesx_hmc: no Langevin proposal (cesx_mh_set_proposal with CESX_MH_LANGEVIN after cesx_set_problem)"; return CESX_ESTATE; }
    if (!e.mh.started || e.mh.lin_started) { e.err = "cesx_hmc: cesx_mh_langevin_start / cesx_gp_langevin_start has not been called (the last start was not one of them)"; return CESX_ESTATE; }
    if (begun && !e.mh.hm_begun) { e.err = "cesx_hmc: no cesx_mh_hmc_begin since the start or the last accept"; return CESX_ESTATE; }
    if (e.mh.ad_armed && e.mh.ad_done >= e.mh.ad_n) { e.err = "cesx_hmc: the adaptation steps of cesx_mh_adapt_set are done: read the multiplier (cesx_mh_adapt_read), then set the proposal (cesx_mh_set_proposal)"; return CESX_ESTATE; }
    return CESX_OK;
}

int cesx_mh_hmc_begin(cesx_handle h, uint64_t step_index, const void* U, const void* xi, void* Q, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, false));
    if (!U || !Q) { e.err = "cesx_mh_hmc_begin: null pointer"; return CESX_EINVAL; }
    if (U == Q) { e.err = "cesx_mh_hmc_begin: Q must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_hmc_begin: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    // the block stays in engine memory, as the Langevin proposal keeps it: the accept step needs |xi|^2
    if (xi) CESX_HIP(hipMemcpyAsync(e.mh.xi, xi, (size_t)e.p * (size_t)e.J * e.esz, hipMemcpyDeviceToDevice, s));
    else TRY(launch_noise(e, mh_step_word(step_index), e.mh.xi, s));
    TRY(launch_hmc(e, 0, 0, Q, nullptr, nullptr, nullptr, nullptr, const_cast<void*>(U), nullptr, 0u, s));
    e.mh.hm_begun = true;
    e.mh.lv_proposed = false;              // (a Langevin proposal's block is overwritten)
    return CESX_OK;
}

int cesx_mh_hmc_leap(cesx_handle h, void* Q, const double* G, const double* DG, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, true));
    if (!Q || !G || !DG) { e.err = "cesx_mh_hmc_leap: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    if (e.mh.grad_source == CESX_MH_GRAD_READY) return launch_darcy_chain(e, 2, Q, G, DG, nullptr, nullptr, 0u, (hipStream_t)stream);
    return launch_hmc(e, 1, CESX_GP_GAMMA, Q, G, nullptr, DG, nullptr, nullptr, nullptr, 0u, (hipStream_t)stream);
}

int cesx_mh_hmc_accept(cesx_handle h, uint64_t step_index, void* U, const void* Q, const double* G, const double* DG,
                       const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, true));
    if (!U || !Q || !G || !DG) { e.err = "cesx_mh_hmc_accept: null pointer"; return CESX_EINVAL; }
    if (U == Q) { e.err = "cesx_mh_hmc_accept: Q must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_hmc_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    if (e.mh.grad_source == CESX_MH_GRAD_READY) TRY(launch_darcy_chain(e, 3, Q, G, DG, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    else TRY(launch_hmc(e, 2, CESX_GP_GAMMA, const_cast<void*>(Q), G, nullptr, DG, nullptr, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    if (e.mh.ad_armed) { TRY(launch_adapt_update(e, (hipStream_t)stream)); ++e.mh.ad_done; }
    e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

// Where the four calls above take the data term of grad phi from (include/cesx.h): an install like cesx_mh_adapt_set -- no chains, no launch
int cesx_mh_grad_source(cesx_handle h, int source) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (source != CESX_MH_GRAD_JACOBIAN && source != CESX_MH_GRAD_READY) { e.err = "cesx_mh_grad_source: source must be CESX_MH_GRAD_JACOBIAN or CESX_MH_GRAD_READY"; return CESX_EINVAL; }
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN) { e.err = "cesx_mh_grad_source: no Langevin proposal (cesx_mh_set_proposal with CESX_MH_LANGEVIN after cesx_set_problem)"; return CESX_ESTATE; }
    if (source == CESX_MH_GRAD_READY && e.p > 256) { e.err = "cesx_mh_grad_source: CESX_MH_GRAD_READY serves p <= 256 (the chain's vectors live in LDS)"; return CESX_EUNSUPPORTED; }
    e.mh.grad_source = source;
    return CESX_OK;
}

int cesx_gp_hmc_leap(cesx_handle h, int mode, void* Q, const double* mean, const double* var, const double* dmean,
                     const double* dvar, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, true));
    if (e.gp.none()) { e.err = "cesx_gp_hmc_leap: cesx_gp_set has not been called"; return CESX_ESTATE; }
    if (!Q) { e.err = "cesx_gp_hmc_leap: null pointer"; return CESX_EINVAL; }
    TRY(langevin_check_mode(e, mode, mean, var, dmean, dvar));
    SET_DEVICE(e);
    FLUSH(e);
    return launch_hmc(e, 1, mode, Q, mean, var, dmean, dvar, nullptr, nullptr, 0u, (hipStream_t)stream);
}

int cesx_gp_hmc_accept(cesx_handle h, int mode, uint64_t step_index, void* U, const void* Q, const double* mean,
                       const double* var, const double* dmean, const double* dvar, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, true));
    if (e.gp.none()) { e.err = "cesx_gp_hmc_accept: cesx_gp_set has not been called"; return CESX_ESTATE; }
    if (!U || !Q) { e.err = "cesx_gp_hmc_accept: null pointer"; return CESX_EINVAL; }
    if (U == Q) { e.err = "cesx_gp_hmc_accept: Q must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_gp_hmc_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    TRY(langevin_check_mode(e, mode, mean, var, dmean, dvar));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_hmc(e, 2, mode, const_cast<void*>(Q), mean, var, dmean, dvar, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    if (e.mh.ad_armed) { TRY(launch_adapt_update(e, (hipStream_t)stream)); ++e.mh.ad_done; }
    e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

// ---- the gradient samplers on the projected Sigma (CESX_GP_PROJ; kernels_gpprojgrad.hip, then the lv_* / hm_* kernels) ----

// what cesx_gp_proj_coef and the cesx_gp_proj_langevin_* / cesx_gp_proj_hmc_* calls need of the descriptor, the emulator and the rows
static int proj_check(Engine& e, const double* mean, const double* var, const double* dmean, const double* dvar, bool grads) {
    if (e.gpp.none()) { e.err = "cesx_gp_proj: no descriptor (cesx_gp_proj_set after cesx_set_problem)"; return CESX_ESTATE; }
    if (e.gp.none()) { e.err = "cesx_gp_proj: cesx_gp_set has not been called"; return CESX_ESTATE; }
    if (e.gp.matern12) { e.err = "cesx_gp_proj: a Matern12 kernel is not differentiable at its training points"; return CESX_EUNSUPPORTED; }
    if (e.gp.n != e.gpp.k) { e.err = "cesx_gp_proj: the emulator's n_gp differs from the descriptor's k"; return CESX_EINVAL; }
    if (!mean || !var || (grads && (!dmean || !dvar))) { e.err = "cesx_gp_proj: null pointer (the projected Sigma needs var and dvar)"; return CESX_EINVAL; }
    return CESX_OK;
}

// lv_a / lv_b hold max(n, k) rows: a descriptor installed after the proposal, with k > n_obs, grows them here (what is in
// them is scratch of one launch; a launch in flight may still read the old ones)
static int proj_rows(Engine& e) {
    const size_t need = (size_t)std::max(e.n, e.gpp.k) * (size_t)e.J * 8;
    if (e.mh.lv_a.bytes >= need && e.mh.lv_b.bytes >= need) return CESX_OK;
    CESX_HIP(hipDeviceSynchronize());
    TRY_BUF(e.mh.lv_a.ensure(need)); TRY_BUF(e.mh.lv_b.ensure(need));
    return CESX_OK;
}

int cesx_gp_proj_coef(cesx_handle h, const double* mean, const double* var, double* phi, double* a, double* b, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(proj_check(e, mean, var, nullptr, nullptr, false));
    if (!phi || !a || !b) { e.err = "cesx_gp_proj_coef: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    return launch_gp_proj_coef(e, mean, var, phi, a, b, (hipStream_t)stream);
}

int cesx_gp_proj_langevin_start(cesx_handle h, const void* U, const double* mean, const double* var, const double* dmean,
                                const double* dvar, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(langevin_check_state(e, false));
    if (!U) { e.err = "cesx_gp_proj_langevin_start: null pointer"; return CESX_EINVAL; }
    TRY(proj_check(e, mean, var, dmean, dvar, true));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(proj_rows(e));
    TRY(launch_gp_proj_coef(e, mean, var, e.mh.phi_data, e.mh.lv_a, e.mh.lv_b, (hipStream_t)stream));
    TRY(launch_gp_langevin(e, 0, CESX_GP_PROJ, U, mean, var, dmean, dvar, nullptr, nullptr, nullptr, 0u, (hipStream_t)stream));
    e.mh.started = true;
    e.mh.lin_started = false;
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    e.mh.steps = 0;
    return CESX_OK;
}

int cesx_gp_proj_langevin_accept(cesx_handle h, uint64_t step_index, void* U, const void* P, const double* mean, const double* var,
                                 const double* dmean, const double* dvar, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(langevin_check_state(e, true));
    if (!e.mh.lv_proposed) { e.err = "cesx_gp_proj_langevin_accept: no cesx_gp_langevin_propose since the start or the last accept"; return CESX_ESTATE; }
    if (!U || !P) { e.err = "cesx_gp_proj_langevin_accept: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_gp_proj_langevin_accept: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_gp_proj_langevin_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    TRY(proj_check(e, mean, var, dmean, dvar, true));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(proj_rows(e));
    TRY(launch_gp_proj_coef(e, mean, var, e.mh.phi_data, e.mh.lv_a, e.mh.lv_b, (hipStream_t)stream));
    TRY(launch_gp_langevin(e, 2, CESX_GP_PROJ, P, mean, var, dmean, dvar, U, nullptr, logu, mh_step_word(step_index), (hipStream_t)stream));
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_gp_proj_hmc_leap(cesx_handle h, void* Q, const double* mean, const double* var, const double* dmean, const double* dvar,
                          void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, true));
    if (!Q) { e.err = "cesx_gp_proj_hmc_leap: null pointer"; return CESX_EINVAL; }
    TRY(proj_check(e, mean, var, dmean, dvar, true));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(proj_rows(e));
    TRY(launch_gp_proj_coef(e, mean, var, e.mh.phi_data, e.mh.lv_a, e.mh.lv_b, (hipStream_t)stream));
    return launch_hmc(e, 1, CESX_GP_PROJ, Q, mean, var, dmean, dvar, nullptr, nullptr, 0u, (hipStream_t)stream);
}

int cesx_gp_proj_hmc_accept(cesx_handle h, uint64_t step_index, void* U, const void* Q, const double* mean, const double* var,
                            const double* dmean, const double* dvar, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hmc_check_state(e, true));
    if (!U || !Q) { e.err = "cesx_gp_proj_hmc_accept: null pointer"; return CESX_EINVAL; }
    if (U == Q) { e.err = "cesx_gp_proj_hmc_accept: Q must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_gp_proj_hmc_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    TRY(proj_check(e, mean, var, dmean, dvar, true));
    SET_DEVICE(e);
    FLUSH(e);
    TRY(proj_rows(e));
    TRY(launch_gp_proj_coef(e, mean, var, e.mh.phi_data, e.mh.lv_a, e.mh.lv_b, (hipStream_t)stream));
    TRY(launch_hmc(e, 2, CESX_GP_PROJ, const_cast<void*>(Q), mean, var, dmean, dvar, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    if (e.mh.ad_armed) { TRY(launch_adapt_update(e, (hipStream_t)stream)); ++e.mh.ad_done; }
    e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_mh_hmc_run_map(cesx_handle h, uint64_t step_index, int n_steps, int leapfrog, int stride, void* U, void* trace,
                        const void* xi, const double* logu, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!U) { e.err = "cesx_mh_hmc_run_map: null pointer"; return CESX_EINVAL; }
    if (n_steps < 1 || stride < 1) { e.err = "cesx_mh_hmc_run_map: n_steps and stride must be >= 1"; return CESX_EINVAL; }
    if (leapfrog < 1 || leapfrog > CESX_HMC_LEAPFROG_MAX) { e.err = "cesx_mh_hmc_run_map: leapfrog must be in 1 .. 64"; return CESX_EINVAL; }
    if ((long long)n_steps * leapfrog > CESX_HMC_LAUNCH_GRADS_MAX) { e.err = "cesx_mh_hmc_run_map: n_steps * leapfrog is limited to 4096 gradient evaluations per launch"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull || step_index + (uint64_t)n_steps > 0x80000000ull) { e.err = "cesx_mh_hmc_run_map: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    TRY(adapt_refuses(e));
    TRY(hmc_check_state(e, false));
    if (!e.mp.fused()) { e.err = "cesx_mh_hmc_run_map: no map of a fused kind is installed (cesx_map_set: CESX_MAP_ELLIPTIC or CESX_MAP_BANANA)"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(launch_mh_hmc_run_map(e, step_index, n_steps, leapfrog, stride, U, trace, xi, logu, (hipStream_t)stream));
    e.mh.lv_proposed = false; e.mh.hm_begun = false;      // (a block drawn before the launch belongs to a state the chains have left)
    e.mh.steps += (unsigned long long)n_steps;
    return CESX_OK;
}

// ---- pooled step-size adaptation of the leapfrog step (include/cesx.h; kernels_adapt.hip, the ADAPT kernels of kernels_hmc.hip) ----

// Failure rule: an argument or state error leaves the handle as it was; behind them a failed allocation leaves it unarmed.
int cesx_mh_adapt_set(cesx_handle h, int n_steps, double target, double gain, double kappa) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (n_steps < 1 || n_steps > CESX_ADAPT_STEPS_MAX) { e.err = "cesx_mh_adapt_set: n_steps must be in 1 .. 65536"; return CESX_EINVAL; }
    if (!(target > 0.0 && target < 1.0)) { e.err = "cesx_mh_adapt_set: target must lie in (0, 1)"; return CESX_EINVAL; }
    if (!(gain > 0.0) || !std::isfinite(gain)) { e.err = "cesx_mh_adapt_set: gain must be finite and > 0"; return CESX_EINVAL; }
    if (!(kappa > 0.5 && kappa <= 1.0)) { e.err = "cesx_mh_adapt_set: kappa must lie in (0.5, 1]"; return CESX_EINVAL; }
    if (e.J != e.Jg) { e.err = "cesx_mh_adapt_set: sharded chains (J_local != J_global) are not pooled: the mean acceptance would need a reduce across ranks"; return CESX_EUNSUPPORTED; }
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN) { e.err = "cesx_mh_adapt_set: no Langevin proposal (cesx_mh_set_proposal with CESX_MH_LANGEVIN after cesx_set_problem)"; return CESX_ESTATE; }
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (an earlier phase's launches may still read the state)
    e.mh.ad_armed = false;
    TRY_BUF(e.mh.ad_alpha.ensure((size_t)e.J * 8));
    TRY_BUF(e.mh.ad_state.ensure(4 * 8));
    TRY_BUF(e.mh.ad_hist.alloc((size_t)n_steps * 2 * 8));
    const double st[4] = {1.0, 0.0, 0.0, 0.0};          // e_1 = 1, log e_1 = 0, log ebar_0 = 0, t = 0
    CESX_HIP(hipMemcpy(e.mh.ad_state, st, sizeof st, hipMemcpyHostToDevice));
    e.mh.ad_n = n_steps; e.mh.ad_done = 0;
    e.mh.ad_target = target; e.mh.ad_gain = gain; e.mh.ad_kappa = kappa;
    e.mh.hm_begun = false;                     // (a trajectory begun at S is not finished at e S)
    e.mh.ad_armed = true;
    return CESX_OK;
}

int cesx_mh_adapt_read(cesx_handle h, double* multiplier, int* steps_done, double* history) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!multiplier || !steps_done) { e.err = "cesx_mh_adapt_read: null pointer"; return CESX_EINVAL; }
    if (!e.mh.ad_armed) { e.err = "cesx_mh_adapt_read: the handle is not armed (cesx_mh_adapt_set after cesx_mh_set_proposal)"; return CESX_ESTATE; }
    SET_DEVICE(e);
    CESX_HIP(hipDeviceSynchronize());
    double st[4];
    CESX_HIP(hipMemcpy(st, e.mh.ad_state, sizeof st, hipMemcpyDeviceToHost));
    *multiplier = std::exp(st[2]);             // ebar_A; no step yet: log ebar_0 = 0, the multiplier 1
    *steps_done = e.mh.ad_done;
    if (history && e.mh.ad_done > 0)
        CESX_HIP(hipMemcpy(history, e.mh.ad_hist, (size_t)e.mh.ad_done * 2 * 8, hipMemcpyDeviceToHost));
    return CESX_OK;
}

// ---- the Langevin step on a linear map: the gradient as update launches (include/cesx.h; kernels_lvlin.hip) ----

// a p x ktot fp64 matrix (row-major, its padding columns zero) into the update kernels' [rpad][ktot] layouts, engine dtype
static int lin_upload(Engine& e, const std::vector<double>& M, int ktot, DevBuf<void>& rm_dev, DevBuf<void>& fm_dev) {
    const size_t len = (size_t)e.rpad * ktot;
    std::vector<double> rm(len, 0.0), fm(len, 0.0);
    const int nkt = ktot / 16;
    for (int i = 0; i < e.p; ++i)
        for (int k = 0; k < ktot; ++k) {
            const double v = M[(size_t)i * ktot + k];
            rm[(size_t)i * ktot + k] = v;
            fm[e.cfg.dtype == CESX_F32 ? wf_index(i, k, nkt) : wd_index(i, k, nkt)] = v;
        }
    TRY_BUF(rm_dev.ensure(len * e.esz)); TRY_BUF(fm_dev.ensure(len * e.esz));
    TRY(upload_T(e, rm_dev, rm.data(), len));
    return upload_T(e, fm_dev, fm.data(), len);
}

static int lin_upload_bias(Engine& e, const std::vector<double>& b, DevBuf<void>& dev) {
    std::vector<double> pad(e.rpad, 0.0);
    std::copy(b.begin(), b.end(), pad.begin());
    TRY_BUF(dev.ensure((size_t)e.rpad * e.esz));
    return upload_T(e, dev, pad.data(), e.rpad);
}

// Failure rule: from the synchronise until the last upload the handle has NO lineal image; a failure leaves it so.
int cesx_mh_langevin_lineal_set(cesx_handle h, const double* A, const double* b, int exp_params) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!A) { e.err = "cesx_mh_langevin_lineal_set: null pointer"; return CESX_EINVAL; }
    if (exp_params != 0 && exp_params != 1) { e.err = "cesx_mh_langevin_lineal_set: exp_params must be 0 or 1"; return CESX_EINVAL; }
    TRY(adapt_refuses(e));
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN) { e.err = "cesx_mh_langevin_lineal_set: no Langevin proposal (cesx_mh_set_proposal with CESX_MH_LANGEVIN after cesx_set_problem)"; return CESX_ESTATE; }
    const int p = e.p, n = e.n, kp = e.kp, kn = e.kn;
    for (size_t i = 0; i < (size_t)n * p; ++i)
        if (!std::isfinite(A[i])) { e.err = "cesx_mh_langevin_lineal_set: A is not finite"; return CESX_EINVAL; }
    for (int i = 0; b && i < n; ++i)       // (b enters through G alone -- the caller's rows carry it --: checked, not stored)
        if (!std::isfinite(b[i])) { e.err = "cesx_mh_langevin_lineal_set: b is not finite"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    CESX_HIP(hipDeviceSynchronize());          // (the images below may be read by launches still in flight)
    if (e.mh.lin_started) e.mh.started = false;        // (the chains' g belonged to the old image)
    e.mh.lin = 0; e.mh.lin_started = false; e.mh.lv_proposed = false; e.mh.hm_begun = false;
    // B = A^T M, p x n, with M (G~ - y~) = Gamma^{-1} (G - y) for the rows G~ the score kernel reads: Gamma^{-1} itself on the
    // caller's rows (diagonal), L_Gamma^{-T} on the whitened ones (dense: B[q][i] = sum_{k <= i} A[k][q] Li[i][k])
    std::vector<double> B((size_t)p * n, 0.0);
    for (int q = 0; q < p; ++q)
        for (int i = 0; i < n; ++i) {
            double acc = 0.0;
            if (e.whiten) for (int k = 0; k <= i; ++k) acc += A[(size_t)k * p + q] * e.h_Li[(size_t)i * n + k];
            else acc = A[(size_t)i * p + q] * e.h_gw[i];
            B[(size_t)q * n + i] = acc;
        }
    std::vector<double> Sinv;
    host_spd_inverse(p, e.h_LSi, Sinv);
    // S^T X for the lower-triangular scales S (p x p) and X (p x m)
    const std::vector<double>& S = e.mh.h_bS;
    auto St_times = [&](const std::vector<double>& X, int m) {
        std::vector<double> out((size_t)p * m, 0.0);
        for (int r = 0; r < p; ++r)
            for (int q = r; q < p; ++q) {
                const double sv = S[(size_t)q * p + r];
                if (sv == 0.0) continue;
                for (int i = 0; i < m; ++i) out[(size_t)r * m + i] += sv * X[(size_t)q * m + i];
            }
        return out;
    };
    const std::vector<double> StSinv = St_times(Sinv, p);
    std::vector<double> bias_prior(p, 0.0);            // -S^T Sigma^{-1} mu
    for (int r = 0; r < p; ++r) {
        double acc = 0.0;
        for (int k = 0; k < p; ++k) acc += StSinv[(size_t)r * p + k] * e.h_mu[k];
        bias_prior[r] = -acc;
    }
    auto minus_times_y = [&](const std::vector<double>& X) {       // -X y~ (X p x n)
        std::vector<double> out(p, 0.0);
        for (int r = 0; r < p; ++r) {
            double acc = 0.0;
            for (int i = 0; i < n; ++i) acc += X[(size_t)r * n + i] * e.h_yw[i];
            out[r] = -acc;
        }
        return out;
    };
    if (!exp_params) {
        // lineal: g = [S^T B | S^T Sigma^{-1}] . [G~ ; X] - S^T B y~ - S^T Sigma^{-1} mu, one launch
        const int kt = kn + kp;
        const std::vector<double> StB = St_times(B, n);
        std::vector<double> W((size_t)p * kt, 0.0), bias = minus_times_y(StB);
        for (int r = 0; r < p; ++r) {
            for (int i = 0; i < n; ++i) W[(size_t)r * kt + i] = StB[(size_t)r * n + i];
            for (int k = 0; k < p; ++k) W[(size_t)r * kt + kn + k] = StSinv[(size_t)r * p + k];
            bias[r] += bias_prior[r];
        }
        TRY(lin_upload(e, W, kt, e.mh.lin_Wa, e.mh.lin_Wa_f));
        TRY(lin_upload_bias(e, bias, e.mh.lin_ba));
    } else {
        // lineal_log: t0 = B . G~ - B y~; h = exp(X) (.) t0; g = [S^T | S^T Sigma^{-1}] . [h ; X] - S^T Sigma^{-1} mu
        std::vector<double> Wa((size_t)p * kn, 0.0), Wb((size_t)p * 2 * kp, 0.0);
        for (int r = 0; r < p; ++r) {
            for (int i = 0; i < n; ++i) Wa[(size_t)r * kn + i] = B[(size_t)r * n + i];
            for (int k = r; k < p; ++k) Wb[(size_t)r * 2 * kp + k] = S[(size_t)k * p + r];
            for (int k = 0; k < p; ++k) Wb[(size_t)r * 2 * kp + kp + k] = StSinv[(size_t)r * p + k];
        }
        TRY(lin_upload(e, Wa, kn, e.mh.lin_Wa, e.mh.lin_Wa_f));
        TRY(lin_upload_bias(e, minus_times_y(B), e.mh.lin_ba));
        TRY(lin_upload(e, Wb, 2 * kp, e.mh.lin_Wb, e.mh.lin_Wb_f));
        TRY(lin_upload_bias(e, bias_prior, e.mh.lin_bb));
        TRY_BUF(e.mh.lin_t.ensure((size_t)p * (size_t)e.J * e.esz));
    }
    if (!e.diag_sigma) {                       // the prior sum runs over w = L_Sigma^{-1} (X - mu): the random walk's images (a Langevin proposal has none)
        TRY(mh_upload_tri(e, e.h_LSi.data(), e.mh.Li, e.mh.Li_f));
        std::vector<double> lb(e.rpad, 0.0);
        for (int i = 0; i < p; ++i) {
            double acc = 0.0;
            for (int k = 0; k <= i; ++k) acc += e.h_LSi[(size_t)i * p + k] * e.h_mu[k];
            lb[i] = -acc;
        }
        TRY_BUF(e.mh.lb.ensure((size_t)e.rpad * e.esz));
        TRY(upload_T(e, e.mh.lb, lb.data(), e.rpad));
        TRY_BUF(e.mh.w.ensure((size_t)p * (size_t)e.J * e.esz));
    }
    const size_t blk = (size_t)p * (size_t)e.J * e.esz;
    TRY_BUF(e.mh.lin_g.ensure(blk)); TRY_BUF(e.mh.lin_gp.ensure(blk)); TRY_BUF(e.mh.lin_z.ensure(blk));
    e.mh.lin = exp_params ? 2 : 1;
    return CESX_OK;
}

// g = S^T grad phi of the states X with their data rows Gw (whitened for a dense Gamma) into `out`
static int lin_grad(Engine& e, const void* X, const void* Gw, void* out, hipStream_t s) {
    if (e.mh.lin == 1)
        return launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.lin_Wa, .Wf = e.mh.lin_Wa_f, .ktot = e.kn + e.kp, .bias = e.mh.lin_ba,
                                             .src = {{Gw, e.n, 0, 0}, {X, e.p, 0, 0}}, .nsrc = 2, .out = out}, s);
    TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.lin_Wa, .Wf = e.mh.lin_Wa_f, .ktot = e.kn, .bias = e.mh.lin_ba,
                                      .src = {{Gw, e.n, 0, 0}}, .nsrc = 1, .out = e.mh.lin_t}, s));
    TRY(launch_lvlin_exph(e, X, e.mh.lin_t, s));
    return launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.lin_Wb, .Wf = e.mh.lin_Wb_f, .ktot = 2 * e.kp, .bias = e.mh.lin_bb,
                                         .src = {{e.mh.lin_t, e.p, 0, 0}, {X, e.p, 0, 0}}, .nsrc = 2, .out = out}, s);
}

// phi and g of the states X with their forward map G (start: into the engine's phi and g; accept: the test, U := X, g := g(X))
static int lin_score(Engine& e, bool start, const void* X, const void* G, void* U, const double* logu, unsigned step, hipStream_t s) {
    WHITEN(e, G, s, true);
    if (!e.diag_sigma)
        TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.Li, .Wf = e.mh.Li_f, .ktot = e.kp, .bias = e.mh.lb,
                                          .src = {{X, e.p, 0, 1}}, .nsrc = 1, .out = e.mh.w}, s));
    TRY(lin_grad(e, X, G, start ? e.mh.lin_g.get() : e.mh.lin_gp.get(), s));
    return launch_lvlin_score(e, start, X, G, U, logu, step, s);
}

// what every cesx_mh_langevin_lineal_* call behind the set needs before it looks at its own arguments
static int lin_check_state(Engine& e, bool started) {
    TRY(adapt_refuses(e));
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN || !e.mh.lin) { e.err = "cesx_mh_langevin_lineal: no lineal image (cesx_mh_langevin_lineal_set after cesx_mh_set_proposal with CESX_MH_LANGEVIN)"; return CESX_ESTATE; }
    if (started && !(e.mh.started && e.mh.lin_started)) { e.err = "cesx_mh_langevin_lineal: the last start was not cesx_mh_langevin_lineal_start"; return CESX_ESTATE; }
    return CESX_OK;
}

int cesx_mh_langevin_lineal_start(cesx_handle h, const void* U, const void* G, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(lin_check_state(e, false));
    if (!U || !G) { e.err = "cesx_mh_langevin_lineal_start: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(lin_score(e, true, U, G, nullptr, nullptr, 0u, (hipStream_t)stream));
    e.mh.started = true;
    e.mh.lin_started = true;
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    e.mh.steps = 0;
    return CESX_OK;
}

int cesx_mh_langevin_lineal_propose(cesx_handle h, uint64_t step_index, const void* U, const void* xi, void* P, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(lin_check_state(e, true));
    if (!U || !P) { e.err = "cesx_mh_langevin_lineal_propose: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_mh_langevin_lineal_propose: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_langevin_lineal_propose: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    // the block stays in engine memory: the accept step needs it again
    if (xi) CESX_HIP(hipMemcpyAsync(e.mh.xi, xi, (size_t)e.p * (size_t)e.J * e.esz, hipMemcpyDeviceToDevice, s));
    else TRY(launch_noise(e, mh_step_word(step_index), e.mh.xi, s));
    TRY(launch_lvlin_z(e, s));
    // P = U + S z: the random walk's triangular launch on z = xi - g / 2
    TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.W, .Wf = e.mh.Wf, .ktot = e.kp,
                                      .src = {{e.mh.lin_z, e.p, 0, 1}}, .nsrc = 1, .add1 = {U, nullptr, 1.0}, .out = P}, s));
    e.mh.lv_proposed = true; e.mh.hm_begun = false;      // (the block of a trajectory in flight is overwritten)
    return CESX_OK;
}

int cesx_mh_langevin_lineal_accept(cesx_handle h, uint64_t step_index, void* U, const void* P, const void* GP, const double* logu,
                                   void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(lin_check_state(e, true));
    if (!e.mh.lv_proposed) { e.err = "cesx_mh_langevin_lineal_accept: no cesx_mh_langevin_lineal_propose since the start or the last accept"; return CESX_ESTATE; }
    if (!U || !P || !GP) { e.err = "cesx_mh_langevin_lineal_accept: null pointer"; return CESX_EINVAL; }
    if (U == P) { e.err = "cesx_mh_langevin_lineal_accept: P must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_langevin_lineal_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    TRY(lin_score(e, false, P, GP, U, logu, mh_step_word(step_index), (hipStream_t)stream));
    e.mh.lv_proposed = false; e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

int cesx_mh_langevin_lineal_g(cesx_handle h, double* g_host) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(lin_check_state(e, true));
    if (!g_host) { e.err = "cesx_mh_langevin_lineal_g: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    const size_t len = (size_t)e.p * (size_t)e.J;
    CESX_HIP(hipDeviceSynchronize());
    if (e.cfg.dtype == CESX_F64) {
        CESX_HIP(hipMemcpy(g_host, e.mh.lin_g, len * 8, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp(len);
        CESX_HIP(hipMemcpy(tmp.data(), e.mh.lin_g, len * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < len; ++i) g_host[i] = (double)tmp[i];
    }
    return CESX_OK;
}

// ---- the leapfrog step on a linear map: the Langevin step's launches around a momentum block (include/cesx.h; kernels_hmclin.hip) ----

// lin_check_state(e, true) without its blanket refusal of an armed handle; `begun`: a cesx_mh_hmc_lineal_begin too
static int hl_check_state(Engine& e, bool begun) {
    if (!e.problem_set || e.mh.none() || e.mh.kind != CESX_MH_LANGEVIN || !e.mh.lin) { e.err = "cesx_mh_hmc_lineal: no lineal image (cesx_mh_langevin_lineal_set after cesx_mh_set_proposal with CESX_MH_LANGEVIN)"; return CESX_ESTATE; }
    if (!(e.mh.started && e.mh.lin_started)) { e.err = "cesx_mh_hmc_lineal: the last start was not cesx_mh_langevin_lineal_start"; return CESX_ESTATE; }
    if (begun && !e.mh.hm_begun) { e.err = "cesx_mh_hmc_lineal: no cesx_mh_hmc_lineal_begin since the start or the last accept"; return CESX_ESTATE; }
    if (e.mh.ad_armed && e.mh.ad_done >= e.mh.ad_n) { e.err = "cesx_mh_hmc_lineal: the adaptation steps of cesx_mh_adapt_set are done: read the multiplier (cesx_mh_adapt_read), then set the proposal (cesx_mh_set_proposal)"; return CESX_ESTATE; }
    return CESX_OK;
}

// out = Q + S z with z in mh.lin_z: the triangular launch of cesx_mh_langevin_lineal_propose (out never aliases Q: the callers refuse it)
static int hl_drift(Engine& e, const void* Q, void* out, hipStream_t s) {
    return launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.W, .Wf = e.mh.Wf, .ktot = e.kp,
                                         .src = {{e.mh.lin_z, e.p, 0, 1}}, .nsrc = 1, .add1 = {Q, nullptr, 1.0}, .out = out}, s);
}

int cesx_mh_hmc_lineal_begin(cesx_handle h, uint64_t step_index, const void* U, const void* xi, void* Q, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hl_check_state(e, false));
    if (!U || !Q) { e.err = "cesx_mh_hmc_lineal_begin: null pointer"; return CESX_EINVAL; }
    if (U == Q) { e.err = "cesx_mh_hmc_lineal_begin: Q must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_hmc_lineal_begin: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    if (e.mh.ad_armed) TRY_BUF(e.mh.lin_r.ensure((size_t)e.p * (size_t)e.J * e.esz));      // (r beside z = e r)
    // the block stays in engine memory, as the Langevin proposal keeps it: the accept step needs |xi|^2
    if (xi) CESX_HIP(hipMemcpyAsync(e.mh.xi, xi, (size_t)e.p * (size_t)e.J * e.esz, hipMemcpyDeviceToDevice, s));
    else TRY(launch_noise(e, mh_step_word(step_index), e.mh.xi, s));
    TRY(launch_hl_kick(e, true, s));
    TRY(hl_drift(e, U, Q, s));
    e.mh.hm_begun = true; e.mh.hl_leaps = 0;
    e.mh.lv_proposed = false;              // (a Langevin proposal's block is overwritten)
    return CESX_OK;
}

int cesx_mh_hmc_lineal_leap(cesx_handle h, const void* Q, const void* GQ, void* Qnext, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hl_check_state(e, true));
    if (!Q || !GQ || !Qnext) { e.err = "cesx_mh_hmc_lineal_leap: null pointer"; return CESX_EINVAL; }
    if (Q == Qnext) { e.err = "cesx_mh_hmc_lineal_leap: Qnext must not alias Q (the drift launch reads Q while it writes Qnext)"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    WHITEN(e, GQ, s, true);
    TRY(lin_grad(e, Q, GQ, e.mh.lin_gp.get(), s));      // (no phi: neither the score kernel nor the Li product of a dense Sigma)
    TRY(launch_hl_kick(e, false, s));
    TRY(hl_drift(e, Q, Qnext, s));
    ++e.mh.hl_leaps;
    return CESX_OK;
}

int cesx_mh_hmc_lineal_accept(cesx_handle h, uint64_t step_index, void* U, const void* Q, const void* GQ, const double* logu,
                              void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    TRY(hl_check_state(e, true));
    if (!U || !Q || !GQ) { e.err = "cesx_mh_hmc_lineal_accept: null pointer"; return CESX_EINVAL; }
    if (U == Q) { e.err = "cesx_mh_hmc_lineal_accept: Q must not alias U"; return CESX_EINVAL; }
    if (step_index >= 0x80000000ull) { e.err = "cesx_mh_hmc_lineal_accept: MH step indices are limited to 2^31"; return CESX_EINVAL; }
    SET_DEVICE(e);
    FLUSH(e);
    hipStream_t s = (hipStream_t)stream;
    if (!e.mh.ad_armed && e.mh.hl_leaps == 0) {
        // L = 1: xi, g(U) and g(Q) are the Langevin accept's inputs, and its launches give its bits
        TRY(lin_score(e, false, Q, GQ, U, logu, mh_step_word(step_index), s));
    } else {
        WHITEN(e, GQ, s, true);
        if (!e.diag_sigma)
            TRY(launch_update(e, UpdateLaunch{.out_rows = e.p, .W = e.mh.Li, .Wf = e.mh.Li_f, .ktot = e.kp, .bias = e.mh.lb,
                                              .src = {{Q, e.p, 0, 1}}, .nsrc = 1, .out = e.mh.w}, s));
        TRY(lin_grad(e, Q, GQ, e.mh.lin_gp.get(), s));
        TRY(launch_hl_accept(e, Q, GQ, U, logu, mh_step_word(step_index), s));
        if (e.mh.ad_armed) { TRY(launch_adapt_update(e, s)); ++e.mh.ad_done; }
    }
    e.mh.hm_begun = false;
    ++e.mh.steps;
    return CESX_OK;
}

// ---- Streaming summaries of the chains' draws (MCMC(..., chains=M, summary=True); kernels_chainsum.hip) ----

int cesx_chain_summary_begin(cesx_handle h, int n_draws, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    (void)stream;                                         // nothing is launched: the first add overwrites the stage's sums
    if (n_draws < 4) { e.err = "cesx_chain_summary_begin: n_draws must be >= 4 (two half-chains of two draws)"; return CESX_EINVAL; }
    if (e.J != e.Jg) { e.err = "cesx_chain_summary_begin: sharded chains (J_local != J_global) are not summarised"; return CESX_EINVAL; }
    SET_DEVICE(e);
    return chainsum_begin(e, n_draws);
}

int cesx_chain_summary_add(cesx_handle h, const void* trace, int kept, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!trace) { e.err = "cesx_chain_summary_add: null pointer"; return CESX_EINVAL; }
    if (kept < 1) { e.err = "cesx_chain_summary_add: kept must be >= 1"; return CESX_EINVAL; }
    if (e.cs.none()) { e.err = "cesx_chain_summary_add: cesx_chain_summary_begin has not been called"; return CESX_ESTATE; }
    if (e.cs.added + kept > e.cs.N) { e.err = "cesx_chain_summary_add: more draws than cesx_chain_summary_begin announced"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return chainsum_add(e, trace, kept, (hipStream_t)stream);
}

int cesx_chain_summary_read(cesx_handle h, double* c, double* s1, double* cc, double* within, double* between, double* half_mean,
                            double* half_var, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!c || !s1 || !cc || !within || !between) { e.err = "cesx_chain_summary_read: null pointer"; return CESX_EINVAL; }
    if (e.cs.none()) { e.err = "cesx_chain_summary_read: cesx_chain_summary_begin has not been called"; return CESX_ESTATE; }
    if (e.cs.added != e.cs.N) { e.err = "cesx_chain_summary_read: fewer draws were added than cesx_chain_summary_begin announced"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return chainsum_read(e, c, s1, cc, within, between, half_mean, half_var, (hipStream_t)stream);
}

// ---- Streaming marginals of the chains' draws (MCMC(..., chains=M, summary=True, marginals=...); kernels_chainhist.hip) ----

// finite and strictly increasing
static bool hist_edges_ok(const double* e, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1]))) return false;
    return true;
}

// Failure rule: a refused begin touches nothing; the run in hand goes on.
int cesx_chain_hist_begin(cesx_handle h, const cesx_chain_hist_desc* d, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!d || d->struct_bytes != (uint32_t)sizeof(cesx_chain_hist_desc)) { e.err = "cesx_chain_hist_begin: bad cesx_chain_hist_desc"; return CESX_EINVAL; }
    if (e.J != e.Jg) { e.err = "cesx_chain_hist_begin: sharded chains (J_local != J_global) are not counted"; return CESX_EINVAL; }
    if (d->bins < 2 || d->bins > CESX_CHAIN_HIST_BINS_MAX) { e.err = "cesx_chain_hist_begin: bins must be in [2, 256]"; return CESX_EINVAL; }
    if (d->bins2d < 2 || d->bins2d > CESX_CHAIN_HIST_BINS2D_MAX) { e.err = "cesx_chain_hist_begin: bins2d must be in [2, 64]"; return CESX_EINVAL; }
    if (d->n_pairs < 0 || d->n_pairs > CESX_CHAIN_HIST_PAIRS_MAX) { e.err = "cesx_chain_hist_begin: n_pairs must be in [0, 64]"; return CESX_EINVAL; }
    if (!d->edges1 || (d->n_pairs > 0 && (!d->edges2 || !d->pairs))) { e.err = "cesx_chain_hist_begin: null pointer"; return CESX_EINVAL; }
    for (int r = 0; r < e.p; ++r)
        if (!hist_edges_ok(d->edges1 + (size_t)r * (d->bins + 1), d->bins + 1)) {
            e.err = "cesx_chain_hist_begin: edges1 of row " + std::to_string(r) + " are not finite and strictly increasing";
            return CESX_EINVAL;
        }
    for (int k = 0; k < d->n_pairs; ++k) {
        const int i = d->pairs[2 * k], j = d->pairs[2 * k + 1];
        if (i < 0 || i >= e.p || j < 0 || j >= e.p || i == j) {
            e.err = "cesx_chain_hist_begin: pair " + std::to_string(k) + " must name two different rows in [0, p)";
            return CESX_EINVAL;
        }
        for (const int r : {i, j})
            if (!hist_edges_ok(d->edges2 + (size_t)r * (d->bins2d + 1), d->bins2d + 1)) {
                e.err = "cesx_chain_hist_begin: edges2 of row " + std::to_string(r) + " are not finite and strictly increasing";
                return CESX_EINVAL;
            }
    }
    SET_DEVICE(e);
    return chainhist_begin(e, d, (hipStream_t)stream);
}

int cesx_chain_hist_add(cesx_handle h, const void* trace, int kept, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!trace) { e.err = "cesx_chain_hist_add: null pointer"; return CESX_EINVAL; }
    if (kept < 1) { e.err = "cesx_chain_hist_add: kept must be >= 1"; return CESX_EINVAL; }
    if (e.ch.none()) { e.err = "cesx_chain_hist_add: cesx_chain_hist_begin has not been called"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return chainhist_add(e, trace, kept, (hipStream_t)stream);
}

int cesx_chain_hist_read(cesx_handle h, unsigned long long* hist1, unsigned long long* out1, unsigned long long* hist2,
                         unsigned long long* out2, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (e.ch.none()) { e.err = "cesx_chain_hist_read: cesx_chain_hist_begin has not been called"; return CESX_ESTATE; }
    if (!hist1 || !out1 || (e.ch.n_pairs > 0 && (!hist2 || !out2))) { e.err = "cesx_chain_hist_read: null pointer"; return CESX_EINVAL; }
    SET_DEVICE(e);
    return chainhist_read(e, hist1, out1, hist2, out2, (hipStream_t)stream);
}

// ---- Streaming lagged sums of the chains' draws (MCMC(..., chains=M, summary=True, autocorr=...); kernels_chainacf.hip) ----

// Failure rule: a refused call launches nothing and touches nothing; the run in hand goes on.
int cesx_chain_acf_begin(cesx_handle h, int n_draws, int lags, int n_chains, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    (void)stream;                                         // nothing is launched: the first lag launch overwrites the stage's sums
    if (e.J != e.Jg) { e.err = "cesx_chain_acf_begin: sharded chains (J_local != J_global) are not followed"; return CESX_EINVAL; }
    if (lags < 1 || lags > CESX_CHAIN_ACF_LAGS_MAX) { e.err = "cesx_chain_acf_begin: lags must be in [1, " + std::to_string(CESX_CHAIN_ACF_LAGS_MAX) + "]"; return CESX_EINVAL; }
    if (n_chains < 1 || n_chains > e.J) { e.err = "cesx_chain_acf_begin: n_chains must be in [1, J_local]"; return CESX_EINVAL; }
    if (n_draws < 4 || n_draws < lags + 2) { e.err = "cesx_chain_acf_begin: n_draws must be >= max(4, lags + 2)"; return CESX_EINVAL; }
    SET_DEVICE(e);
    return chainacf_begin(e, n_draws, lags, n_chains);
}

int cesx_chain_acf_add(cesx_handle h, const void* trace, int kept, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!trace) { e.err = "cesx_chain_acf_add: null pointer"; return CESX_EINVAL; }
    if (kept < 1) { e.err = "cesx_chain_acf_add: kept must be >= 1"; return CESX_EINVAL; }
    if (e.ca.none()) { e.err = "cesx_chain_acf_add: cesx_chain_acf_begin has not been called"; return CESX_ESTATE; }
    if (e.ca.added + kept > e.ca.N) { e.err = "cesx_chain_acf_add: more draws than cesx_chain_acf_begin announced"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return chainacf_add(e, trace, kept, (hipStream_t)stream);
}

int cesx_chain_acf_read(cesx_handle h, double* gsum, double* msum, double* m2sum, double* chain_gamma, double* chain_mean, void* stream) {
    if (!h) return CESX_EINVAL;
    Engine& e = *reinterpret_cast<Engine*>(h);
    if (!gsum || !msum || !m2sum) { e.err = "cesx_chain_acf_read: null pointer"; return CESX_EINVAL; }
    if (e.ca.none()) { e.err = "cesx_chain_acf_read: cesx_chain_acf_begin has not been called"; return CESX_ESTATE; }
    if (e.ca.added != e.ca.N) { e.err = "cesx_chain_acf_read: fewer draws were added than cesx_chain_acf_begin announced"; return CESX_ESTATE; }
    SET_DEVICE(e);
    return chainacf_read(e, gsum, msum, m2sum, chain_gamma, chain_mean, (hipStream_t)stream);
}

}  // extern "C"
