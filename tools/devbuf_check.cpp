// Host check of who owns the engine's device memory (ces_amd/csrc/devbuf.h, cesx_stages.h), without a device:
//   g++ -std=c++17 -Wall -o tools/devbuf_check tools/devbuf_check.cpp && tools/devbuf_check
// (no ROCm include path: that the two headers compile this way is the check that they are free of hip/).  dev_alloc /
// dev_free are defined here over malloc, with a call that can be made to fail.  Every stage struct is filled, with every
// one of its allocations failing in turn, dropped, moved over and destructed; after each scenario no block is live, and no
// pointer was freed that dev_alloc did not hand out or that was freed before.  One "ok" line per scenario, exit status 0.
// The same source under -fsanitize=address,undefined is the by-hand run NOTEBOOK.md records; tests/test_devbuf_host.py
// runs it plain.
#include "../ces_amd/csrc/cesx_stages.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

static std::set<void*> g_live, g_freed;
static int g_calls = 0, g_fail_at = -1, g_frees = 0, g_foreign = 0, g_twice = 0, g_scenarios = 0;

namespace cesx {
int dev_alloc(void** p, size_t bytes, bool zero) {
    *p = nullptr;
    if (g_calls++ == g_fail_at) return 2;          // (any non-zero code: hipErrorOutOfMemory is 2)
    const size_t len = bytes ? bytes : 8;
    void* q = std::malloc(len);
    if (!q) return 2;
    if (zero) std::memset(q, 0, len);
    g_live.insert(q); g_freed.erase(q);            // (malloc may hand an address out again)
    *p = q;
    return 0;
}
void dev_free(void* p) {
    ++g_frees;
    if (g_live.erase(p)) { g_freed.insert(p); std::free(p); }
    else if (g_freed.count(p)) ++g_twice;
    else ++g_foreign;
}
}  // namespace cesx
using namespace cesx;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static void begin(int fail_at = -1) { g_calls = 0; g_fail_at = fail_at; }
static void ok(const char* who, const char* what) {
    REQUIRE(g_live.empty()); REQUIRE(g_foreign == 0); REQUIRE(g_twice == 0);
    g_freed.clear(); g_fail_at = -1;
    ++g_scenarios;
    std::printf("ok %s: %s\n", who, what);
}

// ---- every buffer of every stage, in the order and with the call (alloc / ensure) its cesx_*_set uses; sz scales the sizes ----
// (A model of engine.hip kept by hand: an entry point that changes its order, or alloc for ensure, has to change here too.)
#define AL(b, n) do { if (const int rc_ = (b).alloc((size_t)(n) * sz)) return rc_; } while (0)
#define EN(b, n) do { if (const int rc_ = (b).ensure((size_t)(n) * sz)) return rc_; } while (0)
static int fill(MhState& s, size_t sz) {
    s.drop();
    EN(s.W, 64); EN(s.Wf, 64); EN(s.LSi, 16); EN(s.Li, 64); EN(s.Li_f, 64); EN(s.lb, 8); EN(s.w, 128); EN(s.xi, 128); EN(s.phi, 32); EN(s.cnt, 32);
    s.kind = 0;
    return 0;
}
static int fill(GpState& s, size_t sz) {
    s.drop();
    AL(s.A, 48); AL(s.c, 4); AL(s.Z, 96); AL(s.par, 12); AL(s.mw, 12); AL(s.alpha, 32); AL(s.Li, 256);
    if (s.ws.bytes < 512 * sz) { if (const int rc = s.ws.alloc(512 * sz, false)) return rc; }      // (launch_gp_predict)
    s.n = 3;
    return 0;
}
static int fill(GpDenseState& s, size_t sz) {
    s.drop();
    EN(s.B, 25); EN(s.Bt, 25); EN(s.g0, 5); EN(s.y, 5); EN(s.Gam, 25);
    s.k = 2;
    return 0;
}
static int fill_fit(GpFitState& s, size_t sz) {
    AL(s.X, 68); AL(s.Y, 34); AL(s.Xs, 256); AL(s.r, 64); AL(s.t, 64); AL(s.alpha, 64); AL(s.A, 2048); AL(s.W, 2048); AL(s.Ki, 2048);
    AL(s.Ld, 1024); AL(s.part, 12); AL(s.theta, 12); AL(s.out, 16); AL(s.idx, 2); AL(s.status, 2);
    return 0;
}
static int fill(GpFitState& s, size_t sz) {
    s.drop();
    if (const int rc = fill_fit(s, sz)) { s.drop(); return rc; }      // (cesx_gpfit_set: nothing stays allocated)
    s.h_out.assign(16, 0.0);
    s.n = 2;
    return 0;
}
static int fill(DarcyState& s, size_t sz) {
    s.drop();
    AL(s.mat, 64); AL(s.idx, 9);
    if (const int rc = s.ws.alloc(90 * sz, false)) return rc;      // (cesx_darcy_set_streamed: the workspace, not zeroed)
    s.streamed = true; s.slots = 3;
    s.K = 4;
    return 0;
}
static int fill(L96State& s, size_t sz) {      // (cesx_lorenz_set: the new times first, the old map stays on a failure)
    DevBuf<double> tnew;
    AL(tnew, 21);
    s.t = std::move(tnew);
    s.desc.n_slow = 5;
    return 0;
}

// what drop() keeps: the buffers sized by the engine's shape alone
static void after_drop(const MhState& s, bool full) { REQUIRE(!full || (s.W && s.Wf && s.LSi && s.Li && s.Li_f && s.lb && s.w && s.xi && s.phi && s.cnt)); }
static void after_drop(const GpState& s, bool full) { REQUIRE(!s.A && !s.c && !s.Z && !s.par && !s.mw && !s.alpha && !s.Li); REQUIRE(!full || s.ws); }
static void after_drop(const GpDenseState& s, bool full) { REQUIRE(!full || (s.B && s.Bt && s.g0 && s.y && s.Gam)); }
static void after_drop(const GpFitState& s, bool) {
    REQUIRE(!s.X && !s.Y && !s.Xs && !s.r && !s.t && !s.alpha && !s.A && !s.W && !s.Ki && !s.Ld && !s.part && !s.theta && !s.out && !s.idx && !s.status);
}
static void after_drop(const DarcyState& s, bool) { REQUIRE(!s.mat && !s.idx && !s.ws && !s.streamed && s.slots == 0); }
static void after_drop(const L96State& s, bool) { REQUIRE(!s.t); }

template <typename S> static void stage(const char* who) {
    int N = 0;
    {   // never allocated: nothing to free
        const int frees = g_frees;
        begin();
        { S s; REQUIRE(s.none()); }
        { S s; s.drop(); REQUIRE(s.none()); }
        REQUIRE(g_frees == frees && g_calls == 0);
        ok(who, "default-constructed, dropped, destructed: no dev_free call");
    }
    {   // install, re-install smaller and larger (the engine-sized buffers are kept: no call), drop, destruct
        begin();
        {
            S s;
            REQUIRE(fill(s, 2) == 0); REQUIRE(!s.none());
            N = g_calls;
            REQUIRE(fill(s, 1) == 0); REQUIRE(fill(s, 3) == 0); REQUIRE(!s.none());
            s.drop(); REQUIRE(s.none()); after_drop(s, true);
            REQUIRE(fill(s, 2) == 0); REQUIRE(!s.none());
        }
        ok(who, "install, re-install smaller and larger, drop, install, destruct");
    }
    REQUIRE(N > 0);
    for (int first = 0; first < 2; ++first) {      // every allocation of a first install, and of a re-install over a filled struct, fails in turn
        for (int k = 0; k < N; ++k) {
            S s;
            if (!first) { begin(); REQUIRE(fill(s, 1) == 0); }
            begin(k);
            const int rc = fill(s, 4);             // (larger: a re-install allocates every buffer again)
            REQUIRE(rc != 0); REQUIRE(g_calls == k + 1);
            s.drop(); REQUIRE(s.none()); after_drop(s, false);
        }
        ok(who, first ? "first install, each allocation failing in turn, drop, destruct" : "re-install, each allocation failing in turn, drop, destruct");
    }
    {   // move-assignment over a filled struct, and from a moved-from one
        begin();
        {
            S a, b;
            REQUIRE(fill(a, 1) == 0); REQUIRE(fill(b, 2) == 0);
            a = std::move(b);
            REQUIRE(!a.none());
            b = S{};
            S c(std::move(a));
            REQUIRE(!c.none());
        }
        ok(who, "move-assigned over a filled struct, move-constructed");
    }
}

int main() {
    stage<MhState>("MhState");
    stage<GpState>("GpState");
    stage<GpDenseState>("GpDenseState");
    stage<GpFitState>("GpFitState");
    stage<DarcyState>("DarcyState");
    stage<L96State>("L96State");
    {   // a failed re-install of the Lorenz '96 map leaves the old sample times
        begin();
        {
            L96State s;
            REQUIRE(fill(s, 1) == 0);
            const double* told = s.t;
            begin(0);
            REQUIRE(fill(s, 2) != 0); REQUIRE(!s.none()); REQUIRE(s.t.get() == told);
        }
        ok("L96State", "a failed re-install leaves the old map");
    }
    {
        begin();
        {
        DevBuf<double> b;
        REQUIRE(!b); REQUIRE(b.ensure(64) == 0);
        double* p0 = b;
        REQUIRE(b.bytes == 64 && p0[7] == 0.0);
        p0[3] = 1.5;
        REQUIRE(b.ensure(32) == 0); REQUIRE(b.get() == p0 && b.bytes == 64 && *(b + 3) == 1.5 && g_calls == 1);      // smaller: kept
        REQUIRE(b.ensure(128, false) == 0); REQUIRE(b.bytes == 128 && g_calls == 2 && g_live.size() == 1);       // larger: the old one freed
        REQUIRE(b.alloc(0) == 0); REQUIRE(b && g_live.size() == 1);                                               // never an empty allocation
        begin(0);
        REQUIRE(b.ensure(256) != 0); REQUIRE(!b && b.bytes == 0);                                                 // a failure leaves it empty
        DevBuf<void> v;
        begin();
        REQUIRE(v.alloc(16) == 0);
        REQUIRE(static_cast<const float*>(v.get())[3] == 0.0f);
        v.reset(); v.reset();
        }
        ok("DevBuf", "ensure smaller then larger, alloc(0), a failed ensure, reset twice");
    }
    {   // Engine::core as core_alloc fills it: a failure in the middle, the vector growing (its elements move) before and after
        void* handed[40] = {};
        begin(17);
        {
            std::vector<DevBuf<void>> core;
            int n = 0;
            for (; n < 40; ++n) {
                DevBuf<void> b;
                if (b.alloc(24)) break;
                handed[n] = b.get();
                core.push_back(std::move(b));
            }
            REQUIRE(n == 17 && core.size() == 17 && g_live.size() == 17);
            g_fail_at = -1;
            for (; n < 40; ++n) { DevBuf<void> b; REQUIRE(b.alloc(24, false) == 0); handed[n] = b.get(); core.push_back(std::move(b)); }
            for (int i = 0; i < 40; ++i) REQUIRE(core[(size_t)i].get() == handed[i]);      // the pointers handed out stay good
        }
        ok("core", "40 buffers pushed with allocation 17 failing, destructed");
    }
    std::printf("%d scenarios, all ok\n", g_scenarios);
    return 0;
}
