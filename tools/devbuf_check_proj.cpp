// Host check of who owns the device memory of GpProjState (ces_amd/csrc/cesx_stages.h), without a device:
//   g++ -std=c++17 -Wall -o tools/devbuf_check_proj tools/devbuf_check_proj.cpp && tools/devbuf_check_proj
// The scenarios of tools/devbuf_check.cpp for the one struct that file does not know (no ROCm include path; dev_alloc /
// dev_free over malloc, with a call that can be made to fail): filled, with every allocation failing in turn, dropped, moved
// over and destructed; after each scenario no block is live, and no pointer was freed that dev_alloc did not hand out or
// that was freed before.  One "ok" line per scenario, exit status 0.  tests/test_gp_proj_host.py builds and runs it.
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
static void ok(const char* what) {
    REQUIRE(g_live.empty()); REQUIRE(g_foreign == 0); REQUIRE(g_twice == 0);
    g_freed.clear(); g_fail_at = -1;
    ++g_scenarios;
    std::printf("ok GpProjState: %s\n", what);
}

// the buffers in the order and with the call cesx_gp_proj_set uses; sz scales the sizes
// (A model of engine.hip kept by hand: an entry point that changes its order, or alloc for ensure, has to change here too.)
#define EN(b, n) do { if (const int rc_ = (b).ensure((size_t)(n) * sz)) return rc_; } while (0)
static int fill(GpProjState& s, size_t sz) {
    s.drop();
    EN(s.R, 64); EN(s.Rt, 64); EN(s.a0, 8);
    s.c_perp = 0.5; s.half_logdet_gamma = -3.0; s.logdet = 1;
    s.k = 2;
    return 0;
}
// what drop() keeps: every buffer (sized by CESX_GP_PROJ_KMAX alone)
static void after_drop(const GpProjState& s, bool full) { REQUIRE(!full || (s.R && s.Rt && s.a0)); }

int main() {
    typedef GpProjState S;
    int N = 0;
    {   // never allocated: nothing to free
        const int frees = g_frees;
        begin();
        { S s; REQUIRE(s.none()); }
        { S s; s.drop(); REQUIRE(s.none()); }
        REQUIRE(g_frees == frees && g_calls == 0);
        ok("default-constructed, dropped, destructed: no dev_free call");
    }
    {   // install, re-install smaller and larger, drop (the buffers are kept), install, destruct
        begin();
        {
            S s;
            REQUIRE(fill(s, 2) == 0); REQUIRE(!s.none());
            N = g_calls;
            REQUIRE(fill(s, 1) == 0); REQUIRE(g_calls == N);      // smaller: no call
            REQUIRE(fill(s, 3) == 0); REQUIRE(!s.none());
            s.drop(); REQUIRE(s.none()); after_drop(s, true);
            REQUIRE(fill(s, 2) == 0); REQUIRE(!s.none());
        }
        ok("install, re-install smaller and larger, drop, install, destruct");
    }
    REQUIRE(N == 3);
    for (int first = 0; first < 2; ++first) {      // every allocation of a first install, and of a re-install over a filled struct, fails in turn
        for (int k = 0; k < N; ++k) {
            S s;
            if (!first) { begin(); REQUIRE(fill(s, 1) == 0); }
            begin(k);
            const int rc = fill(s, 4);             // (larger: a re-install allocates every buffer again)
            REQUIRE(rc != 0); REQUIRE(g_calls == k + 1);
            REQUIRE(s.none());                     // (fill drops first, as the entry point does: a failure leaves no descriptor)
            s.drop(); REQUIRE(s.none()); after_drop(s, false);
        }
        ok(first ? "first install, each allocation failing in turn, drop, destruct" : "re-install, each allocation failing in turn, drop, destruct");
    }
    {   // move-assignment over a filled struct, and from a moved-from one
        begin();
        {
            S a, b;
            REQUIRE(fill(a, 1) == 0); REQUIRE(fill(b, 2) == 0);
            a = std::move(b);
            REQUIRE(!a.none() && a.c_perp == 0.5 && a.half_logdet_gamma == -3.0);
            b = S{};
            S c(std::move(a));
            REQUIRE(!c.none());
        }
        ok("move-assigned over a filled struct, move-constructed");
    }
    std::printf("%d scenarios, all ok\n", g_scenarios);
    return 0;
}
