// Stand-alone check of csrc/ctx_mem.hpp (built and run by tests/test_ctx_mem_host.py with the host compiler and its sanitizers).
// The allocator policy is a counting malloc / free that can be told to fail on its k-th call: the owner's release, refusal, group
// rollback and regrow, and the scratch guard on every way out of a function.  The sanitizers watch for the leak and the double free
// that the counters could miss.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../vbmatrixfactorization.jl_amd/csrc/ctx_mem.hpp"

struct Counting {
    static int calls, fail_at, frees, bad_frees;
    static std::set<void*> held;
    static void reset(int fail = 0) { calls = 0; fail_at = fail; frees = 0; }
    static int alloc(void** p, size_t bytes) {
        if (++calls == fail_at) return 2;                 // (an out-of-memory code; *p is left alone, as the device allocator leaves it)
        *p = std::malloc(bytes);
        held.insert(*p);
        return 0;
    }
    static void free(void* p) {
        ++frees;
        if (!held.erase(p)) { ++bad_frees; return; }      // never allocated, or freed twice
        std::free(p);
    }
};
int Counting::calls = 0, Counting::fail_at = 0, Counting::frees = 0, Counting::bad_frees = 0;
std::set<void*> Counting::held;

using Owner = vbmf::MemOwner<Counting>;
template <class T>
using Tmp = vbmf::Scratch<Counting, T>;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// a context in miniature: typed pointer fields of the kinds vbmf_ctx has, an array among them
struct Ctx {
    double *a = nullptr, *b = nullptr, *c = nullptr;
    float *f[2] = {nullptr, nullptr}, *g = nullptr, *h = nullptr;
    int* i = nullptr;
    unsigned char* m = nullptr;
    long long* r = nullptr;
    double *s = nullptr, *t = nullptr;
    size_t bags_bytes = 0;
    Owner mem;
};

static void owner_release() {
    Counting::reset();
    Ctx x;
    const size_t sizes[10] = {8, 16, 24, 4, 4, 400, 12, 7, 64, 1};
    int rc = x.mem.acquire(x.a, sizes[0]);
    rc |= x.mem.acquire(x.b, sizes[1]);
    rc |= x.mem.acquire(x.c, sizes[2]);
    rc |= x.mem.acquire(x.f[0], sizes[3]);
    rc |= x.mem.acquire(x.f[1], sizes[4]);
    rc |= x.mem.acquire(x.g, sizes[5]);
    rc |= x.mem.acquire(x.i, sizes[6]);
    rc |= x.mem.acquire(x.m, sizes[7]);
    rc |= x.mem.acquire(x.r, sizes[8]);
    rc |= x.mem.acquire(x.s, sizes[9]);
    CHECK(rc == 0 && x.mem.live() == 10 && x.mem.live_bytes() == 540 && Counting::held.size() == 10);
    CHECK(x.a && x.b && x.c && x.f[0] && x.f[1] && x.g && x.i && x.m && x.r && x.s);
    x.mem.release_all();
    CHECK(Counting::frees == 10 && Counting::held.empty() && x.mem.live() == 0 && x.mem.live_bytes() == 0);
    CHECK(!x.a && !x.b && !x.c && !x.f[0] && !x.f[1] && !x.g && !x.i && !x.m && !x.r && !x.s);
    x.mem.release_all();                                  // a second one is a no-op
    CHECK(Counting::frees == 10 && Counting::bad_frees == 0);
    {   // an owner that goes out of scope releases too (a context deleted on a failed create)
        Ctx y;
        CHECK(y.mem.acquire(y.a, 32) == 0 && y.mem.acquire(y.i, 32) == 0);
    }
    CHECK(Counting::frees == 12 && Counting::held.empty());
}

static void owner_refusal() {
    Counting::reset();
    Ctx x;
    CHECK(x.mem.acquire(x.a, 4 * sizeof(double)) == 0);
    for (int k = 0; k < 4; ++k) x.a[k] = 1.5 * k;
    double* const was = x.a;
    const int calls = Counting::calls;
    CHECK(x.mem.acquire(x.a, 1024) == vbmf::MEM_SLOT_BUSY);
    CHECK(x.a == was && Counting::calls == calls && Counting::frees == 0 && x.mem.live() == 1 && x.mem.live_bytes() == 4 * sizeof(double));
    for (int k = 0; k < 4; ++k) CHECK(x.a[k] == 1.5 * k);
}

// gram_prepare in miniature: eight buffers after a mark, each acquired only if the ones before it were; on failure, rollback
static int group_of_eight(Ctx& x) {
    const size_t m = x.mem.mark();
    int rc = x.mem.acquire(x.f[0], 100);
    if (rc == 0) rc = x.mem.acquire(x.f[1], 100);
    if (rc == 0) rc = x.mem.acquire(x.g, 200);
    if (rc == 0) rc = x.mem.acquire(x.h, 50);
    if (rc == 0) rc = x.mem.acquire(x.r, 64);
    if (rc == 0) rc = x.mem.acquire(x.m, 3);
    if (rc == 0) rc = x.mem.acquire(x.s, 80);
    if (rc == 0) rc = x.mem.acquire(x.t, 88);
    if (rc != 0) x.mem.rollback(m);
    return rc;
}

static void group_failure_at_every_k() {
    for (int k = 1; k <= 9; ++k) {                        // k = 9: nothing fails
        Counting::reset();
        Ctx x;
        CHECK(x.mem.acquire(x.a, 3 * sizeof(double)) == 0 && x.mem.acquire(x.b, sizeof(double)) == 0 && x.mem.acquire(x.i, 2 * sizeof(int)) == 0);
        x.a[0] = 1.0; x.a[1] = 2.0; x.a[2] = 3.0; x.b[0] = -4.0; x.i[0] = 5; x.i[1] = 6;
        Counting::reset(k);
        const int rc = group_of_eight(x);
        if (k <= 8) {
            CHECK(rc == 2 && x.mem.live() == 3 && Counting::held.size() == 3 && Counting::frees == k - 1);
            CHECK(x.mem.live_bytes() == 4 * sizeof(double) + 2 * sizeof(int));
            CHECK(!x.f[0] && !x.f[1] && !x.g && !x.h && !x.r && !x.m && !x.s && !x.t);
            Counting::reset();
            CHECK(group_of_eight(x) == 0);                // a later call starts from empty slots and succeeds
        } else {
            CHECK(rc == 0);
        }
        CHECK(x.mem.live() == 11 && x.f[0] && x.f[1] && x.g && x.h && x.r && x.m && x.s && x.t);
        CHECK(x.a && x.b && x.i && x.a[0] == 1.0 && x.a[1] == 2.0 && x.a[2] == 3.0 && x.b[0] == -4.0 && x.i[0] == 5 && x.i[1] == 6);
    }
    CHECK(Counting::held.empty() && Counting::bad_frees == 0);
}

// bags_reserve in miniature (host_bags.hpp): the one buffer that grows.  It never shrinks: a request that fits is served from what
// is held, with no call to the allocator -- the size test is the call site's, regrow() itself always frees and allocates.
static int reserve(Ctx& x, size_t bytes, double** d) {
    if (bytes > x.bags_bytes) {
        x.bags_bytes = 0;
        const int rc = x.mem.regrow(x.s, bytes);
        if (rc != 0) return rc;
        x.bags_bytes = bytes;
    }
    *d = x.s;
    return 0;
}

static void regrow() {
    Counting::reset();
    Ctx x;
    double* d = nullptr;
    CHECK(x.mem.acquire(x.a, 8) == 0);
    CHECK(reserve(x, 64, &d) == 0 && d == x.s && d && x.mem.live() == 2 && Counting::frees == 0);      // the first: nothing to free
    void* const first = x.s;
    CHECK(reserve(x, 256, &d) == 0 && d == x.s && x.mem.live() == 2 && x.mem.live_bytes() == 8 + 256);
    CHECK(Counting::frees == 1 && !Counting::held.count(first) && Counting::held.size() == 2);         // the old block, exactly once
    std::memset(x.s, 0, 256);
    const int calls = Counting::calls;
    double* const big = x.s;
    CHECK(reserve(x, 32, &d) == 0 && d == big && x.s == big && Counting::calls == calls && Counting::frees == 1 && x.bags_bytes == 256);
    Counting::reset(1);
    CHECK(reserve(x, 512, &d) == 2);                      // the new allocation fails: the slot is null, one allocation fewer
    CHECK(!x.s && x.bags_bytes == 0 && x.mem.live() == 1 && Counting::frees == 1 && Counting::held.size() == 1);
    Counting::reset();
    CHECK(reserve(x, 32, &d) == 0 && d == x.s && d && x.mem.live() == 2);                               // and the next call recovers
    x.mem.release_all();
    CHECK(Counting::frees == 2 && Counting::held.empty() && Counting::bad_frees == 0 && !x.a && !x.s);
}

#define TRY_(expr)                \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)
static int step(int rc) { return rc; }

static int scratch_user(int early, int step_rc, const double** seen) {
    Tmp<double> tmp;
    TRY_(tmp.alloc(16 * sizeof(double)));
    tmp[3] = 7.0;                                         // used as the plain pointer it stands for
    *seen = tmp.get();
    if (tmp.alloc(8) != vbmf::MEM_SLOT_BUSY) return -9;
    if (early) return 5;                                  // out of the middle
    TRY_(step(step_rc));                                  // out through the file's idiom
    return tmp[3] == 7.0 ? 0 : -8;
}

static void scratch() {
    const double* seen = nullptr;
    Counting::reset();
    CHECK(scratch_user(0, 0, &seen) == 0 && seen && Counting::calls == 1 && Counting::frees == 1 && Counting::held.empty());
    CHECK(scratch_user(1, 0, &seen) == 5 && Counting::frees == 2 && Counting::held.empty());
    CHECK(scratch_user(0, -3, &seen) == -3 && Counting::frees == 3 && Counting::held.empty());
    Counting::reset(1);
    seen = nullptr;
    CHECK(scratch_user(0, 0, &seen) == 2 && !seen && Counting::frees == 0);      // nothing allocated, nothing freed
    Counting::reset();
    {
        Tmp<void> raw;                                    // the staging buffer of vbmf_set_Y_rows is untyped
        CHECK(raw.alloc(10) == 0 && raw.get());
        raw.reset();
        CHECK(!raw.get() && Counting::frees == 1);
        CHECK(raw.alloc(20) == 0);                        // RunFrame arms its trace again in the next run
    }
    CHECK(Counting::frees == 2 && Counting::held.empty() && Counting::bad_frees == 0);
}

int main() {
    owner_release();
    owner_refusal();
    group_failure_at_every_k();
    regrow();
    scratch();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ctx_mem: release, refusal, rollback at every k, regrow and the scratch guard hold\n");
    return 0;
}
