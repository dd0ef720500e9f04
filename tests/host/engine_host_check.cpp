// engine_host_check.cpp -- the rule of engine_host.h, checked on the CPU against fake_hip.cpp: whenever an engine's lock is free
// its stream is idle, so host memory a call handed to the stream is not referenced after any return, failed or not; and the
// success path pays no wait for it.  Exits 0 when every check holds, otherwise prints the first one that does not and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "engine_host.h"
#include "fake_hip.h"

using namespace ssf;
using namespace ssf::eng;

namespace {

struct Work : WorkBase {
    Buf in, out, tab, more;
    PwLeaves leaves;
};
using Call = CallT<Work>;

int g_check = 0;
void begin(int number) {
    g_check = number;
    fake.reset();
}
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            std::printf("FAILED check %d: ", g_check);      \
            std::printf(__VA_ARGS__);                       \
            std::printf("  [%s]\n", #cond);                 \
            std::exit(1);                                   \
        }                                                   \
    } while (0)

bool begins(const std::string &s, const char *head) { return s.rfind(head, 0) == 0; }

// what the stream still holds when the locals of an entry start to die: declared after them, so it goes first
struct Probe {
    int &pending;
    explicit Probe(int &p) : pending(p) { pending = -1; }
    ~Probe() { pending = fake.pending(); }
};

std::vector<double> ramp(size_t n, double first) {
    std::vector<double> v(n);
    std::iota(v.begin(), v.end(), first);
    return v;
}

// ---- 1: input() from the caller's array, then a need() that fails
int entry_input_then_oom(const double *x, size_t n, int &pending_at_exit, std::string *err) {
    Call c(0, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    Probe probe(pending_at_exit);
    if (!c.input(x, w.in, n * sizeof(double))) return c.rc;
    fake.fail_malloc_at = 1;
    if (!c.need(w.more, w.more.cap + 64)) return c.rc;
    return c.sync() ? SSF_OK : c.rc;
}
void check_caller_array() {
    begin(1);
    const std::vector<double> x = ramp(1000, 1.0);
    std::string err;
    int pending = -1;
    const int rc = entry_input_then_oom(x.data(), x.size(), pending, &err);
    CHECK(rc == SSF_ERR_OOM, "rc = %d, expected SSF_ERR_OOM", rc);
    CHECK(begins(err, "hipMalloc: "), "text \"%s\"", err.c_str());
    CHECK(pending == 0, "rc = %d with %d copy pending when the entry's locals died: it would read the caller's array", rc, pending);
    CHECK(fake.pending() == 0, "%d copy pending after the return", fake.pending());
}

// ---- 2: the same with a local vector as the source of an upload and as the target of deliver()
int entry_locals_then_oom(int &pending_at_exit, bool &arrived, std::string *err) {
    Call c(0, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    struct Arrived {                           // dies after probe and before res: looks at res once the failure has returned
        const std::vector<double> &res;
        bool &flag;
        ~Arrived() { flag = res[0] == 7.0 && res.back() == 7.0 + (double)(res.size() - 1); }
    };
    const std::vector<double> tab = ramp(300, 7.0);
    std::vector<double> res(300, 0.0);
    Arrived look{res, arrived};
    Probe probe(pending_at_exit);
    if (!c.upload(w.tab, tab)) return c.rc;
    if (!c.sync()) return c.rc;                                     // (so that deliver has something to bring back)
    if (!c.upload(w.tab, tab) || !c.deliver(res.data(), w.tab.p, res.size() * sizeof(double))) return c.rc;
    fake.fail_malloc_at = 1;
    if (!c.need(w.more, w.more.cap + 64)) return c.rc;
    return c.sync() ? SSF_OK : c.rc;
}
void check_local_vectors() {
    begin(2);
    std::string err;
    int pending = -1;
    bool arrived = false;
    const int rc = entry_locals_then_oom(pending, arrived, &err);
    CHECK(rc == SSF_ERR_OOM && begins(err, "hipMalloc: "), "rc = %d, text \"%s\"", rc, err.c_str());
    CHECK(pending == 0, "%d copies pending when the local vectors died", pending);
    CHECK(arrived, "the result had not reached the local vector when it died");
    CHECK(fake.pending() == 0, "%d copies pending after the return", fake.pending());
}

// ---- 3: the constructor's own failure, and a failure of a call without a stream (w is NULL)
void check_no_stream() {
    begin(3);
    std::string err;
    fake.fail_set_device = true;
    {
        Call c(0, &err, false);
        CHECK(c.rc == SSF_ERR_HIP && begins(err, "hipSetDevice: ") && !c.w, "rc = %d, text \"%s\"", c.rc, err.c_str());
    }
    err.clear();
    {
        Call c(0, &err);                                             // with a stream wanted: it fails before there is one
        CHECK(c.rc == SSF_ERR_HIP && begins(err, "hipSetDevice: ") && !c.w, "rc = %d, text \"%s\"", c.rc, err.c_str());
    }
    fake.fail_set_device = false;
    err.clear();
    Call c(0, &err, false);
    CHECK(c.rc == SSF_OK && !c.w, "rc = %d", c.rc);
    CHECK(!c.ok(hipErrorOutOfMemory, "hipMalloc") && c.rc == SSF_ERR_OOM && err == "hipMalloc: out of memory", "rc = %d, text \"%s\"", c.rc, err.c_str());
    CHECK(fake.waits == 0, "%d waits without a stream", fake.waits);
}

// ---- 4: the drain's own wait fails, and so does a later step: the first failure stays
void check_first_failure_wins() {
    begin(4);
    std::string err;
    Call c(0, &err);
    CHECK(c.rc == SSF_OK, "rc = %d", c.rc);
    fake.fail_malloc_at = 1, fake.fail_wait = true;
    CHECK(!c.need(c.w->more, c.w->more.cap + 64), "the allocation did not fail");
    CHECK(fake.waits == 1, "%d waits at the failure, expected the one drain", fake.waits);
    CHECK(!c.sync() && !c.fft_fail("rocfft_execute failed") && !c.reject(SSF_ERR_BAD_ARG, "later"), "a failed step returned true");
    CHECK(c.rc == SSF_ERR_OOM && err == "hipMalloc: out of memory", "rc = %d, text \"%s\"", c.rc, err.c_str());
}

// ---- 5: nothing added to the success path
int entry_success(const double *x, double *y, size_t n, const std::vector<double> &tab, std::string *err) {
    Call c(0, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const void *xd = c.input(x, w.in, n * sizeof(double));
    if (!xd || !c.upload(w.tab, tab)) return c.rc;
    if (!c.deliver(y, xd, n * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}
void check_success_path() {
    begin(5);
    const std::vector<double> x = ramp(500, 3.0), tab = ramp(64, 0.0);
    std::vector<double> y(500, 0.0);
    std::string err;
    CHECK(entry_success(x.data(), y.data(), x.size(), tab, &err) == SSF_OK, "text \"%s\"", err.c_str());
    CHECK(fake.waits == 1 && fake.copies == 3, "%d waits and %d copies, expected 1 and 3", fake.waits, fake.copies);
    CHECK(y == x, "the result is not the input");

    fake.reset();
    Call c(0, &err);
    long long nleaf = 0;
    const long long *start = nullptr;
    const long long n = 100000;
    CHECK(pairwise_leaves(c, c.w->leaves, n, nleaf, start), "text \"%s\"", err.c_str());
    CHECK(fake.waits == 0 && fake.copies == 1, "new n: %d waits and %d copies, expected 0 and 1", fake.waits, fake.copies);
    CHECK(pairwise_leaves(c, c.w->leaves, n, nleaf, start), "text \"%s\"", err.c_str());
    CHECK(fake.waits == 0 && fake.copies == 1, "same n again: %d waits and %d copies, expected 0 and 1", fake.waits, fake.copies);
    CHECK(c.sync() && start[0] == 0 && start[nleaf] == n, "the leaves on the device run from %lld to %lld", start[0], start[nleaf]);
}

// ---- 6: upload() sizes the buffer and the data arrives, also when it has to grow
void check_upload_grows() {
    begin(6);
    std::string err;
    Call c(0, &err);
    Buf &b = c.w->more;
    const std::vector<double> small = ramp(b.cap / sizeof(double) + 10, 1.0), large = ramp(4 * small.size() + 3, -5.0);
    for (const std::vector<double> *v : {&small, &large}) {
        const size_t before = b.cap, bytes = v->size() * sizeof(double);
        CHECK(c.upload(b, *v) && c.sync(), "text \"%s\"", err.c_str());
        CHECK(b.cap == bytes && b.cap > before, "capacity %zu after %zu, wanted %zu", b.cap, before, bytes);
        CHECK(on_device(b.p) && !std::memcmp(b.p, v->data(), bytes), "the device copy differs from the host data");
    }
    CHECK(c.upload(b, small.data(), 8 * sizeof(double)) && c.sync() && b.cap == large.size() * sizeof(double), "a smaller upload changed the capacity");
}

// ---- 7: reject()
int entry_reject(const double *x, size_t n, int &pending_at_exit, std::string *err) {
    Call c(0, err);
    if (c.rc) return c.rc;
    Probe probe(pending_at_exit);
    if (!c.input(x, c.w->in, n * sizeof(double))) return c.rc;
    if (n) c.reject(SSF_ERR_BAD_ARG, "no correlation peak");
    return c.rc;
}
void check_reject() {
    begin(7);
    const std::vector<double> x = ramp(10, 0.0);
    std::string err;
    int pending = -1;
    const int rc = entry_reject(x.data(), x.size(), pending, &err);
    CHECK(rc == SSF_ERR_BAD_ARG && err == "no correlation peak", "rc = %d, text \"%s\"", rc, err.c_str());
    CHECK(pending == 0 && fake.pending() == 0 && fake.waits == 1, "%d copies pending, %d waits", pending, fake.waits);
}

}  // namespace

int main() {
    void (*const checks[])() = {check_caller_array, check_local_vectors, check_no_stream, check_first_failure_wins,
                                check_success_path, check_upload_grows, check_reject};
    for (auto check : checks) {
        check();
        std::printf("ok %d\n", g_check);
    }
    std::printf("engine_host: all %d checks hold\n", g_check);
    return 0;
}
