// Host test of the staging copies (openshmem-async_amd/csrc/copy_gang.h):
// every copy of a CopyGang, started in the background or made with the caller
// taking a piece, equals its source and leaves the 64 bytes on either side of
// the destination alone, for gangs of 0, 1, 2, 3 and 8 pinned workers and of
// 3 unpinned ones (empty CPU sets), at the sizes around the 64-byte piece rounding and copy()'s 4 MiB
// threshold, at destination offsets 0, 1 and 31 from 32-byte alignment (the
// streaming copy's head and tail), with and without streaming stores.  Then
// the ways staging.cpp uses them: back-to-back starts, a wait with nothing
// started, two gangs at once over disjoint buffers (the pipeline's in and out
// gangs), and copy() from two threads at once (the second finds the gang busy
// and copies alone).  Prints "ok <copies checked>".
#include <sched.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "copy_gang.h"

using shmx::CopyGang;
using Sets = std::vector<std::vector<int>>;

static constexpr size_t kCanary = 64, MiB = size_t(1) << 20;
static constexpr unsigned char kMark = 0xA5;
static const size_t kSizes[] = {0, 1, 63, 64, 65, 4 * MiB - 1, 4 * MiB, 4 * MiB + 65, 16 * MiB + 7};
static const size_t kMax = 16 * MiB + 7;
static long g_checked = 0;

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                              \
            std::fprintf(stderr, "\n");                                     \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// A destination of up to kMax bytes at `off` past 32-byte alignment, between canaries.
struct Dest {
    explicit Dest(size_t off) : raw((unsigned char *)std::aligned_alloc(64, (2 * kCanary + 32 + kMax + 63) & ~size_t(63))) {
        CHECK(raw, "no memory");
        p = raw + kCanary + off;
    }
    ~Dest() { std::free(raw); }
    Dest(const Dest &) = delete;
    void arm(size_t bytes) {
        std::memset(p - kCanary, kMark, kCanary);
        std::memset(p, 0, bytes);
        std::memset(p + bytes, kMark, kCanary);
    }
    void check(const unsigned char *src, size_t bytes, const char *what) {
        CHECK(std::memcmp(p, src, bytes) == 0, "%s: %zu bytes differ from the source", what, bytes);
        for (size_t i = 0; i < kCanary; ++i)
            CHECK(p[-1 - (long)i] == kMark && p[bytes + i] == kMark, "%s: %zu bytes: canary hit", what, bytes);
        ++g_checked;
    }
    unsigned char *raw, *p;
};

static std::vector<unsigned char> make_source() {
    std::vector<unsigned char> s(kMax + 8);
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (auto &b : s) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        b = (unsigned char)(x >> 32);
        if (b == kMark) b = 0;     // the source never looks like a canary
    }
    return s;
}

// `n` workers, worker i on the i-th allowed CPU (wrapping), or unpinned
static Sets sets(unsigned n, bool pinned) {
    std::vector<int> allowed;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (pinned && sched_getaffinity(0, sizeof set, &set) == 0)
        for (int c = 0; c < CPU_SETSIZE; ++c)
            if (CPU_ISSET(c, &set)) allowed.push_back(c);
    Sets s(n);
    for (unsigned i = 0; i < n && !allowed.empty(); ++i) s[i] = {allowed[i % allowed.size()]};
    return s;
}

int main() {
    const std::vector<unsigned char> source = make_source();
    const unsigned char *src = source.data() + 3;     // an unaligned source
    for (unsigned nthreads : {0u, 1u, 2u, 3u, 8u}) {
        for (int pinned = 1; pinned >= (nthreads == 3 ? 0 : 1); --pinned) {   // 3 workers also unpinned
            CopyGang g(sets(nthreads, pinned != 0));
            g.wait();     // nothing started
            for (size_t off : {size_t(0), size_t(1), size_t(31)}) {
                Dest d(off);
                for (size_t bytes : kSizes) {
                    for (int nt = 0; nt < 2; ++nt) {
                        d.arm(bytes);
                        g.start(d.p, src, bytes, nt != 0);
                        g.wait();
                        d.check(src, bytes, "start/wait");
                    }
                    // the caller takes the first of nthreads + 1 pieces
                    d.arm(bytes);
                    g.copy(d.p, src, bytes);
                    d.check(src, bytes, "copy");
                }
            }
        }
    }
    {
        // back to back: the second start waits for the first copy itself
        CopyGang g(sets(3, true));
        Dest a(1), b(31);
        const size_t na = 4 * MiB + 65, nb = 65;
        a.arm(na), b.arm(nb);
        g.start(a.p, src, na, true);
        g.start(b.p, src + 5, nb, false);
        g.wait();
        g.wait();
        a.check(src, na, "first of two starts");
        b.check(src + 5, nb, "second of two starts");
    }
    {
        // the pipeline's use: the in gang and the out gang copy at once,
        // chunk after chunk, each started as soon as its last copy is done
        CopyGang in(sets(4, true)), out(sets(4, false));
        Dest a(0), b(31);
        const size_t n = 4 * MiB + 65;
        for (int k = 0; k < 8; ++k) {
            a.arm(n), b.arm(n);
            in.start(a.p, src + k, n, false);
            out.start(b.p, src + 2 * k, n, true);
            in.wait();
            a.check(src + k, n, "in gang");
            out.wait();
            b.check(src + 2 * k, n, "out gang");
        }
    }
    {
        // copy() from two threads at once: one gets the workers, the other
        // finds the gang busy and copies alone; both are whole
        CopyGang g(sets(3, false));
        Dest a(1), b(0);
        const size_t n = 16 * MiB + 7;
        for (int k = 0; k < 6; ++k) {
            a.arm(n), b.arm(n);
            std::thread other([&] { g.copy(b.p, src + 1, n); });
            g.copy(a.p, src, n);
            other.join();
            a.check(src, n, "copy, this thread");
            b.check(src + 1, n, "copy, the other thread");
        }
    }
    std::printf("ok %ld\n", g_checked);
    return 0;
}
