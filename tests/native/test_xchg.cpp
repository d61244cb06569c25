// Host test of the small-call exchange's slot protocol
// (openshmem-async_amd/csrc/node.cpp xchg_claim / xchg_finish) with real
// processes and no GPU: N forked PEs map one exchange block without
// page-locking it (xchg_attach(false)) and run the same random sequence of
// calls on random, overlapping active sets (PE_start, stride, size);
// non-members skip.  Per call a member does what staging.cpp xchg_reduce does
// on the host side:
//     xchg_claim                      (wait for the readers of my previous call)
//     fill my whole slot              (8-byte words f(call, me, word))
//     node::barrier                   (the entry barrier)
//     read every member's whole slot  (every word must be f(call, member, word))
//     xchg_finish                     (done reading; NO exit barrier)
// On a seeded random quarter of the (call, PE) pairs the reader sleeps
// 50-300 us between the barrier and its check, so the writers run ahead into
// their next calls, on other sets too: only the per-pair done counts keep
// them from overwriting a slot that is still being read.
//
// A mismatch is recorded once in shared memory; every PE then finishes the
// sequence without further checks or sleeps (nobody waits out a barrier
// timeout), and the program prints what was read and exits 1.  A clean run
// prints "ok <calls> calls, <N> PEs".
//
// --write-before-claim is the negative control: the PE fills its slot before
// xchg_claim instead of after it, i.e. without waiting for its readers, and
// every reader sleeps on every call.  That run must exit 1.
//
// The slot size is node::kXchgSlotBytes wherever it is used.
#include <sys/mman.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <vector>

#include "shmem_reduce_mi355x.h"
#include "node.h"

// The two runtime hooks node.cpp calls (runtime.cpp in the library).
namespace shmx {
void trace(int, const char *, ...) {}
[[noreturn]] void fatal(const char *what, const char *detail) {
    std::fprintf(stderr, "FATAL %s: %s\n", what, detail);
    std::abort();
}
}  // namespace shmx

namespace {

struct Set {
    int start, step, size;
};

constexpr int kWords = (int)(shmx::node::kXchgSlotBytes / sizeof(uint64_t));

uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Word w of PE pe's slot in call c.
uint64_t f(int c, int pe, int w) {
    return mix(((uint64_t)c << 20 | (uint64_t)pe << 12 | (uint64_t)w) + 0x9E3779B97F4A7C15ull);
}

// The first mismatch, recorded by the reader that saw it.
struct Report {
    std::atomic<int> bad;
    int call, reader, writer, word;
    uint64_t got, want;
};

void fill(int c, int pe) {
    uint64_t *slot = reinterpret_cast<uint64_t *>(shmx::node::xchg_host(pe));
    for (int w = 0; w < kWords; ++w) slot[w] = f(c, pe, w);
}

void sleep_us(unsigned us) {
    struct timespec ts = {0, (long)us * 1000};
    nanosleep(&ts, nullptr);
}

int run_pe(int pe, int npes, const std::vector<Set> &calls, bool control, Report *rep, const unsigned char *key,
           size_t keylen) {
    namespace node = shmx::node;
    if (!node::attach(pe, npes, key, keylen)) return 10;
    if (!node::xchg_attach(false) || !node::xchg_host(pe) || node::xchg_dev(pe)) return 11;
    node::barrier(0, 1, npes);
    uint64_t counts[node::kMaxPes];
    for (int c = 0; c < (int)calls.size(); ++c) {
        const Set &s = calls[c];
        const int idx = pe - s.start;
        if (idx < 0 || idx % s.step || idx / s.step >= s.size) continue;
        if (control) fill(c, pe);   // before the readers of the previous call are done
        node::xchg_claim(s.start, s.step, s.size, counts);
        if (!control) fill(c, pe);
        node::barrier(s.start, s.step, s.size);
        if (!rep->bad.load(std::memory_order_acquire)) {
            const uint64_t h = mix((uint64_t)c * 64 + pe + 0x5EED);
            if (control || (h & 3) == 0) sleep_us(50 + (unsigned)((h >> 8) % 251));
            for (int i = 0; i < s.size; ++i) {
                const int q = s.start + i * s.step;
                const uint64_t *slot = reinterpret_cast<const uint64_t *>(node::xchg_host(q));
                int w = 0;
                while (w < kWords && slot[w] == f(c, q, w)) ++w;
                if (w == kWords) continue;
                int none = 0;
                if (rep->bad.compare_exchange_strong(none, 2)) {
                    rep->call = c, rep->reader = pe, rep->writer = q, rep->word = w;
                    rep->got = slot[w], rep->want = f(c, q, w);
                    rep->bad.store(1, std::memory_order_release);
                }
                break;
            }
        }
        node::xchg_finish(s.start, s.step, s.size, counts);
    }
    node::barrier(0, 1, npes);
    node::detach(pe == 0);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    int npes = 6, ncalls = 3000, npos = 0;
    bool control = false;
    for (int a = 1; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--write-before-claim")) control = true;
        else if (npos++ == 0) npes = std::atoi(argv[a]);
        else ncalls = std::atoi(argv[a]);
    }
    if (npes < 2 || npes > 8 || ncalls < 1) {
        std::fprintf(stderr, "usage: test_xchg [--write-before-claim] NPES(2-8) [NCALLS]\n");
        return 2;
    }
    // the same call sequence on every PE
    std::mt19937 rng(4242);
    std::vector<Set> calls;
    for (int c = 0; c < ncalls; ++c) {
        const int step = 1 << (rng() % 3);
        const int start = (int)(rng() % npes);
        const int maxsize = (npes - 1 - start) / step + 1;
        calls.push_back(Set{start, step, 1 + (int)(rng() % maxsize)});
    }
    void *shared = mmap(nullptr, sizeof(Report), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (shared == MAP_FAILED) return 3;
    Report *rep = new (shared) Report{};
    unsigned char key[16];
    for (int i = 0; i < 16; ++i) key[i] = (unsigned char)(getpid() >> (i % 4 * 8)) ^ (unsigned char)(i + 0x58);
    std::vector<pid_t> kids;
    for (int pe = 0; pe < npes; ++pe) {
        const pid_t k = fork();
        if (k == 0) _exit(run_pe(pe, npes, calls, control, rep, key, sizeof key));
        kids.push_back(k);
    }
    int fails = 0;
    for (pid_t k : kids) {
        int st = 0;
        waitpid(k, &st, 0);
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) ++fails;
    }
    if (rep->bad.load()) {
        std::printf("FAIL call %d: PE %d read word %d of PE %d's slot as %016llx, not %016llx: the slot was "
                    "written again while a reader of its previous call was still reading it\n",
                    rep->call, rep->reader, rep->word, rep->writer, (unsigned long long)rep->got,
                    (unsigned long long)rep->want);
        return 1;
    }
    if (fails) {
        std::printf("FAIL %d PEs did not finish\n", fails);
        return 3;
    }
    std::printf("ok %d calls, %d PEs\n", ncalls, npes);
    return 0;
}
