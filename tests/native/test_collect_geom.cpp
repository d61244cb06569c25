// collect_plan (set_geom.h), the one definition the collect kernels and this
// program share, against a brute-force model; host only, meant for
// -fsanitize=address,undefined (tests/test_collect_geom_host.py).
//
// For P in 1..16, every member m, element sizes 4 and 8:
//   - counts drawn from {0, 1, 3, 64, 1013} (every combination up to P = 4,
//     a fixed pseudo-random draw of them above), all-zero counts and a single
//     non-zero count in every position;
//   - capacity equal to the total (no overflow) and one short of it
//     (overflow), and a capacity far above it;
//   - one poison count in every position: overflow whatever the capacity;
//   - counts near 2^63 whose sum passes 2^64: the sum saturates, never wraps,
//     and the plan overflows.
// Without overflow, member i's offset is the model's prefix sum, every member
// computes the same offsets and total, the segments of m's order tile
// [0, total) without overlap, the order starts at the first non-empty member
// after m, wrapping, with m's own copy last, and skips exactly the empty
// members.  With overflow the plan has no segment.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "set_geom.h"

using namespace shmx;
typedef unsigned long long u64;

static long g_checks = 0;
static int g_P, g_m;
static u64 g_cap;

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        ++g_checks;                                                                                      \
        if (!(cond)) {                                                                                   \
            std::printf("FAIL %s:%d: %s  (P=%d m=%d capacity=%llu)\n", __FILE__, __LINE__, #cond, g_P, g_m, \
                        g_cap);                                                                          \
            std::exit(1);                                                                                \
        }                                                                                                \
    } while (0)

// the model: 128-bit sums, nothing shared with collect_plan
struct Model {
    bool overflow;
    unsigned __int128 total;
    std::vector<unsigned __int128> offset;
};

static Model model_of(const std::vector<u64> &counts, u64 capacity, u64 esize) {
    Model md{false, 0, {}};
    for (u64 c : counts) {
        md.offset.push_back(md.total);
        md.overflow |= c == ~0ull;
        md.total += c;
    }
    md.overflow |= md.total > capacity || md.total * esize > (unsigned __int128)~0ull;
    return md;
}

static void check_case(const std::vector<u64> &counts, u64 capacity, u64 esize) {
    const int P = (int)counts.size();
    g_P = P;
    g_cap = capacity;
    const Model md = model_of(counts, capacity, esize);
    CollectPlan first;
    for (int m = 0; m < P; ++m) {
        g_m = m;
        CollectPlan p;
        std::memset(&p, 0xEE, sizeof p);
        collect_plan(counts.data(), P, capacity, esize, m, &p);
        CHECK(p.overflow == (md.overflow ? 1u : 0u));
        CHECK(p.total == (md.total > ~0ull ? ~0ull : (u64)md.total));   // saturated, never wrapped
        if (m == 0) first = p;
        // every member computes the same offsets and total
        CHECK(p.total == first.total && p.overflow == first.overflow);
        for (int i = 0; i < P; ++i) CHECK(p.offset[i] == first.offset[i] && p.count[i] == counts[i]);
        if (md.overflow) {
            CHECK(p.nseg == 0);
            continue;
        }
        for (int i = 0; i < P; ++i) CHECK(p.offset[i] == (u64)md.offset[i]);
        // the order: from member m + 1 on, wrapping, m last, the empty ones skipped
        std::vector<int> want;
        for (int r = 0; r < P; ++r)
            if (counts[(m + 1 + r) % P]) want.push_back((m + 1 + r) % P);
        CHECK(p.nseg == want.size());
        for (size_t k = 0; k < want.size(); ++k) CHECK(p.order[k] == (u64)want[k]);
        if (counts[m]) CHECK(p.order[p.nseg - 1] == (u64)m);
        // the segments tile [0, total) without overlap
        std::vector<std::pair<u64, u64>> segs;
        for (u64 k = 0; k < p.nseg; ++k) segs.emplace_back(p.offset[p.order[k]], p.count[p.order[k]]);
        std::sort(segs.begin(), segs.end());
        u64 edge = 0;
        for (const auto &s : segs) {
            CHECK(s.first == edge && s.second > 0);
            edge += s.second;
        }
        CHECK(edge == p.total && p.total <= capacity);
    }
}

static void check_counts(const std::vector<u64> &counts) {
    unsigned __int128 total = 0;
    for (u64 c : counts) total += c;
    for (u64 esize : {4ull, 8ull}) {
        if (total <= ~0ull) {
            check_case(counts, (u64)total, esize);                     // total == capacity
            if (total > 0) check_case(counts, (u64)total - 1, esize);   // total == capacity + 1
            check_case(counts, (u64)total + 1000003, esize);
        }
        check_case(counts, 0, esize);
        check_case(counts, ~0ull >> 8, esize);
    }
}

int main() {
    const u64 draw[5] = {0, 1, 3, 64, 1013};
    unsigned int lcg = 12345;
    auto next = [&] { return (lcg = lcg * 1664525u + 1013904223u) >> 16; };
    for (int P = 1; P <= kCollectMaxMembers; ++P) {
        std::vector<u64> counts(P);
        if (P <= 4) {   // every combination
            int combos = 1;
            for (int i = 0; i < P; ++i) combos *= 5;
            for (int c = 0; c < combos; ++c) {
                for (int i = 0, d = c; i < P; ++i, d /= 5) counts[i] = draw[d % 5];
                check_counts(counts);
            }
        } else {
            for (int rep = 0; rep < 200; ++rep) {
                for (int i = 0; i < P; ++i) counts[i] = draw[next() % 5];
                check_counts(counts);
            }
        }
        check_counts(std::vector<u64>(P, 0));   // all zero
        for (int pos = 0; pos < P; ++pos) {
            for (u64 one : {1ull, 1013ull}) {    // a single non-zero count
                std::vector<u64> c(P, 0);
                c[pos] = one;
                check_counts(c);
            }
            // one poison count in every position, among full and among empty members
            for (u64 other : {0ull, 64ull}) {
                std::vector<u64> c(P, other);
                c[pos] = kCollectPoison;
                check_counts(c);
            }
            // counts near 2^63: two of them pass 2^64
            std::vector<u64> c(P, 3);
            c[pos] = (1ull << 63) + 5;
            check_counts(c);
            c[(pos + 1) % P] = (1ull << 63) - 1;
            check_counts(c);
            if (P > 2) {
                c[(pos + 2) % P] = (1ull << 63) + 7;
                check_counts(c);
            }
        }
    }
    std::printf("ok %ld checks\n", g_checks);
    return 0;
}
