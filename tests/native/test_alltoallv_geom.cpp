// alltoallv_plan (set_geom.h), the one definition the alltoallv kernels and
// this program share, against a brute-force model; host only, meant for
// -fsanitize=address,undefined (tests/test_alltoallv_geom_host.py).
//
// For P in 1..16, every receiver m, element sizes 4 and 8, the pairs
// (counts[i], offsets[i]) = member i's (send_counts[m], send_offsets[m]):
//   - counts drawn from {0, 1, 3, 64, 1013} (every combination up to P = 4, a
//     fixed pseudo-random draw of them above), all-zero counts and a single
//     non-zero count in every position; offsets non-monotonic, anywhere the
//     block still fits its source, including flush with its end;
//   - capacity equal to the total (no overflow), one short of it (overflow)
//     and far above it;
//   - one bad pair in every position, among full and among empty members: a
//     count one above src_capacity, an offset one above src_capacity - count,
//     offset 2^64 - 1, count 2^64 - 1: overflow whatever the capacity;
//   - counts whose sum passes 2^64 (src_capacity near 2^64): the sum saturates,
//     never wraps, and the plan overflows;
//   - the immediate form of the fixed alltoall (every count nelems, every
//     offset m * nelems, both capacities P * nelems): exact, never an overflow.
// Without overflow, sender i's target offset is the model's prefix sum, `from`
// is the offset as read, the segments of m's order tile [0, total) without
// overlap in sender order, the order starts at the first non-empty member
// after m, wrapping, with m's own block last, and skips exactly the empty
// members.  With overflow the plan has no segment.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "set_geom.h"

using namespace shmx;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

static long g_checks = 0;
static int g_P, g_m;
static u64 g_cap, g_scap;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) {                                                                                       \
            std::printf("FAIL %s:%d: %s  (P=%d m=%d capacity=%llu src_capacity=%llu)\n", __FILE__, __LINE__, \
                        #cond, g_P, g_m, g_cap, g_scap);                                                     \
            std::exit(1);                                                                                    \
        }                                                                                                    \
    } while (0)

// the model: 128-bit sums, nothing shared with alltoallv_plan
struct Model {
    bool overflow;
    u128 total;
    std::vector<u128> offset;
};

static Model model_of(const std::vector<u64> &counts, const std::vector<u64> &offs, u64 capacity, u64 scap,
                      u64 esize) {
    Model md{false, 0, {}};
    for (size_t i = 0; i < counts.size(); ++i) {
        md.offset.push_back(md.total);
        md.overflow |= (u128)offs[i] + counts[i] > scap;   // the block leaves its source
        md.total += counts[i];
    }
    md.overflow |= md.total > capacity || md.total * esize > (u128)~0ull;
    return md;
}

static void check_case(const std::vector<u64> &counts, const std::vector<u64> &offs, u64 capacity, u64 scap,
                       u64 esize, int want_overflow = -1) {
    const int P = (int)counts.size();
    g_P = P;
    g_cap = capacity;
    g_scap = scap;
    const Model md = model_of(counts, offs, capacity, scap, esize);
    if (want_overflow >= 0) CHECK(md.overflow == (want_overflow != 0));
    AlltoallvPlan first;
    for (int m = 0; m < P; ++m) {
        g_m = m;
        AlltoallvPlan p;
        std::memset(&p, 0xEE, sizeof p);
        alltoallv_plan(counts.data(), offs.data(), P, capacity, scap, esize, m, &p);
        CHECK(p.overflow == (md.overflow ? 1u : 0u));
        CHECK(p.total == (md.total > ~0ull ? ~0ull : (u64)md.total));   // saturated, never wrapped
        if (m == 0) first = p;
        // the layout does not depend on who asks
        CHECK(p.total == first.total && p.overflow == first.overflow);
        for (int i = 0; i < P; ++i)
            CHECK(p.offset[i] == first.offset[i] && p.count[i] == counts[i] && p.from[i] == offs[i]);
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
        // the target segments tile [0, total) without overlap, in sender order; every source block fits
        std::vector<std::pair<u64, u64>> segs;
        for (u64 k = 0; k < p.nseg; ++k) {
            const u64 i = p.order[k];
            segs.emplace_back(p.offset[i], i);
            CHECK(p.from[i] <= scap && p.count[i] <= scap - p.from[i]);
        }
        std::sort(segs.begin(), segs.end());
        u64 edge = 0, last = 0;
        for (size_t k = 0; k < segs.size(); ++k) {
            CHECK(segs[k].first == edge && p.count[segs[k].second] > 0);
            if (k) CHECK(segs[k].second > last);
            last = segs[k].second;
            edge += p.count[segs[k].second];
        }
        CHECK(edge == p.total && p.total <= capacity);
    }
}

static unsigned int g_lcg = 12345;
static unsigned int next_draw() { return (g_lcg = g_lcg * 1664525u + 1013904223u) >> 16; }

// healthy pairs: offsets anywhere the block fits, one flush with the source's end
static std::vector<u64> offsets_for(const std::vector<u64> &counts, u64 scap) {
    std::vector<u64> offs(counts.size());
    for (size_t i = 0; i < counts.size(); ++i) {
        const u64 room = scap - counts[i];
        offs[i] = i % 3 == 0 ? room : next_draw() % (room + 1);
    }
    return offs;
}

static void check_counts(const std::vector<u64> &counts) {
    u64 total = 0, most = 0;
    for (u64 c : counts) {
        total += c;
        most = std::max(most, c);
    }
    const int P = (int)counts.size();
    for (u64 esize : {4ull, 8ull}) {
        for (u64 scap : {most, most + 7, 5000ull}) {
            const std::vector<u64> offs = offsets_for(counts, scap);
            check_case(counts, offs, total, scap, esize, 0);                     // total == capacity
            if (total > 0) check_case(counts, offs, total - 1, scap, esize, 1);   // total == capacity + 1
            check_case(counts, offs, total + 1000003, scap, esize, 0);
            check_case(counts, offs, ~0ull >> 8, scap, esize, 0);
            // each bad pair in every position
            for (int pos = 0; pos < P; ++pos) {
                std::vector<u64> c = counts, o = offs;
                c[pos] = scap + 1;                        // the count alone is above the source
                o[pos] = 0;
                check_case(c, o, ~0ull >> 8, scap, esize, 1);
                c = counts;
                o = offs;
                o[pos] = scap - c[pos] + 1;               // one element past the source's end
                check_case(c, o, ~0ull >> 8, scap, esize, 1);
                o[pos] = ~0ull;                           // offset + count wraps for any count above 0
                check_case(c, o, ~0ull >> 8, scap, esize, 1);
                o[pos] = ~0ull - c[pos] + 1;              // offset + count == 2^64 exactly
                if (c[pos]) check_case(c, o, ~0ull >> 8, scap, esize, 1);
                c[pos] = ~0ull;
                o[pos] = 0;
                check_case(c, o, ~0ull >> 8, scap, esize, 1);
                o[pos] = 1;
                check_case(c, o, ~0ull, scap, esize, 1);
            }
        }
    }
}

int main() {
    const u64 draw[5] = {0, 1, 3, 64, 1013};
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
            for (int rep = 0; rep < 60; ++rep) {
                for (int i = 0; i < P; ++i) counts[i] = draw[next_draw() % 5];
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
            // sums past 2^64: the source is as large as the numbers, only the total is not
            const u64 scap = ~0ull - 1;
            std::vector<u64> c(P, 3), o(P, 0);
            c[pos] = (1ull << 63) + 5;
            for (u64 esize : {4ull, 8ull}) check_case(c, o, ~0ull, scap, esize, 1);   // bytes wrap
            if (P > 1) {
                c[(pos + 1) % P] = (1ull << 63) - 1;
                for (u64 esize : {4ull, 8ull}) check_case(c, o, ~0ull, scap, esize, 1);
            }
            if (P > 2) {
                c[(pos + 2) % P] = (1ull << 63) + 7;
                for (u64 esize : {4ull, 8ull}) check_case(c, o, ~0ull, scap, esize, 1);
            }
        }
        // the fixed alltoall's immediates: exact at P * nelems, for every m
        for (u64 nelems : {1ull, 3ull, 4ull, 1013ull, 70001ull}) {
            for (int m = 0; m < P; ++m) {
                const std::vector<u64> c(P, nelems), o(P, (u64)m * nelems);
                for (u64 esize : {4ull, 8ull}) {
                    check_case(c, o, (u64)P * nelems, (u64)P * nelems, esize, 0);
                    AlltoallvPlan p;
                    alltoallv_plan(c.data(), o.data(), P, (u64)P * nelems, (u64)P * nelems, esize, m, &p);
                    CHECK(p.total == (u64)P * nelems && p.nseg == (u64)P && !p.overflow);
                    for (int i = 0; i < P; ++i) CHECK(p.offset[i] == (u64)i * nelems && p.from[i] == (u64)m * nelems);
                }
            }
        }
    }
    std::printf("ok %ld checks\n", g_checks);
    return 0;
}
