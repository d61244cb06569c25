// CPU test of the active-set geometry every multi-PE algorithm shares
// (csrc/set_geom.h): the 16-byte granule, the two-shot slices (fixed cases
// and a sweep: they tile [0, n) in order, every non-empty slice starts on a
// granule multiple, only the last non-empty one is short), the whole-job
// test, a member's PE, the fold-input orders and the gather segment lists.
//
//   test_set_geom            prints "ok <checks>"
#include <cstdio>
#include <utility>
#include <vector>

#include "set_geom.h"

using namespace shmx;

static long checks = 0, fails = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++fails;                                                  \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);       \
        }                                                             \
    } while (0)

static void check_slices(size_t n, int P, size_t sz, const std::vector<std::pair<size_t, size_t>> &want) {
    const Slices sl(n, P, sz);
    for (int i = 0; i < P; ++i) {
        CHECK(sl.lo(i) == want[i].first);
        CHECK(sl.hi(i) == want[i].second);
        CHECK(sl.count(i) == want[i].second - want[i].first);
    }
}

static std::vector<int> order(int P, int m, bool own) {
    static const char base[64] = {0};
    std::vector<const void *> ins(P, nullptr);
    fold_inputs(ins.data(), P, m, own, [&](int i) { return base + i; });
    std::vector<int> got;
    for (const void *p : ins) got.push_back((int)(static_cast<const char *>(p) - base));
    return got;
}

// gather_segments over fake arrays: which member each segment reads, its
// byte offset (the same in the owner's array and in the target) and length
struct Segs {
    std::vector<int> member;
    std::vector<size_t> off, len;
};

static Segs segments(const Slices &sl, int m, bool rotated, bool include_m) {
    static char peers[16][256], tgt[256];
    const void *from[16];
    void *to[16];
    size_t len[16];
    const int k = gather_segments(sl, m, rotated, include_m, [&](int i) { return peers[i]; }, tgt, from, to, len);
    Segs g;
    for (int j = 0; j < k; ++j) {
        const size_t at = (size_t)(static_cast<const char *>(from[j]) - &peers[0][0]);
        g.member.push_back((int)(at / 256));
        g.off.push_back(at % 256);
        g.len.push_back(len[j]);
        CHECK(static_cast<char *>(to[j]) == tgt + at % 256);
    }
    return g;
}

int main() {
    // granule
    const size_t sizes[] = {1, 2, 4, 8, 16, 32}, granules[] = {16, 8, 4, 2, 1, 1};
    for (int k = 0; k < 6; ++k) CHECK(granule(sizes[k]) == granules[k]);

    // slices, as [lo, hi) per member
    check_slices(10, 4, 4, {{0, 4}, {4, 8}, {8, 10}, {10, 10}});
    check_slices(1, 8, 8, {{0, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}});
    check_slices(64, 4, 16, {{0, 16}, {16, 32}, {32, 48}, {48, 64}});
    check_slices(5, 3, 32, {{0, 2}, {2, 4}, {4, 5}});
    for (size_t sz : sizes)
        for (int P : {1, 3, 16})
            for (int i = 0; i < P; ++i) CHECK(Slices(0, P, sz).count(i) == 0 && Slices(0, P, sz).lo(i) == 0);

    // the sweep
    for (size_t sz : sizes) {
        const size_t g = granule(sz);
        for (int P = 1; P <= 16; ++P) {
            for (size_t n = 0; n <= 200; ++n) {
                const Slices sl(n, P, sz);
                size_t end = 0;
                bool ok = sl.slice % g == 0, short_seen = false;
                for (int i = 0; i < P; ++i) {
                    ok = ok && sl.lo(i) == end && sl.hi(i) >= sl.lo(i) && sl.count(i) == sl.hi(i) - sl.lo(i);
                    end = sl.hi(i);
                    if (sl.count(i) == 0) continue;
                    // nothing follows a short slice, and every slice starts on a granule
                    ok = ok && !short_seen && sl.lo(i) % g == 0 && sl.count(i) <= sl.slice;
                    short_seen = sl.count(i) < sl.slice;
                }
                ok = ok && end == n;
                CHECK(ok);
                if (!ok) std::printf("  n %zu P %d size %zu\n", n, P, sz);
            }
        }
    }

    // the whole job, and a member's PE
    CHECK((ActiveSet{0, 1, 4}.world(4)));
    CHECK(!(ActiveSet{0, 2, 2}.world(4)));
    CHECK(!(ActiveSet{1, 1, 3}.world(4)));
    CHECK((ActiveSet{0, 4, 1}.world(1)));   // one member: its stride says nothing
    CHECK(ActiveSet::of(0, 2, 1).world(1) && ActiveSet::of(0, 2, 1).step == 4);
    CHECK(ActiveSet::of(0, 0, 4).world(4) && !ActiveSet::of(0, 1, 2).world(4));
    CHECK(!ActiveSet::of(0, 31, 2).world(2) && !ActiveSet::of(0, -1, 2).world(2));
    const ActiveSet s243{2, 4, 3};
    CHECK(s243.pe_of(0) == 2 && s243.pe_of(1) == 6 && s243.pe_of(2) == 10);

    // fold-input order
    CHECK((order(4, 2, false) == std::vector<int>{0, 1, 2, 3}));
    CHECK((order(4, 0, false) == std::vector<int>{0, 1, 2, 3}));
    CHECK((order(4, 2, true) == std::vector<int>{2, 0, 1, 3}));
    CHECK((order(4, 0, true) == std::vector<int>{0, 1, 2, 3}));
    CHECK((order(4, 3, true) == std::vector<int>{3, 0, 1, 2}));
    CHECK((order(1, 0, true) == std::vector<int>{0}));

    // gather segments: n = 10, P = 4, 4-byte elements, member 1 (member 3's slice is empty)
    {
        const Slices sl(10, 4, 4);
        Segs g = segments(sl, 1, true, false);
        CHECK((g.member == std::vector<int>{2, 0}));
        CHECK((g.off == std::vector<size_t>{32, 0}));
        CHECK((g.len == std::vector<size_t>{8, 16}));
        g = segments(sl, 1, true, true);
        CHECK((g.member == std::vector<int>{2, 0, 1}));
        CHECK((g.off == std::vector<size_t>{32, 0, 16}));
        CHECK((g.len == std::vector<size_t>{8, 16, 16}));
        CHECK((segments(sl, 1, false, false).member == std::vector<int>{0, 2}));
        CHECK((segments(sl, 1, false, true).member == std::vector<int>{0, 1, 2}));
        // member 3 owns nothing: it gathers the three others, from member 0 on
        CHECK((segments(sl, 3, true, true).member == std::vector<int>{0, 1, 2}));
        CHECK(segments(Slices(0, 4, 4), 1, true, true).member.empty());
    }

    if (fails) return 1;
    std::printf("ok %ld\n", checks);
    return 0;
}
