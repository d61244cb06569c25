// The geometry of the stream-ordered broadcast and fcollect (set_geom.h:
// BcastSlices, bcast_from_root, bcast_from_peers, fcollect_segments), host
// only, meant for -fsanitize=address,undefined (tests/test_pull_geom_host.py).
// Every member's arrays are real buffers of the largest case's size, so every
// pointer the geometry forms stays inside one.
//
// For P in 1..16, every root, element sizes 4 and 8 and nelems in {0, 1, 3,
// P - 2, P - 1, P, 1013, 70001}:
//   - the non-roots' slices tile [0, nelems) exactly once;
//   - what m gathers from i in phase B is exactly what i pulled in phase A:
//     same offset, same length;
//   - no segment of m's lists overlaps another segment's target range (and
//     together they cover m's whole target);
//   - the fcollect segments tile [0, P * nbytes).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "set_geom.h"

using namespace shmx;

static long g_checks = 0;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        ++g_checks;                                                                          \
        if (!(cond)) {                                                                       \
            std::printf("FAIL %s:%d: %s  (P=%d root=%d esize=%zu nelems=%zu m=%d)\n", __FILE__, __LINE__, #cond, \
                        g_P, g_root, g_esize, g_nelems, g_m);                                 \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

static int g_P, g_root, g_m;
static size_t g_esize, g_nelems;

constexpr int kMaxP = 16;
constexpr size_t kMaxElems = 70001;

struct Seg {
    size_t off, len;
};

// which buffer of `bufs` (cap bytes each) holds p, and where
static int locate(const std::vector<std::vector<char>> &bufs, const void *p, size_t *off) {
    const char *c = static_cast<const char *>(p);
    for (size_t i = 0; i < bufs.size(); ++i) {
        const char *b = bufs[i].data();
        if (c >= b && c < b + bufs[i].size()) {   // segments here are never empty
            *off = (size_t)(c - b);
            return (int)i;
        }
    }
    return -1;
}

// the ranges are disjoint and cover [0, total) exactly
// (sorted by offset, each non-empty range starts where the one before ended)
static void check_tiling(std::vector<Seg> segs, size_t total) {
    std::sort(segs.begin(), segs.end(), [](const Seg &x, const Seg &y) { return x.off < y.off; });
    size_t at = 0;
    for (const Seg &s : segs) {
        if (!s.len) continue;
        CHECK(s.off == at);
        at += s.len;
    }
    CHECK(at == total);
}

int main() {
    // srcs[i], tgts[i]: member i's source and target (the fcollect target
    // holds P sources; its largest case here is 16 x 70001 x 8 bytes)
    std::vector<std::vector<char>> srcs(kMaxP), tgts(kMaxP);
    for (int i = 0; i < kMaxP; ++i) {
        srcs[i].resize(kMaxElems * 8);
        tgts[i].resize(kMaxElems * 8);
    }
    std::vector<char> ftgt(kMaxElems * 8 * kMaxP);
    const void *from[kMaxP];
    void *to[kMaxP];
    size_t len[kMaxP];

    for (int P = 1; P <= kMaxP; ++P) {
        const long sizes[] = {0, 1, 3, P - 2, P - 1, P, 1013, (long)kMaxElems};
        for (size_t esize : {(size_t)4, (size_t)8}) {
            for (long n : sizes) {
                if (n < 0) continue;   // P - 2 at P = 1
                const size_t nelems = (size_t)n, nbytes = nelems * esize;
                g_P = P, g_esize = esize, g_nelems = nelems, g_root = -1, g_m = -1;

                // ---- fcollect: P segments tile [0, P * nbytes), rotated, m last
                for (int m = 0; m < P; ++m) {
                    g_m = m;
                    const int k = fcollect_segments(P, m, nbytes, [&](int i) { return srcs[i].data(); },
                                                    ftgt.data(), from, to, len);
                    CHECK(k == P);
                    std::vector<Seg> segs;
                    for (int r = 0; r < k; ++r) {
                        const int i = (m + 1 + r) % P;
                        CHECK(from[r] == srcs[i].data());
                        CHECK(to[r] == ftgt.data() + (size_t)i * nbytes);
                        CHECK(len[r] == nbytes);
                        segs.push_back(Seg{(size_t)i * nbytes, nbytes});
                    }
                    CHECK(from[k - 1] == srcs[m].data());   // my own copy last
                    check_tiling(segs, (size_t)P * nbytes);
                }

                for (int root = 0; root < P; ++root) {
                    g_root = root, g_m = -1;
                    const BcastSlices bs(nelems, P, root, esize);
                    auto tgt_of = [&](int i) { return tgts[i].data(); };

                    // ---- the non-roots' slices tile [0, nelems) exactly once
                    if (P > 1) {
                        std::vector<Seg> own;
                        int k = 0;
                        for (int i = 0; i < P; ++i) {
                            if (i == root) {
                                CHECK(bs.count(i) == 0);
                                continue;
                            }
                            CHECK(bs.index(i) == k++);   // the non-roots in set order
                            CHECK(bs.lo(i) <= bs.hi(i) && bs.hi(i) <= nelems);
                            // every non-empty slice starts on a 16-byte granule of the array
                            if (bs.count(i)) CHECK(bs.lo(i) * esize % 16 == 0);
                            own.push_back(Seg{bs.lo(i), bs.count(i)});
                        }
                        check_tiling(own, nelems);
                    }

                    // ---- phase A of every member, one phase and two phase
                    std::vector<Seg> a_of(P, Seg{0, 0});
                    for (int m = 0; m < P; ++m) {
                        g_m = m;
                        int k = bcast_from_root(bs, m, false, srcs[root].data(), tgts[m].data(), from, to, len);
                        if (m == root || nbytes == 0) {
                            CHECK(k == 0);
                        } else {   // one phase: the whole array
                            CHECK(k == 1 && from[0] == srcs[root].data() && to[0] == tgts[m].data() &&
                                  len[0] == nbytes);
                        }
                        k = bcast_from_root(bs, m, true, srcs[root].data(), tgts[m].data(), from, to, len);
                        if (m == root || bs.count(m) == 0) {
                            CHECK(k == 0);
                            continue;
                        }
                        CHECK(k == 1);
                        size_t so = 0, to_ = 0;
                        CHECK(locate(srcs, from[0], &so) == root);
                        CHECK(locate(tgts, to[0], &to_) == m);
                        CHECK(so == to_ && so == bs.lo(m) * esize && len[0] == bs.count(m) * esize);
                        a_of[m] = Seg{so, len[0]};
                    }

                    // ---- phase B: from i exactly what i pulled in phase A;
                    // m's segments of both lists are disjoint and cover its target
                    for (int m = 0; m < P; ++m) {
                        g_m = m;
                        const int k = bcast_from_peers(bs, m, tgt_of, tgts[m].data(), from, to, len);
                        if (m == root) {
                            CHECK(k == 0);
                            continue;
                        }
                        CHECK(k <= P - 2 || (P < 2 && k == 0));
                        std::vector<Seg> mine;
                        if (a_of[m].len) mine.push_back(a_of[m]);
                        std::vector<int> seen(P, 0);
                        int prev_r = -1;
                        for (int j = 0; j < k; ++j) {
                            size_t so = 0, to_ = 0;
                            const int i = locate(tgts, from[j], &so);
                            CHECK(i >= 0 && i != m && i != root && !seen[i]);
                            seen[i] = 1;
                            CHECK(locate(tgts, to[j], &to_) == m);
                            CHECK(len[j] > 0 && so == to_);
                            CHECK(so == a_of[i].off && len[j] == a_of[i].len);
                            // rotated: from member m + 1 on, wrapping
                            const int r = (i - m - 1 + P) % P;
                            CHECK(r > prev_r);
                            prev_r = r;
                            mine.push_back(Seg{to_, len[j]});
                        }
                        for (int i = 0; i < P; ++i)   // nobody with a slice is left out
                            if (i != m && i != root && bs.count(i)) CHECK(seen[i]);
                        check_tiling(mine, nbytes);
                    }
                }
            }
        }
    }
    std::printf("ok %ld checks\n", g_checks);
    return 0;
}
