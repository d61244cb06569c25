// OWNSLICE's geometry (set_geom.h: order_slot, order_slots_bytes,
// gather_order_slots) on the CPU: for every P, element size and a sweep of
// chunk sizes, the owner's P - 1 result slots are disjoint, 16-byte aligned
// and inside the slot area; every member gathers, from every other owner of
// a non-empty slice, exactly the slot that owner wrote for it, to that slice
// of its target; and the slot area stays within the bound direct.cpp sizes
// its chunks by: at most the chunk's bytes plus 16 (P - 1).
//   test_order_slots            prints "ok <checks>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "set_geom.h"

using namespace shmx;

static long checks = 0;
#define CHECK(c)                                                                     \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(c)) {                                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);               \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

int main() {
    const size_t sizes[] = {4, 8, 16};
    const size_t counts[] = {1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 1013, 4096, 70001, 131072 - 4};
    for (int P = 2; P <= 16; ++P)
        for (size_t sz : sizes)
            for (size_t cnt : counts) {
                const Slices sl(cnt, P, sz);
                const size_t area = order_slots_bytes(sl);
                CHECK(area == (size_t)(P - 1) * sl.slice * sz);
                CHECK(area <= cnt * sz + 16 * (size_t)(P - 1));
                // every owner's slots: one per other member, disjoint, aligned, inside
                for (int m = 0; m < P; ++m) {
                    std::vector<char> used(area, 0);
                    for (int k = 0; k < P; ++k) {
                        if (k == m) continue;
                        const size_t off = order_slot(sl, m, k);
                        CHECK(off % 16 == 0);
                        CHECK(off + sl.count(m) * sz <= area);
                        for (size_t b = off; b < off + sl.count(m) * sz; ++b) {
                            CHECK(!used[b]);
                            used[b] = 1;
                        }
                    }
                }
                // every member's gather: from each other owner of a non-empty
                // slice, the slot written for it, to that slice of its target
                std::vector<std::vector<char>> slots(P, std::vector<char>(area + 1));
                std::vector<char> tgt(cnt * sz + 1);
                for (int m = 0; m < P; ++m) {
                    const void *from[16];
                    void *to[16];
                    size_t len[16];
                    const int nseg = gather_order_slots(
                        sl, m, [&](int i) { return slots[i].data(); }, tgt.data(), from, to, len);
                    int want = 0;
                    std::vector<char> seen(P, 0);
                    for (int i = 0; i < P; ++i) want += i != m && sl.count(i) > 0;
                    CHECK(nseg == want && nseg <= P - 1);
                    size_t covered = 0;
                    for (int s = 0; s < nseg; ++s) {
                        const size_t toff = static_cast<char *>(to[s]) - tgt.data();
                        CHECK(toff % (sl.slice * sz) == 0);
                        const int i = (int)(toff / (sl.slice * sz));   // the owner
                        CHECK(i != m && i < P && !seen[i]);
                        seen[i] = 1;
                        CHECK(toff == sl.lo(i) * sz && len[s] == sl.count(i) * sz);
                        CHECK(from[s] == slots[i].data() + order_slot(sl, i, m));
                        covered += len[s];
                    }
                    CHECK(covered + sl.count(m) * sz == cnt * sz);
                    // rotated: the first segment is the next non-empty owner after m
                    if (nseg) {
                        int first = (m + 1) % P;
                        while (sl.count(first) == 0 || first == m) first = (first + 1) % P;
                        CHECK(to[0] == tgt.data() + sl.lo(first) * sz);
                    }
                }
            }
    std::printf("ok %ld\n", checks);
    return 0;
}
