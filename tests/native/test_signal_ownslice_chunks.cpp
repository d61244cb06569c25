// The chunking of SIGNAL's own slice (signal.cpp signal_ownslice; set_geom.h
// order_chunk_elems, Slices, order_slot, order_slots_bytes,
// gather_order_slots) on the CPU: a call of n elements whose result slots
// live in `half` bytes (half the IPC scratch) runs in chunks of
// order_chunk_elems(half, P, sz) elements, each a whole schedule.  For P in
// 2..16, every element size, halves from the smallest that holds one granule
// per slot upward and n including n < P:
//   * the chunks tile [0, n);
//   * each chunk's slot area, at any skew below 16 bytes, fits the half;
//   * every owner's slots of a chunk are disjoint and inside the area;
//   * every member gathers, from every other owner of a non-empty slice of
//     the chunk, exactly the slot that owner wrote for it, into that slice of
//     the chunk in its target, and with its own slice that covers the chunk.
//   test_signal_ownslice_chunks   prints "ok <checks>"
#include <algorithm>
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

static void one_call(int P, size_t sz, size_t half, size_t n, size_t skew) {
    const size_t g = granule(sz);
    const size_t C = std::min(std::max<size_t>(n, 1), order_chunk_elems(half, P, sz));
    CHECK(C >= 1 && (C == n || C % g == 0));
    std::vector<std::vector<char>> scratch(P, std::vector<char>(half));
    std::vector<char> tgt(n * sz + 1);
    auto slots_of = [&](int i) { return scratch[i].data() + skew; };
    size_t next = 0;
    for (size_t c0 = 0; c0 < n; c0 += C) {
        CHECK(c0 == next);
        const size_t cnt = std::min(C, n - c0);
        CHECK(cnt >= 1);
        next = c0 + cnt;
        const Slices sl(cnt, P, sz);
        const size_t area = order_slots_bytes(sl);
        CHECK(skew + area <= half);
        // what every owner writes: P - 1 slots, disjoint, inside its area
        for (int i = 0; i < P; ++i) {
            size_t end_prev = 0;
            for (int k = 0; k < P; ++k) {
                if (k == i) continue;
                const size_t off = order_slot(sl, i, k);
                CHECK(off >= end_prev && off % 16 == 0);
                end_prev = off + sl.count(i) * sz;
                CHECK(end_prev <= area);
            }
        }
        // what every member gathers
        for (int m = 0; m < P; ++m) {
            const void *from[16];
            void *to[16];
            size_t len[16];
            const int nseg = gather_order_slots(sl, m, slots_of, tgt.data() + c0 * sz, from, to, len);
            CHECK(nseg >= 0 && nseg <= P - 1);
            std::vector<char> seen(P, 0);
            size_t covered = sl.count(m) * sz;
            for (int s = 0; s < nseg; ++s) {
                const size_t toff = static_cast<char *>(to[s]) - tgt.data();
                CHECK(toff >= c0 * sz && (toff - c0 * sz) % (sl.slice * sz) == 0);
                const int i = (int)((toff - c0 * sz) / (sl.slice * sz));   // the owner
                CHECK(i < P && i != m && !seen[i] && sl.count(i) > 0);
                seen[i] = 1;
                CHECK(toff == (c0 + sl.lo(i)) * sz && len[s] == sl.count(i) * sz);
                CHECK(toff + len[s] <= n * sz);
                // the slot owner i wrote for member m
                CHECK(from[s] == slots_of(i) + order_slot(sl, i, m));
                CHECK(static_cast<const char *>(from[s]) + len[s] <= scratch[i].data() + half);
                covered += len[s];
            }
            CHECK(covered == cnt * sz);
        }
    }
    CHECK(next == n);
}

int main() {
    const size_t sizes[] = {4, 8, 16};
    for (int P = 2; P <= 16; ++P)
        for (size_t sz : sizes) {
            // the smallest half that holds the rounding, a skew and one
            // granule per slot; a few bytes more; and real ones (1 MiB of
            // scratch gives 512 KiB)
            const size_t least = (size_t)16 * (P + 2);
            const size_t halves[] = {least, least + 1, least + 16, least + 16 * (size_t)P, 4096, 65536 + 24,
                                     (size_t)512 << 10};
            const size_t ns[] = {1, 2, (size_t)P - 1, (size_t)P, (size_t)P + 1, 63, 1013, 70001, 150001};
            for (size_t half : halves)
                for (size_t n : ns) {
                    // a small half takes one granule or so per chunk: keep its calls short
                    if (half < 4096 && n > 1013) continue;
                    for (size_t skew : {(size_t)0, (size_t)8, (size_t)15}) one_call(P, sz, half, n, skew);
                }
        }
    std::printf("ok %ld\n", checks);
    return 0;
}
