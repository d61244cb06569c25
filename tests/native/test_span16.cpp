// CPU test of the fold-family kernels' split and grid rules (csrc/span16.h):
// for element sizes 2 / 4 / 8 / 16, 1 to 3 arrays at every byte offset 0-31
// each, and n in 0-70 plus large values (one above 2^32, one past the block
// cap), split16 tiles [0, n) as head + vectors + tail; a body, where there is
// one, starts 16 B-aligned in every array, is as long as it can be and leaves
// less than a vector on either side; arrays of different offsets, or an
// offset that is no whole number of elements, give {n, 0, 0}; span_blocks
// equals the launch's grid expression, restated here; and the forecast "this
// copy is one workgroup" equals copy_blocks == 1, around the three boundaries
// (kBlock scalars, kBlock x kUnrollCopy vectors, and one more); the
// cache-policy predicate and the launch choice built on it (nt_policy,
// copy_choice, fold_choice, orders_choice) one element below, at and above
// the 32 MiB cut for every array count a launch can have, restated here.
// The addresses are numbers: nothing is dereferenced.
//
//   test_span16          prints "ok <splits>"
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "span16.h"

using shmx::Span16;

namespace {

long g_fails = 0;

void fail(const char *what, size_t sz, const uintptr_t *addr, int np, size_t n, const Span16 &s) {
    if (++g_fails > 20) return;
    std::printf("FAIL %s: size %zu n %zu offsets", what, sz, n);
    for (int k = 0; k < np; ++k) std::printf(" %zu", (size_t)(addr[k] & 31u));
    std::printf(" -> head %zu nvec %zu tail %zu\n", s.head, s.nvec, s.tail);
}

// the grid expression of the fold launches, written out on its own
size_t blocks_restated(size_t head, size_t nvec, size_t tail, int unroll) {
    size_t work;
    if (nvec > 0)
        work = (nvec + (size_t)256 * unroll - 1) / ((size_t)256 * unroll);
    else
        work = (head + tail + 255) / 256;
    const size_t cap = nvec == 0 ? 2048 : (size_t)1 << 30;
    size_t blocks = work < cap ? work : cap;
    if (blocks < 1) blocks = 1;
    if (blocks > (size_t)INT_MAX) blocks = INT_MAX;
    return blocks;
}

// "a copy of n >= 1 elements from src to dst runs as one workgroup", written
// out on its own: all scalar up to 256 elements, else up to 256 x 8 vectors
bool one_workgroup_restated(size_t sz, uintptr_t dst, uintptr_t src, size_t n) {
    const uintptr_t off = dst & 15u;
    if (off % sz != 0 || (src & 15u) != off) return n <= 256;
    size_t head = ((16 - off) & 15u) / sz;
    if (head > n) head = n;
    const size_t E = 16 / sz, nvec = (n - head) / E, tail = n - head - nvec * E;
    if (nvec == 0) return head + tail <= 256;
    return nvec <= (size_t)256 * 8;
}

void fail_policy(const char *what, size_t arrays, size_t sz, size_t n) {
    if (++g_fails > 20) return;
    std::printf("FAIL %s: arrays %zu size %zu n %zu\n", what, arrays, sz, n);
}

// n elements of size sz at a 16-byte aligned address, split as split16 would
Span16 aligned_span(size_t sz, size_t n) {
    const size_t E = 16 / sz;
    return Span16{0, n / E, n % E};
}

// The cache-policy rule and the launch choice around the cut, for every
// array count a launch can have: 2 (the copy), nins + 1 = 3..17 (the folds of
// 2..16 inputs), 2 nins = 2..32 (the P-order fold of 1..16 inputs): one
// element below the cut (the last n whose arrays hold less than 32 MiB), the
// cut itself (exactly 32 MiB where arrays x size divides it) and one above.
void policy_edges() {
    const size_t cut_bytes = (size_t)33554432;
    if (shmx::kNtThresholdBytes != cut_bytes) fail_policy("the cut is not 32 MiB", 0, 0, 0);
    for (size_t sz : {size_t(2), size_t(4), size_t(8), size_t(16)}) {
        for (size_t arrays = 2; arrays <= 32; ++arrays) {
            const size_t cut = (cut_bytes + arrays * sz - 1) / (arrays * sz);   // first n at or past 32 MiB
            const size_t ns[3] = {cut - 1, cut, cut + 1};
            for (size_t n : ns) {
                const bool want = arrays * n * sz >= cut_bytes;
                if (want != (n >= cut)) fail_policy("the restated cut is not monotonic", arrays, sz, n);
                if (shmx::nt_policy(arrays, n, sz) != want) fail_policy("nt_policy", arrays, sz, n);
                const Span16 s = aligned_span(sz, n);
                if (shmx::span_elems(s, sz) != n) fail_policy("span_elems", arrays, sz, n);
                const int nt = want ? 3 : 0;
                if (arrays == 2) {
                    const shmx::LaunchChoice c = shmx::copy_choice(s, sz);
                    if (c.family != shmx::kFamilyCopy || c.maxin != 0 || c.nt != nt || c.unroll != 1 ||
                        c.blocks != blocks_restated(s.head, s.nvec, s.tail, 1))
                        fail_policy("copy_choice", arrays, sz, n);
                }
                if (arrays >= 3 && arrays <= 17) {
                    const int nins = (int)arrays - 1;
                    for (int peers = 0; peers <= 1; ++peers)
                        for (int heavy = 0; heavy <= 1; ++heavy) {
                            const shmx::LaunchChoice c = shmx::fold_choice(s, sz, nins, peers != 0, heavy != 0);
                            int family = shmx::kFamilyFoldN, maxin = 0, unroll = 4;
                            if (nins == 2) {
                                family = shmx::kFamilyFold2;
                            } else if (peers && !heavy) {
                                family = shmx::kFamilyPeers;
                                maxin = nins <= 4 ? 4 : nins <= 8 ? 8 : 16;
                                unroll = maxin == 16 ? 2 : 4;
                            }
                            if (c.family != family || c.maxin != maxin || c.unroll != unroll || c.nt != nt ||
                                c.blocks != blocks_restated(s.head, s.nvec, s.tail, unroll))
                                fail_policy("fold_choice", arrays, sz, n);
                        }
                }
                if (arrays % 2 == 0) {
                    const int nins = (int)arrays / 2;
                    const shmx::LaunchChoice c = shmx::orders_choice(s, sz, nins);
                    if (c.family != shmx::kFamilyOrders || c.maxin != (nins <= 8 ? 8 : 16) || c.unroll != 1 ||
                        c.nt != nt || c.blocks != blocks_restated(s.head, s.nvec, s.tail, 1))
                        fail_policy("orders_choice", arrays, sz, n);
                }
            }
            // exactly 32 MiB moved is non-temporal
            if (cut_bytes % (arrays * sz) == 0 && arrays * cut * sz != cut_bytes)
                fail_policy("the cut case is not exactly 32 MiB", arrays, sz, cut);
        }
        // small calls: the copy's 8 vectors per lane, and no policy bits
        const shmx::LaunchChoice c = shmx::copy_choice(aligned_span(sz, 64), sz);
        if (c.unroll != 8 || c.nt != 0 || c.blocks != 1) fail_policy("small copy_choice", 2, sz, 64);
    }
    // the scalar loop's trips over 2048 blocks of 256 lanes: B elements take
    // one trip, B + 1 two, 2 B + 257 three
    const size_t B = (size_t)2048 * 256;
    const size_t want_trips[4][2] = {{1, 1}, {B, 1}, {B + 1, 2}, {2 * B + 257, 3}};
    for (const auto &w : want_trips) {
        const Span16 s{w[0], 0, 0};
        const size_t blocks = shmx::span_blocks(s, 4);
        if (shmx::scalar_trips(s, blocks) != w[1]) fail_policy("scalar_trips", 0, 0, w[0]);
    }
}

}  // namespace

int main() {
    static_assert(shmx::kBlock == 256 && shmx::kUnrollCopy == 8 && shmx::kUnrollCopyLarge == 1,
                  "the restated rules above carry these numbers");
    long splits = 0;
    for (size_t sz : {size_t(2), size_t(4), size_t(8), size_t(16)}) {
        const size_t E = 16 / sz;
        std::vector<size_t> ns;
        for (size_t n = 0; n <= 70; ++n) ns.push_back(n);
        for (size_t n : {size_t(1) << 20, (size_t(1) << 31) + 5, (size_t(1) << 32) + 77, (size_t(1) << 43) + 5})
            ns.push_back(n);
        // the copy's boundaries: kBlock scalars, kBlock x kUnrollCopy vectors
        std::vector<size_t> copy_ns = ns;
        for (size_t n = 250; n <= 262; ++n) copy_ns.push_back(n);
        for (size_t n = 2048 * E - 2 * E; n <= 2048 * E + 2 * E; ++n) copy_ns.push_back(n);

        for (int np = 1; np <= 3; ++np) {
            const unsigned combos = 1u << (5 * np);   // 32 offsets per array
            for (unsigned c = 0; c < combos; ++c) {
                uintptr_t addr[3];
                const void *ptrs[3];
                bool same = true;
                for (int k = 0; k < np; ++k) {
                    addr[k] = (uintptr_t)0x100000 * (k + 1) + ((c >> (5 * k)) & 31u);
                    ptrs[k] = reinterpret_cast<const void *>(addr[k]);
                    same = same && (addr[k] & 15u) == (addr[0] & 15u);
                }
                const bool body = same && (addr[0] & 15u) % sz == 0;
                for (size_t n : np == 2 ? copy_ns : ns) {
                    const Span16 s = shmx::split16(ptrs, np, sz, n);
                    ++splits;
                    if (s.head + s.nvec * E + s.tail != n) fail("does not tile n", sz, addr, np, n, s);
                    if (!body) {
                        if (s.head != n || s.nvec || s.tail) fail("mixed alignment has a body", sz, addr, np, n, s);
                    } else {
                        // the first aligned element of every array
                        const size_t first = ((16 - (addr[0] & 15u)) & 15u) / sz;
                        if (s.nvec == 0 && n >= first + E) fail("no body where one fits", sz, addr, np, n, s);
                        if (s.nvec > 0) {
                            for (int k = 0; k < np; ++k)
                                if ((addr[k] + s.head * sz) & 15u) fail("body not aligned", sz, addr, np, n, s);
                            if (s.head >= E || s.tail >= E) fail("body not maximal", sz, addr, np, n, s);
                        }
                    }
                    for (int unroll : {1, 2, 4, 8})
                        if (shmx::span_blocks(s, unroll) != blocks_restated(s.head, s.nvec, s.tail, unroll))
                            fail("span_blocks differs from the grid expression", sz, addr, np, n, s);
                    if (np == 2 && n > 0 &&
                        (shmx::copy_blocks(s) == 1) != one_workgroup_restated(sz, addr[0], addr[1], n))
                        fail("one-workgroup forecast differs from copy_blocks == 1", sz, addr, np, n, s);
                }
            }
        }
    }
    policy_edges();
    if (g_fails) return 1;
    std::printf("ok %ld\n", splits);
    return 0;
}
