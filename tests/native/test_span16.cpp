// CPU test of the fold-family kernels' split and grid rules (csrc/span16.h):
// for element sizes 2 / 4 / 8 / 16, 1 to 3 arrays at every byte offset 0-31
// each, and n in 0-70 plus large values (one above 2^32, one past the block
// cap), split16 tiles [0, n) as head + vectors + tail; a body, where there is
// one, starts 16 B-aligned in every array, is as long as it can be and leaves
// less than a vector on either side; arrays of different offsets, or an
// offset that is no whole number of elements, give {n, 0, 0}; span_blocks
// equals the launch's grid expression, restated here; and the forecast "this
// copy is one workgroup" equals copy_blocks == 1, around the three boundaries
// (kBlock scalars, kBlock x kUnrollCopy vectors, and one more).
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
    if (g_fails) return 1;
    std::printf("ok %ld\n", splits);
    return 0;
}
