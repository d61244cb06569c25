// How the fold-family kernels (fold_kernels.hip) cut n elements into a scalar
// head, a body of 16-byte vectors and a scalar tail, and how many workgroups
// such a launch takes.  The staging path (copy_one_workgroup) relies on the
// launch and its own forecast agreeing, so each rule has one definition here.
// Header-only and host-only, so tests/native/test_span16.cpp checks it on the
// CPU.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>

namespace shmx {

constexpr int kBlock = 256;  // lanes per workgroup: 4 waves of 64

struct Span16 {
    size_t head;   // scalar elements before the first 16-B aligned vector
    size_t nvec;   // 16-B vectors in the aligned body
    size_t tail;   // scalar elements after it
};

// The body exists only if all nptrs arrays share one offset mod 16 that is a
// whole number of elements; otherwise (and for an unknown element size) all n
// elements are head.
inline Span16 split16(const void *const *ptrs, int nptrs, size_t elem_size, size_t n) {
    const uintptr_t off = reinterpret_cast<uintptr_t>(ptrs[0]) & 15u;
    bool same = elem_size && (off % elem_size) == 0;
    for (int k = 1; k < nptrs && same; ++k) same = (reinterpret_cast<uintptr_t>(ptrs[k]) & 15u) == off;
    if (!same) return Span16{n, 0, 0};
    size_t head = ((16 - off) & 15u) / elem_size;
    if (head > n) head = n;
    const size_t E = 16 / elem_size, nvec = (n - head) / E;
    return Span16{head, nvec, n - head - nvec * E};
}

// One chunk of kBlock x unroll vectors per block (persistent grids, caps and
// XCD remaps measured no faster: DESIGN_history.md §4.2); the scalar-only
// case (inputs of different alignment) grid-strides over at most 2048 blocks.
inline size_t span_blocks(const Span16 &s, int unroll) {
    const size_t chunk = (size_t)kBlock * unroll;
    size_t blocks = s.nvec > 0 ? (s.nvec + chunk - 1) / chunk : (s.head + s.tail + kBlock - 1) / kBlock;
    const size_t cap = s.nvec == 0 ? 2048 : (size_t)1 << 30;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    if (blocks > (size_t)INT_MAX) blocks = INT_MAX;
    return blocks;
}

// The copy's shape (fold_kernels.hip, launch_copy_nt): up to 32 KiB of body,
// 8 vectors per lane, so the copy is one workgroup that can store the host
// signal itself; beyond, one vector per lane, 4 KiB per workgroup.
constexpr int kUnrollCopy = 8;
constexpr int kUnrollCopyLarge = 1;
inline bool copy_small(const Span16 &s) { return s.nvec <= (size_t)kBlock * kUnrollCopy; }
inline size_t copy_blocks(const Span16 &s) {
    return span_blocks(s, copy_small(s) ? kUnrollCopy : kUnrollCopyLarge);
}

}  // namespace shmx
