// How the fold-family kernels (fold_kernels.hip) cut n elements into a scalar
// head, a body of 16-byte vectors and a scalar tail, how many workgroups such
// a launch takes, and which kernel instance it is: family, inputs unrolled,
// vectors per lane, cache policy.  The staging path (copy_one_workgroup) and
// the launch-shape query (shmemx_fold_launch_shape) rely on the launch and
// their own forecast agreeing, so each rule has one definition here.
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

// ------------------------------------------------------------ cache policy
// Working sets of 32 MiB and more go non-temporal on both loads and stores.
// Round 1 set the cut at the 256 MiB Infinity Cache from back-to-back (warm)
// runs; round 3 measured the 4-64 Mi-float fold cold
// (tools/cold_midsize_probe.py, profiles/r03_cold_midsize.txt): after a
// producer's writes leave dirty lines in the MALL, the default policy runs
// 3.1 / 4.1 TB/s at 48 / 192 MiB against 4.3 / 5.8 non-temporal (the
// default's stores evict those lines and pay their write-back); from a clean
// cache the default leads by 5-7 %, back to back the two tie.  So
// non-temporal, whose worst case is the better one, from 32 MiB up; below
// it a call is launch-bound and the default keeps L2/MALL hits.  (Loads or
// stores alone non-temporal, and the sc0/sc1 bits, measured no better:
// profiles/r03_policy_lab*.txt.)
// `arrays` is how many arrays of n elements the call moves: nins + 1 for a
// fold (its inputs and its output), 2 for the copy, 2 nins for the P-order
// fold (P reads, P writes).
constexpr size_t kNtThresholdBytes = size_t(32) << 20;
constexpr int kNtBoth = 3;   // fold_ops.h ld16 / st16: bit 0 loads, bit 1 stores
inline bool nt_policy(size_t arrays, size_t n, size_t elem_size) {
    return arrays * n * elem_size >= kNtThresholdBytes;
}

// ----------------------------------------------------------- launch choice
// Which kernel instance a call launches, and its grid.  The launchers of
// fold_kernels.hip switch on a LaunchChoice and nothing else, and
// shmemx_fold_launch_shape reports the same one, so what the tests are told
// was launched is what was launched.
enum FoldFamily {
    kFamilyFold2 = 0,    // fold_kernel<T, OP, 2, kUnrollFold2, NT>
    kFamilyFoldN = 1,    // fold_kernel<T, OP, 0, kUnrollN, NT>: run-time input count
    kFamilyPeers = 2,    // fold_peers_kernel<T, OP, MAXIN, NT>
    kFamilyOrders = 3,   // fold_orders_kernel<T, OP, MAXIN, NT>
    kFamilyCopy = 4,     // fold_kernel<T, SUM, 1, kUnrollCopy | kUnrollCopyLarge, NT>
};
struct LaunchChoice {
    int family;      // FoldFamily
    int maxin;       // inputs unrolled at compile time (peers, orders); else 0
    int unroll;      // 16-byte vectors per lane per input in a chunk
    int nt;          // 0, or kNtBoth
    size_t blocks;   // the grid
};

// 16-B vectors per lane per input for the runtime-nins kernel, and for the
// two-input fold (2 and 8 measured no faster at 32-64 Mi elements:
// DESIGN_history.md §4.2); for the peers kernels 4 up to 8 inputs (32
// vectors in registers), 2 up to 16; one for the P-order fold
// (fold_kernels.hip has the measurements behind each).
constexpr int kUnrollN = 4;
constexpr int kUnrollFold2 = 4;
constexpr int peers_unroll(int maxin) { return maxin <= 8 ? 4 : 2; }
constexpr int kUnrollOrders = 1;

inline size_t span_elems(const Span16 &s, size_t elem_size) { return s.head + s.nvec * (16 / elem_size) + s.tail; }

// A fold of nins >= 2 inputs.  Two inputs: the two-input kernel, whatever the
// route.  More, on the peers route: the peers kernel for up to 4, 8 or 16
// inputs, except for a heavy pair (fold_ops.h kHeavyOp: long double and the
// complex products), which keeps the runtime-nins kernel as every fold of
// the plain route does.
inline LaunchChoice fold_choice(const Span16 &s, size_t elem_size, int nins, bool peers, bool heavy) {
    LaunchChoice c{};
    if (nins == 2) {
        c.family = kFamilyFold2;
        c.unroll = kUnrollFold2;
    } else if (peers && !heavy) {
        c.family = kFamilyPeers;
        c.maxin = nins <= 4 ? 4 : nins <= 8 ? 8 : 16;
        c.unroll = peers_unroll(c.maxin);
    } else {
        c.family = kFamilyFoldN;
        c.unroll = kUnrollN;
    }
    c.nt = nt_policy((size_t)nins + 1, span_elems(s, elem_size), elem_size) ? kNtBoth : 0;
    c.blocks = span_blocks(s, c.unroll);
    return c;
}

// The copy (one input).
inline LaunchChoice copy_choice(const Span16 &s, size_t elem_size) {
    LaunchChoice c{};
    c.family = kFamilyCopy;
    c.unroll = copy_small(s) ? kUnrollCopy : kUnrollCopyLarge;
    c.nt = nt_policy(2, span_elems(s, elem_size), elem_size) ? kNtBoth : 0;
    c.blocks = copy_blocks(s);
    return c;
}

// The P-order fold: nins inputs, nins outputs.
inline LaunchChoice orders_choice(const Span16 &s, size_t elem_size, int nins) {
    LaunchChoice c{};
    c.family = kFamilyOrders;
    c.maxin = nins <= 8 ? 8 : 16;
    c.unroll = kUnrollOrders;
    c.nt = nt_policy(2 * (size_t)nins, span_elems(s, elem_size), elem_size) ? kNtBoth : 0;
    c.blocks = span_blocks(s, c.unroll);
    return c;
}

// Trips of the kernels' grid-stride loop over the scalar head and tail
// (for_scalar_edges): the whole array when the operands differ mod 16.
inline size_t scalar_trips(const Span16 &s, size_t blocks) {
    const size_t nthr = blocks * kBlock;
    return nthr ? (s.head + s.tail + nthr - 1) / nthr : 0;
}

}  // namespace shmx
