// The geometry every multi-PE algorithm shares: an active set's members, the
// 16-byte granule, the two-shot slices, the order a member folds its inputs
// in and the segments it gathers.  Every member of a set must compute these
// alike (a gather reads a peer's slice where the peer's fold wrote it), so
// each has one definition here.  Header-only, and host-only but for
// collect_plan and alltoallv_plan (which the kernels run too), so
// tests/native/test_set_geom.cpp checks it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>

#if defined(__HIPCC__)
#define SHMX_HOST_DEVICE __host__ __device__
#else
#define SHMX_HOST_DEVICE
#endif

namespace shmx {

// (PE_start, 1 << logPE_stride, PE_size): member i is PE start + i * step.
struct ActiveSet {
    int start = 0, step = 1, size = 0;
    // a logPE_stride outside [0, 30] (refused by the set's validation, which
    // may come later) gives step 0, which no test below takes for a stride
    static ActiveSet of(int start, int logstride, int size) {
        return ActiveSet{start, logstride >= 0 && logstride <= 30 ? 1 << logstride : 0, size};
    }
    int pe_of(int i) const { return start + i * step; }
    // the set is the whole job (a one-member set has no stride to speak of)
    bool world(int npes) const { return start == 0 && (step == 1 || size == 1) && size == npes; }
};

// elements per 16-byte granule
inline size_t granule(size_t elem_size) { return elem_size >= 16 ? 1 : 16 / elem_size; }

// The two-shot slices of n elements over P members: member i owns elements
// [lo(i), hi(i)), ceil(n / P) rounded up to the granule each, so every
// non-empty slice starts 16 bytes-aligned relative to the array; the last
// non-empty one may be short and the ones after it are empty.
struct Slices {
    size_t n, slice, elem_size;
    int P;
    Slices(size_t n_, int P_, size_t elem_size_) : n(n_), elem_size(elem_size_), P(P_) {
        const size_t g = granule(elem_size);
        slice = ((n + P - 1) / P + g - 1) / g * g;
    }
    size_t lo(int i) const { return std::min(n, (size_t)i * slice); }
    size_t hi(int i) const { return std::min(n, (size_t)(i + 1) * slice); }
    size_t count(int i) const { return hi(i) - lo(i); }
};

// ins[0..P) = at(i) for the members in set order (PE_start first), or in
// member m's own order: m first, then the others ascending
// (reduce-op.c:219-248).
template <class At>
inline void fold_inputs(const void **ins, int P, int m, bool own_order, At at) {
    int k = 0;
    if (own_order) ins[k++] = at(m);
    for (int i = 0; i < P; ++i)
        if (!own_order || i != m) ins[k++] = at(i);
}

// The non-empty slices member m gathers, as byte ranges (room for P each):
// slice i from its owner's array at base_of(i) to the same place in tgt.
// Returns how many.  rotated: from member m + 1 on, wrapping (the gather
// kernel gives its first blocks to its first segment, so the members start
// on different peers' slices and no member's HBM and links take every reader
// at once), m itself last; else ascending.  include_m: m's own slice too (its
// target is staged).
template <class BaseOf>
inline int gather_segments(const Slices &sl, int m, bool rotated, bool include_m, BaseOf base_of, char *tgt,
                           const void **from, void **to, size_t *len) {
    int k = 0;
    for (int r = 0; r < sl.P; ++r) {
        const int i = rotated ? (m + 1 + r) % sl.P : r;
        if ((i == m && !include_m) || sl.count(i) == 0) continue;
        const size_t off = sl.lo(i) * sl.elem_size;
        from[k] = base_of(i) + off;
        to[k] = tgt + off;
        len[k++] = sl.count(i) * sl.elem_size;
    }
    return k;
}

// OWNSLICE: the owner of a slice folds it once per member order and keeps
// the P - 1 results that are not its own in consecutive slots of sl.slice
// elements each, in member order with its own index left out.  The byte
// offset of member k's result in owner's slot area (k != owner); the area is
// order_slots_bytes(sl) long.
inline size_t order_slot(const Slices &sl, int owner, int k) {
    return (size_t)(k < owner ? k : k - 1) * sl.slice * sl.elem_size;
}
inline size_t order_slots_bytes(const Slices &sl) { return (size_t)(sl.P - 1) * sl.slice * sl.elem_size; }

// Elements per chunk of an OWNSLICE call whose result slots live in `half`
// bytes (half the IPC scratch): the most whose P - 1 slots, each slice rounded
// up to the granule, and a skew of < 16 bytes (the slots start at the
// sources' offset mod 16) fit; a whole number of granules, at least one.
inline size_t order_chunk_elems(size_t half, int P, size_t elem_size) {
    const size_t g = granule(elem_size);
    const size_t room = half - std::min(half, (size_t)16 * (P + 1));
    return std::max(g, (room / elem_size) / g * g);
}

// The segments member m gathers in OWNSLICE's second phase: from every other
// owner i of a non-empty slice, m's result slot in i's slot area at
// slots_of(i), to slice i of tgt; from member m + 1 on, wrapping, as the
// rotated gather above.  Returns how many (room for P - 1 each).
template <class SlotsOf>
inline int gather_order_slots(const Slices &sl, int m, SlotsOf slots_of, char *tgt, const void **from,
                              void **to, size_t *len) {
    int k = 0;
    for (int r = 0; r + 1 < sl.P; ++r) {
        const int i = (m + 1 + r) % sl.P;
        if (sl.count(i) == 0) continue;
        from[k] = slots_of(i) + order_slot(sl, i, m);
        to[k] = tgt + sl.lo(i) * sl.elem_size;
        len[k++] = sl.count(i) * sl.elem_size;
    }
    return k;
}

// The stream-ordered broadcast (pull.cpp), scatter + all-gather: the P - 1
// non-roots, in set order, own the slices of Slices(nelems, P - 1, esize);
// non-root i has slice index (i < root ? i : i - 1) and the root owns nothing.
// A one-member set has no non-root: its one slice belongs to nobody.
struct BcastSlices {
    Slices sl;
    int P, root;
    BcastSlices(size_t nelems, int P_, int root_, size_t elem_size)
        : sl(nelems, P_ > 1 ? P_ - 1 : 1, elem_size), P(P_), root(root_) {}
    int index(int i) const { return i < root ? i : i - 1; }   // i != root
    size_t lo(int i) const { return i == root ? 0 : sl.lo(index(i)); }
    size_t hi(int i) const { return i == root ? 0 : sl.hi(index(i)); }
    size_t count(int i) const { return hi(i) - lo(i); }
};

// Phase A of the broadcast: what member m pulls from the root's source at
// root_src, as byte ranges (room for 1): its slice, to the same place in tgt
// (two_phase), or the whole array (one phase).  Nothing for the root or an
// empty range.  Returns how many.
inline int bcast_from_root(const BcastSlices &b, int m, bool two_phase, const char *root_src, char *tgt,
                           const void **from, void **to, size_t *len) {
    if (m == b.root) return 0;
    const size_t lo = two_phase ? b.lo(m) : 0, hi = two_phase ? b.hi(m) : b.sl.n;
    if (hi == lo) return 0;
    from[0] = root_src + lo * b.sl.elem_size;
    to[0] = tgt + lo * b.sl.elem_size;
    len[0] = (hi - lo) * b.sl.elem_size;
    return 1;
}

// Phase B of the two-phase broadcast: every other non-root's non-empty slice,
// from that member's target at tgt_of(i), where its phase A put it, to the
// same place in tgt; from member m + 1 on, wrapping, as the rotated gather
// above.  Nothing for the root.  Returns how many (room for P - 2).
template <class TgtOf>
inline int bcast_from_peers(const BcastSlices &b, int m, TgtOf tgt_of, char *tgt, const void **from, void **to,
                            size_t *len) {
    if (m == b.root) return 0;
    int k = 0;
    for (int r = 0; r + 1 < b.P; ++r) {
        const int i = (m + 1 + r) % b.P;
        if (i == b.root || b.count(i) == 0) continue;
        const size_t off = b.lo(i) * b.sl.elem_size;
        from[k] = tgt_of(i) + off;
        to[k] = tgt + off;
        len[k++] = b.count(i) * b.sl.elem_size;
    }
    return k;
}

// fcollect: member i's nbytes of source at src_of(i) to tgt + i * nbytes, for
// all P members, from member m + 1 on, wrapping, m's own copy last.  Returns
// P (room for P).
template <class SrcOf>
inline int fcollect_segments(int P, int m, size_t nbytes, SrcOf src_of, char *tgt, const void **from, void **to,
                             size_t *len) {
    for (int r = 0; r < P; ++r) {
        const int i = (m + 1 + r) % P;
        from[r] = src_of(i);
        to[r] = tgt + (size_t)i * nbytes;
        len[r] = nbytes;
    }
    return P;
}

// The stream-ordered collect (pull.cpp): the members learn each other's
// counts on the device, and every member derives the same layout from them.
// counts[i] is member i's element count as it published it, or kCollectPoison
// for a member that could not take part (its count was above the capacity or
// past its source's room).  Member i's elements land at element offset[i] =
// sum of counts[j], j < i, of every target; total is the sum.  overflow: a
// count is poison, or the total is above `capacity` elements or its bytes
// (times esize) would wrap; the sum saturates at kCollectPoison and never
// wraps, so every member sees the same overflow.  Nothing may be written
// then, and nseg is 0.  Otherwise order[0..nseg) are the members whose
// segments member m copies: from member m + 1 on, wrapping, its own copy
// last, as fcollect_segments, the empty ones left out.  All words are 8 bytes
// wide, so the plan travels between workgroups as kCollectPlanWords words.
constexpr int kCollectMaxMembers = 16;
constexpr unsigned long long kCollectPoison = ~0ull;
struct CollectPlan {
    unsigned long long overflow;   // 0 or 1
    unsigned long long total;      // elements
    unsigned long long nseg;
    unsigned long long offset[kCollectMaxMembers];   // elements
    unsigned long long count[kCollectMaxMembers];    // the counts as read
    unsigned long long order[kCollectMaxMembers];    // members
};
constexpr int kCollectPlanWords = (int)(sizeof(CollectPlan) / sizeof(unsigned long long));

SHMX_HOST_DEVICE inline void collect_plan(const unsigned long long *counts, int P, unsigned long long capacity,
                                          unsigned long long esize, int m, CollectPlan *p) {
    unsigned long long sum = 0;
    bool bad = false;
    for (int i = 0; i < P; ++i) {
        const unsigned long long c = counts[i];
        p->offset[i] = sum;
        p->count[i] = c;
        bad |= c == kCollectPoison;
        sum = c > kCollectPoison - sum ? kCollectPoison : sum + c;
    }
    bad |= sum > capacity || sum > kCollectPoison / esize;
    p->total = sum;
    p->overflow = bad ? 1 : 0;
    int k = 0;
    for (int r = 0; r < P && !bad; ++r) {
        const int i = (m + 1 + r) % P;
        if (counts[i] != 0) p->order[k++] = (unsigned long long)i;
    }
    p->nseg = (unsigned long long)k;
}

// The stream-ordered alltoallv (pull.cpp): receiver m reads, from each member
// i, the pair (send_counts_i[m], send_offsets_i[m]) and packs what it receives
// in set order.  counts[i] / offsets[i] are those pairs as read; sender i's
// block of counts[i] elements, which starts at element from[i] = offsets[i] of
// i's source, lands at element offset[i] = sum of counts[k], k < i, of m's
// target; total is the sum.  A pair is bad if its count is above
// `src_capacity` (the elements every source holds) or its offset above
// src_capacity - count: a peer's garbage must never send a load outside that
// peer's source.  overflow: a bad pair, or the total above `capacity` or its
// bytes (times esize) wrapping; the sum saturates at kCollectPoison.  Nothing
// may be written then, and nseg is 0.  Otherwise order[0..nseg) as in
// collect_plan: from member m + 1 on, wrapping, m's own block last, the empty
// ones left out.  The fixed alltoall is the same plan with immediates: every
// count nelems, every offset m * nelems, both capacities P * nelems.
struct AlltoallvPlan {
    unsigned long long overflow;   // 0 or 1
    unsigned long long total;      // elements
    unsigned long long nseg;
    unsigned long long offset[kCollectMaxMembers];   // elements, in m's target
    unsigned long long count[kCollectMaxMembers];    // the counts as read
    unsigned long long order[kCollectMaxMembers];    // members
    unsigned long long from[kCollectMaxMembers];     // elements, in sender i's source
};
constexpr int kAlltoallvPlanWords = (int)(sizeof(AlltoallvPlan) / sizeof(unsigned long long));

SHMX_HOST_DEVICE inline void alltoallv_plan(const unsigned long long *counts, const unsigned long long *offsets, int P,
                                            unsigned long long capacity, unsigned long long src_capacity,
                                            unsigned long long esize, int m, AlltoallvPlan *p) {
    unsigned long long sum = 0;
    bool bad = false;
    for (int i = 0; i < P; ++i) {
        const unsigned long long c = counts[i], o = offsets[i];
        p->offset[i] = sum;
        p->count[i] = c;
        p->from[i] = o;
        bad |= c > src_capacity || o > src_capacity - c;
        sum = c > kCollectPoison - sum ? kCollectPoison : sum + c;
    }
    bad |= sum > capacity || sum > kCollectPoison / esize;
    p->total = sum;
    p->overflow = bad ? 1 : 0;
    int k = 0;
    for (int r = 0; r < P && !bad; ++r) {
        const int i = (m + 1 + r) % P;
        if (counts[i] != 0) p->order[k++] = (unsigned long long)i;
    }
    p->nseg = (unsigned long long)k;
}

}  // namespace shmx
