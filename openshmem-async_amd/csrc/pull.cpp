// Stream-ordered barrier, broadcast and fcollect: the
// collectives next to every reduction, as pure stream work under SIGNAL's
// device barriers (signal.cpp) — no host wait, no host barrier, no descriptor
// exchange, capturable into a hipGraph after one warm call of the set has
// mapped the peers' heaps.
//
// Operands must be symmetric — target and source both in the heap on every
// member — so every member computes every peer's address from its own
// offsets.  A call whose operands are not returns ENOTSUP before any launch;
// every refusal depends on what the members share (sizes, offsets, set, root,
// settings), so no member refuses alone.
//
//   barrier    flush of the mirrored heap's view, system fence, signal wave.
//   fcollect   barrier                 every source is final; nobody reads my target
//              gather                  all P sources -> my target (set_geom.h
//                                      fcollect_segments: from member m + 1
//                                      on, my own copy last)
//              barrier                 nobody reads my source any more
//   broadcast  one phase (P == 2, or up to $SHMEMX_BCAST_TWOPHASE_KB): every
//              non-root pulls the whole array from the root between two
//              barriers: S over the one link to the root.
//              two phase (scatter + all-gather): the P - 1 non-roots own the
//              slices of Slices(nelems, P - 1, esize):
//              barrier                 the root's source is final
//              gather A                my slice from the root's source
//              barrier                 every non-root's slice is final
//              gather B                the other slices from the other
//                                      non-roots' targets
//              barrier                 nobody reads my source or target any more
//              — 2 S / (P - 1) per link over P - 1 links at once.  The root
//              runs every barrier and writes nothing (its target is never
//              written, as in the blocking call).
//   collect    the counts are known only to their owners, and no host learns
//              them: each member publishes its count (an immediate, or a word
//              of device memory read when the call executes) in a word of its
//              own signal area, reads the others' after the entry barrier and
//              derives the layout (set_geom.h collect_plan):
//              publish                 my count, or poison if it cannot be served
//              barrier                 every source and count is final
//              plan                    one thread reads the P counts
//              copy                    every non-empty source -> its prefix-sum
//                                      offset of my target (from member m + 1
//                                      on, my own copy last); nothing on overflow
//              barrier                 nobody reads my source or count any more
//              The target's capacity is the one size the members share: the
//              route and the grid come from it alone.
//   alltoallv  the collect's all-to-all generalisation, and the fixed alltoall
//              with it: member i's send_counts[j] elements from element
//              send_offsets[j] of its source go to member j, which packs what
//              it receives in set order.  The two tables are symmetric
//              objects, final before the entry barrier like the sources, so
//              nothing is published and no signal-area word is used:
//              barrier                 every source and table is final
//              plan                    one thread reads the P (count, offset)
//                                      pairs meant for me (set_geom.h
//                                      alltoallv_plan; none for the fixed form)
//              copy                    every non-empty block -> its prefix-sum
//                                      offset of my target; nothing if a pair
//                                      is bad or the total is over capacity
//              barrier                 nobody reads my source or tables any more
//              An overflow is the receiver's alone; its peers complete.
//   reduce-    the one collective here that folds: SIGNAL's two shot without
//   scatter    its second phase.  Member m's target is the set-
//              order fold of block m of every member's source:
//              barrier                 every source is final; nobody reads my target
//              fold                    block m of all P sources -> my target
//              barrier                 nobody reads my source any more
//              One launch (launch_signal_reduce_scatter) while the source's
//              P * nelems * size bytes are within $SHMEMX_FUSED_TWOSHOT_KB,
//              above it the unfused barriers around launch_fold_peers.
// Up to $SHMEMX_FUSED_TWOSHOT_KB (the array for a broadcast, the P-fold target
// for an fcollect, the target's capacity for a collect or an alltoallv) a call
// is ONE launch, launch_signal_pull / launch_signal_collect /
// launch_signal_alltoallv; above it the unfused barriers (launch_sys_fence +
// launch_signal) around launch_gather, or around the collect's publish, plan
// and copy launches, or the alltoallv's plan and copy.
//
// Calls of one PE must not overlap in time (they share the grid barrier's
// words with SIGNAL's launches): one stream, or stream order between them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "heap.h"
#include "internal.h"
#include "node.h"
#include "set_geom.h"
#include "shmem_reduce_mi355x.h"
#include "state.h"

namespace shmx {

namespace {

// The one-phase / two-phase crossover of the broadcast, derived, not measured
// (unmeasured on xGMI, the first 8-GPU run sets it): one phase
// costs S / BW, two phases 2 S / ((P - 1) BW) + t for the one handshake more,
// so S* = t BW (P - 1) / (P - 3); with t = 6.2 us (half of the 12.38 us a
// whole fused one-shot call with its two handshakes takes,
// profiles/r05_fused_blocks.txt), BW = 153 GB/s and P = 8: 1.33 MB, rounded
// up to a power of two in KiB.
constexpr long kDefaultBcastTwoPhaseKb = 2048;

long twophase_kb_from_env() {
    const char *e = std::getenv("SHMEMX_BCAST_TWOPHASE_KB");
    return e ? std::max(0L, std::atol(e)) : kDefaultBcastTwoPhaseKb;
}
long g_bcast_twophase_kb = twophase_kb_from_env();

size_t bcast_twophase_bytes() { return size_t(g_bcast_twophase_kb) << 10; }

// shmemx_pull_stats
enum { kBarriers = 0, kBroadcasts, kFcollects, kFusedCalls, kTwoPhase, kNumStats };
unsigned long long g_stats[kNumStats];

enum { kFcollect = 0, kBroadcast = 1 };

// How a call of `bytes` per member over P members runs: schedule 0 nothing to
// do, 1 one phase, 2 two phases; fused: as one launch.  Shared inputs only.
struct Route {
    int schedule;
    bool fused;
};
Route route_of(int kind, size_t bytes, int P) {
    if (!bytes || P < 2) return Route{0, false};
    if (kind == kFcollect) return Route{1, (size_t)P * bytes <= fused_twoshot_bytes()};
    const bool two = P > 2 && bytes > bcast_twophase_bytes();
    return Route{two ? 2 : 1, bytes <= fused_twoshot_bytes()};
}

bool set_shape_ok(int start, int logstride, int size) {
    return start >= 0 && logstride >= 0 && logstride <= 30 && size >= 1;
}

// nelems * esize * 16 members must not wrap
bool size_ok(size_t esize, size_t nelems) { return nelems <= SIZE_MAX / (esize * kMaxFoldInputs); }

bool ranges_meet(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// The caller's set, its index in it and, after map_members, the device
// barrier's arguments and the members' heap bases.
struct Members {
    ActiveSet set;
    int m = -1;
    SignalArgs sa;
    std::vector<char *> hb;
};

// After the argument checks: the job is up, the set lies inside it and the
// caller is a member.
int enter(int start, int logstride, int size, Members *mb) {
    if (int rc = ensure_init()) return rc;
    if ((long long)start + (long long)(size - 1) * (1LL << logstride) >= g_state.npes)
        return set_error(SHMEMX_EINVAL);
    mb->set = ActiveSet::of(start, logstride, size);
    if (!is_member(g_state.pe, start, logstride, size, &mb->m)) return set_error(SHMEMX_ENOTMEMBER);
    return SHMEMX_OK;
}

// The peers' heap segments (mapped and voted on the first time the set meets
// them, plain lookups afterwards) and the signal counters in them.
int map_members(Members *mb) {
    const int P = mb->set.size;
    if (!node::up() || P > kMaxFoldInputs || !heap::signal_area()) return set_error(SHMEMX_ENOTSUP);
    std::vector<std::pair<node::Region, int>> regs;
    for (int i = 0; i < P; ++i) regs.emplace_back(node::kHeap, mb->set.pe_of(i));
    if (!map_regions(regs, mb->set)) {
        trace(LOG_INFO, "stream-ordered pull: a member could not map a peer heap (%s)", node::last_ipc_error());
        return set_error(SHMEMX_ENOTSUP);
    }
    if (!signal_args(mb->set, &mb->sa)) return set_error(SHMEMX_ENOTSUP);
    mb->hb.resize(P);
    for (int i = 0; i < P; ++i) mb->hb[i] = node::peer_base(node::kHeap, mb->set.pe_of(i));
    return SHMEMX_OK;
}

hipStream_t stream_of(void *stream) {
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : g_state.stream;
    if (s == g_state.stream) g_state.lib_stream_dirty = true;   // (service.hip)
    return s;
}

void device_barrier(const SignalArgs &sa, hipStream_t s) {
    SHMX_HIP(launch_sys_fence(s, sa.seen));
    SHMX_HIP(launch_signal(sa, s));
}

SignalPullArgs pull_args(const SignalArgs &sa, bool two_phase) {
    SignalPullArgs pa{};
    pa.sig = sa;
    pa.gsync = fence_records().gsync;
    pa.two_phase = two_phase ? 1 : 0;
    return pa;
}

// One call's lists, fused or between the unfused barriers.
void run(const SignalPullArgs &pa, bool fused, hipStream_t s) {
    if (fused) {
        SHMX_HIP(launch_signal_pull(pa, s));
        return;
    }
    device_barrier(pa.sig, s);   // every source is final; nobody still reads my target
    SHMX_HIP(launch_gather(pa.a.gsrc, pa.a.gdst, pa.a.glen, pa.a.nseg, s));
    if (pa.two_phase) {
        device_barrier(pa.sig, s);   // every non-root's slice is final
        SHMX_HIP(launch_gather(pa.b.gsrc, pa.b.gdst, pa.b.glen, pa.b.nseg, s));
    }
    device_barrier(pa.sig, s);   // nobody reads my source or target any more
}

int broadcast_on_stream(size_t esize, void *target, const void *source, size_t nelems, int root, int start,
                        int logstride, int size, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!set_shape_ok(start, logstride, size) || root < 0 || root >= size || !size_ok(esize, nelems))
        return set_error(SHMEMX_EINVAL);
    const size_t bytes = nelems * esize;
    if (bytes && (!target || !source)) return set_error(SHMEMX_EINVAL);
    if (bytes && overlap(target, source, bytes)) return set_error(SHMEMX_EINVAL);   // partial; in place is allowed
    Members mb;
    if (int rc = enter(start, logstride, size, &mb)) return rc;
    const int P = size, m = mb.m;
    trace(LOG_BROADCAST, "stream-ordered: %zu bytes from set member %d, set (%d,%d,%d) member %d", bytes, root,
          start, logstride, size, m);
    const Route rt = route_of(kBroadcast, bytes, P);
    if (!rt.schedule) return SHMEMX_OK;   // the root's target is never written
    uint64_t soff = 0, toff = 0;
    if (!heap::offset_of(heap::twin(source), bytes, &soff) || !heap::offset_of(heap::twin(target), bytes, &toff))
        return set_error(SHMEMX_ENOTSUP);
    if (int rc = map_members(&mb)) return rc;
    hipStream_t s = stream_of(stream);
    // mirrored heap: the root's host stores go to HBM, a non-root's target is
    // DEVICE_NEWER from here; the root opens no write
    if (m == root) (void)heap::device_operand(source, bytes);
    heap::DeviceWrite tw(m == root ? nullptr : target, bytes, s);
    char *const tgt = mb.hb[m] + toff;
    const bool two = rt.schedule == 2;
    const BcastSlices bs(nelems, P, root, esize);
    SignalPullArgs pa = pull_args(mb.sa, two);
    pa.a.nseg = bcast_from_root(bs, m, two, mb.hb[root] + soff, tgt, pa.a.gsrc, pa.a.gdst, pa.a.glen);
    if (two)
        pa.b.nseg = bcast_from_peers(bs, m, [&](int i) { return mb.hb[i] + toff; }, tgt, pa.b.gsrc, pa.b.gdst,
                                     pa.b.glen);
    run(pa, rt.fused, s);
    g_stats[kBroadcasts] += 1;
    g_stats[kFusedCalls] += rt.fused;
    g_stats[kTwoPhase] += two;
    return SHMEMX_OK;
}

int fcollect_on_stream(size_t esize, void *target, const void *source, size_t nelems, int start, int logstride,
                       int size, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!set_shape_ok(start, logstride, size) || !size_ok(esize, nelems)) return set_error(SHMEMX_EINVAL);
    const size_t nbytes = nelems * esize;
    if (nbytes && (!target || !source)) return set_error(SHMEMX_EINVAL);
    if (nbytes && ranges_meet(target, (size_t)size * nbytes, source, nbytes)) return set_error(SHMEMX_EINVAL);
    Members mb;
    if (int rc = enter(start, logstride, size, &mb)) return rc;
    const int P = size, m = mb.m;
    trace(LOG_COLLECT, "stream-ordered fcollect: %zu bytes mine, set (%d,%d,%d) member %d", nbytes, start, logstride,
          size, m);
    if (!nbytes) return SHMEMX_OK;
    if (P == 1) {
        // no kernel: the one member's source is its whole result
        hipStream_t s = stream_of(stream);
        const void *src = heap::device_operand(source, nbytes);
        heap::DeviceWrite tw(target, nbytes, s);
        SHMX_HIP(hipMemcpyAsync(tw.ptr(), src, nbytes, hipMemcpyDefault, s));
        return SHMEMX_OK;
    }
    const Route rt = route_of(kFcollect, nbytes, P);
    uint64_t soff = 0, toff = 0;
    if (!heap::offset_of(heap::twin(source), nbytes, &soff) ||
        !heap::offset_of(heap::twin(target), (size_t)P * nbytes, &toff))
        return set_error(SHMEMX_ENOTSUP);
    if (int rc = map_members(&mb)) return rc;
    hipStream_t s = stream_of(stream);
    (void)heap::device_operand(source, nbytes);
    heap::DeviceWrite tw(target, (size_t)P * nbytes, s);
    SignalPullArgs pa = pull_args(mb.sa, false);
    pa.a.nseg = fcollect_segments(P, m, nbytes, [&](int i) { return mb.hb[i] + soff; }, mb.hb[m] + toff, pa.a.gsrc,
                                  pa.a.gdst, pa.a.glen);
    run(pa, rt.fused, s);
    g_stats[kFcollects] += 1;
    g_stats[kFusedCalls] += rt.fused;
    return SHMEMX_OK;
}

// ------------------------------------------------------------- collect
// shmemx_collect_stats: [collects, those that ran as one fused launch]; the
// overflows are counted on the device, in CollectState::overflows.
enum { kCollects = 0, kCollectsFused, kNumCollectStats };
unsigned long long g_collect_stats[kNumCollectStats];

// What the collect kernels need besides the operands, made on first use
// (under capture the warm call has made it) and kept: the plan buffer, and a
// private array of count words, a count and a where[] for the one-member set
// and the loopback hook, all device memory; the overflow counter, host-mapped.
struct CollectState {
    unsigned long long *plan = nullptr;    // kCollectPlanWords
    unsigned long long *words = nullptr;   // kMaxFoldInputs
    unsigned long long *count = nullptr;   // 1
    unsigned long long *where = nullptr;   // 2
    unsigned long long *overflows = nullptr;
};
CollectState g_collect;

bool collect_state() {
    if (g_collect.plan) return true;
    void *d = nullptr, *h = nullptr;
    const size_t words = kCollectPlanWords + kMaxFoldInputs + 1 + 2;
    if (hipMalloc(&d, words * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(d, 0, words * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc(&h, sizeof(unsigned long long), hipHostMallocCoherent) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        return false;
    }
    *static_cast<volatile unsigned long long *>(h) = 0;
    g_collect.plan = static_cast<unsigned long long *>(d);
    g_collect.words = g_collect.plan + kCollectPlanWords;
    g_collect.count = g_collect.words + kMaxFoldInputs;
    g_collect.where = g_collect.count + 1;
    g_collect.overflows = static_cast<unsigned long long *>(h);
    return true;
}

bool collect_route_fused(size_t esize, size_t capacity) { return capacity * esize <= fused_twoshot_bytes(); }

bool elem_aligned(const void *p, size_t esize) { return reinterpret_cast<uintptr_t>(p) % esize == 0; }

// The elements member-local reads of a source at `src` may cover: up to the
// target where the source lies below it (a source that starts inside the
// target is refused on the host), and no further than `limit` elements.
unsigned long long source_room(const char *src, const char *tgt, size_t esize, unsigned long long limit) {
    if (src < tgt) limit = std::min<unsigned long long>(limit, (unsigned long long)(tgt - src) / esize);
    return limit;
}

// One call's launches.  Fused: one.  Unfused: publish, the two launches of a
// barrier, plan, copy, the two launches of a barrier: seven.
void run_collect(const SignalCollectArgs &ca, bool fused, hipStream_t s) {
    if (fused) {
        SHMX_HIP(launch_signal_collect(ca, s));
        return;
    }
    SHMX_HIP(launch_collect_publish(ca.c, s));
    device_barrier(ca.sig, s);   // every source and count is final; nobody still reads my target
    SHMX_HIP(launch_collect_plan(ca.c, s));
    SHMX_HIP(launch_collect_copy(ca.c, s));
    device_barrier(ca.sig, s);   // nobody reads my source, my target or my count any more
}

// The count word.  Each member's count is ONE 8-byte word in its own signal
// area (heap::count_word_offset(), past the barrier counters); peer i's is at
// peer_base(i) + signal_offset + that offset, as signal_args finds the
// counters.  One word per member suffices for every call of every set:
//   - a peer reads my word only between its entry and its exit handshake of
//     the call that published it (the exchange follows the entry handshake in
//     the same thread, or in stream order);
//   - I overwrite it only in my next call, which starts (stream order, and
//     calls of one PE never overlap) after my exit handshake of this call has
//     seen every peer's exit counter, so every peer's read is behind it.
// A member that is in two sets runs their calls one after the other, so the
// argument holds across sets too.
int collect_on_stream(size_t esize, void *target, const void *source, size_t nelems,
                      const unsigned long long *nelems_dev, unsigned long long *where_dev, bool counted,
                      size_t capacity, int start, int logstride, int size, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!set_shape_ok(start, logstride, size) || !size_ok(esize, capacity)) return set_error(SHMEMX_EINVAL);
    if (counted && !nelems_dev) return set_error(SHMEMX_EINVAL);
    if ((reinterpret_cast<uintptr_t>(nelems_dev) | reinterpret_cast<uintptr_t>(where_dev)) % 8)
        return set_error(SHMEMX_EINVAL);
    const size_t cbytes = capacity * esize;
    if (capacity && (!target || !source)) return set_error(SHMEMX_EINVAL);
    // whole elements: the offsets are symmetric, so this is a shared fact
    if (capacity && (!elem_aligned(target, esize) || !elem_aligned(source, esize))) return set_error(SHMEMX_EINVAL);
    // a source that STARTS inside the target; how far it reaches is a
    // member-local fact, which the device judges
    if (capacity && ranges_meet(target, cbytes, source, 1)) return set_error(SHMEMX_EINVAL);
    Members mb;
    if (int rc = enter(start, logstride, size, &mb)) return rc;
    const int P = size, m = mb.m;
    trace(LOG_COLLECT, "stream-ordered collect: capacity %zu elements of %zu bytes, set (%d,%d,%d) member %d",
          capacity, esize, start, logstride, size, m);
    if (!capacity) return SHMEMX_OK;
    const bool fused = collect_route_fused(esize, capacity);
    SignalCollectArgs ca{};
    CollectArgs &c = ca.c;
    unsigned long long limit = kCollectPoison >> 1;   // the source's room in the heap, elements
    if (P == 1) {
        // no peer: any device memory serves, a private count word, no handshake
        if (!loopback_signal_args(1, &ca.sig) || !collect_state()) return set_error(SHMEMX_ENOMEM);
        ca.sig.timeout_ticks = signal_timeout_ticks();
        uint64_t soff = 0;
        if (heap::offset_of(heap::twin(source), esize, &soff)) limit = (heap::signal_offset() - soff) / esize;
        c.my_word = g_collect.words;
        c.word[0] = g_collect.words;
        c.src[0] = heap::twin(source);
        c.tgt = heap::twin(target);
    } else {
        uint64_t soff = 0, toff = 0;
        if (!heap::offset_of(heap::twin(source), esize, &soff) || !heap::offset_of(heap::twin(target), cbytes, &toff))
            return set_error(SHMEMX_ENOTSUP);
        if (int rc = map_members(&mb)) return rc;
        if (!collect_state()) return set_error(SHMEMX_ENOMEM);
        ca.sig = mb.sa;
        limit = (heap::signal_offset() - soff) / esize;
        const uint64_t woff = heap::signal_offset() + heap::count_word_offset();
        for (int i = 0; i < P; ++i) {
            c.word[i] = reinterpret_cast<const unsigned long long *>(mb.hb[i] + woff);
            c.src[i] = mb.hb[i] + soff;
        }
        c.my_word = reinterpret_cast<unsigned long long *>(mb.hb[m] + woff);
        c.tgt = mb.hb[m] + toff;
    }
    hipStream_t s = stream_of(stream);
    ca.gsync = fence_records().gsync;
    c.P = P;
    c.m = m;
    c.esize = (unsigned int)esize;
    c.capacity = capacity;
    c.src_room = source_room(static_cast<const char *>(c.src[m]), static_cast<const char *>(c.tgt), esize, limit);
    c.count = counted ? 0 : nelems;
    c.count_dev = counted ? static_cast<const unsigned long long *>(heap::device_operand(nelems_dev, 8)) : nullptr;
    c.where = static_cast<unsigned long long *>(heap::twin(where_dev));
    c.plan = g_collect.plan;
    c.overflows = g_collect.overflows;
    // mirrored heap: the host's stores to the source go to HBM for the bound
    // the host knows (the count, or the room up to the capacity); the target
    // is DEVICE_NEWER for the whole capacity from here
    const unsigned long long known = std::min<unsigned long long>(counted ? capacity : std::min(nelems, capacity), limit);
    (void)heap::device_operand(source, (size_t)known * esize);
    heap::DeviceWrite tw(target, cbytes, s);
    heap::DeviceWrite ww(where_dev, where_dev ? 2 * sizeof(unsigned long long) : 0, s);
    run_collect(ca, fused, s);
    g_collect_stats[kCollects] += 1;
    g_collect_stats[kCollectsFused] += fused;
    return SHMEMX_OK;
}

// ------------------------------------------------ alltoall, alltoallv
// shmemx_alltoall_stats: [alltoalls, alltoallvs, of those fused]; the
// overflows are counted on the device, in AlltoallState::overflows.
enum { kAlltoalls = 0, kAlltoallvs, kAlltoallFused, kNumAlltoallStats };
unsigned long long g_alltoall_stats[kNumAlltoallStats];

// What the alltoallv kernels need besides the operands, made on first use
// (under capture the warm call has made it) and kept: the plan buffer and,
// for the loopback hook, private P x P count and offset tables and a where[],
// all device memory; the overflow counter, host-mapped.
struct AlltoallState {
    unsigned long long *plan = nullptr;      // kAlltoallvPlanWords
    unsigned long long *counts = nullptr;    // kMaxFoldInputs^2
    unsigned long long *offsets = nullptr;   // kMaxFoldInputs^2
    unsigned long long *where = nullptr;     // kMaxFoldInputs + 1
    unsigned long long *overflows = nullptr;
};
AlltoallState g_alltoall;
constexpr size_t kTableWords = (size_t)kMaxFoldInputs * kMaxFoldInputs;

bool alltoall_state() {
    if (g_alltoall.plan) return true;
    void *d = nullptr, *h = nullptr;
    const size_t words = kAlltoallvPlanWords + 2 * kTableWords + kMaxFoldInputs + 1;
    if (hipMalloc(&d, words * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(d, 0, words * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc(&h, sizeof(unsigned long long), hipHostMallocCoherent) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        return false;
    }
    *static_cast<volatile unsigned long long *>(h) = 0;
    g_alltoall.plan = static_cast<unsigned long long *>(d);
    g_alltoall.counts = g_alltoall.plan + kAlltoallvPlanWords;
    g_alltoall.offsets = g_alltoall.counts + kTableWords;
    g_alltoall.where = g_alltoall.offsets + kTableWords;
    g_alltoall.overflows = static_cast<unsigned long long *>(h);
    return true;
}

// One call's launches.  Fused: one.  Unfused: the two launches of a barrier,
// plan, copy, the two launches of a barrier: six.  Nothing is published: the
// tables already live in the heap.
hipError_t launch_alltoallv(const SignalAlltoallvArgs &aa, bool fused, hipStream_t s) {
    if (fused) return launch_signal_alltoallv(aa, s);
    hipError_t e = launch_sys_fence(s, aa.sig.seen);   // every source and table is final; nobody reads my target
    if (e == hipSuccess) e = launch_signal(aa.sig, s);
    if (e == hipSuccess) e = launch_alltoallv_plan(aa.c, s);
    if (e == hipSuccess) e = launch_alltoallv_copy(aa.c, s);
    if (e == hipSuccess) e = launch_sys_fence(s, aa.sig.seen);   // nobody reads my source or my tables any more
    if (e == hipSuccess) e = launch_signal(aa.sig, s);
    return e;
}

// counts == nullptr: the fixed alltoall of `nelems` elements per pair
// (capacity == src_capacity == size * nelems, the caller's product).
int alltoallv_on_stream(size_t esize, void *target, const void *source, const unsigned long long *counts,
                        const unsigned long long *offsets, bool fixed, size_t nelems, unsigned long long *where_dev,
                        size_t capacity, size_t src_capacity, int start, int logstride, int size, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!set_shape_ok(start, logstride, size)) return set_error(SHMEMX_EINVAL);
    if (fixed) {
        if (nelems > SIZE_MAX / (esize * kMaxFoldInputs) / (size_t)size) return set_error(SHMEMX_EINVAL);
        capacity = src_capacity = (size_t)size * nelems;
    }
    if (!size_ok(esize, capacity) || !size_ok(esize, src_capacity)) return set_error(SHMEMX_EINVAL);
    const size_t cbytes = capacity * esize, sbytes = src_capacity * esize;
    const size_t tbytes = (size_t)size * sizeof(unsigned long long);
    const bool work = capacity && src_capacity;
    if (!fixed && (!counts || !offsets)) return set_error(SHMEMX_EINVAL);
    if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(offsets) |
         reinterpret_cast<uintptr_t>(where_dev)) % 8)
        return set_error(SHMEMX_EINVAL);
    if (work && (!target || !source)) return set_error(SHMEMX_EINVAL);
    // whole elements: the offsets are symmetric, so this is a shared fact
    if (work && (!elem_aligned(target, esize) || !elem_aligned(source, esize))) return set_error(SHMEMX_EINVAL);
    // target, source and the two tables pairwise disjoint: symmetric offsets again
    if (work && ranges_meet(target, cbytes, source, sbytes)) return set_error(SHMEMX_EINVAL);
    if (work && !fixed &&
        (ranges_meet(target, cbytes, counts, tbytes) || ranges_meet(target, cbytes, offsets, tbytes) ||
         ranges_meet(source, sbytes, counts, tbytes) || ranges_meet(source, sbytes, offsets, tbytes) ||
         ranges_meet(counts, tbytes, offsets, tbytes)))
        return set_error(SHMEMX_EINVAL);
    Members mb;
    if (int rc = enter(start, logstride, size, &mb)) return rc;
    const int P = size, m = mb.m;
    trace(LOG_COLLECT, "stream-ordered alltoall%s: capacity %zu, source %zu elements of %zu bytes, set (%d,%d,%d) member %d",
          fixed ? "" : "v", capacity, src_capacity, esize, start, logstride, size, m);
    if (!work) return SHMEMX_OK;
    const bool fused = collect_route_fused(esize, capacity);
    SignalAlltoallvArgs aa{};
    AlltoallvArgs &c = aa.c;
    if (P == 1) {
        // no peer: any device memory serves, no handshake
        if (!loopback_signal_args(1, &aa.sig) || !alltoall_state()) return set_error(SHMEMX_ENOMEM);
        aa.sig.timeout_ticks = signal_timeout_ticks();
        c.src[0] = heap::twin(source);
        c.tgt = heap::twin(target);
        if (!fixed) {
            c.cnt[0] = static_cast<const unsigned long long *>(heap::twin(counts));
            c.off[0] = static_cast<const unsigned long long *>(heap::twin(offsets));
        }
    } else {
        uint64_t soff = 0, toff = 0, coff = 0, ooff = 0;
        if (!heap::offset_of(heap::twin(source), sbytes, &soff) || !heap::offset_of(heap::twin(target), cbytes, &toff))
            return set_error(SHMEMX_ENOTSUP);
        if (!fixed && (!heap::offset_of(heap::twin(counts), tbytes, &coff) ||
                       !heap::offset_of(heap::twin(offsets), tbytes, &ooff)))
            return set_error(SHMEMX_ENOTSUP);
        if (int rc = map_members(&mb)) return rc;
        if (!alltoall_state()) return set_error(SHMEMX_ENOMEM);
        aa.sig = mb.sa;
        for (int i = 0; i < P; ++i) {
            c.src[i] = mb.hb[i] + soff;
            if (fixed) continue;
            // member i's pair for me: word m of its tables
            c.cnt[i] = reinterpret_cast<const unsigned long long *>(mb.hb[i] + coff) + m;
            c.off[i] = reinterpret_cast<const unsigned long long *>(mb.hb[i] + ooff) + m;
        }
        c.tgt = mb.hb[m] + toff;
    }
    hipStream_t s = stream_of(stream);
    aa.gsync = fence_records().gsync;
    c.P = P;
    c.m = m;
    c.esize = (unsigned int)esize;
    c.nelems = fixed ? nelems : 0;
    c.capacity = capacity;
    c.src_capacity = src_capacity;
    c.where = static_cast<unsigned long long *>(heap::twin(where_dev));
    c.plan = g_alltoall.plan;
    c.overflows = g_alltoall.overflows;
    // mirrored heap: the host's stores to the source and the tables go to HBM;
    // the target's capacity and where_dev are DEVICE_NEWER from here
    (void)heap::device_operand(source, sbytes);
    if (!fixed) {
        (void)heap::device_operand(counts, tbytes);
        (void)heap::device_operand(offsets, tbytes);
    }
    heap::DeviceWrite tw(target, cbytes, s);
    heap::DeviceWrite ww(where_dev, where_dev ? (size_t)(P + 1) * sizeof(unsigned long long) : 0, s);
    SHMX_HIP(launch_alltoallv(aa, fused, s));
    g_alltoall_stats[fixed ? kAlltoalls : kAlltoallvs] += 1;
    g_alltoall_stats[kAlltoallFused] += fused;
    return SHMEMX_OK;
}

// ------------------------------------------------------ reduce-scatter
// shmemx_reduce_scatter_stats: [calls, those that ran as one fused launch]
enum { kReduceScatters = 0, kReduceScattersFused, kNumReduceScatterStats };
unsigned long long g_reduce_scatter_stats[kNumReduceScatterStats];

// P * nelems * size * 16 must not wrap
bool reduce_scatter_size_ok(size_t sz, size_t nelems, int P) {
    return nelems <= SIZE_MAX / (sz * kMaxFoldInputs) / (size_t)P;
}

// The source's bytes against the two shot's limit: every member pulls what
// the two shot's fold phase pulls at that array size.
bool reduce_scatter_route_fused(size_t sz, size_t nelems, int P) {
    return (size_t)P * nelems * sz <= fused_twoshot_bytes();
}

// What an operand must be a multiple of: the element, or 8 bytes for the
// 16-byte types (two doubles; the x87 slot's 8-byte significand)
size_t elem_alignment(size_t sz) { return std::min<size_t>(sz, 8); }

// One call's launches.  Fused: one.  Unfused: the two launches of a barrier,
// the peers fold, the two launches of a barrier: five (signal_reduce's
// unfused one shot on the P block pointers).
hipError_t launch_reduce_scatter(int type, int op, const SignalFoldArgs &fa, bool fused, hipStream_t s) {
    if (fused) return launch_signal_reduce_scatter(type, op, fa, s);
    hipError_t e = launch_sys_fence(s, fa.sig.seen);   // every source is final; nobody still reads my target
    if (e == hipSuccess) e = launch_signal(fa.sig, s);
    if (e == hipSuccess) e = launch_fold_peers(type, op, fa.out, fa.ins, fa.nins, fa.n, s);
    if (e == hipSuccess) e = launch_sys_fence(s, fa.sig.seen);   // nobody reads my source any more
    if (e == hipSuccess) e = launch_signal(fa.sig, s);
    return e;
}

// Member m's launch arguments: block m of every member's source, set order.
template <class SrcOf>
SignalFoldArgs reduce_scatter_args(const SignalArgs &sa, void *tgt, int P, int m, size_t nelems, size_t sz,
                                   SrcOf src_of) {
    const void *ins[kMaxFoldInputs];
    for (int i = 0; i < P; ++i) ins[i] = static_cast<const char *>(src_of(i)) + (size_t)m * nelems * sz;
    SignalFoldArgs fa = fused_args(sa, tgt, ins, P, nelems);
    fa.lo = 0;
    fa.hi = nelems;
    return fa;
}

int reduce_scatter_on_stream(int type, int op, void *target, const void *source, size_t nelems, int start,
                             int logstride, int size, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!set_shape_ok(start, logstride, size) || !op_valid(type, op)) return set_error(SHMEMX_EINVAL);
    const size_t sz = type_size(type);
    if (!reduce_scatter_size_ok(sz, nelems, size)) return set_error(SHMEMX_EINVAL);
    const size_t tbytes = nelems * sz, sbytes = (size_t)size * tbytes;
    if (tbytes && (!target || !source)) return set_error(SHMEMX_EINVAL);
    // whole elements: the offsets are symmetric, so this is a shared fact
    if (tbytes && (!elem_aligned(target, elem_alignment(sz)) || !elem_aligned(source, elem_alignment(sz))))
        return set_error(SHMEMX_EINVAL);
    // no in-place form: symmetric offsets again
    if (tbytes && ranges_meet(target, tbytes, source, sbytes)) return set_error(SHMEMX_EINVAL);
    Members mb;
    if (int rc = enter(start, logstride, size, &mb)) return rc;
    const int P = size, m = mb.m;
    trace(LOG_REDUCTION, "stream-ordered reduce-scatter: %zu bytes mine, set (%d,%d,%d) member %d", tbytes, start,
          logstride, size, m);
    if (!op_on_device(type, op)) return set_error(SHMEMX_ENOTSUP);
    if (!tbytes) return SHMEMX_OK;
    if (P == 1) {
        // no kernel: the one member's source is its whole result
        hipStream_t s = stream_of(stream);
        const void *src = heap::device_operand(source, tbytes);
        heap::DeviceWrite tw(target, tbytes, s);
        SHMX_HIP(hipMemcpyAsync(tw.ptr(), src, tbytes, hipMemcpyDefault, s));
        g_reduce_scatter_stats[kReduceScatters] += 1;
        return SHMEMX_OK;
    }
    const bool fused = reduce_scatter_route_fused(sz, nelems, P);
    uint64_t soff = 0, toff = 0;
    if (!heap::offset_of(heap::twin(source), sbytes, &soff) || !heap::offset_of(heap::twin(target), tbytes, &toff))
        return set_error(SHMEMX_ENOTSUP);
    if (int rc = map_members(&mb)) return rc;
    hipStream_t s = stream_of(stream);
    // mirrored heap: the host's stores to the source go to HBM, the target is
    // DEVICE_NEWER from here
    (void)heap::device_operand(source, sbytes);
    heap::DeviceWrite tw(target, tbytes, s);
    const SignalFoldArgs fa =
        reduce_scatter_args(mb.sa, mb.hb[m] + toff, P, m, nelems, sz, [&](int i) { return mb.hb[i] + soff; });
    SHMX_HIP(launch_reduce_scatter(type, op, fa, fused, s));
    g_reduce_scatter_stats[kReduceScatters] += 1;
    g_reduce_scatter_stats[kReduceScattersFused] += fused;
    return SHMEMX_OK;
}

}  // namespace

}  // namespace shmx

using namespace shmx;

extern "C" {

int shmemx_reduce_scatter_on_stream(int type, int op, void *target, const void *source, size_t nelems,
                                    int PE_start, int logPE_stride, int PE_size, void *stream) {
    return reduce_scatter_on_stream(type, op, target, source, nelems, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_reduce_scatter_route(int type, size_t nelems, int P, int *fused) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    const size_t sz = type_size(type);
    if (!fused || !sz || P < 1 || P > kMaxFoldInputs || !reduce_scatter_size_ok(sz, nelems, P))
        return set_error(SHMEMX_EINVAL);
    *fused = nelems && P > 1 && reduce_scatter_route_fused(sz, nelems, P) ? 1 : 0;
    return SHMEMX_OK;
}

int shmemx_reduce_scatter_stats(unsigned long long *out, int nout, int reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const int k = std::max(0, std::min(nout, (int)kNumReduceScatterStats));
    for (int i = 0; out && i < k; ++i) out[i] = g_reduce_scatter_stats[i];
    if (reset)
        for (unsigned long long &v : g_reduce_scatter_stats) v = 0;
    return out ? k : 0;
}

int shmemx_reduce_scatter_loopback(int type, int op, int P, int m, void *tgt, const void *const *srcs,
                                   size_t nelems, int fused, unsigned int *signal_error_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!op_valid(type, op) || P < 1 || P > kMaxFoldInputs || m < 0 || m >= P) return set_error(SHMEMX_EINVAL);
    const size_t sz = type_size(type);
    if (!reduce_scatter_size_ok(sz, nelems, P)) return set_error(SHMEMX_EINVAL);
    if (!op_on_device(type, op)) return set_error(SHMEMX_ENOTSUP);
    if (nelems == 0) return SHMEMX_OK;
    if (!tgt || !srcs || !elem_aligned(tgt, elem_alignment(sz))) return set_error(SHMEMX_EINVAL);
    for (int i = 0; i < P; ++i)
        if (!srcs[i] || !elem_aligned(srcs[i], elem_alignment(sz)) ||
            ranges_meet(tgt, nelems * sz, srcs[i], (size_t)P * nelems * sz))
            return set_error(SHMEMX_EINVAL);
    const LocalDevice dev(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SignalArgs sa{};
    if (!loopback_signal_args(P, &sa)) return set_error(SHMEMX_ENOMEM);
    const SignalFoldArgs fa = reduce_scatter_args(sa, tgt, P, m, nelems, sz, [&](int i) { return srcs[i]; });
    hipError_t e = launch_reduce_scatter(type, op, fa, fused != 0, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipGetLastError();
    const unsigned int err = signal_error();
    if (signal_error_out) *signal_error_out = err;
    if (e != hipSuccess || err) return set_error(SHMEMX_EDEVICE);
    return SHMEMX_OK;
}

int shmemx_barrier_on_stream(int PE_start, int logPE_stride, int PE_size, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!set_shape_ok(PE_start, logPE_stride, PE_size)) return set_error(SHMEMX_EINVAL);
    Members mb;
    if (int rc = enter(PE_start, logPE_stride, PE_size, &mb)) return rc;
    trace(LOG_BARRIER, "stream-ordered: set (%d,%d,%d) member %d", PE_start, logPE_stride, PE_size, mb.m);
    if (PE_size == 1) return SHMEMX_OK;
    // mirrored heap: the host's stores to symmetric objects reach HBM, where
    // the peers' kernels read them after the barrier
    heap::flush_view();
    if (int rc = map_members(&mb)) return rc;
    device_barrier(mb.sa, stream_of(stream));
    g_stats[kBarriers] += 1;
    return SHMEMX_OK;
}

int shmemx_broadcast32_on_stream(void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                                 int logPE_stride, int PE_size, void *stream) {
    return broadcast_on_stream(4, target, source, nelems, PE_root, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_broadcast64_on_stream(void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                                 int logPE_stride, int PE_size, void *stream) {
    return broadcast_on_stream(8, target, source, nelems, PE_root, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_fcollect32_on_stream(void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                                int PE_size, void *stream) {
    return fcollect_on_stream(4, target, source, nelems, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_fcollect64_on_stream(void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                                int PE_size, void *stream) {
    return fcollect_on_stream(8, target, source, nelems, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_collect32_on_stream(void *target, const void *source, size_t nelems, size_t capacity, int PE_start,
                               int logPE_stride, int PE_size, void *stream) {
    return collect_on_stream(4, target, source, nelems, nullptr, nullptr, false, capacity, PE_start, logPE_stride,
                             PE_size, stream);
}

int shmemx_collect64_on_stream(void *target, const void *source, size_t nelems, size_t capacity, int PE_start,
                               int logPE_stride, int PE_size, void *stream) {
    return collect_on_stream(8, target, source, nelems, nullptr, nullptr, false, capacity, PE_start, logPE_stride,
                             PE_size, stream);
}

int shmemx_collect32_counted_on_stream(void *target, const void *source, const unsigned long long *nelems_dev,
                                       unsigned long long *where_dev, size_t capacity, int PE_start,
                                       int logPE_stride, int PE_size, void *stream) {
    return collect_on_stream(4, target, source, 0, nelems_dev, where_dev, true, capacity, PE_start, logPE_stride,
                             PE_size, stream);
}

int shmemx_collect64_counted_on_stream(void *target, const void *source, const unsigned long long *nelems_dev,
                                       unsigned long long *where_dev, size_t capacity, int PE_start,
                                       int logPE_stride, int PE_size, void *stream) {
    return collect_on_stream(8, target, source, 0, nelems_dev, where_dev, true, capacity, PE_start, logPE_stride,
                             PE_size, stream);
}

int shmemx_collect_stats(unsigned long long *out, int nout, int reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    volatile unsigned long long *over = g_collect.overflows;   // none before the first launch
    const unsigned long long all[3] = {g_collect_stats[kCollects], g_collect_stats[kCollectsFused], over ? *over : 0};
    const int k = std::max(0, std::min(nout, 3));
    for (int i = 0; out && i < k; ++i) out[i] = all[i];
    if (reset) {
        for (unsigned long long &v : g_collect_stats) v = 0;
        if (over) *over = 0;
    }
    return out ? k : 0;
}

int shmemx_collect_route(size_t esize, size_t capacity, int P, int *fused) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!fused || (esize != 4 && esize != 8) || P < 1 || P > kMaxFoldInputs || !size_ok(esize, capacity))
        return set_error(SHMEMX_EINVAL);
    *fused = capacity && collect_route_fused(esize, capacity) ? 1 : 0;
    return SHMEMX_OK;
}

int shmemx_collect_loopback(int P, int m, size_t esize, void *tgt, const void *const *srcs,
                            const unsigned long long *counts, size_t capacity, int fused, int counted,
                            unsigned long long *where_out, unsigned int *overflow_out,
                            unsigned int *signal_error_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (P < 1 || P > kMaxFoldInputs || m < 0 || m >= P || (esize != 4 && esize != 8) || !size_ok(esize, capacity) ||
        !counts)
        return set_error(SHMEMX_EINVAL);
    if (capacity == 0) return SHMEMX_OK;
    if (!tgt || !srcs || !elem_aligned(tgt, esize)) return set_error(SHMEMX_EINVAL);
    for (int i = 0; i < P; ++i)
        if (!srcs[i] || !elem_aligned(srcs[i], esize)) return set_error(SHMEMX_EINVAL);
    if (ranges_meet(tgt, capacity * esize, srcs[m], 1)) return set_error(SHMEMX_EINVAL);
    const LocalDevice dev(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SignalCollectArgs ca{};
    if (!loopback_signal_args(P, &ca.sig) || !collect_state()) return set_error(SHMEMX_ENOMEM);
    ca.gsync = fence_records().gsync;
    CollectArgs &c = ca.c;
    c.P = P;
    c.m = m;
    c.esize = (unsigned int)esize;
    c.capacity = capacity;
    c.src_room = source_room(static_cast<const char *>(srcs[m]), static_cast<const char *>(tgt), esize,
                             kCollectPoison >> 1);
    c.count = counted ? 0 : counts[m];
    c.count_dev = counted ? g_collect.count : nullptr;
    c.my_word = g_collect.words + m;
    for (int i = 0; i < P; ++i) {
        c.word[i] = g_collect.words + i;
        c.src[i] = srcs[i];
    }
    c.tgt = tgt;
    c.plan = g_collect.plan;
    c.where = where_out ? g_collect.where : nullptr;
    c.overflows = g_collect.overflows;
    // the peers' words as they would have published them; entry m is the
    // kernel's to write, and holds something no test passes until it has
    unsigned long long words[kMaxFoldInputs] = {}, stale[2] = {0x5157414c45ull, 0x5157414c45ull};
    for (int i = 0; i < P; ++i) words[i] = i == m ? 0x5354414c45ull : counts[i];
    volatile unsigned long long *over = g_collect.overflows;
    const unsigned long long over0 = *over;
    hipError_t e = hipMemcpyAsync(g_collect.words, words, sizeof words, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g_collect.count, counts + m, sizeof counts[m], hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g_collect.where, stale, sizeof stale, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        if (fused) {
            e = launch_signal_collect(ca, s);
        } else {
            e = launch_collect_publish(c, s);
            if (e == hipSuccess) e = launch_sys_fence(s, ca.sig.seen);
            if (e == hipSuccess) e = launch_signal(ca.sig, s);
            if (e == hipSuccess) e = launch_collect_plan(c, s);
            if (e == hipSuccess) e = launch_collect_copy(c, s);
            if (e == hipSuccess) e = launch_sys_fence(s, ca.sig.seen);
            if (e == hipSuccess) e = launch_signal(ca.sig, s);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && where_out) e = hipMemcpy(where_out, g_collect.where, sizeof stale, hipMemcpyDeviceToHost);
    if (e != hipSuccess) (void)hipGetLastError();
    const unsigned int err = signal_error();
    if (signal_error_out) *signal_error_out = err;
    if (overflow_out) *overflow_out = (unsigned int)(*over - over0);
    if (e != hipSuccess || err) return set_error(SHMEMX_EDEVICE);
    return SHMEMX_OK;
}

int shmemx_alltoall32_on_stream(void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                                int PE_size, void *stream) {
    return alltoallv_on_stream(4, target, source, nullptr, nullptr, true, nelems, nullptr, 0, 0, PE_start,
                               logPE_stride, PE_size, stream);
}

int shmemx_alltoall64_on_stream(void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                                int PE_size, void *stream) {
    return alltoallv_on_stream(8, target, source, nullptr, nullptr, true, nelems, nullptr, 0, 0, PE_start,
                               logPE_stride, PE_size, stream);
}

int shmemx_alltoallv32_on_stream(void *target, const void *source, const unsigned long long *send_counts,
                                 const unsigned long long *send_offsets, unsigned long long *where_dev,
                                 size_t capacity, size_t src_capacity, int PE_start, int logPE_stride, int PE_size,
                                 void *stream) {
    return alltoallv_on_stream(4, target, source, send_counts, send_offsets, false, 0, where_dev, capacity,
                               src_capacity, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_alltoallv64_on_stream(void *target, const void *source, const unsigned long long *send_counts,
                                 const unsigned long long *send_offsets, unsigned long long *where_dev,
                                 size_t capacity, size_t src_capacity, int PE_start, int logPE_stride, int PE_size,
                                 void *stream) {
    return alltoallv_on_stream(8, target, source, send_counts, send_offsets, false, 0, where_dev, capacity,
                               src_capacity, PE_start, logPE_stride, PE_size, stream);
}

int shmemx_alltoall_stats(unsigned long long *out, int nout, int reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    volatile unsigned long long *over = g_alltoall.overflows;   // none before the first launch
    const unsigned long long all[4] = {g_alltoall_stats[kAlltoalls], g_alltoall_stats[kAlltoallvs],
                                       g_alltoall_stats[kAlltoallFused], over ? *over : 0};
    const int k = std::max(0, std::min(nout, 4));
    for (int i = 0; out && i < k; ++i) out[i] = all[i];
    if (reset) {
        for (unsigned long long &v : g_alltoall_stats) v = 0;
        if (over) *over = 0;
    }
    return out ? k : 0;
}

int shmemx_alltoallv_route(size_t esize, size_t capacity, int P, int *fused) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!fused || (esize != 4 && esize != 8) || P < 1 || P > kMaxFoldInputs || !size_ok(esize, capacity))
        return set_error(SHMEMX_EINVAL);
    *fused = capacity && collect_route_fused(esize, capacity) ? 1 : 0;
    return SHMEMX_OK;
}

int shmemx_alltoallv_loopback(int P, int m, size_t esize, void *tgt, const void *const *srcs,
                              const unsigned long long *counts, const unsigned long long *offsets, size_t capacity,
                              size_t src_capacity, int fused, unsigned long long *where_out,
                              unsigned int *overflow_out, unsigned int *signal_error_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (P < 1 || P > kMaxFoldInputs || m < 0 || m >= P || (esize != 4 && esize != 8) || !size_ok(esize, capacity))
        return set_error(SHMEMX_EINVAL);
    const bool fixed = !counts;
    if (fixed) {
        if (offsets || capacity % (size_t)P) return set_error(SHMEMX_EINVAL);
        src_capacity = capacity;
    } else if (!offsets || !size_ok(esize, src_capacity)) {
        return set_error(SHMEMX_EINVAL);
    }
    if (capacity == 0 || src_capacity == 0) return SHMEMX_OK;
    if (!tgt || !srcs || !elem_aligned(tgt, esize)) return set_error(SHMEMX_EINVAL);
    for (int i = 0; i < P; ++i)
        if (!srcs[i] || !elem_aligned(srcs[i], esize) ||
            ranges_meet(tgt, capacity * esize, srcs[i], src_capacity * esize))
            return set_error(SHMEMX_EINVAL);
    const LocalDevice dev(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SignalAlltoallvArgs aa{};
    if (!loopback_signal_args(P, &aa.sig) || !alltoall_state()) return set_error(SHMEMX_ENOMEM);
    aa.gsync = fence_records().gsync;
    AlltoallvArgs &c = aa.c;
    c.P = P;
    c.m = m;
    c.esize = (unsigned int)esize;
    c.nelems = fixed ? capacity / (size_t)P : 0;
    c.capacity = capacity;
    c.src_capacity = src_capacity;
    for (int i = 0; i < P; ++i) {
        c.src[i] = srcs[i];
        if (fixed) continue;
        c.cnt[i] = g_alltoall.counts + (size_t)i * P + m;   // row i is what member i sends
        c.off[i] = g_alltoall.offsets + (size_t)i * P + m;
    }
    c.tgt = tgt;
    c.plan = g_alltoall.plan;
    c.where = where_out ? g_alltoall.where : nullptr;
    c.overflows = g_alltoall.overflows;
    // where[] holds something no test passes until the kernel has written it
    unsigned long long stale[kMaxFoldInputs + 1];
    for (unsigned long long &v : stale) v = 0x5157414c45ull;
    const size_t wbytes = (size_t)(P + 1) * sizeof(unsigned long long);
    const size_t tbytes = (size_t)P * P * sizeof(unsigned long long);
    volatile unsigned long long *over = g_alltoall.overflows;
    const unsigned long long over0 = *over;
    hipError_t e = hipMemcpyAsync(g_alltoall.where, stale, wbytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !fixed) e = hipMemcpyAsync(g_alltoall.counts, counts, tbytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !fixed) e = hipMemcpyAsync(g_alltoall.offsets, offsets, tbytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = launch_alltoallv(aa, fused != 0, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && where_out) e = hipMemcpy(where_out, g_alltoall.where, wbytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) (void)hipGetLastError();
    const unsigned int err = signal_error();
    if (signal_error_out) *signal_error_out = err;
    if (overflow_out) *overflow_out = (unsigned int)(*over - over0);
    if (e != hipSuccess || err) return set_error(SHMEMX_EDEVICE);
    return SHMEMX_OK;
}

long shmemx_set_bcast_twophase_kb(long kb) {
    if (kb < 0) {
        set_error(SHMEMX_EINVAL);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const long prev = g_bcast_twophase_kb;
    g_bcast_twophase_kb = kb;
    return prev;
}

int shmemx_pull_stats(unsigned long long *out, int nout, int reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const int k = std::max(0, std::min(nout, (int)kNumStats));
    for (int i = 0; out && i < k; ++i) out[i] = g_stats[i];
    if (reset)
        for (unsigned long long &v : g_stats) v = 0;
    return out ? k : 0;
}

int shmemx_pull_plan(int kind, size_t esize, size_t nelems, int P, int m, int root, shmemx_pull_plan_t *plan) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!plan || (kind != kFcollect && kind != kBroadcast) || (esize != 4 && esize != 8) || P < 1 ||
        P > kMaxFoldInputs || m < 0 || m >= P || (kind == kBroadcast && (root < 0 || root >= P)) ||
        !size_ok(esize, nelems))
        return set_error(SHMEMX_EINVAL);
    *plan = shmemx_pull_plan_t{};
    const Route rt = route_of(kind, nelems * esize, P);
    plan->schedule = rt.schedule;
    if (!rt.schedule) return SHMEMX_OK;
    plan->fused = rt.fused ? 1 : 0;
    if (kind == kFcollect) {
        plan->nseg_a = P;
        return SHMEMX_OK;
    }
    if (m == root) return SHMEMX_OK;   // every handshake, no segment
    const BcastSlices bs(nelems, P, root, esize);
    if (rt.schedule == 1) {
        plan->nseg_a = 1;
        return SHMEMX_OK;
    }
    plan->lo = (long long)bs.lo(m);
    plan->hi = (long long)bs.hi(m);
    plan->nseg_a = bs.count(m) ? 1 : 0;
    for (int i = 0; i < P; ++i) plan->nseg_b += i != m && i != root && bs.count(i) ? 1 : 0;
    return SHMEMX_OK;
}

int shmemx_pull_loopback(int schedule, int P, int m, int root, size_t esize, void *const *tgts,
                         const void *const *srcs, size_t nelems, unsigned int *signal_error_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (schedule < 0 || schedule > 2 || P < 1 || P > kMaxFoldInputs || m < 0 || m >= P ||
        (schedule != 0 && (root < 0 || root >= P)) || (esize != 4 && esize != 8) || !size_ok(esize, nelems))
        return set_error(SHMEMX_EINVAL);
    if (nelems == 0) return SHMEMX_OK;
    if (!tgts || !srcs) return set_error(SHMEMX_EINVAL);
    for (int i = 0; i < P; ++i)
        if (!tgts[i] || !srcs[i]) return set_error(SHMEMX_EINVAL);
    const LocalDevice dev(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SignalArgs sa{};
    if (!loopback_signal_args(P, &sa)) return set_error(SHMEMX_ENOMEM);
    char *const tgt = static_cast<char *>(tgts[m]);
    SignalPullArgs pa = pull_args(sa, schedule == 2);
    if (schedule == 0) {
        pa.a.nseg = fcollect_segments(P, m, nelems * esize, [&](int i) { return static_cast<const char *>(srcs[i]); },
                                      tgt, pa.a.gsrc, pa.a.gdst, pa.a.glen);
    } else {
        const BcastSlices bs(nelems, P, root, esize);
        pa.a.nseg = bcast_from_root(bs, m, schedule == 2, static_cast<const char *>(srcs[root]), tgt, pa.a.gsrc,
                                    pa.a.gdst, pa.a.glen);
        if (schedule == 2)
            pa.b.nseg = bcast_from_peers(bs, m, [&](int i) { return static_cast<char *>(tgts[i]); }, tgt, pa.b.gsrc,
                                         pa.b.gdst, pa.b.glen);
    }
    hipError_t e = launch_signal_pull(pa, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipGetLastError();
    const unsigned int err = signal_error();
    if (signal_error_out) *signal_error_out = err;
    if (e != hipSuccess || err) return set_error(SHMEMX_EDEVICE);
    return SHMEMX_OK;
}

}  // extern "C"
