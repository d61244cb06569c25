// SIGNAL algorithm: DIRECT's pulls (direct.cpp) with the barriers moved onto
// the GPU, so a reduction is pure stream work — no host wait, no host
// barrier, capturable into a hipGraph.
//
// The reference synchronises its reduction with two linear barriers
// (reduce-op.c:217,250; barrier-linear.c:51-77: remote increments of pSync
// counters, then a wait until the local counter has heard from every peer).
// Here each barrier is two stream-ordered launches:
//   launch_sys_fence  every XCD writes back its L2 and drops stale peer lines
//                     (this GPU's results become visible over xGMI); each
//                     block records its XCD;
//   launch_signal     one wave checks that the fence reached every XCD (else
//                     the call fails loudly: error word 2), then bumps this PE's per-peer counters in its own
//                     signal area (system-scope stores) and polls the peers'
//                     counters for it over xGMI (system-scope loads);
// the counters live at the top of every PE's heap segment
// (heap::signal_area), at the same offset on every PE.
//
// Operands must be symmetric — both in the heap, which is what OpenSHMEM
// requires of source and target — so every member computes every peer's
// address from its own offsets, with no descriptor exchange.  A member whose
// operands are not in the heap returns ENOTSUP; its peers' device barriers
// then time out ($SHMEMX_SIGNAL_TIMEOUT seconds, default 20) and the next
// blocking call reports it.
//
// Two-shot (set order, PE_start bits on every member, as DIRECT):
//   barrier                 every source is final; nobody reads my target
//   fold                    slice m of all P sources -> my target's slice m
//   barrier                 every slice is final
//   gather                  the other P-1 slices from the peers' targets
//   barrier                 nobody reads my source or target any more
// — as ONE fused launch up to $SHMEMX_FUSED_TWOSHOT_KB (default 4 MiB):
// launch_signal_fold with two_shot, three handshakes and two grid barriers
// inside one 64-block kernel, instead of seven launches.
// One shot (arrays up to $SHMEMX_DIRECT_ONESHOT_KB, target != source):
//   barrier; fold all of every source -> my target; barrier — as ONE fused
//   launch (launch_signal_fold: the fence, both handshakes and the fold in
//   one kernel, with a self-resetting grid barrier).
// Own order (float / double / long double min and max, own_order_pair): the
//   one shot at every size, each member folding src_me first, then the other
//   members ascending (reduce-op.c:219-248); in place, into the private
//   temporary, copied over the target after the second barrier.
// Own slice ($SHMEMX_SIGNAL_OWNSLICE=1 / shmemx_set_signal_ownslice, default
//   off; the same six pairs above the one-shot limit): OWNSLICE's schedule
//   (direct.cpp) under these device barriers, so own order at the two shot's
//   traffic is stream-ordered and capturable too:
//   barrier                 every source is final; nobody reads my slots
//   fold in all P orders    slice m of all P sources: my order -> my target's
//                           slice m, the others -> my result slots
//   barrier                 every owner's slots are final
//   gather                  my slot from every other owner -> my target
//   barrier                 nobody reads my source or my slots any more
//   — as ONE fused launch per chunk up to $SHMEMX_FUSED_TWOSHOT_KB
//   (launch_signal_orders), five launches above it.  The slots are the
//   second half of every PE's IPC scratch region, whose size is a plan
//   setting, so every member computes every owner's slot addresses itself; a
//   call whose slots do not fit is cut into chunks, each a whole schedule.
//   Only its owner writes a target, a slice at a time after the phase that
//   read it: exact in place needs no temporary, and nothing on this route is
//   refused on one member alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "heap.h"
#include "internal.h"
#include "node.h"
#include "set_geom.h"
#include "shmem_reduce_mi355x.h"
#include "state.h"

namespace shmx {

unsigned long long signal_timeout_ticks() {   // s_memrealtime runs at 100 MHz
    static const unsigned long long t = [] {
        const char *e = std::getenv("SHMEMX_SIGNAL_TIMEOUT");
        const double s = e ? std::atof(e) : 0.0;
        return (unsigned long long)((s > 0 ? s : 20.0) * 1e8);
    }();
    return t;
}

// Host-mapped error word the signal kernels set on a timeout.
unsigned int *signal_error_word() {
    static unsigned int *w = [] {
        void *p = nullptr;
        SHMX_HIP(hipHostMalloc(&p, sizeof(unsigned int), hipHostMallocCoherent));
        *static_cast<volatile unsigned int *>(p) = 0;
        return static_cast<unsigned int *>(p);
    }();
    return w;
}

unsigned int signal_error() {
    volatile unsigned int *w = signal_error_word();
    const unsigned int e = *w;
    *w = 0;
    return e;
}

void check_signal_error(const char *what) {
    switch (signal_error()) {
    case 0: break;
    case 2: fatal(what, "a system fence before a device barrier missed an XCD");
    default: fatal(what, "a member never reached the device barrier");
    }
}

SignalFoldArgs fused_args(const SignalArgs &sa, void *out, const void *const *ins, int P, size_t n) {
    SignalFoldArgs fa{};
    fa.sig = sa;
    fa.gsync = fence_records().gsync;
    fa.out = out;
    for (int i = 0; i < P; ++i) fa.ins[i] = ins[i];
    fa.nins = P;
    fa.n = n;
    return fa;
}

namespace {

long signal_ownslice_from_env() {
    const char *e = std::getenv("SHMEMX_SIGNAL_OWNSLICE");
    return e && std::atol(e) > 0 ? 1 : 0;
}
long g_signal_ownslice = signal_ownslice_from_env();

// the sets that have met the own-slice route (their scratch regions published,
// mapped and voted on), with the generation of this PE's scratch at the time:
// after a finalize and a new init every PE publishes again
std::set<std::tuple<int, int, int, uint64_t>> g_ownslice_met;

// The peers' scratch regions for the own-slice route.  The first time a set
// meets it every member allocates and publishes its scratch, the members
// pass one host barrier (so nobody looks for a region before its owner has
// published it), and only then map and vote: an allocation or a mapping that
// failed on one member fails the call on all of them alike.  Later calls are
// plain lookups.  (Under capture the warm call has done this.)
bool map_slot_areas(const ActiveSet &set, size_t *half) {
    size_t bytes = 0;
    const bool have = ipc_scratch(&bytes) != nullptr;
    const auto key = std::make_tuple(set.start, set.step, set.size, node::region_gen(node::kScratch, g_state.pe));
    if (!g_ownslice_met.count(key)) node::barrier(set.start, set.step, set.size);
    std::vector<std::pair<node::Region, int>> regs;
    for (int i = 0; i < set.size; ++i) regs.emplace_back(node::kScratch, set.pe_of(i));
    if (!map_regions(regs, set, have)) return false;
    g_ownslice_met.insert(key);
    *half = bytes / 2;
    return true;
}

// SIGNAL's own slice (the header comment): member m of the set, operands at
// heap offsets soff / toff, hb the members' heap bases.
int signal_ownslice(int type, int op, char *tgt, size_t n, size_t sz, const ActiveSet &set, int m,
                    const SignalArgs &sa, const std::vector<char *> &hb, uint64_t soff, hipStream_t s) {
    const int P = set.size;
    size_t half = 0;
    if (!map_slot_areas(set, &half)) {
        trace(LOG_REDUCTION, "SIGNAL own slice: a member has no scratch region or could not map a peer's (%s)",
              node::last_ipc_error());
        return set_error(SHMEMX_ENOTSUP);
    }
    // every owner's slots start at the sources' offset mod 16, so the fold's
    // 2 P arrays share an alignment whenever the target does (as direct.cpp)
    const size_t skew = soff & 15u;
    auto slots_of = [&](int i) { return node::peer_base(node::kScratch, set.pe_of(i)) + half + skew; };
    const size_t C = std::min(std::max<size_t>(n, 1), order_chunk_elems(half, P, sz));
    const bool fused = C * sz <= fused_twoshot_bytes();
    auto barrier = [&] {
        SHMX_HIP(launch_sys_fence(s, sa.seen));
        SHMX_HIP(launch_signal(sa, s));
    };
    ws_acquire(s);   // the slots serve every stream, and DIRECT's OWNSLICE
    for (size_t c0 = 0; c0 < n; c0 += C) {
        const size_t cnt = std::min(C, n - c0);
        const Slices sl(cnt, P, sz);
        const size_t lo = sl.lo(m), hi = sl.hi(m);
        SignalOrdersArgs oa{};
        const void *ins[kMaxFoldInputs];
        for (int i = 0; i < P; ++i) {
            ins[i] = hb[i] + soff + c0 * sz;
            oa.outs[i] = i == m ? tgt + (c0 + lo) * sz : slots_of(m) + order_slot(sl, m, i);
        }
        oa.f = fused_args(sa, tgt, ins, P, cnt);
        oa.f.lo = lo;
        oa.f.hi = hi;
        oa.f.nseg = gather_order_slots(sl, m, slots_of, tgt + c0 * sz, oa.f.gsrc, oa.f.gdst, oa.f.glen);
        if (fused) {
            SHMX_HIP(launch_signal_orders(type, op, oa, s));   // reduce-op.c:217-250
            continue;
        }
        barrier();   // reduce-op.c:217
        if (hi > lo) {
            for (int i = 0; i < P; ++i) ins[i] = hb[i] + soff + (c0 + lo) * sz;
            SHMX_HIP(launch_fold_orders(type, op, oa.outs, ins, P, hi - lo, s));
        }
        barrier();   // every owner's slots are final
        SHMX_HIP(launch_gather(oa.f.gsrc, oa.f.gdst, oa.f.glen, oa.f.nseg, s));
        barrier();   // reduce-op.c:250
    }
    ws_release(s);
    count_signal_ownslice_call(fused);
    return SHMEMX_OK;
}

}  // namespace

bool signal_ownslice_enabled() { return g_signal_ownslice != 0; }

long set_signal_ownslice(long on) {
    const long prev = g_signal_ownslice;
    g_signal_ownslice = on ? 1 : 0;
    return prev;
}

int signal_reduce(int type, int op, char *tgt, const char *src, int nreduce, int start,
                  int logstride, const shmemx_plan_t &p, bool own_order, hipStream_t s) {
    const int P = p.nmembers, m = p.member;
    const ActiveSet set = ActiveSet::of(start, logstride, P);
    if (!node::up() || P > kMaxFoldInputs) return set_error(SHMEMX_ENOTSUP);
    const size_t sz = (size_t)p.elem_size;
    const size_t n = (size_t)nreduce;
    const size_t bytes = n * sz;
    uint64_t soff = 0, toff = 0;
    const bool partial = tgt != src && tgt < src + bytes && src < tgt + bytes;
    if (partial || !heap::offset_of(src, bytes, &soff) || !heap::offset_of(tgt, bytes, &toff))
        return set_error(SHMEMX_ENOTSUP);
    if (!heap::signal_area()) return set_error(SHMEMX_ENOTSUP);
    // The peers' heap segments: mapped (and voted on) the first time this set
    // meets them, plain lookups afterwards.
    std::vector<std::pair<node::Region, int>> regs;
    for (int i = 0; i < P; ++i) regs.emplace_back(node::kHeap, set.pe_of(i));
    if (!map_regions(regs, set)) {
        trace(LOG_REDUCTION, "SIGNAL: a member could not map a peer heap (%s)", node::last_ipc_error());
        return set_error(SHMEMX_ENOTSUP);
    }
    SignalArgs sa;
    if (!signal_args(set, &sa)) return set_error(SHMEMX_ENOTSUP);
    std::vector<char *> hb(P);
    for (int i = 0; i < P; ++i) hb[i] = node::peer_base(node::kHeap, set.pe_of(i));
    if (signal_ownslice_route(own_order && P > 1 && own_order_pair(type, op), bytes))
        return signal_ownslice(type, op, tgt, n, sz, set, m, sa, hb, soff, s);
    // every whole source, in set order, or in my own (src_me first, then
    // the other members ascending: reduce-op.c:219-248)
    const void *ins[kMaxFoldInputs];
    fold_inputs(ins, P, m, own_order, [&](int i) { return hb[i] + soff; });
    if (tgt != src && bytes <= oneshot_bytes() && fused_oneshot_enabled()) {
        // barrier, fold of every whole source, barrier: one fused launch
        SHMX_HIP(launch_signal_fold(type, op, fused_args(sa, tgt, ins, P, n), s));   // reduce-op.c:217-250
        count_fused_call();
        return SHMEMX_OK;
    }
    auto barrier = [&] {
        SHMX_HIP(launch_sys_fence(s, sa.seen));
        SHMX_HIP(launch_signal(sa, s));
    };
    if (tgt != src && (bytes <= oneshot_bytes() || own_order)) {   // the one shot, unfused
        barrier();   // reduce-op.c:217
        SHMX_HIP(launch_fold_peers(type, op, tgt, ins, P, n, s));
        barrier();   // reduce-op.c:250
        return SHMEMX_OK;
    }
    if (own_order) {
        // in place: the peers read my source (= my target) until the second
        // barrier, so the fold goes to the private temporary (the
        // reference's own temporary target, reduce-op.c:187-203, 251-259).
        // A captured call cannot allocate it: ENOTSUP before any barrier
        // (the peers' barriers then time out, as for any refused operand).
        if (stream_capturing(s) && g_state.tmp_bytes < bytes) return set_error(SHMEMX_ENOTSUP);
        void *t = grow(g_state.tmp, g_state.tmp_bytes, bytes);
        if (!t) return set_error(SHMEMX_ENOMEM);
        ws_acquire(s);
        barrier();   // reduce-op.c:217
        SHMX_HIP(launch_fold_peers(type, op, t, ins, P, n, s));
        barrier();   // reduce-op.c:250
        SHMX_HIP(hipMemcpyAsync(tgt, t, bytes, hipMemcpyDeviceToDevice, s));
        ws_release(s);
        return SHMEMX_OK;
    }
    const Slices sl(n, P, sz);
    auto tgt_of = [&](int i) { return hb[i] + toff; };
    if (bytes <= fused_twoshot_bytes()) {
        // barrier, slice fold, barrier, gather, barrier: one fused launch
        // (set order from here on: ins holds every source in it)
        SignalFoldArgs fa = fused_args(sa, tgt, ins, P, n);
        two_shot_args(&fa, sl, m, tgt_of, tgt);
        SHMX_HIP(launch_signal_fold(type, op, fa, s));   // reduce-op.c:217-250
        count_fused_twoshot_call();
        return SHMEMX_OK;
    }
    barrier();   // reduce-op.c:217
    if (sl.count(m) > 0) {
        for (int i = 0; i < P; ++i) ins[i] = hb[i] + soff + sl.lo(m) * sz;
        SHMX_HIP(launch_fold_peers(type, op, tgt + sl.lo(m) * sz, ins, P, sl.count(m), s));
    }
    barrier();   // every member's slice is final
    const void *from[kMaxFoldInputs];
    void *to[kMaxFoldInputs];
    size_t len[kMaxFoldInputs];
    // from member m + 1 on, wrapping
    const int nseg = gather_segments(sl, m, true, false, tgt_of, tgt, from, to, len);
    SHMX_HIP(launch_gather(from, to, len, nseg, s));
    barrier();   // reduce-op.c:250
    return SHMEMX_OK;
}

// The looped-back handshakes of the test hooks below (and pull.cpp's): PE 0 of
// PEs 0..P-1 over the private signal area, where peer[i] + me is the word
// mine + pe[i] the launch has just bumped.  False if the area cannot be had.
bool loopback_signal_args(int P, SignalArgs *sa) {
    *sa = SignalArgs{};
    sa->mine = loopback_signal_area();
    if (!sa->mine) return false;
    sa->P = P;
    sa->me = 0;
    for (int i = 0; i < P; ++i) {
        sa->pe[i] = i;
        sa->peer[i] = sa->mine + i;
    }
    // a bound, not a tuned number: a broken barrier ends the kernel in
    // seconds (2 s of the 100 MHz clock), not at $SHMEMX_SIGNAL_TIMEOUT
    sa->timeout_ticks = 200000000ull;
    sa->err = signal_error_word();
    const FenceRecords fr = fence_records();
    sa->seen = fr.seen;
    sa->nxcc = fr.nxcc;
    sa->fence_stats = fr.stats;
    return true;
}

}  // namespace shmx

using namespace shmx;

// Test hook: member m's launch of a P-member set whose members' arrays all
// belong to this process, with the peer handshakes looped back onto the
// launch's own counters (peer[i] + me is the word mine + pe[i] it has just
// bumped), so the grid barrier, the fences, the XCD-coverage check, the fold
// and the gather run for real on one GPU with no heap and no peers.
extern "C" int shmemx_fused_loopback(int type, int op, int schedule, int P, int m, int own_order,
                                     void *const *tgts, const void *const *srcs, size_t nelems,
                                     unsigned int *signal_error_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!op_valid(type, op) || schedule < 0 || schedule > 2 || P < 1 || P > kMaxFoldInputs || m < 0 ||
        m >= P || (own_order && schedule == 1))
        return set_error(SHMEMX_EINVAL);
    if (!op_on_device(type, op)) return set_error(SHMEMX_ENOTSUP);
    if (schedule != 2) {
        if (nelems == 0) return SHMEMX_OK;
        if (!tgts || !srcs) return set_error(SHMEMX_EINVAL);
        for (int i = 0; i < P; ++i)
            if (!tgts[i] || !srcs[i]) return set_error(SHMEMX_EINVAL);
    }
    const LocalDevice dev(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SignalArgs sa{};
    if (!loopback_signal_args(P, &sa)) return set_error(SHMEMX_ENOMEM);
    hipError_t e = hipSuccess;
    HostSignal sig{nullptr, 0};
    if (schedule == 2) {
        e = launch_sys_fence(s, sa.seen);
        if (e == hipSuccess) e = launch_signal(sa, s);
    } else {
        const void *ins[kMaxFoldInputs];
        fold_inputs(ins, P, m, own_order != 0, [&](int i) { return srcs[i]; });
        char *const tgt = static_cast<char *>(tgts[m]);
        SignalFoldArgs fa = fused_args(sa, tgt, ins, P, nelems);
        if (schedule == 1) {
            const Slices sl(nelems, P, type_size(type));
            two_shot_args(&fa, sl, m, [&](int i) { return static_cast<char *>(tgts[i]); }, tgt);
        } else if (nelems <= kFusedTinyElems) {
            // the tiny one shot tells the host itself, as under DIRECT
            sig = next_host_signal();
            fa.host_word = sig.word;
            fa.host_value = sig.value;
        }
        e = launch_signal_fold(type, op, fa, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipGetLastError();
    const unsigned int err = signal_error();
    if (signal_error_out) *signal_error_out = err;
    if (e != hipSuccess || err) return set_error(SHMEMX_EDEVICE);
    if (sig.word && *static_cast<volatile unsigned long long *>(sig.word) != sig.value)
        return set_error(SHMEMX_EDEVICE);
    return SHMEMX_OK;
}

// Test hook: member m's fused own-slice launch (launch_signal_orders, set up
// as signal_ownslice sets it up) of a P-member set whose members' sources,
// targets and slot areas all belong to this process; the handshakes looped
// back as above.
extern "C" int shmemx_fused_orders_loopback(int type, int op, int P, int m, void *const *tgts,
                                            const void *const *srcs, void *const *slots, size_t nelems,
                                            unsigned int *signal_error_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    if (!op_valid(type, op) || P < 1 || P > kMaxFoldInputs || m < 0 || m >= P) return set_error(SHMEMX_EINVAL);
    if (!own_order_pair(type, op)) return set_error(SHMEMX_ENOTSUP);
    if (nelems == 0) return SHMEMX_OK;
    if (!tgts || !srcs || !slots) return set_error(SHMEMX_EINVAL);
    for (int i = 0; i < P; ++i)
        if (!tgts[i] || !srcs[i] || (P > 1 && !slots[i])) return set_error(SHMEMX_EINVAL);
    const LocalDevice dev(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SignalArgs sa{};
    if (!loopback_signal_args(P, &sa)) return set_error(SHMEMX_ENOMEM);
    const size_t sz = type_size(type);
    const Slices sl(nelems, P, sz);
    char *const tgt = static_cast<char *>(tgts[m]);
    auto slots_of = [&](int i) { return static_cast<char *>(slots[i]); };
    SignalOrdersArgs oa{};
    oa.f = fused_args(sa, tgt, srcs, P, nelems);
    oa.f.lo = sl.lo(m);
    oa.f.hi = sl.hi(m);
    for (int i = 0; i < P; ++i)
        oa.outs[i] = i == m ? tgt + sl.lo(m) * sz : slots_of(m) + order_slot(sl, m, i);
    oa.f.nseg = gather_order_slots(sl, m, slots_of, tgt, oa.f.gsrc, oa.f.gdst, oa.f.glen);
    hipError_t e = launch_signal_orders(type, op, oa, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipGetLastError();
    const unsigned int err = signal_error();
    if (signal_error_out) *signal_error_out = err;
    if (e != hipSuccess || err) return set_error(SHMEMX_EDEVICE);
    return SHMEMX_OK;
}

// Host only: the bytes of one member's result slots for an array of nelems
// elements over P members (set_geom.h order_slots_bytes); 0 for an unknown
// type or P outside 1..16.
extern "C" size_t shmemx_order_slots_bytes(int type, int P, size_t nelems) {
    const size_t sz = type_size(type);
    if (!sz || P < 1 || P > kMaxFoldInputs) return 0;
    return order_slots_bytes(Slices(nelems, P, sz));
}

extern "C" long shmemx_set_signal_ownslice(long on) {
    if (on < 0) {
        set_error(SHMEMX_EINVAL);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return set_signal_ownslice(on);
}
