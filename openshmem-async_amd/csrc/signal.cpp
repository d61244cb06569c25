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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
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
    sa.mine = loopback_signal_area();
    if (!sa.mine) return set_error(SHMEMX_ENOMEM);
    sa.P = P;
    sa.me = 0;
    for (int i = 0; i < P; ++i) {
        sa.pe[i] = i;
        sa.peer[i] = sa.mine + i;
    }
    // a bound, not a tuned number: a broken barrier ends the kernel in
    // seconds (2 s of the 100 MHz clock), not at $SHMEMX_SIGNAL_TIMEOUT
    sa.timeout_ticks = 200000000ull;
    sa.err = signal_error_word();
    const FenceRecords fr = fence_records();
    sa.seen = fr.seen;
    sa.nxcc = fr.nxcc;
    sa.fence_stats = fr.stats;
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
