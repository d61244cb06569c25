// Internal interfaces between the C-ABI/runtime (runtime.cpp, entry.cpp) and
// the gfx950 kernels (fold_kernels.hip).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "span16.h"   // Span16, LaunchChoice

namespace shmx {

// Upper bound on inputs one fold launch reads; longer folds are chained
// (out = fold(ins[0..15]); out = fold(out, ins[16..30]); ...) which keeps the
// reference's left-to-right order.
constexpr int kMaxFoldInputs = 16;

// Element sizes per SHMEMX_TYPE_* (long double is the host's 16-byte x87
// slot; long and long long are both 8 bytes on LP64).
size_t type_size(int type);
bool op_valid(int type, int op);       // reference defines the pair
bool op_on_device(int type, int op);   // this build has a HIP kernel for it

// out[i] = op(...op(ins[0][i], ins[1][i])..., ins[nins-1][i]) for i < n.
// nins in [1, kMaxFoldInputs]; nins == 1 is a copy.  out may be the very
// same array as any input (each element is read by the lane that writes it,
// before it writes it) but must not partially overlap one.  Returns
// hipSuccess or the launch error.
hipError_t launch_fold(int type, int op, void *out, const void *const *ins,
                       int nins, size_t n, hipStream_t stream);

// A host-visible completion signal: a page-locked, host-coherent word and
// the value a launch stores there (system-scope release) once its work is
// done.  A blocking call spins on the word instead of waiting for the stream:
// 6.8 against 11.9 us for a one-element copy when the kernel stores it
// itself, 9.6 with a one-thread marker kernel after it
// (tools/latency_breakdown.hip, profiles/r03_latency_breakdown.txt).
struct HostSignal {
    unsigned long long *word;
    unsigned long long value;
};
// The next signal value (the word is shared: blocking calls hold the
// library lock), and the wait for it: spin until the word holds the value or
// the stream has drained; after ~2 ms of spinning (long work) or an error
// the stream wait takes over (and reports the error).
HostSignal next_host_signal();
void wait_host_signal(const HostSignal &sig, hipStream_t s);
// launch_fold whose completion stores sig: the fold kernel itself when the
// launch is one workgroup (every wave drains its stores, then lane 0 of the
// workgroup stores the value with a system-scope release), otherwise a
// one-thread marker kernel right after it.
hipError_t launch_fold_signal(int type, int op, void *out, const void *const *ins, int nins, size_t n,
                              hipStream_t stream, const HostSignal &sig);
// Does a copy (launch_fold with nins == 1) of n elements of `type` from
// src to dst run as ONE workgroup (so launch_fold_signal's workgroup stores
// the signal itself, after its own stores drained and a system-scope
// release)?
bool copy_one_workgroup(int type, const void *dst, const void *src, size_t n);
// A copy (launch_fold with nins == 1) of n elements of `type` from `in` to
// both `out` and `out2` in one launch, then sig as launch_fold_signal stores
// it (a small blocking result into HBM and into the mirrored heap's view).
hipError_t launch_copy2_signal(int type, void *out, void *out2, const void *in, size_t n, hipStream_t stream,
                               const HostSignal &sig);
// The one-thread marker kernel alone: stores sig once everything enqueued
// before it on the stream has completed.
hipError_t launch_host_signal(const HostSignal &sig, hipStream_t stream);

// launch_fold for inputs in other GPUs' HBM (DIRECT and SIGNAL): every lane
// issues its loads of all inputs before folding any, so every peer's link is
// busy at once; same results as launch_fold.
hipError_t launch_fold_peers(int type, int op, void *out, const void *const *ins, int nins, size_t n,
                             hipStream_t stream);

// The P-order fold: outs[k] = ins[k] folded with the other inputs ascending,
// for every k in one pass (each member's own reference order; float, double
// and long double min / max only).  outs[k] may be ins[k]; no other overlap.
hipError_t launch_fold_orders(int type, int op, void *const *outs, const void *const *ins, int nins, size_t n,
                              hipStream_t stream);

// What one of the three launches above would launch (shmemx_fold_launch_shape):
// route 0 launch_fold, 1 launch_fold_peers, 2 launch_fold_orders; outs is
// the one output, or the P-order fold's nins outputs.  The same checks,
// 16-byte split and choice (span16.h LaunchChoice) as the launch itself, from
// the addresses mod 16 alone: no HIP call, nothing dereferenced.  False where
// the launch would refuse the arguments; launches == false (and all else
// zero) where it would have nothing to do (n == 0).
enum FoldRoute { kRoutePlain = 0, kRoutePeers = 1, kRouteOrders = 2 };
struct FoldLaunchShape {
    bool launches;
    LaunchChoice choice;
    Span16 span;
    size_t scalar_trips;    // trips of the grid-stride loop over head + tail
    bool ld80_pipelined;    // fold_body's long double branch for nins >= 3
};
bool fold_launch_shape(int type, int op, int route, void *const *outs, const void *const *ins, int nins, size_t n,
                       FoldLaunchShape *shape);

// Copy nseg (<= kMaxFoldInputs) byte ranges srcs[i] -> dsts[i] in one launch
// (DIRECT all-gather: the peers' result slices, read concurrently).
hipError_t launch_gather(const void *const *srcs, void *const *dsts, const size_t *bytes, int nseg,
                         hipStream_t stream);

// System-scope release + acquire on every XCD's L2 (buffer_wbl2 sc0 sc1 +
// buffer_inv sc0 sc1 from blocks spread over all 8 XCDs), stream-ordered:
// this GPU's writes become visible to peers reading its HBM over xGMI, and
// no line of a peer's memory cached here survives into the next kernel.
// Enqueued before every host barrier that hands data between GPUs.
// Each of the kFenceBlocks blocks stores kFenceSeen | (its XCC id) into
// seen[block] (system scope), so the reader can prove every XCD fenced:
// fence_and_wait (host, seen host-coherent) or the next signal_kernel (seen
// in device memory; it also clears the records).
constexpr int kFenceBlocks = 64;
constexpr unsigned int kFenceSeen = 0x100u;
hipError_t launch_sys_fence(hipStream_t stream, unsigned int *seen);

// Device-side barrier of the SIGNAL algorithm (signal.cpp): the reference's
// linear barrier (barrier-linear.c:51-77: every member bumps a counter of
// every other member, then waits for its own to reach PE_size - 1) as one
// 64-lane wave, with the counters kept where only their owner writes them.
// cnt[q] in a PE's signal area = barriers that PE has entered together with
// PE q.  Lane i (member i != me) bumps mine[pe[i]] with a system-scope store,
// then polls peer[i][me] (member i's counter for me, read over xGMI) until it
// has caught up.  Counter state lives on the device, so a captured graph
// replays correctly.  A wait longer than timeout_ticks (s_memrealtime, 100
// MHz) sets *err and gives up, so a missing peer never hangs the GPU.
// Enqueue launch_sys_fence first: it publishes this GPU's writes and drops
// stale peer lines on every XCD, which a single wave cannot do.
struct SignalArgs {
    unsigned long long *mine;
    const unsigned long long *peer[kMaxFoldInputs];
    int pe[kMaxFoldInputs];
    int P, me;
    unsigned long long timeout_ticks;
    unsigned int *err;   // host-mapped: 1 = a peer timed out, 2 = a fence missed an XCD
    // the preceding launch_sys_fence's records (device memory, kFenceBlocks
    // words): fewer than nxcc distinct XCDs sets *err = 2.  fence_stats[0] +=
    // 1 per check, fence_stats[1] += 1 per incomplete fence (device memory).
    unsigned int *seen;
    int nxcc;
    unsigned long long *fence_stats;
};
hipError_t launch_signal(const SignalArgs &a, hipStream_t stream);

// The one-shot reduction of a small array as ONE launch (SIGNAL's one shot,
// and DIRECT's when every member can take it): kFenceBlocks blocks each run
// the system fence and record their XCD; the last block to arrive checks
// the XCD coverage and does the entry handshake with the peers (the signal
// counters of SignalArgs); every block then folds its share of
// out[i] = op(...op(ins[0][i], ins[1][i])..., ins[nins-1][i]); the last block
// to finish does the exit handshake.  gsync: 2 words of device memory, zero
// at the first launch and left zero (an arrival counter, a generation).
// sig.seen must hold kFenceBlocks words.  Launches on one GPU must not
// overlap (stream order, or one stream).
//
// Two-shot (two_shot != 0: SIGNAL's and DIRECT's two-shot schedule for
// mid-size arrays, as ONE launch): after the entry handshake every block
// folds its share of elements [lo, hi) only (out, ins indexed alike), then
// every block writes back its XCD's L2 and arrives; the last block does the
// mid handshake with the peers (every member's slice is final) and releases
// the grid; every block drops stale peer lines (system acquire) and copies
// the nseg byte ranges gsrc[k] -> gdst[k] (the peers' result slices); the
// last block to finish does the exit handshake.
// The fused one shot folds an array of at most this many elements (4 per
// lane of one 256-lane workgroup) in the last workgroup to arrive alone.
constexpr size_t kFusedTinyElems = 4 * 256;
struct SignalFoldArgs {
    SignalArgs sig;
    // the one shot's tiny case (one workgroup does all the work): stores
    // host_value into host_word after its exit handshake (nullptr: no store)
    unsigned long long *host_word;
    unsigned long long host_value;
    unsigned int *gsync;
    void *out;
    const void *ins[kMaxFoldInputs];
    int nins;
    size_t n;
    int two_shot;
    size_t lo, hi;
    int nseg;
    const void *gsrc[kMaxFoldInputs];
    void *gdst[kMaxFoldInputs];
    size_t glen[kMaxFoldInputs];   // bytes
};
hipError_t launch_signal_fold(int type, int op, const SignalFoldArgs &a, hipStream_t stream);

// SIGNAL's own slice as ONE launch (signal.cpp; the six own-order pairs only):
// the fused two shot above with the P-order fold in place of the slice fold.
// After the entry handshake every block folds its share of elements [lo, hi)
// of the f.nins sources f.ins[k] (set order, indexed as the array) in every
// member's order at once: order k's result of element lo + i goes to
// outs[k][i] (outs[me]: slice me of this member's target; the others: its
// result slots).  outs[k] may be exactly f.ins[k] + lo (in place); no other
// overlap.  Mid handshake (every owner's slots are final), then the nseg byte
// ranges f.gsrc[k] -> f.gdst[k] (this member's slot in every other owner's
// area, gather_order_slots), exit handshake.  f.out is this member's target
// (checked, not written through); f.two_shot, f.host_word are ignored.  Its
// own struct, so the kernarg layout of the launches above does not move.
struct SignalOrdersArgs {
    SignalFoldArgs f;
    void *outs[kMaxFoldInputs];
};
hipError_t launch_signal_orders(int type, int op, const SignalOrdersArgs &a, hipStream_t stream);

// The stream-ordered broadcast and fcollect as ONE launch (pull.cpp): the
// fused two shot above with nothing to fold.  After the entry handshake every
// block copies its share of list a's byte ranges gsrc[k] -> gdst[k]; with
// two_phase != 0 (or a non-empty list b) the mid handshake and list b follow;
// then the exit handshake.  Every member of a set must pass the same
// two_phase: the handshakes run whatever the lists hold, empty ones too (a
// broadcast's root).  A list is copied in 16-byte vectors when every
// segment's source and target are 16-byte aligned, else byte by byte.
// gsync, sig as for launch_signal_fold.  Its own struct, so the kernarg
// layout of the launches above does not move.
struct SegList {
    int nseg;
    const void *gsrc[kMaxFoldInputs];
    void *gdst[kMaxFoldInputs];
    size_t glen[kMaxFoldInputs];   // bytes
};
struct SignalPullArgs {
    SignalArgs sig;
    unsigned int *gsync;
    int two_phase;
    SegList a, b;
};
hipError_t launch_signal_pull(const SignalPullArgs &a, hipStream_t stream);

// The stream-ordered reduce-scatter as ONE launch (pull.cpp): the fused two
// shot above without its second phase.  After the entry handshake every block
// folds its share of out[i] = op(...op(ins[0][i], ins[1][i])..., ins[nins-1][i])
// for i < n, where ins[k] is member k's source at this member's block (set
// order) and out this member's target; then the exit handshake.  No mid
// handshake, no gather, no tiny path.  lo must be 0 and hi n; two_shot,
// host_word and the segment list are ignored.  16-byte vectors when out and
// every ins[k] are 16-byte aligned, else the element loop.  gsync, sig as for
// launch_signal_fold, whose struct it takes as it stands.
hipError_t launch_signal_reduce_scatter(int type, int op, const SignalFoldArgs &a, hipStream_t stream);

// The stream-ordered collect (pull.cpp): the members' counts are exchanged on
// the device.  Member m publishes its count (`count`, or *count_dev read by
// the call's first kernel; kCollectPoison if it is above `capacity` or
// `src_room`, both in elements) in my_word; after the entry barrier one
// thread reads all P words word[i] (word[m] is my_word), runs collect_plan
// (set_geom.h) and leaves the plan in `plan` (kCollectPlanWords words of
// device memory), member m's offset and the total in where[0..2) (all ones
// on overflow; where may be null) and, on overflow, one more in *overflows
// (host-mapped; this GPU's launches are its only writer).  Every workgroup
// then copies its share of the non-empty segments src[i] -> tgt +
// offset[i] * esize, or nothing on overflow.  esize is 4 or 8 and every
// pointer a whole number of elements.
struct CollectArgs {
    int P, m;
    unsigned int esize;
    unsigned long long count;
    const unsigned long long *count_dev;   // null: `count`
    unsigned long long capacity, src_room;
    unsigned long long *my_word;
    const unsigned long long *word[kMaxFoldInputs];
    const void *src[kMaxFoldInputs];
    void *tgt;
    unsigned long long *plan;
    unsigned long long *where;
    unsigned long long *overflows;
};
// As ONE launch: publish, the fused launches' entry (the last workgroup's
// first lane reads the words and plans before it releases the grid), copy,
// exit.  gsync, sig as for launch_signal_fold.
struct SignalCollectArgs {
    SignalArgs sig;
    unsigned int *gsync;
    CollectArgs c;
};
hipError_t launch_signal_collect(const SignalCollectArgs &a, hipStream_t stream);
// The same between the unfused barriers: publish (one wave) before the first
// barrier; plan (one wave) and copy (a sixteenth of the grid copy_blocks
// gives `capacity` elements, a lane holding 16 units of a step, so every
// member launches the same shape) after it.
hipError_t launch_collect_publish(const CollectArgs &c, hipStream_t stream);
hipError_t launch_collect_plan(const CollectArgs &c, hipStream_t stream);
hipError_t launch_collect_copy(const CollectArgs &c, hipStream_t stream);

// The stream-ordered alltoall and alltoallv (pull.cpp): the personalised
// exchange.  Receiver m reads, after the entry barrier, the pair (*cnt[i],
// *off[i]) from every member i: member i's send_counts[m] and send_offsets[m],
// words of i's heap; one thread issues all 2 P system-scope loads before it
// uses the first, runs alltoallv_plan (set_geom.h) and leaves the plan in
// `plan` (kAlltoallvPlanWords words of device memory), the P block offsets and
// the total in where[0..P] (all ones on overflow; where may be null) and, on
// overflow, one more in *overflows (host-mapped; this GPU's launches are its
// only writer).  Every workgroup then copies its share of the non-empty
// blocks src[i] + from[i] * esize -> tgt + offset[i] * esize, or nothing on
// overflow.  cnt[0] == nullptr means immediates and no remote loads (the fixed
// alltoall): every count `nelems`, every offset m * nelems.  esize is 4 or 8
// and every pointer a whole number of elements.
struct AlltoallvArgs {
    int P, m;
    unsigned int esize;
    unsigned long long nelems;   // immediates only
    unsigned long long capacity, src_capacity;
    const unsigned long long *cnt[kMaxFoldInputs];
    const unsigned long long *off[kMaxFoldInputs];
    const void *src[kMaxFoldInputs];
    void *tgt;
    unsigned long long *plan;
    unsigned long long *where;
    unsigned long long *overflows;
};
// As ONE launch: the fused launches' entry (the last workgroup's first lane
// reads the pairs and plans before it releases the grid), copy, exit.
struct SignalAlltoallvArgs {
    SignalArgs sig;
    unsigned int *gsync;
    AlltoallvArgs c;
};
hipError_t launch_signal_alltoallv(const SignalAlltoallvArgs &a, hipStream_t stream);
// The same between the unfused barriers: plan (one wave) and copy (the
// collect's grid for `capacity` elements, so every member launches the same
// shape).
hipError_t launch_alltoallv_plan(const AlltoallvArgs &c, hipStream_t stream);
hipError_t launch_alltoallv_copy(const AlltoallvArgs &c, hipStream_t stream);

// Position-aware 64-bit checksum of n elements of `type` at device address
// ptr (16-byte aligned) into out[0], then `epoch` into out[1] (device memory
// or host-mapped page-locked memory: system-scope stores, in that order),
// stream-ordered, one launch.  Calls must not overlap in time (one arrival
// counter per process).
constexpr int kChecksumMaxBlocks = 4096;
hipError_t launch_checksum(int type, const void *ptr, size_t n, unsigned long long *out,
                           unsigned long long epoch, hipStream_t stream);

// The kernel clock (fold_kernels.hip; shmemx_kernel_timing /
// shmemx_kernel_times): while on, every fold-family launch carries a
// start / stop event pair of its own dispatch (hipExtLaunchKernelGGL), up to
// 4096 launches between reads.  kernel_times waits for them and returns
// their durations (us) and kinds (0 fold, 1 copy, 2 peers fold, 3 gather,
// 4 P-order fold) in launch order, then starts over.
int kernel_timing(int on);
int kernel_times(double *us, int *kind, int max, unsigned long long *dropped);


}  // namespace shmx
