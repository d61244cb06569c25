// gfx950 kernels of the device-side synchronisation of the IPC algorithms
// (DIRECT, SIGNAL): the system-scope fence on every XCD with
// its XCD records, the SIGNAL barrier wave, and the fused one-shot and
// two-shot launches (fence, grid barriers, peer handshakes, fold and gather
// in one kernel), and the fused pull of the stream-ordered broadcast and
// fcollect (the same barriers around one or two gathers), and the
// stream-ordered collect (the members' counts exchanged under the entry
// barrier, fused and unfused), and the stream-ordered alltoall and alltoallv
// (the peers' count and offset tables read under the entry barrier).  The
// element ops are fold_ops.h's, shared with the fold.
#include "fold_ops.h"
#include "set_geom.h"   // collect_plan, alltoallv_plan

namespace shmx {

namespace {

// The per-XCD L2s are not coherent with each other or with the peers, so a
// system-scope fence must run on EVERY XCD.  Dispatch spreads workgroups
// round-robin over the XCDs in practice, so 64 one-wave blocks put 8 on each
// — but the block -> XCD map is not architecturally defined, so each block
// also records the XCD it ran on (HW_REG_XCC_ID) in seen[blockIdx.x]: the host
// (fence_and_wait) or the next signal_kernel checks that every XCD of the
// device reported, and refills or fails loudly if one did not.
// s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 4): id 20, offset 0, size 4
constexpr int kXccIdReg = 20 | (0 << 6) | ((4 - 1) << 11);

__global__ __launch_bounds__(64) void sys_fence_kernel(unsigned int *seen) {
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "");   // system scope
        const unsigned int xcc = (unsigned int)__builtin_amdgcn_s_getreg(kXccIdReg) & 15u;
        __hip_atomic_store(seen + blockIdx.x, kFenceSeen | xcc, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// One whole wave, lane b holding block b's record (0: none): the XCDs that
// reported, counted; fewer than the device has is error word 2.
__device__ __forceinline__ void count_coverage(const SignalArgs &a, unsigned int rec) {
    int covered = 0;
#pragma unroll
    for (unsigned int x = 0; x < 16; ++x) covered += __ballot(rec == (kFenceSeen | x)) != 0 ? 1 : 0;
    if (threadIdx.x == 0) {
        atomicAdd(a.fence_stats, 1ull);
        if (covered < a.nxcc) {
            atomicAdd(a.fence_stats + 1, 1ull);
            __hip_atomic_store(a.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

__device__ __forceinline__ void check_fence(const SignalArgs &a) {
    // lane b reads block b's record of the fence just before this kernel
    const int lane = threadIdx.x;
    unsigned int rec = 0;
    if (a.seen && lane < kFenceBlocks) {
        rec = __hip_atomic_load(a.seen + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.seen + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!a.seen) return;
    count_coverage(a, rec);
}

__global__ __launch_bounds__(64) void signal_kernel(SignalArgs a) {
    check_fence(a);
    const int i = threadIdx.x;
    if (i >= a.P || a.pe[i] == a.me) return;
    unsigned long long *mine = a.mine + a.pe[i];
    const unsigned long long want =
        __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1;
    __hip_atomic_store(mine, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long *theirs = a.peer[i] + a.me;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(theirs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
            __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// ------------------------------------------------ fused one-shot (SIGNAL)
// Thread 0 of the last block to arrive: bump my counter for every peer
// (system-scope release: everything this GPU's blocks fenced before arriving
// is in memory first), then wait for every peer's counter for me.
__device__ void peer_handshake(const SignalArgs &a) {
    unsigned long long want[kMaxFoldInputs];
    for (int i = 0; i < a.P; ++i) {
        if (a.pe[i] == a.me) continue;
        unsigned long long *c = a.mine + a.pe[i];
        want[i] = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1;
        __hip_atomic_store(c, want[i], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < a.P; ++i) {
        if (a.pe[i] == a.me) continue;
        const unsigned long long *theirs = a.peer[i] + a.me;
        while (__hip_atomic_load(theirs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want[i]) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
                __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // system scope
}

// One element of the one-shot fold: the peers' values are remote loads
// (µs each over xGMI), so all nins of them are issued before the first op
// instead of one load's latency per input; heavy ops keep the loop.
template <typename T, int OP>
__device__ __forceinline__ T fold_elem(const SignalFoldArgs &a, size_t i) {
    if constexpr (kHeavyOp<T, OP>) {
        T acc = static_cast<const T *>(a.ins[0])[i];
        for (int k = 1; k < a.nins; ++k) acc = Op<T, OP>::ap(acc, static_cast<const T *>(a.ins[k])[i]);
        return acc;
    } else {
        T x[kMaxFoldInputs];
#pragma unroll
        for (int k = 0; k < kMaxFoldInputs; ++k)
            if (k < a.nins) x[k] = static_cast<const T *>(a.ins[k])[i];
        T acc = x[0];
#pragma unroll
        for (int k = 1; k < kMaxFoldInputs; ++k)
            if (k < a.nins) acc = Op<T, OP>::ap(acc, x[k]);
        return acc;
    }
}

// The entry of a fused launch, one shot and two shot: every block records
// its XCD, fences and arrives at the self-resetting grid barrier (gsync: an
// arrival counter and a generation); the last block to arrive checks the XCD
// coverage, does the entry handshake with the peers (reduce-op.c:217: every
// source is final) and releases the generation.  wait: a block that is not
// the last waits for that release; without it such a block returns at once
// (false), having fenced and arrived, and must leave.  Returns whether this
// block was the last to arrive; *gen0 is the generation the launch found.
// hook: what the last block's lane 0 does between the entry handshake and the
// release of the grid (the collect reads the peers' counts there); nothing
// unless a launch says so.
struct NoEntryHook {
    __device__ __forceinline__ void operator()() const {}
};
template <class Args, class Hook = NoEntryHook>   // Args: their sig and gsync
__device__ __forceinline__ bool fused_entry(const Args &a, bool wait, unsigned int *gen0_out, Hook hook = Hook()) {
    unsigned int *const count = a.gsync, *const gen = a.gsync + 1;
    __shared__ int s_last;
    __shared__ unsigned int s_gen0;
    if (threadIdx.x == 0) {
        // record this block's XCD, then write back the XCD's L2 and drop
        // stale peer lines (the fence also orders the record), arrive
        const unsigned int xcc = (unsigned int)__builtin_amdgcn_s_getreg(kXccIdReg) & 15u;
        __hip_atomic_store(a.sig.seen + blockIdx.x, kFenceSeen | xcc, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "");   // system scope
        const unsigned int gen0 = __hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int old = __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == gridDim.x - 1;
        if (!s_last && wait) {
            // relaxed polls (an acquire load would invalidate the L2 on every
            // poll), one acquire once the generation moved
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen0) {
                if (__builtin_amdgcn_s_memrealtime() - t0 > a.sig.timeout_ticks) {
                    // only if launches overlapped on this GPU (they must not)
                    __hip_atomic_store(a.sig.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        if (s_last || wait) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_gen0 = gen0;   // for the checking wave
    }
    __syncthreads();
    const bool last = s_last;
    *gen0_out = s_gen0;
    if (!last && !wait) return false;
    if (last && threadIdx.x < 64) {
        // the last block's first wave: every block's XCD record at once (lane
        // b reads block b's), then lane 0 does the entry handshake
        const int lane = threadIdx.x;
        unsigned int rec = 0;
        if (lane < (int)gridDim.x) {
            rec = __hip_atomic_load(a.sig.seen + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.sig.seen + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        count_coverage(a.sig, rec);
        if (lane == 0) {
            peer_handshake(a.sig);
            hook();
            __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(gen, s_gen0 + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return last;
}

// The exit of a fused launch: the last block to finish reading tells the
// peers (reduce-op.c:250).
template <class Args>
__device__ __forceinline__ void fused_exit(const Args &a) {
    unsigned int *const count = a.gsync;
    __syncthreads();
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
        __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        peer_handshake(a.sig);
    }
}

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void signal_fold_kernel(SignalFoldArgs a) {
    // up to 4 elements per lane of one block: the last block to arrive folds
    // alone, and no block waits for a release or arrives at the exit
    const bool tiny = a.n <= kFusedTinyElems;
    static_assert(kFusedTinyElems == (size_t)4 * kBlock, "the tiny case is 4 elements per lane of one block");
    unsigned int gen0;
    // a tiny array is folded by the last block alone: the others have fenced
    // and arrived, and leave
    if (!fused_entry(a, !tiny, &gen0) && tiny) return;
    T *out = static_cast<T *>(a.out);
    if (tiny) {
        for (size_t i = threadIdx.x; i < a.n; i += kBlock) out[i] = fold_elem<T, OP>(a, i);
        if (a.host_word) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave's stores landed
        __syncthreads();
        if (threadIdx.x == 0) {
            peer_handshake(a.sig);   // reduce-op.c:250
            // this workgroup did all the work: tell the host (system-scope
            // release: the L2 is written back first)
            if (a.host_word)
                __hip_atomic_store(a.host_word, a.host_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    for (size_t i = tid; i < a.n; i += nthr) out[i] = fold_elem<T, OP>(a, i);
    fused_exit(a);
}

// ------------------------------------------------ fused two-shot (SIGNAL)
// The peers' operands are read over xGMI, where a load's latency (µs) rather
// than HBM bounds a 64-block grid: every lane issues its U 16-B loads from
// each of the nins inputs (uniform predicates, unrolled) before folding any,
// so a block keeps U x nins x 4 KiB in flight per step; U = 16 / MAXIN (4
// vectors per input up to 4 inputs, 2 up to 8, 1 up to 16: 16 vectors in
// registers either way).
template <typename T, int OP, int MAXIN>
__device__ __forceinline__ void fold_vecs(const SignalFoldArgs &a, u32x4 *out, size_t nvec, size_t tid,
                                          size_t nthr) {
    constexpr int U = kMaxFoldInputs / MAXIN;
    const size_t step = nthr * U;
    auto in = [&](int k) {
        return reinterpret_cast<const u32x4 *>(static_cast<const T *>(a.ins[k]) + a.lo);
    };
    size_t v = (tid / kBlock) * kBlock * U + tid % kBlock;   // U vectors of a block are kBlock apart
    for (; v + (size_t)(U - 1) * kBlock < nvec; v += step) {
        u32x4 x[MAXIN][U];
#pragma unroll
        for (int k = 0; k < MAXIN; ++k)
            if (k < a.nins)
#pragma unroll
                for (int u = 0; u < U; ++u) x[k][u] = __builtin_nontemporal_load(in(k) + v + u * kBlock);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 acc = x[0][u];
#pragma unroll
            for (int k = 1; k < MAXIN; ++k)
                if (k < a.nins) acc = apply16<T, OP>(acc, x[k][u]);
            out[v + u * kBlock] = acc;
        }
    }
    for (int u = 0; u < U; ++u) {   // the last partial step
        const size_t w = v + (size_t)u * kBlock;
        if (w >= nvec) break;
        u32x4 acc = __builtin_nontemporal_load(in(0) + w);
        for (int k = 1; k < a.nins; ++k) acc = apply16<T, OP>(acc, __builtin_nontemporal_load(in(k) + w));
        out[w] = acc;
    }
}

template <typename T, int OP>
__device__ __forceinline__ void fold_span(const SignalFoldArgs &a, size_t tid, size_t nthr) {
    constexpr int E = 16 / sizeof(T);
    const size_t lo = a.lo, n = a.hi - a.lo;
    T *const out = static_cast<T *>(a.out) + lo;
    bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int k = 0; k < a.nins; ++k)
        vec &= (reinterpret_cast<uintptr_t>(static_cast<const T *>(a.ins[k]) + lo) & 15) == 0;
    const size_t nvec = vec ? n / E : 0;
    u32x4 *const vout = reinterpret_cast<u32x4 *>(out);
    // soft x87 and the complex products (Annex G recovery branch) unrolled
    // 16 vectors deep would spill: one vector of one input at a time
    if constexpr (kHeavyOp<T, OP>) {
        for (size_t v = tid; v < nvec; v += nthr) {
            u32x4 acc = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(
                                                       static_cast<const T *>(a.ins[0]) + lo) + v);
            for (int k = 1; k < a.nins; ++k)
                acc = apply16<T, OP>(acc, __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(
                                                  static_cast<const T *>(a.ins[k]) + lo) + v));
            vout[v] = acc;
        }
    } else if (a.nins <= 4) {
        fold_vecs<T, OP, 4>(a, vout, nvec, tid, nthr);
    } else if (a.nins <= 8) {
        fold_vecs<T, OP, 8>(a, vout, nvec, tid, nthr);
    } else {
        fold_vecs<T, OP, 16>(a, vout, nvec, tid, nthr);
    }
    for (size_t i = nvec * E + tid; i < n; i += nthr) {
        T acc = static_cast<const T *>(a.ins[0])[lo + i];
        for (int k = 1; k < a.nins; ++k) acc = Op<T, OP>::ap(acc, static_cast<const T *>(a.ins[k])[lo + i]);
        out[i] = acc;
    }
}

// The all-gather of the two-shot: every segment's loads of a step issued
// before any store, so all peers' links are busy at once (U vectors per
// segment per lane, as fold_vecs).
template <int MAXSEG, class Segs>   // SignalFoldArgs or SegList: their nseg, gsrc, gdst, glen
__device__ __forceinline__ void gather_vecs(const Segs &a, size_t nvec, size_t tid, size_t nthr) {
    constexpr int U = kMaxFoldInputs / MAXSEG;
    for (size_t v = (tid / kBlock) * kBlock * U + tid % kBlock; v < nvec; v += nthr * U) {
        u32x4 x[MAXSEG][U];
#pragma unroll
        for (int k = 0; k < MAXSEG; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k < a.nseg && v + u * kBlock < a.glen[k] / 16)
                    x[k][u] = __builtin_nontemporal_load(static_cast<const u32x4 *>(a.gsrc[k]) + v + u * kBlock);
#pragma unroll
        for (int k = 0; k < MAXSEG; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k < a.nseg && v + u * kBlock < a.glen[k] / 16)
                    static_cast<u32x4 *>(a.gdst[k])[v + u * kBlock] = x[k][u];
    }
}

template <class Segs>
__device__ __forceinline__ void gather_span(const Segs &a, size_t tid, size_t nthr) {
    bool vec = true;
    size_t most = 0;
    for (int k = 0; k < a.nseg; ++k) {
        vec &= ((reinterpret_cast<uintptr_t>(a.gsrc[k]) | reinterpret_cast<uintptr_t>(a.gdst[k])) & 15) == 0;
        most = a.glen[k] > most ? a.glen[k] : most;
    }
    if (!vec) {
        for (int k = 0; k < a.nseg; ++k)
            for (size_t i = tid; i < a.glen[k]; i += nthr)
                static_cast<unsigned char *>(a.gdst[k])[i] = static_cast<const unsigned char *>(a.gsrc[k])[i];
        return;
    }
    if (a.nseg <= 4) gather_vecs<4>(a, most / 16, tid, nthr);
    else if (a.nseg <= 8) gather_vecs<8>(a, most / 16, tid, nthr);
    else gather_vecs<16>(a, most / 16, tid, nthr);
    for (int k = 0; k < a.nseg; ++k)
        for (size_t i = a.glen[k] / 16 * 16 + tid; i < a.glen[k]; i += nthr)
            static_cast<unsigned char *>(a.gdst[k])[i] = static_cast<const unsigned char *>(a.gsrc[k])[i];
}

// Grid barrier + peer handshake inside the kernel: every block writes back
// its XCD's L2 (its own stores become visible over xGMI) and arrives; the
// last one does the handshake and releases the generation gen_now + 1; every
// block then drops stale lines of the peers' memory (system acquire) before
// it reads what the peers wrote.
template <class Args>
__device__ void grid_handshake(const Args &a, unsigned int gen_now) {
    unsigned int *const count = a.gsync, *const gen = a.gsync + 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope
        if (__hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            peer_handshake(a.sig);
            __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(gen, gen_now + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen_now) {
                if (__builtin_amdgcn_s_memrealtime() - t0 > a.sig.timeout_ticks) {
                    __hip_atomic_store(a.sig.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // system scope
    }
    __syncthreads();
}

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void signal_fold2_kernel(SignalFoldArgs a) {
    unsigned int gen0;
    fused_entry(a, true, &gen0);        // every block waits for the entry handshake
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    fold_span<T, OP>(a, tid, nthr);     // my slice from every member's source
    grid_handshake(a, gen0 + 1u);       // every member's slice is final
    gather_span(a, tid, nthr);          // the other slices from the peers' targets
    fused_exit(a);
}

// ------------------------------------------- fused own slice (SIGNAL)
// The fused two shot for the six own-order pairs: the owner of a slice folds
// it in all P member orders at once (fold_orders_of, fold_ops.h), its own
// order into its target's slice, the other P - 1 into its result slots; after
// the mid handshake every member gathers its slot from every other owner.
//
// The fold is fold_orders_kernel's vector body (fold_kernels.hip, whose
// measured table says why): ONE 16-byte vector per input per lane, all nins
// loads of a vector issued back to back under the one guard v < nvec before
// the first select and before any store (so outs[k] may be ins[k] + lo: the
// in-place call), MAXIN 8 / 16, the rolled order loop for long double.
// Non-temporal loads, plain stores, as fold_vecs.  The vector body runs only
// when all P inputs at lo and all P outputs are 16-byte aligned; otherwise
// the scalar loop takes the whole slice, as fold_span decides.
//
// Both MAXIN bodies are in one kernel, so its registers are the MAXIN 16
// body's.  hipcc (ROCm 7), gfx950, -O3, per instance: VGPRs / AGPRs / SGPRs /
// scratch bytes per lane / waves per SIMD
//     float        min, max   151 / 0 / 106 / 0 / 3
//     double       min, max   151 / 0 / 106 / 0 / 3
//     long double  min        150 / 0 / 106 / 0 / 3
//     long double  max        147 / 0 / 106 / 0 / 3
// No instance touches scratch memory.  The 2 P array pointers and the gather's
// 3 x 16 words are all wave-uniform, more than the SGPR file: 38 SGPRs (float,
// double) and 364 (long double, around the rolled loop's soft-x87 compare)
// are parked in VGPR lanes (v_writelane / v_readlane), which the VGPR counts
// above include.
template <typename T, int OP, int MAXIN>
__device__ __forceinline__ void orders_span_of(const SignalOrdersArgs &a, bool vec, size_t tid, size_t nthr) {
    constexpr int E = 16 / sizeof(T);
    constexpr bool ROLLED = std::is_same<T, ld80>::value;
    const int nins = a.f.nins;
    const size_t lo = a.f.lo, n = a.f.hi - a.f.lo;
    const size_t nvec = vec ? n / E : 0;
    auto in = [&](int k) { return reinterpret_cast<const u32x4 *>(static_cast<const T *>(a.f.ins[k]) + lo); };
    for (size_t v = tid; v < nvec; v += nthr) {
        u32x4 x[MAXIN];
#pragma unroll
        for (int k = 0; k < MAXIN; ++k)
            if (k < nins) x[k] = __builtin_nontemporal_load(in(k) + v);
        fold_orders_of<T, OP, MAXIN, ROLLED>(
            x, nins, [](u32x4 p, u32x4 q) { return apply16<T, OP>(p, q); },
            [&](int k, u32x4 r) { static_cast<u32x4 *>(a.outs[k])[v] = r; });
    }
    for (size_t i = nvec * E + tid; i < n; i += nthr) {
        T x[MAXIN];
#pragma unroll
        for (int k = 0; k < MAXIN; ++k)
            if (k < nins) x[k] = static_cast<const T *>(a.f.ins[k])[lo + i];
        fold_orders_of<T, OP, MAXIN, ROLLED>(
            x, nins, [](T p, T q) { return Op<T, OP>::ap(p, q); },
            [&](int k, T r) { static_cast<T *>(a.outs[k])[i] = r; });
    }
}

template <typename T, int OP>
__device__ __forceinline__ void orders_span(const SignalOrdersArgs &a, size_t tid, size_t nthr) {
    bool vec = true;
    for (int k = 0; k < a.f.nins; ++k)
        vec &= ((reinterpret_cast<uintptr_t>(static_cast<const T *>(a.f.ins[k]) + a.f.lo) |
                 reinterpret_cast<uintptr_t>(a.outs[k])) & 15) == 0;
    if (a.f.nins <= 8) orders_span_of<T, OP, 8>(a, vec, tid, nthr);
    else orders_span_of<T, OP, 16>(a, vec, tid, nthr);
}

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void signal_orders2_kernel(SignalOrdersArgs a) {
    unsigned int gen0;
    fused_entry(a.f, true, &gen0);        // every block waits for the entry handshake
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    orders_span<T, OP>(a, tid, nthr);     // my slice of every source, in every member's order
    grid_handshake(a.f, gen0 + 1u);       // every owner's slots are final
    gather_span(a.f, tid, nthr);          // my slot of every other owner's slice
    fused_exit(a.f);
}

// ------------------------------------------------ fused pull (SIGNAL)
// The stream-ordered broadcast and fcollect (pull.cpp): byte ranges pulled
// from the peers' heaps under the fused launches' barriers, untyped, one
// instance.  List a after the entry handshake (fcollect: every member's
// source; broadcast: this member's part of the root's source); with two_phase
// a mid handshake (every non-root's slice is final and visible over xGMI) and
// list b (the other slices from the other non-roots' targets).  Every member
// of a set runs the same handshakes whatever its lists hold: the root of a
// broadcast has none and still runs them all.
//
// hipcc (ROCm 7), gfx950, -O3: VGPRs / AGPRs / SGPRs / scratch bytes per lane
// / waves per SIMD
//     signal_pull_kernel   147 / 0 / 106 / 0 / 3
// No scratch memory.  Both lists' 3 x 16 words are wave-uniform, more than
// the SGPR file: 38 SGPRs are parked in VGPR lanes (v_writelane /
// v_readlane), which the VGPR count includes, as in the own-slice kernel.
__global__ __launch_bounds__(kBlock) void signal_pull_kernel(SignalPullArgs a) {
    unsigned int gen0;
    fused_entry(a, true, &gen0);        // every source is final; nobody still reads my target
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    gather_span(a.a, tid, nthr);
    if (a.two_phase || a.b.nseg > 0) {
        grid_handshake(a, gen0 + 1u);   // every non-root's slice is final
        gather_span(a.b, tid, nthr);    // the other slices from the other non-roots' targets
    }
    fused_exit(a);                      // nobody reads my source or target any more
}

// ------------------------------------------------ collect (SIGNAL)
// The stream-ordered collect (pull.cpp): the fused pull with the members'
// counts exchanged on the device first.  The count word protocol:
//   publish   one thread stores this member's count (or poison) in its own
//             word, system scope, BEFORE its block's fence-and-arrive (fused)
//             or in a kernel before the first barrier's fence (unfused): the
//             entry handshake's release covers it;
//   exchange  after the entry handshake ONE thread (the last block's lane 0
//             before it releases the grid; the plan kernel's lane 0) reads all
//             P words with system-scope loads, as the counters are polled,
//             all loads issued before the first is used, runs collect_plan
//             (set_geom.h) and leaves the plan in a device buffer (8-byte
//             agent-scope stores), so the blocks do not each read P remote
//             words; it also stores where[] and counts an overflow;
//   setup     every block reads the plan (8-byte agent-scope loads, after the
//             grid's acquire or the kernel boundary) into LDS and lists its
//             segments there;
//   copy      collect_span, or nothing on overflow; then the exit handshake.
// An overflow leaves the SIGNAL error word alone: it is an answer, not a
// fault, and every member sees the same one.
//
// collect_span decides per segment: source and target congruent mod 16 take
// 16-byte vectors between a head and a tail of element-wide words, any other
// segment element-wide (4- or 8-byte) words throughout; no byte loop (the
// operands are whole elements) and no realigned vectors.  As gather_vecs, a
// lane issues the loads of all segments of a step before any store, U = 16 /
// MAXSEG units per segment.  The segments are known only on the device, so
// they live in LDS, not in the kernarg's SGPRs as gather_vecs' do.
//
// hipcc (ROCm 7), gfx950, -O3: VGPRs / AGPRs / SGPRs / scratch bytes per lane
// / LDS bytes / waves per SIMD
//     signal_collect_kernel    170 / 0 / 106 / 0 / 1328 / 2
//     collect_copy_kernel      171 / 0 / 106 / 0 / 1200 / 2
//     collect_publish_kernel     3 / 0 /  18 / 0 /    0 / 8
//     collect_plan_kernel       33 / 0 /  74 / 0 /  544 / 8
// No scratch memory.  The copy kernel parks 34 SGPRs in VGPR lanes, which its
// VGPR count includes; the fused kernel none.  Two waves per SIMD are more
// than the fused launch's 64 blocks of 4 waves on 256 CUs ever place.
struct CollectSegs {
    unsigned long long most;                    // the longest segment's units
    const char *src[kMaxFoldInputs];            // the body's first byte
    char *dst[kMaxFoldInputs];
    unsigned long long units[kMaxFoldInputs];   // 16-byte vectors, or elements
    unsigned long long len[kMaxFoldInputs];     // bytes, head and tail included
    unsigned int head[kMaxFoldInputs];          // bytes before the body (vector segments)
    unsigned int vec[kMaxFoldInputs];
};

static_assert(kCollectMaxMembers == kMaxFoldInputs, "one member per fold input");
static_assert(kCollectPlanWords <= 64, "one wave reads the plan");

// one thread
__device__ __forceinline__ void collect_publish(const CollectArgs &c) {
    unsigned long long n =
        c.count_dev ? __hip_atomic_load(c.count_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : c.count;
    if (n > c.capacity || n > c.src_room) n = kCollectPoison;
    __hip_atomic_store(c.my_word, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// one thread; counts and plan are its block's LDS
__device__ __forceinline__ void collect_exchange(const CollectArgs &c, unsigned long long *counts,
                                                 CollectPlan *plan) {
    unsigned long long x[kMaxFoldInputs];
#pragma unroll
    for (int i = 0; i < kMaxFoldInputs; ++i)
        if (i < c.P) x[i] = __hip_atomic_load(c.word[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
    for (int i = 0; i < kMaxFoldInputs; ++i)
        if (i < c.P) counts[i] = x[i];
    collect_plan(counts, c.P, c.capacity, c.esize, c.m, plan);
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(plan);
    for (int k = 0; k < kCollectPlanWords; ++k)
        __hip_atomic_store(c.plan + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool over = plan->overflow != 0;
    if (c.where) {
        __hip_atomic_store(c.where, over ? kCollectPoison : plan->offset[c.m], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(c.where + 1, over ? kCollectPoison : plan->total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (over)   // this GPU's launches, which never overlap, are the only writer
        __hip_atomic_store(c.overflows,
                           __hip_atomic_load(c.overflows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// every thread of a block: the plan from the device buffer, then the block's
// segment list (none on overflow)
__device__ __forceinline__ void collect_setup(const CollectArgs &c, CollectPlan *plan, const void **srcs,
                                              CollectSegs *g) {
    unsigned long long *const w = reinterpret_cast<unsigned long long *>(plan);
    if (threadIdx.x < kCollectPlanWords)
        w[threadIdx.x] = __hip_atomic_load(c.plan + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kMaxFoldInputs; ++i) srcs[i] = c.src[i];
    }
    __syncthreads();
    const int nseg = plan->nseg <= (unsigned long long)c.P ? (int)plan->nseg : 0;
    const int k = threadIdx.x;
    if (k < nseg) {
        const int i = (int)(plan->order[k] % kMaxFoldInputs);
        const char *s = static_cast<const char *>(srcs[i]);
        char *d = static_cast<char *>(c.tgt) + plan->offset[i] * c.esize;
        const unsigned long long len = plan->count[i] * c.esize;
        const bool vec = ((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d)) & 15) == 0;
        unsigned long long head = vec ? (16 - (reinterpret_cast<uintptr_t>(s) & 15)) & 15 : 0;
        if (head > len) head = len;
        g->src[k] = s + head;
        g->dst[k] = d + head;
        g->len[k] = len;
        g->head[k] = (unsigned int)head;
        g->vec[k] = vec ? 1u : 0u;
        g->units[k] = vec ? (len - head) / 16 : len / c.esize;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long most = 0;
        for (int j = 0; j < nseg; ++j) most = g->units[j] > most ? g->units[j] : most;
        g->most = most;
    }
    __syncthreads();
}

template <int MAXSEG, typename W>   // W: the element-wide word
__device__ __forceinline__ void collect_units(const CollectSegs &g, int nseg, size_t tid, size_t nthr) {
    constexpr int U = kMaxFoldInputs / MAXSEG;
    const size_t most = g.most;
    for (size_t v = (tid / kBlock) * kBlock * U + tid % kBlock; v < most; v += nthr * U) {
        u32x4 x[MAXSEG][U];
#pragma unroll
        for (int k = 0; k < MAXSEG; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k < nseg && v + u * kBlock < g.units[k]) {
                    if (g.vec[k]) {
                        x[k][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(g.src[k]) + v + u * kBlock);
                    } else {
                        const W e = __builtin_nontemporal_load(reinterpret_cast<const W *>(g.src[k]) + v + u * kBlock);
                        x[k][u].x = (unsigned int)e;
                        if constexpr (sizeof(W) == 8) x[k][u].y = (unsigned int)(e >> 32);
                    }
                }
#pragma unroll
        for (int k = 0; k < MAXSEG; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k < nseg && v + u * kBlock < g.units[k]) {
                    if (g.vec[k]) {
                        reinterpret_cast<u32x4 *>(g.dst[k])[v + u * kBlock] = x[k][u];
                    } else {
                        W e = x[k][u].x;
                        if constexpr (sizeof(W) == 8) e |= (W)x[k][u].y << 32;
                        reinterpret_cast<W *>(g.dst[k])[v + u * kBlock] = e;
                    }
                }
    }
}

template <typename W>
__device__ __forceinline__ void collect_span(const CollectSegs &g, int nseg, size_t tid, size_t nthr) {
    if (nseg <= 4) collect_units<4, W>(g, nseg, tid, nthr);
    else if (nseg <= 8) collect_units<8, W>(g, nseg, tid, nthr);
    else collect_units<16, W>(g, nseg, tid, nthr);
    // a vector segment's head and tail: fewer than 16 bytes each
    for (int k = 0; k < nseg; ++k) {
        if (!g.vec[k]) continue;
        const size_t head = g.head[k], body = (size_t)g.units[k] * 16;
        const size_t he = head / sizeof(W), te = ((size_t)g.len[k] - head - body) / sizeof(W);
        if (tid >= he + te) continue;
        // relative to the body's first byte
        const ptrdiff_t off = tid < he ? (ptrdiff_t)(tid * sizeof(W)) - (ptrdiff_t)head
                                       : (ptrdiff_t)(body + (tid - he) * sizeof(W));
        *reinterpret_cast<W *>(g.dst[k] + off) = *reinterpret_cast<const W *>(g.src[k] + off);
    }
}

__device__ __forceinline__ void collect_copy(const CollectArgs &c, const CollectPlan &plan, const CollectSegs &g) {
    const int nseg = plan.overflow || plan.nseg > (unsigned long long)c.P ? 0 : (int)plan.nseg;
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    if (c.esize == 4) collect_span<unsigned int>(g, nseg, tid, nthr);
    else collect_span<unsigned long long>(g, nseg, tid, nthr);
}

__global__ __launch_bounds__(kBlock) void signal_collect_kernel(SignalCollectArgs a) {
    __shared__ CollectPlan s_plan;
    __shared__ unsigned long long s_counts[kMaxFoldInputs];
    __shared__ const void *s_srcs[kMaxFoldInputs];
    __shared__ CollectSegs s_segs;
    if (blockIdx.x == 0 && threadIdx.x == 0) collect_publish(a.c);   // before this block's fence-and-arrive
    unsigned int gen0;
    // every source and every count is final; nobody still reads my target
    fused_entry(a, true, &gen0, [&] { collect_exchange(a.c, s_counts, &s_plan); });
    collect_setup(a.c, &s_plan, s_srcs, &s_segs);
    collect_copy(a.c, s_plan, s_segs);
    fused_exit(a);   // nobody reads my source, my target or my count any more
}

__global__ __launch_bounds__(64) void collect_publish_kernel(CollectArgs c) {
    if (threadIdx.x == 0) collect_publish(c);
}

__global__ __launch_bounds__(64) void collect_plan_kernel(CollectArgs c) {
    __shared__ CollectPlan s_plan;
    __shared__ unsigned long long s_counts[kMaxFoldInputs];
    if (threadIdx.x == 0) collect_exchange(c, s_counts, &s_plan);
}

__global__ __launch_bounds__(kBlock) void collect_copy_kernel(CollectArgs c) {
    __shared__ CollectPlan s_plan;
    __shared__ const void *s_srcs[kMaxFoldInputs];
    __shared__ CollectSegs s_segs;
    collect_setup(c, &s_plan, s_srcs, &s_segs);
    collect_copy(c, s_plan, s_segs);
}

// ------------------------------------------------ alltoallv (SIGNAL)
// The stream-ordered alltoall and alltoallv (pull.cpp): the collect's
// all-to-all generalisation.  Nothing is published: the count and offset
// tables are ordinary symmetric objects, final before their owner's entry
// handshake like every source.
//   exchange  after the entry handshake ONE thread (the last block's lane 0
//             before it releases the grid; the plan kernel's lane 0) reads the
//             pair (send_counts_i[m], send_offsets_i[m]) of every member i
//             with system-scope loads, all 2 P issued before the first is
//             used, runs alltoallv_plan (set_geom.h), which rejects a pair
//             that would read outside its sender's source, and leaves the
//             plan in a device buffer (8-byte agent-scope stores); it also
//             stores where[0..P] and counts an overflow.  With immediates
//             (the fixed alltoall: cnt[0] is null) it loads nothing;
//   setup     every block reads the plan (8-byte agent-scope loads) into LDS
//             and lists its segments there, sender i's from
//             src[i] + from[i] * esize;
//   copy      collect_span, under its rule, or nothing on overflow; then the
//             exit handshake.
// The overflow is this receiver's alone: its peers complete normally, and the
// SIGNAL error word is left alone.
//
// hipcc (ROCm 7), gfx950, -O3: VGPRs / AGPRs / SGPRs / scratch bytes per lane
// / LDS bytes / waves per SIMD
//     signal_alltoallv_kernel  170 / 0 / 106 / 0 / 1584 / 2
//     alltoallv_copy_kernel    171 / 0 / 106 / 0 / 1328 / 2
//     alltoallv_plan_kernel     65 / 0 /  94 / 0 /  800 / 7
// No scratch memory.  As the collect's, the copy kernel parks 34 SGPRs in VGPR
// lanes, which its VGPR count includes; the fused kernel none.
static_assert(kAlltoallvPlanWords <= kBlock, "one block reads the plan");

// one thread; counts, offs and plan are its block's LDS
__device__ __forceinline__ void alltoallv_exchange(const AlltoallvArgs &c, unsigned long long *counts,
                                                   unsigned long long *offs, AlltoallvPlan *plan) {
    if (c.cnt[0]) {
        unsigned long long x[kMaxFoldInputs], y[kMaxFoldInputs];
#pragma unroll
        for (int i = 0; i < kMaxFoldInputs; ++i)
            if (i < c.P) {
                x[i] = __hip_atomic_load(c.cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                y[i] = __hip_atomic_load(c.off[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
#pragma unroll
        for (int i = 0; i < kMaxFoldInputs; ++i)
            if (i < c.P) {
                counts[i] = x[i];
                offs[i] = y[i];
            }
    } else {
        for (int i = 0; i < c.P; ++i) {
            counts[i] = c.nelems;
            offs[i] = (unsigned long long)c.m * c.nelems;
        }
    }
    alltoallv_plan(counts, offs, c.P, c.capacity, c.src_capacity, c.esize, c.m, plan);
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(plan);
    for (int k = 0; k < kAlltoallvPlanWords; ++k)
        __hip_atomic_store(c.plan + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool over = plan->overflow != 0;
    if (c.where) {
        for (int i = 0; i < c.P; ++i)
            __hip_atomic_store(c.where + i, over ? kCollectPoison : plan->offset[i], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(c.where + c.P, over ? kCollectPoison : plan->total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (over)   // this GPU's launches, which never overlap, are the only writer
        __hip_atomic_store(c.overflows,
                           __hip_atomic_load(c.overflows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// every thread of a block: the plan from the device buffer, then the block's
// segment list (none on overflow)
__device__ __forceinline__ void alltoallv_setup(const AlltoallvArgs &c, AlltoallvPlan *plan, const void **srcs,
                                                CollectSegs *g) {
    unsigned long long *const w = reinterpret_cast<unsigned long long *>(plan);
    if (threadIdx.x < kAlltoallvPlanWords)
        w[threadIdx.x] = __hip_atomic_load(c.plan + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kMaxFoldInputs; ++i) srcs[i] = c.src[i];
    }
    __syncthreads();
    const int nseg = plan->overflow || plan->nseg > (unsigned long long)c.P ? 0 : (int)plan->nseg;
    const int k = threadIdx.x;
    if (k < nseg) {
        const int i = (int)(plan->order[k] % kMaxFoldInputs);
        const char *s = static_cast<const char *>(srcs[i]) + plan->from[i] * c.esize;
        char *d = static_cast<char *>(c.tgt) + plan->offset[i] * c.esize;
        const unsigned long long len = plan->count[i] * c.esize;
        const bool vec = ((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d)) & 15) == 0;
        unsigned long long head = vec ? (16 - (reinterpret_cast<uintptr_t>(s) & 15)) & 15 : 0;
        if (head > len) head = len;
        g->src[k] = s + head;
        g->dst[k] = d + head;
        g->len[k] = len;
        g->head[k] = (unsigned int)head;
        g->vec[k] = vec ? 1u : 0u;
        g->units[k] = vec ? (len - head) / 16 : len / c.esize;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long most = 0;
        for (int j = 0; j < nseg; ++j) most = g->units[j] > most ? g->units[j] : most;
        g->most = most;
    }
    __syncthreads();
}

__device__ __forceinline__ void alltoallv_copy(const AlltoallvArgs &c, const AlltoallvPlan &plan,
                                               const CollectSegs &g) {
    const int nseg = plan.overflow || plan.nseg > (unsigned long long)c.P ? 0 : (int)plan.nseg;
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    if (c.esize == 4) collect_span<unsigned int>(g, nseg, tid, nthr);
    else collect_span<unsigned long long>(g, nseg, tid, nthr);
}

__global__ __launch_bounds__(kBlock) void signal_alltoallv_kernel(SignalAlltoallvArgs a) {
    __shared__ AlltoallvPlan s_plan;
    __shared__ unsigned long long s_counts[kMaxFoldInputs], s_offs[kMaxFoldInputs];
    __shared__ const void *s_srcs[kMaxFoldInputs];
    __shared__ CollectSegs s_segs;
    unsigned int gen0;
    // every source and every table is final; nobody still reads my target
    fused_entry(a, true, &gen0, [&] { alltoallv_exchange(a.c, s_counts, s_offs, &s_plan); });
    alltoallv_setup(a.c, &s_plan, s_srcs, &s_segs);
    alltoallv_copy(a.c, s_plan, s_segs);
    fused_exit(a);   // nobody reads my source or my tables any more
}

__global__ __launch_bounds__(64) void alltoallv_plan_kernel(AlltoallvArgs c) {
    __shared__ AlltoallvPlan s_plan;
    __shared__ unsigned long long s_counts[kMaxFoldInputs], s_offs[kMaxFoldInputs];
    if (threadIdx.x == 0) alltoallv_exchange(c, s_counts, s_offs, &s_plan);
}

__global__ __launch_bounds__(kBlock) void alltoallv_copy_kernel(AlltoallvArgs c) {
    __shared__ AlltoallvPlan s_plan;
    __shared__ const void *s_srcs[kMaxFoldInputs];
    __shared__ CollectSegs s_segs;
    alltoallv_setup(c, &s_plan, s_srcs, &s_segs);
    alltoallv_copy(c, s_plan, s_segs);
}

// ------------------------------------------------ reduce-scatter (SIGNAL)
// The stream-ordered reduce-scatter (pull.cpp): the fused two shot's first
// phase alone.  After the entry handshake (every source is final; nobody still
// reads my target) every block folds its share of the P blocks ins[k] (member
// k's source at this member's block, set order) into out, elements [lo, hi) =
// [0, nelems); the exit handshake tells the peers that this member reads their
// sources no more.  No mid handshake and no gather: nobody reads a target.
// No tiny path and no host word: the call never blocks.
//
// The fold is fold_span under its rule: 16-byte vectors when the target and
// all P block starts are 16-byte aligned, the element loop otherwise; no
// realigned vectors.
//
// hipcc (ROCm 7), gfx950, -O3, per instance: VGPRs / AGPRs / SGPRs / scratch
// bytes per lane / waves per SIMD
//     int          sum    110 / 0 / 84 /  0 / 4
//     double       sum    110 / 0 / 84 /  0 / 4
//     float        min    110 / 0 / 80 /  0 / 4
//     long double  sum     40 / 0 / 98 / 40 / 8
//     complexd     prod    40 / 0 / 56 /  0 / 8
// Every light instance (every pair but soft x87's and the complex products)
// has 110-113 VGPRs, 80-84 SGPRs, 4 waves per SIMD and no scratch memory, and
// no instance spills a register.  Of the heavy ones only long double sum and
// product use scratch, the 40 bytes per lane of soft x87's rounding that
// signal_fold2_kernel<ld80, sum> has too: it is the same fold.
template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void signal_reduce_scatter_kernel(SignalFoldArgs a) {
    unsigned int gen0;
    fused_entry(a, true, &gen0);        // every source is final; nobody still reads my target
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    fold_span<T, OP>(a, tid, nthr);     // my block of every member's source
    fused_exit(a);                      // nobody reads my source any more
}

// Blocks of the fused launches: kFenceBlocks, so every XCD gets 8 (the entry
// check counts them); 8-32 blocks measured within 1 us of it
// (profiles/r05_fused_blocks.txt).
constexpr unsigned kFusedBlocks = kFenceBlocks;

template <typename T, int OP>
hipError_t sf_launch(const SignalFoldArgs &a, hipStream_t s) {
    if (a.two_shot)
        hipLaunchKernelGGL((signal_fold2_kernel<T, OP>), dim3(kFusedBlocks), dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL((signal_fold_kernel<T, OP>), dim3(kFusedBlocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_signal_fold(int type, int op, const SignalFoldArgs &a, hipStream_t stream) {
    if (!op_on_device(type, op) || a.nins < 1 || a.nins > kMaxFoldInputs || !a.out || !a.gsync ||
        !a.sig.seen || !a.sig.fence_stats || a.sig.P < 1 || a.sig.P > kMaxFoldInputs || !a.sig.mine ||
        !a.sig.err)
        return hipErrorInvalidValue;
    for (int k = 0; k < a.nins; ++k)
        if (!a.ins[k]) return hipErrorInvalidValue;
    for (int i = 0; i < a.sig.P; ++i)
        if (a.sig.pe[i] != a.sig.me && !a.sig.peer[i]) return hipErrorInvalidValue;
    if (a.two_shot) {
        if (a.lo > a.hi || a.hi > a.n || a.nseg < 0 || a.nseg > kMaxFoldInputs) return hipErrorInvalidValue;
        for (int k = 0; k < a.nseg; ++k)
            if (a.glen[k] && (!a.gsrc[k] || !a.gdst[k])) return hipErrorInvalidValue;
    }
    hipError_t e = hipErrorInvalidValue;
    with_type_op(type, op, [&](auto t, auto o) {
        e = sf_launch<typename decltype(t)::type, decltype(o)::value>(a, stream);
    });
    return e;
}

hipError_t launch_signal_orders(int type, int op, const SignalOrdersArgs &a, hipStream_t stream) {
    const SignalFoldArgs &f = a.f;
    if (f.nins < 1 || f.nins > kMaxFoldInputs || !f.out || !f.gsync || !f.sig.seen || !f.sig.fence_stats ||
        f.sig.P < 1 || f.sig.P > kMaxFoldInputs || !f.sig.mine || !f.sig.err)
        return hipErrorInvalidValue;
    for (int k = 0; k < f.nins; ++k)
        if (!f.ins[k] || !a.outs[k]) return hipErrorInvalidValue;
    for (int i = 0; i < f.sig.P; ++i)
        if (f.sig.pe[i] != f.sig.me && !f.sig.peer[i]) return hipErrorInvalidValue;
    if (f.lo > f.hi || f.hi > f.n || f.nseg < 0 || f.nseg > kMaxFoldInputs) return hipErrorInvalidValue;
    for (int k = 0; k < f.nseg; ++k)
        if (f.glen[k] && (!f.gsrc[k] || !f.gdst[k])) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;   // any pair but the six
    with_type_op(type, op, [&](auto t, auto o) {
        using T = typename decltype(t)::type;
        constexpr int OP = decltype(o)::value;
        if constexpr (kOwnOrderPair<T, OP>) {
            hipLaunchKernelGGL((signal_orders2_kernel<T, OP>), dim3(kFusedBlocks), dim3(kBlock), 0, stream, a);
            e = hipGetLastError();
        }
    });
    return e;
}

hipError_t launch_signal_pull(const SignalPullArgs &a, hipStream_t stream) {
    if (!a.gsync || !a.sig.seen || !a.sig.fence_stats || a.sig.P < 1 || a.sig.P > kMaxFoldInputs || !a.sig.mine ||
        !a.sig.err)
        return hipErrorInvalidValue;
    for (int i = 0; i < a.sig.P; ++i)
        if (a.sig.pe[i] != a.sig.me && !a.sig.peer[i]) return hipErrorInvalidValue;
    for (const SegList *l : {&a.a, &a.b}) {
        if (l->nseg < 0 || l->nseg > kMaxFoldInputs) return hipErrorInvalidValue;
        for (int k = 0; k < l->nseg; ++k)
            if (l->glen[k] && (!l->gsrc[k] || !l->gdst[k])) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(signal_pull_kernel, dim3(kFusedBlocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_signal_reduce_scatter(int type, int op, const SignalFoldArgs &a, hipStream_t stream) {
    if (!op_on_device(type, op) || a.nins < 1 || a.nins > kMaxFoldInputs || !a.out || !a.gsync ||
        !a.sig.seen || !a.sig.fence_stats || a.sig.P < 1 || a.sig.P > kMaxFoldInputs || !a.sig.mine ||
        !a.sig.err || a.lo != 0 || a.hi != a.n)
        return hipErrorInvalidValue;
    for (int k = 0; k < a.nins; ++k)
        if (!a.ins[k]) return hipErrorInvalidValue;
    for (int i = 0; i < a.sig.P; ++i)
        if (a.sig.pe[i] != a.sig.me && !a.sig.peer[i]) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    with_type_op(type, op, [&](auto t, auto o) {
        hipLaunchKernelGGL((signal_reduce_scatter_kernel<typename decltype(t)::type, decltype(o)::value>),
                           dim3(kFusedBlocks), dim3(kBlock), 0, stream, a);
        e = hipGetLastError();
    });
    return e;
}

namespace {
bool collect_args_ok(const CollectArgs &c) {
    if (c.P < 1 || c.P > kMaxFoldInputs || c.m < 0 || c.m >= c.P || (c.esize != 4 && c.esize != 8) || !c.my_word ||
        !c.tgt || !c.plan || !c.overflows || c.capacity > SIZE_MAX / c.esize)
        return false;
    if (reinterpret_cast<uintptr_t>(c.tgt) % c.esize ||
        (reinterpret_cast<uintptr_t>(c.count_dev) | reinterpret_cast<uintptr_t>(c.where)) % 8)
        return false;
    for (int i = 0; i < c.P; ++i)
        if (!c.word[i] || !c.src[i] || reinterpret_cast<uintptr_t>(c.src[i]) % c.esize) return false;
    return true;
}
}  // namespace

hipError_t launch_signal_collect(const SignalCollectArgs &a, hipStream_t stream) {
    if (!a.gsync || !a.sig.seen || !a.sig.fence_stats || a.sig.P < 1 || a.sig.P > kMaxFoldInputs || !a.sig.mine ||
        !a.sig.err || !collect_args_ok(a.c))
        return hipErrorInvalidValue;
    for (int i = 0; i < a.sig.P; ++i)
        if (a.sig.pe[i] != a.sig.me && !a.sig.peer[i]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(signal_collect_kernel, dim3(kFusedBlocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_collect_publish(const CollectArgs &c, hipStream_t stream) {
    if (!collect_args_ok(c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(collect_publish_kernel, dim3(1), dim3(64), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_collect_plan(const CollectArgs &c, hipStream_t stream) {
    if (!collect_args_ok(c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(collect_plan_kernel, dim3(1), dim3(64), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_collect_copy(const CollectArgs &c, hipStream_t stream) {
    if (!collect_args_ok(c)) return hipErrorInvalidValue;
    // the grid from the capacity alone, which every member shares: a lane holds 16 units of a step
    const size_t blocks = (copy_blocks(Span16{0, (size_t)(c.capacity * c.esize / 16), 0}) + 15) / kMaxFoldInputs;
    hipLaunchKernelGGL(collect_copy_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

namespace {
bool alltoallv_args_ok(const AlltoallvArgs &c) {
    if (c.P < 1 || c.P > kMaxFoldInputs || c.m < 0 || c.m >= c.P || (c.esize != 4 && c.esize != 8) || !c.tgt ||
        !c.plan || !c.overflows || c.capacity > SIZE_MAX / c.esize || c.src_capacity > SIZE_MAX / c.esize)
        return false;
    if (reinterpret_cast<uintptr_t>(c.tgt) % c.esize || reinterpret_cast<uintptr_t>(c.where) % 8) return false;
    const bool imm = !c.cnt[0];
    for (int i = 0; i < c.P; ++i) {
        if (!c.src[i] || reinterpret_cast<uintptr_t>(c.src[i]) % c.esize) return false;
        if (imm ? c.cnt[i] || c.off[i] : !c.cnt[i] || !c.off[i]) return false;
        if ((reinterpret_cast<uintptr_t>(c.cnt[i]) | reinterpret_cast<uintptr_t>(c.off[i])) % 8) return false;
    }
    // immediates: every block m * nelems + nelems inside the source
    if (imm && (c.nelems > c.src_capacity / c.P || c.nelems > c.capacity / c.P)) return false;
    return true;
}
}  // namespace

hipError_t launch_signal_alltoallv(const SignalAlltoallvArgs &a, hipStream_t stream) {
    if (!a.gsync || !a.sig.seen || !a.sig.fence_stats || a.sig.P < 1 || a.sig.P > kMaxFoldInputs || !a.sig.mine ||
        !a.sig.err || !alltoallv_args_ok(a.c))
        return hipErrorInvalidValue;
    for (int i = 0; i < a.sig.P; ++i)
        if (a.sig.pe[i] != a.sig.me && !a.sig.peer[i]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(signal_alltoallv_kernel, dim3(kFusedBlocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_alltoallv_plan(const AlltoallvArgs &c, hipStream_t stream) {
    if (!alltoallv_args_ok(c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alltoallv_plan_kernel, dim3(1), dim3(64), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_alltoallv_copy(const AlltoallvArgs &c, hipStream_t stream) {
    if (!alltoallv_args_ok(c)) return hipErrorInvalidValue;
    // the collect's grid, from the capacity alone, which every member shares: a lane holds 16 units of a step
    const size_t blocks = (copy_blocks(Span16{0, (size_t)(c.capacity * c.esize / 16), 0}) + 15) / kMaxFoldInputs;
    hipLaunchKernelGGL(alltoallv_copy_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_signal(const SignalArgs &a, hipStream_t stream) {
    if (a.P < 1 || a.P > kMaxFoldInputs || !a.mine || !a.err) return hipErrorInvalidValue;
    for (int i = 0; i < a.P; ++i)
        if (a.pe[i] != a.me && !a.peer[i]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_sys_fence(hipStream_t stream, unsigned int *seen) {
    if (!seen) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sys_fence_kernel, dim3(kFenceBlocks), dim3(64), 0, stream, seen);
    return hipGetLastError();
}

}  // namespace shmx
