// Host-resident operands of the blocking entry points: the reference's
// symmetric heap is host memory (memory/symmem.c:168-227, dlmalloc), so
// target and source may live there.  They are staged over PCIe: small arrays
// bounce through page-locked buffers with one wait; large ones go in chunks,
// H2D on one copy stream, the reduction on the library stream, D2H on a
// second copy stream, so both PCIe directions and the device work overlap
// (DESIGN.md §6).  Pageable memory goes through a page-locked ring filled and
// emptied by gangs of CPU threads (copy_gang.h).
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <string>
#include <vector>

#include "copy_gang.h"
#include "heap.h"
#include "internal.h"
#include "shmem_reduce_mi355x.h"
#include "node.h"
#include "state.h"
#include "stage_plan.h"
#include "topology.h"

namespace shmx {

// Host-resident arrays move over PCIe in chunks of this size (pipelined);
// up to kSmallHostBytes they bounce through page-locked buffers instead.
constexpr size_t kStageChunkBytes = size_t(16) << 20;
constexpr size_t kSmallHostBytes = size_t(256) << 10;
constexpr size_t kRingSlots = 4;     // page-locked bounce slots per direction

// ------------------------------------------- page-locked ring, copy pool
// Pageable host arrays (dlmalloc'd heaps, numpy) cannot be DMA'd
// asynchronously; they go through kRingSlots page-locked slots per direction,
// filled and emptied by a small pool of CPU threads, so the CPU copies of
// one chunk overlap the PCIe transfers and device work of its neighbours.
// (A THP-backed ring registered with hipHostRegister measured the same:
// profiles/r05_e2e_nt.txt.)
void ring_free() {
    if (!g_state.ring) return;
    (void)hipHostFree(g_state.ring);
    g_state.ring = nullptr;
    g_state.ring_slot = 0;
}

static bool ring_reserve(size_t slot_bytes) {
    if (g_state.ring && g_state.ring_slot >= slot_bytes) return true;
    if (g_state.ring) {
        device_sync();
        ring_free();
    }
    const size_t bytes = 2 * kRingSlots * slot_bytes;
    if (hipHostMalloc(&g_state.ring, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        g_state.ring = nullptr;
        g_state.ring_slot = 0;
        return false;
    }
    g_state.ring_slot = slot_bytes;
    return true;
}
static char *ring_in(size_t slot) { return static_cast<char *>(g_state.ring) + slot * g_state.ring_slot; }
static char *ring_out(size_t slot) {
    return static_cast<char *>(g_state.ring) + (kRingSlots + slot) * g_state.ring_slot;
}

// this process's allowed CPUs
static std::vector<int> allowed_cpus() {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) != 0) return {};
    std::vector<int> out;
    for (int c = 0; c < CPU_SETSIZE; ++c)
        if (CPU_ISSET(c, &set)) out.push_back(c);
    return out;
}

// allowed CPUs of NUMA node `node` (empty if unknown)
static std::vector<int> node_cpus(int node) { return topo::node_cpus("/sys", node, allowed_cpus()); }

// NUMA node of a GPU (its PCI device's numa_node), or -1
int gpu_numa_node(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    std::string id(bus);
    for (auto &c : id) c = (char)std::tolower((unsigned char)c);
    std::ifstream nf("/sys/bus/pci/devices/" + id + "/numa_node");
    int node = -1;
    if (!(nf >> node) || node < 0) return -1;
    return node;
}

// The staging copy threads of this PE, as CPU sets (topo::plan_copy_threads),
// made once: the job's CPU budget (the cgroup quota, else this process's
// allowed CPUs) shared by the PEs on the node, at most 8 per PE
// ($SHMEMX_COPY_THREADS: that many, as given), each thread confined to its
// own last-level-cache domain (CCD) of the GPU's NUMA node, offset by the PE's
// rank among the PEs whose GPUs share that node.  One thread per domain runs
// 36.8-37.7 GiB/s where the scheduler's placement gave 27.2-37.7 (one PE,
// profiles/r05_e2e_spread.txt); with every PE putting its thread i on domain i
// (round 5), eight PEs stacked theirs on the same CCDs, and 8 x 15 threads
// against a 16-CPU quota ran pageable at 0.53 of pinned.
// Within a domain the scheduler picks an idle core; an unknown topology
// leaves the threads unpinned.
static const std::vector<std::vector<int>> &copy_threads() {
    static const std::vector<std::vector<int>> plan = [] {
        const char *e = std::getenv("SHMEMX_COPY_THREADS");
        const unsigned want = e && *e ? (unsigned)std::max(2, std::min(64, std::atoi(e))) : 8u;
        const std::vector<int> allowed = allowed_cpus();
        const int quota = topo::cgroup_cpu_quota("/sys/fs/cgroup");
        const int budget = e && *e ? 0 : quota > 0 ? std::min(quota, (int)allowed.size()) : (int)allowed.size();
        const int mine = gpu_numa_node(g_state.device);
        int pes = 1, rank = 0;
        if (node::up()) {
            pes = node::npes();
            for (int q = 0; q < g_state.pe; ++q) rank += node::gpu_numa(q) == mine ? 1 : 0;
        }
        const std::vector<std::vector<int>> domains =
            mine >= 0 ? topo::cache_domains("/sys", node_cpus(mine)) : std::vector<std::vector<int>>{};
        std::vector<std::vector<int>> p = topo::plan_copy_threads(want, budget, pes, rank, domains);
        if (log_enabled(LOG_INFO)) {
            std::string l;
            for (const auto &x : p) l += x.empty() ? "- " : std::to_string(x.front()) + "+" + std::to_string(x.size() - 1) + " ";
            trace(LOG_INFO, "staging copy threads: %zu (CPU budget %d over %d PEs, quota %d; rank %d on NUMA node "
                  "%d of %zu cache domains), first CPU+others of each: %s", p.size(), budget, pes, quota, rank,
                  mine, domains.size(), l.c_str());
        }
        return p;
    }();
    return plan;
}

// memcpy split over the staging budget (copy_threads) from 4 MiB up: the
// caller does piece 0 where it runs, worker i sits on thread i's domain.  A
// caller that finds the workers busy copies alone (CopyGang::copy).
void parallel_copy(void *dst, const void *src, size_t bytes) {
    static CopyGang pool([] {
        std::vector<std::vector<int>> workers = copy_threads();
        if (!workers.empty()) workers.erase(workers.begin());
        return workers;
    }());
    pool.copy(dst, src, bytes);
}

// The staging pipeline's two gangs, made on first use: this PE's copy
// threads (copy_threads) alternate between them, the in gang taking threads
// 0, 2, 4, ... and the out gang 1, 3, 5, ..., so no two share a domain
// while there are domains enough (a gang left without one gets an unpinned
// thread).  Only the out gang, which writes the caller's target, copies with
// streaming stores: its 4 threads copy 94 against 81 GB/s with them in the
// copy lab, and the pipeline averages 36.0 against 34.9 GiB/s over
// interleaved runs, with the smaller dip (profiles/r05_e2e_nt.txt); into the
// ring they lose (30.3 against 36.2: the H2D DMA reads the slot right after).
static CopyGang &gang(int which) {
    static const std::array<std::vector<std::vector<int>>, 2> halves = [] {
        const std::vector<std::vector<int>> &all = copy_threads();
        std::array<std::vector<std::vector<int>>, 2> h;
        for (size_t i = 0; i < all.size(); ++i) h[i % 2].push_back(all[i]);
        for (auto &half : h)
            if (half.empty()) half.emplace_back();
        return h;
    }();
    static CopyGang in(halves[0]), out(halves[1]);
    return which == 0 ? in : out;
}

// The small-message bounce buffers: fine-grained (coherent) page-locked
// memory, so a kernel that reads or writes them in place sees the host's
// bytes and the host sees its stores after the stream wait, with no cached
// copy in any XCD's L2 across calls.
static bool small_bounce_reserve() {
    if (g_state.bounce) return true;
    if (hipHostMalloc(&g_state.bounce, 2 * kSmallHostBytes, hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        g_state.bounce = nullptr;
        g_state.bounce_bytes = 0;
        return false;
    }
    g_state.bounce_bytes = kSmallHostBytes;
    return true;
}

// Every member must issue the same sequence of collective calls, as every PE
// of the reference runs one call sequence (reduce-op.c:213-250).  Device
// arrays reduce in one call; host arrays above kSmallHostBytes in one call
// per staging chunk.  Before a collective call of that size the members
// compare their call counts (one 8-byte exchange); if any differs — one PE
// passed host arrays, another device arrays — every member returns
// SHMEMX_ENOTSUP instead of issuing mismatched collectives.
static bool calls_agree(int start, int logstride, int size, size_t ncalls) {
    std::vector<unsigned long long> all;
    if (exchange_u64(start, logstride, size, ncalls, all)) return false;
    for (unsigned long long v : all) {
        if (v != ncalls) {
            trace(LOG_REDUCTION, "members disagree on the call's chunking (%llu vs %zu calls: host "
                  "and device arrays mixed across PEs): ENOTSUP", v, ncalls);
            set_error(SHMEMX_ENOTSUP);
            return false;
        }
    }
    return true;
}

// Whether a blocking call of `bytes` per PE over several PEs takes the
// exchange: every member decides alike (the same size and settings;
// g_state.xchg was agreed at init).
static bool xchg_eligible(size_t bytes) {
    return bytes <= node::kXchgSlotBytes && g_state.xchg && g_state.algo == SHMEMX_ALGO_AUTO &&
           !g_state.force_collective && service_available();
}

// One blocking call on its way down the paths below: reduce_blocking fills in
// the arguments (operands of the mirrored heap's host view replaced by their
// HBM twins) and what the mirrored heap asks of the call; run_blocking adds
// the rest.
struct BlockingCall {
    int type, op;
    void *target;
    const void *source;
    int nreduce, start, logstride, size;
    size_t bytes = 0;
    bool tdev = false, sdev = false;   // the operands are device-accessible
    shmemx_plan_t plan{};
    // A small host-view target: the device address where the call's last
    // kernel also stores the result (the view's page-locked alias, heap.h
    // DeviceWrite::settle_dst), and whether it did, before the host signal.
    void *settle_dst = nullptr;
    bool settled = false;
    // a host-view source's current bytes, for the exchange (its HBM twin is
    // not flushed)
    const void *xchg_src_host = nullptr;

    size_t n() const { return (size_t)nreduce; }
    bool collective() const { return size > 1 || g_state.force_collective; }
};

// The two small-message bounce buffers (small_bounce_reserve): in, out.
struct Bounce {
    char *in, *out;
};
static Bounce bounce_halves() {
    char *b = static_cast<char *>(g_state.bounce);
    return {b, b + kSmallHostBytes};
}

// The wait that ends a call: for the host signal of its last kernel on the
// library stream, which stored `stored` (or null) as well; no stream wait.
static void wait_on_signal(BlockingCall &c, const HostSignal &sig, const void *stored) {
    wait_host_signal(sig, g_state.stream);
    if (stored && stored == c.settle_dst) c.settled = true;
}

// The last kernel of a call and the wait for it: a one-input fold (a copy)
// of copy_src into copy_dst whose one workgroup then signals the host, or,
// without a copy_dst, a marker.
static void finish_on_signal(BlockingCall &c, void *copy_dst, const void *copy_src) {
    const HostSignal sig = next_host_signal();
    if (copy_dst) {
        const void *in[1] = {copy_src};
        SHMX_HIP(launch_fold_signal(c.type, c.op, copy_dst, in, 1, c.n(), g_state.stream, sig));
    } else {
        SHMX_HIP(launch_host_signal(sig, g_state.stream));
    }
    wait_on_signal(c, sig, copy_dst);
}

// After the engine (reduce_device, result rc) and the wait for its work: a
// failed call waited for nothing, so the stream is drained here; then the
// device barriers' error word is read.
static void engine_done(int rc) {
    if (rc != SHMEMX_OK) SHMX_HIP(hipStreamSynchronize(g_state.stream));
    check_signal_error("SIGNAL reduction");
}

// A small blocking call over several PEs (<= 4 KiB per PE): the reference's
// barrier, gets and barrier (reduce-op.c:217-250) with the gets and the fold
// done by each member's resident service workgroup (service.hip), no kernel
// launch.  Each member leaves its source in its slot of the job's page-locked
// exchange (node.h; a device source by a service copy, a host one by the
// CPU), passes the entry barrier, has its workgroup fold every member's slot
// (its own order for the pairs where the order decides the answer, else
// PE_start's, as DIRECT and A2A do) into its target (a host target through
// the bounce buffer), and marks itself done with every member's slot; a
// member writes its slot again only once the readers of its previous call
// are done (node::xchg_claim), which takes the place of the reference's exit
// barrier.  Host memory is the meeting point, so no GPU reads
// another GPU's memory and no L2 write-back beyond each workgroup's own
// system-scope release is needed.
static void xchg_reduce(BlockingCall &c) {
    const int step = 1 << c.logstride;
    const bool own_order = own_order_pair(c.type, c.op);
    if (log_enabled(LOG_REDUCTION))
        trace(LOG_REDUCTION, "type %d op %d nreduce %zu set (%d,%d,%d) algo service exchange%s", c.type, c.op,
              c.n(), c.start, c.logstride, c.size, own_order ? " (own order)" : "");
    if (!c.tdev && !small_bounce_reserve())
        fatal("small multi-PE call", "no page-locked bounce buffer for a host target");
    uint64_t counts[node::kMaxPes];
    node::xchg_claim(c.start, step, c.size, counts);   // the slot is free again
    if (c.xchg_src_host) {   // a mirrored-heap source's current view bytes
        std::memcpy(node::xchg_host(g_state.pe), c.xchg_src_host, c.bytes);
    } else if (c.sdev) {
        if (!service_copy(node::xchg_dev(g_state.pe), nullptr, c.source, c.bytes))
            fatal("small multi-PE call", "the service workgroup did not take the source");
    } else {
        std::memcpy(node::xchg_host(g_state.pe), c.source, c.bytes);
    }
    node::barrier(c.start, step, c.size);
    char *bout = bounce_halves().out;
    void *dst2 = c.tdev ? c.settle_dst : nullptr;
    service_fold(c.type, c.op, own_order, c.start, c.logstride, c.size, c.tdev ? c.target : bout, dst2, c.bytes);
    node::xchg_finish(c.start, step, c.size, counts);   // (no exit barrier: xchg_claim)
    if (dst2) c.settled = true;
    if (!c.tdev) std::memcpy(c.target, bout, c.bytes);
}

// Device-accessible operands: a one-member set is a copy; everything else is
// the engine's.
static void device_operands(BlockingCall &c) {
    hipStream_t s = g_state.stream;
    if (c.collective() && c.bytes > kSmallHostBytes && !calls_agree(c.start, c.logstride, c.size, 1)) return;
    if (c.plan.nmembers == 1 && !c.collective() && !overlap(c.target, c.source, c.bytes)) {
        // a one-member set is a copy (reduce-op.c:213-216): up to 32 KiB by
        // the resident service workgroup when the streams it is ordered
        // after are idle (no launch; service.hip), else the copy kernel,
        // which tells the host itself when it is done (one workgroup; a
        // marker kernel otherwise): no stream wait either way
        if (c.bytes <= kServiceMaxBytes && service_copy(c.target, c.settle_dst, c.source, c.bytes)) {
            if (c.settle_dst) c.settled = true;
        } else if (c.settle_dst) {
            // a small mirrored target: one copy kernel stores the result
            // into HBM and into the view's alias, and its workgroup signals
            const HostSignal sig = next_host_signal();
            SHMX_HIP(launch_copy2_signal(c.type, c.target, c.settle_dst, c.source, c.n(), s, sig));
            wait_on_signal(c, sig, c.settle_dst);
        } else {
            finish_on_signal(c, c.target, c.source);
        }
        return;
    }
    const int rc = reduce_device(c.type, c.op, c.target, c.source, c.nreduce, c.start, c.logstride, c.size,
                                 g_state.algo, s);
    // DIRECT and own-order GATHER over IPC return with their work done
    // (host barriers, or the fused launch's host signal): no stream wait
    // on top — a hipStreamSynchronize entered while a kernel is still
    // retiring costs ~9 us more than the kernel's remaining time
    // (profiles/r03_latency_ab.txt).  The stream-ordered algorithms end
    // with a marker the host spins on; a small mirrored target with its
    // result going into the view's alias, by the one workgroup that then
    // signals.
    const bool waits_itself = c.collective() && pulls_over_ipc(c.plan);
    if (rc == SHMEMX_OK && (!waits_itself || c.settle_dst)) finish_on_signal(c, c.settle_dst, c.target);
    engine_done(rc);
}

// A small host PE_size 1 call is a copy (reduce-op.c:213-216).  The copy
// kernel reads and writes the page-locked bounce buffers in place over PCIe
// (zero-copy): one launch and one wait, no DMA commands.
static void small_host_copy(BlockingCall &c) {
    const Bounce b = bounce_halves();
    if (!c.sdev) std::memcpy(b.in, c.source, c.bytes);
    void *t = c.tdev ? c.target : b.out;
    const void *in = c.sdev ? c.source : b.in;
    if (overlap(t, in, c.bytes)) {
        const int rc = reduce_device(c.type, c.op, t, in, c.nreduce, c.start, c.logstride, c.size, g_state.algo,
                                     g_state.stream);
        SHMX_HIP(hipStreamSynchronize(g_state.stream));
        if (!rc && !c.tdev) std::memcpy(c.target, b.out, c.bytes);
        return;
    }
    // the service workgroup (service.hip), or the copy kernel, which
    // signals the host when its stores have landed
    if (!(c.bytes <= kServiceMaxBytes && service_copy(t, nullptr, in, c.bytes))) finish_on_signal(c, t, in);
    if (!c.tdev) std::memcpy(c.target, b.out, c.bytes);
}

// The device staging buffers of host operands, grow-only; false: ENOMEM.
static bool stage_reserve(size_t bytes) {
    if (bytes <= g_state.stage_bytes) return true;
    device_sync();
    if (g_state.stage_src) SHMX_HIP(hipFree(g_state.stage_src));
    if (g_state.stage_tgt) SHMX_HIP(hipFree(g_state.stage_tgt));
    g_state.stage_src = g_state.stage_tgt = nullptr;
    g_state.stage_bytes = 0;
    if (hipMalloc(&g_state.stage_src, bytes) != hipSuccess || hipMalloc(&g_state.stage_tgt, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error(SHMEMX_ENOMEM);
        return false;
    }
    g_state.stage_bytes = bytes;
    return true;
}

// Small host messages over several PEs (the ISx nreduce = 1 case,
// isx.c:617): latency, not bandwidth.  Bounce through the page-locked
// buffers; copy kernels on the library stream move them to and from the
// device (no DMA command: 25 vs 33 us per call at 32 KiB,
// profiles/archive/r01_host_latency.txt), and the host waits once.
static void small_host_collective(BlockingCall &c) {
    hipStream_t s = g_state.stream;
    const Bounce b = bounce_halves();
    // DIRECT and own-order GATHER over IPC take the bounce buffers
    // themselves (page-locked, device-accessible): the source goes
    // straight into the IPC scratch the peers read, the fold writes the
    // result into the out buffer over PCIe, and the call returns with its
    // work done, so the copy kernels on either side and the extra wait go.
    // RCCL's algorithms need device memory: they keep the staging copies.
    const bool pulls = c.collective() && pulls_over_ipc(c.plan);
    const void *dsrc = c.source;
    if (!c.sdev) {
        std::memcpy(b.in, c.source, c.bytes);
        if (pulls) {
            dsrc = b.in;
        } else {
            const void *in[1] = {b.in};
            fold_chain(c.type, c.op, g_state.stage_src, in, 1, c.n(), s);
            dsrc = g_state.stage_src;
        }
    }
    void *dtgt = c.tdev ? c.target : pulls ? static_cast<void *>(b.out) : g_state.stage_tgt;
    const int rc = reduce_device(c.type, c.op, dtgt, dsrc, c.nreduce, c.start, c.logstride, c.size, g_state.algo, s);
    // the pulls returned with the result in place (host barriers, or the
    // fused launch's host signal); otherwise the last copy (or a marker)
    // signals the host: no stream wait
    if (!rc && !pulls) finish_on_signal(c, c.tdev ? nullptr : b.out, dtgt);
    engine_done(rc);
    if (!rc && !c.tdev) std::memcpy(c.target, b.out, c.bytes);
}

// Host-resident symmetric arrays (the reference's heap) above
// kSmallHostBytes: staged over PCIe in chunks, H2D on one copy stream, the
// reduction on the library stream, D2H on a second copy stream, so the two
// PCIe directions and the device work overlap.  Every PE cuts the same
// chunks, so the collective sequence matches across PEs (calls_agree checks
// it).
static void host_pipeline(BlockingCall &c) {
    hipStream_t s = g_state.stream;
    if (!g_state.h2d) {
        SHMX_HIP(hipStreamCreateWithFlags(&g_state.h2d, hipStreamNonBlocking));
        SHMX_HIP(hipStreamCreateWithFlags(&g_state.d2h, hipStreamNonBlocking));
    }
    const size_t sz = type_size(c.type);
    const size_t g = granule(sz);
    static const size_t stage_chunk = [] {
        const char *e = std::getenv("SHMEMX_STAGE_CHUNK_MB");
        const int mb = e ? std::atoi(e) : 0;
        return mb > 0 ? size_t(mb) << 20 : kStageChunkBytes;
    }();
    size_t chunk = ((stage_chunk / sz) / g) * g;
    if (chunk == 0) chunk = g;
    // a host target that partially overlaps the host source would be
    // overwritten under a later chunk's H2D: no pipelining then
    const bool host_overlap = !c.tdev && !c.sdev && overlap(c.target, c.source, c.bytes);
    if (host_overlap) chunk = c.n();
    // The chunk schedule (elements, stage_plan.h: quarter and half chunks at
    // both ends, +1.1 %, profiles/r05_e2e_ramp.txt), the same on every PE
    // (calls_agree compares its length).
    std::vector<size_t> c_off, c_n;
    stage_plan(c.n(), chunk, g, !host_overlap, c_off, c_n);
    const size_t nchunks = c_n.size();
    if (c.collective() && !calls_agree(c.start, c.logstride, c.size, nchunks)) return;
    // How each end reaches the device: directly (device memory), by DMA
    // (page-locked host memory), or through the page-locked bounce ring
    // (pageable memory: CPU copy by a gang, then DMA).
    const bool in_bounce = !c.sdev && !host_pinned(c.source) && !host_overlap;
    const bool out_bounce = !c.tdev && !host_pinned(c.target) && !host_overlap;
    if ((in_bounce || out_bounce) && !ring_reserve(chunk * sz)) {
        set_error(SHMEMX_ENOMEM);
        return;
    }
    while (g_state.events.size() < 2 * nchunks + 2 * kRingSlots) {
        hipEvent_t e;
        SHMX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        g_state.events.push_back(e);
    }
    hipEvent_t *ev_chunk = g_state.events.data();             // 2 per chunk
    hipEvent_t *ev_in_slot = ev_chunk + 2 * nchunks;          // ring slot free again
    hipEvent_t *ev_out_slot = ev_in_slot + kRingSlots;        // ring slot filled
    char *hsrc = static_cast<char *>(const_cast<void *>(c.source));
    char *htgt = static_cast<char *>(c.target);
    char *ssrc = static_cast<char *>(g_state.stage_src);
    char *stgt = static_cast<char *>(g_state.stage_tgt);
    // Pageable ends run through the ring with two CPU gangs working at once
    // (bounce in: source -> ring_in[k % kRingSlots], read by the H2D of chunk
    // k; bounce out: ring_out[k % kRingSlots], written by the D2H of chunk k,
    // -> target), so the CPU copies in and out overlap each other and the
    // DMA and the fold of the chunks between them.  Slot reuse: the in-copy
    // of chunk k waits for the H2D of chunk k - kRingSlots (event), the D2H of
    // chunk k for the out-copy of chunk k - kRingSlots (host side).
    auto start_in = [&](size_t k) {
        const size_t slot = k % kRingSlots;
        if (k >= kRingSlots) SHMX_HIP(hipEventSynchronize(ev_in_slot[slot]));
        gang(0).start(ring_in(slot), hsrc + c_off[k] * sz, c_n[k] * sz, false);
    };
    size_t out_started = 0;   // out-copies started; all but the last are complete
    auto start_out = [&]() {
        const size_t j = out_started++;
        SHMX_HIP(hipEventSynchronize(ev_out_slot[j % kRingSlots]));
        gang(1).start(htgt + c_off[j] * sz, ring_out(j % kRingSlots), c_n[j] * sz, true);   // streaming stores
    };
    // the out-copy of chunk j has completed (starting the ones before it)
    auto out_done = [&](size_t j) {
        while (out_started <= j) start_out();
        gang(1).wait();
    };
    int rc = SHMEMX_OK;
    if (in_bounce && nchunks) start_in(0);
    for (size_t k = 0; k < nchunks && !rc; ++k) {
        const size_t off = c_off[k] * sz;
        const size_t b = c_n[k] * sz;
        const size_t slot = k % kRingSlots;
        const void *dsrc = hsrc + off;
        if (!c.sdev) {
            const char *from = hsrc + off;
            if (in_bounce) {
                gang(0).wait();              // chunk k is in its ring slot
                from = ring_in(slot);
            }
            SHMX_HIP(hipMemcpyAsync(ssrc + off, from, b, hipMemcpyHostToDevice, g_state.h2d));
            SHMX_HIP(hipEventRecord(ev_chunk[2 * k], g_state.h2d));
            if (in_bounce) SHMX_HIP(hipEventRecord(ev_in_slot[slot], g_state.h2d));
            SHMX_HIP(hipStreamWaitEvent(s, ev_chunk[2 * k], 0));
            dsrc = ssrc + off;
            if (in_bounce && k + 1 < nchunks) start_in(k + 1);   // runs while this chunk moves
        }
        void *dtgt = c.tdev ? static_cast<void *>(htgt + off) : static_cast<void *>(stgt + off);
        rc = reduce_device(c.type, c.op, dtgt, dsrc, (int)c_n[k], c.start, c.logstride, c.size, g_state.algo, s);
        if (!rc && !c.tdev) {
            SHMX_HIP(hipEventRecord(ev_chunk[2 * k + 1], s));
            SHMX_HIP(hipStreamWaitEvent(g_state.d2h, ev_chunk[2 * k + 1], 0));
            if (out_bounce) {
                if (k >= kRingSlots) out_done(k - kRingSlots);   // the slot's previous chunk is out
                SHMX_HIP(hipMemcpyAsync(ring_out(slot), dtgt, b, hipMemcpyDeviceToHost, g_state.d2h));
                SHMX_HIP(hipEventRecord(ev_out_slot[slot], g_state.d2h));
                // keep the out gang on the oldest chunk whose D2H is enqueued
                // one behind, so this thread is free to enqueue the next one
                if (k >= 1 && out_started < k) {
                    gang(1).wait();
                    start_out();
                }
            } else {
                SHMX_HIP(hipMemcpyAsync(htgt + off, dtgt, b, hipMemcpyDeviceToHost, g_state.d2h));
            }
        }
    }
    if (in_bounce) gang(0).wait();          // no copy still writes the ring
    if (out_bounce && !rc && nchunks) out_done(nchunks - 1);
    if (out_bounce) gang(1).wait();
    SHMX_HIP(hipStreamSynchronize(g_state.h2d));
    SHMX_HIP(hipStreamSynchronize(s));
    SHMX_HIP(hipStreamSynchronize(g_state.d2h));
}

// Checks the call, plans it and sends it down its path.  trace_call: the
// operands are the caller's own addresses (reduce-op.c:199-210's trace line).
static void run_blocking(BlockingCall &c, bool trace_call) {
    if (ensure_init()) {
        trace(LOG_FATAL, "reduction called before shmem_init with npes > 1");
        return;
    }
    if (!op_on_device(c.type, c.op)) {
        set_error(op_valid(c.type, c.op) ? SHMEMX_ENOTSUP : SHMEMX_EINVAL);
        return;
    }
    if (c.nreduce < 0 || (c.nreduce > 0 && (!c.target || !c.source))) {
        set_error(SHMEMX_EINVAL);
        return;
    }
    // (n == 0: nothing moves, but the plan validates membership like a call would)
    const int rc = make_plan(c.type, c.op, c.nreduce, c.start, c.logstride, c.size, g_state.pe, g_state.npes,
                             g_state.algo, &c.plan);
    if (rc) {
        set_error(rc);
        return;
    }
    c.bytes = type_size(c.type) * c.n();
    if (trace_call) trace_reference_overlap(c.target, c.source, c.bytes);   // the caller's arrays
    if (c.nreduce == 0) return;
    // (the small-message bounce buffer is mapped into the GPU: a source
    // staged there by the mirrored heap's PE_size 1 light path is read in place)
    c.tdev = device_accessible(c.target);
    c.sdev = (c.source == g_state.bounce && g_state.bounce) || device_accessible(c.source);
    // A small call over several PEs under auto: through the exchange and the
    // service workgroups (xchg_reduce).
    if (c.size > 1 && xchg_eligible(c.bytes)) return xchg_reduce(c);
    if (c.tdev && c.sdev) return device_operands(c);
    if (c.bytes <= kSmallHostBytes) {
        if (!small_bounce_reserve()) {
            set_error(SHMEMX_ENOMEM);
            return;
        }
        if (c.plan.nmembers == 1 && !g_state.force_collective) return small_host_copy(c);
    }
    if (!stage_reserve(c.bytes)) return;
    if (c.bytes <= kSmallHostBytes) return small_host_collective(c);
    host_pipeline(c);
}

// The blocking entry point body: host- or device-resident arrays.  Operands
// in the mirrored heap's host view run on their HBM twins (heap.h).
void reduce_blocking(int type, int op, void *target, const void *source,
                     int nreduce, int start, int logstride, int size) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    clear_error();
    // a blocking call returns as soon as its work's host signal arrives
    struct Early {
        Early() { g_state.return_on_signal = true; }
        ~Early() { g_state.return_on_signal = false; }
    } early;
    BlockingCall c{type, op, target, source, nreduce, start, logstride, size};
    const size_t sz = type_size(type);
    if (!(nreduce > 0 && sz && target && source && op_valid(type, op) &&
          (heap::twin(target) != target || heap::twin(source) != source)))
        return run_blocking(c, true);
    const size_t bytes = sz * (size_t)nreduce;
    // the host's stores to the operands' blocks go up on the library
    // stream, ahead of the call's own work there: no host wait for
    // them (the DIRECT / SIGNAL peers read this PE's HBM only after a
    // barrier that waits for the stream, or in stream order)
    heap::SameStreamFlush same_stream;
    // Small operands whose result one workgroup can also store into
    // the view's alias (the ISx nreduce = 1 use) take the light path:
    // only the source's own host-written bytes go up, and no block
    // changes state or protection (mirror.h begin_light_write), so
    // the host's next store into those blocks takes no fault either
    void *adst = bytes <= kSmallHostBytes ? heap::alias_device(target, bytes) : nullptr;
    const bool light = adst && heap::twin(target) != target && heap::twin(source) != source &&
                       copy_one_workgroup(type, adst, heap::twin(target), (size_t)nreduce);
    // PE_size 1 (a copy, reduce-op.c:213-216) on the light path, with
    // the source's view bytes current: they go through the coherent
    // bounce buffer (a CPU copy, as small host arrays do) and the copy
    // kernel reads them there, instead of a DMA to the source's HBM
    // twin first (its blocks keep their state: a HOST_NEWER block is
    // flushed whole by the next call that needs it in HBM).  ISx's
    // nreduce = 1 round: profiles/r05_isx_mirror.txt.
    // A small call over several PEs through the exchange (xchg_reduce)
    // on the same terms: the view's current bytes go into this PE's
    // exchange slot by a CPU copy, and the source's HBM twin, neither
    // flushed nor read, keeps its blocks' state.
    const bool xchg = size > 1 && xchg_eligible(bytes);
    const void *cur = light && (size == 1 || xchg) && !g_state.force_collective && bytes <= kSmallHostBytes
                          ? heap::current_host_bytes(source, bytes) : nullptr;
    if (cur && size == 1 && small_bounce_reserve()) {
        std::memcpy(g_state.bounce, cur, bytes);
        c.source = g_state.bounce;
    } else if (cur && xchg) {
        c.xchg_src_host = cur;
        c.source = heap::twin(source);
    } else {
        c.source = light ? heap::device_operand_bytes(source, bytes) : heap::device_operand(source, bytes);
    }
    trace_reference_overlap(target, source, bytes);   // the caller's addresses
    // blocks of a host-view target: DEVICE_NEWER from before the call
    // (host accesses wait for it), or on the light path unchanged; the
    // blocking call completes on the library stream, its recorded writer
    heap::DeviceWrite t(target, bytes, g_state.stream, light);
    c.target = t.ptr();
    // A result of up to kSmallHostBytes (the bounce path's size) is back in
    // the view before the call returns, its blocks CLEAN (ISx's round 42.8 ->
    // 30.1 us, the host load 19.9 -> 0.26 us: profiles/r04_isx_mirror.txt).
    // It also goes straight into the view's page-locked alias: the call's
    // last kernel stores it there before the host signal (one workgroup, so
    // its own drained stores and system-scope release precede the signal)
    c.settle_dst = t.settle_dst(kSmallHostBytes);
    if (c.settle_dst && !copy_one_workgroup(type, c.settle_dst, t.ptr(), (size_t)nreduce)) c.settle_dst = nullptr;
    run_blocking(c, false);
    // the call's work is complete: a small result is back in the view
    // (copied above, or now), so the caller's system calls can read
    // it (larger targets are fetched on first access).
    // A call that failed wrote no target: on the light path the view
    // already holds the target's bytes, and HBM may not (a
    // host-written target block is not flushed there), so nothing is
    // copied back
    const bool failed = shmemx_reduce_last_error() != SHMEMX_OK;
    // A call that failed before its own work (a bad set, a call-count
    // mismatch) never waited for the library stream, where the flush
    // of the host's bytes (SameStreamFlush) may still be in flight:
    // settle()'s copy-back, and the next call on another stream, must
    // not read HBM before it has landed
    if (failed) SHMX_HIP(hipStreamSynchronize(g_state.stream));
    // every blocking call returns with its work complete: no writer
    // event on the library stream (it would keep the stream busy for
    // the next call's service check, service.hip)
    t.completed();
    t.settle(kSmallHostBytes, c.settled || (failed && t.light()));
}

}  // namespace shmx
