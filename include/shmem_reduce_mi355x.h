/*
 * shmem_reduce_mi355x.h — C ABI of the MI355X-native OpenSHMEM reduction
 * collectives (libshmem_reduce_mi355x.so).
 *
 * Part 1 declares, with the reference's exact prototypes, the 44
 * shmem_<TYPE>_<OP>_to_all entry points that replace
 * /root/reference/src/reduce/reduce-op.c:372-431 (declared in the reference at
 * src/shmem.h:1412-1648, profiling names src/pshmem.h:328-526).  As with the
 * reference built --enable-pshmem (reduce-op.c:275-364), every pshmem_* name is
 * the strong symbol and every shmem_* name a weak alias of it, so profilers
 * (TAU and friends) can still interpose.
 *
 * Part 2 is the minimum runtime the path needs: the PE identity that
 * GET_STATE(mype)/shmem_my_pe() give the reference (utils/state.h,
 * updown/updown.c:131-184), here one PE = one process = one MI355X.
 *
 * Part 3 holds extensions (shmemx_*): stream-ordered (graph-capturable)
 * forms of the reduction, the local fold kernel on its own, the algorithm
 * selector, the exchange plan query and error reporting.
 *
 * Semantics kept from the reference (see DESIGN.md "Boundary"):
 *   - blocking collective over the active set PE_start + i*2^logPE_stride,
 *     i < PE_size; every member calls with the same arguments;
 *   - target/source may be host memory (as the reference's symmetric heap,
 *     memory/symmem.c:168-227) or device memory; they may be the same array;
 *   - pWrk is accepted and never touched; pSync is never written (so it stays
 *     all SHMEM_SYNC_VALUE, the state barrier-linear.c:75 restores);
 *   - no return value.  Bad arguments (nreduce < 0, caller not in the active
 *     set, ...) leave target untouched and set shmemx_reduce_last_error();
 *     HIP/RCCL failures print a FATAL line and abort, like the reference's
 *     shmemi_trace(SHMEM_LOG_FATAL) (utils/trace.c:424-427).
 */
#ifndef SHMEM_REDUCE_MI355X_H
#define SHMEM_REDUCE_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
#include <complex>
#define SHMEMX_COMPLEX(T) std::complex<T>
extern "C" {
#else
#include <complex.h>
#define SHMEMX_COMPLEX(T) T complex
#endif

/* Constants as the reference defines them on LP64 (shmem.h:1400-1410). */
#ifndef SHMEM_REDUCE_SYNC_SIZE
#define SHMEM_REDUCE_SYNC_SIZE        128L
#define SHMEM_REDUCE_MIN_WRKDATA_SIZE 64L
#define SHMEM_SYNC_VALUE              (-1L)
#endif

/* ------------------------------------------------------------------------ */
/* Part 1: the 44 reduction entry points (shmem.h:1412-1648).               */

#define SHMEMX_DECL_REDUCE(Name, Op, T)                                        \
    void shmem_##Name##_##Op##_to_all(T *target, T *source, int nreduce,     \
                                      int PE_start, int logPE_stride,        \
                                      int PE_size, T *pWrk, long *pSync);    \
    void pshmem_##Name##_##Op##_to_all(T *target, T *source, int nreduce,    \
                                       int PE_start, int logPE_stride,       \
                                       int PE_size, T *pWrk, long *pSync);

#define SHMEMX_DECL_ARITH(Name, T) \
    SHMEMX_DECL_REDUCE(Name, sum, T) SHMEMX_DECL_REDUCE(Name, prod, T)
#define SHMEMX_DECL_LOGIC(Name, T)                                             \
    SHMEMX_DECL_REDUCE(Name, and, T) SHMEMX_DECL_REDUCE(Name, or, T)         \
    SHMEMX_DECL_REDUCE(Name, xor, T)
#define SHMEMX_DECL_MINMAX(Name, T) \
    SHMEMX_DECL_REDUCE(Name, min, T) SHMEMX_DECL_REDUCE(Name, max, T)

/* sum/prod: 9 types (reduce-op.c:388-405) */
SHMEMX_DECL_ARITH(short, short)
SHMEMX_DECL_ARITH(int, int)
SHMEMX_DECL_ARITH(long, long)
SHMEMX_DECL_ARITH(longlong, long long)
SHMEMX_DECL_ARITH(float, float)
SHMEMX_DECL_ARITH(double, double)
SHMEMX_DECL_ARITH(longdouble, long double)
SHMEMX_DECL_ARITH(complexd, SHMEMX_COMPLEX(double))
SHMEMX_DECL_ARITH(complexf, SHMEMX_COMPLEX(float))
/* and/or/xor: 4 integer types (reduce-op.c:406-417) */
SHMEMX_DECL_LOGIC(short, short)
SHMEMX_DECL_LOGIC(int, int)
SHMEMX_DECL_LOGIC(long, long)
SHMEMX_DECL_LOGIC(longlong, long long)
/* min/max: 7 real types (reduce-op.c:418-431) */
SHMEMX_DECL_MINMAX(short, short)
SHMEMX_DECL_MINMAX(int, int)
SHMEMX_DECL_MINMAX(long, long)
SHMEMX_DECL_MINMAX(longlong, long long)
SHMEMX_DECL_MINMAX(float, float)
SHMEMX_DECL_MINMAX(double, double)
SHMEMX_DECL_MINMAX(longdouble, long double)

/* Fortran bindings (reference src/fortran/fortran.c:1003-1054, gfortran
 * name mangling FORTRANIFY(sym) = sym##_): arguments by reference, pSync an
 * INTEGER array; each forwards to the C routine above. */
#define SHMEMX_DECL_FORTRAN(Fname, Op, T)                                      \
    void shmem_##Fname##_##Op##_to_all_(T *target, T *source, int *nreduce,  \
                                        int *PE_start, int *logPE_stride,    \
                                        int *PE_size, T *pWrk, int *pSync);  \
    void pshmem_##Fname##_##Op##_to_all_(T *target, T *source, int *nreduce, \
                                         int *PE_start, int *logPE_stride,   \
                                         int *PE_size, T *pWrk, int *pSync);
#define SHMEMX_DECL_FORTRAN_REAL(Op)                                           \
    SHMEMX_DECL_FORTRAN(int2, Op, short) SHMEMX_DECL_FORTRAN(int4, Op, int)  \
    SHMEMX_DECL_FORTRAN(int8, Op, long) SHMEMX_DECL_FORTRAN(real4, Op, float)\
    SHMEMX_DECL_FORTRAN(real8, Op, double)                                   \
    SHMEMX_DECL_FORTRAN(real16, Op, long double)
#define SHMEMX_DECL_FORTRAN_INT(Op)                                            \
    SHMEMX_DECL_FORTRAN(int2, Op, short) SHMEMX_DECL_FORTRAN(int4, Op, int)  \
    SHMEMX_DECL_FORTRAN(int8, Op, long)
SHMEMX_DECL_FORTRAN_REAL(sum)
SHMEMX_DECL_FORTRAN_REAL(prod)
SHMEMX_DECL_FORTRAN_REAL(max)
SHMEMX_DECL_FORTRAN_REAL(min)
SHMEMX_DECL_FORTRAN_INT(and)
SHMEMX_DECL_FORTRAN_INT(or)
SHMEMX_DECL_FORTRAN_INT(xor)
SHMEMX_DECL_FORTRAN(comp4, sum, SHMEMX_COMPLEX(float))
SHMEMX_DECL_FORTRAN(comp8, sum, SHMEMX_COMPLEX(double))
SHMEMX_DECL_FORTRAN(comp4, prod, SHMEMX_COMPLEX(float))
SHMEMX_DECL_FORTRAN(comp8, prod, SHMEMX_COMPLEX(double))

/* ------------------------------------------------------------------------ */
/* Part 2: runtime (replaces shmem_init updown.c:160, shmem_my_pe/n_pes).   */

/* Bootstrap from the environment: PE = $SHMEM_PE or $RANK, npes =
 * $SHMEM_NPES or $WORLD_SIZE (default 1), device = $LOCAL_RANK or PE mod the
 * visible device count.  With npes > 1 the RCCL unique id is exchanged through
 * the file $SHMEM_BOOTSTRAP_FILE (PE 0 writes it, the others wait for it);
 * launchers that have their own channel should call shmemx_init_attr(). */
void shmem_init(void);
void shmem_finalize(void);
int shmem_my_pe(void);
int shmem_n_pes(void);
void pshmem_init(void);
void pshmem_finalize(void);
int pshmem_my_pe(void);
int pshmem_n_pes(void);

/* ------------------------------------------------------------------------ */
/* Part 2b: the collectives next to the reductions and the symmetric heap   */
/* (SURVEY.md §8f).  Reference prototypes: shmem.h:595-651 (barrier),       */
/* :1654-1684 (broadcast, [f]collect), :821-941 (symmetric heap).  The heap */
/* is one HBM segment per PE; by default shmem_malloc returns addresses in  */
/* a host view of it (the mirrored heap, below), so host code dereferences  */
/* symmetric objects as with the reference's host heap while collectives    */
/* run on HBM.  $SHMEMX_HEAP_MEMORY=device returns the HBM addresses        */
/* themselves (for programs whose own kernels use them); =host makes the    */
/* heap page-locked host memory.                                            */

#ifndef SHMEM_BCAST_SYNC_SIZE
#define SHMEM_BCAST_SYNC_SIZE   64L
#define SHMEM_BARRIER_SYNC_SIZE 64L
#define SHMEM_COLLECT_SYNC_SIZE 64L
#endif

#define SHMEMX_DECL_BOTH(ret, name, args) ret name args; ret p##name args;
SHMEMX_DECL_BOTH(void, shmem_barrier, (int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void, shmem_barrier_all, (void))
SHMEMX_DECL_BOTH(void, shmem_broadcast32, (void *target, const void *source, size_t nelems,
                 int PE_root, int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void, shmem_broadcast64, (void *target, const void *source, size_t nelems,
                 int PE_root, int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void, shmem_fcollect32, (void *target, const void *source, size_t nelems,
                 int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void, shmem_fcollect64, (void *target, const void *source, size_t nelems,
                 int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void, shmem_collect32, (void *target, const void *source, size_t nelems,
                 int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void, shmem_collect64, (void *target, const void *source, size_t nelems,
                 int PE_start, int logPE_stride, int PE_size, long *pSync))
SHMEMX_DECL_BOTH(void *, shmem_malloc, (size_t size))
SHMEMX_DECL_BOTH(void *, shmem_align, (size_t alignment, size_t size))
SHMEMX_DECL_BOTH(void, shmem_free, (void *ptr))
SHMEMX_DECL_BOTH(void *, shmem_realloc, (void *ptr, size_t size))
SHMEMX_DECL_BOTH(void *, shmalloc, (size_t size))
SHMEMX_DECL_BOTH(void, shfree, (void *ptr))
SHMEMX_DECL_BOTH(void *, shrealloc, (void *ptr, size_t size))
SHMEMX_DECL_BOTH(void *, shmemalign, (size_t alignment, size_t size))

/* ------------------------------------------------------------------------ */
/* Part 3: extensions.                                                      */

/* Type and op codes. */
enum {
    SHMEMX_TYPE_SHORT = 0, SHMEMX_TYPE_INT, SHMEMX_TYPE_LONG,
    SHMEMX_TYPE_LONGLONG, SHMEMX_TYPE_FLOAT, SHMEMX_TYPE_DOUBLE,
    SHMEMX_TYPE_LONGDOUBLE, SHMEMX_TYPE_COMPLEXD, SHMEMX_TYPE_COMPLEXF,
    SHMEMX_NTYPES
};
enum {
    SHMEMX_OP_SUM = 0, SHMEMX_OP_PROD, SHMEMX_OP_AND, SHMEMX_OP_OR,
    SHMEMX_OP_XOR, SHMEMX_OP_MIN, SHMEMX_OP_MAX, SHMEMX_NOPS
};

/* Exchange algorithms (DESIGN.md "Multi-GPU").
 *   AUTO    on the whole job RCCL (ALLREDUCE up to 4 MiB) for what RCCL
 *           reduces exactly as specified, A2A otherwise; a partial set takes
 *           A2A ($SHMEMX_AUTO_PARTIAL may name rccl / allreduce: the set's own
 *           communicator, so far run against the RCCL test double only);
 *           float / double / long double min and max take GATHER (below)
 *   RCCL    ncclReduceScatter + ncclAllGather (+ ncclAllReduce on the
 *           <P*16-byte tail); RCCL-native type/op only; the whole job on the
 *           world communicator, a partial set on its own members-only
 *           communicator (made at the set's first RCCL call, cached)
 *   A2A     shard exchange (grouped ncclSend/ncclRecv) -> HIP fold of the P
 *           shards in active-set order -> shard all-gather; any set, any op;
 *           every PE gets the reference's PE_start result bit for bit
 *   GATHER  every PE receives every source and folds in its own reference
 *           order: bit-exact with the reference on EVERY PE, (P-1)x traffic
 *   ALLREDUCE  one ncclAllReduce (RCCL-native pairs, any set, as RCCL)
 *   DIRECT  one HIP kernel per PE reads slice m of every member's source
 *           straight from the peers' HBM (IPC-mapped symmetric heap, over
 *           xGMI) and folds it in active-set order into its own target; a
 *           second kernel pulls the other members' result slices.  Host
 *           barriers around and between (the reference's two plus one).
 *           Any set of <= 16 PEs, any op, PE_start bits on every PE.
 *           Operands outside the symmetric heap are staged through an IPC
 *           scratch region.  Host-synchronous.  Arrays up to 256 KiB
 *           ($SHMEMX_DIRECT_ONESHOT_KB) take one shot: every PE folds the
 *           whole array, as one fused launch (fence, device barriers and
 *           fold in one kernel) when every member has a heap segment.
 *   SIGNAL  DIRECT's pulls with device-side barriers (per-peer counters in
 *           each PE's heap segment, polled over xGMI): no host wait,
 *           stream-ordered, capturable.  Source and target must both be in
 *           the symmetric heap on every member (ENOTSUP otherwise); calls on
 *           one PE must not overlap in time.  The one shot is one fused
 *           launch.  A peer that never arrives
 *           times out after $SHMEMX_SIGNAL_TIMEOUT s (default 20); the next
 *           blocking call then aborts with a FATAL line.
 *           Own slice, opt-in ($SHMEMX_SIGNAL_OWNSLICE=1, every PE alike, or
 *           shmemx_set_signal_ownslice; default off): the six own-order pairs
 *           (below) above $SHMEMX_DIRECT_ONESHOT_KB run OWNSLICE's schedule
 *           under SIGNAL's device barriers instead of every member reading
 *           every whole source: member m folds slice m of every source in
 *           all P orders, its own into its target and the others into slots
 *           in the second half of its IPC scratch region
 *           ($SHMEMX_DIRECT_SCRATCH_MB), device barrier, every member copies
 *           its slot from every other owner.  2(P-1)/P of the array per PE
 *           instead of (P-1)x, stream-ordered and capturable (after one warm
 *           call of the set, which allocates, maps and votes on the scratch
 *           regions); exact in place needs no temporary.  One fused launch
 *           per chunk up to $SHMEMX_FUSED_TWOSHOT_KB, five launches above;
 *           a call whose slots exceed half the scratch runs in chunks.
 *   OWNSLICE  opt-in, for the six own-order pairs (below) at two-shot cost:
 *           member m reads slice m of every member's source (as DIRECT's
 *           first phase) and folds it in all P orders at once, one result
 *           per member: its own into slice m of its own target, the others
 *           into P-1 slots of its IPC scratch region.  After a host barrier
 *           member k copies "its" result of every other slice from the
 *           owners' slots into its target (one gather launch).  2(P-1)/P of
 *           the array crosses xGMI per PE, as reads only, against (P-1)x
 *           for the other algorithms on these pairs; workspace (P-1) slices
 *           of scratch, no allocation.  Each PE's own reference bits.  Any
 *           set of 2..16 PEs, both transports, host-synchronous; operands
 *           anywhere (a source outside the heap or partially overlapping
 *           the target is staged through scratch, as DIRECT's).  Arrays up
 *           to $SHMEMX_DIRECT_ONESHOT_KB take DIRECT's own-order one shot.
 *           Every other pair, and a one-member set, plans and runs as
 *           DIRECT, so it may be set job-wide.  AUTO never chooses it.
 * With $SHMEMX_TRANSPORT=ipc there is no RCCL communicator: AUTO means
 * DIRECT, GATHER runs as a DIRECT-style kernel in each PE's own order, and
 * RCCL / A2A / ALLREDUCE are ENOTSUP; SIGNAL runs on both transports.
 * Float, double and long double min / max: a<b?a:b under NaN and +-0 gives
 * each PE its own reference answer (reduce-op.c:130-142, 219-248), so on
 * these six pairs every algorithm folds in the calling PE's own order: A2A
 * runs as GATHER, DIRECT and SIGNAL read every member's whole source;
 * OWNSLICE (and SIGNAL with its own slice on) has each slice's owner fold
 * it in every member's order. */
enum {
    SHMEMX_ALGO_AUTO = 0, SHMEMX_ALGO_RCCL, SHMEMX_ALGO_A2A,
    SHMEMX_ALGO_GATHER, SHMEMX_ALGO_ALLREDUCE, SHMEMX_ALGO_DIRECT, SHMEMX_ALGO_SIGNAL,
    SHMEMX_ALGO_OWNSLICE,
    SHMEMX_NALGOS
};

/* Error codes returned by shmemx_* and stored for shmemx_reduce_last_error. */
enum {
    SHMEMX_OK = 0,
    SHMEMX_EINVAL = 1,     /* bad argument (nreduce < 0, bad set, ...)     */
    SHMEMX_ENOTMEMBER = 2, /* calling PE is not in the active set          */
    SHMEMX_ENOTSUP = 3,    /* type/op/algorithm combination not supported  */
    SHMEMX_ENOINIT = 4,    /* runtime not initialised and npes > 1         */
    SHMEMX_ENOMEM = 5,     /* device workspace allocation failed           */
    SHMEMX_EDEVICE = 6     /* HIP or RCCL reported an error                */
};

/* Bootstrap with a caller-distributed RCCL unique id (128 bytes): PE `pe` of
 * `npes` on HIP device `device` (-1: pe mod device count).  PE 0 creates the
 * id with shmemx_get_uniqueid() and the launcher broadcasts it.  The id also
 * names the job's intra-node block (/dev/shm) that carries the symmetric-heap
 * IPC handles and the host barrier; all PEs run on one node.
 * $SHMEMX_TRANSPORT=ipc (set alike on every PE) skips RCCL entirely. */
int shmemx_uniqueid_size(void);
int shmemx_get_uniqueid(void *uid_out);
int shmemx_init_attr(int pe, int npes, int device, const void *uid);
int shmemx_initialized(void);

/* The HIP stream (hipStream_t) the blocking entry points run on. */
void *shmemx_get_stream(void);

/* Algorithm used by the entry points (default AUTO, or $SHMEM_REDUCE_ALGO =
 * auto|rccl|a2a|gather|allreduce|direct|signal|ownslice).  Returns the
 * previous value. */
int shmemx_set_algo(int algo);

/* Stream-ordered reduction: enqueue on `stream` (hipStream_t; NULL = the
 * runtime's stream) and return without waiting.  Buffers must be device
 * memory.  Capturable into a hipGraph once a call of the same shape has run
 * (workspaces are allocated on first use). */
int shmemx_reduce_on_stream(int type, int op, void *target, const void *source,
                            int nreduce, int PE_start, int logPE_stride,
                            int PE_size, int algo, void *stream);

/* The local element-wise fold, reduce-op.c:231-235 as one HIP kernel:
 *   acc[i] = op(acc[i], in[i])                              (fold2)
 *   out[i] = op(...op(op(ins[0][i], ins[1][i]), ins[2][i])..., ins[nins-1][i])
 * out may alias ins[0].  Device pointers, stream-ordered.  These local folds
 * (and shmemx_gather_on_stream) need no shmem_init and leave the calling
 * thread's current HIP device as it was; with a NULL stream after shmem_init
 * they launch on the PE's device.  Every other entry point makes the PE's
 * device current on the calling thread (hipSetDevice) and leaves it so. */
int shmemx_fold_on_stream(int type, int op, void *acc, const void *in,
                          size_t nelems, void *stream);
int shmemx_fold_n_on_stream(int type, int op, void *out,
                            const void *const *ins, int nins, size_t nelems,
                            void *stream);
/* The same fold for inputs that live in other GPUs' HBM (IPC-mapped peer
 * memory, as DIRECT and SIGNAL read it): every lane issues its loads of all
 * inputs before folding any, so every peer's xGMI link carries traffic at
 * once (the kernel above folds input k before loading input k + 1, which
 * keeps all waves behind one link at a time).  Same results, bit for bit. */
int shmemx_fold_n_peers_on_stream(int type, int op, void *out,
                                  const void *const *ins, int nins, size_t nelems,
                                  void *stream);

/* The P-order fold: nins inputs, nins outputs, one pass,
 *   outs[k][i] = op(...op(op(ins[k][i], ins[j0][i]), ins[j1][i])...)
 * with j ascending over the other inputs: for every k at once, the order in
 * which member k of a set folds (its own source first, reduce-op.c:219-248).
 * For the six pairs whose answer depends on that order (float, double and
 * long double min / max): ENOTSUP for any other reference pair.  outs[k] may
 * be exactly ins[k] (every lane loads all inputs of a vector before storing
 * any output of it); EINVAL for any other overlap between an output and an
 * input or another output, for nins outside 1..16, a pair the reference
 * lacks, or, with nelems > 0, NULL arrays or entries: all before any HIP
 * call.  nelems == 0 launches nothing.  Device pointers, stream-ordered;
 * device and shmem_init as for the local folds above.  OWNSLICE's first
 * phase; the kernel clock reports it as kind 4. */
int shmemx_fold_orders_on_stream(int type, int op, void *const *outs,
                                 const void *const *ins, int nins,
                                 size_t nelems, void *stream);

/* DIRECT's all-gather step as one launch: nseg (<= 16) byte ranges
 * srcs[i] -> dsts[i] copied concurrently (consecutive runs of up to 256
 * workgroups take the segments in turn, each workgroup 32 KiB of its
 * segment), so reads from every peer's HBM are in flight at once.  Any byte
 * alignment: 16-byte vectors where a segment's source and target agree mod
 * 16, bytes where they do not.  Zero-length segments are skipped (their
 * pointers may be NULL).  Device (or IPC-mapped peer) pointers,
 * stream-ordered; ranges must not overlap.  EINVAL, before anything is
 * launched, for nseg outside 0..16 or a segment whose source and target
 * are distinct and overlap. */
int shmemx_gather_on_stream(const void *const *srcs, void *const *dsts,
                            const size_t *bytes, int nseg, void *stream);

/* Test hook: the fused SIGNAL / DIRECT launches on one GPU, with no heap and
 * no peers.  Runs member m's launch of a P-member set (P <= 16) whose
 * members' sources srcs[i] and targets tgts[i] are all device arrays of the
 * calling process, on `stream`, and waits for it (blocking).
 *   schedule 0  the fused one shot: tgts[m] = fold of every whole source, in
 *               set order, or in m's own order (m first, then the others
 *               ascending) with own_order != 0;
 *   schedule 1  the fused two shot, set up as a SIGNAL call sets it up: m
 *               folds its slice of every source into tgts[m], then copies
 *               every other member's slice from tgts[i] to the same place in
 *               tgts[m] (own_order must be 0);
 *   schedule 2  the unfused device barrier alone (the system fence, then the
 *               signal wave); tgts, srcs and nelems are ignored.
 * What loops back is the peer handshake only: the launch is PE 0 of PEs
 * 0..P-1 over a private, zeroed signal area in which every "peer's counter
 * for me" is the very word the launch has just bumped for that peer, so
 * every wait is satisfied by the launch's own store.  The grid barrier, the
 * fences, the XCD-coverage check (counted in shmemx_direct_stats), the fold
 * and the gather run as in a multi-PE call.  A barrier that does not
 * complete gives up after 2 s.  The launch shares the device-side barrier
 * state of the SIGNAL and DIRECT algorithms: no SIGNAL or DIRECT call may be
 * in flight on this GPU.  Needs no shmem_init; the current device is treated
 * as by the local folds above.
 * *signal_error (may be NULL) receives the device barriers' error word after
 * the launch (0; 1 a wait timed out; 2 a fence missed an XCD), which is
 * cleared.  Returns OK (at once, for nelems == 0 with schedule 0 or 1);
 * EDEVICE for a failed launch, a non-zero error word, or a tiny one shot
 * (nelems <= 1024) whose host signal did not arrive; EINVAL, before any HIP
 * call, for a pair the reference lacks, schedule outside 0..2, P outside
 * 1..16, m outside 0..P-1, own_order with schedule 1, or, for schedules 0
 * and 1 with nelems > 0, NULL tgts / srcs or a NULL entry. */
int shmemx_fused_loopback(int type, int op, int schedule, int P, int m, int own_order,
                          void *const *tgts, const void *const *srcs, size_t nelems,
                          unsigned int *signal_error, void *stream);

/* Register (on != 0) or deregister the symmetric heap's HBM segment with
 * the library's RCCL communicator (ncclCommRegister), so RCCL may use
 * collectives' heap operands in place instead of staging them through its
 * own buffers.  Off by default: the N > 1 bench times the RCCL algorithms
 * both ways (extras.rccl_registered) before it is adopted.  A collective over
 * the whole job (the PEs agree with an ncclAllReduce that every one of them
 * registered): every PE must call it, in the same order as the other world
 * collectives, or the callers hang.  ENOTSUP without an RCCL communicator or
 * an HBM segment. */
int shmemx_rccl_register_heap(int on);

/* The kernel clock: with on != 0, every launch of the fold family (the
 * 2-input and P-input folds, the copy of a one-member call, the peers fold,
 * the gather, the P-order fold) carries start / stop events of its own dispatch
 * (hipExtLaunchKernelGGL), i.e. the kernel's execution time alone, with no
 * launch boundary and no event-marker latency; up to 4096 launches are
 * timed between reads.  shmemx_kernel_times waits for them and writes up to
 * max durations in microseconds to us[] and their kinds (0 fold, 1 copy,
 * 2 peers fold, 3 gather, 4 P-order fold) to kind[] (may be NULL), in launch order, and the
 * launches past the 4096 that went untimed to *dropped (may be NULL); it
 * returns how many were written and starts over.  Off by default; timing
 * does not change what runs. */
/* The resident service workgroup (DESIGN.md §6 "Small messages"): a
 * blocking one-member call (PE_size 1, a copy) of at most 32 KiB is done by
 * one workgroup that stays on the GPU polling a host-coherent mailbox, with
 * no kernel launch, after the legacy default stream's and the library
 * stream's earlier work (the host waits for them first when they still have
 * some); it leaves after 200 us without a request (so a
 * program's hipDeviceSynchronize waits that long at most) and at
 * shmem_finalize.  A blocking call over several PEs of at most 4 KiB per PE
 * under SHMEMX_ALGO_AUTO is served the same way: each member leaves its
 * source in a page-locked exchange shared by the job's PEs, and after the
 * entry barrier its workgroup folds every member's source into its target
 * (no kernel launch, no GPU reading another GPU's memory); a member writes
 * its part of the exchange again only once the readers of its previous call
 * are done with it.  $SHMEMX_SERVICE=0 turns both off (every PE alike); they are also
 * off when several PE processes of the job share one GPU, unless
 * $SHMEMX_SERVICE=1.  Stats:
 * out[0] requests served, out[1] launches of the workgroup, out[2] / out[3]
 * requests that found the legacy default stream / the library's stream busy
 * and waited for it, out[4] / out[5] nanoseconds summed over the served
 * requests from the check's start to the post / from the post to the result,
 * out[6] folds of the exchange (multi-PE calls); returns how many were
 * written. */
int shmemx_service_stats(unsigned long long *out, int nout, int reset);

/* Test hook: one fold request of the small-call exchange, in one process.
 * The set is (PE_start, logPE_stride, PE_size) among PEs 0..63 and the caller
 * plays PE `me`, a member.  srcs[i] is a host array of nelems elements, the
 * source of member PE_start + (i << logPE_stride).  The hook keeps a private
 * image of the exchange's 64 slots (page-locked, device-mapped, 4 KiB-aligned;
 * made on first use, freed at shmem_finalize), fills every byte of all 64
 * slots with 0xA5, copies each srcs[i] to the start of its member's slot, and
 * posts one fold request to the resident service workgroup, exactly as a
 * small multi-PE blocking call does after its entry barrier: the workgroup
 * folds the members' slots in PE_start's order, or with own_order != 0 in
 * me's own order (me first, then the others ascending), into dst and, if not
 * NULL, dst2 as well.  dst and dst2 are device-accessible addresses of the
 * caller's (device memory or page-locked host memory) with any element
 * alignment.  Blocking; the request counts in shmemx_service_stats as served
 * and as a fold.
 * What is real: the kernel, the mailbox request and its cfg word, the loads of
 * the slots and the stores to the targets.  What is not: the image comes from
 * hipHostMalloc, while the job's exchange is POSIX shared memory page-locked
 * with hipHostRegister, so the hook shows nothing about that mapping kind nor
 * about one GPU seeing what another PE's CPU or GPU wrote into a slot.
 * Returns EINVAL, before any HIP call, for a pair the reference lacks,
 * PE_size outside 1..64, PE_start < 0, logPE_stride outside 0..7, a last
 * member at 64 or above, me not a member, nelems elements larger than one
 * slot (4 KiB), NULL dst, or, with nelems > 0, NULL srcs or a NULL entry;
 * else OK at once for nelems == 0; else ENOTSUP without shmem_init or with
 * the service off ($SHMEMX_SERVICE=0, or PE processes sharing the GPU);
 * EDEVICE if the mailbox or the image cannot be had. */
int shmemx_service_fold_loopback(int type, int op, int own_order,
                                 int PE_start, int logPE_stride, int PE_size, int me,
                                 void *dst, void *dst2,
                                 const void *const *srcs, size_t nelems);

/* Test hook: which kernel instance one local fold launch would be, and on
 * which grid.  Pure host logic: the very argument checks, 16-byte split and
 * launch choice that the launch itself goes through (one definition each,
 * csrc/span16.h), from the addresses mod 16 alone.  Nothing is dereferenced
 * and no HIP call is made, so it needs no device and no shmem_init.
 *   route   SHMEMX_FOLD_ROUTE_PLAIN   one launch of shmemx_fold_on_stream
 *                                     (ins = {acc, in}, outs = {acc}) or of
 *                                     shmemx_fold_n_on_stream; nins == 1 is
 *                                     the copy;
 *           SHMEMX_FOLD_ROUTE_PEERS   ... of shmemx_fold_n_peers_on_stream;
 *           SHMEMX_FOLD_ROUTE_ORDERS  shmemx_fold_orders_on_stream;
 *   outs    the output (one entry), or the P-order fold's nins outputs;
 *   ins     the nins inputs.
 * One launch reads at most 16 inputs (shmemx_fold_n_on_stream chains longer
 * folds, 16 and then 15 inputs at a time into the output); nins above 16 is
 * refused here as by the launch.
 * On OK *shape holds
 *   family            SHMEMX_FOLD_FAMILY_*: the two-input fold, the fold with
 *                     a run-time input count, the peers fold, the P-order
 *                     fold, the copy; SHMEMX_FOLD_FAMILY_NONE (every other
 *                     field 0) for nelems == 0, which launches nothing;
 *   maxin             inputs the peers / P-order kernel unrolls (4, 8, 16 /
 *                     8, 16); 0 for the other families;
 *   vectors_per_lane  16-byte vectors per input each lane moves in one chunk;
 *   nt                cache policy bits: 1 non-temporal loads, 2 non-temporal
 *                     stores (3 from 32 MiB moved, else 0);
 *   blocks            workgroups (of 256 lanes);
 *   head, nvec, tail  scalar elements before, 16-byte vectors in, and scalar
 *                     elements after the vector body (nvec == 0: the arrays
 *                     differ mod 16 and all nelems are head);
 *   scalar_trips      trips of the grid-stride loop over the scalar elements,
 *                     ceil((head + tail) / (blocks * 256));
 *   ld80_pipelined    the call runs the software-pipelined long double branch
 *                     (long double, run-time input count, nins >= 3, at
 *                     least one whole chunk of vectors).
 * EINVAL exactly where the launch refuses: a pair the reference lacks (for
 * the P-order fold: any but its six pairs), a route outside 0..2, nins outside
 * 1..16, NULL shape or outs, a NULL output (the P-order fold: with
 * nelems > 0), NULL ins or a NULL input with nelems > 0 (the P-order fold:
 * NULL ins with any nelems). */
#define SHMEMX_FOLD_ROUTE_PLAIN 0
#define SHMEMX_FOLD_ROUTE_PEERS 1
#define SHMEMX_FOLD_ROUTE_ORDERS 2
#define SHMEMX_FOLD_FAMILY_NONE (-1)
#define SHMEMX_FOLD_FAMILY_FOLD2 0
#define SHMEMX_FOLD_FAMILY_FOLD_N 1
#define SHMEMX_FOLD_FAMILY_PEERS 2
#define SHMEMX_FOLD_FAMILY_ORDERS 3
#define SHMEMX_FOLD_FAMILY_COPY 4
typedef struct {
    int family;
    int maxin;
    int vectors_per_lane;
    int nt;
    int ld80_pipelined;
    long long blocks;
    long long head, nvec, tail;
    long long scalar_trips;
} shmemx_fold_launch_shape_t;
int shmemx_fold_launch_shape(int type, int op, int route, int nins, size_t nelems,
                             void *const *outs, const void *const *ins,
                             shmemx_fold_launch_shape_t *shape);

int shmemx_kernel_timing(int on);
int shmemx_kernel_times(double *us, int *kind, int max, unsigned long long *dropped);

/* Members-only RCCL communicators this PE holds for partial active sets
 * (PE_start, logPE_stride, PE_size other than the whole job): the RCCL
 * algorithms run on a set's own communicator, made by its members alone at
 * the set's first RCCL call and cached until shmem_finalize.  Returns how
 * many exist; $SHMEMX_SET_COMMS=0 (every PE alike) keeps partial sets on the
 * world communicator's grouped send/recv schedules instead. */
int shmemx_set_comms(void);

/* Largest DIRECT / SIGNAL two-shot call, in KiB, that runs as one fused
 * launch (default $SHMEMX_FUSED_TWOSHOT_KB, else 4096; 0 = never).  Every
 * member of a set must hold the same value when it calls (the members choose
 * their schedules independently).  Returns the previous value, or -1 (and
 * EINVAL) for kb < 0. */
long shmemx_set_fused_twoshot_kb(long kb);

/* SIGNAL's own slice (the SIGNAL paragraph above): on != 0 turns it on, 0
 * off (default $SHMEMX_SIGNAL_OWNSLICE, else off).  Every member of a set
 * must hold the same value when it calls.  Returns the previous value (0 or
 * 1), or -1 (and EINVAL) for on < 0.  With it on, shmemx_reduce_plan reports
 * the slice as chunk and the P - 1 result slots as ws_bytes for the calls
 * that take it; shmemx_direct_stats counts them in [14] and [15]. */
long shmemx_set_signal_ownslice(long on);

/* Bytes of one member's result slots in OWNSLICE's and SIGNAL's own-slice
 * schedules for nelems elements of `type` over P members: P - 1 slots of one
 * slice (ceil(nelems / P) elements rounded up to 16 bytes) each.  Host logic
 * only.  0 for an unknown type or P outside 1..16. */
size_t shmemx_order_slots_bytes(int type, int P, size_t nelems);

/* Test hook: SIGNAL's fused own-slice launch on one GPU, with no heap and no
 * peers, as shmemx_fused_loopback runs the other fused launches (the same
 * looped-back handshakes, 2 s bound, shared device-side barrier state and
 * device handling).  Runs member m's launch of a P-member set whose sources
 * srcs[i], targets tgts[i] and slot areas slots[i]
 * (shmemx_order_slots_bytes(type, P, nelems) bytes each) are all device
 * arrays of the calling process, and waits for it.  With [lo(i), hi(i)) the
 * two-shot slices of nelems over P: m folds elements [lo(m), hi(m)) of every
 * source in every member's own order (k first, then the others ascending),
 * order m into tgts[m] there and order k != m into slots[m] at slot
 * (k < m ? k : k - 1), slots of one whole slice each; then it copies, for
 * every other owner i of a non-empty slice, slot (m < i ? m : m - 1) of
 * slots[i] to tgts[m][lo(i), hi(i)).  tgts[i] may be srcs[i] exactly.
 * *signal_error as for shmemx_fused_loopback.  Returns OK (at once for
 * nelems == 0); EDEVICE for a failed launch or a non-zero error word; before
 * any HIP call, EINVAL for a pair the reference lacks, P outside 1..16, m
 * outside 0..P-1 or, with nelems > 0, NULL tgts / srcs / slots or a NULL
 * entry (slots' entries may be NULL for P == 1), and ENOTSUP for a reference
 * pair outside the six. */
int shmemx_fused_orders_loopback(int type, int op, int P, int m,
                                 void *const *tgts, const void *const *srcs,
                                 void *const *slots, size_t nelems,
                                 unsigned int *signal_error, void *stream);

/* Stream-ordered barrier, broadcast and fcollect: the collectives of Part 2b
 * as pure stream work under SIGNAL's device barriers, so a step that holds a
 * reduction, a broadcast and a barrier can be captured into one hipGraph.  No
 * host wait, no host barrier and no descriptor exchange: target and source
 * must both lie in the symmetric heap on every member (every member computes
 * every peer's address from its own offsets), on a job whose PEs share the
 * intra-node block.  A call is capturable after one warm call of the same set
 * has mapped the peers' heaps.  A NULL stream means the runtime's stream.
 * Calls of one PE, and its SIGNAL reductions, must not overlap in time (one
 * stream, or stream order between them).  Every member of the set must make
 * the call with the same sizes, root and settings.
 *   barrier    the mirrored heap's host stores go to HBM, then a system fence
 *              on every XCD and the device barrier, on the stream.
 *   fcollect   member i's nelems elements land at element i * nelems of every
 *              member's target.  One fused launch while PE_size * nelems *
 *              size is at most the shmemx_set_fused_twoshot_kb limit, else
 *              barrier, gather, barrier.  Any overlap of target and source is
 *              EINVAL.
 *   broadcast  PE_root is the index in the set, as in the blocking call; the
 *              root's target is never written.  target == source is allowed,
 *              a partial overlap is EINVAL.  Up to the
 *              shmemx_set_bcast_twophase_kb limit, and at PE_size 2, every
 *              non-root pulls the whole array from the root (one phase).
 *              Above it the PE_size - 1 non-roots each pull one slice from
 *              the root and the other slices from each other (two phases: the
 *              same bytes per GPU over PE_size - 1 links instead of one).
 *              One fused launch up to the shmemx_set_fused_twoshot_kb limit.
 * Return SHMEMX_OK or an error code, also left in shmemx_reduce_last_error():
 * EINVAL, before any HIP call, for a bad set, a root outside 0..PE_size-1, or
 * NULL operands with nelems > 0; EINVAL for a set that reaches past the job,
 * ENOTMEMBER for a caller outside the set; ENOTSUP, before any launch, for
 * operands outside the heap, more than 16 members, or no intra-node block.
 * nelems == 0 launches nothing, nor does a one-member set (a one-member
 * fcollect is one stream-ordered copy).
 * shmem_collect has per-PE counts that only the peers know; its
 * stream-ordered form, shmemx_collect{32,64}[_counted]_on_stream below,
 * exchanges them on the device, under the entry barrier. */
int shmemx_barrier_on_stream(int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_broadcast32_on_stream(void *target, const void *source, size_t nelems, int PE_root,
                                 int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_broadcast64_on_stream(void *target, const void *source, size_t nelems, int PE_root,
                                 int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_fcollect32_on_stream(void *target, const void *source, size_t nelems,
                                int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_fcollect64_on_stream(void *target, const void *source, size_t nelems,
                                int PE_start, int logPE_stride, int PE_size, void *stream);

/* Stream-ordered collect: shmem_collect{32,64} (member i's nelems_i elements
 * land at element sum of nelems_j, j < i, of every member's target, in set
 * order) under the same device barriers and the same rules as the calls above.
 * No host learns the peers' counts: each member publishes its count in a word
 * of its heap's signal area before the entry barrier and reads the others'
 * after it, on the device.
 *   capacity    the elements the target holds, the same on every member.  It
 *               is the only size the members share, so the route (one fused
 *               launch while capacity * size is at most the
 *               shmemx_set_fused_twoshot_kb limit, else seven launches:
 *               publish, barrier, plan, copy, barrier) and the grid come from
 *               it, PE_size and the element size alone.
 *   _counted    the count is *nelems_dev (8-byte aligned, device-accessible,
 *               inside the heap or not), read once by the call's first kernel
 *               when the call EXECUTES: a kernel earlier on the stream may
 *               have written it, and a graph replay reads it again.
 *               where_dev, unless NULL, receives two words: this member's
 *               offset and the total, in elements.
 * A member-local fact never refuses on the host (a lone refusal would leave
 * the peers in their barrier's timeout); the device judges it, alike on every
 * member: a member whose count is above capacity, or whose source would run
 * past the heap's end or into its target, publishes a poison count (all
 * ones).  If any count is poison or the total exceeds capacity, every member
 * writes nothing to its target, stores all ones to both where_dev words,
 * counts one overflow (shmemx_collect_stats) and still runs the exit
 * handshake.  The device barriers' error word is not touched: an overflow is
 * an answer, not a fault, and the next calls are healthy.
 * EINVAL, before any HIP call: a bad set, capacity * size * 16 wrapping, NULL
 * or not element-aligned target / source with capacity > 0, a NULL nelems_dev
 * (counted), nelems_dev / where_dev not 8-byte aligned, a source that STARTS
 * inside [target, target + capacity * size).  EINVAL / ENOTMEMBER for the set
 * as above.  ENOTSUP, before any launch: the source's start or the target's
 * capacity elements outside the heap, more than 16 members, no intra-node
 * block.  capacity == 0 launches nothing.  A one-member set needs no heap: it
 * is a copy of the member's own count, through the same kernels. */
int shmemx_collect32_on_stream(void *target, const void *source, size_t nelems, size_t capacity,
                               int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_collect64_on_stream(void *target, const void *source, size_t nelems, size_t capacity,
                               int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_collect32_counted_on_stream(void *target, const void *source,
                                       const unsigned long long *nelems_dev,
                                       unsigned long long *where_dev, size_t capacity,
                                       int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_collect64_counted_on_stream(void *target, const void *source,
                                       const unsigned long long *nelems_dev,
                                       unsigned long long *where_dev, size_t capacity,
                                       int PE_start, int logPE_stride, int PE_size, void *stream);

/* Counts of the stream-ordered collects since the last reset, up to nout of
 * them: [0] collects, [1] those that ran as one fused launch, [2] overflows
 * seen on the device (valid once the caller has synchronised the stream; the
 * loopback hook's launches count here too).  shmemx_pull_stats is unchanged.
 * Returns how many were written. */
int shmemx_collect_stats(unsigned long long *out, int nout, int reset);

/* Pure host logic: *fused = 1 if a stream-ordered collect of `capacity`
 * elements of esize (4 or 8) bytes over P members would run as one fused
 * launch under the current limit, 0 if unfused or capacity == 0.  EINVAL for
 * esize other than 4 or 8, P outside 1..16, a wrapping size or a NULL fused. */
int shmemx_collect_route(size_t esize, size_t capacity, int P, int *fused);

/* Test hook: member m's collect launches on one GPU, set up as
 * shmemx_pull_loopback (the same 2 s bound, shared device-side barrier state
 * and device handling, no shmem_init); waits for them.  The count words are a
 * private 16-word device array: the hook fills the peers' entries from counts
 * and leaves entry m to the kernel.  With counted != 0, counts[m] is first
 * copied to a device word the kernel reads.  fused != 0 selects the fused
 * launch, 0 the seven unfused launches, whatever the capacity.  srcs[m]'s room
 * ends at tgt where it lies below it.  where_out (unless NULL) receives the
 * two where words, *overflow_out the overflows this call counted,
 * *signal_error as for shmemx_fused_loopback.  Returns OK (at once for
 * capacity == 0); EDEVICE for a failed launch or a non-zero error word;
 * EINVAL, before any HIP call, for P outside 1..16, m outside 0..P-1, esize
 * other than 4 or 8, NULL counts, a wrapping capacity or, with capacity > 0,
 * a NULL or not element-aligned tgt / srcs / entry, or srcs[m] starting
 * inside the target. */
int shmemx_collect_loopback(int P, int m, size_t esize, void *tgt, const void *const *srcs,
                            const unsigned long long *counts, size_t capacity, int fused,
                            int counted, unsigned long long *where_out,
                            unsigned int *overflow_out, unsigned int *signal_error,
                            void *stream);

/* Stream-ordered alltoall and alltoallv: the personalised exchange (member i
 * hands a different block to each member j) under the same device barriers
 * and the same rules as the calls above.
 * alltoall follows OpenSHMEM 1.3 shmem_alltoall{32,64}: member i's elements
 * [j * nelems, (j + 1) * nelems) of source land at elements [i * nelems,
 * (i + 1) * nelems) of member j's target; both arrays hold PE_size * nelems
 * elements on every member, and any overlap of the two is EINVAL.
 * alltoallv, per member: send_counts[j] elements starting at element
 * send_offsets[j] of my source go to member j.  Member m packs what it
 * receives in set order: sender i's block lands at element sum of
 * send_counts_k[m], k < i, of m's target (a bucket ordered by sender, as the
 * collect's).  where_dev, unless NULL, receives PE_size + 1 words: the
 * element offset of every sender's block, then the total received.
 *   capacity      the elements the target holds, src_capacity the elements
 *                 the source holds, both the same on every member.  The route
 *                 (one fused launch while capacity * size is at most the
 *                 shmemx_set_fused_twoshot_kb limit, else six launches:
 *                 barrier, plan, copy, barrier) and the grid come from
 *                 capacity, PE_size and the element size alone.
 *   send_counts,  8-byte aligned symmetric-heap arrays of PE_size words, read
 *   send_offsets  by the PEERS when the call EXECUTES, after the entry
 *                 handshake: a kernel earlier on any member's stream may have
 *                 written them, and a graph replay reads them again.  No
 *                 signal-area word is used.
 * Target, source and the two tables must be pairwise disjoint.
 * What a member cannot know the device judges, per receiver: a pair whose
 * count exceeds src_capacity or whose offset exceeds src_capacity - count (a
 * peer's garbage never sends a load outside that peer's source), or a total
 * above capacity.  That member then writes nothing to its target, stores all
 * ones to all PE_size + 1 where_dev words, counts one overflow
 * (shmemx_alltoall_stats) and still runs the exit handshake; the other
 * members complete normally.  The device barriers' error word is not touched.
 * EINVAL, before any HIP call: a bad set, capacity or src_capacity * size * 16
 * wrapping (alltoall: PE_size * nelems * size * 16), NULL or not
 * element-aligned target / source with something to move, NULL tables, tables
 * or where_dev not 8-byte aligned, any overlap among target, source and the
 * tables.  EINVAL / ENOTMEMBER for the set as above.  ENOTSUP, before any
 * launch: target, source or either table outside the heap, more than 16
 * members, no intra-node block.  capacity == 0 or src_capacity == 0 (alltoall:
 * nelems == 0) launches nothing and writes no where_dev.  A one-member set
 * needs no heap and no handshake.
 * There are NO blocking shmem_alltoall* names: the reference's shmem.h is
 * OpenSHMEM 1.2 and does not declare them, and its own examples/sample_sort.c
 * defines shmem_alltoall32 with another signature, so declaring the 1.3
 * prototype here would break a reference program that builds today.  A
 * caller who wants the blocking form synchronises the stream. */
int shmemx_alltoall32_on_stream(void *target, const void *source, size_t nelems,
                                int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_alltoall64_on_stream(void *target, const void *source, size_t nelems,
                                int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_alltoallv32_on_stream(void *target, const void *source,
                                 const unsigned long long *send_counts,
                                 const unsigned long long *send_offsets,
                                 unsigned long long *where_dev, size_t capacity, size_t src_capacity,
                                 int PE_start, int logPE_stride, int PE_size, void *stream);
int shmemx_alltoallv64_on_stream(void *target, const void *source,
                                 const unsigned long long *send_counts,
                                 const unsigned long long *send_offsets,
                                 unsigned long long *where_dev, size_t capacity, size_t src_capacity,
                                 int PE_start, int logPE_stride, int PE_size, void *stream);

/* Counts of the stream-ordered alltoalls since the last reset, up to nout of
 * them: [0] alltoalls, [1] alltoallvs, [2] of those, the ones that ran as one
 * fused launch, [3] overflows seen on the device (valid once the caller has
 * synchronised the stream; the loopback hook's launches count here too).
 * Returns how many were written. */
int shmemx_alltoall_stats(unsigned long long *out, int nout, int reset);

/* Pure host logic: *fused = 1 if a stream-ordered alltoallv whose target
 * holds `capacity` elements of esize (4 or 8) bytes (alltoall: PE_size *
 * nelems) over P members would run as one fused launch under the current
 * limit, 0 if unfused or capacity == 0.  The limit is the fold's, inherited,
 * not measured for this call.  EINVAL for esize other than 4 or 8, P outside
 * 1..16, a wrapping size or a NULL fused. */
int shmemx_alltoallv_route(size_t esize, size_t capacity, int P, int *fused);

/* Test hook: member m's alltoallv launches on one GPU, set up as
 * shmemx_collect_loopback (the same 2 s bound, looped-back handshakes, no
 * shmem_init); waits for them.  counts and offsets are host P x P matrices,
 * row i what member i sends; the hook copies them to private device tables,
 * of which member m's kernels read column m.  NULL counts (and offsets) with
 * capacity = P * nelems runs the fixed alltoall; src_capacity is then taken
 * as capacity.  fused != 0 selects the fused launch, 0 the six unfused
 * launches, whatever the capacity.  where_out (unless NULL) receives the
 * P + 1 where words, *overflow_out the overflows this call counted,
 * *signal_error as for shmemx_fused_loopback.  Returns OK (at once for
 * capacity == 0 or src_capacity == 0); EDEVICE for a failed launch or a
 * non-zero error word; EINVAL, before any HIP call, for P outside 1..16, m
 * outside 0..P-1, esize other than 4 or 8, a wrapping capacity or
 * src_capacity, counts without offsets or the reverse, NULL counts with a
 * capacity that is no multiple of P or, with something to move, a NULL or not
 * element-aligned tgt / srcs / entry, or a source that meets the target. */
int shmemx_alltoallv_loopback(int P, int m, size_t esize, void *tgt, const void *const *srcs,
                              const unsigned long long *counts,
                              const unsigned long long *offsets, size_t capacity,
                              size_t src_capacity, int fused, unsigned long long *where_out,
                              unsigned int *overflow_out, unsigned int *signal_error,
                              void *stream);

/* Stream-ordered reduce-scatter: the one collective of this family that
 * folds, under the same device barriers and the same rules as the calls above.
 * Every member of the set holds a source of PE_size * nelems elements of
 * `type` and a target of nelems elements.  Element e of the target of the
 * member with index m in the set receives
 *   op(...op(op(src_0[m * nelems + e], src_1[m * nelems + e]),
 *            src_2[m * nelems + e])..., src_{P-1}[m * nelems + e]),
 * a left fold over the members in SET order, the order
 * shmemx_fold_n_on_stream documents, for every pair: the result equals
 * shmemx_fold_n_on_stream on the P blocks bit for bit, long double in soft x87
 * and the complex products included.  Float, double and long double min and
 * max take set order too, not the own order of the to_all calls: the
 * reference has no reduce-scatter, so there is no own-order answer to
 * reproduce.
 * When the call completes on the stream the member's target is final and its
 * source may be overwritten (the exit handshake has seen every peer finish
 * reading).  shmemx_reduce_scatter_on_stream followed by a kernel of the
 * caller's own on the slice and shmemx_fcollect{32,64}_on_stream is an
 * allreduce in one graph with the caller's kernel fused between its halves.
 *   route       one fused launch while PE_size * nelems * size (the source's
 *               bytes) is at most the shmemx_set_fused_twoshot_kb limit, else
 *               five launches: barrier, fold of the P blocks, barrier.
 *   vectors     the fold runs on 16-byte vectors when the target and all P
 *               block starts are 16-byte aligned, element by element
 *               otherwise.  Block m starts m * nelems * size bytes into the
 *               source, so a caller who wants vectors keeps nelems * size a
 *               multiple of 16 (and both operands 16-byte aligned).
 * EINVAL, before any HIP call: a bad set, a pair the reference lacks
 * (shmemx_op_valid), NULL or not element-aligned target / source with nelems
 * > 0 (8-byte alignment serves the 16-byte types), PE_size * nelems * size *
 * 16 wrapping, any overlap of [target, target + nelems * size) with [source,
 * source + PE_size * nelems * size): there is no in-place form.  EINVAL /
 * ENOTMEMBER for the set as above.  ENOTSUP, before any launch: an operand
 * outside the heap, more than 16 members, no intra-node block, a pair with
 * shmemx_op_on_device == 0.  nelems == 0 launches nothing.  A one-member set
 * needs no heap: it is one stream-ordered copy.  On the mirrored heap the
 * host-newer blocks of the source are flushed up and the target's blocks
 * marked device-newer, as for fcollect.  Calls of one PE share the grid
 * barrier's words with SIGNAL and the calls above and must not overlap them
 * in time; capturable after one warm call of the same set. */
int shmemx_reduce_scatter_on_stream(int type, int op, void *target, const void *source,
                                    size_t nelems, int PE_start, int logPE_stride,
                                    int PE_size, void *stream);

/* Pure host logic: *fused = 1 if a stream-ordered reduce-scatter of nelems
 * elements of `type` per member over P members would run as one fused launch
 * under the current limit, 0 if unfused or with nothing to launch (nelems ==
 * 0, P == 1).  EINVAL for an unknown type, P outside 1..16, a wrapping size or
 * a NULL fused. */
int shmemx_reduce_scatter_route(int type, size_t nelems, int P, int *fused);

/* Counts of the stream-ordered reduce-scatters since the last reset, up to
 * nout of them: [0] calls that had work, [1] those that ran as one fused
 * launch.  shmemx_pull_stats, shmemx_collect_stats and shmemx_alltoall_stats
 * are unchanged.  Returns how many were written. */
int shmemx_reduce_scatter_stats(unsigned long long *out, int nout, int reset);

/* Test hook: member m's reduce-scatter launches on one GPU, set up as
 * shmemx_fused_loopback (the same private signal area, the same 2 s bound,
 * looped-back handshakes, no shmem_init); waits for them.  srcs[k] is member
 * k's whole source of P * nelems elements, tgt member m's target.  fused != 0
 * selects the fused launch, 0 the five unfused launches, whatever the size.
 * *signal_error as for shmemx_fused_loopback.  Returns OK (at once for nelems
 * == 0); EDEVICE for a failed launch or a non-zero error word; ENOTSUP for a
 * pair with no kernel; EINVAL, before any HIP call, for a pair the reference
 * lacks, P outside 1..16, m outside 0..P-1, a wrapping size or, with nelems >
 * 0, a NULL or not element-aligned tgt / srcs / entry, or a source that meets
 * the target. */
int shmemx_reduce_scatter_loopback(int type, int op, int P, int m, void *tgt,
                                   const void *const *srcs, size_t nelems, int fused,
                                   unsigned int *signal_error, void *stream);

/* Largest stream-ordered broadcast, in KiB, that stays one phase (default
 * $SHMEMX_BCAST_TWOPHASE_KB, else 2048: derived, not measured on xGMI; 0 =
 * two phases whenever PE_size > 2).  Every member of a set must hold the same
 * value when it calls.  Returns the previous value, or -1 (and EINVAL) for
 * kb < 0. */
long shmemx_set_bcast_twophase_kb(long kb);

/* Counts of the stream-ordered calls above since the last reset, up to nout
 * of them: [0] barriers, [1] broadcasts, [2] fcollects, [3] the calls of [1]
 * and [2] that ran as one fused launch, [4] two-phase broadcasts (calls that
 * launched nothing are not counted).  Returns how many were written. */
int shmemx_pull_stats(unsigned long long *out, int nout, int reset);

/* Pure host logic: how member m's stream-ordered fcollect (kind 0) or
 * broadcast (kind 1) of nelems elements of esize (4 or 8) bytes over P
 * members would run under the current limits.  schedule 0: nothing is
 * launched (no elements, or one member).  nseg_a / nseg_b: the byte ranges m
 * pulls before / after the mid handshake (the root of a broadcast: none).
 * lo, hi: the slice m pulls from the root, in elements (two-phase non-root).
 * EINVAL for kind outside 0..1, esize other than 4 or 8, P outside 1..16, m
 * outside 0..P-1, for a broadcast a root outside 0..P-1, or a NULL plan. */
typedef struct { int schedule;   /* 0 none, 1 one-phase, 2 two-phase */
                 int fused; int nseg_a, nseg_b;
                 long long lo, hi;            /* my slice, elements (two-phase non-root) */
               } shmemx_pull_plan_t;
int shmemx_pull_plan(int kind, size_t esize, size_t nelems, int P, int m, int root,
                     shmemx_pull_plan_t *plan);

/* Test hook: member m's fused pull launch on one GPU, with no heap and no
 * peers, the handshakes looped back as shmemx_fused_loopback's (the same 2 s
 * bound, shared device-side barrier state and device handling); waits for it.
 *   schedule 0  fcollect: srcs[i]'s nelems elements to element i * nelems of
 *               tgts[m], for all P members;
 *   schedule 1  one-phase broadcast: all of srcs[root] to tgts[m];
 *   schedule 2  two-phase broadcast: m pulls its slice from srcs[root] and
 *               the other non-roots' slices from whatever the caller put in
 *               tgts[i].
 * For m == root a broadcast runs its handshakes and leaves tgts[m] as it was.
 * tgts[i] may be srcs[i] exactly (broadcast).  *signal_error as for
 * shmemx_fused_loopback.  Returns OK (at once for nelems == 0); EDEVICE for a
 * failed launch or a non-zero error word; EINVAL, before any HIP call, for a
 * schedule outside 0..2, P outside 1..16, m outside 0..P-1, for a broadcast a
 * root outside 0..P-1, esize other than 4 or 8 or, with nelems > 0, NULL
 * tgts / srcs or a NULL entry. */
int shmemx_pull_loopback(int schedule, int P, int m, int root, size_t esize,
                         void *const *tgts, const void *const *srcs, size_t nelems,
                         unsigned int *signal_error, void *stream);

/* How a call would be executed (pure host logic, no device needed). */
typedef struct {
    int algo;          /* resolved SHMEMX_ALGO_* (never AUTO)               */
    int member;        /* index of `pe` in the active set, -1 if none       */
    int nmembers;      /* PE_size                                           */
    int elem_size;     /* bytes per element                                 */
    long long chunk;   /* elements per shard (A2A) / per RCCL shard (RCCL)  */
    long long main;    /* RCCL: elements done by reduce-scatter+all-gather  */
    long long tail;    /* RCCL: elements done by the all-reduce tail        */
    long long ws_bytes;/* device workspace this call needs                  */
} shmemx_plan_t;
int shmemx_reduce_plan(int type, int op, int nreduce, int PE_start,
                       int logPE_stride, int PE_size, int pe, int npes,
                       int algo, shmemx_plan_t *plan);

/* Address of the symmetric object `addr` (in this PE's symmetric heap) as
 * mapped on this PE for PE `pe`'s copy — a device pointer a HIP kernel here
 * can load from / store to over xGMI (the shmem_ptr idea, querying/ptr.c).
 * NULL if `addr` is not in the heap segment or the peer is not mapped.  For a
 * mirrored heap's host-view address: `addr` itself for this PE, NULL for the
 * others (a store into a peer's HBM would go behind that peer's host view);
 * device-side puts take the twin (shmemx_mirror_device_ptr), whose peer
 * addresses this returns, and the receiver calls shmemx_mirror_invalidate on
 * the range after the barrier that orders the puts. */
void *shmemx_heap_ptr(const void *addr, int pe);

/* Mirrored heap (the default; $SHMEMX_HEAP_MEMORY=mirrored): the symmetric
 * heap is HBM and shmem_malloc returns addresses in a host view of it, so
 * host code reads and
 * writes symmetric objects as with the reference's host heap
 * (memory/symmem.c:168-227).  The collectives run on the HBM copy; the view
 * is kept coherent in 64 KiB blocks (page protection: a block the host stored
 * to is copied up when a collective next uses it, a block a collective wrote
 * is copied back when the host next touches it), so only touched blocks
 * cross PCIe.  Host-view addresses must not be handed to HIP calls directly.
 *   shmemx_mirror_device_ptr  the HBM twin of a host-view address (for the
 *                             caller's own kernels), NULL if not in the view;
 *   shmemx_mirror_sync        copy the host's stores in [addr, addr + bytes)
 *                             to HBM now;
 *   shmemx_mirror_invalidate  after the caller's own kernels wrote the HBM
 *                             twin: the host view re-reads it on next access;
 *   shmemx_mirror_acquire     make [addr, addr + bytes) current in the view
 *                             (and, with for_write, writable) now, for code
 *                             that cannot take the page fault: a system call
 *                             given a view address (write(2) of a result,
 *                             read(2) into a source) fails with EFAULT on a
 *                             block the library has not opened;
 *   shmemx_mirror_stats       out[0..6] = write faults, read faults, blocks
 *                             copied to HBM (whole, or a small operand's own
 *                             bytes of them), blocks copied back, blocks
 *                             marked device-newer, faults that waited for a
 *                             collective writing their block, blocks whose
 *                             result a blocking call put into the view
 *                             before returning (up to
 *                             $SHMEMX_MIRROR_SETTLE_KB, default 256 KiB);
 *                             returns how many were filled.
 * A host access to a block a collective is writing waits for it (from any
 * thread), then reads the result; a fetch waits only for the streams that
 * wrote the view (the caller's stream of a stream-ordered call, not the whole
 * device), and its HIP work runs on a service thread, never in the SIGSEGV
 * handler ("Mirrored heap"). */
void *shmemx_mirror_device_ptr(const void *addr);
int shmemx_mirror_sync(const void *addr, size_t bytes);
int shmemx_mirror_invalidate(const void *addr, size_t bytes);
int shmemx_mirror_acquire(const void *addr, size_t bytes, int for_write);
int shmemx_mirror_stats(unsigned long long *out, int nout, int reset);

/* Host-side phase times of the DIRECT algorithm since the last reset, for
 * tuning: out[0] = calls, then microseconds summed over them: [1] waiting for
 * this PE's source (entry fence + stream), [2] entry barrier, [3] fold kernel
 * (reduce-scatter from the peers' HBM), [4] barrier after it, [5] gather
 * kernel (all-gather from the peers' HBM), [6] exit barrier(s); then the
 * system-fence coverage counters (every XCD must run the fence that hands
 * data to the peers): [7] fences checked on the host, [8] of them run again
 * because a block did not reach some XCD, [9] fences checked by the SIGNAL
 * device barrier, [10] of them incomplete (the call fails); [11] one-shot
 * calls (DIRECT or SIGNAL) that ran as one fused launch, [12] two-shot calls
 * that did ($SHMEMX_FUSED_TWOSHOT_KB, default 4096), [13] calls that ran
 * OWNSLICE's two-phase schedule (its phases are timed in [3]-[6]: the P-order
 * fold as the fold, the pull of the result slots as the gather), [14] SIGNAL
 * calls that ran its own slice, [15] those of them whose every chunk was one
 * fused launch.  Fills at most
 * nout values and returns how many; reset != 0 zeroes the counters. */
int shmemx_direct_stats(double *out, int nout, int reset);

/* Page-lock a host range that will be handed to the entry points — the
 * reference's symmetric heap segment, posix_memalign'd once at start-up
 * (comms-inline.h:752-769) and handed to shmemi_mem_init (:794).  Host
 * targets/sources inside it then take the pinned H2D/reduce/D2H pipeline
 * instead of the pageable bounce ring.  SHMEMX_OK, or SHMEMX_EDEVICE when HIP
 * refuses (the range stays pageable and still works).  Unregister before the
 * range is freed. */
int shmemx_host_register(void *base, size_t bytes);
int shmemx_host_unregister(void *base);

/* Element size in bytes of a SHMEMX_TYPE_* (0 if unknown); 1 if the
 * reference defines shmem_<type>_<op>_to_all (reduce-op.c:388-431);
 * 1 if this build runs that pair on the GPU. */
size_t shmemx_type_size(int type);
int shmemx_op_valid(int type, int op);
int shmemx_op_on_device(int type, int op);

/* Position-aware 64-bit checksum of nelems elements (host or device memory;
 * long double: value bytes only) — XOR over 8-byte words w_j of
 * splitmix64-finalise(w_j + (j+1) * 0x9E3779B97F4A7C15); computed by a gfx950
 * kernel (wave shuffle + LDS partials).  The pointer needs only the
 * element's own alignment: host memory is staged into a device workspace, and
 * device memory that is not 16-byte aligned (a heap block at +8, a slice) is
 * first copied there too, on the library's stream; 16-byte aligned device
 * memory is read in place.  shmemx_verify: collective over the
 * active set, *all_equal = 1 iff every member's target has the same checksum
 * (what the A2A and RCCL algorithms guarantee after a reduction). */
int shmemx_checksum(int type, const void *ptr, size_t nelems, unsigned long long *out);
int shmemx_verify(int type, const void *target, int nreduce, int PE_start,
                  int logPE_stride, int PE_size, int *all_equal);

/* Last error of this thread and its text. */
int shmemx_reduce_last_error(void);
const char *shmemx_reduce_error_string(int err);

/* Last words.  FATAL conditions abort the process, as the reference's
 * SHMEM_LOG_FATAL exits it (trace.c:424-427); so do GPU memory faults (HSA)
 * and a launcher's SIGTERM when another PE died.  A caller holding a result
 * it must not lose registers it here: on SIGABRT, SIGSEGV, SIGBUS, SIGFPE,
 * SIGILL or SIGTERM the text is written to stdout and the process leaves
 * with _exit: exit_code for SIGTERM, 128 + the signal number for the others
 * (a crash stays visible in the exit status).  Calling again replaces the
 * text; NULL uninstalls and restores the previous handlers.  SHMEMX_OK or
 * SHMEMX_ENOMEM. */
int shmemx_set_fatal_note(const char *text, int exit_code);

/* Typed stream-ordered forms of all 44 entry points: shmemx_reduce_on_stream
 * with the type and op in the name, SHMEMX_ALGO_AUTO (or the algorithm set
 * with shmemx_set_algo / $SHMEM_REDUCE_ALGO).  Return SHMEMX_OK or the error
 * code (also left in shmemx_reduce_last_error()). */
#define SHMEMX_DECL_REDUCE_STREAM(Name, Op, T)                                 \
    int shmemx_##Name##_##Op##_to_all_on_stream(                             \
        T *target, const T *source, int nreduce, int PE_start,               \
        int logPE_stride, int PE_size, void *stream);
#define SHMEMX_DECL_STREAM_ARITH(Name, T)                                      \
    SHMEMX_DECL_REDUCE_STREAM(Name, sum, T) SHMEMX_DECL_REDUCE_STREAM(Name, prod, T)
#define SHMEMX_DECL_STREAM_LOGIC(Name, T)                                      \
    SHMEMX_DECL_REDUCE_STREAM(Name, and, T) SHMEMX_DECL_REDUCE_STREAM(Name, or, T) \
    SHMEMX_DECL_REDUCE_STREAM(Name, xor, T)
#define SHMEMX_DECL_STREAM_MINMAX(Name, T)                                     \
    SHMEMX_DECL_REDUCE_STREAM(Name, min, T) SHMEMX_DECL_REDUCE_STREAM(Name, max, T)
SHMEMX_DECL_STREAM_ARITH(short, short)
SHMEMX_DECL_STREAM_ARITH(int, int)
SHMEMX_DECL_STREAM_ARITH(long, long)
SHMEMX_DECL_STREAM_ARITH(longlong, long long)
SHMEMX_DECL_STREAM_ARITH(float, float)
SHMEMX_DECL_STREAM_ARITH(double, double)
SHMEMX_DECL_STREAM_ARITH(longdouble, long double)
SHMEMX_DECL_STREAM_ARITH(complexd, SHMEMX_COMPLEX(double))
SHMEMX_DECL_STREAM_ARITH(complexf, SHMEMX_COMPLEX(float))
SHMEMX_DECL_STREAM_LOGIC(short, short)
SHMEMX_DECL_STREAM_LOGIC(int, int)
SHMEMX_DECL_STREAM_LOGIC(long, long)
SHMEMX_DECL_STREAM_LOGIC(longlong, long long)
SHMEMX_DECL_STREAM_MINMAX(short, short)
SHMEMX_DECL_STREAM_MINMAX(int, int)
SHMEMX_DECL_STREAM_MINMAX(long, long)
SHMEMX_DECL_STREAM_MINMAX(longlong, long long)
SHMEMX_DECL_STREAM_MINMAX(float, float)
SHMEMX_DECL_STREAM_MINMAX(double, double)
SHMEMX_DECL_STREAM_MINMAX(longdouble, long double)

#ifdef __cplusplus
}
#endif
#endif /* SHMEM_REDUCE_MI355X_H */
