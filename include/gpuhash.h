/*
 * gpuhash.h -- C ABI of the MI355X (gfx950) nonce-search engine.
 *
 * Drop-in for the ONE hot path of mohitreddy1996/BitCoin-Miner: the miner's min-hash
 * loop over a Request's inclusive [Lower, Upper].  The reference has no FFI; the
 * boundary is the Go call site that the unimplemented miner loop would occupy:
 *
 *   src/github.com/cmu440/bitcoin/miner/miner.go:15   // TODO: implement this!
 *     spec (p1.pdf pp.12-14): for n in [Lower, Upper] { h := bitcoin.Hash(Data, n) }
 *     keep the least h and its nonce, reply bitcoin.NewResult(h, n)
 *   src/github.com/cmu440/bitcoin/hash.go:11-15        bitcoin.Hash(msg, nonce) uint64
 *   src/github.com/cmu440/bitcoin/message.go:25-42     NewRequest(data, lower, upper),
 *                                                      NewResult(hash, nonce)
 *
 * A Go miner binds it with cgo (INTEGRATION.md shows the stub).  Plain C types only:
 * pointers + sizes + uint64; no torch, no HIP types.  All integers host-endian.
 *
 * Semantics reproduced bit-exactly:
 *   Hash(msg, n) = big-endian uint64 of SHA-256(msg ‖ ' ' ‖ decimal(n))[0:8]
 *   gpuhash_min  = argmin over the INCLUSIVE range of the key (Hash, nonce): the least
 *                  hash, and among equal hashes the lowest nonce (what an ascending
 *                  scan with strict '<' returns).  Overflow-safe at upper = 2^64-1.
 *
 * Threading: calls on one context are serialised internally (a second caller waits);
 * separate contexts run concurrently.  gpuhash_close must not race other calls on
 * the same context.  Every entry point leaves the calling thread's current HIP device
 * as it found it (device work may run on the caller's thread, which a cgo-locked
 * goroutine or a torch process may share).
 *
 * Errors are negative return codes (gpuhash_strerror); nothing is printed, and no C++
 * exception crosses the ABI (allocation failures map to GPUHASH_ENOMEM, any other
 * host-side failure, e.g. thread creation, to GPUHASH_EHIP).  GPUHASH_EINVAL and
 * GPUHASH_ETOOLONG are deterministic argument errors: retrying the same call elsewhere
 * fails the same way.  GPUHASH_ENODEV / EHIP / ENOMEM are device or resource errors, and
 * GPUHASH_ECANCELED is neither: the caller asked for it (gpuhash_cancel).  The HIP
 * path is the only compute path: with no usable device gpuhash_open fails with
 * GPUHASH_ENODEV -- there is no silent CPU fallback.
 */
#ifndef GPUHASH_H
#define GPUHASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPUHASH_OK 0
#define GPUHASH_EINVAL (-1)   /* null pointer, lower > upper, bad device list / count */
#define GPUHASH_ENODEV (-2)   /* no usable gfx950 device */
#define GPUHASH_EHIP (-3)     /* a HIP runtime call or kernel launch failed */
#define GPUHASH_ETOOLONG (-4) /* msg_len > GPUHASH_MAX_MSG */
#define GPUHASH_ENOMEM (-5)   /* device or host allocation failed */
#define GPUHASH_ECANCELED (-6) /* the context's cancel latch is set (gpuhash_cancel) */

/* The reference carries the message in a JSON frame inside <=2000-byte LSP datagrams
 * (lspnet/conn.go:35), so real messages are ~1.3 KB at most; the engine accepts more. */
#define GPUHASH_MAX_MSG (1u << 20)

typedef struct gpuhash_ctx gpuhash_ctx;

/* Per-call measurements of the last gpuhash_min / gpuhash_first_below /
 * gpuhash_collect_below / gpuhash_hash_range on a context. */
typedef struct gpuhash_stats {
    uint64_t nonces;          /* nonces searched by the last call (gpuhash_first_below: */
                              /*    those an ascending scan would have examined;        */
                              /*    gpuhash_collect_below: the span, all of it hashed)  */
    uint32_t launches;        /* scan-kernel launches (all devices; gpuhash_collect_below: */
                              /*    re-runs of overflowed sub-ranges included)          */
    uint32_t ndevices;        /* devices that received a non-empty shard              */
    double wall_ms;           /* host wall time of the call                           */
    double kernel_ms;         /* sum over devices of HIP-event time of scan launches  */
    double max_dev_kernel_ms; /* slowest device's scan-kernel time                    */
} gpuhash_stats;

/* One scan-kernel launch of the last call (bench.py derives the dominant kernel's
 * average launch time and algorithmic work from these). */
typedef struct gpuhash_launch_record {
    int32_t device;   /* HIP ordinal of the context entry that ran the launch       */
    int32_t J;        /* kernel variant: loop-word index in the final block (0..15) */
    int32_t C2;       /* 1: lane digits spill into block B-1, per-nonce schedule;   */
                      /* 2: block B's W_0/W_1 hold only loop digits, schedules      */
                      /*    shared per wave through LDS; 3: lane table (per-lane    */
                      /*    block-B schedule, block B-1 state from a p-table)       */
    int32_t EX;       /* 1: extra all-constant padding block                        */
    int32_t digits;   /* decimal digits of every nonce in the launch                */
    int32_t c;        /* 64-byte blocks holding nonce digits (1 or 2)               */
    int32_t shard;    /* index of the context entry (gpuhash_open's list position)  */
    int32_t stream_device; /* ordinal the HIP runtime reports for the stream the    */
                      /*    kernel was launched on (hipStreamGetDevice): evidence   */
                      /*    that the shard ran on `device`, not on device 0         */
    uint64_t lo, hi;  /* the shard's inclusive nonce range in this slice            */
                      /*    (gpuhash_min_batch: the index of the first and the last */
                      /*    job of the entry's run, see there)                      */
    uint64_t nonces;  /* nonces covered by the launch                               */
    double ms;        /* HIP-event time of the launch on the device's stream        */
    double sclk_mhz;  /* shader clock over the launch, measured in the kernel:      */
                      /*    s_memtime ticks / s_memrealtime (100 MHz) of workgroup 0 */
} gpuhash_launch_record;

/* Opens the listed devices (HIP ordinals); ndevices == 0 means every visible device.
 * Allocates per-device streams, events and a small candidate buffer.  An ordinal may be
 * listed more than once (each entry is a separate shard with its own stream).
 * Replaces: nothing in the reference (the miner would call it once at start-up,
 * miner.go:8-16). */
int gpuhash_open(const int *devices, int ndevices, gpuhash_ctx **out);

/* Number of devices a context drives. */
int gpuhash_ndevices(const gpuhash_ctx *ctx);

/* Number of visible HIP devices (0 if none).  Lets a host check a device list before
 * gpuhash_open (bench.py --gpus N refuses N above it).  Replaces nothing in the reference. */
int gpuhash_device_count(void);

/* The static partition gpuhash_min applies over n devices, for hosts that shard one
 * search over PROCESSES instead (gpuhash.dist: one process per GPU):
 * nshards contiguous shards of the inclusive [lower, upper], in order, of equal estimated
 * cost -- nonces x the layout's relative cost per digit group, so a range whose digit
 * groups differ in SHA blocks (message lengths 45-54, 1 -> 2 blocks at some digit count)
 * is balanced by work, not by count.  Shard k is [out_lower[k], out_upper[k]];
 * out_lower[k] > out_upper[k] (1 > 0) marks an empty shard.  Returns the number of
 * non-empty shards, or GPUHASH_EINVAL (nshards < 1, null outputs, lower > upper) /
 * GPUHASH_ETOOLONG.  Host-only: needs no device.  Replaces the server's job split of
 * p1.pdf p.14 within one node; the merge is the same (hash, nonce) argmin. */
int gpuhash_shard_range(size_t msg_len, uint64_t lower, uint64_t upper, int nshards,
                        uint64_t *out_lower, uint64_t *out_upper);

/* gpuhash_shard_range under a layout policy (gpuhash_set_layout_policy's values): the
 * cost of a digit group depends on the layout that runs it, so gpuhash_min's in-process
 * cuts under a non-AUTO policy are these, and a host sharding over processes with that
 * policy passes it here to cut the same way.  gpuhash_shard_range is this with
 * GPUHASH_LAYOUT_AUTO.  GPUHASH_EINVAL also for an invalid policy.  Host-only. */
int gpuhash_shard_range_policy(size_t msg_len, uint64_t lower, uint64_t upper, int nshards, int policy,
                               uint64_t *out_lower, uint64_t *out_upper);

/* Layout choice for a digit group whose digits straddle two SHA blocks with the loop word
 * at W_1 of the last block, i.e. 5-8 digits in the last block.  Let
 * q = the digits in block B's W_0/W_1 (RQ = 10^q nonces per block B-1 value), nb1 = the
 * digits in block B-1, span = the search's nonces in that digit group, and N =
 * (span - 1) / RQ + 2, the block B-1 values such a span can touch.  This comment is
 * the ONE statement of the rule; csrc/plan.cpp (layout_for) implements it and
 * tests/test_plan.py checks the two against each other.
 *   AUTO (default)  span < 2 * RQ                                -> C2 = 1 (classic)
 *                   else nb1 >= 3 and N > GPUHASH_LANETABLE_MAX  -> C2 = 2 (two-word loop)
 *                   else                                         -> C2 = 3 (lane table)
 *   UNIFORM         nb1 >= 3 -> C2 = 2, else C2 = 3
 *   CLASSIC         C2 = 1 always (the per-nonce-schedule layout)
 *   LANETABLE       C2 = 3 up to N = GPUHASH_LANETABLE_MAX, C2 = 2 beyond it (each value
 *                   costs 64 B of table and one compression, so the cap bounds memory)
 * Results are identical under every policy; only speed differs.  Exposed for tuning and
 * so that parity tests can drive every kernel over small ranges.  Replaces nothing in
 * the reference. */
#define GPUHASH_LAYOUT_AUTO 0
#define GPUHASH_LAYOUT_UNIFORM 1
#define GPUHASH_LAYOUT_CLASSIC 2
#define GPUHASH_LAYOUT_LANETABLE 3
#define GPUHASH_LANETABLE_MAX 65536u
/* Tail-digit launches, for any policy above: a digit group whose last
 * digit-bearing word holds ONE digit after a word of four (e.g. "bradfitz" at 8 and 12
 * digits) would loop over only 10 values per 256-lane row; it runs instead as ten
 * launches, one per last digit t, over the nonces = t (mod 10) with t a constant message
 * byte, looping over the previous word's 10^4 values.  Taken when the search spans at
 * least GPUHASH_TAIL_MIN_SPAN nonces of the group (below that, the launches' partial rows
 * cost more than the short loop); OR GPUHASH_LAYOUT_TAIL_ALWAYS or _NEVER into the policy
 * to force either way (parity tests, tuning).  Results are identical either way. */
#define GPUHASH_LAYOUT_TAIL_ALWAYS 16
#define GPUHASH_LAYOUT_TAIL_NEVER 32
#define GPUHASH_TAIL_MIN_SPAN 8589934592ull
/* Packed tiny jobs, for any policy above, with or without a tail flag: OR
 * GPUHASH_LAYOUT_PACKED_ALWAYS into the policy and every job of gpuhash_min_batch[_ex] and
 * gpuhash_collect_below_batch[_ex] that has at most GPUHASH_PACKED_MAX_SPAN nonces is packed:
 * it runs in one launch of a kernel whose every lane hashes one (job, nonce) from the job's
 * midstate, so that no lane idles where the layouts above would fill a 256-lane row with a
 * single nonce.  Larger jobs of the same call run exactly as without the flag, in the same
 * stage.  Every other entry point accepts the flag and ignores it: the single calls
 * (gpuhash_min, gpuhash_first_below, gpuhash_collect_below and their _ex forms),
 * gpuhash_first_below_batch[_ex] (its value is its digit-ordered early exit, which packing
 * would not help), gpuhash_hash_range and gpuhash_shard_range_policy.  Results are identical
 * with and without the flag; only speed differs, and a packed nonce costs more instructions
 * than a nonce of a full row: the flag is for hosts that know their jobs are tiny.  The cap is
 * structural (at 10^6 nonces and more the layouts above fill their rows, and a packed job's
 * index arithmetic stays within 32 bits), not a measured crossover: the flag forces packing up
 * to it even where packing is slower. */
#define GPUHASH_LAYOUT_PACKED_ALWAYS 64
#define GPUHASH_PACKED_MAX_SPAN (1u << 20)
int gpuhash_set_layout_policy(gpuhash_ctx *ctx, int policy);

/* argmin_{n in [lower, upper]} (Hash(msg, n), n) -> *out_hash, *out_nonce.
 * Replaces the miner loop of p1.pdf pp.12-14 (miner.go:15) and feeds
 * bitcoin.NewResult(hash, nonce) (message.go:36-42).  msg is read during the call
 * only (cgo pointer rules); the range is split statically over the context's devices
 * (one host thread + one stream each), reduced on the host.  Blocking, but not beyond reach:
 * another thread, or a signal handler, ends the call with gpuhash_cancel and reads how far it
 * is with gpuhash_progress (below).  Any span is
 * accepted, up to the full [0, 2^64-1]: spans over 2^38 nonces per device run as
 * consecutive slices (env GPUHASH_SLICE_NONCES overrides the per-device slice). */
int gpuhash_min(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len, uint64_t lower,
                uint64_t upper, uint64_t *out_hash, uint64_t *out_nonce);

/* Same search, caller-chosen work-item granularity (r values per workgroup; 0 =
 * default).  Exposed for tuning and for parity tests of the chunked paths. */
int gpuhash_min_ex(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len, uint64_t lower,
                   uint64_t upper, uint32_t rchunk, uint64_t *out_hash, uint64_t *out_nonce);

/* The lowest n in the inclusive [lower, upper] with Hash(msg, n) <= target: what an ascending
 * scan that stops at its first hit returns (proof-of-work's question; gpuhash_min answers
 * "the least hash").  *out_found = 1 and (*out_hash, *out_nonce) = that nonce and its hash,
 * or *out_found = 0 (outputs untouched) when no nonce of the range qualifies.  The
 * comparison is <=, so target = 2^64-1 returns lower.  A nonce of 2^64-1 is a legal answer:
 * only *out_found says whether there is one.  The answer is exact -- the LOWEST qualifying
 * nonce, never merely some qualifying nonce -- under every layout policy and rchunk: the
 * kernels skip work only above a qualifying nonce they have already found,
 * so the call returns long before the range is exhausted when a hit lies early in it.
 * Errors, threading, device-guard behaviour, GPUHASH_MAX_MSG, layout policies, slices and
 * any span up to [0, 2^64-1] are as for gpuhash_min.  Devices take the same contiguous
 * shards and the lowest-nonce hit wins; a search over several slices stops after the first
 * slice that has a hit.  Afterwards gpuhash_last_stats().nonces is what the ascending scan
 * would have examined -- nonce - lower + 1 when found, the span otherwise -- not what the
 * devices hashed, and gpuhash_last_launches reports the launches that ran.  Replaces
 * nothing in the reference (its protocol has no target field). */
int gpuhash_first_below(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len, uint64_t lower,
                        uint64_t upper, uint64_t target, uint64_t *out_hash, uint64_t *out_nonce,
                        int *out_found);

/* Same search, caller-chosen work-item granularity (as gpuhash_min_ex). */
int gpuhash_first_below_ex(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len, uint64_t lower,
                           uint64_t upper, uint64_t target, uint32_t rchunk, uint64_t *out_hash,
                           uint64_t *out_nonce, int *out_found);

/* Every n in the inclusive [lower, upper] with Hash(msg, n) <= target: how many there are, and
 * the lowest of them (a pool miner's shares; the hit count of a range at a trial target;
 * gpuhash_first_below answers "the first one").  *out_total = the EXACT number of qualifying
 * nonces; it saturates at 2^64-1, which only [0, 2^64-1] with target = 2^64-1 reaches.
 * out_nonces[i], out_hashes[i] for i < min(cap, total) = the LOWEST min(cap, total) qualifying
 * nonces, ascending by nonce, and their hashes -- never merely some qualifying nonces, under
 * every layout policy and rchunk and however many devices ran.  Entries from min(cap, total)
 * on are untouched.  cap == 0 is a pure count; out_nonces and out_hashes may then be null.
 * The comparison is <=, so target = 2^64-1 counts the span.  A nonce of 2^64-1 is a legal hit.
 * GPUHASH_EINVAL, checked before any use of ctx's contents: cap > GPUHASH_COLLECT_MAX, null
 * out_total, cap > 0 with a null array (and gpuhash_min's: null ctx, lower > upper).
 * Built for SPARSE hits: per nonce it costs what gpuhash_min costs (one compare against the
 * target's high word and a ballot), and every hit costs an append to a device list of
 * GPUHASH_COLLECT_MAX entries (16 MB per context entry, allocated on its first collecting
 * call; env GPUHASH_COLLECT_BUFFER=<entries> overrides the size).  A dense target is still
 * exact but slower: every wave iteration then takes the append path (one atomic add per
 * 64 nonces and a store per listed hit; counting 2^28 nonces at target 2^62, a quarter of
 * them hits, took 6x gpuhash_min's time), and a sub-range with more hits than
 * the list holds is split and run again while the output still has room (once cap hits are
 * held the rest of the range is only counted).
 * Every nonce of the range is hashed, there is no early exit: gpuhash_last_stats().nonces is
 * the span, and gpuhash_last_launches reports what ran, re-runs included.  Errors, threading,
 * device-guard behaviour, GPUHASH_MAX_MSG, layout policies and tail flags, rchunk, contiguous
 * shards over the context's entries, slices and any span up to [0, 2^64-1] are as for
 * gpuhash_min.  Replaces nothing in the reference (its protocol has no target field). */
#define GPUHASH_COLLECT_MAX (1u << 20)
int gpuhash_collect_below(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len, uint64_t lower,
                          uint64_t upper, uint64_t target, uint64_t *out_nonces, uint64_t *out_hashes,
                          size_t cap, uint64_t *out_total);

/* Same collection, caller-chosen work-item granularity (as gpuhash_min_ex). */
int gpuhash_collect_below_ex(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len, uint64_t lower,
                             uint64_t upper, uint64_t target, uint32_t rchunk, uint64_t *out_nonces,
                             uint64_t *out_hashes, size_t cap, uint64_t *out_total);

/* njobs independent gpuhash_min searches in one call: (out_hashes[k], out_nonces[k]) is exactly
 * what gpuhash_min(ctx, msg_k, len_k, lower[k], upper[k]) returns -- the least hash, and the
 * lowest nonce among equal hashes -- under every layout policy, tail flag and rchunk, however
 * many context entries ran and in whatever order the jobs are listed.  For hosts whose searches
 * are many and small (a server's jobs, config-1-sized requests): a gpuhash_min call costs ~70 us
 * whatever its range, a batch runs ONE scan launch per kernel variant among all its jobs
 * (DESIGN.md 3.11), not one per variant per job.
 * The arrays are flat (no pointers inside structs: cgo's pointer rules).  Job k's message is
 * msgs[msg_off[k] .. msg_off[k+1]); msg_off has njobs + 1 entries and never decreases.  Messages
 * may be empty (msgs may be null when all are), and jobs may share or repeat a message.  The jobs
 * are independent: overlapping ranges of one message are two separate searches.
 * Whole-call argument errors, detected before any use of ctx's contents and before anything is
 * written to the outputs, deterministic as gpuhash_min's: GPUHASH_EINVAL for a null pointer,
 * njobs == 0 or njobs > GPUHASH_BATCH_MAX_JOBS, a msg_off that decreases, any lower[k] >
 * upper[k], any job of more than GPUHASH_BATCH_MAX_SPAN nonces (one slice: split longer searches
 * or use gpuhash_min); GPUHASH_ETOOLONG for any message over GPUHASH_MAX_MSG.
 * A batch runs as consecutive SUB-BATCHES of whole jobs, each holding as many jobs as keep its
 * launch metadata, result list and K+W tables within GPUHASH_BATCH_BYTES_DEFAULT bytes per
 * context entry (env GPUHASH_BATCH_BYTES=<bytes> overrides it, up to 1 GiB; a single job always
 * fits).  A sub-batch's jobs are cut into contiguous runs of about equal estimated cost, one per
 * context entry, which run concurrently; a job is never split across entries.  Splitting never
 * changes a result.
 * Afterwards gpuhash_last_stats().nonces is the sum of the jobs' spans (saturating) and
 * .launches the scan launches that ran; gpuhash_last_launches gives one record per kernel
 * variant per context entry per sub-batch, with `nonces` the total of that variant's launches
 * and -- for batch records only -- `lo` and `hi` the INDEX of the first and the last job of that
 * entry's run, not nonces.  Threading, device-guard behaviour, errors and the no-exception rule
 * are as for gpuhash_min.  Replaces nothing in the reference (its miner takes one job at a time). */
#define GPUHASH_BATCH_MAX_JOBS (1u << 16)
#define GPUHASH_BATCH_MAX_SPAN (1ull << 38)   /* nonces per job: one slice */
#define GPUHASH_BATCH_BYTES_DEFAULT (32u << 20)
int gpuhash_min_batch(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                      const uint64_t *lower, const uint64_t *upper,
                      uint64_t *out_hashes, uint64_t *out_nonces);

/* Same batch, caller-chosen work-item granularity (as gpuhash_min_ex). */
int gpuhash_min_batch_ex(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                         const uint64_t *lower, const uint64_t *upper, uint32_t rchunk,
                         uint64_t *out_hashes, uint64_t *out_nonces);

/* njobs independent gpuhash_first_below searches in one call (a service that mints one
 * proof-of-work stamp per request): out_found[k], and when it is 1 (out_hashes[k], out_nonces[k]),
 * are exactly what gpuhash_first_below(ctx, msg_k, len_k, lower[k], upper[k], target[k], ...)
 * returns -- the LOWEST nonce of the job's range whose hash is <= target[k], and its hash -- under
 * every layout policy, tail flag and rchunk, however many context entries ran and in whatever order
 * the jobs are listed.  A job with out_found[k] == 0 leaves its two outputs untouched.  The
 * comparison is <=, and a nonce of 2^64-1 is a legal answer.  The jobs are independent: two jobs of
 * one message with different targets or overlapping ranges are two searches.
 * A gpuhash_first_below call costs ~0.4 ms however early its hit lies; a batch runs one scan
 * launch per DIGIT COUNT per kernel variant among all its jobs, in ascending digit order, so a
 * job whose answer has d digits never hashes a nonce of more than d digits, and skips within its
 * digit count as gpuhash_first_below does.
 * The flat arrays, msg_off, the whole-call argument errors (detected before any use of ctx's
 * contents and before anything is written to the outputs; a null target or out_found is
 * GPUHASH_EINVAL too), GPUHASH_BATCH_MAX_JOBS, GPUHASH_BATCH_MAX_SPAN, the sub-batches under
 * GPUHASH_BATCH_BYTES and the runs of whole jobs over the context's entries are as for
 * gpuhash_min_batch.
 * Afterwards gpuhash_last_stats().nonces is the saturating sum over the jobs of what an ascending
 * scan would have examined -- nonce - lower + 1 when found, the span otherwise -- and .launches
 * the scan launches that ran; gpuhash_last_launches gives one record per (digits, kernel variant)
 * per context entry per sub-batch, in launch order, with `digits` exact, `nonces` the total the
 * launch covers (not what it hashed) and `lo`, `hi` job indices as for gpuhash_min_batch.
 * Threading, device-guard behaviour, errors and the no-exception rule are as for gpuhash_min.
 * Replaces nothing in the reference (its protocol has no target field). */
int gpuhash_first_below_batch(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                              const uint64_t *lower, const uint64_t *upper, const uint64_t *target,
                              uint64_t *out_hashes, uint64_t *out_nonces, int *out_found);

/* Same batch, caller-chosen work-item granularity (as gpuhash_min_ex). */
int gpuhash_first_below_batch_ex(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                                 const uint64_t *lower, const uint64_t *upper, const uint64_t *target,
                                 uint32_t rchunk, uint64_t *out_hashes, uint64_t *out_nonces, int *out_found);

/* gpuhash_first_below_batch_ex for jobs whose first hit lies EARLY in their range (stamp jobs: a
 * range of 2^32 nonces, an answer some 10^4-10^6 nonces in).  The results are exactly those of
 * gpuhash_first_below_batch_ex on the same arguments -- the LOWEST qualifying nonce per job, under
 * every layout policy, tail flag, rchunk, prefix and number of context entries; only speed differs.
 * The front of every job runs PACKED, every lane hashing one (job, nonce) as under
 * GPUHASH_LAYOUT_PACKED_ALWAYS (which this call ignores), in ascending rounds whose pieces double:
 * round r gives every job still open the next min(c_r, what is left of its front) nonces, c_0 =
 * 2^20 / (jobs with a front) rounded up to a power of two and clamped to [64, 2^20], c_(r+1) =
 * min(2 c_r, 2^20).  One launch per round, per context entry, per sub-batch; a job with a hit in a
 * round is answered by that round's lowest hit and closed.  A job whose answer lies x nonces above
 * lower[k], inside its front, hashes at most 2x + c_0 packed nonces.  What is left of the jobs
 * still open after their fronts runs as gpuhash_first_below_batch_ex runs it, with rchunk.
 * The front of job k is its first limit_k nonces.  prefix != 0 forces limit_k = min(span_k, prefix)
 * for every job (tuning and tests, as rchunk).  prefix == 0 is the rule, stated here ONCE
 * (csrc/stage.h, early_limit, implements it): with E_k = ceil(2^64 / (target[k] + 1)), the expected
 * position of the first hit,
 *   4 * E_k <= GPUHASH_EARLY_MAX_PREFIX  -> limit_k = min(span_k, 4 * E_k)
 *   otherwise                            -> limit_k = 0
 * (a geometric first hit lies beyond 4 * E_k with probability e^-4).  So a job with target 0 goes
 * straight to the scan path.  GPUHASH_EARLY_MAX_PREFIX is the largest power of two, up to 16 *
 * GPUHASH_PACKED_MAX_SPAN, at which the packed front measured faster than
 * gpuhash_first_below_batch (0.81 of its time at 2^24, 1.34 at 2^26).
 * Whole-call argument errors: everything gpuhash_first_below_batch_ex refuses, and GPUHASH_EINVAL
 * for prefix > GPUHASH_BATCH_MAX_SPAN; all detected before any use of ctx's contents and before
 * anything is written to the outputs.  There is no _ex twin: rchunk is an argument.
 * Afterwards gpuhash_last_stats().nonces is the ascending-scan figure of
 * gpuhash_first_below_batch and .launches every launch that ran.  gpuhash_last_launches gives one
 * record per round per sub-batch, the rounds of one context entry together and in order -- J = -1,
 * C2 = 4, EX = 0, digits = 0, `c` the most tail blocks, `nonces` the round's items, `lo` and `hi`
 * the lowest and the highest batch index among its jobs -- and then the remainder's records as
 * gpuhash_first_below_batch writes them, with the same meaning of `lo` and `hi`.  gpuhash_cancel is
 * read before every round and every sub-batch too, and gpuhash_progress counts the pieces handed
 * out.  Replaces nothing in the reference. */
#define GPUHASH_EARLY_MAX_PREFIX (1u << 24)
int gpuhash_first_below_batch_early(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                                    const uint64_t *lower, const uint64_t *upper, const uint64_t *target,
                                    uint64_t prefix, uint32_t rchunk,
                                    uint64_t *out_hashes, uint64_t *out_nonces, int *out_found);

/* njobs independent gpuhash_collect_below collections in one call (a miner holding many short work
 * units, each with its own message, range and share target; a service counting hits per message
 * to calibrate a difficulty): out_totals[k] is exactly what gpuhash_collect_below(ctx, msg_k,
 * len_k, lower[k], upper[k], target[k], ...) reports as *out_total, the EXACT number of nonces of
 * the job's range whose hash is <= target[k].  Job k's room in the two output arrays is
 * cap_k = out_off[k+1] - out_off[k] entries from out_off[k] on: out_nonces[out_off[k] + i] and
 * out_hashes[out_off[k] + i] for i < min(cap_k, total_k) are the LOWEST min(cap_k, total_k)
 * qualifying nonces of job k, ascending by nonce, and their hashes -- never merely some qualifying
 * nonces -- under every layout policy, tail flag and rchunk, however many context entries ran and
 * in whatever order the jobs are listed.  Entries from min(cap_k, total_k) on are untouched.  The
 * comparison is <=, a nonce of 2^64-1 is a legal hit, and the jobs are independent: two jobs of one
 * message with different targets or overlapping ranges are two collections.
 * out_off has njobs + 1 entries and never decreases; out_off == NULL means every cap_k = 0, a pure
 * count, and out_nonces and out_hashes may then be null.
 * A gpuhash_collect_below call costs ~0.1 ms whatever its range (three launches, two waits); a
 * batch runs ONE scan launch per kernel variant among all its jobs.  Every job
 * has an exact hit counter of its own on the device; the hits of all listing jobs go to ONE device
 * list per context entry of GPUHASH_COLLECT_MAX entries (24 MB, allocated on the entry's first
 * listing batch; env GPUHASH_COLLECT_BUFFER=<entries> overrides the size, as for
 * gpuhash_collect_below).  Built for SPARSE hits: a job all of whose hits found room in the list
 * is answered from it; a job cut short by a full list is run again alone, after the batch, as
 * gpuhash_collect_below runs it, so a batch dense enough to overflow the list costs as much as
 * the loop of single calls does, and is still exact.  Raising GPUHASH_COLLECT_BUFFER is the remedy.
 * The flat arrays, msg_off, empty messages, GPUHASH_BATCH_MAX_JOBS, GPUHASH_BATCH_MAX_SPAN, the
 * sub-batches under GPUHASH_BATCH_BYTES (which counts the launch metadata and the K+W tables, not
 * the fixed list) and the runs of whole jobs over the context's entries are as for
 * gpuhash_min_batch.  Whole-call argument errors, detected before any use of ctx's contents and
 * before anything is written to the outputs, deterministic: everything
 * gpuhash_first_below_batch refuses, and GPUHASH_EINVAL for a null out_totals, an out_off that
 * decreases, any cap_k > GPUHASH_COLLECT_MAX, and out_off[njobs] > 0 with a null out_nonces or
 * out_hashes.
 * Every nonce of every job is hashed, there is no early exit: afterwards
 * gpuhash_last_stats().nonces is the saturating sum of the jobs' spans and .launches every scan
 * launch that ran, re-runs included; gpuhash_last_launches gives one record per kernel variant per
 * context entry per sub-batch with `lo`, `hi` job indices as for gpuhash_min_batch, and every
 * launch of a re-run of job k carries lo == hi == k.  Threading, device-guard behaviour, errors and
 * the no-exception rule are as for gpuhash_min.  Replaces nothing in the reference (its protocol
 * has no target field). */
int gpuhash_collect_below_batch(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                                const uint64_t *lower, const uint64_t *upper, const uint64_t *target,
                                const size_t *out_off, uint64_t *out_nonces, uint64_t *out_hashes,
                                uint64_t *out_totals);

/* Same batch, caller-chosen work-item granularity (as gpuhash_min_ex). */
int gpuhash_collect_below_batch_ex(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *msg_off, size_t njobs,
                                   const uint64_t *lower, const uint64_t *upper, const uint64_t *target,
                                   uint32_t rchunk, const size_t *out_off, uint64_t *out_nonces,
                                   uint64_t *out_hashes, uint64_t *out_totals);

/* out[i] = Hash(msg, lower + i) for i < count, computed on the first device by the
 * SAME kernels as gpuhash_min (per-nonce dump mode).  count <= 2^26; lower + count - 1
 * must not wrap.  Parity/diagnostic API (batch form of hash.go:11-15). */
int gpuhash_hash_range(gpuhash_ctx *ctx, const uint8_t *msg, size_t msg_len,
                       uint64_t lower, uint64_t count, uint64_t *out);

/* bitcoin.Hash(msg, nonce) for ONE nonce on the host (hash.go:11-15): the miner's
 * optional self-check of a returned (hash, nonce); never used by gpuhash_min. */
uint64_t gpuhash_hash_cpu(const uint8_t *msg, size_t msg_len, uint64_t nonce);

/* Measurements of the last call on ctx. */
int gpuhash_last_stats(const gpuhash_ctx *ctx, gpuhash_stats *out);

/* Copies up to cap launch records of the last call; returns how many exist. */
int gpuhash_last_launches(const gpuhash_ctx *ctx, gpuhash_launch_record *out, int cap);

/* Stops the search in flight on ctx, and every search after it until gpuhash_resume.
 * Sets a LATCH on the context, not a one-shot signal: a cancel that arrives a microsecond before
 * the call starts is not lost (Go's context.Context and C++ stop tokens behave the same way).
 * May be called from any thread while another thread is inside any call on ctx; it takes no lock
 * and does not wait.  It is ONE lock-free atomic store and nothing else, so it is
 * async-signal-safe: gpuhash_cli and gpuhash_miner call it from their SIGINT / SIGTERM handlers.
 * Returns GPUHASH_OK, or GPUHASH_EINVAL for a null ctx.
 * While the latch is set every search entry point -- gpuhash_min, gpuhash_first_below,
 * gpuhash_collect_below, their three batches, all their _ex forms and gpuhash_hash_range --
 * returns GPUHASH_ECANCELED: the call in flight, promptly; callers queued on the context, when
 * their turn comes; and calls made later.  A cancelled call writes NOTHING to its outputs and
 * leaves gpuhash_last_stats / gpuhash_last_launches as any failed call leaves them.  Argument
 * errors still win: GPUHASH_EINVAL / GPUHASH_ETOOLONG are returned before the latch is looked at.
 * gpuhash_open, gpuhash_close, gpuhash_set_layout_policy, gpuhash_last_*, gpuhash_shard_range*
 * and gpuhash_hash_cpu ignore the latch.
 * How promptly: the thread that waits for the device polls the latch every 100 us (the default
 * GPUHASH_HOST_WAIT=poll) and, when it sees it, overwrites the work counters of the launches in
 * flight from a second stream, after which every resident workgroup finishes the piece it holds
 * and leaves: milliseconds, whatever the range.  The latch is also read at call
 * entry and before every slice, sub-batch and re-run.  Under GPUHASH_HOST_WAIT=stream or =event
 * the waiting thread sleeps inside the HIP runtime, so there the latch is honoured at those
 * launch boundaries ONLY: a cancel takes effect when the launches already enqueued have run.
 * Replaces nothing in the reference; it is what a Go miner needs to honour a context.Context. */
int gpuhash_cancel(gpuhash_ctx *ctx);

/* Clears the latch.  A call that has already observed the latch still returns
 * GPUHASH_ECANCELED; calls that start after gpuhash_resume returns run normally and are exact --
 * nothing of a cancelled run (drained counters, half-filled lists, thresholds) reaches a later
 * call: every call re-arms what it uses.  Any thread; no lock.  GPUHASH_EINVAL for a null ctx. */
int gpuhash_resume(gpuhash_ctx *ctx);

/* How far the search in flight on ctx is.  *out_total = the call's nonce count, saturating: the
 * span; for a batch the sum of the spans; for gpuhash_first_below the span too (not the
 * ascending-scan figure of gpuhash_last_stats).  *out_done = an estimate of the nonces whose work
 * has been HANDED OUT to the device: the nonces of the slices, sub-batches and launches that are
 * over, plus, for each launch now running, its nonces x the share of its work counter.  Within a
 * call it never decreases and never exceeds *out_total; a first-hit search that stops early ends
 * below it.  With no call in flight, or when the call ends before the answer is ready, both are 0.
 * May be called from any thread; it takes no lock that a search holds, so it does not wait for
 * the call as gpuhash_last_stats does.  The calling thread makes no HIP call: it posts a request,
 * and the call's waiting threads answer it from their poll loop with one copy of the counters
 * (about 0.1-0.3 ms).  A call nobody asks about enqueues nothing for it.  Under
 * GPUHASH_HOST_WAIT=stream or =event the answer is what is over at launch boundaries, at once.
 * Returns GPUHASH_OK, or GPUHASH_EINVAL for a null argument. */
int gpuhash_progress(gpuhash_ctx *ctx, uint64_t *out_done, uint64_t *out_total);

void gpuhash_close(gpuhash_ctx *ctx);

const char *gpuhash_strerror(int rc);

/* Library/ABI version, "gpuhash <major>.<minor> gfx950 build=<id>": <id> is a hash of
 * the sources the library was built from (bench.py matches it against profiled builds). */
const char *gpuhash_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GPUHASH_H */
