/* utmos_hip.h -- C ABI of libutmos_hip.so: greedy maximum-coverage selection on MI355X (gfx950).
 *
 * The reference (ACEnglish/utmos v2.2.0) has no FFI/plugin interface; its only seam for this
 * path is the Python call chain
 *
 *     run_selection   utmos/select.py:147-195
 *       greedy_select utmos/select.py:69-137   (generator; mutates sample_mask in place, :100)
 *         calculate_scores utmos/select.py:24-53  -> (idx, new_count) | (None, None)
 *
 * so the entry points below are what a ctypes binding inside utmos/select.py would call in place
 * of calculate_scores / greedy_select (INTEGRATION.md shows that binding).  Plain pointers and
 * sizes only; no Python, numpy or torch types.
 *
 * Conventions
 *   - every function returns 0 (UTM_OK) or a negative UTM_E* code; utm_last_error() gives the text
 *     of the last failure on the calling thread.
 *   - host buffers are borrowed for the duration of the call; device memory belongs to the context.
 *   - one context = one GPU = one contiguous shard [first_sample, first_sample + n_local) of the
 *     sample axis.  A context is not thread-safe; it owns one HIP stream.
 *   - the matrix is a list of *chunks* along the variant axis (the replacement for the reference's
 *     row-chunked hdf5 store, select.py:198-231).  Inside a chunk every sample is one column:
 *     W = ceil(n_var/64) little-endian uint64 words, variant v of the chunk = bit (v & 63) of word
 *     (v >> 6), zero padded.
 *   - sample states follow select.py:169-179: 1 selectable, 0 already used (covers), 2 excluded.  A used sample
 *     covers on EVERY shard: utm_reset fetches a remote one through the P2P mapping or an ncclBroadcast, and
 *     fails with UTM_ESTATE on a shard that has neither.
 *
 * Environment.  None of these changes a result; they move launch shapes and thresholds (tools/tune.py sweeps them)
 * or are test hooks.  ONE table in utmos_amd/csrc/utmos_hip.hip (g_knobs) names them all with defaults and ranges; a context
 * reads them at utm_ctx_create and again at every utm_reset (read_tune) and nowhere else, so nothing on the
 * per-iteration path touches the environment.  The first context of a process lists on stderr the ones that are set;
 * utm_env_overrides() returns the same list (bench.py reports it as `env_overrides`).
 *   Every knob has a legal range, written here as (default; range): lo..hi, "step" for a multiple, or {the values}.  A
 *   value outside it, or one that is not a number, is ignored -- the default holds -- and the first context of a process
 *   names it on stderr.
 *   UTM_TARGET_WGS (32768; 1..2^24)          workgroups a scoring launch aims for
 *   UTM_MIN_WGS (128; 0..2^24), UTM_MIN_WGS_BIG (8192; 0..2^24)       smallest grids the 8 KiB / 32 KiB tiles are used for
 *   UTM_TILE_STEPS (0; {0, 2, 4, 8, 16, 32})  force the covered tile to 32/16/8/4/2 KiB (0: by the grid)
 *   UTM_NT_LOADS (-1; -1..1)                 non-temporal column loads on/off (-1: by the matrix size)
 *   UTM_NT_MIN_MB (512; 0..2^24)             matrix size from which they are used
 *   UTM_SCORE_FORM (1; 0..1)                 integer launches at 32 / 16 KiB tiles: 0 = k_score_int (LDS tile), 1 = k_score_intq
 *   UTM_FUSE_PICK (1; 0..1)                  pick inside the scoring launch (one shard or mailbox exchange, integer scores)
 *   UTM_CHAIN_PICK (1; 0..1)                 AF with candidate chains: pick inside the chain launch (one shard)
 *   UTM_AF_VERIFY (1; 0..1)                  ... and candidates, compaction, chains and pick as stages of ONE launch (one shard)
 *   UTM_AF_RECORD (1; 0..1)                  AF: a chain's float64 sum stays on record per sample for as long as the sample's count does not change
 *   UTM_AF_DEFER (1; 0..1)                   AF, one shard: exact float64 scores of unambiguous winners are finished per batch from a
 *                             log of newly-covered masks (needs 64 columns + 8 bytes per variant of HBM; 0: chained on the spot)
 *   UTM_PICK_THREADS (0; 0..1024 step 64)    threads of the stand-alone k_pick (0: by the sample count)
 *   UTM_BATCH (0; 0..65536)                  iterations between host syncs (0: 256; AF 64)
 *   UTM_AF_STEPS (16; {16, 32}), UTM_AF_SWITCH (0.2; 0..2), UTM_AF_TARGET_WGS (16384; 1..2^24)   AF kernels: tile, dense->streaming switch, grid
 *   UTM_AF_TABLES (1; 0..1)                  the full dense AF pass as table lookups (k_score_aft) where every fixed-point value is below 2^45; 0: k_score_afq
 *   UTM_AF_TABLE_WGS_PER_CU (8; 1..1024), UTM_AF_TABLE_RUN (0; 0..65536)   ... its grid: workgroups per CU, or tiles per workgroup outright (0: by the grid)
 *   UTM_AF_DENSE_DELTA (0.05; 0..2)          AF delta passes take the LDS-tile kernel while the last winner newly covered more than this share of all variants
 *   UTM_DECR_FIRST_BATCH (8; 1..65536), UTM_DECR_INTERLEAVED (1; 0..1)   decremental mode: first batch size, second copy on/off
 *   UTM_P2P_REPLICATE (1; 0..1)              copy the peers' columns once (0: read winners in place over the mappings)
 *   UTM_TEST_REMOTE_WINNER (0; 0..1)         test hook: read local winners from the exchange's winner-column buffer too
 *   UTM_PERSISTENT (1; 0..1)                 integer scores (weighted or not) and the verified-parallel AF forms, one chunk, the only shard: a
 *                             batch of iterations as ONE persistent
 *                             launch (k_loop_int: workers keep their covered tile in LDS, the picker's record replaces the kernel
 *                             boundary, two batches per wave run ahead across the hand-off)
 *   UTM_PERSIST_MAX_MB (560; 0..2^24), UTM_PERSIST_MAX_SAMPLES (2560; 0..2^28), UTM_PERSIST_MAX_TILES (32; 1..4095)   largest matrix /
 *                             sample count run that way (0: no limit), and the tile count the tile size (8 / 16 / 32 / 64 KiB) is
 *                             chosen for; UTM_PERSIST_TILE_KIB (0; {0, 8, 16, 32, 64}) forces one; tiles above 8 KiB (columns taller
 *                             than 32 tiles) only up to UTM_PERSIST_TALL_MAX_SAMPLES (640; 0..2^28) samples.  A tile grid of more
 *                             tiles than the loop's arrival fields count (4,095; the AF forms 255) always keeps the launches
 *   UTM_PERSIST_WGS_PER_CU (0; 0..16)        resident 512-thread blocks per CU the grid is sized for (0: what the occupancy query allows)
 *   UTM_PERSIST_AHEAD_TICKS (400; 0..2^30), UTM_PERSIST_AHEAD0_TICKS (0; 0..2^30)   10 ns ticks before the next record is due at which a
 *                             wave requests its second / first run-ahead batch (0: as soon as it runs out of work)
 *   UTM_PERSIST_AF (1; 0..1)                 AF scores: the delta iterations run inside the persistent loop too -- float32 AF in its exact fixed-point
 *                             phase, and (UTM_PERSIST_AF_INTERVAL (1; 0..1)) float64 AF / float32 sums outside the exact range with score
 *                             intervals: the picker lists the candidates, UTM_PERSIST_CHAINERS (4; 1..8) blocks at the end of the grid
 *                             keep their sequential float64 sums on record, working ahead while iterations take longer than
 *                             UTM_PERSIST_SPEC_TICKS (1000; -2..2^30) x 10 ns (-1: only on request; -2: test hook, the chainers leave
 *                             and every request times out).  Both AF forms: 8 KiB tiles only, at most UTM_PERSIST_AF_MAX_TILES (26; 1..255)
 *   UTM_PERSIST_CLAIMS (1; 0..1)             positions behind a wave's two static ones are claimed from per-tile counters (0: dealt statically)
 *   UTM_MBOX_SPINS_LOG2 (24; 4..28)          mailbox exchange: polls (x ~0.5 us) before a peer's record is declared lost (UTM_ECOMM)
 *   UTM_TEST_MUTE_EXCHANGE (0; 0..INT_MAX)   test hook: in that iteration since the reset this shard posts no record into the mailboxes
 *   UTM_TEST_DROP_ARRIVAL (0; 0..INT_MAX)    test hook: in that scoring launch / persistent iteration since the reset one partial count is
 *                             withheld, so that the pick's bounded wait runs out (UTM_EHIP; the context works again after utm_reset)
 */
#ifndef UTMOS_HIP_H
#define UTMOS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UTM_OK 0
#define UTM_EINVAL (-1)   /* bad argument */
#define UTM_EHIP (-2)     /* HIP runtime error */
#define UTM_ENOMEM (-3)   /* allocation failed */
#define UTM_ESTATE (-4)   /* call not valid in the context's current state */
#define UTM_ECOMM (-5)    /* RCCL error / RCCL not available */

#define UTM_ABI_VERSION 3 /* 2: utm_stats.exchange / rccl_ranks; host-memory mailbox and replica entry points removed
                           * 3: utm_env_overrides; utm_stats.persist_launches / persist_iterations; utm_stream_calibration */

typedef struct utm_ctx utm_ctx;

/* AF value modes (utm_set_af).  F32 restates the reference's hdf5 store (float32 presence*AF,
 * select.py:218-223); F64 its in-memory matrix (float64, select.py:314-321). */
#define UTM_AF_NONE 0
#define UTM_AF_F32 1
#define UTM_AF_F64 2

/* utm_ctx_create flags */
#define UTM_FLAG_PROFILE_EVENTS 1u /* bracket every scoring launch with HIP events (utm_stats.score_ms) */
#define UTM_FLAG_AF_SEQUENTIAL 2u  /* never use the order-independent fixed-point form for F32 AF */
#define UTM_FLAG_DECREMENTAL 4u    /* allow decremental scoring (utm_set_decremental) */

/* One local-best record, as exchanged between shards (64 bytes). */
typedef struct utm_record {
    double score;      /* final (masked, weighted) score of the shard's best selectable sample */
    int64_t idx;       /* its GLOBAL sample index, or -1 when the shard has no selectable sample */
    int64_t new_count; /* variants it would newly capture (counts[use], select.py:49) */
    int64_t pad[5];
} utm_record;

typedef struct utm_stats {
    int64_t iterations;      /* greedy iterations completed since the last utm_reset */
    int64_t tot_captured;    /* running total of new_count */
    int64_t score_launches;  /* scoring-kernel launches since the last utm_reset */
    double score_ms;         /* summed HIP-event time of those launches (UTM_FLAG_PROFILE_EVENTS), else 0 */
    double loop_ms;          /* HIP-event time of the last utm_run or utm_apply_order (stream time, first launch to last) */
    int64_t algo_bytes;      /* algorithmic HBM bytes of the iterations since the last utm_reset */
    int32_t af_mode;         /* UTM_AF_* in effect */
    int32_t af_fixed_point;  /* AF estimate: 1 = int64 fixed point at a unit no AF value loses a bit to, 2 = coarser unit
                              * (mass would overflow: addends floored, intervals widened), 0 = sequential kernel */
    int32_t af_q;            /* fixed-point scale: scores = sum / 2^q */
    int32_t n_chunks;
    int64_t decr_iterations;   /* iterations scored decrementally (0 unless enabled) */
    int64_t brute_force_bytes; /* what full re-scoring of every iteration would have had to read */
    int64_t p2p_replica_bytes; /* HBM holding copies of the other shards' columns (utm_p2p_import; 0: read in place) */
    int64_t decr_interleaved_bytes; /* HBM held by the word-interleaved copy the decremental iterations stream (0: gather form) */
    int32_t exchange;        /* UTM_EXCHANGE_*: how utm_run's iterations meet the other shards */
    int32_t rccl_ranks;      /* ncclCommCount of the context's communicator, 0 without one */
    /* allele-frequency scoring, verified-parallel form, since the last utm_reset: */
    int64_t af_chained_iterations; /* iterations whose pick needed sequential float64 chains on the spot (near-ties) */
    int64_t af_deferred_rows;      /* rows whose exact float64 score was finished after their batch (one launch set per batch) */
    /* persistent loop (one chunk, the only shard; integer scores and the verified-parallel AF forms): batches of iterations run as ONE launch */
    int64_t persist_launches;      /* such launches since the last utm_reset (each counts once in score_launches) */
    int64_t persist_iterations;    /* rows they produced (0: every iteration was a launch of its own) */
    int64_t persist_unresolved;    /* launches (interval form of the AF loop) that left their last iteration to a verification launch */
    int64_t af_table_passes;       /* full dense AF passes (one per chunk) that ran as table lookups (k_score_aft) since the last utm_reset */
} utm_stats;

/* utm_stats.exchange */
#define UTM_EXCHANGE_NONE 0    /* the context holds every sample: nothing to exchange */
#define UTM_EXCHANGE_MAILBOX 1 /* 64-byte records through hipIpc-mapped device mailboxes; winner column read from a peer mapping / local copy */
#define UTM_EXCHANGE_RCCL 2    /* ncclAllGather of the records, then ncclBroadcast of the winner's column from its owner */
#define UTM_EXCHANGE_CALLER 3  /* a shard without a device-side exchange: the caller drives utm_local_best / utm_apply_records */
#define UTM_EXCHANGE_RCCL_SUM 4 /* RCCL, root-free: ncclAllGather of the records, then ncclAllReduce(sum) of a buffer that holds the winner's column on its owner and zeros elsewhere (utm_comm_column_by_allreduce) */

const char *utm_last_error(void);
int utm_abi_version(void);
int utm_device_count(int *n);
/* The UTM_* environment knobs that are set right now, as "NAME=value NAME=value" (empty string: none), into buf[cap].
 * A context reads the knobs when it is created and again at every utm_reset -- never inside the loop. */
int utm_env_overrides(char *buf, uint64_t cap);
/* Free and total HBM of a device in bytes (hipMemGetInfo): what the host's is_memsafe policy (select.py:56-63) asks. */
int utm_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- context ------------------------------------------------------------------------------ */
int utm_ctx_create(int device, uint32_t n_samp_total, uint32_t first_sample, uint32_t n_samp_local,
                   uint32_t flags, utm_ctx **out);
int utm_ctx_destroy(utm_ctx *ctx);

/* ---- matrix (select.py:275-321 builds the reference's; here it is built in HBM) -------------- */
/* Append an all-zero chunk of n_var variants; returns its index in *chunk. */
int utm_add_chunk(utm_ctx *ctx, uint64_t n_var, int32_t *chunk);
/* Upload n_cols whole columns of a chunk, local column first_col onwards.
 * cols[c * stride_words + w], stride_words >= ceil(n_var/64). */
int utm_upload_columns(utm_ctx *ctx, int32_t chunk, uint32_t first_col, uint32_t n_cols,
                       const uint64_t *cols, uint64_t stride_words);
/* Upload n_rows variants in the reference's own packing (numpy.packbits(axis=1), MSB first,
 * convert.py:85): rows[r * row_stride_bytes + (s >> 3)] bit (7 - (s & 7)) = GLOBAL sample s.
 * The bit transpose to column-major runs on the GPU.  first_var must be a multiple of 64. */
int utm_upload_rows_packed(utm_ctx *ctx, int32_t chunk, uint64_t first_var, uint64_t n_rows,
                           const uint8_t *rows, uint64_t row_stride_bytes);
int utm_download_columns(utm_ctx *ctx, int32_t chunk, uint32_t first_col, uint32_t n_cols,
                         uint64_t *cols, uint64_t stride_words);
/* Per-sample carrier totals over all chunks (var_count, select.py:281-284), n_samp_local values. */
int utm_var_count(utm_ctx *ctx, int64_t *out);
/* Seeded synthetic chunk contents generated on the GPU (bench/test input, DESIGN.md "Synthetic input"). */
int utm_synth_fill(utm_ctx *ctx, int32_t chunk, uint64_t seed, uint64_t first_var_global);
/* The same generator on the host (no GPU call): columns of samples [first, first+n) and/or per-variant AF. */
int utm_synth_host(uint64_t seed, uint64_t first_var_global, uint64_t n_var, uint32_t n_samp_total,
                   uint32_t first_sample, uint32_t n_samp, uint64_t *cols, uint64_t stride_words,
                   float *af_out);

/* ---- scoring options ------------------------------------------------------------------------ */
/* state[n_samp_total]: 1 selectable / 0 used / 2 excluded.  Implies utm_reset. */
int utm_set_sample_state(utm_ctx *ctx, const uint8_t *state);
/* weights[n_samp_total] (select.py:181-187) or NULL for none.  Must be finite. */
int utm_set_weights(utm_ctx *ctx, const double *weights);
/* Per-variant AF of one chunk: mode UTM_AF_F32 (const float*) or UTM_AF_F64 (const double*), n_var
 * values, finite and >= 0.  All chunks must use the same mode.  UTM_AF_NONE with af == NULL clears. */
int utm_set_af(utm_ctx *ctx, int32_t chunk, int mode, const void *af);

/* ---- the greedy loop ------------------------------------------------------------------------ */
/* Restart: covered := OR of the columns of all used (state 0) samples, local or not; tot_captured := 0. */
int utm_reset(utm_ctx *ctx);
/* One iteration = calculate_scores (select.py:24-53) + the winner update (select.py:99-100).
 * *idx = global sample index or -1 for the reference's (None, None). */
int utm_step(utm_ctx *ctx, int64_t *idx, int64_t *new_count, double *score);
/* Up to k_max iterations, device resident; stops like greedy_select (select.py:93-96, :110-112).
 * Outputs need k_max entries (score_out may be NULL); *n_done = rows produced. */
int utm_run(utm_ctx *ctx, int64_t k_max, int64_t *idx_out, int64_t *new_out, double *score_out,
            int64_t *n_done);
/* Select the given samples in the given order, without scoring anyone else: new_out[i] = variants sample
 * global_idx[i] newly captures after the ones before it (and after whatever is covered already).  Each becomes
 * used (state 0), leaves act[], and its columns are ORed into covered; iterations and tot_captured advance.
 * Stops like greedy_select after the row that captures the last variant: *n_done rows are valid, and only those
 * samples become used.  A row whose new count is 0 is still a row.  Valid after utm_reset, before or between
 * utm_run / utm_step calls.  The following utm_run continues as if those samples had been state 0 at the reset.
 * One streaming pass over the listed columns (k_order_curve), one launch per chunk.
 * UTM_EINVAL, with the context untouched, for NULL arguments, an index out of range, a duplicate in the list or a
 * sample that is already used; excluded (state 2) samples are accepted.  UTM_ESTATE on a context that holds only a
 * shard of the samples or has an exchange set up.  n == 0 is a no-op that returns 0 rows. */
int utm_apply_order(utm_ctx *ctx, const int64_t *global_idx, int64_t n, int64_t *new_out, int64_t *n_done);
/* With a depth M > 1 (utm_set_depth): one k_depth_apply launch per listed sample and chunk; new_out = the units gained,
 * and the rows end after the one that makes tot_captured = M x variants. */
/* The walk of k_order_curve built for the CPU: cols[s * wp + w] of one chunk, covered[wp] (updated in place), a list
 * of n column indices; counts[i] += what column order[i] newly covers.  Needs no GPU. */
int utm_order_curve_host(const uint64_t *cols, uint64_t wp, uint64_t *covered, const uint32_t *order, uint64_t n,
                         uint64_t *counts);
/* ---- capture ranks ---------------------------------------------------------------------------- */
/* For a list of samples and a depth m in 1..255: rank_out[v] = the smallest i such that m of the samples
 * global_idx[0..i] carry variant v of the chunk, or -1 when the list never gets there (m = 1: the position of v's first
 * carrier).  One int32 per variant answers every prefix panel of the list at once: a panel of the first k samples
 * captures the variants with 0 <= rank < k.  rank_out takes the chunk's n_var values.  One streaming pass over the
 * listed columns of the chunk (k_capture_rank), one launch; *pass_ms = its HIP-event time (may be NULL).
 * Stateless: it reads the chunk's columns and nothing else, and starts from an empty mask whatever the context's states
 * are -- covered, the depth planes, the sample states, the rows, a pending winner, utm_stats and everything the loop
 * caches are neither read nor changed, so a utm_run before or after it is unaffected.  Valid any time after the chunk's
 * columns are uploaded.  Used and excluded samples are accepted in the list.  Rows cleared by an AF of 0 (utm_set_af)
 * have no carriers: -1.  n == 0: all -1.
 * UTM_EINVAL, with rank_out untouched, for a NULL global_idx with n > 0, a NULL rank_out, a chunk or an index out of
 * range, a duplicate in the list, or m outside 1..255.  UTM_ESTATE on a context that holds only a shard of the samples
 * or has an exchange set up, as utm_apply_order. */
int utm_capture_rank(utm_ctx *ctx, int32_t chunk, const int64_t *global_idx, int64_t n, int32_t m,
                     int32_t *rank_out /* n_var of the chunk */, double *pass_ms /* may be NULL */);
/* The walk of k_capture_rank built for the CPU: cols[s * wp + w] of one chunk holding n_var <= 64 * wp variants, a list
 * of n column indices, a depth m in 1..255; rank_out[n_var] as above.  Needs no GPU. */
int utm_capture_rank_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, const uint32_t *order, uint64_t n,
                          int32_t m, int32_t *rank_out);
/* ---- swap gains ------------------------------------------------------------------------------- */
/* For a panel of k samples: gain_out[i * n_samp_total + t] = F(panel - panel[i] + t) - F(panel) for every sample t, where
 * F = the number of variants (summed over all chunks) that some member carries -- what every exchange of ONE member for
 * ONE other sample would capture, the move of a 1-swap local search.  gain = g_t + x[i][t] - u_i with u_i = the variants
 * only member i carries (unique_out[i]: what the panel loses without it), g_t = the variants t carries and no member does
 * (new_out[t]) and x[i][t] = the variants t carries of those u_i.  No special case: t = panel[i] gives 0, another member
 * gives -u_i.  *base_out = F(panel).  Two launches per chunk (k_swap_masks: one pass over the panel's columns;
 * k_swap_pairs: the bit-matrix product of k + 1 masks with every column); *pass_ms = their HIP-event time.
 * Stateless, exactly as utm_capture_rank: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats and everything the loop caches are neither read nor changed.  Used and
 * excluded samples are accepted, as members and as candidates.  Rows cleared by an AF of 0 (utm_set_af) have no carriers.
 * k == 0: *base_out = 0 and nothing else is written.
 * UTM_EINVAL, with the outputs untouched, for a NULL panel or a NULL gain_out with k > 0, an index out of range or a
 * duplicate in the panel.  UTM_ESTATE on a context that holds only a shard of the samples or has an exchange set up. */
int utm_swap_gains(utm_ctx *ctx, const int64_t *panel, int64_t k,
                   int64_t *gain_out   /* k * n_samp_total, row i = panel[i] leaves */,
                   int64_t *unique_out /* k: u_i, may be NULL */,
                   int64_t *new_out    /* n_samp_total: g_t, may be NULL */,
                   int64_t *base_out   /* F(panel), may be NULL */,
                   double *pass_ms     /* may be NULL */);
/* The arithmetic of the two kernels built for the CPU: cols[s * wp + w] of ONE chunk holding n_var <= 64 * wp variants
 * of n_samp samples, a panel of k column indices; the outputs as above.  Needs no GPU. */
int utm_swap_gains_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp,
                        const uint32_t *panel, uint64_t k, int64_t *gain_out, int64_t *unique_out,
                        int64_t *new_out, int64_t *base_out);
/* ---- pair counts ------------------------------------------------------------------------------- */
/* For a list of n samples: out[i * n + j] = the variants (summed over all chunks) that global_idx[i] and global_idx[j]
 * both carry and no sample of `given` carries; the diagonal is each sample's own count under that mask.  Symmetric.
 * Per chunk one k_swap_masks launch over the `given` columns (none without a `given` list: there is no mask then) and
 * one k_pair_counts launch: a bit-matrix product of the list with itself over 64 x 64 block pairs, both operands staged
 * in LDS, only the blocks on and above the diagonal computed.  *pass_ms = the launches' HIP-event time.
 * tile_groups: 0 = automatic (about 8,192 workgroups over the block pairs); above 0 = that many groups of 4 KiB variant
 * tiles per block pair, clamped to the tile count and raised where a workgroup would walk more than 32,768 tiles.  It
 * moves the launch shape only and never changes a result.
 * Stateless, exactly as utm_swap_gains: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats and everything the loop caches are neither read nor changed.  Used and
 * excluded samples are accepted in both lists; a sample in both has an all-zero row.  Rows cleared by an AF of 0
 * (utm_set_af) have no carriers.  n == 0 writes nothing.
 * UTM_EINVAL, with `out` untouched, for a NULL list with a nonzero length, a NULL out with n > 0, an index out of range or
 * a duplicate within either list.  UTM_ENOMEM when the n x n device buffer cannot be had.  UTM_ESTATE on a context that
 * holds only a shard of the samples or has an exchange set up. */
int utm_pair_counts(utm_ctx *ctx, const int64_t *global_idx, int64_t n,
                    const int64_t *given, int64_t n_given /* may be NULL / 0 */,
                    uint32_t tile_groups                  /* 0: automatic */,
                    int64_t *out                          /* n * n */,
                    double *pass_ms                       /* may be NULL */);
/* The arithmetic of the two kernels built for the CPU: cols[s * wp + w] of ONE chunk holding n_var <= 64 * wp variants
 * of n_samp samples (padding bits zero), a list of n and a `given` list of n_given column indices; out as above.
 * Needs no GPU. */
int utm_pair_counts_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp,
                         const uint32_t *idx, uint64_t n, const uint32_t *given, uint64_t n_given, int64_t *out);
/* ---- carrier counts ----------------------------------------------------------------------------- */
/* For a list of n samples: hist_out[c] = the number of variants of the chunk that exactly c of the samples global_idx[]
 * carry and no sample of `given` carries -- the site-frequency spectrum of the list, beyond the `given` panel.  The sum
 * of hist_out is the chunk's n_var minus the variants a `given` sample carries.  count_out[v] = the number of listed
 * samples that carry variant v, or -1 where a `given` sample carries it.  Either output may be NULL, not both.
 * One k_swap_masks launch over the `given` columns (none without a `given` list: the mask is then the chunk's valid
 * bits) and one streaming pass over the listed columns (k_carrier_counts): the counts live in registers as bit planes,
 * 16 columns are folded in at a time by carry-save adders, bins 0..7 are popcounts of plane combinations and only the
 * variants with a higher count are decoded one by one.  *pass_ms = the launches' HIP-event time.
 * hist_mode: 0 = automatic, 1 = the decoded variants meet in LDS bins first (n + 1 <= 4,096 bins), 2 = they go to the
 * global bins directly.  It moves the launch shape only and never changes a result.
 * Stateless, exactly as utm_capture_rank: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats and everything the loop caches are neither read nor changed.  Used and
 * excluded samples are accepted in both lists; a sample in both contributes nothing, because its variants are masked.
 * Rows cleared by an AF of 0 (utm_set_af) have no carriers: they fall in bin 0.  n == 0: hist_out[0] is everything not
 * masked.
 * UTM_EINVAL, with both outputs untouched, for a NULL list with a nonzero length, both outputs NULL, a chunk or an index
 * out of range, a duplicate within either list, hist_mode above 2 or 1 with more than 4,096 bins, or n above 2^20 - 1.
 * UTM_ESTATE on a context that holds only a shard of the samples or has an exchange set up. */
int utm_carrier_counts(utm_ctx *ctx, int32_t chunk, const int64_t *global_idx, int64_t n,
                       const int64_t *given, int64_t n_given /* may be NULL / 0 */,
                       uint32_t hist_mode                    /* 0 automatic, 1 LDS bins, 2 global bins */,
                       int64_t *hist_out                     /* n + 1, written (not added to); may be NULL */,
                       int32_t *count_out                    /* n_var of the chunk; may be NULL */,
                       double *pass_ms                       /* may be NULL */);
/* The arithmetic of the kernels built for the CPU, block of 16 columns by block: cols[s * wp + w] of ONE chunk holding
 * n_var <= 64 * wp variants of n_samp samples (padding bits zero), a list of n and a `given` list of n_given column
 * indices; hist_out[n + 1] and count_out[n_var] as above.  Needs no GPU. */
int utm_carrier_counts_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp,
                            const uint32_t *idx, uint64_t n, const uint32_t *given, uint64_t n_given,
                            int64_t *hist_out, int32_t *count_out);
/* ---- group curves ------------------------------------------------------------------------------- */
#define UTM_GROUPS_MAX 64
/* For a group id per sample (group_of[s] in 0..n_groups-1, or -1 = in no group) and a list of n samples: with U_g = the
 * variants of the chunk that some sample of group g carries, multi = the variants in two or more U_g and P_g = U_g &
 * ~multi (the group's private variants; ungrouped samples play no part in it),
 *     new_out[g * n + j]  = the variants of U_g whose first carrier in the list is global_idx[j] (utm_capture_rank == j
 *                           at m = 1): what the sample at position j adds to group g's captured variants,
 *     priv_out[g * n + j] = the same over P_g,
 *     total_out[g] = |U_g|, ptotal_out[g] = |P_g|.
 * A group's never-captured count is total - sum_j new.  A group id without samples has an empty U_g.  The list may hold
 * ungrouped samples.  Two launches: k_group_unions, one pass over the columns of all grouped samples (sorted by group on
 * the host) that writes the G union masks and multi and sums the totals; k_group_curve, the walk of k_capture_rank at
 * m = 1 over the list, which reads the masks only where a position captures something.  *pass_ms = the launches'
 * HIP-event time.  n == 0: only the first launch, only the totals are written.  priv_out == NULL: the private bins are
 * not computed and multi is not read by the second launch.
 * bin_mode: 0 = automatic, 1 = the first positions of the list meet in LDS bins (as many as 8,192 bins hold for
 * n_groups, or twice n_groups with priv_out, bin rows; the rest go to the global bins), 2 = global bins only.  It moves
 * the launch shape only and never changes a result.
 * Stateless, exactly as utm_capture_rank: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats and everything the loop caches are neither read nor changed.  Used and
 * excluded samples are accepted.  Rows cleared by an AF of 0 (utm_set_af) have no carriers.
 * UTM_EINVAL, with every output untouched, for a NULL group_of or total_out, a NULL global_idx or new_out with n > 0,
 * n_groups outside 1..64, a group id outside -1..n_groups-1, a chunk or an index out of range, a duplicate in the list,
 * or bin_mode above 2.  UTM_ENOMEM when the (n_groups + 1) x wp mask buffer cannot be had.  UTM_ESTATE on a context that
 * holds only a shard of the samples or has an exchange set up. */
int utm_group_curve(utm_ctx *ctx, int32_t chunk, const int32_t *group_of /* n_samp_total */, int32_t n_groups,
                    const int64_t *global_idx, int64_t n, uint32_t bin_mode /* 0 automatic, 1 LDS head, 2 global only */,
                    int64_t *new_out    /* n_groups * n */,
                    int64_t *priv_out   /* same, may be NULL */,
                    int64_t *total_out  /* n_groups */,
                    int64_t *ptotal_out /* n_groups, may be NULL */,
                    double *pass_ms     /* may be NULL */);
/* The arithmetic of the two kernels built for the CPU, word by word: cols[s * wp + w] of ONE chunk holding n_var <=
 * 64 * wp variants of n_samp samples (padding bits zero), group_of[n_samp], a list of n column indices; the outputs as
 * above.  Needs no GPU. */
int utm_group_curve_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp,
                         const int32_t *group_of, int32_t n_groups, const uint32_t *order, uint64_t n,
                         int64_t *new_out, int64_t *priv_out, int64_t *total_out, int64_t *ptotal_out);
/* ---- class counts ------------------------------------------------------------------------------- */
#define UTM_CLASSES_MAX 16384
/* For a class label per variant of the chunk (class_of[v] in 0..n_classes-1, or -1 = counted nowhere) and a list of
 * samples: table_out[j * n_classes + c] = the number of variants of class c that sample global_idx[j] carries.  With
 * class = utm_capture_rank's rank it is every sample's own capture curve under any panel, with class =
 * utm_carrier_counts' count every sample's own frequency spectrum.  n == 0 (global_idx may be NULL): every sample of the
 * matrix, in index order, n_samp_total rows; otherwise n rows.  The table is written, not added to.
 * One launch (k_class_counts) over a grid of (variant tile groups, blocks of min(16, 16384 / n_classes) listed columns):
 * a workgroup keeps its columns' bins in LDS, walks the set bits of every column word, looks the variant's label up and
 * adds 1 to the (column, class) bin, and leaves with one 64-bit atomic per non-zero bin.  The work beyond the column loads
 * is bounded by the set bits, whatever n_classes is.  *pass_ms = the launch's HIP-event time.
 * tile_groups: 0 = automatic (about 8,192 workgroups over the column blocks); above 0 = that many groups of 4 KiB variant
 * tiles per column block, clamped to the tile count and raised where a workgroup would walk more than 32,768 tiles.
 * mode: 0 = automatic, 1 = the bit walk, 2 = reserved for a form that popcounts the most populous classes in front of
 * the walk, which is not built: it runs the walk too.  Both move the launch shape only and never change a result.
 * Stateless, exactly as utm_capture_rank: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats and everything the loop caches are neither read nor changed.  Used and
 * excluded samples are accepted in the list.  Rows cleared by an AF of 0 (utm_set_af) have no carriers: they are counted
 * for no sample.
 * UTM_EINVAL, with table_out untouched, for a NULL class_of or table_out, a NULL list with a nonzero length, n_classes
 * outside 1..16,384, a label outside -1..n_classes-1, a chunk or an index out of range, a duplicate in the list, mode
 * above 2, or more than 65,535 column blocks.  UTM_ENOMEM when the device buffers (the labels, the n x n_classes table)
 * cannot be had.  UTM_ESTATE on a context that holds only a shard of the samples or has an exchange set up, as
 * utm_apply_order. */
int utm_class_counts(utm_ctx *ctx, int32_t chunk, const int32_t *class_of /* n_var of the chunk */, int32_t n_classes,
                     const int64_t *global_idx, int64_t n /* NULL / 0: every sample, in index order */,
                     uint32_t tile_groups /* 0: automatic */,
                     uint32_t mode        /* 0 automatic, 1 walk only, 2 reserved (walks) */,
                     int64_t *table_out   /* n_rows * n_classes, written (not added to) */,
                     double *pass_ms      /* may be NULL */);
/* The kernel's arithmetic built for the CPU, word by word: cols[s * wp + w] of ONE chunk holding n_var <= 64 * wp
 * variants of n_samp samples (padding bits zero), class_of[n_var], a list of n column indices (NULL / 0: every column in
 * index order); table_out as above.  Needs no GPU. */
int utm_class_counts_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const int32_t *class_of,
                          int32_t n_classes, const uint32_t *idx, uint64_t n, int64_t *table_out);
/* ---- variant filters ----------------------------------------------------------------------------- */
/* Keep only the variants of one chunk whose bit is set in keep[] (ceil(n_var/64) words, variant v = bit v&63 of word
 * v>>6; bits at or above n_var are ignored).  Kept variants keep their order.  Every local column is compacted, the
 * chunk's AF values (either mode) with it; wp shrinks to the new count's padded width, padding is zero.  *n_kept (may be
 * NULL) may be 0: the chunk stays in the list, index unchanged, with no variants (and one zero KiB per column).  What the
 * reference offers instead is filtering the VCF (bcftools view) before `utmos convert` and converting again.
 * Out of place: the compacted columns are written into a new block (k_filter_prefix: exclusive prefix of the keep words'
 * popcounts; k_filter_compact: parallel-suffix compress of every word, the pieces merged in LDS), then the old block is
 * freed -- peak memory is the matrix plus one chunk.  UTM_ENOMEM, with the chunk untouched, when that does not fit.
 * Afterwards the chunk is in the state utm_add_chunk + an upload of the kept rows + utm_set_af of the kept values would
 * have left: covered, the depth planes, the decremental copy, the AF tables and everything else derived from the old
 * columns are dropped and built again by the utm_reset this call implies.  utm_var_count counts the columns as they are
 * now (rows an earlier utm_set_af cleared for an AF of 0 stay cleared).  A mask that keeps everything changes nothing but
 * still restarts the loop.  A filtered chunk can be filtered again.  *pass_ms (may be NULL): HIP-event time of the two
 * launches and the zero fill of the new block.
 * UTM_EINVAL for a chunk out of range or a NULL keep.  UTM_ESTATE once the columns are exported (utm_p2p_export /
 * utm_p2p_import / utm_comm_init): the peers have mapped the old column bases.  A shard context before that is fine --
 * the mask is the same for every shard. */
int utm_filter_variants(utm_ctx *ctx, int32_t chunk, const uint64_t *keep, uint64_t *n_kept, double *pass_ms);
/* The same word arithmetic on the host, no GPU call: cols[c * wp + w] holding n_var <= 64 * wp variants of n_cols columns
 * -> out[c * wp_out + w], written whole (padding zero); *n_kept (may be NULL) = the kept count, which must fit wp_out
 * words.  What it replaces: as utm_filter_variants. */
int utm_filter_columns_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_cols,
                            const uint64_t *keep, uint64_t *out, uint64_t wp_out, uint64_t *n_kept);
/* ---- replicated selection ------------------------------------------------------------------------ */
/* n_rep (1..256) greedy selections at once, each over its own subset of the variants and with its own sample states:
 * replicate b is exactly what utm_set_sample_state(state + b * n_samp_total), utm_reset and utm_run(k) give on the matrix
 * reduced to the variants of its keep mask (delete-half resampling of the variants, per-class panels, leave-one-out runs).
 * The columns of a replicate's used samples (state 0) are covered from its start and used samples are never picked;
 * excluded samples (state 2) are never picked; every row takes the first maximum of popcount(column & live_b), the smallest
 * sample index among the maxima; a replicate ends silently when its best score is 0, and after the row that captures its
 * last kept variant.  order_out[b * k + i] = the global sample index of replicate b's row i (-1 after its last row),
 * new_out[b * k + i] = the variants that row newly captured (0 after the last row), kept_out[b] = the replicate's
 * variants, n_done[b] = its rows.
 * keep[chunk][b * W + w], W = ceil(n_var / 64) words of that chunk: the replicate's variants (bits at or above n_var are
 * ignored).  keep == NULL: hashed masks -- variant v, counted from 0 over all chunks in order, belongs to replicate b iff
 * (z >> 32) < keep_threshold with z = seed + 0x9E3779B97F4A7C15 * (v + 1) + 0xD1B54A32D192ED03 * (b + 1), z = (z ^ z >> 30)
 * * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^= z >> 31 (mod 2^64); a threshold of 2^32 keeps
 * everything.  They are made on the device (k_multi_keep); utm_multi_keep_host is the same function on the host.
 * Per chunk one k_multi_init launch (live_b = keep_b & valid & ~OR(columns of b's used samples)); per iteration and
 * chunk k_multi_score, the bit-matrix product of the n_rep live masks with every column (the shape of k_swap_pairs, the
 * mask rows read from the live buffer), and k_multi_apply (live_b &= ~column of b's winner), with one k_multi_pick in
 * between.  The k iterations are enqueued without a host round trip per iteration; every launch returns at once when no
 * replicate is left, and the host looks every 32 iterations.  *pass_ms = the launches' HIP-event time.
 * Stateless, exactly as utm_swap_gains: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats, the working views and the list views are neither read nor changed.  The
 * outputs are staged in memory of the call and copied out last.  Rows cleared by an AF of 0 (utm_set_af) have no carriers.
 * UTM_EINVAL, with the outputs untouched, for n_rep outside 1..256, k < 0, a NULL state or output, a state byte above 2 or
 * a NULL entry in keep.  UTM_ENOMEM when the n_rep x (words per column) live masks or the n_rep x n_samp_total scores
 * cannot be had.  UTM_ESTATE on a context that holds only a shard of the samples or has an exchange set up, as
 * utm_apply_order. */
int utm_multi_select(utm_ctx *ctx, uint32_t n_rep,
                     const uint8_t *state,            /* n_rep * n_samp_total: 1 selectable / 0 used / 2 excluded */
                     const uint64_t *const *keep,     /* n_chunks pointers, each n_rep * ceil(n_var/64) words; NULL: hashed masks */
                     uint64_t seed, uint64_t keep_threshold,   /* used when keep == NULL */
                     int64_t k,
                     int32_t *order_out,              /* n_rep * k global sample indices, -1 after a replicate's last row */
                     int64_t *new_out,                /* n_rep * k, 0 after the last row */
                     int64_t *kept_out,               /* n_rep: variants of the replicate (kept bits below n_var, all chunks) */
                     int64_t *n_done,                 /* n_rep: rows written */
                     double *pass_ms);                /* may be NULL */
/* The kernels' arithmetic built for the CPU, replicate by replicate: cols[s * wp + w] of ONE chunk holding n_var <= 64 * wp
 * variants of n_samp samples (padding bits zero), state[n_rep * n_samp], keep[n_rep * ceil(n_var/64)]; the outputs as
 * above.  Needs no GPU. */
int utm_multi_select_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, uint32_t n_rep,
                          const uint8_t *state, const uint64_t *keep, int64_t k,
                          int32_t *order_out, int64_t *new_out, int64_t *kept_out, int64_t *n_done);
/* The hashed mask of replicate `rep` for the n_var variants from global index first_var_global on: ceil(n_var/64) words,
 * bits at or above n_var zero.  Needs no GPU. */
int utm_multi_keep_host(uint64_t seed, uint32_t rep, uint64_t first_var_global, uint64_t n_var,
                        uint64_t keep_threshold, uint64_t *words);
/* ---- coverage bound ------------------------------------------------------------------------------ */
/* A certified upper bound on what ANY panel of k of the candidate samples can capture beyond the `given` samples, by
 * Lagrangian relaxation of maximum coverage.  For multipliers lambda_v in [0, 1] and any k columns S,
 *     F(S) <= sum_v (1 - lambda_v) + (the k largest column sums s_j = sum_{v in j} lambda_v) = L(lambda),
 * and `iters` projected subgradient steps on L approach the LP bound.  lambda is 16-bit fixed point, Q = 65,536 = 1.0, so
 * everything is an integer.  live = the valid variant bits & ~OR(columns of `given`), over all chunks; lambda_v = Q on the
 * live variants at the start.  For t = 0 .. iters - 1:
 *   s_j   = sum of lambda_v over the live variants column cand[j] carries (int64, all chunks);
 *   P_t   = the min(k, n_cand) positions j with the largest s_j, ties to the smaller position in cand;
 *   L_t   = sum_live (Q - lambda_v) + sum_{j in P_t} s_j                                   -> hist_out[t];
 *   c_v   = the j in P_t whose column carries v;   eta_t = max(1, step0 >> min(63, t / period));
 *   lambda_v <- min(Q, max(0, lambda_v - eta_t * (c_v - 1))) for every live v.
 * *n_live_out = the live variants, *bound_out = min(n_live, min_t floor(L_t / Q)), *best_iter_out = the first t at that
 * minimum; hist_out[0] / Q is the trivial bound, the k largest live column counts.  lambda_out[chunk][v] = lambda after the
 * last update, 0 where v is not live.  The call is deterministic: the lambda behind best_iter is what iters = best_iter
 * returns.  step0 == 0: Q / 4; period == 0: max(1, iters / 14).  cand == NULL with n_cand == 0: every sample, in index order.
 * Per chunk one k_swap_masks launch (the live mask, as utm_pair_counts) and one k_bound_init; per iteration and chunk
 * k_bound_sums (every candidate column once, 4-variant nibble tables of lambda in LDS) and k_bound_update (the picked
 * columns into bit-plane counters, the clamp update, the next constant term), with one single-workgroup k_bound_pick in
 * between.  All iterations are enqueued at once; the history comes back once at the end.  *pass_ms = their HIP-event time.
 * Stateless, exactly as utm_swap_gains: it reads the columns and nothing else -- covered, the depth planes, the sample
 * states, the rows, a pending winner, utm_stats, the working views and the list views are neither read nor changed.  Used
 * and excluded samples are accepted in both lists; a sample in both has no live variants.  Rows cleared by an AF of 0
 * (utm_set_af) have no carriers: such a row stays live at lambda = Q and adds nothing.
 * UTM_EINVAL, with the outputs untouched, for a NULL hist_out, a NULL list with a nonzero length, an index out of range, a
 * duplicate within either list, k < 1, iters outside 1..65,535, step0 above 65,536 or a NULL entry in lambda_out.
 * UTM_ENOMEM when the lambda, mask or sum buffers cannot be had.  UTM_ESTATE on a context that holds only a shard of the
 * samples or has an exchange set up, as utm_apply_order. */
int utm_coverage_bound(utm_ctx *ctx, const int64_t *cand, int64_t n_cand,   /* NULL / 0: every sample, index order */
                       const int64_t *given, int64_t n_given,               /* may be NULL / 0 */
                       int64_t k, int32_t iters, uint32_t step0, uint32_t period,   /* 0: defaults */
                       int64_t *hist_out      /* iters values L_t */,
                       int64_t *bound_out, int32_t *best_iter_out, int64_t *n_live_out,   /* each may be NULL */
                       uint32_t *const *lambda_out /* n_chunks pointers of n_var each, or NULL */,
                       double *pass_ms /* may be NULL */);
/* ms_out[3] = the summed HIP-event times of the last utm_coverage_bound's k_bound_sums, k_bound_pick and k_bound_update
 * launches; zeros unless the context was created with UTM_FLAG_PROFILE_EVENTS. */
int utm_coverage_bound_times(utm_ctx *ctx, double *ms_out);
/* The same arithmetic built for the CPU: cols[s * wp + w] of ONE chunk holding n_var <= 64 * wp variants of n_samp samples
 * (padding bits zero); lambda_out[n_var] or NULL; the other outputs as above.  Needs no GPU. */
int utm_coverage_bound_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const uint32_t *cand, uint64_t n_cand,
                            const uint32_t *given, uint64_t n_given, int64_t k, int32_t iters, uint32_t step0, uint32_t period,
                            int64_t *hist_out, int64_t *bound_out, int32_t *best_iter_out, int64_t *n_live_out, uint32_t *lambda_out);
/* Scores of the NEXT iteration without selecting: counts[n_local] (new variants per local sample,
 * 0 for non-selectable) and final scores[n_local].  Either may be NULL.  Parity/debug aid. */
int utm_peek_scores(utm_ctx *ctx, int64_t *counts, double *scores);
/* AF modes in fixed point (utm_stats.af_fixed_point != 0): the same, from the PARALLEL full pass the loop's first iteration
 * runs (k_score_aft / k_score_afq / k_score_afs) instead of the sequential chains -- scores[s] = int64 sum * 2^-q (* weight),
 * which IS the reference's float64 sum wherever the sums are exact (float32 AF, lossless unit, below 2^53 units).
 * UTM_ESTATE otherwise.  Parity/debug aid: what the tests compare the first pass with. */
int utm_peek_estimates(utm_ctx *ctx, int64_t *counts, double *scores);
/* Current covered mask of a chunk (all pending updates applied), ceil(n_var/64) words.  With a depth M > 1 this is the
 * mask the scoring uses: the variants whose support has reached M. */
int utm_get_covered(utm_ctx *ctx, int32_t chunk, uint64_t *out);
int utm_get_stats(utm_ctx *ctx, utm_stats *out);
/* ---- coverage depth (set multicover) ----------------------------------------------------------- */
/* Every variant counts until m selected samples carry it: with support(v) = the number of used samples that carry v the
 * loop maximises F = sum_v min(support(v), m), so a sample's count is popcount(column & ~saturated) -- the scoring kernels
 * as they are, with `covered` = the mask of variants whose support has reached m.  m = 1 (the default) is the plain
 * selection: nothing is allocated and no other kernel runs.  m > 1 keeps bit_length(m) bit planes per chunk (plane p =
 * bit p of every variant's support, the word layout of covered); k_depth_apply adds the winner's column after every
 * pick, and every iteration is a full scoring pass: the persistent loop, decremental scoring, AF delta passes and
 * deferred AF scores are off while m > 1 (utm_stats: persist_iterations, decr_iterations and af_deferred_rows stay 0).
 * new_count = units gained, tot_captured = F, and the loop ends after the row that makes F = m x variants or when the
 * best score is 0.  Samples that start out used (state 0) add support at utm_reset, in index order, without counting
 * towards tot_captured.  Rows cleared by an AF of 0 have no carriers: their support stays 0 and they are in no sum.
 * Valid before utm_reset (implies one).  UTM_EINVAL outside 1..255; m > 1 on a context that holds a shard of the samples
 * or has an exchange set up: UTM_ESTATE, as utm_apply_order. */
int utm_set_depth(utm_ctx *ctx, int32_t m);
/* *m = the depth in effect; *apply_launches = k_depth_apply launches since the last utm_reset, *apply_ms their summed
 * HIP-event time (UTM_FLAG_PROFILE_EVENTS, else 0).  Any output may be NULL. */
int utm_get_depth(utm_ctx *ctx, int32_t *m, int64_t *apply_launches, double *apply_ms);
/* out[i] = the number of variants with support >= m after row first_row + i (rows of utm_run / utm_step /
 * utm_apply_order since the last utm_reset; used samples of the reset included in the count).  UTM_ESTATE at m = 1. */
int utm_get_at_depth(utm_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *out);
/* Per-variant support (0..m) of a chunk, n_var bytes, decoded from the planes (m = 1: the covered bit). */
int utm_get_support(utm_ctx *ctx, int32_t chunk, uint8_t *out);
/* k_depth_apply's word arithmetic built for the CPU: one column col[wp] into covered[wp] and planes[p * wp + w],
 * p < bit_length(m), updated in place (covered must be the mask support == m of the planes); *units += the units gained,
 * *newly_saturated += the variants that reached m.  Needs no GPU. */
int utm_depth_apply_host(const uint64_t *col, uint64_t wp, uint64_t *covered, uint64_t *planes, int32_t m, uint64_t *units,
                         uint64_t *newly_saturated);
/* Decremental scoring: after a full scoring pass, later iterations only subtract the
 * contribution of the variants the last winner newly covered (counts and fixed-point AF sums stay exact;
 * same rows).  Reads far fewer bytes than the brute-force loop, so it is off by default and its numbers
 * are reported separately from the brute-force roofline.  When free HBM allows, the context keeps a
 * second, word-interleaved copy of the matrix (rows_t[word][sample]) for these iterations: a newly
 * covered word is then one contiguous read over all samples instead of one 8-byte gather per column
 * (utm_stats.decr_interleaved_bytes; UTM_DECR_INTERLEAVED=0 or lack of room keeps the gather form).
 * threshold = largest fraction of a column's words that may be newly covered for an iteration to go
 * decremental (<= 0: default -- 1.0 with the interleaved copy, 0.2 gathering). */
int utm_set_decremental(utm_ctx *ctx, int32_t on, double threshold);
/* AF modes: the winner of an iteration is always the reference's (sample order, new_count are exact).  The reported
 * *score* is, by default (on = 1), also the reference's float64 running sum bit for bit, which costs one sequential
 * chain per iteration whenever the parallel sum is not provably exact.  on = 0 skips that chain when the winner is
 * unambiguous and reports the parallel estimate (relative error <= 2^-24 + n 2^-53) -- what a caller that only
 * writes the reference's TSV columns needs.  Ambiguous iterations (ties within the error bound) are always chained,
 * and so is everything on a context that holds only a shard of the samples (its records meet other shards'). */
int utm_set_af_exact_scores(utm_ctx *ctx, int32_t on);
/* Streaming-read calibration: `launches` plain read-only passes over the context's resident columns with the scoring
 * kernel's access shape (16 B per lane non-temporal loads, 1 KiB per wave instruction, 8 in flight, ~32k workgroups) and
 * nothing else -- *gbps_out = bytes read / stream time.  What the box delivers today, beside the 8 TB/s spec peak: the bench
 * reports it as roofline.stream_calibration_gbps so that box-to-box variance can be told from kernel quality. */
int utm_stream_calibration(utm_ctx *ctx, int32_t launches, double *gbps_out);
/* ---- working views of the integer loop ---------------------------------------------------------- */
/* Integer scores on the only shard (no AF, depth 1, not decremental, no exchange): at a batch boundary the loop may go on
 * scoring a copy of the columns compacted to the variants that are still uncovered -- same rows bit for bit, fewer bytes per
 * iteration.  The first copy of a run is made from the chunk, every later one from the copy before it (two column blocks,
 * used in turn), and a pass moves only the columns of the samples that are still selectable.
 * mode 0 = off, 1 = on (the default).  min_vars = 0 and ratio <= 0 (the default): the library decides by cost -- a chunk is
 * compacted at a batch boundary while one iteration still streams more than stream_bytes from what the loop scores
 * (selectable samples x bytes per column; what the Infinity Cache would serve is left alone) and the bytes the next batch
 * would read for nothing exceed pass_cost x the bytes of the pass.  min_vars > 0 or ratio > 0: a chunk of V working
 * variants is compacted when V >= min_vars and at most ratio x V of them are uncovered (the one left at 0 stands for 2^21 /
 * 0.5); ratio must be below 1.
 * The chunks, utm_get_covered and every other entry point see the matrix as it was uploaded.  The call itself drops any
 * view in use (the buffers stay).  The blocks are allocated at the first and the second compaction, kept across utm_reset
 * and freed with the context; if the first does not fit half of the free HBM the context never compacts
 * (utm_compaction_stats.refused), if the second does not, the chunk keeps the view it has for that run (view_refused). */
int utm_set_compaction(utm_ctx *ctx, int32_t mode, uint64_t min_vars, double ratio);
typedef struct utm_compaction_stats {
    int64_t compactions;    /* compaction passes since the last utm_reset */
    uint64_t working_vars;  /* variants per column in what the loop scores now, summed over chunks */
    int64_t pass_bytes;     /* HBM bytes of the compaction and covered-flush passes (part of utm_stats.algo_bytes) */
    double pass_ms;         /* ... and their HIP-event time */
    int32_t refused;        /* the copy did not fit half of the free HBM */
    int32_t mode;
    uint64_t min_vars;      /* 0 and 0.0: the library's policy by cost */
    double ratio;
    int64_t log_iter[16];   /* the first 16 passes: rows out when the pass ran, */
    uint64_t log_vars[16];  /* variants kept by it, */
    double log_ms[16];      /* its time (measuring what was left included) */
    int64_t view_passes;    /* the passes among `compactions` that read the view before them, not the chunk */
    int64_t view_refused;   /* times a view's other block did not fit half of the free HBM: the chunk kept its view */
    uint64_t stream_bytes;  /* the library's own policy: bytes per iteration below which a view is left alone, */
    double pass_cost;       /* and what a pass byte costs in scoring bytes */
    int32_t log_src[16];    /* the first 16 passes: 0 = read the chunk, 1 = read a view */
} utm_compaction_stats;
int utm_get_compaction_stats(utm_ctx *ctx, utm_compaction_stats *out);
/* ---- list views of the integer loop -------------------------------------------------------------- */
/* Beside a working view that a compaction pass has just written, the loop may keep every still selectable column as lists
 * of its set positions (tile-local 32-bit entries in per-tile segments) and score those: an iteration then reads 4 bytes
 * per carrier instead of one bit per variant -- same rows bit for bit.  A list is built after a pass when
 * 4 x (the previous winner's gain) x ratio <= 8 x (words per column of the new view) and one iteration of the new view
 * streams more than min_stream_bytes; once a run has a list, every later pass rebuilds it.  While a list is valid the
 * loop runs one launch per iteration.  mode 0 = off, 1 = on (the default); min_stream_bytes = 0 and ratio = 0 stand for
 * the defaults (1 GiB, 2.0), other values are taken as given.  The call drops any list in use (the views stay).  The entry
 * buffer of a chunk is allocated at its first build within half of the free HBM, kept across utm_reset and freed with
 * the context; a build that does not fit leaves the chunk on its bitmap view for that run (utm_list_stats.refused). */
int utm_set_list_mode(utm_ctx *ctx, int32_t mode, uint64_t min_stream_bytes, double ratio);
/* Test hook: tile_log2 = 13, 16, 18 or 20 fixes the tile of every build (0: the library's rule); max_entries > 0 refuses a
 * build of more padded entries than that, as if the buffer had not fitted. */
int utm_set_list_test(utm_ctx *ctx, int32_t tile_log2, uint64_t max_entries);
typedef struct utm_list_stats {
    int64_t builds;          /* list builds since the last utm_reset */
    int64_t refused;         /* builds refused: no room, or more tiles than a count word can count */
    int64_t build_bytes;     /* HBM bytes of the builds (part of utm_stats.algo_bytes) */
    double build_ms;         /* ... and their HIP-event time */
    int32_t mode;
    int32_t valid;           /* chunks whose list view is valid now */
    uint64_t min_stream_bytes;
    double ratio;
    int64_t log_iter[16];    /* the first 16 builds: rows out when the build ran, */
    int32_t log_tiles[16];   /* tiles, */
    int32_t log_t[16];       /* log2 of the tile's positions, */
    uint64_t log_entries[16];/* entries, */
    uint64_t log_padded[16]; /* entries with the segments' padding, */
    double log_ms[16];       /* time */
    int64_t log_bytes[16];   /* and HBM bytes */
} utm_list_stats;
int utm_get_list_stats(utm_ctx *ctx, utm_list_stats *out);
/* The shape of the launches that score a list.  A wave walks one segment with all 64 lanes, or -- for a build whose mean
 * segment is at most 64 quads of entries -- four segments at once, 16 lanes each; the launches of such a build aim at a
 * workgroup target of their own.  lanes = 16 or 64 fixes the form of every build from the next one on (a list in use
 * keeps its form; tiles of 2^18 and 2^20 positions have the 64-lane form only), 0 = the library's rule.  target_wgs =
 * 1 .. 65536 replaces the target of the 16-lane launches from the next launch on, 0 = the library's.  Anything else is
 * UTM_EINVAL and changes nothing.  The call drops nothing and the rows are the same bit for bit; the setting outlives
 * utm_reset. */
int utm_set_list_shape(utm_ctx *ctx, int32_t lanes, int32_t target_wgs);
/* For the first 16 builds since the last utm_reset (as utm_list_stats.log_*): lanes[k] = the lanes that share a segment in
 * the launches of build k, as decided once at the build (64 for a tile without the 16-lane form, whatever was asked);
 * wgs[k] = the scoring workgroups of its first launch (0: none yet); *n = builds reported.  lanes and wgs hold 16 values
 * each. */
int utm_get_list_shape(utm_ctx *ctx, int32_t *lanes, int32_t *wgs, int32_t *n);
/* Switch per-launch HIP-event timing of the scoring kernels on/off (same as UTM_FLAG_PROFILE_EVENTS). */
int utm_set_profile(utm_ctx *ctx, int32_t on);

/* ---- sharded operation: building blocks for any transport ------------------------------------- */
/* Score locally and report this shard's best candidate; nothing is selected. */
int utm_local_best(utm_ctx *ctx, utm_record *rec);
/* Words per sample summed over chunks (length of a whole-column buffer). */
int utm_column_words(utm_ctx *ctx, uint64_t *n_words);
/* Concatenated chunk columns of a LOCAL sample (global index), utm_column_words() words. */
int utm_get_column(utm_ctx *ctx, int64_t global_idx, uint64_t *out);
/* Apply one exchanged decision: recs[n_ranks] are all shards' records in rank order; the winner is
 * chosen exactly as the fused path does (score desc, index asc).  winner_col is the winner's whole
 * column, or NULL when the winner is local to this context.  Outputs as utm_step. */
int utm_apply_records(utm_ctx *ctx, const utm_record *recs, int32_t n_ranks, const uint64_t *winner_col,
                      int64_t *idx, int64_t *new_count, double *score);

/* ---- P2P column access (optional; utm_comm_init sets it up by itself) ---------------------------- */
/* Every shard can map the other shards' columns (hipIpc) and read a remote winner's column in place
 * instead of receiving it: export one blob per shard, hand all shards' blobs (rank order) to import.
 * Afterwards utm_apply_records accepts winner_col == NULL for remote winners. */
int utm_p2p_blob_bytes(utm_ctx *ctx, uint64_t *n_bytes);
int utm_p2p_export(utm_ctx *ctx, void *blob);
int utm_p2p_import(utm_ctx *ctx, int32_t rank, int32_t n_ranks, const void *blobs);
/* Record mailboxes: with the mappings in place the shards can also exchange their per-iteration records on
 * the device (remote stores into each other's uncached mailbox slots, bounded polling) -- no collective and no
 * host in the loop.  utm_p2p_selftest is collective (every shard calls it): *ok = 1 when this shard received
 * every peer's test record.  If ALL shards report 1, call utm_p2p_use_mailboxes(ctx, 1) on every shard; utm_run
 * is then collective over the shards exactly like after utm_comm_init. */
int utm_p2p_selftest(utm_ctx *ctx, int32_t *ok);
/* on = 1: as above.  on = 2: also on a context that is the ONLY shard (exported to and imported from itself): it then posts
 * to and collects from its own mailbox every iteration -- the exchange's own per-iteration cost, measurable on one GPU
 * (bench.py --force-mailboxes).  on = 0: off. */
int utm_p2p_use_mailboxes(utm_ctx *ctx, int32_t on);
/* ---- RCCL (one process per GPU; ids are exchanged by the caller) ------------------------------ */
#define UTM_UNIQUE_ID_BYTES 128
int utm_comm_get_unique_id(void *id);
/* One communicator per context, one rank per GPU.  After this utm_step / utm_run / utm_reset are collective over
 * the ranks and one greedy iteration is SURVEY.md 8e's protocol:
 *   local scoring + local best  ->  ncclAllGather of the 64-byte records (RCCL has no MAXLOC; every rank then takes
 *   the same maximum: score descending, global index ascending = np.argmax's first maximum, select.py:48)
 *   ->  ncclBroadcast of the winner's column (W x 8 bytes per chunk) from the rank that owns it  ->  every rank ORs
 *   it into its covered replica while it stages the next scoring pass.
 * The broadcast's root is known on the host only after the decision, so this mode synchronises the stream once per
 * iteration.  If the record mailboxes are also enabled (utm_p2p_use_mailboxes) they carry the loop and the
 * communicator is left to utm_comm_allreduce_max; utm_stats.exchange says which.  Samples that start out used
 * (state 0) on another rank are broadcast by their owner at utm_reset. */
int utm_comm_init(utm_ctx *ctx, int32_t rank, int32_t n_ranks, const void *id);
int utm_comm_allreduce_max(utm_ctx *ctx, double *value); /* in place; also a barrier */
/* How the winner's column travels in the RCCL exchange.  0 (default): ncclBroadcast from its owner -- the root is
 * data dependent, so the host reads it after every iteration (one stream sync per iteration).  1: the owner puts the
 * column into the winner-column buffer, everybody else zeros, and one ncclAllReduce(sum, uint64) leaves the column
 * on every rank -- about twice the bytes on the links, but no root and therefore no host in the loop (iterations are
 * enqueued in batches like on one GPU).  Same rows either way. */
int utm_comm_column_by_allreduce(utm_ctx *ctx, int32_t on);

/* ---- VCF genotype parsing (no utm_ctx) ---------------------------------------------------------- */
/* The genotype half of the reference's `convert` (utmos/convert.py:43-88; utmos_amd/vcfio.py restates it on the CPU):
 * VCF record text -> per record the packed presence row (numpy.packbits order, MSB = lowest sample, convert.py:85-86;
 * present = het or hom-alt of a fully called call of ploidy >= 2, convert.py:64-70), AF = largest alt-allele count /
 * called alleles (convert.py:75-77), the record's het / hom-alt cell counts (convert.py:64-69) and its singleton flag
 * (counts[1] == 1 or counts[0] == 1, convert.py:58-61).  The caller strips the header (## lines, #CHROM) and inflates.
 * A context holds two batch slots, each with its own stream, so the host can fill one while the GPU parses the other. */
#define UTM_VCF_MAX_SAMPLES 524288u          /* the presence row of one record lives in LDS (64 KiB) */
#define UTM_VCF_MAX_BATCH 4294967232ull      /* 2^32 - 64: offsets inside a batch are 32-bit */
#define UTM_VCF_SINGLETON 1u                 /* utm_vcf_fetch flags: the record is a singleton (convert.py:58-61) */
#define UTM_VCF_SKIPPED 2u                   /* ... a `##` line or an empty line among the records: not a variant */
typedef struct utm_vcf utm_vcf;
int utm_vcf_create(int device, uint32_t n_samples, uint64_t batch_bytes, utm_vcf **out);
int utm_vcf_destroy(utm_vcf *vcf);
/* Pinned staging of the slot the next utm_vcf_parse uses, grown to at least n_bytes (contents kept): the caller may
 * read or inflate the batch straight into it.  *cap = its size. */
int utm_vcf_staging(utm_vcf *vcf, uint64_t n_bytes, uint8_t **buf, uint64_t *cap);
/* Queue one batch: n_bytes of whole records, the last one ending in '\n' (CR before it is dropped).  text may be the
 * staging buffer (no copy) or any host memory.  Returns once the text is on the device and the parse is queued;
 * *n_records = lines in the batch (skipped lines included).  At most two batches wait for utm_vcf_fetch. */
int utm_vcf_parse(utm_vcf *vcf, const uint8_t *text, uint64_t n_bytes, uint64_t *n_records);
/* Wait for the oldest queued batch and copy its results out: rows[n_records * ceil(S/8)], af, n_het, n_hom and flags
 * (UTM_VCF_*) per line.  A malformed record (fewer than ten columns, a sample count other than the header's, no GT,
 * an allele token that is neither `.` nor an unsigned decimal, more than 4096 alt alleles, #CHROM among the records)
 * fails the batch with UTM_EINVAL naming its line in the batch; the context stays usable. */
int utm_vcf_fetch(utm_vcf *vcf, uint8_t *rows, double *af, uint32_t *n_het, uint32_t *n_hom, uint8_t *flags);
/* HIP-event time summed over the fetched batches: ms[0] host-to-device text, ms[1] kernels, ms[2] device-to-host results. */
int utm_vcf_timing(utm_vcf *vcf, double *ms);
/* BGZF batches inflated on the device.  `packed` holds n_members whole BGZF members back to back (it may be the staging
 * of utm_vcf_staging: no copy); members[2 i] = member i's size in bytes (BSIZE + 1), members[2 i + 1] its ISIZE.  The
 * text of the batch is: the carry of the previous batch, then prefix[0, prefix_bytes) (the first batch: the text after
 * the header, inflated by the caller), then the members' text.  Records are cut at the last newline; the bytes after it
 * (*carry_bytes; the whole batch when it has no newline) stay on the device and open the next batch.  flags:
 * UTM_BGZF_FIRST starts a file (drops any carry), UTM_BGZF_LAST ends it (a final record without a newline gets one).
 * Every member is checked (block structure, CRC32, ISIZE); a bad one fails the call with UTM_EINVAL and
 * utm_last_error() = "member <i> of the batch: <reason>", and the context stays usable.  Otherwise as utm_vcf_parse. */
#define UTM_BGZF_FIRST 1u
#define UTM_BGZF_LAST 2u
int utm_vcf_parse_bgzf(utm_vcf *vcf, const uint8_t *prefix, uint64_t prefix_bytes, const uint8_t *packed,
                       uint64_t packed_bytes, const uint32_t *members, uint64_t n_members, uint32_t flags,
                       uint64_t *n_records, uint64_t *carry_bytes);
/* BCF2 batches on the same context: the genotype half of the reference's `convert` (utmos/convert.py:43-88) for the
 * records of a BCF stream (DESIGN §8.4 states the format subset; utmos_amd/bcfio.py restates the reader on the CPU).
 * The caller reads the header (magic, l_text, the header text) and resolves gt_key, GT's index in the header
 * dictionary.  The text of the batch is: the carry of the previous batch, then prefix[0, prefix_bytes) (the first
 * batch: the stream bytes after the header that the caller already holds), then either n_members whole BGZF members
 * (`packed`, `members` as in utm_vcf_parse_bgzf, inflated and checked on the device) or, with n_members = 0,
 * packed[0, packed_bytes) as stream bytes the caller has inflated (`packed` may be the staging: no copy).  The device
 * follows the records' length prefixes; *n_records whole records are parsed, and the bytes after the last of them
 * (*carry_bytes: a prefix of fewer than 8 bytes, or a record that runs past the batch) stay on the device and open the
 * next batch.  UTM_BGZF_FIRST starts a file (drops any carry); with UTM_BGZF_LAST a non-empty carry fails the call with
 * UTM_EINVAL and "truncated record ...".  A bad member fails the call as in utm_vcf_parse_bgzf.  A bad record
 * (l_shared below 24, an n_sample other than the context's, more than 4096 alt alleles, a FORMAT field that runs past
 * l_indiv, an unknown type code, a GT field of a non-integer type, no GT field) fails its batch at utm_vcf_fetch with
 * UTM_EINVAL and "record <i> of the batch: <reason>".  The context stays usable either way.  utm_vcf_fetch returns
 * the same per-record outputs as for VCF (no record is ever flagged UTM_VCF_SKIPPED). */
int utm_vcf_parse_bcf(utm_vcf *vcf, const uint8_t *prefix, uint64_t prefix_bytes, const uint8_t *packed,
                      uint64_t packed_bytes, const uint32_t *members, uint64_t n_members, uint32_t gt_key,
                      uint32_t flags, uint64_t *n_records, uint64_t *carry_bytes);
/* The device's BCF record walk and genotype decode built for the CPU (utmos/convert.py:43-88 for BCF input, as
 * utm_vcf_parse_bcf): stream[0, n_bytes) = the bytes after the header.  *n_records = whole records, *carry_bytes = the
 * bytes after the last of them.  With every output NULL only these two are set; otherwise rows[n_records * ceil(S/8)],
 * af, n_het, n_hom and flags receive what utm_vcf_fetch would return (max_records = their room), and a bad record
 * fails the call with UTM_EINVAL and "record <i> of the batch: <reason>".  Needs no GPU. */
int utm_bcf_parse_host(const uint8_t *stream, uint64_t n_bytes, uint32_t n_samples, uint32_t gt_key,
                       uint64_t max_records, uint8_t *rows, double *af, uint32_t *n_het, uint32_t *n_hom,
                       uint8_t *flags, uint64_t *n_records, uint64_t *carry_bytes);
/* The kernel time of utm_vcf_timing (its ms[1]) in two parts, summed over the fetched batches: ms[0] finding the
 * records (VCF: the newline count and scan; BCF: k_bcf_chain), ms[1] parsing them (VCF: the newline offsets and
 * k_vcf_parse; BCF: k_bcf_parse). */
int utm_vcf_kernel_timing(utm_vcf *vcf, double *ms);
/* HIP-event time of the BGZF inflate kernels summed over the fetched batches (ms[0]). */
int utm_vcf_inflate_timing(utm_vcf *vcf, double *ms);
/* The device's BGZF member decoder built for the CPU: one whole member (gzip header to trailer) -> its text, at most
 * out_cap bytes of it copied to out.  *status = 0 when the member is good (structure, CRC32, ISIZE), else a nonzero
 * code in bits 0-7; bits 8.. hold the bytes decoded.  Needs no GPU. */
int utm_bgzf_inflate_host(const uint8_t *member, uint64_t member_bytes, uint8_t *out, uint64_t out_cap,
                          uint32_t *status);

/* ---- DEFLATE encoding (no utm_ctx) ------------------------------------------------------------- */
/* A raw DEFLATE stream (RFC 1951) compressed on the GPU, for the zlib stream of a joblib part file: the input is cut
 * into 64 KiB segments at stream offsets, each compressed on its own (fresh 32 KiB window, one dynamic-Huffman block,
 * or stored blocks when they are smaller).  Every segment but the last ends byte-aligned with an empty stored block
 * (zlib's Z_SYNC_FLUSH); the last sets BFINAL.  Levels 1..9 set the match search effort (csrc/deflate.hip.h).  The
 * caller writes the zlib header and the Adler-32 trailer (utm_deflate_adler).  The bytes depend only on the input, the
 * level and the segment borders: utm_deflate_host produces the same bytes on the CPU. */
#define UTM_DEFLATE_MAX_BATCH 1073741824ull  /* 2^30 input bytes per batch */
#define UTM_DEFLATE_LAST 1u                  /* utm_deflate_push: the batch ends the stream */
typedef struct utm_deflate utm_deflate;
/* *bound = the most raw-deflate bytes n_bytes of input can take: n + 15 per started 64 KiB segment (at least one). */
int utm_deflate_bound(uint64_t n_bytes, uint64_t *bound);
/* A context for batches of up to batch_bytes (rounded up to a multiple of 64 KiB) at one level. */
int utm_deflate_create(int device, uint64_t batch_bytes, int level, utm_deflate **out);
int utm_deflate_destroy(utm_deflate *deflate);
/* The pinned staging buffer (*cap = the batch size): a caller may fill it and pass it to utm_deflate_push (no copy). */
int utm_deflate_staging(utm_deflate *deflate, uint8_t **buf, uint64_t *cap);
/* Queue one batch of the stream: in[0, n_bytes) (the staging or any host memory).  A batch without UTM_DEFLATE_LAST
 * must be a multiple of 64 KiB; the last one may be any size up to the batch, 0 included.  Returns once the input is on
 * the device and the kernels are queued (the staging may be filled again).  At most two batches wait for
 * utm_deflate_pull.  After a UTM_DEFLATE_LAST batch the next push starts a new stream.  A bad argument changes
 * nothing. */
int utm_deflate_push(utm_deflate *deflate, const uint8_t *in, uint64_t n_bytes, uint32_t flags);
/* Wait for the oldest pushed batch: *out = its compressed bytes in pinned memory, valid until the push after next;
 * *out_bytes = their count (at most utm_deflate_bound of the batch). */
int utm_deflate_pull(utm_deflate *deflate, const uint8_t **out, uint64_t *out_bytes);
/* *adler = the Adler-32 of the current stream's pulled batches (after its last batch: the zlib trailer, big-endian). */
int utm_deflate_adler(utm_deflate *deflate, uint32_t *adler);
/* HIP-event time summed over the pulled batches: ms[0] host-to-device input, ms[1] kernels, ms[2] device-to-host output,
 * ms[3] the part of ms[1] spent in the serial parse (k_deflate_parse). */
int utm_deflate_timing(utm_deflate *deflate, double *ms);
/* The device encoder built for the CPU: in[0, n_bytes) as one whole stream at `level` -> out (the same bytes the device
 * produces), *out_bytes and the stream's Adler-32.  An out_cap below the output fails with UTM_EINVAL and writes
 * nothing past out_cap.  Needs no GPU. */
int utm_deflate_host(const uint8_t *in, uint64_t n_bytes, int level, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_bytes, uint32_t *adler);

/* ---- HDF5 store chunks (no utm_ctx) ------------------------------------------------------------ */
/* The `data` dataset of the reference's `--lowmem` store (utmos/select.py:198-229): chunks of whole rows, every column,
 * LZF-compressed by h5py (filter 32000) or stored raw, cells of one byte (bool / int8 / uint8) or four (float32
 * GT * AF).  utmos_amd/h5store.py reads the file's structure; the chunks are decoded and packed on the device
 * (csrc/lzf.hip.h).  A context is made for one dataset's chunk shape (chunk_rows x n_cols cells of itemsize bytes)
 * and holds two batch slots, each with its own stream, so the host reads one batch from the file while the GPU
 * decodes the other. */
#define UTM_H5_MAX_STAGE 2147479552ull        /* 2^31 - 4096 stored bytes per batch */
#define UTM_H5_MAX_CHUNKS 65536u              /* chunks per batch */
#define UTM_H5_MAX_CHUNK_BYTES 2147418112ull  /* 2^31 - 2^16 decoded bytes per chunk */
#define UTM_LZF_E_INPUT 1                     /* chunk status: a token runs past the stored bytes */
#define UTM_LZF_E_OUTPUT 2                    /* ... more output than the chunk holds (a raw chunk: larger than it) */
#define UTM_LZF_E_SHORT 3                     /* ... less output than the chunk holds (a raw chunk: smaller than it) */
#define UTM_LZF_E_BACKREF 4                   /* ... a back-reference before the start of the chunk */
#define UTM_H5_E_VALUES 5                     /* ... float32: a row's nonzero cells differ, or one is negative or NaN */
typedef struct utm_h5 utm_h5;
int utm_h5_create(int device, uint64_t stage_bytes, uint32_t max_chunks, uint32_t chunk_rows, uint32_t n_cols,
                  uint32_t itemsize, utm_h5 **out);
int utm_h5_destroy(utm_h5 *h5);
/* The pinned staging buffer (*cap = stage_bytes): a caller may read a batch into it and pass it to utm_h5_decode. */
int utm_h5_staging(utm_h5 *h5, uint8_t **buf, uint64_t *cap);
/* Queue one batch of n_chunks chunks: chunk i's stored bytes are in[offsets[i], offsets[i] + sizes[i]) (any
 * alignment; `in` is the staging, no copy, or any host memory), masks[i] its HDF5 filter mask (bit 0: stored raw, then
 * sizes[i] must be the chunk's decoded size), rows[i] its rows below the end of the dataset, which are packed
 * (a partial last chunk is stored full size).  sizes[i] == 0: the chunk is absent and reads as zeros.  Returns once
 * the batch is on the device and the kernels are queued (the staging may be filled again).  At most two batches wait
 * for utm_h5_fetch. */
int utm_h5_decode(utm_h5 *h5, const uint8_t *in, uint64_t n_bytes, const uint64_t *offsets, const uint64_t *sizes,
                  const uint32_t *masks, const uint32_t *rows, uint32_t n_chunks);
/* Wait for the oldest batch and copy out: rows[sum(rows) * ceil(n_cols / 8)] in numpy.packbits order (cell 0 = MSB of
 * byte 0), for itemsize 4 af[sum(rows)] (the row's common nonzero value, 0 for an all-zero row), and status[n_chunks]
 * (0 or UTM_LZF_E_* / UTM_H5_E_VALUES; the rows of a chunk whose status is not 0 are undefined). */
int utm_h5_fetch(utm_h5 *h5, uint8_t *rows, float *af, uint32_t *status);
/* HIP-event time summed over the fetched batches: ms[0] host-to-device, ms[1] decode, ms[2] pack, ms[3] device-to-host. */
int utm_h5_timing(utm_h5 *h5, double *ms);
/* The device's LZF decoder built for the CPU: one chunk in[0, n_in) -> out[0, n_out).  *status = 0 when it decodes to
 * exactly n_out bytes, else a UTM_LZF_E_* code (out is then partly written).  Needs no GPU. */
int utm_lzf_decode_host(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t n_out, uint32_t *status);

/* ---- HDF5 store chunks, written (no utm_ctx) ---------------------------------------------------- */
/* The writer side: packbits rows -> the stored chunks of the `data` dataset as h5py writes them (chunk_rows x n_cols
 * cells of itemsize bytes: 1 = h5py's bool, 4 = float32 GT * AF), LZF-compressed with the parse of h5py's filter, or
 * raw (filter mask bit 0) where the compressed chunk would not fit in the chunk's own size (csrc/lzf_enc.hip.h).
 * utmos_amd/h5write.py writes the file around them.  Two batch slots, each with its own stream. */
#define UTM_H5W_MAX_BATCH_BYTES 4294901760ull /* 2^32 - 2^16 cell bytes per batch (max_chunks x chunk bytes) */
typedef struct utm_h5w utm_h5w;
int utm_h5w_create(int device, uint32_t chunk_rows, uint32_t n_cols, uint32_t itemsize, uint32_t max_chunks,
                   utm_h5w **out);
int utm_h5w_destroy(utm_h5w *h5w);
/* The pinned staging buffer (*cap = max_chunks x chunk_rows x ceil(n_cols / 8) bytes): a caller may fill it with
 * packbits rows and pass it to utm_h5w_encode (no copy). */
int utm_h5w_staging(utm_h5w *h5w, uint8_t **buf, uint64_t *cap);
/* Queue one batch: rows[n_rows * ceil(n_cols / 8)] in numpy.packbits order (the staging or any host memory), for
 * itemsize 4 af[n_rows] (float32; the cells are float32(GT) * af).  1 <= n_rows <= max_chunks x chunk_rows; the batch
 * is ceil(n_rows / chunk_rows) chunks, the last one zero-padded to full size unless n_rows fills it.  Returns once the
 * rows are on the device and the kernels are queued.  At most two batches wait for utm_h5w_fetch.  A bad argument
 * changes nothing. */
int utm_h5w_encode(utm_h5w *h5w, const uint8_t *rows, const float *af, uint64_t n_rows);
/* Wait for the oldest batch: *out = its chunks' stored bytes back to back in pinned memory (valid until the next
 * utm_h5w_fetch), *out_bytes = their count, *n_chunks = the batch's chunks, sizes[*n_chunks] their stored bytes and
 * masks[*n_chunks] their HDF5 filter masks (0: LZF, 1: raw).  sizes and masks take max_chunks entries. */
int utm_h5w_fetch(utm_h5w *h5w, const uint8_t **out, uint64_t *out_bytes, uint32_t *sizes, uint32_t *masks,
                  uint32_t *n_chunks);
/* HIP-event time summed over the fetched batches: ms[0] host-to-device, ms[1] cells, ms[2] encode (scan and gather
 * included), ms[3] device-to-host. */
int utm_h5w_timing(utm_h5w *h5w, double *ms);
/* The device's LZF encoder built for the CPU (liblzf's full hash table; the same bytes): in[0, n_in) -> out, at most
 * out_cap bytes.  *out_bytes = the compressed size, or 0 when it would not fit in out_cap (h5py's filter runs with
 * out_cap = n_in and stores such a chunk raw).  Needs no GPU. */
int utm_lzf_encode_host(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UTMOS_HIP_H */
