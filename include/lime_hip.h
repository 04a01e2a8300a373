/*
 * lime_hip.h -- C ABI of liblime_hip.so: the MI355X (gfx950) implementation of LiME's
 * alpha-cluster detection + read x genome similarity accumulation hot path.
 *
 * The reference (veronicaguerrini/LiME) has no library or FFI surface: its boundary is
 * process + argv + files (src/ClusterLCP.cpp:56-71, src/ClusterBWT_DA.cpp:496-529).  The
 * entry points below are what a binding of that path would call; each names the reference
 * code it replaces.  The drop-in executables `ClusterLCP` and `ClusterBWT_DA`
 * (lime_amd/csrc/cli_*.cpp) are thin argv/file shells over this ABI, and
 * INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain C types; no exceptions cross the ABI; every function returns LIME_OK
 * or a negative code, with text in lime_last_error(); one lime_ctx per device per process;
 * calls on one ctx are not thread-safe.  All files/arrays are little-endian, headerless:
 *   lcp  u32[N]  lcp[i] = LCP(suffix i-1, suffix i), lcp[0] = 0
 *   da   u32[N]  document id; ids < n_reads are reads, the others genomes (id - n_reads)
 *   ebwt u8[N]   symbol preceding suffix i
 *   sim  u8[n_reads * n_refs] row-major, sums modulo 256 (Tools.h:68 dataTypeSim = uchar)
 * There is NO CPU fallback: without a usable HIP device lime_init fails.
 */
#ifndef LIME_HIP_H
#define LIME_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIME_OK            0
#define LIME_ERR_ARG      (-1)  /* bad argument (NULL, misaligned, out-of-range cluster, ...) */
#define LIME_ERR_HIP      (-2)  /* HIP runtime error / no device                              */
#define LIME_ERR_NOMEM    (-3)  /* host or device allocation failed                           */
#define LIME_ERR_MAXLEN   (-4)  /* a cluster is longer than LIME_MAX_CLUSTER (ClusterBWT_DA.cpp:558-562) */
#define LIME_ERR_HALO     (-5)  /* shard: a run owned by this shard does not close inside its halo       */
#define LIME_ERR_DOCID    (-6)  /* a da value >= n_reads + n_refs was met while scoring.  Holds on every update path and
                                 * for every cluster size, on all 32 bits of the value; no kernel of such a pass writes
                                 * outside the buffers it was given (the table's contents are unspecified, but they are
                                 * contents of the table); calls that do more after the pass return the error and hand
                                 * out no lists, pairs or verdicts                                                    */
#define LIME_ERR_IO       (-7)  /* file I/O (CLI helpers)                                     */

#define LIME_MAX_CLUSTER  65536u /* Tools.h:33 sizeMaxBuf */
#define LIME_TILE         4096u  /* positions per workgroup tile; shard cuts must be multiples */
#define LIME_FASTA_BLOCK  4096u  /* input bytes one workgroup pass of the device FASTA and FASTQ parsers handles (lime_docs_from_*) */

typedef struct lime_ctx lime_ctx;

/* == ElementCluster, Tools.h:85-88; record of fileFasta.<alpha>.clrs */
typedef struct { uint64_t pStart, len; } lime_cluster_t;

/* a non-zero cell of a read's table row: the (idRef, sim) pair clusterChoose collects
 * (ClusterBWT_DA.cpp:390-402; the reference's pair_sim holds sim already divided by norm) */
typedef struct { uint32_t id_ref, sim; } lime_pair_t;

/* Counters of the last scan on a ctx (device-resident until lime_get_stats syncs). */
typedef struct {
    uint64_t n_clusters;   /* ClusterLCP.cpp:136 nClusters                                  */
    uint64_t max_len;      /* ClusterLCP.cpp:136 maxLen                                     */
    uint64_t n_updates;    /* table cells incremented (t > 0), ClusterBWT_DA.cpp:178-184    */
    uint32_t n_cross;      /* clusters that crossed a tile edge (scored by the list kernel)  */
    uint32_t n_big;        /* clusters longer than the in-tile limit (scored by the big kernel) */
    uint32_t flags;        /* LIME_FLAG_* */
    uint32_t wave_records_max; /* binned table updates: most update records one wave produced    */
    uint32_t edge;         /* LIME_EDGE_* of a shard (see lime_fused_dev)                        */
    uint32_t reserved;
} lime_stats_t;

#define LIME_FLAG_MAXLEN 1u
#define LIME_FLAG_HALO   2u
#define LIME_FLAG_DOCID  4u
#define LIME_FLAG_BADCLUSTER 8u
#define LIME_FLAG_OVERFLOW 16u   /* an internal cluster list was too small (cannot happen with the default sizing) */
#define LIME_FLAG_POOL_FULL 32u  /* binned table updates: the record pool was too small; lime_get_stats repeats the pass */
#define LIME_FLAG_CAS_FALLBACK 128u /* the pass wanted the binned update path and found no device memory for its records: it ran by compare-and-swap on the table instead (same result, several times slower); the reason is in lime_last_error().  Set by lime_get_stats; not an error */
#define LIME_FLAG_INTERNAL 64u   /* a device-side invariant did not hold (the scan's window hand-out): the pass is invalid, LIME_ERR_HIP */

/* Edge word of a shard (lime_stats_t.edge): what the host needs to decide about a run that crosses shard borders
 * and is longer than the read-ahead halo.  LEAD_*: the positions before the shard's first cluster head (they belong
 * to a run that started in an earlier shard) hold a read / a genome, and whether the shard has a head at all.
 * OPEN*: a run headed in the shard's owned range is still open at the end of its arrays (and already longer than
 * LIME_MAX_CLUSTER), with what it holds so far.  lime_combine_edges decides. */
#define LIME_EDGE_LEAD_HEAD 1u
#define LIME_EDGE_LEAD_R    2u
#define LIME_EDGE_LEAD_G    4u
#define LIME_EDGE_OPEN      8u
#define LIME_EDGE_OPEN_R   16u
#define LIME_EDGE_OPEN_G   32u

/* ---- lifecycle ------------------------------------------------------------------------ */
/* device < 0: keep the process's current HIP device.  Replaces the reference's
 * omp_set_num_threads set-up (ClusterLCP.cpp:73-84). */
int  lime_init(int device, lime_ctx **out);
void lime_shutdown(lime_ctx *ctx);
const char *lime_last_error(void);
void lime_free(void *p);                 /* frees host buffers returned by this library     */
const char *lime_version(void);
int  lime_device_count(void);            /* HIP devices visible to the process (0 if none) */
int  lime_pick_device(unsigned salt);    /* the device with the most free memory (ties by salt, e.g. the pid): for
                                          * LiME_paired.sh's four concurrent ClusterLCP processes (:44-53) */
/* Tuning and test knobs of a ctx, by name (value as text; "" = back to the library's own choice where that exists).  None changes a result;
 * most pick which kernel variant or update path runs.  Not a stable interface -- lime_amd/csrc/lime_api.cpp:set_option is the list:
 * update_path (cas|bin|auto), bin_levels ("one,two"), pool_density, pool_slack, scan_static_pct, second_level (tiles|sweeps), part_split, no_probe,
 * probe_min, force_p64, p64_test_base, max_blocks, choose_free, apply_wide, sort_nt, part_lines, no_staging, force_staging, detect_chunk,
 * score_chunk, force_rccl, io_threads, dense_min, no_direct, flush_gran (16|64), apply_group, debug_stats, debug_alloc, poison_cache.
 * The ENVIRONMENT is read by lime_init only: LIME_IO_THREADS (host staging threads; the reference's `threads` argument, ClusterLCP.cpp:73-84)
 * always, and -- only when LIME_TEST_HOOKS=1 is set -- a LIME_<KNOB> variable per knob above (tests, experiments).  bench.py refuses to run
 * under LIME_TEST_HOOKS. */
int  lime_set_option(lime_ctx *ctx, const char *key, const char *value);
/* Device blocks of 64 MB and more that the contexts of this process have released (lime_shutdown, scratch that was replaced by a larger block)
 * stay with the library for the next context instead of going back to the driver: on this platform a hipMalloc that is served from recycled
 * pages waits while the driver clears them (about 30 GB/s: seconds for a record pool).  At most a quarter of the device's
 * memory is held; a failed allocation releases it.  lime_trim_cache gives everything back now; returns the bytes released.  (Which pages are
 * "recycled" is not in this process's hands: pages that ANY process freed stay uncleared until the driver hands them out again -- see lime_reserve.) */
size_t lime_trim_cache(void);
/* Takes `bytes` of device memory (current device) from the driver NOW, in one block, for the large buffers of every context of this process: record
 * pools, binned records and the other blocks of 64 MB and more are carved from it (first fit, 2 MB granules) before anything is asked of the driver,
 * and go back to it when their context closes.  For a process that knows what it will need (a server; bench.py): where that hipMalloc meets
 * recycled pages it takes its 30 ms per GB here, once, at start-up, and no pass pays for an allocation again.  May be called again (another
 * block).  lime_trim_cache releases the reserved blocks nothing is carved from.  LIME_ERR_NOMEM if the driver refuses. */
int lime_reserve(size_t bytes);

/* ---- host-pointer API (pageable host arrays; the library stages them through HBM) ------ */

/* ClusterLCP main scan, src/ClusterLCP.cpp:140-283 (StartOrRemain :14-32, Close :34-43).
 * *clusters: library-owned host buffer (lime_free), ascending pStart = the reference's
 * 1-thread order; *max_len / *n_clusters as written to the aux .out file (:304-308). */
int lime_detect(lime_ctx *ctx, const uint32_t *lcp, const uint32_t *da, uint64_t n,
                uint32_t n_reads, uint32_t alpha,
                lime_cluster_t **clusters, uint64_t *n_clusters, uint64_t *max_len);

/* lime_detect with the records appended to the file `path` (fileFasta.<alpha>.clrs, ClusterLCP.cpp:229-235) as the chunks complete --
 * no list of the whole collection in host memory.  What the drop-in ClusterLCP calls. */
int lime_detect_to_file(lime_ctx *ctx, const uint32_t *lcp, const uint32_t *da, uint64_t n,
                        uint32_t n_reads, uint32_t alpha, const char *path, uint64_t *n_clusters, uint64_t *max_len);

/* The host-pointer entry points take arrays in pageable memory and stage them through pinned buffers on a few host threads.  When an array IS a
 * mapped file (the drop-in programs map fileFasta.lcp / .da / .ebwt / .clrs), registering the mapping lets those threads fill the pinned buffers with
 * pread() from `fd` instead of touching the mapping page by page (ClusterLCP.cpp:100-123 reads with one FILE* per thread).  The library keeps its
 * own duplicate of the descriptor until lime_unregister_file(base).
 * Contract: `base` maps the file from offset 0 (byte k of the mapping = byte k of the file), `bytes` is at most the file's size, the caller does
 * not write through the mapping (MAP_PRIVATE copies would be ignored: the FILE is read), registrations do not overlap, and the range is
 * unregistered BEFORE it is unmapped -- a stale registration would make a later array at the same address read the old file.  A registration
 * that breaks the checkable parts of this (size, overlap) is refused with LIME_ERR_ARG. */
int  lime_register_file(const void *base, size_t bytes, int fd);
void lime_unregister_file(const void *base);

/* clusterAnalyze, src/ClusterBWT_DA.cpp:256-358 (Update_ref_symb :81-105,
 * Analysis_and_updating :107-190 / :192-252).  ebwt == NULL selects the EBWT=0 build.
 * sim: caller-owned n_reads*n_refs bytes; it is OVERWRITTEN with the table for these
 * clusters (the reference starts from zero, :606-611).  Clusters may come in any order. */
int lime_score(lime_ctx *ctx, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
               const lime_cluster_t *clusters, uint64_t n_clusters,
               uint32_t n_reads, uint32_t n_refs, uint8_t *sim);

/* ClusterLCP + clusterAnalyze in one pass over the arrays (no .clrs materialised): the
 * benchmark path, 9 B/symbol (EBWT=1) or 8 B/symbol (ebwt == NULL). */
int lime_fused(lime_ctx *ctx, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt,
               uint64_t n, uint32_t n_reads, uint32_t n_refs, uint32_t alpha,
               uint8_t *sim, uint64_t *n_clusters, uint64_t *max_len);

/* lime_fused for collections of any size: the arrays stream from host memory (pageable or pinned)
 * through HBM in position-range chunks of `chunk` symbols (0 = 64 Mi; rounded up to LIME_TILE), each
 * with a read-ahead halo of LIME_MAX_CLUSTER + LIME_TILE positions, the copy of one chunk overlapping
 * the scan of the previous one; the table stays in HBM until the end.  Same results as lime_fused. */
int lime_fused_stream(lime_ctx *ctx, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt,
                      uint64_t n, uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint64_t chunk,
                      uint8_t *sim, uint64_t *n_clusters, uint64_t *max_len);

/* clusterChoose row scan, src/ClusterBWT_DA.cpp:385-402: per read the maximum cell and the
 * number of non-zero cells.  Normalisation/formatting stays on the host (:404-441). */
int lime_choose(lime_ctx *ctx, const uint8_t *sim, uint32_t n_reads, uint32_t n_refs,
                uint8_t *row_max, uint32_t *row_nnz);

/* clusterAnalyze + clusterChoose in one call (what the ClusterBWT_DA program does between reading
 * its inputs and writing .res.*, ClusterBWT_DA.cpp:605-443): like lime_score, but the table never
 * leaves the device; outputs as lime_choose_pairs_dev.  sim may be NULL (else it receives the table). */
int lime_score_choose(lime_ctx *ctx, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                      const lime_cluster_t *clusters, uint64_t n_clusters,
                      uint32_t n_reads, uint32_t n_refs, uint32_t norm, float beta,
                      uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs, uint64_t *n_pairs,
                      uint8_t *sim);

/* ---- device-pointer API (arrays already resident in HBM; asynchronous on `stream`) ----- *
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  Device arrays must be
 * 16-byte aligned (hipMalloc is) and d_sim must be allocated with lime_sim_bytes() bytes.   */

size_t lime_sim_bytes(uint32_t n_reads, uint32_t n_refs);  /* n_reads*n_refs rounded up to 16 */

/* One shard of a position-range partition (single GPU: n_own = n_avail = n, eof = 1).
 * The arrays hold positions [0, n_avail) of the shard: the first n_own are owned, the rest
 * is the read-ahead halo (the reference's straddle loop, ClusterLCP.cpp:246-264).  A cluster
 * belongs to the shard that owns its first position.  eof != 0: the arrays end at the true
 * end of the collection, so an open run closes at n_avail (ClusterLCP.cpp:244-245).
 * zero_sim != 0: clear d_sim first.  Counters: lime_get_stats.
 * Asynchronous on `stream`, except the FIRST pass on a ctx over 2^28 symbols or more (option probe_min, floor 2^24): it is preceded by a
 * sampled density probe (1/64 .. 1/256 of the windows, counted only) that synchronises the stream once -- the update path and the record pool
 * are chosen from what it finds, so that the one pass LiME_paired.sh:62-68 runs lands right.  A first pass of fewer symbols runs without the
 * probe, on the binned update path where the table allows it, with a record pool for 0.45 update records per owned symbol: 2 x 4 bytes x
 * 0.45 x 1.25 x 1.35 = about 6 bytes of extra HBM per symbol until a pass has measured the density.
 * Device memory taken on a pass's first call (scratch, record pool) is allocated synchronously: see lime_trim_cache for what that can cost. */
int lime_fused_dev(lime_ctx *ctx, const uint32_t *d_lcp, const uint32_t *d_da,
                   const uint8_t *d_ebwt, uint64_t n_own, uint64_t n_avail, int eof,
                   uint32_t n_reads, uint32_t n_refs, uint32_t alpha,
                   uint8_t *d_sim, int zero_sim, void *stream);

/* ---- owner-partitioned exchange of table updates (several GPUs, large tables) ----
 * lime_fused_records_dev: the same pass as lime_fused_dev, but no table is built: the shard's table updates are left as
 * 32-bit records grouped by table bin (bin b = table bytes [b << bin_shift, (b+1) << bin_shift); record = offset inside
 * the bin | t << bin_shift), the updates of clusters longer than the in-window limit as 64-bit records (cell | t << 40).
 * The layout is a pure function of the table's shape: every rank gets the same (lime_records_layout).  After
 * lime_get_stats (which also repeats a pass whose record pool proved too small), lime_records_get returns the device
 * arrays (valid until the next pass on the ctx) and, optionally, the bin bases on the host.  The owner of bins
 * [b0, b0 + nb) gathers the slices d_recs[binbase[b0] .. binbase[b0 + nb]) of every rank into one buffer and calls
 * lime_apply_records_dev, which builds bytes [b0 << bin_shift, ...) of the table in d_block (every byte written; add
 * the long clusters' records of ALL ranks).  lime_comm_exchange_records does the transport with RCCL.
 * The t field of a 32-bit record: the contract is t == 1 (a score of t leaves the pass as t records), and a word whose t
 * field is 0 is "no record": it is skipped wherever it stands between h_srcoff's bounds, so a caller may pad with such
 * words.  What a 32-bit record with t >= 2 adds is unspecified (the kernels differ), and d_rx is not validated: that
 * would cost a read of every record.  The 64-bit records carry any t of 1 .. 255 (added modulo 256).
 * lime_apply_records_dev refuses with LIME_ERR_ARG, before anything is launched: n_src == 0, nb > 3072, bin_shift
 * outside 16 .. 25, block_bytes not a multiple of 16 or beyond nb << bin_shift, d_block not 16-byte aligned, cell_lo not
 * a multiple of 1 << bin_shift, and source offsets that descend.
 * Reference counterpart: the cluster-range split over threads adding into one table, ClusterBWT_DA.cpp:630-670. */
typedef struct {
    uint32_t n_bins, bin_shift;
    const uint32_t *d_recs;            /* device: records grouped by bin */
    const uint64_t *d_binbase;         /* device: n_bins + 1 positions in d_recs */
    const uint64_t *d_bigrecs;         /* device: updates of the long clusters, cell | t << 40 */
    uint64_t n_bigrecs;
} lime_records_t;
int lime_records_layout(lime_ctx *ctx, uint32_t n_reads, uint32_t n_refs, uint32_t *n_bins, uint32_t *bin_shift);
int lime_fused_records_dev(lime_ctx *ctx, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt,
                           uint64_t n_own, uint64_t n_avail, int eof, uint32_t n_reads, uint32_t n_refs,
                           uint32_t alpha, void *stream);
int lime_records_get(lime_ctx *ctx, lime_records_t *out, uint64_t *h_binbase /* n_bins + 1, may be NULL */, void *stream);
int lime_apply_records_dev(lime_ctx *ctx, uint32_t n_src, const uint32_t *d_rx, const uint64_t *h_srcoff /* [n_src][nb + 1] */,
                           uint32_t nb, uint32_t bin_shift, const uint64_t *d_bigrecs, uint64_t n_bigrecs,
                           uint64_t cell_lo, uint64_t block_bytes, uint8_t *d_block, void *stream);

/* Test and diagnosis hook, like lime_apply_records_dev for the stage behind it: the FIRST-LEVEL PARTITION of the binned update path alone
 * (k_bin_rowscan, k_bin_bases, then k_part or k_part_lines -- whichever a pass with this layout would get) on a record pool the caller made.
 * h_pool: n_prod * prod_waves * n_sub * cap_w host words laid out as the scan lays them: the segment of (wave w, sub-region s) starts at
 * (w * n_sub + s) * cap_w and holds h_wave_cnt[w * n_sub + s] records; producer p owns the waves p * prod_waves .. + prod_waves - 1.  A pool
 * record is the cell's low 32 bits, its bin (rec >> bin_shift) + (s << (32 - bin_shift)) (lime_rec_bin).  What a segment holds beyond its
 * count is never used as a record.
 * d_out (device, out_words words): the records grouped by bin, each as (rec & ((1 << bin_shift) - 1)) | 1 << bin_shift; bin b's start
 * goes to h_binbase[b] (n_bins + 1 words: h_binbase[b] = the lower bins' records, h_binbase[n_bins] = all records), and producer p's
 * records of bin b lie at h_binbase[b] + (the records of b of the producers below p) ..; the order INSIDE one (bin, producer) range is
 * unspecified.  Words of d_out from h_binbase[n_bins] on are not written.  *kernel: 1 if k_part_lines ran, 0 if k_part.
 * Honours the ctx options part_lines, force_p64 and p64_test_base (the positions then start at that number; h_binbase is reported without it).
 * Refused with LIME_ERR_ARG before anything is launched: a NULL pointer, n_prod == 0, prod_waves outside 1 .. 16, n_sub outside 1 .. 8,
 * cap_w not a multiple of 16 (or prod_waves * n_sub * cap_w beyond 2^32 - 16), a count above cap_w, bin_shift outside 16 .. 25, n_bins
 * outside 1 .. 3072, a record whose bin is n_bins or more, more records than out_words, d_out not 64-byte aligned.
 * Uploads the pool into the ctx's own scratch, waits for `stream`, and leaves nothing for lime_get_stats to repeat. */
int lime_partition_records_dev(lime_ctx *ctx, uint32_t n_prod, uint32_t prod_waves, uint32_t n_sub, uint32_t cap_w, const uint32_t *h_pool,
                               const uint32_t *h_wave_cnt, uint32_t n_bins, uint32_t bin_shift, uint32_t *d_out, uint64_t out_words,
                               uint64_t *h_binbase /* n_bins + 1, out */, int *kernel /* out */, void *stream);

/* Runs longer than the halo that cross shard borders: the reference reads on without limit (ClusterLCP.cpp:246-264)
 * and only refuses CLUSTERS longer than LIME_MAX_CLUSTER (ClusterBWT_DA.cpp:558-562).  A shard that ends inside such a
 * run reports it in lime_stats_t.edge (and lime_get_stats returns LIME_ERR_HALO to callers that do not look);
 * edge[k] = the edge word of shard k, shards in position order, the first one starting at position 0 and the last one
 * run with eof != 0.  Returns LIME_OK if no border-crossing run is a read+genome cluster (nothing to score: the
 * shards' tables are complete), LIME_ERR_MAXLEN if one is (the reference fails on such input too). */
int lime_combine_edges(const uint32_t *edge, uint32_t n_shards);

/* Detection only.  *d_clusters: library-owned DEVICE buffer valid until the next
 * lime_detect_dev/lime_shutdown on this ctx; pStart = pos_base + local position.
 * Synchronises `stream` (the record count sizes the output). */
int lime_detect_dev(lime_ctx *ctx, const uint32_t *d_lcp, const uint32_t *d_da,
                    uint64_t n_own, uint64_t n_avail, int eof, uint64_t pos_base,
                    uint32_t n_reads, uint32_t alpha,
                    const lime_cluster_t **d_clusters, uint64_t *n_clusters, uint64_t *max_len,
                    void *stream);

/* Scoring of a device-resident cluster list (pStart local to d_da/d_ebwt). */
int lime_score_dev(lime_ctx *ctx, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                   const lime_cluster_t *d_clusters, uint64_t n_clusters,
                   uint32_t n_reads, uint32_t n_refs, uint8_t *d_sim, int zero_sim, void *stream);

int lime_choose_dev(lime_ctx *ctx, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs,
                    uint8_t *d_row_max, uint32_t *d_row_nnz, void *stream);

/* clusterChoose with the table left in HBM (ClusterBWT_DA.cpp:385-423): the row scan AND the
 * (idRef, sim) lists of the reads that pass `float(max)/norm > beta` (:404-406) are made on the
 * device; only row_max (n_reads bytes) and the compact lists come back.  HOST outputs:
 * row_max[n_reads], row_off[n_reads+1] (cells of read r = pairs[row_off[r] .. row_off[r+1]),
 * ascending idRef; empty for a read that does not pass), *pairs library-allocated (lime_free). */
int lime_choose_pairs_dev(lime_ctx *ctx, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs,
                          uint32_t norm, float beta, uint8_t *row_max, uint64_t *row_off,
                          lime_pair_t **pairs, uint64_t *n_pairs, void *stream);

/* ClusterLCP scan + clusterAnalyze + clusterChoose (ClusterLCP.cpp:140-283, ClusterBWT_DA.cpp:256-358, :385-423) on device-resident arrays of the
 * whole collection, outputs as lime_choose_pairs_dev.  Where the binned update path serves the pass (tables beyond 64 MB, n_refs >= 256) the
 * table is never written or read: its 64 KB regions are built in LDS and give the rows' maxima / non-zero counts, then the passing rows' lists.
 * Elsewhere the table is built and scanned.  *stats (may be NULL) as lime_get_stats.  Synchronises `stream`. */
int lime_fused_choose_dev(lime_ctx *ctx, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                          uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta,
                          uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs, uint64_t *n_pairs,
                          lime_stats_t *stats, void *stream);

/* Synthetic inputs of SURVEY.md section 8(d): element i is a pure function of (seed, i0+i).
 * Any of the three outputs may be NULL.  mode 0 = iid, 1 = block-correlated symbols. */
int lime_synth_dev(lime_ctx *ctx, uint64_t seed, uint64_t i0, uint64_t count,
                   uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t mode,
                   uint32_t *d_lcp, uint32_t *d_da, uint8_t *d_ebwt, void *stream);

/* Waits for `stream`, returns the counters of the last *_dev scan, and maps flags to an
 * error code (LIME_ERR_MAXLEN / _HALO / _DOCID) -- stats are filled either way.  The results of a
 * lime_fused_dev pass are final only once this has returned: a pass on the binned update path whose record
 * pool proved too small is repeated here with a larger one (the caller's arrays must still be in place). */
int lime_get_stats(lime_ctx *ctx, lime_stats_t *out, void *stream);

/* Average device time (ms) of the main scan kernel over the launches since the last call,
 * measured with HIP events on the launch stream; enabled by lime_set_timing(ctx, 1). */
int lime_set_timing(lime_ctx *ctx, int on);
int lime_get_timing(lime_ctx *ctx, double *scan_ms_avg, uint64_t *launches);
/* the same with the parts of a lime_fused_dev pass: ms_avg[0] the scan kernel, [1] the whole pass (table clear or
 * table build included), [2] everything after the scan kernel, [3] everything before it */
int lime_get_timing_ex(lime_ctx *ctx, double ms_avg[4], uint64_t *launches);
/* What the passes on this ctx have cost on the host side so far (LiME_paired.sh:62-68 runs every collection once: a cold pass pays all of it):
 * out[0] ms inside device allocations, [1] ms inside the sampled density probe in front of the ctx's first pass (synchronisation included),
 * [2] probes run, [3] passes repeated by lime_get_stats (record pool too small), [4] passes that fell back to compare-and-swap
 * (LIME_FLAG_CAS_FALLBACK), [5] update records per owned symbol as last measured (-1: nothing measured yet), [6] lime_fused_choose_dev calls
 * served without the table, [7] reserved. */
int lime_get_host_times(lime_ctx *ctx, double out[8]);

/* ---- multi-GPU: the one exchange step of the path (RCCL over xGMI; librccl is loaded on first use) ---- *
 * The reference partitions positions over OpenMP threads (ClusterLCP.cpp:150-161, skip :196-202, straddle
 * :246-264) and adds into ONE shared table with `omp atomic` (ClusterBWT_DA.cpp:178-184, 243-248).  Here every
 * GPU scans one position range (lime_fused_dev with n_own / n_avail / eof) into its own table and the tables are
 * summed modulo 256 -- addition modulo 256 is associative, so the result is bit-identical.
 * One process per GPU: rank 0 calls lime_comm_unique_id, carries the bytes to the others, all call lime_comm_init
 * (the process's current HIP device is the rank's GPU).  Error text: lime_comm_error(). */
#define LIME_COMM_ID_BYTES 128
typedef struct lime_comm lime_comm;
int  lime_comm_unique_id(uint8_t id[LIME_COMM_ID_BYTES]);
int  lime_comm_init(const uint8_t id[LIME_COMM_ID_BYTES], int rank, int world, lime_comm **out);
void lime_comm_destroy(lime_comm *comm);
int  lime_comm_count(lime_comm *comm, int *ranks);   /* ncclCommCount: the ranks RCCL counts in the communicator */
const char *lime_comm_error(void);
/* d_sim: world * block_bytes bytes (the table, zero padded); rank r receives block r of the sum in d_block
 * (ncclReduceScatter, ncclUint8, ncclSum).  Asynchronous on `stream`. */
int  lime_comm_reduce_scatter_tables(lime_comm *comm, const uint8_t *d_sim, uint8_t *d_block, size_t block_bytes, void *stream);
int  lime_comm_allreduce_tables(lime_comm *comm, uint8_t *d_sim, size_t bytes, void *stream);   /* whole table everywhere, in place */
/* d_sum_max: device array of two u64: [0] summed over the ranks (cluster count), [1] maximum (longest cluster) */
int  lime_comm_combine_counters(lime_comm *comm, uint64_t *d_sum_max, void *stream);
/* Owner-partitioned exchange of the update records lime_fused_records_dev left on `ctx` (call lime_get_stats first): rank r
 * ends with bytes [*cell_lo, *cell_lo + *block_bytes) of the finished table in d_block -- the bins r * per .. (r+1) * per,
 * per = ceil(n_bins / world), see lime_records_layout; block_cap >= per << bin_shift.  Collective: every rank calls it. */
int  lime_comm_exchange_records(lime_comm *comm, lime_ctx *ctx, uint32_t n_reads, uint32_t n_refs, uint8_t *d_block,
                                size_t block_cap, uint64_t *cell_lo, uint64_t *block_bytes, void *stream);

/* One process, n_dev GPUs (devices == NULL: 0 .. n_dev-1): lime_fused of host arrays with the collection cut into
 * n_dev position ranges, one reduce-scatter of the tables by read-row blocks, the blocks copied back into `sim`.
 * What the drop-in ClusterBWT_DA-side programs use under LIME_GPUS=k. */
int  lime_fused_multi(int n_dev, const int *devices, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt,
                      uint64_t n, uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint8_t *sim,
                      uint64_t *n_clusters, uint64_t *max_len);

/* lime_score_choose on n_dev GPUs of one process (what the drop-in ClusterBWT_DA does under LIME_GPUS=k): the cluster
 * list is cut by position into n_dev parts, every device scores its part into its own table, one RCCL reduce-scatter
 * by read-row blocks, row scan and list compaction per block.  Outputs as lime_score_choose. */
int  lime_score_choose_multi(int n_dev, const int *devices, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                             const lime_cluster_t *clusters, uint64_t n_clusters, uint32_t n_reads, uint32_t n_refs,
                             uint32_t norm, float beta, uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs,
                             uint64_t *n_pairs);

/* ---- pure host helpers (no device work; used by the CLIs and by CPU-side tests) -------- */
uint8_t lime_sym_index(uint8_t byte);                              /* ClusterBWT_DA.cpp:455-470 */
uint8_t lime_pair_score(const uint8_t cr[16], const uint8_t cg[16]); /* :129-177, host build of the device routine */

/* The update records of the binned path, as the scan writes them and the partition kernels bin them (one definition,
 * lime_device.h).  cell = read * n_refs + genome index; record = the cell's low 32 bits, sub-region = its high part,
 * bin = cell >> bin_shift.  lime_rec_layout: the layout a table of that shape gets (one_level = two_level = 0: the
 * defaults, else as LIME_BIN_LEVELS).  lime_rec_valid: the test every genome index (da - n_reads) passes, on all 32 bits,
 * before anything is stored for it.  lime_rec_batch: what the scan stores for each of n pairs -- nothing for an index that
 * fails the test, or (fixed_slot: a slot handed out before the test, one sub-region) a stand-in record inside the table --
 * and the bin the partition kernels compute for it. */
typedef struct { uint32_t n_bins, bin_shift, n_sub, sub_rb, sub_gb; } lime_rec_layout_t;
int      lime_rec_layout(uint32_t n_reads, uint32_t n_refs, uint32_t one_level, uint32_t two_level, lime_rec_layout_t *out);
int      lime_rec_valid(uint32_t gd, uint32_t n_refs);
uint32_t lime_rec_of(uint32_t rd, uint32_t gd, uint32_t n_refs);
uint32_t lime_rec_sub2(uint32_t rd, uint32_t gd, uint32_t sub_rb, uint32_t sub_gb);
uint32_t lime_rec_bin(uint32_t rec, uint32_t sub, uint32_t bin_shift);
int      lime_rec_batch(const uint32_t *rd, const uint32_t *gd, uint64_t n, uint32_t n_refs, const lime_rec_layout_t *layout,
                        int fixed_slot, uint8_t *valid, uint8_t *stored, uint32_t *rec, uint32_t *sub, uint32_t *bin);
/* The record buffers of a scan wave whose scorers write the records (tables of one or two sub-regions): records each holds in the
 * EBWT=0 / EBWT=1 kernel, the most a flush that makes room leaves waiting (whole lines of 16 leave), and the most the flush at a
 * window's top leaves where it takes batches of 64 (option flush_gran). */
typedef struct { uint32_t cap, cap_short, room_left, top_left; } lime_scan_queue_t;
void     lime_scan_queue(lime_scan_queue_t *out);

/* Writers of the reference's files (byte-identical formats). */
int lime_write_clrs(const char *path, const lime_cluster_t *clusters, uint64_t n_clusters); /* ClusterLCP.cpp:229-235 */
int lime_write_aux(const char *path, uint32_t n_reads, uint32_t n_refs, uint32_t alpha,
                   uint64_t max_len, uint64_t n_clusters);                                  /* ClusterLCP.cpp:294-310 */
int lime_read_aux(const char *path, uint32_t *n_reads, uint32_t *n_refs, uint32_t *alpha,
                  uint64_t *max_len, uint64_t *n_clusters);                                 /* ClusterBWT_DA.cpp:531-551 */
/* clusterChoose output, ClusterBWT_DA.cpp:361-450.  row_max may be NULL (then recomputed). */
int lime_write_res_txt(const char *path, const uint8_t *sim, const uint8_t *row_max,
                       uint32_t n_reads, uint32_t n_refs, uint32_t norm, float beta);
int lime_write_res_bin(const char *path_bin, const char *path_pos, const uint8_t *sim,
                       const uint8_t *row_max, uint32_t n_reads, uint32_t n_refs,
                       uint32_t norm, float beta);
/* the same files from the compact form of lime_choose_pairs_dev / lime_score_choose */
int lime_write_res_txt_pairs(const char *path, const uint8_t *row_max, const uint64_t *row_off,
                             const lime_pair_t *pairs, uint32_t n_reads, uint32_t norm, float beta);
int lime_write_res_bin_pairs(const char *path_bin, const char *path_pos, const uint8_t *row_max,
                             const uint64_t *row_off, const lime_pair_t *pairs, uint32_t n_reads,
                             uint32_t norm, float beta);

/* ---- read assignment from the .res files (the consumer of the path, src/Classify.cpp) ---- *
 * inputs: n_files (2 single-end, 4 paired-end) .res base names, in the reference's argv order
 * (Classify.cpp:352-360); binary != 0 reads base.bin + base.pos (BIN=1, the Makefile default), else
 * base.txt; rank 0..6 as the reference's taxRank; higher != 0 = the HIGHER=1 build.  Writes the
 * reference's classification file; counts = {classified, not classified, ambiguous, higher rank}.
 * Pure host code.  Error text: lime_classify_error(). */
int lime_classify(uint32_t n_files, const char *const *inputs, int binary, uint32_t n_reads,
                  uint32_t n_targ, const char *path_out, const char *path_tax, int rank, int higher,
                  uint64_t counts[4]);
const char *lime_classify_error(void);

/* ---- read assignment from lists resident in HBM ------------------------------------------ *
 * One read's decision: type 'C' / 'U' / 'A' / 'H' (classified, not classified, ambiguous, higher rank), the taxon ('C', 'H'),
 * the similarity written next to it, and the rule that decided (0 = U; 1, 2, 3 as in lime_classify.cpp). 12 bytes. */
typedef struct { uint32_t taxon; float sim; uint8_t type; uint8_t rule; uint8_t pad[2]; } lime_verdict_t;

/* One collection's clusterChoose result left in HBM (ctx-owned, opaque): row_max u8[n_reads], row_off u64[n_reads + 1], the pairs
 * (ascending idRef inside each row) and the norm / beta it was made with -- what lime_choose_pairs_dev / lime_fused_choose_dev return
 * on the host, which are now "make the lists, copy them out".  Any number may live at once (four for a paired-end sample); each is
 * released by lime_lists_free, or by lime_shutdown of its ctx (not both).  These calls synchronise `stream`. */
typedef struct lime_lists lime_lists;
int lime_choose_lists_dev(lime_ctx *ctx, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs, uint32_t norm, float beta,
                          lime_lists **out, void *stream);
int lime_fused_choose_lists_dev(lime_ctx *ctx, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                                uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta, lime_lists **out,
                                lime_stats_t *stats, void *stream);
/* the same from host arrays or mapped files (registered with lime_register_file: read with pread()), staged through pinned memory */
int lime_fused_choose_lists(lime_ctx *ctx, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                            uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta, lime_lists **out,
                            lime_stats_t *stats);
/* host copies: row_max[n_reads], row_off[n_reads + 1] (caller's), *pairs library-allocated (lime_free; NULL when there are none) */
int lime_lists_get(const lime_lists *lists, uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs, uint64_t *n_pairs);
int lime_lists_info(const lime_lists *lists, uint32_t *n_reads, uint64_t *n_pairs, uint32_t *norm, float *beta);
void lime_lists_free(lime_lists *lists);
/* The lists of column shards of one table made into the whole table's list.  A table column depends on its genome and the reads and on no
 * other genome, so P >= 1 parts -- lists over the same n_reads and norm, part p holding genomes id_base[p] ..
 * id_base[p] + n_refs_part[p] - 1 of the whole table, each made with a beta every non-zero row passes (a negative one) -- hold all its
 * non-zero cells.  What does not split is clusterChoose's test, `float(max) / norm > beta` with max over the WHOLE row: it is applied here,
 * once, on the maximum over the parts, and a passing row lists all its parts' pairs (id_ref + id_base[p], sim unchanged; ascending idRef
 * is kept).  *out is an ordinary lime_lists with the parts' norm and this beta; the parts stay the caller's.  A negative beta keeps every
 * non-zero row, so acc = concat(acc, part) step by step, then one call with the single part acc and the real beta, equals the one-step
 * call.  On the device: one pass over the rows, one 64-bit prefix sum, 8 bytes to the host (the total sizes the pairs' block), one pass
 * that copies the pairs; no row comes to the host.  Device memory next to *out: 32 bytes per part + 8 per read + the prefix sum's,
 * given back before the call returns.
 * LIME_ERR_ARG, with text in lime_last_error() and before any launch: n_parts = 0, a NULL part or one of another context, parts of
 * different n_reads or norm, id_base[p] < id_base[p - 1] + n_refs_part[p - 1] (not ascending, or id ranges that overlap), id_base[p] +
 * n_refs_part[p] > 2^32 - 1.  On any error nothing stays allocated.  Synchronises `stream`. */
int lime_lists_concat_dev(lime_ctx *ctx, uint32_t n_parts, const lime_lists *const *parts, const uint32_t *id_base,
                          const uint32_t *n_refs_part, float beta, lime_lists **out, void *stream);
/* the last lime_lists_concat_dev of the ctx: with lime_set_timing on, HIP-event ms of out[0] the pass over the rows (k_lc_rows), out[1] the
 * prefix sum, out[2] the pass that copies the pairs (k_lc_copy); out[3] the pairs it wrote */
int lime_get_concat_info(lime_ctx *ctx, double out[4]);
/* The same with clusterChoose's test taken PER READ: read r passes where `float(max) / d_norms[r] > beta` (the reference's expression in the
 * reference's types, from a 256 x 256 table the host builds for the norms 1 .. 255; a norm of 0 passes nothing; nothing is divided on the
 * device).  d_norms: u8[n_reads] in device memory, e.g. lime_docs_norms_dev's.  The parts are as above -- made with a negative beta, their
 * own norm plays no part but is equal among them; parts that hold per-read norms themselves are taken too, and theirs are ignored -- and
 * one part with id_base 0 is the plain per-read filter of a list.  Same passes as above (k_rn_rows in place of k_lc_rows; the prefix sum and
 * k_lc_copy unchanged), same argument checks and texts, same lime_get_concat_info; d_norms == NULL with n_reads > 0: LIME_ERR_ARG.  A negative
 * beta keeps every non-zero row, as above.  *out owns a copy of the norms: lime_lists_info reports norm 0 for it, lime_lists_get_norms copies
 * them out (LIME_ERR_ARG for a list made with one norm), lime_classify_lists_dev takes it, alone or next to lists with one norm, and
 * lime_lists_concat_dev refuses it as a part (LIME_ERR_ARG). */
int lime_lists_concat_norms_dev(lime_ctx *ctx, uint32_t n_parts, const lime_lists *const *parts, const uint32_t *id_base,
                                const uint32_t *n_refs_part, const uint8_t *d_norms, float beta, lime_lists **out, void *stream);
int lime_lists_get_norms(const lime_lists *lists, uint8_t *norms);   /* host copy into the caller's n_reads bytes */

/* The lineage file (';'-separated, a header line; Classify.cpp:32-85) at taxRank `rank` (0 = genome .. 6), with the higher ranks'
 * columns when higher != 0 (the HIGHER=1 build; needs rank >= 1).  Host only; the device copy is made by the first device
 * classification that uses it.  A file with other than n_targ genomes: LIME_ERR_ARG ("poor taxonomy information").
 * Errors of lime_taxonomy_load, lime_classify_mem and lime_write_classification: lime_classify_error(). */
typedef struct lime_taxonomy lime_taxonomy;
int  lime_taxonomy_load(const char *path, int rank, int higher, uint32_t n_targ, lime_taxonomy **out);
void lime_taxonomy_free(lime_taxonomy *tx);

/* Classify (Classify.cpp:503-690, the decision of lime_classify) on the device over 2 (single-end) or 4 (paired-end, the
 * script's F, F_RC, R, R_RC order) lists of one ctx: one verdict per read into the host array verdicts[n_reads] (12 bytes per read
 * cross PCIe); counts = {C, U, A, H}.  binary != 0: the values the BIN=1 build reads (float(k) / norm), else the .res.txt ones (%.5f).
 * LIME_ERR_ARG (lime_last_error) for n_lists other than 2 / 4, lists with different n_reads, a taxonomy of another n_targ and an
 * idRef >= n_targ.  Synchronises `stream`.  One taxonomy may serve contexts on several threads and devices (its device copy is made
 * on first use, per device, under a lock; calls that use it on different devices take turns). */
/* Lists with a norm per read (lime_lists_concat_norms_dev) are taken alone or next to lists with one norm, which behave as if every read
 * had that norm: read r's values in list i are those of lime_cls value tables for norms_i[r], built by the host for the norms 1 .. 255 at the
 * list's beta (float[256][2][256], 512 KB of device memory per distinct beta for the call's duration) and read by a second instantiation
 * of the same decision, k_classify_norms.  A call without such a list runs k_classify, exactly as before. */
int lime_classify_lists_dev(lime_ctx *ctx, uint32_t n_lists, const lime_lists *const *lists, uint32_t n_targ,
                            const lime_taxonomy *tx, int binary, lime_verdict_t *verdicts, uint64_t counts[4], void *stream);
/* The same decision on the host over lists held in memory (lime_lists_get's copies): the CPU reference of the device path. */
int lime_classify_mem(uint32_t n_files, const uint8_t *const *row_max, const uint64_t *const *row_off, const lime_pair_t *const *pairs,
                      const uint32_t *norms, const float *betas, int binary, uint32_t n_reads, uint32_t n_targ,
                      const lime_taxonomy *tx, lime_verdict_t *verdicts, uint64_t counts[4]);
/* lime_classify_mem with a norm per read: read_norms[i] (u8[n_reads]) gives list i's norm for every read; an entry may be NULL, and then
 * norms[i] is used for all reads as in lime_classify_mem.  A read norm of 0 gives the read no record in that list.  The same decide(). */
int lime_classify_mem_norms(uint32_t n_files, const uint8_t *const *row_max, const uint64_t *const *row_off, const lime_pair_t *const *pairs,
                            const uint32_t *norms, const uint8_t *const *read_norms, const float *betas, int binary, uint32_t n_reads,
                            uint32_t n_targ, const lime_taxonomy *tx, lime_verdict_t *verdicts, uint64_t counts[4]);
/* The classification file of lime_classify (header, "C,read,taxon,sim" lines, same float formatting) from verdicts. */
int lime_write_classification(const char *path, const lime_verdict_t *verdicts, uint32_t n_reads);

/* ---- ebwt / lcp / da from the sequences: a generalized suffix sort on the device ---------- *
 * What the reference leaves to BCR_LCP_GSA / eGSA / eGap (Preprocessing.sh), in the convention the calls above consume and
 * lime_amd/builder.py defines: the documents are the reads (ids 0 .. n_reads - 1) followed by the genomes, each followed by its own
 * terminator; a terminator sorts below every symbol, two terminators by document id; symbols compare as unsigned bytes (all 256 values
 * are legal, empty documents too).  da[i] = document of suffix i, ebwt[i] = the byte in front of it (`term` for a document's whole
 * suffix), lcp[i] = leading non-terminator symbols suffixes i - 1 and i share (lcp[0] = 0), min(lcp[i], lcp_cap) when lcp_cap > 0
 * (eGap's --trlcp; the scan needs lcp_cap >= alpha), the full value when lcp_cap == 0.
 * text: the documents' symbols back to back WITHOUT terminators, reads first; doc_off[n_docs + 1] their starts (doc_off[0] = 0).
 * Outputs: N = doc_off[n_docs] + n_docs elements each (lime_index_size); any of the three may be NULL.
 * Limits: N <= 2^32 - 1, one GPU, the whole collection resident -- beyond them, and for a doc_off that does not start at 0, decreases
 * or (device call) does not end at n_text: LIME_ERR_ARG.  Device memory: 52 bytes of scratch per position (N) next to the text
 * (1 byte per symbol), doc_off (8 bytes per document) and the outputs (9 bytes per position), taken from lime_reserve's arena / the
 * block cache and given back before the call returns; LIME_ERR_NOMEM without it.
 * Cost: a radix sort of N 64-bit keys, then one sort per doubling round over the suffixes whose rank is not unique yet (repeats
 * longer than the 64-bit key's symbols: genome repeats; a run of L equal symbols takes log2 L rounds); the LCP step compares
 * sum(lcp) / 8 words of text in the worst case (near-identical genomes), at most N * lcp_cap / 8 with a cap.
 * Reads can be merged into a genome index that was built once: lime_gindex_build / lime_merge_index below.
 * Out of scope: several GPUs, collections larger than HBM. */
uint64_t lime_index_size(const uint64_t *doc_off, uint32_t n_docs);
/* host arrays, staged through HBM like the other host calls */
int lime_build_index(lime_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint8_t term, uint32_t lcp_cap,
                     uint8_t *ebwt, uint32_t *lcp, uint32_t *da);
/* device arrays; outputs that are 16-byte aligned go straight into lime_fused_dev / lime_fused_choose_lists_dev.  Synchronises `stream`. */
int lime_build_index_dev(lime_ctx *ctx, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                         uint8_t term, uint32_t lcp_cap, uint8_t *d_ebwt, uint32_t *d_lcp, uint32_t *d_da, void *stream);
/* the last build of the ctx: out[0] doubling rounds run, out[1 .. 4] suffixes still without a unique rank after the first sort and
 * after rounds 1, 2, 3; with lime_set_timing on, HIP-event ms of out[5] preparation + first sort, out[6] the doubling rounds,
 * out[7] da / ebwt / lcp */
int lime_get_index_info(lime_ctx *ctx, double out[8]);
/* FASTA: '>' lines are headers, every other line's bytes minus CR/LF are appended as they are (no case folding; lines in front of the
 * first header are skipped); rc != 0 reverse-complements each record (A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H, S, W, N and
 * every other byte unchanged, case kept).  *text (at least one byte) and *doc_off[*n_docs + 1] are library-owned (lime_free).
 * Pure host code.  LIME_ERR_IO when the file cannot be read. */
int lime_fasta_read(const char *path, int rc, uint8_t **text, uint64_t **doc_off, uint32_t *n_docs);
/* FASTQ, the four-line form (wrapped sequences are refused, not guessed at): line 4k is the '@' header, 4k + 1 the sequence, 4k + 2 the
 * '+' separator, 4k + 3 the quality string.  Records are found by counting lines, never by looking for '@' (a quality string may begin with
 * '@' or '+').  A line ends at its LF or at the end of the file; bytes after the last LF are a line, nothing after it is none.  The sequence
 * line's bytes minus CR are the record's symbols as they are (an empty read is a record); the header, the separator's text and the
 * quality values are not kept.  An empty file: no record, doc_off = {0}.  rc, ownership and LIME_ERR_IO as lime_fasta_read.
 * LIME_ERR_ARG, with lime_last_error() = "<who>: line <L>: <reason>", L counted from 1, for the lowest offending line, and of two reasons
 * on one line the first of:
 *   "record does not start with '@'"               the first byte of a line 4k is not '@' (an empty line included)
 *   "separator line does not start with '+'"       the first byte of a line 4k + 2 is not '+'
 *   "quality length differs from sequence length"  line 4k + 3 has another number of bytes that are neither CR nor LF than line 4k + 1
 *   "truncated record"                             the number of lines is no multiple of 4; L is the last line
 * Pure host code, a plain line reader: the oracle of the device parser below. */
int lime_fastq_read(const char *path, int rc, uint8_t **text, uint64_t **doc_off, uint32_t *n_docs);
/* lime_fastq_read(path, 0) and the quality strings: *qual holds, laid out by the same *doc_off as *text, the bytes of every line 4k + 3
 * that are neither CR nor LF, as they are (no offset is taken off).  The same refusals, codes and texts (they start with this call's name).
 * *qual is library-owned too (lime_free).  Pure host code: the oracle of lime_docs_from_fastq_qual*. */
int lime_fastq_read_qual(const char *path, uint8_t **text, uint8_t **qual, uint64_t **doc_off, uint32_t *n_docs);
/* Quality trimming, the BWA / cutadapt rule.  For a read with quality bytes b[0 .. L) let q[i] = b[i] - 33 as a signed integer (Phred+33,
 * the only offset; a byte below 33 is a negative quality).  Two cutoffs, q5 for the 5' end and q3 for the 3' end, each 0 .. 93; a cutoff
 * of 0 leaves that end alone whatever the bytes.
 *   3' end  S(i) = sum over j in [i, L) of (q[j] - q3).  B = the largest i with S(i) > 0, or -1.  m = min S(j) over B < j < L.  If
 *           B + 1 < L and m < 0, hi = the LARGEST j in that range with S(j) = m; otherwise hi = L.  As a loop: walk from the end, add
 *           q[i] - q3, stop at the first sum above 0, keep the index of the strictly lowest sum seen.
 *   5' end  P(i) = sum over j in [0, i] of (q5 - q[j]).  E = the smallest i with P(i) < 0, or L.  M = max P(j) over 0 <= j < E.  If E > 0
 *           and M > 0, lo = 1 + the SMALLEST such j with P(j) = M; otherwise lo = 0.
 *   Both ends are computed on the whole read, independently.  lo >= hi: the read becomes empty; otherwise it becomes text[lo .. hi).
 * The sums are exact for every read (64 bits).  Read indices never change: as many documents come out as went in, an emptied read is an
 * empty document, and no read is dropped for its length.
 * lime_trim_info_t: n_reads; n_changed, the reads that lost a symbol; n_empty, the reads that held symbols and keep none; the symbols
 * before and after.
 * lime_quality_trim is the loop form in plain host code, the oracle of lime_docs_trim_dev: text / qual / doc_off[n_docs + 1] as
 * lime_fastq_read_qual gives them; *out_text (at least one byte) and *out_doc_off[n_docs + 1] are library-owned (lime_free); info may
 * be NULL.  LIME_ERR_ARG with a text: a NULL array, a cutoff above 93, doc_off that does not start at 0 or decreases. */
typedef struct { uint64_t n_reads, n_changed, n_empty, symbols_in, symbols_out; } lime_trim_info_t;
int lime_quality_trim(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t q5, uint32_t q3,
                      uint8_t **out_text, uint64_t **out_doc_off, lime_trim_info_t *info);
/* Adapter trimming: a 3' adapter with mismatches only and no indels, the leftmost match (cutadapt's `-a ADAPTER --no-indels`; the simple
 * mode of fastp and Trimmomatic).  Integers only.  The read is s[0 .. L), the adapter a[0 .. M) with 1 <= M <= 64, every byte of it one
 * of ACGT after folding with & 0xDF (acgt are taken as ACGT).  min_overlap O, 1 <= O <= M (LiME_fasta's default: 3); max_err_pct E, whole
 * percent, 0 <= E <= 50 (default: 10).
 *   For a start p in [0, L): k(p) = min(M, L - p), the places at which read and adapter overlap; mm(p) = the number of j < k(p) with
 *   (s[p + j] & 0xDF) != a[j] -- lower case in the read matches; N, IUPAC codes and every other byte are mismatches.
 *   p is a hit when k(p) >= O and mm(p) <= (k(p) * E) / 100 by integer division.
 *   The read keeps s[0 .. p*), p* the SMALLEST hit; without a hit it is unchanged.  p* = 0 leaves an empty read.
 * Read indices never change, as for lime_quality_trim: an emptied read is an empty document and no read is dropped.
 * lime_adapter_trim is the loop form in plain host code, the oracle of lime_docs_trim_adapter_dev: text / doc_off[n_docs + 1] as the
 * readers give them; *out_text (at least one byte) and *out_doc_off[n_docs + 1] are library-owned (lime_free); info may be NULL.
 * LIME_ERR_ARG with a text: a NULL array, m of 0 or above 64, an adapter byte outside ACGTacgt, min_overlap of 0 or above m,
 * max_err_pct above 50, doc_off that does not start at 0 or decreases. */
int lime_adapter_trim(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint8_t *adapter, uint32_t m, uint32_t min_overlap,
                      uint32_t max_err_pct, uint8_t **out_text, uint64_t **out_doc_off, lime_trim_info_t *info);
/* The read filter: poly-X tails, a length cap, and reads dropped for their length, their N's or their complexity (what fastp and cutadapt
 * do behind the trims).  Integers only.  class(byte) is A, C, G or T after folding with & 0xDF (acgt are taken as ACGT); every other byte
 * -- N, IUPAC codes, anything -- is the one class "other".  The read is s[0 .. L).  The steps, in this order:
 *   1. Poly-X tail.  polyx_mask: bit 0 is A, bit 1 C, bit 2 G, bit 3 T; 0 switches the step off.  polyx_min T, 1 .. 255 (LiME_fasta's
 *      default: 10).  For a base X of the mask and a tail length t, 1 <= t <= L: mm_X(t) = the number of j in [L - t, L) with
 *      class(s[j]) != X.  t is admissible for X when t >= T, class(s[L - t]) = X and 8 * mm_X(t) <= t: one mismatch per eight symbols, and
 *      the tail begins with X.  t* = the LARGEST admissible t over every X of the mask, each X on its own; 0 without one.  hi = L - t*.
 *      Admissibility is not monotone in t: the rule takes the largest t, not the first run.
 *   2. Cap.  max_len K, 0 for none: hi = min(hi, K).
 *   3. Filters on the kept s[0 .. n), n = hi; the first that fails empties the read, and the read is counted under that reason alone.  A
 *      read that came in empty (L = 0) is counted nowhere.
 *        short           n < min_len (0: off).
 *        many N          the number of j < n with class(s[j]) = other exceeds max_n (LIME_FILTER_OFF: no limit).
 *        low complexity  min_complexity C, 0 .. 100 percent, 0 for off: with d = the number of j in [0, n - 1) with
 *                        class(s[j]) != class(s[j + 1]), the read fails when n >= 2 and 100 * d < C * (n - 1); n < 2 passes (fastp's
 *                        measure, taken on classes).
 * Read indices never change, as for both trims: an emptied read is an empty document and no read is dropped.
 * lime_filter_info_t: n_reads; n_polyx, the reads with t* > 0; n_capped, the reads that step 2 shortened; the reads each filter emptied;
 * the symbols before and after.
 * lime_read_filter is the loop form in plain host code, the oracle of lime_docs_filter_dev: text / doc_off[n_docs + 1] as the readers give
 * them; *out_text (at least one byte) and *out_doc_off[n_docs + 1] are library-owned (lime_free); info may be NULL.  LIME_ERR_ARG with a
 * text: a NULL array, polyx_mask above 15, polyx_min of 0 or above 255 while the mask is set, min_complexity above 100, every field at
 * its off value (nothing asked), doc_off that does not start at 0 or decreases. */
typedef struct { uint32_t polyx_mask, polyx_min, max_len, min_len, max_n, min_complexity; } lime_filter_t;
#define LIME_FILTER_OFF 0xFFFFFFFFu   /* max_n: no limit */
typedef struct { uint64_t n_reads, n_polyx, n_capped, n_short, n_many_n, n_low_complexity, symbols_in, symbols_out; } lime_filter_info_t;
int lime_read_filter(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const lime_filter_t *filter, uint8_t **out_text, uint64_t **out_doc_off,
                     lime_filter_info_t *info);
/* The overlap cut: adapter read-through found from the two mates of a pair alone, with no adapter sequence given (what fastp does for
 * paired data).  When the fragment (insert) is shorter than a read, both mates run through it into the adapter, and the first I symbols of
 * mate 1 are the reverse complement of the first I symbols of mate 2.  Integers only, on the strings as given.  Mates a[0 .. La) and
 * b[0 .. Lb) of pair r; min_overlap O >= 1 (LiME_fasta's default: 30); max_err_pct E, whole percent, 0 <= E <= 50 (default: 10).
 *   class(byte) is A, C, G or T after folding with & 0xDF (acgt are taken as ACGT); every other byte -- N, IUPAC codes, anything -- has no
 *   class and agrees with nothing, not even with itself.  comp swaps A / T and C / G.
 *   For a candidate insert length I the places are the j in [max(0, I - Lb), min(La, I)); n(I) = min(La, I) - max(0, I - Lb) is their
 *   number.  Place j agrees when a[j] has a class and class(a[j]) = comp(class(b[I - 1 - j])).  mis(I) = n(I) - the agreeing places.
 *   I is admissible when n(I) >= O and mis(I) <= (n(I) * E) / 100 by integer division.
 *   I* = the LARGEST admissible I in [O, La + Lb - O]: largest, not first-found and not best-scoring, so that it cuts least and a pair of
 *   low complexity with many admissible I is decided the same way everywhere.  Without one the pair is unchanged and insert[r] = 0.
 *   Mate 1 keeps a[0 .. min(La, I*)), mate 2 keeps b[0 .. min(Lb, I*)).  I* >= max(La, Lb) is an ordinary overlap of a long fragment: it
 *   cuts nothing and is still reported in insert[r].
 * Hence nothing is ever cut below O symbols and no read is emptied; an empty mate gives no overlap; read indices never change.
 * The rule is symmetric in the mates.  It runs LAST, behind each mate's quality trim, adapter trim and filter: it is the only stage that
 * needs both mates, and every per-mate stage makes the comparison cleaner.  So --min-len judges a read before this cut (the floor behind
 * it is O), and a 5' quality cut (Q5) moves a read's anchor: such a pair is judged on the strings as they are and usually has no overlap.
 * lime_overlap_info_t: n_pairs; n_overlap, the pairs with an I*; n_cut, the pairs of which a mate got shorter; the symbols of both mates
 * before and after.
 * lime_pair_overlap_trim is the loop form in plain host code, the oracle of lime_docs_trim_overlap_dev: two collections of n_docs reads
 * each; the four outputs as lime_adapter_trim's; *insert (may be NULL: not wanted) = I* per pair, n_docs words (at least one),
 * library-owned (lime_free); info may be NULL.  LIME_ERR_ARG with a text: a NULL array, min_overlap of 0, max_err_pct above 50, a doc_off
 * that does not start at 0 or decreases. */
typedef struct { uint64_t n_pairs, n_overlap, n_cut, symbols_in, symbols_out; } lime_overlap_info_t;
int lime_pair_overlap_trim(const uint8_t *text1, const uint64_t *doc_off1, const uint8_t *text2, const uint64_t *doc_off2, uint32_t n_docs,
                           uint32_t min_overlap, uint32_t max_err_pct, uint8_t **out_text1, uint64_t **out_doc_off1, uint8_t **out_text2,
                           uint64_t **out_doc_off2, uint32_t **insert, lime_overlap_info_t *info);
/* Per-position read statistics: what the reads look like, cycle by cycle (what fastp and FastQC report before and after filtering).
 * Integers only.  class(byte) is A, C, G or T after folding with & 0xDF, every other byte is the one class "other": the rule at
 * lime_read_filter.  Quality bytes are taken raw, with no offset removed (the reader of the tables subtracts 33).
 * n_pos, 1 .. LIME_QC_MAX_POS, is the number of positions with a row of their own; it need not be a multiple of 64.  The tables are
 * LIME_QC_WORDS(n_pos) words of uint64_t, in this order:
 *   row[p][8], p in 0 .. n_pos.  Row p < n_pos counts, over all reads with a symbol at position p: the symbols of class A, C, G, T and
 *     other (words 0 .. 4); qsum, the sum of the quality bytes at p (5); q20, the quality bytes >= 53 (6); q30, the quality bytes >= 63 (7).
 *     Row n_pos pools every position >= n_pos with the same eight counters, so that the five class counters summed over all rows are n_text.
 *   len_hist[n_pos + 1]: a read of length L adds 1 at min(L, n_pos); an empty read is counted at 0.
 *   gc_hist[101]: a read with acgt >= 1 symbols of a base class, gc of them C or G, adds 1 at (100 * gc) / acgt by integer division; a
 *     read without a base is counted nowhere.
 *   mq_hist[256]: a read with L >= 1 and qualities adds 1 at (the sum of its quality bytes) / L by integer division.
 * Documents without qualities (qual == NULL) leave qsum, q20, q30 and mq_hist untouched.
 * Every call ADDS to the caller's tables: batches, files and mates sum by calling again; the caller zeroes them.  Every word is exact
 * for any documents a lime_docs can hold: n_docs <= 2^32 - 1, n_text < 2^32, one document that may be the whole text.
 * lime_read_qc is the loop form in plain host code, the oracle of lime_docs_qc_dev.  LIME_ERR_ARG with a text: a NULL array (qual may be
 * NULL), n_pos of 0 or above LIME_QC_MAX_POS, doc_off that does not start at 0 or decreases. */
#define LIME_QC_MAX_POS 512u
#define LIME_QC_WORDS(n_pos) (9u * ((n_pos) + 1u) + 101u + 256u)
int lime_read_qc(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t n_pos, uint64_t *tables);
/* The statistics of n_files reads files as JSON, integers only, keys in a fixed order:
 *   {"lime_qc_report": 1, "positions": P, "files": [{"file": "...", "format": "fasta" | "fastq", "before": {...}, "after": {...}}, ...]}
 * before[k], after[k]: LIME_QC_WORDS(n_pos) words each, file k as parsed and as it enters classification; formats[k]: 0 FASTA, 1 FASTQ.
 * A section holds reads, empty, symbols, gc (the C + G symbols), bases {"A": [P + 1 numbers], "C", "G", "T", "other"}, length_hist,
 * gc_hist; `before` of a FASTQ file then q20, q30 (totals), qual_sum, qual_ge20, qual_ge30 (P + 1 numbers each) and mean_qual_hist
 * (256).  `after` never holds quality keys: the stages drop the qualities.  The file is written under a temporary name beside `path` and
 * renamed: a failure leaves no file.  LIME_ERR_ARG with a text: a NULL argument, n_files of 0, n_pos out of range, a format other than
 * 0 or 1; LIME_ERR_IO with a text when the file cannot be written.  Pure host code. */
int lime_qc_report_write(const char *path, uint32_t n_files, const char *const *names, const int *formats, uint32_t n_pos,
                         const uint64_t *const *before, const uint64_t *const *after);
/* *format = 1 (FASTQ) if the file's first byte is '@', else 0 (FASTA: an empty file and text in front of the first header included).
 * LIME_ERR_IO when the file cannot be read.  Pure host code. */
int lime_seq_format(const char *path, int *format);

/* ---- reads merged into a prebuilt genome index (eGap's role when the genome database is indexed once) ---------- *
 * lime_gindex: the index of the genome collection alone, left in HBM (ctx-owned, opaque; documents 0 .. n_refs - 1): text, doc_off,
 * sa, lcp (capped at the lcp_cap it was built with), da, ebwt, term: 14 bytes per genome position + 8 per genome.  Any number may live
 * at once; each is released by lime_gindex_free, or by lime_shutdown of its ctx (not both).  lime_gindex_build[_dev] are
 * lime_build_index[_dev] run on the genomes alone, keeping the suffix array (same arguments, limits, scratch and errors).
 *
 * The file (lime_gindex_save / _load / _probe), little-endian, written under a temporary name and renamed:
 *   header, 64 bytes:  0 magic "LGIX"   4 u16 version (1)   6 u8 term   7 u8 0   8 u32 n_docs   12 u32 lcp_cap   16 u64 n_text
 *                     24 u64 doc_off bytes = (n_docs + 1) * 8   32 u64 sa bytes   40 u64 lcp bytes   48 u64 da bytes (each N * 4,
 *                     N = n_text + n_docs)   56 u32 text bytes = n_text   60 u32 ebwt bytes = N
 *   body: the sections doc_off, sa, lcp, da, text, ebwt in this order, each padded with zeros to a multiple of 16 bytes; the file
 *         ends with the last section's padding.
 * load and probe check the magic, the version, every section size against n_docs and n_text, N <= 2^32 - 1 and the file's length;
 * load also checks doc_off by lime_build_index's rules before anything is indexed with it.  A file that is too short or cannot be
 * read: LIME_ERR_IO; one that is inconsistent: LIME_ERR_ARG; nothing stays allocated.  sa is NOT verified to be the sorted permutation
 * (the file is trusted as a .da file is): the merge clamps every value it indexes with, so a damaged file gives wrong output, no fault. */
typedef struct lime_gindex lime_gindex;
int lime_gindex_build(lime_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint8_t term, uint32_t lcp_cap,
                      lime_gindex **out);
int lime_gindex_build_dev(lime_ctx *ctx, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                          uint8_t term, uint32_t lcp_cap, void *stream, lime_gindex **out);
int lime_gindex_save(const lime_gindex *gi, const char *path);
int lime_gindex_load(lime_ctx *ctx, const char *path, lime_gindex **out);
int lime_gindex_info(const lime_gindex *gi, uint32_t *n_docs, uint64_t *n_text, uint32_t *lcp_cap, uint8_t *term);
/* the header and size checks of lime_gindex_load without a device (pure host code) */
int lime_gindex_probe(const char *path, uint32_t *n_docs, uint64_t *n_text, uint32_t *lcp_cap, uint8_t *term);
void lime_gindex_free(lime_gindex *gi);
/* A genome collection cut into index shards (pure host code): greedy in order, a shard takes consecutive genomes while its positions
 * (symbols + one terminator per genome) stay <= max_positions.  doc_off[n_docs + 1] as lime_gindex_build takes it; first_doc[0 ..
 * *n_shards] receive the cuts (shard s = genomes first_doc[s] .. first_doc[s + 1] - 1; first_doc[*n_shards] = n_docs), `cap` is the
 * number of entries first_doc holds.  No genome: *n_shards = 0.  LIME_ERR_ARG: a genome with more than max_positions positions (named
 * in lime_last_error(); a genome is never cut), max_positions = 0, more than cap - 1 shards. */
int lime_gindex_shard_plan(const uint64_t *doc_off, uint32_t n_docs, uint64_t max_positions, uint32_t *first_doc, uint32_t cap,
                           uint32_t *n_shards);

/* ebwt / lcp / da of the collection reads + genomes, bit for bit what lime_build_index[_dev] gives for it with the index's term and
 * the same lcp_cap, without sorting the genomes again: the reads are sorted alone (lime_build_index_dev's scratch, 52 bytes per READ
 * position, given back before the next step), every read suffix finds its place among the genome suffixes by a binary search over the
 * index's suffix array that compares text (a read suffix ends at its terminator, so a probe costs at most readLen / 8 word
 * compares), and both sides are written to their slots; the lcp of two neighbours of the same side is that side's own.
 * reads_text / reads_doc_off: the reads alone, as lime_build_index takes a collection (doc_off[0] = 0).  Outputs:
 * lime_merge_size elements each (reads' positions + the index's); any may be NULL.
 * lcp_cap must be servable from the index: an index built with cap 0 serves any cap, one built with cap c > 0 serves 1 .. c; anything
 * else, and more than 2^32 - 1 positions in all, is LIME_ERR_ARG before any launch.
 * Device memory next to the inputs and outputs, taken like lime_build_index_dev's and given back before the call returns: 17 bytes
 * per read position (the reads' sa, da, lcp, ebwt and j) and 8 per genome position (c and the words it is scanned from), after the
 * reads' build has returned its own scratch.  Synchronises `stream`.
 * Cost: the reads' own sort + about log2(genome positions) probes per read position + one pass over both sides.  Where the reads are most
 * of the collection this is SLOWER than lime_build_index_dev on reads + genomes (measured: DESIGN.md section 9 f7). */
uint64_t lime_merge_size(const lime_gindex *gi, const uint64_t *reads_doc_off, uint32_t n_reads);
int lime_merge_index_dev(lime_ctx *ctx, const uint8_t *d_reads_text, const uint64_t *d_reads_doc_off, uint32_t n_reads,
                         uint64_t n_reads_text, const lime_gindex *gi, uint32_t lcp_cap, uint8_t *d_ebwt, uint32_t *d_lcp,
                         uint32_t *d_da, void *stream);
/* host arrays, staged through HBM like lime_build_index */
int lime_merge_index(lime_ctx *ctx, const uint8_t *reads_text, const uint64_t *reads_doc_off, uint32_t n_reads,
                     const lime_gindex *gi, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da);
/* the last merge of the ctx: out[0] doubling rounds of the reads' build, out[1] read suffixes, out[2] runs of read suffixes in the
 * merged order; with lime_set_timing on, HIP-event ms of out[3] the reads' build, out[4] the rank search, out[5] placement + the lcp
 * across the sides; out[6], out[7] are 0 */
int lime_get_merge_info(lime_ctx *ctx, double out[8]);

/* ---- FASTA to documents on the device, and a whole sample from documents to verdicts ------------------------------ *
 * lime_docs: a document collection left in HBM (ctx-owned, opaque): text, the symbols back to back (16-byte aligned), and
 * doc_off[n_docs + 1] -- what lime_build_index_dev / lime_gindex_build_dev / lime_merge_index_dev take.  Any number may live at once; each
 * is released by lime_docs_free, or by lime_shutdown of its ctx (not both).
 * The from_* calls parse the raw bytes of a FASTA file with kernels and give exactly lime_fasta_read(path, 0)'s text and doc_off (a file
 * without a header line: n_docs = 0, doc_off = {0}).  The input is cut into blocks of LIME_FASTA_BLOCK bytes; three passes read it and
 * one writes the kept bytes: at most 4 bytes of HBM traffic per input byte.  Inputs of 2^32 bytes and more: LIME_ERR_ARG before any
 * launch.  Device memory next to the handle: the raw bytes (from_fasta / from_bytes; from_bytes_dev reads the caller's, at any alignment)
 * and 24 bytes per block; all of it is given back before the call returns.  The calls synchronise `stream` (from_fasta and from_bytes
 * work on the default stream). */
typedef struct lime_docs lime_docs;
int  lime_docs_from_fasta(lime_ctx *ctx, const char *path, lime_docs **out);   /* file -> pinned staging -> HBM -> parse; LIME_ERR_IO if unreadable */
int  lime_docs_from_bytes(lime_ctx *ctx, const uint8_t *bytes, uint64_t n, lime_docs **out);   /* host bytes of a FASTA file */
int  lime_docs_from_bytes_dev(lime_ctx *ctx, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out);
/* The same three for four-line FASTQ: exactly lime_fastq_read(path, 0)'s text and doc_off, and its refusals with the same code, line and
 * reason (the text starts with the name of the call that was made); on a refusal nothing stays allocated and *out is NULL.  The rule per
 * byte is at the head of lime_fastq_kernel.hip.  The same blocks, limit (2^32 - 1 bytes, refused before any launch), staging and
 * synchronisation as above: three passes read the input, one writes the kept bytes (the sequence lines); the offending line comes back with
 * the reads the call waits for anyway.  Device memory next to the handle: the raw bytes (from_fastq / from_fastq_bytes) and 24 bytes per
 * block (the blocks' counts of LF, of kept bytes and of kept minus quality bytes, and their prefix sums); all of it is given back before
 * the call returns. */
int  lime_docs_from_fastq(lime_ctx *ctx, const char *path, lime_docs **out);
int  lime_docs_from_fastq_bytes(lime_ctx *ctx, const uint8_t *bytes, uint64_t n, lime_docs **out);
int  lime_docs_from_fastq_bytes_dev(lime_ctx *ctx, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out);
/* The same three, keeping the quality strings: text, doc_off and every refusal (code, line, reason; the text starts with the name of the
 * call that was made) are exactly those of the calls above; next to them the handle holds qual[0 .. n_text), lime_fastq_read_qual's,
 * written by a fourth pass (lime_fqtrim_kernel.hip: k_fq_qual) from the prefix sums the other passes made: 1 more read per input byte
 * and 1 write per quality byte.  A malformed file may hold more quality bytes than sequence bytes: only qual[0 .. n_text) is ever
 * written, and the file is refused as above.  lime_docs_qual_device: *d_qual = the device pointer, or NULL for documents without
 * qualities -- those of every other lime_docs_from_*, of lime_docs_revcomp, lime_docs_trim_dev and a reader without set_trim.
 * lime_docs_get_qual: the host copy into the caller's n_text bytes; LIME_ERR_ARG for documents without qualities. */
int  lime_docs_from_fastq_qual(lime_ctx *ctx, const char *path, lime_docs **out);
int  lime_docs_from_fastq_qual_bytes(lime_ctx *ctx, const uint8_t *bytes, uint64_t n, lime_docs **out);
int  lime_docs_from_fastq_qual_bytes_dev(lime_ctx *ctx, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out);
int  lime_docs_qual_device(const lime_docs *docs, const uint8_t **d_qual);
int  lime_docs_get_qual(const lime_docs *docs, uint8_t *qual);
/* The documents cut by the rule at lime_quality_trim, on the device: *out = new documents (the caller's; no qualities) whose text and
 * doc_off are byte for byte lime_quality_trim's, *info (may be NULL) its counts.  k_trim_bounds finds (lo, hi) of every read -- 16 lanes
 * on a read, 256 quality bytes a step, the running sums carried in 64 bits -- one rocPRIM prefix sum places the new lengths, k_trim_copy
 * moves text[lo .. hi) and writes doc_off.  Device memory next to the two handles: 12 bytes per read + the prefix sum's, given back
 * before the call returns.  LIME_ERR_ARG with a text, before any launch: documents without qualities, a cutoff above 93, documents of
 * another context.  On every error nothing stays allocated and *out is NULL.  Synchronises `stream`. */
int  lime_docs_trim_dev(lime_ctx *ctx, const lime_docs *docs, uint32_t q5, uint32_t q3, void *stream, lime_docs **out, lime_trim_info_t *info);
/* The documents cut by the rule at lime_adapter_trim, on the device: *out = new documents (the caller's; no qualities) whose text and
 * doc_off are byte for byte lime_adapter_trim's, *info (may be NULL) its counts.  Any documents are taken: of a FASTA or FASTQ parse, with
 * or without qualities, or lime_docs_trim_dev's.  k_adapter_bounds (lime_adapter_kernel.hip) finds p* of every read -- one wave on a
 * read, 64 symbols a step, the read as four 64-bit words of ballots against the adapter's four masks -- and the prefix sum and
 * k_trim_copy of lime_docs_trim_dev follow.  Device memory next to the two handles: 12 bytes per read + the prefix sum's, given back
 * before the call returns.  LIME_ERR_ARG with a text, before any launch: a NULL argument, documents of another context, m of 0 or above
 * 64, an adapter byte outside ACGTacgt, min_overlap of 0 or above m, max_err_pct above 50.  On every error nothing stays allocated and
 * *out is NULL.  Synchronises `stream`. */
int  lime_docs_trim_adapter_dev(lime_ctx *ctx, const lime_docs *docs, const uint8_t *adapter, uint32_t m, uint32_t min_overlap, uint32_t max_err_pct,
                                void *stream, lime_docs **out, lime_trim_info_t *info);
/* The documents filtered by the rule at lime_read_filter, on the device: *out = new documents (the caller's; no qualities) whose text and
 * doc_off are byte for byte lime_read_filter's, *info (may be NULL) its counts.  Any documents are taken, with or without qualities, either
 * trim's output included.  k_filter_bounds (lime_filter_kernel.hip) finds what every read keeps -- one wave on a read, 64 symbols a word,
 * four class ballots a word: the tail walked from the last word down, the N's and the equal neighbours counted by set bits -- and the
 * prefix sum and k_trim_copy of lime_docs_trim_dev follow.  Device memory next to the two handles: 12 bytes per read + the prefix sum's,
 * given back before the call returns.  LIME_ERR_ARG with a text, before any launch: a NULL argument, documents of another context, and
 * lime_read_filter's refusals of the parameters.  On every error nothing stays allocated and *out is NULL.  Synchronises `stream`. */
int  lime_docs_filter_dev(lime_ctx *ctx, const lime_docs *docs, const lime_filter_t *filter, void *stream, lime_docs **out, lime_filter_info_t *info);
/* The statistics of the rule at lime_read_qc, on the device: tables (host memory, LIME_QC_WORDS(n_pos) words) += the documents' counts,
 * every word lime_read_qc's.  Any documents are taken; those with qualities fill the quality counters too.  k_qc_reads
 * (lime_qc_kernel.hip): one wave on a read, 64 symbols a word; the rows p < n_pos are counted in a per-workgroup table in LDS (32-bit
 * counters, counter-major), the pooled row (64-bit counters in LDS) and the per-read sums from set bits of ballots; every workgroup
 * adds its non-zero counters to the 64-bit tables once, at its end.  Device memory next to the handle: the tables, given back before
 * the call returns.  LIME_ERR_ARG with a text, before any launch: a NULL argument, documents of another context, n_pos of 0 or above
 * LIME_QC_MAX_POS.  No documents (n_docs = 0) add nothing.  On every error nothing stays allocated.  Synchronises `stream`. */
int  lime_docs_qc_dev(lime_ctx *ctx, const lime_docs *docs, uint32_t n_pos, void *stream, uint64_t *tables);
/* The two mates' documents cut by the rule at lime_pair_overlap_trim, on the device: *out1, *out2 = new documents (the caller's; no
 * qualities) whose texts and doc_off are byte for byte the oracle's, d_insert (device memory, n_docs words, may be NULL) its insert[],
 * *info (may be NULL) its counts.  Any documents are taken, as for the other trims; input qualities are dropped.  k_overlap_bounds
 * (lime_overlap_kernel.hip) finds I* of every pair -- one wave on a pair; mate 1 as four class ballots per 64 symbols, mate 2 as those of
 * its reverse complement, read backwards in place; a lane takes one candidate I, 64 candidates a step from the largest down, the agreeing
 * places counted as set bits of (a funnel-shifted window of one read's words) & (the other's) -- and per mate the prefix sum and
 * k_trim_copy of lime_docs_trim_dev follow.  The cost is quadratic in the read length.  Device memory next to the four handles: 24 bytes
 * per pair + the prefix sums', given back before the call returns.  LIME_ERR_ARG with a text, before any launch: a NULL argument, documents
 * of another context, collections of different n_docs, min_overlap of 0, max_err_pct above 50.  On every error nothing stays allocated
 * and *out1, *out2 are NULL.  Synchronises `stream`. */
int  lime_docs_trim_overlap_dev(lime_ctx *ctx, const lime_docs *docs1, const lime_docs *docs2, uint32_t min_overlap, uint32_t max_err_pct,
                                uint32_t *d_insert, void *stream, lime_docs **out1, lime_docs **out2, lime_overlap_info_t *info);
/* lime_docs_from_fastq or lime_docs_from_fasta, by lime_seq_format(path): the one place a file's format is decided */
int  lime_docs_from_file(lime_ctx *ctx, const char *path, lime_docs **out);
/* documents that are parsed already (copied); doc_off is checked on the device by lime_build_index's rules: LIME_ERR_ARG */
int  lime_docs_from_arrays_dev(lime_ctx *ctx, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                               void *stream, lime_docs **out);
/* every document reversed and complemented, byte for byte lime_fasta_read(path, 1)'s text (its table; doc_off is the same) */
int  lime_docs_revcomp(lime_ctx *ctx, const lime_docs *in, void *stream, lime_docs **out);
int  lime_docs_info(const lime_docs *docs, uint32_t *n_docs, uint64_t *n_text);
int  lime_docs_device(const lime_docs *docs, const uint8_t **d_text, const uint64_t **d_doc_off);
int  lime_docs_get(const lime_docs *docs, uint8_t *text, uint64_t *doc_off);   /* host copies into the caller's n_text bytes / n_docs + 1 words */
void lime_docs_free(lime_docs *docs);
/* A norm per read from the documents' own lengths: d_norms[r] (u8[n_docs], device memory) = len + 1 - alpha where len = doc_off[r + 1] -
 * doc_off[r] >= alpha -- the reference's norm = readLen + 1 - alpha (ClusterBWT_DA.cpp:555) with the read's own length -- and 1 for a shorter
 * read, which is in no alpha-cluster and whose rows are empty.  One pass over doc_off (k_rn_norms), 8 bytes come back.  LIME_ERR_ARG for
 * alpha == 0, and for a read of more than 255 symbols (the longest --readlen names, and the cells are bytes): the text gives the lowest such
 * read's index, counted from 0, and its length; d_norms is then unspecified.  Synchronises `stream`. */
int  lime_docs_norms_dev(lime_ctx *ctx, const lime_docs *docs, uint32_t alpha, uint8_t *d_norms, void *stream);

/* Preprocessing.sh + LiME_paired.sh for one sample whose reads and genome index are in HBM: n_mates = 1 (single-end) or 2 (paired-end)
 * read sets of equally many reads; the collections are worked on in the script's order F, F_RC, R, R_RC.  Each one: the reverse complement
 * (RC strands), lime_merge_index_dev into scratch arrays, lime_fused_choose_lists_dev (n_reads = the set's documents, n_refs = the
 * index's; no ebwt when use_ebwt == 0); the three arrays and the reverse complement are given back before the next collection starts, only
 * the lists stay.  Then lime_classify_lists_dev over the 2 or 4 lists, which are freed.  verdicts[n_reads], counts = {C, U, A, H};
 * stats (may be NULL): 2 * n_mates entries, the collections' scan counters.  lcp_cap: 0 = the index's own; else it must be servable
 * by the index (lime_merge_index_dev's rule).
 * Peak device memory next to the read sets and the index: one collection's arrays (9 bytes per position of reads + genomes, 8 without
 * ebwt) + the merge's scratch (17 bytes per read position + 8 per genome position, after the reads' build has returned its 52 per read
 * position) + the reverse complement (1 byte per read symbol + 8 per read) + the lists made so far; afterwards the scan's own.
 * LIME_ERR_ARG, with text in lime_last_error() and before any launch: n_mates other than 1 or 2, read sets with different document
 * counts, a read set without documents, alpha == 0, a taxonomy of another n_targ than the index's genomes, a cap the index cannot
 * serve or below alpha.  On any error nothing stays allocated.  Synchronises `stream`. */
/* norm = LIME_NORM_PER_READ (this call, lime_classify_sample_shards_dev and the two stream calls; every other call that takes a norm refuses
 * it with LIME_ERR_ARG): every read is normalised by its own length, for files whose reads differ in length (trimmed FASTQ).  Per mate
 * lime_docs_norms_dev gives the norms (F and RC of a mate share them); every collection's lists are made with beta -1 and
 * lime_lists_concat_norms_dev applies the real beta per read, for one shard or many; the stream calls take each batch's norms from the
 * batch's documents.  With reads of one length L the verdicts are those of norm = L + 1 - alpha.  A read shorter than alpha has empty rows.
 * A read of more than 255 symbols ends the call with LIME_ERR_ARG before any collection is made; the text names the read set (0 or 1) and
 * the read's index in the whole sample; nothing stays allocated (and the stream calls' caller is left without an output file). */
#define LIME_NORM_PER_READ 0xFFFFFFFFu
int lime_classify_sample_dev(lime_ctx *ctx, uint32_t n_mates, const lime_docs *const *mates, const lime_gindex *gi,
                             const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt, int binary,
                             uint32_t lcp_cap, lime_verdict_t *verdicts, uint64_t counts[4], lime_stats_t *stats, void *stream);
/* The same against a genome database cut into n_shards >= 1 indexes of one ctx (lime_gindex_shard_plan; shard s holds the genomes that
 * follow shard s - 1's, the taxonomy's order is their concatenation), all resident.  n_shards == 1 makes exactly the calls above.
 * Otherwise, per collection: the reverse complement once; per shard lime_merge_index_dev and lime_fused_choose_lists_dev with beta -1
 * (every non-zero row), the arrays given back before the next shard; lime_lists_concat_dev with the real beta; the shards' lists freed.
 * Then lime_classify_lists_dev with n_targ = the shards' genomes in all.  The verdicts are those of one index over all the genomes.
 * stats (may be NULL): n_shards * 2 * n_mates entries, shard-major (stats[s * 2 * n_mates + k]); they are PER-SHARD figures: a cluster
 * with genomes of three shards counts three times.  A cluster longer than LIME_MAX_CLUSTER over all genomes may be shorter in every
 * shard: sharding can succeed where the one index is LIME_ERR_MAXLEN, never the reverse.
 * Peak device memory next to the read sets: lime_classify_sample_dev's for the largest shard, plus the other shards (14 bytes per
 * genome position), plus one collection's unfiltered lists of all shards (8 bytes per non-zero cell + 9 per read and shard).
 * Refusals before any launch, next to the ones above: n_shards = 0, a NULL shard or one of another context, shards built with different
 * term or lcp_cap, a taxonomy whose n_targ is not the shards' genomes in all. */
int lime_classify_sample_shards_dev(lime_ctx *ctx, uint32_t n_mates, const lime_docs *const *mates, uint32_t n_shards,
                                    const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta,
                                    int use_ebwt, int binary, uint32_t lcp_cap, lime_verdict_t *verdicts, uint64_t counts[4],
                                    lime_stats_t *stats, void *stream);

/* ---- a reads file in batches of records, and a sample of any size classified batch by batch ------------------------ *
 * A read's verdict depends on that read and the genomes and on no other read, so a sample cut into batches of reads, each merged into
 * the same genome index, gives the verdicts of the whole sample.
 *
 * The cut (lime_seqcut_kernel.hip).  d_bytes[0 .. n), n <= 2^32 - 1, at any alignment, is a window of a reads file that begins at a record
 * start or is the file's first window; format is lime_seq_format's (0 FASTA, 1 FASTQ); max_reads >= 1; eof != 0: the window ends at the
 * file's end.  Out come *cut, *n_records = m and *n_markers: d_bytes[0 .. cut) holds exactly the next m whole records, d_bytes[cut .. n)
 * belongs to the next window.
 *   FASTQ  a marker is an LF, T their number.  eof and T / 4 < max_reads: cut = n and m = the records the parser will find or refuse
 *          (n_lines / 4; a last line without LF is a line).  Otherwise m = min(max_reads, T / 4) and cut = 1 + the position of LF number
 *          4m (counted from 1); m = 0: cut = 0.
 *   FASTA  a marker is a line-first '>' (byte i is '>' and i = 0 or byte i - 1 is LF), H their number.
 *          m = min(max_reads, eof ? H : max(H, 1) - 1).  cut = n where eof and m = H; otherwise cut = the position of marker number m
 *          counted from 0 (H = 0: cut = 0).  Bytes in front of the first marker of the file's first window stay in front of record 0,
 *          where the parser skips them.
 * One pass counts the markers per block of LIME_FASTA_BLOCK bytes, one prefix sum numbers them, one pass finds the wanted one; 24 bytes
 * come back.  Device memory: 8 bytes per block + the prefix sum's, given back before the call returns.  Synchronises `stream`. */
int lime_seq_cut_dev(lime_ctx *ctx, const uint8_t *d_bytes, uint64_t n, int format, uint32_t max_reads, int eof, void *stream,
                     uint64_t *cut, uint64_t *n_records, uint64_t *n_markers);

/* lime_seq_reader (ctx-owned, opaque): a FASTA or four-line FASTQ file, or such a file's bytes in host memory the caller keeps alive,
 * handed out in batches of records without ever being parsed whole.  window_bytes: the raw device window's size; 0 = 64 MiB, at most the
 * source's size; any value >= 1 is legal.
 * next: *docs = the next max_reads (>= 1) records as an ordinary lime_docs (the caller's, lime_docs_free); every batch but the last holds
 * exactly max_reads.  *docs = NULL with LIME_OK: the end of the file.  *first_record (may be NULL): the number of the batch's first record.
 * The window is refilled through two pinned buffers, cut (lime_seq_cut_dev) and parsed up to the cut with the passes of
 * lime_docs_from_bytes_dev / lime_docs_from_fastq_bytes_dev; the bytes behind the cut stay and move to the window's front only when it is
 * refilled.  A window that holds fewer than max_reads whole records and is not at the file's end is refilled; where it is full it is
 * doubled, up to 2^32 - 1 bytes, beyond which the call is LIME_ERR_ARG with a text that says so.
 * The batches' texts and offsets, concatenated, are byte for byte lime_fastq_read's / lime_fasta_read's of the whole file, for every
 * max_reads and every window_bytes.  A malformed FASTQ ends the call that meets it with the whole-file call's code, reason and line
 * number in the FILE; the batches before it have been handed out, *docs = NULL, nothing of that call stays allocated, and later calls
 * repeat the refusal.  More than 2^32 - 1 records in all: LIME_ERR_ARG.  LIME_ERR_IO where the file cannot be read.
 * Device memory: the window (+ a second one while it moves its tail or doubles), the cut's and the parse's scratch for one batch.
 * info: any pointer may be NULL; *n_lines counts FASTQ lines (4 per record handed out), 0 for FASTA.
 * A reader is released by lime_seq_reader_close, or by lime_shutdown of its ctx (not both).  The calls work on the default stream. */
typedef struct lime_seq_reader lime_seq_reader;
int  lime_seq_reader_open(lime_ctx *ctx, const char *path, uint64_t window_bytes, lime_seq_reader **out);
int  lime_seq_reader_open_bytes(lime_ctx *ctx, const uint8_t *bytes, uint64_t n, int format, uint64_t window_bytes, lime_seq_reader **out);
int  lime_seq_reader_next(lime_seq_reader *r, uint32_t max_reads, lime_docs **docs, uint64_t *first_record);
int  lime_seq_reader_info(const lime_seq_reader *r, int *format, uint64_t *n_records, uint64_t *n_lines, uint64_t *n_bytes,
                          uint64_t *window_bytes);
/* set_trim: from here on every batch is parsed with its qualities (lime_docs_from_fastq_qual_bytes_dev's passes) and handed out trimmed
 * (lime_docs_trim_dev with q5, q3): the batches, concatenated, are the whole file's trimmed documents.  LIME_ERR_ARG with a text: a FASTA
 * reader, a cutoff above 93, a reader whose lime_seq_reader_next has been called.  trim_info: the sums over the batches handed out so
 * far (zeros without set_trim). */
int  lime_seq_reader_set_trim(lime_seq_reader *r, uint32_t q5, uint32_t q3);
int  lime_seq_reader_trim_info(const lime_seq_reader *r, lime_trim_info_t *info);
/* set_adapter: from here on every batch is handed out cut at its reads' adapters (lime_docs_trim_adapter_dev), a FASTA reader's too.  With
 * set_trim as well every batch is quality-trimmed first and adapter-trimmed second (the order of an outside trimmer, and the only one:
 * the quality trim's output holds no qualities).  The batches, concatenated, are the whole file's trimmed documents.  LIME_ERR_ARG with a
 * text: the adapter's refusals as above, a reader whose lime_seq_reader_next has been called.  adapter_info: the sums over the batches
 * handed out so far (zeros without set_adapter); symbols_in counts what the adapter trim was given, the quality trim's output included. */
int  lime_seq_reader_set_adapter(lime_seq_reader *r, const uint8_t *adapter, uint32_t m, uint32_t min_overlap, uint32_t max_err_pct);
int  lime_seq_reader_adapter_info(const lime_seq_reader *r, lime_trim_info_t *info);
/* set_filter: from here on every batch is handed out filtered (lime_docs_filter_dev), a FASTA reader's too: third, behind the quality trim
 * and the adapter trim where those are set.  LIME_ERR_ARG with a text: lime_read_filter's refusals of the parameters, a reader whose
 * lime_seq_reader_next has been called.  filter_info: the sums over the batches handed out so far (zeros without set_filter); symbols_in
 * counts what the filter was given, the trims' output included. */
int  lime_seq_reader_set_filter(lime_seq_reader *r, const lime_filter_t *filter);
int  lime_seq_reader_filter_info(const lime_seq_reader *r, lime_filter_info_t *info);
/* set_overlap: links two readers of one ctx, the two mates' files, so that lime_seq_reader_next_pair hands out their batches cut by the
 * rule at lime_pair_overlap_trim.  The cut needs both mates of a batch, so it cannot sit in one reader's next: lime_seq_reader_next on a
 * linked reader alone hands out the UNCUT batch (each mate's own stages applied).  LIME_ERR_ARG with a text: a NULL reader, one reader
 * given twice, readers of different contexts, min_overlap of 0, max_err_pct above 50, a reader whose lime_seq_reader_next has been
 * called, a reader that is linked already.  Closing a linked reader unlinks the other.
 * next_pair: a batch of max_reads records from each reader, each through its own stages (quality trim, adapter trim, filter), then the
 * pair cut LAST (lime_docs_trim_overlap_dev).  *docs1 = *docs2 = NULL with LIME_OK: the end of both files.  LIME_ERR_ARG with a text:
 * readers that are not linked to each other, batches of different record counts (one file has ended before the other; both batches are
 * dropped).  The batches, concatenated, are the whole files' documents cut as one pair of collections.
 * overlap_info: the sums over the batches next_pair handed out so far, from either reader of the link (zeros without one). */
int  lime_seq_reader_set_overlap(lime_seq_reader *r1, lime_seq_reader *r2, uint32_t min_overlap, uint32_t max_err_pct);
int  lime_seq_reader_next_pair(lime_seq_reader *r1, lime_seq_reader *r2, uint32_t max_reads, lime_docs **docs1, lime_docs **docs2,
                               uint64_t *first_record);
int  lime_seq_reader_overlap_info(const lime_seq_reader *r, lime_overlap_info_t *info);
/* set_qc: from here on every batch adds to two sets of the tables of lime_read_qc (lime_docs_qc_dev), with n_pos rows: RAW (which = 0),
 * the batch as parsed -- a FASTQ reader then parses with qualities even without set_trim, and drops them behind this pass -- and OUT
 * (which = 1), the batch as handed out: by lime_seq_reader_next behind the reader's own stages, by lime_seq_reader_next_pair behind the
 * overlap cut (its inner next adds nothing: a batch is counted once).  The text and doc_off handed out, and whether the documents carry
 * qualities, are what they are without set_qc.  LIME_ERR_ARG with a text: a NULL reader, n_pos of 0 or above LIME_QC_MAX_POS, a reader
 * whose lime_seq_reader_next has been called.
 * qc: tables[0 .. LIME_QC_WORDS(n_pos)) = the sums over the batches so far (overwritten).  Without set_qc n_pos counts as 1 and the
 * LIME_QC_WORDS(1) words are zeros.  LIME_ERR_ARG with a text: a NULL argument, which above 1. */
int  lime_seq_reader_set_qc(lime_seq_reader *r, uint32_t n_pos);
int  lime_seq_reader_qc(const lime_seq_reader *r, int which, uint64_t *tables);
void lime_seq_reader_close(lime_seq_reader *r);

/* lime_classify_sample_dev batch by batch: per batch, batch_reads (>= 1) records from each of the n_mates readers, one unchanged
 * lime_classify_sample_dev call on them, then sink(user, first_read, verdicts, n, stats) with the batch's verdicts and its 2 * n_mates
 * scan counters (sink may be NULL), then the batch is freed.  counts (may be NULL) = {C, U, A, H} summed over the batches; *n_reads,
 * *n_batches (may be NULL) what was classified.  stats are PER-BATCH figures: a cluster with reads of three batches counts three times,
 * and max_len is that of the batch's part of a cluster; they are not the whole sample's numbers.  A cluster longer than
 * LIME_MAX_CLUSTER in the whole sample may be shorter in every batch: batching can succeed where the whole run is LIME_ERR_MAXLEN,
 * never the reverse.
 * Two readers that lime_seq_reader_set_overlap linked to each other are read with lime_seq_reader_next_pair: every batch is cut at the
 * mates' overlap before it is classified.  A reader linked to one that is not in the call is refused.
 * LIME_ERR_ARG before any read: lime_classify_sample_dev's argument refusals, a NULL reader or one of another context, batch_reads = 0.
 * A mate that ends before the other: LIME_ERR_ARG, "the read sets hold different numbers of reads" with both record counts (the longer
 * file is read to its end for it); no read at all: LIME_ERR_ARG.  A reader's refusal ends the call with it.  A non-zero return of the
 * sink ends the call with that value.  On any error nothing of this call stays allocated (the readers stay open, where they stopped).
 * Peak device memory, independent of the sample's size: lime_classify_sample_dev's for n_mates read sets of batch_reads reads (see
 * there: with P = a batch's read positions + the index's, 9 P for a collection's arrays + 17 per read position + 8 per genome position
 * of merge scratch + the reverse complement + the batch's lists) + the batch's documents + the readers' windows. */
typedef int (*lime_verdict_sink)(void *user, uint64_t first_read, const lime_verdict_t *verdicts, uint32_t n, const lime_stats_t *stats);
int lime_classify_sample_stream(lime_ctx *ctx, uint32_t n_mates, lime_seq_reader *const *readers, const lime_gindex *gi,
                                const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt, int binary,
                                uint32_t lcp_cap, uint32_t batch_reads, lime_verdict_sink sink, void *user, uint64_t counts[4],
                                uint64_t *n_reads, uint64_t *n_batches, void *stream);
/* The same with lime_classify_sample_shards_dev per batch; the sink's stats are the batch's n_shards * 2 * n_mates entries, shard-major. */
int lime_classify_sample_stream_shards(lime_ctx *ctx, uint32_t n_mates, lime_seq_reader *const *readers, uint32_t n_shards,
                                       const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta,
                                       int use_ebwt, int binary, uint32_t lcp_cap, uint32_t batch_reads, lime_verdict_sink sink, void *user,
                                       uint64_t counts[4], uint64_t *n_reads, uint64_t *n_batches, void *stream);

/* The classification file in parts: open writes the header under a temporary name, append the lines of verdicts[0 .. n) with the read
 * ids first_read + i, close(commit != 0) renames the file to `path`, close(0) removes it.  Appending the parts of a verdict array gives
 * lime_write_classification's file byte for byte.  Pure host code; errors in lime_classify_error(). */
typedef struct lime_classification_writer lime_classification_writer;
int lime_classification_writer_open(const char *path, lime_classification_writer **out);
int lime_classification_writer_append(lime_classification_writer *w, uint64_t first_read, const lime_verdict_t *verdicts, uint32_t n);
int lime_classification_writer_close(lime_classification_writer *w, int commit);

#ifdef __cplusplus
}
#endif
#endif /* LIME_HIP_H */
