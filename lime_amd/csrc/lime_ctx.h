// lime_ctx.h -- what the host-side translation units of the library share (lime_api.cpp, lime_alloc.cpp, lime_pass.cpp, lime_stream.cpp,
// lime_choose.cpp, lime_build.cpp, lime_merge.cpp, lime_docs.cpp, lime_reader.cpp, lime_comm.cpp): the context and the lists object, error reporting, the device-block helpers and the
// declarations of the functions one file defines and another calls.  Internal: include/lime_hip.h is the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <vector>

#include "lime_hip.h"
#include "lime_kernels.h"

// Functions shared between the host files live here: hidden, so the library's dynamic symbol table holds the C ABI and nothing of these
namespace lime_host __attribute__((visibility("hidden"))) {
int fail(int code, const char *fmt, ...);                 // lime_api.cpp: sets what lime_last_error() returns (one thread_local string), returns code
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? LIME_ERR_NOMEM : LIME_ERR_HIP,            \
                        "%s: %s", #expr, hipGetErrorString(e_));                              \
    } while (0)

namespace lime_host __attribute__((visibility("hidden"))) {
// lime_alloc.cpp: device blocks through the process-wide cache
extern std::atomic<bool> g_debug_alloc, g_poison_cache;
void dev_release(void *p);
hipError_t dev_acquire(void **p, size_t bytes);

// One grow-only device array of a ctx: the pointer and its capacity (in elements) change together, so a growth that fails leaves an
// empty array (p == nullptr, cap == 0) and never a null pointer with its old capacity.  How much to ask for stays with the callers.
template <typename T> struct DevArr {
    T *p = nullptr;
    size_t cap = 0;
    DevArr() = default;
    DevArr(const DevArr &) = delete;
    DevArr &operator=(const DevArr &) = delete;
    ~DevArr() { release(); }
    void release() { if (p) dev_release(p); p = nullptr; cap = 0; }      // (large blocks stay in the process's cache: BlockCache)
    void swap(DevArr &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    // a block of `count` elements for an array that has none, by the plain path: no timing, no debug_alloc line (the lists' blocks, bigrec)
    int acquire(size_t count)
    {
        void *q = nullptr;
        HIP_TRY(dev_acquire(&q, count * sizeof(T)));
        p = static_cast<T *>(q); cap = count;
        return LIME_OK;
    }
    // the old block goes, a block of `count` elements comes; *account (may be NULL) += the host time spent in hipFree / hipMalloc
    int grow(size_t count, double *account)
    {
        const auto t0 = std::chrono::steady_clock::now();
        size_t f0 = 0, f1 = 0, tot = 0;
        const bool dbg = g_debug_alloc.load(std::memory_order_relaxed);
        if (dbg) (void)hipMemGetInfo(&f0, &tot);
        const bool had = p != nullptr;
        release();
        const auto t1 = std::chrono::steady_clock::now();
        void *q = nullptr;
        const hipError_t e = dev_acquire(&q, count * sizeof(T));
        const auto t2 = std::chrono::steady_clock::now();
        if (account) *account += std::chrono::duration<double, std::milli>(t2 - t0).count();
        if (dbg) {
            (void)hipMemGetInfo(&f1, &tot);
            fprintf(stderr, "regrow: %.3f GB%s release %.3f ms acquire %.3f ms; free before %.2f after %.2f of %.2f GB\n", (double)(count * sizeof(T)) / 1e9, had ? " (replaces a block)" : "",
                    std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(), (double)f0 / 1e9, (double)f1 / 1e9, (double)tot / 1e9);
        }
        HIP_TRY(e);
        p = static_cast<T *>(q); cap = count;
        return LIME_OK;
    }
    // room for `count` elements; whatever `st` still runs on the old block is waited for before it goes
    int ensure(size_t count, hipStream_t st, double *account)
    {
        if (count <= cap) return LIME_OK;
        HIP_TRY(hipStreamSynchronize(st));
        return grow(count, account);
    }
};
// a few words of fixed size, straight from hipMalloc (allocated once per ctx, never regrown)
template <typename T> struct DevWords {
    T *p = nullptr;
    DevWords() = default;
    DevWords(const DevWords &) = delete;
    DevWords &operator=(const DevWords &) = delete;
    ~DevWords() { if (p) dev_release(p); }
    int alloc(size_t bytes) { HIP_TRY(hipMalloc(&p, bytes)); return LIME_OK; }
};

// One mate's read-preparation stages (lime_docs.cpp: docs_stages runs them, in its one order): what the lime_seq_reader_set_* calls asked
// for, each stage's counts summed over the batches handed out, and the statistics of the batches as parsed and as handed out
struct MateStages {
    bool trim = false; uint32_t q5 = 0, q3 = 0;            // lime_seq_reader_set_trim
    bool adapter = false; uint64_t ad_masks[4] = {0, 0, 0, 0}; uint32_t ad_m = 0, ad_overlap = 0, ad_err = 0;     // lime_seq_reader_set_adapter
    bool filter = false; lime_filter_t fl = {0, 0, 0, 0, LIME_FILTER_OFF, 0};      // lime_seq_reader_set_filter
    uint32_t n_pos = 0;                                    // lime_seq_reader_set_qc; 0 without
    lime_trim_info_t trimmed = {0, 0, 0, 0, 0}, ad_trimmed = {0, 0, 0, 0, 0};
    lime_filter_info_t filtered = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> qc_raw, qc_out;
    bool needs_qual() const { return trim || n_pos; }      // does any stage read the qualities of a FASTQ batch?
};

// a stage's counts for one batch added to the sum over the batches
inline void add_info(lime_trim_info_t &s, const lime_trim_info_t &x)
{
    s.n_reads += x.n_reads; s.n_changed += x.n_changed; s.n_empty += x.n_empty; s.symbols_in += x.symbols_in; s.symbols_out += x.symbols_out;
}
inline void add_info(lime_filter_info_t &s, const lime_filter_info_t &x)
{
    s.n_reads += x.n_reads; s.n_polyx += x.n_polyx; s.n_capped += x.n_capped; s.n_short += x.n_short; s.n_many_n += x.n_many_n;
    s.n_low_complexity += x.n_low_complexity; s.symbols_in += x.symbols_in; s.symbols_out += x.symbols_out;
}
inline void add_info(lime_overlap_info_t &s, const lime_overlap_info_t &x)
{
    s.n_pairs += x.n_pairs; s.n_overlap += x.n_overlap; s.n_cut += x.n_cut; s.symbols_in += x.symbols_in; s.symbols_out += x.symbols_out;
}
}

struct __attribute__((visibility("hidden"))) lime_ctx {              // (hidden: its implicit destructor is no export of the library)
    int device = 0;
    lime_host::DevWords<lime::DevStats> stats;                // followed by the sticky word: passes with a pool overflow not settled by lime_get_stats
    uint32_t *d_sticky = nullptr;
    // clusterChoose's scratch, kept between calls (round 5: per call four hipMalloc / hipFree pairs, two 4 MB copies into pageable vectors and 10^6
    // float divisions were 1.3 ms of configs[2]'s 4.3 ms lime_fused_choose_dev): device words for the rows' max / non-zero counts (+ the
    // table-free finish's region words), pinned host words where they land
    lime_host::DevArr<uint8_t> choose;
    void *h_choose = nullptr; size_t h_choose_cap = 0;
    void *h_stats = nullptr;                    // pinned: where read_stats lands the counters (a copy into pageable memory is staged by the runtime: +30 us per call)
    lime_host::DevWords<unsigned long long> total;
    // per-tile scratch (capacities in tiles; the first four grow together: ensure_scratch)
    lime_host::DevArr<lime::TileSummary> summ;
    lime_host::DevArr<uint32_t> tile_cnt;
    lime_host::DevArr<uint64_t> tile_off;
    lime_host::DevArr<lime::CrossRec> cross;
    lime_host::DevArr<lime::WinMasks> wmask;
    // cluster lists
    lime_host::DevArr<lime_cluster_t> small, big, out;
    lime_host::DevArr<uint32_t> big_scratch;
    uint32_t max_blocks = 0;                // persistent grid of the scan kernel; 0 = as many workgroups as fit the device (LIME_MAX_BLOCKS)
    uint32_t list_blocks = 8192;
    int ablate = 0;                         // LIME_ABLATE (only in a -DLIME_ABLATE_BUILD library): kernel timing experiments, results invalid when != 0
    // binned table updates (bin-then-apply): record pool, per-bin counters, binned records
    lime_host::DevArr<uint32_t> pool, recs;             // 32-bit records (n_waves x n_sub x cap_w); both allocated with 16 records of slack (ensure_binned)
    lime_host::DevArr<uint32_t> wave_cnt, counts;
    lime_host::DevWords<uint32_t> totals; lime_host::DevWords<uint64_t> binbase;
    lime_host::DevArr<uint64_t> regbase;
    lime_host::DevWords<uint32_t> tbase;                  // second level by tiles: tiles before each bin, and the tiles' region index
    lime_host::DevArr<uint16_t> tidx;
    bool by_tiles = true;                   // LIME_SECOND_LEVEL=sweeps: k_part2 + k_apply instead (comparison runs)
    // owner-partitioned exchange: the long clusters' update records of this rank; the owner's regrouped records
    lime_host::DevArr<uint64_t> bigrec; lime_host::DevWords<uint32_t> bigrec_n;
    lime_host::DevArr<uint32_t> xrecs, xrecs2;         // (grow together: lime_apply_records_dev)
    lime_host::DevArr<uint64_t> xoff, xreg;
    uint64_t *h_xoff = nullptr; size_t h_xoff_cap = 0; hipEvent_t ev_xoff = nullptr; bool ev_xoff_pending = false;   // pinned staging of the offsets lime_apply_records_dev uploads (no stream synchronisation in an exchange step)
    uint32_t rec_n_bins = 0, rec_bin_shift = 0;                // layout of the records the last lime_fused_records_dev left
    int upd_pref = -1;                      // LIME_UPDATE_PATH: -1 auto, 0 compare-and-swap on the table, 1 binned
    bool density_known = false; double density = 0.0;          // table updates per owned symbol of the last pass read back
    bool bin_levels_forced = false;
    uint32_t bin_one_level = lime::BIN_ONE_LEVEL, bin_two_level = lime::BIN_TWO_LEVEL;   // LIME_BIN_LEVELS="a,b" (tests: force the second level on small tables)
    double pool_density = 0.45;             // records per owned symbol the pool is sized for before anything has been measured (first passes below 2^28 symbols, which run without the density probe: text has 0.24 .. 0.39; grows on LIME_FLAG_POOL_FULL)
    bool pool_density_fixed = false;        // set by LIME_POOL_DENSITY or by a repeated pass: sizing_density() then leaves it alone
    int scan_static_pct = -1;               // share (%) of the scan's rounds of window chunks that go round-robin, the rest is handed out as workgroups get there; -1: by the input's length (base_args); LIME_SCAN_STATIC_PCT: tests, comparison runs
    uint32_t part_split = 2;                // producers (of k_part) per scan workgroup at most (LIME_PART_SPLIT: comparison runs): two = one partition workgroup per resident slot of the device; four -- round 4's first choice -- cut the streams into more, less filled tiles: k_part_lines +4 % at N = 1e10 and on the text workload
    uint32_t pool_slack = 512;              // + this many records per wave and sub-region (LIME_POOL_SLACK: tests make pools overflow)
    uint64_t probe_min = 1ull << 28;        // first passes of fewer symbols run without the density probe (binned, pool for 0.45 records per symbol); LIME_PROBE_MIN: tests
    bool probe = true;                      // LIME_NO_PROBE: no sampled density probe in front of a ctx's first pass (tests, comparison runs)
    bool force_p64 = false;                 // LIME_FORCE_P64: the partition kernels' 64-bit-position variants on any pass (tests)
    uint64_t p64_test_base = 0;             // LIME_P64_TEST_BASE (tests): the binned records' positions start at this number instead of 0 -- the bin bases are
                                            // shifted by it and the kernels get the records' array address minus it --, so that a small pass crosses a multiple of 2^32
    double alloc_ms = 0.0, probe_ms = 0.0; uint32_t n_probes = 0, n_repeats = 0, n_fallbacks = 0, n_table_free = 0;   // host-side costs a cold pass pays (lime_get_host_times)
    struct Last {                           // the last lime_fused_dev call, so that lime_get_stats can repeat it with a larger pool
        bool valid = false, binned = false;
        const uint32_t *lcp = nullptr, *da = nullptr; const uint8_t *ebwt = nullptr;
        uint64_t n_own = 0, n_avail = 0; int eof = 0; uint32_t n_reads = 0, n_refs = 0, alpha = 0;
        uint8_t *sim = nullptr; int zero_sim = 0; hipStream_t st = nullptr; uint32_t n_waves = 0; bool records_only = false;
        uint64_t own_total = 0;             // owned symbols the counters in d_stats stand for (chunks of a stream accumulate)
        double share = 1.0;                 // binned: the part of a wave's records one sub-region was sized for (sub_share)
        bool fell_back = false;             // the binned path was wanted and could not be had (memory): LIME_FLAG_CAS_FALLBACK
    } last;
    // knobs of lime_set_option that have no other home (all -1 / 0 / false = the library's own choice)
    int apply_wide = -1, sort_nt = -1, part_lines = -1;     // which variant of k_apply_tiles / of k_sort_tiles' row stores / whether k_part_lines may run
    int choose_free = -1;                   // lime_fused_choose_dev: 1 = without the table wherever the layout has a second level, 0 = never
    bool no_staging = false, force_staging = false, force_rccl = false, debug_stats = false;
    uint64_t detect_chunk = 0, score_chunk = 0;             // symbols per chunk of lime_detect / lime_score* walks (0: by the sources)
    bool no_direct = false;                 // binned updates through the update queue (k_scan<., 0, 1>) even for tables of one or two sub-regions (option no_direct: comparison runs, tests)
    uint32_t dense_min = 64;                // k_scan: windows with more accepted clusters list their 2-symbol clusters apart (option dense_min; tests: 0 = every window)
    uint32_t flush_gran = 0;                // k_scan<., 0, 2>: records per batch that leaves at a window's top (option flush_gran: 16 or 64; 0 = by the table's sub-regions)
    int io_threads = 0;                     // host threads that stage pageable sources into the pinned ring (0: 8, at most the CPUs this process may use)
    // timing with HIP events on the launch stream: per pass {pass start, scan start, scan end, pass end}
    bool timing = false;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    double cls_ms = 0.0;                    // the last lime_classify_lists_dev kernel (timing on)
    double idx_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // the last lime_build_index_dev (lime_get_index_info)
    double mrg_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // the last lime_merge_index_dev (lime_get_merge_info)
    double lc_info[4] = {0, 0, 0, 0};                       // the last lime_lists_concat_dev (lime_get_concat_info)
    std::vector<lime_lists *> lists;        // clusterChoose results left in HBM that are still alive (lime_lists_free / lime_shutdown)
    std::vector<lime_gindex *> gidx;        // genome indexes left in HBM that are still alive (lime_gindex_free / lime_shutdown)
    std::vector<lime_docs *> docs;          // document collections left in HBM that are still alive (lime_docs_free / lime_shutdown)
    std::vector<lime_seq_reader *> readers; // open readers of reads files (lime_seq_reader_close / lime_shutdown)
};

// one collection's clusterChoose result in HBM: [row_off u64[n_reads + 1]][row_max u8[n_reads]] in one block, the pairs in another
struct __attribute__((visibility("hidden"))) lime_lists {
    lime_ctx *ctx = nullptr;
    uint32_t n_reads = 0, norm = 0; float beta = 0.0f;
    uint64_t n_pairs = 0;
    lime_host::DevArr<uint8_t> rows;
    lime_host::DevArr<lime_pair_t> pairs;
    lime_host::DevArr<uint8_t> norms;       // a norm per read (lime_lists_concat_norms_dev: u8[n_reads], and norm is 0), else empty
    bool per_read() const { return norms.p != nullptr; }
    const uint64_t *row_off() const { return reinterpret_cast<const uint64_t *>(rows.p); }
    const uint8_t *row_max() const { return rows.p + ((size_t)n_reads + 1) * 8; }
};

// a genome collection's index in HBM (lime_merge.cpp): one block, the sections in the order and at the offsets of the file's body
// (doc_off, sa, lcp, da, text, ebwt, each 16-byte aligned), so that save and load are one copy each
struct __attribute__((visibility("hidden"))) lime_gindex {
    lime_ctx *ctx = nullptr;
    uint32_t n_docs = 0, lcp_cap = 0; uint8_t term = 0;
    uint64_t n_text = 0;
    lime_host::DevArr<uint8_t> blk;
    uint64_t n() const { return n_text + n_docs; }
    static uint64_t up16(uint64_t b) { return (b + 15u) & ~(uint64_t)15; }
    uint64_t off_sa() const { return up16(((uint64_t)n_docs + 1) * 8); }
    uint64_t off_lcp() const { return off_sa() + up16(n() * 4); }
    uint64_t off_da() const { return off_lcp() + up16(n() * 4); }
    uint64_t off_text() const { return off_da() + up16(n() * 4); }
    uint64_t off_ebwt() const { return off_text() + up16(n_text); }
    uint64_t body_bytes() const { return off_ebwt() + up16(n()); }
    uint64_t *doc_off() const { return reinterpret_cast<uint64_t *>(blk.p); }
    uint32_t *sa() const { return reinterpret_cast<uint32_t *>(blk.p + off_sa()); }
    uint32_t *lcp() const { return reinterpret_cast<uint32_t *>(blk.p + off_lcp()); }
    uint32_t *da() const { return reinterpret_cast<uint32_t *>(blk.p + off_da()); }
    uint8_t *text() const { return blk.p + off_text(); }
    uint8_t *ebwt() const { return blk.p + off_ebwt(); }
};

// a document collection in HBM (lime_docs.cpp): the symbols back to back (16-byte aligned, at least one byte) and doc_off[n_docs + 1]
struct __attribute__((visibility("hidden"))) lime_docs {
    lime_ctx *ctx = nullptr;
    uint32_t n_docs = 0;
    uint64_t n_text = 0;
    lime_host::DevArr<uint8_t> text;
    lime_host::DevArr<uint64_t> doc_off;
    lime_host::DevArr<uint8_t> qual;        // the reads' quality bytes, laid out like text (lime_docs_from_fastq_qual*), or none
};

// a reads file handed out in batches of records (lime_reader.cpp): the raw bytes win[start .. fill) of the file, which begin at a record
// start (or are the file's first bytes), in a device window that is refilled through two pinned buffers and doubled where a batch does not fit
struct __attribute__((visibility("hidden"))) lime_seq_reader {
    lime_ctx *ctx = nullptr;
    int format = 0;                         // 0 FASTA, 1 FASTQ
    FILE *f = nullptr;                      // the source: a file ...
    const uint8_t *host = nullptr;          // ... or the caller's bytes
    uint64_t src_size = 0, src_pos = 0;     // the source's bytes, and how many of them have gone to the window
    lime_host::DevArr<uint8_t> win;         // win.cap = the window size (+ 16 allocated)
    uint64_t start = 0, fill = 0;
    void *pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; size_t pin_bytes = 0; int pin_k = 0;
    uint64_t n_records = 0, n_lines = 0, n_bytes = 0;      // handed out so far
    int failed = 0; std::string failure;    // a refusal is final: later calls repeat it
    bool asked = false;                     // lime_seq_reader_next has been called
    lime_host::MateStages stages;           // what every batch goes through before it is handed out
    lime_seq_reader *mate = nullptr; uint32_t ov_overlap = 0, ov_err = 0;       // lime_seq_reader_set_overlap: the other mate's reader; next_pair cuts
    lime_overlap_info_t overlapped = {0, 0, 0, 0, 0};      // every batch of the two at the mates' overlap, last (the sums: kept in both readers)
    ~lime_seq_reader();
};

namespace lime_host __attribute__((visibility("hidden"))) {
inline int check_ctx(lime_ctx *c, const char *who)
{
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    HIP_TRY(hipSetDevice(c->device));
    return LIME_OK;
}

inline bool misaligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) dev_release(p); }                  // (large ones stay in the process's block cache)
    int alloc(size_t bytes) { HIP_TRY(dev_acquire(&p, bytes ? bytes : 16)); return LIME_OK; }
    int upload(const void *src, size_t bytes) {
        int rc = alloc(bytes + 16); if (rc) return rc;
        if (bytes) HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return LIME_OK;
    }
};

// The scratch of a pass over `count` items in one block: n_arr arrays of count + 1 32-bit words, each rounded up to 256 bytes, then one
// 256-byte cell (an error word, a few counters), then rocPRIM's temporary of tmp_bytes
struct WordScratch {
    DevBuf buf;
    size_t stride = 0, n_arr = 0, tmp_bytes = 0;         // stride: the bytes of one array
    static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
    int alloc(size_t arrays, size_t count, size_t tmp)
    {
        n_arr = arrays; stride = up((count + 1) * 4); tmp_bytes = tmp;
        return buf.alloc(n_arr * stride + 256 + up(tmp_bytes));
    }
    uint32_t *words(size_t i) const { return reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(buf.p) + i * stride); }
    void *cell() const { return words(n_arr); }
    void *tmp() const { return static_cast<uint8_t *>(cell()) + 256; }
};

// lime_api.cpp
int flags_to_rc(uint32_t flags);
int timing_mark(lime_ctx *c, hipStream_t st);
int read_stats(lime_ctx *c, lime_stats_t *s, hipStream_t st, uint32_t *sticky = nullptr);
// lime_pass.cpp
double sizing_density(const lime_ctx *c);
void bin_layout_of(uint32_t one_level, uint32_t two_level, bool levels_forced, size_t sim_bytes, uint32_t *n_bins, uint32_t *bin_shift_out);
void bin_layout(const lime_ctx *c, size_t sim_bytes, uint32_t *n_bins, uint32_t *bin_shift_out);
void sub_layout(size_t sim_bytes, uint32_t n_refs, uint32_t *n_sub, uint32_t *sub_rb, uint32_t *sub_gb);
bool many_records_of(const lime_ctx *c, double records);
bool big_rows_of(const lime_ctx *c, double records);
int fused_dev_impl(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt,
                   uint64_t n_own, uint64_t n_avail, int eof, uint32_t n_reads, uint32_t n_refs,
                   uint32_t alpha, uint8_t *d_sim, int zero_sim, bool keep_stats, hipStream_t st,
                   uint32_t *d_edge = nullptr, bool no_bin = false, bool records_only = false);
int score_dev_impl(lime_ctx *c, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                   const lime_cluster_t *d_clusters, uint64_t n_clusters, uint32_t n_reads,
                   uint32_t n_refs, uint8_t *d_sim, int zero_sim, uint64_t pos_base, hipStream_t st);
// lime_build.cpp: the index builder behind lime_build_index_dev, lime_gindex_build* and the reads' side of lime_merge_index_dev;
// d_sa (may be NULL) receives the suffix array (u32[N]); `who` names the public call in error messages
int build_index_impl(lime_ctx *c, const char *who, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                     uint8_t term, uint32_t lcp_cap, uint8_t *d_ebwt, uint32_t *d_lcp, uint32_t *d_da, uint32_t *d_sa, hipStream_t st);
// lime_docs.cpp: the device parsers behind lime_docs_from_* on d_bytes[0 .. n), n < 2^32; line_base: the lines in front of d_bytes[0]
int docs_parse_fasta_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, hipStream_t st, lime_docs **out);
int docs_parse_fastq_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, uint64_t line_base, hipStream_t st, lime_docs **out,
                         bool with_qual = false);
// lime_docs.cpp: the adapter's refusals (LIME_ERR_ARG with a text) and its four masks, bit j of masks[b] set where symbol j is "ACGT"[b]
int adapter_masks(const char *who, const uint8_t *adapter, uint32_t m, uint32_t min_overlap, uint32_t max_err_pct, uint64_t masks[4]);
// lime_host.cpp: the filter's refusals of its parameters (LIME_ERR_ARG with a text)
int filter_check(const char *who, const lime_filter_t *f);
// lime_host.cpp: the overlap cut's refusals of its parameters (LIME_ERR_ARG with a text); lime_docs.cpp: lime_docs_trim_overlap_dev without
// its argument checks
int overlap_check(const char *who, uint32_t min_overlap, uint32_t max_err_pct);
int docs_overlap_impl(lime_ctx *c, const char *who, const lime_docs *docs1, const lime_docs *docs2, uint32_t min_overlap, uint32_t max_err_pct,
                      uint32_t *d_insert, hipStream_t st, lime_docs **out1, lime_docs **out2, lime_overlap_info_t *info);
// lime_docs.cpp: one mate's stages on a batch as parsed (*docs is replaced by what they leave; NULL and nothing allocated on an error), and
// a batch as it is handed out added to the mate's OUT tables (on an error the batch, and the pair's other batch if given, are freed and NULL)
int docs_stages(lime_ctx *c, const char *who, MateStages &s, lime_docs **docs);
int docs_count_out(lime_ctx *c, const char *who, MateStages &s, lime_docs **batch, lime_docs **other = nullptr);
// lime_docs.cpp: the genome side's refusals of the sample calls, with one index or with shards (the read sets' own come between the two)
int sample_check_shards(const char *who, lime_ctx *c, uint32_t n_shards, const lime_gindex *const *shards);
int sample_check_rules(const char *who, uint32_t n_shards, const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha,
                       uint32_t lcp_cap, uint32_t *n_refs, uint32_t *cap);
// lime_docs.cpp: the reads' norms of lime_docs_norms_dev without its refusal: *n_long reads hold more than 255 symbols, the lowest of them is
// *first with *first_len symbols (d_norms is then unspecified); the callers word the refusal
int docs_norms_impl(lime_ctx *c, const lime_docs *docs, uint32_t alpha, uint8_t *d_norms, hipStream_t st, uint32_t *n_long, uint32_t *first,
                    uint64_t *first_len);
// lime_docs.cpp: lime_classify_sample_dev / lime_classify_sample_shards_dev for a batch whose first read is read_base of the whole sample
// (a refusal under LIME_NORM_PER_READ names the read by its index in the sample)
int classify_sample_at(const char *who, lime_ctx *c, uint32_t n_mates, const lime_docs *const *mates, uint32_t n_shards,
                       const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt, int binary,
                       uint32_t lcp_cap, lime_verdict_t *verdicts, uint64_t counts[4], lime_stats_t *stats, void *stream, uint64_t read_base);
// lime_stream.cpp
int score_in_chunks(lime_ctx *c, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                    const lime_cluster_t *clusters, uint64_t n_clusters, uint32_t n_reads, uint32_t n_refs,
                    uint8_t *d_sim);
int d2h_pageable(const lime_ctx *c, void *dst, const void *d_src, size_t bytes, hipStream_t st);    // large results into the caller's pageable memory: staged by this library's threads
}

// Internal entry points other translation units call; not in include/lime_hip.h
int lime_internal_records_peek(lime_ctx *c, lime_records_t *out, const uint32_t **d_bigrec_n, uint32_t *bigrec_cap);   // lime_pass.cpp: no synchronisation
int lime_internal_upload(int n_arr, const void *const *src, void *const *dst, const size_t *bytes, hipStream_t st);   // lime_stream.cpp: through the pinned staging ring
int lime_internal_reduce_scatter(int n_dev, const int *devs, uint8_t *const *d_sim, uint8_t *const *d_blk, size_t blk);   // lime_comm.cpp
