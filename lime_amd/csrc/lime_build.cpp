// lime_build.cpp -- the index builder's host sequencing: ebwt / lcp / da from the sequences by prefix doubling, the kernels of
// lime_index_kernel.hip and rocPRIM's sorts and prefix sums (lime_index_sort.hip) in order (build_index_impl, behind
// lime_build_index_dev, lime_gindex_build_dev and the reads' side of lime_merge_index_dev), and the host-array front end.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "lime_index.h"
#include "lime_ctx.h"

using namespace lime;
using namespace lime_host;

// ---- ebwt / lcp / da from the sequences (lime_index_kernel.hip, lime_index_sort.hip; include/lime_hip.h) ------------------------------
extern "C" uint64_t lime_index_size(const uint64_t *doc_off, uint32_t n_docs) { return doc_off ? doc_off[n_docs] + n_docs : 0; }

extern "C" int lime_get_index_info(lime_ctx *c, double out[8])
{
    if (!c || !out) return fail(LIME_ERR_ARG, "lime_get_index_info: NULL argument");
    for (int k = 0; k < 8; ++k) out[k] = c->idx_info[k];
    return LIME_OK;
}

static uint32_t bits_for(uint64_t v) { uint32_t b = 0; while (b < 64u && (v >> b)) ++b; return b; }      // bits that hold 0 .. v

int lime_host::build_index_impl(lime_ctx *c, const char *who, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                                uint8_t term, uint32_t lcp_cap, uint8_t *d_ebwt, uint32_t *d_lcp, uint32_t *d_da, uint32_t *d_sa, hipStream_t st)
{
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    if (n_text > 0xFFFFFFFFull || n_text + n_docs > 0xFFFFFFFFull)
        return fail(LIME_ERR_ARG, "%s: %llu symbols + %u terminators exceed 2^32 - 1 positions (one GPU, 32-bit suffix positions)", who,
                    (unsigned long long)n_text, n_docs);
    if (!d_doc_off || (n_text && !d_text)) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if (!n_docs && n_text) return fail(LIME_ERR_ARG, "%s: %llu symbols in no document", who, (unsigned long long)n_text);
    int rc = check_ctx(c, who); if (rc) return rc;
    for (double &v : c->idx_info) v = 0.0;
    const uint32_t n = (uint32_t)(n_text + n_docs);
    if (!n) return LIME_OK;

    // rocPRIM's temporary storage: the largest of the calls below
    size_t tmp_bytes = 0;
    {
        IdxPairs q = {{nullptr, nullptr}, {nullptr, nullptr}, 0};
        size_t b = 0;
        HIP_TRY(idx_sort_pairs(nullptr, &b, &q, n, 0, 64, st)); tmp_bytes = std::max(tmp_bytes, b);
        HIP_TRY(idx_scan_sum(nullptr, &b, nullptr, nullptr, n, true, st)); tmp_bytes = std::max(tmp_bytes, b);
        HIP_TRY(idx_scan_sum(nullptr, &b, nullptr, nullptr, n, false, st)); tmp_bytes = std::max(tmp_bytes, b);
        HIP_TRY(idx_scan_max(nullptr, &b, nullptr, nullptr, n, st)); tmp_bytes = std::max(tmp_bytes, b);
    }
    // one block: 52 bytes per position (two key and two suffix buffers of the sort, two slot lists, two words of flags / sums, sa, rank,
    // doc_of) + rocPRIM's storage + the small words
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t w4 = up((size_t)n * 4), w8 = up((size_t)n * 8), small_bytes = up(256 * 4 + 256 * 2 + 64);
    DevBuf blk;
    if ((rc = blk.alloc(2 * w8 + 9 * w4 + up(tmp_bytes) + small_bytes)))
        return fail(rc, "%s: no device memory for %u positions (52 bytes each): %s", who, n, lime_last_error());
    uint8_t *at = static_cast<uint8_t *>(blk.p);
    auto take = [&](size_t b) { uint8_t *p = at; at += b; return p; };
    IdxPairs pr;
    pr.keys[0] = (uint64_t *)take(w8); pr.keys[1] = (uint64_t *)take(w8);
    pr.vals[0] = (uint32_t *)take(w4); pr.vals[1] = (uint32_t *)take(w4); pr.cur = 0;
    uint32_t *slots[2] = {(uint32_t *)take(w4), (uint32_t *)take(w4)};
    uint32_t *t1 = (uint32_t *)take(w4), *t2 = (uint32_t *)take(w4);
    uint32_t *sa = (uint32_t *)take(w4), *rank = (uint32_t *)take(w4), *doc_of = (uint32_t *)take(w4);
    void *tmp = take(up(tmp_bytes));
    uint32_t *present = (uint32_t *)take(small_bytes);
    uint16_t *code = (uint16_t *)(present + 256);
    uint32_t *words = (uint32_t *)(code + 256);                          // [0] doc_off is wrong, [1] sigma

    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
    if (c->timing) { for (auto &e : ev) HIP_TRY(hipEventCreate(&e)); HIP_TRY(hipEventRecord(ev[0], st)); }

    // the documents' bounds are checked before anything is indexed with them; dense codes of the bytes that occur
    HIP_TRY(hipMemsetAsync(present, 0, small_bytes, st));
    idx_launch_check(d_doc_off, n_docs, n_text, d_text, present, &words[0], st);
    idx_launch_codes(present, code, &words[1], st);
    HIP_TRY(hipGetLastError());
    uint32_t hw[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(hw, words, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hw[0]) return fail(LIME_ERR_ARG, "%s: doc_off must start at 0, never decrease and end at n_text (%llu)", who, (unsigned long long)n_text);
    const uint32_t bits = std::max(2u, bits_for(hw[1])), k_syms = std::min(64u / bits, 32u);
    const uint64_t low_mask = (1ull << bits) - 1u;
    const uint32_t nb = std::max(1u, bits_for((uint64_t)n - 1u));

    HIP_TRY(hipMemsetAsync(t1, 0, (size_t)n * 4, st));
    idx_launch_doc_heads(d_doc_off, n_docs, t1, st);
    HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, t1, doc_of, n, true, st));
    IdxText tx = {d_text, d_doc_off, doc_of, n_text, n_docs, n};
    idx_launch_pack(tx, code, k_syms, bits, pr.keys[0], pr.vals[0], st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(idx_sort_pairs(tmp, &tmp_bytes, &pr, n, 0, k_syms * bits, st));

    uint32_t m = n, rounds = 0;
    const uint32_t *slot = nullptr;                                      // NULL: element j sits at slot j (the first round)
    uint64_t mask = low_mask, h = k_syms;
    for (;;) {
        idx_launch_heads(pr.keys[pr.cur], slot, m, mask, t1, st);
        HIP_TRY(idx_scan_max(tmp, &tmp_bytes, t1, t2, m, st));
        idx_launch_settle(pr.keys[pr.cur], pr.vals[pr.cur], slot, t2, m, mask, n, rank, sa, t1, st);
        HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, t1, t2, m, false, st));
        HIP_TRY(hipGetLastError());
        uint32_t lastw[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&lastw[0], t1 + (m - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&lastw[1], t2 + (m - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t left = lastw[0] + lastw[1];
        if (left > m) return fail(LIME_ERR_HIP, "%s: internal error (%u of %u suffixes left)", who, left, m);
        if (rounds < 4) c->idx_info[1 + rounds] = (double)left;
        if (c->timing && rounds == 0) HIP_TRY(hipEventRecord(ev[1], st));
        if (!left) break;
        if (++rounds > 64) return fail(LIME_ERR_HIP, "%s: internal error (no end of the doubling rounds)", who);
        uint32_t *out_slot = slots[slot == slots[0] ? 1 : 0];
        idx_launch_compact(pr.vals[pr.cur], slot, t1, t2, m, pr.vals[pr.cur ^ 1], out_slot, st);
        pr.cur ^= 1; slot = out_slot; m = left; mask = 0;
        idx_launch_double(pr.vals[pr.cur], m, rank, n, h, nb, pr.keys[pr.cur], st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(idx_sort_pairs(tmp, &tmp_bytes, &pr, m, 0, 2 * nb, st));
        h *= 2;
    }
    c->idx_info[0] = (double)rounds;
    if (c->timing) HIP_TRY(hipEventRecord(ev[2], st));
    if (d_da || d_ebwt) idx_launch_gather(tx, sa, term, d_da, d_ebwt, st);
    if (d_lcp) idx_launch_lcp(tx, sa, rank, lcp_cap, d_lcp, st);
    if (d_sa) HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    if (c->timing) HIP_TRY(hipEventRecord(ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));                                   // (the scratch goes back when this returns)
    if (c->timing)
        for (int k = 0; k < 3; ++k) { float ms = 0.0f; if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) c->idx_info[5 + k] = ms; }
    return LIME_OK;
}

extern "C" int lime_build_index_dev(lime_ctx *c, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                                    uint8_t term, uint32_t lcp_cap, uint8_t *d_ebwt, uint32_t *d_lcp, uint32_t *d_da, void *stream)
{
    return build_index_impl(c, "lime_build_index_dev", d_text, d_doc_off, n_docs, n_text, term, lcp_cap, d_ebwt, d_lcp, d_da, nullptr, (hipStream_t)stream);
}

extern "C" int lime_build_index(lime_ctx *c, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint8_t term, uint32_t lcp_cap,
                                uint8_t *ebwt, uint32_t *lcp, uint32_t *da)
{
    if (!c) return fail(LIME_ERR_ARG, "lime_build_index: ctx is NULL");
    if (!doc_off) return fail(LIME_ERR_ARG, "lime_build_index: doc_off is NULL");
    if (doc_off[0] != 0) return fail(LIME_ERR_ARG, "lime_build_index: doc_off[0] is %llu, not 0", (unsigned long long)doc_off[0]);
    for (uint32_t k = 0; k < n_docs; ++k)
        if (doc_off[k + 1] < doc_off[k]) return fail(LIME_ERR_ARG, "lime_build_index: doc_off decreases at document %u", k);
    const uint64_t n_text = doc_off[n_docs];
    if (n_text > 0xFFFFFFFFull || n_text + n_docs > 0xFFFFFFFFull)
        return fail(LIME_ERR_ARG, "lime_build_index: %llu symbols + %u terminators exceed 2^32 - 1 positions (one GPU, 32-bit suffix positions)",
                    (unsigned long long)n_text, n_docs);
    if (n_text && !text) return fail(LIME_ERR_ARG, "lime_build_index: text is NULL");
    int rc = check_ctx(c, "lime_build_index"); if (rc) return rc;
    const uint64_t n = n_text + n_docs;
    if (!n) return LIME_OK;
    DevBuf dt, df, de, dl, dd;
    if ((rc = dt.upload(text, n_text)) || (rc = df.upload(doc_off, ((size_t)n_docs + 1) * 8))) return rc;
    if ((ebwt && (rc = de.alloc(n))) || (lcp && (rc = dl.alloc(n * 4))) || (da && (rc = dd.alloc(n * 4)))) return rc;
    rc = lime_build_index_dev(c, (const uint8_t *)dt.p, (const uint64_t *)df.p, n_docs, n_text, term, lcp_cap,
                              (uint8_t *)de.p, (uint32_t *)dl.p, (uint32_t *)dd.p, nullptr);
    if (rc) return rc;
    if (ebwt && (rc = d2h_pageable(c, ebwt, de.p, n, nullptr))) return rc;
    if (lcp && (rc = d2h_pageable(c, lcp, dl.p, n * 4, nullptr))) return rc;
    if (da && (rc = d2h_pageable(c, da, dd.p, n * 4, nullptr))) return rc;
    return LIME_OK;
}
