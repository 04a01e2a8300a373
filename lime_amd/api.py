"""Host-side mirror of the reference's interface for the hot path.

The reference exposes two programs (argv + files): `ClusterLCP fileFasta numReads numGenomes
alpha threads` (src/ClusterLCP.cpp:56-71) and `ClusterBWT_DA fileFasta readLen beta threads`
(src/ClusterBWT_DA.cpp:496-529).  `cluster_lcp` / `cluster_bwt_da` below take the same
arguments and read/write the same files; `detect` / `score` / `fused` / `choose` are the
array-level calls underneath (numpy in, numpy out), all through the C ABI in
include/lime_hip.h -- i.e. through the HIP kernels.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Cluster, LimeError, Stats, check, check_cls  # noqa: F401

# lime_verdict_t: one read's classification (type C/U/A/H as a byte, rule 0 = U, 1, 2, 3)
FASTA_BLOCK = _lib.FASTA_BLOCK          # LIME_FASTA_BLOCK: input bytes one workgroup pass of the device FASTA parser handles
NORM_PER_READ = 0xFFFFFFFF              # LIME_NORM_PER_READ: the norm of the sample calls that normalises every read by its own length
VERDICT = np.dtype([("taxon", "<u4"), ("sim", "<f4"), ("type", "u1"), ("rule", "u1"), ("pad", "u1", (2,))])


class _LibBuf:
    """a host buffer returned by the library (uint32 words), exposed through the array interface and freed with the last array on it"""
    def __init__(self, lib, ptr, words):
        self._lib, self._ptr = lib, ptr
        self.__array_interface__ = {"data": (ptr, False), "shape": (words,), "typestr": "<u4", "version": 3}

    def __del__(self):
        try:
            self._lib.lime_free(C.c_void_p(self._ptr))
        except Exception:        # interpreter shutdown: the library handle may be gone before the last array
            pass


class Context:
    """One lime_ctx (one device).  `device=None` keeps the current HIP device."""

    def __init__(self, device=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.lime_init(-1 if device is None else int(device), C.byref(h)))
        self.h = h
        self._lists = []                     # Lists and GenomeIndex objects of this ctx still alive: lime_shutdown frees them

    def set_option(self, key, value=""):
        """a tuning / test knob of the ctx by name (lime_set_option; include/lime_hip.h lists them); "" = the library's own choice"""
        check(self.lib.lime_set_option(self.h, str(key).encode(), str(value).encode()))

    def close(self):
        if self.h:
            for ref in self._lists:
                li = ref()
                if li is not None:
                    li.h = None              # (freed by lime_shutdown)
            self._lists = []
            self.lib.lime_shutdown(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- array level, host pointers ------------------------------------------------------
    def detect(self, lcp, da, n_reads, alpha):
        """ClusterLCP scan -> (clusters u64[nC,2] ascending pStart, n_clusters, max_len)."""
        lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
        da = np.ascontiguousarray(da, dtype=np.uint32)
        if len(lcp) != len(da):
            raise ValueError("lcp and da differ in length")
        out = C.c_void_p()
        nc, ml = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.lime_detect(self.h, lcp.ctypes.data, da.ctypes.data, len(lcp), n_reads, alpha,
                                   C.byref(out), C.byref(nc), C.byref(ml)))
        if nc.value:
            arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(nc.value, 2)).copy()
            self.lib.lime_free(out)
        else:
            arr = np.zeros((0, 2), dtype=np.uint64)
        return arr, int(nc.value), int(ml.value)

    def score(self, da, ebwt, clusters, n_reads, n_refs):
        """clusterAnalyze -> sim u8[n_reads, n_refs]; ebwt=None is the EBWT=0 build."""
        da = np.ascontiguousarray(da, dtype=np.uint32)
        cl = np.ascontiguousarray(clusters, dtype=np.uint64).reshape(-1, 2)
        eb = None if ebwt is None else np.ascontiguousarray(ebwt, dtype=np.uint8)
        sim = np.zeros((n_reads, n_refs), dtype=np.uint8)
        check(self.lib.lime_score(self.h, da.ctypes.data, None if eb is None else eb.ctypes.data, len(da),
                                  cl.ctypes.data if len(cl) else None, len(cl), n_reads, n_refs, sim.ctypes.data))
        return sim

    def fused(self, lcp, da, ebwt, n_reads, n_refs, alpha):
        """detect + score in one pass -> (sim, n_clusters, max_len)."""
        lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
        da = np.ascontiguousarray(da, dtype=np.uint32)
        eb = None if ebwt is None else np.ascontiguousarray(ebwt, dtype=np.uint8)
        sim = np.zeros((n_reads, n_refs), dtype=np.uint8)
        nc, ml = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.lime_fused(self.h, lcp.ctypes.data, da.ctypes.data, None if eb is None else eb.ctypes.data,
                                  len(lcp), n_reads, n_refs, alpha, sim.ctypes.data, C.byref(nc), C.byref(ml)))
        return sim, int(nc.value), int(ml.value)

    def fused_stream(self, lcp, da, ebwt, n_reads, n_refs, alpha, chunk=0):
        """lime_fused through HBM in position-range chunks (copy of chunk k+1 under the scan of chunk k)."""
        lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
        da = np.ascontiguousarray(da, dtype=np.uint32)
        eb = None if ebwt is None else np.ascontiguousarray(ebwt, dtype=np.uint8)
        sim = np.zeros((n_reads, n_refs), dtype=np.uint8)
        nc, ml = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.lime_fused_stream(self.h, lcp.ctypes.data, da.ctypes.data, None if eb is None else eb.ctypes.data,
                                         len(lcp), n_reads, n_refs, alpha, chunk, sim.ctypes.data, C.byref(nc), C.byref(ml)))
        return sim, int(nc.value), int(ml.value)

    def choose(self, sim):
        sim = np.ascontiguousarray(sim, dtype=np.uint8)
        nr, ng = sim.shape
        mx = np.zeros(nr, dtype=np.uint8)
        nz = np.zeros(nr, dtype=np.uint32)
        check(self.lib.lime_choose(self.h, sim.ctypes.data, nr, ng, mx.ctypes.data, nz.ctypes.data))
        return mx, nz

    def _pairs_out(self, pp, npairs):
        """the library's pair list as an array WITHOUT a copy (0.7 GB when most of configs[2]'s rows pass: zeroing + copying it cost more than the
        device side of the call); the buffer goes back to lime_free when the last view of it dies"""
        n = int(npairs.value)
        if not n or not pp.value:
            if pp.value:
                self.lib.lime_free(pp)
            return np.zeros((0, 2), dtype=np.uint32)
        return np.asarray(_LibBuf(self.lib, pp.value, 2 * n)).reshape(n, 2)

    def score_choose(self, da, ebwt, clusters, n_reads, n_refs, norm, beta, want_sim=False):
        """clusterAnalyze + clusterChoose with the table kept in HBM -> (row_max u8[n_reads],
        row_off u64[n_reads+1], pairs u32[n,2] = (idRef, sim)[, sim])."""
        da = np.ascontiguousarray(da, dtype=np.uint32)
        cl = np.ascontiguousarray(clusters, dtype=np.uint64).reshape(-1, 2)
        eb = None if ebwt is None else np.ascontiguousarray(ebwt, dtype=np.uint8)
        mx = np.zeros(n_reads + 1, dtype=np.uint8)
        off = np.zeros(n_reads + 2, dtype=np.uint64)
        sim = np.zeros((n_reads, n_refs), dtype=np.uint8) if want_sim else None
        pp, npairs = C.c_void_p(), C.c_uint64(0)
        check(self.lib.lime_score_choose(self.h, da.ctypes.data, None if eb is None else eb.ctypes.data, len(da),
                                         cl.ctypes.data if len(cl) else None, len(cl), n_reads, n_refs, norm, beta,
                                         mx.ctypes.data, off.ctypes.data, C.byref(pp), C.byref(npairs),
                                         None if sim is None else sim.ctypes.data))
        pairs = self._pairs_out(pp, npairs)
        res = (mx[:n_reads], off[:n_reads + 1], pairs)
        return res + (sim,) if want_sim else res

    def choose_pairs_dev(self, sim_t, n_reads, n_refs, norm, beta, stream=None):
        """clusterChoose of a device-resident table -> (row_max, row_off, pairs) on the host."""
        mx = np.zeros(n_reads + 1, dtype=np.uint8)
        off = np.zeros(n_reads + 2, dtype=np.uint64)
        pp, npairs = C.c_void_p(), C.c_uint64(0)
        check(self.lib.lime_choose_pairs_dev(self.h, _ptr(sim_t), n_reads, n_refs, norm, beta, mx.ctypes.data,
                                             off.ctypes.data, C.byref(pp), C.byref(npairs), stream))
        return mx[:n_reads], off[:n_reads + 1], self._pairs_out(pp, npairs)

    def fused_choose_dev(self, lcp_t, da_t, ebwt_t, n, n_reads, n_refs, alpha, norm, beta, stream=None, out=None):
        """scan + clusterAnalyze + clusterChoose on device-resident arrays, without the table where the binned path serves the pass
        -> (row_max, row_off, pairs, Stats)"""
        if out is None:                                       # out: the caller's (uint8[n_reads + 1], uint64[n_reads + 2]) to fill instead of fresh arrays
            out = (np.zeros(n_reads + 1, dtype=np.uint8), np.zeros(n_reads + 2, dtype=np.uint64))       # (9 MB of fresh pages at 10^6 reads: 0.5 ms)
        mx, off = out
        assert mx.dtype == np.uint8 and off.dtype == np.uint64 and len(mx) >= n_reads + 1 and len(off) >= n_reads + 2
        pp, npairs, s = C.c_void_p(), C.c_uint64(0), Stats()
        check(self.lib.lime_fused_choose_dev(self.h, _ptr(lcp_t), _ptr(da_t), _ptr(ebwt_t), n, n_reads, n_refs, alpha, norm, beta,
                                             mx.ctypes.data, off.ctypes.data, C.byref(pp), C.byref(npairs), C.byref(s), stream))
        return mx[:n_reads], off[:n_reads + 1], self._pairs_out(pp, npairs), s

    # ---- clusterChoose results left in HBM, classified there (include/lime_hip.h: lime_lists) ----
    def _lists_of(self, h):
        import weakref
        li = Lists(self, h)
        self._lists = [r for r in self._lists if r() is not None] + [weakref.ref(li)]
        return li

    def choose_lists_dev(self, sim_t, n_reads, n_refs, norm, beta, stream=None):
        """clusterChoose of a device-resident table, the lists left in HBM -> Lists"""
        h = C.c_void_p()
        check(self.lib.lime_choose_lists_dev(self.h, _ptr(sim_t), n_reads, n_refs, norm, beta, C.byref(h), stream))
        return self._lists_of(h)

    def fused_choose_lists_dev(self, lcp_t, da_t, ebwt_t, n, n_reads, n_refs, alpha, norm, beta, stream=None):
        """scan + clusterAnalyze + clusterChoose on device-resident arrays, the lists left in HBM -> (Lists, Stats)"""
        h, s = C.c_void_p(), Stats()
        check(self.lib.lime_fused_choose_lists_dev(self.h, _ptr(lcp_t), _ptr(da_t), _ptr(ebwt_t), n, n_reads, n_refs, alpha, norm, beta,
                                                   C.byref(h), C.byref(s), stream))
        return self._lists_of(h), s

    def fused_choose_lists(self, lcp, da, ebwt, n_reads, n_refs, alpha, norm, beta):
        """the same from host arrays (or np.memmap'd files; the collection is as long as the shortest of them) -> (Lists, Stats)"""
        lcp = np.ascontiguousarray(lcp, dtype=np.uint32) if not isinstance(lcp, np.memmap) else lcp
        da = np.ascontiguousarray(da, dtype=np.uint32) if not isinstance(da, np.memmap) else da
        n = min(len(lcp), len(da)) if ebwt is None else min(len(lcp), len(da), len(ebwt))     # (a short file: no read past its end)
        h, s = C.c_void_p(), Stats()
        check(self.lib.lime_fused_choose_lists(self.h, lcp.ctypes.data, da.ctypes.data, None if ebwt is None else ebwt.ctypes.data,
                                               n, n_reads, n_refs, alpha, norm, beta, C.byref(h), C.byref(s)))
        return self._lists_of(h), s

    def lists_concat(self, parts, id_base, n_refs_part, beta, stream=None):
        """the Lists of column shards of one table (each made with a negative beta: every non-zero row) made into the whole table's Lists:
        part p holds the genomes id_base[p] .. id_base[p] + n_refs_part[p] - 1, clusterChoose's test is taken on the maximum over the parts
        (lime_lists_concat_dev).  The parts stay the caller's -> Lists"""
        k = len(parts)
        hs = (C.c_void_p * max(k, 1))(*[None if li is None else li.h for li in parts])
        base = np.ascontiguousarray(id_base, dtype=np.uint32)
        cnt = np.ascontiguousarray(n_refs_part, dtype=np.uint32)
        if len(base) != k or len(cnt) != k:
            raise ValueError("lists_concat: one id_base and one n_refs_part per part")
        h = C.c_void_p()
        check(self.lib.lime_lists_concat_dev(self.h, k, hs, base.ctypes.data if k else None, cnt.ctypes.data if k else None, float(beta), C.byref(h), stream))
        return self._lists_of(h)

    def lists_concat_norms(self, parts, id_base, n_refs_part, norms_t, beta, stream=None):
        """lists_concat with clusterChoose's test taken per read: norms_t is a torch uint8 device tensor [n_reads] (docs_norms), read r
        passes where float(max) / norms[r] > beta (lime_lists_concat_norms_dev).  One part with id_base 0 is the plain per-read filter.
        -> Lists that own a copy of the norms (Lists.norms(); info() reports norm 0)"""
        k = len(parts)
        hs = (C.c_void_p * max(k, 1))(*[None if li is None else li.h for li in parts])
        base = np.ascontiguousarray(id_base, dtype=np.uint32)
        cnt = np.ascontiguousarray(n_refs_part, dtype=np.uint32)
        if len(base) != k or len(cnt) != k:
            raise ValueError("lists_concat_norms: one id_base and one n_refs_part per part")
        h = C.c_void_p()
        check(self.lib.lime_lists_concat_norms_dev(self.h, k, hs, base.ctypes.data if k else None, cnt.ctypes.data if k else None,
                                                   None if norms_t is None else _ptr(norms_t), float(beta), C.byref(h), stream))
        return self._lists_of(h)

    def docs_norms(self, docs, alpha, stream=None, out=None):
        """a norm per read from the documents' own lengths: len + 1 - alpha, 1 for a read shorter than alpha (lime_docs_norms_dev; a read of
        more than 255 symbols: LimeError with its index and length) -> torch uint8 device tensor [n_docs] (out: a tensor or view to fill)"""
        import torch
        n = docs.info()[0]
        t = out if out is not None else torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")      # (torch's current device: the ctx's, as for the other *_dev calls' tensors)
        check(self.lib.lime_docs_norms_dev(self.h, docs.h, int(alpha), _ptr(t), stream))
        return t[:n]

    def concat_info(self):
        """the last lists_concat of this context (lime_get_concat_info); the ms need set_timing(True)"""
        v = (C.c_double * 4)()
        check(self.lib.lime_get_concat_info(self.h, v))
        return {"rows_ms": v[0], "scan_ms": v[1], "copy_ms": v[2], "pairs": int(v[3])}

    def classify_lists_dev(self, lists, n_targ, taxonomy, binary=True, stream=None):
        """Classify over 2 or 4 Lists of this ctx -> (verdicts: numpy VERDICT[n_reads], counts {C, U, A, H} as a list)"""
        hs = (C.c_void_p * len(lists))(*[li.h for li in lists])
        n_reads = lists[0].info()[0] if lists and lists[0].h else 0
        v = np.zeros(max(n_reads, 1), dtype=VERDICT)
        counts = (C.c_uint64 * 4)()
        check(self.lib.lime_classify_lists_dev(self.h, len(lists), hs, n_targ, taxonomy.h, int(bool(binary)), v.ctypes.data, counts, stream))
        return v[:n_reads], list(counts)

    # ---- array level, device pointers (torch tensors on this ctx's device) ---------------
    def stats(self, stream=None):
        s = Stats()
        rc = self.lib.lime_get_stats(self.h, C.byref(s), stream)
        return s, rc

    def synth_dev(self, seed, i0, count, n_reads, n_refs, alpha, mode, lcp_t, da_t, ebwt_t, stream=None):
        check(self.lib.lime_synth_dev(self.h, seed, i0, count, n_reads, n_refs, alpha, mode,
                                      _ptr(lcp_t), _ptr(da_t), _ptr(ebwt_t), stream))

    def fused_dev(self, lcp_t, da_t, ebwt_t, n_own, n_avail, eof, n_reads, n_refs, alpha, sim_t,
                  zero_sim=True, stream=None):
        check(self.lib.lime_fused_dev(self.h, _ptr(lcp_t), _ptr(da_t), _ptr(ebwt_t), n_own, n_avail, int(eof),
                                      n_reads, n_refs, alpha, _ptr(sim_t), int(zero_sim), stream))

    # ---- owner-partitioned exchange of table updates (include/lime_hip.h) ----
    def records_layout(self, n_reads, n_refs):
        nb, sh = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.lime_records_layout(self.h, n_reads, n_refs, C.byref(nb), C.byref(sh)))
        return int(nb.value), int(sh.value)

    def fused_records_dev(self, lcp_t, da_t, ebwt_t, n_own, n_avail, eof, n_reads, n_refs, alpha, stream=None):
        self._rec_shape = self.records_layout(n_reads, n_refs)
        check(self.lib.lime_fused_records_dev(self.h, _ptr(lcp_t), _ptr(da_t), _ptr(ebwt_t), n_own, n_avail, int(eof),
                                              n_reads, n_refs, alpha, stream))

    def records_get(self, stream=None):
        """-> (Records with device pointers valid until the next pass, numpy bin bases [n_bins + 1])"""
        import numpy as np
        from ._lib import Records
        nb, _ = self._rec_shape
        r = Records()
        base = np.zeros(nb + 1, dtype=np.uint64)
        check(self.lib.lime_records_get(self.h, C.byref(r), base.ctypes.data, stream))
        return r, base

    def apply_records_dev(self, n_src, rx_t, srcoff, nb, bin_shift, bigrecs_t, n_big, cell_lo, block_bytes, block_t, stream=None):
        import numpy as np
        so = np.ascontiguousarray(srcoff, dtype=np.uint64)
        check(self.lib.lime_apply_records_dev(self.h, n_src, _ptr(rx_t), so.ctypes.data, nb, bin_shift, _ptr(bigrecs_t), n_big,
                                              cell_lo, block_bytes, _ptr(block_t), stream))

    def partition_records(self, n_prod, prod_waves, n_sub, cap_w, pool, wave_cnt, n_bins, bin_shift, out_t, out_words=None, stream=None):
        """test hook (lime_partition_records_dev): the first-level partition alone on a host pool of n_prod * prod_waves * n_sub segments of
        cap_w words with wave_cnt records each, into the torch device tensor out_t (int32 / uint32 words)
        -> (numpy bin bases [n_bins + 1], 1 if k_part_lines ran else 0).  Waits for the stream."""
        import numpy as np
        pool = np.ascontiguousarray(pool, dtype=np.uint32)
        wc = np.ascontiguousarray(wave_cnt, dtype=np.uint32)
        base = np.zeros(n_bins + 1, dtype=np.uint64)
        kernel = C.c_int(-1)
        check(self.lib.lime_partition_records_dev(self.h, n_prod, prod_waves, n_sub, cap_w, pool.ctypes.data, wc.ctypes.data, n_bins, bin_shift,
                                                  _ptr(out_t), out_t.numel() if out_words is None else out_words, base.ctypes.data,
                                                  C.byref(kernel), stream))
        return base, int(kernel.value)

    def detect_dev(self, lcp_t, da_t, n_own, n_avail, eof, pos_base, n_reads, alpha, stream=None):
        """-> (device pointer of the library-owned record list, n_clusters, max_len); the list stays valid
        until the next detect_dev on this context."""
        dc, nc, ml = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        check(self.lib.lime_detect_dev(self.h, _ptr(lcp_t), _ptr(da_t), n_own, n_avail, int(eof), pos_base, n_reads,
                                       alpha, C.byref(dc), C.byref(nc), C.byref(ml), stream))
        return dc.value, int(nc.value), int(ml.value)

    def score_dev(self, da_t, ebwt_t, n, clusters_ptr, n_clusters, n_reads, n_refs, sim_t, zero_sim=True, stream=None):
        """clusters_ptr: device address of n_clusters lime_cluster_t records (e.g. from detect_dev)"""
        check(self.lib.lime_score_dev(self.h, _ptr(da_t), _ptr(ebwt_t), n, C.c_void_p(clusters_ptr), n_clusters, n_reads,
                                      n_refs, _ptr(sim_t), int(zero_sim), stream))

    def choose_dev(self, sim_t, n_reads, n_refs, max_t, nnz_t, stream=None):
        check(self.lib.lime_choose_dev(self.h, _ptr(sim_t), n_reads, n_refs, _ptr(max_t), _ptr(nnz_t), stream))

    def set_timing(self, on):
        check(self.lib.lime_set_timing(self.h, int(on)))

    def get_timing(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        check(self.lib.lime_get_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def get_timing_ex(self):
        """-> ({scan, pass, after_scan, before_scan} average ms per lime_fused_dev pass, passes timed)"""
        ms, n = (C.c_double * 4)(), C.c_uint64(0)
        check(self.lib.lime_get_timing_ex(self.h, ms, C.byref(n)))
        return {"scan": ms[0], "pass": ms[1], "after_scan": ms[2], "before_scan": ms[3]}, int(n.value)


    def host_times(self):
        """what the passes on this context cost on the host so far (lime_get_host_times)"""
        v = (C.c_double * 8)()
        check(self.lib.lime_get_host_times(self.h, v))
        return {"alloc_ms": v[0], "probe_ms": v[1], "probes": int(v[2]), "repeats": int(v[3]), "cas_fallbacks": int(v[4]),
                "records_per_symbol": None if v[5] < 0 else v[5], "choose_without_table": int(v[6]), "classify_kernel_ms": v[7]}

    # ---- ebwt / lcp / da from the sequences (include/lime_hip.h: lime_build_index) ----
    def build_index(self, reads, genomes, term=0, lcp_cap=0):
        """the collection reads + genomes -> (ebwt u8[N], lcp u32[N], da u32[N]) numpy arrays: lime_amd.builder.build_arrays' contract, sorted
        on the device; lcp_cap > 0 stores min(lcp, lcp_cap)"""
        text, off = pack_documents(reads, genomes)
        n = int(off[-1]) + len(off) - 1
        ebwt, lcp, da = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        check(self.lib.lime_build_index(self.h, text.ctypes.data, off.ctypes.data, len(off) - 1, int(term), int(lcp_cap),
                                        ebwt.ctypes.data, lcp.ctypes.data, da.ctypes.data))
        return ebwt[:n], lcp[:n], da[:n]

    def build_index_dev(self, text_t, doc_off_t, n_docs, n_text, term=0, lcp_cap=0, stream=None, out=None):
        """the same on torch device tensors: text_t uint8[n_text] (no terminators), doc_off_t int64[n_docs + 1] -> (ebwt_t uint8[N],
        lcp_t, da_t int32[N] holding the u32 values), fresh tensors unless `out` gives the three (any of them None: not computed)"""
        import torch
        n = int(n_text) + int(n_docs)
        if out is None:
            dev = text_t.device
            out = (torch.empty(max(n, 1), dtype=torch.uint8, device=dev), torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                   torch.empty(max(n, 1), dtype=torch.int32, device=dev))
        ebwt_t, lcp_t, da_t = out
        check(self.lib.lime_build_index_dev(self.h, _ptr(text_t), _ptr(doc_off_t), int(n_docs), int(n_text), int(term), int(lcp_cap),
                                            _ptr(ebwt_t), _ptr(lcp_t), _ptr(da_t), stream))
        return tuple(None if t is None else t[:n] for t in out)

    def index_info(self):
        """the last build_index* of this context (lime_get_index_info); the ms need set_timing(True)"""
        v = (C.c_double * 8)()
        check(self.lib.lime_get_index_info(self.h, v))
        return {"rounds": int(v[0]), "unresolved": [int(v[1]), int(v[2]), int(v[3]), int(v[4])], "sort_ms": v[5], "doubling_ms": v[6], "lcp_ms": v[7]}


    # ---- reads merged into a prebuilt genome index (include/lime_hip.h: lime_gindex, lime_merge_index) ----
    def _gindex_of(self, h):
        import weakref
        gi = GenomeIndex(self, h)
        self._lists = [r for r in self._lists if r() is not None] + [weakref.ref(gi)]
        return gi

    def build_genome_index(self, genomes, term=0, lcp_cap=0):
        """the genomes alone, sorted once and left in HBM -> GenomeIndex"""
        text, off = pack_documents([], genomes)
        h = C.c_void_p()
        check(self.lib.lime_gindex_build(self.h, text.ctypes.data, off.ctypes.data, len(off) - 1, int(term), int(lcp_cap), C.byref(h)))
        return self._gindex_of(h)

    def build_genome_index_dev(self, text_t, doc_off_t, n_docs, n_text, term=0, lcp_cap=0, stream=None):
        """the same from torch device tensors (build_index_dev's arguments)"""
        h = C.c_void_p()
        check(self.lib.lime_gindex_build_dev(self.h, _ptr(text_t), _ptr(doc_off_t), int(n_docs), int(n_text), int(term), int(lcp_cap), stream, C.byref(h)))
        return self._gindex_of(h)

    def load_genome_index(self, path):
        """a file written by GenomeIndex.save (or BuildIndex --refs) -> GenomeIndex"""
        h = C.c_void_p()
        check(self.lib.lime_gindex_load(self.h, os.fsencode(path), C.byref(h)))
        return self._gindex_of(h)

    def merge_index(self, reads, gi, lcp_cap=0):
        """build_index(reads, the index's genomes, the index's term, lcp_cap) without sorting the genomes again -> (ebwt, lcp, da)"""
        text, off = pack_documents(reads, [])
        n = int(self.lib.lime_merge_size(gi.h, off.ctypes.data, len(off) - 1))
        ebwt, lcp, da = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        check(self.lib.lime_merge_index(self.h, text.ctypes.data, off.ctypes.data, len(off) - 1, gi.h, int(lcp_cap),
                                        ebwt.ctypes.data, lcp.ctypes.data, da.ctypes.data))
        return ebwt[:n], lcp[:n], da[:n]

    def merge_index_dev(self, text_t, doc_off_t, n_reads, n_text, gi, lcp_cap=0, stream=None, out=None):
        """the same on torch device tensors: the reads' text_t uint8[n_text] and doc_off_t int64[n_reads + 1] -> (ebwt_t uint8[N], lcp_t,
        da_t int32[N] holding the u32 values), N = read positions + the index's; fresh tensors unless `out` gives the three (any None: not computed)"""
        import torch
        n = int(n_text) + int(n_reads) + gi.info()["positions"]
        if out is None:
            dev = doc_off_t.device
            out = (torch.empty(max(n, 1), dtype=torch.uint8, device=dev), torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                   torch.empty(max(n, 1), dtype=torch.int32, device=dev))
        ebwt_t, lcp_t, da_t = out
        check(self.lib.lime_merge_index_dev(self.h, _ptr(text_t), _ptr(doc_off_t), int(n_reads), int(n_text), gi.h, int(lcp_cap),
                                            _ptr(ebwt_t), _ptr(lcp_t), _ptr(da_t), stream))
        return tuple(None if t is None else t[:n] for t in out)

    def merge_info(self):
        """the last merge_index* of this context (lime_get_merge_info); the ms need set_timing(True)"""
        v = (C.c_double * 8)()
        check(self.lib.lime_get_merge_info(self.h, v))
        return {"reads_rounds": int(v[0]), "read_suffixes": int(v[1]), "read_runs": int(v[2]), "reads_build_ms": v[3], "rank_ms": v[4], "place_ms": v[5]}

    # ---- FASTA to documents on the device, a sample from documents to verdicts (include/lime_hip.h: lime_docs) ----
    def _docs_of(self, h):
        import weakref
        d = Docs(self, h)
        self._lists = [r for r in self._lists if r() is not None] + [weakref.ref(d)]
        return d

    def docs_from_fasta(self, path):
        """a FASTA file, parsed on the device -> Docs (fasta_read(path)'s records, left in HBM)"""
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fasta(self.h, os.fsencode(path), C.byref(h)))
        return self._docs_of(h)

    def docs_from_bytes(self, data):
        """the bytes of a FASTA file (bytes or a uint8 array) -> Docs"""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        h = C.c_void_p()
        check(self.lib.lime_docs_from_bytes(self.h, a.ctypes.data if len(a) else None, len(a), C.byref(h)))
        return self._docs_of(h)

    def docs_from_bytes_dev(self, bytes_t, n=None, stream=None):
        """the same from a torch uint8 device tensor (a view at any alignment); n: its first n bytes, even beyond 2^32 (refused, nothing is read)"""
        n = int(bytes_t.numel()) if n is None else int(n)
        h = C.c_void_p()
        check(self.lib.lime_docs_from_bytes_dev(self.h, _ptr(bytes_t), n, stream, C.byref(h)))
        return self._docs_of(h)

    def docs_from_fastq(self, path):
        """a four-line FASTQ file, parsed on the device -> Docs (fastq_read(path)'s records; its refusals as LimeError with the line and reason)"""
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fastq(self.h, os.fsencode(path), C.byref(h)))
        return self._docs_of(h)

    def docs_from_fastq_bytes(self, data):
        """the bytes of a FASTQ file (bytes or a uint8 array) -> Docs"""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fastq_bytes(self.h, a.ctypes.data if len(a) else None, len(a), C.byref(h)))
        return self._docs_of(h)

    def docs_from_fastq_bytes_dev(self, bytes_t, n=None, stream=None):
        """the same from a torch uint8 device tensor (a view at any alignment); n as for docs_from_bytes_dev"""
        n = int(bytes_t.numel()) if n is None else int(n)
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fastq_bytes_dev(self.h, _ptr(bytes_t), n, stream, C.byref(h)))
        return self._docs_of(h)

    def docs_from_fastq_qual(self, path):
        """docs_from_fastq, keeping the quality strings next to the reads (Docs.qual) -> Docs"""
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fastq_qual(self.h, os.fsencode(path), C.byref(h)))
        return self._docs_of(h)

    def docs_from_fastq_qual_bytes(self, data):
        """the same from the bytes of a FASTQ file (bytes or a uint8 array)"""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fastq_qual_bytes(self.h, a.ctypes.data if len(a) else None, len(a), C.byref(h)))
        return self._docs_of(h)

    def docs_from_fastq_qual_bytes_dev(self, bytes_t, n=None, stream=None):
        """the same from a torch uint8 device tensor (a view at any alignment); n as for docs_from_bytes_dev"""
        n = int(bytes_t.numel()) if n is None else int(n)
        h = C.c_void_p()
        check(self.lib.lime_docs_from_fastq_qual_bytes_dev(self.h, _ptr(bytes_t), n, stream, C.byref(h)))
        return self._docs_of(h)

    def docs_trim(self, docs, q5, q3, stream=None):
        """Docs with qualities cut at both ends by the quality rule (lime_docs_trim_dev; a cutoff of 0 leaves that end alone)
        -> (Docs without qualities, info: dict of n_reads, n_changed, n_empty, symbols_in, symbols_out)"""
        h, ti = C.c_void_p(), _lib.TrimInfo()
        check(self.lib.lime_docs_trim_dev(self.h, docs.h, int(q5), int(q3), stream, C.byref(h), C.byref(ti)))
        return self._docs_of(h), _trim_info(ti)

    def docs_trim_adapter(self, docs, adapter, min_overlap=3, max_err_pct=10, stream=None):
        """any Docs cut where the 3' adapter (str or bytes, 1 .. 64 of ACGT) begins in each read (lime_docs_trim_adapter_dev; the rule is at
        lime_adapter_trim in include/lime_hip.h) -> (Docs without qualities, info: dict as docs_trim gives)"""
        a = _adapter_bytes(adapter)
        h, ti = C.c_void_p(), _lib.TrimInfo()
        check(self.lib.lime_docs_trim_adapter_dev(self.h, docs.h, a, len(a), int(min_overlap), int(max_err_pct), stream, C.byref(h), C.byref(ti)))
        return self._docs_of(h), _trim_info(ti)

    def docs_filter(self, docs, polyx=None, polyx_min=10, max_len=0, min_len=0, max_n=None, min_complexity=0, stream=None):
        """any Docs through the read filter (lime_docs_filter_dev; the rule is at lime_read_filter in include/lime_hip.h): polyx, the bases whose
        tails are cut ("G", "GA", or the mask), of polyx_min symbols or more; max_len, the cap; then reads shorter than min_len, with more than
        max_n N's (None: no limit) or below min_complexity percent are emptied -> (Docs without qualities, info: dict of n_reads, n_polyx,
        n_capped, n_short, n_many_n, n_low_complexity, symbols_in, symbols_out)"""
        f = _filter_of(polyx, polyx_min, max_len, min_len, max_n, min_complexity)
        h, fi = C.c_void_p(), _lib.FilterInfo()
        check(self.lib.lime_docs_filter_dev(self.h, docs.h, C.byref(f), stream, C.byref(h), C.byref(fi)))
        return self._docs_of(h), _filter_info(fi)

    def docs_qc(self, docs, n_pos=256, tables=None, stream=None):
        """the per-position statistics of any Docs (lime_docs_qc_dev; the rule is at lime_read_qc in include/lime_hip.h): tables, the flat
        uint64 array of qc_words(n_pos) words that the counts are ADDED to (None: fresh zeros) -> the tables split as read_qc gives them"""
        t = _qc_tables(n_pos, tables)
        check(self.lib.lime_docs_qc_dev(self.h, docs.h, int(n_pos), stream, t.ctypes.data))
        return qc_split(t, n_pos)

    def docs_trim_overlap(self, d1, d2, min_overlap=30, max_err_pct=10, want_insert=False, stream=None):
        """the two mates' Docs cut at the mates' overlap: adapter read-through found with no adapter given (lime_docs_trim_overlap_dev; the rule
        is at lime_pair_overlap_trim in include/lime_hip.h).  It is the last stage: give it what each mate's trims and filter left
        -> (Docs, Docs, info: dict of n_pairs, n_overlap, n_cut, symbols_in, symbols_out), and with want_insert also insert: numpy uint32 per
        pair, I* or 0"""
        h1, h2, oi = C.c_void_p(), C.c_void_p(), _lib.OverlapInfo()
        ins = None
        if want_insert:
            import torch
            n = d1.info()[0]
            ins = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")      # (torch's current device: the ctx's, as for docs_norms)
        check(self.lib.lime_docs_trim_overlap_dev(self.h, d1.h, d2.h, int(min_overlap), int(max_err_pct), _ptr(ins), stream, C.byref(h1), C.byref(h2),
                                                  C.byref(oi)))
        out = (self._docs_of(h1), self._docs_of(h2), _overlap_info(oi))
        if want_insert:
            out += (ins[:n].cpu().numpy().view(np.uint32),)
        return out

    def docs_from_file(self, path):
        """a FASTA or FASTQ file, by seq_format(path) -> Docs"""
        h = C.c_void_p()
        check(self.lib.lime_docs_from_file(self.h, os.fsencode(path), C.byref(h)))
        return self._docs_of(h)

    def docs_from_arrays_dev(self, text_t, doc_off_t, n_docs, n_text, stream=None):
        """documents that are parsed already: text_t uint8[n_text], doc_off_t int64[n_docs + 1] on the device (copied) -> Docs"""
        h = C.c_void_p()
        check(self.lib.lime_docs_from_arrays_dev(self.h, _ptr(text_t), _ptr(doc_off_t), int(n_docs), int(n_text), stream, C.byref(h)))
        return self._docs_of(h)

    def classify_sample(self, mates, gi, taxonomy, alpha, norm, beta, ebwt=True, binary=True, lcp_cap=0, stream=None):
        """one sample from its read sets (1 or 2 Docs) and a GenomeIndex to verdicts, everything in HBM (lime_classify_sample_dev)
        -> (verdicts: numpy VERDICT[n_reads], counts {C, U, A, H} as a list, stats: one Stats per collection F, F_RC[, R, R_RC])"""
        k = len(mates)
        hs = (C.c_void_p * max(k, 1))(*[m.h for m in mates])
        n_reads = mates[0].info()[0] if k and mates[0].h else 0
        v = np.zeros(max(n_reads, 1), dtype=VERDICT)
        counts = (C.c_uint64 * 4)()
        st = (Stats * 4)()
        check(self.lib.lime_classify_sample_dev(self.h, k, hs, gi.h, taxonomy.h, int(alpha), int(norm) & 0xFFFFFFFF, float(beta), int(bool(ebwt)),
                                                int(bool(binary)), int(lcp_cap), v.ctypes.data, counts, st, stream))
        return v[:n_reads], list(counts), [st[i] for i in range(2 * k)]

    def classify_sample_shards(self, mates, shards, taxonomy, alpha, norm, beta, ebwt=True, binary=True, lcp_cap=0, stream=None):
        """classify_sample against a genome database cut into GenomeIndex shards, in genome order (lime_classify_sample_shards_dev)
        -> (verdicts, counts, stats: one Stats per shard and collection, shard-major: stats[s * 2 * len(mates) + k])"""
        k, ns = len(mates), len(shards)
        hs = (C.c_void_p * max(k, 1))(*[m.h for m in mates])
        gs = (C.c_void_p * max(ns, 1))(*[None if g is None else g.h for g in shards])
        n_reads = mates[0].info()[0] if k and mates[0].h else 0
        v = np.zeros(max(n_reads, 1), dtype=VERDICT)
        counts = (C.c_uint64 * 4)()
        st = (Stats * (4 * max(ns, 1)))()
        check(self.lib.lime_classify_sample_shards_dev(self.h, k, hs, ns, gs, taxonomy.h, int(alpha), int(norm) & 0xFFFFFFFF, float(beta), int(bool(ebwt)),
                                                       int(bool(binary)), int(lcp_cap), v.ctypes.data, counts, st, stream))
        return v[:n_reads], list(counts), [st[i] for i in range(ns * 2 * k)]

    # ---- a reads file in batches of records, a sample of any size batch by batch (include/lime_hip.h: lime_seq_reader) ----
    def seq_cut_dev(self, bytes_t, fmt, max_reads, eof, n=None, stream=None):
        """where a window of a reads file (a torch uint8 device tensor, a view at any alignment) is cut so that whole records stand in front
        (lime_seq_cut_dev); fmt "fasta" / "fastq" or 0 / 1 -> (cut, n_records, n_markers)"""
        n = int(bytes_t.numel()) if n is None else int(n)
        cut, m, t = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(self.lib.lime_seq_cut_dev(self.h, _ptr(bytes_t), n, _format_of(fmt), int(max_reads), int(bool(eof)), stream,
                                        C.byref(cut), C.byref(m), C.byref(t)))
        return int(cut.value), int(m.value), int(t.value)

    def _reader_of(self, h, keep=None):
        import weakref
        r = SeqReader(self, h, keep)
        self._lists = [x for x in self._lists if x() is not None] + [weakref.ref(r)]
        return r

    def seq_reader(self, path, window_bytes=0):
        """a FASTA or FASTQ file (by seq_format(path)) handed out in batches of records -> SeqReader"""
        h = C.c_void_p()
        check(self.lib.lime_seq_reader_open(self.h, os.fsencode(path), int(window_bytes), C.byref(h)))
        return self._reader_of(h)

    def seq_reader_bytes(self, data, fmt, window_bytes=0):
        """the same over the bytes of such a file (bytes or a uint8 array, kept alive by the reader)"""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        h = C.c_void_p()
        check(self.lib.lime_seq_reader_open_bytes(self.h, a.ctypes.data if len(a) else None, len(a), _format_of(fmt), int(window_bytes), C.byref(h)))
        return self._reader_of(h, a)

    def classify_sample_stream(self, readers, gi, taxonomy, alpha, norm, beta, batch_reads, ebwt=True, binary=True, lcp_cap=0, sink=None, stream=None):
        """classify_sample batch by batch over 1 or 2 SeqReaders (lime_classify_sample_stream).  gi: a GenomeIndex, or a list of them: the
        shards of one genome database in genome order (lime_classify_sample_stream_shards; the Stats are then per shard and collection,
        shard-major).  sink(first_read, verdicts, stats) is called
        per batch with a VERDICT array that is only valid during the call and the batch's Stats; a non-zero return ends the call (LimeError
        with that code).  Without a sink -> (verdicts of all reads, counts {C, U, A, H}, [per-batch list of Stats]); with one ->
        (n_reads, counts, n_batches)"""
        k = len(readers)
        hs = (C.c_void_p * max(k, 1))(*[r.h for r in readers])
        parts, per_batch, raised = [], [], []
        shards = list(gi) if isinstance(gi, (list, tuple)) else None
        n_stats = 2 * k * (len(shards) if shards is not None else 1)

        def cb(_user, first_read, pv, n, pst):
            try:
                v = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_uint8)), shape=(n * VERDICT.itemsize,)).view(VERDICT)
                st = [Stats.from_buffer_copy(pst[i]) for i in range(n_stats)]
                if sink is None:
                    parts.append(v.copy()); per_batch.append(st)
                    return 0
                return int(sink(int(first_read), v, st) or 0)
            except BaseException as e:               # (an exception cannot cross the C frames: it is raised again below)
                raised.append(e)
                return _lib.ERR_ARG
        fn = _lib.VERDICT_SINK(cb)
        counts = (C.c_uint64 * 4)()
        n_reads, n_batches = C.c_uint64(0), C.c_uint64(0)
        if shards is not None:
            gs = (C.c_void_p * max(len(shards), 1))(*[None if g is None else g.h for g in shards])
            rc = self.lib.lime_classify_sample_stream_shards(self.h, k, hs, len(shards), gs, taxonomy.h, int(alpha), int(norm) & 0xFFFFFFFF, float(beta),
                                                             int(bool(ebwt)), int(bool(binary)), int(lcp_cap), int(batch_reads), C.cast(fn, C.c_void_p), None, counts,
                                                             C.byref(n_reads), C.byref(n_batches), stream)
        else:
            rc = self.lib.lime_classify_sample_stream(self.h, k, hs, gi.h, taxonomy.h, int(alpha), int(norm) & 0xFFFFFFFF, float(beta), int(bool(ebwt)),
                                                      int(bool(binary)), int(lcp_cap), int(batch_reads), C.cast(fn, C.c_void_p), None, counts, C.byref(n_reads), C.byref(n_batches),
                                                      stream)
        if raised:
            raise raised[0]
        if rc > 0:
            raise LimeError(rc, "the sink ended the call")
        check(rc)
        if sink is None:
            return (np.concatenate(parts) if parts else np.zeros(0, dtype=VERDICT)), list(counts), per_batch
        return int(n_reads.value), list(counts), int(n_batches.value)


def _trim_info(ti):
    return {k: int(getattr(ti, k)) for k, _ in _lib.TrimInfo._fields_}


def _overlap_info(oi):
    return {k: int(getattr(oi, k)) for k, _ in _lib.OverlapInfo._fields_}


def _overlap_arg(trim_overlap):
    """O, "O", "O,E" or (O, E) -> (O, E), as `--trim-overlap` reads them (E defaults to 10)"""
    if isinstance(trim_overlap, bytes):
        trim_overlap = trim_overlap.decode("latin-1")
    if isinstance(trim_overlap, str):
        trim_overlap = [int(x) for x in trim_overlap.split(",")]
    v = [int(trim_overlap)] if isinstance(trim_overlap, (int, np.integer)) else [int(x) for x in trim_overlap]
    if len(v) not in (1, 2) or v[0] < 1 or not 0 <= (v[1] if len(v) == 2 else 10) <= 50:
        raise ValueError("trim_overlap is O or (O, E): O 1 or more, E 0 .. 50")
    return v[0], (v[1] if len(v) == 2 else 10)


def _filter_info(fi):
    return {k: int(getattr(fi, k)) for k, _ in _lib.FilterInfo._fields_}


def polyx_mask(polyx):
    """None, "", "G", "GA", b"ga" or the mask itself -> lime_filter_t.polyx_mask: bit 0 is A, bit 1 C, bit 2 G, bit 3 T"""
    if polyx is None:
        return 0
    if isinstance(polyx, (int, np.integer)):
        return int(polyx)
    mask = 0
    for ch in (polyx.decode("latin-1") if isinstance(polyx, (bytes, bytearray)) else polyx).upper():
        if ch not in "ACGT":
            raise ValueError("the poly-X bases are of A, C, G and T")
        mask |= 1 << "ACGT".index(ch)
    return mask


def _filter_of(polyx, polyx_min, max_len, min_len, max_n, min_complexity):
    vals = (polyx_mask(polyx), int(polyx_min), int(max_len), int(min_len), _lib.FILTER_OFF if max_n is None else int(max_n), int(min_complexity))
    if any(not 0 <= v <= 0xFFFFFFFF for v in vals):
        raise ValueError("the filter's parameters are unsigned 32-bit numbers")
    return _lib.Filter(*vals)


def _adapter_bytes(adapter):
    return adapter.encode("latin-1") if isinstance(adapter, str) else bytes(adapter)


def _adapters(trim_adapter, n_reads):
    """SEQ, "SEQ,SEQ2" or (SEQ, SEQ2) -> one adapter per reads file, as `--trim-adapter` reads them"""
    ad = trim_adapter.split(",") if isinstance(trim_adapter, str) else ([trim_adapter] if isinstance(trim_adapter, bytes) else list(trim_adapter))
    ad = [_adapter_bytes(x) for x in ad]
    if len(ad) not in (1, 2) or any(not 1 <= len(x) <= 64 or any(chr(b & 0xDF) not in "ACGT" for b in x) for x in ad):
        raise ValueError("trim_adapter is SEQ or (SEQ, SEQ2), each 1 .. 64 of ACGT")
    if len(ad) == 2 and n_reads != 2:
        raise ValueError("trim_adapter: a second adapter needs a second reads file")
    return ad * 2 if len(ad) == 1 else ad


def _polyx_arg(trim_polyx):
    """None, "G", "GA,12" or (BASES, T) -> (mask, T), as `--trim-polyx` reads them (T defaults to 10)"""
    if trim_polyx is None:
        return 0, 10
    if isinstance(trim_polyx, bytes):
        trim_polyx = trim_polyx.decode("latin-1")
    parts = trim_polyx.split(",") if isinstance(trim_polyx, str) else list(trim_polyx)
    if len(parts) not in (1, 2) or not parts[0]:
        raise ValueError("trim_polyx is BASES or (BASES, T): BASES of A, C, G and T, T 1 .. 255")
    mask, t = polyx_mask(parts[0]), int(parts[1]) if len(parts) == 2 else 10
    if not 1 <= mask <= 15 or not 1 <= t <= 255:
        raise ValueError("trim_polyx is BASES or (BASES, T): BASES of A, C, G and T, T 1 .. 255")
    return mask, t


def _trim_cutoffs(trim_qual):
    """Q, "Q", (Q5, Q3) or "Q5,Q3" -> (q5, q3), as `--trim-qual` reads them"""
    if isinstance(trim_qual, str):
        trim_qual = [int(x) for x in trim_qual.split(",")]
    q = [int(trim_qual)] if isinstance(trim_qual, (int, np.integer)) else [int(x) for x in trim_qual]
    if len(q) not in (1, 2) or any(not 0 <= x <= 93 for x in q):
        raise ValueError("trim_qual is Q or (Q5, Q3), each 0 .. 93")
    return (0, q[0]) if len(q) == 1 else (q[0], q[1])


def _format_of(fmt):
    if fmt in ("fasta", "fastq"):
        return int(fmt == "fastq")
    return int(fmt)


class SeqReader:
    """a reads file handed out in batches of records (lime_seq_reader), owned by its Context; iterating gives Docs of `batch` records"""

    def __init__(self, ctx, h, keep=None, batch=65536):
        self.ctx, self.h, self._keep, self.batch = ctx, h, keep, batch

    def next(self, max_reads):
        """the next max_reads records -> (Docs, number of its first record), or None at the end of the file"""
        d, first = C.c_void_p(), C.c_uint64(0)
        check(self.ctx.lib.lime_seq_reader_next(self.h, int(max_reads), C.byref(d), C.byref(first)))
        if not d:
            return None
        return self.ctx._docs_of(d), int(first.value)

    def __iter__(self):
        while True:
            b = self.next(self.batch)
            if b is None:
                return
            yield b[0]

    def set_trim(self, q5, q3):
        """every batch from here on is parsed with its qualities and handed out trimmed (lime_seq_reader_set_trim: before the first next, FASTQ only)"""
        check(self.ctx.lib.lime_seq_reader_set_trim(self.h, int(q5), int(q3)))

    def set_adapter(self, adapter, min_overlap=3, max_err_pct=10):
        """every batch from here on is handed out cut at its reads' adapters, behind the quality trim where set_trim is set too
        (lime_seq_reader_set_adapter: before the first next; FASTA or FASTQ)"""
        a = _adapter_bytes(adapter)
        check(self.ctx.lib.lime_seq_reader_set_adapter(self.h, a, len(a), int(min_overlap), int(max_err_pct)))

    def adapter_info(self):
        """the adapter trim's counts summed over the batches handed out so far -> dict as Context.docs_trim gives"""
        ti = _lib.TrimInfo()
        check(self.ctx.lib.lime_seq_reader_adapter_info(self.h, C.byref(ti)))
        return _trim_info(ti)

    def set_filter(self, polyx=None, polyx_min=10, max_len=0, min_len=0, max_n=None, min_complexity=0):
        """every batch from here on is handed out filtered, behind the quality trim and the adapter trim where those are set
        (lime_seq_reader_set_filter: before the first next; FASTA or FASTQ; the parameters as Context.docs_filter takes them)"""
        f = _filter_of(polyx, polyx_min, max_len, min_len, max_n, min_complexity)
        check(self.ctx.lib.lime_seq_reader_set_filter(self.h, C.byref(f)))

    def filter_info(self):
        """the filter's counts summed over the batches handed out so far -> dict as Context.docs_filter gives"""
        fi = _lib.FilterInfo()
        check(self.ctx.lib.lime_seq_reader_filter_info(self.h, C.byref(fi)))
        return _filter_info(fi)

    def set_qc(self, n_pos=256):
        """every batch from here on adds to the reader's two sets of statistics with n_pos rows: the batch as parsed and as handed out
        (lime_seq_reader_set_qc: before the first next; FASTA or FASTQ)"""
        check(self.ctx.lib.lime_seq_reader_set_qc(self.h, int(n_pos)))
        self._qc_pos = int(n_pos)

    def qc(self, which):
        """the statistics summed over the batches so far, which = 0 or "raw": as parsed, 1 or "out": as handed out (lime_seq_reader_qc)
        -> the tables split as read_qc gives them; without set_qc zeros with one row"""
        which = {"raw": 0, "out": 1}.get(which, which)
        n_pos = getattr(self, "_qc_pos", 1)
        t = np.zeros(qc_words(n_pos), dtype=np.uint64)
        check(self.ctx.lib.lime_seq_reader_qc(self.h, int(which), t.ctypes.data))
        return qc_split(t, n_pos)

    def set_overlap(self, other, min_overlap=30, max_err_pct=10):
        """links this reader and `other`, the two mates' files, so that next_pair hands out their batches cut at the mates' overlap
        (lime_seq_reader_set_overlap: before the first next of either).  next() on a linked reader alone hands out the UNCUT batch"""
        check(self.ctx.lib.lime_seq_reader_set_overlap(self.h, other.h, int(min_overlap), int(max_err_pct)))

    def next_pair(self, other, max_reads):
        """the next max_reads records of this reader and of `other`, each through its own stages, then cut at the mates' overlap, last
        (lime_seq_reader_next_pair) -> (Docs, Docs, number of the first record), or None at the end of both files"""
        d1, d2, first = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        check(self.ctx.lib.lime_seq_reader_next_pair(self.h, other.h, int(max_reads), C.byref(d1), C.byref(d2), C.byref(first)))
        if not d1:
            return None
        return self.ctx._docs_of(d1), self.ctx._docs_of(d2), int(first.value)

    def overlap_info(self):
        """the overlap cut's counts summed over the batches next_pair handed out so far -> dict as Context.docs_trim_overlap gives"""
        oi = _lib.OverlapInfo()
        check(self.ctx.lib.lime_seq_reader_overlap_info(self.h, C.byref(oi)))
        return _overlap_info(oi)

    def trim_info(self):
        """the trim's counts summed over the batches handed out so far -> dict as Context.docs_trim gives"""
        ti = _lib.TrimInfo()
        check(self.ctx.lib.lime_seq_reader_trim_info(self.h, C.byref(ti)))
        return _trim_info(ti)

    def info(self):
        f, nr, nl, nb, w = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(self.ctx.lib.lime_seq_reader_info(self.h, C.byref(f), C.byref(nr), C.byref(nl), C.byref(nb), C.byref(w)))
        return {"format": "fastq" if f.value == 1 else "fasta", "records": int(nr.value), "lines": int(nl.value), "bytes": int(nb.value),
                "window_bytes": int(w.value)}

    def close(self):
        if self.h:
            if self.ctx.h:                   # (a context that is closed already released it: lime_shutdown, also when both go in one collection)
                self.ctx.lib.lime_seq_reader_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Docs:
    """a document collection resident in HBM (lime_docs), owned by its Context"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def info(self):
        """-> (n_docs, n_text)"""
        nd, nt = C.c_uint32(), C.c_uint64()
        check(self.ctx.lib.lime_docs_info(self.h, C.byref(nd), C.byref(nt)))
        return int(nd.value), int(nt.value)

    def device(self):
        """-> (address of text, address of doc_off) in HBM, for the *_dev calls that take documents"""
        pt, po = C.c_void_p(), C.c_void_p()
        check(self.ctx.lib.lime_docs_device(self.h, C.byref(pt), C.byref(po)))
        return pt.value, po.value

    def get(self):
        """host copies -> (text uint8[n_text], doc_off uint64[n_docs + 1])"""
        nd, nt = self.info()
        text, off = np.zeros(max(nt, 1), dtype=np.uint8), np.zeros(nd + 1, dtype=np.uint64)
        check(self.ctx.lib.lime_docs_get(self.h, text.ctypes.data, off.ctypes.data))
        return text[:nt], off

    @property
    def has_qual(self):
        """do the documents hold their reads' quality strings (docs_from_fastq_qual*)?"""
        p = C.c_void_p()
        check(self.ctx.lib.lime_docs_qual_device(self.h, C.byref(p)))
        return bool(p.value)

    @property
    def qual(self):
        """host copy of the quality bytes, uint8[n_text], laid out like text by doc_off (LimeError for documents without)"""
        nt = self.info()[1]
        q = np.zeros(max(nt, 1), dtype=np.uint8)
        check(self.ctx.lib.lime_docs_get_qual(self.h, q.ctypes.data))
        return q[:nt]

    def qual_device(self):
        """-> address of the quality bytes in HBM, or None"""
        p = C.c_void_p()
        check(self.ctx.lib.lime_docs_qual_device(self.h, C.byref(p)))
        return p.value

    def revcomp(self, stream=None):
        """every document reversed and complemented (fasta_read(path, rc=True)'s records) -> Docs"""
        h = C.c_void_p()
        check(self.ctx.lib.lime_docs_revcomp(self.ctx.h, self.h, stream, C.byref(h)))
        return self.ctx._docs_of(h)

    def close(self):
        if self.h:
            if self.ctx.h:                   # (a context that is closed already released it: lime_shutdown, also when both go in one collection)
                self.ctx.lib.lime_docs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GenomeIndex:
    """a genome collection's index resident in HBM (lime_gindex), owned by its Context"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def info(self):
        nd, nt, cap, term = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint8()
        check(self.ctx.lib.lime_gindex_info(self.h, C.byref(nd), C.byref(nt), C.byref(cap), C.byref(term)))
        return {"n_docs": int(nd.value), "n_text": int(nt.value), "lcp_cap": int(cap.value), "term": int(term.value),
                "positions": int(nt.value) + int(nd.value)}

    def save(self, path):
        check(self.ctx.lib.lime_gindex_save(self.h, os.fsencode(path)))

    def close(self):
        if self.h:
            if self.ctx.h:                   # (a context that is closed already released it: lime_shutdown, also when both go in one collection)
                self.ctx.lib.lime_gindex_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Lists:
    """one collection's clusterChoose result resident in HBM (lime_lists), owned by its Context"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def info(self):
        """-> (n_reads, n_pairs, norm, beta)"""
        nr, npairs, norm, beta = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_float()
        check(self.ctx.lib.lime_lists_info(self.h, C.byref(nr), C.byref(npairs), C.byref(norm), C.byref(beta)))
        return int(nr.value), int(npairs.value), int(norm.value), float(beta.value)

    def get(self):
        """host copies -> (row_max u8[n_reads], row_off u64[n_reads + 1], pairs u32[n, 2] = (idRef, sim))"""
        nr = self.info()[0]
        mx = np.zeros(nr + 1, dtype=np.uint8)
        off = np.zeros(nr + 1, dtype=np.uint64)
        pp, npairs = C.c_void_p(), C.c_uint64(0)
        check(self.ctx.lib.lime_lists_get(self.h, mx.ctypes.data, off.ctypes.data, C.byref(pp), C.byref(npairs)))
        return mx[:nr], off, self.ctx._pairs_out(pp, npairs)

    def norms(self):
        """the norms of Lists made with one per read (lists_concat_norms) -> u8[n_reads]; LimeError for Lists with one norm"""
        nr = self.info()[0]
        nm = np.zeros(nr + 1, dtype=np.uint8)
        check(self.ctx.lib.lime_lists_get_norms(self.h, nm.ctypes.data))
        return nm[:nr]

    def close(self):
        if self.h:
            if self.ctx.h:                   # (a context that is closed already released it: lime_shutdown, also when both go in one collection)
                self.ctx.lib.lime_lists_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Taxonomy:
    """a lineage file at one rank (lime_taxonomy_load); its device copy is made by the first classification on a device"""

    def __init__(self, path, rank, higher, n_targ):
        self.lib = _lib.load()
        h = C.c_void_p()
        check_cls(self.lib.lime_taxonomy_load(str(path).encode(), int(rank), int(bool(higher)), int(n_targ), C.byref(h)))
        self.h, self.n_targ = h, int(n_targ)

    def close(self):
        if self.h:
            self.lib.lime_taxonomy_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_taxonomy(path, rank, higher, n_targ):
    return Taxonomy(path, rank, higher, n_targ)


def write_classification(path, verdicts):
    """the classification file (lime_classify's bytes) from VERDICT records"""
    v = np.ascontiguousarray(verdicts, dtype=VERDICT)
    check_cls(_lib.load().lime_write_classification(str(path).encode(), v.ctypes.data if len(v) else None, len(v)))


class ClassificationWriter:
    """the classification file in parts (lime_classification_writer): written under a temporary name, renamed by close(commit=True).
    As a context manager it commits on a clean exit and removes the file on an exception"""

    def __init__(self, path):
        self.lib = _lib.load()
        h = C.c_void_p()
        check_cls(self.lib.lime_classification_writer_open(os.fsencode(path), C.byref(h)))
        self.h = h

    def append(self, first_read, verdicts):
        v = np.ascontiguousarray(verdicts, dtype=VERDICT)
        check_cls(self.lib.lime_classification_writer_append(self.h, int(first_read), v.ctypes.data if len(v) else None, len(v)))

    def close(self, commit=True):
        if self.h:
            h, self.h = self.h, None
            check_cls(self.lib.lime_classification_writer_close(h, int(bool(commit))))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(commit=exc_type is None)
        return False

    def __del__(self):
        try:
            self.close(commit=False)
        except Exception:
            pass


def classify_mem(lists, norms, betas, n_targ, taxonomy, binary=True, read_norms=None):
    """Classify on the host over 2 or 4 (row_max, row_off, pairs) triples (Lists.get's copies) -> (verdicts, counts).  read_norms: per list
    None or u8[n_reads], the list's norm for every read (lime_classify_mem_norms; norms[i] serves the lists whose entry is None)"""
    lib = _lib.load()
    k = len(lists)
    mx = [np.ascontiguousarray(l[0], dtype=np.uint8) for l in lists]
    off = [np.ascontiguousarray(l[1], dtype=np.uint64) for l in lists]
    pr = [np.ascontiguousarray(np.asarray(l[2], dtype=np.uint32).reshape(-1, 2)) for l in lists]
    n_reads = len(mx[0]) if k else 0
    P = lambda arrs: (C.c_void_p * k)(*[a.ctypes.data for a in arrs])
    nm = np.ascontiguousarray(norms, dtype=np.uint32)
    bt = np.ascontiguousarray(betas, dtype=np.float32)
    v = np.zeros(max(n_reads, 1), dtype=VERDICT)
    counts = (C.c_uint64 * 4)()
    if read_norms is None:
        check_cls(lib.lime_classify_mem(k, P(mx), P(off), P(pr), nm.ctypes.data, bt.ctypes.data, int(bool(binary)), n_reads, n_targ,
                                        taxonomy.h, v.ctypes.data, counts))
    else:
        if len(read_norms) != k:
            raise ValueError("classify_mem: one read_norms entry (None or u8[n_reads]) per list")
        rn = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in read_norms]
        for a in rn:
            if a is not None and len(a) != n_reads:
                raise ValueError("classify_mem: read_norms entries hold one norm per read")
        prn = (C.c_void_p * k)(*[None if a is None else a.ctypes.data for a in rn])
        check_cls(lib.lime_classify_mem_norms(k, P(mx), P(off), P(pr), nm.ctypes.data, prn, bt.ctypes.data, int(bool(binary)), n_reads, n_targ,
                                              taxonomy.h, v.ctypes.data, counts))
    return v[:n_reads], list(counts)


def pack_documents(reads, genomes):
    """lists of bytes / str -> (text uint8: the documents back to back without terminators, reads first; doc_off uint64[n_docs + 1])"""
    docs = [d.encode() if isinstance(d, str) else bytes(d) for d in list(reads) + list(genomes)]
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    text = np.frombuffer(b"".join(docs), dtype=np.uint8) if int(off[-1]) else np.zeros(1, np.uint8)
    return np.ascontiguousarray(text), off


def build_index(reads, genomes, term=0, lcp_cap=0, ctx=None):
    """lime_amd.builder.build_arrays(reads, genomes, term) on the GPU -> (ebwt, lcp, da); lcp_cap > 0: min(lcp, lcp_cap).  ctx: a Context to
    run on (default: a fresh one on the current device, closed again)"""
    own = ctx is None
    ctx = ctx or Context()
    try:
        return ctx.build_index(reads, genomes, term, lcp_cap)
    finally:
        if own:
            ctx.close()


def build_index_dev(ctx, text_t, doc_off_t, n_docs, n_text, term=0, lcp_cap=0, stream=None, out=None):
    """Context.build_index_dev"""
    return ctx.build_index_dev(text_t, doc_off_t, n_docs, n_text, term, lcp_cap, stream, out)


def build_genome_index(ctx, genomes, term=0, lcp_cap=0):
    """Context.build_genome_index"""
    return ctx.build_genome_index(genomes, term, lcp_cap)


def load_genome_index(ctx, path):
    """Context.load_genome_index"""
    return ctx.load_genome_index(path)


def merge_index(ctx, reads, gi, lcp_cap=0):
    """Context.merge_index"""
    return ctx.merge_index(reads, gi, lcp_cap)


def merge_index_dev(ctx, text_t, doc_off_t, n_reads, n_text, gi, lcp_cap=0, stream=None, out=None):
    """Context.merge_index_dev"""
    return ctx.merge_index_dev(text_t, doc_off_t, n_reads, n_text, gi, lcp_cap, stream, out)


def gindex_probe(path):
    """the header and size checks of a genome index file without a device -> {n_docs, n_text, lcp_cap, term}"""
    nd, nt, cap, term = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint8()
    check(_lib.load().lime_gindex_probe(os.fsencode(path), C.byref(nd), C.byref(nt), C.byref(cap), C.byref(term)))
    return {"n_docs": int(nd.value), "n_text": int(nt.value), "lcp_cap": int(cap.value), "term": int(term.value)}


def gindex_shard_plan(doc_off, max_positions):
    """a genome collection cut into index shards (lime_gindex_shard_plan; no device): doc_off[n_docs + 1] the genomes' starts in their
    text -> the cuts [first genome of shard 0, of shard 1, ..., n_docs]: consecutive genomes while a shard's positions (symbols + one
    terminator per genome) stay <= max_positions.  LimeError for a genome above the budget"""
    off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    n_docs = len(off) - 1
    first = np.zeros(n_docs + 2, dtype=np.uint32)
    ns = C.c_uint32(0)
    check(_lib.load().lime_gindex_shard_plan(off.ctypes.data, n_docs, int(max_positions), first.ctypes.data, len(first), C.byref(ns)))
    return [int(x) for x in first[:ns.value + 1]]


def index_size(doc_off):
    off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    return int(_lib.load().lime_index_size(off.ctypes.data, len(off) - 1))


def fasta_read(path, rc=False):
    """a FASTA file's records -> list of bytes (lime_fasta_read: header lines dropped, CR / LF dropped, case kept; rc: reverse complements)"""
    lib = _lib.load()
    pt, po, nd = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
    rcode = lib.lime_fasta_read(os.fsencode(path), int(bool(rc)), C.byref(pt), C.byref(po), C.byref(nd))
    if rcode != 0:
        raise LimeError(rcode, f"lime_fasta_read: {path}")
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(nd.value + 1,)).copy()
        raw = C.string_at(pt, int(off[-1]))
    finally:
        lib.lime_free(pt); lib.lime_free(po)
    return [raw[int(off[k]):int(off[k + 1])] for k in range(nd.value)]


def fastq_read(path, rc=False):
    """a four-line FASTQ file's reads -> list of bytes (lime_fastq_read: the sequence lines, CR dropped, case kept; rc: reverse complements).
    A malformed file: LimeError with `line <L>: <reason>`"""
    lib = _lib.load()
    pt, po, nd = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
    check(lib.lime_fastq_read(os.fsencode(path), int(bool(rc)), C.byref(pt), C.byref(po), C.byref(nd)))
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(nd.value + 1,)).copy()
        raw = C.string_at(pt, int(off[-1]))
    finally:
        lib.lime_free(pt); lib.lime_free(po)
    return [raw[int(off[k]):int(off[k + 1])] for k in range(nd.value)]


def fastq_read_qual(path):
    """fastq_read with the quality strings (lime_fastq_read_qual) -> (text uint8[n], qual uint8[n], doc_off uint64[n_docs + 1])"""
    lib = _lib.load()
    pt, pq, po, nd = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(0)
    check(lib.lime_fastq_read_qual(os.fsencode(path), C.byref(pt), C.byref(pq), C.byref(po), C.byref(nd)))
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(nd.value + 1,)).copy()
        text = np.frombuffer(C.string_at(pt, int(off[-1])), dtype=np.uint8).copy()
        qual = np.frombuffer(C.string_at(pq, int(off[-1])), dtype=np.uint8).copy()
    finally:
        lib.lime_free(pt); lib.lime_free(pq); lib.lime_free(po)
    return text, qual, off


def quality_trim(text, qual, doc_off, q5, q3):
    """the quality rule in plain host code (lime_quality_trim) -> (text, doc_off, info dict)"""
    lib = _lib.load()
    t = np.ascontiguousarray(text, dtype=np.uint8); q = np.ascontiguousarray(qual, dtype=np.uint8); off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    pt, po, ti = C.c_void_p(), C.c_void_p(), _lib.TrimInfo()
    check(lib.lime_quality_trim(t.ctypes.data if len(t) else None, q.ctypes.data if len(q) else None, off.ctypes.data, len(off) - 1, int(q5), int(q3),
                                C.byref(pt), C.byref(po), C.byref(ti)))
    try:
        new_off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(len(off),)).copy()
        new_text = np.frombuffer(C.string_at(pt, int(new_off[-1])), dtype=np.uint8).copy()
    finally:
        lib.lime_free(pt); lib.lime_free(po)
    return new_text, new_off, _trim_info(ti)


def adapter_trim(text, doc_off, adapter, min_overlap=3, max_err_pct=10):
    """the adapter rule in plain host code (lime_adapter_trim) -> (text, doc_off, info dict)"""
    lib = _lib.load()
    t = np.ascontiguousarray(text, dtype=np.uint8); off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    a = _adapter_bytes(adapter)
    pt, po, ti = C.c_void_p(), C.c_void_p(), _lib.TrimInfo()
    check(lib.lime_adapter_trim(t.ctypes.data if len(t) else None, off.ctypes.data, len(off) - 1, a, len(a), int(min_overlap), int(max_err_pct),
                                C.byref(pt), C.byref(po), C.byref(ti)))
    try:
        new_off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(len(off),)).copy()
        new_text = np.frombuffer(C.string_at(pt, int(new_off[-1])), dtype=np.uint8).copy()
    finally:
        lib.lime_free(pt); lib.lime_free(po)
    return new_text, new_off, _trim_info(ti)


def overlap_trim(text1, doc_off1, text2, doc_off2, min_overlap=30, max_err_pct=10):
    """the overlap cut's rule in plain host code (lime_pair_overlap_trim) -> (text1, doc_off1, text2, doc_off2, insert uint32 per pair, info dict)"""
    lib = _lib.load()
    t1 = np.ascontiguousarray(text1, dtype=np.uint8); o1 = np.ascontiguousarray(doc_off1, dtype=np.uint64)
    t2 = np.ascontiguousarray(text2, dtype=np.uint8); o2 = np.ascontiguousarray(doc_off2, dtype=np.uint64)
    if len(o1) != len(o2):
        raise ValueError("overlap_trim: the mates hold different numbers of reads")
    p1, q1, p2, q2, pi, oi = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), _lib.OverlapInfo()
    check(lib.lime_pair_overlap_trim(t1.ctypes.data if len(t1) else None, o1.ctypes.data, t2.ctypes.data if len(t2) else None, o2.ctypes.data, len(o1) - 1,
                                     int(min_overlap), int(max_err_pct), C.byref(p1), C.byref(q1), C.byref(p2), C.byref(q2), C.byref(pi), C.byref(oi)))
    try:
        n = len(o1) - 1
        n1 = np.ctypeslib.as_array(C.cast(q1, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        n2 = np.ctypeslib.as_array(C.cast(q2, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        x1 = np.frombuffer(C.string_at(p1, int(n1[-1])), dtype=np.uint8).copy()
        x2 = np.frombuffer(C.string_at(p2, int(n2[-1])), dtype=np.uint8).copy()
        ins = np.frombuffer(C.string_at(pi, 4 * n), dtype=np.uint32).copy()
    finally:
        for p in (p1, q1, p2, q2, pi):
            lib.lime_free(p)
    return x1, n1, x2, n2, ins, _overlap_info(oi)


def read_filter(text, doc_off, polyx=None, polyx_min=10, max_len=0, min_len=0, max_n=None, min_complexity=0):
    """the read filter's rule in plain host code (lime_read_filter; the parameters as Context.docs_filter takes them) -> (text, doc_off, info dict)"""
    lib = _lib.load()
    t = np.ascontiguousarray(text, dtype=np.uint8); off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    f = _filter_of(polyx, polyx_min, max_len, min_len, max_n, min_complexity)
    pt, po, fi = C.c_void_p(), C.c_void_p(), _lib.FilterInfo()
    check(lib.lime_read_filter(t.ctypes.data if len(t) else None, off.ctypes.data, len(off) - 1, C.byref(f), C.byref(pt), C.byref(po), C.byref(fi)))
    try:
        new_off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(len(off),)).copy()
        new_text = np.frombuffer(C.string_at(pt, int(new_off[-1])), dtype=np.uint8).copy()
    finally:
        lib.lime_free(pt); lib.lime_free(po)
    return new_text, new_off, _filter_info(fi)


def qc_words(n_pos):
    """LIME_QC_WORDS(n_pos): the uint64 words of the tables of read_qc"""
    return 9 * (int(n_pos) + 1) + 101 + 256


def _qc_tables(n_pos, tables):
    if not 1 <= int(n_pos) <= _lib.QC_MAX_POS:
        raise ValueError(f"n_pos is 1 .. {_lib.QC_MAX_POS}")
    if tables is None:
        return np.zeros(qc_words(n_pos), dtype=np.uint64)
    if not (isinstance(tables, np.ndarray) and tables.dtype == np.uint64 and tables.flags.c_contiguous and tables.shape == (qc_words(n_pos),)):
        raise ValueError("tables is a contiguous uint64 array of qc_words(n_pos) words")
    return tables


def qc_split(tables, n_pos):
    """the flat tables -> dict of views: rows (n_pos + 1, 8) [A, C, G, T, other, qsum, q20, q30], len_hist (n_pos + 1), gc_hist (101), mq_hist (256),
    and tables, the flat array itself"""
    n = int(n_pos) + 1
    return {"rows": tables[:8 * n].reshape(n, 8), "len_hist": tables[8 * n:9 * n], "gc_hist": tables[9 * n:9 * n + 101], "mq_hist": tables[9 * n + 101:],
            "tables": tables}


def read_qc(text, doc_off, n_pos=256, qual=None, tables=None):
    """the per-position statistics' rule in plain host code (lime_read_qc; the oracle of Context.docs_qc): qual, the quality bytes laid out like
    text, or None; tables as Context.docs_qc takes them (the counts are ADDED) -> dict as qc_split gives"""
    lib = _lib.load()
    t = np.ascontiguousarray(text, dtype=np.uint8); off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    q = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
    if q is not None and len(q) != len(t):
        raise ValueError("read_qc: qual is laid out like text")
    out = _qc_tables(n_pos, tables)
    if q is not None and not len(q):
        q = np.zeros(1, dtype=np.uint8)             # (no symbol, but qualities: not NULL)
    check(lib.lime_read_qc(t.ctypes.data if len(t) else None, None if q is None else q.ctypes.data, off.ctypes.data, len(off) - 1, int(n_pos),
                           out.ctypes.data))
    return qc_split(out, n_pos)


def qc_report_write(path, names, formats, n_pos, before, after):
    """the statistics of the reads files `names` as JSON (lime_qc_report_write): formats, "fasta" / "fastq" (or 0 / 1) per file; before, after:
    per file the tables (the flat array, or the dict that read_qc / Context.docs_qc give)"""
    k = len(names)
    if not (len(formats) == len(before) == len(after) == k):
        raise ValueError("qc_report_write: one format and two sets of tables per file")
    flat = [[np.ascontiguousarray(x["tables"] if isinstance(x, dict) else x, dtype=np.uint64) for x in side] for side in (before, after)]
    for side in flat:
        for x in side:
            if x.shape != (qc_words(n_pos),):
                raise ValueError("qc_report_write: tables of qc_words(n_pos) words")
    nm = (C.c_char_p * max(k, 1))(*[os.fsencode(n) for n in names])
    fm = (C.c_int * max(k, 1))(*[_format_of(f) for f in formats])
    pb = (C.c_void_p * max(k, 1))(*[x.ctypes.data for x in flat[0]])
    pa = (C.c_void_p * max(k, 1))(*[x.ctypes.data for x in flat[1]])
    check(_lib.load().lime_qc_report_write(os.fsencode(path), k, nm, fm, int(n_pos), pb, pa))


def seq_format(path):
    """"fastq" if the file's first byte is '@', else "fasta" (lime_seq_format)"""
    f = C.c_int(0)
    check(_lib.load().lime_seq_format(os.fsencode(path), C.byref(f)))
    return "fastq" if f.value == 1 else "fasta"


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def trim_cache():
    """give the device blocks that closed contexts left with the library back to the driver (lime_trim_cache); returns the bytes released"""
    return int(_lib.load().lime_trim_cache())


def reserve(nbytes):
    """take `nbytes` of device memory from the driver now, once, for the large buffers of every later context (lime_reserve); LimeError if refused"""
    rc = _lib.load().lime_reserve(int(nbytes))
    if rc != 0:
        raise LimeError(rc, "lime_reserve")


def sim_bytes(n_reads, n_refs):
    return int(_lib.load().lime_sim_bytes(n_reads, n_refs))


def aux_name(file_fasta):
    k = file_fasta.find(".fasta")               # ClusterLCP.cpp:294
    return (file_fasta if k < 0 else file_fasta[:k]) + ".out"


# ---- program level: same arguments and files as the reference's executables ----------------
def cluster_lcp(file_fasta, num_reads, num_genomes, alpha, threads=1, ctx=None):
    """`ClusterLCP fileFasta numReads numGenomes alpha threads` (src/ClusterLCP.cpp:47-320)."""
    lib = _lib.load()
    for ext in (".lcp", ".da"):
        if not os.path.exists(file_fasta + ext):
            raise FileNotFoundError(f"Error opening {file_fasta + ext}.")
    lcp = np.memmap(file_fasta + ".lcp", dtype="<u4", mode="r") if os.path.getsize(file_fasta + ".lcp") else np.zeros(0, np.uint32)
    da = np.memmap(file_fasta + ".da", dtype="<u4", mode="r") if os.path.getsize(file_fasta + ".da") else np.zeros(0, np.uint32)
    own = ctx is None
    ctx = ctx or Context()
    try:
        cl, nc, ml = ctx.detect(lcp, da[:len(lcp)], num_reads, alpha)
    finally:
        if own:
            ctx.close()
    cl = np.ascontiguousarray(cl)
    check(lib.lime_write_clrs(f"{file_fasta}.{alpha}.clrs".encode(), cl.ctypes.data if nc else None, nc))
    check(lib.lime_write_aux(aux_name(file_fasta).encode(), num_reads, num_genomes, alpha, ml, nc))
    return nc, ml


def lime_paired(files, output, num_reads, num_genomes, lineage, read_len, threads=1, ebwt=True, higher=False, binary=True, ctx=None):
    """`LiME_paired.sh File1_F File1_RC File2_F File2_RC output numReads numGenomes LineageFile readLen threads` (LiME_paired.sh:44-79) in
    one process, like lime_amd/bin/LiME_paired: alpha 16, beta 0.25, taxRank 1; reads <file>.lcp / .da / .ebwt, writes only `output`
    (no .clrs, .out or .res.* files).  -> counts {C, U, A, H}"""
    if len(files) != 4:
        raise ValueError("LiME_paired takes four collections: File1_F File1_RC File2_F File2_RC")
    alpha, beta, rank = 16, float(np.float32(0.25)), 1
    norm = ((int(read_len) & 0xFF) + 1 - alpha) & 0xFFFFFFFF
    tx = Taxonomy(lineage, rank, higher, num_genomes)
    own = ctx is None
    ctx = ctx or Context()
    try:
        lists = []
        for f in files:
            lcp = np.memmap(f + ".lcp", dtype="<u4", mode="r")
            da = np.memmap(f + ".da", dtype="<u4", mode="r")
            eb = np.memmap(f + ".ebwt", dtype=np.uint8, mode="r") if ebwt else None
            li, _ = ctx.fused_choose_lists(lcp, da, eb, num_reads, num_genomes, alpha, norm, beta)
            lists.append(li)
        v, counts = ctx.classify_lists_dev(lists, num_genomes, tx, binary)
        for li in lists:
            li.close()
    finally:
        if own:
            ctx.close()
        tx.close()
    write_classification(output, v)
    return counts


def lime_fasta(reads, lineage, read_len, output, refs=None, gidx=None, alpha=16, beta=0.25, rank=1, trlcp=0, ebwt=True, higher=False, binary=True,
               ctx=None, batch_reads=0, window_bytes=0, trim_qual=None, trim_adapter=None,
               adapter_overlap=3, adapter_error=10, trim_polyx=None, max_len=0, min_len=0, max_n=None, min_complexity=0, trim_overlap=None,
               qc_report=None, qc_positions=None):
    """`LiME_fasta reads_1.fasta [reads_2.fasta] (--refs refs.fasta | --gidx file.gidx) --lineage LineageFile --readlen (L | auto) --out output
    [--alpha 16] [--beta 0.25] [--rank 1] [--trlcp k]`, like lime_amd/bin/LiME_fasta (read_len="auto": every read by its own length): the files are parsed on the device (each reads file
    FASTA or four-line FASTQ, by its first byte; refs FASTA), the
    genome index is built there (refs) or loaded (gidx: a file, or a list of files, the index shards of one database in genome order:
    repeated `--gidx`), only `output` is written.  batch_reads > 0: `--batch-reads N [--window-bytes W]`,
    the sample read and classified N reads at a time, `output` appended to batch by batch and renamed at the end.  trim_qual: `--trim-qual`,
    Q (the 3' end) or (Q5, Q3): the reads, FASTQ, are cut by the quality rule on the device first; read_len must be "auto".
    trim_adapter: `--trim-adapter`, SEQ or (SEQ, SEQ2) (SEQ2 for the second reads file), with adapter_overlap and adapter_error
    (`--adapter-overlap`, `--adapter-error`): the reads, FASTA or FASTQ, are cut where the 3' adapter begins, behind the quality trim;
    read_len must be "auto".
    trim_polyx, max_len, min_len, max_n, min_complexity: `--trim-polyx BASES[,T]` ("G", "GA,12" or (BASES, T)), `--max-len`, `--min-len`,
    `--max-n`, `--min-complexity`: the read filter (Context.docs_filter), behind both trims, each mate on its own.  trim_polyx and max_len
    change lengths and need read_len="auto"; the other three only empty reads and are taken with a fixed read_len too.
    trim_overlap: `--trim-overlap O[,E]`, O or (O, E): adapter read-through cut from the two mates' overlap, with no adapter given
    (Context.docs_trim_overlap), last, behind each mate's trims and filter; it needs two reads files and read_len="auto".
    qc_report, qc_positions: `--qc-report FILE [--qc-positions P]`: the per-position statistics of every reads file as parsed and as it enters
    classification (Context.docs_qc; SeqReader.set_qc with batch_reads), written to FILE as JSON (qc_report_write); P is 1 .. 512, default 256.
    -> counts {C, U, A, H}"""
    reads = [reads] if isinstance(reads, (str, bytes, os.PathLike)) else list(reads)
    if len(reads) not in (1, 2) or (refs is None) == (gidx is None):
        raise ValueError("LiME_fasta takes one or two reads files and either refs or gidx")
    if qc_positions is not None and qc_report is None:
        raise ValueError("LiME_fasta: qc_positions needs qc_report")
    qc_pos = 256 if qc_positions is None else int(qc_positions)
    if not 1 <= qc_pos <= _lib.QC_MAX_POS:
        raise ValueError(f"LiME_fasta: qc_positions is 1 .. {_lib.QC_MAX_POS}")
    formats = [seq_format(r) for r in reads] if qc_report is not None else None
    qc_before, qc_after = [], []
    # each mate's stages in their one order (the readers': lime_seq_reader in include/lime_hip.h), per stage: set it on the reader of mate k,
    # run it on the Docs of mate k -> (Docs, info)
    stages = []
    if trim_qual is not None:
        q5, q3 = _trim_cutoffs(trim_qual)
        if read_len != "auto":
            raise ValueError("LiME_fasta: trim_qual needs read_len=\"auto\": a fixed norm does not fit trimmed reads")
        for r in reads:
            if seq_format(r) != "fastq":
                raise ValueError(f"LiME_fasta: {os.fspath(r)}: trim_qual needs the qualities of a FASTQ file; this one is FASTA")
        stages.append((lambda m, k: m.set_trim(q5, q3), lambda m, k: ctx.docs_trim(m, q5, q3)))
    if trim_adapter is not None:
        adapters = _adapters(trim_adapter, len(reads))
        if read_len != "auto":
            raise ValueError("LiME_fasta: trim_adapter needs read_len=\"auto\": a fixed norm does not fit trimmed reads")
        if not 1 <= int(adapter_overlap) <= min(len(a) for a in adapters) or not 0 <= int(adapter_error) <= 50:
            raise ValueError("LiME_fasta: adapter_overlap is 1 .. the adapter's length, adapter_error 0 .. 50")
        stages.append((lambda m, k: m.set_adapter(adapters[k], adapter_overlap, adapter_error),
                       lambda m, k: ctx.docs_trim_adapter(m, adapters[k], adapter_overlap, adapter_error)))
    if trim_polyx is not None or max_len or min_len or max_n is not None or min_complexity:
        px, px_min = _polyx_arg(trim_polyx)
        if (px or max_len) and read_len != "auto":
            raise ValueError("LiME_fasta: trim_polyx and max_len need read_len=\"auto\": a fixed norm does not fit shortened reads")
        if not 0 <= int(min_complexity) <= 100 or int(max_len) < 0 or int(min_len) < 0 or (max_n is not None and int(max_n) < 0):
            raise ValueError("LiME_fasta: min_complexity is 0 .. 100 percent; max_len, min_len and max_n are not negative")
        flt = dict(polyx=px, polyx_min=px_min, max_len=max_len, min_len=min_len, max_n=max_n, min_complexity=min_complexity)
        stages.append((lambda m, k: m.set_filter(**flt), lambda m, k: ctx.docs_filter(m, **flt)))
    if trim_overlap is not None:                                    # last: the one stage that needs both mates
        ov = _overlap_arg(trim_overlap)
        if read_len != "auto" or len(reads) != 2:
            raise ValueError("LiME_fasta: trim_overlap needs two reads files and read_len=\"auto\": a fixed norm does not fit trimmed reads")
    norm = NORM_PER_READ if read_len == "auto" else ((int(read_len) & 0xFF) + 1 - int(alpha)) & 0xFFFFFFFF     # (`--readlen auto`)
    own = ctx is None
    ctx = ctx or Context()
    tx = None
    try:
        mates = []
        for k, r in enumerate(reads):
            if batch_reads:
                m = ctx.seq_reader(r, window_bytes)
                for on_reader, _ in stages:
                    on_reader(m, k)
                if qc_report is not None:
                    m.set_qc(qc_pos)
            else:   # with the qualities for the quality trim and for the report's quality tables (the reads then keep them: no later step looks at them)
                m = ctx.docs_from_fastq_qual(r) if trim_qual is not None or (formats and formats[k] == "fastq") else ctx.docs_from_file(r)
                if qc_report is not None:
                    qc_before.append(ctx.docs_qc(m, qc_pos))
                for _, on_docs in stages:
                    whole, m = m, on_docs(m, k)[0]
                    whole.close()
            mates.append(m)
        if trim_overlap is not None:
            if batch_reads:
                mates[0].set_overlap(mates[1], *ov)
            else:
                whole = mates
                mates = list(ctx.docs_trim_overlap(whole[0], whole[1], *ov)[:2])
                for m in whole:
                    m.close()
        if qc_report is not None and not batch_reads:               # the reads as they enter classification
            qc_after = [ctx.docs_qc(m, qc_pos) for m in mates]
        if refs is not None:
            g = ctx.docs_from_fasta(refs)
            nd, nt = g.info()
            pt, po = g.device()
            h = C.c_void_p()
            check(ctx.lib.lime_gindex_build_dev(ctx.h, pt, po, nd, nt, 0, int(trlcp), None, C.byref(h)))
            gi = ctx._gindex_of(h)
            g.close()
        elif isinstance(gidx, (list, tuple)):                       # the shards of one genome database, in genome order
            for g in gidx:
                p = gindex_probe(g)
                if (p["lcp_cap"], p["term"]) != (gindex_probe(gidx[0])["lcp_cap"], gindex_probe(gidx[0])["term"]):
                    raise ValueError(f"LiME_fasta: {g} and {gidx[0]} were built with different lcp_cap or terminators")
            gi = [ctx.load_genome_index(g) for g in gidx]
        else:
            gi = ctx.load_genome_index(gidx)
        shards = gi if isinstance(gi, list) else [gi]
        tx = Taxonomy(lineage, rank, higher, sum(g.info()["n_docs"] for g in shards))
        if batch_reads:
            with ClassificationWriter(output) as w:
                _, counts, _ = ctx.classify_sample_stream(mates, gi, tx, alpha, norm, float(np.float32(beta)), batch_reads, ebwt, binary,
                                                          0 if refs is not None else trlcp, sink=lambda first, v, st: w.append(first, v))
        elif isinstance(gi, list):
            v, counts, _ = ctx.classify_sample_shards(mates, gi, tx, alpha, norm, float(np.float32(beta)), ebwt, binary, trlcp)
        else:
            v, counts, _ = ctx.classify_sample(mates, gi, tx, alpha, norm, float(np.float32(beta)), ebwt, binary, 0 if refs is not None else trlcp)
        if qc_report is not None and batch_reads:
            qc_before = [m.qc("raw") for m in mates]
            qc_after = [m.qc("out") for m in mates]
        for d in mates:
            d.close()
        for g in shards:
            g.close()
    finally:
        if own:
            ctx.close()
        if tx is not None:
            tx.close()
    if not batch_reads:
        write_classification(output, v)
    if qc_report is not None:
        qc_report_write(qc_report, [os.fspath(r) for r in reads], formats, qc_pos, qc_before, qc_after)
    return counts


def cluster_bwt_da(file_fasta, read_len, beta, threads=1, ebwt=True, binary=True, ctx=None):
    """`ClusterBWT_DA fileFasta readLen beta threads` (src/ClusterBWT_DA.cpp:453-773).
    ebwt / binary stand for the reference's compile-time EBWT / BIN switches (Makefile:12-13)."""
    lib = _lib.load()
    nr, ng, al = C.c_uint32(), C.c_uint32(), C.c_uint32()
    ml, nc = C.c_uint64(), C.c_uint64()
    if lib.lime_read_aux(aux_name(file_fasta).encode(), C.byref(nr), C.byref(ng), C.byref(al), C.byref(ml), C.byref(nc)):
        raise FileNotFoundError(f"Error opening {aux_name(file_fasta)}.")
    if ml.value > _lib.MAX_CLUSTER:
        raise LimeError(_lib.ERR_MAXLEN, f"maximum cluster size is {ml.value} greater than sizeMaxBuf")
    read_len = int(read_len) & 0xFF                       # %hhu, :519-521
    norm = (read_len + 1 - al.value) & 0xFFFFFFFF         # :555
    clrs = np.fromfile(f"{file_fasta}.{al.value}.clrs", dtype="<u8").reshape(-1, 2)[:nc.value]
    da = np.fromfile(file_fasta + ".da", dtype="<u4")
    eb = np.fromfile(file_fasta + ".ebwt", dtype=np.uint8) if ebwt else None
    own = ctx is None
    ctx = ctx or Context()
    try:
        sim = ctx.score(da, eb, clrs, nr.value, ng.value)
        mx, _ = ctx.choose(sim) if nr.value else (np.zeros(0, np.uint8), None)
    finally:
        if own:
            ctx.close()
    beta32 = float(np.float32(beta))
    res = file_fasta + ".res"
    if binary:
        check(lib.lime_write_res_bin((res + ".bin").encode(), (res + ".pos").encode(), sim.ctypes.data,
                                     mx.ctypes.data, nr.value, ng.value, norm, beta32))
    else:
        check(lib.lime_write_res_txt((res + ".txt").encode(), sim.ctypes.data, mx.ctypes.data,
                                     nr.value, ng.value, norm, beta32))
    return sim
