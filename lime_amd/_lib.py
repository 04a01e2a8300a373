"""ctypes loader of liblime_hip.so (the C ABI in include/lime_hip.h).

The library is the product: if it is missing or cannot be loaded this module raises -- there
is no Python or CPU substitute for the kernels.
"""
from __future__ import annotations

import ctypes as C
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
# LIME_LIB: another build of the library (ablation / timing variants of tools/*.sh) -- loaded INSTEAD of the installed one, which those scripts
# used to overwrite; bench.py refuses to run with it
LIB_PATH = os.environ.get("LIME_LIB") or os.path.join(_DIR, "liblime_hip.so")

LIME_OK = 0
ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_MAXLEN, ERR_HALO, ERR_DOCID, ERR_IO = -1, -2, -3, -4, -5, -6, -7
MAX_CLUSTER = 65536
TILE = 4096
FASTA_BLOCK = 4096


class Cluster(C.Structure):
    _fields_ = [("pStart", C.c_uint64), ("len", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("n_clusters", C.c_uint64), ("max_len", C.c_uint64), ("n_updates", C.c_uint64),
                ("n_cross", C.c_uint32), ("n_big", C.c_uint32), ("flags", C.c_uint32), ("wave_records_max", C.c_uint32), ("edge", C.c_uint32), ("reserved", C.c_uint32)]


class Records(C.Structure):
    _fields_ = [("n_bins", C.c_uint32), ("bin_shift", C.c_uint32), ("d_recs", C.c_void_p), ("d_binbase", C.c_void_p),
                ("d_bigrecs", C.c_void_p), ("n_bigrecs", C.c_uint64)]


class TrimInfo(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_changed", C.c_uint64), ("n_empty", C.c_uint64), ("symbols_in", C.c_uint64), ("symbols_out", C.c_uint64)]


QC_MAX_POS = 512                             # LIME_QC_MAX_POS: the most positions with a row of their own in the tables of lime_read_qc
FILTER_OFF = 0xFFFFFFFF                      # LIME_FILTER_OFF: lime_filter_t.max_n without a limit


class Filter(C.Structure):                   # lime_filter_t
    _fields_ = [("polyx_mask", C.c_uint32), ("polyx_min", C.c_uint32), ("max_len", C.c_uint32), ("min_len", C.c_uint32), ("max_n", C.c_uint32),
                ("min_complexity", C.c_uint32)]


class FilterInfo(C.Structure):               # lime_filter_info_t
    _fields_ = [("n_reads", C.c_uint64), ("n_polyx", C.c_uint64), ("n_capped", C.c_uint64), ("n_short", C.c_uint64), ("n_many_n", C.c_uint64),
                ("n_low_complexity", C.c_uint64), ("symbols_in", C.c_uint64), ("symbols_out", C.c_uint64)]


class OverlapInfo(C.Structure):              # lime_overlap_info_t
    _fields_ = [("n_pairs", C.c_uint64), ("n_overlap", C.c_uint64), ("n_cut", C.c_uint64), ("symbols_in", C.c_uint64), ("symbols_out", C.c_uint64)]


class LimeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lime error {code}: {msg}")
        self.code = code


# every symbol include/lime_hip.h declares: (restype, argtypes)
_vp, _u32, _u64, _i, _sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_size_t
_pp = C.POINTER(C.c_void_p)
_pu64 = C.POINTER(C.c_uint64)
SYMBOLS = {
    "lime_init": (_i, [_i, _pp]),
    "lime_shutdown": (None, [_vp]),
    "lime_last_error": (C.c_char_p, []),
    "lime_free": (None, [_vp]),
    "lime_version": (C.c_char_p, []),
    "lime_device_count": (_i, []),
    "lime_pick_device": (_i, [C.c_uint]),
    "lime_set_option": (_i, [_vp, C.c_char_p, C.c_char_p]),
    "lime_trim_cache": (_sz, []),
    "lime_reserve": (C.c_int, [_sz]),
    "lime_detect": (_i, [_vp, _vp, _vp, _u64, _u32, _u32, _pp, _pu64, _pu64]),
    "lime_detect_to_file": (_i, [_vp, _vp, _vp, _u64, _u32, _u32, C.c_char_p, _pu64, _pu64]),
    "lime_register_file": (_i, [_vp, _sz, _i]),
    "lime_unregister_file": (None, [_vp]),
    "lime_score": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp]),
    "lime_fused": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp, _pu64, _pu64]),
    "lime_choose": (_i, [_vp, _vp, _u32, _u32, _vp, _vp]),
    "lime_sim_bytes": (_sz, [_u32, _u32]),
    "lime_fused_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u64, _i, _u32, _u32, _u32, _vp, _i, _vp]),
    "lime_detect_dev": (_i, [_vp, _vp, _vp, _u64, _u64, _i, _u64, _u32, _u32, _pp, _pu64, _pu64, _vp]),
    "lime_score_dev": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp, _i, _vp]),
    "lime_choose_dev": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "lime_synth_dev": (_i, [_vp, _u64, _u64, _u64, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "lime_get_stats": (_i, [_vp, C.POINTER(Stats), _vp]),
    "lime_set_timing": (_i, [_vp, _i]),
    "lime_get_timing": (_i, [_vp, C.POINTER(C.c_double), _pu64]),
    "lime_get_timing_ex": (_i, [_vp, C.POINTER(C.c_double), _pu64]),
    "lime_get_host_times": (_i, [_vp, C.POINTER(C.c_double)]),
    "lime_sym_index": (C.c_uint8, [C.c_uint8]),
    "lime_pair_score": (C.c_uint8, [_vp, _vp]),
    "lime_rec_layout": (_i, [_u32, _u32, _u32, _u32, _vp]),
    "lime_rec_valid": (_i, [_u32, _u32]),
    "lime_rec_of": (_u32, [_u32, _u32, _u32]),
    "lime_rec_sub2": (_u32, [_u32, _u32, _u32, _u32]),
    "lime_rec_bin": (_u32, [_u32, _u32, _u32]),
    "lime_rec_batch": (_i, [_vp, _vp, _u64, _u32, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "lime_scan_queue": (None, [_vp]),
    "lime_write_clrs": (_i, [C.c_char_p, _vp, _u64]),
    "lime_write_aux": (_i, [C.c_char_p, _u32, _u32, _u32, _u64, _u64]),
    "lime_read_aux": (_i, [C.c_char_p, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), _pu64, _pu64]),
    "lime_write_res_txt": (_i, [C.c_char_p, _vp, _vp, _u32, _u32, _u32, C.c_float]),
    "lime_write_res_bin": (_i, [C.c_char_p, C.c_char_p, _vp, _vp, _u32, _u32, _u32, C.c_float]),
    "lime_classify": (_i, [_u32, _vp, _i, _u32, _u32, C.c_char_p, C.c_char_p, _i, _i, _vp]),
    "lime_classify_error": (C.c_char_p, []),
    "lime_fused_stream": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u64, _vp, _pu64, _pu64]),
    "lime_choose_pairs_dev": (_i, [_vp, _vp, _u32, _u32, _u32, C.c_float, _vp, _vp, _pp, _pu64, _vp]),
    "lime_fused_choose_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u32, C.c_float, _vp, _vp, _pp, _pu64, C.POINTER(Stats), _vp]),
    "lime_score_choose": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _u32, C.c_float, _vp, _vp, _pp, _pu64, _vp]),
    "lime_combine_edges": (_i, [_vp, _u32]),
    "lime_comm_unique_id": (_i, [_vp]),
    "lime_comm_init": (_i, [_vp, _i, _i, _pp]),
    "lime_comm_destroy": (None, [_vp]),
    "lime_comm_count": (_i, [_vp, C.POINTER(_i)]),
    "lime_comm_error": (C.c_char_p, []),
    "lime_comm_reduce_scatter_tables": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "lime_comm_allreduce_tables": (_i, [_vp, _vp, _sz, _vp]),
    "lime_comm_combine_counters": (_i, [_vp, _vp, _vp]),
    "lime_records_layout": (_i, [_vp, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "lime_fused_records_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u64, _i, _u32, _u32, _u32, _vp]),
    "lime_records_get": (_i, [_vp, _vp, _vp, _vp]),
    "lime_apply_records_dev": (_i, [_vp, _u32, _vp, _vp, _u32, _u32, _vp, _u64, _u64, _u64, _vp, _vp]),
    "lime_partition_records_dev": (_i, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _u32, _u32, _vp, _u64, _vp, C.POINTER(_i), _vp]),
    "lime_comm_exchange_records": (_i, [_vp, _vp, _u32, _u32, _vp, _sz, _pu64, _pu64, _vp]),
    "lime_fused_multi": (_i, [_i, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp, _pu64, _pu64]),
    "lime_score_choose_multi": (_i, [_i, _vp, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _u32, C.c_float, _vp, _vp, _pp, _pu64]),
    "lime_write_res_txt_pairs": (_i, [C.c_char_p, _vp, _vp, _vp, _u32, _u32, C.c_float]),
    "lime_write_res_bin_pairs": (_i, [C.c_char_p, C.c_char_p, _vp, _vp, _vp, _u32, _u32, C.c_float]),
    "lime_choose_lists_dev": (_i, [_vp, _vp, _u32, _u32, _u32, C.c_float, _pp, _vp]),
    "lime_fused_choose_lists_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u32, C.c_float, _pp, C.POINTER(Stats), _vp]),
    "lime_fused_choose_lists": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u32, C.c_float, _pp, C.POINTER(Stats)]),
    "lime_lists_get": (_i, [_vp, _vp, _vp, _pp, _pu64]),
    "lime_lists_info": (_i, [_vp, C.POINTER(_u32), _pu64, C.POINTER(_u32), C.POINTER(C.c_float)]),
    "lime_lists_free": (None, [_vp]),
    "lime_lists_concat_dev": (_i, [_vp, _u32, _vp, _vp, _vp, C.c_float, _pp, _vp]),
    "lime_lists_concat_norms_dev": (_i, [_vp, _u32, _vp, _vp, _vp, _vp, C.c_float, _pp, _vp]),
    "lime_lists_get_norms": (_i, [_vp, _vp]),
    "lime_taxonomy_load": (_i, [C.c_char_p, _i, _i, _u32, _pp]),
    "lime_taxonomy_free": (None, [_vp]),
    "lime_classify_lists_dev": (_i, [_vp, _u32, _vp, _u32, _vp, _i, _vp, _vp, _vp]),
    "lime_classify_mem": (_i, [_u32, _vp, _vp, _vp, _vp, _vp, _i, _u32, _u32, _vp, _vp, _vp]),
    "lime_classify_mem_norms": (_i, [_u32, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u32, _u32, _vp, _vp, _vp]),
    "lime_write_classification": (_i, [C.c_char_p, _vp, _u32]),
    "lime_index_size": (_u64, [_vp, _u32]),
    "lime_build_index": (_i, [_vp, _vp, _vp, _u32, C.c_uint8, _u32, _vp, _vp, _vp]),
    "lime_build_index_dev": (_i, [_vp, _vp, _vp, _u32, _u64, C.c_uint8, _u32, _vp, _vp, _vp, _vp]),
    "lime_get_index_info": (_i, [_vp, C.POINTER(C.c_double)]),
    "lime_fasta_read": (_i, [C.c_char_p, _i, _pp, _pp, C.POINTER(_u32)]),
    "lime_gindex_build": (_i, [_vp, _vp, _vp, _u32, C.c_uint8, _u32, _pp]),
    "lime_gindex_build_dev": (_i, [_vp, _vp, _vp, _u32, _u64, C.c_uint8, _u32, _vp, _pp]),
    "lime_gindex_save": (_i, [_vp, C.c_char_p]),
    "lime_gindex_load": (_i, [_vp, C.c_char_p, _pp]),
    "lime_gindex_info": (_i, [_vp, C.POINTER(_u32), _pu64, C.POINTER(_u32), C.POINTER(C.c_uint8)]),
    "lime_gindex_probe": (_i, [C.c_char_p, C.POINTER(_u32), _pu64, C.POINTER(_u32), C.POINTER(C.c_uint8)]),
    "lime_gindex_free": (None, [_vp]),
    "lime_get_concat_info": (_i, [_vp, C.POINTER(C.c_double)]),
    "lime_gindex_shard_plan": (_i, [_vp, _u32, _u64, _vp, _u32, C.POINTER(_u32)]),
    "lime_merge_size": (_u64, [_vp, _vp, _u32]),
    "lime_merge_index_dev": (_i, [_vp, _vp, _vp, _u32, _u64, _vp, _u32, _vp, _vp, _vp, _vp]),
    "lime_merge_index": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "lime_get_merge_info": (_i, [_vp, C.POINTER(C.c_double)]),
    "lime_docs_from_fasta": (_i, [_vp, C.c_char_p, _pp]),
    "lime_docs_from_bytes": (_i, [_vp, _vp, _u64, _pp]),
    "lime_docs_from_bytes_dev": (_i, [_vp, _vp, _u64, _vp, _pp]),
    "lime_fastq_read": (_i, [C.c_char_p, _i, _pp, _pp, C.POINTER(_u32)]),
    "lime_seq_format": (_i, [C.c_char_p, C.POINTER(_i)]),
    "lime_docs_from_fastq": (_i, [_vp, C.c_char_p, _pp]),
    "lime_docs_from_fastq_bytes": (_i, [_vp, _vp, _u64, _pp]),
    "lime_docs_from_fastq_bytes_dev": (_i, [_vp, _vp, _u64, _vp, _pp]),
    "lime_fastq_read_qual": (_i, [C.c_char_p, _pp, _pp, _pp, C.POINTER(_u32)]),
    "lime_quality_trim": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _pp, _pp, C.POINTER(TrimInfo)]),
    "lime_docs_from_fastq_qual": (_i, [_vp, C.c_char_p, _pp]),
    "lime_docs_from_fastq_qual_bytes": (_i, [_vp, _vp, _u64, _pp]),
    "lime_docs_from_fastq_qual_bytes_dev": (_i, [_vp, _vp, _u64, _vp, _pp]),
    "lime_docs_qual_device": (_i, [_vp, _pp]),
    "lime_docs_get_qual": (_i, [_vp, _vp]),
    "lime_docs_trim_dev": (_i, [_vp, _vp, _u32, _u32, _vp, _pp, C.POINTER(TrimInfo)]),
    "lime_seq_reader_set_trim": (_i, [_vp, _u32, _u32]),
    "lime_seq_reader_trim_info": (_i, [_vp, C.POINTER(TrimInfo)]),
    "lime_adapter_trim": (_i, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _pp, _pp, C.POINTER(TrimInfo)]),
    "lime_docs_trim_adapter_dev": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _pp, C.POINTER(TrimInfo)]),
    "lime_seq_reader_set_adapter": (_i, [_vp, _vp, _u32, _u32, _u32]),
    "lime_seq_reader_adapter_info": (_i, [_vp, C.POINTER(TrimInfo)]),
    "lime_read_filter": (_i, [_vp, _vp, _u32, C.POINTER(Filter), _pp, _pp, C.POINTER(FilterInfo)]),
    "lime_docs_filter_dev": (_i, [_vp, _vp, C.POINTER(Filter), _vp, _pp, C.POINTER(FilterInfo)]),
    "lime_seq_reader_set_filter": (_i, [_vp, C.POINTER(Filter)]),
    "lime_seq_reader_filter_info": (_i, [_vp, C.POINTER(FilterInfo)]),
    "lime_read_qc": (_i, [_vp, _vp, _vp, _u32, _u32, _vp]),
    "lime_docs_qc_dev": (_i, [_vp, _vp, _u32, _vp, _vp]),
    "lime_seq_reader_set_qc": (_i, [_vp, _u32]),
    "lime_seq_reader_qc": (_i, [_vp, _i, _vp]),
    "lime_qc_report_write": (_i, [C.c_char_p, _u32, _vp, _vp, _u32, _vp, _vp]),
    "lime_pair_overlap_trim": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _pp, _pp, _pp, _pp, _pp, C.POINTER(OverlapInfo)]),
    "lime_docs_trim_overlap_dev": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _pp, _pp, C.POINTER(OverlapInfo)]),
    "lime_seq_reader_set_overlap": (_i, [_vp, _vp, _u32, _u32]),
    "lime_seq_reader_next_pair": (_i, [_vp, _vp, _u32, _pp, _pp, _pu64]),
    "lime_seq_reader_overlap_info": (_i, [_vp, C.POINTER(OverlapInfo)]),
    "lime_docs_from_file": (_i, [_vp, C.c_char_p, _pp]),
    "lime_docs_from_arrays_dev": (_i, [_vp, _vp, _vp, _u32, _u64, _vp, _pp]),
    "lime_docs_revcomp": (_i, [_vp, _vp, _vp, _pp]),
    "lime_docs_info": (_i, [_vp, C.POINTER(_u32), _pu64]),
    "lime_docs_device": (_i, [_vp, _pp, _pp]),
    "lime_docs_get": (_i, [_vp, _vp, _vp]),
    "lime_docs_free": (None, [_vp]),
    "lime_docs_norms_dev": (_i, [_vp, _vp, _u32, _vp, _vp]),
    "lime_classify_sample_dev": (_i, [_vp, _u32, _vp, _vp, _vp, _u32, _u32, C.c_float, _i, _i, _u32, _vp, _vp, _vp, _vp]),
    "lime_classify_sample_shards_dev": (_i, [_vp, _u32, _vp, _u32, _vp, _vp, _u32, _u32, C.c_float, _i, _i, _u32, _vp, _vp, _vp, _vp]),
    "lime_seq_cut_dev": (_i, [_vp, _vp, _u64, _i, _u32, _i, _vp, _pu64, _pu64, _pu64]),
    "lime_seq_reader_open": (_i, [_vp, C.c_char_p, _u64, _pp]),
    "lime_seq_reader_open_bytes": (_i, [_vp, _vp, _u64, _i, _u64, _pp]),
    "lime_seq_reader_next": (_i, [_vp, _u32, _pp, _pu64]),
    "lime_seq_reader_info": (_i, [_vp, C.POINTER(_i), _pu64, _pu64, _pu64, _pu64]),
    "lime_seq_reader_close": (None, [_vp]),
    "lime_classify_sample_stream": (_i, [_vp, _u32, _vp, _vp, _vp, _u32, _u32, C.c_float, _i, _i, _u32, _u32, _vp, _vp, _vp, _pu64, _pu64, _vp]),
    "lime_classify_sample_stream_shards": (_i, [_vp, _u32, _vp, _u32, _vp, _vp, _u32, _u32, C.c_float, _i, _i, _u32, _u32, _vp, _vp, _vp, _pu64, _pu64, _vp]),
    "lime_classification_writer_open": (_i, [C.c_char_p, _pp]),
    "lime_classification_writer_append": (_i, [_vp, _u64, _vp, _u32]),
    "lime_classification_writer_close": (_i, [_vp, _i]),
}
# lime_verdict_sink: int (*)(void *user, uint64_t first_read, const lime_verdict_t *verdicts, uint32_t n, const lime_stats_t *stats)
VERDICT_SINK = C.CFUNCTYPE(_i, _vp, _u64, _vp, _u32, C.POINTER(Stats))

_LIB = None


def load():
    """Load liblime_hip.so (importing torch first so both share one HIP runtime)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C lime_amd/csrc` "
                          "(or __graft_entry__.build()); lime_amd has no fallback path")
    try:
        import torch  # noqa: F401  (loads libamdhip64.so.7 that the library binds to)
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc):
    if rc != LIME_OK:
        raise LimeError(rc, load().lime_last_error().decode(errors="replace"))


def check_cls(rc):
    """the host-side read-assignment calls (taxonomy, lime_classify_mem, lime_write_classification) report in lime_classify_error"""
    if rc != LIME_OK:
        raise LimeError(rc, load().lime_classify_error().decode(errors="replace"))


def hip_memcpy_d2d(dst, src, nbytes):
    """device-to-device copy through the HIP runtime torch already loaded (tests: library-owned lists)"""
    hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip.hipMemcpy(dst, src, nbytes, 3)          # hipMemcpyDeviceToDevice
