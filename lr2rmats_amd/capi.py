"""ctypes view of the C-ABI in ``include/lr2rmats_hip.h`` (``libl2r_hip.so``).

This is plumbing for tests, bench.py and the multi-GPU driver; the product
host code is C (``lr2rmats_amd/host``) and links the same library.  There is no
fallback: if the shared library is missing or no GPU is usable, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("L2R_HIP_LIB") or os.path.join(HERE, "lib", "libl2r_hip.so")      # (L2R_HIP_LIB: diagnostics, tools/ab.py compares builds)

INFO_KNOWN, INFO_KNOWN_SITE, INFO_FULL, INFO_REV, INFO_UNREL, INFO_SJ_CHECKED, INFO_SJ_PASS, INFO_ACCEPTED = \
    1, 2, 4, 8, 16, 32, 64, 128
EXF_NOVEL_EXON, EXF_NOVEL_DON, EXF_NOVEL_ACC, EXF_NOVEL_JUNC, EXF_UNREL_JUNC = 1, 2, 4, 8, 16
WANT_RESULTS, WANT_ACCEPTED = 1, 2
N_STAGES = 8
STAGE_NAMES = ["pass_a", "scan_tiles", "classify_fast", "classify_generic", "validate_sj", "scan_accepted",
               "gather_accepted", "reserved"]

EXPORTS = [
    "l2r_abi_version", "l2r_last_error", "l2r_device_count", "l2r_create", "l2r_destroy", "l2r_set_params",
    "l2r_set_outputs", "l2r_set_annotation", "l2r_set_junctions", "l2r_upload_reads", "l2r_run", "l2r_sync", "l2r_run_timed",
    "l2r_result_sizes", "l2r_download", "l2r_download_accepted", "l2r_device_view_get", "l2r_stream", "l2r_classify",
    "l2r_stage_kernel", "l2r_set_annotation_cache", "l2r_annotation_cache_state", "l2r_filter_score", "l2r_filter_select",
    "l2r_debug_counters", "l2r_debug_stamps", "l2r_debug_tile_times", "l2r_upload_index_ms", "l2r_hint_single_run",
    "l2r_xchg_id_bytes", "l2r_xchg_unique_id", "l2r_xchg_create", "l2r_xchg_gather_results", "l2r_xchg_gather_accepted", "l2r_xchg_destroy",
    "l2r_sj_begin", "l2r_sj_add", "l2r_sj_add_rows", "l2r_sj_finish", "l2r_sj_download", "l2r_sj_stats",
    "l2r_sj_begin_tab", "l2r_sj_add_rows_over", "l2r_sj_annotate", "l2r_sj_filter_rows", "l2r_sj_download_tab", "l2r_sj_filter_rows2",
    "l2r_fusion_segments", "l2r_fusion_select", "l2r_fusion_stats",
    "l2r_sort_order", "l2r_sort_stats",
    "l2r_name_order", "l2r_name_stats",
    "l2r_gtf_order", "l2r_gtf_rows_out", "l2r_gtf_stats", "l2r_gtf_check",
    "l2r_bed_begin", "l2r_bed_lines", "l2r_bed_text_out", "l2r_bed_cut", "l2r_bed_stats",
    "l2r_uniq_merge", "l2r_uniq_out", "l2r_uniq_stats",
    "l2r_gtftext_begin", "l2r_gtftext_rows", "l2r_gtftext_blocks", "l2r_gtftext_lines", "l2r_gtftext_out", "l2r_gtftext_stats",
    "l2r_gtftext_anno", "l2r_gtftext_reads", "l2r_gtftext_list", "l2r_gtftext_list_out",
    "l2r_detail_begin", "l2r_detail_rows", "l2r_detail_lines", "l2r_detail_out", "l2r_detail_stats",
    "l2r_summary_begin", "l2r_summary_add", "l2r_summary_finish", "l2r_summary_stats",
    "l2r_novel_begin", "l2r_novel_add", "l2r_novel_finish", "l2r_novel_entries_out", "l2r_novel_names", "l2r_novel_rows_out", "l2r_novel_lines", "l2r_novel_out", "l2r_novel_stats",
]
SJ_E_UNKNOWN_TID = -3

_i32p, _i64p, _u8p, _u32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


class Params(C.Structure):
    _fields_ = [("min_exon", C.c_int32), ("min_intron", C.c_int32), ("max_delet", C.c_int32), ("ss_dis", C.c_int32),
                ("end_dis", C.c_int32), ("full_level", C.c_int32), ("split_trans", C.c_int32), ("use_multi", C.c_int32),
                ("min_sj_cnt", C.c_int32), ("force_strand", C.c_int32), ("single_exon_ovlp_frac", C.c_float)]


class CAnnotation(C.Structure):
    _fields_ = [("n_tx", C.c_int64), ("n_exon", C.c_int64), ("tx_tid", _i32p), ("tx_start", _i32p), ("tx_end", _i32p),
                ("tx_rev", _u8p), ("tx_ex_off", _i64p), ("ex_start", _i32p), ("ex_end", _i32p)]


class CJunctions(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", _i32p), ("don", _i32p), ("acc", _i32p), ("uniq_c", _i32p), ("multi_c", _i32p)]


class CReads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_cigar", C.c_int64), ("tid", _i32p), ("pos", _i32p), ("rev", _u8p),
                ("cig_off", _i64p), ("cig", _u32p), ("first_read_index", C.c_int64), ("cig_summary", _u32p)]


class CResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("ex_cap", C.c_int64), ("n_exons", C.c_int64), ("ex_off", _i64p),
                ("ex_start", _i32p), ("ex_end", _i32p), ("ex_flag", _u8p), ("info", _u32p), ("ref_tx", _i32p)]


class CAccepted(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("ex_cap", C.c_int64), ("n_exons", C.c_int64), ("rec", C.c_void_p),
                ("ex_off", _i64p), ("ex_start", _i32p), ("ex_end", _i32p), ("ex_flag", _u8p)]


class CDeviceView(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_exons", C.c_int64), ("n_accepted", C.c_int64), ("n_accepted_exons", C.c_int64),
                ("ex_off", C.c_void_p), ("ex_start", C.c_void_p), ("ex_end", C.c_void_p), ("ex_flag", C.c_void_p),
                ("info", C.c_void_p), ("ref_tx", C.c_void_p), ("acc_rec", C.c_void_p), ("acc_ex_off", C.c_void_p),
                ("acc_ex_start", C.c_void_p), ("acc_ex_end", C.c_void_p), ("acc_ex_flag", C.c_void_p)]


class CFilterParams(C.Structure):
    _fields_ = [("cov_rate", C.c_float), ("map_qual", C.c_float), ("sec_rat", C.c_float), ("min_intron_n", C.c_int32)]


class CFilterRecords(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_cigar", C.c_int64), ("flag", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p),
                ("l_qseq", C.c_void_p), ("nm", C.c_void_p), ("cig_off", C.c_void_p), ("cig", C.c_void_p)]


class CFusionParams(C.Structure):
    _fields_ = [("ovlp_frac", C.c_float), ("each_cov", C.c_float), ("all_cov", C.c_float), ("dis", C.c_int32)]


class CFilterSpans(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p)]


class CSjParams(C.Structure):
    _fields_ = [("min_intron", C.c_int32), ("pair_only", C.c_int32)]


class CSjGenome(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("seq_off", C.c_void_p), ("bases", C.c_void_p)]


class CSjRecords(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_cigar", C.c_int64), ("flag", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p),
                ("uniq", C.c_void_p), ("cig_off", C.c_void_p), ("cig", C.c_void_p)]


class CSjTable(C.Structure):
    _fields_ = [("cap", C.c_int64), ("n", C.c_int64), ("tid", C.c_void_p), ("don", C.c_void_p), ("acc", C.c_void_p),
                ("uniq_c", C.c_void_p), ("multi_c", C.c_void_p), ("strand", C.c_void_p), ("motif", C.c_void_p)]


class CSjTab(C.Structure):
    _fields_ = CSjTable._fields_ + [("anno", C.c_void_p), ("max_over", C.c_void_p)]


class CSjFilter(C.Structure):
    _fields_ = [("anchor_min", C.c_int32 * 5), ("uniq_min", C.c_int32 * 5), ("all_min", C.c_int32 * 5)]


class CSjFilter2(C.Structure):
    _fields_ = [("dist_min", C.c_int32 * 5), ("n_intron_max", C.c_int32), ("intron_max", C.c_int32 * 8)]


SJ_FILTER_DEFAULTS = ((1, 30, 12, 12, 12), (0, 3, 1, 1, 1), (0, 3, 1, 1, 1))      # anchor, unique, total: STAR's outSJfilter* behind the annotated class
SJ_FILTER2_STAR = ((0, 10, 0, 5, 10), (50000, 100000, 200000))                    # dist_min, intron_max: outSJfilterDistToOtherSJmin, outSJfilterIntronMaxVsReadN


class CSortRecords(C.Structure):
    _fields_ = [("n", C.c_int64), ("flag", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p)]


class CNameRecords(C.Structure):
    _fields_ = [("n", C.c_int64), ("name_off", C.c_void_p), ("names", C.c_void_p)]


class CGtfText(C.Structure):
    _fields_ = [("n_bytes", C.c_int64), ("text", C.c_void_p)]


class CGtfRows(C.Structure):
    _fields_ = [("cap", C.c_int64), ("n", C.c_int64), ("start", C.c_void_p), ("len", C.c_void_p), ("line", C.c_void_p)]


class CBedRecords(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_cigar", C.c_int64), ("flag", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p), ("mapq", C.c_void_p),
                ("cig_off", C.c_void_p), ("cig", C.c_void_p), ("name_off", C.c_void_p), ("names", C.c_void_p)]


class CBedParams(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_off", C.c_void_p), ("ref_names", C.c_void_p), ("color_len", C.c_int32), ("color", C.c_uint8 * 12)]


class CUniqTrans(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("rev", C.c_void_p), ("ex_off", C.c_void_p), ("xs", C.c_void_p), ("xe", C.c_void_p)]


class CGtxParams(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_off", C.c_void_p), ("ref_names", C.c_void_p), ("form", C.c_int32), ("src_len", C.c_int32), ("src", C.c_void_p)]


class CGtxRows(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("rev", C.c_void_p), ("ex_off", C.c_void_p), ("xs", C.c_void_p), ("xe", C.c_void_p),
                ("names_len", C.c_int64), ("names", C.c_void_p), ("gid", C.c_void_p), ("tids", C.c_void_p), ("gname", C.c_void_p), ("tname", C.c_void_p)]


class CGtxBlocks(C.Structure):
    _fields_ = [("m", C.c_int64), ("sel", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p), ("cov", C.c_void_p)]


class CGtxAnno(C.Structure):
    _fields_ = [("n_tx", C.c_int64), ("anno_names_len", C.c_int64), ("anno_names", C.c_void_p), ("tx_gid", C.c_void_p), ("tx_gname", C.c_void_p)]


class CGtxReads(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("names_len", C.c_int64), ("names", C.c_void_p), ("qname", C.c_void_p), ("tid_name", C.c_void_p),
                ("res", C.c_void_p), ("has_sj", C.c_int32), ("split", C.c_int32)]


class CDetailParams(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_off", C.c_void_p), ("ref_names", C.c_void_p), ("n_tx", C.c_int64), ("anno_names_len", C.c_int64),
                ("anno_names", C.c_void_p), ("tx_gid", C.c_void_p), ("tx_gname", C.c_void_p)]


class CDetailReads(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("names_len", C.c_int64), ("names", C.c_void_p), ("qname", C.c_void_p), ("res", C.c_void_p)]


class CTiming(C.Structure):
    _fields_ = [("stage_ms", C.c_float * N_STAGES), ("total_ms", C.c_float), ("iters", C.c_int32)]


def accepted_mask(info: np.ndarray, has_sj: bool, split: bool) -> np.ndarray:
    """Which reads check_trans() hands to novel_T / merge_trans (src/update_gtf.c:943-960), from the other info bits:
    full, not known, has a known site; with a junction table additionally the junction check passed, or -s is set
    (the read then goes on as split pieces).  The engine stores this as INFO_ACCEPTED."""
    cand = (info & (INFO_FULL | INFO_KNOWN | INFO_KNOWN_SITE)) == (INFO_FULL | INFO_KNOWN_SITE)
    if not has_sj:
        return cand
    return cand & (((info & INFO_SJ_PASS) != 0) | bool(split))


ACC_REC_DTYPE = np.dtype([("read_lo", "<u4"), ("read_hi", "<u4"), ("info", "<u4"), ("ref_tx", "<i4")])


def default_params(**kw) -> Params:
    """Defaults of reference src/update_gtf.c:24-35."""
    p = Params(3, 3, 50, 0, 0x7fffffff, 5, 0, 0, 1, 0, 0.80)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_lib = None


def load_library():
    """Load libl2r_hip.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s is missing: build it with `make -C lr2rmats_amd/csrc` (no CPU fallback exists)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.l2r_last_error.restype = C.c_char_p
        lib.l2r_create.restype = C.c_void_p
        lib.l2r_create.argtypes = [C.c_int]
        lib.l2r_destroy.argtypes = [C.c_void_p]
        lib.l2r_stream.restype = C.c_void_p
        lib.l2r_stream.argtypes = [C.c_void_p]
        for name in ("l2r_set_params", "l2r_set_outputs", "l2r_set_annotation", "l2r_set_junctions", "l2r_upload_reads", "l2r_download",
                     "l2r_download_accepted", "l2r_device_view_get"):
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_set_outputs.argtypes = [C.c_void_p, C.c_uint]
        lib.l2r_run.argtypes = [C.c_void_p]
        lib.l2r_sync.argtypes = [C.c_void_p]
        lib.l2r_run_timed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.l2r_result_sizes.argtypes = [C.c_void_p, _i64p, _i64p, _i64p, _i64p]
        lib.l2r_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_set_annotation_cache.argtypes = [C.c_void_p, C.c_char_p]
        lib.l2r_annotation_cache_state.argtypes = [C.c_void_p]
        lib.l2r_filter_score.argtypes = [C.c_void_p] * 7
        lib.l2r_filter_select.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        lib.l2r_fusion_segments.argtypes = [C.c_void_p] * 7
        lib.l2r_fusion_select.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 12
        lib.l2r_fusion_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_hint_single_run.argtypes = [C.c_void_p, C.c_int]
        lib.l2r_upload_index_ms.restype = C.c_float
        lib.l2r_upload_index_ms.argtypes = [C.c_void_p]
        lib.l2r_stage_kernel.restype = C.c_char_p
        lib.l2r_stage_kernel.argtypes = [C.c_void_p, C.c_int]
        for name in ("l2r_sj_add", "l2r_sj_add_rows", "l2r_sj_finish", "l2r_sj_download"):
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_sj_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_sj_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_sj_begin_tab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_sj_add_rows_over.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_sj_annotate.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_sj_filter_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_sj_download_tab.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_sj_filter_rows2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_sort_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_sort_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_name_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_name_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_gtf_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_gtf_rows_out.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_gtf_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_gtf_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_bed_begin.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_bed_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_bed_text_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.l2r_bed_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
        lib.l2r_bed_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_uniq_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_uniq_out.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        lib.l2r_uniq_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_gtftext_begin.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_rows.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_lines.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.l2r_gtftext_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_gtftext_anno.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_reads.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_list.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_gtftext_list_out.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_detail_begin.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_detail_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_detail_lines.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.l2r_detail_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.l2r_detail_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_summary_begin.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_summary_add.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_summary_finish.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_summary_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.l2r_novel_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_novel_add.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_novel_finish.argtypes = [C.c_void_p, C.c_void_p]
        lib.l2r_novel_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.l2r_novel_entries_out.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        lib.l2r_novel_rows_out.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        lib.l2r_novel_lines.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.l2r_novel_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.l2r_novel_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib = lib
    return _lib


class L2RError(RuntimeError):
    pass


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(t)


@dataclass
class Result:
    ex_off: np.ndarray
    ex_start: np.ndarray
    ex_end: np.ndarray
    ex_flag: np.ndarray
    info: np.ndarray
    ref_tx: np.ndarray


@dataclass
class SjTable:
    """The junction table of ``bam2sj``: sorted by (tid, don, acc), one row per junction."""
    tid: np.ndarray
    don: np.ndarray
    acc: np.ndarray
    uniq_c: np.ndarray
    multi_c: np.ndarray
    strand: np.ndarray
    motif: np.ndarray


@dataclass
class SjTab(SjTable):
    """The table of ``sjtab``: SjTable and the annotated flag and the maximum overhang of every row."""
    anno: np.ndarray
    max_over: np.ndarray


SJ_STAT_NAMES = ["rows_made", "rounds", "radix_passes", "rows_in", "rows_out", "k_sj_count", "k_scan_u32 (counts)", "k_sj_fill", "k_sj_hist12",
                 "k_radix_digit_hist<SjRows>", "k_scan_u32 (tile histograms)", "k_radix_scatter<SjRows>", "k_sj_heads + scan", "k_sj_reduce", "k_sj_motif",
                 "rows_dropped", "anno_introns", "k_sj_introns", "k_sj_annotate", "k_sj_keep", "k_scan_u32 (keep flags)", "k_sj_take",
                 "intron sort + reduce", "rows_dropped_near", "acc_radix_passes", "k_radix_keys<SjAccKeyOf>", "acceptor order passes", "k_sj_near_acc",
                 "k_sj_keep_near", "rows_dropped_long"]


SORT_STAT_NAMES = ["rows", "radix_passes", "in_order", "k_radix_keys<SortKeyOf>", "k_radix_digit_hist<SortRows>", "k_scan_u32 (tile histograms)", "k_radix_scatter<SortRows>"]


NAME_STAT_NAMES = ["rows", "groups", "radix_passes", "identity", "route", "mismatches", "k_radix_keys<NameHashOf>", "radix passes (hist + scan + scatter)",
                   "k_name_heads", "k_scan_u32 (heads, sizes)", "k_name_firsts + k_name_sizes + k_name_place"]


GTF_STAT_NAMES = ["bytes", "lines", "rows", "transcripts", "heads", "names_beyond_table", "passes_stage1", "passes_stage2", "identity", "route",
                  "k_gtf_count + k_gtf_starts", "k_gtf_fields", "k_scan_u32 (tiles, kept + transcripts, heads)", "k_gtf_rows + heads + k_gtf_triples",
                  "key kernels + radix passes", "k_gtf_compose", "names"]


def header_define(name: str) -> int:
    """The value of an integer #define of include/lr2rmats_hip.h."""
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lr2rmats_hip.h")).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M).group(1))


def gtf_bytes(text) -> np.ndarray:
    """The bytes of a GTF text as an array, without a copy (an empty text gets one byte to point at)."""
    return np.frombuffer(text, np.uint8) if len(text) else np.zeros(1, np.uint8)


def gtf_check(text: bytes):
    """(in_order, line, counts) of GTF text as ``sort-gtf-check`` sees it (l2r_gtf_check: no context, no GPU): line = the first kept line
    whose key is below its predecessor's (0: none); counts = lines, kept rows, transcript lines, chromosome names.  A text outside the
    domain raises RuntimeError with the engine's message."""
    lib = load_library()
    buf = gtf_bytes(text)
    t = CGtfText(len(text), buf.ctypes.data)
    line = C.c_int64(0)
    counts = np.zeros(4, np.int64)
    rc = lib.l2r_gtf_check(C.byref(t), C.byref(line), counts.ctypes.data)
    if rc < 0:
        raise RuntimeError(lib.l2r_last_error().decode())
    return rc == 0, int(line.value), [int(v) for v in counts]


def pack_names(names):
    """A sequence of byte strings as l2r_name_records wants them: (name_off int64 [n + 1], blob uint8)."""
    names = [bytes(x) for x in names]
    off = np.zeros(len(names) + 1, np.int64)
    if names:
        off[1:] = np.cumsum([len(x) for x in names])
    return off, np.frombuffer(b"".join(names) + b"\0", np.uint8)[:int(off[-1])]


def sort_keys(flag, tid, pos) -> np.ndarray:
    """The 64-bit keys of l2r_sort_order (include/lr2rmats_hip.h), in numpy: what ``sort_order`` sorts by, stably."""
    t = np.asarray(tid, np.int64)
    t = np.where(t < 0, 0x7fffffff, t).astype(np.uint64)
    p = (np.asarray(pos, np.int64) + 1).astype(np.uint32).astype(np.uint64)
    return (t << np.uint64(33)) | (p << np.uint64(1)) | ((np.asarray(flag, np.uint64) >> np.uint64(4)) & np.uint64(1))


BED_STAT_NAMES = ["records", "lines", "bytes", "wave_form", "tiles_lds", "tiles_direct", "route", "guard_intact", "k_bed_measure", "k_scan_u32", "k_bed_write"]


def _bed_params(ref_names, color):
    """(CBedParams, arrays to keep alive) of a sequence of reference names (byte strings) and a colour string."""
    color = bytes(color)
    if len(color) > 12:
        raise ValueError("a colour of %d bytes (at most 12)" % len(color))
    off, blob = pack_names(ref_names)
    keep = blob if blob.size else np.zeros(1, np.uint8)
    return CBedParams(len(off) - 1, off.ctypes.data, keep.ctypes.data, len(color), (C.c_uint8 * 12)(*color)), (off, keep)


def _bed_records(flag, tid, pos, mapq, cigars, names):
    """(CBedRecords, arrays to keep alive).  ``cigars``: (cig_off int64 [n + 1], cig uint32); ``names``: byte strings, or (name_off, blob).
    The offset columns may be windows of larger ones (they need not start at 0)."""
    cig_off, cig = cigars
    name_off, blob = names if isinstance(names, tuple) else pack_names(names)
    a = [np.ascontiguousarray(flag, np.uint16), np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(mapq, np.uint8),
         np.ascontiguousarray(cig_off, np.int64), np.ascontiguousarray(cig, np.uint32), np.ascontiguousarray(name_off, np.int64), np.ascontiguousarray(blob, np.uint8)]
    n, n_cigar = int(a[0].shape[0]), int(a[5].shape[0])
    for k in (5, 7):
        if a[k].size == 0:
            a[k] = np.zeros(1, a[k].dtype)
    return CBedRecords(n, n_cigar, *[x.ctypes.data for x in a]), a


def bed_cut(flag, tid, cigars, names, ref_names, first: int, max_records: int, max_bytes: int, color=b"255,0,0") -> int:
    """l2r_bed_cut (no context, no GPU): how many records from ``first`` one batch of at most ``max_records`` records and ``max_bytes``
    summed line bounds takes (always one).  A record whose bound alone is beyond one batch raises RuntimeError."""
    lib = load_library()
    n = len(flag)
    recs, keep = _bed_records(flag, tid, np.zeros(n, np.int32), np.zeros(n, np.uint8), cigars, names)
    prm, keep2 = _bed_params(ref_names, color)
    take = C.c_int64(0)
    if lib.l2r_bed_cut(C.byref(recs), C.byref(prm), first, max_records, max_bytes, C.byref(take)):
        raise RuntimeError(lib.l2r_last_error().decode())
    return int(take.value)


GTX_PLAIN, GTX_READ = 0, 1
GTX_TILE, GTX_LDS_BYTES = 32, 32768         # L2R_GTX_TILE, L2R_GTX_LDS_BYTES (include/lr2rmats_hip.h)
DETAIL_TILE, DETAIL_LDS_BYTES = 32, 32768   # L2R_DETAIL_TILE, L2R_DETAIL_LDS_BYTES (include/lr2rmats_hip.h)
DETAIL_STAT_NAMES = ["rows", "lines", "bytes", "wave_form", "tiles_lds", "tiles_direct", "route", "guard_intact", "batches", "k_detail_measure", "k_scan_u32", "k_detail_write"]
GTX_STAT_NAMES = ["blocks", "lines", "bytes", "wave_form", "tiles_lds", "tiles_direct", "route", "guard_intact", "batches", "k_gtx_measure", "k_scan_u32", "k_gtx_write",
                  "k_rl_select", "piece_blocks"]
GTX_LIST_ALL, GTX_LIST_KNOWN, GTX_LIST_NOVEL, GTX_LIST_UNRECOG = 0, 1, 2, 3


UNIQ_STAT_NAMES = ["rows", "unique", "clusters", "largest_cluster", "route", "hits_identical", "hits_contained", "hits_single", "end_extensions",
                   "k_uniq_heads + cluster cut", "k_uniq_merge", "k_scan_u32 (list lengths) + k_uniq_take"]


SUMMARY_STAT_NAMES = ["reads", "exons", "adds", "route", "clusters", "largest_cluster", "wave_form",
                      "k_sum_class + k_sum_place + scans", "k_sum_gather", "cluster cut", "k_uniq_merge", "k_uniq_take + k_sum_count"]
SUMMARY_COUNT_NAMES = ["known", "reliable", "unreliable", "unrecognised"]


class CSummaryReads(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("res", C.c_void_p)]


NOVEL_LIST_NAMES = ["exons", "donors", "acceptors", "junctions", "genes", "known_genes"]
NOVEL_STAT_NAMES = (["reads", "offers", "split_reads", "known_reads", "adds", "route", "clusters", "largest_cluster", "entries", "hits", "widened"] +
                    ["items_" + k for k in NOVEL_LIST_NAMES] + ["kept_" + k for k in NOVEL_LIST_NAMES] +
                    ["wave_form", "guard_intact", "selection", "merge", "items", "sort", "heads + sums + compaction", "k_nov_bed_measure", "k_scan_u32 (text)", "k_nov_bed_write"])
NOVEL_GTF, NOVEL_BED = 0, 1


class CNovelParams(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_off", C.c_void_p), ("ref_names", C.c_void_p), ("n_tx", C.c_int64), ("tx_gene", C.c_void_p), ("na_gene", C.c_uint32),
                ("has_sj", C.c_int32), ("src_len", C.c_int32), ("src", C.c_void_p), ("anno_names_len", C.c_int64), ("anno_names", C.c_void_p), ("tx_gid", C.c_void_p),
                ("tx_gname", C.c_void_p)]


class CNovelNameTable(C.Structure):
    _fields_ = [("names_len", C.c_int64), ("names", C.c_void_p), ("qname", C.c_void_p), ("tid_name", C.c_void_p)]


FUSION_STAT_NAMES = ["wave_form", "k_fusion_seg", "k_fusion_select", "k_filter_score", "k_filter_select"]


@dataclass
class Accepted:
    rec: np.ndarray          # structured ACC_REC_DTYPE
    ex_off: np.ndarray
    ex_start: np.ndarray
    ex_end: np.ndarray
    ex_flag: np.ndarray

    @property
    def read_index(self) -> np.ndarray:
        return self.rec["read_lo"].astype(np.int64) | (self.rec["read_hi"].astype(np.int64) << 32)


class Engine:
    """One GPU context (one process per GPU)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.ctx = self.lib.l2r_create(device)
        if not self.ctx:
            raise L2RError(self.lib.l2r_last_error().decode())
        self._keep = {}

    def close(self):
        if self.ctx:
            self.lib.l2r_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise L2RError("rc=%d: %s" % (rc, self.lib.l2r_last_error().decode()))

    def set_params(self, p: Params):
        self._chk(self.lib.l2r_set_params(self.ctx, C.byref(p)))

    def set_outputs(self, want: int):
        """WANT_RESULTS (1) and/or WANT_ACCEPTED (2): include/lr2rmats_hip.h l2r_set_outputs."""
        self._chk(self.lib.l2r_set_outputs(self.ctx, want))

    def set_annotation(self, tx_tid, tx_start, tx_end, tx_rev, tx_ex_off, ex_start, ex_end):
        a = [np.ascontiguousarray(tx_tid, np.int32), np.ascontiguousarray(tx_start, np.int32),
             np.ascontiguousarray(tx_end, np.int32), np.ascontiguousarray(tx_rev, np.uint8),
             np.ascontiguousarray(tx_ex_off, np.int64), np.ascontiguousarray(ex_start, np.int32),
             np.ascontiguousarray(ex_end, np.int32)]
        ca = CAnnotation(len(a[0]), len(a[5]), _ptr(a[0], _i32p), _ptr(a[1], _i32p), _ptr(a[2], _i32p), _ptr(a[3], _u8p),
                         _ptr(a[4], _i64p), _ptr(a[5], _i32p), _ptr(a[6], _i32p))
        self._chk(self.lib.l2r_set_annotation(self.ctx, C.byref(ca)))

    def set_junctions(self, sj):
        if sj is None or len(sj[0]) == 0:
            self._chk(self.lib.l2r_set_junctions(self.ctx, None))
            return
        a = [np.ascontiguousarray(x, np.int32) for x in sj]
        cj = CJunctions(len(a[0]), *[_ptr(x, _i32p) for x in a])
        self._chk(self.lib.l2r_set_junctions(self.ctx, C.byref(cj)))

    # ---- `filter` (include/lr2rmats_hip.h: l2r_filter_score / l2r_filter_select)
    def filter_score(self, flag, tid, pos, l_qseq, nm, cig_off, cig, prm: "CFilterParams", spans=None):
        """(drop, score, intron_n) of every record; spans = (tid, start, end) of the -r transcripts in file order."""
        a = [np.ascontiguousarray(flag, np.uint16), np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(pos, np.int32),
             np.ascontiguousarray(l_qseq, np.int32), np.ascontiguousarray(nm, np.int32), np.ascontiguousarray(cig_off, np.int64),
             np.ascontiguousarray(cig, np.uint32)]
        n = int(a[0].shape[0])
        recs = CFilterRecords(n, int(a[6].shape[0]), *[x.ctypes.data for x in a])
        sp = None
        if spans is not None:
            s = [np.ascontiguousarray(x, np.int32) for x in spans]
            sp = CFilterSpans(int(s[0].shape[0]), *[x.ctypes.data for x in s])
        drop = np.zeros(max(n, 1), np.uint8); score = np.zeros(max(n, 1), np.int32); intron = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.l2r_filter_score(self.ctx, C.byref(recs), C.byref(prm), C.byref(sp) if sp is not None else None,
                                            drop.ctypes.data, score.ctypes.data, intron.ctypes.data))
        return drop[:n], score[:n], intron[:n]

    def filter_select(self, group_off, score, intron_n, prm: "CFilterParams"):
        g = np.ascontiguousarray(group_off, np.int64); s = np.ascontiguousarray(score, np.int32); i = np.ascontiguousarray(intron_n, np.int32)
        ng = int(g.shape[0]) - 1
        win = np.zeros(max(ng, 1), np.int64)
        self._chk(self.lib.l2r_filter_select(self.ctx, ng, g.ctypes.data, s.ctypes.data, i.ctypes.data, C.byref(prm), win.ctypes.data))
        return win[:ng]

    # ---- `fusion` (include/lr2rmats_hip.h: l2r_fusion_segments / l2r_fusion_select)
    def fusion_segments(self, flag, pos, cig_off, cig):
        """(read_start, read_end, ref_start, ref_end, qlen) of every record; the rows of unmapped records are 0."""
        a = [np.ascontiguousarray(flag, np.uint16), np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(cig_off, np.int64),
             np.ascontiguousarray(cig, np.uint32)]
        n = int(a[0].shape[0])
        recs = CFilterRecords(n, int(a[3].shape[0]), a[0].ctypes.data, None, a[1].ctypes.data, None, None, a[2].ctypes.data, a[3].ctypes.data)
        out = [np.zeros(max(n, 1), np.int32) for _ in range(5)]
        self._chk(self.lib.l2r_fusion_segments(self.ctx, C.byref(recs), *[x.ctypes.data for x in out]))
        return tuple(x[:n] for x in out)

    def fusion_select(self, group_off, score, ed, tid, read_start, read_end, ref_start, ref_end, rlen_of_group, prm: "CFusionParams"):
        """(first, second): per group the rows of the two segments of a candidate, or -1, -1."""
        g = np.ascontiguousarray(group_off, np.int64)
        cols = [np.ascontiguousarray(x, np.int32) for x in (score, ed, tid, read_start, read_end, ref_start, ref_end, rlen_of_group)]
        ng = int(g.shape[0]) - 1
        first = np.zeros(max(ng, 1), np.int64); second = np.zeros(max(ng, 1), np.int64)
        self._chk(self.lib.l2r_fusion_select(self.ctx, ng, g.ctypes.data, *[x.ctypes.data for x in cols], C.byref(prm),
                                             first.ctypes.data, second.ctypes.data))
        return first[:ng], second[:ng]

    def fusion_stats(self) -> dict:
        """l2r_fusion_stats: the form of the last fusion_segments, and with L2R_FUSION_TIMING=1 device milliseconds per kernel."""
        out = np.zeros(len(FUSION_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_fusion_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(FUSION_STAT_NAMES, out)}

    # ---- `bam2sj` (include/lr2rmats_hip.h: l2r_sj_begin / _add / _add_rows / _finish / _download)
    def sj_begin(self, min_intron: int = 3, pair_only: bool = True, genome=None, tab: bool = False):
        """``genome``: (seq_off [n_seq + 1] int64, bases uint8) with the sequences in file order, or None (no -g).
        ``tab``: l2r_sj_begin_tab -- the table carries the overhang column (``sj_begin_tab``)."""
        prm = CSjParams(min_intron, 1 if pair_only else 0)
        begin = self.lib.l2r_sj_begin_tab if tab else self.lib.l2r_sj_begin
        self._sj_tab = bool(tab)
        if genome is None:
            self._chk(begin(self.ctx, C.byref(prm), None))
            return
        off = np.ascontiguousarray(genome[0], np.int64); bases = np.ascontiguousarray(genome[1], np.uint8)
        g = CSjGenome(len(off) - 1, off.ctypes.data, bases.ctypes.data)
        self._chk(begin(self.ctx, C.byref(prm), C.byref(g)))

    def sj_begin_tab(self, min_intron: int = 3, pair_only: bool = False, genome=None):
        """The table of ``sjtab``: as sj_begin, with the overhang of every row tracked; sj_finish then returns an SjTab."""
        self.sj_begin(min_intron, pair_only, genome, tab=True)

    def sj_add(self, flag, tid, pos, uniq, cig_off, cig):
        """One batch of records (the columns of l2r_sj_records)."""
        a = [np.ascontiguousarray(flag, np.uint16), np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(pos, np.int32),
             np.ascontiguousarray(uniq, np.uint8), np.ascontiguousarray(cig_off, np.int64), np.ascontiguousarray(cig, np.uint32)]
        r = CSjRecords(int(a[0].shape[0]), int(a[5].shape[0]), *[x.ctypes.data for x in a])
        self._chk(self.lib.l2r_sj_add(self.ctx, C.byref(r)))

    def sj_add_rows(self, tid, don, acc, uniq_c, multi_c):
        """Rows that are counted already: their count columns are summed per junction."""
        a = [np.ascontiguousarray(x, np.int32) for x in (tid, don, acc, uniq_c, multi_c)]
        cj = CJunctions(len(a[0]), *[_ptr(x, _i32p) for x in a])
        self._chk(self.lib.l2r_sj_add_rows(self.ctx, C.byref(cj)))

    def sj_add_rows_over(self, tid, don, acc, uniq_c, multi_c, max_over):
        """Rows of tables that carry the overhang column: counts summed, overhangs by maximum (a table of sj_begin_tab only)."""
        a = [np.ascontiguousarray(x, np.int32) for x in (tid, don, acc, uniq_c, multi_c, max_over)]
        cj = CJunctions(len(a[0]), *[_ptr(x, _i32p) for x in a[:5]])
        self._chk(self.lib.l2r_sj_add_rows_over(self.ctx, C.byref(cj), a[5].ctypes.data))

    def sj_finish(self) -> SjTable:
        """Sort + reduce + motifs, then the table as numpy columns (an SjTab with its nine columns for a table of sj_begin_tab).
        An unknown tid raises L2RError (rc = SJ_E_UNKNOWN_TID)."""
        n = C.c_int64(0)
        self._chk(self.lib.l2r_sj_finish(self.ctx, C.byref(n)))
        m = int(n.value)
        if getattr(self, "_sj_tab", False):
            return self.sj_download_tab(m)
        cols = [np.zeros(max(m, 1), np.int32) for _ in range(5)] + [np.zeros(max(m, 1), np.uint8) for _ in range(2)]
        t = CSjTable(max(m, 1), 0, *[x.ctypes.data for x in cols])
        self._chk(self.lib.l2r_sj_download(self.ctx, C.byref(t)))
        return SjTable(*[x[:m] for x in cols])

    def sj_download_tab(self, n_rows: int) -> SjTab:
        """l2r_sj_download_tab into room for ``n_rows`` rows (what sj_finish / sj_filter_rows reported)."""
        m = max(int(n_rows), 1)
        cols = [np.zeros(m, np.int32) for _ in range(5)] + [np.zeros(m, np.uint8) for _ in range(3)] + [np.zeros(m, np.int32)]
        t = CSjTab(int(n_rows), 0, *[x.ctypes.data for x in cols])
        self._chk(self.lib.l2r_sj_download_tab(self.ctx, C.byref(t)))
        return SjTab(*[x[:int(t.n)] for x in cols])

    def sj_annotate(self, tx_tid, tx_ex_off, ex_start, ex_end) -> None:
        """l2r_sj_annotate (behind sj_finish): rows that are an intron of these transcripts get anno = 1."""
        a = [np.ascontiguousarray(tx_tid, np.int32), np.ascontiguousarray(tx_ex_off, np.int64), np.ascontiguousarray(ex_start, np.int32),
             np.ascontiguousarray(ex_end, np.int32)]
        ca = CAnnotation(len(a[0]), len(a[2]), _ptr(a[0], _i32p), None, None, None, _ptr(a[1], _i64p), _ptr(a[2], _i32p), _ptr(a[3], _i32p))
        self._chk(self.lib.l2r_sj_annotate(self.ctx, C.byref(ca)))

    def sj_filter_rows(self, anchor_min=SJ_FILTER_DEFAULTS[0], uniq_min=SJ_FILTER_DEFAULTS[1], all_min=SJ_FILTER_DEFAULTS[2]) -> SjTab:
        """l2r_sj_filter_rows (behind sj_finish and sj_annotate): the rows that stay, as an SjTab."""
        f = CSjFilter((C.c_int32 * 5)(*[int(v) for v in anchor_min]), (C.c_int32 * 5)(*[int(v) for v in uniq_min]), (C.c_int32 * 5)(*[int(v) for v in all_min]))
        n = C.c_int64(0)
        self._chk(self.lib.l2r_sj_filter_rows(self.ctx, C.byref(f), C.byref(n)))
        return self.sj_download_tab(int(n.value))

    def sj_filter_rows2(self, anchor_min=SJ_FILTER_DEFAULTS[0], uniq_min=SJ_FILTER_DEFAULTS[1], all_min=SJ_FILTER_DEFAULTS[2], dist_min=(0,) * 5,
                        intron_max=()) -> SjTab:
        """l2r_sj_filter_rows2: sj_filter_rows and the intron-size rule (``intron_max``, up to eight lengths) and the distance to the
        nearest other donor and acceptor (``dist_min``); SJ_FILTER2_STAR holds STAR's defaults for the two."""
        f = CSjFilter((C.c_int32 * 5)(*[int(v) for v in anchor_min]), (C.c_int32 * 5)(*[int(v) for v in uniq_min]), (C.c_int32 * 5)(*[int(v) for v in all_min]))
        lens = [int(v) for v in intron_max]
        g = CSjFilter2((C.c_int32 * 5)(*[int(v) for v in dist_min]), len(lens), (C.c_int32 * 8)(*lens[:8]))
        n = C.c_int64(0)
        self._chk(self.lib.l2r_sj_filter_rows2(self.ctx, C.byref(f), C.byref(g), C.byref(n)))
        return self.sj_download_tab(int(n.value))

    def sj_stats(self) -> dict:
        """l2r_sj_stats: counters, and with L2R_SJ_TIMING=1 device milliseconds per kernel."""
        out = np.zeros(len(SJ_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_sj_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(SJ_STAT_NAMES, out)}

    # ---- `sort`, `filter -S` (include/lr2rmats_hip.h: l2r_sort_order / l2r_sort_stats)
    def sort_order(self, flag, tid, pos) -> np.ndarray:
        """order[k] = index of the record at rank k in coordinate order (uint32); records with equal keys keep their input order."""
        a = [np.ascontiguousarray(flag, np.uint16), np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(pos, np.int32)]
        n = int(a[0].shape[0])
        recs = CSortRecords(n, *[x.ctypes.data for x in a])
        order = np.zeros(max(n, 1), np.uint32)
        self._chk(self.lib.l2r_sort_order(self.ctx, C.byref(recs), order.ctypes.data))
        return order[:n]

    def sort_stats(self) -> dict:
        """l2r_sort_stats of the last sort_order: rows, passes run, in_order, and with L2R_SORT_TIMING=1 device milliseconds per kernel."""
        out = np.zeros(len(SORT_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_sort_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(SORT_STAT_NAMES, out)}

    # ---- `sort -n`, `filter -N`, `fusion -N` (include/lr2rmats_hip.h: l2r_name_order / l2r_name_stats)
    def name_order(self, names):
        """(order, n_groups): order[k] = index of the record at rank k in name order (uint32) -- records with one name consecutive, groups by
        first appearance, input order inside a group.  ``names``: a sequence of byte strings, or (name_off, blob) as ``pack_names`` gives."""
        off, blob = names if isinstance(names, tuple) else pack_names(names)
        off = np.ascontiguousarray(off, np.int64)
        blob = np.ascontiguousarray(blob, np.uint8)
        n = int(off.shape[0]) - 1
        keep = blob if blob.size else np.zeros(1, np.uint8)
        recs = CNameRecords(n, off.ctypes.data, keep.ctypes.data)
        order = np.zeros(max(n, 1), np.uint32)
        groups = C.c_int64(0)
        self._chk(self.lib.l2r_name_order(self.ctx, C.byref(recs), order.ctypes.data, C.byref(groups)))
        return order[:n], int(groups.value)

    def name_stats(self) -> dict:
        """l2r_name_stats of the last name_order: rows, groups, passes run, identity, route (0 first seed, 1 second seed, 2 host), mismatching
        pairs on the first seed, and with L2R_SORT_TIMING=1 device milliseconds per kernel."""
        out = np.zeros(len(NAME_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_name_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(NAME_STAT_NAMES, out)}

    # ---- `sort-gtf` (include/lr2rmats_hip.h: l2r_gtf_order / l2r_gtf_rows_out / l2r_gtf_stats)
    def gtf_order(self, text):
        """(start uint64, length uint32, line uint32): the kept lines of GTF text (bytes, several files concatenated) in the order
        update-gtf wants -- by (chromosome rank, start, end) of the last transcript line at or before them, then by line number.
        A text outside the domain raises RuntimeError naming the smallest bad line."""
        buf = gtf_bytes(text)
        t = CGtfText(len(text), buf.ctypes.data)
        n_rows = C.c_int64(0)
        self._chk(self.lib.l2r_gtf_order(self.ctx, C.byref(t), C.byref(n_rows)))
        r = int(n_rows.value)
        start, length, line = np.zeros(max(r, 1), np.uint64), np.zeros(max(r, 1), np.uint32), np.zeros(max(r, 1), np.uint32)
        rows = CGtfRows(r, 0, start.ctypes.data, length.ctypes.data, line.ctypes.data)
        self._chk(self.lib.l2r_gtf_rows_out(self.ctx, C.byref(rows)))
        assert int(rows.n) == r
        return start[:r], length[:r], line[:r]

    def gtf_stats(self) -> dict:
        """l2r_gtf_stats of the last gtf_order: bytes, lines, kept rows, transcript lines, heads sent to the host, names ranked beyond the
        table, passes of both stages, identity, route (0 device, 1 host), with L2R_SORT_TIMING=1 device milliseconds per kernel group,
        and the distinct chromosome names."""
        out = np.zeros(len(GTF_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_gtf_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(GTF_STAT_NAMES, out)}

    # ---- `bam2bed` (include/lr2rmats_hip.h: l2r_bed_begin / _lines / _text_out / _stats)
    def bed_begin(self, ref_names, color=b"255,0,0") -> None:
        """The reference names (byte strings, by tid) and the colour string of the lines that follow."""
        prm, _keep = _bed_params(ref_names, color)
        self._chk(self.lib.l2r_bed_begin(self.ctx, C.byref(prm)))

    def bed_lines(self, flag, tid, pos, mapq, cigars, names) -> bytes:
        """The BED12 text of one batch of records: ``cigars`` = (cig_off int64 [n + 1], cig uint32 words len << 4 | op), ``names`` = byte
        strings or (name_off, blob).  A record outside the domain raises L2RError naming the smallest such record and the kind."""
        recs, _keep = _bed_records(flag, tid, pos, mapq, cigars, names)
        n_lines, n_bytes = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_bed_lines(self.ctx, C.byref(recs), C.byref(n_lines), C.byref(n_bytes)))
        self.bed_n_lines = int(n_lines.value)
        return self.bed_text_out(int(n_bytes.value))

    def bed_text_out(self, cap: int) -> bytes:
        """l2r_bed_text_out into room for ``cap`` bytes: the text of the last bed_lines (L2RError where that failed or cap is too small)."""
        buf = np.zeros(max(int(cap), 1), np.uint8)
        self._chk(self.lib.l2r_bed_text_out(self.ctx, buf.ctypes.data, int(cap)))
        n = int(self.bed_stats()["bytes"])
        return buf[:n].tobytes()

    def bed_stats(self) -> dict:
        """l2r_bed_stats of the last bed_lines: records, lines, bytes, the form of k_bed_measure (0 thread, 1 wave), tiles on the LDS and on
        the direct path, route (0 device, 1 host), guard_intact, and with L2R_BED_TIMING=1 device milliseconds per kernel."""
        out = np.zeros(len(BED_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_bed_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(BED_STAT_NAMES, out)}

    # ---- the GTF text of `bam2gtf` / `unique-gtf` (include/lr2rmats_hip.h: l2r_gtftext_begin / _rows / _blocks / _lines / _out / _stats)
    def gtftext_begin(self, ref_names, source=b"lr2rmats", form=GTX_PLAIN) -> None:
        """The reference names (byte strings, by tid), the source string and the form (GTX_PLAIN, GTX_READ) of the blocks that follow."""
        off, blob = pack_names(ref_names)
        keep = blob if blob.size else np.zeros(1, np.uint8)
        src = np.frombuffer(bytes(source) + b"\0", np.uint8)
        prm = CGtxParams(len(off) - 1, off.ctypes.data, keep.ctypes.data, int(form), len(bytes(source)), src.ctypes.data)
        self._chk(self.lib.l2r_gtftext_begin(self.ctx, C.byref(prm)))

    def gtftext_rows(self, tid, rev, ex_off, xs, xe, names, gid, tids, gname=None, tname=None, n=None) -> None:
        """The transcripts: tid, rev, exons [ex_off[i], ex_off[i + 1]) of xs / xe, the table ``names`` (bytes: NUL-terminated strings) and
        the id columns (byte offsets into it; an array passed twice is sent once).  ``xs`` None: the exon chains of the last run, where
        they lie in HBM (ex_off and xe are not read; ``n`` overrides the transcript count, which must equal the run's reads)."""
        names = np.frombuffer(bytes(names), np.uint8) if not isinstance(names, np.ndarray) else np.ascontiguousarray(names, np.uint8)
        cols = {}

        def col(a, t):
            if a is None:
                return None
            if id(a) not in cols:
                cols[id(a)] = np.ascontiguousarray(a, t)
            return cols[id(a)]
        a = [col(tid, np.int32), col(rev, np.uint8), None if xs is None else col(ex_off, np.int64), None if xs is None else col(xs, np.int32),
             None if xs is None else col(xe, np.int32)]
        ids = [col(gid, np.uint32), col(tids, np.uint32), col(gname, np.uint32), col(tname, np.uint32)]
        n = int(a[0].shape[0]) if n is None else int(n)
        ptr = [None if x is None else (x.ctypes.data if x.size else None) for x in a + ids]
        rows = CGtxRows(n, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], int(names.size), names.ctypes.data if names.size else None, *ptr[5:])
        self._chk(self.lib.l2r_gtftext_rows(self.ctx, C.byref(rows)))

    def gtftext_blocks(self, m=None, sel=None, start=None, end=None, cov=None):
        """The selection: block q is transcript sel[q] (None: q, ``m`` blocks), with the optional overrides.  (n_lines, n_bytes) of its
        text; a block outside the domain raises L2RError (rc=-1) naming the smallest such block and the kind."""
        a = [None if x is None else np.ascontiguousarray(x, np.int32) for x in (sel, start, end, cov)]
        sizes = {int(x.shape[0]) for x in a if x is not None}
        if m is None:
            if len(sizes) != 1:
                raise ValueError("gtftext_blocks: m, or columns of one length")
            m = sizes.pop()
        keep = [np.zeros(1, np.int32) if (x is not None and x.size == 0) else x for x in a]
        blk = CGtxBlocks(int(m), *[None if x is None else x.ctypes.data for x in keep])
        n_lines, n_bytes = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_gtftext_blocks(self.ctx, C.byref(blk), C.byref(n_lines), C.byref(n_bytes)))
        return int(n_lines.value), int(n_bytes.value)

    def gtftext_lines(self, first: int, max_blocks: int = 1 << 20, max_bytes: int = 1 << 30, cap=None, buf=None):
        """One batch from block ``first``: (blocks taken, its text).  ``cap``: the room offered to l2r_gtftext_out (None: the batch's bytes).
        ``buf``: a uint8 array the text is fetched into -- the text is then a view of it, not a copy (tools/bench_gtx.py)."""
        n_taken, n_bytes = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_gtftext_lines(self.ctx, int(first), int(max_blocks), int(max_bytes), C.byref(n_taken), C.byref(n_bytes)))
        if buf is not None:
            self._chk(self.lib.l2r_gtftext_out(self.ctx, buf.ctypes.data, int(buf.size)))
            return int(n_taken.value), buf[:int(n_bytes.value)]
        cap = int(n_bytes.value) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), np.uint8)
        self._chk(self.lib.l2r_gtftext_out(self.ctx, out.ctypes.data, cap))
        return int(n_taken.value), out[:int(n_bytes.value)].tobytes()

    def gtftext_all(self, m: int, max_blocks: int = 1 << 20, max_bytes: int = 1 << 30) -> bytes:
        """The text of the whole selection of ``m`` blocks, batch by batch."""
        out, first = [], 0
        while first < m:
            k, t = self.gtftext_lines(first, max_blocks, max_bytes)
            out.append(t)
            first += k
        return b"".join(out)

    def gtftext_stats(self) -> dict:
        """l2r_gtftext_stats: blocks of the selection, lines and bytes of the last batch, the form of k_gtx_measure (0 thread, 1 wave), tiles
        on the LDS and on the direct path, route (0 device, 1 host), guard_intact, batches, and with L2R_GTX_TIMING=1 device milliseconds
        per kernel."""
        out = np.zeros(len(GTX_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_gtftext_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(GTX_STAT_NAMES, out)}

    # ---- the read lists of `update-gtf -a / -k / -v / -u` (include/lr2rmats_hip.h: l2r_gtftext_anno / _reads / _list / _list_out)
    def gtftext_anno(self, anno_names=b"", tx_gid=(), tx_gname=()) -> None:
        """Behind gtftext_begin with form GTX_READ: the annotation's gene tables, as in detail_begin."""
        anno = np.frombuffer(bytes(anno_names), np.uint8) if not isinstance(anno_names, np.ndarray) else np.ascontiguousarray(anno_names, np.uint8)
        gid, gname = np.ascontiguousarray(tx_gid, np.uint32), np.ascontiguousarray(tx_gname, np.uint32)
        if gid.shape != gname.shape:
            raise ValueError("gtftext_anno: tx_gid and tx_gname of one length")
        a = CGtxAnno(int(gid.size), int(anno.size), anno.ctypes.data if anno.size else None, gid.ctypes.data if gid.size else None, gname.ctypes.data if gname.size else None)
        self._chk(self.lib.l2r_gtftext_anno(self.ctx, C.byref(a)))

    def gtftext_reads(self, tid, names, qname, tid_name=None, res=None, has_sj=False, split=False, n=None) -> None:
        """The classified reads: tid, the table ``names``, ``qname`` and ``tid_name`` (byte offsets; None: qname stands for it) and ``res``,
        a Result (the arrays of a download), which is uploaded; None: the results of the last run where they lie in HBM (``n`` overrides
        the read count, which must equal the run's reads)."""
        names = np.frombuffer(bytes(names), np.uint8) if not isinstance(names, np.ndarray) else np.ascontiguousarray(names, np.uint8)
        tid, qname = np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(qname, np.uint32)
        tn = None if tid_name is None else np.ascontiguousarray(tid_name, np.uint32)
        n = int(tid.shape[0]) if n is None else int(n)
        keep, cres = [], None
        if res is not None:
            a = [np.ascontiguousarray(res.ex_off, np.int64), np.ascontiguousarray(res.ex_start, np.int32), np.ascontiguousarray(res.ex_end, np.int32),
                 np.ascontiguousarray(res.ex_flag, np.uint8), np.ascontiguousarray(res.info, np.uint32), np.ascontiguousarray(res.ref_tx, np.int32)]
            x = int(a[0][-1]) if a[0].size else 0
            keep = [v if v.size else np.zeros(1, v.dtype) for v in a]
            cres = CResult(n, x, x, keep[0].ctypes.data_as(_i64p), keep[1].ctypes.data_as(_i32p), keep[2].ctypes.data_as(_i32p), keep[3].ctypes.data_as(_u8p),
                           keep[4].ctypes.data_as(_u32p), keep[5].ctypes.data_as(_i32p))
        rd = CGtxReads(n, tid.ctypes.data if tid.size else None, int(names.size), names.ctypes.data if names.size else None, qname.ctypes.data if qname.size else None,
                       None if tn is None or not tn.size else tn.ctypes.data, None if cres is None else C.addressof(cres), int(bool(has_sj)), int(bool(split)))
        self._chk(self.lib.l2r_gtftext_reads(self.ctx, C.byref(rd)))

    def gtftext_list(self, which: int):
        """One list (GTX_LIST_*) of the reads: (blocks, n_lines, n_bytes) of its text; a block outside the domain raises L2RError (rc=-1)
        naming the smallest such block of the list and the kind.  gtftext_lines / gtftext_all then give its text."""
        m, n_lines, n_bytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_gtftext_list(self.ctx, int(which), C.byref(m), C.byref(n_lines), C.byref(n_bytes)))
        return int(m.value), int(n_lines.value), int(n_bytes.value)

    def gtftext_list_out(self, m: int):
        """The selection of the last gtftext_list of ``m`` blocks: the columns read, first, count, piece (int32 each)."""
        cols = [np.zeros(max(int(m), 1), np.int32) for _ in range(4)]
        self._chk(self.lib.l2r_gtftext_list_out(self.ctx, *[c.ctypes.data for c in cols]))
        return tuple(c[:int(m)] for c in cols)

    # ---- the detail table of `update-gtf -A` (include/lr2rmats_hip.h: l2r_detail_begin / _rows / _lines / _out / _stats)
    def detail_begin(self, ref_names, anno_names=b"", tx_gid=(), tx_gname=()) -> None:
        """The reference names (byte strings, by tid) and the annotation's gene tables: ``anno_names`` (bytes: NUL-terminated strings) and
        per annotation transcript the byte offsets of its gene id and gene name."""
        off, blob = pack_names(ref_names)
        keep = blob if blob.size else np.zeros(1, np.uint8)
        anno = np.frombuffer(bytes(anno_names), np.uint8) if not isinstance(anno_names, np.ndarray) else np.ascontiguousarray(anno_names, np.uint8)
        gid, gname = np.ascontiguousarray(tx_gid, np.uint32), np.ascontiguousarray(tx_gname, np.uint32)
        if gid.shape != gname.shape:
            raise ValueError("detail_begin: tx_gid and tx_gname of one length")
        prm = CDetailParams(len(off) - 1, off.ctypes.data, keep.ctypes.data, int(gid.size), int(anno.size), anno.ctypes.data if anno.size else None,
                            gid.ctypes.data if gid.size else None, gname.ctypes.data if gname.size else None)
        self._chk(self.lib.l2r_detail_begin(self.ctx, C.byref(prm)))

    def detail_rows(self, tid, names, qname, res=None, n=None) -> int:
        """The reads: tid, the table ``names`` (bytes: NUL-terminated strings), ``qname`` (byte offsets of the read names) and ``res``, a
        Result (the arrays of a download), which is uploaded; None: the results of the last run where they lie in HBM (``n`` overrides the
        row count, which must equal the run's reads).  The bytes of the whole text; a read outside the domain raises L2RError (rc=-1)
        naming the smallest such read and the kind."""
        names = np.frombuffer(bytes(names), np.uint8) if not isinstance(names, np.ndarray) else np.ascontiguousarray(names, np.uint8)
        tid, qname = np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(qname, np.uint32)
        n = int(tid.shape[0]) if n is None else int(n)
        keep, cres = [], None
        if res is not None:
            a = [np.ascontiguousarray(res.ex_off, np.int64), np.ascontiguousarray(res.ex_start, np.int32), np.ascontiguousarray(res.ex_end, np.int32),
                 np.ascontiguousarray(res.ex_flag, np.uint8), np.ascontiguousarray(res.info, np.uint32), np.ascontiguousarray(res.ref_tx, np.int32)]
            x = int(a[0][-1]) if a[0].size else 0
            keep = [v if v.size else np.zeros(1, v.dtype) for v in a]
            cres = CResult(n, x, x, keep[0].ctypes.data_as(_i64p), keep[1].ctypes.data_as(_i32p), keep[2].ctypes.data_as(_i32p), keep[3].ctypes.data_as(_u8p),
                           keep[4].ctypes.data_as(_u32p), keep[5].ctypes.data_as(_i32p))
        rows = CDetailReads(n, tid.ctypes.data if tid.size else None, int(names.size), names.ctypes.data if names.size else None,
                            qname.ctypes.data if qname.size else None, None if cres is None else C.addressof(cres))
        n_bytes = C.c_int64(0)
        self._chk(self.lib.l2r_detail_rows(self.ctx, C.byref(rows), C.byref(n_bytes)))
        return int(n_bytes.value)

    def detail_lines(self, first: int, max_rows: int = 1 << 20, max_bytes: int = 1 << 30, cap=None, buf=None):
        """One batch from read ``first``: (reads taken, its text).  ``cap``: the room offered to l2r_detail_out (None: the batch's bytes).
        ``buf``: a uint8 array the text is fetched into -- the text is then a view of it, not a copy (tools/bench_detail.py)."""
        n_taken, n_bytes = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_detail_lines(self.ctx, int(first), int(max_rows), int(max_bytes), C.byref(n_taken), C.byref(n_bytes)))
        if buf is not None:
            self._chk(self.lib.l2r_detail_out(self.ctx, buf.ctypes.data, int(buf.size)))
            return int(n_taken.value), buf[:int(n_bytes.value)]
        cap = int(n_bytes.value) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), np.uint8)
        self._chk(self.lib.l2r_detail_out(self.ctx, out.ctypes.data, cap))
        return int(n_taken.value), out[:int(n_bytes.value)].tobytes()

    def detail_all(self, n: int, max_rows: int = 1 << 20, max_bytes: int = 1 << 30) -> bytes:
        """The text of all ``n`` rows, batch by batch."""
        out, first = [], 0
        while first < n:
            k, t = self.detail_lines(first, max_rows, max_bytes)
            out.append(t)
            first += k
        return b"".join(out)

    def detail_stats(self) -> dict:
        """l2r_detail_stats: rows, lines and bytes of the last batch, the form of k_detail_measure (0 thread, 1 wave), tiles on the LDS and
        on the direct path, route (0 device, 1 host), guard_intact, batches, and with L2R_DETAIL_TIMING=1 device milliseconds per kernel."""
        out = np.zeros(len(DETAIL_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_detail_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(DETAIL_STAT_NAMES, out)}

    # ---- `unique-gtf` (include/lr2rmats_hip.h: l2r_uniq_merge / _out / _stats)
    def uniq_merge(self, tid, rev, ex_off, xs, xe, force_strand=0, ss_dis=0, end_dis=0x7fffffff, frac=0.8) -> dict:
        """merge_trans over the transcripts (tid, rev, exons [ex_off[i], ex_off[i + 1]) of xs / xe) in input order: a dict of ``merged``,
        ``uniq_of`` (per offer) and ``u_src``, ``u_start``, ``u_end``, ``u_cov`` (per list entry).  -s, -d, -D, -f as the command's."""
        a = [np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(rev, np.uint8), np.ascontiguousarray(ex_off, np.int64),
             np.ascontiguousarray(xs, np.int32), np.ascontiguousarray(xe, np.int32)]
        n = int(a[0].shape[0])
        ptr = [x.ctypes.data if x.size else None for x in a]
        trans = CUniqTrans(n, *ptr)
        prm = Params(3, 3, 50, int(ss_dis), int(end_dis), 5, 0, 0, 1, int(force_strand), float(frac))
        n_unique = C.c_int64(0)
        self._chk(self.lib.l2r_uniq_merge(self.ctx, C.byref(prm), C.byref(trans), C.byref(n_unique)))
        u = int(n_unique.value)
        out = {"merged": np.zeros(n, np.uint8), "uniq_of": np.zeros(n, np.int32)}
        for k in ("u_src", "u_start", "u_end", "u_cov"):
            out[k] = np.zeros(u, np.int32)
        self._chk(self.lib.l2r_uniq_out(self.ctx, *[out[k].ctypes.data if out[k].size else None for k in ("merged", "uniq_of", "u_src", "u_start", "u_end", "u_cov")]))
        return out

    def uniq_stats(self) -> dict:
        """l2r_uniq_stats of the last uniq_merge: rows, unique, clusters, largest cluster, route (0 device, 1 host), hits by kind, end
        extensions, and with L2R_SORT_TIMING=1 device milliseconds per kernel group."""
        out = np.zeros(len(UNIQ_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_uniq_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(UNIQ_STAT_NAMES, out)}

    # ---- the read classes of `update-gtf -y` (include/lr2rmats_hip.h: l2r_summary_begin / _add / _finish / _stats)
    def summary_begin(self, force_strand=0, ss_dis=0, end_dis=0x7fffffff, frac=0.8) -> None:
        """-s, -d, -D, -f as the command's; the accumulators are emptied."""
        prm = Params(3, 3, 50, int(ss_dis), int(end_dis), 5, 0, 0, 1, int(force_strand), float(frac))
        self._chk(self.lib.l2r_summary_begin(self.ctx, C.byref(prm)))

    def summary_add(self, tid, res=None, n=None) -> None:
        """``tid`` of the reads and ``res``, a Result (the arrays of a download), which is uploaded; None: the results of the last run where
        they lie in HBM (``n`` overrides the read count, which must equal the run's reads)."""
        tid = np.ascontiguousarray(tid, np.int32)
        n = int(tid.shape[0]) if n is None else int(n)
        keep, cres = [], None
        if res is not None:
            keep = [np.ascontiguousarray(res.ex_off, np.int64), np.ascontiguousarray(res.ex_start, np.int32), np.ascontiguousarray(res.ex_end, np.int32),
                    np.ascontiguousarray(res.ex_flag, np.uint8), np.ascontiguousarray(res.info, np.uint32), np.ascontiguousarray(res.ref_tx, np.int32)]
            x = int(keep[0][-1]) if keep[0].size else 0
            keep = [a if a.size else np.zeros(1, a.dtype) for a in keep]
            cres = CResult(n, x, x, keep[0].ctypes.data_as(_i64p), keep[1].ctypes.data_as(_i32p), keep[2].ctypes.data_as(_i32p), keep[3].ctypes.data_as(_u8p),
                           keep[4].ctypes.data_as(_u32p), keep[5].ctypes.data_as(_i32p))
        rd = CSummaryReads(n, tid.ctypes.data if tid.size else None, None if cres is None else C.addressof(cres))
        self._chk(self.lib.l2r_summary_add(self.ctx, C.byref(rd)))

    def summary_finish(self) -> list:
        """The eight counts: the reads of the classes known, reliable, unreliable, unrecognised, then their unique transcripts.  A read outside
        the domain raises L2RError (rc=-1) naming the smallest such read and the kind."""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.l2r_summary_finish(self.ctx, out.ctypes.data))
        return [int(v) for v in out]

    def summary_stats(self) -> dict:
        """l2r_summary_stats: reads, exons, adds, route (0 device, 1 host), clusters, largest cluster, the form of k_sum_gather (0 thread, 1
        wave), and with L2R_SORT_TIMING=1 device milliseconds per kernel group."""
        out = np.zeros(len(SUMMARY_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_summary_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(SUMMARY_STAT_NAMES, out)}

    # ---- the novel list of `update-gtf` (include/lr2rmats_hip.h: l2r_novel_begin / _add / _finish / _entries_out / _rows_out / _lines / _out / _stats)
    def novel_begin(self, ref_names, tx_gene, na_gene, has_sj=0, split=0, force_strand=0, ss_dis=0, end_dis=0x7fffffff, frac=0.8, source=None, anno_names=b"", tx_gid=None,
                    tx_gname=None) -> None:
        """The reference names (byte strings, by tid), the gene ordinal of every annotation transcript and NA's, whether a junction table
        was set, and -s, -c, -d, -D, -f as the command's; the accumulators are emptied.  ``source`` with the annotation's gene tables
        (``anno_names``: NUL-terminated strings, ``tx_gid`` / ``tx_gname``: byte offsets per transcript): the updated GTF can be composed."""
        off, blob = pack_names(ref_names)
        keep = blob if blob.size else np.zeros(1, np.uint8)
        tx_gene = np.ascontiguousarray(tx_gene, np.uint32)
        prm = Params(3, 3, 50, int(ss_dis), int(end_dis), 5, int(split), 0, 1, int(force_strand), float(frac))
        src = None if source is None else np.frombuffer(bytes(source) + b"\0", np.uint8)
        an = np.frombuffer(bytes(anno_names) + b"\0", np.uint8)
        gid = np.ascontiguousarray(tx_gid if tx_gid is not None else [], np.uint32)
        gname = np.ascontiguousarray(tx_gname if tx_gname is not None else [], np.uint32)
        np_ = CNovelParams(len(off) - 1, off.ctypes.data, keep.ctypes.data, int(tx_gene.shape[0]), tx_gene.ctypes.data if tx_gene.size else None, int(na_gene), int(has_sj),
                           0 if source is None else len(bytes(source)), None if src is None else src.ctypes.data, len(bytes(anno_names)), an.ctypes.data,
                           gid.ctypes.data if gid.size else None, gname.ctypes.data if gname.size else None)
        self._chk(self.lib.l2r_novel_begin(self.ctx, C.byref(prm), C.byref(np_)))

    def novel_add(self, tid, res=None, n=None) -> None:
        """``tid`` of the reads and ``res``, a Result (the arrays of a download), which is uploaded; None: the results of the last run where
        they lie in HBM (``n`` overrides the read count, which must equal the run's reads)."""
        tid = np.ascontiguousarray(tid, np.int32)
        n = int(tid.shape[0]) if n is None else int(n)
        keep, cres = [], None
        if res is not None:
            keep = [np.ascontiguousarray(res.ex_off, np.int64), np.ascontiguousarray(res.ex_start, np.int32), np.ascontiguousarray(res.ex_end, np.int32),
                    np.ascontiguousarray(res.ex_flag, np.uint8), np.ascontiguousarray(res.info, np.uint32), np.ascontiguousarray(res.ref_tx, np.int32)]
            x = int(keep[0][-1]) if keep[0].size else 0
            keep = [a if a.size else np.zeros(1, a.dtype) for a in keep]
            cres = CResult(n, x, x, keep[0].ctypes.data_as(_i64p), keep[1].ctypes.data_as(_i32p), keep[2].ctypes.data_as(_i32p), keep[3].ctypes.data_as(_u8p),
                           keep[4].ctypes.data_as(_u32p), keep[5].ctypes.data_as(_i32p))
        rd = CSummaryReads(n, tid.ctypes.data if tid.size else None, None if cres is None else C.addressof(cres))
        self._chk(self.lib.l2r_novel_add(self.ctx, C.byref(rd)))

    def novel_finish(self) -> list:
        """The eight counts in the order of summary.txt: genes, entries, 0, exons, sites, junctions, 0, known genes.  A read outside the
        domain raises L2RError (rc=-1) naming the smallest such read and the kind; split-route reads raise rc=-3."""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.l2r_novel_finish(self.ctx, out.ctypes.data))
        return [int(v) for v in out]

    def novel_entries(self) -> dict:
        """src, start, end, cov of the entries of the last novel_finish."""
        u = int(self.novel_stats()["entries"])
        out = {k: np.zeros(u, np.int32) for k in ("src", "start", "end", "cov")}
        self._chk(self.lib.l2r_novel_entries_out(self.ctx, *[out[k].ctypes.data if u else None for k in ("src", "start", "end", "cov")]))
        return out

    def novel_names(self, names, qname, tid_name=None):
        """The names table (bytes: NUL-terminated strings) and per entry the byte offsets of its read name and, or None, its transcript id:
        the updated GTF is measured; (lines, bytes)."""
        tab = np.frombuffer(bytes(names) + b"\0", np.uint8)
        q = np.ascontiguousarray(qname, np.uint32)
        t = None if tid_name is None else np.ascontiguousarray(tid_name, np.uint32)
        nt = CNovelNameTable(len(bytes(names)), tab.ctypes.data, q.ctypes.data if q.size else None, None if t is None or not t.size else t.ctypes.data)
        nl, nb = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_novel_names(self.ctx, C.byref(nt), C.byref(nl), C.byref(nb)))
        return int(nl.value), int(nb.value)

    def novel_rows(self, which: int) -> dict:
        """The kept rows of list ``which`` (0 exons .. 5 known genes): tid, a, b, score, meta."""
        r = int(self.novel_stats()["kept_" + NOVEL_LIST_NAMES[which]])
        out = {k: np.zeros(r, np.int32) for k in ("tid", "a", "b", "score")}
        out["meta"] = np.zeros(r, np.uint8)
        self._chk(self.lib.l2r_novel_rows_out(self.ctx, int(which), *[out[k].ctypes.data if r else None for k in ("tid", "a", "b", "score", "meta")]))
        return out

    def novel_lines(self, which=NOVEL_BED, first=0, max_rows=1 << 20, max_bytes=1 << 30):
        """One batch of text: (rows taken, its bytes)."""
        take, nb = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l2r_novel_lines(self.ctx, int(which), int(first), int(max_rows), int(max_bytes), C.byref(take), C.byref(nb)))
        buf = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.l2r_novel_out(self.ctx, buf.ctypes.data, int(nb.value)))
        return int(take.value), buf[:int(nb.value)].tobytes()

    def novel_text(self, which=NOVEL_BED, max_rows=1 << 20, max_bytes=1 << 30) -> bytes:
        """The whole text, batch by batch; empty where there is no row."""
        n = int(self.novel_stats()["kept_exons" if which == NOVEL_BED else "entries"])
        parts, first = [], 0
        while first < n:
            take, text = self.novel_lines(which, first, max_rows, max_bytes)
            if take < 1:
                raise L2RError("l2r_novel_lines took no row")
            parts.append(text)
            first += take
        return b"".join(parts)

    def novel_stats(self) -> dict:
        """l2r_novel_stats: see include/lr2rmats_hip.h; with L2R_SORT_TIMING=1 device milliseconds per kernel group."""
        out = np.zeros(len(NOVEL_STAT_NAMES), np.float64)
        self._chk(self.lib.l2r_novel_stats(self.ctx, out.ctypes.data, len(out)))
        return {k: float(v) for k, v in zip(NOVEL_STAT_NAMES, out)}

    def set_annotation_cache(self, directory) -> None:
        """Keep the annotation tables on disk under ``directory`` (None: off); see include/lr2rmats_hip.h."""
        self._chk(self.lib.l2r_set_annotation_cache(self.ctx, directory.encode() if directory else None))

    def annotation_cache_state(self) -> int:
        """0 no cache, 1 built and stored, 2 read from the cache (last set_annotation)."""
        return int(self.lib.l2r_annotation_cache_state(self.ctx))

    def upload_reads(self, tid, pos, rev, cig_off, cig, first_read_index: int = 0, cig_summary=None):
        """``cig_summary``: the reader's per-record CIGAR summaries ([N, 3] uint32, ``synth.cigar_summary``; None: the engine walks the CIGARs)."""
        a = [np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(rev, np.uint8),
             np.ascontiguousarray(cig_off, np.int64), np.ascontiguousarray(cig, np.uint32)]
        sm = None if cig_summary is None else np.ascontiguousarray(cig_summary, np.uint32)
        if sm is not None and sm.shape != (len(a[0]), 3):
            raise ValueError("cig_summary: expected shape (n_reads, 3)")
        cr = CReads(len(a[0]), len(a[4]), _ptr(a[0], _i32p), _ptr(a[1], _i32p), _ptr(a[2], _u8p), _ptr(a[3], _i64p),
                    _ptr(a[4], _u32p), first_read_index, _ptr(sm, _u32p) if sm is not None else None)
        self._chk(self.lib.l2r_upload_reads(self.ctx, C.byref(cr)))

    def hint_single_run(self, on: bool = True):
        """Every following upload will be classified once (l2r_hint_single_run): no tile index, the two-kernel pipeline."""
        self._chk(self.lib.l2r_hint_single_run(self.ctx, 1 if on else 0))

    def upload_index_ms(self) -> float:
        """GPU time of the last upload's tile index (k_tile_index), ms."""
        return float(self.lib.l2r_upload_index_ms(self.ctx))

    def run(self):
        self._chk(self.lib.l2r_run(self.ctx))

    def sync(self):
        self._chk(self.lib.l2r_sync(self.ctx))

    def run_timed(self, iters: int) -> dict:
        t = CTiming()
        self._chk(self.lib.l2r_run_timed(self.ctx, iters, C.byref(t)))
        return {"total_ms": float(t.total_ms), "iters": int(t.iters),
                "stage_ms": {STAGE_NAMES[i]: float(t.stage_ms[i]) for i in range(N_STAGES - 1)},
                # the kernel behind every stage for the pipeline the engine chose for these records (slab / classic)
                "kernel_ms": {(self.lib.l2r_stage_kernel(self.ctx, i) or b"").decode(): float(t.stage_ms[i])
                              for i in range(N_STAGES - 1) if self.lib.l2r_stage_kernel(self.ctx, i)}}

    def sizes(self):
        v = [C.c_int64(0) for _ in range(4)]
        self._chk(self.lib.l2r_result_sizes(self.ctx, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def download(self) -> Result:
        n, x, _, _ = self.sizes()
        off = np.zeros(n + 1, np.int64); s = np.zeros(max(x, 1), np.int32); e = np.zeros(max(x, 1), np.int32)
        f = np.zeros(max(x, 1), np.uint8); info = np.zeros(max(n, 1), np.uint32); ref = np.zeros(max(n, 1), np.int32)
        cr = CResult(n, max(x, 1), 0, _ptr(off, _i64p), _ptr(s, _i32p), _ptr(e, _i32p), _ptr(f, _u8p), _ptr(info, _u32p),
                     _ptr(ref, _i32p))
        self._chk(self.lib.l2r_download(self.ctx, C.byref(cr)))
        return Result(off, s[:x], e[:x], f[:x], info[:n], ref[:n])

    def download_accepted(self) -> Accepted:
        _, _, m, x = self.sizes()
        rec = np.zeros(max(m, 1), ACC_REC_DTYPE); off = np.zeros(m + 1, np.int64)
        s = np.zeros(max(x, 1), np.int32); e = np.zeros(max(x, 1), np.int32); f = np.zeros(max(x, 1), np.uint8)
        ca = CAccepted(max(m, 1), max(x, 1), 0, rec.ctypes.data, _ptr(off, _i64p), _ptr(s, _i32p), _ptr(e, _i32p), _ptr(f, _u8p))
        self._chk(self.lib.l2r_download_accepted(self.ctx, C.byref(ca)))
        return Accepted(rec[:m], off, s[:x], e[:x], f[:x])

    def device_view(self) -> CDeviceView:
        v = CDeviceView()
        self._chk(self.lib.l2r_device_view_get(self.ctx, C.byref(v)))
        return v

    def classify(self, reads, params: Optional[Params] = None, first_read_index: int = 0) -> Result:
        """upload + run + sync + download for a ``synth.Reads``-like object."""
        if params is not None:
            self.set_params(params)
        self.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig, first_read_index, getattr(reads, "cig_summary", None))
        self.run()
        self.sync()
        return self.download()
