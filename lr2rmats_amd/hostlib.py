"""ctypes view of ``libl2r_host.so`` -- the C host side in its staged form.

``Job.open(argv)`` parses the update-gtf options and reads all inputs (C code),
``job.views()`` exposes the structure-of-arrays the engine consumes as numpy
arrays (zero copy), ``job.finish(result)`` runs the sequential tail and writes
every output file.  Used by the one-process-per-GPU driver (``dist.py``).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List

import numpy as np

from . import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("L2R_HOST_LIB") or os.path.join(HERE, "lib", "libl2r_host.so")      # (L2R_HOST_LIB: the sanitizer tests load libl2r_host_asan.so)
CLI_PATH = os.path.join(HERE, "bin", "lr2rmats")

_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s is missing: build it with `make -C lr2rmats_amd/host`" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.h_job_open.restype = C.c_void_p
        lib.h_job_open.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
        lib.h_job_open2.restype = C.c_void_p
        lib.h_job_open2.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int]
        lib.h_job_open_rank.restype = C.c_void_p
        lib.h_job_open_rank.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]
        lib.h_job_shard.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.h_job_shard.restype = C.c_int
        lib.h_job_shard_blocks.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.h_job_shard_blocks.restype = None
        lib.h_job_views.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.h_job_detail_views.argtypes = [C.c_void_p, C.c_void_p]
        lib.h_job_finish.argtypes = [C.c_void_p, C.c_void_p]
        lib.h_job_finish.restype = C.c_int
        lib.h_job_free.argtypes = [C.c_void_p]
        lib.h_job_part_last_gene.argtypes = [C.c_void_p, C.c_int]
        lib.h_job_part_last_gene.restype = C.c_char_p
        lib.h_job_part_has_first_gene.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
        lib.h_job_part_has_first_gene.restype = C.c_int
        lib.h_records_to_bam.argtypes = [C.c_char_p, C.c_char_p]
        lib.h_records_to_bam.restype = C.c_int
        lib.h_job_needs_all_reads.argtypes = [C.c_void_p]
        lib.h_job_needs_all_reads.restype = C.c_int
        lib.h_job_list_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_char_p]
        lib.h_job_list_rows.restype = C.c_int
        lib.h_job_finish_accepted.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.h_job_finish_accepted.restype = C.c_int
        lib.h_job_finish_part.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]
        lib.h_job_finish_part.restype = C.c_int
        lib.h_job_out_path.argtypes = [C.c_void_p, C.c_int]
        lib.h_job_out_path.restype = C.c_char_p
        lib.h_job_write_summary.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_char_p]
        lib.h_job_write_summary.restype = C.c_int
        lib.h_job_open_outputs.argtypes = [C.c_void_p]
        lib.h_job_set_out_path.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
        lib.h_cigar_summaries.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.h_cigar_summaries.restype = None
        lib.h_read_fasta.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p]
        lib.h_read_fasta.restype = None
        lib.h_fasta_free.argtypes = [C.c_void_p]
        lib.h_fasta_free.restype = None
        lib.h_sj_literal.argtypes = [C.c_int64] + [C.c_void_p] * 10
        lib.h_sj_literal.restype = C.c_int64
        lib.h_sj_source_open.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p]
        lib.h_sj_source_open.restype = C.c_void_p
        lib.h_sj_source_next.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.h_sj_source_next.restype = C.c_int64
        lib.h_sj_source_close.argtypes = [C.c_void_p]
        lib.h_sj_source_close.restype = None
        lib.h_sj_batch_free.argtypes = [C.c_void_p]
        lib.h_sj_batch_free.restype = None
        lib.h_sj_five_ints.argtypes = [C.c_char_p, C.c_void_p]
        lib.h_sj_five_ints.restype = C.c_int
        lib.h_sj_int_list.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
        lib.h_sj_int_list.restype = C.c_int
        lib.h_chroms_free.argtypes = [C.c_void_p]
        lib.h_chroms_free.restype = None
        lib.h_read_records.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_char_p]
        lib.h_read_records.restype = None
        lib.h_records_free.argtypes = [C.c_void_p]
        lib.h_records_free.restype = None
        lib.h_fusion_groups.argtypes = [C.c_void_p] * 5
        lib.h_fusion_groups.restype = C.c_int64
        lib.h_header_coordinate.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.h_header_coordinate.restype = C.c_int64
        lib.h_sort_key.argtypes = [C.c_int32, C.c_int32, C.c_uint32]
        lib.h_sort_key.restype = C.c_uint64
        lib.h_header_grouped.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.h_header_grouped.restype = C.c_int64
        lib.h_name_grouped.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.h_name_grouped.restype = C.c_int64
        lib.h_gtf_write_rows_path.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
        lib.h_gtf_write_rows_path.restype = C.c_int
        lib.h_bed_run_path.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int64)]
        lib.h_bed_run_path.restype = C.c_int
        lib.h_bed_color_ok.argtypes = [C.c_char_p]
        lib.h_bed_color_ok.restype = C.c_int
        _lib = lib
    return _lib


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype) if False else np.frombuffer(
        (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(C.addressof(ptr.contents)), dtype=dtype, count=n)


def cigar_summaries(cig_off, cig) -> np.ndarray:
    """The reader's per-record CIGAR summaries (l2r_reads::cig_summary, [N, 3] uint32) of records that are in memory already: the C loop of
    host/aln_reader.c (``synth.cigar_summary`` is the numpy form of the same rule, which the tests hold this to)."""
    off = np.ascontiguousarray(cig_off, np.int64)
    cg = np.ascontiguousarray(cig, np.uint32)
    out = np.empty((len(off) - 1, 3), np.uint32)
    load_library().h_cigar_summaries(len(off) - 1, off.ctypes.data, cg.ctypes.data, out.ctypes.data)
    return out

# ---- `bam2sj` (host/sj.c): the FASTA reader, the batch-bounded record source and the reference's junction list (no GPU)

class _CFasta(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("seq_off", C.POINTER(C.c_int64)), ("bases", C.POINTER(C.c_uint8)), ("name", C.POINTER(C.c_char_p))]


class _CChroms(C.Structure):
    _fields_ = [("name", C.POINTER(C.c_char_p)), ("n", C.c_int), ("cap", C.c_int), ("n_hdr", C.c_int)]


class _CSjBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("cap", C.c_int64), ("flag", C.POINTER(C.c_uint16)), ("tid", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int32)),
                ("uniq", C.POINTER(C.c_uint8)), ("nh_seen", C.POINTER(C.c_uint8)), ("cig_off", C.POINTER(C.c_int64)), ("cig", C.POINTER(C.c_uint32)),
                ("n_cig", C.c_int64), ("cap_cig", C.c_int64)]


def read_fasta(path: str):
    """(names, seq_off [n + 1] int64, bases uint8): the sequences of a plain or gzip FASTA in FILE order (h_read_fasta)."""
    lib = load_library()
    f = _CFasta()
    lib.h_read_fasta(path.encode(), C.byref(f), b"read_fasta")
    n = int(f.n_seq)
    names = [f.name[i].decode() for i in range(n)]
    off = _arr(f.seq_off, n + 1, np.int64).copy()
    bases = _arr(f.bases, int(off[n]), np.uint8).copy()
    lib.h_fasta_free(C.byref(f))
    return names, off, bases


def sj_five_ints(text: str):
    """A -a / -U / -A list of ``sjtab`` as the command parses it (h_sj_five_ints): five ints, or None where the usage is printed."""
    out = (C.c_int32 * 5)()
    return [int(v) for v in out] if load_library().h_sj_five_ints(text.encode(), out) else None


def sj_int_list(text: str, cap: int = 8):
    """A -m list of ``sjtab`` as the command parses it (h_sj_int_list): 1 to ``cap`` ints, or None where the usage is printed."""
    out = (C.c_int32 * max(cap, 1))()
    k = load_library().h_sj_int_list(text.encode(), out, cap)
    return [int(v) for v in out[:k]] if k > 0 else None


def sj_literal(tid, don, acc, uniq_c, multi_c):
    """Junction rows in record order -> the list the reference's insertion builds (h_sj_literal): five int32 columns."""
    a = [np.ascontiguousarray(x, np.int32) for x in (tid, don, acc, uniq_c, multi_c)]
    n = len(a[0])
    o = [np.zeros(max(n, 1), np.int32) for _ in range(5)]
    m = load_library().h_sj_literal(n, *[x.ctypes.data for x in a], *[x.ctypes.data for x in o])
    return tuple(x[:m] for x in o)


def sj_read_records(path: str, batch: int = 1 << 20):
    """Every record of a SAM / gzip SAM / BAM file through the record source of ``bam2sj``, ``batch`` records at a time:
    dict of flag, tid, pos, uniq, nh_seen, cig_off, cig (concatenated over the batches) and the header's reference names."""
    lib = load_library()
    chr_ = _CChroms()
    src = lib.h_sj_source_open(path.encode(), C.byref(chr_), b"sj_read_records")
    b = _CSjBatch()
    cols = {k: [] for k in ("flag", "tid", "pos", "uniq", "nh_seen", "cig")}
    lens = []
    while lib.h_sj_source_next(src, C.byref(b), batch) > 0:
        n = int(b.n)
        for k, t in (("flag", np.uint16), ("tid", np.int32), ("pos", np.int32), ("uniq", np.uint8), ("nh_seen", np.uint8)):
            cols[k].append(_arr(getattr(b, k), n, t).copy())
        cols["cig"].append(_arr(b.cig, int(b.n_cig), np.uint32).copy())
        lens.append(np.diff(_arr(b.cig_off, n + 1, np.int64)))
    names = [chr_.name[i].decode() for i in range(chr_.n_hdr)]
    lib.h_sj_source_close(src); lib.h_sj_batch_free(C.byref(b)); lib.h_chroms_free(C.byref(chr_))
    dt = dict(flag=np.uint16, tid=np.int32, pos=np.int32, uniq=np.uint8, nh_seen=np.uint8, cig=np.uint32)
    out = {k: (np.concatenate(v) if v else np.zeros(0, dt[k])) for k, v in cols.items()}
    out["cig_off"] = np.concatenate([[0], np.cumsum(np.concatenate(lens) if lens else np.zeros(0, np.int64))]).astype(np.int64)
    out["names"] = names
    return out


# ---- `fusion` (host/fusion.c): the grouping by read name (no GPU)

class _CRecords(C.Structure):
    _fields_ = [("hdr", C.c_void_p), ("hdr_len", C.c_size_t), ("buf", C.c_void_p), ("buf_len", C.c_size_t), ("n", C.c_int64), ("cap", C.c_int64),
                ("rec_off", C.POINTER(C.c_int64)), ("flag", C.POINTER(C.c_uint16)), ("tid", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int32)),
                ("l_qseq", C.POINTER(C.c_int32)), ("nm", C.POINTER(C.c_int32)), ("nm_seen", C.POINTER(C.c_uint8)),
                ("cig_off", C.POINTER(C.c_int64)), ("cig", C.POINTER(C.c_uint32)), ("n_cig", C.c_int64), ("cap_cig", C.c_int64),
                ("as_score", C.POINTER(C.c_int32))]


def fusion_groups(path: str):
    """The records of a SAM / gzip SAM / BAM file as ``fusion`` groups them (h_read_records + h_fusion_groups, query lengths walked on the
    host): dict of rows (record index of every mapped record), group_off, rlen per group, and the records' as_score / nm / flag columns."""
    lib = load_library()
    chr_, r = _CChroms(), _CRecords()
    lib.h_read_records(path.encode(), C.byref(chr_), C.byref(r), b"fusion_groups")
    n = int(r.n)
    rows = np.zeros(n + 1, np.int64); goff = np.zeros(n + 2, np.int64); rlen = np.zeros(n + 1, np.int32)
    g = int(lib.h_fusion_groups(C.byref(r), None, rows.ctypes.data, goff.ctypes.data, rlen.ctypes.data))
    out = dict(rows=rows[:int(goff[g])].copy(), group_off=goff[:g + 1].copy(), rlen=rlen[:g].copy(),
               as_score=_arr(r.as_score, n, np.int32).copy(), nm=_arr(r.nm, n, np.int32).copy(), flag=_arr(r.flag, n, np.uint16).copy())
    lib.h_records_free(C.byref(r)); lib.h_chroms_free(C.byref(chr_))
    return out


# ---- `sort`, `filter -S` (host/sort.c): the header rewrite and the key (no GPU)

HEADER_SO_ROOM = 32


def header_coordinate(block: bytes):
    """The BAM header block (magic, l_text, text, n_ref, references) with SO:coordinate in its @HD line (h_header_coordinate);
    None where the bytes are no such block."""
    lib = load_library()
    out = C.create_string_buffer(len(block) + HEADER_SO_ROOM)
    n = int(lib.h_header_coordinate(block, len(block), out, len(out)))
    return None if n < 0 else out.raw[:n]


def sort_key(tid: int, pos: int, flag: int) -> int:
    """The 64-bit key of one record as the host computes it (h_sort_key; ``sort-check`` walks these)."""
    return int(load_library().h_sort_key(tid, pos, flag))


# ---- `sort -n`, `sort-check -n`, `filter -N`, `fusion -N` (host/sort.c): the header rewrite and the grouping check (no GPU)

HEADER_GO_ROOM = 48


def header_grouped(block: bytes):
    """The BAM header block with SO:unsorted and GO:query in its @HD line (h_header_grouped); None where the bytes are no such block."""
    lib = load_library()
    out = C.create_string_buffer(len(block) + HEADER_GO_ROOM)
    n = int(lib.h_header_grouped(block, len(block), out, len(out)))
    return None if n < 0 else out.raw[:n]


def name_grouped(path: str):
    """(bad, n_groups) of a SAM / gzip SAM / BAM file as ``sort-check -n`` sees it (h_read_records + h_name_grouped): bad = -1 where every
    name's records are consecutive, else the first record whose name was seen in an earlier group; n_groups = runs of one name."""
    lib = load_library()
    chr_, r = _CChroms(), _CRecords()
    lib.h_read_records(path.encode(), C.byref(chr_), C.byref(r), b"name_grouped")
    g = C.c_int64(0)
    bad = int(lib.h_name_grouped(C.byref(r), C.byref(g)))
    lib.h_records_free(C.byref(r)); lib.h_chroms_free(C.byref(chr_))
    return bad, int(g.value)


# ---- `sort-gtf` (host/gtfsort.c): the writer of the ordered rows (no GPU)

def gtf_write_rows(text: bytes, start, length, line, path: str) -> None:
    """The rows (the three columns of ``Engine.gtf_order``) of ``text`` into ``path`` as `sort-gtf` writes them (h_gtf_write_rows): the
    first nine tab-separated columns of every line, missing columns empty."""
    lib = load_library()
    buf = capi.gtf_bytes(text)
    start = np.ascontiguousarray(start, np.uint64)
    length = np.ascontiguousarray(length, np.uint32)
    line = np.ascontiguousarray(line, np.uint32)
    assert start.shape == length.shape == line.shape
    keep = [x if x.size else np.zeros(1, x.dtype) for x in (start, length, line)]
    if lib.h_gtf_write_rows_path(buf.ctypes.data, len(text), int(start.shape[0]), keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, path.encode()):
        raise OSError("h_gtf_write_rows: a row beyond the text, or %s can not be written" % path)


# ---- `bam2bed` (host/bed.c)

def bed_color_ok(text: str) -> bool:
    """Whether ``text`` is a colour of `bam2bed -c`: three decimal numbers 0..255 with commas and nothing else (no GPU)."""
    return bool(load_library().h_bed_color_ok(text.encode()))


def bed_run(in_path: str, out_path: str, color: str = "255,0,0"):
    """`lr2rmats bam2bed -o out_path -c color in_path` in this process (h_bed_run; needs a GPU): (rc, [records, lines, bytes, batches])."""
    counts = (C.c_int64 * 4)()
    rc = load_library().h_bed_run_path(in_path.encode(), color.encode(), out_path.encode(), counts)
    return int(rc), [int(v) for v in counts]


class _CDetailViews(C.Structure):
    _fields_ = [("n_chr", C.c_int32), ("chr", C.POINTER(C.c_char_p)), ("names_len", C.c_int64), ("names", C.c_void_p), ("qname", C.POINTER(C.c_uint32)),
                ("anno_names_len", C.c_int64), ("anno_names", C.c_void_p), ("tx_gid", C.POINTER(C.c_uint32)), ("tx_gname", C.POINTER(C.c_uint32))]


class Job:
    """One ``update-gtf`` invocation: argv = ["update-gtf", options..., in.bam, old.gtf]."""

    def __init__(self, argv: List[str], open_outputs: bool = True, rank: int = 0, world: int = 1):
        """``rank`` / ``world`` > 1: a rank of a one-process-per-GPU run -- for a coordinate-sorted BAM on the partitioned
        route only the rank's chromosome-aligned shard of the records is loaded (``shard()``)."""
        self.lib = load_library()
        args = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        rc = C.c_int(0)
        self._argv_keep = args
        if world > 1:
            self.h = self.lib.h_job_open_rank(len(argv), args, C.byref(rc), 1 if open_outputs else 0, rank, world)
        else:
            self.h = self.lib.h_job_open2(len(argv), args, C.byref(rc), 1 if open_outputs else 0)
        self.exit_code = rc.value
        if not self.h:
            raise SystemExit(self.exit_code or 1)
        self.prm = capi.Params()
        self.anno = capi.CAnnotation()
        self.sj = capi.CJunctions()
        self.reads = capi.CReads()
        self.lib.h_job_views(self.h, C.byref(self.prm), C.byref(self.anno), C.byref(self.sj), C.byref(self.reads))

    def shard(self):
        """(sharded, lo, hi, n_total): with ``sharded`` the read arrays hold the records [lo, hi) of the file only."""
        lo, hi, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        s = self.lib.h_job_shard(self.h, C.byref(lo), C.byref(hi), C.byref(n))
        return int(s), int(lo.value), int(hi.value), int(n.value)

    def shard_blocks(self):
        """shard()[0] == 2: [start block offset, offset in it, end block offset, offset in it, compressed bytes inflated, file size,
        records] of the rank's block range (host/aln_reader.c h_read_alignments_blocks)."""
        info = (C.c_int64 * 8)()
        self.lib.h_job_shard_blocks(self.h, info)
        return [int(x) for x in info[:7]]

    # numpy views (zero copy, valid until close())
    def annotation_arrays(self):
        a = self.anno
        t, e = a.n_tx, a.n_exon
        return dict(tx_tid=_arr(a.tx_tid, t, np.int32), tx_start=_arr(a.tx_start, t, np.int32), tx_end=_arr(a.tx_end, t, np.int32),
                    tx_rev=_arr(a.tx_rev, t, np.uint8), tx_ex_off=_arr(a.tx_ex_off, t + 1, np.int64),
                    ex_start=_arr(a.ex_start, e, np.int32), ex_end=_arr(a.ex_end, e, np.int32))

    def junction_arrays(self):
        s = self.sj
        if s.n == 0:
            return None
        return tuple(_arr(p, s.n, np.int32) for p in (s.tid, s.don, s.acc, s.uniq_c, s.multi_c))

    def read_arrays(self):
        r = self.reads
        # (cig_summary: the reader's per-record CIGAR summaries, l2r_reads::cig_summary; None for `-m g` input)
        sm = _arr(r.cig_summary, 3 * r.n_reads, np.uint32).reshape(-1, 3) if r.cig_summary else None
        return dict(tid=_arr(r.tid, r.n_reads, np.int32), pos=_arr(r.pos, r.n_reads, np.int32), rev=_arr(r.rev, r.n_reads, np.uint8),
                    cig_off=_arr(r.cig_off, r.n_reads + 1, np.int64), cig=_arr(r.cig, r.n_cigar, np.uint32), cig_summary=sm)

    def detail_views(self):
        """What a detail line needs beside the results (capi.Engine.detail_begin / detail_rows): ``refs`` (chromosome names by tid), the
        read-name table ``names`` with ``qname``, the annotation's table ``anno`` with ``tx_gid`` and ``tx_gname`` (copies)."""
        v = _CDetailViews()
        self.lib.h_job_detail_views(self.h, C.byref(v))
        return dict(refs=[v.chr[k] for k in range(v.n_chr)], names=C.string_at(v.names, v.names_len) if v.names else b"", qname=_arr(v.qname, self.reads.n_reads, np.uint32).copy(),
                    anno=C.string_at(v.anno_names, v.anno_names_len) if v.anno_names else b"", tx_gid=_arr(v.tx_gid, self.anno.n_tx, np.uint32).copy(),
                    tx_gname=_arr(v.tx_gname, self.anno.n_tx, np.uint32).copy())

    def finish(self, ex_off, ex_start, ex_end, ex_flag, info, ref_tx) -> int:
        """Sequential tail + writers.  Arrays as in ``capi.Result`` (info carries the exon count in bits 8..31)."""
        n = int(info.shape[0])
        x = int(ex_start.shape[0])
        keep = [np.ascontiguousarray(ex_off, np.int64), np.ascontiguousarray(ex_start, np.int32), np.ascontiguousarray(ex_end, np.int32),
                np.ascontiguousarray(ex_flag, np.uint8), np.ascontiguousarray(info, np.uint32), np.ascontiguousarray(ref_tx, np.int32)]
        res = capi.CResult(n, x, x, keep[0].ctypes.data_as(capi._i64p), keep[1].ctypes.data_as(capi._i32p), keep[2].ctypes.data_as(capi._i32p),
                           keep[3].ctypes.data_as(capi._u8p), keep[4].ctypes.data_as(capi._u32p), keep[5].ctypes.data_as(capi._i32p))
        return self.lib.h_job_finish(self.h, C.byref(res))

    def list_rows(self, which: int, lo: int, hi: int, path: str, ex_off, ex_start, ex_end, ex_flag, info, ref_tx) -> int:
        """Read list ``which`` (capi.GTX_LIST_*) of the reads [lo, hi) by the writer the command falls back on (h_list_rows), appended to
        ``path``.  Arrays as in ``finish``, of the whole input."""
        n, x = int(info.shape[0]), int(ex_start.shape[0])
        keep = [np.ascontiguousarray(ex_off, np.int64), np.ascontiguousarray(ex_start, np.int32), np.ascontiguousarray(ex_end, np.int32),
                np.ascontiguousarray(ex_flag, np.uint8), np.ascontiguousarray(info, np.uint32), np.ascontiguousarray(ref_tx, np.int32)]
        res = capi.CResult(n, x, x, keep[0].ctypes.data_as(capi._i64p), keep[1].ctypes.data_as(capi._i32p), keep[2].ctypes.data_as(capi._i32p),
                           keep[3].ctypes.data_as(capi._u8p), keep[4].ctypes.data_as(capi._u32p), keep[5].ctypes.data_as(capi._i32p))
        return self.lib.h_job_list_rows(self.h, C.byref(res), int(which), int(lo), int(hi), path.encode())

    def needs_all_reads(self) -> bool:
        """An output of this run lists every read (detail.txt, -a / -k / -u, summary.txt)."""
        return bool(self.lib.h_job_needs_all_reads(self.h))

    def finish_accepted(self, read_idx, ex_off, ex_start, ex_end, ex_flag, info, ref_tx) -> int:
        """Tail + writers with the rows of the accepted reads only (input order; read_idx[k] = input index of row k)."""
        n, x = int(info.shape[0]), int(ex_start.shape[0])
        keep = [np.ascontiguousarray(ex_off, np.int64), np.ascontiguousarray(ex_start, np.int32), np.ascontiguousarray(ex_end, np.int32),
                np.ascontiguousarray(ex_flag, np.uint8), np.ascontiguousarray(info, np.uint32), np.ascontiguousarray(ref_tx, np.int32)]
        idx = np.ascontiguousarray(read_idx, np.int64)
        res = capi.CResult(n, x, x, keep[0].ctypes.data_as(capi._i64p), keep[1].ctypes.data_as(capi._i32p), keep[2].ctypes.data_as(capi._i32p),
                           keep[3].ctypes.data_as(capi._u8p), keep[4].ctypes.data_as(capi._u32p), keep[5].ctypes.data_as(capi._i32p))
        return self.lib.h_job_finish_accepted(self.h, C.byref(res), idx.ctypes.data_as(C.POINTER(C.c_int64)))

    # ---- partitioned tail (shards cut at chromosome boundaries; see l2r_host.h h_job_finish_part)
    N_SUMMARY = 16
    OUTPUTS = ("gtf", "bed", "bam_gtf", "detail", "known", "novel", "unrecog", "summary")

    def open_outputs(self) -> None:
        self.lib.h_job_open_outputs(self.h)

    def set_out_path(self, which: int, path: str) -> None:
        self.lib.h_job_set_out_path(self.h, which, path.encode())

    def out_path(self, which: int):
        p = self.lib.h_job_out_path(self.h, which)
        return p.decode() if p else None

    def finish_part(self, lo: int, hi: int, ex_off, ex_start, ex_end, ex_flag, info, ref_tx, suffix: str, stdout_base: str,
                    first_part: bool) -> np.ndarray:
        """Tail + writers for the reads [lo, hi) into "<output><suffix>" files; returns the summary counters."""
        n, x = int(info.shape[0]), int(ex_start.shape[0])
        keep = [np.ascontiguousarray(ex_off, np.int64), np.ascontiguousarray(ex_start, np.int32), np.ascontiguousarray(ex_end, np.int32),
                np.ascontiguousarray(ex_flag, np.uint8), np.ascontiguousarray(info, np.uint32), np.ascontiguousarray(ref_tx, np.int32)]
        res = capi.CResult(n, x, x, keep[0].ctypes.data_as(capi._i64p), keep[1].ctypes.data_as(capi._i32p), keep[2].ctypes.data_as(capi._i32p),
                           keep[3].ctypes.data_as(capi._u8p), keep[4].ctypes.data_as(capi._u32p), keep[5].ctypes.data_as(capi._i32p))
        cnt = np.zeros(self.N_SUMMARY, np.int64)
        self.lib.h_job_finish_part(self.h, lo, hi, C.byref(res), suffix.encode(), stdout_base.encode(), 1 if first_part else 0,
                                   cnt.ctypes.data_as(C.POINTER(C.c_int64)))
        return cnt

    # The two gene lists of summary.txt (genes of the updated transcripts, genes of the known reads) are the one place where
    # the reference looks across a chromosome boundary: the last entry's gene_id is compared before the tid break
    # (l2r_host.h h_part_genes).  After finish_part(): the part's last ids, and whether an id was added under its first tid.
    GENE_COUNTERS = (0, 7)

    def part_last_genes(self):
        out = []
        for q in range(2):
            g = self.lib.h_job_part_last_gene(self.h, q)
            out.append(g.decode() if g is not None else None)
        return out

    def part_has_first_gene(self, which: int, gid) -> bool:
        return gid is not None and bool(self.lib.h_job_part_has_first_gene(self.h, which, gid.encode()))

    def write_summary(self, counters: np.ndarray, path: str) -> None:
        c = np.ascontiguousarray(counters, np.int64)
        self.lib.h_job_write_summary(self.h, c.ctypes.data_as(C.POINTER(C.c_int64)), path.encode())

    def close(self):
        if self.h:
            self.lib.h_job_free(self.h)
            self.h = None


def records_to_bam(in_path: str, out_path: str) -> int:
    """Every alignment record of ``in_path`` (SAM / gzip SAM / BAM) written as a BAM file: the reader, SAM->BAM encoder and
    BGZF writer of ``lr2rmats filter`` without its tests (no GPU)."""
    return load_library().h_records_to_bam(in_path.encode(), out_path.encode())


def run_cli(args, stdout_path=None, cwd=None, env=None) -> subprocess.CompletedProcess:
    """Run the C binary ``lr2rmats <args>`` (needs a GPU for update-gtf / bam2gtf / unique-gtf -m b / filter / bam2sj / sjtab / fusion / sort / bam2bed).
    ``env``: extra environment variables (L2R_CHUNK_READS, L2R_ROUTE, L2R_THREADS ...)."""
    full_env = None
    if env:
        full_env = dict(os.environ)
        full_env.update({k: str(v) for k, v in env.items()})
    if stdout_path:
        with open(stdout_path, "wb") as fh:
            return subprocess.run([CLI_PATH] + list(args), stdout=fh, stderr=subprocess.PIPE, cwd=cwd, env=full_env)
    return subprocess.run([CLI_PATH] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=cwd, env=full_env)
