"""Cases of the GTF block shared by tests/test_gtf_text_cpu.py and tests/test_gpu_gtf_text.py: a generator of column dicts in the form
tests/gtf_text_restatement.py reads, the case file of tests/gtx_dump.hip, and the calls that take a case through capi.Engine."""
import struct

import numpy as np

from tests import gtf_text_restatement as gr

EDGES = [0, 9, 10, 99999, 100000, 999999999, 1000000000, 2147483647]


def make_case(seed, exons, form=gr.PLAIN, refs=(b"chr1", b"chr2", b"chrUn_KI270302v1"), source=b"lr2rmats", name_len=(1, 24), empty_names=0.0, coord_max=250000000):
    """A case of len(exons) transcripts with exons[i] exons each; identity selection, no overrides."""
    rng = np.random.default_rng(seed)
    exons = np.asarray(exons, np.int64)
    n = len(exons)
    ex_off = np.zeros(n + 1, np.int64)
    ex_off[1:] = np.cumsum(exons)
    X = int(ex_off[-1])
    xs, xe = np.zeros(X, np.int32), np.zeros(X, np.int32)
    for i in range(n):
        k = int(exons[i])
        if k:
            # ascending, digit counts mixed: the first coordinates small, then steps of very different size
            steps = rng.integers(1, max(2, coord_max // (2 * k + 1)), 2 * k).astype(np.int64)
            steps[0] = rng.choice([1, 7, 95, 99990, steps[0]])
            c = np.cumsum(steps)
            xs[ex_off[i]:ex_off[i + 1]] = c[0::2]
            xe[ex_off[i]:ex_off[i + 1]] = c[1::2]
    alphabet = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/-", np.uint8)

    def name():
        if rng.random() < empty_names:
            return b""
        return bytes(rng.choice(alphabet, int(rng.integers(name_len[0], name_len[1] + 1))))
    strings = [name() for _ in range(4 * n)]
    if form == gr.PLAIN:
        strings[2 * n:] = [b""] * (2 * n)
    table, ids = gr.pack_table(strings)
    return {"form": form, "source": bytes(source), "refs": [bytes(r) for r in refs], "tid": rng.integers(0, len(refs), n).astype(np.int32),
            "rev": rng.integers(0, 2, n).astype(np.uint8), "ex_off": ex_off, "xs": xs, "xe": xe, "table": table,
            "gid": np.asarray(ids[:n], np.uint32), "tids": np.asarray(ids[n:2 * n], np.uint32), "gname": np.asarray(ids[2 * n:3 * n], np.uint32),
            "tname": np.asarray(ids[3 * n:], np.uint32), "sel": None, "start": None, "end": None, "cov": None, "m": n}


def with_selection(case, sel=None, seed=None, overrides=False):
    """A copy with the selection ``sel`` (None: identity) and, with ``overrides``, start / end / cov columns near the chains' own ends."""
    c = dict(case)
    c["sel"] = None if sel is None else np.asarray(sel, np.int32)
    c["m"] = len(case["tid"]) if sel is None else len(sel)
    if overrides:
        rng = np.random.default_rng(seed)
        t = np.arange(c["m"]) if sel is None else np.asarray(sel, np.int64)
        first, last = np.asarray(case["xs"])[case["ex_off"][t]], np.asarray(case["xe"])[case["ex_off"][t + 1] - 1]
        c["start"] = np.maximum(first.astype(np.int64) - rng.integers(0, 50, c["m"]), 0).astype(np.int32)
        c["end"] = np.minimum(last.astype(np.int64) + rng.integers(0, 50, c["m"]), 2147483647).astype(np.int32)
        c["cov"] = rng.choice([1, 2, 9, 10, 99, 100, 12345], c["m"]).astype(np.int32)
    return c


def case_file(case, first=0, max_blocks=1 << 20, max_bytes=1 << 30, sums_only=0):
    """The case file tests/gtx_dump.hip reads."""
    n, refs = len(case["tid"]), case["refs"]
    ref_off = np.zeros(len(refs) + 1, np.int64)
    ref_off[1:] = np.cumsum([len(r) for r in refs])
    bits = sum(1 << k for k, c in enumerate(("sel", "start", "end", "cov")) if case.get(c) is not None)
    head = struct.pack("<12q", n, len(case["xs"]), len(case["table"]), len(refs), case["form"], len(case["source"]), case["m"], bits, first, max_blocks, max_bytes, sums_only)
    body = [np.asarray(case["tid"], np.int32), np.asarray(case["rev"], np.uint8), np.asarray(case["ex_off"], np.int64), np.asarray(case["xs"], np.int32),
            np.asarray(case["xe"], np.int32), np.frombuffer(case["table"], np.uint8)] + [np.asarray(case[c], np.uint32) for c in ("gid", "tids", "gname", "tname")]
    tail = [np.asarray(case[c], np.int32) for c in ("sel", "start", "end", "cov") if case.get(c) is not None]
    return head + b"".join(a.tobytes() for a in body) + ref_off.tobytes() + b"".join(refs) + case["source"] + b"".join(a.tobytes() for a in tail)


def engine_rows(eng, case):
    read = case["form"] == gr.READ
    eng.gtftext_begin(case["refs"], case["source"], case["form"])
    eng.gtftext_rows(case["tid"], case["rev"], case["ex_off"], case["xs"], case["xe"], case["table"], case["gid"], case["tids"],
                     case["gname"] if read else None, case["tname"] if read else None)


def engine_blocks(eng, case):
    return eng.gtftext_blocks(case["m"], case.get("sel"), case.get("start"), case.get("end"), case.get("cov"))


def engine_text(eng, case, max_blocks=1 << 20, max_bytes=1 << 30):
    """begin, rows, blocks and every batch: (text, n_lines, n_bytes, the stats after the last batch)."""
    engine_rows(eng, case)
    n_lines, n_bytes = engine_blocks(eng, case)
    text = eng.gtftext_all(case["m"], max_blocks, max_bytes)
    return text, n_lines, n_bytes, eng.gtftext_stats()
