"""merge_trans over a list of transcripts (`unique-gtf`, l2r_uniq_merge), restated in plain Python from the rule as
lr2rmats_amd/csrc/l2r_uniqplan.hip.h states it -- not from its code.  A transcript is (tid, rev, [(start, end), ...])."""
import numpy as np

INT_MAX = 0x7fffffff


def columns(trans):
    """tid, rev, ex_off, xs, xe of a list of transcripts."""
    tid = np.asarray([t[0] for t in trans], np.int32)
    rev = np.asarray([t[1] for t in trans], np.uint8)
    ex_off = np.zeros(len(trans) + 1, np.int64)
    ex_off[1:] = np.cumsum([len(t[2]) for t in trans])
    xs = np.asarray([e[0] for t in trans for e in t[2]], np.int32)
    xe = np.asarray([e[1] for t in trans for e in t[2]], np.int32)
    return tid, rev, ex_off, xs, xe


def fraction(s1, e1, s2, e2):
    """The overlap over the shorter exon: a double divide, returned as float."""
    if s1 > e2 or s2 > e1:
        return np.float32(0.0)
    return np.float32(np.float64(min(e1, e2) - max(s1, s2) + 1) / np.float64(min(e1 - s1 + 1, e2 - s2 + 1)))


def chains(a, b, d, D):
    """Two chains of several exons each: 'identical', 'contained' or None."""
    if len(a) == len(b):
        if abs(a[0][0] - b[0][0]) > D or abs(a[-1][1] - b[-1][1]) > D:
            return None
        for i in range(len(a) - 1):
            if abs(a[i][1] - b[i][1]) > d or abs(a[i + 1][0] - b[i + 1][0]) > d:
                return None
        return "identical"
    lg, sh = (a, b) if len(a) > len(b) else (b, a)
    if abs(lg[0][0] - sh[0][0]) > D:
        return None
    found = None
    for i in range(len(lg) - 1):
        # the shorter one's first intron among the longer one's: the first place that fits is the only one tried
        if abs(lg[i][1] - sh[0][1]) <= d and abs(lg[i + 1][0] - sh[1][0]) <= d:
            found = i
            break
    if found is not None:
        i, j = found + 1, 1
        while i + 1 < len(lg) and j + 1 < len(sh):
            if abs(lg[i][1] - sh[j][1]) > d or abs(lg[i + 1][0] - sh[j + 1][0]) > d:
                return None
            i, j = i + 1, j + 1
    if abs(lg[-1][1] - sh[-1][1]) > D:
        return None
    return "contained" if found is not None else None


def judge(t, T, s, d, D, f):
    """The offer t against the entry T (dicts of tid, rev, chain): 'stop', None (skip), 'identical', 'contained' or 'single'."""
    tc, Tc = t["chain"], T["chain"]
    if t["tid"] > T["tid"] or tc[0][0] > Tc[-1][1]:
        return "stop"
    if s and t["rev"] != T["rev"]:
        return None
    if len(tc) == 1 and len(Tc) == 1:
        if abs(tc[0][0] - Tc[0][0]) > D or abs(tc[0][1] - Tc[0][1]) > D:
            return None
        return "single" if fraction(tc[0][0], tc[0][1], Tc[0][0], Tc[0][1]) >= np.float32(f) else None
    if len(tc) > 1 and len(Tc) > 1:
        return chains(tc, Tc, d, D)
    return None


def merge(trans, s=0, d=0, D=INT_MAX, f=0.8):
    """The verdicts: merged, uniq_of per offer; u_src, u_start, u_end, u_cov per list entry; hits by kind and the ends raised."""
    lst, merged, uniq_of = [], [], []
    hits = {"identical": 0, "contained": 0, "single": 0}
    end_ext = 0
    for i, (tid, rev, chain) in enumerate(trans):
        t = {"tid": int(tid), "rev": int(rev) != 0, "chain": [list(map(int, e)) for e in chain]}
        verdict, at = "stop", None
        for k in range(len(lst) - 1, -1, -1):
            v = judge(t, lst[k], s, d, D, f)
            if v is not None:
                verdict, at = v, k
                break
        if verdict == "stop":
            lst.append({"tid": t["tid"], "rev": t["rev"], "chain": [list(e) for e in t["chain"]], "src": i, "cov": 1})
            merged.append(0)
            uniq_of.append(len(lst) - 1)
            continue
        merged.append(1)
        uniq_of.append(at)
        hits[verdict] += 1
        if verdict != "contained":
            T = lst[at]
            T["cov"] += 1
            if t["chain"][0][0] < T["chain"][0][0]:
                T["chain"][0][0] = t["chain"][0][0]
            if t["chain"][-1][1] > T["chain"][-1][1]:
                T["chain"][-1][1] = t["chain"][-1][1]
                end_ext += 1
    return {"merged": np.asarray(merged, np.uint8), "uniq_of": np.asarray(uniq_of, np.int32),
            "u_src": np.asarray([e["src"] for e in lst], np.int32), "u_start": np.asarray([e["chain"][0][0] for e in lst], np.int32),
            "u_end": np.asarray([e["chain"][-1][1] for e in lst], np.int32), "u_cov": np.asarray([e["cov"] for e in lst], np.int32),
            "hits": np.asarray([hits["identical"], hits["contained"], hits["single"]], np.int64), "end_ext": end_ext}


def in_order(trans):
    keys = [(t[0], t[2][0][0]) for t in trans]
    return all(keys[i - 1] <= keys[i] for i in range(1, len(keys)))


def as_list(cols):
    """The transcripts of columns (tid, rev, ex_off, xs, xe) as a list: small cases only."""
    tid, rev, ex_off, xs, xe = cols
    return [(int(tid[i]), int(rev[i]), [(int(xs[k]), int(xe[k])) for k in range(int(ex_off[i]), int(ex_off[i + 1]))]) for i in range(len(tid))]


def heads_columns(cols):
    """heads() of columns in order, by a running maximum over (tid, end) written as tid * 2^32 + end (coordinates are below 2^31)."""
    tid, _rev, ex_off, xs, xe = cols
    if len(tid) == 0:
        return np.zeros(0, np.uint8)
    t = tid.astype(np.int64) * (1 << 32)                       # tid in [-1, 2^31): the product stays inside int64
    start, end = t + xs[ex_off[:-1]], t + xe[ex_off[1:] - 1]
    out = np.ones(len(tid), np.uint8)
    out[1:] = start[1:] > np.maximum.accumulate(end)[:-1]
    return out


def heads(trans):
    """Of input in order: 1 where a transcript starts beyond every earlier end on its chromosome (or is the first of all)."""
    out, reach = [], None
    for i, (tid, _rev, chain) in enumerate(trans):
        start, end = (tid, chain[0][0]), (tid, chain[-1][1])
        out.append(1 if i == 0 or start > reach else 0)
        reach = end if reach is None else max(reach, end)
    return np.asarray(out, np.uint8)
