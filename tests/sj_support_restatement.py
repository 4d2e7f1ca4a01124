"""Restatement of `update-gtf -j` junction support in literal Python: the pin of the engine's four implementations of it.

The three functions of the reference, src/update_gtf.c:
    check_short_sj1      (:589-603)  one junction against the table, a linear scan from the cursor row
    check_short_sj       (:609-627)  the read's cursor row, the Q7 exits, every novel junction
    check_with_short_sj  (:698-709)  the novel-junction map and has_unreliable_junction
and check_trans's loop over them (:938-964): ONE cursor over the reads in input order, which only moves forward.

No search, no directory, no numpy expression: loops over lists.  The reads' exon chains, their novel-junction flags and which reads
are candidates (full, not known, has a known site) come from a classification WITHOUT a table; this file shares nothing with the C
oracle's junction check.  Nothing here imports lr2rmats_amd.
"""

INFO_KNOWN, INFO_KNOWN_SITE, INFO_FULL = 1, 2, 4
INFO_UNREL, INFO_SJ_CHECKED, INFO_SJ_PASS = 0x10, 0x20, 0x40           # oracle/oracle.h
EXF_NOVEL_JUNC, EXF_UNREL_JUNC = 0x08, 0x10


def check_short_sj1(tid, start, end, sj_group, i_start, dis, min_cnt, use_multi):
    """1: some row from i_start on lies within dis of (start, end) and has the count; the scan ends at a later chromosome or at a row whose
    donor is not in front of `end`"""
    i = i_start
    while i < len(sj_group):
        s_tid, s_don, s_acc, s_uniq, s_multi = sj_group[i]
        if s_tid > tid or (s_tid == tid and s_don >= end):
            return 0
        if abs(s_don - start) <= dis and abs(s_acc - end) <= dis:
            sj_cnt = s_uniq + s_multi if use_multi else s_uniq
            if sj_cnt >= min_cnt:
                return 1
        i += 1
    return 0


def check_short_sj(read, sj_map, sj_group, cursor, dis, min_cnt, use_multi):
    """read = dict(tid, start, end, exons [(start, end)], unreliable [0 / 1 per junction]); cursor = [row], moved in place.
    -> (1 supported / 0 not, the cursor row the junctions were looked up from or None)"""
    i = cursor[0]
    while i < len(sj_group):
        s_tid, s_don, s_acc = sj_group[i][0], sj_group[i][1], sj_group[i][2]
        if s_tid < read["tid"] or (s_tid == read["tid"] and s_acc <= read["start"]):
            i += 1
            cursor[0] = i
        elif s_tid > read["tid"] or (s_tid == read["tid"] and s_don >= read["end"]):
            return 0, None
        else:
            ret = 1
            ex = read["exons"]
            for j in range(len(ex) - 1):
                if sj_map[j] == 0 and check_short_sj1(read["tid"], ex[j][1] + 1, ex[j + 1][0] - 1, sj_group, i, dis, min_cnt, use_multi) == 0:
                    read["unreliable"][j] = 1
                    ret = 0
            return ret, i
    return 0, None


def check_with_short_sj(read, novel_junction, sj_group, cursor, dis, min_cnt, use_multi):
    sj_map = [1 - f for f in novel_junction]
    ret, row = check_short_sj(read, sj_map, sj_group, cursor, dis, min_cnt, use_multi)
    read["has_unreliable"] = 1 - ret
    return ret, row


def junction_support(read_tid, base, table, ss_dis=0, min_sj_cnt=1, use_multi=0):
    """base: the classification of the reads without a table (ex_off, ex_start, ex_end, ex_flag, info); table: [(tid, don, acc, uniq, multi)].
    -> per read, in input order: (info & 0x70, [unreliable flag per exon], cursor row of the lookups or None)"""
    out = []
    cursor = [0]
    for r in range(len(read_tid)):
        lo, hi = int(base.ex_off[r]), int(base.ex_off[r + 1])
        exons = [(int(base.ex_start[k]), int(base.ex_end[k])) for k in range(lo, hi)]
        info = int(base.info[r])
        bits, row = 0, None
        read = dict(tid=int(read_tid[r]), start=exons[0][0], end=exons[-1][1], exons=exons, unreliable=[0] * (len(exons) - 1))
        full, known, known_site = info & INFO_FULL, info & INFO_KNOWN, info & INFO_KNOWN_SITE
        if full and not known and known_site and len(table) > 0:                 # check_trans :943-947
            novel = [1 if int(base.ex_flag[k]) & EXF_NOVEL_JUNC else 0 for k in range(lo, hi - 1)]
            ret, row = check_with_short_sj(read, novel, table, cursor, ss_dis, min_sj_cnt, use_multi)
            bits = INFO_SJ_CHECKED | (INFO_SJ_PASS if ret else 0) | (INFO_UNREL if read["has_unreliable"] else 0)
        out.append((bits, read["unreliable"] + [0], row))
    return out


def outcome(bits, unreliable):
    """the words of tests/sj_support_cases.py"""
    if not bits & INFO_SJ_CHECKED:
        return "not_checked"
    if bits & INFO_SJ_PASS:
        return "pass"
    flagged = [k for k, f in enumerate(unreliable) if f]
    return ("fail", flagged) if flagged else "q7"
