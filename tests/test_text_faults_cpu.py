"""The argument checks and the batch cut that the detail table, the read lists and the GTF text share (text_check_ref_off,
text_check_genes, text_check_reads and batch_cut of lr2rmats_amd/csrc/l2r_gtftextplan.hip.h): one case per fault branch, reached through
each caller's own check by the `faults` command of its dump program (tests/text_faults.hip.h) under ASan + UBSan.  The messages and
return codes below are written out as the entry points gave them before the checks were stated once; they are part of the C-ABI's
behaviour (l2r_last_error) and stay byte for byte."""
import os
import shutil
import subprocess

import pytest

from tests.test_upload_plan_cpu import MARKS, SAN_ENV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def reads_faults(who, noun):
    return {
        "reads_sound": (0, ""),
        "reads_run_results": (0, ""),
        "reads_null": (-2, "[%s] null argument" % who),
        "reads_n_negative": (-2, "[%s] -1 reads (below 2^31)" % who),
        "reads_n_2p31": (-2, "[%s] 2147483648 reads (below 2^31)" % who),
        "reads_names_len_negative": (-2, "[%s] a names table of -1 bytes (at most 2^32 - 1)" % who),
        "reads_names_len_2p32": (-2, "[%s] a names table of 4294967296 bytes (at most 2^32 - 1)" % who),
        "reads_null_names": (-2, "[%s] null names" % who),
        "reads_null_tid": (-2, "[%s] null column" % who),
        "reads_null_qname": (-2, "[%s] null column" % who),
        "reads_n_reads_mismatch": (-2, "[%s] results of 3 reads for 2 %s" % (who, noun)),
        "reads_n_exons_negative": (-2, "[%s] results of -1 exons (at most 2^32 - 1)" % who),
        "reads_n_exons_2p32": (-2, "[%s] results of 4294967296 exons (at most 2^32 - 1)" % who),
        "reads_null_ex_off": (-2, "[%s] null ex_off" % who),
        "reads_null_info": (-2, "[%s] null result column" % who),
        "reads_null_ref_tx": (-2, "[%s] null result column" % who),
        "reads_null_ex_start": (-2, "[%s] null exon column" % who),
        "reads_null_ex_flag": (-2, "[%s] null exon column" % who),
        "reads_ex_off_starts_at_1": (-2, "[%s] ex_off does not start at 0" % who),
        "reads_ex_off_info_read_0": (-2, "[%s] read 0: ex_off gives 1 exons, info 2" % who),
        "reads_ex_off_info_last_read": (-2, "[%s] read 1: ex_off gives 1 exons, info 3" % who),
        "reads_ex_off_end": (-2, "[%s] ex_off ends at 3, the results hold 4 exons" % who),
    }


def genes_faults(who):
    return {
        "genes_sound": (0, ""),
        "genes_n_tx_negative": (-2, "[%s] -1 annotation transcripts (below 2^31)" % who),
        "genes_n_tx_2p31": (-2, "[%s] 2147483648 annotation transcripts (below 2^31)" % who),
        "genes_names_len_negative": (-2, "[%s] an annotation names table of -1 bytes (at most 2^32 - 1)" % who),
        "genes_names_len_2p32": (-2, "[%s] an annotation names table of 4294967296 bytes (at most 2^32 - 1)" % who),
        "genes_null_names": (-2, "[%s] null anno_names" % who),
        "genes_null_gid": (-2, "[%s] null gene column" % who),
        "genes_null_gname": (-2, "[%s] null gene column" % who),
    }


def refs_faults(who):
    return {
        "ref_sound": (0, ""),
        "ref_null_off": (-2, "[%s] null ref_off" % who),
        "ref_starts_at_1": (-2, "[%s] ref_off does not start at 0" % who),
        "ref_descends": (-2, "[%s] ref_off descends at name 1" % who),
        "ref_name_65536": (-2, "[%s] reference name 1 has 65536 bytes (at most 65535)" % who),
        "ref_name_65535_null_names": (-2, "[%s] null ref_names" % who),
        "ref_null_names": (-2, "[%s] null ref_names" % who),
    }


def cut_faults(who, noun):
    return {
        "cut_null": (-2, "[%s] null argument" % who),
        "cut_first_negative": (-2, "[%s] first %s -1 of 5" % (who, noun)),
        "cut_first_at_m": (-2, "[%s] first %s 5 of 5" % (who, noun)),
        "cut_max_items_0": (-2, "[%s] a batch of 0 %ss and 1000 bytes" % (who, noun)),
        "cut_max_bytes_0": (-2, "[%s] a batch of 9 %ss and 0 bytes" % (who, noun)),
        "cut_always_one": (0, "take 1 bytes 40"),                   # lengths 10 20 30 40 50, from 3, max_bytes 39
        "cut_stop_at_max_bytes": (0, "take 3 bytes 60"),            # from 0, max_bytes 60
        "cut_stop_below_max_bytes": (0, "take 2 bytes 30"),         # from 0, max_bytes 59
        "cut_stop_at_max_items": (0, "take 2 bytes 50"),            # from 1, two items
        "cut_to_the_end": (0, "take 3 bytes 120"),
        "cut_two_of_2p31": (0, "take 1 bytes 2147483648"),          # 2^31 2^31 7: the sum would reach 2^32 - 64
        "cut_behind_2p31": (0, "take 2 bytes 2147483655"),
    }


WANT = {
    "detail": {"params_null": (-2, "[l2r_detail_begin] null argument"), **refs_faults("l2r_detail_begin"), **genes_faults("l2r_detail_begin"),
               **reads_faults("l2r_detail_rows", "rows"), **cut_faults("l2r_detail_lines", "row")},
    "lists": {"anno_null": (-2, "[l2r_gtftext_anno] null argument"), **genes_faults("l2r_gtftext_anno"), **reads_faults("l2r_gtftext_reads", "reads")},
    "gtx": {**refs_faults("l2r_gtftext_begin"), **cut_faults("l2r_gtftext_lines", "block"),
            # an argument with two faults reports the one l2r_gtftext_begin has always reported: the null ref_off first, then the form
            # and the source, the walk of ref_off last
            "ref_descends_and_form_2": (-2, "[l2r_gtftext_begin] form 2 (0 plain, 1 read)"),
            "ref_null_off_and_src_len_negative": (-2, "[l2r_gtftext_begin] null ref_off")},
}

_got = {}


def faults_of(stem):
    """The lines of `<stem>_dump faults`, from one build and one run of the program a module."""
    if stem not in _got:
        if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
            pytest.skip("no hipcc")
        r = subprocess.run(["make", "-C", CSRC, stem + "-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        env = dict(os.environ)
        env.update(SAN_ENV)
        r = subprocess.run([os.path.join(ROOT, "lr2rmats_amd", "lib", stem + "_dump"), "faults"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        for m in MARKS:
            assert m not in r.stderr, "sanitizer report\n" + r.stderr.decode(errors="replace")[-3000:]
        assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-1500:])
        lines = [l.split("\t") for l in r.stdout.decode().split("\n")[:-1]]
        _got[stem] = {name: (int(rc), msg) for name, rc, msg in lines}
        assert len(_got[stem]) == len(lines)
    return _got[stem]


@pytest.mark.parametrize("stem,name", [(s, n) for s in sorted(WANT) for n in WANT[s]])
def test_fault_message_and_code(stem, name):
    assert faults_of(stem)[name] == WANT[stem][name]


@pytest.mark.parametrize("stem", sorted(WANT))
def test_every_case_of_the_program_is_expected(stem):
    assert sorted(faults_of(stem)) == sorted(WANT[stem])
