// text_faults.hip.h -- the `faults` command of detail_dump, lists_dump and gtx_dump: every argument-fault branch of the checks the text
// commands share (text_check_ref_off, text_check_genes, text_check_reads of lr2rmats_amd/csrc/l2r_gtftextplan.hip.h) and every branch of
// batch_cut, each reached through the caller's own check with arguments that are sound but for the one fault.  One line per case on
// stdout, <name>\t<rc>\t<message>, and for a cut that succeeds "take <rows> bytes <sum>" as its message.  tests/test_text_faults_cpu.py
// holds the lines it expects, word for word.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../include/lr2rmats_hip.h"

namespace text_faults {

static void say(const char *name, int rc, const std::string &msg) { printf("%s\t%d\t%s\n", name, rc, msg.c_str()); }

// Reads is l2r_detail_reads or l2r_gtx_reads; check(const Reads *, msg) the caller's check.  Two reads of two exons and of one.
template <typename Reads, typename Check> static void reads(Check check)
{
    int32_t tid[2] = {0, 0}, ref_tx[2] = {-1, -1}, xs[3] = {1, 5, 1}, xe[3] = {2, 6, 2};
    uint32_t qname[2] = {0, 2}, info[2] = {2u << 8, 1u << 8};
    uint8_t names[4] = {'a', 0, 'b', 0}, fl[3] = {0, 0, 0};
    const l2r_result s0 = {2, 3, 3, nullptr, xs, xe, fl, info, ref_tx};
    auto one = [&](const char *name, auto change) {
        int64_t ex_off[3] = {0, 2, 3};
        l2r_result s = s0;
        s.ex_off = ex_off;
        Reads r{};
        r.n = 2; r.tid = tid; r.names_len = 4; r.names = names; r.qname = qname; r.res = &s;
        const Reads *arg = &r;
        change(r, s, arg);
        std::string msg;
        const int rc = check(arg, msg);
        say(name, rc, msg);
    };
    one("reads_sound", [](Reads &, l2r_result &, const Reads *&) {});
    one("reads_run_results", [](Reads &r, l2r_result &, const Reads *&) { r.res = nullptr; });
    one("reads_null", [](Reads &, l2r_result &, const Reads *&arg) { arg = nullptr; });
    one("reads_n_negative", [](Reads &r, l2r_result &, const Reads *&) { r.n = -1; });
    one("reads_n_2p31", [](Reads &r, l2r_result &, const Reads *&) { r.n = (int64_t)1 << 31; });
    one("reads_names_len_negative", [](Reads &r, l2r_result &, const Reads *&) { r.names_len = -1; });
    one("reads_names_len_2p32", [](Reads &r, l2r_result &, const Reads *&) { r.names_len = (int64_t)1 << 32; });
    one("reads_null_names", [](Reads &r, l2r_result &, const Reads *&) { r.names = nullptr; });
    one("reads_null_tid", [](Reads &r, l2r_result &, const Reads *&) { r.tid = nullptr; });
    one("reads_null_qname", [](Reads &r, l2r_result &, const Reads *&) { r.qname = nullptr; });
    one("reads_n_reads_mismatch", [](Reads &, l2r_result &s, const Reads *&) { s.n_reads = 3; });
    one("reads_n_exons_negative", [](Reads &, l2r_result &s, const Reads *&) { s.n_exons = -1; });
    one("reads_n_exons_2p32", [](Reads &, l2r_result &s, const Reads *&) { s.n_exons = (int64_t)1 << 32; });
    one("reads_null_ex_off", [](Reads &, l2r_result &s, const Reads *&) { s.ex_off = nullptr; });
    one("reads_null_info", [](Reads &, l2r_result &s, const Reads *&) { s.info = nullptr; });
    one("reads_null_ref_tx", [](Reads &, l2r_result &s, const Reads *&) { s.ref_tx = nullptr; });
    one("reads_null_ex_start", [](Reads &, l2r_result &s, const Reads *&) { s.ex_start = nullptr; });
    one("reads_null_ex_flag", [](Reads &, l2r_result &s, const Reads *&) { s.ex_flag = nullptr; });
    one("reads_ex_off_starts_at_1", [](Reads &, l2r_result &s, const Reads *&) { s.ex_off[0] = 1; });
    one("reads_ex_off_info_read_0", [](Reads &, l2r_result &s, const Reads *&) { s.ex_off[1] = 1; s.ex_off[2] = 2; s.n_exons = 2; });
    one("reads_ex_off_info_last_read", [](Reads &, l2r_result &s, const Reads *&) { static uint32_t other[2] = {2u << 8, 3u << 8}; s.info = other; });
    one("reads_ex_off_end", [](Reads &, l2r_result &s, const Reads *&) { s.n_exons = 4; });
}

// Genes is l2r_detail_params or l2r_gtx_anno: the four faults of the gene tables
template <typename Genes, typename Check> static void genes(Genes sound, Check check)
{
    auto one = [&](const char *name, auto change) { Genes g = sound; change(g); std::string msg; const int rc = check(&g, msg); say(name, rc, msg); };
    one("genes_sound", [](Genes &) {});
    one("genes_n_tx_negative", [](Genes &g) { g.n_tx = -1; });
    one("genes_n_tx_2p31", [](Genes &g) { g.n_tx = (int64_t)1 << 31; });
    one("genes_names_len_negative", [](Genes &g) { g.anno_names_len = -1; });
    one("genes_names_len_2p32", [](Genes &g) { g.anno_names_len = (int64_t)1 << 32; });
    one("genes_null_names", [](Genes &g) { g.anno_names = nullptr; });
    one("genes_null_gid", [](Genes &g) { g.tx_gid = nullptr; });
    one("genes_null_gname", [](Genes &g) { g.tx_gname = nullptr; });
}

// Params is l2r_detail_params or l2r_gtx_params, `sound` with two reference names: the four faults of the reference-offset table
template <typename Params, typename Check> static void refs(Params sound, Check check)
{
    static const int64_t from_1[3] = {1, 2, 4}, down[3] = {0, 3, 2}, long_name[3] = {0, 2, 2 + 65536}, longest[3] = {0, 2, 2 + 65535};
    auto one = [&](const char *name, auto change) { Params p = sound; change(p); std::string msg; const int rc = check(&p, msg); say(name, rc, msg); };
    one("ref_sound", [](Params &) {});
    one("ref_null_off", [](Params &p) { p.ref_off = nullptr; });
    one("ref_starts_at_1", [](Params &p) { p.ref_off = from_1; });
    one("ref_descends", [](Params &p) { p.ref_off = down; });
    one("ref_name_65536", [](Params &p) { p.ref_off = long_name; });
    one("ref_name_65535_null_names", [](Params &p) { p.ref_off = longest; p.ref_names = nullptr; });
    one("ref_null_names", [](Params &p) { p.ref_names = nullptr; });
}

// cut(len, m, first, max_items, max_bytes, &take, &bytes, msg): the caller's cut
template <typename Cut> static void cuts(Cut cut)
{
    const uint32_t len[5] = {10, 20, 30, 40, 50}, big[3] = {1u << 31, 1u << 31, 7};
    auto one = [&](const char *name, const uint32_t *l, int64_t m, int64_t first, int64_t max_items, int64_t max_bytes, bool null_out = false) {
        int64_t take = -7, bytes = -7;
        std::string msg;
        const int rc = cut(l, m, first, max_items, max_bytes, null_out ? nullptr : &take, &bytes, msg);
        if (!rc) msg = "take " + std::to_string(take) + " bytes " + std::to_string(bytes);
        say(name, rc, msg);
    };
    one("cut_null", len, 5, 0, 9, 1000, true);
    one("cut_first_negative", len, 5, -1, 9, 1000);
    one("cut_first_at_m", len, 5, 5, 9, 1000);
    one("cut_max_items_0", len, 5, 0, 0, 1000);
    one("cut_max_bytes_0", len, 5, 0, 9, 0);
    one("cut_always_one", len, 5, 3, 9, 39);
    one("cut_stop_at_max_bytes", len, 5, 0, 9, 60);
    one("cut_stop_below_max_bytes", len, 5, 0, 9, 59);
    one("cut_stop_at_max_items", len, 5, 1, 2, 1000);
    one("cut_to_the_end", len, 5, 2, 9, 1000);
    one("cut_two_of_2p31", big, 3, 0, 9, (int64_t)1 << 40);
    one("cut_behind_2p31", big, 3, 1, 9, (int64_t)1 << 40);
}

}  // namespace text_faults
