// name_dump.hip -- the host side of l2r_name_order (lr2rmats_amd/csrc/l2r_nameorder.hip.h) as a stand-alone host program, for
// tests/test_name_order_cpu.py:
//     name_dump <case file> <output file>
// runs the argument checks and then name_order_host, the exact routine the engine falls back to.  No HIP function is called and no GPU is
// needed; `make -C lr2rmats_amd/csrc name-dump` builds it with ASan + UBSan on the host code.
//
// Case file (little endian): int64 n, int64 name_off[n + 1], then the name bytes (as many as the file holds).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc`, then `order` and
// `n_groups`, or for a rejected case `error`.  The seconds name_order_host took go to stderr (tools/bench_names.py reads them from the
// build without sanitizers, `make -C lr2rmats_amd/csrc name-host`).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_nameorder.hip.h"

using namespace l2r;

static FILE *g_out = nullptr;

static void put(const char *name, const char *type, const void *data, size_t size, int64_t count)
{
    char head[32];
    memset(head, 0, sizeof head);
    snprintf(head, 24, "%s", name);
    snprintf(head + 24, 8, "%s", type);
    fwrite(head, 1, sizeof head, g_out);
    fwrite(&count, 8, 1, g_out);
    if (count) fwrite(data, size, (size_t)count, g_out);
}
static void put_i64(const char *name, int64_t v) { put(name, "<i8", &v, 8, 1); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: name_dump <case file> <output file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0 || n > ((int64_t)1 << 28)) { fprintf(stderr, "name_dump: bad header\n"); return 2; }
    std::vector<int64_t> off((size_t)n + 1);
    if (fread(off.data(), 8, off.size(), f) != off.size()) { fprintf(stderr, "name_dump: short case file\n"); return 2; }
    std::vector<uint8_t> bytes;
    {   uint8_t buf[4096]; size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + k); }
    fclose(f);
    // exactly the bytes the offsets name: a read beyond them is the sanitizer's to report
    std::vector<uint8_t> names(bytes);
    names.shrink_to_fit();

    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 2; }
    std::vector<uint32_t> order((size_t)n);
    uint32_t none_u = 0; uint8_t none_b = 0;
    const l2r_name_records r = {n, off.data(), names.empty() ? &none_b : names.data()};
    int64_t n_groups = -1;
    std::string msg;
    int rc = name_check(&r, n ? order.data() : &none_u, &n_groups, msg);
    if (!rc && n && (off[0] != 0 || off[(size_t)n] > (int64_t)names.size())) rc = name_fail(msg, "name_dump: the offsets reach beyond the bytes of the case file");
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    const auto t0 = std::chrono::steady_clock::now();
    n_groups = name_order_host(n, off.data(), r.names, order.data());
    fprintf(stderr, "name_order_host: %lld records, %lld groups, %.6f s\n", (long long)n, (long long)n_groups,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    put("order", "<u4", order.data(), 4, n);
    put_i64("n_groups", n_groups);
    return fclose(g_out) ? 2 : 0;
}
