"""Diagnostics: end-to-end wall clock of the C CLI on config-3-like input.
    tools/e2e_time.py [reads = 1000000]
E2E_CMD = update-gtf (default: BAM + GTF in -> GTF/detail/summary/bed out), bam2gtf or unique-gtf (-m b; BAM in -> GTF out).
E2E_RUNS = runs (default 1).  E2E_OTHER_BIN = a second `lr2rmats` binary (a build of another commit, with its own ../lib): the two are
run alternately, E2E_RUNS times each, the outputs are compared, and the medians and the spread (max - min) of both are printed.
E2E_OTHER_ENV = "NAME=value NAME=value": this binary again with these variables set (a route switched off, e.g. L2R_NOVEL_ROUTE=off) -- instead
of a second binary, or with E2E_OTHER_BIN as a third leg ("env"): this build, the other build and this build with the route off, alternately.
E2E_PLAIN = 1: update-gtf writes the updated GTF alone (the pipeline's first call), no -A / -y / -E.
E2E_LISTS = 1: update-gtf also writes the four read lists (-a -k -v -u), and they are compared too."""
import filecmp, os, subprocess, sys, time, tempfile
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lr2rmats_amd import synth, workload, hostlib
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
cmd = os.environ.get("E2E_CMD", "update-gtf")
cfg = dict(workload.CONFIGS['cfg3']); cfg['n_reads'] = N
anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1)
reads = synth.make_reads(anno, N, cfg["n_exons"], cfg["seed"] * 1000)
d = tempfile.mkdtemp(prefix="l2r_e2e_", dir=os.environ.get("TMPDIR", "/tmp"))
bam, gtf = os.path.join(d, "r.bam"), os.path.join(d, "a.gtf")
t0 = time.time(); synth.write_bam(reads, bam); anno.write_gtf(gtf)
print("inputs written in %.1f s: bam %.1f MB, gtf %.1f MB" % (time.time() - t0, os.path.getsize(bam) / 1e6, os.path.getsize(gtf) / 1e6), flush=True)
env = dict(os.environ); env["L2R_TIMING"] = "1"
runs = int(os.environ.get("E2E_RUNS", "1"))
this_bin = hostlib.BIN_PATH if hasattr(hostlib, "BIN_PATH") else os.path.join(os.path.dirname(hostlib.__file__), "bin", "lr2rmats")
bins = [("this", this_bin)] + ([("other", os.environ["E2E_OTHER_BIN"])] if os.environ.get("E2E_OTHER_BIN") else [])
other_env = dict(kv.split("=", 1) for kv in os.environ.get("E2E_OTHER_ENV", "").split())
if other_env:
    bins.append(("other" if len(bins) == 1 else "env", this_bin))
env_tag = bins[-1][0] if other_env else None
plain = bool(os.environ.get("E2E_PLAIN")) and cmd == "update-gtf"
lists = ("all", "known", "novel", "unrec") if os.environ.get("E2E_LISTS") and cmd == "update-gtf" else ()
walls = {tag: [] for tag, _ in bins}
for k in range(runs):
    for tag, exe in bins:
        out = {k_: os.path.join(d, "%s.%s" % (tag, k_)) for k_ in ("gtf", "detail", "summary", "bed") + lists}
        if cmd == "update-gtf":
            more = ["-a", out["all"], "-k", out["known"], "-v", out["novel"], "-u", out["unrec"]] if lists else []
            args, stdout = ["update-gtf", "-l", "3"] + ([] if plain else ["-A", out["detail"], "-y", out["summary"], "-E", out["bed"]]) + more + ["-o", out["gtf"], bam, gtf], None
        elif cmd == "bam2gtf":
            args, stdout = ["bam2gtf", bam], open(out["gtf"], "wb")
        else:
            args, stdout = ["unique-gtf", "-m", "b", "-o", out["gtf"], bam], None
        t0 = time.time()
        r = subprocess.run([exe] + args, env=dict(env, **other_env) if tag == env_tag else env, stdout=stdout, stderr=subprocess.PIPE)
        dt = time.time() - t0
        if stdout:
            stdout.close()
        walls[tag].append(dt)
        if runs == 1 and len(bins) == 1:
            print(r.stderr.decode()[-1500:])
        else:
            print("run", k, tag, " | ".join(l.replace("[timing]", "").strip() for l in r.stderr.decode().splitlines() if l.startswith("[timing]") or "gtf text:" in l or "detail text:" in l or "read lists:" in l or "novel list:" in l))
        print("rc", r.returncode, "%s wall %.2f s for %d reads; outputs:" % (tag, dt, N), {k_: round(os.path.getsize(v) / 1e6, 1) for k_, v in out.items() if os.path.exists(v)}, flush=True)
for tag, _ in bins[1:]:
    print("outputs of %s equal:" % tag, all(filecmp.cmp(os.path.join(d, "this." + k_), os.path.join(d, tag + "." + k_), shallow=False)
                                           for k_ in ("gtf",) + ((("detail", "summary", "bed") if not plain else ()) + lists if cmd == "update-gtf" else ())))
for tag, w in walls.items():
    w = sorted(w)
    print("%s %s: median %.3f s, min %.3f, max %.3f, spread %.3f over %d runs" % (cmd, tag, w[len(w) // 2], w[0], w[-1], w[-1] - w[0], len(w)), flush=True)
