"""profiles/mask_template/isa_compare.py <parent.s> <new.s> <resources_parent.txt> <resources_new.txt> [resources.txt]: per kernel of l2r_engine.hip's device code
(hipcc, the Makefile's flags plus --cuda-device-only -S) the opcode sequence of the parent and of this tree, and the figures of
`make resources` (VGPRs, spills, scratch, LDS, occupancy).  One line per kernel: instruction counts, "same sequence" / "same mix" (the same
opcodes in another order) / the opcodes whose counts differ, and the figures where they differ.  Group A = the instances that only ever
hold 32-bit masks (k_classify_fast, k_probe_slab, k_tile without WIDE), group B = the 64-bit and chunked ones."""
import collections
import re
import subprocess
import sys


def kernels(path):
    out, name, ops = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, ops = m.group(1), []
            continue
        if name is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            out[name] = ops
            name = None
        elif t and not t.startswith((".", ";", "//")) and not t.endswith(":"):
            ops.append(t.split()[0])
    return out


def resources(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def group(demangled):
    if "k_classify_fast" in demangled or re.search(r"k_probe_slab<", demangled):
        return "A"
    if "k_tile<" in demangled:                                   # k_tile<LEVEL, DIS, ACC, WIDE, EXACT>
        args = demangled[demangled.index("k_tile<") + 7:].split(">")[0].split(", ")
        return "B" if args[3] in ("true", "1") else "A"
    if re.search(r"k_probe_slab_wide|k_probe_slab_chunked|k_tile_chunk", demangled):
        return "B"
    return "-"


FIGURES = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize", "LDS Size", "Occupancy")


def main():
    kp, kn = kernels(sys.argv[1]), kernels(sys.argv[2])
    rp, rn = resources(sys.argv[3]), resources(sys.argv[4])
    if len(sys.argv) > 5:                                        # both resource reports, one line per kernel (the reports themselves are 2000 lines each)
        with open(sys.argv[5], "w") as f:
            f.write("# kernel: " + " / ".join(FIGURES) + ", parent | new\n")
            for k in rp:
                f.write("%s: %s | %s\n" % (k, " / ".join(str(rp[k].get(x)) for x in FIGURES), " / ".join(str(rn.get(k, {}).get(x)) for x in FIGURES)))
    names = [k for k in kp if k in rp]
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    print("kernels: parent %d, new %d, in both %d" % (len(rp), len(rn), len(set(rp) & set(rn))))
    for k in sorted(set(rp) ^ set(rn)):
        print("ONLY IN ONE:", k)
    tally = collections.Counter()
    for k in names:
        if k not in kn:
            continue
        short = re.sub(r"^void l2r::", "", dem[k]).split("(")[0]
        g = group(dem[k])
        a, b = kp[k], kn[k]
        if a == b:
            verdict = "same sequence"
        elif collections.Counter(a) == collections.Counter(b):
            verdict = "same mix"
        else:
            ca, cb = collections.Counter(a), collections.Counter(b)
            verdict = str({o: (ca[o], cb[o]) for o in sorted(set(ca) | set(cb)) if ca[o] != cb[o]})
        res = "figures same" if rp[k] == rn[k] else "FIGURES " + str({f: (rp[k][f], rn[k].get(f)) for f in rp[k] if rp[k][f] != rn[k].get(f)})
        tally[(g, verdict if verdict.startswith("same") else "differs", res.split(" ")[0])] += 1
        if g != "-" or verdict != "same sequence" or res != "figures same":
            print("%s %s %d %d %s; %s; VGPRs %d occupancy %d" % (g, short, len(a), len(b), verdict, res, rn[k]["VGPRs"], rn[k]["Occupancy"]))
    print()
    for key in sorted(tally):
        print("group %s: %-14s %-8s %d kernels" % (key + (tally[key],)))


main()
