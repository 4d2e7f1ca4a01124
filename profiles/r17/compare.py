"""profiles/r17/compare.py <dir>: the outputs <tool>_<round>_<parent|new>.txt of tools/bench_sort.py and tools/bench_sj.py in <dir> -> comparison.md:
per kernel the parent library's runs with their min - max, the new library's runs with their median, and whether the median lies inside."""
import glob, json, re, statistics as S, sys
d = sys.argv[1]
def parse(path):
    out, sec = {}, None
    for l in open(path, errors='replace'):
        m = re.match(r'\| kernel ?(\([^)]*\))? \|', l)
        if m: sec = (m.group(1) or '(plain leg)'); continue
        m = re.match(r'\| (.+?) \| ([0-9.]+) \|$', l.strip())
        if m and sec: out[(sec, m.group(1))] = float(m.group(2)); continue
        if l.startswith('{'):
            j = json.loads(l)
            tag = sec or j.get('form') or j.get('leg') or 'line'
            for k in ('call_s_median', 'wall_s_median'):
                if k in j: out[(sec or tag, 'whole call, median of its rounds (ms)')] = j[k] * 1e3
            for k in ('radix_passes', 'acc_radix_passes'):
                if k in j: out[(sec or tag, k)] = j[k]
            if 'results' in j or 'ms_per_step' in j or 'step_ms' in j: out[('bench.py', 'line')] = l.strip()
    return out
for tool in ('sort', 'sj', 'sj_forced'):
    runs = {'parent': [], 'new': []}
    for lib in runs:
        pat = '%s/%s_%s.txt' % (d, tool, lib) if tool == 'sj_forced' else '%s/%s_[0-9]_%s.txt' % (d, tool, lib)
        for p in sorted(glob.glob(pat)): runs[lib].append(parse(p))
    if not runs['parent'] or not runs['new']: continue
    print('\n### %s (%d parent runs, %d new runs)\n' % ({'sort': 'tools/bench_sort.py cfg3 7', 'sj': 'tools/bench_sj.py 10000000', 'sj_forced': 'tools/bench_sj.py 10000000, L2R_SORT_FORCE=1'}[tool], len(runs['parent']), len(runs['new'])))
    print('| section | figure | parent runs | parent min – max | new runs | new median | inside |\n|---|---|---|---|---|---|---|')
    for key in runs['parent'][0]:
        pv = [r[key] for r in runs['parent'] if key in r]; nv = [r[key] for r in runs['new'] if key in r]
        if not nv or isinstance(pv[0], str): continue
        med = S.median(nv)
        f = lambda v: ' '.join('%.3f' % x for x in v)
        print('| %s | %s | %s | %.3f – %.3f | %s | %.3f | %s |' % (key[0], key[1], f(pv), min(pv), max(pv), f(nv), med, 'yes' if min(pv) <= med <= max(pv) else ('below' if med < min(pv) else 'ABOVE')))
