"""A/B of two library builds on bench.py (EXPERIMENTS.md section AS): DIR holds <side>_<form>_<rep>.json, side parent | branch, form
eager | graph, each the output of `HIERDIFF_LIB=<library> python bench.py --gpus 1 --steps 2 --warmup 1 --full --no-cpu-baseline
[--graph]`, the sides alternating.  Flattens every number of the JSON lines and says, per figure, whether the branch's values lie
within the range of the parent's own repeats; writes DIR/summary.json.  usage: python scratch/bench_ab_compare.py DIR"""
import glob
import json
import os
import re
import sys

d = sys.argv[1]
SKIP = re.compile(r"steps$|warmup$|n_gpus|batch|n_nodes|hidden|n_layers|timesteps|rccl|launches|_B$|\.B$|\.N$|\.H$|\.L$|\.T$")


def flat(o, pre=""):
    out = {}
    if isinstance(o, dict):
        for k, v in o.items():
            out.update(flat(v, f"{pre}.{k}" if pre else k))
    elif isinstance(o, list):
        for i, v in enumerate(o):
            out.update(flat(v, f"{pre}[{i}]"))
    elif isinstance(o, (int, float)) and not isinstance(o, bool):
        out[pre] = float(o)
    return out


res = {}
for f in sorted(glob.glob(os.path.join(d, "*_*_*.json"))):
    side, form, rep = os.path.basename(f)[:-5].split("_")
    lines = [ln for ln in open(f).read().splitlines() if ln.startswith("{")]
    if not lines:
        continue
    res.setdefault(form, {}).setdefault(side, []).append(flat(json.loads(lines[-1])))
summary = {}
for form, sides in res.items():
    p, b = sides.get("parent", []), sides.get("branch", [])
    print(f"== {form}: {len(p)} parent runs, {len(b)} branch runs")
    rows = []
    for k in p[0]:
        pv = [r[k] for r in p if k in r]
        bv = [r[k] for r in b if k in r]
        if not bv or len(set(pv + bv)) == 1 or SKIP.search(k):
            continue
        lo, hi = min(pv), max(pv)
        inside = all(lo <= v <= hi for v in bv)
        med = sorted(bv)[len(bv) // 2]
        rows.append((k, pv, bv, inside))
        summary.setdefault(form, {})[k] = {"parent": pv, "branch": bv, "branch_within_parent_range": inside,
                                          "branch_median_vs_parent_range": 0.0 if lo <= med <= hi else (med - hi if med > hi else med - lo)}
    for k, pv, bv, inside in rows:
        print(f"{'  ' if inside else 'OUT'} {k}: parent {pv} branch {bv}")
json.dump(summary, open(os.path.join(d, "summary.json"), "w"), indent=1)
