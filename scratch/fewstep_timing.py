"""Cost of few-step sampling (hd_sample_path) next to the plain loop, at the headline shape.

    python scratch/fewstep_timing.py [--out profiles/fewstep_timing.json] [--reps 3] [--precisions fp32 fp16x3]
                                     [--root DIR] [--plain-only] [--merge OTHER.json] [--rows K:ETA ...] [--plain-launches]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay.  Per precision, wall time of one whole `sample_from_masks` call (z_T,
the loop, the decode; stream synchronised before and after; one untimed warm-up call each, which also captures the graph):
  plain                the plain loop (defaults)
  path_K<K>_eta<e>     K in {1000, 250, 100, 50, 20}, eta in {1, 0}; K = 1000, eta = 1 is the identity path forced through the
                       path loop
Every entry keeps all repetitions; the summary holds median, min and max.  `--root DIR --plain-only` times the plain loop of
another checkout (the parent commit) in the same session; `--merge` copies that file's result in as "parent_plain".
`--rows 20:1 20:0 50:1 1000:1` times only those path rows (no plain loop, nothing derived); `--plain-launches` turns graph replay
off (`use_graph = False`: the host walks the library's launch code every transition).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

KS = [1000, 250, 100, 50, 20]
DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--rows", nargs="*", default=None)
    ap.add_argument("--plain-launches", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T = 256, 30, 256, 6, 1000
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV)
    model.use_graph = not args.plain_launches
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, reps=args.reps, device=torch.cuda.get_device_name(0), root=os.path.basename(
        os.path.abspath(args.root)), use_graph=not args.plain_launches), "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            if args.rows is not None:
                row = {}
                for K, eta in (r.split(":") for r in args.rows):
                    model._force_path_loop = True
                    name = f"path_K{K}_eta{eta}"
                    row[name] = summary(timed(lambda: model.sample_from_masks(nm, None, steps=int(K), eta=float(eta)), args.reps))
                    model._force_path_loop = False
                    print(prec, name, json.dumps(row[name]), flush=True)
                res["seconds"][prec] = row
                continue
            row = {"plain": summary(timed(lambda: model.sample_from_masks(nm, None), args.reps))}
            print(prec, "plain", json.dumps(row["plain"]), flush=True)
            if not args.plain_only:
                for K in KS:
                    for eta in (1.0, 0.0):
                        model._force_path_loop = True
                        name = f"path_K{K}_eta{int(eta)}"
                        row[name] = summary(timed(lambda: model.sample_from_masks(nm, None, steps=K, eta=eta), args.reps))
                        model._force_path_loop = False
                        row[name]["molecules_per_s"] = B / row[name]["median"]
                        print(prec, name, json.dumps(row[name]), flush=True)
                row["plain_again"] = summary(timed(lambda: model.sample_from_masks(nm, None), args.reps))
                print(prec, "plain_again", json.dumps(row["plain_again"]), flush=True)
                med = lambda k: row[k]["median"]
                row["derived"] = {
                    "path_K1000_over_plain": med("path_K1000_eta1") / med("plain"),
                    "per_transition_ms_K1000_vs_K100": [(med(f"path_K{k}_eta1") - med("path_K20_eta1")) / (k - 20) * 1e3 for k in (1000, 100)],
                    "eta0_saving_us_per_transition": (med("path_K1000_eta1") - med("path_K1000_eta0")) / 1000 * 1e6,
                }
                print(prec, "derived", json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.merge and os.path.exists(args.merge):
        with open(args.merge) as fh:
            other = json.load(fh)
        for prec, row in other["seconds"].items():
            res["seconds"].setdefault(prec, {})["parent_plain"] = row["plain"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
