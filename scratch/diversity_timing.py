"""Cost of diverse sampling next to the same build's call without it, at the headline shape.

    python scratch/diversity_timing.py [--out profiles/diversity_timing.json] [--reps 3] [--precisions fp32 fp16x3]

B = 256 as 32 groups of 8, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole
`sample_from_masks` call (stream synchronised before and after), the kinds alternating repeat by repeat after one untimed call of each:
  path                 the unrestrained call through the path loop (`_force_path_loop`: the identity path, ancestral steps);
  diverse              the same with diversity=Diversity(8, length, strength, clip=0.1) (one k_diverse_eps per transition);
  diverse+restrained   the diverse call on top of the 200 obstacles + 4 pairs + 2 anchors of scratch/restraint_timing.py;
  restrained           that restrained call alone (what the diverse launch is added to there).
`derived` holds the cost of the diverse launch in microseconds per transition in both settings, and the run-to-run spread
(max - min) / median of every kind.  No bar is set.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

DEV = "cuda:0"


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.diversity import Diversity
    from hierdiff_amd.restraints import Restraints
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T, P = 256, 30, 256, 6, 1000, 8
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(0)
    obs = torch.cat([torch.randn(200, 3, generator=g) * 6.0, torch.full((200, 1), 2.0), torch.ones(200, 1)], dim=1)
    rs = Restraints(obstacles=obs, pairs=[[0, 1, 1.0, 2.0, 1.0], [2, 3, 1.0, 2.0, 1.0], [4, 5, 3.0, 4.0, 1.0], [6, 7, 0.0, 5.0, 1.0]],
                    anchors=[[0, 1.0, 0.0, 0.0, 0.5, 1.0], [9, -1.0, 0.0, 0.0, 0.5, 1.0]])
    rkw = dict(restraints=rs, restraint_scale=0.01, restraint_clip=0.1)
    dv = Diversity(P, 2.0, strength=0.05, clip=0.1)
    model._force_path_loop = True                            # the plain call too runs hd_sample_path on the identity path
    few = {}
    kinds = [("path", lambda: model.sample_from_masks(nm, None, None, **few)),
             ("diverse", lambda: model.sample_from_masks(nm, None, None, diversity=dv, **few)),
             ("restrained", lambda: model.sample_from_masks(nm, None, None, **few, **rkw)),
             ("diverse+restrained", lambda: model.sample_from_masks(nm, None, None, diversity=dv, **few, **rkw))]
    res = {"config": dict(B=B, groups=B // P, particles=P, N=N, H=H, L=L, T=T, obstacles=200, pairs=4, anchors=2, reps=args.reps,
                          length=dv.length, strength=dv.strength, device=torch.cuda.get_device_name(0)), "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            runs = {name: [] for name, _ in kinds}
            for _, call in kinds:
                call()                                       # untimed: tables and the graph of this kind
            for _ in range(args.reps):
                for name, call in kinds:
                    runs[name].append(once(call))
            row = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v,
                          "spread": (max(v) - min(v)) / statistics.median(v)} for name, v in runs.items()}
            last = model.diversity_last
            row["derived"] = {"us_per_transition_alone": (row["diverse"]["median"] - row["path"]["median"]) / T * 1e6,
                              "us_per_transition_on_restraints": (row["diverse+restrained"]["median"] - row["restrained"]["median"]) / T * 1e6,
                              "ratio_diverse_over_path": row["diverse"]["median"] / row["path"]["median"],
                              "mean_pairwise_rmsd_of_the_last_call": float(torch.nanmean(last.mean_rmsd))}
            print(prec, json.dumps({k: v["median"] for k, v in row.items() if k != "derived"}), json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
