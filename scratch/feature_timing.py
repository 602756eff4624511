"""Cost of feature restraints next to the same build's unrestrained and obstacle-restrained calls, at the headline shape.

    python scratch/feature_timing.py [--out profiles/feature_timing.json] [--reps 3] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole `sample_from_masks` call
(stream synchronised before and after), the kinds alternating repeat by repeat after one untimed call of each:
  path        the unrestrained call through the path loop on the identity path (what a restrained call runs without restraints);
  obstacles   the 200 obstacles, 4 pairs and 2 anchors of scratch/restraint_timing.py (one k_restrain_eps per transition);
  features    dense bands on all 30 nodes x 8 channels plus 8 sums, no other table (k_restrain_eps on empty tables and
              one k_restrain_feat per transition);
  both        obstacles and features.
`derived` holds the ratios of the medians over `path`, the run-to-run spread (max - min) / median of every kind and the difference
of the medians per transition in microseconds.  Expectation from the code, not a bar: one more launch of a few microseconds per
transition beside a forward of 5.4 / 2.3 ms.
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
    from hierdiff_amd.restraints import Features, FeatureSum, Restraints
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T, F = 256, 30, 256, 6, 1000, 8
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(0)
    obs = torch.cat([torch.randn(200, 3, generator=g) * 6.0, torch.full((200, 1), 2.0), torch.ones(200, 1)], dim=1)
    tabs = dict(obstacles=obs, pairs=[[0, 1, 1.0, 2.0, 1.0], [2, 3, 1.0, 2.0, 1.0], [4, 5, 3.0, 4.0, 1.0], [6, 7, 0.0, 5.0, 1.0]],
                anchors=[[0, 1.0, 0.0, 0.0, 0.5, 1.0], [9, -1.0, 0.0, 0.0, 0.5, 1.0]])
    ft = Features.target(torch.randn(N, F, generator=g), k=1.0, tol=0.25,
                         sums=[FeatureSum(torch.randn(F, generator=g), lo=-1.0, hi=1.0, reduce="mean" if r % 2 else "sum") for r in range(8)])
    kw = dict(restraint_scale=0.01, restraint_clip=0.1)

    def path_call():
        model._force_path_loop = True
        try:
            return model.sample_from_masks(nm, None, None)
        finally:
            model._force_path_loop = False

    kinds = [("path", path_call),
             ("obstacles", lambda: model.sample_from_masks(nm, None, None, restraints=Restraints(**tabs), **kw)),
             ("features", lambda: model.sample_from_masks(nm, None, None, restraints=Restraints(features=ft), **kw)),
             ("both", lambda: model.sample_from_masks(nm, None, None, restraints=Restraints(features=ft, **tabs), **kw))]
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, P=200, Q=4, A=2, W=N, F=F, S=8, reps=args.reps, device=torch.cuda.get_device_name(0)),
           "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            runs = {name: [] for name, _ in kinds}
            for _, call in kinds:
                call()                                       # untimed: tables and the graph of this kind
            for _ in range(args.reps):
                for name, call in kinds:
                    runs[name].append(once(call))
            row = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / statistics.median(v),
                          "runs": v} for name, v in runs.items()}
            p = row["path"]["median"]
            us = lambda a, b: (row[a]["median"] - row[b]["median"]) / T * 1e6
            row["derived"] = {"ratio_obstacles_over_path": row["obstacles"]["median"] / p, "ratio_features_over_path": row["features"]["median"] / p,
                              "ratio_both_over_path": row["both"]["median"] / p, "us_per_transition_features_minus_path": us("features", "path"),
                              "us_per_transition_both_minus_obstacles": us("both", "obstacles")}
            print(prec, json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
