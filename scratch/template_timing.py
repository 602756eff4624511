"""Cost of a template restraint next to the same build's unrestrained call, at the headline shape.

    python scratch/template_timing.py [--out profiles/template_timing.json] [--reps 3] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole `sample_from_masks` call
(stream synchronised before and after), the kinds alternating repeat by repeat after one untimed call of each:
  path                 the unrestrained call through the path loop on the identity path (what a restrained call runs without restraints);
  template             the same with one rigid template of 10 rows shared by all molecules (k_restrain_eps<false, true> per transition:
                       two block sums, the serial Jacobi solve by one thread, the gather);
  obstacles            the 200 obstacles, 4 pairs and 2 anchors of scratch/restraint_timing.py (k_restrain_eps<false, false>);
  obstacles+template   both.
`derived` holds the ratios of the medians, the cost per transition in microseconds and the run-to-run spread (max - min) / median
of `path`.  Expectation from the code, not a bar: the solver's serial stretch is a few microseconds per transition beside a forward
of 5.4 / 2.3 ms.
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
    from hierdiff_amd.restraints import Restraints, Template
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T = 256, 30, 256, 6, 1000
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(0)
    obs = torch.cat([torch.randn(200, 3, generator=g) * 6.0, torch.full((200, 1), 2.0), torch.ones(200, 1)], dim=1)
    tables = dict(obstacles=obs, pairs=[[0, 1, 1.0, 2.0, 1.0], [2, 3, 1.0, 2.0, 1.0], [4, 5, 3.0, 4.0, 1.0], [6, 7, 0.0, 5.0, 1.0]],
                  anchors=[[0, 1.0, 0.0, 0.0, 0.5, 1.0], [9, -1.0, 0.0, 0.0, 0.5, 1.0]])
    tpl = Template(list(range(0, 30, 3)), torch.randn(10, 3, generator=g) * 2.0, k=1.0)
    sets = {"template": Restraints(templates=tpl), "obstacles": Restraints(**tables), "obstacles+template": Restraints(templates=tpl, **tables)}

    def path_call():
        model._force_path_loop = True
        try:
            return model.sample_from_masks(nm, None, None)
        finally:
            model._force_path_loop = False

    def restrained(name):
        return lambda: model.sample_from_masks(nm, None, None, restraints=sets[name], restraint_scale=0.01, restraint_clip=0.1)

    kinds = [("path", path_call)] + [(name, restrained(name)) for name in sets]
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, M=10, P=200, Q=4, A=2, reps=args.reps, device=torch.cuda.get_device_name(0)), "seconds": {}}
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
            a = row["path"]["median"]
            row["derived"] = {"spread_path": row["path"]["spread"],
                              "ratio_template_over_path": row["template"]["median"] / a,
                              "ratio_obstacles_over_path": row["obstacles"]["median"] / a,
                              "ratio_both_over_obstacles": row["obstacles+template"]["median"] / row["obstacles"]["median"],
                              "us_per_transition_template": (row["template"]["median"] - a) / T * 1e6,
                              "us_per_transition_obstacles": (row["obstacles"]["median"] - a) / T * 1e6,
                              "us_per_transition_template_on_obstacles":
                                  (row["obstacles+template"]["median"] - row["obstacles"]["median"]) / T * 1e6}
            print(prec, json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
