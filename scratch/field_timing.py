"""Cost of a lattice field next to the obstacle list it was rasterised from, at the headline shape, and the regression guard of the
plain restrained call against the parent commit.

    python scratch/field_timing.py [--out profiles/field_timing.json] [--reps 3] [--precisions fp32 fp16x3]
                                   [--parent PARENT.json --this THIS.json]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole `sample_from_masks` call
(stream synchronised before and after), the kinds alternating repeat by repeat after one untimed call of each:
  path        the unrestrained call through the path loop on the identity path;
  obstacles   the 200-obstacle call of scratch/restraint_timing.py (200 obstacles, 4 pairs, 2 anchors);
  field       one 64^3 field made from those same 200 obstacles with `Field.from_obstacles` (spacing 0.5 around the origin), alone;
  both        the obstacle tables and the field together.
`derived` holds the ratios of the medians, the spread (max - min) / median of every kind and the microseconds per transition above
`path`.  Expectation from the code, not a bar: 8 loads per node against 200 distance evaluations - the field call costs no more than
the obstacle call.

--parent / --this: the JSON files `scratch/restraint_timing.py` wrote on the parent commit and on this one in the same session.  Their
`restrained` medians go into `regression_guard` with the parent's own run-to-run spread of that kind; `within_parent_spread` says
whether this commit's median exceeds the parent's by no more than that spread (a call without fields runs the same loops, plus one
loop test per node group on NF = 0).
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


def guard(parent, this):
    out = {}
    for prec, row in parent["seconds"].items():
        if prec not in this["seconds"]:
            continue
        p, t = row["restrained"], this["seconds"][prec]["restrained"]
        spread = (p["max"] - p["min"]) / p["median"]
        out[prec] = {"parent_median": p["median"], "this_median": t["median"], "parent_spread": spread,
                     "ratio_this_over_parent": t["median"] / p["median"],
                     "within_parent_spread": t["median"] <= p["median"] * (1.0 + spread), "parent_runs": p["runs"], "this_runs": t["runs"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--this", default=None)
    args = ap.parse_args()
    if (args.parent is None) != (args.this is None):
        ap.error("--parent and --this go together")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.restraints import Field, Restraints
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T, G = 256, 30, 256, 6, 1000, 64
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(0)
    obs = torch.cat([torch.randn(200, 3, generator=g) * 6.0, torch.full((200, 1), 2.0), torch.ones(200, 1)], dim=1)
    pairs = [[0, 1, 1.0, 2.0, 1.0], [2, 3, 1.0, 2.0, 1.0], [4, 5, 3.0, 4.0, 1.0], [6, 7, 0.0, 5.0, 1.0]]
    anchors = [[0, 1.0, 0.0, 0.0, 0.5, 1.0], [9, -1.0, 0.0, 0.0, 0.5, 1.0]]
    h = 0.5
    t0 = time.perf_counter()
    field = Field.from_obstacles(obs, [-0.5 * h * (G - 1)] * 3, (G, G, G), h)
    raster = time.perf_counter() - t0
    sets = {"obstacles": Restraints(obstacles=obs, pairs=pairs, anchors=anchors), "field": Restraints(fields=field),
            "both": Restraints(obstacles=obs, pairs=pairs, anchors=anchors, fields=field)}

    def path_call():
        model._force_path_loop = True
        try:
            return model.sample_from_masks(nm, None, None)
        finally:
            model._force_path_loop = False

    restrained = lambda k: (lambda: model.sample_from_masks(nm, None, None, restraints=sets[k], restraint_scale=0.01, restraint_clip=0.1))
    kinds = [("path", path_call)] + [(k, restrained(k)) for k in ("obstacles", "field", "both")]
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, P=200, Q=4, A=2, lattice=[G, G, G], spacing=h, reps=args.reps,
                          rasterise_seconds_cpu=raster, device=torch.cuda.get_device_name(0)), "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            runs = {name: [] for name, _ in kinds}
            for _, call in kinds:
                call()                                       # untimed: tables, the lattice's upload and the graph of this kind
            for _ in range(args.reps):
                for name, call in kinds:
                    runs[name].append(once(call))
            row = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / statistics.median(v),
                          "runs": v} for name, v in runs.items()}
            p = row["path"]["median"]
            row["derived"] = {f"ratio_{k}_over_path": row[k]["median"] / p for k in ("obstacles", "field", "both")}
            row["derived"].update({f"{k}_minus_path_us_per_transition": (row[k]["median"] - p) / T * 1e6 for k in ("obstacles", "field", "both")})
            row["derived"]["ratio_field_over_obstacles"] = row["field"]["median"] / row["obstacles"]["median"]
            print(prec, json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.parent is not None:
        with open(args.parent) as fh:
            parent = json.load(fh)
        with open(args.this) as fh:
            this = json.load(fh)
        res["regression_guard"] = guard(parent, this)
        print("regression guard", json.dumps({k: {a: b for a, b in v.items() if not a.endswith("runs")}
                                              for k, v in res["regression_guard"].items()}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
