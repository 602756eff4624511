"""Cost of restrained inpainting (restraints in the known fragments' frame) next to the same build's unrestrained inpainting call, at
the headline shape, and the regression guard of the plain restrained call against the parent commit.

    python scratch/restraint_inpaint_timing.py [--out profiles/restraint_inpaint_timing.json] [--reps 3] [--precisions fp32 fp16x3]
                                               [--parent PARENT.json --this THIS.json]

B = 256, N = 30 (the first 10 nodes known, around (12, -7, 30)), H = 256, L = 6, T = 1000, one resampling round, graph replay, one
process.  Per precision, wall time of one whole `sample_inpaint` call (stream synchronised before and after), the kinds alternating
repeat by repeat after one untimed call of each:
  plain     the unrestrained inpainting call as it always was (the every-step loop);
  path      the unrestrained call through the path loop on the identity path (what a framed call runs without restraints);
  framed    the same with 200 obstacles, 4 pairs and 2 anchors around the known fragments, restraint_frame="known" (one
            k_restrain_eps<true> per transition; the call also evaluates the energy of its result once).
`derived` holds the ratios of the medians and the run-to-run spread (max - min) / median of `plain`.  A report, not a bar; the
expectation from the code is the plain restraint's 20 - 30 us per transition plus one more double reduction.

--parent / --this: the JSON files `scratch/restraint_timing.py` wrote on the parent commit and on this one in the same session.  Their
`restrained` medians go into `regression_guard` with the parent's own run-to-run spread of that kind; `within_parent_spread` says
whether this commit's median exceeds the parent's by no more than that spread (the FRAMED = false instantiation is meant to be the
same code)."""
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
    from hierdiff_amd.restraints import Restraints
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T, KN = 256, 30, 256, 6, 1000, 10
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    fm = torch.zeros(B, N, 1, dtype=torch.bool, device=DEV)
    fm[:, :KN] = True
    g = torch.Generator().manual_seed(0)
    centre = torch.tensor([12.0, -7.0, 30.0])
    xk = ((centre + torch.randn(B, N, 3, generator=g) * 1.5) * fm.cpu()).to(DEV)
    hk = (torch.randn(B, N, 8, generator=g) * fm.cpu()).to(DEV)
    obs = torch.cat([centre + torch.randn(200, 3, generator=g) * 6.0, torch.full((200, 1), 2.0), torch.ones(200, 1)], dim=1)
    rs = Restraints(obstacles=obs, pairs=[[0, 11, 1.0, 2.0, 1.0], [12, 13, 1.0, 2.0, 1.0], [14, 15, 3.0, 4.0, 1.0], [16, 17, 0.0, 5.0, 1.0]],
                    anchors=[[20, 13.0, -7.0, 30.0, 0.5, 1.0], [29, 11.0, -7.0, 30.0, 0.5, 1.0]])

    def path_call():
        model._force_path_loop = True
        try:
            return model.sample_inpaint(nm, fm, xk, hk)
        finally:
            model._force_path_loop = False

    kinds = [("plain", lambda: model.sample_inpaint(nm, fm, xk, hk)),
             ("path", path_call),
             ("framed", lambda: model.sample_inpaint(nm, fm, xk, hk, restraints=rs, restraint_scale=0.01, restraint_clip=0.1,
                                                     restraint_frame="known"))]
    res = {"config": dict(B=B, N=N, known=KN, H=H, L=L, T=T, P=200, Q=4, A=2, resamplings=1, reps=args.reps,
                          device=torch.cuda.get_device_name(0)), "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            runs = {name: [] for name, _ in kinds}
            for _, call in kinds:
                call()                                       # untimed: tables and the graph of this kind
            for _ in range(args.reps):
                for name, call in kinds:
                    runs[name].append(once(call))
            row = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for name, v in runs.items()}
            a = row["plain"]
            row["derived"] = {"spread_plain": (a["max"] - a["min"]) / a["median"],
                              "ratio_path_over_plain": row["path"]["median"] / a["median"],
                              "ratio_framed_over_plain": row["framed"]["median"] / a["median"],
                              "ratio_framed_over_path": row["framed"]["median"] / row["path"]["median"],
                              "framed_minus_path_us_per_transition": (row["framed"]["median"] - row["path"]["median"]) / T * 1e6}
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
