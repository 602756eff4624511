"""Cost of predictor-corrector sampling (corrector=Corrector(C)) next to the plain path loop, at the headline shape.

    python scratch/corrector_timing.py [--out profiles/corrector_timing.json] [--reps 3] [--steps 50] [--precisions fp32 fp16x3]
                                       [--plain-only]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole `path_steps` call (stream
synchronised before and after) on the SAME uniform K-step ancestral path: the plain call, C = 1 and C = 2, alternating repeat by repeat
in the same run, after one untimed call of each kind (switching re-instantiates the captured transition, so every timed call is
preceded by an untimed one of the same kind).  Every entry keeps all repetitions; the summary holds median, min and max; `derived` holds
the ratios of the medians to (C + 1) times the plain median - the expectation from the code is (C + 1) forwards per transition plus
one launch of a few microseconds, which is not a gate - and the run-to-run spread (max - min) / median of the plain runs.
`--plain-only` times the plain call alone and imports nothing of the corrector: the regression guard is this script with that flag in
a checkout of the parent commit and in this one, in one session, one process each.
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


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T, K = 256, 30, 256, 6, 1000, args.steps
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(B, N, 11, generator=gen)
    z[:, :, :3] -= z[:, :, :3].mean(1, keepdim=True)
    z = z.to(DEV)
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, steps=K, reps=args.reps, device=torch.cuda.get_device_name(0),
                          plain_only=args.plain_only), "seconds": {}}
    kinds = [("plain", dict())]
    if not args.plain_only:
        from hierdiff_amd.corrector import Corrector
        kinds += [("C1", dict(corrector=Corrector(1))), ("C2", dict(corrector=Corrector(2)))]
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            runs = {name: [] for name, _ in kinds}
            for _ in range(args.reps):
                for name, kw in kinds:
                    call = lambda: model.path_steps(z, nm, steps=K, eta=1.0, **kw)
                    call()                                   # untimed: the graph of this kind
                    runs[name].append(once(call))
            row = {name: summary(v) for name, v in runs.items()}
            p = row["plain"]
            row["derived"] = {"spread_plain": (p["max"] - p["min"]) / p["median"], "ms_per_transition_plain": p["median"] / K * 1e3}
            for name, c in (("C1", 1), ("C2", 2)):
                if name in row:
                    row["derived"][f"ratio_{name}_over_{c + 1}x_plain"] = row[name]["median"] / ((c + 1) * p["median"])
                    row["derived"][f"spread_{name}"] = (row[name]["max"] - row[name]["min"]) / row[name]["median"]
            print(prec, json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res["seconds"]))


if __name__ == "__main__":
    main()
