"""Cost of the stochastic second-order multistep solver (solver="sde2m") next to the ancestral (eta = 1) path loop, at the headline
shape.

    python scratch/sde_solver_timing.py [--out profiles/sde_solver_timing.json] [--reps 3] [--steps 50] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision and K, wall time of one whole `path_steps` call
(stream synchronised before and after) on the SAME uniform K-step path, `eta=1` and `solver="sde2m"` alternating repeat by repeat in
the same run, after one untimed call of each.  Switching between the two re-uploads the path and re-instantiates the captured
transition, so every timed call is preceded by an untimed one of the same kind.  Every entry keeps all repetitions; the summary
holds median, min and max; `derived` holds the ratio of the medians and the run-to-run spread (max - min) / median of the eta = 1
runs.  No bar: the expectation from the code is that the two are equal within that spread - the difference is one extra [B,N,D] read
and write per transition beside a forward of several milliseconds.
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
    ap.add_argument("--steps", type=int, nargs="*", default=[50])
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T = 256, 30, 256, 6, 1000
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(B, N, 11, generator=gen)
    z[:, :, :3] -= z[:, :, :3].mean(1, keepdim=True)
    z = z.to(DEV)
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, steps=args.steps, reps=args.reps, device=torch.cuda.get_device_name(0)),
           "seconds": {}}
    kinds = (("eta1", dict(eta=1.0)), ("sde2m", dict(solver="sde2m")))
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            res["seconds"][prec] = {}
            for K in args.steps:
                runs = {name: [] for name, _ in kinds}
                for _ in range(args.reps):
                    for name, kw in kinds:
                        call = lambda: model.path_steps(z, nm, steps=K, **kw)
                        call()                               # untimed: the path upload and the graph of this kind
                        runs[name].append(once(call))
                row = {name: summary(v) for name, v in runs.items()}
                e1 = row["eta1"]
                row["derived"] = {"ratio_sde2m_over_eta1": row["sde2m"]["median"] / e1["median"],
                                  "spread_eta1": (e1["max"] - e1["min"]) / e1["median"],
                                  "ms_per_transition_eta1": e1["median"] / K * 1e3,
                                  "ms_per_transition_sde2m": row["sde2m"]["median"] / K * 1e3}
                print(prec, K, json.dumps(row["derived"]), flush=True)
                res["seconds"][prec][f"K{K}"] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
