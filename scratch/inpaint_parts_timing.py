"""Cost of partial inpainting (positions or features alone) next to the whole-node call.

    python scratch/inpaint_parts_timing.py [--out profiles/inpaint_parts_timing.json] [--reps 3] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, 10 of 30 nodes known, graph replay.  Per precision, wall time of one whole
`sample_inpaint` call (stream synchronised before and after; one untimed warm-up call each, which also captures the graph),
median of `reps` with its spread (max - min) / median:
  whole   fixed_mask                                  (the call of scratch/inpaint_timing.py, with 10 known nodes)
  x_only  fixed_x_mask = fixed_mask, fixed_h_mask empty   (positions known, features sampled)
  h_only  fixed_h_mask = fixed_mask, fixed_x_mask empty   (features known, positions sampled)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hierdiff_amd import DiffusionQM9, default_config  # noqa: E402
from hierdiff_amd.weights import synthetic_state_dict  # noqa: E402

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
    med = statistics.median(out)
    return {"seconds": out, "median": med, "spread": (max(out) - min(out)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    ap.add_argument("--timesteps", type=int, default=1000)
    args = ap.parse_args()
    B, N, H, L, T, known = 256, 30, 256, 6, args.timesteps, 10
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV)
    model.use_graph = True
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    fm = torch.zeros_like(nm)
    fm[:, :known] = True
    none = torch.zeros_like(nm)
    g = torch.Generator().manual_seed(0)
    xk, hk = torch.randn(B, N, 3, generator=g).to(DEV), torch.randn(B, N, 8, generator=g).to(DEV)
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, known_per_molecule=known, reps=args.reps, use_graph=True,
                          device=torch.cuda.get_device_name(0)), "results": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            row = {"whole": timed(lambda: model.sample_inpaint(nm, fm, xk, hk), args.reps),
                   "x_only": timed(lambda: model.sample_inpaint(nm, None, xk, hk, fixed_x_mask=fm, fixed_h_mask=none), args.reps),
                   "h_only": timed(lambda: model.sample_inpaint(nm, None, xk, hk, fixed_x_mask=none, fixed_h_mask=fm), args.reps)}
            row["ratio_to_whole"] = {k: row[k]["median"] / row["whole"]["median"] for k in ("x_only", "h_only")}
            res["results"][prec] = row
            print(prec, json.dumps({k: [round(v["median"], 4), round(v["spread"], 4)] for k, v in row.items() if k != "ratio_to_whole"}),
                  json.dumps(row["ratio_to_whole"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
