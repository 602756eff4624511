"""Cost of classifier-free guidance next to the unguided path loop, at the headline shape.

    python scratch/guidance_timing.py [--out profiles/guidance_timing.json] [--reps 3] [--steps 200] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, one context column, graph replay, one process.  Per precision, wall time of one whole
`path_steps` call (stream synchronised before and after; one untimed warm-up call each, which also captures the graph) on the SAME
uniform K-step path (default K = 200 of the T = 1000 grid; --steps 1000 is the full chain), eta = 1, in the same run:
  unguided            hd_sample_path
  guided_w2.5         hd_sample_path_guided, one shared scale, phi = 0
  guided_rows_phi0.7  hd_sample_path_guided, one scale per molecule, phi = 0.7 (the reductions of k_guide_combine run)
Every entry keeps all repetitions; the summary holds median, min and max; `derived` holds the per-transition times and the ratios.
Expectation from the code, not a bar: a guided transition is two forwards plus one k_guide_combine of a few microseconds, i.e. about
2.0x the unguided one.  A clearly larger ratio is a finding to explain.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T, K = 256, 30, 256, 6, 1000, args.steps
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, context_node_nf=1, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 1, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(B, N, 11, generator=gen)
    z[:, :, :3] -= z[:, :, :3].mean(1, keepdim=True)
    z = z.to(DEV)
    ctx = torch.randn(B, 1, 1, generator=gen).expand(B, N, 1).contiguous().to(DEV)
    w_rows = torch.linspace(0.5, 3.0, B)
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, K=K, context_node_nf=1, reps=args.reps, device=torch.cuda.get_device_name(0)),
           "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            row = {}
            for name, kw in (("unguided", dict()),
                             ("guided_w2.5", dict(guidance_scale=2.5)),
                             ("guided_rows_phi0.7", dict(guidance_scale=w_rows, guidance_rescale=0.7))):
                row[name] = summary(timed(lambda: model.path_steps(z, nm, None, ctx, steps=K, eta=1.0, **kw), args.reps))
                print(prec, name, json.dumps(row[name]), flush=True)
            med = lambda k: row[k]["median"]
            row["derived"] = {"ms_per_transition_unguided": med("unguided") / K * 1e3,
                              "ms_per_transition_guided_w2.5": med("guided_w2.5") / K * 1e3,
                              "ms_per_transition_guided_rows_phi0.7": med("guided_rows_phi0.7") / K * 1e3,
                              "ratio_guided_w2.5": med("guided_w2.5") / med("unguided"),
                              "ratio_guided_rows_phi0.7": med("guided_rows_phi0.7") / med("unguided")}
            print(prec, "derived", json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
