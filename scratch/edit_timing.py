"""Cost of editing given molecules (DiffusionQM9.encode / vary / slerp) next to plain few-step sampling, at the headline shape.

    python scratch/edit_timing.py [--out profiles/edit_timing.json] [--reps 3] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole call (stream
synchronised before and after; one untimed warm-up call each, which also captures the graph):
  encode_K1000        `encode` on every grid point (K = T ascending transitions, no decode)
  vary_K500           `vary` of 256 molecules at t_start = T / 2 with K = 500 (diffuse, 500 transitions, decode, host list handling)
  latent_K500         its device part alone: `diffuse` + `sample_from_latent(t_start = T / 2, steps = 500)`
  sample_K1000 / sample_K500   plain `sample_from_masks(steps=K)` for the same K (K = 1000 forced through the path loop)
  diffuse, slerp_8    one `diffuse` call, one `slerp` call with 8 frames
Every entry keeps all repetitions; the summary holds median, min and max; `derived` holds the per-transition times.  Expectation
from the code: an inversion transition is one forward plus one k_post_step, the cost of a few-step transition; k_diffuse and k_slerp
are a few microseconds, once per call.
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
    x = torch.randn(B, N, 3, generator=gen)
    x = (x - x.mean(1, keepdim=True))
    h = torch.randn(B, N, 8, generator=gen)
    mols = [{"x": x[i].clone(), "h": h[i].clone()} for i in range(B)]
    x, h = x.to(DEV), h.to(DEV)
    za = torch.randn(B, N, 11, generator=gen).to(DEV)
    zb = torch.randn(B, N, 11, generator=gen).to(DEV)
    lam = [i / 7 for i in range(8)]
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, reps=args.reps, device=torch.cuda.get_device_name(0)), "seconds": {}}

    def plain_full():
        model._force_path_loop = True
        try:
            return model.sample_from_masks(nm, None, steps=T)
        finally:
            model._force_path_loop = False

    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            row = {}
            for name, fn in (("encode_K1000", lambda: model.encode(x, h, nm)),
                             ("sample_K1000", plain_full),
                             ("vary_K500", lambda: model.vary(mols, DEV, T // 2, steps=500)),
                             ("latent_K500", lambda: model.sample_from_latent(model.diffuse(x, h, nm, T // 2), nm, t_start=T // 2, steps=500)),
                             ("sample_K500", lambda: model.sample_from_masks(nm, None, steps=500)),
                             ("diffuse", lambda: model.diffuse(x, h, nm, T // 2)),
                             ("slerp_8", lambda: model.slerp(za, zb, lam, nm))):
                row[name] = summary(timed(fn, args.reps))
                print(prec, name, json.dumps(row[name]), flush=True)
            med = lambda k: row[k]["median"]
            row["derived"] = {"ms_per_transition_encode_K1000": med("encode_K1000") / T * 1e3,
                              "ms_per_transition_sample_K1000": med("sample_K1000") / T * 1e3,
                              "ms_per_transition_latent_K500": med("latent_K500") / 500 * 1e3,
                              "ms_per_transition_vary_K500": med("vary_K500") / 500 * 1e3,
                              "ms_per_transition_sample_K500": med("sample_K500") / 500 * 1e3}
            print(prec, "derived", json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
