"""Cost of scoring (DiffusionQM9.nll_full: hd_nll_terms / hd_nll_finish) next to one sampling run, at the headline shape.

    python scratch/nll_timing.py [--out profiles/nll_timing.json] [--reps 3] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole call (stream
synchronised before and after; one untimed warm-up call each, which also captures the graph):
  nll_full_all        `nll_full` with all T terms (T + 1 network calls)
  nll_full_terms50    `nll_full(terms=50)`
  sample_plain        the plain 1000-step `sample_from_masks` on the same masks (T + 1 network calls)
  eager_loop          what `nll_full` replaces: eval-mode `model.nll` once per t with `t_int` replayed (two network calls and ~350
                      element-wise launches each), timed on 20 terms and scaled to T - marked `extrapolated`
Every entry keeps all repetitions; the summary holds median, min and max.  Expectation from the code: one term is one forward plus
two small kernels, one sampling step one forward plus one - `nll_full_all` within 1.05 x `sample_plain`.
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

    B, N, H, L, T, EAGER = 256, 30, 256, 6, 1000, 20
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    em = (~torch.eye(N, dtype=torch.bool, device=DEV)).expand(B, N, N).reshape(B, N * N).contiguous()
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, N, 3, generator=gen)
    x = (x - x.mean(1, keepdim=True)).to(DEV)
    h = torch.randn(B, N, 8, generator=gen).to(DEV)
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, reps=args.reps, device=torch.cuda.get_device_name(0)), "seconds": {}}

    def eager():
        for t in range(T, T - EAGER, -1):
            model.nll(x, h, nm, em, None, t_int=torch.full((B, 1), float(t), device=DEV))

    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            row = {}
            for name, fn in (("nll_full_all", lambda: model.nll_full(x, h, nm)),
                             ("nll_full_terms50", lambda: model.nll_full(x, h, nm, terms=50)),
                             ("sample_plain", lambda: model.sample_from_masks(nm, None)),
                             ("nll_full_all_again", lambda: model.nll_full(x, h, nm))):
                row[name] = summary(timed(fn, args.reps))
                print(prec, name, json.dumps(row[name]), flush=True)
            e = summary([v * T / EAGER for v in timed(eager, args.reps)])
            e.update(extrapolated=True, timed_terms=EAGER)
            row["eager_loop"] = e
            print(prec, "eager_loop", json.dumps(e), flush=True)
            med = lambda k: row[k]["median"]
            row["derived"] = {"nll_full_all_over_sample_plain": med("nll_full_all") / med("sample_plain"),
                              "nll_full_all_again_over_sample_plain": med("nll_full_all_again") / med("sample_plain"),
                              "ms_per_term": (med("nll_full_all") - med("nll_full_terms50")) / (T - 50) * 1e3,
                              "eager_loop_over_nll_full_all": med("eager_loop") / med("nll_full_all"),
                              "molecules_per_s": B / med("nll_full_all")}
            print(prec, "derived", json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
