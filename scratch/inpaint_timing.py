"""Cost of fragment-constrained sampling next to plain sampling and next to the step-by-step Python loop it replaces.

    python scratch/inpaint_timing.py [--out profiles/inpaint_timing.json] [--reps 2] [--precisions fp32 fp16x3]

B = 256, N = 30, H = 256, L = 6, T = 1000, half of every molecule fixed.  Per precision, wall time of one whole call (stream
synchronised before and after; one untimed warm-up call each, which also captures the graph):
  plain         DiffusionQM9.sample_from_masks
  inpaint_r1/3  DiffusionQM9.sample_inpaint(resamplings = 1 / 3)
  python_loop   sample_p_zs_given_zt per step + the replacement step in torch ops (the only way before hd_sample_loop_inpaint)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hierdiff_amd import DiffusionQM9, default_config  # noqa: E402
from hierdiff_amd.weights import synthetic_state_dict  # noqa: E402

DEV = "cuda:0"


def python_loop(model, nm, fm, xh_known, gg):
    """Today's way: the reference-style per-step API with torch blending in between (torch.randn noise)."""
    B, N = nm.shape[:2]
    T = model.T
    nmf, fmf = nm.float(), fm.float()
    nfix = fmf.sum(1, keepdim=True).clamp(min=1)
    z = model.sample_combined_position_feature_noise(B, N, nm)
    for s in reversed(range(T)):
        s_arr = torch.full((B, 1), s, device=DEV)
        gm = (gg[s].expand(B, 1), gg[s + 1].expand(B, 1))
        z = model.sample_p_zs_given_zt(s_arr / T, (s_arr + 1) / T, z, nm, None, None, mol_shape=N, gammas=gm)
        a_s, s_s = torch.sqrt(torch.sigmoid(-gg[s])).to(DEV), torch.sqrt(torch.sigmoid(gg[s])).to(DEV)
        z_kn = (a_s * xh_known + s_s * torch.randn_like(z)) * fmf
        c = (z[:, :, :3] * fmf).sum(1, keepdim=True) / nfix - (z_kn[:, :, :3] * fmf).sum(1, keepdim=True) / nfix
        z_kn = torch.cat([z_kn[:, :, :3] + c, z_kn[:, :, 3:]], dim=2)
        z = torch.where(fm, z_kn, z)
        zx = z[:, :, :3]
        z = torch.cat([zx - (zx.sum(1, keepdim=True) / nmf.sum(1, keepdim=True)) * nmf, z[:, :, 3:]], dim=2)
    return z


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--skip-python-loop", action="store_true")
    args = ap.parse_args()
    B, N, H, L, T = 256, 30, 256, 6, args.timesteps
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV)
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    fm = torch.zeros_like(nm)
    fm[:, :N // 2] = True
    g = torch.Generator().manual_seed(0)
    xk, hk = torch.randn(B, N, 3, generator=g).to(DEV), torch.randn(B, N, 8, generator=g).to(DEV)
    xh_known = torch.cat([xk, hk], dim=2) * fm.float()
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, fixed_per_molecule=N // 2, reps=args.reps,
                          device=torch.cuda.get_device_name(0)), "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            gg = model._schedule(rows=B)["gamma"]
            row = {"plain": timed(lambda: model.sample_from_masks(nm, None), args.reps),
                   "inpaint_r1": timed(lambda: model.sample_inpaint(nm, fm, xk, hk, resamplings=1), args.reps),
                   "inpaint_r3": timed(lambda: model.sample_inpaint(nm, fm, xk, hk, resamplings=3), max(1, args.reps - 1))}
            if not args.skip_python_loop:
                row["python_loop"] = timed(lambda: python_loop(model, nm, fm, xh_known, gg), max(1, args.reps - 1))
            best = {k: min(v) for k, v in row.items()}
            row["ratio_to_plain"] = {k: best[k] / best["plain"] for k in best if k != "plain"}
            res["seconds"][prec] = row
            print(prec, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in best.items()}),
                  json.dumps(row["ratio_to_plain"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
