"""Cost of recording a trajectory (keep_frames) next to the plain sampling call, at the headline shape.

    python scratch/chain_timing.py [--out profiles/chain_timing.json] [--reps 3] [--precisions fp32 fp16x3] [--no-python-loop]
    python scratch/chain_timing.py --alternate-with PARENT_CHECKOUT ...     # (a) against a built checkout of the parent commit

B = 256, N = 30, H = 256, L = 6, T = 1000, graph replay, one process.  Per precision, wall time of one whole call (stream synchronised
before and after), the kinds alternating repeat by repeat in the same run after one untimed call of each:
  (a) plain       `sample_from_masks` as it always was (the every-step loop).  With --alternate-with DIR (a built checkout of the
                  parent commit) it is first measured against the parent: three pairs of fresh processes, parent then this tree, each
                  one untimed and one timed call per precision (`alternating`; this script with --root DIR --plain-only, which
                  needs no keep_frames);
  (b) keep1000 / keep100   the same call with keep_frames = T and = 100 (the identity path in the path loop, one k_chain_frame per
                  transition, 1000 / 100 of which write a frame);
  (c) python_loop the loop this replaces: one `path_steps(k_lo=k, k_hi=k+1)` call per transition, `unnormalize` in torch and a copy
                  into the frame for the 100 kept ones, then the decode's share is left out (it is common to all).
Every entry keeps all repetitions; `derived` holds the ratios of the medians to (a) and the run-to-run spread (max - min) / median
of (a).  Expectation from the code, not a bar: (b) within the spread of (a) - one 338 KB write per kept frame beside a forward of
5.4 / 2.3 ms.
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
    ap.add_argument("--precisions", nargs="*", default=["fp32", "fp16x3"])
    ap.add_argument("--plain-only", action="store_true", help="measure (a) alone: works on a commit that has no keep_frames")
    ap.add_argument("--no-python-loop", action="store_true", help="leave (c) out")
    ap.add_argument("--root", default=None, help="import hierdiff_amd from this checkout (default: the one this script lies in)")
    ap.add_argument("--alternate-with", default=None, metavar="DIR", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--pairs", type=int, default=3)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    alternating = None
    if args.alternate_with:
        import subprocess
        import tempfile
        alternating = {"parent": {p: [] for p in args.precisions}, "this": {p: [] for p in args.precisions}}
        for _ in range(args.pairs):
            for side, root in (("parent", os.path.abspath(args.alternate_with)), ("this", here)):
                with tempfile.TemporaryDirectory() as tmp:
                    out = os.path.join(tmp, "plain.json")
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--plain-only", "--reps", "1", "--out", out,
                                    "--precisions"] + list(args.precisions), check=True, timeout=240, cwd=root)
                    with open(out) as fh:
                        got = json.load(fh)["seconds"]
                for p in args.precisions:
                    alternating[side][p].append(got[p]["plain"]["median"])
        print("alternating", json.dumps(alternating), flush=True)
    sys.path.insert(0, args.root or here)
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T = 256, 30, 256, 6, 1000
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)

    def python_loop(keep=100):
        from hierdiff_amd import paths
        frame_of = paths.chain_frames(T, keep).frame_of
        z = model.sample_combined_position_feature_noise(B, N, nm)
        chain = torch.zeros(keep, B, N, 11, device=DEV)
        for k in range(T):
            z = model.path_steps(z, nm, k_lo=k, k_hi=k + 1)
            if frame_of[k] >= 0:
                x, h = model.unnormalize(z[:, :, :3], z[:, :, 3:], nm.float())
                chain[frame_of[k]] = torch.cat([x, h], dim=2)
        return chain

    kinds = [("plain", lambda: model.sample_from_masks(nm, None, None))]
    if not args.plain_only:
        kinds += [("keep1000", lambda: model.sample_from_masks(nm, None, None, keep_frames=T)),
                  ("keep100", lambda: model.sample_from_masks(nm, None, None, keep_frames=100))]
        if not args.no_python_loop:
            kinds.append(("python_loop", python_loop))
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, reps=args.reps, device=torch.cuda.get_device_name(0)), "seconds": {}}
    with torch.no_grad():
        for prec in args.precisions:
            model.dynamics.precision = prec
            runs = {name: [] for name, _ in kinds}
            for name, call in kinds:
                if name != "python_loop":
                    call()                                   # untimed: tables and the graph of this kind
            for _ in range(args.reps):
                for name, call in kinds:
                    runs[name].append(once(call))
            row = {name: summary(v) for name, v in runs.items()}
            a = row["plain"]
            row["derived"] = {"spread_plain": (a["max"] - a["min"]) / a["median"]}
            for name in runs:
                if name != "plain":
                    row["derived"][f"ratio_{name}_over_plain"] = row[name]["median"] / a["median"]
            print(prec, json.dumps(row["derived"]), flush=True)
            res["seconds"][prec] = row
    if alternating:
        res["alternating"] = alternating
        for prec in args.precisions:
            pa, th = alternating["parent"][prec], alternating["this"][prec]
            res["seconds"][prec]["derived"].update(
                plain_parent_mean=statistics.mean(pa), plain_this_mean=statistics.mean(th),
                plain_parent_spread=max(pa) - min(pa), plain_this_spread=max(th) - min(th),
                ratio_plain_this_over_parent=statistics.mean(th) / statistics.mean(pa))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
