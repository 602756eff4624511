"""Host-side cost per call of the restraint entry points, resolved in microseconds: what a change to the host code around the
restraint kernels can move (the kernels themselves being the same).

    python scratch/restraint_state_timing.py [--out FILE.json] [--reps 300] [--path-reps 40]

B = 256, N = 30, H = 256, L = 6, T = 1000, fp32, graph replay, one process; 200 obstacles, 4 pairs, 2 anchors, one 16^3 field and
one 10-row template shared by all molecules.  Wall time of one call, stream synchronised before and after, after 10 untimed calls:
  attach            `Restraints.attach` + `detach` on the topology (hd_restraint_attach, _fields, _templates, _detach: the copies
                    of tables of unchanged sizes)
  energy            `Restraints.energy` on a device tensor (attach, hd_restraint_energy, detach)
  field_energy      `Restraints.field_energy`
  template_energy   `Restraints.template_energy`
  path              `sample_from_masks(steps=4)` with these restraints: attach, rows, four replayed transitions, decode
Per kind: median, quartiles and minimum in microseconds.  Uses the public Python API only, so the same file runs on older commits.
--compare A.json B.json ... : print the medians of several such files side by side."""
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
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--path-reps", type=int, default=40)
    ap.add_argument("--compare", nargs="*", default=None)
    args = ap.parse_args()
    if args.compare:
        files = [json.load(open(f)) for f in args.compare]
        for kind in files[0]["microseconds"]:
            print(f"{kind:16s}", "  ".join(f"{f['microseconds'][kind]['median']:9.1f}" for f in files))
        return 0
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.dynamics import _stream
    from hierdiff_amd.restraints import Field, Restraints, Template
    from hierdiff_amd.weights import synthetic_state_dict

    B, N, H, L, T = 256, 30, 256, 6, 1000
    model = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, timesteps=T))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 1, 1.0).items()})
    model = model.to(DEV).eval()
    model.dynamics.precision = "fp32"
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(0)
    obs = torch.cat([torch.randn(200, 3, generator=g) * 6.0, torch.full((200, 1), 2.0), torch.ones(200, 1)], dim=1)
    rs = Restraints(obstacles=obs, pairs=[[0, 1, 1.0, 2.0, 1.0], [2, 3, 1.0, 2.0, 1.0], [4, 5, 3.0, 4.0, 1.0], [6, 7, 0.0, 5.0, 1.0]],
                    anchors=[[0, 1.0, 0.0, 0.0, 0.5, 1.0], [9, -1.0, 0.0, 0.0, 0.5, 1.0]],
                    fields=Field(torch.randn(16, 16, 16, generator=g), [-8.0, -8.0, -8.0], 16.0 / 15.0, k=1.0),
                    templates=Template(list(range(0, 30, 3)), torch.randn(10, 3, generator=g) * 2.0, k=1.0))
    x = (torch.randn(B, N, 3, generator=g) * 2.0).to(DEV)
    dev = torch.device(DEV)
    topo = model.dynamics.topology(nm, None, B, N)
    scale, nv0 = torch.full((1,), 0.01), float(model.norm_values[0])

    def attach():
        rs.attach(topo, scale, nv0, dev, _stream(dev))
        rs.detach(topo)

    kw = dict(model=model, _attach=(scale, nv0))
    kinds = [("attach", attach, args.reps),
             ("energy", lambda: rs.energy(x, nm, **kw), args.reps),
             ("field_energy", lambda: rs.field_energy(x, nm, **kw), args.reps),
             ("template_energy", lambda: rs.template_energy(x, nm, **kw), args.reps),
             ("path", lambda: model.sample_from_masks(nm, None, None, steps=4, restraints=rs, restraint_scale=0.01, restraint_clip=0.1),
              args.path_reps)]
    res = {"config": dict(B=B, N=N, H=H, L=L, T=T, P=200, Q=4, A=2, field=[16, 16, 16], M=10, reps=args.reps, path_reps=args.path_reps,
                          device=torch.cuda.get_device_name(0)), "microseconds": {}}
    with torch.no_grad():
        for name, call, reps in kinds:
            for _ in range(10):
                call()
            v = sorted(once(call) for _ in range(reps))
            q = statistics.quantiles(v, n=4)
            res["microseconds"][name] = {"median": statistics.median(v), "p25": q[0], "p75": q[2], "min": v[0]}
            print(name, json.dumps(res["microseconds"][name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
