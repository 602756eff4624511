"""Bits of every Python sampling and scoring entry point, to compare two versions of hierdiff_amd/diffusion.py on the same library,
or two versions of the library.

    python scratch/sampling_bits.py --out profiles/sampling_bits_<name>.json [--root DIR] [--detail FILE]

The matrix of tests/make_golden_dispatch.py (every entry point crossed with steps / eta / solver / guidance / keep_frames + record /
restraints / injected noise / fix_noise / k_lo > 0) run to completion at B = 3, sizes [7, 4, 1], T = 8, hidden 32, 2 layers, synthetic
weights, the model's fixed seed, with `use_graph` on and off.  Per row: SHA-256 of every returned tensor (x, h, chain; of the list
forms x, h, context, chain_x, chain_h, chain_t, restraint_energy over all molecules), or the type of the argument error, and what a second,
warm call of the same row adds to the graph build counters (hd_path_graph_builds, hd_guided_graph_builds, hd_chain_graph_builds,
hd_nll_graph_builds).  Behind the matrix, the scoring loop at the same shape (`scoring_matrix`): DiffusionQM9.nll_full over all terms,
a 4-term uniform list and an explicit subset, with and without the per-term errors and injected noise; the same in two calls of the
term loop, the second from k_lo = 2 (`nll_split`); and `score` on the list form.
Behind the scoring rows, the single-step ABI paths that no loop reaches (`steps_group`): hd_posterior_step at every case of
tests/sampling_reference.py (coef_rows = B, mol_shape < N with out_stride = mol, shared noise, in place), hd_multistep_step and
hd_multistep_sde_step with host rows at the shapes `wrap`, `F1`, `B1`, `pocket` of tests/test_gpu_sde_solver.py and the masks of
tests/test_gpu_solver.py, injected, shared and generated noise, aliased outputs - inputs from those tests' own generators.
Behind them, the loop terms the matrix does not attach (`terms_group`): B = 4, sizes [5, 5, 5, 5] as two groups of 2, steps = 4 on the same
model - steered + restrained, diverse, diverse + restrained + features, recorded diverse - with `use_graph` on and off, hashed as the rows above.
A row the library refuses before it launches anything (solver "dpm2m" from k_lo > 0 without the transition before it) holds
"HD_E_STATE"; any other library error ends the run.
`--out` holds, per `use_graph` value and entry point, the number of rows, how they ended, the warm builds summed, and one SHA-256 over
the rows' records in matrix order - small enough to commit; `--detail FILE` also writes every row's record (862 KB), which is what to
compare when two `--out` files differ.  `--root DIR` runs another checkout (the parent commit).  Two runs agree when their files are
identical."""
import argparse
import hashlib
import json
import os
import sys

import torch

DEV = "cuda:0"
HD_E_STATE = -4                   # include/hierdiff_hip.h
COUNTERS = ("hd_path_graph_builds", "hd_guided_graph_builds", "hd_chain_graph_builds", "hd_nll_graph_builds")


def digest(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(str((tuple(t.shape), str(t.dtype))).encode() + t.numpy().tobytes()).hexdigest()


def digests(got):
    if torch.is_tensor(got):
        return {"z": digest(got)}
    if isinstance(got, tuple):
        return {name: digest(t) for name, t in zip(("x", "h", "chain"), got)}
    return {k: digest(torch.cat([res[k].reshape(-1).double() for res in got])) for k in sorted(got[0])}       # a list: per key


def scoring_matrix():
    """(key, entry, opt) of the scoring rows, in the form of make_golden_dispatch.matrix()."""
    rows = []
    for entry in ("nll_full", "nll_split"):
        for terms in ({}, {"terms": 4}, {"timesteps": [7, 2, 5]}):
            for errors in (False, True):
                for injected in (False, True):
                    opt = dict(terms, return_terms=errors, injected=injected)
                    rows.append((entry + "|" + ",".join(f"{k}={v}" for k, v in opt.items()), entry, opt))
    return rows + [(f"score|{kw}", "score", kw) for kw in ({}, {"terms": 4})]


def score_call(case, entry, opt, graph):
    from tests import edit_reference as er
    m = case.model
    if entry == "score":
        return {"nll": digest(m.score(case.samples, case.device, sample_id_base=3, use_graph=graph, **opt))}
    kw = {k: v for k, v in opt.items() if k in ("terms", "timesteps")}
    K = len(kw.get("timesteps", ())) or kw.get("terms", case.T)
    raws = [(a.to(case.device), b.to(case.device)) for a, b in er.raw_draws(K + 1, case.B, case.N, 5)] if opt["injected"] else None
    args = (case.x, case.h, case.nm, None, case.ctx)
    if entry == "nll_full":
        got = m.nll_full(*args, sample_id_base=3, raw_noises=raws, return_terms=opt["return_terms"], use_graph=graph, **kw)
        nll, err = (got[0], got[1][1]) if opt["return_terms"] else (got, None)
    else:                                                 # the term loop in two calls, the second from k_lo = 2
        st = m._nll_setup(*args, kw.get("terms"), kw.get("timesteps"), None, 3, raws, opt["return_terms"], graph)
        m._nll_terms(st, 0, 2)
        m._nll_terms(st, 2, st.K)
        nll, err = m._nll_finish(st), st.err
    return {"nll": digest(nll)} if err is None else {"nll": digest(nll), "err": digest(err)}


def steps_group():
    """{row name: {tensor: sha256}} of the three single-step functions, straight at the C ABI."""
    import ctypes as C

    import numpy as np
    from oracle import egnn_oracle as orc
    from tests import sampling_reference as smp
    from tests import sde_solver_reference as sd
    from tests import solver_reference as sol
    from tests import test_gpu_sampling_kernels as tk
    from tests import test_gpu_sde_solver as ts
    from tests import test_gpu_solver as tm
    from tests.test_gpu_restraint import Bare

    out = {}
    from hierdiff_amd import _lib
    lib = _lib.load()
    cases = smp.cases()
    for name in smp.STEP_CASES:                                                    # hd_posterior_step
        c = cases[name]
        h = C.c_void_p()
        cfg = tk.make_config(c["F"])
        assert lib.hd_create(C.byref(cfg), 0, C.byref(h)) == 0, lib.hd_last_error()
        with tk.topology(lib, h, c["nm"]) as topo:
            for in_place in ((False, True) if c["mol"] == c["N"] else (False,)):
                out[f"hd_posterior_step|{name}|in_place={int(in_place)}"] = {"zs": digest(torch.from_numpy(tk.device_step(lib, h, topo, c, in_place)))}
        assert lib.hd_destroy(h) == 0
    T, K = ts.T, ts.K
    path = sd.uniform_path(T, K)
    rows6 = sd.sde_rows(sd.analytic_grid(T), path, lower_order_final=False)
    rows5 = sol.multistep_rows(sol.analytic_grid(T), sol.uniform_path(T, K), lower_order_final=False)
    shapes = {name: ts.kernel_case(name) for name in ("wrap", "F1", "B1", "pocket")}
    for name, sizes in tm.MASKS.items():
        shapes[name] = (orc.canonical_masks(sizes)[0].bool().reshape(len(sizes), -1), 8, None)
    for name, (nm, F, mol) in shapes.items():
        B, N = nm.shape
        n = N if mol is None else mol
        zt, eps, xp = ts.kernel_inputs(nm, F, 1)
        g = torch.Generator().manual_seed(2)
        raw_b = (torch.randn(B, n, 3, generator=g), torch.randn(B, n, F, generator=g))
        sources = [("injected", raw_b, B, 0), ("shared row", (raw_b[0][:1], raw_b[1][:1]), 1, 0), ("generator", None, B, 0),
                   ("generator, shared", None, B, 1)]
        bare = Bare(3 + F, nm)
        topo = argparse.Namespace(ptr=bare.topo)
        try:
            for k in (0, 3, K - 1):
                hist = None if k == 0 else xp
                for in_place in (False, True):                                     # hd_multistep_step (no mol_shape: whole molecules)
                    xk, zs = tm.step_on_device(lib, bare.h, topo, tm.f32(rows5[k]), ts.dev(zt), ts.dev(eps), ts.dev(hist), in_place)
                    torch.cuda.synchronize()
                    out[f"hd_multistep_step|{name}|row {k}|in_place={int(in_place)}"] = {"x": digest(xk), "zs": digest(zs)}
                if name not in tm.MASKS:
                    for what, raw, noise_rows, share in sources:                   # hd_multistep_sde_step
                        for alias in ((False, True) if mol is None else (False,)):
                            xk, zs = ts.sde_step(bare, ts.f32(rows6[k]), zt, eps, hist, raw, noise_rows, mol, share, alias=alias)
                            out[f"hd_multistep_sde_step|{name}|row {k}|{what}|alias={int(alias)}"] = {"x": digest(xk), "zs": digest(zs)}
        finally:
            bare.close()
    return out


def terms_group(case):
    """{row name: {tensor: sha256}} of the steered and diverse calls, `use_graph` on and off."""
    from hierdiff_amd.diversity import Diversity
    from hierdiff_amd.restraints import Features, FeatureSum, Restraints
    m = case.model
    B, N, F = 4, 5, int(m.in_node_nf)
    nm = torch.ones(B, N, 1, dtype=torch.bool, device=case.device)
    ctx = torch.tensor([0.25, 0.25, -0.5, -0.5], device=case.device).reshape(B, 1, 1).expand(B, N, 1).contiguous()
    rs = lambda **kw: Restraints(obstacles=[[0.0, 0.0, 0.0, 1.0, 1.0]], pairs=[[0, 1, 0.5, 1.5, 1.0]], anchors=[[0, 0.0, 0.0, 0.0, 0.5, 1.0]], **kw)
    feat = Features(lo=[[-0.5] * F] * 2, hi=[[0.5] * F] * 2, k=1.0, sums=[FeatureSum([1.0] * F, lo=-1.0, hi=1.0, reduce="mean")])
    dv = lambda: Diversity(particles=2, length=1.0, strength=4.0, scale=[1.0, 0.5], clip=0.3)
    kinds = {
        "steered+restrained": lambda: dict(restraints=rs(), restraint_scale=0.5, restraint_clip=0.3, particles=2, steer_scale=1.0, eta=1.0),
        "diverse": lambda: dict(diversity=dv()),
        "diverse+restrained+features": lambda: dict(diversity=dv(), restraints=rs(features=feat), restraint_scale=0.5, restraint_clip=0.3),
        "recorded diverse": lambda: dict(diversity=dv(), keep_frames=2),
    }
    out = {}
    for graph in (True, False):
        m.use_graph = graph
        for kind, kw in kinds.items():
            for call in ("first", "second"):
                got = m.sample_from_masks(nm, None, ctx, sample_id_base=3, steps=4, **kw())
                torch.cuda.synchronize()
                out[f"graph={int(graph)}|{kind}|{call}"] = digests(got)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--detail", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from hierdiff_amd import _lib
    from tests import make_golden_dispatch as gd

    case = gd.Case(T=8, device=DEV)
    lib = _lib.load()
    # (the counters belong to the topology; every row runs on the masks of sizes [7, 4, 1], which the dynamics caches by content)
    counters = lambda m: [int(getattr(lib, c)(m.dynamics.topology(case.nm, None, case.B, case.N).ptr)) for c in COUNTERS]
    res = {"config": dict(B=3, sizes=gd.N_LIST, T=8, H=gd.H, L=gd.L, seed=case.model.seed), "rows": {}}
    for graph in (True, False):
        case.model.use_graph = case.edm.use_graph = graph
        for key, entry, opt in gd.matrix() + scoring_matrix():
            m = case.edm if entry.startswith("edm_") else case.model
            name = f"graph={int(graph)}|{key}"
            run = (lambda: score_call(case, entry, opt, graph)) if entry in ("nll_full", "nll_split", "score") else \
                (lambda: digests(case.call(entry, opt)))
            try:
                first = run()
                before = counters(m)
                second = run()
                row = {"sha256": first, "warm_builds": [a - b for a, b in zip(counters(m), before)]}
                if second != first:
                    row["second_call_differs"] = second
            except (ValueError, NotImplementedError) as e:
                row = {"error": type(e).__name__}
            except _lib.HierDiffHipError as e:        # only the state refusal, raised before anything is launched; all else ends the run
                if f"({HD_E_STATE})" not in str(e) or "multistep path" not in str(e):
                    raise
                row = {"error": "HD_E_STATE"}
            res["rows"][name] = row
        torch.cuda.synchronize()
        print(f"use_graph={graph}: {len(res['rows'])} rows", flush=True)
    for name, sha in steps_group().items():
        res["rows"][f"steps|{name.split('|')[0]}|{name}"] = {"sha256": sha}
    print(f"steps: {len(res['rows'])} rows", flush=True)
    for name, sha in terms_group(case).items():
        res["rows"][f"terms|sample_from_masks|{name}"] = {"sha256": sha}
    print(f"terms: {len(res['rows'])} rows", flush=True)
    groups = {}
    for name, row in res["rows"].items():
        g = groups.setdefault("|".join(name.split("|")[:2]), {"rows": 0, "ended": {}, "warm_builds": [0] * len(COUNTERS), "sha256": hashlib.sha256()})
        g["rows"] += 1
        end = row.get("error", "completed")
        g["ended"][end] = g["ended"].get(end, 0) + 1
        g["warm_builds"] = [a + b for a, b in zip(g["warm_builds"], row.get("warm_builds", [0] * len(COUNTERS)))]
        g["sha256"].update((name + json.dumps(row, sort_keys=True)).encode())
    for g in groups.values():
        g["sha256"] = g["sha256"].hexdigest()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write('{"config": ' + json.dumps(res["config"]) + ',\n"entry_points": {\n' + ",\n".join(
            f"{json.dumps(k)}: {json.dumps(g)}" for k, g in groups.items()) + "\n}}\n")
    if args.detail:
        with open(args.detail, "w") as fh:
            fh.write("{\n" + json.dumps("config") + ": " + json.dumps(res["config"]) + ",\n\"rows\": {\n" + ",\n".join(
                f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in res["rows"].items()) + "\n}}\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
