"""Randomised gradient sweep of ONE stage-2 layer E_GCL under autograd (hd_egcl_forward_train / hd_egcl_backward through
hierdiff_amd.stage2.E_GCL) against torch.autograd through the CPU oracle (oracle/egnn_oracle.py:e_gcl_forward) evaluated in FLOAT64.
usage: fuzz_egcl_grads.py [cases] [seed] [big] [--oracle-only]

Per case: H in {32, 64, 128, 256}, De in {1, 2, 4, H}, ctx in {0, 2}, attention / edge_update (De == H) / coord_update / recurrent /
tanh, geo (no self edges then, every edge with radial >= 0.05), node / edge mask present or not; graphs: dense per-molecule blocks with
the canonical masks, sparse without self edges, sparse with repeats and self edges, "ragged" (nodes that only send, only receive or do
neither, and one hub node on at least a third of all edges).  Upstream: random weights on h_out, x_out, edge_attr_out - in a third of
the cases on one of them only (autograd then hands zeros for the others); edge_attr.requires_grad on / off (dedge_attr NULL).
Default tier: M in 1..40 (case 0: M = 1 with self edges only), E in 1..4M.
"big": E around the sizes at which hd_egcl_backward changes path - 500..530 (split-K starts at 512 rows), 1000..1100, 8150..8250
(the split reaches its cap of 32 slabs), 20,000..30,000 - with M from about 20 to about 1,100 (the node-level weight gradients split
at M >= 512); every odd case has E % 4 != 0.
Bars (tests/test_gpu_stage2_training.py:_close): every parameter gradient, dh, dx, dedge_attr: |diff| <= 1e-4 |ref| + 1e-7 scale
sqrt(size), scale = the largest parameter-gradient element of the reference; forward values rel-L2 <= 1e-5.  Rows of masked-out nodes
are compared like all others.  No case is skipped or excused: any exception is a failure.
--oracle-only (no GPU): the float32 oracle's gradients against the float64 oracle's on the same cases, at ONE TENTH of the bars -
the inputs, not the kernel, never eat the tolerance."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from oracle import egnn_oracle as orc

DEV = "cuda:0"
TOL, FLOOR, VTOL = 1e-4, 1e-7, 1e-5
BANDS = [(500, 530), (1000, 1100), (8150, 8250), (20000, 30000)]
MIN_RADIAL = 0.05


# ----------------------------------------------------------------------------- graphs
def dense_graph(bs, n):
    """All pairs incl. self edges within each of bs blocks of n nodes."""
    return orc.edge_index(n, bs)


def sparse_graph(rng, M, E, self_edges):
    """E random edges; with self_edges: repeats and self edges as they fall, else row != col (needs M >= 2; repeats stay)."""
    row = rng.integers(0, M, size=E)
    col = rng.integers(0, M, size=E) if self_edges else (row + rng.integers(1, M, size=E)) % M
    return torch.from_numpy(row), torch.from_numpy(col)


def ragged_graph(rng, M, E, self_edges):
    """Nodes that send nothing, receive nothing or do neither, and a hub (node `hub`, sends and receives) on >= 40 % of the edges.
    Needs M >= 6."""
    perm = rng.permutation(M)
    q = max(1, M // 5)
    only_send, only_recv = perm[:q], perm[q:2 * q]      # perm[2q:3q]: isolated
    both = perm[3 * q:]
    hub = int(both[0])
    senders, receivers = np.concatenate([only_send, both]), np.concatenate([only_recv, both])
    nh = (2 * E + 4) // 5
    row = senders[rng.integers(0, len(senders), size=E)]
    col = receivers[rng.integers(0, len(receivers), size=E)]
    out = rng.random(nh) < 0.5
    row[:nh] = np.where(out, hub, row[:nh])
    col[:nh] = np.where(out, col[:nh], hub)
    if not self_edges:
        others_r, others_s = receivers[receivers != hub], senders[senders != hub]
        for _ in range(64):
            bad = np.nonzero(row == col)[0]
            if bad.size == 0:
                break
            isrow = rng.random(bad.size) < 0.5           # re-draw one end from the lists without the hub: the hub keeps its share
            fix_c = (row[bad] == hub) | ~isrow
            col[bad] = np.where(fix_c, others_r[rng.integers(0, len(others_r), size=bad.size)], col[bad])
            row[bad] = np.where(fix_c, row[bad], others_s[rng.integers(0, len(others_s), size=bad.size)])
        assert not (row == col).any()
    order = rng.permutation(E)
    return torch.from_numpy(row[order].astype(np.int64)), torch.from_numpy(col[order].astype(np.int64))


def well_separated(rng, M, row, col):
    """Coordinates with |x[row] - x[col]|^2 >= MIN_RADIAL on every edge (geo: the message model sees 1 / radial^2): the ends of a
    short edge are drawn again until none is left."""
    x = rng.standard_normal((M, 3)).astype(np.float32)
    r, c = row.numpy(), col.numpy()
    for _ in range(1000):
        d = x[r] - x[c]
        short = (d * d).sum(1) < 1.2 * MIN_RADIAL
        if not short.any():
            return torch.from_numpy(x)
        again = np.unique(r[short])
        x[again] = rng.standard_normal((again.size, 3)).astype(np.float32)
    raise RuntimeError("no well separated coordinates found")


# ----------------------------------------------------------------------------- cases
def make_case(rng, *, H, De, ctx=0, att=True, eu=True, cu=True, rec=True, tanh=True, geo=False, M, row, col, nm=None, em=None,
              weight_seed=0, only=None, ea_grad=True, kind="given"):
    """A case from a configuration and a graph: weights, inputs and upstream weights drawn from rng.  nm / em: None, a tensor, or
    True = random 80 % masks.  only: None = every output weighted, or the index (indices) of the weighted output(s)."""
    from hierdiff_amd.stage2 import synthetic_egcl_state_dict
    assert not eu or De == H
    E = int(row.numel())
    sd = synthetic_egcl_state_dict(H, De, ctx, att, eu, weight_seed, coord_gain=0.3)
    if not cu:
        sd = {k: v for k, v in sd.items() if not k.startswith("coord_mlp")}
    if nm is True:
        nm = torch.from_numpy((rng.random((M, 1)) > 0.2).astype(np.float32))
    if em is True:
        em = torch.from_numpy((rng.random((E, 1)) > 0.2).astype(np.float32))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    c = dict(H=H, De=De, ctx=ctx, att=att, eu=eu, cu=cu, rec=rec, tanh=tanh, geo=geo, M=M, E=E, kind=kind, row=row.long(), col=col.long(),
             nm=nm, em=em, sd=sd, only=only, ea_grad=ea_grad)
    c["h"] = f(M, H + ctx)
    c["x"] = well_separated(rng, M, row, col) if geo else f(M, 3)
    c["ea"] = f(E, De)
    c["ups"] = [f(M, H + ctx), f(M, 3)] + ([f(E, H)] if eu else [])
    assert only is None or max((only,) if isinstance(only, int) else only) < len(c["ups"])
    return c


def draw_case(seed, case, big):
    """Case number `case` of the sweep with this seed: its own generator, so that one case can be re-run alone."""
    rng = np.random.Generator(np.random.PCG64([int(seed), int(case), int(big)]))
    H = int(rng.choice([32, 64, 128, 256]))
    wide = bool(rng.integers(0, 2))
    De = H if wide else int(rng.choice([1, 2, 4]))
    ctx = int(rng.choice([0, 2]))
    att, eu = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)) and wide
    cu, rec, tanh = bool(rng.integers(0, 2)), bool(rng.random() < 0.8), bool(rng.integers(0, 2))
    geo = bool(rng.random() < 0.25)
    kind = int(rng.integers(0, 4))                    # 0 dense blocks, 1 sparse no self edges, 2 sparse repeats + self, 3 ragged
    masked, has_em = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    nm, em = (True if masked else None), (True if has_em else None)
    if not big:
        M = 1 if case == 0 else int(rng.integers(1, 41))
        E = int(rng.integers(1, 4 * M + 1))
        if M == 1:
            geo, kind = False, 2                      # self edges only
    else:
        lo, hi = BANDS[case % 4]
        E = int(rng.integers(lo, hi + 1))
        if case % 2 == 1 and E % 4 == 0:
            E += 1                                    # every odd case: E neither a multiple of 4 nor of 32
        sizes, pick = [rng.integers(20, 41), rng.integers(200, 512), rng.integers(512, 1101)], int(rng.integers(0, 3))
        # (20,000..30,000 edges on 20..40 nodes: a node then sums thousands of O(1) messages, and the float32 ORACLE itself misses one
        # tenth of the value bar - measured 1.03e-6 at M = 39, E = 28,503 - so the smallest M go with the bands up to 8,250 edges)
        M = int(sizes[max(pick, 1) if case % 4 == 3 else pick])
        if kind == 0 and case % 4 != 3:
            kind = 3                                  # dense blocks only in the 20,000..30,000 band (whole molecules of 25..35 nodes)
    if geo and kind in (0, 2):
        kind = 1                                      # 1 / radial^2: no self edges
    if kind == 3 and M < 6:
        kind = 1 if geo else 2
    if M < 2:
        geo, kind = False, 2
    if kind == 0:
        if big:
            n = int(rng.integers(25, 36)); bs = max(1, E // (n * n))
        else:
            bs = int(rng.integers(1, 5)); n = max(1, M // bs)
        M = bs * n
        row, col = dense_graph(bs, n)
        if masked or has_em:                          # the canonical masks of a batch of molecules with n_i <= n atoms
            nmb, emb = orc.canonical_masks([int(rng.integers(1, n + 1)) for _ in range(bs)], n)
            nm = nmb.reshape(-1, 1).float() if masked else None
            em = emb.reshape(-1, 1).float() if has_em else None
    elif kind == 3:
        row, col = ragged_graph(rng, M, E, self_edges=not geo)
    else:
        row, col = sparse_graph(rng, M, E, self_edges=kind == 2)
    n_out = 3 if eu else 2
    only = int(rng.integers(0, n_out)) if rng.random() < 1 / 3 else None
    ea_grad = bool(rng.integers(0, 2))
    kinds = ["dense", "sparse", "sparse+self", "ragged"]
    return make_case(rng, H=H, De=De, ctx=ctx, att=att, eu=eu, cu=cu, rec=rec, tanh=tanh, geo=geo, M=M, row=row, col=col, nm=nm, em=em,
                     weight_seed=9000 + 10 * case + (5 if big else 0), only=only, ea_grad=ea_grad, kind=kinds[kind])


def describe(c):
    only = "all" if c["only"] is None else ("h", "x", "ea")[c["only"]] if isinstance(c["only"], int) else "+".join(("h", "x", "ea")[i] for i in c["only"])
    return (f"H={c['H']:3d} De={c['De']:3d} ctx={c['ctx']} att={int(c['att'])} eu={int(c['eu'])} cu={int(c['cu'])} rec={int(c['rec'])} "
            f"tanh={int(c['tanh'])} geo={int(c['geo'])} M={c['M']:4d} E={c['E']:5d} graph={c['kind']:11s} nm={int(c['nm'] is not None)} "
            f"em={int(c['em'] is not None)} up={only:3s} dea={int(c['ea_grad'])}")


# ----------------------------------------------------------------------------- the two sides
def _loss(outs, ups, only, cast):
    sel = range(len(outs)) if only is None else ((only,) if isinstance(only, int) else tuple(only))
    return sum((outs[i] * cast(ups[i])).sum() for i in sel)


def oracle_grads(c, dtype=torch.float64):
    """(outputs, gradients by name) of torch.autograd through the oracle in `dtype`: 'h', 'x', 'edge_attr' (if asked for) and every
    parameter by its state_dict key."""
    cfg = orc.EGCLCfg(hidden_nf=c["H"], edges_in_d=c["De"], context_nf=c["ctx"], attention=c["att"], tanh=c["tanh"], coords_range=30.0,
                      coord_update=c["cu"], edge_update=c["eu"], recurrent=c["rec"], geo=c["geo"])
    cast = lambda t: t.to(dtype)

    def run():
        sd = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in c["sd"].items()}
        h, x = cast(c["h"]).requires_grad_(True), cast(c["x"]).requires_grad_(True)
        ea = cast(c["ea"]).requires_grad_(c["ea_grad"])
        outs = [o for o in orc.e_gcl_forward(sd, cfg, h, c["row"], c["col"], x, ea, c["nm"], c["em"]) if o is not None]
        assert all(o.dtype == dtype for o in outs), [o.dtype for o in outs]
        _loss(outs, c["ups"], c["only"], cast).backward()
        z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad        # (an input with no path to the weighted outputs)
        grads = {"h": z(h), "x": z(x)}
        if c["ea_grad"]:
            grads["edge_attr"] = z(ea)
        grads.update({k: z(v) for k, v in sd.items()})
        return [o.detach() for o in outs], grads
    if dtype == torch.float64:
        with orc.float64():
            return run()
    return run()


def hip_layer(c):
    from hierdiff_amd.stage2 import E_GCL
    H = c["H"]
    m = E_GCL(H, H, H, context_nf=c["ctx"], edges_in_d=c["De"], attention=c["att"], tanh=c["tanh"], coords_range=30, edge_update=c["eu"],
              coord_update=c["cu"], recurrent=c["rec"], geo=c["geo"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["sd"].items()})            # strict: the same set of keys
    return m.to(DEV)


def hip_grads(c, m=None):
    """The same through hierdiff_amd.stage2.E_GCL on the GPU.  Outputs that carry no weight stay out of the loss: autograd hands the
    backward zeros for them."""
    m = hip_layer(c) if m is None else m
    g = lambda t: None if t is None else t.to(DEV)
    h, x = c["h"].to(DEV).requires_grad_(True), c["x"].to(DEV).requires_grad_(True)
    ea = c["ea"].to(DEV).requires_grad_(c["ea_grad"])
    outs = m(h, [g(c["row"]), g(c["col"])], x, edge_attr=ea, node_mask=g(c["nm"]), edge_mask=g(c["em"]))
    m.zero_grad(set_to_none=True)
    _loss(outs, c["ups"], c["only"], g).backward()
    grads = {"h": h.grad, "x": x.grad}
    if c["ea_grad"]:
        grads["edge_attr"] = ea.grad
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        grads[k] = p.grad
    return [o.detach().cpu() for o in outs], {k: v.detach().cpu() for k, v in grads.items()}


def grad_scale(c, ref):
    return max(float(ref[k].abs().max()) for k in c["sd"])


def compare(c, got, ref, factor=1.0):
    """(names that miss their bar, worst rel-L2 of a gradient above the absolute floor, worst rel-L2 of a forward value)."""
    (gouts, ggr), (routs, rgr) = got, ref
    bad, worst, vworst = [], 0.0, 0.0
    if len(gouts) != len(routs) or set(ggr) != set(rgr):
        return ["structure"], float("nan"), float("nan")
    for i, (a, b) in enumerate(zip(gouts, routs)):
        a, b = a.double(), b.double()
        r = float((a - b).norm() / max(float(b.norm()), 1e-30))
        vworst = max(vworst, r)
        if not r <= VTOL * factor:
            bad.append(f"value{i}")
    scale = grad_scale(c, rgr)
    for k, r in rgr.items():
        r = r.double().numpy(); a = ggr[k].double().numpy()
        if a.shape != r.shape:
            bad.append(k + ":shape"); continue
        err, nr = np.linalg.norm(a - r), np.linalg.norm(r)
        floor = FLOOR * scale * np.sqrt(max(r.size, 1))
        if not err <= factor * (TOL * nr + floor):
            bad.append(k)
        if TOL * nr > floor:
            worst = max(worst, err / nr)
    return bad, worst, vworst


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    oracle_only = "--oracle-only" in argv
    cases = int(args[0]) if len(args) > 0 else 40
    seed = int(args[1]) if len(args) > 1 else 17
    big = len(args) > 2 and args[2] == "big"
    factor = 0.1 if oracle_only else 1.0
    fails, worst_all, vworst_all = 0, 0.0, 0.0
    t0 = time.time()
    for case in range(cases):
        c = draw_case(seed, case, big)
        line = f"case {case:3d} " + describe(c)
        try:
            ref = oracle_grads(c, torch.float64)
            got = oracle_grads(c, torch.float32) if oracle_only else hip_grads(c)
            bad, worst, vworst = compare(c, got, ref, factor)
        except Exception as exc:                    # nothing is excused: a combination the layer refuses is a failure too
            bad, worst, vworst = [f"{type(exc).__name__}: {str(exc)[:120]}"], float("nan"), float("nan")
        fails += int(bool(bad))
        worst_all, vworst_all = max(worst_all, worst), max(vworst_all, vworst)      # (NaN compares false: counted through `bad`)
        print(line + f"  value {vworst:.1e} worst grad {worst:.1e}{' FAIL ' + ','.join(bad) if bad else ''}", flush=True)
    what = "float32 oracle vs float64 oracle at 0.1 x bars" if oracle_only else "HIP vs float64 oracle"
    print(f"{'big' if big else 'default'} tier, seed {seed}, {what}: {cases} cases in {time.time() - t0:.0f} s, failures {fails}, skipped 0, "
          f"worst gradient rel-L2 {worst_all:.2e}, worst value rel-L2 {vworst_all:.2e}")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
