"""What the device loops answer to calls they refuse: the records of tests/golden/loop_refusals.json and the code that makes them
(tests/test_gpu_loop_refusals.py runs it again and compares).

    python -m tests.make_golden_loop_refusals [OUT]     # needs a GPU; rewrites the fixture (or OUT) from the library as it stands

The five sampling entry points (hd_sample_loop, hd_sample_loop_inpaint, hd_sample_path, hd_sample_path_inpaint,
hd_sample_path_guided) and hd_nll_terms at the C ABI, on ONE handle and ONE topology: B = 3, sizes [7, 4, 1], T = 8, hidden 32,
2 layers, one context column, fp32.  The handle is walked through its states - no weights, no schedule, no path / inpainting rows /
terms, everything set, then an attached sink, attached restraints, the other kinds of path, a newer schedule - and in every state each
refusal that state allows is provoked by a call with exactly that one thing wrong; the "two wrong" records are calls with two things wrong, chosen
where two entry points order their checks differently (their names say which answer the order implies).  A record is
[return code, hd_last_error text].  Every call returns before anything is launched: each has something wrong that the library checks
on the host, and `refused` stops at the first call that comes back HD_OK.  All pointers are live device tensors of the right size all
the same.  Not reachable on this handle, so not recorded: "needs a time-conditioned model", "needs a context-conditioned model" (other
configurations) and "N * D floats exceed one workgroup's LDS" (N > 1489).

Behind those states, appended (`attachments`): the argument refusals of hd_set_steer, hd_set_diversity, hd_steer_attach,
hd_diversity_attach and of the single-transition entry points hd_restrain_eps(_framed), hd_restrain_feat, hd_diverse_eps,
hd_steer_step and hd_diversity_energy, called directly; then every refusal of the path loop's ready checks (sink, restraints,
steering, diversity) through each of hd_sample_path, hd_sample_path_inpaint and hd_sample_path_guided that can reach it.  The attach
calls that succeed on the way copy small tables and start a steering chain (one small launch); the refused calls launch nothing.

The fixture records this project's own behaviour; nothing in it comes from the reference."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

DEV = "cuda:0"
T, H, L, N_LIST, F, CTX = 8, 32, 2, [7, 4, 1], 5, 1
B, N, D = len(N_LIST), max(N_LIST), F + 3
K = 4                                                    # transitions of the caller's paths, and scoring terms
SEED, BASE = 99, 10
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_refusals.json")

ENTRY = ("hd_sample_loop", "hd_sample_loop_inpaint", "hd_sample_path", "hd_sample_path_inpaint", "hd_sample_path_guided", "hd_nll_terms")
# the arguments of every entry point in ABI order (h and topo in front); `lo` / `hi` are the range in path order (k_lo, k_hi) - the
# every-step loops take it as (s_hi, s_lo) = (T - lo, T - hi)
_NOISE = "rx rh rows seed base use_graph"
ARGS = {
    "hd_sample_loop": f"z ctx mol_shape s_hi s_lo {_NOISE} stream",
    "hd_sample_loop_inpaint": f"z ctx mol_shape s_hi s_lo {_NOISE} fixed known R stream",
    "hd_sample_path": f"z ctx mol_shape lo hi {_NOISE} stream",
    "hd_sample_path_inpaint": f"z ctx mol_shape lo hi {_NOISE} fixed known R stream",
    "hd_sample_path_guided": f"z ctx ctx_u w w_rows phi lo hi {_NOISE} fixed known R stream",
    "hd_nll_terms": f"xh ctx mol_shape lo hi {_NOISE} acc err stream",
}
INPAINTS = ("hd_sample_loop_inpaint", "hd_sample_path_inpaint")


def f32(*v):
    return (C.c_float * len(v))(*v)


def i32(*v):
    return (C.c_int * len(v))(*v)


def records(lib):
    """{name: [rc, text]} of every refused call, in the order of the walk."""
    from hierdiff_amd._lib import HdConfig
    cfg = HdConfig(in_node_nf=F + 1, context_node_nf=CTX, n_dims=3, hidden_nf=H, n_layers=L, inv_sublayers=2, attention=1, tanh=1,
                   condition_time=1, norm_constant=0.0, normalization_factor=10.0, coords_range=30.0, precision=0, aggregation_mean=0)
    h, other, topo = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, lib.hd_last_error()

    ok(lib.hd_create(C.byref(cfg), 0, C.byref(h)))
    ok(lib.hd_create(C.byref(cfg), 0, C.byref(other)))
    nm = np.zeros((B, N), dtype=np.uint8)
    for b, n in enumerate(N_LIST):
        nm[b, :n] = 1
    ok(lib.hd_topology_create(h, nm.ctypes.data, None, B, N, C.byref(topo)))

    zeros = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    buf = dict(z=zeros(B, N, D), xh=zeros(B, N, D), ctx=zeros(B, N, CTX), ctx_u=zeros(B, N, CTX), w=zeros(B), rx=zeros(K, B, N, 3),
               rh=zeros(K, B, N, F), fixed=zeros(B, N, dtype=torch.uint8), known=zeros(B, N, D), acc=zeros(B, dtype=torch.float64),
               err=zeros(T, B), sink=zeros(2, B, N, D), scale=zeros(1), eps=zeros(B, N, D), out=zeros(B, N, D))
    ptr = {k: v.data_ptr() for k, v in buf.items()}
    out = {}

    def good(entry):
        """A call of `entry` with nothing wrong (once everything is set): transitions 1 .. 3 of the K = 4, or steps 4 .. 7 of T = 8."""
        a = dict(z=ptr["z"], xh=ptr["xh"], ctx=ptr["ctx"], ctx_u=ptr["ctx_u"], w=ptr["w"], w_rows=B, phi=0.5, mol_shape=-1, lo=1, hi=3,
                 rx=None, rh=None, rows=B, seed=SEED, base=BASE, use_graph=1, fixed=None, known=None, R=0, acc=ptr["acc"],
                 err=ptr["err"], stream=None)
        if entry in INPAINTS:
            a.update(fixed=ptr["fixed"], known=ptr["known"], R=2)
        return a

    def refused(name, entry, handle=h, topology=topo, **wrong):
        a = good(entry)
        a.update(wrong)
        a["s_hi"], a["s_lo"] = T - a["lo"], T - a["hi"]
        rc = getattr(lib, entry)(handle, topology, *[a[k] for k in ARGS[entry].split()])
        assert rc != 0, f"{name}: {entry} was not refused"
        assert name not in out, name
        out[name] = [rc, lib.hd_last_error().decode()]

    def every(label, only=ENTRY, **wrong):
        for entry in only:
            refused(f"{entry}|{label}", entry, **wrong)

    loops, paths = ENTRY[:2], ENTRY[2:5]
    with_fixed = dict(fixed=ptr["fixed"], known=ptr["known"], R=2)
    guided_ip = lambda label, **wrong: refused(f"hd_sample_path_guided|inpainting|{label}", "hd_sample_path_guided", **{**with_fixed, **wrong})

    # --- no weights
    every("null handle", handle=None)
    every("null topology", topology=None)
    every("topology of another handle", handle=other)
    every("weights not set")
    refused("two wrong|hd_sample_loop|s_hi > T, weights not set: weights", "hd_sample_loop", lo=-1)
    refused("two wrong|hd_sample_path|k_lo > k_hi, null handle: range", "hd_sample_path", handle=None, lo=3, hi=1)
    refused("two wrong|hd_sample_loop|s_lo > s_hi, null handle: handle", "hd_sample_loop", handle=None, lo=3, hi=1)
    n = lib.hd_weight_count(h)
    blob = (np.random.default_rng(0).standard_normal(n) * 0.05).astype(np.float32)
    ok(lib.hd_set_weights(h, blob.ctypes.data, n, 0, None))

    # --- weights, no schedule
    every("schedule not set")
    refused("two wrong|hd_sample_loop|schedule not set, null z: schedule", "hd_sample_loop", z=None)
    refused("two wrong|hd_sample_path|schedule not set, k_lo > k_hi: range", "hd_sample_path", lo=3, hi=1)
    rows = np.tile(np.array([0.9, 0.3, 0.5, 0.2], dtype=np.float32), (T, 1))
    rows_p = rows.ctypes.data_as(C.POINTER(C.c_float))
    ok(lib.hd_set_schedule(h, T, f32(*np.linspace(0.0, 1.0, T + 1)), rows_p))

    # --- a schedule, nothing else
    refused("hd_sample_loop_inpaint|inpainting schedule not set", "hd_sample_loop_inpaint")
    every("path not set", only=paths)
    refused("hd_nll_terms|terms not set", "hd_nll_terms")
    refused("two wrong|hd_sample_path|path not set, k_hi > K: path", "hd_sample_path", hi=K + 1)
    ok(lib.hd_set_inpaint_schedule(h, T, rows_p))
    t_idx, s_idx = i32(8, 6, 4, 2), i32(6, 4, 2, 0)
    ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 0, rows_p))
    ok(lib.hd_set_nll_terms(h, K, i32(1, 3, 5, 8), rows_p))

    # --- everything set: the arguments
    every("lo < 0", lo=-1)                                                   # (the every-step loops: s_hi > T)
    every("lo > hi", lo=3, hi=1)
    every("hi beyond the end", hi=K + 1, only=paths + ("hd_nll_terms",))
    every("hi beyond the end", hi=T + 1, only=loops)                         # s_lo < 0
    every("null z", z=None, only=ENTRY[:5])
    refused("hd_nll_terms|null xh", "hd_nll_terms", xh=None)
    refused("hd_nll_terms|null acc", "hd_nll_terms", acc=None)
    every("no context", ctx=None)
    plain = ("hd_sample_loop", "hd_sample_path", "hd_sample_path_guided", "hd_nll_terms")
    every("raw_x without raw_h", rx=ptr["rx"], only=plain)
    every("raw_h without raw_x", rh=ptr["rh"], only=plain)
    every("noise_rows 2", rows=2)
    every("noise_rows 1", rows=1, only=INPAINTS + ("hd_nll_terms",))
    every("mol_shape < N", mol_shape=N - 1, only=INPAINTS + ("hd_nll_terms",))
    for entry in INPAINTS:
        refused(f"{entry}|null fixed_mask", entry, fixed=None)
        refused(f"{entry}|null xh_known", entry, known=None)
        refused(f"{entry}|injected noise", entry, rx=ptr["rx"], rh=ptr["rh"])
        refused(f"{entry}|resamplings 0", entry, R=0)
        refused(f"{entry}|draw index overflows", entry, R=0xFFFFFFFF // (3 * (T + 2)) + 1)
    refused("hd_sample_path_guided|null context_u", "hd_sample_path_guided", ctx_u=None)
    refused("hd_sample_path_guided|null w", "hd_sample_path_guided", w=None)
    refused("hd_sample_path_guided|w_rows 2", "hd_sample_path_guided", w_rows=2)
    refused("hd_sample_path_guided|rescale > 1", "hd_sample_path_guided", phi=1.5)
    refused("hd_sample_path_guided|rescale nan", "hd_sample_path_guided", phi=float("nan"))
    guided_ip("fixed_mask without xh_known", known=None)
    guided_ip("injected noise", rx=ptr["rx"], rh=ptr["rh"])
    guided_ip("noise_rows 1", rows=1)
    guided_ip("resamplings 0", R=0)
    guided_ip("draw index overflows", R=0xFFFFFFFF // (3 * (T + 2)) + 1)
    refused("two wrong|hd_sample_path|k_hi > K, null z: range", "hd_sample_path", hi=K + 1, z=None)
    refused("two wrong|hd_sample_loop|s_lo < 0, null z: z", "hd_sample_loop", hi=T + 1, z=None)
    refused("two wrong|hd_sample_path|k_hi > K, noise_rows 2: range", "hd_sample_path", hi=K + 1, rows=2)
    refused("two wrong|hd_nll_terms|k_hi > K, noise_rows 2: rows", "hd_nll_terms", hi=K + 1, rows=2)
    refused("two wrong|hd_nll_terms|k_hi > K, null xh: range", "hd_nll_terms", hi=K + 1, xh=None)
    refused("two wrong|hd_sample_loop_inpaint|s_lo < 0, null fixed_mask: mask", "hd_sample_loop_inpaint", hi=T + 1, fixed=None)
    refused("two wrong|hd_sample_path_guided|w_rows 2, null z: z", "hd_sample_path_guided", w_rows=2, z=None)
    refused("two wrong|hd_sample_path_guided|inpainting, raw_x alone, resamplings 0: noise", "hd_sample_path_guided",
            **{**with_fixed, "rx": ptr["rx"], "R": 0})

    # --- a sink attached (the caller's path records; the every-step loops never do, so they are not asked)
    sink = lambda frames, what: ok(lib.hd_chain_attach(topo, ptr["sink"], frames, what, 1.0, 1.0, 0.0))
    recording = ("hd_sample_path", "hd_sample_path_guided")
    sink(2, 0)
    every("sink attached, chain tables not set", only=recording)
    ok(lib.hd_set_chain(h, K, i32(0, -1, 1, 2), None, 3))
    every("sink of 2 frames, chain tables of 3", only=recording)
    ok(lib.hd_set_chain(h, K, i32(0, -1, 1, -1), None, 2))
    refused("hd_sample_path|sink attached, mol_shape < N", "hd_sample_path", mol_shape=N - 1)
    sink(2, 1)
    every("sink of the data prediction, no alpha / sigma rows", only=recording)
    ok(lib.hd_chain_detach(topo))

    # --- restraints attached (empty tables are enough to be asked)
    ok(lib.hd_restraint_attach(topo, None, 1, 0, None, None, 1, 0, None, None, 1, 0, ptr["scale"], 1, 1.0, None))
    every("restraints attached, rows not set", only=recording)
    refused("hd_sample_path_inpaint|restraints attached", "hd_sample_path_inpaint")
    guided_ip("restraints attached")
    refused("two wrong|hd_sample_path_inpaint|restraints attached, k_hi > K: restraints", "hd_sample_path_inpaint", hi=K + 1)
    refused("two wrong|hd_sample_path_guided|inpainting, restraints attached, k_hi > K: range", "hd_sample_path_guided",
            **{**with_fixed, "hi": K + 1})
    ok(lib.hd_set_restraint(h, K, rows_p))
    refused("hd_sample_path|restraints attached, mol_shape < N", "hd_sample_path", mol_shape=N - 1)
    ok(lib.hd_restraint_detach(topo))

    # --- the other kinds of path
    ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 0, None))
    refused("hd_sample_path_inpaint|path without inpainting rows", "hd_sample_path_inpaint")
    guided_ip("path without inpainting rows")
    ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 1, None))
    refused("hd_sample_path_inpaint|linear rows", "hd_sample_path_inpaint")
    guided_ip("linear rows")
    refused("two wrong|hd_sample_path_inpaint|linear rows, null fixed_mask: rows", "hd_sample_path_inpaint", fixed=None)
    up = np.tile(np.array([1.1, 0.2, 0.0, 0.0], dtype=np.float32), (K, 1))
    ok(lib.hd_set_path_up(h, K, i32(0, 2, 4, 6), i32(2, 4, 6, 8), up.ctypes.data_as(C.POINTER(C.c_float))))
    refused("hd_sample_path_inpaint|ascending path", "hd_sample_path_inpaint")
    guided_ip("ascending path")
    rows5 = np.tile(np.array([0.9, 0.3, 0.1, 0.5, 0.5], dtype=np.float32), (K, 1))
    rows5[0, 2] = 0.0
    ok(lib.hd_set_path_multistep(h, K, t_idx, s_idx, rows5.ctypes.data_as(C.POINTER(C.c_float))))
    refused("hd_sample_path_inpaint|multistep rows", "hd_sample_path_inpaint")
    every("multistep rows, no history for k_lo", only=recording)
    refused("hd_sample_path|multistep rows, no history for k_lo, plain launches", "hd_sample_path", use_graph=0)

    # --- a schedule newer than the path / terms
    ok(lib.hd_set_schedule(h, T, f32(*np.linspace(0.0, 1.0, T + 1)), rows_p))
    every("path older than the schedule", only=paths)
    refused("hd_sample_loop_inpaint|inpainting schedule older than the schedule", "hd_sample_loop_inpaint")
    refused("hd_nll_terms|terms older than the schedule", "hd_nll_terms")

    attachments(lib, h, topo, ptr, out, ok, refused, every, guided_ip, rows_p, (t_idx, s_idx), rows5)

    torch.cuda.synchronize()
    ok(lib.hd_topology_destroy(topo))
    ok(lib.hd_destroy(h))
    ok(lib.hd_destroy(other))
    return out


def attachments(lib, h, topo, ptr, out, ok, refused, every, guided_ip, rows_p, path_idx, rows5):
    """The states behind the older ones: what a caller attaches to the topology for a call - steering, diversity, restraints in the
    known fragments' frame, a sink - and what the path loop says when an attachment does not fit the call; in front of them the
    argument refusals of the setters, the attach calls and the single-transition entry points of these terms.  B = 3 allows groups
    of P = 3 alone.  Not reachable, so not recorded: the path loop's own "restraints are attached ..., and inpainting takes none" (the
    entry points that inpaint refuse it first, in their own words) and hd_diversity_attach's LDS bound (P <= 3 here)."""
    t_idx, s_idx = path_idx
    paths, recording = ENTRY[2:5], ("hd_sample_path", "hd_sample_path_guided")
    inpaint = "hd_sample_path_inpaint"

    def direct(name, fn, *args):
        rc = getattr(lib, fn)(*args)
        assert rc != 0, f"{name}: {fn} was not refused"
        assert name not in out, name
        out[name] = [rc, lib.hd_last_error().decode()]

    rows3 = np.tile(np.array([0.9, 0.3, 1.0], dtype=np.float32), (K, 1))
    rows3_p = rows3.ctypes.data_as(C.POINTER(C.c_float))
    z, eps, dst, known, fixed = ptr["z"], ptr["eps"], ptr["out"], ptr["known"], ptr["fixed"]
    row4, row3 = f32(0.9, 0.3, 0.5, 0.2), f32(0.9, 0.3, 1.0)
    one = f32(1.0)
    rs_on = lambda: ok(lib.hd_restraint_attach(topo, None, 1, 0, None, None, 1, 0, None, None, 1, 0, ptr["scale"], 1, 1.0, None))
    rs_off = lambda: ok(lib.hd_restraint_detach(topo))
    st_on = lambda: ok(lib.hd_steer_attach(topo, B, 0.5, 1, None))
    st_off = lambda: ok(lib.hd_steer_detach(topo))
    dv_on = lambda: ok(lib.hd_diversity_attach(topo, B, 1.0, 1.0, one, 1, 1.0, None))
    dv_off = lambda: ok(lib.hd_diversity_detach(topo))
    fresh_path = lambda: ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 0, rows_p))     # every row table goes stale

    # --- the row setters (the path is still older than the schedule), the attach calls
    for fn, bad_row in (("hd_set_steer", (0.9, 0.3, -1.0)), ("hd_set_diversity", (0.9, 0.3, 0.5, 0.0))):
        rows = rows3_p if fn == "hd_set_steer" else rows_p
        bad = f32(*(bad_row * K))
        direct(f"{fn}|null handle", fn, None, K, rows)
        direct(f"{fn}|null rows", fn, h, K, None)
        direct(f"{fn}|K 0", fn, h, 0, rows)
        direct(f"{fn}|path older than the schedule", fn, h, K, rows)
        fresh_path()
        direct(f"{fn}|K differs from the path's", fn, h, K - 1, rows)
        direct(f"{fn}|bad row", fn, h, K, bad)
        direct(f"two wrong|{fn}|K differs, bad row: K", fn, h, K - 1, bad)
        ok(lib.hd_set_schedule(h, T, f32(*np.linspace(0.0, 1.0, T + 1)), rows_p))
    fresh_path()
    direct("hd_steer_attach|null topology", "hd_steer_attach", None, B, 0.5, 1, None)
    direct("hd_steer_attach|P 1", "hd_steer_attach", topo, 1, 0.5, 1, None)
    direct("hd_steer_attach|P 257", "hd_steer_attach", topo, 257, 0.5, 1, None)
    direct("hd_steer_attach|B no multiple of P", "hd_steer_attach", topo, 2, 0.5, 1, None)
    direct("hd_steer_attach|ess 0", "hd_steer_attach", topo, B, 0.0, 1, None)
    direct("hd_steer_attach|ess > 1", "hd_steer_attach", topo, B, 1.5, 1, None)
    direct("hd_steer_attach|ess nan", "hd_steer_attach", topo, B, float("nan"), 1, None)
    direct("hd_steer_attach|reset 0 without a chain", "hd_steer_attach", topo, B, 0.5, 0, None)
    direct("two wrong|hd_steer_attach|P 1, ess 0: P", "hd_steer_attach", topo, 1, 0.0, 1, None)
    dva = lambda label, *args: direct(f"hd_diversity_attach|{label}", "hd_diversity_attach", *args)
    dva("null topology", None, B, 1.0, 1.0, one, 1, 1.0, None)
    dva("P 1", topo, 1, 1.0, 1.0, one, 1, 1.0, None)
    dva("P 33", topo, 33, 1.0, 1.0, one, 1, 1.0, None)
    dva("B no multiple of P", topo, 2, 1.0, 1.0, one, 1, 1.0, None)
    dva("null scale", topo, B, 1.0, 1.0, None, 1, 1.0, None)
    dva("scale_rows 2", topo, B, 1.0, 1.0, f32(1.0, 1.0), 2, 1.0, None)
    dva("kappa < 0", topo, B, -1.0, 1.0, one, 1, 1.0, None)
    dva("kappa nan", topo, B, float("nan"), 1.0, one, 1, 1.0, None)
    dva("length 0", topo, B, 1.0, 0.0, one, 1, 1.0, None)
    dva("length inf", topo, B, 1.0, float("inf"), one, 1, 1.0, None)
    dva("nv0 0", topo, B, 1.0, 1.0, one, 1, 0.0, None)
    dva("scale nan", topo, B, 1.0, 1.0, f32(float("nan")), 1, 1.0, None)
    direct("two wrong|hd_diversity_attach|kappa < 0, null scale: scale", "hd_diversity_attach", topo, B, -1.0, 1.0, None, 1, 1.0, None)

    # --- the single-transition entry points: nothing attached, then one term after the other
    shifted = eps + 4                                                        # one float into eps
    eps_fns = ("hd_restrain_eps", "hd_restrain_feat", "hd_diverse_eps")
    call = lambda fn, hh=h, tt=topo, zz=z, ee=eps, rr=row4, oo=dst: (fn, hh, tt, zz, ee, rr, oo, None)
    framed = lambda hh=h, zz=z, rr=row4, ff=fixed, kk=known, oo=dst: ("hd_restrain_eps_framed", hh, topo, zz, eps, rr, ff, kk, oo, None)
    steer = lambda hh=h, zz=z, ee=eps, rr=row3: ("hd_steer_step", hh, topo, zz, ee, rr, 5, SEED, BASE, None)
    for fn in eps_fns:
        direct(f"{fn}|null handle", *call(fn, hh=None))
        direct(f"{fn}|null topology", *call(fn, tt=None))
        direct(f"{fn}|null z", *call(fn, zz=None))
        direct(f"{fn}|null row", *call(fn, rr=None))
        direct(f"{fn}|null out", *call(fn, oo=None))
        direct(f"{fn}|nothing attached", *call(fn))
    direct("hd_restrain_eps_framed|null handle", *framed(hh=None))
    direct("hd_restrain_eps_framed|null fixed_mask", *framed(ff=None))
    direct("hd_restrain_eps_framed|null xh_known", *framed(kk=None))
    direct("hd_restrain_eps_framed|nothing attached", *framed())
    direct("hd_steer_step|null handle", *steer(hh=None))
    direct("hd_steer_step|null z", *steer(zz=None))
    direct("hd_steer_step|null row", *steer(rr=None))
    direct("hd_steer_step|nothing attached", *steer())
    direct("hd_diversity_energy|null handle", "hd_diversity_energy", None, topo, z, ptr["acc"], None, None)
    direct("hd_diversity_energy|null x", "hd_diversity_energy", h, topo, None, ptr["acc"], None, None)
    direct("hd_diversity_energy|null phi", "hd_diversity_energy", h, topo, z, None, None, None)
    direct("hd_diversity_energy|nothing attached", "hd_diversity_energy", h, topo, z, ptr["acc"], None, None)
    direct("two wrong|hd_diverse_eps|nothing attached, bad row: diversity", *call("hd_diverse_eps", rr=f32(0.0, 0.3, 0.5, 0.2)))
    st_on()
    direct("hd_steer_step|steering attached, no restraints", *steer())
    direct("two wrong|hd_steer_step|no restraints, bad row: restraints", *steer(rr=f32(0.9, 0.3, -1.0)))
    rs_on()
    direct("hd_steer_step|alpha 0", *steer(rr=f32(0.0, 0.3, 1.0)))
    direct("hd_steer_step|beta < 0", *steer(rr=f32(0.9, 0.3, -1.0)))
    direct("hd_steer_step|eps is z", *steer(ee=z))
    direct("hd_steer_step|eps overlaps z", *steer(ee=z + 4))
    st_off()
    direct("hd_steer_step|restraints attached, no steering", *steer())
    direct("hd_restrain_feat|restraints attached, no features", *call("hd_restrain_feat"))
    dv_on()
    nf = D - 3
    band = lambda v: (C.c_float * nf)(*([v] * nf))
    ok(lib.hd_restraint_features(topo, band(-1.0), band(1.0), band(1.0), 1, 1, None, None, 1, 0, 1.0, 0.0, 1.0, None))
    for fn in eps_fns:
        direct(f"{fn}|alpha 0", *call(fn, rr=f32(0.0, 0.3, 0.5, 0.2)))
        direct(f"{fn}|sigma < 0", *call(fn, rr=f32(0.9, -0.3, 0.5, 0.2)))
        direct(f"{fn}|lambda nan", *call(fn, rr=f32(0.9, 0.3, float("nan"), 0.2)))
        direct(f"{fn}|clip 0", *call(fn, rr=f32(0.9, 0.3, 0.5, 0.0)))
        direct(f"{fn}|out is z", *call(fn, oo=z))
        direct(f"{fn}|out overlaps z", *call(fn, oo=z + 4))
        direct(f"{fn}|out overlaps eps", *call(fn, oo=shifted))
        direct(f"two wrong|{fn}|out is z, out overlaps eps: z", *call(fn, ee=z + 4, oo=z))
    direct("hd_restrain_eps_framed|clip 0", *framed(rr=f32(0.9, 0.3, 0.5, 0.0)))
    direct("hd_restrain_eps_framed|out is z", *framed(oo=z))
    direct("hd_restrain_eps_framed|out is xh_known", *framed(oo=known))
    direct("hd_restrain_eps_framed|out overlaps xh_known", *framed(oo=known + 4))
    direct("hd_restrain_eps_framed|out overlaps eps", *framed(oo=shifted))
    direct("two wrong|hd_restrain_eps_framed|out is xh_known, clip 0: row", *framed(oo=known, rr=f32(0.9, 0.3, 0.5, 0.0)))
    dv_off()
    rs_off()

    # --- the path loop: steering attached (the path is fresh: no rows are set for it)
    st_on()
    every("steering attached, no restraints", only=paths)
    guided_ip("steering attached, no restraints")
    dv_on()
    for entry in paths:
        refused(f"two wrong|{entry}|steering without restraints, diversity attached: steering", entry)
    dv_off()
    rs_on()
    for entry in recording:
        refused(f"two wrong|{entry}|restraint rows not set, steering rows not set: restraints", entry)
    ok(lib.hd_set_restraint(h, K, rows_p))
    every("steering attached, rows not set", only=recording)
    refused("two wrong|hd_sample_path|steering rows not set, noise_rows 1: rows", "hd_sample_path", rows=1)
    ok(lib.hd_set_steer(h, K, rows3_p))
    every("steering attached, noise_rows 1", rows=1, only=recording)
    dv_on()
    for entry in recording:
        refused(f"two wrong|{entry}|diversity and steering attached, diversity rows not set: both", entry)
    ok(lib.hd_set_diversity(h, K, rows_p))
    every("diversity and steering attached", only=recording)
    refused("two wrong|hd_sample_path|diversity and steering attached, noise_rows 1: noise", "hd_sample_path", rows=1)
    dv_off()

    # --- ... and the restraints in the known fragments' frame
    ok(lib.hd_restraint_frame(topo, 1))
    every("framed restraints, no fixed fragments", only=recording)
    refused(f"{inpaint}|framed restraints, steering attached", inpaint)
    guided_ip("framed restraints, steering attached")
    st_off()
    refused("two wrong|hd_sample_path|framed restraints, no fixed fragments, noise_rows 2: rows", "hd_sample_path", rows=2)
    dv_on()
    refused(f"{inpaint}|framed restraints, diversity attached", inpaint)
    guided_ip("framed restraints, diversity attached")
    rs_off()

    # --- diversity attached alone
    refused(f"{inpaint}|diversity attached", inpaint)
    guided_ip("diversity attached")
    refused("hd_sample_path|diversity attached, mol_shape < N", "hd_sample_path", mol_shape=N - 1)
    every("diversity attached, shared noise on a stochastic path", rows=1, only=recording)
    fresh_path()
    every("diversity attached, rows not set", only=recording)
    refused("two wrong|hd_sample_path|diversity rows not set, mol_shape < N: whole molecules", "hd_sample_path", mol_shape=N - 1)
    refused(f"two wrong|{inpaint}|diversity attached, rows not set: inpainting", inpaint)
    dv_off()

    # --- a sink and framed restraints through the entry points that inpaint (the chain tables and the rows are stale)
    sink = lambda frames, what: ok(lib.hd_chain_attach(topo, ptr["sink"], frames, what, 1.0, 1.0, 0.0))
    sink(2, 0)
    refused(f"{inpaint}|sink attached, chain tables not set", inpaint)
    guided_ip("sink attached, chain tables not set")
    rs_on()
    ok(lib.hd_restraint_frame(topo, 1))
    refused(f"two wrong|{inpaint}|chain tables not set, restraint rows not set: sink", inpaint)
    ok(lib.hd_set_chain(h, K, i32(0, -1, 1, 2), None, 3))
    refused(f"two wrong|{inpaint}|sink of 2 frames, chain tables of 3, restraint rows not set: sink", inpaint)
    ok(lib.hd_chain_detach(topo))
    refused(f"{inpaint}|framed restraints, rows not set", inpaint)
    guided_ip("framed restraints, rows not set")
    rs_off()
    sink(2, 0)
    refused(f"{inpaint}|sink of 2 frames, chain tables of 3", inpaint)
    guided_ip("sink of 2 frames, chain tables of 3")
    ok(lib.hd_set_chain(h, K, i32(0, -1, 1, -1), None, 2))
    sink(2, 1)
    refused(f"{inpaint}|sink of the data prediction, no alpha / sigma rows", inpaint)
    guided_ip("sink of the data prediction, no alpha / sigma rows")
    st_on()
    refused("two wrong|hd_sample_path|sink of the data prediction without rows, steering without restraints: sink", "hd_sample_path")
    st_off()
    ok(lib.hd_chain_detach(topo))

    # --- steering on multistep rows, which draw nothing
    ok(lib.hd_set_path_multistep(h, K, t_idx, s_idx, rows5.ctypes.data_as(C.POINTER(C.c_float))))
    rs_on()
    ok(lib.hd_set_restraint(h, K, rows_p))
    ok(lib.hd_set_steer(h, K, rows3_p))
    st_on()
    every("steering attached, multistep rows", lo=0, only=recording)
    refused("two wrong|hd_sample_path|steering attached, multistep rows, noise_rows 1: multistep", "hd_sample_path", lo=0, rows=1)
    st_off()
    rs_off()


def main():
    from hierdiff_amd import _lib
    _lib.require_gpu()
    got = records(_lib.load())
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in got.items()) + "\n}\n")
    print(f"{len(got)} refusals -> {path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
