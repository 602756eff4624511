"""What the path and row setters answer to calls they refuse: the records of tests/golden/setter_refusals.json and the code that makes
them (tests/test_gpu_setter_refusals.py runs it again and compares).

    python -m tests.make_golden_setter_refusals [OUT]     # needs a GPU; rewrites the fixture (or OUT) from the library as it stands

hd_set_path, hd_set_path_up, hd_set_path_multistep, hd_set_path_multistep_sde, hd_set_restraint, hd_set_steer and the row checks of
hd_restrain_eps at the C ABI, on ONE handle and ONE topology: B = 2, N = 4, T = 8, hidden 32, 2 layers, fp32, no weights (no setter
asks for them).  The handle is walked through its states - no schedule, a schedule and no path, a path, a schedule newer than the
path - and in every state each refusal that state allows is provoked by a call with exactly that one thing wrong; the "two wrong"
records are calls with two things wrong, which pin the order of the checks (their names say which answer the order implies).  A record
is [return code, hd_last_error text].  Every call returns before anything is launched or uploaded: each has something wrong that the
library checks on the host, and `refused` stops at the first call that comes back HD_OK.

The fixture records this project's own behaviour; nothing in it comes from the reference."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

DEV = "cuda:0"
T, H, L, F = 8, 32, 2, 5
B, N, D = 2, 4, F + 3
K = 4
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "setter_refusals.json")

DOWN = ("hd_set_path", "hd_set_path_multistep", "hd_set_path_multistep_sde")      # the setters of descending paths
PATHS = DOWN + ("hd_set_path_up",)
ROWS = ("hd_set_restraint", "hd_set_steer")
ENTRY = PATHS + ROWS + ("hd_restrain_eps",)
# a row of every table with nothing wrong (the multistep ones: row 0, whose c2 is 0)
ROW = {"hd_set_path": [0.9, 0.3, 0.5, 0.2], "hd_set_path_up": [1.1, 0.2, 0.0, 0.0], "hd_set_path_multistep": [0.9, 0.3, 0.0, 0.5, 0.5],
       "hd_set_path_multistep_sde": [0.9, 0.3, 0.2, 0.0, 0.5, 0.5], "hd_set_restraint": [0.9, 0.3, 0.5, float("inf")],
       "hd_set_steer": [0.9, 0.3, 0.5]}
INF, NAN = float("inf"), float("nan")


def i32(v):
    return (C.c_int * len(v))(*v)


def table(entry, k, edits=()):
    """[k][width] float rows of `entry`, all good but for `edits`: (row, column, value)."""
    r = np.tile(np.array(ROW[entry], dtype=np.float32), (k, 1))
    for row, col, val in edits:
        r[row, col] = val
    return r


def records(lib):
    """{name: [rc, text]} of every refused call, in the order of the walk."""
    from hierdiff_amd._lib import HdConfig
    cfg = HdConfig(in_node_nf=F + 1, context_node_nf=1, n_dims=3, hidden_nf=H, n_layers=L, inv_sublayers=2, attention=1, tanh=1,
                   condition_time=1, norm_constant=0.0, normalization_factor=10.0, coords_range=30.0, precision=0, aggregation_mean=0)
    h, topo = C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, lib.hd_last_error()

    ok(lib.hd_create(C.byref(cfg), 0, C.byref(h)))
    nm = np.ones((B, N), dtype=np.uint8)
    nm[1, 3] = 0
    ok(lib.hd_topology_create(h, nm.ctypes.data, None, B, N, C.byref(topo)))
    buf = {k: torch.zeros(B, N, D, device=DEV) for k in ("z", "eps", "out")}
    scale = torch.zeros(1, device=DEV)
    out = {}
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def refused(name, entry, handle=h, k=K, t=None, s=None, edits=(), rows=True, form=0, ip=False, null=()):
        """One call of the setter `entry`: `t` / `s` the departures / arrivals (hd_set_path_up: from / to; None: a good path), `rows`
        False a null table, `null` the index arrays to pass as null, `ip` inpainting rows (hd_set_path)."""
        up = entry == "hd_set_path_up"
        t = t if t is not None else ((0, 2, 4, 6) if up else (8, 6, 4, 2))
        s = s if s is not None else ((2, 4, 6, 8) if up else (6, 4, 2, 0))
        n = max(k, len(t), 1)
        r = table(entry, n, edits)
        a = [handle, k]
        if entry in PATHS:
            t, s = list(t) + [0] * (n - len(t)), list(s) + [0] * (n - len(s))
            a += [None if "t" in null else i32(t), None if "s" in null else i32(s)]
        a.append(fp(r) if rows else None)
        if entry == "hd_set_path":
            a += [form, fp(table(entry, n)) if ip else None]
        rc = getattr(lib, entry)(*a)
        assert rc != 0, f"{name}: {entry} was not refused"
        assert name not in out, name
        out[name] = [rc, lib.hd_last_error().decode()]

    def every(label, only, **wrong):
        two = "two wrong|"
        for entry in only:
            refused(f"{two}{entry}|{label[len(two):]}" if label.startswith(two) else f"{entry}|{label}", entry, **wrong)

    def eps_refused(name, row4, topology=topo, out_buf="out"):
        r = np.array(row4, dtype=np.float32)
        rc = lib.hd_restrain_eps(h, topology, buf["z"].data_ptr(), buf["eps"].data_ptr(), fp(r), buf[out_buf].data_ptr(), None)
        assert rc != 0, f"{name}: hd_restrain_eps was not refused"
        assert name not in out, name
        out[name] = [rc, lib.hd_last_error().decode()]

    # --- no schedule
    every("schedule not set", PATHS)
    every("path not set, no schedule", ROWS)
    refused("hd_set_path|form 2", "hd_set_path", form=2)
    refused("hd_set_path|form -1", "hd_set_path", form=-1)
    refused("hd_set_path|linear rows with inpainting rows", "hd_set_path", form=1, ip=True)
    refused("two wrong|hd_set_path|form 2, null handle: form", "hd_set_path", form=2, handle=None)
    refused("two wrong|hd_set_path|linear rows with inpainting rows, K 0: inpainting rows", "hd_set_path", form=1, ip=True, k=0)
    refused("two wrong|hd_set_path|schedule not set, ascending transition: schedule", "hd_set_path", t=(8, 6, 2, 4), s=(6, 2, 4, 0))
    refused("two wrong|hd_set_path_up|schedule not set, rows draw: rows", "hd_set_path_up", edits=[(1, 2, 0.5)])
    refused("two wrong|hd_set_path_up|null handle, descending transition: transition", "hd_set_path_up", handle=None,
            t=(0, 4, 2, 6), s=(4, 2, 6, 8))
    refused("two wrong|hd_set_path_up|null handle, K 0: argument", "hd_set_path_up", handle=None, k=0)
    refused("two wrong|hd_set_path_multistep|schedule not set, c2 of row 0: schedule", "hd_set_path_multistep", edits=[(0, 2, 0.1)])
    refused("two wrong|hd_set_path_multistep_sde|schedule not set, c2 of row 0: schedule", "hd_set_path_multistep_sde", edits=[(0, 3, 0.1)])
    sched = table("hd_set_path", T)
    tau = (C.c_float * (T + 1))(*np.linspace(0.0, 1.0, T + 1))
    ok(lib.hd_set_schedule(h, T, tau, fp(sched)))

    # --- a schedule, no path
    every("null handle", PATHS + ROWS, handle=None)
    every("null t_idx", PATHS, null=("t",))
    every("null s_idx", PATHS, null=("s",))
    every("null rows", PATHS + ROWS, rows=False)
    every("K 0", PATHS + ROWS, k=0)
    every("path not set", ROWS)
    every("K > T", DOWN, k=T + 1, t=tuple(range(T + 1, 0, -1)), s=tuple(range(T, -1, -1)))
    refused("hd_set_path_up|K > T", "hd_set_path_up", k=T + 1, t=tuple(range(0, T + 1)), s=tuple(range(1, T + 2)))
    every("t_idx > T", DOWN, t=(9, 6, 4, 2))
    every("s_idx < 0", DOWN, s=(6, 4, 2, -1))
    every("s_idx == t_idx", DOWN, t=(8, 6, 4, 4), s=(6, 4, 4, 0))
    every("ascending transition", DOWN, t=(8, 6, 2, 4), s=(6, 2, 4, 0))
    every("transition 2 starts elsewhere", DOWN, t=(8, 6, 3, 2), s=(6, 4, 2, 0))
    refused("hd_set_path_multistep|c2 of row 0", "hd_set_path_multistep", edits=[(0, 2, 0.1)])
    refused("hd_set_path_multistep_sde|c2 of row 0", "hd_set_path_multistep_sde", edits=[(0, 3, 0.1)])
    refused("hd_set_path_up|rows with c", "hd_set_path_up", edits=[(2, 2, 0.5)])
    refused("hd_set_path_up|rows with a fourth column", "hd_set_path_up", edits=[(3, 3, 0.5)])
    refused("hd_set_path_up|from_idx < 0", "hd_set_path_up", t=(-1, 2, 4, 6))
    refused("hd_set_path_up|descending transition", "hd_set_path_up", t=(0, 4, 2, 6), s=(4, 2, 6, 8))
    refused("hd_set_path_up|to_idx == from_idx", "hd_set_path_up", t=(0, 2, 4, 4), s=(2, 4, 4, 8))
    refused("hd_set_path_up|transition 2 starts elsewhere", "hd_set_path_up", t=(0, 2, 5, 6), s=(2, 4, 6, 8))
    refused("hd_set_path_up|to_idx > T", "hd_set_path_up", s=(2, 4, 6, 9))
    every("two wrong|K > T, t_idx > T: K", DOWN, k=T + 1, t=tuple(range(T + 2, 1, -1)), s=tuple(range(T + 1, 0, -1)))
    every("two wrong|transition 1 starts elsewhere, s_idx < 0 in transition 3: start", DOWN, t=(8, 5, 4, 2), s=(6, 4, 2, -1))
    every("two wrong|transition 1 starts elsewhere and ascends: range", DOWN, t=(8, 5, 4, 2), s=(6, 7, 2, 0))
    every("two wrong|K 0, t_idx > T: argument", DOWN, k=0, t=(9, 6, 4, 2))
    refused("two wrong|hd_set_path|form 2, K > T: form", "hd_set_path", form=2, k=T + 1, t=tuple(range(T + 1, 0, -1)),
            s=tuple(range(T, -1, -1)))
    refused("two wrong|hd_set_path_multistep|c2 of row 0, s_idx < 0: range", "hd_set_path_multistep", edits=[(0, 2, 0.1)], s=(6, 4, 2, -1))
    refused("two wrong|hd_set_path_multistep_sde|c2 of row 0, transition 2 starts elsewhere: start", "hd_set_path_multistep_sde",
            edits=[(0, 3, 0.1)], t=(8, 6, 3, 2))
    refused("two wrong|hd_set_path_up|rows with c in row 2, descending transition 1: transition", "hd_set_path_up", edits=[(2, 2, 0.5)],
            t=(0, 4, 2, 6), s=(4, 2, 6, 8))
    refused("two wrong|hd_set_path_up|rows with c in row 1, descending transition 1: rows", "hd_set_path_up", edits=[(1, 2, 0.5)],
            t=(0, 4, 2, 6), s=(4, 2, 6, 8))
    refused("two wrong|hd_set_path_up|K > T, to_idx > T: K", "hd_set_path_up", k=T + 1, t=tuple(range(1, T + 2)), s=tuple(range(2, T + 3)))
    refused("two wrong|hd_set_path_up|to_idx > T, transition 2 starts elsewhere: start", "hd_set_path_up", t=(0, 2, 5, 6), s=(2, 4, 6, 9))
    refused("two wrong|hd_set_restraint|path not set, clip 0: path", "hd_set_restraint", edits=[(0, 3, 0.0)])
    refused("two wrong|hd_set_steer|path not set, beta < 0: path", "hd_set_steer", edits=[(0, 2, -1.0)])
    ok(lib.hd_set_path(h, K, i32((8, 6, 4, 2)), i32((6, 4, 2, 0)), fp(sched), 0, None))

    # --- a path: the rows
    every("K differs from the path's", ROWS, k=K - 1)
    for label, col, val in (("alpha_t 0", 0, 0.0), ("alpha_t nan", 0, NAN), ("sigma_t < 0", 1, -0.1), ("sigma_t nan", 1, NAN)):
        every(label, ROWS, edits=[(1, col, val)])
    for label, val in (("lambda inf", INF), ("lambda -inf", -INF), ("lambda nan", NAN)):
        refused(f"hd_set_restraint|{label}", "hd_set_restraint", edits=[(3, 2, val)])
    for label, val in (("clip 0", 0.0), ("clip < 0", -1.0), ("clip nan", NAN)):
        refused(f"hd_set_restraint|{label}", "hd_set_restraint", edits=[(2, 3, val)])
    for label, val in (("beta < 0", -0.5), ("beta inf", INF), ("beta nan", NAN)):
        refused(f"hd_set_steer|{label}", "hd_set_steer", edits=[(3, 2, val)])
    every("two wrong|K differs from the path's, alpha_t 0: K", ROWS, k=K - 1, edits=[(0, 0, 0.0)])
    every("two wrong|null rows, K differs from the path's: argument", ROWS, k=K - 1, rows=False)

    # --- hd_restrain_eps: the row
    good = ROW["hd_set_restraint"]
    eps_refused("two wrong|hd_restrain_eps|no restraints attached, alpha_t 0: restraints", [0.0] + good[1:])
    ok(lib.hd_restraint_attach(topo, None, 1, 0, None, None, 1, 0, None, None, 1, 0, scale.data_ptr(), 1, 1.0, None))
    for label, col, val in (("alpha_t 0", 0, 0.0), ("alpha_t nan", 0, NAN), ("sigma_t < 0", 1, -0.1), ("lambda inf", 2, INF),
                            ("lambda nan", 2, NAN), ("clip 0", 3, 0.0), ("clip < 0", 3, -1.0), ("clip nan", 3, NAN)):
        row = list(good)
        row[col] = val
        eps_refused(f"hd_restrain_eps|{label}", row)
    eps_refused("two wrong|hd_restrain_eps|clip 0, out is z: row", good[:3] + [0.0], out_buf="z")
    ok(lib.hd_restraint_detach(topo))

    # --- a schedule newer than the path
    ok(lib.hd_set_schedule(h, T, tau, fp(sched)))
    every("path older than the schedule", ROWS)

    torch.cuda.synchronize()
    ok(lib.hd_topology_destroy(topo))
    ok(lib.hd_destroy(h))
    return out


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
