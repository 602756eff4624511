"""Which library calls every Python sampling entry point makes, and with which scalars: the traces of
tests/golden/sampling_dispatch.json and the code that records them (tests/test_sampling_dispatch_cpu.py replays it).

    python -m tests.make_golden_dispatch          # rewrites the fixture from the code as it stands

No GPU: a stub library records every call and stops the entry point at the first loop entry point (hd_sample_loop,
hd_sample_loop_inpaint, hd_sample_path, hd_sample_path_inpaint, hd_sample_path_guided); the inputs are tensors that claim a CUDA
device, and the handle, the schedule upload, the topology and the stream are stubbed.  A trace is
    {"calls": [library calls in order, the loop entry point last], "args": {its scalars; pointers as "ptr" / "null"}}
    or {"error": "<exception type>"} (raised before any library call);
the fixture holds every distinct call sequence and argument set once and, per entry point, their indices for each row of `matrix()`.
B = 3, sizes [7, 4, 1], T = 6, hidden 32, 2 layers.  Every cache of uploaded tables is emptied before a row, so a row does not
depend on the rows before it.  The fixture records this project's own behaviour; nothing in it comes from the reference."""
import contextlib
import itertools
import json
import os
import sys

import torch

from tests import edit_reference as er

T, H, L, N_LIST = 6, 32, 2, [7, 4, 1]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_dispatch.json")

_LOOP = "h topo z ctx mol_shape {a} {b} rx rh rows seed base use_graph"
_INP = " fixed known R stream"
LOOPS = {
    "hd_sample_loop": (_LOOP.format(a="s_hi", b="s_lo") + " stream").split(),
    "hd_sample_loop_inpaint": (_LOOP.format(a="s_hi", b="s_lo") + _INP).split(),
    "hd_sample_path": (_LOOP.format(a="k_lo", b="k_hi") + " stream").split(),
    "hd_sample_path_inpaint": (_LOOP.format(a="k_lo", b="k_hi") + _INP).split(),
    "hd_sample_path_guided": "h topo z ctx ctx_u w w_rows phi k_lo k_hi rx rh rows seed base use_graph fixed known R stream".split(),
}
POINTERS = {"z", "ctx", "ctx_u", "w", "rx", "rh", "fixed", "known"}
CACHES = ("_path_cache", "_row_caches", "_inpaint_tabs")


class Reached(Exception):
    pass


class OnGpu(torch.Tensor):
    """A CPU tensor that claims to live on cuda:0 (the entry points look at `.device` before they touch the library)."""

    @property
    def device(self):
        return torch.device("cuda", 0)

    @property
    def is_cuda(self):
        return True


def _is_cuda(v):
    return isinstance(v, (str, torch.device)) and torch.device(v).type == "cuda"


@contextlib.contextmanager
def stubbed(seen):
    """The stubs, for the time of the block: `seen` collects (name, args) of every library call."""
    import hierdiff_amd
    from hierdiff_amd import _lib
    from hierdiff_amd.diffusion import DiffusionQM9
    from hierdiff_amd.dynamics import EGNN_dynamics_QM9
    from hierdiff_amd.noise_model import schedule_tables

    class Stub:
        def __getattr__(self, name):
            def f(*a):
                seen.append((name, a))
                if name in LOOPS:
                    raise Reached(name)
                return 0
            return f

    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    orig_to = torch.Tensor.to

    def to(self, *a, **kw):
        if not (any(_is_cuda(v) for v in a) or _is_cuda(kw.get("device"))):
            return orig_to(self, *a, **kw)
        a = [v for v in a if not _is_cuda(v)]
        kw = {k: v for k, v in kw.items() if k != "device"}
        return (orig_to(self, *a, **kw) if a or kw else self).as_subclass(OnGpu)

    def factory(fn):
        def f(*a, **kw):
            dev = kw.pop("device", None)
            out = fn(*a, **kw)
            return out.as_subclass(OnGpu) if _is_cuda(dev) else out
        return f

    tabs = {}

    def schedule(self, rows=1):
        if id(self) not in tabs:
            tabs[id(self)] = schedule_tables(self.gamma, self.T, None, "fp64", 1)
        return tabs[id(self)]

    try:
        patch(_lib, "load", lambda: Stub())
        patch(DiffusionQM9, "_lib_handle", lambda self, synced=False: 1)
        patch(DiffusionQM9, "_schedule", schedule)
        patch(EGNN_dynamics_QM9, "topology", lambda self, *a: type("Topo", (), {"ptr": 1})())
        for name, mod in list(sys.modules.items()):
            if name.startswith(hierdiff_amd.__name__ + ".") and hasattr(mod, "_stream"):
                patch(mod, "_stream", lambda dev: 0)
        patch(torch.Tensor, "to", to)
        for name in ("empty", "zeros", "ones", "full", "eye", "tensor", "as_tensor", "arange", "randn"):
            patch(torch, name, factory(getattr(torch, name)))
        yield
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


# ----------------------------------------------------------------------------- the matrix
OPTIONS = {                      # name -> the values after "not given"
    "steps": [5], "eta": [0.0], "solver": ["dpm2m"], "guidance": [2.5], "keep": ["z", "x0"], "restraints": [True], "injected": [True],
    "fix_noise": [True], "k_lo": [True], "record": ["z", "x0"], "debug_checks": [True],
}
ACCEPTS = {
    "sample_from_masks": "steps eta solver guidance keep restraints injected fix_noise",
    "path_steps": "steps eta solver guidance restraints fix_noise k_lo",
    "latent_steps": "steps eta solver guidance restraints injected fix_noise k_lo",
    "sample_from_latent": "steps eta solver guidance keep restraints injected fix_noise",
    "inpaint_steps": "k_lo",
    "sample_inpaint": "steps eta solver guidance keep restraints debug_checks",
    "sample": "steps eta solver guidance keep restraints",
    "sample_grow": "steps eta solver guidance keep restraints",
    "vary": "steps eta solver guidance keep restraints",
    "edm_sample": "steps eta solver guidance fix_noise",
    "edm_sample_chain": "steps eta solver guidance keep",
    "edm_sample_chain_all": "steps eta solver guidance record",          # keep_frames=None: every transition is kept
}


def matrix():
    """[(row key, entry point, options)]: every entry point crossed with every combination of the options it accepts."""
    rows = []
    for entry, names in ACCEPTS.items():
        names = names.split()
        for combo in itertools.product(*[[None] + OPTIONS[n] for n in names]):
            opt = {n: v for n, v in zip(names, combo) if v is not None}
            rows.append((entry + "|" + ",".join(f"{k}={v}" for k, v in opt.items()), entry, opt))
    return rows


class Case:
    """The models and inputs every row shares.  `device`: None for tensors that only claim to be on a GPU (the traces), or a real
    device (scratch/sampling_bits.py runs the same rows to completion)."""

    def __init__(self, T=T, device=None):
        from hierdiff_amd import EnVariationalDiffusion
        from hierdiff_amd.diffusion import default_config
        from hierdiff_amd.restraints import Restraints
        sd_np, _ = er.weights(H, L, C_=1)
        self.model = er.cpu_diffusion(sd_np, H, L, T, C_=1)
        self.edm = EnVariationalDiffusion(default_config(hidden_nf=H, n_layers=L, context_node_nf=1, timesteps=T))
        self.edm.load_state_dict(self.model.state_dict())
        for m in (self.model, self.edm):
            m.nodes_dist.sample = lambda n: list(N_LIST)             # (`sample` draws the sizes)
        x, h, nm, _, ctx = er.molecules(N_LIST, C_=1)
        self.B, self.N = int(nm.shape[0]), int(nm.shape[1])
        self.T, self.device = T, "cuda:0" if device is None else device
        gpu = (lambda t: t.as_subclass(OnGpu)) if device is None else (lambda t: t.to(device))
        if device is not None:
            self.model, self.edm = self.model.to(device), self.edm.to(device)
        self.nm, self.ctx, self.x, self.h = gpu(nm), gpu(ctx), gpu(x), gpu(h)
        self.z = gpu(torch.cat([x, h], dim=2))
        ks = [2, 1, 0]
        self.fm = gpu((torch.arange(self.N)[None, :] < torch.tensor(ks)[:, None]).unsqueeze(-1))
        self.known = [{"x": x[i, :k].clone(), "h": h[i, :k].clone()} for i, k in enumerate(ks)]
        self.samples = [{"x": x[i, :n].clone(), "h": h[i, :n].clone(), "context": ctx[i, :n].clone()} for i, n in enumerate(N_LIST)]
        self.rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 1.0, 1.0]], pairs=[[0, 1, 0.5, 1.5, 1.0]], anchors=[[0, 0.0, 0.0, 0.0, 0.5, 1.0]])

    def keywords(self, opt):
        kw = {}
        if "steps" in opt:
            kw["steps"] = opt["steps"]
        if "eta" in opt:
            kw["eta"] = opt["eta"]
        if "solver" in opt:
            kw["solver"] = opt["solver"]
        if "guidance" in opt:
            kw["guidance_scale"] = opt["guidance"]
        if "keep" in opt:
            kw.update(keep_frames=3, record=opt["keep"])
        if "record" in opt:
            kw["record"] = opt["record"]
        if "restraints" in opt:
            kw.update(restraints=self.rs, restraint_scale=0.5)
        return kw

    def call(self, entry, opt):
        m, kw = self.model, self.keywords(opt)
        T = self.T
        K = opt.get("steps", T)
        nb = 1 if opt.get("fix_noise") else self.B
        k_lo = 2 if opt.get("k_lo") else 0
        if "fix_noise" in opt:
            kw["fix_noise"] = True
        raws = lambda n: er.raw_draws(n, self.B, self.N, 3, rows=nb)
        if entry == "sample_from_masks":
            if "injected" in opt:
                kw["raw_noises"] = raws(K + 2)
            return m.sample_from_masks(self.nm, None, self.ctx, **kw)
        if entry == "path_steps":
            return m.path_steps(self.z, self.nm, None, self.ctx, k_lo=k_lo, **kw)
        if entry == "latent_steps":
            if "injected" in opt:
                kw["raw_noises"] = raws(K - k_lo)
            return m.latent_steps(self.z, self.nm, None, self.ctx, k_lo=k_lo, **kw)
        if entry == "sample_from_latent":
            if "injected" in opt:
                kw["raw_noises"] = raws(K + 1)
            return m.sample_from_latent(self.z, self.nm, None, self.ctx, **kw)
        if entry == "inpaint_steps":
            s_hi, s_lo = (4, 1) if k_lo else (T, 0)
            return m.inpaint_steps(self.z, s_hi, s_lo, self.nm, self.fm, self.x, self.h, self.ctx, 2)
        if entry == "sample_inpaint":
            kw.pop("restraint_scale", None)
            m.debug_checks = "debug_checks" in opt       # the loop in single steps, the invariant checked after each
            try:
                return m.sample_inpaint(self.nm, self.fm, self.x, self.h, self.ctx, 2, **kw)
            finally:
                m.debug_checks = False
        if entry == "sample":
            return m.sample(self.B, self.device, context=0.5, **kw)
        if entry == "sample_grow":
            kw.pop("restraint_scale", None)
            return m.sample_grow(self.known, N_LIST, self.device, context=0.5, resamplings=2, **kw)
        if entry == "vary":
            return m.vary(self.samples, self.device, 4 if "steps" not in opt else T, **kw)
        if entry == "edm_sample":
            return self.edm.sample(self.B, self.N, self.nm, None, self.ctx, **kw)
        if entry == "edm_sample_chain":
            keep = kw.pop("keep_frames", None)
            return self.edm.sample_chain(self.B, self.N, self.nm, None, self.ctx, keep, **kw)
        if entry == "edm_sample_chain_all":
            return self.edm.sample_chain(self.B, self.N, self.nm, None, self.ctx, None, **kw)
        raise KeyError(entry)


def trace(case, entry, opt):
    """One row of the fixture."""
    seen = []
    for m in (case.model, case.edm):
        for name in CACHES:
            m.__dict__.pop(name, None)
    with stubbed(seen):
        try:
            case.call(entry, opt)
        except Reached as r:
            name, a = seen[[n for n, _ in seen].index(str(r))]
            args = {}
            for key, v in zip(LOOPS[name], a):
                if key in POINTERS:
                    args[key] = "null" if not v else "ptr"
                elif key not in ("h", "topo", "stream"):
                    args[key] = v
            calls = [n for n, _ in seen]
            return {"calls": calls[:calls.index(name) + 1], "args": args}
        except (ValueError, NotImplementedError) as e:
            assert not seen, f"{entry} {opt}: {type(e).__name__} after the library calls {[n for n, _ in seen]}"
            return {"error": type(e).__name__}
    raise AssertionError(f"{entry} {opt}: returned without reaching a loop entry point")


def _index(table, value):
    if value not in table:
        table.append(value)
    return table.index(value)


def traces():
    """The fixture: the matrix it covers, every distinct call sequence and every distinct set of loop arguments once (in order of first
    appearance), and per entry point one [calls index, args index] - or the error's type - for each of its rows in `matrix()` order."""
    case = Case()
    calls, args, rows = [], [], {entry: [] for entry in ACCEPTS}
    for _, entry, opt in matrix():
        row = trace(case, entry, opt)
        rows[entry].append(row["error"] if "error" in row else [_index(calls, row["calls"]), _index(args, row["args"])])
    return {"matrix": {"accepts": ACCEPTS, "options": OPTIONS}, "calls": calls, "args": args, "rows": rows}


def expected(fixture, entry, i):
    """Row i of `entry` as `trace` returns it."""
    row = fixture["rows"][entry][i]
    return {"error": row} if isinstance(row, str) else {"calls": fixture["calls"][row[0]], "args": fixture["args"][row[1]]}


def main():
    fx = traces()
    line = lambda v: json.dumps(v, separators=(",", ":"))
    block = lambda k: f'"{k}": [\n' + ",\n".join(line(t) for t in fx[k]) + "]"
    with open(FIXTURE, "w") as fh:
        fh.write('{"matrix": ' + line(fx["matrix"]) + ",\n" + block("calls") + ",\n" + block("args") + ',\n"rows": {\n'
                 + ",\n".join(f"{json.dumps(e)}: {line(v)}" for e, v in fx["rows"].items()) + "}}\n")
    print(f"{sum(len(v) for v in fx['rows'].values())} rows, {len(fx['calls'])} call sequences, {len(fx['args'])} argument sets -> {FIXTURE}")


if __name__ == "__main__":
    main()
