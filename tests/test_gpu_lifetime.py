"""GPU tier (-m gpu): after everything is destroyed, the library holds nothing.

hd_live_allocations counts the device allocations the library holds in this process (pooled arenas included) and their bytes.  Every
test trims the arena pool, reads (count, bytes) as its base, builds and uses its objects - the count is above the base while they
live - destroys them, trims again and finds exactly the base; the whole cycle runs three times, so a recycled arena and a second
first use are both seen.  Between them the tests make every lazily allocated buffer of a handle and a topology exist before the
destroy.  Nothing is made to fail.

The sampling shapes are those of tests/make_golden_loop_refusals.py, driven at the C ABI like there: hidden 32, two layers, one context
column, T = 8, synthetic weights; B = 3 with sizes [7, 4, 1], and B = 4 as two groups of 2 (N = 5, four valid nodes in every row) where
a term needs groups.  All tensors are zeros of the right size: what a call computes is not looked at here."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from tests.make_golden_loop_refusals import ARGS, CTX, F, H, L, SEED, BASE, T, D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 4
CYCLES = 3


def f32(*v):
    return (C.c_float * len(v))(*v)


def i32(*v):
    return (C.c_int * len(v))(*v)


def rows_of(row, k):
    a = np.tile(np.asarray(row, dtype=np.float32), (k, 1))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def live(lib):
    b = C.c_longlong(-1)
    n = int(lib.hd_live_allocations(C.byref(b)))
    return n, int(b.value)


def settle(lib):
    """Everything a finished test or cycle still references goes; the pool is emptied."""
    gc.collect()
    torch.cuda.synchronize()
    _lib.check(lib.hd_arena_pool_trim(), "hd_arena_pool_trim")
    return live(lib)


class Loops:
    """One handle with weights, schedule, inpainting rows and a K-transition path; topologies and calls on it."""

    def __init__(self, lib):
        self.lib, self.seen = lib, []
        cfg = _lib.HdConfig(in_node_nf=F + 1, context_node_nf=CTX, n_dims=3, hidden_nf=H, n_layers=L, inv_sublayers=2, attention=1,
                            tanh=1, condition_time=1, norm_constant=0.0, normalization_factor=10.0, coords_range=30.0, precision=0,
                            aggregation_mean=0)
        self.h = C.c_void_p()
        self.ok(lib.hd_create(C.byref(cfg), 0, C.byref(self.h)))
        n = lib.hd_weight_count(self.h)
        blob = (np.random.default_rng(0).standard_normal(n) * 0.05).astype(np.float32)
        for _ in range(2):                                   # the second call finds the packed weights in place
            self.ok(lib.hd_set_weights(self.h, blob.ctypes.data, n, 0, None))
        self.rows, self.rows_p = rows_of([0.9, 0.3, 0.5, 0.2], T)
        self.ok(lib.hd_set_schedule(self.h, T, f32(*np.linspace(0.0, 1.0, T + 1)), self.rows_p))
        self.ok(lib.hd_set_inpaint_schedule(self.h, T, self.rows_p))
        self.path(K)
        self.note("handle")

    def ok(self, rc):
        assert rc == 0, self.lib.hd_last_error().decode()

    def note(self, what):
        self.seen.append((what,) + live(self.lib))
        print(f"  {what:40s} count {self.seen[-1][1]:3d}  bytes {self.seen[-1][2]}")

    def path(self, k):
        """An ancestral path of k transitions with inpainting rows (k = 4: 8 -> 6 -> 4 -> 2 -> 0; k = 2: 8 -> 4 -> 0)."""
        step = T // k
        self.K = k
        self.t_idx, self.s_idx = i32(*range(T, 0, -step)), i32(*range(T - step, -1, -step))
        self.ok(self.lib.hd_set_path(self.h, k, self.t_idx, self.s_idx, self.rows_p, 0, self.rows_p))

    def topology(self, sizes, n):
        nm = np.zeros((len(sizes), n), dtype=np.uint8)
        for b, s in enumerate(sizes):
            nm[b, :s] = 1
        topo = C.c_void_p()
        self.ok(self.lib.hd_topology_create(self.h, nm.ctypes.data, None, len(sizes), n, C.byref(topo)))
        return topo

    def buffers(self, B, N):
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
        self.B, self.N = B, N
        self.buf = dict(z=z(B, N, D), xh=z(B, N, D), ctx=z(B, N, CTX), ctx_u=z(B, N, CTX), w=z(B), fixed=z(B, N, dtype=torch.uint8),
                        known=z(B, N, D), parts=z(B, N, F, dtype=torch.uint8), acc=z(B, dtype=torch.float64), err=z(T, B),
                        sink=z(2, B, N, D))
        self.buf["fixed"][:, 0] = 1                          # the first node of every molecule is known
        self.ptr = {k: v.data_ptr() for k, v in self.buf.items()}

    def call(self, entry, topo, **kw):
        p = self.ptr
        a = dict(z=p["z"], xh=p["xh"], ctx=p["ctx"], ctx_u=p["ctx_u"], w=p["w"], w_rows=self.B, phi=0.5, mol_shape=-1, lo=0, hi=self.K,
                 rx=None, rh=None, rows=self.B, seed=SEED, base=BASE, use_graph=1, fixed=None, known=None, R=0, acc=p["acc"],
                 err=p["err"], stream=None)
        a.update(kw)
        a["s_hi"], a["s_lo"] = T - a["lo"], T - a["hi"]
        self.ok(getattr(self.lib, entry)(self.h, topo, *[a[k] for k in ARGS[entry].split()]))

    def destroy(self, *topos):
        torch.cuda.synchronize()
        for t in topos:
            self.ok(self.lib.hd_topology_destroy(t))
        self.ok(self.lib.hd_destroy(self.h))


def sampling_cycle(lib):
    """Plain, every-step, inpainting with channel masks, guided, multistep, recording and scoring calls on one topology of B = 3."""
    lp = Loops(lib)
    topo = lp.topology([7, 4, 1], 7)
    lp.buffers(3, 7)
    p, h = lp.ptr, lp.h
    lp.note("topology")
    lp.call("hd_sample_path", topo)
    lp.note("graph-replayed path call")
    lp.call("hd_sample_loop", topo, hi=T)
    lp.note("every-step loop")
    ip = dict(fixed=p["fixed"], known=p["known"])
    lp.ok(lib.hd_inpaint_parts(h, topo, p["parts"], None))
    lp.call("hd_sample_loop_inpaint", topo, hi=T, R=1, **ip)
    lp.note("every-step inpainting, channel masks")
    lp.call("hd_sample_loop_inpaint", topo, hi=T, R=2, **ip)
    lp.note("... resamplings 1 -> 2")
    lp.call("hd_sample_path_inpaint", topo, R=2, **ip)
    lp.ok(lib.hd_inpaint_parts(h, topo, None, None))
    lp.note("path inpainting")
    lp.call("hd_sample_path_guided", topo)
    lp.note("guided call")
    rows5, rows5_p = rows_of([0.9, 0.3, 0.1, 0.5, 0.5], K)
    rows5[0, 2] = 0.0
    lp.ok(lib.hd_set_path_multistep(h, K, lp.t_idx, lp.s_idx, rows5_p))
    lp.call("hd_sample_path", topo)
    lp.note("dpm2m call")
    lp.path(K)
    as_rows, as_p = rows_of([0.9, 0.3], K)                   # (as_rows keeps the memory as_p points at)
    for what, alsig in ((0, None), (1, as_p)):               # the state, then the data prediction (which needs alpha / sigma rows)
        lp.ok(lib.hd_set_chain(h, K, i32(0, -1, 1, -1), alsig, 2))
        lp.ok(lib.hd_chain_attach(topo, p["sink"], 2, what, 1.0, 1.0, 0.0))
        lp.call("hd_sample_path", topo)
    lp.ok(lib.hd_chain_detach(topo))
    lp.note("recording calls")
    lp.ok(lib.hd_set_nll_terms(h, 4, i32(1, 3, 5, 8), lp.rows_p))
    lp.call("hd_nll_terms", topo, hi=4)
    lp.note("scoring, 4 terms with their errors")
    lp.ok(lib.hd_set_nll_terms(h, 6, i32(1, 2, 3, 5, 7, 8), lp.rows_p))
    lp.call("hd_nll_terms", topo, hi=6)
    lp.note("scoring, 6 terms")
    return lp, (topo,)


def terms_cycle(lib):
    """Restraints with fields, templates and features on B = 3; steering and diversity on B = 4 as two groups of 2; then a path of
    another K on the same handle, which re-allocates the path tables and the row tables."""
    lp = Loops(lib)
    h = lp.h
    t3, t4 = lp.topology([7, 4, 1], 7), lp.topology([4, 4, 4, 4], 5)
    lp.note("two topologies")
    rows3, rows3_p = rows_of([0.9, 0.3, 1.0], K)
    one = f32(1.0)

    def restraints(topo, n):
        """One obstacle, no pairs, one anchor on node 0 (valid in every molecule); one 2 x 2 x 2 field; one translation-fitted
        template on node 0; a band on node 0 and one sum over the features."""
        lp.ok(lib.hd_restraint_attach(topo, f32(0.5, 0.0, 0.0, 1.5, 2.0), 1, 1, None, None, 1, 0, i32(0), f32(1.0, 1.0, 1.0, 0.25, 1.5), 1, 1,
                                      one, 1, 1.0, None))
        lp.ok(lib.hd_restraint_fields(topo, 1, f32(*([0.5] * 8)), (C.c_longlong * 2)(0, 8), i32(2, 2, 2),
                                      f32(-1.0, -1.0, -1.0, 2.0, 2.0, 2.0, 1.0, 0.5), f32(*([1.0] * n)), 1, None))
        lp.ok(lib.hd_restraint_templates(topo, 1, 1, 1, i32(0), f32(0.0, 0.0, 0.0, 1.0), f32(1.0, 1.0), None))
        band = lambda v: f32(*([v] * F))
        lp.ok(lib.hd_restraint_features(topo, band(-1.0), band(1.0), band(1.0), 1, 1, band(1.0), f32(-1.0, 1.0, 1.0, 0.0), 1, 1,
                                        1.0, 0.0, 1.0, None))

    lp.buffers(3, 7)
    restraints(t3, 7)
    lp.ok(lib.hd_set_restraint(h, K, lp.rows_p))
    lp.call("hd_sample_path", t3)
    lp.ok(lib.hd_restraint_detach(t3))
    lp.note("restraints: fields, templates, features")

    lp.buffers(4, 5)
    restraints(t4, 5)
    lp.ok(lib.hd_set_steer(h, K, rows3_p))
    lp.ok(lib.hd_steer_attach(t4, 2, 0.5, 1, None))
    lp.call("hd_sample_path", t4)
    lp.ok(lib.hd_steer_detach(t4))
    lp.ok(lib.hd_restraint_detach(t4))
    lp.note("steering, two groups of 2")
    lp.ok(lib.hd_set_diversity(h, K, lp.rows_p))
    lp.ok(lib.hd_diversity_attach(t4, 2, 1.0, 1.0, one, 1, 1.0, None))
    lp.call("hd_sample_path", t4)
    lp.note("diversity, two groups of 2")

    lp.path(2)                                               # another K: the path tables and all three row tables move
    restraints(t4, 5)
    lp.ok(lib.hd_set_restraint(h, 2, lp.rows_p))
    lp.ok(lib.hd_set_diversity(h, 2, lp.rows_p))
    lp.call("hd_sample_path", t4)
    lp.ok(lib.hd_diversity_detach(t4))
    lp.ok(lib.hd_set_steer(h, 2, rows3_p))
    lp.ok(lib.hd_steer_attach(t4, 2, 0.5, 1, None))
    lp.call("hd_sample_path", t4)
    lp.note("a path of 2 transitions, all terms again")
    return lp, (t3, t4)


@pytest.mark.parametrize("cycle", [sampling_cycle, terms_cycle], ids=lambda f: f.__name__)
def test_handle_and_topologies_give_everything_back(cycle):
    _lib.require_gpu()
    lib = _lib.load()
    base = settle(lib)
    for c in range(CYCLES):
        print(f"cycle {c}: base count {base[0]}, bytes {base[1]}")
        lp, topos = cycle(lib)
        counts = [n for _, n, _ in lp.seen]
        assert min(counts) > base[0], lp.seen
        assert max(counts) >= counts[0] + 10, f"the lazily allocated buffers did not appear: {lp.seen}"
        at = {what: n for what, n, _ in lp.seen}
        if "graph-replayed path call" in at:                 # calls that do not inpaint, guide or record allocate nothing
            assert at["graph-replayed path call"] == at["every-step loop"] == at["topology"], lp.seen
        lp.destroy(*topos)
        assert settle(lib) == base, f"cycle {c}: left behind {lp.seen[-1]} -> {live(lib)}, base {base}"


@pytest.mark.autograd
def test_stage2_layer_gives_everything_back():
    """hd_egcl_create, a graph, the inference forward, hd_egcl_forward_train + hd_egcl_backward (the backward workspace), destroy."""
    from tests.test_gpu_stage2_training import _hip_layer, _layer_case, _run_hip, _upstream
    lib = _lib.load()
    Hh, kw, _, sd_np, inp = _layer_case("f15_egcl_full_h64")
    g = lambda t: None if t is None else t.to(DEV)
    base = settle(lib)
    for c in range(CYCLES):
        m = _hip_layer(Hh, kw, sd_np)
        with torch.no_grad():
            outs = m(g(inp["h"]), [g(inp["row"]), g(inp["col"])], g(inp["x"]), edge_attr=g(inp["ea"]), node_mask=g(inp["nm"]),
                     edge_mask=g(inp["em"]))
        torch.cuda.synchronize()
        fwd = live(lib)
        _run_hip(m, inp, _upstream(outs, 3))
        torch.cuda.synchronize()
        bwd = live(lib)
        print(f"cycle {c}: base {base}, after the forward {fwd}, after the backward {bwd}")
        assert fwd[0] > base[0] and bwd[0] > fwd[0] and bwd[1] > fwd[1]              # the backward adds its workspace
        del m, outs
        assert settle(lib) == base, f"cycle {c}"


def _permuted():
    import itertools
    orders = list(itertools.permutations([3, 4, 5, 6, 7, 8]))[::60]
    assert len(set(orders)) == 12
    return [dict(sizes=o) for o in orders]


@pytest.mark.autograd
@pytest.mark.parametrize("masks", ["permuted", "ragged"])
def test_training_topology_churn_stays_bounded_and_gives_everything_back(masks):
    """12 differentiable forwards (dynamics_forward_train) at H = 64 on never-repeated masks go through the 8-entry topology caches
    and the arena pool: with the handle and its weights in place, the count stays within the pool's bound of 12 arenas; after
    clearing the caches and release_cached_memory() it is back at the base.

    `ragged`: the batches of test_pipelined_fit_epoch_equals_step_by_step (E = 92 .. 290 edges), the case where a batch outgrows the
    10 % head room of every pooled arena's pinned twin and gets a new slot by design.  With them the count read 943, 944, ... 951,
    952, 952, 952 (942 with the handle): one new arena per forward up to the tenth, whose batch is the largest of the 12.  So "the
    last four readings are equal" cannot hold for them under the pool's size policy, and is asserted for `permuted` alone.

    `permuted`: 12 different orders of the sizes 3 .. 8 (B = 6, N = 9), as scratch/fresh_masks_time.py permutes one set of sizes.
    Every batch then needs the same bytes (hd_topology_layout gives the same M, E, tiles, parts and padded edge rows for all 12), so a
    count that keeps growing can only be a leak.  Expected: one arena per forward while the caches fill (8), one more at the ninth
    (the caches let go of the oldest topology after the new one exists), none from the tenth on."""
    from hierdiff_amd.dynamics import release_cached_memory
    from tests.test_gpu_training import _host_batch, _small_model
    lib = _lib.load()
    POOL_SLOTS = 12
    batches = _permuted() if masks == "permuted" else [{}] * 12
    base = settle(lib)
    for c in range(CYCLES):
        model = _small_model()                               # H = 64, two layers, training mode
        dyn = model.dynamics
        dyn._handle()
        dyn.sync_weights()
        held = live(lib)
        assert held[0] > base[0]
        counts = []
        for k, kw in enumerate(batches):
            loss = model.training_step({key: v.to(DEV) for key, v in _host_batch(100 + k, **kw).items()})
            assert loss.requires_grad                        # the training path
            loss.backward()
            torch.cuda.synchronize()
            del loss
            counts.append(live(lib)[0])
        print(f"{masks}, cycle {c}: base {base}, with the handle {held}, after each forward {counts}")
        assert counts[-1] <= held[0] + POOL_SLOTS and max(counts) <= held[0] + POOL_SLOTS, counts
        if masks == "permuted":
            assert len(set(counts[-4:])) == 1, f"still growing: {counts}"
        dyn._topo_cache.clear(); dyn._topo_by_content.clear()
        del dyn, model
        gc.collect()
        release_cached_memory()
        assert settle(lib) == base, f"{masks}, cycle {c}"
