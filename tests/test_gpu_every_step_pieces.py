"""GPU tier (-m gpu) of the every-step entry points of the C ABI cut into pieces: hd_sample_loop and hd_sample_loop_inpaint with
s_hi < T.  Both run the path loop on the handle's built-in every-step tables (step s is position T - 1 - s), so a piece (s_hi, s_lo) is
the transitions T - s_hi ... T - s_lo - 1; Python only ever asks hd_sample_loop for the whole chain (T, 0).

Bit equality only (`torch.equal`): draws are keyed by the step, so the pieces give the bits of the whole; injected normals are
indexed from the first step of the call, so each piece is handed the pointers of its own first step; graph replay gives the bits of
plain launches; a sink attached to the topology is not written.  Shapes: T = 6, H = 32, L = 1, n_list = [5, 3, 5] (B = 3, N = 5, one
molecule shorter than N)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests.test_gpu_fewstep import DEV, dev, make_model, raw_draws
from tests.test_gpu_inpaint import make_case
from tests.test_gpu_parity import PRECISIONS

pytestmark = pytest.mark.gpu

T, H, L = 6, 32, 1
N_LIST = [5, 3, 5]
PIECES = [(6, 4), (4, 1), (1, 0)]
SEED, BASE = 2022, 13


def ptr(t):
    return None if t is None else t.data_ptr()


def start_state(nm, seed=1):
    rx, rh = raw_draws(1, nm.shape[0], nm.shape[1], seed=seed)[0]
    return dev(orc.combined_noise(rx, rh, nm.float()))


def plain_setup(precision):
    from hierdiff_amd import _lib
    model, _, _ = make_model(H, L, T, precision=precision)
    nm, _ = orc.canonical_masks(N_LIST)
    nm = nm.bool()
    B, N = nm.shape[:2]
    model._schedule(rows=B)
    topo = model.dynamics.topology(dev(nm), None, B, N)
    lib = _lib.load()

    def run(z, s_hi, s_lo, graph, rows=B, rx=None, rh=None):
        z = z.clone()
        h = model._lib_handle()                  # through the model, which owns the handle: the closure keeps both alive
        rc = lib.hd_sample_loop(h, topo.ptr, z.data_ptr(), None, -1, s_hi, s_lo, ptr(rx), ptr(rh), rows, SEED, BASE, int(graph), None)
        assert rc == 0, lib.hd_last_error()
        return z

    return model, lib, topo, nm, run


def in_pieces(run, z, **kw):
    """[z behind every piece of PIECES], each piece continuing the one before."""
    out = []
    for s_hi, s_lo in PIECES:
        z = run(z, s_hi, s_lo, **kw)
        out.append(z)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [0, 1])
def test_sample_loop_in_pieces_is_the_whole_chain(graph, precision):
    _, _, _, nm, run = plain_setup(precision)
    B, N = nm.shape[:2]
    zT = start_state(nm)
    # counter-based noise, one row of it per molecule and one shared row
    for rows in (B, 1):
        whole = run(zT, T, 0, graph, rows=rows)
        assert torch.isfinite(whole).all() and not torch.equal(whole, zT)
        assert torch.equal(in_pieces(run, zT, graph=graph, rows=rows)[-1], whole), rows
        assert torch.equal(whole, run(zT, T, 0, 0, rows=rows)), rows
    # injected normals [T, rows, N, 3 | F] in step order: a piece reads from the pointers of its own first step, T - s_hi
    for rows in (B, 1):
        raws = raw_draws(T, B, N, seed=8, rows=rows)
        rx, rh = dev(torch.stack([r[0] for r in raws]).contiguous()), dev(torch.stack([r[1] for r in raws]).contiguous())
        whole = run(zT, T, 0, graph, rows=rows, rx=rx, rh=rh)
        assert not torch.equal(whole, run(zT, T, 0, graph, rows=rows))
        z = zT
        for s_hi, s_lo in PIECES:
            z = run(z, s_hi, s_lo, graph, rows=rows, rx=rx[T - s_hi:], rh=rh[T - s_hi:])
        assert torch.equal(z, whole), rows
        assert torch.equal(whole, run(zT, T, 0, 0, rows=rows, rx=rx, rh=rh)), rows
        if graph:
            # two pieces that start at different s_hi read the SAME pointers from their own first step on: the cached graph of the
            # first must not serve the second (its key holds the start)
            for s_hi, s_lo in PIECES[:2]:
                got, ref = (run(zT, s_hi, s_lo, g, rows=rows, rx=rx, rh=rh) for g in (1, 0))
                assert torch.equal(got, ref), (rows, s_hi)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [0, 1])
def test_sample_loop_inpaint_in_pieces_is_the_whole_chain(graph, precision):
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _ = make_model(H, L, T, precision=precision)
    nm, _, fm, xk, hk, _ = make_case(n_list=N_LIST, n_fixed=[2, 0, 3])
    B = nm.shape[0]
    st = model._inpaint_setup(dev(nm), dev(fm), dev(xk), dev(hk), None, 2, None)       # schedule and inpainting schedule are set

    def run(z, s_hi, s_lo, graph):
        z = z.clone()
        rc = lib.hd_sample_loop_inpaint(st.h, st.topo.ptr, z.data_ptr(), None, -1, s_hi, s_lo, None, None, B, SEED, BASE, int(graph),
                                        st.fm_u8.data_ptr(), st.xh_known.data_ptr(), 2, None)
        assert rc == 0, lib.hd_last_error()
        return z

    zT = start_state(nm)
    whole = run(zT, T, 0, graph)
    assert torch.isfinite(whole).all() and not torch.equal(whole, zT)
    cuts = in_pieces(run, zT, graph=graph)
    assert torch.equal(cuts[-1], whole)
    for got, ref in zip(cuts + [whole], in_pieces(run, zT, graph=0) + [run(zT, T, 0, 0)]):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [0, 1])
def test_sample_loop_ignores_an_attached_sink(graph, precision):
    from hierdiff_amd import paths
    model, lib, topo, nm, run = plain_setup(precision)
    h = model._lib_handle()
    B, N = nm.shape[:2]
    zT = start_state(nm)
    bare = run(zT, T, 0, graph)
    model._path_tables(h, model._schedule(rows=B), paths.build_path(T), 1.0)            # hd_set_path: the identity path
    frame_of = np.arange(T, dtype=np.int32)
    assert lib.hd_set_chain(h, T, frame_of.ctypes.data_as(C.POINTER(C.c_int)), None, T) == 0, lib.hd_last_error()
    sink = torch.full((T, B, N, zT.shape[2]), -7.25, device=DEV)
    assert lib.hd_chain_attach(topo.ptr, sink.data_ptr(), T, 0, 1.0, 1.0, 0.0) == 0, lib.hd_last_error()
    try:
        with_sink = run(zT, T, 0, graph)
    finally:
        assert lib.hd_chain_detach(topo.ptr) == 0
    assert torch.equal(sink.view(torch.int32), torch.full_like(sink, -7.25).view(torch.int32))
    assert torch.equal(with_sink, bare)
    assert torch.equal(run(zT, T, 0, graph), bare)
