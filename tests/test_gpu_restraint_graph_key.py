"""GPU tier (-m gpu): when the cached path graph of a restrained call is rebuilt.  One sequence of calls on one topology - re-attached
tables, fields and templates coming and going, another M, the known fragments' frame, a plain call in between - with
hd_path_graph_builds read after every step, and a replayed call compared bit for bit with the freshly built one in three places.

The expected counts are not derived from the code under test: they were printed by this test on commit 775496d (the parent of the
change that gathered the restraint state of a topology into one struct) and are kept as literals.  Model: the `small_model` of the
restraint tests (H = 32, one layer, T = 20), B = 2, N = 5, a 3-transition path, P = Q = A = 1, one 2x2x2 field, one 3-row template."""
import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from hierdiff_amd.restraints import Field, Restraints, Template
from tests.test_restraint_cpu import small_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, N = 2, 5

# hd_path_graph_builds after every step, less its value before the first (commit 775496d)
BUILDS = [1, 1, 1, 2, 2, 3, 4, 4, 5, 6, 7, 8, 9]


def tables(shift=0.0, fields=None, templates=None):
    return Restraints(obstacles=[[0.5 + shift, 0.0, 0.0, 1.5, 2.0]], pairs=[[0, 1, 2.0 + shift, 2.5, 1.0]],
                      anchors=[[2, 1.0, 1.0 + shift, 1.0, 0.25, 1.5]], fields=fields, templates=templates)


def test_when_the_path_graph_is_rebuilt():
    lib = _lib.load()
    torch.manual_seed(7)
    model = small_model().to(DEV)
    model.seed, model.use_graph = 11, True
    model.eval()
    g = np.random.Generator(np.random.PCG64(3))
    field = [Field(g.normal(0.0, 2.0, (2, 2, 2)), [-4.0, -4.0, -4.0], 8.0, k=1.0)]
    tpl = lambda M: [Template(np.arange(M), g.normal(0.0, 1.5, (M, 3)), k=1.5)]
    tpl3, tpl4 = tpl(3), tpl(4)
    nm = torch.ones(B, N, 1, dtype=torch.bool)
    nm[1, 4:] = False
    nmd = nm.to(DEV)
    fm = torch.zeros(B, N, 1, dtype=torch.bool)
    fm[:, :2] = True
    xk = (torch.randn(B, N, 3) * fm).to(DEV)
    hk = (torch.randn(B, N, 8) * fm).to(DEV)
    kw = dict(sample_id_base=3, steps=3, restraint_scale=0.05, restraint_clip=0.3)
    topo = model.dynamics.topology(nmd, None, B, N)
    n0 = lib.hd_path_graph_builds(topo.ptr)
    seen, outs = [], []

    def step(what, rs, inpaint=False):
        k = dict(kw, restraints=rs) if rs is not None else dict(sample_id_base=3, steps=3)
        if inpaint:
            got = model.sample_inpaint(nmd, fm.to(DEV), xk, hk, restraint_frame="known", **k)
        else:
            got = model.sample_from_masks(nmd, None, None, **k)
        torch.cuda.synchronize()
        seen.append(int(lib.hd_path_graph_builds(topo.ptr) - n0))
        outs.append((got[0].clone(), got[1].clone()))
        print(f"step {len(seen):2d} ({what}): hd_path_graph_builds {seen[-1]}")

    step("restrained call", tables())
    step("the same call again", tables())
    step("the same tables with other values", tables(shift=0.25))
    step("add a field", tables(fields=field))
    step("the same again", tables(fields=field))
    step("attach without the field", tables())
    step("add a template", tables(templates=tpl3))
    step("the same again", tables(templates=tpl3))
    step("templates and fields together", tables(fields=field, templates=tpl3))
    step("change M", tables(fields=field, templates=tpl4))
    step("change the frame, through the inpainting path", tables(fields=field, templates=tpl4), inpaint=True)
    step("detach and run plain", None)
    step("restrained again", tables())
    print("BUILDS =", seen)

    bits = lambda t: t.contiguous().view(torch.int32)
    same = lambda i, j: all(torch.equal(bits(a), bits(b)) for a, b in zip(outs[i - 1], outs[j - 1]))
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)
    assert same(2, 1) and same(5, 4) and same(8, 7)           # a replayed call equals the freshly built one bit for bit
    assert same(6, 1) and same(13, 1)                         # ... and so does a rebuilt one, the other kinds long gone
    assert not same(3, 1) and not same(4, 1) and not same(7, 1) and not same(9, 7) and not same(12, 1)
    assert seen == BUILDS, seen
