"""GPU tier (-m gpu): when the cached graphs of the path loop are rebuilt as steering, diversity and a sink come and go.  One sequence
of Python calls on one topology - steered restrained calls with another rho, beta and P, diverse calls with another strength, length and
number of scale rows, recording calls of the state and of the data prediction, a plain call in between - with hd_path_graph_builds and
hd_chain_graph_builds read after every step, a replayed call compared bit for bit with the freshly built one in three places, and the
first steered call repeated at the end.

The expected counts are not derived from the code under test: they were printed by this test on commit bac1693 (the parent of the
change that gathered the steering, diversity and sink state of a topology into structs and their key parts into sub-keys) and are kept
as literals.  Model: the `small_model` of the restraint tests (H = 32, one layer, T = 20), B = 4 as two groups of 2 (one group of 4 in
step 5), N = 5 with four valid nodes in every row, a 3-transition path, P = Q = A = 1."""
import pytest
import torch

from hierdiff_amd import _lib
from hierdiff_amd.diversity import Diversity
from hierdiff_amd.restraints import Restraints
from tests.test_restraint_cpu import small_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, N = 4, 5

# (hd_path_graph_builds, hd_chain_graph_builds) after every step, less their values before the first (commit bac1693)
BUILDS = [(1, 0), (1, 0), (2, 0), (2, 0), (3, 0), (4, 0), (4, 0), (5, 0), (6, 0), (7, 0), (7, 1), (7, 1), (7, 2), (8, 2), (9, 2)]


def test_when_the_path_and_chain_graphs_are_rebuilt():
    lib = _lib.load()
    torch.manual_seed(7)
    model = small_model().to(DEV)
    model.seed, model.use_graph = 11, True
    model.eval()
    rs = lambda: Restraints(obstacles=[[0.5, 0.0, 0.0, 1.5, 2.0]], pairs=[[0, 1, 2.0, 2.5, 1.0]], anchors=[[2, 1.0, 1.0, 1.0, 0.25, 1.5]])
    nm = torch.ones(B, N, 1, dtype=torch.bool)
    nm[:, 4:] = False                                    # equal masks: the rows form two groups of 2 or one of 4
    nmd = nm.to(DEV)
    base = dict(sample_id_base=3, steps=3, eta=1.0)
    steered = dict(base, restraint_scale=0.05, restraint_clip=0.3, particles=2, steer_scale=1.0, steer_ess=0.5)
    # (synthetic weights: the data predictions of the noisy levels are hundreds of units wide, so a length of 50 keeps the Gaussian alive)
    diverse = dict(particles=2, length=50.0, strength=2500.0, clip=0.3)
    topo = model.dynamics.topology(nmd, None, B, N)
    p0, c0 = lib.hd_path_graph_builds(topo.ptr), lib.hd_chain_graph_builds(topo.ptr)
    seen, outs = [], []

    def step(what, **kw):
        if "particles" in kw:
            kw["restraints"] = rs()
        got = model.sample_from_masks(nmd, None, None, **kw)
        torch.cuda.synchronize()
        seen.append((int(lib.hd_path_graph_builds(topo.ptr) - p0), int(lib.hd_chain_graph_builds(topo.ptr) - c0)))
        outs.append(tuple(t.clone() for t in got))
        print(f"step {len(seen):2d} ({what}): hd_path_graph_builds {seen[-1][0]}, hd_chain_graph_builds {seen[-1][1]}")

    step("steered restrained call", **steered)
    step("the same call again", **steered)
    step("another steer_ess", **dict(steered, steer_ess=0.8))
    step("another steer_scale, the same K", **dict(steered, steer_ess=0.8, steer_scale=2.0))
    step("particles 2 -> 4", **dict(steered, steer_ess=0.8, steer_scale=2.0, particles=4))
    step("detach steering, a diverse call", diversity=Diversity(**diverse), **base)
    step("the same again", diversity=Diversity(**diverse), **base)
    step("another strength", diversity=Diversity(**dict(diverse, strength=5000.0)), **base)
    step("another length", diversity=Diversity(**dict(diverse, strength=5000.0, length=60.0)), **base)
    step("scale rows 1 -> G", diversity=Diversity(**dict(diverse, strength=5000.0, length=60.0, scale=[1.0, 0.5])), **base)
    step("a recording call", keep_frames=2, **base)
    step("the same again", keep_frames=2, **base)
    step("record the data prediction", keep_frames=2, record="x0", **base)
    step("a plain call", **base)
    step("the first steered call once more", **steered)
    print("BUILDS =", seen)

    bits = lambda t: t.contiguous().view(torch.int32)
    same = lambda i, j: len(outs[i - 1]) == len(outs[j - 1]) and all(torch.equal(bits(a), bits(b)) for a, b in zip(outs[i - 1], outs[j - 1]))
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)
    assert all(len(outs[i - 1]) == 3 for i in (11, 12, 13))   # the recording calls return their chain
    assert same(2, 1) and same(7, 6) and same(12, 11)         # a replayed call equals the freshly built one bit for bit
    assert same(15, 1)                                        # ... and so does a rebuilt one, the other terms long gone
    assert not same(6, 14)                                    # the diverse steps run the term whose key they count
    assert seen == BUILDS, seen
