"""The plain k_edge launch after the packed-VALU form (exact fp32, H = 256: HD_EDGE_PACKED) and the neighbour sums by row quad (every
whole-tile edge kernel, both arithmetics) - k_edge.hpp.  One block (two GCL layers + the coordinate layer) at H = 128 and 256:

  * batch A: molecules of 2, 3, 5, 7 and 30 nodes at the head of a 150-molecule batch (more than 3,072 tiles: plain k_edge) - tail
    tiles of many short segments, a segment over several tiles, padding rows and padding tiles;
  * batch B: twenty 2-node molecules at the head of such a batch - a molecule of two nodes has two edges, tails sit at 4-row-aligned
    offsets, so their tile is the fullest the layout makes: sixteen one-row segments, two per row quad side by side with padding;

each against the float64 oracle at the bar of tests/test_gpu_parity.py (assert_parity) and torch.equal with the same molecules run
alone (k_edge_split, which keeps the scalar arithmetic and the full segment loop);

  * batch A with a NaN in one input feature of the 3-node molecule, whose edges share a tail tile with its neighbours': the select
    path of the segment sums skips the same row quads.  The velocity is reset batch-wide as in the reference (en_dynamics.py:109-111),
    the features of every other molecule keep the bits they have without the NaN, the NaN molecule's features are NaN.
"""
import pytest
import torch

from oracle import egnn_oracle as orc
from tests.helpers import assert_parity
from tests.test_gpu_parity import DEV, PRECISIONS, build_dynamics

pytestmark = pytest.mark.gpu

N_MAX = 30
HEADS = {"mixed": [2, 3, 5, 7, 30], "pairs": [2] * 20}
B_BIG = 150
NAN_MOL = 1                  # the 3-node molecule of the "mixed" head
_REF = {}


def _case(H, head):
    """(weights, inputs of the 150-molecule batch, float64 reference of the head molecules): once per width and head."""
    if (H, head) not in _REF:
        from hierdiff_amd.weights import synthetic_state_dict
        sd_np = synthetic_state_dict(9, 0, H, 1, 2, True, 900 + H, 1.0)
        sizes = HEADS[head] + [30] * (B_BIG - len(HEADS[head]))
        xh, nm, em = orc.random_inputs(sizes, 8, 83 + len(HEADS[head]), N_MAX)
        t = torch.linspace(0.05, 0.95, xh.shape[0]).view(-1, 1)
        cfg = orc.DynCfg(in_node_nf=9, context_node_nf=0, hidden_nf=H, n_layers=1, normalization_factor=10.0)
        k = len(HEADS[head])
        with torch.no_grad(), orc.float64():
            ref = orc.dynamics_forward(orc.as_torch_sd(sd_np), cfg, t[:k], xh[:k], nm[:k], em[:k].contiguous(), None, None,
                                       prefix="dynamics.egnn.")
        _REF[(H, head)] = (sd_np, xh, nm, em, t, ref.numpy())
    return _REF[(H, head)]


def _forward(dyn, t, xh, nm, em, k):
    nmk, emk = nm[:k].contiguous().to(DEV), em[:k].contiguous().to(DEV)
    tiles = dyn.topology(nmk, emk, k, N_MAX).info()["tiles"]
    return dyn._forward(t[:k].to(DEV), xh[:k].contiguous().to(DEV), nmk, emk, None, None), tiles


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("head", sorted(HEADS))
@pytest.mark.parametrize("H", [128, 256])
def test_plain_launch_vs_float64_and_alone(H, head, precision):
    sd_np, xh, nm, em, t, ref = _case(H, head)
    dyn = build_dynamics(sd_np, H, 1)
    dyn.precision = precision
    k = len(HEADS[head])
    alone, tiles = _forward(dyn, t, xh, nm, em, k)
    assert 0 < tiles <= 512, tiles                                # the column-split kernel
    big, tiles = _forward(dyn, t, xh, nm, em, B_BIG)
    assert tiles > 3072, tiles                                    # past the mixed range: plain k_edge
    assert_parity(alone.cpu().numpy(), ref, f"H={H} {precision}, {head} head alone")
    assert_parity(big[:k].cpu().numpy(), ref, f"H={H} {precision}, {head} head of {B_BIG}")
    assert torch.equal(big[:k], alone), f"k_edge vs alone: max diff {(big[:k] - alone).abs().max().item():.3e}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", [128, 256])
def test_nan_molecule_stays_inside_its_segments(H, precision):
    sd_np, xh, nm, em, t, _ = _case(H, "mixed")
    dyn = build_dynamics(sd_np, H, 1)
    dyn.precision = precision
    clean, tiles = _forward(dyn, t, xh, nm, em, B_BIG)
    assert tiles > 3072, tiles
    assert torch.isfinite(clean).all()
    bad = xh.clone()
    bad[NAN_MOL, 0, 3] = float("nan")                            # one feature of one node
    dirty, _ = _forward(dyn, t, bad, nm, em, B_BIG)
    others = [b for b in range(B_BIG) if b != NAN_MOL]
    assert torch.equal(dirty[others][..., 3:], clean[others][..., 3:]), "a neighbour's features changed with the NaN molecule"
    assert torch.equal(dirty[..., :3], torch.zeros_like(dirty[..., :3])), "velocity reset is batch-wide"
    valid = nm[NAN_MOL, :, 0].bool().to(DEV)
    assert torch.isnan(dirty[NAN_MOL][valid][:, 3:]).all() and (dirty[NAN_MOL][~valid] == 0).all()
