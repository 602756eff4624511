"""The edge kernels after the K-loop units were fenced (k_edge.hpp): one block (two GCL layers + the coordinate layer) at every
width, i.e. every number of K chunks (H = 32, 64, 128, 256: 1, 2, 4, 8 - the last-only, the second-to-last + last and the loop +
both peeled forms), both arithmetics, on three molecules of 5, 7 and 30 nodes (tiles of many segments, a segment over many tiles,
the short tails of several molecules in one tile, padding rows and padding tiles).

  * against the float64 evaluation of the oracle, at the bar tests/test_gpu_parity.py holds single-block models to (assert_parity);
  * torch.equal between the three kernel families that share the arithmetic: the molecules alone (k_edge_split at H >= 128), at the
    head of a 46-molecule batch (k_edge_mixed) and at the head of a 150-molecule batch (k_edge) - chosen by the batch size as in
    test_mixed_edge_launch_is_bit_identical.
"""
import pytest
import torch

from oracle import egnn_oracle as orc
from tests.helpers import assert_parity
from tests.test_gpu_parity import DEV, PRECISIONS, build_dynamics

pytestmark = pytest.mark.gpu

N_HEAD = [5, 7, 30]
N_MAX = 30
_REF = {}


def _case(H):
    """(weights, inputs of the 150-molecule batch, float64 reference of its first three molecules): once per width."""
    if H not in _REF:
        from hierdiff_amd.weights import synthetic_state_dict
        sd_np = synthetic_state_dict(9, 0, H, 1, 2, True, 700 + H, 1.0)
        xh, nm, em = orc.random_inputs(N_HEAD + [30] * 147, 8, 71, N_MAX)
        t = torch.linspace(0.05, 0.95, xh.shape[0]).view(-1, 1)
        cfg = orc.DynCfg(in_node_nf=9, context_node_nf=0, hidden_nf=H, n_layers=1, normalization_factor=10.0)
        k = len(N_HEAD)
        with torch.no_grad(), orc.float64():
            ref = orc.dynamics_forward(orc.as_torch_sd(sd_np), cfg, t[:k], xh[:k], nm[:k], em[:k].contiguous(), None, None,
                                       prefix="dynamics.egnn.")
        _REF[H] = (sd_np, xh, nm, em, t, ref.numpy())
    return _REF[H]


def _forward(dyn, t, xh, nm, em, k):
    nmk, emk = nm[:k].contiguous().to(DEV), em[:k].contiguous().to(DEV)
    tiles = dyn.topology(nmk, emk, k, N_MAX).info()["tiles"]
    return dyn._forward(t[:k].to(DEV), xh[:k].to(DEV), nmk, emk, None, None), tiles


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", [32, 64, 128, 256])
def test_one_block_vs_float64_and_across_kernel_families(H, precision):
    sd_np, xh, nm, em, t, ref = _case(H)
    dyn = build_dynamics(sd_np, H, 1)
    dyn.precision = precision
    k = len(N_HEAD)
    alone, tiles = _forward(dyn, t, xh, nm, em, k)
    assert 0 < tiles <= 512, tiles                                # H >= 128: the column-split kernel
    assert_parity(alone.cpu().numpy(), ref, f"H={H} {precision}, {N_HEAD} alone")
    # 46 molecules: more than one whole-tile workgroup per CU (1,024 tiles) and at most one left-over tile per CU behind the
    # full rounds - the mixed launch in both arithmetics (H >= 128); 150 molecules: past the mixed range, plain k_edge
    mid, tiles = _forward(dyn, t, xh, nm, em, 46)
    assert 1024 < tiles <= 1024 + 256, tiles
    big, tiles = _forward(dyn, t, xh, nm, em, 150)
    assert tiles > 3072, tiles
    assert_parity(big[:k].cpu().numpy(), ref, f"H={H} {precision}, head of 150")
    assert torch.equal(big[:k], alone), f"k_edge vs alone: max diff {(big[:k] - alone).abs().max().item():.3e}"
    assert torch.equal(big[:k], mid[:k]), f"k_edge vs head of 46: max diff {(big[:k] - mid[:k]).abs().max().item():.3e}"
