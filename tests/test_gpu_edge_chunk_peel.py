"""GPU tier: the peeled K loop of the whole-tile edge kernel (k_edge.hpp, edge_tile_body).

The loop over the H/32 K chunks has three forms of its body: the chunks up to the third-to-last stream the next chunk of W2,
build the next chunk's operands and fetch the rows of the chunk after it; the second-to-last fetches no rows; the last does
the matrix work only.  Widths 32 / 64 / 128 have 1 / 2 / 4 chunks, so "the first chunk is the last", "the first is the
second-to-last" and "a middle chunk exists" all occur, in both arithmetics and - a forward has gated layers and a coordinate
layer - both variants of the kernel.  Width 256 (8 chunks) is there because the fp16x3 forms are peeled less far from that
width on (only the last chunk; the training forward's unscaled form not at all): another path through the same code.

Batches (N = 30, molecule sizes 5, 17, 30 first: tiles with several receiving nodes and padding rows):
  SMALL  37 tiles    widths 128, 256: k_edge_split;  below 128 every batch runs k_edge
  WHOLE  773 tiles   widths 128, 256: k_edge; 773 = 4 * 193 + 1, so three wavefronts of the last workgroup have no tile
  MIXED  1,045 tiles widths 128, 256: k_edge_mixed on a 256-CU device, 256 whole-tile workgroups of four tiles each + 21
                     column-split tiles
The tile counts are asserted, so a change of the layout or of the launch rule shows up here and not as a test that quietly
checks another kernel.
"""
import functools

import pytest
import torch

from oracle import egnn_oracle as orc
from tests.helpers import assert_parity
from tests.test_gpu_parity import DEV, PRECISIONS, build_dynamics

pytestmark = pytest.mark.gpu

N, L = 30, 1
N_CU = 256          # MI355X; the batches below are sized for it
HEAD = [5, 17, 30]
BATCHES = {"small": HEAD, "whole": HEAD + [30] * 27, "mixed": HEAD + [30] * 37}
TILES = {"small": 37, "whole": 773, "mixed": 1045}
WIDTHS = [32, 64, 128, 256]


@functools.lru_cache(maxsize=None)
def _case(H):
    """Weights, the MIXED batch (the other batches are its leading molecules) and the float64 oracle's output for the
    WHOLE batch, once per width."""
    from hierdiff_amd.weights import synthetic_state_dict
    sd_np = synthetic_state_dict(9, 0, H, L, 2, True, 700 + H, 1.0)
    cfg = orc.DynCfg(in_node_nf=9, context_node_nf=0, hidden_nf=H, n_layers=L, normalization_factor=10.0)
    xh, nm, em = orc.random_inputs(BATCHES["mixed"], 8, 71, N)
    B = xh.shape[0]
    t = torch.linspace(0.05, 0.95, B).view(B, 1)
    k = len(BATCHES["whole"])
    with torch.no_grad(), orc.float64():
        ref64 = orc.dynamics_forward(orc.as_torch_sd(sd_np), cfg, t[:k], xh[:k], nm[:k], em[:k], None, None,
                                     prefix="dynamics.egnn.").numpy()
    return sd_np, xh, nm, em, t, ref64


def _forward(dyn, which, xh, nm, em, t):
    k = len(BATCHES[which])
    nmk, emk = nm[:k].contiguous().to(DEV), em[:k].contiguous().to(DEV)
    assert dyn.topology(nmk, emk, k, N).info()["tiles"] == TILES[which]
    # the launch rule counts in rounds of four tiles per CU: MIXED (1,045 tiles) takes k_edge_mixed, and WHOLE (773) plain k_edge,
    # only where one round is 1,024 tiles
    assert torch.cuda.get_device_properties(DEV).multi_processor_count == N_CU
    return dyn._forward(t[:k].to(DEV), xh[:k].to(DEV), nmk, emk, None, None)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", WIDTHS)
def test_edge_paths_agree_bitwise_and_with_the_float64_oracle(H, precision):
    """One forward per batch.  The WHOLE batch (k_edge at every width, ragged last workgroup) against the float64 oracle
    within the bar of the parity suite; the three leading molecules bit-equal between the three batches - from width 128
    on that is k_edge_split / k_edge / k_edge_mixed on the same input, below it k_edge with the tiles in other workgroups."""
    sd_np, xh, nm, em, t, ref64 = _case(H)
    dyn = build_dynamics(sd_np, H, L)
    dyn.precision = precision
    out = {w: _forward(dyn, w, xh, nm, em, t) for w in BATCHES}
    assert_parity(out["whole"].cpu().numpy(), ref64, f"H={H} {precision} whole-tile kernel vs float64 oracle")
    k = len(HEAD)
    for w in ("whole", "mixed"):
        assert torch.isfinite(out[w]).all()
        assert torch.equal(out["small"], out[w][:k]), f"small vs {w}: max diff {(out['small'] - out[w][:k]).abs().max().item():.3e}"
    kw = len(BATCHES["whole"])
    assert torch.equal(out["whole"], out["mixed"][:kw])


@pytest.mark.autograd
@pytest.mark.parametrize("H", WIDTHS)
def test_training_forward_that_keeps_pre_activations_equals_the_plain_one(H):
    """The training forward runs the same loop with the accumulators stored as they leave it (`keep_edge_activations`, the
    whole-tile kernel: WHOLE batch); switched off, the plain kernel runs.  Same output bits, and inside the parity bar of the
    float64 oracle."""
    sd_np, xh, nm, em, t, ref64 = _case(H)
    res = {}
    for keep in (True, False):
        dyn = build_dynamics(sd_np, H, L)
        dyn.precision = "fp32"
        dyn.keep_edge_activations = keep
        k = len(BATCHES["whole"])
        xg = xh[:k].to(DEV).requires_grad_(True)
        res[keep] = dyn._forward(t[:k].to(DEV), xg, nm[:k].contiguous().to(DEV), em[:k].contiguous().to(DEV), None, None).detach()
    assert torch.equal(res[True], res[False])
    assert_parity(res[True].cpu().numpy(), ref64, f"H={H} training forward vs float64 oracle")


@pytest.mark.autograd
@pytest.mark.parametrize("H", [128, 256])
def test_fp16x3_training_forward_vs_the_float64_oracle(H):
    """`training_precision = "fp16x3"` (from width 128 on): the unscaled fp16x3 form of the loop, keeping its pre-activations."""
    sd_np, xh, nm, em, t, ref64 = _case(H)
    dyn = build_dynamics(sd_np, H, L)
    dyn.precision = "fp32"
    dyn.training_precision = "fp16x3"
    k = len(BATCHES["whole"])
    xg = xh[:k].to(DEV).requires_grad_(True)
    out = dyn._forward(t[:k].to(DEV), xg, nm[:k].contiguous().to(DEV), em[:k].contiguous().to(DEV), None, None).detach()
    assert_parity(out.cpu().numpy(), ref64, f"H={H} fp16x3 training forward vs float64 oracle")
