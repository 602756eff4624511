"""CPU tier of partial inpainting (positions or features alone, per channel): the new C-ABI symbols and their refusals, the Python
and command-line argument errors (all before a device is touched), the parsing of the new `known` forms, and the restatement of
tests/inpaint_parts_reference.py pinned before a GPU sees it - against `tests.test_inpaint_cpu.replace_ref` where the masks
coincide, against its own float64 form within the kernel test's bar, and against its mutants."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from tests import inpaint_parts_reference as pr
from tests import sampling_reference as sref
from tests.test_inpaint_cpu import cpu_model, philox_raw, replace_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_inpaint_parts", "hd_inpaint_replace", "hd_inpaint_decode_fix_parts"]


def test_parts_symbols_exported_declared_and_bound(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays
    assert "PARTIAL INPAINTING" in hdr and "no per-axis mask" in hdr


def test_parts_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.hd_inpaint_parts(None, None, None, None) == -1 and b"hd_inpaint_parts" in lib.hd_last_error()
    assert lib.hd_inpaint_replace(None, None, None, None, None, None, 0.8, 0.6, 0, 0, 0, None) == -1
    assert b"hd_inpaint_replace" in lib.hd_last_error()
    assert lib.hd_inpaint_decode_fix_parts(None, None, None, None, None, None, None, None, None) == -1
    assert b"hd_inpaint_decode_fix_parts" in lib.hd_last_error()


# ----------------------------------------------------------------------------- Python and the command line

def test_python_argument_errors_come_before_the_device():
    m, _ = cpu_model(T=4, L=1)
    B, N = 2, 4
    nm = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool).view(B, N, 1)
    fm = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool).view(B, N, 1)
    xk, hk = torch.zeros(B, N, 3), torch.zeros(B, N, 8)
    for call in (lambda *a, **k: m.sample_inpaint(*a, **k), lambda *a, **k: m.inpaint_steps(torch.zeros(B, N, 11), 2, 1, *a, **k)):
        with pytest.raises(ValueError, match="fixed_mask may be None only"):
            call(nm, None, xk, hk)
        with pytest.raises(ValueError, match="fixed_mask may be None only"):
            call(nm, None, xk, hk, fixed_x_mask=fm)
        with pytest.raises(ValueError, match="fixed_mask may be None only"):
            call(nm, None, xk, hk, fixed_h_mask=fm)
        with pytest.raises(ValueError, match="fixed_x_mask must be"):
            call(nm, fm, xk, hk, fixed_x_mask=fm.expand(B, N, 3))
        with pytest.raises(ValueError, match="fixed_h_mask must be"):
            call(nm, fm, xk, hk, fixed_h_mask=fm.expand(B, N, 3))
        with pytest.raises(ValueError, match="fixed_x_mask must be a subset"):
            call(nm, fm, xk, hk, fixed_x_mask=torch.ones_like(nm))
        with pytest.raises(ValueError, match="fixed_h_mask must be a subset"):
            call(nm, None, xk, hk, fixed_x_mask=fm, fixed_h_mask=torch.ones(B, N, 8, dtype=torch.bool))
        with pytest.raises(ValueError, match="fixed_mask must be"):
            call(nm, fm[:, :3], xk, hk, fixed_h_mask=fm)
    # what inpainting refuses stays refused with partial masks
    for kw in (dict(eta=0.5, steps=2), dict(solver="dpm2m", steps=2), dict(solver="sde2m", steps=2)):
        with pytest.raises(ValueError):
            m.sample_inpaint(nm, fm, xk, hk, fixed_h_mask=fm, **kw)
    m.noise_mode = "torch"
    with pytest.raises(NotImplementedError, match="torch"):
        m.sample_inpaint(nm, None, xk, hk, fixed_x_mask=fm, fixed_h_mask=fm)
    m.noise_mode = "philox"
    m.dynamics.mode = "gnn_dynamics"
    with pytest.raises(NotImplementedError, match="gnn_dynamics"):
        m.sample_inpaint(nm, None, xk, hk, fixed_x_mask=fm, fixed_h_mask=fm)
    m.dynamics.mode = "egnn_dynamics"
    m.pocket = True
    with pytest.raises(NotImplementedError, match="pocket"):
        m.sample_inpaint(nm, None, xk, hk, fixed_x_mask=fm, fixed_h_mask=fm)
    m.pocket = False
    if not torch.cuda.is_available():           # valid input, no GPU: the library's loud error, not a fallback
        with pytest.raises(_lib.HierDiffHipError):
            m.sample_inpaint(nm, None, xk, hk, fixed_x_mask=fm, fixed_h_mask=fm.expand(B, N, 8))


def test_sample_grow_parses_the_new_forms(monkeypatch):
    m, _ = cpu_model(T=4, L=1)
    seen = {}

    def fake(node_mask, fixed_mask, x_known, h_known, **kw):
        seen.update(nm=node_mask, fm=fixed_mask, xk=x_known, hk=h_known, kw=kw)
        B, N = node_mask.shape[:2]
        return torch.zeros(B, N, 3), torch.zeros(B, N, 8)

    monkeypatch.setattr(m, "sample_inpaint", fake)
    g = torch.Generator().manual_seed(0)
    x3, h3, h2 = torch.randn(3, 3, generator=g), torch.randn(3, 8, generator=g), torch.randn(2, 8, generator=g)
    hm = torch.zeros(2, 8, dtype=torch.bool)
    hm[0, [0, 3, 7]] = True
    known = [{"x": x3}, {"h": h2, "h_mask": hm}, {"x": x3, "h": h3, "x_mask": torch.tensor([True, False, True])},
             {"x": x3, "h": h3, "h_mask": torch.tensor([False, True, True])}]
    out = m.sample_grow(known, [4, 2, 3, 5], "cpu")
    assert [tuple(o["x"].shape) for o in out] == [(4, 3), (2, 3), (3, 3), (5, 3)]
    fxm, fhm = seen["kw"]["fixed_x_mask"], seen["kw"]["fixed_h_mask"]
    assert fxm.shape == (4, 5, 1) and fhm.shape == (4, 5, 8) and fxm.dtype == fhm.dtype == torch.bool
    assert fxm[:, :, 0].tolist() == [[True, True, True, False, False], [False] * 5, [True, False, True, False, False],
                                     [True, True, True, False, False]]
    assert not fhm[0].any() and torch.equal(fhm[1, :2], hm) and not fhm[1, 2:].any()
    assert fhm[2, :3].all() and not fhm[2, 3:].any()
    assert fhm[3].all(1).tolist() == [False, True, True, False, False] and fhm[3].any(1).tolist() == [False, True, True, False, False]
    assert torch.equal(seen["xk"][0, :3], x3) and torch.equal(seen["hk"][1, :2], h2) and not seen["hk"][0].any()
    assert seen["nm"][:, :, 0].sum(1).tolist() == [4, 2, 3, 5]
    # whole entries without masks: the whole-node call, as before
    m.sample_grow([{"x": x3, "h": h3}], [4], "cpu")
    assert "fixed_x_mask" not in seen["kw"] and "fixed_h_mask" not in seen["kw"]
    for bad, what in (([{}], "need 'x'"), ([{"x": x3, "h": h2}], r"known\[0\]"), ([{"h": h2, "x_mask": torch.ones(2, dtype=torch.bool)}], "x_mask"),
                      ([{"h": h2, "h_mask": torch.ones(3, dtype=torch.bool)}], "h_mask"), ([{"x": x3, "h_mask": torch.ones(3, dtype=torch.bool)}], "h_mask"),
                      ([{"h": h3}], "smaller")):
        with pytest.raises(ValueError, match=what):
            m.sample_grow(bad, [2], "cpu")


def test_cli_known_parts_and_read_known(tmp_path, capsys):
    from hierdiff_amd import sampler
    with pytest.raises(SystemExit):
        sampler.main(["--known-parts", "h"])
    with pytest.raises(SystemExit):
        sampler.main(["--known", "x.pkl", "--grow", "0", "--known-parts", "z"])
    args = sampler.parse_args(["--known", "x.pkl", "--grow", "0", "--known-parts", "h", "--restraints", "r.pkl", "--restraint-frame", "known"])
    assert args.known_parts == "h" and args.restraint_frame == "known"
    with pytest.raises(SystemExit):
        sampler.parse_args(["--help"])
    assert "model's frame (tau = 0)" in " ".join(capsys.readouterr().out.split())      # the help says what --known-parts h does to the frame
    res = [{"x": torch.randn(3, 3)}, {"h": torch.randn(2, 8), "h_mask": torch.ones(2, dtype=torch.bool)}]
    a, b, c = tmp_path / "a.pkl", tmp_path / "b.pkl", tmp_path / "c.pt"
    pickle.dump(res, open(a, "wb"))
    pickle.dump((res, ["t0", "t1"]), open(b, "wb"))
    torch.save(res, c)
    for p in (a, b, c):
        got = sampler.read_known(str(p))
        assert len(got) == 2 and torch.equal(got[0]["x"], res[0]["x"]) and torch.equal(got[1]["h"], res[1]["h"]) and "h" not in got[0]
    pickle.dump([{"y": 1}], open(a, "wb"))
    with pytest.raises(ValueError):
        sampler.read_known(str(a))
    both = [{"x": torch.zeros(3, 3), "h": torch.zeros(3, 8), "x_mask": torch.ones(3, dtype=torch.bool), "h_mask": torch.ones(3, dtype=torch.bool)}]
    assert sampler.known_parts(both, "both") is both
    assert set(sampler.known_parts(both, "h")[0]) == {"h", "h_mask"} and set(sampler.known_parts(both, "x")[0]) == {"x", "x_mask"}
    assert sampler.known_rows(sampler.known_parts(both, "h")[0]) == 3
    with pytest.raises(ValueError, match="known-parts h"):
        sampler.known_parts(res, "h")


# ----------------------------------------------------------------------------- the restatement, pinned

def _raw(c):
    g = torch.Generator().manual_seed(7 + c.N + c.F)
    return torch.randn(c.B, c.N, 3, generator=g), torch.randn(c.B, c.N, c.F, generator=g)


@pytest.mark.parametrize("N,F", pr.KERNEL_SHAPES)
def test_coinciding_masks_give_the_bits_of_the_whole_node_restatement(N, F):
    c = pr.kernel_case(N, F)
    raw = _raw(c)
    nmf = c.nm[:, :, None].float()
    for fm in (c.fx, c.fh.any(2), torch.zeros_like(c.fx), c.nm.clone()):
        fmf = (fm & c.nm)[:, :, None].float()
        want = replace_ref(c.z, c.known * fmf, nmf, fmf, c.alpha, c.sigma, raw)
        got = pr.replace_parts_ref(c.z, c.known, nmf, fm[:, :, None], fm[:, :, None].expand(c.B, N, F), c.alpha, c.sigma, raw)
        assert torch.equal(got, want)


@pytest.mark.parametrize("N,F", pr.KERNEL_SHAPES)
def test_positions_free_keeps_them_and_features_free_keeps_those(N, F):
    c = pr.kernel_case(N, F)
    raw = _raw(c)
    nmf = c.nm[:, :, None].float()
    got = pr.replace_parts_ref(c.z, c.known, nmf, torch.zeros_like(c.fx), c.fh, c.alpha, c.sigma, raw)
    assert torch.equal(got[:, :, :3], c.z[:, :, :3])                         # |Fx| = 0: the position part unchanged
    rep = (c.fh & c.nm[:, :, None])
    assert not torch.equal(got[:, :, 3:], c.z[:, :, 3:]) and torch.equal(got[:, :, 3:][~rep], c.z[:, :, 3:][~rep])
    got = pr.replace_parts_ref(c.z, c.known, nmf, c.fx, torch.zeros_like(c.fh), c.alpha, c.sigma, raw)
    assert torch.equal(got[:, :, 3:], c.z[:, :, 3:])                         # fh empty: the features unchanged
    assert float((got[:, :, :3] * nmf).sum(1).abs().max()) < 1e-5 * float(got[:, :, :3].abs().max())
    assert not torch.equal(got[:, :, :3], c.z[:, :, :3])
    assert torch.all(got[~c.nm] == 0)


@pytest.mark.parametrize("N,F", pr.KERNEL_SHAPES)
def test_fp32_restatement_sits_far_inside_the_bar_and_every_mutant_far_outside(lib, N, F):
    """The kernel test's inputs, normals from the generator's host twin.  The float32 evaluation of the restatement against its
    float64 form: inside the bar (BOUND = 8 units).  Each mutant, in float64, against the float64 form: the factor by which it
    misses the bar is printed, and has to exceed 1 wherever the mutant is not the identity by construction (F = 1 has one channel:
    "any channel" and the transposed read are the mask itself)."""
    c = pr.kernel_case(N, F)
    ids = [c.base + b for b in range(c.B)]
    raw = philox_raw(lib, c.seed, ids, c.draw, N, F)
    nm = c.nm[:, :, None]
    args64 = (c.z.double(), c.known.double(), nm, c.fx, c.fh, c.alpha, c.sigma, tuple(r.double() for r in raw))
    ref = pr.replace_parts_ref(*args64)
    mag = pr.replace_parts_mag(c.z, c.known, nm, c.fx, c.fh, c.alpha, c.sigma, raw)
    f32 = pr.replace_parts_ref(c.z, c.known, nm, c.fx, c.fh, c.alpha, c.sigma, raw)
    r32 = pr.kernel_ratio(f32.numpy(), ref.numpy(), mag.numpy())
    print(f"replace N={N} F={F}: fp32 restatement worst err / bound {r32:.3f} (1.0 = {sref.BOUND:g} units of 2^-23 sum|terms|)")
    assert r32 <= 1.0
    for mutant in pr.MUTANTS:
        out = pr.replace_parts_ref(*args64, mutant=mutant)
        err = np.abs(out.numpy() - ref.numpy())
        factor = float((err / np.maximum(sref.BOUND * sref.U * mag.numpy(), 1e-300)).max())
        print(f"replace N={N} F={F}: mutant {mutant} misses the bar by a factor of {factor:.3g}")
        if F == 1 and mutant in ("any_channel", "transposed"):
            assert factor == 0.0
        else:
            assert factor > 1.0, (mutant, factor)


def test_decode_fix_restatement():
    c = pr.kernel_case(5, 8)
    g = torch.Generator().manual_seed(1)
    x, h = torch.randn(c.B, 5, 3, generator=g), torch.randn(c.B, 5, 8, generator=g)
    xk, hk = c.known[:, :, :3] * pr.NV0, c.known[:, :, 3:]
    nm = c.nm[:, :, None]
    x1, h1 = pr.decode_fix_parts_ref(x, h, xk, hk, nm, c.fx, c.fh)
    rep = c.fh & nm
    assert torch.equal(h1[rep], hk[rep]) and torch.equal(h1[~rep], h[~rep])
    fxv = c.fx & c.nm
    assert torch.equal(x1[~fxv], x[~fxv])
    d = (x1 - xk)[1][fxv[1]]
    assert float((d - d[0]).abs().max()) <= 2 * float(np.spacing(np.float32(x1[1].abs().max())))
