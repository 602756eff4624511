"""The packed-VALU form of the exact-fp32 edge kernel (HD_EDGE_PACKED, k_edge.hpp), read from the assembly hipcc emits (no GPU
needed).

The plain fp32 launch runs k_edge<256, *, 0, HD_EDGE_PACKED>: operand generation, the mul / +1 / mul stages of the epilogue SiLU and
the gate dot on pairs of values (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32).  The file is built with -fno-slp-vectorize and hipcc
splits packed instructions behind an MFMA back into scalar ones unless it is stopped (the empty asm in front of the operand
generation), so whether the packed instructions are there, and only there, is a property of the emitted code: this test pins it.

Regions of a kernel: a chunk body starts at the inline-asm block of four ds_read_b128 that fetches its first unit's fragments
(lds_read4); the code in front of the first is the prologue, the code behind the kernel's last MFMA the epilogue.
"""
import re
import subprocess

import pytest

from hierdiff_amd import build as hbuild
from tests.test_edge_kloop_schedule import kernel_bodies, kernel_metadata

PACKED_ABL = 2048            # HD_EDGE_PACKED
SYMBOL = "_Z6k_edgeILi256ELb{coord}ELi0ELi{abl}EEv8EdgeArgs"
TU = """#include "k_edge.hpp"
static_assert(HD_EDGE_PACKED == 2048, "the flag's value is part of the kernel's name");
template __global__ void k_edge<256, false, 0>(EdgeArgs);
template __global__ void k_edge<256, true, 0>(EdgeArgs);
template __global__ void k_edge<256, false, 0, HD_EDGE_PACKED>(EdgeArgs);
template __global__ void k_edge<256, true, 0, HD_EDGE_PACKED>(EdgeArgs);
"""
CHUNK_BODIES = 3             # the runtime loop's body + the two peeled bodies (edge_peel_level = 2 in fp32)
PACKED_OPS = ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")


def _hipcc():
    try:
        return hbuild._hipcc()
    except RuntimeError:
        return None


def regions(body: list) -> dict:
    """{'prologue' | 'chunk0' .. | 'epilogue': [instructions]} of one kernel (see the module docstring)."""
    cuts, i = [], 0
    while i < len(body):
        if body[i] == ";;#ASMSTART":
            j = i + 1
            while body[j] != ";;#ASMEND":
                j += 1
            block = body[i + 1:j]
            if len(block) == 4 and all(b.startswith("ds_read_b128") for b in block):
                cuts.append(i)
            i = j
        i += 1
    last_mfma = max(k for k, ins in enumerate(body) if ins.startswith("v_mfma"))
    bounds = [0] + cuts + [last_mfma + 1, len(body)]
    names = ["prologue"] + [f"chunk{k}" for k in range(len(cuts))] + ["epilogue"]
    return {nm: body[a:b] for nm, a, b in zip(names, bounds[:-1], bounds[1:])}


def valu(seg: list) -> list:
    """The vector-ALU instructions of a region that are not matrix instructions."""
    return [s for s in seg if s.startswith("v_") and not s.startswith("v_mfma")]


def packed_f32(seg: list) -> list:
    return [s for s in seg if re.match(r"v_pk_\w+_f32\b", s)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("packed")
    src, out = d / "edge_tu.hip", d / "edge_tu.s"
    src.write_text(TU)
    cmd = [hipcc] + hbuild.KERNEL_FLAGS + ["--cuda-device-only", "-S", "-I", hbuild.CSRC, "-o", str(out), str(src)]
    proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr
    return out.read_text()


@pytest.mark.parametrize("coord", [0, 1])
def test_packed_form_fits_two_waves_per_simd(asm, coord):
    meta = kernel_metadata(asm, SYMBOL.format(coord=coord, abl=PACKED_ABL))
    print(coord, meta)
    assert meta["vgpr_spill"] == 0 and meta["sgpr_spill"] == 0 and meta["scratch"] == 0, meta
    assert meta["vgpr"] <= 256, meta


@pytest.mark.parametrize("coord", [0, 1])
def test_packed_ops_in_chunk_bodies_and_epilogue(asm, coord):
    bodies = kernel_bodies(asm)
    pk = regions(bodies[SYMBOL.format(coord=coord, abl=PACKED_ABL)])
    sc = regions(bodies[SYMBOL.format(coord=coord, abl=0)])
    assert sorted(pk) == sorted(sc) == sorted(["prologue", "epilogue"] + [f"chunk{k}" for k in range(CHUNK_BODIES)])
    for nm in sorted(pk):
        print(f"coord={coord} {nm}: VALU scalar form {len(valu(sc[nm]))}, packed form {len(valu(pk[nm]))} "
              f"({len(packed_f32(pk[nm]))} packed)")
    # the bodies that produce operands (the loop's and the second-to-last chunk's; the last chunk produces nothing) and the epilogue
    for nm in ["chunk0", "chunk1", "epilogue"]:
        for op in PACKED_OPS:
            assert any(s.startswith(op) for s in pk[nm]), f"no {op} in {nm}"
        assert len(valu(pk[nm])) < len(valu(sc[nm])), (nm, len(valu(pk[nm])), len(valu(sc[nm])))
    # a quad of operands: 12 packed + 8 transcendental instructions instead of 32; four quads a body
    for nm in ["chunk0", "chunk1"]:
        assert len(packed_f32(pk[nm])) == 48, (nm, len(packed_f32(pk[nm])))
    assert len(valu(pk["chunk2"])) <= len(valu(sc["chunk2"])) + 1 and not packed_f32(pk["chunk2"])
    # epilogue: 8 column tiles x (mul, +1, mul, gate fma) x 8 pairs
    assert len(packed_f32(pk["epilogue"])) == 256, len(packed_f32(pk["epilogue"]))


@pytest.mark.parametrize("coord", [0, 1])
def test_scalar_form_has_no_packed_f32(asm, coord):
    body = kernel_bodies(asm)[SYMBOL.format(coord=coord, abl=0)]
    assert packed_f32(body) == []


def test_build_audits_the_packed_instantiations():
    assert hbuild._packed_edge(SYMBOL.format(coord=0, abl=PACKED_ABL)) and hbuild._packed_edge(SYMBOL.format(coord=1, abl=PACKED_ABL))
    assert not hbuild._packed_edge(SYMBOL.format(coord=0, abl=0))
    spill = {SYMBOL.format(coord=0, abl=PACKED_ABL): {"VGPRs": 256, "AGPRs": 0, "ScratchSize": 16, "VGPRs Spill": 4}}
    wide = {SYMBOL.format(coord=1, abl=PACKED_ABL): {"VGPRs": 256, "AGPRs": 8, "ScratchSize": 0, "VGPRs Spill": 0}}
    fine = {SYMBOL.format(coord=1, abl=PACKED_ABL): {"VGPRs": 244, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0}}
    assert len(hbuild.audit(spill)) == 1 and len(hbuild.audit(wide)) == 1 and hbuild.audit(fine) == []
