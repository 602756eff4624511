"""Instruction placement in the K loop of the exact-fp32 edge kernel, read from the assembly hipcc emits (no GPU needed).

A unit of the K loop is 16 v_mfma_f32_32x32x2_f32 on four W2 fragments.  The fragments of unit u+1 are fetched by four inline-asm
ds_read_b128 each (lds_read1, k_edge.hpp; unit 0: lds_read4) and released by an s_waitcnt lgkmcnt in front of unit u+1; at least 12
MFMAs of unit u have to sit BETWEEN the last of the four reads and that wait, or every unit starts with an exposed LDS round trip.
hipcc is free to move the MFMA builtins across the volatile asms, and did (count 0 everywhere, EXPERIMENTS.md section AM): this
test pins the emitted order.
"""
import re
import subprocess

import pytest

from hierdiff_amd import build as hbuild

KERNELS = {"gcl": "_Z6k_edgeILi256ELb0ELi0ELi0EEv8EdgeArgs", "coord": "_Z6k_edgeILi256ELb1ELi0ELi0EEv8EdgeArgs"}
TU = """#include "k_edge.hpp"
template __global__ void k_edge<256, false, 0>(EdgeArgs);
template __global__ void k_edge<256, true, 0>(EdgeArgs);
"""
UNITS_PER_CHUNK = 8          # H = 256: 4 k-quads x 2 halves of the column tiles
CHUNK_BODIES = 3             # the runtime loop's body + the two peeled bodies (edge_peel_level = 2 in fp32)
MFMA_PER_UNIT = 16
MIN_COVERED = 12


def _hipcc():
    try:
        return hbuild._hipcc()
    except RuntimeError:
        return None


def kernel_bodies(asm: str) -> dict:
    """{symbol: [instruction lines]} of every function of an AMDGPU assembly file (comments, labels, directives dropped)."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or s[0] in ".;" or s.endswith(":"):
            if cur is not None and s in (";;#ASMSTART", ";;#ASMEND"):
                cur.append(s)
            continue
        cur.append(s)
    return out


def fragment_groups(body: list) -> list:
    """One (first read's offset, MFMAs between the group's last read and the next s_waitcnt lgkmcnt) per group of four W2
    fragment reads.  The fragment reads are the ds_read_b128 of inline-asm blocks (lds_read4: four in a block, lds_read1: one;
    the w_r / w_d reads are compiler-generated and stand outside such blocks); four consecutive ones are a unit's fragments."""
    reads, i = [], 0                      # (index of the instruction behind the read's asm block, offset)
    while i < len(body):
        if body[i] != ";;#ASMSTART":
            i += 1
            continue
        j = i + 1
        while body[j] != ";;#ASMEND":
            j += 1
        block = body[i + 1:j]
        i = j + 1
        if block and all(b.startswith("ds_read_b128") for b in block):
            for b in block:
                m = re.search(r"offset:(\w+)", b)
                reads.append((j + 1, int(m.group(1), 0) if m else 0))
    assert len(reads) % 4 == 0, len(reads)
    groups = []
    for g in range(0, len(reads), 4):
        covered = 0
        for ins in body[reads[g + 3][0]:]:
            if ins.startswith("s_waitcnt") and "lgkmcnt" in ins:
                break
            if ins.startswith("v_mfma"):
                covered += 1
        groups.append((reads[g][1], covered))
    return groups


def kernel_metadata(asm: str, symbol: str) -> dict:
    """Register counts of one kernel from the amdhsa metadata: an entry runs from `.agpr_count` (first key) to `.wavefront_size`."""
    entries = re.findall(r"- \.agpr_count.*?\.wavefront_size:\s+\d+", asm, re.S)
    text = next(e for e in entries if re.search(r"\.name:\s+" + re.escape(symbol) + r"\s", e))
    get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", text).group(1))
    return {"vgpr": get("vgpr_count"), "vgpr_spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
            "scratch": get("private_segment_fixed_size")}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("kloop")
    src, out = d / "edge_tu.hip", d / "edge_tu.s"
    src.write_text(TU)
    cmd = [hipcc] + hbuild.KERNEL_FLAGS + ["--cuda-device-only", "-S", "-I", hbuild.CSRC, "-o", str(out), str(src)]
    proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr
    return out.read_text()


@pytest.mark.parametrize("form", sorted(KERNELS))
def test_fragment_reads_run_under_the_mfmas(asm, form):
    body = kernel_bodies(asm)[KERNELS[form]]
    groups = fragment_groups(body)
    print(form, "(first offset, MFMAs between reads and wait):", groups)
    assert len(groups) == CHUNK_BODIES * UNITS_PER_CHUNK, groups
    first = [g for g in groups if g[0] == 0]
    assert len(first) == CHUNK_BODIES, "one unit-0 read (offset 0, covered by the stream issue) per chunk body"
    later = [g for g in groups if g[0] != 0]
    assert all(MIN_COVERED <= c <= MFMA_PER_UNIT for _, c in later), later


@pytest.mark.parametrize("form", sorted(KERNELS))
def test_no_spill_two_waves_per_simd(asm, form):
    meta = kernel_metadata(asm, KERNELS[form])
    print(form, meta)
    assert meta["vgpr_spill"] == 0 and meta["scratch"] == 0, meta
    assert meta["vgpr"] <= 256, meta
