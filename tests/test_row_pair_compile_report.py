"""Compile report of the row kernels that carry the second round of a paired launch (fused_kernels.h: pair_row_length).

The two-round loop fits the 256 registers that two workgroups per CU leave a thread only because the operator is held in scalar
registers and the sines and cosines are made in front of the loop; a row kernel that spills is a measured loss (profiles/
APPENDIX_rejected.md #3, #10, #12).  Nothing else would fail if a change to the kernel, or another compiler, brought the spills
back, so the kernels are cross-compiled for gfx950 here (no GPU needed, a few seconds) and their resource records are read:
no scratch memory, no spilled vector registers, at most 256 vector registers and no accumulation registers (= two waves per
SIMD), code well inside the 64 KB instruction cache."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticommpy_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LENGTHS = (10, 11, 12)

# the double-precision unit's own preamble (engine_fused_f64.hip) and explicit instantiations of the three kernels
UNIT = """#define SSF_CIS2PI_OWN 1
#include "engine_fused_impl.h"
namespace ssf { namespace {
%s
} }
""" % "\n".join("template __global__ void k_row<double, 256, 2, %d>(const fused::RowArgs<double>);" % lg for lg in LENGTHS)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("rowpair")
    src, asm = d / "rows.hip", d / "rows.s"
    src.write_text(UNIT)
    # the flags of opticommpy_amd/csrc/Makefile for the fused units (CXXFLAGS + FUSED_FLAGS), device code only
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-Wno-pass-failed", "-mllvm", "-amdgpu-use-amdgpu-trackers=1", "--cuda-device-only", "-S", str(src), "-o", str(asm)],
                   check=True, capture_output=True, timeout=600)
    txt = asm.read_text()
    size = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*\.type\s+(\S+),@function.*?; codeLenInByte = (\d+)", txt, re.S | re.M)}
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", txt, re.S):
        blk = m.group(0)
        rec = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
               for k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        rec["code_bytes"] = size[name]
        out[name] = rec
    return out


@pytest.mark.parametrize("lg", LENGTHS)
def test_paired_row_kernel_has_no_scratch_and_two_waves_per_simd(records, lg):
    hits = [(n, r) for n, r in records.items() if "k_rowIdLi256ELi2ELi%dE" % lg in n]
    assert len(hits) == 1, list(records)
    name, r = hits[0]
    print(name, r)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 256 and r["agpr_count"] == 0, r
    assert r["code_bytes"] <= 48 * 1024, r                    # (44 - 45 KB today; the column kernel it alternates with shares the 64 KB)
