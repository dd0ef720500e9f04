"""Compile report of the column kernel that chains a step's final stage with the next step's H stage (fused_kernels.h: col_body,
kChain): k_col<double, 8 | 9, CM_MK, 0, SG_H | SG_RARE>.

The merged path pays only while the kernel keeps two waves per SIMD and does not spill (a column kernel that spills is a measured
loss: profiles/APPENDIX_rejected.md #12, #41).  Nothing else would fail if a change to the kernel, or another compiler, brought
spills in, so the kernels are cross-compiled for gfx950 here (no GPU needed) and their resource records are read: no scratch
memory, no spilled registers, at most 256 vector registers and no accumulation registers, code within the sum of the two kernels
it merges.  FIN and ADV are built in the same unit: they carry none of the chained code, and their figures are printed.

Figures of the kernels as committed (columns of 256 | 512): 250 | 252 vector registers, nothing spilled, no scratch,
44 200 | 50 452 bytes of code (H + rare alone was 30 096 | 34 320, FIN is 17 916 | 20 056 with this compiler).  The kernel forwards
the control block through vector registers: through scalar ones, as the other stage kernels do, twelve scalar registers were
spilled into lanes of a vector register."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticommpy_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LENGTHS = (8, 9)
SG_H_RARE, SG_ADV, SG_FIN = 9, 2, 4

# the double-precision unit's own preamble (engine_fused_f64.hip) and explicit instantiations of the stage kernels
UNIT = """#define SSF_CIS2PI_OWN 1
#include "engine_fused_impl.h"
namespace ssf { namespace {
%s
} }
""" % "\n".join("template __global__ void k_col<double, %d, fused::CM_MK, 0, %d>(const fused::ColArgs<double>);" % (lg, sg)
                for lg in LENGTHS for sg in (SG_H_RARE, SG_ADV, SG_FIN))


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("colchain")
    src, asm = d / "cols.hip", d / "cols.s"
    src.write_text(UNIT)
    # the flags of opticommpy_amd/csrc/Makefile for the fused units of the product library (CXXFLAGS + FUSED_FLAGS), device code only
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-Wno-pass-failed", "-mllvm", "-amdgpu-use-amdgpu-trackers=1", "--cuda-device-only", "-S", str(src), "-o", str(asm)],
                   check=True, capture_output=True, timeout=900)
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


def _one(records, lg, sg):
    hits = [(n, r) for n, r in records.items() if "k_colIdLi%dELi3ELi0ELi%dE" % (lg, sg) in n]
    assert len(hits) == 1, list(records)
    return hits[0]


@pytest.mark.parametrize("lg", LENGTHS)
def test_chaining_column_kernel_has_no_scratch_and_two_waves_per_simd(records, lg):
    for sg in (SG_ADV, SG_FIN):                                 # (for the record: these carry none of the chained code)
        print(*_one(records, lg, sg))
    name, r = _one(records, lg, SG_H_RARE)
    print(name, r)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 256 and r["agpr_count"] == 0, r
    # the sum of the two kernels it merges, rounded up to the next KB: H + rare 30 096 | 34 320 bytes and FIN 17 916 | 20 056 bytes
    # with the compiler and flags of this test (DESIGN.md 3.3a quotes an earlier compiler's 22.9 and 18.3 KB for columns of 256)
    assert r["code_bytes"] <= {8: 47, 9: 54}[lg] * 1024, r    # (measured: 44 200 | 50 452 bytes)
