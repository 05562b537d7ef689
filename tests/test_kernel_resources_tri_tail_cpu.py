"""Build-time guard for the triangular-tail instantiations of the posterior's two row-tile kernels (runs without a GPU: hipcc
cross-compiles gfx950), by the method of tests/test_kernel_resources_cpu.py: compile, read the resource remarks.  The tail variants hold
several copies of the k-tile body, which is where a register allocation can tip over: no scratch, the accumulators stay in 256 VGPRs
at one workgroup per CU (256-row kernel) and in 128 at two (128-row kernel), and the LDS footprints are the general kernels'."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    src = os.path.join(ROOT, "gp_algos_amd", "csrc", "kernels_gemm.hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path_factory.mktemp("tri") / "x.o"), src], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        name = blk.split()[0]
        res[name] = {f: int(re.search(re.escape(f) + r": (\d+)", blk).group(1)) for f in FIELDS}
    return res


def _one(remarks, pattern):
    hits = [n for n in remarks if re.search(pattern, n)]
    assert len(hits) == 1, (pattern, hits)
    return remarks[hits[0]]


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not available")
def test_tail_instantiations_fit_their_register_budgets(remarks):
    # template arguments <LOWER, HAS_BETA, RR, WV, TRI> and <LOWER, HAS_BETA, NW, RR, TRI>
    fused, fused_tri = _one(remarks, r"gemm_fused_kernelILi0ELi0ELi1ELi8ELi0EE"), _one(remarks, r"gemm_fused_kernelILi0ELi0ELi1ELi8ELi1EE")
    rows, rows_tri = _one(remarks, r"gemm_nt_f64_kernelILi0ELi0ELi8ELi1ELi0EE"), _one(remarks, r"gemm_nt_f64_kernelILi0ELi0ELi8ELi1ELi1EE")
    for r in (fused, fused_tri, rows, rows_tri):
        assert r["ScratchSize [bytes/lane]"] == 0, r
    assert fused_tri["VGPRs"] + fused_tri["AGPRs"] <= 256      # 8 waves, one workgroup per CU: 2 waves per SIMD
    assert rows_tri["VGPRs"] + rows_tri["AGPRs"] <= 128        # __launch_bounds__(512, 4): two workgroups per CU
    assert fused_tri["LDS Size [bytes/block]"] == fused["LDS Size [bytes/block]"] == 0      # dynamic: 106 KB, set by the launcher
    assert rows_tri["LDS Size [bytes/block]"] == rows["LDS Size [bytes/block]"] == 73728
