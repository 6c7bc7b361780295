"""The lean batch-norm backward kernels fit beside a resident weight-gradient workgroup: a SIMD has 512 VGPRs per lane, the
8-wavefront workgroups of conv_wgrad_hl_kernel / conv_wgrad_hlrp_kernel put two wavefronts of <= 232 on it, so 48 are left --
and a 256-work-item workgroup (one wavefront per SIMD) that allocates <= 48, no scratch and <= 32 KB of LDS is placed there
while the GEMM runs.  Read from the built library (tools/kernel_resources.py), like tests/test_kernel_resources.py.  CPU only."""
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

LEAN = ("bn_bwd_reduce_lean_kernel", "bn_bwd_finalize_lean_kernel", "bn_bwd_apply_blocked_lean_kernel")


@pytest.fixture(scope="module")
def rows():
    from dcn_hip import build
    import kernel_resources
    return kernel_resources.kernels(build.build_library())


def test_lean_kernels_fit_beside_a_weight_gradient_workgroup(rows):
    lean = [r for r in rows if any(k in r["name"] for k in LEAN) or "bn_bwd_apply_kernel" in r["name"]]
    names = " ".join(r["name"] for r in lean)
    # every instance the launcher can pick: four reduction widths, finalize, the blocked apply with and without the
    # pixel-blocked image, and the plain apply pass (which always fitted)
    assert sum("bn_bwd_reduce_lean_kernel" in r["name"] for r in lean) == 4, names
    assert sum("bn_bwd_apply_blocked_lean_kernel" in r["name"] for r in lean) == 2, names
    assert "bn_bwd_finalize_lean_kernel" in names and "bn_bwd_apply_kernel" in names, names
    for r in lean:
        assert r["vgpr_count"] + r["agpr_count"] <= 48, r
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
        assert r["group_segment_fixed_size"] <= 32768, r


def test_weight_gradient_kernels_leave_48_registers(rows):
    wg = [r for r in rows if "conv_wgrad_hl_kernel" in r["name"] or "conv_wgrad_hlrp_kernel" in r["name"]]
    assert len(wg) == 2, wg
    for r in wg:
        assert r["vgpr_count"] + r["agpr_count"] <= 232, r
