"""The deep instances of the batch-norm backward apply pass (DCN_BN_BWD_LEAN_DEPTH) keep the budget of the lean ones (test_bn_bwd_lean_resources.py):
<= 48 VGPRs + AGPRs, no scratch, no spills and <= 32 KB of LDS, so that a 256-work-item workgroup of them is placed on a CU beside
a resident weight-gradient workgroup.  Read from the built library (tools/kernel_resources.py).  CPU only."""
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def rows():
    from dcn_hip import build
    import kernel_resources
    return kernel_resources.kernels(build.build_library())


def test_deep_kernels_fit_beside_a_weight_gradient_workgroup(rows):
    deep = [r for r in rows if "bn_bwd_apply_blocked_deep_kernel" in r["name"]]
    names = " ".join(r["name"] for r in deep)
    # every instance the launcher can pick: without the pixel-blocked image at two and at three rows in flight, with it at two
    assert len(deep) == 3, names
    for r in deep:
        assert r["vgpr_count"] + r["agpr_count"] <= 48, r
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
        assert r["group_segment_fixed_size"] <= 32768, r
