"""The deep batch-norm backward apply instances (DCN_BN_BWD_LEAN_DEPTH) on the host-emulated kernels: same bits as the full-width
and the one-row lean kernels (tests/bn_bwd_deep_checks.py).  Shapes at which a schedule of several rows can go wrong, C = 64 /
128 / 512 each: 234 rows (ragged last pixel quad; three straight-line workgroups and a guarded one at C = 64), 18 rows, two groups
of 44 (a workgroup that straddles the groups), 5 rows (fewer than the depth; rows 5-7 of the second quad lie past the end), and
at C = 64 16 421 rows (129 chunks of 128, the last holding 37)."""
import pytest
import torch

import bn_bwd_deep_checks as chk
from helpers import use_emulation_library


@pytest.fixture(scope="module")
def L():
    return use_emulation_library()


@pytest.mark.parametrize("rows,groups", [(234, 1), (18, 1), (88, 2), (5, 1)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_deep_kernels_same_bits(L, dcn_env, C, rows, groups):
    chk.check_three_settings(L, "cpu", dcn_env, C, rows, groups)


def test_deep_kernels_same_bits_every_pipeline_remainder(L, dcn_env):
    chk.check_three_settings(L, "cpu", dcn_env, 64, 16421, 1, only=chk.FEW)


def test_depth_is_reread(L, dcn_env):
    """DCN_BN_BWD_LEAN_DEPTH is read again by dcn_reload_env: depth 1, 2 and the default in one process, the same bytes."""
    inp = chk.make_inputs(128, 88, 2, seed=5)
    args = (L, "cpu", inp, 128, 88, 2, "hl_blocked_keep", "bytes", True, True)
    dcn_env(DCN_BN_BWD_LEAN=1)
    default = chk.run_once(*args)
    for depth in (1, 2, 3):
        dcn_env(DCN_BN_BWD_LEAN=1, DCN_BN_BWD_LEAN_DEPTH=depth)
        got = chk.run_once(*args)
        assert got.keys() == default.keys()
        for k in got:
            assert torch.equal(got[k], default[k]), (depth, k)
        for k in ("dgamma", "dbeta", "k123"):
            assert torch.isfinite(got[k].view(torch.float32)).all() and not (got[k] == 0x5A).all(), (depth, k)
