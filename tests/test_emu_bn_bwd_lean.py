"""DCN_BN_BWD_LEAN = 1 against 0 on the host-emulated kernels: the lean instances of the batch-norm backward kernels compute the
same bits (tests/bn_bwd_lean_checks.py).  Shapes: the smallest that take every path -- C = 64 / 128 / 512 (the 16-quad, the
32-quad and the capped wider-quad reduction), one group with a row count that is no multiple of 4 (2 x 9 x 13), two groups of
44 rows (a multiple of 4, not of the 32-row chunk), and fewer rows than one chunk."""
import pytest

import bn_bwd_lean_checks as chk
from helpers import use_emulation_library


@pytest.fixture(scope="module")
def L():
    return use_emulation_library()


@pytest.mark.parametrize("rows,groups", [(2 * 9 * 13, 1), (88, 2), (18, 1)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_lean_kernels_same_bits(L, dcn_env, C, rows, groups):
    chk.check_lean_equals_full(L, "cpu", dcn_env, C, rows, groups)


def test_switches_are_reread(L, dcn_env):
    """DCN_BN_BWD_LEAN_MASK narrows the switch to single kernels; every mask gives the same bits as none."""
    inp = chk.make_inputs(128, 88, 2, seed=5)
    dcn_env(DCN_BN_BWD_LEAN=0)
    want = chk.run_once(L, "cpu", inp, 128, 88, 2, "hl_blocked_keep", "bytes", True, True)
    for mask in (1, 2, 4, 7):
        dcn_env(DCN_BN_BWD_LEAN=1, DCN_BN_BWD_LEAN_MASK=mask)
        got = chk.run_once(L, "cpu", inp, 128, 88, 2, "hl_blocked_keep", "bytes", True, True)
        for k in want:
            assert (want[k] == got[k]).all(), (mask, k)
