"""The deep batch-norm backward instances (DCN_BN_BWD_LEAN_DEPTH) on the MI355X: same bits as the full-width and the one-row lean
kernels, and the same launch twice gives the same bits (tests/bn_bwd_deep_checks.py).  The small shapes of
test_emu_bn_bwd_deep.py; 16 421 rows (129 chunks of 128, the last holding 37) and two groups of 8 236 (64-row chunks, the last
holding 44) at C = 64 / 128 / 512 -- many workgroups of the apply pass that take the straight-line path, and the guarded one at the
end; and 131 073 rows at C = 64: an EMPTY last chunk, and the only shape here at which the apply pass's grid-stride loop runs a
second round for some workgroups (32 769 quads x 16 > 2048 x 256)."""
import pytest
import torch

import bn_bwd_deep_checks as chk
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = use_gfx950_library()
    assert torch.cuda.is_available()
    return lib


@pytest.mark.parametrize("rows,groups", [(234, 1), (18, 1), (88, 2), (5, 1)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_deep_kernels_same_bits(L, dcn_env, C, rows, groups):
    chk.check_three_settings(L, "cuda", dcn_env, C, rows, groups, repeat=True)


@pytest.mark.parametrize("rows,groups", [(16421, 1), (2 * 8236, 2)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_deep_kernels_same_bits_many_workgroups(L, dcn_env, C, rows, groups):
    chk.check_three_settings(L, "cuda", dcn_env, C, rows, groups, only=chk.FEW)


def test_second_round_of_the_apply_loop_and_an_empty_chunk(L, dcn_env):
    chk.check_three_settings(L, "cuda", dcn_env, 64, 131073, 1, only=(1, 9, 13, 22))
