"""DCN_BN_BWD_LEAN = 1 against 0 on the MI355X: the lean instances of the batch-norm backward kernels compute the same bits as
the full-width ones, and the same launch twice gives the same bits (tests/bn_bwd_lean_checks.py).  Shapes: C = 64 / 128 / 512
(the 16-quad, the 32-quad and the capped wider-quad reduction); one group of 2 x 37 x 53 rows (no multiple of 4, 123 chunks),
two groups of 1036 rows (a multiple of 4, not of the 32-row chunk), and 18 rows (less than one chunk)."""
import pytest
import torch

import bn_bwd_lean_checks as chk
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = use_gfx950_library()
    assert torch.cuda.is_available()
    return lib


@pytest.mark.parametrize("rows,groups", [(2 * 37 * 53, 1), (2072, 2), (18, 1)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_lean_kernels_same_bits(L, dcn_env, C, rows, groups):
    chk.check_lean_equals_full(L, "cuda", dcn_env, C, rows, groups, repeat=True)


def test_empty_chunks_behind_the_chunk_cap(L, dcn_env):
    """131 073 rows: more than 1024 chunks of 128 rows, so the chunk count is capped and a chunk holds 129 rows -- 1023 x 129 is
    past the end, the last chunk is EMPTY (its first row lies behind the group).  The lean reduction walks a chunk by 32-bit
    offsets from the chunk's first row and must not turn that negative length into a long one."""
    chk.check_lean_equals_full(L, "cuda", dcn_env, 64, 131073, 1, only=(1, 9, 22))
