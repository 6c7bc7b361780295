"""Max pool, upsample, normalisation backward, the layout kernels and the fc.bias column sums on the host-emulated kernels, each
against float64 with ties and planted extremes (tests/resample_checks.py; test_gpu_resample.py runs the same on the MI355X)."""
import pytest

import resample_checks as chk
from helpers import use_emulation_library

DEV = "cpu"


@pytest.fixture(scope="module")
def L():
    return use_emulation_library()


@pytest.mark.parametrize("kind", chk.POOL_KINDS)
@pytest.mark.parametrize("shape", chk.POOL_SHAPES, ids=str)
def test_maxpool_exact(L, shape, kind):
    chk.check_maxpool_exact(L, DEV, shape, kind)


def test_new_entry_points_reject_bad_arguments(L):
    chk.check_pool_argument_checks(L, DEV)


@pytest.mark.parametrize("shape", chk.STEM_SHAPES, ids=str)
def test_stem_pool_fused_equals_apply_then_pool(L, shape):
    chk.check_stem_pool_fused(L, DEV, shape)


@pytest.mark.parametrize("shape", chk.STEM_SHAPES, ids=str)
def test_stem_tail_chain_vs_float64_autograd(L, dcn_env, shape):
    chk.check_stem_chain(L, DEV, dcn_env, shape)


@pytest.mark.parametrize("d", chk.UPSAMPLE_DIMS)
@pytest.mark.parametrize("sizes", chk.UPSAMPLE_EXACT, ids=str)
def test_upsample_exact(L, sizes, d):
    chk.check_upsample_exact(L, DEV, sizes, d)


@pytest.mark.parametrize("shape", chk.UPSAMPLE_INEXACT, ids=str)
def test_upsample_inexact(L, shape):
    chk.check_upsample_inexact(L, DEV, shape)


@pytest.mark.parametrize("shape", [(2, 4, 5, 3, 32, 40), (4, 3, 3, 16, 24, 24), (4, 6, 8, 5, 41, 59)], ids=str)
def test_upsample_backward_two_tensors(L, shape):
    chk.check_upsample_backward_two_tensors(L, DEV, shape)


@pytest.mark.parametrize("shape", [(2, 4, 5, 3, 32, 40), (1, 6, 8, 5, 41, 59)], ids=str)
def test_upsample_backward_absmax(L, shape):
    chk.check_upsample_backward_absmax(L, DEV, shape)


@pytest.mark.parametrize("d", chk.UPSAMPLE_DIMS)
@pytest.mark.parametrize("shape", chk.NORMALIZE_SHAPES, ids=str)
def test_normalize_backward_vs_float64(L, shape, d):
    chk.check_normalize_backward(L, DEV, shape, d)


@pytest.mark.parametrize("shape", chk.NORMALIZE_SHAPES, ids=str)
def test_normalize_backward_one_channel(L, shape):
    chk.check_normalize_backward_one_channel(L, DEV, shape)


def test_normalize_zero_cell_is_nan_where_float64_is(L):
    chk.check_normalize_zero_cell(L, DEV)


@pytest.mark.parametrize("size", chk.IMAGE_SIZES, ids=str)
def test_image_to_nhwc4(L, size):
    chk.check_image_to_nhwc4(L, DEV, size)


@pytest.mark.parametrize("rows", [1, 49 * 8, 257])
def test_pad_channels_round_trip(L, rows):
    chk.check_pad_channels_round_trip(L, DEV, rows)


@pytest.mark.parametrize("d,ld", chk.COLSUM_DIMS)
def test_pad_rows(L, d, ld):
    chk.check_pad_rows(L, DEV, d, ld)


@pytest.mark.parametrize("d,ld", chk.COLSUM_DIMS)
@pytest.mark.parametrize("rows", chk.COLSUM_ROWS)
def test_column_sums(L, rows, d, ld):
    chk.check_column_sums(L, DEV, rows, d, ld)
