"""Abs-max bounds, the fused inference convolution, the weight-range status and the engine's batch-norm backward on the
host-emulated kernels, each against float64 (tests/range_checks.py)."""
import itertools

import pytest

import range_checks as chk
from helpers import use_emulation_library


@pytest.fixture(scope="module")
def L():
    return use_emulation_library()


@pytest.mark.parametrize("case", chk.FUSED_CASES, ids=str)
def test_fused_conv_every_option(L, case):
    """bias x add x relu x out_absmax (absent / from 0), then the word pre-set above and below the maximum, then inputs far
    outside fp16's range with their in_absmax."""
    for bias, add, relu, absmax0 in itertools.product((True, False), (True, False), (0, 1), (None, 0.0)):
        chk.check_fused_conv(L, "cpu", case, bias=bias, add=add, relu=relu, absmax0=absmax0)
    chk.check_fused_conv(L, "cpu", case, absmax0=1.0e3)     # above the true maximum: unchanged
    chk.check_fused_conv(L, "cpu", case, absmax0=1.0e-3)    # a small positive value: raised to the maximum
    chk.check_fused_conv(L, "cpu", case, relu=1, absmax0=1.0e-3)
    for big in (2.0e5, 1.0e-7):
        chk.check_fused_conv(L, "cpu", case, relu=1, absmax0=0.0, in_scale=big)
        chk.check_fused_conv(L, "cpu", case, add=False, relu=0, absmax0=None, in_scale=big)


PLANTS = [
    ("last_row", chk.FUSED_CASES[0]),      # (a) M = 147: row 146 is the 19th row of the third 64-row tile
    ("last_row", chk.FUSED_CASES[1]),
    ("last_col", chk.FUSED_CASES[1]),      # (b) cout = 136: column 135
    ("neg", chk.FUSED_CASES[0]),           # (c)
    ("neg", chk.FUSED_CASES[3]),
    ("neg_relu", chk.FUSED_CASES[0]),      # (d)
    ("neg_relu", chk.FUSED_CASES[3]),
    ("cancel", chk.FUSED_CASES[0]),        # (e) ragged last M tile in all three
    ("cancel", chk.FUSED_CASES[1]),
    ("cancel", chk.FUSED_CASES[2]),
]


@pytest.mark.parametrize("tile_m", ["64", "128", "256"])
@pytest.mark.parametrize("plant,case", PLANTS, ids=str)
def test_fused_conv_planted_maximum(L, dcn_env, plant, case, tile_m):
    dcn_env(DCN_GEMM_TILE_M=tile_m, DCN_GEMM_SK=0)
    chk.check_fused_conv(L, "cpu", case, relu=0, absmax0=0.0, plant=plant)


# every (tile height, forced stream-K workgroups) at which the shape really is split (dcn_conv_gemm_workspace_f16 > 8, asserted)
STREAM_K = [(c, t, s) for c, t, s in itertools.product(chk.FUSED_CASES, ("64", "128", "256"), ("3", "5", "7"))
            if (c, t, s) not in chk.NOT_STREAM_K]


@pytest.mark.parametrize("case,tile_m,sk", STREAM_K, ids=str)
def test_fused_conv_stream_k_tiles(L, dcn_env, case, tile_m, sk):
    chk.check_fused_conv_stream_k(L, "cpu", dcn_env, case, tile_m, sk)


def test_weight_range_status(L):
    chk.check_weight_range_status(L, "cpu")


def test_eval_fold_pushes_a_legal_weight_out_of_range(L):
    chk.check_eval_fold_weight_range("cpu")


@pytest.mark.parametrize("C,rows,groups", [(32, 147, 1), (32, 264, 2), (8, 147, 1), (64, 520, 2)])
def test_bn_backward_full_vs_float64(L, dcn_env, C, rows, groups):
    chk.check_bn_backward_full_vs_float64(L, "cpu", dcn_env, C, rows, groups)


@pytest.mark.parametrize("arch", ["Resnet18_8s", "Resnet34_8s", "Resnet50_8s"])
def test_activation_slots_vs_oracle(L, arch):
    chk.check_activation_slots("cpu", arch)


@pytest.mark.parametrize("arch", ["Resnet18_8s", "Resnet50_8s"])
def test_activation_slots_forward_pair(L, arch):
    """Two groups: every bound is the maximum over both batches.  64 x 64 images: at 32 x 40 the rows of a batch are no
    multiple of the 64-row tile and forward_pair falls back to two calls."""
    chk.check_activation_slots("cpu", arch, pair=True, size=(64, 64))
