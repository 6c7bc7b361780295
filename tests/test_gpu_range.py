"""-m gpu: abs-max bounds, the fused inference convolution, the weight-range status and the engine's batch-norm backward on the
MI355X, each against float64 on the CPU (tests/range_checks.py; the same functions test_emu_range.py points at the emulation)."""
import itertools

import pytest
import torch

import range_checks as chk
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = use_gfx950_library()
    assert torch.cuda.is_available()
    return lib


@pytest.mark.parametrize("case", chk.FUSED_CASES_GPU, ids=str)
def test_fused_conv_every_option(L, case):
    for bias, add, relu, absmax0 in itertools.product((True, False), (True, False), (0, 1), (None, 0.0)):
        chk.check_fused_conv(L, "cuda", case, bias=bias, add=add, relu=relu, absmax0=absmax0)
    chk.check_fused_conv(L, "cuda", case, absmax0=1.0e3)     # above the true maximum: unchanged
    chk.check_fused_conv(L, "cuda", case, absmax0=1.0e-3)    # a small positive value: raised to the maximum
    chk.check_fused_conv(L, "cuda", case, relu=1, absmax0=1.0e-3)
    for big in (2.0e5, 1.0e-7):
        chk.check_fused_conv(L, "cuda", case, relu=1, absmax0=0.0, in_scale=big)
        chk.check_fused_conv(L, "cuda", case, add=False, relu=0, absmax0=None, in_scale=big)


PLANTS = [
    ("last_row", chk.FUSED_CASES_GPU[0]), ("last_row", chk.FUSED_CASES_GPU[1]), ("last_row", chk.FUSED_CASES_GPU[5]),
    ("last_col", chk.FUSED_CASES_GPU[1]), ("last_col", chk.FUSED_CASES_GPU[5]),
    ("neg", chk.FUSED_CASES_GPU[0]), ("neg", chk.FUSED_CASES_GPU[3]), ("neg", chk.FUSED_CASES_GPU[4]),
    ("neg_relu", chk.FUSED_CASES_GPU[0]), ("neg_relu", chk.FUSED_CASES_GPU[3]), ("neg_relu", chk.FUSED_CASES_GPU[4]),
    ("cancel", chk.FUSED_CASES_GPU[0]), ("cancel", chk.FUSED_CASES_GPU[1]), ("cancel", chk.FUSED_CASES_GPU[2]),
    ("cancel", chk.FUSED_CASES_GPU[5]),    # M = 300: ragged last tile at 64, 128 and 256 rows
]


@pytest.mark.parametrize("tile_m", ["64", "128", "256"])
@pytest.mark.parametrize("plant,case", PLANTS, ids=str)
def test_fused_conv_planted_maximum(L, dcn_env, plant, case, tile_m):
    dcn_env(DCN_GEMM_TILE_M=tile_m, DCN_GEMM_SK=0)
    chk.check_fused_conv(L, "cuda", case, relu=0, absmax0=0.0, plant=plant)


STREAM_K = [(c, t, s) for c, t, s in itertools.product(chk.FUSED_CASES_GPU, ("64", "128", "256"), ("3", "5", "7"))
            if (c, t, s) not in chk.NOT_STREAM_K]


@pytest.mark.parametrize("case,tile_m,sk", STREAM_K, ids=str)
def test_fused_conv_stream_k_tiles(L, dcn_env, case, tile_m, sk):
    chk.check_fused_conv_stream_k(L, "cuda", dcn_env, case, tile_m, sk)


def test_weight_range_status(L):
    chk.check_weight_range_status(L, "cuda")


def test_eval_fold_pushes_a_legal_weight_out_of_range(L):
    chk.check_eval_fold_weight_range("cuda")


@pytest.mark.parametrize("C,rows,groups", [(32, 147, 1), (32, 264, 2), (8, 147, 1), (64, 520, 2), (128, 4800, 2)])
def test_bn_backward_full_vs_float64(L, dcn_env, C, rows, groups):
    chk.check_bn_backward_full_vs_float64(L, "cuda", dcn_env, C, rows, groups)


@pytest.mark.parametrize("arch", ["Resnet18_8s", "Resnet34_8s", "Resnet50_8s"])
def test_activation_slots_vs_oracle(L, arch):
    chk.check_activation_slots("cuda", arch)


@pytest.mark.parametrize("arch", ["Resnet18_8s", "Resnet50_8s"])
def test_activation_slots_forward_pair(L, arch):
    """Two groups: every bound is the maximum over both batches (64 x 64 images: see test_emu_range.py)."""
    chk.check_activation_slots("cuda", arch, pair=True, size=(64, 64))
