"""The whole backbone engine at image sizes that are not multiples of 8 (plan -> forward -> backward through the C ABI,
host-emulated), in both convolution arithmetics: tests/odd_size_checks.py explains the yard-stick and why gradient parity is
only claimed on well-conditioned cases.  Every other backbone test runs at sizes that divide by 8; here the floor / ceil sizes
of the stem, the max pool and layer2, ragged M tiles and batch-norm partial-sum tiles, ragged ReLU mask bytes and a
non-integer upsample ratio meet in one plan."""
import ctypes

import pytest

import odd_size_checks as oc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.fixture(autouse=True, params=["fp32", "f16x3"])
def conv_mode(request):
    """Every test of this file runs in both convolution arithmetics; the tolerances are the same (include/dcn_hip.h)."""
    from dcn_hip import backbone
    backbone.set_conv_mode(request.param)
    yield request.param
    backbone.set_conv_mode(None)


ODD = ("Resnet18_8s", 8, (2, 37, 53), 3)     # the size of the data pipeline's odd fixtures (augment, merge, samples, evaluation)
# Sizes that are no multiple of 8 and still admit the grouped plan (every batch-normed tensor: a multiple of 64 rows per
# group): W = 127 gives maps 64, 32 and 16 wide behind the stem, the max pool and layer2
PAIR_CASES = [("Resnet18_8s", 8, (2, 29, 127), True), ("Resnet34_8s", 8, (1, 61, 127), True), ("Resnet18_8s", 8, (2, 37, 53), False)]


def test_the_cases_are_odd():
    for _, _, (_, H, W), _ in oc.TRAIN_CASES + oc.BOTTLENECK_CASES:
        assert H % 8 or W % 8
    assert any(H % 8 and not W % 8 for _, _, (_, H, W), _ in oc.TRAIN_CASES)
    assert any(W % 8 and not H % 8 for _, _, (_, H, W), _ in oc.TRAIN_CASES)
    assert oc.low_res(37, 53) == ((19, 27), (10, 14), (5, 7)) and oc.low_res(8, 8)[2] == (1, 1) and oc.low_res(29, 8)[2] == (4, 1)


@pytest.mark.parametrize("arch,bw,shape,D", oc.TRAIN_CASES)
def test_train_forward_backward_vs_float64_oracle(arch, bw, shape, D):
    oc.check_train_vs_float64(arch, bw, shape, D, "cpu")


@pytest.mark.parametrize("arch,bw,shape,D", oc.BOTTLENECK_CASES)
def test_bottleneck_network_train_step(arch, bw, shape, D):
    """Resnet50_8s: forward parity; gradients in the distribution over the tensors only (odd_size_checks.BOTTLENECK_CASES:
    the float32 oracle's own gradients are 1.1e-1 off float64 at this case, so the conditioning assertion cannot hold)."""
    oc.check_train_vs_float64(arch, bw, shape, D, "cpu", gradient_parity=False)


def test_the_conditioning_assertion_refuses_an_ill_conditioned_case():
    """2 x 29 x 8: a 4 x 1 low-resolution map.  The assertion that guards the gradient-parity cases must fire on it."""
    arch, bw, (N, H, W), D = "Resnet50_8s", 8, (2, 29, 8), 5
    _, o = oc.make_pair(arch, D, bw, "cpu")
    x, gy = oc.inputs(N, H, W, D)
    yo, y64, o64 = oc.oracle_train_step(o, x, gy)
    with pytest.raises(AssertionError, match="ill-conditioned case"):
        oc.assert_well_conditioned(o, o64, yo, y64, "4 x 1 map")


@pytest.mark.parametrize("arch,bw,shape,grouped", PAIR_CASES)
def test_grouped_pair_equals_two_forward_calls(arch, bw, shape, grouped):
    oc.check_pair_equals_two_calls(arch, bw, shape, "cpu", grouped)


def test_forward_backward_with_stream_k_forced(dcn_env, conv_mode):
    """Every gather-GEMM launch through the stream-K split + fix-up path, on the ragged tiles of 2 x 37 x 53."""
    from dcn_hip import _lib as L
    dcn_env(DCN_GEMM_SK=5)
    arch, bw, (N, H, W), D = ODD
    lib = L.get()
    ws = lib.dcn_conv_gemm_workspace if conv_mode == "fp32" else lib.dcn_conv_gemm_workspace_f16
    (h2, w2), (hp, wp), (hl, wl) = oc.low_res(H, W)
    # the 3 x 3 convolutions of layers 2 - 4, forward and dgrad, split their K loop (layer1's K = 72 is a single stage of the
    # split-fp16 kernel: nothing to split there)
    for c, dil in ((2 * bw, 1), (4 * bw, 2), (8 * bw, 4)):
        d = L.ConvDesc(N, hl, wl, c, hl, wl, c, 3, 3, 1, dil, dil, c, 0)
        assert ws(ctypes.byref(d), 0) > 8 and ws(ctypes.byref(d), 1) > 8, "stream-K is not exercised at this shape"
    oc.check_train_vs_float64(arch, bw, (N, H, W), D, "cpu")


@pytest.mark.parametrize("arch,groups", [("Resnet18_8s", 1), ("Resnet50_8s", 1), ("Resnet18_8s", 2)])
def test_bn_backward_reduction_fused_into_dgrad(arch, groups, conv_mode, dcn_env):
    oc.check_bn_backward_reduction_fused("cpu", dcn_env, arch, groups, conv_mode, (2, 29, 127) if groups == 2 else (2, 37, 53))


class TestHl32:
    """The hl32 path belongs to the split-fp16 arithmetic: these tests run in it alone (the class's own conv_mode)."""

    @pytest.fixture(autouse=True)
    def conv_mode(self):
        from dcn_hip import backbone
        backbone.set_conv_mode("f16x3")
        yield "f16x3"
        backbone.set_conv_mode(None)

    @pytest.mark.parametrize("rows", [160, 192, 256, 320])
    def test_wide_layers_through_the_hl32_path(self, rows, dcn_env):
        """1 x 69 x 93, base width 32: maps of 18 x 24 = 432 rows (layer1: two or three tiles, the last one ragged) and
        9 x 12 = 108 rows (layers 2 - 4: less than one tile) -- a multiple of none of the four tile heights of the hl32
        kernels, each forced in turn."""
        from dcn_hip import _lib as L
        oc.check_hl32_at_odd_size(L, "cpu", dcn_env, "Resnet18_8s", 32, (1, 69, 93), rows)


def test_normalized_descriptors_forward_backward():
    """normalize=True: res / ||res||_2 over D fused into the upsample kernel, and backward through it."""
    oc.check_train_vs_float64("Resnet18_8s", 8, (2, 37, 53), 4, "cpu", normalize=True)


@pytest.mark.parametrize("arch,bw,shape,D", oc.TRAIN_CASES + oc.BOTTLENECK_CASES
                         + [("Resnet18_8s", 8, s, 3) for s in oc.TINY_SHAPES] + [("Resnet50_8s", 8, s, 5) for s in oc.TINY_SHAPES])
def test_eval_mode_vs_float64_oracle(arch, bw, shape, D):
    oc.check_eval_vs_float64(arch, bw, shape, D, "cpu")


@pytest.mark.parametrize("arch,bw,D", [("Resnet18_8s", 8, 3), ("Resnet50_8s", 8, 5)])
@pytest.mark.parametrize("shape", oc.TINY_SHAPES)
def test_train_mode_on_tiny_maps_is_finite(arch, bw, D, shape):
    oc.check_tiny_train_forward(arch, bw, shape, D, "cpu")


@pytest.mark.parametrize("arch,bw,shape,D", [ODD, ("Resnet50_8s", 8, (2, 45, 61), 5)])
def test_two_identical_train_steps_are_bit_identical(arch, bw, shape, D):
    oc.check_bit_reproducible(arch, bw, shape, D, "cpu")


def test_evaluate_network_on_the_37x53_store(conv_mode):
    """The one place where the data pipeline's odd-size fixtures meet the network: dcn_hip.evaluate on a 37 x 53 frame
    store with the tiny network of tests/test_emu_evaluate.py."""
    from test_emu_evaluate import _tiny_dcn
    oc.check_evaluate_on_store("cpu", 37, 53, _tiny_dcn)
