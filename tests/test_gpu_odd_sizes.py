"""The whole backbone at image sizes that are not multiples of 8, on a real MI355X through libdcn_hip.so: the checks of
tests/odd_size_checks.py on "cuda" at the small cases of tests/test_emu_odd_sizes.py, and the real networks (base width 64) at
479 x 637 and 239 x 317.  The oracle, float32 and float64, runs live on the host cores: nothing is compared with itself."""
import ctypes

import pytest
import torch

import odd_size_checks as oc
from helpers import rel_err, use_gfx950_library

pytestmark = pytest.mark.gpu
TOL = 1e-4
ODD = ("Resnet18_8s", 8, (2, 37, 53), 3)


@pytest.fixture(scope="module")
def L():
    lib = use_gfx950_library()
    assert torch.cuda.is_available()
    info = lib.library_info()
    assert info["path"].endswith("libdcn_hip.so") and "gfx950" in info["version"] and not info["hostemu"]
    return lib


@pytest.fixture(params=["f16x3", "fp32"])
def conv_mode(request):
    from dcn_hip import backbone
    backbone.set_conv_mode(request.param)
    yield request.param
    backbone.set_conv_mode(None)


# ------------------------------------------------------------------------------------------------ the small cases
@pytest.mark.parametrize("arch,bw,shape,D", oc.TRAIN_CASES)
def test_train_forward_backward_vs_float64_oracle(L, conv_mode, arch, bw, shape, D):
    oc.check_train_vs_float64(arch, bw, shape, D, "cuda")


@pytest.mark.parametrize("arch,bw,shape,D", oc.BOTTLENECK_CASES)
def test_bottleneck_network_train_step(L, conv_mode, arch, bw, shape, D):
    oc.check_train_vs_float64(arch, bw, shape, D, "cuda", gradient_parity=False)


def test_normalized_descriptors_forward_backward(L, conv_mode):
    oc.check_train_vs_float64("Resnet18_8s", 8, (2, 37, 53), 4, "cuda", normalize=True)


@pytest.mark.parametrize("arch,bw,shape,grouped", [("Resnet18_8s", 8, (2, 29, 127), True), ("Resnet18_8s", 8, (2, 37, 53), False)])
def test_grouped_pair_equals_two_forward_calls(L, conv_mode, arch, bw, shape, grouped):
    oc.check_pair_equals_two_calls(arch, bw, shape, "cuda", grouped, fwd_tol=2e-5, grad_tol=1e-4, buffer_tol=1e-5)


@pytest.mark.parametrize("arch,bw,shape,D", oc.TRAIN_CASES[:2] + oc.BOTTLENECK_CASES
                         + [("Resnet18_8s", 8, s, 3) for s in oc.TINY_SHAPES] + [("Resnet50_8s", 8, s, 5) for s in oc.TINY_SHAPES])
def test_eval_mode_vs_float64_oracle(L, conv_mode, arch, bw, shape, D):
    oc.check_eval_vs_float64(arch, bw, shape, D, "cuda")


@pytest.mark.parametrize("arch,bw,D", [("Resnet18_8s", 8, 3), ("Resnet50_8s", 8, 5)])
@pytest.mark.parametrize("shape", oc.TINY_SHAPES)
def test_train_mode_on_tiny_maps_is_finite(L, conv_mode, arch, bw, D, shape):
    oc.check_tiny_train_forward(arch, bw, shape, D, "cuda")


@pytest.mark.parametrize("arch,bw,shape,D", [ODD, ("Resnet50_8s", 8, (2, 45, 61), 5)])
def test_two_identical_train_steps_are_bit_identical(L, conv_mode, arch, bw, shape, D):
    oc.check_bit_reproducible(arch, bw, shape, D, "cuda")


def test_forward_backward_with_stream_k_forced(L, conv_mode, dcn_env):
    dcn_env(DCN_GEMM_SK=5)
    arch, bw, (N, H, W), D = ODD
    lib = L.get()
    ws = lib.dcn_conv_gemm_workspace if conv_mode == "fp32" else lib.dcn_conv_gemm_workspace_f16
    _, _, (hl, wl) = oc.low_res(H, W)
    for c, dil in ((2 * bw, 1), (4 * bw, 2), (8 * bw, 4)):
        d = L.ConvDesc(N, hl, wl, c, hl, wl, c, 3, 3, 1, dil, dil, c, 0)
        assert ws(ctypes.byref(d), 0) > 8 and ws(ctypes.byref(d), 1) > 8, "stream-K is not exercised at this shape"
    oc.check_train_vs_float64(arch, bw, (N, H, W), D, "cuda")


@pytest.mark.parametrize("arch,groups", [("Resnet18_8s", 1), ("Resnet50_8s", 1), ("Resnet18_8s", 2)])
def test_bn_backward_reduction_fused_into_dgrad(L, conv_mode, dcn_env, arch, groups):
    oc.check_bn_backward_reduction_fused("cuda", dcn_env, arch, groups, conv_mode, (2, 29, 127) if groups == 2 else (2, 37, 53))


def test_evaluate_network_on_the_37x53_store(L, conv_mode):
    from test_emu_evaluate import _tiny_dcn
    oc.check_evaluate_on_store("cuda", 37, 53, _tiny_dcn)


@pytest.mark.parametrize("rows", [160, 192, 256, 320])
def test_wide_layers_through_the_hl32_path(L, dcn_env, rows):
    from dcn_hip import backbone
    backbone.set_conv_mode("f16x3")
    try:
        oc.check_hl32_at_odd_size(L, "cuda", dcn_env, "Resnet18_8s", 32, (1, 69, 93), rows)
    finally:
        backbone.set_conv_mode(None)


# ------------------------------------------------------------------------------------------------ real width
def _real_width_train_step(arch, shape, D):
    """One train step of the real network on the GPU against the live oracle, float32 and float64, on the host.  Tolerances
    of tests/test_gpu_parity.py::test_config1_full_size_vs_live_oracle: descriptors within 1e-4 of the float32 oracle's;
    gradients NOT float32 against float32 tensor by tensor but in the distribution over the tensors -- the relative L2
    distance from the float32 oracle within 2.5 x (r.m.s.) / 3 x (worst tensor) the float32 oracle's own from float64, here
    from the live float64 run instead of a fixture.
    The conditioning assertion holds for the forward pass only.  At base width 64 the float32 oracle's gradients are
    6.3e-2 (Resnet34_8s 2 x 479 x 637), 5.6e-2 (2 x 239 x 317), 5.3e-2 (4 x 119 x 157), 5.5e-2 (base width 32, 2 x 239 x 317)
    off float64 in the largest element, 108 of 110 tensors above 1e-4, at every size tried (host measurements): per-tensor
    gradient parity cannot be claimed at real width, which is why the full-size tests use the distribution."""
    N, H, W = shape
    o, o64, yo, y64, init = oc.cached_oracle_train_step(arch, D, 64, shape)   # (once for both arithmetics)
    m = oc.product_module(arch, D, 64, "cuda", init)
    x, gy = oc.inputs(N, H, W, D)
    cond = rel_err(yo, y64)
    assert cond < oc.CONDITION, "ill-conditioned case, float32 oracle forward %.2e off float64" % cond
    m.train()
    y = m(x.cuda())
    oc.assert_output_layout(y, N, D, H, W)
    assert oc.status_clear(m)
    e32, e64 = rel_err(y.detach().cpu(), yo), rel_err(y.detach().cpu(), y64)
    print("odd-size %s bw64 %dx%dx%d: forward engine vs float64 %.2e / fp32 oracle %.2e; engine vs fp32 oracle %.2e"
          % (arch, N, H, W, e64, cond, e32))
    assert e32 < TOL and e64 < TOL, (e32, e64)
    (y * gy.cuda()).sum().backward()
    rel, ref, rel64 = [], [], []
    for p, po, p6 in zip(m.parameters(), o.parameters(), o64.parameters()):
        n6 = float(p6.grad.norm())
        g = p.grad.cpu()
        assert bool(torch.isfinite(g).all())
        rel.append(float((g - po.grad).norm() / po.grad.norm()))
        ref.append(float((po.grad.double() - p6.grad).norm()) / n6)
        rel64.append(float((g.double() - p6.grad).norm()) / n6)
    rms = lambda v: float(torch.tensor(v).square().mean().sqrt())
    print("odd-size %s bw64 %dx%dx%d: gradients, relative L2 over the tensors: engine vs fp32 oracle r.m.s. %.2e worst %.2e; "
          "engine vs float64 r.m.s. %.2e worst %.2e; fp32 oracle vs float64 r.m.s. %.2e worst %.2e"
          % (arch, N, H, W, rms(rel), max(rel), rms(rel64), max(rel64), rms(ref), max(ref)))
    assert rms(rel) <= 2.5 * rms(ref), (rms(rel), rms(ref))
    assert max(rel) <= 3.0 * max(ref), (max(rel), max(ref))
    for b, bo in zip(m.buffers(), o.buffers()):
        b = b.float().cpu()
        assert rel_err(b, bo.float()) < 1e-4 or float((b - bo.float()).abs().max()) < 1e-5
    torch.cuda.empty_cache()


def test_real_width_resnet34_479x637_vs_live_oracle(L, conv_mode):
    _real_width_train_step("Resnet34_8s", (2, 479, 637), 3)


def test_real_width_resnet50_239x317_vs_live_oracle(L, conv_mode):
    """The bottleneck network at real width, held to the standard of
    tests/test_gpu_parity.py::test_resnet50_8s_forward_backward_vs_oracle (odd_size_checks.BOTTLENECK_CASES says why)."""
    oc.check_train_vs_float64("Resnet50_8s", 64, (1, 239, 317), 3, "cuda", gradient_parity=False)
    torch.cuda.empty_cache()


def test_real_width_grouped_pair_479x637(L, conv_mode):
    """Four images per batch: 4 x 240 x 319 rows behind the stem are a multiple of 64, so the grouped plan exists."""
    oc.check_pair_equals_two_calls("Resnet34_8s", 64, (4, 479, 637), "cuda", True, oracle_forward=False, fwd_tol=5e-5, grad_tol=TOL,
                                   buffer_tol=1e-5, real_width=True)
    torch.cuda.empty_cache()


def test_real_width_eval_mode_479x637(L, conv_mode):
    oc.check_eval_vs_float64("Resnet34_8s", 64, (2, 479, 637), 3, "cuda")
    torch.cuda.empty_cache()
