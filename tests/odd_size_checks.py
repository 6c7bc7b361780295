"""Whole-network checks at image sizes that are not multiples of 8, shared by the CPU (host-emulated) and the -m gpu suites
(not a test module): the same calls on `device` ("cpu" with the emulation library loaded, "cuda" with libdcn_hip.so).

The engine accepts every image of at least 8 x 8 and upsamples back to the input size, so between the image and the
descriptor map sit the floor / ceil sizes of the stem (ceil(H / 2)), the max pool (ceil of that / 2) and the stride-2 layer2,
row counts N * h * w that are a multiple of no tile height, ragged 4-per-byte ReLU masks and a non-integer upsample ratio.

Yard-stick, as in tests/test_emu_backbone.py: a float64 copy of the oracle.  The engine must be as close to it as the
float32 oracle is: forward 3 * err(fp32 oracle) + 1e-5, every parameter gradient 3 * err(fp32 oracle) + 2e-5.  Train-mode
gradient parity is only claimed where the float32 oracle itself is well conditioned (assert_well_conditioned): on a 2 x 2 or
4 x 1 low-resolution map the batch norms normalise over a handful of rows and float32 PyTorch is 15 % off its float64 self
(Resnet50_8s, base width 8, 2 x 29 x 8: 0.15) -- a parity test there fails without any kernel being wrong.  Such sizes are
checked in eval mode (no batch statistics) and for finite train-mode output only."""
import copy
import ctypes
import warnings

import numpy as np
import torch

from helpers import rel_err

FWD_FLOOR, GRAD_FLOOR = 1e-5, 2e-5
CONDITION = 1e-4          # the float32 oracle against its float64 copy: forward and every parameter gradient below this

# (arch, base width, (N, H, W), D): train forward + backward against the float64 oracle.  Behind each case: the float32
# oracle against float64 as measured on the host, forward / worst parameter gradient -- all more than 10 x below CONDITION.
TRAIN_CASES = [
    ("Resnet18_8s", 8, (2, 37, 53), 3),      # 2.0e-6 / 3.8e-6
    ("Resnet34_8s", 8, (1, 33, 47), 4),      # 4.3e-6 / 8.5e-6
    ("Resnet34_8s", 16, (2, 41, 35), 16),    # 4.8e-6 / 9.3e-6
    ("Resnet34_8s", 8, (2, 45, 61), 5),      # 4.7e-6 / 8.1e-6   (stands in for the bottleneck network at this size: see below)
    ("Resnet18_8s", 8, (2, 43, 48), 3),      # 2.1e-6 / 4.3e-6   H odd, W a multiple of 8
    ("Resnet18_8s", 8, (2, 40, 51), 3),      # 3.1e-6 / 4.2e-6   H a multiple of 8, W odd
]
# Resnet50_8s, base width 8, 2 x 45 x 61, D = 5 FAILS the conditioning assertion: forward 5.7e-5, but the float32 oracle's
# gradient of layer4.0.downsample.0.weight is 1.1e-1 off float64 and 141 of its 161 parameter gradients are more than 1e-4 off.
# No size, width or seed makes the train-mode bottleneck network well conditioned -- worst gradient of the float32 oracle:
# 2 x 32 x 40 5.7e-3, 2 x 93 x 125 8.2e-2, 4 x 77 x 93 7.7e-2, 2 x 141 x 189 1.1e-1, base width 16 at 2 x 77 x 93 8.4e-2,
# base width 64 at 1 x 45 x 61 1.4e-1, input seeds 1 .. 5 at 2 x 45 x 61 1.2e-2 .. 2.3e-1, weight seeds 1 .. 3 3.8e-2 .. 1.5e-1
# (48 train-mode batch norms in a row amplify float32 round-off) -- so per-tensor gradient parity is not claimed for it.  What
# is: forward parity (well conditioned), and gradients as accurate as the float32 oracle's in the distribution over the
# tensors (the standard tests/test_gpu_parity.py::test_resnet50_8s_forward_backward_vs_oracle holds this network to).
BOTTLENECK_CASES = [
    ("Resnet50_8s", 8, (2, 45, 61), 5),
]
# low-resolution maps of 1 x 1, 2 x 2, 4 x 1 and 1 x 8: eval-mode parity and finite train-mode output only (two images: a
# train-mode batch norm needs more than one value per channel)
TINY_SHAPES = [(2, 8, 8), (2, 9, 15), (2, 29, 8), (2, 8, 64)]


def low_res(H, W):
    """Sizes behind the stem (7 x 7 / 2, pad 3), the max pool (3 x 3 / 2, pad 1) and layer2 (3 x 3 / 2, pad 1)."""
    half = lambda v: (v - 1) // 2 + 1
    return (half(H), half(W)), (half(half(H)), half(half(W))), (half(half(half(H))), half(half(half(W))))


def make_pair(arch, D, bw, device, seed=0):
    """(product module on `device`, float32 oracle on the host) with the same seeded weights."""
    from oracle import resnet_dilated_oracle as orc
    from pytorch_segmentation_detection.models import resnet_dilated as prod
    o = orc.build(arch, D, seed=seed, base_width=bw)
    m = getattr(prod, arch)(num_classes=D, base_width=bw)
    m.load_state_dict(o.state_dict(), strict=True)
    return m.to(device), o


def inputs(N, H, W, D, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 3, H, W, generator=g), torch.randn(N, D, H, W, generator=g)


def status_clear(m):
    amax, status = m.last_forward_status()
    return int(status.cpu()[0] if status.dim() else status) == 0 and bool(torch.isfinite(amax).all())


def assert_output_layout(y, N, D, H, W):
    assert tuple(y.shape) == (N, D, H, W), tuple(y.shape)
    assert y.is_contiguous(memory_format=torch.channels_last)


def oracle_train_step(o, x, gy, normalize=False):
    """-> (y32, y64, o64) of the float32 oracle and its float64 copy, both differentiated with the cotangent gy."""
    o64 = copy.deepcopy(o).double()
    o.train(); o64.train()
    yo, y64 = o(x), o64(x.double())
    if normalize:
        yo, y64 = yo / torch.norm(yo, 2, 1, keepdim=True), y64 / torch.norm(y64, 2, 1, keepdim=True)
    (yo * gy).sum().backward(); (y64 * gy.double()).sum().backward()
    return yo.detach(), y64.detach(), o64


_ORACLE_STEPS = {}   # the host oracle's runs depend on the case only, not on the engine's arithmetic or device: made once per process


def product_module(arch, D, bw, device, state_dict):
    from pytorch_segmentation_detection.models import resnet_dilated as prod
    m = getattr(prod, arch)(num_classes=D, base_width=bw)
    m.load_state_dict(state_dict, strict=True)
    return m.to(device)


def cached_oracle_train_step(arch, D, bw, shape, seed=11, normalize=False):
    """-> (o, o64, y32, y64, initial state dict): oracle_train_step of the seeded oracle on inputs(*shape, D, seed)."""
    key = ("train", arch, D, bw, tuple(shape), seed, normalize)
    if key not in _ORACLE_STEPS:
        from oracle import resnet_dilated_oracle as orc
        o = orc.build(arch, D, seed=0, base_width=bw)
        init = copy.deepcopy(o.state_dict())
        x, gy = inputs(*shape, D, seed)
        yo, y64, o64 = oracle_train_step(o, x, gy, normalize)
        _ORACLE_STEPS[key] = (o, o64, yo, y64, init)
    return _ORACLE_STEPS[key]


def assert_well_conditioned(o, o64, yo, y64, what):
    """A condition on the INPUT of a gradient-parity case, not a measurement of the engine: the float32 oracle is within
    CONDITION of its float64 copy, forward and every parameter gradient -- so that the 3 * err(fp32 oracle) term of the
    tolerances cannot swallow a real defect.  An ill-conditioned shape fails here, loudly, whatever the engine does."""
    e = rel_err(yo, y64)
    assert e < CONDITION, "%s: ill-conditioned case, float32 oracle forward %.2e off float64" % (what, e)
    worst = max(((rel_err(po.grad, p6.grad), k) for (k, po), p6 in zip(o.named_parameters(), o64.parameters())))
    assert worst[0] < CONDITION, "%s: ill-conditioned case, float32 oracle gradient of %s %.2e off float64" % ((what,) + worst[::-1])
    return e, worst[0]


def check_train_vs_float64(arch, bw, shape, D, device, normalize=False, seed=11, gradient_parity=True):
    """Train-mode forward + backward of the engine against the float64 oracle (the tolerances of
    test_forward_backward_vs_oracle), behind the conditioning assertion.  gradient_parity=False (BOTTLENECK_CASES): only the
    forward pass must be well conditioned, and the gradients are held to parity_common.assert_as_accurate_as_float32.
    -> the measured figures."""
    N, H, W = shape
    what = "%s bw%d %dx%dx%d D%d%s" % (arch, bw, N, H, W, D, " normalized" if normalize else "")
    o, o64, yo, y64, init = cached_oracle_train_step(arch, D, bw, shape, seed, normalize)
    m = product_module(arch, D, bw, device, init)
    x, gy = inputs(N, H, W, D, seed)
    if gradient_parity:
        cond_f, cond_g = assert_well_conditioned(o, o64, yo, y64, what)
    else:
        cond_f, cond_g = rel_err(yo, y64), float("nan")
        assert cond_f < CONDITION, "%s: ill-conditioned case, float32 oracle forward %.2e off float64" % (what, cond_f)
    m.train()
    y = m(x.to(device), normalize=normalize)
    assert_output_layout(y, N, D, H, W)
    assert status_clear(m), what
    fig = {"case": what, "fwd": rel_err(y.detach().cpu(), y64), "fwd_o32": cond_f, "grad_o32": cond_g}
    print("odd-size %s: forward engine %.2e / fp32 oracle %.2e" % (what, fig["fwd"], cond_f))
    tol = 3 * cond_f + FWD_FLOOR
    assert fig["fwd"] < tol, (what, fig["fwd"], tol)
    if normalize:
        assert float((y.detach().norm(2, 1) - 1).abs().max()) < 1e-5
    (y * gy.to(device)).sum().backward()
    if not gradient_parity:
        import parity_common as pc
        st = pc.grad_error_stats(m.named_parameters(), o.parameters(), o64.parameters(), ())
        fig.update(grad_rms=st["rms_gpu"], grad_rms_o32=st["rms_o32"], grad_max=st["max_gpu"], grad_max_o32=st["max_o32"])
        print("odd-size %s: gradients, relative L2 against float64 over the tensors: r.m.s. engine %.2e / fp32 oracle %.2e, worst "
              "engine %.2e / fp32 oracle %.2e" % (what, st["rms_gpu"], st["rms_o32"], st["max_gpu"], st["max_o32"]))
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters()), what
        pc.assert_as_accurate_as_float32(st, factor=2.0, floor=5e-4)
        assert_buffers_follow_oracle(m, o, what)
        return fig
    worst = (-1.0, None, 0.0, 0.0)
    failures = []
    for (k, p), po, p6 in zip(m.named_parameters(), o.parameters(), o64.parameters()):
        e, eo = rel_err(p.grad.cpu(), p6.grad), rel_err(po.grad, p6.grad)
        tol = 3 * eo + GRAD_FLOOR
        if e / tol > worst[0]:
            worst = (e / tol, k, e, eo)
        if not e < tol:
            failures.append((k, e, tol))
    fig.update(grad_worst=worst[1], grad=worst[2], grad_worst_o32=worst[3])
    print("odd-size %s: gradient furthest over its tolerance %s engine %.2e / fp32 oracle %.2e" % ((what,) + worst[1:]))
    assert not failures, (what, failures)
    assert_buffers_follow_oracle(m, o, what)
    return fig


def assert_buffers_follow_oracle(m, o, what):
    """BN running statistics / counters follow nn.BatchNorm2d."""
    for (k, b), bo in zip(m.named_buffers(), o.buffers()):
        b = b.cpu()
        assert rel_err(b.float(), bo.float()) < 1e-4 or float((b.float() - bo.float()).abs().max()) < 1e-5, (what, k)


def randomize_running_statistics(o, seed=5):
    """Running statistics away from their initial (0, 1), without a train-mode pass (tiny sizes have none worth using)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, b in o.named_buffers():
            if k.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif k.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)


def check_eval_vs_float64(arch, bw, shape, D, device, seed=2):
    """Eval mode (running statistics; in the split-fp16 arithmetic conv + folded BN (+ residual) + ReLU as one fused pass)
    against the float64 oracle: 3 * err(fp32 oracle) + 1e-5, plain and normalized; buffers untouched."""
    N, H, W = shape
    what = "%s bw%d %dx%dx%d D%d eval" % (arch, bw, N, H, W, D)
    key = ("eval", arch, D, bw, tuple(shape), seed)
    x, _ = inputs(N, H, W, D, seed)
    if key not in _ORACLE_STEPS:
        _, o = make_pair(arch, D, bw, "cpu")
        randomize_running_statistics(o)
        o64 = copy.deepcopy(o).double()
        o.eval(); o64.eval()
        with torch.no_grad():
            _ORACLE_STEPS[key] = (o.state_dict(), o(x), o64(x.double()))
    state, yo, y64 = _ORACLE_STEPS[key]
    m = product_module(arch, D, bw, device, state)
    m.eval()
    before = [b.clone() for b in m.buffers()]
    with torch.no_grad():
        y = m(x.to(device))
        assert_output_layout(y, N, D, H, W)
        assert status_clear(m), what
        cond = rel_err(yo, y64)
        fig = {"case": what, "fwd": rel_err(y.cpu(), y64), "fwd_o32": cond}
        print("odd-size %s: forward engine %.2e / fp32 oracle %.2e" % (what, fig["fwd"], cond))
        assert fig["fwd"] < 3 * cond + FWD_FLOOR, (what, fig)
        yn = m(x.to(device), normalize=True)
        n32, n64 = yo / yo.norm(2, 1, keepdim=True), y64 / y64.norm(2, 1, keepdim=True)
        fig.update(norm=rel_err(yn.cpu(), n64), norm_o32=rel_err(n32, n64))
        assert fig["norm"] < 3 * fig["norm_o32"] + FWD_FLOOR, (what, fig)
    assert all(torch.equal(a, b) for a, b in zip(before, m.buffers())), what
    return fig


def check_tiny_train_forward(arch, bw, shape, D, device):
    """Train mode on a 1 x 1 ... 4 x 1 low-resolution map: finite output of the right shape and a clear status word.  No
    parity claim (module docstring)."""
    N, H, W = shape
    m, _ = make_pair(arch, D, bw, device)
    x, gy = inputs(N, H, W, D, 3)
    m.train()
    y = m(x.to(device))
    assert_output_layout(y, N, D, H, W)
    assert bool(torch.isfinite(y).all()) and status_clear(m), (arch, shape)
    (y * gy.to(device)).sum().backward()
    assert all(p.grad is not None and tuple(p.grad.shape) == tuple(p.shape) and bool(torch.isfinite(p.grad).all())
               for p in m.parameters()), (arch, shape)


def check_pair_equals_two_calls(arch, bw, shape, device, expect_grouped, D=3, oracle_forward=True, fwd_tol=1e-6, grad_tol=1e-5,
                                buffer_tol=1e-6, real_width=False):
    """forward_pair(a, b) == (forward(a), forward(b)) at an odd size, to the standard of
    test_grouped_pair_forward_equals_two_forward_calls: outputs within 1e-6 of the engine's own two calls (and 2e-5 of the
    oracle called twice), parameter gradients = the sum of both calls' gradients within 1e-5, running statistics updated once
    per batch.  expect_grouped: the size admits the grouped plan (every batch-normed tensor has a multiple of 64 rows per
    group) and must take it; otherwise forward_pair must say that it runs two calls.
    fwd_tol / grad_tol: the defaults hold where both routes run the same kernels on the same tiles (host emulation).  On the
    GPU the grouped plan has twice the rows and may pick other tiles, i.e. another summation order: two float32-accurate
    results then, each within the parity tolerances of float64 -- 2e-5 forward; gradients 2 * (3 * 1e-5 + 2e-5) = 1e-4 on the
    well-conditioned narrow cases (float32 oracle below 1e-5 there).  real_width: the standard of
    tests/test_gpu_parity.py::test_forward_pair_equals_two_forward_calls_full_size -- every gradient tensor but fc.bias within
    2e-2 in the relative L2 norm (ill-conditioned: ReLU kinks), and on top the scoring layer's weight, which sees the forward
    activations and no ReLU / batch norm behind it, within grad_tol in the largest element."""
    from dcn_hip import backbone as _bb
    N, H, W = shape
    m, o = make_pair(arch, D, bw, device)
    m2 = copy.deepcopy(m)
    g = torch.Generator().manual_seed(3)
    xa = torch.randn(N, 3, H, W, generator=g)
    xb = torch.randn(N, 3, H, W, generator=g) * 1.7 + 0.3        # different statistics per batch
    ga = torch.randn(N, D, H, W, generator=g).to(device)
    gb = torch.randn(N, D, H, W, generator=g).to(device)
    m.train(); m2.train(); o.train()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ya, yb = m.forward_pair(xa.to(device), xb.to(device))
    grouped = any(k[-1] == 2 and k[2] == 2 * N and k[3:5] == (H, W) for k in _bb._PLANS)
    assert grouped == expect_grouped, (shape, sorted(_bb._PLANS))
    if expect_grouped:
        assert m._last_plan.groups == 2
    else:
        assert any("two forward calls" in str(w.message) for w in caught)
    assert_output_layout(ya, N, D, H, W); assert_output_layout(yb, N, D, H, W)
    assert status_clear(m)
    za, zb = m2(xa.to(device)), m2(xb.to(device))
    assert rel_err(ya.detach().cpu(), za.detach().cpu()) < fwd_tol and rel_err(yb.detach().cpu(), zb.detach().cpu()) < fwd_tol
    if oracle_forward:
        with torch.no_grad():
            oa, ob = o(xa), o(xb)
        assert rel_err(ya.detach().cpu(), oa) < 2e-5 and rel_err(yb.detach().cpu(), ob) < 2e-5
    ((ya * ga).sum() + (yb * gb).sum()).backward()
    ((za * ga).sum() + (zb * gb).sum()).backward()
    for (k, p), p2 in zip(m.named_parameters(), m2.parameters()):
        assert bool(torch.isfinite(p.grad).all()), k
        if real_width:
            if not k.endswith("fc.bias"):
                l2n = float((p.grad - p2.grad).norm() / p2.grad.norm())
                assert l2n < 2e-2, (k, l2n)
            if not k.endswith("fc.weight"):
                continue
        assert rel_err(p.grad.cpu(), p2.grad.cpu()) < grad_tol, (k, rel_err(p.grad.cpu(), p2.grad.cpu()))
    for (k, b), b2 in zip(m.named_buffers(), m2.buffers()):
        assert rel_err(b.float().cpu(), b2.float().cpu()) < buffer_tol, k
    if oracle_forward:
        for (k, b), bo in zip(m.named_buffers(), o.buffers()):
            b = b.cpu()
            assert rel_err(b.float(), bo.float()) < 1e-4 or float((b.float() - bo.float()).abs().max()) < 1e-5, k


def check_bit_reproducible(arch, bw, shape, D, device):
    """Two identical train steps: torch.equal outputs, gradients and running statistics."""
    N, H, W = shape
    m, _ = make_pair(arch, D, bw, device)
    m2 = copy.deepcopy(m)
    x, gy = inputs(N, H, W, D, 8)
    outs = []
    for net in (m, m2):
        net.train()
        y = net(x.to(device))
        (y * gy.to(device)).sum().backward()
        outs.append(y.detach())
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    for (k, p), p2 in zip(m.named_parameters(), m2.parameters()):
        assert bool(torch.isfinite(p.grad).all()) and torch.equal(p.grad, p2.grad), k
    for (k, b), b2 in zip(m.named_buffers(), m2.buffers()):
        assert torch.equal(b, b2), k


def wide_layer_descs(L, N, H, W, bw):
    """Descriptors of the stride-1 3 x 3 convolutions of layer1 and layer2 (basic blocks) at this image size."""
    _, (hp, wp), (hl, wl) = low_res(H, W)
    return [L.ConvDesc(N, hp, wp, bw, hp, wp, bw, 3, 3, 1, 1, 1, bw, 0),
            L.ConvDesc(N, hl, wl, 2 * bw, hl, wl, 2 * bw, 3, 3, 1, 1, 1, 2 * bw, 0)]


def check_hl32_at_odd_size(L, device, set_env, arch, bw, shape, rows, D=3):
    """The wide layers through the pre-split (hl32) kernels (DCN_GEMM_HL=2, DCN_WGRAD_HL=2) with the tile height forced to
    `rows`, at a size whose row counts are a multiple of no tile height: forward against the float64 oracle and the engine's
    own fp32-operand kernels; backward on the SAME saved arena against the fp32-operand dgrads and weight gradients (the
    standard of test_wide_layers_through_the_hl32_path).  That the hl32 kernel ran, on ragged tiles of that height, is
    asserted: from the tile arithmetic the engine itself uses and from the profile's hl32 launch count."""
    from dcn_hip import backbone as _bb
    lib = L.get()
    N, H, W = shape
    m, o = make_pair(arch, D, bw, device)
    m2, m3 = copy.deepcopy(m), copy.deepcopy(m)
    o64 = copy.deepcopy(o).double()
    x, gy = inputs(N, H, W, D, 7)
    xd, gyd = x.to(device), gy.to(device)
    for net in (m, m2, m3, o, o64):
        net.train()
    _, _, (hl, wl) = low_res(H, W)
    assert all((N * hl * wl) % r for r in (160, 192, 256, 320)), "choose a size whose low-resolution rows are ragged"
    try:
        set_env(DCN_GEMM_HL=2, DCN_WGRAD_HL=2, DCN_GEMM_HL_ROWS=rows)
        _bb._PLANS.clear()                     # (plans reserve the saved hl32 images when they are built: after the switches are set)
        for d in wide_layer_descs(L, N, H, W, bw):
            M = d.n * d.hout * d.wout
            for dgrad in (0, 1):
                assert lib.dcn_conv_hl_eligible(ctypes.byref(d), dgrad) == 1
                assert lib.dcn_conv_tile_rows_hl(ctypes.byref(d), dgrad) == rows
            assert M % rows != 0 and lib.dcn_conv_num_mtiles_hl(ctypes.byref(d)) == (M + rows - 1) // rows
        plan = _bb.get_plan(arch, bw, N, H, W, D)
        plan.profile_begin()
        y = m(xd)
        prof = plan.profile_end()
        n_hl = prof["conv_gemm_hl"][1]
        # every stride-1 convolution of 32-channel granularity but the stem and the scoring layer: at least two per block
        # of layers 1, 3 and 4 and of layer2 behind its first
        assert n_hl >= 12 and prof["conv_gemm"][1] > n_hl, prof
        assert status_clear(m)
        set_env(DCN_GEMM_HL=0, DCN_WGRAD_HL=2, DCN_GEMM_HL_ROWS=rows)
        y2, y3 = m2(xd), m3(xd)
        yo, y64 = o(x), o64(x.double())
        cond = rel_err(yo, y64)
        fig = {"fwd": rel_err(y.detach().cpu(), y64), "fwd_o32": cond, "hl_launches": n_hl}
        assert fig["fwd"] < 3 * cond + FWD_FLOOR, fig
        assert rel_err(y.detach().cpu(), y2.detach().cpu()) < 3 * cond + 2e-5
        for (k, b), b2 in zip(m.named_buffers(), m2.buffers()):
            b, b2 = b.float().cpu(), b2.float().cpu()
            assert rel_err(b, b2) < 1e-4 or float((b - b2).abs().max()) < 1e-5, k
        set_env(DCN_GEMM_HL=0, DCN_WGRAD_HL=0, DCN_GEMM_HL_ROWS=rows)
        (y2 * gyd).sum().backward()            # fp32-operand dgrads and weight gradients
        set_env(DCN_GEMM_HL=2, DCN_WGRAD_HL=2, DCN_GEMM_HL_ROWS=rows)
        plan.profile_begin()
        (y3 * gyd).sum().backward()            # hl32 dgrads and weight gradients on an identical saved arena
        assert plan.profile_end()["conv_gemm_hl"][1] >= 12
        for (k, p2), p3 in zip(m2.named_parameters(), m3.parameters()):
            e = rel_err(p3.grad.cpu(), p2.grad.cpu())
            assert e < 3e-5, (k, e)
    finally:
        _bb._PLANS.clear()
    return fig


def check_bn_backward_reduction_fused(device, set_env, arch, groups, conv_mode, shape):
    """The fused dgrad + batch-norm backward reduction against the separate reduce pass (DCN_BN_BWD_FUSED=0), as
    tests/test_emu_backbone.py::test_bn_backward_reduction_fused_into_dgrad holds it at 32 x 40 / 64 x 64: here the dgrad M
    tiles and the mask bytes are ragged.
    Fused against separate under the SAME K split: the forward passes are then identical bit for bit -- same ReLU masks -- and
    only the summation order of the reduction differs (1e-3, the bound of the original for that comparison).  Across K splits
    (stream-K forced or not) the forward passes differ in round-off, which the basic-block network carries (1e-2, as in the
    original) and the bottleneck network does not: Resnet50_8s at 2 x 37 x 53 measures 2.1e-1 between the two SEPARATE runs,
    with the float64 oracle 2.1e-1 from one and 1.6e-2 from the other (a ReLU element on the other side of zero)."""
    N, H, W = shape
    grads = {}
    for fused, sk, fix in ((0, None, None), (1, None, None), (0, 3, "inline"), (1, 3, "inline"), (1, 3, "kernel")):
        env = {"DCN_BN_BWD_FUSED": fused}
        if sk:
            env.update(DCN_GEMM_SK=sk, DCN_GEMM_SK_FIXUP=fix)
        set_env(**env)
        m, _ = make_pair(arch, 3, 8, device)
        g = torch.Generator().manual_seed(5)
        xa = torch.randn(N, 3, H, W, generator=g).to(device)
        xb = torch.randn(N, 3, H, W, generator=g).to(device)
        gy = torch.randn(N, 3, H, W, generator=g).to(device)
        m.train()
        if groups == 2:
            ya, yb = m.forward_pair(xa, xb)
            ((ya * gy).sum() + (yb * gy).sum()).backward()
        else:
            (m(xa) * gy).sum().backward()
        plan = m._last_plan
        assert plan.groups == groups and (plan.h, plan.w) == (H, W)
        n_bn = len(plan.bn_names)
        n_down = sum(1 for k in plan.bn_names if "downsample" in k)
        want = (n_bn - n_down - 1) if (fused and conv_mode == "f16x3") else 0
        assert plan.fused_bn_backward() == want, (plan.fused_bn_backward(), want)
        grads[(fused, sk, fix)] = [p.grad.cpu().clone() for p in m.parameters()]
        set_env(DCN_GEMM_SK=-1, DCN_GEMM_SK_FIXUP="inline")   # (back to the defaults for the next round of the loop)
    worst = lambda a, b: max(rel_err(x, y) for x, y in zip(grads[a], grads[b]))
    assert worst((1, None, None), (0, None, None)) < 1e-3
    assert worst((1, 3, "inline"), (0, 3, "inline")) < 1e-3
    if arch != "Resnet50_8s":
        for key in grads:
            assert worst(key, (0, None, None)) < (1e-2 if key[1] else 1e-3), key
    assert all(torch.equal(a, b) for a, b in zip(grads[(1, 3, "inline")], grads[(1, 3, "kernel")]))


def check_evaluate_on_store(device, h, w, tiny_dcn):
    """dcn_hip.evaluate.evaluate_network / evaluate_frame_pairs on an h x w synthetic frame store with the real tiny network:
    the reference's columns, the row count of the device path run by hand, the same table twice for a fixed generator, train /
    eval mode restored, and every pair's best matches against the per-pair public pieces (forward_image_tensors +
    match.find_best_matches).  On the host emulation the pixels are equal.  On the GPU the per-pair call has another batch
    shape than the batched one, i.e. other tiles and another summation order: the backbone's parity bound is 1e-4 of the
    descriptor image's largest magnitude per element, so a distance between two descriptors of D elements may move by
    tol = 2 * sqrt(D) * 1e-4 * max|descriptor|, and the chosen pixel may differ only where its distance on the per-pair
    descriptors lies within 2 * tol of the best (the argument of tests/test_gpu_evaluate.py)."""
    import evaluate_common as ec
    from dcn_hip import augment, evaluate, match, samples
    dev = torch.device(device)
    on_host = dev.type == "cpu"
    D = 3
    store = ec.synthetic_store(device, h, w)
    assert tuple(store.rgb.shape[1:3]) == (h, w)
    dcn = tiny_dcn(h, w)
    if not on_host:
        dcn = dcn.to(dev)
    dcn.train()
    gen = lambda: torch.Generator(device).manual_seed(4)
    run = lambda: evaluate.evaluate_network(dcn, store, num_image_pairs=6, num_matches_per_image_pair=7,
                                            host_rng=np.random.RandomState(2), generator=gen())
    table, df = run()
    assert dcn.training
    names = set(evaluate.COLUMNS) | {"is_valid", "is_valid_masked", "scene_name", "img_a_idx", "img_b_idx"}
    assert set(table) == names
    assert set(evaluate.COLUMNS) | {"is_valid", "is_valid_masked"} <= {
        "is_valid", "is_valid_masked", "norm_diff_descriptor_ground_truth", "norm_diff_descriptor",
        "norm_diff_descriptor_masked", "norm_diff_ground_truth_3d", "norm_diff_pred_3d", "norm_diff_pred_3d_masked",
        "pixel_match_error_l2", "pixel_match_error_l2_masked", "pixel_match_error_l1",
        "fraction_pixels_closer_than_ground_truth", "fraction_pixels_closer_than_ground_truth_masked",
        "average_l2_distance_for_false_positives", "average_l2_distance_for_false_positives_masked"}
    try:
        import pandas  # noqa: F401
        assert list(df.columns) == list(evaluate.COLUMNS) + ["is_valid", "is_valid_masked", "scene_name", "img_a_idx",
                                                             "img_b_idx"] and len(df) == len(table["is_valid"])
    except ImportError:
        assert df is None
    # the row count: sum over the chosen pairs of min(num_matches, total), from the device path run by hand
    chosen = evaluate.choose_pairs(store, 6, np.random.RandomState(2))
    t = evaluate.evaluate_frame_pairs(dcn, store, chosen, 7, generator=gen())
    assert int(t.status.cpu()[0]) == 0
    ia, ib = torch.from_numpy(chosen[:, 1]).to(dev), torch.from_numpy(chosen[:, 2]).to(dev)
    poses = store.poses.cpu().numpy().reshape(-1, 4, 4)
    cams = samples._cameras(store.K[chosen[:, 0]], poses[chosen[:, 1]], poses[chosen[:, 2]], len(chosen), dev)
    mm = evaluate.find_eval_matches(store.depth[ia], store.depth[ib], store.mask[ia], cams, 7, generator=gen())
    rows = int(np.minimum(mm.totals.cpu().numpy(), 7).sum())
    assert rows > 0 and len(table["is_valid"]) == rows == int(t.offsets.cpu()[-1])
    assert all(len(v) == rows for v in table.values())
    rp = t.row_pair.cpu().numpy()[:rows]
    assert np.array_equal(table["img_a_idx"], (chosen[:, 1] - np.asarray(store.scene_first_frame_host)[chosen[:, 0]])[rp])
    assert table["scene_name"].tolist() == [store.scene_names[s] for s in chosen[rp, 0]]
    # deterministic for a fixed generator; eval mode is restored too
    table2, _ = run()
    for k in names:
        assert np.array_equal(table[k], table2[k], equal_nan=True) if table[k].dtype != object else \
            table[k].tolist() == table2[k].tolist(), k
    dcn.eval()
    run()
    assert not dcn.training
    # descriptors in eval mode: every pair's best matches equal the per-pair public pieces
    off = t.offsets.cpu().numpy()
    mean = torch.tensor(augment.DEFAULT_IMAGE_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(augment.DEFAULT_IMAGE_STD_DEV, device=dev).view(1, 3, 1, 1)
    checked = 0
    for p in range(len(chosen)):
        lo, hi = int(off[p]), int(off[p + 1])
        if hi == lo:
            continue
        a, b = int(chosen[p, 1]), int(chosen[p, 2])
        x = (torch.stack([store.rgb[a], store.rgb[b]]).permute(0, 3, 1, 2).float().div(255) - mean) / std
        res = dcn.forward_image_tensors(x)
        assert tuple(res.shape) == (2, h, w, D)
        q = res[0][t.v_a[lo:hi].long(), t.u_a[lo:hi].long()]
        idx, _dist, _ = match.find_best_matches(res[1], q)
        pu, pv = t.pred_uv[0, lo:hi].long(), t.pred_uv[1, lo:hi].long()
        same = (idx % w == pu) & (idx // w == pv)
        if on_host:
            assert bool(same.all()), p
        else:
            tol = 2.0 * np.sqrt(D) * 1e-4 * float(res.abs().max())
            nd = (res[1].reshape(1, h * w, D).double() - q.double()[:, None, :]).norm(dim=2)      # [rows, HW]
            rr = torch.arange(hi - lo, device=dev)
            assert bool((same | (nd[rr, pv * w + pu] - nd.min(dim=1).values <= 2 * tol)).all()), p
        checked += hi - lo
    assert checked == rows
