"""Abs-max bounds, the fused inference convolution and the engine's batch-norm backward against float64 (shared by
test_emu_range.py -- host emulation -- and test_gpu_range.py -- MI355X; not a test module).

Every convolution operand of the split-fp16 arithmetic is pre-scaled by a power of two chosen from a device scalar that must be
>= max |tensor| (pow2_scale, csrc/f16_split.h).  A scalar that comes out too low overflows fp16, one far too high sinks the lo
halves into subnormals -- neither makes any other test fail.  The checks below hold every producer of such a scalar, and the
kernels around them, to a plain torch reference evaluated in float64 on the CPU from the same fp32 inputs."""
import copy
import ctypes
import functools

import torch
import torch.nn.functional as F

from helpers import rel_err
from kernel_checks import garbage, hl32_decode

SPLIT_TOL = 3e-7      # (hi + lo) / scale against the fp32 value: what the project holds every split image to
FUSED_TOL = 3e-6      # dcn_conv_forward_f16's bound at these shapes (test_conv_f16x3_forward_dgrad); the epilogue adds fp32 additions
BN_TOL = 2e-5         # check_dgrad_with_bn_backward's bound for dx / dgamma / dbeta
GE = 1.0 - 2.0 ** -20   # "bound >= true maximum": one part in 2^20 for the float32 rounding of the bound itself

# n, h, w, cin, cout, k, stride, pad, dil
FUSED_CASES = [
    (3, 7, 7, 8, 8, 3, 1, 1, 1),         # M = 147: the last M tile is ragged at every tile height
    (1, 10, 12, 20, 136, 3, 1, 2, 2),    # two N tiles, the second ragged (column 135 is the last valid one); M = 120
    (1, 12, 10, 16, 24, 3, 2, 1, 1),     # stride 2, M = 30
    (2, 5, 6, 32, 512, 1, 1, 0, 1),      # 1x1, K = 32 (one stage: never stream-K), four N tiles, M = 60
]
FUSED_CASES_GPU = FUSED_CASES + [
    (2, 30, 40, 64, 64, 3, 1, 1, 1),     # M = 2400, the uniform-tap path
    (1, 15, 20, 128, 136, 3, 1, 2, 2),   # K = 1152, ragged N tile, M = 300
]

# (case, DCN_GEMM_TILE_M, DCN_GEMM_SK) at which f16_shape (csrc/conv_f16_kernels.hip) does not split: K = 32 is a single stage; a
# tile count that is a multiple of the forced workgroup count stays data-parallel (M = 147: three 64-row tiles -- 256 falls
# back to 64 for cout <= 64 --; M = 300 x two N tiles: ten 64-row tiles, six 128-row tiles)
NOT_STREAM_K = {(FUSED_CASES_GPU[3], t, s) for t in ("64", "128", "256") for s in ("3", "5", "7")} | {
    (FUSED_CASES_GPU[0], "64", "3"), (FUSED_CASES_GPU[0], "256", "3"), (FUSED_CASES_GPU[5], "64", "5"), (FUSED_CASES_GPU[5], "128", "3")}


def _arr(ty, vals):
    return (ty * len(vals))(*vals)


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ weight images
def split_weights(L, dev, ws, row_scales=None, status=None, scale=64.0):
    """dcn_split_weights_scaled_f16 (status None) or dcn_split_weights_checked_f16 over the table `ws` of [cout][taps][cin]
    tensors: (his, los) of NaN-prefilled [cout][kpad] fp16 images.  row_scales: None or a list of None / [cout] vectors."""
    lib = L.get()
    n = len(ws)
    P, I = ctypes.c_void_p, ctypes.c_int
    wd = [w.to(dev).contiguous() for w in ws]
    rs = None if row_scales is None else [None if r is None else r.to(dev).contiguous() for r in row_scales]
    his, los = [], []
    for w in ws:
        co, tp, ci = w.shape
        kp = lib.dcn_f16_kpad(tp * ci)
        his.append(torch.full((co, kp), float("nan"), dtype=torch.float16, device=dev))
        los.append(torch.full((co, kp), float("nan"), dtype=torch.float16, device=dev))
    a_w = _arr(P, [w.data_ptr() for w in wd])
    a_rs = None if rs is None else _arr(P, [None if r is None else r.data_ptr() for r in rs])
    a_hi, a_lo = _arr(P, [t.data_ptr() for t in his]), _arr(P, [t.data_ptr() for t in los])
    a_co, a_tp, a_ci = (_arr(I, [w.shape[j] for w in ws]) for j in range(3))
    if status is None:
        rc = lib.dcn_split_weights_scaled_f16(n, a_w, a_rs, a_hi, a_lo, a_co, a_tp, a_ci, a_co, 0, scale, None)
    else:
        rc = lib.dcn_split_weights_checked_f16(n, a_w, a_rs, a_hi, a_lo, a_co, a_tp, a_ci, scale, L.ptr(status), None)
    assert rc == 0, rc
    _sync(dev)   # (wd / rs are released on return)
    return his, los


# ------------------------------------------------------------------------------------------------ 1. fused inference convolution
@functools.lru_cache(maxsize=None)
def _fused_problem(case, seed=0):
    """Inputs of one shape and the float64 convolution of them (computed once, shared by every option combination)."""
    n, hin, win, cin, cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hin, win, cin, generator=g)
    w = torch.randn(cout, k, k, cin, generator=g) / (k * k * cin) ** 0.5    # outputs O(1) at every K: a planted 50 stands out
    rs = torch.rand(cout, generator=g) + 0.5                                # positive per-channel factors (a folded BN scale)
    hout = (hin + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wout = (win + 2 * pad - dil * (k - 1) - 1) // stride + 1
    bias = torch.randn(cout, generator=g) * 0.5
    add = torch.randn(n, hout, wout, cout, generator=g)
    ws64 = w.double() * rs.double().reshape(cout, 1, 1, 1)
    conv64 = F.conv2d(x.double().permute(0, 3, 1, 2), ws64.permute(0, 3, 1, 2), None, stride, pad, dil).permute(0, 2, 3, 1).contiguous()
    conv32 = F.conv2d(x.permute(0, 3, 1, 2), ws64.float().permute(0, 3, 1, 2), None, stride, pad, dil).permute(0, 2, 3, 1).contiguous()
    return {"x": x, "w": w, "rs": rs, "bias": bias, "add": add, "conv64": conv64, "conv32": conv32, "hout": hout, "wout": wout}


def _epilogue64(conv, bias, add, relu):
    out = conv.double()
    if bias is not None:
        out = out + bias.double()
    if add is not None:
        out = out + add.double()
    return torch.relu(out) if relu else out


def _epilogue32(conv32, bias, add, relu):
    """The float32 torch reference of the same operation (what a tolerance is measured with, never compared against)."""
    out = conv32
    if bias is not None:
        out = out + bias
    if add is not None:
        out = out + add
    return torch.relu(out) if relu else out


def planted(case, plant, P):
    """(bias, add, relu or None, where) of a planted-maximum case: the extreme value enters through `add` / `bias`, so its
    position does not depend on the kernel.  where = (row, column) of the planted element of the [M][cout] output."""
    cout = case[4]
    M = case[0] * P["hout"] * P["wout"]
    bias, add = P["bias"].clone(), P["add"].clone().reshape(M, cout)
    relu = None
    if plant == "last_row":            # (a) the last valid row of the ragged last M tile
        where = (M - 1, cout // 2)
        add[where] = 50.0
    elif plant == "last_col":          # (b) the last valid column of the ragged N tile
        where = (M // 3, cout - 1)
        add[where] = 50.0
    elif plant == "last_tile":         # stream-K: the last row AND the last column -- the last tile of the launch
        where = (M - 1, cout - 1)
        add[where] = 50.0
    elif plant in ("neg", "neg_relu"):   # (c) / (d)
        where = (M // 2, cout // 3)
        add[where] = -50.0
        relu = 1 if plant == "neg_relu" else 0
    elif plant == "cancel":            # (e) bias +100 against add -100 in one channel: rows >= M would read 0 + 100
        where = (M - 1, cout - 1)
        bias[cout - 1] = 100.0
        add[:, cout - 1] -= 100.0
    else:
        raise ValueError(plant)
    return bias, add.reshape(P["add"].shape), relu, where


def fused_images(L, dev, case, P):
    """The weight images of the case from dcn_split_weights_scaled_f16, checked against w * row_scale."""
    n, hin, win, cin, cout, k, stride, pad, dil = case
    K = k * k * cin
    his, los = split_weights(L, dev, [P["w"].reshape(cout, k * k, cin)], [P["rs"]])
    wh, wl = his[0], los[0]
    rec = (wh.cpu().double() + wl.cpu().double()) / 64.0
    want = (P["w"].double() * P["rs"].double().reshape(cout, 1, 1, 1)).reshape(cout, K)
    e = rel_err(rec[:, :K], want)
    assert e < SPLIT_TOL, e
    if rec.shape[1] > K:   # pad columns K .. kpad: exactly zero in both halves (NaN-prefilled, so also: written)
        assert float(wh.cpu()[:, K:].abs().max()) == 0.0 and float(wl.cpu()[:, K:].abs().max()) == 0.0
    return wh, wl


def run_fused(L, dev, case, P, wh, wl, bias, add, relu, absmax0=None, in_scale=None, ws=None, launches=1):
    """dcn_conv_forward_fused_f16 `launches` times on the same workspace; returns [(out, out_absmax or None)] as CPU tensors.
    absmax0: None (no out_absmax), or the value the word holds before each launch.  in_scale: None, or the input (and bias /
    add) are multiplied by it and max |input| is passed as in_absmax."""
    lib = L.get()
    n, hin, win, cin, cout, k, stride, pad, dil = case
    d = L.ConvDesc(n, hin, win, cin, P["hout"], P["wout"], cout, k, k, stride, pad, dil, cout, 0)
    f = 1.0 if in_scale is None else in_scale
    xd = (P["x"] * f).to(dev).contiguous()
    ax = xd.abs().max().reshape(1).clone() if in_scale is not None else None
    bd = (bias * f).to(dev).contiguous() if bias is not None else None
    ad = (add * f).to(dev).contiguous() if add is not None else None
    res = []
    for _ in range(launches):
        out = torch.full((n, P["hout"], P["wout"], cout), float("nan"), device=dev)
        am = torch.full((1,), float(absmax0), device=dev) if absmax0 is not None else None
        rc = lib.dcn_conv_forward_fused_f16(ctypes.byref(d), L.ptr(xd), L.ptr(ax) if ax is not None else None, L.ptr(wh), L.ptr(wl),
                                            64.0, L.ptr(bd) if bd is not None else None, L.ptr(ad) if ad is not None else None,
                                            int(relu), L.ptr(out), L.ptr(am) if am is not None else None,
                                            L.ptr(ws) if ws is not None else None, None)
        assert rc == 0, rc
        res.append((out.cpu(), am.cpu() if am is not None else None))
    return res


def _hold_fused(out, am, ref64, tol, absmax0, what):
    e = rel_err(out, ref64)
    assert e < tol, (what, e, tol)
    if am is None:
        return e
    m = out.abs().max().reshape(1)          # max |out| of the tensor the kernel stored: the word is a max of stored values
    if absmax0 > float(m):
        assert float(am) == float(torch.tensor(absmax0, dtype=torch.float32)), (what, float(am), absmax0)   # pre-set above: unchanged
    else:
        assert torch.equal(am, m), (what, float(am), float(m))             # from 0 or from below: the maximum, bit for bit
    return e


def check_fused_conv(L, dev, case, bias=True, add=True, relu=0, absmax0=0.0, in_scale=None, plant=None):
    """One option combination of out = [relu](conv(in, w * row_scale) + bias [+ add]) against F.conv2d in float64 at
    rel_err < 3e-6, and out_absmax against max |out| of the stored tensor, bit for bit.

    No case needs more than 3e-6.  The one that comes close is the planted `cancel` case ((e): bias = +100, add = -100 in one
    channel): the intermediate conv + 100 is rounded to float32's 7.6e-6 spacing at 100 while the stored values are O(1).
    Measured for it -- float32 torch (F.conv2d, + bias, + add) against the float64 reference on the same inputs: 4.8e-7 to
    9.4e-7 over the six shapes (1.4e-7 to 9.4e-7 without the plant); 3 x that stays inside 3e-6, which is held as it is."""
    P = _fused_problem(case)
    wh, wl = fused_images(L, dev, case, P)
    b, a = (P["bias"] if bias else None), (P["add"] if add else None)
    where = None
    tol = FUSED_TOL
    if plant is not None:
        b, a, r, where = planted(case, plant, P)
        relu = relu if r is None else r
    ref = _epilogue64(P["conv64"], b, a, relu)
    cout = case[4]
    if plant is not None:
        flat = ref.reshape(-1, cout)
        mx = float(flat.abs().max())
        if plant in ("last_row", "last_col", "last_tile", "neg"):
            assert mx > 40.0 and abs(float(flat[where])) == mx       # the planted element IS the maximum ...
            flat2 = flat.clone(); flat2[where] = 0.0
            assert float(flat2.abs().max()) < 10.0                   # ... and every other output is O(1)
        else:
            assert mx < 10.0, mx                                     # (d), (e): the true maximum is O(1), not 50 / 100
        if plant == "cancel":
            print("fused conv %s cancel: float32 torch vs float64 = %.2e" % (case, rel_err(_epilogue32(P["conv32"], b, a, relu), ref)))
    f = 1.0 if in_scale is None else in_scale
    (out, am), = run_fused(L, dev, case, P, wh, wl, b, a, relu, absmax0=None if absmax0 is None else absmax0 * f, in_scale=in_scale)
    e = _hold_fused(out, am, ref * f, tol, None if absmax0 is None else absmax0 * f, (case, bias, add, relu, absmax0, in_scale, plant))
    if am is not None and plant in ("neg_relu", "cancel"):
        assert float(am) < 10.0, float(am)
    return e


def check_fused_conv_stream_k(L, dev, set_env, case, tile_m, sk):
    """The epilogue on stream-K'd tiles: completed inside the launch (DCN_GEMM_SK_FIXUP=inline) and by the fix-up kernel
    (=kernel), on a garbage-filled workspace, twice on the workspace left behind; the planted maximum sits in the last tile."""
    lib = L.get()
    P = _fused_problem(case)
    n, hin, win, cin, cout, k, stride, pad, dil = case
    d = L.ConvDesc(n, hin, win, cin, P["hout"], P["wout"], cout, k, k, stride, pad, dil, cout, 0)
    b, a, _, where = planted(case, "last_tile", P)
    res = {}
    for mode in ("kernel", "inline"):
        set_env(DCN_GEMM_TILE_M=tile_m, DCN_GEMM_SK=sk, DCN_GEMM_SK_FIXUP=mode)
        wh, wl = fused_images(L, dev, case, P)
        nbytes = lib.dcn_conv_gemm_workspace_f16(ctypes.byref(d), 0)
        assert nbytes > 8, "stream-K is not exercised by this shape"
        ws = garbage(nbytes, dev, seed=11)
        res[mode] = run_fused(L, dev, case, P, wh, wl, b, a, 1, absmax0=0.0, ws=ws, launches=2)
    ref = _epilogue64(P["conv64"], b, a, 1)
    flat = ref.reshape(-1, cout)
    assert float(flat[where]) == float(flat.abs().max()) > 40.0
    o_k, m_k = res["kernel"][0]
    for mode in ("kernel", "inline"):
        for out, am in res[mode]:
            _hold_fused(out, am, ref, FUSED_TOL, 0.0, (case, tile_m, sk, mode))
            assert torch.equal(out, o_k) and torch.equal(am, m_k), (case, tile_m, sk, mode)
            assert float(out.reshape(-1, cout)[where]) == float(am)     # the maximum is the planted element of the last tile


# ------------------------------------------------------------------------------------------------ 2. weight range status
def _status_after(L, dev, ws, row_scales, start):
    """dcn_split_weights_checked_f16 on a status word holding `start`; the images must equal dcn_split_weights_scaled_f16's on
    the same arguments bit for bit (NaN payloads included: compared as 16-bit words)."""
    st = torch.full((1,), start, dtype=torch.int32, device=dev)
    his, los = split_weights(L, dev, ws, row_scales, status=st)
    rh, rl = split_weights(L, dev, ws, row_scales)
    for t, r in zip(his + los, rh + rl):
        assert torch.equal(t.cpu().view(torch.int16), r.cpu().view(torch.int16))
    return int(st.cpu()[0])


def check_weight_range_status(L, dev):
    """flag_weight_range (csrc/conv_f16_kernels.hip): bit 1 is raised iff some |scale * row_scale * w| > 65504 or a weight is
    NaN; the word is never cleared and no other bit is touched.  scale = 64."""
    g = torch.Generator().manual_seed(3)
    base = torch.randn(8, 9, 8, generator=g) * 0.1
    for start in (0, 1, 2, 5):                                        # all weights in range: unchanged
        assert _status_after(L, dev, [base], None, start) == start
    edge = torch.tensor(1023.5)                                       # 64 * 1023.5 = 65504 exactly: the largest finite fp16
    above = torch.nextafter(edge, torch.tensor(float("inf")))
    assert float(above) > 1023.5

    def one(value, rs=None, start=0, pos=(5, 4, 3)):
        w = base.clone()
        w[pos] = value
        return _status_after(L, dev, [w], None if rs is None else [torch.full((8,), float(rs))], start)
    assert one(edge) == 0 and one(-edge) == 0
    assert one(above) == 2 and one(-above) == 2
    assert one(above, start=1) == 3 and one(above, start=5) == 7      # raised next to the other bits; 2 | 2 stays 2
    assert one(above, start=2) == 2
    assert one(10.0, rs=100) == 0                                     # 64 * 100 * 10 = 64000
    assert one(10.0, rs=103) == 2                                     # 64 * 103 * 10 = 65920
    assert one(-10.0, rs=103) == 2
    assert one(float("nan")) == 2
    assert one(float("inf")) == 2 and one(float("-inf")) == 2
    # more than one batch of the table (48 tensors per launch): the very last element of the last of 66 tensors
    shapes = [(64, 49, 4), (64, 9, 64), (128, 9, 64), (3, 1, 32), (40, 1, 24), (8, 9, 8)] * 11
    table = [torch.randn(*s, generator=g) * 0.1 for s in shapes]
    assert len(table) == 66 and _status_after(L, dev, table, None, 0) == 0
    table[-1][-1, -1, -1] = float(above)
    assert _status_after(L, dev, table, None, 0) == 2
    rs = [torch.rand(s[0], generator=g) + 0.5 if i % 2 else None for i, s in enumerate(shapes)]    # some entries scaled, some not
    table[-1][-1, -1, -1] = 0.1
    assert _status_after(L, dev, table, rs, 4) == 4
    # K % 8 != 0 (taps 49, cin 4: K = 196, kpad = 200): the last real k of the last row sits in front of four pad halves
    w = torch.randn(12, 49, 4, generator=g) * 0.1
    assert _status_after(L, dev, [w], None, 0) == 0
    w[-1, -1, -1] = float(above)
    assert _status_after(L, dev, [w], None, 0) == 2
    w[-1, -1, -1] = float("nan")
    assert _status_after(L, dev, [w], None, 1) == 3


def build_pair(arch, D, bw, seed=0):
    """(engine model, float32 oracle) with the same parameters (oracle/resnet_dilated_oracle.py)."""
    from oracle import resnet_dilated_oracle as orc
    from pytorch_segmentation_detection.models import resnet_dilated as prod
    o = orc.build(arch, D, seed=seed, base_width=bw)
    m = getattr(prod, arch)(num_classes=D, base_width=bw)
    m.load_state_dict(o.state_dict(), strict=True)
    return m, o


def check_eval_fold_weight_range(dev):
    """Engine, f16x3: every weight legal, but one channel's running variance so small that the eval-mode fold
    64 * w * gamma / sqrt(var + eps) leaves fp16's range: bit 1 in eval mode, not in train mode."""
    from dcn_hip import backbone
    backbone.set_conv_mode("f16x3")
    try:
        m, _ = build_pair("Resnet18_8s", 3, 8)
        m = m.to(dev)
        net = m.resnet18_8s
        x = torch.randn(2, 3, 32, 40, generator=torch.Generator().manual_seed(4)).to(dev)
        with torch.no_grad():
            wt = net.get_parameter("layer2.0.conv1.weight")
            wt[3, 2, 1, 1] = 5.0                                                 # 64 * 5 = 320: legal
            assert float(wt.abs().max()) == 5.0
            bn = net.get_submodule("layer2.0.bn1")
            bn.running_var[3] = 1.0e-5                                           # gamma / sqrt(var + eps) = 1 / sqrt(2e-5) = 223.6
            fold = 64.0 * 5.0 * float(bn.weight[3]) / float(torch.sqrt(bn.running_var[3].double() + m.bn_eps))
            assert fold > 65504.0, fold                                          # 71 554
        with torch.no_grad():
            bn.running_var[3] = 1.0
        m.eval()
        with torch.no_grad():
            m(x)
        assert int(m.last_forward_status()[1]) == 0                              # the same weights with a legal fold (320): clear
        with torch.no_grad():
            bn.running_var[3] = 1.0e-5
        m.train()                                                                # train mode: batch statistics, nothing folded
        m(x)
        assert int(m.last_forward_status()[1]) == 0
        with torch.no_grad():
            bn.running_var[3] = 1.0e-5                                           # (the train call moved it)
        m(x)                                                                     # (no FloatingPointError: nothing was flagged)
        assert int(m.last_forward_status()[1]) == 0
        with torch.no_grad():
            bn.running_var[3] = 1.0e-5
        # eval mode last: the call after a flagged one raises FloatingPointError
        # (test_status_word_flags_nan_input_and_out_of_range_weights)
        m.eval()
        with torch.no_grad():
            m(x)
        assert int(m.last_forward_status()[1]) == 2
    finally:
        backbone.set_conv_mode(None)


# ------------------------------------------------------------------------------------------------ 3. batch-norm backward
BN_SETTINGS = ({"DCN_BN_BWD_LEAN": 0}, {"DCN_BN_BWD_LEAN": 1}, {"DCN_BN_BWD_LEAN": 1, "DCN_BN_BWD_LEAN_DEPTH": 1})
OUT_MODES = ("plain", "blocked", "hl_only", "hl_blocked_keep")
MASK_MODES = ("bytes", "relu_out", "none")


def bn_inputs(C, rows, groups, seed):
    """Random inputs with the largest |g| planted in the LAST row and the largest |xhat| in another row of the last chunk (every
    channel, so that the last group's term is the maximum of the bound whatever the channel's gamma * invstd)."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(rows, C, generator=g)
    dy2 = 0.5 * torch.randn(rows, C, generator=g)
    x = 3.0 * torch.randn(rows, C, generator=g) + 0.7
    relu_out = torch.randn(rows, C, generator=g)
    mask = torch.randint(0, 16, (rows * C // 4,), generator=g, dtype=torch.uint8)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    stats = torch.randn(groups, 4, C, generator=g)
    stats[:, 3] = 0.2 + stats[:, 3].abs()                                    # invstd > 0
    if groups == 2:                                                          # the groups' invstd differ, by less than the plant's factor
        stats[1, 3] = stats[0, 3] * (0.8 + 0.45 * torch.rand(C, generator=g))
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    last, other = rows - 1, rows - 3
    dy[last] = 40.0 * sign
    dy2[last] = 0.0
    relu_out[last] = 1.0
    mask.view(rows, C // 4)[last] = 15
    x[other] = stats[groups - 1, 2] + 60.0 * sign / stats[groups - 1, 3]    # xhat = +-60 there
    return {"dy": dy.reshape(-1), "dy2": dy2.reshape(-1), "x": x.reshape(-1), "relu_out": relu_out.reshape(-1), "mask": mask,
            "gamma": gamma, "stats": stats.reshape(-1).contiguous()}


def bn_reference(inp, C, rows, groups, mask_mode, with_dy2):
    """dx, g, dgamma, dbeta, k1 / k2 / k3 and the abs-max bound of the formula, all in float64."""
    M = rows // groups
    dy, x = inp["dy"].double().reshape(rows, C), inp["x"].double().reshape(rows, C)
    g = dy + inp["dy2"].double().reshape(rows, C) if with_dy2 else dy.clone()
    if mask_mode == "bytes":      # bit j of byte i = element 4 i + j
        bits = (inp["mask"].to(torch.int64).reshape(-1, 1) >> torch.arange(4)) & 1
        g = g * bits.reshape(rows, C).double()
    elif mask_mode == "relu_out":
        g = g * (inp["relu_out"].reshape(rows, C) > 0).double()
    stats = inp["stats"].double().reshape(groups, 4, C)
    gamma = inp["gamma"].double()
    dx = torch.empty(rows, C, dtype=torch.float64)
    k = torch.empty(groups, 3, C, dtype=torch.float64)
    dgamma, dbeta = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    bounds = []
    for gi in range(groups):
        sl = slice(gi * M, (gi + 1) * M)
        mean, invstd = stats[gi, 2], stats[gi, 3]
        xh = (x[sl] - mean) * invstd
        db, dg = g[sl].sum(0), (g[sl] * xh).sum(0)
        k[gi, 0], k[gi, 1], k[gi, 2] = gamma * invstd, db / M, dg / M
        dx[sl] = k[gi, 0] * (g[sl] - k[gi, 1] - xh * k[gi, 2])
        dbeta += db
        dgamma += dg
        bounds.append(k[gi, 0].abs() * (g[sl].abs().amax(0) + k[gi, 1].abs() + xh.abs().amax(0) * k[gi, 2].abs()))
    return {"dx": dx, "g": g, "dgamma": dgamma, "dbeta": dbeta, "k": k, "bound": float(torch.stack(bounds).max()),
            "bound_without_last_group": float(torch.stack(bounds[:-1]).max()) if groups > 1 else 0.0}


def bn_run(L, dev, inp, C, rows, groups, out_mode, mask_mode, with_dy2, with_gout, absmax0=0.0):
    """One dcn_bn_backward_full call; everything it wrote as CPU tensors (0x5A-prefilled, so an element left out shows)."""
    lib = L.get()
    d = {k: v.to(dev) for k, v in inp.items()}
    u8 = lambda nbytes: torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    rq = (rows + 3) // 4
    out = {"dgamma": u8(4 * C), "dbeta": u8(4 * C)}
    if out_mode != "hl_only":
        out["dx"] = u8(4 * rows * C)
    if with_gout:
        out["g_out"] = u8(4 * rows * C)
    if out_mode in ("blocked", "hl_blocked_keep"):
        out["dq"] = u8(4 * C * rq * 4)
    if out_mode in ("hl_only", "hl_blocked_keep"):
        out["hl"] = u8(4 * rows * C)
    absmax = torch.full((1,), float(absmax0), device=dev)
    ws_bytes = lib.dcn_bn_backward_full_workspace(rows, C, groups)
    assert ws_bytes > 0
    ws = u8(ws_bytes)
    P = lambda t: L.ptr(t) if t is not None else None
    rc = lib.dcn_bn_backward_full(P(d["dy"]), P(d["dy2"]) if with_dy2 else None, P(d["relu_out"]) if mask_mode == "relu_out" else None,
                                  P(d["mask"]) if mask_mode == "bytes" else None, P(d["x"]), P(d["stats"]), P(d["gamma"]), C, rows,
                                  groups, P(out["dgamma"]), P(out["dbeta"]), P(out.get("dx")), P(out.get("g_out")), P(absmax),
                                  P(out.get("dq")), P(out.get("hl")), 1 if out_mode == "hl_blocked_keep" else 0, P(ws), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    res = {k_: v.cpu() for k_, v in out.items()}
    for k_ in ("dgamma", "dbeta", "dx", "g_out"):
        if k_ in res:
            res[k_] = res[k_].view(torch.float32)
    res["k"] = ws[ws_bytes - 4 * groups * 3 * C:].cpu().view(torch.float32).reshape(groups, 3, C)
    res["absmax"] = absmax.cpu()
    return res


def decode_blocked(dq_bytes, rq, C):
    """dq [m/4][4 sub-planes][C/4][2 channels x 4 pixels] fp16 (hi pairs, then lo pairs) -> (hi, lo) float32 [4 rq][C], as
    test_conv_f16x3_forward_dgrad decodes dcn_split_grad_blocked_f16."""
    t = dq_bytes.view(torch.float16).reshape(rq, 4, C // 4, 2, 4).float()
    unblock = lambda v: v.permute(0, 4, 2, 1, 3).reshape(rq * 4, C)       # [rq][2 pairs][C/4][2][4 px] -> [pixel][channel]
    return unblock(t[:, :2]), unblock(t[:, 2:])


def _hold_bn(res, ref, C, rows, groups, out_mode, what):
    k = ref["k"]
    for name, got, want in (("dgamma", res["dgamma"], ref["dgamma"]), ("dbeta", res["dbeta"], ref["dbeta"]),
                            ("k1", res["k"][:, 0], k[:, 0]), ("k2", res["k"][:, 1], k[:, 1]), ("k3", res["k"][:, 2], k[:, 2])):
        e = rel_err(got, want)
        assert e < BN_TOL, (name, e, what)
    if "dx" in res:
        e = rel_err(res["dx"].reshape(rows, C), ref["dx"])
        assert e < BN_TOL, ("dx", e, what)
    if "g_out" in res:
        e = rel_err(res["g_out"].reshape(rows, C), ref["g"])
        assert e < BN_TOL, ("g_out", e, what)
    am = float(res["absmax"])
    true_max = float(ref["dx"].abs().max())
    assert am >= true_max * GE, ("absmax below max |dx|", am, true_max, what)
    assert abs(am - ref["bound"]) <= BN_TOL * ref["bound"], ("absmax vs the formula", am, ref["bound"], what)
    if groups > 1:   # the planted last group carries the maximum: a bound that skipped it would fail the line above
        assert ref["bound_without_last_group"] < ref["bound"] * 0.5
    if out_mode == "plain":
        return
    s = 2.0 ** torch.floor(torch.log2(4096.0 / res["absmax"].double()))
    dev_dx = res["dx"].reshape(rows, C) if "dx" in res else None
    images = []
    if "hl" in res:
        images.append(("hl",) + hl32_decode(res["hl"].view(torch.float32), rows, C))
    if "dq" in res:
        rq = (rows + 3) // 4
        hi, lo = decode_blocked(res["dq"], rq, C)
        if rq * 4 > rows:   # rows past `rows` of the ragged last 4-row block: exactly zero
            assert float(hi[rows:].abs().max()) == 0.0 and float(lo[rows:].abs().max()) == 0.0, what
        images.append(("dq", hi[:rows], lo[:rows]))
    for name, hi, lo in images:
        assert float(hi.abs().max()) <= 4096.0, (name, float(hi.abs().max()), what)
        rec = (hi.double() + lo.double()) / s
        if dev_dx is not None:
            e = rel_err(rec, dev_dx)
            assert e < SPLIT_TOL, (name, e, what)
        else:             # hl_only: no fp32 dx is kept
            e = rel_err(rec, ref["dx"])
            assert e < BN_TOL, (name, e, what)


def bn_combos(C):
    """(out_mode, mask_mode, dy2, g_out): every output mode the channel count allows with every mask mode; dy2 and g_out
    alternate so that each is seen on and off with every output mode and every mask mode."""
    modes = OUT_MODES if C % 32 == 0 else ("plain", "blocked")
    for i, om in enumerate(modes):
        for j, mm in enumerate(MASK_MODES):
            yield om, mm, (i + j) % 2 == 0, (i + 2 * j) % 3 != 1


def check_bn_backward_full_vs_float64(L, dev, set_env, C, rows, groups, combos=None):
    """dcn_bn_backward_full -- the engine's batch-norm backward -- against the formula in float64 under every kernel-variant
    setting (full width, the default lean depth, one row in flight)."""
    inp = bn_inputs(C, rows, groups, seed=C + rows)
    picked = list(bn_combos(C)) if combos is None else combos
    refs = {}
    for setting in BN_SETTINGS:        # (the depth is set last: set_env cannot take a variable away again)
        set_env(**setting)
        for om, mm, d2, go in picked:
            if (mm, d2) not in refs:
                refs[(mm, d2)] = bn_reference(inp, C, rows, groups, mm, d2)
            ref = refs[(mm, d2)]
            what = (setting, om, mm, d2, go, C, rows, groups)
            res = bn_run(L, dev, inp, C, rows, groups, om, mm, d2, go)
            _hold_bn(res, ref, C, rows, groups, om, what)
            if om == "blocked" and mm == "bytes":      # a word pre-set above the bound stays
                big = 8.0 * ref["bound"]
                res2 = bn_run(L, dev, inp, C, rows, groups, om, mm, d2, go, absmax0=big)
                assert float(res2["absmax"]) == float(torch.tensor(big, dtype=torch.float32)), what


# ------------------------------------------------------------------------------------------------ 4. engine activation slots
class _Tap:
    """Forward hooks on an oracle: the output of every convolution, batch norm and block, one list entry per forward call."""

    def __init__(self, model):
        self.net = getattr(model, model._attr)
        self.conv, self.bn, self.block, self.hooks = {}, {}, {}, []
        for name, mod in self.net.named_modules():
            if isinstance(mod, torch.nn.Conv2d):
                self._hook(mod, self.conv, name)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                self._hook(mod, self.bn, name)
            elif hasattr(mod, "downsample"):
                self._hook(mod, self.block, name)

    def _hook(self, mod, store, name):
        self.hooks.append(mod.register_forward_hook(lambda m_, i_, out: store.setdefault(name, []).append(out.detach())))

    def remove(self):
        for h in self.hooks:
            h.remove()

    def bn_bound(self, conv, bn):
        """max over groups (forward calls) and channels of |gamma invstd| max|conv out| + |beta - mean gamma invstd|, batch
        statistics, in the oracle's own precision."""
        mod = self.net.get_submodule(bn)
        best = 0.0
        for y in self.conv[conv]:
            mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
            sc = mod.weight.detach() / torch.sqrt(var + mod.eps)
            b = sc.abs() * y.abs().amax((0, 2, 3)) + (mod.bias.detach() - mean * sc).abs()
            best = max(best, float(b.max()))
        return best

    def slots(self, x_max):
        """[(name, max |true activation|, bound formula, engine line that writes it in eval mode or None)] in the order of
        build_plan (csrc/backbone_engine.hip): image, stem activation, then per block its mid activations, its output and its
        downsample branch."""
        amax = lambda ts: max(float(t.abs().max()) for t in ts)
        relu_max = lambda ts: max(float(torch.relu(t).max()) for t in ts)
        out = [("image", x_max, x_max, True), ("stem", relu_max(self.bn["bn1"]), self.bn_bound("conv1", "bn1"), True)]
        prev = 1
        for bname in self.block:
            blk = self.net.get_submodule(bname)
            nconv = 3 if hasattr(blk, "conv3") else 2
            for i in range(1, nconv):
                out.append(("%s.mid%d" % (bname, i), relu_max(self.bn["%s.bn%d" % (bname, i)]),
                            self.bn_bound("%s.conv%d" % (bname, i), "%s.bn%d" % (bname, i)), True))
            last = self.bn_bound("%s.conv%d" % (bname, nconv), "%s.bn%d" % (bname, nconv))
            if blk.downsample is not None:
                down = self.bn_bound(bname + ".downsample.0", bname + ".downsample.1")
                res = down
            else:
                res = out[prev][2]
            out.append((bname + ".out", amax(self.block[bname]), last + res, True))
            prev = len(out) - 1
            if blk.downsample is not None:
                # eval mode never writes this slot: conv_fused(dc, in, nullptr, 0, R.S(dc.x), -1) in forward_impl -- the branch's
                # output is read by the block's last fused epilogue as `add`, never by a convolution as an operand
                out.append((bname + ".down", amax(self.bn[bname + ".downsample.1"]), down, False))
        return out


@functools.lru_cache(maxsize=None)
def _slot_run(dev, arch, pair, size):
    """The engine's slots (f16x3) and the oracles' figures for them, train mode and -- single call only -- eval mode after two
    train calls: {"train" | "eval": (slots, float64 figures, float32 figures)}.  Run once per (arch, pair), shared by the checks."""
    from dcn_hip import backbone
    backbone.set_conv_mode("f16x3")
    try:
        m, o = build_pair(arch, 3, 8)
        o64 = copy.deepcopy(o).double()
        m = m.to(dev)
        g = torch.Generator().manual_seed(5)
        H, W = size
        xs = [torch.randn(2, 3, H, W, generator=g) * 3]
        if pair:
            xs.append(torch.randn(2, 3, H, W, generator=g) * 0.4 + 0.2)
        x_max = max(float(x.abs().max()) for x in xs)

        def oracle_slots(model, dtype):
            tap = _Tap(model)
            with torch.no_grad():
                for x in xs:
                    model(x.to(dtype))
            tap.remove()
            return tap.slots(x_max)

        def engine_slots():
            with torch.no_grad():
                if pair:
                    m.forward_pair(xs[0].to(dev), xs[1].to(dev))
                    assert m._last_plan.groups == 2, "forward_pair fell back to two calls: the grouped launch is not exercised"
                else:
                    m(xs[0].to(dev))
            amax, status = m.last_forward_status()
            assert int(status) == 0                                                     # status word 0 throughout
            return amax.cpu().double()

        m.train(); o.train(); o64.train()
        s32, s64 = oracle_slots(o, torch.float32), oracle_slots(o64, torch.float64)    # (also the first train call of the oracles)
        res = {"x_max": x_max, "train": (engine_slots(), s64, s32)}
        if not pair:
            engine_slots()                                                              # second train call: the running statistics move on
            # the running statistics are INPUTS of the eval-mode pass: the references take the engine's own fp32 buffers (as they
            # take its fp32 weights and image), so that the float64 figures are computed from the same fp32 inputs
            o.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
            o64 = copy.deepcopy(o).double()
            assert int(getattr(o, o._attr).bn1.num_batches_tracked) == 2
            m.eval(); o.eval(); o64.eval()
            s32, s64 = oracle_slots(o, torch.float32), oracle_slots(o64, torch.float64)
            res["eval"] = (engine_slots(), s64, s32)
        return res
    finally:
        backbone.set_conv_mode(None)


def _hold_slots(run, mode, what):
    amax, s64, s32 = run[mode]
    assert amax.numel() == len(s64), (amax.numel(), len(s64))
    for i, ((name, true64, form64, written), (_, true32, form32, _)) in enumerate(zip(s64, s32)):
        slot = float(amax[i])
        if mode == "eval" and not written:
            assert slot == 0.0, (what, i, name, slot)      # no eval-mode launch writes it: named in _Tap.slots with the engine line
            continue
        # train: the bound formula on the oracle's convolution outputs and statistics; eval: the maximum itself
        want64, want32 = (true64, true32) if mode == "eval" else (form64, form32)
        tol = 3.0 * abs(want32 - want64) + 1e-5 * want64
        print("%s slot %2d %-22s %.8g / true max %.8g = 1 %+.3e   (expected %.8g +- %.2g)"
              % (what, i, name, slot, true64, slot / true64 - 1.0, want64, tol))
        assert slot >= true64 * GE, (what, i, name, slot, true64, slot / true64 - 1.0)
        if i == 0:
            assert slot == run["x_max"], (what, slot, run["x_max"])          # the image: exact
        else:
            assert abs(slot - want64) <= tol, (what, i, name, slot, want64, tol)


def check_activation_slots(dev, arch, pair=False, size=(32, 40)):
    """Every abs-max slot of the engine (f16x3) against the float64 oracle.  Train mode: each slot >= max |true activation|
    (1 - 2^-20) and equal to the bound formula of bn_finalize_kernel evaluated in float64.  Eval mode (after two train calls;
    the oracles then take the engine's running statistics, the fp32 inputs of that pass): each slot the fused epilogue writes
    equals max |true activation| and satisfies the same >= condition -- measured slot / float64 maximum - 1 at worst -8.4e-7 on
    the emulation and -6.1e-7 on the MI355X (Resnet50_8s both), against the -9.5e-7 allowed; the float32 oracle's own maxima
    come out at -7.9e-7.  Tolerance of the equalities: 3 |float32 oracle - float64| + 1e-5, the project's way of bounding network
    quantities.  pair: forward_pair on two differently scaled batches (two groups)."""
    run = _slot_run(dev, arch, pair, size)
    _hold_slots(run, "train", "%s train%s" % (arch, " pair" if pair else ""))
    if not pair:
        _hold_slots(run, "eval", "%s eval" % arch)
