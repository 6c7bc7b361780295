"""Max pool, bilinear upsample (forward, backward, normalisation backward), the layout kernels and the small reductions around
them against float64 on the CPU, ties and planted extremes included (shared by test_emu_resample.py -- host emulation -- and
test_gpu_resample.py -- MI355X; not a test module).

These are the kernels of the "resample" profiling category (DCN_PROF_RESAMPLE) and their neighbours, in the variants the engine
launches by default: the pool that applies the stem's batch norm + ReLU on the way in and writes the sign mask, the pool backward
that sums two cotangents, the two-tensor upsample backward with its abs-max word, the image layout pass with its abs-max word.
Every output buffer is filled with 0x5A bytes (1.5e16 as a float, 90 as an argmax byte) before the call: an element the kernel
leaves out shows."""
import functools

import torch
import torch.nn.functional as F

from helpers import rel_err
from odd_size_checks import FWD_FLOOR
from range_checks import BN_SETTINGS, BN_TOL

EPS = 1e-5
UPSAMPLE_TOL = {"cpu": 3e-6, "cuda": 1e-5}     # test_upsample_forward_backward / test_upsample_kernels_vs_torch_cpu


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _bytes(nbytes, dev, value=0x5A):
    return torch.full((nbytes,), value, dtype=torch.uint8, device=dev)


def _floats(shape, dev):
    """A float32 tensor of `shape` whose bytes are all 0x5A."""
    numel = 1
    for s in shape:
        numel *= s
    return _bytes(4 * numel, dev).view(torch.float32).reshape(shape)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_values(got, want64, what):
    """got (float32) equals the float64 reference exactly: NaN in the same places, equal elsewhere (inf included)."""
    got = got.double()
    gn, wn = torch.isnan(got), torch.isnan(want64)
    assert torch.equal(gn, wn), (what, "NaN positions", int(gn.sum()), int(wn.sum()))
    assert torch.equal(torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want64), want64)), what


def _small_ints(shape, g, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------ a. max pool, exact
# (n, hin, win, c): odd and even sides, a side of 1, more than one 256-work-item block
POOL_SHAPES = [(2, 9, 7, 8), (1, 8, 10, 4), (1, 1, 1, 4), (1, 1, 6, 4), (1, 5, 1, 4), (2, 2, 2, 12), (3, 13, 11, 20)]
POOL_KINDS = ("ties", "relu", "neg", "neg_inf", "nan")


def pool_data(kind, shape, seed=0):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed + 1000 * h + w)
    if kind == "ties":
        return torch.randint(0, 3, shape, generator=g).float()
    if kind == "relu":                                   # the network's case: most windows tie at 0, border windows are all ties
        return torch.relu(torch.randn(shape, generator=g))
    if kind == "neg":                                    # a zero padding value would win every border window
        return -(torch.rand(shape, generator=g) + 0.25)
    if kind == "neg_inf":
        return torch.full(shape, float("-inf"))
    if kind == "nan":                                    # about 2 % NaN and a few +-inf, the first and the last element among them
        x = torch.randn(shape, generator=g)
        x[torch.rand(shape, generator=g) < 0.02] = float("nan")
        flat = x.reshape(-1)
        flat[torch.randint(0, flat.numel(), (3,), generator=g)] = float("inf")
        flat[torch.randint(0, flat.numel(), (3,), generator=g)] = float("-inf")
        flat[0] = float("nan")
        flat[-1] = float("nan") if flat.numel() > 4 else float("inf")
        return x
    raise ValueError(kind)


def pool_reference(x):
    """F.max_pool2d in float64 on the CPU: pooled values [n,ho,wo,c] and the window tap 0..8 of every maximum.  ATen keeps the
    first maximum in row-major window order, lets a NaN win and a later NaN replace an earlier one, and reports the first
    in-bounds element of a window that is -inf throughout: the kernel's rules."""
    n, h, w, c = x.shape
    y, idx = F.max_pool2d(x.double().permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    ho, wo = y.shape[2:]
    iy, ix = idx // w, idx % w
    oy = torch.arange(ho).reshape(1, 1, ho, 1)
    ox = torch.arange(wo).reshape(1, 1, 1, wo)
    tap = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 8
    return y.permute(0, 2, 3, 1).contiguous(), tap.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def pool_scatter(g64, tap, hin, win):
    """Gradient of the pool's input from the gradient of its output g64 [n,ho,wo,c] and the taps (float64, exact for small
    integers): what autograd does with the indices."""
    n, ho, wo, c = g64.shape
    t = tap.to(torch.int64)
    iy = 2 * torch.arange(ho).reshape(1, ho, 1, 1) - 1 + t // 3
    ix = 2 * torch.arange(wo).reshape(1, 1, wo, 1) - 1 + t % 3
    assert int(iy.min()) >= 0 and int(iy.max()) < hin and int(ix.min()) >= 0 and int(ix.max()) < win
    flat = ((torch.arange(n).reshape(n, 1, 1, 1) * hin + iy) * win + ix) * c + torch.arange(c).reshape(1, 1, 1, c)
    gin = torch.zeros(n * hin * win * c, dtype=torch.float64)
    gin.index_add_(0, flat.reshape(-1), g64.reshape(-1))
    return gin.reshape(n, hin, win, c)


def run_pool_forward(L, dev, x, full, stats=None, groups=1, with_mask=False):
    """(out, argmax[, mask]) as CPU tensors from dcn_maxpool_forward (full False) or dcn_maxpool_forward_full."""
    lib = L.get()
    n, h, w, c = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    xd = x.to(dev).contiguous()
    sd = stats.to(dev).contiguous() if stats is not None else None
    out = _floats((n, ho, wo, c), dev)
    am = _bytes(n * ho * wo * c, dev)
    mask = _bytes(n * h * w * c // 4, dev, 0xFF) if with_mask else None
    if full:
        rc = lib.dcn_maxpool_forward_full(L.ptr(xd), L.ptr(sd), groups, n, h, w, c, L.ptr(out), L.ptr(am), L.ptr(mask), L.stream_ptr())
    else:
        rc = lib.dcn_maxpool_forward(L.ptr(xd), n, h, w, c, L.ptr(out), L.ptr(am), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    res = (out.cpu(), am.cpu().reshape(n, ho, wo, c))
    return res + (mask.cpu(),) if with_mask else res


def run_pool_backward(L, dev, gout, gout2, argmax, shape, full):
    lib = L.get()
    n, h, w, c = shape
    gd = gout.to(dev).contiguous()
    g2 = gout2.to(dev).contiguous() if gout2 is not None else None
    ad = argmax.to(dev).contiguous()
    gin = _floats(shape, dev)
    if full:
        rc = lib.dcn_maxpool_backward_full(L.ptr(gd), L.ptr(g2), L.ptr(ad), n, h, w, c, L.ptr(gin), L.stream_ptr())
    else:
        assert gout2 is None
        rc = lib.dcn_maxpool_backward(L.ptr(gd), L.ptr(ad), n, h, w, c, L.ptr(gin), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    return gin.cpu()


def check_maxpool_exact(L, dev, shape, kind):
    """Pooled values, every argmax byte and -- small-integer cotangents, every sum exact -- the backward gather, each equal to
    F.max_pool2d / autograd in float64; the plain entry points and the _full ones with their options null."""
    n, h, w, c = shape
    x = pool_data(kind, shape)
    if kind == "neg":
        assert float(x.max()) < 0.0
    want, tap = pool_reference(x)
    for full in (False, True):
        out, am = run_pool_forward(L, dev, x, full)
        _same_values(out, want, (shape, kind, full, "pooled values"))
        assert torch.equal(am, tap), (shape, kind, full, "argmax", int((am != tap).sum()))
    if kind == "nan":
        return
    g = torch.Generator().manual_seed(7 + h)
    g1, g2 = _small_ints(want.shape, g), _small_ints(want.shape, g)
    # autograd's own gradient in float64 (its indices are the taps just compared)
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y64 = F.max_pool2d(x64, 3, 2, 1)
    ref1, = torch.autograd.grad(y64, x64, g1.double().permute(0, 3, 1, 2), retain_graph=True)
    ref12, = torch.autograd.grad(y64, x64, (g1 + g2).double().permute(0, 3, 1, 2))
    ref1, ref12 = ref1.permute(0, 2, 3, 1), ref12.permute(0, 2, 3, 1)
    assert torch.equal(ref1, pool_scatter(g1.double(), tap, h, w))
    for full in (False, True):
        gin = run_pool_backward(L, dev, g1, None, am, shape, full)
        assert torch.equal(gin.double(), ref1), (shape, kind, full, "gin")
    gin = run_pool_backward(L, dev, g1, g2, am, shape, True)
    assert torch.equal(gin.double(), ref12), (shape, kind, "gin of gout + gout2")


def check_pool_argument_checks(L, dev):
    """DCN_E_INVALID like the neighbours: null required pointers, c % 4, groups outside {1, 2}, n % groups, ldl < d."""
    lib = L.get()
    t = torch.zeros(4096, device=dev)
    b = torch.zeros(4096, dtype=torch.uint8, device=dev)
    P, S = L.ptr, L.stream_ptr()
    assert lib.dcn_maxpool_forward_full(None, None, 1, 1, 4, 4, 4, P(t), P(b), None, S) == -1
    assert lib.dcn_maxpool_forward_full(P(t), None, 1, 1, 4, 4, 6, P(t), P(b), None, S) == -1
    assert lib.dcn_maxpool_forward_full(P(t), P(t), 3, 3, 4, 4, 4, P(t), P(b), None, S) == -1
    assert lib.dcn_maxpool_forward_full(P(t), P(t), 2, 3, 4, 4, 4, P(t), P(b), None, S) == -1
    assert lib.dcn_maxpool_forward_full(P(t), None, 1, 1, 4, 4, 4, P(t), P(b), P(b), S) == -1     # a mask without statistics
    assert lib.dcn_maxpool_backward_full(P(t), None, None, 1, 4, 4, 4, P(t), S) == -1
    assert lib.dcn_maxpool_backward_full(P(t), None, P(b), 1, 4, 4, 6, P(t), S) == -1
    assert lib.dcn_normalize_backward(P(t), 1, 2, 2, 2, 3, 4, 4, P(t), P(t), S) == -1               # ldl < d
    assert lib.dcn_normalize_backward(P(t), 1, 2, 2, 4, 3, 4, 4, None, P(t), S) == -1
    assert lib.dcn_upsample_backward_full(P(t), None, 1, 2, 2, 2, 3, 4, 4, P(t), P(t), None, S) == -1
    assert lib.dcn_upsample_backward_full(P(t), P(t), 3, 2, 2, 4, 3, 4, 4, P(t), P(t), None, S) == -1   # two halves of an odd batch
    assert lib.dcn_image_to_nhwc4(None, 1, 4, P(t), None, S) == -1
    assert lib.dcn_pad_c3_to_c4(P(t), None, 4, S) == -1 and lib.dcn_unpad_c4_to_c3(None, P(t), 4, S) == -1
    assert lib.dcn_pad_rows(P(t), P(t), 4, 5, 4, S) == -1
    assert lib.dcn_column_sums(P(t), 4, 4, 5, P(t), S) == -1 and lib.dcn_column_sums(None, 4, 4, 3, P(t), S) == -1
    _sync(dev)


# ------------------------------------------------------------------------------------------------ b. / c. the stem tail
# (n, groups, hin, win, c)
STEM_SHAPES = [(2, 1, 9, 7, 8), (2, 2, 9, 7, 8), (2, 2, 3, 2, 4), (4, 2, 12, 10, 64)]


@functools.lru_cache(maxsize=None)
def stem_problem(shape, seed=0):
    """A convolution output with per-channel scale and offset; with two groups the second batch is scaled and shifted
    differently, so that group 0's statistics applied to group 1 cannot pass."""
    n, groups, h, w, c = shape
    g = torch.Generator().manual_seed(seed + 31 * h + c)
    ch = torch.arange(c)
    x = torch.randn(n, h, w, c, generator=g) * (0.5 + 0.5 * (ch % 5)) + 0.4 * (ch % 3 - 1.0)
    if groups == 2:
        x[n // 2:] = x[n // 2:] * 2.5 + 1.5
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.2
    ho, wo = (h + 1) // 2, (w + 1) // 2
    g1 = torch.randn(n, ho, wo, c, generator=g)
    g2 = 0.5 * torch.randn(n, ho, wo, c, generator=g)
    return {"x": x.contiguous(), "gamma": gamma, "beta": beta, "g1": g1, "g2": g2}


def stem_unfused(L, dev, shape, x, gamma, beta, x_stats=None):
    """Per group dcn_bn_forward(relu = 1) from partial sums built in float64 (one tile per group = the group's column sums, the
    pattern of kernel_checks.check_dgrad_with_bn_backward): y, mask, stats as CPU tensors.  x_stats: the tensor the statistics
    are made from when it is not x itself."""
    lib = L.get()
    n, groups, h, w, c = shape
    rows = n * h * w
    rpg = rows // groups
    t = lambda a: a.to(dev).contiguous()
    xd, gd, bd = t(x), t(gamma), t(beta)
    stats = _floats((groups, 4, c), dev)
    y = _floats((rows, c), dev)
    mask = _bytes(rows * c // 4, dev, 0xFF)
    keep = []
    for gi in range(groups):
        xg = (x if x_stats is None else x_stats).double().reshape(groups, rpg, c)[gi]
        part = t(torch.stack([xg.sum(0), (xg ** 2).sum(0), xg.abs().amax(0)]).float().reshape(1, 3, c))
        keep.append(part)
        rc = lib.dcn_bn_forward(L.ptr(xd.reshape(groups, rpg, c)[gi]), L.ptr(part), 1, c, rpg, L.ptr(gd), L.ptr(bd), None, None,
                                0.1, EPS, 1, None, 1, L.ptr(y[gi * rpg:]), L.ptr(mask[gi * rpg * c // 4:]), L.ptr(stats[gi]),
                                L.stream_ptr())
        assert rc == 0, rc
    _sync(dev)
    return y.cpu().reshape(n, h, w, c), mask.cpu(), stats.cpu()


def stem_bn64(shape, x, gamma, beta):
    """Train-mode batch norm per group in float64: (pre-activation, mean, invstd)."""
    n, groups, h, w, c = shape
    xg = x.double().reshape(groups, -1, c)
    mean = xg.mean(1, keepdim=True)
    invstd = 1.0 / torch.sqrt(xg.var(1, unbiased=False, keepdim=True) + EPS)
    pre = (xg - mean) * invstd * gamma.double() + beta.double()
    return pre.reshape(n, h, w, c), mean.reshape(groups, c), invstd.reshape(groups, c)


def plant_non_finite(x):
    """NaN and +-inf in border rows and columns, in the interior, in both halves of the batch."""
    n, h, w, c = x.shape
    x = x.clone()
    nan, inf = float("nan"), float("inf")
    x[0, 0, 0, 0] = nan
    x[0, h - 1, w - 1, c - 1] = inf
    x[0, 0, w - 1, 1] = -inf
    x[n - 1, h - 1, 0, 2] = nan
    x[n - 1, h // 2, w // 2, 3] = inf
    x[n - 1, 0, w // 2, 0] = -inf
    x[n - 1, h // 2, 0, c - 1] = nan
    return x


def check_stem_pool_fused(L, dev, shape):
    """maxpool_fwd_kernel with scale / shift (the engine's default, DCN_STEM_POOL_FUSED=1) against the apply pass followed by the
    plain pool: pooled output, argmax bytes and all rows * C / 4 mask bytes bit for bit; again with NaN / +-inf planted in x after
    the statistics were made (both paths turn a NaN into 0 through fmaxf).  The unfused y itself against float64 at 1e-5."""
    n, groups, h, w, c = shape
    P = stem_problem(shape)
    y, mask, stats = stem_unfused(L, dev, shape, P["x"], P["gamma"], P["beta"])
    pre, _, _ = stem_bn64(shape, P["x"], P["gamma"], P["beta"])
    e = rel_err(y, torch.relu(pre))
    assert e < 1e-5, (shape, "unfused y", e)
    if groups == 2:                                  # the groups' statistics differ by far more than any tolerance
        assert rel_err(stats[0, 2], stats[1, 2]) > 0.1 and rel_err(stats[0, 0], stats[1, 0]) > 0.1
    for planted in (False, True):
        x = plant_non_finite(P["x"]) if planted else P["x"]
        if planted:                                  # same statistics: they were made before the values were planted
            y, mask, stats2 = stem_unfused(L, dev, shape, x, P["gamma"], P["beta"], x_stats=P["x"])
            assert torch.equal(_bits(stats2), _bits(stats))
        out_u, am_u = run_pool_forward(L, dev, y, False)
        out_f, am_f, mask_f = run_pool_forward(L, dev, x, True, stats=stats, groups=groups, with_mask=True)
        assert not bool(torch.isnan(out_u).any()) and not bool(torch.isnan(out_f).any())
        assert torch.equal(out_f, out_u), (shape, planted, "pooled", int((out_f != out_u).sum()), rel_err(out_f, out_u))
        assert torch.equal(am_f, am_u), (shape, planted, "argmax", int((am_f != am_u).sum()))
        assert torch.equal(mask_f, mask), (shape, planted, "mask", int((mask_f != mask).sum()))
        bits = (y.reshape(-1, 4) > 0).to(torch.uint8)
        assert torch.equal(mask, bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | (bits[:, 3] << 3))


def _mask_bits(mask, shape4):
    return ((mask.to(torch.int64).reshape(-1, 1) >> torch.arange(4)) & 1).reshape(shape4)


def check_stem_chain(L, dev, set_env, shape):
    """x -> BN (train, per group) -> ReLU -> pool and back with two cotangents of the pooled tensor: dcn_maxpool_forward_full,
    dcn_maxpool_backward_full(g1, g2), dcn_bn_backward_full(relu_mask = the pool's mask) against float64 at BN_TOL, under every
    batch-norm backward variant.  The float64 formula is evaluated with the device's own mask and argmax (an element within
    round-off of the kink or of a tie cannot flip the comparison); where those equal the float64 ones, also plain autograd."""
    lib = L.get()
    n, groups, h, w, c = shape
    rows = n * h * w
    P = stem_problem(shape)
    x, gamma, beta, g1, g2 = P["x"], P["gamma"], P["beta"], P["g1"], P["g2"]
    _, _, stats = stem_unfused(L, dev, shape, x, gamma, beta)
    out, am, mask = run_pool_forward(L, dev, x, True, stats=stats, groups=groups, with_mask=True)
    gin = run_pool_backward(L, dev, g1, g2, am, (n, h, w, c), True)
    # ---- float64 with the device's mask and argmax
    pre, mean, invstd = stem_bn64(shape, x, gamma, beta)
    m_dev = _mask_bits(mask, (n, h, w, c)).double()
    gin64 = pool_scatter(g1.double() + g2.double(), am, h, w)
    e = rel_err(gin, gin64)
    assert e < 1e-6, (shape, "gin", e)                                        # one float32 addition per element
    gm = (gin64 * m_dev).reshape(groups, -1, c)
    xhat = (x.double().reshape(groups, -1, c) - mean.unsqueeze(1)) * invstd.unsqueeze(1)
    M = rows // groups
    db, dg = gm.sum(1), (gm * xhat).sum(1)
    dx64 = ((gamma.double() * invstd).unsqueeze(1) * (gm - db.unsqueeze(1) / M - xhat * dg.unsqueeze(1) / M)).reshape(rows, c)
    dgamma64, dbeta64 = dg.sum(0), db.sum(0)
    # ---- plain float64 autograd, comparable when nothing sat on the kink or on a tie
    x64 = x.double().requires_grad_(True)
    gam64, bet64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ys = [F.batch_norm(x64.reshape(groups, -1, c)[gi], None, None, gam64, bet64, True, 0.1, EPS) for gi in range(groups)]
    y64 = torch.relu(torch.stack(ys).reshape(n, h, w, c))
    p64, idx = F.max_pool2d(y64.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    p64.backward((g1.double() + g2.double()).permute(0, 3, 1, 2))
    want_out, want_tap = pool_reference(y64.detach())
    e = rel_err(out, want_out)
    assert e < 1e-5, (shape, "pooled", e)
    same = torch.equal(m_dev, (y64.detach() > 0).double()) and torch.equal(am, want_tap)
    print("stem chain %s: mask and argmax %s the float64 ones" % (shape, "equal" if same else "differ from"))
    ta = lambda a: a.to(dev).contiguous()
    xd, sd, gd, gind, md = ta(x), ta(stats), ta(gamma), ta(gin), ta(mask)
    ws_bytes = lib.dcn_bn_backward_full_workspace(rows, c, groups)
    assert ws_bytes > 0
    for setting in BN_SETTINGS:
        set_env(**setting)
        dgam, dbet, dx = _floats((c,), dev), _floats((c,), dev), _floats((rows, c), dev)
        ws = _bytes(ws_bytes, dev)
        rc = lib.dcn_bn_backward_full(L.ptr(gind), None, None, L.ptr(md), L.ptr(xd), L.ptr(sd), L.ptr(gd), c, rows, groups,
                                      L.ptr(dgam), L.ptr(dbet), L.ptr(dx), None, None, None, None, 1, L.ptr(ws), L.stream_ptr())
        assert rc == 0, rc
        _sync(dev)
        for name, got, want, auto in (("dx", dx, dx64, x64.grad.reshape(rows, c)), ("dgamma", dgam, dgamma64, gam64.grad),
                                      ("dbeta", dbet, dbeta64, bet64.grad)):
            e = rel_err(got.cpu(), want)
            assert e < BN_TOL, (shape, setting, name, e)
            if same:
                e = rel_err(got.cpu(), auto)
                assert e < BN_TOL, (shape, setting, name, "autograd", e)
    return same


# ------------------------------------------------------------------------------------------------ d. upsample
# (hl, wl, h, w): (h - 1) / (hl - 1) and (w - 1) / (wl - 1) are powers of two -- every interpolation weight is a multiple of 1 / 8
# and exact in float32, so with small-integer data every product and every sum is exact
UPSAMPLE_EXACT = [(3, 2, 9, 9), (5, 3, 17, 9), (2, 5, 9, 17)]
UPSAMPLE_DIMS = (3, 5, 16)
# (n, hl, wl, d, h, w): test_upsample_kernels_vs_torch_cpu's small cases and the emulation suite's
UPSAMPLE_INEXACT = [(1, 1, 1, 3, 8, 8), (1, 1, 2, 4, 8, 13), (2, 4, 1, 5, 29, 8), (1, 6, 8, 5, 41, 59), (2, 4, 5, 3, 32, 40)]


def _pad_channels(low_nhwc, ld):
    """[n,hl,wl,d] -> [n,hl,wl,ld]; the pad channels hold a value no output may pick up."""
    n, hl, wl, d = low_nhwc.shape
    lowp = torch.full((n, hl, wl, ld), 777.0)
    lowp[..., :d] = low_nhwc
    return lowp


def run_upsample_forward(L, dev, lowp, d, h, w, normalize):
    lib = L.get()
    n, hl, wl, ld = lowp.shape
    ld_ = lowp.to(dev).contiguous()
    out = _floats((n, h, w, d), dev)
    rc = lib.dcn_upsample_forward(L.ptr(ld_), n, hl, wl, ld, d, h, w, normalize, L.ptr(out), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    return out.cpu()


def run_upsample_backward(L, dev, gout, hl, wl, ld, full=False, gout_b=None, absmax0=None):
    """glow [n,hl,wl,ld] (and the abs-max word) from dcn_upsample_backward / dcn_upsample_backward_full; n counts both halves."""
    lib = L.get()
    nh, h, w, d = gout.shape
    n = nh * (2 if gout_b is not None else 1)
    gd = gout.to(dev).contiguous()
    gb = gout_b.to(dev).contiguous() if gout_b is not None else None
    glow = _floats((n, hl, wl, ld), dev)
    tmp = _bytes(lib.dcn_upsample_backward_tmp_bytes(n, hl, w, d), dev)
    am = torch.full((1,), float(absmax0), device=dev) if absmax0 is not None else None
    if full:
        rc = lib.dcn_upsample_backward_full(L.ptr(gd), L.ptr(gb), n, hl, wl, ld, d, h, w, L.ptr(glow), L.ptr(tmp), L.ptr(am),
                                            L.stream_ptr())
    else:
        rc = lib.dcn_upsample_backward(L.ptr(gd), n, hl, wl, ld, d, h, w, L.ptr(glow), L.ptr(tmp), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    return (glow.cpu(), am.cpu()) if am is not None else glow.cpu()


def _interp64(low_nhwc, h, w):
    """(low as a float64 NCHW leaf, F.interpolate(align_corners=True) of it)"""
    low64 = low_nhwc.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    return low64, F.interpolate(low64, size=(h, w), mode="bilinear", align_corners=True)


def check_upsample_exact(L, dev, sizes, d):
    hl, wl, h, w = sizes
    n, ld = 2, (d + 3) // 4 * 4
    g = torch.Generator().manual_seed(d + h)
    low = _small_ints((n, hl, wl, d), g)
    gout = _small_ints((n, h, w, d), g)
    low64, ref = _interp64(low, h, w)
    ref.backward(gout.double().permute(0, 3, 1, 2))
    out = run_upsample_forward(L, dev, _pad_channels(low, ld), d, h, w, 0)
    assert torch.equal(out.double(), ref.detach().permute(0, 2, 3, 1)), (sizes, d, "forward")
    for full in (False, True):
        glow = run_upsample_backward(L, dev, gout, hl, wl, ld, full=full)
        assert torch.equal(glow[..., :d].double(), low64.grad.permute(0, 2, 3, 1)), (sizes, d, full, "backward")
        assert torch.equal(glow[..., d:], torch.zeros(n, hl, wl, ld - d)), (sizes, d, full, "pad channels")


def check_upsample_inexact(L, dev, shape):
    n, hl, wl, d, h, w = shape
    ld = (d + 3) // 4 * 4
    tol = UPSAMPLE_TOL[dev]
    g = torch.Generator().manual_seed(d)
    low = torch.randn(n, hl, wl, d, generator=g)
    gout = torch.randn(n, h, w, d, generator=g)
    low64, ref = _interp64(low, h, w)
    ref.backward(gout.double().permute(0, 3, 1, 2))
    v = ref.detach().permute(0, 2, 3, 1)
    lowp = _pad_channels(low, ld)
    e = rel_err(run_upsample_forward(L, dev, lowp, d, h, w, 0), v)
    assert e < tol, (shape, "forward", e)
    e = rel_err(run_upsample_forward(L, dev, lowp, d, h, w, 1), v / v.norm(2, 3, keepdim=True))
    assert e < tol, (shape, "normalised forward", e)
    glow = run_upsample_backward(L, dev, gout, hl, wl, ld)
    e = rel_err(glow[..., :d], low64.grad.permute(0, 2, 3, 1))
    assert e < tol, (shape, "backward", e)
    assert torch.equal(glow[..., d:], torch.zeros(n, hl, wl, ld - d)), (shape, "pad channels")
    # the weights of every output pixel sum to one: an all-ones gradient comes back as n h w per channel
    ones = run_upsample_backward(L, dev, torch.ones(n, h, w, d), hl, wl, ld)
    total = ones[..., :d].double().sum((0, 1, 2))
    worst = float((total / (n * h * w) - 1.0).abs().max())
    assert worst <= h * w * 2.0 ** -23, (shape, "sum of the weights", worst)


def check_upsample_backward_two_tensors(L, dev, shape):
    """gout_b (the engine's forward_pair path: two row-pass launches into the two halves of the intermediate): bit-equal to the
    single-tensor call on the concatenation."""
    n, hl, wl, d, h, w = shape
    assert n % 2 == 0
    ld = (d + 3) // 4 * 4
    g = torch.Generator().manual_seed(n + d)
    ga, gb = torch.randn(n // 2, h, w, d, generator=g), 3.0 * torch.randn(n // 2, h, w, d, generator=g)
    whole = run_upsample_backward(L, dev, torch.cat([ga, gb]), hl, wl, ld)
    whole_full = run_upsample_backward(L, dev, torch.cat([ga, gb]), hl, wl, ld, full=True)
    halves = run_upsample_backward(L, dev, ga, hl, wl, ld, full=True, gout_b=gb)
    assert torch.equal(_bits(whole_full), _bits(whole)), shape
    assert torch.equal(_bits(halves), _bits(whole)), (shape, rel_err(halves, whole))
    assert float(whole[n // 2:].abs().max()) > float(whole[:n // 2].abs().max())      # (the halves differ: a swap would show)


def check_upsample_backward_absmax(L, dev, shape):
    """absmax_kernel behind the column pass: the word's bits are max |glow|; a word pre-set above stays; a positive one below
    is raised."""
    n, hl, wl, d, h, w = shape
    ld = (d + 3) // 4 * 4
    g = torch.Generator().manual_seed(3 * d + h)
    gout = torch.randn(n, h, w, d, generator=g)
    gout[n - 1, h - 1, w - 1, d - 1] = -60.0                          # the largest |glow| is negative and in the last element
    plain = run_upsample_backward(L, dev, gout, hl, wl, ld)
    m = plain.abs().max().reshape(1)
    assert float(m) == -float(plain[n - 1, hl - 1, wl - 1, d - 1])
    for a0 in (0.0, 1.0e-3, 4.0 * float(m)):
        glow, am = run_upsample_backward(L, dev, gout, hl, wl, ld, full=True, absmax0=a0)
        assert torch.equal(_bits(glow), _bits(plain)), (shape, a0)
        want = m if a0 < float(m) else torch.tensor([a0], dtype=torch.float32)
        assert torch.equal(_bits(am), _bits(want)), (shape, a0, float(am), float(want))


# dcn_normalize_backward against float64 autograd of v / ||v||.  Tolerance: 3 x (torch's float32 evaluation of the same expression
# against float64, same inputs) + FWD_FLOOR, the project's convention.  Measured over D in {3, 5, 16} and the three shapes below:
#   float32 torch against float64        1.5e-7 ... 2.7e-7
#   normalize_bwd_kernel against float64 1.6e-7 ... 2.5e-7, the same figures on the host emulation and on the MI355X
NORMALIZE_SHAPES = [(1, 6, 8, 41, 59), (2, 4, 5, 32, 40), (2, 5, 3, 17, 9)]      # (n, hl, wl, h, w): two inexact, one exact
MIN_NORM = 0.5


def _normalize_problem(shape, d, seed=0):
    n, hl, wl, h, w = shape
    g = torch.Generator().manual_seed(seed + d + h)
    low = 0.4 * torch.randn(n, hl, wl, d, generator=g)
    low[..., 0] += 2.0                                                # keeps ||v|| away from zero (asserted by the caller)
    gout = torch.randn(n, h, w, d, generator=g)
    return low, gout


def _normalize_reference(low, gout, h, w, dtype):
    """d/dv of sum(gout * v / ||v||), v = the interpolated map of `low`, evaluated in `dtype`: (gv [n,h,w,d], min ||v||)."""
    lo = low.to(dtype).permute(0, 3, 1, 2).contiguous()
    v = F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=True).detach().requires_grad_(True)
    nrm = v.norm(2, 1, keepdim=True)
    (v / nrm).backward(gout.to(dtype).permute(0, 3, 1, 2))
    return v.grad.permute(0, 2, 3, 1), float(nrm.detach().min())


def run_normalize_backward(L, dev, lowp, gout, d):
    lib = L.get()
    n, hl, wl, ld = lowp.shape
    _, h, w, _ = gout.shape
    ld_, gd = lowp.to(dev).contiguous(), gout.to(dev).contiguous()
    gv = _floats((n, h, w, d), dev)
    rc = lib.dcn_normalize_backward(L.ptr(ld_), n, hl, wl, ld, d, h, w, L.ptr(gd), L.ptr(gv), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    return gv.cpu()


def check_normalize_backward(L, dev, shape, d):
    n, hl, wl, h, w = shape
    ld = (d + 3) // 4 * 4
    low, gout = _normalize_problem(shape, d)
    ref, min_norm = _normalize_reference(low, gout, h, w, torch.float64)
    assert min_norm > MIN_NORM, (shape, d, min_norm)                  # the condition on the inputs
    ref32, _ = _normalize_reference(low, gout, h, w, torch.float32)
    e32 = rel_err(ref32, ref)
    gv = run_normalize_backward(L, dev, _pad_channels(low, ld), gout, d)
    e = rel_err(gv, ref)
    print("normalize backward %s D=%d: kernel %.2e, float32 torch %.2e against float64" % (shape, d, e, e32))
    assert e < 3.0 * e32 + FWD_FLOOR, (shape, d, e, e32)
    return e, e32


def check_normalize_backward_one_channel(L, dev, shape):
    """D = 1: v / |v| is constant, the true gradient is 0; what is left is the round-off of 1 - y^2."""
    n, hl, wl, h, w = shape
    low, gout = _normalize_problem(shape, 1)
    _, min_norm = _normalize_reference(low, gout, h, w, torch.float64)
    assert min_norm > MIN_NORM
    gv = run_normalize_backward(L, dev, _pad_channels(low, 4), gout, 1)
    bound = 4.0 * 2.0 ** -24 * float(gout.abs().max()) / min_norm
    assert float(gv.abs().max()) <= bound, (shape, float(gv.abs().max()), bound)


def check_normalize_zero_cell(L, dev, d=3):
    """A 2 x 2 cell of `low` that is zero in every channel (exact shape: a pixel on the cell's border has exactly zero weight on
    the corners outside): forward output with normalize = 1 and gv are NaN exactly where float64 is, finite elsewhere."""
    shape = NORMALIZE_SHAPES[2]
    n, hl, wl, h, w = shape
    low, gout = _normalize_problem(shape, d)
    low[1, 1:3, 0:2, :] = 0.0
    ld = (d + 3) // 4 * 4
    low64, v = _interp64(low, h, w)
    v = v.detach().permute(0, 2, 3, 1)
    y64 = v / v.norm(2, 3, keepdim=True)
    ref, _ = _normalize_reference(low, gout, h, w, torch.float64)
    want = torch.isnan(y64)
    assert int(want.sum()) == 5 * 5 * d and torch.equal(torch.isnan(ref), want)          # rows 4 .. 8, columns 0 .. 4 of image 1
    lowp = _pad_channels(low, ld)
    out = run_upsample_forward(L, dev, lowp, d, h, w, 1)
    gv = run_normalize_backward(L, dev, lowp, gout, d)
    for name, got in (("forward", out), ("gv", gv)):
        assert torch.equal(torch.isnan(got), want), (name, int(torch.isnan(got).sum()))
        assert bool(torch.isfinite(got[~want]).all()), name


# ------------------------------------------------------------------------------------------------ e. layout, small reductions
GRID_CAP_PIXELS = 2048 * 256       # kGridCap * 256 (csrc/elementwise_kernels.hip): beyond it the grid-stride loop takes a second trip
IMAGE_SIZES = [(2, 35), (3, 700), (1, GRID_CAP_PIXELS + 257)]       # (n, pixels per image)


def run_image_to_nhwc4(L, dev, img, absmax0=0.0):
    lib = L.get()
    n, _, hw = img.shape
    im = img.to(dev).contiguous()
    out = _floats((n, hw, 4), dev)
    am = torch.full((1,), float(absmax0), device=dev) if absmax0 is not None else None
    rc = lib.dcn_image_to_nhwc4(L.ptr(im), n, hw, L.ptr(out), L.ptr(am), L.stream_ptr())
    assert rc == 0, rc
    _sync(dev)
    return out.cpu(), (am.cpu() if am is not None else None)


def check_image_to_nhwc4(L, dev, size):
    n, hw = size
    g = torch.Generator().manual_seed(hw)
    img = torch.randn(n, 3, hw, generator=g)
    img[n - 1, 2, hw - 1] = -9.5                     # the maximum: channel 2 of the last pixel of the last image
    want = torch.cat([img.permute(0, 2, 1), torch.zeros(n, hw, 1)], 2).contiguous()
    m = img.abs().max().reshape(1)
    assert float(m) == 9.5
    for a0 in (0.0, 1.0e-3, 100.0, None):
        out, am = run_image_to_nhwc4(L, dev, img, a0)
        assert torch.equal(_bits(out), _bits(want)), (size, a0)
        if a0 is not None:
            want_am = m if a0 < 9.5 else torch.tensor([a0], dtype=torch.float32)
            assert torch.equal(_bits(am), _bits(want_am)), (size, a0, float(am))
    for ch, pos in ((0, 0), (1, hw // 2), (2, hw - 1)):      # a NaN in any channel is reported as +inf (fmaxf would drop it)
        bad = img.clone()
        bad[n - 1, ch, pos] = float("nan")
        out, am = run_image_to_nhwc4(L, dev, bad, 0.0)
        assert float(am) == float("inf"), (size, ch, float(am))
        _same_values(out, torch.cat([bad.permute(0, 2, 1), torch.zeros(n, hw, 1)], 2).double(), (size, ch))


def check_pad_channels_round_trip(L, dev, rows):
    lib = L.get()
    g = torch.Generator().manual_seed(rows)
    src = torch.randn(rows, 3, generator=g)
    sd = src.to(dev)
    p4 = torch.full((rows + 1, 4), float("nan"), device=dev)         # (one row more: nothing is written past `rows`)
    assert lib.dcn_pad_c3_to_c4(L.ptr(sd), L.ptr(p4), rows, L.stream_ptr()) == 0
    back = torch.full((rows + 1, 3), float("nan"), device=dev)
    assert lib.dcn_unpad_c4_to_c3(L.ptr(p4), L.ptr(back), rows, L.stream_ptr()) == 0
    _sync(dev)
    p4, back = p4.cpu(), back.cpu()
    assert torch.equal(p4[:rows, :3], src) and torch.equal(p4[:rows, 3], torch.zeros(rows))
    assert torch.equal(back[:rows], src)
    assert bool(torch.isnan(p4[rows]).all()) and bool(torch.isnan(back[rows]).all())


def check_pad_rows(L, dev, d, ld, rows=67):
    lib = L.get()
    g = torch.Generator().manual_seed(d)
    src = torch.randn(rows, d, generator=g)
    sd = src.to(dev)
    dst = torch.full((rows + 1, ld), float("nan"), device=dev)
    assert lib.dcn_pad_rows(L.ptr(sd), L.ptr(dst), rows, d, ld, L.stream_ptr()) == 0
    _sync(dev)
    dst = dst.cpu()
    assert torch.equal(dst[:rows, :d], src) and torch.equal(dst[:rows, d:], torch.zeros(rows, ld - d))
    assert bool(torch.isnan(dst[rows]).all())


COLSUM_ROWS = (1, 1023, 4096, 4097, 9000)      # the tail alone, the 4 x 1024-row unrolled loop alone, both together
COLSUM_DIMS = ((3, 4), (5, 8), (16, 16))


def check_column_sums(L, dev, rows, d, ld):
    """colsum_kernel (the fc.bias gradient) within 1 ulp of the float32 rounding of the float64 column sum; columns from d on
    hold NaN: they are not read into the result, and out[d ...] is not written."""
    lib = L.get()
    g = torch.Generator().manual_seed(rows + d)
    m = torch.randn(rows, ld, generator=g) + 0.25
    m[rows - 1, d - 1] = 1000.0                                       # the last row of the last column counts
    m[:, d:] = float("nan")
    md = m.to(dev)
    out = _floats((ld + 1,), dev)
    assert lib.dcn_column_sums(L.ptr(md), rows, ld, d, L.ptr(out), L.stream_ptr()) == 0
    _sync(dev)
    out = out.cpu()
    want = m[:, :d].double().sum(0).float()
    lo, hi = torch.nextafter(want, torch.full_like(want, float("-inf"))), torch.nextafter(want, torch.full_like(want, float("inf")))
    assert bool(((out[:d] >= lo) & (out[:d] <= hi)).all()), (rows, d, ld, out[:d], want)
    assert torch.equal(_bits(out[d:]), _bits(_floats((ld + 1 - d,), "cpu"))), (rows, d, ld)
