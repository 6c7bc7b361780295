"""Device augmentation (csrc/augment_kernels.hip) on the MI355X: the mirror module against the reference's golden outputs, the
batched path at training size against the numpy restatement and torch's normalization, the statistics of the device draws, no
host synchronization, and one end-to-end pass pair generation -> augmentation -> non-matches -> loss -> backward."""
import numpy as np
import pytest
import torch

import augment_common as ac
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("path", ac.GOLDENS, ids=ac.GOLDEN_IDS)
def test_mirror_replays_reference_golden_on_device(path):
    ac.replay_golden(path, "cuda")


@pytest.mark.parametrize("h,w", [(480, 640), (37, 53)])
def test_batched_path_with_explicit_params_full_size(h, w):
    from dcn_hip import augment
    B = 4
    rgb, mask = ac.scene(2 * B, h, w, seed=5)
    rec = ac.example_params(2 * B, seed=11)
    n_uv = [700, 0, 1234, 5]
    off = np.concatenate([[0], np.cumsum(n_uv)])
    rng = np.random.RandomState(2)
    ua, va = rng.randint(0, w, off[-1]), rng.randint(0, h, off[-1])
    ub = (rng.randint(0, w, off[-1]) + rng.rand(off[-1])).astype(np.float32)
    vb = (rng.randint(0, h, off[-1]) + rng.rand(off[-1])).astype(np.float32)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = augment.augment_image_pairs(c(rgb[:B]), c(rgb[B:]), c(mask[:B]), c(mask[B:]), (c(ua), c(va)), (c(ub), c(vb)),
                                    offsets=c(off), params=c(rec), return_rgb=True)
    torch.cuda.synchronize()
    for k in range(2 * B):
        side, i = divmod(k, B)
        exp_rgb, exp_mask = ac.restated_augment(rgb[k], mask[k], rec[k], k)
        assert np.array_equal((r.rgb_b if side else r.rgb_a)[i].cpu().numpy(), exp_rgb), (k, rec[k])
        assert np.array_equal((r.mask_b if side else r.mask_a)[i].cpu().numpy(), exp_mask.astype(np.float32)), k
        exp_in = ac.normalize_torch(exp_rgb[None], augment.DEFAULT_IMAGE_MEAN, augment.DEFAULT_IMAGE_STD_DEV)
        assert torch.equal((r.input_b if side else r.input_a)[i:i + 1].cpu(), exp_in), k
    for b in range(B):
        s = slice(off[b], off[b + 1])
        for got, u, v, k in ((r.uv_a, ua, va, b), (r.uv_b, ub, vb, B + b)):
            eu, ev = ac.restated_uv(u[s], v[s], rec[k], h, w)
            assert np.array_equal(got[0][s].cpu().numpy(), eu) and np.array_equal(got[1][s].cpu().numpy(), ev), k


def test_device_draws_statistics_and_replay():
    """~2 000 images: every decision at frequency 1/2 (5 sigma), a and b rotated independently, colours in 0..254, the noise
    difference triangular on -49..49 (loose chi-square), and the same generator state gives the same bits."""
    from dcn_hip import augment
    B, h, w = 1000, 16, 16
    rgb = torch.randint(0, 256, (2 * B, h, w, 3), dtype=torch.uint8, device="cuda")
    zero = torch.zeros(2 * B, h, w, dtype=torch.uint8, device="cuda")      # all background: the output IS the background
    g = torch.Generator(device="cuda").manual_seed(1234)
    r = augment.augment_image_pairs(rgb[:B], rgb[B:], zero[:B], zero[B:], generator=g, return_rgb=True)
    g2 = torch.Generator(device="cuda").manual_seed(1234)
    r2 = augment.augment_image_pairs(rgb[:B], rgb[B:], zero[:B], zero[B:], generator=g2, return_rgb=True)
    assert torch.equal(r.params, r2.params) and torch.equal(r.input_a, r2.input_a) and torch.equal(r.rgb_b, r2.rgb_b)
    p = r.params.cpu().numpy()
    f = p[:, 0]
    n = len(f)

    def half(sel, within):
        k, m = int(sel.sum()), int(within.sum())
        assert abs(k - 0.5 * m) <= 5 * np.sqrt(0.25 * m), (k, m)
    rnd = (f & ac.RANDOMIZE) != 0
    grad = (f & ac.GRADIENT) != 0
    half(rnd, np.ones(n, bool))
    half(grad & rnd, rnd)
    half(((f & ac.VERTICAL) != 0) & grad, grad)
    half(((f & ac.NOISE) != 0) & rnd, rnd)
    rot = (f & ac.FLIP_V) != 0
    assert np.array_equal(rot, (f & ac.FLIP_H) != 0)
    half(rot, np.ones(n, bool))
    both = int((rot[:B] & rot[B:]).sum())
    assert abs(both - 0.25 * B) <= 5 * np.sqrt(0.25 * 0.75 * B), both                 # independent rotations of a and b
    assert p[:, 1:7].min() >= 0 and p[:, 1:7].max() <= 254 and len(np.unique(p[:, 1:7])) == 255
    out = torch.cat([r.rgb_a, r.rgb_b]).cpu().numpy().astype(np.int64)
    solid = rnd & ~grad
    plain = solid & ((f & ac.NOISE) == 0)
    assert np.array_equal(out[plain], np.broadcast_to(p[plain][:, None, None, 1:4], out[plain].shape))
    noisy = solid & ((f & ac.NOISE) != 0)
    d = (out[noisy] - p[noisy][:, None, None, 1:4]) % 256
    d = np.where(d >= 128, d - 256, d).ravel()
    assert d.min() >= -49 and d.max() <= 49
    hist = np.bincount(d + 49, minlength=99)
    expect = d.size * (50 - np.abs(np.arange(-49, 50))) / 2500.0
    chi2 = float(((hist - expect) ** 2 / expect).sum())
    assert chi2 < 98 + 10 * np.sqrt(2 * 98), chi2
    kept = ~rnd
    src = rgb.cpu().numpy()[kept].astype(np.int64)
    assert np.array_equal(out[kept], np.stack([np.flip(x, (0, 1)) if fr else x for x, fr in zip(src, rot[kept])]))


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return [x for x in names if "DtoH" in x or "DeviceToHost" in x or x == "aten::item" or x == "aten::_local_scalar_dense"]


def test_batched_call_never_synchronizes():
    from dcn_hip import augment
    B, h, w = 4, 480, 640
    rgb = torch.randint(0, 256, (2 * B, h, w, 3), dtype=torch.uint8, device="cuda")
    mask = (torch.rand(2 * B, h, w, device="cuda") > 0.3).to(torch.uint8)
    uv = (torch.randint(0, w, (400,), device="cuda"), torch.randint(0, h, (400,), device="cuda"))
    off = torch.tensor([0, 100, 200, 300, 400], device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    call = lambda: augment.augment_image_pairs(rgb[:B], rgb[B:], mask[:B], mask[B:], uv, uv, offsets=off, generator=g)
    call()
    torch.cuda.synchronize()
    honoured = True
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.zeros(1, device="cuda").item()                   # a sync: must raise if the mode is honoured
            honoured = False
        except RuntimeError:
            pass
        if honoured:
            call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:   # (sync debug mode not honoured by this build): no device -> host copy or scalar read in the call
        assert _d2h_copies(call) == []
    torch.cuda.synchronize()


def test_end_to_end_pairgen_augment_nonmatches_loss_backward():
    """bench.py --workload pairgen's synthetic scene: device correspondences -> augment_image_pairs -> masked non-matches from
    the ROTATED mask_b -> batched loss -> backward through the network, at 640 x 480, B = 4 pairs."""
    from dcn_hip import augment
    from dcn_hip.loss import PairLists
    from dense_correspondence.correspondence_tools import correspondence_finder as cf
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    import parity_common as pc
    from oracle import synth
    H, W, B, NM = 480, 640, 4, 150
    rng = np.random.RandomState(2)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

    def surf():
        d = 900 + 150 * np.sin(xs / (60 + 40 * rng.rand())) + 120 * np.cos(ys / (50 + 30 * rng.rand())) + 40 * rng.rand()
        d[rng.rand(H, W) < 0.02] = 0
        return d.astype(np.uint16)

    def pose(ry, t):
        T = np.eye(4)
        T[:3, :3] = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
        T[:3, 3] = t
        return T
    depth_a, depth_b = surf(), surf()
    pose_a, pose_b = pose(0.01, [0.02, 0.0, 0.01]), pose(-0.06, [0.08, -0.03, 0.05])
    mask_np = np.zeros((H, W), np.uint8)
    mask_np[150:380, 180:470] = 1
    mask_np[150:200, 180:260] = 0                                           # not symmetric under the rotation
    mask = torch.from_numpy(mask_np).cuda()
    da = torch.from_numpy(depth_a.view(np.int16)).cuda()
    db = torch.from_numpy(depth_b.view(np.int16)).cuda()
    torch.manual_seed(0)
    found = [cf.batch_find_pixel_correspondences(da, pose_a, db, pose_b, num_attempts=2000, img_a_mask=mask.float())
             for _ in range(B)]
    lens = [int(f[0][0].numel()) for f in found]
    assert min(lens) > 50
    off = np.concatenate([[0], np.cumsum(lens)])
    uv_a = (torch.cat([f[0][0] for f in found]), torch.cat([f[0][1] for f in found]))
    uv_b = (torch.cat([f[1][0] for f in found]), torch.cat([f[1][1] for f in found]))
    rgb = torch.randint(0, 256, (2 * B, H, W, 3), dtype=torch.uint8, device="cuda")
    masks = mask.expand(2 * B, H, W).contiguous()
    g = torch.Generator(device="cuda").manual_seed(42)
    params = augment.draw_params(2 * B, "cuda", generator=g)
    params[:, 0] |= torch.tensor([0, 3, 0, 3, 3, 0, 0, 3], dtype=torch.int32, device="cuda")   # both outcomes on a and b
    r = augment.augment_image_pairs(rgb[:B], rgb[B:], masks[:B], masks[B:], uv_a, uv_b, offsets=off, params=params)
    rec = params.cpu().numpy()
    pcl = PixelwiseContrastiveLoss(image_shape=(H, W), config=synth.LOSS_CONFIG)
    tuples = []
    for b in range(B):
        s = slice(int(off[b]), int(off[b + 1]))
        for got, src, k in ((r.uv_a, uv_a, b), (r.uv_b, uv_b, B + b)):
            eu, ev = ac.restated_uv(src[0][s].cpu().numpy(), src[1][s].cpu().numpy(), rec[k], H, W)
            assert np.array_equal(got[0][s].cpu().numpy(), eu) and np.array_equal(got[1][s].cpu().numpy(), ev)
        ub, vb = r.uv_b[0][s], r.uv_b[1][s]
        mb = r.mask_b[b]
        assert torch.equal(mb, (torch.flip(mask, (0, 1)) if rec[B + b, 0] & 3 else mask).float())
        nu, nv = cf.create_non_correspondences((ub, vb), (H, W), NM, img_b_mask=mb)
        assert bool((mb[nv.long(), nu.long()] == 1).all())                # masked non-matches inside the rotated mask_b
        ma = r.uv_a[0][s] + r.uv_a[1][s] * W
        mbf = ub.long() + vb.long() * W
        tuples.append((ma, mbf, ma.repeat(NM), (nu.long() + nv.long() * W).reshape(-1), None, None, None, None))
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    ya, yb = dcn.forward_pair(r.input_a, r.input_b)
    loss = loss_composer.get_loss_batched(pcl, 0, dcn.process_network_output(ya, B), dcn.process_network_output(yb, B),
                                          PairLists.from_lists(tuples, "cuda", hw=H * W))[0]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    gw = [p.grad for p in dcn.parameters() if p.grad is not None]
    assert gw and all(bool(torch.isfinite(x).all()) for x in gw)
