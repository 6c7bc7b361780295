"""Training samples on the device (csrc/sample_kernels.hip) on the MI355X: the reference's goldens, the full-size batch
against the numpy restatement, drawn-mode properties, complete_samples after the merge, no host synchronization, and
end-to-end build -> forward_pair -> get_loss_batched -> backward with an empty pair in the batch."""
import numpy as np
import pytest
import torch

import samples_common as sc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu

H, W, B = 480, 640, 4
A, K1, K2 = 10000, 75, 75                                          # training.yaml counts


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


def scene(n, seed=0):
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    depth, masks = np.zeros((2, n, H, W), np.uint16), np.zeros((2, n, H, W), np.uint8)
    for k in range(2):
        for p in range(n):
            d = 900 + 150 * np.sin(xs / (60 + 40 * rng.rand())) + 120 * np.cos(ys / (50 + 30 * rng.rand())) + 40 * rng.rand()
            d[rng.rand(H, W) < 0.02] = 0
            depth[k, p] = d.astype(np.uint16)
            masks[k, p, 120 + 10 * p:360, 100:380 + 20 * k] = 1
    pa = np.stack([np.eye(4)] * n)
    pb = np.stack([sc_pose(0.01 * p) for p in range(n)])
    return depth, masks, pa, pb


def sc_pose(ry):
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]]
    T[:3, 3] = [0.02, -0.01, 0.01]
    return T


def build(depth, masks, pa, pb, **kw):
    from dcn_hip import samples
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return samples.build_within_scene_samples(c(depth[0].view(np.int16)), c(depth[1].view(np.int16)), c(masks[0]),
                                              c(masks[1]), pa, pb, num_matching_attempts=A, sample_matches_only_off_mask=True,
                                              num_masked_non_matches_per_match=K1, num_background_non_matches_per_match=K2,
                                              use_image_b_mask_inv=True, **kw)


@pytest.mark.parametrize("path", sc.GOLDENS, ids=sc.GOLDEN_IDS)
def test_golden_replays_on_device(path):
    z = np.load(path)
    r = sc.run_golden_batch([z], "cuda")
    sc.check_golden(r, 0, z)
    sc.check_layout(r)


def test_full_size_batch_matches_restatement():
    depth, masks, pa, pb = scene(B)
    params = sc.params_from_flips([True, False, True, False], [False, True, True, False])
    r = build(depth, masks, pa, pb, generator=torch.Generator(device="cuda").manual_seed(1), aug_params=params)
    torch.cuda.synchronize()
    sc.check_layout(r)
    K = sc.default_K()
    for p in range(B):
        got = sc.batch_lists(r, p)
        assert len(got[0]) > 100
        assert len(got[2]) == K1 * len(got[0]) and len(got[4]) == K2 * len(got[0])
        assert np.array_equal(got[2], np.repeat(got[0], K1)) and np.array_equal(got[4], np.repeat(got[0], K2))
    # one pair in full through the restatement with small counts
    from dcn_hip import samples
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = samples.build_within_scene_samples(c(depth[0, :1].view(np.int16)), c(depth[1, :1].view(np.int16)), c(masks[0, :1]),
                                           c(masks[1, :1]), pa[:1], pb[:1], num_matching_attempts=1500,
                                           sample_matches_only_off_mask=True, num_masked_non_matches_per_match=2,
                                           num_background_non_matches_per_match=2, use_image_b_mask_inv=True,
                                           aug_params=params[[0, B]], generator=torch.Generator(device="cuda").manual_seed(2))
    U = lambda site, k, s=int(r.seeds[0]): sc.hash_uniform(s, site, k)
    lists, typ = sc.restated_within(depth[0, 0], depth[1, 0], masks[0, 0], masks[1, 0], sc.cams_of(K, pa[0], pb[0]), True,
                                    False, 1500, True, 2, 2, True, U)
    sc.check_against_restatement(r, 0, lists, typ)


def test_drawn_mode_properties_and_determinism():
    depth, masks, pa, pb = scene(B, seed=2)
    r = build(depth, masks, pa, pb, generator=torch.Generator(device="cuda").manual_seed(3))
    r2 = build(depth, masks, pa, pb, seeds=r.seeds, aug_params=r.aug_params)
    assert torch.equal(r.idx_a, r2.idx_a) and torch.equal(r.idx_b, r2.idx_b) and torch.equal(r.offsets, r2.offsets)
    sc.check_layout(r)
    params = r.aug_params.cpu().numpy()
    for p in range(B):
        rot = lambda m, f: m[::-1, ::-1] if f else m
        ma = rot(masks[0, p], params[p, 0] & 3).reshape(-1)
        mb = rot(masks[1, p], params[B + p, 0] & 3).reshape(-1)
        l = sc.batch_lists(r, p)
        assert (mb[l[3]] == 1).all() and (mb[l[5]] == 0).all()
        assert (ma[l[6]] == 1).all() and not np.isin(l[6], l[0]).any() and (mb[l[7]] == 1).all()
        # loose uniformity of the masked b draws over mask b's pixels: every quarter of the list gets its share
        lst = np.flatnonzero(mb)
        q = np.searchsorted(lst, l[3]) * 4 // lst.size
        share = np.bincount(q, minlength=4) / l[3].size
        assert (np.abs(share - 0.25) < 0.02).all(), share


def test_complete_samples_after_merge():
    import merge_common as mc
    from dcn_hip import samples
    rgb, masks, lists = mc.example_batch(B, H, W, [3000] * B, [2000] * B, seed=7)
    fg = np.array([[0, 1], [1, 0], [1, 1], [1, 0]], dtype=np.int32)
    m = mc.run_batched(rgb, masks, lists, fg, "cuda", return_rgb=False)
    r = samples.complete_samples(m.uv_1, m.uv_2, m.offsets, m.mask_1, m.mask_2, num_masked_non_matches_per_match=K1,
                                 num_background_non_matches_per_match=K2, use_image_b_mask_inv=True,
                                 generator=torch.Generator(device="cuda").manual_seed(4))
    sc.check_layout(r)
    off = m.offsets.cpu().numpy()
    for p in range(B):
        l = sc.batch_lists(r, p)
        sl = slice(int(off[p]), int(off[p + 1]))
        assert np.array_equal(l[0], (m.uv_1[1][sl] * W + m.uv_1[0][sl]).cpu().numpy())
        mb = m.mask_2[p].cpu().numpy().reshape(-1)
        assert (mb[l[3]] == 1).all() and (mb[l[5]] == 0).all()
    assert r.empty.tolist() == m.empty.tolist()


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return [x for x in names if "DtoH" in x or "DeviceToHost" in x or x == "aten::item" or x == "aten::_local_scalar_dense"]


def test_builders_never_synchronize():
    from dcn_hip import samples
    depth, masks, pa, pb = scene(B, seed=3)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d0, d1, m0, m1 = c(depth[0].view(np.int16)), c(depth[1].view(np.int16)), c(masks[0]), c(masks[1])
    rgb = torch.randint(0, 256, (2, B, H, W, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    kw = dict(num_matching_attempts=A, sample_matches_only_off_mask=True, num_masked_non_matches_per_match=K1,
              num_background_non_matches_per_match=K2, use_image_b_mask_inv=True, generator=g)

    def call():
        samples.build_within_scene_samples(d0, d1, m0, m1, pa, pb, None, rgb[0], rgb[1], **kw)
        samples.build_across_scene_samples(m0, m1, rgb[0], rgb[1], num_samples=1000, generator=g)
    call()
    torch.cuda.synchronize()
    honoured = True
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.zeros(1, device="cuda").item()
            honoured = False
        except RuntimeError:
            pass
        if honoured:
            call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        assert _d2h_copies(call) == []
    torch.cuda.synchronize()


@pytest.mark.parametrize("across", [False, True])
def test_end_to_end_build_forward_loss_backward(across):
    """build -> forward_pair -> get_loss_batched -> backward with pair 1 empty.  The batched loss kernel gives an empty pair
    (every list empty) a loss of exactly 0, and the batch loss is the mean over the pairs with that 0 included."""
    from dcn_hip import samples
    from dense_correspondence.dataset.spartan_dataset_masked import SpartanDatasetDataType as DT
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    import parity_common as pc
    from oracle import synth
    n = 2
    depth, masks, pa, pb = scene(n, seed=5)
    masks[0, 1] = 0                                                   # pair 1: empty mask a
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rgb = torch.randint(0, 256, (2, n, H, W, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(6)
    if across:
        r = samples.build_across_scene_samples(c(masks[0]), c(masks[1]), rgb[0], rgb[1], num_samples=1000, generator=g)
        dt = DT.SINGLE_OBJECT_ACROSS_SCENE
    else:
        r = samples.build_within_scene_samples(c(depth[0].view(np.int16)), c(depth[1].view(np.int16)), c(masks[0]),
                                               c(masks[1]), pa, pb, None, rgb[0], rgb[1], num_matching_attempts=A,
                                               sample_matches_only_off_mask=True, num_masked_non_matches_per_match=K1,
                                               num_background_non_matches_per_match=K2, use_image_b_mask_inv=True,
                                               generator=g)
        dt = DT.SINGLE_OBJECT_WITHIN_SCENE
    assert r.empty.tolist() == [False, True] and r.type.tolist() == [int(dt), -1]
    pl = r.pair_lists()
    assert all(pl.length(1, t) == 0 for t in range(4))
    pcl = PixelwiseContrastiveLoss(image_shape=(H, W), config=synth.LOSS_CONFIG)
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    ya, yb = dcn.forward_pair(r.input_a, r.input_b)
    out = loss_composer.get_loss_batched(pcl, dt, dcn.process_network_output(ya, n), dcn.process_network_output(yb, n), pl)
    loss = out[0]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    terms = out[1]
    assert bool((terms[1] == 0).all())                                 # the empty pair: every term exactly 0 ...
    assert torch.allclose(loss, terms[:, 0].mean())                    # ... and it counts in the batch mean
    gw = [p.grad for p in dcn.parameters() if p.grad is not None]
    assert gw and all(bool(torch.isfinite(x).all()) for x in gw)
