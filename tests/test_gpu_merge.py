"""Synthetic multi-object merge (csrc/merge_kernels.hip) on the MI355X: the mirror module against the reference's golden
outputs, the batched path at training size against the numpy restatement, no host synchronization, and one end-to-end pass
device correspondences of two objects -> batched merge -> non-matches on mask_2 -> SYNTHETIC_MULTI_OBJECT loss -> backward."""
import numpy as np
import pytest
import torch

import merge_common as mc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu

H, W, B, NM = 480, 640, 4, 5000


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.fixture(scope="module")
def batch():
    """B = 4 samples at 640 x 480 with 5 000 matches per object and sample; sample 3's b is fully covered in frame 2."""
    rgb, masks, lists = mc.example_batch(B, H, W, [NM] * B, [NM] * B, seed=7)
    masks[1, 3] = 1
    fg = np.array([[0, 1], [1, 0], [1, 1], [1, 0]], dtype=np.int32)
    return rgb, masks, lists, fg


@pytest.mark.parametrize("path", mc.GOLDENS, ids=mc.GOLDEN_IDS)
def test_mirror_replays_reference_golden_on_device(path):
    mc.replay_golden(path, "cuda")


def test_batched_path_full_size_matches_restatement(batch):
    rgb, masks, lists, fg = batch
    r = mc.run_batched(rgb, masks, lists, fg, "cuda")
    torch.cuda.synchronize()
    assert bool(r.empty[3]) and not bool(r.empty[:3].any())
    mc.check_batched_against_restatement(r, rgb, masks, lists, fg)


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return [x for x in names if "DtoH" in x or "DeviceToHost" in x or x == "aten::item" or x == "aten::_local_scalar_dense"]


def test_batched_call_never_synchronizes(batch):
    from dcn_hip import merge
    rgb, masks, lists, _ = batch
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ims, mks = [c(x) for x in rgb], [c(x) for x in masks]
    (ua1, va1, ua2, va2, offa), (ub1, vb1, ub2, vb2, offb) = [[c(x) for x in l] for l in lists]
    g = torch.Generator(device="cuda").manual_seed(3)
    call = lambda: merge.merge_synthetic_samples(*ims, *mks, (ua1, va1), (ua2, va2), (ub1, vb1), (ub2, vb2), offa, offb,
                                                 generator=g)
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


def test_end_to_end_correspondences_merge_nonmatches_loss_backward():
    """Two synthetic objects, each with device correspondences between its frames 1 and 2 -> merge_synthetic_samples ->
    masked non-matches on the merged mask_2 -> batched SYNTHETIC_MULTI_OBJECT loss -> backward through the network."""
    from dcn_hip import merge
    from dcn_hip.loss import PairLists
    from dense_correspondence.correspondence_tools import correspondence_finder as cf
    from dense_correspondence.dataset.spartan_dataset_masked import SpartanDatasetDataType
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    import parity_common as pc
    from oracle import synth
    NB, NNM = 2, 150
    rng = np.random.RandomState(3)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

    def surf():
        d = 900 + 150 * np.sin(xs / (60 + 40 * rng.rand())) + 120 * np.cos(ys / (50 + 30 * rng.rand())) + 40 * rng.rand()
        d[rng.rand(H, W) < 0.02] = 0
        return torch.from_numpy(d.astype(np.uint16).view(np.int16)).cuda()

    def pose(ry, t):
        T = np.eye(4)
        T[:3, :3] = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
        T[:3, 3] = t
        return T
    mask_np = np.zeros((2, H, W), np.uint8)
    mask_np[0, 120:360, 100:380] = 1                                   # object a, left
    mask_np[1, 150:400, 300:560] = 1                                   # object b, right: they overlap
    masks = torch.from_numpy(mask_np).cuda()
    torch.manual_seed(0)
    uv, off = {}, {}
    for o in range(2):
        d1, d2 = surf(), surf()
        found = [cf.batch_find_pixel_correspondences(d1, pose(0.01, [0.02, 0, 0.01]), d2, pose(-0.05, [0.07, -0.03, 0.04]),
                                                     num_attempts=2000, img_a_mask=masks[o].float()) for _ in range(NB)]
        lens = [int(f[0][0].numel()) for f in found]
        assert min(lens) > 50
        off[o] = np.concatenate([[0], np.cumsum(lens)])
        uv[o] = ((torch.cat([f[0][0] for f in found]), torch.cat([f[0][1] for f in found])),
                 (torch.cat([f[1][0].long() for f in found]), torch.cat([f[1][1].long() for f in found])))
    rgb = torch.randint(0, 256, (4, NB, H, W, 3), dtype=torch.uint8, device="cuda")
    mk = [masks[o].expand(NB, H, W).contiguous() for o in (0, 0, 1, 1)]     # a1, a2, b1, b2
    fg = torch.tensor([[1, 0], [0, 1]], dtype=torch.int32)
    r = merge.merge_synthetic_samples(rgb[0], rgb[1], rgb[2], rgb[3], *mk, uv[0][0], uv[0][1], uv[1][0], uv[1][1], off[0],
                                      off[1], foreground=fg)
    offsets = r.offsets.cpu().numpy()
    assert int(r.status.cpu()[0]) == 0 and not bool(r.empty.any())
    pcl = PixelwiseContrastiveLoss(image_shape=(H, W), config=synth.LOSS_CONFIG)
    merged_2 = (masks[0] | masks[1]).float()
    tuples = []
    for s in range(NB):
        sl = slice(int(offsets[s]), int(offsets[s + 1]))
        assert sl.stop - sl.start > 50
        u1, v1, u2, v2 = r.uv_1[0][sl], r.uv_1[1][sl], r.uv_2[0][sl], r.uv_2[1][sl]
        assert torch.equal(r.mask_2[s], merged_2)
        nu, nv = cf.create_non_correspondences((u2.float(), v2.float()), (H, W), NNM, img_b_mask=r.mask_2[s])
        assert bool((r.mask_2[s][nv.long(), nu.long()] == 1).all())
        ma, mb = u1 + v1 * W, u2 + v2 * W
        tuples.append((ma, mb, ma.repeat(NNM), (nu.long() + nv.long() * W).reshape(-1), None, None, None, None))
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    ya, yb = dcn.forward_pair(r.input_1, r.input_2)
    loss = loss_composer.get_loss_batched(pcl, SpartanDatasetDataType.SYNTHETIC_MULTI_OBJECT,
                                          dcn.process_network_output(ya, NB), dcn.process_network_output(yb, NB),
                                          PairLists.from_lists(tuples, "cuda", hw=H * W))[0]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    gw = [p.grad for p in dcn.parameters() if p.grad is not None]
    assert gw and all(bool(torch.isfinite(x).all()) for x in gw)
