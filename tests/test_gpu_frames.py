"""Frame store on the device (csrc/frame_kernels.hip) on the MI355X: the reference's goldens, the full-size gather against
indexing, drawn-mode properties, no host synchronization in draw_training_batch, and store -> draw_training_batch ->
forward_pair -> get_loss_batched -> backward with an empty pair in the batch."""
import numpy as np
import pytest
import torch

import frames_common as fc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu

H, W = 480, 640
CFG = {"training": {"num_matching_attempts": 10000, "sample_matches_only_off_mask": True, "num_non_matches_per_match": 150,
                    "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5,
                    "cross_scene_num_samples": 10000, "use_image_b_mask_inv": True, "domain_randomize": False,
                    "data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 1.0, "SINGLE_OBJECT_ACROSS_SCENE": 0.0,
                                                "DIFFERENT_OBJECT": 0.0, "MULTI_OBJECT": 0.0,
                                                "SYNTHETIC_MULTI_OBJECT": 0.0}}}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


def _pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def training_store(h=H, w=W):
    """Object 0: scene ``moving`` (4 frames >= 0.25 m apart: image b always found) and scene ``still`` (4 equal poses: never);
    object 1: two moving scenes.  A flat wall at 0.9 m (with no-return holes) seen by cameras translated in its plane, and
    rectangular 0/1 masks, so that within-scene pairs have many matches."""
    from dcn_hip import frames
    rng = np.random.RandomState(0)
    moving = [_pose(t) for t in ([0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0.25, 0.25, 0])]
    poses = moving + [_pose([0.1, 0, 0])] * 4 + moving + moving
    F = len(poses)
    depth = np.full((F, h, w), 900, np.uint16)
    depth[rng.rand(F, h, w) < 0.02] = 0
    mask = np.zeros((F, h, w), np.uint8)
    mask[:, h // 4:3 * h // 4, w // 6:5 * w // 6] = 1
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rgb = torch.randint(0, 256, (F, h, w, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    return frames.FrameStore.from_tensors(rgb, c(depth.view(np.int16)), c(mask), np.stack(poses), [0, 4, 8, 12, 16],
                                          [0, 0, 1, 1])


@pytest.mark.parametrize("path", fc.GOLDENS, ids=fc.GOLDEN_IDS)
def test_golden_replays_on_device(path):
    z = np.load(path)
    store, fb = fc.run_golden(z, "cuda")
    torch.cuda.synchronize()
    fc.check_golden(fb, z)
    fc.check_gather(store, fb)


@pytest.mark.parametrize("data_type", [0, 4])
def test_full_size_gather_matches_indexing(data_type):
    """About 64 frames of 640 x 480 in 8 scenes of two objects; B = 4 pairs gathered against store indexing, camera rows
    against samples._cameras."""
    from dcn_hip import frames
    rng = np.random.RandomState(3)
    poses = np.stack([_pose(rng.normal(0, 0.2, 3)) for _ in range(64)])
    first = np.arange(0, 65, 8)
    store = fc.store_from_tables(first, [0, 0, 0, 0, 1, 1, 1, 1], poses, "cuda", h=H, w=W, seed=5)
    fb = frames.select_frames(store, 4, data_type, generator=torch.Generator(device="cuda").manual_seed(2))
    torch.cuda.synchronize()
    assert int(fb.status[0]) == 0
    fc.check_gather(store, fb)
    assert torch.equal(fb.cams.cpu(), fc.host_cameras(store, fb))


def test_drawn_mode_properties_and_determinism():
    """Frame a uniform over its scene (loose chi-square), every accepted image b passes the pose test and every empty pair
    had none to find, scenes of the drawn objects, and the same seeds give the same batch."""
    from dcn_hip import frames
    rng = np.random.RandomState(4)
    poses = np.stack([_pose(rng.normal(0, 0.15, 3)) for _ in range(10)] + [_pose([0.3, 0, 0])] * 5)
    store = fc.store_from_tables([0, 10, 15], [-1, -1], poses, "cuda", h=8, w=16)
    n = 2000
    fb = frames.select_frames(store, n, frames.MULTI_OBJECT, generator=torch.Generator(device="cuda").manual_seed(5))
    f, empty, sc = fb.frames.cpu().numpy(), fb.empty.cpu().numpy(), fb.scenes.cpu().numpy()
    assert int(fb.status[0]) == 0
    in_first = sc[:, 0] == 0
    assert abs(in_first.mean() - 0.5) < 0.05                               # uniform over the two multi-object scenes
    counts = np.bincount(f[in_first, 0], minlength=10)[:10]
    expect = in_first.sum() / 10.0
    assert ((counts - expect) ** 2 / expect).sum() < 40.0                  # chi-square, 9 degrees of freedom
    assert empty[~in_first].all()                                          # every pose of scene 1 is the same
    for p in np.nonzero(in_first & ~empty)[0]:
        assert fc.passes(poses, f[p, 0], f[p, 1])
    for p in np.nonzero(in_first & empty)[0]:
        assert not any(fc.passes(poses, f[p, 0], j) for j in range(10))
    again = frames.select_frames(store, n, frames.MULTI_OBJECT, seeds=fb.seeds)
    assert torch.equal(again.frames, fb.frames) and torch.equal(again.rgb, fb.rgb) and torch.equal(again.cams, fb.cams)


def test_training_batch_type_frequencies():
    from dcn_hip import frames
    store = training_store(h=16, w=32)
    cfg = {"training": dict(CFG["training"], num_matching_attempts=50, cross_scene_num_samples=20,
                            data_type_probabilities={"SINGLE_OBJECT_WITHIN_SCENE": 2.0, "SINGLE_OBJECT_ACROSS_SCENE": 1.0,
                                                     "DIFFERENT_OBJECT": 1.0, "MULTI_OBJECT": 0.0,
                                                     "SYNTHETIC_MULTI_OBJECT": 0.0})}
    host = np.random.RandomState(6)
    g = torch.Generator(device="cuda").manual_seed(6)
    seen = []
    for _ in range(300):
        sb, dt, fb = frames.draw_training_batch(store, 2, cfg, generator=g, host_rng=host)
        seen.append(dt)
    torch.cuda.synchronize()
    freq = np.bincount(seen, minlength=3)[:3] / 300.0
    assert np.all(np.abs(freq - [0.5, 0.25, 0.25]) < 0.1), freq


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return [x for x in names if "DtoH" in x or "DeviceToHost" in x or x == "aten::item" or x == "aten::_local_scalar_dense"]


def test_draw_training_batch_never_synchronizes():
    from dcn_hip import frames
    store = training_store()
    g = torch.Generator(device="cuda").manual_seed(7)
    host = np.random.RandomState(7)

    def call():
        frames.draw_training_batch(store, 4, CFG, generator=g, host_rng=host)
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


def test_end_to_end_store_to_loss_backward():
    """draw_training_batch -> forward_pair -> get_loss_batched -> backward, with one pair drawn from the scene where no image
    b has a different enough pose: that pair is empty and its loss is exactly 0, counted in the batch mean."""
    from dcn_hip import frames
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    import parity_common as pc
    from oracle import synth
    store = training_store()
    n = 2
    for seed in range(64):                       # the first seed that draws one empty and one non-empty pair
        g = torch.Generator(device="cuda").manual_seed(seed)
        sb, dt, fb = frames.draw_training_batch(store, n, CFG, generator=g, host_rng=np.random.RandomState(seed))
        if sorted(fb.empty.tolist()) == [False, True]:
            break
    else:
        raise AssertionError("no seed gave a batch with one empty pair")
    assert dt == frames.SINGLE_OBJECT_WITHIN_SCENE and int(fb.status[0]) == 0
    e = int(np.nonzero(fb.empty.cpu().numpy())[0][0])
    assert sb.empty.tolist()[e] and sb.type.tolist()[e] == -1 and sb.type.tolist()[1 - e] == dt
    pl = sb.pair_lists()
    assert all(pl.length(e, t) == 0 for t in range(4)) and pl.length(1 - e, 0) > 100
    pcl = PixelwiseContrastiveLoss(image_shape=(H, W), config=synth.LOSS_CONFIG)
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
    out = loss_composer.get_loss_batched(pcl, dt, dcn.process_network_output(ya, n), dcn.process_network_output(yb, n), pl)
    loss = out[0]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    terms = out[1]
    assert bool((terms[e] == 0).all())
    assert torch.allclose(loss, terms[:, 0].mean())
    gw = [p.grad for p in dcn.parameters() if p.grad is not None]
    assert gw and all(bool(torch.isfinite(x).all()) for x in gw)
