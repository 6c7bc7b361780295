"""Frame store on the device (csrc/frame_kernels.hip, dcn_hip/frames.py) through the host-emulation build: the reference's own
frame choice replayed exactly, the gather against plain indexing, the camera rows against samples._cameras, an empty pair
through the sample builder, the host-side ValueErrors, and FrameStore.from_dataset on an in-memory reference dataset."""
import numpy as np
import pytest
import torch

import frames_common as fc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set_is_complete():
    assert sorted(fc.GOLDEN_IDS) == sorted(fc.TYPE_IDS)


@pytest.mark.parametrize("path", fc.GOLDENS, ids=fc.GOLDEN_IDS)
def test_golden_replays_exactly(path):
    z = np.load(path)
    store, fb = fc.run_golden(z, "cpu")
    fc.check_golden(fb, z)
    fc.check_gather(store, fb)


def test_goldens_cover_the_pose_test_edges():
    """Within-scene goldens: attempts just below / above 0.2 m, the pure 90-degree rotation rejected, a pair with no image b,
    and single-frame scenes chosen."""
    z = np.load(fc.GOLDENS[fc.GOLDEN_IDS.index("single_object_within_scene")])
    poses = z["poses"].reshape(-1, 4, 4)
    first = z["scene_first_frame"]
    seen = set()
    for p in range(z["draws"].shape[0]):
        fa = int(z["ref_frames"][p, 0])
        s = int(np.searchsorted(first, fa, side="right") - 1)
        if first[s + 1] - first[s] == 1:
            seen.add("single")
        for k in range(int(z["num_attempts"])):
            fb = int(first[s] + z["draws"][p, 8 + k])
            d = np.linalg.norm(poses[fa][:3, 3] - poses[fb][:3, 3])
            ok = fc.passes(poses, fa, fb)
            if 0.2 - 1e-5 < d < 0.2:
                seen.add("below")
            if 0.2 < d < 0.2 + 1e-5 and ok and int(z["ref_frames"][p, 1]) == fb:
                seen.add("above")
            R = poses[fa][:3, :3].T.dot(poses[fb][:3, :3])
            if d == 0 and abs(np.trace(R) - 1.0) < 1e-9:
                seen.add("rotation_rejected")
            if ok:
                assert int(z["ref_frames"][p, 1]) == fb
                break
        if z["ref_empty"][p]:
            seen.add("empty")
    assert seen == {"single", "below", "above", "rotation_rejected", "empty"}, seen


@pytest.mark.parametrize("shape", [(6, 10), (4, 16)], ids=["bytes", "vec16"])
@pytest.mark.parametrize("data_type", [0, 1, 2, 3, 4])
def test_drawn_gather_and_camera_rows(shape, data_type):
    from dcn_hip import frames
    z = np.load(fc.GOLDENS[0])
    S = len(z["scene_object"])
    K = np.stack([[[500.0 + 3 * s, 0, 320.5], [0, 510.0 - s, 240.25], [0, 0, 1]] for s in range(S)])
    store = fc.store_from_golden(z, "cpu", h=shape[0], w=shape[1], K=K)
    fb = frames.select_frames(store, 7, data_type, generator=torch.Generator().manual_seed(data_type))
    assert int(fb.status[0]) == 0
    fc.check_gather(store, fb)
    assert torch.equal(fb.cams, fc.host_cameras(store, fb))
    again = frames.select_frames(store, 7, data_type, seeds=fb.seeds)
    assert torch.equal(again.frames, fb.frames) and torch.equal(again.rgb, fb.rgb)


def test_empty_pair_is_empty_after_the_builder():
    from dcn_hip import frames, samples
    h, w = 24, 32
    poses = np.stack([np.eye(4)] * 3 + [np.eye(4)] * 3)
    poses[4, 0, 3] = 0.05                                     # scene 1: frames 3 and 5 differ from 4 ...
    poses[3, 2, 3] = poses[5, 2, 3] = 0.5                     # ... scene 0: every pose the same: no image b
    ys, xs = np.mgrid[0:h, 0:w]
    rgb, _, _ = fc.frames_for(6, h, w, 3)
    depth = torch.from_numpy(np.broadcast_to(900 + 3 * xs + 2 * ys, (6, h, w)).astype(np.int16).copy())
    mask = torch.zeros((6, h, w), dtype=torch.uint8)
    mask[:, 4:20, 6:26] = 1
    store = frames.FrameStore.from_tensors(rgb, depth, mask, poses, [0, 3, 6], [0, 1])
    draws = frames.pack_draws([dict(object_a=0, scene_a=0, frame_a=1, attempts_a=[0, 2]),
                               dict(object_a=1, scene_a=0, frame_a=1, attempts_a=[0, 2])], 4)
    fb = frames.select_frames(store, 2, frames.SINGLE_OBJECT_WITHIN_SCENE, draws=draws, num_attempts=4)
    assert fb.empty.tolist() == [True, False] and fb.frames[:, :2].tolist() == [[1, 1], [4, 3]]
    assert int(fb.status[0]) == 0
    sb = samples.build_within_scene_samples(fb.depth[0], fb.depth[1], fb.mask[0], fb.mask[1], None, None, None, fb.rgb[0],
                                            fb.rgb[1], num_matching_attempts=200, sample_matches_only_off_mask=True,
                                            num_masked_non_matches_per_match=2, num_background_non_matches_per_match=2,
                                            use_image_b_mask_inv=True, generator=torch.Generator().manual_seed(1),
                                            cameras=fb.cams[0])
    assert sb.type.tolist()[0] == -1 and bool(sb.empty[0])
    off = sb.offsets.tolist()
    assert off[4] == off[0]
    # the camera rows stand in for K / poses: the same lists as the host path
    ref = samples.build_within_scene_samples(fb.depth[0], fb.depth[1], fb.mask[0], fb.mask[1], poses[[1, 4]], poses[[1, 3]],
                                             None, num_matching_attempts=200, sample_matches_only_off_mask=True,
                                             num_masked_non_matches_per_match=2, num_background_non_matches_per_match=2,
                                             use_image_b_mask_inv=True, seeds=sb.seeds, aug_params=sb.aug_params)
    assert torch.equal(ref.offsets, sb.offsets) and torch.equal(ref.idx_a, sb.idx_a) and torch.equal(ref.idx_b, sb.idx_b)


def test_bad_replay_draws_raise_status():
    from dcn_hip import frames
    z = np.load(fc.GOLDENS[fc.GOLDEN_IDS.index("different_object")])
    d = z["draws"][:2].copy()
    d[0, 0] = d[0, 1]                                          # np.random.choice's two positions equal
    d[1, 5] = 99                                               # image a outside its scene
    store = fc.store_from_golden(z, "cpu")
    fb = frames.select_frames(store, 2, frames.DIFFERENT_OBJECT, draws=d, num_attempts=50)
    assert int(fb.status[0]) & frames.BAD_DRAWS


def test_host_side_value_errors():
    from dcn_hip import frames
    one_scene = dict(first=[0, 2, 4], sobj=[0, 1])
    poses = np.stack([np.eye(4)] * 4)
    store = fc.store_from_tables(one_scene["first"], one_scene["sobj"], poses, "cpu")
    assert store.supported_types == [frames.SINGLE_OBJECT_WITHIN_SCENE, frames.DIFFERENT_OBJECT,
                                     frames.SYNTHETIC_MULTI_OBJECT]
    with pytest.raises(ValueError, match="only one scene"):
        frames.select_frames(store, 2, frames.SINGLE_OBJECT_ACROSS_SCENE)
    with pytest.raises(ValueError, match="no multi object scenes"):
        frames.select_frames(store, 2, frames.MULTI_OBJECT)
    with pytest.raises(ValueError, match="only one scene"):
        fc.store_from_tables(one_scene["first"], one_scene["sobj"], poses, "cpu",
                             data_types=[frames.SINGLE_OBJECT_ACROSS_SCENE])
    with pytest.raises(ValueError, match="only one object"):
        fc.store_from_tables([0, 2, 4], [0, 0], poses, "cpu", data_types=[frames.DIFFERENT_OBJECT])
    with pytest.raises(ValueError, match="no single object scenes"):
        fc.store_from_tables([0, 4], [-1], poses, "cpu", data_types=[frames.SINGLE_OBJECT_WITHIN_SCENE])
    with pytest.raises(ValueError, match="increasing"):
        fc.store_from_tables([0, 2, 2, 4], [0, 0, 1], poses, "cpu")
    with pytest.raises(ValueError, match="numbered"):
        fc.store_from_tables([0, 2, 4], [0, 2], poses, "cpu")


def test_training_batch_type_distribution_and_synthetic_refusal():
    from dcn_hip import frames
    cfg = {"training": {"data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 0.5, "SINGLE_OBJECT_ACROSS_SCENE": 0.0,
                                                    "DIFFERENT_OBJECT": 0.25, "MULTI_OBJECT": 0.75,
                                                    "SYNTHETIC_MULTI_OBJECT": 0.0}}}
    types, ps = frames.data_type_distribution(cfg)
    assert types == [0, 2, 3] and np.allclose(ps, [1 / 3, 1 / 6, 1 / 2])
    cfg["training"]["data_type_probabilities"]["SYNTHETIC_MULTI_OBJECT"] = 0.1
    store = fc.store_from_tables([0, 2, 4], [0, 1], np.stack([np.eye(4)] * 4), "cpu")
    with pytest.raises(NotImplementedError, match="SYNTHETIC_MULTI_OBJECT"):
        frames.draw_training_batch(store, 2, cfg)


def test_from_dataset_reads_every_frame_once():
    """In its own process: the reference's SpartanDataset module must be imported from the reference tree, which other tests'
    imports of the product-root placeholder would shadow in this one."""
    import os
    import subprocess
    import sys
    import reference_py3 as rp
    if not rp.available():
        pytest.skip("the reference tree is not on this machine")
    root = os.path.dirname(fc.HERE)
    code = ("import sys; sys.path[:0] = %r\n"
            "from helpers import use_emulation_library\n"
            "use_emulation_library()\n"
            "import frames_common as fc\n"
            "fc.check_from_dataset()\n"
            "print('FROM_DATASET_OK')\n" % [fc.HERE, os.path.join(fc.HERE, "golden"), root,
                                            os.path.join(root, "pytorch-dense-correspondence_amd")])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FROM_DATASET_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
