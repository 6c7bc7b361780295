"""Shared by tests/test_emu_frames.py and tests/test_gpu_frames.py: frame stores built from the goldens' pose tables (frames
are synthetic: only the selection reads poses), the golden check, and a numpy restatement of the pose test of
get_img_idx_with_different_pose (dense_correspondence_dataset_masked.py:260-287, utils.compute_distance_between_poses)."""
import glob
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "frame_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("frame_ref_"):-4] for p in GOLDENS]
TYPE_IDS = ["single_object_within_scene", "single_object_across_scene", "different_object", "multi_object",
            "synthetic_multi_object"]


def frames_for(F, h, w, seed):
    """Distinct random frames: rgb uint8 [F, h, w, 3], depth int16 (uint16 bits) [F, h, w], mask 0/1 uint8 [F, h, w]."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (F, h, w, 3), dtype=torch.uint8, generator=g)
    depth = torch.randint(-2 ** 15, 2 ** 15, (F, h, w), dtype=torch.int16, generator=g)
    mask = torch.randint(0, 2, (F, h, w), dtype=torch.uint8, generator=g)
    return rgb, depth, mask


def store_from_tables(first, sobj, poses, device, h=6, w=10, K=None, seed=0, **kw):
    from dcn_hip import frames
    F = int(first[-1])
    rgb, depth, mask = frames_for(F, h, w, seed)
    return frames.FrameStore.from_tensors(rgb.to(device), depth.to(device), mask.to(device), np.asarray(poses), first, sobj,
                                          K, **kw)


def store_from_golden(z, device, **kw):
    return store_from_tables(z["scene_first_frame"], z["scene_object"], z["poses"], device, **kw)


def run_golden(z, device, gather=True, **kw):
    from dcn_hip import frames
    store = store_from_golden(z, device, **kw)
    n = int(z["draws"].shape[0])
    return store, frames.select_frames(store, n, int(z["type"]), draws=z["draws"], num_attempts=int(z["num_attempts"]),
                                       gather=gather)


def check_golden(fb, z):
    """The reference's chosen frames (-1: None, then frame b := frame a; -2: never chosen), empty flags, scenes, objects."""
    got = fb.frames.cpu().numpy()
    empty = fb.empty.cpu().numpy()
    assert int(fb.status.cpu()[0]) == 0
    assert np.array_equal(empty, z["ref_empty"]), (empty, z["ref_empty"])
    synthetic = int(z["type"]) == 4
    for p in range(got.shape[0]):
        ref = z["ref_frames"][p]
        for k in range(4):
            if ref[k] >= 0:
                assert got[p, k] == ref[k], (p, k, got[p], ref)
            elif ref[k] == -1:
                assert empty[p] and got[p, k] == got[p, k - 1], (p, k, got[p], ref)
        if not synthetic:
            assert got[p, 2] == -1 and got[p, 3] == -1
        elif empty[p]:
            assert got[p, 1] == got[p, 0] or got[p, 3] == got[p, 2]
        for k in range(2):
            if z["ref_scenes"][p, k] >= 0:
                assert int(fb.scenes[p, k]) == int(z["ref_scenes"][p, k]), (p, k)
                assert int(fb.objects[p, k]) == int(z["ref_objects"][p, k]), (p, k)


def passes(poses, fa, fb, threshold=0.2):
    """utils.compute_distance_between_poses(pose_a, pose_b) > threshold (the angle clause never passes at 20 radians)"""
    return np.linalg.norm(poses[fa][0:3, 3] - poses[fb][0:3, 3]) > threshold


def check_gather(store, fb):
    """The gathered planes equal plain indexing of the store, bit for bit; an empty pair's depth is zero."""
    f = fb.frames.cpu().long()
    k = int(fb.rgb.shape[0])
    empty = fb.empty.cpu()
    for s in range(k):
        idx = f[:, s].to(store.rgb.device)
        assert torch.equal(fb.rgb[s], store.rgb[idx])
        assert torch.equal(fb.mask[s], store.mask[idx])
        want = store.depth[idx].clone()
        want[empty.to(want.device)] = 0
        assert torch.equal(fb.depth[s], want)


def host_cameras(store, fb):
    """samples._cameras' rows for every camera row of the batch: [k / 2, B, 50] on the host."""
    from dcn_hip import samples
    f = fb.frames.cpu().numpy()
    first = np.asarray(store.scene_first_frame_host)
    poses = store.poses.cpu().numpy().reshape(-1, 4, 4)
    rows = []
    for j in range(int(fb.cams.shape[0])):
        fa, fbb = f[:, 2 * j], f[:, 2 * j + 1]
        scene = np.searchsorted(first, fa, side="right") - 1
        rows.append(samples._cameras(store.K[scene], poses[fa], poses[fbb], len(fa), torch.device("cpu")))
    return torch.stack(rows)


def check_from_dataset():
    """FrameStore.from_dataset on the in-memory reference dataset of make_frame_goldens_from_reference.py (a fresh process:
    needs the reference tree)."""
    import make_frame_goldens_from_reference as mk
    from dcn_hip import frames
    sdm, _ = mk.setup()
    ds, objects, multi, poses = mk.make_dataset(sdm)
    h, w = 4, 8
    calls = []

    def load(scene, idx):
        calls.append((scene, int(idx)))
        seed = len(calls)
        rng = np.random.RandomState(seed)
        return (rng.randint(0, 256, (h, w, 3)).astype(np.uint8), rng.randint(0, 65536, (h, w)).astype(np.uint16),
                (rng.rand(h, w) < 0.5).astype(np.uint8) * 255, poses[scene][int(idx)])

    class Cam(object):
        def __init__(self, s):
            self.s = s

        def get_camera_matrix(self):
            return np.array([[500.0 + len(self.s), 0, 4], [0, 500.0, 2], [0, 0, 1]])
    ds.get_rgbd_mask_pose = load
    ds.get_camera_intrinsics = Cam
    store = frames.FrameStore.from_dataset(ds, device="cpu")
    order = [s for o in objects for s in objects[o]] + list(multi)
    assert store.scene_names == order and store.object_ids == list(objects)
    assert calls == [(s, i) for s in order for i in range(len(poses[s]))]
    assert store.scene_object_host == [0, 0, 1, 1, 2, 2, -1, -1]
    for f, (s, i) in enumerate(calls):
        rng = np.random.RandomState(f + 1)
        r = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        d = rng.randint(0, 65536, (h, w)).astype(np.uint16)
        m = (rng.rand(h, w) < 0.5).astype(np.uint8)
        assert np.array_equal(store.rgb[f].numpy(), r) and np.array_equal(store.depth[f].numpy().view(np.uint16), d)
        assert np.array_equal(store.mask[f].numpy(), m)
        assert np.array_equal(store.poses[f].numpy().reshape(4, 4), poses[s][i])
    assert np.array_equal(store.K[0], Cam("thresh").get_camera_matrix())
    assert store.nbytes >= store.num_frames * h * w * 6
    z = np.load(GOLDENS[GOLDEN_IDS.index("single_object_within_scene")])
    assert np.array_equal(np.asarray(store.scene_first_frame_host), z["scene_first_frame"])
    fb = frames.select_frames(store, int(z["draws"].shape[0]), 0, draws=z["draws"], num_attempts=50)
    check_golden(fb, z)
