"""Shared by tests/test_emu_evaluate.py and tests/test_gpu_evaluate.py: the evalpairs goldens (the reference's own match search,
``random.sample`` and compute_descriptor_match_statistics on synthetic pairs, tests/golden/
make_evalpairs_goldens_from_reference.py) replayed through dcn_hip.evaluate, a float64 numpy restatement of the depth / 3D half
(evaluation.py:1102-1135, :1148-1164), and a numpy restatement of the pair choice."""
import glob
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "evalpairs_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("evalpairs_ref_"):-4] for p in GOLDENS]


def py2_round(x):
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def golden_inputs(z, device):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(device)
    d = {k: t(k) for k in ("res_a", "res_b", "mask_a", "mask_b", "cams")}
    d["depth_a"] = torch.from_numpy(z["depth_a"].view(np.int16)).to(device)
    d["depth_b"] = torch.from_numpy(z["depth_b"].view(np.int16)).to(device)
    return d


def golden_matches(z, d):
    """The reference's candidate draws and match_list replayed through find_eval_matches"""
    from dcn_hip import evaluate
    P = int(z["mask_a"].shape[0])
    ro = z["rand_cand_offsets"]
    draws = {"cand": [z["rand_cand"][ro[p]:ro[p + 1]] for p in range(P)]}
    return evaluate.find_eval_matches(d["depth_a"], d["depth_b"], d["mask_a"], d["cams"], int(z["num_matches"]),
                                      num_attempts=int(z["num_attempts"]), draws=draws, match_order=z["match_order"])


def check_matches(m, z):
    """Rows in match_list order: pixels of image a equal; the float projection to 1e-4 px (the reference inverts pose b
    once more than the camera row, which can move the last bit), its rounded and clipped pixel equal."""
    assert int(m.status.cpu()[0]) == 0
    assert np.array_equal(m.totals.cpu().numpy(), z["totals"])
    off = m.offsets.cpu().numpy()
    assert np.array_equal(off, z["offsets"])
    R = int(off[-1])
    assert R == len(z["row_pair"])
    assert np.array_equal(m.u_a.cpu().numpy()[:R], z["u_a"]) and np.array_equal(m.v_a.cpu().numpy()[:R], z["v_a"])
    ub, vb = m.u_b.cpu().numpy(), m.v_b.cpu().numpy()
    np.testing.assert_allclose(ub[:R], z["u_b"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(vb[:R], z["v_b"], rtol=0, atol=1e-4)
    w, h = int(z["w"]), int(z["h"])
    assert [min(py2_round(x), w - 1) for x in ub[:R]] == z["gt_u"].tolist()
    assert [min(py2_round(x), h - 1) for x in vb[:R]] == z["gt_v"].tolist()
    assert (m.u_a.cpu().numpy()[R:] == -1).all() and (ub[R:] == 0).all()


def check_table(t, z, rows=None):
    """An EvalTable against the golden's rows (``rows``: the golden rows the table's rows correspond to, default all).
    Tolerances: those of test_match_statistics_vs_reference_golden (rtol 1e-5 for descriptor distances, rtol / atol 1e-6 for
    pixel errors, counts +-1 for a distance that ties with the ground truth's, averages where the count exceeds 20 at rtol
    0.1); fractions are the counts over a constant, so +-1 count; 3D columns 1e-9 m absolute (float64 on both sides)."""
    from dcn_hip import evaluate
    sel = np.arange(len(z["row_pair"])) if rows is None else np.asarray(rows)
    R = len(sel)
    assert int(t.status.cpu()[0]) == 0
    cols = t.columns.cpu().numpy()
    assert cols.shape == (len(evaluate.COLUMNS), R)
    got = {k: cols[i] for i, k in enumerate(evaluate.COLUMNS)}
    pred, valid, closer = t.pred_uv.cpu().numpy(), t.is_valid.cpu().numpy(), t.closer.cpu().numpy().astype(np.int64)
    for i, k in enumerate(("pred_u", "pred_v", "pred_u_masked", "pred_v_masked")):
        assert np.array_equal(pred[i], z[k][sel]), k
    assert np.array_equal(valid[0] != 0, z["is_valid"][sel]) and np.array_equal(valid[1] != 0, z["is_valid_masked"][sel])
    assert np.array_equal(t.row_pair.cpu().numpy(), z["row_pair"][sel])
    for k in evaluate.COLUMNS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(z[k][sel])), k
    for k in ("norm_diff_descriptor_ground_truth", "norm_diff_descriptor", "norm_diff_descriptor_masked"):
        np.testing.assert_allclose(got[k], z[k][sel], rtol=1e-5, err_msg=k)
    for k in ("pixel_match_error_l2", "pixel_match_error_l2_masked", "pixel_match_error_l1"):
        np.testing.assert_allclose(got[k], z[k][sel], rtol=1e-6, atol=1e-6, err_msg=k)
    hw = float(z["h"]) * float(z["w"])
    n_mask = (z["mask_b"] != 0).reshape(z["mask_b"].shape[0], -1).sum(1)
    assert np.array_equal(t.mask_pixels.cpu().numpy(), n_mask)
    denom = {"": np.full(R, hw), "_masked": n_mask[z["row_pair"][sel]].astype(np.float64)}
    for i, name in enumerate(("", "_masked")):
        ref = z["closer" + name][sel]
        assert np.abs(closer[i] - ref).max() <= 1, name
        np.testing.assert_allclose(got["fraction_pixels_closer_than_ground_truth" + name], closer[i] / denom[name], rtol=1e-12)
        assert np.abs(got["fraction_pixels_closer_than_ground_truth" + name]
                      - z["fraction_pixels_closer_than_ground_truth" + name][sel]).max() <= 1.0 / denom[name].min() + 1e-12
        big = ref > 20
        np.testing.assert_allclose(got["average_l2_distance_for_false_positives" + name][big],
                                   z["average_l2_distance_for_false_positives" + name][sel][big], rtol=0.1)
    for k in ("norm_diff_ground_truth_3d", "norm_diff_pred_3d", "norm_diff_pred_3d_masked"):
        ok = ~np.isnan(z[k][sel])
        assert np.abs(got[k][ok] - z[k][sel][ok]).max() <= 1e-9 if ok.any() else True, k


def rigid_inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -out[:3, :3].dot(T[:3, 3])
    return out


def numpy_3d_from_poses(K, pose_a, pose_b, depth_a, depth_b, uv_a, gt, pred, pred_masked):
    """evaluation.py:1102-1135 + :1148-1164 for one row, float64: -> (is_valid, is_valid_masked, norm_diff_ground_truth_3d,
    norm_diff_pred_3d, norm_diff_pred_3d_masked).  (Also the 3D half of tools/evaluate_bench.py's baseline.)"""
    Ki = np.linalg.inv(K)

    def pos(uv, z, pose):
        return pose.dot(np.append(z * Ki.dot(np.array([uv[0], uv[1], 1.0])), 1.0))[:3]
    valid = lambda d: d > 0 and d < 10.0
    za = float(depth_a[uv_a[1], uv_a[0]]) / 1000.0
    zb = float(depth_b[gt[1], gt[0]]) / 1000.0
    z0 = float(depth_b[pred[1], pred[0]]) / 1000.0
    z1 = float(depth_b[pred_masked[1], pred_masked[0]]) / 1000.0
    pa, pb = pos(uv_a, za, pose_a), pos(gt, zb, pose_b)
    gt3d = np.linalg.norm(pb - pa) if valid(zb) else np.nan
    p3d = np.linalg.norm(pb - pos(pred, z0, pose_b)) if valid(zb) and valid(z0) else np.nan
    p3dm = np.linalg.norm(pb - pos(pred_masked, z1, pose_b)) if valid(zb) and valid(z1) else np.nan
    return valid(z0), valid(z1), gt3d, p3d, p3dm


def numpy_3d_columns(cam, depth_a, depth_b, uv_a, gt, pred, pred_masked):
    """numpy_3d_from_poses from an fp32 camera row (K, K^-1, pose a, pose b^-1): K and pose a cast to float64, pose b the
    float64 rigid inverse of the row's pose b^-1"""
    cam = np.asarray(cam, np.float32).astype(np.float64)
    return numpy_3d_from_poses(cam[:9].reshape(3, 3), cam[18:34].reshape(4, 4), rigid_inverse(cam[34:50].reshape(4, 4)),
                               depth_a, depth_b, uv_a, gt, pred, pred_masked)


def synthetic_store(device, h, w, seed=0, still_scene=True):
    """Two objects: object 0 with a moving scene (4 frames, 6 cm apart) and, optionally, a scene whose frames all coincide;
    object 1 with one moving scene.  A wavy wall around 0.9 m (no-return holes), rectangular masks, the default K scaled to
    the image, random RGB."""
    from dcn_hip import frames
    rng = np.random.RandomState(seed)

    def pose(t):
        T = np.eye(4)
        T[:3, 3] = t
        return T
    s = 0.06                       # (about 5.6 % of the image width at 0.9 m)
    moving = [pose(t) for t in ([0, 0, 0], [s, 0, 0], [0, s, 0], [s, s, 0.01])]
    poses = moving + ([pose([0.1, 0, 0])] * 3 if still_scene else []) + moving
    first = [0, 4, 7, 11] if still_scene else [0, 4, 8]
    sobj = [0, 0, 1] if still_scene else [0, 1]
    F = len(poses)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = np.stack([900 + 40 * np.sin(xs / (0.1 * w) + f) + 30 * np.cos(ys / (0.12 * h) - f) for f in range(F)])
    depth[rng.rand(F, h, w) < 0.03] = 0
    depth = depth.astype(np.uint16)
    mask = np.zeros((F, h, w), np.uint8)
    mask[:, h // 5:4 * h // 5, w // 6:5 * w // 6] = 1
    rgb = rng.randint(0, 256, (F, h, w, 3)).astype(np.uint8)
    K = np.array([[533.6 * w / 640.0, 0, 0.5 * w - 0.3], [0, 534.8 * h / 480.0, 0.5 * h + 0.2], [0, 0, 1.0]])
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return frames.FrameStore.from_tensors(c(rgb), c(depth.view(np.int16)), c(mask), np.stack(poses), first, sobj, K)


def numpy_choose_pairs(store, n, rng, threshold=0.05, max_num_attempts=100):
    """The reference's per-pair rule restated on the store's host tables (see evaluate.choose_pairs)"""
    first = np.asarray(store.scene_first_frame_host)
    poses = store.poses.cpu().numpy().reshape(-1, 4, 4)
    multi, per_object = store.multi_scenes_host, store.object_scenes_host
    out = []
    for _ in range(n):
        k = rng.randint(len(multi) + len(per_object))
        if k < len(multi):
            s = multi[rng.randint(len(multi))]
        else:
            scenes = per_object[rng.randint(len(per_object))]
            s = scenes[rng.randint(len(scenes))]
        cnt = first[s + 1] - first[s]
        a = first[s] + rng.randint(cnt)
        for _i in range(max_num_attempts):
            b = first[s] + rng.randint(cnt)
            if np.linalg.norm(poses[a][0:3, 3] - poses[b][0:3, 3]) > threshold:
                out.append((s, a, b))
                break
    return np.asarray(out, np.int64).reshape(-1, 3)
