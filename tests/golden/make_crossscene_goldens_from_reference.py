"""Pins the cross-scene evaluation (csrc/crossscene_kernels.hip, dcn_hip/evaluate/cross_scene.py): executes the REFERENCE's own source
text -- read from /root/reference at run time, never copied --
  dense_correspondence/evaluation/evaluation.py single_cross_scene_image_pair_quantitative_analysis (:610-781; the Python-2
  text converted in memory by lib2to3, as tests/reference_py3.py converts modules)
  what make_evalpairs_goldens_from_reference.load_reference binds: compute_descriptor_match_statistics' body (:1045-1175),
  clip_pixel_to_image_size_and_round, find_best_match, DCNEvaluationPandaTemplate, correspondence_finder's search
  SpartanDataset.get_img_idx_with_different_pose (dense_correspondence_dataset_masked.py:260-287) and get_random_image_index
  (spartan_dataset_masked.py:408-420), bound to a stub dataset by subclassing
against a stub dataset of two synthetic scenes (analytic depth with no-return holes; frames far from the labelled image, which
are drawn as views, and frames near it, which fail the 0.2 m test) and a stub network that returns stored descriptor images.
``round`` is bound to Python 2's (half away from zero).  J = K = 10 as hard-coded there; I = 3 labels, so that image b's group
has 3 + 30 rows at most, one more than the statistics kernel's query tile.

Stores, in tests/golden/crossscene_ref_*.npz: the scenes (poses, K, depth, masks, the descriptor images as int16 multiples of
``res_scale``), the labels, every view request (the frame the reference drew or -1 for None, whether the search found the
pixel, the raw projection) and every output row in the reference's order.  Frames the reference never loads have no images.

Poses: scene a's are fp32-representable (the device's camera rows carry pose a in fp32) with general rotations: its views
turn about the point the labelled image's central pixel sees.  Scene b's are the poses their fp32 inverse represents (as
make_evalpairs_goldens_from_reference: the rows carry pose b^-1), and the generator requires that inverting them again the
device's way gives that fp32 inverse back exactly -- an fp32 rotation is orthonormal to 1e-8 only, so scene b keeps ONE exactly
orthonormal rotation (a quarter turn) and its views withdraw along the central pixel's ray instead.  (A general pose b in the
3D columns is what the evalpairs goldens pin; a general inverse is exercised here by the a-views' reprojection.)  K is
fp32-representable.

The generator ASSERTS, from the reference's results alone, that the case is meaningful (see ``check``) and takes the first
seed that passes.

    python tests/golden/make_crossscene_goldens_from_reference.py
"""
import logging
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_evalpairs_goldens_from_reference as me                                   # noqa: E402
import make_sample_goldens_from_reference as ms                                      # noqa: E402
import reference_py3 as rp                                                           # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

COLUMNS = me.COLUMNS
NUM_LABELS, J, K_VIEWS = 3, 10, 10
RES_SCALE = 1.0 / 4096.0
NO_VIEW, NO_MATCH, FOUND = 0, 1, 2


def rotation(axis, angle):
    """Rodrigues"""
    n = np.asarray(axis, np.float64)
    n = n / np.linalg.norm(n)
    X = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * X + (1 - np.cos(angle)) * X.dot(X)


def device_inverse32(T):
    """The rigid inverse as the device's camera rows carry it: R^T, -(R^T t) summed left to right in float64, then fp32"""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    for i in range(3):
        s = T[0, i] * T[0, 3]
        s = s + T[1, i] * T[1, 3]
        s = s + T[2, i] * T[2, 3]
        out[i, 3] = -s
    return me.f32(out)


def pivot_ray(cf, h, w):
    """The point the central pixel sees at 0.9 m, in camera coordinates (the default K's, which the reprojection uses)"""
    return 0.9 * np.linalg.inv(cf.get_default_K_matrix()).dot([0.5 * w, 0.5 * h, 1.0])


def turned_poses(rng, cf, h, w, base, n_near, n_far):
    """The labelled image's pose, then ``n_near`` poses that fail get_img_idx_with_different_pose's test against it and
    ``n_far`` that pass: the camera turned about the point its central pixel sees at 0.9 m, so that the view still shows it"""
    pivot = base[:3, :3].dot(pivot_ray(cf, h, w)) + base[:3, 3]
    main = [1.0, 0, 0] if w == 1 else [0, 1.0, 0]         # (a 1-pixel-wide image keeps x / z only under a turn about x)
    poses = [base]
    for far in [False] * n_near + [True] * n_far:
        ang = np.deg2rad(rng.uniform(12.5, 16.0) if far else rng.uniform(0.3, 2.5)) * rng.choice([-1, 1])
        R = rotation(np.asarray(main) + 0.04 * rng.randn(3), ang)
        T = np.eye(4)
        T[:3, :3] = R.dot(base[:3, :3])
        T[:3, 3] = R.dot(base[:3, 3] - pivot) + pivot
        T[:3, 3] += T[:3, :3].dot([0, 0, rng.uniform(-0.006, 0.004)])      # a few millimetres along the optical axis
        poses.append(T)
    return poses, [0.0] * len(poses)


def withdrawn_poses(rng, cf, h, w, base, n_near, n_far):
    """As turned_poses, but the rotation stays the labelled image's: near frames a few centimetres beside it, far frames
    0.21 .. 0.3 m back along the central pixel's ray (the view still shows that point, smaller) -> (poses, how much farther
    the scene is from each)"""
    ray = pivot_ray(cf, h, w)
    ray = ray / np.linalg.norm(ray)
    poses, back = [base], [0.0]
    for far in [False] * n_near + [True] * n_far:
        T = base.copy()
        if far:
            s = rng.uniform(0.21, 0.3)
            T[:3, 3] += base[:3, :3].dot(-s * ray + 0.003 * rng.randn(3))
            back.append(s * ray[2])
        else:
            T[:3, 3] += base[:3, :3].dot(0.03 * rng.randn(3))
            back.append(0.0)
        poses.append(T)
    return poses, back


def make_scenes(cf, h, w, D, seed):
    rng = np.random.RandomState(seed)
    base_a = ms.pose(0.01, -0.02, [0.1, -0.05, 0.02])
    base_b = np.array([[0, -1.0, 0, -0.2], [1.0, 0, 0, 0.03], [0, 0, 1.0, 0.3], [0, 0, 0, 1.0]])    # a quarter turn about z
    # scene a: 3 near, 6 far; scene b: 60 near and 2 far -- 50 attempts there fail now and then, and a far frame is drawn twice
    pa, back_a = turned_poses(rng, cf, h, w, base_a, 3, 6)
    pa = [me.f32(T).astype(np.float64) for T in pa]
    pb, back_b = withdrawn_poses(rng, cf, h, w, base_b, 60, 2)
    inv32 = [me.f32(me.invert_rigid(T)) for T in pb]
    pb = [me.invert_rigid(t.astype(np.float64)) for t in inv32]
    for T, t in zip(pb, inv32):
        assert np.array_equal(device_inverse32(T), t), "a scene b pose is not the fixed point of the device's inverse"
    poses = np.stack(pa + pb)
    first = [0, len(pa), len(pa) + len(pb)]
    F = first[-1]
    ids = [[100 + 3 * j for j in range(len(pa))], [7 + 2 * j for j in range(len(pb))]]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = np.zeros((F, h, w), np.uint16)
    mask = np.zeros((F, h, w), np.uint8)
    for f, back in enumerate(back_a + back_b):
        d = 900 + 1000 * back + 25 * np.sin(xs / (6 + 4 * rng.rand())) + 20 * np.cos(ys / (5 + 3 * rng.rand())) + 30 * rng.rand()
        d[rng.rand(h, w) < 0.05] = 0
        depth[f] = d.astype(np.uint16)
        cy, cx = 0.5 + 0.1 * rng.rand(), 0.45 + 0.1 * rng.rand()
        mask[f] = (((ys - cy * h) / (0.3 * h + 0.6)) ** 2 + ((xs - cx * w) / (0.3 * w + 0.6)) ** 2 <= 1.0).astype(np.uint8)
    base = rng.randn(h, w, D)
    res_q = np.round((base[None] + 0.35 * np.sqrt(D / 3.0) * rng.randn(F, h, w, D)) / RES_SCALE).astype(np.int16)
    Kd = cf.get_default_K_matrix()
    K = np.array([[Kd[0, 0] * 0.9, 0, Kd[0, 2] + 1.5], [0, Kd[1, 1] * 0.9, Kd[1, 2] - 2.0], [0, 0, 1.0]])
    return dict(poses=poses, first=first, ids=ids, depth=depth, mask=mask, res_q=res_q, K=me.f32(K).astype(np.float64))


def make_labels(rng, sc, h, w):
    """Three labelled matches: one next to the last row and column (its views' projections leave the image or round up at the
    clip), one around the middle with fractional coordinates (a .5 included: Python 2's round), one on a pixel of image a
    without a depth return"""
    fa, fb = 0, sc["first"][1]
    mid = lambda n: n // 2 + int(rng.randint(-(n // 6), n // 6 + 1)) if n > 1 else 0
    px = [[mid(w), mid(h), mid(w), mid(h)] for _ in range(NUM_LABELS)]
    px[0] = [max(w - 2, 0), max(h - 2, 0), max(w - 3, 0), max(h - 2, 0)]
    px[1] = [px[1][0] + (0.5 if w > 2 else 0.0), px[1][1] - (0.25 if h > 2 else 0.0), px[1][2] + 0.3 * (w > 2),
             px[1][3] + (0.5 if h > 2 else 0.0)]
    holes = np.argwhere(sc["depth"][fa] == 0)
    assert len(holes), "image a has no pixel without a depth return"
    centre = np.abs(holes[:, 0] - h // 2) * w + np.abs(holes[:, 1] - w // 2)
    v0, u0 = holes[np.argmin(centre)]
    px[2][0], px[2][1] = int(u0), int(v0)
    return px


def load_function(ev_lines):
    """The reference's single_cross_scene_image_pair_quantitative_analysis, its text converted in memory"""
    text = me.method_source(ev_lines, "single_cross_scene_image_pair_quantitative_analysis")
    return compile(str(rp._refactoring_tool().refactor_string(text + "\n", me.EVAL)), me.EVAL, "exec")


def case(ref, fn_code, sdm, name, h, w, D, seed):
    cf, DCE0, block, env0, read = ref
    sc = make_scenes(cf, h, w, D, seed)
    rng = np.random.RandomState(seed + 1000)
    px = make_labels(rng, sc, h, w)
    first, ids, poses = sc["first"], sc["ids"], sc["poses"]
    names = ["scene_a", "scene_b"]
    res = sc["res_q"].astype(np.float32) * np.float32(RES_SCALE)
    frame_of = lambda scene, idx: first[names.index(scene)] + ids[names.index(scene)].index(int(idx))
    loaded = np.zeros(first[-1], bool)
    requests, rows, extras = [], [], []

    class Dataset(sdm.SpartanDataset):
        def __init__(self):                    # (no scene files)
            self.debug, self.mode = False, "train"

        def get_pose_data(self, scene_name):
            s = names.index(scene_name)
            return dict((i, None) for i in ids[s])

        def get_pose_from_scene_name_and_idx(self, scene_name, idx):
            return poses[frame_of(scene_name, idx)]

        def get_rgbd_mask_pose(self, scene_name, idx):
            f = frame_of(scene_name, idx)
            loaded[f] = True
            return f, sc["depth"][f], sc["mask"][f], poses[f]

        def rgb_image_to_tensor(self, rgb):
            return rgb

        def get_camera_intrinsics(self, scene_name=None):
            return type("Intrinsics", (object,), {"K": sc["K"]})()

        def get_img_idx_with_different_pose(self, scene_name, pose, **kw):
            idx = sdm.SpartanDataset.get_img_idx_with_different_pose(self, scene_name, pose, **kw)
            requests.append(dict(side=1 + names.index(scene_name), frame=-1 if idx is None else frame_of(scene_name, idx),
                                 outcome=NO_VIEW, u=0.0, v=0.0))
            return idx

    class Descriptors(object):
        """``.data.cpu().numpy()`` of a stored descriptor image"""

        def __init__(self, a):
            self.a, self.data = a, self

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    class Network(object):
        image_shape = (h, w)

        def forward_single_image_tensor(self, f):
            return Descriptors(res[f])

    class Finder(object):
        @staticmethod
        def batch_find_pixel_correspondences(depth_a, pose_a, depth_b, pose_b, uv_a=None):
            got = cf.batch_find_pixel_correspondences(depth_a, pose_a, depth_b, pose_b, uv_a=uv_a)
            r = requests[-1]
            r["src_uv"] = uv_a
            if got[0] is None or got[0][0].numel() == 0:
                r["outcome"] = NO_MATCH
            else:
                r["outcome"], r["u"], r["v"] = FOUND, float(got[1][0][0]), float(got[1][1][0])
            return got

    class Row(object):
        """What compute_descriptor_match_statistics returns here: the reference's template plus what the test compares"""

        def __init__(self, template, env):
            self.t, self.extra = template, {}
            self.env = {k: env[k] for k in ("uv_b_pred", "uv_b_pred_masked", "num_pixels_closer_than_ground_truth",
                                            "num_pixels_closer_than_ground_truth_masked", "uv_a", "uv_b")}
            for k, nd in (("gap", env["norm_diffs"]), ("gap_masked", env["masked_norm_diffs"])):
                two = np.sort(np.asarray(nd, np.float64).reshape(-1))[:2]
                self.env[k] = (two[1] - two[0]) / two[1] if len(two) == 2 else 1.0
            self.env["search"] = env["search_frame"]
            self.request = len(requests) - 1 if env["after_labels"][0] else -1

        def set_value(self, key, value):
            self.extra[key] = value

        dataframe = property(lambda self: self)

    after_labels = [False]

    def statistics(depth_a, depth_b, mask_a, mask_b, uv_a, uv_b, pose_a, pose_b, res_a, res_b, camera_matrix, params=None,
                   rgb_a=None, rgb_b=None, debug=False):
        env = dict(env0, depth_a=depth_a, depth_b=depth_b, mask_a=mask_a, mask_b=mask_b, uv_a=uv_a, uv_b=uv_b, pose_a=pose_a,
                   pose_b=pose_b, res_a=res_a, res_b=res_b, camera_matrix=camera_matrix)
        exec(block, env)
        env["search_frame"], env["after_labels"] = int(rgb_b), after_labels
        return Row(env["pd_template"], env)

    class DCE(DCE0):
        compute_descriptor_match_statistics = staticmethod(statistics)

    ds = Dataset()
    orig = ds.get_img_idx_with_different_pose

    def first_view(*a, **k):
        after_labels[0] = True
        return orig(*a, **k)
    ds.get_img_idx_with_different_pose = first_view
    ns = {"np": np, "DenseCorrespondenceEvaluation": DCE, "correspondence_finder": Finder, "logging": logging,
          "round": me.py2_round}
    exec(fn_code, ns)
    random.seed(seed)
    torch.manual_seed(seed)
    pixels = lambda c: [{"u": p[c], "v": p[c + 1]} for p in px]
    out = ns["single_cross_scene_image_pair_quantitative_analysis"](Network(), ds, names[0], ids[0][0], names[1], ids[1][0],
                                                                    pixels(0), pixels(2))
    # ---- pack
    z = dict(h=np.array(h), w=np.array(w), D=np.array(D), K=sc["K"], poses=poses, first=np.array(first, np.int64),
             frame_ids=np.array(ids[0] + ids[1], np.int64), loaded=loaded, res_scale=np.array(RES_SCALE),
             depth=np.where(loaded[:, None, None], sc["depth"], 0).astype(np.uint16),
             mask=np.where(loaded[:, None, None], sc["mask"], 0).astype(np.uint8),
             res_q=np.where(loaded[:, None, None, None], sc["res_q"], 0).astype(np.int16),
             label_pixels=np.array(px, np.float64), frame_a=np.array(0), frame_b=np.array(first[1]),
             scene_names=np.array(names), columns=np.array(COLUMNS))
    z["request_side"] = np.array([r["side"] for r in requests], np.int64)
    z["request_label"] = np.repeat(np.arange(NUM_LABELS), J + K_VIEWS).astype(np.int64)
    z["request_frame"] = np.array([r["frame"] for r in requests], np.int64)
    z["request_outcome"] = np.array([r["outcome"] for r in requests], np.int64)
    z["request_u"] = np.array([r["u"] for r in requests], np.float32)
    z["request_v"] = np.array([r["v"] for r in requests], np.float32)
    assert len(requests) == NUM_LABELS * (J + K_VIEWS), len(requests)
    assert [r["side"] for r in requests] == ([1] * J + [2] * K_VIEWS) * NUM_LABELS
    rows_out = {k: [] for k in COLUMNS}
    ints = {k: [] for k in ("row_request", "search_frame", "u_a", "v_a", "gt_u", "gt_v", "pred_u", "pred_v", "pred_u_masked",
                            "pred_v_masked", "closer", "closer_masked", "img_a_idx", "img_b_idx")}
    flags, gaps, scene_name = {"is_valid": [], "is_valid_masked": []}, {"gap": [], "gap_masked": []}, []
    for r in out:
        for k in COLUMNS:
            rows_out[k].append(float(read(r.t, k)))
        for k in flags:
            flags[k].append(bool(read(r.t, k)))
        for k in gaps:
            gaps[k].append(r.env[k])
        scene_name.append(r.extra["scene_name"])
        for k, val in (("row_request", r.request), ("search_frame", r.env["search"]), ("u_a", r.env["uv_a"][0]),
                       ("v_a", r.env["uv_a"][1]), ("gt_u", r.env["uv_b"][0]), ("gt_v", r.env["uv_b"][1]),
                       ("pred_u", r.env["uv_b_pred"][0]), ("pred_v", r.env["uv_b_pred"][1]),
                       ("pred_u_masked", r.env["uv_b_pred_masked"][0]), ("pred_v_masked", r.env["uv_b_pred_masked"][1]),
                       ("closer", r.env["num_pixels_closer_than_ground_truth"]),
                       ("closer_masked", r.env["num_pixels_closer_than_ground_truth_masked"]),
                       ("img_a_idx", r.extra["img_a_idx"]), ("img_b_idx", r.extra["img_b_idx"])):
            ints[k].append(int(val))
    for k, val in rows_out.items():
        z[k] = np.asarray(val, np.float64)
    for k, val in ints.items():
        z[k] = np.asarray(val, np.int64)
    for k, val in flags.items():
        z[k] = np.asarray(val, bool)
    for k, val in gaps.items():
        z[k] = np.asarray(val, np.float64)
    z["scene_name"] = np.array(scene_name)
    check(name, z, cf)
    write_npz(os.path.join(HERE, "crossscene_ref_%s.npz" % name), z)
    return "rows %d, outcomes (none, no match, found) %s, group of image b %d rows, %d frames loaded" % (
        len(z["row_request"]), np.bincount(z["request_outcome"], minlength=3).tolist(),
        int((z["search_frame"] == z["frame_b"]).sum()), int(loaded.sum()))


def margins(z, cf):
    """Per view request whose source pixel has depth: how far its projection is from the nearest bound of the field-of-view
    test, pixels, and, when it is inside, how far the occlusion decision is from its margin, metres (a float64 restatement of
    the search's tests, used for these distances only) -> (occlusion, field of view)"""
    Kd = cf.get_default_K_matrix()
    h, w = int(z["h"]), int(z["w"])
    out, edge = [], []
    for q in range(len(z["request_side"])):
        if z["request_frame"][q] < 0:
            continue
        side = int(z["request_side"][q])
        src = int(z["frame_a"] if side == 1 else z["frame_b"])
        lp = z["label_pixels"][z["request_label"][q]]
        u = min(me.py2_round(lp[0 if side == 1 else 2]), w - 1)
        v = min(me.py2_round(lp[1 if side == 1 else 3]), h - 1)
        d = z["depth"][src][v, u] / 1000.0
        if d == 0:
            continue
        pc = d * np.linalg.inv(Kd).dot([u, v, 1.0])
        pw = z["poses"][src][:3, :3].dot(pc) + z["poses"][src][:3, 3]
        dst = z["poses"][z["request_frame"][q]]
        p2 = dst[:3, :3].T.dot(pw - dst[:3, 3])
        uv = Kd.dot(p2)
        u2, v2 = uv[0] / uv[2], uv[1] / uv[2]
        edge.append(min(abs(u2), abs(u2 - (w - 1e-3)), abs(v2), abs(v2 - (h - 1e-3))))
        if not (0 < u2 <= w - 1e-3 and 0 < v2 <= h - 1e-3):
            continue
        d2 = z["depth"][z["request_frame"][q]][int(v2), int(u2)] / 1000.0
        out.append(abs(d2 - (p2[2] - 0.003)) if d2 > 0 else 1.0)
    return np.asarray(out), np.asarray(edge)


def check(name, z, cf):
    """What makes the comparison meaningful, from the reference's results alone"""
    h, w = int(z["h"]), int(z["w"])
    oc, side = z["request_outcome"], z["request_side"]
    assert (oc == NO_VIEW).any(), (name, "no view request returned None")
    assert ((oc == NO_VIEW) == (z["request_frame"] < 0)).all()
    for s in (1, 2):
        assert ((oc == NO_MATCH) & (side == s)).any(), (name, "every reprojection succeeds on side %d" % s)
        assert ((oc == FOUND) & (side == s)).any(), (name, "no reprojection succeeds on side %d" % s)
    b_views = z["request_frame"][(side == 2) & (oc != NO_VIEW)]
    assert len(set(b_views.tolist())) < len(b_views), (name, "no b-view frame drawn twice")
    fu, fv = z["request_u"][oc == FOUND], z["request_v"][oc == FOUND]
    up = (np.array([me.py2_round(x) for x in fu]) > w - 1) | (np.array([me.py2_round(x) for x in fv]) > h - 1)
    assert up.any(), (name, "no projection rounds up into the last row or column")
    lab = np.array([[min(me.py2_round(p[0]), w - 1), min(me.py2_round(p[1]), h - 1)] for p in z["label_pixels"]])
    assert (z["depth"][int(z["frame_a"])][lab[:, 1], lab[:, 0]] == 0).any(), (name, "no label on a pixel without depth")
    assert (~z["is_valid"]).any(), (name, "no row with an invalid predicted depth")
    ok = ~np.isnan(z["norm_diff_ground_truth_3d"]) & ~np.isnan(z["norm_diff_pred_3d"]) & ~np.isnan(z["norm_diff_pred_3d_masked"])
    assert ok.any(), (name, "no row with all three 3D columns valid")
    assert ((z["pred_u"] != z["pred_u_masked"]) | (z["pred_v"] != z["pred_v_masked"])).any(), (name, "masked == image everywhere")
    assert z["gap"].min() > 1e-4 and z["gap_masked"].min() > 1e-4, (name, z["gap"].min(), z["gap_masked"].min())
    for x in np.concatenate([fu, fv]):
        assert abs((x % 1.0) - 0.5) > 1e-3, (name, "a projection within 1e-3 pixel of a half-integer", x)
    m, edge = margins(z, cf)
    assert len(m) and m.min() > 1e-5, (name, "an occlusion decision within 1e-5 m of its margin", m.min())
    assert edge.min() > 1e-4, (name, "a projection within 1e-4 pixel of a bound of the field of view", edge.min())
    # the group of image b: the labelled rows and every a-view row
    assert (z["search_frame"] == z["frame_b"]).sum() == NUM_LABELS + ((oc == FOUND) & (side == 1)).sum()
    assert len(z["row_request"]) == NUM_LABELS + (oc == FOUND).sum()


def main():
    ref = me.load_reference()
    import dense_correspondence.dataset.spartan_dataset_masked as sdm
    fn_code = load_function(open(me.EVAL).read().split("\n"))
    logging.disable(logging.CRITICAL)
    only = sys.argv[1:]
    # seeds: the first (from 1 up) for which the reference's results pass ``check``
    for name, h, w, D in (("48x64_d3", 48, 64, 3), ("37x53_d16", 37, 53, 16), ("1x64_d1", 1, 64, 1), ("48x1_d1", 48, 1, 1)):
        if only and name not in only:
            continue
        for seed in range(1, 400):
            try:
                sys.stdout, keep = open(os.devnull, "w"), sys.stdout         # (the reference prints every label and pixel)
                try:
                    said = case(ref, fn_code, sdm, name, h, w, D, seed)
                finally:
                    sys.stdout.close()
                    sys.stdout = keep
                print(name, "seed", seed, said)
                break
            except AssertionError as e:
                print(name, "seed", seed, "rejected:", e)
        else:
            raise SystemExit("no seed passes for " + name)


if __name__ == "__main__":
    main()
