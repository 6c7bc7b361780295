"""Pins the class-consistent keypoint evaluation (dcn_hip/evaluate/keypoints.py: keypoint_labels, keypoint_rows, evaluate_keypoint_rows,
keypoint_table; csrc/crossscene_kernels.hip's wide statistics kernel): executes the REFERENCE's own source text -- read from
/root/reference at run time, never copied --
  dense_correspondence/evaluation/evaluation.py single_image_pair_cross_scene_keypoints_quantitative_analysis (:1433-1552; the
  Python-2 text converted in memory by lib2to3, as tests/reference_py3.py converts modules)
  what make_evalpairs_goldens_from_reference.load_reference binds: compute_descriptor_match_statistics' body (:1045-1175),
  clip_pixel_to_image_size_and_round, find_best_match, DCNEvaluationPandaTemplate
over ``itertools.combinations`` of the labelled images with the descriptor images handed in, as
evaluate_network_cross_scene_keypoints (:407-472) does, against a stub dataset and stub descriptor images.  ``round`` is bound
to Python 2's (half away from zero).

A case: 4 labelled images in 3 scenes -- images 0 and 1 share scene_a; scene_a and scene_c have the same K, scene_b another --
with 3 keypoints each (the last image has one more, which the reference ignores): 6 combinations x 3 keypoints x 2 orders = 36
rows, 9 per searched image.  Descriptor images are int16 multiples of ``res_scale``; depth comes from smooth surfaces with
no-return holes.  The labels hold a half-integer coordinate and one beyond the image's edge, which clips.

Poses: every labelled image is image 1 of some rows and image 2 of others, so its pose must be fp32-representable (the device's
camera rows carry pose 1 in fp32) AND equal the pose its fp32 inverse represents (they carry pose 2^-1): rotations are signed
permutations (quarter turns) and translations multiples of 2^-10 m, for which the rigid inverse is exact in fp32.  (General
poses on either side are what the evalpairs and crossscene goldens pin.)  Both K are fp32-representable.

Stores, in tests/golden/keypoints_ref_*.npz: the scenes, the annotations and every output row in the reference's order.  The
generator ASSERTS, from the reference's results alone, that the case is meaningful (see ``check``) and takes the first seed
that passes.

    python tests/golden/make_keypoints_goldens_from_reference.py
"""
import collections
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_evalpairs_goldens_from_reference as me                                   # noqa: E402
import reference_py3 as rp                                                           # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

COLUMNS = me.COLUMNS
RES_SCALE = 1.0 / 4096.0
FUNCTION = "single_image_pair_cross_scene_keypoints_quantitative_analysis"
SCENES = ["scene_a", "scene_b", "scene_c"]
FIRST = [0, 3, 5, 7]                           # frames per scene: 3, 2, 2
LABELLED = [(0, 0), (0, 2), (1, 1), (2, 0)]   # (scene, frame of it) of the four labelled images
OBJECTS = ["shoe_red_nike", "shoe_red_nike", "shoe_green_nike", "shoe_brown"]
NAMES = ["toe", "heel", "top_of_shoelaces"]
QUARTER_TURNS = [np.eye(3), [[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]], [[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]],
                 [[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]]]


def make_scenes(cf, h, w, D, seed):
    rng = np.random.RandomState(seed)
    F = FIRST[-1]
    poses = np.stack([np.eye(4)] * F)
    for f in range(F):
        poses[f, :3, :3] = QUARTER_TURNS[rng.randint(len(QUARTER_TURNS))]
        poses[f, :3, 3] = rng.randint(-300, 301, 3) / 1024.0
    for T in poses:                                         # exact on both sides of a camera row
        assert np.array_equal(me.f32(T).astype(np.float64), T)
        assert np.array_equal(me.invert_rigid(me.f32(me.invert_rigid(T)).astype(np.float64)), T)
    ids = [[100 + 3 * j for j in range(3)], [7 + 2 * j for j in range(2)], [40 + j for j in range(2)]]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = np.zeros((F, h, w), np.uint16)
    mask = np.zeros((F, h, w), np.uint8)
    for f in range(F):
        d = 900 + 25 * np.sin(xs / (6 + 4 * rng.rand())) + 20 * np.cos(ys / (5 + 3 * rng.rand())) + 30 * rng.rand()
        d[rng.rand(h, w) < 0.15] = 0
        depth[f] = d.astype(np.uint16)
        cy, cx = 0.5 + 0.1 * rng.rand(), 0.45 + 0.1 * rng.rand()
        mask[f] = (((ys - cy * h) / (0.3 * h + 0.6)) ** 2 + ((xs - cx * w) / (0.3 * w + 0.6)) ** 2 <= 1.0).astype(np.uint8)
    base = rng.randn(h, w, D)
    res_q = np.round((base[None] + 0.6 * np.sqrt(D / 3.0) * rng.randn(F, h, w, D)) / RES_SCALE).astype(np.int16)
    Kd = cf.get_default_K_matrix()
    Kb = np.array([[Kd[0, 0] * 0.9, 0, Kd[0, 2] + 1.5], [0, Kd[1, 1] * 0.9, Kd[1, 2] - 2.0], [0, 0, 1.0]])
    K = np.stack([me.f32(Kd), me.f32(Kb), me.f32(Kd)]).astype(np.float64)
    return dict(poses=poses, ids=ids, depth=depth, mask=mask, res_q=res_q, K=K)


def make_annotations(rng, sc, h, w):
    """The reference's list of dicts: keypoints spread over the image with fractional coordinates; image 0's first keypoint
    on a half-integer, image 1's second beyond the last column and row (it clips), the last image with a name more"""
    out = []
    for i, (s, j) in enumerate(LABELLED):
        kps = collections.OrderedDict()
        for k, name in enumerate(NAMES):
            u = float(rng.randint(0, w)) + (float(rng.randint(0, 4)) * 0.25 if w > 1 else 0.0)
            v = float(rng.randint(0, h)) + (float(rng.randint(0, 4)) * 0.25 if h > 1 else 0.0)
            if i == 0 and k == 0:
                u, v = (np.floor(u) + 0.5 if w > 1 else 0.5), (np.floor(v) + 0.5 if h > 1 else 0.0)
            if i == 1 and k == 1:
                u, v = w + 0.7, h + 1.2
            kps[name] = {"keypoint": name, "u": u, "v": v}
        if i == len(LABELLED) - 1:
            kps["extra"] = {"keypoint": "extra", "u": 0.0, "v": 0.0}
        out.append({"scene_name": SCENES[s], "image_idx": sc["ids"][s][j], "object_id": OBJECTS[i], "keypoints": kps})
    return out


def load_function(ev_lines):
    text = me.method_source(ev_lines, FUNCTION)
    return compile(str(rp._refactoring_tool().refactor_string(text + "\n", me.EVAL)), me.EVAL, "exec")


def case(ref, fn_code, name, h, w, D, seed):
    cf, DCE0, block, env0, read = ref
    sc = make_scenes(cf, h, w, D, seed)
    ann = make_annotations(np.random.RandomState(seed + 1000), sc, h, w)
    res = sc["res_q"].astype(np.float32) * np.float32(RES_SCALE)
    frame_of = lambda scene, idx: FIRST[SCENES.index(scene)] + sc["ids"][SCENES.index(scene)].index(int(idx))

    class Dataset(object):
        def get_rgbd_mask_pose(self, scene_name, idx):
            f = frame_of(scene_name, idx)
            return f, sc["depth"][f], sc["mask"][f], sc["poses"][f]

        def get_camera_intrinsics(self, scene_name=None):
            return type("Intrinsics", (object,), {"K": sc["K"][SCENES.index(scene_name)]})()

    class Network(object):
        image_shape = (h, w)

    class Row(object):
        """What compute_descriptor_match_statistics returns here: the reference's template plus what the test compares"""

        def __init__(self, template, env, other_k):
            self.t, self.extra, self.other_k = template, {}, other_k
            self.env = {k: env[k] for k in ("uv_b_pred", "uv_b_pred_masked", "num_pixels_closer_than_ground_truth",
                                            "num_pixels_closer_than_ground_truth_masked", "uv_a", "uv_b")}
            for k, nd in (("gap", env["norm_diffs"]), ("gap_masked", env["masked_norm_diffs"])):
                two = np.sort(np.asarray(nd, np.float64).reshape(-1))[:2]
                self.env[k] = (two[1] - two[0]) / two[1] if len(two) == 2 and two[1] > 0 else 1.0
            self.env["query"], self.env["search"] = env["query_frame"], env["search_frame"]

        def set_value(self, key, value):
            self.extra[key] = value

        dataframe = property(lambda self: self)

    def statistics(depth_a, depth_b, mask_a, mask_b, uv_a, uv_b, pose_a, pose_b, res_a, res_b, camera_matrix, params=None,
                   rgb_a=None, rgb_b=None, debug=False):
        run = lambda K: dict(env0, depth_a=depth_a, depth_b=depth_b, mask_a=mask_a, mask_b=mask_b, uv_a=uv_a, uv_b=uv_b,
                             pose_a=pose_a, pose_b=pose_b, res_a=res_a, res_b=res_b, camera_matrix=K)
        env = run(camera_matrix)
        exec(block, env)
        env["query_frame"], env["search_frame"] = int(rgb_a), int(rgb_b)
        # the same row under the K of the other image's scene (for a reverse row: what a K chosen per order would give)
        scene_of = lambda f: int(np.searchsorted(FIRST, int(f), side="right") - 1)
        Ks = [sc["K"][scene_of(rgb_a)], sc["K"][scene_of(rgb_b)]]
        other = run(Ks[1] if np.array_equal(Ks[0], camera_matrix) else Ks[0])
        exec(block, other)
        return Row(env["pd_template"], env, [float(read(other["pd_template"], k)) for k in COLUMNS[3:6]])

    class DCE(DCE0):
        compute_descriptor_match_statistics = staticmethod(statistics)

    ns = {"np": np, "DenseCorrespondenceEvaluation": DCE, "round": me.py2_round}
    exec(fn_code, ns)
    out = []
    for a, b in itertools.combinations(ann, 2):           # evaluate_network_cross_scene_keypoints, :447-461
        out += ns[FUNCTION](Network(), Dataset(), a, b, res[frame_of(a["scene_name"], a["image_idx"])],
                            res[frame_of(b["scene_name"], b["image_idx"])])
    # ---- pack
    flat = [(i, n, kp["u"], kp["v"]) for i, an in enumerate(ann) for n, kp in an["keypoints"].items()]
    z = dict(h=np.array(h), w=np.array(w), D=np.array(D), K=sc["K"], poses=sc["poses"], first=np.array(FIRST, np.int64),
             frame_ids=np.array(sum(sc["ids"], []), np.int64), scene_names=np.array(SCENES), res_scale=np.array(RES_SCALE),
             depth=sc["depth"], mask=sc["mask"], res_q=sc["res_q"], columns=np.array(COLUMNS),
             ann_scene_name=np.array([an["scene_name"] for an in ann]), ann_image_idx=np.array([an["image_idx"] for an in ann]),
             ann_object_id=np.array([an["object_id"] for an in ann]), kp_image=np.array([f[0] for f in flat], np.int64),
             kp_name=np.array([f[1] for f in flat]), kp_u=np.array([f[2] for f in flat], np.float64),
             kp_v=np.array([f[3] for f in flat], np.float64))
    for k in COLUMNS:
        z[k] = np.asarray([float(read(r.t, k)) for r in out], np.float64)
    for k in ("is_valid", "is_valid_masked"):
        z[k] = np.asarray([bool(read(r.t, k)) for r in out], bool)
    ints = (("query_frame", lambda r: r.env["query"]), ("search_frame", lambda r: r.env["search"]),
            ("u_a", lambda r: r.env["uv_a"][0]), ("v_a", lambda r: r.env["uv_a"][1]), ("gt_u", lambda r: r.env["uv_b"][0]),
            ("gt_v", lambda r: r.env["uv_b"][1]), ("pred_u", lambda r: r.env["uv_b_pred"][0]),
            ("pred_v", lambda r: r.env["uv_b_pred"][1]), ("pred_u_masked", lambda r: r.env["uv_b_pred_masked"][0]),
            ("pred_v_masked", lambda r: r.env["uv_b_pred_masked"][1]),
            ("closer", lambda r: r.env["num_pixels_closer_than_ground_truth"]),
            ("closer_masked", lambda r: r.env["num_pixels_closer_than_ground_truth_masked"]),
            ("img_a_idx", lambda r: r.extra["img_a_idx"]), ("img_b_idx", lambda r: r.extra["img_b_idx"]))
    for k, get in ints:
        z[k] = np.asarray([int(get(r)) for r in out], np.int64)
    for k in ("scene_name_a", "scene_name_b", "object_id_a", "object_id_b", "keypoint_name"):
        z[k] = np.array([str(r.extra[k]) for r in out])
    for k in ("gap", "gap_masked"):
        z[k] = np.asarray([r.env[k] for r in out], np.float64)
    z["other_k_3d"] = np.asarray([r.other_k for r in out], np.float64)
    z["row_pair"] = np.arange(len(out), dtype=np.int64)     # (evaluate_common.check_table: one searched image per row)
    check(name, z)
    write_npz(os.path.join(HERE, "keypoints_ref_%s.npz" % name), z)
    return "rows %d, rows per searched image %s, invalid %d, masked != image %d, min gap %.1e" % (
        len(out), np.bincount(z["search_frame"])[np.unique(z["search_frame"])].tolist(), int((~z["is_valid"]).sum()),
        int(((z["pred_u"] != z["pred_u_masked"]) | (z["pred_v"] != z["pred_v_masked"])).sum()),
        min(z["gap"].min(), z["gap_masked"].min()))


def check(name, z):
    """What makes the comparison meaningful, from the reference's results alone"""
    h, w = int(z["h"]), int(z["w"])
    R = len(z["row_pair"])
    assert R == 36 and (np.bincount(z["search_frame"])[np.unique(z["search_frame"])] == 9).all(), (name, "not 4 x 9 rows")
    assert "extra" not in z["keypoint_name"].tolist()
    frac = np.concatenate([z["kp_u"], z["kp_v"]]) % 1.0
    assert (frac == 0.5).any(), (name, "no half-integer label")
    assert (z["kp_u"] > w - 0.5).any() and (z["kp_v"] > h - 0.5).any(), (name, "no label beyond the edge")
    assert (z["gt_u"] == w - 1).any() and (z["gt_v"] == h - 1).any()
    if h > 1 and w > 1:                                     # the query pixel takes its v from the OTHER image (:1523)
        assert (z["v_a"] == z["gt_v"]).all() and (z["u_a"] != z["gt_u"]).any()
    assert ((z["pred_u"] != z["pred_u_masked"]) | (z["pred_v"] != z["pred_v_masked"])).any(), (name, "masked == image everywhere")
    assert z["is_valid"].any() and (~z["is_valid"]).any(), (name, "one value of is_valid only")
    assert z["is_valid_masked"].any() and (~z["is_valid_masked"]).any(), (name, "one value of is_valid_masked only")
    assert np.isnan(z["norm_diff_pred_3d"][~z["is_valid"]]).all()
    assert z["gap"].min() > 1e-4 and z["gap_masked"].min() > 1e-4, (name, z["gap"].min(), z["gap_masked"].min())
    # a reverse row (odd rows) between scenes of different K whose 3D columns the other scene's K would change
    got = np.stack([z[k] for k in COLUMNS[3:6]], axis=1)
    moved = np.nan_to_num(np.abs(got - z["other_k_3d"])).max(axis=1) > 1e-4
    assert moved[1::2].any(), (name, "no reverse row tells the two K apart")
    same_scene = z["scene_name_a"] == z["scene_name_b"]
    assert same_scene.any() and not moved[same_scene].any()


def main():
    ref = me.load_reference()
    fn_code = load_function(open(me.EVAL).read().split("\n"))
    only = sys.argv[1:]
    # seeds: the first (from 1 up) for which the reference's results pass ``check``
    for name, h, w, D in (("48x64_d3", 48, 64, 3), ("37x53_d16", 37, 53, 16), ("1x64_d1", 1, 64, 1), ("48x1_d1", 48, 1, 1)):
        if only and name not in only:
            continue
        for seed in range(1, 400):
            try:
                print(name, "seed", seed, case(ref, fn_code, name, h, w, D, seed))
                break
            except AssertionError as e:
                print(name, "seed", seed, "rejected:", e)
        else:
            raise SystemExit("no seed passes for " + name)


if __name__ == "__main__":
    main()
