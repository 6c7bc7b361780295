"""Pins the batched evaluation (csrc/evaluate_kernels.hip, the matches-only entry of csrc/sample_kernels.hip,
dcn_hip/evaluate/pairs.py): executes the REFERENCE's own source lines -- read from /root/reference at run time, never copied --
  dense_correspondence/evaluation/evaluation.py:1045-1175   (the body of compute_descriptor_match_statistics)
  evaluation.py clip_pixel_to_image_size_and_round (:604-607), is_depth_valid (:961-972), compute_3d_position (:1181-1200)
  evaluation.py:37-64 DCNEvaluationPandaTemplate on evaluation/utils.py's PandaDataFrameWrapper (a recording stub when pandas
  is absent)
  dense_correspondence/network/dense_correspondence_network.py:486-525   (find_best_match)
  correspondence_finder.batch_find_pixel_correspondences / pinhole_projection_image_to_world (imported through
  tests/reference_py3.py with the patches of make_sample_goldens_from_reference.py)
on seeded synthetic image pairs, the way single_same_scene_image_pair_quantitative_analysis (:908-950) chains them: the match
search with img_a_mask = mask a and its default num_attempts and K, ``random.sample`` of the matches, then the statistics per
chosen match.  ``round`` is bound to Python 2's (half away from zero).  Stores inputs, the candidate draws, ``match_list``
and every output column in tests/golden/evalpairs_ref_*.npz.

Cameras: the statistics receive the float32-rounded K cast to float64, pose a likewise, and for pose b the float64 rigid
inverse of the fp32 pose b^-1 of the camera row: the device's camera rows (stored as ``cams``: K, K^-1, pose a, pose b^-1 in
fp32) carry pose b^-1, so this is the pose b they represent.  (The search inverts that pose b again in float64 and rounds to
fp32, which can differ from the row in the last bit of a translation entry: the fp32 rotation is orthonormal to 1e-8 only.)
Depth comes from smooth analytic surfaces with no-return holes
(make_sample_goldens_from_reference.frames), descriptors are given directly: res_b is res_a moved by the pairs' typical flow
plus noise (growing with sqrt(D), so that wrong best matches occur at every D), so the ground truth is usually a good match.

The generator ASSERTS that the fixtures make the comparison meaningful (see ``check``).

    python tests/golden/make_evalpairs_goldens_from_reference.py
"""
import math
import os
import random
import re
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_sample_goldens_from_reference as ms                                      # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

NET = "/root/reference/dense_correspondence/network/dense_correspondence_network.py"
EVAL = "/root/reference/dense_correspondence/evaluation/evaluation.py"
EUTILS = "/root/reference/dense_correspondence/evaluation/utils.py"
COLUMNS = ("norm_diff_descriptor_ground_truth", "norm_diff_descriptor", "norm_diff_descriptor_masked",
           "norm_diff_ground_truth_3d", "norm_diff_pred_3d", "norm_diff_pred_3d_masked", "pixel_match_error_l2",
           "pixel_match_error_l2_masked", "pixel_match_error_l1", "fraction_pixels_closer_than_ground_truth",
           "fraction_pixels_closer_than_ground_truth_masked", "average_l2_distance_for_false_positives",
           "average_l2_distance_for_false_positives_masked")


def py2_round(x):
    x = float(x)
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def method_source(lines, name):
    """The dedented text of ``def name`` (without decorators) of a class body"""
    start = next(i for i, l in enumerate(lines) if re.match(r"\s+def %s\(" % name, l))
    indent = len(lines[start]) - len(lines[start].lstrip())
    end = start + 1
    while end < len(lines) and (not lines[end].strip() or len(lines[end]) - len(lines[end].lstrip()) > indent):
        end += 1
    return textwrap.dedent("\n".join(lines[start:end]))


def class_source(lines, name):
    start = next(i for i, l in enumerate(lines) if l.startswith("class %s(" % name))
    end = start + 1
    while end < len(lines) and (not lines[end].strip() or lines[end][0] in " \t"):
        end += 1
    return "\n".join(lines[start:end])


def load_reference():
    _sdm, cf = ms.setup()
    from dense_correspondence_manipulation.utils.constants import DEPTH_IM_SCALE
    net = open(NET).read().split("\n")
    ev = open(EVAL).read().split("\n")
    fbm = textwrap.dedent("\n".join(net[486:525]))
    fbm = re.sub(r'print "([^"]*)", (\w[\w.]*)', r'print("\1", \2)', fbm)
    ns = {"np": np}
    exec(compile(fbm, NET, "exec"), ns)

    class DenseCorrespondenceNetwork(object):
        find_best_match = staticmethod(ns["find_best_match"])
    fns = {"np": np, "correspondence_finder": cf, "round": py2_round}
    for name in ("clip_pixel_to_image_size_and_round", "is_depth_valid", "compute_3d_position"):
        exec(compile(method_source(ev, name), EVAL, "exec"), fns)

    class DCE(object):
        clip_pixel_to_image_size_and_round = staticmethod(fns["clip_pixel_to_image_size_and_round"])
        is_depth_valid = staticmethod(fns["is_depth_valid"])
        compute_3d_position = staticmethod(fns["compute_3d_position"])
    try:
        import pandas as pd
        tns = {"np": np, "pd": pd}
        exec(compile(class_source(open(EUTILS).read().split("\n"), "PandaDataFrameWrapper").replace("%(key)", "% (key)"),
                     EUTILS, "exec"), tns)
        exec(compile(class_source(ev, "DCNEvaluationPandaTemplate"), EVAL, "exec"), tns)
        template = tns["DCNEvaluationPandaTemplate"]
        read = lambda t, k: np.asarray(t.dataframe[k])[0]
    except ImportError:
        class template(object):
            def __init__(self):
                self.values = {}

            def set_value(self, key, value):
                self.values[key] = value
        read = lambda t, k: t.values[k]
    block = compile(textwrap.dedent("\n".join(ev[1044:1175])), EVAL, "exec")
    env = {"np": np, "DenseCorrespondenceNetwork": DenseCorrespondenceNetwork, "DenseCorrespondenceEvaluation": DCE, "DCE": DCE,
           "DEPTH_IM_SCALE": DEPTH_IM_SCALE, "DCNEvaluationPandaTemplate": template, "debug": False, "rgb_a": None,
           "rgb_b": None}
    return cf, DCE, block, env, read


def invert_rigid(T):
    out = np.eye(4)
    R = T[:3, :3].T
    out[:3, :3] = R
    out[:3, 3] = -R.dot(T[:3, 3])
    return out


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def search(cf, fr, pose_a, pose_b, mask_a, seed, num_attempts=None):
    """The reference's match search as the evaluation calls it (:908), with its torch.rand draws recorded"""
    torch.manual_seed(seed)
    rec = ms.Recorder(cf)
    rec.across = False
    kw = {} if num_attempts is None else {"num_attempts": num_attempts}
    with rec:
        uv_a, uv_b = cf.batch_find_pixel_correspondences(fr["depth_a"], pose_a, fr["depth_b"], pose_b, device='CPU',
                                                         img_a_mask=mask_a, **kw)
    got = [v for s, v in rec.calls if s == "cand"]
    draws = (got[1] if len(got) == 2 else got[0]).astype(np.float32) if got else np.zeros(0, np.float32)
    if uv_a is None:
        return None, None, draws
    return ([t.numpy().astype(np.int64) for t in uv_a], [t.numpy().astype(np.float32) for t in uv_b], draws)


def make_pair(cf, h, w, seed, kind):
    fr = ms.frames(h, w, seed)
    if kind == "clip":                                  # a view that moves the matches towards the last row / column
        fr["pose_b"] = ms.pose(0.002, -0.003, [-0.006, -0.004, 0.0])
    pose_a = f32(fr["pose_a"]).astype(np.float64)
    tbinv32 = f32(invert_rigid(fr["pose_b"]))           # the camera row's pose b^-1 ...
    pose_b = invert_rigid(tbinv32.astype(np.float64))   # ... and the pose b it represents
    if kind == "no_match":
        fr["depth_b"] = np.zeros_like(fr["depth_b"])
    if kind == "clip":
        # mask a := the pixels whose projection rounds past the last column / row (found by a dense probe of the same search)
        ua, ub, _ = search(cf, fr, pose_a, pose_b, np.ones((h, w), np.uint8), seed, num_attempts=20000)
        sel = (ub[0] > w - 0.5) | (ub[1] > h - 0.5)
        assert sel.any(), "no projection rounds up at the clip"
        m = np.zeros((h, w), np.uint8)
        m[ua[1][sel], ua[0][sel]] = 1
        fr["mask_a"] = m
    return fr, pose_a, pose_b, tbinv32


def case(ref, name, h, w, D, kinds, num_matches, seed):
    cf, DCE, block, env0, read = ref
    rng = np.random.RandomState(seed)
    K = f32(cf.get_default_K_matrix()).astype(np.float64)
    P = len(kinds)
    out = {k: [] for k in COLUMNS + ("is_valid", "is_valid_masked", "row_pair", "u_a", "v_a", "u_b", "v_b", "gt_u", "gt_v",
                                     "pred_u", "pred_v", "pred_u_masked", "pred_v_masked", "closer", "closer_masked", "gap",
                                     "gap_masked")}
    pairs = {k: [] for k in ("depth_a", "depth_b", "mask_a", "mask_b", "pose_a", "pose_b", "res_a", "res_b", "rand_cand",
                             "totals", "match_order", "cams", "all_u_a", "all_v_a", "all_u_b", "all_v_b")}
    for p, kind in enumerate(kinds):
        fr, pose_a, pose_b, tbinv32 = make_pair(cf, h, w, seed + 10 * p, kind)
        pairs["cams"].append(np.concatenate([f32(K).reshape(-1), f32(np.linalg.inv(cf.get_default_K_matrix())).reshape(-1),
                                             f32(pose_a).reshape(-1), tbinv32.reshape(-1)]))
        uv_a, uv_b, draws = search(cf, fr, pose_a, pose_b, fr["mask_a"], seed + p)
        res_a = rng.randn(h, w, D).astype(np.float32)
        res_b = (np.roll(res_a, (1, 2), axis=(0, 1)) + 0.35 * np.sqrt(D / 3.0) * rng.randn(h, w, D)).astype(np.float32)
        total = 0 if uv_a is None else len(uv_a[0])
        random.seed(seed + p)
        match_list = random.sample(range(0, total), min(num_matches, total)) if total else []
        for key, val in (("depth_a", fr["depth_a"]), ("depth_b", fr["depth_b"]), ("mask_a", fr["mask_a"]),
                         ("mask_b", fr["mask_b"]), ("pose_a", pose_a), ("pose_b", pose_b), ("res_a", res_a), ("res_b", res_b),
                         ("rand_cand", draws), ("totals", total),
                         ("match_order", np.array(match_list + [-1] * (num_matches - len(match_list)), np.int32))):
            pairs[key].append(val)
        for j, key in enumerate(("all_u_a", "all_v_a")):
            pairs[key].append(np.zeros(0, np.int64) if uv_a is None else uv_a[j])
        for j, key in enumerate(("all_u_b", "all_v_b")):
            pairs[key].append(np.zeros(0, np.float32) if uv_b is None else uv_b[j])
        for i in match_list:
            a = (int(uv_a[0][i]), int(uv_a[1][i]))
            raw = (uv_b[0][i], uv_b[1][i])
            b = DCE.clip_pixel_to_image_size_and_round(raw, w, h)
            env = dict(env0, depth_a=fr["depth_a"], depth_b=fr["depth_b"], mask_a=fr["mask_a"], mask_b=fr["mask_b"], uv_a=a,
                       uv_b=b, pose_a=pose_a, pose_b=pose_b, res_a=res_a, res_b=res_b, camera_matrix=K)
            exec(block, env)
            t = env["pd_template"]
            for k in COLUMNS:
                out[k].append(float(read(t, k)))
            out["is_valid"].append(bool(read(t, "is_valid")))
            out["is_valid_masked"].append(bool(read(t, "is_valid_masked")))
            for k, v in (("row_pair", p), ("u_a", a[0]), ("v_a", a[1]), ("u_b", raw[0]), ("v_b", raw[1]), ("gt_u", b[0]),
                         ("gt_v", b[1]), ("pred_u", env["uv_b_pred"][0]), ("pred_v", env["uv_b_pred"][1]),
                         ("pred_u_masked", env["uv_b_pred_masked"][0]), ("pred_v_masked", env["uv_b_pred_masked"][1]),
                         ("closer", env["num_pixels_closer_than_ground_truth"]),
                         ("closer_masked", env["num_pixels_closer_than_ground_truth_masked"])):
                out[k].append(v)
            for k, nd in (("gap", env["norm_diffs"]), ("gap_masked", env["masked_norm_diffs"])):
                two = np.sort(np.asarray(nd, np.float64).reshape(-1))[:2]
                out[k].append((two[1] - two[0]) / two[1])
    z = dict(h=np.array(h), w=np.array(w), D=np.array(D), num_matches=np.array(num_matches), num_attempts=np.array(20), K=K,
             depth_a=np.stack(pairs["depth_a"]), depth_b=np.stack(pairs["depth_b"]), mask_a=np.stack(pairs["mask_a"]),
             mask_b=np.stack(pairs["mask_b"]), pose_a=np.stack(pairs["pose_a"]), pose_b=np.stack(pairs["pose_b"]), cams=np.stack(pairs["cams"]).astype(np.float32),
             res_a=np.stack(pairs["res_a"]), res_b=np.stack(pairs["res_b"]), totals=np.array(pairs["totals"], np.int32),
             match_order=np.stack(pairs["match_order"]), rand_cand=np.concatenate(pairs["rand_cand"]),
             rand_cand_offsets=np.cumsum([0] + [len(x) for x in pairs["rand_cand"]]).astype(np.int64),
             match_offsets=np.cumsum([0] + pairs["totals"]).astype(np.int64))
    for k in ("all_u_a", "all_v_a", "all_u_b", "all_v_b"):
        z[k] = np.concatenate(pairs[k])
    ints = ("row_pair", "u_a", "v_a", "gt_u", "gt_v", "pred_u", "pred_v", "pred_u_masked", "pred_v_masked", "closer",
            "closer_masked")
    for k, v in out.items():
        z[k] = np.asarray(v, np.int64 if k in ints else bool if k.startswith("is_valid") else
                          np.float32 if k in ("u_b", "v_b") else np.float64)
    z["offsets"] = np.searchsorted(z["row_pair"], np.arange(P + 1)).astype(np.int64)
    check(name, z)
    write_npz(os.path.join(HERE, "evalpairs_ref_%s.npz" % name), z)
    print(name, "pairs", P, "totals", z["totals"].tolist(), "rows", len(z["row_pair"]), "invalid pred", int((~z["is_valid"]).sum()),
          "masked != image", int(((z["pred_u"] != z["pred_u_masked"]) | (z["pred_v"] != z["pred_v_masked"])).sum()),
          "clipped", int(((z["u_b"] > z["w"] - 0.5) | (z["v_b"] > z["h"] - 0.5)).sum()),
          "min gap %.2e" % min(z["gap"].min(), z["gap_masked"].min()))


def check(name, z):
    """What makes the comparison meaningful, from the reference's results alone"""
    assert len(z["row_pair"]) > 0, name
    # best and second-best distance differ by more than 1e-4 relative: the argmin cannot flip with the summation order
    assert z["gap"].min() > 1e-4 and z["gap_masked"].min() > 1e-4, (name, z["gap"].min(), z["gap_masked"].min())
    assert (~z["is_valid"]).any(), (name, "no row with an invalid predicted depth")
    assert np.isnan(z["norm_diff_pred_3d"][~z["is_valid"]]).all()
    ok = ~np.isnan(z["norm_diff_ground_truth_3d"]) & ~np.isnan(z["norm_diff_pred_3d"]) & ~np.isnan(z["norm_diff_pred_3d_masked"])
    assert ok.any(), (name, "no row with all three 3D columns valid")
    assert ((z["pred_u"] != z["pred_u_masked"]) | (z["pred_v"] != z["pred_v_masked"])).any(), (name, "masked == image everywhere")
    assert (z["totals"] == 0).any(), (name, "no pair without matches")
    up = (np.array([py2_round(x) for x in z["u_b"]]) > z["w"] - 1) | (np.array([py2_round(x) for x in z["v_b"]]) > z["h"] - 1)
    assert up.any(), (name, "no ground-truth coordinate rounds up at the clip")
    assert (z["gt_u"][up] == z["w"] - 1).any() or (z["gt_v"][up] == z["h"] - 1).any()


def main():
    ref = load_reference()
    # seeds: the first (from 1 up) for which the reference's results pass ``check``
    for name, h, w, D, kinds, num_matches in (("48x64_d3", 48, 64, 3, ("normal", "clip", "no_match", "normal"), 100),
                                              ("37x53_d16", 37, 53, 16, ("normal", "no_match", "clip"), 12)):
        for seed in range(1, 60):
            try:
                case(ref, name, h, w, D, kinds, num_matches, seed)
                print(name, "seed", seed)
                break
            except AssertionError as e:
                print(name, "seed", seed, "rejected:", e)
        else:
            raise SystemExit("no seed passes for " + name)


if __name__ == "__main__":
    main()
