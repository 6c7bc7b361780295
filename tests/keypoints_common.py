"""Shared by tests/test_emu_keypoints.py and tests/test_gpu_keypoints.py: the keypoints goldens (the reference's own
single_image_pair_cross_scene_keypoints_quantitative_analysis over itertools.combinations of four labelled images,
tests/golden/make_keypoints_goldens_from_reference.py) replayed through dcn_hip.evaluate, and the wide statistics entry
against the grouped one on crossscene_common's random rows."""
import collections
import glob
import os

import numpy as np
import torch

import crossscene_common as cc
import evaluate_common as ec

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "keypoints_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("keypoints_ref_"):-4] for p in GOLDENS]
# (group sizes, (h, w), D, strip_pixels, keep_fraction): rows up to, at and past one workgroup's 256 and past two; 20 x 28
# with strips of 256 pixels is three strips, the last one partial; one-row and one-column images; every specialised kind of D
# (3, 16), the generic path (1, 5) and its largest (64); rows all left out; the automatic strip
WIDE_CASES = [((0, 1, 255, 256, 257), (20, 28), 3, 256, 0.8), ((513, 0, 3), (20, 28), 16, 256, 0.8),
              ((513, 0, 3), (20, 28), 5, 256, 0.8), ((0, 1, 255, 256, 257), (1, 64), 1, 16, 0.8),
              ((513, 0, 3), (48, 1), 1, 0, 0.8), ((0, 1, 255, 256, 257), (20, 28), 64, 256, 0.8),
              ((513, 0, 3), (20, 28), 3, 256, 0.0), ((0, 1, 255, 256, 257), (20, 28), 16, 0, 0.8),
              ((513, 0, 3), (20, 28), 64, 0, 0.8)]
WIDE_IDS = ["%s-%dx%d-d%d-s%d-k%g" % ("x".join(map(str, c[0])), c[1][0], c[1][1], c[2], c[3], c[4]) for c in WIDE_CASES]


def golden_store(z, device):
    """(store, network) of a golden: its three scenes as a frame store (K per scene), its descriptor images behind a
    crossscene_common.StoredNetwork"""
    from dcn_hip import augment, frames
    h, w, F = int(z["h"]), int(z["w"]), int(z["poses"].shape[0])
    first = z["first"].tolist()
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    ids = z["frame_ids"].tolist()
    S = len(first) - 1
    store = frames.FrameStore.from_tensors(
        c(cc.frame_coded_rgb(F, h, w)), c(z["depth"].view(np.int16)), c(z["mask"]), z["poses"], first, list(range(S)), z["K"],
        scene_names=[str(s) for s in z["scene_names"]], frame_ids=[ids[first[s]:first[s + 1]] for s in range(S)])
    res = c(z["res_q"].astype(np.float32) * np.float32(z["res_scale"]))
    return store, cc.StoredNetwork(res, augment.DEFAULT_IMAGE_MEAN, augment.DEFAULT_IMAGE_STD_DEV)


def golden_annotations(z):
    """The annotation list as the reference's YAML would hold it"""
    out = []
    for i in range(len(z["ann_scene_name"])):
        kps = collections.OrderedDict()
        for j in np.nonzero(z["kp_image"] == i)[0]:
            kps[str(z["kp_name"][j])] = {"keypoint": str(z["kp_name"][j]), "u": float(z["kp_u"][j]), "v": float(z["kp_v"][j])}
        out.append({"scene_name": str(z["ann_scene_name"][i]), "image_idx": int(z["ann_image_idx"][i]),
                    "object_id": str(z["ann_object_id"][i]), "keypoints": kps})
    return out


def check_golden(z, device, **chain):
    """A golden through the chain: the rows in the reference's order with its query pixels and ground truths (exact), every
    column (evaluate_common.check_table and its tolerances), the names, and one forward pass per distinct frame"""
    from dcn_hip import evaluate
    store, net = golden_store(z, device)
    ann = golden_annotations(z)
    labels = evaluate.keypoint_labels(store, ann)
    assert labels.skipped == [] and labels.images[:, 0].tolist() == list(range(len(ann)))
    rows = evaluate.keypoint_rows(labels)
    R = len(z["row_pair"])
    assert rows.shape == (R, len(evaluate.KEYPOINT_ROW_COLUMNS))
    assert np.array_equal(rows[:, 3], z["query_frame"]) and np.array_equal(rows[:, 4], z["search_frame"])
    assert np.array_equal(rows[:, 5], z["u_a"]) and np.array_equal(rows[:, 6], z["v_a"])       # the (u_1, v_2) rule
    assert np.array_equal(rows[:, 7], z["gt_u"]) and np.array_equal(rows[:, 8], z["gt_v"])
    assert rows[:, 2].tolist() == [evaluate.STANDARD, evaluate.REVERSE] * (R // 2)
    net.train()
    t = evaluate.evaluate_keypoint_rows(net, store, labels, rows, **chain)
    assert net.training
    assert int(t.status.cpu()[0]) == 0
    assert np.array_equal(t.row_pair.cpu().numpy(), rows[:, 0]) and t.offsets.cpu().tolist() == list(range(0, R + 1, 6))
    assert np.array_equal(t.u_a.cpu().numpy(), z["u_a"]) and np.array_equal(t.v_a.cpu().numpy(), z["v_a"])
    assert np.array_equal(t.u_b.cpu().numpy(), z["gt_u"]) and np.array_equal(t.v_b.cpu().numpy(), z["gt_v"])
    # every column: check_table wants one searched image per "pair" -- here one per row
    zz = {k: z[k] for k in z.files}
    zz["mask_b"] = z["mask"][z["search_frame"]]
    ec.check_table(t._replace(row_pair=torch.arange(R, dtype=torch.int32)), zz)
    # the names
    table = evaluate.keypoint_table(store, labels, rows, t)
    for k in ("scene_name_a", "scene_name_b", "object_id_a", "object_id_b", "keypoint_name"):
        assert table[k].tolist() == [str(s) for s in z[k]], k
    assert np.array_equal(table["img_a_idx"], z["img_a_idx"]) and np.array_equal(table["img_b_idx"], z["img_b_idx"])
    assert np.array_equal(table["is_valid"], z["is_valid"]) and np.array_equal(table["is_valid_masked"], z["is_valid_masked"])
    assert np.array_equal(cc.bits(torch.from_numpy(table["pixel_match_error_l2"])), cc.bits(t.columns[6]))
    return store, net, labels, rows, t


def check_golden_every_way(z, device):
    """check_golden with the wide entry, with the grouped one and with a max_search_bytes that forces the two sweeps: one
    forward pass per distinct frame (two in the two-sweep path: the searched frames again), and the same bits three times"""
    frames = sorted(set(z["query_frame"].tolist()) | set(z["search_frame"].tolist()))
    _, net, _, _, wide = check_golden(z, device, batch_frames=3, search="wide")
    assert sum(net.seen, []) == frames
    _, net, _, _, groups = check_golden(z, device, batch_frames=3, search="groups")
    assert sum(net.seen, []) == frames
    one_image = int(z["h"]) * int(z["w"]) * int(z["D"]) * 4
    _, net, _, _, swept = check_golden(z, device, batch_frames=2, search="wide", max_search_bytes=2 * one_image)
    assert sum(net.seen, []) == frames + frames
    _, net, _, _, default = check_golden(z, device)
    assert sum(net.seen, []) == frames
    for other in (groups, swept, default):
        cc.same_tables(wide, other)
        assert torch.equal(wide.offsets.cpu(), other.offsets.cpu())
    return wide


def check_wide_against_groups(sizes, hw, d, strip, keep_fraction, device):
    """The wide entry and the grouped entry on the same random rows: every output bit for bit; also with a mask of all zeros
    and one of all ones"""
    from dcn_hip import evaluate
    groups, _, _ = cc.random_groups(sizes, hw[0], hw[1], d, seed=sum(sizes) + d, device=device, keep_fraction=keep_fraction)
    for mask in (None, 0, 1):
        if mask is not None:
            groups["mask_b"] = torch.full_like(groups["mask_b"], mask)
        a = evaluate.match_statistics_groups(**groups)
        b = evaluate.match_statistics_groups_wide(strip_pixels=strip, **groups)
        assert int(a.status.cpu()[0]) == 0
        cc.same_tables(a, b)
        assert torch.equal(b.row_pair.cpu() >= 0, groups["keep"].cpu() != 0)
    return groups


def check_planted_tie(device, h=20, w=28, strip=256):
    """Two pixels of the searched image in DIFFERENT strips, both equal to a row's query: the distance 0 ties exactly, the
    smaller flat index wins in the image and under the mask, and two runs give the same bits"""
    from dcn_hip import evaluate
    groups, _, _ = cc.random_groups((3, 300), h, w, 3, seed=11, device=device, keep_fraction=1.0)
    r, g = 270, 1                                           # a row of the second group's second row block
    lo, hi = 3 * w + 9, 15 * w + 5                          # flat indices 93 and 425: strips 0 and 1
    assert lo // strip != hi // strip
    for flat in (lo, hi):
        groups["res_b"][g].view(h * w, 3)[flat] = groups["queries"][r]
        groups["mask_b"][g].view(h * w)[flat] = 1
    a = evaluate.match_statistics_groups_wide(strip_pixels=strip, **groups)
    assert int(a.status.cpu()[0]) == 0
    assert a.pred_uv[:, r].tolist() == [lo % w, lo // w, lo % w, lo // w]
    assert float(a.column("norm_diff_descriptor")[r]) == 0.0 and float(a.column("norm_diff_descriptor_masked")[r]) == 0.0
    groups["mask_b"][g].view(h * w)[lo] = 0                  # off the mask, the first one is a million away
    b = evaluate.match_statistics_groups_wide(strip_pixels=strip, **groups)
    assert b.pred_uv[:, r].tolist() == [lo % w, lo // w, hi % w, hi // w]
    cc.same_tables(b, evaluate.match_statistics_groups_wide(strip_pixels=strip, **groups))
    cc.same_tables(b, evaluate.match_statistics_groups_wide(**groups))
    cc.same_tables(b, evaluate.match_statistics_groups(**groups))
