"""Class-consistent keypoint evaluation (dcn_hip/evaluate/keypoints.py, the wide statistics kernel of csrc/crossscene_kernels.hip) through
the host-emulation build: the reference's own per-pair analysis replayed (keypoints goldens), the wide entry against the
grouped one bit for bit, a planted tie across strips, the host rules, the device-side status bits,
evaluate_network_cross_instance and the csv file."""
import collections
import csv
import itertools

import numpy as np
import pytest
import torch

import acrossobj_common as ac
import crossscene_common as cc
import evaluate_common as ec
import keypoints_common as kc
from dcn_hip import evaluate
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert sorted(kc.GOLDEN_IDS) == ["1x64_d1", "37x53_d16", "48x1_d1", "48x64_d3"]


@pytest.mark.parametrize("path", kc.GOLDENS, ids=kc.GOLDEN_IDS)
def test_golden_through_the_chain(path):
    z = np.load(path)
    assert list(z["columns"]) == list(evaluate.COLUMNS)
    kc.check_golden_every_way(z, "cpu")
    # the fixtures hold what they are named for
    assert len(z["row_pair"]) == 36 and np.bincount(z["search_frame"]).max() == 9
    assert z["is_valid"].any() and (~z["is_valid"]).any()
    assert ((z["pred_u"] != z["pred_u_masked"]) | (z["pred_v"] != z["pred_v_masked"])).any()
    assert ((np.concatenate([z["kp_u"], z["kp_v"]]) % 1.0) == 0.5).any() and (z["kp_u"] > int(z["w"])).any()
    assert not np.array_equal(z["K"][0], z["K"][1])


@pytest.mark.parametrize("case", kc.WIDE_CASES, ids=kc.WIDE_IDS)
def test_wide_equals_groups_bit_for_bit(case):
    kc.check_wide_against_groups(*case, device="cpu")


def test_two_runs_are_bit_identical_with_a_planted_tie_across_strips():
    kc.check_planted_tie("cpu")


def test_wide_entry_status_bits_and_arguments():
    """Decreasing offsets, a cut group and an out-of-image u_a give the grouped entry's status bits and tables (emulation only:
    no bad input is sent to a GPU)"""
    groups, _, _ = cc.random_groups((4, 6, 3), 9, 13, 3, seed=3)
    both = lambda **kw: (evaluate.match_statistics_groups(**kw), evaluate.match_statistics_groups_wide(strip_pixels=32, **kw))
    for bad in ([0, 4, 3, 13], [0, 4, 10, 14], [-1, 4, 10, 13]):
        a, b = both(**dict(groups, offsets=torch.tensor(bad)))
        assert int(b.status[0]) & evaluate.BAD_OFFSETS, bad
        cc.same_tables(a, b)
        assert (b.row_pair == -1).all() and torch.isnan(b.columns).all()
    a, b = both(max_group_rows=5, **groups)
    assert int(b.status[0]) == evaluate.BAD_OFFSETS
    cc.same_tables(a, b)
    groups["keep"][:] = 1
    groups["u_a"][5] = 13                                    # one past the last column
    a, b = both(**groups)
    assert int(b.status[0]) == evaluate.BAD_INDEX
    cc.same_tables(a, b)
    groups["keep"][5] = 0                                    # what a row left out carries is never looked at
    groups["u_b"][5] = float("nan")
    a, b = both(**groups)
    assert int(b.status[0]) == 0 and int(b.row_pair[5]) == -1
    cc.same_tables(a, b)
    with pytest.raises(ValueError):
        evaluate.match_statistics_groups_wide(strip_pixels=-1, **groups)
    with pytest.raises(ValueError):
        evaluate.match_statistics_groups_wide(**dict(groups, keep=groups["keep"][:-1]))


def _annotation(scene, idx, object_id, keypoints):
    kps = collections.OrderedDict((n, {"keypoint": n, "u": u, "v": v}) for n, (u, v) in keypoints)
    return {"scene_name": scene, "image_idx": idx, "object_id": object_id, "keypoints": kps}


def _annotations():
    return [_annotation("scene_a", 1, "mug_1", [("rim", (2.5, 3.49)), ("handle", (11.6, 7.5))]),
            _annotation("scene_x", 1, "mug_2", [("rim", (1, 1)), ("handle", (1, 1))]),
            _annotation("scene_c", 23, "mug_3", [("handle", (4, 5)), ("rim", (6, 2))]),
            _annotation("scene_e", 45, "mug_4", [("rim", (1, 1)), ("handle", (1, 1))]),
            _annotation("scene_e", 41, "mug_5", [("rim", (0, 6.5)), ("handle", (3, 3)), ("base", (1, 1))])]


def test_keypoint_labels_and_rows():
    store = ac.three_object_store("cpu", 8, 12)              # frame ids 10 s + j, scenes scene_a .. scene_e
    lab = evaluate.keypoint_labels(store, _annotations())
    assert lab.images.tolist() == [[0, 0, 1], [2, 2, 8], [4, 4, 12]] and lab.size == (8, 12)
    assert [i for i, _ in lab.skipped] == [1, 3] and "scene_x" in lab.skipped[0][1] and "45" in lab.skipped[1][1]
    assert lab.names == [["rim", "handle"], ["handle", "rim"], ["rim", "handle", "base"]]
    assert lab.uv[0].tolist() == [[2.5, 3.49], [11.6, 7.5]] and lab.object_ids == ["mug_1", "mug_3", "mug_5"]
    rows = evaluate.keypoint_rows(lab)
    # combinations (0, 1), (0, 2), (1, 2); the keypoints of the FIRST image in its order; standard, then reverse; an extra name
    # of the second image ("base" in combinations (0, 2) and (1, 2)) is ignored
    assert rows[:, 0].tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert rows[:, 1].tolist() == [0, 0, 1, 1] * 2 + [0, 0, 1, 1] and rows[:, 2].tolist() == [0, 1] * 6
    assert rows[:, 3].tolist() == [1, 8, 1, 8, 1, 12, 1, 12, 8, 12, 8, 12]
    assert rows[:, 4].tolist() == [8, 1, 8, 1, 12, 1, 12, 1, 12, 8, 12, 8]
    # K of both orders: the combination's first image
    assert rows[:, 9].tolist() == [1] * 8 + [8] * 4
    # combination (0, 1), "rim": (2.5, 3.49) and (6, 2).  Standard: query (u_1, v_2) = (3, 2) -- Python 2's round -- ground truth
    # (6, 2); reverse: query (6, 3), ground truth (3, 3)
    assert rows[0, 5:9].tolist() == [3, 2, 6, 2] and rows[1, 5:9].tolist() == [6, 3, 3, 3]
    # "handle": (11.6, 7.5) clips to (11, 7); and (4, 5)
    assert rows[2, 5:9].tolist() == [11, 5, 4, 5] and rows[3, 5:9].tolist() == [4, 7, 11, 7]
    own = evaluate.keypoint_rows(lab, reference_query_pixel=False)
    assert np.array_equal(own[:, [0, 1, 2, 3, 4, 7, 8, 9]], rows[:, [0, 1, 2, 3, 4, 7, 8, 9]])
    assert own[0, 5:7].tolist() == [3, 3] and own[1, 5:7].tolist() == [6, 2] and own[2, 5:7].tolist() == [11, 7]
    # the first image's name missing from the second: the reference's error; the combination order decides
    ann = _annotations()
    del ann[4]["keypoints"]["handle"]
    with pytest.raises(ValueError, match="keypoint handle appears in one list of annotated data but not the other"):
        evaluate.keypoint_rows(evaluate.keypoint_labels(store, ann))
    ann = _annotations()
    ann[0]["keypoints"]["rim"]["v"] = -0.6
    with pytest.raises(ValueError, match="negative"):
        evaluate.keypoint_rows(evaluate.keypoint_labels(store, ann))
    ann[0]["keypoints"]["rim"]["v"] = -0.4                    # (rounds to zero: the reference's pixel)
    assert evaluate.keypoint_rows(evaluate.keypoint_labels(store, ann))[1, 6] == 0
    with pytest.raises(ValueError, match="no keypoint"):
        evaluate.keypoint_labels(store, [])
    one = evaluate.keypoint_labels(store, _annotations()[:2])
    assert one.images.shape == (1, 3) and evaluate.keypoint_rows(one).shape == (0, 10)


def test_reverse_rows_take_k_from_the_first_image():
    """On a golden whose scenes differ in K: the camera rows' K slots are those of the combination's first image for both
    orders, and a K chosen per order would change the 3D columns of a reverse row"""
    z = np.load([p for p, i in zip(kc.GOLDENS, kc.GOLDEN_IDS) if i == "48x64_d3"][0])
    store, net = kc.golden_store(z, "cpu")
    labels = evaluate.keypoint_labels(store, kc.golden_annotations(z))
    rows = evaluate.keypoint_rows(labels)
    t = evaluate.evaluate_keypoint_rows(net, store, labels, rows)
    per_order = rows.copy()
    per_order[:, 9] = per_order[:, 3]                        # K of the row's own image 1
    u = evaluate.evaluate_keypoint_rows(net, store, labels, per_order)
    scene = np.searchsorted(z["first"], rows[:, [3, 9]], side="right") - 1
    differs = ~(z["K"][scene[:, 0]] == z["K"][scene[:, 1]]).all(axis=(1, 2))
    assert differs.any() and not differs[rows[:, 2] == evaluate.STANDARD].any()
    a, b = t.columns[3:6].numpy(), u.columns[3:6].numpy()
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    assert same[:, ~differs].all() and not same[:, differs].all()
    assert np.array_equal(cc.bits(t.columns[[0, 1, 2, 6, 7, 8]]), cc.bits(u.columns[[0, 1, 2, 6, 7, 8]]))
    np.testing.assert_allclose(np.nan_to_num(b.T[differs]), np.nan_to_num(z["other_k_3d"][differs]), rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        evaluate.evaluate_keypoint_rows(net, store, labels, rows[:, :9])
    with pytest.raises(ValueError):
        evaluate.evaluate_keypoint_rows(net, store, labels, rows, search="narrow")
    far = rows.copy()
    far[0, 4] = store.num_frames
    with pytest.raises(ValueError):
        evaluate.evaluate_keypoint_rows(net, store, labels, far)


def test_evaluate_network_cross_scene_keypoints_and_its_csv(tmp_path):
    store = ac.three_object_store("cpu", 8, 12)
    ann = _annotations()
    dcn = ac.StubNetwork()
    dcn.train()
    table, df = evaluate.evaluate_network_cross_scene_keypoints(dcn, store, ann, save_to=str(tmp_path / "analysis" / "kp"))
    assert dcn.training
    assert sum(int(o.shape[0]) for o in dcn.outputs) == 3     # one forward pass per labelled frame the store holds
    names = list(evaluate.COLUMNS) + ["is_valid", "is_valid_masked", "img_a_idx", "img_b_idx", "scene_name_a", "scene_name_b",
                                      "object_id_a", "object_id_b", "keypoint_name"]
    assert sorted(table) == sorted(names) and len(table["is_valid"]) == 12
    assert table["keypoint_name"].tolist() == ["rim", "rim", "handle", "handle"] * 2 + ["handle", "handle", "rim", "rim"]
    assert table["img_a_idx"].tolist() == [1, 23, 1, 23, 1, 41, 1, 41, 23, 41, 23, 41]
    assert table["img_b_idx"].tolist() == [23, 1, 23, 1, 41, 1, 41, 1, 41, 23, 41, 23]
    assert table["scene_name_a"].tolist()[:2] == ["scene_a", "scene_c"] and table["object_id_b"].tolist()[:2] == ["mug_3", "mug_1"]
    # the file of run_cross_instance_keypoint_evaluation_on_network: the reference's column set (its template's columns and the
    # seven it sets per row) behind pandas' index column
    with open(str(tmp_path / "analysis" / "kp" / "data.csv")) as f:
        lines = list(csv.reader(f))
    assert lines[0][0] == "" and sorted(lines[0][1:]) == sorted(names) and len(lines) == 13
    at = lines[0].index("keypoint_name")
    assert [l[at] for l in lines[1:]] == table["keypoint_name"].tolist()
    np.testing.assert_allclose([float(l[lines[0].index("norm_diff_descriptor")]) for l in lines[1:]], table["norm_diff_descriptor"])
    if df is not None:
        assert sorted(df.columns) == sorted(names) and len(df) == 12
    # the same rows as the pieces give
    labels = evaluate.keypoint_labels(store, ann)
    rows = evaluate.keypoint_rows(labels)
    t = evaluate.evaluate_keypoint_rows(ac.StubNetwork(), store, labels, rows, search="wide")
    assert np.array_equal(cc.bits(torch.from_numpy(table["norm_diff_descriptor"])), cc.bits(t.column("norm_diff_descriptor")))
    # fewer than two usable images: an empty table, not an error
    table, df = evaluate.evaluate_network_cross_scene_keypoints(ac.StubNetwork(), store, ann[:2])
    assert sorted(table) == sorted(names) and all(len(v) == 0 for v in table.values())


def test_evaluate_network_cross_instance_expands_the_combinations():
    from dcn_hip import frames
    s = ec.synthetic_store("cpu", 24, 32)
    store = frames.FrameStore.from_tensors(s.rgb, s.depth, s.mask, s.poses_host, s.scene_first_frame_host, s.scene_object_host,
                                           s.K, scene_names=["moving", "still", "other"],
                                           frame_ids=[[3, 5, 8, 13], [2, 4, 6], [1, 10, 100, 1000]])
    px = lambda l: [{"u": u, "v": v} for u, v in l]
    images = [{"image": {"scene_name": "moving", "image_idx": 5, "pixels": px([(12, 9), (20.5, 14)])}},
              {"image": {"scene_name": "other", "image_idx": 100, "pixels": px([(15, 11), (9, 16)])}},
              {"image": {"scene_name": "still", "image_idx": 4, "pixels": px([(16, 12), (14, 10)])}}]
    pairs = [{"image_a": a["image"], "image_b": b["image"]} for a, b in itertools.combinations(images, 2)]
    assert [(p["image_a"]["scene_name"], p["image_b"]["scene_name"]) for p in pairs] == [
        ("moving", "other"), ("moving", "still"), ("other", "still")]
    rng = lambda: np.random.RandomState(7)
    got, _ = evaluate.evaluate_network_cross_instance(ac.StubNetwork(), store, images, 4, 3, host_rng=rng())
    want, _ = evaluate.evaluate_network_cross_scene(ac.StubNetwork(), store, pairs, 4, 3, host_rng=rng())
    assert sorted(got) == sorted(want) and len(got["is_valid"]) >= 6
    for k in want:
        if want[k].dtype == np.float64:
            assert np.array_equal(cc.bits(torch.from_numpy(got[k])), cc.bits(torch.from_numpy(want[k]))), k
        else:
            assert got[k].tolist() == want[k].tolist(), k
