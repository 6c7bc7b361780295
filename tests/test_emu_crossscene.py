"""Cross-scene evaluation (csrc/crossscene_kernels.hip, dcn_hip/evaluate/cross_scene.py) through the host-emulation build: the reference's
own per-pair analysis replayed (crossscene goldens), the grouped statistics against the pair-wise entry bit for bit, the
reprojection against the match search, the device-side status bits, the label and view rules on the host and
evaluate_network_cross_scene on a small store."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import acrossobj_common as ac
import crossscene_common as cc
import evaluate_common as ec
from dcn_hip import evaluate
from helpers import PKG, use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert sorted(cc.GOLDEN_IDS) == ["1x64_d1", "37x53_d16", "48x1_d1", "48x64_d3"]


@pytest.mark.parametrize("path", cc.GOLDENS, ids=cc.GOLDEN_IDS)
def test_golden_through_the_chain(path):
    z = np.load(path)
    assert list(z["columns"]) == list(evaluate.COLUMNS)
    cc.check_golden(z, "cpu", batch_frames=4)
    # the fixtures hold what they are named for
    oc = z["request_outcome"]
    assert (oc == cc.NO_VIEW).any() and (oc == cc.NO_MATCH).any() and (oc == cc.FOUND).any()
    views = cc.golden_views(z)
    assert ((views[:, 4] == int(z["frame_b"])) & (views[:, 3] >= 0)).sum() == 33     # image b's group: one past the query tile


@pytest.mark.parametrize("sizes", [(1,), (32,), (33,), (70,), (3, 1, 33, 0, 2)], ids=lambda s: "x".join(map(str, s)))
def test_groups_equal_pairs_bit_for_bit(sizes):
    groups, pairs, group = cc.random_groups(sizes, 9, 13, 3, seed=sum(sizes))
    cc.check_groups_against_pairs(groups, pairs, group)
    cc.check_groups_against_pairs(groups, pairs, group, max_group_rows=max(sizes))


@pytest.mark.parametrize("d", [7, 64, 4])
def test_other_descriptor_dimensions(d):
    """A dimension without a kernel of its own (D = 7), the largest one (64), and a 16-byte-load dimension (D = 4)"""
    groups, pairs, group = cc.random_groups((5, 34), 7, 11, d, seed=d)
    cc.check_groups_against_pairs(groups, pairs, group)


def test_a_group_with_every_row_left_out_and_an_empty_mask():
    groups, pairs, group = cc.random_groups((4, 6, 3), 9, 13, 3, seed=2)
    groups["keep"][4:10] = 0                                # group 1: no row takes part
    groups["keep"][:4] = 1
    groups["mask_b"][0] = 0                                 # group 0 searches an image whose mask is empty
    pairs["mask_b"][:4] = 0
    tg, _ = cc.check_groups_against_pairs(groups, pairs, group)
    assert tg.row_pair.tolist()[:10] == [0] * 4 + [-1] * 6 and int(tg.mask_pixels[0]) == 0
    assert torch.isnan(tg.column("fraction_pixels_closer_than_ground_truth_masked")[:4]).all()
    assert not torch.isnan(tg.column("fraction_pixels_closer_than_ground_truth")[:4]).any()
    # what a row left out carries is never looked at
    groups["u_a"][5], groups["u_b"][6] = -7, float("nan")
    assert int(evaluate.match_statistics_groups(**groups).status[0]) == 0
    groups["keep"][5] = 1
    assert int(evaluate.match_statistics_groups(**groups).status[0]) == evaluate.BAD_INDEX


def test_bad_offsets_and_max_group_rows():
    groups, _, _ = cc.random_groups((4, 6, 3), 9, 13, 3, seed=3)
    assert int(evaluate.match_statistics_groups(**groups).status[0]) == 0
    cut = evaluate.match_statistics_groups(max_group_rows=5, **groups)
    assert int(cut.status[0]) == evaluate.BAD_OFFSETS
    kept = groups["keep"].bool()
    assert torch.equal(cut.row_pair[:9] >= 0, kept[:9]) and int(cut.row_pair[9]) == -1     # group 1 cut after 5 rows
    for bad in ([0, 4, 3, 13], [0, 4, 10, 14], [-1, 4, 10, 13]):
        t = evaluate.match_statistics_groups(**dict(groups, offsets=torch.tensor(bad)))
        assert int(t.status[0]) & evaluate.BAD_OFFSETS, bad
        assert (t.row_pair == -1).all() and torch.isnan(t.columns).all()
    with pytest.raises(ValueError):
        evaluate.match_statistics_groups(**dict(groups, offsets=torch.tensor([0, 4, 10])))
    with pytest.raises(ValueError):
        evaluate.match_statistics_groups(**dict(groups, keep=groups["keep"][:-1]))
    with pytest.raises(ValueError):
        evaluate.match_statistics_groups(**dict(groups, queries=groups["queries"].double()))
    with pytest.raises(ValueError):
        evaluate.match_statistics_groups(**dict(groups, depth_q=groups["depth_q"].float()))


def test_reprojection_equals_the_match_search():
    """The candidates find_eval_matches keeps, asked of reproject_pixels one by one: the same projections, bit for bit; a
    pixel the search drops is not found"""
    h, w = 24, 32
    store = ec.synthetic_store("cpu", h, w, seed=3, still_scene=False)
    fr = np.array([[0, 1], [1, 3], [2, 0], [5, 6]])
    _, depth, mask, cams, _ = evaluate._gather_host_frames(store, fr, ("depth", "mask", "cams"))
    m = evaluate.find_eval_matches(depth[0], depth[1], torch.ones_like(mask[0]), cams[0], 200, num_attempts=200,
                                   generator=torch.Generator().manual_seed(1))
    off = m.offsets.tolist()
    assert int(m.status[0]) == 0 and off[-1] > 50
    pair = np.repeat(np.arange(len(fr)), np.diff(off))
    R = off[-1]
    req = np.stack([fr[pair, 0], m.u_a[:R].numpy(), m.v_a[:R].numpy(), fr[pair, 1]], axis=1)
    rp = evaluate.reproject_pixels(store, req, K=store.K[0])
    assert int(rp.status[0]) == 0 and (rp.found == 1).all()
    assert torch.equal(cc.bits(rp.u), cc.bits(m.u_b[:R])) and torch.equal(cc.bits(rp.v), cc.bits(m.v_b[:R]))
    assert rp.uv[0].tolist() == [min(ec.py2_round(x), w - 1) for x in m.u_b[:R].tolist()]
    assert rp.uv[1].tolist() == [min(ec.py2_round(x), h - 1) for x in m.v_b[:R].tolist()]
    # every pixel of frame 0 into frame 1: found exactly where the search (all pixels as candidates) keeps it
    vs, us = np.mgrid[0:h, 0:w]
    every = evaluate.reproject_pixels(store, np.stack([np.zeros(h * w, int), us.ravel(), vs.ravel(), np.ones(h * w, int)], 1),
                                      K=store.K[0])
    kept = set((m.v_a[:off[1]] * w + m.u_a[:off[1]]).tolist())
    found = set(np.nonzero(every.found.numpy())[0].tolist())
    assert kept <= found and 0 < len(found) < h * w
    no_depth = np.nonzero(store.depth[0].numpy().ravel() == 0)[0]
    assert len(no_depth) and not (set(no_depth.tolist()) & found)
    assert (every.uv[:, every.found == 0] == -1).all()
    # the default K is the reference's, not the store's
    default = evaluate.reproject_pixels(store, req)
    assert not torch.equal(default.u, rp.u)
    assert evaluate.reproject_pixels(store, np.zeros((0, 4), np.int64)).found.numel() == 0


def test_out_of_range_requests_raise_the_status_bit():
    store = ec.synthetic_store("cpu", 12, 16, seed=1, still_scene=False)
    F = store.num_frames
    good = [0, 5, 5, 1]
    assert int(evaluate.reproject_pixels(store, [good]).status[0]) == 0
    for bad in ([F, 5, 5, 1], [0, 5, 5, F], [-1, 5, 5, 1], [0, 5, 5, -1], [0, 16, 5, 1], [0, 5, 12, 1], [0, -1, 5, 1],
                [0, 5, -1, 1]):
        rp = evaluate.reproject_pixels(store, [good, bad, good])
        assert int(rp.status[0]) == evaluate.BAD_FRAME, bad
        assert int(rp.found[1]) == 0 and rp.uv[:, 1].tolist() == [-1, -1]
        assert torch.equal(rp.found[[0, 2]], evaluate.reproject_pixels(store, [good, good]).found)
    with pytest.raises(ValueError):
        evaluate.reproject_pixels(store, [[0, 1, 2]])


def _annotation(scene_a, idx_a, scene_b, idx_b, pixels_a, pixels_b):
    px = lambda l: [{"u": u, "v": v} for u, v in l]
    return {"image_a": {"scene_name": scene_a, "image_idx": idx_a, "pixels": px(pixels_a)},
            "image_b": {"scene_name": scene_b, "image_idx": idx_b, "pixels": px(pixels_b)}}


def test_cross_scene_labels():
    store = ac.three_object_store("cpu", 8, 12)                                  # frame ids 10 s + j, scenes scene_a .. scene_e
    ann = [_annotation("scene_a", 1, "scene_b", 11, [(2.5, 3.49), (11.6, 7.5)], [(0, 0), (40, 3)]),
           _annotation("scene_x", 1, "scene_b", 11, [(1, 1)], [(1, 1)]),
           _annotation("scene_c", 23, "scene_e", 45, [(1, 1)], [(1, 1)]),
           _annotation("scene_c", 23, "scene_e", 41, [(4, 5)], [(6, 7)])]
    lab = evaluate.cross_scene_labels(store, ann)
    assert lab.pairs.tolist() == [[0, 0, 1, 1, 4], [3, 2, 8, 4, 12]]
    # Python 2's round (2.5 -> 3), then min(..., size - 1)
    assert lab.pixels.tolist() == [[0, 3, 3, 0, 0], [0, 11, 7, 11, 3], [1, 4, 5, 6, 7]]
    assert [i for i, _ in lab.skipped] == [1, 2] and "scene_x" in lab.skipped[0][1] and "45" in lab.skipped[1][1]
    with pytest.raises(ValueError, match="no annotated"):
        evaluate.cross_scene_labels(store, [])
    with pytest.raises(ValueError, match="2 pixels in image a but 1"):
        evaluate.cross_scene_labels(store, [_annotation("scene_a", 1, "scene_b", 11, [(1, 1), (2, 2)], [(1, 1)])])
    with pytest.raises(ValueError, match="negative"):
        evaluate.cross_scene_labels(store, [_annotation("scene_a", 1, "scene_b", 11, [(1, -0.6)], [(1, 1)])])
    assert evaluate.cross_scene_labels(store, [_annotation("scene_a", 1, "scene_b", 11, [(1, -0.4)], [(1, 1)])]) \
        .pixels.tolist() == [[0, 1, 0, 1, 1]]                                     # (rounds to zero: the reference's pixel)
    none = evaluate.cross_scene_labels(store, ann[1:3])
    assert none.pairs.shape == (0, 5) and none.pixels.shape == (0, 5) and len(none.skipped) == 2


def _two_scene_store(device, h=24, w=32, seed=0):
    """ec.synthetic_store's three scenes under names of their own, its cameras four times closer together (the reprojection
    runs with the reference's default K, under which 6 cm at 0.9 m is more than this image's width): 4 frames 1.5 cm apart, 3
    coinciding frames, 4 frames"""
    from dcn_hip import frames
    s = ec.synthetic_store(device, h, w, seed=seed)
    poses = s.poses_host.copy()
    poses[:, :3, 3] *= 0.25
    return frames.FrameStore.from_tensors(s.rgb, s.depth, s.mask, poses, s.scene_first_frame_host, s.scene_object_host, s.K,
                                          scene_names=["moving", "still", "other"],
                                          frame_ids=[[3, 5, 8, 13], [2, 4, 6], [1, 10, 100, 1000]])


def test_choose_cross_scene_views_follows_the_rule():
    store = _two_scene_store("cpu")
    ann = [_annotation("moving", 5, "other", 100, [(3, 4), (5, 6)], [(7, 8), (9, 10)]),
           _annotation("other", 1, "still", 4, [(1, 2)], [(3, 4)])]
    lab = evaluate.cross_scene_labels(store, ann)
    views = evaluate.choose_cross_scene_views(store, lab, host_rng=np.random.RandomState(4), threshold=0.0125)
    assert views.shape == (2 + 2 * 20 + 1 + 20, 5) and views.dtype == np.int64
    assert np.array_equal(views, evaluate.choose_cross_scene_views(store, lab, host_rng=np.random.RandomState(4), threshold=0.0125))
    assert not np.array_equal(views, evaluate.choose_cross_scene_views(store, lab, host_rng=np.random.RandomState(5),
                                                                       threshold=0.0125))
    # the reference's row order: the labelled rows of a pair, then per label 10 a-views and 10 b-views
    kinds = [0, 0] + ([1] * 10 + [2] * 10) * 2 + [0] + [1] * 10 + [2] * 10
    assert views[:, 2].tolist() == kinds and views[:, 0].tolist() == [0] * 42 + [1] * 21
    assert views[:, 1].tolist() == [0, 1] + [0] * 20 + [1] * 20 + [2] * 21
    first, t = store.scene_first_frame_host, store.translations_host
    fa, fb = lab.pairs[views[:, 0], 2], lab.pairs[views[:, 0], 4]
    k = views[:, 2]
    assert (views[k != 1, 3] == fa[k != 1]).all() and (views[k != 2, 4] == fb[k != 2]).all()
    for n, l, kind, a, b in views[k == 1]:                                       # an a-view: a frame of scene a, far enough
        sa = lab.pairs[n, 1]
        assert first[sa] <= a < first[sa + 1] and np.linalg.norm(t[a] - t[lab.pairs[n, 2]]) > 0.0125
    moved = views[(k == 2) & (views[:, 0] == 0)]
    assert len(moved) == 20 and all(first[2] <= b < first[3] and np.linalg.norm(t[b] - t[lab.pairs[0, 4]]) > 0.0125
                                    for b in moved[:, 4])
    assert len(set(moved[:, 4].tolist())) > 1
    # no frame of the still scene differs from its labelled image: no view
    assert (views[(k == 2) & (views[:, 0] == 1), 4] == -1).all()
    # at the reference's 0.2 m nothing in this store qualifies; the angle is compared in the reference's units and never fires
    strict = evaluate.choose_cross_scene_views(store, lab, host_rng=np.random.RandomState(4))
    assert (strict[k == 1, 3] == -1).all() and (strict[k == 2, 4] == -1).all() and np.array_equal(strict[:, :3], views[:, :3])
    poses = store.poses_host.copy()
    c, s = np.cos(2.0), np.sin(2.0)
    poses[first[2] + 1, :3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]            # two radians, but far below "20"
    store.poses_host = poses
    assert (evaluate.choose_cross_scene_views(store, lab, host_rng=np.random.RandomState(4))[:, 3:5].min(1)[k != 0] == -1).all()
    turned = evaluate.choose_cross_scene_views(store, lab, host_rng=np.random.RandomState(4), angle_threshold=1.5)
    assert set(turned[(k == 2) & (turned[:, 0] == 0), 4].tolist()) == {first[2] + 1}
    few = evaluate.choose_cross_scene_views(store, lab, 2, 0, np.random.default_rng(1), threshold=0.0125)   # a numpy Generator too
    assert few.shape == (2 + 2 * 2 + 1 + 2, 5)


def test_evaluate_network_cross_scene_on_a_small_store():
    h, w = 24, 32
    store = _two_scene_store("cpu", h, w)
    ann = [_annotation("moving", 5, "other", 100, [(12, 9), (20.5, 14)], [(15, 11), (9, 16)]),
           _annotation("nowhere", 1, "still", 4, [(1, 2)], [(3, 4)]),
           _annotation("other", 1, "still", 4, [(16, 12)], [(14, 10)])]
    lab = evaluate.cross_scene_labels(store, ann)
    rng = lambda: np.random.RandomState(7)
    views = evaluate.choose_cross_scene_views(store, lab, 4, 3, rng(), threshold=0.0125)
    dcn = ac.StubNetwork()
    dcn.train()
    t = evaluate.evaluate_cross_scene_rows(dcn, store, lab, views)
    assert dcn.training and int(t.status[0]) == 0
    assert t.columns.shape[1] == views.shape[0] == 2 + 2 * 7 + 1 + 7 and t.offsets.tolist() == [0, 16, 24]
    # a row exists where both frames do and the labelled pixel projects into the view
    has = (t.row_pair >= 0).numpy()
    assert has[views[:, 2] == 0].all() and not has[(views[:, 3:5] < 0).any(1)].any()
    assert 3 < has.sum() < len(has) and (t.row_pair[has] == torch.from_numpy(views[has, 0]).int()).all()
    # one forward pass per distinct frame, whatever the batches; the same table for every batch and chunk size
    assert sum(int(o.shape[0]) for o in dcn.outputs) == len(set(views[views[:, 3:5].min(1) >= 0, 3].tolist())) \
        + len(set(views[views[:, 3:5].min(1) >= 0, 4].tolist()))
    for kw in (dict(batch_frames=1), dict(batch_frames=3, max_search_bytes=1), dict(max_search_bytes=2 * h * w * 3 * 4)):
        cc.same_tables(t, evaluate.evaluate_cross_scene_rows(ac.StubNetwork(), store, lab, views, **kw))
    # each row is the pair-wise entry's row for its two images
    net = ac.StubNetwork()
    rows = np.nonzero(has)[0]
    fr = views[rows, 3:5]
    rgb, depth, mask, cams, _ = evaluate._gather_host_frames(store, fr, ("rgb", "depth", "mask", "cams"))
    res = []
    evaluate._forward_in_eval_mode(net, rgb[0], mask[0], rgb[1], mask[1], 64, evaluate._aug.DEFAULT_IMAGE_MEAN,
                                   evaluate._aug.DEFAULT_IMAGE_STD_DEV, lambda lo, n, y: res.append(y))
    n = len(rows)
    at = torch.from_numpy(rows)
    tp = evaluate.match_statistics_pairs(res[0][:n].contiguous(), res[0][n:].contiguous(), mask[1], depth[0], depth[1], cams[0],
                                         t.u_a[at], t.v_a[at], t.u_b[at], t.v_b[at], torch.arange(n + 1))
    assert int(tp.status[0]) == 0
    for k in ("columns", "is_valid", "pred_uv", "closer"):
        assert torch.equal(cc.bits(getattr(t, k)[:, at]), cc.bits(getattr(tp, k))), k
    assert torch.equal(t.mask_pixels[at], tp.mask_pixels)
    # the composed call: the same rows, named
    composed = ac.StubNetwork()
    composed.train()
    table, df = evaluate.evaluate_network_cross_scene(composed, store, ann, 4, 3, host_rng=rng())
    assert composed.training
    # (its views are drawn at the reference's 0.2 m, which nothing in this store passes: the labelled rows alone)
    assert len(table["norm_diff_descriptor"]) == 3 and list(df.columns) == list(evaluate.COLUMNS) + [
        "is_valid", "is_valid_masked", "scene_name", "img_a_idx", "img_b_idx"]
    assert table["scene_name"].tolist() == ["moving+other"] * 2 + ["other+still"]
    assert table["img_a_idx"].tolist() == [5, 5, 1] and table["img_b_idx"].tolist() == [100, 100, 4]
    named = evaluate.cross_scene_table(store, lab, views, t)
    assert len(named["is_valid"]) == has.sum() and named["scene_name"].tolist() == [
        "moving+other" if p == 0 else "other+still" for p in views[has, 0]]
    ids = {f: i for s in range(3) for f, i in zip(range(store.scene_first_frame_host[s], store.scene_first_frame_host[s + 1]),
                                                   store.frame_ids[s])}
    assert named["img_a_idx"].tolist() == [ids[f] for f in views[has, 3]]
    assert named["img_b_idx"].tolist() == [ids[f] for f in views[has, 4]]
    assert np.array_equal(named["norm_diff_descriptor"][:2], table["norm_diff_descriptor"][:2])
    # no usable annotated pair: an empty table, not an error
    table, df = evaluate.evaluate_network_cross_scene(ac.StubNetwork(), store, ann[1:2])
    assert all(len(v) == 0 for v in table.values()) and len(df) == 0
    with pytest.raises(ValueError):
        evaluate.evaluate_cross_scene_rows(ac.StubNetwork(), store, lab, views[:, :4])
    with pytest.raises(ValueError):
        evaluate.evaluate_cross_scene_rows(ac.StubNetwork(), store, lab, np.array([[0, 0, 0, 0, store.num_frames]]))


def test_the_device_library_refuses_cpu_tensors():
    """In a process of its own, which loads the shipped library (this one keeps the emulation)"""
    from dcn_hip import build
    code = r"""
import sys, torch
sys.path.insert(0, %r)
from dcn_hip import _lib, evaluate
_lib.load(%r)
class Store(object):
    device = torch.device("cpu")
z = lambda *s, **k: torch.zeros(*s, **k)
said = []
for call in (lambda: evaluate.reproject_pixels(Store(), [[0, 0, 0, 0]]),
             lambda: evaluate.match_statistics_groups(z(1, 4, 4, 3), z(1, 4, 4, dtype=torch.uint8), z(1, 4, 4, dtype=torch.int16),
                                                      z(2, 3), z(2, dtype=torch.int64), z(2, dtype=torch.int64),
                                                      z(2, dtype=torch.int16), z(2), z(2), z(2, 50), z(2, dtype=torch.uint8),
                                                      torch.tensor([0, 2]))):
    try:
        call()
    except ValueError as e:
        said.append("no CPU fallback" in str(e))
print("REFUSED" if said == [True, True] else said)
""" % (PKG, build.build_library())
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert b"REFUSED" in out.stdout, out.stderr.decode()[-2000:]
