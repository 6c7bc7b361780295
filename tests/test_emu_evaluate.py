"""Evaluation on frame-store image pairs (csrc/evaluate_kernels.hip, dcn_eval_matches of csrc/sample_kernels.hip,
dcn_hip/evaluate/pairs.py) through the host-emulation build: the reference's own match search, subsample and
compute_descriptor_match_statistics replayed (evalpairs goldens), the batched kernel against the per-pair one, the pair choice,
evaluate_network on a small store with a tiny network, and the host-side ValueErrors."""
import collections

import numpy as np
import pytest
import torch

import evaluate_common as ec
import frames_common as fc
from dcn_hip import evaluate
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert sorted(ec.GOLDEN_IDS) == ["37x53_d16", "48x64_d3"]


@pytest.mark.parametrize("path", ec.GOLDENS, ids=ec.GOLDEN_IDS)
def test_golden_matches_and_table(path):
    z = np.load(path)
    d = ec.golden_inputs(z, "cpu")
    m = ec.golden_matches(z, d)
    ec.check_matches(m, z)
    t = evaluate.match_statistics_pairs(d["res_a"], d["res_b"], d["mask_b"], d["depth_a"], d["depth_b"], d["cams"], m.u_a, m.v_a,
                                        m.u_b, m.v_b, m.offsets, max_pair_rows=int(z["num_attempts"]))
    R = len(z["row_pair"])
    full = evaluate.EvalTable(t.columns[:, :R], t.is_valid[:, :R], t.pred_uv[:, :R], t.closer[:, :R], t.row_pair[:R],
                              *t[5:])
    ec.check_table(full, z)
    # the rows past the last one: NaN columns, -1 pairs and pixels
    assert torch.isnan(t.columns[:, R:]).all() and (t.row_pair[R:] == -1).all() and (t.pred_uv[:, R:] == -1).all()


@pytest.mark.parametrize("path", ec.GOLDENS, ids=ec.GOLDEN_IDS)
def test_golden_table_from_the_reference_rows(path):
    """The statistics alone, on the reference's own rows (no capacity tail)"""
    z = np.load(path)
    d = ec.golden_inputs(z, "cpu")
    t = evaluate.match_statistics_pairs(d["res_a"], d["res_b"], d["mask_b"], d["depth_a"], d["depth_b"], d["cams"],
                                        torch.from_numpy(z["u_a"]), torch.from_numpy(z["v_a"]), torch.from_numpy(z["u_b"]),
                                        torch.from_numpy(z["v_b"]), torch.from_numpy(z["offsets"]))
    ec.check_table(t, z)


def test_seeded_subsample_is_a_sample_without_replacement():
    z = np.load(ec.GOLDENS[ec.GOLDEN_IDS.index("48x64_d3")])
    d = ec.golden_inputs(z, "cpu")
    P = int(z["mask_a"].shape[0])
    ro = z["rand_cand_offsets"]
    draws = {"cand": [z["rand_cand"][ro[p]:ro[p + 1]] for p in range(P)]}
    full = evaluate.find_eval_matches(d["depth_a"], d["depth_b"], d["mask_a"], d["cams"], 100, draws=draws,
                                      order_seeds=torch.arange(P))
    full_off = full.offsets.numpy()
    assert np.array_equal(np.diff(full_off), z["totals"])
    for k in (100, 5):
        a = evaluate.find_eval_matches(d["depth_a"], d["depth_b"], d["mask_a"], d["cams"], k, draws=draws,
                                       order_seeds=torch.arange(P) + 7)
        b = evaluate.find_eval_matches(d["depth_a"], d["depth_b"], d["mask_a"], d["cams"], k, draws=draws,
                                       order_seeds=torch.arange(P) + 7)
        c = evaluate.find_eval_matches(d["depth_a"], d["depth_b"], d["mask_a"], d["cams"], k, draws=draws,
                                       order_seeds=torch.arange(P) + 8)
        assert torch.equal(a.u_a, b.u_a) and torch.equal(a.u_b, b.u_b)
        off = a.offsets.numpy()
        assert np.array_equal(np.diff(off), np.minimum(z["totals"], k))
        differs = False
        for p in range(P):
            # without replacement: the chosen rows are a sub-MULTISET of the pair's survivors (a pixel drawn twice as a
            # candidate is two survivors; no survivor may be chosen more often than it occurs).  The survivors are the
            # device's own (k = all of them), which check_matches pins to the reference's.
            key = lambda m_, lo, hi: collections.Counter(zip(m_.u_a[lo:hi].tolist(), m_.v_a[lo:hi].tolist(),
                                                             m_.u_b[lo:hi].tolist(), m_.v_b[lo:hi].tolist()))
            everyone = key(full, int(full_off[p]), int(full_off[p + 1]))
            rows = key(a, int(off[p]), int(off[p + 1]))
            assert sum(everyone.values()) == int(z["totals"][p])
            assert sum(rows.values()) == min(int(z["totals"][p]), k)
            assert not rows - everyone, rows - everyone
            if k >= int(z["totals"][p]):
                assert rows == everyone
            differs |= not torch.equal(a.u_b[off[p]:off[p + 1]], c.u_b[off[p]:off[p + 1]])
        assert differs


def test_batched_kernel_equals_the_per_pair_kernel():
    from dcn_hip import match
    g = torch.Generator().manual_seed(3)
    P, H, W, D = 3, 20, 28, 5
    res_a = torch.randn(P, H, W, D, generator=g)
    res_b = res_a + 0.4 * torch.randn(P, H, W, D, generator=g)
    mask = (torch.rand(P, H, W, generator=g) < 0.4).to(torch.uint8)
    depth = torch.randint(0, 2000, (P, H, W), generator=g).to(torch.int16)
    cams = torch.from_numpy(np.load(ec.GOLDENS[0])["cams"][:1]).repeat(P, 1)
    counts = [40, 0, 7]                                   # (more than one LDS chunk of queries; a pair without rows)
    off = torch.tensor(np.cumsum([0] + counts))
    R = int(off[-1])
    ua, va = torch.randint(0, W, (R,), generator=g), torch.randint(0, H, (R,), generator=g)
    ub, vb = torch.randint(0, W, (R,), generator=g).float(), torch.randint(0, H, (R,), generator=g).float()
    t = evaluate.match_statistics_pairs(res_a, res_b, mask, depth, depth, cams, ua, va, ub, vb, off)
    assert int(t.status[0]) == 0
    assert np.array_equal(t.mask_pixels.numpy(), mask.view(P, -1).sum(1).numpy())
    for p in range(P):
        lo, hi = int(off[p]), int(off[p + 1])
        if hi == lo:
            continue
        s = match.match_statistics(res_b[p], res_a[p][va[lo:hi], ua[lo:hi]], (ub[lo:hi] + W * vb[lo:hi]).long(), mask[p])
        idx = s["best_idx"]
        assert torch.equal(t.pred_uv[0, lo:hi].long(), idx[0] % W) and torch.equal(t.pred_uv[1, lo:hi].long(), idx[0] // W)
        assert torch.equal(t.pred_uv[2, lo:hi].long(), idx[1] % W) and torch.equal(t.pred_uv[3, lo:hi].long(), idx[1] // W)
        assert torch.equal(t.closer[:, lo:hi], s["count"])
        for name, ref in (("norm_diff_descriptor", s["best_dist"][0]), ("norm_diff_descriptor_masked", s["best_dist"][1]),
                          ("norm_diff_descriptor_ground_truth", s["gt_dist"])):
            np.testing.assert_allclose(t.column(name)[lo:hi].numpy(), ref.numpy(), rtol=1e-5, err_msg=name)
        assert torch.equal(t.row_pair[lo:hi], torch.full((hi - lo,), p, dtype=torch.int32))
        for q in range(lo, hi):
            pred = (int(t.pred_uv[0, q]), int(t.pred_uv[1, q]))
            predm = (int(t.pred_uv[2, q]), int(t.pred_uv[3, q]))
            want = ec.numpy_3d_columns(cams[p].numpy(), depth[p].numpy().view(np.uint16), depth[p].numpy().view(np.uint16),
                                       (int(ua[q]), int(va[q])), (int(ub[q]), int(vb[q])), pred, predm)
            got = (bool(t.is_valid[0, q]), bool(t.is_valid[1, q]), float(t.column("norm_diff_ground_truth_3d")[q]),
                   float(t.column("norm_diff_pred_3d")[q]), float(t.column("norm_diff_pred_3d_masked")[q]))
            assert got[:2] == want[:2]
            np.testing.assert_allclose(got[2:], want[2:], rtol=0, atol=1e-9, equal_nan=True)


@pytest.mark.parametrize("path", fc.GOLDENS, ids=fc.GOLDEN_IDS)
def test_choose_pairs_follows_the_rule(path):
    z = np.load(path)
    store = fc.store_from_golden(z, "cpu")
    got = evaluate.choose_pairs(store, 60, np.random.RandomState(5))
    want = ec.numpy_choose_pairs(store, 60, np.random.RandomState(5))
    assert np.array_equal(got, want) and len(got) > 0
    t = store.translations_host
    assert np.array_equal(t, store.poses.numpy().reshape(-1, 4, 4)[:, :3, 3])
    first = np.asarray(store.scene_first_frame_host)
    for s, a, b in got:
        assert first[s] <= a < first[s + 1] and first[s] <= b < first[s + 1]
        assert np.linalg.norm(t[a] - t[b]) > 0.05
    # never at or below the threshold, whatever it is; a numpy Generator works as well
    got = evaluate.choose_pairs(store, 40, np.random.default_rng(1), threshold=0.3, max_num_attempts=3)
    assert all(np.linalg.norm(t[a] - t[b]) > 0.3 for _, a, b in got)


def test_choose_pairs_skips_a_scene_whose_frames_coincide():
    store = ec.synthetic_store("cpu", 8, 12)
    got = evaluate.choose_pairs(store, 80, np.random.RandomState(0))
    assert 0 < len(got) < 80 and 1 not in got[:, 0].tolist()
    poses = np.stack([np.eye(4)] * 3)
    still = fc.store_from_tables([0, 3], [0], poses, "cpu")
    assert evaluate.choose_pairs(still, 10, np.random.RandomState(0)).shape == (0, 3)


def _tiny_dcn(h, w):
    import pytorch_segmentation_detection.models.resnet_dilated as rd
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    torch.manual_seed(0)
    return DenseCorrespondenceNetwork(rd.Resnet18_8s(num_classes=3, base_width=8), 3, image_width=w, image_height=h)


def test_evaluate_network_on_a_small_store():
    import odd_size_checks as oc
    oc.check_evaluate_on_store("cpu", 32, 48, _tiny_dcn)


def test_error_paths():
    z = np.load(ec.GOLDENS[0])
    d = ec.golden_inputs(z, "cpu")
    rows = [torch.from_numpy(z[k]) for k in ("u_a", "v_a", "u_b", "v_b")]
    off = torch.from_numpy(z["offsets"])
    args = [d["res_a"], d["res_b"], d["mask_b"], d["depth_a"], d["depth_b"], d["cams"]]
    with pytest.raises(ValueError):                        # mismatched descriptor images
        evaluate.match_statistics_pairs(args[0], args[1][:, :-1], *args[2:], *rows, off)
    with pytest.raises(ValueError):                        # a mask of another shape
        evaluate.match_statistics_pairs(args[0], args[1], args[2][:-1], *args[3:], *rows, off)
    with pytest.raises(ValueError):                        # camera rows of the wrong width
        evaluate.match_statistics_pairs(*args[:5], args[5][:, :18], *rows, off)
    with pytest.raises(ValueError):                        # lists of different lengths
        evaluate.match_statistics_pairs(*args, rows[0], rows[1][:-1], rows[2], rows[3], off)
    with pytest.raises(ValueError):                        # offsets of the wrong length
        evaluate.match_statistics_pairs(*args, *rows, off[:-1])
    with pytest.raises(ValueError):                        # match_order of the wrong shape
        evaluate.find_eval_matches(d["depth_a"], d["depth_b"], d["mask_a"], d["cams"], 5, match_order=z["match_order"])
    store = ec.synthetic_store("cpu", 8, 12)
    dcn = _tiny_dcn(8, 12)
    for bad in ([[0, store.num_frames]], [[-1, 0]], [[0, 1, 2, 3]], []):
        with pytest.raises(ValueError):
            evaluate.evaluate_frame_pairs(dcn, store, np.asarray(bad, np.int64).reshape(len(bad), -1))
    # device-side checks: bad rows are flagged, not followed
    bad_u = rows[0].clone()
    bad_u[0] = 10 ** 6
    t = evaluate.match_statistics_pairs(*args, bad_u, *rows[1:], off)
    assert int(t.status[0]) & evaluate.BAD_INDEX
    bad_off = off.clone()
    bad_off[-1] = 10 ** 6
    t = evaluate.match_statistics_pairs(*args, *rows, bad_off)
    assert int(t.status[0]) & evaluate.BAD_OFFSETS
    # offsets that overlap between pairs: flagged, and then no pair has rows
    overlap = off.clone()
    overlap[1] = off[-1]                                   # pair 0 takes every row, pair 1 runs backwards into them
    assert overlap[1] > overlap[2]
    t = evaluate.match_statistics_pairs(*args, *rows, overlap)
    assert int(t.status[0]) & evaluate.BAD_OFFSETS
    assert torch.isnan(t.columns).all() and (t.row_pair == -1).all() and (t.closer == 0).all()
    # the chain's status word carries the match search's: a match_order position outside the pair's matches
    h, w = 32, 48
    store = ec.synthetic_store("cpu", h, w)
    dcn = _tiny_dcn(h, w)
    chosen = evaluate.choose_pairs(store, 3, np.random.RandomState(2))
    good = evaluate.evaluate_frame_pairs(dcn, store, chosen, 4, generator=torch.Generator().manual_seed(1))
    assert int(good.status[0]) == 0 and int(good.offsets[-1]) > 0
    order = np.full((len(chosen), 4), 25, np.int64)        # (position 25: more than the 20 attempts)
    t = evaluate.evaluate_frame_pairs(dcn, store, chosen, 4, generator=torch.Generator().manual_seed(1), match_order=order)
    assert int(t.status[0]) & evaluate.BAD_DRAWS
    # an object without scenes in the store's tables
    store.object_scenes_host = [store.object_scenes_host[0], []]
    with pytest.raises(ValueError, match="has no scene"):
        evaluate.choose_pairs(store, 50, np.random.RandomState(0))
