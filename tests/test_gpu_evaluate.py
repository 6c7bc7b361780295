"""Evaluation on frame-store image pairs (csrc/evaluate_kernels.hip, dcn_hip/evaluate/pairs.py) on the MI355X: the evalpairs goldens
(the reference's own match search, subsample and statistics), and one full-size case -- 480 x 640, D = 3, 8 pairs of a synthetic
store -- for the batched kernel against the per-pair kernel plus a float64 numpy restatement of the 3D half, and for
evaluate_frame_pairs with the real backbone against the same pipeline run pair by pair.  Reads tests/golden only."""
import numpy as np
import pytest
import torch

import evaluate_common as ec
from dcn_hip import evaluate
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu

H, W, D, P = 480, 640, 3, 8


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("path", ec.GOLDENS, ids=ec.GOLDEN_IDS)
def test_golden_matches_and_table(path):
    z = np.load(path)
    d = ec.golden_inputs(z, "cuda")
    m = ec.golden_matches(z, d)
    ec.check_matches(m, z)
    t = evaluate.match_statistics_pairs(d["res_a"], d["res_b"], d["mask_b"], d["depth_a"], d["depth_b"], d["cams"], m.u_a, m.v_a,
                                        m.u_b, m.v_b, m.offsets, max_pair_rows=int(z["num_attempts"]))
    R = len(z["row_pair"])
    full = evaluate.EvalTable(t.columns[:, :R], t.is_valid[:, :R], t.pred_uv[:, :R], t.closer[:, :R], t.row_pair[:R],
                              *t[5:])
    ec.check_table(full, z)
    assert torch.isnan(t.columns[:, R:]).all() and (t.row_pair[R:] == -1).all() and (t.pred_uv[:, R:] == -1).all()


@pytest.mark.parametrize("path", ec.GOLDENS, ids=ec.GOLDEN_IDS)
def test_golden_table_from_the_reference_rows(path):
    z = np.load(path)
    d = ec.golden_inputs(z, "cuda")
    c = lambda k: torch.from_numpy(z[k]).cuda()
    t = evaluate.match_statistics_pairs(d["res_a"], d["res_b"], d["mask_b"], d["depth_a"], d["depth_b"], d["cams"], c("u_a"),
                                        c("v_a"), c("u_b"), c("v_b"), c("offsets"))
    ec.check_table(t, z)


def _chosen(store):
    chosen = evaluate.choose_pairs(store, P, np.random.RandomState(1))
    assert len(chosen) == P
    return chosen


def _gathered(store, chosen):
    a, b = torch.from_numpy(chosen[:, 1]).cuda(), torch.from_numpy(chosen[:, 2]).cuda()
    from dcn_hip import samples
    poses = store.poses.cpu().numpy().reshape(-1, 4, 4)
    cams = samples._cameras(store.K[chosen[:, 0]], poses[chosen[:, 1]], poses[chosen[:, 2]], len(chosen), torch.device("cuda"))
    return store.depth[a], store.depth[b], store.mask[a], store.mask[b], cams


def test_full_size_batched_kernel_against_per_pair_kernel_and_numpy_3d():
    from dcn_hip import match
    store = ec.synthetic_store("cuda", H, W, still_scene=False)
    chosen = _chosen(store)
    depth_a, depth_b, mask_a, mask_b, cams = _gathered(store, chosen)
    g = torch.Generator("cuda").manual_seed(2)
    res_a = torch.randn(P, H, W, D, device="cuda", generator=g)
    res_b = torch.roll(res_a, (0, 30), dims=(1, 2)) + 0.3 * torch.randn(P, H, W, D, device="cuda", generator=g)
    m = evaluate.find_eval_matches(depth_a, depth_b, mask_a, cams, 100, generator=g)
    t = evaluate.match_statistics_pairs(res_a, res_b, mask_b, depth_a, depth_b, cams, m.u_a, m.v_a, m.u_b, m.v_b, m.offsets,
                                        max_pair_rows=evaluate.NUM_ATTEMPTS)
    assert int(t.status.cpu()[0]) == 0 and int(m.status.cpu()[0]) == 0
    off = m.offsets.cpu().numpy()
    assert off[-1] >= 4 * P, off                                # (the synthetic views overlap: most attempts survive)
    assert np.array_equal(t.mask_pixels.cpu().numpy(), mask_b.view(P, -1).sum(1).cpu().numpy())
    cols = {k: t.column(k).cpu().numpy() for k in evaluate.COLUMNS}
    pred, valid = t.pred_uv.cpu().numpy(), t.is_valid.cpu().numpy()
    ua, va, ub, vb = (x.cpu().numpy() for x in (m.u_a, m.v_a, m.u_b, m.v_b))
    da, db, cm = depth_a.cpu().numpy().view(np.uint16), depth_b.cpu().numpy().view(np.uint16), cams.cpu().numpy()
    for p in range(P):
        lo, hi = int(off[p]), int(off[p + 1])
        if hi == lo:
            continue
        gu = np.array([min(ec.py2_round(x), W - 1) for x in ub[lo:hi]])
        gv = np.array([min(ec.py2_round(x), H - 1) for x in vb[lo:hi]])
        s = match.match_statistics(res_b[p], res_a[p][m.v_a[lo:hi], m.u_a[lo:hi]], torch.from_numpy(gu + W * gv).cuda(),
                                   mask_b[p])
        idx = s["best_idx"].cpu().numpy()
        assert np.array_equal(pred[0, lo:hi], idx[0] % W) and np.array_equal(pred[1, lo:hi], idx[0] // W)
        assert np.array_equal(pred[2, lo:hi], idx[1] % W) and np.array_equal(pred[3, lo:hi], idx[1] // W)
        assert np.array_equal(t.closer[:, lo:hi].cpu().numpy(), s["count"].cpu().numpy())
        for name, ref in (("norm_diff_descriptor", s["best_dist"][0]), ("norm_diff_descriptor_masked", s["best_dist"][1]),
                          ("norm_diff_descriptor_ground_truth", s["gt_dist"])):
            np.testing.assert_allclose(cols[name][lo:hi], ref.cpu().numpy(), rtol=1e-5, err_msg=name)
        cnt = s["count"].cpu().numpy().astype(np.float64)
        avg = np.where(cnt > 0, s["dist_sum"].cpu().numpy() / np.maximum(cnt, 1), 0.0)
        np.testing.assert_allclose(cols["average_l2_distance_for_false_positives"][lo:hi], avg[0], rtol=1e-4)
        np.testing.assert_allclose(cols["average_l2_distance_for_false_positives_masked"][lo:hi], avg[1], rtol=1e-4)
        for q in range(lo, hi):
            want = ec.numpy_3d_columns(cm[p], da[p], db[p], (int(ua[q]), int(va[q])), (int(gu[q - lo]), int(gv[q - lo])),
                                       (int(pred[0, q]), int(pred[1, q])), (int(pred[2, q]), int(pred[3, q])))
            got = (bool(valid[0, q]), bool(valid[1, q]), cols["norm_diff_ground_truth_3d"][q], cols["norm_diff_pred_3d"][q],
                   cols["norm_diff_pred_3d_masked"][q])
            assert got[:2] == want[:2]
            np.testing.assert_allclose(got[2:], want[2:], rtol=0, atol=1e-9, equal_nan=True)
            l2 = np.hypot(float(gu[q - lo] - pred[0, q]), float(gv[q - lo] - pred[1, q]))
            assert abs(cols["pixel_match_error_l2"][q] - l2) <= 1e-6 * max(1.0, l2)
    assert not np.isnan(cols["norm_diff_pred_3d"]).all() and np.isfinite(cols["norm_diff_ground_truth_3d"]).any()


def test_full_size_evaluate_frame_pairs_against_the_pipeline_pair_by_pair():
    """The real backbone; descriptors are computed twice (8 pairs at a time in batches of 3, then pair by pair), so the
    descriptors carry the backbone's batch-shape dependence.  The backbone's parity bound is 1e-4 of the descriptor image's
    largest magnitude per element (the bound of smoke() and the parity tests), so a distance between two descriptors of D
    elements may move by tol = 2 * sqrt(D) * 1e-4 * max|descriptor|: that is the tolerance of the distance columns.  The
    chosen pixel may differ only where a runner-up lies within 2 * tol of the best (checked row by row on the per-pair
    descriptors); the pixel-dependent columns, image and masked, are compared on the rows where it is the same.  How many
    rows that must be: with descriptors spread in D = 3 dimensions the number of pixels within distance r of a query grows
    like (r / d1)^3, d1 the best distance, so about 3 * 2 * tol / d1 pixels are expected within 2 * tol of the best -- a few
    per cent of the rows for d1 of some 1e-2 .. 1e-1 and tol of some 1e-4 -- so at least 0.8 of the rows must agree."""
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    store = ec.synthetic_store("cuda", H, W, still_scene=False)
    chosen = _chosen(store)
    torch.manual_seed(0)
    dcn = DenseCorrespondenceNetwork.from_config({"descriptor_dimension": D, "image_width": W, "image_height": H},
                                                 load_stored_params=False)
    assert dcn.training
    seed = 11
    t = evaluate.evaluate_frame_pairs(dcn, store, chosen, 100, generator=torch.Generator("cuda").manual_seed(seed),
                                      batch_pairs=3)
    assert dcn.training and int(t.status.cpu()[0]) == 0
    off = t.offsets.cpu().numpy()
    assert off[-1] >= 4 * P
    # the same generator stream pair by pair: the seeds of all pairs are drawn first (two draws of P), then used per pair
    g = torch.Generator("cuda").manual_seed(seed)
    from dcn_hip import samples
    cand_seeds, order_seeds = samples.draw_seeds(P, store.device, g), samples.draw_seeds(P, store.device, g)
    depth_a, depth_b, mask_a, mask_b, cams = _gathered(store, chosen)
    mean = torch.tensor(evaluate._aug.DEFAULT_IMAGE_MEAN, device="cuda").view(3, 1, 1)
    std = torch.tensor(evaluate._aug.DEFAULT_IMAGE_STD_DEV, device="cuda").view(3, 1, 1)
    dcn.eval()
    rows, all_same, bands = 0, ([], []), ([], [])
    for p in range(P):
        m = evaluate.find_eval_matches(depth_a[p:p + 1], depth_b[p:p + 1], mask_a[p:p + 1], cams[p:p + 1], 100,
                                       seeds=cand_seeds[p:p + 1], order_seeds=order_seeds[p:p + 1])
        lo, hi = int(off[p]), int(off[p + 1])
        n = int(m.offsets.cpu()[1])
        assert n == hi - lo
        assert torch.equal(m.u_a[:n], t.u_a[lo:hi]) and torch.equal(m.u_b[:n], t.u_b[lo:hi])
        if n == 0:
            continue
        rows += n
        res = []
        for f in (int(chosen[p, 1]), int(chosen[p, 2])):
            x = (store.rgb[f].permute(2, 0, 1).float().div(255) - mean) / std
            res.append(dcn.forward_single_image_tensor(x))
        tol = 2.0 * np.sqrt(D) * 1e-4 * float(max(res[0].abs().max(), res[1].abs().max()))
        one = evaluate.match_statistics_pairs(res[0][None], res[1][None], mask_b[p:p + 1], depth_a[p:p + 1], depth_b[p:p + 1],
                                              cams[p:p + 1], m.u_a[:n], m.v_a[:n], m.u_b[:n], m.v_b[:n], m.offsets)
        for k in ("norm_diff_descriptor_ground_truth", "norm_diff_descriptor", "norm_diff_descriptor_masked"):
            a, b = t.column(k)[lo:hi].cpu().numpy(), one.column(k).cpu().numpy()
            np.testing.assert_allclose(a, b, rtol=0, atol=tol, err_msg=k)
        # per-pair distance images of the rows (float64 on the per-pair descriptors) for the near-tie and band arguments
        q = res[0][m.v_a[:n], m.u_a[:n]].double()
        nd = (res[1].reshape(1, H * W, D).double() - q[:, None, :]).norm(dim=2)              # [n, HW]
        on = mask_b[p].reshape(-1) != 0
        gt_d = one.column("norm_diff_descriptor_ground_truth").double()
        rr = torch.arange(n, device="cuda")
        for half, (ku, kv, masked) in enumerate(((0, 1, ""), (2, 3, "_masked"))):
            same = ((t.pred_uv[ku, lo:hi] == one.pred_uv[ku]) & (t.pred_uv[kv, lo:hi] == one.pred_uv[kv]))
            # a different pixel is allowed only as a near-tie: on the per-pair descriptors the batched path's pixel is within
            # 2 * tol of the best distance (each of the two distances may have moved by tol)
            alt = nd[rr, t.pred_uv[kv, lo:hi].long() * W + t.pred_uv[ku, lo:hi].long()]
            best = one.column("norm_diff_descriptor" + masked).double()
            assert bool(((alt - best <= 2 * tol) | same).all()), (p, masked)
            same = same.cpu().numpy()
            all_same[half].append(same)
            cols = ("norm_diff_pred_3d", "pixel_match_error_l2") + (("pixel_match_error_l1",) if not masked else ())
            for k in cols:
                np.testing.assert_allclose(t.column(k + masked)[lo:hi].cpu().numpy()[same],
                                           one.column(k + masked).cpu().numpy()[same], rtol=0, atol=1e-9, equal_nan=True,
                                           err_msg=k + masked)
            assert np.array_equal(t.is_valid[half, lo:hi].cpu().numpy()[same], one.is_valid[half].cpu().numpy()[same])
            # closer-than-ground-truth counts: only a pixel whose distance lies within 2 * tol of the ground truth's can be
            # counted by one run and not by the other, so the band's population bounds the difference; where the band is
            # empty the counted sets are the same and so are the (order-independent) averages
            cand = on[None, :] if masked else torch.ones_like(on)[None, :]
            band = (((nd - gt_d[:, None]).abs() <= 2 * tol) & cand).sum(1).cpu().numpy()
            diff = np.abs(t.closer[half, lo:hi].cpu().numpy().astype(np.int64) - one.closer[half].cpu().numpy())
            assert (diff <= band).all(), (p, masked, diff, band)
            denom = float(on.sum()) if masked else float(H * W)
            fk = "fraction_pixels_closer_than_ground_truth" + masked
            assert (np.abs(t.column(fk)[lo:hi].cpu().numpy() - one.column(fk).cpu().numpy()) <= band / denom + 1e-12).all()
            ak = "average_l2_distance_for_false_positives" + masked
            empty = band == 0
            bands[half].append(empty)
            np.testing.assert_allclose(t.column(ak)[lo:hi].cpu().numpy()[empty], one.column(ak).cpu().numpy()[empty], rtol=0,
                                       atol=1e-9, err_msg=ak)
        np.testing.assert_allclose(t.column("norm_diff_ground_truth_3d")[lo:hi].cpu().numpy(),
                                   one.column("norm_diff_ground_truth_3d").cpu().numpy(), rtol=0, atol=1e-9, equal_nan=True)
    assert rows == off[-1]
    for half, name in enumerate(("image", "masked")):
        same, empty = np.concatenate(all_same[half]), np.concatenate(bands[half])
        print("%s: rows with the same best match %d of %d; rows with an empty band around the ground truth %d"
              % (name, int(same.sum()), rows, int(empty.sum())))
        assert same.mean() >= 0.8, (name, same.mean())


def test_evaluate_network_returns_the_reference_columns():
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    h, w = 64, 96
    store = ec.synthetic_store("cuda", h, w)
    dcn = DenseCorrespondenceNetwork.from_config({"descriptor_dimension": D, "image_width": w, "image_height": h},
                                                 load_stored_params=False)
    dcn.eval()
    table, _df = evaluate.evaluate_network(dcn, store, num_image_pairs=10, num_matches_per_image_pair=100,
                                           host_rng=np.random.RandomState(0), generator=torch.Generator("cuda").manual_seed(0))
    assert not dcn.training
    assert set(evaluate.COLUMNS) | {"is_valid", "is_valid_masked", "scene_name", "img_a_idx", "img_b_idx"} == set(table)
    n = len(table["is_valid"])
    assert n > 0 and all(len(v) == n for v in table.values())
    assert np.isfinite(table["norm_diff_descriptor"]).all() and (table["pixel_match_error_l2"] >= 0).all()
    assert "scene_1" not in table["scene_name"].tolist()          # (its frames coincide: never chosen)
