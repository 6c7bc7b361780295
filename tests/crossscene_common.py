"""Shared by tests/test_emu_crossscene.py and tests/test_gpu_crossscene.py: the crossscene goldens (the reference's own
single_cross_scene_image_pair_quantitative_analysis on two synthetic scenes, tests/golden/
make_crossscene_goldens_from_reference.py) replayed through dcn_hip.evaluate, a stand-in network that returns stored descriptor
images, and random rows for the grouped statistics fed pair-wise to the pair-wise entry."""
import glob
import os

import numpy as np
import torch

import evaluate_common as ec

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "crossscene_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("crossscene_ref_"):-4] for p in GOLDENS]
NO_VIEW, NO_MATCH, FOUND = 0, 1, 2


class StoredNetwork(torch.nn.Module):
    """A ``dcn`` that returns stored descriptor images: frame f's RGB image holds the value f everywhere, which the network
    reads back from the normalized tensor"""

    def __init__(self, table, mean, std):
        super().__init__()
        self.table, self.mean, self.std = table, float(mean[0]), float(std[0])
        self.seen = []

    def forward_image_tensors(self, x):
        assert not self.training
        f = torch.round((x[:, 0, 0, 0] * self.std + self.mean) * 255.0).long()
        self.seen.append(f.cpu().tolist())
        return self.table[f]


def frame_coded_rgb(F, h, w):
    assert F <= 256
    return np.broadcast_to(np.arange(F, dtype=np.uint8)[:, None, None, None], (F, h, w, 3)).copy()


def golden_store(z, device):
    """(store, network) of a golden: its two scenes as a frame store, its descriptor images behind a StoredNetwork"""
    from dcn_hip import augment, frames
    h, w, F = int(z["h"]), int(z["w"]), int(z["poses"].shape[0])
    first = z["first"].tolist()
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    ids = z["frame_ids"].tolist()
    store = frames.FrameStore.from_tensors(
        c(frame_coded_rgb(F, h, w)), c(z["depth"].view(np.int16)), c(z["mask"]), z["poses"], first, [0, 1], z["K"],
        scene_names=[str(s) for s in z["scene_names"]], frame_ids=[ids[first[s]:first[s + 1]] for s in range(2)])
    res = c(z["res_q"].astype(np.float32) * np.float32(z["res_scale"]))
    return store, StoredNetwork(res, augment.DEFAULT_IMAGE_MEAN, augment.DEFAULT_IMAGE_STD_DEV)


def golden_annotations(z):
    """The annotated pair as the reference's parse_cross_scene_data would hold it"""
    ids, px = z["frame_ids"], z["label_pixels"]
    side = lambda scene, frame, c: {"scene_name": str(z["scene_names"][scene]), "image_idx": int(ids[int(frame)]),
                                    "pixels": [{"u": float(p[c]), "v": float(p[c + 1])} for p in px]}
    return [{"image_a": side(0, z["frame_a"], 0), "image_b": side(1, z["frame_b"], 2)}]


def golden_views(z):
    """The views the reference drew, as choose_cross_scene_views' table"""
    from dcn_hip import evaluate
    fa, fb, I = int(z["frame_a"]), int(z["frame_b"]), len(z["label_pixels"])
    rows = [(0, l, evaluate.LABELLED, fa, fb) for l in range(I)]
    for l in range(I):
        for q in np.nonzero(z["request_label"] == l)[0]:
            f = int(z["request_frame"][q])
            rows.append((0, l, evaluate.VIEW_OF_A, f, fb) if z["request_side"][q] == 1 else (0, l, evaluate.VIEW_OF_B, fa, f))
    return np.asarray(rows, np.int64)


def bits(t):
    """A tensor's bit pattern, for comparisons that treat NaN as equal to itself"""
    t = t.contiguous().cpu()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same_tables(a, b):
    for k in ("columns", "is_valid", "pred_uv", "closer", "row_pair", "mask_pixels", "status"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k


def check_golden(z, device, **chain):
    """A golden through the chain with the reference's views replayed: which rows exist, the integer pixels, the projections,
    every column (evaluate_common.check_table and its tolerances), the row order and the names"""
    from dcn_hip import evaluate
    store, net = golden_store(z, device)
    labels = evaluate.cross_scene_labels(store, golden_annotations(z))
    assert labels.skipped == [] and labels.pairs.tolist() == [[0, 0, int(z["frame_a"]), 1, int(z["frame_b"])]]
    views = golden_views(z)
    h, w, I = int(z["h"]), int(z["w"]), len(z["label_pixels"])
    # ---- the reprojection on its own: every request the reference searched
    asked = np.nonzero(z["request_outcome"] != NO_VIEW)[0]
    side, lab = z["request_side"][asked], z["request_label"][asked]
    src = np.where(side == 1, int(z["frame_a"]), int(z["frame_b"]))
    u = np.where(side == 1, labels.pixels[lab, 1], labels.pixels[lab, 3])
    v = np.where(side == 1, labels.pixels[lab, 2], labels.pixels[lab, 4])
    rp = evaluate.reproject_pixels(store, np.stack([src, u, v, z["request_frame"][asked]], axis=1))
    assert int(rp.status.cpu()[0]) == 0
    found = z["request_outcome"][asked] == FOUND
    assert np.array_equal(rp.found.cpu().numpy() != 0, found)                    # exact
    np.testing.assert_allclose(rp.u.cpu().numpy()[found], z["request_u"][asked][found], rtol=0, atol=1e-4)
    np.testing.assert_allclose(rp.v.cpu().numpy()[found], z["request_v"][asked][found], rtol=0, atol=1e-4)
    uv = rp.uv.cpu().numpy()
    assert (uv[:, ~found] == -1).all()
    assert uv[0, found].tolist() == [min(ec.py2_round(x), w - 1) for x in z["request_u"][asked][found]]
    assert uv[1, found].tolist() == [min(ec.py2_round(x), h - 1) for x in z["request_v"][asked][found]]
    # ---- the chain
    net.train()
    t = evaluate.evaluate_cross_scene_rows(net, store, labels, views, **chain)
    assert net.training
    assert int(t.status.cpu()[0]) == 0
    T = I + len(z["request_outcome"])
    assert t.columns.shape == (len(evaluate.COLUMNS), T) and views.shape[0] == T
    pair = t.row_pair.cpu().numpy()
    expect = np.concatenate([np.ones(I, bool), np.zeros(len(z["request_outcome"]), bool)])
    for l in range(I):                                     # (the table's order: per label its 10 + 10 requests)
        q = np.nonzero(z["request_label"] == l)[0]
        expect[I + q] = z["request_outcome"][q] == FOUND
    assert np.array_equal(pair >= 0, expect) and (pair[expect] == 0).all() and (pair[~expect] == -1).all()
    sel = np.nonzero(expect)[0]
    R = len(sel)
    assert R == len(z["row_request"])                      # the reference's rows, in its order
    assert np.array_equal(sel[I:] - I, z["row_request"][I:]) and (z["row_request"][:I] == -1).all()
    assert np.array_equal(t.u_a.cpu().numpy()[sel], z["u_a"]) and np.array_equal(t.v_a.cpu().numpy()[sel], z["v_a"])
    ub, vb = t.u_b.cpu().numpy()[sel], t.v_b.cpu().numpy()[sel]
    assert [min(ec.py2_round(x), w - 1) for x in ub] == z["gt_u"].tolist()
    assert [min(ec.py2_round(x), h - 1) for x in vb] == z["gt_v"].tolist()
    of_b = z["row_request"] >= 0
    of_b[of_b] = z["request_side"][z["row_request"][of_b]] == 2
    np.testing.assert_allclose(ub[of_b], z["request_u"][z["row_request"][of_b]], rtol=0, atol=1e-4)
    np.testing.assert_allclose(vb[of_b], z["request_v"][z["row_request"][of_b]], rtol=0, atol=1e-4)
    # rows without a result look like rows past the end
    gone = torch.from_numpy(np.nonzero(~expect)[0]).to(t.columns.device)
    assert torch.isnan(t.columns[:, gone]).all() and (t.pred_uv[:, gone] == -1).all() and (t.closer[:, gone] == 0).all()
    assert (t.is_valid[:, gone] == 0).all() and (t.mask_pixels[gone] == 0).all()
    # every column: check_table wants the rows in use and one searched image per "pair" -- here one per row
    at = torch.from_numpy(sel).to(t.columns.device)
    compact = t._replace(columns=t.columns[:, at], is_valid=t.is_valid[:, at], pred_uv=t.pred_uv[:, at],
                         closer=t.closer[:, at], row_pair=torch.arange(R, dtype=torch.int32), mask_pixels=t.mask_pixels[at])
    zz = {k: z[k] for k in z.files}
    zz["row_pair"], zz["mask_b"] = np.arange(R), z["mask"][z["search_frame"]]
    ec.check_table(compact, zz)
    # the names
    table = evaluate.cross_scene_table(store, labels, views, t)
    assert table["scene_name"].tolist() == [str(s) for s in z["scene_name"]]
    assert np.array_equal(table["img_a_idx"], z["img_a_idx"]) and np.array_equal(table["img_b_idx"], z["img_b_idx"])
    assert np.array_equal(table["is_valid"], z["is_valid"]) and len(table["norm_diff_descriptor"]) == R
    assert np.array_equal(bits(torch.from_numpy(table["pixel_match_error_l2"])), bits(compact.columns[6]))
    # one forward pass per distinct frame: a's side first, then the searched frames
    seen = sum(net.seen, [])
    a_side = sorted(set(views[(views[:, 3] >= 0) & (views[:, 4] >= 0), 3].tolist()))
    b_side = sorted(set(views[(views[:, 3] >= 0) & (views[:, 4] >= 0), 4].tolist()))
    assert seen == a_side + b_side
    return store, net, labels, views, t


def random_groups(sizes, h, w, d, seed, device="cpu", keep_fraction=0.8):
    """Rows for match_statistics_groups (one group per entry of ``sizes``) together with the same rows as pairs of images for
    match_statistics_pairs, one pair per row: -> (groups dict, pairs dict)"""
    g = torch.Generator().manual_seed(seed)
    G, R = len(sizes), int(sum(sizes))
    group = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    res_b = torch.randn(G, h, w, d, generator=g)
    mask_b = (torch.rand(G, h, w, generator=g) < 0.4).to(torch.uint8)
    depth = lambda n: torch.where(torch.rand(n, h, w, generator=g) < 0.1, torch.zeros(n, h, w),
                                  800 + 200 * torch.rand(n, h, w, generator=g)).to(torch.int16)
    depth_b, depth_a = depth(G), depth(R)
    res_a = torch.randn(R, h, w, d, generator=g)
    u_a, v_a = torch.randint(0, w, (R,), generator=g), torch.randint(0, h, (R,), generator=g)
    u_b = torch.rand(R, generator=g) * (w + 0.4)           # (some round past the last column)
    v_b = torch.rand(R, generator=g) * (h + 0.4)
    cams = torch.zeros(R, 50)
    K = torch.tensor([[533.6 * w / 640.0, 0, 0.5 * w], [0, 534.8 * h / 480.0, 0.5 * h], [0, 0, 1.0]])
    cams[:, :9], cams[:, 9:18] = K.reshape(-1), torch.linalg.inv(K).reshape(-1)
    for c in (18, 34):
        pose = torch.eye(4).repeat(R, 1, 1)
        pose[:, :3, 3] = 0.05 * torch.randn(R, 3, generator=g)
        cams[:, c:c + 16] = pose.reshape(R, 16)
    keep = (torch.rand(R, generator=g) < keep_fraction).to(torch.uint8)
    rows = torch.arange(R)
    offsets = torch.tensor(np.cumsum([0] + list(sizes)), dtype=torch.int64)
    to = lambda t: t.to(device)
    groups = dict(res_b=to(res_b), mask_b=to(mask_b), depth_b=to(depth_b), queries=to(res_a[rows, v_a, u_a].contiguous()),
                  u_a=to(u_a), v_a=to(v_a), depth_q=to(depth_a[rows, v_a, u_a].contiguous()), u_b=to(u_b), v_b=to(v_b),
                  cams=to(cams), keep=to(keep), offsets=to(offsets))
    pairs = dict(res_a=to(res_a), res_b=to(res_b[group].contiguous()), mask_b=to(mask_b[group].contiguous()),
                 depth_a=to(depth_a), depth_b=to(depth_b[group].contiguous()), cams=to(cams), u_a=to(u_a), v_a=to(v_a),
                 u_b=to(u_b), v_b=to(v_b), offsets=to(torch.arange(R + 1, dtype=torch.int64)))
    return groups, pairs, group


def check_groups_against_pairs(groups, pairs, group, **kw):
    """The grouped entry and the pair-wise entry on the same rows: integers equal, floats equal bit for bit; a row left out
    looks like a row past the end"""
    from dcn_hip import evaluate
    tg = evaluate.match_statistics_groups(max_group_rows=kw.pop("max_group_rows", None), **groups)
    tp = evaluate.match_statistics_pairs(**pairs)
    assert int(tg.status.cpu()[0]) == 0 and int(tp.status.cpu()[0]) == 0
    keep = groups["keep"].cpu() != 0
    on, off = torch.nonzero(keep)[:, 0], torch.nonzero(~keep)[:, 0]
    for k in ("columns", "is_valid", "pred_uv", "closer"):
        assert torch.equal(bits(getattr(tg, k))[:, on], bits(getattr(tp, k))[:, on]), k
    assert torch.equal(tg.row_pair.cpu()[on].long(), group[on]) and torch.equal(tp.row_pair.cpu()[on].long(), on)
    assert torch.equal(tg.mask_pixels.cpu(), groups["mask_b"].cpu().view(len(tg.mask_pixels), -1).ne(0).sum(1).int())
    assert torch.equal(tp.mask_pixels.cpu(), tg.mask_pixels.cpu()[group])
    assert torch.isnan(tg.columns.cpu()[:, off]).all() and (tg.pred_uv.cpu()[:, off] == -1).all()
    assert (tg.row_pair.cpu()[off] == -1).all() and (tg.closer.cpu()[:, off] == 0).all() and (tg.is_valid.cpu()[:, off] == 0).all()
    return tg, tp
