"""The cross-scene and cross-instance tables (csrc/crossscene_kernels.hip): ``evaluate_network_cross_scene``
(evaluation.py:253-301, :610-781) and ``evaluate_network_cross_instance`` (:350-404)."""
import collections
import ctypes

import numpy as np
import torch

from .. import _args, _lib
from .. import augment as _aug
from ._chain import (BAD_FRAME, COLUMNS, _alloc_eval_table, _below, _camera_rows_of, _columns_to_dict, _dataframe,
                     _descriptor_images, _empty_table, _eval_table_of, _forward_in_eval_mode, _gather_frame_list, _image_index,
                     _nan_table, _offsets_arg, _on_device, _py2_round, _queries_arg, _queries_of_frames, _rows, _table_block,
                     _uploader, _valid_pointers, _yaml_file)

CrossSceneLabels = collections.namedtuple("CrossSceneLabels", "pairs pixels skipped")
LABELLED, VIEW_OF_A, VIEW_OF_B = 0, 1, 2      # a row's kind in choose_cross_scene_views' table


def cross_scene_labels(store, annotated_pairs):
    """The reference's list of human-labelled cross-scene matches (``parse_cross_scene_data``, evaluation.py:1844-1874: dicts
    ``image_a`` / ``image_b``: {scene_name, image_idx, pixels: [{u, v}, ...]}) resolved to the frames of ``store`` through
    ``store.scene_names`` / ``store.frame_ids``, the pixels rounded and clipped like the reference
    (clip_pixel_to_image_size_and_round, :604-607: Python 2's ``round``, ``min(..., size - 1)``).

    -> CrossSceneLabels: ``pairs`` int64 [N, 5] of (index in ``annotated_pairs``, scene a, frame a, scene b, frame b), frames
    as store indices; ``pixels`` int64 [L, 5] of (row of ``pairs``, u_a, v_a, u_b, v_b), the labels of a pair in the order
    given; ``skipped``: [(index, reason)] for the pairs naming a scene or an image the store does not hold (the reference
    skips the pairs whose scene directories are missing, :269-272).  ValueError for an empty list of pairs, for pixel lists of
    unequal length (the reference's assert, :660) and for a pixel that rounds below zero -- the reference would index from the
    far edge of the image there without saying so."""
    if annotated_pairs is None or len(annotated_pairs) == 0:
        raise ValueError("no annotated cross-scene pairs given")
    first = store.scene_first_frame_host
    pairs, pixels, skipped = [], [], []
    for i, ap in enumerate(annotated_pairs):
        side = [ap["image_a"], ap["image_b"]]
        if len(side[0]["pixels"]) != len(side[1]["pixels"]):
            raise ValueError("annotated pair %d: %d pixels in image a but %d in image b" % (i, len(side[0]["pixels"]),
                                                                                          len(side[1]["pixels"])))
        uv = []
        for a, b in zip(side[0]["pixels"], side[1]["pixels"]):
            row = [min(_py2_round(x), size - 1) for x, size in ((a["u"], store.w), (a["v"], store.h), (b["u"], store.w),
                                                                (b["v"], store.h))]
            if min(row) < 0:
                raise ValueError("annotated pair %d: a labelled pixel is negative: %s / %s" % (i, dict(a), dict(b)))
            uv.append(row)
        found = []
        for im in side:
            if im["scene_name"] not in store.scene_names:
                skipped.append((i, "the store holds no scene %r" % (im["scene_name"],)))
                break
            sc = store.scene_names.index(im["scene_name"])
            ids = [int(x) for x in store.frame_ids[sc]]
            if int(im["image_idx"]) not in ids:
                skipped.append((i, "scene %r holds no image %r" % (im["scene_name"], im["image_idx"])))
                break
            found.extend([sc, first[sc] + ids.index(int(im["image_idx"]))])
        else:
            pixels.extend([len(pairs)] + row for row in uv)
            pairs.append([i] + found)
    return CrossSceneLabels(np.asarray(pairs, np.int64).reshape(-1, 5), np.asarray(pixels, np.int64).reshape(-1, 5), skipped)


def _different_pose(poses, lo, cnt, fa, rng, threshold, angle_threshold, num_attempts):
    """``get_img_idx_with_different_pose`` (dense_correspondence_dataset_masked.py:260-287) on host poses [F, 4, 4]: the first
    of up to ``num_attempts`` uniform frames of [lo, lo + cnt) that passes the test against frame ``fa``, or -1"""
    Ra, ta = poses[fa, :3, :3], poses[fa, :3, 3]
    for _ in range(int(num_attempts)):
        f = lo + _below(rng, cnt)
        c = min(1.0, max(-1.0, (float(np.sum(Ra * poses[f, :3, :3])) - 1.0) * 0.5))
        if np.linalg.norm(ta - poses[f, :3, 3]) > threshold or 2.0 * np.arccos(c) > angle_threshold:
            return f
    return -1


def choose_cross_scene_views(store, labels, num_views_a=10, num_views_b=10, host_rng=None, threshold=0.2, angle_threshold=20,
                             num_attempts=50):
    """The other views single_cross_scene_image_pair_quantitative_analysis draws (evaluation.py:702-757), on the host: per
    labelled match ``num_views_a`` (the reference's J = 10) views of scene a, then ``num_views_b`` (K = 10) of scene b, each by
    ``get_img_idx_with_different_pose(scene, pose, num_attempts=50)``: the first of up to ``num_attempts`` uniform frames of the
    scene whose translation is more than ``threshold`` from the labelled image's (float64 norm) or whose angle to it exceeds
    ``angle_threshold``; when none does there is no view (the reference ``continue``s).  The angle is taken in the reference's
    own units, as the frame selection on the device does: ``compute_angle_between_poses`` returns radians, at most 2 pi, and is
    compared with 20 -- so that clause never fires for a proper rotation.  Reads ``store.poses_host``; ``host_rng``: a numpy
    RandomState / Generator (default ``np.random``).  As in ``choose_pairs`` only the rule is replayed, not the reference's
    ``random`` stream (``get_random_image_index`` draws twice and discards one).

    -> int64 array [T, 5] of (row of ``labels.pairs``, row of ``labels.pixels``, kind, frame a, frame b): the two frames the
    row compares, as store indices, in the reference's row order -- per annotated pair its I labelled rows (kind LABELLED),
    then per label its a-views (VIEW_OF_A: frame a is the view) and its b-views (VIEW_OF_B: frame b is the view), with -1
    for "no view".  T = sum over the pairs of I + I * (num_views_a + num_views_b)."""
    rng = host_rng if host_rng is not None else np.random
    first, poses = store.scene_first_frame_host, store.poses_host
    out = []
    for n, (_i, sa, fa, sb, fb) in enumerate(labels.pairs.tolist()):
        mine = np.nonzero(labels.pixels[:, 0] == n)[0].tolist()
        out.extend((n, l, LABELLED, fa, fb) for l in mine)
        for l in mine:
            for _j in range(int(num_views_a)):
                out.append((n, l, VIEW_OF_A, _different_pose(poses, first[sa], first[sa + 1] - first[sa], fa, rng, threshold,
                                                             angle_threshold, num_attempts), fb))
            for _k in range(int(num_views_b)):
                out.append((n, l, VIEW_OF_B, fa, _different_pose(poses, first[sb], first[sb + 1] - first[sb], fb, rng,
                                                                 threshold, angle_threshold, num_attempts)))
    return np.asarray(out, dtype=np.int64).reshape(-1, 5)


Reprojection = collections.namedtuple("Reprojection", "found u v uv status")


def reproject_pixels(store, requests, K=None):
    """``batch_find_pixel_correspondences(depth_src, pose_src, depth_dst, pose_dst, uv_a=(u, v))`` (correspondence_finder.py
    :409-619) for V single pixels over the frames of ``store``, nothing gathered: ``requests`` integer [V, 4] of (src frame, u,
    v, dst frame), host array or device tensor.  K: [3, 3] on the host; the default is ``get_default_K_matrix()`` and NOT the
    scene's K, because the reference passes no K to this search -- while the statistics of the resulting rows use scene a's K
    (evaluation.py:653-658, :721, :756).  That is how the reference does it.
    -> Reprojection: found uint8 [V]; u, v float32 [V], the projection as the reference's search returns it; uv int32 [2, V],
    its ``clip_pixel_to_image_size_and_round`` (-1 when not found); status int32 [1] (BAD_FRAME for a frame or a pixel outside
    the store: that request is not found).  The answer is the one find_eval_matches gives that candidate pixel.  No host
    synchronization."""
    lib = _lib.get()
    dev = store.device
    if torch.is_tensor(requests):
        req = requests.to(device=dev, dtype=torch.int32)
    else:
        req = torch.from_numpy(np.ascontiguousarray(np.asarray(requests, np.int64).astype(np.int32))).to(dev)
    if req.dim() != 2 or int(req.shape[1]) != 4:
        raise ValueError("requests must be [V, 4] of (src frame, u, v, dst frame), got %s" % (tuple(req.shape),))
    req = req.contiguous()
    V = int(req.shape[0])
    kcam = torch.from_numpy(np.ascontiguousarray(_args.camera_k_rows(K, 1)[1][0], dtype=np.float32)).to(dev)
    _on_device(req, kcam)
    found = torch.empty(V, dtype=torch.uint8, device=dev)
    u, v = torch.empty(V, dtype=torch.float32, device=dev), torch.empty(V, dtype=torch.float32, device=dev)
    uv = torch.empty((2, V), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if V:
        p = _lib.ptr
        rc = lib.dcn_reproject_pixels(V, ctypes.byref(store.desc), p(kcam), p(req), p(found), p(u), p(v), p(uv), p(status),
                                      _lib.stream_ptr())
        _lib.check(rc, "dcn_reproject_pixels")
    return Reprojection(found, u, v, uv, status)


def match_statistics_groups(res_b, mask_b, depth_b, queries, u_a, v_a, depth_q, u_b, v_b, cams, keep, offsets,
                            max_group_rows=None, _strip_pixels=None):
    """``match_statistics_pairs`` for GROUPS of rows that search one image, each row with a query of its own: every column of
    the reference's evaluation table, in two launches, with res_b read once whatever the number of rows.

    res_b: float32 [G, H, W, D]; mask_b: [G, H, W]; depth_b: 16-bit [G, H, W] millimetres -- the searched images.  Per row:
    queries float32 [R, D]; u_a, v_a int64 [R], the query pixel; depth_q 16-bit [R], the depth there; u_b, v_b float32 [R], the
    ground truth in the group's image (rounded and clipped like the reference); cams float32 [R, 50] (K, K^-1, pose a, pose
    b^-1); keep uint8 / bool [R]: a row with keep == 0 costs no search and comes out like a row past the end (NaN, -1, pair
    -1).  offsets: int64 [G + 1] device tensor, group g's rows at offsets[g]:offsets[g+1]; max_group_rows: a bound on one
    group's rows (default R).
    -> EvalTable, ``row_pair`` holding the row's group and ``mask_pixels`` int32 [G].  The arithmetic is
    match_statistics_pairs' (the same device functions).  No host synchronization."""
    lib = _lib.get()
    rb, G, h, w, d = _descriptor_images(res_b, "res_b")
    mb, db = _args.mask(mask_b, G, h, w, "mask_b"), _args.depth(depth_b, G, h, w, "depth_b")
    q = _queries_arg(queries, d)
    R = int(q.shape[0])
    ua, va = _rows(u_a, torch.int64, "u_a", R), _rows(v_a, torch.int64, "v_a", R)
    ub, vb = _rows(u_b, torch.float32, "u_b", R), _rows(v_b, torch.float32, "v_b", R)
    if depth_q.dim() != 1 or int(depth_q.numel()) != R or depth_q.element_size() != 2 or depth_q.is_floating_point():
        raise ValueError("depth_q must be 16-bit integer [%d] millimetres, got %s %s" % (R, depth_q.dtype, tuple(depth_q.shape)))
    dq = depth_q.contiguous()
    cams = _args.camera_rows(cams, R, "cams")
    if keep.dtype not in (torch.uint8, torch.bool) or keep.dim() != 1 or int(keep.numel()) != R:
        raise ValueError("keep must be uint8 (or bool) [%d], got %s %s" % (R, keep.dtype, tuple(keep.shape)))
    kp = keep.to(torch.uint8).contiguous()
    off = _offsets_arg(offsets, G, "G")
    _on_device(rb, mb, db, q, ua, va, dq, ub, vb, cams, kp, off)
    cap = max(R, 1)
    q, ua, va, ub, vb, dq, cams, kp = _valid_pointers(R, q, ua, va, ub, vb, dq, cams, kp)
    mgr = cap if max_group_rows is None else max(1, min(int(max_group_rows), cap))
    outs = _alloc_eval_table(cap, G, rb.device, lib.dcn_match_statistics_groups_workspace(cap))
    p = _lib.ptr
    rows_in = (G, h, w, d, p(rb), p(mb), p(db), p(q), p(ua), p(va), p(dq), p(ub), p(vb), p(cams), p(kp), p(off), cap, mgr)
    rows_out = tuple(p(t) for t in outs) + (_lib.stream_ptr(),)
    if _strip_pixels is None:
        _lib.check(lib.dcn_match_statistics_groups(*(rows_in + rows_out)), "dcn_match_statistics_groups")
    else:                                                   # (match_statistics_groups_wide)
        _lib.check(lib.dcn_match_statistics_groups_wide(*(rows_in + (int(_strip_pixels),) + rows_out)),
                   "dcn_match_statistics_groups_wide")
    return _eval_table_of(outs, R, off, u_a, v_a, u_b, v_b)


def match_statistics_groups_wide(res_b, mask_b, depth_b, queries, u_a, v_a, depth_q, u_b, v_b, cams, keep, offsets,
                                 max_group_rows=None, strip_pixels=0):
    """``match_statistics_groups`` -- its arguments, its EvalTable, its bits -- by the row-per-lane kernel
    (``dcn_match_statistics_groups_wide``), made for groups of MANY rows: a workgroup takes up to 256 rows of one group and a
    strip of ``strip_pixels`` pixels of its image (0: chosen by the library so that the grid fills the device) and every
    work-item keeps one row's running keys, counts and sums while the strip's pixels pass by, with no reduction across
    lanes.  Every accumulation is an integer one (packed-key minima, counts, distance sums in units of 2^-20 pixel), so the
    result does not depend on ``strip_pixels`` and equals match_statistics_groups' bit for bit.  No host synchronization."""
    if int(strip_pixels) < 0:
        raise ValueError("strip_pixels must be >= 0 (0 = automatic), got %d" % int(strip_pixels))
    return match_statistics_groups(res_b, mask_b, depth_b, queries, u_a, v_a, depth_q, u_b, v_b, cams, keep, offsets,
                                   max_group_rows, _strip_pixels=int(strip_pixels))


def _cross_scene_views(labels, views):
    v = np.asarray(views.cpu() if torch.is_tensor(views) else views)
    if v.ndim != 2 or v.shape[1] != 5 or not np.issubdtype(v.dtype, np.integer):
        raise ValueError("views must be choose_cross_scene_views' integer table [T, 5], got %s" % (v.shape,))
    v = v.astype(np.int64)
    if v.shape[0] and (v[:, 0].min() < 0 or v[:, 0].max() >= labels.pairs.shape[0] or v[:, 1].min() < 0
                       or v[:, 1].max() >= labels.pixels.shape[0] or v[:, 2].min() < LABELLED or v[:, 2].max() > VIEW_OF_B):
        raise ValueError("views name a pair, a label or a kind outside the labels")
    return v


def _search_rows_by_frame(dcn, store, out, word, fb, kept, pair, queries, depth_q, cams, keep, batch_frames, max_search_bytes,
                          mean, std, statistics, resident=None):
    """The search of evaluate_cross_scene_rows and evaluate_keypoint_rows: the rows ``kept`` (host indices into the T rows of
    the nan-filled EvalTable ``out``, whose u_a .. v_b are the rows' pixels) sorted by the frame ``fb`` they search, one group
    per frame; the searched frames in chunks whose descriptor images stay within ``max_search_bytes`` -- forwarded through
    ``dcn``, or taken from ``resident`` = (sorted frames, their descriptor images) -- and one ``statistics`` call
    (match_statistics_groups or its wide twin) per chunk, whose rows go back to their places in ``out``; ``row_pair`` becomes
    ``pair`` of the row and ``mask_pixels`` the mask pixels of the image it searched.  -> the status word, joined to ``word``"""
    dev, h, w, d = store.device, store.h, store.w, int(queries.shape[1])
    up = _uploader(dev)
    b_frames, b_group = np.unique(fb[kept], return_inverse=True)
    by_group = np.argsort(b_group, kind="stable")
    order = up(kept[by_group])                                # table rows in search order
    g_off = np.searchsorted(b_group[by_group], np.arange(len(b_frames) + 1)).astype(np.int64)
    g_off_dev = up(g_off)
    per_chunk = min(1024, max(1, int(max_search_bytes) // (h * w * d * 4)))      # (images per statistics call)
    mask_pixels = out.mask_pixels
    for g0 in range(0, len(b_frames), per_chunk):
        g1 = min(g0 + per_chunk, len(b_frames))
        if resident is None:
            rgb, depth_b, mask_b, bad = _gather_frame_list(store, b_frames[g0:g1], ("rgb", "depth", "mask"))
            res = []
            _forward_in_eval_mode(dcn, rgb, mask_b, None, None, int(batch_frames), mean, std, lambda lo, n, y: res.append(y))
            res_b = (res[0] if len(res) == 1 else torch.cat(res)).float().contiguous()
            del rgb, res
        else:
            _, depth_b, mask_b, bad = _gather_frame_list(store, b_frames[g0:g1], ("depth", "mask"))
            at = np.searchsorted(resident[0], b_frames[g0:g1])
            res_b = resident[1][int(at[0]):int(at[-1]) + 1] if int(at[-1]) - int(at[0]) + 1 == len(at) else resident[1][up(at)]
        word = word | (bad & 1) * BAD_FRAME
        rows = order[g_off[g0]:g_off[g1]]
        t = statistics(res_b, mask_b, depth_b, queries[rows], out.u_a[rows], out.v_a[rows], depth_q[rows], out.u_b[rows],
                       out.v_b[rows], cams[rows], keep[rows], g_off_dev[g0:g1 + 1] - int(g_off[g0]),
                       max_group_rows=int(np.diff(g_off[g0:g1 + 1]).max()))
        del res_b
        out.columns[:, rows], out.is_valid[:, rows], out.pred_uv[:, rows], out.closer[:, rows] = (t.columns, t.is_valid,
                                                                                                   t.pred_uv, t.closer)
        has = t.row_pair >= 0
        out.row_pair[rows] = torch.where(has, up(pair[kept[by_group][g_off[g0]:g_off[g1]]].astype(np.int32)), t.row_pair)
        mask_pixels[rows] = torch.where(has, t.mask_pixels[t.row_pair.clamp_min(0).long()], torch.zeros_like(t.row_pair))
        word = word | t.status
    return word


def evaluate_cross_scene_rows(dcn, store, labels, views, *, batch_frames=16, max_search_bytes=2 << 30,
                              mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV):
    """single_cross_scene_image_pair_quantitative_analysis (evaluation.py:610-781) for every row of ``views``
    (choose_cross_scene_views' table over ``labels``) on the device, nothing read back:
    1. reproject_pixels for every view: the labelled pixel of image a into an a-view, that of image b into a b-view (default
    K, as the reference); a view into which it does not project has no row, like "no view"; 2. ``dcn.forward_image_tensors`` in
    eval mode ONCE per distinct a-side frame, ``batch_frames`` at a time, keeping after each batch only the rows' query
    descriptors; 3. the rows sorted by the frame they search (a b-view drawn twice is one group), those frames forwarded in
    chunks whose descriptor images stay within ``max_search_bytes``, one match_statistics_groups call per chunk with camera
    rows from ``dcn_gather_frames`` over (a-side frame, b-side frame): K of the a-side scene, pose a, pose b^-1; 4. the tables
    concatenated and put back into the order of ``views``.  Views whose reprojection fails are still forwarded: leaving them
    out would need a read-back.

    -> EvalTable with one row per row of ``views``, rows without a result as past-the-end rows (NaN, -1): ``row_pair`` the
    row's annotated pair (row of ``labels.pairs``) or -1; ``offsets`` int64 [N + 1], the pairs' row ranges; ``mask_pixels``
    int32 [T], PER ROW: the mask pixels of the image the row searched (0 without a result); u_a, v_a the query pixel and u_b,
    v_b the ground truth as given to the statistics; ``status`` covers the chain: the statistics' bits and BAD_FRAME for the
    gathers and the reprojection.  ``dcn.training`` is left as found."""
    v = _cross_scene_views(labels, views)
    if int(batch_frames) < 1 or int(max_search_bytes) < 1:
        raise ValueError("batch_frames and max_search_bytes must be >= 1")
    T, dev, h, w = int(v.shape[0]), store.device, store.h, store.w
    pair, lab, kind, fa, fb = (v[:, i] for i in range(5))
    if T and (max(fa.max(), fb.max()) >= store.num_frames or min(fa.min(), fb.min()) < -1):
        raise ValueError("views name a frame outside the store's %d frames" % store.num_frames)
    up = _uploader(dev)
    px = labels.pixels
    host_keep = (fa >= 0) & (fb >= 0)
    u_a, v_a = up(px[lab, 1]), up(px[lab, 2])
    u_b, v_b = up(px[lab, 3].astype(np.float32)), up(px[lab, 4].astype(np.float32))
    keep = up(host_keep.astype(np.uint8))
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    # 1. the labelled pixel of the side that was replaced, into its view
    for k, col, frame, view in ((VIEW_OF_A, 1, 2, fa), (VIEW_OF_B, 3, 4, fb)):
        rows = np.nonzero((kind == k) & host_keep)[0]
        if len(rows) == 0:
            continue
        rp = reproject_pixels(store, np.stack([labels.pairs[pair[rows], frame], px[lab[rows], col], px[lab[rows], col + 1],
                                               view[rows]], axis=1))
        at = up(rows)
        if k == VIEW_OF_A:                                    # the view's pixel is the query
            u_a[at], v_a[at] = rp.uv[0].long().clamp_min(0), rp.uv[1].long().clamp_min(0)
        else:                                                 # ... the ground truth, as the search returns it
            u_b[at], v_b[at] = rp.u, rp.v
        keep[at] = rp.found
        word = word | rp.status
    offsets = up(np.searchsorted(pair, np.arange(labels.pairs.shape[0] + 1)).astype(np.int64))
    kept = np.nonzero(host_keep)[0]
    if len(kept) == 0:
        return _nan_table(T, offsets, word, u_a, v_a, u_b, v_b, dev)
    # 2. the query descriptors: one forward pass per distinct a-side frame
    a_frames, a_slot = np.unique(fa[kept], return_inverse=True)
    queries, _, bad = _queries_of_frames(dcn, store, a_frames, a_slot, kept, u_a, v_a, T, batch_frames, mean, std)
    word = word | bad
    depth_q = store.depth[up(np.where(host_keep, fa, 0)), v_a, u_a]
    # camera rows per row (frames of rows without both reach the gather as frame 0: the row is left out anyway)
    cams, bad = _camera_rows_of(store, v[:, 3:5], host_keep)
    word = word | bad
    # 3. the rows by the frame they search, the searched frames in chunks; 4. back into the order of ``views``
    out = _nan_table(T, offsets, word, u_a, v_a, u_b, v_b, dev)
    word = _search_rows_by_frame(dcn, store, out, word, fb, kept, pair, queries, depth_q, cams, keep, int(batch_frames),
                                 int(max_search_bytes), mean, std, match_statistics_groups)
    return out._replace(status=word.to(torch.int32))


def cross_scene_table(store, labels, views, t):
    """evaluate_cross_scene_rows' EvalTable ``t`` (over ``views``) as the reference's table, with ONE copy to the host: a dict
    of numpy columns under the reference's column names (COLUMNS as float64, ``is_valid`` / ``is_valid_masked`` as bool) plus
    ``scene_name`` = "<scene a>+<scene b>" and ``img_a_idx`` / ``img_b_idx``, the dataset's image indices of the two images
    actually compared (the view's index on the side that was replaced); the rows without a result are dropped, the others
    keep the reference's order.  RuntimeError when the chain's status word is not zero."""
    views = _cross_scene_views(labels, views)
    block, rows, word = _table_block([t.columns, t.is_valid.double()], t.row_pair, t.status)
    if word:
        raise RuntimeError("dcn_hip: the cross-scene evaluation failed on the device (status %d)" % word)
    table = _columns_to_dict(block)
    pairs = labels.pairs[views[rows, 0]]
    table["scene_name"] = np.array([store.scene_names[a] + "+" + store.scene_names[b] for a, b in pairs[:, [1, 3]]],
                                   dtype=object)
    for key, col in (("img_a_idx", 3), ("img_b_idx", 4)):
        table[key] = _image_index(store, views[rows, col])[1]
    return table


def evaluate_network_cross_scene(dcn, store, annotated_pairs, num_views_a=10, num_views_b=10, host_rng=None):
    """``DenseCorrespondenceEvaluation.evaluate_network_cross_scene`` (evaluation.py:253-301) on a frame store:
    cross_scene_labels, choose_cross_scene_views, evaluate_cross_scene_rows, then cross_scene_table's ONE copy to the host.
    -> (table, dataframe) like ``evaluate_network``: ``table`` as cross_scene_table returns it; ``dataframe`` a
    ``pandas.DataFrame`` of it when pandas imports, else None.  Views that do not exist or into which the labelled pixel does
    not project contribute no rows; no usable annotated pair gives an empty table.  ``dcn.training`` is left as found."""
    labels = cross_scene_labels(store, annotated_pairs)
    views = choose_cross_scene_views(store, labels, num_views_a, num_views_b, host_rng)
    names = COLUMNS + ("is_valid", "is_valid_masked", "scene_name", "img_a_idx", "img_b_idx")
    if views.shape[0] == 0:
        table = _empty_table(names)
    else:
        table = cross_scene_table(store, labels, views, evaluate_cross_scene_rows(dcn, store, labels, views))
    return table, _dataframe(table, names)


def evaluate_network_cross_instance(dcn, store, labelled_images, num_views_a=10, num_views_b=10, host_rng=None):
    """``DenseCorrespondenceEvaluation.evaluate_network_cross_instance`` (evaluation.py:350-404) on a frame store:
    ``labelled_images`` is the reference's list of dicts {"image": {scene_name, image_idx, pixels: [{u, v}, ...]}} (or a path to
    its YAML); every ``itertools.combinations(labelled_images, 2)`` becomes an annotated pair (image_a, image_b) in that order
    and the list goes to ``evaluate_network_cross_scene``.  -> (table, dataframe) as it returns them."""
    import itertools
    if isinstance(labelled_images, str):
        labelled_images = _yaml_file(labelled_images)
    pairs = [{"image_a": a["image"], "image_b": b["image"]} for a, b in itertools.combinations(labelled_images, 2)]
    return evaluate_network_cross_scene(dcn, store, pairs, num_views_a, num_views_b, host_rng)
