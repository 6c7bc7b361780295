"""The same-scene table (csrc/evaluate_kernels.hip, the matches-only entry of csrc/sample_kernels.hip): ``evaluate_network``
(evaluation.py:475-527) and what it calls per image pair."""
import collections

import numpy as np
import torch

from .. import _args, _lib
from .. import augment as _aug
from ..samples import random_source
from ._chain import (BAD_DRAWS, BAD_FRAME, COLUMNS, _alloc_eval_table, _below, _columns_to_dict, _dataframe,
                     _descriptor_dimension, _empty_table, _eval_table_of, _forward_pairs, _frame_pairs, _image_index, _lots,
                     _offsets_arg, _random_scene, _rows, _table_block, _valid_pointers)

NUM_ATTEMPTS = 20          # batch_find_pixel_correspondences' default num_attempts, which the evaluation uses (:908)


def match_statistics_pairs(res_a, res_b, mask_b, depth_a, depth_b, cams, u_a, v_a, u_b, v_b, offsets, max_pair_rows=None):
    """Every column of the reference's evaluation table for the query rows of P image pairs, in two launches.

    res_a, res_b: float32 [P, H, W, D] descriptor images; mask_b: [P, H, W] (non-zero = on the object); depth_a, depth_b: 16-bit
    [P, H, W] millimetres; cams: float32 [P, 50] camera rows (K, K^-1, pose a, pose b^-1; frames.FrameBatch.cams[0]); u_a, v_a:
    int64 [R] query pixels in image a; u_b, v_b: float32 [R] ground truth in image b as the correspondence search returns it
    (rounded and clipped like the reference); offsets: int64 [P + 1] device tensor, pair p's rows at offsets[p]:offsets[p+1]
    (rows from offsets[P] on are ignored).  max_pair_rows: a bound on one pair's rows (default R).
    -> EvalTable.  No host synchronization."""
    lib = _lib.get()
    if res_a.dim() != 4 or res_a.shape != res_b.shape:
        raise ValueError("res_a and res_b must be [P, H, W, D] of one shape, got %s and %s" % (tuple(res_a.shape),
                                                                                          tuple(res_b.shape)))
    P, h, w, d = (int(s) for s in res_a.shape)
    _descriptor_dimension(d)
    ra, rb = res_a.contiguous().float(), res_b.contiguous().float()
    mb = _args.mask(mask_b, P, h, w, "mask_b")
    da, db = _args.depth(depth_a, P, h, w, "depth_a"), _args.depth(depth_b, P, h, w, "depth_b")
    cams = _args.camera_rows(cams, P, "cams")
    ua = _rows(u_a, torch.int64, "u_a")
    R = int(ua.numel())
    va, ub, vb = _rows(v_a, torch.int64, "v_a", R), _rows(u_b, torch.float32, "u_b", R), _rows(v_b, torch.float32, "v_b", R)
    off = _offsets_arg(offsets, P, "P")
    _lib.require_device(ra, rb, mb, da, db, cams, ua, va, ub, vb, off)
    cap = max(R, 1)
    ua, va, ub, vb = _valid_pointers(R, ua, va, ub, vb)
    mpr = cap if max_pair_rows is None else max(1, min(int(max_pair_rows), cap))
    outs = _alloc_eval_table(cap, P, ra.device, lib.dcn_match_statistics_pairs_workspace(cap))
    p = _lib.ptr
    rc = lib.dcn_match_statistics_pairs(P, h, w, d, p(ra), p(rb), p(mb), p(da), p(db), p(cams), p(ua), p(va), p(ub), p(vb),
                                        p(off), cap, mpr, *([p(t) for t in outs] + [_lib.stream_ptr()]))
    _lib.check(rc, "dcn_match_statistics_pairs")
    return _eval_table_of(outs, R, off, u_a, v_a, u_b, v_b)


EvalMatches = collections.namedtuple("EvalMatches", "u_a v_a u_b v_b offsets totals status order_seeds")


def find_eval_matches(depth_a, depth_b, mask_a, cams, num_matches=100, *, num_attempts=NUM_ATTEMPTS, generator=None,
                      draws=None, seeds=None, match_order=None, order_seeds=None):
    """The ground-truth matches the evaluation uses, per pair: ``batch_find_pixel_correspondences(depth_a, pose_a, depth_b,
    pose_b, img_a_mask=mask_a)`` with ``num_attempts`` candidates from mask a's pixels (the search of
    samples.build_within_scene_samples, without non-matches or rotation), then ``random.sample(range(total), min(num_matches,
    total))`` (evaluation.py:919-921) on the device.

    depth_a, depth_b: 16-bit [P, H, W]; mask_a: [P, H, W]; cams: float32 [P, 50].  ``draws``: {"cand": per-pair torch.rand
    streams} to replay (samples.pack_draws), otherwise per-pair ``seeds`` (drawn with ``generator`` when None).
    ``match_order``: int [P, num_matches], -1 padded, the reference's ``match_list`` per pair to replay; otherwise the order
    comes from ``order_seeds`` (int64 [P], drawn with ``generator`` when None).
    -> EvalMatches: u_a, v_a int64 and u_b, v_b float32 [P * min(num_matches, num_attempts)], pair p's rows at
    offsets[p]:offsets[p+1] in ``match_list`` order (a pair without matches has none; -1 / 0 after offsets[P]); totals int32
    [P] (matches found before the subsample); status int32 [1] (samples.BAD_DRAWS).  No host synchronization."""
    lib = _lib.get()
    n, h, w = int(mask_a.shape[0]), int(mask_a.shape[1]), int(mask_a.shape[2])
    dev = mask_a.device
    da, db = _args.depth(depth_a, n, h, w, "depth_a"), _args.depth(depth_b, n, h, w, "depth_b")
    ma = _args.mask(mask_a, n, h, w, "mask_a")
    A, M = int(num_attempts), int(num_matches)
    if A < 1 or A > 4096 or M < 1 or n > 1024:
        raise ValueError("num_attempts must be 1 .. 4096, num_matches >= 1 and at most 1024 pairs per call")
    cams = _args.camera_rows(cams, n, "cams")
    sd, rand, roff = random_source(n, dev, generator, draws, seeds)
    order = None if match_order is None else _args.replay_table(match_order, (n, M), "match_order", dev)
    osd = None if match_order is not None else _args.seeds_for(n, dev, generator, order_seeds, "order_seeds")
    _lib.require_device(da, db, ma, cams, sd, rand, roff, order, osd)
    cap = n * min(M, A)
    ua, va = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    ub, vb = torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.float32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.dcn_eval_matches_workspace(n, h, w, A)), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_eval_matches(n, h, w, p(da), p(db), p(ma), p(cams), A, p(sd), p(rand), p(roff), M, p(order), p(osd), p(ua),
                              p(va), p(ub), p(vb), p(offsets), p(totals), p(status), p(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_eval_matches")
    return EvalMatches(ua, va, ub, vb, offsets, totals, status, osd)


def choose_pairs(store, num_image_pairs, host_rng=None, threshold=0.05, max_num_attempts=100):
    """``num_image_pairs`` times the reference's per-pair rule, on the host: a scene by ``get_random_scene_name``
    (spartan_dataset_masked.py:521-541: one lot per multi-object scene and per object; then uniform over the multi-object
    scenes, or a uniform object and a uniform scene of it), image a uniform over the scene's frames, image b the first of up
    to ``max_num_attempts`` uniform frames whose translation differs from a's by more than ``threshold`` (float64 norm,
    ``get_image_pair_with_poses_diff_above_threshold``, evaluation.py:175-203); a pair for which none does is skipped, as
    ``evaluate_network`` skips ``None``.  Reads ``store.translations_host``; ``host_rng``: a numpy RandomState / Generator
    (default ``np.random``).

    All pairs are drawn up front.  The reference interleaves these draws with the data-dependent ``random.sample`` of every
    pair's matches, so its random STREAM is deliberately not replayed: only the rule is.

    -> int64 array [n, 3] of (scene, frame a, frame b), frames as store indices; n <= num_image_pairs."""
    rng = host_rng if host_rng is not None else np.random
    first = store.scene_first_frame_host
    lots = _lots(store)
    t = store.translations_host
    out = []
    for _ in range(int(num_image_pairs)):
        s = _random_scene(store, rng, lots)
        lo, cnt = first[s], first[s + 1] - first[s]
        a = lo + _below(rng, cnt)
        for _attempt in range(int(max_num_attempts)):
            b = lo + _below(rng, cnt)
            if np.linalg.norm(t[a] - t[b]) > threshold:
                out.append((s, a, b))
                break
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def evaluate_frame_pairs(dcn, store, pairs, num_matches=100, *, generator=None, draws=None, match_order=None, batch_pairs=8,
                         mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV):
    """The reference's per-pair evaluation for ``pairs`` ([P, 2] store frame indices (a, b), or choose_pairs' [P, 3]; P <=
    1024) on the device: 1. ``dcn_gather_frames`` of the chosen frames, 2. ToTensor + Normalize by the augmentation kernel with
    every augmentation switched off (``mean`` / ``std``: the dataset's, as ``rgb_image_to_tensor``), 3. ``dcn.forward_image_tensors`` in eval mode, ``batch_pairs`` pairs (2 x ``batch_pairs``
    images) at a time, 4. find_eval_matches (``draws`` / ``match_order`` replay, otherwise ``generator``), 5.
    match_statistics_pairs.  -> EvalTable, its ``status`` covering the whole chain.  The pair list is given on the host; nothing is read back.  ``dcn.training`` is
    left as found."""
    res_a, res_b, depth, mask, cams, status = _forward_pairs(dcn, store, _frame_pairs(store, pairs),
                                                             ("rgb", "depth", "mask", "cams"), batch_pairs, mean, std)
    m = find_eval_matches(depth[0], depth[1], mask[0], cams[0], num_matches, generator=generator, draws=draws,
                          match_order=match_order)
    t = match_statistics_pairs(res_a, res_b, mask[1], depth[0], depth[1], cams[0], m.u_a, m.v_a, m.u_b, m.v_b, m.offsets,
                               max_pair_rows=min(int(num_matches), NUM_ATTEMPTS))
    # one status word for the chain (on the device): the search's BAD_DRAWS bit and the gather's BAD_INDEX bit join the table's
    word = t.status | ((m.status >> 1) & 1) * BAD_DRAWS | (status & 1) * BAD_FRAME
    return t._replace(status=word.to(torch.int32))


def evaluate_network(dcn, store, num_image_pairs=25, num_matches_per_image_pair=100, host_rng=None, generator=None):
    """``DenseCorrespondenceEvaluation.evaluate_network`` (evaluation.py:475-527) on a frame store: choose_pairs, then
    evaluate_frame_pairs, then ONE copy to the host.  -> (table, dataframe): ``table`` a dict of numpy columns under the
    reference's column names (COLUMNS as float64, ``is_valid`` / ``is_valid_masked`` as bool) plus ``scene_name``,
    ``img_a_idx``, ``img_b_idx`` per row; ``dataframe`` a ``pandas.DataFrame`` of it when pandas imports, else None.  Pairs
    without matches contribute no rows, as in the reference.  ``dcn.training`` is left as found."""
    chosen = choose_pairs(store, num_image_pairs, host_rng)
    names = COLUMNS + ("is_valid", "is_valid_masked", "scene_name", "img_a_idx", "img_b_idx")
    if chosen.shape[0] == 0:
        table = _empty_table(names)
    else:
        t = evaluate_frame_pairs(dcn, store, chosen, num_matches_per_image_pair, generator=generator)
        block, _, _ = _table_block([t.columns, t.is_valid.double()], t.row_pair)      # (the status word is not looked at)
        table = _columns_to_dict(block)
        pair = block[-1].astype(np.int64)
        table["scene_name"], table["img_a_idx"] = _image_index(store, chosen[pair, 1])
        table["img_b_idx"] = _image_index(store, chosen[pair, 2])[1]
    return table, _dataframe(table, names)
