"""Host side of the evaluation kernels (csrc/evaluate_kernels.hip, the matches-only entry of csrc/sample_kernels.hip): the
reference's quantitative evaluation, ``DenseCorrespondenceEvaluation.evaluate_network``
(dense_correspondence/evaluation/evaluation.py:475-527) and what it calls per image pair
(single_same_scene_image_pair_quantitative_analysis :862-958, compute_descriptor_match_statistics :1007-1178), on the frames
of a ``frames.FrameStore``.

``choose_pairs`` draws the image pairs on the host (a few integers per pair).  ``evaluate_frame_pairs`` then gathers the
frames, normalizes them, runs the network in eval mode, finds and subsamples the ground-truth matches and computes every
column of the reference's table for all pairs, without reading anything back; ``evaluate_network`` composes the two and
copies the table to the host once.

``compute_descriptor_statistics_on_dataset`` (csrc/descstats_kernels.hip) is the first quantitative part of the reference's
``run_evaluation_on_network`` (evaluation.py:2157-2304): the per-channel min, max and mean of the descriptors over random
frames of the store, for the whole image and for the object mask, written to ``descriptor_statistics.yaml``.

``evaluate_network`` above, called on the train and on the test store, is the second part.

``evaluate_network_cross_scene`` (csrc/crossscene_kernels.hip) is the third, ``evaluate_network_cross_scene``
(evaluation.py:253-301, single_cross_scene_image_pair_quantitative_analysis :610-781): the only table built from human-labelled
matches between DIFFERENT scenes.  ``cross_scene_labels`` resolves the annotated pairs to store frames,
``choose_cross_scene_views`` draws the other views of either scene on the host, and ``evaluate_cross_scene_rows`` reprojects the
labelled pixels into them (``reproject_pixels``), runs the network once per distinct frame and computes the table's rows with
every searched image read once (``match_statistics_groups``).

``evaluate_network_cross_instance`` feeds the same chain with every combination of two pixel-labelled images.

``evaluate_network_cross_scene_keypoints`` is the class-consistent keypoint table (evaluation.py:407-472, single_image_pair_
cross_scene_keypoints_quantitative_analysis :1433-1552): named keypoints on different object instances, every combination of two
labelled images, both orders (``keypoint_labels``, ``keypoint_rows``, ``evaluate_keypoint_rows``, ``keypoint_table``).  A labelled
image is searched by (images - 1) * keypoints rows there, which is what ``match_statistics_groups_wide`` (the row-per-lane
kernel of csrc/crossscene_kernels.hip) is for.

``evaluate_network_across_objects`` (csrc/acrossobj_kernels.hip) is its fourth part, ``evaluate_network_across_objects``
(evaluation.py:305-337): pairs of frames of two different objects (``choose_object_pairs``), pixels sampled from mask a and
their best matches over the whole of image b (``evaluate_object_pairs``: ``across_object_queries`` + ``best_match_pairs``).
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _args, _lib
from . import augment as _aug
from .frames import gather_frames
from .samples import random_source

COLUMNS = ("norm_diff_descriptor_ground_truth", "norm_diff_descriptor", "norm_diff_descriptor_masked",
           "norm_diff_ground_truth_3d", "norm_diff_pred_3d", "norm_diff_pred_3d_masked", "pixel_match_error_l2",
           "pixel_match_error_l2_masked", "pixel_match_error_l1", "fraction_pixels_closer_than_ground_truth",
           "fraction_pixels_closer_than_ground_truth_masked", "average_l2_distance_for_false_positives",
           "average_l2_distance_for_false_positives_masked")
BAD_INDEX, BAD_OFFSETS, BAD_DRAWS, BAD_FRAME, TOO_FEW_MASK_PIXELS = 1, 2, 4, 8, 16
ACROSS_OBJECT_COLUMNS = ("scene_name_a", "scene_name_b", "img_a_idx", "img_b_idx", "object_id_a", "object_id_b",
                         "norm_diff_descriptor_best_match")   # DCNEvaluationPandaTemplateAcrossObject.columns
NUM_ATTEMPTS = 20          # batch_find_pixel_correspondences' default num_attempts, which the evaluation uses (:908)


class EvalTable(collections.namedtuple(
        "EvalTable", "columns is_valid pred_uv closer row_pair offsets mask_pixels status u_a v_a u_b v_b")):
    """Device tensors, R = the row capacity; the rows in use are [0, offsets[-1]), pair p's at offsets[p]:offsets[p+1].
    columns float64 [13, R] in the order of COLUMNS (NaN past the last row); is_valid uint8 [2, R] (is_valid,
    is_valid_masked); pred_uv int32 [4, R] (u, v of the best match over the image, u, v over the mask; -1 past the last row);
    closer int32 [2, R] (pixels closer than the ground truth: image, masked); row_pair int32 [R] (the row's pair, -1 past the
    last row); offsets int64 [P + 1]; mask_pixels int32 [P]; status int32 [1] (BAD_INDEX | BAD_OFFSETS from the statistics; evaluate_frame_pairs adds
    BAD_DRAWS for a replay stream or ``match_order`` the match search rejected and BAD_FRAME for a frame the gather rejected); u_a, v_a int64 [R]
    and u_b, v_b float32 [R]: the query rows."""

    def column(self, name):
        return self.columns[COLUMNS.index(name)]


def _rows(t, dtype, what, count=None):
    if t.dtype != dtype or t.dim() != 1 or (count is not None and int(t.numel()) != count):
        raise ValueError("%s must be a 1-D %s tensor%s, got %s %s" % (what, dtype, "" if count is None else " of %d" % count,
                                                                     t.dtype, tuple(t.shape)))
    return t.contiguous()


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
    if d < 1 or d > 64:
        raise ValueError("descriptor dimension must be 1 .. 64, got %d" % d)
    ra, rb = res_a.contiguous().float(), res_b.contiguous().float()
    mb = _args.mask(mask_b, P, h, w, "mask_b")
    da, db = _args.depth(depth_a, P, h, w, "depth_a"), _args.depth(depth_b, P, h, w, "depth_b")
    cams = _args.camera_rows(cams, P, "cams")
    ua = _rows(u_a, torch.int64, "u_a")
    R = int(ua.numel())
    va, ub, vb = _rows(v_a, torch.int64, "v_a", R), _rows(u_b, torch.float32, "u_b", R), _rows(v_b, torch.float32, "v_b", R)
    if not torch.is_tensor(offsets) or offsets.dtype != torch.int64 or int(offsets.numel()) != P + 1:
        raise ValueError("offsets must be an int64 tensor of P + 1 = %d entries" % (P + 1))
    off = offsets.contiguous().view(-1)
    _lib.require_device(ra, rb, mb, da, db, cams, ua, va, ub, vb, off)
    dev = ra.device
    cap = max(R, 1)
    if R == 0:                                             # (no rows at all: the kernels still want valid pointers)
        ua = va = torch.zeros(1, dtype=torch.int64, device=dev)
        ub = vb = torch.zeros(1, dtype=torch.float32, device=dev)
    mpr = cap if max_pair_rows is None else max(1, min(int(max_pair_rows), cap))
    cols = torch.empty((len(COLUMNS), cap), dtype=torch.float64, device=dev)
    valid = torch.empty((2, cap), dtype=torch.uint8, device=dev)
    pred = torch.empty((4, cap), dtype=torch.int32, device=dev)
    closer = torch.empty((2, cap), dtype=torch.int32, device=dev)
    row_pair = torch.empty(cap, dtype=torch.int32, device=dev)
    mask_pixels = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.dcn_match_statistics_pairs_workspace(cap)), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_match_statistics_pairs(P, h, w, d, p(ra), p(rb), p(mb), p(da), p(db), p(cams), p(ua), p(va), p(ub), p(vb),
                                        p(off), cap, mpr, p(cols), p(valid), p(pred), p(closer), p(row_pair), p(mask_pixels),
                                        p(status), p(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_match_statistics_pairs")
    return EvalTable(cols[:, :R], valid[:, :R], pred[:, :R], closer[:, :R], row_pair[:R], off, mask_pixels, status,
                     u_a, v_a, u_b, v_b)


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


def _below(rng, n):
    return int(rng.integers(n)) if hasattr(rng, "integers") else int(rng.randint(n))


def _lots(store):
    lots = len(store.multi_scenes_host) + len(store.object_scenes_host)
    if lots == 0:
        raise ValueError("I don't think you have any scenes?")
    return lots


def _random_scene(store, rng, lots):
    """``get_random_scene_name`` (spartan_dataset_masked.py:521-541) on the store's host tables: two or three draws;
    ``lots`` = _lots(store)"""
    multi, per_object = store.multi_scenes_host, store.object_scenes_host
    k = _below(rng, lots)
    if k < len(multi):
        return multi[_below(rng, len(multi))]
    o = _below(rng, len(per_object))
    scenes = per_object[o]
    if not scenes:
        raise ValueError("object %s has no scene in this store" % (store.object_ids[o],))
    return scenes[_below(rng, len(scenes))]


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


def _frame_pairs(store, pairs):
    a = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs)
    if a.ndim != 2 or a.shape[1] not in (2, 3) or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("pairs must be an integer array [P, 2] of (frame a, frame b) or [P, 3] of (scene, frame a, frame b), "
                         "P >= 1")
    fr = a[:, -2:].astype(np.int64)
    if fr.min() < 0 or fr.max() >= store.num_frames:
        raise ValueError("pairs name a frame outside the store's %d frames" % store.num_frames)
    return fr


def _gather_host_frames(store, fr, want):
    """``gather_frames`` of a host table ``fr`` (int [P, 2] store frame indices: slots 0 and 1) -> (rgb, depth, mask, cams,
    status); status int32 [1], zero unless the gather rejected a frame index."""
    P, dev = int(fr.shape[0]), store.device
    frames = torch.from_numpy(np.concatenate([fr, np.full((P, 2), -1, np.int64)], axis=1).astype(np.int32))
    if torch.device(dev).type == "cuda":     # (a pageable copy would wait for the stream: the trainer validates without a wait)
        frames = frames.pin_memory()
    frames = frames.to(dev, non_blocking=True)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    return gather_frames(store, frames, None, status, 2, want) + (status,)


def _forward_in_eval_mode(dcn, rgb, mask, rgb_b, mask_b, step, mean, std, consume):
    """``dcn`` in eval mode over the frames of ``rgb`` (pairs of frames with ``rgb_b``), ``step`` at a time: ToTensor +
    Normalize by the augmentation kernel with every augmentation switched off (zero records), ``forward_image_tensors`` (a's
    images, then b's), ``consume(lo, n, descriptors)``.  ``dcn.training`` is left as found."""
    count, sides = int(rgb.shape[0]), 1 if rgb_b is None else 2
    params = torch.zeros((sides * min(step, count), _aug.PARAM_WORDS), dtype=torch.int32, device=rgb.device)
    was_training = dcn.training
    dcn.eval()
    try:
        for lo in range(0, count, step):
            n = min(step, count - lo)
            b = {} if rgb_b is None else dict(rgb_b=rgb_b[lo:lo + n], mask_b=mask_b[lo:lo + n])
            x = _aug.augment_images(rgb[lo:lo + n], mask[lo:lo + n], params[:sides * n], mean=mean, std=std, want_mask=False, **b)
            x = x["input_a"] if rgb_b is None else torch.cat([x["input_a"], x["input_b"]])
            consume(lo, n, dcn.forward_image_tensors(x))
    finally:
        dcn.train(was_training)


def evaluate_frame_pairs(dcn, store, pairs, num_matches=100, *, generator=None, draws=None, match_order=None, batch_pairs=8,
                         mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV):
    """The reference's per-pair evaluation for ``pairs`` ([P, 2] store frame indices (a, b), or choose_pairs' [P, 3]; P <=
    1024) on the device: 1. ``dcn_gather_frames`` of the chosen frames, 2. ToTensor + Normalize by the augmentation kernel with
    every augmentation switched off (``mean`` / ``std``: the dataset's, as ``rgb_image_to_tensor``), 3. ``dcn.forward_image_tensors`` in eval mode, ``batch_pairs`` pairs (2 x ``batch_pairs``
    images) at a time, 4. find_eval_matches (``draws`` / ``match_order`` replay, otherwise ``generator``), 5.
    match_statistics_pairs.  -> EvalTable, its ``status`` covering the whole chain.  The pair list is given on the host; nothing is read back.  ``dcn.training`` is
    left as found."""
    fr = _frame_pairs(store, pairs)
    P = int(fr.shape[0])
    if P > 1024:
        raise ValueError("at most 1024 pairs per call, got %d" % P)
    if int(batch_pairs) < 1:
        raise ValueError("batch_pairs must be >= 1")
    rgb, depth, mask, cams, status = _gather_host_frames(store, fr, ("rgb", "depth", "mask", "cams"))
    res = [[], []]

    def keep(lo, n, y):
        res[0].append(y[:n])
        res[1].append(y[n:])
    _forward_in_eval_mode(dcn, rgb[0], mask[0], rgb[1], mask[1], int(batch_pairs), mean, std, keep)
    res_a, res_b = torch.cat(res[0]).contiguous(), torch.cat(res[1]).contiguous()
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
        table = {k: np.zeros(0, np.float64) for k in COLUMNS}
        table.update(is_valid=np.zeros(0, bool), is_valid_masked=np.zeros(0, bool), scene_name=np.zeros(0, object),
                     img_a_idx=np.zeros(0, np.int64), img_b_idx=np.zeros(0, np.int64))
    else:
        t = evaluate_frame_pairs(dcn, store, chosen, num_matches_per_image_pair, generator=generator)
        R = int(t.row_pair.numel())
        # one transfer: everything packed into one float64 block (ints up to 2^31 are exact)
        block = torch.cat([t.columns, t.is_valid.double(), t.row_pair.double().view(1, R)]).cpu().numpy()
        block = block[:, :int(np.sum(block[-1] >= 0))]       # (rows past the last one carry pair -1)
        table = {k: block[i].copy() for i, k in enumerate(COLUMNS)}
        table["is_valid"] = block[len(COLUMNS)] != 0
        table["is_valid_masked"] = block[len(COLUMNS) + 1] != 0
        pair = block[len(COLUMNS) + 2].astype(np.int64)
        first = np.asarray(store.scene_first_frame_host, np.int64)
        scene = chosen[pair, 0]
        table["scene_name"] = np.array([store.scene_names[s] for s in scene], dtype=object)
        for key, col in (("img_a_idx", 1), ("img_b_idx", 2)):
            local = chosen[pair, col] - first[scene]
            table[key] = np.array([int(store.frame_ids[s][j]) for s, j in zip(scene, local)], dtype=np.int64)
    assert set(table) == set(names)
    try:
        import pandas
        df = pandas.DataFrame({k: table[k] for k in names})
    except ImportError:
        df = None
    return table, df


def choose_object_pairs(store, num_image_pairs, host_rng=None):
    """``num_image_pairs`` times the rule of ``evaluate_network_across_objects`` (evaluation.py:316-322), on the host: two
    different objects uniformly without replacement from the store's single-object classes (``get_two_different_object_ids``,
    spartan_dataset_masked.py:476-494), a uniform scene of each (:442-451) and a uniform frame of each scene (:408-420).  As in
    ``choose_pairs`` the rule is replayed, not the reference's random stream (it mixes numpy's and Python's generators, draws
    every frame twice and interleaves the per-pair ``random.sample``).  ``host_rng``: a numpy RandomState / Generator (default
    ``np.random``).

    -> int64 array [num_image_pairs, 6] of (object a, object b, scene a, scene b, frame a, frame b), frames as store indices."""
    rng = host_rng if host_rng is not None else np.random
    per_object = store.object_scenes_host
    if len(per_object) < 2:
        raise ValueError("There is only one object, can't sample a different one")
    first = store.scene_first_frame_host
    out = []
    for _ in range(int(num_image_pairs)):
        oa = _below(rng, len(per_object))
        ob = _below(rng, len(per_object) - 1)
        ob += 1 if ob >= oa else 0                           # (uniform over the ordered pairs of different objects)
        row = [oa, ob]
        for o in (oa, ob):
            if not per_object[o]:
                raise ValueError("object %s has no scene in this store" % (store.object_ids[o],))
            row.append(per_object[o][_below(rng, len(per_object[o]))])
        row.extend(first[s] + _below(rng, first[s + 1] - first[s]) for s in row[2:4])
        out.append(row)
    return np.asarray(out, dtype=np.int64).reshape(-1, 6)


AcrossQueries = collections.namedtuple("AcrossQueries", "u_a v_a queries offsets mask_pixels status order_seeds")


def _descriptor_images(res, what):
    if not torch.is_tensor(res) or res.dim() != 4:
        raise ValueError("%s must be a [P, H, W, D] tensor" % what)
    if res.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (what, res.dtype))
    P, h, w, d = (int(x) for x in res.shape)
    if d < 1 or d > 64:
        raise ValueError("descriptor dimension must be 1 .. 64, got %d" % d)
    if P < 1 or P > 1024 or h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError("%s must hold 1 .. 1024 images of 1 <= H * W < 2^31 pixels, got %s" % (what, tuple(res.shape)))
    return res.contiguous(), P, h, w, d


def _on_device(*tensors):
    try:
        _lib.require_device(*tensors)
    except RuntimeError as e:
        raise ValueError(str(e))


def across_object_queries(mask_a, res_a, num_samples=100, *, generator=None, sample_order=None, order_seeds=None):
    """``random_sample_from_masked_image(mask_a, num_samples)`` (correspondence_finder.py:68-90) for P pairs on the device,
    with the descriptors of the sampled pixels.

    mask_a: uint8 or bool [P, H, W] (non-zero = on the object); res_a: float32 [P, H, W, D].  ``sample_order``: int [P,
    num_samples], the reference's ``rand_inds`` per pair to replay (ranks among the mask's non-zero pixels in row-major
    order); otherwise the ranks come from ``order_seeds`` (int64 [P], drawn with ``generator`` when None).
    -> AcrossQueries: u_a, v_a int64 [P * num_samples] and queries float32 [P * num_samples, D], pair p's rows at
    offsets[p]:offsets[p+1] (num_samples rows, or none for a mask with fewer pixels; -1 / 0 after offsets[P]); mask_pixels
    int32 [P]; status int32 [1] (TOO_FEW_MASK_PIXELS for a mask with 1 .. num_samples - 1 pixels, BAD_DRAWS for a replay rank
    outside the mask's pixels or repeated).  No host synchronization."""
    lib = _lib.get()
    ra, P, h, w, d = _descriptor_images(res_a, "res_a")
    if not torch.is_tensor(mask_a) or mask_a.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mask_a must be a uint8 (or bool) tensor")
    ma = _args.mask(mask_a, P, h, w, "mask_a")
    Q = int(num_samples)
    if Q < 1 or Q > 1024:
        raise ValueError("num_samples must be 1 .. 1024, got %d" % Q)
    dev = ra.device
    order = None if sample_order is None else _args.replay_table(sample_order, (P, Q), "sample_order", dev)
    osd = None if sample_order is not None else _args.seeds_for(P, dev, generator, order_seeds, "order_seeds")
    _on_device(ra, ma, order, osd)
    ua, va = torch.empty(P * Q, dtype=torch.int64, device=dev), torch.empty(P * Q, dtype=torch.int64, device=dev)
    queries = torch.empty((P * Q, d), dtype=torch.float32, device=dev)
    offsets = torch.empty(P + 1, dtype=torch.int64, device=dev)
    mask_pixels = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, int(lib.dcn_across_object_queries_workspace(P, h, w))), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_across_object_queries(P, h, w, d, p(ma), p(ra), Q, p(order), p(osd), p(ua), p(va), p(queries), p(offsets),
                                       p(mask_pixels), p(status), p(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_across_object_queries")
    return AcrossQueries(ua, va, queries, offsets, mask_pixels, status, osd)


BestMatches = collections.namedtuple("BestMatches", "norm_diff_descriptor_best_match best_uv row_pair status")


def best_match_pairs(res_b, queries, offsets, max_pair_rows=None):
    """``DenseCorrespondenceNetwork.find_best_match`` (dense_correspondence_network.py:488-550, no mask) for the query rows of
    P pairs in one pass over ``res_b``.

    res_b: float32 [P, H, W, D]; queries: float32 [R, D]; offsets: int64 [P + 1] device tensor, pair p's rows at
    offsets[p]:offsets[p+1] (rows from offsets[P] on are ignored).  max_pair_rows: a bound on one pair's rows (default and
    at most 1024).
    -> BestMatches: norm_diff_descriptor_best_match float32 [R]; best_uv int32 [2, R] (u, v of the first minimum in row-major
    order); row_pair int32 [R]; NaN / -1 / -1 from offsets[P] on; status int32 [1] (BAD_OFFSETS).  Bit-identical from run to
    run.  No host synchronization."""
    lib = _lib.get()
    rb, P, h, w, d = _descriptor_images(res_b, "res_b")
    if not torch.is_tensor(queries) or queries.dtype != torch.float32 or queries.dim() != 2 or int(queries.shape[1]) != d:
        raise ValueError("queries must be float32 [R, %d]" % d)
    if not torch.is_tensor(offsets) or offsets.dtype != torch.int64 or int(offsets.numel()) != P + 1:
        raise ValueError("offsets must be an int64 tensor of P + 1 = %d entries" % (P + 1))
    q, off = queries.contiguous(), offsets.contiguous().view(-1)
    _on_device(rb, q, off)
    dev = rb.device
    R = int(q.shape[0])
    cap = max(R, 1)
    if R == 0:                                             # (no rows at all: the kernels still want a valid pointer)
        q = torch.zeros((1, d), dtype=torch.float32, device=dev)
    mpr = min(cap, 1024) if max_pair_rows is None else max(1, min(int(max_pair_rows), cap, 1024))
    norm = torch.empty(cap, dtype=torch.float32, device=dev)
    uv = torch.empty((2, cap), dtype=torch.int32, device=dev)
    row_pair = torch.empty(cap, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.dcn_best_match_pairs_workspace(cap)), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_best_match_pairs(P, h, w, d, p(rb), p(q), p(off), cap, mpr, p(norm), p(uv), p(row_pair), p(status), p(ws),
                                  _lib.stream_ptr())
    _lib.check(rc, "dcn_best_match_pairs")
    return BestMatches(norm[:R], uv[:, :R], row_pair[:R], status)


class AcrossObjectTable(collections.namedtuple(
        "AcrossObjectTable", "norm_diff_descriptor_best_match best_uv row_pair offsets mask_pixels status u_a v_a")):
    """Device tensors, R = P * num_uv_a_samples the row capacity; the rows in use are [0, offsets[-1]), pair p's at
    offsets[p]:offsets[p+1].  norm_diff_descriptor_best_match float32 [R] (NaN past the last row); best_uv int32 [2, R] (u, v
    of the best match in image b; -1 past the last row); row_pair int32 [R] (-1 past the last row); offsets int64 [P + 1];
    mask_pixels int32 [P] (mask a's); status int32 [1] (TOO_FEW_MASK_PIXELS | BAD_DRAWS from the queries, BAD_OFFSETS from
    the search, BAD_FRAME for a frame the gather rejected); u_a, v_a int64 [R]: the sampled pixels of image a."""


def _object_pairs(store, pairs):
    a = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs)
    if a.ndim != 2 or a.shape[1] not in (2, 6) or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("pairs must be an integer array [P, 2] of (frame a, frame b) or choose_object_pairs' [P, 6], P >= 1")
    return _frame_pairs(store, a[:, -2:])


def evaluate_object_pairs(dcn, store, pairs, num_uv_a_samples=100, *, generator=None, sample_order=None, batch_pairs=8,
                          mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV):
    """``single_across_object_image_pair_quantitative_analysis`` (evaluation.py:784-859) for ``pairs`` ([P, 2] store frame
    indices (a, b), or choose_object_pairs' [P, 6]; P <= 1024) on the device: 1. ``dcn_gather_frames`` of the chosen frames'
    images and masks, 2. ToTensor + Normalize and ``dcn.forward_image_tensors`` in eval mode, ``batch_pairs`` pairs at a time
    (as ``evaluate_frame_pairs``), 3. across_object_queries on mask a (``sample_order`` replay, otherwise ``generator``), 4.
    best_match_pairs over image b.  -> AcrossObjectTable, its ``status`` covering the whole chain.  The pair list is given on
    the host; nothing is read back.  ``dcn.training`` is left as found."""
    fr = _object_pairs(store, pairs)
    P = int(fr.shape[0])
    if P > 1024:
        raise ValueError("at most 1024 pairs per call, got %d" % P)
    if int(batch_pairs) < 1:
        raise ValueError("batch_pairs must be >= 1")
    rgb, _, mask, _, status = _gather_host_frames(store, fr, ("rgb", "mask"))
    res = [[], []]

    def keep(lo, n, y):
        res[0].append(y[:n])
        res[1].append(y[n:])
    _forward_in_eval_mode(dcn, rgb[0], mask[0], rgb[1], mask[1], int(batch_pairs), mean, std, keep)
    res_a, res_b = torch.cat(res[0]).contiguous(), torch.cat(res[1]).contiguous()
    q = across_object_queries(mask[0], res_a, num_uv_a_samples, generator=generator, sample_order=sample_order)
    m = best_match_pairs(res_b, q.queries, q.offsets, max_pair_rows=int(num_uv_a_samples))
    word = q.status | m.status | (status & 1) * BAD_FRAME     # one status word for the chain (on the device)
    return AcrossObjectTable(m.norm_diff_descriptor_best_match, m.best_uv, m.row_pair, q.offsets, q.mask_pixels,
                             word.to(torch.int32), q.u_a, q.v_a)


def evaluate_network_across_objects(dcn, store, num_image_pairs=25, num_uv_a_samples=100, host_rng=None, generator=None):
    """``DenseCorrespondenceEvaluation.evaluate_network_across_objects`` (evaluation.py:305-337) on a frame store:
    choose_object_pairs, then evaluate_object_pairs, then ONE copy to the host.  -> (table, dataframe): ``table`` a dict of
    numpy columns under ACROSS_OBJECT_COLUMNS, the reference's ``DCNEvaluationPandaTemplateAcrossObject.columns``
    (``norm_diff_descriptor_best_match`` float32, the image indices int64, names and object ids as objects); ``dataframe`` a
    ``pandas.DataFrame`` of it when pandas imports, else None.  A pair whose mask a is empty contributes no rows, as in the
    reference; ValueError("Sample larger than population"), the reference's ``random.sample`` error, when a mask a has pixels
    but fewer than ``num_uv_a_samples``.  ``dcn.training`` is left as found."""
    chosen = choose_object_pairs(store, num_image_pairs, host_rng)
    if chosen.shape[0] == 0:
        norm, pair = np.zeros(0, np.float32), np.zeros(0, np.int64)
    else:
        t = evaluate_object_pairs(dcn, store, chosen, num_uv_a_samples, generator=generator)
        # one transfer: the distances, the rows' pairs and the status word packed into one float64 block
        block = torch.stack([t.norm_diff_descriptor_best_match.double(), t.row_pair.double(),
                             t.status.double().expand_as(t.row_pair)]).cpu().numpy()
        word = int(block[2, 0])
        if word & TOO_FEW_MASK_PIXELS:
            raise ValueError("Sample larger than population")
        if word:
            raise RuntimeError("dcn_hip: the across-object evaluation failed on the device (status %d)" % word)
        rows = int(np.sum(block[1] >= 0))                      # (rows past the last one carry pair -1)
        norm, pair = block[0, :rows].astype(np.float32), block[1, :rows].astype(np.int64)
    first = np.asarray(store.scene_first_frame_host, np.int64)
    table = {"norm_diff_descriptor_best_match": norm}
    for side, (o, s, f) in (("a", (0, 2, 4)), ("b", (1, 3, 5))):
        scene = chosen[pair, s] if len(pair) else np.zeros(0, np.int64)
        local = (chosen[pair, f] if len(pair) else np.zeros(0, np.int64)) - first[scene]
        table["scene_name_" + side] = np.array([store.scene_names[i] for i in scene], dtype=object)
        table["object_id_" + side] = np.array([store.object_ids[i] for i in (chosen[pair, o] if len(pair) else [])],
                                              dtype=object)
        table["img_%s_idx" % side] = np.array([int(store.frame_ids[i][j]) for i, j in zip(scene, local)], dtype=np.int64)
    assert set(table) == set(ACROSS_OBJECT_COLUMNS)
    try:
        import pandas
        df = pandas.DataFrame({k: table[k] for k in ACROSS_OBJECT_COLUMNS})
    except ImportError:
        df = None
    return table, df


# ---- cross-scene evaluation (evaluation.py:253-301, :610-781) -------------------------------------------------------------
CrossSceneLabels = collections.namedtuple("CrossSceneLabels", "pairs pixels skipped")
LABELLED, VIEW_OF_A, VIEW_OF_B = 0, 1, 2      # a row's kind in choose_cross_scene_views' table


def _py2_round(x):
    """Python 2's ``round``: half away from zero"""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


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
    if not torch.is_tensor(queries) or queries.dtype != torch.float32 or queries.dim() != 2 or int(queries.shape[1]) != d:
        raise ValueError("queries must be float32 [R, %d]" % d)
    q = queries.contiguous()
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
    if not torch.is_tensor(offsets) or offsets.dtype != torch.int64 or int(offsets.numel()) != G + 1:
        raise ValueError("offsets must be an int64 tensor of G + 1 = %d entries" % (G + 1))
    off = offsets.contiguous().view(-1)
    _on_device(rb, mb, db, q, ua, va, dq, ub, vb, cams, kp, off)
    dev = rb.device
    cap = max(R, 1)
    if R == 0:                                             # (no rows at all: the kernels still want valid pointers)
        q = torch.zeros((1, d), dtype=torch.float32, device=dev)
        ua = va = torch.zeros(1, dtype=torch.int64, device=dev)
        ub = vb = torch.zeros(1, dtype=torch.float32, device=dev)
        dq = torch.zeros(1, dtype=torch.int16, device=dev)
        cams = torch.zeros((1, _args.CAM_FLOATS), dtype=torch.float32, device=dev)
        kp = torch.zeros(1, dtype=torch.uint8, device=dev)
    mgr = cap if max_group_rows is None else max(1, min(int(max_group_rows), cap))
    cols = torch.empty((len(COLUMNS), cap), dtype=torch.float64, device=dev)
    valid = torch.empty((2, cap), dtype=torch.uint8, device=dev)
    pred = torch.empty((4, cap), dtype=torch.int32, device=dev)
    closer = torch.empty((2, cap), dtype=torch.int32, device=dev)
    row_pair = torch.empty(cap, dtype=torch.int32, device=dev)
    mask_pixels = torch.empty(G, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.dcn_match_statistics_groups_workspace(cap)), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rows_in = (G, h, w, d, p(rb), p(mb), p(db), p(q), p(ua), p(va), p(dq), p(ub), p(vb), p(cams), p(kp), p(off), cap, mgr)
    rows_out = (p(cols), p(valid), p(pred), p(closer), p(row_pair), p(mask_pixels), p(status), p(ws), _lib.stream_ptr())
    if _strip_pixels is None:
        _lib.check(lib.dcn_match_statistics_groups(*(rows_in + rows_out)), "dcn_match_statistics_groups")
    else:                                                   # (match_statistics_groups_wide)
        _lib.check(lib.dcn_match_statistics_groups_wide(*(rows_in + (int(_strip_pixels),) + rows_out)),
                   "dcn_match_statistics_groups_wide")
    return EvalTable(cols[:, :R], valid[:, :R], pred[:, :R], closer[:, :R], row_pair[:R], off, mask_pixels, status,
                     u_a, v_a, u_b, v_b)


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


def _gather_frame_list(store, frames, want):
    """``_gather_host_frames`` of a host LIST of n frames: they travel as the two slots of (n + 1) // 2 pairs (an odd n repeats
    the last frame), so that the [2, P] planes, flattened, are the n frames in order -> (rgb, depth, mask, status)"""
    n = len(frames)
    P = (n + 1) // 2
    fr = np.concatenate([frames, frames[-1:]])[:2 * P].reshape(2, P).T
    rgb, depth, mask, _, status = _gather_host_frames(store, fr, want)
    flat = lambda t, tail: None if t is None else t.view((2 * P, store.h, store.w) + tail)[:n]
    return flat(rgb, (3,)), flat(depth, ()), flat(mask, ()), status


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
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
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


def _camera_rows_of(store, fr, host_keep):
    """Camera rows (K of slot 0's scene, K^-1, pose of slot 0, inverse pose of slot 1) for T rows from ``dcn_gather_frames``
    over ``fr`` (host int [T, 2]); rows without both frames (``host_keep`` false) reach the gather as frame 0 -- they are
    left out anyway.  -> (cams float32 [T, 50], BAD_FRAME status word)"""
    cams, word = [], 0
    for lo in range(0, int(fr.shape[0]), 16384):
        got = _gather_host_frames(store, np.where(host_keep[lo:lo + 16384, None], fr[lo:lo + 16384], 0), ("cams",))
        cams.append(got[3][0])
        word = word | (got[4] & 1) * BAD_FRAME
    return torch.cat(cams), word


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
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
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
    nan_table = lambda: EvalTable(
        torch.full((len(COLUMNS), T), float("nan"), dtype=torch.float64, device=dev),
        torch.zeros((2, T), dtype=torch.uint8, device=dev), torch.full((4, T), -1, dtype=torch.int32, device=dev),
        torch.zeros((2, T), dtype=torch.int32, device=dev), torch.full((T,), -1, dtype=torch.int32, device=dev), offsets,
        torch.zeros(T, dtype=torch.int32, device=dev), word, u_a, v_a, u_b, v_b)
    kept = np.nonzero(host_keep)[0]
    if len(kept) == 0:
        return nan_table()
    # 2. the query descriptors: one forward pass per distinct a-side frame
    a_frames, a_slot = np.unique(fa[kept], return_inverse=True)
    by_slot = np.argsort(a_slot, kind="stable")
    a_rows, a_local = up(kept[by_slot]), up(a_slot[by_slot])
    a_bounds = np.searchsorted(a_slot[by_slot], np.arange(len(a_frames) + 1))
    rgb, _, mask, bad = _gather_frame_list(store, a_frames, ("rgb", "mask"))
    word = word | (bad & 1) * BAD_FRAME
    queries = []

    def take(lo, n, res):
        if not queries:
            queries.append(torch.zeros((T, int(res.shape[3])), dtype=torch.float32, device=dev))
        rows = a_rows[a_bounds[lo]:a_bounds[lo + n]]
        queries[0][rows] = res[a_local[a_bounds[lo]:a_bounds[lo + n]] - lo, v_a[rows], u_a[rows]].float()
    _forward_in_eval_mode(dcn, rgb, mask, None, None, int(batch_frames), mean, std, take)
    del rgb, mask
    queries = queries[0]
    d = int(queries.shape[1])
    depth_q = store.depth[up(np.where(host_keep, fa, 0)), v_a, u_a]
    # camera rows per row (frames of rows without both reach the gather as frame 0: the row is left out anyway)
    cams, bad = _camera_rows_of(store, v[:, 3:5], host_keep)
    word = word | bad
    # 3. the rows by the frame they search, the searched frames in chunks; 4. back into the order of ``views``
    out = nan_table()
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
    # one transfer: everything packed into one float64 block (ints up to 2^31 are exact)
    block = torch.cat([t.columns, t.is_valid.double(), t.row_pair.double().view(1, -1),
                       t.status.double().expand_as(t.row_pair).view(1, -1)]).cpu().numpy()
    if block.shape[1] and int(block[-1, 0]):
        raise RuntimeError("dcn_hip: the cross-scene evaluation failed on the device (status %d)" % int(block[-1, 0]))
    rows = np.nonzero(block[-2] >= 0)[0]
    block = block[:, rows]
    table = {k: block[i].copy() for i, k in enumerate(COLUMNS)}
    table["is_valid"] = block[len(COLUMNS)] != 0
    table["is_valid_masked"] = block[len(COLUMNS) + 1] != 0
    first = np.asarray(store.scene_first_frame_host, np.int64)
    pairs = labels.pairs[views[rows, 0]]
    table["scene_name"] = np.array([store.scene_names[a] + "+" + store.scene_names[b] for a, b in pairs[:, [1, 3]]],
                                   dtype=object)
    for key, col in (("img_a_idx", 3), ("img_b_idx", 4)):
        scene = np.searchsorted(first, views[rows, col], side="right") - 1
        table[key] = np.array([int(store.frame_ids[s][f - first[s]]) for s, f in zip(scene, views[rows, col])],
                              dtype=np.int64)
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
        table = {k: np.zeros(0, np.float64) for k in COLUMNS}
        table.update(is_valid=np.zeros(0, bool), is_valid_masked=np.zeros(0, bool), scene_name=np.zeros(0, object),
                     img_a_idx=np.zeros(0, np.int64), img_b_idx=np.zeros(0, np.int64))
    else:
        table = cross_scene_table(store, labels, views, evaluate_cross_scene_rows(dcn, store, labels, views))
    assert set(table) == set(names)
    try:
        import pandas
        df = pandas.DataFrame({k: table[k] for k in names})
    except ImportError:
        df = None
    return table, df


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


# ---- class-consistent keypoints (evaluation.py:407-472, :1433-1552, :2413-2462) ----------------------------------------------
KeypointLabels = collections.namedtuple("KeypointLabels", "images names uv object_ids size skipped")
KEYPOINT_ROW_COLUMNS = ("combination", "keypoint", "order", "frame_1", "frame_2", "u_1", "v_1", "u_2", "v_2", "k_frame")
KEYPOINT_COLUMNS = ("img_a_idx", "img_b_idx", "scene_name_a", "scene_name_b", "object_id_a", "object_id_b", "keypoint_name")
STANDARD, REVERSE = 0, 1                      # a row's order in keypoint_rows' table
WIDE_GROUP_MIN_ROWS = 24                      # evaluate_keypoint_rows(search=None): mean rows per searched image from which
#                                               the wide entry is used.  Measured (profiles/keypoint_bench_crossover.json, 8
#                                               images of 640x480): at 21 rows the two entries tie (1.29x at D = 3, 0.96x at
#                                               D = 16), at 28 the wide one wins at both (1.66x, 1.25x), at 14 it loses


def _yaml_file(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def keypoint_labels(store, annotations):
    """The reference's class-consistent keypoint annotations (evaluation/utils.py:59-81: a list of dicts {scene_name,
    image_idx, object_id, keypoints: {name: {u, v, ...}}}, or a path to its YAML) resolved to the frames of ``store`` through
    ``store.scene_names`` / ``store.frame_ids``, as ``cross_scene_labels`` resolves its pairs.

    -> KeypointLabels: ``images`` int64 [K, 3] of (index in ``annotations``, scene, frame), frame as a store index; ``names``:
    per image the keypoint names in the order of its mapping; ``uv``: per image float64 [M, 2], u and v AS GIVEN (they are
    rounded per row, keypoint_rows); ``object_ids``: per image, the annotation's; ``size`` (h, w) of the store's images;
    ``skipped``: [(index, reason)] for the images whose scene or image the store does not hold.  ValueError for an empty
    list."""
    if isinstance(annotations, str):
        annotations = _yaml_file(annotations)
    if annotations is None or len(annotations) == 0:
        raise ValueError("no keypoint annotations given")
    first = store.scene_first_frame_host
    images, names, uv, object_ids, skipped = [], [], [], [], []
    for i, an in enumerate(annotations):
        if an["scene_name"] not in store.scene_names:
            skipped.append((i, "the store holds no scene %r" % (an["scene_name"],)))
            continue
        sc = store.scene_names.index(an["scene_name"])
        ids = [int(x) for x in store.frame_ids[sc]]
        if int(an["image_idx"]) not in ids:
            skipped.append((i, "scene %r holds no image %r" % (an["scene_name"], an["image_idx"])))
            continue
        images.append([i, sc, first[sc] + ids.index(int(an["image_idx"]))])
        names.append([str(k) for k in an["keypoints"]])
        uv.append(np.asarray([[float(kp["u"]), float(kp["v"])] for kp in an["keypoints"].values()], np.float64).reshape(-1, 2))
        object_ids.append(an.get("object_id"))
    return KeypointLabels(np.asarray(images, np.int64).reshape(-1, 3), names, uv, object_ids, (int(store.h), int(store.w)),
                          skipped)


def keypoint_rows(labels, reference_query_pixel=True):
    """The rows of single_image_pair_cross_scene_keypoints_quantitative_analysis (evaluation.py:1433-1552) over
    ``itertools.combinations(images, 2)`` (:447), on the host and in the reference's order: per combination the keypoints of
    its FIRST image in that image's order, per keypoint "standard" (image 1 = the first image, searched image 2 = the second)
    then "reverse".

    Kept from the reference ON PURPOSE: ValueError("keypoint %s appears in one list of annotated data but not the other") when
    a name of the first image is missing from the second, while extra names of the second are ignored (:1505-1508); the query
    pixel is (u of image 1, v of image 2) -- evaluation.py:1523 as written, ``(data[idx_1]['u'], data[idx_2]['v'])`` --
    unless ``reference_query_pixel`` is False, which gives (u_1, v_1); both pixels go through
    clip_pixel_to_image_size_and_round (Python 2's ``round``, ``min(..., size - 1)``), and a pixel that rounds below zero is
    a ValueError as in ``cross_scene_labels``; the K of a row is that of the scene of the combination's FIRST image for both
    orders (:1490-1495).

    -> int64 array [R, 10] in the order of KEYPOINT_ROW_COLUMNS: combination (its index in ``itertools.combinations``),
    keypoint (index among the first image's names), order (STANDARD / REVERSE), frame 1 (the query's), frame 2 (the searched
    one), u_1, v_1 (the query pixel), u_2, v_2 (the ground truth in frame 2), and the frame whose scene supplies K; frames as
    store indices."""
    import itertools
    h, w = labels.size
    out = []
    for c, (i, j) in enumerate(itertools.combinations(range(labels.images.shape[0]), 2)):
        for k, name in enumerate(labels.names[i]):
            if name not in labels.names[j]:
                raise ValueError("keypoint %s appears in one list of annotated data but not the other" % (name,))
            data = (labels.uv[i][k], labels.uv[j][labels.names[j].index(name)])
            for order, (i1, i2) in ((STANDARD, (0, 1)), (REVERSE, (1, 0))):
                query = (data[i1][0], data[i2][1] if reference_query_pixel else data[i1][1])
                px = [min(_py2_round(x), size - 1) for x, size in ((query[0], w), (query[1], h), (data[i2][0], w),
                                                                   (data[i2][1], h))]
                if min(px) < 0:
                    raise ValueError("keypoint %s of annotations %d / %d: a labelled pixel is negative" % (
                        name, labels.images[i, 0], labels.images[j, 0]))
                frames = (labels.images[i, 2], labels.images[j, 2])
                out.append([c, k, order, frames[i1], frames[i2]] + px + [frames[0]])
    return np.asarray(out, np.int64).reshape(-1, len(KEYPOINT_ROW_COLUMNS))


def _keypoint_rows_table(store, rows):
    r = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows)
    if r.ndim != 2 or r.shape[1] != len(KEYPOINT_ROW_COLUMNS) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("rows must be keypoint_rows' integer table [R, %d], got %s" % (len(KEYPOINT_ROW_COLUMNS), r.shape))
    r = r.astype(np.int64)
    if r.shape[0] and (r[:, [3, 4, 9]].min() < 0 or r[:, [3, 4, 9]].max() >= store.num_frames):
        raise ValueError("rows name a frame outside the store's %d frames" % store.num_frames)
    return r


def evaluate_keypoint_rows(dcn, store, labels, rows, *, batch_frames=16, max_search_bytes=2 << 30, search=None,
                           mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV):
    """compute_descriptor_match_statistics for every row of ``rows`` (keypoint_rows' table over ``labels``) on the device,
    nothing read back: 1. ``dcn.forward_image_tensors`` in eval mode ONCE per distinct labelled frame (the reference caches
    per (scene, image_idx) too, :428-441), ``batch_frames`` at a time, keeping the rows' query descriptors -- and the
    descriptor images themselves when all of them fit in ``max_search_bytes``; otherwise evaluate_cross_scene_rows' two
    sweeps: the searched frames are forwarded again, chunk by chunk; 2. the rows sorted by the frame they search, one group per
    frame, camera rows from ``dcn_gather_frames`` over (frame 1, frame 2) with the K and K^-1 slots replaced by those of the
    row's K frame; 3. the statistics by ``search``: "wide" (match_statistics_groups_wide), "groups" (match_statistics_groups)
    or None: wide from WIDE_GROUP_MIN_ROWS rows per searched image on average.  Both give the same bits, so the choice does
    not show in the result.

    -> EvalTable with one row per row of ``rows``, in that order: ``row_pair`` the row's combination; ``offsets`` int64 [C + 1],
    the combinations' row ranges; ``mask_pixels`` int32 [R], PER ROW: the mask pixels of the image the row searched; u_a, v_a
    the query pixel, u_b, v_b the ground truth; ``status``: the statistics' bits and BAD_FRAME for the gathers.
    ``dcn.training`` is left as found."""
    v = _keypoint_rows_table(store, rows)
    if int(batch_frames) < 1 or int(max_search_bytes) < 1:
        raise ValueError("batch_frames and max_search_bytes must be >= 1")
    if search not in (None, "wide", "groups"):
        raise ValueError('search must be None, "wide" or "groups", got %r' % (search,))
    T, dev, h, w = int(v.shape[0]), store.device, store.h, store.w
    if T == 0:
        raise ValueError("no keypoint rows given")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    comb, fa, fb, kf = v[:, 0], v[:, 3], v[:, 4], v[:, 9]
    u_a, v_a = up(v[:, 5]), up(v[:, 6])
    u_b, v_b = up(v[:, 7].astype(np.float32)), up(v[:, 8].astype(np.float32))
    keep = torch.ones(T, dtype=torch.uint8, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    ncomb = int(comb.max()) + 1
    offsets = up(np.searchsorted(comb, np.arange(ncomb + 1)).astype(np.int64))
    # 1. one forward pass per distinct labelled frame
    frames = np.unique(np.concatenate([fa, fb]))
    slot = np.searchsorted(frames, fa)
    by_slot = np.argsort(slot, kind="stable")
    a_rows, a_local = up(by_slot), up(slot[by_slot])
    a_bounds = np.searchsorted(slot[by_slot], np.arange(len(frames) + 1))
    rgb, _, mask, bad = _gather_frame_list(store, frames, ("rgb", "mask"))
    word = word | (bad & 1) * BAD_FRAME
    queries, images = [], []

    def take(lo, n, res):
        if not queries:
            queries.append(torch.zeros((T, int(res.shape[3])), dtype=torch.float32, device=dev))
            if len(frames) * h * w * int(res.shape[3]) * 4 <= int(max_search_bytes):      # every image stays
                images.append(torch.empty((len(frames), h, w, int(res.shape[3])), dtype=torch.float32, device=dev))
        at = a_rows[a_bounds[lo]:a_bounds[lo + n]]
        queries[0][at] = res[a_local[a_bounds[lo]:a_bounds[lo + n]] - lo, v_a[at], u_a[at]].float()
        if images:
            images[0][lo:lo + n] = res
    _forward_in_eval_mode(dcn, rgb, mask, None, None, int(batch_frames), mean, std, take)
    del rgb, mask
    queries = queries[0]
    depth_q = store.depth[up(fa), v_a, u_a]
    # 2. camera rows: pose 1 and pose 2^-1 of the row's frames, K and K^-1 of the combination's first image
    cams, bad = _camera_rows_of(store, v[:, 3:5], np.ones(T, bool))
    of_k, bad_k = _camera_rows_of(store, np.stack([kf, kf], axis=1), np.ones(T, bool))
    cams[:, :18] = of_k[:, :18]
    word = word | bad | bad_k
    # 3. the rows by the frame they search
    if search is None:
        search = "wide" if T >= WIDE_GROUP_MIN_ROWS * len(np.unique(fb)) else "groups"
    out = EvalTable(
        torch.full((len(COLUMNS), T), float("nan"), dtype=torch.float64, device=dev),
        torch.zeros((2, T), dtype=torch.uint8, device=dev), torch.full((4, T), -1, dtype=torch.int32, device=dev),
        torch.zeros((2, T), dtype=torch.int32, device=dev), torch.full((T,), -1, dtype=torch.int32, device=dev), offsets,
        torch.zeros(T, dtype=torch.int32, device=dev), word, u_a, v_a, u_b, v_b)
    word = _search_rows_by_frame(dcn, store, out, word, fb, np.arange(T), comb, queries, depth_q, cams, keep, int(batch_frames),
                                 int(max_search_bytes), mean, std,
                                 match_statistics_groups_wide if search == "wide" else match_statistics_groups,
                                 resident=(frames, images[0]) if images else None)
    return out._replace(status=word.to(torch.int32))


def keypoint_table(store, labels, rows, t):
    """evaluate_keypoint_rows' EvalTable ``t`` (over ``rows``) as the reference's table, with ONE copy to the host: a dict of
    numpy columns under the reference's column names (COLUMNS as float64, ``is_valid`` / ``is_valid_masked`` as bool) plus
    KEYPOINT_COLUMNS by the row's order (evaluation.py:1541-1547): ``img_a_idx`` / ``scene_name_a`` / ``object_id_a`` of the
    image the query comes from, ``..._b`` of the image searched, and ``keypoint_name``.  RuntimeError when the chain's status
    word is not zero."""
    import itertools
    rows = _keypoint_rows_table(store, rows)
    # one transfer: everything packed into one float64 block (ints up to 2^31 are exact)
    block = torch.cat([t.columns, t.is_valid.double(), t.status.double().expand_as(t.row_pair).view(1, -1)]).cpu().numpy()
    if block.shape[1] and int(block[-1, 0]):
        raise RuntimeError("dcn_hip: the keypoint evaluation failed on the device (status %d)" % int(block[-1, 0]))
    table = {k: block[i].copy() for i, k in enumerate(COLUMNS)}
    table["is_valid"] = block[len(COLUMNS)] != 0
    table["is_valid_masked"] = block[len(COLUMNS) + 1] != 0
    combos = np.asarray(list(itertools.combinations(range(labels.images.shape[0]), 2)), np.int64).reshape(-1, 2)
    first = np.asarray(store.scene_first_frame_host, np.int64)
    pair = combos[rows[:, 0]]                                                   # (first image, second image) per row
    table["keypoint_name"] = np.array([labels.names[i][k] for i, k in zip(pair[:, 0], rows[:, 1])], dtype=object)
    reverse = rows[:, 2] == REVERSE
    for side, image in (("a", np.where(reverse, pair[:, 1], pair[:, 0])), ("b", np.where(reverse, pair[:, 0], pair[:, 1]))):
        scene, frame = labels.images[image, 1], labels.images[image, 2]
        table["scene_name_" + side] = np.array([store.scene_names[s] for s in scene], dtype=object)
        table["img_%s_idx" % side] = np.array([int(store.frame_ids[s][f - first[s]]) for s, f in zip(scene, frame)],
                                              dtype=np.int64)
        table["object_id_" + side] = np.array([labels.object_ids[i] for i in image], dtype=object)
    return table


def evaluate_network_cross_scene_keypoints(dcn, store, annotations, save_to=None):
    """``DenseCorrespondenceEvaluation.evaluate_network_cross_scene_keypoints`` (evaluation.py:407-472) on a frame store:
    keypoint_labels, keypoint_rows, evaluate_keypoint_rows, then keypoint_table's ONE copy to the host.  -> (table,
    dataframe) like ``evaluate_network``: ``table`` as keypoint_table returns it; ``dataframe`` a ``pandas.DataFrame`` of it
    when pandas imports, else None.  ``save_to``: a folder that receives ``data.csv``, the file
    run_cross_instance_keypoint_evaluation_on_network (:2413-2462) writes into ``<model folder>/analysis/
    cross_scene_keypoints`` (by pandas when it imports, otherwise by the csv module with the same header and index column).
    Fewer than two usable labelled images give an empty table.  ``dcn.training`` is left as found."""
    labels = keypoint_labels(store, annotations)
    rows = keypoint_rows(labels)
    names = COLUMNS + ("is_valid", "is_valid_masked") + KEYPOINT_COLUMNS
    if rows.shape[0] == 0:
        table = {k: np.zeros(0, np.float64) for k in COLUMNS}
        table.update(is_valid=np.zeros(0, bool), is_valid_masked=np.zeros(0, bool), img_a_idx=np.zeros(0, np.int64),
                     img_b_idx=np.zeros(0, np.int64))
        table.update({k: np.zeros(0, object) for k in KEYPOINT_COLUMNS if k not in table})
    else:
        table = keypoint_table(store, labels, rows, evaluate_keypoint_rows(dcn, store, labels, rows))
    assert set(table) == set(names)
    try:
        import pandas
        df = pandas.DataFrame({k: table[k] for k in names})
    except ImportError:
        df = None
    if save_to is not None:
        if not os.path.isdir(save_to):
            os.makedirs(save_to)
        path = os.path.join(save_to, "data.csv")
        if df is not None:
            df.to_csv(path)
        else:
            import csv
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(("",) + names)
                for i in range(len(table["is_valid"])):
                    out.writerow([i] + [table[k][i] for k in names])
    return table, df


def descriptor_statistics(res, mask):
    """``compute_descriptor_statistics`` (evaluation.py:2177-2219) for n descriptor images in ONE pass over ``res`` and ``mask``.

    res: float32 [n, H, W, D] descriptor images, channel last, as ``forward_image_tensors`` returns them (D = 1 .. 64); mask:
    uint8 or bool [n, H, W] (non-zero = on the object).
    -> (per_image float32 [n, 2, 3, D]: axis 1 entire image, mask; axis 2 min, max, mean; mask_pixels int32 [n]).  Sums in
    float64, the mean rounded to float32 once; bit-identical from run to run; NaN as in torch (a NaN in a channel makes its
    min, max and mean NaN; for the mask rows only a NaN under the mask); an empty mask gives mask_pixels 0 and NaN mask rows.
    No host synchronization."""
    lib = _lib.get()
    if not torch.is_tensor(res) or not torch.is_tensor(mask):
        raise ValueError("res and mask must be tensors")
    if res.dim() != 4:
        raise ValueError("res must be [n, H, W, D], got %s" % (tuple(res.shape),))
    if res.dtype != torch.float32:
        raise ValueError("res must be float32, got %s" % res.dtype)
    n, h, w, d = (int(x) for x in res.shape)
    if d < 1 or d > 64:
        raise ValueError("descriptor dimension must be 1 .. 64, got %d" % d)
    if n < 1 or n > 65535 or h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError("res must hold 1 .. 65535 images of 1 <= H * W < 2^31 pixels, got %s" % (tuple(res.shape),))
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mask must be uint8 (or bool), got %s" % mask.dtype)
    m = _args.mask(mask, n, h, w, "mask")
    r = res.contiguous()
    try:
        _lib.require_device(r, m)
    except RuntimeError as e:
        raise ValueError(str(e))
    if r.device != m.device:
        raise ValueError("res and mask must be on one device, got %s and %s" % (r.device, m.device))
    dev = r.device
    per_image = torch.empty((n, 2, 3, d), dtype=torch.float32, device=dev)
    mask_pixels = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, int(lib.dcn_descriptor_statistics_workspace(n, h, w, d))), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_descriptor_statistics(n, h, w, d, p(r), p(m), p(per_image), p(mask_pixels), p(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_descriptor_statistics")
    return per_image, mask_pixels


def combine_descriptor_statistics(per_image, mask_pixels, num_images=None):
    """The reference's ``update_stats`` loop and final scaling (evaluation.py:2237-2292) over ``descriptor_statistics``'
    outputs (per_image float32 [N, 2, 3, D], mask_pixels int32 [N]) in one launch: images with an empty mask are skipped for
    both sets of statistics, min / max over the images used, mean = the float32 sum of their means in image order times
    float32(1.0 / num_images) -- ``num_images`` (default N), not the number used, as in the reference.
    -> (stats float32 [2, 3, D], used int32 [1]); ``stats`` is NaN when no image was used.  No host synchronization."""
    lib = _lib.get()
    if not torch.is_tensor(per_image) or per_image.dim() != 4 or tuple(per_image.shape[1:3]) != (2, 3) \
            or per_image.dtype != torch.float32:
        raise ValueError("per_image must be float32 [N, 2, 3, D]")
    N, d = int(per_image.shape[0]), int(per_image.shape[3])
    if N < 1 or d < 1 or d > 64:
        raise ValueError("per_image must hold N >= 1 images of 1 .. 64 channels, got %s" % (tuple(per_image.shape),))
    if not torch.is_tensor(mask_pixels) or mask_pixels.dtype != torch.int32 or tuple(mask_pixels.shape) != (N,):
        raise ValueError("mask_pixels must be int32 [%d]" % N)
    num = N if num_images is None else int(num_images)
    if num < 1:
        raise ValueError("num_images must be >= 1, got %d" % num)
    pi, mp = per_image.contiguous(), mask_pixels.contiguous()
    try:
        _lib.require_device(pi, mp)
    except RuntimeError as e:
        raise ValueError(str(e))
    dev = pi.device
    stats = torch.empty((2, 3, d), dtype=torch.float32, device=dev)
    used = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = lib.dcn_descriptor_statistics_combine(N, d, p(pi), p(mp), num, p(stats), p(used), _lib.stream_ptr())
    _lib.check(rc, "dcn_descriptor_statistics_combine")
    return stats, used


def choose_frames(store, num_images, host_rng=None):
    """``num_images`` times the rule of ``get_random_rgbd_mask_pose`` (spartan_dataset_masked.py:410-421), on the host: a scene
    by ``get_random_scene_name`` (as ``choose_pairs``), then a frame uniform over that scene's frames.  As in ``choose_pairs``
    the rule is replayed, not the reference's random stream (it draws the scene and the image twice, :418-419).
    ``host_rng``: a numpy RandomState / Generator (default ``np.random``).
    -> int64 array [num_images, 2] of (scene, frame), frames as store indices."""
    rng = host_rng if host_rng is not None else np.random
    first = store.scene_first_frame_host
    lots = _lots(store)
    out = []
    for _ in range(int(num_images)):
        s = _random_scene(store, rng, lots)
        out.append((s, first[s] + _below(rng, first[s + 1] - first[s])))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


STAT_SETS, STAT_FIELDS = ("entire_image", "mask_image"), ("min", "max", "mean")


def compute_descriptor_statistics_on_dataset(dcn, store, num_images=100, save_to_file=True, filename=None, host_rng=None,
                                             batch_images=16):
    """``DenseCorrespondenceEvaluation.compute_descriptor_statistics_on_dataset`` (evaluation.py:2157-2304) on a frame store:
    1. choose_frames, 2. ONE ``dcn_gather_frames`` of their images and masks, 3. ToTensor + Normalize by the augmentation kernel
    with every augmentation switched off (the dataset's mean and standard deviation, as ``evaluate_frame_pairs``), 4. ``dcn.forward_image_tensors`` in eval mode,
    ``batch_images`` images at a time, 5. descriptor_statistics per batch into slices of one [num_images, 2, 3, D] tensor,
    6. one combine_descriptor_statistics launch, 7. ONE copy to the host.
    -> the reference's dict {'entire_image': {'min': [...], 'max': [...], 'mean': [...]}, 'mask_image': {...}} of lists of
    Python floats, written with ``utils.saveToYaml`` when ``save_to_file`` -- to ``filename``, by default
    ``<dcn's network params folder>/descriptor_statistics.yaml``, the file ``dcn.descriptor_image_stats`` reads.  ValueError
    when every chosen frame's mask was empty (the reference fails on ``None.tolist()``).  ``dcn.training`` is left as found."""
    n = int(num_images)
    step = int(batch_images)
    if n < 1 or n > 65534:
        raise ValueError("num_images must be 1 .. 65534, got %d" % n)
    if step < 1:
        raise ValueError("batch_images must be >= 1")
    if save_to_file and filename is None:                   # (before any work: a network without the folder cannot save)
        import dense_correspondence_manipulation.utils.utils as utils
        filename = os.path.join(utils.convert_to_absolute_path(dcn.path_to_network_params_folder),
                                "descriptor_statistics.yaml")
    chosen = choose_frames(store, n, host_rng)
    dev = store.device
    h, w = store.h, store.w
    # the gather copies pairs of frames: frames [0, P) in slot 0 and [P, n) in slot 1 (an odd n repeats the last frame), so
    # that the [2, P] planes, flattened, are the n frames in order
    P = (n + 1) // 2
    fr = np.concatenate([chosen[:, 1], chosen[-1:, 1]])[:2 * P].reshape(2, P).T
    rgb, _, mask, _, bad_frame = _gather_host_frames(store, fr, ("rgb", "mask"))
    rgb, mask = rgb.view(2 * P, h, w, 3)[:n], mask.view(2 * P, h, w)[:n]
    out = []

    def statistics(lo, k, res):
        if not out:
            out.extend([torch.empty((n, 2, 3, int(res.shape[3])), dtype=torch.float32, device=dev),
                        torch.empty(n, dtype=torch.int32, device=dev)])
        out[0][lo:lo + k], out[1][lo:lo + k] = descriptor_statistics(res, mask[lo:lo + k])
    _forward_in_eval_mode(dcn, rgb, mask, None, None, step, _aug.DEFAULT_IMAGE_MEAN, _aug.DEFAULT_IMAGE_STD_DEV, statistics)
    stats, used = combine_descriptor_statistics(out[0], out[1], n)
    # one transfer: the statistics, the number of images used and the gather's status word in one float64 block
    block = torch.cat([stats.double().view(-1), used.double(), bad_frame.double()]).cpu().numpy()
    if int(block[-1]) != 0:
        raise RuntimeError("dcn_hip: the frame gather rejected a frame index (status %d)" % int(block[-1]))
    if int(block[-2]) == 0:
        raise ValueError("every one of the %d chosen frames has an empty mask: no descriptor statistics" % n)
    table = block[:-2].reshape(2, 3, -1)
    out = {s: {f: [float(v) for v in table[i, j]] for j, f in enumerate(STAT_FIELDS)} for i, s in enumerate(STAT_SETS)}
    if save_to_file:
        import dense_correspondence_manipulation.utils.utils as utils
        utils.saveToYaml(out, filename)
    return out


# ---- curves: make_cdf_plot and compute_area_above_curve (evaluation.py:2658-2674, :2844-2863) ------------------------------
CURVE_FIELDS = ("pixel_match_error_l2", "pixel_match_error_l2_masked", "norm_diff_pred_3d", "norm_diff_pred_3d_masked",
                "norm_diff_descriptor_ground_truth", "fraction_pixels_closer_than_ground_truth",
                "fraction_pixels_closer_than_ground_truth_masked", "average_l2_distance_for_false_positives",
                "average_l2_distance_for_false_positives_masked")     # the nine columns the reference plots
CURVE_DROP_NAN = ("norm_diff_pred_3d", "norm_diff_pred_3d_masked")    # the two it dropna()s (make_descriptor_accuracy_plot)
CURVE_EMPTY, CURVE_NAN, CURVE_NONFINITE = 1, 2, 4                     # DCN_CURVE_*
CURVE_SUMMARY = ("count", "dropped", "min", "max", "lowerlimit", "binsize", "area_above_curve", "flags")
MAX_CURVES, MAX_CURVE_BINS = 64, 4096


class EvalCurves(collections.namedtuple("EvalCurves", "fields cumcount cdf summary status num_bins")):
    """``fields``: the curves' names, C of them; device tensors cumcount int64 [C, num_bins], cdf float64 [C, num_bins],
    summary float64 [C, 8] in the order of CURVE_SUMMARY, status int32 [1] (the OR of the curves' flags)."""


def cumulative_frequencies(values, row_pair=None, num_bins=100, drop_nan=False, out_summary=None, fields=None):
    """``scipy.stats.cumfreq(values[k], num_bins)`` times ``1.0 / len(values[k])`` and the area above it, for every row k of
    ``values`` (float64 [C, R] or [R]; C <= 64) in one launch (csrc/curve_kernels.hip, include/dcn_hip.h section 14).
    ``row_pair`` int32 [R]: rows with a negative entry do not belong to the table.  ``drop_nan``: a bool or one per curve
    (``dropna()``).  ``out_summary``: the contiguous float64 [C, 8] device tensor the kernel writes its summary to (a view
    into a larger tensor will do).  ``fields``: names for EvalCurves.fields (default 0 .. C - 1).  Nothing is read back."""
    if not torch.is_tensor(values) or values.dtype != torch.float64:
        raise TypeError("values must be a float64 tensor, got %s" % (values.dtype if torch.is_tensor(values) else
                                                                     type(values).__name__))
    if values.dim() == 1:
        values = values.view(1, -1)
    if values.dim() != 2:
        raise ValueError("values must be [C, R] or [R], got %s" % (tuple(values.shape),))
    C, R = int(values.shape[0]), int(values.shape[1])
    nb = int(num_bins)
    if not 1 <= C <= MAX_CURVES:
        raise ValueError("1 .. %d curves per call, got %d" % (MAX_CURVES, C))
    if not 2 <= nb <= MAX_CURVE_BINS:
        raise ValueError("num_bins must be 2 .. %d, got %d" % (MAX_CURVE_BINS, nb))
    if R > 0 and (values.stride(1) != 1 or (C > 1 and values.stride(0) < R)):
        values = values.contiguous()
    ld = int(values.stride(0)) if C > 1 and R > 0 else R
    dev = values.device
    if row_pair is not None:
        row_pair = _rows(row_pair, torch.int32, "row_pair", R)
        if row_pair.device != dev:
            raise ValueError("row_pair is on %s, values on %s" % (row_pair.device, dev))
    drops = [bool(drop_nan)] * C if isinstance(drop_nan, (bool, int, np.bool_)) else [bool(d) for d in drop_nan]
    if len(drops) != C:
        raise ValueError("drop_nan: one per curve (%d), got %d" % (C, len(drops)))
    names = tuple(range(C)) if fields is None else tuple(fields)
    if len(names) != C:
        raise ValueError("fields: one per curve (%d), got %d" % (C, len(names)))
    if out_summary is None:
        out_summary = torch.empty((C, len(CURVE_SUMMARY)), dtype=torch.float64, device=dev)
    elif out_summary.dtype != torch.float64 or tuple(out_summary.shape) != (C, len(CURVE_SUMMARY)) \
            or not out_summary.is_contiguous() or out_summary.device != dev:
        raise ValueError("out_summary must be a contiguous float64 [%d, %d] tensor on %s" % (C, len(CURVE_SUMMARY), dev))
    _lib.require_device(values, row_pair, out_summary)
    # (a bool tensor filled from the host: stream-ordered, no read)
    drop = torch.tensor(drops, dtype=torch.uint8).to(dev, non_blocking=True)
    cumcount = torch.empty((C, nb), dtype=torch.int64, device=dev)
    cdf = torch.empty((C, nb), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = _lib.get().dcn_eval_curves(C, R, ld, p(values) if R > 0 else None, p(row_pair), p(drop), nb, p(cumcount), p(cdf),
                                    p(out_summary), p(status), _lib.stream_ptr())
    _lib.check(rc, "dcn_eval_curves")
    return EvalCurves(names, cumcount, cdf, out_summary, status, nb)


def evaluation_curves(table, fields=None, num_bins=100, *, drop_nan=None, out_summary=None):
    """The curves of an evaluation table on the device.  ``table``: an EvalTable (same-scene, cross-scene, cross-instance or
    keypoints: the rows of ``columns`` named by ``fields``, default CURVE_FIELDS, NaNs dropped for the fields of
    CURVE_DROP_NAN) or an AcrossObjectTable (``norm_diff_descriptor_best_match``, converted to float64 on the device, no
    NaN dropped); ``row_pair`` selects the rows.  ``drop_nan`` overrides the per-field rule (``area_above_curve`` passes
    True).  ValueError for a field the table does not have.  -> EvalCurves; nothing is read back."""
    if isinstance(table, AcrossObjectTable):
        have = ("norm_diff_descriptor_best_match",)
        fields = have if fields is None else tuple(fields)
        rows = {have[0]: table.norm_diff_descriptor_best_match}
    elif isinstance(table, EvalTable):
        have = COLUMNS
        fields = CURVE_FIELDS if fields is None else tuple(fields)
        rows = None
    else:
        raise TypeError("table must be an EvalTable or an AcrossObjectTable, got %s" % type(table).__name__)
    unknown = [f for f in fields if f not in have]
    if unknown or not fields:
        raise ValueError("unknown field(s) %s: this table has %s" % (unknown, ", ".join(have)))
    if rows is None:
        values = torch.stack([table.columns[COLUMNS.index(f)] for f in fields])
        drops = [f in CURVE_DROP_NAN for f in fields]
    else:
        values = torch.stack([rows[f].double() for f in fields])
        drops = [False] * len(fields)
    if drop_nan is not None:
        drops = [bool(drop_nan)] * len(fields)
    return cumulative_frequencies(values, table.row_pair, num_bins, drops, out_summary, fields)


def _refused_range(mn, mx, num_bins):
    """numpy's message for the range scipy.stats.cumfreq derives from a minimum and a maximum that are not finite"""
    with np.errstate(all="ignore"):
        s = (np.float64(mx) - np.float64(mn)) / (2. * (num_bins - 1.))
        return "supplied range of [{}, {}] is not finite".format(np.float64(mn) - s, np.float64(mx) + s)


def curves_to_host(curves):
    """ONE copy to the host.  -> {field: {"x_axis": lowerlimit + binsize * arange(num_bins) (``make_cdf_plot``'s, before its
    cosmetic scale factor), "cdf", "cumcount", "count", "area_above_curve"}}.  Raises what the reference's call on that
    column would have raised: ValueError in numpy's words for a curve with a NaN (not dropped) or a value that is not finite,
    ZeroDivisionError for one without values."""
    C, nb = len(curves.fields), int(curves.num_bins)
    block = torch.cat([curves.cumcount.double().view(-1), curves.cdf.reshape(-1), curves.summary.reshape(-1)]).cpu().numpy()
    cumcount = block[:C * nb].reshape(C, nb).astype(np.int64)      # (counts below 2^53 are exact in float64)
    cdf = block[C * nb:2 * C * nb].reshape(C, nb)
    summary = block[2 * C * nb:].reshape(C, len(CURVE_SUMMARY))
    out = {}
    for k, field in enumerate(curves.fields):
        n, _, mn, mx, lowerlimit, binsize, area, flags = summary[k]
        flags = int(flags)
        if flags & CURVE_NAN:
            raise ValueError("%s: %s" % (field, _refused_range(np.nan, np.nan, nb)))
        if flags & CURVE_NONFINITE:
            raise ValueError("%s: %s" % (field, _refused_range(mn, mx, nb)))
        if flags & CURVE_EMPTY:
            raise ZeroDivisionError("%s: float division by zero (no value in this column)" % (field,))
        out[field] = {"x_axis": lowerlimit + binsize * np.arange(0, nb), "cdf": cdf[k].copy(), "cumcount": cumcount[k].copy(),
                      "count": int(n), "area_above_curve": float(area)}
    return out


def area_above_curve(table, field, num_bins=100):
    """``DenseCorrespondenceEvaluationPlotter.compute_area_above_curve(df, field, num_bins)`` (evaluation.py:2844-2863) on a
    device table: NaNs dropped whatever the field, as there.  One launch, one copy.  -> float."""
    return curves_to_host(evaluation_curves(table, (field,), num_bins, drop_nan=True))[field]["area_above_curve"]


def write_stats_yaml(table, output_dir):
    """What ``run_on_single_dataframe`` saves (evaluation.py:2953-2975): ``<output_dir>/stats.yaml`` with the one key
    ``norm_diff_3d_area_above_curve``.  -> the dict written."""
    import dense_correspondence_manipulation.utils.utils as utils
    d = {"norm_diff_3d_area_above_curve": float(area_above_curve(table, "norm_diff_pred_3d"))}
    os.makedirs(output_dir, exist_ok=True)
    utils.saveToYaml(d, os.path.join(output_dir, "stats.yaml"))
    return d
