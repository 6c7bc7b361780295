"""The across-object table (csrc/acrossobj_kernels.hip): ``evaluate_network_across_objects`` (evaluation.py:305-337)."""
import collections

import numpy as np
import torch

from .. import _args, _lib
from .. import augment as _aug
from ._chain import (BAD_FRAME, TOO_FEW_MASK_PIXELS, _below, _dataframe, _descriptor_images, _forward_pairs, _frame_pairs,
                     _image_index, _offsets_arg, _on_device, _queries_arg, _table_block, _valid_pointers)

ACROSS_OBJECT_COLUMNS = ("scene_name_a", "scene_name_b", "img_a_idx", "img_b_idx", "object_id_a", "object_id_b",
                         "norm_diff_descriptor_best_match")   # DCNEvaluationPandaTemplateAcrossObject.columns


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
    q, off = _queries_arg(queries, d), _offsets_arg(offsets, P, "P")
    _on_device(rb, q, off)
    dev = rb.device
    R = int(q.shape[0])
    cap = max(R, 1)
    q, = _valid_pointers(R, q)
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
    res_a, res_b, _, mask, _, status = _forward_pairs(dcn, store, _object_pairs(store, pairs), ("rgb", "mask"), batch_pairs,
                                                      mean, std)
    q =across_object_queries(mask[0], res_a, num_uv_a_samples, generator=generator, sample_order=sample_order)
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
        # one transfer: the distances, the rows' pairs and the status word
        block, _, word = _table_block([t.norm_diff_descriptor_best_match.double()], t.row_pair, t.status)
        if word & TOO_FEW_MASK_PIXELS:
            raise ValueError("Sample larger than population")
        if word:
            raise RuntimeError("dcn_hip: the across-object evaluation failed on the device (status %d)" % word)
        norm, pair = block[0].astype(np.float32), block[1].astype(np.int64)
    table = {"norm_diff_descriptor_best_match": norm}
    picked = chosen[pair]
    for side, (o, f) in (("a", (0, 4)), ("b", (1, 5))):
        table["scene_name_" + side], index = _image_index(store, picked[:, f])
        table["object_id_" + side] = np.array([store.object_ids[i] for i in picked[:, o]], dtype=object)
        table["img_%s_idx" % side] = index
    return table, _dataframe(table, ACROSS_OBJECT_COLUMNS)
