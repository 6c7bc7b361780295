"""The class-consistent keypoint table (the wide statistics kernel of csrc/crossscene_kernels.hip):
``evaluate_network_cross_scene_keypoints`` (evaluation.py:407-472, :1433-1552, :2413-2462)."""
import collections
import os

import numpy as np
import torch

from .. import augment as _aug
from ._chain import (COLUMNS, _camera_rows_of, _columns_to_dict, _dataframe, _empty_table, _image_index, _nan_table,
                     _py2_round, _queries_of_frames, _table_block, _uploader, _yaml_file)
from .cross_scene import _search_rows_by_frame, match_statistics_groups, match_statistics_groups_wide

KeypointLabels = collections.namedtuple("KeypointLabels", "images names uv object_ids size skipped")
KEYPOINT_ROW_COLUMNS = ("combination", "keypoint", "order", "frame_1", "frame_2", "u_1", "v_1", "u_2", "v_2", "k_frame")
KEYPOINT_COLUMNS = ("img_a_idx", "img_b_idx", "scene_name_a", "scene_name_b", "object_id_a", "object_id_b", "keypoint_name")
STANDARD, REVERSE = 0, 1                      # a row's order in keypoint_rows' table
WIDE_GROUP_MIN_ROWS = 24                      # evaluate_keypoint_rows(search=None): mean rows per searched image from which
#                                               the wide entry is used.  Measured (profiles/keypoint_bench_crossover.json, 8
#                                               images of 640x480): at 21 rows the two entries tie (1.29x at D = 3, 0.96x at
#                                               D = 16), at 28 the wide one wins at both (1.66x, 1.25x), at 14 it loses


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
    up = _uploader(dev)
    comb, fa, fb, kf = v[:, 0], v[:, 3], v[:, 4], v[:, 9]
    u_a, v_a = up(v[:, 5]), up(v[:, 6])
    u_b, v_b = up(v[:, 7].astype(np.float32)), up(v[:, 8].astype(np.float32))
    keep = torch.ones(T, dtype=torch.uint8, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    ncomb = int(comb.max()) + 1
    offsets = up(np.searchsorted(comb, np.arange(ncomb + 1)).astype(np.int64))
    # 1. one forward pass per distinct labelled frame
    frames = np.unique(np.concatenate([fa, fb]))
    queries, images, bad = _queries_of_frames(dcn, store, frames, np.searchsorted(frames, fa), np.arange(T), u_a, v_a, T,
                                              batch_frames, mean, std, keep_images_within=max_search_bytes)
    word = word | bad
    depth_q = store.depth[up(fa), v_a, u_a]
    # 2. camera rows: pose 1 and pose 2^-1 of the row's frames, K and K^-1 of the combination's first image
    cams, bad = _camera_rows_of(store, v[:, 3:5], np.ones(T, bool))
    of_k, bad_k = _camera_rows_of(store, np.stack([kf, kf], axis=1), np.ones(T, bool))
    cams[:, :18] = of_k[:, :18]
    word = word | bad | bad_k
    # 3. the rows by the frame they search
    if search is None:
        search = "wide" if T >= WIDE_GROUP_MIN_ROWS * len(np.unique(fb)) else "groups"
    out = _nan_table(T, offsets, word, u_a, v_a, u_b, v_b, dev)
    word =_search_rows_by_frame(dcn, store, out, word, fb, np.arange(T), comb, queries, depth_q, cams, keep, int(batch_frames),
                                 int(max_search_bytes), mean, std,
                                 match_statistics_groups_wide if search == "wide" else match_statistics_groups,
                                 resident=(frames, images) if images is not None else None)
    return out._replace(status=word.to(torch.int32))


def keypoint_table(store, labels, rows, t):
    """evaluate_keypoint_rows' EvalTable ``t`` (over ``rows``) as the reference's table, with ONE copy to the host: a dict of
    numpy columns under the reference's column names (COLUMNS as float64, ``is_valid`` / ``is_valid_masked`` as bool) plus
    KEYPOINT_COLUMNS by the row's order (evaluation.py:1541-1547): ``img_a_idx`` / ``scene_name_a`` / ``object_id_a`` of the
    image the query comes from, ``..._b`` of the image searched, and ``keypoint_name``.  RuntimeError when the chain's status
    word is not zero."""
    import itertools
    rows = _keypoint_rows_table(store, rows)
    block, _, word = _table_block([t.columns, t.is_valid.double()], None, t.status)      # (every row stays)
    if word:
        raise RuntimeError("dcn_hip: the keypoint evaluation failed on the device (status %d)" % word)
    table = _columns_to_dict(block)
    combos = np.asarray(list(itertools.combinations(range(labels.images.shape[0]), 2)), np.int64).reshape(-1, 2)
    pair = combos[rows[:, 0]]                                                   # (first image, second image) per row
    table["keypoint_name"] = np.array([labels.names[i][k] for i, k in zip(pair[:, 0], rows[:, 1])], dtype=object)
    reverse = rows[:, 2] == REVERSE
    for side, image in (("a", np.where(reverse, pair[:, 1], pair[:, 0])), ("b", np.where(reverse, pair[:, 0], pair[:, 1]))):
        table["scene_name_" + side], table["img_%s_idx" % side] = _image_index(store, labels.images[image, 2])
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
        table = _empty_table(names)
    else:
        table = keypoint_table(store, labels, rows, evaluate_keypoint_rows(dcn, store, labels, rows))
    df = _dataframe(table, names)
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
