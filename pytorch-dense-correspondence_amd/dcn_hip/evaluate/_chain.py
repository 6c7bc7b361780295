"""The steps the evaluation tables share: the table's layout and status bits, the argument checks of the statistics entries,
the scene and frame draws, the frame gathers, the forward pass in eval mode and the host tail of a table."""
import collections

import numpy as np
import torch

from .. import _lib
from .. import augment as _aug
from ..frames import gather_frames

COLUMNS = ("norm_diff_descriptor_ground_truth", "norm_diff_descriptor", "norm_diff_descriptor_masked",
           "norm_diff_ground_truth_3d", "norm_diff_pred_3d", "norm_diff_pred_3d_masked", "pixel_match_error_l2",
           "pixel_match_error_l2_masked", "pixel_match_error_l1", "fraction_pixels_closer_than_ground_truth",
           "fraction_pixels_closer_than_ground_truth_masked", "average_l2_distance_for_false_positives",
           "average_l2_distance_for_false_positives_masked")
BAD_INDEX, BAD_OFFSETS, BAD_DRAWS, BAD_FRAME, TOO_FEW_MASK_PIXELS = 1, 2, 4, 8, 16


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


def _forward_pairs(dcn, store, fr, want, batch_pairs, mean, std):
    """The first steps of evaluate_frame_pairs and evaluate_object_pairs for the host table ``fr`` (int [P, 2] store frame
    indices (a, b); P <= 1024): ``dcn_gather_frames`` of the planes ``want``, then ``_forward_in_eval_mode`` over the pairs,
    ``batch_pairs`` at a time.  -> (res_a, res_b float32 [P, H, W, D], depth, mask, cams, status) -- the planes as
    ``_gather_host_frames`` returns them, [2, P, ...]."""
    P = int(fr.shape[0])
    if P > 1024:
        raise ValueError("at most 1024 pairs per call, got %d" % P)
    if int(batch_pairs) < 1:
        raise ValueError("batch_pairs must be >= 1")
    rgb, depth, mask, cams, status = _gather_host_frames(store, fr, want)
    res = [[], []]

    def keep(lo, n, y):
        res[0].append(y[:n])
        res[1].append(y[n:])
    _forward_in_eval_mode(dcn, rgb[0], mask[0], rgb[1], mask[1], int(batch_pairs), mean, std, keep)
    return torch.cat(res[0]).contiguous(), torch.cat(res[1]).contiguous(), depth, mask, cams, status


def _uploader(dev):
    """host array -> tensor on ``dev``"""
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _queries_of_frames(dcn, store, frames, slot_of_row, rows, u_a, v_a, T, batch_frames, mean, std, keep_images_within=None):
    """The query descriptors of evaluate_cross_scene_rows and evaluate_keypoint_rows: ONE forward pass per frame of the sorted
    host list ``frames``, ``batch_frames`` at a time, keeping after each batch the descriptors at (u_a, v_a) of the table rows
    ``rows`` (host indices into the T rows), row i's frame being ``frames[slot_of_row[i]]`` -- and the descriptor images
    themselves when all of them fit in ``keep_images_within`` bytes.
    -> (queries float32 [T, D], zero for the other rows; images float32 [len(frames), H, W, D] or None; the gather's BAD_FRAME
    status word)"""
    dev, h, w = store.device, store.h, store.w
    up = _uploader(dev)
    by_slot = np.argsort(slot_of_row, kind="stable")
    a_rows, a_local = up(rows[by_slot]), up(slot_of_row[by_slot])
    a_bounds = np.searchsorted(slot_of_row[by_slot], np.arange(len(frames) + 1))
    rgb, _, mask, bad = _gather_frame_list(store, frames, ("rgb", "mask"))
    bad = (bad & 1) * BAD_FRAME
    queries, images = [], []

    def take(lo, n, res):
        if not queries:
            queries.append(torch.zeros((T, int(res.shape[3])), dtype=torch.float32, device=dev))
            if keep_images_within is not None and len(frames) * h * w * int(res.shape[3]) * 4 <= int(keep_images_within):
                images.append(torch.empty((len(frames), h, w, int(res.shape[3])), dtype=torch.float32, device=dev))
        at = a_rows[a_bounds[lo]:a_bounds[lo + n]]
        queries[0][at] = res[a_local[a_bounds[lo]:a_bounds[lo + n]] - lo, v_a[at], u_a[at]].float()
        if images:                                           # every image stays
            images[0][lo:lo + n] = res
    _forward_in_eval_mode(dcn, rgb, mask, None, None, int(batch_frames), mean, std, take)
    return queries[0], images[0] if images else None, bad


def _nan_table(T, offsets, word, u_a, v_a, u_b, v_b, dev):
    """An EvalTable of T rows without a result (NaN, 0, -1 like rows past the end) for the searches to fill"""
    return EvalTable(
        torch.full((len(COLUMNS), T), float("nan"), dtype=torch.float64, device=dev),
        torch.zeros((2, T), dtype=torch.uint8, device=dev), torch.full((4, T), -1, dtype=torch.int32, device=dev),
        torch.zeros((2, T), dtype=torch.int32, device=dev), torch.full((T,), -1, dtype=torch.int32, device=dev), offsets,
        torch.zeros(T, dtype=torch.int32, device=dev), word, u_a, v_a, u_b, v_b)


def _descriptor_dimension(d):
    if d < 1 or d > 64:
        raise ValueError("descriptor dimension must be 1 .. 64, got %d" % d)


def _descriptor_images(res, what, max_images=1024):
    if not torch.is_tensor(res) or res.dim() != 4:
        raise ValueError("%s must be a [P, H, W, D] tensor" % what)
    if res.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (what, res.dtype))
    P, h, w, d = (int(x) for x in res.shape)
    _descriptor_dimension(d)
    if P < 1 or P > max_images or h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError("%s must hold 1 .. %d images of 1 <= H * W < 2^31 pixels, got %s" % (what, max_images,
                                                                                            tuple(res.shape)))
    return res.contiguous(), P, h, w, d


def _on_device(*tensors):
    try:
        _lib.require_device(*tensors)
    except RuntimeError as e:
        raise ValueError(str(e))


def _offsets_arg(offsets, count, letter):
    """The row lists of ``count`` pairs (``letter`` "P") or groups ("G"): int64 [count + 1] -> contiguous and flat"""
    if not torch.is_tensor(offsets) or offsets.dtype != torch.int64 or int(offsets.numel()) != count + 1:
        raise ValueError("offsets must be an int64 tensor of %s + 1 = %d entries" % (letter, count + 1))
    return offsets.contiguous().view(-1)


def _queries_arg(queries, d):
    if not torch.is_tensor(queries) or queries.dtype != torch.float32 or queries.dim() != 2 or int(queries.shape[1]) != d:
        raise ValueError("queries must be float32 [R, %d]" % d)
    return queries.contiguous()


def _valid_pointers(R, *per_row):
    """No rows at all (R == 0): the kernels still want valid pointers -> one zero row in place of each empty tensor"""
    if R:
        return per_row
    return tuple(torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in per_row)


def _alloc_eval_table(cap, groups, dev, workspace_bytes):
    """The outputs of a statistics entry for ``cap`` rows of ``groups`` pairs or groups, in the entry's argument order: columns,
    is_valid, pred_uv, closer, row_pair, mask_pixels, status, workspace"""
    return (torch.empty((len(COLUMNS), cap), dtype=torch.float64, device=dev),
            torch.empty((2, cap), dtype=torch.uint8, device=dev), torch.empty((4, cap), dtype=torch.int32, device=dev),
            torch.empty((2, cap), dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
            torch.empty(groups, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
            torch.empty(int(workspace_bytes), dtype=torch.uint8, device=dev))


def _eval_table_of(outs, R, offsets, u_a, v_a, u_b, v_b):
    """``_alloc_eval_table``'s outputs cut to the R rows given, as an EvalTable"""
    cols, valid, pred, closer, row_pair, mask_pixels, status, _ = outs
    return EvalTable(cols[:, :R], valid[:, :R], pred[:, :R], closer[:, :R], row_pair[:R], offsets, mask_pixels, status,
                     u_a, v_a, u_b, v_b)


# ---- the host tail of a table ---------------------------------------------------------------------------------------------
def _table_block(rows, row_pair=None, status=None):
    """ONE copy to the host: the device tensors ``rows`` (float64 [k, R] or [R]), then ``row_pair`` and the ``status`` word
    where given, packed into one float64 block (ints up to 2^31 are exact).
    -> (block: the rows of ``rows``, then row_pair, cut to the table's rows -- those with row_pair >= 0 (rows without a result
    and rows past the last one carry -1), all of them without ``row_pair``; the indices of those rows; the status word, 0
    without ``status``)"""
    parts = [r if r.dim() == 2 else r.view(1, -1) for r in rows]
    R = int(parts[0].shape[1])
    if row_pair is not None:
        parts.append(row_pair.double().view(1, R))
    if status is not None:
        parts.append(status.double().expand(R).view(1, R))
    block = torch.cat(parts).cpu().numpy()
    word = 0
    if status is not None:
        word = int(block[-1, 0]) if R else 0
        block = block[:-1]
    at = np.arange(R) if row_pair is None else np.nonzero(block[-1] >= 0)[0]
    return block[:, at], at, word


def _columns_to_dict(block):
    """The first rows of a host block -- COLUMNS, is_valid, is_valid_masked -- under the reference's column names"""
    table = {k: block[i].copy() for i, k in enumerate(COLUMNS)}
    table["is_valid"] = block[len(COLUMNS)] != 0
    table["is_valid_masked"] = block[len(COLUMNS) + 1] != 0
    return table


def _image_index(store, frames):
    """Store frame indices (host) -> (their scenes' names, objects; the dataset's image indices ``store.frame_ids`` gives
    them, int64)"""
    first = np.asarray(store.scene_first_frame_host, np.int64)
    frames = np.asarray(frames, np.int64)
    scene = np.searchsorted(first, frames, side="right") - 1
    return (np.array([store.scene_names[s] for s in scene], dtype=object),
            np.array([int(store.frame_ids[s][f - first[s]]) for s, f in zip(scene, frames)], dtype=np.int64))


def _empty_table(names):
    """A table without rows: COLUMNS as float64, the validity flags as bool, image indices as int64, the rest as objects"""
    kind = lambda k: np.float64 if k in COLUMNS else bool if k.startswith("is_valid") else np.int64 if k.startswith("img_") \
        else object
    return {k: np.zeros(0, kind(k)) for k in names}


def _dataframe(table, names):
    """A ``pandas.DataFrame`` of ``table`` with the columns in the order of ``names`` when pandas imports, else None"""
    assert set(table) == set(names)
    try:
        import pandas
    except ImportError:
        return None
    return pandas.DataFrame({k: table[k] for k in names})


def _py2_round(x):
    """Python 2's ``round``: half away from zero"""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def _gather_frame_list(store, frames, want):
    """``_gather_host_frames`` of a host LIST of n frames: they travel as the two slots of (n + 1) // 2 pairs (an odd n repeats
    the last frame), so that the [2, P] planes, flattened, are the n frames in order -> (rgb, depth, mask, status)"""
    n = len(frames)
    P = (n + 1) // 2
    fr = np.concatenate([frames, frames[-1:]])[:2 * P].reshape(2, P).T
    rgb, depth, mask, _, status = _gather_host_frames(store, fr, want)
    flat = lambda t, tail: None if t is None else t.view((2 * P, store.h, store.w) + tail)[:n]
    return flat(rgb, (3,)), flat(depth, ()), flat(mask, ()), status


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


def _yaml_file(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)
