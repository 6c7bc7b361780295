"""Qualitative evaluation (csrc/picture_kernels.hip): ``evaluate_network_qualitative`` (evaluation.py:1979-2070), the descriptor
pictures of ``plot_descriptor_colormaps`` (:530-601) with the three normalisations of evaluation/plotting.py:5-87, and the
distance heat map of ``compute_gaussian_kernel_heatmap_from_norm_diffs`` (utils/visualization.py:8-33).  Nothing OpenCV draws
is here: no drawMatches, reticles, blending, ``applyColorMap`` table or gray conversion.

Deviations: masks count as 0 / 1 (the dataset's masks are); a one-channel picture is the plane itself (the reference's D = 1
figure goes through matplotlib's autoscaled colormap) -- colour it with ``colour_table`` if wanted; the byte of a NaN pixel is
0 and not pinned to matplotlib's."""
import collections
import ctypes
import os

import numpy as np
import torch

from .. import _args, _lib
from .. import augment as _aug
from ._chain import (BAD_FRAME, _below, _descriptor_images, _forward_pairs, _frame_pairs, _image_index, _lots, _offsets_arg,
                     _on_device, _queries_arg, _random_scene, _valid_pointers)
from .across_objects import across_object_queries, best_match_pairs
from .cross_scene import _different_pose

EMPTY_RANGE = 1                         # DCN_PICTURE_EMPTY_RANGE
NORM_NONE, NORM_PAIR, NORM_MASKED_PAIR, NORM_STATS, NORM_STATS_MASKED, NORM_SCALAR = range(6)   # DCN_NORM_*
HEATMAP_KERNEL_VARIANCE = 0.25          # kernel_variance of config/dense_correspondence/heatmap_vis/heatmap.yaml
QUALITATIVE_COLUMNS = ("scene_name_a", "scene_name_b", "img_a_idx", "img_b_idx", "u_a", "v_a", "u_b", "v_b", "norm_diff")

Ranges = collections.namedtuple("Ranges", "image pair scalar status")


class Normalized(collections.namedtuple("Normalized", "normed picture ranges status")):
    """Device tensors.  normed: the normalised image(s) (float32; float64 with a stats dict) or None; picture: uint8
    [.., H, W, 3] (one plane [.., H, W] for D = 1) or None; ranges: the ``Ranges`` used (None with a stats dict); status int32
    [P]: EMPTY_RANGE for a pair whose masked non-zero set is empty in some channel (the reference raises ValueError there)."""


def _images(res, what, like=None):
    r, P, h, w, d = _descriptor_images(res, what)
    if like is not None and tuple(like.shape) != tuple(r.shape):
        raise ValueError("%s must have the shape of the other image, %s, got %s" % (what, tuple(like.shape), tuple(r.shape)))
    return r, P, h, w, d


def _mask(m, P, h, w, what):
    if not torch.is_tensor(m) or m.dtype not in (torch.uint8, torch.bool):
        raise ValueError("%s must be a uint8 (or bool) tensor" % what)
    return _args.mask(m, P, h, w, what)


def _same_device(*tensors):
    _on_device(*tensors)
    devs = set(t.device for t in tensors if t is not None)
    if len(devs) > 1:
        raise ValueError("all tensors must be on one device, got %s" % sorted(str(d) for d in devs))


def _want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(x not in ("normed", "picture") for x in want):
        raise ValueError("want must name 'normed' and / or 'picture', got %r" % (want,))
    return "normed" in want, "picture" in want


def _channels(d, channels):
    """-> the image channels a picture shows: all three for D = 3, the one for D = 1, otherwise ``channels`` = (i, j, k)"""
    if channels is None:
        if d not in (1, 3):
            raise ValueError("a picture of a %d-channel descriptor image needs channels=(i, j, k)" % d)
        return tuple(range(d))
    ch = tuple(int(c) for c in channels)
    if len(ch) != 3 or min(ch) < 0 or max(ch) >= d:
        raise ValueError("channels must be three of 0 .. %d, got %r" % (d - 1, channels))
    return ch


def _stats_rows(stats, d, dev):
    """A stats dict {'min': [...], 'max': [...]} -> float64 [2, D] on ``dev``"""
    try:
        rows = np.stack([np.asarray(stats["min"], np.float64).reshape(-1), np.asarray(stats["max"], np.float64).reshape(-1)])
    except (KeyError, TypeError, ValueError):
        raise ValueError("stats must be a dict with per-channel 'min' and 'max'")
    if rows.shape != (2, d):
        raise ValueError("stats must hold %d values per field, got %s" % (d, rows.shape[1:]))
    return torch.from_numpy(rows).to(dev)


def descriptor_ranges(res_a, res_b=None, mask_a=None, mask_b=None):
    """The ranges the reference's normalisations take, for P pairs (or P single images) with every image read once.

    -> Ranges: image float32 [2, P, 4, D] (a's, b's; min, max over the image, min, max over the non-zero products x * m as
    plotting.py:59-75 forms them: zeros under the mask are skipped, a non-finite value outside it poisons the range); pair
    float32 [P, 4, D], the two combined by Python's min / max (a NaN in image a stays, one in b alone is dropped); scalar
    float32 [2, P, 2], ``res.min()``, ``res.max()``; status int32 [P] (EMPTY_RANGE).  Without ``res_b`` side 1 is not
    written.  No host synchronization."""
    lib = _lib.get()
    ra, P, h, w, d = _images(res_a, "res_a")
    rb = None if res_b is None else _images(res_b, "res_b", ra)[0]
    if (mask_a is None) != (mask_b is None) and rb is not None:
        raise ValueError("give both masks or neither")
    ma = None if mask_a is None else _mask(mask_a, P, h, w, "mask_a")
    mb = None if mask_b is None or rb is None else _mask(mask_b, P, h, w, "mask_b")
    _same_device(ra, rb, ma, mb)
    dev = ra.device
    image = torch.full((2, P, 4, d), float("nan"), dtype=torch.float32, device=dev)
    pair = torch.empty((P, 4, d), dtype=torch.float32, device=dev)
    scalar = torch.full((2, P, 2), float("nan"), dtype=torch.float32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, int(lib.dcn_descriptor_ranges_workspace(P, h, w, d))), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_descriptor_ranges(P, h, w, d, p(ra), p(rb), p(ma), p(mb), p(image), p(pair), p(scalar), p(status), p(ws),
                                   _lib.stream_ptr())
    _lib.check(rc, "dcn_descriptor_ranges")
    return Ranges(image, pair, scalar, status)


def _normalize(ra, rb, ma, mb, ranges, families):
    """One ``dcn_descriptor_normalize`` launch.  families: up to two of (mode, stats rows or None, want_normed, picture tensor or
    None with its (side stride, pair stride) in bytes, channels) -> [(normed or None, picture or None)]"""
    lib = _lib.get()
    P, h, w, d = (int(x) for x in ra.shape)
    dev = ra.device
    sides = 1 if rb is None else 2
    fams = (_lib.PictureFamily * 2)()
    out, keep = [], []
    for i, (mode, stats, want_normed, picture, strides, channels) in enumerate(families):
        f = fams[i]
        f.mode = mode
        normed = None
        if want_normed:
            normed = torch.empty((sides, P, h, w, d), dtype=torch.float64 if stats is not None else torch.float32, device=dev)
            f.normed = normed.data_ptr()
        if picture is not None:
            f.picture = picture.data_ptr()
            f.picture_channels = len(channels)
            for j, c in enumerate(channels):
                f.channel[j] = c
            f.side_stride, f.pair_stride = strides
        if stats is not None:
            f.stats = stats.data_ptr()
            keep.append(stats)
        out.append((normed, picture))
    p = _lib.ptr
    rc = lib.dcn_descriptor_normalize(P, h, w, d, p(ra), p(rb), p(ma), p(mb), p(None if ranges is None else ranges.pair),
                                      p(None if ranges is None else ranges.scalar), ctypes.byref(fams), _lib.stream_ptr())
    _lib.check(rc, "dcn_descriptor_normalize")
    return out


def _own_picture(sides, P, h, w, channels, dev):
    """A picture tensor [sides, P, H, W(, 3)] of its own and its strides"""
    n = h * w * len(channels)
    pic = torch.empty((sides, P, h, w) + ((3,) if len(channels) == 3 else ()), dtype=torch.uint8, device=dev)
    return pic, (P * n, n)


def _one_family(ra, rb, ma, mb, ranges, mode, stats, want, channels, status):
    want_normed, want_picture = _want(want)
    P, h, w, d = (int(x) for x in ra.shape)
    ch = _channels(d, channels) if want_picture else None
    sides = 1 if rb is None else 2
    pic, strides = _own_picture(sides, P, h, w, ch, ra.device) if want_picture else (None, None)
    (normed, pic), = _normalize(ra, rb, ma, mb, ranges, [(mode, stats, want_normed, pic, strides, ch)])
    if rb is None:
        normed, pic = (None if normed is None else normed[0]), (None if pic is None else pic[0])
    return Normalized(normed, pic, ranges, status)


def normalize_descriptor(res, stats=None, *, mask=None, want=("normed",), channels=None):
    """``normalize_descriptor(res, stats)`` (plotting.py:5-26) for a batch ``res`` float32 [P, H, W, D].

    stats None: float32 throughout with the image's own scalar range, ``(res - res.min()) / ((res.max() - res.min()) + eps)``
    as numpy >= 2 evaluates that text.  stats a dict with per-channel 'min' and 'max': numpy promotes to float64 --
    ``clip(double(res), min, max)``, then ``(v - min) / ((max - min) + 1e-10)``; ``normed`` is float64.  With ``mask`` (uint8
    [P, H, W]; needs stats) the input is ``res * mask`` and the result is multiplied by the mask again, the lower row of
    ``plot_descriptor_colormaps`` (evaluation.py:585-598).
    want: "normed" and / or "picture"; channels: the (i, j, k) a picture shows when D is neither 1 nor 3.
    -> Normalized, normed [P, H, W, D], picture [P, H, W, 3] (or [P, H, W] for D = 1).  No host synchronization."""
    r, P, h, w, d = _images(res, "res")
    _want(want)
    if mask is not None and stats is None:
        raise ValueError("a mask needs a stats dict")
    m = None if mask is None else _mask(mask, P, h, w, "mask")
    _same_device(r, m)
    status = torch.zeros(P, dtype=torch.int32, device=r.device)
    if stats is None:
        ranges = descriptor_ranges(r)
        return _one_family(r, None, None, None, ranges, NORM_SCALAR, None, want, channels, status)
    rows = _stats_rows(stats, d, r.device)
    return _one_family(r, None, m, None, None, NORM_STATS if m is None else NORM_STATS_MASKED, rows, want, channels, status)


def normalize_descriptor_pair(res_a, res_b, *, want=("normed",), channels=None):
    """``normalize_descriptor_pair`` (plotting.py:28-50) for P pairs: per channel ``(x - both_min) / (both_max - both_min)`` in
    float32, the pair's range as Python's ``min`` / ``max`` of the two images' give it.  A constant channel gives 0 / 0 = NaN, as
    in the reference.  -> Normalized with normed float32 [2 (a, b), P, H, W, D], picture [2, P, H, W, 3] (or [2, P, H, W])."""
    ra, P, h, w, d = _images(res_a, "res_a")
    rb = _images(res_b, "res_b", ra)[0]
    _want(want)
    _same_device(ra, rb)
    ranges = descriptor_ranges(ra, rb)
    return _one_family(ra, rb, None, None, ranges, NORM_PAIR, None, want, channels,
                       torch.zeros(P, dtype=torch.int32, device=ra.device))


def normalize_masked_descriptor_pair(res_a, res_b, mask_a, mask_b, *, want=("normed",), channels=None):
    """``normalize_masked_descriptor_pair`` (plotting.py:52-87) for P pairs: the pair's range over the non-zero products
    ``res * mask`` per channel, ``(x - both_min) / (both_max - both_min)`` times the mask, in float32.  status carries
    EMPTY_RANGE for a pair with an image whose non-zero set is empty in some channel (``pictures_to_host`` raises the
    reference's ValueError for it).  -> Normalized, shapes as ``normalize_descriptor_pair``."""
    ra, P, h, w, d = _images(res_a, "res_a")
    rb = _images(res_b, "res_b", ra)[0]
    _want(want)
    ma, mb = _mask(mask_a, P, h, w, "mask_a"), _mask(mask_b, P, h, w, "mask_b")
    _same_device(ra, rb, ma, mb)
    ranges = descriptor_ranges(ra, rb, ma, mb)
    return _one_family(ra, rb, ma, mb, ranges, NORM_MASKED_PAIR, None, want, channels, ranges.status)


DescriptorPictures = collections.namedtuple("DescriptorPictures", "pictures ranges status")


def descriptor_pictures(res_a, res_b, mask_a, mask_b, descriptor_image_stats=None, descriptor_norm_type="mask_image", *,
                        channels=None):
    """The four pictures of ``plot_descriptor_colormaps(res_a, res_b, descriptor_image_stats, mask_a, mask_b, plot_masked=True,
    descriptor_norm_type)`` (evaluation.py:530-601) for P pairs, as the bytes ``imshow`` displays.

    Without ``descriptor_image_stats``: the upper row by ``normalize_descriptor_pair``, the lower by
    ``normalize_masked_descriptor_pair``.  With it (the dict of ``descriptor_statistics.yaml``): the upper row by
    ``normalize_descriptor`` with ``stats[descriptor_norm_type]``, the lower on ``res * mask`` with ``stats['mask_image']``, times
    the mask -- as the reference chooses.  One ranges launch (none with stats) and one normalise launch: each image is read
    twice in total.
    -> DescriptorPictures: pictures uint8 [P, 2 (full, masked), 2 (a, b), H, W, 3] ([P, 2, 2, H, W] for D = 1); ranges (None
    with stats); status int32 [P] (EMPTY_RANGE).  No host synchronization."""
    ra, P, h, w, d = _images(res_a, "res_a")
    rb = _images(res_b, "res_b", ra)[0]
    ma, mb = _mask(mask_a, P, h, w, "mask_a"), _mask(mask_b, P, h, w, "mask_b")
    _same_device(ra, rb, ma, mb)
    ch = _channels(d, channels)
    dev = ra.device
    n = h * w * len(ch)
    pictures = torch.empty((P, 2, 2, h, w) + ((3,) if len(ch) == 3 else ()), dtype=torch.uint8, device=dev)
    strides = (n, 4 * n)                                    # (side, pair) in bytes
    flat = pictures.view(-1)
    if descriptor_image_stats is None:
        ranges = descriptor_ranges(ra, rb, ma, mb)
        fams = [(NORM_PAIR, None, False, flat, strides, ch), (NORM_MASKED_PAIR, None, False, flat[2 * n:], strides, ch)]
        status = ranges.status
    else:
        if descriptor_norm_type not in descriptor_image_stats or "mask_image" not in descriptor_image_stats:
            raise ValueError("descriptor_image_stats must hold %r and 'mask_image'" % (descriptor_norm_type,))
        ranges = None
        fams = [(NORM_STATS, _stats_rows(descriptor_image_stats[descriptor_norm_type], d, dev), False, flat, strides, ch),
                (NORM_STATS_MASKED, _stats_rows(descriptor_image_stats["mask_image"], d, dev), False, flat[2 * n:], strides, ch)]
        status = torch.zeros(P, dtype=torch.int32, device=dev)
    _normalize(ra, rb, ma, mb, ranges, fams)
    return DescriptorPictures(pictures, ranges, status)


HeatMaps = collections.namedtuple("HeatMaps", "maps status")


def heat_maps(res_b, queries, offsets, variance=HEATMAP_KERNEL_VARIANCE, colour_table=None):
    """``compute_gaussian_kernel_heatmap_from_norm_diffs(norm_diffs, variance)`` (utils/visualization.py:27-31, up to the
    ``applyColorMap`` line) for R query descriptors against the images of P pairs, with each image read once.

    res_b: float32 [P, H, W, D]; queries float32 [R, D]; offsets int64 [P + 1] device tensor, pair p's rows at
    offsets[p]:offsets[p+1], exactly as ``best_match_pairs``.  The plane is ``uint8(exp(-d / float32(variance)) * 255)``, d the
    float32 distance ``find_best_matches(..., return_norm_diffs=True)`` returns, quotient and product in float32, the
    exponential taken in float64 from the float32 quotient and rounded once (numpy's float32 ``exp`` is another implementation
    and differs by one level on about one byte in a million).  colour_table: uint8 [256, 3] (``colour_table()``) gives
    ``table[plane]``, written directly.
    -> HeatMaps: maps uint8 [R, H, W] (or [R, H, W, 3]); rows from offsets[P] on are left UNTOUCHED (uninitialised memory);
    status int32 [1] (BAD_OFFSETS).  Bit-identical from run to run.  No host synchronization."""
    lib = _lib.get()
    rb, P, h, w, d = _descriptor_images(res_b, "res_b")
    q, off = _queries_arg(queries, d), _offsets_arg(offsets, P, "P")
    var = float(variance)
    if not np.float32(var) > 0:
        raise ValueError("variance must be positive, got %r" % (variance,))
    table = None
    if colour_table is not None:
        if not torch.is_tensor(colour_table) or colour_table.dtype != torch.uint8 or tuple(colour_table.shape) != (256, 3):
            raise ValueError("colour_table must be a uint8 [256, 3] tensor")
        table = colour_table.contiguous()
    _same_device(rb, q, off, table)
    dev = rb.device
    R = int(q.shape[0])
    q, = _valid_pointers(R, q)
    maps = torch.empty((max(R, 1), h, w) + ((3,) if table is not None else ()), dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(2048, dtype=torch.uint8, device=dev)   # DCN_HEAT_WORKSPACE_BYTES
    p = _lib.ptr
    rc = lib.dcn_heat_maps(P, h, w, d, p(rb), p(q), p(off), max(R, 1), var, p(table), p(maps), p(status), p(ws),
                           _lib.stream_ptr())
    _lib.check(rc, "dcn_heat_maps")
    return HeatMaps(maps[:R], status)


_tables = {}


def colour_table(name="jet"):
    """256 x 3 bytes of MATPLOTLIB's colormap ``name`` (``uint8(cmap(i / 255)[:3] * 255)`` through its own ``bytes=True``), a
    uint8 [256, 3] host tensor, computed once.  This is matplotlib's table and NOT OpenCV's: ``cv2.applyColorMap(...,
    COLORMAP_JET)``, which the reference's heat map uses, has its own (and BGR order).  Move it to the device for
    ``heat_maps``."""
    if name not in _tables:
        import matplotlib
        cmap = matplotlib.colormaps[name]
        _tables[name] = torch.from_numpy(np.ascontiguousarray(cmap(np.arange(256), bytes=True)[:, :3].astype(np.uint8)))
    return _tables[name]


def pictures_to_host(result):
    """ONE copy of a ``Normalized`` / ``DescriptorPictures`` / ``HeatMaps`` / ``QualitativeResult`` to the host -> the same
    named tuple of numpy arrays (None stays None, host values stay).  ValueError, the reference's from ``np.min`` of an empty
    array, for a pair flagged EMPTY_RANGE; RuntimeError for any other status."""
    fields = result._asdict()
    tensors = {}

    def collect(prefix, value):
        if torch.is_tensor(value):
            tensors[prefix] = value
        elif isinstance(value, tuple) and hasattr(value, "_asdict"):
            for k, v in value._asdict().items():
                collect(prefix + (k,), v)
    for k, v in fields.items():
        collect((k,), v)
    names = [k for k in tensors if tensors[k].is_cuda]
    if names:                                               # one transfer: every tensor as bytes in one block
        parts = [tensors[k].contiguous().view(-1).view(torch.uint8) for k in names]
        block = torch.cat(parts).cpu()
        at = 0
        for k, part in zip(names, parts):
            t = tensors[k]
            tensors[k] = block[at:at + part.numel()].clone().view(t.dtype).view(t.shape)
            at += part.numel()

    def rebuild(prefix, value):
        if torch.is_tensor(value):
            return tensors[prefix].numpy()
        if isinstance(value, tuple) and hasattr(value, "_asdict"):
            return type(value)(**{k: rebuild(prefix + (k,), v) for k, v in value._asdict().items()})
        return value
    out = type(result)(**{k: rebuild((k,), v) for k, v in fields.items()})
    status = np.asarray(out.status).reshape(-1)
    if isinstance(result, HeatMaps):
        if status.any():
            raise RuntimeError("dcn_hip: the heat maps' row lists were rejected on the device (status %d)" % int(status[0]))
        return out
    bad = np.nonzero(status & EMPTY_RANGE)[0]
    if len(bad):
        raise ValueError("zero-size array to reduction operation minimum which has no identity (pair %s: no non-zero "
                         "descriptor under a mask)" % ", ".join(str(int(b)) for b in bad))
    word = getattr(out, "chain_status", None)
    if word is not None and int(np.asarray(word).reshape(-1)[0]):
        raise RuntimeError("dcn_hip: the qualitative evaluation failed on the device (status %d)"
                           % int(np.asarray(word).reshape(-1)[0]))
    return out


def choose_qualitative_pairs(store, num_image_pairs=5, host_rng=None, one_scene=False):
    """``get_random_scenes_and_image_pairs`` (evaluation.py:1950-1976) and, with ``one_scene``, ``get_random_image_pairs``
    (:1925-1947), on the host: a scene by ``get_random_scene_name`` (per pair, or once), image a uniform over its frames, image b
    by ``get_img_idx_with_different_pose(scene, pose_a, num_attempts=100)``; a pair without a b is dropped.  The reference
    draws 5 pairs.  As in ``choose_pairs`` the rule is replayed, not the reference's random stream.
    -> int64 array [n, 3] of (scene, frame a, frame b), frames as store indices; n <= num_image_pairs."""
    rng = host_rng if host_rng is not None else np.random
    first, poses = store.scene_first_frame_host, store.poses_host
    lots = _lots(store)
    out = []
    s = _random_scene(store, rng, lots) if one_scene else None
    for _ in range(int(num_image_pairs)):
        if not one_scene:
            s = _random_scene(store, rng, lots)
        lo, cnt = first[s], first[s + 1] - first[s]
        a = lo + _below(rng, cnt)
        b = _different_pose(poses, lo, cnt, a, rng, 0.2, 20, 100)    # (the defaults of get_img_idx_with_different_pose)
        if b >= 0:
            out.append((s, a, b))
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


class QualitativeResult(collections.namedtuple(
        "QualitativeResult", "pictures heat_maps u_a v_a best_uv norm_diff offsets pairs status chain_status")):
    """Device tensors but ``pairs``.  pictures uint8 [P, 2 (full, masked), 2 (a, b), H, W, 3]; heat_maps uint8 [R, H, W] over
    image b or None; u_a, v_a int64 [R] the sampled pixels of image a; best_uv int32 [2, R] (u, v) and norm_diff float32 [R]
    their best matches in image b; pair p's rows at offsets[p]:offsets[p+1] (offsets int64 [P + 1]; -1 / NaN after
    offsets[P]); pairs: the host array [P, 3] of (scene, frame a, frame b); status int32 [P] (EMPTY_RANGE); chain_status int32
    [1]: the sampling's, the search's, the heat maps' and the gather's status words."""


def _stats_of(dcn):
    try:                                                    # (evaluation.py:1395-1400)
        return dcn.descriptor_image_stats
    except Exception:
        return None


def evaluate_network_qualitative(dcn, store, num_image_pairs=5, num_matches=10, *, pairs=None, host_rng=None, generator=None,
                                 sample_order=None, heat_variance=None, save_to=None, batch_pairs=8,
                                 mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV):
    """``evaluate_network_qualitative(dcn, dataset, num_image_pairs, randomize=True)`` (evaluation.py:1979-2070) with
    ``single_image_pair_qualitative_analysis`` (:1347-1430) per pair, on a frame store: 1. choose_qualitative_pairs (or
    ``pairs``: [P, 2] store frame indices (a, b) or [P, 3] with the scene first), 2. the frames gathered and the network run in
    eval mode, ``batch_pairs`` pairs at a time, 3. ``across_object_queries(mask_a, res_a, num_matches)`` --
    ``random_sample_from_masked_image``, with its ``sample_order`` replay --, 4. ``best_match_pairs`` over image b, 5.
    ``descriptor_pictures`` with ``dcn.descriptor_image_stats`` when that file exists, otherwise the pair normalisations, 6. with
    ``heat_variance`` the heat maps of the sampled rows over image b.  -> QualitativeResult, everything on the device.
    ``save_to``: a directory; one copy to the host, then ``<k>_a_full.png``, ``<k>_b_full.png``, ``<k>_a_masked.png``,
    ``<k>_b_masked.png`` per pair k (PIL) and ``matches.csv`` with QUALITATIVE_COLUMNS.  ``dcn.training`` is left as found.
    ValueError when no draw found an image b with a different pose (the reference would show nothing)."""
    chosen = choose_qualitative_pairs(store, num_image_pairs, host_rng) if pairs is None else np.asarray(
        pairs.cpu() if torch.is_tensor(pairs) else pairs)
    if chosen.shape[0] == 0:
        raise ValueError("no image pair with a different pose was found")
    fr = _frame_pairs(store, chosen)
    if chosen.shape[1] == 2:                                # the scene of frame a
        first = np.asarray(store.scene_first_frame_host, np.int64)
        chosen = np.concatenate([(np.searchsorted(first, fr[:, :1], side="right") - 1), fr], axis=1)
    res_a, res_b, _, mask, _, gathered = _forward_pairs(dcn, store, fr, ("rgb", "mask"), batch_pairs, mean, std)
    q = across_object_queries(mask[0], res_a, num_matches, generator=generator, sample_order=sample_order)
    m = best_match_pairs(res_b, q.queries, q.offsets, max_pair_rows=int(num_matches))
    pics = descriptor_pictures(res_a, res_b, mask[0], mask[1], _stats_of(dcn))
    word = q.status | m.status | (gathered & 1) * BAD_FRAME
    heat = None
    if heat_variance is not None:
        hm = heat_maps(res_b, q.queries, q.offsets, heat_variance)
        heat, word = hm.maps, word | hm.status
    result = QualitativeResult(pics.pictures, heat, q.u_a, q.v_a, m.best_uv, m.norm_diff_descriptor_best_match, q.offsets,
                               chosen.astype(np.int64), pics.status, word.to(torch.int32))
    if save_to is not None:
        save_qualitative(store, result, save_to)
    return result


def save_qualitative(store, result, directory):
    """``pictures_to_host``, then the PNGs and ``matches.csv`` of ``evaluate_network_qualitative`` into ``directory``
    -> the host copy"""
    from PIL import Image
    host = pictures_to_host(result)
    os.makedirs(directory, exist_ok=True)
    for k in range(host.pictures.shape[0]):
        for i, kind in enumerate(("full", "masked")):
            for j, side in enumerate("ab"):
                Image.fromarray(host.pictures[k, i, j]).save(os.path.join(directory, "%d_%s_%s.png" % (k, side, kind)))
    names_a, idx_a = _image_index(store, host.pairs[:, 1])
    names_b, idx_b = _image_index(store, host.pairs[:, 2])
    off = host.offsets
    with open(os.path.join(directory, "matches.csv"), "w") as f:
        f.write(",".join(QUALITATIVE_COLUMNS) + "\n")
        for p in range(host.pairs.shape[0]):
            for r in range(int(off[p]), int(off[p + 1])):
                f.write("%s,%s,%d,%d,%d,%d,%d,%d,%r\n" % (names_a[p], names_b[p], idx_a[p], idx_b[p], host.u_a[r], host.v_a[r],
                                                        host.best_uv[0, r], host.best_uv[1, r], float(host.norm_diff[r])))
    return host
