"""Host side of the merge kernels (csrc/merge_kernels.hip): the SYNTHETIC_MULTI_OBJECT sample of the reference
(dense_correspondence/dataset/spartan_dataset_masked.py:890-960) for a batch of device-resident samples.

Per sample, objects a and b each bring two frames (images, 0/1 masks) and a match list between them.  Frame 1 and frame 2
each paste one object over the other (object b in front with probability 1/2, independently per frame), as
correspondence_augmentation.merge_images_with_occlusions does; every match of the object behind that falls inside the front
object's mask is dropped (prune_matches_if_occluded, frame 1's pair first, then frame 2's swapped pair), and the kept lists are
concatenated, object a's first (merge_matches).  A sample in which every match of a or of b is occluded is empty, as the
reference returns an empty sample then.  The foreground decisions are drawn on the device with the caller's generator into
``[B, 2]`` int32 records (1 = object b in front), or replayed.  Nothing here waits for the device.
"""
import collections

import torch

from . import _args, _lib
from .augment import DEFAULT_IMAGE_MEAN, DEFAULT_IMAGE_STD_DEV

FG_A, FG_B = 0, 1
DROP_EMPTY = 1
BAD_INDEX, BAD_OFFSETS = 1, 2

MergedSamples = collections.namedtuple(
    "MergedSamples", "input_1 input_2 mask_1 mask_2 uv_1 uv_2 offsets empty status foreground rgb_1 rgb_2")


def draw_foreground(num_samples, device, generator=None):
    """[num_samples, 2] int32 records on ``device``: frame 1's and frame 2's front object, FG_B with probability 1/2."""
    return torch.randint(0, 2, (num_samples, 2), device=device, generator=generator, dtype=torch.int32)


def _mask(t, n, h, w, what):
    return None if t is None else _args.mask(t, n, h, w, what)


def _foreground(fg, n, dev):
    fg = torch.as_tensor(fg)
    if tuple(fg.shape) != (n, 2):
        raise ValueError("foreground must be [%d, 2] records, got %s" % (n, tuple(fg.shape)))
    return fg.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()


def merge_images(rgb_a, rgb_b, mask_a, mask_b, foreground, frames=1, mean=DEFAULT_IMAGE_MEAN, std=DEFAULT_IMAGE_STD_DEV,
                 want_input=True, want_mask=True, want_rgb=False):
    """One ``dcn_merge_images`` launch.  rgb_a / rgb_b / mask_a / mask_b: one tensor per frame each (sequences of ``frames``
    tensors), uint8 [N, H, W, 3] images and 0/1 [N, H, W] masks; foreground [N, 2] int32 device records.
    -> dict of lists per frame: input float [N, 3, H, W], mask float [N, H, W], rgb uint8 [N, H, W, 3] (None if not wanted)."""
    lib = _lib.get()
    n, h, w = int(rgb_a[0].shape[0]), int(rgb_a[0].shape[1]), int(rgb_a[0].shape[2])
    if frames not in (1, 2) or not all(len(x) == frames for x in (rgb_a, rgb_b, mask_a, mask_b)):
        raise ValueError("merge_images: 1 or 2 frames, one image and mask per object and frame")
    ia = [_args.image(t, n, h, w, "rgb_a") for t in rgb_a]
    ib = [_args.image(t, n, h, w, "rgb_b") for t in rgb_b]
    ma = [_mask(t, n, h, w, "mask_a") for t in mask_a]
    mb = [_mask(t, n, h, w, "mask_b") for t in mask_b]
    if foreground.dtype != torch.int32 or tuple(foreground.shape) != (n, 2) or not foreground.is_contiguous():
        raise ValueError("foreground must be a contiguous int32 [%d, 2] tensor" % n)
    _lib.require_device(*ia, *ib, *ma, *mb, foreground)
    dev = ia[0].device
    out = {"input": [torch.empty(n, 3, h, w, dtype=torch.float32, device=dev) if want_input else None for _ in range(frames)],
           "mask": [torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_mask else None for _ in range(frames)],
           "rgb": [torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev) if want_rgb else None for _ in range(frames)]}
    f2 = lambda lst: _lib.ptr(lst[1]) if frames == 2 else None
    m, sd = _args.mean_std(mean), _args.mean_std(std)
    rc = lib.dcn_merge_images(n, frames, h, w, _lib.ptr(foreground), _lib.ptr(ia[0]), _lib.ptr(ib[0]), f2(ia), f2(ib),
                              _lib.ptr(ma[0]), _lib.ptr(mb[0]), f2(ma), f2(mb), _lib.host_ptr(m), _lib.host_ptr(sd),
                              _lib.ptr(out["input"][0]), f2(out["input"]), _lib.ptr(out["mask"][0]), f2(out["mask"]),
                              _lib.ptr(out["rgb"][0]), f2(out["rgb"]), _lib.stream_ptr())
    _lib.check(rc, "dcn_merge_images")
    return out


def _list(uv, what):
    """(u, v) int64 -> two contiguous tensors."""
    u, v = uv
    if u.dtype != torch.int64 or v.dtype != torch.int64 or u.dim() != 1 or u.shape != v.shape:
        raise ValueError("%s must be two int64 [N] tensors of one length, got %s %s / %s %s"
                         % (what, u.dtype, tuple(u.shape), v.dtype, tuple(v.shape)))
    return u.contiguous(), v.contiguous()


def prune_and_concat(h, w, foreground, list_a, list_b, masks, drop_empty=True):
    """One ``dcn_merge_prune`` call (two launches).  list_a / list_b: (uv_1, uv_2, offsets, count) with uv_f = (u, v) int64
    device tensors; masks: {(frame, object): uint8 [N, H, W] or None} with frame 1 / 2 and object "a" / "b".
    -> (uv_1, uv_2, offsets, empty, status): outputs of capacity count_a + count_b (tail -1), see include/dcn_hip.h section 8."""
    lib = _lib.get()
    n = int(foreground.shape[0])
    dev = foreground.device
    args = []
    for uv1, uv2, off, cnt in (list_a, list_b):
        u1, v1 = _list(uv1, "uv_1")
        u2, v2 = _list(uv2, "uv_2")
        if u1.numel() != cnt or u2.numel() != cnt:
            raise ValueError("a match pair needs two lists of one length")
        _lib.require_device(u1, v1, u2, v2, off)
        args += [_lib.ptr(u1), _lib.ptr(v1), _lib.ptr(u2), _lib.ptr(v2), _lib.ptr(off), int(cnt)]
    cap = int(list_a[3]) + int(list_b[3])
    ws = torch.empty(int(lib.dcn_merge_prune_workspace(n, int(list_a[3]), int(list_b[3]))), dtype=torch.uint8, device=dev)
    uv = torch.empty(4, cap, dtype=torch.int64, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    empty = torch.empty(n, dtype=torch.bool, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    mk = [masks.get(k) for k in ((1, "a"), (1, "b"), (2, "a"), (2, "b"))]
    _lib.require_device(foreground, *mk)
    rc = lib.dcn_merge_prune(n, int(h), int(w), _lib.ptr(foreground), *[_lib.ptr(m) for m in mk], *args,
                             DROP_EMPTY if drop_empty else 0, _lib.ptr(uv[0]), _lib.ptr(uv[1]), _lib.ptr(uv[2]),
                             _lib.ptr(uv[3]), _lib.ptr(offsets), _lib.ptr(empty), _lib.ptr(status), _lib.ptr(ws),
                             _lib.stream_ptr())
    _lib.check(rc, "dcn_merge_prune")
    return (uv[0], uv[1]), (uv[2], uv[3]), offsets, empty, status


def merge_synthetic_samples(rgb_a1, rgb_a2, rgb_b1, rgb_b2, mask_a1, mask_a2, mask_b1, mask_b2, uv_a1, uv_a2, uv_b1, uv_b2,
                            offsets_a, offsets_b, *, mean=DEFAULT_IMAGE_MEAN, std=DEFAULT_IMAGE_STD_DEV, generator=None,
                            foreground=None, return_rgb=False):
    """Builds B synthetic multi-object samples on the device and writes the network's inputs.

    rgb_*: uint8 [B, H, W, 3] images of object a / b in frame 1 / 2; mask_*: 0/1 [B, H, W] (uint8, or anything ``.to(uint8)``
    maps onto 0/1); uv_a1, uv_a2: object a's matches between its frames 1 and 2, ``(u, v)`` int64, the B samples' lists
    concatenated with ``offsets_a`` [B + 1] (tensor or sequence); uv_b1, uv_b2, offsets_b likewise.  ``foreground``: [B, 2]
    records (FG_A / FG_B per frame) to replay, otherwise drawn with ``generator``.

    -> MergedSamples(input_1, input_2: float [B, 3, H, W] for ``dcn.forward`` / ``forward_pair``; mask_1, mask_2: the merged
    masks as float 0/1 [B, H, W] (what ``pairgen.mask_nonzero`` takes); uv_1, uv_2: the concatenated kept matches
    (``merge_matches(uv_a1, uv_b1)`` / ``(uv_a2, uv_b2)`` per sample), int64 of capacity len(uv_a1) + len(uv_b1) with sample
    s at ``offsets[s]:offsets[s+1]`` and -1 after ``offsets[B]``; offsets int64 [B + 1]; empty bool [B] (a sample whose a or
    b matches were all occluded: no entries); status int32 [1] (BAD_INDEX: an entry outside the image, dropped; BAD_OFFSETS);
    foreground; rgb_1, rgb_2: the merged uint8 images when ``return_rgb``, else None).
    One merge launch plus two prune launches; no host synchronization."""
    n, h, w = int(rgb_a1.shape[0]), int(rgb_a1.shape[1]), int(rgb_a1.shape[2])
    dev = rgb_a1.device
    if foreground is None:
        foreground = draw_foreground(n, dev, generator=generator)
    else:
        foreground = _foreground(foreground, n, dev)
    masks = [_mask(t, n, h, w, k) for t, k in ((mask_a1, "mask_a1"), (mask_a2, "mask_a2"), (mask_b1, "mask_b1"),
                                                (mask_b2, "mask_b2"))]
    ma1, ma2, mb1, mb2 = masks
    out = merge_images([rgb_a1, rgb_a2], [rgb_b1, rgb_b2], [ma1, ma2], [mb1, mb2], foreground, frames=2, mean=mean, std=std,
                       want_rgb=return_rgb)
    la = (uv_a1, uv_a2, _args.offsets(offsets_a, n, dev, "offsets_a"), int(uv_a1[0].numel()))
    lb = (uv_b1, uv_b2, _args.offsets(offsets_b, n, dev, "offsets_b"), int(uv_b1[0].numel()))
    uv_1, uv_2, offsets, empty, status = prune_and_concat(
        h, w, foreground, la, lb, {(1, "a"): ma1, (1, "b"): mb1, (2, "a"): ma2, (2, "b"): mb2})
    return MergedSamples(out["input"][0], out["input"][1], out["mask"][0], out["mask"][1], uv_1, uv_2, offsets, empty, status,
                         foreground, out["rgb"][0], out["rgb"][1])
