"""Host side of the augmentation kernels (csrc/augment_kernels.hip): the data augmentation the reference applies to every
within-scene sample (dense_correspondence/dataset/spartan_dataset_masked.py:667-680) plus its ToTensor + Normalize (:297-304),
for a batch of device-resident image pairs in one launch.

Per image (a and b drawn independently), as correspondence_augmentation.py does it:
  * with probability 1/2 the background (mask == 0) is replaced (random_domain_randomize_background, :86-94): a solid colour or,
    with probability 1/2, a two-colour linear gradient (vertical with probability 1/2), colours uniform on 0..254
    (get_random_rgb, :148-153); then, with probability 1/2, +-50 uniform noise (add_noise, :201-215);
  * with probability 1/2 the image, its mask and its pixel lists are rotated by 180 degrees
    (random_image_and_indices_mutation, :19-56).
The decisions are drawn on the device (``torch.randint`` with the caller's generator) into one record of
``PARAM_WORDS`` int32 per image (layout: include/dcn_hip.h section 7); the noise itself comes from a counter-based hash keyed by
the record's seed, so a batch replays bit for bit from its ``params``.  Nothing here waits for the device.
"""
import collections

import numpy as np
import torch

from . import _args, _lib

PARAM_WORDS = 16
FLIP_V, FLIP_H, RANDOMIZE, GRADIENT, VERTICAL, NOISE = 1, 2, 4, 8, 16, 32
UV_INT64, UV_FLOAT32 = _args.UV_INT64, _args.UV_FLOAT32

DEFAULT_IMAGE_MEAN = [0.5573105812072754, 0.37420374155044556, 0.37020164728164673]   # constants.py:11-12
DEFAULT_IMAGE_STD_DEV = [0.24336038529872894, 0.2987397611141205, 0.31875079870224]

AugmentedPairs = collections.namedtuple("AugmentedPairs", "input_a input_b mask_a mask_b uv_a uv_b params rgb_a rgb_b")


def draw_params(num_images, device, generator=None, domain_randomize=True, flip=True):
    """[num_images, PARAM_WORDS] int32 records on ``device``: every decision with probability 1/2, colours uniform on 0..254
    (the distribution of ``uint8(U * 255)``), a random 64-bit noise seed.  A handful of small launches, no host sync."""
    kw = dict(device=device, generator=generator, dtype=torch.int32)
    bits = torch.randint(0, 2, (num_images, 5), **kw)               # randomize, gradient, vertical, noise, rotate
    colours = torch.randint(0, 255, (num_images, 6), **kw)
    seeds = torch.randint(-2 ** 31, 2 ** 31 - 1, (num_images, 2), **kw)
    rnd = bits[:, 0] * int(bool(domain_randomize))
    flags = rnd * (RANDOMIZE + bits[:, 1] * GRADIENT + bits[:, 1] * bits[:, 2] * VERTICAL + bits[:, 3] * NOISE)
    flags = flags + bits[:, 4] * int(bool(flip)) * (FLIP_V | FLIP_H)
    zeros = torch.zeros(num_images, 1, **{k: v for k, v in kw.items() if k != "generator"})
    return torch.cat([flags.view(-1, 1), colours, zeros, seeds, zeros.expand(num_images, 6)], dim=1).contiguous()


def flip_uv(uv, h, w, params=None, offsets=None, flags=FLIP_V | FLIP_H):
    """(u, v) -> ((w-1) - u, (h-1) - v) per the FLIP_H / FLIP_V bits of each entry's image (``params`` records, entries of image b
    at ``offsets[b]:offsets[b+1]``) or of ``flags``.  dtype kept (int64 / float32)."""
    if uv is None:
        return None
    lib = _lib.get()
    u, v = uv[0].contiguous(), uv[1].contiguous()
    if u.dtype != v.dtype or u.numel() != v.numel():
        raise ValueError("u and v must have the same dtype and length")
    _lib.require_device(u, v, params, offsets)
    uo, vo = torch.empty_like(u), torch.empty_like(v)
    n = 1 if offsets is None else int(offsets.numel()) - 1
    if n < 1 or (params is not None and (params.dtype != torch.int32 or params.dim() != 2 or params.shape[0] < n
                                         or params.shape[1] != PARAM_WORDS or not params.is_contiguous())):
        raise ValueError("flip_uv: offsets need >= 2 entries and params one contiguous int32 record per image")
    if offsets is not None and (offsets.dtype != torch.int64 or not offsets.is_contiguous()):
        raise ValueError("flip_uv: offsets must be a contiguous int64 tensor")
    rc = lib.dcn_flip_uv(_args.uv_dtype(u), _lib.ptr(u), _lib.ptr(v), _lib.ptr(uo), _lib.ptr(vo), u.numel(), n, _lib.ptr(offsets),
                         _lib.ptr(params), int(flags), int(h), int(w), _lib.stream_ptr())
    _lib.check(rc, "dcn_flip_uv")
    return uo, vo


def flip_planes(t, flip_v, flip_h, pixel_dims=1):
    """A flipped copy of ``t`` [..., H, W, <pixel>]: the last ``pixel_dims`` dims make up one pixel (1 for HWC images, 0 for
    [H, W] masks and depth maps), the dims before H are separate planes.  Any dtype (the kernel moves bytes)."""
    lib = _lib.get()
    t = t.contiguous()
    _lib.require_device(t)
    hd = t.dim() - pixel_dims - 2           # index of H
    if hd < 0:
        raise ValueError("need [..., H, W] + %d pixel dims, got shape %s" % (pixel_dims, tuple(t.shape)))
    h, w = int(t.shape[hd]), int(t.shape[hd + 1])
    planes = int(np.prod(t.shape[:hd], dtype=np.int64))
    bpp = t.element_size() * int(np.prod(t.shape[hd + 2:], dtype=np.int64))
    if t.numel() == 0 or not (flip_v or flip_h):
        return t.clone()
    out = torch.empty_like(t)
    rc = lib.dcn_flip_planes(_lib.ptr(t), _lib.ptr(out), planes, h, w, bpp, int(bool(flip_v)), int(bool(flip_h)),
                             _lib.stream_ptr())
    _lib.check(rc, "dcn_flip_planes")
    return out


def augment_images(rgb_a, mask_a, params, rgb_b=None, mask_b=None, noise=None, mean=DEFAULT_IMAGE_MEAN,
                   std=DEFAULT_IMAGE_STD_DEV, want_input=True, want_rgb=False, want_mask=True):
    """One ``dcn_augment_images`` launch over uint8 [N, H, W, 3] images and uint8 [N, H, W] masks of side a (and b).
    -> dict of the requested outputs: input_a/_b float [N, 3, H, W], rgb_a/_b uint8 [N, H, W, 3], mask_a/_b float [N, H, W]."""
    lib = _lib.get()
    sides = [("a", rgb_a, mask_a)] + ([("b", rgb_b, mask_b)] if rgb_b is not None else [])
    n, h, w = int(rgb_a.shape[0]), int(rgb_a.shape[1]), int(rgb_a.shape[2])
    args, out = {}, {}
    for s, rgb, mask in sides:
        rgb, mask = _args.image(rgb, n, h, w, "rgb_" + s), _args.mask(mask, n, h, w, "mask_" + s)
        _lib.require_device(rgb, mask)
        args["rgb_" + s], args["mask_" + s] = rgb, mask
        dev = rgb.device
        out["input_" + s] = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev) if want_input else None
        out["rgb_" + s] = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev) if want_rgb else None
        out["mask_" + s] = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_mask else None
    if params.dtype != torch.int32 or tuple(params.shape) != (len(sides) * n, PARAM_WORDS):
        raise ValueError("params must be int32 [%d, %d], got %s %s" % (len(sides) * n, PARAM_WORDS, params.dtype,
                                                                        tuple(params.shape)))
    params = params.contiguous()
    noise = None if noise is None else noise.contiguous()
    if noise is not None and (noise.dtype != torch.uint8 or tuple(noise.shape) != (len(sides) * n, h, w, 3)):
        raise ValueError("noise must be uint8 [%d, %d, %d, 3]" % (len(sides) * n, h, w))
    _lib.require_device(params, noise)
    g = lambda k: _lib.ptr(args.get(k))
    o = lambda k: _lib.ptr(out.get(k))
    m, sd = _args.mean_std(mean), _args.mean_std(std)
    rc = lib.dcn_augment_images(n, h, w, g("rgb_a"), g("rgb_b"), g("mask_a"), g("mask_b"), _lib.ptr(params),
                                _lib.ptr(noise), _lib.host_ptr(m), _lib.host_ptr(sd), o("input_a"),
                                o("input_b"), o("rgb_a"), o("rgb_b"), o("mask_a"), o("mask_b"), _lib.stream_ptr())
    _lib.check(rc, "dcn_augment_images")
    return out


def _offsets(offsets, n, dev):
    if offsets is None:
        if n != 1:
            raise ValueError("offsets [B + 1] are needed to split concatenated pixel lists over B = %d images" % n)
        return None
    return _args.offsets(offsets, n, dev)


def augment_image_pairs(rgb_a, rgb_b, mask_a, mask_b, uv_a=None, uv_b=None, offsets=None, *, domain_randomize=True,
                        flip=True, mean=DEFAULT_IMAGE_MEAN, std=DEFAULT_IMAGE_STD_DEV, generator=None, params=None,
                        return_rgb=False):
    """Augments B image pairs on the device and writes the network's inputs.

    rgb_a, rgb_b: uint8 [B, H, W, 3]; mask_a, mask_b: 0/1 [B, H, W] (uint8, or anything ``.to(uint8)`` maps onto 0/1);
    uv_a, uv_b: optional ``(u, v)`` pixel lists found on the unaugmented images, int64 or float32, the B images' lists
    concatenated with ``offsets`` [B + 1] (tensor or sequence; may be omitted for B = 1); ``params``: [2B, PARAM_WORDS] int32
    records (a's first) to replay, otherwise drawn with ``generator`` (``domain_randomize`` / ``flip`` switch the two steps).

    -> AugmentedPairs(input_a, input_b: float [B, 3, H, W] for ``dcn.forward`` / ``forward_pair``; mask_a, mask_b: the rotated
    masks as float 0/1 [B, H, W] (what ``pairgen.mask_nonzero`` takes); uv_a, uv_b: the rotated lists (dtype kept, None if not
    given); params; rgb_a, rgb_b: the augmented uint8 images when ``return_rgb``, else None).
    One augmentation launch plus one per pixel list; no host synchronization."""
    n = int(rgb_a.shape[0])
    dev = rgb_a.device
    if params is None:
        params = draw_params(2 * n, dev, generator=generator, domain_randomize=domain_randomize, flip=flip)
    else:
        params = params.to(device=dev, dtype=torch.int32, non_blocking=True)
    out = augment_images(rgb_a, mask_a, params, rgb_b=rgb_b, mask_b=mask_b, mean=mean, std=std, want_rgb=return_rgb)
    h, w = int(rgb_a.shape[1]), int(rgb_a.shape[2])
    off = _offsets(offsets, n, dev) if (uv_a is not None or uv_b is not None) else None
    ua = flip_uv(uv_a, h, w, params=params[:n], offsets=off)
    ub = flip_uv(uv_b, h, w, params=params[n:], offsets=off)
    return AugmentedPairs(out["input_a"], out["input_b"], out["mask_a"], out["mask_b"], ua, ub, params, out["rgb_a"],
                          out["rgb_b"])
