"""MI355X mirror of ``dense_correspondence/correspondence_tools/correspondence_augmentation.py``: the augmentation every
within-scene sample goes through (``spartan_dataset_masked.py:667-680``), same names and semantics, for DEVICE tensors.

* Image tensors (HWC: uint8 RGB [H, W, 3], masks / depth maps [H, W] of any dtype, which is kept) take the device path
  (csrc/augment_kernels.hip).  It consumes Python's ``random`` and ``numpy.random`` in exactly the reference's order -- each
  ``random.random()`` decision, each ``np.random.uniform(size=3)`` colour, the ``np.random.uniform()`` gradient direction and
  the two full-size noise planes, drawn on the host and uploaded as one (n1 - n2) mod 256 plane -- so that after
  ``random.seed(s); np.random.seed(s)`` its output is byte-identical to the reference's and both streams are left in the same
  state.  Masks are 0 / 1 (the reference's uint8 formula rgb*m + (1-m)*bg is applied to other values too, but they are
  outside the contract).
* PIL images and numpy arrays -- the reference's CPU loader -- go unchanged to the reference's own module (behind this source
  root, dcn_hip/_dropin.py), and raise with the reason when it does not import.
* ``merge_images_with_occlusions``, ``prune_matches_if_occluded`` and ``merge_matches`` (the SYNTHETIC_MULTI_OBJECT sample,
  ``spartan_dataset_masked.py:890-960``) take image tensors the same way (csrc/merge_kernels.hip): one ``random.random()`` per
  merge, a uint8 tensor where the reference returns a PIL image or a numpy array, ``(None, None)`` when every match is
  occluded (one host read of the kept count), ``IndexError`` for a match outside the image.
* Every other name (``get_random_image`` ...) is handed on to the reference's module.

The batched paths that write the network's inputs for a whole batch in one launch are ``dcn_hip.augment.augment_image_pairs``
and ``dcn_hip.merge.merge_synthetic_samples``.
"""
import random

import numpy as np
import torch

from dcn_hip import augment as _aug
from dcn_hip import merge as _merge
from dcn_hip._dropin import reference_sibling as _reference_sibling

_ref = _reference_sibling(__name__, __file__)


def __getattr__(name):
    return _ref.attr(name)


def _reference(name):
    ref = _ref.get()
    if ref is None:
        raise TypeError("correspondence_augmentation.%s: this module takes image TENSORS (device path); PIL images and numpy "
                        "arrays go to the reference's own module, which is not available here (%s)" % (name, _ref.why_not()))
    return getattr(ref, name)


def _tensors(images):
    return all(torch.is_tensor(im) for im in images)


def _flip(images, uv_pixel_positions, flip_v, flip_h):
    out = [_aug.flip_planes(im, flip_v, flip_h, pixel_dims=im.dim() - 2) for im in images]
    if uv_pixel_positions is None:
        return out, None
    last = images[-1]            # the reference reads the size of the list's LAST image (see flip_vertical)
    h, w = int(last.shape[0]), int(last.shape[1])
    dev = last.device
    uv = (torch.as_tensor(uv_pixel_positions[0], device=dev), torch.as_tensor(uv_pixel_positions[1], device=dev))
    flags = (_aug.FLIP_V if flip_v else 0) | (_aug.FLIP_H if flip_h else 0)
    return out, _aug.flip_uv(uv, h, w, flags=flags)


def random_image_and_indices_mutation(images, uv_pixel_positions):
    """:19-56.  With probability 1/2 (one ``random.random()``) the images and the (u, v) lists come back as they are, otherwise
    rotated by 180 degrees (flip_vertical then flip_horizontal, done as one flip per image)."""
    if not _tensors(images):
        return _reference("random_image_and_indices_mutation")(images, uv_pixel_positions)
    if random.random() < 0.5:
        return images, uv_pixel_positions
    return _flip(images, uv_pixel_positions, True, True)


def flip_vertical(images, uv_pixel_positions):
    """:59-69.  v -> (H-1) - v with H the height of the LAST image of the list: the reference reads ``image.height`` from its
    list comprehension's variable, which Python 2 leaks (Python 3 raises NameError there)."""
    if not _tensors(images):
        return _reference("flip_vertical")(images, uv_pixel_positions)
    return _flip(images, uv_pixel_positions, True, False)


def flip_horizontal(images, uv_pixel_positions):
    """:72-83.  u -> (W-1) - u, W of the last image (as flip_vertical)."""
    if not _tensors(images):
        return _reference("flip_horizontal")(images, uv_pixel_positions)
    return _flip(images, uv_pixel_positions, False, True)


def random_domain_randomize_background(image_rgb, image_mask):
    """:86-94.  One ``random.random()``: below 1/2 the image comes back as it is."""
    if not torch.is_tensor(image_rgb):
        return _reference("random_domain_randomize_background")(image_rgb, image_mask)
    if random.random() < 0.5:
        return image_rgb
    return domain_randomize_background(image_rgb, image_mask)


def _random_rgb():
    return np.array(np.random.uniform(size=3) * 255, dtype=np.uint8)        # get_random_rgb, :148-153


def domain_randomize_background(image_rgb, image_mask):
    """:96-123 with get_random_image (:125-146): every pixel whose mask is 0 gets the random background.  uint8 [H, W, 3] in,
    uint8 [H, W, 3] out (the reference returns a PIL image of the same bytes)."""
    if not torch.is_tensor(image_rgb):
        return _reference("domain_randomize_background")(image_rgb, image_mask)
    if image_rgb.dim() != 3 or image_rgb.shape[2] != 3 or image_rgb.dtype != torch.uint8:
        raise ValueError("image_rgb must be a uint8 [H, W, 3] tensor, got %s %s" % (image_rgb.dtype, tuple(image_rgb.shape)))
    h, w = int(image_rgb.shape[0]), int(image_rgb.shape[1])
    dev = image_rgb.device
    mask = image_mask if torch.is_tensor(image_mask) else torch.as_tensor(np.asarray(image_mask))
    flags = _aug.RANDOMIZE
    rgb2 = np.zeros(3, dtype=np.uint8)
    if random.random() < 0.5:                                                 # :135-142
        rgb1 = _random_rgb()
    else:
        rgb1 = _random_rgb()
        rgb2 = _random_rgb()
        flags |= _aug.GRADIENT | (_aug.VERTICAL if bool(np.random.uniform() > 0.5) else 0)
    noise = None
    if not random.random() < 0.5:                                             # :143-146, add_noise :201-215
        n1 = np.array(np.random.uniform(size=(h, w, 3)) * 50, dtype=np.uint8)
        n2 = np.array(np.random.uniform(size=(h, w, 3)) * 50, dtype=np.uint8)
        noise = torch.from_numpy(n1 - n2).to(dev).view(1, h, w, 3)            # (uint8: wraps, as the reference's sum)
        flags |= _aug.NOISE
    rec = np.zeros((1, _aug.PARAM_WORDS), dtype=np.int32)
    rec[0, 0] = flags
    rec[0, 1:4] = rgb1
    rec[0, 4:7] = rgb2
    out = _aug.augment_images(image_rgb.view(1, h, w, 3), mask.to(dev).reshape(1, h, w),
                              torch.from_numpy(rec).to(dev), noise=noise, want_input=False, want_rgb=True, want_mask=False)
    return out["rgb_a"][0]


def merge_images_with_occlusions(image_a, image_b, mask_a, mask_b, matches_pair_a, matches_pair_b):
    """:217-297.  One ``random.random()``: below 1/2 object b is in front, otherwise a.  uint8 [H, W, 3] images and 0/1 [H, W]
    masks in; -> (merged uint8 [H, W, 3], merged mask uint8 [H, W] = clip(mask_a + mask_b, 0, 1), matches_a,
    associated_matches_a, matches_b, associated_matches_b): the front object's pair as given, the other's pruned by the front
    mask (``(None, None)`` when nothing stays)."""
    if not torch.is_tensor(image_a):
        return _reference("merge_images_with_occlusions")(image_a, image_b, mask_a, mask_b, matches_pair_a, matches_pair_b)
    front_b = random.random() < 0.5
    if image_a.dim() != 3 or image_a.shape[2] != 3 or image_a.dtype != torch.uint8:
        raise ValueError("images must be uint8 [H, W, 3] tensors, got %s %s" % (image_a.dtype, tuple(image_a.shape)))
    h, w = int(image_a.shape[0]), int(image_a.shape[1])
    dev = image_a.device
    masks = [(m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m))).to(dev).reshape(1, h, w) for m in (mask_a, mask_b)]
    fg = torch.tensor([[_merge.FG_B if front_b else _merge.FG_A, _merge.FG_A]], dtype=torch.int32).to(dev)
    out = _merge.merge_images([image_a.reshape(1, h, w, 3)], [image_b.reshape(1, h, w, 3)], [masks[0]], [masks[1]], fg,
                              frames=1, want_input=False, want_rgb=True)
    merged_mask = out["mask"][0][0].to(torch.uint8)
    if front_b:
        back = prune_matches_if_occluded(masks[1][0], matches_pair_a)
        pair_a, pair_b = back, matches_pair_b
    else:
        back = prune_matches_if_occluded(masks[0][0], matches_pair_b)
        pair_a, pair_b = matches_pair_a, back
    return out["rgb"][0][0], merged_mask, pair_a[0], pair_a[1], pair_b[0], pair_b[1]


def prune_matches_if_occluded(foreground_mask_numpy, background_matches_pair):
    """:300-335.  Entry i of both lists of the pair stays when ``foreground_mask[v_i, u_i] == 0`` for the FIRST list's (u, v);
    order is kept.  int64 lists; ``(None, None)`` when nothing stays (one host read), IndexError for an entry of the first list
    outside the mask (negative ones included: numpy would wrap them)."""
    if not torch.is_tensor(foreground_mask_numpy):
        return _reference("prune_matches_if_occluded")(foreground_mask_numpy, background_matches_pair)
    mask = foreground_mask_numpy
    if mask.dim() != 2:
        raise ValueError("the foreground mask must be [H, W], got %s" % (tuple(mask.shape),))
    h, w = int(mask.shape[0]), int(mask.shape[1])
    dev = mask.device
    first, second = background_matches_pair
    n = int(first[0].numel())
    mask = (mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)).contiguous().view(1, h, w)
    none = torch.empty(0, dtype=torch.int64, device=dev)
    fg = torch.tensor([[_merge.FG_B, _merge.FG_A]], dtype=torch.int32).to(dev)
    off = torch.tensor([0, n], dtype=torch.int64).to(dev)
    uv_1, uv_2, offsets, _, status = _merge.prune_and_concat(h, w, fg, (first, second, off, n),
                                                             ((none, none), (none, none), None, 0), {(1, "b"): mask},
                                                             drop_empty=False)
    kept, bad = (int(x) for x in torch.cat([offsets[1:], status.to(torch.int64)]).cpu())
    if bad & _merge.BAD_INDEX:
        raise IndexError("prune_matches_if_occluded: a match lies outside the %d x %d mask" % (h, w))
    if kept == 0:
        return (None, None)
    return ((uv_1[0][:kept], uv_1[1][:kept]), (uv_2[0][:kept], uv_2[1][:kept]))


def merge_matches(matches_one, matches_two):
    """:337-345.  (cat(u_one, u_two), cat(v_one, v_two)) -- the reference's own torch.cat, on the tensors' device."""
    if not (_tensors(matches_one) and _tensors(matches_two)):
        return _reference("merge_matches")(matches_one, matches_two)
    return (torch.cat((matches_one[0], matches_two[0])), torch.cat((matches_one[1], matches_two[1])))
