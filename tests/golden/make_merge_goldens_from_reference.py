"""Pins the device merge (csrc/merge_kernels.hip, the merge names of dense_correspondence/correspondence_tools/
correspondence_augmentation.py of this root): executes the REFERENCE's own source text of
dense_correspondence/correspondence_tools/correspondence_augmentation.py (read from /root/reference at run time, never copied)
on PIL images after ``random.seed(s)`` and stores seed, inputs, outputs and the next ``random.random()`` as
tests/golden/merge_ref_*.npz (not augment_ref_*: tests/augment_common.py replays those).

Seeds are the first ones (from 0 up) that take the wanted foreground branch; inputs are structured (they compress) and the
archives are written with fixed zip timestamps, so running this again regenerates the files byte for byte.

    python tests/golden/make_merge_goldens_from_reference.py
"""
import os
import random

import numpy as np
import torch
from PIL import Image

from make_augmentation_goldens_from_reference import HERE, first_seed, load_reference, write_npz


def scene(h, w, cy, cx, ry, rx, phase):
    """uint8 RGB of 8 x 8 blocks and a 0/1 elliptical object mask centred at (cy, cx) * (h, w) with radii (ry, rx) * (h, w)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    bx, by = x // 8 + phase, y // 8
    rgb = np.stack([(17 * bx + 29 * by) % 256, (37 * bx + 39 * by + 11) % 256, (57 * bx + 49 * by + 101) % 256],
                   axis=-1).astype(np.uint8)
    mask = ((((y - cy * (h - 1)) / (ry * h + 0.5)) ** 2 + ((x - cx * (w - 1)) / (rx * w + 0.5)) ** 2) <= 1.0)
    return rgb, mask.astype(np.uint8)


def matches(h, w, n, k):
    """A pair of int64 (u, v) lists of n entries covering the image in a fixed pattern."""
    i = np.arange(n, dtype=np.int64)
    u1, v1 = (i * 37 + 5 + k) % w, (i * 53 + 3 + 2 * k) % h
    u2, v2 = (i * 41 + 7 + k) % w, (i * 31 + 1 + k) % h
    return u1, v1, u2, v2


def front_b(seed):
    random.seed(seed)
    return random.random() < 0.5


def pair(u1, v1, u2, v2):
    t = torch.from_numpy
    return ((t(u1), t(v1)), (t(u2), t(v2)))


def arr(x):
    return np.zeros(0, np.int64) if x is None else x.numpy()


def merge_case(ref, name, h, w, want_b, obj_a, obj_b, n_a=97, n_b=61):
    seed = first_seed(lambda s: front_b(s) == want_b)
    rgb_a, mask_a = scene(h, w, *obj_a, phase=0)
    rgb_b, mask_b = scene(h, w, *obj_b, phase=3)
    la, lb = matches(h, w, n_a, 0), matches(h, w, n_b, 1)
    random.seed(seed)
    merged, merged_mask, ma, ama, mb, amb = ref["merge_images_with_occlusions"](
        Image.fromarray(rgb_a), Image.fromarray(rgb_b), Image.fromarray(mask_a), Image.fromarray(mask_b), pair(*la), pair(*lb))
    after = np.array([random.random()])
    rec = dict(fn=np.array("merge_images_with_occlusions"), seed=np.array(seed), rgb_a=rgb_a, rgb_b=rgb_b, mask_a=mask_a,
               mask_b=mask_b, after_random=after, out_rgb=np.asarray(merged), out_mask=np.asarray(merged_mask))
    for k, x in zip(("u_a1", "v_a1", "u_a2", "v_a2"), la):
        rec[k] = x
    for k, x in zip(("u_b1", "v_b1", "u_b2", "v_b2"), lb):
        rec[k] = x
    for k, uv in (("a1", ma), ("a2", ama), ("b1", mb), ("b2", amb)):
        rec["none_" + k] = np.array(uv is None)
        rec["out_u_" + k] = arr(None if uv is None else uv[0])
        rec["out_v_" + k] = arr(None if uv is None else uv[1])
    write_npz(os.path.join(HERE, "merge_ref_%s.npz" % name), rec)


def prune_case(ref, name, h, w, obj, n):
    _, mask = scene(h, w, *obj, phase=0)
    l = matches(h, w, n, 2)
    out = ref["prune_matches_if_occluded"](mask, pair(*l))
    rec = dict(fn=np.array("prune_matches_if_occluded"), mask=mask, u_1=l[0], v_1=l[1], u_2=l[2], v_2=l[3],
               none=np.array(out[0] is None))
    if out[0] is not None:
        rec.update(out_u_1=out[0][0].numpy(), out_v_1=out[0][1].numpy(), out_u_2=out[1][0].numpy(), out_v_2=out[1][1].numpy())
    write_npz(os.path.join(HERE, "merge_ref_%s.npz" % name), rec)


def merge_matches_case(ref, name):
    a, b = matches(9, 11, 13, 0), matches(9, 11, 5, 1)
    t = torch.from_numpy
    u, v = ref["merge_matches"]((t(a[0]), t(a[1])), (t(b[0]), t(b[1])))
    write_npz(os.path.join(HERE, "merge_ref_%s.npz" % name),
              dict(fn=np.array("merge_matches"), u_1=a[0], v_1=a[1], u_2=b[0], v_2=b[1], out_u=u.numpy(), out_v=v.numpy()))


def main():
    ref = load_reference()
    center = (0.5, 0.5, 0.3, 0.3)           # object in the middle
    left = (0.5, 0.25, 0.4, 0.2)
    whole = (0.5, 0.5, 2.0, 2.0)            # covers the image
    tiny = (0.0, 0.0, 0.01, 0.01)           # a corner pixel or so
    outside = (5.0, 5.0, 0.1, 0.1)          # no pixel of the image
    for want_b, tag in ((True, "front_b"), (False, "front_a")):
        merge_case(ref, "partial_%s_37x53" % tag, 37, 53, want_b, center, left)
        merge_case(ref, "partial_%s" % tag, 480, 640, want_b, center, left, n_a=5000, n_b=3000)
    merge_case(ref, "no_occlusion_front_b_37x53", 37, 53, True, left, outside)
    merge_case(ref, "full_occlusion_front_b_37x53", 37, 53, True, center, whole)
    merge_case(ref, "full_occlusion_front_a_1x64", 1, 64, False, whole, center)
    merge_case(ref, "partial_front_b_1x64", 1, 64, True, center, left)
    merge_case(ref, "partial_front_a_48x1", 48, 1, False, left, center)
    merge_case(ref, "tiny_front_b_48x1", 48, 1, True, center, tiny)
    prune_case(ref, "prune_partial_37x53", 37, 53, center, 211)
    prune_case(ref, "prune_none_kept_37x53", 37, 53, whole, 50)
    prune_case(ref, "prune_all_kept_1x64", 1, 64, outside, 40)
    prune_case(ref, "prune_partial_48x1", 48, 1, center, 30)
    merge_matches_case(ref, "merge_matches")
    print("wrote", sorted(f for f in os.listdir(HERE) if f.startswith("merge_ref_")))


if __name__ == "__main__":
    main()
