"""Pins the device augmentation (csrc/augment_kernels.hip, dense_correspondence/correspondence_tools/correspondence_augmentation.py
of this root): executes the REFERENCE's own source text of dense_correspondence/correspondence_tools/correspondence_augmentation.py
(read from /root/reference at run time, never copied) on PIL images after ``random.seed(s); np.random.seed(s)`` and stores
seed, inputs, outputs and the next draw of both random streams as tests/golden/augment_ref_*.npz.

One in-memory patch (nothing else is touched): flip_vertical / flip_horizontal read ``image.height`` / ``image.width`` from
their list comprehension's variable, which Python 2 leaks and Python 3 does not (NameError); it is replaced by ``images[-1]``,
the value it has under Python 2.

Seeds are the first ones (from 0 up) that take the wanted branch; inputs are structured (they compress) and the archives are
written with fixed zip timestamps, so running this again regenerates the files byte for byte.

    python tests/golden/make_augmentation_goldens_from_reference.py
"""
import io
import os
import random
import zipfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "/root/reference/dense_correspondence/correspondence_tools/correspondence_augmentation.py"


def load_reference():
    text = open(SRC).read()
    for old, new in (("(image.height-1) - v_pixel_positions", "(images[-1].height-1) - v_pixel_positions"),
                     ("(image.width-1) - u_pixel_positions", "(images[-1].width-1) - u_pixel_positions")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    ns = {"__name__": "reference_correspondence_augmentation"}
    exec(compile(text, SRC, "exec"), ns)
    return ns


def scene(h, w):
    """uint8 RGB of 8 x 8 blocks (every value 0..255 occurs, and it compresses), a 0/1 elliptical object mask (~80 % of the
    image), 16-bit depth in millimetres."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    bx, by = x // 8, y // 8
    rgb = np.stack([(17 * bx + 29 * by) % 256, (37 * bx + 39 * by + 11) % 256, (57 * bx + 49 * by + 101) % 256],
                   axis=-1).astype(np.uint8)
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    mask = ((((y - cy) / (0.5 * h + 0.5)) ** 2 + ((x - cx) / (0.5 * w + 0.5)) ** 2) <= 1.0).astype(np.uint8)
    depth = (700 + 10 * (x // 16) + 7 * (y // 16) + 40 * (mask == 1)).astype(np.uint16)
    return rgb, mask, depth


def uv_lists(h, w, n, dtype):
    k = np.arange(n, dtype=np.int64)
    u, v = (k * 37 + 5) % w, (k * 53 + 3) % h
    if dtype == "float32":
        return u.astype(np.float32) + 0.25, v.astype(np.float32) + 0.75
    return u, v


def branches_background(seed):
    """The branch random_domain_randomize_background takes after seeding: None (kept) or (gradient, vertical, noise)."""
    random.seed(seed)
    np.random.seed(seed)
    if random.random() < 0.5:
        return None
    gradient = not random.random() < 0.5
    np.random.uniform(size=3)
    vertical = False
    if gradient:
        np.random.uniform(size=3)
        vertical = bool(np.random.uniform() > 0.5)
    noise = not random.random() < 0.5
    return (gradient, vertical, noise)


def first_seed(pred):
    for s in range(100000):
        if pred(s):
            return s
    raise RuntimeError("no seed")


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps (byte-identical on every run)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def after_draws():
    return np.array([random.random()]), np.array([np.random.uniform()])


def background_case(ref, name, h, w, want):
    seed = first_seed(lambda s: branches_background(s) == want)
    rgb, mask, _ = scene(h, w)
    random.seed(seed)
    np.random.seed(seed)
    out = ref["random_domain_randomize_background"](Image.fromarray(rgb), Image.fromarray(mask))
    ar, an = after_draws()
    write_npz(os.path.join(HERE, "augment_ref_%s.npz" % name),
              dict(fn=np.array("random_domain_randomize_background"), seed=np.array(seed), rgb=rgb, mask=mask,
                   out_rgb=np.asarray(out), after_random=ar, after_numpy=an))


def mutation_case(ref, name, fn, h, w, with_depth, uv_dtype, want_flip=None):
    import torch
    rgb, mask, depth = scene(h, w)
    u, v = uv_lists(h, w, 97, uv_dtype)
    if want_flip is None:
        seed = 0
    else:
        seed = first_seed(lambda s: (random.seed(s), random.random() >= 0.5)[1] == want_flip)
    images = [Image.fromarray(rgb)] + ([Image.fromarray(depth)] if with_depth else []) + [Image.fromarray(mask)]
    random.seed(seed)
    np.random.seed(seed)
    out_images, (ou, ov) = ref[fn](images, (torch.from_numpy(u), torch.from_numpy(v)))
    ar, an = after_draws()
    rec = dict(fn=np.array(fn), seed=np.array(seed), rgb=rgb, mask=mask, u=u, v=v, out_rgb=np.asarray(out_images[0]),
               out_mask=np.asarray(out_images[-1]), out_u=ou.numpy(), out_v=ov.numpy(), after_random=ar, after_numpy=an)
    if with_depth:
        rec.update(depth=depth, out_depth=np.asarray(out_images[1]))
    write_npz(os.path.join(HERE, "augment_ref_%s.npz" % name), rec)


def main():
    ref = load_reference()
    H, W = 480, 640
    for grad, vert, tag in ((False, False, "solid"), (True, True, "gradient_vertical"), (True, False, "gradient_horizontal")):
        for noise in (False, True):
            background_case(ref, "bg_%s%s" % (tag, "_noise" if noise else ""), H, W, (grad, vert, noise))
    background_case(ref, "bg_kept_37x53", 37, 53, None)
    background_case(ref, "bg_gradient_horizontal_noise_37x53", 37, 53, (True, False, True))
    background_case(ref, "bg_gradient_vertical_noise_37x53", 37, 53, (True, True, True))
    background_case(ref, "bg_gradient_vertical_1x64", 1, 64, (True, True, False))
    background_case(ref, "bg_gradient_horizontal_noise_1x64", 1, 64, (True, False, True))
    background_case(ref, "bg_gradient_horizontal_48x1", 48, 1, (True, False, False))
    background_case(ref, "bg_gradient_vertical_noise_48x1", 48, 1, (True, True, True))
    mut = "random_image_and_indices_mutation"
    mutation_case(ref, "mutation_rgb_mask_int64_rotated", mut, H, W, False, "int64", True)
    mutation_case(ref, "mutation_rgb_mask_int64_kept", mut, H, W, False, "int64", False)
    mutation_case(ref, "mutation_rgb_depth_mask_float32_rotated", mut, H, W, True, "float32", True)
    mutation_case(ref, "mutation_rgb_depth_mask_float32_kept", mut, 37, 53, True, "float32", False)
    mutation_case(ref, "mutation_rgb_depth_mask_int64_rotated_37x53", mut, 37, 53, True, "int64", True)
    mutation_case(ref, "mutation_rgb_mask_float32_rotated_1x64", mut, 1, 64, False, "float32", True)
    mutation_case(ref, "mutation_rgb_depth_mask_int64_rotated_48x1", mut, 48, 1, True, "int64", True)
    for fn in ("flip_vertical", "flip_horizontal"):
        mutation_case(ref, fn + "_37x53", fn, 37, 53, True, "int64")
        mutation_case(ref, fn + "_float32_1x64", fn, 1, 64, False, "float32")
    print("wrote", sorted(f for f in os.listdir(HERE) if f.startswith("augment_ref_")))


if __name__ == "__main__":
    main()
