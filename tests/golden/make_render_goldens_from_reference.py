"""Pins the mask rules of the render chain (csrc/render_kernels.hip mask_kernel, dcn_hip/render.py foreground_masks): executes
the REFERENCE's own source lines -- read from /root/reference at run time, never copied --
  modules/dense_correspondence_manipulation/change_detection/change_detection.py
    :315-329   computeForegroundMaskFromDepthImagePair
    :251-257   computeForegroundMask's preparation (zeros become INT32_MAX), its call of the pair function, depth_img_change
    :298-300   computeForegroundMaskUsingCropStrategy's rule
    :388       ChangeDetection.run's visible mask
on prepared depth pairs.  The slices are taken, not the module: change_detection.py imports director.  The int32 conversion
of the two images (:248-249 read them from the depth scanners) is done here with the same ``np.array(..., dtype=np.int32)``.

The rasteriser itself has NO reference text to pin to: the reference renders through VTK / OpenGL.  Its yardstick is the
numpy statement in tests/render_common.py.

Stores in tests/golden/render_ref_masks_<H>x<W>.npz: depth_f, depth_b uint16 [2, H, W]; thresholds; per threshold mask uint8,
visible uint8, depth_change uint16; crop_mask, crop_visible uint8.  The pairs include zeros in either image and in both,
differences of exactly threshold and threshold + 1 for every threshold, and 65535 in either image.  The generator ASSERTS that
the reference's outputs equal tests/render_common.py's np_masks and that every planted pair is present.

    python tests/golden/make_render_goldens_from_reference.py
"""
import ast
import hashlib
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import render_common as rc                                                           # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

SRC = "/root/reference/modules/dense_correspondence_manipulation/change_detection/change_detection.py"
PAIR = (SRC, 315, 329, "95442cf32bc2e948faf703465d6ab6a93ef21e69b19ec48afada4074d7ce7662")
PREPARE = (SRC, 251, 257, "a111531f364571af4de1f7ec525af6454a2c9d3b44083775f46e79bc38c4721a")
CROP = (SRC, 298, 300, "60101c0de6c97e8f5b41684da01e98e1b9635e1f90cd2d7b0b5e277e645e84e1")
VISIBLE = (SRC, 388, 388, "58a53fec390b09a4ed322810527a2dd4e5b202116de508c5739c36e28964ffe2")
THRESHOLDS = (10, 0, 25)


def take(spec):
    path, first, last, sha = spec
    lines = open(path).read().split("\n")[first - 1:last]
    got = hashlib.sha256("\n".join(l.strip() for l in lines).encode()).hexdigest()
    assert got == sha, "the reference changed: %s:%d-%d (%s)" % (path, first, last, got)
    return textwrap.dedent("\n".join(lines)), path


def load_reference():
    """-> change(raw_f, raw_b, threshold) -> (mask, depth_img_change), crop(raw_f) -> mask, visible(mask).  Each slice is
    validated by its structure, without quoting it, and by the hash of its text."""
    text, path = take(PAIR)
    body = ast.parse(text).body
    assert len(body) == 1 and isinstance(body[0], ast.FunctionDef) and len(body[0].args.args) == 3, "not the slice"
    env = {"np": np}
    exec(compile(text, path, "exec"), env)
    holder = types.SimpleNamespace(**{body[0].name: env[body[0].name]})
    text, path = take(PREPARE)
    body = ast.parse(text).body
    assert len(body) == 4 and all(isinstance(n, ast.Assign) for n in body), "not the slice"
    names = [n.targets[0] for n in body]
    assert isinstance(names[0], ast.Subscript) and isinstance(names[1], ast.Subscript) and isinstance(names[2], ast.Tuple)
    img_b, img_f = names[0].value.id, names[1].value.id
    mask_name, change_name = names[2].elts[1].id, names[3].id
    class_name = body[2].value.func.value.id
    prepare = compile(text, path, "exec")

    def change(raw_f, raw_b, threshold):
        e = {"np": np, img_f: np.array(raw_f, dtype=np.int32), img_b: np.array(raw_b, dtype=np.int32),
             class_name: holder, "self": types.SimpleNamespace(threshold=threshold)}
        exec(prepare, e)
        return e[mask_name], e[change_name]
    text, path = take(CROP)
    body = ast.parse(text).body
    assert len(body) == 3 and all(isinstance(n, ast.Assign) for n in body) and isinstance(body[0].value, ast.Compare), "not the slice"
    crop_in, crop_out = body[0].value.left.id, body[1].targets[0].id
    crop_code = compile(text, path, "exec")

    def crop(raw_f):
        e = {"np": np, crop_in: np.array(raw_f, dtype=np.int32)}
        exec(crop_code, e)
        return e[crop_out]
    text, path = take(VISIBLE)
    body = ast.parse(text).body
    assert len(body) == 1 and isinstance(body[0].value, ast.BinOp) and isinstance(body[0].value.op, ast.Mult), "not the slice"
    vis_in, vis_out = body[0].value.left.id, body[0].targets[0].id
    vis_code = compile(text, path, "exec")

    def visible(mask):
        e = {vis_in: mask}
        exec(vis_code, e)
        return e[vis_out]
    return change, crop, visible


def depth_pairs(h, w, seed):
    rng = np.random.RandomState(seed)
    f = rng.randint(400, 1600, (2, h, w)).astype(np.uint16)
    b = (f.astype(np.int64) + rng.randint(-30, 31, (2, h, w))).astype(np.uint16)
    f[rng.rand(2, h, w) < 0.1] = 0
    b[rng.rand(2, h, w) < 0.1] = 0
    planted = [(0, 0), (0, 900), (900, 0), (65535, 65535), (65535, 0), (0, 65535), (65535, 65500), (65500, 65535), (1, 65535)]
    for t in THRESHOLDS:
        planted += [(1000, 1000 + t), (1000, 1000 + t + 1), (1000 + t, 1000), (65535 - t, 65535), (65535 - t - 1, 65535)]
    flat_f, flat_b = f.reshape(2, -1), b.reshape(2, -1)
    spots = rng.permutation(h * w)[:len(planted)]
    for img in range(2):
        for s, (pf, pb) in zip(spots, planted):
            flat_f[img, s], flat_b[img, s] = pf, pb
    return f, b, planted


def main():
    change, crop, visible = load_reference()
    for h, w in ((37, 53), (48, 64)):
        f, b, planted = depth_pairs(h, w, seed=h + w)
        have = set(zip(f.reshape(-1).tolist(), b.reshape(-1).tolist()))
        assert all(p in have for p in planted)
        out = dict(depth_f=f, depth_b=b, thresholds=np.array(THRESHOLDS, np.int32))
        masks, visibles, changes = [], [], []
        for t in THRESHOLDS:
            mask, dchange = change(f, b, t)
            vis = visible(mask)
            assert set(np.unique(mask)) == {0.0, 1.0} and dchange.min() >= 0 and dchange.max() <= 65535 and vis.max() == 255
            m8, v8, c16 = mask.astype(np.uint8), vis.astype(np.uint8), dchange.astype(np.uint16)
            for got, want in zip((m8, v8, c16), rc.np_masks(f, b, t)):
                assert np.array_equal(got, want), "tests/render_common.py np_masks is not the reference's rule"
            masks.append(m8)
            visibles.append(v8)
            changes.append(c16)
        out.update(mask=np.stack(masks), visible=np.stack(visibles), depth_change=np.stack(changes))
        cm = crop(f)
        out.update(crop_mask=cm.astype(np.uint8), crop_visible=visible(cm).astype(np.uint8))
        for got, want in zip((out["crop_mask"], out["crop_visible"]), rc.np_masks(f)[:2]):
            assert np.array_equal(got, want)
        assert 0 < out["crop_mask"].sum() < out["crop_mask"].size
        path = os.path.join(HERE, "render_ref_masks_%dx%d.npz" % (h, w))
        write_npz(path, out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
