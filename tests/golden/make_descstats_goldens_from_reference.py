"""Pins the descriptor statistics (csrc/descstats_kernels.hip, dcn_hip/evaluate/descstats.py): executes the REFERENCE's own source lines
-- read from /root/reference at run time, never copied --
  dense_correspondence/evaluation/evaluation.py:2177-2292   (the inner functions of compute_descriptor_statistics_on_dataset,
  compute_descriptor_statistics / update_stats, its loop over the images and the final scaling)
on CPU torch, with a stub dataset and a stub network that hand out prepared descriptor images and masks (``to_tensor`` and
``.cuda()`` are stubs too: the mask arrives as it is).  In memory, ``xrange`` / ``iteritems`` are bound to their Python 3
names (the Python 2 text of the slice parses as Python 3 otherwise).  compute_descriptor_statistics is wrapped between the two halves of the text so that its per-image tuples are recorded.

Stores in tests/golden/descstats_ref_*.npz: the inputs (res float32 [n, H, W, D], mask uint8 [n, H, W]), the reference's final
dict as ``ref_stats`` float32 [2, 3, D] (entire image, mask) x (min, max, mean), its per-image tuples as ``ref_per_image``
float32 [n, 2, 3, D] (NaN rows for an image it skipped, ``ref_used`` says which), ``mask_pixels``, ``mean_f64`` [n, 2, D] (the
float64 per-image means; NaN for an empty mask) and ``ref_mean_err`` = |reference per-image mean - mean_f64| (NaN where the
reference has no tuple).

The generator ASSERTS that every fixture exercises what it is named for (see ``check``).

    python tests/golden/make_descstats_goldens_from_reference.py
"""
import ast
import hashlib
import logging
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

EVAL = "/root/reference/dense_correspondence/evaluation/evaluation.py"
SLICE_SHA256 = "3a2fcd305f2bdcb2030ce5e52c9768c320a6eb55d145cb8a3901e333967810ce"
SETS, FIELDS = ("entire_image", "mask_image"), ("min", "max", "mean")


def load_reference():
    """-> (functions, loop): the two halves of evaluation.py:2177-2292 compiled separately.  The slice is validated by its
    structure, without quoting it: three function definitions (the first takes the descriptor image and the mask, the last the
    running dict and an image's tuple), then statements that end in a loop over the dict; and by the hash of its text."""
    ev = open(EVAL).read().split("\n")
    lines = ev[2176:2292]
    text = textwrap.dedent("\n".join(lines))
    body = ast.parse(text).body
    defs = [n for n in body if isinstance(n, ast.FunctionDef)]
    assert [type(n) for n in body[:3]] == [ast.FunctionDef] * 3 and len(defs) == 3, [type(n).__name__ for n in body]
    assert [len(f.args.args) for f in defs] == [2, 2, 2] and isinstance(body[-1], ast.For), "not the expected slice"
    assert hashlib.sha256("\n".join(l.strip() for l in lines).encode()).hexdigest() == SLICE_SHA256, "the reference changed"
    cut = body[3].lineno - 1
    py3 = lambda part: "\n".join(part).replace("xrange(", "range(").replace(".iteritems()", ".items()")
    parts = text.split("\n")
    return compile(py3(parts[:cut]), EVAL, "exec"), compile(py3(parts[cut:]), EVAL, "exec")


class OnDevice(object):
    """what ``to_tensor(mask)`` returns: ``.cuda()`` hands the tensor on"""

    def __init__(self, t):
        self.t = t

    def cuda(self):
        return self.t


class Dataset(object):
    def __init__(self, res, mask):
        self.res, self.mask, self.i = res, mask, -1

    def get_random_rgbd_mask_pose(self):
        self.i += 1
        return self.i, None, self.mask[self.i], None

    def rgb_image_to_tensor(self, rgb):
        return rgb


class Network(object):
    def __init__(self, res):
        self.res = res

    def forward_single_image_tensor(self, i):
        return torch.from_numpy(self.res[i].copy())


def run_reference(ref, res, mask):
    functions, loop = ref
    n = res.shape[0]
    env = {"torch": torch, "logging": logging, "dataset": Dataset(res, mask), "dcn": Network(res), "num_images": n,
           "to_tensor": lambda m: OnDevice(torch.from_numpy(m.copy())[None])}
    exec(functions, env)
    inner, tuples = env["compute_descriptor_statistics"], []

    def recording(r, m):
        out = inner(r, m)
        tuples.append(None if out[1] is None else [[t.clone().numpy() for t in s] for s in out])
        return out
    env["compute_descriptor_statistics"] = recording
    exec(loop, env)
    assert len(tuples) == n
    stats = env["stats"]
    d = res.shape[3]
    ref_stats = np.array([[stats[s][f] for f in FIELDS] for s in SETS], np.float64).astype(np.float32)
    assert ref_stats.shape == (2, 3, d)
    assert np.array_equal(ref_stats.astype(np.float64), np.array([[stats[s][f] for f in FIELDS] for s in SETS]))
    per_image = np.full((n, 2, 3, d), np.nan, np.float32)
    for i, t in enumerate(tuples):
        if t is not None:
            per_image[i] = np.asarray(t, np.float32)
    return ref_stats, per_image, np.array([t is not None for t in tuples])


def case(ref, name, res, mask):
    res, mask = np.ascontiguousarray(res, np.float32), np.ascontiguousarray(mask, np.uint8)
    n, h, w, d = res.shape
    ref_stats, per_image, used = run_reference(ref, res, mask)
    flat, on = res.reshape(n, h * w, d).astype(np.float64), mask.reshape(n, h * w) != 0
    mean_f64 = np.full((n, 2, d), np.nan)
    for i in range(n):
        mean_f64[i, 0] = flat[i].mean(0)
        if on[i].any():
            mean_f64[i, 1] = flat[i][on[i]].mean(0)
    z = dict(res=res, mask=mask, num_images=np.array(n), ref_stats=ref_stats, ref_per_image=per_image, ref_used=used,
             mask_pixels=on.sum(1).astype(np.int32), mean_f64=mean_f64,
             ref_mean_err=np.abs(per_image[:, :, 2].astype(np.float64) - mean_f64))
    check(name, z)
    path = os.path.join(HERE, "descstats_ref_%s.npz" % name)
    write_npz(path, z)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "evalpairs_ref_37x53_d16.npz")), (name, "too large")
    print(name, "images", n, "used", int(used.sum()), "mask pixels", z["mask_pixels"].tolist(),
          "largest reference mean error %.3e" % np.nanmax(z["ref_mean_err"]), "bytes", os.path.getsize(path))


def check(name, z):
    """What makes the comparison meaningful, from the inputs and the reference's results alone"""
    n = int(z["num_images"])
    used, pix, per = z["ref_used"], z["mask_pixels"], z["ref_per_image"]
    hw = z["mask"].shape[1] * z["mask"].shape[2]
    assert np.array_equal(used, pix > 0), name                               # the reference skips exactly the empty masks
    assert used.any() and np.isfinite(z["ref_stats"]).all(), name
    assert np.isnan(per[~used]).all() and np.isfinite(per[used]).all(), name
    partial = used & (pix < hw)
    for i in np.flatnonzero(partial):                                        # mask statistics differ from the image's
        assert (per[i, 0, 2] != per[i, 1, 2]).all(), (name, i)
    if partial.any():
        assert (per[partial][:, 0, :2] != per[partial][:, 1, :2]).any(), name
        assert (z["ref_stats"][0, 2] != z["ref_stats"][1, 2]).all(), name
    if name.startswith("a_"):
        assert pix[2] == 0 and not used[2], "image 2 is not skipped"
        assert int(used.sum()) != n, "the divisor num_images equals the number of images used"
        assert pix[4] == 1 and z["mask"][4].reshape(-1)[-1] != 0, "image 4's mask is not the last pixel alone"
        # the divisor shows: the mean of the used images' means differs from the reference's scaled sum
        assert not np.allclose(per[used][:, :, 2].mean(0), z["ref_stats"][:, 2]), "the divisor does not show"
    if name.startswith("b_"):
        assert partial.all(), "a mask of b is not partial"
        x = z["res"].astype(np.float64)
        assert abs(x.mean()) > 50 * x.std(), "no common offset: cancellation does not matter"
    if name.startswith("c_"):
        assert z["res"].shape[3] == 1 and 1 in z["res"].shape[1:3] and n == 2, name
    if name.startswith("d_"):
        assert z["res"].shape[3] & (z["res"].shape[3] - 1) and 256 % z["res"].shape[3], "the channel count divides a power of two"
        full = pix == hw
        assert full.sum() == 1 and np.array_equal(per[full][0][0], per[full][0][1]), "no image with a full mask"
        assert partial.sum() == n - 1


def blob_mask(rng, n, h, w, fraction):
    return (rng.rand(n, h, w) < fraction).astype(np.uint8)


def main():
    ref = load_reference()
    rng = np.random.RandomState(1)
    # a: an empty mask (image 2: skipped for both sets, so num_images != used) and a single mask pixel, the last one (image 4)
    res = rng.randn(5, 37, 53, 16) * np.linspace(0.5, 3.0, 16) + np.linspace(-2.0, 2.0, 16)
    mask = blob_mask(rng, 5, 37, 53, 0.3)
    mask[2] = 0
    mask[4] = 0
    mask[4, -1, -1] = 1
    case(ref, "a_37x53_d16", res, mask)
    # b: a large common offset
    res = 100.0 + rng.randn(4, 48, 64, 3)
    mask = np.zeros((4, 48, 64), np.uint8)
    for i in range(4):
        mask[i, 5 + 3 * i:30 + 4 * i, 8 + 2 * i:40 + 5 * i] = 255
    case(ref, "b_48x64_d3", res, mask)
    # c: one row, one column, one channel
    case(ref, "c_1x64_d1", rng.randn(2, 1, 64, 1) + 0.5, blob_mask(rng, 2, 1, 64, 0.5))
    case(ref, "c_48x1_d1", rng.randn(2, 48, 1, 1) - 0.5, blob_mask(rng, 2, 48, 1, 0.4))
    # d: a channel count that divides no power of two; one full mask
    res = rng.randn(3, 37, 53, 5) * 2.0
    mask = blob_mask(rng, 3, 37, 53, 0.25)
    mask[1] = 1
    case(ref, "d_37x53_d5", res, mask)


if __name__ == "__main__":
    main()
