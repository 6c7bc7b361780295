"""Pins the qualitative evaluation (csrc/picture_kernels.hip, dcn_hip/evaluate/pictures.py): executes the REFERENCE's own source
lines -- read from /root/reference at run time, never copied --
  dense_correspondence/evaluation/plotting.py:5-87        (normalize_descriptor, normalize_descriptor_pair,
                                                            normalize_masked_descriptor_pair)
  modules/dense_correspondence_manipulation/utils/visualization.py:27-31   (the heat map, up to but excluding applyColorMap)
  dense_correspondence/network/dense_correspondence_network.py:541-547     (the norm_diffs of find_best_match_for_descriptor)
on prepared descriptor images.  The slices are taken, not the modules: both modules import cv2.  In memory ``xrange`` is bound
to ``range``.  The lower row of plot_descriptor_colormaps with a stats dict (evaluation.py:585-598: normalize_descriptor on
mask * res, times the mask) is those three multiplications around the reference's function.

The picture bytes are matplotlib's own: ``AxesImage.make_image(renderer, unsampled=True)`` on the Agg backend, applied to the
reference's float output (a one-channel image as three equal channels, of which one is kept).

Stores in tests/golden/pictures_ref_<case>.npz: the inputs (res_a, res_b float32 [P, H, W, D], mask_a, mask_b uint8 [P, H, W],
stats_full, stats_mask float64 [2, D] (min, max), channels: what a picture shows); per normalisation ``<kind>_sha``, the SHA-256
of the reference's float output [2 (a, b), P, H, W, D] (every NaN written as one quiet NaN; "ValueError" where the reference
raised), ``<kind>_normed``, that output in full where the images are small, ``<kind>_picture`` uint8; ``pair_ranges`` float32
[P, 4, D] and ``status`` int32 [P] as the reference's text forms them; the numpy and matplotlib versions.  The heat cases hold
res_b, queries, offsets, variances, the reference's norm_diffs float32 [R, H, W] and planes uint8 [2 (variance), R, H, W].

The generator ASSERTS that the reference's output equals the numpy statement of tests/pictures_common.py bit for bit, that
matplotlib's bytes are uint8(255 * clip(v, 0, 1)) wherever v is not NaN, and that every fixture exercises what it is named for.

    python tests/golden/make_pictures_goldens_from_reference.py
"""
import ast
import hashlib
import os
import sys
import textwrap
import warnings

import matplotlib
matplotlib.use("Agg")
import matplotlib.pyplot as plt                                                     # noqa: E402
import numpy as np                                                                   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pictures_common as pc                                                         # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

REF = "/root/reference/"
PLOTTING = (REF + "dense_correspondence/evaluation/plotting.py", 5, 87,
            "ee08d0793928ea266a2c22157d91e71b0db0d11bbe716defcaa0041e44563c80")
HEATMAP = (REF + "modules/dense_correspondence_manipulation/utils/visualization.py", 27, 31,
           "32927bd67ca5c7556891d033f5eea9408588a82bf2907bd9b6029ca7a4df9a2b")
NORM_DIFFS = (REF + "dense_correspondence/network/dense_correspondence_network.py", 541, 547,
              "a325f4d90b999a84990cca678b0d580f56fc028c4519c1563469a0036bc1fad4")
FULL_FLOATS_UP_TO = 4096            # elements of one image: below, the reference's float outputs are stored in full
MAX_BYTES = 400 * 1024


def take(spec):
    path, first, last, sha = spec
    lines = open(path).read().split("\n")[first - 1:last]
    assert hashlib.sha256("\n".join(l.strip() for l in lines).encode()).hexdigest() == sha, "the reference changed: " + path
    return textwrap.dedent("\n".join(lines)).replace("xrange(", "range("), path


def load_reference():
    """-> (the three normalisations, heat(norm_diffs, variance), norm_diffs(res, descriptor)).  Each slice is validated by its
    structure, without quoting it, and by the hash of its text."""
    text, path = take(PLOTTING)
    body = ast.parse(text).body
    assert [type(n) for n in body] == [ast.FunctionDef] * 3 and [len(f.args.args) for f in body] == [2, 2, 4], "not the slice"
    env = {"np": np}
    exec(compile(text, path, "exec"), env)
    norms = [env[f.name] for f in body]
    text, path = take(HEATMAP)
    body = ast.parse(text).body
    assert len(body) == 4 and isinstance(body[2], ast.AugAssign) and all(isinstance(n, ast.Assign) for n in body[:2] + body[3:])
    target = body[0].targets[0].id
    assert all((n.target if isinstance(n, ast.AugAssign) else n.targets[0]).id == target for n in body), "not the slice"
    heat_code = compile(text, path, "exec")

    def heat(norm_diffs, variance):
        e = {"np": np, "norm_diffs": norm_diffs, "variance": variance}
        exec(heat_code, e)
        return e[target]
    text, path = take(NORM_DIFFS)
    body = ast.parse(text).body
    assert isinstance(body[0], ast.Assign) and body[0].targets[0].id == "norm_diffs", "not the slice"
    nd_code = compile(text, path, "exec")

    def norm_diffs(res, descriptor):
        e = {"np": np, "res": res, "descriptor": descriptor}
        exec(nd_code, e)
        return e["norm_diffs"]
    return norms, heat, norm_diffs


_fig = {}


def imshow_bytes(v):
    """The bytes imshow displays for the float RGB image v [H, W, 3]"""
    if "ax" not in _fig:
        _fig["fig"], _fig["ax"] = plt.subplots()
    fig, ax = _fig["fig"], _fig["ax"]
    ax.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        im = ax.imshow(v)
        out = im.make_image(fig.canvas.get_renderer(), unsampled=True)[0]
    assert out.dtype == np.uint8 and out.shape == v.shape[:2] + (4,), (out.dtype, out.shape)
    return out[..., :3].copy()


def pictures_of(normed, channels):
    """normed [2, P, H, W, D] -> matplotlib's bytes [2, P, H, W, 3] (or [2, P, H, W] for one channel)"""
    ch = list(channels) if len(channels) == 3 else [channels[0]] * 3
    out = np.stack([np.stack([imshow_bytes(normed[s, p][..., ch]) for p in range(normed.shape[1])]) for s in range(2)])
    rule = pc.np_picture(normed, ch)
    pinned = ~np.isnan(normed[..., ch])
    assert np.array_equal(out[pinned], rule[pinned]), "matplotlib's bytes are not uint8(255 * clip(v, 0, 1))"
    return out[..., 0] if len(channels) == 1 else out


def run_reference(norms, res_a, res_b, mask_a, mask_b, stats_full, stats_mask):
    """-> {kind: float [2, P, H, W, D] or None where the reference raised ValueError}"""
    normalize_descriptor, normalize_pair, normalize_masked = norms
    P, _, _, D = res_a.shape
    full = {"min": stats_full[0].tolist(), "max": stats_full[1].tolist()}
    under = {"min": stats_mask[0].tolist(), "max": stats_mask[1].tolist()}
    out = {k: [[], []] for k in pc.KINDS}
    raised = np.zeros(P, np.int32)
    with np.errstate(all="ignore"):
        for p in range(P):
            a, b, ma, mb = res_a[p], res_b[p], mask_a[p], mask_b[p]
            for s, x in enumerate(normalize_pair(a, b)):
                out["pair"][s].append(x)
            try:
                for s, x in enumerate(normalize_masked(a, b, ma, mb)):
                    out["masked"][s].append(x)
            except ValueError:
                raised[p] = 1
                for s in range(2):
                    out["masked"][s].append(np.full_like(a, np.nan))
            for s, (x, m) in enumerate(((a, ma), (b, mb))):
                out["scalar"][s].append(normalize_descriptor(x.copy(), None))
                out["stats"][s].append(normalize_descriptor(x.copy(), full))
                repeat = np.repeat(m[:, :, np.newaxis], D, axis=2)                  # evaluation.py:586-598
                out["stats_masked"][s].append(normalize_descriptor(repeat * x, under) * repeat)
    return {k: np.stack([np.stack(v[0]), np.stack(v[1])]) for k, v in out.items()}, raised


def case(norms, name, res_a, res_b, mask_a, mask_b, stats_full, stats_mask, channels=None, special=None):
    res_a, res_b = (np.ascontiguousarray(x, np.float32) for x in (res_a, res_b))
    mask_a, mask_b = (np.ascontiguousarray(x, np.uint8) for x in (mask_a, mask_b))
    assert set(np.unique(mask_a)) | set(np.unique(mask_b)) <= {0, 1}
    P, h, w, D = res_a.shape
    channels = tuple(range(D)) if channels is None else tuple(channels)
    stats_full, stats_mask = np.asarray(stats_full, np.float64), np.asarray(stats_mask, np.float64)
    ref, raised = run_reference(norms, res_a, res_b, mask_a, mask_b, stats_full, stats_mask)
    want, (image, pair, scalar, status) = pc.np_all(res_a, res_b, mask_a, mask_b, stats_full, stats_mask)
    assert np.array_equal(raised, status), (name, raised, status)
    z = dict(res_a=res_a, res_b=res_b, mask_a=mask_a, mask_b=mask_b, stats_full=stats_full, stats_mask=stats_mask,
             channels=np.array(channels), pair_ranges=pair, status=status, numpy_version=np.array(np.__version__),
             matplotlib_version=np.array(matplotlib.__version__))
    for kind in pc.KINDS:
        r = ref[kind]
        assert r.dtype == (np.float64 if kind.startswith("stats") else np.float32), (name, kind, r.dtype)
        if kind == "masked" and raised.any():
            z["masked_sha"] = np.array("ValueError")
            ok = raised == 0
            assert pc.same_bits(r[:, ok], want[kind][:, ok]), (name, kind)
            continue
        assert pc.same_bits(r, want[kind]), (name, kind, "the numpy statement is not the reference")
        z[kind + "_sha"] = np.array(pc.digest(r))
        if h * w * D <= FULL_FLOATS_UP_TO:
            z[kind + "_normed"] = r
        z[kind + "_picture"] = pictures_of(r, channels)
    check(name, z, ref, image, special)
    path = pc.golden(name)
    write_npz(path, z)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(name, "P", P, "shape", (h, w, D), "status", status.tolist(), "bytes", size)


def check(name, z, ref, image, special):
    """What makes the comparison meaningful, from the inputs and the reference's results alone"""
    res = np.stack([z["res_a"], z["res_b"]])
    mask = np.stack([z["mask_a"], z["mask_b"]])
    P, h, w, D = z["res_a"].shape
    on = mask.reshape(2, P, -1).sum(2)
    if special != "empty":
        assert ((on > 0) & (on < h * w)).all(), (name, "a mask is not partial")
    # the stats dicts are narrower than the data: the clip acts on both sides, in every channel
    for stats in (z["stats_full"], z["stats_mask"]):
        finite = np.where(np.isfinite(res), res, 0.0)
        below, above = finite.min((0, 1, 2, 3)) < stats[0], finite.max((0, 1, 2, 3)) > stats[1]
        assert (below | above).all() and (special == "constant" or (below & above).all()), name
    if special is None:
        assert not z["status"].any(), name
        for kind in pc.KINDS:
            assert np.isfinite(ref[kind]).all(), (name, kind, "the reference produces a NaN")
        # the masked range differs from the image's, and the three normalisations differ
        assert (z["pair_ranges"][:, 0] != z["pair_ranges"][:, 2]).any() and (z["pair_ranges"][:, 1] != z["pair_ranges"][:, 3]).any()
        assert not np.array_equal(ref["pair"], ref["scalar"]) and not np.array_equal(z["pair_picture"], z["masked_picture"])
        assert ref["pair"].min() == 0.0 and ref["pair"].max() == 1.0 and ref["stats"].min() == 0.0 and ref["stats"].max() < 1.0
    if name == "37x53_d3":
        assert (h * w * 3) % 4 != 0, "the second picture starts on a dword boundary"
    if special == "zero":
        x, m = z["res_a"][0, :, :, 1], z["mask_a"][0] != 0
        assert (x[m] >= 0).all() and (x[m] == 0).sum() >= 3 and np.signbit(x[m][x[m] == 0]).any(), "no zeros, no -0.0"
        assert image[0, 0, 2, 1] > 0 and (x * m).min() == 0, "the zeros are not the would-be minimum"
        assert np.isfinite(ref["masked"]).all()
    if special == "nan_a":
        assert np.isnan(z["res_a"]).sum() == 1 and not np.isnan(z["res_b"]).any()
        c = int(np.nonzero(np.isnan(z["res_a"]))[3][0])
        assert np.isnan(z["pair_ranges"][0, :, c]).all(), "a NaN in image a does not win"
        assert np.isnan(ref["pair"][:, 0, :, :, c]).all() and np.isfinite(np.delete(ref["pair"], c, axis=4)).all()
    if special == "nan_b":
        assert np.isnan(z["res_b"]).sum() == 1 and not np.isnan(z["res_a"]).any()
        c = int(np.nonzero(np.isnan(z["res_b"]))[3][0])
        assert np.isfinite(z["pair_ranges"]).all(), "a NaN in image b alone is not dropped"
        assert np.array_equal(z["pair_ranges"][0, :, c], image[0, 0, :, c])          # image a's range alone
        assert np.isnan(ref["pair"][..., c]).sum() == 1
    if special == "outside":
        at = np.nonzero(~np.isfinite(z["res_a"]))
        assert len(at[0]) == 1 and z["mask_a"][at[0][0], at[1][0], at[2][0]] == 0, "not one non-finite value outside the mask"
        c = int(at[3][0])
        assert np.isnan(z["pair_ranges"][0, 2:, c]).all() and np.isfinite(np.delete(z["pair_ranges"], c, axis=2)).all()
        assert not z["status"].any()
    if special == "constant":
        c = 1
        assert (res[..., c] == res[0, 0, 0, 0, c]).all()
        assert np.isnan(ref["pair"][..., c]).all() and np.isnan(ref["masked"][..., c]).all()
        assert np.isfinite(ref["stats"]).all() and np.isfinite(ref["stats_masked"]).all() and np.isfinite(ref["scalar"]).all()


def heat_case(heat, norm_diffs, name, res_b, queries, offsets):
    res_b, queries = np.ascontiguousarray(res_b, np.float32), np.ascontiguousarray(queries, np.float32)
    P, h, w, D = res_b.shape
    variances = [0.25, 0.1]
    nd = []
    for p in range(P):
        for r in range(offsets[p], offsets[p + 1]):
            nd.append(norm_diffs(res_b[p], queries[r]))
    nd = np.stack(nd)
    assert nd.dtype == np.float32 and nd.shape == (offsets[-1], h, w) and np.isfinite(nd).all()
    planes = np.stack([np.stack([heat(x, v) for x in nd]) for v in variances])
    assert planes.dtype == np.uint8
    for i, v in enumerate(variances):
        assert np.array_equal(planes[i], pc.np_heat_reference(nd, v))
        assert planes[i].max() == 255 and planes[i].min() < 16 and len(np.unique(planes[i])) > 64, (name, "a flat plane", len(np.unique(planes[i])))
    assert not np.array_equal(planes[0], planes[1])
    z = dict(res_b=res_b, queries=queries, offsets=np.asarray(offsets, np.int64), variances=np.array(variances),
             norm_diffs=nd, planes=planes, numpy_version=np.array(np.__version__),
             matplotlib_version=np.array(matplotlib.__version__))
    path = pc.golden(name)
    write_npz(path, z)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(name, "rows", int(offsets[-1]), "pairs", P, "bytes", size)


def grid(rng, shape, scale=1.0, offset=0.0):
    """Descriptor values on a grid of 1 / 64 (the inputs deflate to a third)"""
    return np.round((rng.standard_normal(shape) * scale + offset) * 64.0) / 64.0


def smooth(rng, shape):
    """Descriptor images that vary slowly over the image, so that the distances to a pixel's descriptor cover a range"""
    P, h, w, D = shape
    ys, xs = np.mgrid[0:h, 0:w]
    f = rng.rand(P, 1, 1, D, 4) * 2.0 + 0.5
    wave = np.sin(f[..., 0] * xs[None, :, :, None] / w * 3 + f[..., 1]) + np.cos(f[..., 2] * ys[None, :, :, None] / h * 3 + f[..., 3])
    return np.round((wave * (0.6 / np.sqrt(D)) + rng.standard_normal(shape) * 0.01) * 4096.0) / 4096.0


def masks(rng, P, h, w):
    out = np.zeros((2, P, h, w), np.uint8)
    for s in range(2):
        for p in range(P):
            if h == 1 or w == 1:
                out[s, p] = rng.rand(h, w) < 0.5
                out[s, p].flat[p + s] = 1
                out[s, p].flat[-1 - p] = 0
            else:
                out[s, p, h // 5 + p:4 * h // 5 - s, w // 6 + 2 * s:5 * w // 6 - p] = 1
                out[s, p] &= rng.rand(h, w) < 0.9
    return out[0], out[1]


def narrow_stats(D):
    """A stats dict narrower than the data on both sides, another one for the mask"""
    c = np.arange(D)
    return np.stack([-0.75 - 0.03125 * c, 1.0 + 0.0625 * c]), np.stack([-0.5 + 0.015625 * c, 0.625 + 0.03125 * c])


def main():
    norms, heat, norm_diffs = load_reference()
    rng = np.random.RandomState(3)
    for name, (h, w, D), channels in (("48x64_d3", (48, 64, 3), None), ("37x53_d3", (37, 53, 3), None),
                                      ("37x53_d16", (37, 53, 16), (14, 0, 7)), ("1x64_d1", (1, 64, 1), None),
                                      ("48x1_d1", (48, 1, 1), None)):
        res = grid(rng, (2, 2, h, w, D), 0.75, 0.125)
        ma, mb = masks(rng, 2, h, w)
        case(norms, name, res[0], res[1], ma, mb, *narrow_stats(D), channels=channels)
    h, w, D = 9, 13, 3
    ma, mb = masks(rng, 2, h, w)
    # exact zeros and a -0.0 under the mask that are the would-be minimum (channel 1 of pair 0, image a, is positive there)
    res = grid(rng, (2, 2, h, w, D), 0.75, 0.125)
    res[0, 0, :, :, 1] = np.abs(res[0, 0, :, :, 1]) + 0.25
    inside = np.argwhere(ma[0] != 0)
    for k, value in enumerate((0.0, -0.0, 0.0)):
        res[0, 0, inside[3 * k + 1][0], inside[3 * k + 1][1], 1] = value
    case(norms, "zero_under_mask", res[0], res[1], ma, mb, *narrow_stats(D), special="zero")
    # one NaN in one channel of image a, respectively b, under the mask
    for side, special in ((0, "nan_a"), (1, "nan_b")):
        res = grid(rng, (2, 2, h, w, D), 0.75, 0.125)
        v, u = np.argwhere((ma, mb)[side][0] != 0)[5]
        res[side, 0, v, u, 2] = np.nan
        case(norms, "nan_in_" + "ab"[side], res[0], res[1], ma, mb, *narrow_stats(D), special=special)
    # a non-finite value outside the mask: inf * 0 = NaN poisons the masked range of that channel
    res = grid(rng, (2, 2, h, w, D), 0.75, 0.125)
    v, u = np.argwhere(ma[0] == 0)[2]
    res[0, 0, v, u, 0] = np.inf
    case(norms, "nan_outside_mask", res[0], res[1], ma, mb, *narrow_stats(D), special="outside")
    # max == min in one channel of every image
    res = grid(rng, (2, 2, h, w, D), 0.75, 0.125)
    res[..., 1] = 0.375
    full, under = narrow_stats(D)
    full[:, 1], under[:, 1] = (0.25, 0.3125), (0.28125, 0.34375)           # (narrower than the data: the constant lies above)
    case(norms, "constant_channel", res[0], res[1], ma, mb, full, under, special="constant")
    # heat maps: R = 5 rows over 2 pairs
    for name, (h, w, D), rows in (("heat_37x53_d3", (37, 53, 3), (2, 3)), ("heat_48x64_d16", (48, 64, 16), (4, 1))):
        res_b = smooth(rng, (2, h, w, D))
        offsets = [0, rows[0], rows[0] + rows[1]]
        queries = np.stack([res_b[0 if r < rows[0] else 1].reshape(-1, D)[rng.randint(h * w)] for r in range(offsets[-1])])
        queries[1::2] += grid(rng, queries[1::2].shape, 0.05)
        heat_case(heat, norm_diffs, name, res_b, queries, offsets)


if __name__ == "__main__":
    main()
