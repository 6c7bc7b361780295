"""Shared by tests/test_emu_pictures.py and tests/test_gpu_pictures.py: the checks of the qualitative evaluation
(csrc/picture_kernels.hip, dcn_hip/evaluate/pictures.py) against the pictures goldens (the reference's own normalize_descriptor,
normalize_descriptor_pair, normalize_masked_descriptor_pair and heat-map lines on prepared descriptor images, with matplotlib's
own bytes; tests/golden/make_pictures_goldens_from_reference.py) and against the numpy statement below.

The bounds.  Ranges, normalised images and status are compared BIT FOR BIT (NaN matches NaN): every operation of the kernels is
one IEEE operation in the precision the reference uses (float32, or float64 once numpy has promoted), with contraction off, so
nothing is left to tolerate.  The numpy statement below states each operation in that precision; the goldens' maker asserts
that the reference's own output equals it bit for bit, and the fixtures keep the reference's output as a SHA-256 of its bytes
(a 37 x 53 x 16 pair in float64 would not fit a committed file) -- in full where the images are small.  Pictures are compared
byte for byte wherever the float is not NaN.

The heat maps are compared with the reference formula in numpy's float32 on the distances of ``match.find_best_matches``: every
byte within 1, at most 0.1 % of a plane's bytes different at all.  That margin covers only numpy's float32 ``exp`` against a
correctly rounded one (about one byte in a million, never more than one level); a wrong quotient, sign, scale or truncation
changes far more than 0.1 %."""
import glob
import hashlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "pictures_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("pictures_ref_"):-4] for p in GOLDENS]
HEAT_IDS = [i for i in GOLDEN_IDS if i.startswith("heat_")]
NORM_IDS = [i for i in GOLDEN_IDS if not i.startswith("heat_")]
EXPECTED_IDS = sorted(["48x64_d3", "37x53_d3", "37x53_d16", "1x64_d1", "48x1_d1", "zero_under_mask", "nan_in_a", "nan_in_b",
                       "nan_outside_mask", "constant_channel", "heat_37x53_d3", "heat_48x64_d16"])
KINDS = ("pair", "masked", "scalar", "stats", "stats_masked")
CHANNELS = (1, 3, 16, 64)
HEAT_MAX_LEVELS, HEAT_MAX_FRACTION = 1, 1e-3
_cache = {}


def golden(name):
    return os.path.join(HERE, "golden", "pictures_ref_%s.npz" % name)


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    return None if t is None else t.cpu().numpy()


def same_bits(a, b):
    """float arrays of one dtype equal bit for bit; a NaN matches a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64), (a.dtype, b.dtype)
    bits = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(bits), b[~nb].view(bits))


def digest(a):
    """SHA-256 of a float array's bytes, every NaN written as the one quiet NaN"""
    a = np.ascontiguousarray(a).copy()
    a[np.isnan(a)] = np.nan
    return hashlib.sha256(a.tobytes()).hexdigest()


# ---- the numpy statement: each operation in the precision the reference computes it in ------------------------------------
def np_ranges(res_a, res_b, mask_a=None, mask_b=None):
    """-> (image float32 [2, P, 4, D], pair float32 [P, 4, D], scalar float32 [2, P, 2], status int32 [P]); rows 2, 3 NaN without
    masks; status 1 where an image of the pair has a channel without a non-zero product"""
    P, _, _, D = res_a.shape
    image = np.full((2, P, 4, D), np.nan, np.float32)
    scalar = np.full((2, P, 2), np.nan, np.float32)
    status = np.zeros(P, np.int32)
    with np.errstate(all="ignore"):
        for s, (res, mask) in enumerate(((res_a, mask_a), (res_b, mask_b))):
            for p in range(P):
                scalar[s, p] = res[p].min(), res[p].max()
                for c in range(D):
                    x = res[p, :, :, c]
                    image[s, p, 0, c], image[s, p, 1, c] = np.min(x), np.max(x)
                    if mask is not None:
                        y = x * (mask[p] != 0)
                        y = y[np.nonzero(y)]
                        if y.size:
                            image[s, p, 2, c], image[s, p, 3, c] = np.min(y), np.max(y)
                        else:
                            status[p] |= 1
    pair = np.empty((P, 4, D), np.float32)
    for p in range(P):
        for k in range(4):
            for c in range(D):
                a, b = image[0, p, k, c], image[1, p, k, c]
                pair[p, k, c] = (max if k & 1 else min)(a, b)            # Python's: b only if the comparison with a holds
    return image, pair, scalar, status


def _m(mask):
    return (mask != 0).astype(np.uint8)[..., None]


def np_pair(res, pair, rows=0):
    with np.errstate(all="ignore"):
        mn, mx = pair[:, None, None, rows], pair[:, None, None, rows + 1]
        out = (res - mn) / (mx - mn)
    assert out.dtype == np.float32
    return out


def np_masked(res, mask, pair):
    with np.errstate(all="ignore"):
        out = np_pair(res, pair, 2) * _m(mask)
    assert out.dtype == np.float32
    return out


def np_scalar(res, scalar):
    with np.errstate(all="ignore"):
        mn, mx = scalar[:, None, None, None, 0], scalar[:, None, None, None, 1]
        out = (res - mn) / ((mx - mn) + np.float32(1e-10))
    assert out.dtype == np.float32
    return out


def np_stats(res, stats, mask=None):
    """stats float64 [2, D]"""
    with np.errstate(all="ignore"):
        x = res if mask is None else res * _m(mask)
        assert x.dtype == np.float32
        v = np.clip(x.astype(np.float64), stats[0], stats[1])
        out = (v - stats[0]) / ((stats[1] - stats[0]) + 1e-10)
        if mask is not None:
            out = out * _m(mask)
    assert out.dtype == np.float64
    return out


def np_picture(v, channels):
    """uint8(255 * clip(v, 0, 1)) in the precision of v, truncated; 0 for NaN.  One channel: the plane"""
    v = v[..., list(channels)]
    with np.errstate(all="ignore"):
        t = v.dtype.type(255) * np.clip(v, 0, 1)
    assert t.dtype == v.dtype
    out = np.where(np.isnan(t), 0, t).astype(np.uint8)
    return out[..., 0] if len(channels) == 1 else out


def np_heat_reference(norm_diffs, variance):
    """visualization.py:27-31 in numpy's own float32"""
    heatmap = np.copy(norm_diffs)
    heatmap = np.exp(-heatmap / variance)
    heatmap *= 255
    return heatmap.astype(np.uint8)


def np_all(res_a, res_b, mask_a, mask_b, stats_full, stats_mask):
    """Every normalisation of a batch of pairs -> ({kind: float [2, P, H, W, D]}, ranges)"""
    image, pair, scalar, status = np_ranges(res_a, res_b, mask_a, mask_b)
    out = {"pair": np.stack([np_pair(res_a, pair), np_pair(res_b, pair)]),
           "masked": np.stack([np_masked(res_a, mask_a, pair), np_masked(res_b, mask_b, pair)]),
           "scalar": np.stack([np_scalar(res_a, scalar[0]), np_scalar(res_b, scalar[1])]),
           "stats": np.stack([np_stats(res_a, stats_full), np_stats(res_b, stats_full)]),
           "stats_masked": np.stack([np_stats(res_a, stats_mask, mask_a), np_stats(res_b, stats_mask, mask_b)])}
    return out, (image, pair, scalar, status)


# ---- running the kernels ----------------------------------------------------------------------------------------------------
def run_all(z, device, channels):
    """Every normalisation through the public functions, normed and picture at once -> {kind: (normed, picture)}, ranges"""
    from dcn_hip import evaluate as ev
    ra, rb, ma, mb = (dev_t(z[k], device) for k in ("res_a", "res_b", "mask_a", "mask_b"))
    full = {"min": z["stats_full"][0].tolist(), "max": z["stats_full"][1].tolist()}
    under = {"min": z["stats_mask"][0].tolist(), "max": z["stats_mask"][1].tolist()}
    want = ("normed", "picture")
    got = {}
    r = ev.normalize_descriptor_pair(ra, rb, want=want, channels=channels)
    got["pair"] = (host(r.normed), host(r.picture))
    r = ev.normalize_masked_descriptor_pair(ra, rb, ma, mb, want=want, channels=channels)
    got["masked"] = (host(r.normed), host(r.picture))
    ranges = tuple(host(t) for t in r.ranges)
    assert np.array_equal(host(r.status), ranges[3])
    sides = [ev.normalize_descriptor(x, None, want=want, channels=channels) for x in (ra, rb)]
    got["scalar"] = tuple(np.stack([host(getattr(s, f)) for s in sides]) for f in ("normed", "picture"))
    for s, side in enumerate(sides):                                     # each image's own scalar range
        ranges[2][s] = host(side.ranges.scalar)[0]
    sides = [ev.normalize_descriptor(x, full, want=want, channels=channels) for x in (ra, rb)]
    got["stats"] = tuple(np.stack([host(getattr(s, f)) for s in sides]) for f in ("normed", "picture"))
    sides = [ev.normalize_descriptor(x, under, mask=m, want=want, channels=channels) for x, m in ((ra, ma), (rb, mb))]
    got["stats_masked"] = tuple(np.stack([host(getattr(s, f)) for s in sides]) for f in ("normed", "picture"))
    return got, ranges


def compare_all(got, ranges, want, want_ranges, channels, what):
    """The kernels' outputs against the numpy statement: bits, and bytes wherever the float is not NaN"""
    for name, a, b in zip(("image", "pair", "scalar"), ranges, want_ranges):
        assert same_bits(a, b), (what, name)
    assert np.array_equal(ranges[3], want_ranges[3]), (what, ranges[3], want_ranges[3])
    for kind in KINDS:
        normed, picture = got[kind]
        assert normed.dtype == (np.float64 if kind.startswith("stats") else np.float32), (what, kind, normed.dtype)
        assert same_bits(normed, want[kind]), (what, kind)
        pinned = ~np.isnan(want[kind][..., list(channels)])
        pinned = pinned[..., 0] if len(channels) == 1 else pinned
        wp = np_picture(want[kind], channels)
        assert picture.dtype == np.uint8 and picture.shape == wp.shape, (what, kind, picture.shape, wp.shape)
        assert np.array_equal(picture[pinned], wp[pinned]), (what, kind)
        assert (picture[~pinned] == 0).all(), (what, kind)                # (what this package states for a NaN)


def channels_of(z):
    return tuple(int(c) for c in z["channels"])


def check_golden(name, device):
    """Check 1"""
    from dcn_hip import evaluate as ev
    z = np.load(golden(name))
    ch = channels_of(z)
    D = z["res_a"].shape[3]
    arg = None if D in (1, 3) else ch
    got, ranges = run_all(z, device, arg)
    want, want_ranges = np_all(z["res_a"], z["res_b"], z["mask_a"], z["mask_b"], z["stats_full"], z["stats_mask"])
    compare_all(got, ranges, want, want_ranges, ch, name)
    # ... and the reference's own: the ranges it formed, the digest of its floats (the floats themselves where the fixture has
    # them), matplotlib's bytes
    assert same_bits(ranges[1], z["pair_ranges"]) and np.array_equal(ranges[3], z["status"]), name
    for kind in KINDS:
        normed, picture = got[kind]
        if kind == "masked" and z["status"].any():                       # the reference raised: nothing of it to compare
            assert str(z["masked_sha"]) == "ValueError"
            continue
        assert digest(normed) == str(z[kind + "_sha"]), (name, kind)
        if kind + "_normed" in z.files:
            assert same_bits(normed, z[kind + "_normed"]), (name, kind)
        pinned = ~np.isnan(normed[..., list(ch)])
        pinned = pinned[..., 0] if len(ch) == 1 else pinned
        assert np.array_equal(picture[pinned], z[kind + "_picture"][pinned]), (name, kind)
    # descriptor_pictures: the four pictures in one launch, without and with the stats dict
    ra, rb, ma, mb = (dev_t(z[k], device) for k in ("res_a", "res_b", "mask_a", "mask_b"))
    four = ev.descriptor_pictures(ra, rb, ma, mb, channels=arg)
    assert np.array_equal(host(four.status), z["status"])
    pics = host(four.pictures)
    P = z["res_a"].shape[0]
    assert pics.shape[:3] == (P, 2, 2) and pics.dtype == np.uint8
    ok = z["status"] == 0
    for i, kind in enumerate(("pair", "masked")):
        for s in range(2):
            assert np.array_equal(pics[ok, i, s], got[kind][1][s][ok]), (name, kind, s)
    stats = {"entire_image": {"min": z["stats_full"][0].tolist(), "max": z["stats_full"][1].tolist()},
             "mask_image": {"min": z["stats_mask"][0].tolist(), "max": z["stats_mask"][1].tolist()}}
    four = ev.descriptor_pictures(ra, rb, ma, mb, stats, "entire_image", channels=arg)
    pics = host(four.pictures)
    assert not host(four.status).any() and four.ranges is None
    for i, kind in enumerate(("stats", "stats_masked")):
        for s in range(2):
            assert np.array_equal(pics[:, i, s], got[kind][1][s]), (name, kind, s)
    # the default norm type is the reference's: 'mask_image' for the upper row too
    same = {"entire_image": stats["mask_image"], "mask_image": stats["mask_image"]}
    assert np.array_equal(host(ev.descriptor_pictures(ra, rb, ma, mb, stats, channels=arg).pictures),
                          host(ev.descriptor_pictures(ra, rb, ma, mb, same, "entire_image", channels=arg).pictures))
    if z["status"].any():
        import pytest
        with pytest.raises(ValueError):
            ev.pictures_to_host(ev.descriptor_pictures(ra, rb, ma, mb, channels=arg))


def random_pairs(D):
    """float32 [3, 240, 320, D] twice (several workgroups per image at every D) and partial masks; one draw shared by all D"""
    if "base" not in _cache:
        rng = np.random.RandomState(11)
        base = (rng.standard_normal((2, 3, 240, 320, 64)) * 1.5 + 0.25).astype(np.float32)
        ys, xs = np.mgrid[0:240, 0:320]
        mask = np.stack([np.stack([((xs - 150 - 20 * i - 9 * s) ** 2 + (ys - 110) ** 2 < (60 + 15 * i) ** 2)
                                   for i in range(3)]) for s in range(2)]).astype(np.uint8)
        mask[1, 2, -1, -1] = 3                                           # (the very last pixel; any non-zero value counts)
        base[0, 1, 100, 150, :] = 0.0                                    # exact zeros under a mask, in every channel
        _cache["base"] = (base, mask)
    base, mask = _cache["base"]
    return (np.ascontiguousarray(base[0][..., :D]), np.ascontiguousarray(base[1][..., :D]), mask[0], mask[1])


def check_statement(D, device):
    """Check 2: 240 x 320, P = 3 against the numpy statement, two runs bit-identical.  The ranges over every channel; the
    pair normalisations (one launch: float images and pictures) at every D, the stats and scalar forms where D is 1 or 3."""
    from dcn_hip import evaluate as ev
    res_a, res_b, mask_a, mask_b = random_pairs(D)
    assert bool(mask_a[1, 100, 150]) and 0 < (mask_a != 0).sum() < mask_a.size
    ch = tuple(range(D)) if D in (1, 3) else (D - 1, 0, D // 2)
    arg = None if D in (1, 3) else ch
    ra, rb, ma, mb = (dev_t(x, device) for x in (res_a, res_b, mask_a, mask_b))
    want_ranges = np_ranges(res_a, res_b, mask_a, mask_b)
    runs = []
    for _ in range(2):
        r = ev.descriptor_ranges(ra, rb, ma, mb)
        m = ev.normalize_masked_descriptor_pair(ra, rb, ma, mb, want=("normed", "picture"), channels=arg)
        four = ev.descriptor_pictures(ra, rb, ma, mb, channels=arg)
        runs.append([host(t) for t in r] + [host(m.normed), host(m.picture), host(four.pictures)])
    for a, b in zip(*runs):
        assert same_bits(a, b) if a.dtype.kind == "f" else np.array_equal(a, b)
    image, pair, scalar, status, normed, picture, four = runs[0]
    for name, a, b in zip(("image", "pair", "scalar"), (image, pair, scalar), want_ranges):
        assert same_bits(a, b), (D, name)
    assert not status.any() and not want_ranges[3].any()
    want = np.stack([np_masked(res_a, mask_a, pair), np_masked(res_b, mask_b, pair)])
    assert same_bits(normed, want) and np.isfinite(want).all()
    assert np.array_equal(picture, np_picture(want, ch))
    assert np.array_equal(four[:, 1], np.moveaxis(picture, 0, 1))
    full = np.stack([np_pair(res_a, pair), np_pair(res_b, pair)])
    assert np.array_equal(four[:, 0], np.moveaxis(np_picture(full, ch), 0, 1))
    if D in (1, 3):
        z = dict(res_a=res_a, res_b=res_b, mask_a=mask_a, mask_b=mask_b,
                 stats_full=np.stack([np.full(D, -1.25), np.full(D, 2.0)]) + np.arange(D) * 0.125,
                 stats_mask=np.stack([np.full(D, -0.75), np.full(D, 1.5)]) - np.arange(D) * 0.0625)
        got, ranges = run_all(z, device, None)
        want_all, want_r = np_all(res_a, res_b, mask_a, mask_b, z["stats_full"], z["stats_mask"])
        compare_all(got, ranges, want_all, want_r, ch, "240x320 D=%d" % D)


# ---- heat maps ------------------------------------------------------------------------------------------------------------------
def heat_reference(res_b, queries, offsets, variance, device):
    """The reference formula on the distances ``match.find_best_matches(..., return_norm_diffs=True)`` returns"""
    from dcn_hip import match
    planes = []
    for p in range(res_b.shape[0]):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        if hi > lo:
            nd = match.find_best_matches(dev_t(res_b[p], device), dev_t(queries[lo:hi], device), return_norm_diffs=True)[2]
            planes.append(np_heat_reference(nd.cpu().numpy(), variance))
    return np.concatenate(planes)


def heat_close(got, want, what):
    """Every byte within one level, at most 0.1 % of a plane's bytes different at all; prints the observed count"""
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32)).reshape(got.shape[0], -1)
    differing = (diff != 0).sum(1)
    print("%s: %d of %d bytes differ from the reference formula, largest difference %d level(s)"
          % (what, int(differing.sum()), diff.size, int(diff.max()) if diff.size else 0))
    assert diff.max() <= HEAT_MAX_LEVELS, what
    assert (differing <= HEAT_MAX_FRACTION * diff.shape[1]).all(), (what, differing.tolist(), diff.shape[1])


def run_heat(res_b, queries, offsets, variance, device, table=None):
    from dcn_hip import evaluate as ev
    out = ev.heat_maps(dev_t(res_b, device), dev_t(queries, device), dev_t(np.asarray(offsets, np.int64), device), variance,
                       None if table is None else table.to(device))
    assert not out.status.cpu().any()
    return out.maps.cpu().numpy()


def check_heat_golden(name, device):
    """Check 3 on the goldens: the reference's own uint8 plane"""
    from dcn_hip import evaluate as ev
    z = np.load(golden(name))
    table = ev.colour_table()
    for i, variance in enumerate(z["variances"].tolist()):
        got = run_heat(z["res_b"], z["queries"], z["offsets"], variance, device)
        heat_close(got, z["planes"][i], "%s variance %g, the golden plane" % (name, variance))
        heat_close(got, heat_reference(z["res_b"], z["queries"], z["offsets"], variance, device),
                   "%s variance %g, find_best_matches' distances" % (name, variance))
        coloured = run_heat(z["res_b"], z["queries"], z["offsets"], variance, device, table)
        assert np.array_equal(coloured, table.numpy()[got])


HEAT_CASES = {  # name: (h, w, d, rows per pair)
    "37x53_d3": (37, 53, 3, (2, 3)), "37x53_d8": (37, 53, 8, (3, 2)), "37x53_d16": (37, 53, 16, (1, 4)),
    "37x53_d5": (37, 53, 5, (4, 1)), "1x64_d1": (1, 64, 1, (2, 3)), "48x1_d1": (48, 1, 1, (3, 2)),
    "240x320_d3": (240, 320, 3, (40, 40)), "9x7_d3_70_rows": (9, 7, 3, (70, 0, 3)),
}


def check_heat(case, device):
    """Check 3 on shapes of every path: 16, 8 and 4 pixels per work-item and the any-D path; 37 x 53 with 5 rows (a row's plane
    starts on every byte offset of a dword; full and partial segments); one row and one column of pixels; 240 x 320 with 2 pairs
    of 40 rows (several workgroups per image, a group wider than one wavefront); more rows than are staged at a time, next to a
    pair without rows.  With a colour table: table[plane], exactly.  Rows from offsets[P] on are left untouched."""
    from dcn_hip import evaluate as ev
    h, w, d, rows = HEAT_CASES[case]
    rng = np.random.RandomState(len(case) + h)
    P = len(rows)
    res_b = (rng.standard_normal((P, h, w, d)) * (0.35 / np.sqrt(d))).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    R = int(offsets[-1])
    pick = rng.randint(0, h * w, R)
    queries = np.stack([res_b[np.searchsorted(offsets, r, side="right") - 1].reshape(h * w, d)[pick[r]] for r in range(R)])
    queries[::2] += (rng.standard_normal((len(queries[::2]), d)) * 0.05).astype(np.float32)
    variance = 0.25
    got = run_heat(res_b, queries, offsets, variance, device)
    assert got.shape == (R, h, w)
    heat_close(got, heat_reference(res_b, queries, offsets, variance, device), case)
    assert (got.reshape(R, -1)[np.arange(1, R, 2), pick[1::2]] == 255).all()    # a query's own pixel: distance 0
    assert got.min() < 128                                                 # (the plane is not saturated)
    again = run_heat(res_b, queries, offsets, variance, device)
    assert np.array_equal(got, again)
    table = ev.colour_table()
    coloured = run_heat(res_b, queries, offsets, variance, device, table)
    assert coloured.shape == (R, h, w, 3) and np.array_equal(coloured, table.numpy()[got])
    # rows past offsets[P]: two more query rows than the offsets use -- the first R planes are the same
    more = np.concatenate([queries, queries[:2]])
    assert np.array_equal(run_heat(res_b, more, offsets, variance, device)[:R], got)
    # another variance changes the plane as the formula says
    other = run_heat(res_b, queries, offsets, 0.1, device)
    heat_close(other, heat_reference(res_b, queries, offsets, 0.1, device), case + " variance 0.1")
    assert not np.array_equal(other, got)


def check_colour_table():
    from dcn_hip import evaluate as ev
    import matplotlib
    t = ev.colour_table()
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 3) and not t.is_cuda and ev.colour_table() is t
    jet = matplotlib.colormaps["jet"]
    assert np.array_equal(t.numpy(), np.array([jet(i, bytes=True)[:3] for i in range(256)], np.uint8))
    assert not np.array_equal(ev.colour_table("viridis").numpy(), t.numpy())


# ---- EMPTY_RANGE ------------------------------------------------------------------------------------------------------------------
def check_empty_range(device):
    """Check 4: an empty mask in one pair of two flags that pair only; the other pair's outputs are those of a call without it"""
    import pytest
    from dcn_hip import evaluate as ev
    rng = np.random.RandomState(2)
    res_a, res_b = (rng.standard_normal((2, 19, 23, 3)).astype(np.float32) for _ in range(2))
    mask_a, mask_b = (np.zeros((2, 19, 23), np.uint8) for _ in range(2))
    mask_a[:, 3:12, 4:20] = 1
    mask_b[:, 5:15, 2:18] = 1
    mask_b[1] = 0                                                        # pair 1, image b: nothing under the mask
    t = lambda *xs: [dev_t(x, device) for x in xs]
    both = ev.normalize_masked_descriptor_pair(*t(res_a, res_b, mask_a, mask_b), want=("normed", "picture"))
    assert host(both.status).tolist() == [0, ev.EMPTY_RANGE]
    with pytest.raises(ValueError, match="zero-size array"):
        ev.pictures_to_host(both)
    four = ev.descriptor_pictures(*t(res_a, res_b, mask_a, mask_b))
    assert host(four.status).tolist() == [0, ev.EMPTY_RANGE]
    with pytest.raises(ValueError, match="pair 1"):
        ev.pictures_to_host(four)
    alone = ev.normalize_masked_descriptor_pair(*t(res_a[:1], res_b[:1], mask_a[:1], mask_b[:1]), want=("normed", "picture"))
    assert host(alone.status).tolist() == [0]
    assert same_bits(host(both.normed)[:, :1], host(alone.normed)) and np.isfinite(host(alone.normed)).all()
    assert np.array_equal(host(both.picture)[:, :1], host(alone.picture))
    assert np.array_equal(host(four.pictures)[:1], host(ev.descriptor_pictures(*t(res_a[:1], res_b[:1], mask_a[:1],
                                                                                  mask_b[:1])).pictures))
    got = ev.pictures_to_host(alone)                                     # one copy: numpy arrays, the same values
    assert isinstance(got.normed, np.ndarray) and same_bits(got.normed, host(alone.normed))
    assert same_bits(got.ranges.pair, host(alone.ranges.pair)) and np.array_equal(got.picture, host(alone.picture))
    # a channel that is zero under the mask (a "dead" channel) is empty too
    dead = res_a.copy()
    dead[0, :, :, 2] *= (mask_a[0] == 0)
    assert host(ev.descriptor_ranges(*t(dead, res_b, mask_a, mask_b)).status).tolist() == [ev.EMPTY_RANGE, ev.EMPTY_RANGE]
    # the unmasked normalisations know no empty range
    assert not host(ev.normalize_descriptor_pair(*t(res_a, res_b)).status).any()


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def check_argument_errors(device, on_emulation):
    """Check 5"""
    import pytest
    from dcn_hip import evaluate as ev
    z = lambda *shape, **kw: torch.zeros(shape, device=device, **kw)
    ok, ok_mask = torch.rand((2, 5, 7, 3), device=device), torch.ones((2, 5, 7), dtype=torch.uint8, device=device)
    stats = {"min": [0.0] * 3, "max": [1.0] * 3}
    ev.normalize_descriptor(ok, stats, mask=ok_mask, want=("normed", "picture"))
    ev.normalize_masked_descriptor_pair(ok, ok, ok_mask, ok_mask.bool(), want="picture")
    bad_calls = [
        lambda: ev.normalize_descriptor(z(2, 5, 7, 0)), lambda: ev.normalize_descriptor(z(2, 5, 7, 65)),      # D = 0, D = 65
        lambda: ev.normalize_descriptor_pair(z(2, 5, 7, 0), z(2, 5, 7, 0)),
        lambda: ev.normalize_descriptor_pair(z(2, 5, 7, 65), z(2, 5, 7, 65)),
        lambda: ev.descriptor_pictures(z(2, 5, 7, 65), z(2, 5, 7, 65), ok_mask, ok_mask),
        lambda: ev.normalize_descriptor_pair(ok, ok[:1]), lambda: ev.normalize_descriptor_pair(ok, ok[:, :, :-1]),   # shapes
        lambda: ev.normalize_descriptor_pair(ok[0], ok[0]),
        lambda: ev.normalize_masked_descriptor_pair(ok, ok, ok_mask, ok_mask[:, :-1]),
        lambda: ev.normalize_masked_descriptor_pair(ok, ok, ok_mask[:1], ok_mask),
        lambda: ev.descriptor_pictures(ok, ok, ok_mask, ok_mask[:, :, :-1]),
        lambda: ev.normalize_descriptor(ok, stats, mask=ok_mask[:1]),
        lambda: ev.normalize_descriptor(ok.double()), lambda: ev.normalize_descriptor_pair(ok, ok.half()),          # dtypes
        lambda: ev.normalize_masked_descriptor_pair(ok, ok, ok_mask.float(), ok_mask),
        lambda: ev.descriptor_pictures(ok, ok, ok_mask, ok_mask.to(torch.int32)),
        lambda: ev.normalize_descriptor(ok, {"min": [0.0] * 2, "max": [1.0] * 2}),                                  # stats
        lambda: ev.normalize_descriptor(ok, {"min": [0.0] * 3}), lambda: ev.normalize_descriptor(ok, None, mask=ok_mask),
        lambda: ev.descriptor_pictures(ok, ok, ok_mask, ok_mask, {"mask_image": stats}, "entire_image"),
        lambda: ev.normalize_descriptor(ok, want=()), lambda: ev.normalize_descriptor(ok, want=("bytes",)),         # want
        lambda: ev.normalize_descriptor(z(2, 5, 7, 2), want=("picture",)),                         # D = 2 pictures, no channels
        lambda: ev.normalize_descriptor_pair(z(2, 5, 7, 2), z(2, 5, 7, 2), want=("normed", "picture")),
        lambda: ev.descriptor_pictures(z(2, 5, 7, 2), z(2, 5, 7, 2), ok_mask, ok_mask),
        lambda: ev.normalize_descriptor(ok, want=("picture",), channels=(0, 1)),
        lambda: ev.normalize_descriptor(ok, want=("picture",), channels=(0, 1, 3)),
        lambda: ev.normalize_descriptor(ok, want=("picture",), channels=(0, -1, 2)),
    ]
    q, off = z(4, 3), torch.tensor([0, 2, 4], device=device)
    table = torch.zeros((256, 3), dtype=torch.uint8, device=device)
    ev.heat_maps(ok, q, off, colour_table=table)
    bad_calls += [
        lambda: ev.heat_maps(z(2, 5, 7, 0), z(4, 0), off), lambda: ev.heat_maps(z(2, 5, 7, 65), z(4, 65), off),
        lambda: ev.heat_maps(ok, z(4, 2), off), lambda: ev.heat_maps(ok, q.double(), off), lambda: ev.heat_maps(ok, q, off[:2]),
        lambda: ev.heat_maps(ok, q, off.to(torch.int32)), lambda: ev.heat_maps(ok[0], q, off),
        lambda: ev.heat_maps(ok, q, off, variance=0.0), lambda: ev.heat_maps(ok, q, off, variance=-1.0),
        lambda: ev.heat_maps(ok, q, off, colour_table=table[:255]),                              # a table of the wrong shape
        lambda: ev.heat_maps(ok, q, off, colour_table=table.t().contiguous()),
        lambda: ev.heat_maps(ok, q, off, colour_table=table.float()),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            print("call %d raised nothing" % i)
    # D = 2 with channels is fine, and so is a picture of one channel
    assert tuple(ev.normalize_descriptor(z(2, 5, 7, 2), want="picture", channels=(0, 1, 1)).picture.shape) == (2, 5, 7, 3)
    assert tuple(ev.normalize_descriptor(z(2, 5, 7, 1), want="picture").picture.shape) == (2, 5, 7)
    # bad offsets are a status bit, read with the result
    out = ev.heat_maps(ok, q, torch.tensor([0, 3, 2], device=device))
    assert int(out.status.cpu()[0]) & ev.BAD_OFFSETS
    with pytest.raises(RuntimeError):
        ev.pictures_to_host(out)
    if not on_emulation:                                                 # CPU tensors passed to the device library
        for call in (lambda: ev.normalize_descriptor(ok.cpu()), lambda: ev.normalize_descriptor_pair(ok, ok.cpu()),
                     lambda: ev.normalize_masked_descriptor_pair(ok, ok, ok_mask.cpu(), ok_mask),
                     lambda: ev.descriptor_pictures(ok.cpu(), ok.cpu(), ok_mask.cpu(), ok_mask.cpu()),
                     lambda: ev.descriptor_ranges(ok.cpu()), lambda: ev.heat_maps(ok, q.cpu(), off),
                     lambda: ev.heat_maps(ok.cpu(), q.cpu(), off.cpu()), lambda: ev.heat_maps(ok, q, off, colour_table=table.cpu())):
            with pytest.raises(ValueError):
                call()


# ---- the pair choice --------------------------------------------------------------------------------------------------------------
def check_choose_pairs(device):
    """Check 6"""
    import evaluate_common as ec
    from dcn_hip import evaluate as ev
    assert ev.choose_qualitative_pairs(ec.synthetic_store(device, 8, 12), 9, np.random.RandomState(5)).shape == (0, 3)
    store = wide_store(device, 8, 12)                                    # (6 cm between frames is no different pose)
    got = ev.choose_qualitative_pairs(store, 60, np.random.RandomState(5))
    assert got.dtype == np.int64 and got.shape[1] == 3 and 0 < got.shape[0] < 60      # (the still scene yields no pair)
    assert np.array_equal(got, ev.choose_qualitative_pairs(store, 60, np.random.RandomState(5)))
    assert not np.array_equal(got, ev.choose_qualitative_pairs(store, 60, np.random.RandomState(6)))
    first = np.asarray(store.scene_first_frame_host)
    poses = np.asarray(store.poses_host).reshape(-1, 4, 4)
    for s, a, b in got.tolist():
        assert first[s] <= a < first[s + 1] and first[s] <= b < first[s + 1]          # a and b lie in one scene
        c = min(1.0, max(-1.0, (np.trace(poses[a, :3, :3].T @ poses[b, :3, :3]) - 1.0) * 0.5))
        assert np.linalg.norm(poses[a, :3, 3] - poses[b, :3, 3]) > 0.2 or 2.0 * np.arccos(c) > 20, (s, a, b)
    assert ev.choose_qualitative_pairs(store, 5, np.random.default_rng(1)).shape[1] == 3
    one = ev.choose_qualitative_pairs(store, 40, np.random.RandomState(3), one_scene=True)
    assert len(set(one[:, 0].tolist())) <= 1
    seen = set()
    for seed in range(12):
        seen |= set(ev.choose_qualitative_pairs(store, 8, np.random.RandomState(seed), one_scene=True)[:, 0].tolist())
    assert len(seen) > 1                                                  # (one scene per call, not one scene ever)
    # a store whose scenes have a single pose yields no pair
    still = ec.synthetic_store(device, 8, 12)
    still.poses_host = np.broadcast_to(np.eye(4), np.asarray(store.poses_host).shape).copy()
    assert ev.choose_qualitative_pairs(still, 7, np.random.RandomState(0)).shape == (0, 3)
    # the scene rule is choose_pairs': the same generator state gives the same first scene
    for seed in range(6):
        a = ev.choose_qualitative_pairs(store, 1, np.random.RandomState(seed))
        b = ev.choose_pairs(store, 1, np.random.RandomState(seed), threshold=-1.0)
        one = ev.choose_qualitative_pairs(store, 1, np.random.RandomState(seed), one_scene=True)
        if len(a):
            assert a[0, 0] == b[0, 0]
        if len(one):
            assert one[0, 0] == b[0, 0]


# ---- the whole call ---------------------------------------------------------------------------------------------------------------
def wide_store(device, h, w):
    """evaluate_common.synthetic_store with its HOST poses -- all the pair choice reads -- spread from 6 cm to 25 cm steps: the
    rule of get_img_idx_with_different_pose wants more than 0.2 m (or 20 radians), which no two frames of that store are apart.
    The frames of its still scene keep one pose: a pair drawn there has no b and is dropped."""
    import evaluate_common as ec
    store = ec.synthetic_store(device, h, w)
    store.poses_host = np.asarray(store.poses_host, np.float64).copy()
    store.poses_host[:, :3, 3] *= 0.25 / 0.06
    return store


def check_whole_call(device, h, w, dcn, tmp_path):
    """Check 7: ``evaluate_network_qualitative(num_image_pairs=3, num_matches=4, heat_variance=0.25, save_to=tmp)`` against the
    same pieces called one after another on the same frames."""
    import csv
    from PIL import Image
    import dense_correspondence_manipulation.utils.utils as utils
    from dcn_hip import augment, evaluate as ev
    store = wide_store(device, h, w)
    dev = torch.device(device)
    dcn.config = {}
    dcn._descriptor_image_stats = None
    dcn.train()
    order = np.array([[0, 5, 17, 11], [3, 2, 1, 0], [20, 9, 4, 30]])
    out_dir = tmp_path / "pair_normalisation"
    # a generator state whose three draws all find a different pose (a draw in the still scene is dropped)
    seed = next(s for s in range(64) if ev.choose_qualitative_pairs(store, 3, np.random.RandomState(s)).shape[0] == 3)
    chosen = ev.choose_qualitative_pairs(store, 3, np.random.RandomState(seed))
    got = ev.evaluate_network_qualitative(dcn, store, num_image_pairs=3, num_matches=4, host_rng=np.random.RandomState(seed),
                                          sample_order=order, heat_variance=0.25, save_to=str(out_dir))
    assert dcn.training
    assert np.array_equal(got.pairs, chosen)
    D = dcn.descriptor_dimension
    assert tuple(got.pictures.shape) == (3, 2, 2, h, w, 3) and got.pictures.dtype == torch.uint8 and D == 3
    assert got.offsets.cpu().tolist() == [0, 4, 8, 12] and not got.status.cpu().any() and not got.chain_status.cpu().any()

    def pieces(stats):
        fa, fb = (torch.from_numpy(chosen[:, k]).to(dev) for k in (1, 2))
        zeros = torch.zeros((6, augment.PARAM_WORDS), dtype=torch.int32, device=dev)
        was = dcn.training
        dcn.eval()
        x = augment.augment_images(store.rgb[fa], store.mask[fa], zeros, want_mask=False, rgb_b=store.rgb[fb],
                                   mask_b=store.mask[fb])
        res = dcn.forward_image_tensors(torch.cat([x["input_a"], x["input_b"]]))
        dcn.train(was)
        res_a, res_b = res[:3].contiguous(), res[3:].contiguous()
        q = ev.across_object_queries(store.mask[fa], res_a, 4, sample_order=order)
        m = ev.best_match_pairs(res_b, q.queries, q.offsets)
        pics = ev.descriptor_pictures(res_a, res_b, store.mask[fa], store.mask[fb], stats)
        heat = ev.heat_maps(res_b, q.queries, q.offsets, 0.25)
        return q, m, pics, heat
    q, m, pics, heat = pieces(None)
    assert torch.equal(got.pictures, pics.pictures) and torch.equal(got.heat_maps, heat.maps)        # byte-equal
    assert torch.equal(got.u_a, q.u_a) and torch.equal(got.v_a, q.v_a) and torch.equal(got.best_uv, m.best_uv)
    assert torch.equal(got.norm_diff, m.norm_diff_descriptor_best_match) and not torch.isnan(got.norm_diff).any()
    # the pictures show something: neither row is one colour, and the masked row is black outside the masks
    pic = got.pictures.cpu().numpy()
    assert all(len(np.unique(pic[k, i, s])) > 8 for k in range(3) for i in range(2) for s in range(2))
    outside = store.mask[torch.from_numpy(chosen[:, 1]).to(dev)].cpu().numpy() == 0
    assert (pic[:, 1, 0][outside] == 0).all()
    # the files: the PNGs decode to the returned pictures, matches.csv has the returned rows
    names = sorted(os.listdir(str(out_dir)))
    assert names == sorted(["%d_%s_%s.png" % (k, s, kind) for k in range(3) for s in "ab" for kind in ("full", "masked")]
                           + ["matches.csv"])
    for k in range(3):
        for i, kind in enumerate(("full", "masked")):
            for j, side in enumerate("ab"):
                decoded = np.array(Image.open(str(out_dir / ("%d_%s_%s.png" % (k, side, kind)))))
                assert np.array_equal(decoded, pic[k, i, j])
    with open(str(out_dir / "matches.csv")) as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == ev.QUALITATIVE_COLUMNS and len(rows) == 1 + 12
    ua, va, uv, nd = got.u_a.cpu().numpy(), got.v_a.cpu().numpy(), got.best_uv.cpu().numpy(), got.norm_diff.cpu().numpy()
    for r, row in enumerate(rows[1:]):
        p = r // 4
        assert row[0] == row[1] == str(store.scene_names[chosen[p, 0]])
        first = store.scene_first_frame_host[chosen[p, 0]]
        assert [int(x) for x in row[2:4]] == [int(store.frame_ids[chosen[p, 0]][chosen[p, k] - first]) for k in (1, 2)]
        assert [int(x) for x in row[4:8]] == [ua[r], va[r], uv[0, r], uv[1, r]]
        assert np.float32(float(row[8])) == nd[r]
    # given pairs, no heat maps, nothing saved; eval mode stays eval mode
    dcn.eval()
    again = ev.evaluate_network_qualitative(dcn, store, num_matches=4, pairs=chosen[:, 1:], sample_order=order)
    assert not dcn.training and again.heat_maps is None and torch.equal(again.pictures, got.pictures)
    assert np.array_equal(again.pairs, chosen)
    # with descriptor_statistics.yaml in the network's folder the stats normalisation is taken
    folder = tmp_path / "network"
    folder.mkdir()
    stats = {"entire_image": {"min": [-0.5, -0.25, -1.0], "max": [0.5, 0.75, 0.25], "mean": [0.0] * 3},
             "mask_image": {"min": [-0.25, -0.125, -0.5], "max": [0.25, 0.5, 0.125], "mean": [0.0] * 3}}
    top = float(torch.cat([q.queries.abs().view(-1)]).max())
    stats = {k: {f: [x * top for x in v] for f, v in s.items()} for k, s in stats.items()}
    utils.saveToYaml(stats, str(folder / "descriptor_statistics.yaml"))
    dcn.config = {"path_to_network_params_folder": str(folder)}
    dcn._descriptor_image_stats = None
    with_stats = ev.evaluate_network_qualitative(dcn, store, num_matches=4, pairs=chosen, sample_order=order)
    assert torch.equal(with_stats.pictures, pieces(dcn.descriptor_image_stats)[2].pictures)
    assert not torch.equal(with_stats.pictures, got.pictures)
    assert torch.equal(with_stats.best_uv, got.best_uv)
