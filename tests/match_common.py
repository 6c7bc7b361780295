"""Shared by tests/test_emu_match.py and tests/test_gpu_match.py: the four best-match searches (match.find_best_matches,
match.match_statistics, evaluate.best_match_pairs, evaluate.match_statistics_pairs) against the reference's own formula,

    norm_diffs = np.sqrt(np.sum(np.square(res_b - d), axis=2));  np.argmin (first occurrence)

Tier 1: inputs on which fp32 arithmetic does not depend on the summation order or on fused multiply-adds (``reference``
asserts that), so numpy in float32 IS the answer, bit for bit, and minima tie all the time: small integer lattices at three
scales, one image that mixes the scales, one whose squared distances all overflow, and images with two pixels whose squared
distances differ while their norms are equal.  Tier 2: random normal data at every descriptor width against float64, with a
bound from the arithmetic.

Not covered: NaN descriptors (np.argmin returns the first NaN; the kernels never choose a NaN while any number exists) and
subnormal squared distances."""
import collections
import zlib

import numpy as np
import torch

import evaluate_common as ec

F32, F64 = np.float32, np.float64
SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 255: (15, 17), 256: (16, 16), 257: (257, 1), 713: (23, 31), 2072: (37, 56)}
SCALES = {"1": 1.0, "2^-30": 2.0 ** -30, "2^30": 2.0 ** 30}
PAIR_TAIL = 5              # rows of the last pair in the pair kernels' batches (the first has q2, the middle one none)

# (m1, m2) first, then (m3, m4), in units of 2^-12: the first has the larger squared distance to the origin, both have the same
# fp32 norm
EQUAL_NORM_PAIRS = (((2728, 973), (2474, 1506)), ((2365, 1672), (2058, 2038)), ((2409, 1608), (2888, 220)))
# pixels of the pair on a 37 x 56 image: one wavefront; two wavefronts of a workgroup; two workgroups of every kernel
# (pair_search_kernel holds 8 pixels per work-item at D = 1, 3, 4: 2048 per workgroup); one work-item of pair_search_kernel
PLACEMENTS = {"wave": (3, 40), "waves": (3, 70), "groups": (5, 2060), "item": (3, 259)}

Case = collections.namedtuple("Case", "name kind res res_a ia mask q1 q2 pair_pixels")


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _mask(kind, h, w, rng):
    m = np.zeros((h, w), np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "one":
        m.reshape(-1)[rng.randint(h * w)] = 1
    elif kind == "rows":
        assert h > 10
        m[10:, :] = 1
    else:
        assert kind == "empty"
    return m


def _lattice_case(d, n, q1, q2, lo, scale, mask):
    name = "lattice_d%d_hw%d_%s_pm%d" % (d, n, scale, lo)
    rng = _rng(name)
    h, w = SHAPES[n]

    def draw():
        if scale == "mixed":     # no zero component: across scales a difference then rounds to the larger operand, exactly
            s = rng.choice(sorted(SCALES.values()), size=(n, 1))
            return (rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=(n, d)) * s).astype(F32)
        return (rng.randint(-lo, lo + 1, (n, d)) * SCALES[scale]).astype(F32)
    if scale == "huge":          # every squared distance overflows: inf everywhere, pixel 0 wins
        res = (rng.choice([-1.0, 1.0], size=(n, d)) * 2.0 ** 70).astype(F32)
        res_a = rng.randint(-lo, lo + 1, (n, d)).astype(F32)
    else:
        res, res_a = draw(), draw()
    ia = rng.randint(0, n, max(q1, q2)).astype(np.int64)
    res_a[ia[0]] = 0.0           # the descriptor of a pixel past the end of the image, were a kernel to let one through
    return Case(name, "lattice_" + scale, res.reshape(h, w, d), res_a.reshape(h, w, d), ia, _mask(mask, h, w, rng), q1, q2,
                None)


def _equal_norm_case(d, last, placement, pair, q1, q2):
    name = "equalnorm_d%d_%s_%s_pair%d" % (d, "last" if last else "first", placement, pair)
    h, w = SHAPES[2072]
    c = d - 2 if last else 0
    res = np.zeros((h * w, d), F32)
    res[:, c:c + 2] = 3.0
    x, y = PLACEMENTS[placement]
    (m1, m2), (m3, m4) = EQUAL_NORM_PAIRS[pair]
    res[x, c:c + 2] = np.array([m1, m2], F32) * F32(2.0 ** -12)
    res[y, c:c + 2] = np.array([m3, m4], F32) * F32(2.0 ** -12)
    mask = np.ones((h, w), np.uint8)
    if pair == 1:
        mask.reshape(-1)[x] = 0                             # the masked search then finds the second pixel
    ia = _rng(name).randint(0, h * w, max(q1, q2)).astype(np.int64)
    return Case(name, "equalnorm", res.reshape(h, w, d), np.zeros((h, w, d), F32), ia, mask, q1, q2, (x, y))


def _tier1_cases():
    out = []
    for row in (
            # D, pixels, Q (single image), Q (first pair), lattice half-width, scale, mask
            (1, 1, 1, 63, 4, "1", "ones"), (1, 256, 32, 64, 4, "2^30", "one"), (1, 2072, 33, 65, 4, "2^-30", "rows"),
            (2, 63, 31, 64, 4, "2^30", "one"), (2, 257, 65, 63, 4, "1", "rows"),
            (3, 1, 31, 63, 4, "1", "ones"), (3, 64, 32, 129, 4, "1", "one"), (3, 713, 33, 65, 4, "2^-30", "rows"),
            (3, 2072, 65, 129, 4, "2^30", "ones"), (3, 713, 31, 63, 4, "mixed", "rows"), (3, 257, 33, 65, 4, "huge", "rows"),
            (4, 255, 33, 65, 4, "1", "rows"), (4, 2072, 31, 63, 4, "mixed", "rows"), (4, 2072, 32, 64, 4, "2^30", "one"),
            (5, 256, 65, 129, 4, "1", "one"), (5, 713, 33, 65, 4, "2^30", "rows"), (5, 713, 31, 63, 4, "2^-30", "ones"),
            (5, 2072, 1, 63, 4, "huge", "rows"),
            (8, 257, 33, 65, 4, "2^-30", "rows"), (8, 2072, 65, 129, 4, "1", "rows"),
            (9, 1, 31, 64, 4, "1", "ones"), (9, 255, 33, 63, 4, "2^30", "rows"),
            (16, 63, 32, 65, 4, "1", "one"), (16, 2072, 33, 129, 4, "2^-30", "rows"), (16, 713, 65, 63, 4, "2^30", "ones"),
            (16, 713, 31, 64, 4, "mixed", "rows"), (16, 256, 1, 63, 4, "huge", "ones"),
            (17, 64, 33, 65, 4, "1", "one"), (17, 713, 65, 129, 4, "2^-30", "rows"),
            (32, 256, 31, 63, 1, "1", "rows"), (32, 2072, 33, 65, 1, "2^30", "rows"), (32, 2072, 32, 64, 4, "1", "one"),
            (33, 255, 33, 65, 1, "1", "rows"), (33, 257, 65, 129, 4, "2^-30", "ones"),
            (64, 63, 31, 63, 1, "1", "one"), (64, 713, 33, 65, 4, "2^30", "rows"), (64, 713, 32, 64, 1, "2^-30", "ones")):
        out.append(_lattice_case(*row))
    q1s, q2s = (1, 31, 32, 33, 65), (63, 64, 65, 129)
    widths = [(2, False), (3, False), (3, True), (4, True), (5, False), (16, True)]
    n = 0
    for placement in ("wave", "waves", "groups", "item"):
        for d, last in widths + ([(8, True)] if placement == "item" else []):
            out.append(_equal_norm_case(d, last, placement, n % 3, q1s[n % 5], q2s[n % 4]))
            n += 1
    return out


TIER1 = _tier1_cases()
TIER1_IDS = [c.name for c in TIER1]
BY_NAME = {c.name: c for c in TIER1}
assert len(BY_NAME) == len(TIER1)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == F32, a.dtype
    return np.ascontiguousarray(a).view(np.int32)


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------------ the reference
Reference = collections.namedtuple("Reference", "queries nd best gt")
_REFERENCES = {}


def reference(case):
    """The reference formula in numpy float32 for all of the case's queries (computed once per case, never written to), and
    the ground-truth pixels the statistics use: pixel 0, the last pixel, a query's own best pixel, then random ones.
    Asserts what makes float32 numpy the answer bit for bit: the sum of squares is the same forwards, backwards, in numpy's
    order and as a chain of fused multiply-adds."""
    if case.name in _REFERENCES:
        return _REFERENCES[case.name]
    h, w, d = case.res.shape
    res = case.res.reshape(-1, d)
    queries = case.res_a.reshape(-1, d)[case.ia]
    with np.errstate(over="ignore"):
        t = res[None, :, :] - queries[:, None, :]
        nd = np.sqrt(np.sum(np.square(t), axis=2))
        fwd, rev, fma = (np.zeros(t.shape[:2], F32) for _ in range(3))
        for k in range(d):
            fwd = fwd + t[..., k] * t[..., k]
            rev = rev + t[..., d - 1 - k] * t[..., d - 1 - k]
            fma = (t[..., k].astype(F64) ** 2 + fma.astype(F64)).astype(F32)    # (the product is exact in float64)
        for other in (fwd, rev, fma):
            assert np.array_equal(bits(np.sqrt(other)), bits(nd)), case.name
    assert nd.dtype == F32 and not np.isnan(nd).any()
    best = nd.argmin(1)
    gt = _rng(case.name + "/gt").randint(0, h * w, len(queries)).astype(np.int64)
    gt[0] = 0
    if len(gt) > 1:
        gt[1] = h * w - 1
    if len(gt) > 2:
        gt[2] = best[2]
    if case.kind.startswith("lattice") and case.kind != "lattice_mixed":       # np.linalg.norm is exact there as well
        with np.errstate(over="ignore"):
            ln = np.array([np.linalg.norm(queries[i] - res[gt[i]]) for i in range(len(gt))], F32)
        assert np.array_equal(bits(ln), bits(nd[np.arange(len(gt)), gt]))
    if case.kind == "lattice_huge":
        assert np.isinf(nd).all() and (best == 0).all()
    if case.kind == "equalnorm":
        x, y = case.pair_pixels
        assert x < y and (queries == 0).all()
        d2 = np.sum(np.square(res), axis=1)
        assert d2[x] > d2[y] and bits(d2[x:x + 1])[0] != bits(d2[y:y + 1])[0]
        assert bits(nd[:, x]).tolist() == bits(nd[:, y]).tolist()
        assert (best == x).all()
        if len(gt) > 3:
            gt[3] = y
        gt[0] = x
    nd.setflags(write=False)
    _REFERENCES[case.name] = Reference(queries, nd, best, gt)
    return _REFERENCES[case.name]


Stats = collections.namedtuple("Stats", "best best_m on_mask gt_dist count count_m sum sum_m pixel_dist")


def stats_reference(nd, gt, mask, w):
    """evaluation.py:1046-1100 on a float32 ``norm_diffs`` [Q, HW]: the masked half in float64, as the reference's
    ``norm_diffs + (1 - mask_b) * 1e6`` is.  Asserts that the float32 replay of that sum orders the pixels the same way
    (it need not where every pixel near the minimum is off the mask), so that the kernels' answer is determined."""
    Q, hw = nd.shape
    rows = np.arange(Q)
    m = mask.reshape(-1) != 0
    g = nd[rows, gt]
    with np.errstate(invalid="ignore"):
        md = nd.astype(F64) + (1.0 - m.astype(F64))[None, :] * 1e6
        md32 = np.where(m[None, :], nd, nd + F32(1e6))
        closer, closer_m = nd < g[:, None], md < g[:, None].astype(F64)
        if m.any():
            assert np.array_equal(md32.argmin(1), md.argmin(1)) and np.array_equal(md32 < g[:, None], closer_m)
    best_m = md.argmin(1)
    u, v = (np.arange(hw) % w).astype(F64), (np.arange(hw) // w).astype(F64)
    pd = np.sqrt((u[None, :] - (gt % w)[:, None]) ** 2 + (v[None, :] - (gt // w)[:, None]) ** 2)
    return Stats(nd.argmin(1), best_m, m[best_m], g, closer.sum(1), closer_m.sum(1), (pd * closer).sum(1),
                 (pd * closer_m).sum(1), pd)


def fixed_point_sum(pd, closer):
    """The kernels' sum of pixel distances: the fp32 distances rounded to 2^-20 pixel, summed as integers (int64 per query)"""
    pf = np.floor(np.sqrt((pd ** 2).astype(F32)).astype(F64) * 1048576.0 + 0.5).astype(np.int64)
    return (pf * closer).sum(1)


def fixed_point_average(pd, closer):
    """evaluate_kernels.hip's column: that sum over the count"""
    total, n = fixed_point_sum(pd, closer), closer.sum(1)
    return np.where(n > 0, total.astype(F64) / 1048576.0 / np.maximum(n, 1), 0.0)


# ------------------------------------------------------------------------------------------------ tier 1 checks
def _masks_for(case):
    h, w, _ = case.res.shape
    rng = _rng(case.name + "/masks")
    out = [("ones", _mask("ones", h, w, rng)), ("one", _mask("one", h, w, rng))]
    if h > 10:
        out.append(("rows", _mask("rows", h, w, rng)))
    return out


def check_find_best_matches(case, device):
    from dcn_hip import match
    r = reference(case)
    Q = case.q1
    nd_ref, best = r.nd[:Q], r.best[:Q]
    res, q = _t(case.res, device), _t(r.queries[:Q], device)
    h, w, _ = case.res.shape
    for with_nd in (True, False):
        idx, dist, nd = match.find_best_matches(res, q, None, with_nd)
        assert np.array_equal(idx.cpu().numpy(), best), (case.name, with_nd)
        assert np.array_equal(bits(dist), bits(nd_ref[np.arange(Q), best])), (case.name, with_nd)
        if with_nd:
            assert tuple(nd.shape) == (Q, h, w)
            got = nd.cpu().numpy().reshape(Q, -1)
            assert np.array_equal(bits(got), bits(nd_ref)), case.name
            assert np.array_equal(idx.cpu().numpy(), got.argmin(1)), case.name    # the first argmin of what the call returns
        else:
            assert nd is None
    for i, (kind, m) in enumerate(_masks_for(case)):
        idx, dist, nd = match.find_best_matches(res, q, _t(m, device), i % 2 == 1)
        # argmin over where(mask, nd, inf), stated over the mask's pixels: the same pixel whenever one of them has a finite
        # distance, and still a pixel of the mask where all of them are inf (the image of +-2^70)
        on = np.nonzero(m.reshape(-1))[0]
        want = on[nd_ref[:, on].argmin(1)]
        if np.isfinite(nd_ref[:, on]).any(1).all():
            assert np.array_equal(want, np.where(m.reshape(-1)[None, :] != 0, nd_ref, F32(np.inf)).argmin(1))
        assert np.array_equal(idx.cpu().numpy(), want), (case.name, kind)
        assert np.array_equal(bits(dist), bits(nd_ref[np.arange(Q), want])), (case.name, kind)
        if nd is not None:
            assert np.array_equal(bits(nd.cpu().numpy().reshape(Q, -1)), bits(nd_ref)), (case.name, kind)
    idx, dist, _ = match.find_best_matches(res, q, _t(np.zeros((h, w), np.uint8), device))
    assert (idx.cpu().numpy() == -1).all() and np.isposinf(dist.cpu().numpy()).all()


def _assert_stats(got, s, nd, name):
    """got: best_idx [2, Q], best_dist [2, Q] float32, count [2, Q], gt_dist [Q] float32 as numpy arrays"""
    rows = np.arange(nd.shape[0])
    best_idx, best_dist, count, gt_dist = got
    assert np.array_equal(best_idx[0], s.best) and np.array_equal(best_idx[1], s.best_m), name
    assert np.array_equal(bits(best_dist[0]), bits(nd[rows, s.best])), name
    on = s.on_mask
    assert np.array_equal(bits(best_dist[1][on]), bits(nd[rows, s.best_m][on])), name
    assert np.array_equal(bits(gt_dist), bits(s.gt_dist)), name
    assert np.array_equal(count[0], s.count) and np.array_equal(count[1], s.count_m), name


def check_match_statistics(case, device):
    from dcn_hip import match
    r = reference(case)
    Q = case.q1
    nd, gt = r.nd[:Q], r.gt[:Q]
    h, w, _ = case.res.shape
    res, q, g = _t(case.res, device), _t(r.queries[:Q], device), _t(gt, device)
    for mask in (case.mask, None):
        s_mask = case.mask if mask is not None else np.ones((h, w), np.uint8)
        s = stats_reference(nd, gt, s_mask, w)
        out = {k: v.cpu().numpy() for k, v in match.match_statistics(res, q, g, None if mask is None else _t(mask, device)).items()}
        _assert_stats((out["best_idx"], out["best_dist"], out["count"], out["gt_dist"]), s, nd, case.name)
        with np.errstate(invalid="ignore"):
            md = nd.astype(F64) + (1.0 - (s_mask.reshape(-1) != 0))[None, :] * 1e6
        closer = (nd < s.gt_dist[:, None], md < s.gt_dist[:, None].astype(F64))
        for half, (n, want) in enumerate(((s.count, s.sum), (s.count_m, s.sum_m))):
            assert (np.abs(out["dist_sum"][half] - want) <= n * 2.0 ** -20 * want).all(), (case.name, half)
            total = fixed_point_sum(s.pixel_dist, closer[half])          # the integer sum, returned as float32(sum / 2^20)
            assert np.array_equal(bits(out["dist_sum"][half]), bits((total.astype(F64) / 1048576.0).astype(F32))), (case.name, half)
        if Q > 2:                                            # the ground truth is the best pixel: nothing is closer
            assert out["count"][0][2] == 0 and out["dist_sum"][0][2] == 0.0
        if mask is None:                                     # both halves equal, the integer sums' float32 bit for bit
            for k in ("best_idx", "best_dist", "count"):
                assert np.array_equal(out[k][0], out[k][1]), (case.name, k)
            assert np.array_equal(bits(out["dist_sum"][0]), bits(out["dist_sum"][1])), case.name
    # Every masked distance is then d + 1e6, so the masked count is 0 only while the ground-truth distances stay below 1e6:
    # not on the lattices scaled by 2^30 (and the mixed one), nor on the image of +-2^70
    if case.kind in ("lattice_1", "lattice_2^-30", "equalnorm"):
        out = match.match_statistics(res, q, g, _t(np.zeros((h, w), np.uint8), device))
        assert (out["count"][1].cpu().numpy() == 0).all()
        idx = out["best_idx"][1].cpu().numpy()
        assert ((idx >= 0) & (idx < h * w)).all()


PairBatch = collections.namedtuple("PairBatch", "res_a res_b mask_b queries offsets ia gt rows")


def pair_batch(case, gt=None, nd=None):
    """Three pairs: the case's image with q2 rows, an image of other values with none, and the case's image with its pixels
    in reverse order with PAIR_TAIL rows.  rows: per pair with rows (pair, first row, norm_diffs, ground truth, mask).
    gt, nd: the ground-truth pixels and the distances [q2, HW] to compare with (default: those of ``reference``)"""
    h, w, d = case.res.shape
    if nd is None:
        ref = reference(case)
        gt, nd = ref.gt, ref.nd
    r = Reference(case.res_a.reshape(-1, d)[case.ia], nd, None, gt)
    n2 = min(PAIR_TAIL, case.q2)
    flip = lambda a: np.ascontiguousarray(a.reshape((h * w,) + a.shape[2:])[::-1]).reshape(a.shape)
    res_b = np.stack([case.res, case.res_a + F32(1.0), flip(case.res)])
    res_a = np.stack([case.res_a] * 3)
    mask_b = np.stack([case.mask, 1 - case.mask, flip(case.mask)])
    Q = case.q2
    queries = np.concatenate([r.queries[:Q], r.queries[:n2]])
    ia = np.concatenate([case.ia[:Q], case.ia[:n2]])
    gt = np.concatenate([r.gt[:Q], h * w - 1 - r.gt[:n2]])
    rows = [(0, 0, r.nd[:Q], r.gt[:Q], case.mask), (2, Q, r.nd[:n2, ::-1], h * w - 1 - r.gt[:n2], flip(case.mask))]
    return PairBatch(res_a, res_b, mask_b, queries, np.array([0, Q, Q, Q + n2], np.int64), ia, gt, rows)


def check_best_match_pairs(case, device):
    from dcn_hip import evaluate
    b = pair_batch(case)
    w = case.res.shape[1]
    m = evaluate.best_match_pairs(_t(b.res_b, device), _t(b.queries, device), _t(b.offsets, device))
    assert int(m.status.cpu()[0]) == 0
    uv, norm, row_pair = m.best_uv.cpu().numpy().astype(np.int64), m.norm_diff_descriptor_best_match.cpu().numpy(), m.row_pair.cpu().numpy()
    for p, lo, nd, _gt, _mask_b in b.rows:
        n = nd.shape[0]
        best = nd.argmin(1)
        assert np.array_equal(uv[1, lo:lo + n] * w + uv[0, lo:lo + n], best), (case.name, p)
        assert np.array_equal(bits(norm[lo:lo + n]), bits(nd[np.arange(n), best])), (case.name, p)
        assert (row_pair[lo:lo + n] == p).all()


def _pair_statistics(case, device, b=None):
    from dcn_hip import evaluate
    b = pair_batch(case) if b is None else b
    h, w, _ = case.res.shape
    rng = _rng(case.name + "/depth")
    depth = _t(rng.randint(0, 2000, (3, h, w)).astype(np.int16), device)
    cams = _t(np.repeat(np.load(ec.GOLDENS[0])["cams"][:1], 3, axis=0), device)
    t = evaluate.match_statistics_pairs(_t(b.res_a, device), _t(b.res_b, device), _t(b.mask_b, device), depth, depth, cams,
                                        _t(b.ia % w, device), _t(b.ia // w, device), _t((b.gt % w).astype(F32), device),
                                        _t((b.gt // w).astype(F32), device), _t(b.offsets, device))
    return b, t


def check_match_statistics_pairs(case, device):
    """Only the descriptor-derived columns (the evalpairs goldens pin the depth and 3D ones)"""
    from dcn_hip import evaluate
    b, t = _pair_statistics(case, device)
    w = case.res.shape[1]
    assert int(t.status.cpu()[0]) == 0
    cols = {k: t.columns.cpu().numpy()[i] for i, k in enumerate(evaluate.COLUMNS)}
    pred, closer, row_pair = t.pred_uv.cpu().numpy().astype(np.int64), t.closer.cpu().numpy(), t.row_pair.cpu().numpy()
    assert np.array_equal(t.mask_pixels.cpu().numpy(), (b.mask_b != 0).reshape(3, -1).sum(1))
    for p, lo, nd, gt, mask_b in b.rows:
        n = nd.shape[0]
        rows = slice(lo, lo + n)
        s = stats_reference(nd, gt, mask_b, w)
        f32 = lambda k: cols[k][rows].astype(F32)
        for k in ("norm_diff_descriptor", "norm_diff_descriptor_masked", "norm_diff_descriptor_ground_truth"):
            assert np.array_equal(f32(k).astype(F64), cols[k][rows]), k             # a float32 value in a float64 column
        best_idx = np.stack([pred[1, rows] * w + pred[0, rows], pred[3, rows] * w + pred[2, rows]])
        _assert_stats((best_idx, np.stack([f32("norm_diff_descriptor"), f32("norm_diff_descriptor_masked")]), closer[:, rows],
                       f32("norm_diff_descriptor_ground_truth")), s, nd, (case.name, p))
        with np.errstate(invalid="ignore"):
            md = nd.astype(F64) + (1.0 - (mask_b.reshape(-1) != 0))[None, :] * 1e6
        for name, c in (("", nd < s.gt_dist[:, None]), ("_masked", md < s.gt_dist[:, None].astype(F64))):
            assert np.array_equal(cols["average_l2_distance_for_false_positives" + name][rows],
                                  fixed_point_average(s.pixel_dist, c)), (case.name, p, name)
        assert (row_pair[rows] == p).all()


def check_four_entry_points_agree(case, device):
    """The same image and queries through all four: one best pixel, one norm, bit for bit"""
    from dcn_hip import evaluate, match
    r = reference(case)
    Q = min(case.q1, case.q2)
    w = case.res.shape[1]
    res, q, g = _t(case.res, device), _t(r.queries[:Q], device), _t(r.gt[:Q], device)
    idx, dist, _ = match.find_best_matches(res, q)
    s = match.match_statistics(res, q, g)
    b, t = _pair_statistics(case, device)
    m = evaluate.best_match_pairs(_t(b.res_b, device), _t(b.queries, device), _t(b.offsets, device))
    want_idx, want_bits = idx.cpu().numpy(), bits(dist)
    assert np.array_equal(want_idx, r.best[:Q])
    uv, pred = m.best_uv.cpu().numpy().astype(np.int64), t.pred_uv.cpu().numpy().astype(np.int64)
    assert np.array_equal(s["best_idx"][0].cpu().numpy(), want_idx) and np.array_equal(bits(s["best_dist"][0]), want_bits)
    assert np.array_equal(uv[1, :Q] * w + uv[0, :Q], want_idx)
    assert np.array_equal(bits(m.norm_diff_descriptor_best_match[:Q]), want_bits)
    assert np.array_equal(pred[1, :Q] * w + pred[0, :Q], want_idx)
    assert np.array_equal(bits(t.column("norm_diff_descriptor")[:Q].float()), want_bits)


def check_run_to_run(case, device):
    """Two consecutive calls of each entry point: identical indices, norm bits and distance sums"""
    from dcn_hip import evaluate, match
    r = reference(case)
    Q = case.q1
    res, q, g, mask = _t(case.res, device), _t(r.queries[:Q], device), _t(r.gt[:Q], device), _t(case.mask, device)
    b = pair_batch(case)

    def calls():
        idx, dist, nd = match.find_best_matches(res, q, None, True)
        s = match.match_statistics(res, q, g, mask)
        m = evaluate.best_match_pairs(_t(b.res_b, device), _t(b.queries, device), _t(b.offsets, device))
        t = _pair_statistics(case, device)[1]
        return [idx, dist, nd, s["best_idx"], s["best_dist"], s["count"], s["dist_sum"], s["gt_dist"], m.best_uv,
                m.norm_diff_descriptor_best_match, t.pred_uv, t.closer, t.column("norm_diff_descriptor"),
                t.column("norm_diff_descriptor_masked"), t.column("average_l2_distance_for_false_positives")]
    for x, y in zip(calls(), calls()):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(x.view(np.uint8 if x.dtype.itemsize == 1 else "i%d" % x.dtype.itemsize),
                              y.view(np.uint8 if y.dtype.itemsize == 1 else "i%d" % y.dtype.itemsize))


def check_reference_shaped_wrappers(case, device):
    """DenseCorrespondenceNetwork.find_best_matches and compute_match_statistics: the (u, v) <-> flat index conversion"""
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork as DCN
    r = reference(case)
    Q = case.q1
    h, w, _ = case.res.shape
    nd, gt, ia = r.nd[:Q], r.gt[:Q], case.ia[:Q]
    rows = np.arange(Q)
    res_a, res_b, mask = _t(case.res_a, device), _t(case.res, device), _t(case.mask, device)
    uv_a = np.stack([ia % w, ia // w], 1)
    uv_b = np.stack([gt % w, gt // w], 1)
    uv, dist, got_nd = DCN.find_best_matches(_t(uv_a, device), res_a, res_b, return_norm_diffs=True)
    assert np.array_equal(uv.cpu().numpy(), np.stack([r.best[:Q] % w, r.best[:Q] // w], 1))
    assert np.array_equal(bits(dist), bits(nd[rows, r.best[:Q]]))
    assert np.array_equal(bits(got_nd.cpu().numpy().reshape(Q, -1)), bits(nd))
    # this repository's numpy port of the reference's single-query find_best_match (the formula of this module's docstring,
    # not an independent oracle): the (u, v) convention of the two functions agrees
    for i in (0, Q - 1):
        ref_uv, ref_diff, ref_nd = DCN.find_best_match((int(uv_a[i, 0]), int(uv_a[i, 1])), case.res_a, case.res)
        assert (int(uv[i, 0]), int(uv[i, 1])) == (int(ref_uv[0]), int(ref_uv[1]))
        assert bits(dist[i:i + 1])[0] == bits(np.array([ref_diff], F32))[0]
        assert np.array_equal(bits(got_nd[i].cpu().numpy()), bits(ref_nd))
    s = stats_reference(nd, gt, case.mask, w)
    out = {k: v.cpu().numpy() for k, v in DCN.compute_match_statistics(_t(uv_a, device), _t(uv_b, device), res_a, res_b, mask).items()}
    for name, best, cnt, denom in (("", s.best, s.count, h * w), ("_masked", s.best_m, s.count_m, int((case.mask != 0).sum()))):
        pred = np.stack([best % w, best // w], 1)
        assert np.array_equal(out["uv_b_pred" + name], pred), name
        assert np.array_equal(out["num_pixels_closer_than_ground_truth" + name], cnt), name
        np.testing.assert_allclose(out["fraction_pixels_closer_than_ground_truth" + name], cnt / float(denom), rtol=2.0 ** -22)
        np.testing.assert_allclose(out["pixel_match_error_l2" + name], np.linalg.norm((uv_b - pred).astype(F64), axis=1),
                                   rtol=2.0 ** -22)
    assert np.array_equal(bits(out["norm_diff_pred"]), bits(nd[rows, s.best]))
    assert np.array_equal(bits(out["norm_diff_descriptor_ground_truth"]), bits(s.gt_dist))
    assert np.array_equal(out["pixel_match_error_l1"], np.abs(uv_b - np.stack([s.best % w, s.best // w], 1)).sum(1).astype(F32))


def check_equal_norm_across_kernels(case, device):
    """The chain of test_gpu_acrossobj.py on a near-tie: best_match_pairs and find_best_matches, pair by pair, give the same
    pixel and the same distance bits where two pixels share a norm and differ in the squared distance."""
    from dcn_hip import evaluate, match
    assert case.kind == "equalnorm"
    b = pair_batch(case)
    w = case.res.shape[1]
    res_b, queries = _t(b.res_b, device), _t(b.queries, device)
    m = evaluate.best_match_pairs(res_b, queries, _t(b.offsets, device))
    for p in (0, 2):
        lo, hi = int(b.offsets[p]), int(b.offsets[p + 1])
        idx, dist, _ = match.find_best_matches(res_b[p], queries[lo:hi])
        assert torch.equal(m.best_uv[1, lo:hi].long() * w + m.best_uv[0, lo:hi].long(), idx)
        assert torch.equal(m.norm_diff_descriptor_best_match[lo:hi].view(torch.int32), dist.view(torch.int32))
    x, y = case.pair_pixels
    assert (m.best_uv[1, :case.q2].long() * w + m.best_uv[0, :case.q2].long() == x).all()           # the earlier pixel
    hw = case.res.shape[0] * w
    assert (m.best_uv[1, case.q2:].long() * w + m.best_uv[0, case.q2:].long() == hw - 1 - y).all()  # reversed: the other one


# ------------------------------------------------------------------------------------------------ tier 2
TIER2 = [(d, n) for d in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64) for n in (713, 2072)]
TIER2_IDS = ["d%d_hw%d" % c for c in TIER2]
T2_Q1, T2_Q2 = 33, 65
_TIER2 = {}


def tier2_bound(d):
    """Twice the forward bound of a length-d fp32 sum of squares of rounded differences followed by one correctly rounded
    square root ((d + 2) * 2^-25 + 2^-24 relative): two candidates each carry it"""
    return 2.0 * ((d + 2) * 2.0 ** -25 + 2.0 ** -24)


def tier2_case(d, n):
    if (d, n) not in _TIER2:
        name = "random_d%d_hw%d" % (d, n)
        rng = _rng(name)
        h, w = SHAPES[n]
        res, res_a = rng.randn(h, w, d).astype(F32), rng.randn(h, w, d).astype(F32)
        ia = rng.randint(0, n, T2_Q2).astype(np.int64)
        gt = rng.randint(0, n, T2_Q2).astype(np.int64)
        mask = (rng.rand(h, w) < 0.4).astype(np.uint8)
        q = res_a.reshape(-1, d)[ia].astype(F64)
        d64 = np.zeros((T2_Q2, n), F64)
        for k in range(d):
            d64 += (res.reshape(-1, d)[None, :, k].astype(F64) - q[:, None, k]) ** 2
        d64 = np.sqrt(d64)
        d64.setflags(write=False)
        _TIER2[(d, n)] = (Case(name, "random", res, res_a, ia, mask, T2_Q1, T2_Q2, None), gt, d64)
    return _TIER2[(d, n)]


def _near_best(idx, d64, s, allowed=None):
    """The returned pixel of EVERY query is within s relative of the float64 minimum (over ``allowed`` pixels)"""
    rows = np.arange(d64.shape[0])
    cand = d64 if allowed is None else np.where(allowed[None, :], d64, np.inf)
    assert ((idx >= 0) & (idx < d64.shape[1])).all()
    if allowed is not None:
        assert allowed[idx].all()
    assert (d64[rows, idx] <= cand.min(1) * (1.0 + s)).all()


def _near(got, want, tol):
    assert (np.abs(got.astype(F64) - want) <= tol * want).all()


def _count_band(count, d64, g64, s, allowed=None):
    ok = np.ones(d64.shape[1], bool) if allowed is None else allowed
    want = ((d64 < g64[:, None]) & ok[None, :]).sum(1)
    band = ((np.abs(d64 - g64[:, None]) <= s * g64[:, None]) & ok[None, :]).sum(1)
    assert (np.abs(count - want) <= band).all()


def check_tier2_single_image(d, n, device):
    from dcn_hip import match
    case, gt, d64 = tier2_case(d, n)
    s = tier2_bound(d)
    Q = case.q1
    d64, gt = d64[:Q], gt[:Q]
    rows = np.arange(Q)
    on = case.mask.reshape(-1) != 0
    res, q = _t(case.res, device), _t(case.res_a.reshape(-1, d)[case.ia[:Q]], device)
    idx, dist, nd = match.find_best_matches(res, q, None, True)
    idx = idx.cpu().numpy()
    _near_best(idx, d64, s)
    _near(dist.cpu().numpy(), d64[rows, idx], s / 2)
    _near(nd.cpu().numpy().reshape(Q, -1), d64, s / 2)
    idx, dist, _ = match.find_best_matches(res, q, _t(case.mask, device))
    _near_best(idx.cpu().numpy(), d64, s, on)
    _near(dist.cpu().numpy(), d64[rows, idx.cpu().numpy()], s / 2)
    out = {k: v.cpu().numpy() for k, v in match.match_statistics(res, q, _t(gt, device), _t(case.mask, device)).items()}
    _near_best(out["best_idx"][0], d64, s)
    _near_best(out["best_idx"][1], d64, s, on)
    for half in (0, 1):
        _near(out["best_dist"][half], d64[rows, out["best_idx"][half]], s / 2)
    g64 = d64[rows, gt]
    _near(out["gt_dist"], g64, s / 2)
    _count_band(out["count"][0], d64, g64, s)
    _count_band(out["count"][1], d64, g64, s, on)


def check_tier2_pairs(d, n, device):
    from dcn_hip import evaluate
    case, gt, d64 = tier2_case(d, n)
    s = tier2_bound(d)
    w = case.res.shape[1]
    b = pair_batch(case, gt, d64)
    m = evaluate.best_match_pairs(_t(b.res_b, device), _t(b.queries, device), _t(b.offsets, device))
    t = _pair_statistics(case, device, b)[1]
    assert int(m.status.cpu()[0]) == 0 and int(t.status.cpu()[0]) == 0
    uv, pred = m.best_uv.cpu().numpy().astype(np.int64), t.pred_uv.cpu().numpy().astype(np.int64)
    norm, closer = m.norm_diff_descriptor_best_match.cpu().numpy(), t.closer.cpu().numpy()
    for _p, lo, dd, g, mask_b in b.rows:
        allowed = mask_b.reshape(-1) != 0
        k = dd.shape[0]
        rows, sl = np.arange(k), slice(lo, lo + k)
        idx = uv[1, sl] * w + uv[0, sl]
        _near_best(idx, dd, s)
        _near(norm[sl], dd[rows, idx], s / 2)
        i0, i1 = pred[1, sl] * w + pred[0, sl], pred[3, sl] * w + pred[2, sl]
        _near_best(i0, dd, s)
        _near_best(i1, dd, s, allowed)
        _near(t.column("norm_diff_descriptor").cpu().numpy()[sl], dd[rows, i0], s / 2)
        _near(t.column("norm_diff_descriptor_masked").cpu().numpy()[sl], dd[rows, i1], s / 2)
        g64 = dd[rows, g]
        _near(t.column("norm_diff_descriptor_ground_truth").cpu().numpy()[sl], g64, s / 2)
        _count_band(closer[0, sl], dd, g64, s)
        _count_band(closer[1, sl], dd, g64, s, allowed)
