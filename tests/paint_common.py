"""Checks of painting mesh vertices from their views (csrc/paint_kernels.hip, csrc/paint_rules.h, dcn_hip/paint.py), shared by
tests/test_emu_paint.py (host emulation) and tests/test_gpu_paint.py (MI355X).

``np_paint`` and ``np_finish`` are the yardsticks: the rules of include/dcn_hip.h section 18 in numpy float64 and integers,
written from the header's text.  Every float64 step is one numpy operation (one correctly rounded IEEE operation): count, sum,
sumsq, mean, variance and colours must EQUAL them.  The only tolerances in this file are the derived bound of the geometry test
and the 2 ulp of ``spread``, whose square root is torch's and not in the kernels' contract."""
import numpy as np
import pytest
import torch

import fusion_common as fc
import render_common as rc

VERTEX_COUNTS = (1, 255, 257, 1000)
IMAGES = ((37, 53), (1, 64), (48, 1))                  # (h, w)
FRAME_COUNTS = (1, 3, 65, 130)                         # both sides of the 64-frame chunk
CHANNELS = (1, 3, 16, 32)
MARGIN = 10.0
RULES = ("behind", "outside", "no depth", "margin", "mask", "row")


# ------------------------------------------------------------------------------------------------ the numpy statement
def empty_state(V, C):
    return np.zeros(V, np.int32), np.zeros((V, C), np.float64), np.zeros((V, C), np.float64)


def np_paint(state, vertices, valid, images, depth, mask, poses, K, pixel_offset=0.0, margin_mm=MARGIN, tally=None):
    """state = (count int32 [V], sum float64 [V, C], sumsq float64 [V, C]) is advanced in place by the frames in their order.
    ``tally``: a dict that counts, per rule, the (vertex, frame) pairs that reach it and those it rejects."""
    count, total, squares = state
    V, C = total.shape
    fx, fy, cx, cy = (np.float64(k) for k in K)
    o, margin = np.float64(pixel_offset), np.float64(margin_mm)
    depth = np.asarray(depth).view(np.uint16)
    F, h, w = depth.shape
    poses = np.asarray(poses, np.float32).reshape(F, 4, 4)
    wx, wy, wz = (np.asarray(vertices, np.float32)[:, k].astype(np.float64) for k in range(3))      # step 1: widened
    row_ok = np.arange(V) < (V if valid is None else int(valid))

    def rule(name, ok, passes):
        if tally is not None:
            reached, rejected = tally.setdefault(name, [0, 0])
            tally[name] = [reached + int(ok.sum()), rejected + int((ok & ~passes).sum())]
        return ok & passes
    for f in range(F):
        a = rc.np_camera(poses[f])                                                               # 16(a)
        with np.errstate(all="ignore"):
            x, y, z = (((a[r, 0] * wx + a[r, 1] * wy) + a[r, 2] * wz) + a[r, 3] for r in range(3))   # 16(b)
            ok = rule("behind", np.ones(V, bool), z > 0)                                         # step 2
            pu = np.floor(((fx * x) / z + cx) + o)                                               # step 3
            pv = np.floor(((fy * y) / z + cy) + o)
            ok = rule("outside", ok, (pu >= 0) & (pu < w) & (pv >= 0) & (pv < h))
            px, py = np.where(ok, pu, 0).astype(np.int64), np.where(ok, pv, 0).astype(np.int64)
            mm = depth[f][py, px].astype(np.int64)
            ok = rule("no depth", ok, mm != 0)                                                   # step 4
            e = z * np.float64(1000.0) - mm.astype(np.float64)                                   # step 5
            ok = rule("margin", ok, (e >= -margin) & (e <= margin))
            if mask is not None:
                ok = rule("mask", ok, np.asarray(mask)[f][py, px] != 0)                          # step 6
            ok = rule("row", ok, row_ok)
            values = np.asarray(images)[f][py, px].astype(np.float64).reshape(V, C)              # step 7
            count[ok] += 1
            for ch in range(C):
                total[ok, ch] = total[ok, ch] + values[ok, ch]
                squares[ok, ch] = squares[ok, ch] + values[ok, ch] * values[ok, ch]
    return state


def np_finish(state, min_views=1, lo=None, hi=None, channels=(0, 1, 2), unseen=(0, 0, 0)):
    """-> (mean float32 [V, C], variance float32 [V], colours uint8 [V, 3]); lo, hi float64 [C]"""
    count, total, squares = state
    V, C = total.shape
    painted = count >= min_views
    with np.errstate(all="ignore"):
        n = count.astype(np.float64)[:, None]
        m = total / n
        var = squares / n - m * m
        var = np.where(var < 0, np.float64(0.0), var)
        summed = np.zeros(V, np.float64)
        for ch in range(C):
            summed = summed + var[:, ch]
        mean = np.where(painted[:, None], m, 0.0).astype(np.float32)
        variance = np.where(painted, summed, np.nan).astype(np.float32)
        colours = np.zeros((V, 3), np.uint8)
        for k, ch in enumerate(channels):
            t = (m[:, ch] - np.float64(lo[ch])) / (np.float64(hi[ch]) - np.float64(lo[ch]))
            bad = np.isnan(t) | (np.float64(hi[ch]) == np.float64(lo[ch]))
            t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
            byte = np.rint(np.where(bad, 0.0, t) * np.float64(255.0))
            colours[:, k] = np.where(painted, byte, unseen[k]).astype(np.uint8)
    return mean, variance, colours


# ------------------------------------------------------------------------------------------------ running
def mesh_on(device, vertices, valid=None):
    """A vertex cloud as a render.Mesh without triangles; with ``valid`` it carries counts as fusion's untrimmed meshes do"""
    from dcn_hip import render
    m = render.Mesh(np.asarray(vertices, np.float32), np.zeros((0, 3), np.int32), device=device)
    if valid is not None:
        m.counts = torch.tensor([int(valid), 0], dtype=torch.int32).to(device)
    return m


def to_device(a, device):
    a = np.ascontiguousarray(a)
    return fc.as_depth(a, device) if a.dtype == np.uint16 else torch.from_numpy(a).to(device)


def state_of(paint):
    return paint.count.cpu().numpy(), paint.sum.cpu().numpy(), paint.sumsq.cpu().numpy()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() == want.tobytes():
        return
    flat_g, flat_w = got.reshape(-1), want.reshape(-1)
    word = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero(flat_g.view(word) != flat_w.view(word))
    both_nan = got.dtype.kind == "f" and np.all(np.isnan(flat_g[bad]) & np.isnan(flat_w[bad]))
    assert both_nan, "%s differs at %d places, first %d: %r, statement %r" % (what, len(bad), bad[0], flat_g[bad[0]],
                                                                             flat_w[bad[0]])


def check_state(paint, want, what):
    for name, g, w in zip(("count", "sum", "sumsq"), state_of(paint), want):
        same_bits(g, w, "%s: %s" % (what, name))


def check_finish(paint, want_state, what, **kw):
    """finish() against np_finish with the same lo / hi (the device's defaults are checked against numpy's own range first)"""
    out = paint.finish(**kw)
    C = want_state[1].shape[1]
    min_views = kw.get("min_views", 1)
    ch = tuple(min(k, C - 1) for k in kw.get("channels", (0, 1, 2)))
    if paint.dtype == torch.uint8:
        lo, hi = kw.get("lo", np.zeros(C)), kw.get("hi", np.full(C, 255.0))
    else:
        m0 = np_finish(want_state, min_views, np.zeros(C), np.ones(C), ch)[0].astype(np.float64)
        painted = want_state[0] >= min_views
        with np.errstate(all="ignore"):                              # (no painted vertex: inf and -inf, every byte 0)
            lo = kw["lo"] if "lo" in kw else np.where(painted[:, None], m0, np.inf).min(axis=0, initial=np.inf)
            hi = kw["hi"] if "hi" in kw else np.where(painted[:, None], m0, -np.inf).max(axis=0, initial=-np.inf)
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (C,)), np.broadcast_to(np.asarray(hi, np.float64), (C,))
    mean, variance, colours = np_finish(want_state, min_views, lo, hi, ch, kw.get("unseen", (0, 0, 0)))
    same_bits(out.mean.cpu().numpy(), mean, what + ": mean")
    same_bits(out.variance.cpu().numpy(), variance, what + ": variance")
    same_bits(out.colours.cpu().numpy(), colours, what + ": colours")
    same_bits(out.count.cpu().numpy(), want_state[0], what + ": count")
    check_spread(out.spread.cpu().numpy(), variance, what)
    return out


def check_spread(spread, variance, what):
    """torch's square root against numpy's float32 one: within 2 ulp, NaN where NaN"""
    with np.errstate(all="ignore"):
        want = np.sqrt(variance.astype(np.float32))
    assert np.array_equal(np.isnan(spread), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.all(np.abs(spread[ok].astype(np.float64) - want[ok]) <= 2 * np.spacing(want[ok]).astype(np.float64)), what


# ------------------------------------------------------------------------------------------------ 1. equal to the statement
def camera_for(h, w):
    """Both focal lengths follow their own axis, so that a one-row and a one-column image still hold half the projections"""
    return (1.5 * w, 1.5 * h, w / 2.0, h / 2.0)


def random_scene(V, hw, F, C, dtype, seed):
    """A vertex cloud from behind the cameras to 1.2 m, poses around it (fusion_common.poses_around: one camera sits inside
    the cloud) and depth images made FROM the projections: a pixel that a vertex projects to holds that vertex's millimetres
    moved by up to 1.5 margins either way, so that about half of the pairs pass rule 5; zeros and far values are sprinkled in;
    mask bytes of 0, 1 and 255."""
    h, w = hw
    rng = np.random.RandomState(seed)
    vertices = np.stack([rng.uniform(-0.45, 0.45, V), rng.uniform(-0.45, 0.45, V), rng.uniform(-0.15, 1.2, V)], 1).astype(np.float32)
    poses = fc.poses_around(F, seed)
    K = camera_for(h, w)
    depth = rng.randint(600, 1300, (F, h, w)).astype(np.uint16)
    wx, wy, wz = (vertices[:, k].astype(np.float64) for k in range(3))
    for f in range(F):
        a = rc.np_camera(poses[f])
        with np.errstate(all="ignore"):
            x, y, z = (((a[r, 0] * wx + a[r, 1] * wy) + a[r, 2] * wz) + a[r, 3] for r in range(3))
            pu, pv = np.floor((K[0] * x) / z + K[2]), np.floor((K[1] * y) / z + K[3])
            ok = (z > 0) & (pu >= 0) & (pu < w) & (pv >= 0) & (pv < h) & (rng.rand(V) < 0.8)
        mm = np.clip(np.trunc(z[ok] * 1000.0) + rng.randint(-15, 16, int(ok.sum())), 1, 65535)
        depth[f][pv[ok].astype(np.int64), pu[ok].astype(np.int64)] = mm.astype(np.uint16)
    depth[rng.rand(F, h, w) < 0.1] = 0
    mask = rng.choice(np.array([0, 0, 1, 1, 255], np.uint8), (F, h, w))
    if dtype == np.uint8:
        images = rng.randint(0, 256, (F, h, w, C)).astype(np.uint8)
    else:
        images = (rng.normal(0, 1, (F, h, w, C)) * rng.choice([1e-3, 1.0, 1e3], (1, 1, 1, C))).astype(np.float32)
    return vertices, poses, K, depth, mask, images


def check_paint_random(V, hw, F, C, dtype, device, seed=0):
    """With and without mask, with and without valid_vertices; the default chunk, 1 and 7 frames per launch, and the same
    frames split over three calls: all equal the statement, for both pixel offsets.  Where there
    are enough pairs (V * F >= 255) every rule is asserted to pass some and reject some."""
    from dcn_hip import paint as pt
    h, w = hw
    vertices, poses, K, depth, mask, images = random_scene(V, hw, F, C, dtype, seed + V + 7 * F + C)
    tdtype = torch.uint8 if dtype == np.uint8 else torch.float32
    dev = dict(images=to_device(images, device), depth=to_device(depth, device), mask=to_device(mask, device))
    tally = {}
    for use_mask, valid, o in ((True, None, 0.0), (False, max(V - 3, 0), 0.5), (True, V // 2, 0.0), (False, None, 0.5)):
        m = mask if use_mask else None
        want = np_paint(empty_state(V, C), vertices, valid, images, depth, m, poses, K, o, tally=tally)
        mesh = mesh_on(device, vertices, valid)
        what = "V=%d %s F=%d C=%d %s mask=%s valid=%s o=%s" % (V, hw, F, C, dtype.__name__, use_mask, valid, o)
        runs = [dict(), dict(frames_per_launch=1), dict(frames_per_launch=7)]
        last = None
        for kw in runs if use_mask == (valid is None) else runs[:1]:
            last = pt.MeshPaint(mesh, C, tdtype)
            last.add(dev["images"], dev["depth"], poses, K, mask=dev["mask"] if use_mask else None, pixel_offset=o, **kw)
            check_state(last, want, "%s %s" % (what, kw))
        check_finish(last, want, what)
        check_finish(last, want, what + " min_views=2", min_views=2, unseen=(9, 8, 7), channels=(C - 1, 0, C // 2))
        if F >= 3:
            cuts = (0, F // 3, F // 3 + 1, F)
            split = pt.MeshPaint(mesh, C, tdtype)
            for a, b in zip(cuts[:-1], cuts[1:]):
                split.add(dev["images"][a:b], dev["depth"][a:b], torch.from_numpy(poses[a:b]).to(device), K,
                          mask=dev["mask"][a:b] if use_mask else None, pixel_offset=o, frames_per_launch=7 if a else None)
            check_state(split, want, what + " three calls")
    if V * F >= 255:
        for name in RULES:
            reached, rejected = tally[name]
            assert 0 < rejected < reached, (name, reached, rejected)


def random_cases():
    """Every vertex count with every frame count; the image shapes, channel counts and view types cycle through them so that
    each value of each meets each value of V and of F at least once over the 32 cases"""
    out = []
    for i, V in enumerate(VERTEX_COUNTS):
        for j, F in enumerate(FRAME_COUNTS):
            for k, dtype in enumerate((np.uint8, np.float32)):
                out.append((V, IMAGES[(i + j + k) % 3], F, CHANNELS[(i + j + 2 * k) % 4], dtype))
    return out


RANDOM_CASES = random_cases()
RANDOM_IDS = ["V%d-%dx%d-F%d-C%d-%s" % (V, hw[0], hw[1], F, C, d.__name__) for V, hw, F, C, d in RANDOM_CASES]


# ------------------------------------------------------------------------------------------------ 2. exact cases
EDGE_K = (4.0, 4.0, 8.0, 6.0)           # u = 4 x / z + 8 on 16 columns, v = 4 y / z + 6 on 12 rows: exact at the ratios below
EDGE_DEPTHS = (990, 1010, 1000, 999, 1001, 0, 1000, 1000, 1000)      # one constant image per frame; frame 6 has a mask of 0,
EDGE_VERTICES = (                                                   # frame 7 a NaN pose, frame 8 a pose of 1e30
    (0.0, 0.0, 1.0),          # 0: u = 8, v = 6
    (0.25, 0.0, 1.0),         # 1: u = 9 exactly, a pixel boundary: column 9 with both offsets
    (0.125, 0.0, 1.0),        # 2: u = 8.5: column 8 with o = 0, column 9 with o = 0.5
    (2.0, 0.0, 1.0),          # 3: u = 16: one past the last column
    (1.875, 0.0, 1.0),        # 4: u = 15.5: the last column with o = 0, outside with o = 0.5
    (-2.125, 0.0, 1.0),       # 5: u = -0.5: outside with o = 0, column 0 with o = 0.5
    (0.0, 1.5, 1.0),          # 6: v = 12: one past the last row
    (0.0, -1.5, 1.0),         # 7: v = 0
    (0.0, 0.0, 0.0),          # 8: z == 0
    (0.0, 0.0, -1.0),         # 9: z < 0
    (np.nan, 0.0, 1.0),       # 10: NaN
    (0.0, 0.0, 1.0),          # 11: the row at valid_vertices
    (0.0, 0.0, 1.0),          # 12: beyond it
)
EDGE_VALID = 11


def edge_inputs():
    F = len(EDGE_DEPTHS)
    depth = np.stack([np.full((12, 16), d, np.uint16) for d in EDGE_DEPTHS])
    mask = np.ones((F, 12, 16), np.uint8)
    mask[6] = 0
    poses = np.stack([np.eye(4, dtype=np.float32)] * F)
    poses[7, 1, 2] = np.nan
    poses[8, :3, :] = 1e30
    images = np.zeros((F, 12, 16, 2), np.float32)
    images[..., 0] = np.arange(16, dtype=np.float32)[None, None, :]                  # channel 0: the column
    images[..., 1] = (np.arange(F, dtype=np.float32) + 1)[:, None, None]             # channel 1: the frame, from 1
    return np.asarray(EDGE_VERTICES, np.float32), depth, mask, poses, images


def check_paint_edges(device):
    """Power-of-two geometry under the identity pose and constant depth images around 1 m: every equality of rules 2-6 is exact
    in float64.  The statement is asserted to take the branch each case is there for; the library must equal the statement."""
    from dcn_hip import paint as pt
    vertices, depth, mask, poses, images = edge_inputs()
    below = float(np.nextafter(10.0, 0.0))

    def frames_of(case, row):
        """the frames that, alone, paint the row under (pixel offset, margin) by the statement"""
        alone = lambda f: np_paint(empty_state(13, 2), vertices, EDGE_VALID, images[f:f + 1], depth[f:f + 1], mask[f:f + 1],
                                   poses[f:f + 1], EDGE_K, case[0], case[1])[0][row]
        return [f for f in range(len(EDGE_DEPTHS)) if alone(f)]
    for o, margin in ((0.0, 10.0), (0.5, 10.0), (0.0, below), (0.0, 0.0), (0.5, 0.0)):
        want = np_paint(empty_state(13, 2), vertices, EDGE_VALID, images, depth, mask, poses, EDGE_K, o, margin)
        count, total, _ = want
        column = lambda row: total[row, 0] / count[row]
        if margin == 10.0:
            assert frames_of((o, margin), 0) == [0, 1, 2, 3, 4]          # e = +-10 kept; depth 0, mask 0, NaN and huge poses not
            assert column(1) == 9 and column(2) == (8 if o == 0.0 else 9)
            assert count[3] == 0 and count[6] == 0 and count[7] == 5
            assert (count[4], count[5]) == ((5, 0) if o == 0.0 else (0, 5))
            assert count[8] == 0 and count[9] == 0 and count[10] == 0
            assert count[11] == 0 and count[12] == 0 and count[0] == 5
        if margin == below:
            assert frames_of((o, margin), 0) == [2, 3, 4]                # e = +-10 is one step outside
        if margin == 0.0:
            assert frames_of((o, margin), 0) == [2]                      # only e == 0
        for kw in (dict(), dict(frames_per_launch=2)):
            p = pt.MeshPaint(mesh_on(device, vertices, EDGE_VALID), 2, torch.float32)
            p.add(to_device(images, device), to_device(depth, device), poses, EDGE_K, mask=to_device(mask, device),
                  pixel_offset=o, margin_mm=margin, **kw)
            check_state(p, want, "edges o=%s margin=%r %s" % (o, margin, kw))
        check_finish(p, want, "edges o=%s margin=%r" % (o, margin), unseen=(1, 2, 3))
        check_finish(p, want, "edges min_views above count", min_views=6, unseen=(255, 0, 7))
        check_finish(p, want, "edges hi == lo", lo=[0.0, 3.0], hi=[0.0, 3.0])
        check_finish(p, want, "edges given range", lo=[8.0, 0.0], hi=[10.0, 6.0], channels=(0, 1, 0))
    # without valid_vertices rows 11 and 12 are painted like row 0
    want = np_paint(empty_state(13, 2), vertices, None, images, depth, None, poses, EDGE_K)
    assert want[0][11] == want[0][12] == want[0][0] == 6
    p = pt.MeshPaint(mesh_on(device, vertices), 2, torch.float32)
    p.add(to_device(images, device), to_device(depth, device), poses, EDGE_K)
    check_state(p, want, "edges without mask and valid")
    # a NaN descriptor propagates: sum, mean and variance NaN, the colour byte 0
    bad = images.copy()
    bad[2, 6, 8, 0] = np.nan
    want = np_paint(empty_state(13, 2), vertices, EDGE_VALID, bad, depth, mask, poses, EDGE_K)
    assert np.isnan(want[1][0, 0]) and not np.isnan(want[1][0, 1]) and not np.isnan(want[1][1]).any()
    p = pt.MeshPaint(mesh_on(device, vertices, EDGE_VALID), 2, torch.float32)
    p.add(to_device(bad, device), to_device(depth, device), poses, EDGE_K, mask=to_device(mask, device))
    check_state(p, want, "NaN descriptor")
    out = check_finish(p, want, "NaN descriptor", lo=[0.0, 0.0], hi=[16.0, 16.0])
    assert np.isnan(out.mean.cpu().numpy()[0, 0]) and np.isnan(out.variance.cpu().numpy()[0])
    assert out.colours.cpu().numpy()[0, 0] == 0 and out.colours.cpu().numpy()[0, 1] > 0


# ------------------------------------------------------------------------------------------------ 3. geometry
def box_cloud():
    """Points on the six faces of render_common's box and on the table around and under it"""
    g = np.linspace(0.0, 1.0, 9)
    lo, hi = np.array([-0.025, -0.025, 0.875]), np.array([0.275, 0.275, 1.25])
    pts, kind = [], []
    for axis in range(3):
        for side, name in ((lo, "near"), (hi, "far")):
            for s in g:
                for t in g:
                    p = lo + (hi - lo) * np.array([s, t, 0.0])[[2, 0, 1] if axis == 0 else ([0, 2, 1] if axis == 1 else [0, 1, 2])]
                    p[axis] = side[axis]
                    pts.append(p)
                    rim = s in (0.0, 1.0) or t in (0.0, 1.0)          # (a silhouette: its pixel's centre may lie beside the box)
                    kind.append((("rim" if rim else "top") if name == "near" else "bottom") if axis == 2 else "side")
    for x in np.linspace(-0.3, 0.55, 18):
        for y in np.linspace(-0.3, 0.55, 18):
            pts.append([x, y, 1.25])
            under = lo[0] < x < hi[0] and lo[1] < y < hi[1]
            kind.append("under" if under else "table")
    return np.asarray(pts, np.float32), np.asarray(kind)


def check_geometry(device):
    """The box scene's rendered depth images, painted with float images whose three channels are the world coordinates
    back-projected from that depth at the pixel centres (numpy float64 on the host): a painted vertex's mean is within
    ``bound`` of its own position, and so is its spread.  The bound, from its parts, per vertex and view, in metres:

        lateral   a vertex and the centre of the pixel that holds it differ by at most half a pixel on each image axis: at the
                  vertex's depth z that is 0.5 * z / fx and 0.5 * z / fy
        along     rule 5 keeps |z * 1000 - mm| <= margin_mm, and mm is the surface's depth truncated to a millimetre (16(g)),
                  read back as mm / 1000: the back-projected point lies within (margin_mm + 1) / 1000 of the vertex's depth
                  along the pixel's ray, whose direction (x / z, y / z, 1) is at most ``ray`` long over the image
        rounding  the images are float32: 2^-24 relative per coordinate, below 2^-22 m for coordinates under 4 m

        bound = sqrt((0.5 z / fx)^2 + (0.5 z / fy)^2) + ray * (margin_mm + 1) / 1000 + 3 * 2^-22

    with z the largest depth of the vertex over the views.  The mean of points within ``bound`` of p is within ``bound`` of p,
    and the variance about the mean is at most the mean squared distance from p, so ``spread`` <= bound too."""
    from dcn_hip import paint as pt
    scene = rc.box_scene_on(device)
    im, K, _, _ = rc.render_box_scene(scene)
    h, w = 48, 64
    fx, fy, cx, cy = K
    poses = rc.scene_poses()
    depth = im.depth.cpu().numpy().view(np.uint16)
    d = depth.astype(np.float64) / 1000.0
    uc, vc = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    images = np.zeros((len(poses), h, w, 3), np.float32)
    for f, pose in enumerate(poses):
        cam = np.stack([(uc - cx) / fx * d[f], (vc - cy) / fy * d[f], d[f]], axis=2)
        images[f] = (cam.dot(pose[:3, :3].T) + pose[:3, 3]).astype(np.float32)
    vertices, kind = box_cloud()
    zs = np.stack([rc.np_camera(p)[2, :3].dot(vertices.T.astype(np.float64)) + rc.np_camera(p)[2, 3] for p in poses]).max(axis=0)
    ray = np.sqrt(1.0 + (max(cx, w - cx) / fx) ** 2 + (max(cy, h - cy) / fy) ** 2)
    bound = np.sqrt((0.5 * zs / fx) ** 2 + (0.5 * zs / fy) ** 2) + ray * (MARGIN + 1.0) / 1000.0 + 3 * 2.0 ** -22
    mesh = mesh_on(device, vertices)
    p = pt.MeshPaint(mesh, 3, torch.float32)
    p.add(to_device(images, device), im.depth, torch.from_numpy(poses).to(device), K)
    want = np_paint(empty_state(len(vertices), 3), vertices, None, images, depth, None, poses, K)
    check_state(p, want, "geometry")
    out = p.finish()
    count, mean, spread = out.count.cpu().numpy(), out.mean.cpu().numpy().astype(np.float64), out.spread.cpu().numpy()
    seen = count > 0
    assert seen.sum() > 300 and (count == len(poses)).sum() > 100
    error = np.linalg.norm(mean - vertices.astype(np.float64), axis=1)
    assert np.all(error[seen] <= bound[seen]), (error[seen].max(), bound[seen].min())
    assert np.all(spread[seen] <= bound[seen]), (spread[seen].max(), bound[seen].min())
    # one frontal view: the far faces of the box and the table under it are hidden, the top and the open table are seen
    front = pt.MeshPaint(mesh, 3, torch.float32)
    front.add(to_device(images[:1], device), im.depth[:1], poses[:1], K)
    c1 = front.count.cpu().numpy()
    interior = lambda name: kind == name
    assert not c1[interior("bottom")].any() and not c1[interior("under")].any()
    inside_image = lambda v: ((fx * v[:, 0] / v[:, 2] + cx >= 0) & (fx * v[:, 0] / v[:, 2] + cx < w)
                              & (fy * v[:, 1] / v[:, 2] + cy >= 0) & (fy * v[:, 1] / v[:, 2] + cy < h))
    top = interior("top") & inside_image(vertices)
    assert top.sum() > 20 and c1[top].all()
    assert c1[interior("table") & inside_image(vertices)].sum() > 20


# ------------------------------------------------------------------------------------------------ 4. constant views
def check_constant_views(device):
    """uint8 images of one colour per channel: that colour exactly, variance exactly 0, colours the input bytes"""
    from dcn_hip import paint as pt
    V, (h, w), F = 257, IMAGES[0], 5
    vertices, poses, K, depth, mask, _ = random_scene(V, (h, w), F, 3, np.uint8, 11)
    colour = np.array([255, 77, 2], np.uint8)
    images = np.broadcast_to(colour, (F, h, w, 3)).copy()
    out = pt.paint_colours(mesh_on(device, vertices), to_device(images, device), to_device(depth, device), poses, K,
                           pixel_offset=0.0, unseen=(1, 1, 1))
    count = out.count.cpu().numpy()
    seen = count > 0
    assert seen.sum() > 20 and (count > 1).sum() > 5 and (~seen).sum() > 5
    assert np.array_equal(out.mean.cpu().numpy()[seen], np.broadcast_to(colour.astype(np.float32), (int(seen.sum()), 3)))
    assert np.all(out.variance.cpu().numpy()[seen] == 0.0) and np.all(out.spread.cpu().numpy()[seen] == 0.0)
    assert np.array_equal(out.colours.cpu().numpy()[seen], np.broadcast_to(colour, (int(seen.sum()), 3)))
    assert np.all(out.colours.cpu().numpy()[~seen] == 1) and np.all(np.isnan(out.variance.cpu().numpy()[~seen]))
    want = np_paint(empty_state(V, 3), vertices, None, images, depth, None, poses, K)
    same_bits(count, want[0], "constant views: count")


# ------------------------------------------------------------------------------------------------ 5. repeatable
def check_repeatable(device):
    from dcn_hip import paint as pt
    V, hw, F, C = 1000, IMAGES[0], 65, 16
    vertices, poses, K, depth, mask, images = random_scene(V, hw, F, C, np.float32, 5)
    runs = []
    for _ in range(2):
        p = pt.MeshPaint(mesh_on(device, vertices), C, torch.float32)
        p.add(to_device(images, device), to_device(depth, device), poses, K, mask=to_device(mask, device))
        out = p.finish()
        runs.append([a.tobytes() for a in state_of(p)] + [t.cpu().numpy().tobytes() for t in out])
    assert runs[0] == runs[1]
    want = np_paint(empty_state(V, C), vertices, None, images, depth, mask, poses, K)
    check_finish(p, want, "repeatable")


# ------------------------------------------------------------------------------------------------ 6., 7. the chains
class PointwiseNetwork(torch.nn.Module):
    """A ``dcn`` whose D = 3 descriptors are a fixed pointwise function of the normalized image: batched and per-image calls
    agree bit for bit.  ``outputs``: what it returned, per call."""

    def __init__(self, keep=True):
        super().__init__()
        self.keep, self.outputs = keep, []

    def forward_image_tensors(self, x):
        assert not self.training
        y = x.permute(0, 2, 3, 1).contiguous()
        out = torch.stack([y[..., 0] + 0.5 * y[..., 1], y[..., 1] * y[..., 2], y[..., 2] - 0.25 * y[..., 0]], dim=3).contiguous()
        if self.keep:
            self.outputs.append(out)
        return out

    @property
    def descriptor_image_stats(self):
        raise IOError("no descriptor statistics file")


def box_scene_images(device):
    """-> (scene of render_common.box_scene_on, its SceneImages, K): the uploads, which happen once"""
    scene = rc.box_scene_on(device)
    im, K, _, _ = rc.render_box_scene(scene)
    return scene, im, K


def fused_box_scene(scene, im, K):
    """-> (fused full mesh, padded; SceneImages of the fused meshes; K; poses on the device): depth images -> fuse_scene ->
    render_scene, nothing read back"""
    fused = fc.fuse_box_scene(im, K, scene[2])
    return fused[0], fc.rerender(fused, K, scene[2]), K, scene[2]


def paint_fused_scene(full, again, K, poses, rgb):
    from dcn_hip import paint as pt
    p = pt.MeshPaint(full, 3, torch.uint8)
    p.add(rgb, again.depth, poses, K)
    return p, p.finish()


def check_fused_paint(p, out, full, again, K, rgb):
    """The padded mesh's paint against the statement on the trimmed arrays: rows beyond counts[0] stay empty"""
    nv = int(full.counts[0])
    V = int(full.vertices.shape[0])
    assert 0 < nv < V
    vertices = full.vertices.cpu().numpy()
    want = np_paint(empty_state(V, 3), vertices, nv, rgb.cpu().numpy(), again.depth.cpu().numpy().view(np.uint16), None,
                    rc.scene_poses(), K)
    check_state(p, want, "fused scene")
    assert want[0][:nv].max() == 4 and not want[0][nv:].any() and (want[0][:nv] > 0).sum() > nv // 4
    check_finish(p, want, "fused scene")


def check_descriptor_chain(device):
    """paint_descriptors, batched, equals ONE MeshPaint.add over all frames' descriptor images bit for bit, with and without
    the store's mask and for a subset of the frames; the summary equals the numpy reduction of the statement"""
    from dcn_hip import paint as pt
    full, again, K, poses = fused_box_scene(*box_scene_images(device))
    store = rc.store_of(again, K, device)
    for kw, rows in ((dict(batch=3), None), (dict(batch=1, mask=False, min_views=2), None), (dict(batch=16, frames=[3, 1]), [3, 1])):
        net = PointwiseNetwork()
        out, summary = pt.paint_descriptors(net, store, full, 0, **kw)
        assert net.training and len(net.outputs) == {3: 2, 1: 4, 16: 1}[kw["batch"]]
        res = torch.cat(net.outputs)
        pick = (lambda t: t) if rows is None else (lambda t: t[torch.as_tensor(rows).to(t.device)])
        one = pt.MeshPaint(full, 3, torch.float32)
        one.add(res, pick(store.depth), pick(store.poses.view(-1, 4, 4)), K, mask=pick(store.mask) if kw.get("mask", True) else None)
        min_views = kw.get("min_views", 1)
        direct = one.finish(min_views=min_views)
        for name, a, b in zip(out._fields, out, direct):
            same_bits(a.cpu().numpy(), b.cpu().numpy(), "paint_descriptors %s: %s" % (kw, name))
        nv, V = int(full.counts[0]), int(full.vertices.shape[0])
        sel = (lambda a: a) if rows is None else (lambda a: a[rows])
        want = np_paint(empty_state(V, 3), full.vertices.cpu().numpy(), nv, res.cpu().numpy(),
                        sel(store.depth.cpu().numpy().view(np.uint16)), sel(store.mask.cpu().numpy()) if kw.get("mask", True) else None,
                        sel(rc.scene_poses()), K)
        check_state(one, want, "paint_descriptors %s" % (kw,))
        check_finish(one, want, "paint_descriptors %s" % (kw,), min_views=min_views)
        painted = want[0] >= min_views
        assert painted.sum() > 10
        with np.errstate(all="ignore"):
            spread = np.sqrt(np_finish(want, min_views, np.zeros(3), np.ones(3))[1]).astype(np.float64)
        got = summary.cpu().numpy()
        assert summary.dtype == torch.float64 and got[0] == painted.sum()
        assert abs(got[1] - spread[painted].mean()) <= 4 * np.spacing(np.float32(spread[painted].max())) and \
            abs(got[2] - spread[painted].max()) <= 2 * np.spacing(np.float32(spread[painted].max()))
    # spread as a one-curve table goes through the evaluation's curve kernel as it is, the unseen vertices dropped as NaN
    curves = pt.spread_curve(out)
    count = curves.summary.cpu().numpy()
    assert curves.fields == ("spread",) and int(curves.status.cpu().numpy().max()) == 0
    assert int(curves.cumcount.cpu().numpy()[0, -1]) == int((want[0] >= 1).sum()) and count.shape == (1, 8)


# ------------------------------------------------------------------------------------------------ 8. PLY
def check_coloured_ply(device, tmp_path):
    from dcn_hip import paint as pt
    from dcn_hip import render
    rng = np.random.RandomState(2)
    verts, tris = fc.random_mesh(4, 50, 70)
    verts = verts.astype(np.float32)
    padded = np.concatenate([tris, -np.ones((5, 3), tris.dtype)]).astype(np.int32)
    colours = rng.randint(0, 256, (len(verts), 3)).astype(np.uint8)
    path = str(tmp_path / "coloured.ply")
    assert pt.write_coloured_ply(path, verts, padded, colours) == path
    v, t = render.read_ply(path)
    assert v.tobytes() == verts.tobytes() and np.array_equal(t, tris.astype(np.int32))
    assert np.array_equal(pt.read_ply_colours(path), colours)
    m = render.Mesh.from_ply(path, device=device)
    assert m.num_vertices == len(verts) and m.num_triangles == len(tris)
    plain = str(tmp_path / "plain.ply")
    render.write_ply(plain, verts, tris)
    with pytest.raises(render.PlyError, match="red"):
        pt.read_ply_colours(plain)
    with pytest.raises(ValueError, match="colours"):
        pt.write_coloured_ply(path, verts, tris, colours[:-1])
    with pytest.raises(ValueError, match="colours"):
        pt.write_coloured_ply(path, verts, tris, colours.astype(np.float32))
    empty = str(tmp_path / "empty.ply")
    pt.write_coloured_ply(empty, np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8))
    assert pt.read_ply_colours(empty).shape == (0, 3) and render.read_ply(empty)[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 9. argument errors
def check_argument_errors(device):
    """Each raises ValueError before any launch: the state stays zero"""
    from dcn_hip import paint as pt
    other = "cpu" if device != "cpu" else "meta"
    V, (h, w), F, C = 5, (6, 8), 2, 3
    vertices, poses, K, depth, mask, images = random_scene(V, (h, w), F, C, np.float32, 1)
    mesh = mesh_on(device, vertices)
    im, d, m = to_device(images, device), to_device(depth, device), to_device(mask, device)
    for c in (0, 33, -1):
        with pytest.raises(ValueError, match="channels"):
            pt.MeshPaint(mesh, c, torch.float32)
    with pytest.raises(ValueError, match="uint8 or"):
        pt.MeshPaint(mesh, 3, torch.float64)
    p = pt.MeshPaint(mesh, C, torch.float32)
    bad = [
        (dict(images=im[..., :2]), "images must be"),                       # mismatched channel count
        (dict(images=im.to(torch.float64)), "images must be a"),            # wrong dtypes
        (dict(images=(im * 0).to(torch.uint8)), "images must be a"),
        (dict(depth=d.to(torch.int32)), "16-bit"),
        (dict(depth=d.to(torch.float32)), "16-bit"),
        (dict(mask=m.to(torch.int16)), "mask must be a uint8"),
        (dict(depth=d[:, :-1]), "depth must be"),                           # mismatched shapes
        (dict(depth=d[:1]), "depth must be"),
        (dict(mask=m[:, :, :-1]), "mask must be"),
        (dict(poses=poses[:1]), "poses for"),
        (dict(poses=poses[:, :3]), "poses must be"),
        (dict(margin_mm=-1.0), "margin_mm"),
        (dict(margin_mm=float("nan")), "margin_mm"),
        (dict(frames_per_launch=0), "frames_per_launch"),
        (dict(frames_per_launch=65), "frames_per_launch"),
        (dict(K=(1.0, 2.0, 3.0)), "K must be"),
        (dict(images=im.to(other)), "are on"),                              # the wrong device
        (dict(depth=d.to(other)), "are on"),
        (dict(mask=m.to(other)), "are on"),
        (dict(poses=torch.from_numpy(poses).to(other)), "are on"),
    ]
    for change, match in bad:
        args = dict(images=im, depth=d, poses=poses, K=K, mask=m)
        args.update(change)
        with pytest.raises(ValueError, match=match):
            p.add(**args)
    for kw, match in ((dict(min_views=0), "min_views"), (dict(channels=(0, 1, 3)), "channels"), (dict(channels=(0, 1)), "channels"),
                      (dict(unseen=(0, 0, 256)), "unseen"), (dict(lo=[0.0, 1.0]), "lo must"),
                      (dict(hi=torch.zeros(3, device=other)), "hi is on")):
        with pytest.raises(ValueError, match=match):
            p.finish(**kw)
    assert not p.count.cpu().numpy().any() and not p.sum.cpu().numpy().any()
    p8 = pt.MeshPaint(mesh, C, torch.uint8)
    with pytest.raises(ValueError, match="images must be a"):
        p8.add(im, d, poses, K)
