"""Checks of the depth renderer (csrc/render_kernels.hip, csrc/render_raster.h, dcn_hip/render.py), shared by
tests/test_emu_render.py (host emulation) and tests/test_gpu_render.py (MI355X).

``np_render`` is the yardstick: rules (a)-(h) of include/dcn_hip.h section 16 in numpy float64 / int64, a plain loop over the
frames and the triangles, written from the header's text.  Every float64 step is one numpy operation (one correctly rounded
IEEE operation), every other step is integer: the device's depth images, status counts and masks must EQUAL it -- there is
no tolerance anywhere in this file.  The mask rules are pinned to the reference's own lines by
tests/golden/render_ref_masks_*.npz (tests/golden/make_render_goldens_from_reference.py); the rasteriser has no reference
text to pin to."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASK_GOLDENS = ("render_ref_masks_37x53", "render_ref_masks_48x64")
SHAPES = ((48, 64), (37, 53), (1, 64), (48, 1))
FRAME_COUNTS = (1, 3)
ALL_LARGE, ALL_SMALL = 0, 2 ** 31 - 1          # large_threshold values that force every triangle down one path
Z_NEAR = 0.05
GUARD = 2 ** 30
EMPTY = 2 ** 32 - 1


# ------------------------------------------------------------------------------------------------ the numpy statement
def np_camera(pose):
    """(a): rows (R^T | -R^T t) of the float32 camera-to-world pose, in float64"""
    p = np.asarray(pose, np.float32).astype(np.float64).reshape(16)
    a = np.zeros((3, 4), np.float64)
    for i in range(3):
        for k in range(3):
            a[i, k] = p[4 * k + i]
        s = p[i] * p[3]
        s = s + p[4 + i] * p[7]
        s = s + p[8 + i] * p[11]
        a[i, 3] = -s
    return a


def _edge(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _owns(ax, ay, bx, by):
    return by < ay or (by == ay and bx > ax)


def np_render(vertices, triangles, poses, K, h, w, z_near=Z_NEAR, counts=None):
    """-> (depth uint16 [F, h, w], status int32 [F, 2]).  ``counts``: a dict whose "fragments" is raised by the number of
    (triangle, covered pixel centre) pairs that reach the minimum of rule (h) -- what tools/render_bench.py divides by time"""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    vertices = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    F = poses.shape[0]
    depth = np.zeros((F, h, w), np.uint16)
    status = np.zeros((F, 2), np.int32)
    for f in range(F):
        a = np_camera(poses[f])
        zbuf = np.full((h, w), EMPTY, np.int64)
        for tri in triangles:
            cam = []
            for x, y, z in vertices[tri]:
                cam.append([((a[r, 0] * x + a[r, 1] * y) + a[r, 2] * z) + a[r, 3] for r in range(3)])      # (b)
            if any(not (c[2] >= z_near) for c in cam):                                                      # (c)
                status[f, 0] += 1
                continue
            pts, outside = [], False
            with np.errstate(all="ignore"):
                for x, y, z in cam:                                                                         # (d)
                    sx = np.rint(((fx * x) / z + cx) * np.float64(256.0))
                    sy = np.rint(((fy * y) / z + cy) * np.float64(256.0))
                    if not (abs(sx) <= GUARD and abs(sy) <= GUARD):
                        outside = True
                        break
                    pts.append((int(sx), int(sy), z))
            if outside:
                status[f, 1] += 1
                continue
            (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = pts
            area = _edge(x0, y0, x1, y1, x2, y2)                                                            # (e), Python integers
            if area == 0:
                continue
            if area < 0:
                (x1, y1, z1), (x2, y2, z2) = (x2, y2, z2), (x1, y1, z1)
            # pixel centres 256 p + 128 inside the bounding box: ceil((lo - 128) / 256) <= p <= floor((hi - 128) / 256)
            px0, px1 = max(-((128 - min(x0, x1, x2)) // 256), 0), min((max(x0, x1, x2) - 128) // 256, w - 1)
            py0, py1 = max(-((128 - min(y0, y1, y2)) // 256), 0), min((max(y0, y1, y2) - 128) // 256, h - 1)
            if px1 < px0 or py1 < py0:
                continue
            ccx = (256 * np.arange(px0, px1 + 1, dtype=np.int64) + 128)[None, :]
            ccy = (256 * np.arange(py0, py1 + 1, dtype=np.int64) + 128)[:, None]
            cover = np.ones((py1 - py0 + 1, px1 - px0 + 1), bool)
            es = []
            for (ax, ay, bx, by) in ((x1, y1, x2, y2), (x2, y2, x0, y0), (x0, y0, x1, y1)):
                e = np.int64(bx - ax) * (ccy - np.int64(ay)) - np.int64(by - ay) * (ccx - np.int64(ax))
                cover &= (e > 0) | ((e == 0) & _owns(ax, ay, bx, by))
                es.append(e)
            with np.errstate(all="ignore"):
                s = (es[0].astype(np.float64) / z0 + es[1].astype(np.float64) / z1) + es[2].astype(np.float64) / z2   # (f)
                z = (es[0] + es[1] + es[2]).astype(np.float64) / s
                if z0 == z1 and z1 == z2:
                    z = np.full(s.shape, z0, np.float64)
                q = z * np.float64(1000.0)                                                                   # (g)
            ok = cover & (q >= 1.0) & (q < 65536.0)
            mm = np.where(ok, np.trunc(np.where(ok, q, 1.0)), EMPTY).astype(np.int64)
            if counts is not None:
                counts["fragments"] = counts.get("fragments", 0) + int(ok.sum())
            view = zbuf[py0:py1 + 1, px0:px1 + 1]
            np.minimum(view, mm, out=view)                                                                   # (h)
        depth[f] = np.where(zbuf == EMPTY, 0, zbuf).astype(np.uint16)
    return depth, status


def np_masks(depth_f, depth_b=None, threshold=10):
    """computeForegroundMask + computeForegroundMaskFromDepthImagePair / computeForegroundMaskUsingCropStrategy
    -> (mask uint8, visible uint8, depth_change uint16)"""
    f = depth_f.astype(np.int32)
    if depth_b is None:
        mask = f > 0
    else:
        b = depth_b.astype(np.int32)
        big = np.iinfo(np.int32).max
        f, b = np.where(f == 0, big, f), np.where(b == 0, big, b)
        mask = (b - f) > threshold
    return mask.astype(np.uint8), (mask * 255).astype(np.uint8), (mask * f).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ scenes
def pinhole(h, w):
    """A dyadic camera: with it and depths that are powers of two, a vertex lands on the 1/256 grid where it is put"""
    return (64.0, 64.0, float(w // 2), float(h // 2))


def at_pixels(K, uvz):
    """World-frame vertices (identity pose) that project to the given (u, v) pixel coordinates at depth z"""
    fx, fy, cx, cy = K
    return np.array([[(u - cx) * z / fx, (v - cy) * z / fy, z] for u, v, z in uvz], np.float32)


def poses_for(F):
    """F distinct camera-to-world poses: the identity, a translation, a rotation about a tilted axis with a translation"""
    out = [np.eye(4)]
    t = np.eye(4)
    t[:3, 3] = [0.0625, -0.03125, 0.015625]
    out.append(t)
    ang, axis = 0.3, np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(4)
    r[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx.dot(Kx)
    r[:3, 3] = [-0.05, 0.02, -0.1]
    out.append(r)
    return np.stack(out[:F]).astype(np.float32)


def mixed_scene(h, w, seed, n_small=203):
    """One triangle over the whole image at z = 2 (the large path) and n_small triangles of 1-3 pixels at random dyadic depths
    (the small path).  V = 3 * (n_small + 1) and T = n_small + 1 are no multiples of 64."""
    rng = np.random.RandomState(seed)
    K = pinhole(h, w)
    uvz = [(-2.0 * w - 8, -2.0 * h - 8, 2.0), (4.0 * w + 8, -2.0 * h - 8, 2.0), (-2.0 * w - 8, 4.0 * h + 8, 2.0)]
    for _ in range(n_small):
        u0, v0 = rng.randint(-2 * 256, (w + 2) * 256) / 256.0, rng.randint(-2 * 256, (h + 2) * 256) / 256.0
        for k in range(3):
            du, dv = rng.randint(0, 3 * 256 + 1, 2) / 256.0
            uvz.append((u0 + du, v0 + dv, rng.randint(32, 160) / 64.0))
    verts = at_pixels(K, uvz)
    tris = np.arange(3 * (n_small + 1), dtype=np.int32).reshape(-1, 3)
    assert verts.shape[0] % 64 and tris.shape[0] % 64
    return verts, tris, K


# ------------------------------------------------------------------------------------------------ running
def run(verts, tris, poses, K, h, w, device, z_near=Z_NEAR, large_threshold=None):
    from dcn_hip import render
    mesh = render.Mesh(verts, tris, device=device)
    depth, status = render.render_depth(mesh, poses, K, (h, w), z_near=z_near, large_threshold=large_threshold)
    return depth.cpu().numpy().view(np.uint16), status.cpu().numpy()


def check_equal(got, want, what):
    (gd, gs), (wd, ws) = got, want
    assert gd.shape == wd.shape and gd.dtype == wd.dtype
    bad = np.argwhere(gd != wd)
    assert bad.size == 0, "%s: %d pixels differ, first %s: %d, statement %d" % (
        what, len(bad), tuple(bad[0]), gd[tuple(bad[0])], wd[tuple(bad[0])])
    assert np.array_equal(gs, ws), "%s: status %s, statement %s" % (what, gs.tolist(), ws.tolist())


def check_every_path(verts, tris, poses, K, h, w, device, what, z_near=Z_NEAR):
    """The default split, every triangle on the tiled path, every triangle on the one-lane path: each equals the statement
    (and so each other)."""
    want = np_render(verts, tris, poses, K, h, w, z_near)
    for name, thr in (("default", None), ("all large", ALL_LARGE), ("all small", ALL_SMALL)):
        check_equal(run(verts, tris, poses, K, h, w, device, z_near, thr), want, "%s, %s" % (what, name))
    return want


# ------------------------------------------------------------------------------------------------ the cases
def check_mixed(h, w, F, device):
    verts, tris, K = mixed_scene(h, w, seed=h * 100 + w + F)
    poses = poses_for(F)
    depth, status = check_every_path(verts, tris, poses, K, h, w, device, "mixed %dx%d F=%d" % (h, w, F))
    assert np.all(depth[0] > 0) and np.any(depth[0] < 2000) and np.any(depth[0] == 2000)   # both kinds of triangle show
    if F == 3:
        assert not np.array_equal(depth[0], depth[1]) and not np.array_equal(depth[0], depth[2])


def shared_edge_scenes(h=48, w=64):
    """name -> (uvz of two triangles A (z = 1) and B (z = 2) sharing an edge that runs through pixel centres, the centres on
    that edge, the depth they must show).  The triangle the top-left rule gives the edge to is the FAR one, so the edge's
    centres read 2000 only when exactly that triangle drew them."""
    out = {}
    # level edge y = 20.5 from x = 10 to 40: B below it (the edge is B's top edge)
    out["horizontal"] = ([(10, 20.5, 1), (40, 20.5, 1), (25, 5, 1)], [(10, 20.5, 2), (40, 20.5, 2), (25, 40, 2)],
                         [(20, x) for x in range(10, 40)], 2000)
    # upright edge x = 30.5 from y = 8 to 40: B to its right (the edge is B's left edge)
    out["vertical"] = ([(30.5, 8, 1), (30.5, 40, 1), (5, 24, 1)], [(30.5, 8, 2), (30.5, 40, 2), (60, 24, 2)],
                       [(y, 30) for y in range(8, 40)], 2000)
    # diagonal through the centres (i + .5, i + .5), i = 5 .. 39: B above and to the right of it (its edge runs upwards)
    out["diagonal"] = ([(5, 5, 1), (40, 40, 1), (5, 40, 1)], [(5, 5, 2), (40, 40, 2), (40, 5, 2)],
                       [(i, i) for i in range(5, 40)], 2000)
    return out


def check_shared_edges(device, h=48, w=64):
    K = pinhole(h, w)
    for name, (ta, tb, centres, value) in sorted(shared_edge_scenes(h, w).items()):
        verts = at_pixels(K, ta + tb)
        for order in ([0, 1, 2, 3, 4, 5], [0, 2, 1, 3, 5, 4], [3, 4, 5, 0, 1, 2], [0, 2, 1, 3, 4, 5]):   # both windings, both orders
            tris = np.array(order, np.int32).reshape(2, 3)
            depth, _ = check_every_path(verts, tris, poses_for(1), K, h, w, device, "shared edge " + name)
            for (y, x) in centres:
                assert depth[0, y, x] == value, (name, y, x, depth[0, y, x])
            assert set(np.unique(depth)) == {0, 1000, 2000}


def check_vertex_on_centre(device, h=48, w=64):
    """Four triangles at four depths around the centre of pixel (10, 20): the centre belongs to exactly one of them, and a
    lone triangle with a vertex on a centre follows the two edges that meet there"""
    K = pinhole(h, w)
    c = (20.5, 10.5)
    ring = [(30.5, 10.5), (20.5, 22.5), (8.5, 10.5), (20.5, 2.5)]
    uvz, tris = [], []
    for k in range(4):
        z = [0.5, 1.0, 2.0, 4.0][k]
        uvz += [(c[0], c[1], z), (ring[k][0], ring[k][1], z), (ring[(k + 1) % 4][0], ring[(k + 1) % 4][1], z)]
        tris.append([3 * k, 3 * k + 1, 3 * k + 2])
    verts = at_pixels(K, uvz)
    depth, _ = check_every_path(verts, np.array(tris, np.int32), poses_for(1), K, h, w, device, "fan around a centre")
    assert depth[0, 10, 20] in (500, 1000, 2000, 4000)
    owners = []
    for k in range(4):
        d, _ = check_every_path(verts, np.array(tris[k:k + 1], np.int32), poses_for(1), K, h, w, device, "fan triangle %d" % k)
        owners.append(int(d[0, 10, 20]))
    assert sorted(owners)[:3] == [0, 0, 0] and max(owners) == depth[0, 10, 20], owners


def check_slivers_and_zero_area(device, h=48, w=64):
    K = pinhole(h, w)
    sliver = at_pixels(K, [(2.625, 3.125, 1), (30.25, 3.25, 1), (2.625, 3.375, 1)])           # between the rows of centres
    depth, status = check_every_path(sliver, np.array([[0, 1, 2]], np.int32), poses_for(1), K, h, w, device, "sliver")
    assert not depth.any() and not status.any()
    flat = at_pixels(K, [(5, 5, 1), (20, 20, 1), (35, 35, 1), (40, 10, 1)])
    tris = np.array([[0, 1, 2], [0, 0, 3], [3, 3, 3]], np.int32)                              # collinear, repeated vertices
    depth, status = check_every_path(flat, tris, poses_for(1), K, h, w, device, "zero area")
    assert not depth.any() and not status.any()


def check_intersecting(device, h=48, w=64):
    """Two triangles that cross: one recedes to the right, the other to the left; the pixel keeps the nearer"""
    K = pinhole(h, w)
    a = [(-20, -30, 1.0), (90, 24, 3.0), (-20, 80, 1.0)]
    b = [(90, -30, 1.0), (-20, 24, 3.0), (90, 80, 1.0)]
    verts = at_pixels(K, a + b)
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    depth, _ = check_every_path(verts, tris, poses_for(1), K, h, w, device, "intersecting")
    only_a = np_render(verts, tris[:1], poses_for(1), K, h, w)[0].astype(np.int64)
    only_b = np_render(verts, tris[1:], poses_for(1), K, h, w)[0].astype(np.int64)
    both = (only_a > 0) & (only_b > 0)
    assert both.sum() > 200 and np.array_equal(depth[both], np.minimum(only_a, only_b)[both])
    assert np.any(only_a[both] < only_b[both]) and np.any(only_b[both] < only_a[both])


def check_dropped_triangles(device, h=48, w=64):
    """Behind the camera, straddling z_near, a vertex exactly at z_near (kept), beyond the guard band, and one plain triangle:
    the dropped ones are counted by rule, as the statement counts them"""
    K = pinhole(h, w)
    z_near = 0.0625
    plain = [(5, 5, 1), (30, 8, 1), (10, 30, 1)]
    verts = np.concatenate([
        at_pixels(K, plain),
        np.array([[0.1, 0.1, -1.0], [0.3, 0.1, -1.0], [0.1, 0.4, -2.0]], np.float32),            # behind
        np.array([[0.0, 0.0, 0.03125], [0.2, 0.0, 1.0], [0.0, 0.2, 1.0]], np.float32),           # straddles z_near
        at_pixels(K, [(40, 30, 0.0625), (60, 30, 0.0625), (50, 44, 0.0625)]),                     # exactly at z_near: drawn
        np.array([[1.0e6, 0.0, 0.0625], [0.0, 0.0, 1.0], [0.0, 0.1, 1.0]], np.float32),          # beyond the guard band
        np.array([[0.0, -3.0e7, 1.0], [0.0, 0.0, 1.0], [0.1, 0.0, 1.0]], np.float32),            # beyond it in y
    ])
    tris = np.arange(18, dtype=np.int32).reshape(6, 3)
    depth, status = check_every_path(verts, tris, poses_for(1), K, h, w, device, "dropped", z_near=z_near)
    assert status.tolist() == [[2, 2]]
    assert depth[0, 35, 50] == 62 and depth[0, 10, 12] == 1000
    # three frames: the counts are per frame
    check_every_path(verts, tris, poses_for(3), K, h, w, device, "dropped F=3", z_near=z_near)


def check_off_screen(device, h=37, w=53):
    K = pinhole(h, w)
    uvz = [(-40, -40, 1), (-10, -40, 1), (-40, -5, 1),            # wholly off screen
           (w + 5, 5, 1), (w + 30, 5, 1), (w + 5, 30, 1),
           (-10, 10, 1), (20, 12, 1), (-10, 30, 2),               # partly: left, bottom right
           (w - 10, h - 10, 0.5), (w + 20, h - 8, 0.5), (w - 12, h + 25, 0.5)]
    verts = at_pixels(K, uvz)
    tris = np.arange(12, dtype=np.int32).reshape(4, 3)
    depth, status = check_every_path(verts, tris, poses_for(1), K, h, w, device, "off screen")
    assert not status.any() and depth[0, h - 5, w - 5] == 500 and depth[0, 12, 0] > 0
    off = np_render(verts, tris[:2], poses_for(1), K, h, w)[0]
    assert not off.any()


def check_no_triangles(device, h=37, w=53):
    from dcn_hip import render
    for verts in (np.zeros((0, 3), np.float32), np.zeros((5, 3), np.float32)):
        mesh = render.Mesh(verts, np.zeros((0, 3), np.int32), device=device)
        depth, status = render.render_depth(mesh, poses_for(3), pinhole(h, w), (h, w))
        assert tuple(depth.shape) == (3, h, w) and not depth.cpu().numpy().any() and not status.cpu().numpy().any()


def check_millimetre_boundaries(device, h=48, w=64):
    """Triangles facing the camera store their own depth's millimetres; 65.536 m and beyond store 0"""
    K = pinhole(h, w)
    far = float(np.float32(65.536))
    zs = [0.5, 1.0, 2.0, 0.25, far, 66.0, 65.5, 0.001 * 777]
    uvz, want = [], []
    for k, z in enumerate(zs):
        u0 = 2 + 7 * k
        uvz += [(u0, 4, z), (u0 + 6, 4, z), (u0, 40, z)]
    verts = at_pixels(K, uvz)
    tris = np.arange(3 * len(zs), dtype=np.int32).reshape(-1, 3)
    depth, _ = check_every_path(verts, tris, poses_for(1), K, h, w, device, "millimetre boundaries")
    col = lambda k: int(depth[0, 6, 2 + 7 * k])
    assert [col(0), col(1), col(2), col(3)] == [500, 1000, 2000, 250]
    assert far * 1000.0 >= 65536.0 and col(4) == 0 and col(5) == 0
    assert col(6) == 65500 and col(7) == 777                # (facing the camera: the vertex depth itself)
    # a far surface does not hide a near one, whatever the order
    uvz = [(2, 4, 70.0), (40, 4, 70.0), (2, 40, 70.0), (2, 4, 1.0), (40, 4, 1.0), (2, 40, 1.0)]
    depth, _ = check_every_path(at_pixels(K, uvz), np.array([[0, 1, 2], [3, 4, 5]], np.int32), poses_for(1), K, h, w, device,
                                "beyond the range")
    assert depth[0, 6, 4] == 1000


def check_repeatable_and_order_free(device, h=37, w=53):
    verts, tris, K = mixed_scene(h, w, seed=11)
    poses = poses_for(3)
    first = run(verts, tris, poses, K, h, w, device)
    again = run(verts, tris, poses, K, h, w, device)
    check_equal(again, first, "second run")
    perm = np.random.RandomState(5).permutation(len(tris))
    for thr in (None, ALL_LARGE, ALL_SMALL):
        check_equal(run(verts, tris[perm], poses, K, h, w, device, large_threshold=thr), first, "permuted triangles")
    check_equal(run(verts, tris[:, [1, 2, 0]], poses, K, h, w, device), first, "rotated vertex order")
    check_equal(run(verts, tris[:, [0, 2, 1]], poses, K, h, w, device), first, "other winding")


def check_pairgen_convention(device, h=48, w=64):
    """A plane facing the camera at z = 1, a strip of it 40 columns wide, seen from the identity and from a camera moved
    0.03125 m along its x: K = (512, 512, 32, 24) moves the strip 16 columns to the LEFT and leaves the rows alone.  Every match
    dcn_hip.pairgen finds between the two depth images is displaced by exactly that -- a flipped axis or a transposed pose
    moves the strip elsewhere and the matches with it."""
    from dcn_hip import pairgen, render
    K = (512.0, 512.0, 32.0, 24.0)
    Km = np.array([[512.0, 0, 32.0], [0, 512.0, 24.0], [0, 0, 1.0]])
    verts = at_pixels(K, [(20, -10, 1), (60, -10, 1), (60, 100, 1), (20, 100, 1)])
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    moved = np.eye(4)
    moved[0, 3] = 0.03125
    poses = np.stack([np.eye(4), moved])
    mesh = render.Mesh(verts, tris, device=device)
    depth, status = render.render_depth(mesh, poses, K, (h, w))
    d = depth.cpu().numpy().view(np.uint16)
    want = np.zeros((2, h, w), np.uint16)
    want[0, :, 20:60] = 1000
    want[1, :, 4:44] = 1000
    assert np.array_equal(d, want) and not status.cpu().numpy().any()
    check_equal((d, status.cpu().numpy()), np_render(verts, tris, poses, K, h, w), "plane")
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cand_u = torch.from_numpy(uu.reshape(-1).astype(np.int64)).to(device)
    cand_v = torch.from_numpy(vv.reshape(-1).astype(np.int64)).to(device)
    ua, va, ub, vb = pairgen.find_correspondences(depth[0], depth[1], Km, poses[0], poses[1], cand_u, cand_v)
    ua, va, ub, vb = (x.cpu().numpy() for x in (ua, va, ub, vb))
    # every pixel of the strip and nothing else; pairgen, as the reference, drops a projection with a coordinate of exactly 0,
    # which is row 0 here
    assert len(ua) == 40 * (h - 1) and va.min() == 1 and va.max() == h - 1
    assert np.array_equal(ub, (ua - 16).astype(np.float32)) and np.array_equal(vb, va.astype(np.float32))
    assert ua.min() == 20 and ua.max() == 59


def check_masks_golden(name, device):
    from dcn_hip import render
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    f, b = z["depth_f"], z["depth_b"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int16))).to(device)
    for k, thr in enumerate(z["thresholds"].tolist()):
        mask, visible, change = render.foreground_masks(t(f), t(b), threshold=thr)
        assert np.array_equal(mask.cpu().numpy(), z["mask"][k]), (name, thr)
        assert np.array_equal(visible.cpu().numpy(), z["visible"][k])
        assert np.array_equal(change.cpu().numpy().view(np.uint16), z["depth_change"][k])
        for got, want in zip((mask, visible, change), np_masks(f, b, thr)):
            assert np.array_equal(got.cpu().numpy().view(want.dtype), want)
    mask, visible, change = render.foreground_masks(t(f))
    assert np.array_equal(mask.cpu().numpy(), z["crop_mask"]) and np.array_equal(visible.cpu().numpy(), z["crop_visible"])
    assert np.array_equal(change.cpu().numpy().view(np.uint16), f)


def check_argument_errors(device):
    import pytest
    from dcn_hip import render
    K = pinhole(8, 8)
    mesh = render.Mesh(at_pixels(K, [(1, 1, 1), (6, 1, 1), (1, 6, 1)]), [[0, 1, 2]], device=device)
    with pytest.raises(RuntimeError):
        render.render_depth(mesh, poses_for(1), K, (8, 8), z_near=0.0)
    with pytest.raises(ValueError):
        render.render_depth(mesh, poses_for(1), K, (0, 8))
    with pytest.raises(ValueError):
        render.render_depth(mesh, np.eye(3), K, (8, 8))
    with pytest.raises(ValueError):
        render.Mesh(np.zeros((3, 3), np.float32), [[0, 1, 3]], device=device)
    with pytest.raises(ValueError):
        render.Mesh(np.zeros((3, 2), np.float32), [[0, 1, 2]], device=device)
    d = torch.zeros((2, 8, 8), dtype=torch.int16, device=device)
    with pytest.raises(ValueError):
        render.foreground_masks(d, d, threshold=-1)
    with pytest.raises(ValueError):
        render.foreground_masks(d.float())
    if device != "cpu":
        with pytest.raises(RuntimeError):
            render.Mesh(np.zeros((3, 3), np.float32), [[0, 1, 2]], device="cpu")


# ------------------------------------------------------------------------------------------------ PLY files
def _ply_mesh():
    rng = np.random.RandomState(3)
    verts = rng.normal(0, 1, (7, 3)).astype(np.float32)
    tris = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3], [1, 5, 2]], np.int32)
    return verts, tris


def write_ply(path, verts, faces, binary, extra=False):
    """A PLY file as meshing tools write them (``extra``: normals-like vertex properties and a face property to skip)"""
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by the test",
            "element vertex %d" % len(verts), "property float x", "property float y", "property float z"]
    if extra:
        head += ["property uchar red", "property double quality"]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices"]
    if extra:
        head += ["property uchar flags"]
    head += ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for k, v in enumerate(verts):
            if binary:
                f.write(np.asarray(v, "<f4").tobytes())
                if extra:
                    f.write(np.uint8(k).tobytes() + np.asarray(0.5 * k, "<f8").tobytes())
            else:
                f.write((" ".join(repr(float(x)) for x in v) + (" %d %r" % (k, 0.5 * k) if extra else "") + "\n").encode())
        for face in faces:
            if binary:
                f.write(np.uint8(len(face)).tobytes() + np.asarray(face, "<i4").tobytes())
                if extra:
                    f.write(np.uint8(7).tobytes())
            else:
                f.write((" ".join(str(int(x)) for x in [len(face)] + list(face)) + (" 7" if extra else "") + "\n").encode())


def check_ply(device, tmp_path):
    import pytest
    from dcn_hip import render
    verts, tris = _ply_mesh()
    for binary in (True, False):
        for extra in (False, True):
            path = str(tmp_path / ("mesh_%d_%d.ply" % (binary, extra)))
            write_ply(path, verts, tris, binary, extra)
            v, t = render.read_ply(path)
            assert v.dtype == np.float32 and t.dtype == np.int32
            assert np.array_equal(v, verts) and np.array_equal(t, tris), (binary, extra)
            mesh = render.Mesh.from_ply(path, device=device)
            assert np.array_equal(mesh.vertices.cpu().numpy(), verts) and np.array_equal(mesh.triangles.cpu().numpy(), tris)
        quad = str(tmp_path / ("quad_%d.ply" % binary))
        write_ply(quad, verts, [[0, 1, 2], [2, 3, 4, 5], [4, 5, 6]], binary)
        with pytest.raises(render.PlyError, match="face 1 has 4 vertices"):
            render.read_ply(quad)
    big = str(tmp_path / "big_endian.ply")
    with open(big, "wb") as f:
        f.write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                b"element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(render.PlyError, match="binary_big_endian"):
        render.read_ply(big)
    bad = str(tmp_path / "index.ply")
    write_ply(bad, verts, [[0, 1, 9]], False)
    with pytest.raises(render.PlyError, match="outside"):
        render.read_ply(bad)


# ------------------------------------------------------------------------------------------------ scene -> store -> batch
def box_over_plane():
    """-> (foreground mesh arrays: a box 0.3 m wide whose top is 0.875 m from the cameras, full mesh arrays: the box and
    the table under it at 1.25 m; both depths are dyadic, so their millimetres are exact)"""
    lo, hi = np.array([-0.025, -0.025, 0.875]), np.array([0.275, 0.275, 1.25])
    corners = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box_t = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    table = np.array([[-4, -4, 1.25], [4, -4, 1.25], [4, 4, 1.25], [-4, 4, 1.25]], np.float32)
    full_v = np.concatenate([corners, table])
    full_t = np.concatenate([box_t, np.array([[8, 9, 10], [8, 10, 11]], np.int32)])
    return (corners, box_t), (full_v, full_t)


def scene_poses():
    out = []
    for t in ([0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0.25, 0.25, 0]):
        p = np.eye(4)
        p[:3, 3] = t
        out.append(p)
    return np.stack(out)


def scene_config():
    probs = dict.fromkeys(("SINGLE_OBJECT_ACROSS_SCENE", "DIFFERENT_OBJECT", "MULTI_OBJECT", "SYNTHETIC_MULTI_OBJECT"), 0.0)
    probs["SINGLE_OBJECT_WITHIN_SCENE"] = 1.0
    return {"training": dict(num_matching_attempts=2000, sample_matches_only_off_mask=True, num_non_matches_per_match=4,
                             fraction_masked_non_matches=0.5, fraction_background_non_matches=0.5, cross_scene_num_samples=20,
                             use_image_b_mask_inv=True, domain_randomize=False, data_type_probabilities=probs)}


BOX_K = (64.0, 64.0, 24.0, 16.0)


def box_scene_on(device):
    """-> (foreground Mesh, full Mesh, poses float64 [4, 4, 4]) on the device: what a scene's files and pose log become once"""
    from dcn_hip import render
    (fg_v, fg_t), (full_v, full_t) = box_over_plane()
    return (render.Mesh(fg_v, fg_t, device=device), render.Mesh(full_v, full_t, device=device),
            torch.from_numpy(scene_poses()).to(device))


def render_box_scene(scene, h=48, w=64):
    """-> (SceneImages, K, foreground arrays, full arrays); ``scene`` from box_scene_on: nothing crosses to or from the host"""
    from dcn_hip import render
    fg, full, poses = scene
    return (render.render_scene(fg, full, poses, BOX_K, (h, w)), BOX_K) + box_over_plane()


def check_scene_images(im, K, fg, full, h=48, w=64):
    """render_scene's four images against the statement and the reference's mask rule"""
    poses = scene_poses()
    d = im.depth.cpu().numpy().view(np.uint16)
    dc = im.depth_cropped.cpu().numpy().view(np.uint16)
    check_equal((d, im.status.cpu().numpy()), np_render(full[0], full[1], poses, K, h, w), "full mesh")
    check_equal((dc, im.status_cropped.cpu().numpy()), np_render(fg[0], fg[1], poses, K, h, w), "foreground mesh")
    mask, visible, _ = np_masks(dc)
    assert np.array_equal(im.mask.cpu().numpy(), mask) and np.array_equal(im.visible_mask.cpu().numpy(), visible)
    assert np.all(d > 0) and set(np.unique(d[mask == 0])) == {1250} and d[mask == 1].min() == 875
    assert np.array_equal(d[mask == 1], dc[mask == 1])            # the box hides the table, never the reverse
    assert all(200 < int(m.sum()) < h * w // 2 for m in mask)


def store_of(im, K, device, h=48, w=64):
    from dcn_hip import frames
    F = int(im.depth.shape[0])
    g = torch.Generator().manual_seed(4)
    rgb = torch.randint(0, 256, (F, h, w, 3), dtype=torch.uint8, generator=g).to(device)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    return frames.FrameStore.from_tensors(rgb, im.depth, im.mask, scene_poses(), [0, F], [0], Km)


def check_batch(sb, data_type):
    off = sb.offsets.cpu().numpy()
    assert int(sb.status[0]) == 0 and data_type == 0
    assert not bool(sb.empty.any()) and sb.type.cpu().tolist() == [0] * len(sb.empty)
    B = len(sb.empty)
    for p in range(B):
        assert off[4 * p + 1] - off[4 * p] > 50, "pair %d has %d matches" % (p, off[4 * p + 1] - off[4 * p])
    assert sb.idx_a.device == sb.offsets.device


def check_written_images(im, tmp_path):
    from PIL import Image
    from dcn_hip import render
    ids = [0, 7, 12, 345]
    paths = render.write_scene_images(str(tmp_path), ids, im)
    assert len(paths) == 16
    d = im.depth.cpu().numpy().view(np.uint16)
    dc = im.depth_cropped.cpu().numpy().view(np.uint16)
    for j, i in enumerate(ids):
        rd = np.asarray(Image.open(str(tmp_path / "rendered_images" / ("%06d_depth.png" % i))))
        rc = np.asarray(Image.open(str(tmp_path / "rendered_images" / ("%06d_depth_cropped.png" % i))))
        rm = np.asarray(Image.open(str(tmp_path / "image_masks" / ("%06d_mask.png" % i))))
        rv = np.asarray(Image.open(str(tmp_path / "image_masks" / ("%06d_visible_mask.png" % i))))
        assert rd.astype(np.int64).max() > 255 and np.array_equal(rd.astype(np.uint16), d[j])
        assert np.array_equal(rc.astype(np.uint16), dc[j])
        assert rm.dtype == np.uint8 and np.array_equal(rm, im.mask[j].cpu().numpy())
        assert np.array_equal(rv, im.visible_mask[j].cpu().numpy())
