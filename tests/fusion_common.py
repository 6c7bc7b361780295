"""Checks of TSDF fusion, surface extraction and the box crop (csrc/fusion_kernels.hip, csrc/fusion_rules.h, dcn_hip/fusion.py),
shared by tests/test_emu_fusion.py (host emulation) and tests/test_gpu_fusion.py (MI355X).

``np_integrate``, ``np_extract`` and ``np_crop`` are the yardsticks: the rules of include/dcn_hip.h section 17 in numpy float64
and integers, written from the header's text.  Every float64 step is one numpy operation (one correctly rounded IEEE
operation), every other step is integer: sums, weights, status, vertices, triangles and counts must EQUAL them -- the only
tolerance in this file is the derived bound of the plane test.  The crop's segment geometry is pinned to the reference's own
lines by tests/golden/fusion_ref_crop_*.npz (tests/golden/make_fusion_from_reference.py); fusion and extraction have no
reference text to pin to."""
import itertools
import os

import numpy as np
import torch

import render_common as rc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CROP_GOLDENS = ("fusion_ref_crop_box", "fusion_ref_crop_rotated")
VOLUMES = ((8, 8, 8), (5, 7, 9), (33, 17, 9))          # (nx, ny, nz)
IMAGES = ((12, 16), (30, 40))                          # (h, w)
FRAME_COUNTS = (1, 3, 8)
CHUNK = 2                                              # frames per launch that F = 3 and F = 8 cross, F = 3 unevenly
MAX_WEIGHT = 65535
MAX_DEPTH_MM = 6000

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # tetrahedron id -> (a, b, c), x < y < z
DIR_BITS = (1, 2, 4, 3, 5, 6, 7)                                               # direction id -> corner bits: x y z xy xz yz xyz


# ------------------------------------------------------------------------------------------------ 17a: the numpy statement
def np_integrate(state, depth, poses, K, origin, s, mu, pixel_offset=0.5, max_depth_mm=MAX_DEPTH_MM):
    """state = (sum int32 [nz, ny, nx], weight int32 [nz, ny, nx], status int64 [1]) is advanced in place by the frames in
    their order; depth uint16 [F, h, w], poses [F, 4, 4]"""
    total, weight, status = state
    nz, ny, nx = total.shape
    fx, fy, cx, cy = (np.float64(k) for k in K)
    o, s, mu = np.float64(pixel_offset), np.float64(s), np.float64(mu)
    depth = np.asarray(depth).view(np.uint16)
    F, h, w = depth.shape
    poses = np.asarray(poses, np.float32).reshape(F, 4, 4)
    wx = (np.float64(origin[0]) + s * np.arange(nx, dtype=np.float64))[None, None, :]           # step 1
    wy = (np.float64(origin[1]) + s * np.arange(ny, dtype=np.float64))[None, :, None]
    wz = (np.float64(origin[2]) + s * np.arange(nz, dtype=np.float64))[:, None, None]
    for f in range(F):
        a = rc.np_camera(poses[f])                                                               # 16(a)
        with np.errstate(all="ignore"):
            x, y, z = (((a[r, 0] * wx + a[r, 1] * wy) + a[r, 2] * wz) + a[r, 3] for r in range(3))   # 16(b)
            ok = z > 0                                                                           # step 3
            pu = np.floor(((fx * x) / z + cx) + o)                                               # step 4
            pv = np.floor(((fy * y) / z + cy) + o)
            ok = ok & (pu >= 0) & (pu < w) & (pv >= 0) & (pv < h)
            mm = depth[f][np.where(ok, pv, 0).astype(np.int64), np.where(ok, pu, 0).astype(np.int64)].astype(np.int64)
            ok = ok & (mm != 0) & (mm <= max_depth_mm)                                           # step 6
            diff = mm.astype(np.float64) / np.float64(1000.0) - z                                # step 7
            ok = ok & (diff > -mu)
            q = np.rint(np.minimum(np.float64(1.0), diff / mu) * np.float64(32768.0))            # step 8
        full = ok & (weight >= MAX_WEIGHT)                                                       # step 9
        take = ok & ~full
        total[take] += q[take].astype(np.int32)                                                  # step 10
        weight[take] += 1
        status[0] += int(full.sum())
    return state


def empty_state(shape):
    nx, ny, nz = shape
    return np.zeros((nz, ny, nx), np.int32), np.zeros((nz, ny, nx), np.int32), np.zeros(1, np.int64)


# ------------------------------------------------------------------------------------------------ 17b: the numpy statement
def tet_corners(tet):
    a, b, _ = PERMS[tet]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def case_edges(m):
    """The crossed edges (p, q) -- p inside, q outside, positions among the tetrahedron's four vertices -- and the triangles
    over them, before orientation"""
    inside = [k for k in range(4) if m >> k & 1]
    outside = [k for k in range(4) if not m >> k & 1]
    if len(inside) == 1:
        return [(inside[0], q) for q in outside], [(0, 1, 2)]
    if len(inside) == 2:
        (p1, p2), (q1, q2) = inside, outside
        return [(p1, q1), (p1, q2), (p2, q2), (p2, q1)], [(0, 1, 2), (0, 2, 3)]
    if len(inside) == 3:
        return [(p, outside[0]) for p in inside], [(0, 1, 2)]
    return [], []


def derive_table():
    """table[tet][m] = the triangles, each three (corner, corner) cube edges, oriented on the unit cube with every t = 1/2 so
    that the normal points from the inside corners to the outside ones"""
    table = []
    for tet in range(6):
        corners = tet_corners(tet)
        pos = [np.array([c & 1, c >> 1 & 1, c >> 2 & 1], np.float64) for c in corners]
        row = []
        for m in range(16):
            edges, tris = case_edges(m)
            out = []
            if edges:
                pts = [(pos[p] + pos[q]) / 2.0 for p, q in edges]
                ins = np.mean([pos[k] for k in range(4) if m >> k & 1], axis=0)
                outs = np.mean([pos[k] for k in range(4) if not m >> k & 1], axis=0)
                for i0, i1, i2 in tris:
                    side = np.dot(np.cross(pts[i1] - pts[i0], pts[i2] - pts[i0]), outs - ins)
                    assert side != 0
                    if side < 0:
                        i1, i2 = i2, i1
                    out.append(tuple((corners[edges[i][0]], corners[edges[i][1]]) for i in (i0, i1, i2)))
            row.append(out)
        table.append(row)
    return table


def packed_cases():
    """The 16 words csrc/fusion_rules.h carries, derived: see tet_case there.  Asserts that mirror-image tetrahedra differ in
    the exchange bit only."""
    table = derive_table()
    words = []
    for m in range(16):
        edges, tris = case_edges(m)
        word = len(tris) << 16
        for e, (p, q) in enumerate(edges):
            word |= (p | q << 2) << (4 * e)
        flips = []
        for tet in range(6):
            corners = tet_corners(tet)
            plain = [tuple((corners[edges[i][0]], corners[edges[i][1]]) for i in t) for t in tris]
            flipped = [(t[0], t[2], t[1]) for t in plain]
            assert table[tet][m] in (plain, flipped)
            odd = PERMS[tet] in ((0, 2, 1), (1, 0, 2), (2, 1, 0))
            flips.append(bool(tris) and (table[tet][m] == flipped) != odd)
        assert len(set(flips)) == 1, (m, flips)
        words.append(word | (int(flips[0]) << 18))
    return words


def _at(arr, dz, dy, dx, fill):
    """out[k, j, i] = arr[k + dz, j + dy, i + dx], ``fill`` outside"""
    nz, ny, nx = arr.shape[:3]
    out = np.full(arr.shape, fill, arr.dtype)
    src = [slice(max(d, 0), n + min(d, 0)) for d, n in ((dz, nz), (dy, ny), (dx, nx))]
    dst = [slice(max(-d, 0), n + min(-d, 0)) for d, n in ((dz, nz), (dy, ny), (dx, nx))]
    if all(s.stop > s.start for s in src):
        out[tuple(dst)] = arr[tuple(src)]
    return out


def np_extract(total, weight, origin, s, min_weight=1, max_vertices=None, max_triangles=None, used=None, edges=None):
    """-> (vertices float32 [V', 3], triangles int32 [T', 3], counts [2]) with V' = min(V, max_vertices) and
    T' = max_triangles if given (unused rows and rows naming an unwritten vertex are -1) else T.  ``used``: a set that receives
    (tetrahedron id, case) of every tetrahedron of a valid cube; ``edges``: a list that receives (k, j, i, direction id) of
    the vertices, in their order."""
    nz, ny, nx = total.shape
    inside = total < 0
    ok = weight >= min_weight
    valid = np.ones((nz, ny, nx), bool)
    for c in range(8):
        valid &= _at(ok, c >> 2 & 1, c >> 1 & 1, c & 1, False)
    with np.errstate(all="ignore"):
        f = total.astype(np.float64) / weight.astype(np.float64)
    active = np.zeros((nz, ny, nx, 7), bool)
    for d, bits in enumerate(DIR_BITS):
        dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
        there = _at(np.ones((nz, ny, nx), bool), dz, dy, dx, False)
        crossed = there & (inside != _at(inside, dz, dy, dx, False))
        holds = np.zeros((nz, ny, nx), bool)                 # a valid cube with both ends among its corners
        for ez, ey, ex in itertools.product(*[(0,) if m else (0, 1) for m in (dz, dy, dx)]):
            holds |= _at(valid, -ez, -ey, -ex, False)
        active[..., d] = crossed & holds
    flat = active.reshape(-1).astype(np.int64)
    vid = (np.cumsum(flat) - flat).reshape(nz, ny, nx, 7)
    kk, jj, ii, dd = np.nonzero(active)                      # ascending (voxel linear index, direction id)
    if edges is not None:
        edges.append((kk, jj, ii, dd))
    bits = np.array(DIR_BITS)[dd]
    dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
    with np.errstate(all="ignore"):
        fa, fb = f[kk, jj, ii], f[kk + dz, jj + dy, ii + dx]
        t = fa / (fa - fb)
        g = [np.where(m == 1, x.astype(np.float64) + t, x.astype(np.float64)) for m, x in ((dx, ii), (dy, jj), (dz, kk))]
        vertices = np.stack([np.float64(origin[a]) + np.float64(s) * g[a] for a in range(3)], axis=1).astype(np.float32)
    vertices = vertices.reshape(-1, 3)
    ck, cj, ci = np.nonzero(valid)                           # ascending cube linear index
    n = len(ck)
    tri = np.full((n, 6, 2, 3), -1, np.int64)
    have = np.zeros((n, 6, 2), bool)
    table = derive_table()
    corner_in = [inside[ck + (c >> 2 & 1), cj + (c >> 1 & 1), ci + (c & 1)] for c in range(8)] if n else []
    for tet in range(6):
        corners = tet_corners(tet)
        m = sum(corner_in[c].astype(np.int64) << k for k, c in enumerate(corners)) if n else np.zeros(0, np.int64)
        for case in range(16):
            sel = np.flatnonzero(m == case)
            if not len(sel):
                continue
            if used is not None:
                used.add((tet, case))
            for slot, edges in enumerate(table[tet][case]):
                have[sel, tet, slot] = True
                for e, (c0, c1) in enumerate(edges):
                    lo, d = min(c0, c1), DIR_BITS.index(c0 ^ c1)
                    assert lo == c0 & c1
                    tri[sel, tet, slot, e] = vid[ck[sel] + (lo >> 2 & 1), cj[sel] + (lo >> 1 & 1), ci[sel] + (lo & 1), d]
    triangles = tri[have]
    counts = np.array([len(vertices), len(triangles)], np.int64)
    return _capped(vertices, triangles, counts, max_vertices, max_triangles)


def _capped(vertices, triangles, counts, max_vertices, max_triangles):
    if max_vertices is not None:
        vertices = vertices[:max_vertices]
        triangles = np.where((triangles >= max_vertices).any(axis=1, keepdims=True), -1, triangles)
    if max_triangles is not None:
        rows = np.full((max_triangles, 3), -1, np.int64)
        rows[:min(max_triangles, len(triangles))] = triangles[:max_triangles]
        triangles = rows
    return vertices, triangles.astype(np.int32).reshape(-1, 3), counts


# ------------------------------------------------------------------------------------------------ 17c: the numpy statement
def np_segments(transform, dimensions):
    """cropToBox / cropToLineSegment's geometry: per axis of the box frame (point1 [3], axis' [3], length'), float64 [3, 7]"""
    T = np.asarray(transform, np.float64).reshape(4, 4)
    origin = np.array(T[:3, 3])
    out = np.zeros((3, 7), np.float64)
    for a, length in enumerate(dimensions):
        crop_axis = np.array(T[:3, a]) * (np.float64(length) / 2.0)
        point1, point2 = origin - crop_axis, origin + crop_axis
        line = point2 - point1
        norm = np.linalg.norm(line)
        out[a, :3], out[a, 3:6], out[a, 6] = point1, line / norm, norm
    return out


def np_crop(vertices, triangles, transform, dimensions, max_vertices=None, max_triangles=None):
    """-> (vertices, triangles, counts) of the cropped mesh: a triangle survives when all its points have
    0 <= dot(p - point1, axis') <= length' on the three axes; the vertices in use keep their order and are renumbered"""
    seg = np_segments(transform, dimensions)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    keep_point = np.ones(len(v), bool)
    for a in range(3):
        d = [v[:, c] - seg[a, c] for c in range(3)]
        sc = (d[0] * seg[a, 3] + d[1] * seg[a, 4]) + d[2] * seg[a, 5]
        keep_point &= (sc >= 0.0) & (sc <= seg[a, 6])
    named = ((t >= 0) & (t < len(v))).all(axis=1)
    keep = named & keep_point[np.where(named[:, None], t, 0)].all(axis=1)
    in_use = np.zeros(len(v), bool)
    in_use[t[keep].reshape(-1)] = True
    new_id = np.cumsum(in_use) - in_use
    out_v = np.asarray(vertices, np.float32).reshape(-1, 3)[in_use]
    out_t = new_id[t[keep]].reshape(-1, 3)
    counts = np.array([len(out_v), len(out_t)], np.int64)
    return _capped(out_v, out_t, counts, max_vertices, max_triangles)


# ------------------------------------------------------------------------------------------------ running
def as_depth(a, device):
    """uint16 millimetres -> the store's int16 tensor with the same bits"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint16)).view(np.int16)).to(device)


def state_of(vol):
    return vol.sum.cpu().numpy(), vol.weight.cpu().numpy(), vol.status.cpu().numpy().astype(np.int64)


def check_state(vol, want, what):
    got = state_of(vol)
    for name, g, w in zip(("sum", "weight", "status"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: %s differs at %d places, first %s: %d, statement %d" % (
            what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


def volume_on(device, shape, origin, s, mu=None, state=None):
    from dcn_hip import fusion
    if state is None:
        return fusion.TsdfVolume(origin, s, shape, mu, device=device)
    return fusion.TsdfVolume.from_tensors(torch.from_numpy(state[0].copy()).to(device), torch.from_numpy(state[1].copy()).to(device),
                                          origin, s, mu, status=torch.from_numpy(state[2].astype(np.int32)).to(device))


def camera_for(h, w):
    """A dyadic pinhole under which a volume of some 0.1-0.5 m at 1 m reaches past the image on its long axis"""
    return (4.0 * w, 4.0 * w, w / 2.0, h / 2.0)


def poses_around(F, seed):
    """The identity, a camera INSIDE the volume (voxels behind it), a tilted rotation, a translation (render_common.poses_for),
    then random small rigid motions"""
    rng = np.random.RandomState(seed)
    out = list(rc.poses_for(3).astype(np.float64))
    inside = np.eye(4)
    inside[:3, 3] = [0.01, -0.02, 1.0]
    out.append(inside)
    while len(out) < F:
        axis = rng.normal(0, 1, 3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-0.25, 0.25)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        p = np.eye(4)
        p[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx.dot(Kx)
        p[:3, 3] = rng.uniform(-0.08, 0.08, 3)
        out.append(p)
    order = [0, 3, 2, 1] + list(range(4, len(out)))            # (F = 3: the identity, the camera inside, the rotation)
    return np.stack([out[k] for k in order][:F]).astype(np.float32)


def volume_geometry(shape):
    nx, ny, nz = shape
    s = 1.0 / 64.0
    return (-0.5 * nx * s, -0.5 * ny * s, 0.9375), s


def random_depth(F, h, w, seed):
    """Depths around the volume's, with the special values of rule 6 sprinkled in"""
    rng = np.random.RandomState(seed)
    d = rng.randint(900, 1200, (F, h, w)).astype(np.uint16)
    special = np.array([0, MAX_DEPTH_MM, MAX_DEPTH_MM + 1, 65535, 1, 1000], np.uint16)
    pick = rng.rand(F, h, w) < 0.15
    d[pick] = special[rng.randint(0, len(special), int(pick.sum()))]
    return d


# ------------------------------------------------------------------------------------------------ 17a: the cases
def check_integrate_random(shape, hw, F, device):
    """Random rigid poses around the volume: the default chunk, chunk = 2, and the frames split over two calls each equal the
    statement, for both pixel offsets"""
    h, w = hw
    origin, s = volume_geometry(shape)
    K = camera_for(h, w)
    poses = poses_around(F, seed=F + shape[0])
    depth = random_depth(F, h, w, seed=h + F)
    dev_depth = as_depth(depth, device)
    for o in (0.5, 0.0):
        want = np_integrate(empty_state(shape), depth, poses, K, origin, s, 5.0 * s, pixel_offset=o)
        assert want[1].max() >= 1
        for chunk in (None, CHUNK):
            vol = volume_on(device, shape, origin, s)
            vol.integrate(dev_depth, poses, K, pixel_offset=o, frames_per_launch=chunk)
            check_state(vol, want, "%s F=%d o=%s chunk=%s" % (shape, F, o, chunk))
        if F > 1:
            cut = F // 2
            vol = volume_on(device, shape, origin, s)
            vol.integrate(dev_depth[:cut], poses[:cut], K, pixel_offset=o, frames_per_launch=CHUNK)
            vol.integrate(dev_depth[cut:], torch.from_numpy(poses[cut:]).to(device), K, pixel_offset=o)
            check_state(vol, want, "%s F=%d o=%s two calls" % (shape, F, o))
    return want


EDGE_SHAPE = (8, 8, 8)
EDGE_ORIGIN = (0.0, 0.0, -0.25)         # z of the voxel layers: -0.25 (behind the camera), 0 (exactly), 0.25 .. 1.5
EDGE_S = 0.25
EDGE_K = (4.0, 4.0, 8.0, 6.0)           # u = 4 x / z + 8 on 16 columns, v = 4 y / z + 6 on 12 rows: integers at the grid's ratios
EDGE_DEPTHS = (500, 1000, 250, 0, MAX_DEPTH_MM, MAX_DEPTH_MM + 1, 65535, 1500)      # one constant image per frame


def edge_inputs():
    F = len(EDGE_DEPTHS)
    depth = np.stack([np.full((12, 16), d, np.uint16) for d in EDGE_DEPTHS])
    return depth, np.stack([np.eye(4, dtype=np.float32)] * F)


def check_integrate_edges(device):
    """Power-of-two geometry under the identity pose, constant images of 0.5 m, 1 m, 0.25 m, 0, max, max + 1, 65535 and 1.5 m:
    every equality of rules 3-8 is exact in float64.  The statement is asserted to take the branch each case is there for."""
    depth, poses = edge_inputs()
    above = float(np.nextafter(0.25, 1.0))
    for mu, o, max_mm in ((0.25, 0.0, MAX_DEPTH_MM), (0.25, 0.5, MAX_DEPTH_MM), (above, 0.0, MAX_DEPTH_MM),
                          (16384.0, 0.0, MAX_DEPTH_MM), (0.25, 0.0, 65535)):
        want = np_integrate(empty_state(EDGE_SHAPE), depth, poses, EDGE_K, EDGE_ORIGIN, EDGE_S, mu, o, max_mm)
        for chunk in (None, CHUNK):
            vol = volume_on(device, EDGE_SHAPE, EDGE_ORIGIN, EDGE_S, mu)
            vol.integrate(as_depth(depth, device), poses, EDGE_K, pixel_offset=o, max_depth_mm=max_mm, frames_per_launch=chunk)
            check_state(vol, want, "edges mu=%r o=%s max=%d chunk=%s" % (mu, o, max_mm, chunk))
        total, weight, _ = want
        assert not weight[0].any() and not weight[1].any()                       # behind the camera, z exactly 0
        one = lambda frame: np_integrate(empty_state(EDGE_SHAPE), depth[frame:frame + 1], poses[:1], EDGE_K, EDGE_ORIGIN,
                                         EDGE_S, mu, o, max_mm)
        if mu == 0.25 and max_mm == MAX_DEPTH_MM:
            # voxel (x, y, z) = (1.75, 0, 1.0) projects to column 15, the last; (0.5, 0, 0.25) to column 16, one past
            assert one(1)[1][5, 0, 7] == 1 and one(2)[1][2, 0, 2] == 0 and one(2)[1][2, 0, 1] == 1
            # rows: (0, 1.25, 1.0) to row 11, the last; (0, 1.5, 1.0) to row 12
            assert one(1)[1][5, 5, 0] == 1 and one(1)[1][5, 6, 0] == 0
            # frame 0 (0.5 m): z = 0.75 has diff == -mu and is skipped, z = 0.5 gives 0, z = 0.25 gives diff == mu: q = 32768
            t0, w0, _ = one(0)
            assert w0[4, 0, 0] == 0 and (w0[3, 0, 0], t0[3, 0, 0]) == (1, 0) and (w0[2, 0, 0], t0[2, 0, 0]) == (1, 32768)
            assert one(1)[0][2, 0, 0] == 32768                                   # diff = 0.75 > mu: clipped
            for frame in (3, 5, 6):                                              # depth 0, max + 1, 65535
                assert not one(frame)[1].any()
            assert one(4)[1].any() and set(np.unique(one(4)[0])) == {0, 32768}   # depth max itself is taken
        if mu == above:
            t0, w0, _ = one(0)                                                   # diff == -0.25 is now above -mu: taken
            assert w0[4, 0, 0] == 1 and t0[4, 0, 0] == -32768
        if mu == 16384.0:
            t0, w0, _ = one(0)                                                   # t * 32768 = 2 diff: 0.25 -> 0.5 -> 0 (tie)
            t1, w1, _ = one(1)                                                   # 0.75 -> 1.5 -> 2 (tie), 0.25 -> 0
            assert (w0[2, 0, 0], t0[2, 0, 0]) == (1, 0) and (w1[2, 0, 0], t1[2, 0, 0]) == (1, 2)
            assert (w0[4, 0, 0], t0[4, 0, 0]) == (1, 0) and (w1[6, 0, 0], t1[6, 0, 0]) == (1, 0)
            tl, wl, _ = one(7)                                                   # 1.5 m: diff 1.25 -> 2.5 -> 2, 0.75 -> 2, 0.25 -> 0
            assert (tl[2, 0, 0], tl[4, 0, 0], tl[6, 0, 0]) == (2, 2, 0) and wl[2, 0, 0] == 1
        if max_mm == 65535:
            assert one(6)[1].any()


def check_integrate_bad_poses(device):
    """A NaN entry and entries of 1e30: every frame with them is skipped everywhere, the others are taken"""
    shape, (h, w) = VOLUMES[1], IMAGES[0]
    origin, s = volume_geometry(shape)
    K = camera_for(h, w)
    depth = random_depth(3, h, w, seed=5)
    poses = poses_around(3, seed=2)[[1, 1, 1]].copy()
    poses[0, 1, 2] = np.nan
    poses[2, :3, :] = 1e30
    want = np_integrate(empty_state(shape), depth, poses, K, origin, s, 5.0 * s)
    alone = np_integrate(empty_state(shape), depth[1:2], poses[1:2], K, origin, s, 5.0 * s)
    assert alone[1].any() and all(np.array_equal(a, b) for a, b in zip(want, alone))
    vol = volume_on(device, shape, origin, s)
    vol.integrate(as_depth(depth, device), poses, K)
    check_state(vol, want, "bad poses")


def check_integrate_saturation(device):
    """weight 65534 preloaded, three frames that all reach a voxel: the first is taken, two are counted in status -- and it
    is the FIRST one's q that is added, whatever the chunking"""
    shape, (h, w) = VOLUMES[0], IMAGES[0]
    origin, s = volume_geometry(shape)
    K = camera_for(h, w)
    poses = np.stack([np.eye(4, dtype=np.float32)] * 3)
    depth = np.stack([np.full((h, w), d, np.uint16) for d in (1000, 1010, 990)])
    start = (np.full(shape[::-1], -7, np.int32), np.full(shape[::-1], MAX_WEIGHT - 1, np.int32), np.zeros(1, np.int64))
    want = np_integrate(tuple(a.copy() for a in start), depth, poses, K, origin, s, 5.0 * s)
    reached = want[1] == MAX_WEIGHT
    assert reached.any() and want[2][0] == 2 * int(reached.sum()) and want[1].max() == MAX_WEIGHT
    first = np_integrate(tuple(a.copy() for a in start), depth[:1], poses[:1], K, origin, s, 5.0 * s)
    assert np.array_equal(want[0], first[0])
    for chunk in (None, CHUNK, 1):
        vol = volume_on(device, shape, origin, s, state=start)
        vol.integrate(as_depth(depth, device), poses, K, frames_per_launch=chunk)
        check_state(vol, want, "saturation chunk=%s" % chunk)


def check_integrate_repeatable(device):
    shape, (h, w) = VOLUMES[2], IMAGES[1]
    origin, s = volume_geometry(shape)
    runs = []
    for _ in range(2):
        vol = volume_on(device, shape, origin, s)
        vol.integrate(as_depth(random_depth(8, h, w, 3), device), poses_around(8, 4), camera_for(h, w))
        runs.append(state_of(vol))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ 17b: the cases
def check_mesh(mesh_or_arrays, want, what):
    """vertices bit for bit, triangles and (where given) counts"""
    if isinstance(mesh_or_arrays, tuple):
        gv, gt, gc = mesh_or_arrays
    else:
        gv, gt, gc = mesh_or_arrays.vertices.cpu().numpy(), mesh_or_arrays.triangles.cpu().numpy(), None
    wv, wt, wc = want
    assert gv.shape == wv.shape and gt.shape == wt.shape, (what, gv.shape, wv.shape, gt.shape, wt.shape)
    assert gv.dtype == np.float32 and gt.dtype == np.int32
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), "%s: vertices differ" % what
    bad = np.argwhere(gt != wt)
    assert bad.size == 0, "%s: %d triangle entries differ, first at %s" % (what, len(bad), tuple(bad[0]))
    if gc is not None:
        assert np.array_equal(np.asarray(gc, np.int64), wc), (what, gc, wc)


def extract_on(device, state, origin, s, min_weight=1):
    from dcn_hip import fusion
    vol = volume_on(device, state[0].shape[::-1], origin, s, state=state)
    return fusion.extract_mesh(vol, min_weight=min_weight)


def plane_depth(h, w, poses, K, normal=(0.1, -0.05, 1.0), at=1.05):
    """Depth images (uint16, the host statement of the renderer) of a big tilted plane through (0, 0, at)"""
    n = np.array(normal) / np.linalg.norm(normal)
    a = np.cross(n, [0, 1, 0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    c = np.array([0, 0, at])
    verts = np.array([c - 3 * a - 3 * b, c + 3 * a - 3 * b, c + 3 * a + 3 * b, c - 3 * a + 3 * b], np.float32)
    return rc.np_render(verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32), poses, K, h, w)[0]


def integrated_state():
    """A tilted plane through the 33 x 17 x 9 volume, seen by three cameras: the state the statement integrates from
    rendered depth images"""
    shape, (h, w) = VOLUMES[2], IMAGES[1]
    origin, s = volume_geometry(shape)
    K = camera_for(h, w)
    poses = rc.poses_for(3)
    state = np_integrate(empty_state(shape), plane_depth(h, w, poses, K, at=origin[2] + 4 * s), poses, K, origin, s, 5.0 * s, 0.0)
    return state, origin, s


def check_extract_integrated(device):
    state, origin, s = integrated_state()
    want = np_extract(state[0], state[1], origin, s)
    assert want[2][0] > 300 and want[2][1] > 500
    check_mesh(extract_on(device, state, origin, s), want, "integrated volume")


SPHERE_CENTRE, SPHERE_RADIUS = 3.5, 2.75


def sphere_state(mu=1.0, s=0.25):
    k, j, i = np.meshgrid(*[np.arange(8, dtype=np.float64)] * 3, indexing="ij")
    sd = (np.sqrt((i - SPHERE_CENTRE) ** 2 + (j - SPHERE_CENTRE) ** 2 + (k - SPHERE_CENTRE) ** 2) - SPHERE_RADIUS) * s
    total = np.rint(np.clip(sd / mu, -1, 1) * 32768.0).astype(np.int32)
    return total, np.ones((8, 8, 8), np.int32), np.zeros(1, np.int64)


def check_extract_sphere(device):
    """A sphere of radius 2.75 voxels inside 8 x 8 x 8: EQUAL to the statement, a closed oriented 2-manifold (every directed
    edge once, its reverse once, V - E + F = 2), every normal pointing away from the centre"""
    s, origin = 0.25, (1.0, -2.0, 0.5)
    state = sphere_state(s=s)
    want = np_extract(state[0], state[1], origin, s)
    mesh = extract_on(device, state, origin, s)
    check_mesh(mesh, want, "sphere")
    v, t = mesh.vertices.cpu().numpy().astype(np.float64), mesh.triangles.cpu().numpy()
    directed = [(a, b) for tri in t.tolist() for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))]
    assert len(set(directed)) == len(directed) and all((b, a) in set(directed) for a, b in directed)
    assert len(np.unique(t)) == len(v)
    assert len(v) - len(directed) // 2 + len(t) == 2
    centre = np.array(origin) + s * SPHERE_CENTRE
    normals = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert np.all((normals * (v[t].mean(axis=1) - centre)).sum(axis=1) > 0)


def check_extract_zeros_and_weights(device):
    """Random small sums with many zeros (a zero is outside: the vertex sits exactly on that voxel), weights 0 .. 3 (cubes
    that touch a weight below min_weight emit nothing), min_weight 1 and 2; and with every weight >= 1 the field meets all
    16 cases in all six tetrahedra, which pins the table inside the library to the derived one"""
    rng = np.random.RandomState(0)
    total = rng.randint(-5, 6, (8, 8, 8)).astype(np.int32)
    weight = rng.randint(0, 4, (8, 8, 8)).astype(np.int32)
    origin, s = (0.0, 0.0, 0.0), 0.25
    for mw in (1, 2):
        want = np_extract(total, weight, origin, s, min_weight=mw)
        assert want[2][1] > 10
        check_mesh(extract_on(device, (total, weight, np.zeros(1, np.int64)), origin, s, mw), want, "min_weight %d" % mw)
    on_voxel = np.all(np.mod(np_extract(total, weight, origin, s)[0] / s, 1.0) == 0, axis=1)
    assert on_voxel.any() and not on_voxel.all()
    used = set()
    full = np.maximum(weight, 1)
    want = np_extract(total, full, origin, s, used=used)
    assert used == set(itertools.product(range(6), range(16)))
    check_mesh(extract_on(device, (total, full, np.zeros(1, np.int64)), origin, s), want, "every case")


def raw_extract(device, state, origin, s, max_v, max_t, guard=64, min_weight=1):
    """dcn_tsdf_extract into buffers with ``guard`` rows of a sentinel behind the capacities -> (vertices, triangles, counts,
    the two guard regions)"""
    from dcn_hip import _lib
    lib = _lib.get()
    nz, ny, nx = state[0].shape
    total, weight = torch.from_numpy(state[0].copy()).to(device), torch.from_numpy(state[1].copy()).to(device)
    v = torch.full((max_v + guard, 3), 12345.0, dtype=torch.float32, device=device)
    t = torch.full((max_t + guard, 3), 777, dtype=torch.int32, device=device)
    counts = torch.zeros(2, dtype=torch.int32, device=device)
    ws = torch.empty(lib.dcn_tsdf_extract_workspace(nx, ny, nz), dtype=torch.uint8, device=device)
    o = np.asarray(origin, np.float64)
    rc_ = lib.dcn_tsdf_extract(nx, ny, nz, _lib.host_ptr(o), float(s), _lib.ptr(total), _lib.ptr(weight), min_weight, max_v, max_t,
                               _lib.ptr(v), _lib.ptr(t), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr())
    assert rc_ == 0
    v, t = v.cpu().numpy(), t.cpu().numpy()
    return v[:max_v], t[:max_t], counts.cpu().numpy(), (v[max_v:], t[max_t:])


def check_extract_capacities(device):
    """Capacities below the true counts: the counts stay true, nothing is written behind a capacity, a triangle that names a
    vertex without a row is -1"""
    from dcn_hip import fusion
    import pytest
    s, origin = 0.25, (0.0, 0.0, 0.0)
    state = sphere_state(s=s)
    V, T = (int(c) for c in np_extract(state[0], state[1], origin, s)[2])
    for max_v, max_t in ((V, T), (V // 2, T), (V, T // 3), (V // 3 + 1, T // 2 + 1), (0, 0), (V + 5, T + 7)):
        want = np_extract(state[0], state[1], origin, s, max_vertices=max_v, max_triangles=max_t)
        gv, gt, gc, (guard_v, guard_t) = raw_extract(device, state, origin, s, max_v, max_t)
        check_mesh((gv[:min(V, max_v)], gt, gc), want, "capacities %d %d" % (max_v, max_t))
        assert np.all(guard_v == 12345.0) and np.all(guard_t == 777)
        if max_v < V and max_t:
            assert (gt[:min(T, max_t)] == -1).all(axis=1).any() and ((gt == -1).all(axis=1) | (gt >= 0).all(axis=1)).all()
    vol = volume_on(device, (8, 8, 8), origin, s, state=state)
    with pytest.raises(RuntimeError, match="do not fit"):
        fusion.extract_mesh(vol, max_vertices=V - 1)
    mesh, counts = fusion.extract_mesh(vol, max_vertices=V + 3, max_triangles=T + 3, trim=False)
    assert tuple(mesh.triangles.shape) == (T + 3, 3) and counts.cpu().tolist() == [V, T]


def check_extract_degenerate(device):
    zero = np.zeros(1, np.int64)
    for name, shape, total, weight in (("empty", (8, 8, 8), 0, 0), ("all inside", (5, 7, 9), -3, 2), ("all outside", (5, 7, 9), 3, 2),
                                       ("nx = 1", (1, 7, 9), None, 1), ("one voxel", (1, 1, 1), -1, 1)):
        nx, ny, nz = shape
        tot = np.full((nz, ny, nx), total, np.int32) if total is not None else \
            np.random.RandomState(1).randint(-3, 4, (nz, ny, nx)).astype(np.int32)
        wt = np.full((nz, ny, nx), weight, np.int32)
        want = np_extract(tot, wt, (0, 0, 0), 0.5)
        assert want[2].tolist() == [0, 0]
        gv, gt, gc, guards = raw_extract(device, (tot, wt, zero), (0, 0, 0), 0.5, 4, 6)
        assert gc.tolist() == [0, 0] and np.all(gt == -1) and np.all(guards[0] == 12345.0) and np.all(guards[1] == 777), name
        mesh = extract_on(device, (tot, wt, zero), (0, 0, 0), 0.5)
        assert mesh.num_vertices == 0 and mesh.num_triangles == 0


def check_plane_accuracy(device):
    """A plane at z = 0.75 m facing three cameras whose optical axes are perpendicular to it, images by render_depth (o = 0),
    s = 1 / 128, mu = 5 s.  The images read 750 mm exactly (rule 16(f): a triangle facing the camera shows its own depth, and
    trunc(0.75 * 1000) = 750), so d = 0.75 and the millimetre truncation of 16(g) costs at most 1 mm TOWARDS the camera; the
    projective distance d - z is the true distance.  Each frame's q is within 1/2 of diff / mu * 32768, so both ends of an
    edge carry the distance to within mu / 65536, and the interpolated crossing, a weighted mean of the two ends' errors over
    a unit gradient, to within the same; the float32 rounding of the vertex (6e-8 at 0.75) fits in the rest of the bound:
    every vertex whose two voxels were seen by every camera lies in [-1 mm - mu / 16384, +mu / 16384] of the plane along z."""
    from dcn_hip import fusion, render
    s = 1.0 / 128.0
    mu = 5.0 * s
    shape = (24, 20, 16)
    origin = (-12.0 * s, -10.0 * s, 0.75 - 7.3 * s)
    h, w = IMAGES[1]
    K = (128.0, 128.0, w / 2.0, h / 2.0)
    poses = np.stack([np.eye(4)] * 3)
    poses[1, :3, 3] = [0.02, -0.01, 0.0]
    poses[2, :3, 3] = [-0.015, 0.02, 0.03125]
    plane = render.Mesh(np.array([[-3, -3, 0.75], [3, -3, 0.75], [3, 3, 0.75], [-3, 3, 0.75]], np.float32), [[0, 1, 2], [0, 2, 3]],
                        device=device)
    depth, _ = render.render_depth(plane, poses, K, (h, w))
    d = depth.cpu().numpy().view(np.uint16)
    assert set(np.unique(d[0])) == {750} and set(np.unique(d[1])) == {750} and set(np.unique(d[2])) == {718}
    vol = fusion.TsdfVolume(origin, s, shape, device=device)
    vol.integrate(depth, poses, K, pixel_offset=0.0)
    state = np_integrate(empty_state(shape), d, poses, K, origin, s, mu, 0.0)
    check_state(vol, state, "plane")
    mesh = fusion.extract_mesh(vol)
    edges = []
    want = np_extract(state[0], state[1], origin, s, edges=edges)
    check_mesh(mesh, want, "plane mesh")
    kk, jj, ii, dd = edges[0]
    bits = np.array(DIR_BITS)[dd]
    seen = (state[1][kk, jj, ii] == 3) & (state[1][kk + (bits >> 2 & 1), jj + (bits >> 1 & 1), ii + (bits & 1)] == 3)
    assert seen.sum() > 500
    z = mesh.vertices.cpu().numpy().astype(np.float64)[seen, 2] - 0.75
    print("plane: %d vertices seen by every camera, z - 0.75 in [%.3e, %.3e], bound [%.3e, %.3e]"
          % (seen.sum(), z.min(), z.max(), -0.001 - mu / 16384, mu / 16384))
    assert z.min() >= -0.001 - mu / 16384 and z.max() <= mu / 16384


# ------------------------------------------------------------------------------------------------ 17c: the cases
def random_mesh(seed, n_points=300, n_triangles=400, lo=0.0, hi=1.0):
    rng = np.random.RandomState(seed)
    return rng.uniform(lo, hi, (n_points, 3)).astype(np.float32), rng.randint(0, n_points, (n_triangles, 3)).astype(np.int32)


def crop_on(device, verts, tris, transform, dims, **kw):
    from dcn_hip import fusion, render
    mesh = fusion._padded_mesh(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(device).reshape(-1, 3),
                               torch.from_numpy(np.ascontiguousarray(tris, np.int32)).to(device).reshape(-1, 3), None)
    return fusion.crop_to_box(mesh, transform, dims, **kw)


def check_crop_golden(name, device):
    """The reference's own lines on recorded points: the segment geometry fusion.box_segments computes and the surviving set"""
    from dcn_hip import fusion
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    seg = fusion.box_segments(z["transform"], z["dimensions"])
    assert np.array_equal(seg, z["segments"]) and np.array_equal(np_segments(z["transform"], z["dimensions"]), z["segments"])
    want = np_crop(z["points"], z["triangles"], z["transform"], z["dimensions"])
    survivors = z["triangles"][z["survives"].astype(bool)]
    assert 0 < len(survivors) < len(z["triangles"]) and int(want[2][1]) == len(survivors)
    mesh = crop_on(device, z["points"], z["triangles"], z["transform"], z["dimensions"])
    check_mesh(mesh, want, name)
    assert np.array_equal(mesh.vertices.cpu().numpy()[mesh.triangles.cpu().numpy()], z["points"][survivors])


def check_crop_cases(device):
    from dcn_hip import fusion
    box = np.eye(4)
    box[:3, 3] = 0.5
    dims = (0.5, 1.0, 0.25)                                    # x in [0.25, 0.75], y in [0, 1], z in [0.375, 0.625]: exact
    verts = np.array([[0.25, 0.0, 0.375], [0.75, 1.0, 0.625], [0.5, 0.5, 0.5],            # on both bounds of every axis, inside
                      [float(np.nextafter(np.float32(0.75), np.float32(1))), 0.5, 0.5],   # one float past a bound
                      [0.3, 0.2, 0.4], [0.7, 0.9, 0.6], [0.5, 0.5, 0.7], [9.0, 9.0, 9.0]], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 2], [-1, -1, -1], [4, 5, 6], [1, 0, 4], [2, 2, 2], [0, 1, 8]], np.int32)
    want = np_crop(verts, tris, box, dims)
    assert want[1].tolist() == [[0, 1, 2], [3, 4, 2], [1, 0, 3], [2, 2, 2]] and want[2].tolist() == [5, 4]
    check_mesh(crop_on(device, verts, tris, box, dims), want, "bounds, one point outside, -1 rows")
    rv, rt = random_mesh(3)
    rt[::7] = -1
    rotated = dict(translation=dict(x=0.45, y=0.5, z=0.55), quaternion=dict(w=0.9, x=0.1, y=-0.2, z=0.3))
    want = np_crop(rv, rt, fusion.box_transform(rotated), (0.7, 0.9, 0.8))
    assert 10 < want[2][1] < 300
    check_mesh(crop_on(device, rv, rt, rotated, dict(x=0.7, y=0.9, z=0.8)), want, "rotated box")
    R = fusion.box_transform(rotated)[:3, :3]
    assert np.allclose(R.dot(R.T), np.eye(3), atol=1e-15) and np.linalg.det(R) > 0.999
    rv, rt = random_mesh(4)
    for what, b, d in (("nothing", box, (1e-3, 1e-3, 1e-3)), ("everything", box, (4.0, 4.0, 4.0))):
        want = np_crop(rv, rt, b, d)
        assert int(want[2][1]) == (0 if what == "nothing" else len(rt))
        check_mesh(crop_on(device, rv, rt, b, d), want, what)
    check_mesh(crop_on(device, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), box, dims),
               np_crop(np.zeros((0, 3)), np.zeros((0, 3)), box, dims), "no mesh")


def check_crop_capacities(device):
    """As for the extraction: true counts, nothing behind a capacity (a raw call with guard rows), -1 for a triangle that
    names a vertex without a row"""
    from dcn_hip import _lib, fusion
    lib = _lib.get()
    rv, rt = random_mesh(5)
    box = np.eye(4)
    box[:3, 3] = 0.5
    dims = (0.9, 0.8, 0.9)
    V, T = (int(c) for c in np_crop(rv, rt, box, dims)[2])
    assert V > 50 and T > 50
    seg = np.ascontiguousarray(fusion.box_segments(box, dims))
    for max_v, max_t in ((V, T), (V // 2, T), (V, T // 2), (V // 3, T // 3), (0, 0)):
        want = np_crop(rv, rt, box, dims, max_vertices=max_v, max_triangles=max_t)
        v_in, t_in = torch.from_numpy(rv).to(device), torch.from_numpy(rt).to(device)
        v = torch.full((max_v + 32, 3), 12345.0, dtype=torch.float32, device=device)
        t = torch.full((max_t + 32, 3), 777, dtype=torch.int32, device=device)
        counts = torch.zeros(2, dtype=torch.int32, device=device)
        ws = torch.empty(lib.dcn_mesh_crop_workspace(len(rv), len(rt)), dtype=torch.uint8, device=device)
        assert lib.dcn_mesh_crop(len(rv), len(rt), _lib.ptr(v_in), _lib.ptr(t_in), _lib.host_ptr(seg), max_v, max_t, _lib.ptr(v),
                                 _lib.ptr(t), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr()) == 0
        v, t = v.cpu().numpy(), t.cpu().numpy()
        check_mesh((v[:min(V, max_v)], t[:max_t], counts.cpu().numpy()), want, "crop capacities %d %d" % (max_v, max_t))
        assert np.all(v[max_v:] == 12345.0) and np.all(t[max_t:] == 777)
        if 0 < max_v < V and max_t:
            assert (t[:min(T, max_t)] == -1).all(axis=1).any()


# ------------------------------------------------------------------------------------------------ PLY, arguments, the scene
def check_ply_round_trip(device, tmp_path):
    import pytest
    from dcn_hip import render
    state = sphere_state()
    mesh = extract_on(device, state, (0, 0, 0), 0.25)
    path = mesh.to_ply(str(tmp_path / "fusion_mesh.ply"))
    back = render.Mesh.from_ply(path, device=device)
    assert np.array_equal(back.vertices.cpu().numpy().view(np.uint32), mesh.vertices.cpu().numpy().view(np.uint32))
    assert np.array_equal(back.triangles.cpu().numpy(), mesh.triangles.cpu().numpy()) and back.num_triangles > 100
    empty = render.Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), device=device)
    assert render.Mesh.from_ply(empty.to_ply(str(tmp_path / "fusion_mesh_foreground.ply")), device=device).num_vertices == 0
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n") + 11]
    assert b"format binary_little_endian 1.0" in head and b"property list uchar int vertex_indices" in head
    assert len(raw) == len(head) + 12 * mesh.num_vertices + 13 * mesh.num_triangles
    # the header is one the reader's own checks accept: cut short and retyped, the reader says what is wrong with it
    cut = str(tmp_path / "cut.ply")
    open(cut, "wb").write(raw[:len(raw) - 5])
    with pytest.raises(render.PlyError, match="ends inside the face element"):
        render.read_ply(cut)
    big = str(tmp_path / "big.ply")
    open(big, "wb").write(raw.replace(b"binary_little_endian", b"binary_big_endian", 1))
    with pytest.raises(render.PlyError, match="binary_big_endian"):
        render.read_ply(big)
    padded = str(tmp_path / "padded.ply")                     # rows of -1 (an untrimmed mesh) are left out
    render.write_ply(padded, mesh.vertices.cpu().numpy(), np.concatenate([mesh.triangles.cpu().numpy(), -np.ones((3, 3), np.int32)]))
    assert np.array_equal(render.read_ply(padded)[1], mesh.triangles.cpu().numpy())


def check_argument_errors(device):
    import pytest
    from dcn_hip import _lib, fusion
    lib = _lib.get()
    for shape in ((0, 8, 8), (8, 1025, 8), (8, 8), (8, 8, -1)):
        with pytest.raises(ValueError):
            fusion.TsdfVolume((0, 0, 0), 0.1, shape, device=device)
    for s, mu in ((0.0, None), (-1.0, None), (0.1, 0.0), (0.1, -2.0), (float("nan"), None)):
        with pytest.raises(ValueError):
            fusion.TsdfVolume((0, 0, 0), s, (4, 4, 4), mu, device=device)
    vol = fusion.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), device=device)
    assert vol.trunc_margin == 0.5 and not vol.sum.any() and not vol.weight.any() and not vol.status.any()
    d = torch.zeros((2, 6, 8), dtype=torch.int16, device=device)
    p = np.stack([np.eye(4)] * 2)
    K = camera_for(6, 8)
    for bad_d, bad_p in ((d.float(), p), (d.to(torch.int32), p), (d, p[:1]), (d[0, 0], p), (d, np.eye(3))):
        with pytest.raises(ValueError):
            vol.integrate(bad_d, bad_p, K)
    with pytest.raises(ValueError):
        vol.integrate(d, p, K, frames_per_launch=0)
    with pytest.raises(ValueError):
        vol.integrate(d, p, K, max_depth_mm=70000)
    with pytest.raises(ValueError):
        fusion.TsdfVolume.from_tensors(vol.sum, vol.weight.float(), (0, 0, 0), 0.1)
    with pytest.raises(ValueError):
        fusion.TsdfVolume.from_tensors(vol.sum, vol.weight[:2], (0, 0, 0), 0.1)
    with pytest.raises(ValueError):
        fusion.extract_mesh(vol, min_weight=0)
    for kw in (dict(max_vertices=-1), dict(max_triangles=-1)):
        with pytest.raises(ValueError):
            fusion.extract_mesh(vol, **kw)
        with pytest.raises(ValueError):
            fusion.crop_to_box(fusion.extract_mesh(vol), np.eye(4), (1, 1, 1), **kw)
    with pytest.raises(ValueError):
        fusion.crop_to_box(fusion.extract_mesh(vol), np.eye(4), (1, 0, 1))
    if device != "cpu":
        with pytest.raises(ValueError):
            vol.integrate(d.cpu(), p, K)
        with pytest.raises(ValueError):
            vol.integrate(d, torch.from_numpy(p), K)
        with pytest.raises(RuntimeError):
            fusion.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    # the C ABI refuses what the Python layer never sends
    o = np.zeros(3)
    one = torch.zeros(8, dtype=torch.int32, device=device)
    args = lambda nx, s, mu: (nx, 2, 2, _lib.host_ptr(o), s, mu, 2, 6, 8, _lib.ptr(d), _lib.ptr(torch.from_numpy(p).float().to(device)),
                              1.0, 1.0, 1.0, 1.0, 0.5, 6000, -1, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), _lib.stream_ptr())
    assert lib.dcn_tsdf_integrate(*args(2, 0.1, 0.5)) == 0
    for bad in (args(0, 0.1, 0.5), args(1025, 0.1, 0.5), args(2, 0.0, 0.5), args(2, 0.1, 0.0), args(2, 0.1, float("nan"))):
        assert lib.dcn_tsdf_integrate(*bad) == -1
    assert lib.dcn_tsdf_extract_workspace(0, 4, 4) == 0 and lib.dcn_tsdf_extract_workspace(4, 4, 1025) == 0
    assert lib.dcn_mesh_crop_workspace(-1, 4) == 0


SCENE_SHAPE = (48, 48, 48)
SCENE_S = 1.0 / 64.0
SCENE_ORIGIN = (-0.25, -0.25, 0.625)                        # 0.75 m cube around the box (top 0.875 m) and the table (1.25 m)
SCENE_CROP = dict(transform=dict(translation=dict(x=0.125, y=0.125, z=1.0), quaternion=dict(w=1, x=0, y=0, z=0)),
                  dimensions=dict(x=0.5, y=0.5, z=0.4375))  # down to 1.21875 m: above the table's surface


def fuse_box_scene(images, K, poses):
    """render_common's box on a table, as rendered -> (full, foreground) meshes, padded, nothing read back"""
    from dcn_hip import fusion
    spec = dict(origin=SCENE_ORIGIN, voxel_size=SCENE_S, shape=SCENE_SHAPE)
    return fusion.fuse_scene(images.depth, poses, K, spec, SCENE_CROP, pixel_offset=0.0)


def rerender(fused, K, poses, h=48, w=64):
    from dcn_hip import render
    full, fg = fused
    return render.render_scene(fg, full, poses, K, (h, w))


def check_fused_scene(fused, again):
    """Plumbing, not accuracy: both meshes hold something, the foreground is part of the full mesh, and its re-rendered mask is
    neither empty nor the whole image"""
    full, fg = fused
    cf, cg = full.counts.cpu().tolist(), fg.counts.cpu().tolist()
    assert 0 < cg[0] < cf[0] <= full.vertices.shape[0] and 0 < cg[1] < cf[1] <= full.triangles.shape[0], (cf, cg)
    t = full.triangles.cpu().numpy()
    assert np.all(t[:cf[1]] >= 0) and np.all(t[cf[1]:] == -1)
    mask = again.mask.cpu().numpy()
    assert mask.shape[0] == 4 and all(0 < int(m.sum()) < m.size for m in mask)
    assert np.all(again.depth.cpu().numpy().view(np.uint16)[mask == 1] > 0)
