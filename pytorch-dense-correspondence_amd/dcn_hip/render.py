"""Host side of the render kernels (csrc/render_kernels.hip, include/dcn_hip.h section 16): depth images and foreground masks
of a scene's meshes from its logged camera poses -- what the reference's data collection produces with director / VTK / OpenGL
(modules/dense_correspondence_manipulation/change_detection/change_detection.py) and what ``frames.FrameStore`` consumes.

    full, fg = Mesh.from_ply("fusion_mesh.ply"), Mesh.from_ply("fusion_mesh_foreground.ply")
    im = render_scene(fg, full, poses, K, (480, 640))            # device tensors, no read-back
    store = frames.FrameStore.from_tensors(rgb, im.depth, im.mask, poses, [0, F], [0], K)
    write_scene_images(processed_dir, frame_ids, im)             # the reference's four files per frame, one copy

The rasteriser's arithmetic is defined in the header (rules (a)-(h)); it is not OpenGL's: a triangle that reaches in front of
``z_near`` is dropped whole, not clipped, and counted in ``status``.  The meshes come from files or from ``dcn_hip.fusion``
(TSDF fusion, surface extraction, box crop); the director applications of the reference are not provided."""
import collections
import os

import numpy as np
import torch

from . import _lib

DEFAULT_Z_NEAR = 0.05
DEFAULT_MASK_THRESHOLD = 10        # ChangeDetection's threshold, millimetres

SceneImages = collections.namedtuple("SceneImages", "depth depth_cropped mask visible_mask status status_cropped")
SceneImages.__doc__ = """depth int16 [F, H, W]: the full mesh in millimetres (uint16 bits, the store's convention; 0: no surface);
depth_cropped: the foreground mesh; mask uint8 0/1 and visible_mask uint8 0/255 [F, H, W]: where the foreground mesh is seen;
status, status_cropped int32 [F, 2]: triangles dropped per frame (in front of z_near, outside the guard band)."""


class PlyError(ValueError):
    pass


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(f, path):
    if f.readline().strip() != b"ply":
        raise PlyError("%s is not a PLY file" % path)
    fmt, elements = None, []
    while True:
        raw = f.readline()
        if not raw:
            raise PlyError("%s: the PLY header does not end" % path)
        line = raw.decode("ascii", "replace").split()
        if not line or line[0] in ("comment", "obj_info"):
            continue
        if line[0] == "end_header":
            break
        if line[0] == "format":
            fmt = line[1]
        elif line[0] == "element":
            elements.append((line[1], int(line[2]), []))
        elif line[0] == "property" and elements:
            props = elements[-1][2]
            if line[1] == "list":
                props.append((line[4], ("list", line[2], line[3])))
            else:
                props.append((line[2], line[1]))
        else:
            raise PlyError("%s: cannot read the header line %r" % (path, raw))
    if fmt not in ("ascii", "binary_little_endian"):
        raise PlyError("%s: PLY format %r is not supported (ascii and binary_little_endian are)" % (path, fmt))
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise PlyError("%s: expected the elements vertex and face, in this order, got %s" % (path, [e[0] for e in elements]))
    for name, _, props in elements:
        for pname, kind in props:
            types = kind[1:] if isinstance(kind, tuple) else (kind,)
            if any(t not in _PLY_TYPES for t in types):
                raise PlyError("%s: unknown type in property %s of element %s" % (path, pname, name))
    (_, nv, vprops), (_, nf, fprops) = elements
    if any(isinstance(k, tuple) for _, k in vprops) or not all(n in [p[0] for p in vprops] for n in "xyz"):
        raise PlyError("%s: the vertex element must have scalar properties, x, y and z among them" % path)
    lists = [p for p in fprops if isinstance(p[1], tuple)]
    if len(lists) != 1 or lists[0][0] not in ("vertex_indices", "vertex_index"):
        raise PlyError("%s: the face element must have exactly one list property, vertex_indices" % path)
    return fmt, nv, vprops, nf, fprops


def _triangles_only(counts, path):
    if counts.size and not np.all(counts == 3):
        bad = int(np.flatnonzero(counts != 3)[0])
        raise PlyError("%s: face %d has %d vertices -- triangles only (triangulate the mesh first)"
                       % (path, bad, int(counts[bad])))


def read_ply(path):
    """-> (vertices float32 [V, 3], triangles int32 [T, 3]) of an ASCII or binary little-endian PLY file whose faces are all
    triangles; other vertex and face properties are skipped.  PlyError (a ValueError) on anything else."""
    with open(path, "rb") as f:
        fmt, nv, vprops, nf, fprops = _ply_header(f, path)
        if fmt == "ascii":
            rows = f.read().decode("ascii", "replace").split("\n")
            rows = [r.split() for r in rows if r.strip()]
            if len(rows) < nv + nf:
                raise PlyError("%s: %d data lines, the header promises %d" % (path, len(rows), nv + nf))
            cols = [p[0] for p in vprops]
            vr = rows[:nv]
            if any(len(r) != len(cols) for r in vr):
                raise PlyError("%s: a vertex line does not have %d values" % (path, len(cols)))
            table = np.array(vr, dtype=np.float64).reshape(nv, len(cols))
            vertices = table[:, [cols.index(n) for n in "xyz"]].astype(np.float32)
            tris = np.zeros((nf, 3), np.int64)
            counts = np.zeros(nf, np.int64)
            for i, r in enumerate(rows[nv:nv + nf]):
                at = 0
                for _, kind in fprops:
                    if isinstance(kind, tuple):
                        counts[i] = int(r[at])
                        if counts[i] == 3:
                            tris[i] = [int(x) for x in r[at + 1:at + 4]]
                        at += 1 + int(counts[i])
                    else:
                        at += 1
            _triangles_only(counts, path)
        else:
            vdt = np.dtype([(n, "<" + _PLY_TYPES[t]) for n, t in vprops])
            vt = np.frombuffer(f.read(vdt.itemsize * nv), dtype=vdt)
            if vt.size != nv:
                raise PlyError("%s: the file ends inside the vertex element" % path)
            vertices = np.stack([vt[n].astype(np.float32) for n in "xyz"], axis=1) if nv else np.zeros((0, 3), np.float32)
            fields = []
            for n, kind in fprops:
                if isinstance(kind, tuple):
                    fields += [("_count", "<" + _PLY_TYPES[kind[1]]), ("_index", "<" + _PLY_TYPES[kind[2]], (3,))]
                else:
                    fields.append((n, "<" + _PLY_TYPES[kind]))
            fdt = np.dtype(fields)
            blob = f.read(fdt.itemsize * nf)
            ft = np.frombuffer(blob[:len(blob) - len(blob) % fdt.itemsize], dtype=fdt)
            # records are read as triangles: the first face that is none is found at its own count (the records before it
            # are whole), whatever it does to those behind it
            _triangles_only(ft["_count"].astype(np.int64), path)
            if ft.size != nf:
                raise PlyError("%s: the file ends inside the face element" % path)
            tris = ft["_index"].astype(np.int64).reshape(nf, 3)
    if tris.size and (tris.min() < 0 or tris.max() >= nv):
        raise PlyError("%s: a face names a vertex outside 0 .. %d" % (path, nv - 1))
    return np.ascontiguousarray(vertices), np.ascontiguousarray(tris.astype(np.int32))


def write_ply(path, vertices, triangles):
    """Writes a binary little-endian PLY file read_ply reads back as it is: float x, y, z and ``uchar int`` face lists.
    Triangle rows that hold a negative index (the padding of dcn_hip.fusion's untrimmed meshes) are left out.  -> path"""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f4").reshape(-1, 3))
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    t = t[(t >= 0).all(axis=1)]
    if t.size and t.max() >= len(v):
        raise ValueError("a triangle names a vertex outside 0 .. %d" % (len(v) - 1))
    faces = np.zeros(len(t), dtype=[("_count", "u1"), ("_index", "<i4", (3,))])
    faces["_count"] = 3
    faces["_index"] = t
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x", "property float y",
            "property float z", "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())
    return path


class Mesh(object):
    """vertices float32 [V, 3] in the world frame and triangles int32 [T, 3] on one device.  Built from host arrays or tensors
    (checked: shapes, every index inside [0, V)); ``device`` defaults to the current GPU (the CPU under the test-only
    host-emulation library)."""

    def __init__(self, vertices, triangles, device=None):
        v = torch.as_tensor(np.asarray(vertices) if not torch.is_tensor(vertices) else vertices)
        t = torch.as_tensor(np.asarray(triangles) if not torch.is_tensor(triangles) else triangles)
        v = v.reshape(0, 3) if v.numel() == 0 else v
        t = t.reshape(0, 3) if t.numel() == 0 else t
        if v.dim() != 2 or v.shape[1] != 3 or not (v.is_floating_point()):
            raise ValueError("vertices must be floating point [V, 3], got %s %s" % (v.dtype, tuple(v.shape)))
        if t.dim() != 2 or t.shape[1] != 3 or t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError("triangles must be integer [T, 3], got %s %s" % (t.dtype, tuple(t.shape)))
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= v.shape[0]):          # (once, where the mesh is built)
            raise ValueError("a triangle names a vertex outside 0 .. %d" % (v.shape[0] - 1))
        if device is None:
            device = "cpu" if _lib.is_hostemu() else torch.device("cuda", torch.cuda.current_device())
        self.vertices = v.to(device=device, dtype=torch.float32).contiguous()
        self.triangles = t.to(device=device, dtype=torch.int32).contiguous()
        _lib.require_device(self.vertices, self.triangles)

    @classmethod
    def from_ply(cls, path, device=None):
        return cls(*read_ply(path), device=device)

    def to_ply(self, path):
        """One copy to the host and ``write_ply``: the reference's fusion_mesh.ply / fusion_mesh_foreground.ply.  -> path"""
        return write_ply(path, self.vertices.cpu().numpy(), self.triangles.cpu().numpy())

    @property
    def device(self):
        return self.vertices.device

    @property
    def num_vertices(self):
        return int(self.vertices.shape[0])

    @property
    def num_triangles(self):
        return int(self.triangles.shape[0])


def _pinhole(K):
    k = np.asarray(K, dtype=np.float64)
    if k.shape == (3, 3):
        return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if k.shape == (4,):
        return tuple(float(x) for x in k)
    raise ValueError("K must be (fx, fy, cx, cy) or a 3 x 3 camera matrix")


def _poses(poses, dev):
    p = poses if torch.is_tensor(poses) else torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64)))
    if p.dim() == 2:
        p = p.unsqueeze(0)
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or p.shape[0] < 1:
        raise ValueError("poses must be [F, 4, 4] camera-to-world, got %s" % (tuple(p.shape),))
    return p.to(device=dev, dtype=torch.float32).contiguous()


def render_depth(mesh, poses, K, shape, z_near=DEFAULT_Z_NEAR, large_threshold=None):
    """The mesh from every pose [F, 4, 4] (camera-to-world, host or device) through the pinhole K = (fx, fy, cx, cy) or 3 x 3,
    at shape = (H, W).  -> (depth int16 [F, H, W] millimetres with uint16 bits, 0: no surface; status int32 [F, 2]: triangles
    dropped whole because a vertex is in front of z_near / a projected vertex is outside the guard band).  No host
    synchronisation.  ``large_threshold``: bounding-box pixels above which a triangle takes the tiled path (None: the library's
    default); the image does not depend on it."""
    lib = _lib.get()
    h, w = int(shape[0]), int(shape[1])
    fx, fy, cx, cy = _pinhole(K)
    dev = mesh.device
    p = _poses(poses, dev)
    _lib.require_device(mesh.vertices, mesh.triangles, p)
    f, v, t = int(p.shape[0]), mesh.num_vertices, mesh.num_triangles
    nbytes = lib.dcn_render_depth_workspace(v, t, f, h, w)
    if nbytes == 0:
        raise ValueError("render_depth: unsupported shape (H, W in 1 .. 16384)")
    depth = torch.empty((f, h, w), dtype=torch.int16, device=dev)
    status = torch.empty((f, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.dcn_render_depth(v, t, f, h, w, _lib.ptr(mesh.vertices), _lib.ptr(mesh.triangles), _lib.ptr(p), fx, fy, cx, cy,
                              float(z_near), -1 if large_threshold is None else int(large_threshold), _lib.ptr(depth),
                              _lib.ptr(status), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_render_depth")
    return depth, status


def foreground_masks(depth_f, depth_b=None, threshold=DEFAULT_MASK_THRESHOLD):
    """16-bit depth images [..., H, W] -> (mask uint8 0/1, visible_mask uint8 0/255, depth_change int16 = mask * depth_f).
    With ``depth_b`` (the background scene from the same poses) the reference's change detection: zeros count as out of
    range, mask = (depth_b - depth_f) > threshold in int32.  Without it the crop strategy ChangeDetection.run uses:
    mask = depth_f > 0."""
    lib = _lib.get()
    if depth_f.element_size() != 2 or depth_f.is_floating_point():
        raise ValueError("depth_f must be a 16-bit integer tensor")
    if depth_b is not None and (depth_b.shape != depth_f.shape or depth_b.element_size() != 2 or depth_b.is_floating_point()):
        raise ValueError("depth_b must be a 16-bit integer tensor of depth_f's shape")
    if int(threshold) < 0:
        raise ValueError("threshold must be >= 0")
    f = depth_f.contiguous()
    b = None if depth_b is None else depth_b.contiguous()
    _lib.require_device(f, b)
    n = int(f.numel())
    mask = torch.empty(f.shape, dtype=torch.uint8, device=f.device)
    visible = torch.empty(f.shape, dtype=torch.uint8, device=f.device)
    change = torch.empty(f.shape, dtype=torch.int16, device=f.device)
    if n:
        rc = lib.dcn_render_masks(n, _lib.ptr(f), _lib.ptr(b), int(threshold), _lib.ptr(mask), _lib.ptr(visible),
                                  _lib.ptr(change), _lib.stream_ptr())
        _lib.check(rc, "dcn_render_masks")
    return mask, visible, change


def render_scene(foreground_mesh, full_mesh, poses, K, shape, z_near=DEFAULT_Z_NEAR):
    """What ChangeDetection.run and render_depth_images leave per frame: the full mesh's depth image, the cropped
    (foreground) mesh's depth image and, by the crop strategy, the object mask and its visible copy.  -> SceneImages of device
    tensors; no host synchronisation and no read-back."""
    depth, status = render_depth(full_mesh, poses, K, shape, z_near)
    cropped, status_c = render_depth(foreground_mesh, poses, K, shape, z_near)
    mask, visible, _ = foreground_masks(cropped)
    return SceneImages(depth, cropped, mask, visible, status, status_c)


def write_scene_images(directory, indices, images):
    """Copies ``images`` (a SceneImages) to the host once and writes, for frame j with image index ``indices[j]``, the
    reference's files: rendered_images/%06d_depth.png and %06d_depth_cropped.png (16-bit PNG, millimetres),
    image_masks/%06d_mask.png (0/1) and %06d_visible_mask.png (0/255).  -> the list of paths."""
    from PIL import Image
    indices = [int(i) for i in indices]
    if len(indices) != int(images.depth.shape[0]):
        raise ValueError("%d indices for %d frames" % (len(indices), int(images.depth.shape[0])))
    host = {"depth": images.depth.cpu().numpy().view(np.uint16), "depth_cropped": images.depth_cropped.cpu().numpy().view(np.uint16),
            "mask": images.mask.cpu().numpy(), "visible_mask": images.visible_mask.cpu().numpy()}
    folder = {"depth": "rendered_images", "depth_cropped": "rendered_images", "mask": "image_masks",
              "visible_mask": "image_masks"}
    for d in set(folder.values()):
        os.makedirs(os.path.join(directory, d), exist_ok=True)
    paths = []
    for j, idx in enumerate(indices):
        for kind in ("depth", "depth_cropped", "mask", "visible_mask"):
            path = os.path.join(directory, folder[kind], "%06d_%s.png" % (idx, kind))
            Image.fromarray(np.ascontiguousarray(host[kind][j])).save(path)
            paths.append(path)
    return paths
