"""Host side of the fusion kernels (csrc/fusion_kernels.hip, include/dcn_hip.h section 17): from a scene's logged sensor depth
images and camera poses to the two meshes ``render.render_scene`` draws -- what the reference's data processing gets from a
CUDA tsdf-fusion binary, marching cubes (doc/data_processing_single_scene.md:42-57) and director's cropToBox
(fusion_reconstruction.py:246-258, 316-332).

    vol = TsdfVolume(origin=(0.3, -0.4, -0.1), voxel_size=1 / 256., shape=(256, 256, 256))
    vol.integrate(depth, poses, K)                                 # int16 / uint16 [F, H, W] millimetres; calls accumulate
    full = extract_mesh(vol)                                       # render.Mesh, fusion_mesh.ply with full.to_ply(path)
    fg = crop_to_box(full, crop_box["transform"], crop_box["dimensions"])
    full, fg = fuse_scene(depth, poses, K, dict(origin=..., voxel_size=..., shape=...), crop_box)   # the same, no read-back

The arithmetic is defined in the header (17a-17c): integers and single correctly rounded float64 operations, the same bit for
bit from run to run.  The surface is extracted by marching tetrahedra, not marching cubes: about twice the triangles.  Colour
fusion is ``dcn_hip.paint``'s; decimation and the director applications are not provided."""
import numpy as np
import torch

from . import _lib
from .render import Mesh, _pinhole, _poses

DEFAULT_MAX_DEPTH_MM = 6000        # tsdf-fusion's 6 m
DEFAULT_PIXEL_OFFSET = 0.5         # sensor images: integer coordinates are pixel centres; 0.0 for images of render_depth
MAX_DIM = 1024


def _device(device):
    if device is not None:
        return torch.device(device)
    return torch.device("cpu") if _lib.is_hostemu() else torch.device("cuda", torch.cuda.current_device())


def _host_doubles(values, n, what):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if a.size != n or not np.all(np.isfinite(a)):
        raise ValueError("%s must be %d finite numbers" % (what, n))
    return a


def default_capacities(shape):
    """(max_vertices, max_triangles) that ``extract_mesh`` allocates when none are given: 12 and 24 per voxel of the volume's
    three faces -- a surface that crosses the volume a few times; a marching-tetrahedra sheet has 4-6 triangles per cube it
    passes and half as many vertices.  Never more than the volume can emit (7 vertices per voxel, 12 triangles per cube)."""
    nx, ny, nz = shape
    faces = nx * ny + ny * nz + nz * nx
    n = nx * ny * nz
    return int(min(12 * faces, 7 * n, 2 ** 31 - 1)), int(min(24 * faces, 12 * n, 2 ** 31 - 1))


class TsdfVolume(object):
    """A truncated signed distance volume on one device: ``shape`` = (nx, ny, nz) voxels (1 .. 1024 each) of ``voxel_size``
    metres, voxel (0, 0, 0) centred at ``origin``; ``trunc_margin`` defaults to five voxels.  State: ``sum`` and ``weight``
    int32 [nz, ny, nx] (the signed distance is sum / weight / 32768 * trunc_margin) and ``status`` int32 [1], the frames that
    saturated voxels (weight 65535) did not take."""

    def __init__(self, origin, voxel_size, shape, trunc_margin=None, device=None):
        self.origin = _host_doubles(origin, 3, "origin")
        self.shape = tuple(int(d) for d in shape)
        if len(self.shape) != 3 or not all(1 <= d <= MAX_DIM for d in self.shape):
            raise ValueError("shape must be (nx, ny, nz), each in 1 .. %d, got %s" % (MAX_DIM, (shape,)))
        self.voxel_size = float(voxel_size)
        self.trunc_margin = 5.0 * self.voxel_size if trunc_margin is None else float(trunc_margin)
        if not (self.voxel_size > 0.0 and np.isfinite(self.voxel_size)):
            raise ValueError("voxel_size must be > 0")
        if not (self.trunc_margin > 0.0 and np.isfinite(self.trunc_margin)):
            raise ValueError("trunc_margin must be > 0")
        dev = _device(device)
        nx, ny, nz = self.shape
        self.sum = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.require_device(self.sum)
        lib = _lib.get()
        for t in (self.sum, self.weight, self.status):                       # (zero-filled by a kernel)
            _lib.check(lib.dcn_fill_bytes(_lib.ptr(t), 0, t.numel() * 4, _lib.stream_ptr()), "dcn_fill_bytes")

    @classmethod
    def from_tensors(cls, sum, weight, origin, voxel_size, trunc_margin=None, status=None):
        """A volume that continues from a saved state: sum, weight int32 [nz, ny, nx] on one device (copied)"""
        for name, t in (("sum", sum), ("weight", weight)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 3:
                raise ValueError("%s must be an int32 tensor [nz, ny, nx]" % name)
        if sum.shape != weight.shape or sum.device != weight.device:
            raise ValueError("sum and weight must have one shape and one device")
        nz, ny, nx = (int(d) for d in sum.shape)
        vol = cls(origin, voxel_size, (nx, ny, nz), trunc_margin, device=sum.device)
        vol.sum.copy_(sum)
        vol.weight.copy_(weight)
        if status is not None:
            vol.status.copy_(status.reshape(1))
        return vol

    @property
    def device(self):
        return self.sum.device

    def integrate(self, depth, poses, K, pixel_offset=DEFAULT_PIXEL_OFFSET, max_depth_mm=DEFAULT_MAX_DEPTH_MM,
                  frames_per_launch=None):
        """Adds the frames, in their order: depth 16-bit integer [F, H, W] millimetres on the volume's device (the store's
        int16 tensors as they are), poses [F, 4, 4] camera-to-world, K = (fx, fy, cx, cy) or 3 x 3.  ``pixel_offset``: 0.5 for
        sensor images, 0.0 for images made by ``render.render_depth``.  ``frames_per_launch`` (None: the library's default)
        does not change the result.  No host synchronisation.  -> self"""
        lib = _lib.get()
        if not torch.is_tensor(depth) or depth.is_floating_point() or depth.element_size() != 2:
            raise ValueError("depth must be a 16-bit integer tensor")
        if depth.dim() == 2:
            depth = depth.unsqueeze(0)
        if depth.dim() != 3 or depth.shape[0] < 1:
            raise ValueError("depth must be [F, H, W], got %s" % (tuple(depth.shape),))
        if depth.device != self.device:
            raise ValueError("depth is on %s, the volume on %s" % (depth.device, self.device))
        if torch.is_tensor(poses) and poses.device != self.device:
            raise ValueError("poses are on %s, the volume on %s" % (poses.device, self.device))
        p = _poses(poses, self.device)
        if p.shape[0] != depth.shape[0]:
            raise ValueError("%d poses for %d depth images" % (p.shape[0], depth.shape[0]))
        if not 0 <= int(max_depth_mm) <= 65535:
            raise ValueError("max_depth_mm must be in 0 .. 65535")
        chunk = -1 if frames_per_launch is None else int(frames_per_launch)
        if chunk == 0 or chunk > 64:
            raise ValueError("frames_per_launch must be in 1 .. 64")
        fx, fy, cx, cy = _pinhole(K)
        d = depth.contiguous()
        _lib.require_device(d, p, self.sum)
        f, h, w = (int(x) for x in d.shape)
        nx, ny, nz = self.shape
        rc = lib.dcn_tsdf_integrate(nx, ny, nz, _lib.host_ptr(self.origin), self.voxel_size, self.trunc_margin, f, h, w,
                                    _lib.ptr(d), _lib.ptr(p), fx, fy, cx, cy, float(pixel_offset), int(max_depth_mm), chunk,
                                    _lib.ptr(self.sum), _lib.ptr(self.weight), _lib.ptr(self.status), _lib.stream_ptr())
        _lib.check(rc, "dcn_tsdf_integrate")
        return self

    def tsdf(self):
        """The signed distance in metres, float32 [nz, ny, nx]; NaN where no frame reached the voxel"""
        w = self.weight.to(torch.float64)
        d = self.sum.to(torch.float64) / w / 32768.0 * self.trunc_margin
        return torch.where(self.weight > 0, d, torch.full_like(d, float("nan"))).to(torch.float32)


def _padded_mesh(vertices, triangles, counts):
    """A Mesh around device buffers as the kernels left them (rows of -1 draw nothing): no index check, which would read back"""
    m = Mesh.__new__(Mesh)
    m.vertices, m.triangles, m.counts = vertices, triangles, counts
    return m


def _capacity(value, default, what):
    if value is None:
        return int(default)
    if int(value) < 0 or int(value) > 2 ** 31 - 1:
        raise ValueError("%s must be in 0 .. 2^31 - 1" % what)
    return int(value)


def _finish(vertices, triangles, counts, trim, what):
    if not trim:
        return _padded_mesh(vertices, triangles, counts), counts
    nv, nt = (int(c) for c in counts.cpu())                                  # (the one read-back)
    if nv > vertices.shape[0] or nt > triangles.shape[0]:
        raise RuntimeError("%s: %d vertices and %d triangles do not fit the capacities %d and %d"
                           % (what, nv, nt, vertices.shape[0], triangles.shape[0]))
    return _padded_mesh(vertices[:nv].contiguous(), triangles[:nt].contiguous(), None)


def extract_mesh(volume, max_vertices=None, max_triangles=None, min_weight=1, trim=True):
    """The zero level of the volume as a ``render.Mesh`` (marching tetrahedra; cubes with a corner of weight < min_weight emit
    nothing).  ``trim=True`` reads the two counts once, slices, and raises if a capacity was exceeded.  ``trim=False`` reads
    nothing: -> (mesh padded to the capacities -- unused triangle rows are -1, which render_depth skips --, counts int32 [2]
    on the device, the true numbers).  Capacities default to ``default_capacities(volume.shape)``."""
    lib = _lib.get()
    if int(min_weight) < 1:
        raise ValueError("min_weight must be >= 1")
    dv, dt = default_capacities(volume.shape)
    max_v, max_t = _capacity(max_vertices, dv, "max_vertices"), _capacity(max_triangles, dt, "max_triangles")
    dev = volume.device
    nx, ny, nz = volume.shape
    vertices = torch.zeros((max_v, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((max_t, 3), dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.dcn_tsdf_extract_workspace(nx, ny, nz), dtype=torch.uint8, device=dev)
    _lib.require_device(volume.sum, volume.weight)
    rc = lib.dcn_tsdf_extract(nx, ny, nz, _lib.host_ptr(volume.origin), volume.voxel_size, _lib.ptr(volume.sum),
                              _lib.ptr(volume.weight), int(min_weight), max_v, max_t, _lib.ptr(vertices), _lib.ptr(triangles),
                              _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_tsdf_extract")
    return _finish(vertices, triangles, counts, trim, "extract_mesh")


def _xyz(v, keys, what):
    if isinstance(v, dict):
        v = [v[k] for k in keys]
    return _host_doubles(v, len(keys), what)


def box_transform(transform):
    """-> float64 [4, 4] of a 4 x 4 matrix or the reference's pose dict: ``translation`` (x, y, z) and ``quaternion``
    (w, x, y, z), each a dict or a list, as crop_box.transform of config/stations/*/change_detection.yaml is written"""
    if isinstance(transform, dict):
        t = _xyz(transform["translation"], "xyz", "translation")
        w, x, y, z = _xyz(transform["quaternion"], "wxyz", "quaternion")
        n = np.sqrt(w * w + x * x + y * y + z * z)
        if not n > 0:
            raise ValueError("the quaternion is zero")
        w, x, y, z = w / n, x / n, y / n, z / n
        T = np.eye(4)
        T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        T[:3, 3] = t
        return T
    return _host_doubles(transform, 16, "transform").reshape(4, 4)


def box_segments(transform, dimensions):
    """cropToBox / cropToLineSegment (director_utils.py:151-178) in numpy float64, in the written order: per axis of the box
    frame point1 [3], axis' [3], length' -> float64 [3, 7]"""
    T = box_transform(transform)
    dims = _xyz(dimensions, "xyz", "dimensions")
    origin = np.array(T[:3, 3])
    out = np.zeros((3, 7), np.float64)
    for a in range(3):
        crop_axis = np.array(T[:3, a]) * (dims[a] / 2.0)
        point1, point2 = origin - crop_axis, origin + crop_axis
        line = np.array(point2) - np.array(point1)
        length = np.linalg.norm(line)
        with np.errstate(all="ignore"):                                      # (a zero length: refused below)
            out[a, :3], out[a, 3:6], out[a, 6] = point1, line / length, length
    if not np.all(np.isfinite(out)):
        raise ValueError("the crop box has an axis of no length")
    return out


def crop_to_box(mesh, transform, dimensions, trim=True, max_vertices=None, max_triangles=None):
    """The triangles of ``mesh`` whose three points all lie in the box (bounds included) -- director's cropToBox, which makes
    fusion_mesh_foreground.ply -- in their order, with the vertices they use, renumbered in theirs.  ``transform``: the box
    frame (see ``box_transform``), ``dimensions``: its three lengths (a list or an x / y / z dict).  ``trim`` as in
    ``extract_mesh``; the capacities default to the mesh's own sizes, which always suffice."""
    lib = _lib.get()
    seg = np.ascontiguousarray(box_segments(transform, dimensions))
    v, t = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    max_v, max_t = _capacity(max_vertices, v, "max_vertices"), _capacity(max_triangles, t, "max_triangles")
    dev = mesh.vertices.device
    _lib.require_device(mesh.vertices, mesh.triangles)
    vertices = torch.zeros((max_v, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((max_t, 3), dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.dcn_mesh_crop_workspace(v, t), dtype=torch.uint8, device=dev)
    rc = lib.dcn_mesh_crop(v, t, _lib.ptr(mesh.vertices), _lib.ptr(mesh.triangles), _lib.host_ptr(seg), max_v, max_t,
                           _lib.ptr(vertices), _lib.ptr(triangles), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_mesh_crop")
    return _finish(vertices, triangles, counts, trim, "crop_to_box")


def fuse_scene(depth, poses, K, volume_spec, crop_box, pixel_offset=DEFAULT_PIXEL_OFFSET, max_depth_mm=DEFAULT_MAX_DEPTH_MM,
               min_weight=1, trim=False):
    """depth images and poses -> (full mesh, foreground mesh), what the reference keeps as fusion_mesh.ply and
    fusion_mesh_foreground.ply.  ``volume_spec``: a dict of TsdfVolume's arguments (origin, voxel_size, shape and optionally
    trunc_margin, max_vertices, max_triangles) or a TsdfVolume to add to; ``crop_box``: a dict with ``transform`` and
    ``dimensions`` as the station's change_detection.yaml has it.  With ``trim=False`` (the default) nothing is read back:
    the meshes are padded to their capacities, carry the true counts as ``.counts`` (int32 [2] on the device) and go into
    ``render.render_scene`` as they are."""
    spec = {} if isinstance(volume_spec, TsdfVolume) else dict(volume_spec)
    caps = (spec.pop("max_vertices", None), spec.pop("max_triangles", None))
    vol = volume_spec if isinstance(volume_spec, TsdfVolume) else TsdfVolume(device=depth.device, **spec)
    vol.integrate(depth, poses, K, pixel_offset=pixel_offset, max_depth_mm=max_depth_mm)
    full = extract_mesh(vol, caps[0], caps[1], min_weight=min_weight, trim=trim)
    full = full if trim else full[0]
    fg = crop_to_box(full, crop_box["transform"], crop_box["dimensions"], trim=trim)
    return full, (fg if trim else fg[0])
