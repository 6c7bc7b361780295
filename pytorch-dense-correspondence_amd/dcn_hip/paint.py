"""Host side of the paint kernels (csrc/paint_kernels.hip, include/dcn_hip.h section 18): carries images, or the network's
output, back onto a scene's mesh -- colour fusion (the colour per vertex that spartan's tsdf-fusion writes into fusion_mesh.ply)
and the descriptor-coloured mesh (mesh_descriptor_color_app.py, DescriptorMeshColor.color_mesh_using_descriptors) as one
operation: for every vertex and every view, project the vertex, decide whether the view sees it, read the view's pixel,
accumulate.

    paint = MeshPaint(mesh, 3, torch.uint8)                        # mesh: render.Mesh, padded ones of fuse_scene included
    paint.add(rgb, depth, poses, K, pixel_offset=0.5)              # [F, H, W, 3] uint8 views; calls accumulate
    out = paint.finish()                                           # mean, variance, spread, count, colours: device tensors
    write_coloured_ply("fusion_mesh.ply", mesh.vertices.cpu(), mesh.triangles.cpu(), out.colours.cpu())
    out, summary = paint_descriptors(dcn, store, mesh, scene=0)    # the network's descriptors of every frame of the scene

``spread`` is the root of the summed per-channel variance of a vertex's descriptors over the views that see it -- what the
contrastive loss pulls towards zero for matches, measured with no labels and no sampled pairs.  The arithmetic is defined in the
header (18a, 18b): single correctly rounded float64 operations, the same bit for bit from run to run, whatever the split of
the frames over calls.  Views are not weighted by viewing angle and pixels are read nearest, not bilinearly."""
import collections

import numpy as np
import torch

from . import _lib
from .render import DEFAULT_MASK_THRESHOLD, PlyError, _ply_header, _pinhole, _poses

MAX_CHANNELS = 32
DEFAULT_MARGIN_MM = float(DEFAULT_MASK_THRESHOLD)      # the change detection's 10 mm

Painted = collections.namedtuple("Painted", "mean variance spread count colours")
Painted.__doc__ = """mean float32 [V, C] (0 where unseen), variance float32 [V] (the per-channel variances summed; NaN where unseen,
the tables' convention), spread = variance.sqrt(), count int32 [V] (the views that saw the vertex), colours uint8 [V, 3]."""


def _image_type(dtype):
    if dtype == torch.uint8:
        return 0
    if dtype == torch.float32:
        return 1
    raise ValueError("views must be torch.uint8 or torch.float32, got %s" % (dtype,))


class MeshPaint(object):
    """The per-vertex state of one mesh on its device: ``count`` int32 [V], ``sum`` and ``sumsq`` float64 [V, C] for views of
    ``channels`` (1 .. 32) values per pixel of ``dtype`` (torch.uint8: the store's RGB; torch.float32: descriptor images).  A
    padded mesh (``fusion.extract_mesh(trim=False)``) brings its true vertex count on the device as ``mesh.counts``: the rows
    beyond it take nothing, and nothing is read back."""

    def __init__(self, mesh, channels, dtype=torch.float32):
        c = int(channels)
        if not 1 <= c <= MAX_CHANNELS:
            raise ValueError("channels must be in 1 .. %d, got %d" % (MAX_CHANNELS, c))
        self.image_type = _image_type(dtype)
        self.dtype, self.channels = dtype, c
        self.vertices = mesh.vertices
        if not torch.is_tensor(self.vertices) or self.vertices.dtype != torch.float32 or self.vertices.dim() != 2 \
                or self.vertices.shape[1] != 3 or not self.vertices.is_contiguous():
            raise ValueError("the mesh's vertices must be a contiguous float32 tensor [V, 3]")
        counts = getattr(mesh, "counts", None)
        self.valid_vertices = None if counts is None else counts[0:1]
        dev = self.vertices.device
        v = int(self.vertices.shape[0])
        self.count = torch.empty(v, dtype=torch.int32, device=dev)
        self.sum = torch.empty((v, c), dtype=torch.float64, device=dev)
        self.sumsq = torch.empty((v, c), dtype=torch.float64, device=dev)
        _lib.require_device(self.vertices, self.valid_vertices)
        lib = _lib.get()
        for t in (self.count, self.sum, self.sumsq):                         # (zero-filled by a kernel)
            if t.numel():
                _lib.check(lib.dcn_fill_bytes(_lib.ptr(t), 0, t.numel() * t.element_size(), _lib.stream_ptr()), "dcn_fill_bytes")

    @property
    def device(self):
        return self.vertices.device

    def add(self, images, depth, poses, K, mask=None, pixel_offset=0.0, margin_mm=DEFAULT_MARGIN_MM, frames_per_launch=None):
        """Adds the views, in their order: images [F, H, W, C] of the paint's dtype, depth 16-bit integer [F, H, W] millimetres
        (the store's int16 tensors as they are), poses [F, 4, 4] camera-to-world, K = (fx, fy, cx, cy) or 3 x 3, mask uint8
        [F, H, W] or None.  A view paints a vertex when the vertex projects into the image, onto a pixel whose depth is within
        ``margin_mm`` of the vertex's own, either way, and whose mask is not 0.  ``pixel_offset``: 0.0 for images on
        ``render.render_depth``'s grid, 0.5 for the sensor's.  ``frames_per_launch`` (1 .. 64; None: the library's default) does
        not change the result.  No host synchronisation.  -> self"""
        lib = _lib.get()
        dev = self.device
        if not torch.is_tensor(images) or images.dtype != self.dtype:
            raise ValueError("images must be a %s tensor" % (self.dtype,))
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if images.dim() != 4 or images.shape[0] < 1 or images.shape[3] != self.channels:
            raise ValueError("images must be [F, H, W, %d], got %s" % (self.channels, tuple(images.shape)))
        f, h, w = (int(x) for x in images.shape[:3])
        if not torch.is_tensor(depth) or depth.is_floating_point() or depth.element_size() != 2:
            raise ValueError("depth must be a 16-bit integer tensor")
        if depth.dim() == 2:
            depth = depth.unsqueeze(0)
        if tuple(depth.shape) != (f, h, w):
            raise ValueError("depth must be [%d, %d, %d], got %s" % (f, h, w, tuple(depth.shape)))
        if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.uint8):
            raise ValueError("mask must be a uint8 tensor")
        if mask is not None and mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if mask is not None and tuple(mask.shape) != (f, h, w):
            raise ValueError("mask must be [%d, %d, %d], got %s" % (f, h, w, tuple(mask.shape)))
        if not 1 <= h <= 16384 or not 1 <= w <= 16384:
            raise ValueError("H and W must be in 1 .. 16384")
        for name, t in (("images", images), ("depth", depth), ("mask", mask), ("poses", poses)):
            if torch.is_tensor(t) and t.device != dev:
                raise ValueError("%s are on %s, the mesh on %s" % (name, t.device, dev))
        p = _poses(poses, dev)
        if p.shape[0] != f:
            raise ValueError("%d poses for %d views" % (p.shape[0], f))
        margin = float(margin_mm)
        if not (margin >= 0.0 and np.isfinite(margin)):
            raise ValueError("margin_mm must be >= 0")
        chunk = -1 if frames_per_launch is None else int(frames_per_launch)
        if chunk == 0 or chunk > 64:
            raise ValueError("frames_per_launch must be in 1 .. 64")
        fx, fy, cx, cy = _pinhole(K)
        im, d = images.contiguous(), depth.contiguous()
        m = None if mask is None else mask.contiguous()
        _lib.require_device(im, d, m, p, self.sum)
        rc = lib.dcn_mesh_paint(int(self.vertices.shape[0]), _lib.ptr(self.vertices), _lib.ptr(self.valid_vertices), f, h, w,
                                self.channels, self.image_type, _lib.ptr(im), _lib.ptr(d), _lib.ptr(m), _lib.ptr(p), fx, fy, cx,
                                cy, float(pixel_offset), margin, chunk, _lib.ptr(self.count), _lib.ptr(self.sum),
                                _lib.ptr(self.sumsq), _lib.stream_ptr())
        _lib.check(rc, "dcn_mesh_paint")
        return self

    def _range(self, value, default, what):
        if value is None:
            return default()
        if torch.is_tensor(value):
            if value.device != self.device:
                raise ValueError("%s is on %s, the mesh on %s" % (what, value.device, self.device))
            t = value.to(torch.float64).reshape(-1)
        else:
            t = torch.from_numpy(np.asarray(value, dtype=np.float64).reshape(-1)).to(self.device)
        if t.numel() == 1:
            t = t.repeat(self.channels)
        if t.numel() != self.channels:
            raise ValueError("%s must hold one number or %d" % (what, self.channels))
        return t.contiguous()

    def finish(self, min_views=1, lo=None, hi=None, channels=(0, 1, 2), unseen=(0, 0, 0)):
        """-> Painted of device tensors; the state stays as it is, so more views may follow.  A vertex seen by fewer than
        ``min_views`` views has mean 0, variance and spread NaN and the ``unseen`` colour.  Colours: the means of the three
        ``channels`` (a paint of fewer than three channels repeats its last) between ``lo`` and ``hi`` -- numbers, one per
        channel or one for all, host or device.  They default to 0 and 255 for uint8 views (the rounded mean colour) and, for
        float views, to the smallest and largest mean of each channel over the painted vertices, taken on the device.  Nothing
        is read back."""
        lib = _lib.get()
        if int(min_views) < 1:
            raise ValueError("min_views must be >= 1")
        c, dev = self.channels, self.device
        ch = [min(int(k), c - 1) if c < 3 else int(k) for k in channels]
        if len(ch) != 3 or not all(0 <= k < c for k in ch):
            raise ValueError("channels must be three channel numbers in 0 .. %d" % (c - 1))
        un = [int(k) for k in unseen]
        if len(un) != 3 or not all(0 <= k <= 255 for k in un):
            raise ValueError("unseen must be three bytes")
        v = int(self.vertices.shape[0])
        mean = torch.empty((v, c), dtype=torch.float32, device=dev)
        variance = torch.empty(v, dtype=torch.float32, device=dev)
        colours = torch.empty((v, 3), dtype=torch.uint8, device=dev)

        def launch(lo_t, hi_t, out):
            rc = lib.dcn_mesh_paint_finish(v, c, _lib.ptr(self.count), _lib.ptr(self.sum), _lib.ptr(self.sumsq), int(min_views),
                                           _lib.ptr(mean), _lib.ptr(variance), ch[0], ch[1], ch[2], _lib.ptr(lo_t),
                                           _lib.ptr(hi_t), un[0], un[1], un[2], _lib.ptr(out), _lib.stream_ptr())
            _lib.check(rc, "dcn_mesh_paint_finish")
        if self.dtype == torch.uint8:
            zeros = lambda: torch.zeros(c, dtype=torch.float64, device=dev)
            launch(self._range(lo, zeros, "lo"), self._range(hi, lambda: zeros() + 255.0, "hi"), colours)
        else:
            if lo is None or hi is None:
                launch(None, None, None)                                     # the means first: their range is the default
                painted = (self.count >= int(min_views)).unsqueeze(1)
                inf = torch.full((1, c), float("inf"), dtype=torch.float32, device=dev)    # (no painted vertex: inf and -inf)
            lo_t = self._range(lo, lambda: torch.cat([torch.where(painted, mean, inf), inf]).amin(0).to(torch.float64), "lo")
            hi_t = self._range(hi, lambda: torch.cat([torch.where(painted, mean, -inf), -inf]).amax(0).to(torch.float64), "hi")
            launch(lo_t, hi_t, colours)
        return Painted(mean, variance, variance.sqrt(), self.count, colours)


def paint_colours(mesh, rgb, depth, poses, K, mask=None, pixel_offset=0.5, margin_mm=DEFAULT_MARGIN_MM, min_views=1,
                  unseen=(0, 0, 0)):
    """Colour fusion in one call: rgb uint8 [F, H, W, 3] (the store's layout) with the depth images and poses they were logged
    with -> Painted; ``colours`` is each vertex's mean colour over the views that see it, rounded.  ``pixel_offset`` defaults
    to the sensor's 0.5."""
    paint = MeshPaint(mesh, 3, torch.uint8)
    paint.add(rgb, depth, poses, K, mask=mask, pixel_offset=pixel_offset, margin_mm=margin_mm)
    return paint.finish(min_views=min_views, unseen=unseen)


def _stats_range(dcn, c, norm_type):
    """(lo, hi) of ``dcn.descriptor_image_stats`` where that file exists and fits, as ``evaluate.descriptor_pictures`` reads it"""
    try:                                                    # (evaluation.py:1395-1400)
        stats = dcn.descriptor_image_stats
    except Exception:
        return None, None
    if not stats or norm_type not in stats:
        return None, None
    lo, hi = list(stats[norm_type]["min"]), list(stats[norm_type]["max"])
    if len(lo) != c or len(hi) != c:
        return None, None
    return lo, hi


def paint_descriptors(dcn, store, mesh, scene, frames=None, batch=16, mask=True, pixel_offset=0.0, margin_mm=DEFAULT_MARGIN_MM,
                      min_views=1, lo=None, hi=None, channels=(0, 1, 2), unseen=(0, 0, 0), descriptor_norm_type="mask_image",
                      mean=None, std=None):
    """The descriptor-coloured mesh of one scene of a frame store: its frames (``frames``: numbers within the scene, by default
    all of them) go, ``batch`` at a time, through ToTensor + Normalize and the network in eval mode -- the path of
    ``compute_descriptor_statistics_on_dataset`` -- and every batch of descriptor images is painted as it is produced with the
    store's depth images and poses (``mask=True``: only through the store's object mask), so a scene's descriptor images are
    never all resident.  ``lo`` / ``hi`` default to ``dcn.descriptor_image_stats[descriptor_norm_type]`` where that file exists
    (as in ``descriptor_pictures``), otherwise to MeshPaint.finish's.  ``pixel_offset`` defaults to 0.0: the store holds rendered
    depth images.  -> (Painted, summary float64 [3] on the device: the number of vertices with count >= min_views, their mean
    spread and their largest spread).  ``spread_curve(painted)`` puts the spread through the evaluation's curve kernel as a
    table of one curve (``drop_nan`` leaves the unseen vertices out).  Nothing is read back."""
    from . import augment as _aug
    from .evaluate._chain import _forward_in_eval_mode
    s = int(scene)
    if not 0 <= s < store.num_scenes:
        raise ValueError("scene must be in 0 .. %d" % (store.num_scenes - 1))
    if int(batch) < 1:
        raise ValueError("batch must be >= 1")
    if mesh.vertices.device != store.device:
        raise ValueError("the mesh is on %s, the store on %s" % (mesh.vertices.device, store.device))
    first, end = int(store.scene_first_frame_host[s]), int(store.scene_first_frame_host[s + 1])
    if frames is None:
        pick = lambda t: t[first:end]
    else:
        rows = np.asarray(frames, dtype=np.int64).reshape(-1)
        if rows.size < 1 or rows.min() < 0 or rows.max() >= end - first:
            raise ValueError("frames must be numbers in 0 .. %d" % (end - first - 1))
        index = torch.from_numpy(rows + first).to(store.device)
        pick = lambda t: t.index_select(0, index)
    rgb, depth, obj, poses = pick(store.rgb), pick(store.depth), pick(store.mask), pick(store.poses).view(-1, 4, 4)
    K = store.K[s]
    state = []

    def consume(at, n, res):
        if not state:
            state.append(MeshPaint(mesh, int(res.shape[3]), torch.float32))
        state[0].add(res, depth[at:at + n], poses[at:at + n], K, mask=obj[at:at + n] if mask else None,
                     pixel_offset=pixel_offset, margin_mm=margin_mm)
    _forward_in_eval_mode(dcn, rgb, obj, None, None, int(batch), _aug.DEFAULT_IMAGE_MEAN if mean is None else mean,
                          _aug.DEFAULT_IMAGE_STD_DEV if std is None else std, consume)
    paint = state[0]
    if lo is None and hi is None:
        lo, hi = _stats_range(dcn, paint.channels, descriptor_norm_type)
    out = paint.finish(min_views=min_views, lo=lo, hi=hi, channels=channels, unseen=unseen)
    return out, spread_summary(out, min_views)


def spread_summary(painted, min_views=1):
    """-> float64 [3] on the device: the number of vertices with count >= min_views, the mean and the maximum of their spread
    (NaN and -inf where there is none)"""
    ok = painted.count >= int(min_views)
    spread = painted.spread.to(torch.float64)
    n = ok.sum().to(torch.float64)
    total = torch.where(ok, spread, torch.zeros_like(spread)).sum()
    top = torch.where(ok, spread, torch.full_like(spread, float("-inf"))).amax() if spread.numel() else total - float("inf")
    return torch.stack([n, total / n, top])


def spread_curve(painted, num_bins=100):
    """``spread`` as a table of one curve through the evaluation's curve kernel, as it is (``evaluate.cumulative_frequencies``,
    the function under ``evaluation_curves``): the unseen vertices' NaN rows are dropped (``drop_nan``).  -> EvalCurves with
    the field "spread": cumulative frequencies and the area above the curve; nothing is read back."""
    from .evaluate.curves import cumulative_frequencies
    return cumulative_frequencies(painted.spread.to(torch.float64), None, num_bins, True, None, ("spread",))


def write_coloured_ply(path, vertices, triangles, colours):
    """Writes a binary little-endian PLY file with ``uchar red, green, blue`` after ``float x, y, z`` per vertex -- the layout of
    the reference's fusion_mesh.ply -- and ``uchar int`` face lists; ``render.read_ply`` reads its geometry back as it is.
    Triangle rows that hold a negative index (the padding of untrimmed meshes) are left out.  Host arrays.  -> path"""
    v = np.asarray(vertices, dtype="<f4").reshape(-1, 3)
    rgb = np.asarray(colours)
    if rgb.dtype != np.uint8 or rgb.shape != (len(v), 3):
        raise ValueError("colours must be uint8 [%d, 3]" % len(v))
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    t = t[(t >= 0).all(axis=1)]
    if t.size and t.max() >= len(v):
        raise ValueError("a triangle names a vertex outside 0 .. %d" % (len(v) - 1))
    rows = np.zeros(len(v), dtype=[("xyz", "<f4", (3,)), ("rgb", "u1", (3,))])
    rows["xyz"], rows["rgb"] = v, rgb
    faces = np.zeros(len(t), dtype=[("_count", "u1"), ("_index", "<i4", (3,))])
    faces["_count"] = 3
    faces["_index"] = t
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x", "property float y",
            "property float z", "property uchar red", "property uchar green", "property uchar blue",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rows.tobytes())
        f.write(faces.tobytes())
    return path


def read_ply_colours(path):
    """-> uint8 [V, 3]: the ``red, green, blue`` vertex properties of a binary little-endian PLY file (the geometry:
    ``render.read_ply``).  PlyError where the file has none."""
    from .render import _PLY_TYPES
    with open(path, "rb") as f:
        fmt, nv, vprops, _, _ = _ply_header(f, path)
        if fmt != "binary_little_endian":
            raise PlyError("%s: colours are read from binary_little_endian files only" % path)
        names = [n for n, _ in vprops]
        if not all(n in names for n in ("red", "green", "blue")):
            raise PlyError("%s: the vertex element has no red, green and blue" % path)
        vdt = np.dtype([(n, "<" + _PLY_TYPES[t]) for n, t in vprops])
        vt = np.frombuffer(f.read(vdt.itemsize * nv), dtype=vdt)
        if vt.size != nv:
            raise PlyError("%s: the file ends inside the vertex element" % path)
    if any(vt[n].dtype != np.uint8 for n in ("red", "green", "blue")):
        raise PlyError("%s: red, green and blue must be uchar" % path)
    return np.ascontiguousarray(np.stack([vt[n] for n in ("red", "green", "blue")], axis=1)) if nv \
        else np.zeros((0, 3), np.uint8)
