"""The host-side argument rules of the device data path (augment, merge, samples, frames, evaluate), each stated once: what a
mask, a depth map, an image, camera rows, an offsets vector, per-pair seeds and a replay table have to be, and what they are
turned into before their pointer goes to the library.  Every checker raises ValueError and returns a contiguous tensor."""
import numpy as np
import torch

CAM_FLOATS = 50            # one camera row: K, K^-1 (9 each), pose a, pose b^-1 (16 each), fp32
UV_INT64, UV_FLOAT32 = 0, 1


def mask(m, n, h, w, what):
    """0/1 mask [n, h, w] of any dtype ``.to(uint8)`` maps onto 0/1 -> uint8"""
    if m is None or tuple(m.shape) != (n, h, w):
        raise ValueError("%s must be [%d, %d, %d], got %s" % (what, n, h, w, None if m is None else tuple(m.shape)))
    return (m if m.dtype == torch.uint8 else m.to(torch.uint8)).contiguous()


def depth(d, n, h, w, what):
    """16-bit integer depth [n, h, w] in millimetres (int16 / uint16: the same bits)"""
    if tuple(d.shape) != (n, h, w) or d.element_size() != 2 or d.is_floating_point():
        raise ValueError("%s must be 16-bit integer [%d, %d, %d] millimetres, got %s %s" % (what, n, h, w, d.dtype,
                                                                                            tuple(d.shape)))
    return d.contiguous()


def image(t, n, h, w, what):
    """uint8 images [n, h, w, 3] (h = w = None: any size)"""
    s = tuple(t.shape)
    if t.dtype != torch.uint8 or len(s) != 4 or s[0] != n or s[3] != 3 or (h is not None and s[1:3] != (h, w)):
        raise ValueError("%s must be uint8 [%d, %s, %s, 3], got %s %s" % (what, n, "H" if h is None else h,
                                                                         "W" if h is None else w, t.dtype, s))
    return t.contiguous()


def camera_rows(c, n, what, as_given=False):
    """float32 camera rows [n, CAM_FLOATS].  ``as_given``: refuse rows that are not contiguous instead of copying them (the
    sample builders, which promise to make no copy of ``cameras``)."""
    if tuple(c.shape) != (n, CAM_FLOATS) or c.dtype != torch.float32 or (as_given and not c.is_contiguous()):
        raise ValueError("%s must be %sfloat32 [%d, %d], got %s %s" % (what, "contiguous " if as_given else "", n, CAM_FLOATS,
                                                                      c.dtype, tuple(c.shape)))
    return c.contiguous()


def offsets(o, n, dev, what="offsets"):
    """[n + 1] offsets, tensor or sequence -> int64 on ``dev``"""
    if not torch.is_tensor(o):
        o = torch.tensor([int(x) for x in o], dtype=torch.int64)
    if o.numel() != n + 1:
        raise ValueError("%s must have B + 1 = %d entries, got %d" % (what, n + 1, o.numel()))
    return o.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous().view(-1)


def seeds_for(n, dev, generator, seeds, what="seeds"):
    """The caller's per-pair seeds, or ``samples.draw_seeds`` with ``generator`` -> int64 [n] on ``dev``"""
    if seeds is None:
        from .samples import draw_seeds
        return draw_seeds(n, dev, generator)
    seeds = torch.as_tensor(seeds).to(device=dev, dtype=torch.int64).contiguous().view(-1)
    if seeds.numel() != n:
        raise ValueError("%s must hold one int64 per pair (%d)" % (what, n))
    return seeds


def replay_table(x, shape, what, dev):
    """A host table of replay positions (anything numpy reads as integers) -> int32 ``shape`` on ``dev``"""
    t = torch.as_tensor(np.asarray(x.cpu() if torch.is_tensor(x) else x, np.int64).astype(np.int32))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be [%s], got %s" % (what, ", ".join(str(int(s)) for s in shape), tuple(t.shape)))
    return t.to(dev).contiguous()


def uv_dtype(t):
    """The library's code for a pixel list's dtype; TypeError for anything but int64 / float32"""
    if t.dtype == torch.int64:
        return UV_INT64
    if t.dtype == torch.float32:
        return UV_FLOAT32
    raise TypeError("pixel lists must be int64 or float32 tensors, got %s" % t.dtype)


def mean_std(v):
    """An image mean or standard deviation -> 3 contiguous float32 on the host"""
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    if a.size != 3:
        raise ValueError("mean / std need 3 entries, got %d" % a.size)
    return a


def f32(a):
    """float64 -> float32, one rounding"""
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def camera_k_rows(K, n):
    """K ([3, 3] or [n, 3, 3] on the host; None: the reference's default K) -> (K float64 [n, 3, 3], float32 [n, 18] rows
    ``K | K^-1``, the inverse taken in float64 and each rounded once)"""
    if K is None:
        from dense_correspondence.correspondence_tools.correspondence_finder import get_default_K_matrix
        K = get_default_K_matrix()
    K = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    Ks = np.broadcast_to(K, (n, 3, 3)) if K.shape == (3, 3) else K
    if Ks.shape != (n, 3, 3):
        raise ValueError("K must be [3, 3] or [%d, 3, 3], got %s" % (n, K.shape))
    return Ks, np.stack([np.concatenate([f32(k).reshape(-1), f32(np.linalg.inv(k)).reshape(-1)]) for k in Ks])
