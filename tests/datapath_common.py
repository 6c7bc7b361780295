"""Shared by tests/test_emu_datapath.py (host emulation, "cpu") and tests/test_gpu_datapath.py (gfx950, "cuda"); not a test
module.  The host side of the device data path (dcn_hip/samples.py, frames.py, evaluate/, merge.py, augment.py, pairgen.py and
the host half of csrc/sample_kernels.hip):

  a. every clause of the argument tests of the five sample entry points, one argument at a time on otherwise valid calls (n = 1,
     7 x 9, 16 attempts, k1 = k2 = 1): DCN_E_INVALID, and nothing launched -- the caller's buffers keep their sentinel;
  b. the Python argument errors of every public function that takes a mask, a depth map, an image, camera rows, offsets, seeds,
     augmentation records or a replay table: the exception type and a fragment of the message;
  c. call sites the rest of the suite does not reach, against samples_common's numpy restatement: uniform candidates without
     the inverted mask at 7 x 9 with more attempts than pixels, complete_samples without a single match, find_eval_matches with
     more attempts than pixels (replayed and seeded), concat_sample_batches of one batch and of a within-scene batch joined
     with an across-scene batch."""
import ctypes

import numpy as np
import pytest
import torch

import samples_common as sc

N, H, W, A, K1, K2, M = 1, 7, 9, 16, 1, 1, 4
HW = H * W
SENTINEL = 0x5A
DCN_E_INVALID = -1
MAX_PAIRS = 1024                                            # kMaxPairs of csrc/sample_kernels.hip
SMALL_K = np.array([[20.0, 0, 4.2], [0, 20.0, 3.1], [0, 0, 1]])
ENTRIES = ["dcn_within_scene_samples", "dcn_across_scene_samples", "dcn_complete_samples", "dcn_eval_matches"]


def _pose(ry, t):
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]]
    T[:3, 3] = t
    return T


def example(n, h, w, seed):
    """depth uint16 [2, n, h, w] (a wavy wall around 0.9 m with no-return holes), masks uint8 [2, n, h, w] (an ellipse each),
    poses a, b [n, 4, 4] a few millimetres apart."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth, masks = np.zeros((2, n, h, w), np.uint16), np.zeros((2, n, h, w), np.uint8)
    for k in range(2):
        for p in range(n):
            d = 900 + 60 * np.sin(xs / (6 + 4 * rng.rand())) + 50 * np.cos(ys / (5 + 3 * rng.rand()))
            d[rng.rand(h, w) < 0.05] = 0
            depth[k, p] = d.astype(np.uint16)
            cy, cx = rng.rand() * h, rng.rand() * w
            masks[k, p] = (((ys - cy) / (0.35 * h)) ** 2 + ((xs - cx) / (0.35 * w)) ** 2) <= 1.0
    pa = np.stack([_pose(0, [0, 0, 0])] * n)
    pb = np.stack([_pose(-0.003, [0.004, 0.002 * p, 0.001]) for p in range(n)])
    return depth, masks, pa, pb


def K_for(h):
    return sc.default_K() if h > 10 else SMALL_K


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------------------------ a. refusals
def _sentinel(nbytes, device):
    return torch.full((int(nbytes),), SENTINEL, dtype=torch.uint8, device=device)


def _refusal_inputs(device):
    depth, masks, pa, pb = example(N, H, W, seed=7)
    masks[:] = 1
    cams = np.stack([sc.cams_of(SMALL_K, pa[p], pb[p]) for p in range(N)]).astype(np.float32)
    return dict(depth_a=_t(depth[0].view(np.int16), device), depth_b=_t(depth[1].view(np.int16), device),
                mask_a=_t(masks[0], device), mask_b=_t(masks[1], device), cams=_t(cams, device),
                seeds=_t(np.array([11], np.int64), device), order_seeds=_t(np.array([5], np.int64), device),
                rand=_t(np.zeros(4, np.float32), device), rand_offsets=_t(np.zeros((6, N + 1), np.int64), device),
                u=_t(np.array([1, 2, 3], np.int64), device), list_offsets=_t(np.array([0, 3], np.int64), device))


def _lists_out(cap, workspace, device):
    """The six outputs of a list builder (16 spare bytes behind idx_a / idx_b for the misaligned clause) and its workspace"""
    return dict(idx_a=_sentinel(8 * cap + 16, device), idx_b=_sentinel(8 * cap + 16, device),
                offsets=_sentinel(8 * (4 * N + 1), device), empty=_sentinel(N, device), type=_sentinel(4 * N, device),
                status=_sentinel(4, device), workspace=_sentinel(workspace, device))


def _common_clauses(nulls, cap_of, seeds_only=False):
    """The clauses the list builders share.  ``cap_of(**changed)``: the capacity that goes with changed sizes, so that only the
    clause under test refuses the call."""
    out = [("%s null" % k, {k: None}) for k in nulls]
    for label, ch in (("n = 0", dict(n=0)), ("n above the pair limit", dict(n=MAX_PAIRS + 1)), ("h = 0", dict(h=0)),
                      ("w = 0", dict(w=0)), ("2^30 pixels", dict(h=1 << 15, w=1 << 15))):
        out.append((label, dict(ch, **cap_of(**ch))))
    out += [("neither seeds nor a replay stream", dict(seeds=None)),
            ("no seeds, replay values without offsets", dict(seeds=None, rand="rand")),
            ("no seeds, replay offsets without values", dict(seeds=None, rand_offsets="rand_offsets"))]
    if not seeds_only:
        out += [("capacity one too large", dict(capacity=cap_of()["capacity"] + 1)),
                ("capacity one too small", dict(capacity=cap_of()["capacity"] - 1)),
                ("idx_a misaligned by 8 bytes", dict(idx_a="idx_a+8")), ("idx_b misaligned by 8 bytes", dict(idx_b="idx_b+8"))]
    return out


def refusal_entries(device):
    """-> {entry point: (argument names in ABI order, valid arguments, output tensors, [(clause, changed arguments)])}; the
    clauses are those of the argument test at the top of each entry point in csrc/sample_kernels.hip.  An argument given as a
    string names a tensor (``"idx_a+8"``: 8 bytes into it)."""
    from dcn_hip import _lib
    lib = _lib.get()
    ins = _refusal_inputs(device)
    E = {}
    # dcn_within_scene_samples
    cap = lambda n=N, h=H, w=W, attempts=A, k_masked=K1, k_background=K2: dict(
        capacity=n * (attempts * (1 + k_masked + k_background) + h * w))
    outs = _lists_out(cap()["capacity"], lib.dcn_sample_workspace(N, H, W, A, A), device)
    names = ["n", "h", "w", "depth_a", "depth_b", "mask_a", "mask_b", "cams", "attempts", "k_masked", "k_background", "flags",
             "aug_params", "seeds", "rand", "rand_offsets", "data_type", "idx_a", "idx_b", "capacity", "offsets", "empty", "type",
             "status", "workspace", "stream"]
    args = dict(n=N, h=H, w=W, depth_a="depth_a", depth_b="depth_b", mask_a="mask_a", mask_b="mask_b", cams="cams", attempts=A,
                k_masked=K1, k_background=K2, flags=3, aug_params=None, seeds="seeds", rand=None, rand_offsets=None, data_type=0,
                idx_a="idx_a", idx_b="idx_b", offsets="offsets", empty="empty", type="type", status="status",
                workspace="workspace", **cap())
    clauses = _common_clauses(["depth_a", "depth_b", "mask_a", "mask_b", "cams"] + list(outs), cap)
    for label, ch in (("attempts = 0", dict(attempts=0)), ("attempts above 2^30", dict(attempts=(1 << 30) + 1)),
                      ("k1 = 0", dict(k_masked=0)), ("k2 = 0", dict(k_background=0))):
        clauses.append((label, dict(ch, **cap(**ch))))
    clauses.append(("an unknown flag bit", dict(flags=4)))
    E["dcn_within_scene_samples"] = (names, args, outs, clauses)
    # dcn_across_scene_samples
    cap = lambda n=N, h=H, w=W, num_samples=A: dict(capacity=n * num_samples)
    outs = _lists_out(cap()["capacity"], lib.dcn_sample_workspace(N, H, W, 0, 0), device)
    names = ["n", "h", "w", "mask_a", "mask_b", "num_samples", "aug_params", "seeds", "rand", "rand_offsets", "data_type",
             "idx_a", "idx_b", "capacity", "offsets", "empty", "type", "status", "workspace", "stream"]
    args = dict(n=N, h=H, w=W, mask_a="mask_a", mask_b="mask_b", num_samples=A, aug_params=None, seeds="seeds", rand=None,
                rand_offsets=None, data_type=1, idx_a="idx_a", idx_b="idx_b", offsets="offsets", empty="empty", type="type",
                status="status", workspace="workspace", **cap())
    clauses = _common_clauses(["mask_a", "mask_b"] + list(outs), cap)
    clauses.append(("num_samples = 0", dict(num_samples=0, **cap(num_samples=0))))
    E["dcn_across_scene_samples"] = (names, args, outs, clauses)
    # dcn_complete_samples
    cap = lambda n=N, h=H, w=W, count=3, k_masked=K1, k_background=K2: dict(
        capacity=count * (1 + k_masked + k_background) + n * h * w)
    outs = _lists_out(cap()["capacity"], lib.dcn_sample_workspace(N, H, W, 0, 3), device)
    names = ["n", "h", "w", "u_a", "v_a", "u_b", "v_b", "uv_b_dtype", "list_offsets", "count", "mask_a", "mask_b", "k_masked",
             "k_background", "flags", "aug_params", "seeds", "rand", "rand_offsets", "data_type", "idx_a", "idx_b", "capacity",
             "offsets", "empty", "type", "status", "workspace", "stream"]
    args = dict(n=N, h=H, w=W, u_a="u", v_a="u", u_b="u", v_b="u", uv_b_dtype=0, list_offsets="list_offsets", count=3,
                mask_a="mask_a", mask_b="mask_b", k_masked=K1, k_background=K2, flags=2, aug_params=None, seeds="seeds", rand=None,
                rand_offsets=None, data_type=4, idx_a="idx_a", idx_b="idx_b", offsets="offsets", empty="empty", type="type",
                status="status", workspace="workspace", **cap())
    clauses = _common_clauses(["u_a", "v_a", "u_b", "v_b", "list_offsets", "mask_a", "mask_b"] + list(outs), cap)
    for label, ch in (("count below 0", dict(count=-1)), ("k1 = 0", dict(k_masked=0)), ("k2 = 0", dict(k_background=0))):
        clauses.append((label, dict(ch, **cap(**ch))))
    clauses += [("an unknown flag bit", dict(flags=4)), ("the within-scene flag bit", dict(flags=1)),
                ("uv_b_dtype 2", dict(uv_b_dtype=2)), ("uv_b_dtype -1", dict(uv_b_dtype=-1))]
    E["dcn_complete_samples"] = (names, args, outs, clauses)
    # dcn_eval_matches
    rows = N * min(M, A)
    outs = dict(u_a=_sentinel(8 * rows, device), v_a=_sentinel(8 * rows, device), u_b=_sentinel(4 * rows, device),
                v_b=_sentinel(4 * rows, device), offsets=_sentinel(8 * (N + 1), device), totals=_sentinel(4 * N, device),
                status=_sentinel(4, device), workspace=_sentinel(lib.dcn_eval_matches_workspace(N, H, W, A), device))
    names = ["n", "h", "w", "depth_a", "depth_b", "mask_a", "cams", "attempts", "seeds", "rand", "rand_offsets", "num_matches",
             "match_order", "order_seeds", "u_a", "v_a", "u_b", "v_b", "offsets", "totals", "status", "workspace", "stream"]
    args = dict(n=N, h=H, w=W, depth_a="depth_a", depth_b="depth_b", mask_a="mask_a", cams="cams", attempts=A, seeds="seeds",
                rand=None, rand_offsets=None, num_matches=M, match_order=None, order_seeds="order_seeds", u_a="u_a", v_a="v_a",
                u_b="u_b", v_b="v_b", offsets="offsets", totals="totals", status="status", workspace="workspace")
    clauses = _common_clauses(["depth_a", "depth_b", "mask_a", "cams"] + list(outs), lambda **ch: {}, seeds_only=True)
    clauses += [("attempts = 0", dict(attempts=0)), ("attempts above 4096", dict(attempts=4097)),
                ("num_matches = 0", dict(num_matches=0)), ("neither match_order nor order_seeds", dict(order_seeds=None))]
    E["dcn_eval_matches"] = (names, args, outs, clauses)
    return E, ins


def _resolve(v, tensors):
    if not isinstance(v, str):
        return v
    name, _, shift = v.partition("+")
    return tensors[name].data_ptr() + int(shift or 0)


def _call(lib, entry, names, args, tensors):
    from dcn_hip import _lib
    vals = [_lib.stream_ptr() if k == "stream" else _resolve(args[k], tensors) for k in names]
    return int(getattr(lib, entry)(*vals))


def _untouched(outs, device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return [k for k, t in outs.items() if not bool((t == SENTINEL).all())]


def check_refusals(entry, device):
    """The valid call is taken first (DCN_OK, so every refusal below is the changed argument's); then each clause."""
    from dcn_hip import _lib
    lib = _lib.get()
    E, ins = refusal_entries(device)
    names, args, outs, clauses = E[entry]
    tensors = dict(ins, **outs)
    assert _call(lib, entry, names, args, tensors) == 0, entry
    assert "status" in _untouched(outs, device)                 # (the valid call did run: it zeroed the status word)
    for t in outs.values():
        t.fill_(SENTINEL)
    assert len(clauses) == len({c[0] for c in clauses})
    for label, changed in clauses:
        assert set(changed) <= set(args), (label, changed)
        rc = _call(lib, entry, names, dict(args, **changed), tensors)
        assert rc == DCN_E_INVALID, (entry, label, rc)
    assert _untouched(outs, device) == [], entry


def check_concat_refusals(device):
    """dcn_concat_samples: one valid group of one pair without entries, then every clause of its argument test (the whole
    call's, and the per-group ones)."""
    from dcn_hip import _lib
    lib = _lib.get()
    src = dict(idx_a=_t(np.full(4, -1, np.int64), device), idx_b=_t(np.full(4, -1, np.int64), device),
               offsets=_t(np.zeros(5, np.int64), device), status=_t(np.zeros(1, np.int32), device))
    outs = dict(idx_a_out=_sentinel(8 * 4 + 16, device), idx_b_out=_sentinel(8 * 4 + 16, device),
                offsets_out=_sentinel(8 * 5, device), status_out=_sentinel(4, device))
    ptrs = lambda k, n=1: (ctypes.c_void_p * 8)(*([src[k].data_ptr()] * n))
    ints = lambda ct, v: (ct * 8)(*v)
    names = ["groups", "n", "idx_a", "idx_b", "offsets", "capacity_in", "status_in", "idx_a_out", "idx_b_out", "capacity",
             "offsets_out", "status", "stream"]
    args = dict(groups=1, n=ints(ctypes.c_int, [1]), idx_a=ptrs("idx_a"), idx_b=ptrs("idx_b"), offsets=ptrs("offsets"),
                capacity_in=ints(ctypes.c_int64, [4]), status_in=ptrs("status"), idx_a_out="idx_a_out", idx_b_out="idx_b_out",
                capacity=4, offsets_out="offsets_out", status="status_out")
    assert _call(lib, "dcn_concat_samples", names, args, outs) == 0
    assert set(_untouched(outs, device)) == {"idx_a_out", "idx_b_out", "offsets_out", "status_out"}
    for t in outs.values():
        t.fill_(SENTINEL)
    null_group = (ctypes.c_void_p * 8)()
    clauses = [("groups = 0", dict(groups=0)), ("more than 8 groups", dict(groups=9)), ("n null", dict(n=None)),
               ("idx_a null", dict(idx_a=None)), ("idx_b null", dict(idx_b=None)), ("offsets null", dict(offsets=None)),
               ("capacity_in null", dict(capacity_in=None)), ("offsets_out null", dict(offsets_out=None)),
               ("status null", dict(status=None)), ("capacity below 0", dict(capacity=-1)),
               ("idx_a_out null with a capacity", dict(idx_a_out=None)), ("idx_b_out null with a capacity", dict(idx_b_out=None)),
               ("idx_a_out misaligned by 8 bytes", dict(idx_a_out="idx_a_out+8")),
               ("idx_b_out misaligned by 8 bytes", dict(idx_b_out="idx_b_out+8")),
               ("a group without pairs", dict(n=ints(ctypes.c_int, [0]))),
               ("a group's offsets null", dict(offsets=null_group)),
               ("a group's capacity below 0", dict(capacity_in=ints(ctypes.c_int64, [-1]))),
               ("a group's idx_a null with a capacity", dict(idx_a=null_group)),
               ("a group's idx_b null with a capacity", dict(idx_b=null_group)),
               ("more pairs than the pair limit", dict(n=ints(ctypes.c_int, [MAX_PAIRS + 1]))),
               ("more pairs than the pair limit over two groups",
                dict(groups=2, n=ints(ctypes.c_int, [MAX_PAIRS, 1]), idx_a=ptrs("idx_a", 2), idx_b=ptrs("idx_b", 2),
                     offsets=ptrs("offsets", 2), capacity_in=ints(ctypes.c_int64, [4, 4])))]
    for label, changed in clauses:
        rc = _call(lib, "dcn_concat_samples", names, dict(args, **changed), outs)
        assert rc == DCN_E_INVALID, (label, rc)
    assert _untouched(outs, device) == []


def check_workspace_refusals():
    from dcn_hip import _lib
    lib = _lib.get()
    assert lib.dcn_sample_workspace(N, H, W, A, A) > 0 and lib.dcn_sample_workspace(N, H, W, 0, 0) > 0
    for bad in ((0, H, W, A, A), (N, 0, W, A, A), (N, H, 0, A, A), (N, H, W, -1, A), (N, H, W, A, -1)):
        assert lib.dcn_sample_workspace(*bad) == 0, bad
    assert lib.dcn_eval_matches_workspace(N, H, W, A) > 0
    for bad in ((0, H, W, A), (N, 0, W, A), (N, H, 0, A), (N, H, W, 0)):
        assert lib.dcn_eval_matches_workspace(*bad) == 0, bad


# ------------------------------------------------------------------------------------------ b. Python argument errors
def _raises(exc, fragment, fn, *a, **kw):
    with pytest.raises(exc, match=fragment):
        fn(*a, **kw)


MASK_MSG, DEPTH_MSG, IMAGE_MSG = r"mask\w* must be \[", r"depth\w* must be 16-bit integer \[", r"must be uint8 \["
CAMS_MSG, OFFSETS_MSG, SEEDS_MSG = r"cam\w* must be (contiguous )?float32 \[\d+, 50\]", r"must have B \+ 1 = \d+ entries", \
    r"seeds must hold one int64 per pair"
PARAMS_MSG = r"params must be int32 \["
FIRST_IMAGE_MSG = "(%s|%s)" % (IMAGE_MSG, MASK_MSG)           # (image a sets the size its mask is then held against)
DEVICE_MSG = r"MI355X only"


def check_sample_argument_errors(device):
    from dcn_hip import samples
    n, h, w = 2, H, W
    depth, masks, pa, pb = example(n, h, w, seed=3)
    da, db = _t(depth[0].view(np.int16), device), _t(depth[1].view(np.int16), device)
    ma, mb = _t(masks[0], device), _t(masks[1], device)
    rgb = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=device)
    kw = dict(num_matching_attempts=A, sample_matches_only_off_mask=True, num_masked_non_matches_per_match=1,
              num_background_non_matches_per_match=1, use_image_b_mask_inv=True, seeds=[1, 2])
    within = lambda *a, **k: samples.build_within_scene_samples(*a, **dict(kw, **k))
    ok = within(da, db, ma, mb, pa, pb, SMALL_K)
    cams = torch.zeros((n, samples.CAM_FLOATS), dtype=torch.float32, device=device)
    within(da, db, ma, mb, None, None, cameras=cams)
    for bad in (mb[:, :-1], mb[:, :, :-1], mb[:1], mb.view(n, h * w)):
        _raises(ValueError, MASK_MSG, within, da, db, ma, bad, pa, pb, SMALL_K)
    for bad in (da.float(), da.to(torch.int32), da.to(torch.uint8), da[:, :-1], da[:1]):
        _raises(ValueError, DEPTH_MSG, within, bad, db, ma, mb, pa, pb, SMALL_K)
        _raises(ValueError, DEPTH_MSG, within, da, bad, ma, mb, pa, pb, SMALL_K)
    for bad in (rgb.float(), rgb[:, :-1], rgb[:1], rgb[..., :2]):
        _raises(ValueError, FIRST_IMAGE_MSG, within, da, db, ma, mb, pa, pb, SMALL_K, bad, rgb)
        _raises(ValueError, IMAGE_MSG, within, da, db, ma, mb, pa, pb, SMALL_K, rgb, bad)
    _raises(ValueError, "go together", within, da, db, ma, mb, pa, pb, SMALL_K, rgb, None)
    wide = torch.zeros((n, 2 * samples.CAM_FLOATS), dtype=torch.float32, device=device)
    for bad in (cams[:, :-1], cams.double(), cams[:1], wide[:, ::2]):        # (the last: not contiguous)
        _raises(ValueError, CAMS_MSG, within, da, db, ma, mb, None, None, cameras=bad)
    for bad in (np.eye(2), np.stack([SMALL_K] * (n + 1))):
        _raises(ValueError, r"K must be \[3, 3\] or \[", within, da, db, ma, mb, pa, pb, bad)
    _raises(ValueError, r"pose_a must be \[", within, da, db, ma, mb, pa[:1], pb, SMALL_K)
    _raises(ValueError, r"pose_b must be \[", within, da, db, ma, mb, pa, pb[:, :3], SMALL_K)
    _raises(ValueError, "must be >= 1", within, da, db, ma, mb, pa, pb, SMALL_K, num_matching_attempts=0)
    across = lambda *a, **k: samples.build_across_scene_samples(*a, **dict(dict(num_samples=5, seeds=[1, 2]), **k))
    across(ma, mb)
    _raises(ValueError, MASK_MSG, across, ma, mb[:, :-1])
    _raises(ValueError, "num_samples must be >= 1", across, ma, mb, num_samples=0)
    uv = (torch.tensor([1, 2, 3], device=device), torch.tensor([0, 1, 2], device=device))
    ckw = dict(num_masked_non_matches_per_match=1, num_background_non_matches_per_match=1, use_image_b_mask_inv=True, seeds=[1, 2])
    complete = lambda *a, **k: samples.complete_samples(*a, **dict(ckw, **k))
    complete(uv, uv, [0, 2, 3], ma, mb)
    _raises(ValueError, MASK_MSG, complete, uv, uv, [0, 2, 3], ma, mb[:1])
    for bad in ([0, 3], [0, 1, 2, 3], torch.tensor([0, 3]), torch.zeros((2, 2), dtype=torch.int64)):
        _raises(ValueError, OFFSETS_MSG, complete, uv, uv, bad, ma, mb)
    _raises(ValueError, "uv_a must be int64", complete, (uv[0].int(), uv[1].int()), uv, [0, 2, 3], ma, mb)
    _raises(ValueError, "all four lists of one length", complete, uv, (uv[0][:2], uv[1][:2]), [0, 2, 3], ma, mb)
    _raises(TypeError, "pixel lists must be int64 or float32", complete, uv, (uv[0].double(), uv[1].double()), [0, 2, 3], ma, mb)
    _raises(ValueError, "must be >= 1", complete, uv, uv, [0, 2, 3], ma, mb, num_masked_non_matches_per_match=0)
    # seeds, augmentation records and replay streams: the three builders
    calls = ((within, (da, db, ma, mb, pa, pb, SMALL_K)), (across, (ma, mb)), (complete, (uv, uv, [0, 2, 3], ma, mb)))
    for fn, a in calls:
        for bad in ([1], [1, 2, 3], torch.zeros((n + 1,), dtype=torch.int64)):
            _raises(ValueError, SEEDS_MSG, fn, *a, seeds=bad)
        for bad in (np.zeros((2 * n, 15), np.int32), np.zeros((n, 16), np.int32), np.zeros((2 * n * 16,), np.int32)):
            _raises(ValueError, "aug_" + PARAMS_MSG, fn, *a, aug_params=bad)
        _raises(ValueError, "needs one entry per pair", fn, *a, seeds=None, draws={"cand": [np.zeros(3, np.float32)]})
        _raises(ValueError, "unknown draw sites", fn, *a, seeds=None, draws={"candidates": [None] * n})
    # what is converted, not refused: a bool or float mask, seeds of any integer type, records as a nested list
    same = across(ma.bool(), mb.float(), seeds=torch.tensor([1, 2], dtype=torch.int32), aug_params=[[0] * 16] * (2 * n))
    ref = across(ma, mb, aug_params=np.zeros((2 * n, 16), np.int32))
    assert torch.equal(same.idx_a, ref.idx_a) and torch.equal(same.idx_b, ref.idx_b) and torch.equal(same.seeds, ref.seeds)
    assert ok.seeds.tolist() == [1, 2] and ok.seeds.dtype == torch.int64
    if torch.device(device).type == "cuda":                       # a host tensor where the library takes device memory
        _raises(RuntimeError, DEVICE_MSG, within, da, db, ma, mb.cpu(), pa, pb, SMALL_K)
        _raises(RuntimeError, DEVICE_MSG, within, da.cpu(), db, ma, mb, pa, pb, SMALL_K)
        _raises(RuntimeError, DEVICE_MSG, within, da, db, ma, mb, None, None, cameras=cams.cpu())
        _raises(RuntimeError, DEVICE_MSG, across, ma, mb.cpu())
        _raises(RuntimeError, DEVICE_MSG, complete, uv, uv, [0, 2, 3], ma.cpu(), mb.cpu())


def check_evaluate_argument_errors(device):
    from dcn_hip import evaluate, samples
    n, h, w = 2, H, W
    depth, masks, pa, pb = example(n, h, w, seed=3)
    da, db = _t(depth[0].view(np.int16), device), _t(depth[1].view(np.int16), device)
    ma, mb = _t(masks[0], device), _t(masks[1], device)
    cams = _t(np.stack([sc.cams_of(SMALL_K, pa[p], pb[p]) for p in range(n)]).astype(np.float32), device)
    find = lambda *a, **k: evaluate.find_eval_matches(*a, **dict(dict(seeds=[1, 2], order_seeds=[3, 4]), **k))
    ok = find(da, db, ma, cams, M)
    for bad in (da.float(), da.to(torch.int64), da[:, :-1], da[:1]):
        _raises(ValueError, DEPTH_MSG, find, bad, db, ma, cams, M)
        _raises(ValueError, DEPTH_MSG, find, da, bad, ma, cams, M)
    for bad in (cams[:, :-1], cams.double(), cams[:1]):
        _raises(ValueError, CAMS_MSG, find, da, db, ma, bad, M)
    # camera rows that are not contiguous: the evaluation copies them (the sample builder refuses them, above)
    wide = torch.zeros((n, 2 * samples.CAM_FLOATS), dtype=torch.float32, device=device)
    wide[:, ::2] = cams
    strided = find(da, db, ma, wide[:, ::2], M)
    assert not wide[:, ::2].is_contiguous() and torch.equal(strided.u_b, ok.u_b) and torch.equal(strided.offsets, ok.offsets)
    for bad in ([1], [1, 2, 3]):
        _raises(ValueError, r"^" + SEEDS_MSG, find, da, db, ma, cams, M, seeds=bad)
        _raises(ValueError, "order_" + SEEDS_MSG, find, da, db, ma, cams, M, order_seeds=bad)
    for bad in (np.zeros((n, M + 1), np.int64), np.zeros((n + 1, M), np.int64), np.zeros((n * M,), np.int64),
                torch.zeros((n, M - 1), dtype=torch.int32)):
        _raises(ValueError, r"match_order must be \[", find, da, db, ma, cams, M, match_order=bad)
    _raises(ValueError, "needs one entry per pair", find, da, db, ma, cams, M, seeds=None, draws={"cand": [None]})
    _raises(ValueError, "num_attempts must be 1 .. 4096", find, da, db, ma, cams, M, num_attempts=4097)
    find(da, db, ma, cams, M, match_order=np.zeros((n, M)))         # (a float table is converted)
    res = torch.zeros((n, h, w, 3), device=device)
    rows = (ok.u_a, ok.v_a, ok.u_b, ok.v_b, ok.offsets)
    evaluate.match_statistics_pairs(res, res, mb, da, db, cams, *rows)
    _raises(ValueError, MASK_MSG, evaluate.match_statistics_pairs, res, res, mb[:, :-1], da, db, cams, *rows)
    _raises(ValueError, DEPTH_MSG, evaluate.match_statistics_pairs, res, res, mb, da.float(), db, cams, *rows)
    _raises(ValueError, DEPTH_MSG, evaluate.match_statistics_pairs, res, res, mb, da, db[:1], cams, *rows)
    for bad in (cams[:, :18], cams.double(), cams[:1]):
        _raises(ValueError, CAMS_MSG, evaluate.match_statistics_pairs, res, res, mb, da, db, bad, *rows)
    _raises(ValueError, "offsets must be an int64 tensor of P", evaluate.match_statistics_pairs, res, res, mb, da, db, cams,
            *rows[:4], rows[4][:-1])
    if torch.device(device).type == "cuda":
        _raises(RuntimeError, DEVICE_MSG, find, da, db.cpu(), ma, cams, M)
        _raises(RuntimeError, DEVICE_MSG, find, da, db, ma, cams.cpu(), M)
        _raises(RuntimeError, DEVICE_MSG, evaluate.match_statistics_pairs, res, res, mb.cpu(), da, db, cams, *rows)


def check_frames_argument_errors(device):
    import frames_common as fc
    from dcn_hip import frames
    first, sobj = [0, 2, 4], [0, 1]
    F, h, w = 4, 6, 10
    poses = np.stack([_pose(0, [0.3 * f, 0, 0]) for f in range(F)])
    rgb, depth, mask = (x.to(device) for x in fc.frames_for(F, h, w, 0))
    make = lambda r=rgb, d=depth, m=mask, p=poses, K=None: frames.FrameStore.from_tensors(r, d, m, p, first, sobj, K)
    store = make()
    for bad in (rgb.float(), rgb[:-1], rgb[..., :2], rgb.view(F, h * w, 3)):
        _raises(ValueError, r"rgb " + IMAGE_MSG, make, r=bad)
    for bad in (depth.float(), depth.to(torch.int32), depth[:, :-1], depth[:-1]):
        _raises(ValueError, DEPTH_MSG, make, d=bad)
    for bad in (mask[:, :-1], mask[:-1]):
        _raises(ValueError, MASK_MSG, make, m=bad)
    _raises(ValueError, r"poses must be \[", make, p=poses[:-1])
    for bad in (np.eye(2), np.stack([SMALL_K] * 3)):
        _raises(ValueError, r"K must be \[3, 3\] or \[", make, K=bad)
    assert make(m=mask.bool()).mask.dtype == torch.uint8 and make(d=depth.view(torch.uint16)).depth.dtype == torch.int16
    select = lambda **k: frames.select_frames(store, 2, frames.SINGLE_OBJECT_WITHIN_SCENE, **k)
    select(seeds=[1, 2])
    for bad in ([1], [1, 2, 3]):
        _raises(ValueError, r"^" + SEEDS_MSG, select, seeds=bad)
    words = frames.draw_words(50)
    for bad in (np.zeros((2, words - 1), np.int64), np.zeros((3, words), np.int64), np.zeros((2 * words,), np.int64),
                torch.zeros((1, words), dtype=torch.int32)):
        _raises(ValueError, r"draws must be \[", select, draws=bad)
    select(draws=np.zeros((2, words)))                               # (a float table is converted)
    _raises(ValueError, "must be >= 1", select, num_attempts=0)
    if torch.device(device).type == "cuda":
        _raises(RuntimeError, DEVICE_MSG, make, m=mask.cpu())
        _raises(RuntimeError, DEVICE_MSG, make, d=depth.cpu())


def samples_within_float16(device):
    from dcn_hip import samples
    z = torch.zeros((1, H, W), dtype=torch.int16, device=device)
    samples.build_within_scene_samples(z.view(torch.float16), z, z, z, np.eye(4)[None], np.eye(4)[None], SMALL_K,
                                       num_matching_attempts=4, sample_matches_only_off_mask=True,
                                       num_masked_non_matches_per_match=1, num_background_non_matches_per_match=1,
                                       use_image_b_mask_inv=True)


def check_merge_augment_pairgen_argument_errors(device):
    from dcn_hip import augment, merge, pairgen
    n, h, w = 2, H, W
    g = torch.Generator().manual_seed(1)
    rgb = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g).to(device)
    mask = torch.randint(0, 2, (n, h, w), dtype=torch.uint8, generator=g).to(device)
    uv = (torch.tensor([1, 2, 3], device=device), torch.tensor([0, 1, 2], device=device))
    fg = np.zeros((n, 2), np.int32)
    ms = lambda ims=(rgb,) * 4, mks=(mask,) * 4, offa=(0, 2, 3), offb=(0, 1, 3): merge.merge_synthetic_samples(
        *ims, *mks, uv, uv, uv, uv, offa, offb, foreground=fg)
    ms()
    for k in range(4):
        for bad in (rgb.float(), rgb[:, :-1], rgb[..., :2]) + ((rgb[:1],) if k else ()):
            _raises(ValueError, r"rgb_\w+ " + IMAGE_MSG if k else FIRST_IMAGE_MSG, ms, ims=(rgb,) * k + (bad,) + (rgb,) * (3 - k))
        for bad in (mask[:, :-1], mask[:1]):
            _raises(ValueError, MASK_MSG, ms, mks=(mask,) * k + (bad,) + (mask,) * (3 - k))
    for bad in ((0, 3), (0, 1, 2, 3), torch.tensor([0, 3])):
        _raises(ValueError, "offsets_a " + OFFSETS_MSG, ms, offa=bad)
        _raises(ValueError, "offsets_b " + OFFSETS_MSG, ms, offb=bad)
    ms(mks=(mask.bool(),) * 4, offa=torch.tensor([0, 2, 3], dtype=torch.int32))
    fgd = torch.zeros((n, 2), dtype=torch.int32, device=device)
    _raises(ValueError, MASK_MSG, merge.merge_images, [rgb], [rgb], [mask], [mask[:, :-1]], fgd)
    _raises(ValueError, IMAGE_MSG, merge.merge_images, [rgb], [rgb.float()], [mask], [mask], fgd)
    pairs = lambda r=rgb, rb=rgb, m=mask, mb=mask, **k: augment.augment_image_pairs(r, rb, m, mb, **k)
    pairs(uv_a=uv, offsets=[0, 2, 3])
    for bad in (rgb.float(), rgb[:, :-1], rgb[..., :2]):
        _raises(ValueError, FIRST_IMAGE_MSG, pairs, r=bad)
        _raises(ValueError, IMAGE_MSG, pairs, rb=bad)
    for bad in (mask[:, :-1], mask[:1]):
        _raises(ValueError, MASK_MSG, pairs, m=bad)
        _raises(ValueError, MASK_MSG, pairs, mb=bad)
    for bad in ([0, 3], [0, 1, 2, 3], torch.tensor([0, 3])):
        _raises(ValueError, "offsets " + OFFSETS_MSG, pairs, uv_a=uv, offsets=bad)
    _raises(ValueError, r"offsets \[B \+ 1\] are needed", pairs, uv_a=uv)
    for bad in (torch.zeros((2 * n, 15), dtype=torch.int32), torch.zeros((n, 16), dtype=torch.int32)):
        _raises(ValueError, PARAMS_MSG, pairs, params=bad)
    zeros = torch.zeros((n, augment.PARAM_WORDS), dtype=torch.int32, device=device)
    _raises(ValueError, PARAMS_MSG, augment.augment_images, rgb, mask, zeros.long())
    _raises(ValueError, MASK_MSG, augment.augment_images, rgb, None, zeros)
    pairs(m=mask.bool(), mb=mask.float())
    d2 = torch.zeros((h, w), dtype=torch.int16, device=device)
    cand = torch.zeros(3, dtype=torch.int64, device=device)
    pairgen.find_correspondences(d2, d2, SMALL_K, np.eye(4), np.eye(4), cand, cand)
    for bad in (d2.float(), d2[:-1], d2.view(1, h, w), d2.to(torch.int32)):
        _raises(ValueError, "16-bit", pairgen.find_correspondences, bad, d2, SMALL_K, np.eye(4), np.eye(4), cand, cand)
    # pairgen's own rule is "two [H, W] maps of one shape and 2 bytes per pixel": unlike the batch checkers it takes the bits of
    # a float16 map as they are (pinned here; it is why pairgen keeps its check)
    pairgen.find_correspondences(d2.view(torch.float16), d2, SMALL_K, np.eye(4), np.eye(4), cand, cand)
    _raises(ValueError, DEPTH_MSG, samples_within_float16, device)
    if torch.device(device).type == "cuda":
        _raises(RuntimeError, DEVICE_MSG, ms, mks=(mask.cpu(),) * 4)
        _raises(RuntimeError, DEVICE_MSG, pairs, m=mask.cpu())
        _raises(RuntimeError, DEVICE_MSG, pairgen.find_correspondences, d2.cpu(), d2, SMALL_K, np.eye(4), np.eye(4), cand, cand)


# ------------------------------------------------------------------------------------------------------- c. call sites
def _within(device, n, h, w, attempts, only_off, inv, k1, k2, seed, gen_seed, params):
    from dcn_hip import samples
    depth, masks, pa, pb = example(n, h, w, seed=seed)
    g = torch.Generator(device=device).manual_seed(gen_seed)
    r = samples.build_within_scene_samples(_t(depth[0].view(np.int16), device), _t(depth[1].view(np.int16), device),
                                           _t(masks[0], device), _t(masks[1], device), pa, pb, K_for(h),
                                           num_matching_attempts=attempts, sample_matches_only_off_mask=only_off,
                                           num_masked_non_matches_per_match=k1, num_background_non_matches_per_match=k2,
                                           use_image_b_mask_inv=inv, generator=g, aug_params=params)
    return r, (depth, masks, pa, pb)


def check_uniform_candidates_more_attempts_than_pixels(device):
    """sample_matches_only_off_mask=False and use_image_b_mask_inv=False at 7 x 9 with 400 attempts: the list stride of the
    workspace is the attempt count, the candidates are uniform over the image, the background non-matches too."""
    n, h, w, attempts, k1, k2 = 3, H, W, 400, 2, 3
    params = sc.params_from_flips([True, False, True], [False, True, True])
    r, (depth, masks, pa, pb) = _within(device, n, h, w, attempts, False, False, k1, k2, 7, 5, params)
    sc.check_layout(r)
    assert attempts > h * w and int(r.offsets[1] - r.offsets[0]) > 0
    assert r.max_list_len == attempts * k2 and r.max_pair_len == attempts * (1 + k1 + k2) + h * w
    seeds = r.seeds.cpu().tolist()
    for p in range(n):
        U = lambda site, k, s=seeds[p]: sc.hash_uniform(s, site, k)
        lists, typ = sc.restated_within(depth[0, p], depth[1, p], masks[0, p], masks[1, p], sc.cams_of(K_for(h), pa[p], pb[p]),
                                        params[p, 0] != 0, params[n + p, 0] != 0, attempts, False, k1, k2, False, U)
        sc.check_against_restatement(r, p, lists, typ)


def check_complete_samples_without_matches(device):
    """count = 0: every pair empty, nothing but the -1 tail in the lists."""
    from dcn_hip import samples
    n, h, w = 2, H, W
    _, masks, _, _ = example(n, h, w, seed=4)
    none = torch.zeros(0, dtype=torch.int64, device=device)
    for offsets in ([0, 0, 0], torch.zeros(n + 1, dtype=torch.int64, device=device)):
        r = samples.complete_samples((none, none), (none, none), offsets, _t(masks[0], device), _t(masks[1], device),
                                     num_masked_non_matches_per_match=2, num_background_non_matches_per_match=3,
                                     use_image_b_mask_inv=True, generator=torch.Generator(device=device).manual_seed(1))
        sc.check_layout(r)
        assert r.empty.tolist() == [True] * n and r.type.tolist() == [-1] * n and r.offsets.tolist() == [0] * (4 * n + 1)
        assert int(r.idx_a.numel()) == n * h * w and bool((r.idx_a == -1).all()) and bool((r.idx_b == -1).all())
        assert r.max_list_len == h * w and r.max_pair_len == h * w and r.input_a is None and r.aug_params is None


def order_key(seed, i):
    """csrc/sample_kernels.hip ``order_key``: the hashed key of survivor i in the seeded subsample"""
    s = int(seed) & 0xffffffffffffffff
    k0 = sc._mix32((s & 0xffffffff) ^ 0x2545F491)
    return sc._mix32(sc._mix32((i ^ k0) & 0xffffffff) ^ ((sc._mix32((s >> 32) ^ k0) + 0x9E3779B9) & 0xffffffff))


def restated_eval_matches(depth_a, depth_b, mask_a, cam, attempts, num_matches, U, order=None, order_seed=None):
    """One pair -> ([(u_a, v_a, u_b, v_b)] in row order, total): the candidates of mask a's pixels, the reprojection test, then
    the replayed positions or the ``min(num_matches, total)`` survivors with the smallest hashed keys, in key order."""
    h, w = mask_a.shape
    la = np.flatnonzero(mask_a.reshape(-1))
    kept = []
    for i in range(attempts if la.size else 0):
        px = sc._pick(la, U(0, i))
        pr = sc._project(depth_a.astype(np.uint16), depth_b.astype(np.uint16), cam, px % w, px // w)
        if pr is not None:
            kept.append((px % w, px // w, pr[0], pr[1]))
    k = min(num_matches, len(kept))
    if order is not None:
        return [kept[int(order[e])] for e in range(k)], len(kept)
    ranked = sorted(range(len(kept)), key=lambda e: (order_key(order_seed, e), e))
    return [kept[e] for e in ranked[:k]], len(kept)


def check_eval_matches_more_attempts_than_pixels(device, replay):
    """find_eval_matches at 7 x 9 with 100 attempts (the list stride is the attempt count).  The float projections are compared
    as check_matches of evaluate_common compares them: 1e-4 px, and the pixel they truncate to exactly."""
    from dcn_hip import evaluate, samples
    n, h, w, attempts, num = 3, H, W, 100, 12
    depth, masks, pa, pb = example(n, h, w, seed=7)
    masks[0, 1] = 0                                                  # pair 1: no candidates at all
    cams = np.stack([sc.cams_of(SMALL_K, pa[p], pb[p]) for p in range(n)]).astype(np.float32)
    da, db = _t(depth[0].view(np.int16), device), _t(depth[1].view(np.int16), device)
    rng = np.random.RandomState(2)
    if replay:
        streams = [rng.rand(attempts).astype(np.float32) for _ in range(n)]
        first = evaluate.find_eval_matches(da, db, _t(masks[0], device), _t(cams, device), num, num_attempts=attempts,
                                           draws={"cand": streams}, order_seeds=[0] * n)
        totals = first.totals.cpu().tolist()
        order = np.full((n, num), -1, np.int64)
        for p in range(n):
            k = min(num, totals[p])
            order[p, :k] = rng.permutation(totals[p])[:k]
        m = evaluate.find_eval_matches(da, db, _t(masks[0], device), _t(cams, device), num, num_attempts=attempts,
                                       draws={"cand": streams}, match_order=order)
        assert m.order_seeds is None
        U = [lambda site, k, s=streams[p]: np.float32(s[k]) for p in range(n)]
        how = [dict(order=order[p]) for p in range(n)]
    else:
        g = torch.Generator(device=device).manual_seed(4)
        m = evaluate.find_eval_matches(da, db, _t(masks[0], device), _t(cams, device), num, num_attempts=attempts, generator=g)
        g = torch.Generator(device=device).manual_seed(4)
        seeds, order_seeds = (samples.draw_seeds(n, torch.device(device), g).cpu().tolist() for _ in range(2))
        assert m.order_seeds.cpu().tolist() == order_seeds          # (the candidates' seeds are drawn first, then the order's)
        U = [lambda site, k, s=seeds[p]: sc.hash_uniform(s, site, k) for p in range(n)]
        how = [dict(order_seed=order_seeds[p]) for p in range(n)]
    assert int(m.status.cpu()[0]) == 0
    off = m.offsets.cpu().tolist()
    ua, va, ub, vb = (x.cpu().numpy() for x in (m.u_a, m.v_a, m.u_b, m.v_b))
    assert ua.size == n * min(num, attempts) and off[0] == 0
    for p in range(n):
        rows, total = restated_eval_matches(depth[0, p], depth[1, p], masks[0, p], cams[p], attempts, num, U[p], **how[p])
        assert int(m.totals[p]) == total and off[p + 1] - off[p] == len(rows) == min(num, total), (p, total)
        sl = slice(off[p], off[p + 1])
        assert ua[sl].tolist() == [r[0] for r in rows] and va[sl].tolist() == [r[1] for r in rows], p
        np.testing.assert_allclose(ub[sl], [r[2] for r in rows], rtol=0, atol=1e-4)
        np.testing.assert_allclose(vb[sl], [r[3] for r in rows], rtol=0, atol=1e-4)
        assert ub[sl].astype(np.int64).tolist() == [int(r[2]) for r in rows]
        assert vb[sl].astype(np.int64).tolist() == [int(r[3]) for r in rows]
    assert int(m.totals[0]) > num and int(m.totals[1]) == 0          # a pair that is subsampled, and one without matches
    assert (ua[off[-1]:] == -1).all() and (va[off[-1]:] == -1).all() and (ub[off[-1]:] == 0).all() and (vb[off[-1]:] == 0).all()


def _same_lists(joined, p, sb, q):
    for a, b in zip(sc.batch_lists(joined, p), sc.batch_lists(sb, q)):
        assert np.array_equal(a, b), (p, q)


def check_concat_of_one_and_of_two(device, h, w):
    """concat_sample_batches of ONE batch is that batch (compacted); a within-scene batch joined with an across-scene batch
    keeps every pair's four lists, types, seeds, records and bounds."""
    from dcn_hip import samples
    attempts = 400 if h * w < 400 else 120
    params = sc.params_from_flips([True, False], [False, True])
    within, (depth, masks, pa, pb) = _within(device, 2, h, w, attempts, True, True, 2, 3, 7, 5, params)
    g = torch.Generator(device=device).manual_seed(6)
    across = samples.build_across_scene_samples(_t(masks[0, :1], device), _t(masks[0, :1], device), num_samples=25, generator=g,
                                                data_type=samples.DIFFERENT_OBJECT)
    one = samples.concat_sample_batches([within])
    sc.check_layout(one)
    for k in ("idx_a", "idx_b", "offsets", "empty", "type", "seeds", "aug_params"):
        assert torch.equal(getattr(one, k), getattr(within, k)), k
    assert int(one.status.cpu()[0]) == 0 and one.input_a is None and one.mask_a is None
    assert (one.max_list_len, one.max_pair_len) == (within.max_list_len, within.max_pair_len)
    joined = samples.concat_sample_batches([within, across])
    sc.check_layout(joined)
    assert joined.idx_a.numel() == within.idx_a.numel() + across.idx_a.numel()
    _same_lists(joined, 0, within, 0)
    _same_lists(joined, 1, within, 1)
    _same_lists(joined, 2, across, 0)
    assert torch.equal(joined.type, torch.cat([within.type, across.type])) and joined.type.tolist()[1:] == [0, 2]
    assert torch.equal(joined.empty, torch.cat([within.empty, across.empty])) and joined.empty.tolist()[1:] == [False, False]
    assert int(joined.offsets[8] - joined.offsets[4]) > 0 and int(joined.offsets[12] - joined.offsets[11]) == 25
    assert torch.equal(joined.seeds, torch.cat([within.seeds, across.seeds]))
    assert torch.equal(joined.aug_params, torch.cat([within.aug_params[:2], across.aug_params[:1], within.aug_params[2:],
                                                     across.aug_params[1:]]))
    assert (joined.max_list_len, joined.max_pair_len) == (within.max_list_len, within.max_pair_len)
    assert joined.input_a is None and joined.mask_b is None
