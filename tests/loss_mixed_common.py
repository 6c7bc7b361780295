"""Shared by tests/test_emu_loss_mixed.py (host emulation, "cpu") and tests/test_gpu_loss_mixed.py (gfx950, "cuda"); not a test
module.  The small helpers of the mixed-loss tests, and the bodies of the checks that take every lane-dispatch arm of
csrc/loss_kernels.hip (4 / 8 / 16 / 32 lanes per pixel pair, and 32 lanes looping over more than 32 components) through every
launch site of the loss."""
import contextlib
import functools

import numpy as np
import torch

from helpers import rel_err

WITHIN, ACROSS, DIFFERENT, MULTI, SYNTHETIC = 0, 1, 2, 3, 4


def pcl_for(H, W, cfg=None):
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    return PixelwiseContrastiveLoss([H, W], cfg or synth.LOSS_CONFIG)


def make_lists(code, HW, sizes, g):
    """One 8-tuple: within-scene compositions fill all four lists (match, masked, background, blind), the across-scene and
    different-object ones only the blind list."""
    r = lambda n: torch.randint(0, HW, (n,), generator=g)
    if code in (WITHIN, MULTI, SYNTHETIC):
        pm, pk, pg, pb = sizes
        return (r(pm), r(pm), r(pk), r(pk), r(pg), r(pg), r(pb) if pb else None, r(pb) if pb else None)
    return (None, None, None, None, None, None, r(sizes[3]), r(sizes[3]))


def device_lists(pairs, types, tail=37, max_list_len=None, max_pair_len=None, device="cpu"):
    """The lists of ``pairs`` as a device-built batch would hold them: concatenated, a -1 tail up to the capacity, device
    offsets and types, and generous bounds (several workgroups past the longest list)."""
    from dcn_hip import loss as K
    pl = K.PairLists.from_lists(pairs, device)
    fill = torch.full((tail,), -1, dtype=torch.int64, device=device)
    ia = torch.cat([pl.idx_a[:pl.total], fill])
    ib = torch.cat([pl.idx_b[:pl.total], fill])
    per_pair = max(pl.offsets_host[4 * p + 4] - pl.offsets_host[4 * p] for p in range(pl.num_pairs))
    return K.DeviceLists(ia, ib, pl.offsets_dev, torch.tensor(types, dtype=torch.int32, device=device),
                         2 * pl.max_len + 1500 if max_list_len is None else max_list_len,
                         per_pair + 1500 if max_pair_len is None else max_pair_len)


def descriptors(B, HW, D, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: ((torch.rand(B, HW, D, generator=g) * 2 - 1) * 0.6 / D ** 0.5).requires_grad_(True)
    return mk(), mk()


def run_mixed(pcl, A, B, lists):
    from dense_correspondence.loss_functions import loss_composer
    A = A.detach().clone().requires_grad_(True)
    B = B.detach().clone().requires_grad_(True)
    loss, terms, hard, nv = loss_composer.get_loss_mixed(pcl, A, B, lists)
    loss.backward()
    return dict(loss=loss.detach(), terms=terms, hard=hard, num_valid=int(nv), gA=A.grad, gB=B.grad, status=int(pcl.last_status))


def run_batched(pcl, code, A, B, pairs):
    from dense_correspondence.loss_functions import loss_composer
    A = A.detach().clone().requires_grad_(True)
    B = B.detach().clone().requires_grad_(True)
    loss, terms, hard = loss_composer.get_loss_batched(pcl, code, A, B, pairs)
    loss.backward()
    return dict(loss=loss.detach(), terms=terms, hard=hard, gA=A.grad, gB=B.grad, status=int(pcl.last_status))


# ------------------------------------------------------------------------------------------------ every arm at every site
# The launch sites and the descriptor widths D of {3, 8, 16, 32, 40} (one per arm) that the rest of the suite takes through
# them, traced on the host emulation by recording (entry point, D) of every call of a whole run:
#   one-type forward, gather backward     3, 16, 40   (test_emu_loss.py: SAVE_PAIR_RECORDS off on the goldens and at D = 40)
#   forward + save, exact backward        all five    (test_emu_loss.py::test_batched_ragged_lists_vs_oracle)
#   saved backward (fp32 atomics)         3, 16       (test_emu_round6.py: EXACT_BACKWARD off on the goldens)
#   mixed forward, mixed exact backward   3, 16       (test_emu_loss_mixed.py)
#   mixed saved backward (fp32 atomics)   3           (test_emu_loss_mixed.py::test_all_pairs_empty)
# The cases below are the rest.  "gather": forward without records + gathering backward; "saved": forward + save and the fp32
# saved backward; the mixed cases: the mixed forward and the exact / fp32 saved backward.
ONE_TYPE_CASES = [("gather", 8), ("gather", 32), ("saved", 8), ("saved", 32), ("saved", 40)]
MIXED_CASES = [("exact", 8), ("exact", 32), ("exact", 40), ("saved", 8), ("saved", 16), ("saved", 32), ("saved", 40)]
DISPATCH_SWITCHES = {"gather": dict(SAVE_PAIR_RECORDS=False), "saved": dict(SAVE_PAIR_RECORDS=True, EXACT_BACKWARD=False),
                     "exact": dict(SAVE_PAIR_RECORDS=True, EXACT_BACKWARD=True)}
DISPATCH_P, DISPATCH_H, DISPATCH_W = 2, 6, 8
DISPATCH_SIZES = [(30, 40, 24, 0), (25, 36, 48, 20)]       # (match, masked, background, blind): pair 0 has no blind list


@contextlib.contextmanager
def loss_switches(**kw):
    from dcn_hip import loss as K
    old = {k: getattr(K, k) for k in kw}
    for k, v in kw.items():
        setattr(K, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(K, k, v)


@functools.lru_cache(maxsize=None)
def dispatch_case(D):
    """-> (A, B, pairs, oracle) on the host, once per D: two within-scene pairs on a 6 x 8 image, and oracle/loss_oracle.py's
    per-pair terms, mean loss and gradient maps for them."""
    from oracle import loss_oracle, synth
    HW = DISPATCH_H * DISPATCH_W
    g = torch.Generator().manual_seed(41 + D)
    pairs = [make_lists(WITHIN, HW, s, g) for s in DISPATCH_SIZES]
    A, B = descriptors(DISPATCH_P, HW, D, 43 + D)
    opcl = loss_oracle.PixelwiseContrastiveLoss([DISPATCH_H, DISPATCH_W], synth.LOSS_CONFIG)
    e = torch.tensor([-1])
    terms, total = [], 0
    for p in range(DISPATCH_P):
        out = loss_oracle.get_loss(opcl, torch.tensor([WITHIN]), A[p:p + 1], B[p:p + 1], *[e if x is None else x for x in pairs[p]])
        terms.append([float(o.detach().sum()) for o in out])
        total = total + out[0]
    (total / DISPATCH_P).backward()
    oracle = dict(loss=float(total) / DISPATCH_P, terms=np.array(terms), gA=A.grad.clone(), gB=B.grad.clone())
    return A.detach(), B.detach(), pairs, oracle


def _assert_matches_oracle(got, oracle, rtol, atol, grad_tol):
    assert got["status"] == 0 and oracle["loss"] > 0
    np.testing.assert_allclose(got["terms"].cpu().numpy(), oracle["terms"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(float(got["loss"]), oracle["loss"], rtol=rtol, atol=atol)
    assert rel_err(got["gA"].cpu(), oracle["gA"]) < grad_tol and rel_err(got["gB"].cpu(), oracle["gB"]) < grad_tol


def _on(device, pairs):
    return [tuple(None if x is None else x.to(device) for x in lists) for lists in pairs]


def check_one_type_dispatch(site, D, device, rtol, atol, grad_tol):
    A, B, pairs, oracle = dispatch_case(D)
    with loss_switches(**DISPATCH_SWITCHES[site]):
        got = run_batched(pcl_for(DISPATCH_H, DISPATCH_W), WITHIN, A.to(device), B.to(device), _on(device, pairs))
    _assert_matches_oracle(got, oracle, rtol, atol, grad_tol)


def check_mixed_dispatch(site, D, device, rtol, atol, grad_tol):
    """... and the one-type call's bits for a one-type batch: the forward outputs always, the gradient maps where the
    accumulation does not depend on the order (the exact backward)."""
    A, B, pairs, oracle = dispatch_case(D)
    A, B, pairs = A.to(device), B.to(device), _on(device, pairs)
    pcl = pcl_for(DISPATCH_H, DISPATCH_W)
    with loss_switches(**DISPATCH_SWITCHES[site]):
        got = run_mixed(pcl, A, B, device_lists(pairs, [WITHIN] * DISPATCH_P, device=device))
        one = run_batched(pcl, WITHIN, A, B, pairs)
    assert got["num_valid"] == DISPATCH_P
    _assert_matches_oracle(got, oracle, rtol, atol, grad_tol)
    for k in ("loss", "terms", "hard") + (("gA", "gB") if site == "exact" else ()):
        assert torch.equal(got[k], one[k]), k
