"""Shared by test_emu_bn_bwd_lean.py (host emulation) and test_gpu_bn_bwd_lean.py (MI355X); not a test module.

The lean instances of the batch-norm backward kernels (DCN_BN_BWD_LEAN, csrc/elementwise_kernels.hip) differ from the
full-width ones in their instruction schedule only, so everything dcn_bn_backward_full writes must be equal BIT FOR BIT
with the switch at 1 and at 0: dx (fp32, hl32 image, pixel-blocked image), g_out, dgamma, dbeta, the k1 / k2 / k3 coefficients
and the abs-max word.  No tolerance anywhere."""
import itertools

import torch

OUT_MODES = ("plain", "blocked", "hl_only", "hl_blocked_keep")   # which images of dx the apply pass writes
MASK_MODES = ("bytes", "relu_out", "none")


def make_inputs(C, rows, groups, seed):
    g = torch.Generator().manual_seed(seed)
    n = rows * C
    t = {"dy": torch.randn(n, generator=g), "dy2": 0.5 * torch.randn(n, generator=g), "x": 3.0 * torch.randn(n, generator=g) + 0.7,
         "relu_out": torch.randn(n, generator=g), "mask": torch.randint(0, 16, (n // 4,), generator=g, dtype=torch.uint8),
         "gamma": 1.0 + 0.3 * torch.randn(C, generator=g)}
    stats = torch.randn(groups, 4, C, generator=g)
    stats[:, 3] = 0.2 + stats[:, 3].abs()   # invstd > 0
    t["stats"] = stats.reshape(-1).contiguous()
    return t


def run_once(L, dev, inp, C, rows, groups, out_mode, mask_mode, with_dy2, with_gout):
    """One dcn_bn_backward_full call; returns {name: CPU tensor of the raw bytes} of everything it wrote."""
    lib = L.get()
    d = {k: v.to(dev) for k, v in inp.items()}
    u8 = lambda nbytes: torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    blocked = out_mode != "plain"
    out = {"dgamma": u8(4 * C), "dbeta": u8(4 * C)}
    if out_mode != "hl_only":
        out["dx"] = u8(4 * rows * C)
    if with_gout:
        out["g_out"] = u8(4 * rows * C)
    if out_mode in ("blocked", "hl_blocked_keep"):
        out["dq"] = u8(4 * C * ((rows + 3) // 4) * 4)
    if out_mode in ("hl_only", "hl_blocked_keep"):
        out["hl"] = u8(4 * rows * C)
    absmax = torch.zeros(1, dtype=torch.float32, device=dev) if blocked else None
    ws_bytes = lib.dcn_bn_backward_full_workspace(rows, C, groups)
    assert ws_bytes > 0
    ws = u8(ws_bytes)
    P = lambda t: L.ptr(t) if t is not None else None
    rc = lib.dcn_bn_backward_full(P(d["dy"]), P(d["dy2"]) if with_dy2 else None, P(d["relu_out"]) if mask_mode == "relu_out" else None,
                                  P(d["mask"]) if mask_mode == "bytes" else None, P(d["x"]), P(d["stats"]), P(d["gamma"]), C, rows,
                                  groups, P(out["dgamma"]), P(out["dbeta"]), P(out.get("dx")), P(out.get("g_out")), P(absmax),
                                  P(out.get("dq")), P(out.get("hl")), 1 if out_mode == "hl_blocked_keep" else 0, P(ws), L.stream_ptr())
    assert rc == 0, rc
    if dev != "cpu":
        torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res["k123"] = ws[ws_bytes - 4 * groups * 3 * C:].cpu()
    if absmax is not None:
        res["absmax"] = absmax.view(torch.uint8).cpu()
    return res


def combos():
    """Every output mode with every mask mode, with and without dy2; g_out alternates so that every output mode and every
    mask mode is seen with and without it."""
    for i, (om, mm, d2) in enumerate(itertools.product(OUT_MODES, MASK_MODES, (False, True))):
        yield om, mm, d2, (i + i // 6) % 2 == 0


def check_lean_equals_full(L, dev, set_env, C, rows, groups, repeat=False, only=None):
    """only: indices into combos() (a large shape runs a few of them)"""
    if C % 32 != 0:
        raise AssertionError("the hl32 image needs C % 32 == 0")
    inp = make_inputs(C, rows, groups, seed=C + rows)
    seen = set()
    for i, (om, mm, d2, go) in enumerate(combos()):
        if only is not None and i not in only:
            continue
        set_env(DCN_BN_BWD_LEAN=0)
        full = run_once(L, dev, inp, C, rows, groups, om, mm, d2, go)
        set_env(DCN_BN_BWD_LEAN=1)
        lean = run_once(L, dev, inp, C, rows, groups, om, mm, d2, go)
        assert full.keys() == lean.keys()
        for k in full:
            assert torch.equal(full[k], lean[k]), (k, om, mm, d2, go, C, rows, groups)
        # the call does something: the statistics are written (not the 0x5A fill) and finite
        assert torch.isfinite(lean["dgamma"].view(torch.float32)).all() and not (lean["dgamma"] == 0x5A).all()
        if repeat and (om, mm) not in seen:   # the same launch again: the same bits (fixed-order reductions)
            again = run_once(L, dev, inp, C, rows, groups, om, mm, d2, go)
            for k in lean:
                assert torch.equal(again[k], lean[k]), ("repeat", k, om, mm, d2, go)
        seen.add((om, mm))
