"""Shared by test_emu_bn_bwd_deep.py (host emulation) and test_gpu_bn_bwd_deep.py (MI355X); not a test module.

The deep instances of the batch-norm backward blocked apply pass (DCN_BN_BWD_LEAN_DEPTH, csrc/elementwise_kernels.hip) keep
several rows of a work-item in flight; like the one-row lean instances they differ from the full-width kernel in their schedule
only.  One dcn_bn_backward_full call therefore writes the same bytes -- dx (fp32, hl32 image, pixel-blocked image), g_out,
dgamma, dbeta, k1 / k2 / k3, the abs-max word -- under all three of
    DCN_BN_BWD_LEAN=0                             full width
    DCN_BN_BWD_LEAN=1                             the default depth (the variable is NOT set)
    DCN_BN_BWD_LEAN=1 DCN_BN_BWD_LEAN_DEPTH=1     one row in flight
No tolerance anywhere."""
import os

import torch

from bn_bwd_lean_checks import combos, make_inputs, run_once

# a handful of combos() for the large shapes: every output mode, every mask mode, with and without dy2, with and without g_out
FEW = (1, 6, 9, 12, 13, 17, 19, 22)


def check_three_settings(L, dev, set_env, C, rows, groups, repeat=False, only=None):
    """only: indices into combos().  The settings run one after the other over all the chosen combinations (the depth is set
    last: set_env cannot take a variable away again)."""
    if C % 32 != 0:
        raise AssertionError("the hl32 image needs C % 32 == 0")
    inp = make_inputs(C, rows, groups, seed=C + rows)
    picked = [c for i, c in enumerate(combos()) if only is None or i in only]
    assert picked
    run_all = lambda: [run_once(L, dev, inp, C, rows, groups, *c) for c in picked]
    set_env(DCN_BN_BWD_LEAN=0)
    full = run_all()
    assert "DCN_BN_BWD_LEAN_DEPTH" not in os.environ
    set_env(DCN_BN_BWD_LEAN=1)
    deep = run_all()
    again = run_all() if repeat else None   # the same launches again: the same bits (fixed-order reductions)
    set_env(DCN_BN_BWD_LEAN=1, DCN_BN_BWD_LEAN_DEPTH=1)
    lean = run_all()
    for c, f, d, l in zip(picked, full, deep, lean):
        assert f.keys() == d.keys() == l.keys()
        for k in f:
            assert torch.equal(f[k], d[k]), ("deep != full", k, c, C, rows, groups)
            assert torch.equal(f[k], l[k]), ("depth 1 != full", k, c, C, rows, groups)
        # the call does something: the statistics are written (not the 0x5A fill) and finite
        assert torch.isfinite(d["dgamma"].view(torch.float32)).all() and not (d["dgamma"] == 0x5A).all()
    if repeat:
        for c, d, a in zip(picked, deep, again):
            for k in d:
                assert torch.equal(d[k], a[k]), ("repeat", k, c)
