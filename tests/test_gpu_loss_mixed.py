"""The loss on device-built batches on the MI355X (dcn_contrastive_loss_mixed_*, dcn_concat_samples): BASELINE config-2 list
sizes (B = 4, 5000 / 2500 / 2500 pairs, 640 x 480) at D = 3 and D = 16 against a float64 torch statement on the device and
against get_loss_batched, run-to-run bit reproducibility of the exact backward, no host synchronization from the frame store
to the optimizer step, and one end-to-end step with an empty pair in a batch of mixed types."""
import numpy as np
import pytest
import torch

import loss_mixed_common as mc
from helpers import rel_err, use_gfx950_library

pytestmark = pytest.mark.gpu

H, W = 480, 640
TOL = 1e-4                                        # test_gpu_parity.py's tolerance for the loss kernels against the oracle
WITHIN, ACROSS, DIFFERENT, MULTI = 0, 1, 2, 3
PM, PK, PG, PB = 5000, 2500, 2500, 3000


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.fixture
def exact(monkeypatch):
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", True)


def pcl_for():
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    return PixelwiseContrastiveLoss([H, W], synth.LOSS_CONFIG)


def make_lists(code, g):
    r = lambda n: torch.randint(0, H * W, (n,), generator=g, device="cuda")
    if code in (WITHIN, MULTI):
        return (r(PM), r(PM), r(PK), r(PK), r(PG), r(PG), r(PB), r(PB))
    return (None, None, None, None, None, None, r(PB), r(PB))


def device_lists(pairs, types, tail=1000):
    from dcn_hip import loss as K
    pl = K.PairLists.from_lists(pairs, "cuda")
    fill = torch.full((tail,), -1, dtype=torch.int64, device="cuda")
    return K.DeviceLists(torch.cat([pl.idx_a[:pl.total], fill]), torch.cat([pl.idx_b[:pl.total], fill]), pl.offsets_dev,
                         torch.tensor(types, dtype=torch.int32, device="cuda"), 2 * pl.max_len, 3 * (PM + PK + PG + PB))


def descriptors(B, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda: ((torch.rand(B, H * W, D, generator=g, device="cuda") * 2 - 1) * 0.6 / D ** 0.5)
    return mk(), mk()


def run_mixed(A, B, lists):
    from dense_correspondence.loss_functions import loss_composer
    pcl = pcl_for()
    A = A.detach().clone().requires_grad_(True)
    B = B.detach().clone().requires_grad_(True)
    loss, terms, hard, nv = loss_composer.get_loss_mixed(pcl, A, B, lists)
    loss.backward()
    return dict(loss=loss.detach(), terms=terms, hard=hard, num_valid=int(nv), gA=A.grad, gB=B.grad, status=int(pcl.last_status))


def run_batched(code, A, B, pairs):
    from dense_correspondence.loss_functions import loss_composer
    A = A.detach().clone().requires_grad_(True)
    B = B.detach().clone().requires_grad_(True)
    loss, terms, hard = loss_composer.get_loss_batched(pcl_for(), code, A, B, pairs)
    loss.backward()
    return dict(loss=loss.detach(), terms=terms, hard=hard, gA=A.grad, gB=B.grad)


def float64_pair_loss(code, a, b, lists):
    """One pair's loss in float64 torch on the device (loss_composer.py:70-212 with training.yaml's weights of 1 and
    scale_by_hard_negatives): a, b [HW, D] float64 leaves."""
    M = 0.5

    def hinge(ia, ib, invert=False):
        d = (a[ia] - b[ib]).norm(dim=1)
        l = torch.clamp(d - M if invert else M - d, min=0) ** 2
        return l.sum(), int((l != 0).sum())
    if code in (WITHIN, MULTI):
        match = ((a[lists[0]] - b[lists[1]]) ** 2).sum(1).mean()
        sk, hk = hinge(lists[2], lists[3])
        sg, hg = hinge(lists[4], lists[5])
        return match + (sk + sg) / max(hk + hg, 1)
    s, h = hinge(lists[6], lists[7], invert=code == ACROSS)
    return s / max(h, 1)


def check_against_float64(got, A, B, pairs, types):
    A64 = A.double().requires_grad_(True)
    B64 = B.double().requires_grad_(True)
    valid = [p for p, t in enumerate(types) if t >= 0]
    per = {p: float64_pair_loss(types[p], A64[p], B64[p], pairs[p]) for p in valid}
    total = sum(per.values()) / max(len(valid), 1)
    total.backward()
    for p in valid:
        assert abs(float(got["terms"][p, 0]) - float(per[p])) <= TOL * abs(float(per[p])), (p, types[p])
    assert abs(float(got["loss"]) - float(total)) <= TOL * abs(float(total))
    assert rel_err(got["gA"].cpu(), A64.grad.cpu()) < TOL and rel_err(got["gB"].cpu(), B64.grad.cpu()) < TOL


@pytest.mark.parametrize("D", [3, 16])
@pytest.mark.parametrize("code", [WITHIN, DIFFERENT, ACROSS], ids=["within_scene", "different_object", "across_scene"])
def test_uniform_type_at_config2_sizes(code, D, exact):
    g = torch.Generator(device="cuda").manual_seed(10 + code)
    pairs = [make_lists(code, g) for _ in range(4)]
    A, B = descriptors(4, D, 3)
    got = run_mixed(A, B, device_lists(pairs, [code] * 4))
    ref = run_batched(code, A, B, pairs)
    torch.cuda.synchronize()
    assert got["status"] == 0 and got["num_valid"] == 4 and float(got["loss"]) > 0
    for k in ("loss", "terms", "hard", "gA", "gB"):
        assert torch.equal(got[k], ref[k]), k
    check_against_float64(got, A, B, pairs, [code] * 4)


@pytest.mark.parametrize("D", [3, 16])
def test_mixed_types_and_an_empty_pair_at_config2_sizes(D, exact):
    types = [WITHIN, DIFFERENT, ACROSS, MULTI]
    g = torch.Generator(device="cuda").manual_seed(20)
    pairs = [make_lists(t, g) for t in types]
    A, B = descriptors(4, D, 4)
    got = run_mixed(A, B, device_lists(pairs, types))
    torch.cuda.synchronize()
    assert got["status"] == 0 and got["num_valid"] == 4
    for p, t in enumerate(types):
        one = run_batched(t, A[p:p + 1], B[p:p + 1], [pairs[p]])
        assert torch.equal(got["terms"][p], one["terms"][0]), p
    check_against_float64(got, A, B, pairs, types)
    # pair 1 left out: the other three as a batch of their own, bit for bit; its rows and gradient slices exactly zero
    types[1] = -1
    got = run_mixed(A, B, device_lists(pairs, types))
    keep = [0, 2, 3]
    three = run_mixed(A[keep], B[keep], device_lists([pairs[p] for p in keep], [types[p] for p in keep]))
    torch.cuda.synchronize()
    assert got["status"] == 0 and got["num_valid"] == 3
    assert torch.equal(got["loss"], three["loss"]) and torch.equal(got["terms"][keep], three["terms"])
    assert torch.equal(got["gA"][keep], three["gA"]) and torch.equal(got["gB"][keep], three["gB"])
    assert not got["terms"][1].any() and not got["gA"][1].any() and not got["gB"][1].any()
    check_against_float64(got, A, B, pairs, types)
    none = run_mixed(A, B, device_lists(pairs, [-1] * 4))
    assert none["num_valid"] == 0 and float(none["loss"]) == 0.0 and not none["gA"].any() and not none["gB"].any()


def test_exact_backward_is_bit_reproducible_with_shuffled_lists(exact):
    """The same pixel pairs in another order within every list (and so in other workgroups): the integer accumulation makes
    the gradient maps independent of it, and a repeated call gives the same bits."""
    types = [WITHIN, DIFFERENT, ACROSS, WITHIN]
    g = torch.Generator(device="cuda").manual_seed(30)
    pairs = [make_lists(t, g) for t in types]
    A, B = descriptors(4, 16, 5)
    first = run_mixed(A, B, device_lists(pairs, types))
    again = run_mixed(A, B, device_lists(pairs, types))
    shuffled = []
    for lists in pairs:
        out = list(lists)
        for t in range(4):
            if lists[2 * t] is not None:
                perm = torch.randperm(lists[2 * t].numel(), generator=g, device="cuda")
                out[2 * t], out[2 * t + 1] = lists[2 * t][perm], lists[2 * t + 1][perm]
        shuffled.append(tuple(out))
    other = run_mixed(A, B, device_lists(shuffled, types))
    torch.cuda.synchronize()
    assert torch.equal(first["gA"], again["gA"]) and torch.equal(first["gB"], again["gB"])
    assert torch.equal(first["loss"], again["loss"]) and torch.equal(first["hard"], other["hard"])
    assert torch.equal(first["gA"], other["gA"]) and torch.equal(first["gB"], other["gB"])
    assert float(first["gA"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ every arm at every site
# (the cases of tests/test_emu_loss_mixed.py on the device, at this file's tolerance)
@pytest.mark.parametrize("site,D", mc.ONE_TYPE_CASES)
def test_one_type_launch_sites_at_the_remaining_descriptor_widths(site, D):
    mc.check_one_type_dispatch(site, D, "cuda", rtol=TOL, atol=0, grad_tol=TOL)


@pytest.mark.parametrize("site,D", mc.MIXED_CASES)
def test_mixed_launch_sites_at_the_remaining_descriptor_widths(site, D):
    mc.check_mixed_dispatch(site, D, "cuda", rtol=TOL, atol=0, grad_tol=TOL)


# ------------------------------------------------------------------------------------------------ frame store -> optimizer step
def _mixed_config():
    from test_gpu_frames import CFG
    return {"training": dict(CFG["training"], data_type_probabilities={
        "SINGLE_OBJECT_WITHIN_SCENE": 2.0, "SINGLE_OBJECT_ACROSS_SCENE": 1.0, "DIFFERENT_OBJECT": 1.0, "MULTI_OBJECT": 0.0,
        "SYNTHETIC_MULTI_OBJECT": 0.0})}


def _training_loop(use_pair_lists):
    """-> step(): one training step from the store; ``use_pair_lists``: the same loop with the host-offsets loss call."""
    import parity_common as pc
    from dcn_hip import frames
    from dcn_hip.optim import Adam
    from dense_correspondence.loss_functions import loss_composer
    from test_gpu_frames import CFG, training_store
    store = training_store()
    cfg = _mixed_config()
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    opt = Adam(dcn.parameters(), lr=1e-4, weight_decay=1e-4)
    pcl = pcl_for()
    g = torch.Generator(device="cuda").manual_seed(7)
    host = np.random.RandomState(7)
    n = 4

    def step():
        opt.zero_grad()
        if use_pair_lists:
            sb, dt, _ = frames.draw_training_batch(store, n, CFG, generator=g, host_rng=host)
        else:
            sb, _, _ = frames.draw_training_batch(store, n, cfg, generator=g, host_rng=host, per_pair_types=True)
        ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
        pa, pb = dcn.process_network_output(ya, n), dcn.process_network_output(yb, n)
        if use_pair_lists:
            loss = loss_composer.get_loss_batched(pcl, dt, pa, pb, sb.pair_lists())[0]
        else:
            loss = loss_composer.get_loss_mixed(pcl, pa, pb, sb.device_lists())[0]
        loss.backward()
        opt.step()
        return loss
    return step


def _sync_mode_honoured():
    try:
        torch.zeros(1, device="cuda").item()
        return False
    except RuntimeError:
        return True


def test_training_step_from_the_store_never_synchronizes():
    """draw_training_batch(per_pair_types=True) -> forward_pair -> get_loss_mixed(device_lists()) -> backward -> optimizer
    step under torch's sync debug mode (or, where the runtime does not honour it, with no device-to-host copy in the profile);
    the same loop with pair_lists() + get_loss_batched trips the check: the host read of the offsets is what is gone."""
    from test_gpu_frames import _d2h_copies
    mixed, parent = _training_loop(False), _training_loop(True)
    for _ in range(2):
        mixed()
        parent()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = _sync_mode_honoured()
        if honoured:
            for _ in range(2):
                loss = mixed()
            with pytest.raises(RuntimeError):
                parent()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        assert _d2h_copies(mixed) == []
        assert _d2h_copies(parent) != []
        loss = mixed()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))


def test_end_to_end_mixed_batch_with_an_empty_pair():
    import parity_common as pc
    from dcn_hip import frames
    from dense_correspondence.loss_functions import loss_composer
    from test_gpu_frames import training_store
    store = training_store()
    cfg = _mixed_config()
    n = 4
    for seed in range(64):                       # the first seed with one empty pair and at least two types among the others
        g = torch.Generator(device="cuda").manual_seed(seed)
        sb, drawn, fbs = frames.draw_training_batch(store, n, cfg, generator=g, host_rng=np.random.RandomState(seed),
                                                    per_pair_types=True)
        types = sb.type.tolist()
        if types.count(-1) == 1 and len(set(types)) >= 3:
            break
    else:
        raise AssertionError("no seed gave a mixed batch with one empty pair")
    assert int(sb.status[0]) == 0 and [t for t in types if t >= 0] == [t for t, d in zip(sorted(drawn), types) if d >= 0]
    e = types.index(-1)
    pcl = pcl_for()
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
    loss, terms, hard, nv = loss_composer.get_loss_mixed(pcl, dcn.process_network_output(ya, n),
                                                         dcn.process_network_output(yb, n), sb.device_lists())
    loss.backward()
    torch.cuda.synchronize()
    assert int(pcl.last_status) == 0 and int(nv) == n - 1
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    assert bool((terms[e] == 0).all()) and bool((hard[e] == 0).all())
    valid = [p for p in range(n) if p != e]
    assert torch.allclose(loss, terms[valid, 0].mean())
    gw = [p.grad for p in dcn.parameters() if p.grad is not None]
    assert gw and all(bool(torch.isfinite(x).all()) for x in gw) and any(float(x.abs().max()) > 0 for x in gw)
