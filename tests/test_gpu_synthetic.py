"""SYNTHETIC_MULTI_OBJECT samples on the MI355X (csrc/synthetic_kernels.hip): the reference's goldens replayed on the device,
small batches against the host-emulation build's result for the same replay tables, no host synchronization in
draw_training_batch(..., synthetic_multi_object=True), and store -> batch -> forward_pair -> get_loss_mixed -> backward with
an empty sample in the batch."""
import numpy as np
import pytest
import torch

import synthetic_common as yc
from helpers import use_emulation_library, use_gfx950_library

pytestmark = pytest.mark.gpu

H, W = 480, 640
A, K1, K2 = 60, 2, 3
CASES = [(5, h, w) for h, w in yc.SHAPES] + [(1, 12, 19)]
FIELDS = ("idx_a", "idx_b", "offsets", "empty", "type", "status", "input_a", "input_b", "mask_a", "mask_b")
EMULATED = {}


def _case(n, h, w):
    ex = yc.example_batch(n, h, w, seed=h * 100 + w)
    return ex, yc.fused_draws(ex, yc.example_draws(n, A, K1, K2, seed=h + w), True)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    """The emulation library's results first (on the host), then the shipped library for everything else"""
    use_emulation_library()
    for n, h, w in CASES:
        ex, draws = _case(n, h, w)
        sb, _ = yc.run_fused(ex, "cpu", A, True, K1, K2, True, draws=draws)
        EMULATED[(n, h, w)] = {k: getattr(sb, k).clone() for k in FIELDS}
    return use_gfx950_library()


@pytest.mark.parametrize("path", yc.GOLDENS, ids=yc.GOLDEN_IDS)
def test_golden_replays_on_device(path):
    z = np.load(path)
    sb = yc.replay_golden(z, "cuda")
    torch.cuda.synchronize()
    yc.check_golden(sb, z)


@pytest.mark.parametrize("n,h,w", CASES, ids=["B%d_%dx%d" % c for c in CASES])
def test_device_equals_emulation(n, h, w):
    ex, draws = _case(n, h, w)
    sb, _ = yc.run_fused(ex, "cuda", A, True, K1, K2, True, draws=draws)
    torch.cuda.synchronize()
    for k in FIELDS:
        assert torch.equal(getattr(sb, k).cpu(), EMULATED[(n, h, w)][k]), k
    assert int(sb.status[0]) == 0
    if h * w > 1:                                # (one pixel: the object behind is always hidden)
        assert not bool(sb.empty.all())


def _cfg(A=10000, non_matches=150):
    return yc.training_config({"SYNTHETIC_MULTI_OBJECT": 1.0}, A, non_matches)


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return [x for x in names if "DtoH" in x or "DeviceToHost" in x or x == "aten::item" or x == "aten::_local_scalar_dense"]


def test_draw_training_batch_never_synchronizes():
    from dcn_hip import frames
    store = yc.training_store("cuda", H, W)
    cfg = _cfg()
    g = torch.Generator(device="cuda").manual_seed(7)
    host = np.random.RandomState(7)

    def call():
        frames.draw_training_batch(store, 2, cfg, generator=g, host_rng=host, synthetic_multi_object=True)
    call()
    torch.cuda.synchronize()
    honoured = True
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.zeros(1, device="cuda").item()
            honoured = False
        except RuntimeError:
            pass
        if honoured:
            call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        assert _d2h_copies(call) == []
    torch.cuda.synchronize()


def test_end_to_end_store_to_loss_backward():
    """draw_training_batch(synthetic_multi_object=True) -> forward_pair -> get_loss_mixed -> backward, with one sample whose
    object came from the scene where no image b has a different enough pose: it is empty, its terms are exactly 0."""
    from dcn_hip import frames
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    import parity_common as pc
    from oracle import synth
    store = yc.training_store("cuda", H, W)
    cfg = _cfg()
    n = 2
    for seed in range(64):                       # the first seed that draws one empty and one non-empty sample
        g = torch.Generator(device="cuda").manual_seed(seed)
        sb, dt, fb = frames.draw_training_batch(store, n, cfg, generator=g, host_rng=np.random.RandomState(seed),
                                                synthetic_multi_object=True)
        if sorted(fb.empty.tolist()) == [False, True]:
            break
    else:
        raise AssertionError("no seed gave a batch with one empty sample")
    assert dt == frames.SYNTHETIC_MULTI_OBJECT and int(fb.status[0]) == 0 and int(sb.status[0]) == 0
    e = int(np.nonzero(fb.empty.cpu().numpy())[0][0])
    assert sb.empty.tolist()[e] and sb.type.tolist() == ([-1, 4] if e == 0 else [4, -1])
    off = sb.offsets.cpu().numpy()
    assert off[4 * e + 4] == off[4 * e] and off[4 * (1 - e) + 1] - off[4 * (1 - e)] > 100
    assert all(off[4 * p + 4] == off[4 * p + 3] for p in range(n))               # no blind list
    pcl = PixelwiseContrastiveLoss(image_shape=(H, W), config=synth.LOSS_CONFIG)
    dcn, _ = pc.build_dcn("Resnet34_8s", 3, H, W)
    ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
    loss, terms, hard, num_valid = loss_composer.get_loss_mixed(pcl, dcn.process_network_output(ya, n),
                                                                dcn.process_network_output(yb, n), sb.device_lists())
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and float(loss) > 0 and int(num_valid[0]) == 1 and int(pcl.last_status[0]) == 0
    assert bool((terms[e] == 0).all()) and bool((hard[e] == 0).all()) and float(terms[1 - e, 0]) > 0
    gw = [p.grad for p in dcn.parameters() if p.grad is not None]
    assert gw and all(bool(torch.isfinite(x).all()) for x in gw)
