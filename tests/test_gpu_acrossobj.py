"""Across-object evaluation on the MI355X (csrc/acrossobj_kernels.hip, dcn_hip/evaluate/across_objects.py): the reference goldens on the device,
the chain on a frame store against the single-image best-match kernel called pair by pair, and run-to-run bit identity."""
import numpy as np
import pytest
import torch

import acrossobj_common as ac
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("path", ac.GOLDENS, ids=ac.GOLDEN_IDS)
def test_golden_queries_and_best_matches(path):
    ac.check_golden(np.load(path), "cuda")


def test_chain_equals_the_single_image_kernel_pair_by_pair():
    """evaluate_object_pairs at 48 x 64 on a from_tensors store: per pair the same descriptors and queries through
    match.find_best_matches give the same pixel, and the same distance bit for bit (one arithmetic: the fma chain over the
    channels, then one correctly rounded square root)."""
    from dcn_hip import evaluate, match
    h, w, Q = 48, 64, 100
    store = ac.three_object_store("cuda", h, w)
    chosen = evaluate.choose_object_pairs(store, 5, np.random.RandomState(1))
    net = ac.StubNetwork().cuda()
    net.train()
    t = evaluate.evaluate_object_pairs(net, store, chosen, Q, generator=torch.Generator("cuda").manual_seed(3), batch_pairs=2)
    assert net.training and int(t.status.cpu()[0]) == 0
    assert t.offsets.cpu().tolist() == [Q * p for p in range(6)]
    res_a, res_b = net.descriptors()
    for p in range(5):
        rows = slice(p * Q, (p + 1) * Q)
        u, v = t.u_a[rows], t.v_a[rows]
        assert (store.mask[int(chosen[p, 4])][v, u] != 0).all() and len(set((v * w + u).cpu().tolist())) == Q
        idx, dist, _ = match.find_best_matches(res_b[p], res_a[p][v, u])
        assert torch.equal(t.best_uv[1, rows].long() * w + t.best_uv[0, rows].long(), idx)
        assert torch.equal(t.norm_diff_descriptor_best_match[rows].view(torch.int32), dist.view(torch.int32))
        assert (t.row_pair[rows] == p).all()


def test_the_search_is_bit_identical_from_run_to_run():
    g = torch.Generator().manual_seed(11)
    P, h, w, d, Q = 4, 37, 53, 16, 100
    res_b = torch.randn(P, h, w, d, generator=g).cuda()
    res_b[1, 5, 7] = res_b[1, 30, 2]                                            # equal minima for a query planted there
    queries = torch.randn(P * Q, d, generator=g).cuda()
    queries[Q] = res_b[1, 5, 7]
    from dcn_hip import evaluate
    off = (torch.arange(P + 1) * Q).cuda()
    a = evaluate.best_match_pairs(res_b, queries, off)
    b = evaluate.best_match_pairs(res_b, queries, off)
    assert int(a.status.cpu()[0]) == 0
    assert torch.equal(a.norm_diff_descriptor_best_match.view(torch.int32), b.norm_diff_descriptor_best_match.view(torch.int32))
    assert torch.equal(a.best_uv, b.best_uv) and torch.equal(a.row_pair, b.row_pair)
    assert a.best_uv[:, Q].cpu().tolist() == [7, 5] and float(a.norm_diff_descriptor_best_match[Q]) == 0.0
