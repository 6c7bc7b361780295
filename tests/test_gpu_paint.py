"""Painting mesh vertices from their views (csrc/paint_kernels.hip, csrc/paint_rules.h, dcn_hip/paint.py) on the MI355X: the
checks of tests/paint_common.py -- count, sum, sumsq, mean, variance and colours EQUAL the numpy statement, the derived bound of
the geometry test, constant views, the coloured PLY file, the argument errors -- and depth images -> fuse_scene ->
render_scene -> MeshPaint.add -> finish and paint_descriptors with no host synchronisation."""
import pytest
import torch

import paint_common as pc
import render_common as rc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("V,hw,F,C,dtype", pc.RANDOM_CASES, ids=pc.RANDOM_IDS)
def test_paint_equals_the_statement_chunked_and_split(V, hw, F, C, dtype):
    pc.check_paint_random(V, hw, F, C, dtype, "cuda")


def test_paint_exact_cases_of_every_rule():
    pc.check_paint_edges("cuda")


def test_painted_positions_within_the_derived_bound_and_occlusion():
    pc.check_geometry("cuda")


def test_constant_views_give_their_colour_exactly():
    pc.check_constant_views("cuda")


def test_paint_is_repeatable_and_spread_is_the_root():
    pc.check_repeatable("cuda")


def test_paint_descriptors_equals_one_add_over_all_frames():
    pc.check_descriptor_chain("cuda")


def test_coloured_ply_round_trip(tmp_path):
    pc.check_coloured_ply("cuda", tmp_path)


def test_argument_errors():
    pc.check_argument_errors("cuda")


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return [x for x in names if "DtoH" in x or "DeviceToHost" in x or x == "aten::item" or x == "aten::_local_scalar_dense"]


def _without_read_back(fn):
    """fn() under torch's sync debug mode "error"; where torch does not honour the mode, no device-to-host copy in its profile"""
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
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        assert _d2h_copies(fn) == []
    torch.cuda.synchronize()


def test_fused_scene_to_painted_mesh_and_descriptors_without_read_back():
    """fuse_scene(trim=False) -> render_scene -> MeshPaint.add -> finish, and paint_descriptors on a store built from those
    images with a pointwise stand-in network, run under torch's sync debug mode: none reads anything back.  The store in
    between keeps host copies of the poses, which come from the host."""
    out = {}
    rgb = torch.randint(0, 256, (4, 48, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(6)).cuda()
    net = pc.PointwiseNetwork(keep=False)
    uploaded = pc.box_scene_images("cuda")

    def colour():
        out["full"], out["again"], out["K"], out["poses"] = pc.fused_box_scene(*uploaded)
        out["paint"], out["painted"] = pc.paint_fused_scene(out["full"], out["again"], out["K"], out["poses"], rgb)

    def describe():
        from dcn_hip import paint
        out["described"] = paint.paint_descriptors(net, out["store"], out["full"], 0, batch=3)
    colour()                                                   # (first calls: allocator warm-up)
    _without_read_back(colour)
    out["store"] = rc.store_of(out["again"], out["K"], "cuda")
    describe()
    _without_read_back(describe)
    painted, summary = out["described"]
    assert painted.spread.is_cuda and summary.is_cuda and out["painted"].colours.is_cuda
    pc.check_fused_paint(out["paint"], out["painted"], out["full"], out["again"], out["K"], rgb)
    assert float(summary[0]) > 10
