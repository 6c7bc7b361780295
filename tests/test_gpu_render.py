"""The depth renderer (csrc/render_kernels.hip, csrc/render_raster.h, dcn_hip/render.py) on the MI355X: the checks of
tests/render_common.py -- depth images, status counts and masks EQUAL the numpy statement on every kernel path, the fill-rule,
drop and range cases, the reference's mask rules (render goldens), the pose convention against dcn_hip.pairgen, the PLY reader
-- and mesh -> render_scene -> FrameStore -> draw_training_batch with no host synchronisation in the render or the draw.
Reads tests/golden only."""
import numpy as np
import pytest
import torch

import render_common as rc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("F", rc.FRAME_COUNTS)
@pytest.mark.parametrize("h,w", rc.SHAPES, ids=["%dx%d" % s for s in rc.SHAPES])
def test_large_and_small_triangles_on_every_path(h, w, F):
    rc.check_mixed(h, w, F, "cuda")


def test_shared_edges_follow_the_top_left_rule():
    rc.check_shared_edges("cuda")


def test_vertex_on_a_pixel_centre():
    rc.check_vertex_on_centre("cuda")


def test_slivers_and_zero_area_triangles_draw_nothing():
    rc.check_slivers_and_zero_area("cuda")


def test_intersecting_triangles_keep_the_minimum():
    rc.check_intersecting("cuda")


def test_dropped_triangles_are_counted_by_rule():
    rc.check_dropped_triangles("cuda")


def test_triangles_off_screen():
    rc.check_off_screen("cuda")


def test_no_triangles():
    rc.check_no_triangles("cuda")


def test_millimetre_boundaries_and_the_far_end():
    rc.check_millimetre_boundaries("cuda")


def test_repeatable_and_independent_of_triangle_order():
    rc.check_repeatable_and_order_free("cuda")


def test_pose_convention_is_pairgens():
    rc.check_pairgen_convention("cuda")


@pytest.mark.parametrize("name", rc.MASK_GOLDENS)
def test_masks_are_the_references(name):
    rc.check_masks_golden(name, "cuda")


def test_argument_errors():
    rc.check_argument_errors("cuda")


def test_ply_reader(tmp_path):
    rc.check_ply("cuda", tmp_path)


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


def test_scene_to_store_to_training_batch_without_read_back(tmp_path):
    """render_scene and draw_training_batch run under torch's sync debug mode (as tests/test_gpu_train_ranks.py uses it):
    neither reads anything back.  The store in between keeps host copies of the poses, which come from the host."""
    from dcn_hip import frames
    g = torch.Generator(device="cuda").manual_seed(3)
    host = np.random.RandomState(3)
    out = {}
    scene = rc.box_scene_on("cuda")

    def render():
        out["scene"] = rc.render_box_scene(scene)

    def draw():
        out["batch"] = frames.draw_training_batch(out["store"], 2, rc.scene_config(), generator=g, host_rng=host)
    render()                                                   # (first calls: library load, allocator warm-up)
    _without_read_back(render)
    im, K, fg, full = out["scene"]
    out["store"] = rc.store_of(im, K, "cuda")
    draw()
    _without_read_back(draw)
    sb, dt, _ = out["batch"]
    assert sb.idx_a.is_cuda and sb.input_a.is_cuda and im.depth.is_cuda and im.mask.is_cuda
    rc.check_batch(sb, dt)
    rc.check_scene_images(im, K, fg, full)
    rc.check_written_images(im, tmp_path)
