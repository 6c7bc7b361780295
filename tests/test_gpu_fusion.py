"""TSDF fusion, surface extraction and the box crop (csrc/fusion_kernels.hip, csrc/fusion_rules.h, dcn_hip/fusion.py) on the
MI355X: the checks of tests/fusion_common.py -- sums, weights, status, vertices, triangles and counts EQUAL the numpy statement,
the derived bound of the plane test, the crop against the reference's own lines (fusion goldens), the PLY writer -- and depth
images -> fuse_scene -> render_scene -> FrameStore -> draw_training_batch with no host synchronisation in the fusion, the
render or the draw.  Reads tests/golden only."""
import numpy as np
import pytest
import torch

import fusion_common as fc
import render_common as rc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("F", fc.FRAME_COUNTS)
@pytest.mark.parametrize("shape,hw", list(zip(fc.VOLUMES, (fc.IMAGES[0], fc.IMAGES[1], fc.IMAGES[1]))),
                         ids=["%dx%dx%d" % s for s in fc.VOLUMES])
def test_integration_equals_the_statement_chunked_and_split(shape, hw, F):
    fc.check_integrate_random(shape, hw, F, "cuda")


def test_integration_exact_cases_of_every_rule():
    fc.check_integrate_edges("cuda")


def test_integration_skips_nan_and_huge_poses():
    fc.check_integrate_bad_poses("cuda")


def test_integration_saturates_in_frame_order():
    fc.check_integrate_saturation("cuda")


def test_integration_is_repeatable():
    fc.check_integrate_repeatable("cuda")


def test_extraction_of_an_integrated_volume():
    fc.check_extract_integrated("cuda")


def test_extraction_of_a_sphere_is_a_closed_oriented_manifold():
    fc.check_extract_sphere("cuda")


def test_extraction_zero_sums_zero_weights_and_every_table_case():
    fc.check_extract_zeros_and_weights("cuda")


def test_extraction_capacities_and_guard_rows():
    fc.check_extract_capacities("cuda")


def test_extraction_degenerate_volumes():
    fc.check_extract_degenerate("cuda")


def test_plane_vertices_within_the_derived_bound():
    fc.check_plane_accuracy("cuda")


@pytest.mark.parametrize("name", fc.CROP_GOLDENS)
def test_crop_is_the_references(name):
    fc.check_crop_golden(name, "cuda")


def test_crop_bounds_rotation_padding_nothing_everything():
    fc.check_crop_cases("cuda")


def test_crop_capacities_and_guard_rows():
    fc.check_crop_capacities("cuda")


def test_ply_round_trip(tmp_path):
    fc.check_ply_round_trip("cuda", tmp_path)


def test_argument_errors():
    fc.check_argument_errors("cuda")


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


def test_depth_images_to_meshes_to_store_to_training_batch_without_read_back():
    """fuse_scene, render_scene on the fused meshes and draw_training_batch run under torch's sync debug mode: none reads
    anything back.  The store in between keeps host copies of the poses, which come from the host."""
    from dcn_hip import frames
    g = torch.Generator(device="cuda").manual_seed(3)
    host = np.random.RandomState(3)
    out = {}
    scene = rc.box_scene_on("cuda")
    im, K, _, _ = rc.render_box_scene(scene)

    def fuse():
        out["fused"] = fc.fuse_box_scene(im, K, scene[2])
        out["again"] = fc.rerender(out["fused"], K, scene[2])

    def draw():
        out["batch"] = frames.draw_training_batch(out["store"], 2, rc.scene_config(), generator=g, host_rng=host)
    fuse()                                                     # (first calls: allocator warm-up)
    _without_read_back(fuse)
    out["store"] = rc.store_of(out["again"], K, "cuda")
    draw()
    _without_read_back(draw)
    sb, dt, _ = out["batch"]
    assert sb.idx_a.is_cuda and out["fused"][0].vertices.is_cuda and out["again"].mask.is_cuda
    fc.check_fused_scene(out["fused"], out["again"])
    rc.check_batch(sb, dt)
