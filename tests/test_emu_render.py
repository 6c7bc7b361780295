"""The depth renderer (csrc/render_kernels.hip, csrc/render_raster.h, dcn_hip/render.py) through the host-emulation build:
depth images, status counts and masks EQUAL the numpy statement of tests/render_common.py on every kernel path, the fill-rule,
drop and range cases, the reference's mask rules (render goldens), the pose convention against dcn_hip.pairgen, the PLY reader,
and mesh -> render_scene -> FrameStore -> draw_training_batch.  The checks are in tests/render_common.py."""
import numpy as np
import pytest
import torch

import render_common as rc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("F", rc.FRAME_COUNTS)
@pytest.mark.parametrize("h,w", rc.SHAPES, ids=["%dx%d" % s for s in rc.SHAPES])
def test_large_and_small_triangles_on_every_path(h, w, F):
    rc.check_mixed(h, w, F, "cpu")


def test_shared_edges_follow_the_top_left_rule():
    rc.check_shared_edges("cpu")


def test_vertex_on_a_pixel_centre():
    rc.check_vertex_on_centre("cpu")


def test_slivers_and_zero_area_triangles_draw_nothing():
    rc.check_slivers_and_zero_area("cpu")


def test_intersecting_triangles_keep_the_minimum():
    rc.check_intersecting("cpu")


def test_dropped_triangles_are_counted_by_rule():
    rc.check_dropped_triangles("cpu")


def test_triangles_off_screen():
    rc.check_off_screen("cpu")


def test_no_triangles():
    rc.check_no_triangles("cpu")


def test_millimetre_boundaries_and_the_far_end():
    rc.check_millimetre_boundaries("cpu")


def test_repeatable_and_independent_of_triangle_order():
    rc.check_repeatable_and_order_free("cpu")


def test_pose_convention_is_pairgens():
    rc.check_pairgen_convention("cpu")


@pytest.mark.parametrize("name", rc.MASK_GOLDENS)
def test_masks_are_the_references(name):
    rc.check_masks_golden(name, "cpu")


def test_argument_errors():
    rc.check_argument_errors("cpu")


def test_ply_reader(tmp_path):
    rc.check_ply("cpu", tmp_path)


def test_scene_to_store_to_training_batch(tmp_path):
    from dcn_hip import frames
    im, K, fg, full = rc.render_box_scene(rc.box_scene_on("cpu"))
    rc.check_scene_images(im, K, fg, full)
    store = rc.store_of(im, K, "cpu")
    sb, dt, _ = frames.draw_training_batch(store, 2, rc.scene_config(), generator=torch.Generator().manual_seed(3),
                                           host_rng=np.random.RandomState(3))
    rc.check_batch(sb, dt)
    rc.check_written_images(im, tmp_path)
