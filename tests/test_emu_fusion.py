"""TSDF fusion, surface extraction and the box crop (csrc/fusion_kernels.hip, csrc/fusion_rules.h, dcn_hip/fusion.py) through
the host-emulation build: sums, weights, status, vertices, triangles and counts EQUAL the numpy statement of
tests/fusion_common.py -- chunked and split integration, the exact cases of every rule, saturation, the extraction's table,
capacities and degenerate volumes, the crop against the reference's own lines (fusion goldens) -- the derived bound of the plane
test, the PLY writer, and depth images -> fuse_scene -> render_scene -> FrameStore -> draw_training_batch.  The checks are in
tests/fusion_common.py."""
import numpy as np
import pytest
import torch

import fusion_common as fc
import render_common as rc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("F", fc.FRAME_COUNTS)
@pytest.mark.parametrize("shape,hw", list(zip(fc.VOLUMES, (fc.IMAGES[0], fc.IMAGES[1], fc.IMAGES[1]))),
                         ids=["%dx%dx%d" % s for s in fc.VOLUMES])
def test_integration_equals_the_statement_chunked_and_split(shape, hw, F):
    fc.check_integrate_random(shape, hw, F, "cpu")


def test_integration_exact_cases_of_every_rule():
    fc.check_integrate_edges("cpu")


def test_integration_skips_nan_and_huge_poses():
    fc.check_integrate_bad_poses("cpu")


def test_integration_saturates_in_frame_order():
    fc.check_integrate_saturation("cpu")


def test_integration_is_repeatable():
    fc.check_integrate_repeatable("cpu")


def test_extraction_of_an_integrated_volume():
    fc.check_extract_integrated("cpu")


def test_extraction_of_a_sphere_is_a_closed_oriented_manifold():
    fc.check_extract_sphere("cpu")


def test_extraction_zero_sums_zero_weights_and_every_table_case():
    fc.check_extract_zeros_and_weights("cpu")


def test_library_table_words_are_the_derived_ones():
    """The 16 words in csrc/fusion_rules.h, read from its text, against the derivation (the equality on the every-case field
    checks the same through the kernel)"""
    import os
    import re
    from helpers import PKG
    text = open(os.path.join(PKG, "csrc", "fusion_rules.h")).read()
    body = re.search(r"kTetCases\[16\] = \{(.*?)\};", text, re.S).group(1)
    assert [int(w.strip().rstrip("u"), 16) for w in body.split(",")] == fc.packed_cases()


def test_extraction_capacities_and_guard_rows():
    fc.check_extract_capacities("cpu")


def test_extraction_degenerate_volumes():
    fc.check_extract_degenerate("cpu")


def test_plane_vertices_within_the_derived_bound():
    fc.check_plane_accuracy("cpu")


@pytest.mark.parametrize("name", fc.CROP_GOLDENS)
def test_crop_is_the_references(name):
    fc.check_crop_golden(name, "cpu")


def test_crop_bounds_rotation_padding_nothing_everything():
    fc.check_crop_cases("cpu")


def test_crop_capacities_and_guard_rows():
    fc.check_crop_capacities("cpu")


def test_ply_round_trip(tmp_path):
    fc.check_ply_round_trip("cpu", tmp_path)


def test_argument_errors():
    fc.check_argument_errors("cpu")


def test_depth_images_to_meshes_to_store_to_training_batch():
    from dcn_hip import frames
    scene = rc.box_scene_on("cpu")
    im, K, _, _ = rc.render_box_scene(scene)
    fused = fc.fuse_box_scene(im, K, scene[2])
    again = fc.rerender(fused, K, scene[2])
    fc.check_fused_scene(fused, again)
    store = rc.store_of(again, K, "cpu")
    sb, dt, _ = frames.draw_training_batch(store, 2, rc.scene_config(), generator=torch.Generator().manual_seed(3),
                                           host_rng=np.random.RandomState(3))
    rc.check_batch(sb, dt)
