"""Painting mesh vertices from their views (csrc/paint_kernels.hip, csrc/paint_rules.h, dcn_hip/paint.py) through the
host-emulation build: count, sum, sumsq, mean, variance and colours EQUAL the numpy statement of tests/paint_common.py --
chunked and split accumulation, the exact cases of every rule --, the derived bound of the geometry test, constant
views, the coloured PLY file, the argument errors, and depth images -> fuse_scene -> render_scene -> MeshPaint and
paint_descriptors.  The checks are in tests/paint_common.py."""
import pytest
import torch

import paint_common as pc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("V,hw,F,C,dtype", pc.RANDOM_CASES, ids=pc.RANDOM_IDS)
def test_paint_equals_the_statement_chunked_and_split(V, hw, F, C, dtype):
    pc.check_paint_random(V, hw, F, C, dtype, "cpu")


def test_paint_exact_cases_of_every_rule():
    pc.check_paint_edges("cpu")


def test_painted_positions_within_the_derived_bound_and_occlusion():
    pc.check_geometry("cpu")


def test_constant_views_give_their_colour_exactly():
    pc.check_constant_views("cpu")


def test_paint_is_repeatable_and_spread_is_the_root():
    pc.check_repeatable("cpu")


def test_fused_scene_to_painted_mesh():
    full, again, K, poses = pc.fused_box_scene(*pc.box_scene_images("cpu"))
    rgb = torch.randint(0, 256, (4, 48, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    p, out = pc.paint_fused_scene(full, again, K, poses, rgb)
    pc.check_fused_paint(p, out, full, again, K, rgb)


def test_paint_descriptors_equals_one_add_over_all_frames():
    pc.check_descriptor_chain("cpu")


def test_coloured_ply_round_trip(tmp_path):
    pc.check_coloured_ply("cpu", tmp_path)


def test_argument_errors():
    pc.check_argument_errors("cpu")
