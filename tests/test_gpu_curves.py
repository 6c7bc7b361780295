"""Evaluation curves on the MI355X (csrc/curve_kernels.hip, dcn_hip.evaluate): every fixture of tests/golden/curves_ref_*.npz
-- the reference's own results and the emulation build's outputs -- bit for bit and run to run, the host rules, and the
wrappers on a same-scene table of the real network, an across-object and a cross-scene table.  Reads tests/golden only."""
import numpy as np
import pytest

import curves_common as cu
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


def test_golden_set():
    assert len(cu.GOLDENS) == 22


@pytest.mark.parametrize("path", cu.GOLDENS, ids=cu.GOLDEN_IDS)
def test_golden(path):
    cu.check_golden(np.load(path), "cuda")


def test_host_rules():
    import torch
    from dcn_hip import _lib, evaluate
    cu.check_host_rules("cuda")
    cu.check_raw_entry_rejects(_lib, "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # a CPU tensor on the GPU build
        evaluate.cumulative_frequencies(torch.zeros((1, 8), dtype=torch.float64))


def test_curves_to_host_raises_what_the_reference_raises():
    cases = {cu.GOLDEN_IDS[i]: cu.golden_case(np.load(p)) for i, p in enumerate(cu.GOLDENS)}
    cu.check_curves_to_host_errors(cases, "cuda")


def _dcn(h, w):
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    return DenseCorrespondenceNetwork.from_config({"descriptor_dimension": 3, "image_width": w, "image_height": h},
                                                  load_stored_params=False).cuda()


def test_curves_of_a_same_scene_table(tmp_path):
    cu.check_same_scene_table("cuda", 64, 96, _dcn, tmp_path)


def test_curves_of_an_across_object_table():
    cu.check_across_object_table("cuda", 48, 64)


def test_curves_of_a_cross_scene_table_with_rows_left_out():
    cu.check_cross_scene_table("cuda")
