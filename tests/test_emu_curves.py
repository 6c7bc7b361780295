"""Evaluation curves (csrc/curve_kernels.hip, dcn_hip.evaluate: cumulative_frequencies, evaluation_curves, curves_to_host,
area_above_curve, write_stats_yaml) through the host-emulation build: every case of tests/curves_common.py against
scipy.stats.cumfreq directly and against the fixtures written from the reference's own functions; the host rules; the wrappers
on a same-scene, an across-object and a cross-scene table."""
import numpy as np
import pytest
import torch

import curves_common as cu
from dcn_hip import evaluate
from helpers import use_emulation_library

CASES = cu.build_cases()


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert sorted(cu.GOLDEN_IDS) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_scipy(name):
    cu.check_case(name, CASES[name], "cpu")


@pytest.mark.parametrize("path", cu.GOLDENS, ids=cu.GOLDEN_IDS)
def test_golden(path):
    z = np.load(path)
    name = cu.GOLDEN_IDS[cu.GOLDENS.index(path)]
    case = cu.golden_case(z)
    # the fixture holds the case it is named for
    assert cu.same_bits(case["values"], CASES[name]["values"]) and case["num_bins"] == CASES[name]["num_bins"]
    assert case["drop_nan"] == CASES[name]["drop_nan"] and (case["row_pair"] is None) == (CASES[name]["row_pair"] is None)
    cu.check_golden(z, "cpu")


def test_the_cases_are_what_they_are_named_for():
    want = {k: cu.oracle(c) for k, c in CASES.items()}
    # the widened range: lowerlimit unwidened, binsize from the widened edges
    for name in ("single", "all_equal"):
        assert want[name]["lowerlimit"][0] == 3.5 and want[name]["binsize"][0] == 0.009999999999999787
        assert want[name]["cumcount"][0].tolist() == [0] * 50 + [int(want[name]["n"][0])] * 50
    assert np.diff(want["integers"]["cumcount"][0], prepend=0).tolist() == [1] * 100          # edges at k - 0.5
    assert want["integers"]["lowerlimit"][0] == -0.5 and want["integers"]["binsize"][0] == 1.0
    # values exactly on the interior edges open their bin
    x = CASES["on_edges"]["values"][0]
    assert np.array_equal(x[50:], cu.edges_of(x[:50], 10)[1:-1])
    assert np.diff(want["on_edges"]["cumcount"][0], prepend=0).tolist() == cu.EDGE_COUNTS
    assert want["row_pair"]["dropped"][0] == 0 and want["row_pair"]["n"][0] == 130 - 17 and want["row_pair"]["flags"][0] == 0
    assert want["nan_dropped"]["dropped"][0] > 20 and want["nan_dropped"]["flags"][0] == 0
    assert want["nan_not_dropped"]["flags"].tolist() == [cu.NAN] and want["inf"]["flags"].tolist() == [cu.NONFINITE]
    assert want["no_rows"]["flags"].tolist() == [cu.EMPTY] and want["all_nan_dropped"]["flags"].tolist() == [cu.EMPTY]
    assert want["nine_curves"]["flags"].tolist() == [0, 0, cu.NAN, 0, cu.NONFINITE, cu.EMPTY, 0, 0, 0]
    assert want["nine_curves"]["dropped"].tolist() == [0, 10, 0, 0, 0, 253, 1, 0, 0]
    assert want["r5000"]["n"][0] > 4 * 1024


def test_strided_rows_and_a_one_dimensional_column():
    """a [C, R] view into a wider tensor is read in place (its row stride is the leading dimension); a [R] column is one curve"""
    case = CASES["nine_curves"]
    want = cu.oracle(case)
    wide = torch.full((9, 300), 7.0, dtype=torch.float64)
    wide[:, :257] = torch.from_numpy(case["values"])
    c = evaluate.cumulative_frequencies(wide[:, :257], torch.from_numpy(case["row_pair"]), 100, case["drop_nan"])
    cu.check_against(cu.to_numpy(c), want, 100, "strided")
    one = evaluate.cumulative_frequencies(torch.from_numpy(CASES["r65"]["values"][0]))
    cu.check_against(cu.to_numpy(one), cu.oracle(CASES["r65"]), 100, "1-D")
    assert one.fields == (0,) and one.num_bins == 100
    # out_summary: a view into a larger tensor is written in place
    hist = torch.zeros((3, 4 + 8), dtype=torch.float64)
    two = evaluate.cumulative_frequencies(torch.from_numpy(CASES["r65"]["values"][0]), out_summary=hist[1, 4:].view(1, 8))
    assert two.summary.data_ptr() == hist[1, 4:].data_ptr() and torch.equal(hist[1, 4:], one.summary[0])
    assert not hist[0].any() and not hist[2].any() and not hist[1, :4].any()


def test_host_rules():
    cu.check_host_rules("cpu")
    from dcn_hip import _lib
    cu.check_raw_entry_rejects(_lib, "cpu")


def test_curves_to_host_raises_what_the_reference_raises():
    cu.check_curves_to_host_errors(CASES, "cpu")


def _tiny_dcn(h, w):
    import pytorch_segmentation_detection.models.resnet_dilated as rd
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    torch.manual_seed(0)
    return DenseCorrespondenceNetwork(rd.Resnet18_8s(num_classes=3, base_width=8), 3, image_width=w, image_height=h)


def test_curves_of_a_same_scene_table(tmp_path):
    cu.check_same_scene_table("cpu", 32, 48, _tiny_dcn, tmp_path)


def test_curves_of_an_across_object_table():
    cu.check_across_object_table("cpu", 24, 32)


def test_curves_of_a_cross_scene_table_with_rows_left_out():
    cu.check_cross_scene_table("cpu")
