"""Pins the evaluation curves (dcn_hip/evaluate/curves.py: cumulative_frequencies, evaluation_curves, curves_to_host,
area_above_curve; csrc/curve_kernels.hip): executes the REFERENCE's own source text -- read from the reference tree at run
time, never copied --
  dense_correspondence/evaluation/evaluation.py DenseCorrespondenceEvaluationPlotter.make_cdf_plot (:2658-2674) and
  compute_area_above_curve (:2844-2863), the Python-2 text converted in memory as tests/reference_py3.py converts modules,
with ``ss`` bound to scipy.stats and ``np`` to numpy, on the cases of tests/curves_common.build_cases.  The two functions
need neither matplotlib nor the rest of the plotter: ``make_cdf_plot`` gets an axis object that records what is plotted,
``compute_area_above_curve`` a pandas DataFrame (its ``dropna()``).  What they do not return -- the counts, ``lowerlimit`` and
``binsize`` -- comes from the same ``scipy.stats.cumfreq`` call made here.

A flagged curve (one for which the reference's call raises) stores its flag and NaN.  The generator asserts that the
reference's results equal tests/curves_common.oracle bit for bit (the oracle the CPU tests use directly), runs the
host-emulation build on the same inputs and stores its outputs beside them (``emu_*``): the GPU tests, which have neither the
reference nor a second implementation at hand, compare with both.

    python tests/golden/make_curves_goldens_from_reference.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_py3 as rp                                                           # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402
from make_evalpairs_goldens_from_reference import method_source                      # noqa: E402

EVAL = os.path.join(rp.REF, "dense_correspondence", "evaluation", "evaluation.py")


def load_reference():
    import scipy.stats as ss
    lines = rp.converted_source(EVAL).split("\n")
    ns = {"np": np, "ss": ss}
    for name in ("make_cdf_plot", "compute_area_above_curve"):
        exec(compile(method_source(lines, name), EVAL, "exec"), ns)
    return ns["make_cdf_plot"], ns["compute_area_above_curve"]


class RecordingAxis(object):
    def plot(self, x, y, label=None):
        self.x, self.y = np.array(x, np.float64), np.array(y, np.float64)
        return [self]


def reference_results(case, make_cdf_plot, compute_area_above_curve):
    import warnings
    import pandas
    import curves_common as cu
    want = cu.oracle(case)
    nb, C = case["num_bins"], case["values"].shape[0]
    x_axis = np.full((C, nb), np.nan)
    for k in range(C):
        data = case["values"][k]
        if case["row_pair"] is not None:
            data = data[case["row_pair"] >= 0]
        series = pandas.Series(data)
        if case["drop_nan"][k]:
            series = series.dropna()
        ax = RecordingAxis()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                make_cdf_plot(ax, series, nb)
                area = compute_area_above_curve(pandas.DataFrame({"field": series}), "field", nb)
        except ValueError:
            assert want["flags"][k] in (cu.NAN, cu.NONFINITE), (k, want["flags"][k])
            continue
        except ZeroDivisionError:
            assert want["flags"][k] == cu.EMPTY, (k, want["flags"][k])
            continue
        assert want["flags"][k] == 0
        assert cu.same_bits(ax.y, want["cdf"][k]) and cu.same_bits(area, want["area"][k]), k
        assert cu.same_bits(ax.x, want["lowerlimit"][k] + want["binsize"][k] * np.arange(0, nb)), k
        x_axis[k] = ax.x
    want["x_axis"] = x_axis
    return want


def main():
    import curves_common as cu
    from helpers import use_emulation_library
    use_emulation_library()
    fns = load_reference()
    cases = cu.build_cases()
    assert np.array_equal(cu.oracle(cases["on_edges"])["cumcount"][0], np.cumsum(cu.EDGE_COUNTS))
    for name, case in cases.items():
        ref = reference_results(case, *fns)
        emu = cu.check_case(name, case, "cpu", ref)
        arrays = dict(values=case["values"], num_bins=np.int64(case["num_bins"]),
                      has_row_pair=np.int64(case["row_pair"] is not None),
                      row_pair=case["row_pair"] if case["row_pair"] is not None else np.zeros(0, np.int32),
                      drop_nan=np.array(case["drop_nan"], np.uint8))
        for key in ("flags", "cumcount", "cdf", "area", "x_axis") + cu.SUMMARY_BITS:
            arrays["ref_" + key] = ref[key]
        for key in ("flags", "cumcount", "cdf", "area") + cu.SUMMARY_BITS:
            arrays["emu_" + key] = emu[key]
        path = os.path.join(HERE, "curves_ref_%s.npz" % name)
        write_npz(path, arrays)
        print("%-18s C %d R %5d bins %4d flags %s  %6d bytes" % (name, case["values"].shape[0], case["values"].shape[1],
                                                              case["num_bins"], list(ref["flags"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
