"""Pins the box crop (csrc/fusion_kernels.hip mark_kernel, dcn_hip/fusion.py box_segments / crop_to_box): executes the
REFERENCE's own source lines -- read from /root/reference at run time, never copied --
  modules/dense_correspondence_manipulation/utils/director_utils.py
    :151-178   cropToLineSegment and cropToBox
on recorded points and triangles.  The lines call director, which is not installed; the two director calls and the two
accessors they need are supplied here in numpy, by what director documents them to do:
  labelPointDistanceAlongAxis(polyData, axis, origin, resultArrayName)   the point array dot(p - origin, axis)
  filterUtils.thresholdCells(polyData, name, [lo, hi], arrayType="points")   vtkThreshold on a point array: a cell is kept when
                                                                          ALL its points have lo <= scalar <= hi
  transform.GetPosition(), transformUtils.getAxesFromTransform(transform)   the translation and the three columns of the rotation
Every call the reference makes is recorded: per axis point1 (the origin it passes), axis', length' (the upper threshold).

The kernels' yardstick is the numpy statement in tests/fusion_common.py; the generator ASSERTS that the statement's segment
geometry equals what the reference's lines computed, and that its surviving set is theirs.

Stores in tests/golden/fusion_ref_crop_<name>.npz: points float32 [P, 3], triangles int32 [T, 3], transform float64 [4, 4],
dimensions float64 [3], segments float64 [3, 7], survives uint8 [T].  ``box`` has crop_box of
config/stations/RLG_iiwa_1/change_detection.yaml, ``rotated`` the same dimensions in a turned frame.

    python tests/golden/make_fusion_from_reference.py
"""
import ast
import hashlib
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import fusion_common as fc                                                           # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

SRC = "/root/reference/modules/dense_correspondence_manipulation/utils/director_utils.py"
CROP = (SRC, 151, 178, "094058d8e63479e99796d722393d0c7fdc7f58e4fdeba1a9909df7de4488aada")
STATION = ((0.66757267, 0.0, 0.18953078), (0.5, 0.7, 0.4))            # crop_box: translation, dimensions


def take(spec):
    path, first, last, sha = spec
    lines = open(path).read().split("\n")[first - 1:last]
    got = hashlib.sha256("\n".join(l.strip() for l in lines).encode()).hexdigest()
    assert got == sha, "the reference changed: %s:%d-%d (%s)" % (path, first, last, got)
    return textwrap.dedent("\n".join(lines)), path


class PolyData(object):
    def __init__(self, points, cells, alive=None):
        self.points, self.cells = points, cells
        self.alive = np.ones(len(cells), bool) if alive is None else alive
        self.arrays = {}


def load_reference(calls):
    """-> the reference's box crop as a function (polyData, transform, dimensions) -> polyData; the slice is validated by its
    structure, without quoting it, and by the hash of its text"""
    text, path = take(CROP)
    body = ast.parse(text).body
    assert len(body) == 2 and all(isinstance(n, ast.FunctionDef) for n in body), "not the slice"
    assert [len(n.args.args) for n in body] == [4, 4], "not the slice"

    def label(poly, axis, origin=None, resultArrayName=None):
        out = PolyData(poly.points, poly.cells, poly.alive)
        out.arrays[resultArrayName] = np.dot(poly.points.astype(np.float64) - np.asarray(origin), np.asarray(axis))
        calls.append((np.array(origin, np.float64), np.array(axis, np.float64)))
        return out

    def threshold_cells(poly, name, rng, arrayType=None):
        assert arrayType == "points"
        sc = poly.arrays[name]
        ok = (sc >= rng[0]) & (sc <= rng[1])
        calls[-1] = calls[-1] + (float(rng[0]), float(rng[1]))
        return PolyData(poly.points, poly.cells, poly.alive & ok[poly.cells].all(axis=1))

    env = {"np": np, "labelPointDistanceAlongAxis": label,
           "filterUtils": types.SimpleNamespace(thresholdCells=threshold_cells),
           "transformUtils": types.SimpleNamespace(getAxesFromTransform=lambda t: [t.matrix[:3, a] for a in range(3)])}
    exec(compile(text, path, "exec"), env)
    return env[body[1].name]


class Transform(object):
    def __init__(self, matrix):
        self.matrix = np.asarray(matrix, np.float64)

    def GetPosition(self):
        return tuple(self.matrix[:3, 3])


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def main():
    for name, rot in (("box", np.eye(3)), ("rotated", rotation([0.3, -0.2, 1.0], 0.4))):
        rng = np.random.RandomState(len(name))
        centre, dims = np.array(STATION[0]), np.array(STATION[1])
        T = np.eye(4)
        T[:3, :3] = rot
        T[:3, 3] = centre
        points = (centre + rng.uniform(-0.3, 0.3, (300, 3))).astype(np.float32)
        near = rng.randint(0, 300, 400)
        triangles = np.stack([near, (near + rng.randint(1, 12, 400)) % 300, rng.randint(0, 300, 400)], axis=1).astype(np.int32)
        calls = []
        crop_to_box = load_reference(calls)
        out = crop_to_box(PolyData(points, triangles), Transform(T), dims)
        assert len(calls) == 3 and all(c[2] == 0.0 for c in calls)
        segments = np.array([list(c[0]) + list(c[1]) + [c[3]] for c in calls], np.float64)
        assert np.array_equal(fc.np_segments(T, dims), segments), "tests/fusion_common.py np_segments is not the reference's geometry"
        want = fc.np_crop(points, triangles, T, dims)
        survivors = triangles[out.alive]
        assert 20 < len(survivors) < 380 and int(want[2][1]) == len(survivors)
        assert np.array_equal(want[0][want[1]], points[survivors]), "tests/fusion_common.py np_crop keeps another set"
        path = os.path.join(HERE, "fusion_ref_crop_%s.npz" % name)
        write_npz(path, dict(points=points, triangles=triangles, transform=T, dimensions=dims, segments=segments,
                             survives=out.alive.astype(np.uint8)))
        print(path, os.path.getsize(path), "bytes,", len(survivors), "of", len(triangles), "triangles survive")


if __name__ == "__main__":
    main()
