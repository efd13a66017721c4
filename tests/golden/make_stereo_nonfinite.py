"""Writes tests/golden/stereo_nonfinite.npz for tests/test_stereo_edges.py: an ordinary 257 x 3 disparity pair and, for every
non-finite or out-of-range value the test puts into it, the occlusion mask that the numpy statement
(tests/sgm_statement.occlusion, i.e. the reference's Stereo.get_occlusion_mask arithmetic) gives for it.

Run on an x86-64 host: there ``astype(int32)`` of NaN and of values outside int32 gives INT_MIN, which the statement's
``xp < 0`` test calls occluded.  The conversion is undefined in C and differs between machines, so the expectation is recorded
here and not recomputed where the test runs."""
import os
import platform
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_stereo_edges as t  # noqa: E402


def main():
    assert platform.machine() in ("x86_64", "AMD64"), "the fixture records what x86-64 numpy gives"
    L, R = t.ordinary_disparities(257, 3)
    R[:, 0] = 5.0               # what a NaN of disp_lr that converts to 0 would read
    L[:, 102] = 2.0             # the pixels that read disp_rl[y][100]
    out = {"L2R": L, "R2L": R}
    golden = {"L2R": L, "R2L": R}
    for side, values in (("lr", t.NONFINITE_LR), ("rl", t.NONFINITE_RL)):
        for name in values:
            golden[f"mask_{side}_{name}"] = None
            l, r, _, where = t.nonfinite_case(golden, side, name)
            m = t.statement_mask(l, r, t.NONFINITE_THR)
            if side == "lr":
                assert np.all(m[where] == 0), (name, m[where])
            else:
                assert np.all(m[where] == (1 if name == "nan" else 0)), (name, m[where])
            out[f"mask_{side}_{name}"] = m
            print(side, name, "visible", float(m.mean()), "at the pixels the value decides:", m[where])
    path = os.path.join(HERE, "stereo_nonfinite.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
