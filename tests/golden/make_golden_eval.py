"""Regenerates tests/golden/dtu_sample_tri.npz from the reference checkout (not needed to run the tests):

    python tests/golden/make_golden_eval.py /path/to/reference

The reference's DTU evaluation has no importable module (eval.py is a script that imports open3d and sklearn at the top), so
its sampler is executed the way make_golden.py executes other functions: `sample_single_tri` is lifted out of
evaluation/DTU/eval_code/eval.py with `ast` and run, fed by the script's own lines 54-65 restated with the same numpy calls
(np.linalg.norm, np.cross, the non-zero-area selection, np.floor).  Stored: data only -- the triangles, the density, and per
triangle the points the reference's function returned."""
import ast
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def triangles(rng):
    """a few dozen triangles of four size classes around a density of 0.2, far from and near the origin"""
    tris = []
    for scale, n in ((0.05, 8), (0.3, 10), (1.0, 10), (4.0, 8)):
        for _ in range(n):
            c = rng.uniform(-300, 300, 3)
            tris.append(c + rng.normal(0, scale, (3, 3)))
    tris.append(np.array([[0, 0, 0], [3.0, 0, 0], [0, 0.02, 0]]))            # needle
    tris.append(np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3.0]]))               # zero area
    tris.append(np.array([[0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]]))             # right triangle on the axes
    return np.array(tris, np.float64)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    src = open(os.path.join(ref, "evaluation", "DTU", "eval_code", "eval.py")).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "sample_single_tri")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "eval.py", "exec"), ns)
    sample_single_tri = ns["sample_single_tri"]

    density = 0.2
    tri_vert = triangles(np.random.default_rng(20))
    v1 = tri_vert[:, 1] - tri_vert[:, 0]
    v2 = tri_vert[:, 2] - tri_vert[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    non_zero_area = (area2 > 0)[:, 0]
    counts = np.zeros(len(tri_vert), np.int64)
    pts = []
    with np.errstate(all="ignore"):
        thr = density * np.sqrt(l1 * l2 / area2)
        n1 = np.floor(l1 / thr)
        n2 = np.floor(l2 / thr)
    for i in np.nonzero(non_zero_area)[0]:
        q = sample_single_tri((n1[i, 0], n2[i, 0], v1[i:i + 1], v2[i:i + 1], tri_vert[i:i + 1, 0]))
        counts[i] = len(q)
        pts.append(q)
    np.savez_compressed(os.path.join(OUT, "dtu_sample_tri.npz"), triangles=tri_vert, density=np.float64(density),
                        counts=counts, points=np.concatenate(pts, 0))
    print(len(tri_vert), "triangles,", int(counts.sum()), "points,", int((counts == 0).sum()), "without a point")


if __name__ == "__main__":
    main()
