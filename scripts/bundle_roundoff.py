#!/usr/bin/env python3
"""Round-off of the bundle adjustment's kernel formulas, measured on the reference alone (CPU, no device).

For every case of tests/test_bundle.py a float64 leg that follows the kernels' formulas (adjugate inverse, 6 x 6 Cholesky,
per-point sums in member order, per-camera sums in list order and again in a permuted order) is compared against the
longdouble leg (bundle_spec.step_reference) by bundle_spec.state_distance.  The bounds of the tests are ten times the
largest figure of each group; the figures go into tests/test_bundle.py and DESIGN.md section 3, item 11.

    python scripts/bundle_roundoff.py            # every group
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import bundle_spec as B  # noqa: E402


def legs(p, ref, **kw):
    n_obs = len(ref["ob"]["pt"])
    perm = np.random.default_rng(2).permutation(n_obs)
    out = []
    for order in (None, perm):
        got = B.run(p, solver="pcg", ft=np.float64, cam_order=order, **kw)
        out.append(B.state_distance(got, ref, dict(R=p["views"]["R"], c=p["views"]["c"], X=p["X"])))
    return out


def main():
    worst = 0.0
    for name, (V, T) in B.step_cases().items():
        p = B.step_problem(V, T)
        for n in B.STEP_COUNTS:
            ref = B.step_reference(p, n)
            d = legs(p, ref, force_accept=True, cg_iters=n, **B.STEP_PARAMS)
            worst = max(worst, *d)
            print("step   %-10s n = %d: list order %.3g, permuted %.3g" % (name, n, d[0], d[1]))
    p, _ = B.list_shapes_problem()
    kw = dict(B.STEP_PARAMS, min_cam_obs=B.DEFAULTS["min_cam_obs"])
    ref = B.step_reference(p, 7, **{k: v for k, v in kw.items() if k != "iters"})
    d = legs(p, ref, force_accept=True, cg_iters=7, **kw)
    worst = max(worst, *d)
    print("lists  n = 7: list order %.3g, permuted %.3g" % tuple(d))
    print("ROUNDOFF = %.3g" % worst)
    conv = 0.0
    for V, T, seed in B.CONVERGED_SCENES:
        p = B.make_problem(V=V, T=T, seed=seed)
        tr = []
        ref = B.run(p, solver="direct", trace=tr, **{k: v for k, v in B.CONVERGED_PARAMS.items() if k not in ("cg_iters", "cg_tol")})
        d = legs(p, ref, **B.CONVERGED_PARAMS)
        conv = max(conv, *d)
        print("converged V = %d: gains %s, list order %.3g, permuted %.3g" % (V, [round(t["gain"], 3) for t in tr], d[0], d[1]))
    print("CONVERGED = %.3g" % conv)
    gap = 0.0
    for V, T, seed in B.DEFAULT_SCENES:
        p = B.make_problem(V=V, T=T, seed=seed, tri=B.OUTLIER_TRI)
        ref = B.run(p, solver="direct")
        for order in (None, np.random.default_rng(2).permutation(ref["n_obs"])):
            got = B.run(p, solver="pcg", cam_order=order)
            g = abs(got["cost_final"] - ref["cost_final"]) / ref["cost_final"]
            gap = max(gap, g)
            print("defaults V = %d: cost %.12g against %.12g, gap %.3g, %d / %d outer iterations" %
                  (V, got["cost_final"], ref["cost_final"], g, got["iters"], ref["iters"]))
    print("DEFAULT_COST_GAP = %.3g" % gap)


if __name__ == "__main__":
    main()
