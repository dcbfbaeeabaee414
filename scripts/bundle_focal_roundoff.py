#!/usr/bin/env python3
"""Round-off of the focal bundle adjustment's kernel formulas, measured on the reference alone (CPU, no device).

For every case of tests/test_bundle_focal.py a float64 leg that follows the kernels' formulas (bundle_focal_spec.step_pcg:
adjugate inverse, 7 x 7 Cholesky with the pinned columns zero, per-point sums in member order, per-camera sums in list order
and again in a permuted order) is compared against the longdouble leg by bundle_focal_spec.state_distance.  The bounds of the
tests are ten times the largest figure of each group; the figures go into tests/test_bundle_focal.py and DESIGN.md section
3, item 11.

    python scripts/bundle_focal_roundoff.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import bundle_focal_spec as F  # noqa: E402


def legs(p, ref, **kw):
    perm = np.random.default_rng(2).permutation(len(ref["ob"]["pt"]))
    return [F.state_distance(F.run(p, solver="pcg", ft=np.float64, cam_order=order, **kw), ref, F.start_of(p)) for order in (None, perm)]


def main():
    worst = 0.0
    for name, (V, T) in F.step_cases().items():
        p = F.step_problem(V, T)
        for n in F.STEP_COUNTS:
            ref = F.step_reference(p, n)
            d = legs(p, ref, force_accept=True, cg_iters=n, **dict(F.STEP_PARAMS, **F.step_kwargs(p)))
            worst = max(worst, *d)
            print("step   %-10s n = %d: list order %.3g, permuted %.3g (%d free poses, %d free focals, %d PCG iterations)" %
                  (name, n, d[0], d[1], ref["n_free_cams"], ref["n_free_focals"], ref["cg_iters_total"]))
    p, _ = F.list_shapes_problem()
    kw = dict(F.STEP_PARAMS, min_cam_obs=F.B.DEFAULTS["min_cam_obs"], min_focal_obs=F.LIST_MIN_FOCAL_OBS)
    ref = F.run(p, solver="pcg", force_accept=True, ft=np.longdouble, cg_iters=7, **kw)
    d = legs(p, ref, force_accept=True, cg_iters=7, **kw)
    worst = max(worst, *d)
    print("lists  n = 7: list order %.3g, permuted %.3g (%d free focals)" % (d[0], d[1], ref["n_free_focals"]))
    print("ROUNDOFF = %.3g" % worst)
    conv = 0.0
    for V, T, seed in F.CONVERGED_SCENES:
        p = F.make_problem(V=V, T=T, seed=seed)
        tr = []
        ref = F.run(p, solver="direct", trace=tr, iters=F.CONVERGED_PARAMS["iters"], min_cam_obs=F.CONVERGED_PARAMS["min_cam_obs"])
        d = legs(p, ref, **F.CONVERGED_PARAMS)
        conv = max(conv, *d)
        print("converged V = %d: gains %s, list order %.3g, permuted %.3g" % (V, [round(t["gain"], 3) for t in tr], d[0], d[1]))
    print("CONVERGED = %.3g" % conv)
    gap = 0.0
    for V, T, seed in F.CONVERGED_SCENES:
        p = F.make_problem(V=V, T=T, seed=seed)
        ref = F.run(p, solver="direct")
        for order in (None, np.random.default_rng(2).permutation(ref["n_obs"])):
            got = F.run(p, solver="pcg", cam_order=order)
            g = abs(got["cost_final"] - ref["cost_final"]) / ref["cost_final"]
            gap = max(gap, g)
            print("defaults V = %d: cost %.12g against %.12g, gap %.3g, %d / %d outer iterations, %d free focals" %
                  (V, got["cost_final"], ref["cost_final"], g, got["iters"], ref["iters"], ref["n_free_focals"]))
    print("DEFAULT_COST_GAP = %.3g" % gap)


if __name__ == "__main__":
    main()
