#!/usr/bin/env python3
"""The round-off bound of tests/test_transavg_steps.py, measured on the reference alone (CPU only).

For every graph and step count of that test, tests/transavg_pcg_ref.py is run twice: the longdouble n-step PCG on the
specification's system (the reference leg) and a float64 leg that follows the kernel's formulas -- closed-form adjugate
inverse, per-view sums over the adjacency in edge order, r -= alpha q, p = z + beta p -- once with the edges as given and
once with the edges permuted, so that another summation order is inside the figure.  Printed: max |c_f64 - c_ld| over the
views relative to the largest step max |c_ld - c0|.  Ten times the largest figure bounds the device in the fixed-step
tests (the factor of scripts/transavg_sensitivity.py; it covers the device's tree reductions and ocml sqrt and division
against libm).  A third float64 leg inverts the diagonal blocks with LAPACK instead: where its figure is much smaller the
adjugate dominates.

The second part is the converged regime (PGI_TRANSAVG_CG_TOL = 1e-11, delta = 1): the distance between irls_fixed at that
tolerance and the direct solves of tests/transavg_spec.py after three outer iterations, in the same measure."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import transavg_spec as TS  # noqa: E402
import transavg_pcg_ref as R  # noqa: E402


def f64_legs(g, c0, roots, **kw):
    """-> [(name, c, iters)]: edge order as given, permuted, and as given with LAPACK inverses."""
    perm = np.random.default_rng(1).permutation(len(g["src"]))
    legs = []
    for name, o, lapack in (("as given", slice(None), False), ("permuted", perm, False), ("lapack inverse", slice(None), True)):
        c, it, _ = R.mirror_irls_fixed(g["V"], g["src"][o], g["dst"][o], g["gamma"][o], g["w"][o], c0, roots,
                                       lapack_inverse=lapack, **kw)
        legs.append((name, c, it))
    return legs


def main():
    t0 = time.time()
    worst = {"as given": 0.0, "permuted": 0.0, "lapack inverse": 0.0}
    print("fixed-step parity and topologies (iters = 1): distance of the float64 legs to the longdouble reference")
    cases = [(name, g, R.STEP_COUNTS) for name, g in R.parity_graphs().items()]
    cases += [(name, g, (R.TOPOLOGY_STEPS,)) for name, g in R.topology_graphs().items()]
    for name, g, counts in cases:
        c0, ref = R.first_step_reference(g, counts)
        roots = TS.spanning_forest_init(g["V"], g["src"], g["dst"], g["gamma"], g["w"])[1]
        line = "%-18s" % name
        for n in counts:
            c_ref, ran = ref[n]
            d = {}
            for leg, c, _ in f64_legs(g, c0, roots, iters=1, cg_iters=n):
                d[leg] = R.distance(c, c_ref, c0)
                worst[leg] = max(worst[leg], d[leg])
            line += "  n=%d(%d): %.1e %.1e [%.1e]" % (n, ran, d["as given"], d["permuted"], d["lapack inverse"])
        print(line)
    print("fixed-step trajectory (iters = %(iters)d, cg_iters = %(cg_iters)d)" % R.TRAJECTORY)
    for name, g in R.trajectory_graphs().items():
        trace = []
        c_ref, it_ref = R.irls_fixed(g["V"], g["src"], g["dst"], g["gamma"], g["w"], trace=trace, **R.TRAJECTORY)
        c0, roots = TS.spanning_forest_init(g["V"], g["src"], g["dst"], g["gamma"], g["w"])
        margin = min(float(np.abs(t["a"] - 1.0).min()) for t in trace[1:])
        line = "%-18s iters %d, min |a - 1| from the second outer iteration on %.2e:" % (name, it_ref, margin)
        for leg, c, it in f64_legs(g, c0, roots, **R.TRAJECTORY):
            d = R.distance(c, c_ref, c0)
            worst[leg] = max(worst[leg], d)
            line += "  %s %.1e (iters %d)" % (leg, d, it)
        print(line)
    print("largest: " + ", ".join("%s %.3g" % kv for kv in worst.items()))
    figure = max(worst["as given"], worst["permuted"])
    print("ROUND-OFF FIGURE %.3g  ->  bound %.3g" % (figure, 10.0 * figure))

    print("converged regime (cg_tol %(cg_tol)g, delta %(delta)g, iters %(iters)d, cap %(cg_iters)d): irls_fixed against direct solves" % R.CONVERGED)
    worst_conv = 0.0
    for name, g in R.converged_graphs().items():
        trace = []
        c, it = R.irls_fixed(g["V"], g["src"], g["dst"], g["gamma"], g["w"], trace=trace, **R.CONVERGED)
        c_dir, it_dir = TS.translation_average(g["V"], g["src"], g["dst"], g["gamma"], g["w"], iters=R.CONVERGED["iters"],
                                               delta=R.CONVERGED["delta"])
        c0, _ = TS.spanning_forest_init(g["V"], g["src"], g["dst"], g["gamma"], g["w"])
        d = R.distance(c, c_dir, c0)
        worst_conv = max(worst_conv, d)
        print("%-18s PCG iterations %s, outer %d / %d, distance %.2e" % (name, [t["cg"] for t in trace], it, it_dir, d))
    print("CONVERGED FIGURE %.3g  ->  bound %.3g" % (worst_conv, 10.0 * worst_conv))
    print("%.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
