#!/usr/bin/env python3
"""The round-off bounds of tests/test_rotavg_steps.py, measured on the reference alone (CPU only).

For every graph, phase, path and step count of that test, tests/rotavg_pcg_ref.py is run twice: the longdouble leg (the
reference) and a float64 leg that follows the kernels' formulas -- Shepperd-branch log, exp with the series below 1e-6,
per-view sums over the incidences in edge order and again with the edges permuted, the plain recurrences and (Jacobi,
two-level) the Chronopoulos-Gear form with the neighbours' z rebuilt, the tree solve by two prefix sums, Ac^-1 by
Gauss-Jordan without pivoting.  Both legs start from their OWN initialisation (float64 / longdouble products along the
forest), so the L1 first step carries the forest edges' round-off residuals (~1e-16, weight w / 1e-4) in its float64 leg.
Printed per case family: the largest  max_k |R_k - R_ref,k|_max / max_k |x_k|.  Ten times that bounds the device.

Families: init (absolute, the forest products), planted / planted-tiny (converged solve of the tiny graphs against the
direct solve), one / many / tree / two per step count (fixed step), pair (plain against Chronopoulos-Gear leg on the graphs
run on both Jacobi paths), trajectory per path, converged (PGI_ROTAVG_CG_TOL = 1e-12, no cap, against the direct solve)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import rotavg_pcg_ref as R  # noqa: E402

NO_CAP = 2000


def legs(path, many=False):
    """(permuted, cg_form) of the float64 legs that apply to a path."""
    if path == "tree":
        return [(False, False), (True, False)]
    if path == "two" or many:
        return [(False, True), (True, True), (False, False)]
    return [(False, False), (True, False), (False, True)]


def fixed_step(family, graphs, path, worst, many=False):
    for name, g in graphs.items():
        perm = np.random.default_rng(1).permutation(len(g["src"]))
        for phase in R.PHASES:
            _, ref = R.step_rotations(g, phase, R.STEP_COUNTS, path)
            line = "%-10s %-12s %-4s" % (family, name, phase)
            for n in R.STEP_COUNTS:
                x, R_ref, ran = ref[n]
                d = 0.0
                for permuted, cg in legs(path, many):
                    _, Rm, _, _ = R.mirror_rotations(g, [phase], n, path, perm=perm if permuted else None, cg_form=cg)
                    d = max(d, R.distance(Rm, R_ref, x))
                key = "%s/%d" % (family, n)
                worst[key] = max(worst.get(key, 0.0), d)
                line += "  n=%d(%s): %.1e" % (n, "".join(str(int(r)) if r < 10 else "+" for r in ran) if min(ran) < n else "all", d)
            print(line, flush=True)


def main():
    t0 = time.time()
    worst = {}
    g = R.init_graph()
    F = R.forest(g["V"], g["src"], g["dst"], g["w"])
    worst["init"] = float(np.abs(R.forest_rotations(F, g["Rrel"], np.float64) - R.forest_rotations(F, g["Rrel"])).max())
    chain = R.path_with_closures(1025, seed=1025)
    Fc = R.forest(chain["V"], chain["src"], chain["dst"], chain["w"])
    dc = float(np.abs(R.forest_rotations(Fc, chain["Rrel"], np.float64) - R.forest_rotations(Fc, chain["Rrel"])).max())
    print("init: forest depth %d: %.2e (absolute); a chain of depth %d: %.2e" % (F["depth"].max(), worst["init"], Fc["depth"].max(), dc))

    for name, g in R.planted_graphs().items():
        fam = "planted-tiny" if name in R.PLANTED_TINY else "planted"
        for phase in R.PHASES:
            _, x, R_ref = R.converged_step(g, phase)
            d = 0.0
            for permuted, cg in legs("jacobi"):
                perm = np.random.default_rng(1).permutation(len(g["src"])) if permuted else None
                _, Rm, _, ran = R.mirror_rotations(g, [phase], NO_CAP, "jacobi", perm=perm, cg_form=cg)
                d = max(d, R.distance(Rm, R_ref, x))
            worst[fam] = max(worst.get(fam, 0.0), d)
            print("%-12s %-20s %-4s |x| %.2e  PCG iterations %s  %.1e" % (fam, name, phase, R.step_scale(x), list(ran[0]), d), flush=True)

    fixed_step("one", R.one_wg_graphs(), "jacobi", worst)
    fixed_step("many", R.many_wg_graphs(), "jacobi", worst, many=True)
    fixed_step("tree", R.tree_graphs(), "tree", worst)
    fixed_step("two", R.two_level_graphs(), "two", worst)

    one = R.one_wg_graphs()
    for name in R.SHARED_ONE_MANY:
        for phase in R.PHASES:
            for n in R.STEP_COUNTS:
                _, ref = R.step_rotations(one[name], phase, (n,), "jacobi")
                _, Ra, _, _ = R.mirror_rotations(one[name], [phase], n, "jacobi")
                _, Rb, _, _ = R.mirror_rotations(one[name], [phase], n, "jacobi", cg_form=True)
                d = R.distance(Ra, Rb.astype(R.LD), ref[n][0])
                worst["pair"] = max(worst.get("pair", 0.0), d)
    print("pair: plain against Chronopoulos-Gear leg on %s: %.2e" % (", ".join(R.SHARED_ONE_MANY), worst["pair"]), flush=True)

    phases = ["l1"] * R.TRAJECTORY["l1_iters"] + ["irls"] * R.TRAJECTORY["irls_iters"]
    for name, (path, g) in R.trajectory_graphs().items():
        _, R_ref, scale, ran = R.trajectory(g, path, **R.TRAJECTORY)
        perm = np.random.default_rng(1).permutation(len(g["src"]))
        d = 0.0
        for permuted, cg in legs(path, name == "many"):
            _, Rm, _, _ = R.mirror_rotations(g, phases, R.TRAJECTORY["cg_iters"], path, perm=perm if permuted else None, cg_form=cg)
            d = max(d, R.distance(Rm, R_ref, scale))
        worst["trajectory/" + name] = d
        print("trajectory %-6s PCG iterations %s  %.1e" % (name, [list(r) for r in ran], d), flush=True)

    for name, (path, g) in R.converged_graphs().items():
        perm = np.random.default_rng(1).permutation(len(g["src"]))
        for phase in R.PHASES:
            _, x, R_ref = R.converged_step(g, phase)
            d = 0.0
            for permuted, cg in legs(path):
                _, Rm, _, ran = R.mirror_rotations(g, [phase], NO_CAP, path, tol=R.CONVERGED_TOL, perm=perm if permuted else None, cg_form=cg)
                d = max(d, R.distance(Rm, R_ref, x))
            worst["converged"] = max(worst.get("converged", 0.0), d)
            print("converged %-16s %-4s PCG iterations %s  %.1e" % (name, phase, list(ran[0]), d), flush=True)

    print("ROUNDOFF = {\n" + "".join('    "%s": %.3g,\n' % kv for kv in worst.items()) + "}")
    print("%.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
