#!/usr/bin/env python3
"""How far inexact inner solves move the translation averaging (CPU only, tests/transavg_spec.py alone).

The active-set switch makes the outer iteration discontinuous, so the distance between the device solver (truncated PCG)
and the specification (direct solves) is not round-off.  This runs the specification on the five graphs of
tests/test_transavg.py with its direct solve and again with scipy CG on the step system stopped at several relative
residuals, and prints the largest position difference relative to the RMS spread of the positions.  The figure at 1e-4
(the device's inner tolerance) times ten is the bound of test_hip_matches_spec; DESIGN.md section 3 item 9 records it."""
import os
import sys

import numpy as np
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import transavg_spec as TS  # noqa: E402

CASES = [(12, 3, 0.5, 0.1, 1), (40, 5, 0.0, 0.0, 1), (50, 6, 1.0, 0.15, 1), (30, 4, 0.5, 0.1, 3), (340, 20, 1.0, 0.2, 1)]


def cg_hook(rtol):
    def solve(A, b, x0):
        d, _ = spla.cg(A, b - A @ x0, rtol=rtol, atol=0.0, maxiter=5000)
        return x0 + d
    return solve


def main():
    worst = {}
    for (V, k, noise, outl, comps) in CASES:
        src, dst, gam, w, c_gt, _ = TS.make_graph(V, k, noise, outl, seed=V, components=comps)
        c, iters = TS.translation_average(V, src, dst, gam, w)
        rms = np.sqrt(((c - c.mean(0)) ** 2).sum(1).mean())
        err = TS.align_error(c, c_gt, np.arange(V) % comps)
        line = "V = %3d, %4d edges, %d iterations, median error %.3g:" % (V, len(src), iters, np.median(err))
        for rtol in (1e-4, 1e-6, 1e-10):
            c2, _ = TS.translation_average(V, src, dst, gam, w, solve=cg_hook(rtol))
            d = float(np.linalg.norm(c2 - c, axis=1).max() / rms)
            worst[rtol] = max(worst.get(rtol, 0.0), d)
            line += "  cg %g -> %.3g" % (rtol, d)
        print(line)
    print("largest:", ", ".join("%g -> %.3g" % kv for kv in sorted(worst.items(), reverse=True)))


if __name__ == "__main__":
    main()
