#!/usr/bin/env python3
"""The figures behind the constants of tests/test_chain_filtered.py, measured on the reference alone (CPU, no device).

The filtered chain scene of tests/chain_ref.py (make_filtered_scene: three estimated wrong edges, wrong nominal focals) goes
through the CPU oracle and the CPU specifications (chain_ref.reference_filtered_chain), with the cycle filter and without:
  * the input conditions: the twin records, the filter's decisions and its margin, the free views of the focal run;
  * against ground truth: rotation / centre / median point error after one similarity alignment and the RMS relative focal
    error, before the focal run, after it, and after re-triangulation at phi f_nominal plus the pose-only run.  The tests
    allow twice these figures;
  * seam 2': the sensitivity of the translation-averaging specification to inner solves stopped at the device's tolerance
    1e-4, on the kept edges;
  * seams 5' and 6': the float64 leg by the kernels' formulas (camera sums in list order and permuted) against the direct
    solves at defaults, for the focal run and for the pose-only run: final-cost gap and state_distance.
The round-off bounds of the tests are ten times the figures.

    python scripts/chain_filtered_roundoff.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "pose-graph-initialization_amd"))
import bundle_focal_spec as BF  # noqa: E402
import bundle_spec as B  # noqa: E402
import chain_ref as CR  # noqa: E402
import cycle_spec as CS  # noqa: E402
import transavg_spec as TA  # noqa: E402
from pyposegraphbuilder import synthetic as S  # noqa: E402
from transavg_sensitivity import cg_hook  # noqa: E402


def print_leg(name, scene, leg):
    fig = CR.leg_figures(scene, leg)
    tri, baf, ba2 = leg["tri"], leg["baf"], leg["ba2"]
    print("%s: %d edges, %d tracks, statuses %s then %s, purity %.6f, %d twin members" %
          (name, len(leg["graph"][0]), len(leg["tracks"]), tri["counts"].tolist(), leg["tri2"]["counts"].tolist(), fig["purity"],
           len(CR.has_twin_member(scene, leg["tracks"]))))
    for st, label in (("before", "before the focal run"), ("focal", "after the focal run"), ("final", "after re-triangulation + pose-only run")):
        e = fig[st]
        print("GROUND TRUTH  %-10s %-40s rotation %.4f deg, centre %.3e, median point %.3e (%d points)" %
              (name, label, e["rot_deg"], e["centre"], e["point"], e["n_points"]))
    print("GROUND TRUTH  %-10s RMS relative focal error over MAIN: %.4e before, %.4e after" % (name, fig["focal_before"], fig["focal_after"]))
    print("              focal run: cost %.6g -> %.6g, %d of %d steps accepted, %d free poses, %d free focals, %d observations, %d points; "
          "pose-only run: cost %.6g -> %.6g, %d of %d" %
          (baf["cost_initial"], baf["cost_final"], baf["accepted"], baf["iters"], baf["n_free_cams"], baf["n_free_focals"], baf["n_obs"],
           baf["n_points"], ba2["cost_initial"], ba2["cost_final"], ba2["accepted"], ba2["iters"]))
    return fig


def main():
    t0 = time.time()
    ref = CR.reference_filtered_chain()
    scene, est, cyc, kept = ref["scene"], ref["est"], ref["cyc"], ref["kept"]
    print("CPU legs in %.1f s; draw %d, FOCAL_ERR %g, n_twin %d, twin pairs %s, focal errors %s" %
          (time.time() - t0, CR.FILTERED_DRAW, CR.FOCAL_ERR, CR.N_TWIN, scene["twin_pairs"], np.round(scene["focal_e"][list(CR.MAIN)], 4).tolist()))
    for p, (s, d) in enumerate(scene["pairs"]):
        if (s, d) in scene["twin_pairs"]:
            m, tw = est["masks"][p].astype(bool), CR.twin_rows(scene, p, est["matches"][p])
            print("TWIN  pair %s: status %d, %.2f deg from the true relative rotation, %d rows (%d twin), mask %d (%d twin), n_tri %d, n_good %d, keep %d" %
                  ((s, d), est["edges"]["status"][p], S.rot_err_deg(est["edges"]["R"][p].reshape(3, 3), CR.true_relative_rotation(scene, s, d)),
                   len(m), tw.sum(), m.sum(), (m & tw).sum(), cyc["n_tri"][p], cyc["n_good"][p], cyc["keep"][p]))
    print("FILTER  %s, dropped %s, margin %.3e (CS.MARGIN %g)" %
          (cyc["summary"], [scene["pairs"][p] for p in np.nonzero(est["ok"] & ~kept)[0]], CS.margins(cyc["quantities"]), CS.MARGIN))
    print_leg("filtered", scene, ref["filtered"])
    print_leg("unfiltered", scene, ref["unfiltered"])

    leg = ref["filtered"]
    src, dst, _, _, w = leg["graph"]
    c, posed = leg["c"], leg["has_pose"]
    rms = np.sqrt(((c[posed] - c[posed].mean(0)) ** 2).sum(1).mean())
    for rtol in (1e-4, 1e-6, 1e-10):
        c2, _ = TA.translation_average(CR.N_VIEWS, src, dst, leg["gamma"], w, solve=cg_hook(rtol))
        print("SEAM 2'  inner solves stopped at %g: max |c - c_direct| / rms spread = %.3g" % (rtol, np.linalg.norm(c2 - c, axis=1).max() / rms))

    tb, mem = leg["track_begin"], leg["members"]
    runs = (("SEAM 5'", "focal run", leg["views"], leg["tri"], leg["baf"], BF.bundle_adjust, BF.state_distance,
             dict(R=leg["views"]["R"], c=leg["views"]["c"], X=leg["tri"]["X"], phi=np.ones(CR.N_VIEWS))),
            ("SEAM 6'", "pose-only run", leg["views2"], leg["tri2"], leg["ba2"], B.bundle_adjust, B.state_distance,
             dict(R=leg["views2"]["R"], c=leg["views2"]["c"], X=leg["tri2"]["X"])))
    for seam, what, views, tri, direct, solve, distance, start in runs:
        gap = dist = 0.0
        for name, order in (("list order", None), ("permuted", np.random.default_rng(2).permutation(direct["n_obs"]))):
            got = solve(tb, mem, views, tri["X"], tri["status"], tri["obs_state"], solver="pcg", cam_order=order)
            ga = abs(got["cost_final"] - direct["cost_final"]) / direct["cost_final"]
            d = distance(got, direct, start)
            gap, dist = max(gap, ga), max(dist, d)
            print("%s  %s, float64 PCG leg (%s) against direct solves: cost %.15g / %.15g, gap %.3g, state distance %.3g, outer %d / %d" %
                  (seam, what, name, got["cost_final"], direct["cost_final"], ga, d, got["iters"], direct["iters"]))
        print("%s  COST_GAP = %.3g, STATE_DISTANCE = %.3g" % (seam, gap, dist))
    print("%.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
