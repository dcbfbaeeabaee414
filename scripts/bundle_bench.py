"""Bundle adjustment at scale (not part of bench.py): the scene of scripts/triangulate_bench.py (10^6 tracks over 5000 views)
with its ground-truth poses perturbed, triangulated on the device, then refined.  Reports the time per Levenberg-Marquardt
iteration at defaults, the time per PCG iteration (HIP events around calls of iters = 1 that differ only in cg_iters,
acceptance forced, median of the warm calls), the algorithmic bytes of the two matvec passes over that time as a fraction of
the HBM peak, and the PCG iteration count of every outer step (PGI_BUNDLE_TRACE lines on stderr).  --focal: the same with
every view's focal scale among the unknowns (pgi_bundle_adjust_focal, phi = 1 at the start: the seven-parameter kernels).
--lm-calls repeats the call at defaults, so that the run-to-run spread of both figures is printed with them.

    python scripts/bundle_bench.py [--tracks 1000000] [--views 5000] [--calls 5] [--iters 6] [--lm-calls 1] [--focal]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pose-graph-initialization_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HBM_PEAK = 8.0e12  # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--views", type=int, default=5000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rot-deg", type=float, default=0.02)
    ap.add_argument("--centre-sigma", type=float, default=0.005)
    ap.add_argument("--lm-calls", type=int, default=1)
    ap.add_argument("--focal", action="store_true")
    a = ap.parse_args()
    import torch
    import triangulate_spec as TS
    from pyposegraphbuilder import Engine
    from triangulate_bench import make
    tb, mem, views, length = make(a.tracks, a.views)
    rng = np.random.default_rng(1)
    V = a.views
    R0 = TS._rodrigues(rng.standard_normal((V, 3)) * np.deg2rad(a.rot_deg)) @ views["R"]
    c0 = views["c"] + rng.standard_normal((V, 3)) * a.centre_sigma
    eng = Engine()
    kps = [eng.upload_keypoints(views["xy"][v], 1000.0, 2000.0, 2000.0) for v in range(V)]
    d_tb = torch.from_numpy(tb.view(np.int32)).to(eng.device)
    d_mem = torch.from_numpy(mem.view(np.int64)).to(eng.device)
    tri = eng.triangulate_tracks(d_tb, d_mem, kps, R0, c0, thr_px=8.0)
    print("tracks %d, members %d, views %d; triangulated from the perturbed poses: %s" %
          (a.tracks, len(mem), V, dict(zip(("OK", "TOO_FEW", "DEGENERATE", "BEHIND", "REPROJ", "LOW_PARALLAX"), tri.counts.tolist()))))

    def call(**kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if a.focal:
            kw.update(refine_focal=True, min_focal_obs=30)
        r = eng.bundle_adjust(d_tb, d_mem, kps, R0, c0, tri.X, tri.status, tri.obs_state, **kw)
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1)

    # (1) defaults, a fixed number of outer iterations, traced
    os.environ["PGI_BUNDLE_TRACE"] = "1"
    r, ms = call(iters=a.iters)
    os.environ.pop("PGI_BUNDLE_TRACE")
    lm = [ms / max(r.iters, 1)] + [call(iters=a.iters)[1] / max(r.iters, 1) for _ in range(a.lm_calls - 1)]
    if a.focal:
        print("focal scales: %d focal-free views" % r.n_free_focals)
    N, T = r.n_obs, r.n_points
    print("defaults, %d outer iterations: %s" % (a.iters, r.report()))
    print("whole call %.1f ms (preparation, upload of %d view records and Python's marshalling included) = %.1f ms per outer iteration; "
          "%.1f PCG iterations per outer step (cap %d%s)" % (ms, V, ms / max(r.iters, 1), r.cg_iters_total / max(r.iters, 1), 200,
                                                             ": it binds" if r.cg_iters_total >= 200 * r.iters else ""))
    if len(lm) > 1:
        print("ms per outer iteration over %d calls (the first is cold): %s; warm median %.2f, warm spread %.2f .. %.2f" %
              (len(lm), " ".join("%.2f" % x for x in lm), np.median(lm[1:]), min(lm[1:]), max(lm[1:])))
    # (2) one PCG iteration: calls that differ only in the number of iterations
    os.environ["PGI_BUNDLE_FORCE_ACCEPT"] = "1"
    n_lo, n_hi = 8, 40
    t = {n_lo: [], n_hi: []}
    for i in range(a.calls + 1):
        for n in (n_lo, n_hi):
            rr, ms = call(iters=1, cg_iters=n, cg_tol=1e-30)
            assert rr.cg_iters_total == n
            if i:
                t[n].append(ms)
    os.environ.pop("PGI_BUNDLE_FORCE_ACCEPT")
    per = (np.median(t[n_hi]) - np.median(t[n_lo])) / (n_hi - n_lo)
    # per observation and pass: w, J_w, J_p (13 doubles) and one index; per track: two offsets' worth, V^-1 read, t written and
    # read again; per view: p read twice, q written, the damping diagonal
    nc, rec = (7, 15) if a.focal else (6, 13)   # the focal column adds two streamed doubles per observation and pass
    bytes_alg = 2 * N * (rec * 8 + 4) + a.tracks * 4 + T * (48 + 24 + 24) + V * (8 * nc * 4 + 8)
    each = (np.array(t[n_hi]) - np.array(t[n_lo])) / (n_hi - n_lo)
    print("PCG iteration, call pair by call pair: %s ms (spread %.4f .. %.4f)" % (" ".join("%.4f" % x for x in each), each.min(), each.max()))
    print("PCG iteration: %.3f ms (median of %d warm calls at %d and %d iterations: %.1f / %.1f ms); the two matvec passes move %.1f MB "
          "-> %.1f GB/s = %.1f %% of the HBM peak (%.0f GB/s)" % (per, a.calls, n_lo, n_hi, np.median(t[n_lo]), np.median(t[n_hi]),
                                                                   bytes_alg / 1e6, bytes_alg / per / 1e6, 100.0 * bytes_alg / (per * 1e-3) / HBM_PEAK,
                                                                   HBM_PEAK / 1e9))
    eng.close()


if __name__ == "__main__":
    main()
