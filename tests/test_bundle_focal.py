"""Bundle adjustment with per-view focal scales (include/pgi.h: pgi_bundle_adjust_focal, pgi_tracklets_bundle_adjust_focal)
against its CPU specification tests/bundle_focal_spec.py.

The device is compared by bundle_focal_spec.state_distance: max |state - reference| over R, c, phi and the participating X,
relative to the largest move of the reference.  Every device bound comes from the reference alone
(scripts/bundle_focal_roundoff.py, CPU): the float64 leg that follows the kernels' formulas (7 x 7 blocks with the pinned
columns zero, camera sums in list order and permuted) against the longdouble leg.
  * ROUNDOFF = 1.22e-12: the largest figure over the fixed-step cases (1.2e-14 .. 3.6e-13 for 1 .. 65 active cameras at 300
    points, 1.22e-12 for a single point) and the list-shape problem (1.17e-13).
  * CONVERGED = 8.23e-13: cg_tol = 1e-13, three outer iterations against the direct solves (V = 12: 4.0e-13, V = 65: 8.23e-13).
  * DEFAULT_COST_GAP = 1.85e-10: relative gap of the final cost at defaults between the PCG leg and the direct solves
    (V = 12: 5.3e-15; V = 65: 1.85e-10, both legs at the limit of 20 outer iterations).
The bounds are ten times these.  The CPU bounds are ten times (scipy, noise-free) or twice (ground truth) what
test_spec_* print, recorded below and in DESIGN.md section 3, item 11.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bundle_focal_spec as F
import bundle_spec as B

ROUNDOFF = 1.22e-12
STEP_BOUND = 10.0 * ROUNDOFF
CONVERGED = 8.23e-13
CONVERGED_BOUND = 10.0 * CONVERGED
DEFAULT_COST_GAP = 1.85e-10
DEFAULT_COST_BOUND = 10.0 * DEFAULT_COST_GAP
# relative gap between the specification's final cost and scipy.optimize.least_squares' over the same unknowns (12 views,
# 120 tracks, 0.5 px noise, focals off by +-5 %, huber_px = inf, scipy with central differences), measured on the CPU
SCIPY_GAP_MEASURED = 1.57e-14
SCIPY_GAP_BOUND = 10.0 * SCIPY_GAP_MEASURED
# noise-free f64 pixels: RMS reprojection error (pixels) and max |phi fx0 - f_true| / f_true the specification reaches
NOISE_FREE_RMS_MEASURED = 8.44e-14    # from 11.1 px
NOISE_FREE_RMS_BOUND = 10.0 * NOISE_FREE_RMS_MEASURED
NOISE_FREE_FOCAL_MEASURED = 1.71e-15  # from 4.81e-2
NOISE_FREE_FOCAL_BOUND = 10.0 * NOISE_FREE_FOCAL_MEASURED
# 0.5 px noise: RMS relative focal error, RMS rotation error (degrees, mean rotation removed) and aligned centre error of
# the focal leg, measured; the bounds are twice these (ground-truth bounds as in tests/test_chain.py)
#   before     focal 3.28e-2, rotation 0.0999 deg, centres 0.0172
#   pose-only  focal 3.28e-2, rotation 0.52 deg,   centres 0.217     (it bends the poses to absorb the focal error)
#   focal      focal 3.34e-3, rotation 0.0425 deg, centres 0.0118
NOISY_FOCAL_MEASURED, NOISY_ROT_MEASURED, NOISY_CENTRE_MEASURED = 3.34e-3, 0.0425, 0.0118

REPORT = ("iters", "accepted", "cg_iters_total", "stop_reason", "n_obs", "n_points", "n_free_cams")
STEP_CASES = F.step_cases()


@functools.lru_cache(maxsize=None)
def step_problem(name):
    return F.step_problem(*STEP_CASES[name])


@functools.lru_cache(maxsize=None)
def step_reference(name, n):
    return F.step_reference(step_problem(name), n)


@functools.lru_cache(maxsize=None)
def lists():
    return F.list_shapes_problem()


LIST_KW = dict(F.STEP_PARAMS, min_cam_obs=B.DEFAULTS["min_cam_obs"], min_focal_obs=F.LIST_MIN_FOCAL_OBS, cg_iters=7)


@functools.lru_cache(maxsize=None)
def lists_reference():
    return F.run(lists()[0], solver="pcg", force_accept=True, ft=np.longdouble, **LIST_KW)


@functools.lru_cache(maxsize=None)
def noisy(V, T, seed):
    return F.make_problem(V=V, T=T, seed=seed)


@functools.lru_cache(maxsize=None)
def converged_reference(i):
    V, T, seed = F.CONVERGED_SCENES[i]
    trace = []
    ref = F.run(noisy(V, T, seed), solver="direct", trace=trace, iters=F.CONVERGED_PARAMS["iters"], min_cam_obs=F.CONVERGED_PARAMS["min_cam_obs"])
    return ref, trace


@functools.lru_cache(maxsize=None)
def default_reference(i):
    V, T, seed = F.CONVERGED_SCENES[i]
    return F.run(noisy(V, T, seed), solver="direct")


def early_stop_allowed(V, n, ran):
    """Fixed-step cases whose PCG may stop before n iterations: V = 2 (one 1 x 1 block, exact after one iterate) and V = 3 (two
    blocks with a rank-one coupling, exact after three)."""
    return (V == 2 and ran >= 1) or (V == 3 and ran >= min(n, 3))


def focal_errors(p, r):
    gt = p["views_gt"]
    f = np.asarray(r["phi"], np.float64) * p["views"]["K"][:, 0]
    return (float(np.sqrt((((f - gt["K"][:, 0]) / gt["K"][:, 0]) ** 2).mean())), F.rotation_error_deg(r["R"], gt["R"]),
            B.aligned_centre_error(np.asarray(r["c"], np.float64), gt["c"]))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_exports_and_null_arguments():
    from pyposegraphbuilder import _lib as L
    lib = L.load()
    for name in ("pgi_bundle_adjust_focal", "pgi_tracklets_bundle_adjust_focal"):
        assert hasattr(lib, name) and name in L.SYMBOLS, name
    z = None
    assert lib.pgi_bundle_adjust_focal(z, z, z, 0, z, z, z, z, z, 0, z, z, z, z, z, z, 0, z, z) < 0 and b"null context" in lib.pgi_last_error()
    assert lib.pgi_tracklets_bundle_adjust_focal(z, z, z, z, z, z, 0, z, z, z, z, z, z, 0, z, z) < 0 and b"null store" in lib.pgi_last_error()


def test_spec_against_scipy():
    """The specification run to convergence and scipy.optimize.least_squares over the same unknowns (poses, focal scales,
    points) from the same start reach the same cost.  scipy differentiates by central differences (jac="3-point"): with
    forward differences the error of its Jacobian, about 1e-8, decides in the last bits of the dense solves where it stops, and
    its final cost then scatters by more than the bound."""
    from scipy.optimize import least_squares
    p = F.make_problem(V=12, T=120, seed=1, noise_px=0.5, outlier_every=0)
    a = F.run(p, huber_px=np.inf, iters=50, ftol=1e-14)
    ob, ffree = a["ob"], a["ffree"]
    # (how the run ends at ftol = 1e-14, FTOL or LAMBDA, is decided by the last bits of the dense solves: not asserted)
    assert a["accepted"] > 0 and ob["cam_count"].min() >= 30 and a["n_free_cams"] == 11 and a["n_free_focals"] == 12
    cams, fc, pts = np.nonzero(ob["free"])[0], np.nonzero(ffree)[0], np.unique(ob["pt"])
    R0, c0, K0 = np.asarray(p["views"]["R"]).reshape(-1, 3, 3), np.asarray(p["views"]["c"]), p["views"]["K"]
    nC, nF = 6 * len(cams), len(fc)

    def residuals(x):
        R, c, phi, X = R0.copy(), c0.copy(), p["phi0"].copy(), p["X"].copy()
        d = x[:nC].reshape(-1, 6)
        R[cams] = B.rodrigues_update(R0[cams], d[:, :3])
        c[cams] = c0[cams] + d[:, 3:]
        phi[fc] = p["phi0"][fc] + x[nC:nC + nF]
        X[pts] = p["X"][pts] + x[nC + nF:].reshape(-1, 3)
        return F.linearize(R, c, K0, phi, X, ob, np.inf)["r"].reshape(-1)

    s = least_squares(residuals, np.zeros(nC + nF + 3 * len(pts)), method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
    gap = abs(2.0 * s.cost - a["cost_final"]) / a["cost_final"]
    print("cost %.15g, scipy %.15g, gap %.3g (bound %.3g)" % (a["cost_final"], 2.0 * s.cost, gap, SCIPY_GAP_BOUND))
    assert gap <= SCIPY_GAP_BOUND


def test_spec_noise_free_recovers_the_focals():
    p = F.make_problem(V=12, T=120, seed=1, noise_px=0.0, outlier_every=0, pixel_dtype=np.float64)
    a = F.run(p, huber_px=np.inf, iters=50)
    rms0, rms = np.sqrt(a["cost_initial"] / a["n_obs"]), np.sqrt(a["cost_final"] / a["n_obs"])
    f_gt = p["views_gt"]["K"][:, 0]
    # the scale of the scene is free, the focal is not: phi * fx0 is compared as it stands
    err0 = np.abs(p["phi0"] * p["views"]["K"][:, 0] - f_gt).max() / f_gt[0]
    err = np.abs(a["phi"] * p["views"]["K"][:, 0] - f_gt).max() / f_gt[0]
    print("noise-free: rms %.3g px -> %.3g px (bound %.3g); focal error %.3g -> %.3g (bound %.3g)" %
          (rms0, rms, NOISE_FREE_RMS_BOUND, err0, err, NOISE_FREE_FOCAL_BOUND))
    assert rms0 > 1.0 and err0 > 0.03 and a["n_free_focals"] == 12
    assert rms <= NOISE_FREE_RMS_BOUND and err <= NOISE_FREE_FOCAL_BOUND


def test_spec_noisy_beats_pose_only():
    """0.5 px noise, focals off by +-5 %: focal, rotation and aligned-centre error before, after the pose-only
    bundle_spec.bundle_adjust at the wrong focals, and after the focal refinement."""
    p = F.make_problem(V=12, T=120, seed=1, noise_px=0.5, outlier_every=0)
    wrong = dict(p, views=dict(p["views"], K=F.scaled_K(p["views"]["K"], p["phi0"])))
    start = dict(R=p["views"]["R"], c=p["views"]["c"], phi=p["phi0"])
    pose_only = dict(B.run(wrong, iters=50), phi=p["phi0"])
    focal = F.run(p, iters=50)
    legs = [focal_errors(p, r) for r in (start, pose_only, focal)]
    for name, e in zip(("before", "pose-only", "focal"), legs):
        print("%-9s focal %.3g, rotation %.3g deg, centres %.3g" % ((name,) + e))
    assert all(legs[2][k] < legs[1][k] for k in range(3))
    assert legs[2][0] <= 2.0 * NOISY_FOCAL_MEASURED and legs[2][1] <= 2.0 * NOISY_ROT_MEASURED and legs[2][2] <= 2.0 * NOISY_CENTRE_MEASURED


def test_spec_all_held_equals_pose_only_spec():
    """Every focal held: exactly bundle_spec.bundle_adjust on pre-scaled intrinsics (the direct solves; the 7 x 7 kernel
    formulas with a zero column differ from the 6 x 6 ones by round-off, which is why the device dispatches)."""
    p = F.make_problem(V=12, T=60, seed=1)
    scaled = dict(p, views=dict(p["views"], K=F.scaled_K(p["views"]["K"], p["phi0"])))
    for solver in ("direct",):
        want = B.run(scaled, solver=solver)
        for kw in (dict(focal_fixed=np.ones(12, bool)), dict(min_focal_obs=10 ** 6)):
            got = F.run(p, solver=solver, **kw)
            assert got["n_free_focals"] == 0 and np.array_equal(got["phi"], p["phi0"])
            assert all(np.array_equal(got[k], want[k]) for k in ("R", "c", "X")), solver
            assert all(got[k] == want[k] for k in REPORT + ("cost_initial", "cost_final", "lambda_final")), solver


def test_spec_focal_sign_rule():
    """A hand-made step through the decision function: phi_new > 0 fails (non-positive, NaN) -> cost +inf, rejected; the same
    step with a small focal change is accepted."""
    p = F.make_problem(V=12, T=60, seed=1, outlier_every=0)
    a = F.run(p, iters=0, min_focal_obs=1)
    ob, ffree, K0 = a["ob"], a["ffree"], p["views"]["K"]
    state = (a["R"], a["c"], a["phi"], a["X"])
    lin = F.linearize(*state[:2], K0, state[2], state[3], ob, 4.0)
    dcam, dpt = F.step_direct(lin, ob, ffree, 12, 60, 1e-4)
    good = F.trial(state, lin, ob, ffree, K0, dcam, dpt, lin["cost"], 4.0)
    assert good["accepted"] and np.isfinite(good["cost_new"])
    for bad in (-a["phi"][3], -a["phi"][3] - 0.25, np.nan):
        d = dcam.copy()
        d[3, 6] = bad
        t = F.trial(state, lin, ob, ffree, K0, d, dpt, lin["cost"], 4.0)
        assert not t["accepted"] and t["cost_new"] == np.inf, bad
    with pytest.raises(ValueError):
        F.run(p, focal=np.where(np.arange(12) == 3, 0.0, p["phi0"]))


def test_reference_conditions():
    """Conditions on the inputs, on the reference alone: active-camera counts, all four kinds of view in every fixed-step
    scene with more than three views, the step references run all n iterations, the list shapes, the gain margins."""
    for name, (V, T) in STEP_CASES.items():
        ref = step_reference(name, 7)
        free, ffree = ref["ob"]["free"], ref["ffree"]
        active = int((free | ffree).sum())
        if T == 300:
            assert active == V - 1 == int(name[1:].split("-")[0]), (name, active)
        if V > 3 and T > 1:
            kinds = {(bool(a), bool(b)) for a, b in zip(free, ffree)}
            assert len(kinds) == 4, (name, kinds)
            assert ffree[0] and not free[0] and (V == 4 or (ffree[3] and not free[3]))   # the gauge view, a fixed view: focal only
        if T == 300 and V == 3:
            # two blocks, a 1 x 1 (view 0: focal only) and a 7 x 7 (view 1), coupled by a block of rank one: the preconditioned
            # system has three distinct eigenvalues, so three iterates solve it and what follows is round-off
            assert (int(free.sum()), int(ffree.sum())) == (1, 2) and ffree[0] and free[1] and ffree[1]
        if T == 300 and V == 2:
            assert (int(free.sum()), int(ffree.sum())) == (0, 1)   # a single 1 x 1 block: the first iterate solves it
        for n in F.STEP_COUNTS:
            ran = step_reference(name, n)["cg_iters_total"]
            assert ran == n or early_stop_allowed(V, n, ran), (name, n, ran)
    p, idx = lists()
    ref = lists_reference()
    cnt = ref["ob"]["cam_count"]
    assert cnt[idx["one_pass"]] == 64 and cnt[idx["two_pass"]] == 65 and cnt[idx["at_min"]] == 30 and cnt[idx["below_min"]] == 29
    assert ref["ffree"][idx["at_min"]] and not ref["ffree"][idx["below_min"]] and ref["ob"]["free"][idx["below_min"]]
    assert ref["ffree"][0] and not ref["ob"]["free"][0] and not ref["ffree"][305] and not ref["ffree"][idx["held"]]
    lengths = np.diff(p["track_begin"].astype(np.int64))
    assert lengths.min() == 2 and lengths.max() == 70 and not p["views"]["has_pose"][305]
    for i in range(len(F.CONVERGED_SCENES)):
        ref, trace = converged_reference(i)
        assert len(trace) == 3 and all(abs(t["gain"] - B.ACCEPT_RATIO) >= B.GAIN_MARGIN for t in trace), [t["gain"] for t in trace]
        assert ref["n_free_focals"] > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


def upload(eng, views, K=None):
    K = views["K"] if K is None else K
    return [eng.upload_keypoints(np.asarray(views["xy"][i], np.float32).reshape(-1, 2), K[i][0], 2.0 * K[i][2], 2.0 * K[i][3])
            for i in range(len(views["xy"]))]


def device_run(eng, p, kps=None, force=False, **kw):
    v = p["views"]
    kw.setdefault("focal", p["phi0"])
    if force:
        os.environ["PGI_BUNDLE_FORCE_ACCEPT"] = "1"
    try:
        r = eng.bundle_adjust(p["track_begin"], p["members"], kps or upload(eng, v), v["R"], v["c"], p["X"], p["status"], p["obs_state"],
                              has_pose=v.get("has_pose"), refine_focal=True, **kw)
    finally:
        os.environ.pop("PGI_BUNDLE_FORCE_ACCEPT", None)
    return r


def as_state(r):
    return dict(R=r.R, c=r.c, X=r.X.cpu().numpy(), phi=r.focal)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def same_result(a, b):
    return (same_bits(a.R, b.R) and same_bits(a.c, b.c) and same_bits(a.X.cpu().numpy(), b.X.cpu().numpy()) and a.report() == b.report())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_hip_fixed_step_parity(eng, name):
    """iters = 1, cg_iters = n, acceptance forced: the state after the n-th PCG iterate of the first damped system."""
    p = step_problem(name)
    kps = upload(eng, p["views"])
    V = STEP_CASES[name][0]
    for n in F.STEP_COUNTS:
        ref = step_reference(name, n)
        got = device_run(eng, p, kps, force=True, cg_iters=n, **dict(F.STEP_PARAMS, **F.step_kwargs(p)))
        d = F.state_distance(as_state(got), ref, F.start_of(p))
        print("%s n = %d: %.3g (bound %.3g), %d PCG iterations" % (name, n, d, STEP_BOUND, got.cg_iters_total))
        assert (got.iters, got.accepted) == (1, 1)
        # one block, or two coupled by a rank-one block (test_reference_conditions): solved early, the rest is round-off
        assert got.cg_iters_total == ref["cg_iters_total"] == n or early_stop_allowed(V, n, got.cg_iters_total)
        assert (got.n_obs, got.n_points, got.n_free_cams, got.n_free_focals) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"], ref["n_free_focals"])
        assert d <= STEP_BOUND
        held = ~ref["ffree"]
        assert same_bits(got.focal[held], p["phi0"][held]) and not np.any(got.focal[~held] == p["phi0"][~held])


@pytest.mark.gpu
def test_hip_list_shapes(eng):
    p, idx = lists()
    ref = lists_reference()
    got = device_run(eng, p, None, force=True, **LIST_KW)
    d = F.state_distance(as_state(got), ref, F.start_of(p))
    print("list shapes: %.3g (bound %.3g)" % (d, STEP_BOUND))
    assert (got.n_obs, got.n_points, got.n_free_cams, got.n_free_focals, got.cg_iters_total) == \
        (ref["n_obs"], ref["n_points"], ref["n_free_cams"], ref["n_free_focals"], 7)
    assert d <= STEP_BOUND
    held = ~ref["ffree"]
    assert held[idx["below_min"]] and held[305] and held[100:].all() and not held[idx["at_min"]] and not held[0]
    assert same_bits(got.focal[held], p["phi0"][held]) and p["phi0"][305] < 0   # the unposed view's bad phi included
    assert got.focal[idx["at_min"]] != p["phi0"][idx["at_min"]] and got.focal[0] != p["phi0"][0]
    R0, c0 = np.asarray(p["views"]["R"]).reshape(-1, 3, 3), np.asarray(p["views"]["c"])
    pose_held = ~ref["ob"]["free"]
    assert same_bits(got.R[pose_held], R0[pose_held]) and same_bits(got.c[pose_held], c0[pose_held])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(F.CONVERGED_SCENES)))
def test_hip_converged_regime(eng, i):
    V, T, seed = F.CONVERGED_SCENES[i]
    p = noisy(V, T, seed)
    ref, _ = converged_reference(i)
    got = device_run(eng, p, **F.CONVERGED_PARAMS)
    d = F.state_distance(as_state(got), ref, F.start_of(p))
    print("converged V = %d: %.3g (bound %.3g), %d PCG iterations" % (V, d, CONVERGED_BOUND, got.cg_iters_total))
    assert (got.iters, got.accepted) == (ref["iters"], ref["accepted"]) == (3, 3)
    assert d <= CONVERGED_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(F.CONVERGED_SCENES)))
def test_hip_end_to_end_defaults_and_repeatability(eng, i):
    V, T, seed = F.CONVERGED_SCENES[i]
    p = noisy(V, T, seed)
    ref = default_reference(i)
    kps = upload(eng, p["views"])
    got, again = device_run(eng, p, kps), device_run(eng, p, kps)
    gap = abs(got.cost_final - ref["cost_final"]) / ref["cost_final"]
    print("defaults V = %d: cost %.15g against %.15g, gap %.3g (bound %.3g); %s, %d free focals" %
          (V, got.cost_final, ref["cost_final"], gap, DEFAULT_COST_BOUND, got.report(), got.n_free_focals))
    assert (got.n_obs, got.n_points, got.n_free_cams, got.n_free_focals) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"], ref["n_free_focals"])
    assert (got.iters, got.accepted, got.stop_reason) == (ref["iters"], ref["accepted"], ref["stop_reason"])
    assert got.n_free_focals > 0 and got.cost_initial >= got.cost_final and got.accepted > 0
    assert gap <= DEFAULT_COST_BOUND
    assert same_result(got, again) and same_bits(got.focal, again.focal)
    # the inputs are not modified
    assert got.focal is not p["phi0"] and not same_bits(got.focal, p["phi0"])


@pytest.mark.gpu
def test_hip_all_held_dispatch_is_bit_exact(eng):
    """No focal-free view: the bits of pgi_bundle_adjust on views whose fx, fy were multiplied on the host."""
    p = noisy(12, 120, 1)
    v = p["views"]
    kps = upload(eng, v)
    for phi in (np.ones(12), p["phi0"]):
        scaled = upload(eng, v, F.scaled_K(v["K"], phi))
        want = eng.bundle_adjust(p["track_begin"], p["members"], scaled, v["R"], v["c"], p["X"], p["status"], p["obs_state"])
        for kw in (dict(focal_fixed=np.ones(12, bool)), dict(min_focal_obs=10 ** 6)):
            got = device_run(eng, p, kps, focal=phi, **kw)
            assert got.n_free_focals == 0 and same_bits(got.focal, phi) and got.accepted > 0
            assert same_result(got, want)
    # focal=None is phi = 1
    plain = eng.bundle_adjust(p["track_begin"], p["members"], kps, v["R"], v["c"], p["X"], p["status"], p["obs_state"])
    assert same_result(device_run(eng, p, kps, focal=None, focal_fixed=np.ones(12, bool)), plain)


@pytest.mark.gpu
def test_hip_store_path(eng):
    """DeviceTracklets.bundle_adjust(refine_focal=True) gives the bits of the array call on the same tracks."""
    from pyposegraphbuilder.engine import DeviceTracklets
    import triangulate_spec as TS
    p = noisy(12, 120, 1)
    v = p["views"]
    kps = upload(eng, v)
    tb = p["track_begin"]
    calls = {}
    for t in range(len(tb) - 1):
        m = p["members"][tb[t]:tb[t + 1]]
        for a, b in zip(m[:-1], m[1:]):
            va, vb = int(a >> np.uint64(32)), int(b >> np.uint64(32))
            calls.setdefault((va, vb), []).append((int(a & np.uint64(0xFFFFFFFF)), int(b & np.uint64(0xFFFFFFFF))))
    store = DeviceTracklets(eng, 12)
    store.add_batch([(s, d, np.array(m), None) for (s, d), m in sorted(calls.items())])
    n = store.info()["tracks"]
    tri = store.triangulate(upload(eng, v, F.scaled_K(v["K"], p["phi0"])), v["R"], v["c"], **F.FOCAL_TRI)
    got = store.bundle_adjust(kps, v["R"], v["c"], tri.X, tri.status, tri.obs_state, focal=p["phi0"], refine_focal=True)
    tracks = [store.track(i) for i in range(n)]
    tb2 = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32)
    mem2 = np.array([TS.pack(a, b) for t in tracks for a, b in t], np.uint64)
    direct = eng.bundle_adjust(tb2, mem2, kps, v["R"], v["c"], tri.X, tri.status, tri.obs_state, focal=p["phi0"], refine_focal=True)
    assert got.n_points >= 100 and got.accepted > 0 and got.n_free_focals == direct.n_free_focals == 12
    assert same_result(got, direct) and same_bits(got.focal, direct.focal) and not same_bits(got.focal, p["phi0"])
    store.close()


@pytest.mark.gpu
def test_hip_errors(eng):
    from pyposegraphbuilder import _lib as L
    p = noisy(12, 120, 1)
    v = p["views"]
    kps = upload(eng, v)
    for bad in (0.0, -1.0, np.nan, np.inf):
        phi = p["phi0"].copy()
        phi[4] = bad
        with pytest.raises(L.PgiError, match="focal scale"):
            device_run(eng, p, kps, focal=phi)
    with pytest.raises(ValueError):
        device_run(eng, p, kps, focal=np.ones(11))
    # focal / focal_fixed without refine_focal would be ignored: refused
    for kw in (dict(focal=p["phi0"]), dict(focal_fixed=np.ones(12, bool))):
        with pytest.raises(ValueError, match="refine_focal"):
            eng.bundle_adjust(p["track_begin"], p["members"], kps, v["R"], v["c"], p["X"], p["status"], p["obs_state"], **kw)
    # a bad phi on a view without a pose is accepted (and comes back untouched)
    has = np.ones(12, bool)
    has[11] = False
    phi = p["phi0"].copy()
    phi[11] = np.nan
    q = dict(p, views=dict(v, has_pose=has))
    got = device_run(eng, q, kps, focal=phi)
    ref = F.run(q, focal=phi)
    assert got.accepted > 0 and np.isnan(got.focal[11]) and got.n_free_focals == ref["n_free_focals"] == 11
    assert abs(got.cost_final - ref["cost_final"]) / ref["cost_final"] <= DEFAULT_COST_BOUND
    # NULL h_focal through the C entry: PGI_ERR_INVALID, nothing written
    args, (Rh, ch, Xd, rep), keep = eng._bundle_args(kps, v["R"], v["c"], p["X"], p["status"], p["obs_state"], None, None,
                                                     len(p["track_begin"]) - 1, len(p["members"]), {})
    tb = eng_tensor(eng, p["track_begin"], np.uint32, np.int32)
    mem = eng_tensor(eng, p["members"], np.uint64, np.int64)
    n = C.c_uint32(77)
    R_before, X_before = Rh.copy(), Xd.cpu().numpy().copy()
    rc = eng._lib.pgi_bundle_adjust_focal(eng._ctx, C.c_void_p(tb.data_ptr()), C.c_void_p(mem.data_ptr()), len(p["track_begin"]) - 1,
                                          *(args[:-1] + (None, None, 30, args[-1], C.byref(n))))
    assert rc == -1 and b"null focal" in eng._lib.pgi_last_error()
    assert n.value == 77 and same_bits(Rh, R_before) and same_bits(Xd.cpu().numpy(), X_before)


def eng_tensor(eng, a, dtype, view):
    import torch
    return torch.from_numpy(np.array(a, dtype).view(view)).to(eng.device)
