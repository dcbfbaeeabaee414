"""Bundle adjustment (include/pgi.h: pgi_bundle_adjust, pgi_tracklets_bundle_adjust) against its CPU specification
tests/bundle_spec.py.

The device is compared by bundle_spec.state_distance: max |state - reference| over R, c and the participating X, relative
to the largest move of the reference (no alignment).  Every bound comes from the reference alone
(scripts/bundle_roundoff.py, CPU): a float64 leg that follows the kernels' formulas (adjugate inverse, 6 x 6 Cholesky,
per-point sums in member order, per-camera sums in list order and in a permuted order) against the longdouble leg.
  * ROUNDOFF = 3.0e-12: the largest figure over the fixed-step cases (4.3e-14 .. 1.3e-13 for 2 .. 65 free cameras at 300
    points, 2.0e-12 for one free camera, 3.0e-12 for a single point) and the list-shape problem (6.4e-14).
  * CONVERGED = 5.75e-13: cg_tol = 1e-13, three outer iterations against the direct solves (V = 12: 3.8e-13, V = 65: 5.75e-13).
  * DEFAULT_COST_GAP = 1.68e-10: relative gap of the final cost at defaults between the PCG leg (cg_tol = 1e-6) and the
    direct solves: 1.1e-15 on the 12-view scene, which converges in 8 outer iterations, and 1.68e-10 on the 65-view scene,
    where the planted 47 px observations make the IRLS run into the limit of 20 outer iterations in both legs.
The bounds are ten times these.
Measured on the MI355X: fixed steps 2.7e-14 .. 1.8e-12, list shapes 5.3e-14, converged regime 4.1e-13 / 4.6e-13, cost gap at
defaults 8.5e-16 / 1.68e-10.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bundle_spec as B
import triangulate_spec as TS

ROUNDOFF = 3.0e-12
STEP_BOUND = 10.0 * ROUNDOFF
CONVERGED = 5.75e-13
CONVERGED_BOUND = 10.0 * CONVERGED
DEFAULT_COST_GAP = 1.68e-10
DEFAULT_COST_BOUND = 10.0 * DEFAULT_COST_GAP
# relative gap between the specification's final cost and scipy.optimize.least_squares' on the same residuals from the
# same start (12 views, 60 tracks, 0.5 px noise, no outliers, huber_px = inf), measured on the CPU: 2.54e-15
SCIPY_GAP_MEASURED = 2.54e-15
SCIPY_GAP_BOUND = 10.0 * SCIPY_GAP_MEASURED
# RMS reprojection error (pixels) the specification reaches from perturbed poses on exact f64 pixels, measured: 8.27e-14
NOISE_FREE_RMS_MEASURED = 8.27e-14
NOISE_FREE_RMS_BOUND = 10.0 * NOISE_FREE_RMS_MEASURED

REPORT = ("iters", "accepted", "cg_iters_total", "stop_reason", "n_obs", "n_points", "n_free_cams")
STEP_CASES = B.step_cases()


def start_of(p):
    return dict(R=p["views"]["R"], c=p["views"]["c"], X=p["X"])


@functools.lru_cache(maxsize=None)
def step_problem(name):
    return B.step_problem(*STEP_CASES[name])


@functools.lru_cache(maxsize=None)
def step_reference(name, n):
    return B.step_reference(step_problem(name), n)


@functools.lru_cache(maxsize=None)
def lists():
    return B.list_shapes_problem()


@functools.lru_cache(maxsize=None)
def lists_reference():
    return B.step_reference(lists()[0], 7, min_cam_obs=B.DEFAULTS["min_cam_obs"])


@functools.lru_cache(maxsize=None)
def noisy(V, T, seed, outliers=False):
    return B.make_problem(V=V, T=T, seed=seed, **(dict(tri=B.OUTLIER_TRI) if outliers else {}))


@functools.lru_cache(maxsize=None)
def converged_reference(i):
    V, T, seed = B.CONVERGED_SCENES[i]
    trace = []
    ref = B.run(noisy(V, T, seed), solver="direct", trace=trace, iters=B.CONVERGED_PARAMS["iters"], min_cam_obs=B.CONVERGED_PARAMS["min_cam_obs"])
    return ref, trace


@functools.lru_cache(maxsize=None)
def default_reference(i):
    V, T, seed = B.DEFAULT_SCENES[i]
    return B.run(noisy(V, T, seed, True), solver="direct")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_exports_defaults_and_null_arguments():
    import pyposegraphbuilder as P
    from pyposegraphbuilder import _lib as L
    lib = L.load()
    for name in ("pgi_bundle_adjust", "pgi_tracklets_bundle_adjust", "pgi_default_bundle_params"):
        assert hasattr(lib, name) and name in L.SYMBOLS, name
    p = L.BundleParams()
    lib.pgi_default_bundle_params(C.byref(p))
    assert {k: getattr(p, k) for k, _ in L.BundleParams._fields_} == B.DEFAULTS
    z = None
    assert lib.pgi_bundle_adjust(z, z, z, 0, z, z, z, z, z, 0, z, z, z, z, z) < 0 and b"null context" in lib.pgi_last_error()
    assert lib.pgi_tracklets_bundle_adjust(z, z, z, z, z, z, 0, z, z, z, z, z) < 0 and b"null store" in lib.pgi_last_error()
    assert (P.BA_STOP_ITERS, P.BA_STOP_FTOL, P.BA_STOP_LAMBDA, P.BA_STOP_EMPTY) == (B.STOP_ITERS, B.STOP_FTOL, B.STOP_LAMBDA, B.STOP_EMPTY)
    assert P.BundleParams is L.BundleParams and P.BundleReport is L.BundleReport and P.BundleResult.FIELDS[:7] == REPORT


def test_spec_against_scipy():
    """The specification run to convergence and scipy.optimize.least_squares (trust region reflective, its own Jacobian by
    finite differences) on the same residual function from the same start reach the same cost; the refined centres are
    closer to the ground truth than the initialisation's, after a similarity alignment."""
    from scipy.optimize import least_squares
    p = B.make_problem(V=12, T=60, seed=1, noise_px=0.5, outlier_every=0)
    a = B.run(p, huber_px=np.inf, iters=50, ftol=1e-14)
    assert a["stop_reason"] == B.STOP_FTOL and a["n_obs"] == 360 and a["n_free_cams"] == 11
    ob = a["ob"]
    cams, pts = np.nonzero(ob["free"])[0], np.unique(ob["pt"])
    R0, c0, K = np.asarray(p["views"]["R"]).reshape(-1, 3, 3), np.asarray(p["views"]["c"]), p["views"]["K"]

    def residuals(x):
        R, c, X = R0.copy(), c0.copy(), p["X"].copy()
        d = x[:6 * len(cams)].reshape(-1, 6)
        R[cams] = B.rodrigues_update(R0[cams], d[:, :3])
        c[cams] = c0[cams] + d[:, 3:]
        X[pts] = p["X"][pts] + x[6 * len(cams):].reshape(-1, 3)
        return B.linearize(R, c, K, X, ob, np.inf)["r"].reshape(-1)

    s = least_squares(residuals, np.zeros(6 * len(cams) + 3 * len(pts)), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
    gap = abs(2.0 * s.cost - a["cost_final"]) / a["cost_final"]
    before, after = B.aligned_centre_error(c0, p["views_gt"]["c"]), B.aligned_centre_error(a["c"], p["views_gt"]["c"])
    print("cost %.15g, scipy %.15g, gap %.3g (bound %.3g); centre error %.3g -> %.3g" % (a["cost_final"], 2.0 * s.cost, gap, SCIPY_GAP_BOUND, before, after))
    assert gap <= SCIPY_GAP_BOUND
    assert after < before


def test_spec_noise_free():
    p = B.make_problem(V=12, T=60, seed=1, noise_px=0.0, outlier_every=0, pixel_dtype=np.float64)
    a = B.run(p, huber_px=np.inf, iters=50)
    rms0, rms = np.sqrt(a["cost_initial"] / a["n_obs"]), np.sqrt(a["cost_final"] / a["n_obs"])
    print("noise-free: rms %.3g px -> %.3g px (bound %.3g)" % (rms0, rms, NOISE_FREE_RMS_BOUND))
    assert rms0 > 0.1 and rms <= NOISE_FREE_RMS_BOUND


def test_spec_huber():
    """Planted 47 px observations that the triangulation did not trim: the Huber solution lies closer to the ground truth."""
    p = noisy(12, 60, 1, True)
    assert np.all(p["status"] == TS.OK) and np.all(p["obs_state"] == 1) and p["planted"].sum() == 12
    huber, plain = B.run(p), B.run(p, huber_px=np.inf)
    err = lambda r: (B.aligned_centre_error(np.asarray(r["c"]), p["views_gt"]["c"]), np.median(np.linalg.norm(r["X"] - p["X_gt"], axis=1)))
    print("huber: centres %.3g, points %.3g; plain: centres %.3g, points %.3g" % (err(huber) + err(plain)))
    assert err(huber)[0] < err(plain)[0] and err(huber)[1] < err(plain)[1]


def test_spec_trial_step_rejection_and_fatal_start():
    p = B.rejection_problem()
    trace = []
    r = B.run(p, iters=1, trace=trace)
    assert (r["iters"], r["accepted"]) == (1, 0) and trace[0]["cost_new"] == np.inf and not trace[0]["accepted"]
    assert np.array_equal(r["R"], p["views"]["R"]) and np.array_equal(r["c"], p["views"]["c"]) and np.array_equal(r["X"], p["X"])
    assert r["lambda_final"] == B.DEFAULTS["lambda_init"] * 10.0
    full = B.run(p)
    assert full["accepted"] > 0 and full["iters"] > full["accepted"] and full["cost_final"] < full["cost_initial"]
    with pytest.raises(ValueError):
        B.run(B.rejection_problem(-0.05))


def test_reference_conditions():
    """Conditions on the inputs, checked on the reference alone: the step references run all n iterations (so device and
    reference cannot agree by both stopping early; one free camera is solved exactly by its own block), and every gain ratio
    of the converged-regime runs stays GAIN_MARGIN away from the accept threshold."""
    for name in STEP_CASES:
        for n in B.STEP_COUNTS:
            ran = step_reference(name, n)["cg_iters_total"]
            assert ran == n or (STEP_CASES[name][0] == 2 and ran >= 1), (name, n, ran)
    for i in range(len(B.CONVERGED_SCENES)):
        ref, trace = converged_reference(i)
        assert len(trace) == 3 and all(abs(t["gain"] - B.ACCEPT_RATIO) >= B.GAIN_MARGIN for t in trace), [t["gain"] for t in trace]
    p, idx = lists()
    ob = lists_reference()["ob"]
    assert ob["cam_count"][idx["one_pass"]] == 64 and ob["cam_count"].max() > 64 and ob["cam_count"][idx["held"]] == B.DEFAULTS["min_cam_obs"] - 1
    assert not ob["free"][idx["held"]] and ob["free"][idx["one_pass"]] and ob["cam_count"][100:].sum() == 0
    lengths = np.diff(p["track_begin"].astype(np.int64))
    assert lengths.min() == 2 and lengths.max() == 70 and len(p["views"]["xy"]) == 306


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


def upload(eng, views):
    return [eng.upload_keypoints(np.asarray(views["xy"][i], np.float32).reshape(-1, 2), views["K"][i][0], 2.0 * views["K"][i][2],
                                 2.0 * views["K"][i][3]) for i in range(len(views["xy"]))]


def device_run(eng, p, kps=None, force=False, **kw):
    v = p["views"]
    if force:
        os.environ["PGI_BUNDLE_FORCE_ACCEPT"] = "1"
    try:
        r = eng.bundle_adjust(p["track_begin"], p["members"], kps or upload(eng, v), v["R"], v["c"], p["X"], p["status"], p["obs_state"],
                              has_pose=v.get("has_pose"), **kw)
    finally:
        os.environ.pop("PGI_BUNDLE_FORCE_ACCEPT", None)
    return r


def as_state(r):
    return dict(R=r.R, c=r.c, X=r.X.cpu().numpy())


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_hip_fixed_step_parity(eng, name):
    """iters = 1, cg_iters = n, acceptance forced: the state after the n-th PCG iterate of the first damped system."""
    p = step_problem(name)
    kps = upload(eng, p["views"])
    for n in B.STEP_COUNTS:
        ref = step_reference(name, n)
        got = device_run(eng, p, kps, force=True, cg_iters=n, **B.STEP_PARAMS)
        d = B.state_distance(as_state(got), ref, start_of(p))
        print("%s n = %d: %.3g (bound %.3g), %d PCG iterations" % (name, n, d, STEP_BOUND, got.cg_iters_total))
        assert (got.iters, got.accepted) == (1, 1)
        # one free camera: its own block is the whole system, the first iterate solves it and what follows is round-off
        assert got.cg_iters_total == ref["cg_iters_total"] == n or (STEP_CASES[name][0] == 2 and got.cg_iters_total >= 1)
        assert (got.n_obs, got.n_points, got.n_free_cams) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"])
        assert d <= STEP_BOUND


@pytest.mark.gpu
def test_hip_list_shapes(eng):
    p, idx = lists()
    ref = lists_reference()
    kps = upload(eng, p["views"])
    kw = dict(B.STEP_PARAMS, min_cam_obs=B.DEFAULTS["min_cam_obs"], cg_iters=7)
    got = device_run(eng, p, kps, force=True, **kw)
    d = B.state_distance(as_state(got), ref, start_of(p))
    print("list shapes: %.3g (bound %.3g)" % (d, STEP_BOUND))
    assert (got.n_obs, got.n_points, got.n_free_cams, got.cg_iters_total) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"], 7)
    assert d <= STEP_BOUND
    R0, c0 = np.asarray(p["views"]["R"]).reshape(-1, 3, 3), np.asarray(p["views"]["c"])
    held = ~ref["ob"]["free"]
    assert held[idx["held"]] and held[0] and held[100:].all()
    assert same_bits(got.R[held], R0[held]) and same_bits(got.c[held], c0[held])
    assert not same_bits(got.R[idx["one_pass"]], R0[idx["one_pass"]])
    X = got.X.cpu().numpy()
    for t in (idx["reproj"], idx["single"]):
        assert same_bits(X[t], p["X"][t]), t
    assert not same_bits(X[idx["dropped"]], p["X"][idx["dropped"]])
    # members that do not take part contribute nothing: move their pixels, compare bits
    moved = dict(p["views"], xy=[np.array(a, np.float32) for a in p["views"]["xy"]])
    out = np.nonzero(p["obs_state"] != 1)[0]
    assert (p["obs_state"][out] == 2).sum() == 2
    for m in out:
        v, kp = int(p["members"][m] >> np.uint64(32)), int(p["members"][m] & np.uint64(0xFFFFFFFF))
        moved["xy"][v][kp] += 25.0
    again = device_run(eng, dict(p, views=moved), None, force=True, **kw)
    assert same_bits(again.R, got.R) and same_bits(again.c, got.c) and same_bits(again.X.cpu().numpy(), X)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(B.CONVERGED_SCENES)))
def test_hip_converged_regime(eng, i):
    V, T, seed = B.CONVERGED_SCENES[i]
    p = noisy(V, T, seed)
    ref, _ = converged_reference(i)
    got = device_run(eng, p, **B.CONVERGED_PARAMS)
    d = B.state_distance(as_state(got), ref, start_of(p))
    print("converged V = %d: %.3g (bound %.3g), %d PCG iterations" % (V, d, CONVERGED_BOUND, got.cg_iters_total))
    assert (got.iters, got.accepted) == (ref["iters"], ref["accepted"]) == (3, 3)
    assert d <= CONVERGED_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(B.DEFAULT_SCENES)))
def test_hip_end_to_end_defaults(eng, i):
    V, T, seed = B.DEFAULT_SCENES[i]
    p = noisy(V, T, seed, True)
    ref = default_reference(i)
    kps = upload(eng, p["views"])
    got, again = device_run(eng, p, kps), device_run(eng, p, kps)
    gap = abs(got.cost_final - ref["cost_final"]) / ref["cost_final"]
    print("defaults V = %d: cost %.15g against %.15g, gap %.3g (bound %.3g); %s" % (V, got.cost_final, ref["cost_final"], gap, DEFAULT_COST_BOUND, got.report()))
    assert (got.n_obs, got.n_points, got.n_free_cams) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"])
    assert got.cost_initial >= got.cost_final and got.accepted > 0
    assert gap <= DEFAULT_COST_BOUND
    assert same_bits(got.R, again.R) and same_bits(got.c, again.c) and same_bits(got.X.cpu().numpy(), again.X.cpu().numpy())
    assert got.report() == again.report()


@pytest.mark.gpu
def test_hip_parameters_and_masks(eng):
    from pyposegraphbuilder._lib import PgiError
    p = noisy(12, 60, 1, True)
    v = p["views"]
    kps = upload(eng, v)
    R0, c0 = np.asarray(v["R"]).reshape(-1, 3, 3), np.asarray(v["c"])
    call = lambda **kw: eng.bundle_adjust(p["track_begin"], p["members"], kps, v["R"], v["c"], p["X"], p["status"], p["obs_state"], **kw)
    # fixed views come back bit-identical, the others move
    fixed = np.zeros(12, bool)
    fixed[[2, 7]] = True
    r = call(fixed=fixed)
    ref = B.run(p, fixed=fixed)
    assert same_bits(r.R[fixed], R0[fixed]) and same_bits(r.c[fixed], c0[fixed]) and r.n_free_cams == ref["n_free_cams"] == 10
    assert not same_bits(r.c[0], c0[0])
    assert abs(r.cost_final - ref["cost_final"]) / ref["cost_final"] <= DEFAULT_COST_BOUND
    # use_low_parallax adds exactly the LOW_PARALLAX tracks
    status = p["status"].copy()
    status[[4, 9, 30]] = TS.LOW_PARALLAX
    low = dict(p, status=status)
    a, b = device_run(eng, low, kps), device_run(eng, low, kps, use_low_parallax=1)
    assert (a.n_points, b.n_points) == (57, 60) and b.n_points - a.n_points == (status == TS.LOW_PARALLAX).sum()
    assert same_bits(a.X.cpu().numpy()[[4, 9, 30]], p["X"][[4, 9, 30]])
    # iters = 0 returns the input
    z = call(iters=0)
    assert same_bits(z.R, R0) and same_bits(z.c, c0) and same_bits(z.X.cpu().numpy(), p["X"]) and (z.iters, z.accepted) == (0, 0)
    assert z.cost_initial == z.cost_final > 0
    # huber_px = inf equals the plain run of the specification
    plain, want = call(huber_px=np.inf), B.run(p, huber_px=np.inf)
    assert abs(plain.cost_final - want["cost_final"]) / want["cost_final"] <= DEFAULT_COST_BOUND
    assert plain.cost_final > 2.0 * r.cost_final
    # an empty participation set succeeds and changes nothing
    e = device_run(eng, dict(p, status=np.full(60, TS.REPROJ, np.uint8)), kps)
    assert e.stop_reason == B.STOP_EMPTY and e.n_obs == 0 and same_bits(e.R, R0) and same_bits(e.X.cpu().numpy(), p["X"])
    # unknown keyword, bad parameters, bad poses
    with pytest.raises(TypeError):
        call(no_such_parameter=1)
    for kw in (dict(huber_px=0.0), dict(cg_tol=0.0), dict(lambda_init=-1.0)):
        with pytest.raises(PgiError):
            call(**kw)
    Rbad = R0.copy()
    Rbad[3, 1, 1] = np.nan
    with pytest.raises(PgiError):
        eng.bundle_adjust(p["track_begin"], p["members"], kps, Rbad, v["c"], p["X"], p["status"], p["obs_state"])
    zero_f = [dict(k) for k in kps]
    zero_f[2]["fx"] = 0.0
    with pytest.raises(PgiError):
        eng.bundle_adjust(p["track_begin"], p["members"], zero_f, v["R"], v["c"], p["X"], p["status"], p["obs_state"])


@pytest.mark.gpu
def test_hip_trial_step_rejection_and_fatal_start(eng):
    from pyposegraphbuilder._lib import PgiError
    p = B.rejection_problem()
    kps = upload(eng, p["views"])
    r = device_run(eng, p, kps, iters=1)
    assert (r.iters, r.accepted, r.lambda_final) == (1, 0, B.DEFAULTS["lambda_init"] * 10.0)
    assert same_bits(r.R, np.asarray(p["views"]["R"]).reshape(-1, 3, 3)) and same_bits(r.c, p["views"]["c"]) and same_bits(r.X.cpu().numpy(), p["X"])
    full, ref = device_run(eng, p, kps), B.run(p)
    assert (full.iters, full.accepted, full.stop_reason) == (ref["iters"], ref["accepted"], ref["stop_reason"])
    with pytest.raises(PgiError, match="non-positive depth"):
        device_run(eng, B.rejection_problem(-0.05), kps)


@pytest.mark.gpu
def test_hip_store_path(eng):
    """DeviceTracklets.bundle_adjust after DeviceTracklets.triangulate gives the bits of the array call on the same tracks."""
    from pyposegraphbuilder.engine import DeviceTracklets
    p = noisy(12, 60, 1)
    v = p["views"]
    kps = upload(eng, v)
    tb = p["track_begin"]
    calls = {}
    for t in range(len(tb) - 1):   # a track's consecutive members as matches (first view, next view)
        m = p["members"][tb[t]:tb[t + 1]]
        for a, b in zip(m[:-1], m[1:]):
            va, vb = int(a >> np.uint64(32)), int(b >> np.uint64(32))
            calls.setdefault((va, vb), []).append((int(a & np.uint64(0xFFFFFFFF)), int(b & np.uint64(0xFFFFFFFF))))
    store = DeviceTracklets(eng, 12)
    store.add_batch([(s, d, np.array(m), None) for (s, d), m in sorted(calls.items())])
    n = store.info()["tracks"]
    tri = store.triangulate(kps, v["R"], v["c"], thr_px=8.0)
    got = store.bundle_adjust(kps, v["R"], v["c"], tri.X, tri.status, tri.obs_state)
    tracks = [store.track(i) for i in range(n)]
    tb2 = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32)
    mem2 = np.array([TS.pack(a, b) for t in tracks for a, b in t], np.uint64)
    direct = eng.bundle_adjust(tb2, mem2, kps, v["R"], v["c"], tri.X, tri.status, tri.obs_state)
    assert got.n_points >= 55 and got.accepted > 0 and got.report() == direct.report()
    assert same_bits(got.R, direct.R) and same_bits(got.c, direct.c) and same_bits(got.X.cpu().numpy(), direct.X.cpu().numpy())
    assert not same_bits(got.X.cpu().numpy(), tri.X.cpu().numpy())
    store.close()
