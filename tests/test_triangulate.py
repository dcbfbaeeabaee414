"""Track triangulation (include/pgi.h: pgi_triangulate_tracks, pgi_tracklets_triangulate) against its CPU specification
tests/triangulate_spec.py: N-view midpoint, Gauss-Newton on the reprojection error, greedy trimming, parallax test."""
import ctypes as C
import functools

import numpy as np
import pytest

import triangulate_spec as TS

# The scene (TS.make_scene): 12 views, depth 6..12, f = 1000, 0.5 px noise, one observation displaced by 47 px in every
# fifth track.  Greedy drop-the-worst is not infallible on FOUR-view tracks (an outlier along the epipolar direction can
# leave a clean observation with the largest residual: about 1 % of such tracks over seeds 1..12), so the seeds are fixed
# to scenes on which the specification alone removes exactly the planted observations.
NOISY_60, NOISY_240 = dict(V=12, T=60, seed=1), dict(V=12, T=240, seed=8)

# Worst |X - X_gt| / scene size (12, the far depth) of the specification on the noise-free scene below (f64 pixels, so
# that the figure is the algorithm's and not the rounding of the pixels to f32), measured on the CPU: 4.54e-16.
# The bound is 100 times that; the margin is for the conditioning of low-parallax tracks under another seed, not for the
# device, which is compared by bits.
NOISE_FREE_MEASURED = 4.54e-16
NOISE_FREE_BOUND = 100.0 * NOISE_FREE_MEASURED
# Median |X - X_gt| / scene size of the specification on the two noisy scenes, measured on the CPU: 4.45e-4 (T = 60) and
# 5.66e-4 (T = 240); the bound follows the same rule from the larger one.
NOISY_MEDIAN_MEASURED = 5.66e-4
NOISY_MEDIAN_BOUND = 100.0 * NOISY_MEDIAN_MEASURED


def freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def noisy(T):
    return TS.make_scene(**(NOISY_60 if T == 60 else NOISY_240))


@functools.lru_cache(maxsize=None)
def problem(V):
    """The GPU problem over V scene views (+ 6 appended): the constructed tracks, then noise-and-outlier tracks of 4..8
    views and, for V = 300, of up to 70 views; 300 tracks in all.  V = 12 -> 18 views (view table staged in LDS),
    V = 300 -> 306 views (read through L2: the kernel stages at most 256)."""
    sc = TS.make_scene(V=V, T=240, seed=8 if V == 12 else 5)
    con = TS.constructed_tracks(sc)
    both = TS.concatenate(con, sc, con["views"])
    long_ = TS.make_scene(V=V, T=300 - 240 - len(con["expect"]), seed=11, min_len=2, max_len=min(V, 70), cameras=con["views"])
    p = TS.concatenate(both, long_, long_["views"])
    assert len(p["track_begin"]) - 1 == 300
    lengths = np.diff(p["track_begin"].astype(np.int64))
    assert lengths.min() == 0 and lengths.max() == 70
    return freeze(p)


def prefix(p, T):
    tb = p["track_begin"][:T + 1]
    return tb, p["members"][:tb[-1]]


@functools.lru_cache(maxsize=None)
def spec_result(V, T):
    tb, mem = prefix(problem(V), T)
    return freeze(TS.triangulate(tb, mem, problem(V)["views"]))


assert_same = TS.assert_same   # (shared with tests/test_chain.py)


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_exports_defaults_and_null_context():
    import pyposegraphbuilder as P
    from pyposegraphbuilder import _lib as L
    lib = L.load()
    for name in ("pgi_triangulate_tracks", "pgi_tracklets_triangulate", "pgi_default_triangulate_params"):
        assert hasattr(lib, name), name
    p = L.TriangulateParams()
    lib.pgi_default_triangulate_params(C.byref(p))
    assert (p.min_views, p.refine_iters, p.max_drops, p.thr_px, p.min_angle_deg) == (2, 3, 2, 2.0, 1.5)
    assert TS.DEFAULTS == dict(min_views=2, refine_iters=3, max_drops=2, thr_px=2.0, min_angle_deg=1.5)
    z = None
    assert lib.pgi_triangulate_tracks(z, z, z, 0, z, z, z, z, 0, z, z, z, z, z, z, z) < 0 and b"null context" in lib.pgi_last_error()
    assert lib.pgi_tracklets_triangulate(z, z, z, z, z, 0, z, z, z, z, z, z, z) < 0 and b"null store" in lib.pgi_last_error()
    assert (P.TRI_OK, P.TRI_TOO_FEW, P.TRI_DEGENERATE, P.TRI_BEHIND, P.TRI_REPROJ, P.TRI_LOW_PARALLAX) == \
        (TS.OK, TS.TOO_FEW, TS.DEGENERATE, TS.BEHIND, TS.REPROJ, TS.LOW_PARALLAX)
    assert P.TRI_STATUS_COUNT == TS.N_STATUS == len(P.TRI_STATUS_NAMES)


def test_spec_noise_free():
    sc = TS.make_scene(V=12, T=60, seed=1, noise_px=0.0, outlier_every=0, min_len=2, max_len=8, pixel_dtype=np.float64)
    r = TS.triangulate(sc["track_begin"], sc["members"], sc["views"])
    err = np.linalg.norm(r["X"] - sc["X_gt"], axis=1).max() / sc["size"]
    print("noise-free: worst |X - X_gt| / size = %.3g (bound %.3g)" % (err, NOISE_FREE_BOUND))
    assert np.all(r["status"] == TS.OK) and np.all(r["obs_state"] == 1)
    assert np.array_equal(r["n_used"], np.diff(sc["track_begin"]))
    assert r["counts"].tolist() == [60, 0, 0, 0, 0, 0]
    assert err <= NOISE_FREE_BOUND


@pytest.mark.parametrize("T", [60, 240])
def test_spec_noise_and_outliers(T):
    sc = noisy(T)
    assert np.diff(sc["track_begin"]).min() == 4 and np.diff(sc["track_begin"]).max() == 8
    assert sc["planted"].sum() == T // 5
    r = TS.triangulate(sc["track_begin"], sc["members"], sc["views"])
    assert np.array_equal(r["obs_state"] == 2, sc["planted"])     # every planted observation, and only it
    assert np.all(r["obs_state"][~sc["planted"]] == 1)            # every clean track keeps all of its observations
    assert np.all(r["status"] == TS.OK)
    med = np.median(np.linalg.norm(r["X"] - sc["X_gt"], axis=1)) / sc["size"]
    print("T = %d: median |X - X_gt| / size = %.3g (bound %.3g), worst rms %.3g px" % (T, med, NOISY_MEDIAN_BOUND, r["err_rms"].max()))
    assert med <= NOISY_MEDIAN_BOUND
    assert r["err_rms"].max() < 2.0


def test_spec_constructed_tracks():
    con = TS.constructed_tracks(noisy(60))
    r = TS.triangulate(con["track_begin"], con["members"], con["views"])
    tb = con["track_begin"]
    seen = set()
    for i, (name, status, states) in enumerate(con["expect"]):
        got = r["obs_state"][tb[i]:tb[i + 1]].tolist()
        assert r["status"][i] == status, name
        assert states is None or got == states, name
        assert r["n_used"][i] == got.count(1), name
        assert np.all(np.isfinite(r["X"][i])) == (status in (TS.OK, TS.LOW_PARALLAX)), name
        seen.add(status)
        if name == "max_drops + 1 outliers":
            assert got.count(2) == TS.DEFAULTS["max_drops"] and got.count(0) == 0
        if name == "behind":
            assert r["err_rms"][i] == np.inf
    assert seen == set(range(TS.N_STATUS))
    assert r["counts"].sum() == len(con["expect"]) and np.array_equal(r["counts"], np.bincount(r["status"], minlength=6))
    # min_views = 3 turns the two-view tracks into TOO_FEW and keeps trimming from going below three views
    r3 = TS.triangulate(con["track_begin"], con["members"], con["views"], min_views=3)
    two = np.nonzero(r["n_used"] == 2)[0]
    assert len(two) and np.all(r3["status"][two] == TS.TOO_FEW)


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


_kp_cache = {}


def keypoints(eng, V):
    if V not in _kp_cache:
        v = problem(V)["views"]
        _kp_cache[V] = [eng.upload_keypoints(v["xy"][i], v["K"][i][0], 2.0 * v["K"][i][2], 2.0 * v["K"][i][3]) for i in range(len(v["xy"]))]
    return _kp_cache[V]


def run(eng, V, T, **kw):
    p = problem(V)
    tb, mem = prefix(p, T)
    v = p["views"]
    return eng.triangulate_tracks(tb, mem, keypoints(eng, V), v["R"], v["c"], v["has_pose"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("V", [12, 300])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 300])
def test_hip_equals_spec(eng, V, T):
    """Bit for bit, NaNs in the same places: statuses, counts, states, points and errors."""
    got = run(eng, V, T).numpy()
    want = spec_result(V, T)
    assert_same(got, want, "V %d T %d" % (V, T))
    if T == 300:
        assert set(want["status"].tolist()) == set(range(TS.N_STATUS))


@pytest.mark.gpu
@pytest.mark.parametrize("V", [12, 300])
def test_hip_permutation_and_reproducibility(eng, V):
    """Permuting the tracks permutes every output bit for bit (the length order must not leak into the results), and two
    runs give the same bits."""
    p = problem(V)
    base = run(eng, V, 300).numpy()
    assert_same(run(eng, V, 300).numpy(), base, "second run")
    tb = p["track_begin"].astype(np.int64)
    perm = np.random.default_rng(4).permutation(300)
    runs = [p["members"][tb[t]:tb[t + 1]] for t in perm]
    tb2 = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.uint32)
    v = p["views"]
    got = eng.triangulate_tracks(tb2, np.concatenate(runs), keypoints(eng, V), v["R"], v["c"], v["has_pose"]).numpy()
    want = dict(X=base["X"][perm], err_rms=base["err_rms"][perm], status=base["status"][perm], n_used=base["n_used"][perm],
                counts=base["counts"], obs_state=np.concatenate([base["obs_state"][tb[t]:tb[t + 1]] for t in perm]))
    assert_same(got, want, "permuted")


@pytest.mark.gpu
def test_hip_store_path(eng):
    """DeviceTracklets.triangulate after add_batch of ground-truth matches == Engine.triangulate_tracks on the tracks read
    back through track() == the specification."""
    from pyposegraphbuilder.engine import DeviceTracklets
    sc = noisy(60)
    v = sc["views"]
    V = 12
    kps = [eng.upload_keypoints(v["xy"][i], 1000.0, 2000.0, 2000.0) for i in range(V)]
    tb = sc["track_begin"]
    calls = {}
    for t in range(len(tb) - 1):   # a track's consecutive members as matches (first view, next view)
        m = sc["members"][tb[t]:tb[t + 1]]
        for a, b in zip(m[:-1], m[1:]):
            va, vb = int(a >> np.uint64(32)), int(b >> np.uint64(32))
            calls.setdefault((va, vb), []).append((int(a & np.uint64(0xFFFFFFFF)), int(b & np.uint64(0xFFFFFFFF))))
    store = DeviceTracklets(eng, V)
    store.add_batch([(s, d, np.array(m), None) for (s, d), m in sorted(calls.items())])
    n = store.info()["tracks"]
    assert n >= 60
    got = store.triangulate(kps, v["R"], v["c"]).numpy()
    tracks = [store.track(i) for i in range(n)]
    tb2 = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32)
    mem2 = np.array([TS.pack(a, b) for t in tracks for a, b in t], np.uint64)
    assert len(mem2) == store.info()["events"]
    direct = eng.triangulate_tracks(tb2, mem2, kps, v["R"], v["c"]).numpy()
    assert_same(got, direct, "store vs direct")
    assert_same(direct, TS.triangulate(tb2, mem2, v), "direct vs spec")
    assert got["counts"][TS.OK] >= 55
    store.close()


@pytest.mark.gpu
def test_hip_optional_outputs_empty_input_and_errors(eng):
    from pyposegraphbuilder._lib import PgiError
    want = spec_result(12, 65)
    r = run(eng, 12, 65, err_rms=False, n_used=False, obs_state=False)
    assert r.err_rms is None and r.n_used is None and r.obs_state is None
    got = r.numpy()
    assert np.array_equal(got["X"], want["X"], equal_nan=True) and np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["counts"], want["counts"])
    # parameters reach the kernel
    p = problem(12)
    tb, mem = prefix(p, 65)
    kw = dict(min_views=3, refine_iters=1, max_drops=1, thr_px=1.0, min_angle_deg=3.0)
    assert_same(run(eng, 12, 65, **kw).numpy(), TS.triangulate(tb, mem, p["views"], **kw), "parameters")
    # zero tracks
    v = p["views"]
    kps = keypoints(eng, 12)
    e = eng.triangulate_tracks(np.zeros(1, np.uint32), np.zeros(0, np.uint64), kps, v["R"], v["c"], v["has_pose"])
    assert e.X.shape == (0, 3) and e.counts.sum() == 0
    # validation
    for kw in (dict(min_views=1), dict(thr_px=0.0), dict(thr_px=-1.0)):
        with pytest.raises(PgiError):
            run(eng, 12, 1, **kw)
    Rbad, cbad = np.array(v["R"]), np.array(v["c"])
    Rbad[3, 1, 1] = np.nan
    cbad[5, 0] = np.inf
    with pytest.raises(PgiError):
        eng.triangulate_tracks(tb, mem, kps, Rbad, v["c"], v["has_pose"])
    with pytest.raises(PgiError):
        eng.triangulate_tracks(tb, mem, kps, v["R"], cbad, v["has_pose"])
    zero_f = [dict(k) for k in kps]
    zero_f[2]["fx"] = 0.0
    with pytest.raises(PgiError):
        eng.triangulate_tracks(tb, mem, zero_f, v["R"], v["c"], v["has_pose"])
    # ... but not of a view without a pose
    nopose = len(kps) - 6
    assert not v["has_pose"][nopose]
    Rn = np.array(v["R"])
    Rn[nopose] = np.nan
    assert_same(eng.triangulate_tracks(tb, mem, kps, Rn, v["c"], v["has_pose"]).numpy(), want, "NaN pose of a view without a pose")
    assert_same(run(eng, 12, 65).numpy(), want, "the context still works")
