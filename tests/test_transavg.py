"""Translation averaging (include/pgi.h: pgi_translation_average[_edges]) against its CPU specification
tests/transavg_spec.py: robust Least Unsquared Deviations by joint IRLS with an active set."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import transavg_spec as TS

# (V, k, direction noise in degrees, outlier fraction, components).  The first is the smallest graph on which both edge
# classes occur at a fixed point; the last is the only one above the one-workgroup threshold of the device solver.
CASES = [(12, 3, 0.5, 0.1, 1), (40, 5, 0.0, 0.0, 1), (50, 6, 1.0, 0.15, 1), (30, 4, 0.5, 0.1, 3), (340, 20, 1.0, 0.2, 1)]

# The active-set switch makes the outer iteration discontinuous, so the distance between the device (inexact inner solves)
# and the specification (direct solves) is not round-off.  It was measured on the specification alone
# (scripts/transavg_sensitivity.py): the `solve=` hook set to scipy CG on the step system, stopped at the device's inner
# tolerance (relative residual 1e-4), moves the positions after 60 iterations by at most
#     1.56e-6, 3.5e-8, 2.0e-7, 4.77e-6, 5.1e-8   of their RMS spread on the five graphs above
# (at 1e-10: 2e-13 .. 2e-12, i.e. round-off).  The bound is ten times the largest figure; the margin covers the other
# preconditioner and ocml against libm.
SENSITIVITY_AT_1E_4 = 4.77e-6
HIP_VS_SPEC_BOUND = 10.0 * SENSITIVITY_AT_1E_4


@functools.lru_cache(maxsize=None)
def graph(case):
    V, k, noise, outl, comps = case
    src, dst, gamma, w, c_gt, out = TS.make_graph(V, k, noise, outl, seed=V, components=comps)
    return dict(V=V, src=src, dst=dst, gamma=gamma, w=w, c_gt=c_gt, labels=np.arange(V) % comps)


@functools.lru_cache(maxsize=None)
def spec_result(case):
    g = graph(case)
    trace = []
    c, iters = TS.translation_average(g["V"], g["src"], g["dst"], g["gamma"], g["w"], trace=trace)
    c.setflags(write=False)
    return c, iters, trace


def rms_spread(c):
    return float(np.sqrt(((c - c.mean(0)) ** 2).sum(1).mean()))


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_spec_noise_free_recovers_positions():
    case = CASES[1]
    c, iters, _ = spec_result(case)
    g = graph(case)
    err = TS.align_error(c, g["c_gt"])
    print("noise-free: iters %d, median %.3g, max %.3g" % (iters, np.median(err), err.max()))
    assert iters == 60          # the L1 weights sit at delta: a slow tail, not a defect
    assert np.median(err) < 1e-3


def test_spec_noise_and_outliers():
    case = CASES[2]
    c, _, trace = spec_result(case)
    g = graph(case)
    c0, _ = TS.spanning_forest_init(g["V"], g["src"], g["dst"], g["gamma"], g["w"])
    err, err0 = TS.align_error(c, g["c_gt"]), TS.align_error(c0, g["c_gt"])
    print("V = 50: median %.3g (init %.3g), max %.3g, clamped %d -> %d" % (np.median(err), np.median(err0), err.max(),
                                                                        trace[0][0], trace[-1][0]))
    assert np.median(err) < 0.08
    assert np.median(err) < 0.2 * np.median(err0)


def test_spec_three_components():
    case = CASES[3]
    c, _, _ = spec_result(case)
    g = graph(case)
    assert np.array_equal(c[:3], np.zeros((3, 3)))       # views 0, 1, 2: the smallest view of each component
    assert np.all(np.linalg.norm(c[3:], axis=1) > 0)
    err = TS.align_error(c, g["c_gt"], g["labels"])      # each component has its own scale and origin
    for lab in range(3):
        assert np.median(err[g["labels"] == lab]) < 0.08
    assert np.median(TS.align_error(c, g["c_gt"])) > 0.1  # one alignment for all three does not fit


def test_spec_both_edge_classes_on_the_smallest_graph():
    _, _, trace = spec_result(CASES[0])
    n_edges = len(graph(CASES[0])["src"])
    assert 0 < trace[-1][0] < n_edges


def _ground_truth_edges(V, k, seed):
    """Relative poses from ground truth: x_j = R_ij x_i + t_ij with R_ij = R_j R_i^T, t_ij = R_j (c_i - c_j), unit."""
    from scipy.spatial.transform import Rotation
    src, dst, _, _, c_gt, _ = TS.make_graph(V, k, 0.0, 0.0, seed=seed)
    R = Rotation.random(V, random_state=seed).as_matrix()
    t = np.einsum("eij,ej->ei", R[dst], c_gt[src] - c_gt[dst])
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    Rrel = np.einsum("eij,ekj->eik", R[dst], R[src])
    return src, dst, R, Rrel, t, c_gt


def test_directions_from_edges():
    src, dst, R, _, t, c_gt = _ground_truth_edges(40, 5, 3)
    want = c_gt[src] - c_gt[dst]
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    got = TS.directions_from_edges(R, src, dst, t)
    assert np.abs(got - want).max() < 1e-12
    # the package's helper for edge records computes the same bits
    from pyposegraphbuilder import _lib as L, distributed as D
    rec = np.zeros(len(src), L.EDGE_DTYPE)
    rec["t"], rec["status"] = t, 1
    rec["status"][5] = 0
    s, d, gam, w = D.edges_to_translation_graph(rec, src, dst, R)
    ok = rec["status"] == 1
    assert np.array_equal(s, src[ok]) and np.array_equal(d, dst[ok]) and np.array_equal(gam, got[ok]) and np.all(w == 1.0)


def test_library_exports_translation_averaging():
    """Fails before this solver existed: the three entry points of include/pgi.h are exported, and the defaults are the
    documented ones."""
    from pyposegraphbuilder import _lib as L
    lib = L.load()
    for name in ("pgi_translation_average", "pgi_translation_average_edges", "pgi_default_transavg_params"):
        assert hasattr(lib, name), name
    p = L.TransAvgParams()
    lib.pgi_default_transavg_params(C.byref(p))
    assert (p.iters, p.cg_iters, p.eps, p.delta, p.tol) == (60, 200, 1e-3, 1e-4, 1e-9)
    z = C.c_void_p(0)
    assert lib.pgi_translation_average(z, z, 0, 1, None, z, z) < 0 and lib.pgi_last_error()
    assert lib.pgi_translation_average_edges(z, z, z, z, z, 0, 1, z, None, z, z, z) < 0 and lib.pgi_last_error()


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


_hip_cache = {}


def hip_result(eng, case):
    """One device run per graph, shared by the tests below."""
    if case not in _hip_cache:
        g = graph(case)
        _hip_cache[case] = eng.translation_average(g["src"], g["dst"], g["gamma"], g["w"], g["V"])
    return _hip_cache[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "V%d" % c[0])
def test_hip_matches_spec(eng, case):
    """Positions without any alignment (the gauge is identical by construction): within HIP_VS_SPEC_BOUND = 4.77e-5 of the
    RMS spread (ten times the measured sensitivity 4.77e-6 of the iteration to inner solves stopped at 1e-4, see above)."""
    g = graph(case)
    c_spec, it_spec, _ = spec_result(case)
    c, iters = hip_result(eng, case)
    diff = float(np.linalg.norm(c - c_spec, axis=1).max()) / rms_spread(c_spec)
    err = TS.align_error(c, g["c_gt"], g["labels"])
    print("V = %d: iters %d (spec %d), max |c - c_spec| / rms = %.3g (bound %.3g), median error %.3g" %
          (g["V"], iters, it_spec, diff, HIP_VS_SPEC_BOUND, np.median(err)))
    assert abs(iters - it_spec) <= 1
    assert diff <= HIP_VS_SPEC_BOUND
    if case == CASES[1]:
        assert np.median(err) < 1e-3
    if case == CASES[2]:
        c0, _ = TS.spanning_forest_init(g["V"], g["src"], g["dst"], g["gamma"], g["w"])
        assert np.median(err) < 0.08
        assert np.median(err) < 0.2 * np.median(TS.align_error(c0, g["c_gt"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=lambda c: "V%d" % c[0])
def test_hip_is_reproducible(eng, case):
    g = graph(case)
    c, iters = hip_result(eng, case)
    c2, iters2 = eng.translation_average(g["src"], g["dst"], g["gamma"], g["w"], g["V"])
    assert iters == iters2 and np.array_equal(c, c2)


@pytest.mark.gpu
def test_hip_roots_and_empty_input(eng):
    c, _ = hip_result(eng, CASES[3])
    assert np.array_equal(c[:3], np.zeros((3, 3))) and np.all(np.linalg.norm(c[3:], axis=1) > 0)
    c1, _ = hip_result(eng, CASES[0])
    assert np.array_equal(c1[0], np.zeros(3))
    c, iters = eng.translation_average(np.zeros(0, int), np.zeros(0, int), np.zeros((0, 3)), np.zeros(0), 4)
    assert iters == 0 and np.array_equal(c, np.zeros((4, 3)))
    # a view without an edge stays at 0 next to a solved component
    g = graph(CASES[0])
    c, _ = eng.translation_average(g["src"], g["dst"], g["gamma"], g["w"], g["V"] + 2)
    assert np.array_equal(c[g["V"]:], np.zeros((2, 3))) and np.array_equal(c[:g["V"]], c1)
    # directions of any length are normalised: the same problem, so the same accuracy limit as the unit directions (not the
    # same bits -- the last bit of a direction decides the class of the initialisation's tree edges, see transavg_spec.py)
    g = graph(CASES[1])
    c3, _ = eng.translation_average(g["src"], g["dst"], 3.0 * g["gamma"], g["w"], g["V"])
    assert np.median(TS.align_error(c3, g["c_gt"])) < 1e-3


@pytest.mark.gpu
def test_hip_errors(eng):
    from pyposegraphbuilder._lib import PgiError
    with pytest.raises(PgiError):
        eng.translation_average([0], [7], [[1.0, 0.0, 0.0]], [1.0], 3)
    with pytest.raises(PgiError):
        eng.translation_average([0], [1], [[0.0, 0.0, 0.0]], [1.0], 3)
    with pytest.raises(PgiError):
        eng.translation_average([0], [1], [[np.nan, 0.0, 0.0]], [1.0], 3)
    with pytest.raises(PgiError):
        eng.translation_average([1], [1], [[1.0, 0.0, 0.0]], [1.0], 3)
    c, _ = eng.translation_average([0], [1], [[1.0, 0.0, 0.0]], [1.0], 3)   # the context still works: c_0 - c_1 = dir
    assert np.abs(c - np.array([[0, 0, 0], [-1.0, 0, 0], [0, 0, 0]])).max() < 1e-6


@pytest.mark.gpu
def test_hip_from_the_device_edge_table(eng):
    """pgi_translation_average_edges on an uploaded pgi_edge table + ground-truth global rotations == the host-edge entry
    point on directions_from_edges, bit for bit; a record that is not PGI_EDGE_OK is skipped and reported."""
    import torch
    from pyposegraphbuilder import _lib as L
    V = 40
    src, dst, R, Rrel, t, c_gt = _ground_truth_edges(V, 5, 3)
    P = len(src)
    rng = np.random.default_rng(9)
    rows = rng.integers(100, 400, P).astype(np.uint32)
    rec = np.zeros(P, L.EDGE_DTYPE)
    rec["R"], rec["t"], rec["status"] = Rrel.reshape(P, 9), t, 1
    rec["n_inl"] = (rows * rng.uniform(0.3, 1.0, P)).astype(np.uint32)
    rec["status"][7] = 0
    rec["t"][7] = 0.0        # never read
    table = torch.from_numpy(rec.view(np.uint8).reshape(P, 200).copy()).to(eng.device)
    c, iters, used = eng.translation_average_edges(table, src, dst, rows, V, R)
    ok = rec["status"] == 1
    assert used == P - 1
    w = rec["n_inl"][ok].astype(np.float64) / rows[ok].astype(np.float64)
    gam = TS.directions_from_edges(R, src[ok], dst[ok], t[ok])
    c2, iters2 = eng.translation_average(src[ok], dst[ok], gam, w, V)
    assert iters == iters2 and np.array_equal(c, c2)
    assert np.median(TS.align_error(c, c_gt)) < 1e-3
    # uniform weights without the row counts; an endpoint out of range is refused
    c3, _, used3 = eng.translation_average_edges(table, src, dst, None, V, R)
    c4, _ = eng.translation_average(src[ok], dst[ok], gam, np.ones(P - 1), V)
    assert used3 == P - 1 and np.array_equal(c3, c4)
    bad = dst.copy()
    bad[0] = V
    with pytest.raises(L.PgiError):
        eng.translation_average_edges(table, src, bad, rows, V, R)
