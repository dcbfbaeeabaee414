"""Translation averaging, step-exact: the PCG and model kernels of csrc/pgi_transavg.hip against the n-step reference
tests/transavg_pcg_ref.py (longdouble block-Jacobi PCG on the system tests/transavg_spec.py assembles).

With iters = 1 and cg_iters = n the device returns c0 + x_n, the n-th PCG iterate of the first step system, so the
comparison needs neither convergence nor the 4.77e-5 of tests/test_transavg.py.  The measure everywhere is
    max |c - c_ref| over the views / max |c_ref - c0|          (no alignment; transavg_pcg_ref.distance)

The bounds come from the reference alone (scripts/transavg_roundoff.py, CPU):
  * ROUNDOFF = 1.12e-11: the largest distance between the longdouble leg and a float64 leg that follows the kernel's
    formulas (adjugate inverse, per-view sums in edge order, and again with the edges permuted), over every graph and step
    count below.  First-step cases: 1.1e-13 .. 2.3e-12 (largest: the hub graphs); the 4 x 20 trajectory: 3.7e-13 at V = 50
    and 1.12e-11 at V = 321, where the adjugate inverse dominates (2.1e-12 with LAPACK inverses; it makes no difference
    on the first step).  Bound: ten times that, 1.12e-10.
  * CONVERGED = 5.16e-13: irls_fixed at PGI_TRANSAVG_CG_TOL = 1e-11, delta = 1 against the specification's direct solves
    after three outer iterations (V = 12 / 257 / 320: 2.2e-13 / 5.2e-13 / 3.6e-13).  Bound: ten times that, 5.16e-12.
Measured on the MI355X: fixed-step parity 1.1e-13 .. 2.08e-12, topologies 1.5e-13 .. 2.34e-12,
one workgroup against five 2.6e-15 .. 1.4e-14, trajectory 3.15e-13 / 1.18e-11, converged regime 2.21e-13 / 5.16e-13 / 3.59e-13.
"""
import functools

import numpy as np
import pytest

import transavg_pcg_ref as R
import transavg_spec as TS

ROUNDOFF = 1.12e-11
STEP_BOUND = 10.0 * ROUNDOFF
CONVERGED = 5.16e-13
CONVERGED_BOUND = 10.0 * CONVERGED

PARITY = R.parity_graphs()
TOPOLOGY = R.topology_graphs()
TRAJECTORY = R.trajectory_graphs()
CONVERGED_GRAPHS = R.converged_graphs()


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """One longdouble PCG run per graph: -> (c0, {n: (c_ref, iterations run)})."""
    if name in PARITY:
        c0, ref = R.first_step_reference(PARITY[name], R.STEP_COUNTS)
    else:
        c0, ref = R.first_step_reference(TOPOLOGY[name], (R.TOPOLOGY_STEPS,))
    return _freeze(c0), {n: (_freeze(c), ran) for n, (c, ran) in ref.items()}


@functools.lru_cache(maxsize=None)
def trajectory_reference(name):
    g = TRAJECTORY[name]
    trace = []
    c, iters = R.irls_fixed(g["V"], g["src"], g["dst"], g["gamma"], g["w"], trace=trace, **R.TRAJECTORY)
    return _freeze(c), iters, trace


@functools.lru_cache(maxsize=None)
def converged_reference(name):
    """-> (direct-solve specification, irls_fixed at the same tolerance, its iterations, its trace)."""
    g = CONVERGED_GRAPHS[name]
    c_dir, it_dir = TS.translation_average(g["V"], g["src"], g["dst"], g["gamma"], g["w"], iters=R.CONVERGED["iters"],
                                           delta=R.CONVERGED["delta"])
    trace = []
    c, it = R.irls_fixed(g["V"], g["src"], g["dst"], g["gamma"], g["w"], trace=trace, **R.CONVERGED)
    assert it == it_dir
    return _freeze(c_dir), _freeze(c), it, trace


def init_of(g):
    return TS.spanning_forest_init(g["V"], g["src"], g["dst"], g["gamma"], g["w"])


# ---- CPU: the conditions on the reference legs -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PARITY) + list(TOPOLOGY))
def test_reference_runs_every_step(name):
    """The reference must not converge before n, or device and reference could agree by both stopping early.  The single
    edge is the one exception a graph cannot avoid: its only free view makes the preconditioner the exact inverse, so the
    PCG ends after one step whatever n is (and the step itself is round-off: the initialisation is the solution)."""
    _, ref = step_reference(name)
    for n, (_, ran) in ref.items():
        assert ran == (1 if name == "V2" else n), (name, n, ran)


def test_reference_topologies_are_what_they_claim():
    for V in (200, 300):
        g = TOPOLOGY["components-V%d" % V]
        assert list(init_of(g)[1]) == [0, 100]
        assert np.array_equal(g["src"] < 100, g["dst"] < 100)
    for V in (200, 330):
        g, lone = R.with_isolated_views(V)
        assert list(init_of(g)[1]) == sorted([0] + list(lone)) and lone[-1] == V - 1
        assert not np.isin(np.r_[g["src"], g["dst"]], lone).any()
    for V in (30, 260):
        g = TOPOLOGY["doubled-V%d" % V]
        E = len(g["src"]) // 2
        assert np.array_equal(g["src"][:E], g["dst"][E:]) and np.array_equal(g["dst"][:E], g["src"][E:])
        assert np.array_equal(g["gamma"][:E], -g["gamma"][E:]) and np.all(g["w"][:E] != g["w"][E:])
    for V, hub, spokes in ((256, 100, 255), (330, 200, 300)):
        g = TOPOLOGY["hub-V%d" % V]
        assert np.bincount(np.r_[g["src"], g["dst"]], minlength=V)[hub] == spokes
        assert len(set(zip(np.minimum(g["src"], g["dst"]), np.maximum(g["src"], g["dst"])))) == len(g["src"])
    for V in (200, 300):
        g, e = R.zero_weight_chord(V)
        assert g["w"][e] == 0.0 and (g["w"] == 0.0).sum() == 1
        keep = np.arange(len(g["src"])) != e     # not a tree edge: the forest without it reaches the same views
        c0, roots = init_of(g)
        c1, roots1 = TS.spanning_forest_init(V, g["src"][keep], g["dst"][keep], g["gamma"][keep], g["w"][keep])
        assert np.array_equal(c0, c1) and np.array_equal(roots, roots1)


@pytest.mark.parametrize("name", list(TRAJECTORY))
def test_reference_trajectory_has_no_edge_on_the_class_boundary(name):
    """From the second outer iteration on no edge may sit within 1e-6 of a = 1: a class decided by the last bit would make
    the comparison meaningless.  (The first iteration's tree edges sit AT 1; specification and kernel fix that order.)"""
    _, iters, trace = trajectory_reference(name)
    assert iters == R.TRAJECTORY["iters"] and len(trace) == iters
    for t in trace[1:]:
        assert np.abs(t["a"] - 1.0).min() >= 1e-6
    assert all(t["cg"] == R.TRAJECTORY["cg_iters"] for t in trace)   # every solve ends at the cap


@pytest.mark.parametrize("name", list(CONVERGED_GRAPHS))
def test_reference_converges_under_the_cap(name):
    c_dir, c, it, trace = converged_reference(name)
    assert it == R.CONVERGED["iters"]
    assert all(0 < t["cg"] < R.CONVERGED["cg_iters"] for t in trace)
    d = R.distance(c, c_dir, init_of(CONVERGED_GRAPHS[name])[0])
    print("%s: irls_fixed against the direct solves %.3g (recorded largest %.3g)" % (name, d, CONVERGED))
    assert d <= CONVERGED_BOUND      # (the recorded figure is this distance; another LAPACK moves its last digits)


def test_pcg_steps_float64_and_longdouble_agree():
    """The two dtypes of the same recurrence: round-off apart, and both reach the direct solution."""
    g = PARITY["V12"]
    c0, roots = init_of(g)
    free = np.ones(g["V"], bool)
    free[roots] = False
    A, rhs, _, _ = R.step_system(g["V"], g["src"], g["dst"], g["gamma"], g["w"], c0, free, 1e-3, 1e-4)
    x_ld, n_ld = R.pcg_steps(A, rhs, 17)
    x_64, n_64 = R.pcg_steps(A, rhs.astype(np.float64), 17, dtype=np.float64)
    assert n_ld == n_64 == 17 and x_64.dtype == np.float64 and x_ld.dtype == np.longdouble
    assert np.abs(x_64 - x_ld).max() <= 1e-11 * np.abs(x_ld).max()
    x, n = R.pcg_steps(A, rhs, 500, tol=1e-13)
    assert n < 500
    xd = TS.direct_solve(A, rhs.astype(np.float64), None)
    assert np.abs(x - xd).max() <= 1e-8 * np.abs(xd).max()


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


def run(eng, g, **kw):
    return eng.translation_average(g["src"], g["dst"], g["gamma"], g["w"], g["V"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_hip_fixed_step_parity(eng, name):
    """3a: iters = 1, cg_iters = n returns c0 + x_n.  V <= 256: trn_solve_kernel; above: trn_cg_*; V = 4161: 66 workgroups,
    the strided loop of reduce_partials.  n = 16, 17, 33 straddle the host's looks at the state record."""
    g = PARITY[name]
    c0, ref = step_reference(name)
    worst = 0.0
    for n in R.STEP_COUNTS:
        c_ref, ran = ref[n]
        c, iters = run(eng, g, iters=1, cg_iters=n)
        d = R.distance(c, c_ref, c0)
        worst = max(worst, d)
        print("%s n = %d (reference ran %d): distance %.3g (bound %.3g)" % (name, n, ran, d, STEP_BOUND))
        assert iters == 1
        assert d <= STEP_BOUND, (name, n, d)
    print("%s: largest %.3g" % (name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TOPOLOGY))
def test_hip_topologies(eng, name):
    """3b: gauge and isolated views outside block 0, duplicate edges in both orientations, a view of degree 255 / 300, a
    zero-weight chord -- each on the one-workgroup path and on the multi-workgroup path, 17 steps."""
    g = TOPOLOGY[name]
    c0, ref = step_reference(name)
    c_ref, _ = ref[R.TOPOLOGY_STEPS]
    c, iters = run(eng, g, iters=1, cg_iters=R.TOPOLOGY_STEPS)
    d = R.distance(c, c_ref, c0)
    print("%s: distance %.3g (bound %.3g)" % (name, d, STEP_BOUND))
    assert iters == 1 and d <= STEP_BOUND
    roots = init_of(g)[1]
    assert np.array_equal(c[roots], np.zeros((len(roots), 3)))     # gauge and isolated views: exactly 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 17, 33])
def test_hip_one_workgroup_against_many(eng, n):
    """3c: the V = 256 graph, and the same with one isolated view appended (V = 257): trn_solve_kernel against trn_cg_*."""
    g = PARITY["V256"]
    c0, ref = step_reference("V256")
    c_ref, _ = ref[n]
    c_a, _ = run(eng, g, iters=1, cg_iters=n)
    c_b, _ = run(eng, dict(g, V=257), iters=1, cg_iters=n)
    d = R.distance(c_b[:256], c_a, c0)
    print("n = %d: one workgroup against five: %.3g; each against the reference: %.3g, %.3g (bound %.3g)" %
          (n, d, R.distance(c_a, c_ref, c0), R.distance(c_b[:256], c_ref, c0), STEP_BOUND))
    assert np.array_equal(c_b[256], np.zeros(3))
    assert d <= STEP_BOUND
    assert R.distance(c_b[:256], c_ref, c0) <= STEP_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRAJECTORY))
def test_hip_fixed_step_trajectory(eng, name):
    """3d: four outer iterations of twenty PCG steps against irls_fixed: trn_model_kernel and trn_step_kernel over several
    outer steps, every solve ending at the cap."""
    g = TRAJECTORY[name]
    c_ref, it_ref, _ = trajectory_reference(name)
    c, iters = run(eng, g, **R.TRAJECTORY)
    d = R.distance(c, c_ref, init_of(g)[0])
    print("%s: iters %d (reference %d), distance %.3g (bound %.3g)" % (name, iters, it_ref, d, STEP_BOUND))
    assert iters == it_ref
    assert d <= STEP_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONVERGED_GRAPHS))
def test_hip_converged_regime(eng, name, monkeypatch):
    """3e: every solve converges under the cap (the `done` path: the early return of the direction kernel, the copy of the
    state record, the host's break), against the specification's direct solves."""
    monkeypatch.setenv("PGI_TRANSAVG_CG_TOL", "%g" % R.CONVERGED["cg_tol"])
    g = CONVERGED_GRAPHS[name]
    c_dir, _, it_ref, _ = converged_reference(name)
    kw = {k: v for k, v in R.CONVERGED.items() if k != "cg_tol"}
    c, iters = run(eng, g, **kw)
    d = R.distance(c, c_dir, init_of(g)[0])
    print("%s: iters %d, distance to the direct solves %.3g (bound %.3g)" % (name, iters, d, CONVERGED_BOUND))
    assert iters == it_ref
    assert d <= CONVERGED_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["V12", "V320"])
def test_hip_outer_tolerance_stops_the_iteration(eng, name, monkeypatch):
    """3e: tol = 1e-3 ends the outer loop where it ends the reference's, before the iterations passed."""
    monkeypatch.setenv("PGI_TRANSAVG_CG_TOL", "%g" % R.CONVERGED["cg_tol"])
    g = CONVERGED_GRAPHS[name]
    kw = dict(R.CONVERGED, iters=40, tol=1e-3)
    trace = []
    c_ref, it_ref = R.irls_fixed(g["V"], g["src"], g["dst"], g["gamma"], g["w"], trace=trace, **kw)
    assert 1 < it_ref < 40
    assert trace[-2]["step"] > 1.5e-3 and trace[-1]["step"] < 1e-3 / 1.2   # the decision is not a matter of round-off
    del kw["cg_tol"]
    c, iters = run(eng, g, **kw)
    print("%s: iters %d (reference %d), distance %.3g" % (name, iters, it_ref, R.distance(c, c_ref, init_of(g)[0])))
    assert iters == it_ref and iters < 40


@pytest.mark.gpu
def test_hip_parameters(eng):
    """3f: iters = 0, cg_iters = 0, and the values the library refuses."""
    from pyposegraphbuilder._lib import PgiError
    for name in ("V12", "V257"):
        g = PARITY[name]
        c0, ref = step_reference(name)
        c, iters = run(eng, g, iters=0)
        assert iters == 0 and np.array_equal(c, c0)          # the spanning-forest initialisation, bit for bit
        c_0, it_0 = run(eng, g, iters=1, cg_iters=0)         # clamped to one PCG step (include/pgi.h)
        c_1, it_1 = run(eng, g, iters=1, cg_iters=1)
        assert it_0 == it_1 == 1 and np.array_equal(c_0, c_1) and not np.array_equal(c_0, c0)
        assert R.distance(c_0, ref[1][0], c0) <= STEP_BOUND
    g = PARITY["V12"]
    want, _ = run(eng, g, iters=2)
    for bad in (dict(eps=0.0), dict(eps=2.0), dict(delta=0.0), dict(tol=-1.0)):
        with pytest.raises(PgiError):
            run(eng, g, iters=2, **bad)
        again, _ = run(eng, g, iters=2)                      # the context works afterwards
        assert np.array_equal(again, want)
