"""Rotation averaging, step-exact: the residual, update and PCG kernels of csrc/pgi_rotavg.hip against the n-step reference
tests/rotavg_pcg_ref.py (numpy longdouble: forest initialisation, quaternion log, textbook PCG with the Jacobi, tree and
two-level preconditioners).

With l1_iters + irls_iters = 1, cg_iters = n and PGI_ROTAVG_CG_TOL = 1e-14 the engine returns R0 exp(x_n), x_n the n-th
PCG iterate of the first system, on each of the four solver paths (one workgroup, many workgroups, tree with
PGI_ROTAVG_TREE_CG_ITERS = n, two-level with PGI_ROTAVG_TWO_LEVEL = 2).  The measure everywhere is
    max_k |R_k - R_ref,k|_max / max_k |x_n,k|            (relative to the step, no alignment; rotavg_pcg_ref.distance)

The bounds come from the reference alone (scripts/rotavg_roundoff.py, CPU): per case family -- and per step count on the
fixed-step paths, per path for the trajectory -- the largest distance between the longdouble leg and a float64 leg that
follows the kernels' formulas; the test bound is ten times that.  ROUNDOFF below is that script's output.  Measured on the
MI355X (largest per family):
  init 4.13e-16 (absolute) | planted 7.78e-11 | planted-tiny 1.93e-07 (a step of 5e-10 rad against float64's 1e-16 in R)
  one    n = 1 / 2 / 5 / 12: 2.70e-13 / 2.43e-13 / 2.43e-13 / 2.43e-13      many: 3.06e-13 / 2.43e-13 / 2.43e-13 / 2.43e-13
  two    1.15e-12 / 7.26e-13 / 2.55e-13 / 1.60e-13                          tree: 7.23e-12 / 4.55e-12 / 1.41e-11 / 1.78e-02
  one workgroup against many 2.80e-14 | converged 6.40e-12 | trajectory one / many / tree / two 1.83e-14 / 1.50e-14 / 6.69e-03 / 1.22e-14
The device sits where the float64 leg sits, also at tree n = 12: there float64 PCG itself leaves the longdouble iterates
(plain float64 recurrences with exact leaf-to-root tree solves: 1e-12 at n = 5, 2e-8 at 8, 6e-5 at 10, 1e-3 at 12 on path200,
back to 3e-8 at 14) -- the tree-preconditioned spectra have many isolated eigenvalues and the Lanczos process behind CG
loses its orthogonality in float64 a few steps earlier than in longdouble.  So on the tree path the tight nets are n <= 5
(1e-10) and the converged step (6.5e-11); n = 12 and the tree trajectory only catch gross errors.

Exceptions to "the reference runs all n steps" (asserted with their actual counts): a single free view (V = 2: Jacobi is
the exact inverse, one step), two free views (V = 3: two steps), and the ring of 65 views on the tree path (one edge
outside the forest, and the right-hand side lives on its two ends: one step).  At 180 deg - 0.06 deg the trace is -1 + 1e-6: the trace > 0 branch
of the log cannot hold a residual near pi, so it is exercised up to 119 deg (trace 0.03) and the other three at pi - 0.06 deg.
"""
import functools

import numpy as np
import pytest

import rotavg_pcg_ref as R

# printed by scripts/rotavg_roundoff.py: the float64 leg against the longdouble leg, per family (and per step count / path)
ROUNDOFF = {
    "init": 3.72e-16,
    "planted-tiny": 1.93e-07,
    "planted": 7.29e-11,
    "one/1": 2.23e-13,
    "one/2": 2e-13,
    "one/5": 2e-13,
    "one/12": 2.6e-13,
    "many/1": 3.44e-13,
    "many/2": 2e-13,
    "many/5": 2e-13,
    "many/12": 2e-13,
    "tree/1": 1.02e-11,
    "tree/2": 5.36e-12,
    "tree/5": 1.35e-11,
    "tree/12": 0.0182,
    "two/1": 8.7e-13,
    "two/2": 5.22e-13,
    "two/5": 1.93e-13,
    "two/12": 2.24e-13,
    "pair": 3.92e-14,
    "trajectory/one": 1.86e-14,
    "trajectory/many": 1.46e-14,
    "trajectory/tree": 0.00612,
    "trajectory/two": 1.13e-14,
    "converged": 6.54e-12,
}
BOUND = {k: 10.0 * v for k, v in ROUNDOFF.items()}

ONE, MANY, TREE, TWO = R.one_wg_graphs(), R.many_wg_graphs(), R.tree_graphs(), R.two_level_graphs()
PLANTED, TRAJ, CONVERGED = R.planted_graphs(), R.trajectory_graphs(), R.converged_graphs()
FAMILIES = {"one": (ONE, "jacobi"), "many": (MANY, "jacobi"), "tree": (TREE, "tree"), "two": (TWO, "two")}
CASES = [(f, name, phase) for f, (graphs, _) in FAMILIES.items() for name in graphs for phase in R.PHASES]
# the steps the reference can run at most, where a graph cannot avoid converging before n
STEPS_AT_MOST = {("one", "V2"): 1, ("many", "V2"): 1, ("one", "V3"): 2, ("tree", "ring65"): 1}


def _freeze(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def step_reference(family, name, phase):
    graphs, path = FAMILIES[family]
    R0, ref = R.step_rotations(graphs[name], phase, R.STEP_COUNTS, path)
    return _freeze(R0), {n: (_freeze(x), _freeze(Rr), tuple(int(r) for r in ran)) for n, (x, Rr, ran) in ref.items()}


@functools.lru_cache(maxsize=None)
def direct_reference(kind, name, phase):
    g = PLANTED[name] if kind == "planted" else CONVERGED[name][1]
    return tuple(_freeze(a) for a in R.converged_step(g, phase))


@functools.lru_cache(maxsize=None)
def trajectory_reference(name):
    path, g = TRAJ[name]
    R0, Rr, scale, ran = R.trajectory(g, path, **R.TRAJECTORY)
    return _freeze(Rr), scale, ran


def forest_of(g):
    return R.forest(g["V"], g["src"], g["dst"], g["w"])


# ---- CPU: the conditions on the reference legs -------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,phase", CASES)
def test_reference_runs_every_step(family, name, phase):
    """The reference must not converge before n on any axis, or device and reference could agree by both stopping early."""
    _, ref = step_reference(family, name, phase)
    for n, (_, _, ran) in ref.items():
        assert ran == (min(n, STEPS_AT_MOST.get((family, name), n)),) * 3, (family, name, phase, n, ran)


@pytest.mark.parametrize("name", list(TRAJ))
def test_reference_trajectory_runs_every_step(name):
    _, scale, ran = trajectory_reference(name)
    assert len(ran) == 4 and all(tuple(r) == (R.TRAJECTORY["cg_iters"],) * 3 for r in ran) and scale > 1e-3


def test_reference_graphs_take_the_path_they_are_meant_for():
    for g in list(ONE.values()) + list(MANY.values()) + [TRAJ["one"][1], TRAJ["many"][1]]:
        assert len(g["src"]) > 8 * g["V"] or g["V"] > 6144          # a capped Jacobi solve is not diverted to the tree kernel
    for g in list(TREE.values()) + [g for p, g in CONVERGED.values() if p == "tree"]:
        assert len(g["src"]) <= 8 * g["V"] and g["V"] <= 6144
    lanes = {}
    for name, g in ONE.items():
        rl = 16
        while rl > 1 and g["V"] * rl > 1024:
            rl >>= 1
        lanes[name] = rl
    assert [lanes["V%d" % V] for V in (2, 3, 20, 64, 65, 128, 129, 257, 513, 1030)] == [16, 16, 16, 16, 8, 8, 4, 2, 1, 1]
    assert ONE["V1030"]["V"] > 1024                                    # two passes of the product loop
    assert -(-MANY["V4112"]["V"] // 16) == 257                         # the strided partial sum takes a second trip
    assert [-(-TREE[k]["V"] // 1024) for k in ("path1024", "path1025", "seq6144")] == [1, 2, 6]
    for name in R.SHARED_ONE_MANY:
        assert MANY[name] is not None and np.array_equal(MANY[name]["Rrel"], ONE[name]["Rrel"])


def test_reference_topologies_are_what_they_claim():
    g = R.init_graph()
    F = forest_of(g)
    assert len(set(g["w"])) == 1 and list(F["roots"]) == [0, 40, 65, 68] and g["V"] == 69
    assert not np.isin(68, np.r_[g["src"], g["dst"]])
    # the float64 evaluation of the restated forest IS the specification's initialisation
    Ro, roots = R.RO.spanning_forest_init(g["V"], g["src"], g["dst"], g["Rrel"], g["w"])
    assert np.array_equal(roots, F["roots"]) and np.array_equal(Ro, R.forest_rotations(F, g["Rrel"], np.float64))
    assert list(forest_of(ONE["components"])["roots"]) == [0, 24, 54] and ONE["components"]["V"] == 55
    assert list(forest_of(MANY["components"])["roots"]) == [0, 1]
    assert list(forest_of(TREE["components"])["roots"]) == [0, 90, 160] and TREE["components"]["V"] == 161
    assert list(forest_of(TWO["components"])["roots"]) == [0, 1]
    hub = MANY["hub"]
    assert np.bincount(np.r_[hub["src"], hub["dst"]], minlength=300)[77] >= 255 + 16     # more than 16 incidences per lane
    assert forest_of(TREE["star"])["depth"].max() == 1
    for k in ("path200", "path1024", "path1025"):
        assert forest_of(TREE[k])["depth"].max() == TREE[k]["V"] - 1
    ring = TREE["ring65"]
    assert ring["V"] == 65 and len(ring["src"]) == 65 and np.all(np.bincount(np.r_[ring["src"], ring["dst"]]) == 2)
    assert len(forest_of(R.no_plan_graph())["roots"]) == 130


def _shepperd_margin(D):
    """Distance of D from the nearest boundary between the branches of so3_log that matters for it."""
    tr, dg = np.trace(D), np.sort(np.diag(D))
    return abs(tr) if tr > 0 else min(abs(tr), dg[2] - dg[1])


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_residuals_are_where_they_claim(name):
    g = PLANTED[name]
    F = forest_of(g)
    R0 = R.forest_rotations(F, g["Rrel"])
    assert F["depth"].max() == g["V"] - 1 and not np.isin(F["pedge"], [g["V"] - 1]).any()    # the chord is not a forest edge
    D = np.einsum("eji,ejk,ekl->eil", R0[g["dst"]], g["Rrel"].astype(R.LD), R0[g["src"]])
    om = R.log_so3(D)
    ang = np.sqrt((om * om).sum(1))
    assert ang[:g["V"] - 1].max() < 1e-15                             # forest edges: round-off
    chord = g["V"] - 1
    want, axis = R.PLANTED.get(name, (20 * R.DEG, (1, 2, -3)))
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    assert abs(ang[chord] - want) < 1e-15 + 1e-15 * want / 1e-9 and np.abs(om[chord] / ang[chord] - axis).max() < 1e-6
    Dc = D[chord].astype(float)
    assert np.pi - ang[chord] >= 1e-3 and _shepperd_margin(Dc) >= 1e-3
    _, branch = R.mirror_log(Dc[None])
    expect = {"179deg": 3, "pi-x": 1, "pi-y": 2, "pi-z": 3, "pi-x-negative-q0": 1, "pi-z-negative-q0": 3}.get(name, 0)
    assert list(branch[0]).index(True) == expect
    q0_raw = {1: Dc[2, 1] - Dc[1, 2], 2: Dc[0, 2] - Dc[2, 0], 3: Dc[1, 0] - Dc[0, 1]}
    if expect:
        assert (q0_raw[expect] < 0) == name.endswith("negative-q0")   # q0 before the sign flip
    if name == "zero-weight-chord":
        assert g["w"][-1] == 0.0 and (g["w"] == 0.0).sum() == 1
    for phase in R.PHASES:
        _, x, _ = direct_reference("planted", name, phase)
        nx = np.sqrt((np.asarray(x) ** 2).sum(1))
        if name == "1e-9":
            assert 0 < nx.max() < 1e-6                                # the series branch of so3_exp
        elif name != "1e-5":
            assert nx.max() > 1e-6
    assert 1e-5 < 1e-4 < 3e-4 and R.PLANTED["1e-5"][0] == 1e-5 and R.PLANTED["3e-4"][0] == 3e-4   # either side of the L1 clamp


def _connected(members, nb):
    members = set(int(v) for v in members)
    start = next(iter(members))
    seen, todo = {start}, [start]
    while todo:
        for o in nb[todo.pop()]:
            if o in members and o not in seen:
                seen.add(o)
                todo.append(o)
    return seen == members


@pytest.mark.parametrize("name", list(TWO) + ["traj"])
def test_restated_aggregates(name):
    g = TRAJ["two"][1] if name == "traj" else TWO[name]
    F = forest_of(g)
    info = {}
    agg = R.aggregates(g["V"], g["src"], g["dst"], F["roots"], info)
    free = np.ones(g["V"], bool)
    free[F["roots"]] = False
    assert np.all(agg[free] >= 0) and np.all(agg[~free] == -1)         # a partition of the free views
    n = int(agg.max()) + 1
    assert n <= 127 and sorted(set(agg[free])) == list(range(n))
    nb = R.incidence_lists(g["V"], g["src"], g["dst"])
    free_nb = [[o for o in nb[v] if free[o]] for v in range(g["V"])]
    # the components of the graph of the free views
    comp = -np.ones(g["V"], int)
    for v in np.nonzero(free)[0]:
        if comp[v] < 0:
            comp[v] = v
            todo = [int(v)]
            while todo:
                for o in free_nb[todo.pop()]:
                    if comp[o] < 0:
                        comp[o] = v
                        todo.append(o)
    for a in range(n):
        members = np.nonzero(agg == a)[0]
        assert _connected(members, free_nb)
        whole = len(members) == int((comp == comp[members[0]]).sum())
        assert len(members) >= info["target"] // 2 or whole, (name, a, len(members))
    if name == "V20":
        assert n == 1 and (-19) % 16 == 13                             # one aggregate, 13 padding rows
    if name == "V100":
        assert 2 <= n <= 4
    if name == "merge":
        assert info["grown"] > n                                       # a left-over joined a neighbour
    if name == "components":
        assert len(F["roots"]) == 2


def test_graph_of_130_components_has_no_plan():
    g = R.no_plan_graph()
    assert R.aggregates(g["V"], g["src"], g["dst"], forest_of(g)["roots"]) is None


def test_pcg_preconditioners_reach_the_direct_solution():
    """The three preconditioners of the reference converge to the same longdouble solution, which the oracle's sparse
    direct solve confirms to float64."""
    g = ONE["V64"]
    _, x, R_ref = R.converged_step(g, "l1")
    Ro, _ = R.RO.rotation_average(g["V"], g["src"], g["dst"], g["Rrel"], g["w"], l1_iters=1, irls_iters=0, tol=0.0)
    assert np.abs(R_ref - Ro).max() < 1e-13
    F, R0 = R._setup(g)
    om, w = R.residual_and_weights(g, R0, "l1")
    S = R.System(g["V"], g["src"], g["dst"], w, om, F["roots"])
    for path in ("jacobi", "tree", "two"):
        xp, ran = R.pcg(S, 3000, R._preconditioner(S, g, F, path), tol=1e-17)
        assert ran.max() < 3000 and xp.dtype == R.LD
        assert np.abs(xp - x).max() <= 1e-15 * np.abs(x).max(), path


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


PATH_ENV = {"one": {"PGI_ROTAVG_SINGLE_WG_VIEWS": "1000000", "PGI_ROTAVG_TWO_LEVEL": "0"},
            "many": {"PGI_ROTAVG_SINGLE_WG_VIEWS": "0", "PGI_ROTAVG_TWO_LEVEL": "0"},
            "tree": {"PGI_ROTAVG_TWO_LEVEL": "0"},
            "two": {"PGI_ROTAVG_TWO_LEVEL": "2"}}


def run(eng, mp, g, family, n, tol=R.FIXED_STEP_TOL, **kw):
    """One call on a solver path: n PCG steps per solve (n = None: no cap that matters)."""
    for k in ("PGI_ROTAVG_SINGLE_WG_VIEWS", "PGI_ROTAVG_TWO_LEVEL", "PGI_ROTAVG_TREE_CG_ITERS", "PGI_ROTAVG_CG_ITERS", "PGI_ROTAVG_TRACE"):
        mp.delenv(k, raising=False)
    for k, v in PATH_ENV[family].items():
        mp.setenv(k, v)
    mp.setenv("PGI_ROTAVG_CG_TOL", "%g" % tol)
    cg = 2000 if n is None else n
    if family == "tree":
        if n is not None:
            mp.setenv("PGI_ROTAVG_TREE_CG_ITERS", "%d" % n)
        cg = kw.pop("jacobi_cap", 1)          # the Jacobi solve runs into this cap and the tree kernel re-solves the step
    return eng.rotation_average(g["src"], g["dst"], g["Rrel"], g["w"], g["V"], cg_iters=cg, tol=0.0, **kw)


@pytest.mark.gpu
def test_hip_initialisation(eng, monkeypatch):
    """l1_iters = irls_iters = 0: the forest initialisation itself; all weights equal, so (weight desc, index asc) decides."""
    g = R.init_graph()
    F = forest_of(g)
    R_ref = R.forest_rotations(F, g["Rrel"])
    Rd, iters = run(eng, monkeypatch, g, "one", 5, l1_iters=0, irls_iters=0)
    d = float(np.abs(Rd.astype(R.LD) - R_ref).max())
    print("initialisation: |R - R0| %.3g (bound %.3g)" % (d, BOUND["init"]))
    assert iters == 0 and d <= BOUND["init"]
    assert np.array_equal(Rd[F["roots"]], np.tile(np.eye(3), (4, 1, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("name", list(PLANTED))
def test_hip_residual_weights_update(eng, monkeypatch, name, phase):
    """rot_residual_kernel and rot_update_kernel on a planted residual: one converged step against the direct solve."""
    g = PLANTED[name]
    _, x, R_ref = direct_reference("planted", name, phase)
    fam = "planted-tiny" if name in R.PLANTED_TINY else "planted"
    Rd, iters = run(eng, monkeypatch, g, "one", None, **R.PHASE_KW[phase])
    d = R.distance(Rd, R_ref, x)
    print("%s %s: |x| %.3g, distance %.3g (bound %.3g)" % (name, phase, R.step_scale(x), d, BOUND[fam]))
    assert iters == 1 and d <= BOUND[fam]


@pytest.mark.gpu
@pytest.mark.parametrize("family,name,phase", CASES)
def test_hip_fixed_step(eng, monkeypatch, family, name, phase):
    """R0 exp(x_n) for n = 1, 2, 5, 12 on each solver path; every call twice: the same bits."""
    g = FAMILIES[family][0][name]
    _, ref = step_reference(family, name, phase)
    worst = 0.0
    for n in R.STEP_COUNTS:
        x, R_ref, ran = ref[n]
        Rd, iters = run(eng, monkeypatch, g, family, n, **R.PHASE_KW[phase])
        Rd2, _ = run(eng, monkeypatch, g, family, n, **R.PHASE_KW[phase])
        d = R.distance(Rd, R_ref, x)
        worst = max(worst, d)
        bound = BOUND["%s/%d" % (family, n)]
        print("%s %s %s n = %d (reference ran %s): distance %.3g (bound %.3g)" % (family, name, phase, n, ran, d, bound))
        assert iters == 1 and np.array_equal(Rd, Rd2)
        assert d <= bound, (family, name, phase, n, d)
    print("%s %s %s: largest %.3g" % (family, name, phase, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("name", R.SHARED_ONE_MANY)
def test_hip_one_workgroup_against_many(eng, monkeypatch, name, phase):
    """rot_solve_kernel against cg_init_kernel / cg_iteration_kernel on the same graph."""
    g = ONE[name]
    _, ref = step_reference("one", name, phase)
    for n in R.STEP_COUNTS:
        Ra, _ = run(eng, monkeypatch, g, "one", n, **R.PHASE_KW[phase])
        Rb, _ = run(eng, monkeypatch, g, "many", n, **R.PHASE_KW[phase])
        d = R.distance(Ra, Rb.astype(R.LD), ref[n][0])
        print("%s %s n = %d: one workgroup against many %.3g (bound %.3g)" % (name, phase, n, d, BOUND["pair"]))
        assert d <= BOUND["pair"]


@pytest.mark.gpu
@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("name", list(CONVERGED))
def test_hip_converged_step(eng, monkeypatch, name, phase):
    """PGI_ROTAVG_CG_TOL = 1e-12 and no cap that matters (the tree override unset: its cap is 1000) against the direct solve."""
    path, g = CONVERGED[name]
    _, x, R_ref = direct_reference("converged", name, phase)
    Rd, iters = run(eng, monkeypatch, g, path, None, tol=R.CONVERGED_TOL, **R.PHASE_KW[phase])
    d = R.distance(Rd, R_ref, x)
    print("%s %s: distance to the direct solve %.3g (bound %.3g)" % (name, phase, d, BOUND["converged"]))
    assert iters == 1 and d <= BOUND["converged"]


@pytest.mark.gpu
def test_hip_two_level_without_a_plan_is_the_one_level_solve(eng, monkeypatch):
    """130 components of three views cannot have a plan: PGI_ROTAVG_TWO_LEVEL = 2 and 0 give the same bits."""
    g = R.no_plan_graph()
    got = {}
    for mode in ("2", "0"):
        for k in ("PGI_ROTAVG_SINGLE_WG_VIEWS", "PGI_ROTAVG_TREE_CG_ITERS", "PGI_ROTAVG_CG_ITERS", "PGI_ROTAVG_CG_TOL"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("PGI_ROTAVG_TWO_LEVEL", mode)
        got[mode] = eng.rotation_average(g["src"], g["dst"], g["Rrel"], g["w"], g["V"])
    assert got["2"][1] == got["0"][1] > 0 and np.array_equal(got["2"][0], got["0"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRAJ))
def test_hip_fixed_step_trajectory(eng, monkeypatch, name):
    """Two L1 and two IRLS outer iterations of twelve PCG steps on each path: residual, weights and update over several
    outer steps."""
    path, g = TRAJ[name]
    R_ref, scale, _ = trajectory_reference(name)
    kw = dict(l1_iters=R.TRAJECTORY["l1_iters"], irls_iters=R.TRAJECTORY["irls_iters"])
    n = R.TRAJECTORY["cg_iters"]
    Rd, iters = run(eng, monkeypatch, g, name, n, jacobi_cap=n, **kw) if name == "tree" else run(eng, monkeypatch, g, name, n, **kw)
    d = R.distance(Rd, R_ref, scale)
    print("trajectory %s: iters %d, distance %.3g (bound %.3g)" % (name, iters, d, BOUND["trajectory/" + name]))
    assert iters == 4 and d <= BOUND["trajectory/" + name]
