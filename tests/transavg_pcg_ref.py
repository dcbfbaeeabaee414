"""transavg_pcg_ref.py -- n-step reference of the translation averaging's inner solver (test infrastructure).

tests/transavg_spec.py solves every outer system directly, so it can be compared with the device only where the device's
block-Jacobi PCG has converged.  The device solver is deterministic and its parameters are exposed: with iters = 1 and
cg_iters = n it returns c0 + x_n, x_n being the n-th PCG iterate of the STEP system (rhs b - A c0).  This file restates
that recurrence on the system tests/transavg_spec.py assembles, in a dtype of the caller's choice:

  pcg_steps   block-Jacobi PCG of at most n steps from x = 0, the device's stopping rule;  np.longdouble = the reference
  irls_fixed  the outer loop of transavg_spec.translation_average with every solve replaced by pcg_steps on the step
  mirror_*    a float64 leg that follows the KERNEL's formulas (closed-form adjugate inverse, omega M_e as
              omega I + omega (lambda - 1) gamma gamma^T, per-view sums over the adjacency in edge order).  It exists for
              scripts/transavg_roundoff.py alone: its distance to the longdouble leg, with the edges in two orders, is the
              round-off figure that bounds the GPU tests.  No GPU test compares the device with it.
"""
import numpy as np

import transavg_spec as TS

DEVICE_CG_TOL = 1e-4  # kTrnInnerTolerance of csrc/pgi_transavg.hip


def _block_diag_inverse(A, dtype):
    """Inverse of every 3 x 3 diagonal block of A (adjugate over determinant, evaluated in `dtype`; zero where the
    determinant is not positive, like the device) -> [n / 3, 3, 3]."""
    n = A.shape[0] // 3
    D = np.zeros((n, 3, 3), dtype)
    coo = A.tocoo()
    m = (coo.row // 3) == (coo.col // 3)
    np.add.at(D, (coo.row[m] // 3, coo.row[m] % 3, coo.col[m] % 3), coo.data[m].astype(dtype))
    a, b, c, d, e, f = D[:, 0, 0], D[:, 0, 1], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    k = np.where(det > 0, 1 / np.where(det > 0, det, 1), 0).astype(dtype)
    inv = np.empty_like(D)
    inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2] = c00 * k, c01 * k, c02 * k
    inv[:, 1, 0], inv[:, 1, 1], inv[:, 1, 2] = c01 * k, c11 * k, c12 * k
    inv[:, 2, 0], inv[:, 2, 1], inv[:, 2, 2] = c02 * k, c12 * k, c22 * k
    return inv


def _csr_matvec(indptr, indices, data, x):
    """y = A x for a CSR matrix without empty rows, in the dtype of data and x (scipy's kernels stop at float64)."""
    return np.add.reduceat(data * x[indices], indptr[:-1])


def pcg_steps(A, b, n, tol=DEVICE_CG_TOL, dtype=np.longdouble, record=None):
    """Block-Jacobi PCG on A x = b from x = 0, z = D^-1 r per 3 x 3 diagonal block, at most n iterations, stopped BEFORE an
    iteration when not (rz > tol^2 rz0) -- the rule of trn_solve_kernel and trn_cg_direction_kernel.  -> (x, iterations).
    record: a dict; record[k] receives a copy of the iterate after k iterations for every key k already in it."""
    A = A.tocsr()
    A.sort_indices()
    assert np.all(np.diff(A.indptr) > 0)
    indptr, indices, data = A.indptr, A.indices, A.data.astype(dtype)
    Dinv = _block_diag_inverse(A, dtype)
    tol = dtype(tol)

    def precond(r):
        return np.einsum("vij,vj->vi", Dinv, r.reshape(-1, 3)).reshape(-1)
    x = np.zeros(len(b), dtype)
    r = np.asarray(b, dtype).copy()
    z = precond(r)
    p = z.copy()
    rz = rz0 = r @ z
    it = 0
    while it < n:
        if not rz > tol * tol * rz0:
            break
        q = _csr_matvec(indptr, indices, data, p)
        pq = p @ q
        alpha = rz / pq if pq > 0 else dtype(0)
        x += alpha * p
        r -= alpha * q
        z = precond(r)
        rzn = r @ z
        beta = rzn / rz if rz > 0 else dtype(0)
        p = z + beta * p
        rz = rzn
        it += 1
        if record is not None and it in record:
            record[it] = x.copy()
    return x, it


def step_system(n_views, src, dst, gamma, weight, c, free, eps, delta, dtype=np.longdouble):
    """The system of one outer iteration for the STEP: (A restricted to the free views, b - A c in `dtype`, clamped mask,
    a = <D, gamma> per edge).  The model and the assembly are transavg_spec's own float64 ones."""
    P, g, clamped = TS.edge_model(c, src, dst, gamma, weight, eps, delta)
    A, b = TS.assemble(n_views, src, dst, P, g, free)
    A = A.tocsr()
    A.sort_indices()
    cf = c[free].reshape(-1).astype(dtype)
    rhs = b.astype(dtype) - _csr_matvec(A.indptr, A.indices, A.data.astype(dtype), cf)
    D = c[src] - c[dst]
    a = (D[:, 0] * gamma[:, 0] + D[:, 1] * gamma[:, 1]) + D[:, 2] * gamma[:, 2]
    return A, rhs, clamped, a


def irls_fixed(n_views, src, dst, gamma, weight, iters=60, cg_iters=200, cg_tol=DEVICE_CG_TOL, eps=1e-3, delta=1e-4, tol=1e-9,
               dtype=np.longdouble, trace=None):
    """The outer loop of transavg_spec.translation_average with every solve replaced by pcg_steps on the step (rhs b - A c,
    c += x), the positions kept in float64 between the outer iterations as on the device.  -> (c [V,3] float64, iters).
    trace: a list that receives per outer iteration a dict: cg (PCG iterations), step (mean |x|), a (<D, gamma> per edge,
    before the step), clamped (count)."""
    src, dst = np.asarray(src, int), np.asarray(dst, int)
    gamma = np.asarray(gamma, float).reshape(-1, 3)
    weight = np.asarray(weight, float)
    c, roots = TS.spanning_forest_init(n_views, src, dst, gamma, weight)
    free = np.ones(n_views, bool)
    free[roots] = False
    done = 0
    if len(src) == 0 or not free.any():
        return c, done
    cap = max(1, cg_iters)   # the device clamps cg_iters = 0 to 1
    for it in range(iters):
        A, rhs, clamped, a = step_system(n_views, src, dst, gamma, weight, c, free, eps, delta, dtype)
        x, n = pcg_steps(A, rhs, cap, cg_tol, dtype)
        xv = np.zeros((n_views, 3), dtype)
        xv[free] = x.reshape(-1, 3)
        step = float(np.mean(np.sqrt((xv * xv).sum(1))))
        c = (c.astype(dtype) + xv).astype(np.float64)
        done = it + 1
        if trace is not None:
            trace.append(dict(cg=n, step=step, a=a, clamped=int(clamped.sum())))
        if step < tol:
            break
    return c, done


# ---- the float64 leg that follows the kernel's formulas (for scripts/transavg_roundoff.py) ---------------------------
def _mirror_model(c, src, dst, gamma, weight, eps, delta):
    """trn_model_kernel: -> (P [E,6] as xx xy xz yy yz zz, g [E,3])."""
    D = c[src] - c[dst]
    a = (D[:, 0] * gamma[:, 0] + D[:, 1] * gamma[:, 1]) + D[:, 2] * gamma[:, 2]
    clamped = a <= 1.0
    tau, lam = np.where(clamped, 1.0, a), np.where(clamped, 1.0, eps)
    q = D - tau[:, None] * gamma
    r = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    om = weight / np.maximum(r, delta)
    s = om * (lam - 1.0)
    x, y, z = gamma[:, 0], gamma[:, 1], gamma[:, 2]
    P = np.stack([om + s * (x * x), s * (x * y), s * (x * z), om + s * (y * y), s * (y * z), om + s * (z * z)], 1)
    return P, ((om * lam) * tau)[:, None] * gamma


def _sym_mul(S, v):
    return np.stack([(S[:, 0] * v[:, 0] + S[:, 1] * v[:, 1]) + S[:, 2] * v[:, 2],
                     (S[:, 1] * v[:, 0] + S[:, 3] * v[:, 1]) + S[:, 4] * v[:, 2],
                     (S[:, 2] * v[:, 0] + S[:, 4] * v[:, 1]) + S[:, 5] * v[:, 2]], 1)


def _sym_inv(S):
    c00, c01, c02 = S[:, 3] * S[:, 5] - S[:, 4] * S[:, 4], S[:, 2] * S[:, 4] - S[:, 1] * S[:, 5], S[:, 1] * S[:, 4] - S[:, 2] * S[:, 3]
    c11, c12, c22 = S[:, 0] * S[:, 5] - S[:, 2] * S[:, 2], S[:, 1] * S[:, 2] - S[:, 0] * S[:, 4], S[:, 0] * S[:, 3] - S[:, 1] * S[:, 1]
    det = (S[:, 0] * c00 + S[:, 1] * c01) + S[:, 2] * c02
    k = np.where(det > 0.0, 1.0 / np.where(det > 0.0, det, 1.0), 0.0)
    return np.stack([c00 * k, c01 * k, c02 * k, c11 * k, c12 * k, c22 * k], 1)


def _lapack_inv(S):
    M = np.stack([S[:, [0, 1, 2]], S[:, [1, 3, 4]], S[:, [2, 4, 5]]], 1)
    ok = np.linalg.det(M) > 0
    I = np.zeros_like(M)
    I[ok] = np.linalg.inv(M[ok])
    return np.stack([I[:, 0, 0], I[:, 0, 1], I[:, 0, 2], I[:, 1, 1], I[:, 1, 2], I[:, 2, 2]], 1)


def mirror_irls_fixed(n_views, src, dst, gamma, weight, c0, roots, iters, cg_iters, cg_tol=DEVICE_CG_TOL, eps=1e-3, delta=1e-4,
                      tol=1e-9, lapack_inverse=False):
    """The device's data path in float64 numpy: model, view rows, PCG and step as the kernels write them, every per-view
    sum over the incidences in edge order (np.add.at adds in index order).  c0, roots: the initialisation (passed in, so
    that a permuted edge list starts from the same point).  lapack_inverse: invert the diagonal blocks with LAPACK instead
    of the adjugate.  -> (c, iters, PCG iterations per outer iteration)."""
    src, dst = np.asarray(src, int), np.asarray(dst, int)
    E = len(src)
    # incidences sorted by (view, edge): the CSR adjacency of transavg_solve
    view = np.concatenate([src, dst])
    other = np.concatenate([dst, src])
    edge = np.concatenate([np.arange(E), np.arange(E)])
    sign = np.concatenate([np.ones(E), -np.ones(E)])
    o = np.lexsort((edge, view))
    view, other, edge, sign = view[o], other[o], edge[o], sign[o]
    live = np.ones(n_views, bool)
    live[roots] = False
    keep = live[view]
    view, other, edge, sign = view[keep], other[keep], edge[keep], sign[keep]

    def view_sum(t):
        y = np.zeros((n_views, t.shape[1]))
        np.add.at(y, view, t)
        return y
    c = np.array(c0, float)
    cgs, done = [], 0
    for it in range(iters):
        P, g = _mirror_model(c, src, dst, gamma, weight, eps, delta)
        Pa = P[edge]
        Dg = view_sum(Pa)
        r = view_sum(sign[:, None] * g[edge] - _sym_mul(Pa, c[view] - c[other]))
        Dinv = _lapack_inv(Dg) if lapack_inverse else _sym_inv(Dg)
        Dinv[~live] = 0.0
        z = _sym_mul(Dinv, r)
        p = z.copy()
        x = np.zeros_like(c)
        rz = rz0 = float((r * z).sum())
        n = 0
        while n < max(1, cg_iters):
            if not rz > cg_tol * cg_tol * rz0:
                break
            q = view_sum(_sym_mul(Pa, p[view] - p[other]))
            pq = float((p * q).sum())
            alpha = rz / pq if pq > 0.0 else 0.0
            x += alpha * p
            r -= alpha * q
            z = _sym_mul(Dinv, r)
            rzn = float((r * z).sum())
            beta = rzn / rz if rz > 0.0 else 0.0
            p = z + beta * p
            rz = rzn
            n += 1
        cgs.append(n)
        step = float(np.mean(np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])))
        c = c + x
        done = it + 1
        if step < tol:
            break
    return c, done, cgs


# ---- the graphs of tests/test_transavg_steps.py (shared with scripts/transavg_roundoff.py) ---------------------------
def _graph(V, src, dst, gamma, w):
    return dict(V=int(V), src=np.asarray(src, int), dst=np.asarray(dst, int), gamma=np.asarray(gamma, float), w=np.asarray(w, float))


def random_graph(V, k, seed, noise_deg=1.0, outlier_frac=0.1):
    src, dst, gamma, w, _, _ = TS.make_graph(V, k, noise_deg, outlier_frac, seed=seed)
    return _graph(V, src, dst, gamma, w)


def single_edge_graph():
    g = np.array([[2.0, -1.0, 2.0]]) / 3.0
    return _graph(2, [0], [1], g, [0.7])


def two_range_components(V, k=4, seed=5):
    """Views 0..99 and 100..V-1 are two components: the second gauge view is view 100."""
    a, b = random_graph(100, k, seed), random_graph(V - 100, k, seed + 1)
    return _graph(V, np.r_[a["src"], b["src"] + 100], np.r_[a["dst"], b["dst"] + 100], np.r_[a["gamma"], b["gamma"]],
                  np.r_[a["w"], b["w"]])


def with_isolated_views(V, k=4, seed=6):
    """Views V // 3, 2 V // 3 and V - 1 have no edge."""
    lone = np.array([V // 3, 2 * V // 3, V - 1])
    ids = np.setdiff1d(np.arange(V), lone)
    a = random_graph(V - 3, k, seed)
    return _graph(V, ids[a["src"]], ids[a["dst"]], a["gamma"], a["w"]), lone


def doubled_edges(V, k=3, seed=7):
    """Every edge twice: as it is and reversed (direction negated) with a weight of its own."""
    a = random_graph(V, k, seed)
    w2 = np.random.default_rng(seed + 100).uniform(0.2, 1.0, len(a["w"]))
    return _graph(V, np.r_[a["src"], a["dst"]], np.r_[a["dst"], a["src"]], np.r_[a["gamma"], -a["gamma"]], np.r_[a["w"], w2])


def hub_and_ring(V, hub, spokes, seed=8):
    """View `hub` joined to `spokes` other views, plus the ring v -- v + 1 over all views; directions from random centres
    with 1 degree of noise."""
    rng = np.random.default_rng(seed)
    c_gt = rng.standard_normal((V, 3)) * 5.0
    others = np.setdiff1d(np.arange(V), [hub])
    far = others[(others != (hub + 1) % V) & (others != (hub - 1) % V)]
    ends = np.sort(rng.choice(far, size=spokes - 2, replace=False))   # the ring supplies the two neighbours
    src = np.r_[np.arange(V), np.full(len(ends), hub)]
    dst = np.r_[(np.arange(V) + 1) % V, ends]
    flip = rng.random(len(src)) < 0.5
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    gamma = c_gt[src] - c_gt[dst]
    gamma /= np.linalg.norm(gamma, axis=1, keepdims=True)
    noise = TS._rodrigues(rng.standard_normal((len(src), 3)) * np.deg2rad(1.0) / np.sqrt(3))
    gamma = np.einsum("eij,ej->ei", noise, gamma)
    return _graph(V, src, dst, gamma, rng.uniform(0.4, 1.0, len(src)))


def zero_weight_chord(V, k=4, seed=9):
    """One edge outside the spanning forest gets weight 0 -> (graph, its index)."""
    a = random_graph(V, k, seed)
    deg = np.bincount(np.r_[a["src"], a["dst"]], minlength=V)
    e = int(np.nonzero((deg[a["src"]] > 2) & (deg[a["dst"]] > 2))[0][len(a["src"]) // 2])
    a["w"][e] = 0.0
    return a, e


STEP_COUNTS = (1, 2, 3, 16, 17, 33)   # 16, 17 and 33 straddle the host's looks at the state record (16, 32, 48, ...)
TOPOLOGY_STEPS = 17
TRAJECTORY = dict(iters=4, cg_iters=20)
CONVERGED = dict(iters=3, cg_iters=2000, cg_tol=1e-11, delta=1.0)


def parity_graphs():
    """Fixed-step parity: one workgroup up to V = 256, 64-lane workgroups above; 4161 views = 66 of them."""
    out = {"V2": single_edge_graph()}
    for V, k in ((12, 3), (64, 4), (255, 4), (256, 4), (257, 4), (320, 4), (321, 4), (4161, 3)):
        out["V%d" % V] = random_graph(V, k, seed=V)
    return out


def topology_graphs():
    """Every topology once at V <= 256 and once above.  The hub has 300 spokes where the graph has that many views; the
    one-workgroup case joins it to all 255 others."""
    return {"components-V200": two_range_components(200), "components-V300": two_range_components(300),
            "isolated-V200": with_isolated_views(200)[0], "isolated-V330": with_isolated_views(330)[0],
            "doubled-V30": doubled_edges(30), "doubled-V260": doubled_edges(260),
            "hub-V256": hub_and_ring(256, 100, 255), "hub-V330": hub_and_ring(330, 200, 300),
            "zero-weight-V200": zero_weight_chord(200)[0], "zero-weight-V300": zero_weight_chord(300)[0]}


def trajectory_graphs():
    return {"V50": random_graph(50, 6, seed=50, noise_deg=1.0, outlier_frac=0.15), "V321": random_graph(321, 4, seed=321)}


def converged_graphs():
    return {"V12": random_graph(12, 3, seed=12), "V257": random_graph(257, 4, seed=257), "V320": random_graph(320, 4, seed=320)}


def first_step_reference(g, counts, tol=DEVICE_CG_TOL, dtype=np.longdouble):
    """iters = 1: -> (c0, {n: (c0 + x_n as float64 [V,3], iterations run)} for n in counts)."""
    V = g["V"]
    c0, roots = TS.spanning_forest_init(V, g["src"], g["dst"], g["gamma"], g["w"])
    free = np.ones(V, bool)
    free[roots] = False
    A, rhs, _, _ = step_system(V, g["src"], g["dst"], g["gamma"], g["w"], c0, free, 1e-3, 1e-4, dtype)
    record = {n: None for n in counts}
    x, ran = pcg_steps(A, rhs, max(counts), tol, dtype, record)
    out = {}
    for n in counts:
        xn = record[n] if record[n] is not None else x   # stopped before n: the last iterate
        c = c0.astype(dtype)
        c[free] += xn.reshape(-1, 3)
        out[n] = (c.astype(np.float64), min(n, ran))
    return c0, out


def distance(c, c_ref, c0):
    """max |c - c_ref| over the views / max |c_ref - c0|: the error of the step, relative to the largest step.  Where the
    reference does not move at all (a single edge: the initialisation is the solution) the scale is max |c_ref|."""
    scale = float(np.linalg.norm(c_ref - c0, axis=1).max())
    if scale == 0.0:
        scale = float(np.linalg.norm(c_ref, axis=1).max())
    return float(np.linalg.norm(c - c_ref, axis=1).max()) / scale
