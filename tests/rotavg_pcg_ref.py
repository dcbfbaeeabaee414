"""rotavg_pcg_ref.py -- n-step reference of the rotation averaging's inner solvers (test infrastructure).

oracle/rotavg_oracle.py solves every outer system directly, so it can be compared with the device only after convergence.
The device solvers are deterministic and their parameters are exposed: with l1_iters + irls_iters = 1, cg_iters = n and
PGI_ROTAVG_CG_TOL = 1e-14 the engine returns R0 exp(x_n), R0 the spanning-forest initialisation and x_n the n-th PCG
iterate of the first system (three independent systems, one per axis).  This file restates that in numpy longdouble:

  forest / forest_rotations  the initialisation of rotavg_oracle.spanning_forest_init, the products in a dtype of choice
  residual_and_weights       omega = log(R_dst^T R_rel R_src) through a unit quaternion, L1 / Geman-McClure weights
  System, pcg                the grounded weighted Laplacian per axis, textbook PCG with the Jacobi, tree (L_T^-1 by two
                             sweeps over the forest) and two-level (D^-1 + P Ac^-1 P^T) preconditioners
  aggregates                 the region-growing rule of plan_two_level, restated
  step_rotations, trajectory, converged_step, distance
  mirror_*                   a float64 leg that follows the KERNELS' formulas (Shepperd-branch log, series exp, per-view sums
                             in incidence order, plain and Chronopoulos-Gear recurrences, prefix-sum tree solve, Gauss-Jordan
                             without pivoting).  It exists for scripts/rotavg_roundoff.py alone: its distance to the
                             longdouble leg is the round-off figure that bounds the GPU tests.  No GPU test compares the
                             device with it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rotavg_oracle as RO  # noqa: E402

LD = np.longdouble
FIXED_STEP_TOL = 1e-14            # PGI_ROTAVG_CG_TOL of the fixed-step tests (the smallest value the engine accepts)
CONVERGED_TOL = 1e-12             # ... of the converged one-step regime
SIGMA = 5.0 * 3.14159265358979323846 / 180.0   # rotavg_solve's sigma for sigma_deg = 5
STEP_COUNTS = (1, 2, 5, 12)
TRAJECTORY = dict(l1_iters=2, irls_iters=2, cg_iters=12)


# ---- graphs ------------------------------------------------------------------------------------------------------------
def _graph(V, src, dst, Rrel, w):
    return dict(V=int(V), src=np.asarray(src, int), dst=np.asarray(dst, int), Rrel=np.asarray(Rrel, float).reshape(-1, 3, 3),
                w=np.asarray(w, float))


def sequence_graph(V, reach, noise_deg, outlier_frac, seed, components=1):
    """An image-sequence view graph: view i sees views i+1 .. i+reach (per component), like a video or a walk-through.
    Its Laplacian is banded: Jacobi-preconditioned CG needs ~(V / reach) iterations times a large constant."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    Rgt = Rotation.random(V, random_state=seed).as_matrix()
    src, dst = [], []
    for c in range(components):
        idx = np.arange(c, V, components)
        for a in range(len(idx)):
            for s_ in range(1, reach + 1):
                if a + s_ < len(idx):
                    i, j = (idx[a], idx[a + s_]) if rng.random() < 0.5 else (idx[a + s_], idx[a])
                    src.append(i); dst.append(j)
    src, dst = np.array(src), np.array(dst)
    Rrel = np.einsum("eij,ekj->eik", Rgt[dst], Rgt[src])
    Rrel = np.einsum("eij,ejk->eik", Rotation.from_rotvec(rng.standard_normal((len(src), 3)) * np.deg2rad(noise_deg) / np.sqrt(3)).as_matrix(), Rrel)
    out = rng.random(len(src)) < outlier_frac
    Rrel[out] = Rotation.random(int(out.sum()), random_state=seed + 1).as_matrix()
    w = np.where(out, rng.uniform(0.1, 0.4, len(src)), rng.uniform(0.4, 1.0, len(src)))
    return src, dst, Rrel, w, Rgt


def random_graph(V, k, seed, components=1):
    src, dst, Rrel, w, _, _ = RO.make_graph(V, k, 1.0, 0.1, seed=seed, components=components)
    return _graph(V, src, dst, Rrel, w)


# With a degree of noise the L1 weights of the first step are w / 1e-4 on the forest (residuals of round-off) and ~ w / 0.02 off
# it: the forest is then nearly the whole matrix and the tree-preconditioned PCG is done in a handful of steps.  At 0.003
# degrees most residuals sit under the clamp, all weights are alike and the solve needs its iterations.
TREE_NOISE_DEG = 0.003


def seq_graph(V, reach, seed, components=1, noise_deg=1.0):
    return _graph(V, *sequence_graph(V, reach, noise_deg, 0.05, seed, components)[:4])


def edges_graph(V, src, dst, seed, w=None, noise_deg=1.0, outlier_frac=0.1):
    """Noisy relative rotations (and weights) for a given edge list: every edge its own noise, parallel edges included."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    src, dst = np.asarray(src, int), np.asarray(dst, int)
    E = len(src)
    Rgt = Rotation.random(V, random_state=seed).as_matrix()
    Rrel = np.einsum("eij,ekj->eik", Rgt[dst], Rgt[src])
    Rrel = np.einsum("eij,ejk->eik", Rotation.from_rotvec(rng.standard_normal((E, 3)) * np.deg2rad(noise_deg) / np.sqrt(3)).as_matrix(), Rrel)
    out = rng.random(E) < outlier_frac
    Rrel[out] = Rotation.random(int(out.sum()), random_state=seed + 1).as_matrix()
    wr = np.where(out, rng.uniform(0.1, 0.4, E), rng.uniform(0.4, 1.0, E))
    return _graph(V, src, dst, Rrel, wr if w is None else w)


def dense_multigraph(V, seed, per_view=9):
    """The ring over all views plus per_view * V random pairs, repetitions allowed (a simple graph on fewer than 18 views
    cannot have E > 8 V)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, V, per_view * V)
    b = (a + rng.integers(1, V, per_view * V)) % V
    ring = np.arange(V if V > 2 else 1)
    src, dst = np.r_[ring, a], np.r_[(ring + 1) % V, b]
    flip = rng.random(len(src)) < 0.5
    return edges_graph(V, np.where(flip, dst, src), np.where(flip, src, dst), seed)


def join(parts, isolated=0):
    """The graphs side by side as components of one (view ids shifted), `isolated` views without an edge appended."""
    off, src, dst, Rrel, w = 0, [], [], [], []
    for g in parts:
        src.append(g["src"] + off); dst.append(g["dst"] + off); Rrel.append(g["Rrel"]); w.append(g["w"])
        off += g["V"]
    return _graph(off + isolated, np.concatenate(src), np.concatenate(dst), np.concatenate(Rrel), np.concatenate(w))


def hub_graph(V, hub, spokes, seed):
    """random_graph(V, 10) plus edges from view `hub` to `spokes` other views."""
    g = random_graph(V, 10, seed)
    rng = np.random.default_rng(seed + 1)
    ends = np.sort(rng.choice(np.setdiff1d(np.arange(V), [hub]), spokes, replace=False))
    h = edges_graph(V, np.full(spokes, hub), ends, seed + 2)
    return _graph(V, np.r_[g["src"], h["src"]], np.r_[g["dst"], h["dst"]], np.r_[g["Rrel"], h["Rrel"]], np.r_[g["w"], h["w"]])


def ring_graph(V, seed):
    i = np.arange(V)
    return edges_graph(V, i, (i + 1) % V, seed, outlier_frac=0.0)


def path_with_closures(V, seed, closures=None):
    """The path 0 - 1 - ... - V-1 with heavy edges (the maximum-weight forest: depth V - 1) and light long-range closures."""
    rng = np.random.default_rng(seed)
    n = V if closures is None else closures
    a = rng.integers(0, V - 3, n)
    b = np.minimum(V - 1, a + rng.integers(2, max(3, V // 3), n))
    i = np.arange(V - 1)
    w = np.r_[rng.uniform(0.8, 1.0, V - 1), rng.uniform(0.5, 0.79, n)]
    return edges_graph(V, np.r_[i, a], np.r_[i + 1, b], seed, w=w, noise_deg=TREE_NOISE_DEG, outlier_frac=0.05)


def star_with_chords(V, seed):
    """View 0 joined to every other view by heavy edges (the forest: depth 1) and V light chords among the others."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, V, 2 * V)
    b = 1 + (a - 1 + rng.integers(1, V - 1, 2 * V)) % (V - 1)
    i = np.arange(1, V)
    w = np.r_[rng.uniform(0.8, 1.0, V - 1), rng.uniform(0.5, 0.79, 2 * V)]
    return edges_graph(V, np.r_[np.zeros(V - 1, int), a], np.r_[i, b], seed, w=w, noise_deg=TREE_NOISE_DEG, outlier_frac=0.05)


def init_graph():
    """All weights equal, so the tie-break (weight desc, index asc) decides the forest: a 40-view path with chords listed
    BEFORE some of its path edges, a random component, a triangle and an isolated view."""
    rng = np.random.default_rng(77)
    i = np.arange(39)
    a = rng.integers(0, 36, 30)
    b = a + rng.integers(2, 4, 30)
    o = rng.permutation(69)
    p = edges_graph(40, np.r_[i, a][o], np.r_[i + 1, b][o], 77)
    g = join([p, random_graph(25, 4, 78), edges_graph(3, [0, 1, 2], [1, 2, 0], 79)], isolated=1)
    g["w"] = np.full(len(g["src"]), 0.5)
    return g


def _rodrigues_ld(v):
    v = np.asarray(v, LD)
    t = np.sqrt((v * v).sum())
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], LD)
    if t < LD(1e-8):
        return np.eye(3, dtype=LD) + K + K @ K / 2
    return np.eye(3, dtype=LD) + (np.sin(t) / t) * K + ((1 - np.cos(t)) / (t * t)) * (K @ K)


def planted_graph(angle, axis, views=4, seed=3, zero_chord=False):
    """A path of `views` views (heavy edges: the forest) and the chord 0 -> views-1 whose relative rotation is chosen so that
    R_dst^T R_rel R_src = exp(angle axis / |axis|) at the initialisation (to the rounding of R_rel to float64).
    zero_chord: a second chord 0 -> views-2 of weight 0 with an arbitrary rotation."""
    from scipy.spatial.transform import Rotation
    Rgt = Rotation.random(views, random_state=seed).as_matrix()
    i = np.arange(views - 1)
    src, dst = np.r_[i, 0], np.r_[i + 1, views - 1]
    Rrel = np.einsum("eij,ekj->eik", Rgt[dst], Rgt[src])
    w = np.r_[np.linspace(1.0, 0.9, views - 1), 0.5]
    R0 = forest_rotations(forest(views, src[:-1], dst[:-1], w[:-1]), Rrel[:-1], LD)
    axis = np.asarray(axis, LD)
    plant = _rodrigues_ld(LD(angle) * axis / np.sqrt((axis * axis).sum()))
    Rrel[-1] = (R0[views - 1] @ plant @ R0[0].T).astype(np.float64)
    if zero_chord:
        src, dst, w = np.r_[src, 0], np.r_[dst, views - 2], np.r_[w, 0.0]
        Rrel = np.concatenate([Rrel, Rotation.random(1, random_state=seed + 5).as_matrix()])
    return _graph(views, src, dst, Rrel, w)


# ---- initialisation ----------------------------------------------------------------------------------------------------
def forest(V, src, dst, weight):
    """Maximum-weight spanning forest, Kruskal over (weight desc, index asc), rooted at the smallest view of every component
    (rotavg_oracle.spanning_forest_init without the rotations).  -> dict: roots, parent, pedge, pinv (the tree edge is
    stored child -> parent, i.e. the parent is its dst), order (the non-root views, parents before children), depth."""
    order = sorted(range(len(src)), key=lambda e: (-weight[e], e))
    uf = list(range(V))

    def find(a):
        while uf[a] != a:
            uf[a] = uf[uf[a]]
            a = uf[a]
        return a
    adj = [[] for _ in range(V)]
    for e in order:
        a, b = find(src[e]), find(dst[e])
        if a != b:
            uf[max(a, b)] = min(a, b)
            adj[src[e]].append((int(dst[e]), e, False))
            adj[dst[e]].append((int(src[e]), e, True))
    parent, pedge, pinv = -np.ones(V, int), -np.ones(V, int), np.zeros(V, bool)
    depth, seen, roots, walk = np.zeros(V, int), np.zeros(V, bool), [], []
    for r in range(V):
        if seen[r]:
            continue
        roots.append(r)
        seen[r] = True
        queue = [r]
        while queue:
            nxt = []
            for u in queue:
                for v, e, inv in sorted(adj[u], key=lambda t: t[1]):
                    if seen[v]:
                        continue
                    seen[v] = True
                    parent[v], pedge[v], pinv[v], depth[v] = u, e, inv, depth[u] + 1
                    walk.append(v)
                    nxt.append(v)
            queue = nxt
    return dict(V=V, roots=np.array(roots), parent=parent, pedge=pedge, pinv=pinv, order=np.array(walk, int), depth=depth)


def forest_rotations(F, Rrel, dtype=LD):
    """R_root = I, R_v = R_uv R_u (u the parent; the transposed relative rotation where the edge runs v -> u), in `dtype`."""
    R = np.tile(np.eye(3, dtype=dtype), (F["V"], 1, 1))
    Rrel = np.asarray(Rrel).astype(dtype)
    for v in F["order"]:
        M = Rrel[F["pedge"][v]]
        R[v] = (M.T if F["pinv"][v] else M) @ R[F["parent"][v]]
    return R


# ---- residual, weights, exponential ------------------------------------------------------------------------------------
def log_so3(D):
    """Rotation vectors of D [E,3,3] through the unit quaternion; the component of the largest magnitude among the four is
    taken from the diagonal, the others from the off-diagonal sums and differences.  In the dtype of D."""
    D = np.asarray(D)
    E = len(D)
    c = np.stack([1 + D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2], 1 + D[:, 0, 0] - D[:, 1, 1] - D[:, 2, 2],
                  1 - D[:, 0, 0] + D[:, 1, 1] - D[:, 2, 2], 1 - D[:, 0, 0] - D[:, 1, 1] + D[:, 2, 2]], 1)
    j = np.argmax(c, 1)
    s = 2 * np.sqrt(c[np.arange(E), j])
    a = np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1)   # 4 q0 (q1, q2, q3)
    b = np.stack([D[:, 0, 1] + D[:, 1, 0], D[:, 0, 2] + D[:, 2, 0], D[:, 1, 2] + D[:, 2, 1]], 1)   # 4 q1q2, 4 q1q3, 4 q2q3
    q = np.zeros((E, 4), D.dtype)
    cols = {0: (None, a[:, 0], a[:, 1], a[:, 2]), 1: (a[:, 0], None, b[:, 0], b[:, 1]), 2: (a[:, 1], b[:, 0], None, b[:, 2]),
            3: (a[:, 2], b[:, 1], b[:, 2], None)}
    for jj, parts in cols.items():
        m = j == jj
        for i, v in enumerate(parts):
            q[m, i] = (s[m] / 4) if v is None else v[m] / s[m]
    q[q[:, 0] < 0] *= -1
    nv = np.sqrt((q[:, 1:] ** 2).sum(1))
    k = np.where(nv > 0, 2 * np.arctan2(nv, q[:, 0]) / np.where(nv > 0, nv, 1), 2)
    return k[:, None] * q[:, 1:]


def exp_so3(x):
    """Rodrigues in the dtype of x [V,3] (series below 1e-8, far under the switch of the kernel's float64 formula)."""
    x = np.asarray(x)
    t2 = (x * x).sum(1)
    t = np.sqrt(t2)
    small = t < 1e-8
    ts = np.where(small, 1, t)
    a = np.where(small, 1 - t2 / 6, np.sin(ts) / ts)
    b = np.where(small, 0.5 - t2 / 24, (1 - np.cos(ts)) / (ts * ts))
    K = np.zeros((len(x), 3, 3), x.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -x[:, 2], x[:, 1], x[:, 2], -x[:, 0], -x[:, 1], x[:, 0]
    return np.eye(3, dtype=x.dtype) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def residual_and_weights(g, R, phase, dtype=LD):
    """-> (omega [E,3], w [E]) at the rotations R: phase "l1": weight / max(|omega|, 1e-4); "irls": Geman-McClure,
    weight sigma^2 / (|omega|^2 + sigma^2)^2 sigma^2 (the oracle's docstring)."""
    R = np.asarray(R).astype(dtype)
    D = np.einsum("eji,ejk,ekl->eil", R[g["dst"]], g["Rrel"].astype(dtype), R[g["src"]])
    om = log_so3(D)
    n2 = (om * om).sum(1)
    wt = g["w"].astype(dtype)
    if phase == "l1":
        return om, wt / np.maximum(np.sqrt(n2), dtype(1e-4))
    s2 = dtype(SIGMA) * dtype(SIGMA)
    return om, wt * s2 * s2 / ((n2 + s2) * (n2 + s2))


# ---- the system and the PCG --------------------------------------------------------------------------------------------
def _scatter(V, idx, vals):
    y = np.zeros((V,) + vals.shape[1:], vals.dtype)
    np.add.at(y, idx, vals)
    return y


class System:
    """The grounded weighted Laplacian (x) I3: minimise sum_e w_e |d_dst - d_src - omega_e|^2 with d_root = 0.  Vectors are
    [V, 3] with zeros in the root rows; the three columns are three independent systems."""

    def __init__(self, V, src, dst, w, omega, roots):
        self.V, self.src, self.dst, self.w = V, np.asarray(src, int), np.asarray(dst, int), w
        self.free = np.ones(V, bool)
        self.free[roots] = False
        self.d = _scatter(V, self.src, w) + _scatter(V, self.dst, w)
        self.d[~self.free] = 0
        t = w[:, None] * omega
        self.b = _scatter(V, self.dst, t) - _scatter(V, self.src, t)
        self.b[~self.free] = 0

    def matvec(self, p):
        t = self.w[:, None] * (p[self.dst] - p[self.src])
        y = _scatter(self.V, self.dst, t) - _scatter(self.V, self.src, t)
        y[~self.free] = 0
        return y

    def jacobi(self):
        inv = np.where(self.d > 0, 1 / np.where(self.d > 0, self.d, 1), 0)
        return lambda r: r * inv[:, None]

    def tree(self, F):
        """z = L_T^-1 r, L_T the Laplacian of the forest F with the CURRENT weights, grounded at the roots: the flow on the
        edge above v is the sum of r over the subtree of v (leaves to roots), z_v = z_parent + flow_v / w_v (roots to leaves)."""
        order, parent, wp = F["order"], F["parent"], self.w[F["pedge"]]

        def apply(r):
            f = r.copy()
            for v in order[::-1]:
                f[parent[v]] += f[v]
            z = np.zeros_like(r)
            for v in order:
                z[v] = z[parent[v]] + (f[v] / wp[v] if wp[v] > 0 else 0)
            return z
        return apply

    def coarse(self, agg):
        """Ac = P^T A P, P the indicator of the aggregates agg [V] (-1: a gauge view)."""
        n = int(agg.max()) + 1
        Ac = np.zeros((n, n), self.w.dtype)
        np.add.at(Ac, (agg[self.free], agg[self.free]), self.d[self.free])
        both = self.free[self.src] & self.free[self.dst]
        a, b, w = agg[self.src[both]], agg[self.dst[both]], self.w[both]
        np.add.at(Ac, (a, b), -w)
        np.add.at(Ac, (b, a), -w)
        return Ac

    def two_level(self, agg):
        """M^-1 = D^-1 + P Ac^-1 P^T."""
        jac, Ainv, fr = self.jacobi(), ld_inverse(self.coarse(agg)), self.free

        def apply(r):
            z = jac(r)
            z[fr] += (Ainv @ _scatter(len(Ainv), agg[fr], r[fr]))[agg[fr]]
            return z
        return apply

    def direct(self):
        """The solution of the three systems: sparse LU in float64, refined with longdouble residuals."""
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        idx = -np.ones(self.V, int)
        idx[self.free] = np.arange(self.free.sum())
        both = self.free[self.src] & self.free[self.dst]
        i, j, w = idx[self.src[both]], idx[self.dst[both]], self.w[both].astype(float)
        n = int(self.free.sum())
        A = sp.csc_matrix((np.r_[self.d[self.free].astype(float), -w, -w], (np.r_[np.arange(n), i, j], np.r_[np.arange(n), j, i])), shape=(n, n))
        lu = spla.splu(A)
        x = np.zeros_like(self.b)
        for _ in range(6):
            r = self.b - self.matvec(x)
            x[self.free] += lu.solve(r[self.free].astype(float))
        return x


def ld_inverse(A):
    """Inverse by Gauss-Jordan with partial pivoting in the dtype of A (numpy.linalg stops at float64)."""
    n = len(A)
    M = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        col = M[:, k].copy()
        col[k] = 0
        M -= col[:, None] * M[k][None, :]
    return M[:, n:]


def pcg(S, n, precond, tol=FIXED_STEP_TOL, record=None):
    """Textbook PCG on the three axes from x = 0, at most n iterations; an axis stops BEFORE an iteration when not
    (rz > tol^2 rz0) -- the kernels' rule.  -> (x [V,3], iterations run per axis [3]).  record: a dict; record[k] receives
    (x, iterations run) after k iterations for every key k already in it."""
    dt = S.b.dtype.type
    x = np.zeros_like(S.b)
    r = S.b.copy()
    z = precond(r)
    p = z.copy()
    rz = (r * z).sum(0)
    rz0 = rz.copy()
    ran = np.zeros(3, int)
    tol2 = dt(tol) * dt(tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(n):
            act = rz > tol2 * rz0
            if not act.any():
                break
            q = S.matvec(p)
            pq = (p * q).sum(0)
            alpha = np.where(act & (pq > 0), rz / np.where(pq > 0, pq, 1), 0)
            x += alpha * p
            r -= alpha * q
            z = precond(r)
            rzn = (r * z).sum(0)
            beta = np.where(rz > 0, rzn / np.where(rz > 0, rz, 1), 0)
            p = np.where(act, z + beta * p, p)
            rz = np.where(act, rzn, rz)
            ran += act
            if record is not None and it + 1 in record:
                record[it + 1] = (x.copy(), ran.copy())
    return x, ran


# ---- the aggregates of the two-level preconditioner ----------------------------------------------------------------------
def incidence_lists(V, src, dst):
    """Per view the other ends of its incidences in CSR order (edge order; an edge enters the lists of both its views)."""
    nb = [[] for _ in range(V)]
    for s, d in zip(src, dst):
        nb[s].append(int(d))
        nb[d].append(int(s))
    return nb


def aggregates(V, src, dst, roots, info=None):
    """The region-growing rule plan_two_level documents.  -> agg [V] (aggregate of every free view, -1 for the gauge views),
    or None when more than 127 aggregates remain.  info: a dict that receives target, grown (aggregates before merging)."""
    nb = incidence_lists(V, src, dst)
    is_root = np.zeros(V, bool)
    is_root[roots] = True
    n_free = int((~is_root).sum())
    if n_free == 0:
        return None
    seen = is_root.copy()                      # 1. breadth-first order from the gauge views
    order = [int(v) for v in np.nonzero(is_root)[0]]
    h = 0
    while h < len(order):
        for o in nb[order[h]]:
            if not seen[o]:
                seen[o] = True
                order.append(o)
        h += 1
    target = max(32, -(-n_free // 112))        # 2.
    target = -(-target // 16) * 16
    for attempt in range(6):
        agg = -np.ones(V, int)
        size, members = [], []
        for seed in order:                     # 3. the first `target` unassigned views a breadth-first walk reaches
            if is_root[seed] or agg[seed] >= 0:
                continue
            gid = len(size)
            disc = [seed]
            agg[seed] = gid
            h = 0
            while h < len(disc) and len(disc) < target:
                for o in nb[disc[h]]:
                    if len(disc) >= target:
                        break
                    if is_root[o] or agg[o] >= 0:
                        continue
                    agg[o] = gid
                    disc.append(o)
                h += 1
            size.append(len(disc))
            members.append(disc)
        into = list(range(len(size)))

        def label(a):
            while into[a] != a:
                a = into[a]
            return a
        grown = len(size)
        for gid in range(grown):               # 4. a left-over below target / 2 joins its smallest neighbour (ties: lower id)
            if size[gid] >= target // 2:
                continue
            best = None
            for v in members[gid]:
                for o in nb[v]:
                    if is_root[o]:
                        continue
                    hh = label(agg[o])
                    if hh == gid:
                        continue
                    if best is None or (size[hh], hh) < (size[best], best):
                        best = hh
            if best is None:
                continue                       # a component of its own
            into[gid] = best
            size[best] += size[gid]
        final = {}
        for gid in range(grown):
            if into[gid] == gid:
                final[gid] = len(final)
        if len(final) <= 127:
            if info is not None:
                info.update(target=target, grown=grown)
            out = -np.ones(V, int)
            for v in np.nonzero(agg >= 0)[0]:
                out[v] = final[label(agg[v])]
            return out
        if attempt == 5 or target >= n_free:   # 5. the target doubles, at most five times
            return None
        target *= 2
    return None


# ---- one step, several steps, the converged step ------------------------------------------------------------------------
def _setup(g, dtype=LD):
    F = forest(g["V"], g["src"], g["dst"], g["w"])
    return F, forest_rotations(F, g["Rrel"], dtype)


def _preconditioner(S, g, F, path):
    if path == "jacobi":
        return S.jacobi()
    if path == "tree":
        return S.tree(F)
    assert path == "two"
    return S.two_level(aggregates(g["V"], g["src"], g["dst"], F["roots"]))


def step_rotations(g, phase, counts, path):
    """The first outer step with n PCG iterations for every n in counts: -> (R0, {n: (x_n, R0 exp(x_n), iterations run per
    axis)}), longdouble."""
    F, R0 = _setup(g)
    om, w = residual_and_weights(g, R0, phase)
    S = System(g["V"], g["src"], g["dst"], w, om, F["roots"])
    record = {n: None for n in counts}
    x, ran = pcg(S, max(counts), _preconditioner(S, g, F, path), record=record)
    out = {}
    for n in counts:
        xn, rn = record[n] if record[n] is not None else (x, ran)
        out[n] = (xn, R0 @ exp_so3(xn), rn)
    return R0, out


def converged_step(g, phase):
    """The first outer step solved directly: -> (R0, x, R0 exp(x))."""
    F, R0 = _setup(g)
    om, w = residual_and_weights(g, R0, phase)
    x = System(g["V"], g["src"], g["dst"], w, om, F["roots"]).direct()
    return R0, x, R0 @ exp_so3(x)


def trajectory(g, path, l1_iters, irls_iters, cg_iters):
    """l1_iters + irls_iters outer iterations of cg_iters PCG steps each.  -> (R0, R, the largest |x_k| of all steps,
    iterations run per outer iteration)."""
    F, R0 = _setup(g)
    R, ran, scale = R0, [], 0.0
    for it in range(l1_iters + irls_iters):
        om, w = residual_and_weights(g, R, "l1" if it < l1_iters else "irls")
        S = System(g["V"], g["src"], g["dst"], w, om, F["roots"])
        x, rn = pcg(S, cg_iters, _preconditioner(S, g, F, path))
        ran.append(rn)
        scale = max(scale, step_scale(x))
        R = R @ exp_so3(x)
    return R0, R, scale, ran


def step_scale(x):
    return float(np.sqrt((np.asarray(x, LD) ** 2).sum(1)).max())


def distance(R, R_ref, x):
    """max_k |R_k - R_ref,k|_max / max_k |x_k|: relative to the step (x: the step [V,3], or that scale itself), no gauge
    alignment."""
    return float(np.abs(np.asarray(R, LD) - R_ref).max()) / (x if isinstance(x, float) else step_scale(x))


# ---- the float64 leg that follows the kernels' formulas (for scripts/rotavg_roundoff.py) --------------------------------
def mirror_log(D):
    """so3_log: Shepperd's branches in the kernel's order."""
    tr = D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2]
    b0 = tr > 0.0
    b1 = ~b0 & (D[:, 0, 0] > D[:, 1, 1]) & (D[:, 0, 0] > D[:, 2, 2])
    b2 = ~b0 & ~b1 & (D[:, 1, 1] > D[:, 2, 2])
    b3 = ~b0 & ~b1 & ~b2
    q = np.zeros((len(D), 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(tr + 1.0) * 2.0
        q[b0] = np.stack([0.25 * s, (D[:, 2, 1] - D[:, 1, 2]) / s, (D[:, 0, 2] - D[:, 2, 0]) / s, (D[:, 1, 0] - D[:, 0, 1]) / s], 1)[b0]
        s = np.sqrt(1.0 + D[:, 0, 0] - D[:, 1, 1] - D[:, 2, 2]) * 2.0
        q[b1] = np.stack([(D[:, 2, 1] - D[:, 1, 2]) / s, 0.25 * s, (D[:, 0, 1] + D[:, 1, 0]) / s, (D[:, 0, 2] + D[:, 2, 0]) / s], 1)[b1]
        s = np.sqrt(1.0 + D[:, 1, 1] - D[:, 0, 0] - D[:, 2, 2]) * 2.0
        q[b2] = np.stack([(D[:, 0, 2] - D[:, 2, 0]) / s, (D[:, 0, 1] + D[:, 1, 0]) / s, 0.25 * s, (D[:, 1, 2] + D[:, 2, 1]) / s], 1)[b2]
        s = np.sqrt(1.0 + D[:, 2, 2] - D[:, 0, 0] - D[:, 1, 1]) * 2.0
        q[b3] = np.stack([(D[:, 1, 0] - D[:, 0, 1]) / s, (D[:, 0, 2] + D[:, 2, 0]) / s, (D[:, 1, 2] + D[:, 2, 1]) / s, 0.25 * s], 1)[b3]
    q[q[:, 0] < 0.0] *= -1.0
    nv = np.sqrt(q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    k = np.where(nv < 1e-12, 2.0, 2.0 * np.arctan2(nv, q[:, 0]) / np.where(nv < 1e-12, 1.0, nv))
    return k[:, None] * q[:, 1:], np.stack([b0, b1, b2, b3], 1)


def mirror_exp(x):
    """so3_exp: the series below 1e-6."""
    t2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
    t = np.sqrt(t2)
    small = t < 1e-6
    ts, t2s = np.where(small, 1.0, t), np.where(small, 1.0, t2)
    a = np.where(small, 1.0 - t2 / 6.0, np.sin(ts) / ts)
    b = np.where(small, 0.5 - t2 / 24.0, (1.0 - np.cos(ts)) / t2s)
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    R = np.empty((len(x), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1.0 - b * (Y * Y + Z * Z), -a * Z + b * X * Y, a * Y + b * X * Z
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = a * Z + b * X * Y, 1.0 - b * (X * X + Z * Z), -a * X + b * Y * Z
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -a * Y + b * X * Z, a * X + b * Y * Z, 1.0 - b * (X * X + Y * Y)
    return R


def _mirror_tree_plan(F):
    """Depth-first preorder of the forest, subtree sizes and Euler-tour positions (as rotavg_solve builds them)."""
    V = F["V"]
    kids = [[] for _ in range(V)]
    for v in F["order"]:
        kids[F["parent"][v]].append(int(v))
    n2o, size, enter, leave, o2n, clock = [], np.ones(V, int), np.zeros(V, int), np.zeros(V, int), -np.ones(V, int), 0
    for root in F["roots"]:
        stack = [(int(root), 0)]
        o2n[root] = len(n2o); n2o.append(int(root)); enter[o2n[root]] = clock; clock += 1
        while stack:
            v, i = stack.pop()
            if i < len(kids[v]):
                stack.append((v, i + 1))
                c = kids[v][i]
                o2n[c] = len(n2o); n2o.append(c); enter[o2n[c]] = clock; clock += 1
                stack.append((c, 0))
            else:
                k = o2n[v]
                size[k] = len(n2o) - k
                leave[k] = clock; clock += 1
    return np.array(n2o), size, enter, leave


def mirror_solve(g, F, om, w, n, path, tol, perm=None, cg_form=False, agg=None):
    """One inner solve in float64 as the kernels write it: per-view sums over the incidences in edge order (or in the order
    `perm` ranks the edges), the plain recurrences (rot_solve_kernel, rot_solve_tree_kernel) or the Chronopoulos-Gear form
    with the neighbours' z rebuilt from the previous vectors (cg_iteration_kernel, one- and two-level); the tree solve by
    the two prefix sums; Ac^-1 by Gauss-Jordan without pivoting, symmetrised.  -> (x [V,3], iterations run per axis)."""
    V, src, dst = g["V"], g["src"], g["dst"]
    E = len(src)
    rank = np.arange(E) if perm is None else np.argsort(perm)
    view, other = np.r_[src, dst], np.r_[dst, src]
    edge, sign = np.r_[np.arange(E), np.arange(E)], np.r_[-np.ones(E), np.ones(E)]
    o = np.lexsort((rank[edge], view))
    view, other, edge, sign = view[o], other[o], edge[o], sign[o]
    free = np.ones(V, bool)
    free[F["roots"]] = False
    keep = free[view]
    view, other, edge, sign = view[keep], other[keep], edge[keep], sign[keep]
    we = w[edge]
    d = _scatter(V, view, we)
    b = _scatter(V, view, (sign * we)[:, None] * om[edge])
    inv = np.where(d > 0.0, 1.0 / np.where(d > 0.0, d, 1.0), 0.0)[:, None]
    fo = free[other]                         # incidences whose other end is free
    vf, of, wf = view[fo], other[fo], we[fo][:, None]

    def offdiag(t):                          # sum over the incidences of -w t_other
        return _scatter(V, vf, -(wf * t[of]))
    coarse = None
    if path == "two":
        NA = int(agg.max()) + 1
        Ac = np.zeros((NA, NA))
        np.add.at(Ac, (agg[free], agg[free]), d[free])
        np.add.at(Ac, (agg[vf], agg[of]), -wf[:, 0])
        M = Ac.copy()
        for k in range(NA):                  # cg2_coarse_invert_kernel's rule per entry
            piv = M[k, k]
            pinv = 1.0 / piv
            c, r = M[:, k].copy(), M[k] * pinv
            M = M - c[:, None] * r[None, :]
            M[k], M[:, k], M[k, k] = r, -c * pinv, pinv
        Ainv = 0.5 * (M + M.T)
        ag = np.where(free, agg, 0)

        def coarse(rho):
            return np.where(free[:, None], (Ainv.T @ rho)[ag], 0.0)

        def restrict(t):
            return _scatter(NA, agg[free], t[free])
    if path == "tree":
        n2o, size, enter, leave = _mirror_tree_plan(F)
        pe = F["pedge"][n2o]
        winv = np.where(pe >= 0, 1.0 / np.where(pe >= 0, w[pe], 1.0), 0.0)[:, None]
        k = np.arange(V)

        def precond(r):
            S = np.cumsum(r[n2o], 0)
            f = S[k + size - 1] - np.where((k > 0)[:, None], S[np.maximum(k - 1, 0)], 0.0)
            gg = f * winv
            tour = np.zeros((2 * V, 3))
            tour[enter], tour[leave] = gg, -gg
            T = np.cumsum(tour, 0)
            z = np.zeros_like(r)
            z[n2o] = np.where((pe >= 0)[:, None], T[enter], 0.0)
            return z
    elif path == "two":
        def precond(r):
            return r * inv + coarse(restrict(r))
    else:
        def precond(r):
            return r * inv
    tol2 = tol * tol
    ran = np.zeros(3, int)
    x = np.zeros((V, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        if not cg_form:
            r = b.copy()
            z = precond(r)
            p = z.copy()
            rz = (r * z).sum(0)
            rz0 = rz.copy()
            for _ in range(n):
                act = rz > tol2 * rz0
                if not act.any():
                    break
                q = d[:, None] * p + offdiag(p)
                pq = (p * q).sum(0)
                alpha = np.where(act & (pq > 0.0), rz / pq, 0.0)
                x += alpha * p
                r -= alpha * q
                z = precond(r)
                rzn = (r * z).sum(0)
                beta = np.where(rz > 0.0, rzn / rz, 0.0)
                p = np.where(act, z + beta * p, p)
                rz = np.where(act, rzn, rz)
                ran += act
            return x, ran
        # Chronopoulos-Gear: launch 0 is the init pass (alpha = beta = 0)
        r = b.copy()
        p, q, s = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
        alpha, beta = np.zeros(3), np.zeros(3)
        rho = restrict(r) if coarse else None
        kap = np.zeros_like(rho) if coarse else None
        c_old = coarse(rho) if coarse else 0.0
        rz = rz0 = a_prev = None
        for launch in range(n + 1):
            if launch == 1:
                rz0 = gam.copy()
                alpha, beta = np.where(dl > 0.0, gam / dl, 0.0), np.zeros(3)
                if not (gam > 0.0).any():
                    break
            elif launch > 1:
                if not (gam > tol2 * rz0).any():
                    break
                bt = np.where(rz > 0.0, gam / rz, 0.0)
                den = np.where(a_prev != 0.0, dl - bt * gam / a_prev, dl)
                alpha, beta = np.where(den > 0.0, gam / den, 0.0), bt
            if launch >= 1:
                rz, a_prev = gam, alpha
            if coarse:
                if launch:
                    kap = restrict(s) + beta * kap
                    rho = rho - alpha * kap
                c_new = coarse(rho)
            else:
                c_new = 0.0
            qn = s + beta * q
            rn = r - alpha * qn
            zn = rn * inv + c_new                          # every view rebuilds the z of its neighbours like this
            zn = np.where(free[:, None], zn, 0.0)
            zo = np.where(free[:, None], r * inv + c_old, 0.0)
            p = zo + beta * p
            x += alpha * p
            sn = d[:, None] * zn + offdiag(zn)
            sn = np.where(free[:, None], sn, 0.0)
            gam, dl = (rn * zn).sum(0), (zn * sn).sum(0)
            r, q, s, c_old = rn, qn, sn, c_new
            if launch:
                ran += 1
        return x, ran


def mirror_rotations(g, phases, n, path, tol=FIXED_STEP_TOL, perm=None, cg_form=False):
    """The device's data path in float64: initialisation, then for every entry of phases ("l1" / "irls") residuals, weights,
    one inner solve of at most n iterations and the update.  -> (R0, R, x of the last step, iterations per outer step)."""
    F, R0 = _setup(g, np.float64)
    agg = aggregates(g["V"], g["src"], g["dst"], F["roots"]) if path == "two" else None
    R, x, ran = R0, None, []
    for phase in phases:
        T = np.einsum("eij,ejk->eik", g["Rrel"], R[g["src"]])
        om, _ = mirror_log(np.einsum("eji,ejk->eik", R[g["dst"]], T))
        n2 = om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1] + om[:, 2] * om[:, 2]
        if phase == "l1":
            w = g["w"] / np.maximum(np.sqrt(n2), 1e-4)
        else:
            s2 = SIGMA * SIGMA
            dd = n2 + s2
            w = g["w"] * s2 / (dd * dd) * s2
        x, rn = mirror_solve(g, F, om, w, n, path, tol, perm, cg_form, agg)
        ran.append(rn)
        R = R @ mirror_exp(x)
    return R0, R, x, ran


# ---- the cases of tests/test_rotavg_steps.py (shared with scripts/rotavg_roundoff.py) ------------------------------------
PHASES = ("l1", "irls")
PHASE_KW = {"l1": dict(l1_iters=1, irls_iters=0), "irls": dict(l1_iters=0, irls_iters=1)}


def one_wg_graphs():
    """rot_solve_kernel (E > 8 V everywhere): row_lanes 16 up to V = 64, then 8, 8, 4, 2, 2, 1; V = 1030 makes two passes."""
    out = {"V%d" % V: dense_multigraph(V, seed=V) for V in (2, 3, 20, 64)}
    for V in (65, 128, 129, 257, 300, 513, 1030):
        out["V%d" % V] = random_graph(V, 10, seed=V)
    out["components"] = join([dense_multigraph(24, seed=1), dense_multigraph(30, seed=2)], isolated=1)
    return out


def many_wg_graphs():
    """cg_init_kernel / cg_iteration_kernel (PGI_ROTAVG_SINGLE_WG_VIEWS = 0), 16 views per block; V = 4112: 257 blocks."""
    one = one_wg_graphs()
    out = {"V%d" % V: dense_multigraph(V, seed=V) for V in (2, 15, 16, 17)}
    out.update({k: one[k] for k in ("V20", "V64", "V300")})
    out["V4112"] = random_graph(4112, 9, seed=4112)
    out["hub"] = hub_graph(300, 77, 260, seed=5)
    out["components"] = random_graph(300, 10, seed=6, components=2)
    return out


SHARED_ONE_MANY = ("V20", "V64", "V300")


def tree_graphs():
    """rot_solve_tree_kernel (E <= 8 V, V <= 6144)."""
    return {"ring65": ring_graph(65, seed=65), "path1024": path_with_closures(1024, seed=1024), "path1025": path_with_closures(1025, seed=1025),
            "seq6144": seq_graph(6144, 3, seed=13, noise_deg=TREE_NOISE_DEG), "star": star_with_chords(150, seed=7), "path200": path_with_closures(200, seed=8),
            "components": join([seq_graph(90, 3, seed=9, noise_deg=TREE_NOISE_DEG), path_with_closures(70, seed=10)], isolated=1)}


def two_level_graphs():
    """cg_*_kernel<true>, cg2_coarse_* (PGI_ROTAVG_TWO_LEVEL = 2)."""
    return {"V20": dense_multigraph(20, seed=20), "V100": random_graph(100, 10, seed=100), "band700": seq_graph(700, 12, seed=17),
            "merge": seq_graph(105, 4, seed=18), "components": random_graph(200, 10, seed=19, components=2)}


def no_plan_graph():
    """130 components of three views: more aggregates than the coarse space takes, whatever the target."""
    return seq_graph(390, 2, seed=21, components=130)


DEG = np.pi / 180.0
NEAR_PI = np.pi - 0.06 * DEG
# name -> (angle, axis): the chord's residual at the initialisation
PLANTED = {
    "1e-9": (1e-9, (1, 2, 3)), "1e-5": (1e-5, (1, 2, 3)), "3e-4": (3e-4, (3, 1, 2)),
    "1deg": (1 * DEG, (2, 3, 1)), "90deg": (90 * DEG, (1, -2, 2)), "119deg": (119 * DEG, (1, 1, -1)), "179deg": (179 * DEG, (2, 1, 3)),
    "pi-x": (NEAR_PI, (5, 1, 2)), "pi-y": (NEAR_PI, (1, 5, -2)), "pi-z": (NEAR_PI, (2, -1, 5)),
    "pi-x-negative-q0": (NEAR_PI, (-5, 2, 1)), "pi-z-negative-q0": (NEAR_PI, (1, 2, -5)),
}
PLANTED_TINY = ("1e-9", "1e-5")          # steps of the size of float64's resolution of a rotation matrix: a family of their own


def planted_graphs():
    out = {k: planted_graph(a, ax, views=3 + i % 4, seed=30 + i) for i, (k, (a, ax)) in enumerate(PLANTED.items())}
    out["zero-weight-chord"] = planted_graph(20 * DEG, (1, 2, -3), views=6, seed=50, zero_chord=True)
    return out


def trajectory_graphs():
    return {"one": ("jacobi", one_wg_graphs()["V64"]), "many": ("jacobi", one_wg_graphs()["V300"]),
            "tree": ("tree", tree_graphs()["path200"]), "two": ("two", two_level_graphs()["V100"])}


def converged_graphs():
    """The converged one-step regime: (path, graph)."""
    t, two = tree_graphs(), two_level_graphs()
    return {"tree-ring65": ("tree", t["ring65"]), "tree-path200": ("tree", t["path200"]), "tree-components": ("tree", t["components"]),
            "two-V100": ("two", two["V100"]), "two-band700": ("two", two["band700"])}
