"""transavg_spec.py -- CPU SPECIFICATION of translation averaging (test infrastructure, NOT product code).

The reference contains no translation averaging; like oracle/rotavg_oracle.py this file restates a published
method -- robust Least Unsquared Deviations (Ozyesil & Singer, "Robust Camera Location Estimation by Convex
Programming", CVPR 2015) solved by joint IRLS with an active set -- with INDEPENDENT arithmetic: numpy and a
sparse direct solve (the HIP path, csrc/pgi_transavg.hip, runs a block-Jacobi preconditioned CG).

Conventions: an edge (src=i, dst=j) has x_j = R_ij x_i + t_ij with world->camera rotations R_k, so the world
direction of c_i - c_j is gamma_e = R_j^T t_ij (unit).  The problem is
    min  sum_e w_e |c_i - c_j - s_e gamma_e|   subject to  s_e >= 1,   one gauge view per component at 0.
Eliminating s_e: with D = c_src - c_dst and a = <D, gamma> an edge costs |D - gamma| where a <= 1 (CLAMPED)
and |(I - gamma gamma^T) D| otherwise (FREE).

Specification of one run (mirrored by the device solver):
 1. init: maximum-weight spanning forest (Kruskal over edges sorted by (weight desc, index asc)), BFS from the
    smallest vertex id of each component, c_root = 0, along a tree edge c_dst = c_src - gamma_e (walked
    backwards: c_src = c_dst + gamma_e).
 2. outer iteration, from the current c: a_e = <D, gamma>, clamped iff a_e <= 1;
    residual r_e = |D - gamma| (clamped) or |D - a_e gamma| (free); weight omega_e = w_e / max(r_e, delta);
    model M_e = (I - gamma gamma^T) + lambda_e gamma gamma^T with lambda_e = 1, tau_e = 1 (clamped) or
    lambda_e = eps, tau_e = a_e (free).  The eps term is a proximal term on the length along gamma: it keeps
    the system non-singular when few edges are clamped and vanishes at a fixed point.
 3. solve: minimise sum_e omega_e (D^T M_e D - 2 lambda_e tau_e gamma_e^T D) with the roots fixed at 0 -- a
    3V x 3V block Laplacian with 3 x 3 SPD blocks.
 4. c <- solution; stop when the mean |c_new - c_old| over the views is below tol or after `iters` iterations.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def spanning_forest_init(n_views, src, dst, gamma, weight):
    """-> (c0 [V,3], roots).  Same forest and roots as oracle/rotavg_oracle.py:spanning_forest_init."""
    order = sorted(range(len(src)), key=lambda e: (-weight[e], e))
    parent = list(range(n_views))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    adj = [[] for _ in range(n_views)]
    for e in order:
        a, b = find(src[e]), find(dst[e])
        if a != b:
            parent[max(a, b)] = min(a, b)
            adj[src[e]].append((dst[e], e, False))
            adj[dst[e]].append((src[e], e, True))
    c = np.zeros((n_views, 3))
    seen = np.zeros(n_views, bool)
    roots = []
    for r in range(n_views):
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
                    # forward edge (u = src, v = dst): c_dst = c_src - gamma; reversed: c_src = c_dst + gamma
                    c[v] = c[u] + gamma[e] if inv else c[u] - gamma[e]
                    nxt.append(v)
            queue = nxt
    return c, np.array(roots, int)


def edge_model(c, src, dst, gamma, weight, eps, delta):
    """Step 2 -> (omega M_e [E,3,3], omega lambda tau gamma [E,3], clamped [E] bool)."""
    D = c[src] - c[dst]
    # The class test is exact arithmetic's business on the FIRST iteration: a tree edge of the initialisation has
    # D = -+gamma exactly, so a = |gamma|^2 = 1 to the last bit and its rounding decides the class.  Hence single IEEE
    # operations in a fixed order (no einsum), which the device kernel reproduces.
    a = (D[:, 0] * gamma[:, 0] + D[:, 1] * gamma[:, 1]) + D[:, 2] * gamma[:, 2]
    clamped = a <= 1.0
    tau = np.where(clamped, 1.0, a)
    lam = np.where(clamped, 1.0, eps)
    r = np.linalg.norm(D - tau[:, None] * gamma, axis=1)
    om = weight / np.maximum(r, delta)
    gg = gamma[:, :, None] * gamma[:, None, :]
    M = np.eye(3)[None] - gg + lam[:, None, None] * gg
    return om[:, None, None] * M, (om * lam * tau)[:, None] * gamma, clamped


def assemble(n_views, src, dst, P, g, free):
    """The block Laplacian restricted to the free views and its right-hand side."""
    E = len(src)
    i3 = np.arange(3)
    rows, cols, vals = [], [], []
    for (u, v, sg) in ((src, src, 1.0), (dst, dst, 1.0), (src, dst, -1.0), (dst, src, -1.0)):
        rows.append((3 * u[:, None, None] + i3[None, :, None]) + np.zeros((E, 3, 3), int))
        cols.append((3 * v[:, None, None] + i3[None, None, :]) + np.zeros((E, 3, 3), int))
        vals.append(sg * P)
    A = sp.csr_matrix((np.concatenate(vals).ravel(), (np.concatenate(rows).ravel(), np.concatenate(cols).ravel())),
                      shape=(3 * n_views, 3 * n_views))
    b = np.zeros((n_views, 3))
    np.add.at(b, src, g)
    np.add.at(b, dst, -g)
    dof = np.repeat(free, 3)
    return A[dof][:, dof].tocsc(), b.reshape(-1)[dof]


def direct_solve(A, b, x0):
    n = A.shape[0]
    if n <= 4096 and A.nnz * 20 > n * n:  # the factor of a dense view graph fills in anyway: LAPACK is faster
        return np.linalg.solve(A.toarray(), b)
    return spla.spsolve(A, b)


def translation_average(n_views, src, dst, gamma, weight, iters=60, eps=1e-3, delta=1e-4, tol=1e-9, solve=None,
                        trace=None):
    """-> (c [V,3], iters).  solve(A, b, x0) -> x replaces the sparse direct solve (x0 = the current positions of the
    free views, flattened).  trace: a list that receives (clamped edges, mean step) per outer iteration."""
    src, dst = np.asarray(src, int), np.asarray(dst, int)
    gamma = np.asarray(gamma, float).reshape(-1, 3)
    weight = np.asarray(weight, float)
    solve = solve or direct_solve
    c, roots = spanning_forest_init(n_views, src, dst, gamma, weight)
    free = np.ones(n_views, bool)
    free[roots] = False
    done = 0
    if len(src) == 0 or not free.any():
        return c, done
    for it in range(iters):
        P, g, clamped = edge_model(c, src, dst, gamma, weight, eps, delta)
        A, b = assemble(n_views, src, dst, P, g, free)
        new = np.zeros_like(c)
        new[free] = np.asarray(solve(A, b, c[free].reshape(-1))).reshape(-1, 3)
        step = float(np.mean(np.linalg.norm(new - c, axis=1)))
        c = new
        done = it + 1
        if trace is not None:
            trace.append((int(clamped.sum()), step))
        if step < tol:
            break
    return c, done


def directions_from_edges(R_global, src, dst, t_rel):
    """gamma_e = R_dst^T t_e, normalised: the world direction of c_src - c_dst.  Written out as single IEEE
    operations in a fixed order (no einsum, no norm()), so that the device kernel can reproduce the bits."""
    R = np.asarray(R_global, float).reshape(-1, 3, 3)[np.asarray(dst, int)]
    t = np.asarray(t_rel, float).reshape(-1, 3)
    g = np.stack([R[:, 0, i] * t[:, 0] + R[:, 1, i] * t[:, 1] + R[:, 2, i] * t[:, 2] for i in range(3)], 1)
    n = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    return g / n[:, None]


def _rodrigues(w):
    th = np.linalg.norm(w, axis=1)
    k = w / np.maximum(th, 1e-300)[:, None]
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def make_graph(V, k=6, noise_deg=1.0, outlier_frac=0.1, seed=0, components=1):
    """Random view graph (the topology of rotavg_oracle.make_graph) with ground truth:
    -> (src, dst, gamma, weight, c_gt, outlier mask).  Centres ~ N(0, 5^2) per axis."""
    rng = np.random.default_rng(seed)
    c_gt = rng.standard_normal((V, 3)) * 5.0
    comp = np.arange(V) % components
    edges = set()
    for i in range(V):
        same = np.nonzero(comp == comp[i])[0]
        ring = same[(np.searchsorted(same, i) + 1) % len(same)]
        if ring != i:
            edges.add((min(i, ring), max(i, ring)))
        for j in rng.choice(same, size=min(k, len(same)), replace=False):
            if j != i:
                edges.add((min(i, int(j)), max(i, int(j))))
    edges = sorted(edges)
    src = np.array([e[0] for e in edges])
    dst = np.array([e[1] for e in edges])
    flip = rng.random(len(edges)) < 0.5
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    gamma = c_gt[src] - c_gt[dst]
    gamma /= np.linalg.norm(gamma, axis=1, keepdims=True)
    noise = _rodrigues(rng.standard_normal((len(edges), 3)) * np.deg2rad(noise_deg) / np.sqrt(3))
    gamma = np.einsum("eij,ej->ei", noise, gamma)
    out = rng.random(len(edges)) < outlier_frac
    rnd = rng.standard_normal((len(edges), 3))
    gamma[out] = (rnd / np.linalg.norm(rnd, axis=1, keepdims=True))[out]
    weight = np.where(out, rng.uniform(0.1, 0.4, len(edges)), rng.uniform(0.4, 1.0, len(edges)))
    return src, dst, gamma, weight, c_gt, out


def align_error(c, c_gt, labels=None):
    """Per-view position error after a least-squares scale + translation alignment of every component (the world
    axes are fixed by the global rotations, so the gauge has no rotation), relative to the RMS spread of the
    component's ground-truth centres.  labels: component id per view (None: one component)."""
    c, c_gt = np.asarray(c, float), np.asarray(c_gt, float)
    labels = np.zeros(len(c), int) if labels is None else np.asarray(labels)
    err = np.zeros(len(c))
    for lab in np.unique(labels):
        m = labels == lab
        x, y = c[m] - c[m].mean(0), c_gt[m] - c_gt[m].mean(0)
        den = float((x * x).sum())
        s = float((x * y).sum()) / den if den > 0 else 0.0
        spread = np.sqrt((y * y).sum(1).mean())
        err[m] = np.linalg.norm(s * x - y, axis=1) / (spread if spread > 0 else 1.0)
    return err
