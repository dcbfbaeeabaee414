"""bundle_spec.py -- CPU SPECIFICATION of the bundle adjustment (test infrastructure, NOT product code).

States what csrc/pgi_bundle.hip computes: Levenberg-Marquardt with Marquardt damping on the
Huber-weighted pixel reprojection error over poses and points together.  numpy, float64, direct dense solves; a second
solver follows the kernels' formulas (Schur form, adjugate inverses, Schur-Jacobi PCG) in float64 or longdouble.

Participation.  Member m of track t takes part when obs_state[m] == 1, status[t] is OK (or LOW_PARALLAX with
use_low_parallax), X[t] is finite, its view is < V and has a pose and its keypoint exists.  A track with fewer than two such
members does not take part.  A view is FREE when it has a pose, is not marked in `fixed` and has at least min_cam_obs
participating observations (and at least one).  fixed = None: the smallest-index posed view with participating observations
holds the gauge.  The rest of the gauge (scale, frames of further components) is left to the damping, lambda > 0 always.

Model.  d = X - c;  q_i = (R[i][0]*d0 + R[i][1]*d1) + R[i][2]*d2;  DEPTH SIGN: q2 > 0 (one comparison), else the cost is +inf.
    a = q0/q2;  b = q1/q2;  iz = 1/q2;  r0 = (fx*a + cx) - px;  r1 = (fy*b + cy) - py;  e2 = r0*r0 + r1*r1;  e = sqrt(e2)
    HUBER CLASS: e <= huber_px (one comparison) -> w = 1, rho = e2;  else w = huber_px/e, rho = (2*huber_px)*e - huber_px*huber_px
    sx = fx*iz;  sy = fy*iz
    d r / d X     = [sx*(R[0][i] - a*R[2][i]);  sy*(R[1][i] - b*R[2][i])]           (J_p; d r / d c = -J_p)
    d r / d omega = [-(sx*(a*q1)), sx*(q2 + a*q0), -(sx*q1);  -(sy*(q2 + b*q1)), sy*(b*q0), sy*q0]   (J_w = (d r/d q)(-[q]x))
Update.  R <- E R with E = I + A [w]x + B [w]x^2, th2 = (w0*w0 + w1*w1) + w2*w2, A = sin(th)/th, B = (1 - cos(th))/th2
    (th2 < 1e-12: A = 1 - th2/6, B = 0.5 - th2/24);  c <- c + dc;  X <- X + dX.
Step.  H = J^T W J, g = J^T W r, D = clip(diag H, 1e-6, 1e32);  (H + lambda D) delta = -g.
Decision, in this order:  cost_new = sum rho at the trial point (+inf with a non-positive depth);
    pred = sum w (|r|^2 - |r + J delta|^2);  gain = (cost - cost_new) / pred;
    ACCEPT iff no non-positive depth and pred > 0 and gain > ACCEPT_RATIO.
    accept: rel = (cost - cost_new)/cost; lambda = max(lambda/10, LAMBDA_MIN); stop (FTOL) unless rel >= ftol
    reject: state restored; lambda = lambda*10; stop (LAMBDA) when lambda > LAMBDA_MAX.
A non-positive depth at the start is fatal (ValueError here, PGI_ERR_INVALID on the device; nothing is written).
"""
import numpy as np

import triangulate_spec as TS

DEFAULTS = dict(iters=20, cg_iters=200, min_cam_obs=8, use_low_parallax=0, huber_px=4.0, cg_tol=1e-6, ftol=1e-9, lambda_init=1e-4)
ACCEPT_RATIO = 1e-4
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
DIAG_MIN, DIAG_MAX = 1e-6, 1e32
STOP_ITERS, STOP_FTOL, STOP_LAMBDA, STOP_EMPTY = 0, 1, 2, 3


# ---- participation ----------------------------------------------------------------------------------------------------
def participation(track_begin, members, views, X, status, obs_state, fixed=None, min_cam_obs=8, use_low_parallax=0):
    """-> dict pt, view, member (index into members), px, py [N] in track order; free [V] bool; n_points."""
    tb = np.asarray(track_begin, np.int64)
    mem = np.asarray(members, np.uint64)
    V = len(views["xy"])
    has = np.ones(V, bool) if views.get("has_pose") is None else np.asarray(views["has_pose"], bool)
    pt, view, midx, px, py = [], [], [], [], []
    n_points = 0
    for t in range(len(tb) - 1):
        ok = status[t] == TS.OK or (use_low_parallax and status[t] == TS.LOW_PARALLAX)
        if not ok or not np.all(np.isfinite(X[t])):
            continue
        cand = []
        for m in range(tb[t], tb[t + 1]):
            v, kp = int(mem[m] >> np.uint64(32)), int(mem[m] & np.uint64(0xFFFFFFFF))
            if obs_state[m] == 1 and v < V and has[v] and kp < len(views["xy"][v]):
                cand.append((m, v, kp))
        if len(cand) < 2:
            continue
        n_points += 1
        for m, v, kp in cand:
            pt.append(t), view.append(v), midx.append(m)
            px.append(float(views["xy"][v][kp][0])), py.append(float(views["xy"][v][kp][1]))
    view_a = np.array(view, np.int64)
    cnt = np.bincount(view_a, minlength=V) if len(view_a) else np.zeros(V, np.int64)
    free = has & (cnt >= max(min_cam_obs, 1))
    if fixed is None:
        held = np.nonzero(has & (cnt > 0))[0]
        if len(held):
            free[held[0]] = False
    else:
        free &= ~np.asarray(fixed, bool)
    return dict(pt=np.array(pt, np.int64), view=view_a, member=np.array(midx, np.int64), px=np.array(px), py=np.array(py),
                free=free, cam_count=cnt, n_points=n_points)


# ---- model ------------------------------------------------------------------------------------------------------------
def linearize(R, c, K, X, ob, huber_px, ft=np.float64):
    """-> dict r [N,2], w [N], rho [N], Jw [N,2,3], Jp [N,2,3], nonpos (bool), cost."""
    v, t = ob["view"], ob["pt"]
    Rv = np.asarray(R, ft).reshape(-1, 3, 3)[v]
    d = np.asarray(X, ft)[t] - np.asarray(c, ft)[v]
    Kv = np.asarray(K, ft)[v]
    px, py = ob["px"].astype(ft), ob["py"].astype(ft)
    h = ft(huber_px)
    with np.errstate(all="ignore"):
        q = [(Rv[:, i, 0] * d[:, 0] + Rv[:, i, 1] * d[:, 1]) + Rv[:, i, 2] * d[:, 2] for i in range(3)]
        pos = q[2] > 0
        a, b, iz = q[0] / q[2], q[1] / q[2], 1 / q[2]
        r0 = (Kv[:, 0] * a + Kv[:, 2]) - px
        r1 = (Kv[:, 1] * b + Kv[:, 3]) - py
        e2 = r0 * r0 + r1 * r1
        e = np.sqrt(e2)
        inl = e <= h
        w = np.where(inl, ft(1), h / e)
        rho = np.where(inl, e2, (2 * h) * e - h * h)
        rho = np.where(pos, rho, np.inf)
        sx, sy = Kv[:, 0] * iz, Kv[:, 1] * iz
        Jp = np.stack([np.stack([sx * (Rv[:, 0, i] - a * Rv[:, 2, i]) for i in range(3)], 1),
                       np.stack([sy * (Rv[:, 1, i] - b * Rv[:, 2, i]) for i in range(3)], 1)], 1)
        Jw = np.stack([np.stack([-(sx * (a * q[1])), sx * (q[2] + a * q[0]), -(sx * q[1])], 1),
                       np.stack([-(sy * (q[2] + b * q[1])), sy * (b * q[0]), sy * q[0]], 1)], 1)
    return dict(r=np.stack([r0, r1], 1), w=w, rho=rho, Jw=Jw, Jp=Jp, nonpos=bool((~pos).any()), cost=rho.sum(dtype=ft))


def rodrigues_update(R, om):
    """E R with E = exp([om]x) as written in the module docstring; R [F,3,3], om [F,3]."""
    w0, w1, w2 = om[:, 0], om[:, 1], om[:, 2]
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    small = th2 < 1e-12
    th = np.sqrt(np.where(small, 1, th2))
    A = np.where(small, 1 - th2 / 6, np.sin(th) / th)
    B = np.where(small, 0.5 - th2 / 24, (1 - np.cos(th)) / np.where(small, 1, th2))
    E = np.empty(R.shape, R.dtype)
    E[:, 0, 0] = 1 - B * (w1 * w1 + w2 * w2)
    E[:, 0, 1] = B * (w0 * w1) - A * w2
    E[:, 0, 2] = B * (w0 * w2) + A * w1
    E[:, 1, 0] = B * (w0 * w1) + A * w2
    E[:, 1, 1] = 1 - B * (w0 * w0 + w2 * w2)
    E[:, 1, 2] = B * (w1 * w2) - A * w0
    E[:, 2, 0] = B * (w0 * w2) - A * w1
    E[:, 2, 1] = B * (w1 * w2) + A * w0
    E[:, 2, 2] = 1 - B * (w0 * w0 + w1 * w1)
    return E @ R


def _scatter(n, idx, vals, order=None):
    """sum of vals by idx, sequentially in the given order of the observations (np.add.at adds one by one)."""
    out = np.zeros((n,) + vals.shape[1:], vals.dtype)
    if order is None:
        np.add.at(out, idx, vals)
    else:
        np.add.at(out, idx[order], vals[order])
    return out


# ---- the damped step: direct dense solve ----------------------------------------------------------------------------------
def step_direct(lin, ob, n_views, n_tracks, lam):
    """(H + lam D) delta = -g over the free cameras and the participating points, dense.  -> (dcam [V,6], dpt [T,3])."""
    free = ob["free"]
    cams = np.nonzero(free)[0]
    pts = np.unique(ob["pt"])
    ci = np.full(n_views, -1)
    ci[cams] = np.arange(len(cams))
    pi = np.full(n_tracks, -1)
    pi[pts] = np.arange(len(pts))
    nC, nP = 6 * len(cams), 3 * len(pts)
    J = np.zeros((2 * len(ob["pt"]), nC + nP))
    Jc = np.concatenate([lin["Jw"], -lin["Jp"]], 2)
    for o in range(len(ob["pt"])):
        k = ci[ob["view"][o]]
        if k >= 0:
            J[2 * o:2 * o + 2, 6 * k:6 * k + 6] = Jc[o]
        j = pi[ob["pt"][o]]
        J[2 * o:2 * o + 2, nC + 3 * j:nC + 3 * j + 3] = lin["Jp"][o]
    wv = np.repeat(lin["w"], 2)
    H = J.T @ (J * wv[:, None])
    g = J.T @ (wv * lin["r"].reshape(-1))
    D = np.clip(np.diag(H), DIAG_MIN, DIAG_MAX)
    delta = np.linalg.solve(H + lam * np.diag(D), -g)
    dcam, dpt = np.zeros((n_views, 6)), np.zeros((n_tracks, 3))
    dcam[cams] = delta[:nC].reshape(-1, 6)
    dpt[pts] = delta[nC:].reshape(-1, 3)
    return dcam, dpt


# ---- the damped step by the kernels' formulas ---------------------------------------------------------------------------
def _inv_sym3(M):
    a00, a01, a02, a11, a12, a22 = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    inv = np.stack([np.stack([c00, c01, c02], 1), np.stack([c01, c11, c12], 1), np.stack([c02, c12, c22], 1)], 1)
    return inv / det[:, None, None]


def _chol6(S):
    L = np.zeros_like(S)
    for i in range(6):
        for j in range(i + 1):
            s = S[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)
            L[:, i, j] = np.sqrt(s) if i == j else s / L[:, j, j]
    return L


def _chol_solve(L, r):
    y = np.zeros_like(r)
    for i in range(6):
        y[:, i] = (r[:, i] - (L[:, i, :i] * y[:, :i]).sum(1)) / L[:, i, i]
    z = np.zeros_like(r)
    for i in range(5, -1, -1):
        z[:, i] = (y[:, i] - (L[:, i + 1:, i] * z[:, i + 1:]).sum(1)) / L[:, i, i]
    return z


def step_pcg(lin, ob, n_views, n_tracks, lam, cg_iters, cg_tol, ft=np.float64, cam_order=None, exact_blocks=False):
    """The Schur-form step as the kernels compute it: V^-1 by the adjugate, the Schur-Jacobi blocks as
    sum J_c^T (w I - w^2 J_p V^-1 J_p^T) J_c + lam D, 6 x 6 Cholesky, PCG with the implicit two-pass product, per-point sums
    in member order, per-camera sums in list order (cam_order: a permutation of the observations for the camera sums).
    exact_blocks: LAPACK inverses instead (float64 only).  -> (dcam, dpt, iterations run)."""
    v, t = ob["view"], ob["pt"]
    free = ob["free"]
    w = lin["w"].astype(ft)
    r = lin["r"].astype(ft)
    Jp = lin["Jp"].astype(ft)
    Jc = np.concatenate([lin["Jw"].astype(ft), -Jp], 2)
    lam = ft(lam)
    fo = free[v]                                             # observations of free cameras
    Vb = _scatter(n_tracks, t, w[:, None, None] * np.einsum("nki,nkj->nij", Jp, Jp))
    gp = _scatter(n_tracks, t, w[:, None] * np.einsum("nki,nk->ni", Jp, r))
    part = np.zeros(n_tracks, bool)
    part[t] = True
    i3 = np.arange(3)
    Vb[:, i3, i3] += lam * np.clip(Vb[:, i3, i3], DIAG_MIN, DIAG_MAX)
    Vb[~part] = np.eye(3, dtype=ft)
    Vinv = np.linalg.inv(Vb.astype(np.float64)).astype(ft) if exact_blocks else _inv_sym3(Vb)
    s = np.einsum("tij,tj->ti", Vinv, gp)
    A = np.einsum("nki,nij,nlj->nkl", Jp, Vinv[t], Jp)
    B = w[:, None, None] * np.eye(2, dtype=ft)[None] - (w * w)[:, None, None] * A
    Sb = _scatter(n_views, v[fo], np.einsum("nki,nkl,nlj->nij", Jc, B, Jc)[fo], cam_order_of(cam_order, fo))
    dU = _scatter(n_views, v[fo], (w[:, None] * (Jc * Jc).sum(1))[fo], cam_order_of(cam_order, fo))
    y = w[:, None] * (np.einsum("nki,ni->nk", Jp, s[t]) - r)
    b = _scatter(n_views, v[fo], np.einsum("nki,nk->ni", Jc, y)[fo], cam_order_of(cam_order, fo))
    lamD = lam * np.clip(dU, DIAG_MIN, DIAG_MAX)
    i6 = np.arange(6)
    Sb[:, i6, i6] += lamD
    Sb[~free] = np.eye(6, dtype=ft)
    lamD[~free] = 0
    if exact_blocks:
        Minv = np.linalg.inv(Sb.astype(np.float64))
        prec = lambda x: np.einsum("vij,vj->vi", Minv, x)
    else:
        L = _chol6(Sb)
        prec = lambda x: _chol_solve(L, x)

    def product(p):
        yy = np.einsum("nki,ni->nk", Jc, p[v])
        u = _scatter(n_tracks, t, w[:, None] * np.einsum("nki,nk->ni", Jp, yy))
        tj = np.einsum("tij,tj->ti", Vinv, u)
        yy = w[:, None] * (yy - np.einsum("nki,ni->nk", Jp, tj[t]))
        qq = _scatter(n_views, v[fo], np.einsum("nki,nk->ni", Jc, yy)[fo], cam_order_of(cam_order, fo))
        return qq + lamD * p, tj

    x = np.zeros((n_views, 6), ft)
    rr = b.copy()
    z = prec(rr)
    z[~free] = 0
    p = np.zeros_like(x)
    rz_prev, rz0, ran = ft(0), ft(0), 0
    for it in range(cg_iters + 1):
        rz = (rr * z).sum(dtype=ft)
        if it == 0:
            rz0 = rz
        beta = rz / rz_prev if it > 0 and rz_prev > 0 else ft(0)
        if not rz > (ft(cg_tol) * ft(cg_tol)) * rz0 or it >= cg_iters:
            break
        ran += 1
        p = z + beta * p
        q, _ = product(p)
        pq = (p * q).sum(dtype=ft)
        alpha = rz / pq if pq > 0 else ft(0)
        x = x + alpha * p
        rr = rr - alpha * q
        z = prec(rr)
        z[~free] = 0
        rz_prev = rz
    _, tj = product(x)
    dpt = -(s + tj)
    dpt[~part] = 0
    return x, dpt, ran


def cam_order_of(cam_order, fo):
    """The permutation of the free-camera observations that cam_order induces (None = list order)."""
    if cam_order is None:
        return None
    keep = fo[cam_order]
    rank = np.cumsum(fo) - 1
    return rank[cam_order[keep]]


# ---- Levenberg-Marquardt ---------------------------------------------------------------------------------------------------
def bundle_adjust(track_begin, members, views, X, status, obs_state, fixed=None, solver="direct", force_accept=False,
                  ft=np.float64, cam_order=None, exact_blocks=False, trace=None, **params):
    """-> dict R [V,3,3], c [V,3], X [T,3] (inputs are not modified) and the report fields.  solver: "direct" (dense f64
    solve of the damped normal equations) or "pcg" (step_pcg).  trace (a list) receives one dict per outer iteration:
    gain, accepted, cg_iters, lam, cost, cost_new.  ValueError: a non-positive depth at the start."""
    prm = dict(DEFAULTS)
    for k, val in params.items():
        if k not in prm:
            raise TypeError("unknown parameter %r" % k)
        prm[k] = val
    R = np.array(views["R"], ft).reshape(-1, 3, 3)
    c = np.array(views["c"], ft)
    K = np.asarray(views["K"], np.float64)
    X = np.array(X, ft)
    V, T = len(R), len(X)
    ob = participation(track_begin, members, views, X, status, obs_state, fixed, prm["min_cam_obs"], prm["use_low_parallax"])
    rep = dict(iters=0, accepted=0, cg_iters_total=0, stop_reason=STOP_EMPTY, n_obs=len(ob["pt"]), n_points=ob["n_points"],
               n_free_cams=int(ob["free"].sum()) if len(ob["pt"]) else 0, cost_initial=0.0, cost_final=0.0, lambda_final=prm["lambda_init"])
    if not len(ob["pt"]):
        return dict(R=R, c=c, X=X, ob=ob, **rep)
    lin = linearize(R, c, K, X, ob, prm["huber_px"], ft)
    if lin["nonpos"]:
        raise ValueError("a participating observation has a non-positive depth at the start")
    cost = lin["cost"]
    rep["cost_initial"] = float(cost)
    rep["stop_reason"] = STOP_ITERS
    lam = prm["lambda_init"]
    free = ob["free"]
    for _ in range(prm["iters"]):
        rep["iters"] += 1
        if solver == "direct":
            dcam, dpt = step_direct(lin, ob, V, T, lam)
            ran = 0
        else:
            dcam, dpt, ran = step_pcg(lin, ob, V, T, lam, prm["cg_iters"], prm["cg_tol"], ft, cam_order, exact_blocks)
        rep["cg_iters_total"] += ran
        dcam, dpt = dcam.astype(ft), dpt.astype(ft)
        Rn, cn, Xn = R.copy(), c.copy(), X + dpt
        Rn[free] = rodrigues_update(R[free], dcam[free, :3])
        cn[free] = c[free] + dcam[free, 3:]
        new = linearize(Rn, cn, K, Xn, ob, prm["huber_px"], ft)
        v, t = ob["view"], ob["pt"]
        lr = lin["r"] + np.einsum("nki,ni->nk", lin["Jw"], dcam[v, :3]) + np.einsum("nki,ni->nk", lin["Jp"], dpt[t] - dcam[v, 3:])
        pred = (lin["w"] * ((lin["r"] ** 2).sum(1) - (lr ** 2).sum(1))).sum(dtype=ft)
        with np.errstate(all="ignore"):
            gain = (cost - new["cost"]) / pred
        accept = force_accept or (not new["nonpos"] and pred > 0 and gain > ACCEPT_RATIO)
        if trace is not None:
            trace.append(dict(gain=float(gain), accepted=bool(accept), cg_iters=ran, lam=lam, cost=float(cost), cost_new=float(new["cost"]),
                              R=Rn, c=cn, X=Xn))
        if accept:
            rel = (cost - new["cost"]) / cost
            R, c, X, lin, cost = Rn, cn, Xn, new, new["cost"]
            rep["accepted"] += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            if not force_accept and not rel >= prm["ftol"]:
                rep["stop_reason"] = STOP_FTOL
                break
        else:
            lam = lam * 10.0
            if lam > LAMBDA_MAX:
                rep["stop_reason"] = STOP_LAMBDA
                break
    rep["cost_final"] = float(cost)
    rep["lambda_final"] = lam
    return dict(R=R, c=c, X=X, ob=ob, **rep)


# ---- measures ------------------------------------------------------------------------------------------------------------------
def state_distance(a, b, start):
    """max |a - b| over R, c and X of the participating tracks, relative to the largest move max |b - start| (no alignment)."""
    part = np.zeros(len(b["X"]), bool)
    part[b["ob"]["pt"]] = True
    num = max(np.abs(np.asarray(a["R"], np.longdouble).reshape(-1, 3, 3) - b["R"]).max(), np.abs(a["c"] - b["c"]).max(),
              np.abs(a["X"] - b["X"])[part].max())
    den = max(np.abs(b["R"] - np.asarray(start["R"]).reshape(-1, 3, 3)).max(), np.abs(b["c"] - start["c"]).max(),
              np.abs(b["X"] - start["X"])[part].max())
    return float(num / den)


def aligned_centre_error(c, c_gt):
    """RMS |s Q c + t - c_gt| after the best similarity (Umeyama)."""
    mu, mg = c.mean(0), c_gt.mean(0)
    a, b = c - mu, c_gt - mg
    U, S, Vt = np.linalg.svd(b.T @ a)
    d = np.sign(np.linalg.det(U @ Vt))
    Dm = np.diag([1.0, 1.0, d])
    Q = U @ Dm @ Vt
    s = (S * np.diag(Dm)).sum() / (a ** 2).sum()
    return float(np.sqrt((((s * (Q @ a.T)).T - b) ** 2).sum(1).mean()))


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def make_problem(V=12, T=60, seed=1, rot_deg=0.05, centre_sigma=0.01, tri=None, **scene):
    """triangulate_spec.make_scene with its ground-truth poses perturbed (seeded rotation about a random axis of rot_deg
    degrees RMS per axis, centre noise centre_sigma) and triangulated by the specification from those poses, so that X,
    status and obs_state are consistent.  tri: parameters of the triangulation.
    -> dict track_begin, members, views (perturbed), views_gt, X, status, obs_state, X_gt."""
    sc = TS.make_scene(V=V, T=T, seed=seed, **scene)
    rng = np.random.default_rng(seed + 7919)
    gt = sc["views"]
    R0 = TS._rodrigues(rng.standard_normal((V, 3)) * np.deg2rad(rot_deg)) @ np.asarray(gt["R"]).reshape(V, 3, 3)
    c0 = np.asarray(gt["c"]) + rng.standard_normal((V, 3)) * centre_sigma
    views = dict(gt, R=R0, c=c0)
    tr = TS.triangulate(sc["track_begin"], sc["members"], views, **(tri or dict(thr_px=8.0)))
    return dict(track_begin=sc["track_begin"], members=sc["members"], views=views, views_gt=gt, X=tr["X"], status=tr["status"],
                obs_state=tr["obs_state"], X_gt=sc["X_gt"], planted=sc["planted"])


def run(p, **kw):
    return bundle_adjust(p["track_begin"], p["members"], p["views"], p["X"], p["status"], p["obs_state"], **kw)


# ---- the cases of tests/test_bundle.py and scripts/bundle_roundoff.py ---------------------------------------------------------
STEP_COUNTS = (1, 2, 7)
STEP_PARAMS = dict(iters=1, min_cam_obs=1, cg_tol=1e-30)   # the n-th iterate of the first damped system, never converged
CONVERGED_PARAMS = dict(iters=3, cg_iters=500, cg_tol=1e-13, min_cam_obs=1)
GAIN_MARGIN = 0.1


def step_cases():
    """name -> (V, T): free cameras 1 (V = 2), 2, 63 / 64 / 65 at 300 points; 1, 63, 64, 65 points at 12 views.  The PCG
    has one launch shape for every camera count, so there is no switch to straddle."""
    cases = {"V%d-T300" % V: (V, 300) for V in (2, 3, 64, 65, 66)}
    cases.update({"V12-T%d" % T: (12, T) for T in (1, 63, 64, 65)})
    return cases


def step_problem(V, T):
    return make_problem(V=V, T=T, seed=3, min_len=2 if V < 4 else 4, outlier_every=0)


def step_reference(p, n, ft=np.longdouble, **kw):
    """The state after the n-th PCG iterate of the first damped system, acceptance forced."""
    return run(p, solver="pcg", force_accept=True, ft=ft, cg_iters=n, **dict(STEP_PARAMS, **kw))


def list_shapes_problem():
    """306 views, 300 tracks of 2..70 members over the first 100 views; view 5 has exactly 64 participating observations
    (one pass of a wavefront), most others more; view 6 has min_cam_obs - 1 = 7 (held); views 100..304 are posed and see
    nothing; view 305 has no pose; track 10 is REPROJ, track 11 has a single used member, track 12 has two dropped
    (obs_state 2) members.  -> (problem, dict of the special indices)."""
    base = make_problem(V=100, T=300, seed=5, min_len=2, max_len=70, outlier_every=0)
    V = 306
    v0 = base["views"]
    extra = V - 100
    rng = np.random.default_rng(17)
    views = dict(R=np.concatenate([np.asarray(v0["R"]).reshape(-1, 3, 3), np.tile(np.eye(3), (extra, 1, 1))]),
                 c=np.concatenate([v0["c"], rng.uniform(-1, 1, (extra, 3))]),
                 K=np.concatenate([v0["K"], np.tile(v0["K"][:1], (extra, 1))]),
                 has_pose=np.concatenate([np.ones(V - 1, bool), [False]]),
                 xy=list(v0["xy"]) + [np.zeros((0, 2), np.float32)] * extra)
    state = base["obs_state"].copy()
    status = base["status"].copy()
    mem_view = (base["members"] >> np.uint64(32)).astype(np.int64)
    tb = base["track_begin"].astype(np.int64)
    status[10] = TS.REPROJ
    state[tb[11] + 1:tb[11 + 1]] = 0
    long_t = int(np.argmax(np.diff(tb)))
    assert long_t not in (10, 11)
    state[tb[long_t] + 3:tb[long_t] + 5] = 2
    ok_track = np.repeat((status == TS.OK) & (np.arange(300) != 11), np.diff(tb))
    for view, keep in ((5, 64), (6, DEFAULTS["min_cam_obs"] - 1)):
        mine = np.nonzero((mem_view == view) & (state == 1) & ok_track)[0]
        assert len(mine) > keep
        state[mine[keep:]] = 0
    p = dict(base, views=views, obs_state=state, status=status)
    return p, dict(reproj=10, single=11, dropped=long_t, one_pass=5, held=6)


CONVERGED_SCENES = ((12, 60, 1), (65, 200, 2))   # (V, T, seed)
DEFAULT_SCENES = ((12, 60, 1), (65, 200, 2))     # noisy, with the planted 47 px observations left in (OUTLIER_TRI)
OUTLIER_TRI = dict(thr_px=60.0, max_drops=0)     # triangulation that neither trims nor refuses the planted observations


def rejection_problem(depth=0.05):
    """The noisy 12-view scene plus two hand-made views (12 at the origin, 13 at (1, 0, 0), both looking down +z; one
    observation each, so they are held) and one track at (0.5, 0, depth) whose pixels ask for x / z = +-30 where the point
    gives +-10: the Gauss-Newton step in z is -0.1 / (1 + lambda), so the first trial point lies behind both views.
    depth < 0: the start itself is behind them."""
    p = make_problem(V=12, T=60, seed=1)
    v0 = p["views"]
    eye = np.eye(3)[None]
    views = dict(R=np.concatenate([np.asarray(v0["R"]).reshape(-1, 3, 3), eye, eye]), c=np.concatenate([v0["c"], [[0, 0, 0], [1.0, 0, 0]]]),
                 K=np.concatenate([v0["K"], v0["K"][:2]]), has_pose=np.ones(14, bool),
                 xy=list(v0["xy"]) + [np.array([[31000.0, 1000.0]], np.float32), np.array([[-29000.0, 1000.0]], np.float32)])
    return dict(p, views=views, track_begin=np.concatenate([p["track_begin"], [p["track_begin"][-1] + 2]]).astype(np.uint32),
                members=np.concatenate([p["members"], TS.pack([12, 13], [0, 0])]), X=np.concatenate([p["X"], [[0.5, 0.0, depth]]]),
                status=np.concatenate([p["status"], [TS.OK]]).astype(np.uint8), obs_state=np.concatenate([p["obs_state"], [1, 1]]).astype(np.uint8))
