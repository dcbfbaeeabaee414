"""bundle_focal_spec.py -- CPU SPECIFICATION of the bundle adjustment with per-view focal scales (test infrastructure, NOT
product code).  States what pgi_bundle_adjust_focal computes; everything that is not said
here is bundle_spec.py, which this module imports and leaves as it is.

Parameter.  One scalar phi_v per view; fx = fx0 * phi, fy = fy0 * phi (one multiplication each), fx0 / fy0 the values of the
    view table; cx, cy are not refined.  The residual is bundle_spec.linearize with these fx, fy.
New Jacobian column.  d r / d phi = (fx0 * a, fy0 * b).
Update.  phi <- phi + dphi.
Trial-step rejection.  A trial point is rejected when some phi_new > 0 fails (one comparison, with the depth sign; a NaN
    fails it): the trial cost is +inf.
Focal-free views.  posed, not marked in focal_fixed, at least max(min_focal_obs, 1) participating observations.  This is
    independent of the pose being free: the gauge view and a `fixed` view may have a free focal (a camera block with the
    focal column alone), a pose-free view may have a held focal.  A parameter that is not free is not an unknown.
Everything else (participation, gauge, Huber, D = clip(diag J^T W J, 1e-6, 1e32), gain ratio, stopping rules) is unchanged;
    the damped system and the predicted decrease include the focal unknowns.
The kernel-formula solver (step_pcg) uses 7 x 7 camera blocks whose columns of pinned parameters are zero: their block rows
hold lambda D alone, their right-hand side and PCG components stay 0, which is the same system up to round-off.
"""
import numpy as np

import bundle_spec as B
import triangulate_spec as TS

MIN_FOCAL_OBS = 30   # the default of the Python interface: a choice, not a measurement


def focal_free(ob, views, focal_fixed=None, min_focal_obs=MIN_FOCAL_OBS):
    V = len(views["xy"])
    has = np.ones(V, bool) if views.get("has_pose") is None else np.asarray(views["has_pose"], bool)
    ff = has & (ob["cam_count"] >= max(int(min_focal_obs), 1))
    if focal_fixed is not None:
        ff &= ~np.asarray(focal_fixed, bool)
    return ff


def scaled_K(K0, phi, ft=np.float64):
    K = np.array(K0, ft)
    K[:, 0] = K[:, 0] * np.asarray(phi, ft)
    K[:, 1] = K[:, 1] * np.asarray(phi, ft)
    return K


def linearize(R, c, K0, phi, X, ob, huber_px, ft=np.float64):
    """bundle_spec.linearize at fx0 * phi, fy0 * phi, plus Jf [N,2] = (fx0 * a, fy0 * b) and the phi > 0 rule."""
    lin = B.linearize(R, c, scaled_K(K0, phi, ft), X, ob, huber_px, ft)
    v, t = ob["view"], ob["pt"]
    Rv = np.asarray(R, ft).reshape(-1, 3, 3)[v]
    d = np.asarray(X, ft)[t] - np.asarray(c, ft)[v]
    K0v = np.asarray(K0, ft)[v]
    with np.errstate(all="ignore"):
        q = [(Rv[:, i, 0] * d[:, 0] + Rv[:, i, 1] * d[:, 1]) + Rv[:, i, 2] * d[:, 2] for i in range(3)]
        lin["Jf"] = np.stack([K0v[:, 0] * (q[0] / q[2]), K0v[:, 1] * (q[1] / q[2])], 1)
        bad = ~(np.asarray(phi, ft)[v] > 0)
    if bad.any():
        lin["rho"] = np.where(bad, np.inf, lin["rho"])
        lin["cost"] = lin["rho"].sum(dtype=ft)
        lin["nonpos"] = True
    return lin


def camera_columns(lin, ob, ffree, ft=np.float64):
    """J_c [N,2,7] = (J_w, -J_p, J_f) with the columns of pinned parameters zero."""
    Jc = np.concatenate([lin["Jw"].astype(ft), -lin["Jp"].astype(ft), lin["Jf"].astype(ft)[:, :, None]], 2)
    mask = np.concatenate([np.repeat(ob["free"][:, None], 6, 1), ffree[:, None]], 1)
    return Jc * mask[ob["view"]][:, None, :].astype(ft), mask


# ---- the damped step: direct dense solve over the free parameters only -------------------------------------------------
def step_direct(lin, ob, ffree, n_views, n_tracks, lam):
    """-> (dcam [V,7], dpt [T,3]).  Unknowns: 6 per pose-free view, then 1 per focal-free view, then 3 per point."""
    cams, fcams, pts = np.nonzero(ob["free"])[0], np.nonzero(ffree)[0], np.unique(ob["pt"])
    ci, fi, pi = np.full(n_views, -1), np.full(n_views, -1), np.full(n_tracks, -1)
    ci[cams], fi[fcams], pi[pts] = np.arange(len(cams)), np.arange(len(fcams)), np.arange(len(pts))
    nC, nF, nP = 6 * len(cams), len(fcams), 3 * len(pts)
    J = np.zeros((2 * len(ob["pt"]), nC + nF + nP))
    Jc = np.concatenate([lin["Jw"], -lin["Jp"]], 2)
    for o in range(len(ob["pt"])):
        k = ci[ob["view"][o]]
        if k >= 0:
            J[2 * o:2 * o + 2, 6 * k:6 * k + 6] = Jc[o]
        f = fi[ob["view"][o]]
        if f >= 0:
            J[2 * o:2 * o + 2, nC + f] = lin["Jf"][o]
        j = pi[ob["pt"][o]]
        J[2 * o:2 * o + 2, nC + nF + 3 * j:nC + nF + 3 * j + 3] = lin["Jp"][o]
    wv = np.repeat(lin["w"], 2)
    H = J.T @ (J * wv[:, None])
    g = J.T @ (wv * lin["r"].reshape(-1))
    D = np.clip(np.diag(H), B.DIAG_MIN, B.DIAG_MAX)
    delta = np.linalg.solve(H + lam * np.diag(D), -g)
    dcam, dpt = np.zeros((n_views, 7)), np.zeros((n_tracks, 3))
    dcam[cams, :6] = delta[:nC].reshape(-1, 6)
    dcam[fcams, 6] = delta[nC:nC + nF]
    dpt[pts] = delta[nC + nF:].reshape(-1, 3)
    return dcam, dpt


# ---- the damped step by the kernels' formulas ---------------------------------------------------------------------------
def _chol(S):
    n = S.shape[1]
    L = np.zeros_like(S)
    for i in range(n):
        for j in range(i + 1):
            s = S[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)
            L[:, i, j] = np.sqrt(s) if i == j else s / L[:, j, j]
    return L


def _chol_solve(L, r):
    n = L.shape[1]
    y = np.zeros_like(r)
    for i in range(n):
        y[:, i] = (r[:, i] - (L[:, i, :i] * y[:, :i]).sum(1)) / L[:, i, i]
    z = np.zeros_like(r)
    for i in range(n - 1, -1, -1):
        z[:, i] = (y[:, i] - (L[:, i + 1:, i] * z[:, i + 1:]).sum(1)) / L[:, i, i]
    return z


def step_pcg(lin, ob, ffree, n_views, n_tracks, lam, cg_iters, cg_tol, ft=np.float64, cam_order=None):
    """bundle_spec.step_pcg with 7 x 7 camera blocks (module docstring).  -> (dcam [V,7], dpt, iterations run)."""
    v, t = ob["view"], ob["pt"]
    w, r, Jp = lin["w"].astype(ft), lin["r"].astype(ft), lin["Jp"].astype(ft)
    Jc, mask = camera_columns(lin, ob, ffree, ft)
    lam = ft(lam)
    active = mask.any(1)
    fo = active[v]
    order = B.cam_order_of(cam_order, fo)
    Vb = B._scatter(n_tracks, t, w[:, None, None] * np.einsum("nki,nkj->nij", Jp, Jp))
    gp = B._scatter(n_tracks, t, w[:, None] * np.einsum("nki,nk->ni", Jp, r))
    part = np.zeros(n_tracks, bool)
    part[t] = True
    i3 = np.arange(3)
    Vb[:, i3, i3] += lam * np.clip(Vb[:, i3, i3], B.DIAG_MIN, B.DIAG_MAX)
    Vb[~part] = np.eye(3, dtype=ft)
    Vinv = B._inv_sym3(Vb)
    s = np.einsum("tij,tj->ti", Vinv, gp)
    A = np.einsum("nki,nij,nlj->nkl", Jp, Vinv[t], Jp)
    Bm = w[:, None, None] * np.eye(2, dtype=ft)[None] - (w * w)[:, None, None] * A
    Sb = B._scatter(n_views, v[fo], np.einsum("nki,nkl,nlj->nij", Jc, Bm, Jc)[fo], order)
    dU = B._scatter(n_views, v[fo], (w[:, None] * (Jc * Jc).sum(1))[fo], order)
    y = w[:, None] * (np.einsum("nki,ni->nk", Jp, s[t]) - r)
    b = B._scatter(n_views, v[fo], np.einsum("nki,nk->ni", Jc, y)[fo], order)
    lamD = lam * np.clip(dU, B.DIAG_MIN, B.DIAG_MAX)
    i7 = np.arange(7)
    Sb[:, i7, i7] += lamD
    L = _chol(Sb)

    def prec(x):
        z = _chol_solve(L, x)
        z[~mask] = 0
        return z

    def product(p):
        yy = np.einsum("nki,ni->nk", Jc, p[v])
        u = B._scatter(n_tracks, t, w[:, None] * np.einsum("nki,nk->ni", Jp, yy))
        tj = np.einsum("tij,tj->ti", Vinv, u)
        yy = w[:, None] * (yy - np.einsum("nki,ni->nk", Jp, tj[t]))
        qq = B._scatter(n_views, v[fo], np.einsum("nki,nk->ni", Jc, yy)[fo], order)
        return qq + lamD * p, tj

    x = np.zeros((n_views, 7), ft)
    rr = b.copy()
    z = prec(rr)
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
        rz_prev = rz
    _, tj = product(x)
    dpt = -(s + tj)
    dpt[~part] = 0
    return x, dpt, ran


# ---- the trial point and the decision ---------------------------------------------------------------------------------------
def trial(state, lin, ob, ffree, K0, dcam, dpt, cost, huber_px, ft=np.float64, force_accept=False):
    """The decision function: the state moved by (dcam [V,7], dpt), its cost, the predicted decrease and the verdict.
    -> dict R, c, phi, X, lin, cost_new, pred, gain, accepted."""
    R, c, phi, X = state
    free = ob["free"]
    Rn, cn, pn, Xn = R.copy(), c.copy(), phi.copy(), X + dpt
    Rn[free] = B.rodrigues_update(R[free], dcam[free, :3])
    cn[free] = c[free] + dcam[free, 3:6]
    pn[ffree] = phi[ffree] + dcam[ffree, 6]
    new = linearize(Rn, cn, K0, pn, Xn, ob, huber_px, ft)
    v, t = ob["view"], ob["pt"]
    lr = lin["r"] + np.einsum("nki,ni->nk", lin["Jw"], dcam[v, :3]) + np.einsum("nki,ni->nk", lin["Jp"], dpt[t] - dcam[v, 3:6])
    lr = lr + lin["Jf"] * dcam[v, 6][:, None]
    pred = (lin["w"] * ((lin["r"] ** 2).sum(1) - (lr ** 2).sum(1))).sum(dtype=ft)
    with np.errstate(all="ignore"):
        gain = (cost - new["cost"]) / pred
    accepted = bool(force_accept or (not new["nonpos"] and pred > 0 and gain > B.ACCEPT_RATIO))
    return dict(R=Rn, c=cn, phi=pn, X=Xn, lin=new, cost_new=new["cost"], pred=pred, gain=gain, accepted=accepted)


# ---- Levenberg-Marquardt -------------------------------------------------------------------------------------------------------
def bundle_adjust(track_begin, members, views, X, status, obs_state, focal=None, focal_fixed=None, min_focal_obs=MIN_FOCAL_OBS,
                  fixed=None, solver="direct", force_accept=False, ft=np.float64, cam_order=None, trace=None, **params):
    """bundle_spec.bundle_adjust with the focal scales.  -> dict R, c, X, phi [V] (inputs are not modified), ffree,
    n_free_focals and the report fields.  ValueError: a non-positive depth or focal scale at the start."""
    prm = dict(B.DEFAULTS)
    for k, val in params.items():
        if k not in prm:
            raise TypeError("unknown parameter %r" % k)
        prm[k] = val
    R = np.array(views["R"], ft).reshape(-1, 3, 3)
    c = np.array(views["c"], ft)
    K0 = np.asarray(views["K"], np.float64)
    X = np.array(X, ft)
    V, T = len(R), len(X)
    phi = np.ones(V, ft) if focal is None else np.array(focal, ft)
    ob = B.participation(track_begin, members, views, X, status, obs_state, fixed, prm["min_cam_obs"], prm["use_low_parallax"])
    ffree = focal_free(ob, views, focal_fixed, min_focal_obs) if len(ob["pt"]) else np.zeros(V, bool)
    has = np.ones(V, bool) if views.get("has_pose") is None else np.asarray(views["has_pose"], bool)
    if not np.all(phi[has] > 0) or not np.all(np.isfinite(phi[has].astype(np.float64))):
        raise ValueError("a posed view has a non-positive or non-finite focal scale")
    rep = dict(iters=0, accepted=0, cg_iters_total=0, stop_reason=B.STOP_EMPTY, n_obs=len(ob["pt"]), n_points=ob["n_points"],
               n_free_cams=int(ob["free"].sum()) if len(ob["pt"]) else 0, cost_initial=0.0, cost_final=0.0, lambda_final=prm["lambda_init"])
    out = lambda: dict(R=R, c=c, X=X, phi=phi, ob=ob, ffree=ffree, n_free_focals=int(ffree.sum()), **rep)
    if not len(ob["pt"]):
        return out()
    lin = linearize(R, c, K0, phi, X, ob, prm["huber_px"], ft)
    if lin["nonpos"]:
        raise ValueError("a participating observation has a non-positive depth at the start")
    cost = lin["cost"]
    rep["cost_initial"] = float(cost)
    rep["stop_reason"] = B.STOP_ITERS
    lam = prm["lambda_init"]
    for _ in range(prm["iters"]):
        rep["iters"] += 1
        if solver == "direct":
            dcam, dpt = step_direct(lin, ob, ffree, V, T, lam)
            ran = 0
        else:
            dcam, dpt, ran = step_pcg(lin, ob, ffree, V, T, lam, prm["cg_iters"], prm["cg_tol"], ft, cam_order)
        rep["cg_iters_total"] += ran
        tr = trial((R, c, phi, X), lin, ob, ffree, K0, dcam.astype(ft), dpt.astype(ft), cost, prm["huber_px"], ft, force_accept)
        if trace is not None:
            trace.append(dict(gain=float(tr["gain"]), accepted=tr["accepted"], cg_iters=ran, lam=lam, cost=float(cost),
                              cost_new=float(tr["cost_new"]), phi=tr["phi"]))
        if tr["accepted"]:
            rel = (cost - tr["cost_new"]) / cost
            R, c, phi, X, lin, cost = tr["R"], tr["c"], tr["phi"], tr["X"], tr["lin"], tr["cost_new"]
            rep["accepted"] += 1
            lam = max(lam / 10.0, B.LAMBDA_MIN)
            if not force_accept and not rel >= prm["ftol"]:
                rep["stop_reason"] = B.STOP_FTOL
                break
        else:
            lam = lam * 10.0
            if lam > B.LAMBDA_MAX:
                rep["stop_reason"] = B.STOP_LAMBDA
                break
    rep["cost_final"] = float(cost)
    rep["lambda_final"] = lam
    return out()


# ---- measures ------------------------------------------------------------------------------------------------------------------
def state_distance(a, b, start):
    """bundle_spec.state_distance extended by phi: max |a - b| over R, c, phi and the participating X, relative to the
    reference's largest move."""
    part = np.zeros(len(b["X"]), bool)
    part[b["ob"]["pt"]] = True
    num = max(np.abs(np.asarray(a["R"], np.longdouble).reshape(-1, 3, 3) - b["R"]).max(), np.abs(a["c"] - b["c"]).max(),
              np.abs(a["X"] - b["X"])[part].max(), np.abs(a["phi"] - b["phi"]).max())
    den = max(np.abs(b["R"] - np.asarray(start["R"]).reshape(-1, 3, 3)).max(), np.abs(b["c"] - start["c"]).max(),
              np.abs(b["X"] - start["X"])[part].max(), np.abs(b["phi"] - start["phi"]).max())
    return float(num / den)


def rotation_error_deg(R, R_gt):
    """RMS angle of R_i R_gt_i^T after removing the mean rotation (the gauge), degrees."""
    R, R_gt = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(R_gt, np.float64).reshape(-1, 3, 3)
    rel = np.einsum("vij,vkj->vik", R, R_gt)
    U, _, Vt = np.linalg.svd(rel.sum(0))
    mean = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    res = np.einsum("ji,vjk->vik", mean, rel)
    ang = np.arccos(np.clip((np.trace(res, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0))
    return float(np.rad2deg(np.sqrt((ang ** 2).mean())))


# ---- scenes ------------------------------------------------------------------------------------------------------------------
FOCAL_TRI = dict(thr_px=80.0, max_drops=0)   # the start is triangulated with focals that are 5 % off: nothing is trimmed


def make_problem(V=12, T=120, seed=1, focal_off=0.05, rot_deg=0.05, centre_sigma=0.01, **scene):
    """bundle_spec.make_problem whose starting focal scales are off by a seeded uniform +-focal_off per view: the view table
    holds the true focals (phi_gt = 1), phi0 = 1 + u, and the start is triangulated at fx0 * phi0, fy0 * phi0.
    -> the problem dict plus phi0."""
    sc = TS.make_scene(V=V, T=T, seed=seed, **scene)
    rng = np.random.default_rng(seed + 7919)
    gt = sc["views"]
    R0 = TS._rodrigues(rng.standard_normal((V, 3)) * np.deg2rad(rot_deg)) @ np.asarray(gt["R"]).reshape(V, 3, 3)
    c0 = np.asarray(gt["c"]) + rng.standard_normal((V, 3)) * centre_sigma
    phi0 = 1.0 + rng.uniform(-focal_off, focal_off, V)
    views = dict(gt, R=R0, c=c0)
    tr = TS.triangulate(sc["track_begin"], sc["members"], dict(views, K=scaled_K(gt["K"], phi0)), **FOCAL_TRI)
    return dict(track_begin=sc["track_begin"], members=sc["members"], views=views, views_gt=gt, X=tr["X"], status=tr["status"],
                obs_state=tr["obs_state"], X_gt=sc["X_gt"], planted=sc["planted"], phi0=phi0)


def run(p, **kw):
    kw.setdefault("focal", p["phi0"])
    return bundle_adjust(p["track_begin"], p["members"], p["views"], p["X"], p["status"], p["obs_state"], **kw)


def start_of(p):
    return dict(R=p["views"]["R"], c=p["views"]["c"], X=p["X"], phi=p["phi0"])


# ---- the cases of tests/test_bundle_focal.py and scripts/bundle_focal_roundoff.py ------------------------------------------------
STEP_COUNTS = B.STEP_COUNTS
STEP_PARAMS = dict(B.STEP_PARAMS)
STEP_MIN_FOCAL_OBS = 1
CONVERGED_PARAMS = dict(B.CONVERGED_PARAMS)


def step_cases():
    """name -> (V, T).  The last view is entirely pinned, so the ACTIVE cameras (a free pose or a free focal) number V - 1:
    1, 2, 3, 4, 5 (four cameras per 256-thread block), 63, 64, 65 at 300 points; 1, 63, 64, 65 points at 12 views."""
    cases = {"A%d-T300" % a: (a + 1, 300) for a in (1, 2, 3, 4, 5, 63, 64, 65)}
    cases.update({"V12-T%d" % T: (12, T) for T in (1, 63, 64, 65)})
    return cases


def step_masks(V):
    """The four kinds of view: v % 3 == 0: focal only (view 0 holds the gauge, the others are `fixed` views); v % 3 == 1: pose
    and focal; v % 3 == 2: pose only; the last view: neither.  -> (fixed, focal_fixed)."""
    idx = np.arange(V)
    last = idx == V - 1
    return (idx % 3 == 0) | last, (idx % 3 == 2) | last


def step_problem(V, T):
    return make_problem(V=V, T=T, seed=3, min_len=2 if V < 4 else 4, outlier_every=0)


def step_kwargs(p):
    fixed, focal_fixed = step_masks(len(p["views"]["xy"]))
    return dict(fixed=fixed, focal_fixed=focal_fixed, min_focal_obs=STEP_MIN_FOCAL_OBS)


def step_reference(p, n, ft=np.longdouble, **kw):
    return run(p, solver="pcg", force_accept=True, ft=ft, cg_iters=n, **dict(STEP_PARAMS, **step_kwargs(p), **kw))


LIST_MIN_FOCAL_OBS = 30


def list_shapes_problem():
    """bundle_spec.list_shapes_problem (306 views, tracks of 2 to 70 members, view 305 without a pose, view 5 with exactly 64
    observations) with focal scales off by up to 2 %, view 7 cut to exactly 65 observations, view 8 to exactly
    LIST_MIN_FOCAL_OBS (focal-free) and view 9 to one fewer (focal held).  -> (problem, indices)."""
    p, idx = B.list_shapes_problem()
    state = p["obs_state"].copy()
    mem_view = (p["members"] >> np.uint64(32)).astype(np.int64)
    ob = B.participation(p["track_begin"], p["members"], p["views"], p["X"], p["status"], state)
    for view, keep in ((7, 65), (8, LIST_MIN_FOCAL_OBS), (9, LIST_MIN_FOCAL_OBS - 1)):
        mine = ob["member"][ob["view"] == view]
        assert len(mine) > keep and np.all(mem_view[mine] == view)
        state[mine[keep:]] = 0
    V = len(p["views"]["xy"])
    phi0 = 1.0 + np.random.default_rng(23).uniform(-0.02, 0.02, V)
    phi0[305] = -1.0   # no pose: never read, never checked
    return dict(p, obs_state=state, phi0=phi0), dict(idx, two_pass=7, at_min=8, below_min=9)


CONVERGED_SCENES = ((12, 120, 1), (65, 400, 2))   # (V, T, seed): noisy, every view with at least 30 observations
