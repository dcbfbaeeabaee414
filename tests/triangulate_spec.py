"""triangulate_spec.py -- CPU SPECIFICATION of N-view track triangulation (test infrastructure, NOT product code).

The reference triangulates two views only (4 x 4 SVD, pose_utils.h:491-506); nothing there handles a track of N
views or rejects wrong observations.  This file states what csrc/pgi_triangulate.hip computes: the N-view midpoint,
a few Gauss-Newton steps on the pixel reprojection error, greedy drop-the-worst trimming and a parallax test.

EVERY floating-point statement below is ONE IEEE-754 f64 operation (+ - * / sqrt, all correctly rounded) in the
written order; the loops run over the observation index k (member order) and numpy vectorises across tracks only.
No einsum, no np.linalg, no BLAS.  The device kernel executes the same statements in the same order for one track
per lane (built with -ffp-contract=off), so the outputs agree bit for bit.

Inputs.  View v: R_v (3 x 3 row-major, world->camera), c_v (centre, world), fx fy cx cy, has_pose, keypoints n x 2
(f32 pixels, widened to f64 exactly).  Track t: members[track_begin[t] : track_begin[t + 1]], each view << 32 | keypoint.

Per track:
 1. eligibility, in member order: view < n_views, has_pose, keypoint < n of the view, both pixel coordinates finite,
    and no EARLIER ELIGIBLE member of the track has the same view (first occurrence wins).  state = 1 (used) or 0.
    Fewer than min_views eligible -> TOO_FEW (X, err_rms = NaN; n_used = eligible count; states stay).
 2. midpoint over the used members, accumulated in member order from 0:
        x = (px - cx) / fx;  y = (py - cy) / fy;  n = sqrt((x*x + y*y) + 1);  b = (x/n, y/n, 1/n)
        d_i = (R[0][i]*b0 + R[1][i]*b1) + R[2][i]*b2                      (d = R^T b)
        a00 += 1 - d0*d0;  a11 += 1 - d1*d1;  a22 += 1 - d2*d2;  a01 += -(d0*d1);  a02 += -(d0*d2);  a12 += -(d1*d2)
        dc = (d0*c0 + d1*c1) + d2*c2;   rhs_i += c_i - d_i*dc             ((I - d d^T) c)
    3 x 3 symmetric solve by the adjugate (solve_sym3 below: cofactors, det = (a00*c00 + a01*c01) + a02*c02,
    x_i = ((c_i0*b0 + c_i1*b1) + c_i2*b2) / det).  The matrix is dimensionless (unit rays), so the test is relative to
    the number of rays m only:  DEGENERATE unless  DET_REL * ((m*m)*m) < det < inf   (two rays at angle th: det = 2 sin^2 th).
 3. evaluation at X over the used members, in member order:
        dx = X - c;  q_i = (R[i][0]*dx0 + R[i][1]*dx1) + R[i][2]*dx2
        q2 > 0:  a = q0/q2;  b = q1/q2;  iz = 1/q2;  r0 = (fx*a + cx) - px;  r1 = (fy*b + cy) - py;  e2 = r0*r0 + r1*r1
                 sx = fx*iz;  sy = fy*iz;  ju_i = sx*(R[0][i] - a*R[2][i]);  jv_i = sy*(R[1][i] - b*R[2][i])
                 H_ij += ju_i*ju_j + jv_i*jv_j  (i <= j);   g_i += ju_i*r0 + jv_i*r1
        else:    e2 = +inf, the track is flagged `nonpos`, H and g are left alone
        cost += e2;  (e2 > max_e2) -> max_e2 = e2, arg = k          (max_e2 starts at -1: first maximum)
    refinement: only if the start has no non-positive depth.  Up to refine_iters times: delta = solve_sym3(H, g)
    (stop unless 0 < det < inf), Xn = X - delta, evaluate at Xn; accept iff no depth is non-positive and
    cost(Xn) < cost(X), otherwise stop.
 4. trimming: err = sqrt(max_e2).  While err > thr_px and n_used > max(2, min_views) and drops < max_drops: member
    `arg` goes to state 2, steps 2-3 again on the rest.  Then  not (err <= thr_px)  ->  BEHIND if nonpos else REPROJ.
 5. parallax over the used pairs j < k:  u = X - c;  n = sqrt((u0*u0 + u1*u1) + u2*u2);
        cos = ((uj0*uk0 + uj1*uk1) + uj2*uk2) / (nj*nk);   some cos < cos_min -> OK, else LOW_PARALLAX
    cos_min = cos(radians(min_angle_deg)) is computed once by the caller (libm) and handed over as an f64.
 outputs: X for OK / LOW_PARALLAX (NaN otherwise); err_rms = sqrt(cost / n_used) except TOO_FEW / DEGENERATE (NaN);
 n_used = members in state 1; status; obs_state per member; counts[s] = tracks with status s.
"""
import math

import numpy as np

OK, TOO_FEW, DEGENERATE, BEHIND, REPROJ, LOW_PARALLAX = 0, 1, 2, 3, 4, 5
N_STATUS = 6
DET_REL = 1e-12
DEFAULTS = dict(min_views=2, refine_iters=3, thr_px=2.0, max_drops=2, min_angle_deg=1.5)


def solve_sym3(a00, a01, a02, a11, a12, a22, b0, b1, b2):
    """-> (det, x0, x1, x2) of the symmetric 3 x 3 system by its adjugate, in this operation order."""
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    x0 = ((c00 * b0 + c01 * b1) + c02 * b2) / det
    x1 = ((c01 * b0 + c11 * b1) + c12 * b2) / det
    x2 = ((c02 * b0 + c12 * b1) + c22 * b2) / det
    return det, x0, x1, x2


class _Obs:
    """Per-member inputs padded to [T, L] (data movement only, no arithmetic)."""

    def __init__(self, track_begin, members, views):
        tb = np.asarray(track_begin, np.int64)
        mem = np.asarray(members, np.uint64)
        T = len(tb) - 1
        length = np.maximum(tb[1:] - tb[:-1], 0)
        L = int(length.max()) if T else 0
        R = np.asarray(views["R"], np.float64).reshape(-1, 9)
        c = np.asarray(views["c"], np.float64).reshape(-1, 3)
        K = np.asarray(views["K"], np.float64).reshape(-1, 4)
        V = len(R)
        has = np.ones(V, bool) if views.get("has_pose") is None else np.asarray(views["has_pose"], bool)
        n_kp = np.array([len(a) for a in views["xy"]], np.int64)
        kp_off = np.concatenate([[0], np.cumsum(n_kp)])
        xy = (np.concatenate([np.asarray(a).reshape(-1, 2) for a in views["xy"]]) if V else np.zeros((0, 2))).astype(np.float64)
        xy = np.concatenate([xy, np.zeros((1, 2))])
        k = np.arange(L)[None, :]
        self.present = k < length[:, None]
        idx = np.where(self.present, tb[:-1, None] + k, 0)
        key = mem[idx] if len(mem) else np.zeros((T, L), np.uint64)
        self.view = (key >> np.uint64(32)).astype(np.int64)
        kp = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        vs = np.where(self.view < V, self.view, 0)
        ok = self.present & (self.view < V)
        ok &= has[vs] if V else False
        ok &= kp < (n_kp[vs] if V else 0)
        row = np.where(ok, (kp_off[vs] if V else 0) + kp, len(xy) - 1)
        self.px, self.py = xy[row, 0], xy[row, 1]
        ok &= np.isfinite(self.px) & np.isfinite(self.py)
        self.in_range = ok
        self.R = R[vs] if V else np.zeros((T, L, 9))
        self.c = c[vs] if V else np.zeros((T, L, 3))
        self.K = K[vs] if V else np.ones((T, L, 4))
        self.T, self.L, self.length, self.begin = T, L, length, tb[:-1]


def _eligibility(o):
    state = np.zeros((o.T, o.L), np.uint8)
    for k in range(o.L):
        ok = o.in_range[:, k].copy()
        for j in range(k):
            ok &= ~((state[:, j] == 1) & (o.view[:, j] == o.view[:, k]))
        state[:, k] = ok
    return state


def _midpoint(o, used):
    z = np.zeros(o.T)
    a00, a01, a02, a11, a12, a22, r0, r1, r2 = (z.copy() for _ in range(9))
    for k in range(o.L):
        u = used[:, k]
        R, c = o.R[:, k], o.c[:, k]
        fx, fy, cx, cy = (o.K[:, k, i] for i in range(4))
        x = (o.px[:, k] - cx) / fx
        y = (o.py[:, k] - cy) / fy
        n = np.sqrt((x * x + y * y) + 1.0)
        b0, b1, b2 = x / n, y / n, 1.0 / n
        d0 = (R[:, 0] * b0 + R[:, 3] * b1) + R[:, 6] * b2
        d1 = (R[:, 1] * b0 + R[:, 4] * b1) + R[:, 7] * b2
        d2 = (R[:, 2] * b0 + R[:, 5] * b1) + R[:, 8] * b2
        a00 = np.where(u, a00 + (1.0 - d0 * d0), a00)
        a11 = np.where(u, a11 + (1.0 - d1 * d1), a11)
        a22 = np.where(u, a22 + (1.0 - d2 * d2), a22)
        a01 = np.where(u, a01 + (-(d0 * d1)), a01)
        a02 = np.where(u, a02 + (-(d0 * d2)), a02)
        a12 = np.where(u, a12 + (-(d1 * d2)), a12)
        dc = (d0 * c[:, 0] + d1 * c[:, 1]) + d2 * c[:, 2]
        r0 = np.where(u, r0 + (c[:, 0] - d0 * dc), r0)
        r1 = np.where(u, r1 + (c[:, 1] - d1 * dc), r1)
        r2 = np.where(u, r2 + (c[:, 2] - d2 * dc), r2)
    det, x0, x1, x2 = solve_sym3(a00, a01, a02, a11, a12, a22, r0, r1, r2)
    m = used.sum(1).astype(np.float64)
    ok = (det > DET_REL * ((m * m) * m)) & (det < np.inf)
    return ok, np.stack([x0, x1, x2], 1)


def _evaluate(o, used, X):
    """-> dict(cost, max_e2, arg, nonpos, H [T,6] (00 01 02 11 12 22), g [T,3])."""
    T = o.T
    cost, max_e2 = np.zeros(T), np.full(T, -1.0)
    arg = np.zeros(T, np.int64)
    nonpos = np.zeros(T, bool)
    H, g = np.zeros((T, 6)), np.zeros((T, 3))
    for k in range(o.L):
        u = used[:, k]
        R, c = o.R[:, k], o.c[:, k]
        fx, fy, cx, cy = (o.K[:, k, i] for i in range(4))
        dx0, dx1, dx2 = X[:, 0] - c[:, 0], X[:, 1] - c[:, 1], X[:, 2] - c[:, 2]
        q0 = (R[:, 0] * dx0 + R[:, 1] * dx1) + R[:, 2] * dx2
        q1 = (R[:, 3] * dx0 + R[:, 4] * dx1) + R[:, 5] * dx2
        q2 = (R[:, 6] * dx0 + R[:, 7] * dx1) + R[:, 8] * dx2
        pos = q2 > 0.0
        a, b, iz = q0 / q2, q1 / q2, 1.0 / q2
        r0 = (fx * a + cx) - o.px[:, k]
        r1 = (fy * b + cy) - o.py[:, k]
        e2 = np.where(pos, r0 * r0 + r1 * r1, np.inf)
        sx, sy = fx * iz, fy * iz
        ju = [sx * (R[:, i] - a * R[:, 6 + i]) for i in range(3)]
        jv = [sy * (R[:, 3 + i] - b * R[:, 6 + i]) for i in range(3)]
        up = u & pos
        n = 0
        for i in range(3):
            for j in range(i, 3):
                H[:, n] = np.where(up, H[:, n] + (ju[i] * ju[j] + jv[i] * jv[j]), H[:, n])
                n += 1
            g[:, i] = np.where(up, g[:, i] + (ju[i] * r0 + jv[i] * r1), g[:, i])
        nonpos |= u & ~pos
        cost = np.where(u, cost + e2, cost)
        new = u & (e2 > max_e2)
        max_e2 = np.where(new, e2, max_e2)
        arg = np.where(new, k, arg)
    return dict(cost=cost, max_e2=max_e2, arg=arg, nonpos=nonpos, H=H, g=g)


def _select(mask, new, old):
    return {k: np.where(mask if new[k].ndim == 1 else mask[:, None], new[k], old[k]) for k in old}


def _fit(o, used, refine_iters):
    okdet, X = _midpoint(o, used)
    e = _evaluate(o, used, X)
    can = okdet & ~e["nonpos"]
    for _ in range(refine_iters):
        H, g = e["H"], e["g"]
        det, d0, d1, d2 = solve_sym3(H[:, 0], H[:, 1], H[:, 2], H[:, 3], H[:, 4], H[:, 5], g[:, 0], g[:, 1], g[:, 2])
        can = can & (det > 0.0) & (det < np.inf)
        Xn = np.stack([X[:, 0] - d0, X[:, 1] - d1, X[:, 2] - d2], 1)
        e1 = _evaluate(o, used, Xn)
        acc = can & ~e1["nonpos"] & (e1["cost"] < e["cost"])
        X = np.where(acc[:, None], Xn, X)
        e = _select(acc, e1, e)
        can = acc
    return okdet, X, e


def _wide_enough(o, used, X, cos_min):
    wide = np.zeros(o.T, bool)
    u = [[X[:, i] - o.c[:, k, i] for i in range(3)] for k in range(o.L)]
    nrm = [np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) for w in u]
    for k in range(o.L):
        for j in range(k):
            cosv = ((u[j][0] * u[k][0] + u[j][1] * u[k][1]) + u[j][2] * u[k][2]) / (nrm[j] * nrm[k])
            wide |= used[:, j] & used[:, k] & (cosv < cos_min)
    return wide


def triangulate(track_begin, members, views, min_views=2, refine_iters=3, thr_px=2.0, max_drops=2, min_angle_deg=1.5):
    """views: dict R [V,3,3], c [V,3], K [V,4] = fx fy cx cy, has_pose [V] or None, xy = list of V arrays n x 2.
    -> dict X [T,3], err_rms [T], n_used [T] u32, status [T] u8, obs_state [n_members] u8, counts [6] u32."""
    if min_views < 2 or not thr_px > 0:
        raise ValueError("min_views >= 2 and thr_px > 0 are required")
    cos_min = math.cos(math.radians(min_angle_deg))
    with np.errstate(all="ignore"):
        o = _Obs(track_begin, members, views)
        T = o.T
        state = _eligibility(o)
        n_used = (state == 1).sum(1)
        status = np.full(T, TOO_FEW, np.uint8)
        active = n_used >= min_views
        n_drop = np.zeros(T, np.int64)
        X = np.full((T, 3), np.nan)
        rms = np.full(T, np.nan)
        floor = max(2, min_views)
        rows = np.arange(T)
        for _ in range(max_drops + 1):
            if not active.any():
                break
            used = state == 1
            okdet, Xf, e = _fit(o, used, refine_iters)
            status[active & ~okdet] = DEGENERATE
            active = active & okdet
            err = np.sqrt(e["max_e2"])
            drop = active & (err > thr_px) & (n_used > floor) & (n_drop < max_drops)
            done = active & ~drop
            bad = done & ~(err <= thr_px)
            status[bad & e["nonpos"]] = BEHIND
            status[bad & ~e["nonpos"]] = REPROJ
            good = done & ~bad
            wide = _wide_enough(o, used, Xf, cos_min)
            status[good & wide] = OK
            status[good & ~wide] = LOW_PARALLAX
            X[good] = Xf[good]
            rms[done] = np.sqrt(e["cost"] / n_used.astype(np.float64))[done]
            state[rows[drop], e["arg"][drop]] = 2
            n_used = n_used - drop
            n_drop = n_drop + drop
            active = drop
        assert not active.any()
        obs_state = np.zeros(len(np.asarray(members)), np.uint8)
        obs_state[(o.begin[:, None] + np.arange(o.L)[None, :])[o.present]] = state[o.present]
    return dict(X=X, err_rms=rms, n_used=n_used.astype(np.uint32), status=status, obs_state=obs_state,
                counts=np.bincount(status, minlength=N_STATUS).astype(np.uint32))


def assert_same(got, want, what=""):
    """Two results of triangulate (or of the device call, as numpy) hold the same bits, NaNs in the same places."""
    for k in ("status", "n_used", "obs_state", "counts", "X", "err_rms"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, k)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, k, np.nonzero(~((a == b) | ((a != a) & (b != b))))[0][:8])


# ---- scenes -------------------------------------------------------------------------------------------------------
def _rodrigues(w):
    th = np.linalg.norm(w, axis=1)
    k = w / np.maximum(th, 1e-300)[:, None]
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def pack(view, keypoint):
    return (np.asarray(view, np.uint64) << np.uint64(32)) | np.asarray(keypoint, np.uint64)


def project(R, c, K, X):
    q = R.reshape(3, 3) @ (np.asarray(X, float) - c)
    return np.array([K[0] * q[0] / q[2] + K[2], K[1] * q[1] / q[2] + K[3]])


def make_scene(V=12, T=60, seed=0, noise_px=0.5, outlier_every=5, outlier_px=47.0, min_len=4, max_len=8, n_outliers=1,
               pixel_dtype=np.float32, cameras=None):
    """Ground-truth scene: V cameras (f = 1000, 2000 x 2000 px) scattered in a 6 x 6 x 1 box, turned by up to ~6 degrees,
    looking down +z at points of depth 6..12; track t sees len_t distinct views (len_t cycles through min_len..max_len);
    every outlier_every-th track (t % outlier_every == 0; 0 = none) has n_outliers observations displaced by outlier_px.
    cameras: a `views` dict whose first V cameras observe the tracks instead of new ones; the returned views are
    that dict with the new keypoints appended.
    -> dict track_begin, members, views, X_gt, planted [n_members] bool, size (the far depth, 12)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (V, 3)) * np.array([3.0, 3.0, 0.5])
    R = _rodrigues(rng.standard_normal((V, 3)) * np.deg2rad(3.0))
    K = np.tile(np.array([1000.0, 1000.0, 1000.0, 1000.0]), (V, 1))
    has = np.ones(V, bool)
    xy = [[] for _ in range(V)]
    if cameras is not None:
        R, c, K = np.asarray(cameras["R"]).reshape(-1, 3, 3), np.asarray(cameras["c"]), np.asarray(cameras["K"])
        has = np.asarray(cameras["has_pose"], bool)
        xy = [np.asarray(a, np.float64).reshape(-1, 2).tolist() for a in cameras["xy"]]
    X_gt = np.stack([rng.uniform(-2, 2, T), rng.uniform(-2, 2, T), rng.uniform(6, 12, T)], 1)
    begin, mem, planted = [0], [], []
    for t in range(T):
        n = min(min_len + t % (max_len - min_len + 1), V)
        vs = rng.choice(V, size=n, replace=False)
        bad = set(rng.choice(n, size=n_outliers, replace=False).tolist()) if outlier_every and t % outlier_every == 0 else set()
        for i, v in enumerate(vs):
            p = project(R[v], c[v], K[v], X_gt[t]) + rng.standard_normal(2) * noise_px
            if i in bad:
                ang = rng.uniform(0, 2 * np.pi)
                p = p + outlier_px * np.array([np.cos(ang), np.sin(ang)])
            mem.append(pack(v, len(xy[v])))
            xy[v].append(p)
            planted.append(i in bad)
        begin.append(len(mem))
    views = dict(R=R, c=c, K=K, has_pose=has,
                 xy=[np.asarray(a, np.float64).reshape(-1, 2).astype(pixel_dtype) for a in xy])
    return dict(track_begin=np.array(begin, np.uint32), members=np.array(mem, np.uint64), views=views, X_gt=X_gt,
                planted=np.array(planted, bool), size=12.0)


def constructed_tracks(scene, max_drops=2):
    """One track per status and boundary rule, appended views included.  -> (problem dict like make_scene's, with
    `expect`: list of (name, status, obs_state list or None) per track)."""
    v0 = scene["views"]
    V = len(v0["c"])
    K1 = np.array([1000.0, 1000.0, 1000.0, 1000.0])
    eye = np.eye(3)
    flip = np.diag([-1.0, 1.0, -1.0])  # half a turn about y: looks down -z
    # appended views: V no pose; V+1, V+2 coincident; V+3, V+4 baseline 0.01; V+5 at (1, 0, 0) looking backwards
    R = np.concatenate([np.asarray(v0["R"]).reshape(V, 3, 3), np.stack([eye, eye, eye, eye, eye, flip])])
    c = np.concatenate([v0["c"], np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 0], [0, 0, 0], [0.01, 0, 0], [1.0, 0, 0]])])
    K = np.concatenate([v0["K"], np.tile(K1, (6, 1))])
    has = np.concatenate([np.asarray(v0["has_pose"], bool), [False, True, True, True, True, True]])
    xy = [np.asarray(a, np.float32).reshape(-1, 2).tolist() for a in v0["xy"]] + [[] for _ in range(6)]
    begin, mem, expect = [0], [], []

    def obs(v, p):
        xy[v].append([float(p[0]), float(p[1])])
        return pack(v, len(xy[v]) - 1)

    def see(v, X, shift=(0.0, 0.0)):
        return obs(v, project(R[v], c[v], K[v], X) + np.asarray(shift))

    def track(name, status, states, members):
        mem.extend(members)
        begin.append(len(mem))
        expect.append((name, status, states))

    P = np.array([0.3, -0.2, 8.0])
    track("empty", TOO_FEW, [], [])
    track("one view", TOO_FEW, [1], [see(0, P)])
    track("repeated view", OK, [1, 0, 1, 1], [see(0, P), see(0, P, (30.0, 0.0)), see(1, P), see(2, P)])
    track("no pose", OK, [0, 1, 1], [obs(V, (900.0, 900.0)), see(1, P), see(2, P)])
    track("keypoint out of range", OK, [0, 1, 1], [pack(1, 10 ** 6), see(2, P), see(3, P)])
    track("view out of range", OK, [0, 1, 1], [pack(V + 6, 0), see(2, P), see(3, P)])
    track("non-finite pixel", OK, [0, 1, 1], [obs(1, (np.nan, 5.0)), see(2, P), see(3, P)])
    track("only repeats", TOO_FEW, [1, 0, 0], [see(4, P), see(4, P), see(4, P)])
    track("behind", BEHIND, [1, 1], [see(V + 3, [0.5, 0.0, 5.0]), see(V + 5, [0.5, 0.0, 5.0])])
    track("two gross errors", REPROJ, [1, 1], [see(0, P, (60.0, 80.0)), see(1, P, (-70.0, -90.0))])
    track("low parallax", LOW_PARALLAX, [1, 1], [see(V + 3, [0.1, 0.2, 10.0]), see(V + 4, [0.1, 0.2, 10.0])])
    track("identical rays", DEGENERATE, [1, 1], [obs(V + 1, (1000.0, 1000.0)), obs(V + 2, (1000.0, 1000.0))])
    n = min(V, 8)
    shifts = [(47.0, 0.0), (0.0, -47.0), (-33.0, 33.0)] + [(0.0, 0.0)] * n
    track("max_drops + 1 outliers", REPROJ, None, [see(v, P, shifts[v] if v < max_drops + 1 else (0.0, 0.0)) for v in range(n)])
    # a 70-member track: every posed view of the scene's first min(V, 70), then repeats (state 0)
    first = min(V, 70)
    track("70 members", OK, [1] * first + [0] * (70 - first), [see(k % first, P) for k in range(70)])
    views = dict(R=R, c=c, K=K, has_pose=has, xy=[np.asarray(a, np.float32).reshape(-1, 2) for a in xy])
    return dict(track_begin=np.array(begin, np.uint32), members=np.array(mem, np.uint64), views=views, expect=expect)


def concatenate(a, b, views):
    """Tracks of a, then tracks of b, over `views` (which hold the keypoints of both)."""
    return dict(track_begin=np.concatenate([a["track_begin"], b["track_begin"][1:] + a["track_begin"][-1]]).astype(np.uint32),
                members=np.concatenate([a["members"], b["members"]]), views=views)
