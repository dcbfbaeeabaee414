"""cycle_spec.py -- the cycle-consistency edge filter, written down in numpy f64 (test infrastructure, NOT product code).

This file is the definition of pgi_cycle_filter / pgi_cycle_filter_edges (include/pgi.h).

Input: n_views and P pairs (src[p], dst[p]) with a record R (3 x 3, R_dst_src), unit t (t_dst_src) and status each;
x_dst = R x_src + t.  Only records with status == EDGE_OK take part.  Among them an unordered view pair occurs at most
once and src != dst (ValueError otherwise, the library's PGI_ERR_INVALID).

A triangle is three views a < b < c with an OK record on each of the three unordered pairs, in either orientation.  From
each record the pose is taken in the direction needed -- as stored (R, t) or inverted (R^T, -R^T t) -- which gives
b<-a, c<-b and a<-c.

  rotation      L = R_ac R_cb R_ba; passes when trace(L) >= 1 + 2 cos(rot_thr).  No acos is taken.
  translation   in frame a: u1 = R_ba^T t_ba (direction of c_a - c_b), u2 = R_ba^T (R_cb^T t_cb) (c_b - c_c), u3 = t_ac
                (c_c - c_a), n = u1 x u2.  |n|^2 < sin^2(collinear_thr): the centres are nearly collinear, the test is
                skipped.  Otherwise it passes when (u3 . n)^2 <= sin^2(trn_thr) |n|^2, (u2 x u3) . n > 0 and
                (u3 x u1) . n > 0 (coplanar, and s1 u1 + s2 u2 + s3 u3 = 0 has positive scales).

A triangle is good when it passes every test applied to it.  Per pair: n_tri triangles contain it, n_good of them good
(both 0 for a record that is not OK).  keep = OK and (n_good >= min_good or (n_tri == 0 and keep_untested)).

Every sum has a fixed order (three-term sums as (x0 + x1) + x2, no fused multiply-add), so that the library can follow it
operation by operation; the results compared are integers.
"""
import math

import numpy as np

EDGE_OK = 1
EDGE_INCONSISTENT = -4

DEFAULTS = dict(rot_thr_deg=5.0, trn_thr_deg=15.0, collinear_thr_deg=5.0, min_good=1, keep_untested=1)
SUMMARY_FIELDS = ("n_triangles", "n_good", "n_skipped_translation", "n_ok", "n_dropped")
MARGIN = 1e-9   # margins(): no tested quantity may lie this close (relative) to its threshold


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _matmul(A, B):
    C = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def _matvec(A, x):
    return np.array([(A[i, 0] * x[0] + A[i, 1] * x[1]) + A[i, 2] * x[2] for i in range(3)])


def directed_pose(R, t, invert):
    """The record's pose as stored, or inverted: (R^T, -(R^T t))."""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    if not invert:
        return R.copy(), t.copy()
    Rt = R.T.copy()
    return Rt, -_matvec(Rt, t)


def thresholds(prm):
    """-> (1 + 2 cos(rot_thr), sin^2(trn_thr), sin^2(collinear_thr))."""
    rad = math.pi / 180.0
    return (1.0 + 2.0 * math.cos(prm["rot_thr_deg"] * rad), math.sin(prm["trn_thr_deg"] * rad) ** 2,
            math.sin(prm["collinear_thr_deg"] * rad) ** 2)


def triangle_quantities(ba, cb, ac):
    """ba, cb, ac: (R, t) of b<-a, c<-b, a<-c.  -> dict trace, n2, un (u3 . n), o1 ((u2 x u3) . n), o2 ((u3 x u1) . n)."""
    (R_ba, t_ba), (R_cb, t_cb), (R_ac, t_ac) = ba, cb, ac
    L = _matmul(_matmul(R_ac, R_cb), R_ba)
    trace = (L[0, 0] + L[1, 1]) + L[2, 2]
    R_ab = R_ba.T
    u1 = _matvec(R_ab, t_ba)
    u2 = _matvec(R_ab, _matvec(R_cb.T, t_cb))
    u3 = t_ac
    n = _cross(u1, u2)
    return dict(trace=trace, n2=_dot(n, n), un=_dot(u3, n), o1=_dot(_cross(u2, u3), n), o2=_dot(_cross(u3, u1), n))


def judge(q, thr):
    """-> (good, skipped) of one triangle from its quantities and thresholds()."""
    rot_min, s2_trn, s2_col = thr
    good = q["trace"] >= rot_min
    skipped = q["n2"] < s2_col
    if not skipped:
        good = good and q["un"] * q["un"] <= s2_trn * q["n2"] and q["o1"] > 0.0 and q["o2"] > 0.0
    return bool(good), bool(skipped)


def _params(kw):
    prm = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in prm:
            raise TypeError("unknown parameter %r" % k)
        prm[k] = v
    for k in ("rot_thr_deg", "trn_thr_deg", "collinear_thr_deg"):
        if not (0.0 < prm[k] <= 90.0):
            raise ValueError("%s outside (0, 90] degrees" % k)
    if int(prm["min_good"]) == 0:
        raise ValueError("min_good must be at least 1")
    return prm


def triangles(n_views, src, dst, status):
    """-> (list of (a, b, c, p_ab, p_bc, p_ac), a < b < c, in lexicographic order; pair index of every unordered OK pair).
    Validates the pair list."""
    src, dst, status = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(status, np.int64)
    index, nbrs = {}, [set() for _ in range(n_views)]
    for p in np.nonzero(status == EDGE_OK)[0].tolist():
        s, d = int(src[p]), int(dst[p])
        if s >= n_views or d >= n_views or s < 0 or d < 0:
            raise ValueError("view id out of range")
        if s == d:
            raise ValueError("pair %d joins a view with itself" % p)
        key = (min(s, d), max(s, d))
        if key in index:
            raise ValueError("view pair %s occurs twice among the OK records" % (key,))
        index[key] = p
        nbrs[s].add(d)
        nbrs[d].add(s)
    tri = []
    for (a, b) in sorted(index):
        for c in sorted(nbrs[a] & nbrs[b]):
            if c > b:
                tri.append((a, b, c, index[(a, b)], index[(b, c)], index[(a, c)]))
    return tri, index


def evaluate(src, dst, R, t, tri):
    """The quantities of every triangle of triangles()."""
    src = np.asarray(src, np.int64)
    R, t = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
    out = []
    for a, b, c, pab, pbc, pac in tri:
        ba = directed_pose(R[pab], t[pab], src[pab] != a)
        cb = directed_pose(R[pbc], t[pbc], src[pbc] != b)
        ac = directed_pose(R[pac], t[pac], src[pac] != c)
        out.append(triangle_quantities(ba, cb, ac))
    return out


def cycle_filter(n_views, src, dst, R, t, status=None, details=False, **params):
    """-> dict keep [P] u8, n_tri [P] u32, n_good [P] u32, summary (dict of SUMMARY_FIELDS); with details also triangles
    (the list of triangles()), quantities (evaluate()), good and skipped (bool per triangle)."""
    prm = _params(params)
    P = len(src)
    status = np.full(P, EDGE_OK, np.int64) if status is None else np.asarray(status, np.int64)
    tri, _ = triangles(n_views, src, dst, status)
    qs = evaluate(src, dst, R, t, tri) if tri else []
    thr = thresholds(prm)
    n_tri, n_good = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    good, skipped = np.zeros(len(tri), bool), np.zeros(len(tri), bool)
    for k, (tr, q) in enumerate(zip(tri, qs)):
        good[k], skipped[k] = judge(q, thr)
        for p in tr[3:]:
            n_tri[p] += 1
            n_good[p] += int(good[k])
    ok = status == EDGE_OK
    keep = ok & ((n_good >= int(prm["min_good"])) | ((n_tri == 0) & bool(prm["keep_untested"])))
    summary = dict(n_triangles=len(tri), n_good=int(good.sum()), n_skipped_translation=int(skipped.sum()), n_ok=int(ok.sum()),
                   n_dropped=int((ok & ~keep).sum()))
    out = dict(keep=keep.astype(np.uint8), n_tri=n_tri, n_good=n_good, summary=summary)
    if details:
        out.update(triangles=tri, quantities=qs, good=good, skipped=skipped)
    return out


def filtered_status(status, keep):
    """The status column of the table the library writes: EDGE_INCONSISTENT on the OK records that were not kept."""
    status = np.asarray(status).copy()
    status[(status == EDGE_OK) & (np.asarray(keep) == 0)] = EDGE_INCONSISTENT
    return status


def margins(qs, **params):
    """The smallest relative distance of a tested quantity from its threshold over the triangles qs (inf without one).
    trace against 1 + 2 cos(rot_thr), relative to the threshold; |n|^2 against sin^2(collinear_thr), relative to it; where the
    translation test is applied, (u3 . n)^2 against sin^2(trn_thr) |n|^2, relative to that product, and the two orientation
    products against 0, relative to |n|^2 -- the size both have on a triangle that closes (|u x u'| is |n| over a side length
    ratio there)."""
    rot_min, s2_trn, s2_col = thresholds(_params(params))
    worst = math.inf
    for q in qs:
        m = [abs(q["trace"] - rot_min) / rot_min, abs(q["n2"] - s2_col) / s2_col]
        if not q["n2"] < s2_col:
            rhs = s2_trn * q["n2"]
            m += [abs(q["un"] * q["un"] - rhs) / rhs, abs(q["o1"]) / q["n2"], abs(q["o2"]) / q["n2"]]
        worst = min(worst, min(m))
    return worst


def loop_angles_deg(qs):
    """For reporting only: (loop rotation angle, coplanarity angle asin(|u3 . n| / |n|), NaN where |n| = 0) per triangle."""
    rot = np.array([math.degrees(math.acos(min(1.0, max(-1.0, (q["trace"] - 1.0) / 2.0)))) for q in qs])
    cop = np.array([math.degrees(math.asin(min(1.0, abs(q["un"]) / math.sqrt(q["n2"])))) if q["n2"] > 0 else math.nan for q in qs])
    return rot, cop
