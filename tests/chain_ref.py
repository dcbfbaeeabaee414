"""chain_ref.py -- scene, alignment helpers and CPU leg of tests/test_chain.py (test infrastructure, NOT product code).

One small feature-level scene goes through the whole chain: descriptor matching -> createCorrespondenceMatrix ->
estimatePose -> rotation averaging -> translation averaging -> tracklets -> triangulation -> bundle adjustment.
reference_chain() runs it through the CPU oracle and the CPU specifications only; tests/test_chain.py runs it through the
Python engine and checks every hand-off against the specification of the next stage.

The scene (make_scene): 13 views.
  * MAIN, ten views of one synthetic.make_feature_views scene (general 3-D camera positions, pixel noise, descriptors,
    clutter, point_id ground truth).  They do NOT have the smallest ids: view 0 belongs to the second component, so the
    first posed view, the root of the solved component and the gauge view of the bundle adjustment are all view 1.
  * SECOND, two views (ids 0 and 12) of another point set, candidates only with each other: a second component.
  * CLUTTER, one view (id 6) of unmatched keypoints only; the candidate pairs that touch it yield no edge.
Candidate pairs: every pair inside MAIN, the one pair of SECOND, three pairs that touch CLUTTER; sorted by (src, dst).

has_pose: the views of the largest connected component of the OK edges (ties: the component with the
smallest view id); the library has no call for it.
"""
import functools
import os
import sys

import numpy as np

import bundle_focal_spec as BF
import bundle_spec as B
import cycle_spec as CS
import oracle_lib as O
import transavg_spec as TA
import triangulate_spec as TR
from pyposegraphbuilder import synthetic as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rotavg_oracle as RO  # noqa: E402
import tracklets_oracle as TO  # noqa: E402

SCENE_SEED = 3            # chosen so that test_reference_conditions holds; another seed if a condition fails, never a weaker one
N_VIEWS = 13
MAIN = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11)
SECOND = (0, 12)
CLUTTER = 6
CLUTTER_PAIRS = ((2, 6), (6, 9), (0, 6))
N_POINTS, N_POINTS_SECOND, N_CLUTTER = 130, 90, 60
DESC_NOISE = 0.055         # descriptor noise at which a few false matches pass the ratio test (and one survives a mask)
THR_PX = 0.75             # estimatePose's pixel threshold
ESTIMATOR_SEED = 17


# ---- scene ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_scene(seed=SCENE_SEED):
    """-> dict views [V] of dict(xy, desc, point_id), cam (f, w, h), pairs [(src, dst)], R_gt [V,3,3] world->camera,
    c_gt [V,3] centres (the two components have unrelated world frames; CLUTTER has none: identity and 0), X_gt [points,3]
    (row = point_id), main [V] bool."""
    rng = np.random.default_rng(seed)
    mv, mp, cam, X_main = S.make_feature_views(rng, n_views=len(MAIN), n_points=N_POINTS, n_clutter=N_CLUTTER, desc_noise=DESC_NOISE,
                                               with_points=True)
    sv, sp, _, X_second = S.make_feature_views(rng, n_views=2, n_points=N_POINTS_SECOND, n_clutter=N_CLUTTER, desc_noise=DESC_NOISE,
                                               with_points=True)
    for v in sv:   # the second scene's points follow the first's in X_gt
        v["point_id"] = np.where(v["point_id"] >= 0, v["point_id"] + N_POINTS, -1)
    f, w, h = cam
    n = 3 * N_CLUTTER
    d = np.abs(rng.standard_normal((n, 128))).astype(np.float32)
    clutter = dict(xy=np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(np.float32),
                   desc=(d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), point_id=-np.ones(n, np.int64))
    views = [None] * N_VIEWS
    R_gt = np.tile(np.eye(3), (N_VIEWS, 1, 1))
    c_gt = np.zeros((N_VIEWS, 3))
    for ids, vs, ps in ((MAIN, mv, mp), (SECOND, sv, sp)):
        for i, v, (R, t) in zip(ids, vs, ps):
            views[i], R_gt[i], c_gt[i] = v, R, -R.T @ t
    views[CLUTTER] = clutter
    pairs = [(a, b) for k, a in enumerate(MAIN) for b in MAIN[k + 1:]] + [SECOND] + list(CLUTTER_PAIRS)
    main = np.zeros(N_VIEWS, bool)
    main[list(MAIN)] = True
    for a in (R_gt, c_gt, X_main, X_second, main):
        a.setflags(write=False)
    return dict(views=views, cam=cam, pairs=sorted(pairs), R_gt=R_gt, c_gt=c_gt, X_gt=np.concatenate([X_main, X_second]), main=main)


def camera_K(cam, n_views=N_VIEWS, focal=None):
    """K rows (fx, fy, cx, cy).  focal: None = the camera's f for every view; [n_views] = the per-view form."""
    f, w, h = cam
    K = np.tile(np.array([f, f, w / 2.0, h / 2.0]), (n_views, 1))
    if focal is not None:
        K[:, 0] = K[:, 1] = np.asarray(focal, np.float64)
    return K


# ---- small helpers shared by both legs --------------------------------------------------------------------------------------
def largest_component(n_views, src, dst):
    """has_pose: membership of the largest connected component of the edges (src, dst); ties go to the component with the
    smallest view id.  A view without an edge is a component of its own."""
    parent = list(range(n_views))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(src, dst):
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(v) for v in range(n_views)])
    size = np.bincount(root, minlength=n_views)
    return root == int(np.argmax(size))     # argmax: the first (smallest root id) among the largest


def tracks_to_arrays(tracks):
    """[[(view, keypoint)]] -> (track_begin u32 [T + 1], members u64)."""
    tb = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32)
    mem = np.array([TR.pack(v, k) for t in tracks for v, k in t], np.uint64)
    return tb, mem


def track_point_ids(scene, tracks):
    """-> (majority point id per track (-1: clutter or no majority possible), pure [T] bool: at least two members, all of
    one point id >= 0)."""
    maj, pure = np.full(len(tracks), -1, np.int64), np.zeros(len(tracks), bool)
    for i, t in enumerate(tracks):
        ids = np.array([scene["views"][v]["point_id"][k] for v, k in t], np.int64)
        if not len(ids):
            continue
        vals, cnt = np.unique(ids, return_counts=True)
        maj[i] = vals[np.argmax(cnt)]
        pure[i] = len(ids) >= 2 and len(vals) == 1 and vals[0] >= 0
    return maj, pure


def purity(scene, tracks):
    """The share of the tracks of length >= 2 whose members all carry one point id."""
    _, pure = track_point_ids(scene, tracks)
    long_ = np.array([len(t) >= 2 for t in tracks])
    return float(pure[long_].mean())


def mask_members(pairs, ok, matches, masks):
    """The (view, keypoint) of every row whose mask bit is set in a call of an OK pair."""
    allowed = set()
    for p, (s, d) in enumerate(pairs):
        if not ok[p]:
            continue
        ms, md = matches[p]
        for a, b, m in zip(ms.tolist(), md.tolist(), np.asarray(masks[p]).tolist()):
            if m:
                allowed.add((s, a))
                allowed.add((d, b))
    return allowed


# ---- alignment with the ground truth -----------------------------------------------------------------------------------------
def umeyama(c, c_gt):
    """The similarity (s, Q, t) with c_gt ~ s Q c + t in the least-squares sense (Umeyama 1991)."""
    mu, mg = c.mean(0), c_gt.mean(0)
    a, b = c - mu, c_gt - mg
    U, Sv, Vt = np.linalg.svd(b.T @ a)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    s = float((Sv * np.diag(D)).sum() / (a ** 2).sum())
    return s, Q, mg - s * Q @ mu


def ground_truth_errors(scene, R, c, X, status, tracks):
    """One similarity from the MAIN centres, applied to the points as well.  -> dict rot_deg (mean over MAIN of the angle of
    R Q^T R_gt^T), centre (RMS |s Q c + t - c_gt| over MAIN), point (median |s Q X + t - X_gt[majority point id]| over the
    OK tracks whose majority id is a point), in the units of the ground truth (depths 4..8)."""
    m = scene["main"]
    R, c, X = np.asarray(R, float).reshape(-1, 3, 3), np.asarray(c, float), np.asarray(X, float)
    s, Q, t = umeyama(c[m], scene["c_gt"][m])
    rot = [S.rot_err_deg(R[v] @ Q.T, scene["R_gt"][v]) for v in np.nonzero(m)[0]]
    centre = np.sqrt((((s * (Q @ c[m].T)).T + t - scene["c_gt"][m]) ** 2).sum(1).mean())
    maj, _ = track_point_ids(scene, tracks)
    use = (np.asarray(status) == TR.OK) & (maj >= 0)
    pt = np.linalg.norm((s * (Q @ X[use].T)).T + t - scene["X_gt"][maj[use]], axis=1)
    return dict(rot_deg=float(np.mean(rot)), centre=float(centre), point=float(np.median(pt)), n_points=int(use.sum()))


def direction_cosines(scene, R, src, dst, t):
    """cos of the angle between the world direction R_dst^T t of the edges (src, dst) inside MAIN and c_gt[src] - c_gt[dst],
    the rotations' gauge removed by the rotation-only alignment of the MAIN root (R_root = I in both): MAIN's first view has
    R_gt = I, so the averaged world frame is the ground truth's up to the averaging error."""
    src, dst = np.asarray(src, int), np.asarray(dst, int)
    keep = scene["main"][src] & scene["main"][dst]
    g = TA.directions_from_edges(R, src[keep], dst[keep], np.asarray(t)[keep])
    want = scene["c_gt"][src[keep]] - scene["c_gt"][dst[keep]]
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    return (g * want).sum(1)


# ---- the CPU leg ------------------------------------------------------------------------------------------------------------------
def oracle_edges(scene, focal=None):
    """Oracle matcher -> createCorrespondenceMatrix -> oracle estimator on every candidate pair.  focal: None = the camera's
    f for every view, [V] = the focal every stage is told per view.
    -> dict matches [(src idx, dst idx)], rows [P], edges (structured), masks [per pair], ok [P]."""
    views, cam, pairs = scene["views"], scene["cam"], scene["pairs"]
    cams = [cam] * len(views) if focal is None else [(float(f), cam[1], cam[2]) for f in focal]
    matches, corr, thr = [], [], np.zeros(len(pairs))
    for p, (s, d) in enumerate(pairs):
        oi, oj, _ = O.match_descriptors(views[s]["desc"], views[d]["desc"])
        matches.append((oi.copy(), oj.copy()))
        c, thr[p] = O.ref_normalize_corr(views[s]["xy"], views[d]["xy"], oi, oj, cams[s], cams[d], False, THR_PX)
        corr.append(c.astype(np.float32))
    rows = np.array([len(c) for c in corr], np.int64)
    off = np.zeros(len(pairs) + 1, np.uint64)
    off[1:] = np.cumsum(rows)
    cat = np.concatenate(corr)
    e, m = O.estimate_pose_batch(cat[:, 0].copy(), cat[:, 1].copy(), cat[:, 2].copy(), cat[:, 3].copy(), off, thr, O.default_params(),
                                 ESTIMATOR_SEED)
    masks = [m[int(off[p]):int(off[p + 1])] for p in range(len(pairs))]
    return dict(matches=matches, rows=rows, edges=e, masks=masks, ok=e["status"] == 1, corr=corr, thr=thr)


def ok_graph(scene, edges, rows, ok):
    """The OK records as (src, dst, R_rel [E,3,3], t [E,3], weight = n_inl / rows)."""
    pr = np.array(scene["pairs"], np.int64)
    return (pr[ok, 0], pr[ok, 1], edges["R"][ok].reshape(-1, 3, 3), edges["t"][ok],
            edges["n_inl"][ok].astype(np.float64) / np.asarray(rows)[ok].astype(np.float64))


def spec_views(scene, R, c, has_pose, focal=None):
    return dict(R=np.asarray(R, float).reshape(-1, 3, 3), c=np.asarray(c, float), K=camera_K(scene["cam"], focal=focal), has_pose=np.asarray(has_pose, bool),
                xy=[v["xy"] for v in scene["views"]])


@functools.lru_cache(maxsize=None)
def reference_chain(seed=SCENE_SEED):
    """The whole chain through the oracle and the specifications.  -> dict of every stage's result."""
    scene = make_scene(seed)
    est = oracle_edges(scene)
    src, dst, Rrel, t, w = ok_graph(scene, est["edges"], est["rows"], est["ok"])
    R, rot_iters = RO.rotation_average(N_VIEWS, src, dst, Rrel, w)
    gamma = TA.directions_from_edges(R, src, dst, t)
    c, trn_iters = TA.translation_average(N_VIEWS, src, dst, gamma, w)
    store = TO.Tracklets()
    for p, (s, d) in enumerate(scene["pairs"]):
        if est["ok"][p]:
            store.add(s, d, list(zip(est["matches"][p][0].tolist(), est["matches"][p][1].tolist())), est["masks"][p].tolist())
    tracks = [list(tr) for tr in store.tracks]
    has_pose = largest_component(N_VIEWS, src, dst)
    views = spec_views(scene, R, c, has_pose)
    tb, mem = tracks_to_arrays(tracks)
    tri = TR.triangulate(tb, mem, views)
    trace = []
    ba = B.bundle_adjust(tb, mem, views, tri["X"], tri["status"], tri["obs_state"], trace=trace)
    return dict(scene=scene, est=est, graph=(src, dst, Rrel, t, w), R=R, rot_iters=rot_iters, gamma=gamma, c=c, trn_iters=trn_iters,
                tracks=tracks, has_pose=has_pose, views=views, track_begin=tb, members=mem, tri=tri, ba=ba, ba_trace=trace)


def reference_figures(ref):
    """The figures against ground truth that the bounds of tests/test_chain.py are taken from."""
    scene = ref["scene"]
    src, dst, _, t, _ = ref["graph"]
    cos = direction_cosines(scene, ref["R"], src, dst, t)
    before = ground_truth_errors(scene, ref["R"], ref["c"], ref["tri"]["X"], ref["tri"]["status"], ref["tracks"])
    after = ground_truth_errors(scene, ref["ba"]["R"], ref["ba"]["c"], ref["ba"]["X"], ref["tri"]["status"], ref["tracks"])
    return dict(min_cos=float(cos.min()), before=before, after=after, purity=purity(scene, ref["tracks"]))


# ---- the filtered chain: estimated wrong edges and wrong nominal focals (tests/test_chain_filtered.py) ------------------------
# The base scene stays make_scene(SCENE_SEED); FILTERED_DRAW numbers the draw of twin pairs, twin points and focal errors on top
# of it.  FOCAL_ERR is a ladder, not a measurement: 0.03, then 0.02, then 0.01.  Draws 0..7 were tried at each rung against
# tests/test_chain_filtered.py::test_reference_filtered_conditions, on the reference alone:
#   0.03: draws 0, 1, 2, 5 -- the filter at defaults also drops a TRUE edge ((7, 10), (1, 3) or (3, 8)): with focals that are 3 %
#         off, none of the eight triangles of such an edge closes within 5 / 15 degrees.  Draws 3, 4, 6, 7 pass the filter, but the
#         default triangulation (thr_px = 2) refuses half of the tracks under those focals, so that 2 to 4 MAIN views have fewer
#         than min_focal_obs = 30 observations and view 1 or 3 fewer than min_cam_obs = 8; where that happens the focal run moves
#         the rotations from 0.6 to 5..8 degrees (draws 3, 6, 7).
#   0.02: the filter still drops (7, 10) on draws 0, 1, 2, 6; no other draw has all ten focals free.
#   0.01: draws 2..7 meet every input condition.  Draw 2's focal run worsens the median point error (0.088 -> 0.102), which
#         test_reference_filtered_chain does not allow; draw 3 is the first that meets the conditions and the relations.
FOCAL_ERR = 0.01
FILTERED_DRAW = 3
N_TWIN_PAIRS = 3
N_TWIN = 150              # twin rows per pair: the estimator must prefer the twin model to the ~70 true rows
TWIN_ROT_DEG = (15.0, 25.0)
TWIN_ID_BASE = -2         # point_id of pair k's twin keypoints: TWIN_ID_BASE - k
PX_NOISE = 0.3            # synthetic.make_feature_views' default, which make_scene uses


def _unit_desc(x):
    x = np.abs(x).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_filtered_scene(seed=SCENE_SEED, draw=FILTERED_DRAW, n_twin=N_TWIN, focal_err=FOCAL_ERR):
    """make_scene(seed) with two changes (the base scene's arrays are copied, never written):
      * twin structure on N_TWIN_PAIRS view-disjoint candidate pairs (a, b) of MAIN that avoid the gauge view: n_twin fresh
        points Z seen by a through its true pose, T(Z) seen by b through its true pose, T a rotation of 15..25 degrees about
        the centre of the scene's volume plus a small shift -- consistent with ONE wrong relative pose R_b R_T R_a^T.
      * f_nominal [V] = f_true (1 + e_v), e_v uniform in +-focal_err on MAIN and 0 elsewhere; the pixels are the true focal's.
    -> the scene dict plus f_true, f_nominal [V], focal_e [V], twin_pairs [(a, b)], twin_R [k,3,3]."""
    base = make_scene(seed)
    rng = np.random.default_rng([seed, 0x7F11, draw])
    f, w, h = base["cam"]
    views = [dict(xy=v["xy"].copy(), desc=v["desc"].copy(), point_id=np.asarray(v["point_id"], np.int64).copy()) for v in base["views"]]
    free = rng.permutation([v for v in MAIN if v != MAIN[0]])[:2 * N_TWIN_PAIRS]
    twin_pairs = sorted(tuple(sorted((int(free[2 * k]), int(free[2 * k + 1])))) for k in range(N_TWIN_PAIRS))
    centre = np.array([0.0, 0.0, 6.0])
    twin_R = []

    def project(v, Y):
        Yc = (Y - base["c_gt"][v]) @ base["R_gt"][v].T
        px = np.stack([f * Yc[:, 0] / Yc[:, 2] + w / 2, f * Yc[:, 1] / Yc[:, 2] + h / 2], 1)
        return px, (Yc[:, 2] > 0.5) & (px[:, 0] > 0) & (px[:, 0] < w) & (px[:, 1] > 0) & (px[:, 1] < h)
    for k, (a, b) in enumerate(twin_pairs):
        ax = rng.standard_normal(3)
        RT = S.rodrigues(ax / np.linalg.norm(ax), np.radians(rng.uniform(*TWIN_ROT_DEG)))
        shift = rng.uniform(-0.2, 0.2, 3)
        Z = np.stack([rng.uniform(-2, 2, 4 * n_twin), rng.uniform(-1.5, 1.5, 4 * n_twin), rng.uniform(4, 8, 4 * n_twin)], 1)
        pa, va = project(a, Z)
        pb, vb = project(b, (Z - centre) @ RT.T + centre + shift)
        sel = np.nonzero(va & vb)[0][:n_twin]
        assert len(sel) == n_twin
        D = _unit_desc(rng.standard_normal((n_twin, 128)))
        noise = PX_NOISE * rng.standard_normal((n_twin, 2))          # the same pixel noise in both views
        for v, px in ((a, pa), (b, pb)):
            views[v]["xy"] = np.concatenate([views[v]["xy"], (px[sel] + noise).astype(np.float32)])
            views[v]["desc"] = np.concatenate([views[v]["desc"], _unit_desc(D + DESC_NOISE * rng.standard_normal((n_twin, 128)))])
            views[v]["point_id"] = np.concatenate([views[v]["point_id"], np.full(n_twin, TWIN_ID_BASE - k, np.int64)])
        twin_R.append(RT)
    e = np.zeros(N_VIEWS)
    e[list(MAIN)] = rng.uniform(-focal_err, focal_err, len(MAIN))
    f_nominal = f * (1.0 + e)
    twin_R = np.array(twin_R)
    for a in (e, f_nominal, twin_R):
        a.setflags(write=False)
    return dict(base, views=views, f_true=float(f), f_nominal=f_nominal, focal_e=e, twin_pairs=twin_pairs, twin_R=twin_R)


def true_relative_rotation(scene, s, d):
    return scene["R_gt"][d] @ scene["R_gt"][s].T


def twin_rows(scene, p, matches):
    """bool per match row of pair p: both keypoints are twin keypoints."""
    s, d = scene["pairs"][p]
    ms, md = matches
    return (scene["views"][s]["point_id"][np.asarray(ms, np.int64)] <= TWIN_ID_BASE) & \
           (scene["views"][d]["point_id"][np.asarray(md, np.int64)] <= TWIN_ID_BASE)


def has_twin_member(scene, tracks):
    return [(v, k) for t in tracks for v, k in t if scene["views"][v]["point_id"][k] <= TWIN_ID_BASE]


def focal_rms(scene, phi):
    """RMS over MAIN of |phi f_nominal - f_true| / f_true."""
    m = scene["main"]
    return float(np.sqrt((((np.asarray(phi, float) * scene["f_nominal"] - scene["f_true"])[m] / scene["f_true"]) ** 2).mean()))


def run_leg(scene, est, use):
    """Steps 3..9 of the chain on the records `use` [P] bool (the kept ones, or every OK one): averaging, tracklets of
    those pairs only, has_pose of those edges, triangulation, focal bundle adjustment, K scaled by phi, triangulation again,
    pose-only bundle adjustment.  -> dict of every stage's result."""
    src, dst, Rrel, t, w = ok_graph(scene, est["edges"], est["rows"], use)
    R, rot_iters = RO.rotation_average(N_VIEWS, src, dst, Rrel, w)
    gamma = TA.directions_from_edges(R, src, dst, t)
    c, trn_iters = TA.translation_average(N_VIEWS, src, dst, gamma, w)
    store = TO.Tracklets()
    for p, (s, d) in enumerate(scene["pairs"]):
        if use[p]:
            store.add(s, d, list(zip(est["matches"][p][0].tolist(), est["matches"][p][1].tolist())), est["masks"][p].tolist())
    tracks = [list(tr) for tr in store.tracks]
    has_pose = largest_component(N_VIEWS, src, dst)
    views = spec_views(scene, R, c, has_pose, scene["f_nominal"])
    tb, mem = tracks_to_arrays(tracks)
    tri = TR.triangulate(tb, mem, views)
    trace = []
    baf = BF.bundle_adjust(tb, mem, views, tri["X"], tri["status"], tri["obs_state"], trace=trace)
    views2 = dict(views, R=baf["R"], c=baf["c"], K=BF.scaled_K(views["K"], baf["phi"]))
    tri2 = TR.triangulate(tb, mem, views2)
    ba2 = B.bundle_adjust(tb, mem, views2, tri2["X"], tri2["status"], tri2["obs_state"])
    return dict(graph=(src, dst, Rrel, t, w), R=R, rot_iters=rot_iters, gamma=gamma, c=c, trn_iters=trn_iters, tracks=tracks,
                has_pose=has_pose, views=views, track_begin=tb, members=mem, tri=tri, baf=baf, baf_trace=trace, views2=views2,
                tri2=tri2, ba2=ba2)


def leg_figures(scene, leg):
    """Against ground truth at the three stations: before the focal run, after it, after re-triangulation + pose-only run."""
    tri, baf, tri2, ba2, tracks = leg["tri"], leg["baf"], leg["tri2"], leg["ba2"], leg["tracks"]
    return dict(before=ground_truth_errors(scene, leg["R"], leg["c"], tri["X"], tri["status"], tracks),
                focal=ground_truth_errors(scene, baf["R"], baf["c"], baf["X"], tri["status"], tracks),
                final=ground_truth_errors(scene, ba2["R"], ba2["c"], ba2["X"], tri2["status"], tracks),
                focal_before=focal_rms(scene, np.ones(N_VIEWS)), focal_after=focal_rms(scene, baf["phi"]),
                purity=purity(scene, tracks))


@functools.lru_cache(maxsize=None)
def reference_filtered_chain(seed=SCENE_SEED, draw=FILTERED_DRAW, n_twin=N_TWIN, focal_err=FOCAL_ERR):
    """The filtered chain through the oracle and the specifications, and a second copy without the filter.
    -> dict scene, est, cyc (cycle_spec.cycle_filter with details), kept [P] bool, filtered (run_leg), unfiltered (run_leg)."""
    scene = make_filtered_scene(seed, draw, n_twin, focal_err)
    est = oracle_edges(scene, scene["f_nominal"])
    pr = np.array(scene["pairs"], np.int64)
    cyc = CS.cycle_filter(N_VIEWS, pr[:, 0], pr[:, 1], est["edges"]["R"].reshape(-1, 3, 3), est["edges"]["t"], est["edges"]["status"], details=True)
    kept = cyc["keep"].astype(bool)
    return dict(scene=scene, est=est, cyc=cyc, kept=kept, filtered=run_leg(scene, est, kept), unfiltered=run_leg(scene, est, est["ok"]))
