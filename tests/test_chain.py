"""The chain from features to a refined reconstruction, seam by seam (scene and CPU leg: tests/chain_ref.py).

One small feature-level scene runs through the Python engine once (the module fixture `chain`): prepare_descriptors /
upload_keypoints -> match_descriptors_batch -> build_correspondences -> estimate_pose_batch -> rotation_average_edges ->
translation_average_edges -> DeviceTracklets.add_batch -> triangulate -> bundle_adjust.  At every seam the device's ACTUAL
upstream output goes to the CPU specification of the next stage and is compared with what the device's next stage
returned, under the bound that stage already has; seam 6 compares with the ground truth, seam 7 runs everything again.

The CPU leg (chain_ref.reference_chain: oracle matcher and estimator, then the specifications) gives the figures against
ground truth; scripts/chain_roundoff.py prints them together with the round-off figures of seams 2 and 5, all measured on
the reference alone.  Ground-truth bounds are TWICE the CPU leg's figure (that error is scene noise; a convention error
misses it by far more), round-off bounds TEN times the measured figure.

Measured on the CPU (scripts/chain_roundoff.py), seed 3: 46 OK edges, 719 tracks (680 OK, 37 TOO_FEW, 1 BEHIND,
1 LOW_PARALLAX), 164 dropped observations, purity 0.998609:
  min cos(R_dst^T t, c_src - c_dst) over the main component's edges   0.990079  (1 - cos = 9.921e-3)
  before bundle adjustment: rotation 0.8393 deg, centre 6.102e-3, median point 1.037e-1   (ground-truth units, depth 4..8)
  after  bundle adjustment: rotation 0.0673 deg, centre 1.176e-3, median point 3.432e-2
  seam 2: inner solves stopped at 1e-4 move the positions by 4.53e-6 of the RMS spread of the posed views (1e-6: 8.2e-8,
          1e-10: 1.5e-12); fixed steps, float64 leg by the kernel's formulas against longdouble: 3.7e-13 / 5.1e-13
  seam 5: float64 PCG leg against the direct solves at defaults: cost gap 5.47e-15, state distance 6.27e-8
Measured on the MI355X: seam 1 5.2e-8 rad; seam 2 identical bits through both entry points, positions 1.36e-5 of the RMS
spread, min cos 0.990079; seam 3 tracks equal, purity 0.998609; seam 4 identical bits (680 / 37 / 1 / 1, 163 dropped); seam 5
cost gap 5.6e-15, state distance 7.6e-8, cost 3963 -> 405 in 4 accepted steps; seam 6 before 0.832 deg / 6.05e-3 / 1.03e-1, after
0.068 deg / 1.19e-3 / 3.45e-2.  The device's edge table is the oracle's bit for bit, its rotations are the CPU leg's to 2e-14,
and yet its positions differ from the CPU leg's by up to 0.12 before the alignment: the translation averaging ends at its
iteration cap on this graph and the last bit of a direction picks the trajectory (transavg_spec.edge_model).  On identical
directions device and specification agree (seam 2); against ground truth both legs are equally good (seam 6).
"""
import os
import sys

import numpy as np
import pytest

import bundle_spec as B
import chain_ref as CR
import transavg_spec as TA
import triangulate_spec as TR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rotavg_oracle as RO  # noqa: E402
import tracklets_oracle as TO  # noqa: E402

V = CR.N_VIEWS

# ---- the CPU leg's figures (test_reference_chain demands that the leg still gives them) and the bounds taken from them ----
CPU_MIN_COS = 0.990079
CPU_BEFORE = dict(rot_deg=0.8393, centre=6.102e-3, point=1.037e-1)
CPU_AFTER = dict(rot_deg=0.0673, centre=1.176e-3, point=3.432e-2)
CPU_PURITY = 0.998609
GT_FACTOR = 2.0
ONE_MINUS_COS_BOUND = GT_FACTOR * (1.0 - CPU_MIN_COS)
# seam 1: the existing bound of tests/test_pose_graph_pipeline.py and tests/test_rotavg.py
ROT_HIP_VS_ORACLE_RAD = 1e-5
ROOT_IDENTITY_ATOL = 1e-12
# seam 2: the rule of tests/test_transavg.py (ten times the specification's sensitivity to inner solves stopped at 1e-4),
# re-measured on this graph: 4.53e-6 of the RMS spread of the posed views
TRN_SENSITIVITY_AT_1E_4 = 4.53e-6
TRN_HIP_VS_SPEC_BOUND = 10.0 * TRN_SENSITIVITY_AT_1E_4
# seam 5: ten times the two-leg figures of scripts/chain_roundoff.py on this problem
BA_COST_GAP = 5.47e-15
BA_COST_BOUND = 10.0 * BA_COST_GAP
BA_STATE_DISTANCE = 6.27e-8
BA_STATE_BOUND = 10.0 * BA_STATE_DISTANCE


def angle(Ra, Rb):
    d = np.einsum("...ij,...kj->...ik", Ra, Rb)
    return np.arccos(np.clip((np.trace(d, axis1=-2, axis2=-1) - 1) / 2, -1, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_reference_chain():
    """The CPU leg end to end against ground truth; prints the figures the bounds are taken from and demands that they are
    the constants above (to their printed digits), that the bundle adjustment improves all three errors and that the
    directions point along the ground-truth baselines."""
    ref = CR.reference_chain()
    fig = CR.reference_figures(ref)
    print("min cos %.6f; before %s; after %s; purity %.6f" % (fig["min_cos"], fig["before"], fig["after"], fig["purity"]))
    assert fig["min_cos"] == pytest.approx(CPU_MIN_COS, abs=5e-7)
    assert fig["purity"] == pytest.approx(CPU_PURITY, abs=5e-7)
    for name, want in (("before", CPU_BEFORE), ("after", CPU_AFTER)):
        for k, v in want.items():
            assert fig[name][k] == pytest.approx(v, rel=1e-3), (name, k)
    for k in CPU_BEFORE:
        assert fig["after"][k] <= fig["before"][k], k
    assert fig["before"]["n_points"] >= 200
    # the gauge of both solvers: the roots at identity / 0, the view without an edge too
    for v in (CR.SECOND[0], CR.MAIN[0], CR.CLUTTER):
        assert np.array_equal(ref["R"][v], np.eye(3)) and np.array_equal(ref["c"][v], np.zeros(3))
    assert np.array_equal(ref["has_pose"], ref["scene"]["main"])


def test_reference_conditions():
    """Conditions on the scene, checked on the CPU leg alone.  A seed that fails one is replaced, the condition stays."""
    ref = CR.reference_chain()
    scene, est, tri, ba = ref["scene"], ref["est"], ref["tri"], ref["ba"]
    main = scene["main"]
    for p, (s, d) in enumerate(scene["pairs"]):
        if main[s] and main[d]:
            assert est["ok"][p], (s, d)                 # every pair of the main component is OK
        if CR.CLUTTER in (s, d):
            assert not est["ok"][p], (s, d)             # every pair touching the clutter view is not
    assert max(len(v["xy"]) for v in scene["views"]) <= 700
    assert np.all(ba["ob"]["cam_count"][main] >= B.DEFAULTS["min_cam_obs"])
    assert tri["counts"][TR.OK] >= 200
    # a track that is TOO_FEW because of an unposed view: at least two members, all in views without a pose
    tb = ref["track_begin"].astype(np.int64)
    mem_view = (ref["members"] >> np.uint64(32)).astype(np.int64)
    unposed = [t for t in np.nonzero(tri["status"] == TR.TOO_FEW)[0]
               if tb[t + 1] - tb[t] >= 2 and not ref["has_pose"][mem_view[tb[t]:tb[t + 1]]].any()]
    assert len(unposed) >= 1
    assert (tri["obs_state"] == 2).sum() >= 1 or tri["counts"][TR.REPROJ] >= 1
    assert len(set(np.nonzero(tri["counts"])[0].tolist())) >= 3      # a spread of statuses
    assert ba["accepted"] >= 1 and ba["cost_final"] < ba["cost_initial"]
    # the float64 and longdouble legs by the kernels' formulas take the same accept / reject sequence
    seq = {}
    for ft in (np.float64, np.longdouble):
        trace = []
        B.bundle_adjust(ref["track_begin"], ref["members"], ref["views"], tri["X"], tri["status"], tri["obs_state"], solver="pcg", ft=ft, trace=trace)
        seq[ft] = [t["accepted"] for t in trace]
    assert seq[np.float64] == seq[np.longdouble] == [t["accepted"] for t in ref["ba_trace"]]


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def device_chain(eng, scene):
    """The nine stages on the device, every hand-off in device memory where the API allows it.  -> dict of numpy results
    (and the match / mask rows per pair as the store received them)."""
    from pyposegraphbuilder.engine import DeviceTracklets
    views, cam, pairs = scene["views"], scene["cam"], scene["pairs"]
    P = len(pairs)
    pr = np.array(pairs, np.int64)
    src, dst = pr[:, 0], pr[:, 1]
    images = [eng.prepare_descriptors(v["desc"]) for v in views]
    kps = [eng.upload_keypoints(v["xy"], *cam) for v in views]
    raw = eng.match_descriptors_batch(images, pairs, raw=True)
    batch = eng.build_correspondences(kps, pairs, raw, thr_px=CR.THR_PX, top_k=0, seed=CR.ESTIMATOR_SEED)
    edges, masks = eng.estimate_pose_batch(batch)
    rows = raw[3].cpu().numpy()[:P].astype(np.uint32)
    R, rot_iters, rot_used = eng.rotation_average_edges(edges, src, dst, rows, V)
    c, trn_iters, trn_used = eng.translation_average_edges(edges, src, dst, rows, V, R)
    rec = eng.edges_to_numpy(edges).copy()
    ok = rec["status"] == 1
    off = batch["offsets"].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.diff(off), rows)            # a mask row is a match row
    store = DeviceTracklets(eng, V)
    try:
        store.add_batch([(int(src[p]), int(dst[p]), (raw[0][p, :rows[p]], raw[1][p, :rows[p]]), masks[off[p]:off[p + 1]])
                         for p in range(P) if ok[p]])
        has_pose = CR.largest_component(V, src[ok], dst[ok])
        tri = store.triangulate(kps, R, c, has_pose)
        R_in, c_in, X_in, st_in, ob_in = R.copy(), c.copy(), tri.X.clone(), tri.status.clone(), tri.obs_state.clone()
        ba = store.bundle_adjust(kps, R, c, tri.X, tri.status, tri.obs_state, has_pose=has_pose)
        untouched = (same_bits(R, R_in) and same_bits(c, c_in) and np.array_equal(tri.X.cpu().numpy(), X_in.cpu().numpy(), equal_nan=True)
                     and bool((tri.status == st_in).all()) and bool((tri.obs_state == ob_in).all()))
        tracks = [store.track(i) for i in range(store.info()["tracks"])]
        events = store.info()["events"]
    finally:
        store.close()
    s_h, d_h, m_h = raw[0].cpu().numpy(), raw[1].cpu().numpy(), masks.cpu().numpy()
    matches = [(s_h[p, :rows[p]].astype(np.uint32), d_h[p, :rows[p]].astype(np.uint32)) for p in range(P)]
    x = {k: batch[k].cpu().numpy() for k in ("x1", "y1", "x2", "y2")}
    return dict(src=src, dst=dst, rows=rows, rec=rec, ok=ok, matches=matches, masks=[m_h[off[p]:off[p + 1]] for p in range(P)],
                corr=[np.stack([x[k][off[p]:off[p + 1]] for k in ("x1", "y1", "x2", "y2")], 1) for p in range(P)],
                thr=batch["thr"].cpu().numpy()[:P].copy(), R=R, rot_iters=rot_iters, rot_used=rot_used, c=c, trn_iters=trn_iters,
                trn_used=trn_used, has_pose=has_pose, tracks=tracks, events=events, tri=tri.numpy(), ba=ba, ba_X=ba.X.cpu().numpy(),
                inputs_untouched=untouched)


@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def chain(eng):
    return device_chain(eng, CR.make_scene())


_spec_cache = {}   # CPU results on the device's outputs, shared by the seam tests


def ok_graph(ch):
    return CR.ok_graph(CR.make_scene(), ch["rec"], ch["rows"], ch["ok"])


def spec_positions(ch):
    """transavg_spec on the directions formed from the DEVICE rotations (shared by the seam-2 tests)."""
    cache = _spec_cache
    if "trn" not in cache:
        src, dst, _, t, w = ok_graph(ch)
        gamma = TA.directions_from_edges(ch["R"], src, dst, t)
        cache["trn"] = (gamma,) + TA.translation_average(V, src, dst, gamma, w)
    return cache["trn"]


@pytest.mark.gpu
def test_seam1_edges_to_rotations(chain):
    """Device rotations against rotavg_oracle on the downloaded OK edges with weight n_inl / rows: within 1e-5 rad
    (MI355X: 5.2e-8).  edges_used counts the OK records; the roots of both components and the view without
    an edge come back as the documented gauge."""
    src, dst, Rrel, _, w = ok_graph(chain)
    Ro, it = RO.rotation_average(V, src, dst, Rrel, w)
    worst = float(angle(chain["R"], Ro).max())
    print("seam 1: max angle to the oracle %.3g rad (bound %.3g), iterations %d / %d, %d of %d records OK" %
          (worst, ROT_HIP_VS_ORACLE_RAD, chain["rot_iters"], it, chain["ok"].sum(), len(chain["ok"])))
    assert chain["rot_used"] == chain["ok"].sum() == len(src)
    assert worst < ROT_HIP_VS_ORACLE_RAD
    assert np.array_equal(chain["R"][CR.CLUTTER], np.eye(3))
    for root in (CR.SECOND[0], CR.MAIN[0]):
        assert np.abs(chain["R"][root] - np.eye(3)).max() <= ROOT_IDENTITY_ATOL
    # the second component is one edge: its other view carries that edge's rotation
    p = CR.make_scene()["pairs"].index(CR.SECOND)
    assert chain["ok"][p]
    assert float(angle(chain["R"][CR.SECOND[1]], chain["rec"]["R"][p].reshape(3, 3))) < ROT_HIP_VS_ORACLE_RAD
    assert np.abs(np.einsum("kij,kmj->kim", chain["R"], chain["R"]) - np.eye(3)).max() < 1e-9


@pytest.mark.gpu
def test_seam2_table_entry_point_is_the_edge_entry_point(eng, chain):
    """translation_average_edges on the device table and the device rotations == translation_average on
    transavg_spec.directions_from_edges(R_device, ...) with weight n_inl / rows, bit for bit."""
    src, dst, _, t, w = ok_graph(chain)
    gamma = TA.directions_from_edges(chain["R"], src, dst, t)
    c2, it2 = eng.translation_average(src, dst, gamma, w, V)
    assert chain["trn_used"] == len(src)
    assert it2 == chain["trn_iters"] and same_bits(c2, chain["c"])


@pytest.mark.gpu
def test_seam2_directions_point_along_the_true_baselines(chain):
    """Independent of any solver: R_dst^T t of every OK edge of the main component points along c_gt[src] - c_gt[dst].  The CPU
    leg's smallest cosine is 0.990079; the bound allows twice its 1 - cos.  R_src for R_dst, R for R^T or -t miss it widely."""
    scene = CR.make_scene()
    src, dst, _, t, _ = ok_graph(chain)
    cos = CR.direction_cosines(scene, chain["R"], src, dst, t)
    print("seam 2: %d edges, min cos %.6f, 1 - cos = %.3e (bound %.3e)" % (len(cos), cos.min(), 1 - cos.min(), ONE_MINUS_COS_BOUND))
    assert len(cos) == 45
    assert 1.0 - cos.min() <= ONE_MINUS_COS_BOUND


@pytest.mark.gpu
def test_seam2_rotations_to_positions(chain):
    """Device positions against transavg_spec.translation_average on the same directions, no alignment: within ten times
    the specification's own sensitivity to inner solves stopped at 1e-4, relative to the RMS spread of the posed views.
    Roots and the view without an edge sit at exactly 0."""
    _, c_spec, it_spec = spec_positions(chain)
    posed = chain["has_pose"]
    rms = float(np.sqrt(((c_spec[posed] - c_spec[posed].mean(0)) ** 2).sum(1).mean()))
    diff = float(np.linalg.norm(chain["c"] - c_spec, axis=1).max()) / rms
    print("seam 2: iterations %d (spec %d), max |c - c_spec| / rms = %.3g (bound %.3g)" % (chain["trn_iters"], it_spec, diff, TRN_HIP_VS_SPEC_BOUND))
    assert diff <= TRN_HIP_VS_SPEC_BOUND
    for v in (CR.SECOND[0], CR.MAIN[0], CR.CLUTTER):
        assert np.array_equal(chain["c"][v], np.zeros(3)), v
    assert np.all(np.linalg.norm(chain["c"][[v for v in range(V) if v not in (CR.SECOND[0], CR.MAIN[0], CR.CLUTTER)]], axis=1) > 0)


@pytest.mark.gpu
def test_seam3_matches_and_masks_to_tracks(chain):
    """The store's tracks are tracklets_oracle's on the same calls; every member of a track is a row whose mask bit was set in
    a call of an OK pair; the purity against point_id is no lower than the CPU leg's (0.998609)."""
    scene = CR.make_scene()
    ref = TO.Tracklets()
    for p, (s, d) in enumerate(scene["pairs"]):
        if chain["ok"][p]:
            ref.add(s, d, list(zip(chain["matches"][p][0].tolist(), chain["matches"][p][1].tolist())), chain["masks"][p].tolist())
    assert len(chain["tracks"]) == len(ref.tracks) and chain["events"] == sum(len(t) for t in ref.tracks)
    assert chain["tracks"] == [[tuple(m) for m in t] for t in ref.tracks]
    allowed = CR.mask_members(scene["pairs"], chain["ok"], chain["matches"], chain["masks"])
    members = {m for t in chain["tracks"] for m in t}
    assert members <= allowed and all(len(t) >= 2 for t in chain["tracks"])
    # ... and no member is a row of a failed pair only, or a row the mask dropped: such rows exist, so the test can fail
    dropped = CR.mask_members(scene["pairs"], np.ones(len(scene["pairs"]), bool), chain["matches"], [np.ones(len(m), np.uint8) for m in chain["masks"]]) - allowed
    assert dropped and not (members & dropped)
    assert not any(v == CR.CLUTTER for v, _ in members)
    pur = CR.purity(scene, chain["tracks"])
    print("seam 3: %d tracks, %d members, purity %.6f (CPU leg %.6f)" % (len(chain["tracks"]), chain["events"], pur, CPU_PURITY))
    assert pur >= CPU_PURITY - 5e-7


@pytest.mark.gpu
def test_seam4_tracks_and_poses_to_points(chain):
    """store.triangulate == triangulate_spec.triangulate on the tracks read back and the same R, c, has_pose, bit for bit; a
    realistic spread of statuses; a track with fewer than two posed, eligible members is TOO_FEW."""
    scene = CR.make_scene()
    tb, mem = CR.tracks_to_arrays(chain["tracks"])
    want = TR.triangulate(tb, mem, CR.spec_views(scene, chain["R"], chain["c"], chain["has_pose"]))
    TR.assert_same(chain["tri"], want, "chain")
    counts = chain["tri"]["counts"]
    print("seam 4: statuses %s, %d dropped observations" % (dict(zip(("OK", "TOO_FEW", "DEGENERATE", "BEHIND", "REPROJ", "LOW_PARALLAX"), counts.tolist())),
                                                          int((chain["tri"]["obs_state"] == 2).sum())))
    assert counts[TR.OK] >= 200 and counts[TR.TOO_FEW] >= 1 and np.count_nonzero(counts) >= 3
    assert (chain["tri"]["obs_state"] == 2).sum() >= 1 or counts[TR.REPROJ] >= 1
    for i, t in enumerate(chain["tracks"]):
        posed_views = {v for v, k in t if chain["has_pose"][v] and k < len(scene["views"][v]["xy"])}
        if len(posed_views) < 2:
            assert chain["tri"]["status"][i] == TR.TOO_FEW, i
    assert np.array_equal(chain["has_pose"], scene["main"])


@pytest.mark.gpu
def test_seam5_points_and_poses_to_bundle_adjustment(chain):
    """store.bundle_adjust against bundle_spec.bundle_adjust (direct solves) from the same inputs: final-cost gap and
    state_distance within ten times the two-leg figures of scripts/chain_roundoff.py; the cost decreased, a step was
    accepted, the held views (the gauge view 1 and the views outside the main component) keep their bits, the inputs too."""
    scene = CR.make_scene()
    tb, mem = CR.tracks_to_arrays(chain["tracks"])
    views = CR.spec_views(scene, chain["R"], chain["c"], chain["has_pose"])
    tri, ba = chain["tri"], chain["ba"]
    ref = B.bundle_adjust(tb, mem, views, tri["X"], tri["status"], tri["obs_state"])
    gap = abs(ba.cost_final - ref["cost_final"]) / ref["cost_final"]
    dist = B.state_distance(dict(R=ba.R, c=ba.c, X=chain["ba_X"]), ref, dict(R=views["R"], c=views["c"], X=tri["X"]))
    print("seam 5: cost %.15g against %.15g, gap %.3g (bound %.3g), state distance %.3g (bound %.3g); %s" %
          (ba.cost_final, ref["cost_final"], gap, BA_COST_BOUND, dist, BA_STATE_BOUND, ba.report()))
    assert (ba.n_obs, ba.n_points, ba.n_free_cams) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"])
    assert ba.n_free_cams == len(CR.MAIN) - 1
    assert ba.cost_final < ba.cost_initial and ba.accepted >= 1
    assert gap <= BA_COST_BOUND
    assert dist <= BA_STATE_BOUND
    held = ~scene["main"]
    held[CR.MAIN[0]] = True
    assert same_bits(ba.R[held], chain["R"][held]) and same_bits(ba.c[held], chain["c"][held])
    free = ~held
    assert all(not same_bits(ba.R[v], chain["R"][v]) and not same_bits(ba.c[v], chain["c"][v]) for v in np.nonzero(free)[0])
    part = np.zeros(len(tri["X"]), bool)
    part[ref["ob"]["pt"]] = True
    assert np.array_equal(chain["ba_X"][~part], tri["X"][~part], equal_nan=True)
    assert chain["inputs_untouched"]


@pytest.mark.gpu
def test_seam6_against_ground_truth(chain):
    """One similarity (Umeyama on the main component's centres), applied to the points as well: rotation, centre and median
    point error before and after the bundle adjustment, each within twice the CPU leg's figure; the bundle adjustment makes
    none of them worse."""
    scene = CR.make_scene()
    tri = chain["tri"]
    before = CR.ground_truth_errors(scene, chain["R"], chain["c"], tri["X"], tri["status"], chain["tracks"])
    after = CR.ground_truth_errors(scene, chain["ba"].R, chain["ba"].c, chain["ba_X"], tri["status"], chain["tracks"])
    print("seam 6: before %s (CPU leg %s); after %s (CPU leg %s)" % (before, CPU_BEFORE, after, CPU_AFTER))
    for k in CPU_BEFORE:
        assert before[k] <= GT_FACTOR * CPU_BEFORE[k], ("before", k)
        assert after[k] <= GT_FACTOR * CPU_AFTER[k], ("after", k)
        assert after[k] <= before[k], k
    assert before["n_points"] >= 200


@pytest.mark.gpu
def test_seam7_bits_are_repeatable(eng, chain):
    again = device_chain(eng, CR.make_scene())
    assert same_bits(again["rec"], chain["rec"]) and all(np.array_equal(a, b) for a, b in zip(again["masks"], chain["masks"]))
    assert same_bits(again["R"], chain["R"]) and same_bits(again["c"], chain["c"])
    assert (again["rot_iters"], again["rot_used"], again["trn_iters"], again["trn_used"]) == \
        (chain["rot_iters"], chain["rot_used"], chain["trn_iters"], chain["trn_used"])
    assert again["tracks"] == chain["tracks"]
    TR.assert_same(again["tri"], chain["tri"], "second run")
    assert same_bits(again["ba"].R, chain["ba"].R) and same_bits(again["ba"].c, chain["ba"].c) and same_bits(again["ba_X"], chain["ba_X"])
    assert again["ba"].report() == chain["ba"].report()
