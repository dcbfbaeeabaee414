"""The chain with a wrong edge and wrong focals: cycle filter and focal bundle adjustment inside the chain, seam by seam
(scene and CPU leg: tests/chain_ref.py, make_filtered_scene / reference_filtered_chain).

The scene is the chain scene of tests/test_chain.py with two changes: on three view-disjoint pairs of the main component a
twin structure makes the ESTIMATOR return an OK record with a wrong pose (15..25 degrees off) whose mask selects the twin rows,
and every stage is told focals that are off by up to FOCAL_ERR per view of the main component.  The device chain (module
fixture `chain`): prepare_descriptors / upload_keypoints(f_nominal) -> match_descriptors_batch -> build_correspondences ->
estimate_pose_batch -> cycle_filter_edges(out=filtered) -> rotation_average_edges(filtered) ->
translation_average_edges(filtered) -> DeviceTracklets.add_batch of the pairs whose FILTERED status is OK -> triangulate ->
bundle_adjust(refine_focal=True) -> upload_keypoints(f_nominal * phi) -> triangulate -> bundle_adjust.  At every seam the
device's ACTUAL upstream output goes to the CPU specification of the next stage, under the bound that stage already has.

Conventions pinned here and nowhere else: both averaging entry points skip a PGI_EDGE_INCONSISTENT record of the filtered table;
the caller keeps a dropped pair's matches out of the store; has_pose is the largest component of the KEPT edges; the caller
multiplies fx, fy by phi before triangulating again (include/pgi.h, pgi_bundle_adjust_focal); the pose-only run on the rescaled
views starts no worse than the focal run started, and equals the focal entry with every focal held at phi.

Measured on the CPU (scripts/chain_filtered_roundoff.py), base seed 3, draw 3, FOCAL_ERR 0.01 (the ladder: chain_ref.py), n_twin 150:
twin pairs (4, 9), (5, 8), (10, 11): OK in the oracle's estimator at 19.91 / 17.60 / 24.91 degrees from the truth, masks of
118 / 124 / 121 rows of which 118 / 122 / 121 twin rows; the filter at defaults drops exactly these (8 triangles each, none
good), margin 2.48e-3; 43 kept edges, 641 tracks (508 OK, 37 TOO_FEW, 93 REPROJ, 3 LOW_PARALLAX; 601 OK after phi), purity 1.
                       rotation deg   centre      median point   RMS focal error
  before the focal run    0.6088      9.006e-3    1.479e-1       5.588e-3
  after the focal run     0.5677      7.033e-3    6.867e-2       3.414e-3     (cost 2833 -> 196, 5 of 5 steps, 9 poses, 10 focals)
  re-triangulated + run   0.4657      7.394e-3    5.442e-2                    (cost 442 -> 404)
  without the filter      0.6735 / 1.0373 / 0.8658 deg, 8.712e-3 / 6.049e-3 / 6.068e-3, 1.498e-1 / 1.153e-1 / 1.044e-1, focal 2.725e-3;
                          1003 tracks, purity 0.640080, 722 twin members
  seam 2': inner solves stopped at 1e-4 move the positions by 1.43e-6 of the RMS spread of the posed views
  seam 5': focal run, float64 PCG leg against the direct solves: cost gap 1.26e-14, state distance 1.94e-8
  seam 6': pose-only run, the same: cost gap 9.44e-15, state distance 6.62e-9
Measured on the MI355X: seam F equal to cycle_spec, margin 2.48e-3, the twin records at 19.91 / 17.60 / 24.91 degrees; seam 1'
5.2e-8 rad, 43 edges used; seam 2' identical bits through both entry points, positions 8.0e-6 of the RMS spread; seam 3' tracks
equal, no twin member (361 twin rows with a set mask bit in the dropped pairs), purity 1; seam 4' identical bits (508 / 37 / 93 / 3);
seam 5' cost gap 4.3e-16, state distance 1.6e-8, cost 2844 -> 197 in 5 accepted steps; seam 6' identical bits (601 / 37 / 0 / 3),
cost gap 1.3e-14, state distance 4.9e-9, start 441 against 2844, the held-focal entry returns the pose-only bits; seam 7'
0.607 deg / 9.01e-3 / 1.48e-1, 0.553 / 6.92e-3 / 6.71e-2, 0.448 / 7.38e-3 / 5.28e-2, focal 5.59e-3 -> 3.49e-3; seam 8' identical bits.
"""
import os
import sys

import numpy as np
import pytest

import bundle_focal_spec as BF
import bundle_spec as B
import chain_ref as CR
import cycle_spec as CS
import transavg_spec as TA
import triangulate_spec as TR
from pyposegraphbuilder import synthetic as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rotavg_oracle as RO  # noqa: E402
import tracklets_oracle as TO  # noqa: E402

V = CR.N_VIEWS
TWIN_MIN_ANGLE_DEG = 10.0

# ---- the CPU leg's figures (test_reference_filtered_chain demands that the leg still gives them) and the bounds from them ----
STATIONS = ("before", "focal", "final")
CPU = dict(before=dict(rot_deg=0.6088, centre=9.006e-3, point=1.479e-1),
           focal=dict(rot_deg=0.5677, centre=7.033e-3, point=6.867e-2),
           final=dict(rot_deg=0.4657, centre=7.394e-3, point=5.442e-2))
CPU_FOCAL_BEFORE, CPU_FOCAL_AFTER = 5.5879e-3, 3.4139e-3
CPU_PURITY = 1.0
CPU_UNFILTERED = dict(before=dict(rot_deg=0.6735, centre=8.712e-3, point=1.498e-1),
                      focal=dict(rot_deg=1.0373, centre=6.049e-3, point=1.153e-1),
                      final=dict(rot_deg=0.8658, centre=6.068e-3, point=1.044e-1))
CPU_UNFILTERED_FOCAL_AFTER = 2.7253e-3
CPU_UNFILTERED_PURITY = 0.640080
GT_FACTOR = 2.0
# seam 1': the existing bound of tests/test_chain.py, tests/test_pose_graph_pipeline.py and tests/test_rotavg.py
ROT_HIP_VS_ORACLE_RAD = 1e-5
# seam 2': the rule of tests/test_transavg.py (ten times the specification's sensitivity to inner solves stopped at 1e-4),
# re-measured on the kept edges of this graph by scripts/chain_filtered_roundoff.py: 1.43e-6 of the RMS spread of the posed views
TRN_SENSITIVITY_AT_1E_4 = 1.43e-6
TRN_HIP_VS_SPEC_BOUND = 10.0 * TRN_SENSITIVITY_AT_1E_4
# seams 5' and 6': ten times the two-leg figures of scripts/chain_filtered_roundoff.py on this problem
BAF_COST_GAP, BAF_STATE_DISTANCE = 1.26e-14, 1.94e-8
BA2_COST_GAP, BA2_STATE_DISTANCE = 9.44e-15, 6.62e-9
ROUNDOFF_FACTOR = 10.0


def angle(Ra, Rb):
    d = np.einsum("...ij,...kj->...ik", Ra, Rb)
    return np.arccos(np.clip((np.trace(d, axis1=-2, axis2=-1) - 1) / 2, -1, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def twin_index(scene):
    return [scene["pairs"].index(tp) for tp in scene["twin_pairs"]]


def wrong_by_deg(scene, rec, p):
    s, d = scene["pairs"][p]
    return S.rot_err_deg(np.asarray(rec["R"][p], np.float64).reshape(3, 3), CR.true_relative_rotation(scene, s, d))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_make_scene_is_unchanged_by_the_filtered_scene():
    """make_filtered_scene copies: the base scene's arrays keep their bits, and the twin keypoints are appended behind them."""
    base = CR.make_scene()
    before = [(v["xy"].copy(), v["desc"].copy(), np.array(v["point_id"])) for v in base["views"]]
    sc = CR.make_filtered_scene()
    for v, (xy, desc, pid) in enumerate(before):
        assert same_bits(base["views"][v]["xy"], xy) and same_bits(base["views"][v]["desc"], desc) and np.array_equal(base["views"][v]["point_id"], pid)
        n = len(xy)
        assert same_bits(sc["views"][v]["xy"][:n], xy) and same_bits(sc["views"][v]["desc"][:n], desc)
        twin = sc["views"][v]["point_id"][n:]
        assert len(twin) == (CR.N_TWIN if any(v in tp for tp in sc["twin_pairs"]) else 0) and np.all(twin <= CR.TWIN_ID_BASE)
    assert sc["pairs"] == base["pairs"] and sc["cam"] == base["cam"]
    assert same_bits(CR.camera_K(base["cam"]), CR.camera_K(base["cam"], focal=np.full(V, base["cam"][0])))
    # the twin pairs: three candidate pairs inside MAIN, no shared view, none touching the gauge view
    tv = [v for tp in sc["twin_pairs"] for v in tp]
    assert len(sc["twin_pairs"]) == CR.N_TWIN_PAIRS and len(set(tv)) == 2 * CR.N_TWIN_PAIRS and CR.MAIN[0] not in tv
    assert all(v in CR.MAIN for v in tv) and all(tp in sc["pairs"] for tp in sc["twin_pairs"])
    for RT in sc["twin_R"]:
        assert CR.TWIN_ROT_DEG[0] <= S.rot_err_deg(RT, np.eye(3)) <= CR.TWIN_ROT_DEG[1]
    e = sc["focal_e"]
    assert np.all(e[~sc["main"]] == 0) and np.all(np.abs(e) <= CR.FOCAL_ERR) and np.all(e[sc["main"]] != 0)
    assert same_bits(sc["f_nominal"], sc["f_true"] * (1.0 + e))


def test_reference_filtered_conditions():
    """Conditions on the inputs, checked on the reference alone.  A draw, n_twin or FOCAL_ERR that fails one is replaced (the
    record of what was tried is in chain_ref.py), the condition stays."""
    ref = CR.reference_filtered_chain()
    scene, est, cyc, kept, leg = ref["scene"], ref["est"], ref["cyc"], ref["kept"], ref["filtered"]
    main, pairs = scene["main"], scene["pairs"]
    twins = twin_index(scene)
    assert max(len(v["xy"]) for v in scene["views"]) <= 700
    for p in twins:       # OK in the estimator, a wrong rotation, a mask that selects the twin rows
        m, tw = est["masks"][p].astype(bool), CR.twin_rows(scene, p, est["matches"][p])
        assert est["ok"][p], pairs[p]
        assert wrong_by_deg(scene, est["edges"], p) > TWIN_MIN_ANGLE_DEG, pairs[p]
        assert 2 * (m & tw).sum() > m.sum(), pairs[p]
    for p, (s, d) in enumerate(pairs):
        if main[s] and main[d]:
            assert est["ok"][p], (s, d)
        if CR.CLUTTER in (s, d):
            assert not est["ok"][p], (s, d)
    # the filter at defaults drops exactly the twin records, each of them tested, and no decision sits on a rounding difference
    dropped = np.nonzero(est["ok"] & ~kept)[0].tolist()
    assert dropped == sorted(twins)
    assert np.all(cyc["n_tri"][dropped] > 0)
    assert np.array_equal(kept, est["ok"] & ~np.isin(np.arange(len(pairs)), twins))
    assert CS.margins(cyc["quantities"]) > CS.MARGIN
    src, dst = leg["graph"][:2]
    assert np.array_equal(CR.largest_component(V, src, dst), main)      # the kept edges still join all of MAIN
    # every MAIN view focal-free at the default min_focal_obs, and pose-free except the gauge view
    baf = leg["baf"]
    assert np.array_equal(baf["ffree"], main)
    free = main.copy()
    free[CR.MAIN[0]] = False
    assert np.array_equal(baf["ob"]["free"], free)
    assert baf["n_free_focals"] == len(CR.MAIN) and baf["n_free_cams"] == len(CR.MAIN) - 1
    # the float64 PCG leg, the longdouble leg and the direct-solve leg take the same accept / reject sequence
    tri = leg["tri"]
    seq = {}
    for ft in (np.float64, np.longdouble):
        trace = []
        BF.bundle_adjust(leg["track_begin"], leg["members"], leg["views"], tri["X"], tri["status"], tri["obs_state"], solver="pcg", ft=ft, trace=trace)
        seq[ft] = [t["accepted"] for t in trace]
    assert seq[np.float64] == seq[np.longdouble] == [t["accepted"] for t in leg["baf_trace"]]
    assert baf["accepted"] >= 1 and baf["cost_final"] < baf["cost_initial"]


def test_reference_filtered_chain():
    """The CPU leg against ground truth, with the filter and without; prints the figures the bounds are taken from and demands
    that they are the constants above (to their printed digits), that the focal run lowers the focal error and makes no pose or
    point figure worse, and that the filter lowers the rotation error before any bundle adjustment."""
    ref = CR.reference_filtered_chain()
    scene = ref["scene"]
    fig, unf = CR.leg_figures(scene, ref["filtered"]), CR.leg_figures(scene, ref["unfiltered"])
    for name, f in (("filtered", fig), ("unfiltered", unf)):
        print("%s: %s; focal %.4e -> %.4e; purity %.6f" % (name, {k: f[k] for k in STATIONS}, f["focal_before"], f["focal_after"], f["purity"]))
    for f, want in ((fig, CPU), (unf, CPU_UNFILTERED)):
        for st in STATIONS:
            for k, v in want[st].items():
                assert f[st][k] == pytest.approx(v, rel=1e-3), (st, k)
    assert fig["focal_before"] == unf["focal_before"] == pytest.approx(CPU_FOCAL_BEFORE, rel=1e-3)
    assert fig["focal_after"] == pytest.approx(CPU_FOCAL_AFTER, rel=1e-3)
    assert unf["focal_after"] == pytest.approx(CPU_UNFILTERED_FOCAL_AFTER, rel=1e-3)
    assert fig["purity"] == pytest.approx(CPU_PURITY, abs=5e-7) and unf["purity"] == pytest.approx(CPU_UNFILTERED_PURITY, abs=5e-7)
    assert fig["focal_after"] < fig["focal_before"]
    for k in CPU["before"]:
        assert fig["focal"][k] <= fig["before"][k], k
    assert fig["before"]["rot_deg"] < unf["before"]["rot_deg"]
    assert fig["before"]["n_points"] >= 200
    # the filter earns its place in the store as well: without it the twin keypoints become tracks
    assert not CR.has_twin_member(scene, ref["filtered"]["tracks"]) and CR.has_twin_member(scene, ref["unfiltered"]["tracks"])
    leg = ref["filtered"]
    assert leg["ba2"]["cost_initial"] <= leg["baf"]["cost_initial"]
    for v in (CR.SECOND[0], CR.MAIN[0], CR.CLUTTER):
        assert np.array_equal(leg["R"][v], np.eye(3)) and np.array_equal(leg["c"][v], np.zeros(3))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("unfiltered_table", "all_ok_pairs", "unscaled_second", "unfiltered_has_pose")


def device_chain(eng, scene, mutation=None):
    """The eleven stages on the device, every hand-off in device memory where the API allows it.  -> dict of numpy results.
    mutation (one of MUTATIONS, for the mutation check by hand only): the named convention is broken on purpose."""
    import torch
    from pyposegraphbuilder.engine import DeviceTracklets
    assert mutation is None or mutation in MUTATIONS
    views, (_, w, h), pairs, f_nom = scene["views"], scene["cam"], scene["pairs"], scene["f_nominal"]
    P = len(pairs)
    pr = np.array(pairs, np.int64)
    src, dst = pr[:, 0], pr[:, 1]
    images = [eng.prepare_descriptors(v["desc"]) for v in views]
    kps = [eng.upload_keypoints(v["xy"], f_nom[i], w, h) for i, v in enumerate(views)]
    raw = eng.match_descriptors_batch(images, pairs, raw=True)
    batch = eng.build_correspondences(kps, pairs, raw, thr_px=CR.THR_PX, top_k=0, seed=CR.ESTIMATOR_SEED)
    edges, masks = eng.estimate_pose_batch(batch)
    rows = raw[3].cpu().numpy()[:P].astype(np.uint32)
    table_in = edges.clone()
    filtered = torch.zeros_like(edges)
    keep, n_tri, n_good, summary = eng.cycle_filter_edges(edges, src, dst, V, out=filtered)
    table_untouched = bool((edges == table_in).all())
    averaged = edges if mutation == "unfiltered_table" else filtered
    R, rot_iters, rot_used = eng.rotation_average_edges(averaged, src, dst, rows, V)
    c, trn_iters, trn_used = eng.translation_average_edges(averaged, src, dst, rows, V, R)
    rec = eng.edges_to_numpy(edges).copy()
    frec = eng.edges_to_numpy(filtered).copy()
    ok, okf = rec["status"] == CS.EDGE_OK, frec["status"] == CS.EDGE_OK
    off = batch["offsets"].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.diff(off), rows)            # a mask row is a match row
    inserted = ok if mutation == "all_ok_pairs" else okf
    store = DeviceTracklets(eng, V)
    try:
        store.add_batch([(int(src[p]), int(dst[p]), (raw[0][p, :rows[p]], raw[1][p, :rows[p]]), masks[off[p]:off[p + 1]])
                         for p in range(P) if inserted[p]])
        graph = ok if mutation == "unfiltered_has_pose" else okf
        has_pose = CR.largest_component(V, src[graph], dst[graph])
        tri = store.triangulate(kps, R, c, has_pose)
        R_in, c_in, X_in, st_in, ob_in = R.copy(), c.copy(), tri.X.clone(), tri.status.clone(), tri.obs_state.clone()
        baf = store.bundle_adjust(kps, R, c, tri.X, tri.status, tri.obs_state, has_pose=has_pose, refine_focal=True)
        untouched = (same_bits(R, R_in) and same_bits(c, c_in) and np.array_equal(tri.X.cpu().numpy(), X_in.cpu().numpy(), equal_nan=True)
                     and bool((tri.status == st_in).all()) and bool((tri.obs_state == ob_in).all()))
        phi = baf.focal.copy()
        f2 = f_nom if mutation == "unscaled_second" else f_nom * phi
        kps2 = [eng.upload_keypoints(v["xy"], f2[i], w, h) for i, v in enumerate(views)]
        tri2 = store.triangulate(kps2, baf.R, baf.c, has_pose)
        ba2 = store.bundle_adjust(kps2, baf.R, baf.c, tri2.X, tri2.status, tri2.obs_state, has_pose=has_pose)
        # the focal entry with every focal held at phi, on the UNSCALED keypoints
        ba3 = store.bundle_adjust(kps, baf.R, baf.c, tri2.X, tri2.status, tri2.obs_state, has_pose=has_pose, refine_focal=True,
                                  focal=phi, focal_fixed=np.ones(V, bool))
        tracks = [store.track(i) for i in range(store.info()["tracks"])]
        events = store.info()["events"]
    finally:
        store.close()
    s_h, d_h, m_h = raw[0].cpu().numpy(), raw[1].cpu().numpy(), masks.cpu().numpy()
    matches = [(s_h[p, :rows[p]].astype(np.uint32), d_h[p, :rows[p]].astype(np.uint32)) for p in range(P)]
    x = {k: batch[k].cpu().numpy() for k in ("x1", "y1", "x2", "y2")}
    return dict(src=src, dst=dst, rows=rows, rec=rec, frec=frec, ok=ok, okf=okf, table_untouched=table_untouched,
                corr=[np.stack([x[k][off[p]:off[p + 1]] for k in ("x1", "y1", "x2", "y2")], 1) for p in range(P)],
                thr=batch["thr"].cpu().numpy()[:P].copy(),
                keep=keep.cpu().numpy(), n_tri=n_tri.cpu().numpy().view(np.uint32), n_good=n_good.cpu().numpy().view(np.uint32), summary=summary,
                matches=matches, masks=[m_h[off[p]:off[p + 1]] for p in range(P)], R=R, rot_iters=rot_iters, rot_used=rot_used, c=c,
                trn_iters=trn_iters, trn_used=trn_used, has_pose=has_pose, tracks=tracks, events=events, tri=tri.numpy(), baf=baf,
                baf_X=baf.X.cpu().numpy(), phi=phi, f2=np.asarray(f2, np.float64), tri2=tri2.numpy(), ba2=ba2, ba2_X=ba2.X.cpu().numpy(), ba3=ba3,
                ba3_X=ba3.X.cpu().numpy(), inputs_untouched=untouched)


@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def chain(eng):
    return device_chain(eng, CR.make_filtered_scene())


def kept_graph(ch):
    return CR.ok_graph(CR.make_filtered_scene(), ch["frec"], ch["rows"], ch["okf"])


def device_figures(scene, ch):
    tri, tri2 = ch["tri"], ch["tri2"]
    return dict(before=CR.ground_truth_errors(scene, ch["R"], ch["c"], tri["X"], tri["status"], ch["tracks"]),
                focal=CR.ground_truth_errors(scene, ch["baf"].R, ch["baf"].c, ch["baf_X"], tri["status"], ch["tracks"]),
                final=CR.ground_truth_errors(scene, ch["ba2"].R, ch["ba2"].c, ch["ba2_X"], tri2["status"], ch["tracks"]),
                focal_before=CR.focal_rms(scene, np.ones(V)), focal_after=CR.focal_rms(scene, ch["phi"]))


@pytest.mark.gpu
def test_seamF_table_to_filter(chain):
    """cycle_filter_edges on the estimator's table == cycle_spec on the downloaded table (keep, n_tri, n_good, summary), with no
    decision on a rounding difference; `filtered` is the table with EDGE_INCONSISTENT on exactly the dropped records, byte
    for byte elsewhere; the input table is untouched; the dropped records are the three twin pairs, each an OK record of the
    DEVICE's estimator more than 10 degrees from the truth whose mask selects mostly twin rows."""
    scene = CR.make_filtered_scene()
    rec, frec = chain["rec"], chain["frec"]
    want = CS.cycle_filter(V, chain["src"], chain["dst"], rec["R"].reshape(-1, 3, 3), rec["t"], rec["status"], details=True)
    margin = CS.margins(want["quantities"])
    dropped = np.nonzero(chain["ok"] & (chain["keep"] == 0))[0].tolist()
    print("seam F: %s, dropped %s, margin %.3e (must exceed %g)" % (chain["summary"], [scene["pairs"][p] for p in dropped], margin, CS.MARGIN))
    assert margin > CS.MARGIN
    assert np.array_equal(chain["keep"], want["keep"]) and np.array_equal(chain["n_tri"], want["n_tri"]) and np.array_equal(chain["n_good"], want["n_good"])
    assert chain["summary"] == want["summary"]
    assert chain["table_untouched"]
    status = CS.filtered_status(rec["status"], chain["keep"])
    expect = rec.copy()
    expect["status"] = status
    assert same_bits(frec, expect)
    assert np.nonzero(frec["status"] != rec["status"])[0].tolist() == dropped and np.all(frec["status"][dropped] == CS.EDGE_INCONSISTENT)
    assert dropped == sorted(twin_index(scene))
    for p in dropped:
        m, tw = chain["masks"][p].astype(bool), CR.twin_rows(scene, p, chain["matches"][p])
        deg = wrong_by_deg(scene, rec, p)
        print("        pair %s: %.2f deg from the truth, mask %d rows of which %d twin rows, n_tri %d, n_good %d" %
              (scene["pairs"][p], deg, m.sum(), (m & tw).sum(), chain["n_tri"][p], chain["n_good"][p]))
        assert deg > TWIN_MIN_ANGLE_DEG and 2 * (m & tw).sum() > m.sum() and chain["n_tri"][p] > 0
    for p, (s, d) in enumerate(scene["pairs"]):
        assert chain["ok"][p] == bool(scene["main"][s] and scene["main"][d] or (s, d) == CR.SECOND), (s, d)


@pytest.mark.gpu
def test_seam1_filtered_table_to_rotations(chain):
    """rotation_average_edges on the filtered table skips the INCONSISTENT records: edges_used is the number of kept records,
    and the rotations are rotavg_oracle's on the kept records within 1e-5 rad."""
    src, dst, Rrel, _, w = kept_graph(chain)
    Ro, it = RO.rotation_average(V, src, dst, Rrel, w)
    worst = float(angle(chain["R"], Ro).max())
    n_kept = int(chain["okf"].sum())
    print("seam 1': max angle to the oracle on the kept records %.3g rad (bound %.3g), iterations %d / %d, %d of %d OK records kept" %
          (worst, ROT_HIP_VS_ORACLE_RAD, chain["rot_iters"], it, n_kept, chain["ok"].sum()))
    assert n_kept == int(chain["ok"].sum()) - CR.N_TWIN_PAIRS == len(src)
    assert chain["rot_used"] == n_kept
    assert worst < ROT_HIP_VS_ORACLE_RAD
    assert np.array_equal(chain["R"][CR.CLUTTER], np.eye(3))


@pytest.mark.gpu
def test_seam2_filtered_table_to_positions(eng, chain):
    """translation_average_edges on the filtered table and the device rotations == translation_average on
    directions_from_edges(R_device) of the KEPT records, bit for bit; edges_used is the number of kept records; against
    transavg_spec on the same directions within ten times its sensitivity to inner solves stopped at 1e-4."""
    src, dst, _, t, w = kept_graph(chain)
    gamma = TA.directions_from_edges(chain["R"], src, dst, t)
    c2, it2 = eng.translation_average(src, dst, gamma, w, V)
    assert chain["trn_used"] == len(src) == int(chain["okf"].sum())
    assert it2 == chain["trn_iters"] and same_bits(c2, chain["c"])
    c_spec, it_spec = TA.translation_average(V, src, dst, gamma, w)
    posed = chain["has_pose"]
    rms = float(np.sqrt(((c_spec[posed] - c_spec[posed].mean(0)) ** 2).sum(1).mean()))
    diff = float(np.linalg.norm(chain["c"] - c_spec, axis=1).max()) / rms
    print("seam 2': iterations %d (spec %d), max |c - c_spec| / rms = %.3g (bound %.3g)" % (chain["trn_iters"], it_spec, diff, TRN_HIP_VS_SPEC_BOUND))
    assert diff <= TRN_HIP_VS_SPEC_BOUND
    for v in (CR.SECOND[0], CR.MAIN[0], CR.CLUTTER):
        assert np.array_equal(chain["c"][v], np.zeros(3)), v


@pytest.mark.gpu
def test_seam3_kept_pairs_to_tracks(chain):
    """The store's tracks are tracklets_oracle's on the calls of the kept pairs; no member is a twin keypoint, although twin
    rows with set mask bits exist in the dropped pairs; purity no lower than the CPU leg's."""
    scene = CR.make_filtered_scene()
    ref = TO.Tracklets()
    for p, (s, d) in enumerate(scene["pairs"]):
        if chain["okf"][p]:
            ref.add(s, d, list(zip(chain["matches"][p][0].tolist(), chain["matches"][p][1].tolist())), chain["masks"][p].tolist())
    assert len(chain["tracks"]) == len(ref.tracks) and chain["events"] == sum(len(t) for t in ref.tracks)
    assert chain["tracks"] == [[tuple(m) for m in t] for t in ref.tracks]
    twin_set = sum(int((chain["masks"][p].astype(bool) & CR.twin_rows(scene, p, chain["matches"][p])).sum()) for p in twin_index(scene))
    twin_members = CR.has_twin_member(scene, chain["tracks"])
    pur = CR.purity(scene, chain["tracks"])
    print("seam 3': %d tracks, %d members, %d twin members (%d twin rows with a set mask bit in the dropped pairs), purity %.6f (CPU leg %.6f)" %
          (len(chain["tracks"]), chain["events"], len(twin_members), twin_set, pur, CPU_PURITY))
    assert twin_set > 0 and not twin_members
    allowed = CR.mask_members(scene["pairs"], chain["okf"], chain["matches"], chain["masks"])
    assert {m for t in chain["tracks"] for m in t} <= allowed
    assert pur >= CPU_PURITY - 5e-7


@pytest.mark.gpu
def test_seam4_tracks_and_poses_to_points(chain):
    """store.triangulate == triangulate_spec on the tracks read back and the device's R, c, has_pose at f_nominal, bit for
    bit; has_pose (the largest component of the KEPT edges) is MAIN."""
    scene = CR.make_filtered_scene()
    tb, mem = CR.tracks_to_arrays(chain["tracks"])
    want = TR.triangulate(tb, mem, CR.spec_views(scene, chain["R"], chain["c"], chain["has_pose"], scene["f_nominal"]))
    counts = chain["tri"]["counts"]
    print("seam 4': statuses %s, %d dropped observations" % (counts.tolist(), int((chain["tri"]["obs_state"] == 2).sum())))
    TR.assert_same(chain["tri"], want, "filtered chain")
    assert np.array_equal(chain["has_pose"], scene["main"])
    assert counts[TR.OK] >= 200


@pytest.mark.gpu
def test_seam5_points_and_poses_to_focal_bundle_adjustment(chain):
    """store.bundle_adjust(refine_focal=True) against bundle_focal_spec (direct solves) from the same inputs: final-cost gap and
    state_distance (phi included) within ten times the two-leg figures of scripts/chain_filtered_roundoff.py; the counts are
    equal; phi of every view that is not focal-free and the held poses keep their bits; the inputs are untouched."""
    scene = CR.make_filtered_scene()
    tb, mem = CR.tracks_to_arrays(chain["tracks"])
    views = CR.spec_views(scene, chain["R"], chain["c"], chain["has_pose"], scene["f_nominal"])
    tri, ba = chain["tri"], chain["baf"]
    ref = BF.bundle_adjust(tb, mem, views, tri["X"], tri["status"], tri["obs_state"])
    gap = abs(ba.cost_final - ref["cost_final"]) / ref["cost_final"]
    one = np.ones(V)
    dist = BF.state_distance(dict(R=ba.R, c=ba.c, X=chain["baf_X"], phi=chain["phi"]), ref, dict(R=views["R"], c=views["c"], X=tri["X"], phi=one))
    bounds = (ROUNDOFF_FACTOR * BAF_COST_GAP, ROUNDOFF_FACTOR * BAF_STATE_DISTANCE)
    print("seam 5': cost %.15g against %.15g, gap %.3g (bound %.3g), state distance %.3g (bound %.3g); %d free focals; %s" %
          (ba.cost_final, ref["cost_final"], gap, bounds[0], dist, bounds[1], ba.n_free_focals, ba.report()))
    assert (ba.n_obs, ba.n_points, ba.n_free_cams, ba.n_free_focals) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"], ref["n_free_focals"])
    assert ba.n_free_cams == len(CR.MAIN) - 1 and ba.n_free_focals == len(CR.MAIN)
    assert ba.cost_final < ba.cost_initial and ba.accepted >= 1
    assert gap <= bounds[0]
    assert dist <= bounds[1]
    assert same_bits(chain["phi"][~ref["ffree"]], one[~ref["ffree"]]) and np.array_equal(ref["ffree"], scene["main"])
    assert all(chain["phi"][v] != 1.0 for v in CR.MAIN)
    held = ~scene["main"]
    held[CR.MAIN[0]] = True
    assert same_bits(ba.R[held], chain["R"][held]) and same_bits(ba.c[held], chain["c"][held])
    assert all(not same_bits(ba.R[v], chain["R"][v]) and not same_bits(ba.c[v], chain["c"][v]) for v in np.nonzero(~held)[0])
    part = np.zeros(len(tri["X"]), bool)
    part[ref["ob"]["pt"]] = True
    assert np.array_equal(chain["baf_X"][~part], tri["X"][~part], equal_nan=True)
    assert chain["inputs_untouched"]


@pytest.mark.gpu
def test_seam6_phi_to_retriangulation_and_pose_only_run(chain):
    """The caller's loop of include/pgi.h: fx, fy times the DEVICE's phi, then triangulate again == triangulate_spec with K
    scaled by that phi, bit for bit; the pose-only run on those views against bundle_spec (direct solves) under the seam-5
    rule; it starts no worse than the focal run started; and the focal entry with every focal held at phi on the UNSCALED
    keypoints returns the bits of the pose-only run on the rescaled ones."""
    scene = CR.make_filtered_scene()
    tb, mem = CR.tracks_to_arrays(chain["tracks"])
    baf, ba2, ba3, tri2 = chain["baf"], chain["ba2"], chain["ba3"], chain["tri2"]
    K2 = BF.scaled_K(CR.camera_K(scene["cam"], focal=scene["f_nominal"]), chain["phi"])
    assert same_bits(K2[:, 0], chain["f2"]) and same_bits(K2[:, 1], chain["f2"])      # one multiplication on either side
    views2 = dict(CR.spec_views(scene, baf.R, baf.c, chain["has_pose"]), K=K2)
    want = TR.triangulate(tb, mem, views2)
    print("seam 6': statuses %s after phi (%s before)" % (tri2["counts"].tolist(), chain["tri"]["counts"].tolist()))
    TR.assert_same(tri2, want, "second triangulation")
    ref = B.bundle_adjust(tb, mem, views2, tri2["X"], tri2["status"], tri2["obs_state"])
    gap = abs(ba2.cost_final - ref["cost_final"]) / ref["cost_final"]
    dist = B.state_distance(dict(R=ba2.R, c=ba2.c, X=chain["ba2_X"]), ref, dict(R=views2["R"], c=views2["c"], X=tri2["X"]))
    bounds = (ROUNDOFF_FACTOR * BA2_COST_GAP, ROUNDOFF_FACTOR * BA2_STATE_DISTANCE)
    print("seam 6': cost %.15g against %.15g, gap %.3g (bound %.3g), state distance %.3g (bound %.3g); start %.6g against the focal run's %.6g; %s" %
          (ba2.cost_final, ref["cost_final"], gap, bounds[0], dist, bounds[1], ba2.cost_initial, baf.cost_initial, ba2.report()))
    assert (ba2.n_obs, ba2.n_points, ba2.n_free_cams) == (ref["n_obs"], ref["n_points"], ref["n_free_cams"])
    assert gap <= bounds[0]
    assert dist <= bounds[1]
    assert ba2.cost_initial <= baf.cost_initial
    # the dispatch promise: all focals held == the pose-only entry at fx0 * phi, fy0 * phi
    assert ba3.n_free_focals == 0 and same_bits(ba3.focal, chain["phi"])
    assert same_bits(ba3.R, ba2.R) and same_bits(ba3.c, ba2.c) and same_bits(chain["ba3_X"], chain["ba2_X"])
    assert ba3.report() == ba2.report()


@pytest.mark.gpu
def test_seam7_against_ground_truth(chain):
    """Rotation, centre, median point and focal error at the three stations, each within twice the CPU leg's constant; every
    improvement the CPU leg shows from one station to the next is shown by the device too."""
    scene = CR.make_filtered_scene()
    fig = device_figures(scene, chain)
    print("seam 7': %s; focal %.4e -> %.4e (CPU leg %s; %.4e -> %.4e)" %
          ({k: fig[k] for k in STATIONS}, fig["focal_before"], fig["focal_after"], CPU, CPU_FOCAL_BEFORE, CPU_FOCAL_AFTER))
    for st in STATIONS:
        for k, v in CPU[st].items():
            assert fig[st][k] <= GT_FACTOR * v, (st, k)
    assert fig["focal_after"] <= GT_FACTOR * CPU_FOCAL_AFTER
    assert fig["focal_after"] < fig["focal_before"]
    for a, b in zip(STATIONS[:-1], STATIONS[1:]):
        for k in CPU[a]:
            if CPU[b][k] < CPU[a][k]:
                assert fig[b][k] < fig[a][k], (a, b, k)
    assert fig["before"]["n_points"] >= 200


@pytest.mark.gpu
def test_seam8_bits_are_repeatable(eng, chain):
    again = device_chain(eng, CR.make_filtered_scene())
    assert same_bits(again["rec"], chain["rec"]) and same_bits(again["frec"], chain["frec"])
    assert all(np.array_equal(a, b) for a, b in zip(again["masks"], chain["masks"]))
    for k in ("keep", "n_tri", "n_good", "R", "c", "phi", "baf_X", "ba2_X", "ba3_X"):
        assert same_bits(again[k], chain[k]), k
    assert again["summary"] == chain["summary"]
    assert (again["rot_iters"], again["rot_used"], again["trn_iters"], again["trn_used"]) == \
        (chain["rot_iters"], chain["rot_used"], chain["trn_iters"], chain["trn_used"])
    assert again["tracks"] == chain["tracks"]
    TR.assert_same(again["tri"], chain["tri"], "second run")
    TR.assert_same(again["tri2"], chain["tri2"], "second run, second triangulation")
    for k in ("baf", "ba2", "ba3"):
        assert same_bits(again[k].R, chain[k].R) and same_bits(again[k].c, chain[k].c) and again[k].report() == chain[k].report(), k
