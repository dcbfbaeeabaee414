"""Cycle-consistency edge filter (include/pgi.h: pgi_cycle_filter, pgi_cycle_filter_edges) against its specification
tests/cycle_spec.py.  Every output is an integer, so the GPU tests demand equality.

The defaults (5 deg loop rotation, 15 deg coplanarity, 5 deg collinearity, one good triangle) are choices.  Measured with
the specification on the CPU leg's estimated edges of the chain scene (chain_ref.reference_chain): 120 triangles, all inside
the main component; the largest loop rotation error is CHAIN_MAX_LOOP_ROT_DEG = 0.571188 degrees and the largest coplanarity
angle CHAIN_MAX_COPLANARITY_DEG = 8.117065 degrees; two triangles skip the translation test.  No true edge of that scene
fails a default, so the defaults stand as the issue states them.

The value scene (cycle_scenes.value_scene: 60 views, ring plus 240 chords, 0.3 deg / 1 deg noise, 45 of 300 records replaced
by random poses), CPU only, specification + oracle/rotavg_oracle.py: VALUE_BAD_SURVIVE = 0 corrupted records survive,
VALUE_TRUE_DROPPED = 2 of 255 true records are dropped, the mean rotation error against ground truth is
VALUE_ROT_ERR_FILTERED = 0.122759 degrees with the filter and VALUE_ROT_ERR_UNFILTERED = 90.068417 degrees without (the
unfiltered solve starts from a spanning tree that runs through corrupted records and does not recover).  The GPU seam test takes its bound from
the first (GT_FACTOR of tests/test_chain.py).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import chain_ref as CR
import cycle_scenes as SC
import cycle_spec as CS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rotavg_oracle as RO  # noqa: E402

CHAIN_MAX_LOOP_ROT_DEG = 0.571188
CHAIN_MAX_COPLANARITY_DEG = 8.117065
VALUE_BAD_SURVIVE = 0
VALUE_TRUE_DROPPED = 2
VALUE_ROT_ERR_FILTERED = 0.122759
VALUE_ROT_ERR_UNFILTERED = 90.068417
GT_FACTOR = 2.0   # the rule of tests/test_chain.py: a device figure against ground truth may be twice the CPU leg's


def spec_of(sc, **params):
    return CS.cycle_filter(sc["n_views"], sc["src"], sc["dst"], sc["R"], sc["t"], sc["status"], details=True, **params)


def rotate_about(axis, deg):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.radians(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


# ---- CPU: hand-checked cases of the specification ------------------------------------------------------------------------
def test_exact_triangle_is_good_in_every_orientation():
    want = None
    for pattern in range(8):
        out = spec_of(SC.triangle(pattern))
        assert out["summary"] == dict(n_triangles=1, n_good=1, n_skipped_translation=0, n_ok=3, n_dropped=0), pattern
        assert out["keep"].tolist() == [1, 1, 1] and out["n_tri"].tolist() == [1, 1, 1] and out["n_good"].tolist() == [1, 1, 1]
        q = out["quantities"][0]
        assert q["trace"] == pytest.approx(3.0, abs=1e-12) and abs(q["un"]) < 1e-12 and q["o1"] > 0 and q["o2"] > 0
        got = (out["keep"].tolist(), out["n_tri"].tolist(), out["n_good"].tolist(), out["summary"])
        want = want or got
        assert got == want


def test_rotation_off_by_ten_degrees_fails_the_rotation_test():
    for pattern in (0, 5):
        sc = SC.triangle(pattern)
        sc["R"][1] = rotate_about([1, 2, 3], 10.0) @ sc["R"][1]
        out = spec_of(sc)
        q = out["quantities"][0]
        assert q["trace"] == pytest.approx(1 + 2 * np.cos(np.radians(10.0)), abs=1e-12)
        assert out["summary"]["n_good"] == 0 and out["keep"].tolist() == [0, 0, 0] and out["summary"]["n_dropped"] == 3
        assert spec_of(sc, rot_thr_deg=10.5, trn_thr_deg=90.0)["good"].tolist() == [True]   # (coplanarity opened: the rotation decides)


def test_negated_translation_fails_the_orientation_test():
    for p in range(3):
        sc = SC.triangle(0)
        sc["t"][p] = -sc["t"][p]
        out = spec_of(sc)
        q = out["quantities"][0]
        assert q["trace"] == pytest.approx(3.0, abs=1e-12) and abs(q["un"]) < 1e-12   # rotations exact, still coplanar
        assert q["n2"] >= CS.thresholds(CS.DEFAULTS)[2] and (q["o1"] <= 0 or q["o2"] <= 0)
        assert out["good"].tolist() == [False] and out["keep"].tolist() == [0, 0, 0]


def test_translation_tilted_out_of_the_plane_fails_coplanarity():
    sc = SC.triangle(0)
    q0 = spec_of(sc)["quantities"][0]
    # the record (0, 2) is stored as 2 <- 0; u3 = t_ac is its inverse's t.  Tilt u3 by 30 degrees towards the plane's normal.
    R_ac, u3 = SC.invert(sc["R"][2], sc["t"][2])
    R_ba, t_ba = sc["R"][0], sc["t"][0]
    u1 = R_ba.T @ t_ba
    u2 = R_ba.T @ (sc["R"][1].T @ sc["t"][1])
    n = np.cross(u1, u2)
    n /= np.linalg.norm(n)
    tilted = np.cos(np.radians(30.0)) * u3 + np.sin(np.radians(30.0)) * n
    R_ca, t_ca = SC.invert(R_ac, tilted)
    sc["t"][2] = t_ca
    out = spec_of(sc)
    q = out["quantities"][0]
    _, cop = CS.loop_angles_deg([q])
    assert cop[0] == pytest.approx(30.0, abs=1e-9) and q["trace"] == pytest.approx(q0["trace"], abs=1e-12)
    assert q["o1"] > 0 and q["o2"] > 0                      # the in-plane part still closes: only coplanarity fails
    assert out["good"].tolist() == [False]
    assert spec_of(sc, trn_thr_deg=31.0)["good"].tolist() == [True]


def test_collinear_centres_skip_the_translation_test():
    sc = SC.collinear_triangle()
    out = spec_of(sc)
    assert out["summary"] == dict(n_triangles=1, n_good=1, n_skipped_translation=1, n_ok=3, n_dropped=0)
    sc["t"][1] = -sc["t"][1]                                # would fail the orientation test if it were applied
    assert spec_of(sc)["summary"]["n_good"] == 1
    sc["R"][1] = rotate_about([0, 0, 1], 10.0) @ sc["R"][1]
    out = spec_of(sc)
    assert out["summary"]["n_good"] == 0 and out["summary"]["n_skipped_translation"] == 1


def test_bridge_and_keep_untested():
    sc = SC.bridge()
    assert spec_of(sc)["keep"].tolist() == [1, 1, 1, 1]
    out = spec_of(sc, keep_untested=0)
    assert out["keep"].tolist() == [1, 1, 1, 0] and out["n_tri"].tolist() == [1, 1, 1, 0] and out["summary"]["n_dropped"] == 1


def test_k4_drops_the_corrupted_edge_only():
    out = spec_of(SC.k4())
    assert out["keep"].tolist() == [0, 1, 1, 1, 1, 1] and out["n_tri"].tolist() == [2] * 6
    assert out["n_good"].tolist() == [0, 1, 1, 1, 1, 2] and out["summary"]["n_good"] == 2


def test_validation():
    sc = SC.triangle(0)
    a = (sc["n_views"], sc["src"], sc["dst"], sc["R"], sc["t"])
    for kw in (dict(rot_thr_deg=0.0), dict(trn_thr_deg=90.5), dict(collinear_thr_deg=-1.0), dict(min_good=0)):
        with pytest.raises(ValueError):
            CS.cycle_filter(*a, **kw)
    with pytest.raises(ValueError):
        CS.cycle_filter(2, *a[1:])
    with pytest.raises(ValueError):
        CS.cycle_filter(3, [0, 1, 1], [1, 2, 1], sc["R"], sc["t"])
    with pytest.raises(ValueError):
        CS.cycle_filter(3, [0, 1, 1], [1, 2, 0], sc["R"], sc["t"])                  # (1, 0) repeats (0, 1)
    assert CS.cycle_filter(3, [0, 1, 1], [1, 2, 0], sc["R"], sc["t"], [1, 1, 0])["keep"].tolist() == [1, 1, 0]   # not OK: ignored


def test_enumeration_equals_the_triple_loop():
    sc = SC.random_graph()
    V, ok = sc["n_views"], sc["status"] == CS.EDGE_OK
    assert V == 40 and len(ok) == 200 and 25 <= (~ok).sum() <= 55
    A = np.zeros((V, V), bool)
    A[sc["src"][ok], sc["dst"][ok]] = A[sc["dst"][ok], sc["src"][ok]] = True
    brute = [(a, b, c) for a in range(V) for b in range(a + 1, V) for c in range(b + 1, V) if A[a, b] and A[b, c] and A[a, c]]
    tri, index = CS.triangles(V, sc["src"], sc["dst"], sc["status"])
    assert [t[:3] for t in tri] == brute and len(brute) > 20
    for a, b, c, pab, pbc, pac in tri:
        for p, pair in ((pab, {a, b}), (pbc, {b, c}), (pac, {a, c})):
            assert {int(sc["src"][p]), int(sc["dst"][p])} == pair and ok[p]
    out = spec_of(sc)
    cnt = np.zeros(len(ok), int)
    for t in tri:
        cnt[list(t[3:])] += 1
    assert np.array_equal(out["n_tri"], cnt) and not out["n_tri"][~ok].any() and not out["keep"][~ok].any()


def test_chain_scene_keeps_every_true_edge():
    ref = CR.reference_chain()
    src, dst, Rrel, t, _ = ref["graph"]
    out = CS.cycle_filter(CR.N_VIEWS, src, dst, Rrel, t, details=True)
    main = ref["scene"]["main"]
    inside = np.array([main[a] and main[b] and main[c] for a, b, c, *_ in out["triangles"]])
    rot, cop = CS.loop_angles_deg(out["quantities"])
    print("chain scene: %d triangles, %d in the main component, max loop rotation %.6f deg, max coplanarity angle %.6f deg; %s" %
          (len(inside), inside.sum(), rot[inside].max(), cop[inside].max(), out["summary"]))
    assert inside.sum() >= 100
    assert all(out["keep"][p] for p in range(len(src)) if main[src[p]] and main[dst[p]])
    assert rot[inside].max() == pytest.approx(CHAIN_MAX_LOOP_ROT_DEG, rel=1e-3)
    assert cop[inside].max() == pytest.approx(CHAIN_MAX_COPLANARITY_DEG, rel=1e-3)
    assert rot[inside].max() < CS.DEFAULTS["rot_thr_deg"] and cop[inside].max() < CS.DEFAULTS["trn_thr_deg"]


@pytest.mark.parametrize("name", sorted(SC.gpu_scenes()))
def test_margin_condition(name):
    """No tested quantity of a scene the GPU tests use lies within 1e-9 (relative) of its threshold, so neither a rounding
    difference of sin / cos nor another operation order on the device can flip a decision."""
    sc = SC.gpu_scenes()[name]
    settings = [dict()] + ([dict(keep_untested=0)] if name == "bridge" else [])
    for kw in settings:
        m = CS.margins(spec_of(sc, **kw)["quantities"], **kw)
        print(name, kw, "margin %.3g" % m)
        assert m > CS.MARGIN


def aligned_rotation_error_deg(R, R_gt, views):
    """Mean angle of R_v Q against R_gt_v over `views`, Q the rotation that fits best (chordal mean of R_v^T R_gt_v)."""
    M = sum(R[v].T @ R_gt[v] for v in views)
    U, _, Vt = np.linalg.svd(M)
    Q = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    ang = [np.degrees(np.arccos(np.clip((np.trace(R[v] @ Q @ R_gt[v].T) - 1) / 2, -1, 1))) for v in views]
    return float(np.mean(ang))


def value_figures():
    sc = SC.value_scene()
    out = spec_of(sc)
    keep, bad = out["keep"].astype(bool), sc["bad"]
    V = sc["n_views"]
    assert CR.largest_component(V, sc["src"][keep], sc["dst"][keep]).all()   # the kept edges still join every view
    views = list(range(V))
    w = np.ones(len(keep))
    R_f, _ = RO.rotation_average(V, sc["src"][keep], sc["dst"][keep], sc["R"][keep], w[keep])
    R_u, _ = RO.rotation_average(V, sc["src"], sc["dst"], sc["R"], w)
    tested = bad & (out["n_tri"] > 0)
    return dict(bad_survive=int((bad & keep).sum()), true_dropped=int((~bad & ~keep).sum()), n_true=int((~bad).sum()),
                bad_tested=int(tested.sum()), bad_tested_dropped=int((tested & ~keep).sum()),
                err_filtered=aligned_rotation_error_deg(np.asarray(R_f).reshape(V, 3, 3), sc["R_gt"], views),
                err_unfiltered=aligned_rotation_error_deg(np.asarray(R_u).reshape(V, 3, 3), sc["R_gt"], views), keep=keep)


def test_value_on_a_corrupted_graph():
    sc = SC.value_scene()
    assert sc["n_views"] == 60 and len(sc["src"]) == 300 and sc["bad"].sum() == 45
    f = value_figures()
    print("value scene: %d corrupted records survive, %d of %d true records dropped, %d of %d tested corrupted records dropped; "
          "mean rotation error %.6f deg with the filter, %.6f deg without" %
          (f["bad_survive"], f["true_dropped"], f["n_true"], f["bad_tested_dropped"], f["bad_tested"], f["err_filtered"], f["err_unfiltered"]))
    assert f["true_dropped"] <= 0.02 * f["n_true"]
    assert f["bad_tested"] > 0 and f["bad_tested_dropped"] >= 0.9 * f["bad_tested"]
    assert f["bad_survive"] == VALUE_BAD_SURVIVE and f["true_dropped"] == VALUE_TRUE_DROPPED
    assert f["err_filtered"] == pytest.approx(VALUE_ROT_ERR_FILTERED, rel=1e-3)
    assert f["err_unfiltered"] == pytest.approx(VALUE_ROT_ERR_UNFILTERED, rel=1e-3)
    assert f["err_filtered"] < f["err_unfiltered"]


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from pyposegraphbuilder import Engine
    e = Engine()
    yield e
    e.close()


def upload(eng, rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(len(rec), 200).copy()).to(eng.device)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_against_spec(eng, sc, **params):
    """Both entries against the specification: the host arrays (the OK records, every one taking part) and the table."""
    want = spec_of(sc, **params)
    ok = sc["status"] == CS.EDGE_OK
    keep, n_tri, n_good, summary = eng.cycle_filter(sc["src"][ok], sc["dst"][ok], sc["R"][ok], sc["t"][ok], sc["n_views"], **params)
    assert np.array_equal(keep.numpy(), want["keep"][ok])
    assert np.array_equal(as_u32(n_tri), want["n_tri"][ok]) and np.array_equal(as_u32(n_good), want["n_good"][ok])
    assert summary == want["summary"]
    table = upload(eng, SC.edge_table(sc))
    keep, n_tri, n_good, summary = eng.cycle_filter_edges(table, sc["src"], sc["dst"], sc["n_views"], **params)
    assert np.array_equal(keep.cpu().numpy(), want["keep"])
    assert np.array_equal(as_u32(n_tri), want["n_tri"]) and np.array_equal(as_u32(n_good), want["n_good"])
    assert summary == want["summary"]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sorted(SC.gpu_scenes()) if n != "value"])
def test_hip_equals_the_specification(eng, name):
    want = check_against_spec(eng, SC.gpu_scenes()[name])
    if name == "k4":
        assert want["keep"].tolist() == [0, 1, 1, 1, 1, 1]
    if name == "wheel":
        assert want["summary"]["n_triangles"] == SC.WHEEL_RIM and 0 < want["summary"]["n_good"] < SC.WHEEL_RIM
    if name == "bridge":
        assert check_against_spec(eng, SC.bridge(), keep_untested=0)["keep"].tolist() == [1, 1, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "wheel"])
def test_table_entry_writes_the_filtered_table(eng, name):
    import torch
    sc = SC.gpu_scenes()[name]
    want = spec_of(sc)
    rec = SC.edge_table(sc)
    expect = rec.copy()
    expect["status"] = CS.filtered_status(rec["status"], want["keep"])
    assert (expect["status"] != rec["status"]).sum() == want["summary"]["n_dropped"] > 0
    table = upload(eng, rec)
    out = torch.full_like(table, 0xA5)
    first = eng.cycle_filter_edges(table, sc["src"], sc["dst"], sc["n_views"], out=out)
    assert out.cpu().numpy().tobytes() == expect.tobytes()                  # every byte; only the status of the dropped differs
    assert table.cpu().numpy().tobytes() == rec.tobytes()                   # the input is untouched
    second = eng.cycle_filter_edges(table, sc["src"], sc["dst"], sc["n_views"], out=torch.full_like(table, 0x5A))
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(a, b)
    assert first[3] == second[3] == want["summary"]
    inplace = table.clone()
    third = eng.cycle_filter_edges(inplace, sc["src"], sc["dst"], sc["n_views"], out=inplace)
    assert inplace.cpu().numpy().tobytes() == expect.tobytes()
    assert torch.equal(third[0], first[0]) and third[3] == first[3]
    # the filtered table run again: the dropped records are no longer OK, the kept ones are judged among themselves
    again = spec_of(dict(sc, status=expect["status"]))
    keep4, _, _, summary4 = eng.cycle_filter_edges(inplace, sc["src"], sc["dst"], sc["n_views"])
    assert np.array_equal(keep4.cpu().numpy(), again["keep"]) and summary4 == again["summary"]


@pytest.mark.gpu
def test_seam_filter_then_rotation_averaging(eng):
    sc = SC.value_scene()
    V = sc["n_views"]
    want = spec_of(sc)
    table = upload(eng, SC.edge_table(sc))
    out = table.clone()
    keep, _, _, summary = eng.cycle_filter_edges(table, sc["src"], sc["dst"], V, out=out)
    assert np.array_equal(keep.cpu().numpy(), want["keep"]) and summary == want["summary"]
    R_f, _, used_f = eng.rotation_average_edges(out, sc["src"], sc["dst"], None, V)
    R_u, _, used_u = eng.rotation_average_edges(table, sc["src"], sc["dst"], None, V)
    assert used_f == int(want["keep"].sum()) and used_u == len(sc["src"])
    views = list(range(V))
    err_f = aligned_rotation_error_deg(R_f, sc["R_gt"], views)
    err_u = aligned_rotation_error_deg(R_u, sc["R_gt"], views)
    print("seam: %d of %d records kept; mean rotation error %.6f deg filtered (CPU %.6f, bound %.6f), %.6f deg unfiltered" %
          (used_f, used_u, err_f, VALUE_ROT_ERR_FILTERED, GT_FACTOR * VALUE_ROT_ERR_FILTERED, err_u))
    assert err_f <= GT_FACTOR * VALUE_ROT_ERR_FILTERED
    assert err_f < err_u


@pytest.mark.gpu
def test_errors_come_through_the_engine(eng):
    from pyposegraphbuilder import PgiError, _lib as L
    sc = SC.triangle(0)
    a = (sc["src"], sc["dst"], sc["R"], sc["t"])
    table = upload(eng, SC.edge_table(sc))
    for kw in (dict(rot_thr_deg=0.0), dict(trn_thr_deg=90.5), dict(collinear_thr_deg=float("nan")), dict(min_good=0)):
        with pytest.raises(PgiError, match="parameters out of range"):
            eng.cycle_filter(*a, 3, **kw)
        with pytest.raises(PgiError, match="parameters out of range"):
            eng.cycle_filter_edges(table, sc["src"], sc["dst"], 3, **kw)
    with pytest.raises(PgiError, match="view id out of range"):
        eng.cycle_filter(*a, 2)
    with pytest.raises(PgiError, match="view id out of range"):
        eng.cycle_filter_edges(table, sc["src"], sc["dst"], 2)
    with pytest.raises(PgiError, match="with itself"):
        eng.cycle_filter([0, 1, 1], [1, 2, 1], sc["R"], sc["t"], 3)
    with pytest.raises(PgiError, match="occurs twice"):
        eng.cycle_filter([0, 1, 1], [1, 2, 0], sc["R"], sc["t"], 3)
    with pytest.raises(PgiError, match="occurs twice"):
        eng.cycle_filter_edges(table, [0, 1, 1], [1, 2, 0], 3)
    with pytest.raises(TypeError):
        eng.cycle_filter(*a, 3, no_such_parameter=1)
    # a duplicate among records that are not OK is no error
    rec = SC.edge_table(sc)
    rec["status"][2] = 0
    keep, _, _, summary = eng.cycle_filter_edges(upload(eng, rec), [0, 1, 1], [1, 2, 0], 3)
    assert keep.cpu().numpy().tolist() == [1, 1, 0] and summary["n_ok"] == 2 and summary["n_triangles"] == 0
    # a NULL context returns PGI_ERR_INVALID from both entries, with a message
    lib = L.load()
    s = L.CycleSummary()
    assert lib.pgi_cycle_filter(None, None, 0, 0, None, None, None, None, C.byref(s)) == -1
    assert lib.pgi_cycle_filter_edges(None, None, None, None, 0, 0, None, None, None, None, C.byref(s), None) == -1
    assert "null" in L.last_error()
    # ... and the engine keeps working
    assert eng.cycle_filter(*a, 3)[3]["n_good"] == 1
