"""K1's n-point refit builds its 9x9 normal matrix from the 36 distinct monomials of the design row (two sweeps of 18
accumulators, csrc/pgi_normal_monomials.hpp) while the oracle keeps the 45 products of the upper triangle: the device must
still return the oracle's bytes -- every edge record and every inlier mask.

One ragged batch of 70 pairs (5, 63, 64, 65, 130, 400 and 1400 rows: NaN padding of the last 64-row step, a single step, and
the hybrid LDS / L2 tail at every wavefront count -- 400 rows are hybrid at one wavefront per pair, 1400 at four), inlier
ratio 0.5, at PGI_K1_NW = 1, 2, 4.  lo_linear_pct = 0 sends every refit through the Nister back-end, which consumes the
whole 9x9 matrix, so a wrong entry anywhere shows; 35 is the default mix.  Pose guesses run the refit at 1.5 thr through
the one-wavefront builder (guess_mode 0) and through the rotation-guided path (guess_mode 1); lo_graph_cut = 9 feeds the
builder a labelling instead of the rows inside the bound.  The oracle's answers are computed once per setting and shared
by the three wavefront counts."""
import os

import numpy as np
import pytest

import oracle_lib as O
from pyposegraphbuilder import synthetic as S

pytestmark = pytest.mark.gpu

SIZES = ([5, 63, 64, 65, 130, 400, 1400] * 10)[:70]
THR, SEED, BASE = 7.5e-4, 17, 52000
DEFAULTS = dict(lo_iters=2, lo_linear_pct=35, guess_mode=0, lo_graph_cut=0)

_batch = {}
_oracle = {}


def batch():
    if not _batch:
        ids = np.arange(BASE, BASE + len(SIZES))
        parts = [S.make_pair(int(i), n, inlier_ratio=0.5) for i, n in zip(ids, SIZES)]
        for k in ("x1", "y1", "x2", "y2"):
            _batch[k] = np.concatenate([p[k] for p in parts])
        _batch["offsets"] = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
        rng = np.random.default_rng(3)
        guesses = np.zeros((len(SIZES), 12))
        for i, p in enumerate(parts):  # a rotation half a degree off (every seventh: 40 degrees, the fit falls through to RANSAC)
            Rg = S.rodrigues(rng.standard_normal(3), np.deg2rad(0.5 if i % 7 else 40.0)) @ p["R"]
            guesses[i] = np.r_[Rg.ravel(), p["t"] if i % 3 else rng.standard_normal(3)]
        _batch["guesses"] = guesses
        _batch["has_guess"] = (rng.random(len(SIZES)) < 0.8).astype(np.uint8)
    return _batch


def oracle(with_guesses, **kw):
    key = (with_guesses,) + tuple(sorted(kw.items()))
    if key not in _oracle:
        b = batch()
        g = dict(guesses=b["guesses"], has_guess=b["has_guess"]) if with_guesses else {}
        _oracle[key] = O.estimate_pose_batch(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], THR, O.default_params(**kw), SEED,
                                             pair_id_base=BASE, **g)
    return _oracle[key]


@pytest.fixture(scope="module", params=[1, 2, 4])
def nw_engine(request):
    """one context per wavefront count (the context reads PGI_K1_NW when it is created), the batch uploaded with and without guesses"""
    from pyposegraphbuilder import Engine
    old = os.environ.get("PGI_K1_NW")
    os.environ["PGI_K1_NW"] = str(request.param)
    try:
        e = Engine()
    finally:
        if old is None:
            del os.environ["PGI_K1_NW"]
        else:
            os.environ["PGI_K1_NW"] = old
    b = batch()
    rows = (b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], THR)
    dbs = {False: e.upload(*rows, seed=SEED, pair_id_base=BASE),
           True: e.upload(*rows, guesses=b["guesses"], has_guess=b["has_guess"], seed=SEED, pair_id_base=BASE)}
    yield request.param, e, dbs
    e.close()


def run_and_compare(nw_engine, with_guesses, **kw):
    nw, e, dbs = nw_engine
    exp, emasks = oracle(with_guesses, **kw)
    e.set_params(**{**DEFAULTS, **kw})
    try:
        edges, masks = e.estimate_pose_batch(dbs[with_guesses])
        got, gmasks = e.edges_to_numpy(edges), masks.cpu().numpy()
    finally:
        e.set_params(**DEFAULTS)
    differing = {f: int(np.sum(np.any((got[f] != exp[f]).reshape(len(got), -1), axis=1))) for f in got.dtype.names
                 if got[f].tobytes() != exp[f].tobytes()}
    print("NW=%d guesses=%s %s: pairs with a differing field %s, mask rows differing %d, refits %d, ok %d" % (
        nw, with_guesses, kw, differing, int(np.sum(gmasks != emasks)), int(exp["lo_runs"].sum()), int((exp["status"] == 1).sum())))
    assert gmasks.tobytes() == emasks.tobytes()
    assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), differing
    return exp


@pytest.mark.parametrize("lo_linear_pct", [0, 35])
@pytest.mark.parametrize("lo_iters", [0, 2])
def test_refit_settings_give_the_oracles_bytes(nw_engine, lo_iters, lo_linear_pct):
    exp = run_and_compare(nw_engine, False, lo_iters=lo_iters, lo_linear_pct=lo_linear_pct)
    assert (exp["lo_runs"].sum() > 0) == (lo_iters > 0)  # the refits did run where they are switched on
    assert (exp["status"] == 1).sum() >= 50                # (the 5-row pairs may fail; every larger one fits)


@pytest.mark.parametrize("guess_mode,lo_linear_pct", [(0, 35), (0, 0), (1, 35)])
def test_guess_paths_give_the_oracles_bytes(nw_engine, guess_mode, lo_linear_pct):
    exp = run_and_compare(nw_engine, True, guess_mode=guess_mode, lo_linear_pct=lo_linear_pct)
    assert exp["used_guess"].sum() >= 20


@pytest.mark.parametrize("lo_linear_pct", [35, 0])
def test_graph_cut_labelling_gives_the_oracles_bytes(nw_engine, lo_linear_pct):
    exp = run_and_compare(nw_engine, False, lo_graph_cut=9, lo_linear_pct=lo_linear_pct)
    plain, _ = oracle(False, lo_iters=2, lo_linear_pct=lo_linear_pct)
    assert exp["E"].tobytes() != plain["E"].tobytes()  # the labelling is not a no-op on this batch
