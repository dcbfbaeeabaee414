"""bench.py's final stdout line must stay parseable by the driver (the r05 line had grown to 42 KB,
the driver's bounded tail cut it, `parsed: null`); a plain run prints the line alone, --dump-outputs writes what the timed
path returned.  Host logic only (no GPU, no oracle) but for the one run of the script itself."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _full_record():
    # the complete r05 record (42 KB as one line): the very object whose one-line form the driver could not parse
    return json.load(open(os.path.join(ROOT, "profiles", "r05_bench.json")))


CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def test_compact_line_of_the_r05_record_fits_and_parses():
    B = _bench()
    out = _full_record()
    assert len(json.dumps(out)) > 30000
    line = B.compact_line(out, "bench_full.json")
    assert "\n" not in line and len(line.encode()) < 8192
    j = json.loads(line)
    for k in CONTRACT:
        assert k in j, k
    assert j["value"] == out["value"] and j["ms_per_step"] == out["ms_per_step"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms"):
        assert k in j["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in j["cpu_baseline"], k
    assert j["config"]["workload"].startswith("configs[1]")
    assert "summary" in j and j["summary"]["k1_edges_per_s"] == out["value"]
    assert j["quality"]["rot_err_auc_at_5deg"] == out["quality"]["rot_err_auc_at_5deg"]


@pytest.mark.parametrize("blow", [10, 1000])
def test_compact_line_survives_a_record_that_keeps_growing(blow):
    B = _bench()
    out = _full_record()
    out["graphs"]["more"] = [{"all_repetitions_stage_s": list(range(200))} for _ in range(blow)]
    out["roofline"]["note"] = "x" * 5000
    out["cpu_baseline"]["sample"] = "y" * 5000
    out["config"]["exchange"] = "z" * 5000
    out["summary"] = dict(B.compact_summary(out), **{"extra_%d" % i: "w" * 200 for i in range(blow)})
    line = B.compact_line(out, "bench_full.json")
    assert len(line.encode()) < 8192
    j = json.loads(line)
    for k in CONTRACT:
        assert k in j, k
    assert j["roofline"]["frac"] == pytest.approx(out["roofline"]["frac"], rel=1e-5)


def test_emit_prints_the_line_last_and_writes_the_full_record(tmp_path, capsys, monkeypatch):
    B = _bench()
    out = _full_record()
    monkeypatch.setenv("PGI_BENCH_FULL", str(tmp_path / "bench_full.json"))
    B.emit(out)
    cap = capsys.readouterr()
    lines = cap.out.splitlines()
    assert len(lines) == 1 and json.loads(lines[-1])["metric"] == out["metric"]
    assert json.load(open(tmp_path / "bench_full.json")) == out
    assert "bench_full.json" in cap.err


def test_plain_run_prints_the_line_and_writes_no_record(tmp_path, capsys, monkeypatch):
    """Without --full the record has the contract's keys and the timed kernel's roofline only: one line, no file."""
    B = _bench()
    full = _full_record()
    out = {k: full[k] for k in CONTRACT if k != "cpu_baseline"}
    monkeypatch.setenv("PGI_BENCH_FULL", str(tmp_path / "bench_full.json"))
    B.emit(out, write_full=False)
    cap = capsys.readouterr()
    lines = cap.out.splitlines()
    assert len(lines) == 1 and not os.path.exists(tmp_path / "bench_full.json")
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert j[k] == out[k], k
    assert "full_record" not in j and "cpu_baseline" not in j and "summary" not in j


def _fake_outputs(P, n, seed=3):
    import numpy as np
    B = _bench()
    import pyposegraphbuilder._lib as L
    rng = np.random.default_rng(seed)
    e = np.zeros(P, L.EDGE_DTYPE)
    for name in e.dtype.names:
        e[name] = rng.standard_normal(e[name].shape) if e[name].dtype == np.float64 else rng.integers(0, 1000, e[name].shape)
    masks = (rng.random(P * n) < 0.5).astype(np.uint8)
    return B, np, e, masks, np.arange(P + 1, dtype=np.int64) * n


def test_dump_outputs_writes_every_field_as_float(tmp_path):
    B, np, e, masks, offsets = _fake_outputs(37, 301)
    B.dump_outputs(str(tmp_path / "d"), e, masks, offsets)
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == sorted(["edges_%s.npy" % k for k in e.dtype.names] + ["mask_inliers_per_pair.npy", "masks.npy"])
    for f in files:
        assert np.load(tmp_path / "d" / f).dtype in (np.float32, np.float64), f
    assert np.array_equal(np.load(tmp_path / "d" / "edges_E.npy"), e["E"])
    assert np.array_equal(np.load(tmp_path / "d" / "edges_n_inl.npy"), e["n_inl"].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "d" / "masks.npy"), masks.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "mask_inliers_per_pair.npy"), masks.reshape(37, 301).sum(1))


def test_dump_outputs_samples_a_mask_that_would_not_fit(tmp_path):
    """17 M mask rows are 68 MB as f32: a fixed, seeded sample of rows is stored with its row numbers, the same in every run,
    and the files together stay below 64 MB."""
    B, np, e, masks, offsets = _fake_outputs(17, 1000003)
    for d in ("a", "b"):
        B.dump_outputs(str(tmp_path / d), e, masks, offsets)
    files = os.listdir(tmp_path / "a")
    assert "masks.npy" not in files and "masks_sample.npy" in files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    rows = np.load(tmp_path / "a" / "masks_sample_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "b" / "masks_sample_rows.npy"))
    assert len(rows) == B.DUMP_MASK_SAMPLE and np.all(np.diff(rows) > 0) and rows[-1] < len(masks)
    assert np.array_equal(np.load(tmp_path / "a" / "masks_sample.npy"), masks[rows.astype(np.int64)].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "mask_inliers_per_pair.npy"), masks.reshape(17, 1000003).sum(1))


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_asked_for_and_dumps_what_the_path_returned(tmp_path):
    """bench.py as the driver starts it (small batch): --steps sets the timed steps, the line carries ms_per_step and none of the
    --full legs, and --dump-outputs holds exactly what Engine.estimate_pose_batch returns for the same inputs."""
    import subprocess
    import sys
    import numpy as np
    from pyposegraphbuilder import Engine, synthetic as S
    P, n = 48, 301
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", str(P),
                        "--corrs", str(n), "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PGI_BENCH_FULL=str(tmp_path / "bench_full.json")))
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.splitlines()[-1])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["unit"] == "edges/s" and j["higher_is_better"] is True
    assert j["value"] == pytest.approx(P / (j["ms_per_step"] * 1e-3), rel=1e-2)
    for k in ("cpu_baseline", "quality", "summary", "exchange_verified"):
        assert k not in j, k
    assert not os.path.exists(tmp_path / "bench_full.json")
    b = S.make_batch(np.arange(P), n, inlier_ratio=0.5)
    eng = Engine()
    db = eng.upload(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], 0.75 / S.FOCAL_PX, seed=0xB0BA, pair_id_base=0)
    edges, masks = eng.estimate_pose_batch(db)
    exp = eng.edges_to_numpy(edges)
    for name in exp.dtype.names:
        got = np.load(tmp_path / "out" / ("edges_%s.npy" % name))
        assert got.dtype in (np.float32, np.float64) and np.array_equal(got, exp[name]), name
    assert np.array_equal(np.load(tmp_path / "out" / "masks.npy"), masks.cpu().numpy().astype(np.float32))
    eng.close()
