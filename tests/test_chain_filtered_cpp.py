"""The filtered chain through PoseGraphBuilder (tests/cpp/test_chain_filtered.cpp): on the correspondences of the filtered chain
scene (tests/chain_ref.py) estimateAndAverage gives the Python chain's table, filterEdgesByCycles (device-table overload) its
keep mask, counts, summary and filtered records, and averageTranslations on the filtered table its positions and counts, bit
for bit.  Left out: PoseGraphBuilder has no call that averages the ROTATIONS of a device table (averageRotations takes a pose
graph), so the driver receives the Python chain's rotations; the rotation side of the filtered table is checked through the
Python engine only (tests/test_chain_filtered.py, seam 1')."""
import os
import struct
import subprocess

import numpy as np
import pytest

import chain_ref as CR
from test_chain_filtered import chain, eng, same_bits  # noqa: F401  (the module fixtures of the Python chain)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pose-graph-initialization_amd", "test_chain_filtered")


def test_cpp_driver_is_built():
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_cpp_filter_then_average_on_the_filtered_table(tmp_path, chain):  # noqa: F811
    from pyposegraphbuilder import _lib as L
    scene = CR.make_filtered_scene()
    V, P = CR.N_VIEWS, len(scene["pairs"])
    path, out = str(tmp_path / "pairs.bin"), str(tmp_path / "result.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<IIII", V, P, CR.ESTIMATOR_SEED, 0))
        for p, (s, d) in enumerate(scene["pairs"]):
            rows = chain["corr"][p]          # the device's float32 rows, widened exactly
            f.write(struct.pack("<IIId", s, d, len(rows), float(chain["thr"][p])))
            f.write(np.ascontiguousarray(rows, "<f8").tobytes())
        f.write(np.ascontiguousarray(chain["R"], "<f8").tobytes())
    r = subprocess.run([EXE, path, out], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "input table untouched; in place same table" in r.stdout
    with open(out, "rb") as f:
        rec = np.frombuffer(f.read(200 * P), L.EDGE_DTYPE)
        keep = np.frombuffer(f.read(P), np.uint8)
        n_tri = np.frombuffer(f.read(4 * P), "<u4")
        n_good = np.frombuffer(f.read(4 * P), "<u4")
        summary = dict(zip(("n_triangles", "n_good", "n_skipped_translation", "n_ok", "n_dropped"), struct.unpack("<QQQII", f.read(32))))
        frec = np.frombuffer(f.read(200 * P), L.EDGE_DTYPE)
        head = struct.unpack("<II", f.read(8))
        c = np.frombuffer(f.read(24 * V), "<f8").reshape(V, 3)
        assert f.read() == b""
    assert same_bits(rec, chain["rec"])
    assert np.array_equal(keep, chain["keep"]) and np.array_equal(n_tri, chain["n_tri"]) and np.array_equal(n_good, chain["n_good"])
    assert summary == chain["summary"]
    assert same_bits(frec, chain["frec"])
    assert head == (chain["trn_iters"], chain["trn_used"]) and head[1] == int(chain["okf"].sum())
    assert same_bits(c, chain["c"])
