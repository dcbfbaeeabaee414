"""Cycle-consistency edge filter at scale (not part of bench.py): pgi_cycle_filter_edges on the view graph of the dense
V = 5000, k = 40 scene that `bench.py --full` uses (tests/scene_drivers.py "v5000": 106 151 pairs).  Only the graph is
needed, so the scene is generated with one correspondence row per pair; its 3 % wrong pairs get a random pose, every record
is PGI_EDGE_OK.

Prints the triangle count, the HIP-event time of the device part (uploads of the adjacency and clears; the two kernels) as
the library reports it under PGI_CYCLE_TRACE=1, and the wall time of the whole call, host adjacency included: medians of the
warm calls.  Numbers: DESIGN.md section 6.

    python scripts/cycle_filter_bench.py [repetitions]
"""
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pose-graph-initialization_amd"), os.path.join(ROOT, "tests")]
os.environ["PGI_CYCLE_TRACE"] = "1"

import torch  # noqa: E402
from pyposegraphbuilder import EDGE_DTYPE, Engine, synthetic as S  # noqa: E402
import cycle_scenes as SC  # noqa: E402


def captured_stderr(fn):
    """Runs fn with file descriptor 2 redirected to a file (the library writes its trace line there). -> (result, text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    V, k = 5000, 40
    t0 = time.perf_counter()
    g = S.make_scene_graph_dense(V, k=k, seed=11, outlier_pair_frac=0.03, median_corr=1, min_corr=1, max_corr=1)
    pairs, wrong = g["pairs"], g["wrong"]
    P = len(pairs)
    rec = np.zeros(P, EDGE_DTYPE)
    rec["R"], rec["t"], rec["status"] = g["batch"]["R"].reshape(P, 9), g["batch"]["t"], 1
    rng = np.random.default_rng(1)
    for p in np.nonzero(wrong)[0]:
        rec["R"][p] = SC.random_rotation(rng).reshape(9)
        v = rng.standard_normal(3)
        rec["t"][p] = v / np.linalg.norm(v)
    print("graph: %d views, %d pairs (%d with a random pose), generated in %.1f s" % (V, P, wrong.sum(), time.perf_counter() - t0))
    eng = Engine()
    table = torch.from_numpy(rec.view(np.uint8).reshape(P, 200)).to(eng.device)
    out = torch.empty_like(table)
    src, dst = pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32)
    wall, dev, kern = [], [], []
    summary = None
    for r in range(reps + 2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        (keep, n_tri, n_good, summary), text = captured_stderr(lambda: eng.cycle_filter_edges(table, src, dst, V, out=out))
        dt = time.perf_counter() - t
        m = re.search(r"device ([0-9.]+) ms \(uploads and clears ([0-9.]+) ms, kernels ([0-9.]+) ms\)", text)
        if m is None:
            raise RuntimeError("no trace line from the library: %r" % text)
        if r >= 2:   # two warm-up calls
            wall.append(dt * 1e3)
            dev.append(float(m.group(1)))
            kern.append(float(m.group(3)))
    status = out.cpu().numpy().view(EDGE_DTYPE).reshape(-1)["status"]
    kept = keep.cpu().numpy().astype(bool)
    assert (status == np.where(kept, 1, -4)).all() and int(n_tri.sum().item()) == 3 * summary["n_triangles"]
    print("summary: %s" % summary)
    print("wrong pairs dropped: %d of %d; true pairs dropped: %d of %d" % ((wrong & ~kept).sum(), wrong.sum(), (~wrong & ~kept).sum(), (~wrong).sum()))
    med = lambda a: float(np.median(a))
    print("triangles %d | device part %.3f ms (kernels %.3f ms) | whole call %.3f ms wall (host adjacency and copies: %.3f ms) | "
          "median of %d warm calls, min wall %.3f ms" %
          (summary["n_triangles"], med(dev), med(kern), med(wall), med(wall) - med(dev), reps, min(wall)))
    eng.close()


if __name__ == "__main__":
    main()
