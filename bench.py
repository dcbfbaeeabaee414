#!/usr/bin/env python3
"""bench.py -- pose-graph edges/sec (essential + decompose) on MI355X.

Step   = one pass of the hot path (PoseGraphBuilder::estimatePose, pose_graph_builder.h:940-1078)
         over one batch of synthetic image pairs already resident in HBM: robust essential
         matrix (5-point hypotheses, multi-level Sampson scoring, n-point LO), inlier mask and
         decomposition to (R, t), one kernel launch -- followed, when N > 1, by the RCCL
         all-gather of the per-edge records (the only exchange step of the path).
Workload = BASELINE.json configs[1]: 10 000 pairs x 2 000 correspondences per GPU
         (weak scaling: each rank owns its own 10 000 pairs, ids rank*P ...).
Launch  : python bench.py [--gpus N --steps K --warmup W]; for N > 1 under
         python -m torch.distributed.run --nproc-per-node N ... (one rank per GPU).
Rank 0 prints ONE JSON line.
A plain run sets up, warms up, times the K steps and prints the line (contract keys, `config`, the HBM roofline of the
timed kernel from the timed steps' own HIP events).  --full adds every other leg: quality against the ground truth, the
replayed PMC profile, SURVEY 8d's variants, the graph-level configs 3 / 4 / 5, the secondary kernels, the CPU baseline
with its parity check, and writes the full record to bench_full.json.  --dump-outputs DIR writes what the last timed
step returned (edge records field by field, inlier masks) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "pose-graph-initialization_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
VALU_F32_PEAK_TF = 157.3    # vector fp32 peak
EDGE_RECORD_BYTES = 200     # sizeof(pgi_edge)


def algorithmic_bytes_per_edge(n):
    """rows read once (4 x f32), mask written once (u8), one edge record."""
    return 17 * n + EDGE_RECORD_BYTES


def replay_profile(kind, P, N, L):
    """Counters of the newest committed PMC profile of kernel `kind` ("k1" / "k2"): profiles/rNN_<kind>_pmc.json.
    They are REPLAYED, not measured in this run, and only while the profile was taken from the very kernel sources the
    loaded library was built from (sha256 over csrc/pgi_kernels.hip + pgi_device.hpp, written by scripts/k1_pmc_json.py).
    Returns (profile dict or None, file name or None, reason or None)."""
    import glob
    import re
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc.json" % kind)),
                   key=lambda f: int(re.match(r"r(\d+)_", os.path.basename(f)).group(1)))
    if not cands:
        return None, None, "no profiles/r*_%s_pmc.json" % kind
    f = cands[-1]
    name = "profiles/" + os.path.basename(f)
    try:
        tj = json.load(open(f))
    except Exception as ex:  # noqa: BLE001
        return None, name, "unreadable: %s" % ex
    if P is not None and (tj.get("pairs") != P or tj.get("corrs") != N):
        return None, name, "profiled on another workload (%s x %s)" % (tj.get("pairs"), tj.get("corrs"))
    sha = tj.get("source_sha256")
    if not sha:
        return None, name, "profile carries no source hash (taken before round 3)"
    if sha != (L.kernel_source_sha256() if kind in ("k1", "k2") else L.kernel_source_sha256(tuple(tj.get("source_files") or ("csrc/pgi_match.hip",)))):
        return None, name, "kernel sources changed since the profile was taken (hash mismatch): re-run scripts/profile_k1.sh"
    return tj, name, None


class ClockSampler:
    """The shader clock WHILE a leg runs (a reading before / after the leg is an idle reading): a side thread
    polls the starred line of pp_dpm_sclk every ~2 ms between __enter__ and __exit__; .result() -> {samples, min, median, max}."""

    def __init__(self, period_s=0.002):
        import glob
        self.paths = sorted(glob.glob("/sys/class/drm/card[0-9]*/device/pp_dpm_sclk"))
        self.period, self.vals, self._stop, self._th = period_s, [], False, None

    def _read(self):
        for pth in self.paths:
            try:
                for ln in open(pth).read().splitlines():
                    if ln.strip().endswith("*"):
                        return int("".join(ch for ch in ln.split(":")[1] if ch.isdigit()))
            except Exception:  # noqa: BLE001
                continue
        return None

    def _loop(self):
        while not self._stop:
            v = self._read()
            if v:
                self.vals.append(v)
            time.sleep(self.period)

    def __enter__(self):
        import threading
        if self.paths:
            self._th = threading.Thread(target=self._loop, daemon=True)
            self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self._th:
            self._th.join(timeout=1.0)

    def result(self):
        if not self.vals:
            return None
        v = np.array(self.vals)
        med = int(np.median(v))
        return {"samples": int(len(v)), "min_mhz": int(v.min()), "median_mhz": med, "max_mhz": int(v.max()),
                "source": "pp_dpm_sclk polled by a side thread during the timed calls",
                # (some leases' sysfs keeps showing the idle state -- ~100 MHz -- under full load: such a reading says nothing)
                "plausible": bool(med >= 500)}


def pcie_h2d_peak_gbs(torch, device, mb=256, reps=4):
    """The link's own rate for one large page-locked host -> device copy (what scripts/probes/first_copy_probe.hip measures):
    the yardstick of the graph legs' `convert + upload` stage."""
    h = torch.empty(mb << 20, dtype=torch.uint8).pin_memory()
    d = torch.empty(mb << 20, dtype=torch.uint8, device=device)
    d.copy_(h, non_blocking=True)
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        d.copy_(h, non_blocking=True)
        z.record()
        torch.cuda.synchronize()
        best = max(best, (mb << 20) / (a.elapsed_time(z) * 1e-3) / 1e9)
    return best


def amdahl(total_s, replicated_s):
    """speed-up ceilings of a leg whose `replicated_s` seconds every rank repeats while the rest shards perfectly"""
    total_s = max(total_s, 1e-9)
    rep = min(max(replicated_s, 0.0), total_s)
    return {"n%d" % n: round(total_s / (rep + (total_s - rep) / n), 2) for n in (2, 4, 8)}


REPLICATED_STAGES = ("[Scheduler] candidate order", "[Scheduler] wave formation", "[Pose estimation] pose graph insertion",
                     "[Pose estimation] per-pair arrays (host)", "[Visibility update]")


def graph_companions(g, blob, m, mode, eng, torch, pcie_peak):
    """SURVEY 8d's companions of a graph-level leg: K1's roofline on the leg's own rows (one resident call,
    HIP events), the PCIe share of the upload stage, the stages every rank repeats with the Amdahl ceiling they imply, and --
    config 4 only -- the CPU restatement over the SAME pairs, seeds and mode with every edge compared."""
    from pyposegraphbuilder import synthetic as S
    b = g["batch"]
    P, rows = len(g["pairs"]), int(b["offsets"][-1])
    st = m["stages_s"]
    comp = {}
    if mode == "shard":
        db = eng.upload(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], 7.5e-4, seed=7)
        e_dev, m_dev = eng.estimate_pose_batch(db)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e_dev, m_dev = eng.estimate_pose_batch(db, e_dev, m_dev)
            z.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(z))
        k1_ms = float(np.median(ts))
        k1_bytes = 17 * rows + EDGE_RECORD_BYTES * P
        gbs = k1_bytes / (k1_ms * 1e-3) / 1e9
        comp["roofline"] = {"bound": "hbm", "kernel": "estimate_pose_kernel (all size classes of one call, rows resident)",
                            "kernel_ms": round(k1_ms, 3), "achieved": round(gbs, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(gbs / HBM_PEAK_GBS, 6), "algorithmic_bytes": k1_bytes,
                            "rows_per_s": round(rows / (k1_ms * 1e-3), 1), "share_of_leg": round(k1_ms * 1e-3 / m["seconds"], 3),
                            "traffic": None, "note": "17 B x rows + 200 B x pairs over this run's HIP-event time; K1 is VALU-issue bound by design (DESIGN.md)"}
        res_edges = eng.edges_to_numpy(e_dev)
        del db, e_dev, m_dev
        # CPU restatement over the same pairs, same seed (7, as tests/cpp/test_distributed.cpp), adaptive mode, every host core
        import oracle_lib as O
        cores = int(O.lib().pgo_num_threads())
        t0 = time.perf_counter()
        e_cpu, _mk = O.estimate_pose_batch(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], 7.5e-4, O.default_params(), 7, threads=cores)
        t_cpu = time.perf_counter() - t0
        import scene_drivers as SC
        _hdr, ed = SC.read_shard(blob, P)
        same_leg = bool(np.array_equal(ed["E"], e_cpu["E"]) and np.array_equal(ed["status"], e_cpu["status"]) and np.array_equal(ed["n_inl"], e_cpu["n_inl"]))
        same_res = bool(np.array_equal(res_edges["E"], e_cpu["E"]) and np.array_equal(res_edges["n_inl"], e_cpu["n_inl"]))
        comp["cpu_baseline"] = {"value": round(P / t_cpu, 1), "unit": "pairs/s", "cores": cores, "kind": "port", "seconds": round(t_cpu, 2),
                                "sample": "all %d pairs / %d rows of the leg (pose estimation only: no gather, no averaging); build CPU restatement, not OpenCV" % (P, rows),
                                "gpu_matches_on_sample": same_leg and same_res, "pairs_compared": P, "cpu_model": cpu_model()}
    up_key = "[Pose estimation] convert + upload + launch (chunks)"
    if up_key in st and st[up_key] > 0:
        up_bytes = 16 * rows + 17 * P
        gbs = up_bytes / st[up_key] / 1e9
        comp["pcie"] = {"stage": up_key, "seconds": st[up_key], "bytes": up_bytes, "achieved_GBs": round(gbs, 1),
                        "link_peak_GBs_measured": round(pcie_peak, 1), "frac_of_link": round(gbs / pcie_peak, 3) if pcie_peak else None,
                        "note": "f32 SoA rows + per-pair arrays over the stage's wall clock (conversion and kernel launches share that clock)"}
    rep = sum(st.get(k, 0.0) for k in REPLICATED_STAGES) + m.get("seconds_rotation_averaging", 0.0)
    comp["replicated_host_s"] = round(rep, 4)
    comp["replicated_stages"] = {k: st[k] for k in REPLICATED_STAGES if k in st}
    comp["replicated_stages"]["rotation averaging (replicas only, SURVEY 8e)"] = m.get("seconds_rotation_averaging", 0.0)
    comp["amdahl_speedup_ceiling"] = amdahl(m["seconds"], rep)
    return comp


def compact_summary(out):
    """The claims a reader of the driver's truncated record must be able to check, as one flat object."""
    def dig(*keys):
        v = out
        for k in keys:
            if not isinstance(v, dict) or k not in v:
                return None
            v = v[k]
        return v
    def r(v, n=4):
        return round(v, n) if isinstance(v, float) else v
    s = {"k1_edges_per_s": out.get("value"), "k1_ms": dig("roofline", "kernel_ms"), "k1_frac_hbm": dig("roofline", "frac"),
         "k1_traffic_ratio": dig("roofline", "traffic_over_algorithmic"),
         "k2_frac_hbm": dig("score_pose_k2", "frac_hbm"), "k2_traffic_ratio": dig("score_pose_k2", "traffic_over_algorithmic"),
         "match_exact_frac_mfma": dig("match_descriptors", "roofline", "frac"),
         "match_exact_ms_min_med_max": [dig("match_descriptors", "min_ms"), dig("match_descriptors", "ms"), dig("match_descriptors", "max_ms")],
         "match_first_call_ms": dig("match_descriptors", "first_call_ms"),
         "match_sclk_mhz_median": dig("match_descriptors", "sclk_during_timed_calls", "median_mhz") if dig("match_descriptors", "sclk_during_timed_calls", "plausible") else None,
         "match_screened_ms": dig("match_descriptors", "screened", "ms"),
         "cpu_edges_per_s": dig("cpu_baseline", "value"), "cpu_cores": dig("cpu_baseline", "cores"), "cpu_parity": dig("cpu_baseline", "gpu_matches_on_sample")}
    f = out.get("config3_from_features") or {}
    c3 = [f.get(k, {}) for k in ("plain_every_pair_descriptor_matched", "astar_hashing_reference_guesses", "astar_hashing_rotation_guided")]
    s["config3_s"] = [c.get("features_to_graph_s") for c in c3]
    v5 = dig("graphs", "v5000") or {}
    c4 = v5.get("config4_shard_estimate_gather_average", {})
    c5 = v5.get("config5_astar_waves_rotation_guided", {})
    s.update(config4_s=c4.get("seconds"), config4_k1_ms=dig("graphs", "v5000", "config4_shard_estimate_gather_average", "roofline", "kernel_ms"),
             config4_cpu_pairs_per_s=dig("graphs", "v5000", "config4_shard_estimate_gather_average", "cpu_baseline", "value"),
             config4_cpu_parity=dig("graphs", "v5000", "config4_shard_estimate_gather_average", "cpu_baseline", "gpu_matches_on_sample"),
             config4_replicated_host_s=c4.get("replicated_host_s"), config4_amdahl_n8=(c4.get("amdahl_speedup_ceiling") or {}).get("n8"),
             config5_guided_s=c5.get("seconds"), config5_replicated_host_s=c5.get("replicated_host_s"),
             config5_amdahl_n8=(c5.get("amdahl_speedup_ceiling") or {}).get("n8"),
             config5_reference_guess_s=v5.get("config5_astar_waves_reference_guesses", {}).get("seconds"))
    worst = 0.0
    for reps in [c.get("all_repetitions_s") for c in c3] + [v.get("all_repetitions_s") for v in v5.values() if isinstance(v, dict)]:
        warm = (reps or [])[1:]
        if len(warm) >= 2:
            worst = max(worst, max(warm) / float(np.median(warm)))
    s["worst_over_median_repetition"] = round(worst, 3) if worst else None
    # progressive vs uniform sampling where the cap binds: [edges/s, mean hypotheses, AUC@5] each
    for key, name in (("rho0.3_uniform", "inlier_ratio_0.3_ratio_sorted_uniform"), ("rho0.3_progressive", "inlier_ratio_0.3_ratio_sorted_progressive"),
                      ("thr0.4_uniform", "thr_0.4px_ratio_sorted_uniform"), ("thr0.4_progressive", "thr_0.4px_ratio_sorted_progressive")):
        v = dig("variants", name)
        s["sampler_" + key] = [v.get("edges_per_s"), v.get("mean_hypotheses"), v.get("rot_err_auc_at_5deg")] if v else None
    # graph-cut local optimisation beside the default on the same batches: [edges/s, mean hypotheses, AUC@5]
    for key, name in (("rho0.5", "graph_cut_lo"), ("rho0.3", "inlier_ratio_0.3_graph_cut_lo"), ("rho0.3_default", "inlier_ratio_0.3")):
        v = dig("variants", name)
        s["gc_lo_" + key] = [v.get("edges_per_s"), v.get("mean_hypotheses"), v.get("rot_err_auc_at_5deg")] if v else None
    if out.get("n_gpus", 1) > 1:
        s["exchange_verified"] = out.get("exchange_verified")
        s["allgather_ms"] = dig("exchange", "allgather_ms")
        s["multi_rank_identical"] = [v.get("identical_to_single_process") for v in v5.values() if isinstance(v, dict) and "identical_to_single_process" in v] or None
    return {k: r(v) for k, v in s.items()}


COMPACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "quality", "exchange_verified")
COMPACT_LIMIT = 8192   # the driver keeps a bounded tail of stdout: a longer line is cut at the front and is no JSON any more


def _short(v, n=120):
    """strings cut to n characters, floats to 10 significant digits, containers walked"""
    if isinstance(v, str):
        return v if len(v) <= n else v[:n - 1] + "~"
    if isinstance(v, float):
        return float("%.10g" % v)
    if isinstance(v, dict):
        return {k: _short(x, n) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_short(x, n) for x in v]
    return v


def compact_line(out, full_path=None, summary=True):
    """The ONE line the driver parses: the contract's keys, `roofline`, `cpu_baseline`, `quality` and the flat
    `summary`, never more than COMPACT_LIMIT bytes; every per-leg block, repetition list and variant lives in bench_full.json.
    Notes are dropped before anything else; if a run ever still overflows, the optional blocks go one by one."""
    line = {k: out[k] for k in COMPACT_KEYS if k in out}
    if isinstance(line.get("roofline"), dict):
        line["roofline"] = {k: v for k, v in line["roofline"].items() if k not in ("note",)}
    if isinstance(line.get("cpu_baseline"), dict):
        cb = dict(line["cpu_baseline"])
        ocv = cb.pop("opencv", None)
        cb.pop("build", None)
        if isinstance(ocv, dict):
            cb["opencv_available"] = bool(ocv.get("available"))
        line["cpu_baseline"] = cb
    if isinstance(out.get("exchange"), dict):
        line["exchange"] = {k: v for k, v in out["exchange"].items() if k not in ("note", "uneven_counts")}
    if summary:   # (the flat digest of the --full legs: a plain run has none of them)
        line["summary"] = out.get("summary") or compact_summary(out)
    if full_path:
        line["full_record"] = full_path
    line = _short(line)
    for drop in (None, "full_record", "exchange", "quality"):
        if drop:
            line.pop(drop, None)
        txt = json.dumps(line, separators=(",", ":"))
        if len(txt.encode()) < COMPACT_LIMIT:
            return txt
    # last resort: the contract's scalar keys + roofline + cpu_baseline with every string cut hard
    line = _short({k: v for k, v in line.items() if k != "summary"}, 40)
    return json.dumps(line, separators=(",", ":"))


def emit(out, write_full=True):
    """full record -> bench_full.json beside this script (path on stderr); compact line -> stdout, LAST thing printed.
    A plain run (write_full=False) has no per-leg blocks to keep: it prints the line and writes nothing."""
    if not write_full:
        print(compact_line(out, summary=False), flush=True)
        return
    full_path = os.environ.get("PGI_BENCH_FULL", os.path.join(ROOT, "bench_full.json"))
    try:
        with open(full_path, "w") as f:
            json.dump(out, f)
        print("bench.py: full record (per-leg blocks, repetitions, variants) in %s" % full_path, file=sys.stderr)
    except OSError as ex:
        print("bench.py: could not write %s: %s" % (full_path, ex), file=sys.stderr)
        full_path = None
    sys.stderr.flush()
    print(compact_line(out, os.path.basename(full_path) if full_path else None), flush=True)


DUMP_LIMIT_BYTES = 64 << 20     # --dump-outputs: all files together
DUMP_MASK_SAMPLE = 4 << 20      # rows of the inlier mask kept when the whole mask (as f32) would not fit
DUMP_SAMPLE_SEED = 0xD0


def dump_outputs(dirname, edges_host, masks_host, offsets, gathered_host=None):
    """--dump-outputs: what the timed path returned in its last timed step, as DIR/<name>.npy in f32 / f64 -- every field of the
    edge records (pgi_edge: one row per pair), the inlier count per pair re-counted from the mask, and the mask itself (all rows
    when they fit, otherwise a fixed, seeded sample of row indices, which is stored beside it).  N > 1: rank 0's own block plus the
    essential matrices of every rank's records as gathered."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {}
    for name in edges_host.dtype.names:
        col = edges_host[name]
        arrays["edges_" + name] = np.ascontiguousarray(col, np.float64)   # (f64 holds every u32 / i32 field exactly)
    arrays["mask_inliers_per_pair"] = np.add.reduceat(masks_host.astype(np.int64), offsets[:-1]).astype(np.float64) \
        if len(masks_host) else np.zeros(0)
    if gathered_host is not None:
        arrays["gathered_edges_E"] = np.ascontiguousarray(gathered_host["E"], np.float64)
    room = DUMP_LIMIT_BYTES - sum(a.nbytes for a in arrays.values()) - 4096 * (len(arrays) + 2)
    if 4 * len(masks_host) <= room:
        arrays["masks"] = masks_host.astype(np.float32)
    else:
        k = min(DUMP_MASK_SAMPLE, room // 12, len(masks_host))
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(len(masks_host), size=k, replace=False))
        arrays["masks_sample_rows"] = idx.astype(np.float64)
        arrays["masks_sample"] = masks_host[idx].astype(np.float32)
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_LIMIT_BYTES
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    print("bench.py: %d output arrays (%.1f MB) of the last timed step in %s" % (len(arrays), sum(a.nbytes for a in arrays.values()) / 1e6, dirname),
          file=sys.stderr)


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except Exception:  # noqa: BLE001
        pass
    return "unknown"


def opencv_column(b, m, thr, cores):
    """the harness probes `import cv2`; only if that ever succeeds does it add the reference's own estimator call
    (cv::findEssentialMat(p1, p2, I, USAC_MAGSAC, 0.99, thr) + recoverPose, pose_graph_builder.h:1037-1044) on the same
    pairs, one thread and all threads.  On this image OpenCV is absent and the column says so."""
    try:
        import cv2
    except Exception as ex:  # noqa: BLE001
        return {"available": False, "reason": "import cv2 failed: %s" % type(ex).__name__}
    res = {"available": True, "version": cv2.__version__}
    try:
        for label, nthreads in (("one_thread", 1), ("all_threads", cores)):
            cv2.setNumThreads(nthreads)
            n = min(m, 200 if nthreads == 1 else 2000)
            t0 = time.perf_counter()
            for p in range(n):
                a, z = int(b["offsets"][p]), int(b["offsets"][p + 1])
                p1 = np.stack([b["x1"][a:z], b["y1"][a:z]], 1).astype(np.float64)
                p2 = np.stack([b["x2"][a:z], b["y2"][a:z]], 1).astype(np.float64)
                E, _ = cv2.findEssentialMat(p1, p2, np.eye(3), cv2.USAC_MAGSAC, 0.99, thr)
                if E is not None and E.shape == (3, 3):
                    cv2.recoverPose(E, p1, p2)
            res[label] = {"edges_per_s": round(n / (time.perf_counter() - t0), 1), "pairs": n, "threads": nthreads}
    except Exception as ex:  # noqa: BLE001
        res["error"] = repr(ex)
    return res


def graph_level(world, require_rccl=False, eng=None, torch=None):
    """BASELINE configs 3 / 4 / 5 on the scene graphs of tests/scene_drivers.py (v340: ~7 300 pairs / 5 M rows, v5000:
    ~106 000 pairs / 77 M rows -- SURVEY 8d's k ~ 40 nearest views, median ~ 600 rows per pair, cap 8000) through the C++
    driver as `world` freshly started child processes (one per GPU; never an exec after HIP initialisation).  With
    world > 1 the edge records travel through pgi_allgather_edges over RCCL (dist::attach), every rank's result file must
    equal the single-process run's byte for byte, and the line says so."""
    import hashlib
    import tempfile
    import scene_drivers as SC
    if not os.path.exists(SC.EXE):
        return {"skipped": "host driver %s not built" % SC.EXE}
    graphs = {}
    pcie_peak = pcie_h2d_peak_gbs(torch, eng.device) if (eng is not None and world == 1) else None
    labels = {"shard": "config4_shard_estimate_gather_average", "waves": "config5_astar_waves_reference_guesses",
              "waves_guided": "config5_astar_waves_rotation_guided"}
    with tempfile.TemporaryDirectory() as tmpd:
        for name, label in (("v340", "config 3 surrogate: 340 views, k = 40"), ("v5000", "configs 4/5 surrogate: 5000 views, k = 40")):
            if world > 1 and name != "v5000":
                continue
            t0 = time.time()
            g, wave = SC.make_scene(name)
            scene_path = os.path.join(tmpd, name + ".bin")
            SC.write_scene_bulk(scene_path, g, wave, sim_kind=2)
            entry = {"what": label, "views": len(g["R_gt"]), "candidate_pairs": len(g["pairs"]), "rows": int(g["batch"]["offsets"][-1]),
                     "rows_per_pair_median": int(np.median(g["sizes"])), "wave": wave, "generation_s": round(time.time() - t0, 1)}
            for mode in ("shard", "waves", "waves_guided"):
                single = os.path.join(tmpd, "%s_%s_w1" % (name, mode))
                # (four repetitions inside the driver; the MEDIAN of the three warm ones is reported: the host team shares the box)
                so = SC.run_ranks([SC.EXE, scene_path, single, mode], 1, extra_env={"PGI_DRIVER_REPS": "4", "PGI_QUIET": "1"})[0]
                blob = open(single + ".0", "rb").read()
                m = SC.graph_mode_metrics(g, blob, mode, *SC.seconds_of(so), SC.stages_of(so))
                m["all_repetitions_s"] = SC.all_seconds_of(so)
                m["all_repetitions_stage_s"] = SC.all_stages_of(so)
                if eng is not None and world == 1 and name == "v5000":
                    m.update(graph_companions(g, blob, m, mode, eng, torch, pcie_peak))
                if world > 1:
                    multi = os.path.join(tmpd, "%s_%s_w%d" % (name, mode, world))
                    env = {"PGI_DRIVER_REPS": "4", "PGI_QUIET": "1"}
                    if require_rccl:
                        env["PGI_COMM"] = "rccl"  # dist::attach: RCCL or an error on every rank, no fall-back to the host transport
                    outs = SC.run_ranks([SC.EXE, scene_path, multi, mode], world, extra_env=env)
                    mm = SC.graph_mode_metrics(g, open(multi + ".0", "rb").read(), mode, *SC.seconds_of(outs[0]), SC.stages_of(outs[0]))
                    mm["all_repetitions_s"] = SC.all_seconds_of(outs[0])
                    same = all(open(multi + ".%d" % r, "rb").read() == blob for r in range(world))
                    transports = sorted({o.split("transport ")[1].split()[0] for o in outs if "transport " in o})
                    m = dict(mm, world=world, transport=",".join(transports), identical_to_single_process=same,
                             result_sha256_16=hashlib.sha256(blob).hexdigest()[:16],
                             single_process={"seconds": m["seconds"], "seconds_graph": m["seconds_graph"], "stages_s": m["stages_s"]})
                entry[labels[mode]] = m
            graphs[name] = entry
    return graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=10000, help="pairs per GPU (config 2: 10000)")
    ap.add_argument("--corrs", type=int, default=2000, help="correspondences per pair (config 2: 2000)")
    ap.add_argument("--inlier-ratio", type=float, default=0.5)
    ap.add_argument("--thr-px", type=float, default=0.75)
    ap.add_argument("--fixed-budget", type=int, default=0, help="0 = adaptive (confidence 0.99, cap 1000)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: target CPU-baseline time (rank 0, N=1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline and its parity check")
    ap.add_argument("--no-extra", action="store_true", help="--full without the secondary fixed-256 / score_pose lines")
    ap.add_argument("--no-variants", action="store_true", help="--full without the SURVEY 8d variants (ragged, inlier ratios, 0.4 px) and the graph-level runs")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg (quality, replayed profiles, variants, graph-level configs, "
                         "secondary kernels, CPU baseline and parity) and write bench_full.json; a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (edge records field by field, inlier masks) as DIR/<name>.npy")
    ap.add_argument("--require-rccl", action="store_true",
                    help="N > 1: fail (non-zero exit) unless the exchange runs through pgi_allgather_edges over RCCL")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "RANK" not in os.environ:
        # launched plainly with --gpus N: start the one-process-per-GPU job as a CHILD (never exec after HIP init) and
        # pass its exit code on; the driver's own torch.distributed.run invocation takes the other branch
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", os.environ.get("MASTER_PORT", "29517"), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    n_gpus = world

    from pyposegraphbuilder import Engine, synthetic as S
    from pyposegraphbuilder import _lib as L

    P, N = args.pairs, args.corrs
    thr = args.thr_px / S.FOCAL_PX
    seed = 0xB0BA
    pair_base = rank * P
    t0 = time.time()
    b = S.make_batch(np.arange(pair_base, pair_base + P), N, inlier_ratio=args.inlier_ratio)
    gen_s = time.time() - t0

    eng = Engine(fixed_budget=args.fixed_budget)
    db = eng.upload(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], thr, seed=seed, pair_id_base=pair_base)
    edges = torch.empty((P, EDGE_RECORD_BYTES), dtype=torch.uint8, device=eng.device)
    masks = torch.empty(P * N, dtype=torch.uint8, device=eng.device)
    gathered = torch.empty((world * P, EDGE_RECORD_BYTES), dtype=torch.uint8, device=eng.device) if world > 1 else None
    # the path's one exchange step goes through the C ABI (pgi_allgather_edges: RCCL inside libpgi.so on the engine's
    # stream, bootstrapped here by shipping the 128-byte unique id through torch.distributed); if that cannot be set up
    # the bench falls back to torch.distributed's own all-gather and says so in the JSON line
    comm, exchange, comm_info = None, "none (single GPU)", None
    counts_uneven, gathered_uneven = None, None
    if world > 1:
        from pyposegraphbuilder import distributed as D
        try:
            comm = D.Communicator(eng, transport="rccl")
            exchange = "pgi_allgather_edges (RCCL inside libpgi.so): equal blocks ncclAllGather + an uneven table by grouped ncclSend/ncclRecv"
        except Exception as ex:  # noqa: BLE001
            if args.require_rccl:
                raise SystemExit("bench.py --require-rccl: the C-ABI RCCL communicator could not be set up: %s" % ex)
            comm, exchange = None, "torch.distributed all_gather_into_tensor (C-ABI communicator unavailable: %s)" % ex
        if comm is not None:
            cw, cr, ck = eng.comm_info()   # what libpgi.so itself reports: world, this rank, transport kind
            comm_info = {"rccl_ranks": int(cw) if ck == "rccl" else 0, "transport": ck, "rccl_version": comm.rccl_version}
            if args.require_rccl and (ck != "rccl" or cw != world):
                raise SystemExit("bench.py --require-rccl: libpgi.so reports transport %s with %d rank(s), expected rccl with %d" % (ck, cw, world))
            # the uneven-block path (config 4's row-balanced shards are ragged): rank r contributes the records of a
            # row-balanced block of a ragged pair list; exchanged by grouped ncclSend/ncclRecv, no padding
            rag = np.random.default_rng(5).integers(50, 4001, world * (P // 2))   # half a step's records: every block stays below P
            counts_uneven = [hi - lo for lo, hi in D.shard_bounds(rag, world)]
            assert max(counts_uneven) <= P and len(set(counts_uneven)) > 1 or world == 1
            gathered_uneven = torch.empty((sum(counts_uneven), EDGE_RECORD_BYTES), dtype=torch.uint8, device=eng.device)
    counts = [P] * world

    ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(4)) for _ in range(args.steps)]

    def step(i=None):
        if i is not None:
            ev[i][0].record()
        eng.estimate_pose_batch(db, edges, masks)
        if i is not None:
            ev[i][1].record()
        if world > 1:  # the path's one exchange: per-edge records to every rank (RCCL over xGMI)
            if comm is not None:
                comm.allgather_edges(edges, counts, out=gathered)
                if i is not None:
                    ev[i][2].record()
                comm.allgather_edges(edges[:counts_uneven[rank]], counts_uneven, out=gathered_uneven)
                if i is not None:
                    ev[i][3].record()
            else:
                dist.all_gather_into_tensor(gathered, edges)
                if i is not None:
                    ev[i][2].record()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=eng.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    kern_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))  # HIP events on the launch stream
    allgather_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev])) if world > 1 else None
    allgather_uneven_ms = float(np.mean([e[2].elapsed_time(e[3]) for e in ev])) if comm is not None else None

    # what the last timed step returned, on the host: only a run that uses it (--dump-outputs, --full) downloads it
    got, masks_host = None, None
    if args.full or (rank == 0 and args.dump_outputs):
        got = eng.edges_to_numpy(edges)
        masks_host = masks.cpu().numpy()  # the secondary runs below reuse the device buffers
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, got, masks_host, np.asarray(b["offsets"], np.int64),
                     eng.edges_to_numpy(gathered) if gathered is not None else None)

    value = world * P * args.steps / dt
    bytes_per_launch = P * algorithmic_bytes_per_edge(N)
    achieved_gbs = bytes_per_launch / (kern_ms * 1e-3) / 1e9
    traffic, pmc, roofline_compute, traffic_kernel_us = None, None, None, None
    tj, prof_name, prof_reason = (None, None, "fixed-budget run") if args.fixed_budget else \
        replay_profile("k1", P, N, L) if args.full else (None, None, "plain run (the profile is replayed with --full)")
    if tj:
        traffic = tj.get("hbm_bytes_per_launch")
        traffic_kernel_us = tj.get("kernel_us_trace_avg")
        pmc = {"wave_lifetime_split": tj.get("wave_lifetime_split"),
               "executed_flop_per_launch": tj.get("executed_flop_per_launch"),
               "source": "replayed from %s (rocprofv3 PMC passes of this workload, git %s)" % (prof_name, tj.get("git_head"))}
        roofline_compute = dict(tj.get("roofline_compute", {}), source="replayed from " + prof_name)
    out = {
        "metric": "pose-graph edges/sec (essential+decompose)",
        "value": round(value, 1), "unit": "edges/s", "n_gpus": n_gpus, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32 scoring / f64 solver", "data": "synthetic",
        "config": {"workload": "configs[1]: %d pairs x %d corrs batched essential RANSAC + decompose per GPU" % (P, N),
                   "pairs_per_gpu": P, "corrs_per_pair": N, "inlier_ratio": args.inlier_ratio,
                   "noise_px": 0.25, "thr_px": args.thr_px,
                   "mode": "fixed budget %d" % args.fixed_budget if args.fixed_budget else
                           "adaptive (confidence 0.99, cap 1000, rounds of 32)",
                   "parallelism": "pairs sharded over %d GPU(s)%s" % (world, ", all-gather of edge records" if world > 1 else ""),
                   "exchange": exchange},
        "roofline": {"bound": "hbm", "achieved": round(achieved_gbs, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved_gbs / HBM_PEAK_GBS, 6), "traffic": traffic,
                     "kernel": "estimate_pose_kernel", "kernel_ms": round(kern_ms, 3),
                     "bytes_per_edge": algorithmic_bytes_per_edge(N),
                     "traffic_kernel_us": traffic_kernel_us,   # the profiled kernel's average, next to this run's kernel_ms
                     "traffic_over_algorithmic": round(traffic / bytes_per_launch, 3) if traffic else None,
                     "traffic_source": ("replayed from %s; source hash matches the loaded build" % prof_name) if traffic
                                       else "none: %s" % prof_reason,
                     "note": "K1 stages rows once into LDS: VALU / LDS-latency bound by design (SURVEY 8d), see 'valu'"},
        "setup": {"gen_s": round(gen_s, 1)},
    }
    if args.full:
        ok = got["status"] == 1
        errs = np.array([S.rot_err_deg(got["R"][i].reshape(3, 3), b["R"][i]) if ok[i] else np.inf for i in range(P)])
        out["quality"] = {"rot_err_auc_at_5deg": round(S.auc_at(errs, 5.0), 4), "edges_ok": int(ok.sum()),
                          "median_rot_err_deg": round(float(np.median(errs)), 4), "mean_hypotheses": float(got["iters"].mean()),
                          "mean_lo_refits": float(got["lo_runs"].mean())}
    if world > 1:
        out["exchange"] = dict(comm_info or {"rccl_ranks": 0, "transport": "torch.distributed", "rccl_version": 0},
                               allgather_ms=round(allgather_ms, 4),
                               allgather_uneven_ms=round(allgather_uneven_ms, 4) if allgather_uneven_ms is not None else None,
                               records_per_rank=P, uneven_counts=counts_uneven,
                               note="per step, inside the timed region: one equal-block gather of the step's records and one "
                                    "uneven gather (row-balanced shards of a ragged list); HIP events on the engine's stream")
    # compute side (the kernel is VALU / LDS-latency bound, not HBM bound): measured by PMC, not estimated
    if pmc:
        out["valu"] = pmc
    if roofline_compute:
        out["roofline_compute"] = roofline_compute
    # SURVEY 8d's compute figure: F_edge = T * (F_solve + M * N * 30) with F_solve = 1e4 flop, M = 4 real solutions,
    # 30 flop per Sampson residual and T = the hypotheses actually drawn.  This is ALGORITHMIC work (every model
    # scored on every row); the kernel avoids most of it (pre-verification, exact bail-out), so the figure says how
    # fast the job's nominal arithmetic is retired, not how many flops execute.
    if args.full:
        T_mean = float(got["iters"].mean())
        f_edge = T_mean * (1.0e4 + 4 * N * 30)
        tfs = (P / (kern_ms * 1e-3)) * f_edge / 1e12
        out["valu_algorithmic"] = {"flop_per_edge": round(f_edge), "achieved": round(tfs, 2), "peak": 157.3, "unit": "TFLOP/s",
                                   "frac": round(tfs / 157.3, 4), "hypotheses_per_edge": round(T_mean, 1),
                                   "note": "SURVEY 8d formula; nominal work, not executed flops"}

    # (round 6: the variants and the graph-level legs run BEFORE the secondary kernels -- after the matcher leg, which draws the chip's
    #  full power for seconds, the driver children of configs 4 / 5 read 10-20 % slower: 0.099 / 0.112 s against 0.089 / 0.092 s)
    if args.full and rank == 0 and world == 1 and not args.no_variants and not args.fixed_budget:
        # ---- SURVEY 8d's other settings of config 2 (same kernel, same 10 000 pairs; never `value`) -------------------
        def run_variant(batch, thr_v, reps=3, **prm_v):
            if prm_v:
                eng.set_params(**prm_v)
            try:
                return run_variant_(batch, thr_v, reps)
            finally:
                if prm_v:
                    eng.set_params(**{k: 0 for k in prm_v})   # (only switches that default to 0 are varied here: sampler)

        def run_variant_(batch, thr_v, reps):
            dbv = eng.upload(batch["x1"], batch["y1"], batch["x2"], batch["y2"], batch["offsets"], thr_v, seed=seed, pair_id_base=pair_base)
            ev_, mv_ = eng.estimate_pose_batch(dbv)
            torch.cuda.synchronize()
            a_, z_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record()
            for _ in range(reps):
                ev_, mv_ = eng.estimate_pose_batch(dbv)
            z_.record()
            torch.cuda.synchronize()
            ms_ = a_.elapsed_time(z_) / reps
            gv = eng.edges_to_numpy(ev_)
            okv = gv["status"] == 1
            Pv = len(gv)
            ev_deg = np.array([S.rot_err_deg(gv["R"][i].reshape(3, 3), batch["R"][i]) if okv[i] else np.inf for i in range(Pv)])
            rows_v = int(batch["offsets"][-1])
            return {"edges_per_s": round(Pv / (ms_ * 1e-3), 1), "kernel_ms": round(ms_, 3), "rows": rows_v,
                    "rows_per_s": round(rows_v / (ms_ * 1e-3), 1), "rot_err_auc_at_5deg": round(S.auc_at(ev_deg, 5.0), 4),
                    "edges_ok": int(okv.sum()), "mean_hypotheses": round(float(gv["iters"].mean()), 1)}
        variants = {}
        t0 = time.time()
        variants["thr_0.4px"] = dict(run_variant(b, 0.4 / S.FOCAL_PX), note="the reference's default threshold (examples/cpp_example.cpp:51)")
        ids_v = np.arange(pair_base, pair_base + P)
        sizes_v = S.ragged_sizes(ids_v)
        variants["ragged_N_U50_4000"] = dict(run_variant(S.make_batch(ids_v, sizes_v), thr),
                                             note="N ~ U{50..4000} per pair: bucketed on the device into occupancy classes, one launch per class")
        for rho_v in (0.3, 0.7):
            variants["inlier_ratio_%.1f" % rho_v] = run_variant(S.make_batch(ids_v, N, inlier_ratio=rho_v), thr)
        # Progressive sampling (pgi_params.sampler = 1) where the iteration cap binds, on rows in the reference's order
        # (ascending SNN ratio, feature_utils.h:184-186; S.ratio_sorted): VERDICT r5 item 9.  Uniform sampling on the
        # same sorted rows beside it (the order alone changes nothing for a uniform sampler).
        b_lo = S.ratio_sorted(S.make_batch(ids_v, N, inlier_ratio=0.3))
        b_srt = S.ratio_sorted(b)
        variants["inlier_ratio_0.3_ratio_sorted_uniform"] = run_variant(b_lo, thr)
        variants["inlier_ratio_0.3_ratio_sorted_progressive"] = dict(run_variant(b_lo, thr, sampler=1), note="sampler = 1")
        variants["thr_0.4px_ratio_sorted_uniform"] = run_variant(b_srt, 0.4 / S.FOCAL_PX)
        variants["thr_0.4px_ratio_sorted_progressive"] = dict(run_variant(b_srt, 0.4 / S.FOCAL_PX, sampler=1), note="sampler = 1")
        del b_lo, b_srt
        # Graph-cut local optimisation (pgi_params.lo_graph_cut = 9: lambda 0.14, the "GC" of GC-RANSAC; off by default): the refit's
        # rows are the minimum cut of the spatial-coherence energy.  Same kernel, same batches as `value` / inlier_ratio_0.3.
        variants["graph_cut_lo"] = dict(run_variant(b, thr, lo_graph_cut=9), note="config 2's batch with lo_graph_cut = 9")
        variants["inlier_ratio_0.3_graph_cut_lo"] = dict(run_variant(S.make_batch(ids_v, N, inlier_ratio=0.3), thr, lo_graph_cut=9), note="lo_graph_cut = 9")
        variants["seconds_incl_generation"] = round(time.time() - t0, 1)
        out["variants"] = variants
        # ---- graph level (BASELINE configs 3 / 4 / 5 on their surrogates AT SURVEY 8d's DENSITY; 1DSfM data is on neither box):
        # the C++ host layer (tests/cpp/test_distributed.cpp: PoseGraphBuilder::estimateAndAverage / run + averageRotations)
        # as a child process, its own wall clock and stage clocks, warm repetition; global rotation error after gauge
        # alignment, AUC@5 of the estimated edges
        out["graphs"] = graph_level(1, eng=eng, torch=torch)
        import scene_drivers as SC
        # ---- config 3 FROM FEATURES at its stated size (340 views x ~8000 keypoints x 128-d descriptors = 1.4 GB; the 20 next
        # views of every view as candidates): PoseGraphBuilder::processFeatures -- descriptor matching / tracklet quick matching
        # -> createCorrespondenceMatrix -> A* guesses -> estimatePose -> guided matching -> tracklets in HBM -- as a child
        # process (tests/cpp/test_pipeline.cpp), warm repetition, its own wall clock and stage split
        if os.path.exists(SC.PIPELINE_EXE):
            t0 = time.time()
            fviews, fposes, fcam, fsim, fpairs = S.make_feature_scene(340, 8000, band=20)
            gen_f = time.time() - t0
            with tempfile.TemporaryDirectory() as tmpd:
                fin, fout = os.path.join(tmpd, "features.bin"), os.path.join(tmpd, "features.out")
                SC.write_feature_scene(fin, fviews, fcam, fsim, fpairs, 512)
                kp_mean = float(np.mean([len(v["xy"]) for v in fviews]))
                del fviews
                import subprocess
                r = subprocess.run([SC.PIPELINE_EXE, fin, fout, "024"], capture_output=True, text=True, timeout=1200,
                                   env=dict(os.environ, PGI_DRIVER_REPS="4"))
                slow = [ln for ln in r.stderr.splitlines() if "[processFeatures] upload of" in ln]
                feat = {"views": 340, "keypoints_per_view": round(kp_mean), "candidate_pairs": len(fpairs), "wave": 512,
                        "descriptor_bytes": int(340 * kp_mean * 512), "generation_s": round(gen_f, 1)}
                if r.returncode == 0:
                    tim = SC.pipeline_timings(r.stdout)
                    res = SC.parse_pipeline(open(fout, "rb").read(), 3)
                    for (mode, label), (stf, ef) in zip(((0, "plain_every_pair_descriptor_matched"), (2, "astar_hashing_reference_guesses"),
                                                         (4, "astar_hashing_rotation_guided")), res):
                        kf = dict(zip(SC.PIPELINE_KEYS, stf))
                        errf = np.array([S.rot_err_deg(ef[key][1], fposes[key[1]][0] @ fposes[key[0]][0].T) for key in ef])
                        feat[label] = {"features_to_graph_s": tim[mode]["seconds"], "all_repetitions_s": tim[mode]["all_seconds"],
                                       "repetition_reported": tim[mode]["repetition"],  # the median of the warm repetitions
                                       "all_repetitions_stage_s": tim[mode]["all_stages"],
                                       "stages_s": tim[mode]["stages"],
                                       "pairs_per_s": round(len(fpairs) / tim[mode]["seconds"], 1), "edges": len(ef),
                                       "descriptor_matching_runs": kf["matching_runs"], "tracklet_quick_matching_runs": kf["quick_matching_runs"],
                                       "guided_matching_runs": kf["guided_matching_runs"], "tracks": kf["track_number"],
                                       "poses_from_guess": kf["poses_from_guess"], "quirk_only_guesses": kf["quirk_only_guesses"],
                                       "edge_rot_err_auc_at_5deg": round(S.auc_at(np.concatenate([errf, np.full(len(fpairs) - len(ef), np.inf)]), 5.0), 4),
                                       "edge_rot_err_median_deg": round(float(np.median(errf)), 4)}
                    gj, gname, gwhy = replay_profile("guided", None, None, L)
                    feat["dominant_kernel"] = dict(
                        {"kernel": (gj or {}).get("kernel", "guided_scan_flat_kernel").split(" (")[0], "bound": "latency (seven wavefronts per CU in the sum kernel; VALU 39 % busy); frac_hbm = ALGORITHMIC bytes / time of all kernels of the scan / 8 TB/s, traffic_* = the counters' bytes over the same time"},
                        **({k: gj.get(k) for k in ("kernel_us_trace_avg", "scan_us_all_kernels", "companion_kernels", "dispatches", "share_of_gpu_time", "algorithmic_bytes_per_launch", "hbm_bytes_per_launch",
                                                    "traffic_over_algorithmic", "achieved_GBs", "frac_hbm", "traffic_GBs", "traffic_frac_hbm", "valu_issue_busy_frac", "wave_waiting_frac", "lane_utilisation", "vgprs", "spilled_vgprs")}
                           if gj else {}),
                        source=("replayed from %s; source hash matches the loaded build" % gname) if gj else "none: %s" % gwhy)
                    if slow:  # the upload stage reports itself when it is far slower than PCIe allows (a shared box now and then)
                        feat["slow_uploads"] = slow[:6]
                else:
                    feat["error"] = r.stderr[-500:]
            out["config3_from_features"] = feat

    if args.full and rank == 0 and world == 1 and not args.no_extra:
        # secondary lines (not `value`): fixed budget of 256 hypotheses; the HBM-bound K2 score kernel
        eng.set_params(fixed_budget=256)
        eng.estimate_pose_batch(db, edges, masks)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.estimate_pose_batch(db, edges, masks)
        z.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(z)
        out["fixed_budget_256"] = {"edges_per_s": round(P / (ms * 1e-3), 1), "kernel_ms": round(ms, 3)}
        eng.set_params(fixed_budget=args.fixed_budget)
        # Two batches in flight (never `value`): a launch of 10 000 pairs ends with a drain -- the last workgroups, a few of
        # them on pairs that need 300-1000 hypotheses, keep the kernel alive while most CUs are already idle
        # (scripts/k1_tail_probe.py: T(P) = 0.89 ms + P / 1.79 M edges/s, i.e. 14 % of this launch).  Independent batches on
        # two contexts / streams fill each other's drain; this is what a caller with more than one batch at hand gets.
        eng2 = Engine(fixed_budget=args.fixed_budget)
        s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
        edges_b, masks_b = torch.empty_like(edges), torch.empty_like(masks)
        with torch.cuda.stream(s_b):
            db_b = eng2.upload(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], thr, seed=seed, pair_id_base=pair_base)
        torch.cuda.synchronize()

        def two_in_flight(k):
            for i in range(k):
                if i % 2 == 0:
                    with torch.cuda.stream(s_a):
                        eng.estimate_pose_batch(db, edges, masks)
                else:
                    with torch.cuda.stream(s_b):
                        eng2.estimate_pose_batch(db_b, edges_b, masks_b)
        two_in_flight(4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        two_in_flight(args.steps)
        torch.cuda.synchronize()
        t_pipe2 = time.perf_counter() - t0
        same_b = bool(torch.equal(edges_b, edges) and torch.equal(masks_b, masks))
        eng2.close()
        eng._bind_stream()
        out["two_batches_in_flight"] = {"edges_per_s": round(P * args.steps / t_pipe2, 1), "ms_per_batch": round(1e3 * t_pipe2 / args.steps, 3),
                                        "identical_results": same_b,
                                        "note": "the same %d steps alternating between two contexts on two streams; not `value` (one batch at a time)" % args.steps}
        # PCIe-inclusive rate (never `value`), headline variant first: page-locked caller buffers (hipHostMalloc, here through
        # torch's pinned allocator) -- K1 works on them in place over PCIe: it reads every row once and writes every result once
        px = [torch.from_numpy(np.ascontiguousarray(b[k], np.float32)).pin_memory().numpy() for k in ("x1", "y1", "x2", "y2")]
        pe = torch.zeros(P * EDGE_RECORD_BYTES, dtype=torch.uint8).pin_memory().numpy().view(L.EDGE_DTYPE)
        pm = torch.zeros(P * N, dtype=torch.uint8).pin_memory().numpy()
        for _ in range(4):
            eng.estimate_pose_batch_host(*px, b["offsets"], thr, seed=seed, pair_id_base=pair_base, out=(pe, pm))
        t_pin = []
        for _ in range(5):
            t0 = time.perf_counter()
            eng.estimate_pose_batch_host(*px, b["offsets"], thr, seed=seed, pair_id_base=pair_base, out=(pe, pm))
            t_pin.append(time.perf_counter() - t0)
        t_pin = float(np.median(t_pin))
        # PCIe-inclusive rate: host SoA in, edge records + masks back to the host (never `value`).  (i) the naive
        # sequence upload -> kernel -> download; (ii) pgi_estimate_pose_batch_host: chunks on two streams, copies
        # overlapping kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db2 = eng.upload(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], thr, seed=seed, pair_id_base=pair_base)
        e2, m2 = eng.estimate_pose_batch(db2, edges, masks)
        _ = e2.cpu(), m2.cpu()
        torch.cuda.synchronize()
        t_inc = time.perf_counter() - t0
        del db2
        # (host-pointer runs need a few calls before slots, staging and page mappings are warm: 3 untimed, median of 5)
        for _ in range(3):
            eng.estimate_pose_batch_host(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], thr, seed=seed, pair_id_base=pair_base)
        t_pipe = []
        for _ in range(5):
            t0 = time.perf_counter()
            he, hm = eng.estimate_pose_batch_host(b["x1"], b["y1"], b["x2"], b["y2"], b["offsets"], thr, seed=seed, pair_id_base=pair_base)
            t_pipe.append(time.perf_counter() - t0)
        t_pipe = float(np.median(t_pipe))
        pinned_same = bool(np.array_equal(pm, masks_host) and np.array_equal(pe["E"], got["E"]))
        out["h2d_inclusive"] = {"edges_per_s": round(P / t_pin, 1), "ms": round(1e3 * t_pin, 2),
                                "pageable_edges_per_s": round(P / t_pipe, 1), "pageable_ms": round(1e3 * t_pipe, 2),
                                "sequential_edges_per_s": round(P / t_inc, 1), "sequential_ms": round(1e3 * t_inc, 2),
                                "identical_to_resident_run": bool(np.array_equal(hm, masks_host) and np.array_equal(he["E"], got["E"])
                                                                  and pinned_same),
                                "note": "host SoA in, edges+masks back in host memory; headline = page-locked caller buffers "
                                        "(hipHostMalloc), which K1 reads and writes in place over PCIe; pageable_* = plain numpy "
                                        "arrays, copied through HBM in chunks over four device slots"}
        Egt = np.stack([np.cross(np.eye(3), b["t"][i]) @ b["R"][i] for i in range(P)]).reshape(P, 9)
        dE = torch.from_numpy(Egt).to(eng.device)
        dt2 = torch.full((P,), thr * thr, dtype=torch.float64, device=eng.device)
        cnt = torch.empty(P, dtype=torch.int32, device=eng.device)
        import ctypes as C
        st = eng._batch_struct(db)
        def k2():
            L.check(eng._lib.pgi_score_pose_batch(eng._ctx, C.byref(st), C.c_void_p(dE.data_ptr()), C.c_void_p(dt2.data_ptr()),
                                                  C.c_void_p(cnt.data_ptr()), C.c_void_p(masks.data_ptr())))
        eng._bind_stream()
        for _ in range(3):
            k2()
        torch.cuda.synchronize()
        a.record()
        for _ in range(10):
            k2()
        z.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(z) / 10
        k2_bytes = P * (17 * N + 76 + 8)
        out["score_pose_k2"] = {"kernel_ms": round(ms, 4), "achieved_GBs": round(k2_bytes / (ms * 1e-3) / 1e9, 1),
                                "frac_hbm": round(k2_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "pair_scores_per_s": round(P / (ms * 1e-3), 1)}
        k2j, k2name, k2why = replay_profile("k2", P, N, L)
        out["score_pose_k2"].update(
            {"traffic": k2j["hbm_bytes_per_launch"], "traffic_kernel_us": k2j["kernel_us_trace_avg"],
             "traffic_over_algorithmic": round(k2j["hbm_bytes_per_launch"] / k2_bytes, 3),
             "traffic_source": "replayed from %s; source hash matches the loaded build" % k2name} if k2j
            else {"traffic": None, "traffic_source": "none: %s" % k2why})
        # descriptor matching, the step that feeds the path: 8 images x 8000 keypoints, all 56 ordered
        # pairs.  (i) the all-f32 kernel against the f32-input MFMA peak (useful flop = 2*K*K*128 per pair);
        # (ii) the default screened path (f16 matrix-core screen + exact f32 verification, identical output)
        K, n_img = 8000, 8
        g = torch.Generator(device="cpu").manual_seed(1234)
        descs = []
        for _ in range(n_img):
            d = torch.randn((K, 128), generator=g).abs_()
            descs.append((d / d.norm(dim=1, keepdim=True)).numpy())
        sel = [(i, j) for i in range(n_img) for j in range(n_img) if i != j]

        def time_match(screen):
            """3 warm-ups (the first one timed separately: workspace growth, code-object load), then 10 calls timed one by one
            with HIP events on the launch stream; the line carries min / median / max and the GPU's clock and power around it"""
            imgs = [eng.prepare_descriptors(d, screen=screen) for d in descs]
            torch.cuda.synchronize()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(13)]
            res = None
            for k, (e0, e1) in enumerate(evs[:3]):
                e0.record()
                res = eng.match_descriptors_batch(imgs, sel, raw=True)
                e1.record()
                torch.cuda.synchronize()
            with ClockSampler() as clk:   # the clock the box grants WHILE the ten timed calls run
                for e0, e1 in evs[3:]:
                    e0.record()
                    res = eng.match_descriptors_batch(imgs, sel, raw=True)
                    e1.record()
                torch.cuda.synchronize()
            t = [e0.elapsed_time(e1) for e0, e1 in evs]
            timed = np.array(t[3:])
            return {"ms": float(np.median(timed)), "min_ms": float(timed.min()), "max_ms": float(timed.max()), "first_call_ms": float(t[0]),
                    "calls": len(timed), "sclk": clk.result()}, [x.cpu() for x in res]
        tm, ref = time_match(False)
        tm_s, got_s = time_match(True)
        ms, ms_s = tm["ms"], tm_s["ms"]
        same = all(bool(torch.equal(x, y)) for x, y in zip(ref[3:], got_s[3:])) and all(
            bool(torch.equal(x[p, :ref[3][p]], y[p, :ref[3][p]])) for x, y in zip(ref[:3], got_s[:3]) for p in range(len(sel)))
        tf = 2.0 * K * K * 128 * len(sel) / (ms * 1e-3) / 1e12
        tf_best = 2.0 * K * K * 128 * len(sel) / (tm["min_ms"] * 1e-3) / 1e12
        out["match_descriptors"] = {"pairs": len(sel), "keypoints": K, "ms": round(ms, 3), "min_ms": round(tm["min_ms"], 3),
                                    "max_ms": round(tm["max_ms"], 3), "first_call_ms": round(tm["first_call_ms"], 3), "timed_calls": tm["calls"],
                                    "pairs_per_s": round(len(sel) / (ms * 1e-3), 1),
                                    "sclk_during_timed_calls": tm["sclk"],
                                    "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": 157.3, "unit": "TFLOP/s",
                                                 "frac": round(tf / 157.3, 4), "frac_best_call": round(tf_best / 157.3, 4),
                                                 "dtype": "f32 (v_mfma_f32_32x32x2_f32)",
                                                 "note": "median of the timed calls; the kernel draws the chip's full power, so the rate follows the clock the box grants (sclk_during_timed_calls)"},
                                    "screened": {"ms": round(ms_s, 3), "min_ms": round(tm_s["min_ms"], 3), "max_ms": round(tm_s["max_ms"], 3),
                                                 "first_call_ms": round(tm_s["first_call_ms"], 3),
                                                 "pairs_per_s": round(len(sel) / (ms_s * 1e-3), 1),
                                                 "speedup": round(ms / ms_s, 2), "identical_output": same,
                                                 "note": "f16 MFMA screen + exact f32 verification (default path)"}}

        # rotation averaging (north_star's second stage; BASELINE config 4's graph size): 5000 views, ~21 edges per view,
        # 1 deg noise, 15 % outlier edges, L1 + IRLS to convergence
        from scipy.spatial.transform import Rotation
        rg = np.random.default_rng(2)
        V_ra = 5000
        Rgt = Rotation.random(V_ra, random_state=2).as_matrix()
        es = set()
        for i in range(V_ra):
            es.add((i, i + 1) if i + 1 < V_ra else (0, i))
            for j in rg.choice(V_ra, 20, replace=False):
                if j != i:
                    es.add((min(i, int(j)), max(i, int(j))))
        es = np.array(sorted(es))
        s_ra, d_ra = es[:, 0], es[:, 1]
        Rrel = np.einsum("eij,ekj->eik", Rgt[d_ra], Rgt[s_ra])
        Rrel = np.einsum("eij,ejk->eik", Rotation.from_rotvec(rg.standard_normal((len(es), 3)) * np.deg2rad(1.0) / np.sqrt(3)).as_matrix(), Rrel)
        bad = rg.random(len(es)) < 0.15
        Rrel[bad] = Rotation.random(int(bad.sum()), random_state=3).as_matrix()
        w_ra = np.where(bad, rg.uniform(0.1, 0.4, len(es)), rg.uniform(0.4, 1.0, len(es)))
        eng.rotation_average(s_ra, d_ra, Rrel, w_ra, V_ra)
        t0 = time.perf_counter()
        R_ra, it_ra = eng.rotation_average(s_ra, d_ra, Rrel, w_ra, V_ra)
        t_ra = time.perf_counter() - t0
        Gfix = Rgt[0].T @ R_ra[0]
        dR = np.einsum("kij,jl,kml->kim", Rgt, Gfix, R_ra)
        err_ra = np.degrees(np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1) / 2, -1, 1)))
        out["rotation_averaging"] = {"views": V_ra, "edges": int(len(es)), "ms": round(1e3 * t_ra, 2), "outer_iterations": int(it_ra),
                                     "mean_err_deg": round(float(err_ra.mean()), 4),
                                     "note": "host edge list in, rotations out (uploads, spanning-forest init and downloads included)"}
        # the same on a sparse, sequence-like view graph (5000 views, every view sees the next three): Jacobi-preconditioned
        # CG does not converge there; the solver switches to the spanning-tree-preconditioned kernel (prefix-sum tree solves)
        ss, sd = [], []
        for i in range(V_ra):
            for st_ in (1, 2, 3):
                if i + st_ < V_ra:
                    ss.append(i); sd.append(i + st_)
        ss, sd = np.array(ss), np.array(sd)
        Rs = np.einsum("eij,ekj->eik", Rgt[sd], Rgt[ss])
        Rs = np.einsum("eij,ejk->eik", Rotation.from_rotvec(rg.standard_normal((len(ss), 3)) * np.deg2rad(1.0) / np.sqrt(3)).as_matrix(), Rs)
        bad_s = rg.random(len(ss)) < 0.05
        Rs[bad_s] = Rotation.random(int(bad_s.sum()), random_state=4).as_matrix()
        ws = np.where(bad_s, rg.uniform(0.1, 0.4, len(ss)), rg.uniform(0.4, 1.0, len(ss)))
        eng.rotation_average(ss, sd, Rs, ws, V_ra)
        t0 = time.perf_counter()
        R_s, it_s = eng.rotation_average(ss, sd, Rs, ws, V_ra)
        t_s = time.perf_counter() - t0
        Gs = Rgt[0].T @ R_s[0]
        dRs = np.einsum("kij,jl,kml->kim", Rgt, Gs, R_s)
        err_s = np.degrees(np.arccos(np.clip((np.trace(dRs, axis1=1, axis2=2) - 1) / 2, -1, 1)))
        out["rotation_averaging_sequence_graph"] = {"views": V_ra, "edges": int(len(ss)), "ms": round(1e3 * t_s, 2), "outer_iterations": int(it_s),
                                                    "mean_err_deg": round(float(err_s.mean()), 4),
                                                    "note": "banded graph: errors accumulate along the sequence (mean_err is large by construction); "
                                                            "tree-preconditioned on-chip PCG"}
        # multi-view tracklets in HBM: one committed wave of 120 pairs over 16 views x 8000 keypoints
        from pyposegraphbuilder.engine import DeviceTracklets
        rt = np.random.default_rng(3)
        Vt, Kt = 16, 8000
        perm = [rt.permutation(Kt) for _ in range(Vt)]
        prs = [(a_, b_) for a_ in range(Vt) for b_ in range(a_ + 1, Vt)]
        calls, n_match = [], 0
        for pi in rt.permutation(len(prs))[:120]:
            a_, b_ = prs[pi]
            vis = np.nonzero(rt.random(Kt) < 0.6)[0]
            dd = perm[b_][vis].copy()
            wrong = rt.random(len(vis)) < 0.05
            dd[wrong] = rt.integers(0, Kt, int(wrong.sum()))
            mk = (rt.random(len(vis)) < 0.9).astype(np.uint8)
            calls.append((a_, b_, (torch.as_tensor(perm[a_][vis].astype(np.int32)).to(eng.device), torch.as_tensor(dd.astype(np.int32)).to(eng.device)),
                          torch.as_tensor(mk).to(eng.device)))
            n_match += int(mk.sum())
        trk_times = []
        for rep in range(4):  # first pass warms buffers and code objects
            trk = DeviceTracklets(eng, Vt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trk.add_batch(calls)
            torch.cuda.synchronize()
            t_trk = time.perf_counter() - t0
            trk_times.append(t_trk)
            info_t = trk.info()
            t0 = time.perf_counter()
            qres = trk.get_correspondences_batch([(c_[0], c_[1]) for c_ in calls], 5000, raw=True)
            torch.cuda.synchronize()
            t_q = time.perf_counter() - t0
            trk.close()
        print("tracklets add (s):", ["%.4f" % v for v in trk_times], file=sys.stderr)
        t_trk = float(np.median(trk_times[1:]))
        out["tracklets"] = {"pairs": len(calls), "inlier_matches": n_match, "add_ms": round(1e3 * t_trk, 2),
                            "ns_per_match": round(1e9 * t_trk / n_match, 1), "tracks": info_t["tracks"], "events": info_t["events"],
                            "round_launches": info_t["rounds"], "query_ms": round(1e3 * t_q, 2),
                            "correspondences_returned": int(qres[2].sum().item())}

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        # CPU baseline: the build's own CPU restatement (oracle/), NOT OpenCV (absent on this image),
        # same inputs / seeds / mode, all host cores, bounded sample; also re-checks parity on that sample
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as O
        prm = O.default_params(fixed_budget=args.fixed_budget)
        cores = O.lib().pgo_num_threads()

        def run(m):
            o = b["offsets"][:m + 1]
            r = int(o[-1])
            t0 = time.perf_counter()
            e, mk = O.estimate_pose_batch(b["x1"][:r], b["y1"][:r], b["x2"][:r], b["y2"][:r], o, thr, prm, seed,
                                          pair_id_base=pair_base, threads=cores)
            return time.perf_counter() - t0, e, mk
        m0 = min(P, 4 * cores)
        t_probe, _, _ = run(m0)
        m = int(min(P, max(m0, args.cpu_seconds / max(t_probe / m0, 1e-6))))
        t_cpu, e_cpu, mk_cpu = run(m)
        rows = int(b["offsets"][m])
        parity = bool(np.array_equal(masks_host[:rows], mk_cpu) and
                      np.array_equal(got["E"][:m], e_cpu["E"]) and np.array_equal(got["n_inl"][:m], e_cpu["n_inl"]))
        out["cpu_baseline"] = {"value": round(m / t_cpu, 1), "unit": "edges/s", "cores": int(cores), "kind": "port",
                               "sample": "first %d pairs of the same batch (%.1f s); build CPU restatement, not OpenCV" % (m, t_cpu),
                               "gpu_matches_on_sample": parity, "cpu_model": cpu_model(), "host_logical_cpus": os.cpu_count(),
                               "build": "oracle/pgi_oracle.c: gcc -O3 -mavx2 -mfma -ffp-contract=off, OpenMP over pairs (schedule dynamic)",
                               "opencv": opencv_column(b, m, thr, int(cores))}
    if world > 1 and (args.full or args.require_rccl):
        # every rank must hold EVERY rank's records after the exchange (checked outside the timed region): the owners
        # publish byte checksums of their blocks through torch.distributed, every rank checks all blocks of its copies
        def checksum(t):
            return int(t.to(torch.int64).sum().item()) if t.numel() else 0
        mine_sums = torch.tensor([checksum(edges), checksum(edges[:counts_uneven[rank]]) if comm is not None else 0],
                                 dtype=torch.int64, device=eng.device)
        all_sums = [torch.zeros_like(mine_sums) for _ in range(world)]
        dist.all_gather(all_sums, mine_sums)
        okx = bool(torch.equal(gathered[rank * P:(rank + 1) * P], edges))
        o_u = 0
        for r in range(world):
            okx = okx and checksum(gathered[r * P:(r + 1) * P]) == int(all_sums[r][0].item())
            if comm is not None:
                okx = okx and checksum(gathered_uneven[o_u:o_u + counts_uneven[r]]) == int(all_sums[r][1].item())
                o_u += counts_uneven[r]
        flag = torch.tensor([1 if okx else 0], dtype=torch.int32, device=eng.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        out["exchange_verified"] = bool(flag.item())
        if args.require_rccl and not out["exchange_verified"]:
            if rank == 0:
                emit(out)
            raise SystemExit("bench.py --require-rccl: a rank holds records that differ from their owner's")
    if world > 1 and args.full and not args.no_variants:
        # BASELINE configs 4 and 5 on `world` GPUs: rank 0 starts the C++ driver as world child processes (the bench's own
        # ranks idle at the barrier meanwhile: their GPUs are free) and compares every rank's result with the world-1 run
        if rank == 0:
            try:
                out["graphs"] = graph_level(world, require_rccl=args.require_rccl)
            except Exception as ex:  # noqa: BLE001
                out["graphs"] = {"error": repr(ex)[-800:]}
                if args.require_rccl:
                    emit(out)
                    raise
        dist.barrier()
    if rank == 0:
        if args.full:
            out["summary"] = compact_summary(out)
        emit(out, write_full=args.full)   # compact line (< 8 KB) LAST on stdout; with --full everything else in bench_full.json
    if comm is not None:
        comm.close()
    eng.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
