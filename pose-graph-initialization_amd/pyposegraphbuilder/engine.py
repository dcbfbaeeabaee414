"""Engine: the batched entry points of include/pgi.h over torch device tensors.

torch is used for HBM allocation and the stream only; all compute is in libpgi.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Triangulation:
    """Result of Engine.triangulate_tracks / DeviceTracklets.triangulate: device tensors X [T,3] f64 (NaN unless the
    status is TRI_OK or TRI_LOW_PARALLAX), status [T] u8 (pyposegraphbuilder.TRI_*), err_rms [T] f64, n_used [T] i32,
    obs_state [members] u8 (0 not counted, 1 used, 2 dropped as an outlier; the optional three are None when not asked
    for) and counts, a numpy array with the number of tracks per status."""

    def __init__(self, X, status, err_rms, n_used, obs_state, counts):
        self.X, self.status, self.err_rms, self.n_used, self.obs_state, self.counts = X, status, err_rms, n_used, obs_state, counts

    def numpy(self):
        """-> dict of numpy arrays (n_used as uint32)."""
        f = lambda t: None if t is None else t.cpu().numpy()
        n = f(self.n_used)
        return dict(X=f(self.X), status=f(self.status), err_rms=f(self.err_rms), n_used=None if n is None else n.astype(np.uint32),
                    obs_state=f(self.obs_state), counts=self.counts.copy())


class BundleResult:
    """Result of Engine.bundle_adjust / DeviceTracklets.bundle_adjust: R [V,3,3] and c [V,3] (numpy, refined where the view
    was free), X [T,3] f64 (device tensor, refined where the track took part) and the fields of pgi_bundle_report: iters,
    accepted, cg_iters_total, stop_reason (pyposegraphbuilder.BA_STOP_*), n_obs, n_points, n_free_cams, cost_initial,
    cost_final, lambda_final.  With refine_focal: focal [V] (the focal scales phi, refined where the view was focal-free)
    and n_free_focals; both None otherwise."""
    FIELDS = ("iters", "accepted", "cg_iters_total", "stop_reason", "n_obs", "n_points", "n_free_cams", "cost_initial",
              "cost_final", "lambda_final")

    def __init__(self, R, c, X, report, focal=None, n_free_focals=None):
        self.R, self.c, self.X = R, c, X
        self.focal, self.n_free_focals = focal, n_free_focals
        for k in self.FIELDS:
            setattr(self, k, getattr(report, k))

    def report(self):
        return {k: getattr(self, k) for k in self.FIELDS}


class Engine:
    def __init__(self, device=None, **params):
        lib = L.load()
        if not torch.cuda.is_available():
            raise L.PgiError("no HIP device visible: the pose engine has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.params = L.default_params(**params)
        self._ctx = lib.pgi_create(self.device.index, C.byref(self.params))
        if not self._ctx:
            raise L.PgiError("pgi_create failed: " + L.last_error())
        self._lib = lib

    def close(self):
        if getattr(self, "_ctx", None):
            for child in list(getattr(self, "_children", ())):  # stores that live on this context go first
                child.close()
            self._lib.pgi_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def set_params(self, **kw):
        for k, v in kw.items():
            setattr(self.params, k, v)
        L.check(self._lib.pgi_set_params(self._ctx, C.byref(self.params)))

    def _bind_stream(self):
        L.check(self._lib.pgi_set_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def synchronize(self):
        L.check(self._lib.pgi_synchronize(self._ctx))

    # ---- batches -------------------------------------------------------------------------
    def upload(self, x1, y1, x2, y2, offsets, thr, guesses=None, has_guess=None, seed=0, pair_id_base=0):
        """Host (numpy) flattened SoA -> a device-resident batch dict."""
        dev = self.device
        off = np.ascontiguousarray(offsets, np.uint64)
        P = len(off) - 1
        b = dict(
            x1=torch.from_numpy(np.ascontiguousarray(x1, np.float32)).to(dev),
            y1=torch.from_numpy(np.ascontiguousarray(y1, np.float32)).to(dev),
            x2=torch.from_numpy(np.ascontiguousarray(x2, np.float32)).to(dev),
            y2=torch.from_numpy(np.ascontiguousarray(y2, np.float32)).to(dev),
            offsets=torch.from_numpy(off.view(np.int64)).to(dev),
            thr=torch.from_numpy(np.array(np.broadcast_to(thr, (P,)), np.float64)).to(dev),
            guesses=None, has_guess=None, n_pairs=P,
            max_corr=int(np.diff(off.astype(np.int64)).max()) if P else 0,
            seed=int(seed), pair_id_base=int(pair_id_base))
        if guesses is not None:
            b["guesses"] = torch.from_numpy(np.ascontiguousarray(guesses, np.float64).reshape(P, 12)).to(dev)
            hg = np.ones(P, np.uint8) if has_guess is None else np.ascontiguousarray(has_guess, np.uint8)
            b["has_guess"] = torch.from_numpy(hg).to(dev)
        return b

    def _batch_struct(self, b):
        s = L.Batch()
        s.d_x1, s.d_y1, s.d_x2, s.d_y2 = (b[k].data_ptr() for k in ("x1", "y1", "x2", "y2"))
        s.d_offsets = b["offsets"].data_ptr()
        s.d_thr = b["thr"].data_ptr()
        s.d_guess_Rt = b["guesses"].data_ptr() if b.get("guesses") is not None else None
        s.d_has_guess = b["has_guess"].data_ptr() if b.get("has_guess") is not None else None
        s.n_pairs, s.max_corr = b["n_pairs"], b["max_corr"]
        s.pair_id_base, s.seed = b["pair_id_base"], b["seed"]
        return s

    def estimate_pose_batch(self, b, edges=None, masks=None):
        """Enqueues estimatePose for every pair; returns (edges uint8[P,200], masks uint8[rows]) on device."""
        P, rows = b["n_pairs"], b["x1"].numel()
        if edges is None:
            edges = torch.empty((P, L.EDGE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        if masks is None:
            masks = torch.empty(max(rows, 1), dtype=torch.uint8, device=self.device)
        self._bind_stream()
        s = self._batch_struct(b)
        L.check(self._lib.pgi_estimate_pose_batch(self._ctx, C.byref(s), _ptr(edges), _ptr(masks)))
        return edges, masks[:rows]

    def estimate_pose_batch_host(self, x1, y1, x2, y2, offsets, thr, guesses=None, has_guess=None, seed=0, pair_id_base=0,
                                 out=None):
        """Host (numpy) SoA in, (edges structured array, masks) out; copies are pipelined against the kernels.
        out = (edges, masks): caller-provided (e.g. pinned) result arrays."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x1, y1, x2, y2 = f(x1), f(y1), f(x2), f(y2)
        off = np.ascontiguousarray(offsets, np.uint64)
        P = len(off) - 1
        thr = np.array(np.broadcast_to(thr, (P,)), np.float64)
        g = hg = None
        if guesses is not None:
            g = np.ascontiguousarray(guesses, np.float64).reshape(P, 12)
            hg = np.ones(P, np.uint8) if has_guess is None else np.ascontiguousarray(has_guess, np.uint8)
        if out is None:
            edges = np.zeros(P, L.EDGE_DTYPE)
            masks = np.zeros(max(int(off[-1] - off[0]), 1), np.uint8)
        else:
            edges, masks = out
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        L.check(self._lib.pgi_estimate_pose_batch_host(self._ctx, p(x1), p(y1), p(x2), p(y2), p(off), p(thr), p(g), p(hg), P,
                                                       int(pair_id_base), int(seed), p(edges), p(masks)))
        return edges, masks[:int(off[-1] - off[0])]

    def pin(self, *arrays):
        """Page-locks numpy arrays (pgi_host_register) so estimate_pose_batch_host moves them by asynchronous DMA; returns
        them.  Call unpin() on the same arrays before they are freed."""
        for a in arrays:
            if a.nbytes:
                L.check(self._lib.pgi_host_register(a.ctypes.data_as(C.c_void_p), a.nbytes))
        return arrays

    def unpin(self, *arrays):
        for a in arrays:
            if a.nbytes:
                L.check(self._lib.pgi_host_unregister(a.ctypes.data_as(C.c_void_p)))

    @staticmethod
    def edges_to_numpy(edges):
        return edges.cpu().numpy().view(L.EDGE_DTYPE).reshape(-1)

    def score_pose_batch(self, b, E, tau2, want_masks=True):
        P, rows = b["n_pairs"], b["x1"].numel()
        E = torch.as_tensor(np.ascontiguousarray(E, np.float64).reshape(P, 9)).to(self.device)
        tau2 = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(tau2, (P,)), np.float64)).to(self.device)
        counts = torch.empty(P, dtype=torch.int32, device=self.device)
        masks = torch.empty(max(rows, 1), dtype=torch.uint8, device=self.device) if want_masks else None
        self._bind_stream()
        s = self._batch_struct(b)
        L.check(self._lib.pgi_score_pose_batch(self._ctx, C.byref(s), _ptr(E), _ptr(tau2), _ptr(counts), _ptr(masks)))
        return counts, (masks[:rows] if want_masks else None)

    def score_pose_f64(self, corr_aos, offsets, E, tau2):
        """Reference-layout rows (n x 4 f64, cv::Mat N x 4 CV_64F) and arithmetic."""
        off = np.ascontiguousarray(offsets, np.uint64)
        P = len(off) - 1
        dev = self.device
        c = torch.from_numpy(np.ascontiguousarray(corr_aos, np.float64)).to(dev)
        o = torch.from_numpy(off.view(np.int64)).to(dev)
        E = torch.from_numpy(np.ascontiguousarray(E, np.float64).reshape(P, 9)).to(dev)
        t2 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(tau2, (P,)), np.float64)).to(dev)
        counts = torch.empty(P, dtype=torch.int32, device=dev)
        masks = torch.empty(max(len(corr_aos), 1), dtype=torch.uint8, device=dev)
        self._bind_stream()
        L.check(self._lib.pgi_score_pose_f64(self._ctx, _ptr(c), _ptr(o), P, _ptr(E), _ptr(t2), _ptr(counts),
                                             _ptr(masks)))
        return counts.cpu().numpy().astype(np.uint32), masks[:len(corr_aos)].cpu().numpy()

    def score_pose_host(self, corr_aos, E, tau2, early_exit_at=0, want_mask=True):
        """One pair, host pointers, re-entrant (pgi_score_pose_f64_host): getInliers (early_exit_at = 0, mask) /
        InTraversalPoseTester::test (early_exit_at = kMinimumInlierNumber, no mask) -> (reached, count, mask or None)."""
        c = np.ascontiguousarray(corr_aos, np.float64).reshape(-1, 4)
        Ed = np.ascontiguousarray(E, np.float64).reshape(9)
        n = len(c)
        mask = np.zeros(n, np.uint8) if want_mask else None
        cnt = C.c_uint32(0)
        rc = self._lib.pgi_score_pose_f64_host(self._ctx, c.ctypes.data_as(C.c_void_p), C.c_uint32(n), Ed.ctypes.data_as(C.c_void_p),
                                               C.c_double(tau2), C.c_uint32(early_exit_at), C.byref(cnt),
                                               mask.ctypes.data_as(C.c_void_p) if want_mask and n else None)
        if rc < 0:
            L.check(rc)
        return rc == 1, int(cnt.value), mask

    def pose_from_essential_host(self, E, corr_aos, mask=None):
        """pose::getPoseFromEssentialMatrix (pose_utils.h:172-252) for ONE pair with host pointers, re-entrant
        (pgi_pose_from_essential_host): -> (R[3,3], t[3], votes, cand).  mask None: every row votes (the reference)."""
        c = np.ascontiguousarray(corr_aos, np.float64).reshape(-1, 4)
        Ed = np.ascontiguousarray(E, np.float64).reshape(9)
        n = len(c)
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        if m is not None and len(m) != n:
            raise ValueError("mask must have one byte per row")
        R, t = np.zeros(9), np.zeros(3)
        votes, cand = C.c_uint32(0), C.c_uint32(0)
        L.check(self._lib.pgi_pose_from_essential_host(self._ctx, Ed.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p) if n else None,
                                                       C.c_uint32(n), m.ctypes.data_as(C.c_void_p) if m is not None and n else None,
                                                       R.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.byref(votes), C.byref(cand)))
        return R.reshape(3, 3), t, int(votes.value), int(cand.value)

    def decompose_batch(self, b, E, masks=None):
        P = b["n_pairs"]
        E = torch.as_tensor(np.ascontiguousarray(E, np.float64).reshape(P, 9)).to(self.device)
        edges = torch.zeros((P, L.EDGE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        self._bind_stream()
        s = self._batch_struct(b)
        L.check(self._lib.pgi_decompose_batch(self._ctx, C.byref(s), _ptr(E), _ptr(masks), _ptr(edges)))
        return edges

    def five_point_batch(self, pts, debug=False):
        """pts: [S,5,4] float32 -> (models [S,10,9] f32, counts [S], dbg [S,358] f64 or None)."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 5, 4)
        S = len(pts)
        d_pts = torch.from_numpy(pts).to(self.device)
        models = torch.zeros((S, 10, 9), dtype=torch.float32, device=self.device)
        counts = torch.zeros(S, dtype=torch.int32, device=self.device)
        dbg = torch.zeros((S, L.DBG_DOUBLES), dtype=torch.float64, device=self.device) if debug else None
        self._bind_stream()
        L.check(self._lib.pgi_five_point_batch(self._ctx, _ptr(d_pts), S, _ptr(models), _ptr(counts), _ptr(dbg)))
        return models.cpu().numpy(), counts.cpu().numpy(), (dbg.cpu().numpy() if debug else None)

    # ---- rotation averaging -----------------------------------------------------------------------
    def rotation_average(self, src, dst, R_rel, weight, n_views, **kw):
        """L1 + IRLS rotation averaging over edges (src, dst, R_dst_src, weight) -> (R[n_views,3,3], iters)."""
        E = len(src)
        edges = np.zeros(E, L.ROT_EDGE_DTYPE)
        edges["src"], edges["dst"] = src, dst
        edges["R"] = np.asarray(R_rel, np.float64).reshape(E, 9)
        edges["weight"] = weight
        prm = L.RotAvgParams()
        self._lib.pgi_default_rotavg_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(prm, k, v)
        R = np.zeros((n_views, 3, 3))
        iters = C.c_uint32(0)
        self._bind_stream()
        L.check(self._lib.pgi_rotation_average(self._ctx, edges.ctypes.data_as(C.c_void_p), E, n_views, C.byref(prm),
                                               R.ctypes.data_as(C.c_void_p), C.byref(iters)))
        return R, iters.value

    def rotation_average_edges(self, edges, src, dst, rows, n_views, **kw):
        """The same solve fed from the device-resident edge table (uint8 [P, 200], e.g. the output of allgather_edges):
        only status / n_inl and the spanning forest's rotations travel to the host.  weight = n_inl / rows.
        -> (R[n_views,3,3], iters, edges_used)"""
        P = int(edges.shape[0])
        src = np.ascontiguousarray(src, np.uint32)
        dst = np.ascontiguousarray(dst, np.uint32)
        rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        prm = L.RotAvgParams()
        self._lib.pgi_default_rotavg_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(prm, k, v)
        R = np.zeros((n_views, 3, 3))
        iters, used = C.c_uint32(0), C.c_uint32(0)
        self._bind_stream()
        L.check(self._lib.pgi_rotation_average_edges(
            self._ctx, _ptr(edges), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
            None if rows is None else rows.ctypes.data_as(C.c_void_p), P, n_views, C.byref(prm), R.ctypes.data_as(C.c_void_p),
            C.byref(iters), C.byref(used)))
        return R, iters.value, used.value

    # ---- translation averaging --------------------------------------------------------------------
    def _transavg_params(self, kw):
        prm = L.TransAvgParams()
        self._lib.pgi_default_transavg_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(prm, k, v)
        return prm

    def translation_average(self, src, dst, directions, weight, n_views, **kw):
        """Robust LUD translation averaging over edges (src, dst, unit world direction of c_src - c_dst, weight)
        -> (c[n_views,3], iters).  The smallest view of every component sits at 0; the shortest baselines are ~1."""
        E = len(src)
        edges = np.zeros(E, L.TRANS_EDGE_DTYPE)
        edges["src"], edges["dst"] = src, dst
        edges["dir"] = np.asarray(directions, np.float64).reshape(E, 3)
        edges["weight"] = weight
        prm = self._transavg_params(kw)
        c = np.zeros((n_views, 3))
        iters = C.c_uint32(0)
        self._bind_stream()
        L.check(self._lib.pgi_translation_average(self._ctx, edges.ctypes.data_as(C.c_void_p), E, n_views, C.byref(prm),
                                                  c.ctypes.data_as(C.c_void_p), C.byref(iters)))
        return c, iters.value

    def translation_average_edges(self, edges, src, dst, rows, n_views, R_global, **kw):
        """The same solve fed from the device-resident edge table (uint8 [P, 200]) and the global rotations
        (world->camera, [n_views, 3, 3], e.g. from rotation_average_edges): direction = R_dst^T t of every OK record,
        weight = n_inl / rows.  -> (c[n_views,3], iters, edges_used)"""
        P = int(edges.shape[0])
        src = np.ascontiguousarray(src, np.uint32)
        dst = np.ascontiguousarray(dst, np.uint32)
        rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        Rg = np.ascontiguousarray(R_global, np.float64).reshape(-1)
        if Rg.size != 9 * n_views:
            raise ValueError("R_global must hold n_views 3 x 3 matrices")
        prm = self._transavg_params(kw)
        c = np.zeros((n_views, 3))
        iters, used = C.c_uint32(0), C.c_uint32(0)
        self._bind_stream()
        L.check(self._lib.pgi_translation_average_edges(
            self._ctx, _ptr(edges), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
            None if rows is None else rows.ctypes.data_as(C.c_void_p), P, n_views, Rg.ctypes.data_as(C.c_void_p), C.byref(prm),
            c.ctypes.data_as(C.c_void_p), C.byref(iters), C.byref(used)))
        return c, iters.value, used.value

    # ---- cycle-consistency edge filter ------------------------------------------------------------
    def _cycle_params(self, kw):
        prm = L.CycleParams()
        self._lib.pgi_default_cycle_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(prm, k, v)
        return prm

    @staticmethod
    def _cycle_summary(s):
        return {k: int(getattr(s, k)) for k, _ in L.CycleSummary._fields_}

    def cycle_filter(self, src, dst, R_rel, t, n_views, **params):
        """Triplet checks over the edges (src, dst, R_dst_src, unit t_dst_src), every edge taking part (pgi_cycle_filter;
        tests/cycle_spec.py).  -> (keep u8 [E], n_tri u32 [E], n_good u32 [E] as CPU tensors, summary dict)."""
        E = len(src)
        edges = np.zeros(E, L.CYCLE_EDGE_DTYPE)
        edges["src"], edges["dst"] = src, dst
        edges["R"] = np.asarray(R_rel, np.float64).reshape(E, 9)
        edges["t"] = np.asarray(t, np.float64).reshape(E, 3)
        prm = self._cycle_params(params)
        keep, n_tri, n_good = np.zeros(E, np.uint8), np.zeros(E, np.uint32), np.zeros(E, np.uint32)
        summary = L.CycleSummary()
        p = lambda a: a.ctypes.data_as(C.c_void_p) if E else None
        self._bind_stream()
        L.check(self._lib.pgi_cycle_filter(self._ctx, p(edges), E, n_views, C.byref(prm), p(keep), p(n_tri), p(n_good),
                                           C.byref(summary)))
        return (torch.from_numpy(keep), torch.from_numpy(n_tri.view(np.int32)), torch.from_numpy(n_good.view(np.int32)),
                self._cycle_summary(summary))

    def cycle_filter_edges(self, edges, src, dst, n_views, out=None, **params):
        """The same on the device-resident edge table (uint8 [P, 200], e.g. the output of allgather_edges): records whose
        status is not EDGE_OK take no part.  out: None = no table is written; `edges` itself = in place; another uint8
        [P, 200] device tensor = receives the table with EDGE_INCONSISTENT on the OK records that were not kept.
        -> (keep u8 [P], n_tri i32 [P], n_good i32 [P] as device tensors, summary dict)"""
        P = int(edges.shape[0])
        src = np.ascontiguousarray(src, np.uint32)
        dst = np.ascontiguousarray(dst, np.uint32)
        if len(src) != P or len(dst) != P:
            raise ValueError("src and dst must have one entry per record")
        if out is not None and (out.dtype != torch.uint8 or out.numel() != P * L.EDGE_DTYPE.itemsize or not out.is_contiguous()
                                or out.device != edges.device):
            raise ValueError("out must be a contiguous uint8 [P, 200] tensor on the table's device")
        prm = self._cycle_params(params)
        keep = torch.zeros(P, dtype=torch.uint8, device=self.device)
        n_tri = torch.zeros(P, dtype=torch.int32, device=self.device)
        n_good = torch.zeros(P, dtype=torch.int32, device=self.device)
        summary = L.CycleSummary()
        self._bind_stream()
        L.check(self._lib.pgi_cycle_filter_edges(
            self._ctx, _ptr(edges) if P else None, src.ctypes.data_as(C.c_void_p) if P else None,
            dst.ctypes.data_as(C.c_void_p) if P else None, P, n_views, C.byref(prm), _ptr(keep), _ptr(n_tri), _ptr(n_good),
            C.byref(summary), _ptr(out) if P else None))
        return keep, n_tri, n_good, self._cycle_summary(summary)

    # ---- triangulation of tracks ------------------------------------------------------------------
    def _triangulate_args(self, keypoints, R, c, has_pose, kw):
        """-> (view array, R, c, has_pose, n_views, params): the host arguments pgi_triangulate_tracks and
        pgi_tracklets_triangulate share."""
        prm = L.TriangulateParams()
        self._lib.pgi_default_triangulate_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k) or k == "reserved":
                raise TypeError("unknown parameter %r" % k)
            setattr(prm, k, v)
        V = len(keypoints)
        Rh = np.ascontiguousarray(R, np.float64).reshape(-1)
        ch = np.ascontiguousarray(c, np.float64).reshape(-1)
        if Rh.size != 9 * V or ch.size != 3 * V:
            raise ValueError("R and c must hold one rotation and one centre per view")
        hp = None if has_pose is None else np.ascontiguousarray(np.asarray(has_pose) != 0, np.uint8)
        if hp is not None and hp.size != V:
            raise ValueError("has_pose must have one entry per view")
        views = (L.KeypointView * max(V, 1))()
        for v, kp in enumerate(keypoints):
            views[v].d_xy, views[v].n = (kp["xy"].data_ptr() if kp["n"] else None), kp["n"]
            views[v].fx, views[v].fy, views[v].cx, views[v].cy = kp["fx"], kp["fy"], kp["cx"], kp["cy"]
        return views, Rh, ch, hp, V, prm

    def _triangulate_outputs(self, T, M, err_rms, n_used, obs_state):
        dev = self.device
        return (torch.empty((T, 3), dtype=torch.float64, device=dev), torch.empty(T, dtype=torch.uint8, device=dev),
                torch.empty(T, dtype=torch.float64, device=dev) if err_rms else None,
                torch.empty(T, dtype=torch.int32, device=dev) if n_used else None,
                torch.empty(M, dtype=torch.uint8, device=dev) if obs_state else None)

    def triangulate_tracks(self, track_begin, members, keypoints, R, c, has_pose=None, err_rms=True, n_used=True,
                           obs_state=True, **params):
        """Sparse 3-D points of multi-view tracks (pgi_triangulate_tracks; specification tests/triangulate_spec.py).
        track_begin [T + 1] and members [(view << 32 | keypoint)]: numpy arrays or device tensors (int32 / int64 bit
        patterns); keypoints: one upload_keypoints() object per view; R [V,3,3] world->camera (rotation_average), c [V,3]
        centres (translation_average); has_pose [V] or None = all.  params: min_views, refine_iters, max_drops, thr_px,
        min_angle_deg.  err_rms / n_used / obs_state = False leaves that output out.  -> Triangulation."""
        dev = self.device
        if torch.is_tensor(track_begin):
            tb = track_begin.to(dev)
        else:
            tb = torch.from_numpy(np.array(track_begin, np.uint32).view(np.int32)).to(dev)
        if torch.is_tensor(members):
            mem = members.to(dev)
        else:
            mem = torch.from_numpy(np.array(members, np.uint64).view(np.int64)).to(dev)
        if tb.element_size() != 4 or mem.element_size() != 8:
            raise ValueError("track_begin must be 32-bit and members 64-bit")
        T, M = max(int(tb.numel()) - 1, 0), int(mem.numel())
        views, Rh, ch, hp, V, prm = self._triangulate_args(keypoints, R, c, has_pose, params)
        X, status, err, nu, st = self._triangulate_outputs(T, M, err_rms, n_used, obs_state)
        counts = np.zeros(L.TRI_STATUS_COUNT, np.uint32)
        self._bind_stream()
        L.check(self._lib.pgi_triangulate_tracks(
            self._ctx, _ptr(tb) if T else None, _ptr(mem) if M else None, T, views, Rh.ctypes.data_as(C.c_void_p),
            ch.ctypes.data_as(C.c_void_p), None if hp is None else hp.ctypes.data_as(C.c_void_p), V, C.byref(prm), _ptr(X),
            _ptr(err), _ptr(nu), _ptr(status), _ptr(st) if M else None, counts.ctypes.data_as(C.c_void_p)))
        return Triangulation(X, status, err, nu, st, counts)

    # ---- bundle adjustment -------------------------------------------------------------------------
    def _bundle_args(self, keypoints, R, c, X, status, obs_state, has_pose, fixed, T, M, kw):
        """-> the arguments pgi_bundle_adjust and pgi_tracklets_bundle_adjust share, and what must outlive the call."""
        prm = L.BundleParams()
        self._lib.pgi_default_bundle_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(prm, k, v)
        views, Rh, ch, hp, V, _ = self._triangulate_args(keypoints, R, c, has_pose, {})
        Rh, ch = Rh.copy(), ch.copy()  # in-out: the caller's arrays stay as they are
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
        if fx is not None and fx.size != V:
            raise ValueError("fixed must have one entry per view")
        dev = self.device
        Xd = (X.to(dev, torch.float64) if torch.is_tensor(X) else torch.from_numpy(np.array(X, np.float64)).to(dev)).reshape(-1, 3).clone()
        st = status.to(dev) if torch.is_tensor(status) else torch.from_numpy(np.array(status, np.uint8)).to(dev)
        ob = obs_state.to(dev) if torch.is_tensor(obs_state) else torch.from_numpy(np.array(obs_state, np.uint8)).to(dev)
        if Xd.shape[0] != T or st.numel() != T or ob.numel() != M or st.element_size() != 1 or ob.element_size() != 1:
            raise ValueError("X [T,3], status [T] and obs_state [members] (bytes) must match the tracks")
        rep = L.BundleReport()
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        args = (views, ptr(Rh), ptr(ch), ptr(hp), ptr(fx), V, C.byref(prm), _ptr(Xd) if T else None, _ptr(st) if T else None,
                _ptr(ob) if M else None, C.byref(rep))
        return args, (Rh.reshape(V, 3, 3), ch.reshape(V, 3), Xd, rep), (views, hp, fx, st, ob, prm)

    @staticmethod
    def _focal_keywords(refine_focal, focal, focal_fixed):
        """focal / focal_fixed without refine_focal would be ignored and the result a pose-only one at unscaled focals."""
        if not refine_focal and (focal is not None or focal_fixed is not None):
            raise ValueError("focal and focal_fixed need refine_focal=True")

    @staticmethod
    def _focal_args(args, V, focal, focal_fixed, min_focal_obs):
        """The shared arguments extended to those of the *_focal entries -> (args, phi [V] (a copy), n_free_focals, keep)."""
        phi = np.ones(V, np.float64) if focal is None else np.array(focal, np.float64).reshape(-1)
        ff = None if focal_fixed is None else np.ascontiguousarray(np.asarray(focal_fixed) != 0, np.uint8)
        if phi.size != V or (ff is not None and ff.size != V):
            raise ValueError("focal and focal_fixed must have one entry per view")
        n = C.c_uint32(0)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return args[:-1] + (ptr(phi), ptr(ff), int(min_focal_obs), args[-1], C.byref(n)), phi, n, (ff,)

    def bundle_adjust(self, track_begin, members, keypoints, R, c, X, status, obs_state, has_pose=None, fixed=None, focal=None,
                      focal_fixed=None, min_focal_obs=30, refine_focal=False, **params):
        """Joint refinement of poses and points (pgi_bundle_adjust; specification tests/bundle_spec.py).  Tracks, keypoints,
        R, c and has_pose as in triangulate_tracks; X, status and obs_state as it returned them (arrays or device tensors);
        fixed [V] or None = the first posed view with observations holds the gauge.  params: iters, cg_iters, min_cam_obs,
        use_low_parallax, huber_px, cg_tol, ftol, lambda_init.  The inputs are not modified.  -> BundleResult.
        refine_focal=True (pgi_bundle_adjust_focal; specification tests/bundle_focal_spec.py): each view's focal scale phi
        (focal [V], None = 1) joins the unknowns where the view is posed, not marked in focal_fixed and has at least
        min_focal_obs participating observations (30 is a choice, not a measurement); the result carries focal and
        n_free_focals.  The caller multiplies fx, fy by the returned focal before triangulating again."""
        dev = self.device
        tb = track_begin.to(dev) if torch.is_tensor(track_begin) else torch.from_numpy(np.array(track_begin, np.uint32).view(np.int32)).to(dev)
        mem = members.to(dev) if torch.is_tensor(members) else torch.from_numpy(np.array(members, np.uint64).view(np.int64)).to(dev)
        if tb.element_size() != 4 or mem.element_size() != 8:
            raise ValueError("track_begin must be 32-bit and members 64-bit")
        T, M = max(int(tb.numel()) - 1, 0), int(mem.numel())
        args, (Rh, ch, Xd, rep), keep = self._bundle_args(keypoints, R, c, X, status, obs_state, has_pose, fixed, T, M, params)
        self._bind_stream()
        self._focal_keywords(refine_focal, focal, focal_fixed)
        if refine_focal:
            args, phi, n, keep2 = self._focal_args(args, len(Rh), focal, focal_fixed, min_focal_obs)
            L.check(self._lib.pgi_bundle_adjust_focal(self._ctx, _ptr(tb) if T else None, _ptr(mem) if M else None, T, *args))
            return BundleResult(Rh, ch, Xd, rep, phi, n.value)
        L.check(self._lib.pgi_bundle_adjust(self._ctx, _ptr(tb) if T else None, _ptr(mem) if M else None, T, *args))
        return BundleResult(Rh, ch, Xd, rep)

    # ---- multi-GPU exchange (include/pgi.h: pgi_comm_*, pgi_allgather_edges) ----------------------------------------
    def comm_info(self):
        w, r, k = C.c_uint32(1), C.c_uint32(0), C.c_uint32(0)
        L.check(self._lib.pgi_comm_info(self._ctx, C.byref(w), C.byref(r), C.byref(k)))
        return w.value, r.value, ("none", "rccl", "host")[k.value]

    def allgather_edges(self, local_edges, counts, out=None):
        """local_edges: uint8 [P_r, 200] on this engine's device; counts[r] = records of rank r (counts[rank] == P_r).
        Returns the [sum(counts), 200] table in rank order (asynchronous on the current stream with RCCL)."""
        counts = np.ascontiguousarray(counts, np.uint32)
        total = int(counts.sum())
        if out is None:
            out = torch.empty((total, L.EDGE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        self._bind_stream()
        L.check(self._lib.pgi_allgather_edges(self._ctx, _ptr(local_edges) if local_edges.numel() else None,
                                              counts.ctypes.data_as(C.c_void_p), _ptr(out)))
        return out

    # ---- descriptor matching (feature_utils.h:135-202) ------------------------------------------
    def prepare_descriptors(self, desc, screen=True):
        """n x 128 float32 (numpy or device tensor) -> prepared image (transposed copy + norms in HBM; with screen=True
        also the padded row-major copy and its half-precision rounding that enable the screened matcher)."""
        d = torch.as_tensor(np.ascontiguousarray(desc, np.float32) if isinstance(desc, np.ndarray) else desc,
                            dtype=torch.float32, device=self.device).contiguous()
        n = int(d.shape[0])
        if n and d.shape[1] != 128:
            raise ValueError("descriptors must be n x 128")
        n_pad = int(self._lib.pgi_desc_padded(n))
        dt = torch.empty((128, max(n_pad, 1)), dtype=torch.float32, device=self.device)
        nrm = torch.empty(max(n_pad, 1), dtype=torch.float32, device=self.device)
        self._bind_stream()
        L.check(self._lib.pgi_desc_prepare(self._ctx, _ptr(d) if n else None, n, _ptr(dt), _ptr(nrm)))
        im = {"t": dt, "norm": nrm, "n": n, "n_pad": n_pad, "rm": None, "f16": None}
        if screen:
            im["rm"] = torch.empty((max(n_pad, 1), 128), dtype=torch.float32, device=self.device)
            im["f16"] = torch.empty((max(n_pad, 1), 128), dtype=torch.int16, device=self.device)
            L.check(self._lib.pgi_desc_prepare_screen(self._ctx, _ptr(d) if n else None, n, _ptr(im["rm"]), _ptr(im["f16"])))
        return im

    def match_descriptors_batch(self, images, pairs, max_matches=None, raw=False):
        """images: list of prepared images; pairs: [(src, dst)] -> per pair (src_idx, dst_idx, ratio) sorted by ratio.
        raw=True returns the device tensors (src, dst, ratio, counts) without a host copy."""
        P = len(pairs)
        if max_matches is None:
            max_matches = max([images[s]["n"] for s, _ in pairs] + [1])
        va, vb = (L.DescView * max(P, 1))(), (L.DescView * max(P, 1))()
        for p, (s, d) in enumerate(pairs):
            for v, im in ((va[p], images[s]), (vb[p], images[d])):
                v.d_desc_t, v.d_norm, v.n, v.n_pad = im["t"].data_ptr(), im["norm"].data_ptr(), im["n"], im["n_pad"]
                v.d_desc_rm = im["rm"].data_ptr() if im.get("rm") is not None else None
                v.d_desc_f16 = im["f16"].data_ptr() if im.get("f16") is not None else None
        src = torch.empty((max(P, 1), max_matches), dtype=torch.int32, device=self.device)
        dst = torch.empty_like(src)
        ratio = torch.empty((max(P, 1), max_matches), dtype=torch.float64, device=self.device)
        counts = torch.zeros(max(P, 1), dtype=torch.int32, device=self.device)
        self._bind_stream()
        L.check(self._lib.pgi_match_descriptors_batch(self._ctx, va, vb, P, max_matches, _ptr(src), _ptr(dst), _ptr(ratio),
                                                      _ptr(counts)))
        if raw:
            return src, dst, ratio, counts
        c = counts.cpu().numpy()
        s_h, d_h, r_h = src.cpu().numpy(), dst.cpu().numpy(), ratio.cpu().numpy()
        return [(s_h[p, :c[p]].astype(np.uint32), d_h[p, :c[p]].astype(np.uint32), r_h[p, :c[p]]) for p in range(P)]

    def upload_keypoints(self, xy, f, w, h):
        """cv::KeyPoint::pt array (n x 2 pixels) + pinhole camera K = [f 0 w/2; 0 f h/2] (pose_graph_builder.h:286)."""
        t = torch.as_tensor(np.ascontiguousarray(xy, np.float32).reshape(-1, 2)).to(self.device)
        return {"xy": t, "n": int(t.shape[0]), "fx": float(f), "fy": float(f), "cx": w / 2.0, "cy": h / 2.0,
                "width": float(w), "height": float(h)}

    def build_correspondences(self, keypoints, pairs, matches, thr_px, top_k=0, dst_uses_src_intrinsics=False, seed=0,
                              pair_id_base=0):
        """createCorrespondenceMatrix on the device (pose_graph_builder.h:864-938): `matches` is the raw output of
        match_descriptors_batch(..., raw=True); returns a batch dict for estimate_pose_batch."""
        src, dst, _, counts = matches
        P, mm = len(pairs), int(src.shape[1])
        va, vb = (L.KeypointView * max(P, 1))(), (L.KeypointView * max(P, 1))()
        for p, (s, d) in enumerate(pairs):
            for v, kp in ((va[p], keypoints[s]), (vb[p], keypoints[d])):
                v.d_xy, v.n = (kp["xy"].data_ptr() if kp["n"] else None), kp["n"]
                v.fx, v.fy, v.cx, v.cy = kp["fx"], kp["fy"], kp["cx"], kp["cy"]
        cap = min(mm, top_k) if top_k else mm
        rows = max(P * cap, 1)
        b = dict(x1=torch.empty(rows, dtype=torch.float32, device=self.device), guesses=None, has_guess=None, n_pairs=P,
                 max_corr=cap, seed=int(seed), pair_id_base=int(pair_id_base))
        for k in ("y1", "x2", "y2"):
            b[k] = torch.empty_like(b["x1"])
        b["offsets"] = torch.zeros(P + 1, dtype=torch.int64, device=self.device)
        b["thr"] = torch.zeros(max(P, 1), dtype=torch.float64, device=self.device)
        self._bind_stream()
        L.check(self._lib.pgi_build_correspondences(
            self._ctx, va, vb, P, mm, _ptr(src), _ptr(dst), _ptr(counts), int(top_k), float(thr_px),
            int(bool(dst_uses_src_intrinsics)), _ptr(b["x1"]), _ptr(b["y1"]), _ptr(b["x2"]), _ptr(b["y2"]), _ptr(b["offsets"]),
            _ptr(b["thr"])))
        return b

    def upload_features(self, xy, desc, f, w, h):
        """Keypoints (n x 2 px) + row-major descriptors (n x 128) of one image, for guided matching."""
        kp = self.upload_keypoints(xy, f, w, h)
        kp["desc"] = torch.as_tensor(np.ascontiguousarray(desc, np.float32).reshape(-1, 128)).to(self.device)
        return kp

    def guided_match_batch(self, features, pairs, poses_Rt, max_n=100, raw=False, n_bins=45):
        """HashingBasedMatcherWithPose::match + the top-N cut of guidedMatching (matcher.h:199-405,
        pose_graph_builder.h:715-783) for every (src, dst) pair with pose (R, t) = poses_Rt[p] (12 doubles).
        n_bins = 45 is the reference's epipolar hashing; n_bins = 0 visits every destination keypoint."""
        P = len(pairs)
        va, vb = (L.FeatureView * max(P, 1))(), (L.FeatureView * max(P, 1))()
        for p, (s, d) in enumerate(pairs):
            for v, ft in ((va[p], features[s]), (vb[p], features[d])):
                v.d_xy = ft["xy"].data_ptr() if ft["n"] else None
                v.d_desc = ft["desc"].data_ptr() if ft["n"] else None
                v.n, v.fx, v.fy, v.cx, v.cy = ft["n"], ft["fx"], ft["fy"], ft["cx"], ft["cy"]
                v.width, v.height = ft.get("width", 2.0 * ft["cx"]), ft.get("height", 2.0 * ft["cy"])
        stride = max_n if max_n else max([features[s]["n"] for s, _ in pairs] + [1])
        pose = np.ascontiguousarray(poses_Rt, np.float64).reshape(max(P, 0), 12)
        src = torch.empty((max(P, 1), stride), dtype=torch.int32, device=self.device)
        dst = torch.empty_like(src)
        ratio = torch.empty((max(P, 1), stride), dtype=torch.float64, device=self.device)
        counts = torch.zeros(max(P, 1), dtype=torch.int32, device=self.device)
        self._bind_stream()
        L.check(self._lib.pgi_guided_match_batch(self._ctx, va, vb, P, pose.ctypes.data_as(C.c_void_p), int(n_bins), int(max_n), stride,
                                                 _ptr(src), _ptr(dst), _ptr(ratio), _ptr(counts)))
        if raw:
            return src, dst, ratio, counts
        c = counts.cpu().numpy()
        s_h, d_h, r_h = src.cpu().numpy(), dst.cpu().numpy(), ratio.cpu().numpy()
        return [(s_h[p, :c[p]].astype(np.uint32), d_h[p, :c[p]].astype(np.uint32), r_h[p, :c[p]]) for p in range(P)]

    # ---- single-pair drop-in (host pointers) --------------------------------------------------
    def estimate_pose(self, corr_aos, thr, guesses=None, seed=0, pair_id=0, min_inliers=0):
        """estimatePose(corr N x 4 f64, thr, guesses) -> (ok, Edge, mask) (pose_graph_builder.h:940-1078).
        min_inliers: the seam's kMinimumInlierNumber_ for this call (0 = the engine's parameter).  Re-entrant:
        concurrent callers get private slots (stream + pinned staging) and overlap on the GPU."""
        c = np.ascontiguousarray(corr_aos, np.float64).reshape(-1, 4)
        g = None if guesses is None else np.ascontiguousarray(guesses, np.float64).reshape(-1, 12)
        e = L.Edge()
        mask = np.zeros(max(len(c), 1), np.uint8)
        self._bind_stream()
        rc = L.check(self._lib.pgi_estimate_pose(
            self._ctx, c.ctypes.data_as(C.c_void_p), len(c), float(thr),
            None if g is None else g.ctypes.data_as(C.c_void_p), 0 if g is None else len(g), int(min_inliers),
            int(seed), int(pair_id), C.byref(e), mask.ctypes.data_as(C.c_void_p)))
        return bool(rc), e, mask[:len(c)]


class DeviceTracklets:
    """reconstruction::Tracklets (point_track.h:541-711) resident in HBM: pgi_tracklets_* of include/pgi.h.
    add() takes one or many (src view, dst view, matches, mask) calls and applies them in order."""

    def __init__(self, engine, n_views):
        self.eng, self._lib = engine, engine._lib
        self._t = self._lib.pgi_tracklets_create(engine._ctx, int(n_views))
        if not self._t:
            raise L.PgiError("pgi_tracklets_create failed: " + L.last_error())
        if not hasattr(engine, "_children"):
            import weakref
            engine._children = weakref.WeakSet()
        engine._children.add(self)  # Engine.close() destroys its stores before its context

    def close(self):
        if getattr(self, "_t", None):
            if getattr(self.eng, "_ctx", None):  # (a store outliving its context is abandoned, never touched)
                self._lib.pgi_tracklets_destroy(self._t)
            self._t = None

    __del__ = close

    def add_batch(self, calls):
        """calls: [(src, dst, matches (m x 2 integer array-like or a pair of device int32 tensors), mask or None)]."""
        dev = self.eng.device
        n = len(calls)
        arr = (L.TrackletPair * max(n, 1))()
        keep = []
        for i, (s, d, m, mask) in enumerate(calls):
            if isinstance(m, tuple) and torch.is_tensor(m[0]):
                ts, td = m
            else:
                mm = np.asarray(m, np.int64).reshape(-1, 2)
                ts = torch.as_tensor(mm[:, 0].astype(np.int32)).to(dev)
                td = torch.as_tensor(mm[:, 1].astype(np.int32)).to(dev)
            tm = None
            if mask is not None:
                tm = mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask, np.uint8)).to(dev)
            keep += [ts, td, tm]
            arr[i].view_src, arr[i].view_dst, arr[i].n_max = int(s), int(d), int(ts.numel())
            arr[i].d_src = ts.data_ptr() if ts.numel() else None
            arr[i].d_dst = td.data_ptr() if td.numel() else None
            arr[i].d_mask = tm.data_ptr() if tm is not None and tm.numel() else None
            arr[i].d_count = None
        self.eng._bind_stream()
        L.check(self._lib.pgi_tracklets_add_batch(self._t, arr, n))

    def add(self, src, dst, matches, mask=None):
        self.add_batch([(src, dst, matches, mask)])

    def get_correspondences_batch(self, queries, max_n, raw=False):
        """[(src view, dst view)] -> per query an (m x 2) array of (source keypoint, destination keypoint)."""
        q = np.asarray(queries, np.uint32).reshape(-1, 2)
        n, stride = len(q), int(max_n) + 1
        vs, vd = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])
        dev = self.eng.device
        src = torch.empty((max(n, 1), stride), dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.eng._bind_stream()
        L.check(self._lib.pgi_tracklets_get_batch(self._t, vs.ctypes.data_as(C.c_void_p), vd.ctypes.data_as(C.c_void_p), n, int(max_n), stride,
                                                  _ptr(src), _ptr(dst), _ptr(cnt)))
        if raw:
            return src, dst, cnt
        c, s_h, d_h = cnt.cpu().numpy(), src.cpu().numpy(), dst.cpu().numpy()
        return [np.stack([s_h[i, :c[i]], d_h[i, :c[i]]], 1).astype(np.int64) for i in range(n)]

    def get_correspondences(self, src, dst, max_n):
        return self.get_correspondences_batch([(src, dst)], max_n)[0]

    def triangulate(self, keypoints, R, c, has_pose=None, err_rms=True, n_used=True, obs_state=True, **params):
        """Engine.triangulate_tracks on the store's current by-track ordering (pgi_tracklets_triangulate): track indices
        and member order are those of track(); no member leaves the device.  -> Triangulation."""
        eng = self.eng
        i = self.info()
        T, M = i["tracks"], i["events"]
        views, Rh, ch, hp, V, prm = eng._triangulate_args(keypoints, R, c, has_pose, params)
        X, status, err, nu, st = eng._triangulate_outputs(T, M, err_rms, n_used, obs_state)
        counts = np.zeros(L.TRI_STATUS_COUNT, np.uint32)
        eng._bind_stream()
        L.check(self._lib.pgi_tracklets_triangulate(
            self._t, views, Rh.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.c_void_p),
            None if hp is None else hp.ctypes.data_as(C.c_void_p), V, C.byref(prm), _ptr(X), _ptr(err), _ptr(nu), _ptr(status),
            _ptr(st) if M else None, counts.ctypes.data_as(C.c_void_p)))
        return Triangulation(X, status, err, nu, st, counts)

    def bundle_adjust(self, keypoints, R, c, X, status, obs_state, has_pose=None, fixed=None, focal=None, focal_fixed=None,
                      min_focal_obs=30, refine_focal=False, **params):
        """Engine.bundle_adjust on the store's current by-track ordering (pgi_tracklets_bundle_adjust, or
        pgi_tracklets_bundle_adjust_focal with refine_focal), e.g. with the X, status and obs_state of triangulate(); no
        member leaves the device.  -> BundleResult."""
        eng = self.eng
        i = self.info()
        args, (Rh, ch, Xd, rep), keep = eng._bundle_args(keypoints, R, c, X, status, obs_state, has_pose, fixed, i["tracks"], i["events"], params)
        eng._bind_stream()
        eng._focal_keywords(refine_focal, focal, focal_fixed)
        if refine_focal:
            args, phi, n, keep2 = eng._focal_args(args, len(Rh), focal, focal_fixed, min_focal_obs)
            L.check(self._lib.pgi_tracklets_bundle_adjust_focal(self._t, *args))
            return BundleResult(Rh, ch, Xd, rep, phi, n.value)
        L.check(self._lib.pgi_tracklets_bundle_adjust(self._t, *args))
        return BundleResult(Rh, ch, Xd, rep)

    def info(self):
        a, b, r = C.c_uint64(), C.c_uint64(), C.c_uint32()
        L.check(self._lib.pgi_tracklets_info(self._t, C.byref(a), C.byref(b), C.byref(r)))
        return {"tracks": a.value, "events": b.value, "rounds": r.value}

    def track(self, index):
        n = C.c_uint32()
        L.check(self._lib.pgi_tracklets_track(self._t, int(index), None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.uint64)
        L.check(self._lib.pgi_tracklets_track(self._t, int(index), buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return [(int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF))) for k in buf[:n.value]]
