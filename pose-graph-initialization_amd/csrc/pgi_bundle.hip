// pgi_bundle.hip -- bundle adjustment: joint refinement of the global poses and the triangulated points (include/pgi.h:
// pgi_bundle_adjust, pgi_tracklets_bundle_adjust).  Not in the reference.  The specification is tests/bundle_spec.py
// (DESIGN.md section 3, item 11): Levenberg-Marquardt with Marquardt damping on the Huber-weighted pixel reprojection
// error, normal equations in Schur form, Schur-Jacobi preconditioned CG on the reduced camera system.
//
// Gauge.  With no `fixed` mask the smallest-index posed view with participating observations is held.  The scale (and the
// frames of further components) stay free: the cost is invariant under them, so the gradient has no component along them,
// and with lambda > 0 the damped system is positive definite -- its step has no reason to move along the gauge.
//
// Data path (f64 throughout, -ffp-contract=off, no floating-point atomics, every sum in a fixed order: same input, same bits):
//   ba_count / ba_fill     one track per lane: the participating observations, compacted in track order (exclusive scan of
//                          the per-track counts); per-view counts by integer atomics
//   by-camera order        a stable rocPRIM radix sort of (view, observation) + the CSR of the per-view counts
//   ba_eval_kernel         one observation per lane: residual, depth sign, Huber class and weight, cost term; as the
//                          LINEARISATION it writes r, w, d r / d omega (2 x 3) and d r / d X (2 x 3) as SoA records, once in
//                          track order and once in camera order, so that BOTH matvec passes stream consecutive doubles
//                          (d r / d c = -d r / d X is not stored twice); as the TRIAL it adds the model decrease instead
//   ba_point_setup         one point per lane, members in member order: V + lambda D, V^-1 (adjugate), s = V^-1 g
//   ba_cam_setup           one wavefront per camera, lanes striding its list, xor-tree reduction of the 33 sums: the
//                          camera's diagonal block of S and its diagonal of U, the reduced right-hand side; lane 0 factors
//                          the block (6 x 6 Cholesky) and starts the PCG vectors
//   PCG iteration          ba_cg_dir (beta, stopping test, p = z + beta p) -> ba_point_pass (t_j = V_j^-1 sum_i W_ij^T p_i)
//                          -> ba_cam_pass (q_i = U_i p_i - sum_j W_ij t_j, one wavefront per camera) -> ba_cg_update
//                          (alpha, x, r, z).  S is never formed.  The scalars and the convergence flag stay on the device;
//                          once the state says "done" every launch returns at once, so WHERE the host looks changes no bit.
//   ba_point_pass<true>    the back-substitution of the point steps;  ba_apply_kernel: R <- exp([w]x) R, c += dc, X += dX
// A rejected step restores the view table and X from the copy saved before the update.
//
// Focal scales (pgi_bundle_adjust_focal, pgi_tracklets_bundle_adjust_focal; specification tests/bundle_focal_spec.py).  One
// scalar phi per view, fx = fx0 phi, fy = fy0 phi; d r / d phi = (fx0 a, fy0 b) is appended to the records (17 doubles) and the
// camera block is 7 x 7.  Every kernel that touches a camera block takes the block size NC as a template parameter; a view's
// flags say which of its parameters are free (pose, focal, both, none), and the rows and columns of the pinned ones are cleared
// after the sums, so that they hold lambda D alone and their PCG components stay exactly 0.  A per-view table (fx0, fy0, phi)
// is saved and restored with the view table.  A call with no focal-free view runs the NC = 6 kernels on the scaled table.
#include "pgi_internal.hpp"
#include "pgi_reduce.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace pgi {
namespace {

constexpr int kBaBlock = 256;
constexpr int kBaWave = 64;
constexpr int kBaCamsPerBlock = kBaBlock / kBaWave;
constexpr double kBaDiagMin = 1e-6, kBaDiagMax = 1e32;        // clamp of D = diag(J^T W J)
constexpr double kBaLambdaMin = 1e-12, kBaLambdaMax = 1e12;   // bounds of the damping factor
constexpr double kBaAcceptRatio = 1e-4;                       // ACCEPT_RATIO of the specification
constexpr uint32_t kBaPoll = 16;                              // PCG iterations between two looks at the state record
// record fields (SoA: field k of observation o at k * n_obs + o)
enum { REC_R0 = 0, REC_R1, REC_W, REC_JW = 3 /* u0 u1 u2 v0 v1 v2 */, REC_JP = 9 /* u0 u1 u2 v0 v1 v2 */, REC_FIELDS = 15,
       REC_JF = 15 /* u v: d r / d phi, the seven-parameter records only */ };
// NC = parameters per camera block: 6 (omega, c) or 7 (omega, c, phi: the focal scale, pgi_bundle_adjust_focal).  The
// six-parameter instantiation holds the statements of the pose-only solver in their order; what the seventh adds stands
// under `if constexpr (NC == 7)`.
template <int NC>
struct BaDim {
    static_assert(NC == 6 || NC == 7, "camera block size");
    static constexpr int kTri = NC * (NC + 1) / 2;             // packed lower triangle of the camera block
    static constexpr int kRec = NC == 7 ? REC_JF + 2 : REC_FIELDS;  // doubles per record
};
// per-view flags of the seven-parameter path (the six-parameter path keeps 0 / 1)
constexpr uint8_t kBaPoseFree = 1, kBaFocalFree = 2;

#define BDEV __device__ __forceinline__

struct BaCgState {
    double rz, rz0;
    uint32_t iters;
    int done;
};

// inverse of a symmetric 3 x 3 matrix (00 01 02 11 12 22) by its adjugate, the operation order of tri_solve_sym3
BDEV void ba_inv_sym3(const double* a, double* inv) {
    const double c00 = a[3] * a[5] - a[4] * a[4];
    const double c01 = a[2] * a[4] - a[1] * a[5];
    const double c02 = a[1] * a[4] - a[2] * a[3];
    const double c11 = a[0] * a[5] - a[2] * a[2];
    const double c12 = a[1] * a[2] - a[0] * a[4];
    const double c22 = a[0] * a[3] - a[1] * a[1];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
    inv[3] = c11 / det; inv[4] = c12 / det; inv[5] = c22 / det;
}
BDEV void ba_mul_sym3(const double* S, const double* v, double* y) {
    y[0] = (S[0] * v[0] + S[1] * v[1]) + S[2] * v[2];
    y[1] = (S[1] * v[0] + S[3] * v[1]) + S[4] * v[2];
    y[2] = (S[2] * v[0] + S[4] * v[1]) + S[5] * v[2];
}
// packed lower triangle, row-major: (i, j), j <= i, at i (i + 1) / 2 + j
BDEV constexpr int ba_tri(int i, int j) { return i * (i + 1) / 2 + j; }
// z = (L L^T)^-1 r; the diagonal of L holds the RECIPROCAL pivots
template <int NC>
BDEV void ba_chol_solve(const double* L, const double* r, double* z) {
    double y[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        double s = r[i];
#pragma unroll
        for (int j = 0; j < i; ++j) s -= L[ba_tri(i, j)] * y[j];
        y[i] = s * L[ba_tri(i, i)];
    }
#pragma unroll
    for (int i = NC - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int j = i + 1; j < NC; ++j) s -= L[ba_tri(j, i)] * z[j];
        z[i] = s * L[ba_tri(i, i)];
    }
}

// ---- preparation -----------------------------------------------------------------------------------------------------
struct BaPrep {
    const uint32_t* track_begin;
    const uint64_t* members;
    const uint8_t* obs_state;
    const uint8_t* status;
    const double* X;
    const uint32_t* kp_n;  // per view; 0 for a view without a pose
    uint32_t n_tracks, n_views, member_cap, use_low;
};
BDEV bool ba_member(const BaPrep& A, uint32_t m, uint32_t& v, uint32_t& kp) {
    const uint64_t key = A.members[m];
    v = (uint32_t)(key >> 32), kp = (uint32_t)key;
    return A.obs_state[m] == 1 && v < A.n_views && kp < A.kp_n[v];
}
BDEV void ba_track_range(const BaPrep& A, uint32_t t, uint32_t& beg, uint32_t& end) {
    end = A.track_begin[t + 1], beg = A.track_begin[t];
    if (end > A.member_cap) end = A.member_cap;
    if (beg > end) beg = end;
}
// cnt[t] = participating observations of track t (0 unless at least two); cnt[n_tracks] = 0 closes the scan
__global__ __launch_bounds__(kBaBlock) void ba_count_kernel(BaPrep A, uint32_t* __restrict__ cnt, uint32_t* __restrict__ n_points) {
    const uint32_t t = blockIdx.x * kBaBlock + threadIdx.x;
    if (t > A.n_tracks) return;
    uint32_t n = 0;
    if (t < A.n_tracks) {
        const uint32_t st = A.status[t];
        bool ok = st == PGI_TRI_OK || (A.use_low && st == PGI_TRI_LOW_PARALLAX);
        for (int k = 0; k < 3; ++k) ok = ok && isfinite(A.X[3 * (size_t)t + k]);
        if (ok) {
            uint32_t beg, end, v, kp;
            ba_track_range(A, t, beg, end);
            for (uint32_t m = beg; m < end; ++m) n += ba_member(A, m, v, kp) ? 1u : 0u;
        }
        if (n < 2) n = 0;
        if (n) atomicAdd(n_points, 1u);  // integer counter: the order of the additions does not matter
    }
    cnt[t] = n;
}
__global__ __launch_bounds__(kBaBlock) void ba_fill_kernel(BaPrep A, const uint32_t* __restrict__ obs_begin, const float* const* __restrict__ kp_xy,
                                                           uint32_t* __restrict__ obs_pt, uint32_t* __restrict__ obs_view,
                                                           uint32_t* __restrict__ obs_idx, double* __restrict__ pix,
                                                           uint32_t n_obs, uint32_t* __restrict__ cam_cnt) {
    const uint32_t t = blockIdx.x * kBaBlock + threadIdx.x;
    if (t >= A.n_tracks) return;
    uint32_t o = obs_begin[t];
    const uint32_t oe = obs_begin[t + 1];
    if (o == oe) return;
    uint32_t beg, end, v, kp;
    ba_track_range(A, t, beg, end);
    for (uint32_t m = beg; m < end && o < oe && o < n_obs; ++m) {
        if (!ba_member(A, m, v, kp)) continue;
        const float2 p = reinterpret_cast<const float2*>(kp_xy[v])[kp];
        obs_pt[o] = t;
        obs_view[o] = v;
        obs_idx[o] = o;
        pix[o] = (double)p.x;
        pix[(size_t)n_obs + o] = (double)p.y;
        atomicAdd(&cam_cnt[v], 1u);
        ++o;
    }
}
// cam_list[k] = observation at position k of the by-camera order -> its inverse and the point of every position
__global__ __launch_bounds__(kBaBlock) void ba_invert_kernel(const uint32_t* __restrict__ cam_list, const uint32_t* __restrict__ obs_pt,
                                                             uint32_t n_obs, uint32_t* __restrict__ cam_pos, uint32_t* __restrict__ cam_pt) {
    const uint32_t k = blockIdx.x * kBaBlock + threadIdx.x;
    if (k >= n_obs) return;
    const uint32_t o = cam_list[k];
    if (o >= n_obs) return;
    cam_pos[o] = k;
    cam_pt[k] = obs_pt[o];
}

// ---- residual, linearisation, trial cost -------------------------------------------------------------------------------
struct BaEval {
    const uint32_t* obs_pt;
    const uint32_t* obs_view;
    const uint32_t* cam_pos;
    const double* pix;    // px[n_obs], py[n_obs]
    const double* views;  // n_views x 16: R, c, fx fy cx cy
    const double* X;
    double* rec_t;        // records in track order
    double* rec_c;        // records in camera order
    const double* foc;    // n_views x 3: fx0 fy0 phi, the seven-parameter path only
    const double* x;      // camera steps (NC per view), trial only
    const double* dp;     // point steps (3 per track), trial only
    double* part_cost;    // per block
    double* part_pred;    // per block, trial only
    int* nonpos;
    uint32_t n_obs;
    double huber;
};
// TRIAL = false: writes the records.  TRIAL = true: reads the records of the linearisation point and adds the decrease
// the quadratic model predicts, w (|r|^2 - |r + J delta|^2).
template <bool TRIAL, int NC>
__global__ __launch_bounds__(kBaBlock) void ba_eval_kernel(BaEval A) {
    __shared__ double red[kBaBlock];
    const int tid = threadIdx.x;
    const uint32_t o = blockIdx.x * kBaBlock + (uint32_t)tid;
    const size_t N = A.n_obs;
    double rho = 0.0, pred = 0.0;
    if (o < A.n_obs) {
        const uint32_t t = A.obs_pt[o], v = A.obs_view[o];
        const double* w = A.views + (size_t)v * 16;
        const double px = A.pix[o], py = A.pix[N + o];
        const double dx0 = A.X[3 * (size_t)t] - w[9], dx1 = A.X[3 * (size_t)t + 1] - w[10], dx2 = A.X[3 * (size_t)t + 2] - w[11];
        const double q0 = (w[0] * dx0 + w[1] * dx1) + w[2] * dx2;
        const double q1 = (w[3] * dx0 + w[4] * dx1) + w[5] * dx2;
        const double q2 = (w[6] * dx0 + w[7] * dx1) + w[8] * dx2;
        bool ahead = q2 > 0.0;  // the depth sign: one comparison
        if constexpr (NC == 7) ahead = ahead && A.foc[3 * (size_t)v + 2] > 0.0;  // the focal scale: one comparison (a NaN fails it)
        if (ahead) {
            const double a = q0 / q2, b = q1 / q2, iz = 1.0 / q2;
            const double r0 = (w[12] * a + w[14]) - px;
            const double r1 = (w[13] * b + w[15]) - py;
            const double e2 = r0 * r0 + r1 * r1;
            const double e = sqrt(e2);
            const bool inl = e <= A.huber;  // the Huber class: one comparison
            const double wt = inl ? 1.0 : A.huber / e;
            rho = inl ? e2 : (2.0 * A.huber) * e - A.huber * A.huber;
            if (!TRIAL) {
                const double sx = w[12] * iz, sy = w[13] * iz;
                double rec[BaDim<NC>::kRec];
                rec[REC_R0] = r0, rec[REC_R1] = r1, rec[REC_W] = wt;
                // d r / d omega = (d r / d q) (-[q]x)
                rec[REC_JW + 0] = -(sx * (a * q1));
                rec[REC_JW + 1] = sx * (q2 + a * q0);
                rec[REC_JW + 2] = -(sx * q1);
                rec[REC_JW + 3] = -(sy * (q2 + b * q1));
                rec[REC_JW + 4] = sy * (b * q0);
                rec[REC_JW + 5] = sy * q0;
                // d r / d X = (d r / d q) R;  d r / d c is its negative
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    rec[REC_JP + i] = sx * (w[i] - a * w[6 + i]);
                    rec[REC_JP + 3 + i] = sy * (w[3 + i] - b * w[6 + i]);
                }
                if constexpr (NC == 7) {  // d r / d phi = (fx0 a, fy0 b)
                    rec[REC_JF] = A.foc[3 * (size_t)v] * a;
                    rec[REC_JF + 1] = A.foc[3 * (size_t)v + 1] * b;
                }
                const uint32_t k = A.cam_pos[o];
#pragma unroll
                for (int f = 0; f < BaDim<NC>::kRec; ++f) {
                    A.rec_t[f * N + o] = rec[f];
                    A.rec_c[f * N + k] = rec[f];
                }
            }
        } else {
            rho = std::numeric_limits<double>::infinity();
            atomicOr(A.nonpos, 1);  // every writer stores the same value
        }
        if (TRIAL) {
            const double* xc = A.x + NC * (size_t)v;
            const double* dq = A.dp + 3 * (size_t)t;
            const double d0 = dq[0] - xc[3], d1 = dq[1] - xc[4], d2 = dq[2] - xc[5];  // d r / d c = -d r / d X
            const double* R = A.rec_t;
            const double r0 = R[REC_R0 * N + o], r1 = R[REC_R1 * N + o], wt = R[REC_W * N + o];
            double l0 = (r0 + ((R[(REC_JW + 0) * N + o] * xc[0] + R[(REC_JW + 1) * N + o] * xc[1]) + R[(REC_JW + 2) * N + o] * xc[2])) +
                              ((R[(REC_JP + 0) * N + o] * d0 + R[(REC_JP + 1) * N + o] * d1) + R[(REC_JP + 2) * N + o] * d2);
            double l1 = (r1 + ((R[(REC_JW + 3) * N + o] * xc[0] + R[(REC_JW + 4) * N + o] * xc[1]) + R[(REC_JW + 5) * N + o] * xc[2])) +
                              ((R[(REC_JP + 3) * N + o] * d0 + R[(REC_JP + 4) * N + o] * d1) + R[(REC_JP + 5) * N + o] * d2);
            if constexpr (NC == 7) {
                l0 = l0 + R[REC_JF * N + o] * xc[6];
                l1 = l1 + R[(REC_JF + 1) * N + o] * xc[6];
            }
            pred = wt * ((r0 * r0 + r1 * r1) - (l0 * l0 + l1 * l1));
        }
    }
    const double c = block_tree_sum<kBaBlock>(rho, red, tid);
    if (tid == 0) A.part_cost[blockIdx.x] = c;
    if (TRIAL) {
        const double p = block_tree_sum<kBaBlock>(pred, red, tid);
        if (tid == 0) A.part_pred[blockIdx.x] = p;
    }
}
// out[i] = sum of n partials of array i (fixed order): one workgroup per array
__global__ __launch_bounds__(kBaBlock) void ba_reduce_kernel(const double* __restrict__ part, uint32_t n, uint32_t stride, double* __restrict__ out) {
    __shared__ double red[kBaBlock];
    const int tid = threadIdx.x;
    const double* p = part + (size_t)blockIdx.x * stride;
    double s = 0.0;
    for (uint32_t b = (uint32_t)tid; b < n; b += kBaBlock) s += p[b];
    s = block_tree_sum<kBaBlock>(s, red, tid);
    if (tid == 0) out[blockIdx.x] = s;
}

// ---- the point side ----------------------------------------------------------------------------------------------------
// V_j + lambda D_j, its inverse and s_j = V_j^-1 g_j; members in member order
__global__ __launch_bounds__(kBaBlock) void ba_point_setup_kernel(const uint32_t* __restrict__ obs_begin, uint32_t n_tracks, uint32_t n_obs,
                                                                  const double* __restrict__ rec, double lambda,
                                                                  double* __restrict__ Vinv, double* __restrict__ s_out) {
    const uint32_t t = blockIdx.x * kBaBlock + threadIdx.x;
    if (t >= n_tracks) return;
    const uint32_t ob = obs_begin[t], oe = obs_begin[t + 1];
    if (ob == oe) return;
    const size_t N = n_obs;
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    for (uint32_t o = ob; o < oe; ++o) {
        const double r0 = rec[REC_R0 * N + o], r1 = rec[REC_R1 * N + o], w = rec[REC_W * N + o];
        double ju[3], jv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) ju[i] = rec[(REC_JP + i) * N + o], jv[i] = rec[(REC_JP + 3 + i) * N + o];
        int n = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j, ++n) V[n] = V[n] + w * (ju[i] * ju[j] + jv[i] * jv[j]);
            g[i] = g[i] + w * (ju[i] * r0 + jv[i] * r1);
        }
    }
    const int diag[3] = {0, 3, 5};
#pragma unroll
    for (int i = 0; i < 3; ++i) V[diag[i]] = V[diag[i]] + lambda * fmin(fmax(V[diag[i]], kBaDiagMin), kBaDiagMax);
    double inv[6], s[3];
    ba_inv_sym3(V, inv);
    ba_mul_sym3(inv, g, s);
#pragma unroll
    for (int k = 0; k < 6; ++k) Vinv[6 * (size_t)t + k] = inv[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_out[3 * (size_t)t + k] = s[k];
}
// t_j = V_j^-1 sum_i W_ij^T p_i (the first half of the product), or with BACKSUB the point step -(s_j + t_j) for p = x
template <bool BACKSUB, int NC>
__global__ __launch_bounds__(kBaBlock) void ba_point_pass_kernel(const uint32_t* __restrict__ obs_begin, const uint32_t* __restrict__ obs_view,
                                                                 uint32_t n_tracks, uint32_t n_obs, const double* __restrict__ rec,
                                                                 const double* __restrict__ Vinv, const double* __restrict__ s_in,
                                                                 const double* __restrict__ p, double* __restrict__ out,
                                                                 const BaCgState* __restrict__ st) {
    if (!BACKSUB && st->done) return;  // (uniform)
    const uint32_t t = blockIdx.x * kBaBlock + threadIdx.x;
    if (t >= n_tracks) return;
    const uint32_t ob = obs_begin[t], oe = obs_begin[t + 1];
    if (ob == oe) return;
    const size_t N = n_obs;
    double u[3] = {0, 0, 0};
    for (uint32_t o = ob; o < oe; ++o) {
        const double* pc = p + NC * (size_t)obs_view[o];
        const double w = rec[REC_W * N + o];
        double ju[3], jv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) ju[i] = rec[(REC_JP + i) * N + o], jv[i] = rec[(REC_JP + 3 + i) * N + o];
        // y = J_cam p: the omega columns, and the centre columns = -d r / d X
        double y0 = ((rec[(REC_JW + 0) * N + o] * pc[0] + rec[(REC_JW + 1) * N + o] * pc[1]) + rec[(REC_JW + 2) * N + o] * pc[2]) -
                    ((ju[0] * pc[3] + ju[1] * pc[4]) + ju[2] * pc[5]);
        double y1 = ((rec[(REC_JW + 3) * N + o] * pc[0] + rec[(REC_JW + 4) * N + o] * pc[1]) + rec[(REC_JW + 5) * N + o] * pc[2]) -
                    ((jv[0] * pc[3] + jv[1] * pc[4]) + jv[2] * pc[5]);
        if constexpr (NC == 7) {  // the focal column
            y0 = y0 + rec[REC_JF * N + o] * pc[6];
            y1 = y1 + rec[(REC_JF + 1) * N + o] * pc[6];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) u[i] = u[i] + w * (ju[i] * y0 + jv[i] * y1);
    }
    double inv[6], tj[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) inv[k] = Vinv[6 * (size_t)t + k];
    ba_mul_sym3(inv, u, tj);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (size_t)t + k] = BACKSUB ? -(s_in[3 * (size_t)t + k] + tj[k]) : tj[k];
}

// ---- the camera side: one wavefront per camera -------------------------------------------------------------------------
struct BaCam {
    const uint32_t* cam_begin;  // n_views + 1
    const uint32_t* cam_pt;     // point of every position of the by-camera order
    const uint8_t* is_free;     // six parameters: 0 / 1;  seven: kBaPoseFree | kBaFocalFree
    const double* rec;          // records in camera order
    uint32_t n_views, n_obs;
    double lambda;
};
// The camera's diagonal block of S = U + lambda D - sum_j W V^-1 W^T, per observation J_c^T (w I - w^2 J_p V^-1 J_p^T) J_c;
// diag(U); the reduced right-hand side sum J_c^T w (J_p s_j - r).  Lane 0: Cholesky, then r = b, z = M^-1 r, x = p = 0.
// NC == 7: the sums run over all seven columns; lane 0 then clears the rows and columns of the pinned parameters (the pose
// of a view that is only focal-free, the focal of one that is only pose-free), which is the sum over zero columns: their
// block rows hold lambda D alone, their right-hand side and every PCG component stay exactly 0.
template <int NC>
__global__ __launch_bounds__(kBaBlock) void ba_cam_setup_kernel(BaCam A, const double* __restrict__ Vinv, const double* __restrict__ s_in,
                                                                double* __restrict__ chol, double* __restrict__ lamD,
                                                                double* __restrict__ x, double* __restrict__ r_out, double* __restrict__ z_out,
                                                                double* __restrict__ p, double* __restrict__ part_rz,
                                                                BaCgState* __restrict__ st) {
    const int lane = threadIdx.x & (kBaWave - 1);
    const uint32_t v = blockIdx.x * kBaCamsPerBlock + threadIdx.x / kBaWave;
    if (blockIdx.x == 0 && threadIdx.x == 0) *st = BaCgState{0.0, 0.0, 0u, 0};
    if (v >= A.n_views) return;  // (uniform in the wavefront)
    const size_t N = A.n_obs;
    constexpr int NT = BaDim<NC>::kTri;
    double S[NT], dU[NC], b[NC];
#pragma unroll
    for (int i = 0; i < NT; ++i) S[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NC; ++i) dU[i] = 0.0, b[i] = 0.0;
    const uint8_t flags = A.is_free[v];
    const bool is_free = flags != 0;
    if (is_free) {
        for (uint32_t k = A.cam_begin[v] + (uint32_t)lane; k < A.cam_begin[v + 1]; k += kBaWave) {
            const uint32_t j = A.cam_pt[k];
            const double r0 = A.rec[REC_R0 * N + k], r1 = A.rec[REC_R1 * N + k], w = A.rec[REC_W * N + k];
            double cu[NC], cv[NC], inv[6], mu[3], mv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                cu[i] = A.rec[(REC_JW + i) * N + k], cv[i] = A.rec[(REC_JW + 3 + i) * N + k];
                cu[3 + i] = -A.rec[(REC_JP + i) * N + k], cv[3 + i] = -A.rec[(REC_JP + 3 + i) * N + k];
            }
            if constexpr (NC == 7) cu[6] = A.rec[REC_JF * N + k], cv[6] = A.rec[(REC_JF + 1) * N + k];
#pragma unroll
            for (int i = 0; i < 6; ++i) inv[i] = Vinv[6 * (size_t)j + i];
            const double* sj = s_in + 3 * (size_t)j;
            const double pu[3] = {-cu[3], -cu[4], -cu[5]}, pv[3] = {-cv[3], -cv[4], -cv[5]};  // d r / d X
            ba_mul_sym3(inv, pu, mu);
            ba_mul_sym3(inv, pv, mv);
            const double a00 = (pu[0] * mu[0] + pu[1] * mu[1]) + pu[2] * mu[2];
            const double a01 = (pu[0] * mv[0] + pu[1] * mv[1]) + pu[2] * mv[2];
            const double a11 = (pv[0] * mv[0] + pv[1] * mv[1]) + pv[2] * mv[2];
            const double w2 = w * w;
            const double B00 = w - w2 * a00, B01 = -(w2 * a01), B11 = w - w2 * a11;
            const double y0 = w * (((pu[0] * sj[0] + pu[1] * sj[1]) + pu[2] * sj[2]) - r0);
            const double y1 = w * (((pv[0] * sj[0] + pv[1] * sj[1]) + pv[2] * sj[2]) - r1);
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const double hu = B00 * cu[i] + B01 * cv[i], hv = B01 * cu[i] + B11 * cv[i];
#pragma unroll
                for (int l = 0; l <= i; ++l) S[ba_tri(i, l)] = S[ba_tri(i, l)] + (hu * cu[l] + hv * cv[l]);
                dU[i] = dU[i] + w * (cu[i] * cu[i] + cv[i] * cv[i]);
                b[i] = b[i] + (cu[i] * y0 + cv[i] * y1);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) S[i] = wave_sum(S[i]);
#pragma unroll
    for (int i = 0; i < NC; ++i) dU[i] = wave_sum(dU[i]), b[i] = wave_sum(b[i]);
    if (lane != 0) return;
    double L[NT], z[NC], ld[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) z[i] = 0.0, ld[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) L[i] = 0.0;
    if constexpr (NC == 7) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const bool pin_i = !(flags & (i < 6 ? kBaPoseFree : kBaFocalFree));
            if (pin_i) dU[i] = 0.0, b[i] = 0.0;
#pragma unroll
            for (int l = 0; l <= i; ++l)
                if (pin_i || !(flags & (l < 6 ? kBaPoseFree : kBaFocalFree))) S[ba_tri(i, l)] = 0.0;
        }
    }
    if (is_free) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            ld[i] = A.lambda * fmin(fmax(dU[i], kBaDiagMin), kBaDiagMax);
            S[ba_tri(i, i)] = S[ba_tri(i, i)] + ld[i];
        }
        // Cholesky, row by row; the diagonal keeps the reciprocal pivot (0 where the pivot is not positive)
#pragma unroll
        for (int i = 0; i < NC; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double s = S[ba_tri(i, j)];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= L[ba_tri(i, k)] * L[ba_tri(j, k)];
                if (j < i) L[ba_tri(i, j)] = s * L[ba_tri(j, j)];
                else L[ba_tri(i, i)] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
            }
        }
        ba_chol_solve<NC>(L, b, z);
    }
    double rz = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) chol[NT * (size_t)v + i] = L[i];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const size_t n = NC * (size_t)v + i;
        lamD[n] = ld[i];
        x[n] = 0.0;
        p[n] = 0.0;
        r_out[n] = b[i];
        z_out[n] = z[i];
        rz += b[i] * z[i];
    }
    part_rz[v] = rz;
}
// q_i = U_i p_i + lambda D_i p_i - sum_j W_ij t_j = sum_obs w J_c^T (J_c p_i - J_p t_j) + lambda D_i p_i;  part_pq[i] = p_i . q_i
template <int NC>
__global__ __launch_bounds__(kBaBlock) void ba_cam_pass_kernel(BaCam A, const double* __restrict__ tvec, const double* __restrict__ lamD,
                                                               const double* __restrict__ p, double* __restrict__ q,
                                                               double* __restrict__ part_pq, const BaCgState* __restrict__ st) {
    if (st->done) return;  // (uniform)
    const int lane = threadIdx.x & (kBaWave - 1);
    const uint32_t v = blockIdx.x * kBaCamsPerBlock + threadIdx.x / kBaWave;
    if (v >= A.n_views) return;  // (uniform in the wavefront)
    const size_t N = A.n_obs;
    double acc[NC], pc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0, pc[i] = p[NC * (size_t)v + i];
    const uint8_t flags = A.is_free[v];
    if (flags) {
        for (uint32_t k = A.cam_begin[v] + (uint32_t)lane; k < A.cam_begin[v + 1]; k += kBaWave) {
            const double* tj = tvec + 3 * (size_t)A.cam_pt[k];
            const double w = A.rec[REC_W * N + k];
            double wu[3], wv[3], ju[3], jv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                wu[i] = A.rec[(REC_JW + i) * N + k], wv[i] = A.rec[(REC_JW + 3 + i) * N + k];
                ju[i] = A.rec[(REC_JP + i) * N + k], jv[i] = A.rec[(REC_JP + 3 + i) * N + k];
            }
            const double e0 = pc[3] + tj[0], e1 = pc[4] + tj[1], e2 = pc[5] + tj[2];  // J_c p - J_p t = J_w p_w - J_p (p_c + t)
            double y0, y1;
            if constexpr (NC == 7) {  // the focal column joins J_c p
                const double fu = A.rec[REC_JF * N + k], fv = A.rec[(REC_JF + 1) * N + k];
                y0 = w * ((((wu[0] * pc[0] + wu[1] * pc[1]) + wu[2] * pc[2]) - ((ju[0] * e0 + ju[1] * e1) + ju[2] * e2)) + fu * pc[6]);
                y1 = w * ((((wv[0] * pc[0] + wv[1] * pc[1]) + wv[2] * pc[2]) - ((jv[0] * e0 + jv[1] * e1) + jv[2] * e2)) + fv * pc[6]);
                acc[6] = acc[6] + (fu * y0 + fv * y1);
            } else {
                y0 = w * (((wu[0] * pc[0] + wu[1] * pc[1]) + wu[2] * pc[2]) - ((ju[0] * e0 + ju[1] * e1) + ju[2] * e2));
                y1 = w * (((wv[0] * pc[0] + wv[1] * pc[1]) + wv[2] * pc[2]) - ((jv[0] * e0 + jv[1] * e1) + jv[2] * e2));
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                acc[i] = acc[i] + (wu[i] * y0 + wv[i] * y1);
                acc[3 + i] = acc[3 + i] - (ju[i] * y0 + jv[i] * y1);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = wave_sum(acc[i]);
    if (lane != 0) return;
    double pq = 0.0;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        if constexpr (NC == 7) {  // a pinned parameter's column is zero: so is its row of the product
            if (!(flags & (i < 6 ? kBaPoseFree : kBaFocalFree))) acc[i] = 0.0;
        }
        const double qi = acc[i] + lamD[NC * (size_t)v + i] * pc[i];
        q[NC * (size_t)v + i] = qi;
        pq += pc[i] * qi;
    }
    part_pq[v] = pq;
}

// ---- PCG scalars: one view per lane of one-wavefront workgroups; every workgroup reduces the per-camera partials itself,
// in the same order, so all hold the same bits ----------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(kBaWave) void ba_cg_dir_kernel(uint32_t n_views, const double* __restrict__ z, double* __restrict__ p,
                                                            const double* __restrict__ part_rz, int first, double tol, uint32_t cap,
                                                            const BaCgState* __restrict__ st_prev, BaCgState* __restrict__ st_next) {
    const int lane = threadIdx.x;
    const BaCgState sp = *st_prev;
    if (sp.done) {  // (uniform) finished earlier: keep the record where the host reads it
        if (blockIdx.x == 0 && lane == 0) *st_next = sp;
        return;
    }
    const double rz = wave_sum(strided_sum<kBaWave>(part_rz, n_views, 1, lane));
    const double rz0 = first ? rz : sp.rz0;
    const double beta = (!first && sp.rz > 0.0) ? rz / sp.rz : 0.0;
    const bool done = !(rz > (tol * tol) * rz0) || sp.iters >= cap;
    if (blockIdx.x == 0 && lane == 0) *st_next = BaCgState{rz, rz0, done ? sp.iters : sp.iters + 1u, done ? 1 : 0};
    if (done) return;  // (uniform)
    const uint32_t v = blockIdx.x * kBaWave + (uint32_t)lane;
    if (v >= n_views) return;
#pragma unroll
    for (int i = 0; i < NC; ++i) p[NC * (size_t)v + i] = z[NC * (size_t)v + i] + beta * p[NC * (size_t)v + i];
}
template <int NC>
__global__ __launch_bounds__(kBaWave) void ba_cg_update_kernel(uint32_t n_views, const double* __restrict__ chol, const double* __restrict__ p,
                                                               const double* __restrict__ q, double* __restrict__ x, double* __restrict__ r,
                                                               double* __restrict__ z, const double* __restrict__ part_pq,
                                                               double* __restrict__ part_rz, const BaCgState* __restrict__ st) {
    const BaCgState s = *st;
    if (s.done) return;  // (uniform)
    const int lane = threadIdx.x;
    const double pq = wave_sum(strided_sum<kBaWave>(part_pq, n_views, 1, lane));
    const double alpha = pq > 0.0 ? s.rz / pq : 0.0;
    const uint32_t v = blockIdx.x * kBaWave + (uint32_t)lane;
    if (v >= n_views) return;
    constexpr int NT = BaDim<NC>::kTri;
    double L[NT], rn[NC], zn[NC];
#pragma unroll
    for (int i = 0; i < NT; ++i) L[i] = chol[NT * (size_t)v + i];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const size_t n = NC * (size_t)v + i;
        x[n] = x[n] + alpha * p[n];
        rn[i] = r[n] - alpha * q[n];
    }
    ba_chol_solve<NC>(L, rn, zn);
    double rz = 0.0;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        r[NC * (size_t)v + i] = rn[i];
        z[NC * (size_t)v + i] = zn[i];
        rz += rn[i] * zn[i];
    }
    part_rz[v] = rz;
}

// ---- the update: R <- exp([omega]x) R (Rodrigues as written in the specification), c += dc, X += dX; NC == 7: phi += dphi,
// fx = fx0 phi, fy = fy0 phi, and a view whose pose is pinned keeps its R and c untouched ------------------------------------
template <int NC>
__global__ __launch_bounds__(kBaBlock) void ba_apply_kernel(uint32_t n_views, const uint8_t* __restrict__ is_free, const double* __restrict__ x,
                                                            double* __restrict__ views, double* __restrict__ foc, uint32_t n_tracks,
                                                            const uint32_t* __restrict__ obs_begin, const double* __restrict__ dp,
                                                            double* __restrict__ X) {
    const uint32_t i = blockIdx.x * kBaBlock + threadIdx.x;
    if constexpr (NC == 7) {
        if (i < n_views && (is_free[i] & kBaFocalFree)) {
            double* f = foc + 3 * (size_t)i;
            const double phi = f[2] + x[NC * (size_t)i + 6];
            f[2] = phi;
            views[16 * (size_t)i + 12] = f[0] * phi;
            views[16 * (size_t)i + 13] = f[1] * phi;
        }
    }
    if (i < n_views && (NC == 7 ? (is_free[i] & kBaPoseFree) : is_free[i])) {
        const double* d = x + NC * (size_t)i;
        double* w = views + 16 * (size_t)i;
        const double w0 = d[0], w1 = d[1], w2 = d[2];
        const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
        double A, B;
        if (th2 < 1e-12) {
            A = 1.0 - th2 / 6.0;
            B = 0.5 - th2 / 24.0;
        } else {
            const double th = sqrt(th2);
            A = sin(th) / th;
            B = (1.0 - cos(th)) / th2;
        }
        // E = I + A [w]x + B [w]x^2
        double E[9];
        E[0] = 1.0 - B * (w1 * w1 + w2 * w2);
        E[1] = B * (w0 * w1) - A * w2;
        E[2] = B * (w0 * w2) + A * w1;
        E[3] = B * (w0 * w1) + A * w2;
        E[4] = 1.0 - B * (w0 * w0 + w2 * w2);
        E[5] = B * (w1 * w2) - A * w0;
        E[6] = B * (w0 * w2) - A * w1;
        E[7] = B * (w1 * w2) + A * w0;
        E[8] = 1.0 - B * (w0 * w0 + w1 * w1);
        double Rn[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) Rn[3 * a + b] = (E[3 * a] * w[b] + E[3 * a + 1] * w[3 + b]) + E[3 * a + 2] * w[6 + b];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[9 + k] = w[9 + k] + d[3 + k];
    }
    if (i < n_tracks && obs_begin[i] != obs_begin[i + 1]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) X[3 * (size_t)i + k] = X[3 * (size_t)i + k] + dp[3 * (size_t)i + k];
    }
}

size_t ba_align(size_t n) { return (n + 255) & ~(size_t)255; }

int ba_grow(void** p, size_t* have, size_t need, hipStream_t s, const char* who) {
    if (need <= *have) return PGI_SUCCESS;
    HIP_TRY(hipStreamSynchronize(s));  // kernels in flight may still use the old block
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) return fail(PGI_ERR_NOMEM, std::string(who) + ": device scratch: " + hipGetErrorString(e));
    *have = need;
    return PGI_SUCCESS;
}

int ba_validate(const char* who, const pgi_keypoint_view* h_views, const double* h_R, const double* h_c, const uint8_t* h_has_pose,
                uint32_t n_views, const pgi_bundle_params& prm) {
    if (!(prm.huber_px > 0.0)) return fail(PGI_ERR_INVALID, std::string(who) + ": huber_px must be positive");
    if (!(prm.cg_tol > 0.0) || !std::isfinite(prm.cg_tol)) return fail(PGI_ERR_INVALID, std::string(who) + ": cg_tol must be positive");
    if (!(prm.lambda_init > 0.0) || !std::isfinite(prm.lambda_init)) return fail(PGI_ERR_INVALID, std::string(who) + ": lambda_init must be positive");
    if (!(prm.ftol >= 0.0)) return fail(PGI_ERR_INVALID, std::string(who) + ": ftol must not be negative");
    if (n_views && (!h_views || !h_R || !h_c)) return fail(PGI_ERR_INVALID, std::string(who) + ": null view arrays");
    for (uint32_t v = 0; v < n_views; ++v) {
        if (h_has_pose && !h_has_pose[v]) continue;
        const pgi_keypoint_view& kv = h_views[v];
        if (kv.n && !kv.d_xy) return fail(PGI_ERR_INVALID, std::string(who) + ": view " + std::to_string(v) + " has keypoints but no array");
        if (!(kv.fx > 0.0) || !(kv.fy > 0.0) || !std::isfinite(kv.fx) || !std::isfinite(kv.fy))
            return fail(PGI_ERR_INVALID, std::string(who) + ": view " + std::to_string(v) + " has a non-positive or non-finite focal length");
        bool finite = std::isfinite(kv.cx) && std::isfinite(kv.cy);
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(h_R[(size_t)v * 9 + i]);
        for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(h_c[(size_t)v * 3 + i]);
        if (!finite) return fail(PGI_ERR_INVALID, std::string(who) + ": view " + std::to_string(v) + " has a non-finite pose or principal point");
    }
    return PGI_SUCCESS;
}

// the focal arguments of pgi_bundle_adjust_focal
struct BaFocal {
    double* h_focal;               // n_views, in-out
    const uint8_t* h_focal_fixed;  // n_views or NULL
    uint32_t min_focal_obs;
    uint32_t* n_free_focals;       // optional
};
int ba_validate_focal(const char* who, const BaFocal& F, const uint8_t* h_has_pose, uint32_t n_views) {
    if (!F.h_focal) return fail(PGI_ERR_INVALID, std::string(who) + ": null focal array");
    for (uint32_t v = 0; v < n_views; ++v) {
        if (h_has_pose && !h_has_pose[v]) continue;
        if (!(F.h_focal[v] > 0.0) || !std::isfinite(F.h_focal[v]))
            return fail(PGI_ERR_INVALID, std::string(who) + ": view " + std::to_string(v) + " has a non-positive or non-finite focal scale");
    }
    return PGI_SUCCESS;
}

// ctx->mu held.  focal == nullptr: pgi_bundle_adjust.  Otherwise fx, fy of the table are the views' times phi (one
// multiplication each), and the seven-parameter kernels run when at least one view ends up focal-free.
int ba_run(const char* who, pgi_ctx* ctx, const uint32_t* d_track_begin, const uint64_t* d_members, uint32_t n_tracks, bool members_known,
           uint64_t n_members, const pgi_keypoint_view* h_views, double* h_R, double* h_c, const uint8_t* h_has_pose, const uint8_t* h_fixed,
           uint32_t n_views, const pgi_bundle_params& prm, double* d_X, const uint8_t* d_status, const uint8_t* d_obs_state,
           pgi_bundle_report* report, const BaFocal* focal = nullptr) {
    pgi_bundle_report rep;
    memset(&rep, 0, sizeof rep);
    rep.stop_reason = PGI_BA_STOP_EMPTY;
    rep.lambda_final = prm.lambda_init;
    if (report) *report = rep;
    if (focal && focal->n_free_focals) *focal->n_free_focals = 0;
    if (!n_tracks || !n_views) return PGI_SUCCESS;
    if (!d_track_begin || !d_members || !d_X || !d_status || !d_obs_state) return fail(PGI_ERR_INVALID, std::string(who) + ": null argument");
    if (members_known && n_members > 0xfffffffeull) return fail(PGI_ERR_TOO_LARGE, std::string(who) + ": more than 2^32 - 2 members");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t T = n_tracks, V = n_views;
    const dim3 blk(kBaBlock);
    const dim3 grid_t1(((uint32_t)T + 1 + kBaBlock - 1) / kBaBlock), grid_t(((uint32_t)T + kBaBlock - 1) / kBaBlock);

    // ---- preparation, stage 1: the view table, the per-track counts and their scan
    size_t scan_b = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, T + 1, rocprim::plus<uint32_t>(), s));
    scan_b = ba_align(scan_b);
    const size_t p_views = 0, p_ptr = p_views + ba_align(V * 128), p_kpn = p_ptr + ba_align(V * 8), p_cnt = p_kpn + ba_align(V * 4),
                 p_begin = p_cnt + ba_align((T + 1) * 4), p_camcnt = p_begin + ba_align((T + 1) * 4), p_cambegin = p_camcnt + ba_align(V * 4),
                 p_free = p_cambegin + ba_align((V + 1) * 4), p_small = p_free + ba_align(V), p_scan = p_small + 256,
                 prep_total = p_scan + scan_b;
    if (int rc = ba_grow(&ctx->d_ba_prep, &ctx->ba_prep_bytes, prep_total, s, who)) return rc;
    char* pw = (char*)ctx->d_ba_prep;
    double* d_views = (double*)(pw + p_views);
    uint32_t* d_cnt = (uint32_t*)(pw + p_cnt);
    uint32_t* d_begin = (uint32_t*)(pw + p_begin);
    uint32_t* d_camcnt = (uint32_t*)(pw + p_camcnt);
    uint32_t* d_cambegin = (uint32_t*)(pw + p_cambegin);
    uint8_t* d_free = (uint8_t*)(pw + p_free);
    uint32_t* d_npts = (uint32_t*)(pw + p_small);
    int* d_nonpos = (int*)(pw + p_small + 8);
    double* d_sums = (double*)(pw + p_small + 16);                    // cost, predicted decrease
    BaCgState* d_st = (BaCgState*)(pw + p_small + 64);                // two records
    static_assert(64 + 2 * sizeof(BaCgState) <= 256, "small block");

    std::vector<double> h_tab(V * 16, 0.0);
    std::vector<const float*> h_ptr(V);
    std::vector<uint32_t> h_kpn(V);
    for (size_t v = 0; v < V; ++v) {
        const bool posed = !h_has_pose || h_has_pose[v];
        double* w = &h_tab[v * 16];
        if (posed) {
            for (int i = 0; i < 9; ++i) w[i] = h_R[v * 9 + i];
            for (int i = 0; i < 3; ++i) w[9 + i] = h_c[v * 3 + i];
            w[12] = h_views[v].fx, w[13] = h_views[v].fy, w[14] = h_views[v].cx, w[15] = h_views[v].cy;
            if (focal) w[12] = h_views[v].fx * focal->h_focal[v], w[13] = h_views[v].fy * focal->h_focal[v];
        }
        h_ptr[v] = h_views[v].d_xy;
        h_kpn[v] = posed ? h_views[v].n : 0u;
    }
    HIP_TRY(hipMemcpyAsync(d_views, h_tab.data(), V * 128, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pw + p_ptr, h_ptr.data(), V * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pw + p_kpn, h_kpn.data(), V * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(pw + p_small, 0, 256, s));
    HIP_TRY(hipMemsetAsync(d_camcnt, 0, V * 4, s));
    BaPrep P;
    P.track_begin = d_track_begin, P.members = d_members, P.obs_state = d_obs_state, P.status = d_status, P.X = d_X;
    P.kp_n = (const uint32_t*)(pw + p_kpn);
    P.n_tracks = n_tracks, P.n_views = n_views;
    P.member_cap = members_known ? (uint32_t)n_members : 0xffffffffu;
    P.use_low = prm.use_low_parallax ? 1u : 0u;
    hipLaunchKernelGGL(ba_count_kernel, grid_t1, blk, 0, s, P, d_cnt, d_npts);
    HIP_TRY(rocprim::exclusive_scan(pw + p_scan, scan_b, d_cnt, d_begin, 0u, T + 1, rocprim::plus<uint32_t>(), s));
    uint32_t n_obs = 0, n_pts = 0;
    HIP_TRY(hipMemcpyAsync(&n_obs, d_begin + T, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&n_pts, d_npts, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    rep.n_obs = n_obs, rep.n_points = n_pts;
    if (!n_obs) {
        if (report) *report = rep;
        return PGI_SUCCESS;
    }

    // ---- stage 2: the records in track order, the by-camera order, the workspace of the solve
    const size_t N = n_obs;
    uint32_t bits = 1;
    while (bits < 32 && (1ull << bits) < V) ++bits;
    size_t sort_b = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                      N, 0u, bits, s));
    sort_b = ba_align(sort_b);
    const uint32_t n_eval_blocks = (n_obs + kBaBlock - 1) / kBaBlock;
    // the workspace is laid out before the per-view counts are known: sized for seven parameters wherever a focal may be free
    bool focal_possible = false;
    for (size_t v = 0; focal && v < V; ++v)
        focal_possible = focal_possible || ((!h_has_pose || h_has_pose[v]) && !(focal->h_focal_fixed && focal->h_focal_fixed[v]));
    const size_t ws_nc = focal_possible ? 7 : 6, ws_tri = ws_nc * (ws_nc + 1) / 2, ws_rec = focal_possible ? BaDim<7>::kRec : BaDim<6>::kRec;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += ba_align(bytes);
        return o;
    };
    const size_t o_pt = carve(N * 4), o_view = carve(N * 4), o_idx = carve(N * 4), o_key2 = carve(N * 4), o_list = carve(N * 4),
                 o_pos = carve(N * 4), o_campt = carve(N * 4), o_pix = carve(N * 16), o_rect = carve(N * 8 * ws_rec),
                 o_recc = carve(N * 8 * ws_rec), o_Vinv = carve(T * 48), o_s = carve(T * 24), o_t = carve(T * 24), o_dp = carve(T * 24),
                 o_chol = carve(V * 8 * ws_tri), o_lamD = carve(V * 8 * ws_nc), o_x = carve(V * 8 * ws_nc), o_r = carve(V * 8 * ws_nc),
                 o_z = carve(V * 8 * ws_nc), o_p = carve(V * 8 * ws_nc), o_q = carve(V * 8 * ws_nc), o_prz = carve(V * 8), o_ppq = carve(V * 8),
                 o_part = carve((size_t)n_eval_blocks * 16), o_saveV = carve(V * 128), o_saveX = carve(T * 24), o_sort = carve(sort_b),
                 o_foc = carve(focal_possible ? V * 24 : 0), o_saveF = carve(focal_possible ? V * 24 : 0);
    if (int rc = ba_grow(&ctx->d_ba_ws, &ctx->ba_ws_bytes, off, s, who)) return rc;
    char* ws = (char*)ctx->d_ba_ws;
    uint32_t* d_pt = (uint32_t*)(ws + o_pt);
    uint32_t* d_view = (uint32_t*)(ws + o_view);
    uint32_t* d_list = (uint32_t*)(ws + o_list);
    uint32_t* d_pos = (uint32_t*)(ws + o_pos);
    uint32_t* d_campt = (uint32_t*)(ws + o_campt);
    double* d_rect = (double*)(ws + o_rect);
    double* d_recc = (double*)(ws + o_recc);
    double* d_Vinv = (double*)(ws + o_Vinv);
    double* d_s = (double*)(ws + o_s);
    double* d_t = (double*)(ws + o_t);
    double* d_dp = (double*)(ws + o_dp);
    double* d_x = (double*)(ws + o_x);
    double* d_p = (double*)(ws + o_p);
    double* d_q = (double*)(ws + o_q);
    double* d_part = (double*)(ws + o_part);
    const dim3 grid_o(n_eval_blocks), grid_cam(((uint32_t)V + kBaCamsPerBlock - 1) / kBaCamsPerBlock), grid_v(((uint32_t)V + kBaWave - 1) / kBaWave);
    hipLaunchKernelGGL(ba_fill_kernel, grid_t, blk, 0, s, P, (const uint32_t*)d_begin, (const float* const*)(pw + p_ptr), d_pt, d_view,
                       (uint32_t*)(ws + o_idx), (double*)(ws + o_pix), n_obs, d_camcnt);
    std::vector<uint32_t> cam_cnt(V), cam_begin(V + 1, 0);
    HIP_TRY(hipMemcpyAsync(cam_cnt.data(), d_camcnt, V * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    // free views and the gauge (V entries: host work)
    std::vector<uint8_t> is_free(V, 0);
    bool gauge_done = h_fixed != nullptr;
    for (size_t v = 0; v < V; ++v) {
        cam_begin[v + 1] = cam_begin[v] + cam_cnt[v];
        const bool posed = !h_has_pose || h_has_pose[v];
        if (!posed) continue;
        if (!gauge_done && cam_cnt[v]) {  // the smallest posed view with participating observations holds the gauge
            gauge_done = true;
            continue;
        }
        if (h_fixed && h_fixed[v]) continue;
        is_free[v] = cam_cnt[v] >= prm.min_cam_obs && cam_cnt[v] > 0;
        rep.n_free_cams += is_free[v];
    }
    // focal-free views: independent of the pose (the gauge view and a fixed view may have a free focal)
    uint32_t n_free_focals = 0;
    std::vector<uint8_t> flags(is_free);  // what the device reads: 0 / 1, or the two bits of the seven-parameter path
    std::vector<double> h_foc;
    if (focal) {
        const uint32_t need = std::max(focal->min_focal_obs, 1u);
        for (size_t v = 0; v < V; ++v) {
            const bool posed = !h_has_pose || h_has_pose[v];
            if (!posed || (focal->h_focal_fixed && focal->h_focal_fixed[v]) || cam_cnt[v] < need) continue;
            flags[v] |= kBaFocalFree;
            ++n_free_focals;
        }
        if (n_free_focals) {
            h_foc.assign(V * 3, 0.0);
            for (size_t v = 0; v < V; ++v) {
                const bool posed = !h_has_pose || h_has_pose[v];
                h_foc[3 * v] = posed ? h_views[v].fx : 0.0, h_foc[3 * v + 1] = posed ? h_views[v].fy : 0.0;
                h_foc[3 * v + 2] = posed ? focal->h_focal[v] : 1.0;
            }
            HIP_TRY(hipMemcpyAsync(ws + o_foc, h_foc.data(), V * 24, hipMemcpyHostToDevice, s));
        }
        if (focal->n_free_focals) *focal->n_free_focals = n_free_focals;
    }
    const bool seven = n_free_focals != 0;  // no focal-free view: the six-parameter kernels on the scaled table
    double* d_foc = seven ? (double*)(ws + o_foc) : nullptr;
    HIP_TRY(hipMemcpyAsync(d_cambegin, cam_begin.data(), (V + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_free, flags.data(), V, hipMemcpyHostToDevice, s));
    HIP_TRY(rocprim::radix_sort_pairs(ws + o_sort, sort_b, (const uint32_t*)d_view, (uint32_t*)(ws + o_key2), (const uint32_t*)(ws + o_idx), d_list,
                                      N, 0u, bits, s));
    hipLaunchKernelGGL(ba_invert_kernel, grid_o, blk, 0, s, (const uint32_t*)d_list, (const uint32_t*)d_pt, n_obs, d_pos, d_campt);

    BaEval E;
    E.obs_pt = d_pt, E.obs_view = d_view, E.cam_pos = d_pos, E.pix = (const double*)(ws + o_pix), E.views = d_views, E.X = d_X;
    E.rec_t = d_rect, E.rec_c = d_recc, E.x = d_x, E.dp = d_dp, E.part_cost = d_part, E.part_pred = d_part + n_eval_blocks;
    E.nonpos = d_nonpos, E.n_obs = n_obs, E.huber = prm.huber_px, E.foc = d_foc;
    BaCam Cm;
    Cm.cam_begin = d_cambegin, Cm.cam_pt = d_campt, Cm.is_free = d_free, Cm.rec = d_recc, Cm.n_views = n_views, Cm.n_obs = n_obs;
    struct Sums {
        double cost, pred;
        int nonpos;
    };
    // the Levenberg-Marquardt loop, once per camera block size
    auto solve = [&](auto nc_tag) -> int {
        constexpr int NC = decltype(nc_tag)::value;
        auto evaluate = [&](bool trial, Sums& out) -> int {
            HIP_TRY(hipMemsetAsync(d_nonpos, 0, 4, s));
            if (trial) hipLaunchKernelGGL((ba_eval_kernel<true, NC>), grid_o, blk, 0, s, E);
            else hipLaunchKernelGGL((ba_eval_kernel<false, NC>), grid_o, blk, 0, s, E);
            hipLaunchKernelGGL(ba_reduce_kernel, dim3(trial ? 2 : 1), blk, 0, s, (const double*)d_part, n_eval_blocks, n_eval_blocks, d_sums);
            double h[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(h, d_sums, 16, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(&out.nonpos, d_nonpos, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipGetLastError());
            out.cost = h[0], out.pred = h[1];
            return PGI_SUCCESS;
        };
        Sums cur{};
        if (int rc = evaluate(false, cur)) return rc;
        if (cur.nonpos) return fail(PGI_ERR_INVALID, std::string(who) + ": a participating observation has a non-positive depth at the start");
        rep.cost_initial = rep.cost_final = cur.cost;
        rep.stop_reason = PGI_BA_STOP_ITERS;
        const char* force_env = getenv("PGI_BUNDLE_FORCE_ACCEPT");  // read per call: step-exact tests only
        const bool force = force_env && atoi(force_env) != 0;
        const bool trace = getenv("PGI_BUNDLE_TRACE") != nullptr;  // one line per outer iteration on stderr
        double lambda = prm.lambda_init, cost = cur.cost;
        bool stale = false;  // the records belong to an earlier state
        uint32_t predicted = 0;
        for (uint32_t it = 0; it < prm.iters; ++it) {
            if (stale) {
                Sums again{};
                if (int rc = evaluate(false, again)) return rc;
                stale = false;
            }
            ++rep.iters;
            Cm.lambda = lambda;
            hipLaunchKernelGGL(ba_point_setup_kernel, grid_t, blk, 0, s, (const uint32_t*)d_begin, n_tracks, n_obs, (const double*)d_rect, lambda,
                               d_Vinv, d_s);
            hipLaunchKernelGGL(ba_cam_setup_kernel<NC>, grid_cam, blk, 0, s, Cm, (const double*)d_Vinv, (const double*)d_s, (double*)(ws + o_chol),
                               (double*)(ws + o_lamD), d_x, (double*)(ws + o_r), (double*)(ws + o_z), d_p, (double*)(ws + o_prz), d_st);
            // PCG: the host looks at the state record after a predicted number of iterations, then every kBaPoll
            uint32_t ci = 0;
            int par = 0;
            BaCgState hs{};
            const uint32_t cap = prm.cg_iters;
            for (;;) {
                const uint32_t target = std::min<uint32_t>(cap + 1, ci + (ci == 0 ? std::max<uint32_t>(kBaPoll, predicted + 2u) : kBaPoll));
                for (; ci < target; ++ci) {  // launch cap + 1 carries the stopping test alone
                    hipLaunchKernelGGL(ba_cg_dir_kernel<NC>, grid_v, dim3(kBaWave), 0, s, n_views, (const double*)(ws + o_z), d_p,
                                       (const double*)(ws + o_prz), ci == 0 ? 1 : 0, prm.cg_tol, cap, (const BaCgState*)(d_st + par), d_st + (par ^ 1));
                    par ^= 1;
                    hipLaunchKernelGGL((ba_point_pass_kernel<false, NC>), grid_t, blk, 0, s, (const uint32_t*)d_begin, (const uint32_t*)d_view, n_tracks,
                                       n_obs, (const double*)d_rect, (const double*)d_Vinv, (const double*)d_s, (const double*)d_p, d_t,
                                       (const BaCgState*)(d_st + par));
                    hipLaunchKernelGGL(ba_cam_pass_kernel<NC>, grid_cam, blk, 0, s, Cm, (const double*)d_t, (const double*)(ws + o_lamD),
                                       (const double*)d_p, d_q, (double*)(ws + o_ppq), (const BaCgState*)(d_st + par));
                    hipLaunchKernelGGL(ba_cg_update_kernel<NC>, grid_v, dim3(kBaWave), 0, s, n_views, (const double*)(ws + o_chol), (const double*)d_p,
                                       (const double*)d_q, d_x, (double*)(ws + o_r), (double*)(ws + o_z), (const double*)(ws + o_ppq),
                                       (double*)(ws + o_prz), (const BaCgState*)(d_st + par));
                }
                HIP_TRY(hipMemcpyAsync(&hs, d_st + par, sizeof hs, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                HIP_TRY(hipGetLastError());
                if (hs.done || ci > cap) break;
            }
            rep.cg_iters_total += hs.iters;
            predicted = hs.iters;
            // back-substitution, the saved copy, the update, the trial cost
            hipLaunchKernelGGL((ba_point_pass_kernel<true, NC>), grid_t, blk, 0, s, (const uint32_t*)d_begin, (const uint32_t*)d_view, n_tracks, n_obs,
                               (const double*)d_rect, (const double*)d_Vinv, (const double*)d_s, (const double*)d_x, d_dp,
                               (const BaCgState*)(d_st + par));
            HIP_TRY(hipMemcpyAsync(ws + o_saveV, d_views, V * 128, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(ws + o_saveX, d_X, T * 24, hipMemcpyDeviceToDevice, s));
            if (NC == 7) HIP_TRY(hipMemcpyAsync(ws + o_saveF, d_foc, V * 24, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(ba_apply_kernel<NC>, dim3(((uint32_t)std::max(T, V) + kBaBlock - 1) / kBaBlock), blk, 0, s, n_views,
                               (const uint8_t*)d_free, (const double*)d_x, d_views, d_foc, n_tracks, (const uint32_t*)d_begin, (const double*)d_dp, d_X);
            Sums tr{};
            if (int rc = evaluate(true, tr)) return rc;
            const double gain = (cost - tr.cost) / tr.pred;
            const bool accept = force || (!tr.nonpos && tr.pred > 0.0 && gain > kBaAcceptRatio);
            if (trace)
                std::fprintf(stderr, "[bundle] outer %2u: lambda %.1e, %3u PCG iterations, cost %.9g -> %.9g, gain %.3f, %s\n", it, lambda, hs.iters,
                             cost, tr.cost, gain, accept ? "accepted" : "rejected");
            if (accept) {
                const double rel = (cost - tr.cost) / cost;
                cost = tr.cost;
                ++rep.accepted;
                stale = true;
                lambda = std::max(lambda / 10.0, kBaLambdaMin);
                if (!force && !(rel >= prm.ftol)) {
                    rep.stop_reason = PGI_BA_STOP_FTOL;
                    break;
                }
            } else {
                HIP_TRY(hipMemcpyAsync(d_views, ws + o_saveV, V * 128, hipMemcpyDeviceToDevice, s));
                HIP_TRY(hipMemcpyAsync(d_X, ws + o_saveX, T * 24, hipMemcpyDeviceToDevice, s));
                if (NC == 7) HIP_TRY(hipMemcpyAsync(d_foc, ws + o_saveF, V * 24, hipMemcpyDeviceToDevice, s));
                lambda = lambda * 10.0;
                if (lambda > kBaLambdaMax) {
                    rep.stop_reason = PGI_BA_STOP_LAMBDA;
                    break;
                }
            }
        }
        rep.cost_final = cost;
        rep.lambda_final = lambda;
        return PGI_SUCCESS;
    };
    if (int rc = seven ? solve(std::integral_constant<int, 7>{}) : solve(std::integral_constant<int, 6>{})) return rc;
    if (rep.accepted) {
        HIP_TRY(hipMemcpyAsync(h_tab.data(), d_views, V * 128, hipMemcpyDeviceToHost, s));
        if (seven) HIP_TRY(hipMemcpyAsync(h_foc.data(), d_foc, V * 24, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t v = 0; v < V; ++v) {
            if (seven && (flags[v] & kBaFocalFree)) focal->h_focal[v] = h_foc[3 * v + 2];
            if (!is_free[v]) continue;
            for (int i = 0; i < 9; ++i) h_R[v * 9 + i] = h_tab[v * 16 + i];
            for (int i = 0; i < 3; ++i) h_c[v * 3 + i] = h_tab[v * 16 + 9 + i];
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (report) *report = rep;
    return PGI_SUCCESS;
}

// No C++ exception crosses the C ABI: the host tables of the focal entries are built behind this, with the mapping of the
// cycle filter's guard (pgi_cycle.hip).  pgi_bundle_adjust and pgi_tracklets_bundle_adjust are older than the guard and keep
// their statements as they were; putting them behind it is a change of its own.
template <class Body>
int ba_guarded(const char* who, Body body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(PGI_ERR_NOMEM, std::string(who) + ": out of host memory");
    } catch (const std::exception& e) {
        return fail(PGI_ERR_INVALID, std::string(who) + ": " + e.what());
    } catch (...) {
        return fail(PGI_ERR_INVALID, std::string(who) + ": unknown exception");
    }
}

}  // namespace
}  // namespace pgi

extern "C" {

void pgi_default_bundle_params(pgi_bundle_params* p) {
    if (!p) return;
    p->iters = 20;
    p->cg_iters = 200;
    p->min_cam_obs = 8;
    p->use_low_parallax = 0;
    p->huber_px = 4.0;
    p->cg_tol = 1e-6;
    p->ftol = 1e-9;
    p->lambda_init = 1e-4;
}

int pgi_bundle_adjust(pgi_ctx* ctx, const uint32_t* d_track_begin, const uint64_t* d_members, uint32_t n_tracks,
                      const pgi_keypoint_view* h_views, double* h_R, double* h_c, const uint8_t* h_has_pose, const uint8_t* h_fixed,
                      uint32_t n_views, const pgi_bundle_params* prm, double* d_X, const uint8_t* d_status, const uint8_t* d_obs_state,
                      pgi_bundle_report* report) {
    if (!ctx) return pgi::fail(PGI_ERR_INVALID, "pgi_bundle_adjust: null context");
    pgi_bundle_params p;
    if (prm) p = *prm; else pgi_default_bundle_params(&p);
    if (int rc = pgi::ba_validate("pgi_bundle_adjust", h_views, h_R, h_c, h_has_pose, n_views, p)) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    return pgi::ba_run("pgi_bundle_adjust", ctx, d_track_begin, d_members, n_tracks, false, 0, h_views, h_R, h_c, h_has_pose, h_fixed, n_views, p,
                       d_X, d_status, d_obs_state, report);
}

int pgi_tracklets_bundle_adjust(pgi_tracklets* trk, const pgi_keypoint_view* h_views, double* h_R, double* h_c, const uint8_t* h_has_pose,
                                const uint8_t* h_fixed, uint32_t n_views, const pgi_bundle_params* prm, double* d_X, const uint8_t* d_status,
                                const uint8_t* d_obs_state, pgi_bundle_report* report) {
    if (!trk) return pgi::fail(PGI_ERR_INVALID, "pgi_tracklets_bundle_adjust: null store");
    pgi_bundle_params p;
    if (prm) p = *prm; else pgi_default_bundle_params(&p);
    if (int rc = pgi::ba_validate("pgi_tracklets_bundle_adjust", h_views, h_R, h_c, h_has_pose, n_views, p)) return rc;
    pgi_ctx* ctx = nullptr;
    const uint32_t* d_begin = nullptr;
    const uint64_t* d_members = nullptr;
    uint32_t n_tracks = 0;
    uint64_t n_members = 0;
    pgi::tracklets_by_track(trk, &ctx, &d_begin, &d_members, &n_tracks, &n_members);
    std::lock_guard<std::mutex> lock(ctx->mu);
    return pgi::ba_run("pgi_tracklets_bundle_adjust", ctx, d_begin, d_members, n_tracks, true, n_members, h_views, h_R, h_c, h_has_pose, h_fixed,
                       n_views, p, d_X, d_status, d_obs_state, report);
}

int pgi_bundle_adjust_focal(pgi_ctx* ctx, const uint32_t* d_track_begin, const uint64_t* d_members, uint32_t n_tracks,
                            const pgi_keypoint_view* h_views, double* h_R, double* h_c, const uint8_t* h_has_pose, const uint8_t* h_fixed,
                            uint32_t n_views, const pgi_bundle_params* prm, double* d_X, const uint8_t* d_status, const uint8_t* d_obs_state,
                            double* h_focal, const uint8_t* h_focal_fixed, uint32_t min_focal_obs, pgi_bundle_report* report,
                            uint32_t* n_free_focals) {
    const char* who = "pgi_bundle_adjust_focal";
    if (!ctx) return pgi::fail(PGI_ERR_INVALID, std::string(who) + ": null context");
    return pgi::ba_guarded(who, [&]() -> int {
        pgi_bundle_params p;
        if (prm) p = *prm; else pgi_default_bundle_params(&p);
        const pgi::BaFocal F{h_focal, h_focal_fixed, min_focal_obs, n_free_focals};
        if (int rc = pgi::ba_validate(who, h_views, h_R, h_c, h_has_pose, n_views, p)) return rc;
        if (int rc = pgi::ba_validate_focal(who, F, h_has_pose, n_views)) return rc;
        std::lock_guard<std::mutex> lock(ctx->mu);
        return pgi::ba_run(who, ctx, d_track_begin, d_members, n_tracks, false, 0, h_views, h_R, h_c, h_has_pose, h_fixed, n_views, p, d_X, d_status,
                           d_obs_state, report, &F);
    });
}

int pgi_tracklets_bundle_adjust_focal(pgi_tracklets* trk, const pgi_keypoint_view* h_views, double* h_R, double* h_c, const uint8_t* h_has_pose,
                                      const uint8_t* h_fixed, uint32_t n_views, const pgi_bundle_params* prm, double* d_X, const uint8_t* d_status,
                                      const uint8_t* d_obs_state, double* h_focal, const uint8_t* h_focal_fixed, uint32_t min_focal_obs,
                                      pgi_bundle_report* report, uint32_t* n_free_focals) {
    const char* who = "pgi_tracklets_bundle_adjust_focal";
    if (!trk) return pgi::fail(PGI_ERR_INVALID, std::string(who) + ": null store");
    return pgi::ba_guarded(who, [&]() -> int {
        pgi_bundle_params p;
        if (prm) p = *prm; else pgi_default_bundle_params(&p);
        const pgi::BaFocal F{h_focal, h_focal_fixed, min_focal_obs, n_free_focals};
        if (int rc = pgi::ba_validate(who, h_views, h_R, h_c, h_has_pose, n_views, p)) return rc;
        if (int rc = pgi::ba_validate_focal(who, F, h_has_pose, n_views)) return rc;
        pgi_ctx* ctx = nullptr;
        const uint32_t* d_begin = nullptr;
        const uint64_t* d_members = nullptr;
        uint32_t n_tracks = 0;
        uint64_t n_members = 0;
        pgi::tracklets_by_track(trk, &ctx, &d_begin, &d_members, &n_tracks, &n_members);
        std::lock_guard<std::mutex> lock(ctx->mu);
        return pgi::ba_run(who, ctx, d_begin, d_members, n_tracks, true, n_members, h_views, h_R, h_c, h_has_pose, h_fixed, n_views, p, d_X, d_status,
                           d_obs_state, report, &F);
    });
}

}  // extern "C"
