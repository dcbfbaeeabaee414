// pgi_rotavg.hip -- rotation averaging (L1 + IRLS) on the pose graph.
//
// NOT in the reference: BASELINE.json:north_star adds it downstream of the
// per-edge estimator.  Algorithm: Chatterjee & Govindu (ICCV'13 / TPAMI'18), specified in
// oracle/rotavg_oracle.py and DESIGN.md §3.7.  Edge convention of the reference
// (pose.h:14, graph_traversal.h:340-344): R_rel ~ R_dst R_src^T, world->camera R_k.
//
// Data path: the problem is MB-scale (V <= ~1e4 views) and latency-bound, so it is solved by
//   rot_residual_kernel  one thread per edge   : omega = log(R_dst^T R_rel R_src), robust weight
//   rot_solve_kernel     V <= 64: ONE 1024-thread workgroup, a single launch : weighted-Laplacian normal
//                        equations assembled per vertex from a CSR adjacency (fixed order), Jacobi-
//                        preconditioned CG on the three axes at once; fixed-tree block reductions
//   cg_*_kernel          larger graphs: the same recurrences across all CUs, ONE launch per iteration (16 lanes per
//                        view), CG scalars and the convergence flag resident on the device, the host looks after a
//                        predicted number of launches; deterministic
//   rot_solve_tree_kernel  sparse, sequence-like graphs (E <= 8 V): spanning-tree preconditioner, on chip
//   cg_*_kernel<true>,   dense band-like graphs (deep breadth-first walk): two-level preconditioner, Jacobi + a coarse
//   cg2_coarse_*_kernel  space of <= 127 aggregates of neighbouring views, coarse matrix inverted on the device per step
//   rot_update_kernel    one thread per view   : R_k <- R_k exp(d_k)
// Every floating-point sum goes through pgi_reduce.hpp (one documented association each); the host-side graph preparation
// (incidence CSR, spanning forest, tree order, aggregates) is pgi_graph_host.hpp.
// Multi-GPU: "replicas only" -- after the all-gather of the edge records every rank (or rank 0)
// runs this identical solve; an edge-partitioned CG would pay an all-reduce per iteration for a
// 3V-vector and is pure latency.
#include "pgi_internal.hpp"
#include "pgi_graph_host.hpp"
#include "pgi_reduce.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <numeric>
#include <type_traits>
#include <vector>

namespace pgi {
// Inner solves of the rotation averaging stop at |r|_M <= 1e-4 |r0|_M (round 5; 1e-10 before).  The outer IRLS loop is a fixed-point
// iteration whose steps shrink 3-5x each, and the preconditioned systems have an effective condition of ~40 (75 iterations for ten
// orders of magnitude), so a relative residual of 1e-4 leaves ~6e-4 of a step as error -- two orders below the next step.  Measured
// (scripts/rotavg_bench.py + soak_rotavg.py, 120 random graphs x 2 solver settings): 1e-10 / 1e-6 / 1e-4 / 1e-3 -> V = 5000: 12.2 / 11.0 /
// 9.2 / 8.0 ms, band graph (config 4's shape) 19.7 / 14.6 / 12.1 / 11.1 ms; outer iteration counts and the worst difference from the
// oracle's direct solves (3.4e-7 rad) are THE SAME down to 1e-4; at 1e-3 the first iteration counts move by one.
constexpr double kInnerTolerance = 1e-4;


#define RDEV __device__ __forceinline__
constexpr uint32_t kSingleWgViews = 64;  // at or below (16 lanes per view in one pass): one-workgroup PCG in a single launch

RDEV void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
RDEV void mat3_tmul(const double* A, const double* B, double* C) {  // A^T B
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}

// log map through the unit quaternion (Shepperd's branch selection): robust up to pi
RDEV void so3_log(const double* R, double* w) {
    const double tr = R[0] + R[4] + R[8];
    double q0, q1, q2, q3;  // w, x, y, z
    if (tr > 0.0) {
        const double s = sqrt(tr + 1.0) * 2.0;
        q0 = 0.25 * s; q1 = (R[7] - R[5]) / s; q2 = (R[2] - R[6]) / s; q3 = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
        q0 = (R[7] - R[5]) / s; q1 = 0.25 * s; q2 = (R[1] + R[3]) / s; q3 = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
        q0 = (R[2] - R[6]) / s; q1 = (R[1] + R[3]) / s; q2 = 0.25 * s; q3 = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
        q0 = (R[3] - R[1]) / s; q1 = (R[2] + R[6]) / s; q2 = (R[5] + R[7]) / s; q3 = 0.25 * s;
    }
    if (q0 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
    const double nv = sqrt(q1 * q1 + q2 * q2 + q3 * q3);
    const double k = (nv < 1e-12) ? 2.0 : 2.0 * atan2(nv, q0) / nv;
    w[0] = k * q1; w[1] = k * q2; w[2] = k * q3;
}

RDEV void so3_exp(const double* w, double* R) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double t = sqrt(t2);
    double a, b;  // sin t / t, (1 - cos t) / t^2
    if (t < 1e-6) {
        a = 1.0 - t2 / 6.0;
        b = 0.5 - t2 / 24.0;
    } else {
        a = sin(t) / t;
        b = (1.0 - cos(t)) / t2;
    }
    const double x = w[0], y = w[1], z = w[2];
    R[0] = 1.0 - b * (y * y + z * z); R[1] = -a * z + b * x * y;        R[2] = a * y + b * x * z;
    R[3] = a * z + b * x * y;         R[4] = 1.0 - b * (x * x + z * z); R[5] = -a * x + b * y * z;
    R[6] = -a * y + b * x * z;        R[7] = a * x + b * y * z;         R[8] = 1.0 - b * (x * x + y * y);
}

struct RotEdgeDev {
    uint32_t src, dst;
    double R[9];
    double weight;
};

__global__ __launch_bounds__(256) void rot_residual_kernel(const RotEdgeDev* __restrict__ edges, uint32_t n_edges,
                                                           const double* __restrict__ R, int l1_phase, double sigma,
                                                           double* __restrict__ omega, double* __restrict__ w) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const RotEdgeDev ed = edges[e];
    double Ri[9], Rj[9], T[9], D[9], om[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        Ri[c] = R[9 * (size_t)ed.src + c];
        Rj[c] = R[9 * (size_t)ed.dst + c];
    }
    mat3_mul(ed.R, Ri, T);   // R_rel R_src
    mat3_tmul(Rj, T, D);     // R_dst^T R_rel R_src
    so3_log(D, om);
    const double n2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double wt;
    if (l1_phase) {
        wt = ed.weight / fmax(sqrt(n2), 1e-4);
    } else {
        const double s2 = sigma * sigma, d = n2 + s2;
        wt = ed.weight * s2 / (d * d) * s2;
    }
    omega[3 * (size_t)e + 0] = om[0];
    omega[3 * (size_t)e + 1] = om[1];
    omega[3 * (size_t)e + 2] = om[2];
    w[e] = wt;
}

// adj_ptr[V+1]; adj_edge / adj_other / adj_sign per incidence (sign +1: the vertex is dst, -1: src)
__global__ __launch_bounds__(1024) void rot_solve_kernel(uint32_t n_views, const uint32_t* __restrict__ adj_ptr,
                                                         const uint32_t* __restrict__ adj_edge,
                                                         const uint32_t* __restrict__ adj_other,
                                                         const int8_t* __restrict__ adj_sign,
                                                         const uint8_t* __restrict__ is_root,
                                                         const double* __restrict__ omega, const double* __restrict__ w,
                                                         uint32_t cg_iters, double cg_tol, uint32_t row_lanes, double* __restrict__ diag,
                                                         double* __restrict__ x, double* __restrict__ r,
                                                         double* __restrict__ p, double* __restrict__ Ap,
                                                         double* __restrict__ stats /* mean|d|, cg iterations */) {
    __shared__ double red[3 * 1024];
    const int tid = threadIdx.x;
    // assemble: diag_k = sum w_e ; b_k = sum sign * w_e * omega_e ; x = 0, r = b, z = r / diag, p = z
    double rz[3] = {0, 0, 0};
    for (uint32_t k = tid; k < n_views; k += 1024) {
        double d = 0, b[3] = {0, 0, 0};
        if (!is_root[k]) {
            for (uint32_t a = adj_ptr[k]; a < adj_ptr[k + 1]; ++a) {
                const uint32_t e = adj_edge[a];
                const double we = w[e], sg = (double)adj_sign[a];
                d += we;
                b[0] += sg * we * omega[3 * (size_t)e + 0];
                b[1] += sg * we * omega[3 * (size_t)e + 1];
                b[2] += sg * we * omega[3 * (size_t)e + 2];
            }
        }
        diag[k] = d;
        const double inv = d > 0.0 ? 1.0 / d : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[3 * (size_t)k + c] = 0.0;
            r[3 * (size_t)k + c] = b[c];
            const double z = b[c] * inv;
            p[3 * (size_t)k + c] = z;
            rz[c] += b[c] * z;
        }
    }
    block_tree_sum<3, 1024>(rz, red, tid);
    const double rz0[3] = {rz[0], rz[1], rz[2]};
    uint32_t it = 0;
    for (; it < cg_iters; ++it) {
        bool done = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) done &= !(rz[c] > cg_tol * cg_tol * rz0[c]);
        if (done) break;  // uniform: rz is identical in every thread
        double pAp[3] = {0, 0, 0};
        // `row_lanes` lanes share a view (its incidences strided over them, partial rows combined by a fixed xor tree):
        // one thread per view walks tens of neighbours as a chain of dependent gathers, the whole cost of the product
        const uint32_t sub = (uint32_t)tid & (row_lanes - 1u), per_pass = 1024u / row_lanes;
        for (uint32_t k0 = 0; k0 < n_views; k0 += per_pass) {  // uniform trip count: the shuffles below need every lane
            const uint32_t k = k0 + (uint32_t)tid / row_lanes;
            const bool live = k < n_views, free_k = live && !is_root[k];
            double y[3] = {0, 0, 0};
            if (free_k)
                for (uint32_t a = adj_ptr[k] + sub; a < adj_ptr[k + 1]; a += row_lanes) {
                    const uint32_t o = adj_other[a];
                    if (is_root[o]) continue;
                    const double we = w[adj_edge[a]];
#pragma unroll
                    for (int c = 0; c < 3; ++c) y[c] -= we * p[3 * (size_t)o + c];
                }
            row_lanes_sum<3>(y, row_lanes);
            if (live && sub == 0u) {
                const double d = diag[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double pk = p[3 * (size_t)k + c], yc = free_k ? d * pk + y[c] : 0.0;
                    Ap[3 * (size_t)k + c] = yc;
                    pAp[c] += pk * yc;
                }
            }
        }
        block_tree_sum<3, 1024>(pAp, red, tid);
        double alpha[3], rzn[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; ++c) alpha[c] = pAp[c] > 0.0 ? rz[c] / pAp[c] : 0.0;
        for (uint32_t k = tid; k < n_views; k += 1024) {
            const double d = diag[k], inv = d > 0.0 ? 1.0 / d : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t i = 3 * (size_t)k + c;
                x[i] += alpha[c] * p[i];
                const double rn = r[i] - alpha[c] * Ap[i];
                r[i] = rn;
                rzn[c] += rn * (rn * inv);
            }
        }
        block_tree_sum<3, 1024>(rzn, red, tid);
        for (uint32_t k = tid; k < n_views; k += 1024) {
            const double d = diag[k], inv = d > 0.0 ? 1.0 / d : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t i = 3 * (size_t)k + c;
                const double beta = rz[c] > 0.0 ? rzn[c] / rz[c] : 0.0;
                p[i] = r[i] * inv + beta * p[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) rz[c] = rzn[c];
    }
    double nd[3] = {0, 0, 0};
    for (uint32_t k = tid; k < n_views; k += 1024)
        nd[0] += sqrt(x[3 * (size_t)k] * x[3 * (size_t)k] + x[3 * (size_t)k + 1] * x[3 * (size_t)k + 1] +
                      x[3 * (size_t)k + 2] * x[3 * (size_t)k + 2]);
    block_tree_sum<3, 1024>(nd, red, tid);
    if (tid == 0) {
        stats[0] = nd[0] / (double)n_views;
        stats[1] = (double)it;
    }
}

// ---- on-chip PCG with a spanning-tree preconditioner (sparse / sequence-like view graphs, up to kTreeViews views) ------
// Jacobi-preconditioned CG needs thousands of iterations on path-like view graphs (image sequences: kappa ~ (V / degree)^2;
// 2 100 iterations per solve on the config-4 surrogate) where the Laplacian of the maximum-weight spanning forest -- the
// one the initialisation already built -- as preconditioner needs ~100 (and is useless on dense graphs: 1 400 against
// Jacobi's 19), so the host switches to this kernel when the Jacobi solve runs into its iteration cap.
// A tree system L_T z = r is solved EXACTLY by two prefix sums (no elimination order, no level-by-level sweep -- the
// forest of the surrogate is 1 800 levels deep): with the views numbered in depth-first preorder a subtree is a
// contiguous range, so the flow towards the root on the edge above view k is f_k = S[k + size_k - 1] - S[k - 1]
// (S = prefix sums of r), and z_k = sum over the ancestors-or-self u of f_u / w_u is a prefix sum over the Euler tour
// with +g_u at u's entry and -g_u at its exit.  One workgroup per component of the (Laplacian x I3) system keeps its
// vectors in registers (thread t owns views [t m, t m + m)), the scans and the gathered vector live in LDS; an iteration
// is a dozen workgroup barriers.  Scans run in a fixed order: same input, same bits.
constexpr uint32_t kTreeViews = 6144;
constexpr int kTreeOwn = kTreeViews / 1024;

struct TreeIncidence {  // one 16-byte load per incidence in the products
    double w;
    uint32_t other, pad;
};
// grid = 3 (component), block = 1024.  Views are in depth-first preorder ("new" numbering); new_to_old maps back.
__global__ __launch_bounds__(1024) void rot_solve_tree_kernel(uint32_t n_views, uint32_t m /* views per thread */,
                                                              const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj_edge,
                                                              const uint32_t* __restrict__ adj_other, const int8_t* __restrict__ adj_sign,
                                                              const uint32_t* __restrict__ parent_edge /* 0xFFFFFFFF: root */,
                                                              const uint32_t* __restrict__ sub_size, const uint32_t* __restrict__ tour_enter,
                                                              const uint32_t* __restrict__ tour_exit, const uint32_t* __restrict__ new_to_old,
                                                              const double* __restrict__ omega, const double* __restrict__ w,
                                                              uint32_t cg_iters, double cg_tol, TreeIncidence* __restrict__ inc,
                                                              double* __restrict__ x_out, double* __restrict__ iters_out) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const uint32_t comp = blockIdx.x, vpad = 1024u * m;
    double* tour = lds;          // 2 * vpad: prefix sums (first of r over the preorder, then over the Euler tour)
    double* pvec = lds;          // vpad: the vector being gathered by the products (the scans are idle then)
    double* xvec = tour + 2 * (size_t)vpad;  // vpad: the solution (kept out of the register file)
    double* red = xvec + vpad;   // 16
    const uint32_t k0 = (uint32_t)tid * m;

    double d[kTreeOwn], winv[kTreeOwn], r[kTreeOwn], p[kTreeOwn], q[kTreeOwn], z[kTreeOwn];
    uint32_t sz[kTreeOwn], ten[kTreeOwn], tex[kTreeOwn];
    bool fr[kTreeOwn];
#pragma unroll
    for (int j = 0; j < kTreeOwn; ++j) {
        d[j] = 0.0; winv[j] = 0.0; r[j] = 0.0; p[j] = 0.0; q[j] = 0.0; z[j] = 0.0;
        sz[j] = 1; ten[j] = 0; tex[j] = 0; fr[j] = false;
        const uint32_t k = k0 + (uint32_t)j;
        if ((uint32_t)j < m) xvec[k] = 0.0;  // only its owner ever touches an entry
        if ((uint32_t)j >= m || k >= n_views) continue;
        sz[j] = sub_size[k]; ten[j] = tour_enter[k]; tex[j] = tour_exit[k];
        const uint32_t pe = parent_edge[k];
        fr[j] = pe != 0xFFFFFFFFu;
        if (!fr[j]) continue;
        const double wp = w[pe];
        winv[j] = wp > 0.0 ? 1.0 / wp : 0.0;
        double dd = 0.0, bb = 0.0;
        for (uint32_t t = adj_ptr[k]; t < adj_ptr[k + 1]; ++t) {
            const uint32_t e = adj_edge[t];
            const double we = w[e];
            inc[t] = TreeIncidence{we, adj_other[t], 0u};  // read back by this same thread only (the three workgroups write the same values)
            dd += we;
            bb += (double)adj_sign[t] * we * omega[3 * (size_t)e + comp];
        }
        d[j] = dd;
        r[j] = bb;
    }
    // z = L_T^-1 r
    auto precondition = [&]() {
        // prefix sums of r over the preorder
        double run = 0.0, loc[kTreeOwn];
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) { run += ((uint32_t)j < m) ? r[j] : 0.0; loc[j] = run; }
        const double before = block_prefix_1024(run, red, tid);
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j)
            if ((uint32_t)j < m) tour[k0 + (uint32_t)j] = before + loc[j];
        __syncthreads();
        double g[kTreeOwn];
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) {
            g[j] = 0.0;
            const uint32_t k = k0 + (uint32_t)j;
            if ((uint32_t)j >= m || !fr[j]) continue;
            const double f = tour[k + sz[j] - 1u] - (k ? tour[k - 1u] : 0.0);  // what the subtree of k sends to its parent
            g[j] = f * winv[j];
        }
        __syncthreads();
        // Euler tour: +g at the entry of a view, -g at its exit (every position of the tour is written exactly once)
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) {
            const uint32_t k = k0 + (uint32_t)j;
            if ((uint32_t)j >= m || k >= n_views) continue;
            tour[ten[j]] = g[j];
            tour[tex[j]] = -g[j];
        }
        __syncthreads();
        // inclusive prefix sums over the tour: thread t owns positions [2 t m, 2 t m + 2 m)
        const uint32_t t0 = 2u * k0, tn = 2u * n_views;
        double trun = 0.0;
        for (uint32_t i = 0; i < 2u * m; ++i) trun += (t0 + i < tn) ? tour[t0 + i] : 0.0;
        const double tbefore = block_prefix_1024(trun, red, tid);
        trun = tbefore;
        for (uint32_t i = 0; i < 2u * m; ++i)
            if (t0 + i < tn) { trun += tour[t0 + i]; tour[t0 + i] = trun; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) z[j] = ((uint32_t)j < m && fr[j]) ? tour[ten[j]] : 0.0;
        __syncthreads();  // tour is rewritten by the next call
    };
    precondition();
    double rz = 0.0;
#pragma unroll
    for (int j = 0; j < kTreeOwn; ++j) { p[j] = z[j]; rz += r[j] * z[j]; }
    rz = block_wave_sum_1024(rz, red, tid);
    const double rz0 = rz;
    uint32_t it = 0;
    for (; it < cg_iters; ++it) {
        if (!(rz > cg_tol * cg_tol * rz0)) break;  // uniform: rz is identical in every thread
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j)
            if ((uint32_t)j < m) pvec[k0 + (uint32_t)j] = p[j];
        __syncthreads();
        double pAp = 0.0;
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) {
            const uint32_t k = k0 + (uint32_t)j;
            double y = 0.0;
            if ((uint32_t)j < m && fr[j]) {
                y = d[j] * p[j];
                uint32_t t = adj_ptr[k];
                const uint32_t te = adj_ptr[k + 1];
                for (; t + 4 <= te; t += 4) {  // four independent loads in flight (roots hold p = 0)
                    const TreeIncidence a0 = inc[t], a1 = inc[t + 1], a2 = inc[t + 2], a3 = inc[t + 3];
                    y -= a0.w * pvec[a0.other];
                    y -= a1.w * pvec[a1.other];
                    y -= a2.w * pvec[a2.other];
                    y -= a3.w * pvec[a3.other];
                }
                for (; t < te; ++t) {
                    const TreeIncidence a0 = inc[t];
                    y -= a0.w * pvec[a0.other];
                }
            }
            q[j] = y;
            pAp += p[j] * y;
        }
        pAp = block_wave_sum_1024(pAp, red, tid);
        const double alpha = pAp > 0.0 ? rz / pAp : 0.0;
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) {
            if ((uint32_t)j < m) xvec[k0 + (uint32_t)j] += alpha * p[j];
            r[j] -= alpha * q[j];
        }
        precondition();
        double rzn = 0.0;
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) rzn += r[j] * z[j];
        rzn = block_wave_sum_1024(rzn, red, tid);
        const double beta = rz > 0.0 ? rzn / rz : 0.0;
#pragma unroll
        for (int j = 0; j < kTreeOwn; ++j) p[j] = z[j] + beta * p[j];
        rz = rzn;
    }
#pragma unroll
    for (int j = 0; j < kTreeOwn; ++j) {
        const uint32_t k = k0 + (uint32_t)j;
        if ((uint32_t)j < m && k < n_views) x_out[3 * (size_t)new_to_old[k] + comp] = xvec[k];
    }
    if (tid == 0) iters_out[comp] = (double)it;
}

// ---- multi-workgroup PCG (large graphs): scalars (gamma, alpha, beta, done) resident on the device; block partials
// are reduced in a fixed order.
struct CgState {
    double rz[3], rz0[3], alpha[3], beta[3];
    double mean_step, iters;
    int done;
    unsigned int ticket;  // workgroups that have delivered their partial sums (fused kernels)
};
constexpr int kCgBlock = 256;

constexpr int kRowLanes = 16;
constexpr int kRowsPerBlock = kCgBlock / kRowLanes;
constexpr uint32_t kMaxAggregates = 128;  // of the two-level preconditioner (below); ids stay below kNoAggregate

// What the two-level kernels take on top of the one-level ones (see "two-level PCG" below).  cs_*: rho | kappa | c, 3 n_agg
// each, by launch parity.
struct CoarseLevel {
    uint32_t n_agg;
    const uint8_t* adj_agg;       // per incidence: the aggregate of its other end (kNoAggregate: a gauge view)
    const uint32_t* agg_block;    // n_agg + 1 block starts
    const uint8_t* agg_of_block;
    const double* Ainv;
    const double* rpart;          // block sums of r0 (the init kernel's)
    const double* cs_prev;
    double* cs_next;
};
struct NoCoarseLevel {};
template <bool TWO_LEVEL>
using CoarseArgs = std::conditional_t<TWO_LEVEL, CoarseLevel, NoCoarseLevel>;

// assemble diag / rhs (kRowLanes lanes share a view's incidences: one thread walking the tens of incidences of a dense scene
// graph's view took 47 us per outer step), x = 0, r = b, q0 = s0 = 0, the PCG state records cleared.  One level: p = z = r /
// diag.  Two levels (rows in place of views): p = 0 and the block sums of r (-> rho0 = P^T r0) in rpart.
template <bool TWO_LEVEL>
__global__ __launch_bounds__(kCgBlock) void cg_init_kernel(uint32_t n_views, const uint32_t* __restrict__ adj_ptr,
                                                           const uint32_t* __restrict__ adj_edge,
                                                           const int8_t* __restrict__ adj_sign,
                                                           const uint8_t* __restrict__ is_root,
                                                           const double* __restrict__ omega, const double* __restrict__ w,
                                                           double* __restrict__ diag, double* __restrict__ x,
                                                           double* __restrict__ r, double* __restrict__ p, double* __restrict__ rpart,
                                                           double* __restrict__ q0, double* __restrict__ s0,
                                                           CgState* __restrict__ states) {
    const int tid = threadIdx.x, sub = tid & (kRowLanes - 1);
    const uint32_t k = blockIdx.x * kRowsPerBlock + (uint32_t)(tid / kRowLanes);
    if (blockIdx.x == 0 && tid < 3) states[tid] = CgState{};  // the two launch parities and the record the host reads
    double d = 0, b[3] = {0, 0, 0};
    if (k < n_views && !is_root[k])
        for (uint32_t a = adj_ptr[k] + (uint32_t)sub; a < adj_ptr[k + 1]; a += kRowLanes) {
            const uint32_t e = adj_edge[a];
            const double we = w[e], sg = (double)adj_sign[a];
            d += we;
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c] += sg * we * omega[3 * (size_t)e + c];
        }
    row_lanes_sum<1, kRowLanes>(&d);
    row_lanes_sum<3, kRowLanes>(b);
    double rs[3] = {0, 0, 0};
    if (k < n_views && sub == 0) {
        diag[k] = d;
        const double inv = d > 0.0 ? 1.0 / d : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t i = 3 * (size_t)k + c;
            x[i] = 0.0;
            r[i] = b[c];
            p[i] = TWO_LEVEL ? 0.0 : b[c] * inv;
            q0[i] = s0[i] = 0.0;
            rs[c] = b[c];
        }
    }
    if constexpr (TWO_LEVEL) {
        __shared__ double red[3 * kCgBlock];
        block_tree_sum<3, kCgBlock>(rs, red, tid);
        if (tid == 0)
            for (int c = 0; c < 3; ++c) rpart[3 * (size_t)blockIdx.x + c] = rs[c];
    }
}

// ---- ONE launch per PCG iteration.  The solve is bound by the ~13 us between small dependent kernels and by the depth
// of the gather chains inside them, not by arithmetic, so the iteration is arranged around a single grid-wide
// synchronisation point (the kernel boundary):
//   * Chronopoulos-Gear form of preconditioned CG: with s = A z kept next to q = A p, both inner products of an
//     iteration (gamma = r.z, delta = z.s) belong to the same vectors and are reduced together;
//       beta = gamma' / gamma,  alpha' = gamma' / (delta' - beta gamma' / alpha),
//       p = z + beta p,  q = s + beta q,  x += alpha p,  r -= alpha q,  z = r / diag,  s = A z
//   * a thread rebuilds the z entries it gathers from the PREVIOUS iteration's vectors,
//       z'[o] = (r[o] - alpha (s[o] + beta q[o])) / diag[o],
//     so the vector update needs no launch of its own (r, q, s are double-buffered: neighbours read the old ones);
//   * kRowLanes lanes share a view -- a view of a dense scene graph has tens of neighbours, and one thread walking
//     them is a chain of dependent gathers (40 us per product at V = 5000); the partial rows are combined by a fixed
//     xor tree (row_lanes_sum);
//   * a launch only WRITES its block's partials (gamma, delta per axis; with two levels also the block's sum of s); the
//     NEXT launch starts by reducing the previous launch's partials -- every workgroup redundantly, in the same fixed
//     order (strided sums, then the 256-entry tree), so every workgroup holds the same bits -- and derives alpha, beta and
//     the stopping test from them.  (A grid-wide hand-over at the end of the launch instead -- fence, ticket, the last
//     workgroup reduces -- put an atomic and a serial tail on the critical path of a 15 us kernel.)  Partials and the scalar
//     state are double-buffered by launch parity, so nothing is read and written in the same launch.
// Everything is a fixed function of the graph: same input, same bits, on any number of ranks.
struct CgScalars {
    double alpha[3], beta[3];
    bool stop;  // converged, now or earlier: the launch has nothing more to do
};
// The head of every launch but the init pass: the scalars of this iteration from the block partials (STRIDE doubles per block,
// gamma and delta leading) of the PREVIOUS launch, and the state record written by workgroup 0.  red: 6 * kCgBlock doubles.
template <int STRIDE>
RDEV CgScalars cg_scalars_from_partials(const double* __restrict__ part_prev, uint32_t n_blocks, int prev_was_init, double tol,
                                        const CgState* __restrict__ st_prev, CgState* __restrict__ st_next, double* red, int tid) {
    CgScalars sc{{0, 0, 0}, {0, 0, 0}, true};
    if (st_prev->done) {  // (uniform) converged earlier: keep the record where the host reads it
        if (blockIdx.x == 0 && tid == 0) *st_next = *st_prev;
        return sc;
    }
    double v[6];
    strided_sum<6, kCgBlock>(part_prev, n_blocks, STRIDE, tid, v);
    block_tree_sum<6, kCgBlock>(v, red, tid, TreeInWave0{});
    bool done = true;
    double rz_new[3], rz0[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double g = v[c], dl = v[3 + c];
        if (prev_was_init) {
            rz0[c] = g;
            sc.beta[c] = 0.0;
            sc.alpha[c] = dl > 0.0 ? g / dl : 0.0;
            done &= !(g > 0.0);
        } else {
            rz0[c] = st_prev->rz0[c];
            const double a_prev = st_prev->alpha[c];
            const double bt = st_prev->rz[c] > 0.0 ? g / st_prev->rz[c] : 0.0;
            const double den = a_prev != 0.0 ? dl - bt * g / a_prev : dl;
            sc.beta[c] = bt;
            sc.alpha[c] = den > 0.0 ? g / den : 0.0;
            done &= !(g > tol * tol * rz0[c]);
        }
        rz_new[c] = g;
    }
    if (blockIdx.x == 0 && tid == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            st_next->rz[c] = rz_new[c];
            st_next->rz0[c] = rz0[c];
            st_next->alpha[c] = sc.alpha[c];
            st_next->beta[c] = sc.beta[c];
        }
        st_next->iters = prev_was_init ? 0.0 : st_prev->iters + 1.0;
        st_next->done = done;
        st_next->mean_step = 0.0;
        st_next->ticket = 0;
    }
    sc.stop = done;
    return sc;
}

// mode 1: the init pass (alpha = beta = 0; x and r stay, p becomes z, q becomes 0: produces s0 = A z0 and the partials of
// gamma0, delta0); mode 0: an iteration; mode 2: only the reduction and the state record (what the host reads between chunks
// of launches), no vector is touched.  TWO_LEVEL: rows in place of views, and the coarse correction of "two-level PCG" below.
template <bool TWO_LEVEL>
__global__ __launch_bounds__(kCgBlock) void cg_iteration_kernel(uint32_t n_views, const uint32_t* __restrict__ adj_ptr,
                                                                const uint32_t* __restrict__ adj_edge,
                                                                const uint32_t* __restrict__ adj_other,
                                                                const uint8_t* __restrict__ is_root, const double* __restrict__ w,
                                                                const double* __restrict__ diag, double* __restrict__ x,
                                                                double* __restrict__ p, const double* r_old, double* r_new,
                                                                const double* q_old, double* q_new, const double* s_old,
                                                                double* s_new, int mode, int prev_was_init, double tol,
                                                                const double* __restrict__ part_prev, double* __restrict__ part_next,
                                                                uint32_t n_blocks, const CgState* __restrict__ st_prev,
                                                                CgState* __restrict__ st_next, CoarseArgs<TWO_LEVEL> coarse) {
    constexpr int NP = TWO_LEVEL ? 9 : 6;  // partials per block: gamma (3), delta (3), two levels: the block's sum of s (3)
    __shared__ double lds[NP * kCgBlock + (TWO_LEVEL ? 12 * kMaxAggregates : 0)];
    double* const red = lds;
    const int tid = threadIdx.x, sub = tid & (kRowLanes - 1);
    CgScalars sc{{0, 0, 0}, {0, 0, 0}, false};
    if (mode != 1) {
        sc = cg_scalars_from_partials<NP>(part_prev, n_blocks, prev_was_init, tol, st_prev, st_next, red, tid);
        if (sc.stop || mode == 2) return;  // (uniform)
    }
    const double* const alpha = sc.alpha;
    const double* const beta = sc.beta;
    double c_old[3] = {0, 0, 0}, c_own[3] = {0, 0, 0};  // two levels: c of this block's aggregate, last launch's and this one's
    [[maybe_unused]] double* const l_c = lds + (TWO_LEVEL ? NP * kCgBlock + 3 * kMaxAggregates : 0);  // c = Ac^-1 rho
    if constexpr (TWO_LEVEL) {
        const uint32_t n_agg = coarse.n_agg;
        const uint32_t* __restrict__ agg_block = coarse.agg_block;
        const double* __restrict__ Ainv = coarse.Ainv;
        const double* __restrict__ cs_prev = coarse.cs_prev;
        double* __restrict__ cs_next = coarse.cs_next;
        double* const l_rho = lds + NP * kCgBlock;
        double(*const l_half)[3 * kMaxAggregates] = reinterpret_cast<double(*)[3 * kMaxAggregates]>(l_c + 3 * kMaxAggregates);
        // the coarse vectors of this iteration
        if (tid < (int)n_agg) {
            double rho[3] = {0, 0, 0}, kap[3] = {0, 0, 0};
            if (mode == 1) {
                const double* __restrict__ rpart = coarse.rpart;
                for (uint32_t b = agg_block[tid]; b < agg_block[tid + 1]; ++b)
#pragma unroll
                    for (int c = 0; c < 3; ++c) rho[c] += rpart[3 * (size_t)b + c];
            } else {
                double sig[3] = {0, 0, 0};
                for (uint32_t b = agg_block[tid]; b < agg_block[tid + 1]; ++b)
#pragma unroll
                    for (int c = 0; c < 3; ++c) sig[c] += part_prev[9 * (size_t)b + 6 + c];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    kap[c] = sig[c] + beta[c] * cs_prev[3 * (size_t)n_agg + 3 * tid + c];
                    rho[c] = cs_prev[3 * tid + c] - alpha[c] * kap[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                l_rho[3 * tid + c] = rho[c];
                if (blockIdx.x == 0) {
                    cs_next[3 * tid + c] = rho[c];
                    cs_next[3 * (size_t)n_agg + 3 * tid + c] = kap[c];
                }
            }
        }
        __syncthreads();
        {   // c = Ac^-1 rho: thread (a, half) sums half of the columns (Ac^-1 read through its symmetric counterpart, so that
            // consecutive lanes read consecutive words)
            const uint32_t a = (uint32_t)tid & (kMaxAggregates - 1), h = (uint32_t)tid >> 7, half = (n_agg + 1) / 2;
            const uint32_t b0 = h * half, b1 = min(n_agg, b0 + half);
            double acc[3] = {0, 0, 0};
            if (a < n_agg) {
                for (uint32_t b = b0; b < b1; ++b) {
                    const double m = Ainv[(size_t)b * n_agg + a];
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += m * l_rho[3 * b + c];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) l_half[h][3 * a + c] = acc[c];
            }
        }
        __syncthreads();
        if (tid < (int)n_agg) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double cn = l_half[0][3 * tid + c] + l_half[1][3 * tid + c];
                l_c[3 * tid + c] = cn;
                if (blockIdx.x == 0) cs_next[6 * (size_t)n_agg + 3 * tid + c] = cn;
            }
        }
        __syncthreads();
        const uint32_t my_agg = coarse.agg_of_block[blockIdx.x];
        if (my_agg != kNoAggregate) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                c_own[c] = l_c[3 * my_agg + c];
                c_old[c] = mode == 1 ? c_own[c] : cs_prev[6 * (size_t)n_agg + 3 * my_agg + c];
            }
        }
    }
    const uint32_t k = blockIdx.x * kRowsPerBlock + (uint32_t)(tid / kRowLanes);
    double gd[NP] = {};
    if (k < n_views) {
        const bool free_k = !is_root[k];
        // neighbours: their new z, rebuilt from the old vectors
        double y[3] = {0, 0, 0};
        if (free_k)
            for (uint32_t a = adj_ptr[k] + (uint32_t)sub; a < adj_ptr[k + 1]; a += kRowLanes) {
                uint32_t ag = 0;
                if constexpr (TWO_LEVEL) {
                    ag = coarse.adj_agg[a];
                    if (ag == kNoAggregate) continue;  // a gauge view
                }
                const uint32_t o = adj_other[a];
                if constexpr (!TWO_LEVEL)
                    if (is_root[o]) continue;
                const double we = w[adj_edge[a]], dn = diag[o], inv = dn > 0.0 ? 1.0 / dn : 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const size_t i = 3 * (size_t)o + c;
                    const double qo = s_old[i] + beta[c] * q_old[i];
                    if constexpr (TWO_LEVEL) y[c] -= we * ((r_old[i] - alpha[c] * qo) * inv + l_c[3 * ag + c]);
                    else y[c] -= we * ((r_old[i] - alpha[c] * qo) * inv);
                }
            }
        row_lanes_sum<3, kRowLanes>(y);
        if (sub == 0) {  // the view's own entries of every vector
            const double d = diag[k], inv = d > 0.0 ? 1.0 / d : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t i = 3 * (size_t)k + c;
                const double ro = r_old[i];
                double zo = ro * inv;
                if constexpr (TWO_LEVEL) zo = free_k ? ro * inv + c_old[c] : 0.0;
                const double pk = zo + beta[c] * p[i];
                const double qk = s_old[i] + beta[c] * q_old[i];
                const double rn = ro - alpha[c] * qk;
                double zn = rn * inv;
                if constexpr (TWO_LEVEL) zn = free_k ? rn * inv + c_own[c] : 0.0;
                const double sn = free_k ? d * zn + y[c] : 0.0;
                p[i] = pk;
                q_new[i] = qk;
                x[i] += alpha[c] * pk;
                r_new[i] = rn;
                s_new[i] = sn;
                gd[c] = rn * zn;
                gd[3 + c] = zn * sn;
                if constexpr (TWO_LEVEL) gd[6 + c] = sn;
            }
        }
    }
    block_tree_sum<NP, kCgBlock>(gd, red, tid, TreeInWave0{});
    if (tid == 0)
#pragma unroll
        for (int c = 0; c < NP; ++c) part_next[NP * (size_t)blockIdx.x + c] = gd[c];
}

// (gate: a record of the PCG state on the device, or null.  With a gate the kernel runs only if that solve has converged: the
// host queues it behind the reduce-only launch it is about to look at, so that a converged solve costs ONE round trip.
// veto: a device flag, or null; set = do nothing -- the two-level solve's "coarse matrix not inverted".)
__global__ __launch_bounds__(kCgBlock) void cg_step_norm_kernel(uint32_t n_views, const double* __restrict__ x,
                                                                double* __restrict__ partial, const CgState* __restrict__ gate,
                                                                const int* __restrict__ veto) {
    __shared__ double red[3 * kCgBlock];
    const int tid = threadIdx.x;
    if ((gate && !gate->done) || (veto && *veto)) return;  // (uniform)
    const uint32_t k = blockIdx.x * kCgBlock + tid;
    double nd[3] = {0, 0, 0};
    if (k < n_views)
        nd[0] = sqrt(x[3 * (size_t)k] * x[3 * (size_t)k] + x[3 * (size_t)k + 1] * x[3 * (size_t)k + 1] +
                     x[3 * (size_t)k + 2] * x[3 * (size_t)k + 2]);
    block_tree_sum<3, kCgBlock>(nd, red, tid);
    if (tid == 0)
        for (int c = 0; c < 3; ++c) partial[3 * blockIdx.x + c] = nd[c];
}

// R_view <- R_view exp(x_k).  row_view: null = x is in view numbering; else the view of row k of the two-level solve's
// renumbering (0xFFFFFFFF: a padding row, no view).
__global__ __launch_bounds__(256) void rot_update_kernel(uint32_t n_rows, const double* __restrict__ x,
                                                         const uint32_t* __restrict__ row_view, double* __restrict__ R,
                                                         const CgState* __restrict__ gate, const int* __restrict__ veto) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_rows || (gate && !gate->done) || (veto && *veto)) return;
    const uint32_t v = row_view ? row_view[k] : k;
    if (v == 0xFFFFFFFFu) return;
    double Rk[9], Ex[9], Rn[9];
    const double wv[3] = {x[3 * (size_t)k], x[3 * (size_t)k + 1], x[3 * (size_t)k + 2]};
#pragma unroll
    for (int c = 0; c < 9; ++c) Rk[c] = R[9 * (size_t)v + c];
    so3_exp(wv, Ex);
    mat3_mul(Rk, Ex, Rn);
#pragma unroll
    for (int c = 0; c < 9; ++c) R[9 * (size_t)v + c] = Rn[c];
}

// ---- two-level PCG (dense, band-like view graphs: every Jacobi solve runs into the cap) ----------------------------------
// A view graph whose views see their neighbours along a walk or a ring -- tens of edges per view, so the spanning-tree kernel
// does not take it -- has a Laplacian with kappa ~ (V / reach)^2: Jacobi-preconditioned CG needs hundreds of iterations per
// solve and the cap truncates every one of them (config 4 at V = 5000, k = 40: 13 outer steps x 200 iterations).  Here the
// preconditioner gets a second level:  M^-1 = D^-1 + P Ac^-1 P^T,  P = the indicator of <= 128 AGGREGATES of neighbouring
// views (host: region growing over the adjacency), Ac = P^T A P assembled and inverted on the device for every outer step's
// weights (a dense <= 128 x 128 matrix: Gauss-Jordan in one workgroup's LDS).  The iteration keeps the one-launch form:
//   * the rows are renumbered so that an aggregate is a run of whole 16-row blocks (padding rows are inert): P^T v of a
//     vector written by the previous launch is a fixed-order sum of that launch's block partials;
//   * rho = P^T r and kappa = P^T q follow the same recurrences as r and q (kappa' = sigma + beta kappa, rho' = rho - alpha
//     kappa', sigma = P^T s from the block partials), every workgroup redundantly, workgroup 0 stores them by launch parity;
//   * every workgroup applies Ac^-1 to rho' (<= 128 x 128 doubles from L2, read through the symmetric counterpart so that
//     consecutive lanes read consecutive words) and keeps c = Ac^-1 rho' in LDS; a neighbour's rebuilt z gets c of ITS aggregate
//     (the aggregate id travels with the incidence), the view's own z the block's.
// Same input, same bits: no atomics, every sum in a fixed order.  The kernels: cg_init_kernel<true> and
// cg_iteration_kernel<true> above; the coarse matrix's assembly and inversion here.

// Ac = P^T A P: workgroup a owns row a.  The incidences of the aggregate's rows are one contiguous range of the adjacency: the
// threads stage (column, weight) of a chunk of it in LDS side by side, then thread (b, segment) adds what falls into column b
// within its eighth of the chunk in index order and the eight partial sums are added in segment order -- a fixed order per
// entry, and the loads of a chunk are in flight together (walking them one after the other, every thread alike, took 300 us per
// outer step).  The diagonal entry also takes the rows' diag.
constexpr int kAsmChunk = 2048, kAsmSegments = 8;
__global__ __launch_bounds__(kMaxAggregates * kAsmSegments) void cg2_coarse_assemble_kernel(
    uint32_t n_agg, const uint32_t* __restrict__ agg_block, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj_edge,
    const uint8_t* __restrict__ adj_agg, const uint8_t* __restrict__ is_root, const double* __restrict__ w, const double* __restrict__ diag,
    double* __restrict__ Ac) {
    __shared__ double val[kAsmChunk];
    __shared__ uint8_t col[kAsmChunk];
    __shared__ double seg_sum[kAsmSegments][kMaxAggregates];
    const uint32_t a = blockIdx.x, tid = threadIdx.x, b = tid & (kMaxAggregates - 1), seg = tid / kMaxAggregates;
    constexpr uint32_t kThreads = kMaxAggregates * kAsmSegments, kPerSeg = kAsmChunk / kAsmSegments;
    const uint32_t row0 = agg_block[a] * kRowsPerBlock, row1 = agg_block[a + 1] * kRowsPerBlock;
    double acc = 0;
    // (an inert row -- padding -- has no incidences and diag 0)
    for (uint32_t r0 = row0; r0 < row1; r0 += kAsmChunk) {
        const uint32_t n = min((uint32_t)kAsmChunk, row1 - r0);
        for (uint32_t i = tid; i < n; i += kThreads) val[i] = is_root[r0 + i] ? 0.0 : diag[r0 + i];
        __syncthreads();
        if (tid == a)  // (segment 0, column a)
            for (uint32_t i = 0; i < n; ++i) acc += val[i];
        __syncthreads();
    }
    const uint32_t i0 = adj_ptr[row0], i1 = adj_ptr[row1];
    for (uint32_t c0 = i0; c0 < i1; c0 += kAsmChunk) {
        const uint32_t n = min((uint32_t)kAsmChunk, i1 - c0);
        for (uint32_t i = tid; i < n; i += kThreads) {
            col[i] = adj_agg[c0 + i];
            val[i] = w[adj_edge[c0 + i]];
        }
        __syncthreads();
        double part = 0;
        const uint32_t e1 = min(n, (seg + 1) * kPerSeg);
        for (uint32_t i = seg * kPerSeg; i < e1; ++i)
            if (col[i] == b) part -= val[i];  // (incidences to gauge views carry kNoAggregate)
        seg_sum[seg][b] = part;
        __syncthreads();
        if (seg == 0)
#pragma unroll
            for (int g = 0; g < kAsmSegments; ++g) acc += seg_sum[g][b];
        __syncthreads();
    }
    if (seg == 0 && b < n_agg) Ac[(size_t)a * n_agg + b] = acc;
}

// Ac^-1 by Gauss-Jordan without pivoting (Ac is symmetric positive definite) in one workgroup, symmetrised on the way out;
// status = 1 when a pivot was not positive.  The matrix (padded to 128 x 128 by the identity) lives in REGISTERS: thread
// (ti, tj) of the 32 x 32 owns the 4 x 4 tile at (4 ti, 4 tj) through all steps; a step sends the pivot column and row through
// LDS (double-buffered by step parity: one barrier per step) and every thread reads its four entries of each -- 8 LDS reads
// for 16 updates (one entry per thread and LDS word, or the matrix itself in LDS, was bound by LDS bandwidth: 296 us).
// The rule per entry: (k,k) -> 1/p; row k -> M[k][j] / p; column k -> -M[i][k] / p; else M[i][j] - M[i][k] (M[k][j] / p).
__global__ __launch_bounds__(1024) void cg2_coarse_invert_kernel(uint32_t n, const double* __restrict__ Ac, double* __restrict__ Ainv,
                                                                 int* __restrict__ status) {
    __shared__ double colb[2][kMaxAggregates], rowb[2][kMaxAggregates];
    extern __shared__ double lds_inv[];  // n * n doubles: only for the symmetrisation at the end
    const uint32_t tid = threadIdx.x, ti = tid >> 5, tj = tid & 31;
    double v[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = 4 * ti + a, j = 4 * tj + b;
            v[a][b] = (i < n && j < n) ? Ac[(size_t)i * n + j] : (i == j ? 1.0 : 0.0);
        }
    bool bad = false;
    for (uint32_t k = 0; k < n; ++k) {
        double* col = colb[k & 1];
        double* row = rowb[k & 1];
        const uint32_t kt = k >> 2, kr = k & 3;  // (uniform: the switches below are scalar branches, the register indices static)
        if (tj == kt) {
            switch (kr) {
                case 0: for (int a = 0; a < 4; ++a) col[4 * ti + a] = v[a][0]; break;
                case 1: for (int a = 0; a < 4; ++a) col[4 * ti + a] = v[a][1]; break;
                case 2: for (int a = 0; a < 4; ++a) col[4 * ti + a] = v[a][2]; break;
                default: for (int a = 0; a < 4; ++a) col[4 * ti + a] = v[a][3]; break;
            }
        }
        if (ti == kt) {
            switch (kr) {
                case 0: for (int b = 0; b < 4; ++b) row[4 * tj + b] = v[0][b]; break;
                case 1: for (int b = 0; b < 4; ++b) row[4 * tj + b] = v[1][b]; break;
                case 2: for (int b = 0; b < 4; ++b) row[4 * tj + b] = v[2][b]; break;
                default: for (int b = 0; b < 4; ++b) row[4 * tj + b] = v[3][b]; break;
            }
        }
        __syncthreads();
        const double piv = row[k];
        bad |= !(piv > 0.0);
        const double pinv = piv > 0.0 ? 1.0 / piv : 0.0;
        double c[4], r[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            c[a] = col[4 * ti + a];
            r[a] = row[4 * tj + a] * pinv;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) v[a][b] = v[a][b] - c[a] * r[b];
        // the pivot row, the pivot column and the pivot itself (few lanes; which of a tile's rows / columns is uniform)
        if (ti == kt) {
            switch (kr) {
                case 0: for (int b = 0; b < 4; ++b) v[0][b] = r[b]; break;
                case 1: for (int b = 0; b < 4; ++b) v[1][b] = r[b]; break;
                case 2: for (int b = 0; b < 4; ++b) v[2][b] = r[b]; break;
                default: for (int b = 0; b < 4; ++b) v[3][b] = r[b]; break;
            }
        }
        if (tj == kt) {
            switch (kr) {
                case 0: for (int a = 0; a < 4; ++a) v[a][0] = -c[a] * pinv; break;
                case 1: for (int a = 0; a < 4; ++a) v[a][1] = -c[a] * pinv; break;
                case 2: for (int a = 0; a < 4; ++a) v[a][2] = -c[a] * pinv; break;
                default: for (int a = 0; a < 4; ++a) v[a][3] = -c[a] * pinv; break;
            }
            if (ti == kt) {
                switch (kr) {
                    case 0: v[0][0] = pinv; break;
                    case 1: v[1][1] = pinv; break;
                    case 2: v[2][2] = pinv; break;
                    default: v[3][3] = pinv; break;
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = 4 * ti + a, j = 4 * tj + b;
            if (i < n && j < n) lds_inv[(size_t)i * n + j] = v[a][b];
        }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = 4 * ti + a, j = 4 * tj + b;
            if (i < n && j < n) Ainv[(size_t)i * n + j] = 0.5 * (v[a][b] + lds_inv[(size_t)j * n + i]);
        }
    if (tid == 0) *status = bad ? 1 : 0;
}

// pgi_edge records (status OK) -> rotation-graph edges, all on the device: idx[e] = pair of edge e
__global__ __launch_bounds__(256) void rot_edges_from_table_kernel(const pgi_edge* __restrict__ table, const uint32_t* __restrict__ idx,
                                                                    const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                                                                    const double* __restrict__ weight, uint32_t n_edges,
                                                                    RotEdgeDev* __restrict__ out) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const pgi_edge* rec = table + idx[e];
    RotEdgeDev o;
    o.src = src[e];
    o.dst = dst[e];
#pragma unroll
    for (int c = 0; c < 9; ++c) o.R[c] = rec->R[c];
    o.weight = weight[e];
    out[e] = o;
}
// rotations of selected edges (the spanning forest's) -> a dense array for the host
__global__ __launch_bounds__(256) void rot_gather_R_kernel(const RotEdgeDev* __restrict__ edges, const uint32_t* __restrict__ sel,
                                                           uint32_t n_sel, double* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const RotEdgeDev* e = edges + sel[k];
#pragma unroll
    for (int c = 0; c < 9; ++c) out[9 * (size_t)k + c] = e->R[c];
}

// ---- host: BFS initialisation over the maximum-weight spanning forest (spanning_forest: pgi_graph_host.hpp) ----------------
// BFS over the forest; R_of(e) = pointer to the 9 doubles of edge e's relative rotation
template <class RofE>
static void forest_bfs_init(uint32_t V, const std::vector<std::vector<ForestEdge>>& adj, RofE R_of, std::vector<double>& R,
                            std::vector<uint8_t>& is_root) {
    R.assign((size_t)V * 9, 0.0);
    is_root.assign(V, 0);
    std::vector<uint8_t> seen(V, 0);
    std::vector<uint32_t> queue;
    for (uint32_t root = 0; root < V; ++root) {
        if (seen[root]) continue;
        seen[root] = 1;
        is_root[root] = 1;
        R[9 * (size_t)root] = R[9 * (size_t)root + 4] = R[9 * (size_t)root + 8] = 1.0;
        queue.assign(1, root);
        for (size_t h = 0; h < queue.size(); ++h) {
            const uint32_t u = queue[h];
            for (const ForestEdge& pr : adj[u]) {
                const uint32_t e = pr.edge, v = pr.other & 0x7FFFFFFFu;
                const bool inv = pr.other >> 31;
                if (seen[v]) continue;
                seen[v] = 1;
                const double* Rr = R_of(e);
                const double* Ru = &R[9 * (size_t)u];
                double* Rv = &R[9 * (size_t)v];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) {
                        double s = 0;
                        for (int k = 0; k < 3; ++k) s += (inv ? Rr[3 * k + i] : Rr[3 * i + k]) * Ru[3 * k + j];
                        Rv[3 * i + j] = s;
                    }
                queue.push_back(v);
            }
        }
    }
}

// ---- host: the solve proper.  The rotation-graph edges are already in HBM (RotEdgeDev[n_edges]); the host holds only their
// endpoints, the initial rotations, the root flags and the spanning forest.
//   R <- forest initialisation;  per outer step (l1_iters L1 steps, then IRLS):  residuals and robust weights;  solve the
//   weighted-Laplacian system for the step by ONE of: the two-level PCG (deep, dense graphs), the spanning-tree PCG (sparse
//   graphs on which Jacobi ran into its cap), the one-workgroup PCG (few views), the multi-workgroup Jacobi PCG;  R <- R exp(d);
//   stop when the mean step falls below tol.

// The environment knobs (experiments, tests, diagnosis), read once per call.
struct RotavgKnobs {
    bool timing = false;                        // PGI_ROTAVG_TIMING: wall clock of the host-visible phases on stderr
    bool trace = false;                         // PGI_ROTAVG_TRACE: one line per outer iteration on stderr
    uint32_t single_wg_views = kSingleWgViews;  // PGI_ROTAVG_SINGLE_WG_VIEWS: at or below, the one-workgroup solve
    uint32_t cg_iters = 0;                      // PGI_ROTAVG_CG_ITERS: replaces the parameters' iteration cap (0: not set)
    uint32_t tree_cg_iters = 0;                 // PGI_ROTAVG_TREE_CG_ITERS: replaces the tree kernel's cap (0: not set)
    int two_level = 1;                          // PGI_ROTAVG_TWO_LEVEL: 0 never, 1 by the depth rule, 2 always (tests)
    double cg_tol = kInnerTolerance;            // PGI_ROTAVG_CG_TOL: relative tolerance of every inner solve
};
static RotavgKnobs read_rotavg_knobs() {
    RotavgKnobs k;
    k.timing = std::getenv("PGI_ROTAVG_TIMING") != nullptr;
    k.trace = std::getenv("PGI_ROTAVG_TRACE") != nullptr;
    if (const char* e = std::getenv("PGI_ROTAVG_SINGLE_WG_VIEWS")) k.single_wg_views = (uint32_t)std::max(0, std::atoi(e));
    if (const char* e = std::getenv("PGI_ROTAVG_CG_ITERS")) k.cg_iters = (uint32_t)std::max(1, std::atoi(e));
    if (const char* e = std::getenv("PGI_ROTAVG_TREE_CG_ITERS")) k.tree_cg_iters = (uint32_t)std::max(1, std::atoi(e));
    if (const char* e = std::getenv("PGI_ROTAVG_TWO_LEVEL")) k.two_level = std::atoi(e);
    if (const char* e = std::getenv("PGI_ROTAVG_CG_TOL")) k.cg_tol = std::min(1e-2, std::max(1e-14, std::atof(e)));
    return k;
}
struct PhaseClock {
    bool on;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit PhaseClock(bool enabled) : on(enabled) {}
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[rotavg timing] %-44s %8.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - t).count());
        t = now;
    }
};

// The device buffers of one call (regions of one DeviceWorkspace) and what every solver of the outer loop needs.
struct RotSolve {
    hipStream_t st;
    uint32_t n_views, n_edges;
    pgi_rotavg_params prm;
    double cg_tol;
    double* R;
    uint32_t *ptr, *aedge, *aother;
    int8_t* asign;
    uint8_t* root;
    double *omega, *w, *diag, *x, *p, *r[2], *q[2], *s[2];
    double *stats, *norm, *part;  // stats: mean |d|, iterations (one-workgroup solve); norm, part: block partials
    CgState* cg;                  // two launch parities + the record the host reads
    // tree path (views in the numbering of plan_tree_order)
    uint32_t *tptr, *tedge, *tother, *tn2o, *tpe, *tsz, *ten, *tex;
    int8_t* tsign;
    TreeIncidence* inc;
    double* its;
    std::vector<double> norm_host;  // block partials of the step norm (multi-workgroup, tree and two-level paths)
};

// The step-norm and update launches for a solution x (row_view: see rot_update_kernel), gated on a PCG record and a veto flag or
// not, and the copy of the norm partials.  Queued BEFORE the host looks at the record, so that a solve found converged is
// already applied (one round trip per outer step).
static int queue_step(RotSolve& S, uint32_t n, const double* x, const uint32_t* row_view, double* d_norm, const CgState* gate,
                      const int* veto) {
    const uint32_t nb = (n + kCgBlock - 1) / kCgBlock;
    hipLaunchKernelGGL(cg_step_norm_kernel, dim3(nb), dim3(kCgBlock), 0, S.st, n, x, d_norm, gate, veto);
    hipLaunchKernelGGL(rot_update_kernel, dim3((n + 255) / 256), dim3(256), 0, S.st, n, x, row_view, S.R, gate, veto);
    S.norm_host.resize(3 * (size_t)nb);
    HIP_TRY(hipMemcpyAsync(S.norm_host.data(), d_norm, S.norm_host.size() * sizeof(double), hipMemcpyDeviceToHost, S.st));
    return 0;
}

// Which buffers a launch of cg_iteration_kernel reads and writes.  The vectors r, q, s alternate with every launch that
// touches them; launch j reads parity (j - 1) & 1 of the partials and the state and writes parity j & 1.
struct LaunchParity {
    int cur = 0;          // the buffers holding the vectors of the last finished iteration
    uint32_t launch = 0;  // launches so far
    int prev() const { return (int)((launch + 1) & 1u); }
    int next() const { return (int)(launch & 1u); }
    int prev_was_init() const { return launch == 1 ? 1 : 0; }
    void launched(int mode) {  // (a reduce-only launch, mode 2, moves nothing)
        if (mode == 2) return;
        cur ^= 1;
        ++launch;
    }
};

// Looks at the record between chunks of launches (each look a round trip): after 16, 48, 112, 176, ... launches -- except
// that a solve whose predecessor in the outer loop converged after n iterations first runs n + 2 + n / 8 launches in one go
// (consecutive IRLS systems differ by their weights only and need nearly the same count; launches after convergence are
// no-ops, so WHERE the host looks changes no bit of the result), and one whose predecessor ran into the cap runs the whole
// cap.  Graphs that may still switch to the tree path (slow_break) keep every look from 112 on: the switch is decided there.
// solve.iterate(0): one iteration launch; iterate(2): the reduce-only launch that fills solve.record; solve.finish(record):
// queue_step gated on the record.  Returns < 0 on a HIP error, else 1 / 0 = converged (and applied) or not; hs = the last record.
template <class Solve>
static int pcg_looks(Solve& solve, hipStream_t st, uint32_t cap, uint32_t& pred, bool slow_break, CgState& hs) {
    int done = 0;
    uint32_t ci = 0, boundary = 16, step = 16;
    const uint32_t guess = pred + 2 + pred / 8;
    uint32_t jump = (pred && (!slow_break || guess <= 64)) ? std::min<uint32_t>(guess, cap) : 0;
    while (ci < cap) {
        uint32_t target;
        bool scheduled = true;
        if (jump > ci) {
            target = jump;
            jump = 0;
            scheduled = false;
        } else {
            while (boundary <= ci) {
                step = std::min<uint32_t>(2 * step, 64);
                boundary += step;
            }
            target = std::min<uint32_t>(boundary, cap);
        }
        for (; ci < target; ++ci) solve.iterate(0);  // kernels no-op once converged
        solve.iterate(2);
        {
            const int rc = solve.finish(solve.record);
            if (rc < 0) return rc;
        }
        HIP_TRY(hipMemcpyAsync(&hs, solve.record, sizeof hs, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        done = hs.done;
        pred = done ? (uint32_t)hs.iters : cap;
        if (done) break;
        // hopeless for this preconditioner: after 64 iterations a well-conditioned (dense) graph has gained ten orders of
        // magnitude, a sequence-like one not even three
        if (scheduled && slow_break && ci >= 64) {
            bool slow = false;
            for (int c = 0; c < 3; ++c) slow |= hs.rz[c] > 1e-6 * hs.rz0[c];
            if (slow) break;
        }
    }
    return done;
}

// One multi-workgroup Jacobi PCG solve of the current outer step (construction queues the init kernel and the init pass).
struct JacobiSolve {
    RotSolve& S;
    const uint32_t nbp;  // workgroups: kRowLanes lanes per view
    LaunchParity lp;
    CgState* record;     // written by the reduce-only launch, read by the host
    explicit JacobiSolve(RotSolve& s) : S(s), nbp((s.n_views + kRowsPerBlock - 1) / kRowsPerBlock), record(s.cg + 2) {
        hipLaunchKernelGGL(cg_init_kernel<false>, dim3(nbp), dim3(kCgBlock), 0, S.st, S.n_views, S.ptr, S.aedge, S.asign, S.root, S.omega, S.w,
                           S.diag, S.x, S.r[0], S.p, (double*)nullptr, S.q[0], S.s[0], S.cg);
        iterate(1);
    }
    void iterate(int mode) {  // 1: init pass, 0: iteration, 2: reduce the last launch's partials into `record`
        double* const part[2] = {S.part, S.part + 6 * ((size_t)nbp + 1)};
        const int c = lp.cur, prev = lp.prev(), next = lp.next();
        hipLaunchKernelGGL(cg_iteration_kernel<false>, dim3(mode == 2 ? 1u : nbp), dim3(kCgBlock), 0, S.st, S.n_views, S.ptr, S.aedge, S.aother,
                           S.root, S.w, S.diag, S.x, S.p, S.r[c], S.r[c ^ 1], S.q[c], S.q[c ^ 1], S.s[c], S.s[c ^ 1], mode, lp.prev_was_init(),
                           S.cg_tol, part[prev], part[next], nbp, S.cg + prev, mode == 2 ? record : S.cg + next, NoCoarseLevel{});
        lp.launched(mode);
    }
    int finish(const CgState* gate) { return queue_step(S, S.n_views, S.x, nullptr, S.norm, gate, nullptr); }
};

// ---- two-level preconditioner (see "two-level PCG" above).  WHEN: the graph is too dense for the tree path, too large for
// the one-workgroup solve, and DEEP -- the breadth-first walk from the gauge views needs kTwoLevelDepth levels or more, as on a
// walk or a ring (V / reach levels), where Jacobi needs hundreds of iterations whatever the weights; a densely connected
// graph has a handful of levels, Jacobi converges in ~20 iterations there and a capped first L1 solve is merely a hard
// first step.
constexpr uint32_t kTwoLevelDepth = 12;
struct TwoLevel {  // the plan and its device buffers (a workspace of their own: most graphs never need them)
    TwoLevelPlan plan;
    DeviceWorkspace ws;
    uint32_t *ptr, *edge, *other, *row_view, *agg_block;
    int8_t* sign;
    uint8_t *agg, *root, *agg_of_block;
    double *diag, *x, *p, *r[2], *q[2], *s[2], *part, *rpart, *cs, *Ac, *Ainv, *norm;
    CgState* cg;
    int* status;  // set: the coarse matrix was not inverted
    size_t inv_lds = 0;
};
// 0: ready; 1: this graph cannot have a plan; < 0: error
static int plan_and_upload_two_level(RotSolve& S, const IncidenceCsr& g, const std::vector<uint8_t>& is_root,
                                     const std::vector<uint32_t>& bfs_order, TwoLevel& t) {
    if (!plan_two_level(S.n_views, g, is_root, bfs_order, kRowsPerBlock, kMaxAggregates, t.plan)) return 1;
    const TwoLevelPlan& pl = t.plan;
    const size_t N = pl.n_rows, NB = pl.n_blocks, NA = pl.n_agg, I = pl.aedge.size();
    t.ws.add(t.ptr, N + 1); t.ws.add(t.edge, I); t.ws.add(t.other, I); t.ws.add(t.sign, I); t.ws.add(t.agg, I);
    t.ws.add(t.root, N); t.ws.add(t.row_view, N); t.ws.add(t.agg_block, NA + 1); t.ws.add(t.agg_of_block, NB);
    t.ws.add(t.diag, N); t.ws.add(t.x, 3 * N); t.ws.add(t.p, 3 * N);
    for (int b = 0; b < 2; ++b) { t.ws.add(t.r[b], 3 * N); t.ws.add(t.q[b], 3 * N); t.ws.add(t.s[b], 3 * N); }
    t.ws.add(t.part, 2 * 9 * (NB + 1));  // block partials, by launch parity
    t.ws.add(t.rpart, 3 * NB); t.ws.add(t.cs, 2 * 9 * NA); t.ws.add(t.Ac, NA * NA); t.ws.add(t.Ainv, NA * NA);
    t.ws.add(t.cg, 4); t.ws.add(t.status, 4); t.ws.add(t.norm, 3 * ((N + kCgBlock - 1) / kCgBlock));
    HIP_TRY(t.ws.alloc());
    HIP_TRY(upload(t.ptr, pl.ptr, S.st));
    HIP_TRY(upload(t.edge, pl.aedge, S.st));
    HIP_TRY(upload(t.other, pl.aother, S.st));
    HIP_TRY(upload(t.sign, pl.asign, S.st));
    HIP_TRY(upload(t.agg, pl.aagg, S.st));
    HIP_TRY(upload(t.root, pl.root, S.st));
    HIP_TRY(upload(t.row_view, pl.row_view, S.st));
    HIP_TRY(upload(t.agg_block, pl.agg_block, S.st));
    HIP_TRY(upload(t.agg_of_block, pl.agg_of_block, S.st));
    HIP_TRY(hipStreamSynchronize(S.st));
    t.inv_lds = NA * NA * sizeof(double);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&cg2_coarse_invert_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)t.inv_lds));
    return 0;
}
// One two-level solve of the current outer step (construction queues the init kernel, the coarse matrix and the init pass).
struct TwoLevelSolve {
    RotSolve& S;
    TwoLevel& t;
    const uint32_t N, NB, NA;
    LaunchParity lp;
    CgState* record;
    int status = 0;  // host copy of t.status, valid after the synchronisation that follows a finish()
    TwoLevelSolve(RotSolve& s, TwoLevel& two) : S(s), t(two), N(two.plan.n_rows), NB(two.plan.n_blocks), NA(two.plan.n_agg), record(two.cg + 2) {
        hipLaunchKernelGGL(cg_init_kernel<true>, dim3(NB), dim3(kCgBlock), 0, S.st, N, t.ptr, t.edge, t.sign, t.root, S.omega, S.w, t.diag, t.x,
                           t.r[0], t.p, t.rpart, t.q[0], t.s[0], t.cg);
        hipLaunchKernelGGL(cg2_coarse_assemble_kernel, dim3(NA), dim3(kMaxAggregates * kAsmSegments), 0, S.st, NA, t.agg_block, t.ptr, t.edge, t.agg,
                           t.root, S.w, t.diag, t.Ac);
        hipLaunchKernelGGL(cg2_coarse_invert_kernel, dim3(1), dim3(1024), t.inv_lds, S.st, NA, t.Ac, t.Ainv, t.status);
        iterate(1);
    }
    void iterate(int mode) {
        double* const part[2] = {t.part, t.part + 9 * ((size_t)NB + 1)};
        double* const cs[2] = {t.cs, t.cs + 9 * (size_t)NA};
        const int c = lp.cur, prev = lp.prev(), next = lp.next();
        const CoarseLevel coarse{NA, t.agg, t.agg_block, t.agg_of_block, t.Ainv, t.rpart, cs[prev], cs[next]};
        hipLaunchKernelGGL(cg_iteration_kernel<true>, dim3(mode == 2 ? 1u : NB), dim3(kCgBlock), 0, S.st, N, t.ptr, t.edge, t.other, t.root, S.w,
                           t.diag, t.x, t.p, t.r[c], t.r[c ^ 1], t.q[c], t.q[c ^ 1], t.s[c], t.s[c ^ 1], mode, lp.prev_was_init(), S.cg_tol,
                           part[prev], part[next], NB, t.cg + prev, mode == 2 ? record : t.cg + next, coarse);
        lp.launched(mode);
    }
    int finish(const CgState* gate) {
        const int rc = queue_step(S, N, t.x, t.row_view, t.norm, gate, t.status);
        if (rc < 0) return rc;
        HIP_TRY(hipMemcpyAsync(&status, t.status, sizeof status, hipMemcpyDeviceToHost, S.st));
        return 0;
    }
};
// applied to the rotations, S.norm_host filled, iters = PCG iterations; 1 when the coarse matrix could not be inverted (nothing
// was applied, the caller falls back), < 0 on a HIP error
static int solve_two_level(RotSolve& S, TwoLevel& t, uint32_t& predicted, double& iters) {
    TwoLevelSolve solve(S, t);
    CgState hs{};
    const int done = pcg_looks(solve, S.st, S.prm.cg_iters, predicted, false, hs);
    if (done < 0) return done;
    if (!done) {  // ran into the cap: the truncated solution is the step
        const int rc = solve.finish(nullptr);
        if (rc < 0) return rc;
        HIP_TRY(hipStreamSynchronize(S.st));
    }
    if (solve.status) return 1;
    iters = hs.iters;
    return 0;
}

// ---- tree path (rot_solve_tree_kernel).  Only sparse graphs qualify: the forest holds V - 1 of the E edges, and on a dense
// graph (E / V = 21 in the k = 20 benchmark) it is a far worse preconditioner than Jacobi (1 380 iterations against 19) -- there
// a capped first L1 solve is simply a hard first step, not a reason to switch.
struct TreePath {
    bool ok = false;          // the graph qualifies
    bool in_use = false;      // set once the Jacobi-preconditioned solve has run into its iteration cap
    uint32_t own = 0;         // views per thread
    uint32_t cg_iters = 0;    // iteration cap of the kernel
    size_t lds = 0;
    TreeOrder order;          // (kept: the uploads read it)
};
static void solve_with_tree(RotSolve& S, const TreePath& tp) {  // writes every entry of x
    hipLaunchKernelGGL(rot_solve_tree_kernel, dim3(3), dim3(1024), tp.lds, S.st, S.n_views, tp.own, S.tptr, S.tedge, S.tother, S.tsign, S.tpe,
                       S.tsz, S.ten, S.tex, S.tn2o, S.omega, S.w, tp.cg_iters, S.cg_tol, S.inc, S.x, S.its);
}

// Allocation and uploads: the adjacency, the initial rotations, the root flags, and for a graph that qualifies the tree order.
static int rotavg_setup(RotSolve& S, DeviceWorkspace& ws, const IncidenceCsr& g, const std::vector<double>& R,
                        const std::vector<uint8_t>& is_root, const std::vector<std::vector<ForestEdge>>& forest, TreePath& tp) {
    const size_t V = S.n_views, E = S.n_edges;
    ws.add(S.R, 9 * V); ws.add(S.ptr, V + 1); ws.add(S.aedge, 2 * E); ws.add(S.aother, 2 * E); ws.add(S.asign, 2 * E); ws.add(S.root, V);
    ws.add(S.omega, 3 * E); ws.add(S.w, E); ws.add(S.diag, V); ws.add(S.x, 3 * V); ws.add(S.p, 3 * V);
    for (int b = 0; b < 2; ++b) { ws.add(S.r[b], 3 * V); ws.add(S.q[b], 3 * V); ws.add(S.s[b], 3 * V); }
    ws.add(S.stats, 2); ws.add(S.norm, 3 * ((V + kCgBlock - 1) / kCgBlock)); ws.add(S.cg, 4);
    ws.add(S.part, 2 * 6 * ((V + kRowsPerBlock - 1) / kRowsPerBlock + 1));  // block partials, by launch parity
    ws.add(S.tptr, V + 1); ws.add(S.tedge, 2 * E); ws.add(S.tother, 2 * E); ws.add(S.tsign, 2 * E);
    ws.add(S.tn2o, V); ws.add(S.tpe, V); ws.add(S.tsz, V); ws.add(S.ten, V); ws.add(S.tex, V); ws.add(S.inc, 2 * E); ws.add(S.its, 4);
    HIP_TRY(ws.alloc());
    HIP_TRY(upload(S.R, R, S.st));
    HIP_TRY(upload(S.ptr, g.ptr, S.st));
    HIP_TRY(upload(S.aedge, g.edge, S.st));
    HIP_TRY(upload(S.aother, g.other, S.st));
    HIP_TRY(upload(S.asign, g.sign, S.st));
    HIP_TRY(upload(S.root, is_root, S.st));
    tp.ok = S.n_views <= kTreeViews && (uint64_t)S.n_edges <= 8ull * S.n_views;
    if (!tp.ok) return 0;
    tp.own = std::max<uint32_t>(1u, (S.n_views + 1023u) / 1024u);
    tp.order = plan_tree_order(S.n_views, g, is_root, forest);
    const TreeOrder& t = tp.order;
    HIP_TRY(upload(S.tptr, t.adj.ptr, S.st));
    HIP_TRY(upload(S.tedge, t.adj.edge, S.st));
    HIP_TRY(upload(S.tother, t.adj.other, S.st));
    HIP_TRY(upload(S.tsign, t.adj.sign, S.st));
    HIP_TRY(upload(S.tn2o, t.new_to_old, S.st));
    HIP_TRY(upload(S.tpe, t.parent_edge, S.st));
    HIP_TRY(upload(S.tsz, t.sub_size, S.st));
    HIP_TRY(upload(S.ten, t.tour_enter, S.st));
    HIP_TRY(upload(S.tex, t.tour_exit, S.st));
    tp.lds = ((size_t)3 * 1024 * tp.own + 16) * sizeof(double);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rot_solve_tree_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tp.lds));
    return 0;
}

static int rotavg_solve(pgi_ctx* ctx, const RotavgKnobs& knobs, const pgi_rotavg_params& prm_in, uint32_t n_views, uint32_t n_edges,
                        const uint32_t* h_src, const uint32_t* h_dst, const RotEdgeDev* d_rot, const std::vector<double>& R,
                        const std::vector<uint8_t>& is_root, const std::vector<std::vector<ForestEdge>>& forest, double* h_R_out,
                        uint32_t* h_iters_out) {
    PhaseClock clk(knobs.timing);
    const IncidenceCsr g = build_incidence_csr(n_views, n_edges, h_src, h_dst, -1);  // sign +1: the view is the edge's dst
    RotSolve S{};
    S.st = ctx->stream;
    S.n_views = n_views;
    S.n_edges = n_edges;
    S.prm = prm_in;
    if (knobs.cg_iters) S.prm.cg_iters = knobs.cg_iters;
    S.cg_tol = knobs.cg_tol;
    const pgi_rotavg_params& prm = S.prm;
    hipStream_t st = S.st;
    DeviceWorkspace ws;
    TreePath tree;
    {
        const int rc = rotavg_setup(S, ws, g, R, is_root, forest, tree);
        if (rc < 0) return rc;
    }
    tree.cg_iters = knobs.tree_cg_iters ? knobs.tree_cg_iters : std::max<uint32_t>(prm.cg_iters, 1000u);
    if (clk.on) (void)hipStreamSynchronize(st);
    clk.mark("solve: adjacency, allocation, uploads");

    TwoLevel two;
    bool use_two = false;
    if (knobs.two_level == 2 || (knobs.two_level == 1 && !tree.ok && n_views > knobs.single_wg_views)) {
        std::vector<uint32_t> bfs_order;
        const uint32_t depth = bfs_from_gauge_views(n_views, g, is_root, bfs_order);
        if (knobs.two_level == 2 || depth >= kTwoLevelDepth) {
            const int rc = plan_and_upload_two_level(S, g, is_root, bfs_order, two);
            if (rc < 0) return rc;
            use_two = rc == 0;
        }
        if (clk.on) std::fprintf(stderr, "[rotavg timing] breadth-first depth %u, two-level %s (%u aggregates, %u rows)\n", depth, use_two ? "on" : "off",
                                 two.plan.n_agg, two.plan.n_rows);
        clk.mark("solve: two-level plan");
    }

    const double sigma = prm.sigma_deg * 3.14159265358979323846 / 180.0;
    uint32_t iters = 0;
    uint32_t predicted = 0, predicted2 = 0;  // PCG iterations of the previous outer step's solve: Jacobi, two-level
    for (uint32_t it = 0; it < prm.l1_iters + prm.irls_iters; ++it) {
        hipLaunchKernelGGL(rot_residual_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, st, d_rot, n_edges, S.R, it < prm.l1_iters ? 1 : 0, sigma,
                           S.omega, S.w);
        enum { kTwo, kTree, kSingle, kJacobi } path = kJacobi;  // the solver this step ends up with
        double cg_it = 0;                                      // its PCG iterations (trace)
        if (use_two) {
            const int rc = solve_two_level(S, two, predicted2, cg_it);
            if (rc < 0) return rc;
            if (rc == 1) use_two = false;  // a coarse matrix that could not be inverted: this graph stays with the one-level solvers
            else path = kTwo;
        }
        if (path == kTwo) {
        } else if (tree.in_use) {
            path = kTree;
        } else if (n_views <= knobs.single_wg_views) {
            path = kSingle;
            uint32_t row_lanes = 16;  // as many lanes per view as keep all views in one pass of the 1024 threads
            while (row_lanes > 1 && (uint64_t)n_views * row_lanes > 1024u) row_lanes >>= 1;
            hipLaunchKernelGGL(rot_solve_kernel, dim3(1), dim3(1024), 0, st, n_views, S.ptr, S.aedge, S.aother, S.asign, S.root, S.omega, S.w,
                               prm.cg_iters, S.cg_tol, row_lanes, S.diag, S.x, S.r[0], S.p, S.q[0], S.stats);
            if (tree.ok) {  // a solve that ran into the cap sends this graph to the tree path (see the multi-workgroup branch)
                double probe[2] = {0, 0};
                HIP_TRY(hipMemcpyAsync(probe, S.stats, sizeof probe, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (probe[1] >= (double)prm.cg_iters) path = kTree;
            }
        } else {  // multi-workgroup PCG: launches are cheap next to a one-CU solve at this size
            JacobiSolve solve(S);
            CgState hs{};
            const int done = pcg_looks(solve, st, prm.cg_iters, predicted, tree.ok, hs);
            if (done < 0) return done;
            cg_it = hs.iters;
            // not converged within the cap: the graph is sparse / sequence-like and Jacobi is the wrong preconditioner for
            // it.  This step is solved again, and all following ones, by the tree-preconditioned kernel, so that the
            // iteration follows the exact-solve trajectory from the start.
            if (!done && tree.ok) {
                path = kTree;
            } else if (!done) {  // the truncated solution is the step
                const int rc = solve.finish(nullptr);
                if (rc < 0) return rc;
                HIP_TRY(hipStreamSynchronize(st));
            }
        }
        double stats[2] = {0, 0};  // mean |d|, iterations of the one-workgroup solve
        if (path == kSingle) {
            hipLaunchKernelGGL(rot_update_kernel, dim3((n_views + 255) / 256), dim3(256), 0, st, n_views, S.x, (const uint32_t*)nullptr, S.R,
                               (const CgState*)nullptr, (const int*)nullptr);
            HIP_TRY(hipMemcpyAsync(stats, S.stats, sizeof stats, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            cg_it = stats[1];
        } else {
            if (path == kTree) {
                tree.in_use = true;
                solve_with_tree(S, tree);
                const int rc = queue_step(S, n_views, S.x, nullptr, S.norm, nullptr, nullptr);
                if (rc < 0) return rc;
                HIP_TRY(hipStreamSynchronize(st));
            }
            double sum = 0;  // mean |d| = sum / V
            for (size_t b2 = 0; b2 < S.norm_host.size(); b2 += 3) sum += S.norm_host[b2];
            stats[0] = sum / (double)n_views;
        }
        iters = it + 1;
        if (knobs.trace) {
            if (path == kTree) {
                double its[3];
                HIP_TRY(hipMemcpyAsync(its, S.its, sizeof its, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                cg_it = -std::max(its[0], std::max(its[1], its[2]));  // printed negative: tree-preconditioned iterations
            }
            std::fprintf(stderr, "[rotavg] outer %2u (%s): %3.0f PCG iterations%s, mean step %.3e rad\n", it, it < prm.l1_iters ? "L1" : "IRLS", cg_it,
                         path == kTwo ? " (two-level)" : "", stats[0]);
        }
        if (stats[0] < prm.tol) break;
    }
    clk.mark("solve: outer iterations");
    HIP_TRY(hipMemcpyAsync(h_R_out, S.R, (size_t)n_views * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    clk.mark("solve: rotations back");
    if (h_iters_out) *h_iters_out = iters;
    return PGI_SUCCESS;
}

}  // namespace pgi

using namespace pgi;

extern "C" {

void pgi_default_rotavg_params(pgi_rotavg_params* p) {
    p->l1_iters = 5;
    p->irls_iters = 100;
    p->cg_iters = 200;
    p->sigma_deg = 5.0;
    p->tol = 1e-8;
}

int pgi_rotation_average(pgi_ctx* ctx, const pgi_rot_edge* h_edges, uint32_t n_edges, uint32_t n_views,
                         const pgi_rotavg_params* prm_in, double* h_R_out, uint32_t* h_iters_out) {
    if (!ctx || !h_R_out || (n_edges && !h_edges)) return fail(PGI_ERR_INVALID, "null argument");
    pgi_rotavg_params prm;
    if (prm_in) prm = *prm_in; else pgi_default_rotavg_params(&prm);
    for (uint32_t e = 0; e < n_edges; ++e)
        if (h_edges[e].src >= n_views || h_edges[e].dst >= n_views || h_edges[e].src == h_edges[e].dst)
            return fail(PGI_ERR_INVALID, "edge endpoints out of range");
    if (n_views == 0) return PGI_SUCCESS;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const RotavgKnobs knobs = read_rotavg_knobs();
    PhaseClock clk(knobs.timing);
    std::vector<uint32_t> src(n_edges), dst(n_edges), tree;
    std::vector<double> wt(n_edges);
    for (uint32_t e = 0; e < n_edges; ++e) {
        src[e] = h_edges[e].src;
        dst[e] = h_edges[e].dst;
        wt[e] = h_edges[e].weight;
    }
    std::vector<std::vector<ForestEdge>> adj;
    spanning_forest(n_views, src.data(), dst.data(), wt.data(), n_edges, tree, adj);
    clk.mark("host edges: maximum-weight spanning forest");
    std::vector<double> R;
    std::vector<uint8_t> is_root;
    forest_bfs_init(n_views, adj, [&](uint32_t e) { return h_edges[e].R; }, R, is_root);
    clk.mark("host edges: forest initialisation");
    if (h_iters_out) *h_iters_out = 0;
    if (n_edges == 0) {
        memcpy(h_R_out, R.data(), R.size() * 8);
        return PGI_SUCCESS;
    }
    static_assert(sizeof(RotEdgeDev) == sizeof(pgi_rot_edge), "edge layout");
    RotEdgeDev* d_rot = nullptr;
    DeviceWorkspace ws;
    ws.add(d_rot, n_edges);
    HIP_TRY(ws.alloc());
    HIP_TRY(hipMemcpyAsync(d_rot, h_edges, (size_t)n_edges * sizeof(pgi_rot_edge), hipMemcpyHostToDevice, ctx->stream));
    if (clk.on) (void)hipStreamSynchronize(ctx->stream);
    clk.mark("host edges: edge table to the device");
    return rotavg_solve(ctx, knobs, prm, n_views, n_edges, src.data(), dst.data(), d_rot, R, is_root, adj, h_R_out, h_iters_out);
}

int pgi_rotation_average_edges(pgi_ctx* ctx, const pgi_edge* d_edges, const uint32_t* h_src, const uint32_t* h_dst,
                               const uint32_t* h_rows, uint32_t n_pairs, uint32_t n_views, const pgi_rotavg_params* prm_in,
                               double* h_R_out, uint32_t* h_iters_out, uint32_t* h_edges_used) {
    if (!ctx || !h_R_out || (n_pairs && (!d_edges || !h_src || !h_dst))) return fail(PGI_ERR_INVALID, "null argument");
    pgi_rotavg_params prm;
    if (prm_in) prm = *prm_in; else pgi_default_rotavg_params(&prm);
    if (h_iters_out) *h_iters_out = 0;
    if (h_edges_used) *h_edges_used = 0;
    if (n_views == 0) return PGI_SUCCESS;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const RotavgKnobs knobs = read_rotavg_knobs();
    PhaseClock clk(knobs.timing);
    // (status, n_inl) of every record: an 8-byte column of the 200-byte table
    struct Meta { int32_t status; uint32_t n_inl; };
    std::vector<Meta> meta(n_pairs);
    if (n_pairs) {
        HIP_TRY(hipMemcpy2DAsync(meta.data(), sizeof(Meta), (const char*)d_edges + offsetof(pgi_edge, status), sizeof(pgi_edge),
                                 sizeof(Meta), n_pairs, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    std::vector<uint32_t> idx, src, dst;
    std::vector<double> wt;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (meta[p].status != PGI_EDGE_OK) continue;
        if (h_src[p] >= n_views || h_dst[p] >= n_views || h_src[p] == h_dst[p])
            return fail(PGI_ERR_INVALID, "edge endpoints out of range");
        idx.push_back(p);
        src.push_back(h_src[p]);
        dst.push_back(h_dst[p]);
        wt.push_back(h_rows ? (double)meta[p].n_inl / (double)std::max<uint32_t>(1u, h_rows[p]) : 1.0);
    }
    const uint32_t nE = (uint32_t)idx.size();
    if (h_edges_used) *h_edges_used = nE;
    clk.mark("edges: status column to the host, edge list");
    std::vector<uint32_t> tree;
    std::vector<std::vector<ForestEdge>> adj;
    spanning_forest(n_views, src.data(), dst.data(), wt.data(), nE, tree, adj);
    clk.mark("edges: maximum-weight spanning forest (host)");
    std::vector<double> R;
    std::vector<uint8_t> is_root;
    if (nE == 0) {
        forest_bfs_init(n_views, adj, [&](uint32_t) { return (const double*)nullptr; }, R, is_root);
        memcpy(h_R_out, R.data(), R.size() * 8);
        return PGI_SUCCESS;
    }
    const size_t nT = tree.size();
    RotEdgeDev* d_rot;
    uint32_t *d_idx, *d_src, *d_dst, *d_tree;
    double *d_wt, *d_treeR;
    DeviceWorkspace ws;
    ws.add(d_rot, nE); ws.add(d_idx, nE); ws.add(d_src, nE); ws.add(d_dst, nE); ws.add(d_wt, nE); ws.add(d_tree, nT); ws.add(d_treeR, 9 * nT);
    HIP_TRY(ws.alloc());
    HIP_TRY(upload(d_idx, idx, st));
    HIP_TRY(upload(d_src, src, st));
    HIP_TRY(upload(d_dst, dst, st));
    HIP_TRY(upload(d_wt, wt, st));
    HIP_TRY(upload(d_tree, tree, st));
    hipLaunchKernelGGL(rot_edges_from_table_kernel, dim3((nE + 255) / 256), dim3(256), 0, st, d_edges, d_idx, d_src, d_dst, d_wt, nE, d_rot);
    hipLaunchKernelGGL(rot_gather_R_kernel, dim3(((uint32_t)nT + 255) / 256), dim3(256), 0, st, d_rot, d_tree, (uint32_t)nT, d_treeR);
    std::vector<double> treeR(nT * 9);
    HIP_TRY(hipMemcpyAsync(treeR.data(), d_treeR, treeR.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint32_t> slot(nE, 0u);  // edge -> position in the forest list
    for (size_t k = 0; k < nT; ++k) slot[tree[k]] = (uint32_t)k;
    clk.mark("edges: device edge table, forest rotations back");
    forest_bfs_init(n_views, adj, [&](uint32_t e) { return &treeR[9 * (size_t)slot[e]]; }, R, is_root);
    clk.mark("edges: forest initialisation (host)");
    return rotavg_solve(ctx, knobs, prm, n_views, nE, src.data(), dst.data(), d_rot, R, is_root, adj, h_R_out, h_iters_out);
}

}  // extern "C"
