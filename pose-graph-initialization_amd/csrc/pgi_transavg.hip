// pgi_transavg.hip -- translation averaging on the pose graph: global camera positions from the unit baseline
// directions of the edges and the averaged global rotations.
//
// NOT in the reference (like the rotation averaging of pgi_rotavg.hip).  Algorithm: robust Least Unsquared Deviations
// (Ozyesil & Singer, CVPR 2015) by joint IRLS with an active set, specified in tests/transavg_spec.py and DESIGN.md §3 item 9.
// Edge convention: (src = i, dst = j) has x_j = R_ij x_i + t_ij, so gamma_e = R_j^T t_ij (unit) is the world direction of
// c_i - c_j.  With D = c_src - c_dst and a = <D, gamma> an edge is CLAMPED where a <= 1 (cost |D - gamma|) and FREE
// otherwise (cost |(I - gamma gamma^T) D|).
//
// Data path (f64 throughout, -ffp-contract=off, no float atomics, every sum in a fixed order: same input, same bits):
//   trn_directions_kernel  one thread per edge : gamma = R_dst^T t / |.| from the device edge table (status OK records)
//   trn_model_kernel       one thread per edge : a, class, residual, omega, the six entries of omega M_e, the rhs vector
//   trn_solve_kernel       V <= 256: ONE 256-thread workgroup, a single launch: the 3V x 3V block Laplacian is applied
//                          per view over the vertex-sorted adjacency, block-Jacobi preconditioned CG (the inverse of
//                          every view's 3 x 3 diagonal block in closed form), fixed-tree block reductions
//   trn_cg_*_kernel        larger graphs: the same recurrences across the CUs, two launches per iteration; the CG scalars
//                          and the convergence flag stay on the device, every workgroup reduces the previous launch's
//                          block partials redundantly in the same order, the host looks after a predicted number of launches
//   trn_step_kernel        mean |c_new - c_old| and c += step
// The solve is for the STEP d = c_new - c (right-hand side b - A c), so the inner tolerance is relative to the step and the
// inner error vanishes with it.  Unlike the rotation solve the three coordinates are coupled through the 3 x 3 blocks.
// Multi-GPU: replicated on every rank after the all-gather of the edge records, like the rotation solve.
#include "pgi_internal.hpp"
#include "pgi_graph_host.hpp"
#include "pgi_reduce.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

namespace pgi {
namespace {
// Inner solves stop at |r|_M <= 1e-4 |r0|_M like the rotation solve's.  The active-set switch makes the outer map
// discontinuous, so what an inexact solve costs was measured on the specification: truncated CG at a
// relative residual of 1e-4 moves the positions by at most 4.8e-6 of their RMS spread on the five test graphs.
constexpr double kTrnInnerTolerance = 1e-4;
constexpr uint32_t kTrnSingleWgViews = 256;  // at or below: one workgroup, one launch per solve
constexpr int kTrnBlock = 64;                // multi-workgroup kernels: one wavefront per workgroup, one view per lane

#define TDEV __device__ __forceinline__

struct TrnEdgeDev {
    uint32_t src, dst;
    double dir[3];
    double weight;
};
static_assert(sizeof(TrnEdgeDev) == sizeof(pgi_trans_edge), "edge layout");

// y = S v for a symmetric 3 x 3 matrix stored as xx xy xz yy yz zz
TDEV void sym_mul(const double* S, const double* v, double* y) {
    y[0] = S[0] * v[0] + S[1] * v[1] + S[2] * v[2];
    y[1] = S[1] * v[0] + S[3] * v[1] + S[4] * v[2];
    y[2] = S[2] * v[0] + S[4] * v[1] + S[5] * v[2];
}
// closed-form inverse of a symmetric 3 x 3 matrix (adjugate / determinant); zero where it is not positive
TDEV void sym_inv(const double* S, double* I) {
    const double c00 = S[3] * S[5] - S[4] * S[4], c01 = S[2] * S[4] - S[1] * S[5], c02 = S[1] * S[4] - S[2] * S[3];
    const double c11 = S[0] * S[5] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[4], c22 = S[0] * S[3] - S[1] * S[1];
    const double det = S[0] * c00 + S[1] * c01 + S[2] * c02;
    const double k = det > 0.0 ? 1.0 / det : 0.0;
    I[0] = c00 * k; I[1] = c01 * k; I[2] = c02 * k; I[3] = c11 * k; I[4] = c12 * k; I[5] = c22 * k;
}

// pgi_edge records (status OK, selected by idx) -> translation-graph edges: gamma = R_dst^T t, normalised.
// bad: set when a direction is zero or not finite (every writer stores the same value).
__global__ __launch_bounds__(256) void trn_directions_kernel(const pgi_edge* __restrict__ table, const uint32_t* __restrict__ idx,
                                                             const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                                                             const double* __restrict__ weight, const double* __restrict__ Rg,
                                                             uint32_t n_edges, TrnEdgeDev* __restrict__ out, int* __restrict__ bad) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const pgi_edge* rec = table + idx[e];
    const uint32_t j = dst[e];
    const double* R = Rg + 9 * (size_t)j;
    const double t0 = rec->t[0], t1 = rec->t[1], t2 = rec->t[2];
    const double g0 = R[0] * t0 + R[3] * t1 + R[6] * t2;
    const double g1 = R[1] * t0 + R[4] * t1 + R[7] * t2;
    const double g2 = R[2] * t0 + R[5] * t1 + R[8] * t2;
    const double n = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    if (!(n > 0.0) || !(n < 1.7e308)) *bad = 1;
    TrnEdgeDev o;
    o.src = src[e];
    o.dst = j;
    o.dir[0] = g0 / n; o.dir[1] = g1 / n; o.dir[2] = g2 / n;
    o.weight = weight[e];
    out[e] = o;
}
// directions of selected edges (the spanning forest's) -> a dense array for the host
__global__ __launch_bounds__(256) void trn_gather_dir_kernel(const TrnEdgeDev* __restrict__ edges, const uint32_t* __restrict__ sel,
                                                             uint32_t n_sel, double* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const TrnEdgeDev* e = edges + sel[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * (size_t)k + c] = e->dir[c];
}

// per edge: class, residual, weight; P = omega M_e (xx xy xz yy yz zz), g = omega lambda tau gamma
__global__ __launch_bounds__(256) void trn_model_kernel(const TrnEdgeDev* __restrict__ edges, uint32_t n_edges,
                                                        const double* __restrict__ c, double eps, double delta,
                                                        double* __restrict__ P, double* __restrict__ g,
                                                        unsigned int* __restrict__ n_clamped) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    int clamped = 0;
    if (e < n_edges) {
        const TrnEdgeDev ed = edges[e];
        double D[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) D[k] = c[3 * (size_t)ed.src + k] - c[3 * (size_t)ed.dst + k];
        const double a = D[0] * ed.dir[0] + D[1] * ed.dir[1] + D[2] * ed.dir[2];
        clamped = a <= 1.0;
        const double tau = clamped ? 1.0 : a, lam = clamped ? 1.0 : eps;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = D[k] - tau * ed.dir[k];
        const double r = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        const double om = ed.weight / fmax(r, delta);
        const double s = om * (lam - 1.0);  // omega M = omega I + omega (lambda - 1) gamma gamma^T
        const double x = ed.dir[0], y = ed.dir[1], z = ed.dir[2];
        double* Pe = P + 6 * (size_t)e;
        Pe[0] = om + s * (x * x); Pe[1] = s * (x * y); Pe[2] = s * (x * z);
        Pe[3] = om + s * (y * y); Pe[4] = s * (y * z); Pe[5] = om + s * (z * z);
        const double h = om * lam * tau;
        g[3 * (size_t)e] = h * x; g[3 * (size_t)e + 1] = h * y; g[3 * (size_t)e + 2] = h * z;
    }
    const int cnt = __syncthreads_count(clamped);  // an integer count for the trace: any order gives the same value
    if (threadIdx.x == 0 && cnt) atomicAdd(n_clamped, (unsigned int)cnt);
}

// One view's row of the system from the adjacency: diagonal block D = sum P_e, right-hand side of the STEP
// b - A c = sum_e (sign g_e - P_e (c_v - c_other)); sign +1: the view is the edge's src.
TDEV void view_row(uint32_t v, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj_edge,
                   const uint32_t* __restrict__ adj_other, const int8_t* __restrict__ adj_sign, const double* __restrict__ P,
                   const double* __restrict__ g, const double* __restrict__ c, double* D, double* rhs) {
#pragma unroll
    for (int k = 0; k < 6; ++k) D[k] = 0.0;
    rhs[0] = rhs[1] = rhs[2] = 0.0;
    const double cv[3] = {c[3 * (size_t)v], c[3 * (size_t)v + 1], c[3 * (size_t)v + 2]};
    for (uint32_t a = adj_ptr[v]; a < adj_ptr[v + 1]; ++a) {
        const uint32_t e = adj_edge[a], o = adj_other[a];
        const double sg = (double)adj_sign[a];
        double Pe[6], d[3], y[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) Pe[k] = P[6 * (size_t)e + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = cv[k] - c[3 * (size_t)o + k];
        sym_mul(Pe, d, y);
#pragma unroll
        for (int k = 0; k < 6; ++k) D[k] += Pe[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) rhs[k] += sg * g[3 * (size_t)e + k] - y[k];
    }
}
// (A p)_v = sum_e P_e (p_v - p_other); pv: the view's own entries, p_of(o, out): a neighbour's
template <class POf>
TDEV void view_product(uint32_t v, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj_edge,
                       const uint32_t* __restrict__ adj_other, const double* __restrict__ P, const double* pv, POf p_of, double* y) {
    y[0] = y[1] = y[2] = 0.0;
    for (uint32_t a = adj_ptr[v]; a < adj_ptr[v + 1]; ++a) {
        const uint32_t e = adj_edge[a];
        double Pe[6], po[3], d[3], t[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) Pe[k] = P[6 * (size_t)e + k];
        p_of(adj_other[a], po);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = pv[k] - po[k];
        sym_mul(Pe, d, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) y[k] += t[k];
    }
}

// ---- small graphs: the whole solve in one workgroup, thread v owns view v (its vectors stay in registers; the search
// direction is shared through LDS).  stats: [1] = PCG iterations.
__global__ __launch_bounds__(256) void trn_solve_kernel(uint32_t n_views, const uint32_t* __restrict__ adj_ptr,
                                                        const uint32_t* __restrict__ adj_edge, const uint32_t* __restrict__ adj_other,
                                                        const int8_t* __restrict__ adj_sign, const uint8_t* __restrict__ is_root,
                                                        const double* __restrict__ P, const double* __restrict__ g,
                                                        const double* __restrict__ c, uint32_t cg_iters, double cg_tol,
                                                        double* __restrict__ x_out, double* __restrict__ stats) {
    __shared__ double red[256];
    __shared__ double pl[3 * 256];
    const int tid = threadIdx.x;
    const uint32_t v = (uint32_t)tid;
    const bool live = v < n_views && !is_root[v];  // gauge views and the padding lanes hold zeros throughout
    double Dinv[6] = {0, 0, 0, 0, 0, 0}, r[3] = {0, 0, 0}, x[3] = {0, 0, 0}, p[3] = {0, 0, 0}, z[3], q[3];
    if (live) {
        double D[6];
        view_row(v, adj_ptr, adj_edge, adj_other, adj_sign, P, g, c, D, r);
        sym_inv(D, Dinv);
    }
    sym_mul(Dinv, r, z);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = z[k];
    double rz = block_tree_sum<256>(r[0] * z[0] + r[1] * z[1] + r[2] * z[2], red, tid);
    const double rz0 = rz;
    uint32_t it = 0;
    for (; it < cg_iters; ++it) {
        if (!(rz > cg_tol * cg_tol * rz0)) break;  // uniform: rz is identical in every thread
#pragma unroll
        for (int k = 0; k < 3; ++k) pl[3 * tid + k] = p[k];
        __syncthreads();
        q[0] = q[1] = q[2] = 0.0;
        if (live)
            view_product(v, adj_ptr, adj_edge, adj_other, P, p,
                         [&](uint32_t o, double* po) { po[0] = pl[3 * o]; po[1] = pl[3 * o + 1]; po[2] = pl[3 * o + 2]; }, q);
        const double pAp = block_tree_sum<256>(p[0] * q[0] + p[1] * q[1] + p[2] * q[2], red, tid);  // (its barriers also retire pl)
        const double alpha = pAp > 0.0 ? rz / pAp : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] += alpha * p[k];
            r[k] -= alpha * q[k];
        }
        sym_mul(Dinv, r, z);
        const double rzn = block_tree_sum<256>(r[0] * z[0] + r[1] * z[1] + r[2] * z[2], red, tid);
        const double beta = rz > 0.0 ? rzn / rz : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = z[k] + beta * p[k];
        rz = rzn;
    }
    if (v < n_views)
#pragma unroll
        for (int k = 0; k < 3; ++k) x_out[3 * (size_t)v + k] = x[k];
    if (tid == 0) stats[1] = (double)it;
}

// ---- larger graphs: the same recurrences, one view per lane of one-wavefront workgroups.  Two launches per iteration
// (the kernel boundary is the grid-wide synchronisation), the scalars on the device:
//   direction launch: reduces the r.z partials of the previous launch -> beta and the stopping test; p' = z + beta p
//                     (a neighbour's p' is rebuilt from z and the OLD p, which is why p is double-buffered); q = A p';
//                     writes the p.q partials and the next state record
//   update launch   : reduces the p.q partials -> alpha; x += alpha p, r -= alpha q, z = Dinv r; writes the r.z partials
// Every workgroup reduces the partials itself, in the same order, so all hold the same bits.  Once the state says
// "done" both launches return at once: WHERE the host looks changes no bit of the result.
struct TrnCgState {
    double rz, rz0, iters;
    int done, pad;
};
__global__ __launch_bounds__(kTrnBlock) void trn_cg_init_kernel(uint32_t n_views, const uint32_t* __restrict__ adj_ptr,
                                                                const uint32_t* __restrict__ adj_edge, const uint32_t* __restrict__ adj_other,
                                                                const int8_t* __restrict__ adj_sign, const uint8_t* __restrict__ is_root,
                                                                const double* __restrict__ P, const double* __restrict__ g,
                                                                const double* __restrict__ c, double* __restrict__ Dinv_out,
                                                                double* __restrict__ x, double* __restrict__ r_out, double* __restrict__ z_out,
                                                                double* __restrict__ p0, double* __restrict__ part_rz,
                                                                TrnCgState* __restrict__ st) {
    const int tid = threadIdx.x;
    const uint32_t v = blockIdx.x * kTrnBlock + (uint32_t)tid;
    double Dinv[6] = {0, 0, 0, 0, 0, 0}, r[3] = {0, 0, 0}, z[3];
    if (v < n_views && !is_root[v]) {
        double D[6];
        view_row(v, adj_ptr, adj_edge, adj_other, adj_sign, P, g, c, D, r);
        sym_inv(D, Dinv);
    }
    sym_mul(Dinv, r, z);
    if (v < n_views) {
#pragma unroll
        for (int k = 0; k < 6; ++k) Dinv_out[6 * (size_t)v + k] = Dinv[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t i = 3 * (size_t)v + k;
            x[i] = 0.0;
            r_out[i] = r[k];
            z_out[i] = z[k];
            p0[i] = 0.0;
        }
    }
    const double s = wave_sum(r[0] * z[0] + r[1] * z[1] + r[2] * z[2]);
    if (tid == 0) part_rz[blockIdx.x] = s;
    if (blockIdx.x == 0 && tid == 0) *st = TrnCgState{0.0, 0.0, 0.0, 0, 0};
}

__global__ __launch_bounds__(kTrnBlock) void trn_cg_direction_kernel(uint32_t n_views, const uint32_t* __restrict__ adj_ptr,
                                                                     const uint32_t* __restrict__ adj_edge,
                                                                     const uint32_t* __restrict__ adj_other, const uint8_t* __restrict__ is_root,
                                                                     const double* __restrict__ P, const double* __restrict__ z,
                                                                     const double* __restrict__ p_old, double* __restrict__ p_new,
                                                                     double* __restrict__ q, const double* __restrict__ part_rz,
                                                                     double* __restrict__ part_pq, uint32_t n_blocks, int first, double tol,
                                                                     const TrnCgState* __restrict__ st_prev, TrnCgState* __restrict__ st_next) {
    const int tid = threadIdx.x;
    const TrnCgState sp = *st_prev;
    if (sp.done) {  // (uniform) converged earlier: keep the record where the host reads it
        if (blockIdx.x == 0 && tid == 0) *st_next = sp;
        return;
    }
    const double rz = wave_sum(strided_sum<kTrnBlock>(part_rz, n_blocks, 1, tid));
    const double rz0 = first ? rz : sp.rz0;
    const double beta = (!first && sp.rz > 0.0) ? rz / sp.rz : 0.0;
    const bool done = !(rz > tol * tol * rz0);
    if (blockIdx.x == 0 && tid == 0) *st_next = TrnCgState{rz, rz0, done ? sp.iters : sp.iters + 1.0, done ? 1 : 0, 0};
    if (done) return;  // (uniform)
    const uint32_t v = blockIdx.x * kTrnBlock + (uint32_t)tid;
    double pv[3] = {0, 0, 0}, y[3] = {0, 0, 0};
    if (v < n_views) {
#pragma unroll
        for (int k = 0; k < 3; ++k) pv[k] = z[3 * (size_t)v + k] + beta * p_old[3 * (size_t)v + k];
        if (!is_root[v])
            view_product(v, adj_ptr, adj_edge, adj_other, P, pv,
                         [&](uint32_t o, double* po) {
#pragma unroll
                             for (int k = 0; k < 3; ++k) po[k] = z[3 * (size_t)o + k] + beta * p_old[3 * (size_t)o + k];
                         },
                         y);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p_new[3 * (size_t)v + k] = pv[k];
            q[3 * (size_t)v + k] = y[k];
        }
    }
    const double s = wave_sum(pv[0] * y[0] + pv[1] * y[1] + pv[2] * y[2]);
    if (tid == 0) part_pq[blockIdx.x] = s;
}

__global__ __launch_bounds__(kTrnBlock) void trn_cg_update_kernel(uint32_t n_views, const double* __restrict__ Dinv,
                                                                  const double* __restrict__ p, const double* __restrict__ q,
                                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                  const double* __restrict__ part_pq, double* __restrict__ part_rz,
                                                                  uint32_t n_blocks, const TrnCgState* __restrict__ st) {
    const int tid = threadIdx.x;
    const TrnCgState s = *st;
    if (s.done) return;  // (uniform)
    const double pq = wave_sum(strided_sum<kTrnBlock>(part_pq, n_blocks, 1, tid));
    const double alpha = pq > 0.0 ? s.rz / pq : 0.0;
    const uint32_t v = blockIdx.x * kTrnBlock + (uint32_t)tid;
    double rn[3] = {0, 0, 0}, zn[3] = {0, 0, 0};
    if (v < n_views) {
        double Di[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) Di[k] = Dinv[6 * (size_t)v + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t i = 3 * (size_t)v + k;
            x[i] += alpha * p[i];
            rn[k] = r[i] - alpha * q[i];
        }
        sym_mul(Di, rn, zn);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[3 * (size_t)v + k] = rn[k];
            z[3 * (size_t)v + k] = zn[k];
        }
    }
    const double t = wave_sum(rn[0] * zn[0] + rn[1] * zn[1] + rn[2] * zn[2]);
    if (tid == 0) part_rz[blockIdx.x] = t;
}

// c += x and stats[0] = mean |x_v| : one workgroup strides over the views (fixed order)
__global__ __launch_bounds__(256) void trn_step_kernel(uint32_t n_views, const double* __restrict__ x, double* __restrict__ c,
                                                       double* __restrict__ stats) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (uint32_t v = (uint32_t)tid; v < n_views; v += 256) {
        const double a = x[3 * (size_t)v], b = x[3 * (size_t)v + 1], d = x[3 * (size_t)v + 2];
        s += sqrt(a * a + b * b + d * d);
        c[3 * (size_t)v] += a;
        c[3 * (size_t)v + 1] += b;
        c[3 * (size_t)v + 2] += d;
    }
    s = block_tree_sum<256>(s, red, tid);
    if (tid == 0) stats[0] = s / (double)n_views;
}

// ---- host: BFS initialisation over the maximum-weight spanning forest (spanning_forest of pgi_graph_host.hpp: the forest and
// the roots of the rotation averaging -- Kruskal over (weight desc, edge index asc), roots = the smallest view of every
// component.  The weights that reach it here are finite and not negative: the entry points see to that.) ----------------------
// c_root = 0; along a tree edge c_dst = c_src - gamma, walked backwards c_src = c_dst + gamma.  dir_of(e): 3 doubles.
template <class DirOf>
void trn_forest_init(uint32_t V, const std::vector<std::vector<ForestEdge>>& adj, DirOf dir_of, std::vector<double>& c,
                     std::vector<uint8_t>& is_root) {
    c.assign((size_t)V * 3, 0.0);
    is_root.assign(V, 0);
    std::vector<uint8_t> seen(V, 0);
    std::vector<uint32_t> queue;
    for (uint32_t root = 0; root < V; ++root) {
        if (seen[root]) continue;
        seen[root] = 1;
        is_root[root] = 1;
        queue.assign(1, root);
        for (size_t h = 0; h < queue.size(); ++h) {
            const uint32_t u = queue[h];
            for (const ForestEdge& pr : adj[u]) {
                const uint32_t v = pr.other & 0x7FFFFFFFu;
                if (seen[v]) continue;
                seen[v] = 1;
                const double* gm = dir_of(pr.edge);
                const bool back = pr.other >> 31;  // u is the edge's dst, v its src
                for (int k = 0; k < 3; ++k) c[3 * (size_t)v + k] = back ? c[3 * (size_t)u + k] + gm[k] : c[3 * (size_t)u + k] - gm[k];
                queue.push_back(v);
            }
        }
    }
}

// The solve proper.  The edges are in HBM at d_trn; the host holds their endpoints, the initial positions and the roots.
int transavg_solve(pgi_ctx* ctx, const pgi_transavg_params& prm, uint32_t n_views, uint32_t n_edges, const uint32_t* h_src,
                   const uint32_t* h_dst, const TrnEdgeDev* d_trn, const std::vector<double>& c0, const std::vector<uint8_t>& is_root,
                   double* h_c_out, uint32_t* h_iters_out) {
    const IncidenceCsr adj = build_incidence_csr(n_views, n_edges, h_src, h_dst, +1);  // sign +1: the view is the edge's src
    const size_t V = n_views, E = n_edges;
    const uint32_t n_blocks = (n_views + kTrnBlock - 1) / kTrnBlock;
    double *d_c, *d_P, *d_g, *d_Dinv, *d_x, *d_r, *d_z, *d_pbuf[2], *d_q, *d_prz, *d_ppq, *d_stats;
    uint32_t *d_ptr, *d_aedge, *d_aother;
    int8_t* d_asign;
    uint8_t* d_root;
    TrnCgState* d_st;
    unsigned int* d_cnt;
    DeviceWorkspace ws;
    ws.add(d_c, 3 * V); ws.add(d_ptr, V + 1); ws.add(d_aedge, 2 * E); ws.add(d_aother, 2 * E); ws.add(d_asign, 2 * E); ws.add(d_root, V);
    ws.add(d_P, 6 * E); ws.add(d_g, 3 * E); ws.add(d_Dinv, 6 * V); ws.add(d_x, 3 * V); ws.add(d_r, 3 * V); ws.add(d_z, 3 * V);
    ws.add(d_pbuf[0], 3 * V); ws.add(d_pbuf[1], 3 * V); ws.add(d_q, 3 * V); ws.add(d_prz, n_blocks); ws.add(d_ppq, n_blocks);
    ws.add(d_st, 2); ws.add(d_stats, 2); ws.add(d_cnt, 1);
    HIP_TRY(ws.alloc());
    hipStream_t st = ctx->stream;
    HIP_TRY(upload(d_c, c0, st));
    HIP_TRY(upload(d_ptr, adj.ptr, st));
    HIP_TRY(upload(d_aedge, adj.edge, st));
    HIP_TRY(upload(d_aother, adj.other, st));
    HIP_TRY(upload(d_asign, adj.sign, st));
    HIP_TRY(upload(d_root, is_root, st));

    const bool trace = std::getenv("PGI_TRANSAVG_TRACE") != nullptr;
    double cg_tol = kTrnInnerTolerance;
    if (const char* e = std::getenv("PGI_TRANSAVG_CG_TOL")) {
        const double t = std::atof(e);
        if (t > 0.0 && t < 1.0) cg_tol = t;
    }
    const uint32_t cap = std::max<uint32_t>(1u, prm.cg_iters);
    const bool single = n_views <= kTrnSingleWgViews;
    uint32_t iters = 0, predicted = 0;
    for (uint32_t it = 0; it < prm.iters; ++it) {
        HIP_TRY(hipMemsetAsync(d_cnt, 0, 4, st));
        hipLaunchKernelGGL(trn_model_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, st, d_trn, n_edges, d_c, prm.eps, prm.delta, d_P,
                           d_g, d_cnt);
        double cg_done = 0.0;
        if (single) {
            hipLaunchKernelGGL(trn_solve_kernel, dim3(1), dim3(256), 0, st, n_views, d_ptr, d_aedge, d_aother, d_asign, d_root, d_P,
                               d_g, d_c, cap, cg_tol, d_x, d_stats);
        } else {
            hipLaunchKernelGGL(trn_cg_init_kernel, dim3(n_blocks), dim3(kTrnBlock), 0, st, n_views, d_ptr, d_aedge, d_aother, d_asign,
                               d_root, d_P, d_g, d_c, d_Dinv, d_x, d_r, d_z, d_pbuf[0], d_prz, d_st);
            // The host looks at the state record between chunks of iterations (each look a round trip): first after what
            // the previous outer step's solve needed plus two (consecutive systems differ by their weights only), then every 16.
            uint32_t ci = 0;
            int par = 0;  // d_st[par]: the record the next direction launch reads; d_pbuf[par]: the old search direction
            TrnCgState hs{};
            while (ci < cap) {
                const uint32_t target = std::min<uint32_t>(cap, ci + (ci == 0 ? std::max<uint32_t>(16u, predicted + 2u) : 16u));
                for (; ci < target; ++ci) {
                    hipLaunchKernelGGL(trn_cg_direction_kernel, dim3(n_blocks), dim3(kTrnBlock), 0, st, n_views, d_ptr, d_aedge, d_aother,
                                       d_root, d_P, d_z, d_pbuf[par], d_pbuf[par ^ 1], d_q, d_prz, d_ppq, n_blocks, ci == 0 ? 1 : 0, cg_tol,
                                       d_st + par, d_st + (par ^ 1));
                    hipLaunchKernelGGL(trn_cg_update_kernel, dim3(n_blocks), dim3(kTrnBlock), 0, st, n_views, d_Dinv, d_pbuf[par ^ 1], d_q, d_x,
                                       d_r, d_z, d_ppq, d_prz, n_blocks, d_st + (par ^ 1));
                    par ^= 1;
                }
                HIP_TRY(hipMemcpyAsync(&hs, d_st + par, sizeof hs, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (hs.done) break;
            }
            cg_done = hs.iters;
            predicted = (uint32_t)hs.iters;
        }
        hipLaunchKernelGGL(trn_step_kernel, dim3(1), dim3(256), 0, st, n_views, d_x, d_c, d_stats);
        double stats[2] = {0, 0};
        unsigned int n_clamped = 0;
        HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof stats, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&n_clamped, d_cnt, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipGetLastError());
        iters = it + 1;
        if (trace)  // PGI_TRANSAVG_TRACE=1: one line per outer iteration
            std::fprintf(stderr, "[transavg] outer %2u: %3.0f PCG iterations, %u of %u edges clamped, mean step %.3e\n", it,
                         single ? stats[1] : cg_done, n_clamped, n_edges, stats[0]);
        if (stats[0] < prm.tol) break;
    }
    HIP_TRY(hipMemcpyAsync(h_c_out, d_c, 3 * V * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_iters_out) *h_iters_out = iters;
    return PGI_SUCCESS;
}

bool params_ok(const pgi_transavg_params& p) {
    return p.eps > 0.0 && p.eps <= 1.0 && p.delta > 0.0 && std::isfinite(p.delta) && p.tol >= 0.0;
}
}  // namespace
}  // namespace pgi

using namespace pgi;

extern "C" {

void pgi_default_transavg_params(pgi_transavg_params* p) {
    p->iters = 60;
    p->cg_iters = 200;
    p->eps = 1e-3;
    p->delta = 1e-4;
    p->tol = 1e-9;
}

int pgi_translation_average(pgi_ctx* ctx, const pgi_trans_edge* h_edges, uint32_t n_edges, uint32_t n_views,
                            const pgi_transavg_params* prm_in, double* h_c_out, uint32_t* h_iters_out) {
    if (!ctx || (n_views && !h_c_out) || (n_edges && !h_edges)) return fail(PGI_ERR_INVALID, "null argument");
    pgi_transavg_params prm;
    if (prm_in) prm = *prm_in; else pgi_default_transavg_params(&prm);
    if (!params_ok(prm)) return fail(PGI_ERR_INVALID, "translation averaging parameters out of range");
    if (h_iters_out) *h_iters_out = 0;
    std::vector<TrnEdgeDev> edges(n_edges);
    std::vector<uint32_t> src(n_edges), dst(n_edges);
    std::vector<double> wt(n_edges);
    for (uint32_t e = 0; e < n_edges; ++e) {
        const pgi_trans_edge& he = h_edges[e];
        if (he.src >= n_views || he.dst >= n_views || he.src == he.dst) return fail(PGI_ERR_INVALID, "edge endpoints out of range");
        const double n2 = he.dir[0] * he.dir[0] + he.dir[1] * he.dir[1] + he.dir[2] * he.dir[2];
        if (!(n2 > 0.0) || !std::isfinite(n2)) return fail(PGI_ERR_INVALID, "edge direction zero or not finite");
        if (!std::isfinite(he.weight) || he.weight < 0.0) return fail(PGI_ERR_INVALID, "edge weight negative or not finite");
        TrnEdgeDev& o = edges[e];
        o.src = src[e] = he.src;
        o.dst = dst[e] = he.dst;
        o.weight = wt[e] = he.weight;
        // a direction that is already of unit length is taken as it is (dividing again would move its last bits)
        const bool unit = std::fabs(n2 - 1.0) <= 1e-12;
        const double n = std::sqrt(n2);
        for (int k = 0; k < 3; ++k) o.dir[k] = unit ? he.dir[k] : he.dir[k] / n;
    }
    if (n_views == 0) return PGI_SUCCESS;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint32_t> tree;
    std::vector<std::vector<ForestEdge>> adj;
    spanning_forest(n_views, src.data(), dst.data(), wt.data(), n_edges, tree, adj);
    std::vector<double> c0;
    std::vector<uint8_t> is_root;
    trn_forest_init(n_views, adj, [&](uint32_t e) { return (const double*)edges[e].dir; }, c0, is_root);
    if (n_edges == 0) {
        memcpy(h_c_out, c0.data(), c0.size() * 8);  // all zero
        return PGI_SUCCESS;
    }
    TrnEdgeDev* d_trn = nullptr;
    DeviceWorkspace ws;
    ws.add(d_trn, n_edges);
    HIP_TRY(ws.alloc());
    HIP_TRY(upload(d_trn, edges, ctx->stream));
    return transavg_solve(ctx, prm, n_views, n_edges, src.data(), dst.data(), d_trn, c0, is_root, h_c_out, h_iters_out);
}

int pgi_translation_average_edges(pgi_ctx* ctx, const pgi_edge* d_edges, const uint32_t* h_src, const uint32_t* h_dst,
                                  const uint32_t* h_rows, uint32_t n_pairs, uint32_t n_views, const double* h_R_global,
                                  const pgi_transavg_params* prm_in, double* h_c_out, uint32_t* h_iters_out,
                                  uint32_t* h_edges_used) {
    if (!ctx || (n_views && !h_c_out) || (n_pairs && (!d_edges || !h_src || !h_dst || !h_R_global)))
        return fail(PGI_ERR_INVALID, "null argument");
    pgi_transavg_params prm;
    if (prm_in) prm = *prm_in; else pgi_default_transavg_params(&prm);
    if (!params_ok(prm)) return fail(PGI_ERR_INVALID, "translation averaging parameters out of range");
    if (h_iters_out) *h_iters_out = 0;
    if (h_edges_used) *h_edges_used = 0;
    if (n_views == 0) return PGI_SUCCESS;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
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
    std::vector<uint32_t> tree;
    std::vector<std::vector<ForestEdge>> adj;
    spanning_forest(n_views, src.data(), dst.data(), wt.data(), nE, tree, adj);
    std::vector<double> c0;
    std::vector<uint8_t> is_root;
    if (nE == 0) {
        memset(h_c_out, 0, (size_t)n_views * 3 * sizeof(double));
        return PGI_SUCCESS;
    }
    const size_t nT = tree.size(), V = n_views;
    TrnEdgeDev* d_trn;
    uint32_t *d_idx, *d_src, *d_dst, *d_tree;
    double *d_wt, *d_R, *d_treeD;
    int* d_bad;
    DeviceWorkspace ws;
    ws.add(d_trn, nE); ws.add(d_idx, nE); ws.add(d_src, nE); ws.add(d_dst, nE); ws.add(d_wt, nE); ws.add(d_R, 9 * V); ws.add(d_tree, nT);
    ws.add(d_treeD, 3 * nT); ws.add(d_bad, 1);
    HIP_TRY(ws.alloc());
    HIP_TRY(upload(d_idx, idx, st));
    HIP_TRY(upload(d_src, src, st));
    HIP_TRY(upload(d_dst, dst, st));
    HIP_TRY(upload(d_wt, wt, st));
    HIP_TRY(hipMemcpyAsync(d_R, h_R_global, 9 * V * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(upload(d_tree, tree, st));
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), st));
    hipLaunchKernelGGL(trn_directions_kernel, dim3((nE + 255) / 256), dim3(256), 0, st, d_edges, d_idx, d_src, d_dst, d_wt, d_R, nE, d_trn, d_bad);
    hipLaunchKernelGGL(trn_gather_dir_kernel, dim3(((uint32_t)nT + 255) / 256), dim3(256), 0, st, d_trn, d_tree, (uint32_t)nT, d_treeD);
    std::vector<double> treeD(nT * 3);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(treeD.data(), d_treeD, treeD.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(PGI_ERR_INVALID, "edge direction zero or not finite");
    std::vector<uint32_t> slot(nE, 0u);  // edge -> position in the forest list
    for (size_t k = 0; k < nT; ++k) slot[tree[k]] = (uint32_t)k;
    trn_forest_init(n_views, adj, [&](uint32_t e) { return (const double*)&treeD[3 * (size_t)slot[e]]; }, c0, is_root);
    return transavg_solve(ctx, prm, n_views, nE, src.data(), dst.data(), d_trn, c0, is_root, h_c_out, h_iters_out);
}

}  // extern "C"
