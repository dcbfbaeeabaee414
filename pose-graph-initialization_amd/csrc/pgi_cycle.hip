// pgi_cycle.hip -- cycle-consistency edge filter: loop closure over view triplets before the averaging solves.
//
// NOT in the reference (like the averaging of pgi_rotavg.hip / pgi_transavg.hip).  The rule is specified in
// tests/cycle_spec.py and DESIGN.md §3 item 12: a triangle a < b < c of OK records is GOOD when the loop rotation
// R_ac R_cb R_ba is within rot_thr of the identity and -- unless the three centres are nearly collinear -- the three
// baseline directions, taken to frame a, are coplanar within trn_thr and close with positive scales.  An OK record is kept
// when at least min_good good triangles contain it (or none at all contains it and keep_untested is set).
//
// Data path:
//   host                    CSR of the OK records from h_src / h_dst and the 4-byte status column of the device table:
//                           every view's neighbours sorted by view id, each entry with its pair index and orientation;
//                           the work list = the entries (a, b) with a < b, i.e. every OK pair once
//   cyc_triangles_kernel    one wavefront per OK pair (a, b): the part of b's list above b and the part of a's list above b
//                           (it starts right behind b's own entry) are intersected -- the lanes stride over the shorter part
//                           and look every element up in the longer by binary search, so a hub of thousands of neighbours
//                           costs its partners a logarithm and itself no more than 64 lanes can share.  Every triangle is
//                           found exactly once, from its lowest pair, and evaluated by the lane that found it in f64
//                           straight from the 200-byte records (-ffp-contract=off: the specification's operations one by
//                           one).  n_tri / n_good of (a, c) and (b, c) by integer atomics; those of (a, b) and the three
//                           totals are summed over the wavefront first, one atomic each.  Integer sums: the result does not
//                           depend on the order of execution.
//   cyc_finalize_kernel     one thread per pair: the keep rule, the byte mask, PGI_EDGE_INCONSISTENT into the output table,
//                           the OK / dropped totals (one atomic pair per workgroup)
#include "pgi_internal.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace pgi {
namespace {

#define CDEV __device__ __forceinline__

struct CycThresholds {
    double rot_min;  // 1 + 2 cos(rot_thr)
    double s2_trn;   // sin^2(trn_thr)
    double s2_col;   // sin^2(collinear_thr)
};

// what the triangle kernel adds up; the head of pgi_cycle_summary
struct CycTotals {
    unsigned long long triangles, good, skipped;
    uint32_t n_ok, n_dropped;
};
static_assert(sizeof(CycTotals) == sizeof(pgi_cycle_summary), "summary layout");
static_assert(offsetof(pgi_cycle_summary, n_ok) == offsetof(CycTotals, n_ok), "summary layout");

struct CycPose {
    double R[9], t[3];
};

CDEV double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
CDEV void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
CDEV void matvec3(const double* A, const double* x, double* y) {
    for (int i = 0; i < 3; ++i) y[i] = (A[3 * i] * x[0] + A[3 * i + 1] * x[1]) + A[3 * i + 2] * x[2];
}
CDEV void matmul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
CDEV void transpose3(const double* A, double* T) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * j + i];
}

// the record's pose as stored, or inverted: (R^T, -(R^T t))
CDEV void directed_pose(const pgi_edge* __restrict__ rec, bool invert, CycPose& o) {
    if (!invert) {
        for (int k = 0; k < 9; ++k) o.R[k] = rec->R[k];
        for (int k = 0; k < 3; ++k) o.t[k] = rec->t[k];
        return;
    }
    double R[9], t[3], y[3];
    for (int k = 0; k < 9; ++k) R[k] = rec->R[k];
    for (int k = 0; k < 3; ++k) t[k] = rec->t[k];
    transpose3(R, o.R);
    matvec3(o.R, t, y);
    for (int k = 0; k < 3; ++k) o.t[k] = -y[k];
}

// bit 0: good, bit 1: the translation test was skipped (tests/cycle_spec.py: triangle_quantities, judge)
CDEV uint32_t judge_triangle(const CycPose& ba, const CycPose& cb, const CycPose& ac, const CycThresholds& thr) {
    double M[9], L[9];
    matmul3(ac.R, cb.R, M);
    matmul3(M, ba.R, L);
    const double trace = (L[0] + L[4]) + L[8];
    double Rab[9], Rbc[9], u1[3], u2[3], w[3], n[3], x[3];
    transpose3(ba.R, Rab);
    transpose3(cb.R, Rbc);
    matvec3(Rab, ba.t, u1);
    matvec3(Rbc, cb.t, w);
    matvec3(Rab, w, u2);
    const double* u3 = ac.t;
    cross3(u1, u2, n);
    const double n2 = dot3(n, n);
    bool good = trace >= thr.rot_min;
    const bool skipped = n2 < thr.s2_col;
    if (!skipped) {
        const double un = dot3(u3, n);
        cross3(u2, u3, x);
        const double o1 = dot3(x, n);
        cross3(u3, u1, x);
        const double o2 = dot3(x, n);
        good = good && un * un <= thr.s2_trn * n2 && o1 > 0.0 && o2 > 0.0;
    }
    return (good ? 1u : 0u) | (skipped ? 2u : 0u);
}

CDEV uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// adj_ptr [V + 1], adj_above [V] (first position of v's list with a neighbour above v), adj_nbr / adj_pe [2 E]
// (pe = pair << 1 | 1 when the record is stored as (list owner -> neighbour)), work_a / work_pos [n_work]: the owner a and
// the position of b in a's list for every OK pair a < b.
__global__ __launch_bounds__(256) void cyc_triangles_kernel(const pgi_edge* __restrict__ table, const uint32_t* __restrict__ adj_ptr,
                                                            const uint32_t* __restrict__ adj_above, const uint32_t* __restrict__ adj_nbr,
                                                            const uint32_t* __restrict__ adj_pe, const uint32_t* __restrict__ work_a,
                                                            const uint32_t* __restrict__ work_pos, uint32_t n_work, CycThresholds thr,
                                                            uint32_t* __restrict__ n_tri, uint32_t* __restrict__ n_good,
                                                            CycTotals* __restrict__ totals) {
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wave >= n_work) return;  // (the whole wavefront)
    const uint32_t a = work_a[wave], pos = work_pos[wave];
    const uint32_t b = adj_nbr[pos], pe_ab = adj_pe[pos];
    const uint32_t a0 = pos + 1, a1 = adj_ptr[a + 1];        // a's neighbours above b
    const uint32_t b0 = adj_above[b], b1 = adj_ptr[b + 1];   // b's neighbours above b
    const bool a_short = a1 - a0 <= b1 - b0;
    const uint32_t s0 = a_short ? a0 : b0, s1 = a_short ? a1 : b1, l0 = a_short ? b0 : a0, l1 = a_short ? b1 : a1;
    uint32_t c_tri = 0, c_good = 0, c_skip = 0;
    if (s0 < s1 && l0 < l1) {
        CycPose ba;
        bool have_ba = false;
        for (uint32_t i = s0 + lane; i < s1; i += 64u) {
            const uint32_t c = adj_nbr[i];
            uint32_t lo = l0, hi = l1;  // first position of the longer part that is not below c
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (adj_nbr[mid] < c) lo = mid + 1; else hi = mid;
            }
            if (lo >= l1 || adj_nbr[lo] != c) continue;
            const uint32_t pe_ac = adj_pe[a_short ? i : lo], pe_bc = adj_pe[a_short ? lo : i];
            if (!have_ba) {
                directed_pose(&table[pe_ab >> 1], !(pe_ab & 1u), ba);  // b <- a: as stored when the record is (a -> b)
                have_ba = true;
            }
            CycPose cb, ac;
            directed_pose(&table[pe_bc >> 1], !(pe_bc & 1u), cb);      // c <- b: as stored when the record is (b -> c)
            directed_pose(&table[pe_ac >> 1], (pe_ac & 1u) != 0, ac);  // a <- c: as stored when the record is (c -> a)
            const uint32_t r = judge_triangle(ba, cb, ac, thr);
            const uint32_t g = r & 1u;
            ++c_tri;
            c_good += g;
            c_skip += r >> 1;
            atomicAdd(&n_tri[pe_ac >> 1], 1u);
            atomicAdd(&n_tri[pe_bc >> 1], 1u);
            if (g) {
                atomicAdd(&n_good[pe_ac >> 1], 1u);
                atomicAdd(&n_good[pe_bc >> 1], 1u);
            }
        }
    }
    c_tri = wave_sum(c_tri);
    c_good = wave_sum(c_good);
    c_skip = wave_sum(c_skip);
    if (lane == 0 && c_tri) {
        atomicAdd(&n_tri[pe_ab >> 1], c_tri);
        atomicAdd(&totals->triangles, (unsigned long long)c_tri);
        if (c_good) {
            atomicAdd(&n_good[pe_ab >> 1], c_good);
            atomicAdd(&totals->good, (unsigned long long)c_good);
        }
        if (c_skip) atomicAdd(&totals->skipped, (unsigned long long)c_skip);
    }
}

// table_out may be the input table itself (in place) or a copy of it made before this launch; only the status of a
// dropped record is written.
__global__ __launch_bounds__(256) void cyc_finalize_kernel(const pgi_edge* table, uint32_t n_pairs, const uint32_t* __restrict__ n_tri,
                                                           const uint32_t* __restrict__ n_good, uint32_t min_good, uint32_t keep_untested,
                                                           uint8_t* __restrict__ keep_out, pgi_edge* table_out,
                                                           CycTotals* __restrict__ totals) {
    __shared__ uint32_t s_ok, s_drop;
    if (threadIdx.x == 0) s_ok = s_drop = 0;
    __syncthreads();
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n_pairs) {
        const bool ok = table[p].status == PGI_EDGE_OK;
        const bool keep = ok && (n_good[p] >= min_good || (n_tri[p] == 0 && keep_untested));
        if (keep_out) keep_out[p] = keep ? 1 : 0;
        if (ok) atomicAdd(&s_ok, 1u);
        if (ok && !keep) {
            atomicAdd(&s_drop, 1u);
            if (table_out) table_out[p].status = PGI_EDGE_INCONSISTENT;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_ok) atomicAdd(&totals->n_ok, s_ok);
        if (s_drop) atomicAdd(&totals->n_dropped, s_drop);
    }
}

bool cycle_params_ok(const pgi_cycle_params& p) {
    auto deg_ok = [](double d) { return d > 0.0 && d <= 90.0; };  // (false for NaN)
    return deg_ok(p.rot_thr_deg) && deg_ok(p.trn_thr_deg) && deg_ok(p.collinear_thr_deg) && p.min_good != 0;
}

// The adjacency of the OK records, neighbour lists sorted by view id: two stable counting sorts, by neighbour, then by owner.
struct CycAdjacency {
    std::vector<uint32_t> ptr, above, nbr, pe, work_a, work_pos;
};
int cycle_adjacency(const int32_t* status, const uint32_t* h_src, const uint32_t* h_dst, uint32_t n_pairs, uint32_t n_views,
                    CycAdjacency& adj) {
    if (n_pairs > 0x7fffffffu) return fail(PGI_ERR_TOO_LARGE, "cycle filter: more than 2^31 - 1 pairs");
    const size_t V = n_views;
    std::vector<uint32_t> by_nbr(V + 1, 0u);
    adj.ptr.assign(V + 1, 0u);
    size_t nE = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (status && status[p] != PGI_EDGE_OK) continue;
        const uint32_t s = h_src[p], d = h_dst[p];
        if (s >= n_views || d >= n_views) return fail(PGI_ERR_INVALID, "cycle filter: view id out of range");
        if (s == d) return fail(PGI_ERR_INVALID, "cycle filter: a pair joins a view with itself");
        ++by_nbr[s + 1], ++by_nbr[d + 1];
        ++adj.ptr[s + 1], ++adj.ptr[d + 1];
        ++nE;
    }
    if (nE > 0x3fffffffu) return fail(PGI_ERR_TOO_LARGE, "cycle filter: more than 2^30 - 1 OK records");  // (32-bit list positions)
    for (size_t v = 0; v < V; ++v) by_nbr[v + 1] += by_nbr[v], adj.ptr[v + 1] += adj.ptr[v];
    struct Entry { uint32_t owner, nbr, pe; };
    std::vector<Entry> tmp(2 * nE);
    {
        std::vector<uint32_t> at(by_nbr.begin(), by_nbr.end() - 1);
        for (uint32_t p = 0; p < n_pairs; ++p) {
            if (status && status[p] != PGI_EDGE_OK) continue;
            const uint32_t s = h_src[p], d = h_dst[p];
            tmp[at[d]++] = Entry{s, d, (p << 1) | 1u};  // in s's list: stored as (owner -> neighbour)
            tmp[at[s]++] = Entry{d, s, p << 1};
        }
    }
    adj.nbr.resize(2 * nE);
    adj.pe.resize(2 * nE);
    {
        std::vector<uint32_t> at(adj.ptr.begin(), adj.ptr.end() - 1);
        for (const Entry& e : tmp) {
            const uint32_t k = at[e.owner]++;
            adj.nbr[k] = e.nbr;
            adj.pe[k] = e.pe;
        }
    }
    adj.above.resize(V);
    adj.work_a.reserve(nE);
    adj.work_pos.reserve(nE);
    for (uint32_t v = 0; v < n_views; ++v) {
        uint32_t k = adj.ptr[v];
        const uint32_t end = adj.ptr[v + 1];
        for (; k < end && adj.nbr[k] < v; ++k)
            if (k + 1 < end && adj.nbr[k + 1] == adj.nbr[k]) return fail(PGI_ERR_INVALID, "cycle filter: a view pair occurs twice among the OK records");
        adj.above[v] = k;
        for (; k < end; ++k) {
            if (k + 1 < end && adj.nbr[k + 1] == adj.nbr[k]) return fail(PGI_ERR_INVALID, "cycle filter: a view pair occurs twice among the OK records");
            adj.work_a.push_back(v);
            adj.work_pos.push_back(k);
        }
    }
    return PGI_SUCCESS;
}

// d_edges: the table (device).  status: its status column on the host, or null = every record is OK.
int cycle_run(pgi_ctx* ctx, const pgi_edge* d_edges, const int32_t* status, const uint32_t* h_src, const uint32_t* h_dst,
              uint32_t n_pairs, uint32_t n_views, const pgi_cycle_params& prm, uint8_t* d_keep, uint32_t* d_n_tri, uint32_t* d_n_good,
              pgi_cycle_summary* h_summary, pgi_edge* d_edges_out) {
    hipStream_t st = ctx->stream;
    CycAdjacency adj;
    const int rc = cycle_adjacency(status, h_src, h_dst, n_pairs, n_views, adj);
    if (rc != PGI_SUCCESS) return rc;
    const size_t nW = adj.work_a.size(), nA = adj.nbr.size(), V = n_views, P = n_pairs;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_tot = 0, o_ptr = up(sizeof(CycTotals)), o_above = o_ptr + up((V + 1) * 4), o_nbr = o_above + up(V * 4),
                 o_pe = o_nbr + up(nA * 4), o_wa = o_pe + up(nA * 4), o_wp = o_wa + up(nW * 4), o_nt = o_wp + up(nW * 4),
                 o_ng = o_nt + up(d_n_tri ? 0 : P * 4), total = o_ng + up(d_n_good ? 0 : P * 4) + 256;
    char* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, total));
    struct Guard {
        void* p;
        ~Guard() { (void)hipFree(p); }
    } guard{d};
    uint32_t* n_tri = d_n_tri ? d_n_tri : (uint32_t*)(d + o_nt);
    uint32_t* n_good = d_n_good ? d_n_good : (uint32_t*)(d + o_ng);
    CycTotals* totals = (CycTotals*)(d + o_tot);
    // PGI_CYCLE_TRACE=1: HIP-event times of the uploads and of the two kernels, to stderr (scripts/cycle_filter_bench.py)
    const char* trace_env = getenv("PGI_CYCLE_TRACE");
    const bool trace = trace_env && trace_env[0] == '1';
    struct Events {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    if (trace) {
        for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(hipEventRecord(ev.e[0], st));
    }
    HIP_TRY(hipMemsetAsync(totals, 0, sizeof(CycTotals), st));
    HIP_TRY(hipMemsetAsync(n_tri, 0, P * 4, st));
    HIP_TRY(hipMemsetAsync(n_good, 0, P * 4, st));
    if (d_edges_out && d_edges_out != d_edges)
        HIP_TRY(hipMemcpyAsync(d_edges_out, d_edges, P * sizeof(pgi_edge), hipMemcpyDeviceToDevice, st));
    if (nW) {
        HIP_TRY(hipMemcpyAsync(d + o_ptr, adj.ptr.data(), (V + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + o_above, adj.above.data(), V * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + o_nbr, adj.nbr.data(), nA * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + o_pe, adj.pe.data(), nA * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + o_wa, adj.work_a.data(), nW * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + o_wp, adj.work_pos.data(), nW * 4, hipMemcpyHostToDevice, st));
        if (trace) HIP_TRY(hipEventRecord(ev.e[1], st));
        const double rad = 3.14159265358979323846 / 180.0;
        CycThresholds thr;
        thr.rot_min = 1.0 + 2.0 * std::cos(prm.rot_thr_deg * rad);
        const double st_ = std::sin(prm.trn_thr_deg * rad), sc = std::sin(prm.collinear_thr_deg * rad);
        thr.s2_trn = st_ * st_;
        thr.s2_col = sc * sc;
        hipLaunchKernelGGL(cyc_triangles_kernel, dim3((uint32_t)((nW + 3) / 4)), dim3(256), 0, st, d_edges, (const uint32_t*)(d + o_ptr),
                           (const uint32_t*)(d + o_above), (const uint32_t*)(d + o_nbr), (const uint32_t*)(d + o_pe),
                           (const uint32_t*)(d + o_wa), (const uint32_t*)(d + o_wp), (uint32_t)nW, thr, n_tri, n_good, totals);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cyc_finalize_kernel, dim3((uint32_t)((P + 255) / 256)), dim3(256), 0, st, d_edges, n_pairs, (const uint32_t*)n_tri,
                       (const uint32_t*)n_good, prm.min_good, prm.keep_untested, d_keep, d_edges_out, totals);
    HIP_TRY(hipGetLastError());
    if (trace) HIP_TRY(hipEventRecord(ev.e[2], st));
    pgi_cycle_summary sum;
    HIP_TRY(hipMemcpyAsync(&sum, totals, sizeof(sum), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_summary) *h_summary = sum;
    if (trace) {
        float ms_all = 0.f, ms_k = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_all, ev.e[0], ev.e[2]));
        if (nW) HIP_TRY(hipEventElapsedTime(&ms_k, ev.e[1], ev.e[2]));
        fprintf(stderr, "pgi_cycle: %zu OK pairs, %llu triangles; device %.3f ms (uploads and clears %.3f ms, kernels %.3f ms)\n", nW,
                (unsigned long long)sum.n_triangles, ms_all, ms_all - ms_k, ms_k);
    }
    return PGI_SUCCESS;
}

template <class F>
int guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(PGI_ERR_NOMEM, "cycle filter: out of host memory");
    } catch (const std::exception& e) {
        return fail(PGI_ERR_INVALID, std::string("cycle filter: ") + e.what());
    } catch (...) {
        return fail(PGI_ERR_INVALID, "cycle filter: unknown exception");
    }
}
}  // namespace
}  // namespace pgi

using namespace pgi;

extern "C" {

void pgi_default_cycle_params(pgi_cycle_params* p) {
    p->rot_thr_deg = 5.0;
    p->trn_thr_deg = 15.0;
    p->collinear_thr_deg = 5.0;
    p->min_good = 1;
    p->keep_untested = 1;
}

int pgi_cycle_filter_edges(pgi_ctx* ctx, const pgi_edge* d_edges, const uint32_t* h_src, const uint32_t* h_dst, uint32_t n_pairs,
                           uint32_t n_views, const pgi_cycle_params* prm_in, uint8_t* d_keep, uint32_t* d_n_tri, uint32_t* d_n_good,
                           pgi_cycle_summary* h_summary, pgi_edge* d_edges_out) {
    return guarded([&]() -> int {
        if (!ctx || (n_pairs && (!d_edges || !h_src || !h_dst))) return fail(PGI_ERR_INVALID, "null argument");
        pgi_cycle_params prm;
        if (prm_in) prm = *prm_in; else pgi_default_cycle_params(&prm);
        if (!cycle_params_ok(prm)) return fail(PGI_ERR_INVALID, "cycle filter parameters out of range");
        if (h_summary) memset(h_summary, 0, sizeof(*h_summary));
        if (n_pairs == 0) return PGI_SUCCESS;
        std::lock_guard<std::mutex> lk(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        // the status of every record: a 4-byte column of the 200-byte table
        std::vector<int32_t> status(n_pairs);
        HIP_TRY(hipMemcpy2DAsync(status.data(), 4, (const char*)d_edges + offsetof(pgi_edge, status), sizeof(pgi_edge), 4, n_pairs,
                                 hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return cycle_run(ctx, d_edges, status.data(), h_src, h_dst, n_pairs, n_views, prm, d_keep, d_n_tri, d_n_good, h_summary,
                         d_edges_out);
    });
}

int pgi_cycle_filter(pgi_ctx* ctx, const pgi_cycle_edge* h_edges, uint32_t n_edges, uint32_t n_views, const pgi_cycle_params* prm_in,
                     uint8_t* h_keep, uint32_t* h_n_tri, uint32_t* h_n_good, pgi_cycle_summary* h_summary) {
    return guarded([&]() -> int {
        if (!ctx || (n_edges && !h_edges)) return fail(PGI_ERR_INVALID, "null argument");
        pgi_cycle_params prm;
        if (prm_in) prm = *prm_in; else pgi_default_cycle_params(&prm);
        if (!cycle_params_ok(prm)) return fail(PGI_ERR_INVALID, "cycle filter parameters out of range");
        if (h_summary) memset(h_summary, 0, sizeof(*h_summary));
        if (n_edges == 0) return PGI_SUCCESS;
        const size_t P = n_edges;
        std::vector<uint32_t> src(P), dst(P);
        std::vector<pgi_edge> table(P);
        memset(table.data(), 0, P * sizeof(pgi_edge));
        for (size_t e = 0; e < P; ++e) {
            src[e] = h_edges[e].src;
            dst[e] = h_edges[e].dst;
            memcpy(table[e].R, h_edges[e].R, 72);
            memcpy(table[e].t, h_edges[e].t, 24);
            table[e].status = PGI_EDGE_OK;
        }
        std::lock_guard<std::mutex> lk(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
        const size_t o_keep = up(P * sizeof(pgi_edge)), o_nt = o_keep + up(P), o_ng = o_nt + up(P * 4), total = o_ng + up(P * 4);
        char* d = nullptr;
        HIP_TRY(hipMalloc((void**)&d, total));
        struct Guard {
            void* p;
            ~Guard() { (void)hipFree(p); }
        } guard{d};
        HIP_TRY(hipMemcpyAsync(d, table.data(), P * sizeof(pgi_edge), hipMemcpyHostToDevice, ctx->stream));
        const int rc = cycle_run(ctx, (const pgi_edge*)d, nullptr, src.data(), dst.data(), n_edges, n_views, prm, (uint8_t*)(d + o_keep),
                                 (uint32_t*)(d + o_nt), (uint32_t*)(d + o_ng), h_summary, nullptr);
        if (rc != PGI_SUCCESS) return rc;
        if (h_keep) HIP_TRY(hipMemcpyAsync(h_keep, d + o_keep, P, hipMemcpyDeviceToHost, ctx->stream));
        if (h_n_tri) HIP_TRY(hipMemcpyAsync(h_n_tri, d + o_nt, P * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (h_n_good) HIP_TRY(hipMemcpyAsync(h_n_good, d + o_ng, P * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PGI_SUCCESS;
    });
}

}  // extern "C"
