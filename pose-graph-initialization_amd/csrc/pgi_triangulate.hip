// pgi_triangulate.hip -- sparse 3-D points from the global poses and the multi-view tracks (include/pgi.h:
// pgi_triangulate_tracks, pgi_tracklets_triangulate).  Not in the reference, which triangulates two views by a 4 x 4 SVD
// (pose_utils.h:491-506) and nothing else.
//
// The specification is tests/triangulate_spec.py; every f64 statement here is the same single IEEE operation in the same
// order (-ffp-contract=off), so the outputs equal it bit for bit.
//
// Mapping: one track per lane, every sum sequential in member order -- a track's result depends on nothing but the track.
// Tracks are ragged (mostly 2-4 members, a tail into the tens) and a wavefront runs as long as its longest track, so the
// lanes take the tracks in descending order of length (a stable 16-bit radix sort of (length, index) on the device) and
// scatter the outputs back to track order.  PGI_TRI_SORT=0 in the environment keeps the given order (A/B measurements only).
// The view records (16 f64: R, c, fx fy cx cy) sit in one device table; up to kTriLdsViews views the workgroup stages the
// table in LDS, above that the lanes read it through L2.  Pixels are gathered through a device array of per-view keypoint
// pointers.  The per-member state (0 not counted, 1 used, 2 dropped) lives in the caller's d_obs_state or in scratch.
#include "pgi_internal.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include <rocprim/device/device_radix_sort.hpp>

namespace pgi {
namespace {

constexpr int kTriBlock = 256;
constexpr uint32_t kTriLdsViews = 256;  // 32 KB of LDS: five workgroups of 256 lanes still fit a CU's 160 KB
constexpr double kTriDetRel = 1e-12;    // DET_REL of the specification
constexpr uint32_t kNoArg = 0xffffffffu;

#define TDEV __device__ __forceinline__

struct TriArgs {
    const uint32_t* track_begin;
    const uint64_t* members;
    const uint32_t* order;       // slot -> track (length order), or nullptr = identity
    const double* views;         // n_views x 16
    const float* const* kp_xy;   // n_views
    const uint32_t* kp_n;        // n_views; 0 for a view without a pose
    uint8_t* state;              // one byte per member
    double* X;
    double* err;
    uint32_t* n_used;
    uint8_t* status;
    uint32_t* counts;
    uint32_t n_tracks, n_views;
    uint32_t member_cap;         // members in the arrays (0xffffffff = not known)
    uint32_t min_views, refine_iters, max_drops;
    double thr_px, cos_min;
};

struct TriEval {
    double cost, max_e2;
    double H[6], g[3];
    uint32_t arg;
    bool nonpos;
};

// the specification's solve_sym3: adjugate of the symmetric matrix (00 01 02 11 12 22), fixed operation order
TDEV double tri_solve_sym3(const double* a, const double* b, double* x) {
    const double a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
    const double c00 = a11 * a22 - a12 * a12;
    const double c01 = a02 * a12 - a01 * a22;
    const double c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02;
    const double c12 = a01 * a02 - a00 * a12;
    const double c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    x[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
    x[1] = ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
    x[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
    return det;
}

struct TriTrack {
    const uint64_t* mem;   // the track's members
    uint8_t* state;
    uint32_t n;
    const double* views;   // LDS or global
    const float* const* kp_xy;
};

// member k of a used observation: its view record and pixel (the eligibility pass has checked the indices)
TDEV const double* tri_load(const TriTrack& t, uint32_t k, double& px, double& py) {
    const uint64_t key = t.mem[k];
    const uint32_t v = (uint32_t)(key >> 32), kp = (uint32_t)key;
    const float2 p = reinterpret_cast<const float2*>(t.kp_xy[v])[kp];
    px = (double)p.x;
    py = (double)p.y;
    return t.views + (size_t)v * 16;
}

// step 2 of the specification; returns the determinant
TDEV double tri_midpoint(const TriTrack& t, double* X) {
    double a[6] = {0, 0, 0, 0, 0, 0}, r[3] = {0, 0, 0};
    for (uint32_t k = 0; k < t.n; ++k) {
        if (t.state[k] != 1) continue;
        double px, py;
        const double* w = tri_load(t, k, px, py);
        const double x = (px - w[14]) / w[12];
        const double y = (py - w[15]) / w[13];
        const double n = sqrt((x * x + y * y) + 1.0);
        const double b0 = x / n, b1 = y / n, b2 = 1.0 / n;
        const double d0 = (w[0] * b0 + w[3] * b1) + w[6] * b2;
        const double d1 = (w[1] * b0 + w[4] * b1) + w[7] * b2;
        const double d2 = (w[2] * b0 + w[5] * b1) + w[8] * b2;
        a[0] = a[0] + (1.0 - d0 * d0);
        a[3] = a[3] + (1.0 - d1 * d1);
        a[5] = a[5] + (1.0 - d2 * d2);
        a[1] = a[1] + (-(d0 * d1));
        a[2] = a[2] + (-(d0 * d2));
        a[4] = a[4] + (-(d1 * d2));
        const double dc = (d0 * w[9] + d1 * w[10]) + d2 * w[11];
        r[0] = r[0] + (w[9] - d0 * dc);
        r[1] = r[1] + (w[10] - d1 * dc);
        r[2] = r[2] + (w[11] - d2 * dc);
    }
    return tri_solve_sym3(a, r, X);
}

// step 3 of the specification
TDEV void tri_evaluate(const TriTrack& t, const double* X, TriEval& e) {
    e.cost = 0.0;
    e.max_e2 = -1.0;
    e.arg = kNoArg;
    e.nonpos = false;
    for (int i = 0; i < 6; ++i) e.H[i] = 0.0;
    for (int i = 0; i < 3; ++i) e.g[i] = 0.0;
    for (uint32_t k = 0; k < t.n; ++k) {
        if (t.state[k] != 1) continue;
        double px, py;
        const double* w = tri_load(t, k, px, py);
        const double dx0 = X[0] - w[9], dx1 = X[1] - w[10], dx2 = X[2] - w[11];
        const double q0 = (w[0] * dx0 + w[1] * dx1) + w[2] * dx2;
        const double q1 = (w[3] * dx0 + w[4] * dx1) + w[5] * dx2;
        const double q2 = (w[6] * dx0 + w[7] * dx1) + w[8] * dx2;
        double e2;
        if (q2 > 0.0) {
            const double a = q0 / q2, b = q1 / q2, iz = 1.0 / q2;
            const double r0 = (w[12] * a + w[14]) - px;
            const double r1 = (w[13] * b + w[15]) - py;
            e2 = r0 * r0 + r1 * r1;
            const double sx = w[12] * iz, sy = w[13] * iz;
            double ju[3], jv[3];
            for (int i = 0; i < 3; ++i) {
                ju[i] = sx * (w[i] - a * w[6 + i]);
                jv[i] = sy * (w[3 + i] - b * w[6 + i]);
            }
            int n = 0;
            for (int i = 0; i < 3; ++i) {
                for (int j = i; j < 3; ++j, ++n) e.H[n] = e.H[n] + (ju[i] * ju[j] + jv[i] * jv[j]);
                e.g[i] = e.g[i] + (ju[i] * r0 + jv[i] * r1);
            }
        } else {
            e2 = std::numeric_limits<double>::infinity();
            e.nonpos = true;
        }
        e.cost = e.cost + e2;
        if (e2 > e.max_e2) {
            e.max_e2 = e2;
            e.arg = k;
        }
    }
}

// step 5 of the specification: is some pair of used rays wider apart than the bound?
TDEV bool tri_wide_enough(const TriTrack& t, const double* X, double cos_min) {
    for (uint32_t k = 1; k < t.n; ++k) {
        if (t.state[k] != 1) continue;
        const double* wk = t.views + (size_t)(t.mem[k] >> 32) * 16;
        const double uk0 = X[0] - wk[9], uk1 = X[1] - wk[10], uk2 = X[2] - wk[11];
        const double nk = sqrt((uk0 * uk0 + uk1 * uk1) + uk2 * uk2);
        for (uint32_t j = 0; j < k; ++j) {
            if (t.state[j] != 1) continue;
            const double* wj = t.views + (size_t)(t.mem[j] >> 32) * 16;
            const double uj0 = X[0] - wj[9], uj1 = X[1] - wj[10], uj2 = X[2] - wj[11];
            const double nj = sqrt((uj0 * uj0 + uj1 * uj1) + uj2 * uj2);
            const double cosv = ((uj0 * uk0 + uj1 * uk1) + uj2 * uk2) / (nj * nk);
            if (cosv < cos_min) return true;
        }
    }
    return false;
}

__global__ __launch_bounds__(kTriBlock) void tri_length_kernel(const uint32_t* __restrict__ track_begin, uint32_t n_tracks,
                                                               uint32_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const uint32_t t = blockIdx.x * kTriBlock + threadIdx.x;
    if (t >= n_tracks) return;
    const uint32_t b = track_begin[t], e = track_begin[t + 1];
    const uint32_t len = e > b ? e - b : 0u;
    key[t] = len < 0xffffu ? len : 0xffffu;
    idx[t] = t;
}

template <bool LDS>
__global__ __launch_bounds__(kTriBlock) void tri_tracks_kernel(TriArgs A) {
    extern __shared__ double s_views[];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < A.n_views * 16; i += kTriBlock) s_views[i] = A.views[i];
        __syncthreads();
    }
    const uint32_t slot = blockIdx.x * kTriBlock + threadIdx.x;
    if (slot >= A.n_tracks) return;
    const uint32_t track = A.order ? A.order[slot] : slot;
    uint32_t end = A.track_begin[track + 1], beg = A.track_begin[track];
    if (end > A.member_cap) end = A.member_cap;
    if (beg > end) beg = end;
    TriTrack t;
    t.mem = A.members + beg;
    t.state = A.state + beg;
    t.n = end - beg;
    t.views = LDS ? s_views : A.views;
    t.kp_xy = A.kp_xy;

    // step 1: eligibility, first occurrence of a view wins
    uint32_t n_used = 0;
    for (uint32_t k = 0; k < t.n; ++k) {
        const uint64_t key = t.mem[k];
        const uint32_t v = (uint32_t)(key >> 32), kp = (uint32_t)key;
        bool ok = v < A.n_views && kp < A.kp_n[v];
        if (ok) {
            const float2 p = reinterpret_cast<const float2*>(A.kp_xy[v])[kp];
            ok = isfinite(p.x) && isfinite(p.y);
        }
        for (uint32_t j = 0; ok && j < k; ++j) ok = !(t.state[j] == 1 && (uint32_t)(t.mem[j] >> 32) == v);
        t.state[k] = ok ? 1 : 0;
        n_used += ok ? 1u : 0u;
    }

    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t floor_used = A.min_views > 2 ? A.min_views : 2;
    double X[3] = {nan, nan, nan}, rms = nan;
    uint32_t status = PGI_TRI_TOO_FEW, n_drop = 0;
    bool active = n_used >= A.min_views;
    while (active) {
        double Xf[3];
        const double det = tri_midpoint(t, Xf);
        const double m = (double)n_used;
        if (!(det > kTriDetRel * ((m * m) * m) && det < std::numeric_limits<double>::infinity())) {
            status = PGI_TRI_DEGENERATE;
            break;
        }
        TriEval e;
        tri_evaluate(t, Xf, e);
        bool can = !e.nonpos;
        for (uint32_t it = 0; can && it < A.refine_iters; ++it) {
            double d[3];
            const double dh = tri_solve_sym3(e.H, e.g, d);
            if (!(dh > 0.0 && dh < std::numeric_limits<double>::infinity())) break;
            const double Xn[3] = {Xf[0] - d[0], Xf[1] - d[1], Xf[2] - d[2]};
            TriEval e1;
            tri_evaluate(t, Xn, e1);
            can = !e1.nonpos && e1.cost < e.cost;
            if (can) {
                Xf[0] = Xn[0], Xf[1] = Xn[1], Xf[2] = Xn[2];
                e = e1;
            }
        }
        const double err = sqrt(e.max_e2);
        if (err > A.thr_px && n_used > floor_used && n_drop < A.max_drops && e.arg != kNoArg) {
            t.state[e.arg] = 2;  // step 4: drop the worst, fit the rest again
            --n_used;
            ++n_drop;
            continue;
        }
        rms = sqrt(e.cost / (double)n_used);
        if (!(err <= A.thr_px)) {
            status = e.nonpos ? PGI_TRI_BEHIND : PGI_TRI_REPROJ;
        } else {
            status = tri_wide_enough(t, Xf, A.cos_min) ? PGI_TRI_OK : PGI_TRI_LOW_PARALLAX;
            X[0] = Xf[0], X[1] = Xf[1], X[2] = Xf[2];
        }
        break;
    }
    A.X[(size_t)track * 3 + 0] = X[0];
    A.X[(size_t)track * 3 + 1] = X[1];
    A.X[(size_t)track * 3 + 2] = X[2];
    A.status[track] = (uint8_t)status;
    if (A.err) A.err[track] = rms;
    if (A.n_used) A.n_used[track] = n_used;
    atomicAdd(&A.counts[status], 1u);  // integer counters: the order of the additions does not matter
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int tri_validate(const char* who, const pgi_keypoint_view* h_views, const double* h_R, const double* h_c, const uint8_t* h_has_pose,
                 uint32_t n_views, const pgi_triangulate_params& prm) {
    if (prm.min_views < 2) return fail(PGI_ERR_INVALID, std::string(who) + ": min_views must be at least 2");
    if (!(prm.thr_px > 0.0)) return fail(PGI_ERR_INVALID, std::string(who) + ": thr_px must be positive");
    if (!std::isfinite(prm.min_angle_deg)) return fail(PGI_ERR_INVALID, std::string(who) + ": min_angle_deg must be finite");
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

// ctx->mu held.  n_members: members in d_members when the caller knows it, otherwise read from d_track_begin if scratch needs it
int tri_run(const char* who, pgi_ctx* ctx, const uint32_t* d_track_begin, const uint64_t* d_members, uint32_t n_tracks, bool members_known,
            uint64_t n_members, const pgi_keypoint_view* h_views, const double* h_R, const double* h_c, const uint8_t* h_has_pose,
            uint32_t n_views, const pgi_triangulate_params& prm, double* d_X, double* d_err, uint32_t* d_n_used, uint8_t* d_status,
            uint8_t* d_obs_state, uint32_t* h_status_counts) {
    if (h_status_counts) memset(h_status_counts, 0, PGI_TRI_STATUS_COUNT * sizeof(uint32_t));
    if (!n_tracks) return PGI_SUCCESS;
    if (!d_track_begin || !d_X || !d_status) return fail(PGI_ERR_INVALID, std::string(who) + ": null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (!d_obs_state && !members_known) {  // the member states go to scratch: its size is the last offset
        uint32_t last = 0;
        HIP_TRY(hipMemcpyAsync(&last, d_track_begin + n_tracks, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_members = last;
        members_known = true;
    }
    if (members_known && n_members > 0xfffffffeull) return fail(PGI_ERR_TOO_LARGE, std::string(who) + ": more than 2^32 - 2 members");
    if (members_known && n_members && !d_members) return fail(PGI_ERR_INVALID, std::string(who) + ": null members");
    const char* sort_env = getenv("PGI_TRI_SORT");  // read per call: A/B measurements only
    const bool sort_by_length = !sort_env || atoi(sort_env) != 0;
    const bool lds = n_views <= kTriLdsViews;

    // scratch layout
    const size_t views_b = align256((size_t)n_views * 128), ptr_b = align256((size_t)n_views * 8), cnt_b = align256((size_t)n_views * 4);
    const size_t stage_b = views_b + ptr_b + cnt_b;
    const size_t counts_b = 256, u32_b = align256((size_t)n_tracks * 4);
    const size_t state_b = d_obs_state ? 0 : align256((size_t)n_members);
    size_t sort_b = 0;
    if (sort_by_length)
        HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, sort_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                               (uint32_t*)nullptr, (size_t)n_tracks, 0u, 16u, s));
    sort_b = align256(sort_b);
    const size_t total = stage_b + counts_b + 4 * u32_b + state_b + sort_b;
    if (total > ctx->tri_ws_bytes) {
        HIP_TRY(hipStreamSynchronize(s));  // kernels in flight may still use the old block
        if (ctx->d_tri_ws) (void)hipFree(ctx->d_tri_ws);
        ctx->d_tri_ws = nullptr;
        ctx->tri_ws_bytes = 0;
        hipError_t e = hipMalloc(&ctx->d_tri_ws, total);
        if (e != hipSuccess) return fail(PGI_ERR_NOMEM, std::string(who) + ": device scratch: " + hipGetErrorString(e));
        ctx->tri_ws_bytes = total;
    }
    if (!ctx->tri_stage_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->tri_stage_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ctx->tri_stage_ev));  // the previous call's upload has left the mirror
    if (stage_b > ctx->tri_stage_bytes) {
        if (ctx->h_tri_stage) (void)hipHostFree(ctx->h_tri_stage);
        ctx->h_tri_stage = nullptr;
        ctx->tri_stage_bytes = 0;
        hipError_t e = hipHostMalloc(&ctx->h_tri_stage, stage_b, hipHostMallocDefault);
        if (e != hipSuccess) return fail(PGI_ERR_NOMEM, std::string(who) + ": page-locked staging: " + hipGetErrorString(e));
        ctx->tri_stage_bytes = stage_b;
    }
    char* ws = (char*)ctx->d_tri_ws;
    char* hs = (char*)ctx->h_tri_stage;
    double* h_tab = (double*)hs;
    const float** h_ptr = (const float**)(hs + views_b);
    uint32_t* h_cnt = (uint32_t*)(hs + views_b + ptr_b);
    for (uint32_t v = 0; v < n_views; ++v) {
        const bool posed = !h_has_pose || h_has_pose[v];
        double* w = h_tab + (size_t)v * 16;
        if (posed) {
            for (int i = 0; i < 9; ++i) w[i] = h_R[(size_t)v * 9 + i];
            for (int i = 0; i < 3; ++i) w[9 + i] = h_c[(size_t)v * 3 + i];
            w[12] = h_views[v].fx, w[13] = h_views[v].fy, w[14] = h_views[v].cx, w[15] = h_views[v].cy;
        } else {
            for (int i = 0; i < 16; ++i) w[i] = 0.0;
        }
        h_ptr[v] = h_views[v].d_xy;
        h_cnt[v] = posed ? h_views[v].n : 0u;  // a view without a pose has no usable keypoint
    }
    if (stage_b) HIP_TRY(hipMemcpyAsync(ws, hs, stage_b, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(ctx->tri_stage_ev, s));
    uint32_t* d_counts = (uint32_t*)(ws + stage_b);
    uint32_t* d_key = (uint32_t*)(ws + stage_b + counts_b);
    uint32_t* d_idx = d_key + u32_b / 4;
    uint32_t* d_key2 = d_idx + u32_b / 4;
    uint32_t* d_order = d_key2 + u32_b / 4;
    uint8_t* d_state = d_obs_state ? d_obs_state : (uint8_t*)(ws + stage_b + counts_b + 4 * u32_b);
    void* d_sort = ws + stage_b + counts_b + 4 * u32_b + state_b;
    HIP_TRY(hipMemsetAsync(d_counts, 0, counts_b, s));
    const dim3 grid((n_tracks + kTriBlock - 1) / kTriBlock), block(kTriBlock);
    if (sort_by_length) {
        hipLaunchKernelGGL(tri_length_kernel, grid, block, 0, s, d_track_begin, n_tracks, d_key, d_idx);
        HIP_TRY(rocprim::radix_sort_pairs_desc(d_sort, sort_b, (const uint32_t*)d_key, d_key2, (const uint32_t*)d_idx, d_order,
                                               (size_t)n_tracks, 0u, 16u, s));
    }
    TriArgs A;
    A.track_begin = d_track_begin;
    A.members = d_members;
    A.order = sort_by_length ? d_order : nullptr;
    A.views = (const double*)ws;
    A.kp_xy = (const float* const*)(ws + views_b);
    A.kp_n = (const uint32_t*)(ws + views_b + ptr_b);
    A.state = d_state;
    A.X = d_X, A.err = d_err, A.n_used = d_n_used, A.status = d_status, A.counts = d_counts;
    A.n_tracks = n_tracks, A.n_views = n_views;
    A.member_cap = members_known ? (uint32_t)n_members : 0xffffffffu;
    A.min_views = prm.min_views, A.refine_iters = prm.refine_iters, A.max_drops = prm.max_drops;
    A.thr_px = prm.thr_px;
    A.cos_min = std::cos(prm.min_angle_deg * (M_PI / 180.0));  // the specification's math.cos(math.radians(.)): no trigonometry on the device
    if (lds) hipLaunchKernelGGL(tri_tracks_kernel<true>, grid, block, (size_t)n_views * 128, s, A);
    else hipLaunchKernelGGL(tri_tracks_kernel<false>, grid, block, 0, s, A);
    HIP_TRY(hipGetLastError());
    if (h_status_counts) {
        HIP_TRY(hipMemcpyAsync(h_status_counts, d_counts, PGI_TRI_STATUS_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return PGI_SUCCESS;
}

}  // namespace
}  // namespace pgi

extern "C" {

void pgi_default_triangulate_params(pgi_triangulate_params* p) {
    if (!p) return;
    p->min_views = 2;
    p->refine_iters = 3;
    p->max_drops = 2;
    p->reserved = 0;
    p->thr_px = 2.0;
    p->min_angle_deg = 1.5;
}

int pgi_triangulate_tracks(pgi_ctx* ctx, const uint32_t* d_track_begin, const uint64_t* d_members, uint32_t n_tracks,
                           const pgi_keypoint_view* h_views, const double* h_R, const double* h_c, const uint8_t* h_has_pose,
                           uint32_t n_views, const pgi_triangulate_params* prm, double* d_X, double* d_err, uint32_t* d_n_used,
                           uint8_t* d_status, uint8_t* d_obs_state, uint32_t* h_status_counts) {
    if (!ctx) return pgi::fail(PGI_ERR_INVALID, "pgi_triangulate_tracks: null context");
    pgi_triangulate_params p;
    if (prm) p = *prm; else pgi_default_triangulate_params(&p);
    if (int rc = pgi::tri_validate("pgi_triangulate_tracks", h_views, h_R, h_c, h_has_pose, n_views, p)) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    return pgi::tri_run("pgi_triangulate_tracks", ctx, d_track_begin, d_members, n_tracks, false, 0, h_views, h_R, h_c, h_has_pose, n_views,
                        p, d_X, d_err, d_n_used, d_status, d_obs_state, h_status_counts);
}

int pgi_tracklets_triangulate(pgi_tracklets* trk, const pgi_keypoint_view* h_views, const double* h_R, const double* h_c,
                              const uint8_t* h_has_pose, uint32_t n_views, const pgi_triangulate_params* prm, double* d_X, double* d_err,
                              uint32_t* d_n_used, uint8_t* d_status, uint8_t* d_obs_state, uint32_t* h_status_counts) {
    if (!trk) return pgi::fail(PGI_ERR_INVALID, "pgi_tracklets_triangulate: null store");
    pgi_triangulate_params p;
    if (prm) p = *prm; else pgi_default_triangulate_params(&p);
    if (int rc = pgi::tri_validate("pgi_tracklets_triangulate", h_views, h_R, h_c, h_has_pose, n_views, p)) return rc;
    pgi_ctx* ctx = nullptr;
    const uint32_t* d_begin = nullptr;
    const uint64_t* d_members = nullptr;
    uint32_t n_tracks = 0;
    uint64_t n_members = 0;
    pgi::tracklets_by_track(trk, &ctx, &d_begin, &d_members, &n_tracks, &n_members);
    std::lock_guard<std::mutex> lock(ctx->mu);
    return pgi::tri_run("pgi_tracklets_triangulate", ctx, d_begin, d_members, n_tracks, true, n_members, h_views, h_R, h_c, h_has_pose,
                        n_views, p, d_X, d_err, d_n_used, d_status, d_obs_state, h_status_counts);
}

}  // extern "C"
