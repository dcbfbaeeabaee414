// PoseGraphBuilder::bundleAdjustFocal (host/pose_graph_builder.hpp), both forms, checked bit for bit against the numbers the
// Python engine computed for the same tracks (tests/test_bundle_focal_cpp.py drives this program).
//   test_bundle_focal <input file>
// input (little endian): u32 V; per view: u32 n, f64 f, w, h, R[9], c[3], phi, u8 has_pose, f32 xy[2 n];
//   u32 T, u32 begin[T + 1], u64 members[begin[T]];  f64 X[3 T], u8 status[T], u8 obs_state[begin[T]]  (the start)
//   expected: f64 R[9 V], c[3 V], X[3 T], phi[V], u32 report[7] (iters, accepted, cg_iters_total, stop_reason, n_obs, n_points,
//   n_free_cams), u32 n_free_focals
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "pose_graph_builder.hpp"
#include "tracklets.hpp"

using namespace reconstruction;

template <class T>
static std::vector<T> take(std::ifstream& in, size_t n) {
    std::vector<T> v(n);
    if (n) in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    return v;
}

static bool sameBits(const double* a, const double* b, size_t n) { return n == 0 || std::memcmp(a, b, 8 * n) == 0; }

static int compare(const char* what, const PoseGraphBuilder::BundleAdjustment& got, const double* R, const double* c, const double* X,
                   const double* phi, size_t V, size_t T, const uint32_t* report, uint32_t freeFocals) {
    int bad = 0;
    if (got.rotations.rotations.size() != V || got.positions.positions.size() != V || got.points.size() != T || got.focalScales.size() != V) ++bad;
    for (size_t v = 0; !bad && v < V; ++v)
        if (!sameBits(got.rotations.rotations[v].data(), R + 9 * v, 9) || !sameBits(got.positions.positions[v].data(), c + 3 * v, 3)) ++bad;
    if (!bad && T && !sameBits(got.points[0].data(), X, 3 * T)) ++bad;
    if (!bad && !sameBits(got.focalScales.data(), phi, V)) ++bad;
    const pgi_bundle_report& r = got.report;
    const uint32_t mine[7] = {r.iters, r.accepted, r.cg_iters_total, r.stop_reason, r.n_obs, r.n_points, r.n_free_cams};
    if (std::memcmp(mine, report, sizeof mine) != 0 || got.freeFocals != freeFocals) ++bad;
    std::printf("%s: %zu views, %zu tracks, %u accepted of %u, %u free focals, %s\n", what, V, T, r.accepted, r.iters, got.freeFocals,
                bad ? "MISMATCH" : "identical");
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const uint32_t V = take<uint32_t>(in, 1)[0];
    std::vector<std::vector<float>> xy(V);
    std::vector<PoseGraphBuilder::ViewFeaturesRef> views(V);
    PoseGraphBuilder::GlobalRotations rot;
    PoseGraphBuilder::GlobalPositions pos;
    std::vector<uint8_t> hasPose(V);
    std::vector<double> phi0(V);
    rot.rotations.resize(V);
    pos.positions.resize(V);
    for (uint32_t v = 0; v < V; ++v) {
        const uint32_t n = take<uint32_t>(in, 1)[0];
        const std::vector<double> k = take<double>(in, 3 + 9 + 3 + 1);
        hasPose[v] = take<uint8_t>(in, 1)[0];
        xy[v] = take<float>(in, 2 * (size_t)n);
        views[v].keypoints = xy[v].data();
        views[v].n = n;
        views[v].focalLength = k[0], views[v].width = k[1], views[v].height = k[2];
        std::memcpy(rot.rotations[v].data(), &k[3], 72);
        std::memcpy(pos.positions[v].data(), &k[12], 24);
        phi0[v] = k[15];
    }
    const uint32_t T = take<uint32_t>(in, 1)[0];
    const std::vector<uint32_t> begin = take<uint32_t>(in, (size_t)T + 1);
    const std::vector<uint64_t> members = take<uint64_t>(in, begin[T]);
    PoseGraphBuilder::TriangulatedPoints pts;
    const std::vector<double> X0 = take<double>(in, 3 * (size_t)T);
    pts.points.resize(T);
    if (T) std::memcpy(pts.points[0].data(), X0.data(), 24 * (size_t)T);
    pts.status = take<uint8_t>(in, T);
    pts.observationState = take<uint8_t>(in, begin[T]);
    const std::vector<double> R = take<double>(in, 9 * (size_t)V), c = take<double>(in, 3 * (size_t)V), X = take<double>(in, 3 * (size_t)T),
                              phi = take<double>(in, V);
    const std::vector<uint32_t> report = take<uint32_t>(in, 8);
    if (!in) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    int bad = 0;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.5, 0.4, "", "", "", "", true, true, true);
        // (1) offsets and members as written by the scene
        bad += compare("arrays", builder.bundleAdjustFocal(begin, members, views, rot, pos, pts, phi0, &hasPose), R.data(), c.data(), X.data(),
                       phi.data(), V, T, report.data(), report[7]);
        // (2) a host-only store grown from the same tracks gives the store's own track order; its refinement must equal the
        //     array call on the tracks read back from it (the start: triangulated at the scaled focal lengths, nothing trimmed)
        std::vector<PoseGraphBuilder::ViewFeaturesRef> scaled(views);
        for (uint32_t v = 0; v < V; ++v) scaled[v].focalLength = views[v].focalLength * phi0[v];
        Tracklets store(V);
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t m = begin[t]; m + 1 < begin[t + 1]; ++m) {
                const uint64_t a = members[m], b = members[m + 1];
                if ((a >> 32) == (b >> 32)) continue;
                store.add((size_t)(a >> 32), (size_t)(b >> 32), {Tracklets::Match((size_t)(uint32_t)a, (size_t)(uint32_t)b, 0.0)}, {1});
            }
        std::vector<uint32_t> sb(1, 0);
        std::vector<uint64_t> sm;
        for (size_t t = 0; t < store.trackNumber(); ++t) {
            for (const Tracklets::Pair& p : store.track(t)) sm.push_back(((uint64_t)p.first << 32) | (uint64_t)(uint32_t)p.second);
            sb.push_back((uint32_t)sm.size());
        }
        pgi_triangulate_params tri;
        pgi_default_triangulate_params(&tri);
        tri.thr_px = 80.0, tri.max_drops = 0;  // bundle_focal_spec.FOCAL_TRI
        const PoseGraphBuilder::TriangulatedPoints spts = builder.triangulateTracks(store, scaled, rot, pos, &hasPose, &tri);
        const PoseGraphBuilder::BundleAdjustment viaArrays = builder.bundleAdjustFocal(sb, sm, views, rot, pos, spts, phi0, &hasPose);
        const PoseGraphBuilder::BundleAdjustment viaStore = builder.bundleAdjustFocal(store, views, rot, pos, spts, phi0, &hasPose);
        {
            std::vector<double> sR(9 * (size_t)V), sc(3 * (size_t)V);
            for (uint32_t v = 0; v < V; ++v) {
                std::memcpy(&sR[9 * v], viaArrays.rotations.rotations[v].data(), 72);
                std::memcpy(&sc[3 * v], viaArrays.positions.positions[v].data(), 24);
            }
            const pgi_bundle_report& r = viaArrays.report;
            const uint32_t rep[7] = {r.iters, r.accepted, r.cg_iters_total, r.stop_reason, r.n_obs, r.n_points, r.n_free_cams};
            bad += compare("host store", viaStore, sR.data(), sc.data(), viaArrays.points.empty() ? nullptr : viaArrays.points[0].data(),
                           viaArrays.focalScales.data(), V, viaArrays.points.size(), rep, viaArrays.freeFocals);
            if (viaStore.report.accepted == 0 || viaStore.freeFocals == 0) {
                std::printf("host store: nothing refined\n");
                ++bad;
            }
        }
        // (3) every focal held: the bits of bundleAdjust on focal lengths multiplied by phi here
        std::vector<uint8_t> allHeld(V, 1);
        const PoseGraphBuilder::BundleAdjustment plain = builder.bundleAdjust(begin, members, scaled, rot, pos, pts, &hasPose);
        std::vector<double> pR(9 * (size_t)V), pc(3 * (size_t)V);
        for (uint32_t v = 0; v < V; ++v) {
            std::memcpy(&pR[9 * v], plain.rotations.rotations[v].data(), 72);
            std::memcpy(&pc[3 * v], plain.positions.positions[v].data(), 24);
        }
        const pgi_bundle_report& r = plain.report;
        const uint32_t rep[7] = {r.iters, r.accepted, r.cg_iters_total, r.stop_reason, r.n_obs, r.n_points, r.n_free_cams};
        bad += compare("all held", builder.bundleAdjustFocal(begin, members, views, rot, pos, pts, phi0, &hasPose, nullptr, &allHeld),
                       pR.data(), pc.data(), T ? plain.points[0].data() : nullptr, phi0.data(), V, T, rep, 0);
        // (4) a focal scale the library refuses surfaces as an exception, and the builder keeps working
        std::vector<double> zero(phi0);
        zero[0] = 0.0;
        bool threw = false;
        try {
            builder.bundleAdjustFocal(begin, members, views, rot, pos, pts, zero, &hasPose);
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) ++bad;
        bad += compare("after an error", builder.bundleAdjustFocal(begin, members, views, rot, pos, pts, phi0, &hasPose), R.data(), c.data(),
                       X.data(), phi.data(), V, T, report.data(), report[7]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return bad ? 1 : 0;
}
