// PoseGraphBuilder::bundleAdjust (host/pose_graph_builder.hpp), both forms, checked bit for bit against the numbers the
// Python engine computed for the same tracks (tests/test_bundle_cpp.py drives this program).
//   test_bundle <input file>
// input (little endian): u32 V; per view: u32 n, f64 f, w, h, R[9], c[3], u8 has_pose, f32 xy[2 n];
//   u32 T, u32 begin[T + 1], u64 members[begin[T]];
//   expected: f64 R[9 V], c[3 V], X[3 T], u32 report[7] (iters, accepted, cg_iters_total, stop_reason, n_obs, n_points, n_free_cams)
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

static bool sameBits(const double* a, const double* b, size_t n) {  // NaN == NaN, everything else by value
    for (size_t i = 0; i < n; ++i)
        if (!((a[i] != a[i] && b[i] != b[i]) || std::memcmp(&a[i], &b[i], 8) == 0)) return false;
    return true;
}

static int compare(const char* what, const PoseGraphBuilder::BundleAdjustment& got, const double* R, const double* c, const double* X,
                   size_t V, size_t T, const uint32_t* report) {
    int bad = 0;
    if (got.rotations.rotations.size() != V || got.positions.positions.size() != V || got.points.size() != T) ++bad;
    for (size_t v = 0; !bad && v < V; ++v)
        if (!sameBits(got.rotations.rotations[v].data(), R + 9 * v, 9) || !sameBits(got.positions.positions[v].data(), c + 3 * v, 3)) ++bad;
    if (!bad && T && !sameBits(got.points[0].data(), X, 3 * T)) ++bad;
    const pgi_bundle_report& r = got.report;
    const uint32_t mine[7] = {r.iters, r.accepted, r.cg_iters_total, r.stop_reason, r.n_obs, r.n_points, r.n_free_cams};
    if (report && std::memcmp(mine, report, sizeof mine) != 0) ++bad;
    std::printf("%s: %zu views, %zu tracks, %u accepted of %u, %s\n", what, V, T, r.accepted, r.iters, bad ? "MISMATCH" : "identical");
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
    rot.rotations.resize(V);
    pos.positions.resize(V);
    for (uint32_t v = 0; v < V; ++v) {
        const uint32_t n = take<uint32_t>(in, 1)[0];
        const std::vector<double> k = take<double>(in, 3 + 9 + 3);
        hasPose[v] = take<uint8_t>(in, 1)[0];
        xy[v] = take<float>(in, 2 * (size_t)n);
        views[v].keypoints = xy[v].data();
        views[v].n = n;
        views[v].focalLength = k[0], views[v].width = k[1], views[v].height = k[2];
        std::memcpy(rot.rotations[v].data(), &k[3], 72);
        std::memcpy(pos.positions[v].data(), &k[12], 24);
    }
    const uint32_t T = take<uint32_t>(in, 1)[0];
    const std::vector<uint32_t> begin = take<uint32_t>(in, (size_t)T + 1);
    const std::vector<uint64_t> members = take<uint64_t>(in, begin[T]);
    const std::vector<double> R = take<double>(in, 9 * (size_t)V), c = take<double>(in, 3 * (size_t)V), X = take<double>(in, 3 * (size_t)T);
    const std::vector<uint32_t> report = take<uint32_t>(in, 7);
    if (!in) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    int bad = 0;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.5, 0.4, "", "", "", "", true, true, true);
        pgi_triangulate_params tri;
        pgi_default_triangulate_params(&tri);
        tri.thr_px = 8.0;  // the poses are perturbed: the triangulation of tests/bundle_spec.py make_problem
        // (1) offsets and members as written by the scene
        const PoseGraphBuilder::TriangulatedPoints pts = builder.triangulateTracks(begin, members, views, rot, pos, &hasPose, &tri);
        bad += compare("arrays", builder.bundleAdjust(begin, members, views, rot, pos, pts, &hasPose), R.data(), c.data(), X.data(), V, T,
                       report.data());
        // (2) a host-only store grown from the same tracks gives the store's own track order; its refinement must equal the
        //     array call on the tracks read back from it
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
        const PoseGraphBuilder::TriangulatedPoints spts = builder.triangulateTracks(store, views, rot, pos, &hasPose, &tri);
        const PoseGraphBuilder::BundleAdjustment viaArrays = builder.bundleAdjust(sb, sm, views, rot, pos, spts, &hasPose);
        const PoseGraphBuilder::BundleAdjustment viaStore = builder.bundleAdjust(store, views, rot, pos, spts, &hasPose);
        std::vector<double> sR(9 * (size_t)V), sc(3 * (size_t)V), sX(3 * viaArrays.points.size());
        for (uint32_t v = 0; v < V; ++v) {
            std::memcpy(&sR[9 * v], viaArrays.rotations.rotations[v].data(), 72);
            std::memcpy(&sc[3 * v], viaArrays.positions.positions[v].data(), 24);
        }
        if (!sX.empty()) std::memcpy(sX.data(), viaArrays.points[0].data(), sX.size() * 8);
        const pgi_bundle_report& r = viaArrays.report;
        const uint32_t rep[7] = {r.iters, r.accepted, r.cg_iters_total, r.stop_reason, r.n_obs, r.n_points, r.n_free_cams};
        bad += compare("host store", viaStore, sR.data(), sc.data(), sX.data(), V, viaArrays.points.size(), rep);
        if (viaStore.report.accepted == 0 || viaStore.report.n_points == 0) {
            std::printf("host store: nothing refined\n");
            ++bad;
        }
        // (3) a parameter the library refuses surfaces as an exception, and the builder keeps working
        pgi_bundle_params prm;
        pgi_default_bundle_params(&prm);
        prm.huber_px = 0.0;
        bool threw = false;
        try {
            builder.bundleAdjust(begin, members, views, rot, pos, pts, &hasPose, nullptr, &prm);
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) ++bad;
        bad += compare("after an error", builder.bundleAdjust(begin, members, views, rot, pos, pts, &hasPose), R.data(), c.data(), X.data(), V, T,
                       report.data());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return bad ? 1 : 0;
}
