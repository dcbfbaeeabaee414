// PoseGraphBuilder::triangulateTracks (host/pose_graph_builder.hpp) on a ground-truth scene, checked bit for bit against
// the numbers tests/triangulate_spec.py wrote (tests/test_triangulate_cpp.py drives this program).
//   test_triangulate <input file>
// input (little endian): u32 V; per view: u32 n, f64 f, w, h, R[9], c[3], u8 has_pose, f32 xy[2 n];
//   u32 T, u32 begin[T + 1], u64 members[begin[T]];
//   expected: f64 X[3 T], u8 status[T], f64 err[T], u32 n_used[T], u8 obs_state[begin[T]], u32 counts[6]
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

static int compare(const char* what, const PoseGraphBuilder::TriangulatedPoints& got, const std::vector<double>& X,
                   const std::vector<uint8_t>& status, const std::vector<double>& err, const std::vector<uint32_t>& used,
                   const std::vector<uint8_t>& state, const uint32_t* counts) {
    int bad = 0;
    const size_t T = status.size();
    if (got.points.size() != T || got.status != status || got.viewsUsed != used || got.observationState != state) ++bad;
    if (!bad && T && !sameBits(got.points[0].data(), X.data(), 3 * T)) ++bad;
    if (!bad && T && !sameBits(got.rmsError.data(), err.data(), T)) ++bad;
    if (counts && std::memcmp(got.counts.data(), counts, PGI_TRI_STATUS_COUNT * 4) != 0) ++bad;
    std::printf("%s: %zu tracks, %s\n", what, T, bad ? "MISMATCH" : "identical");
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
    const size_t M = begin[T];
    const std::vector<uint64_t> members = take<uint64_t>(in, M);
    const std::vector<double> X = take<double>(in, 3 * (size_t)T);
    const std::vector<uint8_t> status = take<uint8_t>(in, T);
    const std::vector<double> err = take<double>(in, T);
    const std::vector<uint32_t> used = take<uint32_t>(in, T);
    const std::vector<uint8_t> state = take<uint8_t>(in, M);
    const std::vector<uint32_t> counts = take<uint32_t>(in, PGI_TRI_STATUS_COUNT);
    if (!in) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    int bad = 0;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.5, 0.4, "", "", "", "", true, true, true);
        // (1) offsets and members as written by the specification's scene
        bad += compare("arrays", builder.triangulateTracks(begin, members, views, rot, pos, &hasPose), X, status, err, used, state,
                       counts.data());
        // (2) a host-only store grown from the same tracks (consecutive members as matches) gives the store's own track order;
        //     its triangulation must equal the array call on the tracks read back from it
        Tracklets store(V);
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t m = begin[t]; m + 1 < begin[t + 1]; ++m) {
                const uint64_t a = members[m], b = members[m + 1];
                if ((a >> 32) == (b >> 32)) continue;  // the store takes matches between two different views
                if ((a >> 32) >= V || (b >> 32) >= V || (uint32_t)a >= views[a >> 32].n || (uint32_t)b >= views[b >> 32].n) continue;
                store.add((size_t)(a >> 32), (size_t)(b >> 32), {Tracklets::Match((size_t)(uint32_t)a, (size_t)(uint32_t)b, 0.0)}, {1});
            }
        std::vector<uint32_t> sb(1, 0);
        std::vector<uint64_t> sm;
        for (size_t t = 0; t < store.trackNumber(); ++t) {
            for (const Tracklets::Pair& p : store.track(t)) sm.push_back(((uint64_t)p.first << 32) | (uint64_t)(uint32_t)p.second);
            sb.push_back((uint32_t)sm.size());
        }
        const PoseGraphBuilder::TriangulatedPoints viaArrays = builder.triangulateTracks(sb, sm, views, rot, pos, &hasPose);
        const PoseGraphBuilder::TriangulatedPoints viaStore = builder.triangulateTracks(store, views, rot, pos, &hasPose);
        std::vector<double> sx(3 * viaArrays.points.size());
        if (!sx.empty()) std::memcpy(sx.data(), viaArrays.points[0].data(), sx.size() * 8);
        bad += compare("host store", viaStore, sx, viaArrays.status, viaArrays.rmsError, viaArrays.viewsUsed, viaArrays.observationState,
                       viaArrays.counts.data());
        if (store.trackNumber() == 0 || viaStore.counts[PGI_TRI_OK] == 0) {
            std::printf("host store: no track triangulated\n");
            ++bad;
        }
        // (3) a parameter the library refuses surfaces as an exception, and the builder keeps working
        pgi_triangulate_params prm;
        pgi_default_triangulate_params(&prm);
        prm.min_views = 1;
        bool threw = false;
        try {
            builder.triangulateTracks(begin, members, views, rot, pos, &hasPose, &prm);
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) ++bad;
        bad += compare("after an error", builder.triangulateTracks(begin, members, views, rot, pos, &hasPose), X, status, err, used, state,
                       counts.data());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return bad ? 1 : 0;
}
