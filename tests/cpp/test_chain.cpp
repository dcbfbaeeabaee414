// PoseGraphBuilder::estimateAndAverage with positions_out (host/pose_graph_builder.hpp) on the correspondences of the chain
// scene; the results are written out and tests/test_chain_cpp.py demands that they are the bits of the Python engine's chain
// (estimate_pose_batch -> rotation_average_edges -> translation_average_edges) on the same rows, seed and parameters.
//   test_chain <input file> <output file>
// input (little endian): u32 V, P, seed, 0; per pair u32 src, dst, n; f64 normalised threshold; f64 rows[n][4]
// output: two records of  u32 rotation iterations, rotation edgesUsed, translation iterations, translation edgesUsed;
//         f64 R[9 V]; f64 c[3 V]:
//   (1) estimateAndAverage(..., &positions), followed by its pgi_edge records [P] (200 bytes each)
//   (2) averageRotations on the pose graph that call filled, then the device-table overload of averageTranslations on the
//       uploaded records with those rotations
// Checked here: (1) == (2) bit for bit; P = 0 and numViews = 0 give identities and zeros (numViews = 0: empty vectors).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include <hip/hip_runtime.h>

#include "pose_graph_builder.hpp"

using namespace reconstruction;

static void put(std::ofstream& out, const PoseGraphBuilder::GlobalRotations& r, const PoseGraphBuilder::GlobalPositions& p) {
    const uint32_t head[4] = {r.iterations, r.edgesUsed, p.iterations, p.edgesUsed};
    out.write(reinterpret_cast<const char*>(head), sizeof head);
    out.write(reinterpret_cast<const char*>(r.rotations.data()), (std::streamsize)(r.rotations.size() * sizeof(Matrix3d)));
    out.write(reinterpret_cast<const char*>(p.positions.data()), (std::streamsize)(p.positions.size() * sizeof(Vector3d)));
}

static bool sameBits(const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    uint32_t head[4];
    in.read(reinterpret_cast<char*>(head), sizeof head);
    const uint32_t V = head[0], P = head[1];
    const uint64_t seed = head[2];
    std::vector<PoseGraphBuilder::ViewPair> pairs(P);
    for (uint32_t i = 0; i < P; ++i) {
        uint32_t s, d, n;
        double thr;
        in.read((char*)&s, 4); in.read((char*)&d, 4); in.read((char*)&n, 4); in.read((char*)&thr, 8);
        pairs[i].src = s; pairs[i].dst = d; pairs[i].similarity = 1.0; pairs[i].normalizedThreshold = thr;
        pairs[i].correspondences = CorrespondenceMatrix((int)n);
        if (n) in.read((char*)pairs[i].correspondences.ptr(), (std::streamsize)((size_t)n * 32));
    }
    if (!in) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    int bad = 0;
    pgi_edge* d_table = nullptr;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.05, 0.4, "", "", "", "", false, true, true);
        std::ofstream out(argv[2], std::ios::binary);
        // (1) one call: estimate -> rotation averaging -> translation averaging on the device table
        PoseGraph graph;
        std::vector<pgi_edge> edges;
        PoseGraphBuilder::GlobalPositions pos;
        const PoseGraphBuilder::GlobalRotations rot = builder.estimateAndAverage(pairs, graph, V, seed, &edges, nullptr, &pos, nullptr);
        size_t ok = 0;
        for (const pgi_edge& e : edges) ok += e.status == PGI_EDGE_OK;
        if (edges.size() != P || rot.rotations.size() != V || pos.positions.size() != V || rot.edgesUsed != ok || pos.edgesUsed != ok ||
            graph.numEdges() != ok)
            ++bad;
        put(out, rot, pos);
        out.write(reinterpret_cast<const char*>(edges.data()), (std::streamsize)(edges.size() * sizeof(pgi_edge)));
        // (2) the same in separate calls: the graph's edges, then the uploaded records with the rotations just returned
        const PoseGraphBuilder::GlobalRotations rot2 = builder.averageRotations(graph, V);
        if (hipMalloc((void**)&d_table, (size_t)(P ? P : 1) * sizeof(pgi_edge)) != hipSuccess ||
            hipMemcpy(d_table, edges.data(), (size_t)P * sizeof(pgi_edge), hipMemcpyHostToDevice) != hipSuccess) {
            std::fprintf(stderr, "upload of the edge table failed\n");
            return 3;
        }
        std::vector<uint32_t> src(P), dst(P), rows(P);
        for (uint32_t i = 0; i < P; ++i) {
            src[i] = (uint32_t)pairs[i].src;
            dst[i] = (uint32_t)pairs[i].dst;
            rows[i] = (uint32_t)pairs[i].correspondences.rows;
        }
        const PoseGraphBuilder::GlobalPositions pos2 = builder.averageTranslations(d_table, src, dst, &rows, V, rot2, nullptr);
        put(out, rot2, pos2);
        const bool sameR = rot2.rotations.size() == V && sameBits(rot2.rotations.data(), rot.rotations.data(), (size_t)V * sizeof(Matrix3d));
        const bool sameC = pos2.positions.size() == V && sameBits(pos2.positions.data(), pos.positions.data(), (size_t)V * sizeof(Vector3d));
        const bool sameN = rot2.iterations == rot.iterations && rot2.edgesUsed == rot.edgesUsed && pos2.iterations == pos.iterations &&
                           pos2.edgesUsed == pos.edgesUsed;
        std::printf("one call: %zu of %u pairs OK, rotations %u iterations, positions %u iterations; separate calls: rotations %s, "
                    "positions %s, counts %s\n", ok, P, rot.iterations, pos.iterations, sameR ? "same bits" : "DIFFER",
                    sameC ? "same bits" : "DIFFER", sameN ? "equal" : "DIFFER");
        if (!sameR || !sameC || !sameN) ++bad;
        // the empty cases: no pairs -> an identity and a zero per view; no views -> nothing at all
        int empty = 0;
        {
            PoseGraph g0;
            PoseGraphBuilder::GlobalPositions p0;
            p0.iterations = p0.edgesUsed = 77;   // must be reset
            const PoseGraphBuilder::GlobalRotations r0 = builder.estimateAndAverage({}, g0, V, seed, nullptr, nullptr, &p0, nullptr);
            bool good = r0.rotations.size() == V && p0.positions.size() == V && !r0.iterations && !r0.edgesUsed && !p0.iterations && !p0.edgesUsed &&
                        g0.numEdges() == 0;
            const Matrix3d I{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
            const Vector3d Z{{0, 0, 0}};
            for (uint32_t v = 0; good && v < V; ++v) good = sameBits(&r0.rotations[v], &I, sizeof I) && sameBits(&p0.positions[v], &Z, sizeof Z);
            empty += good;
        }
        {
            PoseGraph g0;
            PoseGraphBuilder::GlobalPositions p0;
            p0.positions.assign(3, Vector3d{{1, 2, 3}});   // must be cleared
            const PoseGraphBuilder::GlobalRotations r0 = builder.estimateAndAverage(pairs, g0, 0, seed, nullptr, nullptr, &p0, nullptr);
            empty += r0.rotations.empty() && p0.positions.empty() && !r0.iterations && !r0.edgesUsed && !p0.iterations && !p0.edgesUsed;
        }
        std::printf("empty input: %d of 2 cases give the documented identity and zeros\n", empty);
        if (empty != 2) ++bad;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        (void)hipFree(d_table);
        return 3;
    }
    (void)hipFree(d_table);
    std::printf("%s\n", bad ? "FAILED" : "done");
    return bad ? 1 : 0;
}
