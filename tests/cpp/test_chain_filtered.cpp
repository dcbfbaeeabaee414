// The filtered chain through PoseGraphBuilder (host/pose_graph_builder.hpp) on the correspondences of the filtered chain scene;
// the results are written out and tests/test_chain_filtered_cpp.py demands that they are the bits of the Python engine's chain
// (estimate_pose_batch -> cycle_filter_edges(out=filtered) -> translation_average_edges(filtered)) on the same rows.
//   test_chain_filtered <input file> <output file>
// input (little endian): u32 V, P, seed, 0; per pair u32 src, dst, n; f64 normalised threshold; f64 rows[n][4]; then f64 R[9 V],
//   the global rotations the positions are averaged with.  PoseGraphBuilder has no call that averages the rotations of a
//   device table (averageRotations takes a pose graph), so the rotations of the filtered table come from the caller.
// output: pgi_edge table[P] (estimateAndAverage's records); u8 keep[P]; u32 triangles[P]; u32 goodTriangles[P];
//   u64 n_triangles, n_good, n_skipped_translation; u32 n_ok, n_dropped; pgi_edge filtered[P];
//   u32 translation iterations, edgesUsed; f64 c[3 V]
// Checked here: the input table is untouched by the filter; the filter in place gives the same table as the filter into a
// second buffer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include <hip/hip_runtime.h>

#include "pose_graph_builder.hpp"

using namespace reconstruction;

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
    PoseGraphBuilder::GlobalRotations rot;
    rot.rotations.resize(V);
    in.read(reinterpret_cast<char*>(rot.rotations.data()), (std::streamsize)((size_t)V * sizeof(Matrix3d)));
    if (!in || P == 0 || V == 0) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    int bad = 0;
    pgi_edge *d_table = nullptr, *d_filtered = nullptr;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.05, 0.4, "", "", "", "", false, true, true);
        std::ofstream out(argv[2], std::ios::binary);
        PoseGraph graph;
        std::vector<pgi_edge> edges;
        PoseGraphBuilder::GlobalPositions unfilteredPos;
        builder.estimateAndAverage(pairs, graph, V, seed, &edges, nullptr, &unfilteredPos, nullptr);
        if (edges.size() != P) ++bad;
        const size_t bytes = (size_t)P * sizeof(pgi_edge);
        if (hipMalloc((void**)&d_table, bytes) != hipSuccess || hipMalloc((void**)&d_filtered, bytes) != hipSuccess ||
            hipMemcpy(d_table, edges.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_filtered, 0, bytes) != hipSuccess) {
            std::fprintf(stderr, "upload of the edge table failed\n");
            return 3;
        }
        std::vector<uint32_t> src(P), dst(P), rows(P);
        for (uint32_t i = 0; i < P; ++i) {
            src[i] = (uint32_t)pairs[i].src;
            dst[i] = (uint32_t)pairs[i].dst;
            rows[i] = (uint32_t)pairs[i].correspondences.rows;
        }
        const PoseGraphBuilder::CycleFilterResult f = builder.filterEdgesByCycles(d_table, src, dst, V, nullptr, d_filtered);
        std::vector<pgi_edge> after(P), filtered(P), inPlace(P);
        if (hipMemcpy(after.data(), d_table, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(filtered.data(), d_filtered, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return 3;
        const bool untouched = std::memcmp(after.data(), edges.data(), bytes) == 0;
        if (f.keep.size() != P || f.triangles.size() != P || f.goodTriangles.size() != P) ++bad;
        const PoseGraphBuilder::GlobalPositions pos = builder.averageTranslations(d_filtered, src, dst, &rows, V, rot, nullptr);
        // the filter in place: the same table
        const PoseGraphBuilder::CycleFilterResult g = builder.filterEdgesByCycles(d_table, src, dst, V, nullptr, d_table);
        if (hipMemcpy(inPlace.data(), d_table, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        const bool sameTable = std::memcmp(inPlace.data(), filtered.data(), bytes) == 0 && g.keep == f.keep;
        size_t kept = 0;
        for (const pgi_edge& e : filtered) kept += e.status == PGI_EDGE_OK;
        std::printf("filter: %u of %u OK records dropped, %zu kept; input table %s; in place %s; positions %u iterations, %u edges used\n",
                    f.summary.n_dropped, f.summary.n_ok, kept, untouched ? "untouched" : "CHANGED", sameTable ? "same table" : "DIFFERS",
                    pos.iterations, pos.edgesUsed);
        if (!untouched || !sameTable || pos.edgesUsed != kept || pos.positions.size() != V) ++bad;
        out.write(reinterpret_cast<const char*>(edges.data()), (std::streamsize)bytes);
        out.write(reinterpret_cast<const char*>(f.keep.data()), (std::streamsize)P);
        out.write(reinterpret_cast<const char*>(f.triangles.data()), (std::streamsize)((size_t)P * 4));
        out.write(reinterpret_cast<const char*>(f.goodTriangles.data()), (std::streamsize)((size_t)P * 4));
        const uint64_t s64[3] = {f.summary.n_triangles, f.summary.n_good, f.summary.n_skipped_translation};
        const uint32_t s32[2] = {f.summary.n_ok, f.summary.n_dropped};
        out.write(reinterpret_cast<const char*>(s64), sizeof s64);
        out.write(reinterpret_cast<const char*>(s32), sizeof s32);
        out.write(reinterpret_cast<const char*>(filtered.data()), (std::streamsize)bytes);
        const uint32_t h2[2] = {pos.iterations, pos.edgesUsed};
        out.write(reinterpret_cast<const char*>(h2), sizeof h2);
        out.write(reinterpret_cast<const char*>(pos.positions.data()), (std::streamsize)(pos.positions.size() * sizeof(Vector3d)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        (void)hipFree(d_table);
        (void)hipFree(d_filtered);
        return 3;
    }
    (void)hipFree(d_table);
    (void)hipFree(d_filtered);
    std::printf("%s\n", bad ? "FAILED" : "done");
    return bad ? 1 : 0;
}
