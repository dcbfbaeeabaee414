// PoseGraphBuilder::averageTranslations (host/pose_graph_builder.hpp), both overloads, on a ground-truth scene; the results
// are written out and tests/test_transavg_cpp.py demands that they equal the Python engine's on the same input bit for bit.
//   test_transavg <input file> <output file>
// input (little endian): u32 V, P, iters, cg_iters; u32 src[P], dst[P], rows[P]; pgi_edge rec[P] (200 bytes each);
//   f64 R_global[9 V] (world->camera, row-major)
// output: three records of f64 c[3 V], u32 iterations, u32 edgesUsed:
//   (1) the pose-graph overload (an edge per OK record, score = n_inl / rows),
//   (2) the device-table overload with the row counts, (3) the same without them (rows = nullptr)
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <vector>

#include <hip/hip_runtime.h>

#include "pose_graph_builder.hpp"

using namespace reconstruction;

template <class T>
static std::vector<T> take(std::ifstream& in, size_t n) {
    std::vector<T> v(n);
    if (n) in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    return v;
}

static void put(std::ofstream& out, const PoseGraphBuilder::GlobalPositions& p) {
    out.write(reinterpret_cast<const char*>(p.positions.data()), (std::streamsize)(p.positions.size() * sizeof(Vector3d)));
    out.write(reinterpret_cast<const char*>(&p.iterations), 4);
    out.write(reinterpret_cast<const char*>(&p.edgesUsed), 4);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<uint32_t> head = take<uint32_t>(in, 4);
    const uint32_t V = head[0], P = head[1];
    const std::vector<uint32_t> src = take<uint32_t>(in, P), dst = take<uint32_t>(in, P), rows = take<uint32_t>(in, P);
    const std::vector<pgi_edge> rec = take<pgi_edge>(in, P);
    PoseGraphBuilder::GlobalRotations rot;
    rot.rotations = take<Matrix3d>(in, V);
    if (!in) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    pgi_transavg_params prm;
    pgi_default_transavg_params(&prm);
    prm.iters = head[2];
    prm.cg_iters = head[3];
    int bad = 0;
    pgi_edge* d_table = nullptr;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.5, 0.4, "", "", "", "", true, true, true);
        std::ofstream out(argv[2], std::ios::binary);
        // (1) the edges already in a pose graph, in insertion order
        PoseGraph graph;
        for (uint32_t v = 0; v < V; ++v) graph.addVertex(v);
        size_t ok = 0;
        for (uint32_t p = 0; p < P; ++p) {
            if (rec[p].status != PGI_EDGE_OK) continue;
            SE3d T;
            for (int c = 0; c < 9; ++c) T.R[c] = rec[p].R[c];
            for (int c = 0; c < 3; ++c) T.t[c] = rec[p].t[c];
            if (!graph.addEdge(src[p], dst[p], Pose(T), (double)rec[p].n_inl / (double)rows[p])) ++bad;
            ++ok;
        }
        const PoseGraphBuilder::GlobalPositions viaGraph = builder.averageTranslations(graph, V, rot, &prm);
        if (viaGraph.positions.size() != V || viaGraph.edgesUsed != ok) ++bad;
        put(out, viaGraph);
        // (2), (3) the same records as a device-resident table
        if (hipMalloc((void**)&d_table, (size_t)P * sizeof(pgi_edge)) != hipSuccess ||
            hipMemcpy(d_table, rec.data(), (size_t)P * sizeof(pgi_edge), hipMemcpyHostToDevice) != hipSuccess) {
            std::fprintf(stderr, "upload of the edge table failed\n");
            return 3;
        }
        const PoseGraphBuilder::GlobalPositions viaTable = builder.averageTranslations(d_table, src, dst, &rows, V, rot, &prm);
        const PoseGraphBuilder::GlobalPositions viaTableUniform = builder.averageTranslations(d_table, src, dst, nullptr, V, rot, &prm);
        if (viaTable.edgesUsed != ok || viaTableUniform.edgesUsed != ok) ++bad;
        put(out, viaTable);
        put(out, viaTableUniform);
        std::printf("graph: %u iterations, %u edges; table: %u iterations, %u of %u records; uniform weights: %u iterations\n",
                    viaGraph.iterations, viaGraph.edgesUsed, viaTable.iterations, viaTable.edgesUsed, P, viaTableUniform.iterations);
        // a rotations vector of the wrong length is refused by both overloads before anything reaches the library
        PoseGraphBuilder::GlobalRotations fewer = rot;
        fewer.rotations.pop_back();
        int refused = 0;
        try {
            builder.averageTranslations(graph, V, fewer, &prm);
        } catch (const std::invalid_argument&) {
            ++refused;
        }
        try {
            builder.averageTranslations(d_table, src, dst, &rows, V, fewer, &prm);
        } catch (const std::invalid_argument&) {
            ++refused;
        }
        std::printf("wrong number of rotations: %d of 2 calls threw std::invalid_argument\n", refused);
        if (refused != 2) ++bad;
        // ... and the builder keeps working
        const PoseGraphBuilder::GlobalPositions again = builder.averageTranslations(d_table, src, dst, &rows, V, rot, &prm);
        if (again.positions != viaTable.positions || again.iterations != viaTable.iterations) ++bad;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        (void)hipFree(d_table);
        return 3;
    }
    (void)hipFree(d_table);
    std::printf("%s\n", bad ? "FAILED" : "done");
    return bad ? 1 : 0;
}
