// PoseGraphBuilder::filterEdgesByCycles (host/pose_graph_builder.hpp), both overloads, checked against the integers
// tests/cycle_spec.py wrote (tests/test_cycle_cpp.py drives this program).
//   test_cycle <input file>
// input (little endian): u32 V, P; u32 src[P], dst[P]; pgi_edge rec[P] (200 bytes each);
//   expected: u8 keep[P], u32 n_tri[P], u32 n_good[P], pgi_cycle_summary (u64 triangles, good, skipped; u32 ok, dropped)
#include <cstdint>
#include <cstdio>
#include <cstring>
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

template <class T>
static int same(const char* form, const char* what, const std::vector<T>& got, const std::vector<T>& want) {
    const bool ok = got == want;
    std::printf("%s: %s %s (%zu entries)\n", form, what, ok ? "identical" : "MISMATCH", want.size());
    return ok ? 0 : 1;
}

static int sameSummary(const char* form, const pgi_cycle_summary& got, const pgi_cycle_summary& want) {
    const bool ok = got.n_triangles == want.n_triangles && got.n_good == want.n_good &&
                    got.n_skipped_translation == want.n_skipped_translation && got.n_ok == want.n_ok && got.n_dropped == want.n_dropped;
    std::printf("%s: summary %s (%llu triangles, %llu good, %u of %u records dropped)\n", form, ok ? "identical" : "MISMATCH",
                (unsigned long long)got.n_triangles, (unsigned long long)got.n_good, got.n_dropped, got.n_ok);
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<uint32_t> head = take<uint32_t>(in, 2);
    const uint32_t V = head[0], P = head[1];
    const std::vector<uint32_t> src = take<uint32_t>(in, P), dst = take<uint32_t>(in, P);
    const std::vector<pgi_edge> rec = take<pgi_edge>(in, P);
    const std::vector<uint8_t> keep = take<uint8_t>(in, P);
    const std::vector<uint32_t> nTri = take<uint32_t>(in, P), nGood = take<uint32_t>(in, P);
    const pgi_cycle_summary summary = take<pgi_cycle_summary>(in, 1)[0];
    if (!in) {
        std::fprintf(stderr, "short input file\n");
        return 2;
    }
    int bad = 0;
    pgi_edge *d_table = nullptr, *d_out = nullptr;
    try {
        PoseGraphBuilder builder(20, 5000, 5, 100, 20, 50, 100, 0.8, 0.5, 0.4, "", "", "", "", true, true, true);
        // (1) the OK records as the edges of a pose graph, in insertion order
        PoseGraph graph;
        for (uint32_t v = 0; v < V; ++v) graph.addVertex(v);
        std::vector<uint8_t> keepOk;
        std::vector<uint32_t> triOk, goodOk;
        for (uint32_t p = 0; p < P; ++p) {
            if (rec[p].status != PGI_EDGE_OK) continue;
            SE3d T;
            for (int c = 0; c < 9; ++c) T.R[c] = rec[p].R[c];
            for (int c = 0; c < 3; ++c) T.t[c] = rec[p].t[c];
            if (!graph.addEdge(src[p], dst[p], Pose(T), 1.0)) ++bad;
            keepOk.push_back(keep[p]);
            triOk.push_back(nTri[p]);
            goodOk.push_back(nGood[p]);
        }
        const PoseGraphBuilder::CycleFilterResult viaGraph = builder.filterEdgesByCycles(graph, V);
        bad += same("graph", "keep", viaGraph.keep, keepOk) + same("graph", "n_tri", viaGraph.triangles, triOk) +
               same("graph", "n_good", viaGraph.goodTriangles, goodOk) + sameSummary("graph", viaGraph.summary, summary);
        // (2) the same records as a device-resident table, written out filtered
        if (hipMalloc((void**)&d_table, (size_t)P * sizeof(pgi_edge) + 1) != hipSuccess ||
            hipMalloc((void**)&d_out, (size_t)P * sizeof(pgi_edge) + 1) != hipSuccess ||
            hipMemcpy(d_table, rec.data(), (size_t)P * sizeof(pgi_edge), hipMemcpyHostToDevice) != hipSuccess) {
            std::fprintf(stderr, "upload of the edge table failed\n");
            return 3;
        }
        const PoseGraphBuilder::CycleFilterResult viaTable = builder.filterEdgesByCycles(d_table, src, dst, V, nullptr, d_out);
        bad += same("table", "keep", viaTable.keep, keep) + same("table", "n_tri", viaTable.triangles, nTri) +
               same("table", "n_good", viaTable.goodTriangles, nGood) + sameSummary("table", viaTable.summary, summary);
        std::vector<pgi_edge> want = rec, got(P);
        for (uint32_t p = 0; p < P; ++p)
            if (rec[p].status == PGI_EDGE_OK && !keep[p]) want[p].status = PGI_EDGE_INCONSISTENT;
        if (hipMemcpy(got.data(), d_out, (size_t)P * sizeof(pgi_edge), hipMemcpyDeviceToHost) != hipSuccess) return 3;
        const bool tableOk = !P || std::memcmp(got.data(), want.data(), (size_t)P * sizeof(pgi_edge)) == 0;
        std::printf("table: filtered records %s\n", tableOk ? "identical" : "MISMATCH");
        bad += tableOk ? 0 : 1;
        // (3) a parameter the library refuses surfaces as an exception, and the builder keeps working
        pgi_cycle_params prm;
        pgi_default_cycle_params(&prm);
        prm.min_good = 0;
        bool threw = false;
        try {
            builder.filterEdgesByCycles(d_table, src, dst, V, &prm);
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) ++bad;
        const PoseGraphBuilder::CycleFilterResult again = builder.filterEdgesByCycles(d_table, src, dst, V);
        bad += same("after an error", "keep", again.keep, keep);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        (void)hipFree(d_table);
        (void)hipFree(d_out);
        return 3;
    }
    (void)hipFree(d_table);
    (void)hipFree(d_out);
    return bad ? 1 : 0;
}
