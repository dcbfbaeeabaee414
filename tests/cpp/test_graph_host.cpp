// Host-only driver of csrc/pgi_graph_host.hpp (no GPU, no HIP): the shared spanning forest against a plain std::stable_sort
// Kruskal, and the incidence CSR with both signs against a brute-force construction.  Prints one line per case; exit status
// 0 = all cases agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "pgi_graph_host.hpp"

namespace {
struct Graph {
    std::string name;
    uint32_t V;
    std::vector<uint32_t> src, dst;
    std::vector<double> w;
};

// Kruskal over (weight desc, edge index asc) by a stable sort on the weights alone
std::vector<uint32_t> kruskal_stable_sort(const Graph& g) {
    const uint32_t nE = (uint32_t)g.src.size();
    std::vector<uint32_t> order(nE), parent(g.V), tree;
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return g.w[a] > g.w[b]; });
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t a) {
        while (parent[a] != a) a = parent[a];
        return a;
    };
    for (uint32_t e : order) {
        const uint32_t a = find(g.src[e]), b = find(g.dst[e]);
        if (a == b) continue;
        parent[std::max(a, b)] = std::min(a, b);
        tree.push_back(e);
    }
    return tree;
}

Graph random_graph(const char* name, uint32_t V, uint32_t E, uint32_t seed, int weight_kind, uint32_t components = 1) {
    Graph g{name, V, {}, {}, {}};
    std::mt19937 rng(seed);
    const double levels[4] = {0.25, 0.5, 0.5, 1.0};
    while (g.src.size() < E) {
        uint32_t a = rng() % V, b = rng() % V;
        if (components > 1) b = b - b % components + a % components;  // stay inside a's residue class
        if (b >= V || a == b) continue;
        g.src.push_back(a);
        g.dst.push_back(b);
        double w;
        switch (weight_kind) {
            case 0: w = levels[rng() % 4]; break;                                             // many ties
            case 1: w = (rng() % 3 == 0) ? 0.7 : ((rng() & 1) ? 0.0 : -0.0); break;           // +0.0 and -0.0 mixed
            case 2: w = 1.0; break;                                                           // all equal
            default: w = (double)(rng() % 100000) / 100000.0 + 1e-9 * (double)(rng() % 7);    // mostly distinct
        }
        g.w.push_back(w);
    }
    return g;
}

bool check_forest(const Graph& g) {
    std::vector<uint32_t> tree;
    std::vector<std::vector<pgi::ForestEdge>> adj;
    pgi::spanning_forest(g.V, g.src.data(), g.dst.data(), g.w.data(), (uint32_t)g.src.size(), tree, adj);
    const std::vector<uint32_t> expect = kruskal_stable_sort(g);
    bool ok = tree == expect && adj.size() == g.V;
    // the adjacency holds every forest edge once from each end, in the order the edges were taken
    std::vector<std::vector<pgi::ForestEdge>> expect_adj(g.V);
    for (uint32_t e : expect) {
        expect_adj[g.src[e]].push_back({e, g.dst[e]});
        expect_adj[g.dst[e]].push_back({e, g.src[e] | 0x80000000u});
    }
    for (uint32_t v = 0; ok && v < g.V; ++v) {
        ok = adj[v].size() == expect_adj[v].size();
        for (size_t i = 0; ok && i < adj[v].size(); ++i) ok = adj[v][i].edge == expect_adj[v][i].edge && adj[v][i].other == expect_adj[v][i].other;
    }
    std::printf("forest %-24s V %5u E %6zu tree %5zu %s\n", g.name.c_str(), g.V, g.src.size(), tree.size(), ok ? "ok" : "MISMATCH");
    return ok;
}

bool check_csr(const Graph& g, int8_t sign_of_src) {
    const uint32_t nE = (uint32_t)g.src.size();
    const pgi::IncidenceCsr c = pgi::build_incidence_csr(g.V, nE, g.src.data(), g.dst.data(), sign_of_src);
    bool ok = c.ptr.size() == (size_t)g.V + 1 && c.ptr[0] == 0 && c.ptr[g.V] == 2 * nE && c.edge.size() == 2 * (size_t)nE &&
              c.other.size() == c.edge.size() && c.sign.size() == c.edge.size();
    for (uint32_t v = 0; ok && v < g.V; ++v) {  // brute force: every edge asked whether it touches v, in edge order
        uint32_t a = c.ptr[v];
        for (uint32_t e = 0; ok && e < nE; ++e) {
            if (g.src[e] == v) {
                ok = a < c.ptr[v + 1] && c.edge[a] == e && c.other[a] == g.dst[e] && c.sign[a] == sign_of_src;
                ++a;
            }
            if (ok && g.dst[e] == v) {
                ok = a < c.ptr[v + 1] && c.edge[a] == e && c.other[a] == g.src[e] && c.sign[a] == -sign_of_src;
                ++a;
            }
        }
        ok = ok && a == c.ptr[v + 1];
    }
    std::printf("csr    %-24s sign %+d %s\n", g.name.c_str(), (int)sign_of_src, ok ? "ok" : "MISMATCH");
    return ok;
}
}  // namespace

int main() {
    std::vector<Graph> graphs;
    graphs.push_back(random_graph("many_ties", 300, 2400, 1, 0));
    graphs.push_back(random_graph("signed_zeros", 200, 1500, 2, 1));
    graphs.push_back(random_graph("all_equal", 257, 1800, 3, 2));
    graphs.push_back(random_graph("distinct", 1000, 9000, 4, 3));
    graphs.push_back(random_graph("disconnected", 300, 1200, 5, 0, 3));
    graphs.push_back(random_graph("sparse_with_isolated", 400, 150, 6, 3));
    graphs.push_back(Graph{"one_view", 1, {}, {}, {}});
    graphs.push_back(Graph{"no_edges", 7, {}, {}, {}});
    graphs.push_back(Graph{"parallel_edges", 3, {0, 1, 0, 1, 2}, {1, 0, 1, 2, 1}, {0.5, 0.5, 0.5, -0.0, 0.0}});
    bool ok = true;
    for (const Graph& g : graphs) {
        ok &= check_forest(g);
        ok &= check_csr(g, -1);
        ok &= check_csr(g, +1);
    }
    std::printf("%s\n", ok ? "all ok" : "FAILED");
    return ok ? 0 : 1;
}
