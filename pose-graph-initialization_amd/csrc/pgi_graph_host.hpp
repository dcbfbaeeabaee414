// pgi_graph_host.hpp -- host-side graph preparation shared by the averaging solvers: the incidence CSR, the maximum-weight
// spanning forest, and the orderings the rotation solve's preconditioners are planned from.  Pure host code (no HIP): it
// compiles with a plain C++ compiler and is tested by tests/cpp/test_graph_host.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

namespace pgi {

// ptr[V + 1]; edge / other / sign per incidence, a view's incidences in edge order.  sign: +-sign_of_src where the view is
// the edge's src, the opposite where it is its dst.
struct IncidenceCsr {
    std::vector<uint32_t> ptr, edge, other;
    std::vector<int8_t> sign;
};
inline IncidenceCsr build_incidence_csr(uint32_t V, uint32_t E, const uint32_t* src, const uint32_t* dst, int8_t sign_of_src) {
    IncidenceCsr g;
    g.ptr.assign((size_t)V + 1, 0);
    g.edge.resize(2 * (size_t)E);
    g.other.resize(2 * (size_t)E);
    g.sign.resize(2 * (size_t)E);
    for (uint32_t e = 0; e < E; ++e) {
        ++g.ptr[src[e] + 1];
        ++g.ptr[dst[e] + 1];
    }
    for (uint32_t k = 0; k < V; ++k) g.ptr[k + 1] += g.ptr[k];
    std::vector<uint32_t> fill(g.ptr.begin(), g.ptr.end() - 1);
    for (uint32_t e = 0; e < E; ++e) {
        uint32_t a = fill[src[e]]++;
        g.edge[a] = e; g.other[a] = dst[e]; g.sign[a] = sign_of_src;
        a = fill[dst[e]]++;
        g.edge[a] = e; g.other[a] = src[e]; g.sign[a] = (int8_t)-sign_of_src;
    }
    return g;
}

// ---- maximum-weight spanning forest ---------------------------------------------------------------------------------------
struct ForestEdge {
    uint32_t edge, other;  // other | backwards << 31 (the view is the edge's dst, `other` its src)
};
// Kruskal on (weight desc, edge index asc); returns the forest's edge list and its adjacency
inline void spanning_forest(uint32_t V, const uint32_t* src, const uint32_t* dst, const double* weight, uint32_t nE,
                            std::vector<uint32_t>& tree, std::vector<std::vector<ForestEdge>>& adj) {
    // (weight desc, edge index asc): ONE integer key per edge -- the order-preserving bit pattern of the weight, inverted -- and a
    // stable sort by it
    std::vector<uint64_t> key[2] = {std::vector<uint64_t>(nE), std::vector<uint64_t>(nE)};
    std::vector<uint32_t> idx[2] = {std::vector<uint32_t>(nE), std::vector<uint32_t>(nE)};
    for (uint32_t e = 0; e < nE; ++e) {
        uint64_t u;
        const double wv = weight[e] == 0.0 ? 0.0 : weight[e];  // (-0.0 and +0.0 compare equal: one key)
        memcpy(&u, &wv, 8);
        u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);  // ascending in the value
        key[0][e] = ~u;                                      // descending
        idx[0][e] = e;
    }
    {   // stable least-significant-digit radix sort, 11-bit digits; a digit all keys share is skipped (std::sort of the
        // pairs took 5.8 ms at 10^5 edges)
        constexpr int kBits = 11, kPasses = 6;
        std::vector<uint32_t> hist((size_t)kPasses << kBits, 0);
        for (uint32_t e = 0; e < nE; ++e)
            for (int ps = 0; ps < kPasses; ++ps) ++hist[((size_t)ps << kBits) + ((key[0][e] >> (ps * kBits)) & ((1u << kBits) - 1))];
        int cur = 0;
        for (int ps = 0; ps < kPasses; ++ps) {
            uint32_t* h = &hist[(size_t)ps << kBits];
            bool single = false;
            for (uint32_t b = 0; b < (1u << kBits); ++b) single |= h[b] == nE;
            if (single) continue;
            uint32_t run = 0;
            for (uint32_t b = 0; b < (1u << kBits); ++b) {
                const uint32_t c = h[b];
                h[b] = run;
                run += c;
            }
            const uint64_t* ks = key[cur].data();
            const uint32_t* is = idx[cur].data();
            uint64_t* kd = key[cur ^ 1].data();
            uint32_t* id = idx[cur ^ 1].data();
            for (uint32_t e = 0; e < nE; ++e) {
                const uint32_t pos = h[(ks[e] >> (ps * kBits)) & ((1u << kBits) - 1)]++;
                kd[pos] = ks[e];
                id[pos] = is[e];
            }
            cur ^= 1;
        }
        if (cur) idx[0].swap(idx[1]);
    }
    const std::vector<uint32_t>& order = idx[0];
    std::vector<uint32_t> parent(V);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t a) {
        while (parent[a] != a) {
            parent[a] = parent[parent[a]];
            a = parent[a];
        }
        return a;
    };
    adj.assign(V, {});
    tree.clear();
    for (uint32_t e : order) {
        const uint32_t a = find(src[e]), b = find(dst[e]);
        if (a == b) continue;
        parent[std::max(a, b)] = std::min(a, b);
        adj[src[e]].push_back({e, dst[e]});
        adj[dst[e]].push_back({e, src[e] | 0x80000000u});
        tree.push_back(e);
        if (tree.size() + 1 == V) break;  // spanning: the remaining edges all close cycles
    }
}

// ---- the tree path's numbering: views in depth-first preorder of the spanning forest (a subtree is a contiguous range), with
// subtree sizes, the edge to the parent (0xFFFFFFFF: a root) and the Euler-tour positions; the adjacency in that numbering.
struct TreeOrder {
    std::vector<uint32_t> new_to_old, parent_edge, sub_size, tour_enter, tour_exit;
    IncidenceCsr adj;
};
inline TreeOrder plan_tree_order(uint32_t V, const IncidenceCsr& g, const std::vector<uint8_t>& is_root,
                                 const std::vector<std::vector<ForestEdge>>& forest) {
    TreeOrder t;
    std::vector<uint32_t> o2n(V, 0xFFFFFFFFu);
    t.new_to_old.reserve(V);
    t.parent_edge.assign(V, 0xFFFFFFFFu);
    t.sub_size.assign(V, 1u);
    t.tour_enter.assign(V, 0u);
    t.tour_exit.assign(V, 0u);
    uint32_t clock = 0;
    struct Frame { uint32_t v, next; };
    std::vector<Frame> stack;
    for (uint32_t root = 0; root < V; ++root) {
        if (!is_root[root]) continue;
        o2n[root] = (uint32_t)t.new_to_old.size();
        t.new_to_old.push_back(root);
        t.tour_enter[o2n[root]] = clock++;
        stack.assign(1, Frame{root, 0u});
        while (!stack.empty()) {
            Frame& f = stack.back();
            if (f.next < forest[f.v].size()) {
                const ForestEdge& pr = forest[f.v][f.next++];
                const uint32_t c = pr.other & 0x7FFFFFFFu;
                if (o2n[c] != 0xFFFFFFFFu) continue;  // the parent
                o2n[c] = (uint32_t)t.new_to_old.size();
                t.new_to_old.push_back(c);
                t.parent_edge[o2n[c]] = pr.edge;
                t.tour_enter[o2n[c]] = clock++;
                stack.push_back(Frame{c, 0u});
            } else {
                const uint32_t k = o2n[f.v];
                t.sub_size[k] = (uint32_t)t.new_to_old.size() - k;
                t.tour_exit[k] = clock++;
                stack.pop_back();
            }
        }
    }
    const size_t I = g.edge.size();
    t.adj.ptr.assign((size_t)V + 1, 0);
    t.adj.edge.resize(I);
    t.adj.other.resize(I);
    t.adj.sign.resize(I);
    for (uint32_t k = 0; k < V; ++k) {
        const uint32_t u = t.new_to_old[k];
        uint32_t o = t.adj.ptr[k];
        for (uint32_t a = g.ptr[u]; a < g.ptr[u + 1]; ++a, ++o) {
            t.adj.edge[o] = g.edge[a];
            t.adj.other[o] = o2n[g.other[a]];
            t.adj.sign[o] = g.sign[a];
        }
        t.adj.ptr[k + 1] = o;
    }
    return t;
}

// ---- the aggregates of the two-level preconditioner and the renumbered adjacency ------------------------------------------
constexpr uint8_t kNoAggregate = 255;
struct TwoLevelPlan {
    uint32_t n_agg = 0, n_rows = 0, n_blocks = 0;
    std::vector<uint32_t> row_view;                 // row -> view, 0xFFFFFFFF = padding
    std::vector<uint32_t> ptr, aedge, aother;       // the adjacency of the rows (incidences in the views' order)
    std::vector<int8_t> asign;
    std::vector<uint8_t> aagg, root, agg_of_block;  // aggregate of the incidence's other end / of the block; row is inert
    std::vector<uint32_t> agg_block;                // n_agg + 1 block starts
};
// Breadth-first order of all views from the gauge views; returns the depth of the deepest view.  A band-like graph (views along
// a walk or a ring) is deep -- V / reach levels -- a densely connected one has a handful of levels.
inline uint32_t bfs_from_gauge_views(uint32_t V, const IncidenceCsr& g, const std::vector<uint8_t>& is_root,
                                     std::vector<uint32_t>& order) {
    order.clear();
    order.reserve(V);
    std::vector<uint32_t> level(V, 0xFFFFFFFFu);
    for (uint32_t v = 0; v < V; ++v)
        if (is_root[v]) { level[v] = 0; order.push_back(v); }
    uint32_t depth = 0;
    for (size_t h = 0; h < order.size(); ++h) {
        const uint32_t u = order[h];
        for (uint32_t a = g.ptr[u]; a < g.ptr[u + 1]; ++a) {
            const uint32_t o = g.other[a];
            if (level[o] != 0xFFFFFFFFu) continue;
            level[o] = level[u] + 1;
            depth = std::max(depth, level[o]);
            order.push_back(o);
        }
    }
    for (uint32_t v = 0; v < V; ++v)
        if (level[v] == 0xFFFFFFFFu) order.push_back(v);  // (not reachable from a gauge view: cannot happen, kept for safety)
    return depth;
}
// Aggregates by region growing: seeds in breadth-first order from the gauge views (`order`), each aggregate the first `target`
// free views a breadth-first walk from its seed reaches among the unassigned ones; left-overs below half the target join
// their smallest neighbouring aggregate.  An aggregate is a run of whole blocks of rows_per_block rows.  false when the graph
// needs more than max_aggregates - 1 (many components).
inline bool plan_two_level(uint32_t V, const IncidenceCsr& g, const std::vector<uint8_t>& is_root, const std::vector<uint32_t>& order,
                           uint32_t rows_per_block, uint32_t max_aggregates, TwoLevelPlan& out) {
    const std::vector<uint32_t>&ptr = g.ptr, &aedge = g.edge, &aother = g.other;
    uint32_t n_free = 0;
    for (uint32_t v = 0; v < V; ++v) n_free += is_root[v] ? 0u : 1u;
    if (n_free == 0) return false;
    const uint32_t kNone = 0xFFFFFFFFu;
    uint32_t target = std::max<uint32_t>(32u, (n_free + 111u) / 112u);
    target = (target + rows_per_block - 1) / rows_per_block * rows_per_block;
    std::vector<uint32_t> agg, disc, size, into, final_id;  // disc: the free views in the order the walks reached them
    uint32_t n_final = 0;
    auto label = [&](uint32_t a) {  // the aggregate a merged one ended up in
        while (into[a] != a) a = into[a] = into[into[a]];
        return a;
    };
    for (int attempt = 0;; ++attempt) {
        agg.assign(V, kNone);
        disc.clear();
        disc.reserve(n_free);
        size.clear();
        for (uint32_t seed : order) {
            if (is_root[seed] || agg[seed] != kNone) continue;
            const uint32_t a0 = (uint32_t)size.size();
            const size_t first = disc.size();
            disc.push_back(seed);
            agg[seed] = a0;
            for (size_t h = first; h < disc.size() && disc.size() - first < target; ++h)
                for (uint32_t a = ptr[disc[h]]; a < ptr[disc[h] + 1] && disc.size() - first < target; ++a) {
                    const uint32_t o = aother[a];
                    if (is_root[o] || agg[o] != kNone) continue;
                    agg[o] = a0;
                    disc.push_back(o);
                }
            size.push_back((uint32_t)(disc.size() - first));
        }
        const uint32_t n0 = (uint32_t)size.size();
        into.resize(n0);
        std::iota(into.begin(), into.end(), 0u);
        // small left-overs join a neighbour (their views are contiguous in disc: walk them through a start table)
        std::vector<uint32_t> start(n0 + 1, 0);
        for (uint32_t a0 = 0; a0 < n0; ++a0) start[a0 + 1] = start[a0] + size[a0];
        for (uint32_t a0 = 0; a0 < n0; ++a0) {
            if (size[a0] >= target / 2) continue;  // (size of the aggregate as grown; one that already took others in is large enough)
            uint32_t best = kNone;
            for (uint32_t i = start[a0]; i < start[a0 + 1]; ++i)
                for (uint32_t a = ptr[disc[i]]; a < ptr[disc[i] + 1]; ++a) {
                    const uint32_t o = aother[a];
                    if (is_root[o]) continue;
                    const uint32_t h = label(agg[o]);
                    if (h == a0) continue;
                    if (best == kNone || size[h] < size[best] || (size[h] == size[best] && h < best)) best = h;
                }
            if (best == kNone) continue;  // a component of its own
            into[a0] = best;
            size[best] += size[a0];
        }
        final_id.assign(n0, kNone);
        n_final = 0;
        for (uint32_t a0 = 0; a0 < n0; ++a0)
            if (into[a0] == a0) final_id[a0] = n_final++;
        if (n_final <= max_aggregates - 1) break;  // (ids stay below kNoAggregate and below the lanes of the coarse product)
        if (attempt == 5 || target >= n_free) return false;
        target *= 2;
    }
    for (uint32_t v = 0; v < V; ++v)
        if (agg[v] != kNone) agg[v] = final_id[label(agg[v])];
    // the views of every aggregate in the order they were reached (a stable counting sort of disc by aggregate)
    std::vector<uint32_t> first_of(n_final + 1, 0);
    for (uint32_t v : disc) ++first_of[agg[v] + 1];
    for (uint32_t a0 = 0; a0 < n_final; ++a0) first_of[a0 + 1] += first_of[a0];
    std::vector<uint32_t> sorted(disc.size()), fill(first_of.begin(), first_of.end() - 1);
    for (uint32_t v : disc) sorted[fill[agg[v]]++] = v;
    // rows: the aggregates one after the other, each padded to whole blocks; the gauge views last
    std::vector<uint32_t> view_row(V, kNone);
    out = TwoLevelPlan();
    out.n_agg = n_final;
    out.agg_block.push_back(0);
    for (uint32_t a0 = 0; a0 < n_final; ++a0) {
        for (uint32_t i = first_of[a0]; i < first_of[a0 + 1]; ++i) {
            view_row[sorted[i]] = (uint32_t)out.row_view.size();
            out.row_view.push_back(sorted[i]);
        }
        while (out.row_view.size() % rows_per_block) out.row_view.push_back(kNone);
        out.agg_block.push_back((uint32_t)(out.row_view.size() / rows_per_block));
    }
    out.agg_of_block.assign(out.row_view.size() / rows_per_block, kNoAggregate);
    for (uint32_t a0 = 0; a0 < out.n_agg; ++a0)
        for (uint32_t b = out.agg_block[a0]; b < out.agg_block[a0 + 1]; ++b) out.agg_of_block[b] = (uint8_t)a0;
    for (uint32_t v = 0; v < V; ++v)
        if (is_root[v]) {
            view_row[v] = (uint32_t)out.row_view.size();
            out.row_view.push_back(v);
        }
    while (out.row_view.size() % rows_per_block) out.row_view.push_back(kNone);
    out.n_rows = (uint32_t)out.row_view.size();
    out.n_blocks = out.n_rows / rows_per_block;
    out.agg_of_block.resize(out.n_blocks, kNoAggregate);
    out.root.assign(out.n_rows, 1);
    out.ptr.assign(out.n_rows + 1, 0);
    out.aedge.reserve(aedge.size()); out.aother.reserve(aedge.size()); out.asign.reserve(aedge.size()); out.aagg.reserve(aedge.size());
    for (uint32_t k = 0; k < out.n_rows; ++k) {
        const uint32_t v = out.row_view[k];
        if (v != kNone) {
            out.root[k] = is_root[v];
            for (uint32_t a = ptr[v]; a < ptr[v + 1]; ++a) {
                const uint32_t o = aother[a];
                out.aedge.push_back(aedge[a]);
                out.aother.push_back(view_row[o]);
                out.asign.push_back(g.sign[a]);
                out.aagg.push_back(is_root[o] ? kNoAggregate : (uint8_t)agg[o]);
            }
        }
        out.ptr[k + 1] = (uint32_t)out.aedge.size();
    }
    return true;
}
}  // namespace pgi
