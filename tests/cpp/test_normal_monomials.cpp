// Host driver of csrc/pgi_normal_monomials.hpp (no GPU, no HIP): the n-point refit builds its 9x9 normal matrix from 36
// distinct monomials instead of the 45 products of the upper triangle.  Checked here, bit for bit:
//   1. the nine pairs of upper-triangle entries that share a monomial give the same f64 product, before and after the
//      QMAGIC rounding, on 10^5 random rows plus rows with zeros, equal coordinates and values near 2^-20;
//   2. the 36-accumulator build of A^T A (normal_accumulate + normal_scatter, the kernels' own code) equals the plain
//      45-product build over 1000 rows, in three row orders;
//   3. the table from monomial to entries covers each of the 81 entries exactly once.
// Prints one line per check and "all ok"; any "MISMATCH" line makes the exit status 1.
#include "pgi_normal_monomials.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace pgi;

static int failures = 0;
static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}
static double quantise(double t) {
    volatile double q = t + QMAGIC;  // (volatile: the two roundings stay two operations whatever the optimiser thinks)
    return q - QMAGIC;
}

struct Row {
    float x1, y1, x2, y2;
};

static std::vector<Row> make_rows(size_t n_random, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-2.0f, 2.0f);
    std::vector<Row> rows;
    for (size_t i = 0; i < n_random; ++i) rows.push_back(Row{U(rng), U(rng), U(rng), U(rng)});
    const float tiny = 9.5367431640625e-07f;  // 2^-20
    const float sp[] = {0.0f, -0.0f, 1.0f, -1.0f, 2.0f, -2.0f, tiny, -tiny, tiny * 1.0000001f, tiny * 0.75f, 0.33333334f, 1.9999999f};
    const int ns = (int)(sizeof(sp) / sizeof(sp[0]));
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b < ns; ++b) {
            rows.push_back(Row{sp[a], sp[b], sp[b], sp[a]});
            rows.push_back(Row{sp[a], sp[a], sp[b], sp[b]});  // equal coordinates inside an image
            rows.push_back(Row{sp[a], sp[b], sp[a], sp[b]});  // equal coordinates across the images
            rows.push_back(Row{sp[a], U(rng), sp[b], U(rng)});
            rows.push_back(Row{U(rng), sp[a], U(rng), sp[b]});
        }
    for (int k = 0; k < 64; ++k) {  // all four near 2^-20, and one random value repeated four times
        const float s = tiny * (1.0f + 0.01f * (float)k);
        rows.push_back(Row{s, -s, s * 1.5f, s * 0.5f});
        const float v = U(rng);
        rows.push_back(Row{v, v, v, v});
    }
    return rows;
}

// the nine duplicates of the upper triangle: entry (i, j) repeats the monomial of entry (k, l)
static const int kDup[9][4] = {{0, 4, 1, 3}, {0, 5, 2, 3}, {1, 5, 2, 4}, {0, 7, 1, 6}, {0, 8, 2, 6},
                               {1, 8, 2, 7}, {3, 7, 4, 6}, {3, 8, 5, 6}, {4, 8, 5, 7}};

static void check_duplicate_products() {
    const std::vector<Row> rows = make_rows(100000, 1u);
    size_t bad_raw = 0, bad_q = 0, nonzero = 0;
    for (const Row& r : rows) {
        double a[9];
        normal_design_row(r.x1, r.y1, r.x2, r.y2, a);
        for (int d = 0; d < 9; ++d) {
            const double t0 = a[kDup[d][0]] * a[kDup[d][1]], t1 = a[kDup[d][2]] * a[kDup[d][3]];
            bad_raw += bits(t0) != bits(t1);
            bad_q += bits(quantise(t0)) != bits(quantise(t1));
            nonzero += t0 != 0.0;
        }
    }
    std::printf("products rows %zu pairs 9 nonzero %zu raw_mismatches %zu quantised_mismatches %zu\n", rows.size(), nonzero, bad_raw, bad_q);
    if (bad_raw || bad_q || rows.size() < 100000 || nonzero < 9 * 90000) {
        std::printf("MISMATCH products\n");
        ++failures;
    }
}

static void build45(const std::vector<Row>& rows, const std::vector<int>& order, double A[81]) {
    double S[9][9] = {};
    for (int idx : order) {
        double a[9];
        normal_design_row(rows[idx].x1, rows[idx].y1, rows[idx].x2, rows[idx].y2, a);
        for (int i = 0; i < 9; ++i)
            for (int j = i; j < 9; ++j) S[i][j] = S[i][j] + quantise(a[i] * a[j]);
    }
    for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j) A[9 * i + j] = A[9 * j + i] = S[i][j];
}

static void build36(const std::vector<Row>& rows, const std::vector<int>& order, double A[81]) {
    double S[2][kNormalPass] = {};
    for (int idx : order) {  // (one row loop here; the kernels sweep the rows once per set of 18 -- the sums are the same)
        double a[9];
        normal_design_row(rows[idx].x1, rows[idx].y1, rows[idx].x2, rows[idx].y2, a);
        normal_accumulate<0>(a, S[0]);
        normal_accumulate<1>(a, S[1]);
    }
    for (int i = 0; i < 81; ++i) A[i] = -7.0;  // every entry must be overwritten
    for (int k = 0; k < kNormalMonomials; ++k) normal_scatter(k, S[k / kNormalPass][k % kNormalPass], A);
}

static void check_matrix() {
    std::vector<Row> rows = make_rows(400, 2u);  // 400 random rows + the special ones, cut to 1000
    std::mt19937 rng(3u);
    std::shuffle(rows.begin(), rows.end(), rng);
    rows.resize(1000);
    std::vector<int> fwd(1000), rev(1000), shuf(1000);
    for (int i = 0; i < 1000; ++i) fwd[i] = i, rev[i] = 999 - i, shuf[i] = i;
    std::shuffle(shuf.begin(), shuf.end(), rng);
    const std::vector<int>* orders[3] = {&fwd, &rev, &shuf};
    const char* names[3] = {"forward", "reverse", "shuffled"};
    double ref[81];
    build45(rows, fwd, ref);
    for (int o = 0; o < 3; ++o) {
        double A45[81], A36[81];
        build45(rows, *orders[o], A45);
        build36(rows, *orders[o], A36);
        int bad = 0;
        for (int i = 0; i < 81; ++i) bad += bits(A45[i]) != bits(A36[i]) || bits(A36[i]) != bits(ref[i]);
        std::printf("matrix order %s rows %zu mismatches %d trace %.17g\n", names[o], rows.size(), bad, A36[0] + A36[40] + A36[80]);
        if (bad) {
            std::printf("MISMATCH matrix %s\n", names[o]);
            ++failures;
        }
    }
}

// exponents of (x1, y1, x2, y2) in a[i]
static void exponents(int i, int e[4]) {
    const int p = i / 3, q = i % 3;
    e[0] = q == 0; e[1] = q == 1; e[2] = p == 0; e[3] = p == 1;
}

static void check_table() {
    int cover[81] = {};
    int bad = 0;
    std::vector<std::vector<int>> seen;
    for (int k = 0; k < kNormalMonomials; ++k) {
        const NormalMonomial m = normal_monomial(k), t = kNormalTab.m[k];
        bad += m.i != t.i || m.j != t.j || m.i2 != t.i2 || m.j2 != t.j2;
        bad += !(0 <= m.i && m.i <= m.j && m.j < 9 && 0 <= m.i2 && m.i2 <= m.j2 && m.j2 < 9);
        bad += (k < kNormalPass) != (m.i < 3);  // sweep 0 multiplies a[0..2] from the left, sweep 1 a[3..8]
        int e0[4], e1[4], f0[4], f1[4];
        exponents(m.i, e0); exponents(m.j, e1); exponents(m.i2, f0); exponents(m.j2, f1);
        std::vector<int> mono(4);
        for (int c = 0; c < 4; ++c) {
            mono[c] = e0[c] + e1[c];
            bad += mono[c] != f0[c] + f1[c];  // both entries carry the same monomial
        }
        bad += std::find(seen.begin(), seen.end(), mono) != seen.end();  // and no two table rows the same one
        seen.push_back(mono);
        // the symmetric pair {(i, j), (j, i)} counts once, and so does the twin pair when there is one
        cover[9 * m.i + m.j] += 1;
        if (m.j != m.i) cover[9 * m.j + m.i] += 1;
        if (m.i2 != m.i || m.j2 != m.j) {
            cover[9 * m.i2 + m.j2] += 1;
            if (m.j2 != m.i2) cover[9 * m.j2 + m.i2] += 1;
        }
    }
    int covered = 0;
    for (int i = 0; i < 81; ++i) {
        covered += cover[i] == 1;
        bad += cover[i] != 1;
    }
    int twins = 0;
    for (int d = 0; d < 9; ++d)  // the nine duplicates are exactly the table's twins
        for (int k = 0; k < kNormalMonomials; ++k) {
            const NormalMonomial m = kNormalTab.m[k];
            twins += m.i == kDup[d][0] && m.j == kDup[d][1] && m.i2 == kDup[d][2] && m.j2 == kDup[d][3];
        }
    bad += twins != 9;
    std::printf("table monomials %d entries_covered_once %d twins %d errors %d\n", kNormalMonomials, covered, twins, bad);
    if (bad) {
        std::printf("MISMATCH table\n");
        ++failures;
    }
}

int main() {
    check_duplicate_products();
    check_matrix();
    check_table();
    if (failures) return 1;
    std::printf("all ok\n");
    return 0;
}
