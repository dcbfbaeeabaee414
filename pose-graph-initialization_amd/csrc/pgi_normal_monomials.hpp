// pgi_normal_monomials.hpp -- the 36 distinct monomials of the n-point refit's 9x9 normal matrix.
//
// The design row of a correspondence is the Kronecker product a = (x2, y2, 1) (x) (x1, y1, 1) of f32 values held in f64:
// a[3p + q] = u[p] * v[q] with u = (x2, y2, 1), v = (x1, y1, 1).  Every a[i] is an EXACT f64 (two 24-bit significands
// multiplied), so a[i] * a[j] is ONE rounding of the exact product u[p] u[r] v[q] v[s] of four floats: its bits depend on
// the monomial alone, not on how the four factors were paired.  Entries (3p+q, 3r+s) and (3p+s, 3r+q) carry the same
// monomial, hence the same bits before and after the QMAGIC rounding, and -- the sums being exact -- the same sum.  The
// 45 entries of the upper triangle are therefore 6 x 6 = 36 distinct sums: (p <= r) x (q <= s).
// Plain C++ (no HIP): the kernels include it through pgi_device.hpp, tests/cpp/test_normal_monomials.cpp directly.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PGI_HD __host__ __device__ __forceinline__
#define PGI_UNROLL _Pragma("unroll")
#else
#define PGI_HD inline
#define PGI_UNROLL
#endif

namespace pgi {

constexpr double QMAGIC = 393216.0;  // 1.5 * 2^18: summands rounded to multiples of 2^-34

constexpr int kNormalMonomials = 36;
constexpr int kNormalPass = 18;  // accumulators per sweep over the rows (two sweeps)

// the six index pairs lo <= hi of {0, 1, 2}: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), two bits per pair -- immediates, so that
// a lane can look its monomial up with two shifts instead of a load or an unranking loop
constexpr uint32_t kSymLo = 0u | (0u << 2) | (0u << 4) | (1u << 6) | (1u << 8) | (2u << 10);
constexpr uint32_t kSymHi = 0u | (1u << 2) | (2u << 4) | (1u << 6) | (2u << 8) | (2u << 10);

// Monomial k = 6 P + Q: pair P picks (p, r) among u, pair Q picks (q, s) among v.  (i, j) is the entry whose product is
// formed; (i2, j2) the other upper-triangle entry that carries the monomial, equal to (i, j) when there is none.
struct NormalMonomial {
    int i, j, i2, j2;
};
PGI_HD constexpr NormalMonomial normal_monomial(int k) {
    const int P = k / 6, Q = k - 6 * P;
    const int p = (int)((kSymLo >> (2 * P)) & 3u), r = (int)((kSymHi >> (2 * P)) & 3u);
    const int q = (int)((kSymLo >> (2 * Q)) & 3u), s = (int)((kSymHi >> (2 * Q)) & 3u);
    const bool twin = p != r && q != s;  // (p == r or q == s: the "other" entry is (i, j) itself or its transpose)
    return NormalMonomial{3 * p + q, 3 * r + s, twin ? 3 * p + s : 3 * p + q, twin ? 3 * r + q : 3 * r + s};
}
struct NormalMonomialTab {
    NormalMonomial m[kNormalMonomials];
};
constexpr NormalMonomialTab make_normal_monomials() {
    NormalMonomialTab t{};
    for (int k = 0; k < kNormalMonomials; ++k) t.m[k] = normal_monomial(k);
    return t;
}
constexpr NormalMonomialTab kNormalTab = make_normal_monomials();

PGI_HD void normal_design_row(float fx1, float fy1, float fx2, float fy2, double a[9]) {
    const double x1 = fx1, y1 = fy1, x2 = fx2, y2 = fy2;
    a[0] = x2 * x1; a[1] = x2 * y1; a[2] = x2;
    a[3] = y2 * x1; a[4] = y2 * y1; a[5] = y2;
    a[6] = x1;      a[7] = y1;      a[8] = 1.0;
}

// One row into the 18 accumulators of sweep PASS (monomials 18 PASS .. 18 PASS + 17; sweep 0 needs a[0..2] as the left
// factor, sweep 1 a[3..8]).  Every index is a compile-time constant once the loop is unrolled.
template <int PASS>
PGI_HD void normal_accumulate(const double a[9], double S[kNormalPass]) {
    PGI_UNROLL
    for (int k = 0; k < kNormalPass; ++k) {
        constexpr NormalMonomialTab T = make_normal_monomials();
        double t = a[T.m[kNormalPass * PASS + k].i] * a[T.m[kNormalPass * PASS + k].j];
        t = (t + QMAGIC) - QMAGIC;
        S[k] = S[k] + t;
    }
}

// The sum of monomial k goes to every entry of the symmetric 9x9 matrix A that carries it: (i, j), (i2, j2) and their
// transposes -- up to four entries, each of the 81 written by exactly one monomial.
PGI_HD void normal_scatter(int k, double v, double* A) {
    const NormalMonomial m = normal_monomial(k);
    A[9 * m.i + m.j] = v;
    A[9 * m.j + m.i] = v;
    A[9 * m.i2 + m.j2] = v;
    A[9 * m.j2 + m.i2] = v;
}

}  // namespace pgi
