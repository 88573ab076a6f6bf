// fasthist_bucket.hpp -- the bucket rule of the range histogram, shared by the bin kernel of fasthist.hip and by a g++ build
// of the same text (tests/test_fasthist_cpu.py).  No dependencies: plain fp64 compares and multiplications; the one division is w = M / b.
//
// With M the largest finite range of the cloud, w = fl(M / b) and edge e_i = fl(i w), a point at range d falls into
//   0 < d < M : the largest i < b with e_i <= d (a point exactly on an interior edge goes to the upper bucket);
//   otherwise : b - 1 (d == 0, d == M, d not finite).
// A point with 0 < d < M and d > e_b (possible only when fl(b w) < M, for d in that last gap) is in bucket b - 1 and reported as unbound.
#pragma once

#ifdef __HIPCC__
#define MRS_FH_HD __host__ __device__
#else
#define MRS_FH_HD
#endif

namespace mrs {

MRS_FH_HD inline double fh_width(double M, int b) { return M / (double)b; }

// bucket of range d; *unbound is set to 1 for the one-ulp gap above e_b and to 0 otherwise.  inv_w = 1 / w (computed once per cloud) only
// feeds the guess: any value, even inf or NaN, gives the same bucket
MRS_FH_HD inline int fh_bucket(double d, double M, double w, double inv_w, int b, int* unbound)
{
    *unbound = 0;
    if (!(d > 0.0 && d < M)) return b - 1;
    // the quotient is a guess (a product with a rounded reciprocal, against edges that are rounded products themselves): off by one at most
    // next to an edge, and meaningless when w underflows; the two walks below settle it against the edges themselves, in at most b steps
    const double q = d * inv_w;
    int g = q < (double)(b - 1) ? (q > 0.0 ? (int)q : 0) : b - 1;      // NaN takes the last branch
    while (g > 0 && (double)g * w > d) --g;
    while (g < b - 1 && (double)(g + 1) * w <= d) ++g;
    if (g == b - 1 && d > (double)b * w) *unbound = 1;
    return g;
}

}  // namespace mrs
