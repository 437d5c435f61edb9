// numpy.interp (compiled_base.c arr_interp) for one point: the interpolation rule of every kernel that resamples a row
// (k_summarize, k_resample, k_recentre, k_cdf_draws, k_synphot).  No HIP include: the same text compiles for the host, where
// tests/host/interp_check.cpp runs it under the address sanitizer over arrays of exactly n doubles.
//
// xp non-decreasing (plateaus allowed); j = last index with xp[j] <= x.  One node: fp(0) whatever x is, NaN included (numpy's
// one-node rule).  NaN nodes:
//   * a NaN after finite nodes orders as +inf (every comparison against it is false), as in numpy's search from a fresh guess: a
//     finite prefix followed by NaNs -- the cumsum of a row with a NaN in it -- gives numpy's result;
//   * xp(0) NaN: a point at or above a later finite node is interpolated there as numpy does; a point with no node at or below it
//     (all nodes NaN, or x below the first finite one) gives that NaN, where numpy's own answer depends on the length of xp and
//     on where its guess-based search starts.  Nothing outside [0, n) is ever evaluated.
#pragma once

#ifdef __HIPCC__
#define FZ_INTERP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define FZ_INTERP_FN inline
#endif

namespace fz {

template <class XP, class FP>
FZ_INTERP_FN double interp1(double x, const XP& xp, const FP& fp, int n) {
    if (n == 1) return fp(0);
    if (x != x) return x;
    if (x < xp(0)) return fp(0);
    if (x > xp(n - 1)) return fp(n - 1);
    int lo = 0, hi = n;                                  // first index with xp > x
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (x >= xp(mid)) lo = mid + 1; else hi = mid; }
    if (lo == 0) return xp(0);                           // xp(0) is NaN and no node is at or below x: j would be -1
    const int j = lo - 1;
    if (j >= n - 1) return fp(n - 1);
    const double xj = xp(j), fj = fp(j);
    if (xj == x) return fj;
    const double fj1 = fp(j + 1), xj1 = xp(j + 1);
    const double slope = (fj1 - fj) / (xj1 - xj);
    double r = slope * (x - xj) + fj;
    if (r != r) {
        r = slope * (x - xj1) + fj1;
        if (r != r && fj == fj1) r = fj;
    }
    return r;
}

}  // namespace fz
