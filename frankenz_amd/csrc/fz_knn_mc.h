// Monte-Carlo draws of the k-NN fitter on the device (docs/knn.md, "Monte-Carlo draws on the device"): the query features of
// knn.py:830-832 and the K feature sets of knn.py:158-188, as normal variates of Philox4x32-10 (fz_philox.h: philox_normal2).
//
//   k_knn_mc_features<MAP>   q[i][b] = map_b(fma(xe[i][b], z, x[i][b]))  in fp64; z of (key, row first + i, band b, set 0)
//   k_knn_mc_sets<MAP>       out[t][j][b] = float32(map_b(double(float32(fma(ye[j][b], z, y[j][b])))));  z of (key, row j, band b, set 1 + t)
//                            -- the reference's two float32 roundings (knn.py:177, 181) with the map in fp64 between them
//
// One thread per (row, band pair): the pair's two variates come from one Philox call.  Rows are read as given (before the library's
// in-place clean; the reference draws first and cleans inside logprob).  xe == 0 gives x itself (fma(0, z, x)); non-finite values follow
// IEEE arithmetic; a negative draw under `magnitude` is nan.  A negative or nan error sets FZ_KNN_MC_ERR_SCALE in flags[0] and the
// smallest such row in the 64-bit word at flags + 2 (NumPy's normal raises "scale < 0"): the host fails the call.
#pragma once
#include "fz_philox.h"

#define FZ_KNN_MAP_IDENTITY 0
#define FZ_KNN_MAP_MAGNITUDE 1
#define FZ_KNN_MAP_LUPTITUDE 2
#define FZ_KNN_MC_FMAX 32                  // bands, as everywhere
#define FZ_KNN_MC_ERR_SCALE 1              // a negative or nan error (the row: the 64-bit word at flags + 2, smallest first)
#define FZ_KNN_MC_NT 256

namespace fz {

// the map's constants per band, formed on the host (fz_knn_mc_host.inc): magnitude a = zeropoint; luptitude a = 2 skynoise,
// b = ln(skynoise / zeropoint)
struct KnnMcMap { double a[FZ_KNN_MC_FMAX], b[FZ_KNN_MC_FMAX]; };

// pdf.py:625-657 / 695-734 (this package's pdf.magnitude / pdf.luptitude), value half, in fp64
template <int MAP> __device__ __forceinline__ double knn_mc_map(double d, double a, double b) {
    if (MAP == FZ_KNN_MAP_MAGNITUDE) return -2.5 * log10(d / a);
    if (MAP == FZ_KNN_MAP_LUPTITUDE) return (-2.5 / 2.302585092994046) * (asinh(d / a) + b);
    return d;
}

__device__ __forceinline__ void knn_mc_flag(double e, int64_t row, int* __restrict__ flags) {
    if (!(e >= 0.0)) {
        atomicOr(flags, FZ_KNN_MC_ERR_SCALE);
        atomicMin((unsigned long long*)(flags + 2), (unsigned long long)row);
    }
}

// x, xe, q (n, F) row-major; the rows are objects first .. first + n - 1 of the caller's set
template <int MAP>
static __global__ __launch_bounds__(FZ_KNN_MC_NT) void k_knn_mc_features(const double* __restrict__ x, const double* __restrict__ xe, int64_t n, int F,
                                                                         KnnMcMap mp, uint32_t k0, uint32_t k1, int64_t first,
                                                                         double* __restrict__ q, int* __restrict__ flags) {
    const int np = (F + 1) >> 1;
    const int64_t t = (int64_t)blockIdx.x * FZ_KNN_MC_NT + threadIdx.x;
    if (t >= n * np) return;
    const int64_t i = t / np;
    const int b0 = 2 * (int)(t - i * np);
    const bool two = b0 + 1 < F;
    const int64_t at = i * F + b0;
    const double x0 = x[at], e0 = xe[at], x1 = two ? x[at + 1] : 0.0, e1 = two ? xe[at + 1] : 0.0;
    double z0, z1;
    philox_normal2(k0, k1, (uint64_t)(first + i), (uint32_t)(b0 >> 1), 0u, z0, z1);
    knn_mc_flag(e0, i, flags);
    q[at] = knn_mc_map<MAP>(fma(e0, z0, x0), mp.a[b0], mp.b[b0]);
    if (two) {
        knn_mc_flag(e1, i, flags);
        q[at + 1] = knn_mc_map<MAP>(fma(e1, z1, x1), mp.a[b0 + 1], mp.b[b0 + 1]);
    }
}

// y, ye (M, F) fp64 row-major; out (K, M, F) float32: the block fz_knn_upload_trees takes
template <int MAP>
static __global__ __launch_bounds__(FZ_KNN_MC_NT) void k_knn_mc_sets(const double* __restrict__ y, const double* __restrict__ ye, int64_t M, int F,
                                                                     KnnMcMap mp, uint32_t k0, uint32_t k1, float* __restrict__ out,
                                                                     int* __restrict__ flags) {
    const int np = (F + 1) >> 1;
    const int64_t t = (int64_t)blockIdx.x * FZ_KNN_MC_NT + threadIdx.x;
    const uint32_t set = blockIdx.y;
    if (t >= M * np) return;
    const int64_t j = t / np;
    const int b0 = 2 * (int)(t - j * np);
    const bool two = b0 + 1 < F;
    const int64_t at = j * F + b0;
    const double y0 = y[at], e0 = ye[at], y1 = two ? y[at + 1] : 0.0, e1 = two ? ye[at + 1] : 0.0;
    double z0, z1;
    philox_normal2(k0, k1, (uint64_t)j, (uint32_t)(b0 >> 1), 1u + set, z0, z1);
    float* o = out + (size_t)set * M * F + at;
    knn_mc_flag(e0, j, flags);
    o[0] = (float)knn_mc_map<MAP>((double)(float)fma(e0, z0, y0), mp.a[b0], mp.b[b0]);
    if (two) {
        knn_mc_flag(e1, j, flags);
        o[1] = (float)knn_mc_map<MAP>((double)(float)fma(e1, z1, y1), mp.a[b0 + 1], mp.b[b0 + 1]);
    }
}

}  // namespace fz
