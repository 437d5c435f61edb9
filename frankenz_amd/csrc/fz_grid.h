// Launch arithmetic that needs no HIP call, as pure functions (fz_launch.h asks the runtime for the numbers and launches); includes
// nothing from HIP: tests/host/grid_check.cpp compiles it with the system compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

// LDS of one compute unit of gfx950: the most a block can be given (static + dynamic)
constexpr size_t FZ_LDS_BYTES = 160 * 1024;

// Grid of a kernel whose blocks stay resident and keep candidate lists in the workspace: `need` blocks cover the launch, `bpc` stay
// resident per CU, the lists of `fit` blocks fit the budget.  Whole multiples of the CU count (an uneven tail of blocks would idle
// most CUs), else -- very large model sets -- whatever fits while that is half the chip (still beats two passes).  0, or +1: none
inline int fz_grid_resident(int64_t need, int bpc, int64_t fit, int cus, int64_t& blocks) {
    blocks = need;
    if (need <= cus) return fit < need ? 1 : 0;
    const int64_t k = std::min<int64_t>(bpc, fit / cus);
    if (k >= 1) blocks = std::min<int64_t>(need, k * cus);
    else if (fit >= cus / 2) blocks = fit;
    else return 1;                                                 // cannot fill even half the chip
    return 0;
}

// Entries per wave of k_hist's ambiguous lists: a thin band of the candidates when the best model fits well (~1 % of M on the
// benchmark).  M up to 131 072 models (can never overflow), M / 8 beyond (an object that overflows is re-run by the exact sweep): a
// 1e6-model set then keeps the whole chip busy inside the budget.  forced: FZ_HIST_AMBCAP = value (tests: the overflow hand-back)
inline int64_t fz_amb_cap(int64_t M, bool forced, int64_t value) {
    if (forced) return std::max<int64_t>(1, value);
    return (M <= 131072) ? M : std::max<int64_t>(131072, M / 8);
}

// k_kde: objects per wave / waves per block from the LDS each object's accumulator (acc_stride doubles) needs
struct fz_kde_geom { int tw, wpb; };
inline fz_kde_geom fz_kde_geometry(int acc_stride) {
    const size_t per_obj = (size_t)acc_stride * 8;
    if (per_obj * 8 <= 53 * 1024) return {2, 4};
    if (per_obj * 4 <= FZ_LDS_BYTES) return {1, 4};
    if (per_obj * 2 <= FZ_LDS_BYTES) return {1, 2};
    return {1, 1};
}

// k_plane_rows: (waves per block, register pairs per lane) for rows of M entries on a grid of G points with kernels of w2 + 1 taps,
// or {0, 0}: not applicable.  Shapes: 5 120 entries (8 waves x 5 register pairs), 10 240 (8 x 10), 20 480 (16 x 10); a row must
// fill 80 % of its shape (a 15 000-entry row on the 20 480 shape is slower than k_plane_fused: 2.56 vs 2.40 ms per 66 000 rows)
struct fz_rows_shape { int nw, e2; };
inline fz_rows_shape fz_plane_rows_shape(int64_t M, int64_t G, int64_t w2, int64_t acc_stride) {
    if (w2 >= 128 || G + w2 > 65535 || G + w2 > acc_stride || G > 8 * 128) return {0, 0};
    const fz_rows_shape s = (M <= 5120) ? fz_rows_shape{8, 5} : (M <= 10240) ? fz_rows_shape{8, 10} : fz_rows_shape{16, 10};
    const int64_t capn = (int64_t)s.nw * 64 * 2 * s.e2;
    if (M > capn || M * 5 < capn * 4) return {0, 0};
    return s;
}
