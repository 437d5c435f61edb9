// Validation of a PDF stack against known values: the arithmetic of the reference's plotting.py (docs/diagnostics.md).
//
//   k_stack_rows  per object: the per-PDF cut (plotting.py:138, 143) and the normalisation of its outer product (plotting.py:155-156)
//   k_stack2d     stack = K^T P summed over objects (plotting.py:129-159): fp64 MFMA, the geometry of k_gemm_f64
//   k_stack_add   the partial tiles of k_stack2d added in split order
//   k_recentre    np.interp(dgrid, disp(pgrid, cent_i), pdf_i) per object (plotting.py:319-320)
//   k_cdf_draws   per object: CDF, np.interp of the Monte-Carlo truths into it, weighted histogram (plotting.py:427-436, 501-505)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fz_summary.h"

namespace fz {

// One selected object of a stack, in the order of its centre.  The host fills row / koff / start / len and puts the object's
// effective weight into `scale`; k_stack_rows replaces `cut` and `scale` by what k_stack2d applies.
struct StackObj {
    double cut, scale;         // P operand: p > cut ? p * scale : 0
    int64_t row;               // row of the PDF array (of the chunk on the device)
    int64_t koff;              // first tap of the object's dictionary kernel in the concatenated table
    int32_t start, len;        // grid index of tap 0 (centre - half-width, may be negative), number of taps
};
// One block of k_stack2d: x tile `tx`, sorted objects [k0, k1)
struct StackItem { int32_t tx, k0, k1, pad_; };

// ---- the per-PDF cut and the scale of an object's outer product: one wave per object ---------------------------------------------
// mode 0: keep = p > max(p) * thresh, q = p / sum(p[keep]); the object's cells are  kern[a] q[j] w / (S_kernel sum(q[keep])).
// mode 1: the row is already cut and divided (the host's per-row CDF rule): every entry is kept, nothing is divided again.
// S_kernel: the taps that fall on the grid [0, Gx), each lane a contiguous run in tap order (not a difference of the dictionary's
// cumulative table: for a window hanging off the low edge by nearly its half-width that difference cancels).
// bad: the smallest object position whose row holds a value that is not finite (INT_MAX: none).
static __global__ __launch_bounds__(256) void k_stack_rows(const double* __restrict__ pdfs, int Gy, int Gx,
                                                           const double* __restrict__ kern, StackObj* __restrict__ objs, int n,
                                                           double thresh, int mode, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const StackObj o = objs[k];
    const double* p = pdfs + o.row * Gy;
    double m = -INFINITY; int nf = 0;
    for (int j = lane; j < Gy; j += 64) { const double v = p[j]; if (!(v - v == 0.0)) nf = 1; m = fmax(m, v); }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = fmax(m, __shfl_xor(m, s, 64));
    if (__ballot(nf)) { if (lane == 0) atomicMin(bad, k); return; }
    const double cut = mode == 0 ? m * thresh : -INFINITY;          // (0 * -inf = nan: nothing passes, as in the reference)
    double S = 0.0;
    for (int j = lane; j < Gy; j += 64) { const double v = p[j]; if (v > cut) S += v; }
    S = wsum(S);
    double S2 = 0.0;
    if (mode == 0) {
        for (int j = lane; j < Gy; j += 64) { const double v = p[j]; if (v > cut) S2 += v / S; }
        S2 = wsum(S2);
    } else { S2 = S; S = 1.0; }
    const int t0 = max(0, -o.start), t1 = min(o.len, Gx - o.start);
    const int per = (max(t1 - t0, 0) + 63) / 64;
    double Sk = 0.0;
    for (int t = t0 + lane * per, e = min(t1, t + per); t < e; ++t) Sk += kern[o.koff + t];
    Sk = wsum(Sk);
    const double d = Sk * S2;
    double scale = (o.scale / d) / S;
    if (!(d != 0.0) || !(S != 0.0) || !(scale - scale == 0.0)) scale = 0.0;      // a row without mass adds nothing
    if (lane == 0) { objs[k].cut = cut; objs[k].scale = scale; }
}

// ---- stack tile partials: part[item][ty] (128 x 128) = sum over the item's objects of K[k][x] P[k][y] ---------------------------
// The tile geometry, LDS layout and MFMA loop of k_gemm_f64 (fz_summary.h); both operands are k-major already (a row is an object),
// so both LDS stores are the straight ones.  K is generated from the dictionary table, P is the cut and scaled PDF row.
static __global__ __launch_bounds__(256) void k_stack2d(const double* __restrict__ pdfs, int Gy, int Gx, const double* __restrict__ kern,
                                                        const StackObj* __restrict__ objs, const StackItem* __restrict__ items,
                                                        double* __restrict__ part) {
    extern __shared__ double smem[];                   // As[2][BK][LD] | Bs[2][BK][LD]
    double* As = smem;
    double* Bs = smem + 2 * FZ_GEMM_BK * FZ_GEMM_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int it_k0 = items[blockIdx.x].k0, it_k1 = items[blockIdx.x].k1;
    const int x0 = items[blockIdx.x].tx * FZ_GEMM_BM, n0 = blockIdx.y * FZ_GEMM_BN;
    const int ok = tid >> 4, seg = (tid & 15) * 8;     // object of the k-step, 8 consecutive x / y
    double ra[8], rb[8];
    auto gload = [&](int kb) {
        const int k = kb + ok;
        if (k < it_k1) {
            const double cut = objs[k].cut, scale = objs[k].scale;
            const int start = objs[k].start, len = objs[k].len;
            const double* p = pdfs + objs[k].row * Gy;
            const double* kn = kern + objs[k].koff;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int col = n0 + seg + q;
                const double v = col < Gy ? p[col] : 0.0;
                rb[q] = (col < Gy && v > cut) ? v * scale : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int x = x0 + seg + q, t = x - start;
                ra[q] = (x < Gx && t >= 0 && t < len) ? kn[t] : 0.0;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) { ra[q] = 0.0; rb[q] = 0.0; }
        }
    };
    auto sstore = [&](int buf) {
        double* a = As + buf * FZ_GEMM_BK * FZ_GEMM_LD + ok * FZ_GEMM_LD + seg;
        double* b = Bs + buf * FZ_GEMM_BK * FZ_GEMM_LD + ok * FZ_GEMM_LD + seg;
#pragma unroll
        for (int q = 0; q < 8; ++q) { a[q] = ra[q]; b[q] = rb[q]; }
    };
    v4f64 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = v4f64{0.0, 0.0, 0.0, 0.0};
    const int nk = (it_k1 - it_k0 + FZ_GEMM_BK - 1) / FZ_GEMM_BK;
    gload(it_k0);
    sstore(0);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) gload(it_k0 + (t + 1) * FZ_GEMM_BK);
        const double* a = As + buf * FZ_GEMM_BK * FZ_GEMM_LD + wr * 64 + (lane & 15);
        const double* b = Bs + buf * FZ_GEMM_BK * FZ_GEMM_LD + wc * 64 + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < FZ_GEMM_BK; kk += 4) {
            const int krow = (kk + (lane >> 4)) * FZ_GEMM_LD;
            double av[4], bv[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) av[mi] = a[krow + mi * 16];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) bv[ni] = b[krow + ni * 16];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
        }
        if (t + 1 < nk) sstore(buf ^ 1);
        __syncthreads();
    }
    // D layout (f64 16x16x4): col = lane & 15, row = (lane >> 4) + 4 * reg; the whole padded tile is written
    double* out = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (FZ_GEMM_BM * FZ_GEMM_BN);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = wc * 64 + ni * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + mi * 16 + (lane >> 4) + 4 * r;
                out[row * FZ_GEMM_BN + col] = acc[mi][ni][r];
            }
        }
}

// stack[x][y] (+)= the partial tiles of x tile x / 128 in split order; tiles: per x tile (first item, items); no items: zeros
static __global__ __launch_bounds__(256) void k_stack_add(const double* __restrict__ part, const int2* __restrict__ tiles, int nty,
                                                          int Gx, int Gy, int accumulate, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Gx * Gy) return;
    const int x = (int)(idx / Gy), y = (int)(idx % Gy);
    const int2 tl = tiles[x / FZ_GEMM_BM];
    const size_t cell = (size_t)(x % FZ_GEMM_BM) * FZ_GEMM_BN + (y % FZ_GEMM_BN);
    double s = accumulate ? out[idx] : 0.0;
    for (int i = tl.x; i < tl.x + tl.y; ++i) s += part[((size_t)i * nty + y / FZ_GEMM_BN) * (FZ_GEMM_BM * FZ_GEMM_BN) + cell];
    out[idx] = s;
}

// ---- plotting.py:319-320: a row resampled onto the dispersion grid around its own centre: one wave per row -----------------------
// mode 0: xp[j] = pgrid[j] - cent; mode 1: xp[j] = (pgrid[j] - cent) / (1 + cent); formed on the fly with the host's roundings.
// Points beyond the ends take the end values (np.interp's default).
static __global__ __launch_bounds__(256) void k_recentre(const double* __restrict__ pdfs, int64_t N, int G, const double* __restrict__ pgrid,
                                                         const double* __restrict__ cent, int mode, int Gd,
                                                         const double* __restrict__ dgrid, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double* p = pdfs + i * G;
    double* o = out + i * Gd;
    const double c = cent[i], den = 1. + c;
    auto XP = [&](int j) { const double d = pgrid[j] - c; return mode ? d / den : d; };
    auto PV = [&](int j) { return p[j]; };
    for (int k = lane; k < Gd; k += 64) o[k] = interp1(dgrid[k], XP, PV, G);
}

// ---- plotting.py:427-431 / 501-505: CDF draws and their weighted histogram: one wave per object ----------------------------------
// Block b serves objects [b * opb, (b + 1) * opb), its waves taking them in turn.  cdf = cumsum(pdf) / cumsum(pdf)[-1] in LDS by
// k_summarize's chunked scan; draw (i, m) = np.interp(mc[i][m], grid, cdf).  Histogram: bin j holds edges[j] <= u < edges[j + 1], the
// last bin closed (np.histogram); a wave counts an object's draws per bin in LDS integers and adds weight * count to its OWN row of
// doubles, so no floating-point sum depends on scheduling; hpart[bin][block * waves + wave] are summed in order afterwards.
// LDS: [waves][G] cdf | [waves][Nbins] double | [waves][Nbins] int
static __global__ __launch_bounds__(256) void k_cdf_draws(const double* __restrict__ pdfs, int64_t N, int G, const double* __restrict__ grid,
                                                          const double* __restrict__ mc, int Nmc, const double* __restrict__ wts,
                                                          const double* __restrict__ edges, int Nbins, int opb,
                                                          double* __restrict__ draws, double* __restrict__ hpart) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* cdf = smem + (size_t)wave * G;
    double* hw = smem + (size_t)nw * G + (size_t)wave * Nbins;
    int* cnt = (int*)(smem + (size_t)nw * G + (size_t)nw * Nbins) + (size_t)wave * Nbins;
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    for (int b = lane; b < Nbins; b += 64) { hw[b] = 0.0; cnt[b] = 0; }
    wave_sync();
    const int CH = (G + 63) / 64;
    const int k0 = lane * CH, k1 = min(G, k0 + CH);
    const int64_t iend = min(N, ((int64_t)blockIdx.x + 1) * opb);
    for (int64_t i = (int64_t)blockIdx.x * opb + wave; i < iend; i += nw) {
        const double* p = pdfs + i * G;
        double sp = 0.0;
        for (int k = k0; k < k1; ++k) sp += p[k];
        double inc = sp;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const double v = __shfl_up(inc, d, 64); if (lane >= d) inc += v; }
        double run = inc - sp;
        for (int k = k0; k < k1; ++k) { run += p[k]; cdf[k] = run; }
        wave_sync();
        const double last = cdf[G - 1];
        wave_sync();
        for (int k = k0; k < k1; ++k) cdf[k] = cdf[k] / last;
        wave_sync();
        auto CDF = [&](int k) { return cdf[k]; };
        auto GRD = [&](int k) { return grid[k]; };
        for (int m = lane; m < Nmc; m += 64) {
            const double u = interp1(mc[i * Nmc + m], GRD, CDF, G);
            if (draws) draws[i * Nmc + m] = u;
            if (hpart && u >= edges[0] && u <= edges[Nbins]) {
                int lo = 0, hi = Nbins;                               // last edge <= u
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (edges[mid] <= u) lo = mid; else hi = mid - 1; }
                atomicAdd(&cnt[min(lo, Nbins - 1)], 1);
            }
        }
        wave_sync();
        if (hpart) {
            const double w = wts[i];
            for (int b = lane; b < Nbins; b += 64) { const int c = cnt[b]; if (c) { hw[b] += w * (double)c; cnt[b] = 0; } }
        }
        wave_sync();
    }
    if (hpart) {
        const int64_t P = (int64_t)gridDim.x * nw, slot = (int64_t)blockIdx.x * nw + wave;
        for (int b = lane; b < Nbins; b += 64) hpart[(int64_t)b * P + slot] = hw[b];
    }
}

}  // namespace fz
