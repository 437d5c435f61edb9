// k_hist, screen form: the objects of a launch are dealt to the waves by their expected settle cost.
//
// A wave of k_hist<screen> takes one object through all M models; what the object costs beyond the 64-pair steps every object pays is
// its settle work: the pairs whose classifier value t lies above the object's drop bar (fz_hist.h) get their weight in fp64.  That
// share differs by a factor of 30 from object to object (bright objects: a few per cent, faint ones: two thirds), and the 16 waves
// of a block meet at a barrier after every tile and at the end of every round -- a round of 16 consecutive catalogue objects lasts
// as long as its heaviest ones.  Dealt in the order of their cost, the objects of a block-round are alike.
//
// The cost is ESTIMATED from a strided sample of the models (every 256th by default, at least 64): chi2 of the pair by the launch's
// own source as k_nl_probe forms it (fz_nolist.h), t = (k/2) log2(chi2 / k) - (chi2 - k) log2(e) / 2 in fp32 (k: the power of chi2
// -- compile-time, or the object's own with per-object band counts), the count of sampled pairs above (the sample's best t) +
// ldrop0, quantised to FZ_HORDER_BINS keys.  A counting sort by key, heaviest bin first, gives order[n]: the object slot the
// launch's r-th wave-round takes.  Nothing the results read is written here; an object's pass over the models is the same
// instruction stream in the same order on whichever wave it runs, so the outputs do not depend on the order (nor on the order
// inside a bin, which the atomics leave open).  Everything is queued on the launch's stream ahead of k_hist: no host round trip.
#pragma once
#include "fz_ctx.h"
#include "fz_kernels.h"
#include "fz_hist.h"

namespace fz {

#define FZ_HORDER_BINS 64        // keys: share of the sampled pairs above the bar, in 64ths
#define FZ_HORDER_CH 64          // sampled records per LDS chunk
#define FZ_HORDER_NT 256         // threads per block: one object slot per lane

// One object slot per lane; the sampled model records go through LDS in chunks and are read back as broadcasts.  Two sweeps over
// the sample: the best t, then the count above the bar.  Writes key[slot] (< FZ_HORDER_BINS) and adds the block's key counts to hist.
template <class SRC, bool OBJK>
__global__ __launch_bounds__(FZ_HORDER_NT) void k_hist_cost(SRC src_, int64_t N, int M, int stride, int offset, int ns, float ldrop0,
                                                            const int* __restrict__ omap, uint8_t* __restrict__ key,
                                                            int* __restrict__ hist) {
    constexpr int BT = SRC::NB, RW = SRC::RW, CH = FZ_HORDER_CH, NT = FZ_HORDER_NT;
    constexpr int KOFF = SRC::LMODE == 2 ? 3 : 2;
    __shared__ __attribute__((aligned(16))) double s_rec[CH * RW];
    __shared__ int s_hist[FZ_HORDER_BINS];
    SRC src = src_;
    src.tb = global_tabs();
    const int tid = threadIdx.x;
    const int64_t slot = (int64_t)blockIdx.x * NT + tid;
    const bool live = slot < N;
    const int64_t sl = live ? slot : N - 1;
    const int64_t oi = omap ? (int64_t)omap[sl] : sl;
    typename SRC::OR ob;
    src.load_obj(oi, ob);
    int wp = SRC::WPOW;
    if constexpr (OBJK) {
        wp = __popc(src.ov.bits[oi]) - KOFF;
        if (wp < 0) wp = 1;                                       // (the object goes to the sweep; any key will do)
        if (!src.lp.dim_prior) wp = 0;
    }
    const float hk = 0.5f * (float)wp, kf = (float)wp;
    const float t0 = wp > 0 ? kf * 0.72134752f - hk * __log2f(kf) : 0.f;
    const float tzero = wp > 0 ? -INFINITY : 0.f;                  // chi2 == 0: weight 0 for every power > 0, weight 1 for power 0
    if (tid < FZ_HORDER_BINS) s_hist[tid] = 0;
    const double* rec = (SRC::LMODE == 0) ? src.mv.rec0 : src.mv.rec1;
    float best = -INFINITY;
    int cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const float bar = best + ldrop0;
        for (int c0 = 0; c0 < ns; c0 += CH) {
            const int nc = ns - c0 < CH ? ns - c0 : CH;
            __syncthreads();
            for (int e = tid; e < nc * RW; e += NT) {
                const int s = e / RW, w = e - s * RW;
                s_rec[e] = rec[((int64_t)offset + (int64_t)(c0 + s) * stride) * RW + w];      // (a model below M: see the launcher)
            }
            __syncthreads();
            for (int s = 0; s < nc; ++s) {
                typename SRC::MR m;
#pragma unroll
                for (int b = 0; b < BT; ++b) {
                    m.y[b] = s_rec[s * RW + b];
                    if (SRC::LMODE == 0) m.ye2[b] = s_rec[s * RW + BT + b];
                }
                m.bits = 0xffffffffu;
                const float cf = (float)src.chi2_of(ob, m);
                float t = fmaf(hk, __log2f(cf), fmaf(cf, -0.72134752f, t0));
                t = (cf <= (float)FZ_HIST_C2ZERO) ? tzero : t;    // the zero of a self match, as in the kernel
                if (pass == 0) best = fmaxf(best, t);
                else cnt += (t > bar) ? 1 : 0;
            }
        }
    }
    int k = (int)(((int64_t)cnt * FZ_HORDER_BINS) / ns);
    k = k < 0 ? 0 : (k > FZ_HORDER_BINS - 1 ? FZ_HORDER_BINS - 1 : k);
    if (live) { key[slot] = (uint8_t)k; atomicAdd(&s_hist[k], 1); }
    __syncthreads();
    if (tid < FZ_HORDER_BINS && s_hist[tid]) atomicAdd(&hist[tid], s_hist[tid]);
}

// one wave: cursor[b] = objects with a key above b (the heaviest bin comes first)
static __global__ __launch_bounds__(64) void k_hist_order_scan(const int* __restrict__ hist, int* __restrict__ cursor) {
    __shared__ int s[FZ_HORDER_BINS];
    const int b = threadIdx.x;
    s[b] = hist[b];
    __syncthreads();
    int above = 0;
    for (int q = b + 1; q < FZ_HORDER_BINS; ++q) above += s[q];
    cursor[b] = above;
}

// the scatter: a block ranks its slots per key in LDS, reserves a run per key with one global atomic, and writes the slots there
static __global__ __launch_bounds__(FZ_HORDER_NT) void k_hist_order_scatter(const uint8_t* __restrict__ key, int64_t N, int* __restrict__ cursor,
                                                                            int* __restrict__ order) {
    __shared__ int s_cnt[FZ_HORDER_BINS], s_base[FZ_HORDER_BINS];
    const int tid = threadIdx.x;
    const int64_t slot = (int64_t)blockIdx.x * FZ_HORDER_NT + tid;
    if (tid < FZ_HORDER_BINS) s_cnt[tid] = 0;
    __syncthreads();
    const bool live = slot < N;
    const int k = live ? (int)key[slot] : 0;
    int rank = 0;
    if (live) rank = atomicAdd(&s_cnt[k], 1);
    __syncthreads();
    if (tid < FZ_HORDER_BINS && s_cnt[tid]) s_base[tid] = atomicAdd(&cursor[tid], s_cnt[tid]);
    __syncthreads();
    if (live) {
        const int64_t pos = (int64_t)s_base[k] + rank;
        if (pos >= 0 && pos < N) order[pos] = (int)slot;           // (always: the runs partition [0, N))
    }
}

}  // namespace fz

// Queues cost kernel, scan and scatter on c->stream; *order_out is the device array of n slot indices (c->d_horder).  `stride` <= 0:
// every 256th model.  The sample never takes fewer than min(M, 64) models: a shorter one is no estimate.
template <class SRC, bool OBJK>
int fz_hist_order_build(fz_ctx* c, const SRC& src, int64_t n, int64_t M, double wt_thresh, int64_t stride, int64_t offset, const int** order_out) {
    if (stride <= 0) stride = 256;
    if (M / stride < 64) stride = std::max<int64_t>(1, M / 64);
    offset = offset < 0 ? 0 : offset % stride;
    const int ns = (int)((M - offset + stride - 1) / stride);      // models offset, offset + stride, ... < M
    // the kernel's drop bar (fz_hist.h): 2^-(55 + ceil log2 M) of the best weight, never above the stacking threshold
    int mbits = 0;
    while (((int64_t)1 << mbits) < M) ++mbits;
    const float lthr2 = (wt_thresh > 0.0) ? (float)std::log2(wt_thresh) : -INFINITY;
    const float ldrop0 = std::min(lthr2, -(float)(55 + mbits));
    // [key counts | cursors | order: n slots | keys: n bytes]
    const size_t head = 2 * FZ_HORDER_BINS * sizeof(int);
    FZCHK(c->d_horder.ensure(head + (size_t)n * (sizeof(int) + 1)));
    int* hist = c->d_horder.as<int>(); int* cursor = hist + FZ_HORDER_BINS; int* order = cursor + FZ_HORDER_BINS;
    uint8_t* key = reinterpret_cast<uint8_t*>(order + n);
    HIPCHK(hipMemsetAsync(hist, 0, head, c->stream));
    const unsigned nb = (unsigned)((n + FZ_HORDER_NT - 1) / FZ_HORDER_NT);
    hipLaunchKernelGGL((fz::k_hist_cost<SRC, OBJK>), dim3(nb), dim3(FZ_HORDER_NT), 0, c->stream, src, n, (int)M, (int)stride, (int)offset, ns,
                       ldrop0, c->omap, key, hist);
    hipLaunchKernelGGL(fz::k_hist_order_scan, dim3(1), dim3(64), 0, c->stream, hist, cursor);
    hipLaunchKernelGGL(fz::k_hist_order_scatter, dim3(nb), dim3(FZ_HORDER_NT), 0, c->stream, key, n, cursor, order);
    HIPCHK(hipGetLastError());
    *order_out = order;
    return 0;
}
