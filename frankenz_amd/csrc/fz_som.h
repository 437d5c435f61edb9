// Training of a self-organizing map (SelfOrganizingMap._train_network, networks.py:1804-1867): ONE persistent workgroup per map
// runs the sequential step loop itself.  Each step draws one (cleaned) model row, takes its ln-probability against every node (the
// nodes act as noiseless, unmasked models), finds the best-matching unit, weighs every node by its grid distance to it, selects the
// nodes by the wt_thresh or the CDF rule and moves them towards the row.  Every node is owned by ONE thread for the whole launch
// (node n by thread n mod NT), so the node work of a step needs no barrier; the BMU reduction is the one barrier of a step under the
// wt_thresh rule (five under the CDF rule).  The nodes and their grid positions live in LDS when they fit (NODES_LDS), otherwise in
// global memory, still owned by the one workgroup.  Draw indices, learning rates and sigmas are host tables; the rows of TRAIN_CHUNK
// steps are staged into LDS together (one exposed global-load latency per chunk instead of per step).  The staging, the
// ln-probability and the arg-max order are fz_train.h's, shared with the growing neural gas.  docs/som.md.
#pragma once
#include "fz_train.h"

namespace fz {

#define SOM_MAXPROJ 8       // grid dimensions

struct SomArgs {
    const double* x;        // (M, B) cleaned model values
    const double* xe;       // (M, B) cleaned model errors
    const double* xm;       // (M, B) cleaned mask (0/1)
    const double* rowk;     // (M, 4) k_train_rowk
    double* nodes;          // (NNODE, B) in/out
    const int32_t* pos;     // (NNODE, NPROJ) integer grid positions
    const int64_t* draws;   // (T) row drawn at each step
    const double* lr;       // (T) learning rate
    const double* sig;      // (T) neighbourhood sigma
    int32_t* bmus;          // (T) out
    int64_t s0, s1;         // step range
    int nnode, nproj, B;    // nproj <= SOM_MAXPROJ
    int kind;               // 0 Gaussian exp(-0.5 d / s^2), 1 Lorentzian s^2 / (d + s^2)
    int use_wt;             // 1: w > wt_thresh * max(w); 0: the CDF rule
    double wt_thresh, cdf_thresh;
    int free_scale, dim_prior, modec, track_scale;
    int dmax;               // largest squared grid distance (CDF rule: histogram bins 0..dmax)
};

// per-step record staged in LDS: the head (fz_train.h), then lr sig
__host__ __device__ constexpr int som_rec_width(int B) { return train_rec_head(B) + 2; }
// the LDS of k_som_train besides the resident nodes and the CDF rule's histogram, in doubles: recs | red 2*2*16 | scan 16*2 | bnd 4
__host__ __device__ constexpr int som_fixed_lds_doubles(int B) { return TRAIN_CHUNK * som_rec_width(B) + 32 + 16 + 16 + 8 + 4; }

__device__ __forceinline__ double som_weight(int kind, double d, double s2) {
    return kind == 0 ? exp(-0.5 * d / s2) : s2 / (d + s2);        // networks.py:81, 111: the reference's operation order
}

template <bool NODES_LDS>
__global__ __launch_bounds__(TRAIN_NT) void k_som_train(SomArgs a) {
    extern __shared__ double s_som[];
    const int t = threadIdx.x, NT = blockDim.x, lane = t & 63, wave = t >> 6, NW = NT >> 6;
    const int B = a.B, RW = som_rec_width(B), NN = a.nnode, NP = a.nproj;
    // LDS layout: [nodes NN*B] [pos NN*NP ints, padded to doubles] | som_fixed_lds_doubles(B): recs, red, scan, bnd | hist
    double* base = s_som;
    double* Y = a.nodes;
    const int32_t* P = a.pos;
    if (NODES_LDS) {
        Y = base; base += (size_t)NN * B;
        P = reinterpret_cast<const int32_t*>(base); base += ((size_t)NN * NP + 1) / 2;
        int32_t* Pw = reinterpret_cast<int32_t*>(Y + (size_t)NN * B);
        for (int e = t; e < NN * B; e += NT) Y[e] = a.nodes[e];
        for (int e = t; e < NN * NP; e += NT) Pw[e] = a.pos[e];
    }
    double* rec = base; base += TRAIN_CHUNK * RW;
    double* redv = base; base += 2 * 16;                         // BMU: value per wave, two buffers (step parity)
    int* redi = reinterpret_cast<int*>(base); base += 16;        //      index per wave (2 * 16 ints)
    double* scw = base; base += 16;                              // CDF: weight sum per wave
    int* scc = reinterpret_cast<int*>(base); base += 8;          //      straddling tie group: members per wave (16 ints)
    double* bnd = base; base += 4;                               //      boundary: wB, k_group, straddle, first bin (int)
    int* hist = reinterpret_cast<int*>(base);                    //      counts per squared distance, 0 .. dmax
    const int nbins = a.use_wt ? 0 : a.dmax + 1;
    const int bpt = (nbins + NT - 1) / NT;                       // bins per thread (the thread's bins are contiguous)
    for (int e = t; e < nbins; e += NT) hist[e] = 0;

    for (int64_t c0 = a.s0; c0 < a.s1; c0 += TRAIN_CHUNK) {
        const int nc = (int)((a.s1 - c0) < TRAIN_CHUNK ? (a.s1 - c0) : TRAIN_CHUNK);
        train_stage(a, c0, nc, rec, RW, t, NT, [&](int64_t step, int64_t, double* tail) { tail[0] = a.lr[step]; tail[1] = a.sig[step]; });
        for (int r = 0; r < nc; ++r) {
            const int64_t step = c0 + r;
            const double* R = rec + r * RW;
            const TrainRow row = train_row(R, B);
            const double lr = R[train_rec_head(B)], sg = R[train_rec_head(B) + 1];
            // ---- node ln-probabilities, the track_scale rescale, the local argmax ----
            double bv = -INFINITY; int bi = 0x7fffffff;
            for (int n = t; n < NN; n += NT) {
                double chi2;
                const double lnl = train_lnl(a, row, Y + (size_t)n * B, chi2);
                if (train_better(lnl, n, bv, bi)) { bv = lnl; bi = n; }
            }
            train_argmax_butterfly(bv, bi);
            const int par = (int)(step & 1);
            if (lane == 0) { redv[par * 16 + wave] = bv; redi[par * 16 + wave] = bi; }
            __syncthreads();
            bv = redv[par * 16]; bi = redi[par * 16];
            for (int w = 1; w < NW; ++w) {
                const double ov = redv[par * 16 + w]; const int oi = redi[par * 16 + w];
                if (train_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            const int bmu = bi;
            if (t == 0) a.bmus[step] = bmu;
            // ---- neighbour weights (exact squared grid distances) ----
            const double s2 = sg * sg;
            int pb[SOM_MAXPROJ];
#pragma unroll
            for (int p = 0; p < SOM_MAXPROJ; ++p) pb[p] = p < NP ? P[(size_t)bmu * NP + p] : 0;
            auto sqd = [&](int n) {                                  // networks.py:80: sum((pos - positions)**2), exact in fp64
                double d = 0.0;
#pragma unroll
                for (int p = 0; p < SOM_MAXPROJ; ++p)
                    if (p < NP) { const double q = (double)(pb[p] - P[(size_t)n * NP + p]); d += q * q; }
                return d;
            };
            // ---- selection ----
            double wlim = 0.0, wB = INFINITY; int kgrp = 0, straddle = 0;
            if (a.use_wt) {
                // max(w) is the weight at distance 0: both kernels are non-increasing in d, and a nan anywhere (sigma = 0 or inf)
                // is also a nan at d = 0, which np.max returns
                wlim = a.wt_thresh * som_weight(a.kind, 0.0, s2);
            } else {
                // The reference sorts the weights ascending and keeps the prefix whose running probability stays <= 1 - cdf_thresh
                // (networks.py:1859-1863).  The weight is a function of the squared distance alone and non-increasing in it, so the
                // ascending order is the descending order of d: a histogram of d and a scan over it give the boundary.
                for (int n = t; n < NN; n += NT) atomicAdd(&hist[(int)sqd(n)], 1);
                __syncthreads();
                // thread t owns scan positions q in [t*bpt, (t+1)*bpt) ; position q is bin dmax - q (ascending weight)
                double lw = 0.0;
                for (int k = 0; k < bpt; ++k) {
                    const int q = t * bpt + k;
                    if (q < nbins) { const int c = hist[a.dmax - q]; if (c) { lw += (double)c * som_weight(a.kind, (double)(a.dmax - q), s2); } }
                }
                double iw = lw;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const double qw = __shfl_up(iw, o, 64);
                    if (lane >= o) iw += qw;
                }
                if (lane == 63) scw[wave] = iw;
                __syncthreads();
                double S = 0.0, pw = 0.0;
                for (int w = 0; w < NW; ++w) { S += scw[w]; if (w < wave) pw += scw[w]; }
                double cw = pw + iw - lw;                                    // exclusive prefix of this thread's first bin
                const double lim = 1.0 - a.cdf_thresh;
                int* qb = reinterpret_cast<int*>(bnd + 3);
                if (t == 0) { bnd[0] = INFINITY; bnd[1] = 0.0; bnd[2] = 0.0; *qb = nbins; }
                if (t == 0 && !(S == S)) bnd[0] = -INFINITY;                 // a nan weight: every cdf is nan, nothing is kept
                __syncthreads();
                // the boundary is the first bin (ascending weight) whose nodes do not all fit: each thread finds its own first such
                // bin, the smallest over the workgroup wins.  No such bin: every node fits and wB stays +inf (all kept); the first
                // bin already failing (lim < 0 or nan, cdf_thresh >= 1) keeps none -- both as the reference's prefix rule
                int myq = nbins; double mycw = 0.0;
                if (S == S) {
                    for (int k = 0; k < bpt; ++k) {
                        const int q = t * bpt + k;
                        if (q >= nbins) break;
                        const int c = hist[a.dmax - q];
                        if (!c) continue;
                        const double w = som_weight(a.kind, (double)(a.dmax - q), s2);
                        if (!((cw + (double)c * w) / S <= lim)) { myq = q; mycw = cw; break; }
                        cw += (double)c * w;
                    }
                    if (myq < nbins) atomicMin(qb, myq);
                }
                __syncthreads();
                const int q = *qb;
                if (q < nbins && q == myq) {
                    // the boundary bin: e of its c nodes fit (the running probability after the e-th stays <= lim)
                    const int c = hist[a.dmax - q];
                    const double w = som_weight(a.kind, (double)(a.dmax - q), s2);
                    double ed = (w > 0.0) ? floor((lim * S - mycw) / w) : ((mycw / S <= lim) ? (double)c : 0.0);
                    if (!(ed >= 0.0)) ed = 0.0;                                 // (nan too)
                    if (ed > (double)c) ed = (double)c;
                    int e = (int)ed;
                    while (e < c && (mycw + (double)(e + 1) * w) / S <= lim) ++e;
                    while (e > 0 && !((mycw + (double)e * w) / S <= lim)) --e;
                    // the tie group of equal weights may span neighbouring bins: the nodes below it are kept, e + the group's
                    // members in earlier bins of it are kept from the group, in node-index order
                    int before = 0, after = 0;
                    for (int qq = q - 1; qq >= 0 && som_weight(a.kind, (double)(a.dmax - qq), s2) == w; --qq) before += hist[a.dmax - qq];
                    for (int qq = q + 1; qq < nbins && som_weight(a.kind, (double)(a.dmax - qq), s2) == w; ++qq) after += hist[a.dmax - qq];
                    const int kg = before + e, gsz = before + c + after;
                    bnd[0] = w; bnd[1] = (double)kg; bnd[2] = (kg > 0 && kg < gsz) ? 1.0 : 0.0;
                }
                __syncthreads();
                wB = bnd[0]; kgrp = (int)bnd[1]; straddle = bnd[2] != 0.0;
                for (int k = 0; k < bpt; ++k) { const int q = t * bpt + k; if (q < nbins) hist[a.dmax - q] = 0; }
            }
            // ---- update (networks.py:1866-1867), node-index rank inside a straddling tie group ----
            int rank_base = 0;
            for (int n0 = 0; n0 < NN; n0 += NT) {
                const int n = n0 + t;
                double w = 0.0; bool keep = false, ingrp = false;
                if (n < NN) {
                    w = som_weight(a.kind, sqd(n), s2);
                    if (a.use_wt) keep = w > wlim;
                    else { keep = w < wB; ingrp = (w == wB); if (ingrp && !straddle) keep = kgrp > 0; }
                }
                if (straddle) {                                       // uniform branch
                    int tot;
                    const int rk = rank_base + train_rank(ingrp, scc, lane, wave, NW, tot);
                    if (ingrp) keep = rk < kgrp;
                    rank_base += tot;
                }
                if (keep) {
                    double* y = Y + (size_t)n * B;
                    const double f = lr * w;
                    for (int b = 0; b < B; ++b) y[b] = y[b] + f * (row.x[b] - y[b]);
                }
            }
        }
    }
    if (NODES_LDS) {
        __syncthreads();
        for (int e = t; e < NN * B; e += NT) a.nodes[e] = Y[e];
    }
}

}  // namespace fz
