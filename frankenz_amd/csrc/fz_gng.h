// Training of a growing neural gas (GrowingNeuralGas._train_network, networks.py:2037-2260): ONE persistent workgroup per network
// runs the sequential step loop itself, batch ends included.  A step draws one (cleaned) model row, takes its ln-probability against
// every live node (noiseless, unmasked models: train_lnl of fz_train.h), finds the best and the second-best node, moves the best
// node and its graph neighbours towards the row, resets or creates the edge between the two and ages the best node's edges.  Every
// nbatch steps the edges that reached max_age are removed, nodes left without edges are dropped (the slots are compacted, so slot
// order is always the reference's node order) and a node is inserted next to the one with the largest accumulated error.
//   * Slot n is owned by thread n mod NT in the all-node phases (likelihood, error decay, arg-max); wave 0 alone applies a step's
//     updates between the two barriers of a step.
//   * Fit copy of the nodes, errors and degrees live in LDS when they fit (NODES_LDS), otherwise in the global state arrays.  Under
//     track_scale the fit copy (rescaled after every fit) differs from the graph positions: the fit copy stays in LDS, the positions
//     are updated in global memory.
//   * Adjacency: a fixed-capacity ordered list of (neighbour slot, edge id) per slot, in global memory (two buffers: a compaction
//     rewrites one into the other).  Edge ids are handed out in creation order and never reused; the age of an edge is age[id].
// docs/gng.md.
#pragma once
#include "fz_train.h"

namespace fz {

#define GNG_NCNT 16         // counters at the head of the integer state
enum { GNG_NN = 0, GNG_NP, GNG_EC, GNG_STATUS, GNG_STEP, GNG_AL0, GNG_AL1, GNG_CUR, GNG_REM };
enum { GNG_OK = 0, GNG_E_DEGREE = 1, GNG_E_PRUNE = 2, GNG_E_NODES = 3, GNG_E_EDGES = 4 };

struct GngArgs {
    const double* x;        // (M, B) cleaned model values
    const double* xe;       // (M, B) cleaned model errors
    const double* xm;       // (M, B) cleaned mask (0/1)
    const double* rowk;     // (M, 4) k_train_rowk
    const int64_t* draws;   // (T) row drawn at each step
    double* fstate;         // pos[cap*B] fit[cap*B] err[cap] alias_rows[2*B]
    int32_t* istate;        // cnt[GNG_NCNT] deg[cap] aux[cap] adj[2][cap*md](nbr, edge) prune[pcap](u, v, edge) age[ecap]
    int64_t* ids;           // (cap) node labels, slot order
    int64_t* bmus;          // (T) out: label of the best node
    int32_t* batch;         // (number of batch ends, 2) out: live nodes after, prune entries at the batch end
    int64_t s0, s1;         // step range
    int64_t nnode_init;     // the label of the node inserted at batch end k is nnode_init + k
    int64_t alias0, alias1; // model rows that ARE the positions of the nodes labelled 0 and 1 (-1: none)
    int B, cap, md, pcap, ecap;
    int nbatch, max_age, max_nodes;
    double learn_best, learn_nbr, f_new, f_all;       // f_new = 1 - new_err_dec, f_all = 1 - all_err_dec
    int free_scale, dim_prior, modec, track_scale;
};

// per-step record staged in LDS: the head (fz_train.h), then alias
__host__ __device__ constexpr int gng_rec_width(int B) { return train_rec_head(B) + 1; }
__host__ __device__ constexpr int gng_fixed_lds_doubles(int B) { return TRAIN_CHUNK * gng_rec_width(B) + 16 * 3 + 16 + 8 + 8; }

// heapq.nlargest order: the larger value, ties to the earlier node (nan ln-probs are mapped to -inf before)
__device__ __forceinline__ bool gng_better(double va, int ia, double vb, int ib) { return va > vb || (va == vb && ia < ib); }

struct GngTop { double v1, c1, v2; int i1, i2; };

__device__ __forceinline__ void gng_merge(GngTop& a, double ov1, int oi1, double oc1, double ov2, int oi2) {
    if (gng_better(ov1, oi1, a.v1, a.i1)) {
        if (gng_better(a.v1, a.i1, ov2, oi2)) { a.v2 = a.v1; a.i2 = a.i1; } else { a.v2 = ov2; a.i2 = oi2; }
        a.v1 = ov1; a.i1 = oi1; a.c1 = oc1;
    } else if (gng_better(ov1, oi1, a.v2, a.i2)) { a.v2 = ov1; a.i2 = oi1; }
}

__device__ __forceinline__ void gng_top_butterfly(GngTop& tp) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov1 = __shfl_xor(tp.v1, o, 64), oc1 = __shfl_xor(tp.c1, o, 64), ov2 = __shfl_xor(tp.v2, o, 64);
        const int oi1 = __shfl_xor(tp.i1, o, 64), oi2 = __shfl_xor(tp.i2, o, 64);
        gng_merge(tp, ov1, oi1, oc1, ov2, oi2);
    }
}

// Stable in-place compaction of the rows of the surviving slots (newslot[s] >= 0, and <= s): every element moves to a lower or equal
// index, so reading a block of NT elements, a barrier and then writing them never overwrites an element that is still to be read.
template <class T>
__device__ __forceinline__ void gng_compact(T* arr, int width, int nslots, const int* newslot, int t, int NT) {
    const int total = nslots * width;
    for (int base = 0; base < total; base += NT) {
        const int e = base + t;
        bool mv = false; T v = T(); int d = 0;
        if (e < total) {
            const int s = e / width, ns = newslot[s];
            if (ns >= 0 && ns != s) { v = arr[e]; d = ns * width + (e - s * width); mv = true; }
        }
        __syncthreads();
        if (mv) arr[d] = v;
        __syncthreads();
    }
}

template <bool NODES_LDS>
__global__ __launch_bounds__(TRAIN_NT) void k_gng_train(GngArgs a) {
    extern __shared__ double s_gng[];
    const int t = threadIdx.x, NT = blockDim.x, lane = t & 63, wave = t >> 6, NW = NT >> 6;
    const int B = a.B, RW = gng_rec_width(B), CAP = a.cap, MD = a.md;
    // the state in global memory
    double* gP = a.fstate; double* gY = gP + (size_t)CAP * B; double* gE = gY + (size_t)CAP * B; double* arow = gE + CAP;
    int* cnt = a.istate; int* gD = cnt + GNG_NCNT; int* gX = gD + CAP;
    int2* adj = reinterpret_cast<int2*>(gX + CAP);
    int* plist = reinterpret_cast<int*>(adj + 2 * (size_t)CAP * MD);
    int* age = plist + 3 * (size_t)a.pcap;
    // LDS layout: [fit CAP*B] [err CAP] [deg CAP ints] [aux CAP ints] | recs TRAIN_CHUNK*RW | red 16*3 | redi 16*2 ints | scan 16 ints | sh 16 ints
    double* base = s_gng;
    double *Y, *P, *E; int *D, *X;                                   // fit copy, graph positions, errors, degrees, aux (0 outside batch ends)
    if (NODES_LDS) {
        Y = base; base += (size_t)CAP * B; E = base; base += CAP;
        D = reinterpret_cast<int*>(base); base += (CAP + 1) / 2;
        X = reinterpret_cast<int*>(base); base += (CAP + 1) / 2;
        P = a.track_scale ? gP : Y;
    } else {
        P = gP; Y = a.track_scale ? gY : gP; E = gE; D = gD; X = gX;
    }
    double* rec = base; base += TRAIN_CHUNK * RW;
    double* red = base; base += 16 * 3;
    int* redi = reinterpret_cast<int*>(base); base += 16;
    int* sc = reinterpret_cast<int*>(base); base += 8;
    int* sh = reinterpret_cast<int*>(base);
    if (t < GNG_NCNT) sh[t] = cnt[t];
    {
        const int n0 = cnt[GNG_NN];
        if (NODES_LDS) {
            const double* src = a.track_scale ? gY : gP;
            for (int e = t; e < n0 * B; e += NT) Y[e] = src[e];
            for (int e = t; e < n0; e += NT) { E[e] = gE[e]; D[e] = gD[e]; }
            for (int e = t; e < CAP; e += NT) X[e] = 0;
        }
    }
    __syncthreads();
    bool pend = false, stop = false;                                 // the previous step's error decay is still to be applied

    for (int64_t c0 = a.s0; c0 < a.s1 && !stop; c0 += TRAIN_CHUNK) {
        const int nc = (int)((a.s1 - c0) < TRAIN_CHUNK ? (a.s1 - c0) : TRAIN_CHUNK);
        train_stage(a, c0, nc, rec, RW, t, NT, [&](int64_t, int64_t j, double* tail) { tail[0] = j == a.alias0 ? 0.0 : (j == a.alias1 ? 1.0 : -1.0); });
        for (int r = 0; r < nc && !stop; ++r) {
            const int64_t step = c0 + r;
            double* R = rec + r * RW;
            const int al = (int)R[train_rec_head(B)];
            if (al >= 0) {
                // the drawn row IS a node's position (the reference's initial nodes are views of the caller's rows): read it live;
                // a removed node left its last position in the row
                const int sl = sh[GNG_AL0 + al];
                if (t < B) R[t] = sl >= 0 ? P[(size_t)sl * B + t] : arow[al * B + t];
                __syncthreads();
            }
            const TrainRow row = train_row(R, B);
            int NN = sh[GNG_NN];
            // ---- the previous step's error decay, node ln-probabilities, the track_scale rescale, the local top two ----
            GngTop tp; tp.v1 = -INFINITY; tp.c1 = 0.0; tp.v2 = -INFINITY; tp.i1 = 0x7fffffff; tp.i2 = 0x7fffffff;
            for (int n = t; n < NN; n += NT) {
                if (pend) E[n] = E[n] * a.f_all;
                double chi2;
                double lnl = train_lnl(a, row, Y + (size_t)n * B, chi2);
                if (lnl != lnl) lnl = -INFINITY;                          // nan ln-probs count as the lowest (docs/deviations.md)
                gng_merge(tp, lnl, n, chi2, -INFINITY, 0x7fffffff);
            }
            pend = true;
            gng_top_butterfly(tp);
            if (lane == 0) { red[wave * 3] = tp.v1; red[wave * 3 + 1] = tp.c1; red[wave * 3 + 2] = tp.v2; redi[wave * 2] = tp.i1; redi[wave * 2 + 1] = tp.i2; }
            __syncthreads();                                              // barrier 1
            if (wave == 0) {
                tp.v1 = -INFINITY; tp.c1 = 0.0; tp.v2 = -INFINITY; tp.i1 = 0x7fffffff; tp.i2 = 0x7fffffff;
                if (lane < NW) { tp.v1 = red[lane * 3]; tp.c1 = red[lane * 3 + 1]; tp.v2 = red[lane * 3 + 2]; tp.i1 = redi[lane * 2]; tp.i2 = redi[lane * 2 + 1]; }
                gng_top_butterfly(tp);
                const int bmu = tp.i1, bmu2 = tp.i2;
                const double chi2b = tp.c1;
                if (lane == 0) a.bmus[step] = a.ids[bmu];
                // ---- the best node (networks.py:2180-2184) ----
                if (lane < B) {
                    const size_t o = (size_t)bmu * B + lane;
                    const double d = a.learn_best * (row.x[lane] - P[o]);
                    P[o] = P[o] + d;
                    if (a.track_scale) Y[o] = Y[o] + d;
                }
                if (lane == 0) E[bmu] = E[bmu] + chi2b;
                // ---- the edge to the second-best node: rejuvenated or created (2186-2191) ----
                int2* A = adj + (size_t)sh[GNG_CUR] * CAP * MD;
                int d = D[bmu];
                int2 ent = make_int2(-1, -1);
                int ag = 0;
                if (lane < d) { ent = A[(size_t)bmu * MD + lane]; ag = age[ent.y]; }
                const unsigned long long hit = __ballot(lane < d && ent.x == bmu2);
                int err = GNG_OK;
                if (hit) {
                    if (lane < d && ent.x == bmu2) ag = 0;
                } else {
                    const int d2 = D[bmu2], ec = sh[GNG_EC];
                    if (d >= MD || d2 >= MD) err = GNG_E_DEGREE;
                    else if (ec >= a.ecap) err = GNG_E_EDGES;
                    else {
                        if (lane == 0) {
                            A[(size_t)bmu * MD + d] = make_int2(bmu2, ec); A[(size_t)bmu2 * MD + d2] = make_int2(bmu, ec);
                            D[bmu] = d + 1; D[bmu2] = d2 + 1; sh[GNG_EC] = ec + 1;
                        }
                        if (lane == d) { ent = make_int2(bmu2, ec); ag = 0; }
                        d += 1;
                    }
                }
                // ---- the neighbours, one lane each (2193-2202) ----
                if (err == GNG_OK) {
                    const bool act = lane < d;
                    if (act) {
                        const size_t o = (size_t)ent.x * B;
                        for (int b = 0; b < B; ++b) {
                            const double dd = a.learn_nbr * (row.x[b] - P[o + b]);
                            P[o + b] = P[o + b] + dd;
                            if (a.track_scale) Y[o + b] = Y[o + b] + dd;
                        }
                        ag += 1;
                        age[ent.y] = ag;
                    }
                    const bool pr = act && ag == a.max_age;
                    const unsigned long long bal = __ballot(pr);
                    if (bal) {
                        const int np = sh[GNG_NP], add = __builtin_popcountll(bal);
                        if (np + add > a.pcap) err = GNG_E_PRUNE;
                        else {
                            const int pre = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
                            if (pr) { int* q = plist + 3 * (size_t)(np + pre); q[0] = bmu; q[1] = ent.x; q[2] = ent.y; }
                            if (lane == 0) sh[GNG_NP] = np + add;
                        }
                    }
                }
                if (err != GNG_OK && lane == 0) { sh[GNG_STATUS] = err; sh[GNG_STEP] = (int)step; }
            }
            __syncthreads();                                              // barrier 2
            if (sh[GNG_STATUS]) { stop = true; break; }
            if (step % a.nbatch != 0) continue;

            // ================= batch end (networks.py:2204-2254) =================
            const int bi = (int)(step / a.nbatch);
            const int np = sh[GNG_NP];
            int cur = sh[GNG_CUR];
            int2* A = adj + (size_t)cur * CAP * MD;
            if (t == 0) { a.batch[2 * bi + 1] = np; sh[GNG_REM] = 0; }
            // ---- prune: every listed edge that still exists goes, whatever its age is now; the outcome does not depend on the order
            for (int p = t; p < np; p += NT) {
                const int* q = plist + 3 * (size_t)p;
                age[q[2]] = -1; X[q[0]] = 1; X[q[1]] = 1;
            }
            __syncthreads();
            for (int n = t; n < NN; n += NT) {
                if (!X[n]) continue;
                int2* L = A + (size_t)n * MD;
                const int dn = D[n];
                int k2 = 0;
                for (int k = 0; k < dn; ++k) {
                    const int2 ent = L[k];
                    if (age[ent.y] >= 0) { if (k2 != k) L[k2] = ent; ++k2; }
                }
                D[n] = k2;
                if (k2 == 0) { X[n] = 2; sh[GNG_REM] = 1; } else X[n] = 0;     // a node left without neighbours is removed
            }
            __syncthreads();
            if (sh[GNG_REM]) {
                // ---- stable compaction of the surviving slots: aux becomes the new slot (or -1) ----
                int run = 0;
                for (int b0 = 0; b0 < NN; b0 += NT) {
                    const int n = b0 + t;
                    const bool alive = n < NN && X[n] != 2;
                    int tot;
                    const int ns = run + train_rank(alive, sc, lane, wave, NW, tot);
                    if (n < NN) X[n] = alive ? ns : -1;
                    run += tot;
                }
                __syncthreads();                                          // every new slot is written
                if (t < 2) {                                              // the aliased rows follow their nodes
                    const int sl = sh[GNG_AL0 + t];
                    if (sl >= 0) {
                        if (X[sl] < 0) { for (int b = 0; b < B; ++b) arow[t * B + b] = P[(size_t)sl * B + b]; sh[GNG_AL0 + t] = -1; }
                        else sh[GNG_AL0 + t] = X[sl];
                    }
                }
                int2* A2 = adj + (size_t)(cur ^ 1) * CAP * MD;
                for (int s = wave; s < NN; s += NW) {
                    const int ns = X[s];
                    if (ns < 0) continue;
                    const int ds = D[s];
                    for (int k = lane; k < ds; k += 64) { int2 ent = A[(size_t)s * MD + k]; ent.x = X[ent.x]; A2[(size_t)ns * MD + k] = ent; }
                }
                __syncthreads();
                gng_compact(P, B, NN, X, t, NT);
                gng_compact(E, 1, NN, X, t, NT);
                gng_compact(D, 1, NN, X, t, NT);
                gng_compact(a.ids, 1, NN, X, t, NT);
                for (int n = t; n < NN; n += NT) X[n] = 0;
                cur ^= 1; A = A2; NN = run;
                if (t == 0) { sh[GNG_NN] = run; sh[GNG_CUR] = cur; }
                __syncthreads();
            }
            if (NN < 2) {                                                 // (the reference fails here too: nlargest(2) / an empty arg-max)
                if (t == 0) { sh[GNG_STATUS] = GNG_E_NODES; sh[GNG_STEP] = (int)step; }
                stop = true;
            } else if (NN < a.max_nodes) {
                // ---- insertion (2221-2243): e1 = first arg-max of the errors, e2 = first arg-max among e1's neighbours ----
                double bv = -INFINITY; int bix = 0x7fffffff;
                for (int n = t; n < NN; n += NT) { const double v = E[n]; if (train_better(v, n, bv, bix)) { bv = v; bix = n; } }
                train_argmax_butterfly(bv, bix);
                if (lane == 0) { red[wave] = bv; redi[wave] = bix; }
                __syncthreads();
                if (wave == 0) {
                    bv = -INFINITY; bix = 0x7fffffff;
                    if (lane < NW) { bv = red[lane]; bix = redi[lane]; }
                    train_argmax_butterfly(bv, bix);
                    const int e1 = bix, ec = sh[GNG_EC];
                    const int d1 = D[e1];
                    int2 ent1 = make_int2(-1, -1);
                    double ev = -INFINITY; int ei = 0x7fffffff;
                    if (lane < d1) { ent1 = A[(size_t)e1 * MD + lane]; ev = E[ent1.x]; ei = lane; }
                    train_argmax_butterfly(ev, ei);
                    const int k2 = ei, e2 = d1 ? __shfl(ent1.x, k2 & 63, 64) : e1;
                    const int d2 = D[e2];
                    int2 ent2 = make_int2(-1, -1);
                    if (lane < d2) ent2 = A[(size_t)e2 * MD + lane];
                    const unsigned long long h2 = __ballot(lane < d2 && ent2.x == e1);
                    const int k1 = h2 ? __builtin_ctzll(h2) : d2;
                    if (d1 == 0 || !h2) {                                 // an isolated node (graph_init): the reference's arg-max of nothing
                        if (lane == 0) { sh[GNG_STATUS] = GNG_E_NODES; sh[GNG_STEP] = (int)step; }
                    } else if (ec + 2 > a.ecap) {
                        if (lane == 0) { sh[GNG_STATUS] = GNG_E_EDGES; sh[GNG_STEP] = (int)step; }
                    } else {
                        // edge (e1, e2) leaves both lists (the later entries move up), the new node is appended to both
                        if (lane < d1 && lane > k2) A[(size_t)e1 * MD + lane - 1] = ent1;
                        if (lane < d2 && lane > k1) A[(size_t)e2 * MD + lane - 1] = ent2;
                        if (lane < B) P[(size_t)NN * B + lane] = 0.5 * (P[(size_t)e1 * B + lane] + P[(size_t)e2 * B + lane]);
                        if (lane == 0) {
                            A[(size_t)e1 * MD + d1 - 1] = make_int2(NN, ec); A[(size_t)e2 * MD + d2 - 1] = make_int2(NN, ec + 1);
                            A[(size_t)NN * MD] = make_int2(e1, ec); A[(size_t)NN * MD + 1] = make_int2(e2, ec + 1);
                            age[ec] = 0; age[ec + 1] = 0; D[NN] = 2;
                            const double f1 = E[e1] * a.f_new;
                            E[e1] = f1; E[e2] = E[e2] * a.f_new; E[NN] = f1;
                            a.ids[NN] = a.nnode_init + bi;
                            sh[GNG_NN] = NN + 1; sh[GNG_EC] = ec + 2;
                        }
                    }
                }
                __syncthreads();
                if (sh[GNG_STATUS]) stop = true;
                NN = sh[GNG_NN];
            }
            if (!stop) {
                if (a.track_scale) for (int e = t; e < NN * B; e += NT) Y[e] = P[e];      // the fit copy is rebuilt from the graph (2245-2251)
                if (t == 0) { a.batch[2 * bi] = NN; sh[GNG_NP] = 0; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int NN = sh[GNG_NN];
    if (pend && !stop) for (int n = t; n < NN; n += NT) E[n] = E[n] * a.f_all;
    __syncthreads();
    if (t < 2 * B) {
        const int al = t / B, b = t - al * B, sl = sh[GNG_AL0 + al];
        if (sl >= 0) arow[al * B + b] = P[(size_t)sl * B + b];
    }
    if (NODES_LDS) {
        double* dst = a.track_scale ? gY : gP;
        for (int e = t; e < NN * B; e += NT) dst[e] = Y[e];
        for (int e = t; e < NN; e += NT) { gE[e] = E[e]; gD[e] = D[e]; }
    }
    if (t < GNG_NCNT) cnt[t] = sh[t];
}

}  // namespace fz
