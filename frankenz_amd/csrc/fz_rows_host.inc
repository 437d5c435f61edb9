// Host side of what the consumers of rows of ln-weights share (fz_rows.h; DESIGN.md, "Adding a row consumer"): the geometry rule, the
// entry checks, the two row bits of the error word, the staged rows / neighbors / nnbr and the chunk loop.
// Included by frankenz_hip.hip in front of fz_draw_host.inc.

namespace {
// The launch geometry of every row consumer, a function of the row length alone: one wave per object up to FZ_DRAW_WAVE_LMAX entries,
// a block of four waves beyond (FZ_DRAW_WPO = 1 / 4 forces one: tests).
struct RowGeometry {
    int wpo, opb;
    dim3 grid(int64_t n) const { return dim3((unsigned)((n + opb - 1) / opb)); }
    // the dynamic LDS of the segment-table kernels (fz_draw.h) for rows of L entries; `what` opens the refusal ("posterior draws")
    int seg_lds(const char* what, int64_t L, size_t* lds) const {
        const size_t nsegL = (size_t)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
        *lds = (FZ_DRAW_HDR + (size_t)opb * 2 * nsegL) * 8;
        if (*lds > FZ_LDS_BYTES) return fail(-5, "%s: rows of %lld entries need %zu bytes of LDS at this geometry", what, (long long)L, *lds);
        return 0;
    }
};
RowGeometry row_geometry(int64_t L) {
    int wpo = L <= FZ_DRAW_WAVE_LMAX ? 1 : 4;
    const long long forced = fz_dbg_int("FZ_DRAW_WPO", 0);
    if (forced == 1 || forced == 4) wpo = (int)forced;
    return {wpo, 4 / wpo};
}

// ---- the entry checks ----
int rows_together(const char* who, const int64_t* neighbors, const int64_t* nnbr) {
    if ((neighbors == nullptr) != (nnbr == nullptr)) return fail(-1, "%s: neighbors and nnbr come together", who);
    return 0;
}
int mw_limits(const char* who, int64_t W, int64_t M, bool dense) {
    if (W < 1 || M < 1) return fail(-4, "%s: rows of %lld entries over %lld models", who, (long long)W, (long long)M);
    if (W > FZ_DRAW_LMAX) return fail(-5, "%s: rows of %lld entries exceed FZ_DRAW_LMAX = %d", who, (long long)W, FZ_DRAW_LMAX);
    if (M >= ((int64_t)1 << 31)) return fail(-5, "%s: %lld models, the limit is M < 2^31 (FZ_MW_MMAX)", who, (long long)M);
    if (dense && W != M) return fail(-4, "%s: dense rows (no neighbors) have one entry per model: W = %lld, M = %lld", who, (long long)W, (long long)M);
    return 0;
}
int rows_entry(const char* who, const int64_t* neighbors, const int64_t* nnbr, int64_t N, int64_t W, int64_t M) {
    FZCHK(rows_together(who, neighbors, nnbr));
    FZCHK(mw_limits(who, W, M, neighbors == nullptr));
    if (N < 0) return fail(-4, "%s: %lld objects", who, (long long)N);
    return 0;
}

// ---- the error word of a call: d_mw[0], zeroed by mw_flags_begin, read once by mw_flags_read ----
int mw_flags_begin(fz_ctx* c, int** d_flags) {
    FZCHK(c->d_mw[0].ensure(64));
    HIPCHK(hipMemsetAsync(c->d_mw[0].p, 0, 64, c->stream));
    *d_flags = c->d_mw[0].as<int>();
    return 0;
}
int mw_flags_read(fz_ctx* c, int* ef) {
    *ef = 0;
    HIPCHK(hipGetLastError());
    return copy_out(c, ef, c->d_mw[0].p, sizeof(int));
}
// the two row bits, which every row kernel raises (fz_rows.h)
int row_flags_check(const char* who, int ef, int64_t W, int64_t M) {
    if (ef & FZ_MW_ERR_NNB) return fail(-3, "%s: Nneighbors outside [0, %lld]", who, (long long)W);
    if (ef & FZ_MW_ERR_NBR) return fail(-3, "%s: a neighbour index outside [0, %lld)", who, (long long)M);
    return 0;
}
int row_flags_check(fz_ctx* c, const char* who, int64_t W, int64_t M) {     // ... of a call that raises no other bit
    int ef;
    FZCHK(mw_flags_read(c, &ef));
    return row_flags_check(who, ef, W, M);
}

// ---- the staged triple and the chunk loop ----
// rows (N, W) / neighbors (N, W) / nnbr (N) over the buffers the site names; after for_row_chunks' at(): the chunk's device views
struct RowsIn {
    StageRows rv, nv, cv;
    RowsIn(fz_ctx* c, const double* rows, const int64_t* neighbors, const int64_t* nnbr, int64_t W, DevBuf& br, DevBuf& bn, DevBuf& bc)
        : rv(c, rows, (size_t)W * 8, br, STAGE_IN), nv(c, neighbors, (size_t)W * 8, bn, STAGE_IN), cv(c, nnbr, 8, bc, STAGE_IN) {}
    const double* rows() const { return rv.as<const double>(); }
    const int64_t* nbr() const { return nv.as<const int64_t>(); }
    const int64_t* nnb() const { return cv.as<const int64_t>(); }
};
// Objects [0, N) in chunks under the workspace limit: the bytes per object are those of the stages a host caller's rows go through
// and of the per-object scratch a site names (a NULL argument with `scratch`); none: one chunk.  Per chunk every stage's view is
// formed (StageRows::as), body(i0, n) runs and the staged outputs go back.
template <class Body>
int for_row_chunks(fz_ctx* c, int64_t N, RowsIn& in, std::initializer_list<StageRows*> more, Body&& body) {
    std::vector<StageRows*> stages{&in.rv, &in.nv, &in.cv};
    stages.insert(stages.end(), more.begin(), more.end());
    int64_t per_obj = 0;
    for (const StageRows* s : stages) if (s->staged() || (s->scratch && !s->dev)) per_obj += (int64_t)s->row;
    int64_t nc = per_obj ? std::min<int64_t>(std::max<int64_t>(1, c->ws_limit / per_obj), 1 << 18) : N;
    nc = std::max<int64_t>(1, std::min(nc, N));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        for (StageRows* s : stages) FZCHK(s->at(i0, n, &s->cur));
        FZCHK(body(i0, n));
        for (const StageRows* s : stages) FZCHK(s->back(i0, n));
    }
    return 0;
}
}  // namespace
