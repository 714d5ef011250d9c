// csrc/mutate_host.hip — the entry points that change a matrix in place from whole operand arrays: scale, the batched delete, droptol,
// update_values, insert_batch and assemble, each with operands in HBM (dsa_mat_X_dev) or in host memory (dsa_mat_X).  Every one is the same
// protocol around the two steps of its engine unit (scale_host.hip, delbatch_host.hip, droptol_host.hip, update_host.hip,
// insert_host.hip, assemble_host.hip): X_prepare — flush, checks and the passes that decide what changes, every error and every call that changes
// nothing with layouts and cached SpMV plans as they were — then mat_commit around X_apply.  One body per mutator (mat_X) serves both
// forms; the host form is stage, mat_X, copy back, sync.
#include "host.h"

using namespace dsa;
using namespace dsa::host;

namespace {

// The content epoch moves, and both cached SpMV plans go, in front of the first write; the SpMV meta is prefetched behind the last
// one, except for update_values (prefetch = false): it moves no cell, and the prefetch launches a kernel when no meta was computed yet.
template <typename Writes>
void mat_commit(dsa_mat* h, bool prefetch, Writes writes) {
    mat_content_changed(h);
    writes();
    if (prefetch) mat_prefetch_spmv_meta(h);
}

// Operands from host memory that the streams of both orientations read: uploaded on the colmajor stream, which is drained before the
// rowmajor stream may read them (the stage functions below).  At destruction the rowmajor stream may still read them (also after an
// error behind a launch): it is drained here, the colmajor one by DevStaging.
struct MatStaging : DevStaging {
    dsa_mat* h;
    explicit MatStaging(dsa_mat* h_) : DevStaging(h_->col.stream), h(h_) {}
    ~MatStaging() { if (h->has_major) (void)hipStreamSynchronize(h->row.stream); }
    void sync_both() { sync(); HIPCHK(hipStreamSynchronize(h->row.stream)); }
};

// n > 0 triples into blocks 0..2, and a byte mask of n bytes as block 3 if one is wanted
void stage_triples(MatStaging& st, const int64_t* I, const int64_t* J, const double* V, int64_t n, bool want_mask) {
    const void* src[3] = {I, J, V};
    for (int q = 0; q < 3; ++q) st.upload(q, src[q], (size_t)n * 8);
    if (want_mask) st.alloc(3, (size_t)n);
    st.sync();
}

// a factor pair into blocks 0 and 1.  A factor of length 0 is handed on as a non-NULL pointer that is never read: "given" and
// "absent" stay apart
struct Factors { const double* r; const double* c; };
Factors stage_factors(MatStaging& st, const double* r, int64_t nr, const double* c, int64_t nc) {
    auto one = [&](int q, const double* f, int64_t n) { return f && n > 0 ? st.upload<const double>(q, f, (size_t)n * sizeof(double)) : f; };
    const Factors d{one(0, r, nr), one(1, c, nc)};
    st.sync();
    return d;
}

// ---- the in-place scaling D_r A D_c (scale.hip): values only
void mat_scale(dsa_mat* h, double alpha, const double* d_r, int64_t nr, const double* d_c, int64_t nc) {
    scale_prepare(h, d_r, nr, d_c, nc);
    mat_commit(h, true, [&] { scale_apply(h, alpha, d_r, d_c); });
}

// ---- batched delete (delbatch.hip): every column (row) of a key list leaves both orientations in one device pass
void mat_delete_batch(dsa_mat* h, int32_t orientation, const int64_t* d_keys, int64_t n, int64_t* removed_out) {
    const int64_t cells = delete_batch_prepare(h, orientation, d_keys, n);
    if (cells < 0) return;
    mat_commit(h, true, [&] { delete_batch_apply(h, orientation, n, cells); });      // (returns with both streams drained)
    if (removed_out) *removed_out = cells;
}

// ---- dropzeros! / droptol! (droptol.hip): every small cell leaves both orientations in place; a call that drops nothing and the
// count-only call change nothing
void mat_droptol(dsa_mat* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc, int32_t count_only,
                 int64_t* dropped_out) {
    const int64_t count = droptol_prepare(h, tol, d_rtol, nr, d_ctol, nc);
    if (count > 0 && !count_only) mat_commit(h, true, [&] { droptol_apply(h, count); });
    if (dropped_out) *dropped_out = count;
}

// ---- update of stored values in place (update.hip): a call without a winning write changes nothing
void mat_update_values(dsa_mat* h, int32_t op, int32_t flags, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n,
                       uint8_t* d_missing, int64_t* updated_out, int64_t* missing_out) {
    const UpdateCounts c = update_prepare(h, op, flags, d_I, d_J, d_V, n, d_missing);
    if (c.updated > 0) mat_commit(h, false, [&] { update_apply(h, op, d_V, n); });
    if (updated_out) *updated_out = c.updated;
    if (missing_out) *missing_out = c.missing;
}

// ---- insert of cells that are not stored yet (insert.hip): a call that inserts nothing changes nothing
void mat_insert_batch(dsa_mat* h, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int32_t flags, uint8_t* d_existing) {
    const InsertCounts c = insert_prepare(h, d_I, d_J, d_V, n, flags, d_existing);
    if (c.ops > 0) mat_commit(h, true, [&] { insert_apply(h, c, d_V, n); });
}

// ---- the general write (assemble.hip): any triples folded to distinct cells, the stored ones updated, the others inserted, under one
// commit.  The SpMV meta is prefetched only when a cell is created: a call that only updates moves no cell
void mat_assemble(dsa_mat* h, int32_t op, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int64_t* distinct_out,
                  int64_t* updated_out, int64_t* inserted_out) {
    const AssembleCounts c = assemble_prepare(h, op, d_I, d_J, d_V, n);
    if (c.updated > 0 || c.missing > 0) mat_commit(h, c.missing > 0, [&] { assemble_apply(h, op, c); });
    if (distinct_out) *distinct_out = c.distinct;
    if (updated_out) *updated_out = c.updated;
    if (inserted_out) *inserted_out = c.missing;
}

}  // namespace

extern "C" {

int32_t dsa_mat_scale_dev(dsa_mat_t* h, double alpha, const double* d_r, int64_t nr, const double* d_c, int64_t nc) {
    API_TRY
    mat_scale(h, alpha, d_r, nr, d_c, nc);
    API_CATCH
}
int32_t dsa_mat_scale(dsa_mat_t* h, double alpha, const double* r, int64_t nr, const double* c, int64_t nc) {
    API_TRY
    mat_flush(h);
    scale_check_args(h, r, nr, c, nc);
    MatStaging st(h);
    const Factors f = stage_factors(st, r, nr, c, nc);
    mat_scale(h, alpha, f.r, nr, f.c, nc);
    st.sync_both();
    API_CATCH
}

int32_t dsa_mat_delete_batch_dev(dsa_mat_t* h, int32_t orientation, const int64_t* d_keys, int64_t n, int64_t* removed_out) {
    API_TRY
    if (removed_out) *removed_out = 0;
    mat_delete_batch(h, orientation, d_keys, n, removed_out);
    API_CATCH
}
int32_t dsa_mat_delete_batch(dsa_mat_t* h, int32_t orientation, const int64_t* keys, int64_t n, int64_t* removed_out) {
    API_TRY
    if (removed_out) *removed_out = 0;
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot delete columns or rows in fill mode");      // (no stream to stage on)
    // every other check is delete_batch_prepare's: a list that is NULL stays NULL, an orientation that is neither is staged for nothing
    DevStaging b((orientation == DSA_ROWMAJOR ? h->row : h->col).stream);      // drains the own stream before the keys go back to the pool
    mat_delete_batch(h, orientation, n > 0 && keys ? b.upload<const int64_t>(0, keys, (size_t)n * sizeof(int64_t)) : nullptr, n, removed_out);
    API_CATCH
}

int32_t dsa_mat_droptol_dev(dsa_mat_t* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc, int32_t count_only,
                            int64_t* dropped_out) {
    API_TRY
    if (dropped_out) *dropped_out = 0;
    mat_droptol(h, tol, d_rtol, nr, d_ctol, nc, count_only, dropped_out);
    API_CATCH
}
int32_t dsa_mat_droptol(dsa_mat_t* h, double tol, const double* rtol, int64_t nr, const double* ctol, int64_t nc, int32_t count_only,
                        int64_t* dropped_out) {
    API_TRY
    if (dropped_out) *dropped_out = 0;
    mat_flush(h);
    scale_check_args(h, rtol, nr, ctol, nc);
    MatStaging st(h);
    const Factors f = stage_factors(st, rtol, nr, ctol, nc);
    mat_droptol(h, tol, f.r, nr, f.c, nc, count_only, dropped_out);
    API_CATCH
}

int32_t dsa_mat_update_values_dev(dsa_mat_t* h, int32_t op, int32_t flags, const int64_t* d_I, const int64_t* d_J, const double* d_V,
                                  int64_t n, uint8_t* d_missing, int64_t* updated_out, int64_t* missing_out) {
    API_TRY
    if (updated_out) *updated_out = 0;
    if (missing_out) *missing_out = 0;
    mat_update_values(h, op, flags, d_I, d_J, d_V, n, d_missing, updated_out, missing_out);
    API_CATCH
}
int32_t dsa_mat_update_values(dsa_mat_t* h, int32_t op, int32_t flags, const int64_t* I, const int64_t* J, const double* V, int64_t n,
                              uint8_t* missing, int64_t* updated_out, int64_t* missing_out) {
    API_TRY
    if (updated_out) *updated_out = 0;
    if (missing_out) *missing_out = 0;
    mat_flush(h);
    update_check_args(h, op, flags, I, J, V, n);
    MatStaging st(h);
    if (n > 0) {
        stage_triples(st, I, J, V, n, missing != nullptr);
        mat_update_values(h, op, flags, st.at<int64_t>(0), st.at<int64_t>(1), st.at<double>(2), n, st.at<uint8_t>(3), updated_out, missing_out);
        if (missing) st.down(missing, st.p[3], (size_t)n);
        st.sync_both();
    }
    API_CATCH
}

int32_t dsa_mat_insert_batch_dev(dsa_mat_t* h, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int32_t flags,
                                 uint8_t* d_existing) {
    API_TRY
    mat_insert_batch(h, d_I, d_J, d_V, n, flags, d_existing);
    if (n > 0 && h->has_major) { HIPCHK(hipStreamSynchronize(h->col.stream)); HIPCHK(hipStreamSynchronize(h->row.stream)); }
    API_CATCH
}
int32_t dsa_mat_insert_batch(dsa_mat_t* h, const int64_t* I, const int64_t* J, const double* V, int64_t n, int32_t flags, uint8_t* existing) {
    API_TRY
    mat_flush(h);
    insert_check_args(h, I, J, V, n, flags);
    MatStaging st(h);
    if (n > 0) {
        stage_triples(st, I, J, V, n, existing != nullptr);
        mat_insert_batch(h, st.at<int64_t>(0), st.at<int64_t>(1), st.at<double>(2), n, flags, st.at<uint8_t>(3));
        if (existing) st.down(existing, st.p[3], (size_t)n);
        st.sync_both();
    }
    API_CATCH
}

int32_t dsa_mat_assemble_dev(dsa_mat_t* h, int32_t op, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n,
                             int64_t* distinct_out, int64_t* updated_out, int64_t* inserted_out) {
    API_TRY
    for (int64_t* out : {distinct_out, updated_out, inserted_out}) if (out) *out = 0;
    mat_assemble(h, op, d_I, d_J, d_V, n, distinct_out, updated_out, inserted_out);
    API_CATCH
}
int32_t dsa_mat_assemble(dsa_mat_t* h, int32_t op, const int64_t* I, const int64_t* J, const double* V, int64_t n, int64_t* distinct_out,
                         int64_t* updated_out, int64_t* inserted_out) {
    API_TRY
    for (int64_t* out : {distinct_out, updated_out, inserted_out}) if (out) *out = 0;
    mat_flush(h);
    assemble_check_args(h, op, I, J, V, n);
    MatStaging st(h);
    if (n > 0) {
        stage_triples(st, I, J, V, n, false);
        mat_assemble(h, op, st.at<int64_t>(0), st.at<int64_t>(1), st.at<double>(2), n, distinct_out, updated_out, inserted_out);
        st.sync_both();
    }
    API_CATCH
}

}  // extern "C"
