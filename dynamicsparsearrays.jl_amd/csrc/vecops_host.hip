// csrc/vecops_host.hip — DynamicSparseVector as a device operand, host side, and its eight entry points: the stored pairs read into
// HBM (dsa_vec_nonzeros_dev), a vector built from pairs in HBM (dsa_vec_create_dev), mat * v with a dynamic vector on both sides
// (dsa_mat_mul_vec), alpha * a + beta * b as a dynamic vector (dsa_vec_axpby_vec), the whole-vector reductions (dsa_vec_reduce), the
// sparse . sparse and sparse . dense dot (dsa_vec_dot, dsa_vec_dot_dense_dev) and densify (dsa_vec_to_dense_dev).  Host-only unit:
// the kernels are in vecops.hip; the pack, the merge, the sparse-x product and the builder are the ones the host forms use
// (vec_pack_alt, launch_merge_axpby, spx_enqueue, pma_build_dev).  Nothing of an operand or a result crosses PCIe except counts, one
// key (the first packed key of x, when the gather strategy of the product has to know that it can address it) and scalars.
//
// Every call starts from the PACKED cells of its vector operands (vec_pack_alt: the alternate slot buffer, ascending keys in their
// physical width).  A kernel that reads the alternate buffer of a vector runs on that vector's own stream — except the second
// operand of a dot or a merge, which is read on the first one's stream after wait_for_pack; those calls end with a host wait that
// covers the read — so a vector's next write, which reuses the buffer, is always ordered behind its readers.
// Read-only for the operands: no epoch moves, a cached SpMV plan of the matrix survives.
#include "host.h"
#include "vecops.h"

#include <algorithm>
#include <cstring>

using namespace dsa;
using namespace dsa::host;

namespace {

// queued writes applied, then the packed cells at the front of the alternate buffer; returns their number
int64_t packed(dsa_vec* h) {
    vec_flush(h);
    if (h->P.h_ctl->nb_elements == 0) return 0;
    const int64_t n = vec_pack_alt(h);
    if (n != h->P.h_ctl->nb_elements) fail(DSA_EASSERT, "stored-cell count differs from nb_elements");
    return n;
}
KeyArr packed_keys(const Pma& P) { return P.KA(1 - P.cur); }
const double* packed_vals(const Pma& P) { return P.vals[1 - P.cur]; }

// what `consumer` enqueues from here on runs behind everything enqueued on P's stream so far (on the device: no host wait)
void order_behind(Pma& P, hipStream_t consumer) {
    if (consumer == P.stream) return;
    if (P.ev_handoff == nullptr) HIPCHK(hipEventCreateWithFlags(&P.ev_handoff, hipEventDisableTiming));
    HIPCHK(hipEventRecord(P.ev_handoff, P.stream));
    HIPCHK(hipStreamWaitEvent(consumer, P.ev_handoff, 0));
}

// one two-stage reduction over the na packed cells of `drv` (na > 0), on its stream; the scalar and the error word come back in one
// hand-over
struct Reduced { double value; unsigned long long err; };
Reduced reduce_packed(dsa_vec* drv, int32_t term, int64_t na, KeyArr kb, const double* vb, int64_t nb, const double* xd, int64_t nx,
                      const char* what) {
    Pma& P = drv->P;
    ExportArea& A = P.vo;
    A.ensure(P.stream, vo_scratch_bytes(na), VO_PIN_WORDS);
    const unsigned long long seq = A.next();
    LAUNCH("vector reduce", launch_vec_reduce(term, packed_keys(P), packed_vals(P), na, kb, vb, nb, xd, nx, A.scratch, A.pin, seq, P.stream));
    wait_handover(P, A.pin + VO_PIN_SEQ, seq, what);
    Reduced r;
    const unsigned long long bits = A.pin[VO_PIN_RESULT];
    std::memcpy(&r.value, &bits, sizeof(double));
    r.err = A.pin[VO_PIN_ERR];
    return r;
}

// a new vector of length `len` from n (key, value) pairs that are complete in HBM, folded by `combine`: dsa_vec_create from the
// upload on (`range`: bounds of the keys, unknown = the builder scans them; it also fixes the physical key width)
dsa_vec* vec_from_pairs_dev(const int64_t* d_keys, const double* d_vals, int64_t n, int32_t combine, int64_t len, KeyRange range) {
    auto* v = new dsa_vec();
    try {
        pma_init_common(v->P, false, false);
        pma_build_dev(v->P, nullptr, d_keys, d_vals, n, combine, 1, 0, needs_wide(range), KeyRange(), range);
    } catch (...) { pma_destroy(v->P); delete v; throw; }
    v->n = len;
    return v;
}

}  // namespace

extern "C" {

int32_t dsa_vec_nonzeros_dev(dsa_vec_t* h, int64_t* d_keys, double* d_vals, int64_t cap, int64_t* n_out) {
    API_TRY
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    *n_out = 0;
    const int64_t n = packed(h);
    *n_out = n;
    if (n > cap) fail(DSA_ECAP, "output buffers too small");
    if (n == 0) return DSA_OK;
    if (!d_keys || !d_vals) fail(DSA_EARG, "output is NULL");
    Pma& P = h->P;
    LAUNCH("vector copy-out", launch_vec_copy_out(packed_keys(P), packed_vals(P), n, d_keys, d_vals, nullptr, 0ull, P.stream));
    API_CATCH
}

int32_t dsa_vec_create_dev(const int64_t* d_keys, const double* d_vals, int64_t n, int32_t combine_op, int64_t len, dsa_vec_t** out) {
    API_TRY
    if (n < 0) fail(DSA_EARG, "negative length");
    if (n > 0xffffffffll) fail(DSA_EARG, "more than 2^32-1 entries in one call");
    if (n > 0 && (!d_keys || !d_vals)) fail(DSA_EARG, "NULL array of a non-empty vector");
    HIPCHK(hipSetDevice(g_device));
    KeyRange keys, again;
    bool z0 = false, z1 = false;
    // the key range fixes the physical key width and the guessed length (one min / max pass on the device; the host never sees a key)
    if (n > 0) launch_check(device_key_scan(d_keys, d_keys, n, &keys, &again, &z0, &z1, nullptr), "key scan: ");
    if (len < 0) len = keys.known() ? std::max<int64_t>(0, keys.hi) : 0;      // _guess_length  src/vector.jl:6
    *out = vec_from_pairs_dev(d_keys, d_vals, n, combine_op, len, keys);
    API_CATCH
}

int32_t dsa_mat_mul_vec(dsa_mat_t* h, int32_t transpose, dsa_vec_t* x, dsa_vec_t** out) {
    API_TRY
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    const int64_t ny = transpose ? h->n : h->m;
    const int64_t ncols = transpose ? h->m : h->n;
    const int64_t nx = packed(x);
    dsa_mat::Spx& sx = h->spx;
    int64_t cnt = 0;
    Pma* walked = nullptr;
    if (ny > 0 && nx > 0) {
        Pma& X = x->P;
        auto side = [&](bool xdriven) -> Pma& { return xdriven ? (transpose ? h->row : h->col) : (transpose ? h->col : h->row); };
        bool xdriven = spx_xdriven(nx, ncols);
        Pma& ruled = side(xdriven);
        if (sx.res_stream) HIPCHK(hipStreamSynchronize(sx.res_stream));      // the last product has let go of dx, oi and ov
        spx_ensure(h, ny, nx, ruled.stream);
        // x as int64 keys | values in the handle's scratch, copied on x's OWN stream right behind the pack.  The gather strategy
        // cannot address a key below 1 (the host knows only length(x)): when the rule chooses it, the first packed key — the smallest
        // — comes back and the x-driven kernel takes over if need be, as dsa_mat_spmv_sparse decides from the caller's array.
        int64_t* d_xi = sx.dx;
        double* d_xv = reinterpret_cast<double*>(sx.dx + nx);
        ExportArea& A = X.vo;
        A.ensure(X.stream, vo_scratch_bytes(0), VO_PIN_WORDS);
        const unsigned long long seq0 = A.next();
        LAUNCH("vector copy-out", launch_vec_copy_out(packed_keys(X), packed_vals(X), nx, d_xi, d_xv, xdriven ? nullptr : A.pin, seq0, X.stream));
        if (!xdriven) {
            wait_handover(X, A.pin + VO_PIN_SEQ, seq0, "mul_vec (first key)");
            if ((int64_t)A.pin[VO_PIN_FIRST] < 1) {
                xdriven = true;
                HIPCHK(hipStreamSynchronize(ruled.stream));      // (spx_ensure may have zeroed fresh scratch there: the product now runs on the twin's stream)
            }
        }
        Pma& P = side(xdriven);
        walked = &P;
        order_behind(X, P.stream);
        sx.res_count = -1; sx.dl_started = false;
        const unsigned long long seq = ++sx.seq;
        __atomic_thread_fence(__ATOMIC_RELEASE);
        sx.res_stream = spx_enqueue(h, transpose, xdriven, d_xi, d_xv, nx, ny, ncols, sx.oi, sx.ov, sx.out_cap, sx.d_count, sx.pin, seq, 0);
        wait_handover(P, sx.pin + 1, seq, "mul_vec");      // the count; also: x's packed cells and the scratch copy have been read
        cnt = sx.pin[0];
        if (cnt < 0 || cnt > ny || cnt > sx.out_cap) fail(DSA_EASSERT, "mul_vec: the product reports an impossible number of touched rows");
    }
    // dynamicsparsevec(rows, values, +, size(mat, 1 | 2)) of the touched rows (ascending, distinct, in 1..ny), on the new vector's stream
    // behind the emit; the build ends with a wait for that stream, so oi / ov are free for the next product on return
    KeyRange rows;
    if (cnt > 0) { rows.lo = 1; rows.hi = ny; }
    auto* v = new dsa_vec();
    try {
        pma_init_common(v->P, false, false);
        if (walked) order_behind(*walked, v->P.stream);
        pma_build_dev(v->P, nullptr, sx.oi, sx.ov, cnt, DSA_COMBINE_ADD, 1, 0, needs_wide(rows), KeyRange(), rows);
    } catch (...) { (void)hipStreamSynchronize(v->P.stream); pma_destroy(v->P); delete v; throw; }
    v->n = std::max<int64_t>(ny, 0);
    *out = v;
    API_CATCH
}

int32_t dsa_vec_axpby_vec(dsa_vec_t* a, double alpha, dsa_vec_t* b, double beta, dsa_vec_t** out) {
    API_TRY
    const int64_t na = packed(a);
    const int64_t nb = b != a ? packed(b) : na;
    const int64_t total = na + nb;
    const int64_t len = std::max(a->n, b->n);
    if (total == 0) { *out = vec_from_pairs_dev(nullptr, nullptr, 0, DSA_COMBINE_ADD, len, KeyRange()); return DSA_OK; }
    Pma &A = a->P, &B = b->P;
    if (b != a) wait_for_pack(b, a);
    // the merge and the compaction of dsa_vec_axpby (same kernels, same scratch layout), the compacted pairs handed to the builder
    const int64_t nwords = (total + 63) >> 6, ntiles = (nwords + 63) / 64;
    const size_t off_mv = (size_t)total * 8, off_ok = 2 * off_mv, off_ov = 3 * off_mv, off_keep = 4 * off_mv,
                 off_cnt = off_keep + (size_t)nwords * 8, off_off = off_cnt + (size_t)(ntiles + 8) * 4, bytes = off_off + (size_t)(ntiles + 8) * 4;
    DevStaging sc(A.stream);
    char* scratch = sc.alloc<char>(0, bytes);
    int64_t* mk = reinterpret_cast<int64_t*>(scratch);
    double* mv = reinterpret_cast<double*>(scratch + off_mv);
    int64_t* ok = reinterpret_cast<int64_t*>(scratch + off_ok);
    double* ov = reinterpret_cast<double*>(scratch + off_ov);
    uint64_t* keep = reinterpret_cast<uint64_t*>(scratch + off_keep);
    RebalanceWork work{reinterpret_cast<uint32_t*>(scratch + off_cnt), reinterpret_cast<uint32_t*>(scratch + off_off), ntiles + 8};
    HIPCHK(hipMemsetAsync(keep, 0, (size_t)nwords * 8, A.stream));
    LAUNCH("merge", launch_merge_axpby(packed_keys(A), packed_vals(A), na, alpha, packed_keys(B), packed_vals(B), nb, beta, mk, mv, keep, A.stream));
    int64_t cnt = pack_small(A, KeyArr{mk, 1, 0}, mv, keep, 1, total, KeyArr{ok, 1, 0}, ov, total);
    if (cnt < 0) {
        LAUNCH("compact", launch_compact_range(KeyArr{mk, 1, 0}, mv, keep, 1, total, KeyArr{ok, 1, 0}, ov, total, &work, &cnt, A.stream));
    }
    sc.sync();      // the compacted pairs are complete (and b's packed cells have been read) before another stream builds from them
    // the merged keys lie between the operands' keys, which the host does not know: the builder scans them (an unknown range)
    auto* v = new dsa_vec();
    try {
        pma_init_common(v->P, false, false);
        pma_build_dev(v->P, nullptr, ok, ov, cnt, DSA_COMBINE_ADD, 1, 0, A.wide || B.wide, KeyRange(), KeyRange());
    } catch (...) { (void)hipStreamSynchronize(v->P.stream); pma_destroy(v->P); delete v; throw; }
    v->n = len;
    *out = v;
    API_CATCH
}

int32_t dsa_vec_reduce(dsa_vec_t* h, int32_t kind, double* out) {
    API_TRY
    if (kind < DSA_RED_SUM || kind > DSA_RED_ABSMAX) fail(DSA_EARG, "kind must be DSA_RED_SUM, _ABSSUM, _SQSUM or _ABSMAX (the count is dsa_vec_nnz)");
    *out = 0.0;
    const int64_t n = packed(h);
    if (n == 0) return DSA_OK;
    *out = reduce_packed(h, kind, n, KeyArr{nullptr, 0, 0}, nullptr, 0, nullptr, 0, "vector reduce").value;
    API_CATCH
}

int32_t dsa_vec_dot(dsa_vec_t* a, dsa_vec_t* b, double* out) {
    API_TRY
    *out = 0.0;
    const int64_t na = packed(a);
    const int64_t nb = b != a ? packed(b) : na;
    if (na == 0 || nb == 0) return DSA_OK;
    // driven by the operand with fewer stored cells (ties: a); the other one is looked up, on the driving operand's stream
    dsa_vec* drv = nb < na ? b : a;
    dsa_vec* oth = nb < na ? a : b;
    if (oth != drv) wait_for_pack(oth, drv);
    *out = reduce_packed(drv, VO_DOT, std::min(na, nb), packed_keys(oth->P), packed_vals(oth->P), std::max(na, nb), nullptr, 0, "vector dot").value;
    API_CATCH
}

int32_t dsa_vec_dot_dense_dev(dsa_vec_t* h, const double* d_x, int64_t nx, double* out) {
    API_TRY
    if (nx < 0 || (nx > 0 && !d_x)) fail(DSA_EARG, "the dense operand is NULL or its length negative");
    *out = 0.0;
    const int64_t n = packed(h);
    if (n == 0) return DSA_OK;
    const Reduced r = reduce_packed(h, VO_DOT_DENSE, n, KeyArr{nullptr, 0, 0}, nullptr, 0, d_x, nx, "vector dot (dense)");
    if (r.err & 1u) fail(DSA_EBOUNDS, "a stored key lies outside 1..nx");
    *out = r.value;
    API_CATCH
}

int32_t dsa_vec_to_dense_dev(dsa_vec_t* h, double* d_x, int64_t nx) {
    API_TRY
    if (nx < 0 || (nx > 0 && !d_x)) fail(DSA_EARG, "the dense operand is NULL or its length negative");
    const int64_t n = packed(h);
    Pma& P = h->P;
    if (n > 0) {
        const Reduced r = reduce_packed(h, VO_BOUNDS, n, KeyArr{nullptr, 0, 0}, nullptr, 0, nullptr, nx, "vector densify (check)");
        if (r.err & 1u) fail(DSA_EBOUNDS, "a stored key lies outside 1..nx");      // before the first write
    }
    if (nx > 0) HIPCHK(hipMemsetAsync(d_x, 0, (size_t)nx * sizeof(double), P.stream));
    LAUNCH("vector scatter", launch_vec_scatter(packed_keys(P), packed_vals(P), n, d_x, nx, P.stream));
    API_CATCH
}

}  // extern "C"
