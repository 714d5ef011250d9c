// csrc/combine_host.hip — host side of dsa_mat_combine: alpha * A + beta * shift(B) as a new matrix (copy, A + B, hcat, vcat, blockdiag
// are all this one primitive).  Argument checks, one K-combine pass (combine.hip) per operand on the operand's own colmajor stream into
// one pooled buffer of triples, one wait per operand for its error word and key ranges, the checks that need those, then the device
// builder (matwrite_host.hip: mat_build_from_dev) on the concatenation.  Host-only unit.  The operands are only read: no epoch moves,
// a cached SpMV plan survives; what stays on an operand is the scratch and the pinned words of its orientation (Pma::cmb).
#include "host.h"
#include "combine.h"

#include <algorithm>
#include <climits>

namespace dsa {
namespace host {

namespace {

// the pooled triples, and the operand streams a pass was enqueued on: drained before the buffer goes back, also on an error
struct Triples {
    void* p = nullptr;
    hipStream_t streams[2] = {nullptr, nullptr};
    Triples() = default;
    Triples(const Triples&) = delete;
    ~Triples() {
        for (hipStream_t s : streams) if (s) (void)hipStreamSynchronize(s);
        pool_free(p);
    }
};

// one operand's pass: role 0 = a, 1 = b (the pinned words of the two roles are apart, so that A + A can wait for both)
struct Pass {
    dsa_mat* h = nullptr;
    double scale = 1.0;
    int64_t row_off = 0, col_off = 0, nnz = 0, at = 0;
    unsigned long long* pin = nullptr; unsigned long long seq = 0;
    KeyRange rows, cols;                 // of the stored cells, before the shift
};

int64_t mat_nnz(const dsa_mat* h) { return h->col.h_ctl->nb_elements - h->col.h_ctl->nb_partitions; }

void enqueue(Pass& p, int role, int64_t* I, int64_t* J, double* V, Triples& buf) {
    if (p.nnz == 0) return;
    Pma& P = p.h->col;
    ExportArea& A = P.cmb;
    A.ensure(P.stream, combine_scratch_bytes(P.capacity()), 2 * CB_WORDS);
    p.seq = A.next();
    p.pin = A.pin + role * CB_WORDS;
    buf.streams[role] = P.stream;
    LAUNCH("combine", launch_combine(P.view(), P.h_ctl->nb_partitions, p.nnz, I + p.at, J + p.at, V + p.at, p.scale, p.row_off, p.col_off,
                                     A.scratch, p.pin, p.seq, P.stream));
}

// the wait for a pass and what its words say; the stream is drained, so that the builder's streams may read the triples
unsigned long long collect(Pass& p) {
    if (p.nnz == 0) return 0;
    Pma& P = p.h->col;
    wait_handover(P, p.pin + CB_WORDS - 1, p.seq, "combine");
    HIPCHK(hipStreamSynchronize(P.stream));
    cb_range(p.pin[1], p.pin[2], &p.rows.lo, &p.rows.hi);
    cb_range(p.pin[3], p.pin[4], &p.cols.lo, &p.cols.hi);
    return __atomic_load_n(p.pin, __ATOMIC_ACQUIRE);
}

// a shifted block must not land on the other operand's cells: every stored key of the shifted dimension inside 1 .. dim
void check_inside(const KeyRange& r, int64_t dim, const char* what) {
    if (r.known() && (r.lo < 1 || r.hi > dim)) fail(DSA_EBOUNDS, what);
}

KeyRange shift_range(const KeyRange& r, int64_t off) {
    if (!r.known()) return r;
    KeyRange s;
    if (__builtin_add_overflow(r.lo, off, &s.lo) || __builtin_add_overflow(r.hi, off, &s.hi))
        fail(DSA_EARG, "an offset moves a stored key out of the int64 range");
    return s;
}

KeyRange join(const KeyRange& x, const KeyRange& y) {
    if (!x.known()) return y;
    if (!y.known()) return x;
    KeyRange r; r.lo = std::min(x.lo, y.lo); r.hi = std::max(x.hi, y.hi);
    return r;
}

int64_t shifted_dim(int64_t dim, int64_t off) {
    int64_t r;
    if (__builtin_add_overflow(dim, off, &r)) fail(DSA_EARG, "an offset moves the size of the second operand out of the int64 range");
    return r;
}

}  // namespace

dsa_mat* mat_combine(dsa_mat* a, double alpha, dsa_mat* b, double beta, int64_t row_off, int64_t col_off, int64_t m, int64_t n) {
    if (!a) fail(DSA_EARG, "the first operand is NULL");
    if (!b) { row_off = 0; col_off = 0; }
    for (dsa_mat* h : {a, b})
        if (h && (h->fillmode || !h->has_major)) fail(DSA_EMODE, "an operand is in fill mode");
    mat_flush(a);
    if (b && b != a) mat_flush(b);
    bind_device(a->col);
    Pass pa, pb;
    pa.h = a; pa.scale = alpha; pa.nnz = mat_nnz(a);
    if (b) { pb.h = b; pb.scale = beta; pb.row_off = row_off; pb.col_off = col_off; pb.nnz = mat_nnz(b); pb.at = pa.nnz; }
    const int64_t total = pa.nnz + pb.nnz;
    if (total > 0xffffffffll) fail(DSA_EARG, "more than 2^32-1 stored entries in the two operands");
    if (m < 0) m = b ? std::max(a->m, shifted_dim(b->m, row_off)) : a->m;
    if (n < 0) n = b ? std::max(a->n, shifted_dim(b->n, col_off)) : a->n;

    Triples buf;
    int64_t *I = nullptr, *J = nullptr; double* V = nullptr;
    if (total > 0) {
        HIPCHK(pool_alloc(&buf.p, (size_t)total * 24));
        I = static_cast<int64_t*>(buf.p); J = I + total; V = reinterpret_cast<double*>(J + total);
    }
    const auto t0 = Clock::now();
    enqueue(pa, 0, I, J, V, buf);
    enqueue(pb, 1, I, J, V, buf);
    const unsigned long long ea = collect(pa), eb = collect(pb);
    if ((ea | eb) & CB_ASSERT) fail(DSA_EASSERT, "combine: slot array and partition tables disagree");
    if (col_off != 0) {
        check_inside(pa.cols, a->n, "a stored entry of the first operand lies outside its columns 1 .. n: a column offset needs both operands inside their size");
        check_inside(pb.cols, b->n, "a stored entry of the second operand lies outside its columns 1 .. n: a column offset needs both operands inside their size");
    }
    if (row_off != 0) {
        check_inside(pa.rows, a->m, "a stored entry of the first operand lies outside its rows 1 .. m: a row offset needs both operands inside their size");
        check_inside(pb.rows, b->m, "a stored entry of the second operand lies outside its rows 1 .. m: a row offset needs both operands inside their size");
    }
    const KeyRange rows = join(pa.rows, shift_range(pb.rows, row_off)), cols = join(pa.cols, shift_range(pb.cols, col_off));
    if ((ea | eb) & CB_ZERO_KEY) fail(DSA_EKEY, "an offset moves a stored key to 0, the reserved semaphore key (src/pcsr.jl:23)");
    const double t_pass = elapsed_ms(t0);
    const auto t1 = Clock::now();
    auto* h = new dsa_mat();
    try { mat_build_from_dev(h, I, J, V, total, rows, cols); }
    catch (...) { mat_discard(h); throw; }
    if (dbg_time()) fprintf(stderr, "[combine] nnz=%lld + %lld: passes %.2f ms  build %.2f ms\n", (long long)pa.nnz, (long long)pb.nnz, t_pass, elapsed_ms(t1));
    h->m = m; h->n = n;
    return h;
}

}  // namespace host
}  // namespace dsa
