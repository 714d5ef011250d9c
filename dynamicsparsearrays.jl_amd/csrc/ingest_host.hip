// csrc/ingest_host.hip — dynamicsparse(I, J, V, m, n) from arrays that are already in HBM: the argument checks, the K-ingest launches
// (ingest.hip) on a stream of their own, the one wait for their verdict and key ranges, and the device builder behind them.  Host-only
// unit.  The caller's arrays are read by the ingest launches (waited for here) and by the builder, whose streams are synchronised
// before it returns and before it throws: nothing enqueued reads them once an entry point is back.
#include "host.h"
#include "ingest.h"

#include <climits>
#include <cstring>

namespace dsa {
namespace host {

namespace {

// device words, pinned landing area and stream of one import; everything goes back when it ends
struct Ingest {
    long long* d_acc = nullptr;
    unsigned long long* pin = nullptr;
    int64_t* d_keys = nullptr;            // 16 * nnz bytes of pooled scratch: the a keys, then the b keys
    hipStream_t stream = nullptr;
    int device = 0;
    bool enqueued = false;
    ~Ingest() {
        if (stream) {
            if (enqueued) (void)hipStreamSynchronize(stream);      // (an error path: a launch may still read the caller's arrays / write the scratch)
            stream_put(stream, device);
        }
        pool_free(d_keys); pool_free(d_acc); pinned_free(pin);
    }
    void open(int64_t key_words) {
        HIPCHK(hipSetDevice(g_device));
        device = g_device;
        HIPCHK(pool_alloc(reinterpret_cast<void**>(&d_acc), IN_WORDS * sizeof(long long)));
        HIPCHK(pinned_alloc(reinterpret_cast<void**>(&pin), IN_WORDS * sizeof(unsigned long long)));
        std::memset(pin, 0, IN_WORDS * sizeof(unsigned long long));
        if (key_words > 0) HIPCHK(pool_alloc(reinterpret_cast<void**>(&d_keys), (size_t)key_words * sizeof(int64_t)));
        HIPCHK(stream_get(&stream));
        enqueued = true;
        LAUNCH("ingest init", launch_in_init(d_acc, stream));
    }
    // the one wait: publishes behind everything enqueued so far and reads the five words
    void verdict(KeyRange& a, KeyRange& b, unsigned long long& flags) {
        LAUNCH("ingest publish", launch_in_publish(d_acc, pin, 1ull, stream));
        launch_check(wait_pinned_seq(pin + 5, 1ull, stream), "ingest: ");
        HIPCHK(hipStreamSynchronize(stream));
        enqueued = false;
        const long long* w = reinterpret_cast<const long long*>(pin);
        a = KeyRange(); b = KeyRange();
        if (w[1] >= w[0]) { a.lo = w[0]; a.hi = w[1]; }
        if (w[3] >= w[2]) { b.lo = w[2]; b.hi = w[3]; }
        flags = pin[4];
    }
};

void check_index_args(int32_t index_bits, int32_t index_base, int64_t nnz) {
    check_index_format(index_bits, index_base);
    if (nnz < 0) fail(DSA_EARG, "negative length");
    if (nnz > 0xffffffffll) fail(DSA_EARG, "more than 2^32-1 triples in one call");
    if (index_bits == 32 && nnz + index_base > INT32_MAX) fail(DSA_EARG, "nnz + base does not fit 32-bit indices");
}

dsa_mat* build_handle(const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, KeyRange rows, KeyRange cols) {
    auto* h = new dsa_mat();
    try { mat_build_from_dev(h, dI, dJ, dV, nnz, rows, cols); }
    catch (...) { mat_discard(h); throw; }
    return h;
}

}  // namespace

dsa_mat* mat_from_coo_dev(const void* d_I, const void* d_J, const double* d_V, int64_t nnz, int32_t index_bits, int32_t index_base,
                          int64_t m, int64_t n) {
    check_index_args(index_bits, index_base, nnz);
    if (index_bits == 32 && (m > INT32_MAX || n > INT32_MAX)) fail(DSA_EARG, "a dimension does not fit 32-bit indices");
    if (nnz > 0 && (d_I == nullptr || d_J == nullptr || d_V == nullptr)) fail(DSA_EARG, "NULL array of a non-empty matrix");
    const auto t0 = Clock::now();
    KeyRange rows, cols;
    const int64_t *dI = nullptr, *dJ = nullptr;
    Ingest in;
    if (nnz > 0) {
        // 64-bit, 1-based arrays ARE the keys: read in place, only folded
        const bool in_place = index_bits == 64 && index_base == 1;
        in.open(in_place ? 0 : 2 * nnz);
        int64_t* kI = in_place ? nullptr : in.d_keys;
        int64_t* kJ = in_place ? nullptr : in.d_keys + nnz;
        LAUNCH("ingest keys", launch_in_keys(d_I, d_J, index_bits, index_base, nnz, kI, kJ, in.d_acc, in.stream));
        unsigned long long flags = 0;
        in.verdict(rows, cols, flags);
        if (flags & (IN_ZERO_A | IN_ZERO_B)) fail(DSA_EKEY, "0 is the reserved semaphore key (src/pcsr.jl:23)");
        dI = in_place ? static_cast<const int64_t*>(d_I) : kI;
        dJ = in_place ? static_cast<const int64_t*>(d_J) : kJ;
    } else {
        HIPCHK(hipSetDevice(g_device));
    }
    const double t_keys = elapsed_ms(t0);
    const auto t1 = Clock::now();
    dsa_mat* h = build_handle(dI, dJ, d_V, nnz, rows, cols);
    if (dbg_time()) fprintf(stderr, "[ingest] coo nnz=%lld bits=%d base=%d: expand 0.00 ms  keys %.2f ms  build %.2f ms\n", (long long)nnz, index_bits, index_base,
                            t_keys, elapsed_ms(t1));
    h->m = m >= 0 ? m : (rows.known() ? std::max<int64_t>(0, rows.hi) : 0);        // _guess_length  src/vector.jl:6
    h->n = n >= 0 ? n : (cols.known() ? std::max<int64_t>(0, cols.hi) : 0);
    return h;
}

dsa_mat* mat_from_compressed_dev(int32_t orientation, int32_t index_bits, int32_t index_base, const void* d_ptr, const void* d_idx,
                                 const double* d_vals, int64_t outer, int64_t inner, int64_t nnz) {
    if (orientation != DSA_COLMAJOR && orientation != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    check_index_args(index_bits, index_base, nnz);
    if (outer < 0 || inner < 0) fail(DSA_EARG, "negative dimension");
    if (index_bits == 32 && (outer > INT32_MAX || inner > INT32_MAX)) fail(DSA_EARG, "a dimension does not fit 32-bit indices");
    if (d_ptr == nullptr) fail(DSA_EARG, "a compressed form needs its ptr array");
    if (nnz > 0 && (d_idx == nullptr || d_vals == nullptr)) fail(DSA_EARG, "NULL array of a non-empty matrix");
    const auto t0 = Clock::now();
    KeyRange ko, ki;
    Ingest in;
    in.open(2 * nnz);
    int64_t* k_outer = in.d_keys;
    int64_t* k_inner = nnz > 0 ? in.d_keys + nnz : nullptr;
    LAUNCH("ingest expand", launch_in_expand(d_ptr, index_bits, index_base, outer, nnz, k_outer, in.d_acc, in.stream));
    double t_expand = 0.0;
    if (dbg_time()) { HIPCHK(hipStreamSynchronize(in.stream)); t_expand = elapsed_ms(t0); }      // (the split of the timing line only)
    LAUNCH("ingest keys", launch_in_keys(nullptr, d_idx, index_bits, index_base, nnz, nullptr, k_inner, in.d_acc, in.stream));
    unsigned long long flags = 0;
    in.verdict(ko, ki, flags);
    if (flags & IN_BAD_PTR) fail(DSA_EARG, "malformed ptr: it must start at base, end at base + nnz and never decrease");
    if (nnz > 0 && (!ki.known() || ki.lo < 1 || ki.hi > inner)) fail(DSA_EBOUNDS, "an inner index lies outside base .. base + inner - 1");
    if (nnz == 0) { ko = KeyRange(); ki = KeyRange(); }
    const double t_keys = elapsed_ms(t0) - t_expand;
    const auto t1 = Clock::now();
    const bool csr = orientation == DSA_ROWMAJOR;
    dsa_mat* h = csr ? build_handle(k_outer, k_inner, d_vals, nnz, ko, ki) : build_handle(k_inner, k_outer, d_vals, nnz, ki, ko);
    if (dbg_time()) fprintf(stderr, "[ingest] %s nnz=%lld bits=%d base=%d: expand %.2f ms  keys %.2f ms  build %.2f ms\n", csr ? "csr" : "csc", (long long)nnz,
                            index_bits, index_base, t_expand, t_keys, elapsed_ms(t1));
    h->m = csr ? outer : inner;
    h->n = csr ? inner : outer;
    return h;
}

}  // namespace host
}  // namespace dsa
