// csrc/fill_host.hip — the fill-mode write buffer of a matrix (FillBuffer in host.h; src/buffer.jl): the rows-already-written set,
// the pinned staging chunks and their cache, the asynchronous upload of staged triples piece by piece, and the drain in front of
// closefillmode!'s build.  Host-only unit: the running key ranges are folded on the device by build.hip (launch_key_scan_acc).
#include "host.h"

#include <algorithm>
#include <cstring>
#include <mutex>

namespace dsa {
namespace host {

bool fill_row_test_and_set(FillBuffer& b, int64_t row) {
    if (row >= 1 && row < ((int64_t)1 << 28)) {
        const size_t w = (size_t)(row >> 6);
        if (w >= b.row_bits.size()) b.row_bits.resize(std::max<size_t>(2 * b.row_bits.size(), w + 1024), 0ull);
        const uint64_t bit = 1ull << (row & 63);
        const bool was = (b.row_bits[w] & bit) != 0;
        b.row_bits[w] |= bit;
        return was;
    }
    return !b.rows_far.insert(row).second;
}

namespace {
// pinned staging chunks are expensive to allocate and free (milliseconds each): one set is kept for the next fill-mode matrix
struct FillStagingCache { std::mutex mu; int64_t* hI[2] = {nullptr, nullptr}; int64_t* hJ[2] = {nullptr, nullptr}; double* hV[2] = {nullptr, nullptr}; int device = -1; };
FillStagingCache g_fill_cache;
}  // namespace

void fill_release(FillBuffer& b) {
    if (b.stream) hipStreamSynchronize(b.stream);
    {
        std::lock_guard<std::mutex> lk(g_fill_cache.mu);
        if (b.hI[0] && g_fill_cache.hI[0] == nullptr) {
            for (int k = 0; k < 2; ++k) { g_fill_cache.hI[k] = b.hI[k]; g_fill_cache.hJ[k] = b.hJ[k]; g_fill_cache.hV[k] = b.hV[k]; b.hI[k] = nullptr; b.hJ[k] = nullptr; b.hV[k] = nullptr; }
            g_fill_cache.device = b.device;
        }
    }
    for (int k = 0; k < 2; ++k) {
        if (b.hI[k]) hipHostFree(b.hI[k]);
        if (b.hJ[k]) hipHostFree(b.hJ[k]);
        if (b.hV[k]) hipHostFree(b.hV[k]);
        if (b.uploaded[k]) hipEventDestroy(b.uploaded[k]);
    }
    pool_free(b.dI); pool_free(b.dJ); pool_free(b.dV);
    pool_free(b.d_acc); pinned_free(b.h_acc);
    if (b.stream) stream_put(b.stream, b.device);
    b = FillBuffer();
}

namespace {

// ---- device-resident fill buffer --------------------------------------------------------------------------------------
void fill_init(FillBuffer& b) {
    if (b.stream) return;
    HIPCHK(hipSetDevice(g_device));
    b.device = g_device;
    HIPCHK(stream_get(&b.stream));
    {
        std::lock_guard<std::mutex> lk(g_fill_cache.mu);
        if (g_fill_cache.hI[0] != nullptr && g_fill_cache.device == b.device)
            for (int k = 0; k < 2; ++k) { b.hI[k] = g_fill_cache.hI[k]; b.hJ[k] = g_fill_cache.hJ[k]; b.hV[k] = g_fill_cache.hV[k]; g_fill_cache.hI[k] = nullptr; g_fill_cache.hJ[k] = nullptr; g_fill_cache.hV[k] = nullptr; }
    }
    {
        void* p = nullptr;
        HIPCHK(pool_alloc(&p, 64)); b.d_acc = static_cast<long long*>(p);
        HIPCHK(pinned_alloc(&p, 64)); b.h_acc = static_cast<long long*>(p);
        b.h_acc[0] = INT64_MAX; b.h_acc[1] = INT64_MIN; b.h_acc[2] = INT64_MAX; b.h_acc[3] = INT64_MIN; b.h_acc[4] = 0;
        HIPCHK(hipMemcpyAsync(b.d_acc, b.h_acc, 5 * sizeof(long long), hipMemcpyHostToDevice, b.stream));
        HIPCHK(hipStreamSynchronize(b.stream));             // (h_acc is reused as the read-back target)
    }
    for (int k = 0; k < 2; ++k) {
        HIPCHK(hipEventCreateWithFlags(&b.uploaded[k], hipEventDisableTiming));
        if (b.hI[k]) continue;
        HIPCHK(hipHostMalloc(&b.hI[k], (size_t)FillBuffer::CHUNK * sizeof(int64_t), hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&b.hJ[k], (size_t)FillBuffer::CHUNK * sizeof(int64_t), hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&b.hV[k], (size_t)FillBuffer::CHUNK * sizeof(double), hipHostMallocDefault));
    }
}
// ships what is staged in the current pinned chunk and not yet sent (triples [b.sent, b.fill)) to HBM, asynchronously; a chunk that
// is full (or `finish`: the end of a batch) is closed — its event recorded — and the other chunk becomes current.  Pieces go up
// while the caller's memcpy fills the rest of the chunk, so that closefillmode! waits for one piece (6 MB), not for a chunk (24 MB).
void fill_upload_chunk(FillBuffer& b, bool finish = true) {
    if (b.fill == 0) return;
    HIPCHK(hipSetDevice(b.device));
    const int64_t npiece = b.fill - b.sent;
    if (npiece > 0) {
        if (b.dlen + npiece > b.dcap) {          // grow geometrically: new arrays, device-to-device copy of what is resident
            const int64_t ncap = std::max<int64_t>(2 * b.dcap, std::max<int64_t>(b.dlen + npiece, 4 * FillBuffer::CHUNK));
            int64_t *nI = nullptr, *nJ = nullptr; double* nV = nullptr;
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&nI), (size_t)ncap * sizeof(int64_t)));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&nJ), (size_t)ncap * sizeof(int64_t)));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&nV), (size_t)ncap * sizeof(double)));
            if (b.dlen > 0) {
                HIPCHK(hipMemcpyAsync(nI, b.dI, (size_t)b.dlen * sizeof(int64_t), hipMemcpyDeviceToDevice, b.stream));
                HIPCHK(hipMemcpyAsync(nJ, b.dJ, (size_t)b.dlen * sizeof(int64_t), hipMemcpyDeviceToDevice, b.stream));
                HIPCHK(hipMemcpyAsync(nV, b.dV, (size_t)b.dlen * sizeof(double), hipMemcpyDeviceToDevice, b.stream));
            }
            HIPCHK(hipStreamSynchronize(b.stream));       // earlier uploads into the old arrays have landed
            pool_free(b.dI); pool_free(b.dJ); pool_free(b.dV);
            b.dI = nI; b.dJ = nJ; b.dV = nV; b.dcap = ncap;
        }
        const int c = b.cur;
        HIPCHK(hipMemcpyAsync(b.dI + b.dlen, b.hI[c] + b.sent, (size_t)npiece * sizeof(int64_t), hipMemcpyHostToDevice, b.stream));
        HIPCHK(hipMemcpyAsync(b.dJ + b.dlen, b.hJ[c] + b.sent, (size_t)npiece * sizeof(int64_t), hipMemcpyHostToDevice, b.stream));
        HIPCHK(hipMemcpyAsync(b.dV + b.dlen, b.hV[c] + b.sent, (size_t)npiece * sizeof(double), hipMemcpyHostToDevice, b.stream));
        // the value ranges of the piece, folded into the running ones behind its upload
        LAUNCH("key range", launch_key_scan_acc(b.dI + b.dlen, b.dJ + b.dlen, npiece, b.d_acc, b.stream));
        b.dlen += npiece;
        b.sent = b.fill;
    }
    if (!finish && b.fill < FillBuffer::CHUNK) return;
    const int c = b.cur;
    HIPCHK(hipEventRecord(b.uploaded[c], b.stream));
    b.in_flight[c] = true;
    b.fill = 0; b.sent = 0;
    b.cur = 1 - c;
    if (b.in_flight[b.cur]) { HIPCHK(hipEventSynchronize(b.uploaded[b.cur])); b.in_flight[b.cur] = false; }   // its pinned memory is free again
}

}  // namespace

// addelem!  src/buffer.jl:20-31 for n entries (n = 1: one setindex! in fill mode)
void fill_append(FillBuffer& b, const int64_t* I, const int64_t* J, const double* V, int64_t n) {
    fill_init(b);
    int64_t k = 0;
    while (k < n) {
        const int64_t room = std::min(FillBuffer::CHUNK - b.fill, FillBuffer::PIECE - (b.fill - b.sent));      // up to the end of the chunk / of the piece
        const int64_t take = std::min(room, n - k);
        std::memcpy(b.hI[b.cur] + b.fill, I + k, (size_t)take * sizeof(int64_t));
        std::memcpy(b.hJ[b.cur] + b.fill, J + k, (size_t)take * sizeof(int64_t));
        std::memcpy(b.hV[b.cur] + b.fill, V + k, (size_t)take * sizeof(double));
        b.fill += take; k += take;
        if (b.fill == FillBuffer::CHUNK || b.fill - b.sent >= FillBuffer::PIECE) fill_upload_chunk(b, false);
    }
    // a batch of appends has ended: what is staged goes up now (asynchronously), so that closefillmode! finds almost nothing left
    // in pinned memory — single-element appends (setindex! in fill mode) only ship whole quarter chunks
    if (b.fill - b.sent >= (n > 1 ? FillBuffer::EAGER : FillBuffer::CHUNK / 4)) fill_upload_chunk(b, false);
    b.length += n;
}

// get_rowids_colids_vals (src/buffer.jl:33-50) is a no-op here: the triples already sit in HBM; only the last partial chunk is still
// in pinned memory.  Every uploaded piece was folded into five running words on the device (k_minmax_acc) — they come back with the
// wait for the last piece; the appends themselves never look at a key twice.
FillDrain fill_drain(FillBuffer& b) {
    FillDrain d;
    if (!b.stream) return d;
    fill_upload_chunk(b);
    HIPCHK(hipMemcpyAsync(b.h_acc, b.d_acc, 5 * sizeof(long long), hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipStreamSynchronize(b.stream));
    d.nnz = b.dlen;
    if (d.nnz > 0) { d.rows.lo = b.h_acc[0]; d.rows.hi = b.h_acc[1]; d.cols.lo = b.h_acc[2]; d.cols.hi = b.h_acc[3]; }
    return d;
}

}  // namespace host
}  // namespace dsa
