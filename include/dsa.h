/* include/dsa.h — C ABI of libdsa_hip.so, the MI355X (gfx950) packed-memory-array /
 * packed-CSR engine.  This is the drop-in boundary a Julia host module `ccall`s
 * (see INTEGRATION.md for the binding).  The reference package
 * (atoptima/DynamicSparseArrays.jl v0.7.2) has no FFI of its own: each entry point
 * below replaces the Julia method cited next to it (paths relative to the
 * reference checkout).
 *
 * Conventions
 *   - K = L = Int64, T = Float64; semaphore key is 0
 *     (src/pcsr.jl:23), so 0 is rejected as a row/column key of a matrix.
 *   - All indices / positions crossing the ABI are 1-BASED, like the reference.
 *   - Inputs are borrowed host pointers valid for the call only; outputs are
 *     caller-allocated host buffers with explicit capacities.  `*_dev` entry points
 *     take DEVICE pointers (HBM-resident) and enqueue on the handle's stream.
 *   - Every function returns an int32 status; no exceptions cross the boundary.
 *     dsa_last_error_message() returns the text of the last failure on this thread.
 *   - A handle is single-writer / not thread-safe (as the reference).  All slot
 *     storage, occupancy bitmaps, semaphore and column-key tables live in HBM.
 *   - There is NO CPU fallback: every data-path operation runs HIP kernels and
 *     fails with DSA_EHIP if no gfx950 device is usable.
 */
#ifndef DSA_H
#define DSA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes; each mirrors a reference exception site */
enum {
    DSA_OK = 0,
    DSA_EARG = 1,      /* ArgumentError: src/vector.jl:49-50, src/pcsr.jl:208,439-442, src/views.jl:12 */
    DSA_EBOUNDS = 2,   /* BoundsError:   src/pcsr.jl:190, src/moves.jl:10-11 */
    DSA_EDELETED = 3,  /* "The partition has been deleted."  src/pcsr.jl:299 */
    DSA_EFULL = 4,     /* "No empty cell to insert a new element."  src/writes.jl:39 */
    DSA_EMODE = 5,     /* fill-mode misuse: src/matrix.jl:73,84,96,105,127 ; src/buffer.jl:13 */
    DSA_EASSERT = 6,   /* reference @assert sites: src/pcsr.jl:124,132,173,182 */
    DSA_EHIP = 7,      /* HIP runtime failure / no device */
    DSA_ECAP = 8,      /* caller-provided output buffer too small */
    DSA_EKEY = 9,      /* reserved key 0 used as a matrix row/column key */
    DSA_ERCCL = 10     /* RCCL failure / librccl.so not loadable (dsa_comm_*) */
};

enum { DSA_COMBINE_ADD = 0, DSA_COMBINE_MUL = 1, DSA_COMBINE_LAST = 2 };
enum { DSA_COLMAJOR = 0, DSA_ROWMAJOR = 1 };

/* index of the scalars returned by the *_info calls */
enum {
    DSA_INFO_CAPACITY = 0,        /* pma.capacity            src/pma.jl:9  */
    DSA_INFO_SEGMENT_CAPACITY = 1,/* pma.segment_capacity    src/pma.jl:10 */
    DSA_INFO_NB_SEGMENTS = 2,     /* pma.nb_segments         src/pma.jl:11 */
    DSA_INFO_NB_ELEMENTS = 3,     /* pma.nb_elements         src/pma.jl:12 */
    DSA_INFO_HEIGHT = 4,          /* pma.height              src/pma.jl:15 */
    DSA_INFO_NB_PARTITIONS = 5,   /* pcsc.nb_partitions      src/pcsr.jl:5  (vector: length n, src/vector.jl:2) */
    DSA_INFO_TABLE_LEN = 6,       /* length(pcsc.semaphores) == length(col_keys) (tombstones included) */
    DSA_INFO_STAT_WINDOW_SLOTS = 7,/* instrumentation: slots inside pack/spread windows so far */
    DSA_INFO_STAT_REBALANCES = 8, /* instrumentation: number of pack/spread windows so far */
    DSA_INFO_STAT_EXTENDS = 9,
    DSA_INFO_STAT_SHRINKS = 10,
    DSA_INFO_STAT_PAR_ROUNDS = 11, /* batch-parallel rounds / ops applied in parallel / ops applied by the sequencer */
    DSA_INFO_STAT_PAR_OPS = 12,
    DSA_INFO_STAT_SEQ_OPS = 13,
    DSA_INFO_STAT_SPMV_NOMEMSET = 14, /* instrumentation: gather SpMV launches over this orientation that needed no memset of y */
    DSA_INFO_HBM_BYTES = 15,          /* bytes of HBM the structure holds (slot buffers x 2, bitmaps, tables, merge scratch, SpMV plan) */
    DSA_INFO_STAT_GRID_REBALANCES = 16, /* instrumentation: launches of the grid-wide pack/spread kernel (windows above 8192 slots, root, _extend!, _shrink!).
                                         * Windows an append run rebalances are replayed on the bitmap (csrc/appendmodel.hip) and moved by ONE K-permute
                                         * at the end of the run, whatever their size: they count in STAT_REBALANCES / STAT_WINDOW_SLOTS, not here. */
    DSA_INFO_STAT_SPMV_PLAN = 17,       /* instrumentation: dense products over this orientation computed from its column-swept plan */
    DSA_INFO_STAT_SPMV_PLAN_BUILDS = 18,/* instrumentation: builds of that plan (one per content epoch, nx, ny at most; DSA_INFO_HBM_BYTES
                                         * counts the plan while it is held: 12 B per stored cell + a small offset table) */
    DSA_INFO_COUNT = 19
};

typedef struct dsa_vec dsa_vec_t;    /* DynamicSparseVector   src/vector.jl:1-4   */
typedef struct dsa_pcsc dsa_pcsc_t;  /* PackedCSC             src/pcsr.jl:4-9     */
typedef struct dsa_mat dsa_mat_t;    /* DynamicSparseMatrix   src/matrix.jl:1-8   */

const char* dsa_last_error_message(void);
/* number of usable gfx950 devices and selection of the device new handles live on */
int32_t dsa_device_count(int32_t* count);
int32_t dsa_set_device(int32_t device);

/* ---------------- DynamicSparseVector (one PMA) ---------------- */
/* dynamicsparsevec(I, V, combine, n)  src/vector.jl:44-62 ; len < 0 => _guess_length(I) (:6) */
int32_t dsa_vec_create(const int64_t* keys, const double* vals, int64_t n, int32_t combine_op,
                       int64_t len, dsa_vec_t** out);
/* dynamicsparsevec(Int[], Float64[]) -> PackedMemoryArray(K,T)  src/pma.jl:86-91 */
int32_t dsa_vec_create_empty(dsa_vec_t** out);
int32_t dsa_vec_destroy(dsa_vec_t* h);
/* getindex(v, key)  src/vector.jl:73 -> src/pma.jl:189-193 */
int32_t dsa_vec_get(dsa_vec_t* h, int64_t key, double* out);
int32_t dsa_vec_get_batch(dsa_vec_t* h, const int64_t* keys, int64_t n, double* out);
/* setindex!(v, value, key)  src/vector.jl:76-81 -> src/pma.jl:196-213.  WRITE-COMBINED: the call queues the write on the
 * host; queued writes are applied in order by one device sequencer launch at the latest before the next call that observes
 * the vector (get, nnz, info, iteration, export, ...) or when 65536 are pending.  length(v) is updated immediately. */
int32_t dsa_vec_set(dsa_vec_t* h, int64_t key, double val);
/* n sequential setindex! calls, applied in order (sequential-equivalent batch) */
int32_t dsa_vec_set_batch(dsa_vec_t* h, const int64_t* keys, const double* vals, int64_t n);
/* nnz(v) src/vector.jl:88 ; length(v) :69 ; shrink_size!(v) :64 */
int32_t dsa_vec_nnz(dsa_vec_t* h, int64_t* out);
int32_t dsa_vec_len(dsa_vec_t* h, int64_t* out);
int32_t dsa_vec_shrink_size(dsa_vec_t* h);
/* iterate(v) src/vector.jl:71 / nonzeroinds+nonzeros :93-109 : stored entries in slot order */
int32_t dsa_vec_nonzeros(dsa_vec_t* h, int64_t* keys, double* vals, int64_t cap, int64_t* n_out);
/* v1 == v2  src/vector.jl:85-87 -> src/pma.jl:262-266 -> _arrays_equal src/pma.jl:236-260: equal length(v), equal nb_elements and
 * pairwise equal stored (key, value) tuples in slot order (layouts may differ).  *out = 1 / 0.  Both vectors are packed and
 * compared on the device; only the verdict crosses PCIe. */
int32_t dsa_vec_equal(dsa_vec_t* a, dsa_vec_t* b, int32_t* out);
/* alpha * a + beta * b as ascending (key, value) pairs: the SparseVector the reference's  v1 + v2  (1, 1),  v1 - v2  (1, -1) and
 * -v  (-1, 0, b = a) evaluate to through the AbstractSparseVector fallbacks over nonzeroinds / nonzeros
 * (src/vector.jl:93-109; test/functional/math.jl:53-94).  A key stored in both operands keeps one entry, dropped when its value
 * is zero; DSA_ECAP when cap < number of result entries (nnz(a) + nnz(b) always suffices).  Merge + compaction on the device. */
int32_t dsa_vec_axpby(dsa_vec_t* a, double alpha, dsa_vec_t* b, double beta, int64_t* keys, double* vals, int64_t cap, int64_t* n_out);
int32_t dsa_vec_info(dsa_vec_t* h, int64_t info[DSA_INFO_COUNT]);
/* parity probe / snapshot: slot array (keys, vals, occ[i] in {0,1}), cap >= capacity */
int32_t dsa_vec_export_layout(dsa_vec_t* h, int64_t* keys, double* vals, uint8_t* occ, int64_t cap);
/* _even_rebalance!(pma, 1, capacity, nb_elements) on the whole array  src/pma.jl:94-103
 * (benchmark / test hook for the full-window pack+spread kernel; layout-idempotent) */
int32_t dsa_vec_rebalance_root(dsa_vec_t* h);
/* Benchmark / test hook (no reference counterpart): puts the cells of the vector into a layout the reference reaches only
 * in the middle of an operation, WITHOUT changing which cells are stored or their order, so that the next
 * dsa_vec_rebalance_root can be timed on it:
 *   1 = pack!(array, 1, capacity, n): all cells in slots 1..n            (src/moves.jl:94-110; the source of _shrink!)
 *   2 = all cells in the LAST n slots (all gaps at the left: the window a run of appends leaves behind)
 *   3 = _extend!  (src/pma.jl:143-151: capacity x 2, root spread)        4 = _shrink! (src/pma.jl:153-161: capacity / 2)
 * 3 and 4 ignore the density thresholds; 1 and 2 leave a layout that violates them until the next root rebalance. */
int32_t dsa_vec_dev_relayout(dsa_vec_t* h, int32_t mode);

/* ---- DynamicSparseVector as a device operand (csrc/vecops.hip, csrc/vecops_host.hip; HIP library only).  d_* are DEVICE arrays; every
 * call applies the queued writes of its vector operands first and works on their packed cells, on the vector's own stream.
 *
 * nonzeroinds(v) / nonzeros(v) (src/vector.jl:93-109) delivered into HBM: the stored pairs in ascending key order, keys as int64
 * whatever the physical key width.  *n_out = nnz(v) on return, also with DSA_ECAP (cap < nnz: nothing is written).  The copy is
 * enqueued on the vector's stream (dsa_vec_set_stream / dsa_vec_sync); the host does not wait for it. */
int32_t dsa_vec_nonzeros_dev(dsa_vec_t* h, int64_t* d_keys, double* d_vals, int64_t cap, int64_t* n_out);
/* dynamicsparsevec(I, V, combine, n) (src/vector.jl:44-62) with I and V in HBM: any order, duplicates folded by combine_op as
 * dsa_vec_create folds them; len < 0 => _guess_length(I) (:6), found on the device.  The result is slot for slot the vector
 * dsa_vec_create builds from the same arrays.  The arrays are read on the new vector's stream and are the caller's again on return. */
int32_t dsa_vec_create_dev(const int64_t* d_keys, const double* d_vals, int64_t n, int32_t combine_op, int64_t len, dsa_vec_t** out);
/* v1 + v2 (1, 1), v1 - v2 (1, -1), -v (-1, 0, b = a) — the AbstractSparseVector fallbacks dsa_vec_axpby serves — as a NEW dynamic
 * vector of length max(length(a), length(b)): *out = dynamicsparsevec of exactly the pairs dsa_vec_axpby delivers (same merge, same
 * both-stored rule, same bits), built from the compacted pairs in HBM.  b == a is allowed.  The operands are only read. */
int32_t dsa_vec_axpby_vec(dsa_vec_t* a, double alpha, dsa_vec_t* b, double beta, dsa_vec_t** out);
/* sum(v), sum(abs, v), sum(abs2, v), maximum(abs, v) over the stored values (the generic AbstractArray fallbacks the reference leaves
 * to Base; norm(v, 1 | 2 | Inf) are these): kind = DSA_RED_SUM, _ABSSUM, _SQSUM or _ABSMAX (DSA_RED_COUNT is DSA_EARG: dsa_vec_nnz).
 * Two stages over the packed cells in a fixed order, products and sums rounded separately, no floating-point atomics: the bits depend
 * on the stored pairs only (not on the layout) and repeat from call to call.  Every sum starts at +0.0 (an empty vector: +0.0; a sum
 * of negative zeros: +0.0).  DSA_RED_ABSMAX propagates NaN. */
int32_t dsa_vec_reduce(dsa_vec_t* h, int32_t kind, double* out);
/* dot(v, w) (the AbstractSparseVector fallback): the sum over the keys stored in BOTH operands of the rounded products a_k * b_k, in
 * the same two stages (driven by the operand with fewer stored cells, ties by a; the other one is bisected).  Empty or disjoint
 * operands: +0.0.  dsa_vec_dot(a, a) is bit for bit dsa_vec_reduce(a, DSA_RED_SQSUM). */
int32_t dsa_vec_dot(dsa_vec_t* a, dsa_vec_t* b, double* out);
/* dot(v, x) with a dense x of nx entries in HBM: the sum of the rounded products v_k * x[k - 1].  DSA_EBOUNDS when v stores a key
 * outside 1..nx (checked in the same pass; *out is then +0.0). */
int32_t dsa_vec_dot_dense_dev(dsa_vec_t* h, const double* d_x, int64_t nx, double* out);
/* Vector(v) into HBM: d_x[0 .. nx) = 0, then d_x[k - 1] = v_k — a dynamic vector as an operand of dsa_mat_spmm_dense_dev.  DSA_EBOUNDS
 * when v stores a key outside 1..nx, found before the first write (d_x is untouched).  The writes are enqueued on the vector's stream
 * (dsa_vec_sync); the host waits for the bounds verdict only. */
int32_t dsa_vec_to_dense_dev(dsa_vec_t* h, double* d_x, int64_t nx);

/* ---------------- PackedCSC (integer-indexed partitions) ---------------- */
/* PackedCSC(row_keys::Vector{Vector}, values::Vector{Vector}, combine)  src/pcsr.jl:26-63
 * given CSC-style: partition p holds entries [colptr[p], colptr[p+1]) (0-based offsets, nparts+1 entries) */
int32_t dsa_pcsc_create(const int64_t* colptr, int64_t nparts, const int64_t* row_keys,
                        const double* vals, int32_t combine_op, dsa_pcsc_t** out);
int32_t dsa_pcsc_create_empty(dsa_pcsc_t** out);                       /* src/pcsr.jl:65-68 */
int32_t dsa_pcsc_destroy(dsa_pcsc_t* h);
int32_t dsa_pcsc_get(dsa_pcsc_t* h, int64_t key, int64_t partition, double* out);   /* src/pcsr.jl:228-232 */
int32_t dsa_pcsc_set(dsa_pcsc_t* h, double val, int64_t key, int64_t partition);    /* src/pcsr.jl:294-310 */
int32_t dsa_pcsc_deletepartition(dsa_pcsc_t* h, int64_t partition);                 /* src/pcsr.jl:188-204 */
int32_t dsa_pcsc_nnz(dsa_pcsc_t* h, int64_t* out);                                  /* src/pcsr.jl:11 */
int32_t dsa_pcsc_nbpartitions(dsa_pcsc_t* h, int64_t* out);                         /* src/pcsr.jl:21 */
int32_t dsa_pcsc_info(dsa_pcsc_t* h, int64_t info[DSA_INFO_COUNT]);
/* semaphores[id] = slot of partition id's semaphore, 0 = nothing (tombstone) */
int32_t dsa_pcsc_export_layout(dsa_pcsc_t* h, int64_t* keys, double* vals, uint8_t* occ, int64_t cap,
                               int64_t* semaphores, int64_t table_cap);

/* ---------------- DynamicSparseMatrix (colmajor + rowmajor MappedPackedCSC, or fill buffer) ---------------- */
/* dynamicsparse(I, J, V, m, n)  src/matrix.jl:15-19 -> dynamicsparsecolmajor src/pcsr.jl:433-445 (x2) ;
 * m, n < 0 => _guess_length */
int32_t dsa_mat_create_from_coo(const int64_t* I, const int64_t* J, const double* V, int64_t nnz,
                                int64_t m, int64_t n, dsa_mat_t** out);
/* dynamicsparse(I, J, V, m, n) with the triples ALREADY IN HBM: every array is a device address and stays the caller's.  index_bits
 * 32 | 64 (d_I and d_J share it), index_base 0 | 1, key = index + 1 - base.  The result is the matrix dsa_mat_create_from_coo builds
 * from those 1-based int64 keys in input order, slot for slot: duplicates summed in input order, a 0.0 stays a stored zero; m, n < 0 =>
 * _guess_length.  With 64 bits and base 1 the arrays are read in place (any non-zero key, negative ones included).  The arrays must be
 * complete when the call is made; when it returns, with success or with an error, nothing enqueued reads them any more.  The number of
 * launches and host waits does not depend on nnz; no device-to-host copy grows with it.
 * DSA_EARG: index_bits / index_base invalid, nnz < 0 or > 2^32 - 1, a NULL array with nnz > 0, with 32 bits a dimension or nnz + base
 * above INT32_MAX.  DSA_EKEY: a key that maps to 0 (found on the device).  On any error *out is untouched. */
int32_t dsa_mat_create_from_coo_dev(const void* d_I, const void* d_J, const double* d_V, int64_t nnz,
                                    int32_t index_bits, int32_t index_base, int64_t m, int64_t n, dsa_mat_t** out);
/* The same from a compressed form in HBM, the conventions of dsa_mat_to_compressed_dev (an export can be fed straight back):
 * orientation DSA_ROWMAJOR = CSR (outer = rows, size = outer x inner), DSA_COLMAJOR = CSC (outer = columns, size = inner x outer);
 * ptr (outer + 1 entries) and idx (nnz entries) share index_bits, index_base offsets both.  The outer key of position p is the j
 * (1-based) with ptr[j-1] - base <= p < ptr[j] - base, the inner key idx[p] + 1 - base; input order is storage order.  The inner
 * indices of a slice need not be sorted or unique.
 * DSA_EARG: orientation / index_bits / index_base invalid, nnz < 0 or > 2^32 - 1, outer or inner < 0, d_ptr NULL (also with nnz = 0),
 * d_idx or d_vals NULL with nnz > 0, with 32 bits a dimension or nnz + base above INT32_MAX, a malformed ptr (ptr[0] != base,
 * ptr[outer] != base + nnz, a decreasing step).  DSA_EBOUNDS: an inner index outside base .. base + inner - 1.  The malformed ptr
 * and the index out of range are found on the device; no input makes a kernel read outside the caller's arrays. */
int32_t dsa_mat_create_from_compressed_dev(int32_t orientation, int32_t index_bits, int32_t index_base,
                                           const void* d_ptr, const void* d_idx, const double* d_vals,
                                           int64_t outer, int64_t inner, int64_t nnz, dsa_mat_t** out);
/* Combine: a new matrix out of one or two existing ones, on the device (not in the reference: Base.copy, +, -, hcat, vcat and
 * blockdiag of the wrappers are all this call).  The result is the matrix dsa_mat_create_from_coo(I, J, V, m, n) builds, slot for
 * slot, from this triple list in this order: every stored cell of `a` in the slot order of its colmajor orientation (the findnz
 * order) as (i, j, alpha * v), then every stored cell of `b` in the same order as (i + row_off, j + col_off, beta * v).
 * b == NULL: no second operand (beta, row_off, col_off ignored): copy / alpha * A.  b == a is allowed (A + A).
 * One IEEE multiply per cell, also for a factor 1.0; no add: a key present in both operands is summed by the builder as it sums any
 * duplicate in input order, a sum that cancels stays a stored zero (dsa_mat_droptol), stored zeros of the operands stay stored.
 * m, n >= 0 give size(result); m < 0: max(a.m, b.m + row_off) (a.m without b), n < 0 likewise.
 * The operands are only read: slots, tables, epochs and cached SpMV plans are untouched.  *out is a fresh handle out of fill mode.
 * The number of launches and host waits does not depend on nnz or on the number of partitions.
 * DSA_EMODE: an operand is in fill mode.  DSA_EARG: a or out NULL, nnz(a) + nnz(b) > 2^32 - 1, an offset whose sum with a stored key or
 * with a dimension leaves int64.  DSA_EKEY: a shifted key equals 0 (found on the device).  DSA_EBOUNDS with col_off != 0: a or b holds
 * a stored entry whose column key lies outside 1 .. n of its own size(); with row_off != 0 the same for rows (a shifted block must
 * not silently land on the other operand's cells; with both offsets 0 nothing is bounds-checked: negative or out-of-size keys are
 * copied and added as they are).  DSA_EASSERT: slots and tables disagree.  On any error *out is untouched and nothing stays allocated. */
int32_t dsa_mat_combine(dsa_mat_t* a, double alpha, dsa_mat_t* b, double beta, int64_t row_off, int64_t col_off,
                        int64_t m, int64_t n, dsa_mat_t** out);
/* dynamicsparse(K, L, T; fill_mode)  src/matrix.jl:31-41 */
int32_t dsa_mat_create_empty(int32_t fill_mode, dsa_mat_t** out);
int32_t dsa_mat_destroy(dsa_mat_t* h);
/* setindex!(m, val, row, col)  src/matrix.jl:43-62 (fill mode: addelem! src/buffer.jl:20-31).  WRITE-COMBINED like
 * dsa_vec_set (size(m) is updated immediately); when the matrix holds deleted columns/rows — the only state in which a write
 * can fail in the reference — the write is applied before the call returns so the error surfaces here. */
int32_t dsa_mat_set(dsa_mat_t* h, double val, int64_t row, int64_t col);
/* n sequential setindex! calls in order.  On success the state equals that of the n calls.  When write k fails (only possible while
 * the matrix holds deleted columns / rows) the status, size(m) and the contents are those of the reference at its
 * exception (src/matrix.jl:43-62 updates colmajor, then rowmajor): both orientations hold writes [0, k), colmajor also holds write k when
 * it was the rowmajor statement that threw.  (The orientation that refused the write keeps its partition tables as they were; the
 * reference leaves them half shifted — a state nothing can continue from.) */
int32_t dsa_mat_set_batch(dsa_mat_t* h, const int64_t* I, const int64_t* J, const double* V, int64_t n);
/* getindex(m, row, col)  src/matrix.jl:64-68 */
int32_t dsa_mat_get(dsa_mat_t* h, int64_t row, int64_t col, double* out);
int32_t dsa_mat_get_batch(dsa_mat_t* h, const int64_t* I, const int64_t* J, int64_t n, double* out);
/* addrow!(matrix, row, colids, vals)  src/matrix.jl:113-124 (fill mode: src/buffer.jl:10-18) */
int32_t dsa_mat_addrow(dsa_mat_t* h, int64_t row, const int64_t* colids, const double* vals, int64_t n);
/* closefillmode!  src/matrix.jl:126-134 */
int32_t dsa_mat_closefillmode(dsa_mat_t* h);
/* deletecolumn! / deleterow!  src/matrix.jl:95-111 */
int32_t dsa_mat_deletecolumn(dsa_mat_t* h, int64_t col);
int32_t dsa_mat_deleterow(dsa_mat_t* h, int64_t row);
/* @view m[:, col] / @view m[row, :] iteration  src/matrix.jl:70-93, src/views.jl:15-35 */
int32_t dsa_mat_col_view(dsa_mat_t* h, int64_t col, int64_t* rows, double* vals, int64_t cap, int64_t* n_out);
int32_t dsa_mat_row_view(dsa_mat_t* h, int64_t row, int64_t* cols, double* vals, int64_t cap, int64_t* n_out);
/* the same views delivered into HBM: d_rows / d_vals are DEVICE arrays of cap entries; the cells are packed on the device and copied
 * device-to-device on the orientation's stream (dsa_mat_set_stream / dsa_mat_sync); *n_out is valid on return.  No cell crosses PCIe. */
int32_t dsa_mat_col_view_dev(dsa_mat_t* h, int64_t col, int64_t* d_rows, double* d_vals, int64_t cap, int64_t* n_out);
int32_t dsa_mat_row_view_dev(dsa_mat_t* h, int64_t row, int64_t* d_cols, double* d_vals, int64_t cap, int64_t* n_out);
/* m[:, col] / m[row, :] as a NEW dynamic sparse vector  (getindex(mpcsc, :, col) src/pcsr.jl:285-291 -> :247-259 ;
 * getindex(mpcsc, row, :) src/pcsr.jl:269-283): the stored entries of the column / row, length = largest key.  Device to device: the
 * view kernel packs the partition into the orientation's idle slot buffer and ONE spread launch writes the new vector's slot array
 * from there (PackedMemoryArray(elements), src/pma.jl:69-84); only the entry count and the largest key reach the host. */
int32_t dsa_mat_col_slice(dsa_mat_t* h, int64_t col, dsa_vec_t** out);
int32_t dsa_mat_row_slice(dsa_mat_t* h, int64_t row, dsa_vec_t** out);
/* nnz(m) src/matrix.jl:91 ; size(m) :92 ; nbpartitions(orientation) src/pcsr.jl:21-22 */
int32_t dsa_mat_nnz(dsa_mat_t* h, int64_t* out);
int32_t dsa_mat_size(dsa_mat_t* h, int64_t* m, int64_t* n);
int32_t dsa_mat_nbpartitions(dsa_mat_t* h, int32_t orientation, int64_t* out);
int32_t dsa_mat_info(dsa_mat_t* h, int32_t orientation, int64_t info[DSA_INFO_COUNT]);
/* parity probe: slot array + semaphores[id] (0 = nothing) + col_keys[id] with col_live[id] in {0,1} */
int32_t dsa_mat_export_layout(dsa_mat_t* h, int32_t orientation, int64_t* keys, double* vals,
                              uint8_t* occ, int64_t cap, int64_t* semaphores, int64_t* col_keys,
                              uint8_t* col_live, int64_t table_cap);
/* _even_rebalance!(pcsc, 1, capacity, nb_elements) of one orientation  src/pcsr.jl:88-97 */
int32_t dsa_mat_rebalance_root(dsa_mat_t* h, int32_t orientation);
/* The stored entries of the matrix in compressed form.  orientation DSA_COLMAJOR: CSC, outer = columns 1..n, inner = rows;
 * DSA_ROWMAJOR: CSR, outer = rows 1..m, inner = columns; (m, n) = dsa_mat_size at the call.  ptr has outer + 1 entries, idx / vals
 * cap entries; *nnz_out = nnz(m) on return, also with DSA_ECAP (cap < nnz, nothing launched).  index_bits 32 | 64 (32: DSA_EARG when
 * a dimension or nnz + base does not fit), index_base 0 | 1.  DSA_EMODE in fill mode; DSA_EBOUNDS when a stored entry lies outside
 * size(m).  Enqueued on the orientation's stream (dsa_mat_set_stream / dsa_mat_sync); waits only for the bounds word.  Stored zeros
 * are exported as stored; idx ascends within every outer index (findnz(m) order for CSC). */
int32_t dsa_mat_to_compressed_dev(dsa_mat_t* h, int32_t orientation, int32_t index_bits, int32_t index_base,
                                  void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out);
/* the same into host arrays, int64 indices (findnz / SparseMatrixCSC / scipy) */
int32_t dsa_mat_to_compressed(dsa_mat_t* h, int32_t orientation, int32_t index_base,
                              int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out);

/* Selected columns (orientation DSA_COLMAJOR: A[:, sel] as CSC) or rows (DSA_ROWMAJOR: A[sel, :] as CSR) in compressed form.  sel holds
 * nsel OUTER keys (column keys for colmajor, row keys for rowmajor): 1-based, in any order, repeats allowed, 0 <= nsel <= 2^31 - 1.  The
 * j-th outer slice of the result is the live partition whose key is sel[j]: ptr has nsel + 1 entries, ptr[j] = base + cells of the
 * slices in front of j; idx / vals hold, for j = 0, 1, ..., the cells of that partition in slot order (ascending inner key),
 * idx = key - 1 + base, values copied bit for bit (stored zeros as stored).  A key inside 1..dim_out without a live partition (never
 * written, deleted, or empty) gives an empty slice.  With repeats the result may hold more cells than nnz(m); nsel = 0 gives
 * ptr = [base].  dim_out = n (colmajor) | m (rowmajor), dim_in the other one, (m, n) = dsa_mat_size at the call.
 * Every cell of a selected partition is delivered; inner-index selection and renumbering (A[I, J] with both lists) is
 * dsa_mat_submatrix_compressed[_dev] below.
 * _dev: every array is a device address; enqueued on the orientation's stream (dsa_mat_set_stream / dsa_mat_sync).  The host waits
 * twice: for the total, which only the device knows, and behind the emit for the bounds word.  The number of launches and waits does
 * not depend on nsel.  *nnz_out = the number of selected cells on return, also with DSA_ECAP.
 * Capacity: cap < total returns DSA_ECAP with *nnz_out = total, ptr COMPLETE AND VALID, idx / vals untouched.  cap = 0 with
 * d_idx = d_vals = NULL is the count-only call (DSA_OK when the total is 0): it sizes the caller's buffers and gives the entries per
 * selected key as the differences of ptr.  The second call looks the keys up again: nothing about a selection stays on the handle.
 * Errors: DSA_EMODE in fill mode.  DSA_EARG: orientation, index_bits (32 | 64) or index_base (0 | 1) invalid; nsel out of range;
 * ptr NULL, sel NULL with nsel > 0, idx or vals NULL with cap > 0; with index_bits 32, dim_in > INT32_MAX or total + base >
 * INT32_MAX (the latter found after the count).  DSA_EBOUNDS: a selected key outside 1..dim_out (0 included), or a cell of a
 * SELECTED partition whose inner key lies outside 1..dim_in (partitions that are not selected are not looked at).  DSA_EASSERT:
 * partition tables and slot array out of step.  Read-only: slots, tables and both epochs stay as they are, a cached SpMV plan
 * survives. */
int32_t dsa_mat_select_compressed_dev(dsa_mat_t* h, int32_t orientation, int32_t index_bits, int32_t index_base,
                                      const int64_t* d_sel, int64_t nsel,
                                      void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out);
/* the same with host arrays and int64 indices, staged through pooled device memory (DSA_ECAP leaves ptr filled) */
int32_t dsa_mat_select_compressed(dsa_mat_t* h, int32_t orientation, int32_t index_base,
                                  const int64_t* sel, int64_t nsel,
                                  int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out);

/* The submatrix A[I, J] in compressed form, both sides selected and renumbered on the device.  orientation DSA_COLMAJOR: outer =
 * column keys, inner = row keys, the result is A[inner, outer] as CSC of shape (ninner, nouter); DSA_ROWMAJOR: outer = row keys,
 * inner = column keys, the result is A[outer, inner] as CSR of shape (nouter, ninner).  The OUTER list behaves exactly as sel of
 * dsa_mat_select_compressed: nouter keys, 1-based, in any order, repeats allowed, a key inside 1..dim_out without a live partition
 * gives an empty slice, nouter = 0 gives ptr = [base].  The INNER list holds ninner keys, 1-based, in any order, all DISTINCT.  A
 * cell of a selected partition is delivered iff its inner key is in the inner list; its idx is the 0-based position of that key in
 * the inner list + base.  ptr has nouter + 1 entries, ptr[j] = base + delivered cells of the slices in front of j.  Within a slice
 * the cells come out in slot order, i.e. by ascending ORIGINAL inner key: idx ascends within every slice iff the inner list
 * ascends (a permuted inner list gives a valid but unsorted CSC / CSR).  Values are copied bit for bit, stored zeros as stored.
 * ninner = 0 gives an all-empty result with a valid ptr.  The result is bit-identical from call to call.
 * _dev: every array is a device address; enqueued on the orientation's stream (dsa_mat_set_stream / dsa_mat_sync).  Six kernel
 * launches and three host waits (work items of the selected spans, the total, the error word behind the emit), whatever nouter,
 * ninner and the lengths of the partitions are; pooled scratch of O(nouter + ninner + selected slots / 2048) bytes: nothing is
 * proportional to the capacity or to dim_in.  *nnz_out = the number of delivered cells on return, also with DSA_ECAP.
 * Capacity: as for dsa_mat_select_compressed_dev.  cap < total returns DSA_ECAP with *nnz_out = total, ptr COMPLETE AND VALID, idx /
 * vals untouched; cap = 0 with d_idx = d_vals = NULL is the count-only call (DSA_OK when the total is 0).  Nothing about a selection
 * stays on the handle.
 * Errors: DSA_EMODE in fill mode.  DSA_EARG: orientation, index_bits (32 | 64) or index_base (0 | 1) invalid; nouter or ninner
 * outside 0 .. 2^31 - 1; ptr NULL, a key list NULL with a length > 0, idx or vals NULL with cap > 0; an inner key listed twice
 * (found on the device); with index_bits 32, ninner > INT32_MAX or total + base > INT32_MAX (dim_in need NOT fit: only positions
 * are written).  DSA_EBOUNDS: an outer key outside 1..dim_out, an inner key outside 1..dim_in, or a cell of a SELECTED partition
 * whose stored inner key lies outside 1..dim_in, whether it is listed or not (found by the count: also reported by the count-only
 * call).  DSA_EASSERT: partition tables and slot array out of step.  Read-only: slots, tables and both epochs stay as they are, a
 * cached SpMV plan survives. */
int32_t dsa_mat_submatrix_compressed_dev(dsa_mat_t* h, int32_t orientation, int32_t index_bits, int32_t index_base,
                                         const int64_t* d_outer, int64_t nouter, const int64_t* d_inner, int64_t ninner,
                                         void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out);
/* the same with host arrays and int64 indices, staged through pooled device memory (DSA_ECAP leaves ptr filled) */
int32_t dsa_mat_submatrix_compressed(dsa_mat_t* h, int32_t orientation, int32_t index_base,
                                     const int64_t* outer, int64_t nouter, const int64_t* inner, int64_t ninner,
                                     int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out);

/* ---- SpMV:  mat * v, transpose(mat) * v   src/operations.jl:14-60 -> _mul :107-135 ---- */
/* dense x (every index of x is a stored entry), dense y of length ny; rows never touched are 0.
 * transpose = 0: y = A x  (nx >= #cols used, ny = m) ; transpose = 1: y = A' x. */
int32_t dsa_mat_spmv_dense(dsa_mat_t* h, int32_t transpose, const double* x, int64_t nx,
                           double* y, int64_t ny);
/* sparse x given by its stored entries (xi ascending) ; result = touched rows only, ascending,
 * stored zeros kept: the shape of _mul_output(result, n)  src/operations.jl:11-12.
 * Only the columns x stores are visited, as in _mul: a stored Inf / NaN of the matrix makes a row non-finite only through a column
 * x stores (a stored 0.0 of x included: 0 * Inf = NaN); an absent entry of x contributes nothing.  This holds for every
 * dsa_mat_spmv_sparse* entry point, however many entries x has. */
int32_t dsa_mat_spmv_sparse(dsa_mat_t* h, int32_t transpose, const int64_t* xi, const double* xv,
                            int64_t nx, int64_t* yi, double* yv, int64_t cap, int64_t* n_out);
/* The same product in two steps, so that the caller allocates exactly what the result needs: _begin computes (result left with the
 * handle: packed in HBM, short ones also in pinned memory) and returns the number of touched rows, _fetch copies the pairs out
 * (DSA_ECAP when cap is too small: the result stays fetchable).  dsa_mat_spmv_sparse == _begin + _fetch.  One result per handle: the
 * next _begin / dsa_mat_spmv_sparse* call replaces it. */
int32_t dsa_mat_spmv_sparse_begin(dsa_mat_t* h, int32_t transpose, const int64_t* xi, const double* xv, int64_t nx, int64_t* n_out);
int32_t dsa_mat_spmv_sparse_fetch(dsa_mat_t* h, int64_t* yi, double* yv, int64_t cap, int64_t* n_out);
/* The sparse product with every operand in HBM, stream-ordered, no host wait: d_xi / d_xv = the nx stored entries of x (ascending
 * indices; not checked), d_yi / d_yv = cap entries for the touched rows (ascending), *d_count (device) = their number — pairs beyond
 * cap are dropped, the count still says how many there are (cap = size(m, 1 | 2) always suffices).  Enqueued on the stream of the
 * orientation that is walked (dsa_mat_set_stream / dsa_mat_sync).  With many stored entries (8 nx >= number of columns: gather over the
 * twin orientation) entries of x outside 1..n are ignored — column keys below 1 need the host entry point or fewer entries. */
int32_t dsa_mat_spmv_sparse_dev(dsa_mat_t* h, int32_t transpose, const int64_t* d_xi, const double* d_xv, int64_t nx,
                                int64_t* d_yi, double* d_yv, int64_t cap, int64_t* d_count);
/* mat * v / transpose(mat) * v for a DynamicSparseVector (src/operations.jl:14-36, the method whose operand is a dynamic vector) with a
 * dynamic vector as the result: *out = dynamicsparsevec(rows, values, +, size(mat, 1 | 2)) of the pairs dsa_mat_spmv_sparse returns for
 * x's stored pairs — same touched rows, same rule for a stored Inf / NaN, keys of x below 1 or beyond the dimension included; what the
 * builder does with a stored zero of the result is what dsa_vec_create does with it.  x is packed and widened on the device, the
 * product runs by the strategy rule of dsa_mat_spmv_sparse (few stored entries: driven by x; many: gather over the twin — then the
 * first packed key of x comes back, and a key below 1 hands the product to the x-driven kernel), the result is built from the packed
 * pairs in HBM: only counts and that one key cross PCIe.  x is only read (its next write is ordered behind the product).  Replaces
 * the result a dsa_mat_spmv_sparse_begin left with the handle.  DSA_EMODE in fill mode.  HIP library only. */
int32_t dsa_mat_mul_vec(dsa_mat_t* h, int32_t transpose, dsa_vec_t* x, dsa_vec_t** out);
/* same as dsa_mat_spmv_dense with x, y resident in HBM; asynchronous on the handle's stream.
 * algo: 0 = gather over the twin orientation (default), 1 = scatter over the reference's own
 * orientation with fp64 atomics (the literal _mul loop nest) */
int32_t dsa_mat_spmv_dense_dev(dsa_mat_t* h, int32_t transpose, int32_t algo, const double* d_x,
                               int64_t nx, double* d_y, int64_t ny);
/* Dense multi-vector product (SpMM), the k-column form of _mul (src/operations.jl:107-135); no reference counterpart.
 * Y = A X (transpose = 0: X is nx x k, Y is ny x k, ny = m) or Y = A' X (transpose = 1), X and Y dense, ROW-MAJOR:
 * X[i, j] = x[i * ldx + j], Y[i, j] = y[i * ldy + j], ldx >= k, ldy >= k.  Column j of Y is what dsa_mat_spmv_dense computes
 * for column j of X: Y[r, j] = 0.0 + a1 * X[c1, j] + a2 * X[c2, j] + ... over the stored cells of row r in ascending key order, added
 * left to right, one multiply then one add per term (no FMA) — the reference's order, for rows of any length.  Rows without a
 * partition are +0.0; a cell whose key is outside 1..nx contributes nothing, a partition whose key is outside 1..ny writes nothing.
 * y[i * ldy + j] for k <= j < ldy is not written.  x and y must not overlap.  k > 16 reads the matrix once per 16 columns.
 * DSA_EARG: k < 1, ldx < k, ldy < k, negative nx / ny, NULL operand of a non-empty shape; DSA_EMODE in fill mode.
 * _dev: operands resident in HBM, asynchronous on the stream of the orientation that is walked (rowmajor for transpose = 0, colmajor
 * for transpose = 1; dsa_mat_set_stream / dsa_mat_sync).  The host form stages through pooled device memory and waits. */
int32_t dsa_mat_spmm_dense_dev(dsa_mat_t* h, int32_t transpose, const double* d_x, int64_t nx, int64_t k, int64_t ldx,
                               double* d_y, int64_t ny, int64_t ldy);
int32_t dsa_mat_spmm_dense(dsa_mat_t* h, int32_t transpose, const double* x, int64_t nx, int64_t k, int64_t ldx,
                           double* y, int64_t ny, int64_t ldy);
/* The same product for a LIST of outer keys only (csrc/selprod.hip): row j of Y (nsel x k, leading dimension ldy) is the product of
 * the live partition whose key is sel[j] with X (nx x k, ldx).  transpose = 0: row keys, the rowmajor orientation, Y = A[sel, :] X;
 * transpose = 1: column keys, colmajor, Y = A[:, sel]' X.  Keys are 1-based, in any order, and may repeat: every occurrence gets its
 * own row.  A row is summed exactly as by dsa_mat_spmm_dense (slot order, from +0.0, one multiply then one add per term, no FMA, any
 * length, no atomics): for a key with a live partition Y[j] is bit-identical to row sel[j] - 1 of the full product, and two calls
 * give the same bits.  A key without a live partition (never written, deleted, beyond size(m)) gives a row of +0.0; a cell whose
 * inner key is outside 1..nx contributes nothing.  Every row of Y is stored exactly once, columns k..ldy-1 are not written.  The
 * cost follows the selected spans, not the capacity; k > 16 reads them once per 16 columns.
 * _dev: every array is a device address; stream-ordered on the stream of the orientation that is walked (dsa_mat_set_stream /
 * dsa_mat_sync): NO host wait and no hand-over, so a bad key cannot be reported: a key < 1 gives the zero row like any other key
 * without a partition.  The host form sees the keys and rejects one < 1 with DSA_EARG before any launch; it stages through pooled
 * device memory and waits.  Arguments are checked before anything is enqueued (Y is untouched on an error): DSA_EMODE in fill mode;
 * DSA_EARG: k < 1, ldx < k, ldy < k, nsel outside 0 .. 2^31 - 1, nx < 0, sel or y NULL with nsel > 0, x NULL with nx > 0.
 * nsel = 0 launches nothing; nx = 0 writes nsel rows of +0.0.  Read-only: a cached SpMV plan survives. */
int32_t dsa_mat_spmm_selected_dev(dsa_mat_t* h, int32_t transpose, const int64_t* d_sel, int64_t nsel,
                                  const double* d_x, int64_t nx, int64_t k, int64_t ldx, double* d_y, int64_t ldy);
int32_t dsa_mat_spmm_selected(dsa_mat_t* h, int32_t transpose, const int64_t* sel, int64_t nsel,
                              const double* x, int64_t nx, int64_t k, int64_t ldx, double* y, int64_t ldy);
/* The batched sparse-x product (csrc/spgemm.hip): Y = A S (transpose = 0: the colmajor orientation is walked, the indices of S are
 * column keys of A, the indices of Y row keys, ny = m) or Y = A' S (transpose = 1: rowmajor, ny = n) for k SPARSE columns.  S and Y are
 * CSC in the conventions of dsa_mat_to_compressed_dev: xptr[k + 1], xidx / xval[nnzx], yptr[k + 1], yidx / yval[total]; index_bits 32 |
 * 64 covers all four index arrays, index_base 0 | 1: ptr[j] = base + entries in front of column j, idx = key - 1 + base.  The result can
 * go straight into dsa_mat_create_from_compressed_dev.
 * Column j of Y is what the reference's _mul (src/operations.jl:62-135) gives for column j of S: the touched rows only, ascending, a
 * touched row whose sum is 0.0 kept.  A value is summed from +0.0 over the stored entries of the column of S in their order, each
 * matching partition in slot order, one multiply then one add per term (no FMA), WITHOUT float atomics: it is bit-identical to what the
 * reference computes for that column and from call to call (dsa_mat_spmv_sparse* adds with fp64 atomics and cannot promise that).  The
 * one exception is the payload of a NaN, which IEEE 754 leaves open: 0 * Inf gives a NaN of the other sign bit on the device than on an
 * x86 host, so a NaN of the result is a NaN of the reference, not necessarily with the same bits (still the same from call to call).  An
 * entry of S whose key has no live partition (never written, deleted, beyond the table, below 1) contributes nothing.  A stored Inf /
 * NaN of A counts only through a column S stores; a stored 0.0 of S times Inf is NaN.
 * Input contract, checked on the device (DSA_EARG): xptr[0] == base, xptr does not decrease, xptr[k] - base == nnzx, xidx ascends
 * strictly within a column (the reference's loop only moves forward).
 * Capacity: as for dsa_mat_select_compressed_dev.  cap < total returns DSA_ECAP with *nnz_out = total, yptr COMPLETE AND VALID, yidx /
 * yval untouched; cap = 0 with d_yidx = d_yval = NULL is the count-only call (DSA_OK when the total is 0).  The second call computes the
 * spans again: nothing about a product stays on the handle.  *nnz_out = the entries of Y on return, also with DSA_ECAP.
 * A column whose products visit at most 1024 stored cells is summed in an LDS hash table; a longer one in a slab of ny doubles (at
 * most 16 slabs and 1 GiB of them per orientation, kept with the handle, all zero between two calls; csrc/spgemm.h names the four
 * constants).  When a single slab would exceed the byte limit the call returns DSA_EARG and nothing of that size is allocated.
 * Errors: DSA_EMODE in fill mode.  DSA_EARG: transpose, index_bits or index_base invalid; k or nnzx outside 0 .. 2^31 - 1; a NULL array
 * of a non-empty shape (xptr and yptr always, xidx / xval with nnzx > 0, yidx / yval with cap > 0); with index_bits 32, ny or total +
 * base above INT32_MAX; the input contract; the slab limit.  DSA_EBOUNDS: a touched row key outside 1..ny.  DSA_EASSERT: partition
 * tables and slot array out of step, or a full hash table.  Every probe sequence on the device is bounded: a defect ends as a status.
 * _dev: every array is a device address; enqueued on the stream of the orientation that is walked (dsa_mat_set_stream / dsa_mat_sync).
 * One memset and at most eight kernel launches (bound, classify; count in LDS, count in slabs, scan; emit from LDS, emit from slabs,
 * hand-over; the slab launches only with long columns) and at most three host waits through pinned words (input contract and long
 * columns; the total; the error word behind the emit), whatever k, nnzx and the lengths of the partitions are.  A call that needs more
 * scratch or more slab bytes than the handle holds (the first call, the first one with long columns, a larger one) adds to that: a
 * pool allocation, a stream synchronisation before the smaller block is let go, and a second memset over the new slabs.  The slabs
 * stay with the handle until it is destroyed (dsa_pool_trim does not see them).  classify and scan are one workgroup each, looping
 * over the k columns: bounded, but slow for k near 2^31.
 * Cost: the call has a fixed cost of three hand-overs, the LDS path walks the entries of a column one after the other, and the slab
 * path is one entry at a time with a barrier in between: for columns that visit more than 1024 cells, and for a single short column,
 * k calls of dsa_mat_spmv_sparse_dev are far faster (README.md holds the measured points).  Read-only: slots, tables and both epochs
 * stay as they are, a cached SpMV plan survives. */
int32_t dsa_mat_spgemm_csc_dev(dsa_mat_t* h, int32_t transpose, int32_t index_bits, int32_t index_base,
                               const void* d_xptr, const void* d_xidx, const double* d_xval, int64_t k, int64_t nnzx,
                               void* d_yptr, void* d_yidx, double* d_yval, int64_t cap, int64_t* nnz_out);
/* the same with host arrays and int64 indices (nnzx = xptr[k] - base), staged through pooled device memory (DSA_ECAP leaves yptr filled) */
int32_t dsa_mat_spgemm_csc(dsa_mat_t* h, int32_t transpose, int32_t index_base,
                           const int64_t* xptr, const int64_t* xidx, const double* xval, int64_t k,
                           int64_t* yptr, int64_t* yidx, double* yval, int64_t cap, int64_t* nnz_out);
/* ---- reductions per row / column and in-place diagonal scaling (csrc/scale.hip).  No reference counterpart: what sum(abs, A; dims),
 * maximum(abs, ...) and SparseArrays' lmul! / rmul! with Diagonal factors do for a SparseMatrixCSC.
 *
 * Reduce: orientation DSA_ROWMAJOR gives one value per row (n_out must equal m, the rowmajor orientation is walked), DSA_COLMAJOR one
 * per column (n_out must equal n, colmajor); (m, n) = dsa_mat_size after the queued single writes have been applied.  out[key - 1] is
 * the reduction over the STORED cells of row / column `key` (stored zeros count): the sum of v, of |v|, of v * v (a rounded multiply,
 * then separate adds: no FMA), the maximum of |v|, or the number of cells (as a double).  A key without stored cells gives +0.0; every
 * sum starts at +0.0.  DSA_RED_ABSMAX propagates NaN (a NaN cell makes its result NaN, like Julia's maximum(abs, ...)).  The order in
 * which the terms of a row are added is fixed by the slot layout alone: no floating-point atomics, two calls on the same state give
 * the same bits; it is NOT the left-to-right order of dsa_mat_spmm_dense.  Rows of any length are summed correctly.  Read-only: a
 * cached SpMV plan survives.
 * DSA_EMODE in fill mode; DSA_EARG: orientation or kind invalid, n_out != the dimension, out NULL with n_out > 0; DSA_EBOUNDS: a
 * stored row / column key outside 1..n_out (possible only after dynamicsparse with an explicit m / n smaller than the keys).
 * _dev: d_out is a device array; enqueued on the stream of the orientation that is walked (dsa_mat_set_stream / dsa_mat_sync); the host
 * waits only for the bounds word.  The host form stages through pooled device memory and waits. */
enum { DSA_RED_SUM = 0, DSA_RED_ABSSUM = 1, DSA_RED_SQSUM = 2, DSA_RED_ABSMAX = 3, DSA_RED_COUNT = 4 };
int32_t dsa_mat_reduce_dev(dsa_mat_t* h, int32_t orientation, int32_t kind, double* d_out, int64_t n_out);
int32_t dsa_mat_reduce(dsa_mat_t* h, int32_t orientation, int32_t kind, double* out, int64_t n_out);
/* Scale: every stored cell A[i, j] = v becomes ((v * alpha) * r[i - 1]) * c[j - 1] — D_r * (alpha A) * D_c — three separately rounded
 * multiplies in that order, in BOTH orientations, so that a cell holds the same bits in colmajor and rowmajor.  r or c NULL (its length
 * argument is then ignored) means that the factor is absent, which equals a factor of 1.0 exactly; when given, nr must equal m and nc
 * must equal n (dsa_mat_size after the queued single writes have been applied).
 * STRUCTURE IS PRESERVED, like lmul! / rmul! on a SparseMatrixCSC: a zero factor leaves a STORED 0.0 — nnz is unchanged, A[i, j] reads
 * 0.0, the cell is still exported and counted by DSA_RED_COUNT.  Non-finite factors follow IEEE (0 * Inf = NaN is stored).  Only the
 * values of stored cells are written: no slot moves, keys, tables, counts and the rebalance / extend statistics stay as they are.  The
 * content changes: cached SpMV plans are dropped.
 * DSA_EMODE in fill mode; DSA_EARG: nr != m or nc != n for a factor that is given; DSA_EBOUNDS: a stored entry outside size(m), found
 * by a pass in front of the first write — NEITHER orientation is modified.
 * _dev: d_r / d_c are device arrays, read on BOTH orientations' streams: they must hold their final contents when the call is made
 * (synchronise the stream that produced them first) and stay valid and unchanged until dsa_mat_sync.  The host waits for the bounds
 * pass only.  The host form stages r and c through pooled device memory and waits for both streams. */
int32_t dsa_mat_scale_dev(dsa_mat_t* h, double alpha, const double* d_r, int64_t nr, const double* d_c, int64_t nc);
int32_t dsa_mat_scale(dsa_mat_t* h, double alpha, const double* r, int64_t nr, const double* c, int64_t nc);
/* Batched delete: every column (orientation = DSA_COLMAJOR) or row (DSA_ROWMAJOR) of a key list leaves the matrix in one device pass.
 * CONTENT, partition tables and size() afterwards are those of deletecolumn! / deleterow! (src/matrix.jl:95-111; deletepartition!,
 * src/pcsr.jl:188-212) called for the same keys one after the other: in the orientation whose partitions the keys name every listed
 * partition goes away with its semaphore and its table entry becomes a tombstone (table_len unchanged); in the other orientation every
 * entry whose inner key is listed goes away and every semaphore stays; size(m) is unchanged.  The LAYOUT is not that of n sequential
 * deletes: capacity, height, segment capacity and thresholds stay, and the surviving cells of each orientation, in slot order, are
 * spread over [1, capacity] by the reference's spread! rule — what dsa_mat_rebalance_root gives (a single-leaf array is not moved).
 * The batch never shrinks; the next write that reaches the root does, as after the reference's own deletes.
 * The list may be in any order and must hold distinct keys, each a live partition of its orientation.  Every error is found before
 * the first write — both orientations and the cached SpMV plans stay as they were: DSA_EMODE in fill mode; DSA_EARG for n < 0, a
 * repeated key, a key that is absent, already deleted or <= 0 (dsa_last_error names the first offending key; of a key listed more than
 * twice the occurrence that counts is the second or a later one).  n = 0 does nothing.  Queued single writes are applied first.
 * removed_out (host pointer, may be NULL) receives the number of matrix entries removed.  The call returns with both streams drained.
 * _dev: d_keys is a device array that holds its final contents when the call is made.  The host form stages the keys through pooled
 * device memory.  For one or two keys dsa_mat_deletecolumn / dsa_mat_deleterow remain the cheaper calls. */
int32_t dsa_mat_delete_batch_dev(dsa_mat_t* h, int32_t orientation, const int64_t* d_keys, int64_t n, int64_t* removed_out);
int32_t dsa_mat_delete_batch(dsa_mat_t* h, int32_t orientation, const int64_t* keys, int64_t n, int64_t* removed_out);
/* dropzeros! / droptol! (csrc/droptol.hip): every small stored entry leaves the matrix in place, in one device pass.  No reference
 * counterpart as a bulk call — SparseArrays' dropzeros! / droptol! for a SparseMatrixCSC; it replaces one setindex! with a zero per
 * cell (src/matrix.jl:43-62).  A cell (i, j) with stored value v is DROPPED iff |v| <= tol, or rtol is given and |v| <= rtol[i - 1],
 * or ctol is given and |v| <= ctol[j - 1].  The comparisons are IEEE: a NaN value is never dropped, a NaN or negative threshold
 * matches nothing, +-Inf goes only against a threshold of +Inf, -0.0 counts as zero.  dropzeros! is tol = 0 without vectors; a negative
 * tol is valid and matches nothing (purely relative dropping through the vectors).  rtol or ctol NULL (its length argument is then
 * ignored) means that the vector is absent; when given, nr must equal m and nc must equal n (dsa_mat_size after the queued single
 * writes have been applied).
 * CONTENT, partition tables, size() and the number of partitions afterwards are those of A[i, j] = 0 for every dropped cell in turn:
 * the cell leaves BOTH orientations; a column or row that loses its last cell stays as an empty live partition — no semaphore is
 * ever cleared, with tol = +Inf every cell goes and every partition stays.  The LAYOUT follows the rule of the batched delete:
 * capacity, segment capacity, height and table_len stay, and the survivors of each orientation, in slot order, are spread over
 * [1, capacity] — what dsa_mat_rebalance_root gives (a single-leaf array is not moved).  The call never shrinks; the next write that
 * reaches the root does.
 * When NOTHING is dropped nothing at all changes: no rebalance, no epoch moves (cached SpMV plans survive), the slot arrays keep
 * their bytes.  count_only != 0 evaluates the predicate and modifies nothing.  dropped_out (host pointer, may be NULL) receives the
 * number of matrix entries the predicate drops.  A call that drops something returns with both streams drained.  The same input
 * gives the same bits on every call (no floating-point atomics).
 * Every error is found before the first write — both orientations and the cached SpMV plans stay as they were: DSA_EMODE in fill
 * mode; DSA_EARG: tol is NaN, nr != m or nc != n for a vector that is given; DSA_EBOUNDS: a vector is given and a stored entry lies
 * outside size(m) (the check of dsa_mat_scale; the scalar-only form needs no bounds and works on such a matrix).  Queued single
 * writes are applied first.
 * _dev: d_rtol / d_ctol are device arrays, read on BOTH orientations' streams: they must hold their final contents when the call is
 * made and stay valid and unchanged until it returns (the host waits for the decide pass).  The host form stages rtol and ctol
 * through pooled device memory.  For a handful of cells dsa_mat_set_batch with zeros remains the cheaper call. */
int32_t dsa_mat_droptol_dev(dsa_mat_t* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc,
                            int32_t count_only, int64_t* dropped_out);
int32_t dsa_mat_droptol(dsa_mat_t* h, double tol, const double* rtol, int64_t nr, const double* ctol, int64_t nc,
                        int32_t count_only, int64_t* dropped_out);
/* Update of STORED values in place (csrc/update.hip): A[I[k], J[k]] = V[k] (DSA_UPD_SET) or A[I[k], J[k]] += V[k] (DSA_UPD_ADD, one
 * IEEE add) for n triples, for cells that are already stored.  No reference counterpart as a bulk call: it is setindex!
 * (src/matrix.jl:43-62) restricted to the case in which no cell is created, deleted or moved — a Jacobian or coefficient refresh on a
 * fixed pattern, values computed on the device from exported arrays — and so it does not go through the write planner of
 * dsa_mat_set_batch.  A cell is STORED iff dsa_mat_get_batch finds it: its column and its row are live partitions and hold the key.
 * SET stores V[k] bit for bit (NaN payloads and -0.0 are kept).  V[k] == 0.0 leaves a STORED zero, as dsa_mat_scale does — NOT the
 * reference's delete-on-zero: nnz is unchanged and the cell is still exported; dsa_mat_droptol removes such cells.  A cell addressed
 * by several ops of a SET ends with the value of the LAST of them (the largest k), which is what the ops one after the other leave.
 * ADD must address a stored cell at most once: a second op on it is DSA_EARG (the ordered sum of duplicates is dsa_mat_assemble's).
 * Both orientations end with identical bits in every cell, and the same call on the same state gives the same bits.  Only values
 * are written: keys, occupancy, tables, counts, capacity and the rebalance / extend statistics stay as they are.  Cached SpMV plans
 * are dropped iff at least one value is written.
 * MISSING cells (no live column or row, an empty one, no such key in it): without DSA_UPD_SKIP_MISSING in flags the first of them
 * is DSA_EARG (dsa_last_error names the op) and nothing at all is modified.  With the flag they are skipped, which makes the call
 * the front end of a general write: the caller sends only the misses through dsa_mat_set_batch.  missing[k] (may be NULL) receives
 * 1 for an op without a stored cell, else 0 (its contents are unspecified after an error); *missing_out and *updated_out (host
 * pointers, may be NULL) the number of missing ops and of winning writes (distinct cells written).  A call in which nothing is
 * written changes nothing: no epoch moves, cached plans survive.
 * Every error is found before the first write — both orientations and the cached SpMV plans stay as they were: DSA_EMODE in fill
 * mode; DSA_EARG: op or flags invalid, n < 0, an operand NULL with n > 0, n or a capacity of 2^32 or more, a miss in the strict
 * form, a repeated stored cell under ADD; DSA_EKEY: an I[k] or J[k] of 0, the reserved semaphore key, in both forms (checked on the
 * device: no kernel of this call writes a slot whose key is 0); DSA_EASSERT: a cell found in one orientation and not in the other.
 * n = 0 does nothing.  Queued single writes are applied first.  The number of launches and the one host wait do not depend on n.
 * _dev: d_I / d_J / d_V (and d_missing) are device arrays, read on BOTH orientations' streams: they must hold their final contents
 * when the call is made and stay valid and unchanged until dsa_mat_sync.  The host waits for the verdict only; the stores are
 * enqueued.  The host form stages the triples through pooled device memory and waits for both streams.  For a handful of cells
 * dsa_mat_set_batch remains the cheaper call. */
enum { DSA_UPD_SET = 0, DSA_UPD_ADD = 1 };
enum { DSA_UPD_SKIP_MISSING = 1 };
int32_t dsa_mat_update_values_dev(dsa_mat_t* h, int32_t op, int32_t flags, const int64_t* d_I, const int64_t* d_J, const double* d_V,
                                  int64_t n, uint8_t* d_missing, int64_t* updated_out, int64_t* missing_out);
int32_t dsa_mat_update_values(dsa_mat_t* h, int32_t op, int32_t flags, const int64_t* I, const int64_t* J, const double* V, int64_t n,
                              uint8_t* missing, int64_t* updated_out, int64_t* missing_out);
/* dsa_mat_get_batch with everything in HBM: d_out[k] = A[d_I[k], d_J[k]] (+0.0 for a cell that is not stored), d_found[k] (may be
 * NULL) = 1 iff the cell is stored — it tells a stored 0.0 from an absent cell.  Enqueued on the colmajor stream (dsa_mat_set_stream /
 * dsa_mat_sync); the host does not wait.  A key of 0 reads as absent.  DSA_EMODE in fill mode; DSA_EARG for n < 0 or a NULL operand
 * with n > 0.  Queued single writes are applied first. */
int32_t dsa_mat_get_batch_dev(dsa_mat_t* h, const int64_t* d_I, const int64_t* d_J, int64_t n, double* d_out, uint8_t* d_found);
/* Insert of cells that are NOT STORED yet, in place (csrc/insert.hip): cell (I[k], J[k]) is created with the value V[k], for n
 * triples, in both orientations — the back end of dsa_mat_update_values' DSA_UPD_SKIP_MISSING.  No reference counterpart as a bulk
 * call.  Afterwards the content, the partition tables as a key -> cells map, nnz and size(m) are those of dsa_mat_set_batch(I, J, V)
 * with the same nonzero triples; V[k] is stored bit for bit (NaN payloads, -0.0), and V[k] == 0.0 creates a STORED zero, as
 * dsa_mat_update_values leaves them: it counts in nnz, raises size(m) like any stored cell, and dsa_mat_droptol removes it.
 * LAYOUT: not the one the writes one after the other leave.  Per orientation the merged cell sequence — old cells and semaphores, new
 * cells, the semaphores of the new partitions, in key order — is spread over [1, capacity] the way dsa_mat_rebalance_root spreads it,
 * as the batched delete does.  The capacity is the current one doubled the fewest times (possibly none) that lets the merged count
 * fit the root's upper density bound; each doubling changes the geometry as the reference's _extend! does (src/pma.jl:143-151:
 * capacity and segments doubled, one more level, the segment size kept).  The call never shrinks.
 * WHERE a new cell may go: into any live partition (in front of its first cell, between two, behind its last), or into a NEW
 * partition whose key is greater than the key of the last table entry, which must be live (an empty table takes any keys).  New
 * partitions get the ids table_len + 1 ... in key order.  Tombstones elsewhere in the table stay.  A new partition that would land in
 * the middle of the table is DSA_EMODE ("use set_batch"): it would shift ids, and the reference can refuse it.
 * Every error is found before the first write — both orientations, the tables, every epoch and the cached SpMV plans stay as they
 * were: DSA_EMODE in fill mode or for a partition in the middle; DSA_EKEY: an I[k] or J[k] below 1; DSA_EARG: unknown flags, n < 0,
 * an operand NULL with n > 0, n or a capacity of 2^31 or more, the same cell twice in the batch (dsa_last_error names the later
 * op), a cell that is already stored (names the op); DSA_EASSERT: the orientations disagree about the stored ops, or a live table
 * entry without a semaphore.  With DSA_INS_SKIP_EXISTING in flags a stored cell is skipped instead: existing[k] (may be NULL) receives
 * 1 for it and 0 for an inserted op (unspecified after an error).  n = 0, or every op skipped, changes nothing: no rebalance, no
 * epoch, plans survive.  Otherwise content and layout epochs move once and the plans are dropped once.  A key beyond Int32 widens
 * the orientation's keys first.  Queued single writes are applied first.  The number of launches and of host waits does not depend
 * on n.
 * _dev: d_I / d_J / d_V (and d_existing) are device arrays, read on BOTH orientations' streams: they must hold their final contents
 * when the call is made and stay valid and unchanged until it returns (it returns with both streams drained).  The host form stages
 * the triples through pooled device memory. */
enum { DSA_INS_SKIP_EXISTING = 1 };
int32_t dsa_mat_insert_batch_dev(dsa_mat_t* h, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int32_t flags,
                                 uint8_t* d_existing);
int32_t dsa_mat_insert_batch(dsa_mat_t* h, const int64_t* I, const int64_t* J, const double* V, int64_t n, int32_t flags,
                             uint8_t* existing);
/* The general write from triples (csrc/assemble.hip): ANY n triples — cells stored or not, repeated or not, in any order — in three
 * steps that never leave HBM.  op is DSA_UPD_SET or DSA_UPD_ADD.
 * 1. FOLD to the distinct cells (I[k], J[k]).  SET: the cell's value is the V of the op with the largest k, bit for bit (NaN payloads,
 *    -0.0).  ADD: s = V[k1]; s = s + V[k2]; ... over the cell's ops in ascending k, one IEEE add each — no FMA, no tree, no atomics:
 *    the left fold of dynamicsparse over duplicates (src/pcsr.jl:374-375).  A cell with one op keeps the bits of its V.
 * 2. STORED cells are written in place as by dsa_mat_update_values: SET stores the folded value, ADD stores stored + s (one more
 *    IEEE add).  No slot moves.
 * 3. Cells that are NOT STORED are created with the folded value as by dsa_mat_insert_batch: its layout (merged and spread as
 *    dsa_mat_rebalance_root spreads, never shrunk), its capacity rule, its table rules.  A zero, or a sum that cancels, is a STORED
 *    zero as everywhere in these calls; dsa_mat_droptol removes it.
 * As algebra: ADD is A <- A + sparse(I, J, V) in place; SET is dsa_mat_set_batch of nonzero triples with the layout of
 * dsa_mat_insert_batch.  *distinct_out = *updated_out + *inserted_out (host pointers, may be NULL): the distinct cells, those written
 * in place, those created.  Both orientations end with identical bits per cell; the same call on the same state gives the same
 * bytes.  The content epoch moves once, and cached SpMV plans are dropped, iff something is written; the layout epoch moves iff a
 * cell is created.  size(m) covers every cell of the batch afterwards, a stored one too, as after setindex!.  n = 0 changes nothing.
 * Queued single writes are applied first.
 * Every error is found before the first write — layouts, tables, epochs and plans stay as they were: DSA_EMODE in fill mode;
 * DSA_EARG: op invalid, n < 0, an operand NULL with n > 0, n > 2^31 - 1; DSA_EKEY: an I[k] or J[k] below 1, in any op, also one that
 * a later op overrides; DSA_EMODE: a new column or row that is not behind the last live entry of its table (dsa_mat_insert_batch's
 * limit: "use set_batch"); DSA_EASSERT: the two halves disagree about what is stored.  Where dsa_last_error names an op it is an op
 * of THIS batch — the last one on the cell, which is named too — never an index into the folded list.
 * Scratch: one block on the handle, grown on demand and kept until the handle is destroyed: about 82 bytes per op (the pair sort 32,
 * the sorted index and keys 20, the folded cells with the index of their last op 28, flags, queue, tile counts and mask 2; the
 * compacted misses take the place of the sort's buffers), besides the scratch of the two halves for the distinct cells.  The number
 * of launches does not depend on n; the host waits for the key scan, the distinct-cell count, the update's verdict and, when cells
 * are created, the insert's key scan and verdicts.
 * _dev: d_I / d_J / d_V are device arrays, read only by the fold, on the colmajor stream: they must hold their final contents when
 * the call is made and stay unchanged until it returns (it does not return before the fold has finished).  When only stored cells are
 * written the stores may still be enqueued (dsa_mat_sync); when cells are created the call returns with both streams drained.  The
 * host form stages the triples through pooled device memory and waits for both streams. */
int32_t dsa_mat_assemble_dev(dsa_mat_t* h, int32_t op, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n,
                             int64_t* distinct_out, int64_t* updated_out, int64_t* inserted_out);
int32_t dsa_mat_assemble(dsa_mat_t* h, int32_t op, const int64_t* I, const int64_t* J, const double* V, int64_t n,
                         int64_t* distinct_out, int64_t* updated_out, int64_t* inserted_out);
/* ---- column-range shards. No reference counterpart: the reference is single-process.  One PROCESS per GPU:
 * each process selects its device (dsa_set_device), builds ITS shard and runs the local SpMV; the single data-path collective —
 * the all-reduce (sum) of the partial y — is dsa_shard_allreduce_dev below (RCCL behind this ABI), or whatever the host layer has
 * (torch.distributed in bench.py / sharding.py).
 * dsa_shard_range: shard g of G owns the global column keys (col0, col0 + ncols].
 * dsa_shard_create_from_coo: the triples of the shard's range as an independent reference-layout matrix (own capacity, height,
 *   semaphores, column table; both orientations) with LOCAL column keys 1..ncols; size m x ncols.  n = global column count.
 * dsa_shard_spmv_dev: y_partial = A[:, range] * x[range]; d_x_local = the shard's slice of x (ncols doubles), d_y_partial = m
 *   doubles, both in HBM; asynchronous on the handle's stream (dsa_mat_set_stream / dsa_mat_sync). */
int32_t dsa_shard_range(int64_t n, int32_t nshards, int32_t shard, int64_t* col0, int64_t* ncols);
int32_t dsa_shard_create_from_coo(const int64_t* I, const int64_t* J, const double* V, int64_t nnz, int64_t m, int64_t n,
                                  int32_t nshards, int32_t shard, dsa_mat_t** out);
int32_t dsa_shard_spmv_dev(dsa_mat_t* shard, const double* d_x_local, int64_t nx, double* d_y_partial, int64_t ny);
/* ---- the one data-path collective: the sum of the partial y over the ranks, RCCL over xGMI, behind the ABI.
 * One process per GPU.  Rank 0 calls dsa_comm_unique_id and hands the 128 bytes to the other ranks by whatever means the host has
 * (MPI.Bcast from Julia, a file, torch.distributed); then EVERY rank calls dsa_comm_init (collective: ncclCommInitRank on the
 * current device).  librccl.so is bound at run time; a copy already mapped into the process is reused.
 * dsa_shard_allreduce_dev: in place, y <- sum over ranks (ncclAllReduce, ncclDouble, ncclSum), asynchronous on hip_stream.
 * dsa_shard_spmv_allreduce_dev: dsa_shard_spmv_dev + that all-reduce on the shard's stream = y = A x of the whole matrix on every
 * rank.  id == NULL with nranks == 1: a communicator without RCCL (single GPU); with an id a real single-rank RCCL communicator. */
#define DSA_COMM_ID_BYTES 128
typedef struct dsa_comm dsa_comm_t;
int32_t dsa_comm_unique_id(uint8_t id[DSA_COMM_ID_BYTES]);
int32_t dsa_comm_init(int32_t rank, int32_t nranks, const uint8_t id[DSA_COMM_ID_BYTES], dsa_comm_t** out);
int32_t dsa_comm_destroy(dsa_comm_t* comm);
int32_t dsa_comm_info(dsa_comm_t* comm, int32_t* rank, int32_t* nranks);
int32_t dsa_shard_allreduce_dev(dsa_comm_t* comm, double* d_y, int64_t m, void* hip_stream);
int32_t dsa_shard_spmv_allreduce_dev(dsa_mat_t* shard, dsa_comm_t* comm, const double* d_x_local, int64_t nx, double* d_y, int64_t ny);
/* Device-side invariant checker (the structural checks of the reference's test/utils.jl:68-113, runnable at full size):
 * report[0] occupied cells, [1] semaphore cells, [2] semaphore cells whose table entry does not point back, [3] key-order
 * violations, [4] bad table entries (not pointing at their semaphore / dead key / unsorted column keys), [5] occupancy bits at or
 * beyond the capacity, [6] 1 if report[0] != nb_elements or report[1] != live partitions.  A healthy structure has [2..6] == 0. */
int32_t dsa_vec_check(dsa_vec_t* h, int64_t report[8]);
int32_t dsa_mat_check(dsa_mat_t* h, int32_t orientation, int64_t report[8]);
int32_t dsa_pcsc_check(dsa_pcsc_t* h, int64_t report[8]);
/* stream control for *_dev entry points (hipStream_t passed as void*; NULL = legacy default stream) */
int32_t dsa_mat_set_stream(dsa_mat_t* h, void* hip_stream);
int32_t dsa_vec_set_stream(dsa_vec_t* h, void* hip_stream);
int32_t dsa_mat_sync(dsa_mat_t* h);
int32_t dsa_vec_sync(dsa_vec_t* h);
/* How the blocking entry points of a handle wait for the device.  No reference counterpart (the reference never waits for anything).
 * DSA_WAIT_SPIN (default): the calling thread polls a word in pinned memory that the last kernel of the launch writes — lowest
 * latency, one host core busy for the duration.  DSA_WAIT_BLOCK: the thread is parked in hipStreamSynchronize first — for hosts that
 * multiplex many tasks on few threads (a Julia process driving Coluna).  Results are identical; DSA_WAIT_POLICY=1 in the environment
 * makes DSA_WAIT_BLOCK the default of new handles. */
enum { DSA_WAIT_SPIN = 0, DSA_WAIT_BLOCK = 1 };
int32_t dsa_vec_set_wait_policy(dsa_vec_t* h, int32_t policy);
int32_t dsa_mat_set_wait_policy(dsa_mat_t* h, int32_t policy);
/* The library keeps freed HBM blocks (slot buffers, tables, build scratch) for reuse — up to DSA_POOL_MAX_MB (default 16384) of idle
 * memory per process.  dsa_pool_idle_bytes reports how much is idle right now, dsa_pool_trim releases idle blocks (largest first)
 * until at most keep_bytes remain: what a host that shares the card with another allocator calls before that one runs short. */
int32_t dsa_pool_idle_bytes(int64_t* bytes);
int32_t dsa_pool_trim(int64_t keep_bytes);
/* Release configuration.  The library has development switches (environment variables DSA_TIGHT, DSA_PARBATCH, DSA_MODEL3, ... that
 * select alternative — parity-tested, slower or instrumented — code paths for A/B runs and fault injection).  A release process IGNORES
 * all of them: they are honoured only when DSA_DEV=1 is set in the environment (or the library was built with -DDSA_DEV).  What stays
 * configurable without it is not a code-path switch: DSA_POOL_MAX_MB, DSA_RCCL_LIB, DSA_WAIT_POLICY, DSA_ROCTX.
 * dsa_dev_switches: the space-separated table of switch names (cap >= 1024 suffices) and whether this process honours them. */
int32_t dsa_dev_switches(char* buf, int64_t cap, int32_t* enabled);

/* ---- parity hooks and snapshots (no reference counterpart as entry points; the primitives they run are the reference's) ----
 * dsa_dbg_raw_*: ONE slot-array primitive of src/finds.jl / src/writes.jl / src/moves.jl executed by the DEVICE code on a
 * caller-supplied raw slot array (keys[i], vals[i], occ[i] in {0,1}, i < len; any length, any content) — the form the reference's
 * own unit tests use (test/unit/finds.jl:4-107, test/unit/writes.jl:5-70).  Arrays are uploaded, the kernel runs, the arrays (and
 * semaphores[], if given) are downloaded again.  engine selects which device implementation runs:
 *   DSA_DBG_ENGINE_BLOCK  the write sequencer's workgroup primitives (d_find / d_find_fast, d_insert_after + blk_shift_*, blk_purge,
 *                         blk_rebalance_small: windows <= 8192 slots)
 *   DSA_DBG_ENGINE_WAVE   the wave-level primitives of the batch-parallel rounds (pb_shift_*, pb_wave_rebalance: windows <= 2048 slots)
 *   DSA_DBG_ENGINE_GRID   the grid-wide rebalance kernel k_move2 (dsa_dbg_raw_rebalance only; windows of whole 64-slot words)
 *   DSA_DBG_ENGINE_GRID_WINDOW  the same kernel as the write path launches it (dsa_dbg_raw_rebalance only; windows of whole 64-slot
 *                         words): an interior window is packed into the scratch buffer and spread back from there (two launches, the
 *                         second on a packed source), the window [1, len] is rebalanced at the root, an empty window has its bitmap cleared
 * fast = 0: K-find replays the reference bisection probe for probe; fast = 1: its wave-parallel 64-ary form, which the write paths
 * use wherever the searched range is key-partitioned (only then are the two required to agree). */
enum { DSA_DBG_ENGINE_BLOCK = 0, DSA_DBG_ENGINE_WAVE = 1, DSA_DBG_ENGINE_GRID = 2, DSA_DBG_ENGINE_GRID_WINDOW = 3 };
/* find(array, key, from, to)  src/finds.jl:29-57 -> (pos, elem) ; *has = 0 <=> elem === nothing */
int32_t dsa_dbg_raw_find(const int64_t* keys, const double* vals, const uint8_t* occ, int64_t len, int64_t key, int64_t from, int64_t to,
                         int32_t engine, int32_t fast, int64_t* pos, int32_t* has, int64_t* fkey, double* fval);
/* insert!(array, key, value, from, to, semaphores)  src/writes.jl:14-43 ; sems may be NULL ; DSA_EFULL as the reference's error */
int32_t dsa_dbg_raw_insert(int64_t* keys, double* vals, uint8_t* occ, int64_t len, int64_t key, double value, int64_t from, int64_t to,
                           int64_t* sems, int64_t nsems, int32_t engine, int32_t fast, int64_t* pos, int32_t* is_new);
/* delete!(array, key, from, to)  src/writes.jl:57-68 */
int32_t dsa_dbg_raw_delete(int64_t* keys, double* vals, uint8_t* occ, int64_t len, int64_t key, int64_t from, int64_t to,
                           int32_t engine, int32_t fast, int64_t* pos, int32_t* deleted);
/* purge!(array, from, to)  src/writes.jl:80-91 -> (mid, number of cells deleted) */
int32_t dsa_dbg_raw_purge(int64_t* keys, double* vals, uint8_t* occ, int64_t len, int64_t from, int64_t to, int64_t* mid, int64_t* nb);
/* pack! + spread! of the window [ws, we] (its cell count is taken from occ)  src/moves.jl:94-171 ; with sems: the semaphore-aware
 * spread! (:142-171).  Windows lie inside one occupancy word or consist of whole words, like every window the density scan yields. */
int32_t dsa_dbg_raw_rebalance(int64_t* keys, double* vals, uint8_t* occ, int64_t len, int64_t ws, int64_t we, int64_t* sems, int64_t nsems,
                              int32_t engine);
/* Handles restored from an exported layout (the inverse of dsa_vec_export_layout / dsa_pcsc_export_layout: snapshot / restore, and
 * the way a test puts a structure into an arbitrary state).  capacity and segment_capacity are powers of two (segment_capacity is
 * state, not a function of the capacity: SURVEY App. A.1); nb_segments, height and the density thresholds follow as in
 * src/pma.jl:42-49,143-161; nb_elements = number of occupied slots; semaphores[id] = slot of the cell (0, id) or 0 (tombstone). */
int32_t dsa_vec_import_layout(const int64_t* keys, const double* vals, const uint8_t* occ, int64_t capacity, int64_t segment_capacity,
                              int64_t len, dsa_vec_t** out);
int32_t dsa_pcsc_import_layout(const int64_t* keys, const double* vals, const uint8_t* occ, int64_t capacity, int64_t segment_capacity,
                               const int64_t* semaphores, int64_t table_len, dsa_pcsc_t** out);

#ifdef __cplusplus
}
#endif
#endif /* DSA_H */
