// csrc/vecops.h — what vecops.hip (kernels) and vecops_host.hip (host side) share: the shape of the two-stage whole-vector
// reductions, the terms they are instantiated for, the scratch and pinned words of a call, and the launch wrappers.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// ---- the shape of a reduction over the packed cells of a vector (dsa_vec_reduce, dsa_vec_dot, dsa_vec_dot_dense_dev)
// stage 1: one lane per packed cell of the driving operand, VO_BLOCK threads per workgroup, one partial per wave of 64 cells
// stage 2: ONE workgroup of VO_FIN_THREADS threads; thread t joins the partials t, t + VO_FIN_THREADS, ... in that order (one pass
//          of the workgroup per VO_FIN_THREADS partials), then the threads are joined in a fixed tree
constexpr int VO_BLOCK = 256;
constexpr int VO_FIN_THREADS = 1024;
// cells of the driving operand one pass of stage 2 covers: from VO_PASS_CELLS + 1 cells on a thread of stage 2 joins two partials
constexpr int64_t VO_PASS_CELLS = (int64_t)VO_FIN_THREADS * 64;

// the term of a lane.  The first four are the DSA_RED_* values of include/dsa.h (sum, sum |v|, sum v*v, max |v|).
enum VoTerm : int32_t {
    VO_SUM = 0, VO_ABSSUM = 1, VO_SQSUM = 2, VO_ABSMAX = 3,
    VO_DOT = 5,           // a_k * b_k for the keys of the driving operand the other operand stores (bisection), +0.0 for the others
    VO_DOT_DENSE = 6,     // v_k * x[k - 1]; a key outside 1..nx sets the bounds bit
    VO_BOUNDS = 7         // +0.0; a key outside 1..nx sets the bounds bit (the check in front of a densify)
};

// pinned words of a call (Pma::sc of the vector whose stream runs it): the result's bits, the error word (bit 0: a key outside
// 1..nx), the first packed key (dsa_mat_mul_vec), the sequence number
constexpr int VO_PIN_RESULT = 0, VO_PIN_ERR = 1, VO_PIN_FIRST = 2, VO_PIN_SEQ = 3, VO_PIN_WORDS = 4;
// pooled scratch of a reduction over n driving cells: 64 B header {result, error word}, then one partial per wave
inline int64_t vo_partials(int64_t n) { return (n + 63) / 64; }
inline size_t vo_scratch_bytes(int64_t n) { return 64 + (size_t)vo_partials(n) * sizeof(double); }

// both stages of one reduction, enqueued on `stream`: the driving operand (ka, va, na), the looked-up operand of VO_DOT (kb, vb, nb),
// the dense operand of VO_DOT_DENSE / the bound of VO_BOUNDS (xd, nx).  The result's bits and the error word go to scratch[0..1] and
// to pin[VO_PIN_RESULT], pin[VO_PIN_ERR]; pin[VO_PIN_SEQ] = seq is published last.  na == 0 is legal (+0.0).
hipError_t launch_vec_reduce(int32_t term, KeyArr ka, const double* va, int64_t na, KeyArr kb, const double* vb, int64_t nb,
                             const double* xd, int64_t nx, void* scratch, unsigned long long* pin, unsigned long long seq,
                             hipStream_t stream);
// packed cells -> int64 keys + values (any physical key width).  pin != nullptr: the first key goes to pin[VO_PIN_FIRST] and
// pin[VO_PIN_SEQ] = seq is published behind it (by the thread that copies cell 0).
hipError_t launch_vec_copy_out(KeyArr k, const double* v, int64_t n, int64_t* out_k, double* out_v, unsigned long long* pin,
                               unsigned long long seq, hipStream_t stream);
// x[key - 1] = value for n packed cells whose keys are known to lie in 1..nx
hipError_t launch_vec_scatter(KeyArr k, const double* v, int64_t n, double* x, int64_t nx, hipStream_t stream);

}  // namespace dsa
