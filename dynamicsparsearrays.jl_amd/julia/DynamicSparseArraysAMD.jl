# DynamicSparseArraysAMD.jl — Julia host module over libdsa_hip.so (include/dsa.h).
#
# Drop-in for the PMA / PCSR hot path of DynamicSparseArrays.jl under Coluna: the same exported names
# (reference src/DynamicSparseArrays.jl:5-16), every method a thin `ccall` into the C-ABI HIP shim.
# The shim fixes K = L = Int64, T = Float64 (SURVEY.md §8b); this file carries the part of the contract
# that cannot cross a C ABI:
#   * the KEY-MAPPING LAYER: containers are parametric in their key types like the reference's
#     (`DynamicSparseVector{K}`, `DynamicSparseMatrix{K,L}`); every key crosses the ABI through
#     `keyint(k)::Int64` (order-preserving: the library keeps partitions and cells in Int64 order, the
#     reference in `isless` order of K) and comes back through `keyfrom(K, i)`.  Methods exist for the
#     Integer types and for `Char` (test/functional/sparsematrix.jl:302-336); an id struct (Coluna's
#     VarId / ConstrId) needs two one-line methods, or only `keyint` — then the container remembers
#     the keys it has been given (`KeyMap.seen`) to translate results back;
#   * arbitrary `combine` functions: `+`, `*` and "last" run in the library, anything else is folded
#     here, left to right in input order, before the call (src/vector.jl:10-36, src/pcsr.jl:365-398).
# NOTE: there is no Julia toolchain in the build image, so this file has not been executed; the ABI
# itself is exercised through the Python mirror (dynamicsparsearrays.jl_amd/api.py) by tests/, and
# tests/test_library_symbols.py checks every `ccall` below against include/dsa.h.
module DynamicSparseArraysAMD

using SparseArrays
using LinearAlgebra: Transpose
import LinearAlgebra

export DynamicSparseVector, DynamicSparseMatrix, DynamicMatrixColView, PackedCSC, dynamicsparsevec, dynamicsparse, nbpartitions,
       deletecolumn!, deleterow!, deletecolumns!, deleterows!, deletepartition!, addrow!, closefillmode!, shrink_size!, set_device!, shard_range, dynamicsparse_shard, comm_unique_id, ShardComm, shard_allreduce!,
       shard_spmv_allreduce!, set_wait_policy!, WAIT_SPIN, WAIT_BLOCK, pool_idle_bytes, pool_trim!,
       keyint, keyfrom, col_view_dev!, row_view_dev!, spmv_sparse_dev!, dynamicsparse_dev, dynamicsparse_compressed_dev,
       scale!, reduce_rows, reduce_cols, mul_rows, mul_cols, mul_sparse, dropzeros!, droptol!, count_droptol,
       update_values!, add_values!, getstored, insert_values!, upsert!, assemble!,
       mul_vec, axpby_vec, dynamicsparsevec_dev, nonzeros_dev!, to_dense_dev!

const libdsa = get(ENV, "DSA_HIP_LIB", joinpath(@__DIR__, "..", "csrc", "libdsa_hip.so"))

# status codes of include/dsa.h -> the exception type the reference throws at the same site
const DSA_OK = Int32(0)
function _check(rc::Int32)
    rc == DSA_OK && return
    msg = unsafe_string(ccall((:dsa_last_error_message, libdsa), Cstring, ()))
    rc == 1 && throw(ArgumentError(msg))          # DSA_EARG
    rc == 9 && throw(ArgumentError(msg))          # DSA_EKEY (0 is the semaphore key)
    rc == 2 && throw(BoundsError(msg))            # DSA_EBOUNDS
    error(msg)                                    # ErrorException: EDELETED, EFULL, EMODE, EASSERT, EHIP, ECAP
end

const COMBINE = IdDict{Function,Int32}(+ => Int32(0), * => Int32(1))
const COMBINE_LAST = Int32(2)

"one process per GPU: select the device before creating handles (dsa_set_device)"
set_device!(dev::Integer) = _check(ccall((:dsa_set_device, libdsa), Int32, (Int32,), dev))
"idle HBM the library's caching allocator holds for reuse — dsa_pool_idle_bytes"
function pool_idle_bytes()
    out = Ref{Int64}(0)
    _check(ccall((:dsa_pool_idle_bytes, libdsa), Int32, (Ptr{Int64},), out))
    return out[]
end
"release idle HBM blocks until at most `keep_bytes` remain — dsa_pool_trim"
pool_trim!(keep_bytes::Integer = 0) = _check(ccall((:dsa_pool_trim, libdsa), Int32, (Int64,), keep_bytes))
"(names, enabled): the library's development switches and whether this process honours them (only with ENV[\"DSA_DEV\"] = \"1\") — dsa_dev_switches"
function dev_switches()
    buf = Vector{UInt8}(undef, 2048); on = Ref{Int32}(0)
    _check(ccall((:dsa_dev_switches, libdsa), Int32, (Ptr{UInt8}, Int64, Ref{Int32}), buf, 2048, on))
    return split(unsafe_string(pointer(buf))), on[] != 0
end
const WAIT_SPIN = Int32(0)      # blocking calls poll a pinned word (lowest latency, one core busy)
const WAIT_BLOCK = Int32(1)     # blocking calls park in hipStreamSynchronize first (a Julia process that runs many tasks)
function device_count()
    n = Ref{Int32}(0)
    _check(ccall((:dsa_device_count, libdsa), Int32, (Ref{Int32},), n))
    return n[]
end

"column keys (col0, col0 + ncols] owned by shard `shard` (0-based) of `nshards` — dsa_shard_range"
function shard_range(n::Integer, nshards::Integer, shard::Integer)
    c0 = Ref{Int64}(0); nc = Ref{Int64}(0)
    _check(ccall((:dsa_shard_range, libdsa), Int32, (Int64, Int32, Int32, Ref{Int64}, Ref{Int64}), n, nshards, shard, c0, nc))
    return c0[], nc[]
end

# ------------------------------------------------------------------ key mapping  (SURVEY.md §8b)
"`keyint(k)::Int64`: the key as it crosses the C ABI.  Must preserve the order of `isless` on the key type; 0 is the semaphore key of matrices (src/pcsr.jl:23)."
keyint(k::Integer) = Int64(k)
keyint(k::Char) = Int64(codepoint(k))
"`keyfrom(K, i)`: inverse of `keyint`.  Optional for user types: without it a container translates through the keys it has seen."
keyfrom(::Type{K}, i::Int64) where {K<:Integer} = K(i)
keyfrom(::Type{Char}, i::Int64) = Char(i)

struct KeyMap{K}
    seen::Union{Nothing,Dict{Int64,K}}            # nothing: keyfrom(K, i) exists
end
KeyMap{K}() where {K} = KeyMap{K}(hasmethod(keyfrom, Tuple{Type{K},Int64}) ? nothing : Dict{Int64,K}())
function _in(km::KeyMap{K}, k) where {K}
    kk = convert(K, k)
    i = keyint(kk)::Int64
    km.seen === nothing || (km.seen[i] = kk)
    return i
end
_in(km::KeyMap{K}, ks::AbstractVector) where {K} = Int64[_in(km, k) for k in ks]
_out(km::KeyMap{K}, i::Int64) where {K} = km.seen === nothing ? keyfrom(K, i) : km.seen[i]
_out(km::KeyMap{K}, is::Vector{Int64}) where {K} = K[_out(km, i) for i in is]

# duplicates of a key (vector) or of a (partition, key) pair folded left to right in input order with an arbitrary `combine`;
# returns the order-preserving selection of first occurrences with the folded values (src/vector.jl:10-36)
function _prefold(keys::Vector{NTuple{N,Int64}}, V::Vector{Float64}, combine::Function) where {N}
    first_at = Dict{NTuple{N,Int64},Int}()
    keep = Int[]; vals = Float64[]
    for k in eachindex(keys)
        j = get(first_at, keys[k], 0)
        if j == 0
            push!(keep, k); push!(vals, V[k]); first_at[keys[k]] = length(keep)
        else
            vals[j] = combine(vals[j], V[k])
        end
    end
    return keep, vals
end

# ------------------------------------------------------------------ vector  (reference src/vector.jl)
mutable struct DynamicSparseVector{K} <: AbstractSparseVector{Float64,K}
    h::Ptr{Cvoid}
    keys::KeyMap{K}
    function DynamicSparseVector{K}(h::Ptr{Cvoid}, km::KeyMap{K} = KeyMap{K}()) where {K}
        v = new{K}(h, km)
        finalizer(x -> ccall((:dsa_vec_destroy, libdsa), Int32, (Ptr{Cvoid},), x.h), v)
        return v
    end
end

"how the blocking calls of `v` wait for the device: WAIT_SPIN (default) or WAIT_BLOCK — dsa_vec_set_wait_policy"
set_wait_policy!(v::DynamicSparseVector, policy::Integer) =
    _check(ccall((:dsa_vec_set_wait_policy, libdsa), Int32, (Ptr{Cvoid}, Int32), v.h, policy))

function dynamicsparsevec(I::AbstractVector{K}, V::AbstractVector, combine::Function = +, n::Integer = -1) where {K}
    length(I) == length(V) || throw(ArgumentError("keys & nonzeros vectors must have same length."))
    km = KeyMap{K}()
    Ii = _in(km, I); Vf = Vector{Float64}(V)
    op = get(COMBINE, combine, COMBINE_LAST)
    if !haskey(COMBINE, combine)       # arbitrary combine: fold duplicates here; the library then sees distinct keys
        keep, Vf = _prefold([(i,) for i in Ii], Vf, combine)
        Ii = Ii[keep]
    end
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Ii Vf _check(ccall((:dsa_vec_create, libdsa), Int32,
        (Ptr{Int64}, Ptr{Float64}, Int64, Int32, Int64, Ref{Ptr{Cvoid}}), Ii, Vf, length(Ii), op, Int64(n), out))
    return DynamicSparseVector{K}(out[], km)
end
dynamicsparsevec(I::AbstractVector, V::AbstractVector, n::Integer) = dynamicsparsevec(I, V, +, n)
function dynamicsparsevec(::Type{K}, ::Type{Float64}) where {K}
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_vec_create_empty, libdsa), Int32, (Ref{Ptr{Cvoid}},), out))
    return DynamicSparseVector{K}(out[])
end

function Base.getindex(v::DynamicSparseVector, key)
    out = Ref{Float64}(0.0)
    _check(ccall((:dsa_vec_get, libdsa), Int32, (Ptr{Cvoid}, Int64, Ref{Float64}), v.h, _in(v.keys, key), out))
    return out[]
end
function Base.setindex!(v::DynamicSparseVector, value, key)
    _check(ccall((:dsa_vec_set, libdsa), Int32, (Ptr{Cvoid}, Int64, Float64), v.h, _in(v.keys, key), Float64(value)))
    return v
end
"n getindex calls in one ccall"
function getindex_batch(v::DynamicSparseVector, keys::AbstractVector)
    ki = _in(v.keys, keys); out = Vector{Float64}(undef, length(ki))
    GC.@preserve ki out _check(ccall((:dsa_vec_get_batch, libdsa), Int32,
        (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Float64}), v.h, ki, length(ki), out))
    return out
end
"n sequential setindex! calls in one ccall (sequential-equivalent batch)"
function setindex_batch!(v::DynamicSparseVector, keys::AbstractVector, vals::AbstractVector)
    ki = _in(v.keys, keys); vf = Vector{Float64}(vals)
    GC.@preserve ki vf _check(ccall((:dsa_vec_set_batch, libdsa), Int32,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Int64), v.h, ki, vf, length(ki)))
    return v
end
function Base.length(v::DynamicSparseVector)
    out = Ref{Int64}(0); _check(ccall((:dsa_vec_len, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}), v.h, out)); out[]
end
Base.size(v::DynamicSparseVector) = (length(v),)
function SparseArrays.nnz(v::DynamicSparseVector)
    out = Ref{Int64}(0); _check(ccall((:dsa_vec_nnz, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}), v.h, out)); out[]
end
shrink_size!(v::DynamicSparseVector) = _check(ccall((:dsa_vec_shrink_size, libdsa), Int32, (Ptr{Cvoid},), v.h))
function _stored_int(v::DynamicSparseVector)
    n = nnz(v); ks = Vector{Int64}(undef, max(n, 1)); vs = Vector{Float64}(undef, max(n, 1)); m = Ref{Int64}(0)
    GC.@preserve ks vs _check(ccall((:dsa_vec_nonzeros, libdsa), Int32,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}), v.h, ks, vs, length(ks), m))
    return resize!(ks, m[]), resize!(vs, m[])
end
_stored(v::DynamicSparseVector) = ((ks, vs) = _stored_int(v); (_out(v.keys, ks), vs))
SparseArrays.nonzeroinds(v::DynamicSparseVector) = _stored(v)[1]
SparseArrays.nonzeros(v::DynamicSparseVector) = _stored(v)[2]
Base.iterate(v::DynamicSparseVector, st = (zip(_stored(v)...), nothing)) =
    (r = st[2] === nothing ? iterate(st[1]) : iterate(st[1], st[2]); r === nothing ? nothing : (r[1], (st[1], r[2])))

# v1 == v2  (src/vector.jl:85-87): compared on the device, only the verdict comes back
function Base.:(==)(a::DynamicSparseVector{K}, b::DynamicSparseVector{K}) where {K}
    out = Ref{Int32}(0)
    _check(ccall((:dsa_vec_equal, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}), a.h, b.h, out))
    return out[] == 1
end
# v1 + v2, v1 - v2: the SparseVector the AbstractSparseVector fallbacks of the reference produce (test/functional/math.jl:53-94),
# merged on the device.  Mixed operands (SparseVector with DynamicSparseVector) and -v keep using the stdlib fallbacks over
# nonzeroinds / nonzeros above.
function _axpby(a::DynamicSparseVector{K}, alpha::Float64, b::DynamicSparseVector{K}, beta::Float64) where {K<:Integer}
    length(a) == length(b) || throw(DimensionMismatch("dimensions must match"))
    cap = max(nnz(a) + nnz(b), 1); ks = Vector{Int64}(undef, cap); vs = Vector{Float64}(undef, cap); m = Ref{Int64}(0)
    GC.@preserve ks vs _check(ccall((:dsa_vec_axpby, libdsa), Int32,
        (Ptr{Cvoid}, Float64, Ptr{Cvoid}, Float64, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}), a.h, alpha, b.h, beta, ks, vs, cap, m))
    return SparseVector(length(a), K.(resize!(ks, m[])), resize!(vs, m[]))
end
Base.:(+)(a::DynamicSparseVector{K}, b::DynamicSparseVector{K}) where {K<:Integer} = _axpby(a, 1.0, b, 1.0)
Base.:(-)(a::DynamicSparseVector{K}, b::DynamicSparseVector{K}) where {K<:Integer} = _axpby(a, 1.0, b, -1.0)
# ---- the vector as a device operand (include/dsa.h: csrc/vecops_host.hip; Integer keys: a device array holds the mapped integers)
"alpha * a + beta * b as a NEW DynamicSparseVector of length max(length(a), length(b)), built on the device from the pairs a + b / a - b
deliver — dsa_vec_axpby_vec"
function axpby_vec(a::DynamicSparseVector{K}, alpha::Real, b::DynamicSparseVector{K}, beta::Real) where {K<:Integer}
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_vec_axpby_vec, libdsa), Int32, (Ptr{Cvoid}, Float64, Ptr{Cvoid}, Float64, Ref{Ptr{Cvoid}}),
                 a.h, Float64(alpha), b.h, Float64(beta), out))
    return DynamicSparseVector{K}(out[])
end
function _vec_reduce(v::DynamicSparseVector, kind::Integer)
    out = Ref{Float64}(0.0)
    _check(ccall((:dsa_vec_reduce, libdsa), Int32, (Ptr{Cvoid}, Int32, Ref{Float64}), v.h, kind, out))
    return out[]
end
# sum(v), norm(v, p) and dot(v, w) over the stored values, reduced on the device in a fixed order (the bits depend on the stored
# pairs only); only the scalar comes back
Base.sum(v::DynamicSparseVector) = _vec_reduce(v, 0)
function LinearAlgebra.norm(v::DynamicSparseVector, p::Real = 2)
    p == 1 && return _vec_reduce(v, 1)
    p == 2 && return sqrt(_vec_reduce(v, 2))
    p == Inf && return _vec_reduce(v, 3)
    throw(ArgumentError("p must be 1, 2 or Inf"))
end
function LinearAlgebra.dot(a::DynamicSparseVector{K}, b::DynamicSparseVector{K}) where {K}
    out = Ref{Float64}(0.0)
    _check(ccall((:dsa_vec_dot, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}), a.h, b.h, out))
    return out[]
end
"dot(v, x) with a dense x of nx Float64 in HBM (device pointer); BoundsError when v stores a key outside 1..nx — dsa_vec_dot_dense_dev"
function LinearAlgebra.dot(v::DynamicSparseVector, d_x::Ptr{Cvoid}, nx::Integer)
    out = Ref{Float64}(0.0)
    _check(ccall((:dsa_vec_dot_dense_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Float64}), v.h, d_x, nx, out))
    return out[]
end
"the stored pairs in ascending key order into device arrays of `cap` Int64 / Float64; returns their number, stream-ordered on the
vector's stream — dsa_vec_nonzeros_dev"
function nonzeros_dev!(v::DynamicSparseVector, d_keys::Ptr{Cvoid}, d_vals::Ptr{Cvoid}, cap::Integer)
    n = Ref{Int64}(0)
    _check(ccall((:dsa_vec_nonzeros_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Int64}), v.h, d_keys, d_vals, cap, n))
    return n[]
end
"d_x[1:nx] = Vector(v) in HBM (device pointer); BoundsError, d_x untouched, when v stores a key outside 1..nx — dsa_vec_to_dense_dev"
function to_dense_dev!(v::DynamicSparseVector, d_x::Ptr{Cvoid}, nx::Integer)
    _check(ccall((:dsa_vec_to_dense_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), v.h, d_x, nx))
    return v
end
"dynamicsparsevec(I, V, combine, n) with I (Int64) and V (Float64) in HBM (device pointers): + , * and \"last\" (any other function)
fold duplicates in the library — dsa_vec_create_dev"
function dynamicsparsevec_dev(d_keys::Ptr{Cvoid}, d_vals::Ptr{Cvoid}, n::Integer, combine::Function = +, len::Integer = -1)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_vec_create_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int64, Ref{Ptr{Cvoid}}),
                 d_keys, d_vals, n, get(COMBINE, combine, COMBINE_LAST), len, out))
    return DynamicSparseVector{Int64}(out[])
end

# filter(f, v)  (src/vector.jl:83 -> src/pma.jl:224-234): the predicate runs in Julia on the packed entries, the result is a new vector
function Base.filter(f, v::DynamicSparseVector{K}) where {K}
    ks, vs = _stored(v)
    keep = [f((ks[i], vs[i])) for i in eachindex(ks)]
    return dynamicsparsevec(ks[keep], vs[keep])
end

# ------------------------------------------------------------------ matrix  (reference src/matrix.jl)
mutable struct DynamicSparseMatrix{K,L}
    h::Ptr{Cvoid}
    rows::KeyMap{K}
    cols::KeyMap{L}
    function DynamicSparseMatrix{K,L}(h::Ptr{Cvoid}, rk::KeyMap{K} = KeyMap{K}(), ck::KeyMap{L} = KeyMap{L}()) where {K,L}
        m = new{K,L}(h, rk, ck)
        finalizer(x -> ccall((:dsa_mat_destroy, libdsa), Int32, (Ptr{Cvoid},), x.h), m)
        return m
    end
end

"how the blocking calls of `m` wait for the device: WAIT_SPIN (default) or WAIT_BLOCK — dsa_mat_set_wait_policy"
set_wait_policy!(m::DynamicSparseMatrix, policy::Integer) =
    _check(ccall((:dsa_mat_set_wait_policy, libdsa), Int32, (Ptr{Cvoid}, Int32), m.h, policy))

# dynamicsparse(I, J, V[, m, n][, combine])  src/matrix.jl:15-19 -> dynamicsparsecolmajor(J, I, V, combine) src/pcsr.jl:433-445:
# the library folds duplicates of (i, j) with +; any other combine is folded here first
function dynamicsparse(I::AbstractVector{K}, J::AbstractVector{L}, V::AbstractVector, m = -1, n = -1, combine::Function = +) where {K,L}
    length(I) == length(J) == length(V) ||
        throw(ArgumentError("rows, columns, and nonzeros do not have same length."))
    rk = KeyMap{K}(); ck = KeyMap{L}()
    Ii = _in(rk, I); Ji = _in(ck, J); Vf = Vector{Float64}(V)
    if combine !== +
        keep, Vf = _prefold([(Ji[k], Ii[k]) for k in eachindex(Ii)], Vf, combine)
        Ii = Ii[keep]; Ji = Ji[keep]
    end
    mi = m isa Integer && m < 0 ? Int64(-1) : _in(rk, m); ni = n isa Integer && n < 0 ? Int64(-1) : _in(ck, n)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Ii Ji Vf _check(ccall((:dsa_mat_create_from_coo, libdsa), Int32,
        (Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Int64, Ref{Ptr{Cvoid}}), Ii, Ji, Vf, length(Ii), mi, ni, out))
    return DynamicSparseMatrix{K,L}(out[], rk, ck)
end
dynamicsparse(I::AbstractVector, J::AbstractVector, V::AbstractVector, combine::Function) = dynamicsparse(I, J, V, -1, -1, combine)
function dynamicsparse(::Type{K}, ::Type{L}, ::Type{Float64}; fill_mode = true) where {K,L}
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_mat_create_empty, libdsa), Int32, (Int32, Ref{Ptr{Cvoid}}), fill_mode ? 1 : 0, out))
    return DynamicSparseMatrix{K,L}(out[])
end
"`dynamicsparse(I, J, V, m, n)` with the triples already in HBM: `d_I` / `d_J` are device pointers to `nnz` indices of `index_bits` (32 | 64)
counted from `index_base` (0 | 1), `d_V` to `nnz` Float64; integer keys only (key = index + 1 - base).  The arrays must be complete at the call
and are the caller's again when it returns — dsa_mat_create_from_coo_dev"
function dynamicsparse_dev(d_I::Ptr{Cvoid}, d_J::Ptr{Cvoid}, d_V::Ptr{Cvoid}, nnz::Integer, m::Integer = -1, n::Integer = -1;
                           index_bits::Integer = 64, index_base::Integer = 1)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_mat_create_from_coo_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Int64, Int64, Ref{Ptr{Cvoid}}),
                 d_I, d_J, d_V, nnz, index_bits, index_base, m, n, out))
    return DynamicSparseMatrix{Int64,Int64}(out[])
end
"the same from a compressed form in HBM, the conventions of dsa_mat_to_compressed_dev: `orientation` 1 = CSR (outer = rows), 0 = CSC (outer =
columns); `d_ptr` has `outer + 1` entries, `d_idx` / `d_vals` `nnz` — dsa_mat_create_from_compressed_dev"
function dynamicsparse_compressed_dev(orientation::Integer, d_ptr::Ptr{Cvoid}, d_idx::Ptr{Cvoid}, d_vals::Ptr{Cvoid}, outer::Integer, inner::Integer,
                                      nnz::Integer; index_bits::Integer = 64, index_base::Integer = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_mat_create_from_compressed_dev, libdsa), Int32,
                 (Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ref{Ptr{Cvoid}}),
                 orientation, index_bits, index_base, d_ptr, d_idx, d_vals, outer, inner, nnz, out))
    return DynamicSparseMatrix{Int64,Int64}(out[])
end

function Base.setindex!(a::DynamicSparseMatrix, val, row, col)
    _check(ccall((:dsa_mat_set, libdsa), Int32, (Ptr{Cvoid}, Float64, Int64, Int64), a.h, Float64(val), _in(a.rows, row), _in(a.cols, col)))
    return a
end
function setindex_batch!(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector, V::AbstractVector)
    Ii = _in(a.rows, I); Ji = _in(a.cols, J); Vf = Vector{Float64}(V)
    GC.@preserve Ii Ji Vf _check(ccall((:dsa_mat_set_batch, libdsa), Int32,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64), a.h, Ii, Ji, Vf, length(Ii)))
    return a
end
function Base.getindex(a::DynamicSparseMatrix, row, col)
    out = Ref{Float64}(0.0)
    _check(ccall((:dsa_mat_get, libdsa), Int32, (Ptr{Cvoid}, Int64, Int64, Ref{Float64}), a.h, _in(a.rows, row), _in(a.cols, col), out))
    return out[]
end
function addrow!(a::DynamicSparseMatrix, row, colids::AbstractVector, vals::AbstractVector)
    ci = _in(a.cols, colids); vf = Vector{Float64}(vals)
    GC.@preserve ci vf _check(ccall((:dsa_mat_addrow, libdsa), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64), a.h, _in(a.rows, row), ci, vf, length(ci)))
    return true
end
closefillmode!(a::DynamicSparseMatrix) = (_check(ccall((:dsa_mat_closefillmode, libdsa), Int32, (Ptr{Cvoid},), a.h)); true)
deletecolumn!(a::DynamicSparseMatrix, col) = (_check(ccall((:dsa_mat_deletecolumn, libdsa), Int32, (Ptr{Cvoid}, Int64), a.h, _in(a.cols, col))); true)
deleterow!(a::DynamicSparseMatrix, row) = (_check(ccall((:dsa_mat_deleterow, libdsa), Int32, (Ptr{Cvoid}, Int64), a.h, _in(a.rows, row))); true)
# deletecolumn! / deleterow! for a list of keys in one device pass (dsa_mat_delete_batch; no reference counterpart: the content and
# the tables are those of the single calls one after the other, the survivors are spread as by a root rebalance).  The keys in any
# order, distinct, each a live column / row whose mapped key is >= 1; an error leaves the matrix untouched.  Returns the number of
# entries removed.  For one or two keys the single calls are cheaper.
function _delete_batch!(a::DynamicSparseMatrix, orientation::Int32, ki::Vector{Int64})
    out = Ref{Int64}(0)
    GC.@preserve ki _check(ccall((:dsa_mat_delete_batch, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Int64, Ref{Int64}), a.h, orientation, ki, length(ki), out))
    return out[]
end
deletecolumns!(a::DynamicSparseMatrix, cols::AbstractVector) = _delete_batch!(a, Int32(0), _in(a.cols, cols))          # DSA_COLMAJOR
deleterows!(a::DynamicSparseMatrix, rows::AbstractVector) = _delete_batch!(a, Int32(1), _in(a.rows, rows))              # DSA_ROWMAJOR
function SparseArrays.nnz(a::DynamicSparseMatrix)
    out = Ref{Int64}(0); _check(ccall((:dsa_mat_nnz, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}), a.h, out)); out[]
end
# size(A) is the running maximum of the keys written with a non-zero value, as keys (src/matrix.jl:44-47; `size == (5, 'e')`
# at test/functional/sparsematrix.jl:302-336)
function Base.size(a::DynamicSparseMatrix)
    m = Ref{Int64}(0); n = Ref{Int64}(0)
    _check(ccall((:dsa_mat_size, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), a.h, m, n))
    return (_out(a.rows, m[]), _out(a.cols, n[]))
end
Base.size(a::DynamicSparseMatrix, i) = size(a)[i]
function _size_int(a::DynamicSparseMatrix)
    m = Ref{Int64}(0); n = Ref{Int64}(0)
    _check(ccall((:dsa_mat_size, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), a.h, m, n)); (m[], n[])
end
# the stored entries in CSC form, 1-based (dsa_mat_to_compressed over colmajor): integer keys only, as they index 1..size(a)
function _csc_int(a::DynamicSparseMatrix{K,L}) where {K,L}
    (K <: Integer && L <: Integer) || throw(ArgumentError("compressed export needs integer row and column keys, got $(K), $(L)"))
    m, n = _size_int(a)
    cap = nnz(a)
    colptr = Vector{Int64}(undef, n + 1); rowval = Vector{Int64}(undef, cap); nzval = Vector{Float64}(undef, cap)
    got = Ref{Int64}(0)
    GC.@preserve colptr rowval nzval _check(ccall((:dsa_mat_to_compressed, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}), a.h, Int32(0), Int32(1), colptr, rowval, nzval, cap, got))
    return m, n, colptr, rowval[1:got[]], nzval[1:got[]]
end
function SparseArrays.findnz(a::DynamicSparseMatrix)
    _, n, colptr, rowval, nzval = _csc_int(a)
    J = Vector{Int64}(undef, length(rowval))
    for j in 1:n, p in colptr[j]:colptr[j + 1] - 1
        J[p] = j
    end
    return rowval, J, nzval
end
function SparseArrays.SparseMatrixCSC(a::DynamicSparseMatrix)
    m, n, colptr, rowval, nzval = _csc_int(a)
    return SparseMatrixCSC(m, n, colptr, rowval, nzval)
end

function nbpartitions(a::DynamicSparseMatrix, orientation::Integer)     # 0 = colmajor, 1 = rowmajor
    out = Ref{Int64}(0); _check(ccall((:dsa_mat_nbpartitions, libdsa), Int32, (Ptr{Cvoid}, Int32, Ref{Int64}), a.h, orientation, out)); out[]
end

# per-column iteration: DynamicMatrixColView (src/views.jl:3-36).  The reference's view is a lazy cursor over the slot array;
# here the occupied cells of the column's slot range are packed on the device in slot order (K-pack, one launch) and the
# view iterates over that snapshot: `for (row, val) in @view A[:, j]`.
struct DynamicMatrixColView{K,L}
    col_key::L
    rows::Vector{K}
    vals::Vector{Float64}
end
Base.iterate(dv::DynamicMatrixColView, i::Int = 1) = i > length(dv.rows) ? nothing : ((dv.rows[i], dv.vals[i]), i + 1)
Base.length(dv::DynamicMatrixColView) = length(dv.rows)
Base.eltype(::Type{DynamicMatrixColView{K,L}}) where {K,L} = Tuple{K,Float64}

# ccall needs a literal (symbol, library) pair: the four entry points are stamped out with @eval
for (fname, sym) in ((:_col_view, :dsa_mat_col_view), (:_row_view, :dsa_mat_row_view))
    @eval function $fname(a::DynamicSparseMatrix, key::Int64)
        cap = 64
        while true
            ks = Vector{Int64}(undef, cap); vs = Vector{Float64}(undef, cap); n = Ref{Int64}(0)
            rc = GC.@preserve ks vs ccall(($(QuoteNode(sym)), libdsa), Int32,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}), a.h, key, ks, vs, cap, n)
            rc == 8 && (cap *= 8; continue)          # DSA_ECAP
            _check(rc)
            return resize!(ks, n[]), resize!(vs, n[])
        end
    end
end
function Base.view(a::DynamicSparseMatrix{K,L}, ::Colon, col) where {K,L}                     # src/matrix.jl:83-88
    ks, vs = _col_view(a, _in(a.cols, col))
    return DynamicMatrixColView{K,L}(convert(L, col), _out(a.rows, ks), vs)
end
function Base.view(a::DynamicSparseMatrix{K,L}, row, ::Colon) where {K,L}                     # src/matrix.jl:70-81 (fill mode: buffer row)
    ks, vs = _row_view(a, _in(a.rows, row))
    return collect(zip(_out(a.cols, ks), vs))
end

for (fname, sym) in ((:_col_slice, :dsa_mat_col_slice), (:_row_slice, :dsa_mat_row_slice))
    @eval function $fname(a::DynamicSparseMatrix, key::Int64)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        _check(ccall(($(QuoteNode(sym)), libdsa), Int32, (Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), a.h, key, out))
        return out[]
    end
end
"`@view A[:, col]` delivered into HBM: `d_rows` / `d_vals` are device pointers to `cap` Int64 / Float64 entries (mapped key integers, see
keyint); returns the number of cells; the copy is enqueued on the colmajor stream — dsa_mat_col_view_dev (the row form: dsa_mat_row_view_dev)"
function col_view_dev!(a::DynamicSparseMatrix, col, d_rows::Ptr{Cvoid}, d_vals::Ptr{Cvoid}, cap::Integer)
    n = Ref{Int64}(0)
    _check(ccall((:dsa_mat_col_view_dev, libdsa), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Int64}), a.h, _in(a.cols, col), d_rows, d_vals, cap, n))
    return n[]
end
function row_view_dev!(a::DynamicSparseMatrix, row, d_cols::Ptr{Cvoid}, d_vals::Ptr{Cvoid}, cap::Integer)
    n = Ref{Int64}(0)
    _check(ccall((:dsa_mat_row_view_dev, libdsa), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Int64}), a.h, _in(a.rows, row), d_cols, d_vals, cap, n))
    return n[]
end
# A[:, col] / A[row, :]: the new vector is built device to device (view kernel -> one spread launch); nothing but its handle comes back
Base.getindex(a::DynamicSparseMatrix{K,L}, ::Colon, col) where {K,L} = DynamicSparseVector{K}(_col_slice(a, _in(a.cols, col)), a.rows)
Base.getindex(a::DynamicSparseMatrix{K,L}, row, ::Colon) where {K,L} = DynamicSparseVector{L}(_row_slice(a, _in(a.rows, row)), a.cols)

# A[:, cols] / A[rows, :] for a list of keys (dsa_mat_select_compressed, 1-based): the partitions of the listed keys as one compressed
# matrix — any order, repeats allowed, a key without entries gives an empty slice.  Integer keys only, like _csc_int.  The first call
# counts (cap = 0: DSA_ECAP leaves ptr filled and the total in `got`), the second one fetches.
function _select_int(a::DynamicSparseMatrix{K,L}, orientation::Int32, keys::AbstractVector{<:Integer}) where {K,L}
    (K <: Integer && L <: Integer) || throw(ArgumentError("a key-list selection needs integer row and column keys, got $(K), $(L)"))
    sel = Vector{Int64}(keys)
    ptr = Vector{Int64}(undef, length(sel) + 1); idx = Int64[]; val = Float64[]
    got = Ref{Int64}(0)
    for _ in 1:2
        cap = length(idx)
        rc = GC.@preserve sel ptr idx val ccall((:dsa_mat_select_compressed, libdsa), Int32,
            (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}),
            a.h, orientation, Int32(1), sel, length(sel), ptr, cap == 0 ? Ptr{Int64}(C_NULL) : pointer(idx),
            cap == 0 ? Ptr{Float64}(C_NULL) : pointer(val), cap, got)
        if rc == 8 && cap == 0                      # DSA_ECAP
            resize!(idx, got[]); resize!(val, got[])
            continue
        end
        _check(rc)
        break
    end
    return ptr, idx, val
end
function Base.getindex(a::DynamicSparseMatrix{K,L}, ::Colon, cols::AbstractVector{<:Integer}) where {K,L}
    colptr, rowval, nzval = _select_int(a, Int32(0), cols)
    return SparseMatrixCSC(_size_int(a)[1], length(cols), colptr, rowval, nzval)
end
# the rowmajor selection is the CSC of the transpose (one column per selected row)
function Base.getindex(a::DynamicSparseMatrix{K,L}, rows::AbstractVector{<:Integer}, ::Colon) where {K,L}
    rowptr, colval, nzval = _select_int(a, Int32(1), rows)
    return SparseMatrixCSC(transpose(SparseMatrixCSC(_size_int(a)[2], length(rows), rowptr, colval, nzval)))
end
# A[rows, cols] with both key lists (dsa_mat_submatrix_compressed, colmajor, 1-based): the columns `cols` (any order, repeats allowed)
# restricted to the rows `rows` (any order, all distinct: a repeated row key is an ArgumentError) and renumbered on the device, entry
# (i, j) of the result = A[rows[i], cols[j]].  Count-only call first, like _select_int.  The device delivers a column in ascending
# ORIGINAL row key; SparseMatrixCSC wants ascending positions, so the columns are sorted here unless `rows` ascends.
function Base.getindex(a::DynamicSparseMatrix{K,L}, rows::AbstractVector{<:Integer}, cols::AbstractVector{<:Integer}) where {K,L}
    (K <: Integer && L <: Integer) || throw(ArgumentError("a key-list selection needs integer row and column keys, got $(K), $(L)"))
    outer = Vector{Int64}(cols); inner = Vector{Int64}(rows)
    ptr = Vector{Int64}(undef, length(outer) + 1); idx = Int64[]; val = Float64[]
    got = Ref{Int64}(0)
    for _ in 1:2
        cap = length(idx)
        rc = GC.@preserve outer inner ptr idx val ccall((:dsa_mat_submatrix_compressed, libdsa), Int32,
            (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}),
            a.h, Int32(0), Int32(1), outer, length(outer), inner, length(inner), ptr, cap == 0 ? Ptr{Int64}(C_NULL) : pointer(idx),
            cap == 0 ? Ptr{Float64}(C_NULL) : pointer(val), cap, got)
        if rc == 8 && cap == 0                      # DSA_ECAP
            resize!(idx, got[]); resize!(val, got[])
            continue
        end
        _check(rc)
        break
    end
    if !issorted(inner; lt = <=)
        for j in 1:length(outer)
            r = ptr[j]:(ptr[j + 1] - 1)
            p = sortperm(view(idx, r))
            idx[r] = idx[r][p]; val[r] = val[r][p]
        end
    end
    return SparseMatrixCSC(length(inner), length(outer), ptr, idx, val)
end
"n getindex calls in one ccall"
function getindex_batch(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector)
    Ii = _in(a.rows, I); Ji = _in(a.cols, J); out = Vector{Float64}(undef, length(Ii))
    GC.@preserve Ii Ji out _check(ccall((:dsa_mat_get_batch, libdsa), Int32,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}), a.h, Ii, Ji, length(Ii), out))
    return out
end

"the column-range shard `shard` of `nshards` of the matrix given by its triples (local column keys 1..ncols) — one process per GPU"
function dynamicsparse_shard(I::Vector{Int64}, J::Vector{Int64}, V::Vector{Float64}, m::Int64, n::Int64, nshards::Integer, shard::Integer)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve I J V _check(ccall((:dsa_shard_create_from_coo, libdsa), Int32,
        (Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Int64, Int32, Int32, Ref{Ptr{Cvoid}}), I, J, V, length(I), m, n, nshards, shard, out))
    return DynamicSparseMatrix{Int64,Int64}(out[])
end

# ---- the collective of the column-range sharded product: RCCL behind the C ABI (include/dsa.h: dsa_comm_*), one process per GPU.
# Rank 0 calls comm_unique_id() and hands the 128 bytes to the other ranks (MPI.Bcast!, a file, ...); every rank then calls
# ShardComm(rank, nranks, id) — a collective — and shard_spmv_allreduce!(shard, comm, x, y) leaves y = A x on every rank.
"128 opaque bytes identifying a new communicator (ncclUniqueId) — dsa_comm_unique_id"
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    GC.@preserve id _check(ccall((:dsa_comm_unique_id, libdsa), Int32, (Ptr{UInt8},), id))
    return id
end
mutable struct ShardComm
    h::Ptr{Cvoid}
    function ShardComm(rank::Integer, nranks::Integer, id::Union{Nothing,Vector{UInt8}})
        out = Ref{Ptr{Cvoid}}(C_NULL)
        idp = id === nothing ? Ptr{UInt8}(C_NULL) : pointer(id)
        GC.@preserve id _check(ccall((:dsa_comm_init, libdsa), Int32, (Int32, Int32, Ptr{UInt8}, Ref{Ptr{Cvoid}}), rank, nranks, idp, out))
        c = new(out[])
        finalizer(x -> ccall((:dsa_comm_destroy, libdsa), Int32, (Ptr{Cvoid},), x.h), c)
        return c
    end
end
"y (a device pointer to m Float64 in HBM) <- sum over the ranks, in place, asynchronous on `stream` — dsa_shard_allreduce_dev.
`stream` has no default: the shard's product runs on the matrix's own non-blocking stream, which is NOT ordered against the legacy
null stream, so the caller names the stream y was produced on (or uses shard_spmv_allreduce!, which takes the matrix's)."
shard_allreduce!(c::ShardComm, d_y::Ptr{Cvoid}, m::Integer, stream::Ptr{Cvoid}) =
    _check(ccall((:dsa_shard_allreduce_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}), c.h, d_y, m, stream))
"y = A x of the whole sharded matrix on every rank: local product + all-reduce, x / y device pointers — dsa_shard_spmv_allreduce_dev"
shard_spmv_allreduce!(a::DynamicSparseMatrix, c::ShardComm, d_x::Ptr{Cvoid}, nx::Integer, d_y::Ptr{Cvoid}, ny::Integer) =
    _check(ccall((:dsa_shard_spmv_allreduce_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64), a.h, c.h, d_x, nx, d_y, ny))

# ------------------------------------------------------------------ PackedCSC  (reference src/pcsr.jl:4-339)
mutable struct PackedCSC{K}
    h::Ptr{Cvoid}
    keys::KeyMap{K}
    function PackedCSC{K}(h::Ptr{Cvoid}, km::KeyMap{K} = KeyMap{K}()) where {K}
        p = new{K}(h, km)
        finalizer(x -> ccall((:dsa_pcsc_destroy, libdsa), Int32, (Ptr{Cvoid},), x.h), p)
        return p
    end
end
"PackedCSC(row_keys, values, combine): one vector of keys / values per partition (src/pcsr.jl:26-63)"
function PackedCSC(row_keys::Vector{Vector{K}}, values::Vector{<:AbstractVector}, combine::Function = +) where {K}
    length(row_keys) == length(values) || throw(ArgumentError("Must have same number of partitions."))
    km = KeyMap{K}()
    colptr = Int64[0]; keys = Int64[]; vals = Float64[]          # CSC-style offsets (0-based, nparts + 1 entries)
    for (p, (ks, vs)) in enumerate(zip(row_keys, values))
        length(ks) == length(vs) || throw(ArgumentError("Partition $p: keys & values must have same length."))
        ki = _in(km, ks); vf = Vector{Float64}(vs)
        if !haskey(COMBINE, combine)      # arbitrary combine: folded per partition here, the library then sees distinct keys
            keep, vf = _prefold([(i,) for i in ki], vf, combine)
            ki = ki[keep]
        end
        append!(keys, ki); append!(vals, vf); push!(colptr, length(keys))
    end
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve colptr keys vals _check(ccall((:dsa_pcsc_create, libdsa), Int32,
        (Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Int32, Ref{Ptr{Cvoid}}),
        colptr, length(row_keys), keys, vals, get(COMBINE, combine, COMBINE_LAST), out))
    return PackedCSC{K}(out[], km)
end
function PackedCSC(::Type{K}, ::Type{Float64}) where {K}                    # src/pcsr.jl:65-68
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_pcsc_create_empty, libdsa), Int32, (Ref{Ptr{Cvoid}},), out))
    return PackedCSC{K}(out[])
end
function Base.getindex(p::PackedCSC, key, partition::Integer)              # src/pcsr.jl:228-232
    out = Ref{Float64}(0.0)
    _check(ccall((:dsa_pcsc_get, libdsa), Int32, (Ptr{Cvoid}, Int64, Int64, Ref{Float64}), p.h, _in(p.keys, key), Int64(partition), out))
    return out[]
end
function Base.setindex!(p::PackedCSC, value, key, partition::Integer)      # src/pcsr.jl:294-310
    _check(ccall((:dsa_pcsc_set, libdsa), Int32, (Ptr{Cvoid}, Float64, Int64, Int64), p.h, Float64(value), _in(p.keys, key), Int64(partition)))
    return p
end
deletepartition!(p::PackedCSC, partition::Integer) =                          # src/pcsr.jl:188-204
    (_check(ccall((:dsa_pcsc_deletepartition, libdsa), Int32, (Ptr{Cvoid}, Int64), p.h, Int64(partition))); nothing)
function SparseArrays.nnz(p::PackedCSC)
    out = Ref{Int64}(0); _check(ccall((:dsa_pcsc_nnz, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}), p.h, out)); out[]
end
function nbpartitions(p::PackedCSC)
    out = Ref{Int64}(0); _check(ccall((:dsa_pcsc_nbpartitions, libdsa), Int32, (Ptr{Cvoid}, Ref{Int64}), p.h, out)); out[]
end

# ------------------------------------------------------------------ SpMV  (reference src/operations.jl)
struct Transposed{T}; array::T; end
Base.transpose(a::DynamicSparseMatrix) = Transposed(a)
Base.size(t::Transposed) = reverse(size(t.array))

# y = A x for a sparse x given by its stored entries: the touched rows in ascending order (_mul_output, src/operations.jl:11-12);
# Integer output keys -> sparsevec, any other key type -> Dict (the reference returns its accumulator Dict there)
function _spmv_sparse(a::DynamicSparseMatrix, tr::Bool, xi::Vector{Int64}, xv::Vector{Float64}, out_keys::KeyMap{KO}, n::Int64) where {KO}
    # two ccalls: the product (result left with the handle), then the copy-out into vectors of exactly the result's size
    k = Ref{Int64}(0)
    _check(GC.@preserve xi xv ccall((:dsa_mat_spmv_sparse_begin, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}), a.h, tr ? 1 : 0, xi, xv, length(xi), k))
    yi = Vector{Int64}(undef, k[]); yv = Vector{Float64}(undef, k[])
    if k[] > 0
        _check(GC.@preserve yi yv ccall((:dsa_mat_spmv_sparse_fetch, libdsa), Int32,
            (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}), a.h, yi, yv, k[], k))
    end
    return KO <: Integer ? sparsevec(KO.(yi), yv, n) : Dict{KO,Float64}(_out(out_keys, yi[j]) => yv[j] for j in eachindex(yi))
end
"the sparse product with every operand in HBM (device pointers; mapped key integers): xi / xv in, the touched rows yi / yv and their count
out, stream-ordered, no host wait — dsa_mat_spmv_sparse_dev"
function spmv_sparse_dev!(a::DynamicSparseMatrix, tr::Bool, d_xi::Ptr{Cvoid}, d_xv::Ptr{Cvoid}, nx::Integer, d_yi::Ptr{Cvoid}, d_yv::Ptr{Cvoid},
                          cap::Integer, d_count::Ptr{Cvoid})
    _check(ccall((:dsa_mat_spmv_sparse_dev, libdsa), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                 a.h, tr ? 1 : 0, d_xi, d_xv, nx, d_yi, d_yv, cap, d_count))
    return a
end
"mat * v / transpose(mat) * v for a DynamicSparseVector as a NEW DynamicSparseVector of length size(mat, 1 | 2): x, the product and the
result stay in HBM (Integer keys) — dsa_mat_mul_vec"
function _mul_vec(a::DynamicSparseMatrix, tr::Bool, v::DynamicSparseVector, ::Type{KO}) where {KO<:Integer}
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:dsa_mat_mul_vec, libdsa), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), a.h, tr ? 1 : 0, v.h, out))
    return DynamicSparseVector{KO}(out[])
end
mul_vec(a::DynamicSparseMatrix{K,L}, v::DynamicSparseVector) where {K,L} = _mul_vec(a, false, v, K)
mul_vec(t::Transposed{DynamicSparseMatrix{K,L}}, v::DynamicSparseVector) where {K,L} = _mul_vec(t.array, true, v, L)
_entries(km::KeyMap, v::DynamicSparseVector) = _stored_int(v)
_entries(km::KeyMap, v::SparseVector) = (_in(km, rowvals(v)), Vector{Float64}(nonzeros(v)))
const SpVec = Union{DynamicSparseVector,SparseVector}
Base.:(*)(a::DynamicSparseMatrix, v::SpVec) = _spmv_sparse(a, false, _entries(a.cols, v)..., a.rows, _size_int(a)[1])          # src/operations.jl:14-24
Base.:(*)(t::Transposed{<:DynamicSparseMatrix}, v::SpVec) = _spmv_sparse(t.array, true, _entries(t.array.rows, v)..., t.array.cols, _size_int(t.array)[2])   # :26-36
Base.:(*)(v::SpVec, t::Transposed{<:DynamicSparseMatrix}) = t.array * v                                                            # :38-48
Base.:(*)(v::SpVec, a::DynamicSparseMatrix) = transpose(a) * v                                                                     # :50-60
"dense x, dense y — the column-generation pricing product on device-resident data (Integer keys 1..n)"
function Base.:(*)(a::DynamicSparseMatrix, x::Vector{Float64})
    y = Vector{Float64}(undef, _size_int(a)[1])
    GC.@preserve x y _check(ccall((:dsa_mat_spmv_dense, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64), a.h, 0, x, length(x), y, length(y)))
    return y
end

# Y = A X / transpose(A) X for k right-hand sides (include/dsa.h: dsa_mat_spmm_dense; no reference counterpart — the k-column form of
# _mul, src/operations.jl:107-135).  The ABI takes X and Y ROW-MAJOR: a k x n Julia matrix (column-major) is exactly the row-major
# n x k operand, so transpose(Xt) goes in without a copy and the result comes back as the transpose of a k x ny matrix.
function _spmm(a::DynamicSparseMatrix, tr::Bool, xt::Matrix{Float64}, ny::Integer)
    k, nx = size(xt)
    yt = Matrix{Float64}(undef, k, ny)
    GC.@preserve xt yt _check(ccall((:dsa_mat_spmm_dense, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64), a.h, tr ? 1 : 0, xt, nx, k, k, yt, ny, k))
    return yt
end
Base.:(*)(a::DynamicSparseMatrix, X::Transpose{Float64,Matrix{Float64}}) = transpose(_spmm(a, false, parent(X), _size_int(a)[1]))
Base.:(*)(a::DynamicSparseMatrix, X::Matrix{Float64}) = permutedims(_spmm(a, false, permutedims(X), _size_int(a)[1]))
Base.:(*)(t::Transposed{<:DynamicSparseMatrix}, X::Transpose{Float64,Matrix{Float64}}) = transpose(_spmm(t.array, true, parent(X), _size_int(t.array)[2]))
Base.:(*)(t::Transposed{<:DynamicSparseMatrix}, X::Matrix{Float64}) = permutedims(_spmm(t.array, true, permutedims(X), _size_int(t.array)[2]))

# mul_rows(A, rows, X) = A[rows, :] * X and mul_cols(A, cols, X) = transpose(A[:, cols]) * X for a list of keys (include/dsa.h:
# dsa_mat_spmm_selected, 1-based; no reference counterpart): any order, repeats allowed, a key without entries gives a zero row, a
# key < 1 is an ArgumentError.  Row j is bit-identical to row keys[j] of A * X / transpose(A) * X, at a cost that follows the selected
# rows / columns only.  Integer keys only, like _select_int.  X goes in as in _spmm: xt is the k x nx Julia matrix.
function _spmm_selected(a::DynamicSparseMatrix{K,L}, tr::Bool, keys::AbstractVector{<:Integer}, xt::Matrix{Float64}) where {K,L}
    (K <: Integer && L <: Integer) || throw(ArgumentError("a key-list product needs integer row and column keys, got $(K), $(L)"))
    sel = Vector{Int64}(keys)
    k, nx = size(xt)
    yt = Matrix{Float64}(undef, k, length(sel))
    GC.@preserve sel xt yt _check(ccall((:dsa_mat_spmm_selected, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64),
        a.h, tr ? 1 : 0, sel, length(sel), xt, nx, k, k, yt, k))
    return yt
end
_mul_selected(a, tr, keys, X::Transpose{Float64,Matrix{Float64}}) = transpose(_spmm_selected(a, tr, keys, parent(X)))
_mul_selected(a, tr, keys, X::Matrix{Float64}) = permutedims(_spmm_selected(a, tr, keys, permutedims(X)))
_mul_selected(a, tr, keys, x::Vector{Float64}) = vec(_spmm_selected(a, tr, keys, reshape(x, 1, length(x))))
mul_rows(a::DynamicSparseMatrix, rows::AbstractVector{<:Integer}, X) = _mul_selected(a, false, rows, X)
mul_cols(a::DynamicSparseMatrix, cols::AbstractVector{<:Integer}, X) = _mul_selected(a, true, cols, X)

# mul_sparse(A, S) = A * S and transpose(A) * S for a SparseMatrixCSC S (include/dsa.h: dsa_mat_spgemm_csc, 1-based; the k-column form of
# the sparse-x product, src/operations.jl:62-135): column j of the result is A * S[:, j] — the touched rows only, stored zeros kept —
# bit for bit and the same on every call.  Integer keys only, like _select_int.  The first call counts (cap = 0: DSA_ECAP leaves ptr
# filled and the total in `got`), the second one fetches.
function _spgemm(a::DynamicSparseMatrix{K,L}, tr::Bool, S::SparseMatrixCSC, ny::Integer) where {K,L}
    (K <: Integer && L <: Integer) || throw(ArgumentError("a sparse-sparse product needs integer row and column keys, got $(K), $(L)"))
    xptr = Vector{Int64}(S.colptr); xidx = Vector{Int64}(rowvals(S)); xval = Vector{Float64}(nonzeros(S))
    k = size(S, 2)
    ptr = Vector{Int64}(undef, k + 1); idx = Int64[]; val = Float64[]
    got = Ref{Int64}(0)
    for _ in 1:2
        cap = length(idx)
        rc = GC.@preserve xptr xidx xval ptr idx val ccall((:dsa_mat_spgemm_csc, libdsa), Int32,
            (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}),
            a.h, Int32(tr ? 1 : 0), Int32(1), xptr, xidx, xval, k, ptr, cap == 0 ? Ptr{Int64}(C_NULL) : pointer(idx),
            cap == 0 ? Ptr{Float64}(C_NULL) : pointer(val), cap, got)
        if rc == 8 && cap == 0                      # DSA_ECAP
            resize!(idx, got[]); resize!(val, got[])
            continue
        end
        _check(rc)
        break
    end
    return SparseMatrixCSC(ny, k, ptr, idx, val)
end
mul_sparse(a::DynamicSparseMatrix, S::SparseMatrixCSC) = _spgemm(a, false, S, _size_int(a)[1])
mul_sparse(t::Transposed{<:DynamicSparseMatrix}, S::SparseMatrixCSC) = _spgemm(t.array, true, S, _size_int(t.array)[2])
Base.:(*)(a::DynamicSparseMatrix, S::SparseMatrixCSC) = mul_sparse(a, S)
Base.:(*)(t::Transposed{<:DynamicSparseMatrix}, S::SparseMatrixCSC) = mul_sparse(t, S)

# Reductions over the stored cells of every row / column and the in-place scaling A <- Diagonal(rows) * (alpha * A) * Diagonal(cols)
# (include/dsa.h: dsa_mat_reduce, dsa_mat_scale; no reference counterpart — sum(abs, A; dims), maximum(abs, ...), lmul! / rmul! of a
# SparseMatrixCSC).  kind: :sum, :abssum, :sqsum, :absmax (NaN propagates like maximum(abs, ...)) or :count (stored cells).
const RED_KINDS = Dict{Symbol,Int32}(:sum => Int32(0), :abssum => Int32(1), :sqsum => Int32(2), :absmax => Int32(3), :count => Int32(4))
function _reduce(a::DynamicSparseMatrix, orientation::Int32, kind::Symbol, n::Integer)
    haskey(RED_KINDS, kind) || throw(ArgumentError("kind must be one of :sum, :abssum, :sqsum, :absmax, :count"))
    y = Vector{Float64}(undef, n)
    GC.@preserve y _check(ccall((:dsa_mat_reduce, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int64), a.h, orientation, RED_KINDS[kind], y, length(y)))
    return y
end
reduce_rows(a::DynamicSparseMatrix, kind::Symbol) = _reduce(a, Int32(1), kind, _size_int(a)[1])          # DSA_ROWMAJOR
reduce_cols(a::DynamicSparseMatrix, kind::Symbol) = _reduce(a, Int32(0), kind, _size_int(a)[2])          # DSA_COLMAJOR
# Structure is preserved like lmul! / rmul!: a zero factor leaves stored zeros.  rows / cols = nothing: the factor is absent.
function scale!(a::DynamicSparseMatrix; alpha::Real = 1.0, rows::Union{Nothing,AbstractVector{<:Real}} = nothing,
                cols::Union{Nothing,AbstractVector{<:Real}} = nothing)
    r = rows === nothing ? Float64[] : Vector{Float64}(rows)
    c = cols === nothing ? Float64[] : Vector{Float64}(cols)
    # an empty factor that IS given still goes in as a non-NULL pointer (never read): NULL means absent
    one = Float64[1.0]
    GC.@preserve r c one _check(ccall((:dsa_mat_scale, libdsa), Int32,
        (Ptr{Cvoid}, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64), a.h, Float64(alpha),
        rows === nothing ? Ptr{Float64}(C_NULL) : pointer(isempty(r) ? one : r), length(r),
        cols === nothing ? Ptr{Float64}(C_NULL) : pointer(isempty(c) ? one : c), length(c)))
    return a
end

# SparseArrays' dropzeros! / droptol! in place on the device (include/dsa.h: dsa_mat_droptol; what the reference does with one
# setindex! of a zero per cell, src/matrix.jl:43-62): a cell with |v| <= tol, <= rows[i] or <= cols[j] leaves both orientations (IEEE
# comparisons: NaN is never dropped), an emptied column or row stays as an empty partition, the survivors are spread as by a root
# rebalance; when nothing is dropped nothing changes.  rows / cols are indexed by the mapped integer key; nothing: the vector is
# absent.  A negative tol matches nothing (purely relative dropping).  Returns a; count_droptol returns the number of entries the same
# call would drop and modifies nothing.
function _droptol(a::DynamicSparseMatrix, tol::Real, rows, cols, count_only::Bool)
    r = rows === nothing ? Float64[] : Vector{Float64}(rows)
    c = cols === nothing ? Float64[] : Vector{Float64}(cols)
    one = Float64[1.0]                                    # a given vector of length 0 is still a non-NULL pointer
    out = Ref{Int64}(0)
    GC.@preserve r c one _check(ccall((:dsa_mat_droptol, libdsa), Int32,
        (Ptr{Cvoid}, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Ref{Int64}), a.h, Float64(tol),
        rows === nothing ? Ptr{Float64}(C_NULL) : pointer(isempty(r) ? one : r), length(r),
        cols === nothing ? Ptr{Float64}(C_NULL) : pointer(isempty(c) ? one : c), length(c), Int32(count_only), out))
    return out[]
end
function SparseArrays.droptol!(a::DynamicSparseMatrix, tol::Real; rows::Union{Nothing,AbstractVector{<:Real}} = nothing,
                               cols::Union{Nothing,AbstractVector{<:Real}} = nothing)
    _droptol(a, tol, rows, cols, false)
    return a
end
SparseArrays.dropzeros!(a::DynamicSparseMatrix) = SparseArrays.droptol!(a, 0.0)
count_droptol(a::DynamicSparseMatrix, tol::Real; rows::Union{Nothing,AbstractVector{<:Real}} = nothing,
              cols::Union{Nothing,AbstractVector{<:Real}} = nothing) = _droptol(a, tol, rows, cols, true)

# The values of cells that are ALREADY STORED, overwritten or added to in place on the device (include/dsa.h: dsa_mat_update_values): no
# cell is created, deleted or moved, so the call does not go through the write planner of setindex_batch!.  A zero leaves a STORED zero
# (not the reference's delete-on-zero: dropzeros! removes it); a cell addressed more than once by update_values! ends with the last
# value, add_values! must address a cell at most once.  skip_missing = false: a cell that is not stored is an ArgumentError and
# nothing is modified; true: such ops are skipped.  Returns (number of cells written, mask of the ops without a stored cell).
function _update_values(a::DynamicSparseMatrix, op::Int32, I::AbstractVector, J::AbstractVector, V::AbstractVector, skip_missing::Bool)
    Ii = _in(a.rows, I); Ji = _in(a.cols, J); Vf = Vector{Float64}(V)
    length(Ii) == length(Ji) == length(Vf) || throw(ArgumentError("rows, columns, and nonzeros do not have same length."))
    missing_mask = zeros(UInt8, length(Ii))
    updated = Ref{Int64}(0); nmissing = Ref{Int64}(0)
    GC.@preserve Ii Ji Vf missing_mask _check(ccall((:dsa_mat_update_values, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{UInt8}, Ref{Int64}, Ref{Int64}),
        a.h, op, Int32(skip_missing), Ii, Ji, Vf, length(Ii), missing_mask, updated, nmissing))
    return updated[], missing_mask .!= 0
end
update_values!(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector, V::AbstractVector; skip_missing::Bool = false) =
    _update_values(a, Int32(0), I, J, V, skip_missing)          # DSA_UPD_SET
add_values!(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector, V::AbstractVector; skip_missing::Bool = false) =
    _update_values(a, Int32(1), I, J, V, skip_missing)          # DSA_UPD_ADD
# Cells that are NOT STORED yet, created in place on the device in both orientations (include/dsa.h: dsa_mat_insert_batch): the back end
# of update_values!(...; skip_missing = true).  Content, nnz and size end as after setindex_batch! of the same nonzero triples; the layout
# is the merged cell sequence spread by the root rebalance, the capacity doubled as often as the merged count needs.  A zero creates a
# STORED zero (dropzeros! removes it).  New columns / rows must lie behind the last entry of their table, which must be live; one in the
# middle is an error (use setindex_batch!).  skip_existing = false: a cell that is already stored is an ArgumentError and nothing is
# modified; true: such ops are skipped.  Returns the mask of the skipped ops.
function insert_values!(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector, V::AbstractVector; skip_existing::Bool = false)
    Ii = _in(a.rows, I); Ji = _in(a.cols, J); Vf = Vector{Float64}(V)
    length(Ii) == length(Ji) == length(Vf) || throw(ArgumentError("rows, columns, and nonzeros do not have same length."))
    existing_mask = zeros(UInt8, length(Ii))
    GC.@preserve Ii Ji Vf existing_mask _check(ccall((:dsa_mat_insert_batch, libdsa), Int32,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int32, Ptr{UInt8}),
        a.h, Ii, Ji, Vf, length(Ii), Int32(skip_existing), existing_mask))      # DSA_INS_SKIP_EXISTING
    return existing_mask .!= 0
end
# A[I[k], J[k]] = V[k] whether the cell is stored or not, for distinct cells: update_values! with skip_missing, then insert_values! of
# the ops it reports missing.  Host arrays only.  Returns (cells updated, cells inserted).
function upsert!(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector, V::AbstractVector)
    updated, miss = update_values!(a, I, J, V; skip_missing = true)
    any(miss) && insert_values!(a, I[miss], J[miss], V[miss])
    return updated, count(miss)
end
# The general write from triples (include/dsa.h: dsa_mat_assemble): ANY triples — cells stored or not, repeated or not, in any order —
# folded to distinct cells on the device (op = +: the values of a cell summed one after the other in the order of the batch, the
# left fold of dynamicsparse over duplicates; op = :set: the last value, bit for bit), the stored cells written in place as by
# update_values! / add_values!, the others created as by insert_values!, with its layout and its limit on new columns / rows.
# op = + is A + sparse(I, J, V) in place.  Any other op is an ArgumentError.  Returns (distinct cells, cells updated, cells inserted).
function assemble!(a::DynamicSparseMatrix, I::AbstractVector, J::AbstractVector, V::AbstractVector; op = +)
    opc = op === (+) ? Int32(1) : op === :set ? Int32(0) :      # DSA_UPD_ADD, DSA_UPD_SET
          throw(ArgumentError("assemble!: op must be + or :set"))
    Ii = _in(a.rows, I); Ji = _in(a.cols, J); Vf = Vector{Float64}(V)
    length(Ii) == length(Ji) == length(Vf) || throw(ArgumentError("rows, columns, and nonzeros do not have same length."))
    distinct = Ref{Int64}(0); updated = Ref{Int64}(0); inserted = Ref{Int64}(0)
    GC.@preserve Ii Ji Vf _check(ccall((:dsa_mat_assemble, libdsa), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}),
        a.h, opc, Ii, Ji, Vf, length(Ii), distinct, updated, inserted))
    return distinct[], updated[], inserted[]
end
"n getindex calls with every operand in HBM (device pointers; mapped key integers): d_out[k] = A[d_I[k], d_J[k]], d_found[k] (n bytes, or
C_NULL) = 1 iff the cell is stored, which tells a stored zero from an absent cell; enqueued on the colmajor stream, no host wait —
dsa_mat_get_batch_dev"
function getstored(a::DynamicSparseMatrix, d_I::Ptr{Cvoid}, d_J::Ptr{Cvoid}, n::Integer, d_out::Ptr{Cvoid}, d_found::Ptr{Cvoid} = C_NULL)
    _check(ccall((:dsa_mat_get_batch_dev, libdsa), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                 a.h, d_I, d_J, n, d_out, d_found))
    return a
end

# Combine on the device (include/dsa.h: dsa_mat_combine; not in the reference, whose Base.copy of a vector is an error and whose
# MappedPackedCSC(mpcsc) is a host deepcopy): alpha * a + beta * b with b's integer keys shifted by (row_off, col_off), as a NEW matrix —
# the one dynamicsparse builds from findnz(a), scaled, followed by findnz(b), shifted and scaled.  A cell of both operands is their sum; a
# sum that cancels stays a stored zero (dropzeros!).  The operands are only read.  m, n < 0: the smallest size that holds both.
_merge(x::KeyMap{K}, y::KeyMap{K}) where {K} = KeyMap{K}(x.seen === nothing ? nothing : merge(x.seen, y.seen))
function _combine(a::DynamicSparseMatrix{K,L}, alpha::Real, b::Union{Nothing,DynamicSparseMatrix{K,L}}, beta::Real, row_off::Integer,
                  col_off::Integer, m::Integer = -1, n::Integer = -1) where {K,L}
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve a b _check(ccall((:dsa_mat_combine, libdsa), Int32,
        (Ptr{Cvoid}, Float64, Ptr{Cvoid}, Float64, Int64, Int64, Int64, Int64, Ref{Ptr{Cvoid}}),
        a.h, Float64(alpha), b === nothing ? C_NULL : b.h, Float64(beta), row_off, col_off, m, n, out))
    b === nothing && return DynamicSparseMatrix{K,L}(out[], _merge(a.rows, a.rows), _merge(a.cols, a.cols))
    return DynamicSparseMatrix{K,L}(out[], _merge(a.rows, b.rows), _merge(a.cols, b.cols))
end
Base.copy(a::DynamicSparseMatrix) = _combine(a, 1.0, nothing, 0.0, 0, 0)
Base.:+(a::DynamicSparseMatrix{K,L}, b::DynamicSparseMatrix{K,L}) where {K,L} = _combine(a, 1.0, b, 1.0, 0, 0)
Base.:-(a::DynamicSparseMatrix{K,L}, b::DynamicSparseMatrix{K,L}) where {K,L} = _combine(a, 1.0, b, -1.0, 0, 0)
Base.:-(a::DynamicSparseMatrix) = _combine(a, -1.0, nothing, 0.0, 0, 0)
Base.:*(alpha::Real, a::DynamicSparseMatrix) = _combine(a, alpha, nothing, 0.0, 0, 0)
# concatenation shifts keys, so it is for integer keys: [a b] needs equal row counts, [a; b] equal column counts
function Base.hcat(a::DynamicSparseMatrix{K,L}, b::DynamicSparseMatrix{K,L}) where {K<:Integer,L<:Integer}
    (ma, na), (mb, _) = _size_int(a), _size_int(b)
    ma == mb || throw(ArgumentError("hcat: the operands have $ma and $mb rows"))
    return _combine(a, 1.0, b, 1.0, 0, na)
end
function Base.vcat(a::DynamicSparseMatrix{K,L}, b::DynamicSparseMatrix{K,L}) where {K<:Integer,L<:Integer}
    (ma, na), (_, nb) = _size_int(a), _size_int(b)
    na == nb || throw(ArgumentError("vcat: the operands have $na and $nb columns"))
    return _combine(a, 1.0, b, 1.0, ma, 0)
end
function SparseArrays.blockdiag(a::DynamicSparseMatrix{K,L}, b::DynamicSparseMatrix{K,L}) where {K<:Integer,L<:Integer}
    ma, na = _size_int(a)
    return _combine(a, 1.0, b, 1.0, ma, na)
end

end # module
