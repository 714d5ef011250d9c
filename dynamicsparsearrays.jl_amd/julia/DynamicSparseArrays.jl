# DynamicSparseArrays.jl — the module under the REFERENCE's name, so that `using DynamicSparseArrays` in Coluna (or in the
# reference's own test-suite) resolves to the MI355X-native implementation without touching the caller: put this
# directory on LOAD_PATH in front of the registered package.  It re-exports exactly the twelve names the reference exports
# (src/DynamicSparseArrays.jl:5-16) from DynamicSparseArraysAMD.jl, plus — unexported, as in the reference — the names its
# tests and Coluna reach through the module (`DynamicSparseArrays.PackedCSC`, `DynamicSparseArrays.nbpartitions`, ...).
# Unexecuted here (no Julia toolchain in the build image); tests/test_library_symbols.py checks the export lists.
module DynamicSparseArrays

include("DynamicSparseArraysAMD.jl")
using .DynamicSparseArraysAMD

export DynamicSparseVector,
       DynamicSparseMatrix,
       DynamicMatrixColView,
       dynamicsparsevec,
       dynamicsparse,
       nbpartitions,
       deletepartition!,
       deletecolumn!,
       deleterow!,
       addrow!,
       closefillmode!,
       shrink_size!

const PackedCSC = DynamicSparseArraysAMD.PackedCSC
const Transposed = DynamicSparseArraysAMD.Transposed
const keyint = DynamicSparseArraysAMD.keyint            # extend these two for id structs used as keys (key-mapping layer)
const keyfrom = DynamicSparseArraysAMD.keyfrom
const set_device! = DynamicSparseArraysAMD.set_device!
const getindex_batch = DynamicSparseArraysAMD.getindex_batch
const setindex_batch! = DynamicSparseArraysAMD.setindex_batch!
const deletecolumns! = DynamicSparseArraysAMD.deletecolumns!      # a list of columns / rows in one device pass (dsa_mat_delete_batch)
const deleterows! = DynamicSparseArraysAMD.deleterows!
const dropzeros! = DynamicSparseArraysAMD.dropzeros!              # SparseArrays' dropzeros! / droptol! in place on the device (dsa_mat_droptol):
const droptol! = DynamicSparseArraysAMD.droptol!                  # droptol!(A, tol; rows = nothing, cols = nothing)
const count_droptol = DynamicSparseArraysAMD.count_droptol
const update_values! = DynamicSparseArraysAMD.update_values!      # values of stored cells overwritten / added to in place (dsa_mat_update_values)
const add_values! = DynamicSparseArraysAMD.add_values!
const insert_values! = DynamicSparseArraysAMD.insert_values!      # cells that are not stored yet created in place (dsa_mat_insert_batch)
const upsert! = DynamicSparseArraysAMD.upsert!                    # update_values! of the stored cells, insert_values! of the others
const getstored = DynamicSparseArraysAMD.getstored                # getindex_batch with every operand in HBM (dsa_mat_get_batch_dev)

end # module
