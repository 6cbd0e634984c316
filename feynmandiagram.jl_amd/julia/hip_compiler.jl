# hip_compiler.jl -- Julia host side of the MI355X evaluator back end.
#
# Drop into src/backend/ of FeynmanDiagram.jl and `include("hip_compiler.jl")`
# from src/backend/compiler.jl after the existing includes (compiler.jl:16-18).
# It adds
#
#     Compilers.compile_hip(graphs; root=[id(g) for g in graphs], backend=:isa)
#         -> (f::GraphFunc, leafmap::Dict{Int,G})
#
# with the *same* `leafmap` (index of `leafVal` -> leaf graph object) that
# `Compilers.compile` / `to_julia_str` return (static.jl:98-133), so
# `FrontEnds.leafstates(leaf_maps, ...)` (frontends.jl:115-232) works unchanged.
#
#     f(root::AbstractVector, leafVal::AbstractVector)   one sample; mutates root,
#                                                        returns the last root written
#     f(root::AbstractMatrix, leafVal::AbstractMatrix)   B samples: leafVal is B x L,
#                                                        root is B x R (column-major
#                                                        Julia matrices = the "leaf
#                                                        major" layout of the C ABI)
#
# STATUS: UNVERIFIED.  Julia is not installed in the build environment or on the
# GPU box, so this file has never been executed.  The C ABI it binds
# (include/fdg.h) is exercised by the Python/ctypes twin (capi.py) in tests/.
#
# The traversal below restates to_julia_str's loop over the arrays of the node
# table instead of over text; it must stay in lock step with static.jl:98-133.

const _libfdg = get(ENV, "FDG_LIB", "libfdg.so")

struct _FdgGraphDesc
    n_leaf::UInt32
    n_node::UInt32
    n_root::UInt32
    n_edge::UInt32
    op::Ptr{UInt8}
    power::Ptr{Int32}
    child_off::Ptr{UInt32}
    child_idx::Ptr{UInt32}
    child_fac::Ptr{Float64}
    root_slot::Ptr{UInt32}
end

const FDG_NO_ROOT = 0xffffffff
const FDG_SPEC_ISA = Cuint(4)
const FDG_SPEC_AUTOTUNE = Cuint(8)

_fdg_check(rc) = rc == 0 ? nothing :
    error("fdg error $rc: " * unsafe_string(ccall((:fdg_last_error, _libfdg), Cstring, ())))

mutable struct GraphFunc
    handle::Ptr{Cvoid}
    n_leaf::Int
    n_root::Int
    last_root::Int          # 1-based index of the root written last, 0 if none
    cache_dir::Union{Nothing,String}   # the JIT cache directory given to compile_hip (nothing: the library's per-user default); later specialisations use it too
    function GraphFunc(h, L, R, last, cache_dir=nothing)
        f = new(h, L, R, last, cache_dir)
        finalizer(x -> ccall((:fdg_graph_destroy, _libfdg), Cint, (Ptr{Cvoid},), x.handle), f)
        return f
    end
end

_opcode(::Type{ComputationalGraphs.Sum}) = (0x00, Int32(0))
_opcode(::Type{ComputationalGraphs.Prod}) = (0x01, Int32(0))
_opcode(::Type{ComputationalGraphs.Power{N}}) where {N} = (0x02, Int32(N))
_opcode(op::Type) = error(                       # same failure as static.jl:6-11
    "Static representation for computational graph nodes with operator $(op) not yet implemented! ")

"""
    lower_to_table(graphs; root) -> (arrays..., leafmap)

Statement order, leaf numbering and root mapping of `to_julia_str` (static.jl:98-133).
"""
function lower_to_table(graphs::AbstractVector{G}; root::AbstractVector{Int}=[id(g) for g in graphs]) where {G<:AbstractGraph}
    leaf_index = Dict{Int,Int}()      # id -> 0-based leaf index
    node_index = Dict{Int,Int}()      # id -> 0-based internal index
    leafmap = Dict{Int,G}()
    order = G[]
    stmt_pos = Dict{Int,Int}()        # id -> position of its statement in the text to_julia_str would emit
    for graph in graphs
        for g in PostOrderDFS(graph)
            g_id = id(g)
            if isempty(subgraphs(g))
                haskey(leaf_index, g_id) && continue
                leaf_index[g_id] = length(leaf_index)
                leafmap[length(leaf_index)] = g
            else
                haskey(node_index, g_id) && continue
                _opcode(operator(g))
                node_index[g_id] = length(order)
                push!(order, g)
            end
            stmt_pos[g_id] = length(stmt_pos)
        end
    end
    L = length(leaf_index)
    vidx(gid) = haskey(leaf_index, gid) ? leaf_index[gid] : L + node_index[gid]
    op = UInt8[]; power = Int32[]; off = UInt32[0]; idx = UInt32[]; fac = Float64[]
    for g in order
        o, p = _opcode(operator(g))
        push!(op, o); push!(power, p)
        for (sg, f) in zip(subgraphs(g), subgraph_factors(g))
            push!(idx, UInt32(vidx(id(sg)))); push!(fac, Float64(f))
        end
        push!(off, UInt32(length(idx)))
    end
    root_slot = fill(UInt32(FDG_NO_ROOT), length(root))
    last_root, last_rank = 0, -1
    for (k, rid) in enumerate(root)
        findfirst(==(rid), root) == k || continue             # findfirst (static.jl:112)
        (haskey(leaf_index, rid) || haskey(node_index, rid)) || continue
        root_slot[k] = UInt32(vidx(rid))
        rank = stmt_pos[rid]          # `root[k] = g` follows g's own statement (static.jl:126-128): the last one is the call's value
        if rank > last_rank
            last_rank, last_root = rank, k
        end
    end
    return L, op, power, off, idx, fac, root_slot, leafmap, last_root
end

"""
    compile_hip(graphs; root, backend=:isa, autotune=false, groups=nothing, cache_dir=nothing, association=:static)

`association = :eval` makes the handle reproduce the interpreter `eval!` (src/computational_graph/eval.jl:1-3,15-39: every operand is
scaled by its factor before it enters the fold, `Prod = (w1*f1) * (w2*f2) * ...`) instead of the generated code of `Compilers.compile`
(src/backend/static.jl:13-46) -- `fdg_graph_set_association(h, FDG_ASSOC_INTERP)`; the two differ only where a `Prod` has a factor other
than +-1 on its second or a later operand.

`groups` (optional `Dict{Int,Int}`: node id => tag) is the scheduling hint of
`fdg_graph_set_schedule_groups`: pass the coefficient -> original-node map of `taylorexpansion!`
(`to_coeff_map`, src/utility.jl:105-135) so that all Taylor coefficients of one node are evaluated
together.  It never changes a value.
"""
function compile_hip(graphs::AbstractVector{<:AbstractGraph};
    root::AbstractVector{Int}=[id(g) for g in graphs], backend::Symbol=:isa, autotune::Bool=false,
    groups::Union{Nothing,Dict{Int,Int}}=nothing, cache_dir::Union{Nothing,String}=nothing, association::Symbol=:static)
    association in (:static, :eval) || error("association must be :static or :eval")
    L, op, power, off, idx, fac, root_slot, leafmap, last_root = lower_to_table(graphs; root=root)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve op power off idx fac root_slot begin
        desc = Ref(_FdgGraphDesc(UInt32(L), UInt32(length(op)), UInt32(length(root_slot)), UInt32(length(idx)),
            pointer(op), pointer(power), pointer(off), pointer(idx), pointer(fac), pointer(root_slot)))
        _fdg_check(ccall((:fdg_graph_create, _libfdg), Cint, (Ref{_FdgGraphDesc}, Ref{Ptr{Cvoid}}), desc, h))
    end
    if association == :eval      # FDG_ASSOC_INTERP = 1; before any specialisation
        _fdg_check(ccall((:fdg_graph_set_association, _libfdg), Cint, (Ptr{Cvoid}, Cint), h[], Cint(1)))
    end
    if !isnothing(groups)
        # internal nodes in statement order, exactly the order lower_to_table numbered them
        seen = Set{Int}(); tags = Dict{Int,UInt32}(); grp = UInt32[]
        for graph in graphs, g in PostOrderDFS(graph)
            (isempty(subgraphs(g)) || id(g) in seen) && continue
            push!(seen, id(g))
            key = get(groups, id(g), -id(g))
            push!(grp, get!(tags, key, UInt32(length(tags))))
        end
        _fdg_check(ccall((:fdg_graph_set_schedule_groups, _libfdg), Cint, (Ptr{Cvoid}, Ptr{UInt32}, UInt32), h[], grp, UInt32(length(grp))))
    end
    if backend != :interp
        flags = backend == :isa ? (FDG_SPEC_ISA | (autotune ? FDG_SPEC_AUTOTUNE : Cuint(0))) : Cuint(0)
        cdir = isnothing(cache_dir) ? C_NULL : cache_dir
        rc = ccall((:fdg_graph_specialize, _libfdg), Cint, (Ptr{Cvoid}, Cstring, Cuint), h[], cdir, flags)
        if rc == -2 && backend == :isa      # FDG_E_UNSUPPORTED (the ISA back end covers every operator of the reference; kept for future ones)
            rc = ccall((:fdg_graph_specialize, _libfdg), Cint, (Ptr{Cvoid}, Cstring, Cuint), h[], cdir, Cuint(0))
        elseif rc == 0 && backend == :isa && L > 1 && length(op) <= 4000
            # a handle without a row-major variant of the ISA kernel (fdg_kernel_info.has_rm == 0: fewer than 16 leaves, the
            # tiny-graph configuration): HIP-source companion for row-major [B, L] input (FDG_SPEC_ROW_MAJOR_COMPANION = 16)
            ki = zeros(UInt8, 256)              # sizeof(fdg_kernel_info) = 168 (48 + 3*8 + 4*3*4 + 4*4, then the pool / rl fields), rounded up
            _fdg_check(ccall((:fdg_graph_kernel_info, _libfdg), Cint, (Ptr{Cvoid}, Ptr{UInt8}), h[], ki))
            has_rm = reinterpret(UInt32, ki[125:128])[1]      # offset 124: has_acc at 120, has_rm at 124
            if has_rm == 0
                rc = ccall((:fdg_graph_specialize, _libfdg), Cint, (Ptr{Cvoid}, Cstring, Cuint), h[], cdir, Cuint(16))
            end
        end
        _fdg_check(rc)
    end
    return GraphFunc(h[], L, length(root_slot), last_root, cache_dir), leafmap
end

# one sample: the calling convention of the generated eval_graph!(root, leafVal)
function (f::GraphFunc)(root::AbstractVector{Float64}, leafVal::AbstractVector{Float64})
    length(leafVal) >= f.n_leaf || throw(BoundsError(leafVal, f.n_leaf))
    length(root) >= f.n_root || throw(BoundsError(root, f.n_root))
    lv = Vector{Float64}(leafVal[1:f.n_leaf]); rt = Vector{Float64}(root[1:f.n_root])
    _fdg_check(ccall((:fdg_eval, _libfdg), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), f.handle, lv, rt, 1))
    root[1:f.n_root] .= rt
    return f.last_root == 0 ? nothing : root[f.last_root]
end

# B samples, host matrices (B x L in, B x R out, column-major): H2D, eval, D2H
function (f::GraphFunc)(root::Matrix{Float64}, leafVal::Matrix{Float64})
    B = size(leafVal, 1)
    size(leafVal, 2) >= f.n_leaf || throw(BoundsError(leafVal, (1, f.n_leaf)))
    size(root) == (B, f.n_root) || throw(DimensionMismatch("root must be B x R"))
    # column-major matrices as they are: sample stride 1, value stride B (no transposition copy on either side;
    # the device sees them leaf-major, the evaluator's fast layout)
    _fdg_check(ccall((:fdg_eval_strided, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64),
        f.handle, leafVal, 1, B, root, 1, B, B))
    return root
end

# B samples, device pointers (e.g. from AMDGPU.jl ROCArrays of size B x L / B x R):
# strides in elements; a column-major B x L matrix is (sample stride 1, leaf stride B)
function eval_device!(f::GraphFunc, d_root::Ptr{Float64}, d_leaf::Ptr{Float64}, B::Integer;
    leaf_strides=(1, B), root_strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_eval_device, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], d_root, root_strides[1], root_strides[2], B, stream))
end

# Element types other than Float64 (the function Compilers.compile returns is generic in eltype(leafVal)): the per-type kernel
# is compiled on first use; a ComplexF64 element is the pair (re, im), strides count elements
const _FDG_DT = Dict{DataType,Cint}(Float64 => 0, Float32 => 1, ComplexF64 => 2, ComplexF32 => 3)
function eval_device!(f::GraphFunc, d_root::Ptr{T}, d_leaf::Ptr{T}, B::Integer;
    leaf_strides=(1, B), root_strides=(1, B), stream::Ptr{Cvoid}=C_NULL) where {T<:Union{Float32,ComplexF64,ComplexF32}}
    dt = _FDG_DT[T]
    # (flag 4 = FDG_SPEC_ISA: ComplexF64 batches whose rows are contiguous -- leaf_strides = (L, 1) -- additionally get the graph spelled out on
    #  real and imaginary parts through the assembly back end; a column-major B x L Julia matrix takes the per-type kernel)
    cdir = isnothing(f.cache_dir) ? C_NULL : f.cache_dir
    _fdg_check(ccall((:fdg_graph_specialize_typed, _libfdg), Cint, (Ptr{Cvoid}, Cint, Cstring, Cuint), f.handle, dt, cdir, Cuint(4)))
    _fdg_check(ccall((:fdg_eval_device_typed, _libfdg), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}),
        f.handle, dt, d_leaf, leaf_strides[1], leaf_strides[2], d_root, root_strides[1], root_strides[2], B, stream))
end
# The Monte-Carlo step for these types (include/fdg.h: fdg_accumulate_device_typed): d_acc[k] += sum_b w[b] * root_k(b) over the roots as
# eval_device! would have stored them, widened to Float64.  d_acc (and d_acc2, the sums of squares; C_NULL: not wanted) is a Vector{Float64}
# of length R for Float32 leaves and a Vector{ComplexF64} of length R for complex leaves; d_weight a Vector{Float64} or C_NULL (weight 1)
function accumulate_device!(f::GraphFunc, d_acc::Ptr, d_leaf::Ptr{T}, d_weight::Ptr{Float64}, B::Integer;
    d_acc2::Ptr=C_NULL, leaf_strides=(1, B), stream::Ptr{Cvoid}=C_NULL) where {T<:Union{Float32,ComplexF64,ComplexF32}}
    dt = _FDG_DT[T]
    cdir = isnothing(f.cache_dir) ? C_NULL : f.cache_dir
    _fdg_check(ccall((:fdg_graph_specialize_typed, _libfdg), Cint, (Ptr{Cvoid}, Cint, Cstring, Cuint), f.handle, dt, cdir, Cuint(4)))
    _fdg_check(ccall((:fdg_accumulate_device_typed, _libfdg), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        f.handle, dt, d_leaf, leaf_strides[1], leaf_strides[2], d_weight, d_acc, d_acc2, B, stream))
end

# Tile-major batches (include/fdg.h: fdg_eval_device_tiled): the leaves as an Array{Float64,3}(undef, 64, L, cld(B, 64)) -- sample in tile,
# leaf, tile -- and the roots as (64, R, cld(B, 64)); what a Monte-Carlo driver that owns its sample batch should allocate: one
# contiguous block of 512 L bytes per wave instead of 64 samples of each of L columns.  Strides in elements: (sample, value, tile).
function eval_device_tiled!(f::GraphFunc, d_root::Ptr{Float64}, d_leaf::Ptr{Float64}, B::Integer;
    leaf_strides=(1, 64, 64 * f.n_leaf), root_strides=(1, 64, 64 * f.n_root), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_eval_device_tiled, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], leaf_strides[3], d_root, root_strides[1], root_strides[2], root_strides[3], B, stream))
end
function accumulate_device_tiled!(f::GraphFunc, d_acc::Ptr{Float64}, d_leaf::Ptr{Float64}, d_weight::Ptr{Float64}, B::Integer;
    leaf_strides=(1, 64, 64 * f.n_leaf), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_accumulate_device_tiled, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], leaf_strides[3], d_weight, d_acc, B, stream))
end
# Binned accumulation (include/fdg.h: fdg_accumulate_device_binned), the `measure` step of an observable that depends on an external variable:
# d_acc[k, j] += w[b] * root_k(b) for every sample b whose bin j = d_bin[b] (1-based: bin_base = 1) lies in 1:n_bin; other samples add nothing.
# d_acc is an R x n_bin Matrix{Float64} on the device, d_bin a Vector{Int32}, d_weight a Vector{Float64} or C_NULL (weight 1), both indexed by
# sample.  Leaves: a column-major B x L matrix (leaf_strides = (1, B), tile_stride = 0) or a tile-major batch (strides (1, 64), tile_stride
# 64 L).  No float atomics: the same arguments give the same bits.
function accumulate_device_binned!(f::GraphFunc, d_acc::Ptr{Float64}, d_leaf::Ptr{Float64}, d_bin::Ptr{Int32}, n_bin::Integer,
    d_weight::Ptr{Float64}, B::Integer; leaf_strides=(1, B), tile_stride::Integer=0, bin_base::Integer=1, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_accumulate_device_binned, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight, d_acc, B, stream))
    return nothing
end
# Second moments as well (fdg_accumulate_device_moments), for Monte-Carlo error bars: with t = w[b] * root_k(b), d_acc[k, j] += t and
# d_acc2[k, j] += t * t.  d_acc and d_acc2 are two distinct R x n_bin matrices; d_acc gets the bits accumulate_device_binned! gives.
# d_bin = C_NULL puts every sample in one bin (n_bin = 1, bin_base ignored): the plain sum with its error bar.  Mean and standard error per
# (root, bin) over the B samples: m = S1 / B, err = sqrt((S2 / B - m^2) / (B - 1)).
function accumulate_device_moments!(f::GraphFunc, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_leaf::Ptr{Float64}, d_bin::Ptr{Int32},
    n_bin::Integer, d_weight::Ptr{Float64}, B::Integer; leaf_strides=(1, B), tile_stride::Integer=0, bin_base::Integer=1,
    stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_accumulate_device_moments, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream))
    return nothing
end
# ---- VEGAS importance sampling (include/fdg.h; no counterpart in the reference: the caller side of example/benchmark.jl:46-51) ---- #
# The map is a (G + 1) x D Matrix{Float64} of cell edges (column d: the edges of variable d, strictly increasing); d_grid is its copy on
# the device.  vegas_sample_device! draws B samples through it: variable d goes to column col[d] (1-based; default d) of the matrix at
# d_x (strides as a B x C column-major matrix by default, what the one-kernel Monte-Carlo route reads in place), d_jac[b] is the weight
# 1/pdf of sample b, d_cell (B x D Int32, optional) the cells.  Counter-based: sample_offset + b is the global sample number.
function vegas_sample_device!(d_x::Ptr{Float64}, d_jac::Ptr{Float64}, d_grid::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer;
    col::Union{Nothing,AbstractVector{<:Integer}}=nothing, seed::Integer=0, sample_offset::Integer=0, x_strides=(1, B),
    d_cell::Ptr{Int32}=Ptr{Int32}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    _fdg_check(ccall((:fdg_vegas_sample_device, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, UInt64, UInt64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, seed, sample_offset, d_x, x_strides[1], x_strides[2], d_jac, d_cell, B, stream))
    return nothing
end
# The accumulate step of an iteration (fdg_accumulate_device_vegas): d_acc, d_acc2 (R each) as accumulate_device_moments! with d_bin = C_NULL
# leaves them, and the training histogram d_hist (G x D, added to): d_hist[c, d] += (w[b] * sum_k coef[k] * root_k(b))^2, c the cell of
# sample b in variable d recomputed from (seed, sample_offset + b, d).  coef: host vector of R factors, or nothing for the plain sum.
function accumulate_device_vegas!(f::GraphFunc, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_hist::Ptr{Float64}, d_leaf::Ptr{Float64},
    d_weight::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer; coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, leaf_strides=(1, B), tile_stride::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_accumulate_device_vegas, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_weight, coef === nothing ? C_NULL : coef, seed, sample_offset,
        n_dim, n_grid, d_acc, d_acc2, d_hist, B, stream))
    return nothing
end
# Lepage's refinement of the map from the training histogram, both on the host (fdg_vegas_refine): grid is (G + 1) x D, hist G x D.
function vegas_refine!(grid::Matrix{Float64}, hist::Matrix{Float64}; alpha::Float64=0.5)
    size(hist) == (size(grid, 1) - 1, size(grid, 2)) || error("hist must be (G, D) for a (G + 1, D) grid")
    _fdg_check(ccall((:fdg_vegas_refine, _libfdg), Cint, (Ptr{Float64}, Ptr{Float64}, UInt32, UInt32, Float64),
        grid, hist, size(grid, 2), size(hist, 1), alpha))
    return grid
end
# ---- adaptive stratified sampling, VEGAS+ (include/fdg.h; no counterpart in the reference: MCIntegration is the caller's side) ---- #
# strat: the strata per variable (a Vector, H = prod(strat) hypercubes, variable 1 fastest); d_start: H + 1 Int64 on the device, the
# prefix sums of the samples per hypercube in global sample indices (0-based values); d_cube[b] receives the sample's hypercube
# (0-based).  Unverified: there is no Julia in the image these wrappers were written in.
function vegas_sample_device_strat!(d_x::Ptr{Float64}, d_jac::Ptr{Float64}, d_cube::Ptr{Int32}, d_grid::Ptr{Float64}, n_dim::Integer,
    n_grid::Integer, strat::AbstractVector{<:Integer}, d_start::Ptr{Int64}, B::Integer;
    col::Union{Nothing,AbstractVector{<:Integer}}=nothing, seed::Integer=0, sample_offset::Integer=0, x_strides=(1, B),
    d_cell::Ptr{Int32}=Ptr{Int32}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    sv = UInt32.(strat)
    _fdg_check(ccall((:fdg_vegas_sample_device_strat, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, Ptr{UInt32}, Ptr{Int64}, UInt64, UInt64, Ptr{Float64}, Int64, Int64, Ptr{Float64},
         Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, sv, d_start, seed, sample_offset, d_x, x_strides[1], x_strides[2], d_jac,
        d_cube, d_cell, B, stream))
    return nothing
end
# accumulate_device_vegas! with the training cells by the stratified formula and the per-hypercube moments d_cube_sum, d_cube_sum2
# ((R + 1) x H each, added to; row R + 1 the coef combination).
function accumulate_device_strat!(f::GraphFunc, d_leaf::Ptr{Float64}, d_weight::Ptr{Float64}, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64},
    d_hist::Ptr{Float64}, strat::AbstractVector{<:Integer}, d_cube::Ptr{Int32}, d_cube_sum::Ptr{Float64}, d_cube_sum2::Ptr{Float64},
    n_dim::Integer, n_grid::Integer, B::Integer; coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, leaf_strides=(1, B), tile_stride::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    sv = UInt32.(strat)
    _fdg_check(ccall((:fdg_accumulate_device_strat, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{UInt32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_weight, coef === nothing ? C_NULL : coef, seed, sample_offset,
        n_dim, n_grid, d_acc, d_acc2, d_hist, sv, d_cube, d_cube_sum, d_cube_sum2, B, stream))
    return nothing
end
function mc_accumulate_device_strat!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_weight::Ptr{Float64}, d_acc::Ptr{Float64},
    d_acc2::Ptr{Float64}, d_hist::Ptr{Float64}, strat::AbstractVector{<:Integer}, d_cube::Ptr{Int32}, d_cube_sum::Ptr{Float64},
    d_cube_sum2::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer; kF::Float64, beta::Float64, lambda::Float64,
    coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0, k_strides=(1, B), t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    sv = UInt32.(strat)
    _fdg_check(ccall((:fdg_mc_accumulate_device_strat, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, UInt64,
         UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Cvoid}),
        f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_weight,
        coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, sv, d_cube, d_cube_sum, d_cube_sum2,
        B, stream))
    return nothing
end
# The next iteration's allocation, on the host (fdg_strat_allocate): cube_sum, cube_sum2 are (R + 1) x H, col the 1-based row the
# allocation follows, start_old H + 1 prefix sums (nothing: no history, the uniform allocation); start_new is filled and returned.
function strat_allocate!(start_new::Vector{Int64}, cube_sum::Union{Nothing,Matrix{Float64}}, cube_sum2::Union{Nothing,Matrix{Float64}},
    col::Integer, start_old::Union{Nothing,Vector{Int64}}, n_total::Integer; beta::Float64=0.75)
    H = length(start_new) - 1
    ld = cube_sum === nothing ? 0 : size(cube_sum, 1)
    _fdg_check(ccall((:fdg_strat_allocate, _libfdg), Cint,
        (Ptr{Float64}, Ptr{Float64}, UInt32, UInt32, Ptr{Int64}, UInt32, Int64, Float64, Ptr{Int64}),
        cube_sum === nothing ? C_NULL : cube_sum, cube_sum2 === nothing ? C_NULL : cube_sum2, ld, max(col - 1, 0),
        start_old === nothing ? C_NULL : start_old, H, n_total, beta, start_new))
    return start_new
end
# The allocation from several rows (fdg_strat_allocate_cols): cols the 1-based rows whose variances are added up, in that order.
function strat_allocate_cols!(start_new::Vector{Int64}, cube_sum::Union{Nothing,Matrix{Float64}}, cube_sum2::Union{Nothing,Matrix{Float64}},
    cols::AbstractVector{<:Integer}, start_old::Union{Nothing,Vector{Int64}}, n_total::Integer; beta::Float64=0.75)
    H = length(start_new) - 1
    ld = cube_sum === nothing ? 0 : size(cube_sum, 1)
    cv = UInt32.(cols .- 1)
    _fdg_check(ccall((:fdg_strat_allocate_cols, _libfdg), Cint,
        (Ptr{Float64}, Ptr{Float64}, UInt32, Ptr{UInt32}, UInt32, Ptr{Int64}, UInt32, Int64, Float64, Ptr{Int64}),
        cube_sum === nothing ? C_NULL : cube_sum, cube_sum2 === nothing ? C_NULL : cube_sum2, ld, cv, length(cv),
        start_old === nothing ? C_NULL : start_old, H, n_total, beta, start_new))
    return start_new
end
# ---- a discrete external variable (include/fdg.h; no counterpart in the reference: the caller's side of test/ver4.jl:224-237) ---- #
# ExtKidx = MCIntegration.Discrete(1, Nk): d_cdf (n_bin + 1, on the device) is the variable's cumulative distribution, d_ext (n_ext x n_bin,
# column j = what value j means) goes to the columns ext_col (1-based) of x; d_bin[b] is the value drawn (1-based by default), d_jac[b] the
# continuous weight divided by the value's probability.  n_bin = 1 is vegas_sample_device! bit for bit.
function vegas_sample_device_discrete!(d_x::Ptr{Float64}, d_jac::Ptr{Float64}, d_bin::Ptr{Int32}, d_grid::Ptr{Float64}, n_dim::Integer,
    n_grid::Integer, d_cdf::Ptr{Float64}, n_bin::Integer, B::Integer; col::Union{Nothing,AbstractVector{<:Integer}}=nothing,
    d_ext::Ptr{Float64}=Ptr{Float64}(C_NULL), ext_col::AbstractVector{<:Integer}=Int[], bin_base::Integer=1, seed::Integer=0,
    sample_offset::Integer=0, x_strides=(1, B), d_cell::Ptr{Int32}=Ptr{Int32}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    e = UInt32.(ext_col .- 1)
    _fdg_check(ccall((:fdg_vegas_sample_device_discrete, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, Ptr{Float64}, UInt32, Int32, Ptr{Float64}, UInt32, Ptr{UInt32}, UInt64, UInt64,
         Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, d_cdf, n_bin, bin_base, d_ext, length(e), isempty(e) ? C_NULL : e, seed,
        sample_offset, d_x, x_strides[1], x_strides[2], d_jac, d_bin, d_cell, B, stream))
    return nothing
end
# The accumulate step with the discrete variable (fdg_accumulate_device_vegas_binned): d_acc, d_acc2 (R x n_bin) as accumulate_device_moments!
# leaves them, d_hist (G x D) as accumulate_device_vegas!, and d_hist_bin (n_bin, or C_NULL: not trained) the same squares summed per value.
function accumulate_device_vegas_binned!(f::GraphFunc, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_hist::Ptr{Float64},
    d_hist_bin::Ptr{Float64}, d_leaf::Ptr{Float64}, d_bin::Ptr{Int32}, n_bin::Integer, d_weight::Ptr{Float64}, n_dim::Integer,
    n_grid::Integer, B::Integer; coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    leaf_strides=(1, B), tile_stride::Integer=0, bin_base::Integer=1, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_accumulate_device_vegas_binned, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight, coef === nothing ? C_NULL : coef,
        seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, B, stream))
    return nothing
end
# The refinement of the probabilities, both on the host (fdg_vegas_refine_discrete): cdf is n_bin + 1, hist_bin n_bin.
function vegas_refine_discrete!(cdf::Vector{Float64}, hist_bin::Vector{Float64}; alpha::Float64=0.5, floor::Float64=0.05)
    length(hist_bin) == length(cdf) - 1 || error("hist_bin must hold n_bin entries for a cdf of n_bin + 1")
    _fdg_check(ccall((:fdg_vegas_refine_discrete, _libfdg), Cint, (Ptr{Float64}, Ptr{Float64}, UInt32, Float64, Float64),
        cdf, hist_bin, length(hist_bin), alpha, floor))
    return cdf
end
# ---- spherical momentum variables (include/fdg.h; no counterpart in the reference: the caller's side of example/benchmark.jl:46) ---- #
# K = MCIntegration.FermiK(dim, kF, 0.2 kF, 10 kF): a group of 2 or 3 consecutive VEGAS variables is (k, phi) or (k, theta, phi), and the
# sampler writes the Cartesian components.  polar: a vector of (var, cols) with var the group's first variable (1-based) and cols its 2 or
# 3 columns of x (1-based); a fdg_vegas_polar is five UInt32 (var, dim, col[3]).  d_cdf = C_NULL: no discrete variable (d_bin may be C_NULL).
function vegas_sample_device_polar!(d_x::Ptr{Float64}, d_jac::Ptr{Float64}, d_grid::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer,
    polar::AbstractVector; col::Union{Nothing,AbstractVector{<:Integer}}=nothing, d_cdf::Ptr{Float64}=Ptr{Float64}(C_NULL), n_bin::Integer=1,
    d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), d_ext::Ptr{Float64}=Ptr{Float64}(C_NULL), ext_col::AbstractVector{<:Integer}=Int[],
    bin_base::Integer=1, seed::Integer=0, sample_offset::Integer=0, x_strides=(1, B), d_cell::Ptr{Int32}=Ptr{Int32}(C_NULL),
    stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    e = UInt32.(ext_col .- 1)
    p = zeros(UInt32, 5 * max(length(polar), 1))
    for (g, (var, cols)) in enumerate(polar)
        length(cols) in (2, 3) || error("a polar group has 2 or 3 columns")
        p[5g-4] = var - 1
        p[5g-3] = length(cols)
        p[5g-2:5g-3+length(cols)] .= UInt32.(cols .- 1)
    end
    _fdg_check(ccall((:fdg_vegas_sample_device_polar, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, Ptr{Float64}, UInt32, Int32, Ptr{Float64}, UInt32, Ptr{UInt32}, Ptr{UInt32}, UInt32, UInt64,
         UInt64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, d_cdf, n_bin, bin_base, d_ext, length(e), isempty(e) ? C_NULL : e,
        isempty(polar) ? C_NULL : p, length(polar), seed, sample_offset, d_x, x_strides[1], x_strides[2], d_jac, d_bin, d_cell, B, stream))
    return nothing
end
# (sin x, cos x) for 0 <= x <= 2 pi by the routine the polar sampler uses (fdg_sincos): the same bits on host and device.
function fdg_sincos(x::Float64)
    s, c = Ref{Float64}(0.0), Ref{Float64}(0.0)
    ccall((:fdg_sincos, _libfdg), Cvoid, (Float64, Ref{Float64}, Ref{Float64}), x, s, c)
    return s[], c[]
end
# ---- projection onto Matsubara frequencies (include/fdg.h; no counterpart in the reference: the caller's side of test/ver4.jl:193) ---- #
# (sin, cos) of omega_n tau by the routine the projection pass uses (fdg_matsubara_phase): omega_n = (2n+1) pi / beta or 2n pi / beta.
function fdg_matsubara_phase(tau::Float64, beta::Float64, n::Integer; fermionic::Bool=true)
    s, c = Ref{Float64}(0.0), Ref{Float64}(0.0)
    ccall((:fdg_matsubara_phase, _libfdg), Cvoid, (Float64, Float64, Int32, Cint, Ref{Float64}, Ref{Float64}), tau, beta, n, fermionic ? 1 : 0, s, c)
    return s[], c[]
end
struct _FdgMatsubara
    n_freq::UInt32
    fermionic::Int32
    freq::Ptr{Int32}
    root_tau_in::Ptr{Int32}
    root_tau_out::Ptr{Int32}
    beta::Float64
    d_T::Ptr{Float64}
    t_sample_stride::Int64
    t_comp_stride::Int64
    n_tau::UInt32
    d_acc_re::Ptr{Float64}
    d_acc_im::Ptr{Float64}
    d_acc2_re::Ptr{Float64}
    d_acc2_im::Ptr{Float64}
end
# Root k times e^{i omega_n (T[tau_out[k]] - T[tau_in[k]])} summed per (root, frequency, bin): d_sums points at four R x n_freq x n_bin
# arrays in a row (real parts, imaginary parts, their squares).  d_bin = C_NULL: one bin.  d_acc / d_acc2 (both or neither): the
# unprojected moments as accumulate_device_moments! leaves them.  n_dim = 0 and d_hist = C_NULL: no training; otherwise d_hist (and
# d_hist_bin) as accumulate_device_vegas[_binned]! leave them.  d_T is B x n_tau column-major by default.
function accumulate_device_matsubara!(f::GraphFunc, d_sums::Ptr{Float64}, d_leaf::Ptr{Float64}, d_T::Ptr{Float64}, freq::Vector{Int},
    root_tau_in::Vector{Int}, root_tau_out::Vector{Int}, B::Integer; beta::Float64, n_tau::Integer, fermionic::Bool=true,
    d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), n_bin::Integer=1, bin_base::Integer=1, d_weight::Ptr{Float64}=Ptr{Float64}(C_NULL),
    coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0, n_dim::Integer=0, n_grid::Integer=0,
    d_acc::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc2::Ptr{Float64}=Ptr{Float64}(C_NULL), d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL), leaf_strides=(1, B), tile_stride::Integer=0, t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    a = [Int32.(v) for v in (freq, root_tau_in, root_tau_out)]
    n = 8 * n_bin * length(freq) * length(root_tau_in)
    GC.@preserve a begin
        mz = _FdgMatsubara(length(freq), fermionic ? 1 : 0, pointer(a[1]), pointer(a[2]), pointer(a[3]), beta, d_T, t_strides[1], t_strides[2],
            n_tau, d_sums, d_sums + n, d_sums + 2n, d_sums + 3n)
        _fdg_check(ccall((:fdg_accumulate_device_matsubara, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32,
             UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{_FdgMatsubara}, Int64, Ptr{Cvoid}),
            f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight,
            coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, mz, B, stream))
    end
    return nothing
end
# the same for the fused step (fdg_mc_accumulate_device_matsubara): the phases are taken of the call's own T
function mc_accumulate_device_matsubara!(f::GraphFunc, d_sums::Ptr{Float64}, d_K::Ptr{Float64}, d_T::Ptr{Float64}, freq::Vector{Int},
    root_tau_in::Vector{Int}, root_tau_out::Vector{Int}, B::Integer; kF::Float64, beta::Float64, lambda::Float64, n_tau::Integer,
    fermionic::Bool=true, d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), n_bin::Integer=1, bin_base::Integer=1,
    d_weight::Ptr{Float64}=Ptr{Float64}(C_NULL), coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    n_dim::Integer=0, n_grid::Integer=0, d_acc::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc2::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL), d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL), k_strides=(1, B), t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    a = [Int32.(v) for v in (freq, root_tau_in, root_tau_out)]
    n = 8 * n_bin * length(freq) * length(root_tau_in)
    GC.@preserve a begin
        mz = _FdgMatsubara(length(freq), fermionic ? 1 : 0, pointer(a[1]), pointer(a[2]), pointer(a[3]), beta, Ptr{Float64}(C_NULL), 0, 0,
            n_tau, d_sums, d_sums + n, d_sums + 2n, d_sums + 3n)
        _fdg_check(ccall((:fdg_mc_accumulate_device_matsubara, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32,
             Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ref{_FdgMatsubara}, Int64, Ptr{Cvoid}),
            f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight,
            coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, mz, B, stream))
    end
    return nothing
end
# ---- weight groups (include/fdg.h; no counterpart in the reference: the caller's side of test/hubbard.jl:81-85) ---- #
# MCIntegration's dof: root i is weighted by the jacobian of its own variables only.  dof[i][p] = how many leading elements of variable
# pool p root i integrates, pools[p] = the VEGAS variables (1-based) of each element of the pool; roots with equal sets share a group.
# Returns (root_group::Vector{UInt32} 0-based, var_mask::Vector{UInt64}).
function weight_groups_from_dof(dof::AbstractVector, pools::AbstractVector)
    masks = UInt64[]
    root_group = UInt32[]
    for row in dof
        length(row) == length(pools) || error("dof holds one count per pool")
        m = UInt64(0)
        for (n, pool) in zip(row, pools)
            0 <= n <= length(pool) || error("dof asks for more elements than the pool holds")
            for element in pool[1:n], d in element
                m |= UInt64(1) << (d - 1)
            end
        end
        g = findfirst(==(m), masks)
        if g === nothing
            push!(masks, m)
            g = length(masks)
        end
        push!(root_group, g - 1)
    end
    return root_group, masks
end
struct _FdgWeightGroups
    n_group::UInt32
    root_group::Ptr{UInt32}
    var_mask::Ptr{UInt64}
    weight_group_stride::Int64
end
# vegas_sample_device_polar! with one jacobian per weight group: d_jac is B x n_group column-major by default (jac_group_stride = B)
function vegas_sample_device_grouped!(d_x::Ptr{Float64}, d_jac::Ptr{Float64}, d_grid::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer,
    polar::AbstractVector, var_mask::Vector{UInt64}; jac_group_stride::Integer=B, col::Union{Nothing,AbstractVector{<:Integer}}=nothing,
    d_cdf::Ptr{Float64}=Ptr{Float64}(C_NULL), n_bin::Integer=1, d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), d_ext::Ptr{Float64}=Ptr{Float64}(C_NULL),
    ext_col::AbstractVector{<:Integer}=Int[], bin_base::Integer=1, seed::Integer=0, sample_offset::Integer=0, x_strides=(1, B),
    d_cell::Ptr{Int32}=Ptr{Int32}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    e = UInt32.(ext_col .- 1)
    p = zeros(UInt32, 5 * max(length(polar), 1))
    for (g, (var, cols)) in enumerate(polar)
        length(cols) in (2, 3) || error("a polar group has 2 or 3 columns")
        p[5g-4] = var - 1
        p[5g-3] = length(cols)
        p[5g-2:5g-3+length(cols)] .= UInt32.(cols .- 1)
    end
    _fdg_check(ccall((:fdg_vegas_sample_device_grouped, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, Ptr{Float64}, UInt32, Int32, Ptr{Float64}, UInt32, Ptr{UInt32}, Ptr{UInt32}, UInt32,
         Ptr{UInt64}, UInt32, Int64, UInt64, UInt64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, d_cdf, n_bin, bin_base, d_ext, length(e), isempty(e) ? C_NULL : e,
        isempty(polar) ? C_NULL : p, length(polar), var_mask, length(var_mask), jac_group_stride, seed, sample_offset, d_x, x_strides[1],
        x_strides[2], d_jac, d_bin, d_cell, B, stream))
    return nothing
end
# The accumulate step with weight groups: d_weight is B x n_group column-major by default, dof / pools as weight_groups_from_dof takes
# them.  Everything else as accumulate_device_matsubara! without a projection (these wrappers pass no descriptor): d_bin = C_NULL: one
# bin; n_dim = 0 and d_hist = C_NULL: no training.
function accumulate_device_grouped!(f::GraphFunc, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_leaf::Ptr{Float64}, d_weight::Ptr{Float64},
    B::Integer; dof::AbstractVector, pools::AbstractVector, weight_group_stride::Integer=B, d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL),
    n_bin::Integer=1, bin_base::Integer=1, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    n_dim::Integer=0, n_grid::Integer=0, d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL), d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL),
    leaf_strides=(1, B), tile_stride::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    root_group, var_mask = weight_groups_from_dof(dof, pools)
    GC.@preserve root_group var_mask begin
        wg = _FdgWeightGroups(length(var_mask), pointer(root_group), pointer(var_mask), weight_group_stride)
        _fdg_check(ccall((:fdg_accumulate_device_grouped, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32,
             UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ref{_FdgWeightGroups}, Int64, Ptr{Cvoid}),
            f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight,
            coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, C_NULL, wg, B, stream))
    end
    return nothing
end
# the same for the fused step (fdg_mc_accumulate_device_grouped)
function mc_accumulate_device_grouped!(f::GraphFunc, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_K::Ptr{Float64}, d_T::Ptr{Float64},
    d_weight::Ptr{Float64}, B::Integer; dof::AbstractVector, pools::AbstractVector, kF::Float64, beta::Float64, lambda::Float64,
    weight_group_stride::Integer=B, d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), n_bin::Integer=1, bin_base::Integer=1,
    coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0, n_dim::Integer=0, n_grid::Integer=0,
    d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL), d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL), k_strides=(1, B), t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    root_group, var_mask = weight_groups_from_dof(dof, pools)
    GC.@preserve root_group var_mask begin
        wg = _FdgWeightGroups(length(var_mask), pointer(root_group), pointer(var_mask), weight_group_stride)
        _fdg_check(ccall((:fdg_mc_accumulate_device_grouped, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32,
             Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Cvoid}, Ref{_FdgWeightGroups}, Int64, Ptr{Cvoid}),
            f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight,
            coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, C_NULL, wg, B, stream))
    end
    return nothing
end
# ---- stratified sampling with polar groups and weight groups (include/fdg.h: the _strat_grouped calls) ---- #
# vegas_sample_device_grouped! without a discrete variable, inside the strata of the sample's hypercube (strat, d_start, d_cube as
# vegas_sample_device_strat! takes them); every group's jacobian carries n_total / (H n_h).  var_mask empty: one jacobian, the full
# fold.  Unverified: there is no Julia in the image these wrappers were written in.
function vegas_sample_device_strat_grouped!(d_x::Ptr{Float64}, d_jac::Ptr{Float64}, d_cube::Ptr{Int32}, d_grid::Ptr{Float64},
    n_dim::Integer, n_grid::Integer, B::Integer, polar::AbstractVector, var_mask::Vector{UInt64}, strat::AbstractVector{<:Integer},
    d_start::Ptr{Int64}; jac_group_stride::Integer=B, col::Union{Nothing,AbstractVector{<:Integer}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, x_strides=(1, B), d_cell::Ptr{Int32}=Ptr{Int32}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    sv = UInt32.(strat)
    p = zeros(UInt32, 5 * max(length(polar), 1))
    for (g, (var, cols)) in enumerate(polar)
        length(cols) in (2, 3) || error("a polar group has 2 or 3 columns")
        p[5g-4] = var - 1
        p[5g-3] = length(cols)
        p[5g-2:5g-3+length(cols)] .= UInt32.(cols .- 1)
    end
    _fdg_check(ccall((:fdg_vegas_sample_device_strat_grouped, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, Ptr{UInt32}, UInt32, Ptr{UInt64}, UInt32, Int64, Ptr{UInt32}, Ptr{Int64}, UInt64,
         UInt64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, isempty(polar) ? C_NULL : p, length(polar),
        isempty(var_mask) ? C_NULL : var_mask, length(var_mask), jac_group_stride, sv, d_start, seed, sample_offset, d_x, x_strides[1],
        x_strides[2], d_jac, d_cube, d_cell, B, stream))
    return nothing
end
# accumulate_device_strat! with weight groups: d_weight is B x n_group column-major by default, d_cube_sum, d_cube_sum2
# ((R + n_group) x H each, added to; row R + g the combination of group g's roots).
function accumulate_device_strat_grouped!(f::GraphFunc, d_leaf::Ptr{Float64}, d_weight::Ptr{Float64}, d_acc::Ptr{Float64},
    d_acc2::Ptr{Float64}, d_hist::Ptr{Float64}, strat::AbstractVector{<:Integer}, d_cube::Ptr{Int32}, d_cube_sum::Ptr{Float64},
    d_cube_sum2::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer; dof::AbstractVector, pools::AbstractVector,
    weight_group_stride::Integer=B, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    leaf_strides=(1, B), tile_stride::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    sv = UInt32.(strat)
    root_group, var_mask = weight_groups_from_dof(dof, pools)
    GC.@preserve root_group var_mask begin
        wg = _FdgWeightGroups(length(var_mask), pointer(root_group), pointer(var_mask), weight_group_stride)
        _fdg_check(ccall((:fdg_accumulate_device_strat_grouped, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{UInt32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ref{_FdgWeightGroups}, Int64, Ptr{Cvoid}),
            f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_weight, coef === nothing ? C_NULL : coef, seed,
            sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, sv, d_cube, d_cube_sum, d_cube_sum2, wg, B, stream))
    end
    return nothing
end
function mc_accumulate_device_strat_grouped!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_weight::Ptr{Float64},
    d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_hist::Ptr{Float64}, strat::AbstractVector{<:Integer}, d_cube::Ptr{Int32},
    d_cube_sum::Ptr{Float64}, d_cube_sum2::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer; dof::AbstractVector,
    pools::AbstractVector, kF::Float64, beta::Float64, lambda::Float64, weight_group_stride::Integer=B,
    coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0, k_strides=(1, B), t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    sv = UInt32.(strat)
    root_group, var_mask = weight_groups_from_dof(dof, pools)
    GC.@preserve root_group var_mask begin
        wg = _FdgWeightGroups(length(var_mask), pointer(root_group), pointer(var_mask), weight_group_stride)
        _fdg_check(ccall((:fdg_mc_accumulate_device_strat_grouped, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64},
             UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
             Ref{_FdgWeightGroups}, Int64, Ptr{Cvoid}),
            f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_weight,
            coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, sv, d_cube, d_cube_sum,
            d_cube_sum2, wg, B, stream))
    end
    return nothing
end
# Observables: linear combinations of the roots and their covariance (fdg_accumulate_device_observables).  coef is n_root x n_obs
# column-major (coef[k, m]: the factor of root k in observable m -- the C side's row-major [n_obs][n_root]); d_obs is n_obs x n_bin and
# d_cov n_obs x n_obs x n_bin column-major, both added to.  d_acc = d_acc2 = C_NULL: no per-root moments.  These wrappers pass one
# weight column (or none) and neither a projection nor weight groups.  Unverified: written against the header, never run.
struct _FdgObservables
    n_obs::UInt32
    coef::Ptr{Float64}
    d_obs::Ptr{Float64}
    d_cov::Ptr{Float64}
end
function accumulate_device_observables!(f::GraphFunc, d_obs::Ptr{Float64}, d_cov::Ptr{Float64}, coef::Matrix{Float64}, d_leaf::Ptr{Float64},
    B::Integer; d_weight::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_acc2::Ptr{Float64}=Ptr{Float64}(C_NULL), d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), n_bin::Integer=1, bin_base::Integer=1,
    train_coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0, n_dim::Integer=0, n_grid::Integer=0,
    d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL), d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL), leaf_strides=(1, B), tile_stride::Integer=0,
    stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve coef begin
        ob = _FdgObservables(size(coef, 2), pointer(coef), d_obs, d_cov)
        _fdg_check(ccall((:fdg_accumulate_device_observables, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32,
             UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{_FdgObservables}, Int64, Ptr{Cvoid}),
            f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight,
            train_coef === nothing ? C_NULL : train_coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, C_NULL, C_NULL,
            ob, B, stream))
    end
    return nothing
end
# the same for the fused step (fdg_mc_accumulate_device_observables)
function mc_accumulate_device_observables!(f::GraphFunc, d_obs::Ptr{Float64}, d_cov::Ptr{Float64}, coef::Matrix{Float64}, d_K::Ptr{Float64},
    d_T::Ptr{Float64}, B::Integer; kF::Float64, beta::Float64, lambda::Float64, d_weight::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_acc::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc2::Ptr{Float64}=Ptr{Float64}(C_NULL), d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL),
    n_bin::Integer=1, bin_base::Integer=1, train_coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    n_dim::Integer=0, n_grid::Integer=0, d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL), d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL),
    k_strides=(1, B), t_strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve coef begin
        ob = _FdgObservables(size(coef, 2), pointer(coef), d_obs, d_cov)
        _fdg_check(ccall((:fdg_mc_accumulate_device_observables, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32,
             Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Cvoid}, Ptr{Cvoid}, Ref{_FdgObservables}, Int64, Ptr{Cvoid}),
            f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight,
            train_coef === nothing ? C_NULL : train_coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, C_NULL, C_NULL,
            ob, B, stream))
    end
    return nothing
end
# Frequency observables: linear combinations of the PROJECTED roots and their covariance (fdg_accumulate_device_freq_observables).
# coef is n_root x M column-major (coef[k, m]: the real factor of root k in observable m); d_fobs is 2M x n_freq x n_bin and d_fcov
# 2M x 2M x n_freq x n_bin column-major (the components Re o_1 .. Re o_M, Im o_1 .. Im o_M), both added to.  The frequencies, the
# roots' time labels (1-based), beta and T as accumulate_device_matsubara! takes them; d_sums = C_NULL: no per-root projected sums,
# else the four arrays in a row as there.  These wrappers pass one weight column (or none), no weight groups and no unprojected
# observables.  Unverified: written against the header, never run.
struct _FdgFreqObservables
    n_obs::UInt32
    coef::Ptr{Float64}
    d_fobs::Ptr{Float64}
    d_fcov::Ptr{Float64}
end
function accumulate_device_freq_observables!(f::GraphFunc, d_fobs::Ptr{Float64}, d_fcov::Ptr{Float64}, coef::Matrix{Float64},
    d_leaf::Ptr{Float64}, d_T::Ptr{Float64}, freq::Vector{Int}, root_tau_in::Vector{Int}, root_tau_out::Vector{Int}, B::Integer;
    beta::Float64, n_tau::Integer, fermionic::Bool=true, d_sums::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_weight::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc2::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), n_bin::Integer=1, bin_base::Integer=1, train_coef::Union{Nothing,Vector{Float64}}=nothing,
    seed::Integer=0, sample_offset::Integer=0, n_dim::Integer=0, n_grid::Integer=0, d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL), leaf_strides=(1, B), tile_stride::Integer=0, t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    a = [Int32.(v) for v in (freq, root_tau_in, root_tau_out)]
    n = d_sums == C_NULL ? 0 : 8 * n_bin * length(freq) * length(root_tau_in)
    GC.@preserve a coef begin
        mz = _FdgMatsubara(length(freq), fermionic ? 1 : 0, pointer(a[1]), pointer(a[2]), pointer(a[3]), beta, d_T, t_strides[1], t_strides[2],
            n_tau, d_sums, d_sums + n, d_sums + 2n, d_sums + 3n)
        fo = _FdgFreqObservables(size(coef, 2), pointer(coef), d_fobs, d_fcov)
        _fdg_check(ccall((:fdg_accumulate_device_freq_observables, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32,
             UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{_FdgMatsubara}, Ptr{Cvoid}, Ptr{Cvoid},
             Ref{_FdgFreqObservables}, Int64, Ptr{Cvoid}),
            f.handle, d_leaf, leaf_strides[1], leaf_strides[2], tile_stride, d_bin, bin_base, n_bin, d_weight,
            train_coef === nothing ? C_NULL : train_coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, mz, C_NULL,
            C_NULL, fo, B, stream))
    end
    return nothing
end
# the same for the fused step (fdg_mc_accumulate_device_freq_observables): the phases are taken of the call's own T
function mc_accumulate_device_freq_observables!(f::GraphFunc, d_fobs::Ptr{Float64}, d_fcov::Ptr{Float64}, coef::Matrix{Float64},
    d_K::Ptr{Float64}, d_T::Ptr{Float64}, freq::Vector{Int}, root_tau_in::Vector{Int}, root_tau_out::Vector{Int}, B::Integer;
    kF::Float64, beta::Float64, lambda::Float64, n_tau::Integer, fermionic::Bool=true, d_sums::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_weight::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc::Ptr{Float64}=Ptr{Float64}(C_NULL), d_acc2::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), n_bin::Integer=1, bin_base::Integer=1, train_coef::Union{Nothing,Vector{Float64}}=nothing,
    seed::Integer=0, sample_offset::Integer=0, n_dim::Integer=0, n_grid::Integer=0, d_hist::Ptr{Float64}=Ptr{Float64}(C_NULL),
    d_hist_bin::Ptr{Float64}=Ptr{Float64}(C_NULL), k_strides=(1, B), t_strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    a = [Int32.(v) for v in (freq, root_tau_in, root_tau_out)]
    n = d_sums == C_NULL ? 0 : 8 * n_bin * length(freq) * length(root_tau_in)
    GC.@preserve a coef begin
        mz = _FdgMatsubara(length(freq), fermionic ? 1 : 0, pointer(a[1]), pointer(a[2]), pointer(a[3]), beta, Ptr{Float64}(C_NULL), 0, 0,
            n_tau, d_sums, d_sums + n, d_sums + 2n, d_sums + 3n)
        fo = _FdgFreqObservables(size(coef, 2), pointer(coef), d_fobs, d_fcov)
        _fdg_check(ccall((:fdg_mc_accumulate_device_freq_observables, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32,
             Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ref{_FdgMatsubara}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{_FdgFreqObservables}, Int64, Ptr{Cvoid}),
            f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight,
            train_coef === nothing ? C_NULL : train_coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, mz, C_NULL,
            C_NULL, fo, B, stream))
    end
    return nothing
end
# device memory for a batch, backed by physical chunks of `chunk_bytes` (0: one allocation): fdg_batch_alloc / fdg_batch_free
function batch_alloc(bytes::Integer; chunk_bytes::Integer=0)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    _fdg_check(ccall((:fdg_batch_alloc, _libfdg), Cint, (Csize_t, Csize_t, Ref{Ptr{Cvoid}}), bytes, chunk_bytes, p))
    return p[]
end
batch_free(p::Ptr{Cvoid}) = _fdg_check(ccall((:fdg_batch_free, _libfdg), Cint, (Ptr{Cvoid},), p))

# The two arrays of a tile-major batch of `f` -- Array{Float64,3}(64, L, T) and (64, R, T) on the device -- with the root chunks chosen by
# timing f's own kernel on (leaf window, root chunk) pairs (fdg_batch_alloc_pair, include/fdg.h).  Returns (d_leaf, d_root, info bytes);
# release each pointer with batch_free.  What a Monte-Carlo driver that evaluates (not only accumulates) should allocate its batch with.
# layout = :leaf_major: a Julia Matrix pair B' x L / B' x R (B' = 64 * the info's chunk_tiles), for batches of up to a few tens of GB; :row_major: compile_Python's.
function batch_alloc_pair(f::GraphFunc, n_sample::Integer; chunk_bytes::Integer=0, calibrate::Bool=true, layout::Symbol=:tile_major)
    dl = Ref{Ptr{Cvoid}}(C_NULL); dr = Ref{Ptr{Cvoid}}(C_NULL)
    info = zeros(UInt8, 128)                 # fdg_batch_pair_info (120 bytes; the last two UInt32: level_reached -- 3 the full search, 2 a span cut
                                             # short by the free memory, 1 mapped in draw order, 0 not calibrated -- and span_gb)
    _fdg_check(ccall((:fdg_batch_alloc_pair, _libfdg), Cint, (Ptr{Cvoid}, Int64, Csize_t, Cuint, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{UInt8}),
        f.handle, n_sample, chunk_bytes, Cuint((calibrate ? 1 : 0) | (layout == :row_major ? 8 : 0) | (layout == :leaf_major ? 16 : 0)), dl, dr, info))
    return Ptr{Float64}(dl[]), Ptr{Float64}(dr[]), info
end

# tile_major!(d_tiled, d_src, B, C; strides): a device matrix in one of the reference's layouts -- a Julia column-major B x C Matrix{Float64}
# (strides = (1, B), the default) or compile_Python's row-major [B, C] (strides = (C, 1)) -- into the tile-major Array{Float64,3}(64, C, cld(B, 64))
# that eval_device_tiled! takes; from_tile_major! is the way back (roots).  One pass at copy speed each (fdg_repack_tile_major / fdg_unpack_tile_major):
# worth it for a batch that is evaluated several times; a producer that can write tile-major itself (the fused Monte-Carlo step does) should.
function tile_major!(d_tiled::Ptr{Float64}, d_src::Ptr{Float64}, B::Integer, C::Integer; strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_repack_tile_major, _libfdg), Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, UInt32, Ptr{Cvoid}),
        d_src, strides[1], strides[2], d_tiled, B, UInt32(C), stream))
end
function from_tile_major!(d_dst::Ptr{Float64}, d_tiled::Ptr{Float64}, B::Integer, C::Integer; strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_unpack_tile_major, _libfdg), Cint, (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, UInt32, Ptr{Cvoid}),
        d_tiled, d_dst, strides[1], strides[2], B, UInt32(C), stream))
end

# Options of a handle (what used to be FDG_* environment switches; the library reads the environment once per process): set_option!(f, "FDG_ISA_NO_POOL", "1")
set_option!(f::GraphFunc, name::AbstractString, value::AbstractString) =
    _fdg_check(ccall((:fdg_graph_set_option, _libfdg), Cint, (Ptr{Cvoid}, Cstring, Cstring), f.handle, name, value))
unset_option!(f::GraphFunc, name::AbstractString) =
    _fdg_check(ccall((:fdg_graph_set_option, _libfdg), Cint, (Ptr{Cvoid}, Cstring, Ptr{UInt8}), f.handle, name, C_NULL))

# acc[k] += sum_b weight[b] * root_k(b), everything on device
function accumulate_device!(f::GraphFunc, d_acc::Ptr{Float64}, d_leaf::Ptr{Float64}, d_weight::Ptr{Float64}, B::Integer;
    leaf_strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_accumulate_device, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_leaf, leaf_strides[1], leaf_strides[2], d_weight, d_acc, B, stream))
end

export compile_hip, GraphFunc, eval_device!, accumulate_device!, eval_device_tiled!, accumulate_device_tiled!, accumulate_device_binned!, mc_accumulate_device_binned!, accumulate_device_moments!, mc_accumulate_device_moments!, vegas_sample_device!, accumulate_device_vegas!, mc_accumulate_device_vegas!, vegas_refine!, vegas_sample_device_discrete!, accumulate_device_vegas_binned!, mc_accumulate_device_vegas_binned!, vegas_refine_discrete!, vegas_sample_device_polar!, fdg_sincos, fdg_matsubara_phase, accumulate_device_matsubara!, mc_accumulate_device_matsubara!, weight_groups_from_dof, vegas_sample_device_grouped!, accumulate_device_grouped!, mc_accumulate_device_grouped!, accumulate_device_observables!, mc_accumulate_device_observables!, accumulate_device_freq_observables!, mc_accumulate_device_freq_observables!, batch_alloc, batch_free, tile_major!, from_tile_major!, vegas_sample_device_strat!, accumulate_device_strat!, mc_accumulate_device_strat!, strat_allocate!, strat_allocate_cols!, vegas_sample_device_strat_grouped!, accumulate_device_strat_grouped!, mc_accumulate_device_strat_grouped!

# ---- Markov-chain sampling on the VEGAS map (include/fdg.h; no counterpart in the reference: the caller's side of test/hubbard.jl:85) ---- #
# The state of B walkers is caller-owned device memory, every array a column-major Julia matrix with the walker as its first index:
# d_x (B x n_col), d_fac (B x n_dim), d_root (B x R), d_a (B), d_sum (B x (R + 1)), d_n_accept (B Int32, optional).
# chain_propose_device! writes the proposal d_xp, d_facp: the variables of `mask` (bit d - 1 = variable d) redrawn through the map for the
# counters (sample_offset + b, d), everything else copied from the state.  col is 1-based (default d).
const FDG_CHAIN_INIT = Cuint(1)
const FDG_CHAIN_MEASURE = Cuint(2)
function chain_propose_device!(d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64}, d_grid::Ptr{Float64},
    n_dim::Integer, n_grid::Integer, n_col::Integer, mask::Integer, B::Integer; col::Union{Nothing,AbstractVector{<:Integer}}=nothing,
    seed::Integer=0, sample_offset::Integer=0, x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    _fdg_check(ccall((:fdg_chain_propose_device, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, UInt32, UInt64, UInt64, UInt64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Float64}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride,
        d_facp, B, stream))
    return nothing
end
# One step after the proposal (fdg_chain_step_device, the leaf form: the columns of d_xp are the graph's leaves): the roots of the
# proposals, the fold, the accept rule u * (a + gamma) < (a' + gamma), the selection into the state and, with FDG_CHAIN_MEASURE, the
# walker's sums d_sum[b, k] += (jac * r_k) / (a + gamma), d_sum[b, R + 1] += 1 / (a + gamma).  FDG_CHAIN_INIT accepts unconditionally.
function chain_step_device!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer, gamma::Float64, B::Integer;
    flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_chain_step_device, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64, Cuint, Ptr{Float64}, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        f.handle, d_xp, xp_col_stride, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed, sample_offset, flags, d_x,
        x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, B, stream))
    return nothing
end
# The Monte-Carlo form (fdg_mc_chain_step_device): d_xp is one B x (n_loop * dim + n_tau) matrix, momentum components first, then the times.
function mc_chain_step_device!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer, gamma::Float64, B::Integer;
    kF::Float64, beta::Float64, lambda::Float64, flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B,
    stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_mc_chain_step_device, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Float64, Float64, Float64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64,
         Cuint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        f.handle, d_xp, xp_col_stride, kF, beta, lambda, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed,
        sample_offset, flags, d_x, x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, B, stream))
    return nothing
end
# The same two steps with the Matsubara projection inside the chain (fdg_[mc_]chain_step_device_matsubara): the weight is
# |jac sum_k c_k r_k e^{i omega tau_k}| at freq[weight_freq] (1-based here), and every root is measured at every frequency into d_sum,
# B x (2 F R + 1): column 2 ((f - 1) R + k - 1) + 1 the real part, the next one the imaginary part, the last one 1 / (a + gamma).
# root_col_in / root_col_out: the 1-based columns of d_x that hold the two times of every root.
struct _FdgChainMatsubara
    n_freq::UInt32
    fermionic::Int32
    freq::Ptr{Int32}
    weight_freq::UInt32
    root_col_in::Ptr{UInt32}
    root_col_out::Ptr{UInt32}
    beta::Float64
end
function chain_step_device_matsubara!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer, gamma::Float64, freq::Vector{Int},
    root_col_in::Vector{Int}, root_col_out::Vector{Int}, B::Integer; beta::Float64, fermionic::Bool=true, weight_freq::Integer=1,
    flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    fr, cin, cout = Int32.(freq), UInt32.(root_col_in .- 1), UInt32.(root_col_out .- 1)
    GC.@preserve fr cin cout begin
        mz = _FdgChainMatsubara(length(fr), fermionic ? 1 : 0, pointer(fr), weight_freq - 1, pointer(cin), pointer(cout), beta)
        _fdg_check(ccall((:fdg_chain_step_device_matsubara, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64, Cuint, Ptr{Float64}, Int64,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{_FdgChainMatsubara}, Int64, Ptr{Cvoid}),
            f.handle, d_xp, xp_col_stride, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed, sample_offset, flags, d_x,
            x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, mz, B, stream))
    end
    return nothing
end
function mc_chain_step_device_matsubara!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer, gamma::Float64, freq::Vector{Int},
    root_col_in::Vector{Int}, root_col_out::Vector{Int}, B::Integer; kF::Float64, beta::Float64, lambda::Float64, fermionic::Bool=true,
    weight_freq::Integer=1, flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    fr, cin, cout = Int32.(freq), UInt32.(root_col_in .- 1), UInt32.(root_col_out .- 1)
    GC.@preserve fr cin cout begin
        mz = _FdgChainMatsubara(length(fr), fermionic ? 1 : 0, pointer(fr), weight_freq - 1, pointer(cin), pointer(cout), beta)
        _fdg_check(ccall((:fdg_mc_chain_step_device_matsubara, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Float64, Float64, Float64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64,
             Cuint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{_FdgChainMatsubara}, Int64,
             Ptr{Cvoid}),
            f.handle, d_xp, xp_col_stride, kF, beta, lambda, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed,
            sample_offset, flags, d_x, x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, mz, B, stream))
    end
    return nothing
end
# The same two steps with weight groups (fdg_[mc_]chain_step_device_grouped): the weight is a = sum_g rho_g |jac_g s_g| with jac_g the
# jacobian of the variables of group g only, and root k is measured with the jacobian of its own group.  dof / pools as
# weight_groups_from_dof takes them; reweight: one factor > 0 per group, or nothing (no factor is applied).  These wrappers pass no
# projection (mz = C_NULL), so d_sum is B x (R + 1).  Unverified: written against the header, never run.
struct _FdgChainGroups
    n_group::UInt32
    root_group::Ptr{UInt32}
    var_mask::Ptr{UInt64}
    reweight::Ptr{Float64}
end
function chain_step_device_grouped!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer, gamma::Float64, B::Integer;
    dof::AbstractVector, pools::AbstractVector, reweight::Union{Nothing,Vector{Float64}}=nothing, flags::Integer=0,
    coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0,
    d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    root_group, var_mask = weight_groups_from_dof(dof, pools)
    rw = reweight === nothing ? Float64[] : reweight
    GC.@preserve root_group var_mask rw begin
        cg = _FdgChainGroups(length(var_mask), pointer(root_group), pointer(var_mask), reweight === nothing ? Ptr{Float64}(C_NULL) : pointer(rw))
        _fdg_check(ccall((:fdg_chain_step_device_grouped, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64, Cuint, Ptr{Float64}, Int64,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{_FdgChainGroups}, Int64, Ptr{Cvoid}),
            f.handle, d_xp, xp_col_stride, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed, sample_offset, flags, d_x,
            x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, C_NULL, cg, B, stream))
    end
    return nothing
end
function mc_chain_step_device_grouped!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer, gamma::Float64, B::Integer;
    dof::AbstractVector, pools::AbstractVector, kF::Float64, beta::Float64, lambda::Float64,
    reweight::Union{Nothing,Vector{Float64}}=nothing, flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B,
    stream::Ptr{Cvoid}=C_NULL)
    root_group, var_mask = weight_groups_from_dof(dof, pools)
    rw = reweight === nothing ? Float64[] : reweight
    GC.@preserve root_group var_mask rw begin
        cg = _FdgChainGroups(length(var_mask), pointer(root_group), pointer(var_mask), reweight === nothing ? Ptr{Float64}(C_NULL) : pointer(rw))
        _fdg_check(ccall((:fdg_mc_chain_step_device_grouped, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Float64, Float64, Float64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64,
             Cuint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{_FdgChainGroups},
             Int64, Ptr{Cvoid}),
            f.handle, d_xp, xp_col_stride, kF, beta, lambda, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed,
            sample_offset, flags, d_x, x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, C_NULL, cg, B, stream))
    end
    return nothing
end
# d_out (3 R + 2, added to) = the sums over the walkers S_c, Q_c = sum A_c^2 (R + 1 each) and X_k = sum A_k A_{R+1} (R) of d_sum.
function chain_reduce_device!(d_out::Ptr{Float64}, d_sum::Ptr{Float64}, n_root::Integer, B::Integer; stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_chain_reduce_device, _libfdg), Cint, (Ptr{Float64}, UInt32, Int64, Ptr{Float64}, Ptr{Cvoid}),
        d_sum, n_root, B, d_out, stream))
    return nothing
end
export chain_propose_device!, chain_step_device!, mc_chain_step_device!, chain_reduce_device!, FDG_CHAIN_INIT, FDG_CHAIN_MEASURE
# Observables of the chain (fdg_chain_reduce_device_observables): d_out ((M + 1) + (M + 1)(M + 2) / 2, added to) = the sums S_p and the
# packed upper triangle P_pq of the rows coef (M x n_use, HOST, row m the factors of observable m) over the window of n_use columns of
# d_sum that starts at the 0-based column col_base, with the 0-based column norm_col as row M.  d_work holds
# chain_reduce_observables_work_bytes(M, n_use) bytes of device memory.  (The size query returns a size_t: it is bound with @ccall.)
const FDG_CHAIN_OBS_MAX = 16
const FDG_CHAIN_OBS_COL_MAX = 1024
const FDG_CHAIN_OBS_GROUPS = 1024
function chain_reduce_observables_work_bytes(n_obs::Integer, n_use::Integer)
    return Int(@ccall _libfdg.fdg_chain_reduce_observables_work_bytes(n_obs::UInt32, n_use::UInt32)::Csize_t)
end
function chain_reduce_device_observables!(d_out::Ptr{Float64}, d_sum::Ptr{Float64}, B::Integer, col_base::Integer, norm_col::Integer,
    coef::Matrix{Float64}, d_work::Ptr{Cvoid}; stream::Ptr{Cvoid}=C_NULL)
    n_obs, n_use = size(coef)
    rows = permutedims(coef)                                 # row-major [n_obs][n_use] for the C side
    _fdg_check(ccall((:fdg_chain_reduce_device_observables, _libfdg), Cint,
        (Ptr{Float64}, Int64, UInt32, UInt32, UInt32, Ptr{Float64}, UInt32, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
        d_sum, B, col_base, n_use, norm_col, rows, n_obs, d_out, d_work, stream))
    return nothing
end
export chain_reduce_observables_work_bytes, chain_reduce_device_observables!, FDG_CHAIN_OBS_MAX, FDG_CHAIN_OBS_COL_MAX, FDG_CHAIN_OBS_GROUPS
export chain_step_device_matsubara!, mc_chain_step_device_matsubara!
export chain_step_device_grouped!, mc_chain_step_device_grouped!
# The chain with one discrete external variable behind the continuous ones (fdg_chain_propose_device_discrete,
# fdg_[mc_]chain_step_device_binned): d_fac / d_facp are B x (n_dim + 1), the last column the factor 1 / p_j of the walker's value j,
# d_bin / d_binp (B Int32) hold the 0-based j, and d_sum is B x (n_bin R + 1): column j R + k root k at value j, the last one
# 1 / (a + gamma).  d_cdf (n_bin + 1) and d_ext (n_ext x n_bin, row j of the C table a column here) lie on the device; ext_col is
# 1-based.  dof / pools nothing: one group of every root and every variable.  These wrappers pass no projection (mz = C_NULL).
# Unverified: written against the header, never run.
function chain_propose_device_discrete!(d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_binp::Ptr{Int32}, d_x::Ptr{Float64}, d_fac::Ptr{Float64},
    d_bin::Ptr{Int32}, d_grid::Ptr{Float64}, d_cdf::Ptr{Float64}, n_dim::Integer, n_grid::Integer, n_bin::Integer, n_col::Integer,
    mask::Integer, move_discrete::Bool, B::Integer; col::Union{Nothing,AbstractVector{<:Integer}}=nothing,
    d_ext::Ptr{Float64}=Ptr{Float64}(C_NULL), ext_col::AbstractVector{<:Integer}=Int[], seed::Integer=0, sample_offset::Integer=0,
    x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    ec = UInt32.(ext_col .- 1)
    _fdg_check(ccall((:fdg_chain_propose_device_discrete, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, UInt32, UInt64, UInt64, UInt64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Float64}, Cint, Ptr{Float64}, UInt32, Ptr{Float64}, UInt32, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride,
        d_facp, move_discrete ? 1 : 0, d_cdf, n_bin, d_ext, length(ec), isempty(ec) ? C_NULL : ec, d_bin, d_binp, B, stream))
    return nothing
end
function chain_step_device_binned!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_binp::Ptr{Int32}, d_x::Ptr{Float64},
    d_fac::Ptr{Float64}, d_bin::Ptr{Int32}, d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer,
    n_bin::Integer, gamma::Float64, B::Integer; dof::Union{Nothing,AbstractVector}=nothing, pools::Union{Nothing,AbstractVector}=nothing,
    reweight::Union{Nothing,Vector{Float64}}=nothing, flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B,
    stream::Ptr{Cvoid}=C_NULL)
    root_group, var_mask = dof === nothing ? (UInt32[], UInt64[]) : weight_groups_from_dof(dof, pools)
    rw = reweight === nothing ? Float64[] : reweight
    GC.@preserve root_group var_mask rw begin
        cg = Ref(_FdgChainGroups(length(var_mask), pointer(root_group), pointer(var_mask), reweight === nothing ? Ptr{Float64}(C_NULL) : pointer(rw)))
        _fdg_check(ccall((:fdg_chain_step_device_binned, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64, Cuint, Ptr{Float64}, Int64,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Ptr{Int32}, Ptr{Int32}, Int64,
             Ptr{Cvoid}),
            f.handle, d_xp, xp_col_stride, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed, sample_offset, flags, d_x,
            x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, C_NULL, dof === nothing ? C_NULL : cg, n_bin, d_binp, d_bin, B, stream))
    end
    return nothing
end
function mc_chain_step_device_binned!(f::GraphFunc, d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_binp::Ptr{Int32}, d_x::Ptr{Float64},
    d_fac::Ptr{Float64}, d_bin::Ptr{Int32}, d_root::Ptr{Float64}, d_a::Ptr{Float64}, d_sum::Ptr{Float64}, n_col::Integer, n_dim::Integer,
    n_bin::Integer, gamma::Float64, B::Integer; kF::Float64, beta::Float64, lambda::Float64,
    dof::Union{Nothing,AbstractVector}=nothing, pools::Union{Nothing,AbstractVector}=nothing,
    reweight::Union{Nothing,Vector{Float64}}=nothing, flags::Integer=0, coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0,
    sample_offset::Integer=0, d_n_accept::Ptr{Int32}=Ptr{Int32}(C_NULL), x_col_stride::Integer=B, xp_col_stride::Integer=B,
    stream::Ptr{Cvoid}=C_NULL)
    root_group, var_mask = dof === nothing ? (UInt32[], UInt64[]) : weight_groups_from_dof(dof, pools)
    rw = reweight === nothing ? Float64[] : reweight
    GC.@preserve root_group var_mask rw begin
        cg = Ref(_FdgChainGroups(length(var_mask), pointer(root_group), pointer(var_mask), reweight === nothing ? Ptr{Float64}(C_NULL) : pointer(rw)))
        _fdg_check(ccall((:fdg_mc_chain_step_device_binned, _libfdg), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Float64, Float64, Float64, Ptr{Float64}, UInt32, UInt32, Ptr{Float64}, Float64, UInt64, UInt64,
             Cuint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32,
             Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Cvoid}),
            f.handle, d_xp, xp_col_stride, kF, beta, lambda, d_facp, n_col, n_dim, coef === nothing ? C_NULL : coef, gamma, seed,
            sample_offset, flags, d_x, x_col_stride, d_fac, d_root, d_a, d_sum, d_n_accept, C_NULL, dof === nothing ? C_NULL : cg, n_bin,
            d_binp, d_bin, B, stream))
    end
    return nothing
end
const FDG_CHAIN_BIN_MAX = 64
export chain_propose_device_discrete!, chain_step_device_binned!, mc_chain_step_device_binned!, FDG_CHAIN_BIN_MAX
# The chain's proposal with spherical momentum variables (fdg_chain_propose_device_polar): chain_propose_device_discrete! with the groups
# of vegas_sample_device_polar! (polar: a vector of (var, cols), 1-based).  A group is redrawn whole (all of its bits in mask) or kept,
# and the polar measure's factors go to the group's own columns of d_facp, so every step wrapper above serves as it is.  d_cdf = C_NULL:
# no discrete variable (d_bin, d_binp may be C_NULL; d_fac / d_facp are B x n_dim).  Unverified: written against the header, never run.
function chain_propose_device_polar!(d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64}, d_grid::Ptr{Float64},
    n_dim::Integer, n_grid::Integer, n_col::Integer, mask::Integer, B::Integer, polar::AbstractVector;
    col::Union{Nothing,AbstractVector{<:Integer}}=nothing, move_discrete::Bool=false, d_cdf::Ptr{Float64}=Ptr{Float64}(C_NULL),
    n_bin::Integer=1, d_ext::Ptr{Float64}=Ptr{Float64}(C_NULL), ext_col::AbstractVector{<:Integer}=Int[],
    d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), d_binp::Ptr{Int32}=Ptr{Int32}(C_NULL), seed::Integer=0, sample_offset::Integer=0,
    x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    c = col === nothing ? nothing : UInt32.(col .- 1)
    ec = UInt32.(ext_col .- 1)
    p = zeros(UInt32, 5 * max(length(polar), 1))
    for (g, (var, cols)) in enumerate(polar)
        length(cols) in (2, 3) || error("a polar group has 2 or 3 columns")
        p[5g-4] = var - 1
        p[5g-3] = length(cols)
        p[5g-2:5g-3+length(cols)] .= UInt32.(cols .- 1)
    end
    _fdg_check(ccall((:fdg_chain_propose_device_polar, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, UInt32, UInt64, UInt64, UInt64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Float64}, Cint, Ptr{Float64}, UInt32, Ptr{Float64}, UInt32, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32}, UInt32, Int64,
         Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride,
        d_facp, move_discrete ? 1 : 0, d_cdf, n_bin, d_ext, length(ec), isempty(ec) ? C_NULL : ec, d_bin, d_binp,
        isempty(polar) ? C_NULL : p, length(polar), B, stream))
    return nothing
end
export chain_propose_device_polar!
# The chain's proposal with local shift moves (fdg_chain_propose_device_local): chain_propose_device_polar! with the variables of local_mask
# shifted in the map's coordinate, y' = y + t h (mod 1), h = width[d] in (0, 0.5] (width: one number per variable, read where local_mask has
# a bit).  mask and local_mask share no bit; a variable of a polar group and the discrete variable cannot be shifted.  The proposal is
# symmetric in y, so every step wrapper above serves as it is.  Unverified: written against the header, never run.
function chain_propose_device_local!(d_xp::Ptr{Float64}, d_facp::Ptr{Float64}, d_x::Ptr{Float64}, d_fac::Ptr{Float64}, d_grid::Ptr{Float64},
    n_dim::Integer, n_grid::Integer, n_col::Integer, mask::Integer, local_mask::Integer, width::Vector{Float64}, B::Integer;
    polar::AbstractVector=[], col::Union{Nothing,AbstractVector{<:Integer}}=nothing, move_discrete::Bool=false,
    d_cdf::Ptr{Float64}=Ptr{Float64}(C_NULL), n_bin::Integer=1, d_ext::Ptr{Float64}=Ptr{Float64}(C_NULL),
    ext_col::AbstractVector{<:Integer}=Int[], d_bin::Ptr{Int32}=Ptr{Int32}(C_NULL), d_binp::Ptr{Int32}=Ptr{Int32}(C_NULL), seed::Integer=0,
    sample_offset::Integer=0, x_col_stride::Integer=B, xp_col_stride::Integer=B, stream::Ptr{Cvoid}=C_NULL)
    length(width) == n_dim || error("width holds one number per variable")
    c = col === nothing ? nothing : UInt32.(col .- 1)
    ec = UInt32.(ext_col .- 1)
    p = zeros(UInt32, 5 * max(length(polar), 1))
    for (g, (var, cols)) in enumerate(polar)
        length(cols) in (2, 3) || error("a polar group has 2 or 3 columns")
        p[5g-4] = var - 1
        p[5g-3] = length(cols)
        p[5g-2:5g-3+length(cols)] .= UInt32.(cols .- 1)
    end
    _fdg_check(ccall((:fdg_chain_propose_device_local, _libfdg), Cint,
        (Ptr{Float64}, UInt32, UInt32, Ptr{UInt32}, UInt32, UInt64, UInt64, Ptr{Float64}, UInt64, UInt64, Ptr{Float64}, Int64, Ptr{Float64},
         Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, UInt32, Ptr{Float64}, UInt32, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32},
         UInt32, Int64, Ptr{Cvoid}),
        d_grid, n_dim, n_grid, c === nothing ? C_NULL : c, n_col, mask, local_mask, width, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp,
        xp_col_stride, d_facp, move_discrete ? 1 : 0, d_cdf, n_bin, d_ext, length(ec), isempty(ec) ? C_NULL : ec, d_bin, d_binp,
        isempty(polar) ? C_NULL : p, length(polar), B, stream))
    return nothing
end
export chain_propose_device_local!

# ---- multi-GPU: one Julia process per GPU, ONE reduction of the accumulated observable ------------ #
# (include/fdg.h, "multi-GPU").  Rank 0 calls `comm_unique_id()` and ships the 128 bytes to the other
# ranks (MPI.jl `MPI.bcast`, a shared file, ...); every rank then builds its communicator with its own
# device current and, after its share of `accumulate_device!` calls, reduces `d_acc` in place.
const FDG_COMM_ID_BYTES = 128

function comm_unique_id()
    id = Vector{UInt8}(undef, FDG_COMM_ID_BYTES)
    _fdg_check(ccall((:fdg_comm_unique_id, _libfdg), Cint, (Ptr{UInt8}, Csize_t), id, FDG_COMM_ID_BYTES))
    return id
end

mutable struct Comm
    handle::Ptr{Cvoid}
    function Comm(id::Vector{UInt8}, rank::Integer, world::Integer)
        length(id) == FDG_COMM_ID_BYTES || error("unique id must be $FDG_COMM_ID_BYTES bytes")
        h = Ref{Ptr{Cvoid}}(C_NULL)
        _fdg_check(ccall((:fdg_comm_create, _libfdg), Cint, (Ptr{UInt8}, Cint, Cint, Ref{Ptr{Cvoid}}), id, rank, world, h))
        c = new(h[])
        finalizer(x -> ccall((:fdg_comm_destroy, _libfdg), Cint, (Ptr{Cvoid},), x.handle), c)
        return c
    end
end

"""`d_acc[1:n]` <- sum over ranks (all ranks get it; `root >= 0`: only that rank), on `stream`."""
function reduce_device!(c::Comm, d_acc::Ptr{Float64}, n::Integer; root::Integer=-1, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_reduce_device, _libfdg), Cint, (Ptr{Cvoid}, Ptr{Float64}, UInt32, Cint, Ptr{Cvoid}),
                     c.handle, d_acc, UInt32(n), Cint(root), stream))
    return nothing
end

# ---- fused Monte-Carlo step: leaves from (K, T) in registers, then the graph (include/fdg.h) --------- #
struct _FdgLeafTables
    n_leaf::UInt32
    n_basis::UInt32
    n_loop::UInt32
    dim::UInt32
    n_tau::UInt32
    leaf_type::Ptr{Int32}
    leaf_order::Ptr{Int32}
    tau_in::Ptr{Int32}
    tau_out::Ptr{Int32}
    loop_index::Ptr{Int32}
    basis::Ptr{Float64}
    kF::Float64
    beta::Float64
    lambda::Float64
end

"""
    specialize_fused!(f, leafType, leafOrder, leafInTau, leafOutTau, leafLoopIndex, loopbasis; dim=3, n_tau)

`leaf*` are one partition of `FrontEnds.leafstates` (1-based indices, `leafOrder` the order of the leaf's own kind),
`loopbasis` its deduplicated basis (`n_loop × n_basis`, columns as returned).  After this,
`mc_accumulate_device!(f, d_K, d_T, d_weight, d_acc, B; kF, beta, lambda)` runs leaves + graph + weighted sum in one kernel.
On a handle compiled with the optimizing back end (`compile(...; backend=:isa)`) that kernel is the back end's own: the
leaves are values of its program, computed in registers from the momenta and times.  It reads `d_K` (`B × n_loop*dim`)
and `d_T` (`B × n_tau`) in place when they are Julia column-major matrices -- the default `k_strides = t_strides = (1, B)`.
`kF`, `beta`, `lambda` are arguments of that kernel: one code object, assembled here, serves every parameter set.
"""
function specialize_fused!(f::GraphFunc, leafType::Vector{Int}, leafOrder::Vector{Int}, leafInTau::Vector{Int}, leafOutTau::Vector{Int},
    leafLoopIndex::Vector{Int}, loopbasis::Matrix{Float64}; dim::Int=3, n_tau::Int, cache_dir::Union{Nothing,String}=nothing,   # nothing: the library's per-user default (include/fdg.h)
    kF::Float64=0.0, beta::Float64=0.0, lambda::Float64=0.0)
    a = [Int32.(v) for v in (leafType, leafOrder, leafInTau, leafOutTau, leafLoopIndex)]
    bs = Matrix{Float64}(loopbasis)      # column-major n_loop × n_basis == row-major [n_basis][n_loop]
    GC.@preserve a bs begin
        tab = _FdgLeafTables(length(a[1]), size(bs, 2), size(bs, 1), dim, n_tau, pointer(a[1]), pointer(a[2]), pointer(a[3]),
            pointer(a[4]), pointer(a[5]), pointer(bs), kF, beta, lambda)
        _fdg_check(ccall((:fdg_graph_specialize_fused, _libfdg), Cint, (Ptr{Cvoid}, Ref{_FdgLeafTables}, Cstring, Cuint), f.handle, tab,
            isnothing(cache_dir) ? C_NULL : cache_dir, Cuint(0)))
    end
    return f
end

function mc_accumulate_device!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_weight::Ptr{Float64}, d_acc::Ptr{Float64}, B::Integer;
    kF::Float64, beta::Float64, lambda::Float64, k_strides=(1, B), t_strides=(1, B), stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_mc_accumulate_device, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_weight, d_acc, B, stream))
    return nothing
end
# the same into bins (fdg_mc_accumulate_device_binned): d_acc is R x n_bin, d_bin 1-based by default, as in accumulate_device_binned!
function mc_accumulate_device_binned!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_bin::Ptr{Int32}, n_bin::Integer,
    d_weight::Ptr{Float64}, d_acc::Ptr{Float64}, B::Integer; kF::Float64, beta::Float64, lambda::Float64, k_strides=(1, B), t_strides=(1, B),
    bin_base::Integer=1, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_mc_accumulate_device_binned, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32, Ptr{Float64},
         Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight, d_acc,
        B, stream))
    return nothing
end
# both moments for the fused step (fdg_mc_accumulate_device_moments): d_acc, d_acc2 and d_bin as in accumulate_device_moments!
function mc_accumulate_device_moments!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_bin::Ptr{Int32}, n_bin::Integer,
    d_weight::Ptr{Float64}, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, B::Integer; kF::Float64, beta::Float64, lambda::Float64,
    k_strides=(1, B), t_strides=(1, B), bin_base::Integer=1, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_mc_accumulate_device_moments, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight, d_acc,
        d_acc2, B, stream))
    return nothing
end
# the VEGAS accumulate step for the fused step (fdg_mc_accumulate_device_vegas): d_acc, d_acc2, d_hist and coef as in accumulate_device_vegas!
function mc_accumulate_device_vegas!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_weight::Ptr{Float64}, d_acc::Ptr{Float64},
    d_acc2::Ptr{Float64}, d_hist::Ptr{Float64}, n_dim::Integer, n_grid::Integer, B::Integer; kF::Float64, beta::Float64, lambda::Float64,
    coef::Union{Nothing,Vector{Float64}}=nothing, seed::Integer=0, sample_offset::Integer=0, k_strides=(1, B), t_strides=(1, B),
    stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_mc_accumulate_device_vegas, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, UInt64,
         UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
        f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_weight,
        coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, B, stream))
    return nothing
end
# the same for the fused step (fdg_mc_accumulate_device_vegas_binned)
function mc_accumulate_device_vegas_binned!(f::GraphFunc, d_K::Ptr{Float64}, d_T::Ptr{Float64}, d_bin::Ptr{Int32}, n_bin::Integer,
    d_weight::Ptr{Float64}, d_acc::Ptr{Float64}, d_acc2::Ptr{Float64}, d_hist::Ptr{Float64}, d_hist_bin::Ptr{Float64}, n_dim::Integer,
    n_grid::Integer, B::Integer; kF::Float64, beta::Float64, lambda::Float64, coef::Union{Nothing,Vector{Float64}}=nothing,
    seed::Integer=0, sample_offset::Integer=0, k_strides=(1, B), t_strides=(1, B), bin_base::Integer=1, stream::Ptr{Cvoid}=C_NULL)
    _fdg_check(ccall((:fdg_mc_accumulate_device_vegas_binned, _libfdg), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64, Float64, Ptr{Int32}, Int32, UInt32,
         Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, UInt32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Cvoid}),
        f.handle, d_K, k_strides[1], k_strides[2], d_T, t_strides[1], t_strides[2], kF, beta, lambda, d_bin, bin_base, n_bin, d_weight,
        coef === nothing ? C_NULL : coef, seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, B, stream))
    return nothing
end

"""
    leaf_eval_device!(d_leaf, leafType, leafOrder, leafInTau, leafOutTau, leafLoopIndex, loopbasis, d_K, d_T, B; dim, n_tau, kF, beta, lambda)

The leaf loop of `example/benchmark.jl:58-81` on the device (`fdg_leaf_eval_device`): fills the `B × L`
column-major leaf matrix at `d_leaf` from the loop momenta `d_K` (`B × (n_loop*dim)`, column-major) and times `d_T`
(`B × n_tau`).  Fermionic leaves of derivative order 0..5, interaction leaves of any order; type-0 leaves untouched.
"""
function leaf_eval_device!(d_leaf::Ptr{Float64}, leafType::Vector{Int}, leafOrder::Vector{Int}, leafInTau::Vector{Int}, leafOutTau::Vector{Int},
    leafLoopIndex::Vector{Int}, loopbasis::Matrix{Float64}, d_K::Ptr{Float64}, d_T::Ptr{Float64}, B::Integer;
    dim::Int=3, n_tau::Int, kF::Float64, beta::Float64, lambda::Float64, stream::Ptr{Cvoid}=C_NULL)
    a = [Int32.(v) for v in (leafType, leafOrder, leafInTau, leafOutTau, leafLoopIndex)]
    bs = Matrix{Float64}(loopbasis)
    GC.@preserve a bs begin
        tab = _FdgLeafTables(length(a[1]), size(bs, 2), size(bs, 1), dim, n_tau, pointer(a[1]), pointer(a[2]), pointer(a[3]),
            pointer(a[4]), pointer(a[5]), pointer(bs), kF, beta, lambda)
        _fdg_check(ccall((:fdg_leaf_eval_device, _libfdg), Cint,
            (Ref{_FdgLeafTables}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Ptr{Cvoid}),
            tab, d_K, 1, B, d_T, 1, B, d_leaf, 1, B, B, stream))
    end
    return nothing
end

"""
    leaf_eval_device_tiled!(d_leaf, leafType, ..., d_K, d_T, B; ...)

The same into a tile-major batch `Array{Float64,3}(64, L, cld(B, 64))` (`fdg_leaf_eval_device_tiled`): what `eval_device_tiled!` and
`accumulate_device_tiled!` read.
"""
function leaf_eval_device_tiled!(d_leaf::Ptr{Float64}, leafType::Vector{Int}, leafOrder::Vector{Int}, leafInTau::Vector{Int}, leafOutTau::Vector{Int},
    leafLoopIndex::Vector{Int}, loopbasis::Matrix{Float64}, d_K::Ptr{Float64}, d_T::Ptr{Float64}, B::Integer;
    dim::Int=3, n_tau::Int, kF::Float64, beta::Float64, lambda::Float64, stream::Ptr{Cvoid}=C_NULL)
    a = [Int32.(v) for v in (leafType, leafOrder, leafInTau, leafOutTau, leafLoopIndex)]
    bs = Matrix{Float64}(loopbasis)
    L = length(a[1])
    GC.@preserve a bs begin
        tab = _FdgLeafTables(L, size(bs, 2), size(bs, 1), dim, n_tau, pointer(a[1]), pointer(a[2]), pointer(a[3]),
            pointer(a[4]), pointer(a[5]), pointer(bs), kF, beta, lambda)
        _fdg_check(ccall((:fdg_leaf_eval_device_tiled, _libfdg), Cint,
            (Ref{_FdgLeafTables}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{Cvoid}),
            tab, d_K, 1, B, d_T, 1, B, d_leaf, 1, 64, 64 * L, B, stream))
    end
    return nothing
end
