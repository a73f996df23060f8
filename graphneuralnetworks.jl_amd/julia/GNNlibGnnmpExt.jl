# GNNlibGnnmpExt.jl — the reference-side binding of libgnnmp.so (include/gnnmp.h).
#
# This is the file a GNNlib.jl maintainer adds next to GNNlib/ext/GNNlibAMDGPUExt.jl (GNNlib/Project.toml:17-23: `AMDGPU`
# is already a weakdep; this extension replaces GNNlibAMDGPUExt in `[extensions]`, ChainRulesCore is already a hard
# dependency, :5).  It replaces the three methods of GNNlibAMDGPUExt.jl:13-32 — which today only *disable* the SpMM fast
# path on ROCm arrays and fall back to gather -> message -> atomic scatter — with calls into the fused HIP kernels, keeps
# them differentiable (ChainRulesCore rrules on every wrapper that hides a @ccall), and routes the four layer bodies of
# the hot path (gcn_conv, graph_conv / sage_conv through `propagate`, gat_conv) to the fused kernels.
#
# Julia is NOT available in the build container, so this file is written against the reference's sources but has never
# been executed (that includes the newest method, random_walk_pe at the end of the file).  What IS executed is the C ABI it calls: tests/test_c_harness.py drives the same entry points with the same
# argument conventions from a plain C program that owns its memory through hipMalloc (no torch anywhere), and
# graphneuralnetworks.jl_amd/gnnmp/ is the tested mirror of every wrapper below.
#
# Layout contract: Julia's column-major (D, N) feature matrix is exactly the C row-major [N][D] the library wants;
# GNNGraph's COO vectors (1-based Int64, or Int32) are passed untouched (idx_bytes, index_base = 1); a Julia weight
# matrix (Dout, Din) column-major is C row-major [Din][Dout], i.e. gnnmp_dense_f32's w_layout = 1 with ldw = Dout.

module GNNlibGnnmpExt

using AMDGPU: AMDGPU, ROCArray, ROCVector, ROCMatrix, AnyROCMatrix
using AMDGPU.rocSPARSE: ROCSparseMatrixCSC
using ChainRulesCore: ChainRulesCore, NoTangent, ZeroTangent, unthunk, @non_differentiable
using GNNlib: GNNlib, propagate, copy_xj, e_mul_xj, w_mul_xj
using GNNGraphs: GNNGraphs, GNNGraph, COO_T, SPARSE_T, edge_index, get_edge_weight, check_num_nodes, check_num_edges
using NNlib: relu
using Statistics: mean

const libgnnmp = get(ENV, "GNNMP_LIB", "libgnnmp.so")

# ---- status / stream plumbing ---------------------------------------------------------------------------------------
struct GnnmpError <: Exception
    status::Cint
    msg::String
end
const EUNSUPPORTED = Cint(-5)
function check(status::Cint)
    status == 0 && return nothing
    msg = unsafe_string(@ccall libgnnmp.gnnmp_last_error()::Cstring)
    throw(GnnmpError(status, msg))
end
stream_ptr() = Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream())   # launch on AMDGPU.jl's task-local stream, no syncs
devptr(x::ROCArray) = Base.unsafe_convert(Ptr{Cvoid}, pointer(x))
devptr(::Nothing) = C_NULL

const SUM, MEAN, MAX, MIN = Cint(0), Cint(1), Cint(2), Cint(3)
aggr_code(::typeof(+)) = SUM
aggr_code(::typeof(mean)) = MEAN
aggr_code(::typeof(max)) = MAX
aggr_code(::typeof(min)) = MIN
const FusedAggr = Union{typeof(+), typeof(mean), typeof(max), typeof(min)}
act_code(::typeof(identity)) = Cint(0)
act_code(::typeof(relu)) = Cint(1)
act_code(σ) = nothing                                              # anything else: applied as a broadcast afterwards

# ---- plans: one dst-sorted CSR per (s, t, num_nodes, self_loops, direction) ---------------------------------------------
mutable struct Plan
    handle::Ptr{Cvoid}
    function Plan(s::ROCVector{I}, t::ROCVector{I}, n_src::Int, n_dst::Int, self_loops::Bool) where {I <: Union{Int32, Int64}}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        # validate = 1: GNNGraph construction does not range-check device vectors (convert.jl:47-54 runs on the CPU copy only)
        check(@ccall libgnnmp.gnnmp_plan_create(h::Ptr{Ptr{Cvoid}}, devptr(s)::Ptr{Cvoid}, devptr(t)::Ptr{Cvoid},
                                                sizeof(I)::Cint, 1::Cint, n_src::Int64, n_dst::Int64,
                                                length(s)::Int64, self_loops::Cint, 1::Cint,
                                                stream_ptr()::Ptr{Cvoid})::Cint)
        p = new(h[])
        finalizer(p -> (@ccall libgnnmp.gnnmp_plan_destroy(p.handle::Ptr{Cvoid})::Cint), p)
        return p
    end
    # GNNGraph{SPARSE_T} on the device: the CSC structure of the adjacency IS the dst-sorted CSR (findnz order = slot order), no sort
    function Plan(A::ROCSparseMatrixCSC{Tv, I}) where {Tv, I <: Union{Int32, Int64}}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(@ccall libgnnmp.gnnmp_plan_from_csc(h::Ptr{Ptr{Cvoid}}, devptr(A.colPtr)::Ptr{Cvoid}, devptr(A.rowVal)::Ptr{Cvoid},
                                                  sizeof(I)::Cint, 1::Cint, size(A, 1)::Int64, size(A, 2)::Int64,
                                                  length(A.rowVal)::Int64, 1::Cint, stream_ptr()::Ptr{Cvoid})::Cint)
        p = new(h[])
        finalizer(p -> (@ccall libgnnmp.gnnmp_plan_destroy(p.handle::Ptr{Cvoid})::Cint), p)
        return p
    end
    # a handle the library made (gnnmp_plan_select / gnnmp_plan_concat: a pooled plan).  gnnmp_plan_destroy in the finalizer — the pooled
    # block is then handed out again only after a device synchronisation; `release!` is the stream-ordered path for a loop that knows
    # when its batch is done (gnnmp_plan_destroy(NULL) is a no-op)
    function Plan(h::Ptr{Cvoid})
        p = new(h)
        finalizer(p -> (@ccall libgnnmp.gnnmp_plan_destroy(p.handle::Ptr{Cvoid})::Cint), p)
        return p
    end
end

# Repair hook (gnnmp.h): a plan's split rows are folded through per-plan arrival counters that every launch leaves at zero — as long as the
# plan is used from one task / stream at a time.  A caller that may have broken that rule (two tasks on one GNNGraph) resets them here.
reset_counters!(p::Plan) = (check(@ccall libgnnmp.gnnmp_plan_reset_counters(p.handle::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint); p)

# The cache is keyed on the IDENTITY of the two index vectors plus everything else a plan depends on.  (Round 1 keyed a
# WeakKeyDict on `s` alone: two graphs sharing s but not t, or num_nodes, got the first graph's plan — and WeakKeyDict hashes
# array CONTENTS, a scalar-indexing O(E) walk of a ROCVector per call.)  GNNGraph is immutable and shares s, t across copies
# (gnngraph.jl:187-211), so identity is the right notion of "same graph".  objectids are recycled after collection: every
# entry carries a liveness flag that finalizers on s and t clear (a finalizer must not lock or allocate — storing a Bool
# is all it does), and a lookup that finds a dead entry rebuilds it.
struct PlanKey
    s::UInt
    t::UInt
    n::Int
    self_loops::Bool
    transposed::Bool
end
mutable struct PlanEntry
    plan::Plan
    @atomic alive::Bool
end
const PLANS = Dict{PlanKey, PlanEntry}()
const PLANS_LOCK = ReentrantLock()

# (s, t) of any device graph on the device: the COO vectors themselves, or findnz order materialised from a sparse graph's plan
# (device_edge_index below — `edge_index` of a ROCSparseMatrixCSC graph is findnz on the device, which AMDGPU.jl does not provide)
coo_index(g::GNNGraph{<:COO_T}) = edge_index(g)

function plan(g::GNNGraph{<:COO_T}; self_loops::Bool = false, transposed::Bool = false)
    s, t = edge_index(g)
    key = PlanKey(objectid(s), objectid(t), g.num_nodes, self_loops, transposed)
    lock(PLANS_LOCK) do
        ent = get(PLANS, key, nothing)
        if ent === nothing || !(@atomic ent.alive)
            filter!(kv -> (@atomic kv.second.alive), PLANS)   # every miss drops the plans of collected graphs: a plan holds device
                                                                 # memory (0.5 GB at the products size) that must not wait for 256 entries
            p = transposed ? Plan(t, s, g.num_nodes, g.num_nodes, self_loops) : Plan(s, t, g.num_nodes, g.num_nodes, self_loops)
            ent = PlanEntry(p, true)
            let ent = ent
                finalizer(_ -> (@atomic ent.alive = false), s)
                finalizer(_ -> (@atomic ent.alive = false), t)
            end
            PLANS[key] = ent
        end
        ent.plan
    end
end
@non_differentiable plan(::Any...)

# ---- propagate: replaces GNNlib/ext/GNNlibAMDGPUExt.jl:13-32 (and extends it to mean / max / min) ----------------------
function fused_propagate(g::GNNGraph, aggr, xj::AnyROCMatrix{Float32}, w; self_loops = false, scale_src = nothing,
                         scale_dst = nothing)
    check_num_nodes(g, xj)                                        # AssertionError contract (GNNGraphs/src/utils.jl:1-28)
    p = plan(g; self_loops)
    D = size(xj, 1)
    out = similar(xj, D, g.num_nodes)
    msg = w === nothing ? Cint(0) : Cint(1)
    check(@ccall libgnnmp.gnnmp_propagate_f32(p.handle::Ptr{Cvoid}, msg::Cint, aggr_code(aggr)::Cint,
                                              devptr(xj)::Ptr{Cvoid}, devptr(w)::Ptr{Cvoid},
                                              devptr(scale_src)::Ptr{Cvoid}, devptr(scale_dst)::Ptr{Cvoid},
                                              devptr(out)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end

function GNNlib.propagate(::typeof(copy_xj), g::GNNGraph{<:COO_T}, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float32}, e)
    fused_propagate(g, aggr, xj, nothing)
end
function GNNlib.propagate(::typeof(e_mul_xj), g::GNNGraph{<:COO_T}, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float32},
                          e::ROCVector{Float32})
    check_num_edges(g, e)
    fused_propagate(g, aggr, xj, e)
end
function GNNlib.propagate(::typeof(w_mul_xj), g::GNNGraph{<:COO_T}, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float32},
                          e::Nothing)
    fused_propagate(g, aggr, xj, get_edge_weight(g))              # the CPU fast path's weighted adjacency (msgpass.jl:234-238)
end

# ---- Float64 features (round 6; the reference's own micro-benchmark, perf/bench_gnn.jl:9-40, runs propagate on rand(100, n)) ---------------
# The three methods of the seam for ROCMatrix{Float64}: same plan, same order of operations, the *_f64 entry points.  Forward only — no
# rrule: differentiating through them falls back to Zygote's generic path (the Float32 methods above carry the adjoint kernels).  Weights of
# another float eltype are promoted like `w .* xj` would.
function fused_propagate64(g::GNNGraph, aggr, xj::AnyROCMatrix{Float64}, w)
    check_num_nodes(g, xj)
    p = plan(g; self_loops = false)
    D = size(xj, 1)
    out = similar(xj, D, g.num_nodes)
    w64 = w === nothing ? nothing : (eltype(w) === Float64 ? w : Float64.(w))
    msg = w64 === nothing ? Cint(0) : Cint(1)
    check(@ccall libgnnmp.gnnmp_propagate_f64(p.handle::Ptr{Cvoid}, msg::Cint, aggr_code(aggr)::Cint, devptr(xj)::Ptr{Cvoid},
                                              devptr(w64)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, devptr(out)::Ptr{Cvoid},
                                              D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
function GNNlib.propagate(::typeof(copy_xj), g::GNNGraph{<:COO_T}, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float64}, e)
    fused_propagate64(g, aggr, xj, nothing)
end
function GNNlib.propagate(::typeof(e_mul_xj), g::GNNGraph{<:COO_T}, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float64},
                          e::ROCVector{<:Union{Float32, Float64}})
    check_num_edges(g, e)
    fused_propagate64(g, aggr, xj, e)
end
function GNNlib.propagate(::typeof(w_mul_xj), g::GNNGraph{<:COO_T}, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float64}, e::Nothing)
    fused_propagate64(g, aggr, xj, get_edge_weight(g))
end
# the leaves for generic closures (GNNGraphs/src/gatherscatter.jl:4,12-18)
function GNNGraphs._gather(x::AnyROCMatrix{Float64}, i::ROCVector{I}) where {I <: Union{Int32, Int64}}
    D = size(x, 1)
    out = similar(x, D, length(i))
    check(@ccall libgnnmp.gnnmp_gather_f64(devptr(x)::Ptr{Cvoid}, devptr(i)::Ptr{Cvoid}, sizeof(I)::Cint, 1::Cint, length(i)::Int64,
                                           devptr(out)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
# _scatter(aggr, m, t, n) with t === the graph's own target vector: the graph's plan is the plan of that scatter (m in edge order)
function scatter_edges64(g::GNNGraph{<:COO_T}, aggr, m::AnyROCMatrix{Float64})
    check_num_edges(g, m)
    D = size(m, 1)
    out = similar(m, D, g.num_nodes)
    check(@ccall libgnnmp.gnnmp_scatter_f64(plan(g; self_loops = false).handle::Ptr{Cvoid}, aggr_code(aggr)::Cint, devptr(m)::Ptr{Cvoid},
                                            devptr(out)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
function GNNlib.aggregate_neighbors(g::GNNGraph{<:COO_T}, aggr::FusedAggr, m::AnyROCMatrix{Float64})
    scatter_edges64(g, aggr, m)
end

# ---- GNNGraph{SPARSE_T}: the other half of the reference seam's Union{COO_T, SPARSE_T} (GNNlibAMDGPUExt.jl:13-32) ----------------------
# The reference's methods gather / scatter over edge_index(g), which for a device sparse matrix is findnz on a ROCSparseMatrixCSC — the
# cases GNNlib/test/msgpass.jl:171-196 mark `broken` on AMDGPU.  Here the adjacency's CSC arrays are the plan (gnnmp_plan_from_csc):
# column t of A lists the sources of t's incoming edges, edge k of findnz(A) is slot k, get_edge_weight(g) is nzVal.
const SparseDeviceGraph = GNNGraph{<:ROCSparseMatrixCSC}
const DeviceGraph = Union{GNNGraph{<:COO_T}, SparseDeviceGraph}

# (s, t) of a sparse graph in findnz order, materialised on the device from the plan (for the plans that need a COO: self loops, reversed)
function device_edge_index(g::SparseDeviceGraph)
    p = plan(g)
    I = eltype(g.graph.colPtr)
    s, t = ROCVector{I}(undef, g.num_edges), ROCVector{I}(undef, g.num_edges)
    check(@ccall libgnnmp.gnnmp_plan_edge_index(p.handle::Ptr{Cvoid}, sizeof(I)::Cint, 1::Cint, devptr(s)::Ptr{Cvoid},
                                                devptr(t)::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint)
    return s, t
end

coo_index(g::SparseDeviceGraph) = device_edge_index(g)

function plan(g::SparseDeviceGraph; self_loops::Bool = false, transposed::Bool = false)
    A = g.graph
    key = PlanKey(objectid(A.colPtr), objectid(A.rowVal), g.num_nodes, self_loops, transposed)
    lock(PLANS_LOCK) do
        ent = get(PLANS, key, nothing)
        if ent === nothing || !(@atomic ent.alive)
            filter!(kv -> (@atomic kv.second.alive), PLANS)
            p = if !self_loops && !transposed
                Plan(A)
            else
                s, t = device_edge_index(g)                      # (recursion ends: that call asks for the plain plan)
                transposed ? Plan(t, s, g.num_nodes, g.num_nodes, self_loops) : Plan(s, t, g.num_nodes, g.num_nodes, self_loops)
            end
            ent = PlanEntry(p, true)
            let ent = ent
                finalizer(_ -> (@atomic ent.alive = false), A.colPtr)
                finalizer(_ -> (@atomic ent.alive = false), A.rowVal)
            end
            PLANS[key] = ent
        end
        ent.plan
    end
end

sparse_weights(g::SparseDeviceGraph) = g.graph.nzVal isa ROCVector{Float32} ? g.graph.nzVal : Float32.(g.graph.nzVal)

function GNNlib.propagate(::typeof(copy_xj), g::SparseDeviceGraph, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float32}, e)
    fused_propagate(g, aggr, xj, nothing)
end
function GNNlib.propagate(::typeof(e_mul_xj), g::SparseDeviceGraph, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float32},
                          e::ROCVector{Float32})
    length(e) == g.num_edges || throw(AssertionError("Got $(length(e)) as last dimension size instead of num_edges=$(g.num_edges)"))
    fused_propagate(g, aggr, xj, e)
end
function GNNlib.propagate(::typeof(w_mul_xj), g::SparseDeviceGraph, aggr::FusedAggr, xi, xj::AnyROCMatrix{Float32},
                          e::Nothing)
    fused_propagate(g, aggr, xj, sparse_weights(g))               # A's stored values (msgpass.jl:234-238: xj * A)
end

# in-degree counts (Float32) of the plan's rows: the mean adjoint divides by them
function in_count(g::GNNGraph, self_loops::Bool)
    d = AMDGPU.zeros(Float32, g.num_nodes)
    check(@ccall libgnnmp.gnnmp_degree_f32(plan(g; self_loops).handle::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, devptr(d)::Ptr{Cvoid},
                                           stream_ptr()::Ptr{Cvoid})::Cint)
    return d
end
@non_differentiable in_count(::Any...)

# The pullback Zygote would compose from NNlib's rules for gather -> message -> scatter (∇scatter(+) = gather, ∇scatter(mean)
# = gather ./ count, ∇scatter(max|min) = (src .== gather(dst)) .* gather(Δ), ∇gather = scatter(+)), as three kernels:
#   Δxj: the SAME fused kernel on the plan of the reversed edge index (scale_src and scale_dst swap roles);
#   Δw : one dot product per edge, walked in plan order;   max / min: their own kernel (ties all receive Δ, like NNlib).
# Mirror of graphneuralnetworks.jl_amd/gnnmp/backward.py (tested against the oracle's restatement of NNlib's rules).
function ChainRulesCore.rrule(::typeof(fused_propagate), g::GNNGraph, aggr, xj::AnyROCMatrix{Float32}, w;
                              self_loops = false, scale_src = nothing, scale_dst = nothing)
    y = fused_propagate(g, aggr, xj, w; self_loops, scale_src, scale_dst)
    function fused_propagate_pullback(Δ̄)
        Δ = convert(typeof(y), unthunk(Δ̄))
        D = size(Δ, 1)
        pt = plan(g; self_loops, transposed = true)
        Δx = similar(xj)
        if aggr === max || aggr === min
            @assert w === nothing && scale_src === nothing && scale_dst === nothing
            check(@ccall libgnnmp.gnnmp_propagate_maxmin_grad_f32(pt.handle::Ptr{Cvoid}, devptr(xj)::Ptr{Cvoid},
                      devptr(y)::Ptr{Cvoid}, devptr(Δ)::Ptr{Cvoid}, devptr(Δx)::Ptr{Cvoid}, D::Int64,
                      stream_ptr()::Ptr{Cvoid})::Cint)
            return NoTangent(), NoTangent(), NoTangent(), Δx, NoTangent()
        end
        sd = scale_dst
        if aggr === mean
            inv = 1f0 ./ max.(in_count(g, self_loops), 1f0)
            sd = sd === nothing ? inv : sd .* inv
        end
        # out_i = sd_i Σ_k w_k ss_{s_k} x_{s_k}  =>  Δx_j = ss_j Σ_{k: s_k = j} w_k (sd Δ)_{t_k}: source factor sd, destination factor ss
        check(@ccall libgnnmp.gnnmp_propagate_f32(pt.handle::Ptr{Cvoid}, (w === nothing ? 0 : 1)::Cint, SUM::Cint,
                  devptr(Δ)::Ptr{Cvoid}, devptr(w)::Ptr{Cvoid}, devptr(sd)::Ptr{Cvoid}, devptr(scale_src)::Ptr{Cvoid},
                  devptr(Δx)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        Δw = NoTangent()
        if w !== nothing
            @assert !self_loops "Δw with plan-added self loops: the appended edges carry no weight to differentiate"
            Δs = sd === nothing ? Δ : Δ .* reshape(sd, 1, :)
            xs = scale_src === nothing ? xj : xj .* reshape(scale_src, 1, :)
            Δw = similar(w)
            # the row kernel keeps a feature row in ONE lane group (<= 64 lanes of 4 / 2 / 1 floats, by width AND pointer alignment: the
            # library decides, GNNMP_EUNSUPPORTED = -5 says "not this one"); wider rows take the COO-order kernel
            st = @ccall libgnnmp.gnnmp_edge_dot_plan_f32(plan(g).handle::Ptr{Cvoid}, devptr(Δs)::Ptr{Cvoid},
                          devptr(xs)::Ptr{Cvoid}, devptr(Δw)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint
            if st != -5
                check(st)
            else
                s, t = coo_index(g)                                     # (a sparse device graph: from its plan, not findnz on the device)
                check(@ccall libgnnmp.gnnmp_edge_dot_f32(devptr(Δs)::Ptr{Cvoid}, devptr(xs)::Ptr{Cvoid}, devptr(s)::Ptr{Cvoid},
                          devptr(t)::Ptr{Cvoid}, sizeof(eltype(s))::Cint, 1::Cint, length(s)::Int64, D::Int64,
                          devptr(Δw)::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint)
            end
        end
        return NoTangent(), NoTangent(), NoTangent(), Δx, Δw
    end
    return y, fused_propagate_pullback
end

# ---- leaf ops for arbitrary closures: GNNGraphs/src/gatherscatter.jl:4,12-18 ------------------------------------------
# _gather keeps NNlib's rrule semantics through its own rule: ∇gather(x, i) = scatter(+, Δ, i) on a throw-away plan
function GNNGraphs._gather(x::ROCArray{Float32}, i::ROCVector{I}) where {I <: Union{Int32, Int64}}
    D = prod(size(x)[1:(end - 1)])
    out = similar(x, size(x)[1:(end - 1)]..., length(i))
    check(@ccall libgnnmp.gnnmp_gather_f32(devptr(x)::Ptr{Cvoid}, devptr(i)::Ptr{Cvoid}, sizeof(I)::Cint, 1::Cint,
                                           length(i)::Int64, devptr(out)::Ptr{Cvoid}, D::Int64,
                                           stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
function scatter_plan(p::Plan, aggr, m::ROCArray{Float32}, n::Int)
    D = prod(size(m)[1:(end - 1)])
    out = similar(m, size(m)[1:(end - 1)]..., n)
    check(@ccall libgnnmp.gnnmp_scatter_f32(p.handle::Ptr{Cvoid}, aggr_code(aggr)::Cint, devptr(m)::Ptr{Cvoid},
                                            devptr(out)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
function ChainRulesCore.rrule(::typeof(GNNGraphs._gather), x::ROCArray{Float32}, i::ROCVector{I}) where {I <: Union{Int32, Int64}}
    y = GNNGraphs._gather(x, i)
    n = size(x)[end]
    function gather_pullback(Δ̄)
        Δ = convert(typeof(y), unthunk(Δ̄))
        ar = ROCArray(collect(I, 1:length(i)))
        Δx = scatter_plan(Plan(ar, i, length(i), n, false), +, Δ, n)
        return NoTangent(), Δx, NoTangent()
    end
    return y, gather_pullback
end
# deterministic, edge-order scatter through the plan of the graph's targets; used by aggregate_neighbors.  Differentiable
# for + and mean (∇scatter = gather [./ count]); max / min closures keep the generic NNlib path (no override below).
function GNNlib.aggregate_neighbors(g::GNNGraph{<:COO_T}, aggr::Union{typeof(+), typeof(mean)}, m::ROCArray{Float32})
    check_num_edges(g, m)
    scatter_edges(g, aggr, m)
end
scatter_edges(g, aggr, m) = scatter_plan(plan(g), aggr, m, g.num_nodes)
function ChainRulesCore.rrule(::typeof(scatter_edges), g, aggr, m::ROCArray{Float32})
    y = scatter_edges(g, aggr, m)
    function scatter_edges_pullback(Δ̄)
        Δ = convert(typeof(y), unthunk(Δ̄))
        _, t = coo_index(g)
        Δs = aggr === mean ? Δ ./ reshape(max.(in_count(g, false), 1f0), ntuple(_ -> 1, ndims(Δ) - 1)..., :) : Δ
        return NoTangent(), NoTangent(), NoTangent(), GNNGraphs._gather(Δs, t)
    end
    return y, scatter_edges_pullback
end

# ---- softmax_edge_neighbors: GNNlib/src/utils.jl:84-97 ----------------------------------------------------------------
function edge_softmax(g::GNNGraph{<:COO_T}, e::ROCArray{Float32})
    @assert size(e)[end] == g.num_edges
    H = prod(size(e)[1:(end - 1)])
    out = similar(e)
    check(@ccall libgnnmp.gnnmp_edge_softmax_f32(plan(g).handle::Ptr{Cvoid}, devptr(e)::Ptr{Cvoid},
                                                 devptr(out)::Ptr{Cvoid}, H::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
GNNlib.softmax_edge_neighbors(g::GNNGraph{<:COO_T}, e::ROCArray{Float32}) = edge_softmax(g, e)
# softmax pullback per destination: Δe = α .* (Δα .- Σ_{N(i)} α Δα) — two calls of kernels that already exist
function ChainRulesCore.rrule(::typeof(edge_softmax), g::GNNGraph{<:COO_T}, e::ROCArray{Float32})
    α = edge_softmax(g, e)
    function edge_softmax_pullback(Δ̄)
        Δ = convert(typeof(α), unthunk(Δ̄))
        _, t = edge_index(g)
        s = GNNGraphs._gather(scatter_edges(g, +, α .* Δ), t)
        return NoTangent(), NoTangent(), α .* (Δ .- s)
    end
    return α, edge_softmax_pullback
end

# ---- reduce_nodes / global_pool: GNNlib/src/utils.jl:12-16 (batch-built indicators are sorted) ---------------------------
function segment_pool(aggr, g::GNNGraph, x::AnyROCMatrix{Float32})
    @assert size(x)[end] == g.num_nodes
    gi = GNNGraphs.graph_indicator(g)
    D = size(x, 1)
    out = similar(x, D, g.num_graphs)
    check(@ccall libgnnmp.gnnmp_segment_pool_f32(aggr_code(aggr)::Cint, devptr(x)::Ptr{Cvoid}, devptr(gi)::Ptr{Cvoid},
                                                 sizeof(eltype(gi))::Cint, 1::Cint, devptr(out)::Ptr{Cvoid}, D::Int64,
                                                 g.num_nodes::Int64, g.num_graphs::Int64,
                                                 stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end
GNNlib.reduce_nodes(aggr::Union{typeof(+), typeof(mean)}, g::GNNGraph, x::AnyROCMatrix{Float32}) = segment_pool(aggr, g, x)
function ChainRulesCore.rrule(::typeof(segment_pool), aggr, g::GNNGraph, x::AnyROCMatrix{Float32})
    y = segment_pool(aggr, g, x)
    function segment_pool_pullback(Δ̄)
        Δ = convert(typeof(y), unthunk(Δ̄))
        gi = GNNGraphs.graph_indicator(g)
        if aggr === mean
            cnt = segment_pool(+, g, AMDGPU.ones(Float32, 1, g.num_nodes))
            Δ = Δ ./ max.(cnt, 1f0)
        end
        return NoTangent(), NoTangent(), NoTangent(), GNNGraphs._gather(Δ, gi)      # broadcast_nodes
    end
    return y, segment_pool_pullback
end

# ---- dense: act.(W * x1 (+ W2 * x2) .+ b) on the fp32 MFMA kernels -------------------------------------------------------
function dense(W::ROCMatrix{Float32}, x::AnyROCMatrix{Float32}, b, σ; W2 = nothing, x2 = nothing)
    Dout, D1 = size(W)
    @assert size(x, 1) == D1
    N = size(x, 2)
    D2 = x2 === nothing ? 0 : size(x2, 1)
    code = act_code(σ)
    out = similar(x, Dout, N)
    bias = b isa AbstractArray ? b : nothing                      # Flux stores `false` for bias = false
    check(@ccall libgnnmp.gnnmp_dense_f32(devptr(x)::Ptr{Cvoid}, devptr(W)::Ptr{Cvoid}, D1::Int64, Dout::Int64,
              devptr(x2)::Ptr{Cvoid}, devptr(W2)::Ptr{Cvoid}, D2::Int64, Dout::Int64, 1::Cint, devptr(bias)::Ptr{Cvoid},
              something(code, Cint(0))::Cint, devptr(out)::Ptr{Cvoid}, N::Int64, Dout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return code === nothing ? σ.(out) : out
end
function ChainRulesCore.rrule(::typeof(dense), W::ROCMatrix{Float32}, x::AnyROCMatrix{Float32}, b, σ)
    code = act_code(σ)
    code === nothing && error("gnnmp dense adjoint covers identity and relu; use Flux.Dense for other activations")
    y = dense(W, x, b, σ)
    function dense_pullback(Δ̄)
        Δ = convert(typeof(y), unthunk(Δ̄))
        Dout, K = size(W)
        N = size(x, 2)
        Δz = similar(Δ)
        check(@ccall libgnnmp.gnnmp_act_grad_f32(devptr(Δ)::Ptr{Cvoid}, devptr(y)::Ptr{Cvoid}, code::Cint, devptr(Δz)::Ptr{Cvoid},
                  length(Δ)::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        nws = @ccall libgnnmp.gnnmp_dense_grad_workspace(N::Int64, Dout::Int64, K::Int64)::Int64
        ws = AMDGPU.zeros(Float32, max(nws, 1))
        ΔWt = similar(W, K, Dout)                                 # the kernel writes C row-major [Dout][K] = Julia (K, Dout)
        Δb = b isa AbstractArray ? similar(b) : nothing
        check(@ccall libgnnmp.gnnmp_dense_grad_w_f32(devptr(Δz)::Ptr{Cvoid}, devptr(x)::Ptr{Cvoid}, N::Int64, Dout::Int64,
                  K::Int64, devptr(ΔWt)::Ptr{Cvoid}, devptr(Δb)::Ptr{Cvoid}, devptr(ws)::Ptr{Cvoid}, length(ws)::Int64,
                  stream_ptr()::Ptr{Cvoid})::Cint)
        # Δx = W' * Δz: the forward kernel with the weight read the other way round (w_layout = 0: Julia (Dout, K) is C [K][Dout])
        Δx = similar(x)
        check(@ccall libgnnmp.gnnmp_dense_f32(devptr(Δz)::Ptr{Cvoid}, devptr(W)::Ptr{Cvoid}, Dout::Int64, Dout::Int64,
                  C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, 0::Int64, 0::Int64, 0::Cint, C_NULL::Ptr{Cvoid}, 0::Cint,
                  devptr(Δx)::Ptr{Cvoid}, N::Int64, K::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        return NoTangent(), permutedims(ΔWt), Δx, (Δb === nothing ? NoTangent() : Δb), NoTangent()
    end
    return y, dense_pullback
end

# ---- gcn_conv: GNNlib/src/layers/conv.jl:14-72 on ROCm arrays ------------------------------------------------------------
# Same statements as the reference body, with (i) add_self_loops inside the plan instead of an index concatenation,
# (ii) `xj .* cout'`, the propagate and `x .* cin'` as ONE kernel (the scalings are its per-node factors), (iii) `weight * x`,
# `.+ bias`, σ on the MFMA kernel — and, when Dout >= Din and nothing is being differentiated, aggregation and product in one
# launch (gnnmp_fused_conv_f32).  Every step is a wrapper with an rrule, so Zygote differentiates the composition.
function gcn_normalisation(l, g::GNNGraph, edge_weight, norm_fn)
    p = plan(g; self_loops = l.add_self_loops)
    w = edge_weight !== nothing ? edge_weight : (l.use_edge_weight ? get_edge_weight(g) : nothing)
    d = AMDGPU.zeros(Float32, g.num_nodes)
    check(@ccall libgnnmp.gnnmp_degree_f32(p.handle::Ptr{Cvoid}, devptr(w)::Ptr{Cvoid}, devptr(d)::Ptr{Cvoid},
                                           stream_ptr()::Ptr{Cvoid})::Cint)   # plan-added self loops weigh 1 (conv.jl:28-33)
    return norm_fn(d), w
end
@non_differentiable gcn_normalisation(::Any...)

function GNNlib.gcn_conv(l, g::GNNGraph{<:COO_T}, x::AnyROCMatrix{Float32}, edge_weight::EW, norm_fn::F,
                         conv_weight::CW) where {EW <: Union{Nothing, ROCVector{Float32}}, CW <: Union{Nothing, ROCMatrix{Float32}}, F}
    GNNlib.check_gcnconv_input(g, edge_weight)
    weight = conv_weight === nothing ? l.weight : conv_weight
    size(weight) == size(l.weight) ||
        throw(ArgumentError("The weight matrix has the wrong size. Expected $(size(l.weight)) but got $(size(weight))"))
    check_num_nodes(g, x)
    Dout, Din = size(weight)
    c, w = gcn_normalisation(l, g, edge_weight, norm_fn)
    if Dout < Din
        x = dense(weight, x, nothing, identity)                    # multiply before convolution (conv.jl:36-40)
    end
    x = fused_propagate(g, +, x, w; self_loops = l.add_self_loops, scale_src = c, scale_dst = c)
    if Dout >= Din
        return dense(weight, x, l.bias, l.σ)
    end
    return l.σ.(x .+ l.bias)
end

# inference-only one-kernel form of the Dout >= Din branch (call it from a layer's forward when no gradient is needed)
function gcn_conv_fused(l, g::GNNGraph{<:COO_T}, x::AnyROCMatrix{Float32}; norm_fn = d -> 1f0 ./ sqrt.(d))
    weight = l.weight
    Dout, Din = size(weight)
    code = act_code(l.σ)
    (Dout >= Din && code !== nothing) || return GNNlib.gcn_conv(l, g, x, nothing, norm_fn, nothing)
    c, w = gcn_normalisation(l, g, nothing, norm_fn)
    out = similar(x, Dout, g.num_nodes)
    bias = l.bias isa AbstractArray ? l.bias : nothing
    st = @ccall libgnnmp.gnnmp_fused_conv_f32(plan(g; self_loops = l.add_self_loops).handle::Ptr{Cvoid}, SUM::Cint,
              devptr(x)::Ptr{Cvoid}, devptr(w)::Ptr{Cvoid}, devptr(c)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
              devptr(c)::Ptr{Cvoid}, Din::Int64, C_NULL::Ptr{Cvoid}, 0::Int64, C_NULL::Ptr{Cvoid}, 0::Int64,
              devptr(weight)::Ptr{Cvoid}, Dout::Int64, 1::Cint, devptr(bias)::Ptr{Cvoid}, code::Cint, devptr(out)::Ptr{Cvoid},
              Dout::Int64, C_NULL::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint
    st == EUNSUPPORTED && return GNNlib.gcn_conv(l, g, x, nothing, norm_fn, nothing)   # shape outside the fused kernel
    check(st)
    return out
end

# ---- gat_conv: GNNlib/src/layers/conv.jl:112-167 with e === nothing -------------------------------------------------------
# Wx = reshape(l.dense_x(x), C, H, N) is the (C*H, N) matrix as stored; l.a (2C, H) column-major is C row-major [H][2C]:
# exactly the layout gnnmp.h asks for, so `l.a` itself is passed — no permutedims.  The forward saves (max, denominator)
# per destination and head for the pullback (8 bytes instead of α: 4 H bytes per EDGE).
function gat_attention(g::GNNGraph{<:COO_T}, Wx::AnyROCMatrix{Float32}, a::ROCMatrix{Float32}, slope::Float32,
                       heads::Int, self_loops::Bool)
    out, _ = gat_attention_stats(g, Wx, a, slope, heads, self_loops, false)
    return out
end
function gat_attention_stats(g, Wx, a, slope, heads, self_loops, want_stats)
    chout = size(Wx, 1) ÷ heads
    out = similar(Wx)
    p = plan(g; self_loops)
    if want_stats
        stats = similar(Wx, 2, heads, g.num_nodes)
        check(@ccall libgnnmp.gnnmp_gat_conv_stats_f32(p.handle::Ptr{Cvoid}, devptr(Wx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
                  devptr(a)::Ptr{Cvoid}, slope::Cfloat, C_NULL::Ptr{Cvoid}, 0::Cint, devptr(out)::Ptr{Cvoid},
                  devptr(stats)::Ptr{Cvoid}, heads::Int64, chout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        return out, stats
    end
    check(@ccall libgnnmp.gnnmp_gat_conv_f32(p.handle::Ptr{Cvoid}, devptr(Wx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
              devptr(a)::Ptr{Cvoid}, slope::Cfloat, C_NULL::Ptr{Cvoid}, 0::Cint, devptr(out)::Ptr{Cvoid}, heads::Int64,
              chout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out, nothing
end
# The training forward also saves o+ / P (gnnmp.h: gnnmp_gat_conv_train_f32): the pullback's destination side is then a node kernel on
# (Δ, out, o+, P) and only the source side walks the edges (gnnmp_gat_conv_grad2_f32: 8.7 ms against 12.8 ms on the products shape).
function ChainRulesCore.rrule(::typeof(gat_attention), g::GNNGraph{<:COO_T}, Wx::AnyROCMatrix{Float32}, a::ROCMatrix{Float32},
                              slope::Float32, heads::Int, self_loops::Bool)
    chout = size(Wx, 1) ÷ heads
    N = g.num_nodes
    out = similar(Wx)
    stats = similar(Wx, 2, heads, N)
    oplus, pplus = similar(Wx), similar(Wx, heads, N)
    check(@ccall libgnnmp.gnnmp_gat_conv_train_f32(plan(g; self_loops).handle::Ptr{Cvoid}, devptr(Wx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
              devptr(a)::Ptr{Cvoid}, slope::Cfloat, C_NULL::Ptr{Cvoid}, 0::Cint, devptr(out)::Ptr{Cvoid}, devptr(stats)::Ptr{Cvoid},
              devptr(oplus)::Ptr{Cvoid}, devptr(pplus)::Ptr{Cvoid}, heads::Int64, chout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    function gat_attention_pullback(Δ̄)
        Δ = convert(typeof(out), unthunk(Δ̄))
        ΔWx, Δa = similar(Wx), similar(a)
        line = similar(Wx, 4, heads, N)                           # scratch the kernel asks the caller for (gnnmp.h)
        dsd, dss = similar(Wx, heads, N), similar(Wx, heads, N)
        check(@ccall libgnnmp.gnnmp_gat_conv_grad2_f32(plan(g; self_loops).handle::Ptr{Cvoid},
                  plan(g; self_loops, transposed = true).handle::Ptr{Cvoid}, devptr(Wx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
                  devptr(a)::Ptr{Cvoid}, slope::Cfloat, devptr(stats)::Ptr{Cvoid}, devptr(out)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
                  devptr(oplus)::Ptr{Cvoid}, devptr(pplus)::Ptr{Cvoid}, devptr(Δ)::Ptr{Cvoid}, devptr(line)::Ptr{Cvoid},
                  devptr(dsd)::Ptr{Cvoid}, devptr(dss)::Ptr{Cvoid}, devptr(ΔWx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
                  devptr(Δa)::Ptr{Cvoid}, heads::Int64, chout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        return NoTangent(), NoTangent(), ΔWx, Δa, NoTangent(), NoTangent(), NoTangent()
    end
    return out, gat_attention_pullback
end

# `α = dropout(α, l.dropout)` (conv.jl:139) inside the same kernel: the coefficients are dropped where the weighted sum is formed, the
# mask is a function of (seed, edge position, head) that forward and pullback both evaluate (gnnmp.h: gnnmp_gat_conv_drop_f32) — no
# (H, E') mask or α array exists.  The seed comes from Julia's default RNG, a fresh one per call, like the reference's mask.
attention_seed() = rand(UInt64)
@non_differentiable attention_seed()
function gat_attention_drop(g::GNNGraph{<:COO_T}, Wx::AnyROCMatrix{Float32}, a::ROCMatrix{Float32}, slope::Float32,
                            heads::Int, self_loops::Bool, p::Float32, seed::UInt64)
    out, _ = gat_attention_drop_stats(g, Wx, a, slope, heads, self_loops, p, seed, false)
    return out
end
function gat_attention_drop_stats(g, Wx, a, slope, heads, self_loops, p, seed, want_stats)
    chout = size(Wx, 1) ÷ heads
    out = similar(Wx)
    stats = want_stats ? similar(Wx, 2, heads, g.num_nodes) : nothing
    check(@ccall libgnnmp.gnnmp_gat_conv_drop_f32(plan(g; self_loops).handle::Ptr{Cvoid}, devptr(Wx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
              devptr(a)::Ptr{Cvoid}, slope::Cfloat, p::Cfloat, seed::UInt64, C_NULL::Ptr{Cvoid}, 0::Cint, devptr(out)::Ptr{Cvoid},
              devptr(stats)::Ptr{Cvoid}, heads::Int64, chout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out, stats
end
function ChainRulesCore.rrule(::typeof(gat_attention_drop), g::GNNGraph{<:COO_T}, Wx::AnyROCMatrix{Float32},
                              a::ROCMatrix{Float32}, slope::Float32, heads::Int, self_loops::Bool, p::Float32, seed::UInt64)
    out, stats = gat_attention_drop_stats(g, Wx, a, slope, heads, self_loops, p, seed, true)
    function gat_attention_drop_pullback(Δ̄)
        Δ = convert(typeof(out), unthunk(Δ̄))
        chout = size(Wx, 1) ÷ heads
        N = g.num_nodes
        ΔWx, Δa = similar(Wx), similar(a)
        line = similar(Wx, 4, heads, N)
        dsd, dss = similar(Wx, heads, N), similar(Wx, heads, N)
        check(@ccall libgnnmp.gnnmp_gat_conv_grad_drop_f32(plan(g; self_loops).handle::Ptr{Cvoid},
                  plan(g; self_loops, transposed = true).handle::Ptr{Cvoid}, devptr(Wx)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
                  devptr(a)::Ptr{Cvoid}, slope::Cfloat, p::Cfloat, seed::UInt64, devptr(stats)::Ptr{Cvoid}, devptr(Δ)::Ptr{Cvoid},
                  devptr(line)::Ptr{Cvoid}, devptr(dsd)::Ptr{Cvoid}, devptr(dss)::Ptr{Cvoid}, devptr(ΔWx)::Ptr{Cvoid},
                  C_NULL::Ptr{Cvoid}, devptr(Δa)::Ptr{Cvoid}, heads::Int64, chout::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        return NoTangent(), NoTangent(), ΔWx, Δa, NoTangent(), NoTangent(), NoTangent(), NoTangent(), NoTangent()
    end
    return out, gat_attention_drop_pullback
end

function GNNlib.gat_conv(l, g::GNNGraph{<:COO_T}, x::AnyROCMatrix{Float32}, e::Nothing = nothing)
    check_num_nodes(g, x)
    @assert l.dense_e === nothing "Input edge features required for this layer"
    _, chout = l.channel
    Wx = l.dense_x(x)                                              # (C*H, N)
    if l.dropout > 0
        (l.heads * chout) ÷ (chout % 4 == 0 ? 4 : (chout % 2 == 0 ? 2 : 1)) <= 64 ||    # rows wider than a wave: the generic path
            return invoke(GNNlib.gat_conv, Tuple{Any, GNNlib.AbstractGNNGraph, Any, Nothing}, l, g, x, e)
        y = gat_attention_drop(g, Wx, l.a, Float32(l.negative_slope), l.heads, l.add_self_loops, Float32(l.dropout), attention_seed())
    else
        y = gat_attention(g, Wx, l.a, Float32(l.negative_slope), l.heads, l.add_self_loops)
    end
    if !l.concat
        y = reshape(mean(reshape(y, chout, l.heads, :), dims = 2), chout, :)
    end
    return l.σ.(y .+ l.bias)
end

# ---- the other attention layers on the same one-pass kernel (gnnmp_attn_conv_f32) -----------------------------------------
# mode 1: gatv2_conv (conv.jl:171-214; Q = Wxi, K = Wxj, a = l.a (C, H) as stored)   mode 2: transformer_conv attention
# (conv.jl:553-616; Q = W3x, K = W4x, V = W2x, scale = l.sqrt_out)   mode 3: agnn_conv (conv.jl:337-352; K = x, scale = l.β[1])
function attention(g::GNNGraph{<:COO_T}, mode::Int, K::AnyROCMatrix{Float32}; Q = nothing, V = nothing, a = nothing,
                   slope = 0.2f0, scale = 1f0, bias = nothing, relu = false, heads::Int = 1, self_loops::Bool,
                   dropout = 0f0, seed::UInt64 = UInt64(0))
    out = similar(K)
    if dropout > 0     # gatv2_conv's `α = dropout(α, l.dropout)` (conv.jl:191) inside the kernel; pass seed = attention_seed()
        check(@ccall libgnnmp.gnnmp_attn_conv_drop_f32(plan(g; self_loops).handle::Ptr{Cvoid}, mode::Cint, devptr(Q)::Ptr{Cvoid},
                                                       devptr(K)::Ptr{Cvoid}, devptr(V)::Ptr{Cvoid}, devptr(a)::Ptr{Cvoid},
                                                       Float32(slope)::Cfloat, Float32(scale)::Cfloat, Float32(dropout)::Cfloat,
                                                       seed::UInt64, devptr(bias)::Ptr{Cvoid}, Cint(relu)::Cint,
                                                       devptr(out)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, heads::Int64,
                                                       (size(K, 1) ÷ heads)::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
        return out
    end
    check(@ccall libgnnmp.gnnmp_attn_conv_f32(plan(g; self_loops).handle::Ptr{Cvoid}, mode::Cint, devptr(Q)::Ptr{Cvoid},
                                              devptr(K)::Ptr{Cvoid}, devptr(V)::Ptr{Cvoid}, devptr(a)::Ptr{Cvoid},
                                              Float32(slope)::Cfloat, Float32(scale)::Cfloat, devptr(bias)::Ptr{Cvoid},
                                              Cint(relu)::Cint, devptr(out)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid},
                                              heads::Int64, (size(K, 1) ÷ heads)::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end

# ---- a whole graph-classification forward in one launch: GNNChain(GraphConv..., GlobalPool, Dense) ------------------------------
# examples/graph_classification_tudataset.jl:79-82 on a batched GNNGraph (MLUtils.batch, GNNGraphs/src/transform.jl:682-709).  The layer
# objects are read through their field names only (weight1, weight2, bias, σ, aggr — GraphNeuralNetworks/src/layers/conv.jl:226-245 —
# and Flux.Dense's weight, bias), so this extension of GNNlib needs no dependency on the Flux front-end; a front-end method
# `(c::GNNChain)(g::GNNGraph, x::AnyROCMatrix)` can try `graphconv_chain` first and fall back to its layer loop on `nothing`.
# Julia's (out, in) weight matrices are passed AS STORED (w_layout = 1).  Forward only (inference / evaluation): no rrule.
mutable struct ChainJobs
    handle::Ptr{Cvoid}
    function ChainJobs(seg_ptr::ROCVector{Int64}, G::Int)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(@ccall libgnnmp.gnnmp_chain_jobs_create(h::Ptr{Ptr{Cvoid}}, devptr(seg_ptr)::Ptr{Cvoid}, G::Int64,
                                                      stream_ptr()::Ptr{Cvoid})::Cint)
        j = new(h[])
        finalizer(j -> (@ccall libgnnmp.gnnmp_chain_jobs_destroy(j.handle::Ptr{Cvoid})::Cint), j)
        return j
    end
    # packed ON THE DEVICE (no copy of the sizes to the host, no synchronisation): the caller states what it knows on the host — the batch's
    # nodes, its largest member, whether a member is empty (num_nodes of every member graph is a host integer, gnngraph.jl:108-117)
    function ChainJobs(seg_ptr::ROCVector{Int64}, G::Int, n_rows::Int, max_graph::Int, has_empty::Bool)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(@ccall libgnnmp.gnnmp_chain_jobs_pack(h::Ptr{Ptr{Cvoid}}, devptr(seg_ptr)::Ptr{Cvoid}, G::Int64, n_rows::Int64,
                                                    max_graph::Int64, has_empty::Cint, stream_ptr()::Ptr{Cvoid})::Cint)
        j = new(h[])
        finalizer(j -> (@ccall libgnnmp.gnnmp_chain_jobs_destroy(j.handle::Ptr{Cvoid})::Cint), j)
        return j
    end
end
function chain_jobs_info(j::ChainJobs)
    info = zeros(Int64, 5)
    check(@ccall libgnnmp.gnnmp_chain_jobs_info(j.handle::Ptr{Cvoid}, info::Ptr{Int64})::Cint)
    return (jobs = info[1], graphs = info[2], rows = info[3], max_graph = info[4], fill = info[5] / 1000)
end
# first node of every member graph (0-based rows, G + 1 entries) from the sorted indicator `batch` builds
function segment_bounds(g::GNNGraph)
    gi = GNNGraphs.graph_indicator(g)
    sp = ROCVector{Int64}(undef, g.num_graphs + 1)
    check(@ccall libgnnmp.gnnmp_segment_bounds(devptr(gi)::Ptr{Cvoid}, sizeof(eltype(gi))::Cint, 1::Cint, g.num_nodes::Int64,
                                               g.num_graphs::Int64, devptr(sp)::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint)
    return sp
end
# per-batch constants, cached like the plans (identity of the indicator vector)
# Per-batch constants, keyed by the identity of the batch's graph_indicator like the plans are by (s, t): an entry dies with that array
# (a finalizer clears its flag) and every miss sweeps the dead ones — a training loop makes a new batch every step, and a ChainJobs holds
# ~16 MB of device memory at the config-5 size.
mutable struct ChainEntry
    seg_ptr::ROCVector{Int64}
    jobs::ChainJobs
    @atomic alive::Bool
end
const CHAIN_CACHE = Dict{UInt, ChainEntry}()
function chain_constants(g::GNNGraph)
    gi = GNNGraphs.graph_indicator(g)
    key = objectid(gi)
    lock(PLANS_LOCK) do
        ent = get(CHAIN_CACHE, key, nothing)
        if ent === nothing || !(@atomic ent.alive)
            filter!(kv -> (@atomic kv.second.alive), CHAIN_CACHE)
            sp = segment_bounds(g)
            ent = ChainEntry(sp, ChainJobs(sp, g.num_graphs), true)
            let ent = ent
                finalizer(_ -> (@atomic ent.alive = false), gi)
            end
            CHAIN_CACHE[key] = ent
        end
        (ent.seg_ptr, ent.jobs)
    end
end
@non_differentiable chain_constants(::Any...)

function graphconv_chain(convs::Tuple, pool_aggr, head_weight::ROCMatrix{Float32}, head_bias, g::GNNGraph{<:COO_T},
                         x::AnyROCMatrix{Float32})
    check_num_nodes(g, x)
    L = length(convs)
    aggr = convs[1].aggr
    (aggr === (+) || aggr === mean) && (pool_aggr === (+) || pool_aggr === mean) || return nothing
    all(c -> c.aggr === aggr && act_code(c.σ) !== nothing, convs) || return nothing
    # TUDataset node features are one-hot labels (MUTAG 7, PROTEINS 3): any input width is zero-padded — exact — to 16 when that makes the
    # chain the wave-pair kernel's shape (16 => 128 => 128), else to the next multiple of 4; x (Din, N) grows by rows, the first layer's
    # (out, in) weights by columns
    din = size(x, 1)
    widths = [size(c.weight1, 1) for c in convs]
    din_p = (L == 2 && widths == [128, 128] && din <= 16) ? 16 : 4 * cld(din, 4)
    w1r, w1a = convs[1].weight1, convs[1].weight2
    if din_p != din
        x = vcat(x, AMDGPU.zeros(Float32, din_p - din, size(x, 2)))
        w1r = hcat(w1r, AMDGPU.zeros(Float32, widths[1], din_p - din))
        w1a = hcat(w1a, AMDGPU.zeros(Float32, widths[1], din_p - din))
    end
    dims = Int64[din_p; widths...]
    nout = size(head_weight, 1)
    sp, jobs = chain_constants(g)
    nfloats = @ccall libgnnmp.gnnmp_graphconv_chain_scratch_floats(g.num_nodes::Int64, L::Cint, dims::Ptr{Int64}, nout::Int64)::Int64
    nfloats < 0 && return nothing
    scratch = ROCVector{Float32}(undef, nfloats)
    out = similar(x, nout, g.num_graphs)
    wr = Ptr{Cvoid}[k == 1 ? devptr(w1r) : devptr(convs[k].weight1) for k in 1:L]
    wa = Ptr{Cvoid}[k == 1 ? devptr(w1a) : devptr(convs[k].weight2) for k in 1:L]
    bs = Ptr{Cvoid}[c.bias isa AbstractArray ? devptr(c.bias) : C_NULL for c in convs]
    acts = Cint[act_code(c.σ) for c in convs]
    hb = head_bias isa AbstractArray ? head_bias : nothing
    GC.@preserve convs head_weight hb scratch w1r w1a x begin
        st = @ccall libgnnmp.gnnmp_graphconv_chain_f32(plan(g).handle::Ptr{Cvoid}, jobs.handle::Ptr{Cvoid}, devptr(sp)::Ptr{Cvoid},
                  g.num_graphs::Int64, devptr(x)::Ptr{Cvoid}, L::Cint, dims::Ptr{Int64}, wr::Ptr{Ptr{Cvoid}}, wa::Ptr{Ptr{Cvoid}},
                  bs::Ptr{Ptr{Cvoid}}, acts::Ptr{Cint}, 1::Cint, aggr_code(aggr)::Cint, aggr_code(pool_aggr)::Cint,
                  devptr(head_weight)::Ptr{Cvoid}, devptr(hb)::Ptr{Cvoid}, nout::Int64, devptr(scratch)::Ptr{Cvoid},
                  devptr(out)::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint
    end
    st == EUNSUPPORTED && return nothing                           # outside the fused kernels' envelope: run the layers one by one
    check(st)
    return out
end

# ---- a NEW batch every step without a sort and without a host synchronisation ----------------------------------------------------------
# examples/graph_classification_tudataset.jl:70-71, 97-104: DataLoader(...; shuffle = true, collate = true) calls MLUtils.batch(gs[idx])
# (GNNGraphs/src/transform.jl:682-709) on the CPU and uploads the result, every step.  With the dataset resident on the device —
# `DeviceDataset(gs)` = batch(gs) |> gpu once, its plan, the node offsets, and the members' sizes as the host integers they already are
# (gnngraph.jl:108-117) — a step's batch is `batch_from(ds, ids)`: the batch's plan from gnnmp_plan_select (the dst-sorted CSR of a batch is
# the concatenation of its members' CSRs: two launches), its COO from gnnmp_plan_edge_index, its features from one gnnmp_gather_f32, the
# fused chain's wave jobs from gnnmp_chain_jobs_pack; the plan and the jobs are registered in the caches above under the new arrays'
# identities, so every layer call on the returned GNNGraph finds them.  Members appear in the order of `ids`, like batch(gs[ids]).
struct DeviceDataset{G <: GNNGraph}
    gall::G                       # MLUtils.batch(all member graphs), COO on the device
    num_nodes::Vector{Int64}      # of every member graph (host)
    num_edges::Vector{Int64}
    node_ptr::ROCVector{Int64}    # 0-based first node of every member graph, G + 1 entries
end
function DeviceDataset(gall::GNNGraph{<:COO_T}, num_nodes::Vector{Int64}, num_edges::Vector{Int64})
    @assert length(num_nodes) == gall.num_graphs == length(num_edges)
    @assert sum(num_nodes) == gall.num_nodes && sum(num_edges) == gall.num_edges
    return DeviceDataset(gall, num_nodes, num_edges, ROCVector{Int64}(vcat(0, cumsum(num_nodes))))
end

adopt_plan(h::Ptr{Cvoid}) = Plan(h)
function release!(p::Plan)
    check(@ccall libgnnmp.gnnmp_plan_release(p.handle::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint)
    p.handle = C_NULL
    return nothing
end

function batch_from(ds::DeviceDataset, ids::Vector{Int}; ids_dev::ROCVector{Int64} = ROCVector{Int64}(ids))
    isempty(ids) && throw(ArgumentError("Cannot batch an empty vector of graphs"))
    gall = ds.gall
    k = length(ids)
    n_rows = sum(@view ds.num_nodes[ids])
    n_edges = sum(@view ds.num_edges[ids])
    seg = ROCVector{Int64}(undef, k + 1)
    nmap = ROCVector{Int32}(undef, n_rows)
    gi = ROCVector{Int64}(undef, n_rows)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(@ccall libgnnmp.gnnmp_plan_select(h::Ptr{Ptr{Cvoid}}, plan(gall).handle::Ptr{Cvoid}, devptr(ds.node_ptr)::Ptr{Cvoid},
                                            gall.num_graphs::Int64, devptr(ids_dev)::Ptr{Cvoid}, 8::Cint, 1::Cint, k::Int64,
                                            n_rows::Int64, n_edges::Int64, devptr(seg)::Ptr{Cvoid}, devptr(nmap)::Ptr{Cvoid},
                                            devptr(gi)::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint)
    p = adopt_plan(h[])
    s, t = ROCVector{Int64}(undef, n_edges), ROCVector{Int64}(undef, n_edges)
    check(@ccall libgnnmp.gnnmp_plan_edge_index(p.handle::Ptr{Cvoid}, 8::Cint, 1::Cint, devptr(s)::Ptr{Cvoid}, devptr(t)::Ptr{Cvoid},
                                                stream_ptr()::Ptr{Cvoid})::Cint)
    x = gall.ndata.x
    D = size(x, 1)
    xb = similar(x, D, n_rows)
    check(@ccall libgnnmp.gnnmp_gather_f32(devptr(x)::Ptr{Cvoid}, devptr(nmap)::Ptr{Cvoid}, 4::Cint, 0::Cint, n_rows::Int64,
                                           devptr(xb)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    g = GNNGraph((s, t, nothing), n_rows, n_edges, k, gi, GNNGraphs.DataStore(n_rows, (; x = xb)), GNNGraphs.DataStore(n_edges),
                 GNNGraphs.DataStore(k))
    jobs = ChainJobs(seg, k, n_rows, maximum(@view ds.num_nodes[ids]), any(==(0), @view ds.num_nodes[ids]))
    lock(PLANS_LOCK) do
        ent = PlanEntry(p, true)
        cent = ChainEntry(seg, jobs, true)
        let ent = ent, cent = cent
            finalizer(_ -> (@atomic ent.alive = false), s)
            finalizer(_ -> (@atomic ent.alive = false), t)
            finalizer(_ -> (@atomic cent.alive = false), gi)
        end
        PLANS[PlanKey(objectid(s), objectid(t), n_rows, false, false)] = ent
        CHAIN_CACHE[objectid(gi)] = cent
    end
    return g
end

# the plan of MLUtils.batch(gs) from the members' cached plans (gnnmp_plan_concat): for a `batch` method on device graphs that keeps the
# members' plans alive — `gs` are the member graphs (COO on the device), `gb` the batched graph MLUtils.batch built from them
function register_concat_plan!(gb::GNNGraph{<:COO_T}, gs::Vector{<:GNNGraph}; self_loops::Bool = false)
    handles = Ptr{Cvoid}[plan(m; self_loops).handle for m in gs]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve gs begin
        check(@ccall libgnnmp.gnnmp_plan_concat(h::Ptr{Ptr{Cvoid}}, handles::Ptr{Ptr{Cvoid}}, length(gs)::Int64, C_NULL::Ptr{Cvoid},
                                                C_NULL::Ptr{Cvoid}, 8::Cint, 1::Cint, stream_ptr()::Ptr{Cvoid})::Cint)
    end
    p = adopt_plan(h[])
    s, t = edge_index(gb)
    lock(PLANS_LOCK) do
        ent = PlanEntry(p, true)
        let ent = ent
            finalizer(_ -> (@atomic ent.alive = false), s)
            finalizer(_ -> (@atomic ent.alive = false), t)
        end
        PLANS[PlanKey(objectid(s), objectid(t), gb.num_nodes, self_loops, false)] = ent
    end
    return p
end

# ---- the structural augmentations on derived plans (csrc/plan_edit.hip) ------------------------------------------------------------------
# remove_nodes (GNNGraphs/src/transform.jl:212-276), add_edges (:319-353), perturb_edges (:385-420) and add_nodes (:553-561) are applied to
# a fresh batch every step of a contrastive training loop and the result is convolved at once.  The child's dst-sorted CSR is a filtered,
# relabelled copy of the parent's: gnnmp_plan_remove_nodes / gnnmp_plan_add_edges write it from the parent's cached plan without a sort of
# the parent's edges, and the plan is registered under the child's arrays like batch_from does, so every layer call on the child finds it.
# The same call on the parent's self-looped or transposed plan (add_edges: with the pair swapped) gives the child's; node data is gathered
# by the node map, edge weights by the edge map.  p::AbstractFloat draws the library's mask (a function of (seed, node)), not Julia's RNG.
const GNNMP_EBOUNDS = Cint(-2)      # include/gnnmp.h: gnnmp_status

function register_child_plan!(h::Ptr{Cvoid}, s, t, n::Integer; self_loops::Bool = false)
    p = adopt_plan(h)
    lock(PLANS_LOCK) do
        ent = PlanEntry(p, true)
        let ent = ent
            finalizer(_ -> (@atomic ent.alive = false), s)
            finalizer(_ -> (@atomic ent.alive = false), t)
        end
        PLANS[PlanKey(objectid(s), objectid(t), n, self_loops, false)] = ent
    end
    return p
end

function remove_nodes_from(g::GNNGraph{<:COO_T}, nodes::Union{ROCVector{Int64}, Nothing}; p::Float32 = 0.0f0, seed::UInt64 = rand(UInt64))
    N, E = g.num_nodes, g.num_edges
    nmap, emap = ROCVector{Int32}(undef, N), ROCVector{UInt32}(undef, E)
    total = zeros(Int64, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall libgnnmp.gnnmp_plan_remove_nodes(h::Ptr{Ptr{Cvoid}}, plan(g).handle::Ptr{Cvoid}, devptr(nodes)::Ptr{Cvoid}, 8::Cint, 1::Cint,
                                                 (nodes === nothing ? 0 : length(nodes))::Int64, p::Cfloat, seed::UInt64,
                                                 devptr(nmap)::Ptr{Cvoid}, C_NULL::Ptr{Cvoid}, devptr(emap)::Ptr{Cvoid},
                                                 total::Ptr{Int64}, stream_ptr()::Ptr{Cvoid})::Cint
    rc == GNNMP_EBOUNDS && throw(BoundsError(1:N, "remove_nodes: a listed node is outside the graph"))
    check(rc)
    n2, e2 = total
    s, t = ROCVector{Int64}(undef, e2), ROCVector{Int64}(undef, e2)
    check(@ccall libgnnmp.gnnmp_plan_edge_index(h[]::Ptr{Cvoid}, 8::Cint, 1::Cint, devptr(s)::Ptr{Cvoid}, devptr(t)::Ptr{Cvoid},
                                                stream_ptr()::Ptr{Cvoid})::Cint)
    register_child_plan!(h[], s, t, n2)
    w = get_edge_weight(g)
    w2 = w === nothing ? nothing : similar(w, e2)
    w === nothing || check(@ccall libgnnmp.gnnmp_gather_f32(devptr(w)::Ptr{Cvoid}, devptr(emap)::Ptr{Cvoid}, 4::Cint, 0::Cint, e2::Int64,
                                                            devptr(w2)::Ptr{Cvoid}, 1::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    x = g.ndata.x
    D = size(x, 1)
    x2 = similar(x, D, n2)
    check(@ccall libgnnmp.gnnmp_gather_f32(devptr(x)::Ptr{Cvoid}, devptr(nmap)::Ptr{Cvoid}, 4::Cint, 0::Cint, n2::Int64,
                                           devptr(x2)::Ptr{Cvoid}, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return GNNGraph((s, t, w2), n2, e2, g.num_graphs, g.graph_indicator, GNNGraphs.DataStore(n2, (; x = x2)), GNNGraphs.DataStore(e2),
                    g.gdata)
end

# snew === nothing: perturb_edges — m pairs drawn on the device, uniform over the ordered pairs of distinct nodes, written to snew / tnew
function add_edges_from(g::GNNGraph{<:COO_T}, snew::Union{ROCVector{Int64}, Nothing}, tnew::Union{ROCVector{Int64}, Nothing}, m::Int,
                        num_nodes::Int = g.num_nodes; seed::UInt64 = rand(UInt64))
    so = snew === nothing ? ROCVector{Int64}(undef, m) : nothing
    to = tnew === nothing ? ROCVector{Int64}(undef, m) : nothing
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall libgnnmp.gnnmp_plan_add_edges(h::Ptr{Ptr{Cvoid}}, plan(g).handle::Ptr{Cvoid}, devptr(snew)::Ptr{Cvoid},
                                              devptr(tnew)::Ptr{Cvoid}, 8::Cint, 1::Cint, m::Int64, num_nodes::Int64, seed::UInt64,
                                              devptr(so)::Ptr{Cvoid}, devptr(to)::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint
    rc == GNNMP_EBOUNDS && throw(AssertionError("minimum(snew) >= 1 && minimum(tnew) >= 1"))
    check(rc)
    E2 = g.num_edges + m
    s, t = ROCVector{Int64}(undef, E2), ROCVector{Int64}(undef, E2)
    check(@ccall libgnnmp.gnnmp_plan_edge_index(h[]::Ptr{Cvoid}, 8::Cint, 1::Cint, devptr(s)::Ptr{Cvoid}, devptr(t)::Ptr{Cvoid},
                                                stream_ptr()::Ptr{Cvoid})::Cint)
    register_child_plan!(h[], s, t, num_nodes)
    return s, t      # the caller builds the GNNGraph with cat_features of the weights, edata and ndata, as add_edges does (transform.jl:332-352)
end

# ---- the fused steps of the graph-classification chain's pullback (INTEGRATION.md §2f; examples/graph_classification_tudataset.jl:79-82) ----
# Thin wrappers over the three round-5 entry points; a chain-level rrule strings them together exactly like the tested Python mirror
# (gnnmp/backward.py: _GraphChainFn.backward) — same calls, same order, bit-identical gradients to the layer-by-layer rules above.
# Δz = relu'(y) .* gather(Δpool, graph_indicator) (.* inv_count[graph] for mean pooling): reduce_nodes' pullback + the activation's, one pass
function pool_grad_act(Δpool::ROCMatrix{Float32}, gi::ROCVector{I}, inv_count::Union{Nothing, ROCVector{Float32}},
                       y::ROCMatrix{Float32}, σ) where {I <: Union{Int32, Int64}}
    D, N = size(y)
    code = act_code(σ)
    # an activation the kernel cannot differentiate is an error, never "identity": that would be a silently wrong gradient
    code === nothing && throw(ArgumentError("pool_grad_act: σ must be identity or relu (got $(σ)); use the layer-by-layer rules"))
    Δz = similar(y)
    check(@ccall libgnnmp.gnnmp_pool_grad_act_f32(devptr(Δpool)::Ptr{Cvoid}, devptr(gi)::Ptr{Cvoid}, sizeof(I)::Cint, 1::Cint,
              devptr(inv_count)::Ptr{Cvoid}, devptr(y)::Ptr{Cvoid}, code::Cint, devptr(Δz)::Ptr{Cvoid},
              N::Int64, size(Δpool, 2)::Int64, D::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return Δz
end
# (ΔW1, ΔW2, Δb) = (Δz * x1', Δz * x2', sum(Δz, dims = 2)) from ONE read of Δz; nothing if the shape is outside the entry point's envelope
function dense_grad_w2(Δz::ROCMatrix{Float32}, x1::AnyROCMatrix{Float32}, x2::AnyROCMatrix{Float32})
    Dout, N = size(Δz)
    K1, K2 = size(x1, 1), size(x2, 1)
    K1 % 16 == 0 || return nothing
    nws = @ccall libgnnmp.gnnmp_dense_grad_w2_workspace(N::Int64, Dout::Int64, K1::Int64, K2::Int64)::Int64
    ws = AMDGPU.zeros(Float32, max(nws, 1))
    out = ROCVector{Float32}(undef, Dout * (K1 + K2) + Dout)
    check(@ccall libgnnmp.gnnmp_dense_grad_w2_f32(devptr(Δz)::Ptr{Cvoid}, devptr(x1)::Ptr{Cvoid}, K1::Int64, devptr(x2)::Ptr{Cvoid},
              K2::Int64, N::Int64, Dout::Int64, devptr(out)::Ptr{Cvoid}, devptr(ws)::Ptr{Cvoid}, length(ws)::Int64,
              stream_ptr()::Ptr{Cvoid})::Cint)
    # C row-major [Dout][K] = Julia (K, Dout): transpose like dense's pullback does
    ΔW1 = permutedims(reshape(view(out, 1:(Dout * K1)), K1, Dout))
    ΔW2 = permutedims(reshape(view(out, (Dout * K1 + 1):(Dout * (K1 + K2))), K2, Dout))
    return ΔW1, ΔW2, out[(Dout * (K1 + K2) + 1):end]
end
# out = relu'(mask_y) .* (addend .+ Aᵀ xj): graph_conv's x-pullback with its sum and the relu' of the layer below in the row kernel's epilogue
function propagate_add_mask(g::DeviceGraph, xj::ROCMatrix{Float32}, addend::Union{Nothing, ROCMatrix{Float32}},
                            mask_y::Union{Nothing, ROCMatrix{Float32}})
    out = similar(xj)
    check(@ccall libgnnmp.gnnmp_propagate_add_mask_f32(plan(g; transposed = true).handle::Ptr{Cvoid}, 0::Cint, devptr(xj)::Ptr{Cvoid},
              C_NULL::Ptr{Cvoid}, devptr(addend)::Ptr{Cvoid}, devptr(mask_y)::Ptr{Cvoid}, devptr(out)::Ptr{Cvoid}, size(xj, 1)::Int64,
              stream_ptr()::Ptr{Cvoid})::Cint)
    return out
end

# ---- the placement arena (csrc/arena.hip): outputs of the gather kernels in a placement class other than their gathered matrix's ---------
# MI355X: device memory falls into three placement classes; propagate / the fused layers / the one-pass attention run 6 % slower when the
# matrix they gather from and their output share a class.  `arena_similar(x, dims...)` = similar(x, dims...) from an arena range whose
# class differs from x's; node features allocated with `arena_array` have a known class from the start.  Arena arrays are bump-allocated
# and live until `arena_reset!()`: use them for buffers that persist across steps (layer outputs of a fixed shape), not for temporaries.
mutable struct Arena
    handle::Ptr{Cvoid}
    n_classes::Int
end
const ARENA = Ref{Union{Nothing, Arena}}(nothing)
const ARENA_TRIED = Ref(false)
function arena(; gib_per_class::Real = parse(Float64, get(ENV, "GNNMP_ARENA_GIB", "4")))
    (ARENA[] === nothing && !ARENA_TRIED[]) || return ARENA[]
    ARENA_TRIED[] = true
    # creation works inside the library's probing budget (32 GiB of blocks held, ~0.3 s) and comes back with the classes it found:
    # info[8] (1-based: C's info[7]) = 0 .. 3 of them.  Fewer than two: no placement on this device today, allocate as usual.
    h = Ref{Ptr{Cvoid}}(C_NULL)
    st = @ccall libgnnmp.gnnmp_arena_create(h::Ptr{Ptr{Cvoid}}, round(Int64, gib_per_class * 2.0^30)::Int64, 3::Cint,
                                            0::Int64, stream_ptr()::Ptr{Cvoid})::Cint
    st == 0 || return nothing
    info = zeros(Int64, 14)
    check(@ccall libgnnmp.gnnmp_arena_info(h[]::Ptr{Cvoid}, info::Ptr{Int64})::Cint)
    if info[8] < 2
        @ccall libgnnmp.gnnmp_arena_destroy(h[]::Ptr{Cvoid})::Cint
        return nothing
    end
    a = Arena(h[], Int(info[8]))
    finalizer(q -> (@ccall libgnnmp.gnnmp_arena_destroy(q.handle::Ptr{Cvoid})::Cint), a)
    ARENA[] = a
    return a
end
function arena_class_of(x::ROCArray{Float32})
    a = arena()
    a === nothing && return 0
    cls = Ref{Cint}(0)
    check(@ccall libgnnmp.gnnmp_arena_class_of(a.handle::Ptr{Cvoid}, devptr(x)::Ptr{Cvoid}, sizeof(x)::Int64, cls::Ptr{Cint},
                                               stream_ptr()::Ptr{Cvoid})::Cint)
    return Int(cls[])
end
function arena_array(dims::Dims, cls::Int)
    a = arena()
    a === nothing && return nothing
    ptr = Ref{Ptr{Cvoid}}(C_NULL)
    st = @ccall libgnnmp.gnnmp_arena_alloc(a.handle::Ptr{Cvoid}, cls::Cint, (4 * prod(dims))::Int64, ptr::Ptr{Ptr{Cvoid}})::Cint
    st == 0 || return nothing                                      # range full: the caller allocates as usual
    return unsafe_wrap(ROCArray, Ptr{Float32}(ptr[]), dims; lock = false)
end
function arena_similar(x::ROCArray{Float32}, dims::Int...; avoid = ())
    a = arena()
    a === nothing && return similar(x, dims...)
    bad = (arena_class_of(x), avoid...)
    for c in 0:(a.n_classes - 1)
        c in bad && continue
        y = arena_array(dims, c)
        y === nothing || return y
    end
    return similar(x, dims...)
end
arena_reset!() = (a = arena(); a === nothing || check(@ccall libgnnmp.gnnmp_arena_reset(a.handle::Ptr{Cvoid})::Cint); nothing)

# ---- graph-parallel step for batched graphs (SURVEY.md §8e): shard by graph, ONE all-gather of the per-shard logits -----------------
# Host side of the recipe in INTEGRATION.md §2b.  `sizes` = num_nodes of every member graph BEFORE batching (a host Vector{Int}).
# Returns (rank_of, gather_index, gmax): rank_of[g] (0-based rank) owns member graph g; after the all-gather of `gmax` padded rows per
# rank, row gather_index[g] (0-based) of the (nout, world * gmax) block is graph g.
function shard_by_size(sizes::Vector{Int64}, world::Int)
    G = length(sizes)
    rank_of = Vector{Int32}(undef, G)
    gather_index = Vector{Int64}(undef, G)
    gmax = Ref{Int64}(0)
    check(@ccall libgnnmp.gnnmp_shard_by_size(sizes::Ptr{Int64}, G::Int64, world::Cint, rank_of::Ptr{Int32}, gather_index::Ptr{Int64},
                                              gmax::Ptr{Int64})::Cint)
    return rank_of, gather_index, gmax[]
end
# the one collective: `comm` is the caller's RCCL communicator (an ncclComm_t as a Ptr{Cvoid}, e.g. from NCCL.jl built against RCCL);
# send = this rank's (nout, gmax) logits (padding columns arbitrary), recv = (nout, world * gmax)
function allgather_logits!(recv::ROCMatrix{Float32}, send::ROCMatrix{Float32}, comm::Ptr{Cvoid})
    check(@ccall libgnnmp.gnnmp_allgather_f32(comm::Ptr{Cvoid}, devptr(send)::Ptr{Cvoid}, devptr(recv)::Ptr{Cvoid},
                                              length(send)::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    return recv
end

# ---- graph prep that the CUDA extension sends to the CPU (GNNGraphs/ext/GNNGraphsCUDAExt.jl:24-30) ---------------------------
function GNNGraphs.sort_edge_index(u::ROCVector{I}, v::ROCVector{I}) where {I <: Union{Int32, Int64}}
    uo, vo = similar(u), similar(v)
    check(@ccall libgnnmp.gnnmp_sort_edge_index(devptr(u)::Ptr{Cvoid}, devptr(v)::Ptr{Cvoid}, sizeof(I)::Cint, 1::Cint,
                                                length(u)::Int64, devptr(uo)::Ptr{Cvoid}, devptr(vo)::Ptr{Cvoid},
                                                stream_ptr()::Ptr{Cvoid})::Cint)
    return uo, vo
end

# ---- random-walk positional encodings (GNNGraphs/src/transform.jl:975-990) -------------------------------------------------------------
# The reference multiplies N x N matrices and keeps their diagonals; the library walks every member graph of a batch inside LDS
# (gnnmp.h: gnnmp_random_walk_pe_f32).  The job record is gnnmp_rwpe_t, field for field.  (walk_length, num_nodes) column-major is the
# library's [N][walk_length].  Like the rest of this file: written against the reference's sources, never executed.
struct RwpeJob
    w::Ptr{Cvoid}
    graph_ptr::Ptr{Cvoid}
    idx_bytes::Cint
    n_graphs::Int64
    walk_length::Int64
    out::Ptr{Cvoid}
end
# A method of the reference's own function, random_walk_pe(g::GNNGraph, walk_length::Int) (transform.jl:975): imported by name, so the
# definition below extends it; graphs that are not on the device go on to the reference's method.
import GNNGraphs: random_walk_pe
function random_walk_pe(g::GNNGraph{<:COO_T}, walk_length::Int)
    s, _ = edge_index(g)
    s isa ROCVector || return invoke(random_walk_pe, Tuple{GNNGraph, Int}, g, walk_length)
    out = ROCMatrix{Float32}(undef, walk_length, g.num_nodes)
    g.num_nodes == 0 && return out
    w = get_edge_weight(g)
    w = w === nothing ? nothing : Float32.(w)
    sp = g.num_graphs > 1 ? segment_bounds(g) : nothing
    p = plan(g; transposed = true)
    job = Ref(RwpeJob(devptr(w), devptr(sp), Cint(8), Int64(sp === nothing ? 1 : g.num_graphs), Int64(walk_length), devptr(out)))
    GC.@preserve w sp out job begin
        check(@ccall libgnnmp.gnnmp_random_walk_pe_f32(p.handle::Ptr{Cvoid}, job::Ptr{Cvoid}, stream_ptr()::Ptr{Cvoid})::Cint)
    end
    return out
end

# ---- heterograph attention (GraphNeuralNetworks/src/layers/heteroconv.jl:57-86 over gat_conv / gatv2_conv, conv.jl:112-214) -----------
# One launch finishes every destination row over all of its incoming attention relations (gnnmp.h: gnnmp_hetero_attn_f32).  The records
# are gnnmp_hetero_attn_rel_t and gnnmp_hetero_attn_dst_t, field for field; the tables are host arrays that the call copies into the
# kernel arguments.  Like the rest of this file: written against the reference's sources, never executed.
struct HeteroAttnRel
    plan::Ptr{Cvoid}
    mode::Cint
    Q::Ptr{Cvoid}
    K::Ptr{Cvoid}
    a::Ptr{Cvoid}
    bias::Ptr{Cvoid}
    stats::Ptr{Cvoid}
    negative_slope::Cfloat
    act::Cint
end
struct HeteroAttnDst
    out::Ptr{Cvoid}
    n_dst::Int64
    combine::Cint
    n_rel::Cint
    rels::Ptr{HeteroAttnRel}
end
# dsts: one (out, combine code, Vector{HeteroAttnRel}) per destination type, out a (H * C, n_dst) ROCMatrix{Float32}
function hetero_attn!(dsts::Vector, H::Int, C::Int)
    tabs = [rels for (_, _, rels) in dsts]
    GC.@preserve tabs dsts begin
        recs = [HeteroAttnDst(devptr(out), Int64(size(out, 2)), Cint(combine), Cint(length(rels)), pointer(rels)) for (out, combine, rels) in dsts]
        check(@ccall libgnnmp.gnnmp_hetero_attn_f32(recs::Ptr{Cvoid}, length(recs)::Cint, H::Int64, C::Int64, stream_ptr()::Ptr{Cvoid})::Cint)
    end
    return nothing
end

end # module
