# CGE_hip.jl -- the Julia side of the drop-in: same exported names and positional signatures as
# CGE.jl's hot path (src/CGE.jl:11-21), each a thin `ccall` into libcge_hip.so (include/cge_hip.h).
#
# UNTESTED -- NEVER EXECUTED IN THIS REPOSITORY'S CI: the build image has no `julia` binary (DESIGN.md, "Boundary").
# The Python mirror (cge.jl_amd/api.py) binds the identical C-ABI and is what the parity tests drive;
# this file is the stub a CGE.jl maintainer would add.  Julia arrays are passed as they are: Int64
# 1-based ids, column-major matrices -- the C-ABI was laid out for exactly that.
module CGE_hip

export landmarks, wGCL, wGCL_directed, split_cluster_rss, split_cluster_rss2, split_cluster_size,
       split_cluster_diameter

const LIB = get(ENV, "CGE_HIP_LIB", joinpath(@__DIR__, "..", "csrc", "build", "libcge_hip.so"))

# The reference passes the split rule as a function (src/auxilary.jl:64-67); the C-ABI takes an enum.  The rule
# is mapped BY NAME, so `CGE.split_cluster_rss` (what CGE's own `parseargs` returns) and the placeholders below
# both work.  Use `using CGE: parseargs` next to `using CGE_hip` (a plain `using CGE` would clash on the exported
# `landmarks`, `wGCL`, `wGCL_directed`).
split_cluster_rss() = nothing
split_cluster_rss2() = nothing
split_cluster_size() = nothing
split_cluster_diameter() = nothing
const METHOD_CODE = Dict{String,Cint}("split_cluster_rss" => 0, "split_cluster_rss2" => 1,
                                      "split_cluster_size" => 2, "split_cluster_diameter" => 3)
function method_code(method::Function)
    name = string(nameof(method))
    haskey(METHOD_CODE, name) || throw(ArgumentError("unknown split rule $name (expected one of $(collect(keys(METHOD_CODE))))"))
    return METHOD_CODE[name]
end

mutable struct Ctx
    h::Ptr{Cvoid}
    function Ctx(device::Integer = 0)
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:cge_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint, Ptr{Cvoid}), ref, device, C_NULL)
        rc == 0 || error("cge_create failed with code $rc (no MI355X visible? there is no CPU fallback)")
        c = new(ref[])
        finalizer(x -> (x.h != C_NULL && ccall((:cge_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), c)
        return c
    end
end

const DEFAULT = Ref{Union{Nothing,Ctx}}(nothing)
function ctx()
    if DEFAULT[] === nothing
        DEFAULT[] = Ctx()
        # tear the context down while the HIP runtime is still alive (streams and events must not outlive it)
        atexit(() -> (c = DEFAULT[]; c !== nothing && c.h != C_NULL &&
                      (ccall((:cge_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.h); c.h = C_NULL)))
    end
    return DEFAULT[]
end

lasterr(c::Ctx) = unsafe_string(ccall((:cge_last_error, LIB), Cstring, (Ptr{Cvoid},), c.h))

# status code -> the exception the reference would have thrown
function check(c::Ctx, rc::Cint)
    rc == 0 && return
    msg = lasterr(c)
    rc == -1 && throw(AssertionError(msg))                 # @assert (src/divergence.jl:50,81,303,363)
    rc == -2 && throw(ErrorException("Trying to split homogenous cluster"))       # src/landmarks.jl:166
    rc == -3 && throw(ErrorException("Unexpected empty cluster generated"))       # src/landmarks.jl:298
    error("libcge_hip error $rc: $msg")
end

function set_inputs!(c::Ctx, edges::Matrix{Int}, weights::Vector{Float64}, vweights::Vector{Float64},
                     comm::Matrix{Int}, embedding::Matrix{Float64})
    m, n, d = size(edges, 1), size(embedding, 1), size(embedding, 2)
    src, dst = pointer(edges), pointer(edges, m + 1)      # the two columns of the m x 2 matrix
    GC.@preserve edges weights vweights comm embedding begin
        check(c, ccall((:cge_set_graph, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int64),
                       c.h, src, dst, weights, m, n))
        check(c, ccall((:cge_set_embedding, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64), c.h, embedding, n, d))
        check(c, ccall((:cge_set_vertex_data, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Int64),
                       c.h, comm, vweights, n))
    end
end

# cge_embedding_view (include/cge_hip.h): an embedding as its owner holds it -- element type, layout, leading dimension
struct EmbeddingView
    data::Ptr{Cvoid}
    d::Int64
    ld::Int64        # leading dimension in elements; 0 = packed
    dtype::Cint      # 0 Float64, 1 Float32, 2 Float16, 3 bfloat16
    on_device::Cint
    row_major::Cint  # a Julia Matrix is column-major: 0
end
view_dtype(::Type{Float64}) = Cint(0)
view_dtype(::Type{Float32}) = Cint(1)
view_dtype(::Type{Float16}) = Cint(2)

# The embedding in its own element type (Float32 / Float16 go over the link as they are and are widened on the device; the
# results are those of the Float64 matrix `Float64.(embedding)`).  The graph must be resident (set_inputs! or cge_set_graph).
function set_embedding!(c::Ctx, embedding::Matrix{T}) where {T<:Union{Float64,Float32,Float16}}
    n, d = size(embedding)
    GC.@preserve embedding begin
        v = EmbeddingView(pointer(embedding), d, n, view_dtype(T), 0, 0)
        check(c, ccall((:cge_set_embedding_view, LIB), Cint, (Ptr{Cvoid}, Ref{EmbeddingView}, Int64), c.h, Ref(v), n))
    end
end

# cge_graph_view / cge_vertex_view (include/cge_hip.h): the edge list and the vertex data as their owner holds them
struct GraphView
    src::Ptr{Cvoid}
    dst::Ptr{Cvoid}
    stride::Int64    # in elements: 1 = two columns (a Julia m x 2 Matrix: dst = src + m elements)
    id_dtype::Cint   # 0 Int64, 1 Int32
    base::Cint       # 0, 1, or -1 = the minimum id must be 0 or 1 (src/auxilary.jl:92-98)
    w::Ptr{Cvoid}    # C_NULL = an unweighted list
    w_dtype::Cint    # 0 Float64, 1 Float32
    on_device::Cint
end
struct VertexView
    comm::Ptr{Cvoid}
    id_dtype::Cint
    base::Cint
    vweights::Ptr{Cvoid}   # C_NULL = derive them from the resident edge list (src/auxilary.jl:104-110)
    vw_dtype::Cint
    on_device::Cint
end
id_dtype(::Type{Int64}) = Cint(0)
id_dtype(::Type{Int32}) = Cint(1)

# The edge list as held (an m x 2 Matrix of Int64 or Int32, 0- or 1-based); n = 0: the maximum id.  Returns n.
function set_graph_view!(c::Ctx, edges::Matrix{T}, weights::Union{Nothing,Vector{W}} = nothing; n::Integer = 0,
                         base::Integer = -1) where {T<:Union{Int64,Int32},W<:Union{Float64,Float32}}
    m = size(edges, 1)
    n_out = Ref{Int64}(0)
    GC.@preserve edges weights begin
        w = weights === nothing ? C_NULL : Ptr{Cvoid}(pointer(weights))
        g = GraphView(pointer(edges), pointer(edges, m + 1), 1, id_dtype(T), base, w,
                      weights === nothing ? Cint(0) : view_dtype(W), 0)
        check(c, ccall((:cge_set_graph_view, LIB), Cint, (Ptr{Cvoid}, Ref{GraphView}, Int64, Int64, Ref{Int64}),
                       c.h, Ref(g), m, n, n_out))
    end
    return n_out[]
end

# Communities as held; the vertex weights are derived by the library when `vweights` is nothing.
function set_vertex_view!(c::Ctx, comm::Array{T}, vweights::Union{Nothing,Vector{Float64}} = nothing;
                          base::Integer = -1) where {T<:Union{Int64,Int32}}
    n = length(comm)
    GC.@preserve comm vweights begin
        vw = vweights === nothing ? C_NULL : Ptr{Cvoid}(pointer(vweights))
        v = VertexView(pointer(comm), id_dtype(T), base, vw, 0, 0)
        check(c, ccall((:cge_set_vertex_view, LIB), Cint, (Ptr{Cvoid}, Ref{VertexView}, Int64), c.h, Ref(v), n))
    end
end

# the resident vweight (e.g. the derived one), for wGCL's `vweights` argument
function vertex_weights(c::Ctx, n::Integer)
    out = Vector{Float64}(undef, n)
    check(c, ccall((:cge_vertex_weights, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), c.h, out, n))
    return out
end

# The Louvain hierarchy of the resident graph (cge_louvain_levels; src/clustering.jl:20-24 keeps level 1 of it): one
# (comm 0-based of the n original vertices, n_comm, modularity, rounds) per level; max_levels <= 0: until a level merges nothing
function louvain_levels(c::Ctx, n::Integer; max_levels::Integer = 0)
    count = Ref{Int64}(0)
    check(c, ccall((:cge_louvain_levels, LIB), Cint,
                   (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                   c.h, max_levels, 0, C_NULL, count, C_NULL, C_NULL, C_NULL))
    cap = count[]
    comm, nc, q, rounds = Matrix{Int64}(undef, n, cap), Vector{Int64}(undef, cap), Vector{Float64}(undef, cap), Vector{Int64}(undef, cap)
    check(c, ccall((:cge_louvain_levels, LIB), Cint,
                   (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                   c.h, max_levels, cap, comm, count, nc, q, rounds))
    return [(comm[:, l], nc[l], q[l], rounds[l]) for l in 1:count[]]
end

# ECG communities of the resident graph (cge_ecg, an extension): (comm 0-based of the n vertices, n_comm, modularity on the
# resident graph, modularity on the reweighted graph)
struct EcgArgs
    members::Int64
    w_min::Float64
    seed::Int64
    final_level::Int64
end
function ecg(c::Ctx, n::Integer; members::Integer = 16, w_min::Real = 0.05, seed::Integer = 0, final_level::Integer = -1)
    comm, nc, q, q_ecg = Vector{Int64}(undef, n), Ref{Int64}(0), Ref{Float64}(0.0), Ref{Float64}(0.0)
    a = EcgArgs(members, w_min, seed, final_level)
    check(c, ccall((:cge_ecg, LIB), Cint,
                   (Ptr{Cvoid}, Ref{EcgArgs}, Ptr{Int64}, Ref{Int64}, Ref{Float64}, Ref{Float64}, Ptr{Float64}),
                   c.h, Ref(a), comm, nc, q, q_ecg, C_NULL))
    return comm, nc[], q[], q_ecg[]
end

# The exact link AUC of the resident link model on the resident graph of m rows (cge_link_auc, an extension): every edge row
# against every non-edge.  (less, ties, n_neg, (W, L, Tq)); the exact local score is 1 - L / (W n_neg), the AUC
# (L + Tq / 2) / (W n_neg).  `part` of `nparts`: a share of the pair tiles, the counts of the parts add up.
function link_auc(c::Ctx, m::Integer; part::Integer = 0, nparts::Integer = 1)
    less, ties = Vector{Int64}(undef, m), Vector{Int64}(undef, m)
    nneg, summary = Ref{Int64}(0), Vector{Float64}(undef, 3)
    check(c, ccall((:cge_link_auc, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ref{Int64}, Ptr{Float64}),
                   c.h, part, nparts, less, ties, C_NULL, nneg, summary))
    return less, ties, nneg[], (summary[1], summary[2], summary[3])
end

# The moments of the resident link model over every pair, for the resident communities of n vertices (cge_link_moments, an
# extension): (deg_out, deg_in, B, V, Cobs, n_comm) -- expected degrees, per community bin (the sweep's vect_B layout) the expected
# edge mass, the variance of a draw's edge count and the sweep's vect_C.  diag adds the self pairs as the exact-mode loops do.
function link_moments(c::Ctx, n::Integer, directed::Bool; diag::Bool = false)
    nc = Ref{Int64}(0)
    sig = (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64})
    check(c, ccall((:cge_link_moments, LIB), Cint, sig, c.h, diag, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, nc))
    L = directed ? nc[] * nc[] : nc[] * (nc[] + 1) ÷ 2
    dout, din = Vector{Float64}(undef, n), Vector{Float64}(undef, n)
    B, V, Cobs = Vector{Float64}(undef, L), Vector{Float64}(undef, L), Vector{Float64}(undef, L)
    check(c, ccall((:cge_link_moments, LIB), Cint, sig, c.h, diag, dout, din, B, V, Cobs, nc))
    return dout, din, B, V, Cobs, nc[]
end

# Expected and observed triangles and wedges per vertex of the resident undirected link model and graph of n vertices
# (cge_link_triangles, an extension): (tri_exp, wed_exp, tri_obs, wed_obs, summary) -- summary = the four sums; transitivity is
# summary[1] / summary[2] (model) and summary[3] / summary[4] (graph).
function link_triangles(c::Ctx, n::Integer)
    te, we = Vector{Float64}(undef, n), Vector{Float64}(undef, n)
    to, wo = Vector{Int64}(undef, n), Vector{Int64}(undef, n)
    summary = Vector{Float64}(undef, 4)
    check(c, ccall((:cge_link_triangles, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                   c.h, te, we, to, wo, summary))
    return te, we, to, wo, summary
end

# clusters derived from the resident communities (src/auxilary.jl:199-208): n_clusters = -1, the two pointers are ignored
function landmarks_run_from_comm!(c::Ctx, land::Int, forced::Int, method::Function, directed::Bool)
    N, ne, trunc = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    check(c, ccall((:cge_landmarks_run, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64, Cint, Cint, Ref{Int64}, Ref{Int64}, Ref{Cint}),
                   c.h, C_NULL, C_NULL, -1, land, forced, method_code(method), directed, N, ne, trunc))
    return N[], ne[], trunc[] != 0
end

"""
    landmarks(edges, weights, vweights, clusters, comm, embedding, verbose, land, forced, method, directed)

Drop-in for `CGE.landmarks` (src/landmarks.jl:365-367); returns the same 7-tuple (:465).
"""
function landmarks(edges::Array{Int,2}, weights::Vector{Float64}, vweights::Vector{Float64},
                   clusters::Vector{Vector{Int}}, comm::Array{Int,2}, embedding::Array{Float64,2},
                   verbose::Bool, land::Int, forced::Int, method::Function, directed::Bool)
    c = ctx()
    verbose && println("Starts landmark generation")
    set_inputs!(c, edges, weights, vweights, comm, embedding)
    flat = reduce(vcat, clusters; init = Int[])
    off = Int64[0; cumsum(length.(clusters))]
    N, ne, trunc = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    check(c, ccall((:cge_landmarks_run, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64, Cint, Cint, Ref{Int64}, Ref{Int64}, Ref{Cint}),
                   c.h, flat, off, length(clusters), land, forced, method_code(method), directed, N, ne, trunc))
    trunc[] != 0 && @warn "Requested number of clusters larger than unique no. embeddings. Truncating to $(N[]) landmarks."
    verbose && println("Landmarks generated"); verbose && println("Using $(N[]) landmarks")
    n, d = size(embedding)
    dii, embed, cluster = zeros(N[]), zeros(N[], d), zeros(Int, N[])
    ledges, lw, lweight, v_to_l = zeros(Int, ne[], 2), zeros(ne[]), zeros(N[]), zeros(Int, n)
    check(c, ccall((:cge_landmarks_fetch, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                   c.h, dii, embed, cluster, ledges, lw, lweight, v_to_l))
    return dii, embed, reshape(cluster, :, 1), ledges, lw, lweight, v_to_l
end

# mirrors `cge_trace` (include/cge_hip.h): n_alpha, iters[64], div[64], auc[64]
mutable struct Trace
    n_alpha::Int64
    iters::NTuple{64,Int64}
    div::NTuple{64,Float64}
    auc::NTuple{64,Float64}
    Trace() = new(0, ntuple(_ -> 0, 64), ntuple(_ -> 0.0, 64), ntuple(_ -> 0.0, 64))
end

# mirrors `cge_wgcl_args` (include/cge_hip.h) field for field
struct WgclArgs
    edges_src::Ptr{Int64}; edges_dst::Ptr{Int64}; eweights::Ptr{Float64}; m::Int64
    comm::Ptr{Int64}; n_comm::Int64
    embed::Ptr{Float64}; embed_rows::Int64; d::Int64
    distances::Ptr{Float64}; n_distances::Int64
    vweights::Ptr{Float64}
    init_vweights::Ptr{Float64}; n_init::Int64
    v_to_l::Ptr{Int64}; n_v_to_l::Int64
    init_edges_src::Ptr{Int64}; init_edges_dst::Ptr{Int64}; m_init::Int64
    init_eweights::Ptr{Float64}; init_embed::Ptr{Float64}
    split::Cint; seed::Int64; auc_samples::Int64; verbose::Cint; directed::Cint
    pos_idx::Ptr{Int64}; neg_i::Ptr{Int64}; neg_j::Ptr{Int64}; pos_idx2::Ptr{Int64}; n_sample_sets::Int64
end

function _wgcl(directed::Bool, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l,
               init_edges, init_eweights, init_embed, split, seed, auc_samples, verbose)
    c = ctx()
    m, mi = size(edges, 1), size(init_edges, 1)
    if verbose                                           # the reference's own lines (src/divergence.jl:43-52,75)
        println("auc_samples: $auc_samples")
        println("Graph has $(maximum(edges)) vertices and $m edges")
        !isempty(v_to_l) && mi > 0 && println("Original graph has $(maximum(init_edges)) vertices and $mi edges")
        println("Graph has $(maximum(comm)) communities")
        println("Embedding has $(size(embed, 2)) dimensions")
    end
    out, olen = zeros(7), Ref{Cint}(7)
    GC.@preserve edges eweights comm embed distances vweights init_vweights v_to_l init_edges init_eweights init_embed begin
        a = WgclArgs(pointer(edges), pointer(edges, m + 1), pointer(eweights), m,
                     pointer(comm), size(comm, 1), pointer(embed), size(embed, 1), size(embed, 2),
                     pointer(distances), length(distances), pointer(vweights),
                     pointer(init_vweights), length(init_vweights), pointer(v_to_l), length(v_to_l),
                     mi > 0 ? pointer(init_edges) : C_NULL, mi > 0 ? pointer(init_edges, mi + 1) : C_NULL, mi,
                     pointer(init_eweights), isempty(init_embed) ? C_NULL : pointer(init_embed),
                     split, seed, auc_samples, verbose, directed,
                     C_NULL, C_NULL, C_NULL, C_NULL, 0)     # samples: drawn by the library (pass arrays to own the RNG)
        tr = Trace()
        rc = ccall((:cge_wgcl, LIB), Cint, (Ptr{Cvoid}, Ref{WgclArgs}, Ptr{Float64}, Ref{Cint}, Ref{Trace}),
                   c.h, Ref(a), out, olen, tr)
        check(c, rc)
    end
    write(stderr, "."^tr.n_alpha, "\n")                  # one "." per alpha (src/divergence.jl:140) and the newline (:255)
    return out[1:olen[]]
end

"Drop-in for `CGE.wGCL` (src/divergence.jl:27-31)."
wGCL(edges::Array{Int,2}, eweights::Vector{Float64}, comm::Matrix{Int}, embed::Matrix{Float64},
     distances::Vector{Float64}, vweights::Vector{Float64}, init_vweights::Vector{Float64}, v_to_l::Vector{Int},
     init_edges::Array{Int,2}, init_eweights::Vector{Float64}, init_embed::Matrix{Float64}, split::Bool,
     seed::Int = -1, auc_samples::Int = 10000, verbose::Bool = false) =
    _wgcl(false, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
          init_eweights, init_embed, split, seed, auc_samples, verbose)

"Drop-in for `CGE.wGCL_directed` (src/divergence.jl:282-286)."
wGCL_directed(edges::Array{Int,2}, eweights::Vector{Float64}, comm::Matrix{Int}, embed::Matrix{Float64},
              distances::Vector{Float64}, vweights::Vector{Float64}, init_vweights::Vector{Float64},
              v_to_l::Vector{Int}, init_edges::Array{Int,2}, init_eweights::Vector{Float64},
              init_embed::Matrix{Float64}, split::Bool, seed::Int = -1, auc_samples::Int = 10000,
              verbose::Bool = false) =
    _wgcl(true, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
          init_eweights, init_embed, split, seed, auc_samples, verbose)

"""
    read_table(fn) -> Matrix{Float64}

Stand-in for `readdlm(fn, Float64)` in `parseargs` (src/auxilary.jl:80-168): parallel reader of the library, header
line (node2vec's "n d") skipped as the reference's retry with `skipstart = 1` does.  Needs no GPU.
"""
function read_table(fn::AbstractString; threads::Integer = 0)
    rows, cols, hdr, h = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Ptr{Cvoid}}(C_NULL)
    err = zeros(UInt8, 512)
    rc = ccall((:cge_text_table_open, LIB), Cint,
               (Cstring, Cint, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ptr{UInt8}, Int64),
               fn, threads, rows, cols, hdr, h, err, length(err))
    rc == 0 || throw(ArgumentError(unsafe_string(pointer(err))))
    M = Matrix{Float64}(undef, rows[], cols[])
    rc = ccall((:cge_text_table_parse, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{UInt8}, Int64),
               h[], M, 1, err, length(err))
    ccall((:cge_text_table_close, LIB), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || throw(ArgumentError(unsafe_string(pointer(err))))
    return M
end

end # module
