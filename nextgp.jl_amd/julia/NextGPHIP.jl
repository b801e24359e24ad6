# NextGPHIP.jl -- reference-side binding of libnextgp_hip.so (include/nextgp_hip.h) for NextGP.jl.
#
# NEVER EXECUTED: the build container has no Julia toolchain (SURVEY.md section 8c), so this file has not been run once.  It is
# the stub a NextGP.jl maintainer adds next to src/samplers.jl; every ccall signature below is checked by hand against
# include/nextgp_hip.h, and the same entry points are exercised through Python ctypes (nextgp.jl_amd/_lib.py).  Two seams, both defined by the reference:
#
#   coarse:  replace `samplers.runSampler!(...)` (src/samplers.jl:23, called at src/MCMC.jl:39)
#            by `NextGPHIP.runSampler!(...)`: the whole chain runs on the GPU, the same *Out files
#            are written (src/samplers.jl:56-103).
#   fine:    replace the stored callback `M[set][:funct]` (src/mme.jl:326,333,355, invoked at
#            src/samplers.jl:52) by `NextGPHIP.sweep!`: fixed / random effects stay in Julia,
#            only the per-SNP sweep of one marker set runs on the GPU.
#
# Ownership: Julia arrays are passed for the duration of the ccall only (GC roots them); the
# library copies what it keeps.  All status codes != 0 become `error(msg)`, like src/mme.jl:77.
module NextGPHIP

using DelimitedFiles
using Mmap
using SparseArrays

const LIB = get(ENV, "NEXTGP_HIP_LIB", "libnextgp_hip")

mutable struct Handle
    ptr::Ptr{Cvoid}
end

function check(h::Handle, rc::Integer)
    rc == 0 && return
    msg = unsafe_string(ccall((:ngp_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr))
    error("libnextgp_hip ($rc): $msg")
end

function Handle(; device::Integer=0, seed::Integer=1, chain::Integer=0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:ngp_create, LIB), Int32, (Int32, UInt64, UInt32, Ref{Ptr{Cvoid}}), device, seed, chain, out)
    rc == 0 || error("ngp_create ($rc): " * unsafe_string(ccall((:ngp_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    h = Handle(out[])
    finalizer(x -> ccall((:ngp_destroy, LIB), Int32, (Ptr{Cvoid},), x.ptr), h)
    return h
end

# M[set][:data] is the centred Float64 N x P matrix of src/prepMatVec.jl:129-131 (centre = 0)
set_panel!(h::Handle, data::Matrix{Float64}; centre::Bool=false) =
    check(h, ccall((:ngp_set_panel_f64, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Int32),
                   h.ptr, data, size(data, 1), size(data, 2), stride(data, 2), centre))

# The same panel one marker set after another (M[s].data are separate matrices, src/mme.jl:296-311): no concatenated host copy.
# begin_panel!(h, N, Ptot); panel_columns!(h, col0, M[s].data) for every set (col0 0-based); end_panel!(h) builds mpm and the Gram window.
begin_panel!(h::Handle, N::Integer, P::Integer) = check(h, ccall((:ngp_begin_panel, LIB), Int32, (Ptr{Cvoid}, Int64, Int64), h.ptr, N, P))
panel_columns!(h::Handle, col0::Integer, data::Matrix{Float64}; centre::Bool=false) =
    check(h, ccall((:ngp_panel_columns_f64, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int64, Int32),
                   h.ptr, col0, data, size(data, 2), stride(data, 2), centre))
panel_columns!(h::Handle, col0::Integer, data::Matrix{Float32}; centre::Bool=false) =
    check(h, ccall((:ngp_panel_columns_f32, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Int64, Int32),
                   h.ptr, col0, data, size(data, 2), stride(data, 2), centre))
panel_columns!(h::Handle, col0::Integer, data::Matrix{UInt8}; centre::Bool=true) =      # genotype codes (the compact storage takes only these)
    check(h, ccall((:ngp_panel_columns_u8, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{UInt8}, Int64, Int64, Int32),
                   h.ptr, col0, data, size(data, 2), stride(data, 2), centre))
end_panel!(h::Handle) = check(h, ccall((:ngp_end_panel, LIB), Int32, (Ptr{Cvoid},), h.ptr))

# ---- PLINK binary filesets (include/nextgp_hip.h, ngp_panel_columns_bed) ----
# read_plink("x") or read_plink("x.bed"): the packed columns as an Mmap-backed ceil(n/4) x P Matrix{UInt8} (one column per SNP, as they
# are in the file; nothing is decoded) plus the IDs of x.fam and x.bim.
function read_plink(prefix::AbstractString)
    stem = endswith(prefix, ".bed") ? prefix[1:end-4] : prefix
    fam = [split(l) for l in eachline(stem * ".fam") if !isempty(strip(l))]
    bim = [split(l) for l in eachline(stem * ".bim") if !isempty(strip(l))]
    n = length(fam); P = length(bim); nb = cld(n, 4)
    io = open(stem * ".bed", "r")
    magic = read(io, 3)
    magic == UInt8[0x6c, 0x1b, 0x00] && error("$stem.bed is sample-major (magic 6c 1b 00): only the SNP-major form is read")
    magic == UInt8[0x6c, 0x1b, 0x01] || error("$stem.bed is not a PLINK .bed file (magic 6c 1b 01)")
    filesize(stem * ".bed") == 3 + P * nb || error("$stem.bed: $P SNPs of $n samples need $(3 + P * nb) bytes")
    bed = Mmap.mmap(io, Matrix{UInt8}, (nb, P), 3)
    return (bed = bed, n = n, P = P, fid = [String(t[1]) for t in fam], iid = [String(t[2]) for t in fam],
            chr = [String(t[1]) for t in bim], snp = [String(t[2]) for t in bim], a1 = [String(t[5]) for t in bim], a2 = [String(t[6]) for t in bim])
end

const BED_MISSING = Dict(:error => 0, :mean => 1, :round => 2)   # NGP_BED_MISSING_*

# Packed columns into columns col0 .. (0-based) of the open panel, decoded on the device.  rows: the file's sample (1-based) of every
# panel row, or nothing for file order; allele: count A1 or A2; missing: :error, :mean (fp32 tiles) or :round.  Returns the
# 4 x ncol counts of 0, 1, 2 and missing calls.
function panel_columns_bed!(h::Handle, col0::Integer, bed::Matrix{UInt8}, n_file::Integer; rows=nothing, allele::Integer=1, missing::Symbol=:mean, centre::Bool=true)
    counts = zeros(Int64, 4, size(bed, 2))
    r0 = rows === nothing ? C_NULL : Int64.(rows) .- 1
    check(h, ccall((:ngp_panel_columns_bed, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{UInt8}, Int64, Int64, Int64, Ptr{Int64}, Int32, Int32, Int32, Ptr{Int64}),
                   h.ptr, col0, bed, size(bed, 2), stride(bed, 2), n_file, r0, allele, BED_MISSING[missing], centre, counts))
    return counts
end
# ... and into the open prediction panel: a missing call takes the training mean (:mean) or its rounded code (:round)
function prediction_columns_bed!(h::Handle, col0::Integer, bed::Matrix{UInt8}, n_file::Integer; rows=nothing, allele::Integer=1, missing::Symbol=:mean, centre::Bool=true)
    counts = zeros(Int64, 4, size(bed, 2))
    r0 = rows === nothing ? C_NULL : Int64.(rows) .- 1
    check(h, ccall((:ngp_prediction_columns_bed, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{UInt8}, Int64, Int64, Int64, Ptr{Int64}, Int32, Int32, Int32, Ptr{Int64}),
                   h.ptr, col0, bed, size(bed, 2), stride(bed, 2), n_file, r0, allele, BED_MISSING[missing], centre, counts))
    return counts
end

# one byte per genotype (raw allele counts, e.g. read from a binary file instead of src/prepMatVec.jl:116): centred on the device
set_panel!(h::Handle, data::Matrix{UInt8}; centre::Bool=true) =
    check(h, ccall((:ngp_set_panel_u8, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Int64, Int64, Int64, Int32),
                   h.ptr, data, size(data, 1), size(data, 2), stride(data, 2), centre))

# Storage of the panel on the device, before it is set: :f32 (centred fp32 tiles) or :u8 (the codes themselves, one byte per
# genotype, centred analytically with the Float64 column means -- include/nextgp_hip.h "panel storage").  :u8 takes codes only:
# set_panel!(h, ::Matrix{UInt8}) or load_panel_file!; the centred Float64 M[set].data of the seam cannot be turned back into codes.
set_storage!(h::Handle, storage::Symbol) =
    check(h, ccall((:ngp_set_storage, LIB), Int32, (Ptr{Cvoid}, Int32), h.ptr, storage === :u8 ? 1 : 0))
# at most n streamer workgroups (taller shards, CUs left free for a second chain on the same device); 0 = automatic
set_max_shards!(h::Handle, n::Integer) = check(h, ccall((:ngp_set_max_shards, LIB), Int32, (Ptr{Cvoid}, Int32), h.ptr, n))
function shards_for_chains(h::Handle, chains::Integer)   # the largest max_shards with which `chains` chains share the device side by side
    v = Ref{Int32}(0)
    check(h, ccall((:ngp_shards_for_chains, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}), h.ptr, chains, v))
    return Int(v[])
end

# Binary panel file in place of the text genotype file (src/prepMatVec.jl:116-131): header + codes, 8 or 2 bits per genotype
function write_panel_file(path::AbstractString, G::Matrix{UInt8}; bits::Integer=8)
    rc = ccall((:ngp_write_panel_file, LIB), Int32, (Cstring, Ptr{UInt8}, Int64, Int64, Int64, Int32),
               path, G, size(G, 1), size(G, 2), stride(G, 2), bits)
    rc == 0 || error("ngp_write_panel_file ($rc): path not writable, or codes above 2 with bits = 2")
end
load_panel_file!(h::Handle, path::AbstractString; centre::Bool=true) =
    check(h, ccall((:ngp_load_panel_file, LIB), Int32, (Ptr{Cvoid}, Cstring, Int32), h.ptr, path, centre))

# ---- held-out records: missing phenotypes, cross-validation folds (include/nextgp_hip.h, "held-out records") ----
# rows: 0-BASED records, strictly increasing, after the panel and before set_y!; nothing / an empty vector removes the mask
function set_holdout!(h::Handle, rows::Union{Nothing,Vector{Int64}})
    r = rows === nothing ? Int64[] : rows
    check(h, ccall((:ngp_set_holdout, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int64), h.ptr, isempty(r) ? C_NULL : pointer(r), length(r)))
end
function holdout_layout(h::Handle)       # m: the number of held-out records (0 without a mask)
    m = Ref{Int64}(0)
    check(h, ccall((:ngp_get_holdout_layout, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), h.ptr, m))
    return m[]
end
function holdout_state(h::Handle, N::Integer)   # rows (0-based), yaug (m each), sum_fit, sum_fit2, n_fit (N each, zero off the rows)
    m = holdout_layout(h)
    rows = Vector{Int64}(undef, m); yaug = Vector{Float64}(undef, m)
    s1 = Vector{Float64}(undef, N); s2 = similar(s1); nf = similar(s1)
    check(h, ccall((:ngp_get_holdout, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
                   h.ptr, rows, yaug, s1, s2, nf, m, N))
    return (rows = rows, yaug = yaug, sum_fit = s1, sum_fit2 = s2, n_fit = nf)
end
set_holdout_state!(h::Handle, yaug::Vector{Float64}, sum_fit::Vector{Float64}, sum_fit2::Vector{Float64}, n_fit::Vector{Float64}) =
    check(h, ccall((:ngp_set_holdout_state, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
                   h.ptr, yaug, sum_fit, sum_fit2, n_fit, length(yaug), length(sum_fit)))
"""
    getHoldout(h, N)

Posterior mean and SD of the fitted value (intercept, fixed, random and marker terms) of every held-out record over the kept draws:
`rows` (1-based), `n`, `mean`, `sd`.
"""
function getHoldout(h::Handle, N::Integer)
    st = holdout_state(h, N)
    keep = findall(>(0), st.n_fit)
    mean = st.sum_fit[keep] ./ st.n_fit[keep]
    sd = sqrt.(max.(0.0, st.sum_fit2[keep] ./ st.n_fit[keep] .- mean .^ 2))
    return (rows = keep, n = Int.(st.n_fit[keep]), mean = mean, sd = sd)
end

# ---- liability traits: binary / ordered classes, censored records (include/nextgp_hip.h, "liability traits") ----
# cls: one class 1..C per record (entries of held-out records are not read), 2 <= C <= 8; after the panel and the hold-out mask and
# before set_y!, which then reads y nowhere; varE is held at 1.  nothing removes the classes.
function set_classes!(h::Handle, cls::Union{Nothing,Vector{Int32}}, C::Integer=(cls === nothing ? 0 : Int(maximum(cls))))
    c = cls === nothing ? Int32[] : cls
    check(h, ccall((:ngp_set_liability_classes, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}, Int32), h.ptr, isempty(c) ? C_NULL : pointer(c), isempty(c) ? 0 : C))
end
# rows: 0-BASED records, strictly increasing, none held out; lo < hi, one of them possibly infinite; set_y! reads y off these rows only
function set_censored!(h::Handle, rows::Vector{Int64}, lo::Vector{Float64}, hi::Vector{Float64})
    m = length(rows)
    check(h, ccall((:ngp_set_liability_bounds, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int64),
                   h.ptr, m == 0 ? C_NULL : pointer(rows), m == 0 ? C_NULL : pointer(lo), m == 0 ? C_NULL : pointer(hi), m))
end
function liability_layout(h::Handle)     # (m, C): augmented records (0 without liabilities), classes (0 for censored records)
    m = Ref{Int64}(0); C = Ref{Int32}(0)
    check(h, ccall((:ngp_get_liability_layout, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}), h.ptr, m, C))
    return (Int(m[]), Int(C[]))
end
function liability_state(h::Handle)      # rows (0-based), liab (m each); thr, sum_thr, sum_thr2: t_1 .. t_{C-1} and their sums over kept draws
    m, C = liability_layout(h)
    nt = max(C - 1, 0)
    rows = Vector{Int64}(undef, m); liab = Vector{Float64}(undef, m)
    thr = Vector{Float64}(undef, nt); s1 = similar(thr); s2 = similar(thr)
    check(h, ccall((:ngp_get_liability, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32),
                   h.ptr, rows, liab, thr, s1, s2, m, C))
    return (rows = rows, liab = liab, thr = thr, sum_thr = s1, sum_thr2 = s2)
end
set_liability_state!(h::Handle, liab::Vector{Float64}, thr::Vector{Float64}, sum_thr::Vector{Float64}, sum_thr2::Vector{Float64}) =
    check(h, ccall((:ngp_set_liability_state, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32),
                   h.ptr, liab, thr, sum_thr, sum_thr2, length(liab), isempty(thr) ? 0 : length(thr) + 1))
function liability_fallthrough(h::Handle)   # truncated-normal draws whose rejection loop ran out of rounds: 0 in any sane chain
    n = Ref{Int64}(0)
    check(h, ccall((:ngp_get_liability_stats, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), h.ptr, n))
    return n[]
end
# v > 0 holds varE = v from set_y! on, 0 returns to sampling
fix_residual_variance!(h::Handle, v::Real) =
    check(h, ccall((:ngp_fix_residual_variance, LIB), Int32, (Ptr{Cvoid}, Float64), h.ptr, v))
function tnormal_indexed(h::Handle, iter::Integer, kind::Integer, index0::Integer, a::Vector{Float64}, b::Vector{Float64})   # probe of the draw layer
    out = Vector{Float64}(undef, length(a))
    check(h, ccall((:ngp_tnormal_indexed, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, UInt64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
                   h.ptr, iter, kind, index0, a, b, length(a), out))
    return out
end
"""
    getThresholds(h, nKept)

Posterior mean and SD of the thresholds `t_2 .. t_{C-1}` of an ordered trait over the kept draws (`nKept` of them).
"""
function getThresholds(h::Handle, nKept::Integer)
    st = liability_state(h)
    mean = st.sum_thr[2:end] ./ nKept
    sd = sqrt.(max.(0.0, st.sum_thr2[2:end] ./ nKept .- mean .^ 2))
    return (mean = mean, sd = sd)
end

# ---- ordered traits: Cowles' threshold step, class probabilities of held-out records (include/nextgp_hip.h, "ordered traits") ----
# mode 0: Albert-Chib (the default), 1: Cowles' joint Metropolis-Hastings move (C >= 3); sigma > 0 a fixed proposal SD, 0 adapted
# during burn-in.  After set_classes!, before set_y!.
set_threshold_step!(h::Handle, mode::Integer=1, sigma::Real=0.0) =
    check(h, ccall((:ngp_set_threshold_step, LIB), Int32, (Ptr{Cvoid}, Int32, Float64), h.ptr, mode, sigma))
function threshold_step(h::Handle)       # mode, the proposal SD in force, the proposals made and taken
    mode = Ref{Int32}(0); sigma = Ref{Float64}(0.0); tries = Ref{Int64}(0); acc = Ref{Int64}(0)
    check(h, ccall((:ngp_get_threshold_step, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Float64}, Ref{Int64}, Ref{Int64}), h.ptr, mode, sigma, tries, acc))
    return (mode = Int(mode[]), sigma = sigma[], tries = tries[], accepted = acc[])
end
set_threshold_step_state!(h::Handle, sigma::Real, tries::Integer, accepted::Integer) =
    check(h, ccall((:ngp_set_threshold_step_state, LIB), Int32, (Ptr{Cvoid}, Float64, Int64, Int64), h.ptr, sigma, tries, accepted))
# needs classes and a hold-out mask; before set_y!
enable_class_probabilities!(h::Handle, on::Bool=true) =
    check(h, ccall((:ngp_enable_class_probabilities, LIB), Int32, (Ptr{Cvoid}, Int32), h.ptr, on))
function class_probability_sums(h::Handle)   # m x C: column c the sums of P(class c) over the kept draws, rows in the order of the hold-out set
    m = Ref{Int64}(0)
    check(h, ccall((:ngp_get_holdout_layout, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), h.ptr, m))
    _, C = liability_layout(h)
    sp = Matrix{Float64}(undef, Int(m[]), C)
    check(h, ccall((:ngp_get_class_probabilities, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32), h.ptr, sp, m[], C))
    return sp
end
set_class_probability_sums!(h::Handle, sp::Matrix{Float64}) =
    check(h, ccall((:ngp_set_class_probabilities, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32), h.ptr, sp, size(sp, 1), size(sp, 2)))
"""
    getClassProbabilities(h, N)

Posterior mean of P(class) of every held-out record over the kept draws: `rows` (1-based), `n`, `prob` (records x classes).
"""
function getClassProbabilities(h::Handle, N::Integer)
    st = holdout_state(h, N)
    n = st.n_fit[st.rows .+ 1]
    keep = findall(>(0), n)
    sp = class_probability_sums(h)
    return (rows = st.rows[keep] .+ 1, n = Int.(n[keep]), prob = sp[keep, :] ./ n[keep])
end

# ---- prediction of new individuals (include/nextgp_hip.h, "prediction") ----
# A second panel beside the training panel: Np individuals x the same columns in the same order, centred with the TRAINING means.
# Every kept iteration then accumulates g = X_new beta per marker set on the device.  Column ranges as for the training panel.
begin_prediction_panel!(h::Handle, Np::Integer) =
    check(h, ccall((:ngp_begin_prediction_panel, LIB), Int32, (Ptr{Cvoid}, Int64), h.ptr, Np))
prediction_columns!(h::Handle, col0::Integer, data::Matrix{Float64}; centre::Bool=true) =
    check(h, ccall((:ngp_prediction_columns_f64, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int64, Int32),
                   h.ptr, col0, data, size(data, 2), stride(data, 2), centre))
prediction_columns!(h::Handle, col0::Integer, data::Matrix{Float32}; centre::Bool=true) =
    check(h, ccall((:ngp_prediction_columns_f32, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Float32}, Int64, Int64, Int32),
                   h.ptr, col0, data, size(data, 2), stride(data, 2), centre))
prediction_columns!(h::Handle, col0::Integer, data::Matrix{UInt8}; centre::Bool=true) =
    check(h, ccall((:ngp_prediction_columns_u8, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{UInt8}, Int64, Int64, Int32),
                   h.ptr, col0, data, size(data, 2), stride(data, 2), centre))
end_prediction_panel!(h::Handle) = check(h, ccall((:ngp_end_prediction_panel, LIB), Int32, (Ptr{Cvoid},), h.ptr))
load_prediction_file!(h::Handle, path::AbstractString; centre::Bool=true) =
    check(h, ccall((:ngp_load_prediction_file, LIB), Int32, (Ptr{Cvoid}, Cstring, Int32), h.ptr, path, centre))

function prediction_layout(h::Handle)   # Np, rows per shard, shards, columns per chunk of the normative sum, rows of the arrays (nsets + 1)
    np = Ref{Int64}(0); r = Ref{Int64}(0); s = Ref{Int64}(0); c = Ref{Int64}(0); rows = Ref{Int64}(0)
    check(h, ccall((:ngp_get_prediction_layout, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                   h.ptr, np, r, s, c, rows))
    return (Np = Int(np[]), R = Int(r[]), S = Int(s[]), chunk = Int(c[]), rows = Int(rows[]))
end

"""
    setPrediction!(h, Mpred::Dict; sets = collect(keys(Mpred)), centre = false)

The genotypes of the individuals to predict, one matrix per marker set under the keys of `M`: handed over one set after another in
the order `runSampler!` hands over `M[set].data` (pass `sets = collect(keys(M))`), never concatenated on the host.  `Mpred[s]` is
`Np x M[s].dims[2]`.  The reference's `M[set].data` is already centred (src/prepMatVec.jl:129) and the library then holds zero means,
so `Mpred[s]` must be centred by the caller with the TRAINING column means (`centre = false`, the default here); with raw codes on
both sides (`set_panel!(h, ::Matrix{UInt8})`) pass `centre = true` and the library subtracts the training means it computed.
"""
function setPrediction!(h::Handle, Mpred::Dict; sets = collect(keys(Mpred)), centre::Bool=false)
    isempty(sets) && error("setPrediction!: no marker set")
    Np = size(Mpred[sets[1]], 1)
    all(s -> size(Mpred[s], 1) == Np, sets) || error("setPrediction!: every set needs the same individuals (rows)")
    begin_prediction_panel!(h, Np)
    col0 = 0
    for s in sets
        prediction_columns!(h, col0, Mpred[s]; centre = centre)
        col0 += size(Mpred[s], 2)
    end
    end_prediction_panel!(h)
    return h
end

"""
    getPrediction(h)

Posterior mean and SD of the breeding values of the prediction panel's individuals over the kept draws: `mean` and `sd` for all
marker sets together, `set_mean` / `set_sd` (`nsets x Np`, in the order the sets were added), `nKept`, and the sums themselves
(`sum`, `sum2`: `Np x (nsets + 1)` as Julia sees the library's row-major `[nsets + 1][Np]`), which `setPrediction_sums!` restores on a
resumed chain.  `sd = sqrt(max(0, sum2 / n - mean^2))`.
"""
function getPrediction(h::Handle)
    lay = prediction_layout(h)
    lay.rows > 0 || error("getPrediction: the handle has no marker set")
    s1 = Matrix{Float64}(undef, lay.Np, lay.rows); s2 = similar(s1); n = Ref{Int64}(0)
    check(h, ccall((:ngp_get_prediction, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ref{Int64}),
                   h.ptr, s1, s2, lay.rows, lay.Np, n))
    nk = max(Int(n[]), 1)
    m = s1 ./ nk
    sd = sqrt.(max.(0.0, s2 ./ nk .- m .* m))
    return (nKept = Int(n[]), mean = m[:, end], sd = sd[:, end], set_mean = permutedims(m[:, 1:end-1]), set_sd = permutedims(sd[:, 1:end-1]),
            sum = s1, sum2 = s2)
end
setPrediction_sums!(h::Handle, s1::Matrix{Float64}, s2::Matrix{Float64}) =
    check(h, ccall((:ngp_set_prediction, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64), h.ptr, s1, s2, size(s1, 2), size(s1, 1)))
function prediction_last(h::Handle)      # g of the last kept draw, Np x (nsets + 1)
    lay = prediction_layout(h)
    out = Matrix{Float64}(undef, lay.Np, lay.rows)
    check(h, ccall((:ngp_get_prediction_last, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64), h.ptr, out, lay.rows, lay.Np))
    return out
end
function prediction_stats(h::Handle)     # launches of the prediction pass this handle made, chains they served
    a = Ref{Int64}(0); b = Ref{Int64}(0)
    check(h, ccall((:ngp_get_prediction_stats, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), h.ptr, a, b))
    return (launches = Int(a[]), chains_served = Int(b[]))
end

# ---- genomic variance of every kept draw (include/nextgp_hip.h, "genomic variance") ----
# windows::Vector{UnitRange{Int}} (1-based columns of the set) -> 0-based [start, stop)
function set_variance_windows!(h::Handle, set_id::Integer, windows)
    ws = Int64[first(w) - 1 for w in windows]
    we = Int64[last(w) for w in windows]
    check(h, ccall((:ngp_set_variance_windows, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Int64), h.ptr, set_id, ws, we, length(ws)))
end
enable_genomic_variance!(h::Handle; on::Bool=true, threshold::Float64=0.01, trace_rows::Integer=0) =
    check(h, ccall((:ngp_enable_genomic_variance, LIB), Int32, (Ptr{Cvoid}, Int32, Float64, Int64), h.ptr, on, threshold, trace_rows))
function genomic_variance_layout(h::Handle)   # slots, windows in all, marker sets, trace rows stored, draws beyond the trace's capacity
    n = Ref{Int64}(0); w = Ref{Int64}(0); s = Ref{Int64}(0); t = Ref{Int64}(0); d = Ref{Int64}(0)
    check(h, ccall((:ngp_get_genomic_variance_layout, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                   h.ptr, n, w, s, t, d))
    return (nslots = Int(n[]), nwin = Int(w[]), nsets = Int(s[]), traced = Int(t[]), dropped = Int(d[]))
end

"""
    getGenomicVariance(h)

Sums over the kept draws per slot (the windows of set 1, of set 2, ..., then one slot per set, then the total): `sumV`, `sumV2`, `sumQ`,
`sumQ2` (q = V / V_g), `count` of q > threshold, `last` (V of the last draw), `ratio = [sum r, sum r^2]` with r = V_g / (V_g + varE), and
`nKept`; with them `meanV`, `meanQ`, `sdQ` and `wppa = count / nKept`.  `setGenomicVariance_sums!` restores them on a resumed chain.
"""
function getGenomicVariance(h::Handle)
    n = genomic_variance_layout(h).nslots
    a = [Vector{Float64}(undef, n) for _ in 1:6]; ratio = Vector{Float64}(undef, 2); k = Ref{Int64}(0)
    check(h, ccall((:ngp_get_genomic_variance, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ref{Int64}),
                   h.ptr, a[1], a[2], a[3], a[4], a[5], a[6], n, ratio, k))
    nk = max(Int(k[]), 1)
    mq = a[3] ./ nk
    return (nKept = Int(k[]), sumV = a[1], sumV2 = a[2], sumQ = a[3], sumQ2 = a[4], count = a[5], last = a[6], ratio = ratio,
            meanV = a[1] ./ nk, meanQ = mq, sdQ = sqrt.(max.(0.0, a[4] ./ nk .- mq .* mq)), wppa = a[5] ./ nk)
end
setGenomicVariance_sums!(h::Handle, sumV::Vector{Float64}, sumV2::Vector{Float64}, sumQ::Vector{Float64}, sumQ2::Vector{Float64},
                         count::Vector{Float64}, last::Vector{Float64}, ratio::Vector{Float64}, nKept::Integer) =
    check(h, ccall((:ngp_set_genomic_variance, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
                   h.ptr, sumV, sumV2, sumQ, sumQ2, count, last, length(sumV), ratio, nKept))
function genomic_variance_trace(h::Handle)    # V (nslots x rows as Julia sees the library's [rows][nslots]) and r of the traced draws
    lay = genomic_variance_layout(h)
    V = Matrix{Float64}(undef, lay.nslots, lay.traced); r = Vector{Float64}(undef, lay.traced)
    check(h, ccall((:ngp_get_genomic_variance_trace, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64), h.ptr, V, r, lay.traced, lay.nslots))
    return (V = V, ratio = r)
end
function genomic_variance_stats(h::Handle)    # variance passes this handle launched, chains they served
    a = Ref{Int64}(0); b = Ref{Int64}(0)
    check(h, ccall((:ngp_get_genomic_variance_stats, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), h.ptr, a, b))
    return (launches = Int(a[]), chains_served = Int(b[]))
end

# ---- convergence diagnostics of every kept draw (include/nextgp_hip.h, "convergence diagnostics") ----
enable_diagnostics!(h::Handle; on::Bool=true, lags::Integer=64, split::Integer=0) =
    check(h, ccall((:ngp_enable_diagnostics, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Int64), h.ptr, on, lags, split))
function diagnostics_layout(h::Handle)        # monitored scalars, lags, split, draws taken, words of the state image
    D = Ref{Int64}(0); L = Ref{Int32}(0); H = Ref{Int64}(0); n = Ref{Int64}(0); w = Ref{Int64}(0)
    check(h, ccall((:ngp_get_diagnostics_layout, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                   h.ptr, D, L, H, n, w))
    return (D = Int(D[]), lags = Int(L[]), split = Int(H[]), n = Int(n[]), words = Int(w[]))
end

"""
    getDiagnostics(h)

Per monitored scalar (the doubles of a kept sample, in record order): `mean`, `var`, `sd`, `ess` (Geyer's initial positive sequence
inside the lag window), `mcse = sqrt(var / ess)`, `truncated` (1: the positive sequence had not ended inside the window, the ESS is an
upper bound), and per half of the run `half_n` (2), `half_mean`, `half_var` (D x 2): the sequences of a split-R-hat.
"""
function getDiagnostics(h::Handle)
    D = diagnostics_layout(h).D
    a = [fill(NaN, D) for _ in 1:5]; hn = zeros(2); hm = fill(NaN, D, 2); hv = fill(NaN, D, 2); n = Ref{Int64}(0)
    check(h, ccall((:ngp_get_diagnostics, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Int64}),
                   h.ptr, a[1], a[2], a[3], a[4], a[5], hn, hm, hv, D, n))
    return (n = Int(n[]), mean = a[1], var = a[2], sd = sqrt.(a[2]), ess = a[3], mcse = a[4], truncated = a[5], half_n = hn, half_mean = hm, half_var = hv)
end
function diagnostics_state(h::Handle)         # x1 | S1[2] | S2[2] | C[lags] | head[lags] | ring[lags], rows of D, and the draws taken
    w = diagnostics_layout(h).words
    st = Vector{Float64}(undef, w); n = Ref{Int64}(0)
    check(h, ccall((:ngp_get_diagnostics_state, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Int64}), h.ptr, st, w, n))
    return (state = st, n = Int(n[]))
end
set_diagnostics_state!(h::Handle, state::Vector{Float64}, n::Integer) =
    check(h, ccall((:ngp_set_diagnostics_state, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64), h.ptr, state, length(state), n))
function diagnostics_stats(h::Handle)         # updates this handle launched
    a = Ref{Int64}(0)
    check(h, ccall((:ngp_get_diagnostics_stats, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), h.ptr, a))
    return Int(a[])
end

"""
    write_diagnostics(h, outPut)

`convergence.txt` of `runSampler!(...; diagnostics = true)`, in the columns `runLMEM` of the host mirror writes: name mean sd mcse ess
rhat truncated, one line per monitored scalar in record order.  The names are `theta:<i>` (the seam does not know the *Out headers) and
rhat is NaN: a single chain is not pooled; its halves are in `getDiagnostics`.
"""
function write_diagnostics(h::Handle, outPut)
    d = getDiagnostics(h)
    open(outPut * "/convergence.txt", "w") do io
        writedlm(io, ["name" "mean" "sd" "mcse" "ess" "rhat" "truncated"])
        for i in 1:length(d.mean)
            writedlm(io, Any["theta:$(i)" d.mean[i] d.sd[i] d.mcse[i] d.ess[i] NaN Int(d.truncated[i])])
        end
    end
    return d
end

"""
    write_genomic_variance(h, outPut, sets, ids, wins)

The files of `runSampler!(...; windows = ...)`, in the reference's *Out format: `windowVar<set>Out` (header win_1 ..., one row per kept
draw) for every set with windows, `genVarOut` (one column per set, then total, then ratio), and `gwas<set>.txt` (window, first and last
SNP, mean V, mean q, SD of q, WPPA).  `sets` in the order they were added, `ids[s]` the library's set id, `wins[s]` 1-based ranges.
"""
function write_genomic_variance(h::Handle, outPut, sets, ids, wins)
    gv = getGenomicVariance(h)
    tr = genomic_variance_trace(h)
    ord = sort(collect(sets), by = s -> ids[s])          # slot order: the library's set order
    nw = [length(get(wins, s, UnitRange{Int}[])) for s in ord]
    nwin = sum(nw)
    o = 0
    for (k, s) in enumerate(ord)
        if nw[k] > 0
            open(outPut * "/windowVar$(s)Out", "w") do io
                writedlm(io, permutedims(["win_$(i)" for i in 1:nw[k]]))
                writedlm(io, permutedims(tr.V[o+1:o+nw[k], :]))
            end
            open(outPut * "/gwas$(s).txt", "w") do io
                writedlm(io, ["window" "firstSNP" "lastSNP" "meanV" "meanQ" "sdQ" "WPPA"])
                for i in 1:nw[k]
                    writedlm(io, Any[i first(wins[s][i]) last(wins[s][i]) gv.meanV[o+i] gv.meanQ[o+i] gv.sdQ[o+i] gv.wppa[o+i]])
                end
            end
        end
        o += nw[k]
    end
    open(outPut * "/genVarOut", "w") do io
        writedlm(io, permutedims(vcat(["$(s)" for s in ord], ["total", "ratio"])))
        writedlm(io, hcat(permutedims(tr.V[nwin+1:end, :]), tr.ratio))
    end
    return gv
end

# regionArray::Vector{UnitRange{Int}} (1-based, src/mme.jl:335-358) -> 0-based [start, stop)
function add_marker_set!(h::Handle, col0::Integer, ncol::Integer, method::Integer, df::Float64, scale::Float64,
                         regionArray, varBeta0::Vector{Float64}; pi0::Float64=0.0, estPi::Bool=false,
                         lhs0=C_NULL, rhs0=C_NULL)
    rs = Int64[first(r) - 1 for r in regionArray]
    re = Int64[last(r) for r in regionArray]
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_marker_set, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Int64, Int32, Float64, Float64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}, Float64, Int32,
                    Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                   h.ptr, col0, ncol, method, df, scale, rs, re, length(rs), varBeta0, pi0, estPi, lhs0, rhs0, id))
    return id[]
end

# BayesR set (src/mme.jl:374-383): ONE variance, M[s].vClass multipliers, M[s].piHat class probabilities
function add_marker_set_r!(h::Handle, col0::Integer, ncol::Integer, df::Float64, scale::Float64, varBeta0::Float64,
                           vClass::Vector{Float64}, pi::Vector{Float64}; estPi::Bool=false, lhs0=C_NULL, rhs0=C_NULL)
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_marker_set_r, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                   h.ptr, col0, ncol, df, scale, varBeta0, vClass, pi, length(vClass), estPi, lhs0, rhs0, id))
    return id[]
end

# BayesRCπ set (src/mme.jl:384-403): annot = M[s].annotInput (nSNPs x nAnnot, entries 0 / 1, no all-zero row), K classes with the
# probabilities every annotation starts from, ONE variance per annotation (all varBeta0 at first).  nAnnot <= 8, nAnnot * K <= 16.
function add_marker_set_rc!(h::Handle, col0::Integer, ncol::Integer, df::Float64, scale::Float64, varBeta0::Float64,
                            vClass::Vector{Float64}, pi::Vector{Float64}, annot::AbstractMatrix; estPi::Bool=false, lhs0=C_NULL, rhs0=C_NULL)
    an = Matrix{Int32}(annot)
    size(an, 1) == ncol || error("BayesRCπ: one annotation row per locus")
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_marker_set_rc, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Int64, Int32, Int32,
                    Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                   h.ptr, col0, ncol, df, scale, varBeta0, vClass, pi, length(vClass), an, size(an, 1), size(an, 2), estPi, lhs0, rhs0, id))
    return id[]
end

# (piHat, sum_pi: A vectors of K entries each, as the reference holds M[s].piHat (src/mme.jl:393); annotProb [ncol x A], annotCat [ncol],
# sum_annot [ncol x A]) of a BayesRCπ set
function rc_state(h::Handle, set_id::Integer, ncol::Integer, A::Integer, K::Integer)
    pi = Vector{Float64}(undef, A * K); sp = similar(pi)
    ap = Matrix{Float64}(undef, ncol, A); sa = similar(ap); cat = Vector{Int32}(undef, ncol)
    check(h, ccall((:ngp_get_rc_state, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                   h.ptr, set_id, pi, sp, ap, cat, sa))
    # the library holds pi annotation-major (slot a K + v): entry a of the reference's vector of A vectors is slots (a-1) K + 1 .. a K
    rows(x) = [x[(a - 1) * K + 1:a * K] for a in 1:A]
    return (piHat = rows(pi), sum_pi = rows(sp), annotProb = ap, annotCat = cat, sum_annot = sa)
end

# the library's copy of a BayesRCπ set's state (nothing: left as it is); piHat / sum_pi as the reference holds piHat: a vector of A
# vectors of K entries (vcat of them is the library's annotation-major order, as src/samplers.jl:86 writes them)
function set_rc_state!(h::Handle, set_id::Integer; piHat=nothing, sum_pi=nothing, annotProb=nothing, annotCat=nothing, sum_annot=nothing)
    pm(x) = x === nothing ? C_NULL : Vector{Float64}(reduce(vcat, x))
    p(x) = x === nothing ? C_NULL : Matrix{Float64}(x)
    c = annotCat === nothing ? C_NULL : Vector{Int32}(vec(annotCat))
    check(h, ccall((:ngp_set_rc_state, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                   h.ptr, set_id, pm(piHat), pm(sum_pi), p(annotProb), c, p(sum_annot)))
end

"""
    sampleBayesRCπ!(h, set_id, mSet, M, beta, delta, ycorr, varE, varBeta)

Fine seam of a BayesRCπ set: the argument list of the reference's `sampleBayesRCπ!(mSet, M, beta, delta, ycorr, varE, varBeta)`
(src/functions.jl:291) plus the handle and the set id.  The caller's `M[mSet].piHat` and `M[mSet].annotProb` go in, one call does the
sweep, the per-annotation variances, pi and the annotation probabilities; `M[mSet].piHat`, `.logPi`, `.annotProb` and `.annotCat` are
written back.  `M[mSet].annotInput` is never changed.
"""
function sampleBayesRCπ!(h::Handle, set_id::Integer, mSet, M, beta, delta, ycorr::Vector{Float64}, varE::Float64, varBeta)
    A, K = length(M[mSet].piHat), length(M[mSet].vClass)   # piHat: A vectors of K probabilities (src/mme.jl:393)
    set_rc_state!(h, set_id; piHat = M[mSet].piHat, annotProb = M[mSet].annotProb)
    b = vec(beta[M[mSet].pos]); d = vec(delta[M[mSet].pos])
    vb = varBeta[mSet] isa Vector{Float64} ? varBeta[mSet] : Float64.(varBeta[mSet])
    check(h, ccall((:ngp_sweep_set, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, set_id, varE, ycorr, b, d, vb, C_NULL))
    varBeta[mSet] isa Vector{Float64} || (varBeta[mSet] .= vb)
    st = rc_state(h, set_id, length(b), A, K)
    for a in 1:A                               # src/functions.jl:355-356
        M[mSet].piHat[a] = st.piHat[a]
        M[mSet].logPi[a] = log.(st.piHat[a])
    end
    M[mSet].annotProb .= st.annotProb
    vec(M[mSet].annotCat) .= st.annotCat       # 1 x P Matrix{Int64} (src/mme.jl:403): vec() shares the memory
    return nothing
end

# BayesLV set (src/mme.jl:418-439): one variance per locus (all varBeta0 at first), covariates = M[s].covariates (the design matrix of
# the variance formula, ncol x ncov), varZeta = M[s].varZeta[1], estVarZeta = M[s].estVarZeta (false / true / a Float64 fraction),
# zeta0 = M[s].SNPVARRESID (the reference's unseeded start) or nothing for the library's keyed start
function add_marker_set_lv!(h::Handle, col0::Integer, ncol::Integer, varBeta0::Float64, covariates::AbstractMatrix, varZeta::Float64,
                            estVarZeta; zeta0=nothing, lhs0=C_NULL, rhs0=C_NULL)
    Cm = Matrix{Float64}(covariates)
    size(Cm, 1) == ncol || error("BayesLV: one covariate row per locus")
    mode = estVarZeta === false ? 0 : (estVarZeta === true ? 1 : 2)
    frac = mode == 2 ? Float64(estVarZeta) : 0.0
    z0 = zeta0 === nothing ? C_NULL : Vector{Float64}(zeta0)
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_marker_set_lv, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Int64, Float64, Ptr{Float64}, Int64, Int32, Float64, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                   h.ptr, col0, ncol, varBeta0, Cm, size(Cm, 1), size(Cm, 2), varZeta, mode, frac, z0, lhs0, rhs0, id))
    return id[]
end

# (c, sum_c, varZeta, sum_varZeta, zeta, iCpC, trapped) of a BayesLV set
function lv_state(h::Handle, set_id::Integer, ncol::Integer, ncov::Integer)
    c = Vector{Float64}(undef, ncov); sc = similar(c); zeta = Vector{Float64}(undef, ncol); ic = Matrix{Float64}(undef, ncov, ncov)
    vz = Ref{Float64}(0.0); svz = Ref{Float64}(0.0); tr = Ref{Int64}(0)
    check(h, ccall((:ngp_get_lv_state, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
                   h.ptr, set_id, c, sc, vz, svz, zeta, ic, tr))
    return (c = c, sum_c = sc, varZeta = vz[], sum_varZeta = svz[], zeta = zeta, iCpC = ic, trapped = tr[])
end

# resume: the library's copy of a BayesLV set's state (nothing: left as it is)
function set_lv_state!(h::Handle, set_id::Integer, varZeta::Float64; c=nothing, sum_c=nothing, sum_varZeta::Float64=0.0, zeta=nothing)
    p(x) = x === nothing ? C_NULL : Vector{Float64}(x)
    check(h, ccall((:ngp_set_lv_state, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}),
                   h.ptr, set_id, p(c), p(sum_c), varZeta, sum_varZeta, p(zeta)))
end

"""
    sampleBayesLV!(h, set_id, mSet, M, beta, delta, ycorr, varE, varBeta)

Fine seam of a BayesLV set: same argument list as the reference's `sampleBayesLV!(mSet, M, beta, delta, ycorr, varE, varBeta)`
(src/functions.jl:421) plus the handle and the set id.  One call does the sweep and the variance model; `M[mSet].c`, `varZeta`, `logVar`
and `SNPVARRESID` are written back from the library, which holds them between the calls.
"""
function sampleBayesLV!(h::Handle, set_id::Integer, mSet, M, beta, delta, ycorr::Vector{Float64}, varE::Float64, varBeta)
    sweep!(h, set_id, mSet, M, beta, delta, ycorr, varE, varBeta)
    st = lv_state(h, set_id, length(varBeta[mSet]), length(M[mSet].c))
    M[mSet].c .= st.c
    M[mSet].varZeta[1] = st.varZeta
    M[mSet].logVar .= log.(varBeta[mSet])
    M[mSet].SNPVARRESID .= st.zeta
    return nothing
end

# Correlated marker sets -- sampleBayesPR!(::Tuple), src/functions.jl:140-154, set-up src/mme.jl:448-489.  M[pSet].data is a Vector of
# N x k matrices X_l (src/mme.jl:456-457); on the device the k columns of a locus sit side by side, floor(64 / k) loci per 64-column
# block from a block boundary on (include/nextgp_hip.h, ngp_add_marker_set_tuple).  tuple_panel builds that block of the panel,
# tuple_columns says where component m of locus l went (1-based panel columns), add_marker_set_tuple! declares the set:
# df = M[pSet].df (3 + k), scale = M[pSet].scale (k x k), regionArray in loci, v = varBeta[pSet][1] (k x k).
function tuple_columns(col0::Integer, nloc::Integer, k::Integer)      # col0: 0-based first panel column of the set (a multiple of 64)
    Lb = 64 ÷ k
    return [col0 + 64 * ((l - 1) ÷ Lb) + k * ((l - 1) % Lb) + m for l in 1:nloc, m in 1:k]   # 1-based panel column of (locus l, component m)
end
function tuple_panel(data::Vector{Matrix{Float64}})                   # data[l] = X_l, N x k
    nloc, (N, k) = length(data), size(data[1])
    Lb = 64 ÷ k; nblk = cld(nloc, Lb)
    out = zeros(Float64, N, 64 * nblk)                                # the set owns its blocks to the end of the last one
    cols = tuple_columns(0, nloc, k)
    for l in 1:nloc, m in 1:k
        out[:, cols[l, m]] .= data[l][:, m]
    end
    return out
end
function add_marker_set_tuple!(h::Handle, col0::Integer, nloc::Integer, k::Integer, df::Float64, scale::Matrix{Float64}, regionArray,
                               v::Matrix{Float64})
    rs = Int64[first(r) - 1 for r in regionArray]
    re = Int64[last(r) for r in regionArray]
    id = Ref{Int32}(0)
    sc = Matrix{Float64}(permutedims(scale)); vb = Matrix{Float64}(permutedims(v))   # row-major for the C side (both are symmetric)
    check(h, ccall((:ngp_add_marker_set_tuple, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Int64, Int32, Float64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}, Ref{Int32}),
                   h.ptr, col0, nloc, k, df, sc, rs, re, length(rs), vb, id))
    # a model with correlated sets takes its block chains in the inverse form (dlt = T e0: Tuple blocks 3.8 -> 3.0 us per block)
    check(h, ccall((:ngp_set_chain_form, LIB), Int32, (Ptr{Cvoid}, Int32), h.ptr, 1))
    return id[]
end

# K chains per pass over the panel: h takes owner's panel by reference (no copy); run_many! then gives all of them ONE sweep
# launch per iteration.  shards_for_pass: the max_shards the first handle needs (before its panel is set) so that K chains fit.
share_panel!(h::Handle, owner::Handle) = check(h, ccall((:ngp_share_panel, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h.ptr, owner.ptr))
function shards_for_pass(h::Handle, chains::Integer)
    v = Ref{Int32}(0)
    check(h, ccall((:ngp_shards_for_pass, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}), h.ptr, chains, v))
    return Int(v[])
end

# The warmer of the last persistent-sweep launch (ngp_get_warmer): did the last reducer workgroup warm the sampler's L2, and how many blocks.
function warmer(h::Handle)
    a = Ref{Int32}(0); b = Ref{Int64}(0)
    check(h, ccall((:ngp_get_warmer, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}), h.ptr, a, b))
    (active = Int(a[]), blocks = Int(b[]))
end

# Kept samples to a binary file while the chain runs (instead of a text row per kept iteration, src/samplers.jl:56-104): call before
# run!, close with `nothing`; nextgp.jl_amd/api.py (samples_to_out_files) or the reader below turn the file into the *Out tables.
set_sample_file!(h::Handle, path::Union{AbstractString,Nothing}) =
    check(h, path === nothing ? ccall((:ngp_set_sample_file, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}), h.ptr, C_NULL) :
                                ccall((:ngp_set_sample_file, LIB), Int32, (Ptr{Cvoid}, Cstring), h.ptr, path))
# f(sets, sample) for every record of the file, one record in memory at a time (a record is 9 bytes per locus)
function foreach_sample(f, path::AbstractString)
    open(path, "r") do io
        magic = String(read(io, 8))
        magic in ("NGPSMP01", "NGPSMP02", "NGPSMP03", "NGPSMP04", "NGPSMP05") || error("not a sample file: $path")
        P, nvb, nsets, nfix, ncls, rec = ntuple(_ -> read(io, Int64), 6)
        sets = [ntuple(_ -> read(io, Int64), 6) for _ in 1:nsets]     # (method, K, col0, ncol, variance entries, tuple k)
        rq = magic != "NGPSMP01" ? [read(io, Int64) for _ in 1:read(io, Int64)] : Int64[]   # random-effect sets: q of each (a tuple set: k - 1 in the bits from 32 up)
        # BayesLV sets ("NGPSMP03"): (marker set, ncov) of each; a record holds c (16 words, ncov used) | varZeta per set behind class_pi
        lvs = magic in ("NGPSMP03", "NGPSMP04", "NGPSMP05") ? [(read(io, Int64), read(io, Int64)) for _ in 1:read(io, Int64)] : Tuple{Int64,Int64}[]
        # BayesRCπ sets ("NGPSMP04"): (marker set, A, K) of each; a record holds annotProb [A][ncol] per set behind the BayesLV words and
        # annotCat [ncol] (one byte each) per set behind delta
        rcs = magic in ("NGPSMP04", "NGPSMP05") ? [(read(io, Int64), read(io, Int64), read(io, Int64)) for _ in 1:read(io, Int64)] : Tuple{Int64,Int64,Int64}[]
        # liability classes, C >= 3 ("NGPSMP05"): a record ends with its nthr thresholds t_2 .. t_{C-1}, behind everything read here
        nthr = magic == "NGPSMP05" ? Int(read(io, Int64)) : 0
        rcn = [Int(sets[r[1] + 1][4]) for r in rcs]                   # loci of each
        rk = [Int(w >> 32) + 1 for w in rq]                           # components of each set (1: a (1|g) / PED / GBLUP set)
        rq = [Int(w & 0xffffffff) * k for (w, k) in zip(rq, rk)]      # words of u per set: q k, the components of a level adjacent
        nr = sum(rq; init = 0) + sum(rk .^ 2; init = 0)               # u (set after set) and varU (k k words per set) between b_fixed and beta
        ncp = 3 + nfix + nr + P + nvb + 2 * nsets + ncls               # doubles in front of the BayesLV words
        nlv = ncp + 17 * length(lvs)
        nd = nlv + sum(Int(r[2]) * n for (r, n) in zip(rcs, rcn); init = 0)
        raw = Vector{UInt8}(undef, rec)
        while !eof(io)
            readbytes!(io, raw, rec) == rec || break
            d = reinterpret(Float64, view(raw, 1:8 * nd))
            ro = 3 + nfix
            u = [d[ro + sum(rq[1:r-1]; init = 0) + 1:ro + sum(rq[1:r]; init = 0)] for r in eachindex(rq)]
            varU = d[ro + sum(rq; init = 0) + 1:ro + nr]
            o = 3 + nr
            f(sets, (iter = reinterpret(Int64, view(raw, 1:8))[1], varE = d[2], b = d[3], b_fixed = d[4:3 + nfix], u = u, varU = varU,
                     beta = d[o + nfix + 1:o + nfix + P], varBeta = d[o + nfix + P + 1:o + nfix + P + nvb],
                     piHat = d[o + nfix + P + nvb + 1:o + nfix + P + nvb + 2 * nsets],
                     class_pi = d[o + nfix + P + nvb + 2 * nsets + 1:ncp],
                     lv_c = [d[ncp + 17 * (i - 1) + 1:ncp + 17 * (i - 1) + lvs[i][2]] for i in eachindex(lvs)],
                     lv_varZeta = [d[ncp + 17 * i] for i in eachindex(lvs)], delta = raw[8 * nd + 1:8 * nd + P],
                     annotProb = [reshape(d[nlv + sum(Int(rcs[j][2]) * rcn[j] for j in 1:i-1; init = 0) + 1:nlv + sum(Int(rcs[j][2]) * rcn[j] for j in 1:i; init = 0)], rcn[i], Int(rcs[i][2])) for i in eachindex(rcs)],   # ncol x A
                     annotCat = [raw[8 * nd + P + sum(rcn[1:i-1]; init = 0) + 1:8 * nd + P + sum(rcn[1:i]; init = 0)] for i in eachindex(rcs)]))
        end
    end
end
function read_sample_file(path::AbstractString)
    samples = NamedTuple[]; sets = nothing
    foreach_sample(path) do st, smp
        sets = st; push!(samples, smp)
    end
    return (sets = sets, samples = samples)
end

# A fixed-effect set given as a sparse matrix (ngp_add_fixed_set_sparse): a factor of thousands of levels, or a block of crossed
# factors and covariates, N x ncol with 2 <= ncol <= 2^20.  A SparseMatrixCSC is the ABI's layout (rows ascending inside a column)
# with 1-based offsets; stored zeros are dropped first.  Bit for bit the dense set of the same design wherever both exist.
function add_fixed_set_sparse!(h::Handle, X::SparseMatrixCSC)
    Xs = dropzeros(X)
    cp = Int64.(Xs.colptr .- 1); rw = Int32.(Xs.rowval .- 1); vl = Float64.(Xs.nzval)
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_fixed_set_sparse, LIB), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ref{Int32}),
                   h.ptr, size(Xs, 1), size(Xs, 2), cp, rw, vl, id))
    return id[]
end

# (1|g) random-effect set (ngp_add_random_set): level[i] in 0..q-1 per record, K = Z.iVarStr (any AbstractMatrix) sent as CSR
function add_random_set!(h::Handle, level::Vector{Int32}, q::Integer, K, df::Float64, scale::Float64, varU0::Float64)
    kp = Vector{Int64}(undef, q + 1); kc = Int32[]; kv = Float64[]
    kp[1] = 0
    for l in 1:q                                 # row l of K, columns ascending (K is symmetric: row l == column l)
        col = K[:, l]
        for c in 1:q
            col[c] == 0.0 && continue
            push!(kc, c - 1); push!(kv, Float64(col[c]))
        end
        kp[l + 1] = length(kc)
    end
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_random_set, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Float64, Float64, Float64, Ref{Int32}),
                   h.ptr, level, q, kp, kc, kv, df, scale, varU0, id))
    return id[]
end
# The Gauss-Seidel engine of a CSR set with off-diagonal K, e.g. a PED set's Ainv (ngp_set_random_schedule): 0 automatic, 1 serial,
# 2 level-scheduled (rows of equal depth side by side).  The bits do not depend on it.  random_schedule: (engine in force, depths, launches).
set_random_schedule!(h::Handle, set_id::Integer, mode::Integer) =
    check(h, ccall((:ngp_set_random_schedule, LIB), Int32, (Ptr{Cvoid}, Int32, Int32), h.ptr, set_id, mode))
function random_schedule(h::Handle, set_id::Integer)
    e = Ref{Int32}(0); d = Ref{Int64}(0); n = Ref{Int64}(0)
    check(h, ccall((:ngp_get_random_schedule, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int64}, Ref{Int64}), h.ptr, set_id, e, d, n))
    (engine = Int(e[]), depths = Int(d[]), launches = Int(n[]))
end
# A^-1 of a pedigree on the host (ngp_pedigree_ainv: Henderson's rules with inbreeding): sire / dam are 1-based positions in a list with
# parents in front of their offspring, 0 = unknown.  Returns (F, k_ptr, k_col, k_val): CSR with 0-based columns, ascending within a row.
function pedigree_ainv(sire::Vector{Int32}, dam::Vector{Int32})
    n = length(sire)
    length(dam) == n || error("pedigree: one sire and one dam per animal")
    F = Vector{Float64}(undef, n); kp = Vector{Int64}(undef, n + 1); nnz = Ref{Int64}(0)
    ccall((:ngp_pedigree_ainv, LIB), Int32, (Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Int64, Ref{Int64}),
          n, sire, dam, F, kp, C_NULL, C_NULL, 0, nnz)                      # counts: refused for the cap, nnz set
    nnz[] > 0 || error("ngp_pedigree_ainv: " * unsafe_string(ccall((:ngp_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    kc = Vector{Int32}(undef, nnz[]); kv = Vector{Float64}(undef, nnz[])
    rc = ccall((:ngp_pedigree_ainv, LIB), Int32, (Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Int64, Ref{Int64}),
               n, sire, dam, F, kp, kc, kv, nnz[], nnz)
    rc == 0 || error("ngp_pedigree_ainv: " * unsafe_string(ccall((:ngp_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    (F, kp, kc, kv)
end
# A random-effect set over a DENSE q x q precision (ngp_add_random_set_dense): GBLUP's Z[z].iVarStr = inv(makeG(M)), which the shim's
# caller has built already (src/prepMatVec.jl:122-126).  level === nothing: the identity incidence (record i is level i).  K is copied to
# the device as it is (symmetric: row- and column-major are the same matrix) and sampled by the blocked engine, K read once per iteration.
function add_random_set_dense!(h::Handle, level::Union{Nothing,Vector{Int32}}, q::Integer, K::Matrix{Float64}, df::Float64, scale::Float64,
                               varU0::Float64)
    size(K) == (q, q) || error("dense random-effect set: K must be $q x $q")
    id = Ref{Int32}(0)
    lv = level === nothing ? Ptr{Int32}(C_NULL) : pointer(level)
    GC.@preserve level check(h, ccall((:ngp_add_random_set_dense, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Float64}, Ptr{Cvoid}, Int32, Float64, Float64, Float64, Ref{Int32}),
                   h.ptr, lv, q, K, C_NULL, 0, df, scale, varU0, id))
    return id[]
end
# a model without marker sets (GBLUP terms only): N records in place of the panel
const RECORDS_ONLY_P = 64   # columns of the inert block such a handle reports as its P (state and file formats)
set_records!(h::Handle, N::Integer) = check(h, ccall((:ngp_set_records, LIB), Int32, (Ptr{Cvoid}, Int64), h.ptr, N))

# VanRaden's G on the device (drop-in for misc.makeG, src/misc.jl:145-160; M is NOT centred in place): fp64 on the matrix cores
grm_begin!(h::Handle, N::Integer, method::Integer) = check(h, ccall((:ngp_grm_begin, LIB), Int32, (Ptr{Cvoid}, Int64, Int32), h.ptr, N, method))
grm_columns!(h::Handle, M::Matrix{Float64}) =
    check(h, ccall((:ngp_grm_columns_f64, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64), h.ptr, M, size(M, 2), size(M, 1)))
grm_columns!(h::Handle, M::Matrix{Float32}) =
    check(h, ccall((:ngp_grm_columns_f32, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64), h.ptr, M, size(M, 2), size(M, 1)))
grm_columns!(h::Handle, M::Matrix{UInt8}) =
    check(h, ccall((:ngp_grm_columns_u8, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Int64, Int64), h.ptr, M, size(M, 2), size(M, 1)))
grm_end!(h::Handle) = check(h, ccall((:ngp_grm_end, LIB), Int32, (Ptr{Cvoid},), h.ptr))
grm_invert!(h::Handle) = check(h, ccall((:ngp_grm_invert, LIB), Int32, (Ptr{Cvoid},), h.ptr))
function grm_get(h::Handle, N::Integer)
    G = Matrix{Float64}(undef, N, N)
    check(h, ccall((:ngp_grm_get, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, G))
    return G
end
# ---- single-step GBLUP (include/nextgp_hip.h): H^-1 = A^-1 + [0 0; 0 inv((1 - w) G + w A22) - inv(A22)].  The reference has no single-step
# model, so nothing of the coarse seam routes here: these are direct bindings for a caller that builds the model itself. ----
# A22 = A[idx, idx] without the dense A (ngp_pedigree_a22: Colleau's indirect method on the host); F from pedigree_ainv, idx 0-based
function pedigree_a22(sire::Vector{Int32}, dam::Vector{Int32}, F::Vector{Float64}, idx::Vector{Int64})
    n = length(sire); m = length(idx)
    (length(dam) == n && length(F) == n && m >= 1) || error("pedigree_a22: one sire, dam and F per animal, and at least one listed animal")
    A22 = Matrix{Float64}(undef, m, m)
    rc = ccall((:ngp_pedigree_a22, LIB), Int32, (Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Int64),
               n, sire, dam, F, idx, m, A22, m)
    rc == 0 || error("ngp_pedigree_a22: " * unsafe_string(ccall((:ngp_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return A22
end
# after grm_end!, in place of grm_invert!: the handle's matrix becomes the corner block D (grm_get returns it)
function grm_single_step!(h::Handle, A22::Matrix{Float64}, w::Float64)
    size(A22, 1) == size(A22, 2) || error("single-step: A22 must be square")
    check(h, ccall((:ngp_grm_single_step, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Float64), h.ptr, A22, size(A22, 1), w))
end
# K = S + embed(D): S as CSR with 0-based ascending columns (pedigree_ainv's layout, renumbered so that the genotyped animals are the
# LAST nd levels); D === nothing takes over the handle's own corner block (grm_single_step!), a matrix is copied to the device
function add_random_set_hybrid!(h::Handle, level::Vector{Int32}, q::Integer, kp::Vector{Int64}, kc::Vector{Int32}, kv::Vector{Float64}, nd::Integer,
                                D::Union{Nothing,Matrix{Float64}}, df::Float64, scale::Float64, varU0::Float64)
    length(kp) == q + 1 || error("hybrid random-effect set: k_ptr needs q + 1 entries")
    (D === nothing || size(D) == (nd, nd)) || error("hybrid random-effect set: D must be $nd x $nd")
    id = Ref{Int32}(0)
    dp = D === nothing ? Ptr{Float64}(C_NULL) : pointer(D)
    GC.@preserve D check(h, ccall((:ngp_add_random_set_hybrid, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Cvoid}, Int32, Float64, Float64, Float64, Ref{Int32}),
                   h.ptr, level, q, kp, kc, kv, nd, dp, C_NULL, 0, df, scale, varU0, id))
    return id[]
end

function makeG(M::Matrix; method::Integer=1, device::Integer=0, inverse::Bool=false)
    h = Handle(device=device)
    grm_begin!(h, size(M, 1), method); grm_columns!(h, M); grm_end!(h)
    inverse && grm_invert!(h)                     # inv(makeG(M)) of src/prepMatVec.jl:124 without leaving the device
    return grm_get(h, size(M, 1))
end

# the level of every record from the one-hot incidence Z.data (src/prepMatVec.jl:143-150); rows that are not one-hot are refused
function random_levels(Zd::AbstractMatrix)
    lv = Vector{Int32}(undef, size(Zd, 1))
    for i in 1:size(Zd, 1)
        r = findall(!iszero, Zd[i, :])
        (length(r) == 1 && Zd[i, r[1]] == 1) || error("random effect: row $i of Z is not one-hot (random slopes stay on the reference path)")
        lv[i] = r[1] - 1
    end
    return lv
end
function random_state(h::Handle, set_id::Integer, q::Integer)
    u = Vector{Float64}(undef, q); su = similar(u); v = Ref{Float64}(0.0); sv = Ref{Float64}(0.0)
    check(h, ccall((:ngp_get_random, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}), h.ptr, set_id, u, su, v, sv))
    return (u = u, sum_u = su, varU = v[], sum_varU = sv[])
end
set_random!(h::Handle, set_id::Integer, u::Vector{Float64}, sum_u::Vector{Float64}, varU::Float64, sum_varU::Float64) =
    check(h, ccall((:ngp_set_random, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Float64, Float64), h.ptr, set_id, u, sum_u, varU, sum_varU))

# Correlated (Tuple) random-effect sets, (:ID, :Dam) (ngp_add_random_set_tuple): levels is N x k (1-based, 0 = the record has no level in
# that component: an all-zero row of that Z), K the shared Z.iVarStr, scale and varU0 k x k.  The state is held as the reference holds
# it: u k x q (Julia's column-major k x q IS the library's q x k with the components of a level adjacent), varU k x k (symmetric).
# THE STEP DRAWS THE EXACT GIBBS CONDITIONAL, not the reference's lines (include/nextgp_hip.h): use these wrappers knowingly; the coarse
# seam (runLMEM_hip) keeps sending Tuple Z sets to the reference sampler.
function add_random_set_tuple!(h::Handle, levels::Matrix{Int32}, q::Integer, K, df::Float64, scale::Matrix{Float64}, varU0::Matrix{Float64})
    k = size(levels, 2)
    (size(scale) == (k, k) && size(varU0) == (k, k)) || error("tuple random-effect set: scale and varU0 must be $k x $k")
    kp = Vector{Int64}(undef, q + 1); kc = Int32[]; kv = Float64[]
    kp[1] = 0
    for l in 1:q                                 # row l of K, columns ascending (K is symmetric: row l == column l)
        col = K[:, l]
        for c in 1:q
            col[c] == 0.0 && continue
            push!(kc, c - 1); push!(kv, Float64(col[c]))
        end
        kp[l + 1] = length(kc)
    end
    lv = vec(levels) .- Int32(1)                 # component-major k x N, 0-based, -1 = no level
    id = Ref{Int32}(0)
    check(h, ccall((:ngp_add_random_set_tuple, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Int32}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                   h.ptr, lv, k, q, kp, kc, kv, df, Matrix(scale'), Matrix(varU0'), id))
    return id[]
end
function random_state_tuple(h::Handle, set_id::Integer, q::Integer, k::Integer)
    u = Matrix{Float64}(undef, k, q); su = similar(u); v = Matrix{Float64}(undef, k, k); sv = similar(v)
    check(h, ccall((:ngp_get_random_tuple, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, set_id, u, su, v, sv))
    return (u = u, sum_u = su, varU = Matrix(v'), sum_varU = Matrix(sv'))
end
set_random_tuple!(h::Handle, set_id::Integer, u::Matrix{Float64}, sum_u::Matrix{Float64}, varU::Matrix{Float64}, sum_varU::Matrix{Float64}) =
    check(h, ccall((:ngp_set_random_tuple, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, set_id, u, sum_u, Matrix(varU'), Matrix(sum_varU')))
# fine seam of a tuple set: the argument list of functions.sampleZ!(zSet::Tuple, Z, u, ycorr, varE, varU) plus the handle and the set id
function sampleZ_tuple!(h::Handle, set_id::Integer, zSet::Tuple, Z, u, ycorr::Vector{Float64}, varE::Float64, varU)
    uv = u[Z[zSet].pos]                          # k x q Matrix{Float64}, updated in place
    v = Matrix{Float64}(Matrix(varU[zSet])')
    check(h, ccall((:ngp_sample_random_set_tuple, LIB), Int32, (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, set_id, varE, ycorr, uv, v))
    varU[zSet] = Matrix(v')
    return nothing
end

"""
    sampleZ!(h, set_id, zSet, Z, u, ycorr, varE, varU)

Fine seam of one (1|g) set: same argument list as the reference's `functions.sampleZ!(zSet, Z, u, ycorr, varE, varU)`
(src/functions.jl:92-97) plus the handle and the set id (from `add_random_set!`).  Mutates `u[Z[zSet].pos]`, `ycorr` and `varU[zSet]`.
"""
function sampleZ!(h::Handle, set_id::Integer, zSet, Z, u, ycorr::Vector{Float64}, varE::Float64, varU)
    uv = vec(u[Z[zSet].pos])                     # 1 x q Matrix{Float64}: vec() shares the memory
    v = Ref{Float64}(Float64(varU[zSet]))
    check(h, ccall((:ngp_sample_random_set, LIB), Int32, (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                   h.ptr, set_id, varE, ycorr, uv, v))
    varU[zSet] = v[]
    return nothing
end

function class_state(h::Handle, set_id::Integer)
    pi = zeros(16); sp = zeros(16); K = Ref{Int64}(0)
    check(h, ccall((:ngp_get_class_state, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int64}), h.ptr, set_id, pi, sp, K))
    return pi[1:K[]], sp[1:K[]]
end

# resume: chain state + posterior sums + stream identity in one file (the role of the append-only *Out files, src/outFiles.jl:17-21)
save_snapshot(h::Handle, path::AbstractString) = check(h, ccall((:ngp_save_snapshot, LIB), Int32, (Ptr{Cvoid}, Cstring), h.ptr, path))
load_snapshot!(h::Handle, path::AbstractString) = check(h, ccall((:ngp_load_snapshot, LIB), Int32, (Ptr{Cvoid}, Cstring), h.ptr, path))

# pooled posterior sums of several chains (one Handle per chain / device): ONE RCCL all-reduce inside the library
# niter iterations of every chain at once, one host thread per handle inside the library (chains sharing a device run side by side
# when their grids fit it together -- set_max_shards! -- and in turns otherwise)
function run_many!(hs::Vector{Handle}, niter::Integer)
    ptrs = [h.ptr for h in hs]
    rc = ccall((:ngp_run_many, LIB), Int32, (Ptr{Ptr{Cvoid}}, Int32, Int64), ptrs, length(ptrs), niter)
    rc == 0 || error("ngp_run_many ($rc): " * join((unsafe_string(ccall((:ngp_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)) for h in hs), " | "))
end

function allreduce_posterior!(hs::Vector{Handle})
    ptrs = Ptr{Cvoid}[x.ptr for x in hs]
    check(hs[1], ccall((:ngp_allreduce_posterior, LIB), Int32, (Ptr{Ptr{Cvoid}}, Int32), ptrs, length(ptrs)))
end

set_y!(h::Handle, y::Vector{Float64}) = check(h, ccall((:ngp_set_y, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64), h.ptr, y, length(y)))
set_residual_prior!(h::Handle, df, scale) = check(h, ccall((:ngp_set_residual_prior, LIB), Int32, (Ptr{Cvoid}, Float64, Float64), h.ptr, df, scale))
# weighted residuals, E.str == "D" (src/mme.jl:71-75): w = E.iVarStr (w_i = 1 / d_ii), BEFORE the panel -- its rows are scaled at upload
set_residual_weights!(h::Handle, w::Vector{Float64}) =
    check(h, ccall((:ngp_set_residual_weights, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64), h.ptr, w, length(w)))
function residual_weights(h::Handle, N::Integer)      # the weights in force (nothing: none set)
    w = zeros(Float64, N)
    rc = ccall((:ngp_get_residual_weights, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64), h.ptr, w, N)
    rc == -2 && return nothing
    check(h, rc)
    return w
end
set_schedule!(h::Handle, n, burn, thin) = check(h, ccall((:ngp_set_schedule, LIB), Int32, (Ptr{Cvoid}, Int64, Int64, Int64), h.ptr, n, burn, thin))
run!(h::Handle, niter) = check(h, ccall((:ngp_run, LIB), Int32, (Ptr{Cvoid}, Int64), h.ptr, niter))

"""
    sweep!(h, set_id, mSet, M, beta, delta, ycorr, varE, varBeta)

Fine seam: same argument list as the reference's `sampleBayesPR!/sampleBayesB!/sampleBayesC!(mSet, M, beta, delta, ycorr,
varE, varBeta)` (src/functions.jl:118,157,197) plus the handle and the set id.  Mutates `beta[M[mSet].pos]`, `delta[M[mSet].pos]`, `ycorr`,
`varBeta[mSet]` and, for BayesB / BayesC, `M[mSet].piHat` / `M[mSet].logPi` in place.
"""
function sweep!(h::Handle, set_id::Integer, mSet, M, beta, delta, ycorr::Vector{Float64}, varE::Float64, varBeta)
    b = vec(beta[M[mSet].pos])                 # 1 x P Matrix{Float64}: vec() shares the memory
    d = vec(delta[M[mSet].pos])                # 1 x P Matrix{Int64}
    vb = varBeta[mSet] isa Vector{Float64} ? varBeta[mSet] : Float64.(varBeta[mSet])
    isR = M[mSet].method == "BayesR"          # K class probabilities (1 x K piHat, src/mme.jl:374-383): read through ngp_get_class_state
    pih = (haskey(M[mSet], :piHat) && !isR) ? vec(M[mSet].piHat) : Float64[0.0, 0.0]
    check(h, ccall((:ngp_sweep_set, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, set_id, varE, ycorr, b, d, vb, pih))
    varBeta[mSet] isa Vector{Float64} || (varBeta[mSet] .= vb)
    if haskey(M[mSet], :piHat)
        if isR
            M[mSet].piHat .= reshape(class_state(h, set_id)[1], size(M[mSet].piHat))   # src/functions.jl:284-288
        else
            M[mSet].piHat .= reshape(pih, size(M[mSet].piHat))
        end
        M[mSet].logPi .= log.(M[mSet].piHat)  # src/functions.jl:193, :289
    end
    return nothing
end

"""
    sweep_dev!(h, set_id, varE, d_ycorr, d_beta, d_delta, d_varBeta, d_piHat = C_NULL)

The fine seam for a host that keeps its state on the GPU (`ROCArray`s of AMDGPU.jl: pass `pointer(a)` converted to `Ptr{Cvoid}`):
`ycorr` (N), the set's `beta` (ncol) and `varBeta` (regions) as Float64, `delta` (ncol) as Int64 or `C_NULL`, `piHat` (2, BayesB /
BayesC) -- all in device memory of the handle's device, updated in place by device-to-device copies (`ngp_sweep_set_dev`).
"""
function sweep_dev!(h::Handle, set_id::Integer, varE::Float64, d_ycorr::Ptr{Cvoid}, d_beta::Ptr{Cvoid}, d_delta::Ptr{Cvoid},
                    d_varBeta::Ptr{Cvoid}, d_piHat::Ptr{Cvoid} = C_NULL)
    check(h, ccall((:ngp_sweep_set_dev, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, set_id, varE, d_ycorr, d_beta, d_delta, d_varBeta, d_piHat))
    return nothing
end

"""
    runSampler!(ycorr, nData, E, X, b, Z, u, varU, M, beta, varBeta, delta, chainLength, burnIn, outputFreq, outPut; seed=1)

Coarse seam: drop-in for `samplers.runSampler!` (src/samplers.jl:23) for models made of fixed effects (intercept, covariates,
factors, blocked groups), Symbol / Expr random effects -- (1|g) terms and PED sets, whose Ainv the reference has built -- and Symbol marker
sets with BayesPR / BayesB / BayesC / BayesR / BayesRCπ / BayesLV priors.  Anything else -- "BayesRCplus" among the methods -- falls back
to the reference sampler.
"""
function runSampler!(ycorr, nData, E, X, b, Z, u, varU, M, beta, varBeta, delta, chainLength, burnIn, outputFreq, outPut;
                     seed::Integer=1, device::Integer=0, windows::Dict=Dict(), windowThreshold::Float64=0.01, genomicVariance::Bool=false,
                     holdout::Vector{Int}=Int[], diagnostics::Union{Bool,Integer}=false)
    all(z -> z isa Union{Symbol,Expr}, keys(Z)) || error("correlated (Tuple) random effects: use the reference sampler (src/functions.jl:75-89, 100-110); the device draws the exact Gibbs conditional of the model, NOT the reference's lines (they leave Z_ID'Z_Dam u_Dam of the other levels in a level's right-hand side), so a run sent there would not be the reference's chain -- add_random_set_tuple! / sampleZ_tuple! are there for callers who want the exact one")
    (E.str == "I" || E.str == "D") || error("residual structure $(E.str): only \"I\" and \"D\" exist (src/mme.jl:63-79)")
    any(s -> M[s].method == "BayesRCplus", keys(M)) && error("BayesRCplus: use the reference sampler (one step per annotation on the same column, src/functions.jl:362-419: not on the device)")
    h = Handle(device=device, seed=seed)
    E.str == "D" && set_residual_weights!(h, Vector{Float64}(E.iVarStr))   # before the panel (src/mme.jl:71-75)
    sets = collect(keys(M))                       # Dict order, as src/samplers.jl:50
    if isempty(sets)                              # GBLUP terms only (src/prepMatVec.jl:122-126): records, no genotype panel
        set_records!(h, nData)
    else
    # consecutive column ranges of ONE panel on the device, handed over set by set (no hcat of the M[s].data on the host)
    begin_panel!(h, size(M[sets[1]].data, 1), sum(M[s].dims[2] for s in sets))
    col0 = 0
    for s in sets
        panel_columns!(h, col0, M[s].data)       # already centred (src/prepMatVec.jl:129)
        col0 += M[s].dims[2]
    end
    end_panel!(h)
    end
    col0 = 0
    ids = Dict{Any,Int32}()
    for s in sets
        P = M[s].dims[2]
        method = M[s].method == "BayesB" ? 1 : (M[s].method == "BayesC" ? 2 : (M[s].method == "BayesR" ? 3 : 0))
        if M[s].method == "BayesLV"   # covariates, varZeta, estVarZeta and the reference's starting zeta (src/mme.jl:418-439)
            ids[s] = add_marker_set_lv!(h, col0, P, Float64(varBeta[s][1]), M[s].covariates, Float64(M[s].varZeta[1]), M[s].estVarZeta;
                                        zeta0 = M[s].SNPVARRESID, lhs0 = Float64.(M[s].lhs), rhs0 = Float64.(M[s].rhs))
        elseif M[s].method == "BayesRCπ"   # per annotation a variance and a row of pi; the annotations as given (src/mme.jl:384-403)
            ids[s] = add_marker_set_rc!(h, col0, P, Float64(M[s].df), Float64(M[s].scale), Float64(varBeta[s][1]), Float64.(vec(M[s].vClass)),
                                        Float64.(M[s].piHat[1]), M[s].annotInput; estPi = M[s].estPi, lhs0 = Float64.(M[s].lhs),
                                        rhs0 = Float64.(M[s].rhs))
        elseif method == 3   # ONE variance, class multipliers and class probabilities (src/mme.jl:374-383)
            ids[s] = add_marker_set_r!(h, col0, P, Float64(M[s].df), Float64(M[s].scale), Float64(varBeta[s][1]), Float64.(vec(M[s].vClass)),
                                       Float64.(vec(M[s].piHat)); estPi = M[s].estPi, lhs0 = Float64.(M[s].lhs), rhs0 = Float64.(M[s].rhs))
        else
            # BayesC loops over one-locus ranges but has ONE variance (nVarCov = 1, src/mme.jl:370): a single region for the library
            regions = method == 2 ? [1:P] : M[s].regionArray
            ids[s] = add_marker_set!(h, col0, P, method, Float64(M[s].df), Float64(M[s].scale), regions,
                                     Float64.(varBeta[s]); pi0 = method >= 1 ? M[s].piHat[2] : 0.0,
                                     estPi = method >= 1 ? M[s].estPi : false, lhs0 = Float64.(M[s].lhs), rhs0 = Float64.(M[s].rhs))
        end
        col0 += P
    end
    # fixed effects: EVERY set of X (the intercept's column of ones included) becomes a fixed-effect set of the library, in the
    # order of keys(X) -- exactly the order src/samplers.jl:39-41 samples them in; the library's own intercept is switched off
    xsets = collect(keys(X))
    for x in xsets
        Xd = Matrix{Float64}(reshape(X[x].data, :, X[x].nCol))
        if X[x].nCol > 64   # wider than a dense set of the library: the same chain through the sparse entry point
            add_fixed_set_sparse!(h, SparseArrays.sparse(Xd))
            continue
        end
        check(h, ccall((:ngp_add_fixed_set, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                       h.ptr, Xd, size(Xd, 1), size(Xd, 2), size(Xd, 1), Float64.(X[x].lhs), Float64.(X[x].rhs), Ref{Int32}(0)))
    end
    nfix = isempty(xsets) ? 0 : sum(X[x].nCol for x in xsets)
    # random effects, after the fixed effects in the order of keys(Z) (src/samplers.jl:43-46): the level of every row from Z.data,
    # K = Z.iVarStr (I, Ainv or inv(str), src/mme.jl:26-37), df / scale / varU as the reference set them up (src/mme.jl:255-272)
    zsets = collect(keys(Z))
    zids = Dict{Any,Int32}()
    for z in zsets
        q = size(Z[z].data, 2)
        if Z[z].method == "GBLUP"                 # dense iVarStr = inv(G), Z = I (src/prepMatVec.jl:124-126): the blocked dense engine
            zids[z] = add_random_set_dense!(h, nothing, q, Matrix{Float64}(Z[z].iVarStr), Float64(Z[z].df), Float64(Z[z].scale), Float64(varU[z]))
        else                                      # every other Z set keeps the CSR call it had: no existing model changes its bits
            zids[z] = add_random_set!(h, random_levels(Z[z].data), q, Z[z].iVarStr, Float64(Z[z].df), Float64(Z[z].scale), Float64(varU[z]))
        end
    end
    # held-out records (1-BASED rows, as Julia counts): their entries of ycorr are not read and may be NaN / missing-coded
    isempty(holdout) || set_holdout!(h, Vector{Int64}(sort(holdout) .- 1))
    set_y!(h, Vector{Float64}(ycorr))            # ycorr == y at this point (src/mme.jl:57)
    set_residual_prior!(h, E.df, E.scale)
    check(h, ccall((:ngp_set_intercept, LIB), Int32, (Ptr{Cvoid}, Int32), h.ptr, 0))
    set_schedule!(h, chainLength, burnIn, outputFreq)
    # genomic variance of every kept draw (windows = Dict(set => W | Vector{UnitRange}), or genomicVariance = true for the set and total
    # slots alone): switched on behind set_y!, one trace row per kept draw; the files are written after the run
    gvar = genomicVariance || !isempty(windows)
    gvwins = Dict{Any,Vector{UnitRange{Int}}}()
    if gvar
        E.str == "I" || error("genomic variance: residual structure \"D\" scales the rows of the tiles (ngp_enable_genomic_variance refuses it)")
        for (s, w) in windows
            haskey(ids, s) || error("windows for an unknown set $(s): the marker sets are $(sets)")
            P = M[s].dims[2]
            gvwins[s] = w isa Integer ? [a:min(a + w - 1, P) for a in 1:w:P] : collect(UnitRange{Int}, w)
            set_variance_windows!(h, ids[s], gvwins[s])
        end
        enable_genomic_variance!(h; threshold = windowThreshold, trace_rows = max(0, div(chainLength - burnIn, outputFreq)))
    end
    # convergence diagnostics (diagnostics = true: a window of 64 lags, or the number of lags): switched on behind set_y!, the halves of
    # the split part at the middle of the planned kept draws; convergence.txt is written after the run
    dlags = diagnostics === true ? 64 : (diagnostics === false ? 0 : Int(diagnostics))
    dlags > 0 && enable_diagnostics!(h; lags = dlags, split = div(max(0, div(chainLength - burnIn, outputFreq)), 2))
    # ONE call for the whole chain: the kept samples (these2Keep, src/samplers.jl:26) go to a binary file through a copy stream and
    # a writer thread of the library while the chain runs -- the device never stops for a sample
    smpfile = joinpath(outPut, "samples.ngp")
    set_sample_file!(h, smpfile)
    run!(h, chainLength)
    set_sample_file!(h, nothing)                 # flushes and closes
    # ... and become the rows of the reference's *Out files afterwards, one record in memory at a time
    lvsets = [s for s in sets if M[s].method == "BayesLV"]                  # in the order the library numbers them
    rcsets = [s for s in sets if M[s].method == "BayesRCπ"]
    foreach_sample(smpfile) do sinfo, smp
        open(io -> writedlm(io, smp.b_fixed'), outPut * "/bOut", "a")       # src/samplers.jl:57
        open(io -> writedlm(io, smp.varE), outPut * "/varEOut", "a")        # src/samplers.jl:58
        for (r, z) in enumerate(zsets)                                      # src/samplers.jl:60-75
            open(io -> writedlm(io, smp.u[r]'), outPut * "/u$(z)Out", "a")
            open(io -> writedlm(io, smp.varU[r:r]'), outPut * "/varU$(z)Out", "a")
        end
        c0 = 0; v0 = 0; k0 = 0
        for (k, s) in enumerate(sets)
            P = M[s].dims[2]
            open(io -> writedlm(io, smp.beta[c0+1:c0+P]'), outPut * "/beta$(s)Out", "a")          # :80
            open(io -> writedlm(io, Int.(smp.delta[c0+1:c0+P])'), outPut * "/delta$(s)Out", "a")  # :81
            M[s].method in ("BayesB", "BayesC") && open(io -> writedlm(io, smp.piHat[2k-1:2k]'), outPut * "/pi$(s)Out", "a")   # :80-82
            if M[s].method == "BayesR"                                                              # one column per class
                K = Int(sinfo[k][2])
                open(io -> writedlm(io, smp.class_pi[k0+1:k0+K]'), outPut * "/pi$(s)Out", "a")
                k0 += K
            end
            if M[s].method == "BayesRCπ"                                                            # :85-87; pi annotation-major
                K = Int(sinfo[k][2])
                open(io -> writedlm(io, smp.class_pi[k0+1:k0+K]'), outPut * "/pi$(s)Out", "a")
                open(io -> writedlm(io, Int.(smp.annotCat[findfirst(==(s), rcsets)])'), outPut * "/annot$(s)Out", "a")
                k0 += K
            end
            if M[s].method == "BayesLV"                                                             # :89-92
                i = findfirst(==(s), lvsets)
                open(io -> writedlm(io, smp.lv_c[i]'), outPut * "/c$(s)Out", "a")
                open(io -> writedlm(io, smp.lv_varZeta[i:i]'), outPut * "/varZeta$(s)Out", "a")
            end
            nr = length(varBeta[s])
            open(io -> writedlm(io, smp.varBeta[v0+1:v0+nr]'), outPut * "/var$(s)Out", "a")       # :101-103
            c0 += P; v0 += nr
        end
    end
    gvar && write_genomic_variance(h, outPut, sets, ids, gvwins)
    dlags > 0 && write_diagnostics(h, outPut)
    if !isempty(holdout)                         # holdoutPredict.txt: record (1-based), y as given, posterior mean and SD of the fitted value
        yin = Vector{Float64}(ycorr); ho = getHoldout(h, nData)
        open(outPut * "/holdoutPredict.txt", "w") do io
            writedlm(io, ["record" "y" "yhat" "sd"])
            for (i, r) in enumerate(ho.rows)
                writedlm(io, Any[r yin[r] ho.mean[i] ho.sd[i]])
            end
        end
    end
    # the caller's arrays as the reference's sampler leaves them: the state after the last iteration
    # read-back buffers by the HANDLE's P: a handle made by set_records! carries one inert block of RECORDS_ONLY_P zero columns, which
    # ngp_get_state copies out like any panel's (include/nextgp_hip.h, ngp_set_records)
    Ptot = isempty(sets) ? RECORDS_ONLY_P : col0
    bet = Vector{Float64}(undef, Ptot); del = Vector{Int64}(undef, Ptot)
    nvb = isempty(sets) ? 0 : sum(length(varBeta[s]) for s in sets)
    vb = Vector{Float64}(undef, max(nvb, 1)); pih = Vector{Float64}(undef, 2 * max(length(sets), 1))
    ve = Ref{Float64}(0.0); bb = Ref{Float64}(0.0); it = Ref{Int64}(0)
    bfix = Vector{Float64}(undef, max(nfix, 1)); sbfix = similar(bfix); nfx = Ref{Int64}(0)
    check(h, ccall((:ngp_get_state, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}, Ref{Int64}),
                   h.ptr, ycorr, bet, del, vb, pih, ve, bb, it))
    check(h, ccall((:ngp_get_fixed, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}), h.ptr, bfix, sbfix, nfx))
    b[1:nfix] .= bfix[1:nfix]                    # positions follow keys(X), like X[xSet].pos (src/mme.jl:112-117)
    for z in zsets
        rs = random_state(h, zids[z], size(Z[z].data, 2))
        vec(u[Z[z].pos]) .= rs.u
        varU[z] = rs.varU
    end
    c0 = 0; v0 = 0
    for s in sets
        P = M[s].dims[2]; nr = length(varBeta[s])
        vec(beta[M[s].pos]) .= bet[c0+1:c0+P]; vec(delta[M[s].pos]) .= del[c0+1:c0+P]
        varBeta[s] isa Vector{Float64} && (varBeta[s] .= vb[v0+1:v0+nr])
        if M[s].method == "BayesRCπ"              # as sampleBayesRCπ! leaves it (src/functions.jl:322-360)
            st = rc_state(h, ids[s], P, length(M[s].piHat), length(M[s].vClass))
            for a in eachindex(M[s].piHat)
                M[s].piHat[a] = st.piHat[a]; M[s].logPi[a] = log.(st.piHat[a])
            end
            M[s].annotProb .= st.annotProb; vec(M[s].annotCat) .= st.annotCat
        end
        if M[s].method == "BayesLV"               # the variance model's state as sampleBayesLV! leaves it (src/functions.jl:466-485)
            st = lv_state(h, ids[s], P, length(M[s].c))
            M[s].c .= st.c; M[s].varZeta[1] = st.varZeta; M[s].logVar .= log.(vb[v0+1:v0+nr]); M[s].SNPVARRESID .= st.zeta
        end
        c0 += P; v0 += nr
    end
    return h
end

end # module
