# VBMatrixFactorizationHIP.jl -- Julia host for the MI355X-native vbmf! path (ccall over include/vbmf_hip.h).
#
# Drop-in for the basic-VBMF surface of VBMatrixFactorization.jl (src/vbmf.jl): the same struct (field
# names, order, Julia types), the same positional/keyword signatures.  Every numeric update runs in
# libvbmf_hip.so (hand-written HIP for gfx950); there is no CPU fallback here.
#
# NOTE: this pipeline has no `julia` binary (neither the build container nor the GPU box), so this
# file cannot be executed or tested here; its tested twin is the Python ctypes host
# (vbmatrixfactorization.jl_amd/__init__.py), which binds the identical entry points.
# Written for Julia >= 1.6 (the reference is Julia 0.5 syntax and does not parse on 1.x).
module VBMatrixFactorizationHIP

export vbmf_parameters, vbmf_init, vbmf, vbmf!, updateA!, updateB!, updateCA!, updateCB!, updateSigma2!, updateYHat!,
       vbls!, vbls_batch!, vbmf_batch!, row_gram_batch, vbmf_sparse_batch!, vbmf_dual_batch!, vbmf_trial_batch!, vbmf_sparse_masked_batch!, copy_vbmf_params, preprocess_device, vbmf_on!, invalidate!,
       vbmf_sparse_parameters, vbmf_sparse_init, vbmf_sparse!, lowerBound, lowerBoundTrimmed,
       residual_batch, lowerBound_batch, lowerBoundTrimmed_batch,
       ols_batch, rls_batch, ls_residual_batch, bag_least_squares_jobs, sparse_fixed_basis_jobs, sparse_scored_jobs, fixed_basis_jobs,
       vbmf_dual_parameters, vbmf_dual_init, vbmf_dual!,
       vbmf_trial_parameters, vbmf_trial_init, vbmf_trial!, set_gram_form!, get_YHat!, get_factor!, set_Y_gather!

const libvbmf = get(ENV, "VBMF_HIP_LIB", joinpath(@__DIR__, "..", "libvbmf_hip.so"))

# ---- the reference struct, src/vbmf.jl:22-40 (same field names, order and types) -----------------
mutable struct vbmf_parameters
    L::Int
    M::Int
    H::Int
    H1::Int
    labels::Array{Int64,1}
    AHat::Array{Float64,2}
    BHat::Array{Float64,2}
    SigmaA::Array{Float64,2}
    SigmaB::Array{Float64,2}
    CA::Array{Float64,2}
    CB::Array{Float64,2}
    invCA::Array{Float64,2}
    invCB::Array{Float64,2}
    sigma2::Float64
    YHat::Array{Float64,2}
    vbmf_parameters() = new()
end

# ---- C ABI ------------------------------------------------------------------------------------------
struct VbmfOpts            # must match vbmf_opts in include/vbmf_hip.h (56 bytes)
    struct_size::Int32
    device::Int32
    y_dtype::Int32
    factor_dtype::Int32
    variant::Int32
    reference_compat::UInt32
    nranks::Int32
    rank::Int32
    L_global::Int64
    row_offset::Int64
    pass1_splits::Int32
    reserved::Int32
end

const VBMF_Y_F32, VBMF_Y_BF16 = Int32(0), Int32(1)
const STEP_A, STEP_B, STEP_CA, STEP_CB, STEP_SIGMA2 = 1, 2, 4, 8, 16
const FIT_FORMS = Dict(:stream => 0, :gram => 1, :auto => 2)     # vbmf_fit_batched_form (include/vbmf_hip.h)
const ARD_FIT_FORMS = Dict(:stream => 0, :auto => 2, :split => 3)  # vbmf_ard_fit_batched_form: these models have no Gram form

# what the basic model takes as Y: the reference's Array{Float64,2}, or an Array{Float32,2} that is uploaded as it is (the
# reference has Float32 methods on this path: scaleY, preprocess, src/util.jl:60,94)
const HostY = Union{Array{Float64,2},Array{Float32,2}}

mutable struct Ctx
    h::Ptr{Cvoid}
    Y::HostY                  # keeps the identity of the uploaded Y
    fp::UInt                  # content fingerprint of Y at upload time (see fingerprint)
end
Ctx(h::Ptr{Cvoid}, Y::HostY) = Ctx(h, Y, fingerprint(Y))

# The reference reads the caller's Y on every call; here it is uploaded once per array object, so a cache hit re-checks a
# content fingerprint (all of Y up to 4M entries, an evenly strided sample of ~64k beyond) and uploads again when the SAME
# array was changed in place (Y .*= lam, Y[:] = other).  invalidate!(Y) drops the device copy explicitly.
function fingerprint(Y::HostY)
    n = length(Y)
    st = n > (1 << 22) ? max(1, n >> 16) : 1
    h = hash(n)
    @inbounds for i in 1:st:n
        h = hash(Y[i], h)
    end
    return h
end

function chk(h::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:vbmf_last_error, libvbmf), Cstring, (Ptr{Cvoid},), h))
    error("vbmf_hip error $rc: $msg")          # the reference signals errors with error(...), src/util.jl:116
end

# after a call that returned OK: the library's note, if any (vbmf_last_error text starting with "note:", e.g. vbmf_run's remark on an
# eps below what d resolves on the device -- include/vbmf_hip.h), becomes a warning
function warn_note(h::Ptr{Cvoid})
    msg = unsafe_string(ccall((:vbmf_last_error, libvbmf), Cstring, (Ptr{Cvoid},), h))
    startswith(msg, "note:") && @warn msg
end

const VBMF_SRC_F64, VBMF_SRC_F32, VBMF_SRC_BF16 = Int32(0), Int32(1), Int32(2)

"Upload Y into the context: a Float64 matrix through vbmf_set_Y; a Float32 matrix in its own format, with no Float64 copy, through vbmf_set_Y_rows (host source, whole matrix, column-major: row stride 1, column stride L)."
set_Y!(h::Ptr{Cvoid}, Y::Array{Float64,2}) =
    chk(h, ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h, Y, size(Y, 1)))
function set_Y!(h::Ptr{Cvoid}, Y::Array{Float32,2})
    L = size(Y, 1)
    chk(h, ccall((:vbmf_set_Y_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Int64),
                 h, Y, VBMF_SRC_F32, Int32(0), 0, L, 1, L))
end

"""
    set_Y_gather!(dst, src, cols)

Y of the context handle `dst` := columns `cols` (1-based, in that order, duplicates allowed) of the Y stored in the context handle `src`,
gathered on the device through vbmf_set_Y_gather: what get_matrices (examples/mil_util.jl:46) builds on the host for every fold, from
a data set that was uploaded once.  `dst` must have length(cols) columns and `src`'s L, storage type and device.
"""
function set_Y_gather!(dst::Ptr{Cvoid}, src::Ptr{Cvoid}, cols::AbstractVector{<:Integer})
    idx = Int64[c - 1 for c in cols]
    chk(dst, ccall((:vbmf_set_Y_gather, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int64), dst, src, idx, length(idx)))
end

const VBMF_DST_F64, VBMF_DST_F32 = Int32(0), Int32(1)

"""
    get_YHat!(ctx, dst; residual = false, row0 = 0)

Rows row0 .. row0 + size(dst, 1) - 1 (0-based row0, this context's local rows) of updateYHat! (src/vbmf.jl:120-122), BHat*AHat', written
into the host matrix `dst` in its own format through vbmf_get_YHat_rows -- no Float64 copy for a Float32 `dst`; `residual = true` gives Y as
stored minus the product.  Host arrays only (column-major: row stride 1, column stride size(dst, 1)).  Returns dst.
"""
function get_YHat!(c::Ctx, dst::Array{Float32,2}; residual::Bool = false, row0::Int = 0)
    n = size(dst, 1); what = Int32(residual ? 1 : 0)
    chk(c.h, ccall((:vbmf_get_YHat_rows, libvbmf), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Int64),
                   c.h, what, dst, VBMF_DST_F32, Int32(0), row0, n, 1, n))
    dst
end
function get_YHat!(c::Ctx, dst::Array{Float64,2}; residual::Bool = false, row0::Int = 0)
    n = size(dst, 1); what = Int32(residual ? 1 : 0)
    chk(c.h, ccall((:vbmf_get_YHat_rows, libvbmf), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Int64),
                   c.h, what, dst, VBMF_DST_F64, Int32(0), row0, n, 1, n))
    dst
end

"""
    get_factor!(ctx, which, dst; row0 = 0)

Rows row0 .. of AHat (`which = :A`, M x H) or of this context's BHat (`:B`, L x H) -- the Float32 values the device holds, what pull! widens --
into the host matrix `dst` (Float32: a copy; Float64: a widening) through vbmf_get_factor_rows.  Returns dst.
"""
function get_factor!(c::Ctx, which::Symbol, dst::Array{Float32,2}; row0::Int = 0)
    n = size(dst, 1); w = Int32(which == :B ? 1 : 0)
    chk(c.h, ccall((:vbmf_get_factor_rows, libvbmf), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Int64),
                   c.h, w, dst, VBMF_DST_F32, Int32(0), row0, n, 1, n))
    dst
end
function get_factor!(c::Ctx, which::Symbol, dst::Array{Float64,2}; row0::Int = 0)
    n = size(dst, 1); w = Int32(which == :B ? 1 : 0)
    chk(c.h, ccall((:vbmf_get_factor_rows, libvbmf), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Int64),
                   c.h, w, dst, VBMF_DST_F64, Int32(0), row0, n, 1, n))
    dst
end

const _cache = Dict{UInt,Ctx}()

# fp32 storage of the caller's Float64 Y by default; ENV["VBMF_HIP_Y"] = "bf16" opts into bf16 storage (the BASELINE headline
# configuration): that changes the data the model sees and must be chosen knowingly
y_dtype() = get(ENV, "VBMF_HIP_Y", "f32") == "bf16" ? VBMF_Y_BF16 : VBMF_Y_F32

function refresh!(c::Ctx, Y::HostY)
    fp = fingerprint(Y)
    if fp != c.fp                                          # same array object, new contents: upload again
        set_Y!(c.h, Y)
        c.fp = fp
    end
    return c
end

"Drop the cached device copies of Y (all of them without an argument)."
function invalidate!(Y = nothing)
    for d in (_cache, _scache), (k, c) in collect(d)
        (Y === nothing || c.Y === Y) && (finalize(c); delete!(d, k))
    end
end

"One device context per Y array (uploaded once, re-uploaded when its contents change)."
function ctx_for(Y::HostY, H::Int)
    key = hash((objectid(Y), size(Y), H))
    haskey(_cache, key) && return refresh!(_cache[key], Y)
    L, M = size(Y)
    ydt = y_dtype()
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, ydt, 0, 0, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts)
    chk(Ptr{Cvoid}(C_NULL), rc)
    c = Ctx(h[], Y)
    finalizer(x -> ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), x.h), c)
    set_Y!(c.h, Y)
    _cache[key] = c
    return c
end

"Context for the updates whose reference signatures take no Y (updateCA!, updateCB!, updateYHat!): never given a matrix."
function ctx_noY(L::Int, M::Int, H::Int; variant::Int = 0)
    key = hash((:noY, L, M, H, variant))
    haskey(_cache, key) && return _cache[key]
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, variant, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    c = Ctx(h[], Array{Float64}(undef, 0, 0), UInt(0))
    finalizer(x -> ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), x.h), c)
    _cache[key] = c
    return c
end

function push!(c::Ctx, p::vbmf_parameters)
    ca = [p.CA[h, h] for h in 1:p.H]; cb = [p.CB[h, h] for h in 1:p.H]
    lab0 = p.labels .- 1                                   # C side is 0-based
    chk(c.h, ccall((:vbmf_set_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Float64, Ptr{Int64}, Int64, Int64),
        c.h, p.AHat, p.M, p.BHat, p.L, p.SigmaA, p.SigmaB, ca, cb, p.sigma2, lab0, length(lab0), p.H1))
end

function pull!(c::Ctx, p::vbmf_parameters)
    # the reference rebinds these fields with fresh arrays (src/vbmf.jl:96-98,110-112) ...
    A = Array{Float64}(undef, p.M, p.H); B = Array{Float64}(undef, p.L, p.H)
    SA = Array{Float64}(undef, p.H, p.H); SB = Array{Float64}(undef, p.H, p.H)
    ca = Array{Float64}(undef, p.H); cb = Array{Float64}(undef, p.H); s2 = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_get_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
        c.h, A, p.M, B, p.L, SA, SB, ca, cb, s2))
    p.AHat, p.BHat, p.SigmaA, p.SigmaB = A, B, SA, SB
    for h in 1:p.H                                          # ... and writes CA/CB diagonals in place (:131,143)
        p.CA[h, h] = ca[h]; p.CB[h, h] = cb[h]
    end
    p.invCA = inv(p.CA); p.invCB = inv(p.CB)
    p.sigma2 = s2[]
    return p
end

step!(Y, p, which) = (c = ctx_for(Y, p.H); push!(c, p); chk(c.h, ccall((:vbmf_step, libvbmf), Cint, (Ptr{Cvoid}, Cint), c.h, which)); pull!(c, p); nothing)

# ---- the reference surface ---------------------------------------------------------------------------
"src/vbmf.jl:48-73 (host side: the random draw is not part of the accelerated path)"
function vbmf_init(Y::HostY, H::Int; ca::Float64 = 1.0, cb::Float64 = 1.0, sigma2::Float64 = 1.0,
                   H1::Int = 0, labels::Array{Int64,1} = Array{Int64,1}())
    params = vbmf_parameters()
    L, M = size(Y)
    params.L, params.M, params.H, params.H1, params.labels = L, M, H, H1, labels
    params.AHat = randn(M, H)
    params.AHat[labels, end-H1+1:end] .= 0.0
    params.BHat = randn(L, H)
    params.SigmaA = zeros(H, H); params.SigmaB = zeros(H, H)
    Id = Matrix{Float64}(I_(H))
    params.CA = ca * Id; params.CB = cb * Id
    params.invCA = inv(params.CA); params.invCB = inv(params.CB)
    params.sigma2 = sigma2
    params.YHat = L * M <= (1 << 24) ? params.BHat * params.AHat' : Array{Float64}(undef, 0, 0)   # lazy above 16M elements
    return params
end
I_(H) = [i == j ? 1.0 : 0.0 for i in 1:H, j in 1:H]

"src/vbmf.jl:80-88 (shallow)"
function Base.copy(params_in::vbmf_parameters)
    params = vbmf_parameters()
    for f in fieldnames(vbmf_parameters)
        isdefined(params_in, f) && setfield!(params, f, getfield(params_in, f))
    end
    return params
end

updateA!(Y::Array{Float64,2}, params::vbmf_parameters) = step!(Y, params, STEP_A)            # src/vbmf.jl:95-102
updateB!(Y::Array{Float64,2}, params::vbmf_parameters) = step!(Y, params, STEP_B)            # :109-113
updateSigma2!(Y::Array{Float64,2}, params::vbmf_parameters) = step!(Y, params, STEP_SIGMA2)  # :153-157
# the reference's updateCA!/updateCB!/updateYHat! take only params (src/vbmf.jl:120-146): so do these -- the library runs
# them from the factors and covariances alone, on a context that holds no matrix
function step_noY!(p::vbmf_parameters, which)
    c = ctx_noY(p.L, p.M, p.H); push!(c, p)
    chk(c.h, ccall((:vbmf_step, libvbmf), Cint, (Ptr{Cvoid}, Cint), c.h, which)); pull!(c, p); nothing
end
updateCA!(params::vbmf_parameters) = step_noY!(params, STEP_CA)                               # :129-134
updateCB!(params::vbmf_parameters) = step_noY!(params, STEP_CB)                               # :141-146
function updateYHat!(params::vbmf_parameters)                                                # :120-122
    c = ctx_noY(params.L, params.M, params.H); push!(c, params)
    params.YHat = Array{Float64}(undef, params.L, params.M)
    chk(c.h, ccall((:vbmf_get_YHat, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), c.h, params.YHat, params.L))
end

"vbmf! -- src/vbmf.jl:175-231"
function vbmf!(Y::Array{Float64,2}, params::vbmf_parameters, niter::Int; eps::Float64 = 1e-6, est_covs::Bool = false,
               est_var::Bool = false, logdir = "", desc = "", verb = false, form = nothing)
    return fit_basic!(Y, params, niter, eps, est_covs, est_var, logdir, verb, form)
end
"vbmf! on a Float32 matrix: uploaded in its own format (vbmf_set_Y_rows), everything else as above"
function vbmf!(Y::Array{Float32,2}, params::vbmf_parameters, niter::Int; eps::Float64 = 1e-6, est_covs::Bool = false,
               est_var::Bool = false, logdir = "", desc = "", verb = false, form = nothing)
    return fit_basic!(Y, params, niter, eps, est_covs, est_var, logdir, verb, form)
end
function fit_basic!(Y::HostY, params::vbmf_parameters, niter::Int, eps::Float64, est_covs::Bool, est_var::Bool, logdir, verb,
                    form = nothing)
    logdir == "" || error("per-iteration logging: drive the sweeps from the reference's own create_log / update_log! / save_log " *
                          "(src/data_manip.jl works unchanged on these structs) around vbmf!(Y, params, 1; ...) calls")
    c = ctx_for(Y, params.H)
    apply_form!(c, form, params.H > 128 ? "H > 128 (the basic model's Gram sweep covers H <= 128)" : "")
    push!(c, params)
    iters = Ref{Int64}(0); d = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_run, libvbmf), Cint,
        (Ptr{Cvoid}, Int64, Float64, Cint, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
        c.h, niter, eps, est_covs, est_var, iters, d, C_NULL))
    warn_note(c.h)
    pull!(c, params)
    params.L * params.M <= (1 << 24) && updateYHat!(params)                                   # :217
    verb && print("Factorization finished after ", iters[], " iterations, eps = ", d[], "\n")  # :221
    return params
end

"vbmf -- src/vbmf.jl:238-248"
function vbmf(Y::HostY, params_in::vbmf_parameters, niter::Int; kwargs...)
    params = copy(params_in)
    params.CA, params.CB = copy(params.CA), copy(params.CB)     # keep params_in reusable (see SURVEY App. A Q2)
    vbmf!(Y, params, niter; kwargs...)
    return params
end

"vbls! -- examples/mil_util.jl:179-203 (vbmf_parameters branch): A/CA/sigma2 sweeps with B frozen; Y'B is formed once"
function vbls!(Y::Array{Float64,2}, params::vbmf_parameters, niter::Int; diag_var::Bool = false, full_cov::Bool = false)
    (diag_var || full_cov) && error("only full_cov=false, diag_var=false is built")
    c = ctx_for(Y, params.H)
    push!(c, params)
    chk(c.h, ccall((:vbmf_run_fixed_basis, libvbmf), Cint, (Ptr{Cvoid}, Int64), c.h, niter))
    pull!(c, params)
    params.L * params.M <= (1 << 24) && updateYHat!(params)                                   # :201
    return params.AHat
end

"""
vbls! over many bags with one fixed basis in ONE device call (examples/mil_util.jl:473-479): does what
`[vbls!(Y, p, niter) for (Y, p) in zip(Ys, ps)]` does for the basic model -- fills AHat, SigmaA, CA, invCA, sigma2 (and YHat up
to 2^24 entries) of every p and returns their AHat.  The bags share L; the parameters share BHat, SigmaB and CB, carry no labels,
and H <= 64 (anything else: vbls! per bag).  The bags are uploaded side by side into one context for the call.
"""
function vbls_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_parameters}, niter::Int)
    nb = length(Ys)
    (nb >= 1 && length(ps) == nb) || error("vbls_batch!: one parameter set per bag")
    p0 = ps[1]
    H, L = p0.H, size(Ys[1], 1)
    H <= 64 || error("vbls_batch!: H = $H > 64; use vbls! per bag")
    for b in 1:nb
        Y, p = Ys[b], ps[b]
        size(Y, 1) == L || error("vbls_batch!: the bags have different L; use vbls! per bag")
        (size(Y, 2) >= 1 && (p.L, p.M, p.H) == (L, size(Y, 2), H)) || error("vbls_batch!: bag $b does not match its parameters")
        (p.H1 == 0 && isempty(p.labels)) || error("vbls_batch!: bag $b has labels; use vbls! per bag")
        (p.BHat == p0.BHat && p.SigmaB == p0.SigmaB && p.CB == p0.CB) ||
            error("vbls_batch!: bag $b does not share BHat, SigmaB and CB with bag 1; use vbls! per bag")
    end
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    M = off[end]
    Yall = reduce(hcat, Ys)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, 0, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    s2 = [p.sigma2 for p in ps]
    ca = Float64[ps[b].CA[i, i] for i in 1:H, b in 1:nb]           # CA_diag[b*H + h] (0-based)
    SA = Array{Float64}(undef, H, H, nb)
    A = Array{Float64}(undef, M, H)
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        ca0 = [p0.CA[i, i] for i in 1:H]; cb0 = [p0.CB[i, i] for i in 1:H]
        chk(h[], ccall((:vbmf_set_state, libvbmf), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Float64, Ptr{Int64}, Int64, Int64),
            h[], zeros(M, H), M, p0.BHat, L, p0.SigmaA, p0.SigmaB, ca0, cb0, p0.sigma2, Int64[], 0, 0))
        chk(h[], ccall((:vbmf_run_fixed_basis_batched, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
            h[], nb, off, niter, s2, ca, SA, A, M))
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
    for b in 1:nb
        p = ps[b]
        p.AHat = A[off[b]+1:off[b+1], :]
        p.SigmaA = SA[:, :, b]
        for i in 1:H                                                # CA diagonal in place (src/vbmf.jl:131)
            p.CA[i, i] = ca[i, b]
        end
        p.invCA = inv(p.CA)
        p.sigma2 = s2[b]
        p.L * p.M <= (1 << 24) && (p.YHat = p.BHat * p.AHat')        # :201
    end
    return [p.AHat for p in ps]
end

"""
vbmf! for many independent fits of the basic model in ONE device call (the two fits of examples/mil_util.jl:110-114 and the folds
around them): does what `[vbmf!(Ys[bag_of[f]], ps[f], niter; eps = eps, est_covs = est_covs, est_var = est_var) for f in 1:length(ps)]`
does -- every fit's whole loop of src/vbmf.jl:175-231 in one workgroup of one launch (vbmf_fit_batched) -- and returns
(d, sweeps run, status) per fit; status 1 = the fit met a non-finite sigma2, a CA / CB entry that is not positive, or a bad pivot, and
stopped.  Fit f works on bag bag_of[f] (1-based).  The bags share L; no labels, H <= 32 (anything else: vbmf! per fit).
form: :stream (Y is read twice per sweep), :gram (the sweep runs on Y*Y', built once per bag: the form for bags much wider than tall) or
:auto (per fit: Gram where M_b >= 2L and its 3*L*H doubles of state fit in LDS) -- the same iteration, different rounding
(vbmf_fit_batched_form).
"""
function vbmf_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_parameters}, niter::Int; eps::Float64 = 1e-6, est_covs::Bool = false,
                     est_var::Bool = false, bag_of::Vector{Int} = collect(1:length(ps)), form::Symbol = :stream)
    haskey(FIT_FORMS, form) || error("vbmf_batch!: form = $form (:stream, :gram or :auto)")
    nb, nf = length(Ys), length(ps)
    (nb >= 1 && nf >= 1 && length(bag_of) == nf) || error("vbmf_batch!: one bag_of entry per parameter set")
    niter >= 1 || error("vbmf_batch!: niter must be >= 1")
    H, L = ps[1].H, size(Ys[1], 1)
    H <= 32 || error("vbmf_batch!: H = $H > 32; use vbmf! per fit")
    all(size(Y, 1) == L && size(Y, 2) >= 1 for Y in Ys) || error("vbmf_batch!: the bags have different L; use vbmf! per fit")
    for (f, p) in enumerate(ps)
        1 <= bag_of[f] <= nb || error("vbmf_batch!: bag_of[$f] = $(bag_of[f]) outside 1..$nb")
        (p.L, p.M, p.H) == (L, size(Ys[bag_of[f]], 2), H) || error("vbmf_batch!: fit $f does not match its bag")
        (p.H1 == 0 && isempty(p.labels)) || error("vbmf_batch!: fit $f has labels; use vbmf! per fit")
    end
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    M = off[end]
    Yall = reduce(hcat, Ys)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, 0, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    fb = Int64[b - 1 for b in bag_of]
    B = reduce(vcat, [vec(Matrix{Float64}(p.BHat)) for p in ps]); SB = reduce(vcat, [vec(Matrix{Float64}(p.SigmaB)) for p in ps])
    ca = Float64[p.CA[i, i] for i in 1:H, p in ps]; cb = Float64[p.CB[i, i] for i in 1:H, p in ps]
    s2 = Float64[p.sigma2 for p in ps]
    A = Array{Float64}(undef, sum(p.M for p in ps) * H)
    SA = Array{Float64}(undef, H, H, nf)
    it = zeros(Int64, nf); dlast = Array{Float64}(undef, nf); st = zeros(Int64, nf)
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        if form == :stream
            chk(h[], ccall((:vbmf_fit_batched, libvbmf), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Float64, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                h[], nb, off, nf, fb, niter, eps, est_covs, est_var, B, SB, ca, cb, s2, A, SA, it, dlast, st, C_NULL))
        else
            chk(h[], ccall((:vbmf_fit_batched_form, libvbmf), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Float64, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64,
                 Ptr{Int64}),
                h[], nb, off, nf, fb, niter, eps, est_covs, est_var, B, SB, ca, cb, s2, A, SA, it, dlast, st, C_NULL, FIT_FORMS[form],
                C_NULL))
        end
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
    s = 0
    for (f, p) in enumerate(ps)
        p.AHat = reshape(A[s+1:s+p.M*H], p.M, H)                    # rebound, like updateA! / updateB! (src/vbmf.jl:96-98,110-112)
        s += p.M * H
        p.BHat = reshape(B[(f-1)*L*H+1:f*L*H], L, H)
        p.SigmaA = SA[:, :, f]
        p.SigmaB = reshape(SB[(f-1)*H*H+1:f*H*H], H, H)
        for i in 1:H                                                # the diagonals in place (src/vbmf.jl:131,143)
            p.CA[i, i] = ca[i, f]
            p.CB[i, i] = cb[i, f]
        end
        p.invCA = inv(p.CA); p.invCB = inv(p.CB)
        p.sigma2 = s2[f]
        p.L * p.M <= (1 << 24) && (p.YHat = p.BHat * p.AHat')        # :217
    end
    return dlast, it, st
end

"""
K_b = Y_b*Y_b' of every bag in ONE device call, in fp64 on Y as stored (vbmf_bags_row_gram): an L x L x nbags array, every slice
symmetric bit for bit.  What vbmf_batch!(...; form = :gram) iterates on; ols / rls callers form B'*K_b*B from it.
"""
function row_gram_batch(Ys::Vector{Matrix{Float64}})
    nb = length(Ys)
    nb >= 1 || error("row_gram_batch: no bags")
    L = size(Ys[1], 1)
    all(size(Y, 1) == L && size(Y, 2) >= 1 for Y in Ys) || error("row_gram_batch: the bags have different L, or one is empty")
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    Yall = reduce(hcat, Ys)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, 0, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, off[end], 1, opts))
    K = Array{Float64}(undef, L, L, nb)
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        chk(h[], ccall((:vbmf_bags_row_gram, libvbmf), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}), h[], nb, off, K))
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
    return K
end

"copy_vbmf_params -- examples/mil_util.jl:212-236 (vbmf_parameters branch)"
function copy_vbmf_params(Y::Array{Float64,2}, old_params::vbmf_parameters)
    params = vbmf_init(Y, old_params.H, sigma2 = old_params.sigma2)
    params.BHat = copy(old_params.BHat); params.SigmaB = copy(old_params.SigmaB)
    params.CB = copy(old_params.CB); params.invCB = copy(old_params.invCB)
    return params
end

"""
preprocess -- src/util.jl:73-86 fused into the upload.  Returns (ctx, used_rows): a device context holding
lambda * scaleY(Y)[used_rows, :] (never materialised on the host) for a factorization of rank H, and the kept rows
(1-based).  Create parameters for L = length(used_rows) and run them with `vbmf_on!(ctx, params, niter; ...)`.
"""
function preprocess_device(Y::Array{Float64,2}, lambda::Float64, H::Int)
    L, M = size(Y)
    plan = Ref{Ptr{Cvoid}}(C_NULL); nused = Ref{Int64}(0)
    rc = ccall((:vbmf_preprocess_open, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Cint, Ptr{Float64}, Int64, Int64, Int64, Ref{Int64}),
               plan, 0, Y, L, M, L, nused)
    rc == 0 || error(unsafe_string(ccall((:vbmf_last_error, libvbmf), Cstring, (Ptr{Cvoid},), C_NULL)))
    rows = Array{Int64}(undef, nused[])
    ccall((:vbmf_preprocess_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}), plan[], rows, C_NULL, C_NULL)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    ydt = y_dtype()
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, ydt, 0, 0, 0xffffffff, 1, 0, 0, 0, 0, 0))
    rc = ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, nused[], M, H, opts)
    rc == 0 || error(unsafe_string(ccall((:vbmf_last_error, libvbmf), Cstring, (Ptr{Cvoid},), C_NULL)))
    chk(h[], ccall((:vbmf_set_Y_preprocessed, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64), h[], plan[], lambda))
    ccall((:vbmf_preprocess_close, libvbmf), Cint, (Ptr{Cvoid},), plan[])
    c = Ctx(h[], Y)
    finalizer(x -> ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), x.h), c)
    return c, rows .+ 1
end

"vbmf! on a context that already holds its matrix (preprocess_device): same loop as vbmf!"
function vbmf_on!(c::Ctx, params::vbmf_parameters, niter::Int; eps::Float64 = 1e-6, est_covs::Bool = false, est_var::Bool = false)
    push!(c, params)
    iters = Ref{Int64}(0); d = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_run, libvbmf), Cint,
        (Ptr{Cvoid}, Int64, Float64, Cint, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
        c.h, niter, eps, est_covs, est_var, iters, d, C_NULL))
    pull!(c, params)
    return params
end

# ---- the ARD-sparse variant, src/vbmf_sparse.jl (full_cov = false | true; diag_var = false | true) ------
# Same field names as the reference's vbmf_sparse_parameters (src/vbmf_sparse.jl:47-90); the dense MH x MH
# SigmaATVec / invSigmaATVec of the full_cov branch are not carried (they cannot exist at scale, :120,122).
mutable struct vbmf_sparse_parameters
    L::Int; M::Int; H::Int; MH::Int; H1::Int
    labels::Array{Int64,1}
    AHat::Array{Float64,2}; ATVecHat::Array{Float64,1}; diagSigmaATVec::Array{Float64,1}; SigmaA::Array{Float64,2}
    BHat::Array{Float64,2}; SigmaB::Array{Float64,2}
    CA::Array{Float64,1}; alpha0::Float64; beta0::Float64; alpha::Float64; beta::Array{Float64,1}
    CB::Array{Float64,1}; gamma0::Float64; delta0::Float64; gamma::Float64; delta::Array{Float64,1}
    sigmaHat::Float64; eta0::Float64; zeta0::Float64; eta::Float64; zeta::Float64
    sigmaVecHat::Array{Float64,1}; etaVec::Array{Float64,1}; zetaVec::Array{Float64,1}
    YHat::Array{Float64,2}; trYTY::Float64
    vbmf_sparse_parameters() = new()
end

struct SparseHyper
    alpha0::Float64; beta0::Float64; gamma0::Float64; delta0::Float64; eta0::Float64; zeta0::Float64
end

"src/vbmf_sparse.jl:101-153"
function vbmf_sparse_init(Y::Array{Float64,2}, H::Int; ca = 1.0, alpha0 = 1e-10, beta0 = 1e-10, cb = 1.0, gamma0 = 1e-10,
                          delta0 = 1e-10, sigma = 1.0, eta0 = 1e-10, zeta0 = 1e-10, H1::Int = 0,
                          labels::Array{Int64,1} = Array{Int64,1}())
    p = vbmf_sparse_parameters(); L, M = size(Y)
    p.L, p.M, p.H, p.MH, p.H1, p.labels = L, M, H, M * H, H1, labels
    p.AHat = randn(M, H); p.AHat[labels, end-H1+1:end] .= 0.0
    p.ATVecHat = reshape(permutedims(p.AHat), M * H); p.diagSigmaATVec = ones(M * H); p.SigmaA = zeros(H, H)
    p.BHat = randn(L, H); p.SigmaB = zeros(H, H)
    p.CA = ca * ones(M * H); p.alpha0, p.beta0, p.alpha, p.beta = alpha0, beta0, alpha0 + 0.5, beta0 * ones(M * H)
    p.CB = cb * ones(H); p.gamma0, p.delta0, p.gamma, p.delta = gamma0, delta0, gamma0 + L / 2, delta0 * ones(H)
    p.sigmaHat, p.eta0, p.zeta0, p.eta, p.zeta = sigma, eta0, zeta0, eta0 + L * M / 2, zeta0
    p.sigmaVecHat, p.etaVec, p.zetaVec = sigma * ones(L), (eta0 + M / 2) * ones(L), zeta0 * ones(L)
    p.YHat = L * M <= (1 << 24) ? p.BHat * p.AHat' : Array{Float64}(undef, 0, 0)
    p.trYTY = sum(abs2, Y)
    return p
end

const _scache = Dict{UInt,Ctx}()
function sparse_ctx_for(Y::Array{Float64,2}, H::Int, diag_var::Bool; variant::Int = diag_var ? 2 : 1)
    key = hash((objectid(Y), size(Y), H, variant))
    haskey(_scache, key) && return refresh!(_scache[key], Y)
    L, M = size(Y)
    ydt = y_dtype()
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, ydt, 0, variant, 0xffffffff, 1, 0, 0, 0, 0, 0))   # VBMF_VARIANT_*
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Y, L))
    c = Ctx(h[], Y); finalizer(x -> ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), x.h), c)
    _scache[key] = c
    return c
end

function spush!(c::Ctx, p::vbmf_sparse_parameters, diag_var::Bool)
    hy = Ref(SparseHyper(p.alpha0, p.beta0, p.gamma0, p.delta0, p.eta0, p.zeta0)); lab0 = p.labels .- 1
    chk(c.h, ccall((:vbmf_sparse_set_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Float64, Float64, Ref{SparseHyper}, Ptr{Int64}, Int64, Int64),
        c.h, p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta, p.BHat, p.L, p.SigmaB, p.CB, p.delta, p.sigmaHat, p.zeta, hy,
        lab0, length(lab0), p.H1))
    diag_var && chk(c.h, ccall((:vbmf_sparse_set_noise_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64),
                               c.h, p.sigmaVecHat, p.zetaVec, p.etaVec[1]))
end

# full_cov = true (src/vbmf_sparse.jl:178-202): the dense MH x MH covariance is block diagonal, the device inverts the M
# H x H blocks; SigmaA is a full matrix then and is handed over explicitly
function set_full_cov!(c::Ctx, p, full_cov::Bool)
    chk(c.h, ccall((:vbmf_sparse_set_full_cov, libvbmf), Cint, (Ptr{Cvoid}, Cint), c.h, full_cov))
    # always: set_state derives a diagonal SigmaA from diagSigmaATVec, which is not what a fresh init holds (zeros, :120-123)
    chk(c.h, ccall((:vbmf_sparse_set_SigmaA, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}), c.h, p.SigmaA))
end
# Which form the run loops take (vbmf_set_gram_form, include/vbmf_hip.h): 0 the library's rule, 1 stream, 2 the Gram form
# wherever the structure allows it -- for the ARD-sparse model up to H = 256 (src/vbmf_sparse.jl:344-412 on G = Y'Y).
const GRAM_FORMS = Dict(:default => 0, :stream => 1, :gram => 2)
function set_gram_form!(c::Ctx, form::Symbol)
    haskey(GRAM_FORMS, form) || error("form must be :stream or :gram (or nothing), not $form")
    chk(c.h, ccall((:vbmf_set_gram_form, libvbmf), Cint, (Ptr{Cvoid}, Cint), c.h, GRAM_FORMS[form]))
end
"true when the context's run loops take the Gram form (word 16 of VBMF_PEEK_DIMS)"
function gram_form_resolved(c::Ctx)
    v = zeros(UInt32, 28)
    chk(c.h, ccall((:vbmf_debug_peek, libvbmf), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt32}, Int64, Int64), c.h, 8, v, 28, 0))
    return v[17] != 0
end
# the `form` keyword of vbmf! / vbmf_sparse!: nothing makes no call; :gram on a context that cannot take the form is an error
# that names the reason (why: what the caller's arguments rule out; the storage formats and row shards otherwise)
function apply_form!(c::Ctx, form, why::String)
    form === nothing && return
    set_gram_form!(c, form)
    if form == :gram && !gram_form_resolved(c)
        set_gram_form!(c, :default)
        error("form = :gram refused: " * (why != "" ? why :
              "the Gram form needs bf16 storage of Y (ENV[\"VBMF_HIP_Y\"] = \"bf16\"; fp32 is the default), bf16x2 factors and one rank"))
    end
end

function pull_SigmaA!(c::Ctx, p)
    S = Array{Float64}(undef, p.H, p.H)
    chk(c.h, ccall((:vbmf_sparse_get_SigmaA, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}), c.h, S))
    p.SigmaA = S
end

function spull!(c::Ctx, p::vbmf_sparse_parameters, diag_var::Bool)
    n = p.M * p.H
    a = Array{Float64}(undef, n); ds = similar(a); ca = similar(a); be = similar(a); sa = Array{Float64}(undef, p.H)
    B = Array{Float64}(undef, p.L, p.H); SB = Array{Float64}(undef, p.H, p.H); cb = Array{Float64}(undef, p.H); dl = similar(cb)
    sh = Ref{Float64}(0.0); ze = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_sparse_get_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}),
        c.h, a, ds, ca, be, sa, B, p.L, SB, cb, dl, sh, ze))
    p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta = a, ds, ca, be
    p.AHat = permutedims(reshape(a, p.H, p.M)); p.SigmaA = [i == j ? sa[i] : 0.0 for i in 1:p.H, j in 1:p.H]
    p.BHat, p.SigmaB, p.CB, p.delta = B, SB, cb, dl
    if diag_var
        s = Array{Float64}(undef, p.L); z = similar(s)
        chk(c.h, ccall((:vbmf_sparse_get_noise_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), c.h, s, z))
        p.sigmaVecHat, p.zetaVec = s, z
    else
        p.sigmaHat, p.zeta = sh[], ze[]
    end
    return p
end

"vbmf_sparse! -- src/vbmf_sparse.jl:344-410 (returns d, like the reference)"
function vbmf_sparse!(Y::Array{Float64,2}, params::vbmf_sparse_parameters, niter::Int; eps::Float64 = 1e-6, diag_var::Bool = false,
                      full_cov::Bool = false, logdir = "", desc = "", verb = false, est_cb::Bool = true, form = nothing)
    full_cov && params.H > 256 && error("full_cov=true is built for H <= 256 (either noise model)")
    logdir == "" || error("trajectory logging lives in the Python host (data_manip.py)")
    c = sparse_ctx_for(Y, params.H, diag_var); spush!(c, params, diag_var)
    set_full_cov!(c, params, full_cov)
    # form = :stream | :gram (an extension: the reference has no such keyword); :gram iterates on Y'Y up to H = 256
    apply_form!(c, form, diag_var ? "diag_var = true" : full_cov ? "full_cov = true" : params.H > 256 ? "H > 256" : "")
    iters = Ref{Int64}(0); d = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_sparse_run, libvbmf), Cint, (Ptr{Cvoid}, Int64, Float64, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
                   c.h, niter, eps, est_cb, iters, d, C_NULL))
    spull!(c, params, diag_var)
    pull_SigmaA!(c, params)
    params.L * params.M <= (1 << 24) && (params.YHat = params.BHat * params.AHat')            # :396
    verb && print("Factorization finished after ", iters[], " iterations, eps = ", d[], "\n")
    return d[]
end

"lowerBound -- src/vbmf_sparse.jl:435-471 (homoscedastic model)"
function lowerBound(Y::Array{Float64,2}, params::vbmf_sparse_parameters)
    c = sparse_ctx_for(Y, params.H, false); spush!(c, params, false); set_full_cov!(c, params, false)
    lb = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_sparse_lower_bound, libvbmf), Cint, (Ptr{Cvoid}, Cint, Ref{Float64}), c.h, 1, lb))
    return lb[]
end

"lowerBoundTrimmed -- src/vbmf_sparse.jl:478-489 (examples/mil_util.jl:505): entries with abs(ATVecHat) <= trim are left out"
function lowerBoundTrimmed(Y::Array{Float64,2}, params::vbmf_sparse_parameters, trim = 1e-1)
    c = sparse_ctx_for(Y, params.H, false); spush!(c, params, false); set_full_cov!(c, params, false)
    lb = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_sparse_lower_bound_trimmed, libvbmf), Cint, (Ptr{Cvoid}, Cint, Float64, Ref{Float64}), c.h, 1, trim, lb))
    return lb[]
end

"updateCA! / updateCB! of the sparse model take no Y (src/vbmf_sparse.jl:284-300)"
function sparse_step_noY!(p::vbmf_sparse_parameters, which)
    c = ctx_noY(p.L, p.M, p.H; variant = 1); spush!(c, p, false); set_full_cov!(c, p, false)
    chk(c.h, ccall((:vbmf_sparse_step, libvbmf), Cint, (Ptr{Cvoid}, Cint), c.h, which)); spull!(c, p, false); nothing
end
updateCA!(params::vbmf_sparse_parameters) = sparse_step_noY!(params, 4)      # VBMF_SSTEP_CA
updateCB!(params::vbmf_sparse_parameters) = sparse_step_noY!(params, 8)      # VBMF_SSTEP_CB

# ---- the two-group variant, src/vbmf_dual.jl ------------------------------------------------------------------------------
# Field names of the reference's vbmf_dual_parameters (src/vbmf_dual.jl:59-112) minus the dense MH x MH pair.
mutable struct vbmf_dual_parameters
    L::Int; M::Int; MH::Int; H::Int; H0::Int; H1::Int
    AHat::Array{Float64,2}; ATVecHat::Array{Float64,1}; diagSigmaATVec::Array{Float64,1}; SigmaA::Array{Float64,2}
    A0Hat::Array{Float64,2}; A1Hat::Array{Float64,2}
    BHat::Array{Float64,2}; SigmaB::Array{Float64,2}
    CA::Array{Float64,1}; alpha::Array{Float64,1}; beta::Array{Float64,1}
    CA0::Array{Float64,1}; alpha00::Float64; beta00::Float64; alpha0::Float64; beta0::Array{Float64,1}
    CA1::Array{Float64,1}; alpha01::Float64; beta01::Float64; alpha1::Float64; beta1::Array{Float64,1}
    CB::Array{Float64,1}; gamma0::Float64; delta0::Float64; gamma::Float64; delta::Array{Float64,1}
    sigmaHat::Float64; eta0::Float64; zeta0::Float64; eta::Float64; zeta::Float64
    sigmaVecHat::Array{Float64,1}; etaVec::Array{Float64,1}; zetaVec::Array{Float64,1}
    YHat::Array{Float64,2}; trYTY::Float64
    vbmf_dual_parameters() = new()
end

# (m, h)-interleaved vector <-> the two per-group vectors of src/vbmf_dual.jl:146-165
dual_split(v, M, H, H0) = (a = reshape(v, H, M); (vec(a[1:H0, :]), vec(a[H0+1:end, :])))
dual_join(v0, v1, M, H, H0) = vec(vcat(reshape(v0, H0, M), reshape(v1, H - H0, M)))

"src/vbmf_dual.jl:122-193"
function vbmf_dual_init(Y::Array{Float64,2}, H::Int, H0::Int; ca = 1.0, alpha0 = 1e-10, beta0 = 1e-10, cb = 1.0, gamma0 = 1e-10,
                        delta0 = 1e-10, sigma = 1.0, eta0 = 1e-10, zeta0 = 1e-10)
    H < H0 && error("H must be at least H0!")
    p = vbmf_dual_parameters(); L, M = size(Y); H1 = H - H0
    p.L, p.M, p.H, p.MH, p.H0, p.H1 = L, M, H, M * H, H0, H1
    p.AHat = randn(M, H); p.ATVecHat = reshape(permutedims(p.AHat), M * H); p.diagSigmaATVec = ones(M * H); p.SigmaA = zeros(H, H)
    p.A0Hat, p.A1Hat = p.AHat[:, 1:H0], p.AHat[:, H0+1:end]
    p.BHat = randn(L, H); p.SigmaB = zeros(H, H)
    p.CA0, p.CA1 = ca * ones(M * H0), ca * ones(M * H1); p.CA = dual_join(p.CA0, p.CA1, M, H, H0)
    p.alpha00 = p.alpha01 = alpha0; p.beta00 = p.beta01 = beta0; p.alpha0 = p.alpha1 = alpha0 + 0.5
    p.beta0, p.beta1 = beta0 * ones(M * H0), beta0 * ones(M * H1)
    p.alpha = [p.alpha0, p.alpha1]; p.beta = dual_join(p.beta0, p.beta1, M, H, H0)
    p.CB = cb * ones(H); p.gamma0, p.delta0, p.gamma, p.delta = gamma0, delta0, gamma0 + L / 2, delta0 * ones(H)
    p.sigmaHat, p.eta0, p.zeta0, p.eta, p.zeta = sigma, eta0, zeta0, eta0 + L * M / 2, zeta0
    p.sigmaVecHat, p.etaVec, p.zetaVec = sigma * ones(L), (eta0 + M / 2) * ones(L), zeta0 * ones(L)
    p.YHat = L * M <= (1 << 24) ? p.BHat * p.AHat' : Array{Float64}(undef, 0, 0)
    p.trYTY = sum(abs2, Y)
    return p
end

# vbls! of the sparse models over many bags with one fixed basis in ONE device call (examples/mil_util.jl:187-193, the classifiers of
# :393-416, :469-479, :497-521): the bags go side by side into one sparse context, every bag runs all niter iterations in one
# workgroup of one launch (vbmf_sparse_run_fixed_basis_batched).  al, b0: updateCA!'s (alpha_h, beta0_h) of every bag, H x nb.
function sparse_batch_run!(Ys::Vector{Matrix{Float64}}, ps, niter::Int, full_cov::Bool, al::Matrix{Float64}, b0::Matrix{Float64})
    nb = length(Ys)
    (nb >= 1 && length(ps) == nb) || error("vbls_batch!: one parameter set per bag")
    p0 = ps[1]
    H, L = p0.H, size(Ys[1], 1)
    H <= 64 || error("vbls_batch!: H = $H > 64; use vbls! per bag")
    for b in 1:nb
        Y, p = Ys[b], ps[b]
        size(Y, 1) == L || error("vbls_batch!: the bags have different L; use vbls! per bag")
        (size(Y, 2) >= 1 && (p.L, p.M, p.H) == (L, size(Y, 2), H)) || error("vbls_batch!: bag $b does not match its parameters")
        (p.BHat == p0.BHat && p.SigmaB == p0.SigmaB) ||
            error("vbls_batch!: bag $b does not share BHat and SigmaB with bag 1; use vbls! per bag")
    end
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    M = off[end]
    Yall = reduce(hcat, Ys)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, 1, 0xffffffff, 1, 0, 0, 0, 0, 0))   # VBMF_VARIANT_SPARSE_DIAG
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    eta = Float64[p.eta0 + p.L * p.M / 2 for p in ps]
    z0 = Float64[p.zeta0 for p in ps]
    sg = Float64[p.sigmaHat for p in ps]
    ca = reduce(vcat, [Vector{Float64}(p.CA) for p in ps])
    ze = Array{Float64}(undef, nb); be = Array{Float64}(undef, M * H); ds = similar(be); a = similar(be)
    SA = Array{Float64}(undef, H, H, nb)
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        hy = Ref(SparseHyper(1e-10, 1e-10, p0.gamma0, p0.delta0, p0.eta0, p0.zeta0))
        z, o = zeros(M * H), ones(M * H)
        chk(h[], ccall((:vbmf_sparse_set_state, libvbmf), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Float64, Float64, Ref{SparseHyper}, Ptr{Int64}, Int64, Int64),
            h[], z, o, o, o, p0.BHat, L, p0.SigmaB, ones(H), ones(H), 1.0, 0.0, hy, C_NULL, 0, 0))
        chk(h[], ccall((:vbmf_sparse_run_fixed_basis_batched, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            h[], nb, off, niter, full_cov, al, b0, eta, z0, sg, ca, ze, be, ds, SA, a))
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
    for b in 1:nb
        p, r = ps[b], off[b]*H+1:off[b+1]*H
        p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta = a[r], ds[r], ca[r], be[r]
        p.AHat = permutedims(reshape(p.ATVecHat, H, p.M))
        p.SigmaA = SA[:, :, b]
        p.sigmaHat, p.zeta = sg[b], ze[b]
        p.L * p.M <= (1 << 24) && (p.YHat = p.BHat * p.AHat')        # :201
    end
    return [p.AHat for p in ps]
end

"""
vbls! on the ARD-sparse model over many bags with one fixed basis in ONE device call (examples/mil_util.jl:187-190, :469-479 and
:393-416): does what `[vbls!(Y, p, niter; full_cov = full_cov) for (Y, p) in zip(Ys, ps)]` does.  No labels, H <= 64.
"""
function vbls_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_sparse_parameters}, niter::Int; full_cov::Bool = false)
    for (b, p) in enumerate(ps)
        (p.H1 == 0 && isempty(p.labels)) || error("vbls_batch!: bag $b has labels; use vbls! per bag")
    end
    al = Float64[p.alpha0 + 0.5 for h in 1:ps[1].H, p in ps]
    b0 = Float64[p.beta0 for h in 1:ps[1].H, p in ps]
    return sparse_batch_run!(Ys, ps, niter, full_cov, al, b0)
end

"""
vbls! on the two-group model over many bags with one fixed basis in ONE device call (examples/mil_util.jl:190-193, :514-521):
does what `[vbls!(Y, p, niter; full_cov = full_cov) for (Y, p) in zip(Ys, ps)]` does, the group views and posterior shapes included.
"""
function vbls_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_dual_parameters}, niter::Int; full_cov::Bool = false)
    H = ps[1].H
    al = Float64[h <= p.H0 ? p.alpha00 + 0.5 : p.alpha01 + 0.5 for h in 1:H, p in ps]
    b0 = Float64[h <= p.H0 ? p.beta00 : p.beta01 for h in 1:H, p in ps]
    out = sparse_batch_run!(Ys, ps, niter, full_cov, al, b0)
    for p in ps
        p.A0Hat, p.A1Hat = p.AHat[:, 1:p.H0], p.AHat[:, p.H0+1:end]
        p.CA0, p.CA1 = dual_split(p.CA, p.M, p.H, p.H0); p.beta0, p.beta1 = dual_split(p.beta, p.M, p.H, p.H0)
        p.alpha0, p.alpha1 = p.alpha00 + 0.5, p.alpha01 + 0.5                                 # src/vbmf_dual.jl:324-325
        p.alpha = [p.alpha0, p.alpha1]
    end
    return out
end

# ---- many fits in ONE device call: the restart loops of examples/mil_util.jl:124-145 (train) and :347-379 (train_dual) -------------
# Fit f works on bag bag_of[f] (1-based), so restarts share one upload; every fit's whole `while i <= niter && d > eps` loop runs in
# one workgroup of one launch (vbmf_sparse_fit_batched).  pri: 4 x nfits = alpha00, beta00, alpha01, beta01 per fit.
# With M0 (one entry per fit: the leading columns of its bag that are the negative instances) the call is vbmf_local_fit_batched: pri is
# 9 x nfits in vbmf_trial_get_priors' order, H0 splits the columns into prior groups 1 and 2 / 3, mask_H1 > 0 holds the last mask_H1
# columns of A at zero in the rows 1:M0.
# With rows (diag_var = true, examples/mil_util.jl:667: one noise precision per row of Y) the call is vbmf_rows_fit_batched: pri is
# 9 x nfits, M0 = nothing goes down as NULL (M0[f] = M_b: the two-group model), the fits start from sigmaVecHat and etaVec[1] and fill
# sigmaVecHat and zetaVec; sigmaHat and zeta stay as they were.
# With form = :split / :auto (or a slice_cols) the call is vbmf_ard_fit_batched_form in either noise model: pri is 9 x nfits, M0 = nothing
# goes down as NULL; :split spreads every fit over ceil(M_b / slice_cols) workgroups (slice_cols = 0: VBMF_FIT_SPLIT_COLS, else a
# multiple of 8), :auto picks per fit by its width.  :gram is the basic model's alone (vbmf_batch!).
function fit_batch_run!(fn::String, Ys::Vector{Matrix{Float64}}, ps, niter::Int, eps::Float64, full_cov::Bool, est_cb::Bool,
                        est_priors::Bool, H0::Int, pri::Matrix{Float64}, bag_of::Vector{Int}, variant::Int;
                        M0::Union{Nothing,Vector{Int64}} = nothing, mask_H1::Int = 0, rows::Bool = false,
                        form::Symbol = :stream, slice_cols::Int = 0)
    form == :gram && error("$fn: form = :gram: the ARD families have no Gram form; it serves the basic model's wide bags through vbmf_batch!")
    haskey(ARD_FIT_FORMS, form) || error("$fn: form = $form (:stream, :split or :auto)")
    (slice_cols == 0 || (slice_cols >= 8 && slice_cols % 8 == 0)) || error("$fn: slice_cols = $slice_cols (0, or a multiple of 8)")
    by_form = form != :stream || slice_cols != 0
    nb, nf = length(Ys), length(ps)
    (nb >= 1 && nf >= 1 && length(bag_of) == nf) || error("$fn: one bag_of entry per parameter set")
    niter >= 1 || error("$fn: niter must be >= 1")
    H, L = ps[1].H, size(Ys[1], 1)
    H <= 32 || error("$fn: H = $H > 32; run such fits one at a time")
    all(size(Y, 1) == L && size(Y, 2) >= 1 for Y in Ys) || error("$fn: the bags have different L; run such fits one at a time")
    for (f, p) in enumerate(ps)
        1 <= bag_of[f] <= nb || error("$fn: bag_of[$f] = $(bag_of[f]) outside 1..$nb")
        (p.L, p.M, p.H) == (L, size(Ys[bag_of[f]], 2), H) || error("$fn: fit $f does not match its bag")
        (full_cov || p.M >= 2) || error("$fn: fit $f works on a 1-column bag: the diagonal form needs M >= 2")
        (!rows || (length(p.sigmaVecHat) == L && length(p.etaVec) >= 1)) || error("$fn: fit $f: diag_var starts from sigmaVecHat (L) and etaVec")
    end
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    M = off[end]
    Yall = reduce(hcat, Ys)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, Int32(variant), 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    fb = Int64[b - 1 for b in bag_of]
    ga = Float64[p.gamma0 + p.L / 2 for p in ps]; d0 = Float64[p.delta0 for p in ps]
    eta = rows ? Float64[p.etaVec[1] for p in ps] : Float64[p.eta0 + p.L * p.M / 2 for p in ps]; z0 = Float64[p.zeta0 for p in ps]
    B = reduce(vcat, [vec(Matrix{Float64}(p.BHat)) for p in ps]); SB = reduce(vcat, [vec(Matrix{Float64}(p.SigmaB)) for p in ps])
    cb = reduce(vcat, [Vector{Float64}(p.CB) for p in ps])
    sg = rows ? reduce(vcat, [Vector{Float64}(p.sigmaVecHat) for p in ps]) : Float64[p.sigmaHat for p in ps]
    ca = reduce(vcat, [Vector{Float64}(p.CA) for p in ps])
    n = length(ca)
    dl = Array{Float64}(undef, nf * H); ze = Array{Float64}(undef, rows ? nf * L : nf); be = Array{Float64}(undef, n); ds = similar(be); a = similar(be)
    SA = Array{Float64}(undef, H, H, nf)
    it = zeros(Int64, nf); dlast = Array{Float64}(undef, nf); st = zeros(Int64, nf)
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        if by_form
        chk(h[], ccall((:vbmf_ard_fit_batched_form, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Float64, Cint, Cint, Cint, Int64, Ptr{Int64}, Int64, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64},
             Ptr{Int64}, Ptr{Float64}, Cint, Int64, Int64, Ptr{Int64}),
            h[], nb, off, nf, fb, niter, eps, full_cov, est_cb, est_priors, H0, M0 === nothing ? C_NULL : M0, mask_H1, ga, d0, eta, z0,
            pri, B, SB, cb, sg, ca, dl, ze, be, ds, SA, a, it, dlast, st, C_NULL, rows, ARD_FIT_FORMS[form], slice_cols, C_NULL))
        elseif rows
        chk(h[], ccall((:vbmf_rows_fit_batched, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Float64, Cint, Cint, Cint, Int64, Ptr{Int64}, Int64, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64},
             Ptr{Int64}, Ptr{Float64}),
            h[], nb, off, nf, fb, niter, eps, full_cov, est_cb, est_priors, H0, M0 === nothing ? C_NULL : M0, mask_H1, ga, d0, eta, z0,
            pri, B, SB, cb, sg, ca, dl, ze, be, ds, SA, a, it, dlast, st, C_NULL))
        elseif M0 === nothing
        chk(h[], ccall((:vbmf_sparse_fit_batched, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Float64, Cint, Cint, Cint, Int64, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64},
             Ptr{Float64}),
            h[], nb, off, nf, fb, niter, eps, full_cov, est_cb, est_priors, H0, ga, d0, eta, z0, pri, B, SB, cb, sg, ca, dl, ze, be, ds,
            SA, a, it, dlast, st, C_NULL))
        else
        chk(h[], ccall((:vbmf_local_fit_batched, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Float64, Cint, Cint, Cint, Int64, Ptr{Int64}, Int64, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64},
             Ptr{Int64}, Ptr{Float64}),
            h[], nb, off, nf, fb, niter, eps, full_cov, est_cb, est_priors, H0, M0, mask_H1, ga, d0, eta, z0, pri, B, SB, cb, sg, ca, dl,
            ze, be, ds, SA, a, it, dlast, st, C_NULL))
        end
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
    s = 0
    for (f, p) in enumerate(ps)
        r = s+1:s+p.M*H
        s += p.M * H
        p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta = a[r], ds[r], ca[r], be[r]
        p.AHat = permutedims(reshape(p.ATVecHat, H, p.M))
        p.SigmaA = SA[:, :, f]
        p.BHat = reshape(B[(f-1)*L*H+1:f*L*H], L, H)
        p.SigmaB = reshape(SB[(f-1)*H*H+1:f*H*H], H, H)
        p.CB = cb[(f-1)*H+1:f*H]
        est_cb && (p.delta = dl[(f-1)*H+1:f*H])
        if rows
            p.sigmaVecHat, p.zetaVec = sg[(f-1)*L+1:f*L], ze[(f-1)*L+1:f*L]
        else
            p.sigmaHat, p.zeta = sg[f], ze[f]
        end
        p.L * p.M <= (1 << 24) && (p.YHat = p.BHat * p.AHat')
    end
    return dlast, it, st
end

"""
vbmf_sparse! for many independent fits in ONE device call (the restart loop of examples/mil_util.jl:124-145): does what
`[vbmf_sparse!(Ys[bag_of[f]], ps[f], niter; eps = eps, full_cov = full_cov) for f in 1:length(ps)]` does and returns
(d, sweeps run, status) per fit; status 1 = the fit met a non-finite precision or a bad pivot and stopped.  No labels, H <= 32.
diag_var = true: one noise precision per row of Y (examples/mil_util.jl:667), through vbmf_rows_fit_batched.
form = :split spreads every fit over ceil(M_b / slice_cols) workgroups, two launches per sweep (the form for a few wide fits;
slice_cols = 0: VBMF_FIT_SPLIT_COLS), :auto picks per fit by its width, :stream (the default) is one workgroup per fit
(vbmf_ard_fit_batched_form); the same iteration in another summation order.
"""
function vbmf_sparse_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_sparse_parameters}, niter::Int; eps::Float64 = 1e-6,
                            full_cov::Bool = false, est_cb::Bool = true, bag_of::Vector{Int} = collect(1:length(ps)),
                            diag_var::Bool = false, form::Symbol = :stream, slice_cols::Int = 0)
    for (f, p) in enumerate(ps)
        (p.H1 == 0 && isempty(p.labels)) || error("vbmf_sparse_batch!: fit $f has labels; use vbmf_sparse! per fit")
    end
    if diag_var || form != :stream || slice_cols != 0               # the nine-slot entries
        pri9 = Float64[(p.alpha0, p.beta0, p.alpha0, p.beta0, p.alpha0, p.beta0, 0.0, 0.0, 0.0)[k] for k in 1:9, p in ps]
        return fit_batch_run!("vbmf_sparse_batch!", Ys, ps, niter, eps, full_cov, est_cb, false, ps[1].H, pri9, bag_of, 1; rows = diag_var,
                              form = form, slice_cols = slice_cols)
    end
    pri = Float64[(p.alpha0, p.beta0, p.alpha0, p.beta0)[k] for k in 1:4, p in ps]
    return fit_batch_run!("vbmf_sparse_batch!", Ys, ps, niter, eps, full_cov, est_cb, false, ps[1].H, pri, bag_of, 1)
end

"""
vbmf_dual! for many independent fits in ONE device call (the restart loop of examples/mil_util.jl:347-379): see vbmf_sparse_batch!;
all fits share one H0; est_priors refits (alpha00, beta00, alpha01, beta01) every sweep (src/vbmf_dual.jl:393-434).
"""
function vbmf_dual_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_dual_parameters}, niter::Int; eps::Float64 = 1e-6,
                          full_cov::Bool = false, est_cb::Bool = true, est_priors::Bool = true,
                          bag_of::Vector{Int} = collect(1:length(ps)), diag_var::Bool = false, form::Symbol = :stream,
                          slice_cols::Int = 0)
    H0 = ps[1].H0
    all(p.H0 == H0 for p in ps) || error("vbmf_dual_batch!: one H0 per call")
    if diag_var || form != :stream || slice_cols != 0               # the nine-slot entries: group 3 is empty, slots 7, 8 the posterior shapes
        pri9 = Float64[(p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha01, p.beta01, 0.0, 0.0, 0.0)[k] for k in 1:9, p in ps]
        out = fit_batch_run!("vbmf_dual_batch!", Ys, ps, niter, eps, full_cov, est_cb, est_priors, H0, pri9, bag_of, 3; rows = diag_var,
                             form = form, slice_cols = slice_cols)
        for (f, p) in enumerate(ps)
            p.A0Hat, p.A1Hat = p.AHat[:, 1:p.H0], p.AHat[:, p.H0+1:end]
            p.CA0, p.CA1 = dual_split(p.CA, p.M, p.H, p.H0); p.beta0, p.beta1 = dual_split(p.beta, p.M, p.H, p.H0)
            p.alpha00, p.beta00, p.alpha01, p.beta01 = pri9[1, f], pri9[2, f], pri9[3, f], pri9[4, f]
            p.alpha0, p.alpha1 = pri9[7, f], pri9[8, f]
            p.alpha = [p.alpha0, p.alpha1]
        end
        return out
    end
    pri = Float64[(p.alpha00, p.beta00, p.alpha01, p.beta01)[k] for k in 1:4, p in ps]
    out = fit_batch_run!("vbmf_dual_batch!", Ys, ps, niter, eps, full_cov, est_cb, est_priors, H0, pri, bag_of, 3)
    for (f, p) in enumerate(ps)
        p.A0Hat, p.A1Hat = p.AHat[:, 1:p.H0], p.AHat[:, p.H0+1:end]
        p.CA0, p.CA1 = dual_split(p.CA, p.M, p.H, p.H0); p.beta0, p.beta1 = dual_split(p.beta, p.M, p.H, p.H0)
        # the posterior shapes as the last updateCA! left them (src/vbmf_dual.jl:324-325): the hyper-prior that sweep started from + 1/2
        p.alpha0 = est_priors && out[2][f] > 0 ? p.CA0[1] * p.beta0[1] : p.alpha00 + 0.5
        p.alpha1 = est_priors && out[2][f] > 0 && !isempty(p.CA1) ? p.CA1[1] * p.beta1[1] : p.alpha01 + 0.5
        p.alpha00, p.beta00, p.alpha01, p.beta01 = pri[1, f], pri[2, f], pri[3, f], pri[4, f]
        p.alpha = [p.alpha0, p.alpha1]
    end
    return out
end

# ---- scoring many bags: what classify (examples/mil_util.jl:453-535) compares once vbls! has run ------------------------------
# The bags go side by side into one context with the shared basis as its state; `body(h, off, M)` makes the scoring call.
function with_scoring_ctx(body, Ys::Vector{Matrix{Float64}}, ps, variant::Int, fn::String)
    nb = length(Ys)
    (nb >= 1 && length(ps) == nb) || error("$fn: one parameter set per bag")
    p0 = ps[1]
    H, L = p0.H, size(Ys[1], 1)
    for b in 1:nb
        Y, p = Ys[b], ps[b]
        size(Y, 1) == L || error("$fn: the bags have different L")
        (size(Y, 2) >= 1 && (p.L, p.M, p.H) == (L, size(Y, 2), H)) || error("$fn: bag $b does not match its parameters")
        (p.BHat == p0.BHat && p.SigmaB == p0.SigmaB && p.CB == p0.CB) || error("$fn: bag $b does not share BHat, SigmaB and CB with bag 1")
    end
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    M = off[end]
    Yall = reduce(hcat, Ys)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, variant, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        if variant == 0
            ca0 = [p0.CA[i, i] for i in 1:H]; cb0 = [p0.CB[i, i] for i in 1:H]
            zA = zeros(M, H)
            chk(h[], ccall((:vbmf_set_state, libvbmf), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Float64, Ptr{Int64}, Int64, Int64),
                h[], zA, M, p0.BHat, L, p0.SigmaA, p0.SigmaB, ca0, cb0, p0.sigma2, C_NULL, 0, 0))
        else
            for (b, p) in enumerate(ps)
                (p.delta == p0.delta && p.gamma0 == p0.gamma0 && p.delta0 == p0.delta0) ||
                    error("$fn: bag $b does not share delta, gamma0 and delta0 with bag 1")
            end
            hy = Ref(SparseHyper(1e-10, 1e-10, p0.gamma0, p0.delta0, p0.eta0, p0.zeta0))
            z, o = zeros(M * H), ones(M * H)
            chk(h[], ccall((:vbmf_sparse_set_state, libvbmf), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Float64, Float64, Ref{SparseHyper}, Ptr{Int64}, Int64, Int64),
                h[], z, o, o, o, p0.BHat, L, p0.SigmaB, p0.CB, p0.delta, 1.0, 1.0, hy, C_NULL, 0, 0))
        end
        return body(h[], off, M)
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
end

function residual_batch_impl(Ys::Vector{Matrix{Float64}}, ps, variant::Int)
    nb = length(Ys)
    A = reduce(vcat, [Matrix{Float64}(p.AHat) for p in ps])
    r2 = Array{Float64}(undef, nb)
    with_scoring_ctx(Ys, ps, variant, "residual_batch") do h, off, M
        chk(h, ccall((:vbmf_bag_residuals, libvbmf), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}),
                     h, nb, off, A, M, r2))
    end
    return sqrt.(r2)
end

"""
norm(Y - BHat*AHat') of every bag (examples/mil_util.jl:483-484, :523-524) in ONE device call, formed entry by entry in fp64 on the
device (vbmf_bag_residuals): `ps` are the parameter sets a `vbls_batch!` filled.
"""
residual_batch(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_parameters}) = residual_batch_impl(Ys, ps, 0)
residual_batch(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_sparse_parameters}) = residual_batch_impl(Ys, ps, 1)
residual_batch(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_dual_parameters}) = residual_batch_impl(Ys, ps, 1)

# apri, bpri, apost: per column of A and bag (H x nb) the ARD hyper-prior (shape, rate) and the posterior shape; trim < 0: lowerBound
function bound_batch_impl(Ys::Vector{Matrix{Float64}}, ps, trim::Float64, grouped::Bool, apri::Matrix{Float64}, bpri::Matrix{Float64},
                          apost::Matrix{Float64})
    nb = length(Ys)
    H = ps[1].H
    H <= 64 || error("lowerBound_batch: H = $H > 64")
    a = reduce(vcat, [Vector{Float64}(p.ATVecHat) for p in ps]); ds = reduce(vcat, [Vector{Float64}(p.diagSigmaATVec) for p in ps])
    ca = reduce(vcat, [Vector{Float64}(p.CA) for p in ps]); be = reduce(vcat, [Vector{Float64}(p.beta) for p in ps])
    SA = Array{Float64}(undef, H, H, nb)
    for b in 1:nb
        SA[:, :, b] = ps[b].SigmaA
    end
    sg = Float64[p.sigmaHat for p in ps]; ze = Float64[p.zeta for p in ps]; et = Float64[p.eta for p in ps]
    e0 = Float64[p.eta0 for p in ps]; z0 = Float64[p.zeta0 for p in ps]
    lb = Array{Float64}(undef, nb)
    with_scoring_ctx(Ys, ps, 1, "lowerBound_batch") do h, off, M
        chk(h, ccall((:vbmf_sparse_lower_bound_batched, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Cint, Float64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}),
            h, nb, off, 1, trim, grouped, a, ds, ca, be, SA, sg, ze, et, e0, z0, apri, bpri, apost, lb, C_NULL))
    end
    return lb
end

function bound_batch(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_sparse_parameters}, trim::Float64)
    H = ps[1].H
    for (b, p) in enumerate(ps)
        (p.H1 == 0 && isempty(p.labels)) || error("lowerBound_batch: bag $b has labels; use lowerBound per bag")
    end
    apri = Float64[p.alpha0 for h in 1:H, p in ps]; bpri = Float64[p.beta0 for h in 1:H, p in ps]
    apost = Float64[p.alpha for h in 1:H, p in ps]
    return bound_batch_impl(Ys, ps, trim, false, apri, bpri, apost)
end

function bound_batch(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_dual_parameters}, trim::Float64)
    H = ps[1].H
    apri = Float64[h <= p.H0 ? p.alpha00 : p.alpha01 for h in 1:H, p in ps]
    bpri = Float64[h <= p.H0 ? p.beta00 : p.beta01 for h in 1:H, p in ps]
    apost = Float64[h <= p.H0 ? p.alpha0 : p.alpha1 for h in 1:H, p in ps]
    return bound_batch_impl(Ys, ps, trim, true, apri, bpri, apost)
end

"""
`[lowerBound(Y, p) for (Y, p) in zip(Ys, ps)]` in ONE device call (src/vbmf_sparse.jl:435-471, src/vbmf_dual.jl:556-599;
examples/mil_util.jl:504): one model type, one fixed basis, no labels, H <= 64 (vbmf_sparse_lower_bound_batched).
"""
lowerBound_batch(Ys::Vector{Matrix{Float64}}, ps) = bound_batch(Ys, ps, -1.0)

"`[lowerBoundTrimmed(Y, p, trim) for (Y, p) in zip(Ys, ps)]` in ONE device call (src/vbmf_sparse.jl:478-489, examples/mil_util.jl:505)"
function lowerBoundTrimmed_batch(Ys::Vector{Matrix{Float64}}, ps, trim = 1e-1)
    trim >= 0 || error("lowerBoundTrimmed_batch: trim must be >= 0")
    return bound_batch(Ys, ps, Float64(trim))
end

# ---- least squares against a caller's basis: ols / rls (examples/mil_util.jl:159-171) over many bags ----------------------------
# The bags go side by side into one basic context, which supplies only Y: the basis is an argument of the call, with its own H.
# Returns (X: H x sum(M_b), the squared residual norms, the column offsets).
function bag_least_squares(Ys::Vector{Matrix{Float64}}, B::Matrix{Float64}, lam::Float64, fn::String)
    nb = length(Ys)
    nb >= 1 || error("$fn: no bags")
    L, H = size(B)
    1 <= H <= 64 || error("$fn: H = $H (built for 1 <= H <= 64)")
    (isfinite(lam) && lam >= 0) || error("$fn: lam must be finite and >= 0")
    for (b, Y) in enumerate(Ys)
        (size(Y, 1) == L && size(Y, 2) >= 1) || error("$fn: bag $b is not L x M_b with L = size(B, 1) = $L and M_b >= 1")
    end
    off = Int64[0; cumsum([Int64(size(Y, 2)) for Y in Ys])]
    M = off[end]
    Yall = reduce(hcat, Ys)
    X = Array{Float64}(undef, H, M)
    r2 = Array{Float64}(undef, nb)
    opts = Ref(VbmfOpts(Int32(sizeof(VbmfOpts)), 0, y_dtype(), 0, 0, 0xffffffff, 1, 0, 0, 0, 0, 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(Ptr{Cvoid}(C_NULL), ccall((:vbmf_create, libvbmf), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ref{VbmfOpts}), h, L, M, H, opts))
    try
        chk(h[], ccall((:vbmf_set_Y, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h[], Yall, L))
        chk(h[], ccall((:vbmf_bag_least_squares, libvbmf), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Float64}, Int64, Ptr{Float64}),
            h[], nb, off, B, L, H, lam, X, H, r2))
    finally
        ccall((:vbmf_destroy, libvbmf), Cint, (Ptr{Cvoid},), h[])
    end
    return X, r2, off
end

"`[ols(Y, B) for Y in Ys]` = inv(B'B)*B'*Y per bag (examples/mil_util.jl:159-161) in ONE device call, fp64 (vbmf_bag_least_squares); H <= 64"
function ols_batch(Ys::Vector{Matrix{Float64}}, B::Matrix{Float64})
    X, _, off = bag_least_squares(Ys, B, 0.0, "ols_batch")
    return [X[:, off[b]+1:off[b+1]] for b in 1:length(Ys)]
end

"`[rls(Y, B, lam) for Y in Ys]` = inv(B'B + lam*I)*B'*Y per bag (examples/mil_util.jl:168-171) in ONE device call"
function rls_batch(Ys::Vector{Matrix{Float64}}, B::Matrix{Float64}, lam::Float64)
    X, _, off = bag_least_squares(Ys, B, lam, "rls_batch")
    return [X[:, off[b]+1:off[b+1]] for b in 1:length(Ys)]
end

"norm(Y_b - B*X_b) with X_b the ols (lam = 0) / rls estimate of every bag (examples/mil_util.jl:483-484), from the pass that forms X_b"
function ls_residual_batch(Ys::Vector{Matrix{Float64}}, B::Matrix{Float64}, lam::Float64 = 0.0)
    _, r2, _ = bag_least_squares(Ys, B, lam, "ls_residual_batch")
    return sqrt.(r2)
end

"""
    bag_least_squares_jobs(ctx, col_off, bases, lams, job_bag, job_basis)

test_classification (examples/mil_util.jl:558-587) of every fold of validate_with_cvs (examples/mil_util.jl:627-648) in ONE device call
(vbmf_bag_least_squares_jobs): `ctx` holds every bag of the data set side by side (bag b = columns col_off[b]+1 .. col_off[b+1], col_off
0-based offsets), `bases[k]` is L x H_k with H_k <= 64 and `lams[k]` its lambda (0 = ols, > 0 = rls), job j scores bag `job_bag[j]`
against basis `job_basis[j]` (both 1-based).  Returns (Xs, r2, status): Xs[j] = inv(B'B + lam I) B' Y_b (H_k x M_b), r2[j] =
norm(Y_b - B Xs[j])^2, status[k] = 1 for a basis whose B'B + lam I is not positive definite (its jobs are NaN; the others are computed).
Every job is bit for bit what vbmf_bag_least_squares gives for that bag with that basis.
"""
function bag_least_squares_jobs(ctx::Ptr{Cvoid}, col_off::Vector{Int64}, bases::Vector{Matrix{Float64}}, lams::Vector{Float64},
                                job_bag::AbstractVector{<:Integer}, job_basis::AbstractVector{<:Integer})
    nb, nk, nj = length(col_off) - 1, length(bases), length(job_bag)
    (nk >= 1 && length(lams) == nk) || error("bag_least_squares_jobs: one lambda per basis, at least one basis")
    (nj >= 1 && length(job_basis) == nj) || error("bag_least_squares_jobs: job_bag and job_basis must have one entry per job, at least one")
    L = size(bases[1], 1)
    all(B -> size(B, 1) == L && 1 <= size(B, 2) <= 64, bases) || error("bag_least_squares_jobs: every basis must be L x H with 1 <= H <= 64")
    all(j -> 1 <= job_bag[j] <= nb && 1 <= job_basis[j] <= nk, 1:nj) || error("bag_least_squares_jobs: a job names a bag or a basis that is not there")
    Hs = Int64[size(B, 2) for B in bases]
    Ball = reduce(vcat, [vec(B) for B in bases])
    jb, jk = Int64[b - 1 for b in job_bag], Int64[k - 1 for k in job_basis]
    shapes = [(Hs[jk[j]+1], col_off[jb[j]+2] - col_off[jb[j]+1]) for j in 1:nj]
    xoff = Int64[0; cumsum([h * m for (h, m) in shapes])]
    X = Array{Float64}(undef, xoff[end])
    r2 = Array{Float64}(undef, nj)
    status = Array{Int64}(undef, nk)
    chk(ctx, ccall((:vbmf_bag_least_squares_jobs, libvbmf), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Int64}),
        ctx, nb, col_off, nk, Hs, Ball, lams, nj, jb, jk, X, r2, status))
    Xs = [reshape(X[xoff[j]+1:xoff[j+1]], shapes[j]) for j in 1:nj]
    return Xs, r2, status
end

"""
    sparse_fixed_basis_jobs(ctx, col_off, H, BHat, SigmaB, alpha, beta0, eta0, zeta0, sigma0, ca0, job_bag, job_model, niter; full_cov)

vbls! of the ARD families (examples/mil_util.jl:187-197) for a list of (bag, model) jobs in ONE device call
(vbmf_sparse_fixed_basis_jobs) -- the "dual" classifier of examples/mil_util.jl:515-530 for every fold at once.  `ctx` holds every bag
of the data set side by side (col_off: 0-based offsets); only its Y is read.  Model k: `BHat[k]` (L x H, H <= 32), `SigmaB[k]` (H x H),
columns k of `alpha` and `beta0` (H x nmodels: updateCA!'s posterior shape and prior rate per column of A), `eta0[k]`, `zeta0[k]` and
the start values `sigma0[k]`, `ca0[k]`.  Job j runs bag `job_bag[j]` against model `job_model[j]` (both 1-based).  Returns a named
tuple: r2, sigmaHat, zeta, status (per job; status 1 = a failed job, NaN in its outputs), SigmaA (H x H x njobs), and ATVecHat,
diagSigmaATVec, CA, beta as one vec(A')-ordered vector per job.
"""
function sparse_fixed_basis_jobs(ctx::Ptr{Cvoid}, col_off::Vector{Int64}, H::Int, BHat::Vector{Matrix{Float64}},
                                 SigmaB::Vector{Matrix{Float64}}, alpha::Matrix{Float64}, beta0::Matrix{Float64}, eta0::Vector{Float64},
                                 zeta0::Vector{Float64}, sigma0::Vector{Float64}, ca0::Vector{Float64},
                                 job_bag::AbstractVector{<:Integer}, job_model::AbstractVector{<:Integer}, niter::Int;
                                 full_cov::Bool = false)
    nb, nk, nj = length(col_off) - 1, length(BHat), length(job_bag)
    (nk >= 1 && length(SigmaB) == nk && size(alpha) == (H, nk) && size(beta0) == (H, nk) && length(eta0) == nk && length(zeta0) == nk &&
     length(sigma0) == nk && length(ca0) == nk) || error("sparse_fixed_basis_jobs: every per-model input needs one entry per model, at least one model")
    (nj >= 1 && length(job_model) == nj) || error("sparse_fixed_basis_jobs: job_bag and job_model must have one entry per job, at least one")
    L = size(BHat[1], 1)
    all(k -> size(BHat[k]) == (L, H) && size(SigmaB[k]) == (H, H), 1:nk) || error("sparse_fixed_basis_jobs: every model needs BHat L x H and SigmaB H x H")
    all(j -> 1 <= job_bag[j] <= nb && 1 <= job_model[j] <= nk, 1:nj) || error("sparse_fixed_basis_jobs: a job names a bag or a model that is not there")
    Ball = reduce(vcat, [vec(B) for B in BHat])
    SBall = reduce(vcat, [vec(S) for S in SigmaB])
    jb, jk = Int64[b - 1 for b in job_bag], Int64[k - 1 for k in job_model]
    off = Int64[0; cumsum([H * (col_off[b+2] - col_off[b+1]) for b in jb])]
    r2, sg, zeta = Array{Float64}(undef, nj), Array{Float64}(undef, nj), Array{Float64}(undef, nj)
    A, dS = Array{Float64}(undef, off[end]), Array{Float64}(undef, off[end])
    CA, beta = Array{Float64}(undef, off[end]), Array{Float64}(undef, off[end])
    SA = Array{Float64}(undef, H, H, nj)
    status = Array{Int64}(undef, nj)
    chk(ctx, ccall((:vbmf_sparse_fixed_basis_jobs, libvbmf), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Int64, Cint, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        ctx, nb, col_off, H, niter, Cint(full_cov), nk, Ball, SBall, alpha, beta0, eta0, zeta0, sigma0, ca0, nj, jb, jk, r2, A, dS, CA, beta,
        SA, sg, zeta, status))
    blocks(v) = [v[off[j]+1:off[j+1]] for j in 1:nj]
    return (r2 = r2, sigmaHat = sg, zeta = zeta, status = status, SigmaA = SA, ATVecHat = blocks(A), diagSigmaATVec = blocks(dS),
            CA = blocks(CA), beta = blocks(beta))
end

"""
    fixed_basis_jobs(ctx, col_off, model_H, BHat, SigmaB, sigma2_0, ca0, job_bag, job_model, niter)

vbls! of the basic model (examples/mil_util.jl:182-185) for a list of (bag, model) jobs in ONE device call (vbmf_fixed_basis_jobs) --
the "vbls" classifier of examples/mil_util.jl:469-479 for every fold at once.  `ctx` holds every bag of the data set side by side
(col_off: 0-based offsets); only its Y is read.  Model k: its own rank `model_H[k]` <= 32, `BHat[k]` (L x H_k), `SigmaB[k]` (H_k x H_k)
and the start values `sigma2_0[k]`, `ca0[k]` (CA = ca0 I).  Job j runs bag `job_bag[j]` against model `job_model[j]` (both 1-based).
Returns a named tuple: r2, sigma2, status (per job; status 1 = a failed job, NaN in its outputs), and per job AHat (M_b x H_k), SigmaA
(H_k x H_k) and CA_diag (H_k).
"""
function fixed_basis_jobs(ctx::Ptr{Cvoid}, col_off::Vector{Int64}, model_H::Vector{Int64}, BHat::Vector{Matrix{Float64}},
                          SigmaB::Vector{Matrix{Float64}}, sigma2_0::Vector{Float64}, ca0::Vector{Float64},
                          job_bag::AbstractVector{<:Integer}, job_model::AbstractVector{<:Integer}, niter::Int)
    nb, nk, nj = length(col_off) - 1, length(BHat), length(job_bag)
    (nk >= 1 && length(model_H) == nk && length(SigmaB) == nk && length(sigma2_0) == nk && length(ca0) == nk) ||
        error("fixed_basis_jobs: every per-model input needs one entry per model, at least one model")
    (nj >= 1 && length(job_model) == nj) || error("fixed_basis_jobs: job_bag and job_model must have one entry per job, at least one")
    L = size(BHat[1], 1)
    all(k -> size(BHat[k]) == (L, model_H[k]) && size(SigmaB[k]) == (model_H[k], model_H[k]), 1:nk) ||
        error("fixed_basis_jobs: every model needs BHat L x H_k and SigmaB H_k x H_k")
    all(j -> 1 <= job_bag[j] <= nb && 1 <= job_model[j] <= nk, 1:nj) || error("fixed_basis_jobs: a job names a bag or a model that is not there")
    Ball = reduce(vcat, [vec(B) for B in BHat])
    SBall = reduce(vcat, [vec(S) for S in SigmaB])
    jb, jk = Int64[b - 1 for b in job_bag], Int64[k - 1 for k in job_model]
    Hj = Int64[model_H[k] for k in job_model]
    Mj = Int64[col_off[b+1] - col_off[b] for b in job_bag]
    off, soff, hoff = Int64[0; cumsum(Mj .* Hj)], Int64[0; cumsum(Hj .* Hj)], Int64[0; cumsum(Hj)]
    r2, sg = Array{Float64}(undef, nj), Array{Float64}(undef, nj)
    A, SA, CA = Array{Float64}(undef, off[end]), Array{Float64}(undef, soff[end]), Array{Float64}(undef, hoff[end])
    status = Array{Int64}(undef, nj)
    chk(ctx, ccall((:vbmf_fixed_basis_jobs, libvbmf), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        ctx, nb, col_off, niter, nk, model_H, Ball, SBall, sigma2_0, ca0, nj, jb, jk, r2, A, SA, CA, sg, status))
    return (r2 = r2, sigma2 = sg, status = status,
            AHat = [reshape(A[off[j]+1:off[j+1]], Int(Mj[j]), Int(Hj[j])) for j in 1:nj],
            SigmaA = [reshape(SA[soff[j]+1:soff[j+1]], Int(Hj[j]), Int(Hj[j])) for j in 1:nj],
            CA_diag = [CA[hoff[j]+1:hoff[j+1]] for j in 1:nj])
end

"""
    sparse_scored_jobs(ctx, col_off, BHat, SigmaB, CB, delta, gamma, gamma0, delta0, a_pri, b_pri, a_post, eta0, zeta0, sigma0, ca0,
                       job_bag, job_model, job_full_cov, job_trim, niter; clamp, grouped)

factorize_bag (examples/mil_util.jl:393-416) and its scores for a list of (bag, model) jobs in ONE device call
(vbmf_sparse_scored_jobs) -- the "lower_bound" and "min_err" classifiers of examples/mil_util.jl:493-514 for every fold at once.  `ctx`
holds every bag side by side (col_off: 0-based offsets); only its Y is read.  Model k has its own rank H_k = size(BHat[k], 2) <= 32:
`BHat[k]` (L x H_k), `SigmaB[k]` (H_k x H_k), `CB[k]`, `delta[k]`, `a_pri[k]`, `b_pri[k]`, `a_post[k]` (H_k each), and the scalars
`gamma[k]`, `gamma0[k]`, `delta0[k]`, `eta0[k]`, `zeta0[k]`, `sigma0[k]`, `ca0[k]`.  Job j runs bag `job_bag[j]` against model
`job_model[j]` (both 1-based) in the full_cov form where `job_full_cov[j]`, and is scored with lowerBound (`job_trim[j] < 0`) or
lowerBoundTrimmed(`job_trim[j]`).  Returns a named tuple: lb, r2, sigmaHat, zeta, status (per job; status 1 = a failed job, NaN in its
outputs), and SigmaA, ATVecHat, diagSigmaATVec, CA, beta as one array per job.
"""
function sparse_scored_jobs(ctx::Ptr{Cvoid}, col_off::Vector{Int64}, BHat::Vector{Matrix{Float64}}, SigmaB::Vector{Matrix{Float64}},
                            CB::Vector{Vector{Float64}}, delta::Vector{Vector{Float64}}, gamma::Vector{Float64}, gamma0::Vector{Float64},
                            delta0::Vector{Float64}, a_pri::Vector{Vector{Float64}}, b_pri::Vector{Vector{Float64}},
                            a_post::Vector{Vector{Float64}}, eta0::Vector{Float64}, zeta0::Vector{Float64}, sigma0::Vector{Float64},
                            ca0::Vector{Float64}, job_bag::AbstractVector{<:Integer}, job_model::AbstractVector{<:Integer},
                            job_full_cov::AbstractVector{Bool}, job_trim::Vector{Float64}, niter::Int; clamp::Bool = true,
                            grouped::Bool = false)
    nb, nk, nj = length(col_off) - 1, length(BHat), length(job_bag)
    (nk >= 1 && all(v -> length(v) == nk, (SigmaB, CB, delta, gamma, gamma0, delta0, a_pri, b_pri, a_post, eta0, zeta0, sigma0, ca0))) ||
        error("sparse_scored_jobs: every per-model input needs one entry per model, at least one model")
    (nj >= 1 && length(job_model) == nj && length(job_full_cov) == nj && length(job_trim) == nj) ||
        error("sparse_scored_jobs: job_bag, job_model, job_full_cov and job_trim must have one entry per job, at least one")
    L = size(BHat[1], 1)
    Hs = Int64[size(B, 2) for B in BHat]
    all(k -> size(BHat[k], 1) == L && size(SigmaB[k]) == (Hs[k], Hs[k]) &&
             all(v -> length(v[k]) == Hs[k], (CB, delta, a_pri, b_pri, a_post)), 1:nk) ||
        error("sparse_scored_jobs: every model needs BHat L x H, SigmaB H x H and CB, delta, a_pri, b_pri, a_post of length H")
    all(j -> 1 <= job_bag[j] <= nb && 1 <= job_model[j] <= nk, 1:nj) || error("sparse_scored_jobs: a job names a bag or a model that is not there")
    cat1(vs) = reduce(vcat, [vec(v) for v in vs])
    jb, jk = Int64[b - 1 for b in job_bag], Int64[k - 1 for k in job_model]
    jf = Int64[f ? 1 : 0 for f in job_full_cov]
    Hj = Int64[Hs[k] for k in job_model]
    off = Int64[0; cumsum([Hj[j] * (col_off[jb[j]+2] - col_off[jb[j]+1]) for j in 1:nj])]
    soff = Int64[0; cumsum(Hj .* Hj)]
    lb, r2 = Array{Float64}(undef, nj), Array{Float64}(undef, nj)
    sg, zeta = Array{Float64}(undef, nj), Array{Float64}(undef, nj)
    A, dS = Array{Float64}(undef, off[end]), Array{Float64}(undef, off[end])
    CA, beta = Array{Float64}(undef, off[end]), Array{Float64}(undef, off[end])
    SA = Array{Float64}(undef, soff[end])
    status = Array{Int64}(undef, nj)
    chk(ctx, ccall((:vbmf_sparse_scored_jobs, libvbmf), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Cint, Cint, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        ctx, nb, col_off, niter, Cint(clamp), Cint(grouped), nk, Hs, cat1(BHat), cat1(SigmaB), cat1(CB), cat1(delta), gamma, gamma0, delta0,
        cat1(a_pri), cat1(b_pri), cat1(a_post), eta0, zeta0, sigma0, ca0, nj, jb, jk, jf, job_trim, lb, r2, A, dS, CA, beta, SA, sg, zeta,
        status))
    blocks(v) = [v[off[j]+1:off[j+1]] for j in 1:nj]
    return (lb = lb, r2 = r2, sigmaHat = sg, zeta = zeta, status = status,
            SigmaA = [reshape(SA[soff[j]+1:soff[j+1]], Hj[j], Hj[j]) for j in 1:nj], ATVecHat = blocks(A),
            diagSigmaATVec = blocks(dS), CA = blocks(CA), beta = blocks(beta))
end

"vbmf_dual! -- src/vbmf_dual.jl:455-530 (returns d); est_priors: the hyper-prior fits of :393-434 run on the device"
function vbmf_dual!(Y::Array{Float64,2}, p::vbmf_dual_parameters, niter::Int; eps::Float64 = 1e-6, diag_var::Bool = false,
                    full_cov::Bool = false, logdir = "", desc = "", verb = false, est_priors = true, est_cb::Bool = true)
    full_cov && p.H > 256 && error("full_cov=true is built for H <= 256 (either noise model)")
    logdir == "" || error("trajectory logging lives in the Python host (data_manip.py)")
    c = sparse_ctx_for(Y, p.H, diag_var; variant = diag_var ? 5 : 3)          # VBMF_VARIANT_DUAL_DIAGVAR / _DUAL_DIAG
    hy = Ref(SparseHyper(p.alpha00, p.beta00, p.gamma0, p.delta0, p.eta0, p.zeta0))
    chk(c.h, ccall((:vbmf_sparse_set_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Float64, Float64, Ref{SparseHyper}, Ptr{Int64}, Int64, Int64),
        c.h, p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta, p.BHat, p.L, p.SigmaB, p.CB, p.delta, p.sigmaHat, p.zeta, hy,
        C_NULL, 0, 0))
    chk(c.h, ccall((:vbmf_dual_set_priors, libvbmf), Cint, (Ptr{Cvoid}, Int64, Float64, Float64, Float64, Float64, Float64, Float64),
                   c.h, p.H0, p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha0, p.alpha1))
    diag_var && chk(c.h, ccall((:vbmf_sparse_set_noise_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64),
                               c.h, p.sigmaVecHat, p.zetaVec, p.etaVec[1]))
    set_full_cov!(c, p, full_cov)
    iters = Ref{Int64}(0); d = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_dual_run, libvbmf), Cint, (Ptr{Cvoid}, Int64, Float64, Cint, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
                   c.h, niter, eps, est_cb, est_priors, iters, d, C_NULL))
    n = p.M * p.H
    a = Array{Float64}(undef, n); ds = similar(a); ca = similar(a); be = similar(a); sa = Array{Float64}(undef, p.H)
    B = Array{Float64}(undef, p.L, p.H); SB = Array{Float64}(undef, p.H, p.H); cb = Array{Float64}(undef, p.H); dl = similar(cb)
    sh = Ref{Float64}(0.0); ze = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_sparse_get_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}),
        c.h, a, ds, ca, be, sa, B, p.L, SB, cb, dl, sh, ze))
    p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta = a, ds, ca, be
    p.AHat = permutedims(reshape(a, p.H, p.M)); p.A0Hat, p.A1Hat = p.AHat[:, 1:p.H0], p.AHat[:, p.H0+1:end]
    p.CA0, p.CA1 = dual_split(ca, p.M, p.H, p.H0); p.beta0, p.beta1 = dual_split(be, p.M, p.H, p.H0)
    pull_SigmaA!(c, p)
    p.BHat, p.SigmaB, p.CB, p.delta = B, SB, cb, dl
    if diag_var
        s = Array{Float64}(undef, p.L); z = similar(s)
        chk(c.h, ccall((:vbmf_sparse_get_noise_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), c.h, s, z))
        p.sigmaVecHat, p.zetaVec = s, z
    else
        p.sigmaHat, p.zeta = sh[], ze[]
    end
    H0r = Ref{Int64}(0); pr = Array{Float64}(undef, 6)
    chk(c.h, ccall((:vbmf_dual_get_priors, libvbmf), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Float64}), c.h, H0r, pr))
    p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha0, p.alpha1 = pr
    p.alpha = [p.alpha0, p.alpha1]
    p.L * p.M <= (1 << 24) && (p.YHat = p.BHat * p.AHat')                                       # :516
    verb && print("Factorization finished after ", iters[], " iterations, eps = ", d[], "\n")
    return d[]
end

# ---- the three-group variant, src/vbmf_trial.jl ---------------------------------------------------------------------------
# Field names of the reference's vbmf_trial_parameters (src/vbmf_trial.jl:68-131) minus the dense MH x MH pair.
mutable struct vbmf_trial_parameters
    L::Int; M::Int; M0::Int; M1::Int; MH::Int; H::Int; H0::Int; H1::Int
    AHat::Array{Float64,2}; ATVecHat::Array{Float64,1}; diagSigmaATVec::Array{Float64,1}; SigmaA::Array{Float64,2}
    A1Hat::Array{Float64,2}; A2Hat::Array{Float64,2}; A3Hat::Array{Float64,2}
    BHat::Array{Float64,2}; SigmaB::Array{Float64,2}
    CA::Array{Float64,1}; alpha::Array{Float64,1}; beta::Array{Float64,1}
    CA1::Array{Float64,1}; alpha01::Float64; beta01::Float64; alpha1::Float64; beta1::Array{Float64,1}
    CA2::Array{Float64,1}; alpha02::Float64; beta02::Float64; alpha2::Float64; beta2::Array{Float64,1}
    CA3::Array{Float64,1}; alpha03::Float64; beta03::Float64; alpha3::Float64; beta3::Array{Float64,1}
    CB::Array{Float64,1}; gamma0::Float64; delta0::Float64; gamma::Float64; delta::Array{Float64,1}
    sigmaHat::Float64; eta0::Float64; zeta0::Float64; eta::Float64; zeta::Float64
    sigmaVecHat::Array{Float64,1}; etaVec::Array{Float64,1}; zetaVec::Array{Float64,1}
    YHat::Array{Float64,2}; trYTY::Float64
    vbmf_trial_parameters() = new()
end

# (m, h)-interleaved vector <-> the three per-group vectors (A1: columns 1:H0, all rows; A2 / A3: the other columns of rows
# 1:M0 / M0+1:M), src/vbmf_trial.jl:160-190
function trial_split(v, M, H, H0, M0)
    a = reshape(v, H, M)
    return vec(a[1:H0, :]), vec(a[H0+1:end, 1:M0]), vec(a[H0+1:end, M0+1:end])
end
function trial_join(v1, v2, v3, M, H, H0, M0)
    H1 = H - H0
    return vec(vcat(reshape(v1, H0, M), hcat(reshape(v2, H1, M0), reshape(v3, H1, M - M0))))
end

"src/vbmf_trial.jl:139-226"
function vbmf_trial_init(Y::Array{Float64,2}, H::Int, H0::Int, M0::Int; ca = 1.0, alpha0 = 1e-10, beta0 = 1e-10, cb = 1.0,
                         gamma0 = 1e-10, delta0 = 1e-10, sigma = 1.0, eta0 = 1e-10, zeta0 = 1e-10)
    H < H0 && error("H must be at least H0!")
    p = vbmf_trial_parameters(); L, M = size(Y); H1 = H - H0; M1 = M - M0
    p.L, p.M, p.M0, p.M1, p.H, p.MH, p.H0, p.H1 = L, M, M0, M1, H, M * H, H0, H1
    p.AHat = randn(M, H); p.ATVecHat = reshape(permutedims(p.AHat), M * H); p.diagSigmaATVec = ones(M * H); p.SigmaA = zeros(H, H)
    p.A1Hat, p.A2Hat, p.A3Hat = p.AHat[:, 1:H0], p.AHat[1:M0, H0+1:end], p.AHat[M0+1:end, H0+1:end]
    p.BHat = randn(L, H); p.SigmaB = zeros(H, H)
    p.CA1, p.CA2, p.CA3 = ca * ones(M * H0), ca * ones(M0 * H1), ca * ones(M1 * H1)
    p.CA = trial_join(p.CA1, p.CA2, p.CA3, M, H, H0, M0)
    p.alpha01 = p.alpha02 = p.alpha03 = alpha0; p.beta01 = p.beta02 = p.beta03 = beta0
    p.alpha1 = p.alpha2 = p.alpha3 = alpha0 + 0.5
    p.beta1, p.beta2, p.beta3 = beta0 * ones(M * H0), beta0 * ones(M0 * H1), beta0 * ones(M1 * H1)
    p.alpha = [p.alpha1, p.alpha2, p.alpha3]; p.beta = trial_join(p.beta1, p.beta2, p.beta3, M, H, H0, M0)
    p.CB = cb * ones(H); p.gamma0, p.delta0, p.gamma, p.delta = gamma0, delta0, gamma0 + L / 2, delta0 * ones(H)
    p.sigmaHat, p.eta0, p.zeta0, p.eta, p.zeta = sigma, eta0, zeta0, eta0 + L * M / 2, zeta0
    p.sigmaVecHat, p.etaVec, p.zetaVec = sigma * ones(L), (eta0 + M / 2) * ones(L), zeta0 * ones(L)
    p.YHat = L * M <= (1 << 24) ? p.BHat * p.AHat' : Array{Float64}(undef, 0, 0)
    p.trYTY = sum(abs2, Y)
    return p
end

"vbmf_trial! -- src/vbmf_trial.jl:528-604 (returns d); est_priors: the six hyper-prior fits of :442-507 run on the device"
function vbmf_trial!(Y::Array{Float64,2}, p::vbmf_trial_parameters, niter::Int; eps::Float64 = 1e-6, diag_var::Bool = false,
                     full_cov::Bool = false, logdir = "", desc = "", verb = false, est_priors = true, est_cb::Bool = true)
    full_cov && p.H > 256 && error("full_cov=true is built for H <= 256 (either noise model)")
    logdir == "" || error("trajectory logging lives in the Python host (data_manip.py)")
    c = sparse_ctx_for(Y, p.H, diag_var; variant = diag_var ? 6 : 4)          # VBMF_VARIANT_TRIAL_DIAGVAR / _TRIAL_DIAG
    hy = Ref(SparseHyper(p.alpha01, p.beta01, p.gamma0, p.delta0, p.eta0, p.zeta0))
    chk(c.h, ccall((:vbmf_sparse_set_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Float64, Float64, Ref{SparseHyper}, Ptr{Int64}, Int64, Int64),
        c.h, p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta, p.BHat, p.L, p.SigmaB, p.CB, p.delta, p.sigmaHat, p.zeta, hy,
        C_NULL, 0, 0))
    pri = Float64[p.alpha01, p.beta01, p.alpha02, p.beta02, p.alpha03, p.beta03, p.alpha1, p.alpha2, p.alpha3]
    chk(c.h, ccall((:vbmf_trial_set_priors, libvbmf), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}), c.h, p.H0, p.M0, pri))
    diag_var && chk(c.h, ccall((:vbmf_sparse_set_noise_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64),
                               c.h, p.sigmaVecHat, p.zetaVec, p.etaVec[1]))
    set_full_cov!(c, p, full_cov)
    iters = Ref{Int64}(0); d = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_trial_run, libvbmf), Cint, (Ptr{Cvoid}, Int64, Float64, Cint, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
                   c.h, niter, eps, est_cb, est_priors, iters, d, C_NULL))
    n = p.M * p.H
    a = Array{Float64}(undef, n); ds = similar(a); ca = similar(a); be = similar(a); sa = Array{Float64}(undef, p.H)
    B = Array{Float64}(undef, p.L, p.H); SB = Array{Float64}(undef, p.H, p.H); cb = Array{Float64}(undef, p.H); dl = similar(cb)
    sh = Ref{Float64}(0.0); ze = Ref{Float64}(0.0)
    chk(c.h, ccall((:vbmf_sparse_get_state, libvbmf), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Float64}),
        c.h, a, ds, ca, be, sa, B, p.L, SB, cb, dl, sh, ze))
    p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta = a, ds, ca, be
    p.AHat = permutedims(reshape(a, p.H, p.M))
    p.A1Hat, p.A2Hat, p.A3Hat = p.AHat[:, 1:p.H0], p.AHat[1:p.M0, p.H0+1:end], p.AHat[p.M0+1:end, p.H0+1:end]
    p.CA1, p.CA2, p.CA3 = trial_split(ca, p.M, p.H, p.H0, p.M0); p.beta1, p.beta2, p.beta3 = trial_split(be, p.M, p.H, p.H0, p.M0)
    pull_SigmaA!(c, p)
    p.BHat, p.SigmaB, p.CB, p.delta = B, SB, cb, dl
    if diag_var
        s = Array{Float64}(undef, p.L); z = similar(s)
        chk(c.h, ccall((:vbmf_sparse_get_noise_rows, libvbmf), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), c.h, s, z))
        p.sigmaVecHat, p.zetaVec = s, z
    else
        p.sigmaHat, p.zeta = sh[], ze[]
    end
    H0r = Ref{Int64}(0); M0r = Ref{Int64}(0); pr = Array{Float64}(undef, 9)
    chk(c.h, ccall((:vbmf_trial_get_priors, libvbmf), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{Float64}), c.h, H0r, M0r, pr))
    p.alpha01, p.beta01, p.alpha02, p.beta02, p.alpha03, p.beta03, p.alpha1, p.alpha2, p.alpha3 = pr
    p.alpha = [p.alpha1, p.alpha2, p.alpha3]
    p.L * p.M <= (1 << 24) && (p.YHat = p.BHat * p.AHat')                                       # :590
    verb && print("Factorization finished after ", iters[], " iterations, eps = ", d[], "\n")
    return d[]
end

# ---- many fits on concatenated matrices [Y0 Y1] in ONE device call (vbmf_local_fit_batched) ------------------------------------------
"""
vbmf_trial! for many independent fits in ONE device call (src/vbmf_trial.jl:528-604): see vbmf_sparse_batch!; all fits share one H0,
M0 is per fit; est_priors refits the three (alpha0g, beta0g) pairs every sweep (:442-507).  Fills what vbmf_trial! fills.
"""
function vbmf_trial_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_trial_parameters}, niter::Int; eps::Float64 = 1e-6,
                           full_cov::Bool = false, est_cb::Bool = true, est_priors::Bool = true,
                           bag_of::Vector{Int} = collect(1:length(ps)), diag_var::Bool = false, form::Symbol = :stream,
                           slice_cols::Int = 0)
    H0 = ps[1].H0
    all(p.H0 == H0 for p in ps) || error("vbmf_trial_batch!: one H0 per call")
    all(0 <= p.M0 <= p.M for p in ps) || error("vbmf_trial_batch!: M0 outside 0..M")
    pri = Float64[(p.alpha01, p.beta01, p.alpha02, p.beta02, p.alpha03, p.beta03, 0.0, 0.0, 0.0)[k] for k in 1:9, p in ps]
    out = fit_batch_run!("vbmf_trial_batch!", Ys, ps, niter, eps, full_cov, est_cb, est_priors, H0, pri, bag_of, 4;
                         M0 = Int64[p.M0 for p in ps], rows = diag_var, form = form, slice_cols = slice_cols)
    for (f, p) in enumerate(ps)
        p.A1Hat, p.A2Hat, p.A3Hat = p.AHat[:, 1:p.H0], p.AHat[1:p.M0, p.H0+1:end], p.AHat[p.M0+1:end, p.H0+1:end]
        p.CA1, p.CA2, p.CA3 = trial_split(p.CA, p.M, p.H, p.H0, p.M0)
        p.beta1, p.beta2, p.beta3 = trial_split(p.beta, p.M, p.H, p.H0, p.M0)
        p.alpha01, p.beta01, p.alpha02, p.beta02, p.alpha03, p.beta03, p.alpha1, p.alpha2, p.alpha3 = pri[:, f]
        p.alpha = [p.alpha1, p.alpha2, p.alpha3]
    end
    return out
end

"""
vbmf_sparse! with a label mask for many independent fits in ONE device call (the fit of train_local, examples/mil_util.jl:302-320, on
Y = [Y0 Y1]): see vbmf_sparse_batch!.  The labels of every fit are exactly 1:M0 (possibly empty; M0 per fit) and all fits share one H1:
the last H1 columns of AHat stay zero in the rows 1:M0 (src/vbmf_sparse.jl:245).  Any other label set: vbmf_sparse! per fit.
"""
function vbmf_sparse_masked_batch!(Ys::Vector{Matrix{Float64}}, ps::Vector{vbmf_sparse_parameters}, niter::Int; eps::Float64 = 1e-6,
                                   full_cov::Bool = false, est_cb::Bool = true, bag_of::Vector{Int} = collect(1:length(ps)),
                                   diag_var::Bool = false, form::Symbol = :stream, slice_cols::Int = 0)
    H1 = ps[1].H1
    for (f, p) in enumerate(ps)
        (p.H1 == H1 && 0 <= H1 <= p.H) || error("vbmf_sparse_masked_batch!: one H1 in 0..H per call")
        (length(p.labels) <= p.M && p.labels == collect(1:length(p.labels))) ||
            error("vbmf_sparse_masked_batch!: the labels of fit $f are not the prefix 1:M0; use vbmf_sparse! per fit")
    end
    pri = Float64[(p.alpha0, p.beta0, p.alpha0, p.beta0, p.alpha0, p.beta0, 0.0, 0.0, 0.0)[k] for k in 1:9, p in ps]
    return fit_batch_run!("vbmf_sparse_masked_batch!", Ys, ps, niter, eps, full_cov, est_cb, false, ps[1].H, pri, bag_of, 1;
                          M0 = Int64[length(p.labels) for p in ps], mask_H1 = H1, rows = diag_var, form = form, slice_cols = slice_cols)
end

end # module
