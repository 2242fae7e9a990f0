"""Per-entry fp64 references of the ARD-sparse updates (csrc/sparse_kernels.hpp; src/vbmf_sparse.jl, diagonal branch) and the
synthetic states they are evaluated on.  Plain NumPy: tests/test_sparse_entry_reference.py pins these functions to the oracle
(1e-12), tests/test_gpu_sparse_entries.py holds the device to them entry by entry.

Every function takes the numbers the device holds (fp32 tables as fp64 arrays, the state block's fp64 matrices) and returns the
value of ONE update in fp64 together with the magnitudes its error bound is stated in; nothing here rounds to fp32."""
import numpy as np

U = 2.0 ** -24            # fp32 unit roundoff
E = 2.0 ** -53            # fp64 unit roundoff
HYPER = dict(alpha0=0.1, beta0=1e-10, gamma0=0.1, delta0=1e-10, eta0=0.1, zeta0=1e-10)


# ---- synthetic states ------------------------------------------------------------------------------------------------------
def loguniform(rng, lo, hi, size):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), size)


def synthetic_state(L, M, H, seed, hyper=HYPER):
    """A state whose arrays span the decades an ARD model reaches after pruning, built directly (a trajectory from ca = cb =
    sigma = 0.1 collapses to A ~ 1e-6 within three sweeps at the edge shapes): A, B standard normal with columns scaled by
    10^linspace(0, -4, H); CA log-uniform over [1e-2, 1e3] with beta = alpha / CA; diagSigmaATVec log-uniform over [1e-4, 1];
    SigmaB = 0.01 (R R'/H + I); CB log-uniform over [1, 1e3] with delta = gamma / CB; sigmaHat = 0.75."""
    rng = np.random.default_rng(seed)
    col = 10.0 ** np.linspace(0.0, -4.0, H)
    A = rng.standard_normal((M, H)) * col
    B = rng.standard_normal((L, H)) * col
    CA = loguniform(rng, 1e-2, 1e3, M * H)
    dS = loguniform(rng, 1e-4, 1.0, M * H)
    R = rng.standard_normal((H, H)) / np.sqrt(H)
    SB = 0.01 * (R @ R.T + np.eye(H))
    CB = loguniform(rng, 1.0, 1e3, H)
    alpha, gamma = hyper["alpha0"] + 0.5, hyper["gamma0"] + 0.5 * L
    return dict(ATVecHat=A.reshape(M * H).copy(), diagSigmaATVec=dS, CA=CA, beta=alpha / CA, BHat=B, SigmaB=SB, CB=CB,
                delta=gamma / CB, sigmaHat=0.75, zeta=(hyper["eta0"] + 0.5 * L * M) / 0.75)


def synthetic_noise_rows(L, M, seed, hyper=HYPER):
    """Row precisions of the heteroscedastic model: sigma_l log-uniform over [0.1, 10], zeta_l consistent with etaVec."""
    rng = np.random.default_rng(seed)
    sig = loguniform(rng, 0.1, 10.0, L)
    etaVec = hyper["eta0"] + 0.5 * M
    return sig, etaVec / sig, etaVec


# ---- updateA!, diagonal branch (:204-247) -----------------------------------------------------------------------------------
def v_index(M, H, compat):
    """Which v[.] position p = m H + h of vec(A') takes: `repeat(v, inner = M-1)` behind the first H entries (QS1), or h."""
    p = np.arange(M * H)
    if compat:
        vi = np.where(p < H, p, (p - H) // max(M - 1, 1))
    else:
        vi = p % H
    return vi.reshape(M, H)


def ref_v(sigmaHat, GB_diag, SB_diag, L):
    """v[h] = sigmaHat (B'B)[h,h] + L SigmaB[h,h]   (:217; sigmaHat does not multiply L SigmaB)"""
    return sigmaHat * np.asarray(GB_diag) + L * np.asarray(SB_diag)


def ref_v_rows(sig, B, mean_sigma, SB_diag, L):
    """diag_var: v[h] = sum_l (sigma_l B[l,h])^2 + L mean(sigma) SigmaB[h,h]   (:211)"""
    sB = np.asarray(sig)[:, None] * B
    return np.sum(sB * sB, axis=0) + L * mean_sigma * np.asarray(SB_diag)


def ref_updateA(Psum, Pabs, v, CA, sig, compat, labels0=(), H1=0):
    """d = 1 / (v[vi] + CA), a = sig d P per entry (m, h); Psum, Pabs: the M x H product Y'B and the sum of its slabs'
    magnitudes; sig: sigmaHat, or 1 under diag_var (sigma is inside P, :230).  Returns (d, a, scale of a's error, mask)."""
    M, H = Psum.shape
    d = 1.0 / (np.asarray(v)[v_index(M, H, compat)] + np.asarray(CA).reshape(M, H))
    a = sig * d * Psum
    mask = np.zeros((M, H), dtype=bool)
    if len(labels0) and H1 > 0:
        mask[np.asarray(labels0, dtype=np.int64), H - H1:] = True
    a = np.where(mask, 0.0, a)
    return d, a, sig * d * Pabs, mask


# ---- updateCA! (:284-288; the grouped models' src/vbmf_dual.jl:322-351, src/vbmf_trial.jl:357-400) --------------------------
def ca_group(M, H, H0, M0):
    """Group of entry (m, h): 0 for h < H0; behind it 1 for rows m < M0, 2 for the rest."""
    g = np.where(np.arange(M)[:, None] < M0, 1, 2) * np.ones((1, H), dtype=np.int64)
    g[:, :H0] = 0
    return g


def ref_updateCA(A, dS, alpha, beta0):
    """b = beta0 + (a^2 + ds) / 2, ca = alpha / b; alpha, beta0 scalars or per-entry arrays (each entry's own group's)."""
    b = beta0 + 0.5 * (A * A + dS)
    return b, alpha / b


# ---- updateB! (:263-265), updateCB! (:295-300), updateSigma! (:308-321) -----------------------------------------------------
def ref_K(CB, sig, GA, SA):
    """The matrix SigmaB inverts: diag(CB) + sigmaHat (A'A + SigmaA)"""
    return np.diag(CB) + sig * (GA + SA)


def ref_updateCB(GB_diag, SB_diag, gamma, delta0):
    delta = delta0 + 0.5 * (np.asarray(GB_diag) + np.asarray(SB_diag))
    return delta, gamma / delta


def ref_zeta(zeta0, trYY, trBQ, GA, SA, GB, SB, L):
    """zeta = zeta0 + trYY/2 - tr(B'YA) + sum (GA + SA) o (GB + L SB) / 2 and the sum of its terms' magnitudes."""
    T = (GA + SA) * (GB + L * SB)
    zeta = zeta0 + 0.5 * trYY - trBQ + 0.5 * float(np.sum(T))
    mag = zeta0 + 0.5 * trYY + abs(trBQ) + 0.5 * float(np.sum(np.abs((GA + SA)) * (np.abs(GB) + L * np.abs(SB))))
    return zeta, mag


def ref_zeta_rows(zeta0, Y, Q, B, G, SB, Gq=None):
    """zeta_l = zeta0 + ||Y_l||^2/2 - Q_l . B_l + (B_l' Gq B_l + tr(G SigmaB))/2 per row (:309-314); Gq: the table the quadratic
    form reads (the device's fp32 copy of G; G itself when None).  Returns (zeta, the sum of the terms' magnitudes,
    |B_l|'|Gq||B_l|)."""
    Gq = G if Gq is None else Gq
    yy = np.sum(Y * Y, axis=1)
    qb = np.sum(Q * B, axis=1)
    quad = np.einsum("lh,hk,lk->l", B, Gq, B)
    tr = float(np.sum(G * SB))
    zeta = zeta0 + 0.5 * yy - qb + 0.5 * (quad + tr)
    aquad = np.einsum("lh,hk,lk->l", np.abs(B), np.abs(Gq), np.abs(B))
    mag = zeta0 + 0.5 * yy + np.sum(np.abs(Q * B), axis=1) + 0.5 * (aquad + float(np.sum(np.abs(G * SB))))
    return zeta, mag, aquad
