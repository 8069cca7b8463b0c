"""Longdouble linear algebra for the tests' reference solutions (numpy's own solvers drop to
float64): the solve and the inverse of a stage's linear system, and the weighted Gram and
Woodbury chi2 the shape sweep compares the kernels against, and the host's Fourier columns;
the sweeps' shared part (c) (step_errors); for the ECORR sweep the elimination of the epoch
block and the block-by-block likelihood of an ECORR-only covariance."""
import numpy as np

LD = np.longdouble


def ld_inverse(A):
    """Gauss-Jordan inverse with partial pivoting in longdouble."""
    A = np.array(A, dtype=np.longdouble)
    n = len(A)
    M = np.concatenate([A, np.eye(n, dtype=np.longdouble)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] /= M[k, k]
        f = M[:, k].copy()
        f[k] = 0
        M -= np.outer(f, M[k])
    return M[:, n:]


def ld_solve(A, b):
    """Gaussian elimination with partial pivoting in longdouble (numpy's solvers drop to
    float64): the reference solution of a stage's linear system."""
    A = np.array(A, dtype=np.longdouble)
    b = np.array(b, dtype=np.longdouble)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:])
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, dtype=np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def ld_gram(M, r, sigma):
    """[M | r]^T N^-1 [M | r] with N = diag(sigma^2), and M's unweighted column sums of
    squares, accumulated in longdouble from the float64 inputs."""
    X = np.concatenate([np.asarray(M, dtype=LD), np.asarray(r, dtype=LD)[:, None]], axis=1)
    W = X / np.asarray(sigma, dtype=LD)[:, None]
    return W.T @ W, np.sum(X[:, :-1] * X[:, :-1], axis=0)


def ld_woodbury_chi2(r, sigma, U, phi):
    """r^T C^-1 r for C = N + U diag(phi) U^T by the Woodbury identity (utils.py:3074
    woodbury_dot) in longdouble: r^T N^-1 r - d^T Sigma^-1 d with Sigma = diag(1 / phi) +
    U^T N^-1 U and d = U^T N^-1 r.  U's columns are scaled to unit weighted norm first (the
    chi2 does not change; Sigma stays well scaled next to a 1e40 prior).  Returns (chi2,
    r^T N^-1 r)."""
    r = np.asarray(r, dtype=LD)
    w = 1 / np.asarray(sigma, dtype=LD) ** 2
    U = np.asarray(U, dtype=LD)
    s = np.sqrt(np.sum(U * U * w[:, None], axis=0))
    Un = U / s
    Sigma = Un.T @ (Un * w[:, None]) + np.diag(1 / (np.asarray(phi, dtype=LD) * s * s))
    d = Un.T @ (w * r)
    rNr = np.sum(w * r * r)
    return rNr - d @ ld_solve(Sigma, d), rNr


def ld_ecorr_eliminate(G, X, sigma, ep):
    """The ECORR block eliminated from G = X^T N^-1 X: G - S^T Sigma_E^-1 S with S = E^T N^-1 X
    (row e: s_e = sum_{i in e} w_i X_i) and Sigma_E = E^T N^-1 E + diag(1 / phi_e).  ep: [(TOA
    indices, phi_e)].  Disjoint epochs: Sigma_E = diag(D_e), D_e = 1 / phi_e + sum_{i in e} w_i;
    a TOA in two epochs couples them and Sigma_E is inverted densely.  Returns (G', S, D_e)."""
    w = 1 / np.asarray(sigma, dtype=LD) ** 2
    Xw = np.asarray(X, dtype=LD) * w[:, None]
    S = np.array([Xw[idx].sum(axis=0) for idx, _ in ep], dtype=LD).reshape(len(ep), Xw.shape[1])
    D = np.array([1 / LD(ph) + np.sum(w[idx]) for idx, ph in ep], dtype=LD)
    allidx = np.concatenate([np.asarray(idx) for idx, _ in ep])
    if len(np.unique(allidx)) == len(allidx):
        return G - (S / D[:, None]).T @ S, S, D
    E = np.zeros((len(w), len(ep)), dtype=LD)
    for e, (idx, _) in enumerate(ep):
        E[idx, e] = 1
    SigE = E.T @ (E * w[:, None]) + np.diag(np.array([1 / LD(ph) for _, ph in ep], dtype=LD))
    return G - S.T @ (ld_inverse(SigE) @ S), S, D


def chol64(A, B):
    """float64 LAPACK Cholesky solve A X = B."""
    L = np.linalg.cholesky(np.asarray(A, dtype=np.float64))
    return np.linalg.solve(L.T, np.linalg.solve(L, np.asarray(B, dtype=np.float64)))


def step_errors(G, colsq, K, ncol, mode, red_phi, dp, er, cov):
    """The sweeps' part (c): the device's step dp, errors er and timing covariance cov against a
    longdouble solve and inverse of the device's own normalised system, built element for element
    from its Gram G and column sums of squares colsq as the solve kernels form it (mode 0: the
    ncol timing columns normalised by the Gram's diagonal; mode 1: all K by sqrt(colsq), 1 / phi
    on the Fourier columns' diagonal).  Returns (e_dev, e_ref, s_dev, s_ref, c_dev, c_ref): the
    device's errors and those of a float64 LAPACK Cholesky solve of the same system, the step in
    units of sigma, the errors relative, the covariance in sigma_i sigma_j."""
    Kf = ncol if mode == 0 else K
    norm = np.sqrt(np.diag(G)[:Kf]) if mode == 0 else np.sqrt(colsq)
    inv = 1.0 / norm
    Ad = G[:Kf, :Kf] * (inv[:, None] * inv[None, :])
    if mode == 1 and K > ncol:
        i = np.arange(ncol, K)
        Ad[i, i] += (inv[ncol:] * inv[ncol:]) / np.asarray(red_phi)
    bd = G[:Kf, K] * inv
    x = ld_solve(Ad, bd) * inv
    X = ld_inverse(Ad) * np.outer(inv, inv)
    sg = np.sqrt(np.diag(X))
    X64 = chol64(Ad, np.eye(Kf)) * np.outer(inv, inv)
    e_ref = float(np.max(np.abs(chol64(Ad, bd) * inv - x) / sg))
    e_dev = float(np.max(np.abs(dp[:Kf] - x) / sg))
    s_ref = float(np.max(np.abs(np.sqrt(np.diag(X64)) / sg - 1)))
    s_dev = float(np.max(np.abs(er[:Kf] / sg - 1)))
    ss = np.outer(sg[:ncol], sg[:ncol])
    c_ref = float(np.max(np.abs(X64[:ncol, :ncol] - X[:ncol, :ncol]) / ss))
    c_dev = float(np.max(np.abs(cov - X[:ncol, :ncol]) / ss))
    return e_dev, e_ref, s_dev, s_ref, c_dev, c_ref


def ld_cholesky(A):
    """Lower Cholesky factor in longdouble."""
    A = np.array(A, dtype=LD)
    n = len(A)
    Lo = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - Lo[j, :j] @ Lo[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        Lo[j, j] = np.sqrt(d)
        Lo[j + 1:, j] = (A[j + 1:, j] - Lo[j + 1:, :j] @ Lo[j, :j]) / Lo[j, j]
    return Lo


def ld_block_likelihood(r, N, ep, dN=(), dphi=()):
    """(chi2 = r^T C^-1 r, logdet C / 2, derivatives) of C = diag(N) + sum_e phi_e 1_e 1_e^T for
    disjoint epochs ep = [(TOA indices, phi_e)], taken block by block in longdouble: one dense
    block N_e + phi_e 1 1^T and its Cholesky factor per epoch, the diagonal rest (no
    Sherman-Morrison algebra).  dN: arrays dN_i / dp (one per parameter p of the diagonal), dphi:
    arrays dphi_e / dp; for each, (1/2 r^T C^-1 dC C^-1 r - 1/2 tr(C^-1 dC), the sum of the absolute
    values of the terms) as d lnL / dp and the scale of its bar.  Last, (1^T C^-1 r, 1^T C^-1 1)."""
    r, N = np.asarray(r, dtype=LD), np.asarray(N, dtype=LD)
    n = len(r)
    y = np.zeros(n, dtype=LD)      # C^-1 r
    cdiag = np.zeros(n, dtype=LD)  # diag(C^-1)
    csum = []                      # 1_e^T C^-1 1_e per epoch
    ysum = []                      # 1_e^T C^-1 r
    ld = LD(0)
    rest = np.ones(n, dtype=bool)
    for idx, ph in ep:
        idx = np.asarray(idx)
        assert np.all(rest[idx]), "overlapping epochs"
        rest[idx] = False
        C = np.diag(N[idx]) + LD(ph)
        Lo = ld_cholesky(C)
        Ci = ld_inverse(C)
        y[idx] = Ci @ r[idx]
        cdiag[idx] = np.diag(Ci)
        csum.append(np.sum(Ci))
        ysum.append(np.sum(y[idx]))
        ld += np.sum(np.log(np.diag(Lo)))
    y[rest] = r[rest] / N[rest]
    cdiag[rest] = 1 / N[rest]
    ld += np.sum(np.log(N[rest])) / 2
    chi2 = r @ y
    grads = []
    for d in dN:
        d = np.asarray(d, dtype=LD)
        a, b = np.sum(y * y * d) / 2, np.sum(cdiag * d) / 2
        grads.append((a - b, abs(a) + abs(b)))
    for d in dphi:
        d = np.asarray(d, dtype=LD)
        a = sum(ys * ys * de for ys, de in zip(ysum, d)) / 2
        b = sum(cs * de for cs, de in zip(csum, d)) / 2
        grads.append((a - b, abs(a) + abs(b)))
    # the 1e40 offset column of _calc_gls_chi2 (kind 2), one rank-1 term on top of the blocks
    ones = (np.sum(y), sum(csum) + np.sum(1 / N[rest]))  # 1^T C^-1 r, 1^T C^-1 1
    return chi2, ld, grads, ones


def host_fourier(lay, toas):
    """sin / cos(2 pi f_k t) in longdouble, t = tdbld * 86400 (noise_model.py:861-880)."""
    t = np.asarray(toas.tdbld, dtype=LD) * LD(86400)
    f = np.asarray(lay.red_freq, dtype=LD)
    F = np.zeros((toas.ntoas, 2 * len(f)), dtype=LD)
    twopi = 8 * np.arctan(LD(1))  # (np.pi is a double)
    F[:, ::2] = np.sin(twopi * t[:, None] * f)
    F[:, 1::2] = np.cos(twopi * t[:, None] * f)
    return F
