"""Longdouble linear algebra for the tests' reference solutions (numpy's own solvers drop to
float64): the solve and the inverse of a stage's linear system, and the weighted Gram and
Woodbury chi2 the shape sweep compares the kernels against, and the host's Fourier columns."""
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


def host_fourier(lay, toas):
    """sin / cos(2 pi f_k t) in longdouble, t = tdbld * 86400 (noise_model.py:861-880)."""
    t = np.asarray(toas.tdbld, dtype=LD) * LD(86400)
    f = np.asarray(lay.red_freq, dtype=LD)
    F = np.zeros((toas.ntoas, 2 * len(f)), dtype=LD)
    twopi = 8 * np.arctan(LD(1))  # (np.pi is a double)
    F[:, ::2] = np.sin(twopi * t[:, None] * f)
    F[:, 1::2] = np.cos(twopi * t[:, None] * f)
    return F
