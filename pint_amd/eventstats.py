"""Pulsation statistics of photon phases (reference ``src/pint/eventstats.py``): the Z^2_m test and
the H-test (de Jager, Raubenheimer & Swanepoel 1989; de Jager & Buesching 2010), their weighted forms
and the analytic calibration of the H-test (Kerr 2011, ApJ 732, 38), with the reference's signatures.

Every statistic is made of the trigonometric sums

    C_j = sum_i w_i cos(2 pi j phi_i),   S_j = sum_i w_i sin(2 pi j phi_i),   sum w,   sum w^2

(w = 1 for unweighted data).  z2m, z2mw, hm and hmw therefore also take them ready-made through the
keyword ``sums``: an array (..., 2 M + 2) laid out as Session.point_photon_trig returns it (C_1, S_1,
..., C_M, S_M, sum w, sum w^2; M >= m), one row per point of a batch, so that a batch's statistics
need no phases read back from the device.  With ``sums`` the phases (and weights) arguments are
ignored and may be None; the result gains the leading axes of ``sums``.
"""
from __future__ import annotations

import numpy as np

__all__ = ["z2m", "z2mw", "hm", "hmw", "em_four", "sf_z2m", "sf_hm", "h2sig", "sig2sigma", "trig_sums"]

TWOPI = 2.0 * np.pi


def trig_sums(phases, m, weights=None):
    """(2 m + 2,): C_1, S_1, ..., C_m, S_m, sum w, sum w^2 of the phases (cycles) on the host."""
    ph = np.asarray(phases, dtype=np.float64) * TWOPI
    w = np.ones_like(ph) if weights is None else np.asarray(weights, dtype=np.float64)
    out = np.empty(2 * m + 2)
    for k in range(1, m + 1):
        out[2 * k - 2] = (w * np.cos(k * ph)).sum()
        out[2 * k - 1] = (w * np.sin(k * ph)).sum()
    out[2 * m] = w.sum()
    out[2 * m + 1] = (w * w).sum()
    return out


def _powers(phases, weights, m, sums):
    """(C_j^2 + S_j^2 for j = 1..m, sum w, sum w^2), from the phases or from ready-made sums."""
    if sums is None:
        sums = trig_sums(phases, m, weights)
    s = np.asarray(sums, dtype=np.float64)
    M = (s.shape[-1] - 2) // 2
    if s.shape[-1] != 2 * M + 2 or M < m or m < 1:
        raise ValueError(f"sums must hold 2 M + 2 values with M >= m = {m}, got {s.shape[-1]}")
    return s[..., 0:2 * m:2] ** 2 + s[..., 1:2 * m:2] ** 2, s[..., -2], s[..., -1]


def z2m(phases, m=2, *, sums=None):
    """The Z^2_k statistics for k = 1..m (de Jager et al. 1989): (2 / n) sum_{j <= k} (C_j^2 + S_j^2)."""
    p, sw, _ = _powers(phases, None, m, sums)
    return (2.0 / np.asarray(sw)[..., None]) * np.cumsum(p, axis=-1)


def z2mw(phases, weights, m=2, *, sums=None):
    """The weighted Z^2_k for k = 1..m: (2 / sum w^2) sum_{j <= k} (C_j^2 + S_j^2), which keeps the
    unweighted calibration (Kerr 2011)."""
    p, _, sw2 = _powers(phases, weights, m, sums)
    return np.cumsum(p, axis=-1) * (2.0 / np.asarray(sw2)[..., None])


def _h_of_z(z, m, c):
    return (z - c * np.arange(0, m)).max(axis=-1)


def hm(phases, m=20, c=4, *, sums=None):
    """The H statistic (de Jager et al. 1989): max over 1 <= k <= m of Z^2_k - c (k - 1)."""
    return _h_of_z(z2m(phases, m, sums=sums), m, c)


def hmw(phases, weights, m=20, c=4, *, sums=None):
    """The weighted H statistic (Kerr 2011): hm on the weighted Z^2_k."""
    return _h_of_z(z2mw(phases, weights, m, sums=sums), m, c)


def em_four(phases, m=2, weights=None):
    """The empirical Fourier coefficients (a_k, b_k), k = 1..m: the (weighted) trigonometric moments
    over n (over sum w with weights)."""
    s = trig_sums(phases, m, weights)
    n = len(np.asarray(phases)) if weights is None else s[-2]
    return (1.0 / n) * s[0:2 * m:2], (1.0 / n) * s[1:2 * m:2]


def sf_z2m(ts, m=2):
    """The asymptotic chance probability of Z^2_m: chi^2 with 2 m degrees of freedom."""
    from scipy.stats import chi2
    return chi2.sf(ts, 2 * m)


def sf_hm(h, m=20, c=4, logprob=False):
    """The asymptotic survival function of the H-test with maximum harmonic m and penalty c per
    harmonic (Kerr 2011, eqs. 7-10; calibrated there for m = 20, c = 4), or its logarithm:

        P(H > h) = exp(-h / 2) sum_{i < m} alpha^i I_i(h),   alpha = exp(-c / 2) / 2,
        I_i(h) = (h + i c)^i / i! - sum_{j < i} I_j(h) ((i - j) c)^(i - j) / (i - j)!.
    """
    from scipy.special import gammaln
    if np.ndim(h) != 0:
        raise NotImplementedError("sf_hm takes one H value at a time (as the reference's)")
    if int(m) != m or m < 1 or not c > 0:
        raise NotImplementedError(f"sf_hm: m = {m}, c = {c} (a positive integer m and a positive c are built)")
    m = int(m)
    if h < 1e-16:
        return 1.0
    d = np.arange(1, m)
    q = np.exp(d * np.log(d * c) - gammaln(d + 1))  # (d c)^d / d!, d = 1..m-1
    ints = np.empty(m)  # I_i(h)
    for i in range(m):
        ints[i] = np.exp(i * np.log(h + i * c) - gammaln(i + 1)) - (ints[:i] * q[:i][::-1]).sum()
    alpha = 0.5 * np.exp(-0.5 * c)
    series = (alpha ** np.arange(0, m) * ints).sum()
    return -0.5 * h + np.log(series) if logprob else np.exp(-0.5 * h) * series


LOG_SQRT_PI = 0.5 * np.log(np.pi)
TINY_TAIL = 1e-300  # below this the tail probability goes through its logarithm


def _tail_sigma(p, logp):
    """sigma with two-tailed normal tail probability p = exp(logp), elementwise.  Down to TINY_TAIL the
    normal quantile itself, -ndtri(p / 2).  Below it p / 2 leaves float64's range and only logp is
    usable; there the reference's closed form is kept, so that values continue across the switch:
    with x0^2 = -2 (logp + log sqrt(pi)), the leading term of 2 Q(x) ~ exp(-x^2 / 2) sqrt(2 / pi) / x
    solved for x, sigma = x0 - log(x0) / (1 + 2 x0) (a first correction for the 1 / x factor; it is
    the reference's eventstats.sig2sigma expression, not a series from the literature)."""
    from scipy.special import ndtri
    out = np.empty_like(p)
    exact = p > TINY_TAIL
    out[exact] = -ndtri(0.5 * p[exact])
    x0 = np.sqrt(-2.0 * (logp[~exact] + LOG_SQRT_PI))
    out[~exact] = x0 - np.log(x0) / (1.0 + 2.0 * x0)
    return out


def sig2sigma(sig, two_tailed=True, logprob=False):
    """The Gaussian "sigma" of a chance probability ``sig`` (its natural logarithm with ``logprob``):
    the x with P(|N(0, 1)| > x) = sig, or, one-tailed, with P(N(0, 1) > x) = sig (negative for
    sig > 0.5).  A scalar gives a scalar."""
    given = np.atleast_1d(np.asarray(sig, dtype=float))
    with np.errstate(divide="ignore", invalid="ignore"):
        p, logp = (np.exp(given), given) if logprob else (given, np.log(given))
    if np.any(logp > 0) or (not logprob and np.any(p <= 0)):
        raise ValueError("Probability must be between 0 and 1.")
    if not two_tailed:  # (a one-tailed probability is half a two-tailed one)
        p, logp = 2.0 * p, logp + np.log(2.0)
    out = _tail_sigma(p, logp)
    return out[0] if given.shape == (1,) else out


def h2sig(h):
    """The significance in sigma of an H-test value (m = 20, c = 4)."""
    return sig2sigma(sf_hm(h, logprob=True), logprob=True)
