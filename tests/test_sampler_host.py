"""The ensemble sampler's host side (pint_amd/sampler.py) and the host-checkable header under its
kernels (pint_amd/csrc/ensemble.hpp), without a GPU.

* Philox4x32-10: tests/csrc/ens_host.cpp, a program with its own main over ensemble.hpp, is built with
  hipcc for the host and must print Random123's published known answers (its kat_vectors file: counter
  and key all zero, all ones, and the digits of pi).  The all-ones and pi vectors are taken from an
  independent numpy Philox written here, which must itself reproduce the published zero vector.
* The same program prints the draw mapping, the double-double proposal and every prior kind for a
  table of inputs.  Draws and z: equal to the numpy twin's, bit for bit.  Proposals: within 2^-100 of
  the parameter's magnitude of the exact value -- computed in rational arithmetic (fractions.Fraction),
  because numpy's longdouble has 64 mantissa bits on x86 and cannot resolve 2^-100; sampler.py's numpy
  double-double gives the program's bits.  Priors: within 4 ulp of scipy.stats' logpdf.
* The API of EnsembleSampler on a small Gaussian target in the host-stepped mode, get_initial_pos, and
  integrated_time on an AR(1) series of known autocorrelation time.
"""
import os
import shutil
import subprocess
import types
import warnings
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LD = np.longdouble
ZERO_KAT = "6627e8d5 e169c58d bc57ac4c 9b00dbd8"  # Random123 kat_vectors: philox4x32 10, counter and key zero
PI_WORDS = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)


def np_philox(ctr, key):
    """Philox4x32-10 written from the paper (Salmon et al. 2011, section 3.3 and table 2's constants),
    independent of pint_amd: one block, Python integers."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def words(c):
    return " ".join(f"{x:08x}" for x in c)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("ens") / "ens_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-x", "hip", "--offload-host-only",
                    "-I", os.path.join(ROOT, "pint_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "ens_host.cpp"),
                    "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return out.stdout.strip().split("\n")
    return run


def test_numpy_philox_zero_vector():
    assert words(np_philox([0] * 4, [0] * 2)) == ZERO_KAT


def test_philox_known_answers(prog):
    from pint_amd import sampler as S
    ones = [0xFFFFFFFF] * 6
    cases = [[0] * 6, ones, list(PI_WORDS)]
    got = prog(["philox " + " ".join(f"{x:x}" for x in c) for c in cases])
    assert got[0] == ZERO_KAT
    for c, g in zip(cases, got):
        assert g == words(np_philox(c[:4], c[4:]))
        mine = S.philox4x32_10(np.array([c[:4]], dtype=np.uint32), np.array(c[4:], dtype=np.uint32))[0]
        assert g == words(int(x) for x in mine)


def test_draw_mapping(prog):
    """u_z (53 bits), the partner and u_acc of one block, and z, against sampler.draws / stretch."""
    from pint_amd import sampler as S
    cases = [(0, 0, 0, 0, 2), (7, 3, 11, 1, 65), (2 ** 63 + 5, 129, 2 ** 33 + 1, 1, 3), (12345, 4095, 24, 0, 2048)]
    got = prog([f"draw {s} {w} {t} {h} {n}" for s, w, t, h, n in cases])
    for (s, w, t, h, n), line in zip(cases, got):
        f = line.split()
        u_z, idx, u_acc = S.draws(s, [w], t, h, n)
        # and from the block itself, as DESIGN.md states the mapping
        r = np_philox([w, t & 0xFFFFFFFF, t >> 32, h], [s & 0xFFFFFFFF, s >> 32])
        m = ((r[1] << 32) | r[0]) >> 11
        assert float.fromhex(f[0]) == u_z[0] == (m + 0.5) * 2.0 ** -53 and 0.0 < u_z[0] < 1.0
        assert int(f[1]) == idx[0] == (r[2] * n) >> 32 and 0 <= idx[0] < n
        assert float.fromhex(f[2]) == u_acc[0] == (r[3] + 0.5) * 2.0 ** -32 and 0.0 < u_acc[0] < 1.0
        assert float.fromhex(f[3]) == S.stretch(2.0, u_z[0]) and 0.5 <= float.fromhex(f[3]) <= 2.0
        assert float.fromhex(f[4]) == S.stretch(1.5, u_z[0])


def test_dd_proposal(prog):
    from pint_amd import sampler as S
    rng = np.random.default_rng(5)
    scale = np.array([61.4854765543, -1.18e-15, 53750.0, 0.0, 1e-7, 223.9])
    rows = []
    for sc in scale:
        for spread in (1e-13, 1e-3, 1.0):
            for _ in range(4):
                x = sc * (1 + spread * rng.standard_normal(2))
                lo = x * 2.0 ** -54 * rng.uniform(-1, 1, 2)
                xs = [(float(h + l), float(l - ((h + l) - h))) for h, l in zip(x, lo)]
                rows.append((xs[0][0], xs[0][1], xs[1][0], xs[1][1], float(rng.uniform(0.5, 2.0))))
    got = prog(["prop " + " ".join(v.hex() for v in r) for r in rows])
    worst = 0.0
    for r, line in zip(rows, got):
        yh, yl = (float.fromhex(t) for t in line.split())
        xk, xj, z = Fraction(r[0]) + Fraction(r[1]), Fraction(r[2]) + Fraction(r[3]), Fraction(r[4])
        exact = xj + z * (xk - xj)
        mag = max(abs(xk), abs(xj))
        err = abs(Fraction(yh) + Fraction(yl) - exact)
        if mag:
            worst = max(worst, float(err / mag))
            assert err <= mag * Fraction(1, 2 ** 100), (r, float(err / mag))
        else:
            assert err == 0
        th, tl = S.propose(*(np.float64(v) for v in r))
        assert (float(th), float(tl)) == (yh, yl)  # the numpy double-double: the same bits
    print(f"worst proposal error {worst:.3g} of the parameter (bar {2.0 ** -100:.3g})")


def _fake_target(priors):
    params = [types.SimpleNamespace(name=f"P{i}", prior=p) for i, p in enumerate(priors)]
    return types.SimpleNamespace(params=params, nparams=len(params))


def test_priors_against_scipy(prog):
    from scipy.stats import norm, uniform
    from pint_amd import sampler as S
    from pint_amd.priors import Prior, UniformUnboundedRV, UniformBoundedRV, GaussianBoundedRV
    rvs = [uniform(-2.5, 7.0), UniformBoundedRV(61.48, 61.49), norm(3.0, 0.25), norm(-1e-15, 3e-17),
           GaussianBoundedRV(1.0, 0.5, 0.0, 2.5), UniformUnboundedRV(), UniformUnboundedRV()()]
    tab = S.prior_table(_fake_target([Prior(r) for r in rvs]))
    xs = {0: [-2.5, 4.5, 4.500000001, -2.6, 0.3, np.nan], 1: [61.48, 61.485, 61.49, 61.4900001], 2: [3.0, 2.1, 9.0, -40.0],
          3: [-1e-15, -1.05e-15, 0.0], 4: [0.0, 1.0, 2.5, 2.6, -0.1, 0.7], 5: [0.0, -1e300], 6: [3.0]}
    lines, ref = [], []
    for j, vals in xs.items():
        for x in vals:
            lines.append("prior " + " ".join(float(t).hex() for t in tab[j]) + " " + float(x).hex())
            with np.errstate(all="ignore"):
                ref.append(float(Prior(rvs[j]).logpdf(np.array([x]))[0]))
    phase = [float(S.L.ENS_PRIOR_PHASE), 0.0, 0.0, 0.0, 0.0, 0.0]
    for x, want in ((0.0, 0.0), (1.0, 0.0), (0.4, 0.0), (-1e-9, -np.inf), (1.0000001, -np.inf)):
        lines.append("prior " + " ".join(t.hex() for t in phase) + " " + float(x).hex())
        ref.append(want)
    got = [float.fromhex(t) for t in prog(lines)]
    for line, g, r in zip(lines, got, ref):
        if np.isnan(r):  # (a NaN value: the host counts a NaN log-prior as -inf)
            assert g == -np.inf
        elif np.isinf(r):
            assert g == r, line
        else:
            assert abs(g - r) <= 4 * np.spacing(abs(r)), (line, g, r)


def test_prior_table_refuses_what_it_cannot_hold():
    from scipy.stats import expon
    from pint_amd import sampler as S
    from pint_amd.priors import Prior, RandomInclinationPrior
    for rv in (expon(0.0, 2.0), RandomInclinationPrior()):
        with pytest.raises(NotImplementedError, match="P0"):
            S.prior_table(_fake_target([Prior(rv)]))


class Gauss:
    """A 3-parameter Gaussian posterior taking (N, 3, 2) pairs, as the sampler's host mode hands them."""
    nparams = 3
    param_labels = ["A", "B", "C"]
    sig = np.array([1.0, 0.1, 10.0])

    def lnposterior_batch(self, p):
        p = np.asarray(p, dtype=np.float64)
        v = p[..., 0] + p[..., 1] if p.ndim == 3 else p
        return -0.5 * np.sum((v / self.sig) ** 2, axis=1)


def test_sampler_api_host_mode():
    from pint_amd import EnsembleSampler
    t = Gauss()
    for bad in (3, 7, 2):
        with pytest.raises(ValueError):
            EnsembleSampler(t, bad, resident=False)
    with pytest.warns(RuntimeWarning, match="twice"):
        EnsembleSampler(t, 4, resident=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = EnsembleSampler(t, 6, seed=3, resident=False)
    with pytest.raises(NotImplementedError):
        EnsembleSampler(t, 6, resident=True)
    assert EnsembleSampler(t, 6, resident=None).resident is False
    p0 = np.random.default_rng(0).standard_normal((6, 3)) * t.sig
    with pytest.raises(ValueError):
        s.run_mcmc(p0[:, :2], 3)
    with pytest.raises(ValueError):
        s.run_mcmc(None, 3)
    bad = p0.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="walker 2"):
        s.run_mcmc(bad, 3)
    s.run_mcmc(p0, 10)
    s.run_mcmc(None, 15)
    c, lp = s.get_chain(), s.get_log_prob()
    assert c.shape == (25, 6, 3) and lp.shape == (25, 6) and c.dtype == np.float64
    assert s.get_chain(longdouble=True).dtype == LD and s.get_chain(flat=True, discard=5, thin=2).shape == (60, 3)
    assert s.get_log_prob(flat=True).shape == (150,)
    assert np.array_equal(lp, t.lnposterior_batch(c.reshape(-1, 3)).reshape(25, 6))
    assert s.acceptance_fraction.shape == (6,) and np.all((s.acceptance_fraction > 0) & (s.acceptance_fraction <= 1))
    assert np.all(s.n_flagged == 0)
    d = s.chains_to_dict(t.param_labels)
    assert list(d) == t.param_labels and np.array_equal(d["B"], c[:, :, 1])
    last, lnl = s.get_last_sample()
    assert np.array_equal(last.astype(np.float64), c[-1]) and np.array_equal(lnl, lp[-1])
    # the chain is a function of the seed, the start and the step numbers
    s2 = EnsembleSampler(t, 6, seed=3, resident=False)
    s2.run_mcmc(p0, 25)
    assert np.array_equal(s2.get_chain_pairs(), s.get_chain_pairs()) and np.array_equal(s2.get_log_prob(), lp)
    s3 = EnsembleSampler(t, 6, seed=4, resident=False)
    s3.run_mcmc(p0, 25)
    assert not np.array_equal(s3.get_chain(), c)
    s2.reset()
    assert s2.get_chain().shape == (0, 6, 3) and s2.iteration == 0
    s2.run_mcmc(p0, 4, thin_by=3)
    assert s2.get_chain().shape == (4, 6, 3) and s2.iteration == 12
    assert np.array_equal(s2.get_chain(), c[2:12:3])


def test_get_initial_pos():
    from pint_amd import EnsembleSampler, get_initial_pos
    keys = ["F0", "ECC", "SINI", "M2", "PX", "PHASE", "GLEP_1", "GLPH_1"]
    vals = np.array([61.5, 0.97, 0.9, 0.3, 1.2, 0.5, 55000.0, 0.0], dtype=LD)
    errs = np.array([1e-10, 0.2, 0.1, 0.1, 0.5, 0.03, 10.0, 0.1])
    pos = get_initial_pos(keys, vals, errs, 0.1, 200, rng=11, minMJD=54000.0, maxMJD=56000.0)
    assert pos.shape == (200, 8) and pos.dtype == LD
    assert np.array_equal(pos, get_initial_pos(keys, vals, errs, 0.1, 200, rng=11, minMJD=54000.0, maxMJD=56000.0))
    assert not np.array_equal(pos, get_initial_pos(keys, vals, errs, 0.1, 200, rng=12, minMJD=54000.0, maxMJD=56000.0))
    assert np.array_equal(pos[0], vals)
    w = pos[1:].astype(np.float64)
    assert np.all(np.abs(w[:, 0] - 61.5) < 6 * 1e-11)
    assert np.all((w[:, 1] >= 0) & (w[:, 1] <= 1.0)) and np.std(w[:, 1]) > 0.05  # (reflected below 1, the full error)
    assert np.all((w[:, 2] >= 0) & (w[:, 2] <= 1)) and np.all((w[:, 3] >= 0.1) & (w[:, 3] <= 0.6))
    assert np.all(w[:, 4] >= 0) and np.all((w[:, 5] >= 0) & (w[:, 5] <= 1))
    assert np.all((w[:, 6] >= 54100) & (w[:, 6] <= 55900)) and np.all(np.abs(w[:, 7]) <= 0.5)
    with pytest.raises(ValueError):
        get_initial_pos(keys, vals, errs, 0.1, 8, rng=1)  # (GLEP_1 without the MJD range)
    with pytest.raises(ValueError):
        get_initial_pos(keys[:3], vals, errs, 0.1, 8)
    s = EnsembleSampler(Gauss(), 8, seed=5, resident=False)
    p = s.get_initial_pos(["A", "B", "C"], np.zeros(3), Gauss.sig, 0.1)
    assert p.shape == (8, 3) and np.array_equal(p, s.get_initial_pos(["A", "B", "C"], np.zeros(3), Gauss.sig, 0.1))


def test_integrated_time_ar1():
    """AR(1) with rho = 0.9 has tau = (1 + rho) / (1 - rho) = 19; at 2e5 samples the estimator's own
    standard error is ~3 %, the bar 10 %."""
    from pint_amd import integrated_time
    rho, n = 0.9, 200000
    e = np.random.default_rng(2024).standard_normal(n)
    x = np.empty(n)
    x[0] = e[0] / np.sqrt(1 - rho ** 2)
    for i in range(1, n):
        x[i] = rho * x[i - 1] + e[i]
    tau = integrated_time(x)
    assert tau.shape == (1,)
    print(f"tau {tau[0]:.3f} (19 expected)")
    assert abs(tau[0] / 19.0 - 1.0) < 0.10
    # walkers are averaged: four independent pieces as four walkers
    tau4 = integrated_time(x.reshape(4, n // 4).T)
    assert abs(tau4[0] / 19.0 - 1.0) < 0.10
