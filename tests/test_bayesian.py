"""BayesianTiming (pint_amd/bayesian.py), the priors (pint_amd/priors.py) and the three entry points
under them (pint_set_points, pint_set_dm_noise_classes, pint_point_lnlike), against fixtures captured
from the reference's pint.bayesian.BayesianTiming (scripts/refgen/gen_bayesian.py):

* bayes_nb    : narrowband, 300 TOAs, ELL1; two EFACs and two EQUADs on overlapping MJD ranges, TOAs
                under no mask, one white-noise class of a single TOA; no PhaseOffset;
* bayes_phoff : the same with PHOFF free;
* bayes_wb    : wideband, 300 TOAs; EFAC, EQUAD, DMEFAC, DMEQUAD, DMJUMP and 20 free DMX bins.

Each holds 16 points within +-3 sigma of the reference's fit (noise parameters within +-30 %) with the
reference's lnlikelihood, its four terms, lnprior, lnposterior and per-point time residuals.  The
reference orders the free noise parameters differently from this package (both keep par-file order
within a component); the tests match columns by name.

Bars.  Residuals: the project's 1 ns.  lnL and chi2_toa against the reference: golden_util.chi2_bar's
rule on bayes_spread.json -- 2 x the reference's own per-ps |delta lnL| (|delta chi2|) of that point x
the measured residual rms difference clamped to 5-30 ps, at least 1e-9 relative.  The log sums: 1e-12
of the sum (300 terms of |log sigma| <= 52, each within a few ulps on both sides).  chi2_dm: no time
residual enters it, so its bar is the rounding of the modelled DM: both sides form a DM of ~|DM| from
a handful of float64 additions, so a row's z = (pp_dm - DM) / sigma carries at most delta = 8 eps
max|DM| / min sigma_dm on either side and |delta chi2_dm| <= 2 delta sum|z| <= 2 delta sqrt(n chi2_dm).
The new pass against the package's own single-point path: 1e-12 relative on each chi2 and 1e-12 of
each log sum (fixed-order double sums of <= 1025 same-sign terms: n eps ~ 2.3e-13).
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, grid_tables, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
NAMES = ("bayes_nb", "bayes_phoff", "bayes_wb")
LN_PCCM3_SI = float(np.log(3.0856775814913673e22))  # log(1 pc cm^-3 in m^-2)
_CACHE = {}


def load(name, par=None):
    """(model, toas, arrays, meta) of a fixture: the arrays, the meta and the TOAs are loaded once,
    shared and never changed; the model is a fresh one per caller."""
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    if name not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        fc = dict(meta["flag_columns"])
        if "wb_pp_dm" in z:  # the wideband -pp_dm / -pp_dme flags, as the tim file carries them
            fc["pp_dm"] = [repr(float(x)) for x in z["wb_pp_dm"]]
            fc["pp_dme"] = [repr(float(x)) for x in z["wb_pp_dme"]]
        _CACHE[name] = (from_arrays_with_tzr(z, fc, name, meta.get("obs_names")), z, meta)
    toas, z, meta = _CACHE[name]
    model = get_model(par if par is not None else os.path.join(GOLDEN, name + ".par"))
    if par is None:
        model.free_params = list(meta["model"]["free_params"])
    return model, toas, z, meta


def _par(name):
    return open(os.path.join(GOLDEN, name + ".par")).read()


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "bayes_spread.json")))
    return _CACHE["spread"]


def bayes(name, **kw):
    from pint_amd import BayesianTiming
    model, toas, z, meta = load(name)
    bt = BayesianTiming(model, toas, prior_info=meta["prior_info"], **kw)
    perm = [meta["labels"].index(p) for p in bt.param_labels]  # the reference's columns in this package's order
    return bt, z, meta, perm


def _pts(z, key, perm):
    return (z[key + "_hi"].astype(LD) + z[key + "_lo"].astype(LD))[:, perm]


def spread_bar(name, kind, k, ref, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule for point k, absolute: 2 x the reference's per-ps spread x the measured
    residual rms (at least 5 ps, at most the calibrated 30 ps), at least floor x |ref|."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind][k] / 5.0, d["30ps"][kind][k] / 30.0)
    return max(floor * abs(ref), 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def model_at(bt, point):
    """A copy of bt's model with the free parameters at `point`."""
    m = copy.deepcopy(bt.model)
    m.set_param_values(dict(zip(bt.param_labels, point)))
    return m


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on, on the committed files."""
    model, toas, z, meta = load(name)
    assert toas.ntoas == 300 and z["pts_hi"].shape == (16, len(meta["labels"]))
    assert meta["is_wideband"] == (name == "bayes_wb") and meta["likelihood_method"] == "wls"
    assert meta["track_mode"] == "nearest"
    assert ("PHOFF" in meta["labels"]) == (name == "bayes_phoff")
    assert np.max(z["pt_wrap"]) < 0.45  # no residual within 0.05 cycle of a wrap at any point
    sizes = meta["noise_class_sizes"]
    assert "none" in sizes and 1 in sizes.values()  # TOAs under no mask; a class of a single TOA
    if name != "bayes_wb":
        assert len(sizes) == 7 and sizes["EQUAD2"] == 1 and "EFAC1+EFAC2+EQUAD1" in sizes
        assert np.all(z["pt_chi2_dm"] == 0) and np.all(z["pt_lsig_dm"] == 0)
    else:
        assert {"DMEFAC1", "DMEQUAD1", "DMJUMP1", "EFAC1", "EQUAD1"} <= set(meta["labels"])
        assert sum(p.startswith("DMX_") for p in meta["labels"]) == 20
        assert np.all(z["pt_chi2_dm"] > 0)
        # the reference's log of the DM errors is of their SI value: log(3.0857e22) per TOA above pc/cm^3
        assert np.allclose(z["pt_lsig_dm"] - z["pt_lsig_dm_pccm3"], 300 * LN_PCCM3_SI, rtol=1e-13, atol=0)
    terms = -z["pt_chi2_toa"] / 2 - z["pt_lsig_toa"] - z["pt_chi2_dm"] / 2 - z["pt_lsig_dm"]
    assert np.allclose(terms, z["pt_lnl"], rtol=1e-12, atol=0)
    assert np.allclose(z["pt_lnprior"] + z["pt_lnl"], z["pt_lnposterior"], rtol=1e-12, atol=0)
    assert np.all(np.isfinite(z["pt_lnprior"])) and np.all(np.isneginf(z["out_lnprior"]))
    sp = _spread()[name]
    for lev in ("5ps", "30ps"):
        for kind in ("lnl", "chi2_toa"):
            v = np.asarray(sp[lev][kind])
            assert v.shape == (16,) and np.all(np.isfinite(v)) and np.all(v > 0)
    assert sp["ref_seconds_per_lnlikelihood"] > 0


def test_priors():
    from scipy.stats import norm, uniform
    from pint_amd.priors import (Prior, UniformUnboundedRV, UniformBoundedRV, GaussianBoundedRV,
                                 RandomInclinationPrior)
    x = np.array([-3.0, 0.25, 1.0, 7.5])
    p = Prior(UniformUnboundedRV())
    assert np.all(p.pdf(x) == 1.0) and np.all(p.logpdf(x) == 0.0) and p.logpdf(LD(2)) == 0.0
    p = Prior(UniformBoundedRV(0.5, 2.0))
    assert np.array_equal(p.logpdf(x), uniform(0.5, 1.5).logpdf(x))
    assert np.isneginf(p.logpdf(0.4)) and np.isneginf(p.logpdf(2.1)) and p.pdf(1.0) == pytest.approx(1 / 1.5, rel=1e-15)
    assert p.ppf(0.5) == pytest.approx(1.25, rel=1e-15) and p.ppf(0.0) == 0.5 and p.ppf(1.0) == 2.0
    assert isinstance(p.logpdf(LD(1)), float) or np.ndim(p.logpdf(LD(1))) == 0
    g = Prior(GaussianBoundedRV(loc=0.9, scale=0.1, lower_bound=0.0, upper_bound=1.0))
    # the reference's meaning: the normal density inside the bounds (not renormalised there), 0 outside
    assert np.allclose(g.pdf(np.array([0.5, 0.9, 0.99])), norm(0.9, 0.1).pdf(np.array([0.5, 0.9, 0.99])), rtol=1e-13)
    assert g.logpdf(0.8) == pytest.approx(norm(0.9, 0.1).logpdf(0.8), rel=1e-13)
    assert g.pdf(1.01) == 0.0 and g.pdf(-0.01) == 0.0 and np.isneginf(g.logpdf(1.5))
    assert 0.0 <= g.ppf(0.3) <= 1.0
    r = Prior(RandomInclinationPrior())
    s = np.array([0.1, 0.5, 0.9])
    assert np.allclose(r.pdf(s), s / np.sqrt(1 - s * s), rtol=1e-13)
    assert np.allclose(r.logpdf(s), np.log(s / np.sqrt(1 - s * s)), rtol=1e-12, atol=1e-15)
    assert r.pdf(1.2) == 0.0 and np.allclose(np.sqrt(1 - r.ppf(s) ** 2), 1 - s, rtol=1e-12)  # cos i uniform
    n = Prior(norm(1.0, 2.0))
    assert n.logpdf(LD("1.5")) == norm(1.0, 2.0).logpdf(1.5)


def test_param_prior_and_set_param_values():
    from pint_amd.priors import Prior, UniformUnboundedRV, UniformBoundedRV
    model, _, _, _ = load("bayes_nb")
    assert isinstance(model.F0.prior, Prior) and isinstance(model.F0.prior._rv, UniformUnboundedRV)
    assert model.F0.prior_pdf() == 1.0 and model.F0.prior_pdf(logpdf=True) == 0.0
    with pytest.raises(ValueError, match=r"prior must be an instance of Prior\(\)"):
        model.F0.prior = 3.0
    model.A1.prior = Prior(UniformBoundedRV(0.0, 10.0))
    assert model.A1.prior_pdf(5.0) == pytest.approx(0.1, rel=1e-15) and np.isneginf(model.A1.prior_pdf(11.0, logpdf=True))
    assert copy.deepcopy(model).A1.prior_pdf(5.0) == pytest.approx(0.1, rel=1e-15)
    # a float lands exactly in long-double and MJD parameters; a longdouble keeps all its bits
    f0, tasc = 345.678901234567, 54801.123456789
    model.set_param_values({"F0": f0, "TASC": tasc, "A1": np.float64(3.25), "EFAC1": 1.5})
    assert type(model.F0.value) is LD and model.F0.value == LD(f0) and float(model.F0.value) == f0
    assert type(model.TASC.value) is LD and model.TASC.value == LD(tasc)
    assert type(model.A1.value) is float and model.A1.value == 3.25 and model.EFAC1.value == 1.5
    v = LD(f0) + LD(2) ** -50  # (below a double's ulp at 345, above a longdouble's)
    assert v != LD(f0) and float(v) == f0
    model.set_param_values({"F0": v, "PEPOCH": LD(54800) + LD(2) ** -40})
    assert model.F0.value == v and model.PEPOCH.value == LD(54800) + LD(2) ** -40
    with pytest.raises(KeyError):
        model.set_param_values({"NOSUCH": 1.0})


@pytest.mark.parametrize("name", NAMES)
def test_attributes_and_priors_against_the_reference(name):
    """Construction needs no device; lnprior and prior_transform are scipy on both sides: 1e-13."""
    bt, z, meta, perm = bayes(name)
    assert bt.param_labels == bt.model.free_params and sorted(bt.param_labels) == sorted(meta["labels"])
    assert bt.nparams == len(meta["labels"]) and [p.name for p in bt.params] == bt.param_labels
    assert bt.is_wideband == meta["is_wideband"] and bt.track_mode == "nearest" and bt.likelihood_method == "wls"
    assert bt.toas is load(name)[1] and bt.model is not load(name)[0]
    pts = _pts(z, "pts", perm)
    assert np.allclose(bt.lnprior_batch(pts), z["pt_lnprior"], rtol=1e-13, atol=0)
    assert np.allclose(bt.lnprior_batch(pts.astype(np.float64)), z["pt_lnprior"], rtol=1e-13, atol=0)
    assert bt.lnprior(pts[3]) == bt.lnprior_batch(pts)[3]
    out = _pts(z, "out", perm)
    assert np.all(np.isneginf(bt.lnprior_batch(out))) and bt.lnprior(out[0]) == -np.inf
    cube = z["cube"][:, perm]
    got = bt.prior_transform_batch(cube)
    assert got.dtype == np.float64 and np.allclose(got, z["cube_transform"][:, perm], rtol=1e-13, atol=0)
    assert np.array_equal(bt.prior_transform(cube[5]), got[5])
    assert np.allclose(bt.lnprior_batch(got), z["cube_lnprior"], rtol=1e-13, atol=0)
    # a NaN log-prior counts as -inf
    bad = pts.copy()
    bad[2, 0] = np.nan
    lp = bt.lnprior_batch(bad)
    assert np.isneginf(lp[2]) and np.all(np.isfinite(np.delete(lp, 2)))


@pytest.mark.parametrize("name", ("bayes_nb", "bayes_phoff"))
def test_refused_forms(name):
    """The reference's refusals, by class and message (recorded under "forms")."""
    from pint_amd import BayesianTiming, get_model
    model, toas, z, meta = load(name)
    forms, pi = meta["forms"], meta["prior_info"]
    first = meta["labels"][0]
    cases = {"distr_lognormal": lambda: BayesianTiming(model, toas, prior_info={**pi, first: {"distr": "lognormal", "mu": 0.0, "sigma": 1.0}}),
             "unbounded_" + first: lambda: BayesianTiming(model, toas, prior_info={k: v for k, v in pi.items() if k != first})}
    bt = BayesianTiming(model, toas, prior_info=pi)
    cases["wrong_length_lnprior"] = lambda: bt.lnprior(np.zeros(bt.nparams + 1))
    cases["wrong_length_lnposterior"] = lambda: bt.lnposterior(np.zeros(bt.nparams - 1))
    for key, extra in (("ecorr", "ECORR mjd 53000 56700 0.5\n"), ("plrednoise", "TNRedAmp -13.8\nTNRedGam 4.1\nTNRedC 10\n"),
                       ("pldmnoise", "TNDMAMP -13.2\nTNDMGAM 2.8\nTNDMC 10\n")):
        m = get_model(_par(name) + extra)
        cases["correlated_" + key] = lambda m=m: BayesianTiming(m, toas, prior_info=pi)

    def not_prior():
        copy.deepcopy(model).F0.prior = 3.0
    cases["prior_setter_float"] = not_prior
    assert set(cases) == set(forms)
    builtins = {"NotImplementedError": NotImplementedError, "IndexError": IndexError, "ValueError": ValueError}
    for key, fn in cases.items():
        with pytest.raises(builtins[forms[key]["error"]]) as e:
            fn()
        assert type(e.value).__name__ == forms[key]["error"] and str(e.value) == forms[key]["message"], key
    # the batch forms refuse a wrong width with the same class
    for fn in (bt.lnprior_batch, bt.prior_transform_batch, bt.lnposterior_batch, bt.lnlikelihood_batch):
        with pytest.raises(IndexError):
            fn(np.zeros((4, bt.nparams + 1)))
    # a free parameter without a table slot that is no white-noise parameter is named
    m = get_model(_par(name) + "ECORR mjd 53000 56700 0.5 1\n")
    m.components.pop("EcorrNoise")  # (so that the correlated-noise refusal does not come first)
    with pytest.raises(NotImplementedError, match="ECORR1"):
        BayesianTiming(m, toas, prior_info={**pi, "ECORR1": {"distr": "uniform", "pmin": 0.1, "pmax": 1.0}})


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(name):
    """lnL, its four terms, lnprior + lnL and the per-point residuals over the fixture's 16 points."""
    from pint_amd import Residuals
    bt, z, meta, perm = bayes(name)
    pts = _pts(z, "pts", perm)
    terms = bt.lnlikelihood_terms_batch(pts)
    post = bt.lnposterior_batch(pts)
    assert terms.shape == (16, 5) and post.dtype == np.float64
    n = bt.toas.ntoas
    for k in range(16):
        r = Residuals(bt.toas, model_at(bt, pts[k]))
        dr = np.max(np.abs(r.time_resids - z["pt_time"][k]))
        rms = rms_ps(r.time_resids, z["pt_time"][k])
        lnl, c2, ls, c2d, lsd = terms[k]
        print(f"{name}[{k}]: max |dr| {dr:.3e} s, rms {rms:.2f} ps; dlnL {lnl - z['pt_lnl'][k]:+.3e} "
              f"(bar {spread_bar(name, 'lnl', k, z['pt_lnl'][k], rms):.3e}); dchi2_toa {c2 - z['pt_chi2_toa'][k]:+.3e}; "
              f"dlsig_toa {ls - z['pt_lsig_toa'][k]:+.3e}; dchi2_dm {c2d - z['pt_chi2_dm'][k]:+.3e}; "
              f"dlsig_dm {lsd - z['pt_lsig_dm'][k]:+.3e}")
        assert dr < 1e-9, (k, dr)
        assert abs(lnl - z["pt_lnl"][k]) <= spread_bar(name, "lnl", k, z["pt_lnl"][k], rms), k
        assert abs(c2 - z["pt_chi2_toa"][k]) <= spread_bar(name, "chi2_toa", k, z["pt_chi2_toa"][k], rms), k
        assert abs(ls - z["pt_lsig_toa"][k]) <= 1e-12 * abs(z["pt_lsig_toa"][k]), k
        if name == "bayes_wb":
            sig_min = float(np.min(bt.toas.get_dm_errors())) * 0.1 * 0.7  # (DMEFAC >= 0.7 x 1.3, errors only grow with DMEQUAD)
            delta = 8 * np.finfo(float).eps * (abs(float(bt.model.DM.value)) + 1.0) / sig_min
            assert abs(c2d - z["pt_chi2_dm"][k]) <= 2 * delta * np.sqrt(n * z["pt_chi2_dm"][k]), k
            assert abs(lsd - z["pt_lsig_dm"][k]) <= 1e-12 * abs(z["pt_lsig_dm"][k]), k
        else:
            assert c2d == 0.0 and lsd == 0.0
        assert abs(post[k] - z["pt_lnposterior"][k]) <= spread_bar(name, "lnl", k, z["pt_lnposterior"][k], rms), k
    assert bt.lnlikelihood(pts[5]) == terms[5, 0] and bt.lnposterior(pts[5]) == post[5]  # the scalar forms: N = 1
    out = _pts(z, "out", perm)
    assert np.all(np.isneginf(bt.lnposterior_batch(out)))
    bt.close()


def _subset(name, n):
    """A synthetic pulsar of n rows: the fixture's TOAs in order, taken round and round."""
    toas = load(name)[1]
    return toas[np.arange(n) % toas.ntoas]


def _noise_lines(kind, mjd):
    """EFAC / EQUAD lines on MJD ranges of the sorted MJDs `mjd`: no mask at all; two overlapping ranges
    (four classes: none, EFAC, EFAC + EQUAD, EQUAD); an EFAC over everything and an EQUAD on the first
    TOA alone (a class of a single TOA while the rows are distinct)."""
    n = len(mjd)
    lo, hi = mjd[0] - 1.0, mjd[-1] + 1.0
    mid = lambda k: 0.5 * (mjd[k - 1] + mjd[k]) if 0 < k < n else (lo if k <= 0 else hi)  # noqa: E731
    if kind == "none":
        return "", []
    if kind == "four":
        return (f"EFAC mjd {lo:.4f} {mid(n // 2):.4f} 1.2 1\nEQUAD mjd {mid(n // 4):.4f} {mid(3 * n // 4):.4f} 0.3 1\n",
                ["EFAC1", "EQUAD1"])
    return f"EFAC mjd {lo:.4f} {hi:.4f} 1.1 1\nEQUAD mjd {lo:.4f} {mid(1):.4f} 0.4 1\n", ["EFAC1", "EQUAD1"]


TIMING = ["F0", "F1", "A1", "EPS1"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("none", "four", "single"))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257, 513, 1025, 4097))
def test_new_pass_against_the_single_point_path(n, kind):
    """pint_point_lnlike against Residuals(toas, model_k).chi2 and scaled_toa_uncertainty, one point at
    a time, for N in {1, 2, 257} points of an n-row pulsar: 1e-12.  513 and 4097 rows are the first
    sizes of the 4-wave and the 8-wave build of the pass (a wave per point up to 512 rows); at 4097
    rows the bar is still above n eps = 9.1e-13."""
    from pint_amd import BayesianTiming, Residuals, get_model
    toas = _subset("bayes_nb", n)
    base = "\n".join(l for l in _par("bayes_nb").splitlines() if not l.startswith(("EFAC", "EQUAD"))) + "\n"
    lines, noise = _noise_lines(kind, np.sort(np.unique(toas.get_mjds())))
    model = get_model(base + lines)
    model.free_params = TIMING + noise
    sig = load("bayes_nb")[3]["fit_sigma"]
    pi = {p: {"distr": "uniform", "pmin": float(model[p].value) - 10 * sig[p], "pmax": float(model[p].value) + 10 * sig[p]}
          for p in TIMING}
    pi.update({p: {"distr": "uniform", "pmin": 0.05, "pmax": 5.0} for p in noise})
    bt = BayesianTiming(model, toas, prior_info=pi)
    assert bt.param_labels == TIMING + noise
    rng = np.random.default_rng(1000 * n + len(kind))
    for N in (1, 2, 257):
        pts = np.empty((N, bt.nparams), dtype=LD)
        for j, p in enumerate(bt.param_labels):
            if p in noise:
                pts[:, j] = float(model[p].value) * rng.uniform(0.7, 1.3, N)
            else:
                pts[:, j] = LD(model[p].value) + LD(sig[p]) * rng.uniform(-2, 2, N).astype(LD)
        terms = bt.lnlikelihood_terms_batch(pts)
        for k in sorted({0, N - 1, N // 2, min(N - 1, 63), min(N - 1, 64)}):
            mk = model_at(bt, pts[k])
            r = Residuals(toas, mk)
            ls = float(np.sum(np.log(mk.scaled_toa_uncertainty(toas) * 1e-6)))
            # (one row: its residual is its own mean, chi2 is the square of a rounding error of z ~ 1e-16
            # on either side, which the 1e-12 bar on z itself covers: 1e-24)
            assert abs(terms[k, 1] - r.chi2) <= 1e-12 * abs(r.chi2) + (1e-24 if n == 1 else 0.0), (N, k, terms[k, 1], r.chi2)
            assert abs(terms[k, 2] - ls) <= 1e-12 * abs(ls), (N, k, terms[k, 2], ls)
            assert terms[k, 3] == 0.0 and terms[k, 4] == 0.0
            assert terms[k, 0] == -0.5 * terms[k, 1] - terms[k, 2]
    bt.close()


@pytest.mark.gpu
def test_new_pass_wideband_against_the_single_point_path():
    """The DM side: WidebandDMResiduals(toas, model_k).chi2 and scaled_dm_sigma, N in {1, 2, 257}."""
    from pint_amd import Residuals, WidebandDMResiduals
    from pint_amd.noise import scaled_dm_sigma
    bt, z, meta, perm = bayes("bayes_wb")
    ref = _pts(z, "pts", perm)
    rng = np.random.default_rng(7)
    for N in (1, 2, 257):
        pts = ref[rng.integers(0, 16, N)].copy()
        for j, p in enumerate(bt.param_labels):  # fresh noise values per point
            if p.startswith(("EFAC", "EQUAD", "DMEFAC", "DMEQUAD")):
                pts[:, j] = float(bt.model[p].value) * rng.uniform(0.7, 1.3, N)
        terms = bt.lnlikelihood_terms_batch(pts)
        for k in sorted({0, N - 1, N // 2}):
            mk = model_at(bt, pts[k])
            r, d = Residuals(bt.toas, mk), WidebandDMResiduals(bt.toas, mk)
            ls = float(np.sum(np.log(mk.scaled_toa_uncertainty(bt.toas) * 1e-6)))
            lsd = float(np.sum(np.log(scaled_dm_sigma(mk, bt.toas)))) + bt.toas.ntoas * LN_PCCM3_SI
            assert abs(terms[k, 1] - r.chi2) <= 1e-12 * abs(r.chi2), (N, k)
            assert abs(terms[k, 2] - ls) <= 1e-12 * abs(ls), (N, k)
            assert abs(terms[k, 3] - d.chi2) <= 1e-12 * abs(d.chi2), (N, k, terms[k, 3], d.chi2)
            assert abs(terms[k, 4] - lsd) <= 1e-12 * abs(lsd), (N, k)
    bt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nvar", (1, 17, "all"))
def test_set_points_tables_and_reuse(nvar):
    """pint_set_points forms the tables golden_util.grid_tables forms on the host, bit for bit, for 1, 17
    and every table parameter; a second call with the same N keeps the resident batch (PINT_QUERY_NREUSE)
    and gives the bits a fresh session gives."""
    from pint_amd.engine import Session, build_layout, pack_table
    model, toas, z, meta = load("bayes_wb")

    def session():
        s = Session()
        lay = s.add(build_layout(model, toas, use_gls_basis=False))
        return s, lay

    s, lay = session()
    names = list(lay.offsets) if nvar == "all" else [p for p in model.free_params if p in lay.offsets][:nvar]
    assert len(names) == (lay.tstride // 2 if nvar == "all" else nvar) and (nvar != "all" or len(names) > 16)
    t0 = pack_table(lay, model)
    N = 37

    def points(seed):
        r = np.random.default_rng(seed)
        v = np.empty((N, len(names)), dtype=LD)
        for j, p in enumerate(names):
            x = LD(0) if model[p].value is None else LD(model[p].value)
            v[:, j] = x + (abs(x) * LD(1e-9) + LD(1e-30)) * r.uniform(-1, 1, N).astype(LD)
        return v

    def expect(v):
        return grid_tables(lay, (t0, [(p, v[:, j], 1, N) for j, p in enumerate(names)], N, 0))

    v1, v2 = points(1), points(2)
    assert np.any(v1 != v1.astype(np.float64).astype(LD))  # (the points need their lo words)
    s.set_points(lay, t0, names, v1)
    assert s.n_batch_reuse() == 0
    assert np.array_equal(s.read_tables_flat().reshape(N, lay.tstride), expect(v1))
    s.eval(False)
    first = np.array(s.read_resids()[2])
    s.set_points(lay, t0, names, v2)
    assert s.n_batch_reuse() == 1
    assert np.array_equal(s.read_tables_flat().reshape(N, lay.tstride), expect(v2))
    s.eval(False)
    got = np.array(s.read_resids()[2])
    s.set_points(lay, t0, names, v2[:5])  # another point count: a fresh batch
    assert s.n_batch_reuse() == 1
    assert np.array_equal(s.read_tables_flat().reshape(5, lay.tstride), expect(v2)[:5])
    s.close()
    f, flay = session()
    f.set_points(flay, t0, names, v2)
    f.eval(False)
    fresh = np.array(f.read_resids()[2])
    f.close()
    assert np.array_equal(got, fresh) and not np.array_equal(got, first)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_consistency(name):
    """A point equal to the base model gives pint_read_resids' own chi2 (1e-12); the same batch twice is
    bit-identical, whatever ran in between."""
    bt, z, meta, perm = bayes(name)
    pts = _pts(z, "pts", perm)
    batch = np.vstack([bt._base_values[None, :], pts])
    a = bt.lnlikelihood_terms_batch(batch)
    own = np.array(bt._device().read_resids()[2])
    assert abs(a[0, 1] - own[0]) <= 1e-12 * own[0], (a[0, 1], own[0])
    bt.lnlikelihood_terms_batch(pts[::-1])
    b = bt.lnlikelihood_terms_batch(batch)
    assert np.array_equal(a, b)
    bt.close()


@pytest.mark.gpu
def test_lnposterior_minus_inf_and_nan():
    """-inf exactly where the prior is -inf (those points run at the base values); NaN for a point the
    prior allows and the device flags: ECC >= 1."""
    from golden_util import load as gload
    from pint_amd import BayesianTiming, get_model
    _, toas, _, _ = gload("pta_dd")
    par = "\n".join(l for l in _par("pta_dd").splitlines() if not l.startswith(("TNRed", "TNRED"))) + "\n"
    model = get_model(par)
    model.free_params = ["F0", "ECC"]
    f0, ecc = float(model.F0.value), float(model.ECC.value)
    bt = BayesianTiming(model, toas, prior_info={"F0": {"distr": "uniform", "pmin": f0 - 1e-9, "pmax": f0 + 1e-9},
                                                 "ECC": {"distr": "uniform", "pmin": 0.0, "pmax": 2.0}})
    pts = np.array([[f0, ecc], [f0, 1.5], [f0 + 1.0, ecc], [f0, 2.5], [f0, ecc], [np.nan, ecc]])
    post = bt.lnposterior_batch(pts)
    assert np.isfinite(post[0]) and post[4] == post[0]
    assert np.isnan(post[1])
    assert np.isneginf(post[2]) and np.isneginf(post[3]) and np.isneginf(post[5])
    assert np.isnan(bt.lnposterior(pts[1])) and bt.lnposterior(pts[3]) == -np.inf
    like = bt.lnlikelihood_batch(pts[:2])
    assert np.isfinite(like[0]) and np.isnan(like[1])
    assert bt.lnposterior_batch(pts[:1])[0] == post[0]  # the flagged neighbours left it alone
    bt.close()


@pytest.mark.gpu
def test_entry_point_errors():
    """PINT_E_INVALID with a message, before any launch; the batch works afterwards."""
    from pint_amd import _lib as L
    from pint_amd.engine import Session, build_layout, pack_table
    from pint_amd.noisefit import white_noise_classes
    lib = L.lib()
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731

    def err(s, rc, text):
        assert rc == L.PINT_E_INVALID, rc
        assert text in lib.pint_last_error(s.ctx).decode(), lib.pint_last_error(s.ctx).decode()

    model, toas, _, _ = load("bayes_wb")
    nb_model, nb_toas, _, _ = load("bayes_nb")
    s = Session()
    lay = s.add(build_layout(model, toas, use_gls_basis=False))
    nbl = s.add(build_layout(nb_model, nb_toas, use_gls_basis=False))
    t0 = pack_table(lay, model)
    ts = lay.tstride
    vals = np.zeros(2 * 4 * 3)
    sp = lambda psr, npts, nvar, toff: lib.pint_set_points(s.ctx, psr, npts, L.ptr(t0), nvar, L.ptr(i32(toff), C.c_int32), L.ptr(vals))  # noqa: E731
    err(s, sp(99, 4, 1, [0]), "bad pulsar id")
    err(s, sp(lay.psr_id, 4, 1, [ts - 1]), "bad variable")
    err(s, sp(lay.psr_id, 4, 1, [-2]), "bad variable")
    err(s, sp(lay.psr_id, 4, 2, [4, 4]), "bad variable")      # the same entries twice
    err(s, sp(lay.psr_id, 4, 2, [4, 5]), "bad variable")      # overlapping pairs
    assert lib.pint_set_points(s.ctx, lay.psr_id, 0, L.ptr(t0), 0, None, None) == L.PINT_E_INVALID
    assert lib.pint_set_points(s.ctx, lay.psr_id, 4, L.ptr(t0), 1, None, L.ptr(vals)) == L.PINT_E_INVALID
    big = i32(np.arange(ts))
    err(s, lib.pint_set_points(s.ctx, lay.psr_id, 1, L.ptr(t0), ts, L.ptr(big, C.c_int32), L.ptr(np.zeros(2 * ts))),
        "more variables than table entries")
    # DM classes: a pulsar without wideband data, lists that do not cover the TOAs once
    ptr, idx, _, _ = white_noise_classes(model, toas, "DMEFAC", "DMEQUAD")
    dme = np.ascontiguousarray(toas.get_dm_errors(), dtype=np.float64)
    dmc = lambda psr, p, i, e: lib.pint_set_dm_noise_classes(s.ctx, psr, len(p) - 1, L.ptr(i32(p), C.c_int32), L.ptr(i32(i), C.c_int32), L.ptr(e))  # noqa: E731
    err(s, dmc(lay.psr_id, ptr, idx, dme), "no wideband DM data")
    s.set_wideband(lay)
    err(s, dmc(nbl.psr_id, ptr, idx, dme), "no wideband DM data")
    twice = np.array(idx).copy()
    twice[1] = twice[0]
    err(s, dmc(lay.psr_id, ptr, twice, dme), "cover every TOA once")
    err(s, dmc(lay.psr_id, np.array(ptr)[:-1], idx, dme), "cover every TOA once")
    err(s, dmc(lay.psr_id, ptr, idx, dme * 0.0), "DM uncertainty must be > 0")
    # the likelihood: no classes, no DM classes, NULL DM values, wrong counts
    N = 3
    s.set_points(lay, t0, ["F0"], np.full((N, 1), LD(model.F0.value)))
    s.eval(False)
    out = np.full(5 * N, -1.0)
    tp, ti, _, _ = white_noise_classes(model, toas)
    ncl, ndc = len(tp) - 1, len(ptr) - 1
    qf = np.tile([0.0, 1.0], N * ncl)
    dqf = np.tile([0.0, 1.0], N * ndc)
    pl = lambda a, q, b, d: lib.pint_point_lnlike(s.ctx, a, L.ptr(q), b, None if d is None else L.ptr(d), L.ptr(out))  # noqa: E731
    err(s, pl(N * ncl, qf, N * ndc, dqf), "no noise classes")
    s.set_noise_classes(lay, tp, ti, toas.get_errors())
    err(s, pl(N * ncl, qf, N * ndc, dqf), "without DM noise classes")
    s.set_dm_noise_classes(lay, ptr, idx, dme)
    err(s, pl(N * ncl, qf, 0, None), "without DM class values")
    err(s, pl(N * ncl - 1, qf, N * ndc, dqf), "class count does not match")
    err(s, pl(N * ncl, qf, N * ndc + 2, dqf), "class count does not match")
    assert lib.pint_point_lnlike(s.ctx, N * ncl, None, N * ndc, L.ptr(dqf), L.ptr(out)) == L.PINT_E_INVALID
    assert np.all(out == -1.0)  # nothing ran
    assert pl(N * ncl, qf, N * ndc, dqf) == 0
    got = out.reshape(N, 5)
    assert np.all(np.isfinite(got)) and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    assert got[0, 0] == -0.5 * got[0, 1] - got[0, 2] - 0.5 * got[0, 3] - got[0, 4]
    s.close()


@pytest.mark.gpu
def test_use_pulse_numbers_computes_them_from_the_initial_model():
    """TOAs without pulse numbers get them from the initial model's device phase; the likelihood at the
    fixture's points is then that of the nearest-integer tracking (no residual is near a wrap)."""
    from pint_amd import BayesianTiming
    from pint_amd.toa import TOAs
    model, shared, z, meta = load("bayes_nb")
    # a copy without the pulse numbers the simulated TOAs carry (the shared TOAs stay as they are)
    toas = TOAs({k: np.array(v) for k, v in shared.arrays.items() if k != "pulse_number"},
                {k: list(v) for k, v in shared.flag_columns.items()}, shared.tzr, shared.name, shared.obs)
    assert toas.get_pulse_numbers() is None and shared.get_pulse_numbers() is not None
    bt = BayesianTiming(model, toas, use_pulse_numbers=True, prior_info=meta["prior_info"])
    pn = toas.get_pulse_numbers()
    assert bt.track_mode == "use_pulse_numbers" and pn is not None and np.all(pn == np.round(pn)) and np.ptp(pn) > 1e9
    # the reference's own pulse numbers of these TOAs (its simulation's model; residuals far from half a turn)
    assert np.array_equal(pn, z["pulse_number"])
    near, _, _, perm = bayes("bayes_nb")
    pts = _pts(z, "pts", perm)
    a, b = bt.lnlikelihood_terms_batch(pts), near.lnlikelihood_terms_batch(pts)
    assert np.allclose(a[:, 1], b[:, 1], rtol=1e-9, atol=0) and np.array_equal(a[:, 2], b[:, 2])
    bt.close()
    near.close()
