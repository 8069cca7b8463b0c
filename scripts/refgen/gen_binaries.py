"""Golden fixtures for the DDS, DDH and ELL1k binary models (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* dds_wls, ddh_wls, ell1k_wls : WLS.  An isolated-pulsar base (equatorial astrometry, DM) with
            the binary block, 300 TOAs at 1400 / 800 MHz from the geocentre over MJD 54500-55600,
            1 us errors (300 rows: a partial second 256-thread block).  Every binary parameter
            of the model is free, except ELL1k's M2 / SINI (frozen, non-zero).  Captured from a
            start moved off the truth in the free binary parameters together, inside their 1-sigma
            ellipsoid and by at most 1e-3 of each value.
            Beside what gen_synth.capture(fit="wls") records: the post-fit as_parfile(), the TZR
            TOA's binary delay, what the reference does with the par lines it rejects or
            rewrites ("forms"), and a 5x5 grid_chisq over (M2, SHAPMAX) / (H3, STIGMA) around the
            reference's Downhill result ("grid_base").
* ddh_gls, ell1k_gls : GLS.  gen_synth.pta_par(seed, "") (DMX, PLRedNoise, EFAC/EQUAD) with the
            binary block appended, 1000 TOAs in four bands.
* bin_fit_spread.json : gen_fit_spread.measure of the five fixtures plus the Downhill spread, in
            fdj_fit_spread.json's schema.

Two derivative defects of the reference are corrected in this process (PATCHES): the STIGMA
column of DDHmodel.d_delayS_d_par carries a stray 1 / Tsun, and ELL1kmodel.d_eps2_d_EPS2 has the
wrong sign.  Every fixture names the corrections ("reference_patches"), keeps the as-is STIGMA /
EPS2 column beside the corrected one (asis_col_*), and `verify` asserts that nothing else moves,
that the corrected STIGMA column is the as-is one times Tsun, and that each corrected column
agrees with the reference's numerical derivative.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_binaries.py [dds_wls ddh_wls ell1k_wls ddh_gls ell1k_gls spread]
"""
import contextlib
import copy
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle", "refgen"))

import astropy.units as u  # noqa: E402
import refcommon  # noqa: E402
from refcommon import GOLDEN, register_clockless_sites, split_ld  # noqa: E402
import gen_synth  # noqa: E402
from gen_synth import pta_par, capture  # noqa: E402  (the real capture: gen_fit_spread replaces the module's)
import pint  # noqa: E402
import pint.simulation as sim  # noqa: E402
import pint.fitter as pfit  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.gridutils import grid_chisq  # noqa: E402
from pint.models.stand_alone_psr_binaries.DDH_model import DDHmodel  # noqa: E402
from pint.models.stand_alone_psr_binaries.ELL1k_model import ELL1kmodel  # noqa: E402

from gen_solar_wind import write_par, downhill_spread  # noqa: E402
from gen_chromatic import check_errors  # noqa: E402
from gen_fdjump import save, parlines  # noqa: E402
import pint.residuals as pres  # noqa: E402
import gen_fit_spread  # noqa: E402  (replaces gen_synth.capture: `capture` above is the real one)

PATCHES = {
    "DDHmodel.d_delayS_d_par": "the STIGMA column times Tsun (both terms of dsDelay_dSTIGMA carry a stray / Tsun.value)",
    "ELL1kmodel.d_eps2_d_EPS2": "+d_eps1_d_EPS1() (the reference returns -d_eps1_d_EPS1())",
}
CORRECTED = {"DDH": "STIGMA", "ELL1k": "EPS2"}
_DDH_ASIS = DDHmodel.d_delayS_d_par
_ELL1K_ASIS = ELL1kmodel.d_eps2_d_EPS2


def _ddh_delayS(self, par):
    d = _DDH_ASIS(self, par)
    return d * pint.Tsun.value if par == "STIGMA" else d


def _ell1k_eps2(self):
    return self.d_eps1_d_EPS1()


def patch(on=True):
    DDHmodel.d_delayS_d_par = _ddh_delayS if on else _DDH_ASIS
    ELL1kmodel.d_eps2_d_EPS2 = _ell1k_eps2 if on else _ELL1K_ASIS


@contextlib.contextmanager
def as_is():
    patch(False)
    try:
        yield
    finally:
        patch(True)


BASE = """PSR J1012-BIN
RAJ 10:12:33.4372 1
DECJ 53:07:02.512 1
F0 218.8118404 1
F1 -4.08e-16 1
PEPOCH 55000
POSEPOCH 55000
DM 9.0233 1
EPHEM builtin
CLK TT(TAI)
UNITS TDB
TZRMJD 55400.1234
TZRFRQ 1400
TZRSITE geocenter
"""
DD_BLOCK = """PB 1.53449474406 1
A1 9.2307805 1
T0 {t0} 1
ECC 0.17 1
OM 110.0 1
OMDOT 0.01 1
GAMMA 1e-4 1
"""
BLOCKS = {
    "DDS": "BINARY DDS\n" + DD_BLOCK + "M2 0.3 1\nSHAPMAX 3.0 1\n",
    "DDH": "BINARY DDH\n" + DD_BLOCK + "H3 1.2e-6 1\nSTIGMA 0.75 1\n",
    "ELL1k": "BINARY ELL1k\nPB 0.3 1\nA1 1.9 1\nTASC {t0} 1\nEPS1 1e-3 1\nEPS2 -2e-3 1\nOMDOT 20.0 1\n"
             "LNEDOT 1e-3 1\nM2 0.25\nSINI 0.9\n",
}
GRID_SPANS = (2.0, 1.0, 0.5, 0.25, 0.1)
GRID = {"DDS": (("M2", u.Msun), ("SHAPMAX", u.dimensionless_unscaled)),
        "DDH": (("H3", u.s), ("STIGMA", u.dimensionless_unscaled))}
FIXTURES = {"dds_wls": ("DDS", "wls", 81), "ddh_wls": ("DDH", "wls", 82), "ell1k_wls": ("ELL1k", "wls", 83),
            "ddh_gls": ("DDH", "gls", 31), "ell1k_gls": ("ELL1k", "gls", 32)}


def true_par(binary, fit, seed):
    if fit == "wls":
        return BASE + BLOCKS[binary].format(t0="55000.123")
    return pta_par(seed, "") + BLOCKS[binary].format(t0="54801.987654321")


def binary_free(model):
    comp = [c for n, c in model.components.items() if n.startswith("Binary")][0]
    return [p for p in model.free_params if p in comp.params]


def make_toas(true, fit, seed):
    np.random.seed(seed)
    if fit == "wls":
        return sim.make_fake_toas_uniform(54500, 55600, 300, true, freq=np.array([1400.0, 800.0]) * u.MHz,
                                          obs="geocenter", error=1 * u.us, add_noise=True, include_bipm=False,
                                          multi_freqs_in_epoch=False)
    return sim.make_fake_toas_uniform(53000, 56652, 1000, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                      obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                      include_bipm=False, multi_freqs_in_epoch=False)


def build(name):
    """(par text of the start, its model, the TOAs): the TOAs are simulated from the true model, the
    start is the truth with the free binary parameters moved together, inside their 1-sigma
    ellipsoid (the covariance of one fit step from the truth) and by at most 1e-3 of each value."""
    binary, fit, seed = FIXTURES[name]
    par = true_par(binary, fit, seed)
    true = get_model(io.StringIO(par))
    ts = make_toas(true, fit, seed)
    if fit == "gls":
        true.find_empty_masks(ts, freeze=True)
    f = (pfit.GLSFitter if fit == "gls" else pfit.WLSFitter)(ts, copy.deepcopy(true))
    f.fit_toas(maxiter=1)
    # the move: 0.3 L z in the free binary parameters alone, L L^T their covariance with the other
    # parameters held (the inverse of the binary block of the inverse covariance), z alternating
    # +-1, scaled down where a parameter would move by more than 1e-3 of its value.  (A1 and GAMMA,
    # OM and T0 are nearly degenerate here: independent moves of a fraction of each marginal sigma
    # leave the chi2 surface's quadratic region by orders of magnitude.)
    names = list(f.parameter_covariance_matrix.get_label_names(axis=0))
    C = np.asarray(f.parameter_covariance_matrix.matrix, dtype=np.float64)
    free = binary_free(true)
    idx = [names.index(p) for p in free]
    D = np.sqrt(np.diag(C))
    for p, i in zip(free, idx):
        assert abs(D[i] / float(getattr(f.model, p).uncertainty_value) - 1) < 1e-6, p
    cond = np.linalg.inv(np.linalg.inv(C / np.outer(D, D))[np.ix_(idx, idx)])
    delta = 0.3 * (np.linalg.cholesky(cond) @ np.array([1.0 if k % 2 == 0 else -1.0 for k in range(len(idx))])) * D[idx]
    vals = np.array([abs(float(getattr(true, p).value)) for p in free])
    delta *= min(1.0, float(np.min(1e-3 * vals / np.abs(delta))))
    moved = {p: np.longdouble(getattr(true, p).value) + np.longdouble(d) for p, d in zip(free, delta)}
    out = []
    for line in par.splitlines():
        tok = line.split()
        if tok and tok[0] in moved and tok[-1] == "1":
            line = f"{tok[0]} {str(moved[tok[0]])} 1"
        out.append(line)
    par = "\n".join(out) + "\n"
    model = get_model(io.StringIO(par))
    if fit == "gls":
        model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def verify(model, ts, binary):
    """The assertions on the corrections; returns the as-is column and the recorded figures."""
    M, names, _ = model.designmatrix(ts)
    names = list(names)
    d1 = model.delay(ts).to_value(u.s)
    with as_is():
        M0, names0, _ = model.designmatrix(ts)
        d0 = model.delay(ts).to_value(u.s)
    assert list(names0) == names and np.array_equal(d0, d1)
    col = CORRECTED.get(binary)
    for j, n in enumerate(names):
        if n != col:
            assert np.array_equal(M[:, j], M0[:, j]), n  # (a) nothing else moves
    rec, arrays = {}, {}
    if col is not None:
        j = names.index(col)
        arrays["asis_col_" + col] = np.asarray(M0[:, j], dtype=np.float64)
        assert not np.array_equal(M[:, j], M0[:, j])
        if col == "STIGMA":  # (b)
            want = M0[:, j] * pint.Tsun.value
            assert np.all(np.abs(M[:, j] - want) <= np.spacing(np.abs(want))), "STIGMA column != as-is x Tsun"
        a = model.d_delay_d_param(ts, col).value
        num = model.d_delay_d_param_num(ts, col, step=1e-4).value
        err = float(np.max(np.abs(num - a)) / np.max(np.abs(a)))
        with as_is():
            a0 = model.d_delay_d_param(ts, col).value
        err0 = float(np.max(np.abs(num - a0)) / np.max(np.abs(a0)))
        print(f"  {col}: corrected column vs numerical {err:.2e} of its maximum (as-is {err0:.2e})", file=sys.stderr)
        assert err < 1e-4, err  # (c)
        rec = {"column": col, "num_rel_err": err, "asis_num_rel_err": err0}
    for n in binary_free(model):
        assert np.max(np.abs(M[:, names.index(n)])) > 0, n
    return arrays, rec


def fixed_point(model, ts, down_cls, step_cls):
    """gen_chromatic.fixed_point's figure, recorded and not bounded: how far one more plain fit step
    moves the reference's Downhill result, in sigma (the worst parameter).  SHAPMAX and STIGMA are
    strongly non-linear, and the reference's Downhill stops (chi2 decrease below its threshold) a few
    1e-3 sigma short of the fixed point in them; the tests' Downhill bar comes from the measured
    spread (bin_fit_spread.json "downhill")."""
    f = down_cls(ts, copy.deepcopy(model))
    f.fit_toas(maxiter=10)
    h = step_cls(ts, copy.deepcopy(f.model))
    h.fit_toas(maxiter=1)
    dev = {p: abs(float((getattr(h.model, p).value - getattr(f.model, p).value) / getattr(f.model, p).uncertainty_value))
           for p in f.model.free_params}
    pw = max(dev, key=dev.get)
    print(f"  Downhill result to one more step: {dev[pw]:.2e} sigma ({pw})", file=sys.stderr)
    return {"sigma": dev[pw], "param": pw, "all": dev}


def forms():
    """What the reference does with the par lines these models reject, ignore or rewrite."""
    par = {b: true_par(b, "wls", 0) for b in BLOCKS}

    def less(text, *names):
        return "".join(l + "\n" for l in text.splitlines() if l.split()[0] not in names)
    cases = {
        "ell1k_eps1dot": par["ELL1k"] + "EPS1DOT 1e-3\n",
        "ell1k_eps2dot": par["ELL1k"] + "EPS2DOT 1e-3\n",
        "ell1k_edot": par["ELL1k"] + "EDOT 1e-15\n",
        "ell1k_upper": par["ELL1k"].replace("BINARY ELL1k", "BINARY ELL1K"),
        "dds_sini": par["DDS"] + "SINI 0.9\n",
        "dds_shapmax_low": par["DDS"].replace("SHAPMAX 3.0", "SHAPMAX -0.7"),
        "dds_no_shapmax": less(par["DDS"], "SHAPMAX"),
        "ddh_m2": par["DDH"] + "M2 0.3\n",
        "ddh_sini": par["DDH"] + "SINI 0.9\n",
        "ddh_varsigma": par["DDH"].replace("STIGMA", "VARSIGMA"),
        "ddh_stig": par["DDH"].replace("STIGMA", "STIG"),
        "ddh_stigma_zero": par["DDH"].replace("STIGMA 0.75", "STIGMA 0.0"),
        "ddh_no_stigma": less(par["DDH"], "STIGMA"),
    }
    rec = {}
    for case, text in cases.items():
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            try:
                m = get_model(io.StringIO(text))
                comp = [c for n, c in m.components.items() if n.startswith("Binary")][0]
                vals = {}
                for n in comp.params:
                    try:
                        v = getattr(m, n).value
                        vals[n] = None if v is None else (str(v) if isinstance(v, (str, bool)) else float(v))
                    except Exception as e:  # (a funcParameter whose inputs are unset)
                        vals[n] = type(e).__name__
                rec[case] = {"result": "ok", "binary_params": list(comp.params), "values": vals,
                             "free": [n for n in m.free_params if n in comp.params],
                             "warnings": sorted({str(x.message) for x in w if "parfile line" in str(x.message)})}
            except Exception as e:  # (recorded: the tests reproduce what the reference does)
                rec[case] = {"result": type(e).__name__, "message": str(e)}
        rec[case]["par"] = text
    return rec


def with_save(name, more_arrays, more_meta):
    def _save(_, arrays, meta):
        arrays = dict(arrays)
        arrays.update(more_arrays)
        meta = dict(meta)
        meta.update(more_meta)
        assert meta["down_status"] == "converged" and meta["down_converged"], meta["down_status"]  # (d)
        save(name, arrays, meta)
    gen_synth.save = _save


def gen(name):
    binary, fit, _ = FIXTURES[name]
    par, model, ts = build(name)
    write_par(name, par)
    more, rec = verify(model, ts, binary)
    meta = {"reference_patches": PATCHES, "corrected": rec, "binary": binary,
            "binary_free": binary_free(model), "binary_component": "Binary" + binary}
    tz = model.get_TZR_toa(ts)
    more["tzr_binary_delay"] = refcommon.component_delays(model, tz)["delay_binarymodel_delay"]
    fcls, dcls = (pfit.GLSFitter, pfit.DownhillGLSFitter) if fit == "gls" else (pfit.WLSFitter, pfit.DownhillWLSFitter)
    f = fcls(ts, copy.deepcopy(model))
    chi2 = f.fit_toas(maxiter=1)
    check_errors(f)
    print(f"  {name}: {fit} chi2 {float(chi2):.3f} on {f.resids.dof} dof", file=sys.stderr)
    meta[fit + "_parfile"] = parlines(f.model)
    meta["start_parfile"] = parlines(model)
    meta["down_fixed_point"] = fixed_point(model, ts, dcls, fcls)
    if fit == "wls":
        meta["forms"] = forms()
        if binary in GRID:
            # the grid stands on the reference's Downhill result (a one-step fit from the start is
            # still ~100 in chi2 above the minimum for DDS: SHAPMAX is strongly non-linear, and a
            # grid of one-step fits from there would measure how the two codes' starts differ)
            (n0, u0), (n1, u1) = GRID[binary]
            fd = dcls(ts, copy.deepcopy(model))
            fd.fit_toas(maxiter=10)
            meta["grid_base"] = {p: list(map(float, split_ld(getattr(fd.model, p).value))) for p in fd.model.free_params}
            # ncpu=2: the reference's executor path (its default), where every point is fitted on a
            # copy of the base model (WrappedFitter.doonefit).  Its single-process path (ncpu=1)
            # fits the points one after another on the same fitter, each from the previous point's
            # fitted parameters: for SHAPMAX / STIGMA grids that is another, order-dependent
            # quantity (here up to 1.2e-5 of chi2 away), not what grid_chisq of the device path, a
            # batch of independent points, computes.
            # the half-width, in sigma: the largest of GRID_SPANS (less where M2 would cross zero: the
            # reference refuses M2 < 0) at which every point's one-step fit is converged by the
            # reference's own Downhill criterion, a second step gaining less than 1e-2 in chi2.
            # Further out the one-step chi2 lies tens above the point's minimum (SHAPMAX and STIGMA
            # are strongly non-linear, A1 / GAMMA and OM / T0 nearly degenerate) and follows the
            # rounding of the linear solve, not the model.
            for span in GRID_SPANS:
                axes = []
                for n in (n0, n1):
                    p = getattr(fd.model, n)
                    k = min(span, 0.8 * abs(float(p.value)) / float(p.uncertainty_value))
                    axes.append(np.longdouble(p.value) + np.linspace(-k, k, 5) * np.longdouble(p.uncertainty_value))
                assert np.all(axes[1] > 0), axes[1]
                grids = []
                for it in (1, 2):
                    fg = pfit.WLSFitter(ts, copy.deepcopy(fd.model))
                    grids.append(np.asarray(grid_chisq(fg, (n0, n1), (axes[0] * u0, axes[1] * u1), ncpu=2,
                                                       printprogress=False, maxiter=it)[0], dtype=np.float64))
                gain = float(np.max(grids[0] - grids[1]))
                # and no point's chi2 moves, under a 5 ps residual shift (gen_fit_spread's first two
                # patterns), by more than twice what the fixture's own one-step fit chi2 does under
                # the same shifts: the tests' bar is twice the spread measured on that fit, and
                # holds where the reference is as stable as there
                sens = np.zeros((5, 5))
                fit_sens = 0.0
                orig = pres.Residuals.calc_time_resids
                try:
                    for pat in gen_fit_spread.patterns(ts)[:2]:
                        shift = pat * 5e-12 * u.s
                        pres.Residuals.calc_time_resids = lambda self, *a, _s=shift, **k: orig(self, *a, **k) + _s
                        fg = pfit.WLSFitter(ts, copy.deepcopy(fd.model))
                        g = np.asarray(grid_chisq(fg, (n0, n1), (axes[0] * u0, axes[1] * u1), ncpu=2,
                                                  printprogress=False)[0], dtype=np.float64)
                        sens = np.maximum(sens, np.abs(g / grids[0] - 1))
                        fs = pfit.WLSFitter(ts, copy.deepcopy(model))
                        fit_sens = max(fit_sens, abs(float(fs.fit_toas(maxiter=1)) / float(chi2) - 1))
                finally:
                    pres.Residuals.calc_time_resids = orig
                print(f"  grid +-{span} sigma: a second step gains at most {gain:.3g} in chi2; 5 ps moves chi2 by at "
                      f"most {sens.max():.2e}, the one-step fit's by {fit_sens:.2e}", file=sys.stderr)
                if gain < 1e-2 and sens.max() <= 2 * fit_sens:
                    break
            else:
                raise SystemExit("no grid span with converged one-step fits")
            c2 = grids[0]
            # the chi2 at each point before its fit (the base model with the two grid values set)
            pre = np.zeros((5, 5))
            for i in range(5):
                for j in range(5):
                    m = copy.deepcopy(fd.model)
                    getattr(m, n0).value, getattr(m, n1).value = axes[0][i], axes[1][j]
                    pre[j, i] = float(pres.Residuals(ts, m).chi2)
            more["grid_pre_chi2"] = pre
            meta["grid_span_sigma"], meta["grid_second_step_gain"] = span, gain
            meta["grid_5ps_spread"] = {"max": float(sens.max()), "one_step_fit": fit_sens}
            for n, g in zip((n0, n1), axes):
                more[f"grid_{n}_hi"], more[f"grid_{n}_lo"] = split_ld(g)
            more["grid_chi2"] = np.asarray(c2, dtype=np.float64)
            meta["grid_params"] = [n0, n1]
            print(f"  grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
            assert np.all(np.isfinite(c2))
    with_save(name, more, meta)
    capture(name, model, ts, fit=fit)


def gen_spread(names):
    path = os.path.join(GOLDEN, "bin_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    for n in names:
        fit = FIXTURES[n][1]
        _, model, ts = build(n)
        gen_fit_spread.check_same(n, ts)
        res[n] = gen_fit_spread.measure(model, ts, fit, True)
        res[n]["downhill"] = downhill_spread(model, ts, pfit.DownhillGLSFitter if fit == "gls" else pfit.DownhillWLSFitter)
        print(n, json.dumps(res[n]), file=sys.stderr, flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    which = sys.argv[1:] or list(FIXTURES) + ["spread"]
    register_clockless_sites()
    patch(True)
    for n in FIXTURES:
        if n in which:
            gen(n)
    if "spread" in which:
        gen_spread([n for n in FIXTURES if n in which] or list(FIXTURES))
