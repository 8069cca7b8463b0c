"""SolarWindDispersion, SWM 0 (solar_wind_dispersion.py:267-412) on the device path, against
fixtures captured from the reference (scripts/refgen/gen_solar_wind.py):

* sw_ecl : WLS, ecliptic astrometry, ELL1, NE_SW free, 5.3 deg off the ecliptic;
* sw_pta : GLS, equatorial astrometry, DD, DMX and red noise (the bench's per-pulsar shape);
* sw_wb  : sw_pta's model with wideband DM measurements.

The bars are the project's bars for every other fixture; the chi2 bars
follow golden_util.chi2_bar's rule, read from sw_fit_spread.json (the reference's own spread
for these fixtures).
"""
import copy
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, ref_value, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
NAMES = ("sw_ecl", "sw_pta", "sw_wb")
_CACHE = {}


def load(name):
    """golden_util.load for the solar-wind fixtures (par file = fixture name); the arrays and
    the meta are loaded once and shared, the model is a fresh copy per caller."""
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    if name not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        fc = dict(meta["flag_columns"])
        if "wb_pp_dm" in z:
            fc["pp_dm"] = [repr(float(x)) for x in z["wb_pp_dm"]]
            fc["pp_dme"] = [repr(float(x)) for x in z["wb_pp_dme"]]
        toas = from_arrays_with_tzr(z, fc, name, meta.get("obs_names"))
        _CACHE[name] = (toas, z, meta)
    toas, z, meta = _CACHE[name]
    model = get_model(os.path.join(GOLDEN, name + ".par"))
    model.free_params = [p for p in meta["model"]["free_params"] if p in model]
    return model, toas, z, meta


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "sw_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on sw_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def downhill_bar(name, p, floor=1e-3):
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _par_without(name, *drop):
    lines = open(os.path.join(GOLDEN, name + ".par")).read().splitlines()
    return "\n".join(l for l in lines if not (l.split() and l.split()[0] in drop)) + "\n"


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixtures_have_effect(name):
    """The fixtures cannot pass with the term missing: the reference's solar-wind delay exceeds
    1 us somewhere (the delay bar is 5 ps) and at least 20 TOAs lie within 15 deg of the Sun."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    assert np.max(np.abs(z["delay_solar_wind_delay"])) > 1e-6
    sun = z["obs_sun_pos_km"]
    ct = np.sum(sun / np.linalg.norm(sun, axis=1)[:, None] * z["psr_dir_icrs"], axis=1)
    assert np.sum(np.degrees(np.arccos(ct)) < 15.0) >= 20


@pytest.mark.parametrize("name", NAMES)
def test_layout_has_ne_sw_column(name):
    from pint_amd import get_model
    from pint_amd.engine import build_layout, pack_table
    model, toas, z, meta = load(name)
    lay = build_layout(model, toas)
    assert lay.columns == meta["dm_params"]  # NE_SW where the reference's design matrix has it
    assert lay.spec.o_NE_SW >= 0 and lay.offsets["NE_SW"] == lay.spec.o_NE_SW
    # NE_SW present, zero and frozen: no slot, and table and spec byte-identical to the same par
    # without the NE_SW / SWM lines
    bare = get_model(_par_without(name, "NE_SW", "SWM"))
    zero = get_model(_par_without(name, "NE_SW", "SWM") + "NE_SW 0\nSWM 0\n")
    free = [p for p in meta["model"]["free_params"] if p != "NE_SW"]
    bare.free_params = free
    zero.free_params = free
    lb, lz = build_layout(bare, toas), build_layout(zero, toas)
    assert lz.spec.o_NE_SW == -1 and lb.spec.o_NE_SW == -1
    assert bytes(lz.spec) == bytes(lb.spec)
    assert lz.offsets == lb.offsets and lz.columns == lb.columns
    assert pack_table(lz).tobytes() == pack_table(lb).tobytes()
    # ... and, apart from the new field, to the layout with the solar wind: the NE_SW slot and
    # column are the only additions
    assert [c for c in lay.columns if c != "NE_SW"] == lb.columns
    assert lay.tstride == lb.tstride + 2


def test_parfile_round_trip():
    """The post-fit sw_ecl model (the reference's fitted values and uncertainties) writes
    NE_SW / SWM lines equal to the reference's as_parfile text; SOLARN0 and NE1AU read as
    NE_SW; SWP is ignored with SWM 0."""
    from pint_amd import get_model
    model, toas, z, meta = load("sw_ecl")
    for p, s in meta["wls_errors"].items():
        v = ref_value(meta, "wls_params", p)
        model[p].value = v if model[p].long_double else float(v)
        model[p].uncertainty = s
    ref = {l.split()[0]: l for l in meta["wls_parfile"].splitlines() if l.split()}
    got = {l.split()[0]: l for l in model.as_parfile().splitlines() if l.split()}
    assert got["NE_SW"] == ref["NE_SW"]
    assert got["SWM"] == ref["SWM"]
    assert "SWP" not in got and "SWP" not in ref
    back = get_model(model.as_parfile())
    assert back.NE_SW.value == model.NE_SW.value and not back.NE_SW.frozen and back.SWM.value == 0
    for alias in ("SOLARN0", "NE1AU"):
        m = get_model(_par_without("sw_ecl", "NE_SW") + f"{alias} 4.5 1\nSWP 2.0\n")
        assert m.NE_SW.value == 4.5 and not m.NE_SW.frozen and m.has_solar_wind


def test_unsupported_forms_raise():
    from pint_amd import get_model
    base = _par_without("sw_ecl", "SWM")
    with pytest.raises(NotImplementedError, match="SWM"):
        get_model(base + "SWM 1\nSWP 2.0\n")
    with pytest.raises(NotImplementedError, match="SWXDM_0001"):
        get_model(base + "SWXDM_0001 1e-3 1\nSWXP_0001 2\nSWXR1_0001 54000\nSWXR2_0001 55000\n")
    with pytest.raises(NotImplementedError, match="CORRECT_TROPOSPHERE"):
        get_model(base + "CORRECT_TROPOSPHERE Y\n")


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sw_ecl", "sw_pta"])
def test_gpu_delay_residuals_columns(name):
    from pint_amd import Residuals
    from pint_amd.engine import evaluate_delay_phase
    model, toas, z, meta = load(name)
    dp = evaluate_delay_phase(model, toas)
    e_d = np.max(np.abs(dp["delay"] - z["delay_total"]))
    e_tz = abs(dp["tzr_delay"] - z["tzr_delay"][0])
    r = Residuals(toas, model)
    e_r = np.max(np.abs(r.time_resids - z["res_time"]))
    M, params, _ = model.designmatrix(toas)
    assert list(params) == meta["dm_params"]
    ref = z["dm_M"]
    scale = np.max(np.abs(ref), axis=0)
    scale[scale == 0] = 1
    err = np.max(np.abs(M - ref) / scale, axis=0)
    j = params.index("NE_SW")
    print(f"{name}: delay {e_d:.2e} s, TZR delay {e_tz:.2e} s, residuals {e_r:.2e} s, "
          f"columns max {err.max():.2e} ({params[int(np.argmax(err))]}), NE_SW column {err[j]:.2e}")
    assert e_d <= 5e-12 and e_tz <= 5e-12
    assert e_r <= 1e-10
    assert np.max(np.abs(ref[:, j])) > 0 and err[j] <= 1e-9
    bad = {params[k]: err[k] for k in np.where(err > 1e-9)[0]}
    assert not bad, bad


def _check_fit(f, meta, key, etol):
    worst = 0.0
    for p in meta[key + "_params"]:
        s = meta[key + "_errors"][p]
        d = float((LD(f.model[p].value) - ref_value(meta, key + "_params", p)) / LD(s))
        worst = max(worst, abs(d))
        assert abs(f.model[p].uncertainty / s - 1) < etol, (p, f.model[p].uncertainty / s - 1)
    return worst


@pytest.mark.gpu
def test_gpu_wls_fit_ecl():
    from pint_amd import WLSFitter
    model, toas, z, meta = load("sw_ecl")
    pre = rms_ps(__import__("pint_amd").Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "wls", 1e-6)
    bar = chi2_bar("sw_ecl", "fit", pre)
    print(f"sw_ecl: WLS worst {worst:.2e} sigma, NE_SW {f.model.NE_SW.value:.6f} +- {f.model.NE_SW.uncertainty:.6f}, "
          f"chi2 rel {c2 / meta['wls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["wls_chi2"] - 1) < bar


@pytest.mark.gpu
def test_gpu_gls_fit_pta():
    from pint_amd import GLSFitter
    model, toas, z, meta = load("sw_pta")
    f = GLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "gls", 1e-5)
    bar = chi2_bar("sw_pta", "fit", rms_ps(f.resids.time_resids, z["gls_post_resid"]))
    print(f"sw_pta: GLS worst {worst:.2e} sigma, NE_SW {f.model.NE_SW.value:.6f} +- {f.model.NE_SW.uncertainty:.6f}, "
          f"chi2 rel {c2 / meta['gls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["gls_chi2"] - 1) < bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sw_ecl", "sw_pta"])
def test_gpu_downhill(name):
    from pint_amd import DownhillGLSFitter, DownhillWLSFitter, Residuals
    from pint_amd.fitter import MaxiterReached, StepProblem
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (DownhillWLSFitter if name == "sw_ecl" else DownhillGLSFitter)(toas, model)
    try:
        f.fit_toas(maxiter=10)
        status = "converged"
    except (MaxiterReached, StepProblem) as e:
        status = type(e).__name__
    assert status == meta["down_status"] == "converged" and f.converged
    bar = chi2_bar(name, "down", pre)
    dev = {p: abs(float((LD(f.model[p].value) - ref_value(meta, "down_params", p)) / LD(meta["down_errors"][p])))
           for p in meta["down_params"]}
    pw = max(dev, key=dev.get)
    print(f"{name}: Downhill chi2 rel {f.resids.chi2 / meta['down_chi2'] - 1:.2e} (bar {bar:.1e}), "
          f"worst {dev[pw]:.2e} sigma ({pw})")
    assert abs(f.resids.chi2 / meta["down_chi2"] - 1) < bar
    for p, d in dev.items():
        assert d < downhill_bar(name, p), (p, d, downhill_bar(name, p))


@pytest.mark.gpu
def test_gpu_wideband():
    """sw_wb at wb_dd's bars (tests/test_wideband.py): the DM residuals (DM_sw in total_dm), the
    DM and combined chi2, and the WidebandTOAFitter step (the NE_SW entry of the DM rows)."""
    from pint_amd import Residuals, WidebandDMResiduals, WidebandTOAFitter, WidebandTOAResiduals
    model, toas, z, meta = load("sw_wb")
    r = Residuals(toas, model, residual_type="dm")
    assert isinstance(r, WidebandDMResiduals)
    e_dm = np.max(np.abs(r.resids - z["wb_dm_resids"]))
    rm = WidebandDMResiduals(toas, model, subtract_mean=True)
    e_dmm = np.max(np.abs(rm.resids - z["wb_dm_resids_mean"]))
    w = WidebandTOAResiduals(toas, model)
    bar = chi2_bar("sw_wb", "pre", rms_ps(w.toa.time_resids, z["res_time"]))
    print(f"sw_wb: dm_resids {e_dm:.2e} (mean removed {e_dmm:.2e}) pc/cm3, DM chi2 rel {r.chi2 / meta['wb_dm_chi2'] - 1:.2e}, "
          f"combined chi2 rel {w.chi2 / meta['wb_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert e_dm <= 1e-12 and e_dmm <= 1e-12
    assert abs(r.chi2 / meta["wb_dm_chi2"] - 1) < 1e-12
    assert abs(w.dm.chi2 / meta["wb_dm_chi2_combined"] - 1) < 1e-12
    assert abs(w.chi2 / meta["wb_chi2"] - 1) < bar
    f = WidebandTOAFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "wbfit", 1e-5)
    rms = rms_ps(f.resids.toa.time_resids, z["wbfit_post_toa_resid"])
    print(f"sw_wb: wideband fit worst {worst:.2e} sigma, NE_SW {f.model.NE_SW.value:.6f} +- "
          f"{f.model.NE_SW.uncertainty:.6f}, chi2 rel {c2 / meta['wbfit_chi2'] - 1:.2e}")
    assert worst <= 1e-3
    assert abs(c2 / meta["wbfit_chi2"] - 1) < chi2_bar("sw_wb", "fit", rms)
    assert abs(f.resids.chi2 / meta["wbfit_post_chi2"] - 1) < chi2_bar("sw_wb", "post", rms)


@pytest.mark.gpu
def test_gpu_grid_ne_sw_dm():
    """The reference's 5x5 (NE_SW, DM) grid_chisq (parallel path) around the one-step fit: the
    larger of the WLS grid bar (rtol 1e-7) and sw_ecl's "fit" spread bar; the same argmin."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    model, toas, z, meta = load("sw_ecl")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    f.fit_toas(maxiter=1)
    g0 = z["grid_NE_SW_hi"].astype(LD) + z["grid_NE_SW_lo"]
    g1 = z["grid_DM_hi"].astype(LD) + z["grid_DM_lo"]
    c2, _ = grid_chisq(f, ("NE_SW", "DM"), (g0, g1))
    ref = z["grid_chi2_parallel"]
    bar = max(1e-7, chi2_bar("sw_ecl", "fit", pre))
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"sw_ecl: (NE_SW, DM) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}")
    assert c2.shape == ref.shape
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)


@pytest.mark.gpu
@pytest.mark.parametrize("isolated", [False, True])
def test_gpu_spin_grid_bit_identical(isolated):
    """A 3x3 (F0, F1) grid on sw_ecl with the shared-head evaluation on and off: the same bits.
    The shared head (k_eval_head / k_eval_spin, whose rows carry the solar-wind geometry as their
    tenth double) serves isolated models outside the fused residual pass, so both runs switch
    that pass off (400 TOAs would otherwise take it).  sw_ecl itself has a binary and stays on
    the full evaluation either way; without its binary lines the grid takes the shared head.
    The centre point is the model itself: its NE_SW column must also equal the column of a plain
    (non-grid) evaluation of the model, which never goes through the head."""
    from pint_amd import get_model
    from pint_amd.engine import Session, build_layout, pack_table
    model, toas, z, meta = load("sw_ecl")
    if isolated:
        binary = ("BINARY", "PB", "A1", "TASC", "EPS1", "EPS2")
        model = get_model(_par_without("sw_ecl", *binary))
        model.free_params = [p for p in meta["model"]["free_params"] if p in model]

    def run(spin):
        s = Session()
        s.set_spin_eval(spin)
        s.set_efuse(False)
        lay = s.add(build_layout(model, toas))
        base = pack_table(lay, model)
        g0 = LD(model.F0.value) + np.linspace(-2, 2, 3) * LD(1e-10)
        g1 = LD(model.F1.value) + np.linspace(-2, 2, 3) * LD(1e-18)
        s.set_grid(lay, base, [("F0", g0, 3, 3), ("F1", g1, 1, 3)], 9)
        s.eval(want_M=True)
        out = [np.array(x, copy=True) for x in s.read_eval()] + [np.array(s.read_designmatrix(), copy=True)]  # (9, n, K)
        s.fit_step(0)
        dp, er, _, cl = s.read_step()
        out += [np.array(x, copy=True) for x in dp] + [np.array(cl, copy=True)]
        s.close()
        return lay, out

    lay, a = run(True)
    _, b = run(False)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # the centre point's NE_SW column against a plain evaluation of the same model
    assert a[4].shape == (9, toas.ntoas, len(lay.columns))
    col = a[4][4][:, lay.columns.index("NE_SW")]
    M, params, _ = model.designmatrix(toas)
    ref = M[:, list(params).index("NE_SW")]
    assert np.max(np.abs(ref)) > 0
    assert np.max(np.abs(col - ref)) <= 1e-12 * np.max(np.abs(ref))


def _gls_steps(items):
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    s = Session()
    bf = BatchFit([(copy.deepcopy(m), t) for m, t in items], mode="gls", session=s)
    s.eval(want_M=Session.FIT)
    s.fit_step(1)
    dp, er, cov, cl = s.read_step()
    c2 = s.chi2_gls()
    out = [(np.array(dp[k], copy=True), np.array(er[k], copy=True), float(cl[k]), float(c2[k])) for k in range(len(items))]
    bf.close()
    s.close()
    return out


@pytest.mark.gpu
def test_gpu_mixed_batch():
    """sw_pta beside pta_iso and pta_ell1 in one session (the per-instance uniform branch, the
    LDS-staged spec): sw_pta's step and chi2 equal its single-session result to 1e-12 relative;
    the neighbours' steps, errors and chi2 are bit-identical to a session without sw_pta."""
    import golden_util
    sw = load("sw_pta")[:2]
    iso, ell1 = golden_util.load("pta_iso")[:2], golden_util.load("pta_ell1")[:2]
    mixed = _gls_steps([iso, sw, ell1])
    (alone,) = _gls_steps([sw])
    plain = _gls_steps([iso, ell1])
    d1, e1, l1, g1 = mixed[1]
    d0, e0, l0, g0 = alone
    n = len(e0) - 1
    # the step to 1e-12 of itself (a step far below its uncertainty: to 1e-12 of the uncertainty)
    assert np.all(np.abs(d1[:n] - d0[:n]) <= 1e-12 * np.maximum(np.abs(d0[:n]), e0[:n]))
    assert np.max(np.abs(e1[:n] / e0[:n] - 1)) < 1e-12
    assert abs(l1 / l0 - 1) < 1e-12 and abs(g1 / g0 - 1) < 1e-12
    for got, want in ((mixed[0], plain[0]), (mixed[2], plain[1])):
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_compact_and_full_layouts():
    """sw_pta's GLS step on the generated-Fourier compact path, the stored-basis compact path
    and the full layout: the same normal equations to rounding (the bars of
    test_generated_fourier_path_matches_stored and test_compact_layout's full-layout check)."""
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    model, toas = load("sw_pta")[:2]
    out = []
    for vgram, want in ((True, Session.FIT), (False, Session.FIT), (True, True)):
        s = Session()
        s.set_vgram(vgram)
        bf = BatchFit([(copy.deepcopy(model), toas)], mode="gls", session=s)
        if want == Session.FIT:
            assert s.fit_layout(bf.layouts[0])[0] == 1 and s.n_vgram() == (1 if vgram else 0)
        s.eval(want_M=want)
        s.fit_step(1)
        dp, er, cov, cl = s.read_step()
        out.append((np.array(dp[0], copy=True), np.array(er[0], copy=True), np.array(cov[0], copy=True), float(cl[0]),
                    float(s.chi2_gls()[0])))
        bf.close()
        s.close()

    def same(a, b, tol_step, tol_err, tol_chi2, lin=True):
        (d1, e1, c1, l1, g1), (d2, e2, c2, l2, g2) = a, b
        n = len(e1) - 1
        sc = np.sqrt(np.outer(np.diag(c2), np.diag(c2)))
        assert np.max(np.abs((d1[:n] - d2[:n]) / e2[:n])) < tol_step
        assert np.max(np.abs(e1[:n] / e2[:n] - 1)) < tol_err
        assert np.max(np.abs(c1 - c2) / sc) < tol_err
        assert not lin or abs(l1 / l2 - 1) < tol_chi2
        assert abs(g1 / g2 - 1) < tol_chi2

    same(out[0], out[1], 1e-8, 1e-9, 1e-10)             # generated vs stored Fourier columns
    same(out[0], out[2], 1e-8, 1e-9, 1e-10, lin=False)  # compact vs full layout
