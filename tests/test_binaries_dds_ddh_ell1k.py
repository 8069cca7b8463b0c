"""The DDS, DDH and ELL1k binary models (binary_dd.py BinaryDDS / BinaryDDH, binary_ell1.py
BinaryELL1k) on the device path, against fixtures captured from the reference
(scripts/refgen/gen_binaries.py):

* dds_wls, ddh_wls, ell1k_wls : WLS, an isolated-pulsar base with the binary block, every binary
            parameter of the model free (ELL1k's M2 / SINI frozen, non-zero), 300 TOAs: two row
            blocks, the second partial, the TZR row in it;
* ddh_gls, ell1k_gls : GLS, the bench's per-pulsar shape (DMX, red noise, EFAC / EQUAD) with the
            binary block, 1000 TOAs: the compact layout and the GLS / Downhill path.

Two columns deviate from the reference on purpose: DDH's STIGMA column (the
reference's carries a stray 1 / Tsun) and ELL1k's EPS2 column (the reference's d_eps2_d_EPS2 has the
wrong sign).  The fixtures hold the corrected columns, produced by the generator's one-line
overrides and checked there against the reference's numerical derivative, and the as-is ones
beside them (asis_col_*).

Bars.  Delays (total, TZR, the TZR TOA's binary delay) and residuals: 1 ns; the binary delay 5 ps
(test_delays' bar); phase 1e-9 s x F0 plus 8 ulps of the reference's longdouble phase.  Binary
columns: the largest absolute error over the column's largest magnitude, at most COL_BAR; every
other column the project's 1e-9.  Fits 1e-3 sigma; chi2 by golden_util.chi2_bar's rule on
bin_fit_spread.json; Downhill by its "downhill" spread.
"""
import copy
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, ref_value, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
WLS = ("dds_wls", "ddh_wls", "ell1k_wls")
GLS = ("ddh_gls", "ell1k_gls")
NAMES = WLS + GLS
BINARY = {"dds_wls": "DDS", "ddh_wls": "DDH", "ell1k_wls": "ELL1k", "ddh_gls": "DDH", "ell1k_gls": "ELL1k"}
CORRECTED = {"DDH": "STIGMA", "ELL1k": "EPS2"}
# binary columns against the reference's, max |error| / max |column|, worst over the five fixtures
# and every free binary parameter: measured on one MI355X MEASURED_COL (see
# test_gpu_delay_phase_residuals_columns' docstring for the per-fixture figures); the bar is 8x
# that (other library builds' sincos / log / exp rounding), and never looser than 1e-12
MEASURED_COL = 3.320e-13
COL_BAR = min(8 * MEASURED_COL, 1e-12)
_CACHE = {}


def load(name):
    """The fixture's arrays and meta (loaded once, shared) and a fresh model."""
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    if name not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        toas = from_arrays_with_tzr(z, dict(meta["flag_columns"]), name, meta.get("obs_names"))
        _CACHE[name] = (toas, z, meta)
    toas, z, meta = _CACHE[name]
    model = get_model(os.path.join(GOLDEN, name + ".par"))
    model.free_params = [p for p in meta["model"]["free_params"] if p in model]
    return model, toas, z, meta


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "bin_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on bin_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def downhill_bar(name, p, floor=1e-3):
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _ref_binary_params(meta):
    """The reference component's parameters that the host model holds, in the reference's order:
    all but FB0 (orbital-frequency orbits are not built) and ELL1k's derived ECC / OM."""
    vals = meta["model"]["values"]
    names = [p for p in meta["model"]["params"] if p in _BIN_NAMES]
    return [p for p in names if p != "FB0" and not (meta["binary"] == "ELL1k" and vals[p]["kind"] == "funcParameter")]


_BIN_NAMES = {"PB", "PBDOT", "XPBDOT", "A1", "A1DOT", "ECC", "EDOT", "T0", "OM", "OMDOT", "M2", "SINI", "FB0", "A0", "B0",
              "GAMMA", "DR", "DTH", "TASC", "EPS1", "EPS2", "SHAPMAX", "H3", "STIGMA", "LNEDOT"}


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on, again on the committed files: every free binary column has a
    non-zero maximum; the corrections are named, the corrected column differs from the as-is one
    (STIGMA: by the factor Tsun to 1 ulp) and agrees with the reference's numerical derivative
    within 1e-4 of its maximum while the as-is one does not; the reference's Downhill fit
    converged; 300 rows are a partial second block."""
    model, toas, z, meta = load(name)
    binary = BINARY[name]
    assert meta["binary"] == binary and meta["binary_component"] in meta["model"]["components"]
    params = meta["dm_params"]
    free = meta["binary_free"]
    assert free and all(p in params for p in free)
    for p in free:
        assert np.max(np.abs(z["dm_M"][:, params.index(p)])) > 0, p
    assert set(meta["reference_patches"]) == {"DDHmodel.d_delayS_d_par", "ELL1kmodel.d_eps2_d_EPS2"}
    col = CORRECTED.get(binary)
    if col is None:
        assert not any(k.startswith("asis_col_") for k in z) and meta["corrected"] == {}
    else:
        assert col in free and meta["corrected"]["column"] == col
        good, asis = z["dm_M"][:, params.index(col)], z["asis_col_" + col]
        assert meta["corrected"]["num_rel_err"] < 1e-4 < 0.1 < meta["corrected"]["asis_num_rel_err"]
        if col == "STIGMA":
            want = asis * 4.92549094830932e-06
            assert np.all(np.abs(good - want) <= np.spacing(np.abs(want)))
        else:
            assert np.max(np.abs(good - asis)) > 0.1 * np.max(np.abs(good))
    assert meta["down_converged"] and meta["down_status"] == "converged"
    assert toas.ntoas == (300 if name in WLS else 1000)
    key = "wls" if name in WLS else "gls"
    assert all(np.isfinite(v) and v > 0 for v in meta[key + "_errors"].values())
    if name in ("dds_wls", "ddh_wls"):
        assert z["grid_chi2"].shape == (5, 5) and np.all(np.isfinite(z["grid_chi2"]))
        assert np.all(z["grid_" + meta["grid_params"][1] + "_hi"] > 0)
        # the grid's points are ones where the reference's one-step fit is converged by its own
        # Downhill criterion (a second step gains < 1e-2 in chi2): the generator's span rule
        assert meta["grid_second_step_gain"] < 1e-2 and meta["grid_span_sigma"] in (2.0, 1.0, 0.5, 0.25, 0.1)
        assert np.argmin(z["grid_chi2"]) == 12 and z["grid_chi2"].max() > z["grid_chi2"].min() + 0.01
    assert abs(z["tzr_binary_delay"][0]) > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_params_components_and_derived(name):
    """free_params, the binary component and its parameters' order against the record; the
    derived SINI (DDS) and SINI / M2 (DDH) read as the reference's funcParameters do, stand where
    the reference has them in params, and are never free or written."""
    model, toas, z, meta = load(name)
    binary = BINARY[name]
    assert model.binary == binary and "Binary" + binary in model.components
    assert meta["binary_component"] == "Binary" + binary
    assert model.free_params == meta["model"]["free_params"]
    ref = _ref_binary_params(meta)
    assert [p for p in model.params if model[p].component == "Binary"] == ref
    vals = meta["model"]["values"]
    derived = {"DDS": ["SINI"], "DDH": ["SINI", "M2"], "ELL1k": []}[binary]
    for p in derived:
        assert vals[p]["kind"] == "funcParameter" and model[p].kind == "func" and model[p].frozen
        assert abs(float(model[p].value) - vals[p]["value"][0]) <= 4 * np.spacing(vals[p]["value"][0]), p
        assert p not in model.free_params
        assert not any(l.split()[0] == p for l in model.as_parfile().splitlines() if l.split())
        model.free_params = model.free_params + [p]  # (asking for it changes nothing)
        assert p not in model.free_params and model[p].frozen
    for p in ref:
        if p in derived:
            continue
        v = vals[p]["value"]
        if v is None:  # (the reference's unset rate; 0 and not written here)
            assert not model[p].value and model[p].frozen, p
        else:
            assert float(model[p].value) == v[0], p
            assert model[p].frozen == vals[p]["frozen"], p


def test_defaults_and_aliases():
    """The components as the reference constructs them: SHAPMAX 0; H3 / STIGMA unset (SINI and M2
    then unset too); ELL1k without EPS1DOT / EPS2DOT / EDOT and with LNEDOT; VARSIGMA and STIG read
    as STIGMA."""
    from pint_amd import get_model
    forms = load("ell1k_wls")[3]["forms"]
    m = get_model(forms["dds_no_shapmax"]["par"])
    rec = forms["dds_no_shapmax"]["values"]
    assert m.SHAPMAX.value == rec["SHAPMAX"] == 0.0 and m.SINI.value == rec["SINI"] == 0.0 and "SHAPMAX" not in m.free_params
    m = get_model(forms["ddh_no_stigma"]["par"])
    rec = forms["ddh_no_stigma"]["values"]
    assert m.STIGMA.value is None and rec["STIGMA"] is None and m.SINI.value is None and m.M2.value is None
    assert rec["SINI"] is None and rec["M2"] is None and float(m.H3.value) == rec["H3"]
    m = load("ell1k_wls")[0]
    assert all(p not in m for p in ("EPS1DOT", "EPS2DOT", "EDOT")) and m.LNEDOT.units == "1 / yr"
    assert m.OMDOT.units == "deg / yr"
    for case in ("ddh_varsigma", "ddh_stig"):
        m = get_model(forms[case]["par"])
        rec = forms[case]["values"]
        assert float(m.STIGMA.value) == rec["STIGMA"] == 0.75 and "STIGMA" in m.free_params
        assert abs(float(m.SINI.value) - rec["SINI"]) < 1e-15 and abs(float(m.M2.value) / rec["M2"] - 1) < 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_parfile_round_trip(name):
    """The post-fit model (the reference's fitted values and uncertainties) writes the BINARY line
    and the binary parameters' lines equal to the reference's as_parfile text, in its order; reading
    them back gives the same values, fit flags and uncertainties."""
    from pint_amd import get_model
    model, toas, z, meta = load(name)
    key = "wls" if name in WLS else "gls"
    for p, s in meta[key + "_errors"].items():
        v = ref_value(meta, key + "_params", p)
        model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
        model[p].uncertainty = s
    own = lambda l: bool(l.split()) and (l.split()[0] in _BIN_NAMES or l.split()[0] == "BINARY")  # noqa: E731
    ref = [l for l in meta[key + "_parfile"].splitlines() if own(l)]
    got = [l for l in model.as_parfile().splitlines() if own(l)]
    assert ref[0].split() == ["BINARY", BINARY[name]] and len(ref) >= 10
    assert got == ref
    back = get_model(model.as_parfile())
    assert back.binary == model.binary
    assert [p for p in back.params if back[p].component == "Binary"] == [p for p in model.params
                                                                         if model[p].component == "Binary"]
    for p in model.params:
        if model[p].component == "Binary":
            a, b = model[p], back[p]
            assert a.value == b.value and a.frozen == b.frozen, p
            assert (a.uncertainty_value or 0.0) == (b.uncertainty_value or 0.0), p


@pytest.mark.parametrize("case", ("ell1k_eps1dot", "ell1k_eps2dot", "ell1k_edot", "ell1k_upper", "dds_sini",
                                  "dds_shapmax_low", "ddh_m2", "ddh_sini"))
def test_removed_and_rejected_forms(case):
    """What the reference does with a parameter the model removed, a misspelt model name and an
    out-of-range SHAPMAX (ell1k_wls.json "forms"): an error of the reference's class that names the
    parameter, or the line accepted and the derived value kept."""
    from pint_amd import get_model
    from pint_amd import timing_model as tm
    rec = load("ell1k_wls")[3]["forms"][case]
    if rec["result"] == "ok":
        m = get_model(rec["par"])
        for p in ("SINI", "M2"):
            if p in rec["values"] and m[p].kind == "func":
                assert abs(float(m[p].value) - rec["values"][p]) <= 1e-15 * abs(rec["values"][p]), p
        assert [p for p in m.free_params if m[p].component == "Binary"] == rec["free"]
        assert case in ("dds_sini", "ddh_m2", "ddh_sini")
        return
    cls = {"TimingModelError": tm.TimingModelError, "UnknownBinaryModel": tm.UnknownBinaryModel,
           "ValueError": ValueError}[rec["result"]]
    word = {"ell1k_eps1dot": "EPS1DOT", "ell1k_eps2dot": "EPS2DOT", "ell1k_edot": "EDOT", "ell1k_upper": "ELL1K",
            "dds_shapmax_low": "SHAPMAX"}[case]
    assert word in rec["message"] or case == "dds_shapmax_low"  # (the reference's SINI check fires first there)
    with pytest.raises(cls, match=word) as ei:
        get_model(rec["par"])
    assert type(ei.value).__name__ == rec["result"] and issubclass(cls, ValueError)


def test_validate_cases():
    """SHAPMAX <= -log 2 (also when set after parsing); ECC outside [0, 1) under DDS and DDH; DDH with
    STIGMA 0 or unset parses, as in the reference, and is refused with a ValueError naming STIGMA
    when it is evaluated (the reference goes on with inf); DDGR and BT_piecewise stay refused."""
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    forms = load("ell1k_wls")[3]["forms"]
    m = load("dds_wls")[0]
    m.SHAPMAX.value = -0.7
    with pytest.raises(ValueError, match="SHAPMAX"):
        m.validate()
    m.SHAPMAX.value = -0.69  # (> -log 2 = -0.6931...)
    m.validate()
    for name in ("dds_wls", "ddh_wls"):
        m = load(name)[0]
        m.ECC.value = 1.0
        with pytest.raises(ValueError, match="Eccentricity"):
            m.validate()
    toas = load("ddh_wls")[1]
    for case in ("ddh_stigma_zero", "ddh_no_stigma"):
        assert forms[case]["result"] == "ok"
        m = get_model(forms[case]["par"])
        with pytest.raises(ValueError, match="STIGMA"):
            build_layout(m, toas)
    par = forms["dds_no_shapmax"]["par"]
    for other in ("DDGR", "BT_piecewise"):
        with pytest.raises(NotImplementedError, match=other.upper()):
            get_model(par.replace("BINARY DDS", "BINARY " + other))


@pytest.mark.parametrize("name", WLS)
def test_layout(name):
    """spec.binary; a table slot for every binary parameter the model holds but the derived ones;
    SHAPMAX's and LNEDOT's slots in the reserve words (1 + slot: PINT_SPEC_O_BINX); the free binary
    parameters as PINT_COL_BIN columns with their ids; the spec's size the parent's."""
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout
    from pint_amd.timing_model import BIN_IDS
    model, toas, z, meta = load(name)
    lay = build_layout(model, toas)
    binary = BINARY[name]
    assert ctypes.sizeof(L.SpecT) == 4128 and L.SpecT.col_kind.offset == L.SpecT.o_GLITCH.offset + 20
    assert (L.BIN_DDS, L.BIN_DDH, L.BIN_ELL1K) == (6, 7, 8)
    assert lay.spec.binary == {"DDS": 6, "DDH": 7, "ELL1k": 8}[binary]
    assert BIN_IDS["SHAPMAX"] == 27 and BIN_IDS["LNEDOT"] == 28 and L.B_NPAR == 27
    held = [p for p in model.params if model[p].component == "Binary" and model[p].kind != "func"]
    slots = {}
    for p, pid in BIN_IDS.items():
        o = lay.spec.o_bin[pid] if pid < L.B_NPAR else lay.spec.rsv_[pid - L.B_NPAR] - 1
        assert (o >= 0) == (p in held), p
        if o >= 0:
            assert o == lay.offsets[p] and o % 2 == 0 and o + 2 <= lay.spec.tstride
            slots[p] = o
    assert len(set(slots.values())) == len(held)
    assert list(lay.spec.rsv_) == {"DDS": [1 + slots.get("SHAPMAX", -1), 0, 0], "DDH": [0, 0, 0],
                                   "ELL1k": [0, 1 + slots.get("LNEDOT", -1), 0]}[binary]
    for p in meta["binary_free"]:
        c = lay.columns.index(p)
        assert (lay.spec.col_kind[c], lay.spec.col_index[c], lay.spec.col_toff[c]) == (L.COL_BIN, BIN_IDS[p], slots[p])
    assert lay.spec.ell1h == 0


@pytest.mark.parametrize("name,table,offsets,spec", (
    ("pta_dd", "2f7ba10d058d1747d5f6f174e6ac66a5398c60ceff3f09b6bef18d3969e8389c",
     "af615b4e0cef586c1ac2fcd8dbe2582cba68ff8bf48725c5527ab8907951e347",
     "53d605f8c6aa22aaf4c843679378fc779956e5144aafb438d0fea0a1ed4b5767"),
    ("pta_ell1", "2ced18a47d0c5d9080d573c7961f2645608b2a93e2021d51a7641274dd5e38e4",
     "2334cdd58332f312042a4a2b7a7e0e8bb31f224b573d239ff63b35b1ef69896d",
     "1f1a82f19ad2f985e41bf10e846963a2a4c5e30d05e1b6ac460e7579d0af052c"),
    ("pta_ddk", "7ec7e01ed368c18721a64cadb60f25ec923a93530118973316d901d0e945cc4f",
     "6659374e8dbce846ddf44359154826f8cddb91516b6109a1406d034d447915f8",
     "8a0cad5b163422f72b3d8fa85eff635fef9cad11b551aa11cab210fdfbec10ef")))
def test_layout_of_other_binaries_is_the_parents(name, table, offsets, spec):
    """A DD, an ELL1 and a DDK pulsar keep the parameter table, the table offsets and every byte of
    the spec that the code before these models gave (hashes recorded from it)."""
    import golden_util
    from pint_amd.engine import build_layout, pack_table
    model, toas, z, meta = golden_util.load(name)
    lay = build_layout(model, toas)
    assert list(lay.spec.rsv_) == [0, 0, 0]
    assert hashlib.sha256(pack_table(lay).tobytes()).hexdigest() == table
    assert hashlib.sha256(repr(list(lay.offsets.items())).encode()).hexdigest() == offsets
    assert hashlib.sha256(bytes(lay.spec)).hexdigest() == spec


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_delay_phase_residuals_columns(name):
    """Measured on one MI355X (dds_wls / ddh_wls / ell1k_wls / ddh_gls / ell1k_gls): total delay 1.7e-13
    / 1.7e-13 / 1.1e-13 / 2.1e-13 / 4.0e-13 s, TZR delay <= 2.6e-13 s, binary delay 1.9e-13 / 1.6e-13 /
    1.4e-13 / 2.2e-13 / 4.1e-13 s, phase 9.3e-10 / 9.3e-10 / 9.3e-10 / 7.5e-9 / 1.5e-8 cycles,
    residuals 5.1e-12 / 4.5e-12 / 5.1e-12 / 1.9e-11 / 1.8e-11 s; binary columns, of the column's
    maximum: T0 1.6e-13 / 3.3e-13 / - / 3.3e-13 / - (the worst: MEASURED_COL), every other DDS / DDH
    column <= 1.7e-14 (SHAPMAX 1.7e-14, H3 1.2e-14, STIGMA 1.5e-14), ELL1k's <= 3.7e-14 (EPS2 2.9e-14,
    OMDOT 2.6e-14, LNEDOT 2.0e-14)."""
    from pint_amd import Residuals
    from pint_amd.engine import evaluate_delay_phase
    model, toas, z, meta = load(name)
    n = toas.ntoas
    dp = evaluate_delay_phase(model, toas)
    e_d = np.max(np.abs(dp["delay"] - z["delay_total"]))
    e_tz = abs(dp["tzr_delay"] - z["tzr_delay"][0])
    # the binary delay: the total less the delays of the components before it in the sum, which the
    # reference records one by one (the binary's is the last here: no FD, no WaveX)
    others = sum(z[k] for k in z if k.startswith("delay_") and k not in ("delay_total", "delay_binarymodel_delay"))
    assert np.max(np.abs(z["delay_total"] - (others + z["delay_binarymodel_delay"]))) < 1e-12
    e_b = float(np.max(np.abs((dp["delay"] - others) - z["delay_binarymodel_delay"])))
    got = dp["phase_hi"].astype(LD) + dp["phase_lo"].astype(LD)
    ref = z["phase_noabs_int"].astype(LD) + z["phase_noabs_frac"].astype(LD)
    e_ph = float(np.max(np.abs(got[:n] - ref)))
    ph_bar = 1e-9 * float(model.F0.value) + 8 * float(np.spacing(np.max(np.abs(ref))))
    r = Residuals(toas, model)
    e_r = np.max(np.abs(r.time_resids - z["res_time"]))
    M, params, units = model.designmatrix(toas)
    assert list(params) == meta["dm_params"]
    refM = z["dm_M"]
    scale = np.max(np.abs(refM), axis=0)
    scale[scale == 0] = 1
    err = np.max(np.abs(M - refM), axis=0) / scale
    bins = [j for j, p in enumerate(params) if p in meta["binary_free"]]
    assert len(bins) == len(meta["binary_free"]) >= 7
    wb = bins[int(np.argmax(err[bins]))]
    print(f"{name}: delay {e_d:.2e} s, TZR delay {e_tz:.2e} s, binary delay {e_b:.2e} s, phase {e_ph:.2e} cycles "
          f"(bar {ph_bar:.1e}), residuals {e_r:.2e} s, columns max {err.max():.2e} ({params[int(np.argmax(err))]}), "
          f"binary columns max {err[wb]:.3e} ({params[wb]}; bar {COL_BAR:.2e}): "
          + ", ".join(f"{params[j]} {err[j]:.1e}" for j in bins))
    assert e_d <= 1e-9 and e_tz <= 1e-9
    assert e_b <= 5e-12
    assert e_ph <= ph_bar
    assert e_r <= 1e-9
    bad = {params[k]: err[k] for k in np.where(err > 1e-9)[0]}
    assert not bad, bad
    assert COL_BAR <= 1e-12
    bad = {params[k]: err[k] for k in bins if err[k] > COL_BAR}
    assert not bad, (bad, COL_BAR)
    col = CORRECTED.get(BINARY[name])
    if col is not None:  # (the as-is column is far from the device's)
        j = list(params).index(col)
        assert np.max(np.abs(M[:, j] - z["asis_col_" + col])) > 0.1 * np.max(np.abs(M[:, j]))


def _check_fit(f, meta, key, etol):
    worst = 0.0
    for p in meta[key + "_params"]:
        s = meta[key + "_errors"][p]
        d = float((LD(f.model[p].value) - ref_value(meta, key + "_params", p)) / LD(s))
        worst = max(worst, abs(d))
        assert abs(f.model[p].uncertainty / s - 1) < etol, (p, f.model[p].uncertainty / s - 1)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fit(name):
    """One WLS (GLS) step with every binary parameter of the model free, STIGMA and EPS2 among them:
    parameters within 1e-3 sigma of the reference's, uncertainties, chi2 within the spread's bar."""
    from pint_amd import GLSFitter, Residuals, WLSFitter
    model, toas, z, meta = load(name)
    key = "wls" if name in WLS else "gls"
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (WLSFitter if key == "wls" else GLSFitter)(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, key, 1e-6 if key == "wls" else 1e-5)
    if key == "gls":
        pre = rms_ps(f.resids.time_resids, z["gls_post_resid"])
    bar = chi2_bar(name, "fit", pre)
    print(f"{name}: {key} worst {worst:.2e} sigma, chi2 rel {c2 / meta[key + '_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta[key + "_chi2"] - 1) < bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_downhill(name):
    from pint_amd import DownhillGLSFitter, DownhillWLSFitter, Residuals
    from pint_amd.fitter import MaxiterReached, StepProblem
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (DownhillWLSFitter if name in WLS else DownhillGLSFitter)(toas, model)
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
          f"worst {dev[pw]:.2e} sigma ({pw}, bar {downhill_bar(name, pw):.1e})")
    assert abs(f.resids.chi2 / meta["down_chi2"] - 1) < bar
    for p, d in dev.items():
        assert d < downhill_bar(name, p), (p, d, downhill_bar(name, p))
        assert abs(f.model[p].uncertainty / meta["down_errors"][p] - 1) < (1e-6 if name in WLS else 1e-5), p


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("dds_wls", "ddh_wls"))
def test_gpu_grid(name):
    """The reference's 5x5 grid_chisq over (M2, SHAPMAX) / (H3, STIGMA) around its Downhill result
    (the model is set to "grid_base", so both grids stand on the same point; the span is the largest
    at which the reference's one-step fits are converged, scripts/refgen/gen_binaries.py), at
    test_gpu_grid_fd1jump_dm's bar (golden_util.chi2_bar's rule on the fixture's "fit" spread); the
    same argmin.  The reference's values come from its executor path (grid_chisq(..., ncpu=2), its
    default), where every point is fitted on a copy of the base model, as the device's batch of
    independent points is.  Its single-process path (ncpu=1) fits the points one after another on one fitter, each
    from the previous point's fitted parameters, which for these non-linear parameters is another,
    order-dependent number (up to 1.2e-5 of chi2 away on dds_wls; the generator's note)."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    for p in meta["grid_base"]:
        v = ref_value(meta, "grid_base", p)
        model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
    f = WLSFitter(toas, model)
    n0, n1 = meta["grid_params"]
    g0 = z[f"grid_{n0}_hi"].astype(LD) + z[f"grid_{n0}_lo"]
    g1 = z[f"grid_{n1}_hi"].astype(LD) + z[f"grid_{n1}_lo"]
    c2, _ = grid_chisq(f, (n0, n1), (g0, g1))
    ref = z["grid_chi2"]
    bar = chi2_bar(name, "fit", pre)
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"{name}: ({n0}, {n1}) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}")
    assert c2.shape == ref.shape == (5, 5)
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)


def _step_all(items, want):
    """Evaluation outputs, design matrix, residuals and one GLS step of every (model, toas) in one
    session."""
    from pint_amd.engine import Session, build_layout, pack_table
    s = Session()
    lays = [s.add(build_layout(copy.deepcopy(m), t)) for m, t in items]
    s.set_instances([(lay, pack_table(lay)) for lay in lays])
    s.eval(want_M=True)
    ev = s.read_eval()
    M = s.read_designmatrix()
    tr, pr, c2 = s.read_resids()
    out = [[np.array(x[k], copy=True) for x in ev] + [np.array(M[k], copy=True), np.array(tr[k], copy=True),
                                                       np.array(pr[k], copy=True), np.float64(c2[k])]
           for k in range(len(items))]
    s.eval(want_M=want)
    s.fit_step(1)
    dp, er, cov, cl = s.read_step()
    for k in range(len(items)):
        out[k] += [np.array(dp[k], copy=True), np.array(er[k], copy=True), np.array(cov[k], copy=True), np.float64(cl[k])]
    s.close()
    return out


def _dds_gls():
    """ddh_gls's TOAs and model with the binary block rewritten for DDS (M2 0.3, SHAPMAX 3.0, both
    free): the batch tests compare the device with itself, so it needs no reference record, and a
    pulsar without a noise basis (dds_wls) would change the batch's Gram path."""
    from pint_amd import get_model
    model, toas, z, meta = load("ddh_gls")
    swap = {"BINARY": "BINARY DDS", "H3": "M2 0.3 1", "STIGMA": "SHAPMAX 3.0 1"}
    par = "".join(swap.get(l.split()[0], l) + "\n" for l in open(os.path.join(GOLDEN, "ddh_gls.par")).read().splitlines())
    m = get_model(par)
    m.free_params = [p for p in model.free_params if p not in ("H3", "STIGMA")] + ["M2", "SHAPMAX"]
    assert m.binary == "DDS" and abs(float(m.SINI.value) - (1 - np.exp(-3.0))) < 1e-15
    return m, toas


def _mixed_items():
    import golden_util
    return [golden_util.load(n)[:2] for n in ("pta_iso", "pta_ell1", "pta_dd", "pta_ddk")] + \
        [_dds_gls()] + [load(n)[:2] for n in ("ddh_gls", "ell1k_gls")]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ("compact", "full"))
def test_gpu_mixed_batch(layout):
    """An isolated, an ELL1, a DD, a DDK, a DDS, a DDH and an ELL1k pulsar in one Session (the merged
    launch for the first three, a launch of its own for each of the others) against each alone:
    evaluation outputs, design matrix, residuals and fit step bit for bit, in the compact fit layout
    and in the full one."""
    from pint_amd.engine import Session
    items = _mixed_items()
    want = Session.FIT if layout == "compact" else True
    mixed = _step_all(items, want)
    for k, it in enumerate(items):
        (alone,) = _step_all([it], want)
        for x, y in zip(mixed[k], alone):
            np.testing.assert_array_equal(x, y)
        assert np.all(np.isfinite(alone[4])) and np.all(np.isfinite(alone[-4]))


@pytest.mark.gpu
def test_gpu_lazy_pipelined():
    """ddh_gls and ell1k_gls in a lazy, pipelined session (the bench's step shape, two steps in
    flight: test_fdjump's test of the same name) against the synchronous session: the step, its
    errors and the noise realisations bit for bit."""
    from pint_amd.engine import Session, build_layout, pack_table
    items = [load("ddh_gls")[:2], load("ell1k_gls")[:2]]

    def fresh():
        s = Session()
        lays = [s.add(build_layout(copy.deepcopy(m), t)) for m, t in items]
        s.set_instances([(l, pack_table(l)) for l in lays])
        return s

    def outputs(s):
        dp, er, _, cl = s.read_step(want_cov=False)
        return [dp, er, cl], s.noise_resids()

    def copied(o):
        (dp, er, cl), nz = o
        return ([np.array(x, copy=True) for x in dp] + [np.array(x, copy=True) for x in er] + [np.array(cl, copy=True)],
                [{k: v.copy() for k, v in d.items()} for d in nz])

    s0 = fresh()
    s0.eval(want_M=Session.FIT)
    s0.fit_step(1)
    want = copied(outputs(s0))
    s0.close()
    s = fresh()
    s.save_tables()
    s.set_lazy(True)
    got, prev = [], None
    for _ in range(3):
        s.restore_tables()
        s.eval(want_M=Session.FIT)
        s.fit_step(1)
        o = outputs(s)
        s.apply_step_uniform(1.0)
        s.eval(want_M=False)
        slot = s.step_end()
        if prev is not None:
            s.check_step(prev[0])
            got.append(copied(prev[1]))
        prev = (slot, o)
    s.check_step(prev[0])
    got.append(copied(prev[1]))
    s.close()
    assert len(got) == 3 and "pl_red_noise" in want[1][0]
    for arrs, nz in got:
        for x, y in zip(arrs, want[0]):
            np.testing.assert_array_equal(x, y)
        for k in range(2):
            assert set(nz[k]) == set(want[1][k])
            for comp in want[1][k]:
                np.testing.assert_array_equal(nz[k][comp], want[1][k][comp])


@pytest.mark.gpu
def test_gpu_graph_replay_matches_direct():
    """ddh_gls and ell1k_gls: a fit step captured into a HIP graph and replayed (the shape of
    test_graph_replay_matches_direct) gives the step, errors, covariance and chi2 of the directly
    enqueued step bit for bit -- the two models' own launches are captured back to back."""
    from pint_amd.engine import Session, build_layout, pack_table
    items = [load("ddh_gls")[:2], load("ell1k_gls")[:2]]
    s = Session()
    lays = [s.add(build_layout(copy.deepcopy(m), t)) for m, t in items]
    tabs = [pack_table(l) for l in lays]
    s.set_instances(list(zip(lays, tabs)))
    flat = np.concatenate(tabs)
    s.set_lazy(True)

    def step(t):
        s.set_tables(t)
        s.eval(want_M=Session.FIT)
        s.fit_step(1)
        out = s.read_step()
        s.apply_step(np.ones(len(lays)))
        s.eval(want_M=False)
        return out, s.chi2_gls()

    def snap(res):
        (dp, er, cov, cl), c2 = res
        return [x.copy() for x in dp] + [x.copy() for x in er] + [x.copy() for x in cov] + [cl.copy(), c2.copy()]

    res = step(flat)
    s.check()
    direct = snap(res)
    cap = s.capture(lambda: step(flat))
    for _ in range(2):  # (replays are repeatable)
        s.replay()
        s.check()
        for x, y in zip(direct, snap(cap)):
            np.testing.assert_array_equal(x, y)
    s.close()
    assert np.all(np.isfinite(direct[-1])) and np.all(direct[-1] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("dds_lognum", "ddh_ecc"))
def test_gpu_invalid_instance_fails_alone(case):
    """Error paths on finite inputs, in a batch of a DDS, a DDH and an ELL1k pulsar.  dds_lognum: a
    table whose SHAPMAX is -5 (SINI = 1 - e^5 = -147: past the host's validate, as a fit step could
    leave it) makes the Shapiro logarithm's argument negative on the rows with sin w (cos E - e) +
    sqrt(1 - e^2) cos w sin E < 0; ddh_ecc: ECC stepped to 1.5.  The checked evaluation reports
    PINT_E_KEPLER, pint_inst_status names that instance alone, and the other instances' outputs are
    finite and bit for bit those of the clean batch (no NaN written for the failing one either)."""
    from pint_amd import _lib as L
    from pint_amd.engine import Session, build_layout, pack_table
    items = [load(n)[:2] for n in WLS]
    s = Session()
    lays = [s.add(build_layout(copy.deepcopy(m), t)) for m, t in items]
    tabs = [pack_table(l) for l in lays]
    s.set_instances(list(zip(lays, tabs)))
    s.eval(want_M=False)
    s.check()
    assert not np.any(s.inst_status())
    clean = [[np.array(a, copy=True) for a in x] for x in s.read_eval()]
    k, p, v = {"dds_lognum": (0, "SHAPMAX", -5.0), "ddh_ecc": (1, "ECC", 1.5)}[case]
    bad = [t.copy() for t in tabs]
    bad[k][lays[k].offsets[p]] = v
    bad[k][lays[k].offsets[p] + 1] = 0.0
    s.set_tables(np.concatenate(bad))
    with pytest.raises(L.PintError) as ei:
        s.eval(want_M=False)
        s.check()
    assert ei.value.code == L.PINT_E_KEPLER
    st = s.inst_status()
    assert [bool(x & (1 << L.PINT_E_KEPLER)) for x in st] == [j == k for j in range(3)]
    got = s.read_eval()
    for x, y in zip(got, clean):
        for j in range(3):
            assert np.all(np.isfinite(x[j])), (case, j)
            if j != k:
                np.testing.assert_array_equal(x[j], y[j])
    s.set_tables(np.concatenate(tabs))  # the valid tables again: the clean outputs, no status
    s.eval(want_M=False)
    s.check()
    assert not np.any(s.inst_status())
    for x, y in zip(s.read_eval(), clean):
        for j in range(3):
            np.testing.assert_array_equal(x[j], y[j])
    s.close()
