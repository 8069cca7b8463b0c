"""The PiecewiseSpindown, Wave and IFunc components (piecewise.py:181-253, wave.py:148-168,
ifunc.py:113-148) on the device path, against fixtures captured from the reference
(scripts/refgen/gen_phase_terms.py):

* pw_wls   : WLS, a Vela-like isolated pulsar with one glitch and three pieces (piece 1: PWPH / PWF0 /
             PWF1 free; piece 2: PWF0 / PWF2 free, overlapping piece 1 by 100 d; piece 3 frozen,
             TZRMJD inside it);
* wave_wls : WLS, the same kind of pulsar with five WAVE terms and SIFUNC 2 with six IFUNC points;
* pw_gls   : GLS, the bench's per-pulsar shape (ELL1, DMX, red noise) with two pieces.

The bars are the project's bars for every other fixture: the absolute phase
within the residual bar as phase, 1e-10 s x F0, plus 8 ulps of the reference's longdouble phase
(test_glitch.py); residuals within 1 ns; the piece columns within 1e-12 of the column's largest
value (test_fbx.py's COL_BAR: one double rounding of the delay against a dt of 1e6 - 1e8 s and a
handful of multiplies sit four orders below it) and exactly 0 outside the window; fitted
parameters within 1e-3 sigma; the chi2 bars by golden_util.chi2_bar's rule, read from
pw_fit_spread.json (the reference's own spread for these fixtures).
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, ref_value, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
NAMES = ("pw_wls", "wave_wls", "pw_gls")
PW_PROPS = ("PWEP_", "PWSTART_", "PWSTOP_", "PWPH_", "PWF0_", "PWF1_", "PWF2_")
PW_FIT = ("PWPH_", "PWF0_", "PWF1_", "PWF2_")
LINES = {"PiecewiseSpindown": ("PWEP_", "PWSTART_", "PWSTOP_", "PWPH_", "PWF0_", "PWF1_", "PWF2_"),
         "Wave": ("WAVE",), "IFunc": ("IFUNC", "SIFUNC")}
COMPONENT_KEY = {"PiecewiseSpindown": "piecewise_phase", "Wave": "wave_phase", "IFunc": "ifunc_phase"}
COL_BAR = 1e-12
_CACHE = {}


def load(name, par=None):
    """golden_util.load for these fixtures (par file = fixture name, or the par text given); the
    arrays and the meta are loaded once and shared and never changed, the model is a fresh copy
    per caller."""
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    if name not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        toas = from_arrays_with_tzr(z, dict(meta["flag_columns"]), name, meta.get("obs_names"))
        _CACHE[name] = (toas, z, meta)
    toas, z, meta = _CACHE[name]
    model = get_model(par if par is not None else os.path.join(GOLDEN, name + ".par"))
    model.free_params = [p for p in meta["model"]["free_params"] if p in model]
    return model, toas, z, meta


def _par(name):
    return open(os.path.join(GOLDEN, name + ".par")).read()


def _par_without(name, *components, text=None):
    """The fixture's par text without the lines of the named components."""
    pre = tuple(p for c in components for p in LINES[c])
    lines = (text if text is not None else _par(name)).splitlines()
    return "\n".join(l for l in lines if not (l.split() and l.split()[0].startswith(pre))) + "\n"


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "pw_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on pw_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def downhill_bar(name, p, floor=1e-3):
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _ld(z, key):
    return z[key + "_hi"].astype(LD) + z[key + "_lo"].astype(LD)


def _times(name):
    """tdbld of the TOAs and of the TZR TOA, and ts = tdbld - delay / 86400 of both (reference's)."""
    _, _, z, _ = load(name)
    t = z["tdb_hi"].astype(LD) + z["tdb_lo"].astype(LD)
    tz = LD(z["tzr_tdb_hi"][0]) + LD(z["tzr_tdb_lo"][0])
    return t, tz, t - z["delay_total"] / LD(86400), tz - z["tzr_delay"][0] / LD(86400)


def _windows(model):
    return {i: (LD(model[f"PWSTART_{i}"].value), LD(model[f"PWSTOP_{i}"].value)) for i in model.pw_indices()}


def _pw_cols(params):
    """{piece index: [(column, parameter)]} of the free piece parameters."""
    out = {}
    for j, p in enumerate(params):
        if p.startswith(PW_FIT):
            out.setdefault(int(p.split("_")[1]), []).append((j, p))
    return out


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on: no TOA nor the TZR TOA within 1 ms of a PWSTART / PWSTOP (on
    tdbld) nor of an IFUNC point (on ts), so no window or interval is decided by rounding; the TOA
    counts and phase sizes the fixtures were built for; every free piece column has a non-zero
    maximum and exact zeros outside its window."""
    model, toas, z, meta = load(name)
    t, tz, ts, tsz = _times(name)
    n = toas.ntoas
    assert n == (1000 if name == "pw_gls" else 300)
    inside = np.zeros(n, dtype=bool)
    wins = _windows(model)
    for i, (a, b) in wins.items():
        for e in (a, b):
            assert np.min(np.abs((t - e) * 86400)) > 1e-3 and abs((tz - e) * 86400) > 1e-3, (i, e)
        inside |= (t >= a) & (t < b)
    if wins:
        assert np.sum(~inside) >= 20
        assert np.max(np.abs(z["piecewise_phase_hi"])) > (1e3 if name == "pw_wls" else 1.0)
        cols = _pw_cols(meta["dm_params"])
        assert sorted(p for lst in cols.values() for _, p in lst) == sorted(
            p for p in meta["model"]["free_params"] if p.startswith("PW"))
        for i, lst in cols.items():
            a, b = wins[i]
            off = ~((t >= a) & (t < b))
            for j, p in lst:
                assert np.max(np.abs(z["dm_M"][:, j])) > 0 and np.all(z["dm_M"][off, j] == 0.0), p
    if name == "pw_wls":
        assert len(wins) == 3 and z["piece1_max_phase"][0] > 1e3 and z["piece2_max_phase"][0] > 1e3
        both = (t >= wins[2][0]) & (t < wins[1][1])  # the overlap of pieces 1 and 2
        assert np.sum(both) >= 20
        assert wins[3][0] <= tz < wins[3][1] and abs(z["tzr_piecewise_phase_hi"][0]) > 0.1
        assert not any(p.startswith("PW") and p.endswith("_3") for p in meta["model"]["free_params"])
        for i, (a, b) in wins.items():  # no epoch at its window's centre
            assert abs(LD(model[f"PWEP_{i}"].value) - (a + b) / 2) > 10
        # the reference's grid is one number per point: its two paths agree far below the chi2 bar
        assert z["grid_chi2"].shape == (5, 5) and np.max(np.abs(z["grid_chi2_serial"] / z["grid_chi2"] - 1)) < 1e-7
    if name == "wave_wls":
        x = np.array([model[p].value[0] for p in model.ifunc_terms()], dtype=LD)
        assert len(x) == 6 and len(model.wave_terms()) == 5 and len(set(np.diff(x))) == 5
        for e in x:
            assert np.min(np.abs((ts - e) * 86400)) > 1e-3 and abs((tsz - e) * 86400) > 1e-3, e
        assert np.sum(ts < x[0]) >= 20 and np.sum(ts > x[-1]) >= 20
        assert model.WAVEEPOCH.value != model.PEPOCH.value
        assert np.max(np.abs(z["wave_phase_hi"])) > 1.0
        counts = [int(np.sum(ts < x[0])), int(np.sum((ts >= x[0]) & (ts < x[1]))), int(np.sum(ts >= x[1]))]
        assert counts == meta["sifunc0_counts"] and min(counts) >= 10  # SIFUNC 0: all three cases
        y = np.array([float(model[p].value[1]) for p in model.ifunc_terms()])
        t0 = _ld(z, "ifunc0_phase") / LD(model.F0.value)
        want = np.where(ts < x[0], y[0], np.where(ts >= x[1], y[5], y[2]))  # (as the reference runs)
        assert np.max(np.abs(t0 - want)) < 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_parse_components_order_round_trip(name):
    from pint_amd import get_model
    model, toas, z, meta = load(name)
    ref = meta["model"]
    ours = ("PW", "WAVE", "IFUNC", "SIFUNC", "GL")
    assert [p for p in model.params if p.startswith(ours)] == [p for p in ref["params"] if p.startswith(ours)]
    assert model.free_params == ref["free_params"]
    for comp in COMPONENT_KEY:
        assert (comp in model.components) == (comp in ref["components"]), comp
    order = [c for c in model.component_names if c in ref["phase_components"]]
    assert order == [c for c in ref["phase_components"] if c in order]
    for p, rec in ref["values"].items():
        if not p.startswith(ours[:4]):
            continue
        par = model[p]
        assert par.frozen == rec["frozen"], p
        if rec["kind"] == "prefixParameter" and isinstance(rec["value"][0], list):  # a pair
            assert par.kind == "pair" and len(par.value) == 2
            for v, (hi, lo) in zip(par.value, rec["value"]):
                assert LD(v) == LD(hi) + LD(lo), p
        else:
            assert LD(par.value) == LD(rec["value"][0]) + LD(rec["value"][1]), p
    # defaults: WAVEEPOCH falls back to PEPOCH; a piece-1 spin term that is not given is 0 and frozen
    if name == "wave_wls":
        m = get_model(_par(name).replace("WAVEEPOCH 54900\n", ""))
        assert m.WAVEEPOCH.value == m.PEPOCH.value
        # a third number on a pair line is ignored; a pair is never free
        assert "WAVE3 0.008 0.004 7" in _par(name) and model.WAVE3.frozen and model.WAVE3.uncertainty_value is None
    if name == "pw_wls":
        m = get_model(_par(name).replace("PWF2_1 0\n", ""))
        assert m.PWF2_1.value == 0.0 and m.PWF2_1.frozen
    # as_parfile: the reference's lines, in its order (the post-fit model where one was recorded)
    if "wls_parfile" in meta:
        for p, s in meta["wls_errors"].items() if name == "pw_wls" else ():
            v = ref_value(meta, "wls_params", p)
            model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
            model[p].uncertainty = s
        mine = tuple(q for c in COMPONENT_KEY for q in LINES[c])
        want = [l for l in meta["wls_parfile"].splitlines() if l.split() and l.split()[0].startswith(mine)]
        got = [l for l in model.as_parfile().splitlines() if l.split() and l.split()[0].startswith(mine)]
        assert len(want) >= 13 and got == want
    back = get_model(model.as_parfile())
    # (the pieces beyond the first keep the order of their par lines, which as_parfile writes epoch first)
    assert sorted(p for p in back.params if p.startswith(ours)) == sorted(p for p in model.params if p.startswith(ours))
    assert back.free_params == model.free_params
    for p in model.params:
        if p.startswith(ours[:4]):
            a, b = model[p], back[p]
            assert a.value == b.value and a.frozen == b.frozen and a.kind == b.kind, p
            assert (a.uncertainty_value or 0.0) == (b.uncertainty_value or 0.0), p


FORMS = {"free_PWEP_1": "PWEP_1", "free_PWSTART_1": "PWSTART_1", "free_WAVE_OM": "WAVE_OM",
         "piece_without_PWPH": "PWPH_2", "piece_without_PWEP": "PWEP_2", "piece_without_PWSTART": "PWSTART_3",
         "piece_without_PWSTOP": "PWSTOP_3", "wave_gap": "WAVE3", "ifunc_gap": "IFUNC4", "no_SIFUNC": "SIFUNC",
         "SIFUNC_1": "Interpolation type 1 not supported"}


@pytest.mark.parametrize("case", sorted(FORMS))
def test_forms(case):
    """Every malformed model recorded from the reference: the same exception class, at loading
    where the reference refuses at loading and at the evaluation's set-up (build_layout) where it
    refuses at its first evaluation or design matrix, with the parameter named in the message."""
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    from pint_amd import timing_model as T
    _, toas, _, meta = load("pw_wls")
    rec = meta["forms"][case]
    classes = {"ValueError": ValueError, "MissingParameter": T.MissingParameter, "UnknownParameter": T.UnknownParameter}
    assert set(meta["forms"]) == set(FORMS) and rec["error"] in classes and FORMS[case] in rec["message"]
    if rec["stage"] == "get_model":
        with pytest.raises(classes[rec["error"]], match=FORMS[case]):
            get_model(rec["par"])
    else:
        model = get_model(rec["par"])
        with pytest.raises(classes[rec["error"]], match=FORMS[case]) as e:
            build_layout(model, toas)
        if case.startswith("free_"):
            assert "unfittable" in str(e.value) and "unfittable" in rec["message"]


def test_sifunc_0_needs_three_points():
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    _, toas, _, _ = load("wave_wls")
    par = _par("wave_wls").replace("SIFUNC 2 0", "SIFUNC 0 0")
    build_layout(get_model(par), toas)
    two = "\n".join(l for l in par.splitlines() if not l.startswith(("IFUNC3", "IFUNC4", "IFUNC5", "IFUNC6"))) + "\n"
    with pytest.raises(ValueError, match="three"):
        build_layout(get_model(two), toas)
    build_layout(get_model(two.replace("SIFUNC 0 0", "SIFUNC 2 0")), toas)


def test_caps():
    """The count at each cap builds a layout; one more is refused, naming the macro."""
    from pint_amd import _lib as L
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    _, toas, _, _ = load("pw_wls")
    bare = _par_without("pw_wls", "PiecewiseSpindown")

    def pieces(k):
        return "".join(f"PWSTART_{i} {54500 + 10 * i}.1\nPWSTOP_{i} {54505 + 10 * i}.2\nPWEP_{i} {54502 + 10 * i}.3\n"
                       f"PWPH_{i} 0.1\nPWF0_{i} 1e-9\nPWF1_{i} 0\nPWF2_{i} 0\n" for i in range(1, k + 1))

    def waves(k):
        return "WAVE_OM 0.005\n" + "".join(f"WAVE{i} 1e-4 -1e-4\n" for i in range(1, k + 1))

    def ifuncs(k):
        return "SIFUNC 2\n" + "".join(f"IFUNC{i} {54000 + i}.5 1e-4\n" for i in range(1, k + 1))

    assert (L.MAX_PW, L.MAX_WAVE, L.MAX_IFUNC, L.COL_PW, L.PW_NPAR) == (64, 128, 1024, 21, 7)
    for make, cap, macro, at in ((pieces, 64, "PINT_MAX_PW", 1), (waves, 128, "PINT_MAX_WAVE", 3),
                                 (ifuncs, 1024, "PINT_MAX_IFUNC", 5)):
        lay = build_layout(get_model(bare + make(cap)), toas)
        assert lay.phase_terms[at] == cap
        with pytest.raises(NotImplementedError, match=macro):
            build_layout(get_model(bare + make(cap + 1)), toas)


def test_layout():
    """The block offsets, the PINT_COL_PW indices and the arguments of pint_set_phase_terms; the
    spec keeps its size, and a model without the components makes no call."""
    import golden_util
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout, pack_table
    assert C.sizeof(L.SpecT) == 4128
    model, toas, z, meta = load("pw_wls")
    lay = build_layout(model, toas)
    assert lay.columns == meta["dm_params"]
    o_pw, npw, o_wave, nwave, sifunc, nif = lay.phase_terms[:6]
    idx = model.pw_indices()
    assert (npw, o_wave, nwave, nif) == (3, -1, 0, 0) and idx == [1, 2, 3] and lay.pairs == []
    tab = pack_table(lay)
    for k, i in enumerate(idx):
        for w, pre in enumerate(PW_PROPS):
            o = lay.offsets[f"{pre}{i}"]
            assert o == o_pw + 14 * k + 2 * w
            assert LD(tab[o]) + LD(tab[o + 1]) == LD(model[f"{pre}{i}"].value)
        for w, pre in enumerate(PW_FIT):
            if f"{pre}{i}" in lay.columns:
                c = lay.columns.index(f"{pre}{i}")
                assert lay.spec.col_kind[c] == L.COL_PW and lay.spec.col_index[c] == 4 * k + w
                assert lay.spec.col_toff[c] == lay.offsets[f"{pre}{i}"]
    assert o_pw + 14 * npw <= lay.tstride
    assert sum(lay.spec.col_kind[c] == L.COL_PW for c in range(lay.spec.ncol)) == 5
    # the par-file order of the pieces does not matter to the layout or the table
    from pint_amd import get_model
    lines = _par("pw_wls").splitlines()
    pw = [l for l in lines if l.startswith("PW")]
    other = get_model("\n".join([l for l in lines if not l.startswith("PW")] + pw[14:] + pw[:14]) + "\n")
    other.free_params = model.free_params
    lb = build_layout(other, toas)
    assert lb.offsets == lay.offsets and pack_table(lb).tobytes() == tab.tobytes()

    model, toas, z, meta = load("wave_wls")
    lay = build_layout(model, toas)
    assert lay.columns == meta["dm_params"]
    o_pw, npw, o_wave, nwave, sifunc, nif, xh, xl, yy = lay.phase_terms
    assert (o_pw, npw, nwave, sifunc, nif) == (-1, 0, 5, 2, 6)
    assert lay.offsets["WAVEEPOCH"] == o_wave and lay.offsets["WAVE_OM"] == o_wave + 2
    assert lay.pairs == [(o_wave + 4 + 2 * k, f"WAVE{k + 1}") for k in range(5)] and o_wave + 14 <= lay.tstride
    tab = pack_table(lay)
    for slot, p in lay.pairs:
        assert (tab[slot], tab[slot + 1]) == tuple(float(v) for v in model[p].value)
    assert not any(p.startswith(("WAVE", "IFUNC")) and p not in ("WAVEEPOCH", "WAVE_OM") for p in lay.offsets)
    x = np.array([model[p].value[0] for p in model.ifunc_terms()], dtype=LD)
    assert np.all(xh.astype(LD) + xl.astype(LD) == x) and xh.dtype == xl.dtype == yy.dtype == np.float64
    assert list(yy) == [float(model[p].value[1]) for p in model.ifunc_terms()]
    # descending points are refused on the host
    bad = get_model(_par("wave_wls").replace("IFUNC2 54700.5", "IFUNC2 54900.5"))
    with pytest.raises(ValueError, match="ascend"):
        build_layout(bad, toas)
    # a model with none of the three: no call, and the table it had
    m, t, _, _ = golden_util.load("pta_iso")
    plain = build_layout(m, t)
    assert plain.phase_terms is None and plain.pairs == []
    m, t = load("pw_wls", par=_par_without("pw_wls", "PiecewiseSpindown"))[:2]
    assert build_layout(m, t).phase_terms is None


def test_wideband_refused():
    from pint_amd import WLSFitter

    class WB:
        def is_wideband(self):
            return True
    for name, comp in (("pw_wls", "PiecewiseSpindown"), ("wave_wls", "Wave")):
        model = load(name)[0]
        with pytest.raises(NotImplementedError, match=comp):
            WLSFitter(WB(), model)


def _check_params(model, rec, prefixes):
    names = [p for p in model.params if p.startswith(prefixes) and model[p].value is not None]
    assert sorted(names) == sorted(rec)
    for p in names:
        vals = model[p].value if model[p].kind == "pair" else [model[p].value]
        assert model[p].frozen == rec[p]["frozen"], p
        for v, (hi, lo) in zip(vals, rec[p]["value"]):
            assert LD(v) == LD(hi) + LD(lo), (p, v, hi, lo)


def test_translation_helpers():
    """translate_wave_to_wavex and translate_wavex_to_wave (utils.py:1794, :1957) against the
    reference's results on the wave_wls model: parameters, values and fit flags."""
    from pint_amd.wavex import translate_wave_to_wavex, translate_wavex_to_wave
    model, toas, z, meta = load("wave_wls")
    wx = translate_wave_to_wavex(model)
    assert "WaveX" in wx.components and "Wave" not in wx.components and "Wave" in model.components
    assert ("WaveX" in meta["wave_to_wavex_components"]) and ("Wave" not in meta["wave_to_wavex_components"])
    assert not any(p.startswith("WAVE") for p in wx.params)
    _check_params(wx, meta["wave_to_wavex"], ("WX",))
    back = translate_wavex_to_wave(wx)
    assert "Wave" in back.components and "WaveX" not in back.components
    _check_params(back, meta["wavex_to_wave"], ("WAVE",))
    wx.WXFREQ_0003.value = wx.WXFREQ_0003.value * 1.5
    with pytest.raises(ValueError, match="consistent WAVEOM"):
        translate_wavex_to_wave(wx)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
def _phase(model, toas):
    from pint_amd.engine import evaluate_delay_phase
    dp = evaluate_delay_phase(model, toas)
    return dp["phase_hi"].astype(LD) + dp["phase_lo"].astype(LD), dp


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_phase_residuals_columns(name):
    from pint_amd import Residuals
    model, toas, z, meta = load(name)
    n = toas.ntoas
    F0 = float(model.F0.value)
    got, dp = _phase(model, toas)
    assert np.max(np.abs(dp["delay"] - z["delay_total"])) <= 5e-12 and abs(dp["tzr_delay"] - z["tzr_delay"][0]) <= 5e-12
    # the absolute phase of the TOAs and of the TZR row, in total
    ref = z["abs_phase_int"].astype(LD) + z["abs_phase_frac_hi"].astype(LD) + z["abs_phase_frac_lo"].astype(LD)
    ref_tz = LD(z["tzr_abs_phase_int"][0]) + LD(z["tzr_abs_phase_frac_hi"][0]) + LD(z["tzr_abs_phase_frac_lo"][0])
    ph_bar = 1e-10 * F0 + 8 * float(np.spacing(np.max(np.abs(ref))))
    e_ph, e_phz = float(np.max(np.abs(got[:n] - ref))), float(abs(got[n] - ref_tz))
    print(f"{name}: phase {e_ph:.2e} / TZR {e_phz:.2e} cycles (bar {ph_bar:.1e})")
    assert e_ph <= ph_bar and e_phz <= ph_bar
    # per component: the phase with the component less the phase without it
    for comp, key in COMPONENT_KEY.items():
        if comp not in model.components:
            continue
        less, _ = _phase(load(name, par=_par_without(name, comp))[0], toas)
        mine = got - less
        want, want_tz = _ld(z, key), _ld(z, "tzr_" + key)[0]
        bar = 1e-10 * F0 + 8 * float(np.spacing(np.max(np.abs(want))))
        e, ez = float(np.max(np.abs(mine[:n] - want))), float(abs(mine[n] - want_tz))
        print(f"{name}: {comp} phase {e:.2e} / TZR {ez:.2e} cycles (bar {bar:.1e}), up to {float(np.max(np.abs(want))):.4g}")
        assert e <= bar and ez <= bar, comp
    e_r = np.max(np.abs(Residuals(toas, model).time_resids - z["res_time"]))
    print(f"{name}: residuals {e_r:.2e} s")
    assert e_r <= 1e-9
    # the columns: the pieces' against the reference's, exact zeros outside the window; every other
    # column equal bit for bit to the same model's without the three components
    M, params, _ = model.designmatrix(toas)
    assert list(params) == meta["dm_params"]
    refM = z["dm_M"]
    t = _times(name)[0]
    wins = _windows(model) if "PiecewiseSpindown" in model.components else {}
    pwj = []
    for i, lst in _pw_cols(params).items():
        off = ~((t >= wins[i][0]) & (t < wins[i][1]))
        assert 20 <= np.sum(off) <= n - 20
        for j, p in lst:
            pwj.append(j)
            err = np.max(np.abs(M[:, j] - refM[:, j])) / np.max(np.abs(refM[:, j]))
            print(f"{name}: column {p} {err:.2e} of its maximum")
            assert err <= COL_BAR, p
            assert np.all(M[off, j] == 0.0) and np.all(refM[off, j] == 0.0), p
    bare = load(name, par=_par_without(name, *COMPONENT_KEY))[0]
    Mb, pb, _ = bare.designmatrix(toas)
    assert list(pb) == [p for j, p in enumerate(params) if j not in pwj]
    np.testing.assert_array_equal(Mb, M[:, [j for j in range(len(params)) if j not in pwj]])
    scale = np.max(np.abs(refM), axis=0)
    scale[scale == 0] = 1
    assert np.max(np.abs(M - refM) / scale) <= 1e-9


@pytest.mark.gpu
def test_gpu_ifunc_sifunc_0():
    """SIFUNC 0 as the reference runs it: the device's IFunc times at the TOAs and at the TZR TOA
    against the recorded array, which holds all three cases."""
    name = "wave_wls"
    model, toas, z, meta = load(name, par=_par(name).replace("SIFUNC 2 0", "SIFUNC 0 0"))
    less = load(name, par=_par_without(name, "IFunc"))[0]
    n = toas.ntoas
    F0 = LD(model.F0.value)
    got = (_phase(model, toas)[0] - _phase(less, toas)[0]) / F0
    want = np.concatenate([_ld(z, "ifunc0_phase"), _ld(z, "tzr_ifunc0_phase")]) / F0
    assert len(set(np.round(want[:n].astype(np.float64), 9))) == 3
    err = float(np.max(np.abs(got - want)))
    print(f"SIFUNC 0 times: {err:.2e} s")
    assert err <= 1e-10


@pytest.mark.gpu
def test_gpu_at_the_caps():
    """128 WAVE terms (the rotation recurrence at its longest), 1024 IFUNC points (a ten-deep search)
    and 64 pieces, every other one overlapping its neighbours, on wave_wls's TOAs: the three
    components' phase, the model's phase with them less its phase without, against the reference's
    formulas (wave.py:148-168, ifunc.py:136-144, piecewise.py:181-211) evaluated here in numpy
    longdouble at the reference's recorded delays.  Bar: 1e-10 s x F0 plus 8 ulps of the largest
    term."""
    name = "wave_wls"
    bare = _par_without(name, "Wave", "IFunc")
    rng = np.random.default_rng(5)
    # (plain Python floats, so the par text is repr's round-trip decimals; the epochs are binary
    # fractions, which every parser reads alike; a control point read from its decimals as a
    # longdouble differs from the float64 by < 1e-11 d, 1e-14 s on these slopes)
    a = (rng.normal(size=(128, 2)) * 2e-3 / np.arange(1, 129)[:, None]).tolist()
    x = (np.round(np.sort(54480.0 + rng.uniform(0, 1140, 1024)) * 1024) / 1024).tolist()
    y = (rng.normal(size=1024) * 1e-3).tolist()
    starts = (54490.25 + 17.0 * np.arange(64)).tolist()
    pw = (rng.normal(size=(64, 4)) * np.array([0.3, 1e-5, 1e-13, 1e-21])).tolist()
    a, x, y, starts, pw = np.array(a), np.array(x), np.array(y), np.array(starts), np.array(pw)
    r = lambda v: repr(float(v))  # noqa: E731
    par = bare + "WAVEEPOCH 54900\nWAVE_OM 0.0057119866\n" + "".join(
        f"WAVE{k + 1} {r(a[k, 0])} {r(a[k, 1])}\n" for k in range(128)) + "SIFUNC 2\n" + "".join(
        f"IFUNC{k + 1} {r(x[k])} {r(y[k])}\n" for k in range(1024)) + "".join(
        f"PWSTART_{k + 1} {r(starts[k])}\nPWSTOP_{k + 1} {r(starts[k] + 30.0)}\nPWEP_{k + 1} {r(starts[k] + 7.0)}\n"
        f"PWPH_{k + 1} {r(pw[k, 0])}\nPWF0_{k + 1} {r(pw[k, 1])}\nPWF1_{k + 1} {r(pw[k, 2])}\nPWF2_{k + 1} {r(pw[k, 3])}\n"
        for k in range(64))
    model, toas, z, meta = load(name, par=par)
    less = load(name, par=bare)[0]
    n = toas.ntoas
    F0 = LD(model.F0.value)
    t, tz, ts, tsz = _times(name)
    tt = np.concatenate([t, [tz]])
    dl = np.concatenate([z["delay_total"], z["tzr_delay"]]).astype(LD)
    tb = tt - dl / LD(86400)
    assert np.min(np.abs(tb[:, None] - x[None, :].astype(LD))) * 86400 > 1e-3  # no row at a control point
    edges = np.concatenate([starts, starts + 30.0]).astype(LD)
    assert np.min(np.abs(tt[:, None] - edges[None, :])) * 86400 > 1e-3         # nor at a window's edge
    b = LD(model.WAVE_OM.value) * (tt - LD(54900) - dl / LD(86400))
    want = np.zeros(n + 1, dtype=LD)
    for k in range(128):
        want += (LD(a[k, 0]) * np.sin((k + 1) * b) + LD(a[k, 1]) * np.cos((k + 1) * b)) * F0
    xl, yl = x.astype(LD), y.astype(LD)
    idx = np.searchsorted(xl, tb)
    mid = (idx > 0) & (idx < 1024)
    im = idx[mid]
    times = np.where(idx == 0, yl[0], yl[-1])
    dx1, dx2 = tb[mid] - xl[im - 1], xl[im] - tb[mid]
    times[mid] = (yl[im] * dx1 + yl[im - 1] * dx2) / (dx1 + dx2)
    want += times * F0
    biggest, both = 0.0, 0
    for k in range(64):
        inside = (tt >= LD(starts[k])) & (tt < LD(starts[k] + 30.0))
        dt = (tt[inside] - LD(starts[k] + 7.0)) * 86400 - dl[inside]
        term = LD(pw[k, 0]) + dt * (LD(pw[k, 1]) + dt * (LD(pw[k, 2]) / 2 + dt * LD(pw[k, 3]) / 6))
        want[inside] += term
        biggest = max(biggest, float(np.max(np.abs(term), initial=0.0)))
        both += int(np.sum(inside))
    assert both > n and biggest > 1.0  # the windows overlap: more memberships than TOAs
    got = _phase(model, toas)[0] - _phase(less, toas)[0]
    bar = 1e-10 * float(F0) + 8 * float(np.spacing(LD(max(biggest, float(np.max(np.abs(want)))))))
    err = float(np.max(np.abs(got - want)))
    print(f"caps: 128 WAVE + 1024 IFUNC + 64 pieces: {err:.2e} cycles (bar {bar:.1e}), up to {float(np.max(np.abs(want))):.4g}")
    assert err <= bar


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
    from pint_amd import GLSFitter, Residuals, WLSFitter
    model, toas, z, meta = load(name)
    key = "gls" if name == "pw_gls" else "wls"
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (GLSFitter if key == "gls" else WLSFitter)(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, key, 1e-5 if key == "gls" else 1e-6)
    if key == "gls":
        e_post = np.max(np.abs(f.resids.time_resids - z["gls_post_resid"]))
        pre = rms_ps(f.resids.time_resids, z["gls_post_resid"])
        print(f"{name}: post-fit residuals {e_post:.2e} s")
        assert e_post <= 1e-9
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
    f = (DownhillGLSFitter if name == "pw_gls" else DownhillWLSFitter)(toas, model)
    try:
        f.fit_toas(maxiter=10)
        status = "converged"
    except (MaxiterReached, StepProblem) as e:
        status = type(e).__name__
    assert status == meta["down_status"]
    bar = chi2_bar(name, "down", pre)
    dev = {p: abs(float((LD(f.model[p].value) - ref_value(meta, "down_params", p)) / LD(meta["down_errors"][p])))
           for p in meta["down_params"]}
    pw = max(dev, key=dev.get)
    print(f"{name}: Downhill {status}, chi2 rel {f.resids.chi2 / meta['down_chi2'] - 1:.2e} (bar {bar:.1e}), "
          f"worst {dev[pw]:.2e} sigma ({pw}, bar {downhill_bar(name, pw):.1e})")
    assert abs(f.resids.chi2 / meta["down_chi2"] - 1) < bar
    for p, d in dev.items():
        assert d < downhill_bar(name, p), (p, d, downhill_bar(name, p))


@pytest.mark.gpu
def test_gpu_grid_pwf0_f0():
    """The reference's 5x5 (PWF0_1, F0) grid_chisq around the one-step fit, by the chi2 rule; the
    same argmin.  The grid is the reference's executor path (every point fitted on a copy of the
    base model, as the device's independent points are); its single-process path, which carries
    each point's fitted parameters into the next, is recorded beside it (grid_chi2_serial) and
    agrees with it to 2e-8 of chi2 on this fixture."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    model, toas, z, meta = load("pw_wls")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    f.fit_toas(maxiter=1)
    c2, _ = grid_chisq(f, ("PWF0_1", "F0"), (_ld(z, "grid_PWF0_1"), _ld(z, "grid_F0")))
    ref = z["grid_chi2"]
    bar = max(1e-7, chi2_bar("pw_wls", "fit", pre))
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"pw_wls: (PWF0_1, F0) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}")
    assert c2.shape == ref.shape == (5, 5)
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)

@pytest.mark.gpu
def test_gpu_row_block_edges():
    """The first 256 TOAs of pw_wls (the TZR row alone in the second row block), the first 255 and
    the first 257: the same per-row phases and piece columns, bit for bit, as the full fixture's
    rows."""
    model, toas, z, meta = load("pw_wls")
    full, _ = _phase(model, toas)
    M, params, _ = model.designmatrix(toas)
    pwj = [j for lst in _pw_cols(params).values() for j, _ in lst]
    assert len(pwj) == 5
    for k in (255, 256, 257):
        sub = toas[:k]
        got, _ = _phase(model, sub)
        assert len(got) == k + 1
        np.testing.assert_array_equal(got[:k], full[:k])
        assert got[k] == full[toas.ntoas]
        Mk, pk, _ = model.designmatrix(sub)
        assert list(pk) == list(params)
        np.testing.assert_array_equal(Mk[:, pwj], M[:k, pwj])
        assert np.max(np.abs(Mk[:, pwj]), axis=0).min() > 0


def _steps(items, mode, want):
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    s = Session()
    bf = BatchFit([(copy.deepcopy(m), t) for m, t in items], mode=mode, session=s)
    s.eval(want_M=want)
    s.fit_step(1 if mode == "gls" else 0)
    dp, er, cov, cl = s.read_step()
    c2 = s.chi2_gls() if mode == "gls" else s.chi2_wls()
    out = [(np.array(dp[k], copy=True), np.array(er[k], copy=True), float(cl[k]), float(c2[k])) for k in range(len(items))]
    bf.close()
    s.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ("compact", "full"))
def test_gpu_mixed_batch(layout):
    """pw_wls, wave_wls and a fixture without the components (gl_wls) in one BatchFit, in the fit
    layout and in the full layout: the last one's step, errors and chi2 are bit-identical to its
    outputs alone, and the first two match theirs.  The same for pw_gls beside gl_gls, whose fit
    layout is the compact one (DMX columns as bin sums)."""
    from pint_amd.engine import Session
    want = Session.FIT if layout == "compact" else True
    for mode, with_terms, plain in (("wls", ("pw_wls", "wave_wls"), "gl_wls"), ("gls", ("pw_gls",), "gl_gls")):
        items = [load(n)[:2] for n in with_terms + (plain,)]  # (the glitch fixtures load the same way)
        mixed = _steps(items, mode, want)
        for k in range(len(items)):
            (alone,) = _steps([items[k]], mode, want)
            if k == len(items) - 1:
                for x, y in zip(mixed[k], alone):
                    np.testing.assert_array_equal(x, y)
                continue
            # a batch picks its own row split of the Gram, so the normal equations differ in their
            # last bits and the solve carries that: the project's bars for the same normal equations
            # to rounding (test_glitch.py's compact-against-full check): the step within 1e-8 of
            # the uncertainty, the uncertainties within 1e-9, the chi2 within 1e-10
            (d1, e1, l1, g1), (d0, e0, l0, g0) = mixed[k], alone
            n = len(e0) - 1
            assert np.max(np.abs((d1[:n] - d0[:n]) / e0[:n])) < 1e-8
            assert np.max(np.abs(e1[:n] / e0[:n] - 1)) < 1e-9
            assert abs(l1 / l0 - 1) < 1e-10 and abs(g1 / g0 - 1) < 1e-10


@pytest.mark.gpu
def test_gpu_setter_validation():
    """Each bad pint_set_phase_terms call returns PINT_E_INVALID and leaves the pulsar as it was:
    after them the evaluation gives the bits of a session that never saw a bad call."""
    from pint_amd import _lib as L
    from pint_amd.engine import Session, build_layout, pack_table
    out = []
    for name in ("pw_wls", "wave_wls"):
        model, toas, z, meta = load(name)
        for abuse in (False, True):
            s = Session()
            lay = s.add(build_layout(model, toas))
            if abuse:
                o_pw, npw, o_wave, nwave, sifunc, nif, xh, xl, yy = lay.phase_terms
                p = L.ptr
                x3, down = np.array([1.0, 2.0, 3.0]), np.array([1.0, 3.0, 2.0])
                zero = np.zeros(3)
                ts = lay.tstride
                bad = [
                    (-1, 1, -1, 0, 0, 0, None, None, None),              # a piece without a slot
                    (0, L.MAX_PW + 1, -1, 0, 0, 0, None, None, None),    # one piece too many
                    (0, -1, -1, 0, 0, 0, None, None, None),              # a negative count
                    (ts - 13, 1, -1, 0, 0, 0, None, None, None),         # a piece block past the table
                    (-1, 0, ts - 5, 1, 0, 0, None, None, None),          # a Wave block past the table
                    (-1, 0, 0, L.MAX_WAVE + 1, 0, 0, None, None, None),  # one term too many
                    (-1, 0, -1, 1, 0, 0, None, None, None),              # terms without a slot
                    (-1, 0, -1, 0, 2, 3, None, p(zero), p(zero)),        # null pointers
                    (-1, 0, -1, 0, 2, 3, p(x3), None, p(zero)),
                    (-1, 0, -1, 0, 2, 3, p(x3), p(zero), None),
                    (-1, 0, -1, 0, 2, 3, p(down), p(zero), p(zero)),     # descending x
                    (-1, 0, -1, 0, 1, 3, p(x3), p(zero), p(zero)),       # SIFUNC 1
                    (-1, 0, -1, 0, 0, 2, p(x3), p(zero), p(zero)),       # SIFUNC 0 with two points
                    (-1, 0, -1, 0, 2, L.MAX_IFUNC + 1, p(x3), p(zero), p(zero)),
                ]
                for args in bad:
                    assert s.L.pint_set_phase_terms(s.ctx, lay.psr_id, *args) == L.PINT_E_INVALID, args[:6]
                assert s.L.pint_set_phase_terms(s.ctx, lay.psr_id + 7, *lay.phase_terms[:6], p(xh), p(xl), p(yy)) == L.PINT_E_INVALID
                # (a good call again: the same description)
                assert s.L.pint_set_phase_terms(s.ctx, lay.psr_id, o_pw, npw, o_wave, nwave, sifunc, nif, p(xh), p(xl),
                                                p(yy)) == L.PINT_OK
            s.set_instances([(lay, pack_table(lay))])
            s.eval(True)
            res = [np.array(x[0], copy=True) for x in s.read_eval()] + [np.array(s.read_designmatrix()[0], copy=True)]
            s.fit_step(0)
            dpar, er, _, cl = s.read_step()
            res += [np.array(dpar[0], copy=True), np.array(er[0], copy=True)]
            s.close()
            out.append(res)
    for a, b in ((out[0], out[1]), (out[2], out[3])):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
