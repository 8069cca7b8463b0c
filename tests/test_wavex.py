"""The WaveX and DMWaveX components (wavex.py, dmwavex.py) on the device path, against fixtures
captured from the reference (scripts/refgen/gen_wavex.py):

* wx_wls : WLS, an isolated pulsar with WaveX harmonics 0001, 0002 (negative frequency, WXSIN free
           and WXCOS frozen non-zero) and 0004 (non-harmonic), WXEPOCH != PEPOCH, and one glitch
           inside the span (k_wavex runs before k_glitch); 400 TOAs: two row blocks, the second
           partial, the TZR row in it;
* wx_gls : GLS, the bench's per-pulsar shape (ELL1, DMX, red noise) with 5 WaveX and 4 DMWaveX
           harmonics from the reference's wavex_setup / dmwavex_setup, DMWXEPOCH from PEPOCH.

Bars.  Delays (total, TZR, the two components'), absolute phase (as time: x F0, plus 8 ulps of
the reference's longdouble phase) and residuals: 1 ns.  WaveX / DMWaveX columns, relative to the
column's largest magnitude: 8 x 2^-53 x (1 + max |a'|), max |a'| the fixture's largest argument
(the reference rounds 2 pi f dt three times; no other evaluation can agree with it better); the
other columns the project's 1e-9.  Fits 1e-3 sigma; chi2 by golden_util.chi2_bar's rule on
wx_fit_spread.json; Downhill by its "downhill" spread.
"""
import copy
import hashlib
import json
import os
import warnings

import numpy as np
import pytest

from golden_util import GOLDEN, ref_value, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
NAMES = ("wx_wls", "wx_gls")
STEMS = {"WaveX": "WX", "DMWaveX": "DMWX"}
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
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (wx_wls: "Frequency WXFREQ_0002 is negative", test_validate)
        model = get_model(os.path.join(GOLDEN, name + ".par"))
    return model, toas, z, meta


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "wx_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on wx_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def downhill_bar(name, p, floor=1e-3):
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _wx_cols(params):
    return [(j, p) for j, p in enumerate(params) if p.startswith(("WXSIN_", "WXCOS_", "DMWXSIN_", "DMWXCOS_"))]


def _col_bar(meta):
    return 8 * 2.0 ** -53 * (1 + meta["wx_max_arg"])


def _args(name):
    """{FREQ parameter: (a', a)} in longdouble: a' = 2 pi f (tdbld - epoch), a = a' - 2 pi f D with
    D the delay accumulated before wavex_delay (days)."""
    model, toas, z, meta = load(name)
    t = z["tdb_hi"].astype(LD) + z["tdb_lo"].astype(LD)
    D = (z["delay_total"] - z["wavex_delay"] - z.get("dmwavex_delay", 0.0)).astype(LD) / 86400
    out = {}
    for stem in STEMS.values():
        for n in model.params:
            if n.startswith(stem + "FREQ_"):
                w = 2 * LD(np.pi) * LD(model[n].value)
                ap = w * (t - LD(model[stem + "EPOCH"].value))
                out[n] = (ap, ap - w * D)
    return out


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on: every free WaveX / DMWaveX column has a non-zero maximum; the
    component delays exceed 100 ns, so no 1 ns test passes with a term missing; in wx_gls sin a and
    sin a' differ by more than 1e-6, so none passes with the two arguments confused; max |a'| is
    the recorded one; the design matrix is solvable (the reference's own figures)."""
    model, toas, z, meta = load(name)
    cols = _wx_cols(meta["dm_params"])
    assert cols
    for j, p in cols:
        assert np.max(np.abs(z["dm_M"][:, j])) > 0, p
    assert np.max(np.abs(z["wavex_delay"])) > 100e-9
    args = _args(name)
    amax = max(float(np.max(np.abs(ap))) for ap, _ in args.values())
    assert abs(amax / meta["wx_max_arg"] - 1) < 1e-12
    if name == "wx_gls":
        assert np.max(np.abs(z["dmwavex_delay"])) > 100e-9
        dsin = max(float(np.max(np.abs(np.sin(a) - np.sin(ap)))) for n, (ap, a) in args.items() if n.startswith("WX"))
        assert dsin > 1e-6
        assert len([p for _, p in cols if p.startswith("WX")]) == 10 and len(cols) == 18
    else:
        assert n_rows_two_blocks(toas.ntoas)
        assert model.WXFREQ_0002.value < 0 and model.WXCOS_0002.frozen and model.WXCOS_0002.value != 0
        assert model.WXEPOCH.value != model.PEPOCH.value
    assert meta["wx_gram_cond"] < 1e12
    key = "wls" if name == "wx_wls" else "gls"
    assert all(np.isfinite(v) and v > 0 for v in meta[key + "_errors"].values())


def n_rows_two_blocks(n):
    """n TOAs + the TZR row fill one 256-row block and part of a second."""
    return 256 < n + 1 < 512


@pytest.mark.parametrize("name", NAMES)
def test_layout(name):
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout
    model, toas, z, meta = load(name)
    assert model.free_params == meta["model"]["free_params"]
    assert [p for p in model.params if "WX" in p] == [p for p in meta["model"]["params"] if "WX" in p]
    assert [c for c in model.components if "Wave" in c] == [c for c in meta["model"]["components"] if "Wave" in c]
    lay = build_layout(model, toas)
    assert lay.columns == meta["dm_params"]
    assert lay.wavex is not None
    for (comp, stem), kind, (o, nh) in zip(STEMS.items(), (L.COL_WX, L.COL_DMWX), (lay.wavex[:2], lay.wavex[2:])):
        idx = model.wavex_indices(comp)
        assert nh == len(idx) and idx == sorted(idx)
        if not idx:
            assert o == -1 and comp not in model.components
            continue
        assert lay.offsets[stem + "EPOCH"] == o - 2
        assert o + 6 * nh <= lay.tstride
        for k, i in enumerate(idx):
            assert lay.offsets[f"{stem}FREQ_{i:04d}"] == o + 6 * k
            for w, part in enumerate(("SIN", "COS")):
                p = f"{stem}{part}_{i:04d}"
                assert lay.offsets[p] == o + 6 * k + 2 + 2 * w
                if p in lay.columns:
                    c = lay.columns.index(p)
                    assert lay.spec.col_kind[c] == kind and lay.spec.col_index[c] == 2 * k + w
                    assert lay.spec.col_toff[c] == lay.offsets[p]
    if name == "wx_gls":  # no DMWXEPOCH line: PEPOCH
        assert model.DMWXEPOCH.value == model.PEPOCH.value and model.WXEPOCH.value == 54900
    else:  # the gap: indices 1, 2, 4 take positions 0, 1, 2
        assert model.wavex_indices() == [1, 2, 4]
        assert list(model.get_wavex_indices()) == [1, 2, 4]


def test_layout_without_wavex_is_the_parents():
    """pta_iso has neither component: its table, offsets and spec bytes hash to the values
    test_glitch.py records, and its layout asks for no pint_set_wavex call."""
    import golden_util
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout, pack_table
    model, toas, z, meta = golden_util.load("pta_iso")
    lay = build_layout(model, toas)
    assert lay.wavex is None
    assert hashlib.sha256(pack_table(lay).tobytes()).hexdigest() == \
        "d50cf50a3018718c5effddf8a65b45cb702d696e8780a3a01f413b7973bcc81f"
    assert hashlib.sha256(repr(list(lay.offsets.items())).encode()).hexdigest() == \
        "ca1ee53fe23016db57b8fdb8e518568678f5375e3dd94c52cb4720b0294bdfe8"
    b = bytes(lay.spec)
    o = L.SpecT.o_GLITCH.offset
    assert hashlib.sha256(b[:o] + bytes(4) + b[o + 20:]).hexdigest() == \
        "d993d9149f99392cd1bc13abec1128320ac9b59fef1cc91d1acf4ae1c21924ee"
    assert (L.COL_WX, L.COL_DMWX, L.MAX_WAVEX) == (15, 16, 128)


@pytest.mark.parametrize("name", NAMES)
def test_parfile_round_trip(name):
    """The post-fit model (the reference's fitted values and uncertainties) writes WaveX / DMWaveX
    lines equal to the reference's as_parfile text, in its order; reading them back gives the same
    values, fit flags and uncertainties."""
    from pint_amd import get_model
    model, toas, z, meta = load(name)
    key = "wls" if name == "wx_wls" else "gls"
    for p, s in meta[key + "_errors"].items():
        v = ref_value(meta, key + "_params", p)
        model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
        model[p].uncertainty = s
    ref = [l for l in meta[key + "_parfile"].splitlines() if l.split() and "WX" in l.split()[0]]
    got = [l for l in model.as_parfile().splitlines() if l.split() and "WX" in l.split()[0]]
    assert len(ref) == (10 if name == "wx_wls" else 29) and got == ref
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        back = get_model(model.as_parfile())
    assert [p for p in back.params if "WX" in p] == [p for p in model.params if "WX" in p]
    for p in model.params:
        if "WX" in p:
            a, b = model[p], back[p]
            assert a.value == b.value and a.frozen == b.frozen, p
            assert (a.uncertainty_value or 0.0) == (b.uncertainty_value or 0.0), p


BASE = "PSR X\nRAJ 10:12:33.4 1\nDECJ 53:07:02.5 1\nF0 218.8 1\nF1 -4e-16 1\nPEPOCH 55000\nDM 9.02 1\nEPHEM builtin\nUNITS TDB\n"


def _h(stem, i, f="0.001", parts=("FREQ", "SIN", "COS")):
    vals = {"FREQ": f"{stem}FREQ_{i:04d} {f}\n", "SIN": f"{stem}SIN_{i:04d} 1e-6 1\n", "COS": f"{stem}COS_{i:04d} 1e-6 1\n"}
    return "".join(vals[p] for p in parts)


@pytest.mark.parametrize("stem", ("WX", "DMWX"))
def test_validate(stem):
    """The reference's validation, each by type (wavex.py:303-360, dmwavex.py:293-350), and what
    its model builder does around it (recorded from it by scripts/refgen/gen_wavex.py and by hand:
    the component always has harmonic 0001, at 0.1 / d with free zero amplitudes when the par file
    does not give it; only the four-digit index is a parameter name)."""
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    from pint_amd.timing_model import MissingParameter
    comp = {v: k for k, v in STEMS.items()}[stem]
    with pytest.raises(ValueError, match=f"{stem}FREQ_ parameters do not match {stem}SIN_"):
        get_model(BASE + _h(stem, 1) + _h(stem, 2, parts=("SIN", "COS")))
    with pytest.raises(ValueError, match=f"{stem}FREQ_ parameters do not match {stem}COS_"):
        get_model(BASE + _h(stem, 1) + _h(stem, 2, parts=("FREQ", "SIN")))
    with pytest.raises(ValueError, match=f"{stem}FREQ_0001 is zero or None"):
        get_model(BASE + _h(stem, 1, f="0"))
    with pytest.raises(ValueError, match=f"{stem}FREQ_0002 is zero or None"):
        get_model(BASE + _h(stem, 1) + _h(stem, 2, f=""))
    with pytest.warns(UserWarning, match=f"Frequency {stem}FREQ_0001 is negative"):
        m = get_model(BASE + _h(stem, 1, f="-0.001"))
    assert comp in m.components and m[stem + "EPOCH"].value == m.PEPOCH.value  # the epoch fill-in
    with pytest.raises(MissingParameter):  # neither the epoch nor PEPOCH
        get_model(BASE.replace("PEPOCH 55000\n", "") + _h(stem, 1))
    # harmonic 0001 as the component is constructed; a missing SIN / COS of it is that default
    m = get_model(BASE + _h(stem, 3))
    assert [p for p in m.params if "WX" in p] == [stem + "EPOCH"] + [f"{stem}{q}_{i:04d}" for i in (1, 3)
                                                                    for q in ("FREQ", "SIN", "COS")]
    assert m[stem + "FREQ_0001"].value == 0.1 and m[stem + "SIN_0001"].value == 0.0 and not m[stem + "SIN_0001"].frozen
    m = get_model(BASE + _h(stem, 1, parts=("FREQ", "SIN")))
    assert m[stem + "COS_0001"].value == 0.0
    with pytest.warns(UserWarning, match="Unrecognized parfile line"):
        m = get_model(BASE + f"{stem}FREQ_1 0.001\n{stem}SIN_1 1e-6 1\n{stem}COS_1 1e-6 1\n")
    assert comp not in m.components
    # a free frequency: the reference's designmatrix refuses it (wx_wls.json "freq_fit")
    rec = load("wx_wls")[3]["freq_fit"]
    assert rec["designmatrix"] == "ValueError" and rec["in_free_params"]
    toas = load("wx_wls")[1]
    m = get_model(BASE + f"{stem}FREQ_0001 0.001 1\n" + _h(stem, 1, parts=("SIN", "COS")))
    assert stem + "FREQ_0001" in m.free_params
    with pytest.raises(ValueError, match="unfittable"):
        build_layout(m, toas)
    # the cap: 128 harmonics build a layout, 129 raise naming the limit
    many = "".join(f"{stem}FREQ_{i:04d} {0.0005 * i}\n{stem}SIN_{i:04d} 1e-7\n{stem}COS_{i:04d} 1e-7\n"
                   for i in range(1, 130))
    lay = build_layout(get_model(BASE + "".join(many.splitlines(True)[:3 * 128])), toas)
    assert lay.wavex[1 if stem == "WX" else 3] == 128
    with pytest.raises(NotImplementedError, match="PINT_MAX_WAVEX"):
        build_layout(get_model(BASE + many), toas)


@pytest.mark.parametrize("which", ("wavex", "dmwavex"))
def test_setup(which):
    """wavex_setup / dmwavex_setup against the indices, frequencies, fit flags and parameter order
    recorded from the reference (wx_wls.json "setup")."""
    import pint_amd
    from pint_amd import get_model
    rec = load("wx_wls")[3]["setup"]
    fn = getattr(pint_amd, which + "_setup")
    stem = "WX" if which == "wavex" else "DMWX"
    for case, kw in (("n3", dict(n_freqs=3)), ("list1", dict(freqs=[0.0025])),
                     ("frozen", dict(n_freqs=2, freeze_params=True))):
        r = rec[f"{which}_{case}"]
        m = get_model(BASE)
        idx = fn(m, 1000.0, **kw)
        assert [int(i) for i in idx] == r["indices"]
        assert [m[f"{stem}FREQ_{i:04d}"].value for i in r["indices"]] == r["freqs"]
        assert [p for p in m.params if "WX" in p] == r["params"]
        assert m.free_params == r["free_params"]
        assert [c for c in m.components if "Wave" in c] == [c for c in r["components"] if "Wave" in c]
        m.validate()
        assert m[stem + "EPOCH"].value == m.PEPOCH.value
    assert rec[f"{which}_both"] == "ValueError"
    with pytest.raises(ValueError, match="Both freqs and n_freqs"):
        fn(get_model(BASE), 1000.0, freqs=[0.001], n_freqs=1)
    with pytest.raises(ValueError, match="not specified"):
        fn(get_model(BASE), 1000.0)
    # a list of several frequencies: the reference's own call stops in a unit comparison of its
    # spacing warning (recorded); here it does what that code sets out to do -- sorted, 1, 2, 3
    assert rec[f"{which}_list"] == {"error": "UnitConversionError"}
    m = get_model(BASE)
    assert list(fn(m, 1000.0, freqs=[0.004, 0.001, 0.0025])) == [1, 2, 3]
    assert [m[f"{stem}FREQ_{i:04d}"].value for i in (1, 2, 3)] == [0.001, 0.0025, 0.004]


def test_add_remove_indices():
    """add_wavex_component(s), remove_wavex_component and get_wavex_indices as the reference's
    (wavex.py:63-289; the sequence below gives [2], [7, 5], indices 1 2 7 5, then 1 7 5, then 1
    there), and get_wavex_freqs / get_wavex_amps."""
    from pint_amd import get_model, get_wavex_amps, get_wavex_freqs
    m = get_model(BASE + _h("WX", 1))
    assert m.add_wavex_component(0.002, wxsin=1e-7) == 2
    assert list(m.get_wavex_indices()) == [1, 2]
    assert m.WXSIN_0002.value == 1e-7 and m.WXSIN_0002.frozen and m.WXFREQ_0002.frozen
    assert m.free_params == ["RAJ", "DECJ", "F0", "F1", "DM", "WXSIN_0001", "WXCOS_0001"]
    assert m.add_wavex_components([0.003, 0.004], indices=[7, 5], frozens=False) == [7, 5]
    assert list(m.get_wavex_indices()) == [1, 2, 7, 5] and m.wavex_indices() == [1, 2, 5, 7]
    assert m.free_params[-4:] == ["WXSIN_0007", "WXCOS_0007", "WXSIN_0005", "WXCOS_0005"]
    assert [p.name for p in get_wavex_freqs(m, [7, 5])] == ["WXFREQ_0007", "WXFREQ_0005"]
    assert get_wavex_freqs(m, 7, quantity=True) == [0.003]
    assert get_wavex_amps(m, 2, quantity=True) == (1e-7, 0.0)
    assert len(get_wavex_amps(m)) == 4
    with pytest.raises(ValueError, match="already in use"):
        m.add_wavex_component(0.002, index=1)
    with pytest.raises(ValueError, match="doesn't match"):
        m.add_wavex_components([0.01, 0.02], wxsins=[1, 2, 3])
    m.remove_wavex_component(2)
    assert list(m.get_wavex_indices()) == [1, 7, 5] and "WXSIN_0002" not in m and "WXSIN_0002" not in m.params
    m.remove_wavex_component([7, 5])
    assert list(m.get_wavex_indices()) == [1]
    with pytest.raises(TypeError):
        m.remove_wavex_component("1")
    # DMWaveX through the same methods
    assert m.add_wavex_component(0.002, component="DMWaveX") == 2
    assert list(m.get_wavex_indices("DMWaveX")) == [1, 2] and "DMWaveX" in m.components


def test_wideband_refused():
    """A fitter given wideband TOAs and a model with either component raises, naming it."""
    import golden_util
    from pint_amd import GLSFitter, WidebandTOAFitter, get_model
    toas = golden_util.load("wb_dd")[1]
    assert toas.is_wideband()
    for stem, comp in (("WX", "WaveX"), ("DMWX", "DMWaveX")):
        m = get_model(BASE + _h(stem, 1))
        for cls in (WidebandTOAFitter, GLSFitter):
            with pytest.raises(NotImplementedError, match=comp):
                cls(toas, m)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
def _zeroed(model, stem):
    m = copy.deepcopy(model)
    for p in m.params:
        if p.startswith((stem + "SIN_", stem + "COS_")):
            m[p].value = 0.0
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_delay_phase_residuals_columns(name):
    from pint_amd import Residuals
    from pint_amd.engine import evaluate_delay_phase
    model, toas, z, meta = load(name)
    model.free_params = meta["model"]["free_params"]
    n = toas.ntoas
    dp = evaluate_delay_phase(model, toas)
    e_d = np.max(np.abs(dp["delay"] - z["delay_total"]))
    e_tz = abs(dp["tzr_delay"] - z["tzr_delay"][0])
    # each component's delay: the total less the total with that component's amplitudes zero
    e_c = {}
    for stem, key in (("WX", "wavex_delay"), ("DMWX", "dmwavex_delay")):
        if key in z:
            d0 = evaluate_delay_phase(_zeroed(model, stem), toas)
            e_c[key] = max(float(np.max(np.abs((dp["delay"] - d0["delay"]) - z[key]))),
                           float(abs((dp["tzr_delay"] - d0["tzr_delay"]) - z["tzr_" + key][0])))
    got = dp["phase_hi"].astype(LD) + dp["phase_lo"].astype(LD)
    ref = z["abs_phase_int"].astype(LD) + z["abs_phase_frac_hi"].astype(LD) + z["abs_phase_frac_lo"].astype(LD)
    ref_tz = LD(z["tzr_abs_phase_int"][0]) + LD(z["tzr_abs_phase_frac_hi"][0]) + LD(z["tzr_abs_phase_frac_lo"][0])
    e_ph = float(np.max(np.abs(got[:n] - ref)))
    e_phz = float(abs(got[n] - ref_tz))
    ph_bar = 1e-9 * float(model.F0.value) + 8 * float(np.spacing(np.max(np.abs(ref))))
    r = Residuals(toas, model)
    e_r = np.max(np.abs(r.time_resids - z["res_time"]))
    M, params, _ = model.designmatrix(toas)
    assert list(params) == meta["dm_params"]
    refM = z["dm_M"]
    scale = np.max(np.abs(refM), axis=0)
    scale[scale == 0] = 1
    err = np.max(np.abs(M - refM) / scale, axis=0)
    wx = [j for j, _ in _wx_cols(params)]
    bar = _col_bar(meta)
    print(f"{name}: delay {e_d:.2e} s, TZR delay {e_tz:.2e} s, components {e_c}, phase {e_ph:.2e} / TZR {e_phz:.2e} "
          f"cycles (bar {ph_bar:.1e}), residuals {e_r:.2e} s, columns max {err.max():.2e} "
          f"({params[int(np.argmax(err))]}), WaveX/DMWaveX columns max {err[wx].max():.2e} (bar {bar:.2e})")
    assert e_d <= 1e-9 and e_tz <= 1e-9
    assert all(v <= 1e-9 for v in e_c.values()), e_c
    assert e_ph <= ph_bar and e_phz <= ph_bar
    assert e_r <= 1e-9
    bad = {params[k]: err[k] for k in np.where(err > 1e-9)[0]}
    assert not bad, bad
    bad = {params[k]: err[k] for k in wx if err[k] > bar}
    assert not bad, (bad, bar)
    assert np.all(M[refM == 0.0] == 0.0)  # zeros exact


def _check_fit(f, meta, key, etol):
    worst = 0.0
    for p in meta[key + "_params"]:
        s = meta[key + "_errors"][p]
        d = float((LD(f.model[p].value) - ref_value(meta, key + "_params", p)) / LD(s))
        worst = max(worst, abs(d))
        assert abs(f.model[p].uncertainty / s - 1) < etol, (p, f.model[p].uncertainty / s - 1)
    return worst


@pytest.mark.gpu
def test_gpu_wls_fit():
    from pint_amd import Residuals, WLSFitter
    model, toas, z, meta = load("wx_wls")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "wls", 1e-6)
    bar = chi2_bar("wx_wls", "fit", pre)
    print(f"wx_wls: WLS worst {worst:.2e} sigma, chi2 rel {c2 / meta['wls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["wls_chi2"] - 1) < bar


@pytest.mark.gpu
def test_gpu_gls_fit():
    from pint_amd import GLSFitter
    model, toas, z, meta = load("wx_gls")
    f = GLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "gls", 1e-5)
    bar = chi2_bar("wx_gls", "fit", rms_ps(f.resids.time_resids, z["gls_post_resid"]))
    print(f"wx_gls: GLS worst {worst:.2e} sigma, chi2 rel {c2 / meta['gls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["gls_chi2"] - 1) < bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_downhill(name):
    from pint_amd import DownhillGLSFitter, DownhillWLSFitter, Residuals
    from pint_amd.fitter import MaxiterReached, StepProblem
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (DownhillWLSFitter if name == "wx_wls" else DownhillGLSFitter)(toas, model)
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


@pytest.mark.gpu
def test_gpu_grid_wxsin_f1():
    """The reference's 5x5 (WXSIN_0001, F1) grid_chisq around the one-step fit, at
    golden_util.chi2_bar's rule for wx_wls's "fit" spread; the same argmin.  WXSIN_0001's table
    slot is a grid variable (pint_set_grid), so the full evaluation and k_wavex run per point."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    model, toas, z, meta = load("wx_wls")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    f.fit_toas(maxiter=1)
    g0 = z["grid_WXSIN_0001_hi"].astype(LD) + z["grid_WXSIN_0001_lo"]
    g1 = z["grid_F1_hi"].astype(LD) + z["grid_F1_lo"]
    c2, _ = grid_chisq(f, ("WXSIN_0001", "F1"), (g0, g1))
    ref = z["grid_chi2"]
    bar = chi2_bar("wx_wls", "fit", pre)
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"wx_wls: (WXSIN_0001, F1) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}")
    assert c2.shape == ref.shape == (5, 5)
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)


@pytest.mark.gpu
def test_gpu_spin_grid_bit_identical():
    """A 3x3 (F0, F1) grid on wx_wls with the shared-head evaluation on and off: the same bits
    (k_wavex and k_glitch run per point after k_eval_spin, on the same delay and phase).  The
    shared head was used (PINT_QUERY_NSPINEVAL).  The centre point is the model itself: its WaveX
    columns equal those of a plain evaluation."""
    from pint_amd.engine import Session, build_layout, pack_table
    model, toas, z, meta = load("wx_wls")

    def run(spin):
        s = Session()
        s.set_spin_eval(spin)
        s.set_efuse(False)
        lay = s.add(build_layout(model, toas))
        base = pack_table(lay, model)
        g0 = LD(model.F0.value) + np.linspace(-2, 2, 3) * LD(1e-11)
        g1 = LD(model.F1.value) + np.linspace(-2, 2, 3) * LD(1e-19)
        s.set_grid(lay, base, [("F0", g0, 3, 3), ("F1", g1, 1, 3)], 9)
        s.eval(want_M=True)
        took = s.n_spin_eval()
        out = [np.array(x, copy=True) for x in s.read_eval()] + [np.array(s.read_designmatrix(), copy=True)]
        s.fit_step(0)
        dp, er, _, cl = s.read_step()
        out += [np.array(x, copy=True) for x in dp] + [np.array(cl, copy=True)]
        s.close()
        return lay, out, took

    lay, a, took_a = run(True)
    _, b, took_b = run(False)
    assert took_a == 1 and took_b == 0
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[4].shape == (9, toas.ntoas, len(lay.columns))
    M, params, _ = model.designmatrix(toas)
    for j, p in _wx_cols(lay.columns):
        ref = M[:, list(params).index(p)]
        assert np.max(np.abs(ref)) > 0
        assert np.max(np.abs(a[4][4][:, j] - ref)) <= 1e-12 * np.max(np.abs(ref)), p


def _eval_all(items):
    """Delay, phase, spin frequency, design matrix and residuals of every (model, toas) in one
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
                                                       np.array(pr[k], copy=True), float(c2[k])]
           for k in range(len(items))]
    s.close()
    return out


@pytest.mark.gpu
def test_gpu_mixed_batch():
    """wx_wls, wx_gls, gl_wls and pta_iso in one batch (k_wavex's per-instance early return, the
    instances with and without either component side by side, k_glitch after it) against each
    alone: the same bits in every evaluation output, design matrix and residual."""
    import golden_util
    import test_glitch
    items = [load("wx_wls")[:2], load("wx_gls")[:2], test_glitch.load("gl_wls")[:2], golden_util.load("pta_iso")[:2]]
    mixed = _eval_all(items)
    for k, it in enumerate(items):
        (alone,) = _eval_all([it])
        for x, y in zip(mixed[k], alone):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_compact_and_full_layouts():
    """wx_gls's GLS step on the generated-Fourier compact path, the stored-basis compact path and
    the full layout: the same normal equations to rounding (test_glitch's bars for the same
    comparison), so k_wavex's columns stand where the compact layout (ColRun.dcol0) and the full
    one expect them."""
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    model, toas = load("wx_gls")[:2]
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


@pytest.mark.gpu
def test_gpu_frozen_amplitudes_delay():
    """wx_wls with every amplitude frozen against the free case: a frozen amplitude still delays
    (the same delay, phase and residuals, bit for bit) and there is no WaveX column."""
    from pint_amd import Residuals
    from pint_amd.engine import evaluate_delay_phase
    model, toas, z, meta = load("wx_wls")
    frozen = copy.deepcopy(model)
    for p in frozen.params:
        if p.startswith(("WXSIN_", "WXCOS_")):
            frozen[p].frozen = True
    a, b = evaluate_delay_phase(model, toas), evaluate_delay_phase(frozen, toas)
    for k in ("delay", "phase_hi", "phase_lo"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["tzr_delay"] == b["tzr_delay"]
    np.testing.assert_array_equal(Residuals(toas, model).time_resids, Residuals(toas, frozen).time_resids)
    assert np.max(np.abs(a["delay"] - z["delay_total"])) <= 1e-9
    M, params, _ = frozen.designmatrix(toas)
    assert not _wx_cols(params) and list(params) == [p for p in meta["dm_params"] if "WX" not in p]
    full = model.designmatrix(toas)[0]
    keep = [j for j, p in enumerate(meta["dm_params"]) if "WX" not in p]
    np.testing.assert_array_equal(M, full[:, keep])
