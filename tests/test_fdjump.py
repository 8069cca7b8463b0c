"""The FDJump and FDJumpDM components (fdjump.py, dispersion_model.py:805-884) on the device path,
against fixtures captured from the reference (scripts/refgen/gen_fdjump.py):

* fdj_wls : WLS, an isolated pulsar timed by three systems (-fe P / L / S, 8 channels each, so y^p
            varies within a system) and two backends: FD1JUMP and FD2JUMP free on L, FD1JUMP free
            on S (the index-1 lines in the tempo2 spelling FDJUMP1), a frozen non-zero FD3JUMP on
            -be B2, an FD1JUMP on an MJD range that holds the TZR TOA and overlaps the others, a
            free FDJUMPDM on P; no FDJUMPLOG line; 400 TOAs: two row blocks, the second partial,
            the TZR row in it;
* fdj_lin : the same par with the other FDJUMPLOG value, 200 TOAs;
* fdj_gls : GLS, the bench's per-pulsar shape (ELL1, DMX, red noise) with FD1JUMP / FD2JUMP free on
            one band, FDJUMPDM free on another, a frozen CM, a DMWaveX harmonic and a glitch, so
            that k_wavex, k_fdjump and k_glitch run in order; 1000 TOAs.

Bars.  Delays (total, TZR, the two components'), absolute phase (as time: x F0, plus 8 ulps of
the reference's longdouble phase) and residuals: 1 ns.  FDJump / FDJumpDM columns: the largest
absolute error over the column's largest magnitude (absolute, because y passes through 0 near
1 GHz), at most COL_BAR; every other column the project's 1e-9.  Fits 1e-3 sigma; chi2 by
golden_util.chi2_bar's rule on fdj_fit_spread.json; Downhill by its "downhill" spread.
"""
import copy
import hashlib
import json
import os
import re
import warnings

import numpy as np
import pytest

from golden_util import GOLDEN, ref_value, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
NAMES = ("fdj_wls", "fdj_lin", "fdj_gls")
ORDER = ("WaveX", "DMWaveX", "ChromaticCM", "CMWaveX", "FDJump", "FDJumpDM")
# FDJump / FDJumpDM columns against the reference's, max |error| / max |column|: measured on one
# MI355X 5.3e-16 (FDJump: y^p by a running product where the reference calls pow, and the chain
# factor's own rounding) and 2.7e-16 (FDJumpDM), worst over the three fixtures; the bar is 8x the
# worst case (log / pow rounding of other library builds) and never looser than 1e-12
COL_BAR = min(8 * 5.316e-16, 1e-12)
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
    return model, toas, z, meta


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "fdj_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on fdj_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def downhill_bar(name, p, floor=1e-3):
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _is_fd(p):
    return bool(re.match(r"^FD\d+JUMP\d+$", p))


def _is_fddm(p):
    return bool(re.match(r"^FDJUMPDM\d+$", p))


def _is_new(p):
    return _is_fd(p) or _is_fddm(p) or p == "FDJUMPLOG"


def _set(meta, params):
    """The reference's FDJump / FDJumpDM parameters that are set (its constructor also declares
    FD1JUMP1 ... FD20JUMP1 without a value; the host model does not carry the unset ones)."""
    return [p for p in params if _is_new(p) and (p == "FDJUMPLOG" or meta["model"]["values"][p]["value"] is not None)]


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on (the generator's check(), again on the committed files): every
    free new column has a non-zero maximum; each component's delay exceeds 100 ns on at least half
    of the rows its masks select (and is 0 on the others), so no 1 ns test passes with a term
    missing; fdj_lin's FDJump delays differ from the other FDJUMPLOG value's by more than 100 ns on
    such rows; the whitened Gram's condition number is below cm_gls's bound; the components
    stand in the order the device sums; the reference's Downhill stop is a fixed point to a
    quarter of the 1e-3 sigma bar."""
    model, toas, z, meta = load(name)
    params = meta["dm_params"]
    cols = [(j, p) for j, p in enumerate(params) if _is_fd(p) or _is_fddm(p)]
    assert len(cols) == (5 if name != "fdj_gls" else 3)
    for j, p in cols:
        assert np.max(np.abs(z["dm_M"][:, j])) > 0, p
    assert toas.ntoas + 1 <= 1001
    for key, pick in (("fdjump_delay", _is_fd), ("fdjumpdm_delay", _is_fddm)):
        sel = np.zeros(toas.ntoas, dtype=bool)
        for p in meta["fdj_params_set"]:
            if pick(p):
                sel |= z["mask_" + p].astype(bool)
        assert sel.any() and np.mean(np.abs(z[key][sel]) > 1e-7) >= 0.5
        assert np.all(z[key][~sel] == 0.0)
        np.testing.assert_array_equal(z[key], z["delay_" + {"fdjump_delay": "fdjump_delay",
                                                            "fdjumpdm_delay": "fdjump_dm_delay"}[key]])
    order = [c for c in meta["delay_components"] if c in ORDER]
    assert order == [c for c in ORDER if c in order] and order[-2:] == ["FDJump", "FDJumpDM"]
    assert meta["model"]["components"][0] == "AbsPhase"
    assert meta["fdj_gram_cond"] < 1e12
    assert meta["down_converged"] and meta["down_status"] == "converged"
    if name == "fdj_lin":
        assert meta["fdjumplog"] != load("fdj_wls")[3]["fdjumplog"] and meta["log_vs_lin_over_100ns"] >= 0.5
        assert toas.ntoas == 200
    else:
        assert meta["down_fixed_point"]["sigma"] < 2.5e-4
    if name == "fdj_wls":
        assert 256 < toas.ntoas + 1 < 512
        assert "FDJUMPLOG" not in open(os.path.join(GOLDEN, name + ".par")).read()
        assert meta["tzr_selected_by"] == ["FD1JUMP3"]
        both = z["mask_FD1JUMP3"].astype(bool) & (z["mask_FD1JUMP1"].astype(bool) | z["mask_FD1JUMP2"].astype(bool))
        assert both.any()  # the overlap
        for fe, (lo, hi) in {"P": (400, 480), "L": (1150, 1750), "S": (1700, 2400)}.items():
            f = z["freq_mhz"][np.array(meta["flag_columns"]["fe"]) == fe]
            assert len(set(f)) == 8 and f.min() == lo and f.max() == hi
        assert model.FD3JUMP1.frozen and model.FD3JUMP1.value != 0 and model.FD3JUMP1.key == "-be"
    if name == "fdj_gls":
        assert all(c in meta["delay_components"] for c in ("DMWaveX", "ChromaticCM")) and "Glitch" in model.components
        assert len(set(np.round(z["freq_mhz"] / 400))) >= 4
    key = "gls" if name == "fdj_gls" else "wls"
    assert all(np.isfinite(v) and v > 0 for v in meta[key + "_errors"].values())


def test_parse_both_spellings():
    """FD{p}JUMP and tempo2's FDJUMP{p} are the same parameter; names, order, keys and FDJUMPLOG's
    value as the reference has them (fdj_wls.json: its parameter list without the unset
    FD{p}JUMP1 its constructor declares)."""
    from pint_amd import get_model
    model, toas, z, meta = load("fdj_wls")
    par = open(os.path.join(GOLDEN, "fdj_wls.par")).read()
    assert "FDJUMP1 -fe L" in par and "FD2JUMP -fe L" in par
    assert [p for p in model.params if _is_new(p)] == _set(meta, meta["model"]["params"]) == meta["fdj_params_set"]
    assert model.FDJUMPLOG.value is meta["fdjumplog"] is True and model.FDJUMPLOG.frozen == meta["fdjumplog_frozen"]
    other = get_model(re.sub(r"FDJUMP(\d) ", r"FD\1JUMP ", par))
    for m in (model, other):
        for p in meta["fdj_params_set"][1:]:
            ref = meta["model"]["values"][p]
            assert m[p].kind == "mask" and m[p].key == ref["key"] and m[p].frozen == ref["frozen"], p
            assert [float(x) if ref["key"] == "mjd" else x for x in m[p].key_value] == \
                [float(x) if ref["key"] == "mjd" else x for x in ref["key_value"]]
            assert LD(m[p].value) == ref_value({"v": {p: ref["value"]}}, "v", p)
            assert m[p].units == ("s" if _is_fd(p) else "pc / cm3")
    assert [p for p in other.params if _is_new(p)] == meta["fdj_params_set"]
    assert model.get_fd_index("FD12JUMP3") == 12 and model.fdjump_params() == meta["fdj_params_set"][1:6]
    assert model.fdjumpdm_params() == ["FDJUMPDM1"]
    with pytest.raises(ValueError):
        model.get_fd_index("JUMP1")
    lin = load("fdj_lin")
    assert lin[0].FDJUMPLOG.value is lin[3]["fdjumplog"] is False
    # FDJUMPLOG alone brings the component; without any line there is none
    assert "FDJump" in get_model(BASE + "FDJUMPLOG N\n").components
    assert "FDJump" not in get_model(BASE).components and "FDJumpDM" not in get_model(BASE).components


@pytest.mark.parametrize("name", NAMES)
def test_params_components_and_masks(name):
    """params, free_params, component order, mask_params and find_empty_masks against the record;
    a free parameter that selects no TOA is reported as a JUMP is."""
    from pint_amd import get_model
    model, toas, z, meta = load(name)
    assert model.free_params == meta["model"]["free_params"]
    assert [p for p in model.params if _is_new(p)] == _set(meta, meta["model"]["params"])
    keep = [c for c in meta["model"]["components"] if c in ORDER]
    assert [c for c in model.components if c in ORDER] != [] and \
        [c for c in model.component_names if c in ORDER] == keep
    for p in meta["fdj_params_set"][1:]:
        np.testing.assert_array_equal(np.sort(toas.select_mask(model[p].key, model[p].key_value)),
                                      np.where(z["mask_" + p])[0])
    assert model.find_empty_masks(toas) == []
    m = get_model(open(os.path.join(GOLDEN, name + ".par")).read() + "FD4JUMP -fe nobody 1e-6 1\nFDJUMPDM -fe nobody 1e-6 1\n"
                  "JUMP -fe nobody 1e-6 1\n")
    empty = m.find_empty_masks(toas)
    assert len(empty) == 3 and sum(map(_is_fd, empty)) == 1 and sum(map(_is_fddm, empty)) == 1
    m.find_empty_masks(toas, freeze=True)
    assert all(m[p].frozen for p in empty) and m.free_params == model.free_params


@pytest.mark.parametrize("name", ("fdj_wls", "fdj_gls"))
def test_parfile_round_trip(name):
    """The post-fit model (the reference's fitted values and uncertainties) writes FDJUMPLOG, FDpJUMP
    and FDJUMPDM lines equal to the reference's as_parfile text (format pint: always FDpJUMP), in
    its order; reading them back gives the same values, fit flags and uncertainties."""
    from pint_amd import get_model
    model, toas, z, meta = load(name)
    key = "wls" if name == "fdj_wls" else "gls"
    for p, s in meta[key + "_errors"].items():
        v = ref_value(meta, key + "_params", p)
        model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
        model[p].uncertainty = s
    new = lambda l: bool(l.split()) and bool(re.match(r"^(FD\d+JUMP|FDJUMPDM|FDJUMPLOG)$", l.split()[0]))  # noqa: E731
    ref = [l for l in meta[key + "_parfile"].splitlines() if new(l)]
    got = [l for l in model.as_parfile().splitlines() if new(l)]
    assert len(ref) == (7 if name == "fdj_wls" else 4) and got == ref
    assert not any(l.startswith("FDJUMP") and l[6].isdigit() for l in got)
    back = get_model(model.as_parfile())
    assert [p for p in back.params if _is_new(p)] == [p for p in model.params if _is_new(p)]
    for p in model.params:
        if _is_new(p):
            a, b = model[p], back[p]
            assert a.value == b.value and a.frozen == b.frozen and a.key == b.key, p
            assert [str(float(x)) if a.key == "mjd" else x for x in a.key_value] == list(b.key_value) or a.key != "mjd"
            assert (a.uncertainty_value or 0.0) == (b.uncertainty_value or 0.0), p


BASE = "PSR X\nRAJ 10:12:33.4 1\nDECJ 53:07:02.5 1\nF0 218.8 1\nF1 -4e-16 1\nPEPOCH 55000\nDM 9.02 1\nEPHEM builtin\nUNITS TDB\n"


@pytest.mark.parametrize("case", ("index_21_pint", "index_21_tempo2", "index_0", "index_20", "mixed_spellings",
                                  "mixed_spellings_reversed"))
def test_rejected_forms(case):
    """What the reference does with an FD index outside 1..20 (the rewritten line is reported as
    unrecognised and ignored), with index 20 (accepted), and with both spellings of one index in
    one file (the lines of the spelling that appears later replace the other's): the record in
    fdj_wls.json "forms", reproduced."""
    from pint_amd import get_model
    rec = load("fdj_wls")[3]["forms"][case]
    par = open(os.path.join(GOLDEN, "fdj_wls.par")).read()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = get_model(par + rec["lines"])
    assert rec["result"] == "ok"
    assert sorted({str(x.message) for x in w if "parfile line" in str(x.message)}) == rec["warnings"]
    assert [p for p in m.params if _is_fd(p) or _is_fddm(p)] == rec["order"]
    for p, (key, kv, value, frozen) in rec["params"].items():
        assert m[p].key == key and m[p].frozen == frozen, p
        assert [float(x) if key == "mjd" else x for x in m[p].key_value] == [float(x) if key == "mjd" else x for x in kv]
        if p not in ("FD1JUMP1", "FD2JUMP1", "FD1JUMP2", "FD1JUMP3", "FDJUMPDM1"):  # (the record has the true par's values)
            assert float(m[p].value) == value, p
    assert m.FDJUMPLOG.value == rec["fdjumplog"]


def test_too_many_parameters():
    """64 parameters per family build; one more raises naming PINT_MAX_FDJUMP."""
    from pint_amd import _lib as L
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    toas = load("fdj_wls")[1]
    assert (L.COL_FDJUMP, L.COL_FDJUMPDM, L.MAX_FDJUMP, L.FDJUMP_MAX_INDEX) == (19, 20, 64, 20)
    for stem in ("FD{}JUMP", "FDJUMPDM"):
        lines = [f"{stem.format(1 + k % 20)} mjd {54500 + 10 * k} {54520 + 10 * k} 1e-7\n" for k in range(65)]
        lay = build_layout(get_model(BASE + "".join(lines[:64])), toas)
        assert lay.fdjump[1 if stem != "FDJUMPDM" else 6] == 64
        with pytest.raises(NotImplementedError, match="PINT_MAX_FDJUMP"):
            build_layout(get_model(BASE + "".join(lines)), toas)


@pytest.mark.parametrize("name", NAMES)
def test_layout_and_masks(name):
    """Table slots (dd pairs, FDJump's block ordered by FD index), column kinds and indices, the
    descriptor, and the n + 1 row masks: bit k of row r says parameter k selects it, the last entry
    the TZR TOA (toas.select_mask(..., tzr=True)), overlapping masks as several bits."""
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout
    model, toas, z, meta = load(name)
    lay = build_layout(model, toas)
    assert lay.columns == meta["dm_params"]
    o_fdj, nfdj, fdidx, use_log, mask, o_dm, ndm, dmmask = lay.fdjump
    n = toas.ntoas
    fds = sorted(model.fdjump_params(), key=model.get_fd_index)
    if name != "fdj_gls":
        assert fds == ["FD1JUMP1", "FD1JUMP2", "FD1JUMP3", "FD2JUMP1", "FD3JUMP1"]
    assert nfdj == len(fds) and list(fdidx) == [model.get_fd_index(p) for p in fds] and fdidx.dtype == np.int32
    assert list(fdidx) == sorted(fdidx) and use_log == (1 if meta["fdjumplog"] else 0)
    assert ndm == 1 and mask.shape == dmmask.shape == (n + 1,) and mask.dtype == dmmask.dtype == np.uint64
    assert 0 <= o_fdj and o_fdj + 2 * nfdj <= lay.tstride and 0 <= o_dm and o_dm + 2 * ndm <= lay.tstride
    for group, o, kind, mk in ((fds, o_fdj, L.COL_FDJUMP, mask), (["FDJUMPDM1"], o_dm, L.COL_FDJUMPDM, dmmask)):
        for k, p in enumerate(group):
            assert lay.offsets[p] == o + 2 * k
            np.testing.assert_array_equal((mk[:n] >> np.uint64(k)) & np.uint64(1), z["mask_" + p])
            tz = len(toas.select_mask(model[p].key, model[p].key_value, tzr=True)) > 0
            assert bool((mk[n] >> np.uint64(k)) & np.uint64(1)) == tz == (p in meta.get("tzr_selected_by", ["FD1JUMP3"])
                                                                        and name != "fdj_gls")
            if p in lay.columns:
                c = lay.columns.index(p)
                assert (lay.spec.col_kind[c], lay.spec.col_index[c], lay.spec.col_toff[c]) == (kind, k, lay.offsets[p])
            else:
                assert model[p].frozen
        assert not np.any(mk >> np.uint64(len(group)))
    if name == "fdj_wls":
        assert np.any((mask[:n] & np.uint64(4)).astype(bool) & (mask[:n] & np.uint64(3)).astype(bool))  # overlap: two bits
        assert "FD3JUMP1" not in lay.columns and mask[n] == 4
    if name == "fdj_gls":
        assert lay.wavex is not None and lay.chromatic is not None and lay.spec.nglitch == 1


def test_layout_without_fdjump_is_the_parents():
    """pta_iso has neither component: its table, offsets and spec bytes hash to the values
    test_glitch.py, test_wavex.py and test_chromatic.py record, and its layout asks for no
    pint_set_fdjump call."""
    import golden_util
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout, pack_table
    model, toas, z, meta = golden_util.load("pta_iso")
    lay = build_layout(model, toas)
    assert lay.fdjump is None and lay.chromatic is None and lay.wavex is None
    assert hashlib.sha256(pack_table(lay).tobytes()).hexdigest() == \
        "d50cf50a3018718c5effddf8a65b45cb702d696e8780a3a01f413b7973bcc81f"
    assert hashlib.sha256(repr(list(lay.offsets.items())).encode()).hexdigest() == \
        "ca1ee53fe23016db57b8fdb8e518568678f5375e3dd94c52cb4720b0294bdfe8"
    b = bytes(lay.spec)
    o = L.SpecT.o_GLITCH.offset
    assert hashlib.sha256(b[:o] + bytes(4) + b[o + 20:]).hexdigest() == \
        "d993d9149f99392cd1bc13abec1128320ac9b59fef1cc91d1acf4ae1c21924ee"


def test_wideband_refused():
    """A fitter given wideband TOAs and a model with either component raises, naming it."""
    import golden_util
    from pint_amd import GLSFitter, WLSFitter, WidebandTOAFitter, get_model
    toas = golden_util.load("wb_dd")[1]
    assert toas.is_wideband()
    for par, comp in ((BASE + "FD1JUMP -fe L 1e-6 1\n", "FDJump"), (BASE + "FDJUMPDM -fe L 1e-4 1\n", "FDJumpDM")):
        m = get_model(par)
        assert comp in m.components
        for cls in (WLSFitter, GLSFitter, WidebandTOAFitter):
            with pytest.raises(NotImplementedError, match=comp + r"\b"):
                cls(toas, m)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
def _zeroed(model, pick):
    m = copy.deepcopy(model)
    for p in m.params:
        if pick(p):
            m[p].value = 0.0
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_delay_phase_residuals_columns(name):
    """Measured on one MI355X (fdj_wls / fdj_lin / fdj_gls): total delay 5.7e-14 / 5.7e-14 / 7.1e-13 s,
    TZR delay 1.1e-13 s, component delays (as differences of totals) 2.8e-14 s, absolute phase
    9.3e-10 / 9.3e-10 / 7.5e-9 cycles (TZR row 0 / 0 / 3.9e-11), residuals 4.4e-12 / 4.8e-12 /
    2.0e-11 s; FDJump columns 5.3e-16 / 2.5e-16 / 4.2e-16 and FDJumpDM columns 2.7e-16 / 1.3e-16 /
    1.7e-16 of the column's maximum (bar COL_BAR = 4.3e-15); every other column <= 1.3e-11."""
    from pint_amd import Residuals
    from pint_amd.engine import evaluate_delay_phase
    model, toas, z, meta = load(name)
    model.free_params = meta["model"]["free_params"]
    n = toas.ntoas
    dp = evaluate_delay_phase(model, toas)
    e_d = np.max(np.abs(dp["delay"] - z["delay_total"]))
    e_tz = abs(dp["tzr_delay"] - z["tzr_delay"][0])
    # each component's delay: the total less the total with that component's values zeroed
    e_c = {}
    for key, pick in (("fdjump_delay", _is_fd), ("fdjumpdm_delay", _is_fddm)):
        d0 = evaluate_delay_phase(_zeroed(model, pick), toas)
        assert np.max(np.abs(dp["delay"] - d0["delay"])) > 1e-7
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
    M, params, units = model.designmatrix(toas)
    assert list(params) == meta["dm_params"]
    refM = z["dm_M"]
    scale = np.max(np.abs(refM), axis=0)
    scale[scale == 0] = 1
    err = np.max(np.abs(M - refM), axis=0) / scale
    fd = [j for j, p in enumerate(params) if _is_fd(p)]
    fdm = [j for j, p in enumerate(params) if _is_fddm(p)]
    assert fd and fdm and all(units[j] == "" for j in fd + fdm)  # (labelled as JUMP columns are)
    print(f"{name}: delay {e_d:.2e} s, TZR delay {e_tz:.2e} s, components {e_c}, phase {e_ph:.2e} / TZR {e_phz:.2e} "
          f"cycles (bar {ph_bar:.1e}), residuals {e_r:.2e} s, columns max {err.max():.2e} "
          f"({params[int(np.argmax(err))]}), FDJump columns max {err[fd].max():.3e}, FDJumpDM columns max "
          f"{err[fdm].max():.3e} (bar {COL_BAR:.2e})")
    assert e_d <= 1e-9 and e_tz <= 1e-9
    assert all(v <= 1e-9 for v in e_c.values()), e_c
    assert e_ph <= ph_bar and e_phz <= ph_bar
    assert e_r <= 1e-9
    bad = {params[k]: err[k] for k in np.where(err > 1e-9)[0]}
    assert not bad, bad
    assert COL_BAR <= 1e-12
    bad = {params[k]: err[k] for k in fd + fdm if err[k] > COL_BAR}
    assert not bad, (bad, COL_BAR)
    for j in fd + fdm:  # exactly 0 on the rows the parameter's mask does not select
        assert np.all(M[z["mask_" + params[j]] == 0, j] == 0.0) and np.all(M[z["mask_" + params[j]] == 1, j] != 0.0)
    assert np.all(M[refM == 0.0] == 0.0)


def _check_fit(f, meta, key, etol):
    worst = 0.0
    for p in meta[key + "_params"]:
        s = meta[key + "_errors"][p]
        d = float((LD(f.model[p].value) - ref_value(meta, key + "_params", p)) / LD(s))
        worst = max(worst, abs(d))
        assert abs(f.model[p].uncertainty / s - 1) < etol, (p, f.model[p].uncertainty / s - 1)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("fdj_wls", "fdj_lin"))
def test_gpu_wls_fit(name):
    from pint_amd import Residuals, WLSFitter
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "wls", 1e-6)
    bar = chi2_bar("fdj_wls", "fit", pre)  # (fdj_lin: the same model shape and errors at half the TOAs)
    print(f"{name}: WLS worst {worst:.2e} sigma, chi2 rel {c2 / meta['wls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["wls_chi2"] - 1) < bar


@pytest.mark.gpu
def test_gpu_gls_fit():
    from pint_amd import GLSFitter
    model, toas, z, meta = load("fdj_gls")
    f = GLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "gls", 1e-5)
    bar = chi2_bar("fdj_gls", "fit", rms_ps(f.resids.time_resids, z["gls_post_resid"]))
    print(f"fdj_gls: GLS worst {worst:.2e} sigma, chi2 rel {c2 / meta['gls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["gls_chi2"] - 1) < bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("fdj_wls", "fdj_gls"))
def test_gpu_downhill(name):
    from pint_amd import DownhillGLSFitter, DownhillWLSFitter, Residuals
    from pint_amd.fitter import MaxiterReached, StepProblem
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (DownhillWLSFitter if name == "fdj_wls" else DownhillGLSFitter)(toas, model)
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
        assert abs(f.model[p].uncertainty / meta["down_errors"][p] - 1) < (1e-6 if name == "fdj_wls" else 1e-5), p


@pytest.mark.gpu
def test_gpu_grid_fd1jump_dm():
    """The reference's 5x5 (FD1JUMP1, DM) grid_chisq around the one-step fit, at golden_util.chi2_bar's
    rule for fdj_wls's "fit" spread; the same argmin.  FD1JUMP1's table slot is a grid variable
    (pint_set_grid), so the full evaluation and k_fdjump run per point."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    model, toas, z, meta = load("fdj_wls")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    f.fit_toas(maxiter=1)
    g0 = z["grid_FD1JUMP1_hi"].astype(LD) + z["grid_FD1JUMP1_lo"]
    g1 = z["grid_DM_hi"].astype(LD) + z["grid_DM_lo"]
    c2, _ = grid_chisq(f, ("FD1JUMP1", "DM"), (g0, g1))
    ref = z["grid_chi2"]
    bar = chi2_bar("fdj_wls", "fit", pre)
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"fdj_wls: (FD1JUMP1, DM) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}")
    assert c2.shape == ref.shape == (5, 5)
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)


@pytest.mark.gpu
def test_gpu_spin_grid():
    """A 3x3 (F0, F1) grid_chisq on fdj_wls: every point's chi2 equals that of a single WLS fit
    with F0 and F1 held at the point's values, within 1e-9 relative, and the grid's first
    evaluation took the shared head (k_eval_head / k_eval_spin, PINT_QUERY_NSPINEVAL): k_fdjump
    follows that route per point."""
    from pint_amd import WLSFitter
    from pint_amd import gridutils
    model, toas, z, meta = load("fdj_wls")
    f = WLSFitter(toas, model)
    g0 = LD(model.F0.value) + np.linspace(-2, 2, 3) * LD(2e-12)
    g1 = LD(model.F1.value) + np.linspace(-2, 2, 3) * LD(2e-19)
    c2, _ = gridutils.grid_chisq(f, ("F0", "F1"), (g0, g1))
    took = sum(s.n_spin_eval() for s, _ in gridutils._GRID["cur"][1])
    assert took >= 1 and c2.shape == (3, 3)
    worst = 0.0
    for i in range(3):
        for j in range(3):
            m = copy.deepcopy(model)
            m.F0.value, m.F1.value = g0[i], g1[j]
            m.F0.frozen = m.F1.frozen = True
            one = WLSFitter(toas, m).fit_toas(maxiter=1)
            worst = max(worst, abs(c2[j, i] / one - 1))  # (meshgrid's "xy" shape: the second axis first)
    print(f"fdj_wls: (F0, F1) grid against single fits, max rel {worst:.2e}; chi2 {c2.min():.3f} .. {c2.max():.3f}")
    assert c2.max() > 1.01 * c2.min()
    assert worst <= 1e-9


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


@pytest.mark.gpu
def test_gpu_mixed_batch():
    """fdj_gls and pta_iso in one Session against each alone: pta_iso (neither component: the
    pass's block-uniform early exit) keeps its evaluation outputs, design matrix, residuals and
    GLS fit step bit for bit, and fdj_gls's results are the same too."""
    import golden_util
    from pint_amd.engine import Session
    items = [load("fdj_gls")[:2], golden_util.load("pta_iso")[:2]]
    mixed = _step_all(items, Session.FIT)
    for k, it in enumerate(items):
        (alone,) = _step_all([it], Session.FIT)
        for x, y in zip(mixed[k], alone):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_compact_and_full_layouts():
    """fdj_gls's GLS step on the generated-Fourier compact path, the stored-basis compact path and
    the full layout: the same normal equations to rounding (test_wavex's and test_chromatic's
    bars for the same comparison), so the FDJump / FDJumpDM columns stand where the compact layout
    (ColRun.dcol0) and the full one expect them."""
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    model, toas = load("fdj_gls")[:2]
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
def test_gpu_lazy_pipelined():
    """fdj_gls and pta_iso in a lazy, pipelined session (the bench's step shape, two steps in
    flight: test_pldm_noise_resids_lazy_pipelined's) against the synchronous session: the step,
    its errors and the noise realisations bit for bit."""
    import golden_util
    from pint_amd.engine import Session, build_layout, pack_table
    items = [load("fdj_gls")[:2], golden_util.load("pta_iso")[:2]]

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
    """fdj_gls and pta_iso: a fit step captured into a HIP graph and replayed (the shape of
    test_graph_replay_matches_direct) gives the step, errors, covariance and chi2 of the directly
    enqueued step bit for bit -- k_fdjump is captured with the evaluation's other launches."""
    import golden_util
    from pint_amd.engine import Session, build_layout, pack_table
    items = [load("fdj_gls")[:2], golden_util.load("pta_iso")[:2]]
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
def test_gpu_added_delay_bound():
    """The phase is moved to the new total delay with the first- and second-order terms, which
    holds 1e-12 cycle for |d| <= 1 s (PINT_MAX_ADDED_DELAY): with FD1JUMP1 = 10 s the FDJump delay
    on the L rows is 1.4 to 5.6 s and the checked evaluation fails with PINT_E_PARAM, naming the
    bound; the same with an FDJUMPDM of 1e5 pc cm^-3 (2e3 s at 440 MHz).  An error return, not a
    fault."""
    from pint_amd import _lib as L
    from pint_amd.engine import evaluate_delay_phase
    for p, v in (("FD1JUMP1", 10.0), ("FDJUMPDM1", 1e5)):
        model, toas, z, meta = load("fdj_wls")
        model[p].value = v
        with pytest.raises(L.PintError, match="PINT_MAX_ADDED_DELAY") as ei:
            evaluate_delay_phase(model, toas)
        assert ei.value.code == L.PINT_E_PARAM


@pytest.mark.gpu
def test_gpu_set_fdjump_bad_arguments():
    """pint_set_fdjump validates counts, slots, FD indices, null pointers and mask bits: each bad call
    returns PINT_E_INVALID and leaves a message in pint_last_error; the good call then succeeds."""
    import ctypes as C
    from pint_amd import _lib as L
    from pint_amd.engine import Session, build_layout
    model, toas, z, meta = load("fdj_lin")
    s = Session()
    lay = s.add(build_layout(model, toas))
    o_fdj, nfdj, fdidx, use_log, mask, o_dm, ndm, dmmask = lay.fdjump
    n, pid = toas.ntoas, lay.psr_id
    i32 = lambda a: L.ptr(np.ascontiguousarray(a, dtype=np.int32), C.c_int32)  # noqa: E731
    u64 = lambda a: L.ptr(np.ascontiguousarray(a, dtype=np.uint64), C.c_uint64)  # noqa: E731
    high = mask.copy()
    high[n] |= np.uint64(1) << np.uint64(nfdj)
    bad = [
        (pid + 7, o_fdj, nfdj, i32(fdidx), use_log, u64(mask), o_dm, ndm, u64(dmmask)),          # pulsar id
        (pid, o_fdj, 65, i32(np.ones(65)), use_log, u64(mask), o_dm, ndm, u64(dmmask)),          # count
        (pid, o_fdj, -1, i32(fdidx), use_log, u64(mask), o_dm, ndm, u64(dmmask)),
        (pid, lay.tstride - 2, nfdj, i32(fdidx), use_log, u64(mask), o_dm, ndm, u64(dmmask)),    # block past the table
        (pid, -1, nfdj, i32(fdidx), use_log, u64(mask), o_dm, ndm, u64(dmmask)),
        (pid, o_fdj, nfdj, None, use_log, u64(mask), o_dm, ndm, u64(dmmask)),                    # null pointers
        (pid, o_fdj, nfdj, i32(fdidx), use_log, None, o_dm, ndm, u64(dmmask)),
        (pid, o_fdj, nfdj, i32(fdidx), use_log, u64(mask), o_dm, ndm, None),
        (pid, o_fdj, nfdj, i32([1, 1, 1, 2, 21]), use_log, u64(mask), o_dm, ndm, u64(dmmask)),   # FD index
        (pid, o_fdj, nfdj, i32([0, 1, 1, 2, 3]), use_log, u64(mask), o_dm, ndm, u64(dmmask)),
        (pid, o_fdj, nfdj, i32([1, 2, 1, 2, 3]), use_log, u64(mask), o_dm, ndm, u64(dmmask)),    # not ascending
        (pid, o_fdj, nfdj, i32(fdidx), use_log, u64(high), o_dm, ndm, u64(dmmask)),              # a bit beyond the count
        (pid, o_fdj, nfdj, i32(fdidx), use_log, u64(mask), lay.tstride, ndm, u64(dmmask)),
        (pid, o_fdj, nfdj, i32(fdidx), use_log, u64(mask), o_dm, 65, u64(dmmask)),
    ]
    assert nfdj == 5
    for args in bad:
        rc = s.L.pint_set_fdjump(s.ctx, *args)
        assert rc == L.PINT_E_INVALID, args
        msg = s.L.pint_last_error(s.ctx).decode()
        assert msg and ("FDJump" in msg or "pulsar" in msg), msg
    assert s.L.pint_set_fdjump(None, *bad[0][0:]) == L.PINT_E_INVALID
    assert s.L.pint_set_fdjump(s.ctx, pid, o_fdj, nfdj, i32(fdidx), use_log, u64(mask), o_dm, ndm, u64(dmmask)) == 0
    s.close()
