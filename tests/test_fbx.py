"""The orbital-frequency orbit FB0 ... FBn (binary_orbits.py:158-239 OrbitFBX) of ELL1, ELL1H, DD and
BT on the device path, against fixtures captured from the reference (scripts/refgen/gen_fbx.py):

* fbx_ell1_wls, fbx_ell1h_wls, fbx_dd_wls, fbx_bt_wls : WLS, an isolated-pulsar base with the binary
            block, FB0 ... FB2 and every other binary parameter of the block free, 300 TOAs (a partial
            second 256-thread block); fbx_ell1_wls also holds the "forms" and a 3x3 (FB0, FB1) grid;
* fbx_ell1_gls, fbx_dd_gls : GLS, the bench's per-pulsar shape (DMX, red noise) with FB0 ... FB3,
            1000 TOAs.

The T0 column of DD and BT is the derivative itself: the reference's is identically zero with this
orbit, and the fixtures were captured with its OrbitFBX corrected in the generator's process
("reference_patches"; the as-is column is kept as asis_col_T0).

Bars.  Delays (total, TZR) and residuals 1 ns, binary delay 5 ps, absolute phase 1 ns x F0 plus 8 ulps
of the reference's longdouble phase; FBn and the other binary columns, the largest absolute error
over the column's largest magnitude, at most COL_BAR; every other column the project's 1e-9.  Fits
max(1e-3 sigma, 2 x the spread of fbx_fit_spread.json); chi2 and the grid by golden_util.chi2_bar's
rule on that file.
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
WLS = ("fbx_ell1_wls", "fbx_ell1h_wls", "fbx_dd_wls", "fbx_bt_wls")
GLS = ("fbx_ell1_gls", "fbx_dd_gls")
NAMES = WLS + GLS
BINARY = {"fbx_ell1_wls": "ELL1", "fbx_ell1h_wls": "ELL1H", "fbx_dd_wls": "DD", "fbx_bt_wls": "BT",
          "fbx_ell1_gls": "ELL1", "fbx_dd_gls": "DD"}
T0_MODELS = ("DD", "BT")
# binary columns (FBn among them) against the reference's, max |error| / max |column|, worst over the
# six fixtures and every free binary parameter: measured on one MI355X MEASURED_COL (the per-fixture
# figures are in test_gpu_delay_phase_residuals_columns' docstring); the bar is 8x that (other
# library builds' sincos / log rounding) and never looser than 1e-12
MEASURED_COL = 1.596e-13
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


def forms():
    return load("fbx_ell1_wls")[3]["forms"]


def _spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "fbx_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on fbx_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def fit_bar(name, kind, p, floor=1e-3):
    """max(1e-3 sigma, 2 x the reference's own spread of the fitted value under a 5 ps residual
    shift).  The file holds that spread for the Downhill result ("downhill"); a one-step fit has
    none recorded and keeps the floor."""
    if kind != "downhill":
        return floor
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _is_fb(p):
    return p.startswith("FB") and p[2:].isdigit()


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on, again on the committed files: every free column has a non-zero
    maximum; the correction is named; for DD and BT the as-is T0 column is identically zero and far
    from the reference's numerical derivative, the corrected one within 1e-4 of its maximum (BT: what
    its chain reaches, below 1e-3: BT_model leaves delayR's own derivatives out for every parameter);
    the reference's Downhill fit converged; 300 rows are a partial second block."""
    model, toas, z, meta = load(name)
    params = meta["dm_params"]
    free = meta["binary_free"]
    nfb = 3 if name in WLS else 4
    assert [p for p in free if _is_fb(p)] == [f"FB{k}" for k in range(nfb)]
    assert len(free) >= 8
    for j, p in enumerate(params):
        assert np.max(np.abs(z["dm_M"][:, j])) > 0, p
    assert set(meta["reference_patches"]) == {"OrbitFBX.d_orbits_d_T0", "OrbitFBX.d_pbprime_d_par", "OrbitFBX.orbit_params"}
    assert meta["binary"] == BINARY[name]
    if BINARY[name] in T0_MODELS:
        rec = meta["corrected"]
        assert rec["column"] == "T0" and rec["asis_max"] == 0.0 and rec["asis_num_rel_err"] == 1.0
        assert rec["num_rel_err"] < (1e-3 if BINARY[name] == "BT" else 1e-4)
        assert np.all(z["asis_col_T0"] == 0.0)
        assert np.max(np.abs(z["dm_M"][:, params.index("T0")])) > 1e-4
    else:
        assert meta["corrected"] == {} and "asis_col_T0" not in z
    assert meta["down_converged"] and meta["down_status"] == "converged"
    assert toas.ntoas == (300 if name in WLS else 1000)
    if name in WLS:
        assert 256 < toas.ntoas + 1 < 512
    # the higher terms matter: without FB1 and FB2 the orbital phase is off by more than 1e-5 orbits
    fb = [LD(meta["model"]["values"][f"FB{k}"]["value"][0]) for k in range(nfb)]
    span = LD(550 if name in WLS else 1800) * 86400
    assert abs(fb[1]) * span ** 2 / 2 > 1e-5 and abs(fb[2]) * span ** 3 / 6 > 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_params_and_values(name):
    """The host model holds the reference's set binary parameters in its order (BT's T0 keeps the
    place this project always gave it), FB0 ... FBn as long-double prefix parameters of the binary
    component with the reference's values and fit flags, and PB unset."""
    model, toas, z, meta = load(name)
    vals = meta["model"]["values"]
    assert model.binary == BINARY[name] and meta["binary_component"] == "Binary" + model.binary
    assert model.free_params == [p for p in meta["model"]["free_params"]] or BINARY[name] == "BT"
    assert sorted(model.free_params) == sorted(meta["model"]["free_params"])
    ref = [p for p in meta["model"]["params"] if (_is_fb(p) or p in ("PB", "SINI", "M2", "A1", "TASC", "T0", "GAMMA", "OMDOT"))
           and p in model]
    got = [p for p in model.params if p in ref]
    if BINARY[name] == "BT":
        ref, got = [p for p in ref if p != "T0"], [p for p in got if p != "T0"]
    assert got == ref
    assert model.PB.value is None and vals["PB"]["value"] is None
    for p in model.fb_terms():
        q = model[p]
        assert q.component == "Binary" and q.long_double and q.kind == "float"
        assert q.units == f"1 / s^{int(p[2:]) + 1}"
        hi, lo = vals[p]["value"]
        assert LD(q.value) == LD(hi) + LD(lo), p
        assert q.frozen == vals[p]["frozen"]
    assert model.fb_terms() == [f"FB{k}" for k in range(3 if name in WLS else 4)]


def test_model_without_fbn_is_unchanged():
    """A model without FBn lines has no FB0 parameter (the reference carries an unset one) and the
    spec, table and offsets it had before (test_binaries_dds_ddh_ell1k's recorded hashes)."""
    import golden_util
    from pint_amd import get_model
    from pint_amd.engine import build_layout, pack_table
    rec = forms()["no_fbn"]
    assert rec["result"] == "ok" and rec["orbit"] == "OrbitPB" and "FB0" in rec["binary_params"]
    m = get_model(rec["par"])
    assert "FB0" not in m and m.fb_terms() == [] and float(m.PB.value) == 0.3
    assert [p for p in m.free_params if m[p].component == "Binary"] == rec["free"]
    for name, table, spec in (("pta_dd", "2f7ba10d058d1747d5f6f174e6ac66a5398c60ceff3f09b6bef18d3969e8389c",
                               "53d605f8c6aa22aaf4c843679378fc779956e5144aafb438d0fea0a1ed4b5767"),
                              ("pta_ell1", "2ced18a47d0c5d9080d573c7961f2645608b2a93e2021d51a7641274dd5e38e4",
                               "1f1a82f19ad2f985e41bf10e846963a2a4c5e30d05e1b6ac460e7579d0af052c")):
        model, toas, z, meta = golden_util.load(name)
        assert "FB0" not in model
        lay = build_layout(model, toas)
        assert list(lay.spec.rsv_) == [0, 0, 0]
        assert hashlib.sha256(pack_table(lay).tobytes()).hexdigest() == table
        assert hashlib.sha256(bytes(lay.spec)).hexdigest() == spec


@pytest.mark.parametrize("case", ("no_fb0", "fb0_negative", "fb0_zero", "fb0_and_pb"))
def test_refused_forms(case):
    """The reference's ValueErrors, with its messages: some FBn set but FB0 unset, FB0 <= 0, values
    for both FB0 and PB."""
    from pint_amd import get_model
    rec = forms()[case]
    assert rec["result"] == "ValueError"
    with pytest.raises(ValueError) as ei:
        get_model(rec["par"])
    if case in ("fb0_negative", "fb0_zero"):  # (the reference prints the quantity with astropy's digits)
        assert str(ei.value).startswith("Binary frequency FB0 must be non-negative (")
        assert rec["message"].startswith("Binary frequency FB0 must be non-negative (")
    else:
        assert str(ei.value) == rec["message"]


def test_gap_alias_and_ignored_forms():
    """A gap in the indices is a ValueError with OrbitFBX's message (the reference means to raise it
    but never does, and silently drops the terms above the gap: recorded); the alias FB names FB0
    (declared by the reference, whose par reader does not honour it: recorded); PBDOT beside FB0 is
    kept, frozen or free, and plays no part; a lone FB0 is a model of its own."""
    from pint_amd import get_model
    f = forms()
    assert f["gap"]["result"] == "ok" and f["gap"]["binary_delay_equals"] == ["fb0_alone", True]
    with pytest.raises(ValueError, match="Indices must be 0 up to some number k without gaps but are"):
        get_model(f["gap"]["par"])
    assert f["alias_fb_alone"]["result"] == "ok" and f["alias_fb_alone"]["orbit"] == "OrbitPB"
    assert any("FB " in w for w in f["alias_fb_alone"]["warnings"])
    m = get_model(f["alias_fb_alone"]["par"])
    assert m.fb_terms() == ["FB0"] and m.FB0.alias == "FB" and not m.FB0.frozen
    assert LD(m.FB0.value) == LD("3.858024691358024691e-05")
    m = get_model(f["alias_fb"]["par"])
    assert m.fb_terms() == ["FB0", "FB1", "FB2"]
    m = get_model(f["fb0_alone"]["par"])
    assert m.fb_terms() == ["FB0"] and [p for p in m.free_params if m[p].component == "Binary"] == f["fb0_alone"]["free"]
    rec = f["pbdot_beside_fb0"]
    assert rec["result"] == "ok" and rec["PBDOT_column_max"] == 0.0 and rec["binary_delay_equals"] == ["base", True]
    m = get_model(rec["par"])
    assert float(m.PBDOT.value) == 1e-11 and not m.PBDOT.frozen and m.PB.value is None
    assert [p for p in m.free_params if m[p].component == "Binary"] == rec["free"]


def test_cap():
    """20 terms (PINT_MAX_FB) build a layout; a 21st line is refused by build_layout with a
    NotImplementedError naming PINT_MAX_FB (the reference sets no limit)."""
    from pint_amd import _lib as L
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    rec = forms()["fb20"]
    assert rec["result"] == "ok" and rec["binary_delay_equals"] == ["base", True]
    toas = load("fbx_ell1_wls")[1]
    m = get_model(rec["par"])
    assert m.fb_terms() == [f"FB{k}" for k in range(20)] and L.MAX_FB == 20
    assert [p for p in m.params if m[p].component == "Binary" and m[p].value is not None and not getattr(m[p], "implicit", False)] == \
        [p for p in rec["binary_params"] if rec["values"][p] is not None and p not in ("ECC", "OM")]
    lay = build_layout(m, toas)
    assert lay.spec.rsv_[2] >> 24 == 20
    m21 = get_model(rec["par"] + "FB20 0.0\n")
    with pytest.raises(NotImplementedError, match="PINT_MAX_FB"):
        build_layout(m21, toas)


@pytest.mark.parametrize("binary", ("DDK", "DDS", "DDH", "ELL1k"))
def test_other_binaries_with_fbn_are_refused(binary):
    from pint_amd import get_model
    par = open(os.path.join(GOLDEN, {"DDK": "pta_ddk", "DDS": "dds_wls", "DDH": "ddh_wls", "ELL1k": "ell1k_wls"}[binary]
                            + ".par")).read()
    assert get_model(par).binary == binary
    par = "".join(l + "\n" for l in par.splitlines() if l.split() and l.split()[0] != "PB") + "FB0 7.5e-6 1\n"
    with pytest.raises(NotImplementedError, match=f"{binary}.*FB0"):
        get_model(par)


@pytest.mark.parametrize("name", NAMES)
def test_layout(name):
    """The FBn block: nfb contiguous dd pairs in ascending order, described by the reserve word
    (PINT_SPEC_NFB / PINT_SPEC_O_FB); PB without a slot; the free FBn as PINT_COL_BIN columns with
    ids PINT_B_FB0 + n; the other reserve words and the spec's size untouched."""
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout, pack_table
    from pint_amd.timing_model import BIN_IDS
    model, toas, z, meta = load(name)
    lay = build_layout(model, toas)
    nfb = 3 if name in WLS else 4
    assert ctypes.sizeof(L.SpecT) == 4128 and L.B_FB0 == 29 and L.B_NPAR == 27
    w = lay.spec.rsv_[2]
    o_fb = (w & 0xFFFFFF) - 1
    assert w >> 24 == nfb and list(lay.spec.rsv_)[:2] == [0, 0]
    assert lay.spec.binary == {"ELL1": L.BIN_ELL1, "ELL1H": L.BIN_ELL1H, "DD": L.BIN_DD, "BT": L.BIN_BT}[BINARY[name]]
    assert lay.spec.o_bin[BIN_IDS["PB"]] == -1 and "PB" not in lay.offsets
    tab = pack_table(lay)
    for k in range(nfb):
        assert lay.offsets[f"FB{k}"] == o_fb + 2 * k and o_fb + 2 * nfb <= lay.spec.tstride
        assert LD(tab[o_fb + 2 * k]) + LD(tab[o_fb + 2 * k + 1]) == LD(model[f"FB{k}"].value)
        c = lay.columns.index(f"FB{k}")
        assert (lay.spec.col_kind[c], lay.spec.col_index[c], lay.spec.col_toff[c]) == (L.COL_BIN, L.B_FB0 + k, o_fb + 2 * k)
    for p in meta["binary_free"]:
        if not _is_fb(p):
            c = lay.columns.index(p)
            assert (lay.spec.col_kind[c], lay.spec.col_index[c]) == (L.COL_BIN, BIN_IDS[p])
    assert lay.columns == meta["dm_params"] or BINARY[name] == "BT"
    assert sorted(lay.columns) == sorted(meta["dm_params"])


@pytest.mark.parametrize("name", NAMES)
def test_parfile_round_trip(name):
    """The post-fit model writes the BINARY line and the binary parameters' lines equal to the
    reference's as_parfile text (FBn with their long-double digits), in its order; reading them back
    gives the same values, fit flags and uncertainties."""
    from pint_amd import get_model
    model, toas, z, meta = load(name)
    key = "wls" if name in WLS else "gls"
    for p, s in meta[key + "_errors"].items():
        v = ref_value(meta, key + "_params", p)
        model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
        model[p].uncertainty = s
    names = {"BINARY", "PB", "PBDOT", "A1", "A1DOT", "ECC", "EDOT", "T0", "OM", "OMDOT", "M2", "SINI", "A0", "B0", "GAMMA",
             "DR", "DTH", "TASC", "EPS1", "EPS2", "H3", "STIGMA"}
    own = lambda l: bool(l.split()) and (l.split()[0] in names or _is_fb(l.split()[0]))  # noqa: E731
    ref = [l for l in meta[key + "_parfile"].splitlines() if own(l)]
    got = [l for l in model.as_parfile().splitlines() if own(l)]
    assert ref[0].split() == ["BINARY", BINARY[name]] and len(ref) >= 9
    assert not any(l.split()[0] == "PB" for l in ref)
    assert got == ref
    back = get_model(model.as_parfile())
    assert back.binary == model.binary and back.fb_terms() == model.fb_terms() and back.PB.value is None
    for p in model.params:
        if model[p].component == "Binary":
            a, b = model[p], back[p]
            assert a.value == b.value and a.frozen == b.frozen, p
            assert (a.uncertainty_value or 0.0) == (b.uncertainty_value or 0.0), p


def test_pb():
    """TimingModel.pb() (pulsar_binary.py:566-625): PB and its uncertainty in days, from PB, or from
    1 / FB0 with sigma_FB0 / FB0^2."""
    import golden_util
    model = load("fbx_dd_wls")[0]
    model.FB0.uncertainty = 6.25e-16
    v, s = model.pb()
    f = LD(model.FB0.value)
    assert abs(v - 1 / f / 86400) < 1e-18 and abs(float(v) - 1.534492) < 1e-6  # (days)
    assert abs(s / (6.25e-16 / float(f) ** 2 / 86400) - 1) < 1e-12
    model.FB0.uncertainty = 0.0
    assert model.pb()[1] is None
    m = golden_util.load("pta_ell1")[0]
    m.PB.uncertainty = 1e-9
    assert m.pb() == (LD(m.PB.value), 1e-9)


def test_spec_bad_arguments():
    """pint_add_pulsar refuses a malformed FBn word before anything touches the device: nfb outside
    1..PINT_MAX_FB, a block outside the table, a model without a binary (or one of the other models),
    a PB slot beside the block; each with -PINT_E_INVALID and a message naming the block."""
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout, pack_toas
    from pint_amd.timing_model import BIN_IDS
    model, toas, z, meta = load("fbx_dd_wls")
    lay = build_layout(model, toas)
    lib = L.lib()
    ctx = lib.pint_ctx_create(0)
    t, keep = pack_toas(lay)
    o_fb = (lay.spec.rsv_[2] & 0xFFFFFF) - 1
    word = lambda o, n: (n << 24) | (o + 1)  # noqa: E731

    def call(change):
        spec = L.SpecT.from_buffer_copy(bytes(lay.spec))
        change(spec)
        rc = lib.pint_add_pulsar(ctx, ctypes.byref(t), ctypes.byref(spec), L.ptr(np.zeros(2)), L.ptr(np.zeros(1)))
        return rc, lib.pint_last_error(ctx).decode()

    def setw(o, n):
        return lambda s: s.rsv_.__setitem__(2, word(o, n))

    def other_binary(b):
        return lambda s: setattr(s, "binary", b)

    bad = [setw(o_fb, 21), setw(o_fb, 0), setw(o_fb, 127), setw(lay.spec.tstride - 4, 3), setw(lay.spec.tstride, 1),
           setw(-1, 3), other_binary(L.BIN_NONE), other_binary(L.BIN_DDK), other_binary(L.BIN_ELL1K),
           lambda s: s.o_bin.__setitem__(BIN_IDS["PB"], 0)]
    for ch in bad:
        rc, msg = call(ch)
        assert rc == -L.PINT_E_INVALID and "FBn block" in msg, (rc, msg)
    lib.pint_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_delay_phase_residuals_columns(name):
    """Measured on one MI355X (fbx_ell1_wls / fbx_ell1h_wls / fbx_dd_wls / fbx_bt_wls / fbx_ell1_gls /
    fbx_dd_gls): total delay 1.7e-13 / 1.1e-13 / 1.7e-13 / 1.1e-13 / 2.9e-13 / 4.8e-13 s, TZR delay <=
    1.7e-13 s, binary delay 1.5e-13 / 1.4e-13 / 1.5e-13 / 1.3e-13 / 3.0e-13 / 4.8e-13 s, phase 9.3e-10 (the
    four WLS) / 7.5e-9 / 3.7e-9 cycles, residuals 4.9e-12 / 4.6e-12 / 5.5e-12 / 6.6e-12 / 1.7e-11 / 2.1e-11
    s; binary columns, of the column's maximum: T0 1.6e-13 on fbx_dd_wls and fbx_dd_gls (the worst:
    MEASURED_COL; BT's T0 8.8e-15), SINI <= 9.6e-14, EPS1 / EPS2 <= 7.7e-14, H3 4.4e-14, STIGMA 6.9e-14;
    FB0 ... FB3 <= 3.7e-14 (ELL1, ELL1H), <= 7.6e-15 (DD), <= 6.4e-15 (BT)."""
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
    params = list(params)
    assert sorted(params) == sorted(meta["dm_params"])
    refM = z["dm_M"][:, [meta["dm_params"].index(p) for p in params]]  # (BT: T0 stands where this project has it)
    scale = np.max(np.abs(refM), axis=0)
    assert np.all(scale > 0)
    err = np.max(np.abs(M - refM), axis=0) / scale
    bins = [j for j, p in enumerate(params) if p in meta["binary_free"]]
    assert len(bins) == len(meta["binary_free"]) >= 8
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
    if BINARY[name] in T0_MODELS:  # (the as-is column is zero)
        assert np.max(np.abs(M[:, params.index("T0")])) > 1e-4


def _check_fit(f, name, meta, key, kind, etol):
    worst = 0.0
    for p in meta[key + "_params"]:
        s = meta[key + "_errors"][p]
        d = abs(float((LD(f.model[p].value) - ref_value(meta, key + "_params", p)) / LD(s)))
        worst = max(worst, d)
        assert d <= fit_bar(name, kind, p), (p, d, fit_bar(name, kind, p))
        assert abs(f.model[p].uncertainty / s - 1) < etol, (p, f.model[p].uncertainty / s - 1)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fit(name):
    """One WLS (GLS) step with FB0 ... FBn and every other binary parameter free: parameters within
    max(1e-3 sigma, 2 x spread) of the reference's, uncertainties, chi2 within the spread's bar."""
    from pint_amd import GLSFitter, Residuals, WLSFitter
    model, toas, z, meta = load(name)
    key = "wls" if name in WLS else "gls"
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (WLSFitter if key == "wls" else GLSFitter)(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, name, meta, key, "fit", 1e-6 if key == "wls" else 1e-5)
    if key == "gls":
        pre = rms_ps(f.resids.time_resids, z["gls_post_resid"])
    bar = chi2_bar(name, "fit", pre)
    print(f"{name}: {key} worst {worst:.2e} sigma, chi2 rel {c2 / meta[key + '_chi2'] - 1:.2e} (bar {bar:.1e})")
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
          f"worst {dev[pw]:.2e} sigma ({pw}, bar {fit_bar(name, 'downhill', pw):.1e})")
    assert abs(f.resids.chi2 / meta["down_chi2"] - 1) < bar
    # the uncertainties belong to the point where the line search stops: they agree to the one-step
    # fits' 1e-6 / 1e-5 where that point is the reference's, and otherwise move with it.  An
    # uncertainty means something only while the model is linear across one sigma, so a stop k sigma
    # away moves it by at most about k of itself; k is bounded by 2 x the spread of the reference's own
    # stop (fbx_fit_spread.json "downhill", the largest over the parameters; no 1e-3 floor here)
    ubar = max(1e-6 if name in WLS else 1e-5, 2.0 * max(_spread()[name]["downhill"]["max_dev_sigma"].values()))
    for p, d in dev.items():
        assert d < fit_bar(name, "downhill", p), (p, d, fit_bar(name, "downhill", p))
        assert abs(f.model[p].uncertainty / meta["down_errors"][p] - 1) < ubar, (p, ubar)


@pytest.mark.gpu
def test_gpu_grid():
    """The reference's 3x3 grid_chisq over (FB0, FB1), +-1 sigma about the start, taken on its
    executor path (every point fitted on a copy of the base model, as the device's batch of
    independent points is), at golden_util.chi2_bar's rule on the fixture's "fit" spread; the same
    argmin."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    name = "fbx_ell1_wls"
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    n0, n1 = meta["grid_params"]
    assert (n0, n1) == ("FB0", "FB1")
    g0 = z[f"grid_{n0}_hi"].astype(LD) + z[f"grid_{n0}_lo"]
    g1 = z[f"grid_{n1}_hi"].astype(LD) + z[f"grid_{n1}_lo"]
    c2, _ = grid_chisq(f, (n0, n1), (g0, g1))
    ref = z["grid_chi2"]
    bar = chi2_bar(name, "fit", pre)
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"{name}: ({n0}, {n1}) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}")
    assert c2.shape == ref.shape == (3, 3)
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)


def _eval_all(items):
    """Evaluation outputs (delay, phase, spin frequency, status), design matrix, residuals and chi2 of
    every (model, toas) in one session."""
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
    s.close()
    return out


@pytest.mark.gpu
def test_gpu_mixed_batch():
    """fbx_ell1_wls, fbx_dd_wls, c5_ell1 and c5_dd in one Session (the period form and the FBn form
    of one binary model share the batch: the merged launch for the c5 pair, a launch of its own for
    each FBn block kind) against each alone: evaluation outputs, design matrix, residuals and chi2 bit
    for bit.  (The fit step is not compared: the Gram's row split, and with it its summation order, is
    chosen per batch from the instance count and the longest instance, 300 rows alone against 5000
    here, so a step differs in its last bits between any two batch shapes, with or without FBn.)"""
    import golden_util
    items = [load(n)[:2] for n in ("fbx_ell1_wls", "fbx_dd_wls")] + [golden_util.load(n)[:2] for n in ("c5_ell1", "c5_dd")]
    mixed = _eval_all(items)
    for k, it in enumerate(items):
        (alone,) = _eval_all([it])
        assert len(alone) == len(mixed[k]) >= 5
        for x, y in zip(mixed[k], alone):
            np.testing.assert_array_equal(x, y)
        assert np.all(np.isfinite(alone[-4])) and np.max(np.abs(alone[-4])) > 0


@pytest.mark.gpu
def test_gpu_lazy_pipelined():
    """fbx_ell1_gls and fbx_dd_gls in a lazy, pipelined session (the bench's step shape, two steps in
    flight: test_fdjump's test of the same name) against the synchronous session: the step, its
    errors and the noise realisations bit for bit -- the FBn block kinds' launches are enqueued like
    the others, and the fused residual pass takes its rows from their block lists."""
    from pint_amd.engine import Session, build_layout, pack_table
    items = [load("fbx_ell1_gls")[:2], load("fbx_dd_gls")[:2]]

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
