"""The Glitch component (glitch.py:127-344) on the device path, against fixtures captured from
the reference (scripts/refgen/gen_glitch.py):

* gl_wls : WLS, a Vela-like isolated pulsar with two glitches (glitch 1: frozen epoch, phase,
           F0/F1/F2 steps and a decaying step with its time constant free; glitch 2, listed first
           in the par file: free epoch, F0/F1 steps, no GLPH line); TZRMJD between the epochs;
* gl_gls : GLS, the bench's per-pulsar shape (ELL1, DMX, red noise) with one glitch in the span.

The bars are the project's bars for every other fixture; the chi2 bars
follow golden_util.chi2_bar's rule, read from gl_fit_spread.json (the reference's own spread
for these fixtures).  The absolute-phase bar is the residual bar as phase, 1e-10 s x F0, plus 8
ulps of the reference's longdouble phase (test_oracle_golden's allowance for it).
"""
import copy
import hashlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, ref_value, rms_ps, SPREAD_MAX_PS

LD = np.longdouble
NAMES = ("gl_wls", "gl_gls")
PROPS = ("GLEP_", "GLPH_", "GLF0_", "GLF1_", "GLF2_", "GLF0D_", "GLTD_")
_CACHE = {}


def load(name):
    """golden_util.load for the glitch fixtures (par file = fixture name); the arrays and the meta
    are loaded once and shared, the model is a fresh copy per caller."""
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
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "gl_fit_spread.json")))
    return _CACHE["spread"]


def chi2_bar(name, kind, resid_rms_ps, floor=1e-9):
    """golden_util.chi2_bar's rule on gl_fit_spread.json: 2 x the reference's per-ps chi2 spread
    x the measured residual rms (at least 5 ps, at most the calibrated 30 ps)."""
    d = _spread()[name]
    per_ps = max(d["5ps"][kind] / 5.0, d["30ps"][kind] / 30.0)
    return max(floor, 2.0 * per_ps * min(max(float(resid_rms_ps), 5.0), SPREAD_MAX_PS))


def downhill_bar(name, p, floor=1e-3):
    return max(floor, 2.0 * _spread()[name]["downhill"]["max_dev_sigma"].get(p, 0.0))


def _par_without(name, *drop):
    lines = open(os.path.join(GOLDEN, name + ".par")).read().splitlines()
    return "\n".join(l for l in lines if not (l.split() and l.split()[0] in drop)) + "\n"


def _glitch_cols(params):
    """{glitch index: [(column, parameter)]} of the free glitch parameters."""
    out = {}
    for j, p in enumerate(params):
        if p.startswith("GL") and "_" in p:
            out.setdefault(int(p.split("_")[1]), []).append((j, p))
    return out


def _glitch_dt(name):
    """The reference's dt = (tdbld - GLEP) 86400 s - delay of every glitch epoch of the fixture's
    model (and of gl_wls's GLEP_2 grid values) at the TOAs and at the TZR TOA."""
    model, toas, z, meta = load(name)
    t = z["tdb_hi"].astype(LD) + z["tdb_lo"].astype(LD)
    tz = LD(z["tzr_tdb_hi"][0]) + LD(z["tzr_tdb_lo"][0])
    eps = {n: LD(model[n].value) for n in model.params if n.startswith("GLEP_")}
    if "grid_GLEP_2_hi" in z:
        for i, (h, l) in enumerate(zip(z["grid_GLEP_2_hi"], z["grid_GLEP_2_lo"])):
            eps[f"grid{i}"] = LD(h) + LD(l)
    return {n: (np.asarray((t - ep) * 86400 - z["delay_total"], dtype=np.float64),
                float((tz - ep) * 86400 - z["tzr_delay"][0])) for n, ep in eps.items()}


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the GPU tests rely on: no TOA nor the TZR TOA within 1 ms of a glitch epoch (the
    grid's GLEP_2 values included), so dt > 0 is never decided by rounding; at least 20 TOAs on
    either side of every glitch; the reference's glitch phase exceeds a cycle, so no test passes
    with the term missing; every free glitch column has a non-zero maximum."""
    model, toas, z, meta = load(name)
    for n, (dt, dz) in _glitch_dt(name).items():
        assert np.min(np.abs(dt)) > 1e-3 and abs(dz) > 1e-3, n
        if n.startswith("GLEP_"):
            assert np.sum(dt < 0) >= 20 and np.sum(dt > 0) >= 20, n
    assert np.max(np.abs(z["glitch_phase_hi"])) > 1.0
    cols = _glitch_cols(meta["dm_params"])
    assert cols
    for k, lst in cols.items():
        for j, p in lst:
            assert np.max(np.abs(z["dm_M"][:, j])) > 0, p
    if name == "gl_wls":  # the TZR TOA lies after glitch 1 and before glitch 2
        assert abs(z["tzr_glitch_phase_hi"][0]) > 1.0
        d = _glitch_dt(name)
        assert d["GLEP_1"][1] > 0 > d["GLEP_2"][1]


@pytest.mark.parametrize("name", NAMES)
def test_layout(name):
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout
    model, toas, z, meta = load(name)
    assert [p for p in model.params if p.startswith("GL")] == [p for p in meta["model"]["params"] if p.startswith("GL")]
    lay = build_layout(model, toas)
    assert lay.columns == meta["dm_params"]  # the glitch columns where the reference's design matrix has them
    idx = model.glitch_indices()
    assert lay.spec.nglitch == len(idx) and lay.spec.o_GLITCH == lay.offsets[f"GLEP_{idx[0]}"]
    for k, i in enumerate(idx):
        for w, pre in enumerate(PROPS):
            assert lay.offsets[f"{pre}{i}"] == lay.spec.o_GLITCH + 14 * k + 2 * w
            if f"{pre}{i}" in lay.columns:
                c = lay.columns.index(f"{pre}{i}")
                assert lay.spec.col_kind[c] == L.COL_GLITCH and lay.spec.col_index[c] == 7 * k + w
                assert lay.spec.col_toff[c] == lay.offsets[f"{pre}{i}"]
    assert lay.spec.o_GLITCH + 14 * len(idx) <= lay.tstride


def test_layout_without_glitch_is_the_parents():
    """pta_iso has no glitch: its parameter table and table offsets are the ones the code before
    this component gave (their hashes, recorded from it), and its spec differs from that code's
    in the new fields alone -- o_GLITCH -1, nglitch 0 and three reserve words where one reserve
    word stood."""
    import golden_util
    from pint_amd import _lib as L
    from pint_amd.engine import build_layout, pack_table
    model, toas, z, meta = golden_util.load("pta_iso")
    lay = build_layout(model, toas)
    assert lay.spec.o_GLITCH == -1 and lay.spec.nglitch == 0 and list(lay.spec.rsv_) == [0, 0, 0]
    assert hashlib.sha256(pack_table(lay).tobytes()).hexdigest() == \
        "d50cf50a3018718c5effddf8a65b45cb702d696e8780a3a01f413b7973bcc81f"
    assert hashlib.sha256(repr(list(lay.offsets.items())).encode()).hexdigest() == \
        "ca1ee53fe23016db57b8fdb8e518568678f5375e3dd94c52cb4720b0294bdfe8"
    b = bytes(lay.spec)
    o = L.SpecT.o_GLITCH.offset
    assert o == L.SpecT.o_NE_SW.offset + 4 and L.SpecT.col_kind.offset == o + 20 and len(b) % 16 == 0
    old = b[:o] + bytes(4) + b[o + 20:]
    assert hashlib.sha256(old).hexdigest() == "d993d9149f99392cd1bc13abec1128320ac9b59fef1cc91d1acf4ae1c21924ee"


def test_parfile_round_trip():
    """The post-fit gl_wls model (the reference's fitted values and uncertainties) writes glitch
    lines equal to the reference's as_parfile text, in its order; reading them back gives the
    same values, fit flags and uncertainties; the par-file order of the glitch indices does not
    matter to the layout or the table."""
    from pint_amd import get_model
    from pint_amd.engine import build_layout, pack_table
    model, toas, z, meta = load("gl_wls")
    for p, s in meta["wls_errors"].items():
        v = ref_value(meta, "wls_params", p)
        model[p].value = v if (model[p].long_double or model[p].kind == "mjd") else float(v)
        model[p].uncertainty = s
    ref = [l for l in meta["wls_parfile"].splitlines() if l.split() and l.split()[0].startswith("GL")]
    got = [l for l in model.as_parfile().splitlines() if l.split() and l.split()[0].startswith("GL")]
    assert len(ref) == 14 and got == ref
    back = get_model(model.as_parfile())
    for i in (1, 2):
        for pre in PROPS:
            a, b = model[f"{pre}{i}"], back[f"{pre}{i}"]
            assert a.value == b.value and a.frozen == b.frozen, a.name
            assert (a.uncertainty_value or 0.0) == (b.uncertainty_value or 0.0), a.name
    # glitch 1's lines first instead of glitch 2's
    lines = open(os.path.join(GOLDEN, "gl_wls.par")).read().splitlines()
    g2 = [l for l in lines if l.split()[0].endswith("_2")]
    g1 = [l for l in lines if l.split()[0].endswith("_1")]
    rest = [l for l in lines if l not in g1 and l not in g2]
    other = get_model("\n".join(rest + g1 + g2) + "\n")
    model, toas, z, meta = load("gl_wls")
    la, lb = build_layout(model, toas), build_layout(other, toas)
    assert la.columns == lb.columns and la.offsets == lb.offsets
    assert pack_table(la).tobytes() == pack_table(lb).tobytes()


def test_validate():
    from pint_amd import get_model
    from pint_amd.engine import build_layout
    from pint_amd.timing_model import MissingParameter
    base = open(os.path.join(GOLDEN, "gl_wls.par")).read()
    with pytest.raises(MissingParameter, match="GLEP_3"):
        get_model(base + "GLF0_3 1e-9 1\n")
    with pytest.raises(ValueError, match="Both the glitch epoch and phase cannot be fit for Glitch 2"):
        get_model(base + "GLPH_2 0.1 1\n")
    with pytest.raises(MissingParameter, match="GLTD_1"):
        get_model(_par_without("gl_wls", "GLTD_1"))
    # setup: every index that appears gets all seven parameters, the missing ones 0 and frozen
    m = get_model(base)
    for pre in ("GLPH_", "GLF2_", "GLF0D_", "GLTD_"):
        assert m[f"{pre}2"].value == 0.0 and m[f"{pre}2"].frozen
    # the cap: 64 glitches build a layout, 65 raise naming the limit
    toas = load("gl_wls")[1]
    bare = _par_without("gl_wls", *[f"{pre}{i}" for i in (1, 2) for pre in PROPS])
    many = "".join(f"GLEP_{i} {54510 + 15 * i}.3\nGLF0_{i} 1e-9\n" for i in range(1, 66))
    lay = build_layout(get_model(bare + "".join(many.splitlines(True)[:128])), toas)
    assert lay.spec.nglitch == 64
    with pytest.raises(NotImplementedError, match="64"):
        build_layout(get_model(bare + many), toas)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_delay_phase_residuals_columns(name):
    from pint_amd import Residuals
    from pint_amd.engine import evaluate_delay_phase
    model, toas, z, meta = load(name)
    n = toas.ntoas
    dp = evaluate_delay_phase(model, toas)
    e_d = np.max(np.abs(dp["delay"] - z["delay_total"]))
    e_tz = abs(dp["tzr_delay"] - z["tzr_delay"][0])
    # the absolute phase of the TOAs and of the TZR row (mean subtraction hides a wrong TZR
    # glitch phase from the residuals)
    got = dp["phase_hi"].astype(LD) + dp["phase_lo"].astype(LD)
    ref = z["abs_phase_int"].astype(LD) + z["abs_phase_frac_hi"].astype(LD) + z["abs_phase_frac_lo"].astype(LD)
    ref_tz = LD(z["tzr_abs_phase_int"][0]) + LD(z["tzr_abs_phase_frac_hi"][0]) + LD(z["tzr_abs_phase_frac_lo"][0])
    e_ph = float(np.max(np.abs(got[:n] - ref)))
    e_phz = float(abs(got[n] - ref_tz))
    ph_bar = 1e-10 * float(model.F0.value) + 8 * float(np.spacing(np.max(np.abs(ref))))
    r = Residuals(toas, model)
    e_r = np.max(np.abs(r.time_resids - z["res_time"]))
    M, params, _ = model.designmatrix(toas)
    assert list(params) == meta["dm_params"]
    refM = z["dm_M"]
    scale = np.max(np.abs(refM), axis=0)
    scale[scale == 0] = 1
    err = np.max(np.abs(M - refM) / scale, axis=0)
    cols = _glitch_cols(params)
    gl = [j for lst in cols.values() for j, _ in lst]
    print(f"{name}: delay {e_d:.2e} s, TZR delay {e_tz:.2e} s, phase {e_ph:.2e} / TZR {e_phz:.2e} cycles "
          f"(bar {ph_bar:.1e}), residuals {e_r:.2e} s, columns max {err.max():.2e} ({params[int(np.argmax(err))]}), "
          f"glitch columns max {err[gl].max():.2e}")
    assert e_d <= 5e-12 and e_tz <= 5e-12
    assert e_ph <= ph_bar and e_phz <= ph_bar
    assert e_r <= 1e-10
    bad = {params[k]: err[k] for k in np.where(err > 1e-9)[0]}
    assert not bad, bad
    # exactly zero on the rows the glitch does not act on
    dts = _glitch_dt(name)
    for k, lst in cols.items():
        off = dts[f"GLEP_{k}"][0] <= 0
        assert 20 <= np.sum(off) <= n - 20
        for j, p in lst:
            assert np.all(M[off, j] == 0.0), p
            assert np.all(refM[off, j] == 0.0), p


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
    model, toas, z, meta = load("gl_wls")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "wls", 1e-6)
    bar = chi2_bar("gl_wls", "fit", pre)
    print(f"gl_wls: WLS worst {worst:.2e} sigma, chi2 rel {c2 / meta['wls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["wls_chi2"] - 1) < bar


@pytest.mark.gpu
def test_gpu_gls_fit():
    from pint_amd import GLSFitter
    model, toas, z, meta = load("gl_gls")
    f = GLSFitter(toas, model)
    c2 = f.fit_toas(maxiter=1)
    worst = _check_fit(f, meta, "gls", 1e-5)
    bar = chi2_bar("gl_gls", "fit", rms_ps(f.resids.time_resids, z["gls_post_resid"]))
    print(f"gl_gls: GLS worst {worst:.2e} sigma, chi2 rel {c2 / meta['gls_chi2'] - 1:.2e} (bar {bar:.1e})")
    assert worst <= 1e-3
    assert abs(c2 / meta["gls_chi2"] - 1) < bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_downhill(name):
    from pint_amd import DownhillGLSFitter, DownhillWLSFitter, Residuals
    from pint_amd.fitter import MaxiterReached, StepProblem
    model, toas, z, meta = load(name)
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = (DownhillWLSFitter if name == "gl_wls" else DownhillGLSFitter)(toas, model)
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
def test_gpu_grid_glep_gltd():
    """The reference's 5x5 (GLEP_2, GLTD_1) grid_chisq around the one-step fit: the larger of the
    WLS grid bar (rtol 1e-7) and gl_wls's "fit" spread bar; the same argmin."""
    from pint_amd import Residuals, WLSFitter
    from pint_amd.gridutils import grid_chisq
    model, toas, z, meta = load("gl_wls")
    pre = rms_ps(Residuals(toas, model).time_resids, z["res_time"])
    f = WLSFitter(toas, model)
    f.fit_toas(maxiter=1)
    g0 = z["grid_GLEP_2_hi"].astype(LD) + z["grid_GLEP_2_lo"]
    g1 = z["grid_GLTD_1_hi"].astype(LD) + z["grid_GLTD_1_lo"]
    c2, _ = grid_chisq(f, ("GLEP_2", "GLTD_1"), (g0, g1))
    ref = z["grid_chi2"]
    bar = max(1e-7, chi2_bar("gl_wls", "fit", pre))
    rel = np.max(np.abs(c2 / ref - 1))
    print(f"gl_wls: (GLEP_2, GLTD_1) grid max rel {rel:.2e} (bar {bar:.1e}), chi2 {ref.min():.3f} .. {ref.max():.3f}, "
          f"{int(np.sum(~np.isfinite(c2)))} points not finite")
    assert c2.shape == ref.shape == (5, 5)
    assert rel < bar
    assert np.argmin(c2) == np.argmin(ref)


@pytest.mark.gpu
def test_gpu_spin_grid_bit_identical():
    """A 3x3 (F1, GLF0_1) grid on gl_wls with the shared-head evaluation on and off: the same
    bits.  A glitch parameter is as phase-only as an F term, so the grid takes the shared head
    (k_eval_head / k_eval_spin; asserted), which serves isolated models outside the fused residual
    pass: both runs switch that pass off.  The centre point is the model itself: its glitch
    columns must also equal those of a plain (non-grid) evaluation, which never goes through the
    head."""
    from pint_amd.engine import Session, build_layout, pack_table
    model, toas, z, meta = load("gl_wls")

    def run(spin):
        s = Session()
        s.set_spin_eval(spin)
        s.set_efuse(False)
        lay = s.add(build_layout(model, toas))
        base = pack_table(lay, model)
        g0 = LD(model.F1.value) + np.linspace(-2, 2, 3) * LD(1e-18)
        g1 = LD(model.GLF0_1.value) + np.linspace(-2, 2, 3) * LD(1e-11)
        s.set_grid(lay, base, [("F1", g0, 3, 3), ("GLF0_1", g1, 1, 3)], 9)
        s.eval(want_M=True)
        took = s.n_spin_eval()
        out = [np.array(x, copy=True) for x in s.read_eval()] + [np.array(s.read_designmatrix(), copy=True)]  # (9, n, K)
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
    for k, lst in _glitch_cols(lay.columns).items():
        for j, p in lst:
            ref = M[:, list(params).index(p)]
            assert np.max(np.abs(ref)) > 0
            assert np.max(np.abs(a[4][4][:, j] - ref)) <= 1e-12 * np.max(np.abs(ref)), p


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
    """gl_gls beside pta_iso and pta_ell1 in one session (the per-instance uniform branch, the
    LDS-staged spec): gl_gls's step and chi2 equal its single-session result to 1e-12 relative;
    the neighbours' steps, errors and chi2 are bit-identical to a session without gl_gls."""
    import golden_util
    gl = load("gl_gls")[:2]
    iso, ell1 = golden_util.load("pta_iso")[:2], golden_util.load("pta_ell1")[:2]
    mixed = _gls_steps([iso, gl, ell1])
    (alone,) = _gls_steps([gl])
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
    """gl_gls's GLS step on the generated-Fourier compact path, the stored-basis compact path
    and the full layout: the same normal equations to rounding (the bars of
    test_generated_fourier_path_matches_stored and test_compact_layout's full-layout check)."""
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    model, toas = load("gl_gls")[:2]
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
