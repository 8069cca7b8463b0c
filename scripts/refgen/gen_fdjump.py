"""Golden fixtures for the FDJump and FDJumpDM components (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* fdj_wls : WLS.  An isolated pulsar (equatorial astrometry, DM, a global FD1) timed by three
            systems (-fe P 400-480 MHz, L 1150-1750 MHz, S 1700-2400 MHz, 8 channels each, so
            y^p varies within a system) and two backends (-be B1 / B2); 400 TOAs from the
            geocentre over MJD 54500-55600, 1 us errors.  FD1JUMP and FD2JUMP free on L (the
            index-1 lines in the tempo2 spelling FDJUMP1), FDJUMP1 free on S, a frozen non-zero
            FD3JUMP on -be B2 (index 3 without 1 and 2 on that mask), an FDJUMP1 keyed on an MJD
            range that holds the TZR TOA and overlaps L and S TOAs, a free FDJUMPDM on P.  No
            FDJUMPLOG line (the constructor's value is recorded).  Captured from a perturbed
            start.  Beside what gen_synth.capture(fit="wls") records: the absolute phase of the
            TOAs and of the TZR TOA, each component's delay for the TZR TOA, the post-fit
            as_parfile(), a 5x5 grid_chisq over (FD1JUMP1, DM), and what the reference does with
            the forms it rejects or rewrites ("forms").
* fdj_lin : the same par with the opposite FDJUMPLOG value, 200 TOAs.
* fdj_gls : GLS.  gen_synth.pta_par(24, "ELL1") (the bench's per-pulsar shape: DMX, PLRedNoise,
            EFAC/EQUAD) with -fe flags by band, FD1JUMP / FD2JUMP free on band A, a free
            FDJUMPDM on band C, a frozen CM, one DMWaveX harmonic and one glitch; 1000 TOAs in
            four bands of +-20 %.
* fdj_fit_spread.json : gen_fit_spread.measure of fdj_wls and fdj_gls plus the Downhill spread,
            in cm_fit_spread.json's schema.

The order of the delay components.  fdjump and fdjumpdm are not categories of the reference's
DEFAULT_ORDER (nor are dmwavex, chromatic_constant and cmwavex): those components follow
everything else in the iteration order of a set of names, which changes with the interpreter's
hash seed.  The device path sums ... WaveX, DMWaveX, ChromaticCM, CMWaveX, FDJump, FDJumpDM and
lists the phase components' parameters first; `find` searches for a seed under which both
fixture models have that order, and every capture asserts it (seed SEED below).

Usage: PYTHONHASHSEED=<SEED> oracle/refenv/run_ref.sh scripts/refgen/gen_fdjump.py [fdj_wls fdj_lin fdj_gls spread]
       oracle/refenv/run_ref.sh scripts/refgen/gen_fdjump.py find
"""
import copy
import io
import json
import os
import subprocess
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
import pint.simulation as sim  # noqa: E402
import pint.fitter as pfit  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.gridutils import grid_chisq  # noqa: E402

from gen_solar_wind import write_par, downhill_spread  # noqa: E402
from gen_chromatic import check_errors, fixed_point  # noqa: E402

SEED = 26  # (what `find` gives; every capture asserts the order it stands for)
CANONICAL = ["WaveX", "DMWaveX", "ChromaticCM", "CMWaveX", "FDJump", "FDJumpDM"]
FDJ_FUNCS = {"fdjump_delay": "fdjump_delay", "fdjumpdm_delay": "fdjump_dm_delay"}
BANDS_WLS = {"P": (400.0, 480.0), "L": (1150.0, 1750.0), "S": (1700.0, 2400.0)}
CM_GLS_COND = 1e12  # the bound cm_gls was generated under (gen_chromatic.check)


def wls_par(a1="1.0e-5", a2="2.0e-5", s1="3.0e-5", m1="2.0e-6", dmj="1.0e-4", dm="9.0233", log_line=""):
    return f"""PSR J1012-FDJ
RAJ 10:12:33.4372 1
DECJ 53:07:02.512 1
F0 218.8118404 1
F1 -4.08e-16 1
PEPOCH 55000
POSEPOCH 55000
DM {dm} 1
FD1 1.2e-5 1
{log_line}FDJUMP1 -fe L {a1} 1
FD2JUMP -fe L {a2} 1
FDJUMP1 -fe S {s1} 1
FD3JUMP -be B2 2.0e-5
FDJUMP1 mjd 55350 55450 {m1} 1
FDJUMPDM -fe P {dmj} 1
EPHEM builtin
CLK TT(TAI)
UNITS TDB
TZRMJD 55400.1234
TZRFRQ 1400
TZRSITE geocenter
"""


def gls_par(scale=1.0):
    return pta_par(24, "ELL1") + f"""FD1JUMP -fe A {2.0e-5 * scale!r} 1
FD2JUMP -fe A {4.0e-5 * scale!r} 1
FDJUMPDM -fe C {3.0e-4 * scale!r} 1
CM 0.02
DMWXEPOCH 54900
DMWXFREQ_0001 0.0005
DMWXSIN_0001 {1.0e-4 * scale!r} 1
DMWXCOS_0001 {-1.4e-4 * scale!r} 1
GLEP_1 55100.3
GLF0_1 {2.0e-9 * scale!r} 1
"""


def is_fdj(n):
    import re
    return bool(re.match(r"^(FD\d+JUMP\d+|FDJUMPDM\d+|FDJUMPLOG)$", n))


def order_ok(model):
    order = [type(c).__name__ for c in model.DelayComponent_list if type(c).__name__ in CANONICAL]
    return order == [c for c in CANONICAL if c in order] and list(model.components.keys())[0] == "AbsPhase"


def find_seed(limit=400):
    """The first hash seed under which both fixture models have the canonical order."""
    run = os.path.join(HERE, "..", "..", "oracle", "refenv", "run_ref.sh")
    for s in range(limit):
        r = subprocess.run([run, os.path.abspath(__file__), "order"], env=dict(os.environ, PYTHONHASHSEED=str(s)),
                           capture_output=True, text=True)
        if r.stdout.strip().endswith("ORDER OK"):
            print(f"PYTHONHASHSEED={s}")
            return s
    raise SystemExit("no seed found")


def set_flags(ts, fe, be=None):
    for i, fl in enumerate(ts.table["flags"]):
        fl["fe"] = fe[i]
        if be is not None:
            fl["be"] = be[i]


def wls_toas(true, n, seed):
    np.random.seed(seed)
    chans = []
    for lo, hi in BANDS_WLS.values():
        chans += list(np.linspace(lo, hi, 8))
    freq = np.resize(np.array(chans), n)
    fe = [list(BANDS_WLS)[(i % 24) // 8] for i in range(n)]
    be = ["B2" if i % 5 < 2 else "B1" for i in range(n)]
    ts = sim.make_fake_toas_uniform(54500, 55600, n, true, freq=freq * u.MHz, obs="geocenter", error=1 * u.us,
                                    add_noise=False, include_bipm=False, multi_freqs_in_epoch=False)
    set_flags(ts, fe, be)
    return sim.make_fake_toas(ts, true, add_noise=True)  # (re-zeroed with the flags in place)


def build_wls(log_line="", n=400, seed=71):
    true = get_model(io.StringIO(wls_par(log_line=log_line)))
    ts = wls_toas(true, n, seed)
    par = wls_par(a1="1.04e-5", a2="1.9e-5", s1="3.1e-5", m1="1.8e-6", dmj="1.1e-4", dm="9.02332", log_line=log_line)
    return par, get_model(io.StringIO(par)), ts


def build_lin():
    probe = get_model(io.StringIO(wls_par()))
    line = "FDJUMPLOG N\n" if probe.FDJUMPLOG.value else "FDJUMPLOG Y\n"
    return build_wls(log_line=line, n=200, seed=72)


def build_gls():
    np.random.seed(29)
    true = get_model(io.StringIO(gls_par()))
    n = 1000
    centre = np.array([800.0, 1200.0, 1600.0, 2000.0])[np.arange(n) % 4]
    freq = centre * (1.0 + 0.2 * (((np.arange(n) // 4) % 8) - 3.5) / 3.5)
    fe = ["ABCD"[i % 4] for i in range(n)]
    ts = sim.make_fake_toas_uniform(53000, 56652, n, true, freq=freq * u.MHz, obs="geocenter", error=0.5 * u.us,
                                    add_noise=False, include_bipm=False, multi_freqs_in_epoch=False)
    set_flags(ts, fe)
    ts = sim.make_fake_toas(ts, true, add_noise=True, add_correlated_noise=True)
    par = gls_par(scale=0.97)
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def extra_arrays(model, ts):
    """The absolute phase (abs_phase=False: no TZR subtraction) of the TOAs and of the TZR TOA, and
    each of the two components' delays for both."""
    out = {}
    tz = model.get_TZR_toa(ts)
    for key, t in (("abs", ts), ("tzr_abs", tz)):
        ph = model.phase(t, abs_phase=False)
        out[key + "_phase_int"] = np.asarray(ph.int.value, dtype=np.float64)
        out[key + "_phase_frac_hi"], out[key + "_phase_frac_lo"] = split_ld(ph.frac.value)
    for key, t in (("", ts), ("tzr_", tz)):
        parts = refcommon.component_delays(model, t)
        for n, fn in FDJ_FUNCS.items():
            out[key + n] = parts["delay_" + fn]
    return out


def selected(model, ts, names):
    sel = np.zeros(ts.ntoas, dtype=bool)
    for n in names:
        sel[getattr(model, n).select_toa_mask(ts)] = True
    return sel


def fdj_names(model):
    return ([n for n in model.components["FDJump"].fdjumps if getattr(model, n).quantity is not None],
            list(model.components["FDJumpDM"].fdjump_dms))


def check(model, ts, more):
    """The conditions the tests rely on; returns the recorded figures."""
    assert order_ok(model), "run with another PYTHONHASHSEED (see `find`)"
    M, names, _ = model.designmatrix(ts)
    names = list(names)
    new = [n for n in names if is_fdj(n)]
    assert new, names
    for n in new:
        assert np.max(np.abs(M[:, names.index(n)])) > 0, n
    fd, fdm = fdj_names(model)
    frac = {}
    for key, group in (("fdjump_delay", fd), ("fdjumpdm_delay", fdm)):
        sel = selected(model, ts, group)
        frac[key] = float(np.mean(np.abs(more[key][sel]) > 1e-7))
        assert sel.any() and frac[key] >= 0.5, (key, frac[key])
        assert np.all(more[key][~sel] == 0.0)
    # the whitened design matrix (rows / sigma, columns to unit norm): below cm_gls's bound
    sig = model.scaled_toa_uncertainty(ts).to_value(u.s)
    W = M / sig[:, None]
    s = W / np.sqrt(np.sum(W * W, axis=0))
    cond = float(np.linalg.cond(s.T @ s))
    print(f"  {len(names)} columns, whitened normalised Gram condition number {cond:.3g}; >100 ns on {frac}; "
          f"fdjump delay up to {np.max(np.abs(more['fdjump_delay'])):.3g} s, fdjumpdm delay up to "
          f"{np.max(np.abs(more['fdjumpdm_delay'])):.3g} s", file=sys.stderr)
    assert cond < CM_GLS_COND, cond
    return {"fdj_gram_cond": cond, "fdj_over_100ns": frac, "hash_seed": os.environ.get("PYTHONHASHSEED"),
            "delay_components": [type(c).__name__ for c in model.DelayComponent_list],
            "fdjumplog": bool(model.FDJUMPLOG.value), "fdjumplog_frozen": bool(model.FDJUMPLOG.frozen),
            "fdj_params_set": [n for n in model.params if is_fdj(n) and getattr(model, n).quantity is not None],
            "delay_funcs": [df.__name__ for df in model.delay_funcs]}


def forms():
    """What the reference does with the forms it rejects, ignores or rewrites."""
    base = wls_par()
    cases = {
        "index_21_pint": "FD21JUMP -fe L 1e-5 1\n",
        "index_21_tempo2": "FDJUMP21 -fe L 1e-5 1\n",
        "index_0": "FD0JUMP -fe L 1e-5\n",
        "index_20": "FD20JUMP -fe L 1e-9\n",
        # both spellings of one index: the lines of the spelling that appears first in the file are lost
        "mixed_spellings": "FD4JUMP -fe L 1e-7 1\nFDJUMP4 -fe S 2e-7 1\n",
        "mixed_spellings_reversed": "FDJUMP4 -fe S 2e-7 1\nFD4JUMP -fe L 1e-7 1\n",
        "fdjumplog_fit_flag": "FDJUMPLOG Y 1\n",
    }
    rec = {}
    for case, extra in cases.items():
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            try:
                m = get_model(io.StringIO(base + extra))
                got = {n: [getattr(m, n).key, [str(x) for x in getattr(m, n).key_value], float(getattr(m, n).value),
                           bool(getattr(m, n).frozen)]
                       for n in m.params if is_fdj(n) and n != "FDJUMPLOG" and getattr(m, n).quantity is not None}
                rec[case] = {"lines": extra, "result": "ok", "params": got, "order": list(got),
                             "fdjumplog": bool(m.FDJUMPLOG.value), "fdjumplog_free": "FDJUMPLOG" in m.free_params,
                             "warnings": sorted({str(x.message) for x in w if "parfile line" in str(x.message)})}
            except Exception as e:  # (recorded: the tests reproduce what the reference does)
                rec[case] = {"lines": extra, "result": type(e).__name__, "message": str(e)}
    return rec


def save(name, arrays, meta):
    """refcommon.save with the json written without indentation (two flag columns of 1000 entries
    would otherwise outgrow cm_gls.json)."""
    if "flags" in meta:
        refcommon.compact_flags(meta)
    meta["name"] = name
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **arrays)
    with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
        json.dump(meta, f, sort_keys=True, default=str)
        f.write("\n")
    for ext, ref in ((".npz", "cm_gls.npz"), (".json", "cm_gls.json")):
        sz, cap = os.path.getsize(os.path.join(GOLDEN, name + ext)), os.path.getsize(os.path.join(GOLDEN, ref))
        print(f"wrote {name}{ext}: {sz} B (cap {cap})", file=sys.stderr)
        assert sz <= cap, (name + ext, sz, cap)


def with_save(name, more_arrays, more_meta):
    def _save(_, arrays, meta):
        arrays = dict(arrays)
        arrays.update(more_arrays)
        meta = dict(meta)
        meta.update(more_meta)
        save(name, arrays, meta)
    gen_synth.save = _save


def parlines(model):
    # (the parameter lines only: the header names the run that wrote it)
    return "".join(l + "\n" for l in model.as_parfile().splitlines() if not l.startswith("#"))


def gen_wls():
    par, model, ts = build_wls()
    write_par("fdj_wls", par)
    f = pfit.WLSFitter(ts, copy.deepcopy(model))
    chi2 = f.fit_toas(maxiter=1)
    check_errors(f)
    p0 = f.model.FD1JUMP1
    print(f"  WLS chi2 {float(chi2):.3f}; FD1JUMP1 {p0.value:.5g} +- {p0.uncertainty_value:.3g}", file=sys.stderr)
    g0 = np.longdouble(p0.value) + np.linspace(-3, 3, 5) * np.longdouble(p0.uncertainty_value)
    g1 = np.longdouble(f.model.DM.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.DM.uncertainty_value)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more)
    more["grid_FD1JUMP1_hi"], more["grid_FD1JUMP1_lo"] = split_ld(g0)
    more["grid_DM_hi"], more["grid_DM_lo"] = split_ld(g1)
    fg = pfit.WLSFitter(ts, copy.deepcopy(f.model))
    c2, _ = grid_chisq(fg, ("FD1JUMP1", "DM"), (g0 * u.s, g1 * u.pc / u.cm ** 3), ncpu=1, printprogress=False)
    more["grid_chi2"] = np.asarray(c2, dtype=np.float64)
    print(f"  grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
    meta["wls_parfile"] = parlines(f.model)
    meta["forms"] = forms()
    tz = model.get_TZR_toa(ts)
    meta["tzr_selected_by"] = [n for n in meta["fdj_params_set"] if n != "FDJUMPLOG"
                               and len(getattr(model, n).select_toa_mask(tz)) > 0]
    assert meta["tzr_selected_by"] == ["FD1JUMP3"], meta["tzr_selected_by"]
    a, b = selected(model, ts, ["FD1JUMP3"]), selected(model, ts, ["FD1JUMP1", "FD1JUMP2"])
    assert (a & b).any()  # (the MJD-keyed FDJUMP overlaps the L and S ones)
    meta["down_fixed_point"] = fixed_point(model, ts, pfit.DownhillWLSFitter, pfit.WLSFitter)
    with_save("fdj_wls", more, meta)
    capture("fdj_wls", model, ts, fit="wls")


def gen_lin():
    par, model, ts = build_lin()
    write_par("fdj_lin", par)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more)
    # against the other FDJUMPLOG value on the same TOAs: more than 100 ns apart on the selected rows
    other = get_model(io.StringIO("".join(l for l in par.splitlines(True) if not l.startswith("FDJUMPLOG"))))
    assert bool(other.FDJUMPLOG.value) != bool(model.FDJUMPLOG.value)
    d_other = refcommon.component_delays(other, ts)["delay_fdjump_delay"]
    sel = selected(model, ts, fdj_names(model)[0])
    frac = float(np.mean(np.abs(d_other[sel] - more["fdjump_delay"][sel]) > 1e-7))
    assert frac >= 0.5, frac
    meta["log_vs_lin_over_100ns"] = frac
    with_save("fdj_lin", more, meta)
    capture("fdj_lin", model, ts, fit="wls")


def gen_gls():
    par, model, ts = build_gls()
    write_par("fdj_gls", par)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more)
    f = pfit.GLSFitter(ts, copy.deepcopy(model))
    f.fit_toas(maxiter=1)
    check_errors(f)
    meta["gls_parfile"] = parlines(f.model)
    meta["down_fixed_point"] = fixed_point(model, ts, pfit.DownhillGLSFitter, pfit.GLSFitter)
    with_save("fdj_gls", more, meta)
    capture("fdj_gls", model, ts, fit="gls")


def gen_spread(names):
    import gen_fit_spread
    path = os.path.join(GOLDEN, "fdj_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    todo = {"fdj_wls": (build_wls, "wls", pfit.DownhillWLSFitter), "fdj_gls": (build_gls, "gls", pfit.DownhillGLSFitter)}
    for n in names:
        build, fit, cls = todo[n]
        _, model, ts = build()
        gen_fit_spread.check_same(n, ts)
        res[n] = gen_fit_spread.measure(model, ts, fit, True)
        res[n]["downhill"] = downhill_spread(model, ts, cls)
        print(n, json.dumps(res[n]), file=sys.stderr, flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["fdj_wls", "fdj_lin", "fdj_gls", "spread"]
    if "find" in which:
        find_seed()
        sys.exit(0)
    if "order" in which:
        ok = all(order_ok(get_model(io.StringIO(p))) for p in (wls_par(), gls_par()))
        print("ORDER OK" if ok else "ORDER other")
        sys.exit(0)
    register_clockless_sites()
    if "fdj_wls" in which:
        gen_wls()
    if "fdj_lin" in which:
        gen_lin()
    if "fdj_gls" in which:
        gen_gls()
    if "spread" in which:
        gen_spread([n for n in ("fdj_wls", "fdj_gls") if n in which] or ["fdj_wls", "fdj_gls"])
