"""Golden fixtures for the orbital-frequency (FB0 ... FBn) binary orbits (reference run; container
only; TEST INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* fbx_ell1_wls, fbx_ell1h_wls, fbx_dd_wls, fbx_bt_wls : WLS.  gen_binaries' isolated-pulsar base
            with the binary block, FB0 ... FB2 in place of PB, 300 TOAs at 1400 / 800 MHz from the
            geocentre over MJD 54500-55600, 1 us errors (300 rows: a partial second 256-thread
            block).  FB0 ... FB2 and every other binary parameter of the block are free.  The start
            is moved off the truth as in gen_binaries.build.  Beside what gen_synth.capture
            records: the post-fit as_parfile(), the TZR TOA's binary delay, and, in fbx_ell1_wls,
            the "forms" (what the reference does with the par lines it rejects, rewrites or ignores)
            and a 3x3 grid_chisq over (FB0, FB1) on the reference's executor path.
* fbx_ell1_gls, fbx_dd_gls : GLS.  gen_synth.pta_par(seed, "") (DMX, PLRedNoise, EFAC/EQUAD) with
            the binary block and FB0 ... FB3, 1000 TOAs in four bands.
* fbx_fit_spread.json : gen_fit_spread.measure of the six fixtures plus the Downhill spread, in
            bin_fit_spread.json's schema.

One derivative defect of the reference is corrected in this process (PATCHES): with OrbitFBX the T0
column of DD and BT is identically zero, because OrbitFBX has no d_orbits_d_T0 (so
Orbit.d_orbits_d_par returns zeros), its d_pbprime_d_par knows the FBn alone, and T0 is not among
its orbit_params.  Every fixture names the correction ("reference_patches"), the DD / BT ones
keep the as-is T0 column beside the corrected one (asis_col_T0), and `verify` asserts that nothing
else moves and that the corrected column agrees with the reference's numerical derivative while
the as-is one does not.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_fbx.py [fbx_ell1_wls ... fbx_dd_gls spread]
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
import pint.simulation as sim  # noqa: E402
import pint.fitter as pfit  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.gridutils import grid_chisq  # noqa: E402
from pint.utils import taylor_horner_deriv  # noqa: E402
from pint.models.stand_alone_psr_binaries.binary_orbits import OrbitFBX  # noqa: E402

from gen_solar_wind import write_par, downhill_spread  # noqa: E402
from gen_chromatic import check_errors  # noqa: E402
from gen_fdjump import parlines  # noqa: E402
from gen_binaries import BASE, binary_free, fixed_point, with_save  # noqa: E402
import gen_fit_spread  # noqa: E402  (replaces gen_synth.capture: `capture` above is the real one)

PATCHES = {
    "OrbitFBX.d_orbits_d_T0": "added: -2 pi sum_n FBn tt0^n / n! (rad / s)",
    "OrbitFBX.d_pbprime_d_par": "T0: -pbdot_orbit() (the FBn as before, every other parameter zero as before)",
    "OrbitFBX.orbit_params": "T0 appended, as OrbitPB has it",
}
_ASIS = (OrbitFBX.__init__, OrbitFBX.d_pbprime_d_par)


def _init(self, parent, orbit_params=("FB0",)):
    _ASIS[0](self, parent, list(orbit_params))
    self.orbit_params = list(self.orbit_params) + ["T0"]


def _d_orbits_d_T0(self):
    return -taylor_horner_deriv(self.tt0, self._FBXs(), 1) * 2 * np.pi * u.rad


def _d_pbprime_d_par(self, par):
    if par == "T0":
        return -self.pbdot_orbit()
    return _ASIS[1](self, par)


def patch(on=True):
    if on:
        OrbitFBX.__init__, OrbitFBX.d_pbprime_d_par, OrbitFBX.d_orbits_d_T0 = _init, _d_pbprime_d_par, _d_orbits_d_T0
    else:
        OrbitFBX.__init__, OrbitFBX.d_pbprime_d_par = _ASIS
        if "d_orbits_d_T0" in OrbitFBX.__dict__:
            del OrbitFBX.d_orbits_d_T0


FB0_03D = "3.858024691358024691e-05"      # 1 / (0.3 d)
FB0_DD = "7.542609117818283e-06"          # 1 / (1.53449474406 d)
FBS = "FB0 {fb0} 1\nFB1 -3e-19 1\nFB2 2e-27 1\n"
ELL1_BLOCK = "A1 1.9 1\nTASC {t0} 1\nEPS1 1e-3 1\nEPS2 -2e-3 1\n"
DD_BLOCK = "A1 9.2307805 1\nT0 {t0} 1\nECC 0.17 1\nOM 110.0 1\nOMDOT 0.01 1\nGAMMA 1e-4 1\n"
BLOCKS = {
    "ELL1": "BINARY ELL1\n" + FBS.format(fb0=FB0_03D) + ELL1_BLOCK + "M2 0.3 1\nSINI 0.97 1\n",
    "ELL1H": "BINARY ELL1H\n" + FBS.format(fb0=FB0_03D) + ELL1_BLOCK + "H3 1.2e-6 1\nSTIGMA 0.75 1\n",
    "DD": "BINARY DD\n" + FBS.format(fb0=FB0_DD) + DD_BLOCK + "M2 0.3 1\nSINI 0.95 1\n",
    "BT": "BINARY BT\n" + FBS.format(fb0=FB0_DD) + DD_BLOCK,
}
FB3 = "FB3 3e-35 1\n"
FIXTURES = {"fbx_ell1_wls": ("ELL1", "wls", 91), "fbx_ell1h_wls": ("ELL1H", "wls", 92),
            "fbx_dd_wls": ("DD", "wls", 93), "fbx_bt_wls": ("BT", "wls", 94),
            "fbx_ell1_gls": ("ELL1", "gls", 33), "fbx_dd_gls": ("DD", "gls", 34)}
T0_MODELS = ("DD", "BT")


@contextlib.contextmanager
def as_is():
    patch(False)
    try:
        yield
    finally:
        patch(True)


def true_par(binary, fit, seed):
    if fit == "wls":
        return BASE + BLOCKS[binary].format(t0="55000.123")
    return pta_par(seed, "") + BLOCKS[binary].format(t0="54801.987654321") + FB3


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
    """gen_binaries.build for these blocks: TOAs simulated from the true model, the start the truth
    with the free binary parameters moved together, inside their 1-sigma ellipsoid and by at most
    1e-3 of each value (FB0 by far less: it is known to 1e-12 or so of its value)."""
    binary, fit, seed = FIXTURES[name]
    par = true_par(binary, fit, seed)
    true = get_model(io.StringIO(par))
    ts = make_toas(true, fit, seed)
    if fit == "gls":
        true.find_empty_masks(ts, freeze=True)
    f = (pfit.GLSFitter if fit == "gls" else pfit.WLSFitter)(ts, copy.deepcopy(true))
    f.fit_toas(maxiter=1)
    names = list(f.parameter_covariance_matrix.get_label_names(axis=0))
    C = np.asarray(f.parameter_covariance_matrix.matrix, dtype=np.float64)
    free = binary_free(true)
    idx = [names.index(p) for p in free]
    D = np.sqrt(np.diag(C))
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


def verify(par, model, ts, binary, fit):
    """The assertions on the correction; returns the as-is T0 column and the recorded figures."""
    M, names, _ = model.designmatrix(ts)
    names = list(names)
    d1 = model.delay(ts).to_value(u.s)
    with as_is():
        m0 = get_model(io.StringIO(par))  # (the orbit object is made by setup(): built again, as-is)
        if fit == "gls":
            m0.find_empty_masks(ts, freeze=True)
        M0, names0, _ = m0.designmatrix(ts)
        d0 = m0.delay(ts).to_value(u.s)
        a0 = m0.d_delay_d_param(ts, "T0").value if binary in T0_MODELS else None
    assert list(names0) == names and np.array_equal(d0, d1)
    col = "T0" if binary in T0_MODELS else None
    for j, n in enumerate(names):
        if n != col:
            assert np.array_equal(M[:, j], M0[:, j]), n  # nothing else moves
    rec, arrays = {}, {}
    if col is not None:
        j = names.index(col)
        arrays["asis_col_T0"] = np.asarray(M0[:, j], dtype=np.float64)
        a = model.d_delay_d_param(ts, col).value
        # (the step is relative to T0's value, an MJD: 2e-10 of it is 1e-5 d, about a second, far
        # below the orbital period; gen_binaries' 1e-4 would be 5.5 d, several orbits)
        num = model.d_delay_d_param_num(ts, col, step=2e-10).value
        err = float(np.max(np.abs(num - a)) / np.max(np.abs(num)))
        err0 = float(np.max(np.abs(num - a0)) / np.max(np.abs(num)))
        print(f"  T0: corrected column vs numerical {err:.2e} of its maximum (as-is {err0:.2e}; as-is max "
              f"{np.max(np.abs(a0)):.3g}, numerical max {np.max(np.abs(num)):.3g})", file=sys.stderr)
        rec = {"column": col, "num_rel_err": err, "asis_num_rel_err": err0, "asis_max": float(np.max(np.abs(a0))),
               "num_max": float(np.max(np.abs(num)))}
        assert err0 > 1e-2, err0
        if binary == "BT":
            # BT_model.d_BTdelay_d_par leaves delayR's own derivatives out for every parameter (its
            # ECC column is off with either orbit form): what the corrected chain reaches is recorded
            rec["note"] = "BT's chain ignores d delayR / d par for every parameter; the figure is what it reaches"
            assert err < 1e-2, err
        else:
            assert err < 1e-4, err
    for n in binary_free(model):
        assert np.max(np.abs(M[:, names.index(n)])) > 0, n
    return arrays, rec


def forms():
    """What the reference does with the FBn par lines it rejects, rewrites or ignores."""
    base = true_par("ELL1", "wls", 0)

    def less(text, *names):
        return "".join(l + "\n" for l in text.splitlines() if l.split()[0] not in names)
    fb20 = less(base, "FB1", "FB2") + "".join(f"FB{n} {'-3e-19' if n == 1 else ('2e-27' if n == 2 else '0.0')}\n"
                                                for n in range(1, 20))
    cases = {
        "no_fb0": less(base, "FB0"),
        "gap": less(base, "FB1"),
        "fb0_negative": base.replace("FB0 " + FB0_03D, "FB0 -" + FB0_03D),
        "fb0_zero": base.replace("FB0 " + FB0_03D, "FB0 0.0"),
        "fb0_and_pb": base + "PB 0.3\n",
        "alias_fb": base.replace("FB0 ", "FB "),
        "alias_fb_alone": less(base, "FB1", "FB2").replace("FB0 ", "FB "),
        "fb0_alone": less(base, "FB1", "FB2"),
        "pbdot_beside_fb0": base + "PBDOT 1e-11 1\n",
        "fb20": fb20,
        "no_fbn": less(base, "FB0", "FB1", "FB2") + "PB 0.3 1\n",
    }
    ts = None
    rec = {}
    for case, text in cases.items():
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            try:
                m = get_model(io.StringIO(text))
                comp = [c for n, c in m.components.items() if n.startswith("Binary")][0]
                vals = {}
                for n in comp.params:
                    v = getattr(m, n).value
                    vals[n] = None if v is None else (str(v) if isinstance(v, (str, bool)) else float(v))
                rec[case] = {"result": "ok", "binary_params": list(comp.params), "values": vals,
                             "free": [n for n in m.free_params if n in comp.params],
                             "orbit": type(comp.binary_instance.orbits_cls).__name__,
                             "warnings": sorted({str(x.message) for x in w if "parfile line" in str(x.message)})}
                if ts is None:
                    np.random.seed(5)
                    ts = sim.make_fake_toas_uniform(54500, 55600, 40, m, freq=np.array([1400.0]) * u.MHz,
                                                    obs="geocenter", error=1 * u.us, include_bipm=False)
                if case in ("pbdot_beside_fb0", "fb20", "gap", "alias_fb_alone"):
                    # (gap: OrbitFBX's check sees no index, every FBn being in the list it is given,
                    # and its sums stop at the first missing index, so FB2 plays no part)
                    other = cases["fb0_alone"] if case in ("gap", "alias_fb_alone") else base
                    d = refcommon.component_delays(m, ts)["delay_binarymodel_delay"]
                    ref = refcommon.component_delays(get_model(io.StringIO(other)), ts)["delay_binarymodel_delay"]
                    rec[case]["binary_delay_equals"] = ["fb0_alone" if other is not base else "base",
                                                        bool(np.array_equal(d, ref))]
                if case == "pbdot_beside_fb0":
                    rec[case]["PBDOT_column_max"] = float(np.max(np.abs(m.d_delay_d_param(ts, "PBDOT").value)))
            except Exception as e:  # (recorded: the tests reproduce what the reference does)
                rec[case] = {"result": type(e).__name__, "message": str(e)}
        rec[case]["par"] = text
    return rec


def gen(name):
    binary, fit, _ = FIXTURES[name]
    par, model, ts = build(name)
    write_par(name, par)
    more, rec = verify(par, model, ts, binary, fit)
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
    # (PulsarBinary.pb() is not recorded: with FBn it divides by a sum of uncertainties.ufloat, and the
    # reference environment's stand-in for that package has no arithmetic)
    meta["down_fixed_point"] = fixed_point(model, ts, dcls, fcls)
    if name == "fbx_ell1_wls":
        meta["forms"] = forms()
        # a 3x3 grid over (FB0, FB1), +-1 sigma about the start, on the reference's executor path
        # (ncpu=2: every point fitted on a copy of the base model, as the device's batch of
        # independent points is; gen_binaries.gen)
        f1 = pfit.WLSFitter(ts, copy.deepcopy(model))
        f1.fit_toas(maxiter=1)
        axes = []
        for n in ("FB0", "FB1"):
            p = getattr(f1.model, n)
            axes.append(np.longdouble(getattr(model, n).value) + np.linspace(-1, 1, 3) * np.longdouble(p.uncertainty_value))
        fg = pfit.WLSFitter(ts, copy.deepcopy(model))
        c2 = np.asarray(grid_chisq(fg, ("FB0", "FB1"), (axes[0] * u.Hz, axes[1] * u.Hz / u.s), ncpu=2,
                                   printprogress=False)[0], dtype=np.float64)
        for n, g in zip(("FB0", "FB1"), axes):
            more[f"grid_{n}_hi"], more[f"grid_{n}_lo"] = split_ld(g)
        more["grid_chi2"] = c2
        meta["grid_params"] = ["FB0", "FB1"]
        print(f"  grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
        assert np.all(np.isfinite(c2))
    with_save(name, more, meta)
    capture(name, model, ts, fit=fit)


def gen_spread(names):
    path = os.path.join(GOLDEN, "fbx_fit_spread.json")
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
