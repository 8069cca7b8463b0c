"""Golden fixtures for Polycos (reference run; container only; TEST INFRASTRUCTURE).
Reuses the committed generators under oracle/refgen as they are.

Offline recipe: register_clockless_sites(), EPHEM builtin, pint.toa.get_TOAs_array wrapped to force
include_bipm=False (generate_polycos does not pass it, and the default would fetch the BIPM table).

Cases (gen_synth.pta_par without its noise, DMX and JUMP lines):

* poly_bary  : isolated, "@", obsFreq 0, span 120 min, 10 coefficients, 20 nodes, MJD 55000.1-55000.6
               (7 segments), TZR lines removed (the add_tzr_toa path): photonphase --polycos' settings
* poly_gbt   : ELL1, gbt, 1400 MHz, 60 / 12 / 20, 55000.1-55000.3 (6 segments)
* poly_short : ELL1, gbt, 430 MHz, 15 / 8 / 20, 55000.1-55000.15 (5 segments)
* poly_long  : ELL1, geocenter, 1400 MHz, 720 / 15 / 40, 55000.1-55000.5 (2 segments)

Per case: the generated table (longdoubles as (hi, lo) pairs), the text the reference writes (from a
copy: its writer edits coeffs[0]), that text with the newline tempo puts after a last short coefficient
line and the reference's own parse of it, per segment np.polyfit's arguments (dtd, rdcPhased) and the
model.phase values of the mid-point and the nodes, the first segment's node TOAs (TDB, positions), 400
sorted check times (every t_start / t_stop the reference's find_entry accepts, the rest uniform in the
covered range, longdouble) with eval_abs_phase, the exact value of the same table (fractions.Fraction on
the stored longdoubles, rounded once), eval_spin_freq, eval_spin_freq_derivative and model.phase of
get_TOAs_array at those times; e_eval = max |eval_abs_phase - exact|, e_fit = max |eval_abs_phase -
model.phase|, and the reference's seconds per generate_polycos segment and per 1e5 eval_abs_phase times.
Also tests/datafile/B1855_polyco.dat (written by tempo) with the parsed table and 100 check times.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_polycos.py [case ...]
"""
import copy
import io
import os
import shutil
import sys
import tempfile
import time
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle", "refgen"))

import refcommon  # noqa: E402
from refcommon import GOLDEN, REFDATA, register_clockless_sites, pack_toas, split_ld  # noqa: E402
from gen_synth import pta_par  # noqa: E402
import pint.toa  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.polycos import Polycos  # noqa: E402

LD = np.longdouble
NCHECK = 400
CASES = {
    "poly_bary": dict(seed=61, binary="", obs="@", freq=0.0, span=120, ncoeff=10, nodes=20, start=55000.1, end=55000.6,
                      nseg=7, tzr=False),
    "poly_gbt": dict(seed=62, binary="ELL1", obs="gbt", freq=1400.0, span=60, ncoeff=12, nodes=20, start=55000.1,
                     end=55000.3, nseg=6, tzr=True),
    "poly_short": dict(seed=62, binary="ELL1", obs="gbt", freq=430.0, span=15, ncoeff=8, nodes=20, start=55000.1,
                       end=55000.15, nseg=5, tzr=True),
    "poly_long": dict(seed=62, binary="ELL1", obs="geocenter", freq=1400.0, span=720, ncoeff=15, nodes=40, start=55000.1,
                      end=55000.5, nseg=2, tzr=True),
}

_calls = []  # (times argument, TOAs) of every get_TOAs_array call
_orig_gta = pint.toa.get_TOAs_array


def _gta_nobipm(*a, **k):
    k["include_bipm"] = False
    t = _orig_gta(*a, **k)
    _calls.append(t)
    return t


pint.toa.get_TOAs_array = _gta_nobipm


def par_text(case):
    drop = ("TNRed", "DMX", "EFAC", "EQUAD", "JUMP") + (() if case["tzr"] else ("TZR",))
    out = []
    for line in pta_par(case["seed"], case["binary"]).splitlines():
        t = line.split()
        if not t or t[0].startswith(drop):
            continue
        out.append(line)
    return "\n".join(out) + "\n"


def frac_of(v):
    """The exact value of a longdouble."""
    hi, lo = split_ld(v)
    return Fraction(float(hi)) + Fraction(float(lo))


def frac_to_pair(x):
    hi = float(x)
    return hi, float(x - Fraction(hi))


def exact_phase(entry, t):
    """(integer, fraction hi, lo): the entry's polynomial at t in rational arithmetic, split once."""
    dt = (frac_of(t) - frac_of(entry.tmid.value)) * 1440
    p = Fraction(0)
    for c in entry.coeffs[::-1]:
        p = p * dt + frac_of(c)
    p += frac_of(entry.rphase.int[0].value) + frac_of(entry.rphase.frac[0].value) + 60 * frac_of(entry.f0) * dt
    k = (p + Fraction(1, 2)).__floor__()
    return (float(k),) + frac_to_pair(p - k)


def circ(ai, af, bi, bf):
    """|a - b| of phases given as (int, frac longdouble)."""
    return np.abs((LD(ai) - LD(bi)) + (LD(af) - LD(bf)))


def table_arrays(p, prefix):
    tab = p.polycoTable
    ents = list(tab["entry"])
    out = {}
    for k, v in (("tmid", [e.tmid.value for e in ents]), ("t_start", [e.tstart.value for e in ents]),
                 ("t_stop", [e.tstop.value for e in ents]), ("rph_frac", [e.rphase.frac[0].value for e in ents]),
                 ("f0", [e.f0 for e in ents]), ("coeffs", [np.asarray(e.coeffs, dtype=LD) for e in ents])):
        out[prefix + k + "_hi"], out[prefix + k + "_lo"] = split_ld(np.array(v, dtype=LD))
    out[prefix + "rph_int"] = np.array([float(e.rphase.int[0].value) for e in ents])
    out[prefix + "ncoeff"] = np.array([e.ncoeff for e in ents])
    meta = {k: [str(x) for x in tab[k]] for k in ("psr", "date", "obs")}
    meta.update({k: [float(x) for x in tab[k]] for k in ("utc", "dm", "doppler", "logrms", "obsfreq")})
    meta["mjd_span"] = [int(x) for x in tab["mjd_span"]]
    if "binary_phase" in tab.colnames:
        meta["binary_phase"] = [float(x) for x in tab["binary_phase"]]
        meta["f_orbit"] = [float(x) for x in tab["f_orbit"]]
    return out, meta


def write_text(p):
    """The file the reference writes, from copies of the entries (a deepcopy of the table shares them)."""
    q = Polycos()
    q.polycoTable = p.polycoTable.copy()
    q.polycoTable["entry"] = [copy.deepcopy(e) for e in p.polycoTable["entry"]]
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "polyco.dat")
        q.write_polyco_file(fn)
        return open(fn).read()


def check_times(p, n, rng):
    tab = p.polycoTable
    ts, te = np.asarray(tab["t_start"], dtype=LD), np.asarray(tab["t_stop"], dtype=LD)
    keep = []
    for t in np.concatenate([ts, te]):
        try:
            p.find_entry(np.array([t], dtype=LD))
            keep.append(t)
        except ValueError:
            pass
    while len(keep) < n:
        t = ts[0] + LD(rng.uniform()) * (te[-1] - ts[0]) + LD(rng.uniform(-1, 1)) * LD(1e-10)
        try:
            p.find_entry(np.array([t], dtype=LD))
            keep.append(t)
        except ValueError:
            pass
    return np.sort(np.array(keep, dtype=LD)), len(keep) - n


def evals(p, t, arrays, prefix=""):
    idx = p.find_entry(t)
    ph = p.eval_abs_phase(t)
    ri, rf = np.asarray(ph.int.value, dtype=np.float64), np.asarray(ph.frac.value, dtype=LD)
    ex = [exact_phase(p.polycoTable["entry"][i], x) for i, x in zip(idx, t)]
    ei = np.array([e[0] for e in ex])
    ef = np.array([LD(e[1]) + LD(e[2]) for e in ex], dtype=LD)
    arrays[prefix + "t_hi"], arrays[prefix + "t_lo"] = split_ld(t)
    arrays[prefix + "entry"] = np.asarray(idx)
    arrays[prefix + "ref_int"] = ri
    arrays[prefix + "ref_frac_hi"], arrays[prefix + "ref_frac_lo"] = split_ld(rf)
    arrays[prefix + "exact_int"] = ei
    arrays[prefix + "exact_frac_hi"] = np.array([e[1] for e in ex])
    arrays[prefix + "exact_frac_lo"] = np.array([e[2] for e in ex])
    arrays[prefix + "freq_hi"], arrays[prefix + "freq_lo"] = split_ld(np.asarray(p.eval_spin_freq(t), dtype=LD))
    arrays[prefix + "fdot_hi"], arrays[prefix + "fdot_lo"] = split_ld(np.asarray(p.eval_spin_freq_derivative(t), dtype=LD))
    return float(np.max(circ(ri, rf, ei, ef))), ri, rf


def gen(name):
    case = CASES[name]
    par = par_text(case)
    with open(os.path.join(GOLDEN, name + ".par"), "w") as f:
        f.write(par)
    model = get_model(io.StringIO(par))
    model.EPHEM.value = "builtin"
    assert ("AbsPhase" in model.components) == case["tzr"]
    phases, fits = [], []
    orig_phase, orig_polyfit = model.phase, np.polyfit

    def rec_phase(toas, abs_phase=None):
        ph = orig_phase(toas, abs_phase=abs_phase)
        phases.append((np.asarray(ph.int.value, dtype=np.float64), np.asarray(ph.frac.value, dtype=LD)))
        return ph

    def rec_polyfit(x, y, deg):
        fits.append((np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)))
        return orig_polyfit(x, y, deg)

    model.phase, np.polyfit = rec_phase, rec_polyfit
    del _calls[:]
    t0 = time.perf_counter()
    try:
        p = Polycos.generate_polycos(model, case["start"], case["end"], case["obs"], case["span"], case["ncoeff"],
                                     case["freq"], numNodes=case["nodes"], progress=False)
    finally:
        np.polyfit = orig_polyfit
        del model.phase
    sec_gen = (time.perf_counter() - t0) / len(p)
    nseg, nn, nc = len(p), case["nodes"], case["ncoeff"]
    assert nseg == case["nseg"] and len(fits) == nseg and len(phases) == 2 * nseg, (nseg, len(fits), len(phases))
    arrays, meta_tab = table_arrays(p, "")
    meta = {"name": name, "case": case, "table": meta_tab, "F0": float(model.F0.value),
            "tzrmjd": repr(float(model.TZRMJD.value)), "tzrsite": str(model.TZRSITE.value), "tzrfrq": str(model.TZRFRQ.value)}
    # what the writer gives (from a copy), and the same with tempo's newline after a short last line
    text = write_text(p)
    singles = []
    for i in range(nseg):
        q = Polycos()
        q.polycoTable = p.polycoTable[i:i + 1]
        singles.append(write_text(q))
    assert "".join(singles) == text
    text_nl = "".join(s if s.endswith("\n") else s + "\n" for s in singles)
    meta["text"], meta["text_nl"] = text, text_nl
    try:
        rd = Polycos.read(io.StringIO(text_nl))
    except ValueError as e:  # (a site name longer than the 5-character column runs into f0: poly_long)
        meta["rd_error"] = str(e)
    else:
        a2, m2 = table_arrays(rd, "rd_")
        arrays.update(a2)
        meta["rd_table"] = m2
    # the segments' fits and phases
    arrays["dtd"] = np.array([f[0] for f in fits])
    arrays["rdc"] = np.array([f[1] for f in fits])
    arrays["mid_int"] = np.array([phases[2 * s][0][0] for s in range(nseg)])
    arrays["mid_frac_hi"], arrays["mid_frac_lo"] = split_ld(np.array([phases[2 * s][1][0] for s in range(nseg)], dtype=LD))
    arrays["node_int"] = np.array([phases[2 * s + 1][0] for s in range(nseg)])
    arrays["node_frac_hi"], arrays["node_frac_lo"] = split_ld(np.array([phases[2 * s + 1][1] for s in range(nseg)], dtype=LD))
    tmids = np.array([e.tmid.value for e in p.polycoTable["entry"]], dtype=LD)
    dt = np.array([(np.linspace(tm - LD(case["span"]) / 1440 / 2, tm + LD(case["span"]) / 1440 / 2, nn) - tm) * LD(1440.0)
                   for tm in tmids], dtype=LD)
    assert np.array_equal(dt.astype(np.float64), arrays["dtd"])
    arrays["dt_hi"], arrays["dt_lo"] = split_ld(dt)
    first_nodes = [c for c in _calls if c.ntoas == nn][0]
    pk, _ = pack_toas(first_nodes)
    arrays.update({"n0_" + k: v for k, v in pk.items()})
    # check times
    rng = np.random.default_rng(case["seed"])
    t, _ = check_times(p, NCHECK, rng)
    e_eval, ri, rf = evals(p, t, arrays)
    ts = pint.toa.get_TOAs_array(t, case["obs"], freqs=case["freq"], ephem="builtin")
    mp = model.phase(ts, abs_phase=True)
    mi, mf = np.asarray(mp.int.value, dtype=np.float64), np.asarray(mp.frac.value, dtype=LD)
    arrays["model_int"] = mi
    arrays["model_frac_hi"], arrays["model_frac_lo"] = split_ld(mf)
    e_fit = float(np.max(circ(ri, rf, mi, mf)))
    big = np.sort(LD(rng.uniform(size=100000)) * (t[-1] - t[0]) + t[0])
    t0 = time.perf_counter()
    p.eval_abs_phase(big)
    sec_eval = time.perf_counter() - t0
    meta.update({"e_eval": e_eval, "e_fit": e_fit, "ref_seconds_per_segment": sec_gen, "ref_seconds_per_1e5_eval": sec_eval,
                 "n_boundary_times": int(np.sum(np.isin(t, np.concatenate([p.polycoTable["t_start"], p.polycoTable["t_stop"]]))))})
    print(f"{name}: {nseg} segments; e_eval {e_eval:.3g}; e_fit {e_fit:.3g}; {sec_gen:.2f} s per segment; "
          f"{sec_eval:.2f} s per 1e5 times; TZRMJD {meta['tzrmjd']}", file=sys.stderr)
    refcommon.save(name, arrays, meta)


def gen_b1855():
    name = "B1855_polyco.dat"
    shutil.copyfile(os.path.join(REFDATA, name), os.path.join(GOLDEN, name))
    p = Polycos.read(os.path.join(REFDATA, name))
    arrays, meta_tab = table_arrays(p, "")
    rng = np.random.default_rng(1855)
    t, _ = check_times(p, 100, rng)
    e_eval, _, _ = evals(p, t, arrays)
    meta = {"name": "poly_b1855", "table": meta_tab, "e_eval": e_eval}
    print(f"poly_b1855: {len(p)} entries; e_eval {e_eval:.3g}", file=sys.stderr)
    refcommon.save("poly_b1855", arrays, meta)


if __name__ == "__main__":
    register_clockless_sites()
    names = sys.argv[1:] or list(CASES) + ["b1855"]
    for nm in names:
        gen_b1855() if nm == "b1855" else gen(nm)
