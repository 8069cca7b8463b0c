"""Polycos on the host (no GPU): the tempo reader and writer, find_entry, the longdouble evaluation
(device=False) and get_TOAs_array, against the reference's values in tests/golden/poly_*.{npz,json}
(scripts/refgen/gen_polycos.py) and the reference's own test file B1855_polyco.dat (written by tempo)."""
import io
import json
import os

import numpy as np
import pytest

from pint_amd import get_model
from pint_amd.polycos import Phase, PolycoEntry, Polycos, split_pairs

LD = np.longdouble
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["poly_bary", "poly_gbt", "poly_short", "poly_long"]
READABLE = ["poly_bary", "poly_gbt", "poly_short"]  # (poly_long's site name runs into f0: the reference cannot read it)


def load(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    with open(os.path.join(GOLD, name + ".json")) as f:
        return z, json.load(f)


def pair(z, k):
    return z[k + "_hi"].astype(LD) + z[k + "_lo"].astype(LD)


def table_from(z, meta, prefix=""):
    """A Polycos from a stored table (longdoubles from their pairs)."""
    rows = []
    tab = meta["rd_table" if prefix else "table"]
    co = pair(z, prefix + "coeffs")
    for k in range(len(z[prefix + "rph_int"])):
        e = PolycoEntry(pair(z, prefix + "tmid")[k], tab["mjd_span"][k], z[prefix + "rph_int"][k],
                        pair(z, prefix + "rph_frac")[k], pair(z, prefix + "f0")[k], int(z[prefix + "ncoeff"][k]), co[k])
        row = {c: tab[c][k] for c in ("psr", "date", "utc", "dm", "doppler", "logrms", "mjd_span", "obs", "obsfreq")}
        row.update(tmid=e.tmid, t_start=e.tstart, t_stop=e.tstop)
        if "binary_phase" in tab:
            row.update(binary_phase=tab["binary_phase"][k], f_orbit=tab["f_orbit"][k])
        row["entry"] = e
        rows.append(row)
    return Polycos.from_table(rows)


def assert_table(p, z, tab, prefix=""):
    ents = list(p["entry"])
    assert len(p) == len(z[prefix + "rph_int"])
    for k, want in (("tmid", [e.tmid for e in ents]), ("t_start", p["t_start"]), ("t_stop", p["t_stop"]),
                    ("f0", [e.f0 for e in ents]), ("rph_frac", [e.rphase.frac[0] for e in ents])):
        assert np.array_equal(np.array(want, dtype=LD), pair(z, prefix + k)), k  # to the last longdouble bit
    assert np.array_equal(np.array([e.rphase.int[0] for e in ents], dtype=np.float64), z[prefix + "rph_int"])
    assert np.array_equal(np.array([e.coeffs for e in ents], dtype=LD), pair(z, prefix + "coeffs"))
    assert [e.ncoeff for e in ents] == list(z[prefix + "ncoeff"])
    for c in ("psr", "date", "obs"):
        assert [str(x) for x in p[c]] == tab[c], c
    for c in ("utc", "dm", "doppler", "logrms", "mjd_span", "obsfreq") + (("binary_phase", "f_orbit") if "f_orbit" in tab else ()):
        assert list(p[c]) == tab[c], c
    assert ("binary_phase" in p.polycoTable.colnames) == ("binary_phase" in tab)


def test_read_b1855():
    z, meta = load("poly_b1855")
    p = Polycos.read(os.path.join(GOLD, "B1855_polyco.dat"))
    assert_table(p, z, meta["table"])
    assert len(p) == 8 and p[0]["entry"] is p["entry"][0] and len(p["t_start"]) == 8


@pytest.mark.parametrize("name", READABLE)
def test_read_case_text(name):
    z, meta = load(name)
    assert_table(Polycos.read(io.StringIO(meta["text_nl"])), z, meta["rd_table"], "rd_")


def test_read_long_site_name_fails_as_the_reference():
    _, meta = load("poly_long")
    assert "rd_error" in meta
    with pytest.raises(ValueError):
        Polycos.read(io.StringIO(meta["text_nl"]))


@pytest.mark.parametrize("name", CASES)
def test_write_reproduces_the_reference_text(name):
    z, meta = load(name)
    p = table_from(z, meta)
    before = [np.array(e.coeffs) for e in p["entry"]]
    out = io.StringIO()
    p.write_polyco_file(out)
    nc = meta["case"]["ncoeff"]
    if nc % 3 == 0:  # 12 and 15: byte for byte
        assert out.getvalue() == meta["text"]
    assert out.getvalue() == meta["text_nl"]  # 8 and 10: every byte, plus tempo's newline after the last short line
    assert meta["text_nl"].replace("\n", "") == meta["text"].replace("\n", "") and len(meta["text_nl"]) - len(meta["text"]) == (
        len(p) if nc % 3 else 0)
    out2 = io.StringIO()
    p.write_polyco_file(out2)  # a second write gives the same file: the caller's coefficients are left alone
    assert out2.getvalue() == out.getvalue()
    assert all(np.array_equal(a, e.coeffs) for a, e in zip(before, p["entry"]))
    if name in READABLE:
        assert_table(Polycos.read(io.StringIO(out.getvalue())), z, meta["rd_table"], "rd_")


def test_write_file_and_formats(tmp_path):
    z, meta = load("poly_gbt")
    p = table_from(z, meta)
    fn = tmp_path / "polyco.dat"
    p.write_polyco_file(fn)
    assert fn.read_text() == meta["text"]
    assert len(Polycos.read(str(fn))) == len(p)
    with pytest.raises(ValueError, match="Unknown polyco file format"):
        p.write_polyco_file(fn, format="tempo2")
    with pytest.raises(ValueError, match="Unknown polyco file format"):
        Polycos.read(str(fn), format="psrfits")
    with pytest.raises(DeprecationWarning):
        p.read_polyco_file(str(fn))


@pytest.mark.parametrize("name", CASES + ["poly_b1855"])
def test_find_entry(name):
    z, meta = load(name)
    p = Polycos.read(os.path.join(GOLD, "B1855_polyco.dat")) if name == "poly_b1855" else table_from(z, meta)
    t = pair(z, "t")
    assert np.array_equal(p.find_entry(t), z["entry"])
    ts, te = p["t_start"], p["t_stop"]
    for k in range(1, len(p)):  # a boundary shared by two entries belongs to the earlier one
        if te[k - 1] == ts[k]:
            assert p.find_entry(ts[k])[0] == k - 1
    assert p.find_entry(te[-1])[0] == len(p) - 1
    for bad in (ts[0], ts[0] - LD(1e-9), te[-1] + LD(1e-9), LD(0.0)):  # the first t_start itself is not covered
        with pytest.raises(ValueError, match="Some input times not covered by Polyco entries."):
            p.find_entry(bad)
    with pytest.raises(ValueError, match="not covered"):
        p.find_entry(np.array([ts[0] + LD(1e-6), te[-1] + LD(1.0)]))
    assert p.find_entry(float(ts[0]) + 1e-6)[0] == 0 and p.find_entry([float(ts[0]) + 1e-6])[0] == 0


def test_find_entry_b1855_gaps():
    """tempo's 11-decimal TMIDs leave gaps and overlaps of some 1e-11 day between neighbouring entries
    (7e-11 and -3e-11 day here): a time inside either is not covered, as in the reference."""
    p = Polycos.read(os.path.join(GOLD, "B1855_polyco.dat"))
    ts, te = p["t_start"], p["t_stop"]
    d = [float(ts[k] - te[k - 1]) for k in range(1, len(p))]
    gaps = [k for k in range(1, len(p)) if 0 < d[k - 1] < 1e-10]
    laps = [k for k in range(1, len(p)) if -1e-10 < d[k - 1] < 0]
    assert gaps and laps
    for k in gaps + laps:
        a, b = sorted((te[k - 1], ts[k]))
        mid = a + (b - a) / 2
        assert a < mid < b
        with pytest.raises(ValueError, match="not covered"):
            p.find_entry(mid)
    for k in gaps:
        with pytest.raises(ValueError, match="not covered"):
            p.find_entry(ts[k])  # (count(t_start < t) - 1 is k - 1 there, count(t_stop < t) is k)
        assert p.find_entry(te[k - 1])[0] == k - 1
    for k in laps:
        assert p.find_entry(ts[k])[0] == k - 1  # the start of the overlap still belongs to the earlier entry


@pytest.mark.parametrize("name", CASES + ["poly_b1855"])
def test_host_evaluation(name):
    z, meta = load(name)
    p = Polycos.read(os.path.join(GOLD, "B1855_polyco.dat")) if name == "poly_b1855" else table_from(z, meta)
    t = pair(z, "t")
    ph = p.eval_abs_phase(t, device=False)
    assert ph.int.dtype == LD and np.all((ph.frac >= -0.5) & (ph.frac < 0.5))
    d_ref = np.abs((ph.int - z["ref_int"]) + (ph.frac - pair(z, "ref_frac")))
    d_exact = np.abs((ph.int - z["exact_int"]) + (ph.frac - pair(z, "exact_frac")))
    print(f"{name}: |host - reference| {float(d_ref.max()):.3g}, |host - exact| {float(d_exact.max()):.3g}, "
          f"e_eval {meta['e_eval']:.3g}")
    assert d_ref.max() <= 2 * meta["e_eval"]
    assert d_exact.max() <= 2 * meta["e_eval"]
    assert np.array_equal(p.eval_phase(t, device=False), ph.frac)
    perm = np.random.default_rng(3).permutation(len(t))  # input order is kept
    q = p.eval_abs_phase(t[perm], device=False)
    assert np.array_equal(q.int, ph.int[perm]) and np.array_equal(q.frac, ph.frac[perm])
    f, fd = p.eval_spin_freq(t, device=False), p.eval_spin_freq_derivative(t, device=False)
    assert np.max(np.abs(f - pair(z, "freq")) / np.abs(f)) < 4 * np.finfo(LD).eps
    scale = np.max(np.abs(pair(z, "fdot")))
    assert np.max(np.abs(fd - pair(z, "fdot"))) <= 64 * np.finfo(LD).eps * scale
    one = p.eval_abs_phase(float(t[5]), device=False)  # a scalar float64 time
    assert one.int.shape == (1,)


def test_entry_methods_and_phase():
    z, meta = load("poly_gbt")
    p = table_from(z, meta)
    e = p[2]["entry"]
    assert e.tstart == e.tmid - e.mjdspan / 2 and e.tstop == e.tmid + e.mjdspan / 2 and float(e.mjdspan) * 1440 == 60
    t = pair(z, "t")[z["entry"] == 2]
    a = e.evalabsphase(t)
    assert np.array_equal(e.evalphase(t), a.frac)
    h = LD(1e-3) / 1440  # the frequency is the derivative of the phase: a central difference in dt agrees
    num = ((e.evalabsphase(t + h) - e.evalabsphase(t - h)).value / (2 * LD(1e-3) * 60))
    assert np.max(np.abs(num - e.evalfreq(t))) < 1e-6
    x = Phase(LD(3.75))
    assert x.int[0] == 4 and x.frac[0] == -0.25
    y = Phase(LD(-1.0), LD(-0.5))
    assert y.int[0] == -1 and y.frac[0] == -0.5
    hi, lo = split_pairs(np.array([LD(55000) + LD(1) / 3]))
    assert LD(hi[0]) + LD(lo[0]) == LD(55000) + LD(1) / 3 and abs(lo[0]) <= np.spacing(hi[0]) / 2


@pytest.mark.parametrize("name", CASES)
def test_get_toas_array_nodes(name):
    """get_TOAs_array at the first segment's nodes, handed over as generate_polycos does ((fraction,
    integer) parts): TDB and positions at the bars tests/test_prep.py holds prep.prepare to."""
    from pint_amd.toa import get_TOAs_array
    import pint_amd
    assert pint_amd.get_TOAs_array is get_TOAs_array
    z, meta = load(name)
    case = meta["case"]
    tm = pair(z, "tmid")[0]
    span = LD(case["span"]) / 1440
    nodes = np.linspace(tm - span / 2, tm + span / 2, case["nodes"])
    fr, ip = np.modf(nodes)
    model = get_model(os.path.join(GOLD, name + ".par"))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (no clock files for gbt: as the fixture was made)
        t = get_TOAs_array((fr, ip), case["obs"], freqs=case["freq"], model=model, include_bipm=False)
    assert t.ntoas == case["nodes"] and t.prepared is not None
    tdb = t.tdbld
    assert float(np.max(np.abs(tdb - pair(z, "n0_tdb")))) * 86400 < 1e-9
    for k, tol in (("ssb_obs_pos_km", 1e-4), ("obs_sun_pos_km", 1e-4), ("ssb_obs_vel_kms", 1e-9)):
        assert np.max(np.abs(t.arrays[k] - z["n0_" + k])) < tol, k
    assert np.array_equal(t.arrays["freq_mhz"], z["n0_freq_mhz"])  # (obsFreq 0: infinite frequency)
    assert np.array_equal(t.arrays["is_bary"], z["n0_is_bary"])
    # the same times as one longdouble array, and as float64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        t2 = get_TOAs_array(nodes, case["obs"], freqs=case["freq"], include_bipm=False, ephem="builtin")
        t3 = get_TOAs_array(nodes.astype(np.float64), case["obs"], errors=2.0, flags={"be": "X"}, include_bipm=False)
    assert float(np.max(np.abs(t2.tdbld - tdb))) * 86400 < 1e-9
    assert float(np.max(np.abs(t3.tdbld - tdb))) * 86400 < 1e-6 and np.all(t3.get_errors() == 2.0)
    assert t3.flag_columns["be"] == ("X",) * case["nodes"]
    with pytest.raises(NotImplementedError):
        get_TOAs_array(nodes, case["obs"], include_bipm=True)
    with pytest.raises(AttributeError):
        get_TOAs_array(nodes, case["obs"], freqs=[1.0, 2.0], include_bipm=False)


def test_generate_argument_errors():
    model = get_model(os.path.join(GOLD, "poly_gbt.par"))
    with pytest.raises(ValueError, match="Maximum hour angle != 12.0 is not supported."):
        Polycos.generate_polycos(model, 55000.1, 55000.3, "gbt", 60, 12, 1400.0, maxha=6.0)
    with pytest.raises(NotImplementedError, match="Only TEMPO method has been implemented."):
        Polycos.generate_polycos(model, 55000.1, 55000.3, "gbt", 60, 12, 1400.0, method="CHEBY")
    with pytest.raises(ValueError, match="at most 16 coefficients"):
        Polycos.generate_polycos(model, 55000.1, 55000.3, "gbt", 60, 17, 1400.0)


def test_add_tzr_to_a_model_without_one():
    """A model without TZRMJD ends with the reference's: the first segment's mid-point as a float64 MJD,
    at the barycenter, at infinite frequency."""
    z, meta = load("poly_bary")
    model = get_model(os.path.join(GOLD, "poly_bary.par"))
    assert "TZRMJD" not in model
    Polycos._add_tzr(model, pair(z, "tmid")[0])
    assert "AbsPhase" in model.components
    assert repr(float(model.TZRMJD.value)) == meta["tzrmjd"]
    assert str(model.TZRSITE.value) == meta["tzrsite"] == "ssb"
    assert str(float(model.TZRFRQ.value)) == meta["tzrfrq"] == "inf"
