"""Polycos on the device: k_polyco_eval, k_polyco_fit, k_polyco_trig and generate_polycos, against the
reference's values in tests/golden/poly_*.{npz,json} (scripts/refgen/gen_polycos.py).

Bars.  e_eval and e_fit are the reference's own recorded errors (its eval_abs_phase against the exact
value of the same table; its polyco against its own model phase).
  evaluation   |device - exact| <= e_eval + 2^-53 (the device must not be worse than the reference's
               longdouble arithmetic; 2^-53 is half an ulp of the float64 fraction it returns), and
               |device - reference| <= 2 e_eval + 2^-53; frequency and derivative within 8 float64 ulps.
  solver       max |P_dev - P_exact| <= 16 max |P_polyfit - P_exact| + 2^-50 max |y| on 101 points of the
               segment, P_exact the rational least-squares solution of the same float64 data: np.polyfit
               is the reference's solver, so its error is measured here; two backward-stable solvers
               scatter by about an order of magnitude around eps cond, normal equations by cond^2.
  end to end   |device polyco - reference model phase| <= e_fit + Lambda (1 ns F0 + 8 longdouble ulps of
               the absolute phase), Lambda the max-norm gain of the least-squares fit on the nodes (from the
               hat matrix), the bracket the standing bar of the absolute-phase tests.
  sums         tests/test_photon.py's: harmonic j 16 (j + log2 n) eps sum |w|, the weight sums 16 log2 n eps
               x the sum, against trig_numpy on the device's own phases read back through eval_phase.
"""
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

from pint_amd import eventstats, get_model
from pint_amd.polycos import Polycos
from test_photon import trig_numpy
from test_polycos import CASES, GOLD, load, pair, table_from

pytestmark = pytest.mark.gpu

LD = np.longdouble
LDEPS = float(np.finfo(LD).eps)


def polycos_of(name):
    z, meta = load(name)
    p = Polycos.read(os.path.join(GOLD, "B1855_polyco.dat")) if name == "poly_b1855" else table_from(z, meta)
    return p, z, meta


def circ(ai, af, bi, bf):
    return np.abs((LD(ai) - LD(bi)) + (LD(af) - LD(bf)))


def frac_of(v):
    v = LD(v)
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - LD(hi)))


def exact_phase(e, t):
    """The entry's phase at t in rational arithmetic, as (int, frac longdouble), split once."""
    dt = (frac_of(t) - frac_of(e.tmid)) * 1440
    p = Fraction(0)
    for c in e.coeffs[::-1]:
        p = p * dt + frac_of(c)
    p += frac_of(e.rphase.int[0]) + frac_of(e.rphase.frac[0]) + 60 * frac_of(e.f0) * dt
    k = (p + Fraction(1, 2)).__floor__()
    f = p - k
    hi = float(f)
    return float(k), LD(hi) + LD(float(f - Fraction(hi)))


@pytest.fixture(scope="module")
def device_tables():
    """Each table on the device once, with its phases at the check times."""
    out = {}
    for name in CASES + ["poly_b1855"]:
        p, z, meta = polycos_of(name)
        t = pair(z, "t")
        out[name] = (p, z, meta, t, p.eval_abs_phase(t))
    return out


# ---------------------------------------------------------------------------------------
# the evaluation kernel
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ["poly_b1855"])
def test_eval_phase(device_tables, name):
    p, z, meta, t, ph = device_tables[name]
    assert np.all((ph.frac >= -0.5) & (ph.frac < 0.5)) and np.array_equal(ph.int, np.round(ph.int))
    d_exact = circ(ph.int, ph.frac, z["exact_int"], pair(z, "exact_frac"))
    d_ref = circ(ph.int, ph.frac, z["ref_int"], pair(z, "ref_frac"))
    print(f"{name}: |device - exact| {float(d_exact.max()):.3g}, |device - reference| {float(d_ref.max()):.3g}, "
          f"e_eval {meta['e_eval']:.3g}")
    assert d_exact.max() <= meta["e_eval"] + 2.0 ** -53
    assert d_ref.max() <= 2 * meta["e_eval"] + 2.0 ** -53
    for n in (1, 63, 64, 65, 400):  # one lane, a wave less one, a wave, a wave and one, more than a workgroup
        if n > len(t):
            continue
        q = p.eval_abs_phase(t[:n])
        assert np.array_equal(q.int, ph.int[:n]) and np.array_equal(q.frac, ph.frac[:n]), n
    assert np.array_equal(p.eval_phase(t), ph.frac)
    perm = np.random.default_rng(5).permutation(len(t))  # unsorted input: the sorted answer, permuted
    q = p.eval_abs_phase(t[perm])
    assert np.array_equal(q.int, ph.int[perm]) and np.array_equal(q.frac, ph.frac[perm])
    t64 = t.astype(np.float64)  # float64 times travel with a zero low part (those still covered after the rounding)
    t64 = t64[np.searchsorted(p["t_start"], t64) - 1 == np.searchsorted(p["t_stop"], t64)]
    assert len(t64) > len(t) // 2
    q = p.eval_abs_phase(t64)
    h = p.eval_abs_phase(t64, device=False)
    assert circ(q.int, q.frac, h.int, h.frac).max() <= 2 * meta["e_eval"] + 2.0 ** -53


@pytest.mark.parametrize("name", CASES + ["poly_b1855"])
def test_eval_freq(device_tables, name):
    p, z, meta, t, _ = device_tables[name]
    f, fd = p.eval_spin_freq(t), p.eval_spin_freq_derivative(t)
    rf, rfd = pair(z, "freq"), pair(z, "fdot")
    uf = np.abs(f - rf) / np.spacing(np.abs(rf.astype(np.float64)))
    ufd = np.abs(fd - rfd) / np.spacing(np.abs(rfd.astype(np.float64)))
    print(f"{name}: frequency {float(uf.max()):.2f} ulp, derivative {float(ufd.max()):.2f} ulp")
    assert uf.max() <= 8 and ufd.max() <= 8
    assert f.dtype == LD and fd.dtype == LD


@pytest.mark.parametrize("name", CASES + ["poly_b1855"])
def test_eval_boundaries_and_uncovered(device_tables, name):
    p, z, meta, t, _ = device_tables[name]
    ts, te = p["t_start"], p["t_stop"]
    bar = meta["e_eval"] + 2.0 ** -53
    shared = [k for k in range(1, len(p)) if te[k - 1] == ts[k]]
    for k in shared + [len(p)]:  # a boundary time goes to the earlier entry (the last t_stop to the last entry)
        tb = te[k - 1]
        q = p.eval_abs_phase(np.array([tb], dtype=LD))
        ei, ef = exact_phase(p[k - 1]["entry"], tb)
        assert circ(q.int, q.frac, ei, ef)[0] <= bar, k
    if name != "poly_b1855":
        assert shared  # (the generated tables have entries that share a boundary exactly)
    # (neighbouring entries differ at their boundary by about the fit's error, far above the bar, so the
    # wrong entry would be seen; shown on the first shared boundary)
    for k in shared[:1]:
        oi, of = exact_phase(p[k]["entry"], te[k - 1])
        ei, ef = exact_phase(p[k - 1]["entry"], te[k - 1])
        assert circ(oi, of, ei, ef) > 4 * bar
    bad = np.array([ts[0], ts[0] - LD(1e-9), te[-1] + LD(1e-9)], dtype=LD)  # the first t_start itself is not covered
    for sel, cnt in ((slice(0, 1), 1), (slice(0, 3), 3)):
        tt = np.concatenate([t[:5], bad[sel], t[5:70]])
        with pytest.raises(ValueError, match=rf"Some input times not covered by Polyco entries. \({cnt} of {len(tt)}\)"):
            p.eval_abs_phase(tt)
        with pytest.raises(ValueError, match=rf"\({cnt} of {len(tt)}\)"):
            p.htest(tt)
    with pytest.raises(ValueError, match=r"\(1 of 1\)"):
        p.eval_spin_freq(np.array([np.nan]))
    s = p._device()
    hi, lo = t[:3].astype(np.float64), np.zeros(3)
    hi[1] = float(te[-1]) + 1.0
    oi, of, ofr, ofd, nunc = s.polyco_eval(hi, lo, 7)
    assert nunc == 1 and all(np.isnan(o[1]) and np.all(np.isfinite(o[[0, 2]])) for o in (oi, of, ofr, ofd))


def test_eval_b1855_gaps(device_tables):
    """Times inside tempo's 1e-11 day gaps and overlaps are not covered (find_entry's rule, on pairs)."""
    p = device_tables["poly_b1855"][0]
    ts, te = p["t_start"], p["t_stop"]
    n = 0
    for k in range(1, len(p)):
        d = float(ts[k] - te[k - 1])
        if 0 < abs(d) < 1e-10:
            a, b = sorted((te[k - 1], ts[k]))
            with pytest.raises(ValueError, match=r"\(1 of 1\)"):
                p.eval_abs_phase(np.array([a + (b - a) / 2], dtype=LD))
            n += 1
    assert n >= 2


def test_session_argument_errors(device_tables):
    from pint_amd._lib import PintError
    from pint_amd.engine import Session
    s = Session()
    try:
        with pytest.raises(PintError, match="no polyco table"):
            s.polyco_eval(np.array([55000.0]), np.zeros(1))
        with pytest.raises(PintError, match="no polyco table"):
            s.polyco_trig(np.array([55000.0]), np.zeros(1))
        hdr = np.zeros((11, 2))
        hdr[2] = [2.0, 1.0]  # t_start not sorted
        with pytest.raises(PintError, match="not sorted by t_start"):
            s.set_polycos(hdr, np.zeros((2, 3)), np.zeros((2, 3)))
        with pytest.raises(PintError, match="coefficients"):
            s.set_polycos(np.zeros((11, 2)), np.zeros((2, 17)), np.zeros((2, 17)))
        with pytest.raises(PintError, match="no coefficients given"):
            s.set_polycos(np.zeros((11, 2)), ncoeff=3)
        for nn, nc in ((65, 12), (20, 17), (5, 8), (20, 0)):  # outside the caps, or fewer nodes than coefficients
            with pytest.raises(PintError, match="coefficients"):
                s.polyco_fit_host(1, nn, nc, np.zeros(nn + 2), np.zeros(nn + 2), np.zeros(nn), np.zeros(nn), 1.0)
        with pytest.raises(PintError, match="no evaluated batch"):
            s.polyco_fit(1, 20, 12, np.zeros(20), np.zeros(20), 1.0)
    finally:
        s.close()
    p = device_tables["poly_gbt"][0]
    with pytest.raises(PintError, match="harmonics"):
        p._device().polyco_trig(np.array([55000.15]), np.zeros(1), None, 65)


# ---------------------------------------------------------------------------------------
# the solver (pint_polyco_fit_host)
# ---------------------------------------------------------------------------------------
def exact_lstsq(x, y, nc):
    """The least-squares polynomial of nc coefficients through the float64 data, in rational arithmetic
    (normal equations are exact there)."""
    xs, ys = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in y]
    pw = [[Fraction(1)] * len(xs)]
    for _ in range(2 * nc - 2):
        pw.append([a * b for a, b in zip(pw[-1], xs)])
    mom = [sum(r) for r in pw]
    A = [[mom[i + j] for j in range(nc)] + [sum(a * b for a, b in zip(pw[i], ys))] for i in range(nc)]
    for i in range(nc):
        piv = next(r for r in range(i, nc) if A[r][i] != 0)
        A[i], A[piv] = A[piv], A[i]
        inv = 1 / A[i][i]
        A[i] = [v * inv for v in A[i]]
        for r in range(nc):
            if r != i and A[r][i] != 0:
                f = A[r][i]
                A[r] = [a - f * b for a, b in zip(A[r], A[i])]
    return [A[i][nc] for i in range(nc)]


def poly_at(c, pts):
    out = []
    for x in pts:
        v = Fraction(0)
        for a in c[::-1]:
            v = v * x + (a if isinstance(a, Fraction) else Fraction(float(a)))
        out.append(v)
    return out


_EXACT = {}  # the exact solution and polyfit's error of a data set, computed once (key: the caller's)


def solver_check(x, y, nc, c_dev, tag, key=None):
    """The requirement on one segment; returns (device error, polyfit error) for the printout."""
    if key is None or key not in _EXACT:
        pts = [Fraction(float(v)) for v in np.linspace(x.min(), x.max(), 101)]
        pe = poly_at(exact_lstsq(x, y, nc), pts)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (polyfit's RankWarning on the raw dt of the 15- and 16-coefficient shapes)
            cp = np.polyfit(x, y, nc - 1)[::-1]
        ep = float(max(abs(a - b) for a, b in zip(poly_at(list(cp), pts), pe)))
        _EXACT[key if key is not None else tag] = (pts, pe, ep)
    pts, pe, ep = _EXACT[key if key is not None else tag]
    ed = float(max(abs(a - b) for a, b in zip(poly_at(list(c_dev), pts), pe)))
    assert ed <= 16 * ep + 2.0 ** -50 * float(np.max(np.abs(y))), (tag, ed, ep)
    return ed, ep


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


@pytest.fixture(scope="module")
def session():
    from pint_amd.engine import Session
    s = Session()
    yield s
    s.close()


@pytest.mark.parametrize("name", CASES)
def test_fit_stored_node_phases(session, name):
    """The reference's node and mid-point phases of every segment through the kernel: the coefficients
    against the exact solution of the same data (y_j as the kernel forms them: exact, rounded once), and
    rphase against the stored one."""
    z, meta = load(name)
    case = meta["case"]
    nseg, nn, nc = case["nseg"], case["nodes"], case["ncoeff"]
    f0 = pair(z, "f0")[0]
    ni, nfh, nfl = z["node_int"], z["node_frac_hi"], z["node_frac_lo"]
    mi, mfh, mfl = z["mid_int"], z["mid_frac_hi"], z["mid_frac_lo"]
    rows_i = np.concatenate([ni, mi[:, None]], axis=1).reshape(-1)
    rows_h = np.concatenate([nfh, mfh[:, None]], axis=1).reshape(-1)
    rows_l = np.concatenate([nfl, mfl[:, None]], axis=1).reshape(-1)
    hi, e = two_sum(rows_i, rows_h)  # int + frac as a normalised pair (|frac| <= 1/2, so e + lo is the low part)
    ph_hi, ph_lo = np.append(hi, 0.0), np.append(e + rows_l, 0.0)  # (the TZR row: phase 0, the phases are absolute)
    fit = session.polyco_fit_host(nseg, nn, nc, ph_hi, ph_lo, z["dt_hi"], z["dt_lo"], f0)
    assert np.array_equal(fit["rph_int"], z["rph_int"])
    assert np.max(np.abs((LD(fit["rph_frac_hi"]) + LD(fit["rph_frac_lo"])) - pair(z, "rph_frac"))) <= 2.0 ** -60
    F0 = frac_of(f0)
    worst = (0.0, 0.0)
    for s in range(nseg):
        mid = Fraction(float(mi[s])) + Fraction(float(mfh[s])) + Fraction(float(mfl[s]))
        y = np.array([float(Fraction(float(ni[s, j])) + Fraction(float(nfh[s, j])) + Fraction(float(nfl[s, j])) - mid
                            - 60 * F0 * (Fraction(float(z["dt_hi"][s, j])) + Fraction(float(z["dt_lo"][s, j]))))
                      for j in range(nn)])
        # (the reference's own y_j: formed in longdouble from terms of the size of 60 F0 dt)
        big = 60 * float(f0) * np.max(np.abs(z["dtd"][s]))
        assert np.max(np.abs(y - z["rdc"][s])) <= 4 * LDEPS * big + 4 * np.spacing(np.max(np.abs(y)))
        worst = max(worst, solver_check(z["dtd"][s], y, nc, fit["coeffs"][s], (name, s)))
        r = np.polyval(fit["coeffs"][s][::-1].astype(LD), z["dtd"][s].astype(LD)) - y
        want = float(np.sqrt(np.mean(r * r)))
        assert abs(fit["rms"][s] - want) <= 1e-6 * want + 1e-13 * np.max(np.abs(y))
    print(f"{name}: max |P_dev - P_exact| {worst[0]:.3g}, polyfit's {worst[1]:.3g}")


@pytest.mark.parametrize("nn,nc", [(20, 1), (20, 2), (12, 12), (16, 16), (33, 12), (64, 16)])
@pytest.mark.parametrize("nseg", [1, 5, 67])
def test_fit_synthetic(session, nn, nc, nseg):
    """Smooth-plus-noise data (F0 0 and a zero mid-point, so y_j is the node's phase itself).  Three
    distinct data sets cycle through the segments; every segment is checked."""
    rng = np.random.default_rng(100 * nn + nc)
    span = 720.0 if nc >= 15 else 60.0
    data = []
    for d in range(min(3, nseg)):
        x = np.linspace(-span / 2, span / 2, nn) + (rng.uniform(-1e-3, 1e-3, nn) if d == 2 else 0.0)
        u = x / (span / 2)
        y = (0.3 * np.sin(2.1 * u + d) + 0.05 * u ** 3 - 0.2 * u + 1e-3 * np.cos(7 * u)) * 10.0 ** (-3 * d) \
            + 1e-9 * rng.standard_normal(nn)
        data.append((x, y))
    ph = np.zeros(nseg * (nn + 1) + 1)
    dt = np.zeros((nseg, nn))
    for s in range(nseg):
        x, y = data[s % len(data)]
        ph[s * (nn + 1):s * (nn + 1) + nn] = y
        dt[s] = x
    fit = session.polyco_fit_host(nseg, nn, nc, ph, np.zeros_like(ph), dt, np.zeros_like(dt), 0.0)
    assert np.all(fit["rph_int"] == 0) and np.all(fit["rph_frac_hi"] == 0)
    for s in range(len(data), nseg):  # the same data, the same bits, whichever wave and workgroup took it
        assert np.array_equal(fit["coeffs"][s], fit["coeffs"][s % len(data)]) and fit["rms"][s] == fit["rms"][s % len(data)]
    for d, (x, y) in enumerate(data):
        ed, ep = solver_check(x, y, nc, fit["coeffs"][d], (nn, nc, nseg, d), key=(nn, nc, d))  # (the data do not depend on nseg)
        if nn > nc:  # the reported rms is that of the fit's node residuals
            r = np.polyval(fit["coeffs"][d][::-1].astype(LD), x.astype(LD)) - y
            want = float(np.sqrt(np.mean(r * r)))
            assert abs(fit["rms"][d] - want) <= 1e-6 * want + 1e-13 * np.max(np.abs(y))
        if d == 0:
            print(f"nnode {nn} ncoeff {nc}: max |P_dev - P_exact| {ed:.3g}, polyfit's {ep:.3g}")


# ---------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------
def fit_gain(dtd, nc, pts):
    """Lambda: the largest absolute row sum of the hat matrix V(pts) pinv(V(nodes)), in x = dt / max |dt|."""
    h = np.max(np.abs(dtd))
    V = np.vander(dtd / h, nc, increasing=True)
    W = np.vander(pts / h, nc, increasing=True)
    return float(np.max(np.sum(np.abs(W @ np.linalg.pinv(V)), axis=1)))


@pytest.fixture(scope="module")
def generated():
    out = {}
    for name in CASES:
        z, meta = load(name)
        case = meta["case"]
        model = get_model(os.path.join(GOLD, name + ".par"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)  # (no clock files for gbt: as the fixture was made)
            p = Polycos.generate_polycos(model, case["start"], case["end"], case["obs"], case["span"], case["ncoeff"],
                                         case["freq"], numNodes=case["nodes"])
        out[name] = (p, model, z, meta)
    return out


@pytest.mark.parametrize("name", CASES)
def test_generate_polycos(generated, name):
    p, model, z, meta = generated[name]
    case, tab = meta["case"], meta["table"]
    assert len(p) == case["nseg"]
    t = pair(z, "t")
    ph = p.eval_abs_phase(t)
    F0 = meta["F0"]
    pts = (t - pair(z, "tmid")[z["entry"]]).astype(np.float64) * 1440.0
    lam = max(fit_gain(z["dtd"][s], case["ncoeff"], np.append(pts[z["entry"] == s], 0.0)) for s in range(case["nseg"]))
    absph = float(np.max(np.abs(z["model_int"])))
    bar = meta["e_fit"] + lam * (1e-9 * F0 + 8 * LDEPS * absph)
    d = circ(ph.int, ph.frac, z["model_int"], pair(z, "model_frac"))
    ents = list(p["entry"])
    dr = circ([e.rphase.int[0] for e in ents], [e.rphase.frac[0] for e in ents], z["rph_int"], pair(z, "rph_frac"))
    print(f"{name}: |device polyco - reference model phase| {float(d.max()):.3g}, rphase {float(dr.max()):.3g}, bar {bar:.3g} "
          f"(e_fit {meta['e_fit']:.3g}, Lambda {lam:.2f}); fit rms {float(np.max(p.fit_rms)):.3g}")
    assert d.max() <= bar
    assert dr.max() <= bar
    for k, want in (("tmid", pair(z, "tmid")), ("t_start", pair(z, "t_start")), ("t_stop", pair(z, "t_stop"))):
        assert np.array_equal(p[k], want), k
    for k in ("mjd_span", "date", "utc", "dm", "obs", "obsfreq", "doppler", "logrms"):
        assert list(p[k]) == tab[k], k
    assert [str(x) for x in p["psr"]] == tab["psr"]
    assert all(e.f0 == pair(z, "f0")[0] and e.ncoeff == case["ncoeff"] for e in ents)
    if "f_orbit" in tab:
        assert list(p["f_orbit"]) == tab["f_orbit"]
        db = np.abs(np.array(p["binary_phase"]) - np.array(tab["binary_phase"]))
        assert np.max(np.minimum(db, 1 - db)) <= 1e-9
    else:
        assert "binary_phase" not in p.polycoTable.colnames
    assert repr(float(model.TZRMJD.value)) == meta["tzrmjd"]  # (poly_bary: the TZR the call left on the model)
    # the table adopted on the device is the table on the host: a fresh upload gives the same phases, to the
    # rounding of the fraction (the adopted rphase fraction is the kernel's pair, the host's its longdouble sum)
    q = Polycos.from_table(p.polycoTable[0:len(p)])
    ph2 = q.eval_abs_phase(t)
    assert circ(ph2.int, ph2.frac, ph.int, ph.frac).max() <= 2.0 ** -53
    h = p.eval_abs_phase(t, device=False)
    assert circ(ph.int, ph.frac, h.int, h.frac).max() <= 2 * meta["e_eval"] + 2.0 ** -53
    if name == "poly_gbt":  # written and read back, it evaluates within the 6-decimal rphase of the file
        import io
        out = io.StringIO()
        p.write_polyco_file(out)
        assert len(Polycos.read(io.StringIO(out.getvalue()))) == len(p)


# ---------------------------------------------------------------------------------------
# the sums
# ---------------------------------------------------------------------------------------
NS = [1, 255, 256, 257, 100003]
MS = [1, 8, 9, 20, 64]


@pytest.fixture(scope="module")
def sum_data(device_tables):
    """Per n: times repeated across poly_gbt's covered range, weights, the device's own phases and
    trig_numpy's sums and bars of them at m = 64, unweighted and weighted (harmonic j is the same
    expression at every m)."""
    p, z, meta, t, _ = device_tables["poly_gbt"]
    rng = np.random.default_rng(11)
    out = {}
    for n in NS:
        tt = np.tile(t, n // len(t) + 1)[:n] if n > 1 else t[137:138]
        w = rng.beta(1.2, 1.6, n)
        phi = np.asarray(p.eval_phase(tt), dtype=np.float64)
        out[n] = (tt, w, phi, trig_numpy(phi, None, 64), trig_numpy(phi, w, 64))
    return p, out


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", NS)
def test_trig_sums(sum_data, n, weighted):
    p, data = sum_data
    tt, w, phi, ref_u, ref_w = data[n]
    ref, bar = ref_w if weighted else ref_u
    wt = w if weighted else None
    for m in MS:
        got = p.device_trig(tt, wt, m)
        sel = np.r_[0:2 * m, 128, 129]
        err = np.abs(got.astype(LD) - ref[sel]).astype(np.float64)
        b = bar[sel].copy()
        b[-2:] = 16 * np.log2(n) * 2.0 ** -53 * np.abs(ref[sel][-2:]).astype(np.float64)
        assert np.all(err <= b), (n, m, weighted, float(np.max(err - b)))
        assert np.array_equal(p.device_trig(tt, wt, m), got)  # two calls, identical bits
        if m == 20:
            H, Z = p.htest(tt, wt, m=20)
            ph1 = phi % 1.0
            if weighted:
                assert H == eventstats.hmw(None, None, 20, sums=got) and np.array_equal(Z, eventstats.z2mw(None, None, 20, sums=got))
                want = eventstats.hmw(ph1, w, 20)
            else:
                assert H == eventstats.hm(None, 20, sums=got) and np.array_equal(Z, eventstats.z2m(None, 20, sums=got))
                want = eventstats.hm(ph1, 20)
            assert Z.shape == (20,)
            assert abs(H - want) <= 1e-9 * max(1.0, abs(want))
