"""The photon-event path on the device (pint_set_photons, pint_point_photon_lnlike, pint_point_photon_trig,
PhotonTiming) against fixtures captured from the reference's scripts/event_optimize.py and eventstats.py
(scripts/refgen/gen_photon.py):

* photon_geo  : 1500 weighted photons at the geocenter, ELL1, AbsPhase, 256-bin template (1501 rows: two
                1024-row residual blocks);
* photon_bary : 256 unweighted photons at the barycentre, isolated, no AbsPhase, 100-bin template (257
                rows: the TZR row alone in the second 256-row block).

Bars.
Phase against the reference, circular: 1 ns x F0 plus 8 ulps of the (longdouble) absolute phase, the bar of
the absolute-phase tests (tests/test_wavex.py).
Kernels against numpy on the device's own phases (read_eval's hi and lo, the fraction taken in longdouble,
the reference's expressions restated): only the rounding of log, the summation order and the last ulp of
x differ, so with eps = 2^-53
  lnL          64 eps (sum_i |log term_i| + sum_i |w_i T'(x_i) / (w_i T(x_i) + 1 - w_i)|),
  harmonic j   16 (j + log2 n) eps sum_i |w_i|   (the numpy side in longdouble),
  sum w, w^2   16 log2 n eps x the sum;
a wrong harmonic, bin or weight misses these by many orders of magnitude.  No x lies within 1e-12 of the
template's last node (L - 1) / L (asserted; the offsets are chosen on the CPU so that this excludes none).
End to end against the reference: 2 x the reference's own spread (photon_spread.json: its phases shifted by
5 ps x F0 and 30 ps x F0 rms) scaled to the measured rms phase difference, clamped to the calibrated
5-30 ps, as golden_util.chi2_bar does.
"""
import numpy as np
import pytest

from photon_util import NAMES, load, points, spread

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
SPREAD_MAX_PS = 30.0


# ---------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------
def template_of(L, meta):
    """A positive template of L bins: the fixture's Gaussian file, divided by its mean."""
    import io
    from pint_amd.event_optimize import read_gaussfitfile
    if L == 1:
        return np.array([1.0])
    t = read_gaussfitfile(io.StringIO(meta["gauss"]), L)
    return t / t.mean()


def device_fractions(s, abs_phase):
    """The photon phases of every instance from the device's own hi and lo: d - floor(d) in longdouble,
    rounded to float64 and kept in [0, 1)."""
    hi, lo, _, _ = s.read_eval()
    out = []
    for h, l in zip(hi, lo):
        # (an absolute phase of ~3e10 cycles has a longdouble ulp of 3.5e-9, so the integer parts go first:
        # hi - floor(hi) is exact in float64, and the integers do not enter the fraction of a difference)
        fh = LD(h - np.floor(h))
        a = fh[:-1] - fh[-1] if abs_phase else fh[:-1]
        b = LD(l[:-1]) - LD(l[-1]) if abs_phase else LD(l[:-1])
        d = a + b
        f = (d - np.floor(d)).astype(np.float64)
        out.append(np.where(f >= 1.0, np.nextafter(1.0, 0.0), f))
    return out


def lnl_numpy(phi, w, tmpl, phs):
    """(lnL, bar, x) of one offset: the reference's expressions, and the docstring's bar."""
    L = len(tmpl)
    xp = np.arange(L) * 1.0 / L
    x = (phi.astype(np.float64) + np.float64(phs)) % 1
    p = np.interp(x, xp, tmpl, right=tmpl[0])
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, max(L - 2, 0))
    slope = np.where(x > xp[-1], 0.0, (tmpl[np.minimum(j + 1, L - 1)] - tmpl[j]) * L) if L > 1 else np.zeros_like(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        if w is None:
            terms, sens = np.log(p), np.abs(slope / p)
        else:
            arg = w * p + 1.0 - w
            terms, sens = np.log(arg), np.abs(w * slope / arg)
    tot = float(np.sum(terms.astype(LD)))
    bar = 64 * EPS * (float(np.sum(np.abs(terms))) + float(np.sum(sens)))
    return tot, bar, x


def trig_numpy(phi, w, m):
    """(sums (2 m + 2), bars (2 m + 2)) in longdouble."""
    n = len(phi)
    wl = np.ones(n, dtype=LD) if w is None else w.astype(LD)
    a = 2 * LD(np.pi) * phi.astype(LD)
    out, bar = np.zeros(2 * m + 2, dtype=LD), np.zeros(2 * m + 2)
    sw = float(np.sum(np.abs(wl)))
    for j in range(1, m + 1):
        out[2 * j - 2], out[2 * j - 1] = np.sum(wl * np.cos(j * a)), np.sum(wl * np.sin(j * a))
        bar[2 * j - 2] = bar[2 * j - 1] = 16 * (j + np.log2(n)) * EPS * sw
    w2 = np.ones(n) if w is None else w * w  # (the float64 products, summed in longdouble)
    out[2 * m], out[2 * m + 1] = np.sum(wl), np.sum(w2.astype(LD))
    bar[2 * m], bar[2 * m + 1] = 16 * np.log2(n) * EPS * float(out[2 * m]), 16 * np.log2(n) * EPS * float(out[2 * m + 1])
    return out, bar


def choose_offsets(phi, L, nphs, seed):
    """nphs offsets in [0, 1) chosen on the CPU from the device's phases: the first four put photon 0 in the
    middle of the last segment, just below 1, just across the wrap, and leave it where it is; the rest are
    drawn.  Any that would bring a photon within 1e-12 of the last node is moved by 1e-9 until none is."""
    edge = (L - 1.0) / L
    rng = np.random.default_rng(seed)
    special = [(edge + 0.5 / L - phi[0]) % 1, (1.0 - 1e-9 - phi[0]) % 1, (1.0 + 1e-9 - phi[0]) % 1, 0.0]
    off = np.concatenate([special, rng.uniform(0, 1, max(nphs - 4, 0))])[:nphs]
    for i in range(len(off)):
        while np.min(np.abs((phi + off[i]) % 1 - edge)) <= 1e-12:
            off[i] = (off[i] + 1e-9) % 1
    return off


def open_session(name, n=None, weights="fixture", L=None):
    """(session, layout, base table, weights, template, meta): the fixture's pulsar (its first n photons,
    the TZR row kept) resident with its photon data, one instance at the par file's values, evaluated."""
    from pint_amd.engine import Session, build_layout, pack_table
    model, toas, z, meta = load(name)
    if n is not None:
        toas = toas[:n]
    n = toas.ntoas
    tmpl = z["tmpl"] if L is None else template_of(L, meta)
    if isinstance(weights, str):
        w = {"fixture": z.get("weights"), "none": None, "ones": np.ones(n),
             "zero_one": np.where(np.arange(n) % 3 == 0, 0.0, np.where(np.arange(n) % 3 == 1, 1.0, 0.37))}[weights]
        w = None if w is None else np.ascontiguousarray(w[:n])
    else:
        w = weights
    s = Session()
    lay = s.add(build_layout(model, toas, track_mode="nearest", use_gls_basis=False))
    s.set_photons(lay, w, tmpl, meta["abs_phase"])
    tab = pack_table(lay, model)
    s.set_instances([(lay, tab)])
    s.eval(False)
    return s, lay, tab, w, tmpl, meta


def check_kernels(s, phi, w, tmpl, m, nphs, seed=0):
    """Both kernels of a one-instance batch against numpy on the device's phases phi."""
    L = len(tmpl)
    off = choose_offsets(phi, L, nphs, seed)
    got = s.point_photon_lnlike(off[None, :])[0]
    edge = (L - 1.0) / L
    worst, in_last = 0.0, 0
    for j in range(nphs):
        ref, bar, x = lnl_numpy(phi, w, tmpl, off[j])
        assert np.min(np.abs(x - edge)) > 1e-12
        in_last += int(np.count_nonzero(x > edge))
        assert abs(got[j] - ref) <= bar, (j, got[j], ref, bar)
        worst = max(worst, abs(got[j] - ref) / bar if bar else 0.0)
    if nphs >= 3 and L > 1:  # the chosen photon was in the last segment, and crossed the wrap
        assert ((phi[0] + off[0]) % 1 > edge) and ((phi[0] + off[1]) % 1 > edge) and ((phi[0] + off[2]) % 1 < 1e-8)
    sums = s.point_photon_trig(m)[0]
    ref, bar = trig_numpy(phi, w, m)
    err = np.abs(sums.astype(LD) - ref).astype(np.float64)
    assert np.all(err <= bar), (np.argmax(err - bar), err.max())
    print(f"n {len(phi)} L {L} m {m} nphs {nphs}: lnL worst {worst:.3f} of its bar, {in_last} photon-offsets in the last "
          f"segment; trig worst {np.max(err[:-2] / bar[:-2]):.3f} of its bar")


# ---------------------------------------------------------------------------------------
# phase
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_phase_against_the_reference(name):
    from pint_amd import PhotonTiming
    model, toas, z, meta = load(name)
    pt = PhotonTiming(model, toas, z["tmpl"], weights=z.get("weights"), prior_info=meta["prior_info"])
    pts = points(pt, z, meta)
    got = pt.get_event_phases(pts)
    d = got - z["pt_phase"]
    d -= np.round(d)
    hi = pt._device().read_eval()[0]
    bar = 1e-9 * float(model.F0.value) + 8 * float(np.spacing(LD(np.max(np.abs(hi[0])))))
    print(f"{name}: max |dphi| {np.max(np.abs(d)):.3g} cycles (bar {bar:.3g})")
    assert got.shape == (16, toas.ntoas) and np.all((got >= 0) & (got < 1))
    assert np.max(np.abs(d)) <= bar
    assert np.array_equal(pt.get_event_phases(pts[5]), got[5])
    base = pt.get_event_phases()
    assert base.shape == (toas.ntoas,) and np.all((base >= 0) & (base < 1))
    pt.close()


# ---------------------------------------------------------------------------------------
# kernels against numpy on the device's own phases
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025])
def test_kernels_row_counts(n):
    s, lay, tab, w, tmpl, meta = open_session("photon_geo", n=n)
    try:
        phi = device_fractions(s, meta["abs_phase"])[0]
        assert phi.shape == (n,)
        check_kernels(s, phi, w, tmpl, 20, 8 if n > 1 else 4, seed=n)
    finally:
        s.close()


@pytest.mark.parametrize("L", [1, 2, 100, 256, 4096])
def test_kernels_template_sizes(L):
    s, lay, tab, w, tmpl, meta = open_session("photon_geo", n=257, L=L)
    try:
        assert len(tmpl) == L
        check_kernels(s, device_fractions(s, True)[0], w, tmpl, 1, 9, seed=L)
    finally:
        s.close()


@pytest.mark.parametrize("m,nphs,weights", [(1, 1, "fixture"), (20, 64, "none"), (64, 1024, "ones"), (64, 1, "zero_one"),
                                            (20, 64, "zero_one")])
def test_kernels_harmonics_offsets_weights(m, nphs, weights):
    s, lay, tab, w, tmpl, meta = open_session("photon_geo", n=1025, weights=weights)
    try:
        if weights == "zero_one":
            assert np.any(w == 0.0) and np.any(w == 1.0)
        check_kernels(s, device_fractions(s, True)[0], w, tmpl, m, nphs, seed=m + nphs)
    finally:
        s.close()


def test_kernels_no_abs_phase():
    """photon_bary: the row's phase itself, unweighted, a template of 100 bins (no power of two)."""
    s, lay, tab, w, tmpl, meta = open_session("photon_bary")
    try:
        assert w is None and not meta["abs_phase"] and len(tmpl) == 100
        check_kernels(s, device_fractions(s, False)[0], w, tmpl, 20, 64, seed=3)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------
# end to end against the reference
# ---------------------------------------------------------------------------------------
def spread_bar(name, kind, k, rms_ps, floor=0.0):
    d = spread()[name]
    per_ps = np.maximum(np.asarray(d["5ps"][kind][k]) / 5.0, np.asarray(d["30ps"][kind][k]) / 30.0)
    return np.maximum(floor, 2.0 * per_ps * min(max(float(rms_ps), 5.0), SPREAD_MAX_PS))


@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(name):
    from pint_amd import PhotonTiming
    model, toas, z, meta = load(name)
    w = z.get("weights")
    pt = PhotonTiming(model, toas, z["tmpl"], weights=w, prior_info=meta["prior_info"])
    pts = points(pt, z, meta)
    dphi = pt.get_event_phases(pts) - z["pt_phase"]
    dphi -= np.round(dphi)
    f0 = spread()[name]["F0"]
    lnl = pt.lnlikelihood_batch(pts)
    post = pt.lnposterior_batch(pts)
    H, Z = pt.htest_batch(pts, m=20, c=4)
    off, best, scan = pt.phase_scan(pts, resolution=1.0 / 64)
    assert lnl.shape == (16,) and H.shape == (16,) and Z.shape == (16, 20) and scan.shape == (16, 64)
    hk, zk = ("pt_hmw", "pt_z2mw") if w is not None else ("pt_hm", "pt_z2m")
    for k in range(16):
        rms = float(np.sqrt(np.mean(dphi[k] ** 2))) / f0 * 1e12
        b = spread_bar(name, "lnl", k, rms)
        print(f"{name} point {k}: rms {rms:.2f} ps; dlnL {abs(lnl[k] - z['pt_lnl'][k]):.3g} (bar {b:.3g}); "
              f"dH {abs(H[k] - z[hk][k]):.3g} (bar {spread_bar(name, 'h', k, rms):.3g})")
        assert abs(lnl[k] - z["pt_lnl"][k]) <= b
        assert abs(post[k] - z["pt_post"][k, 0]) <= b + 1e-12 * abs(z["pt_post"][k, 1])
        assert abs(H[k] - z[hk][k]) <= spread_bar(name, "h", k, rms)
        assert np.all(np.abs(Z[k] - z[zk][k]) <= spread_bar(name, "z2", k, rms))
        assert np.all(np.abs(scan[k] - z["pt_scan"][k]) <= spread_bar(name, "scan", k, rms))
        assert off[k] == z["pt_scan_ret"][k, 0]  # the argmax of the scan
        assert abs(best[k] - z["pt_scan_ret"][k, 1]) <= spread_bar(name, "scan", k, rms)
    assert pt.lnlikelihood(pts[4]) == lnl[4] and pt.lnposterior(pts[4]) == post[4]
    # outside the prior: -inf, and the point is not evaluated on its own values
    out = pts[:2].copy()
    out[0, -1] = LD(1.5)
    out[1, 0] += LD(1.0)
    assert np.all(np.isneginf(pt.lnposterior_batch(out)))
    pt.close()


# ---------------------------------------------------------------------------------------
# reproducibility, mixed batches
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reproducible_and_batch_independent(name):
    from pint_amd import PhotonTiming
    model, toas, z, meta = load(name)
    pt = PhotonTiming(model, toas, z["tmpl"], weights=z.get("weights"), prior_info=meta["prior_info"])
    pts = points(pt, z, meta)

    def run(p):
        return (pt.lnlikelihood_batch(p), *pt.htest_batch(p, m=20), pt.phase_scan(p, resolution=1.0 / 64)[2],
                pt.htest_batch(p, m=64)[1])
    a, b = run(pts), run(pts)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    alone = run(pts[7:8])
    two = run(pts[[3, 7]])
    many = run(np.concatenate([np.tile(pts[:8], (8, 1)), pts[7:8]]))  # 65 points, point 7 last
    for x, y1, y2, y3 in zip(a, alone, two, many):
        assert np.array_equal(x[7], y1[0]) and np.array_equal(x[7], y2[1]) and np.array_equal(x[7], y3[64])
        assert np.array_equal(x[7], y3[7])
    pt.close()


def test_mixed_batch():
    """photon_geo and photon_bary instances interleaved in one batch give each fixture's own bits."""
    from pint_amd.engine import Session, build_layout, pack_table
    s = Session()
    try:
        lays, tabs, data = [], [], []
        for name in NAMES:
            model, toas, z, meta = load(name)
            lay = s.add(build_layout(model, toas, track_mode="nearest", use_gls_basis=False))
            s.set_photons(lay, z.get("weights"), z["tmpl"], meta["abs_phase"])
            t0 = pack_table(lay, model)
            t1 = t0.copy()
            t1[lay.offsets["F1"]] *= 1.0 + 1e-3
            lays.append(lay)
            tabs.append((t0, t1))
        off = np.random.default_rng(5).uniform(0, 1, (4, 7))
        alone = []
        for lay, (t0, t1) in zip(lays, tabs):
            s.set_instances([(lay, t0), (lay, t1)])
            s.eval(False)
            i = len(alone)
            alone.append((s.point_photon_lnlike(off[[i, i + 2]]).copy(), s.point_photon_trig(20).copy()))
        s.set_instances([(lays[0], tabs[0][0]), (lays[1], tabs[1][0]), (lays[0], tabs[0][1]), (lays[1], tabs[1][1])])
        s.eval(False)
        lnl, trig = s.point_photon_lnlike(off), s.point_photon_trig(20)
        assert np.all(np.isfinite(lnl)) and not np.array_equal(lnl[0], lnl[2])
        for p in range(2):
            assert np.array_equal(lnl[[p, p + 2]], alone[p][0]) and np.array_equal(trig[[p, p + 2]], alone[p][1])
    finally:
        s.close()


def test_lazy_mode():
    """Lazy mode only enqueues: the outputs are pinned buffers, complete after check(), with the eager
    bits; the offsets are kept alive until then."""
    s, lay, tab, w, tmpl, meta = open_session("photon_geo", n=700)
    try:
        off = np.random.default_rng(11).uniform(0, 1, (2, 9))
        tab2 = tab.copy()
        tab2[lay.offsets["F1"]] *= 1.0 + 1e-3
        s.set_instances([(lay, tab), (lay, tab2)])
        s.eval(False)
        eager = (s.point_photon_lnlike(off).copy(), s.point_photon_trig(20).copy(), s.point_photon_trig(64).copy())
        s.set_lazy(True)
        s.set_instances([(lay, tab), (lay, tab2)])
        s.eval(False)
        lnl = s.point_photon_lnlike(off.copy())  # (a temporary: the Session keeps it until check())
        assert len(s._keep) >= 1 and s._keep[-1].shape == (2, 9)
        t20 = s.point_photon_trig(20)
        s.check()
        assert not s._keep
        got20 = t20.copy()                         # (the next call reuses the pinned buffer)
        t64 = s.point_photon_trig(64)
        s.check()
        assert lnl.shape == (2, 9) and got20.shape == (2, 42) and t64.shape == (2, 130)
        assert np.array_equal(lnl, eager[0]) and np.array_equal(got20, eager[1]) and np.array_equal(t64, eager[2])
        s.set_lazy(False)
        assert np.array_equal(s.point_photon_lnlike(off), eager[0])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------
# errors, IEEE results, the unchanged path
# ---------------------------------------------------------------------------------------
def test_entry_point_errors():
    from pint_amd import _lib as L
    from pint_amd.engine import Session, build_layout, pack_table
    s, lay, tab, w, tmpl, meta = open_session("photon_geo", n=300)
    try:
        off = np.array([[0.1, 0.6]])
        lnl0, trig0 = s.point_photon_lnlike(off).copy(), s.point_photon_trig(20).copy()
        dp = L.ptr
        bad = [lambda: s.L.pint_set_photons(s.ctx, lay.psr_id, 2, dp(w), len(tmpl), dp(tmpl)),        # abs_phase
               lambda: s.L.pint_set_photons(s.ctx, 5, 1, dp(w), len(tmpl), dp(tmpl)),                  # no such pulsar
               lambda: s.L.pint_set_photons(s.ctx, -1, 1, dp(w), len(tmpl), dp(tmpl)),
               lambda: s.L.pint_set_photons(s.ctx, lay.psr_id, 1, dp(w), 0, dp(tmpl)),                 # count 0 with a template
               lambda: s.L.pint_set_photons(s.ctx, lay.psr_id, 1, dp(w), L.MAX_TEMPLATE + 1, dp(np.ones(L.MAX_TEMPLATE + 1))),
               lambda: s.L.pint_set_photons(s.ctx, lay.psr_id, 1, dp(w), -3, dp(tmpl)),
               lambda: s.L.pint_set_photons(s.ctx, lay.psr_id, 1, dp(w), 16, None)]                    # a count without a template
        for f in bad:
            assert f() == L.PINT_E_INVALID
            assert b"pint_set_photons" in s.L.pint_last_error(s.ctx)
            # the previous data are in force
            assert np.array_equal(s.point_photon_lnlike(off), lnl0) and np.array_equal(s.point_photon_trig(20), trig0)
        with pytest.raises(ValueError, match="weights must have 300 entries"):
            s.set_photons(lay, np.ones(7), tmpl)
        out = np.zeros(4096)
        for nphs in (0, -1, L.MAX_PHOTON_PHS + 1):
            assert s.L.pint_point_photon_lnlike(s.ctx, nphs, dp(out), dp(out)) == L.PINT_E_INVALID
            assert b"phase offsets per instance" in s.L.pint_last_error(s.ctx)
        assert s.L.pint_point_photon_lnlike(s.ctx, 1, None, dp(out)) == L.PINT_E_INVALID
        for m in (0, -2, L.MAX_PHOTON_HARM + 1):
            assert s.L.pint_point_photon_trig(s.ctx, m, dp(out)) == L.PINT_E_INVALID
            assert b"harmonics" in s.L.pint_last_error(s.ctx)
        with pytest.raises(ValueError, match=r"phs must be \(1, nphs\)"):
            s.point_photon_lnlike(np.zeros((2, 3)))
        # a batch that was set but not evaluated since: refused, not read
        s.set_instances([(lay, tab)])
        for call in (lambda: s.point_photon_lnlike(off), lambda: s.point_photon_trig(20)):
            with pytest.raises(L.PintError, match="no evaluated batch"):
                call()
        s.eval(False)
        assert np.array_equal(s.point_photon_lnlike(off), lnl0)
        s.set_tables(tab)
        with pytest.raises(L.PintError, match="no evaluated batch"):
            s.point_photon_trig(20)
        s.eval(False)
        assert np.array_equal(s.point_photon_trig(20), trig0)
        # a second call replaces the data: no template -> the likelihood is refused, the sums are not
        s.set_photons(lay, None, None, True)
        with pytest.raises(L.PintError, match="has no template"):
            s.point_photon_lnlike(off)
        unweighted = s.point_photon_trig(20)
        assert unweighted[0, -2] == 300.0 and unweighted[0, -1] == 300.0 and not np.array_equal(unweighted, trig0)
        s.set_photons(lay, w, tmpl, True)
        assert np.array_equal(s.point_photon_lnlike(off), lnl0) and np.array_equal(s.point_photon_trig(20), trig0)
        # a pulsar of the batch without photon data
        model2, toas2, _, _ = load("photon_bary")
        lay2 = s.add(build_layout(model2, toas2, track_mode="nearest", use_gls_basis=False))
        s.set_instances([(lay, tab), (lay2, pack_table(lay2, model2))])
        s.eval(False)
        for call in (lambda: s.point_photon_lnlike(np.zeros((2, 1))), lambda: s.point_photon_trig(3)):
            with pytest.raises(L.PintError, match="pulsar 1 of the batch has no photon data"):
                call()
    finally:
        s.close()
    s2 = Session()
    try:  # nothing evaluated
        assert s2.L.pint_point_photon_trig(s2.ctx, 3, L.ptr(np.zeros(8))) == L.PINT_E_INVALID
    finally:
        s2.close()


def test_non_positive_log_argument():
    """A template with a span of zeros (log 0 = -inf) and one with negative values (NaN), unweighted: the
    instance whose offset puts a photon there gets IEEE's result, the other instance its finite value."""
    from pint_amd.engine import Session
    s, lay, tab, w, tmpl, meta = open_session("photon_geo", n=5, weights="none")
    try:
        phi = device_fractions(s, True)[0]
        L = 64
        for fill, test in ((0.0, np.isneginf), (-0.5, np.isnan)):
            t = np.ones(L)
            t[20:26] = fill
            s.set_photons(lay, None, t, True)
            s.set_instances([(lay, tab), (lay, tab)])
            s.eval(False)
            inside = (22.5 / L - phi[0]) % 1          # photon 0 in the middle of the span
            outside = None
            for c in np.linspace(0, 1, 400, endpoint=False):  # an offset that keeps every photon clear of it
                x = (phi + c) % 1
                if np.all((x < 18.0 / L) | (x > 28.0 / L)) and np.all(x < (L - 1.5) / L):
                    outside = c
                    break
            assert outside is not None
            got = s.point_photon_lnlike(np.array([[inside], [outside]]))[:, 0]
            ref_in, _, _ = lnl_numpy(phi, None, t, inside)
            ref_out, bar, _ = lnl_numpy(phi, None, t, outside)
            assert test(got[0]) and test(ref_in)
            assert np.isfinite(got[1]) and abs(got[1] - ref_out) <= bar
    finally:
        s.close()


def test_existing_paths_unchanged_by_photon_data():
    """A BayesianTiming batch and a GLS fit step give identical bits before and after pint_set_photons on
    the same context."""
    import golden_util
    import test_bayesian as tb
    from pint_amd.engine import Session
    from pint_amd.fitter import BatchFit
    bt, z, meta, perm = tb.bayes("bayes_nb")
    pts = tb._pts(z, "pts", perm)
    before = bt.lnlikelihood_terms_batch(pts)
    s = bt._device()
    s.set_photons(bt.lay, np.full(bt.lay.n, 0.5), np.ones(32), True)
    assert np.array_equal(bt.lnlikelihood_terms_batch(pts), before)
    bt.lnlikelihood_batch(pts[:3])
    assert s.point_photon_trig(2).shape == (3, 6)  # (and the photon calls work on that context)
    assert np.array_equal(bt.lnlikelihood_terms_batch(pts), before)
    bt.close()

    model, toas, _, _ = golden_util.load("pta_ell1")
    bf = BatchFit([(model, toas)], mode="gls")
    s = bf.s

    def step():
        s.eval(want_M=Session.FIT)
        s.fit_step(1)
        dp, er, cov, _ = s.read_step()
        return np.array(dp[0]), np.array(er[0]), np.array(cov[0])
    a = step()
    s.set_photons(s.layouts[0], None, np.ones(8), True)
    b = step()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
