"""Host checks of the residual sweep's case table (resid_cases.py), no device: the masks stated
by hand against the dispatch arithmetic, the models and option sets against the layout's spec,
the fit flow's models against the k_gram_v layout rules, and -- from the F0 / F1 offsets alone,
to the ~1e-2 turns the TOAs' noise and delays leave -- the wander of the phase residual, the
half-integer margin of the `nearest` branch and the r^T N^-1 r / chi2 <= 10 condition of the
cases that check a GLS chi2 (the GPU test asserts the last two on the device's own phases)."""
import numpy as np
import pytest

import resid_cases as RC
import shape_cases as SC

CASES = RC.cases()
_TOAS = {}


def host_toas(n):
    """The first n rows of the unzeroed fake TOA set (host only)."""
    if not _TOAS:
        from pint_amd.simulation import _row_arrays, _times_freqs, _tzr
        from pint_amd.toa import TOAs
        base = RC.model_of(RC.RCase("base", (RC.N_ALL,), 0), False)
        sp = RC.toa_spec(base)
        t, f = _times_freqs(sp["start"], sp["end"], sp["ntoas"], sp["freq"], False)
        fl = {"name": ["fake"] * len(t), "f": ["fake"] * len(t)}
        toas = TOAs(_row_arrays(t, f, sp["error_us"], sp["obs"]), fl, _tzr(base, sp["obs"]), "fake")
        toas.arrays["pulse_number"] = np.zeros(len(t))
        toas.arrays["delta_pulse_number"] = RC.delta_pulse_numbers()
        _TOAS[RC.N_ALL] = toas
    if n not in _TOAS:
        _TOAS[n] = _TOAS[RC.N_ALL][np.arange(n)]
    return _TOAS[n]


def test_masks():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    union = 0
    for c in CASES:
        assert RC.predict_mask(c) == (c.mask, c.mask_read), c.name
        union |= c.mask | c.mask_read
    assert union == 255
    # the fit flow's limit: 64 evaluation blocks of 254 rows, or 64 residual blocks of 1024
    by = {c.name: c for c in CASES}
    assert by["defer_n16256"].mask & RC.DEFERRED and not by["defer_n16257_not"].mask & RC.DEFERRED
    assert 64 * RC.EF_ROWS == 16256 == RC.N_ALL - 1
    # hand-written rows of the dispatch table
    assert RC.predict_mask(RC.RCase("x", (256,), 0)) == (RC.R12, 0)
    assert RC.predict_mask(RC.RCase("x", (257,), 0)) == (RC.EFUSED | RC.R2_256, 0)
    assert RC.predict_mask(RC.RCase("x", (256,), 0, small=False, efuse=False)) == (RC.R1_256 | RC.R2_256, 0)
    assert RC.predict_mask(RC.RCase("x", (256,), 0, flow="tiles")) == (RC.R1_64 | RC.R2_64 | RC.TILES, 0)
    assert RC.predict_mask(RC.RCase("x", (256,), 0, flow="tiles", nred=64)) == (RC.R12, 0)
    assert RC.predict_mask(RC.RCase("x", (65537,), 0, flow="fit", efuse=False)) == (RC.R1_256 | RC.R2_256, 0)
    assert RC.predict_mask(RC.RCase("x", (256,), 0, flow="fit")) == (RC.R1_64 | RC.DEFERRED, RC.R2_64)
    assert RC.predict_mask(RC.RCase("x", (256,), 0, flow="fit"), vgram=False) == (RC.R12, 0)


def test_inputs():
    e, d = RC.err_us(), RC.delta_pulse_numbers()
    assert set(e) == {0.5, 5.0} and 0.4 < np.mean(e == 0.5) < 0.6
    assert np.count_nonzero(d) == RC.N_ALL // 10 and set(d) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    # every prefix of at least 63 rows holds rows of both classes and some shifted rows
    assert len(set(e[:63])) == 2 and np.count_nonzero(d[:63]) >= 3
    assert len(RC.OPTIONS) == 8 and len({o.name for o in RC.OPTIONS}) == 8
    # the weighted and the unweighted mean of an O(1)-turn residual differ by far more than a bar
    full, _ = RC.approx_full(1025, 0, RC.OPTIONS[0])
    w = 1 / e[:1025] ** 2
    assert abs(np.sum(w * full) / np.sum(w) - np.mean(full)) > 1e-3


@pytest.mark.parametrize("c", [c for c in CASES if c.name in ("small_n1_x1_r12", "small_n2_x3_r12", "efused_n254",
                                                              "tiles_n65_nred63_efused", "defer_n1025")],
                         ids=lambda c: c.name)
def test_models_and_specs(c):
    from pint_amd.engine import build_layout
    n = c.ns[0]
    for o in RC.OPTIONS:
        m = RC.model_of(c, o.phoff, n)
        assert ("PhaseOffset" in m.components) == o.phoff and ("PHOFF" in m.free_params) == o.phoff
        assert ("PLRedNoise" in m.components) == (c.nred > 0)
        lay = build_layout(m, host_toas(n), track_mode=o.track, subtract_mean=o.sub, use_weighted_mean=o.wm)
        assert (lay.spec.track_pn, lay.spec.subtract_mean, lay.spec.weighted_mean) == \
            (int(o.track == "use_pulse_numbers"), int(o.mean), int(o.wm))
        assert lay.nred == c.nred and lay.n == n
        assert ("PHOFF" in lay.columns, "Offset" in lay.columns) == (o.phoff, not o.phoff)
        tab = RC.table_of(lay, n, 1)
        from pint_amd.engine import pack_table
        base = pack_table(lay)
        d0, d1 = RC.f_offsets(n, 1)
        o0, o1 = lay.offsets["F0"], lay.offsets["F1"]
        tl, bl = tab.astype(np.longdouble), base.astype(np.longdouble)
        for oo, d in ((o0, d0), (o1, d1)):  # (the pair's value moved by d, to longdouble's rounding of the value)
            assert abs((tl[oo] - bl[oo]) + (tl[oo + 1] - bl[oo + 1]) - d) <= 2.0 ** -62 * abs(bl[oo]) + 1e-18 * abs(d)
            assert abs(tab[oo + 1]) <= np.spacing(abs(tab[oo])) / 2
        changed = np.flatnonzero(tab != base)
        assert set(changed) <= {o0, o0 + 1, o1, o1 + 1}


@pytest.mark.parametrize("c", [c for c in CASES if c.flow == "fit"], ids=lambda c: c.name)
def test_fit_flow_takes_gram_v(c):
    """The fit flow's models lie on the k_gram_v path by shape_cases.vgram_layout's rules (the
    GPU test asserts n_vgram() == ninst): 20 free bins over the prefix's own span."""
    n = c.ns[0]
    m = RC.model_of(c, False, n)
    P = m._params
    r1 = np.array([float(P["DMXR1_" + t[4:]].value) for t in m.dmx_params()])
    r2 = np.array([float(P["DMXR2_" + t[4:]].value) for t in m.dmx_params()])
    mjd = SC.MJD0 + np.arange(n) * (SC.TSPAN / (RC.N_ALL - 1))
    drow = np.full(n, -1)
    for a in range(len(r1)):
        drow[(mjd >= r1[a]) & (mjd <= r2[a])] = a
    assert np.all(drow >= 0) and len(set(drow)) == SC.BASE_NDMX and min(np.bincount(drow)) >= 16
    sc = SC.Case("resid", c.ntim, SC.BASE_NDMX, c.nred, layout="fit")
    assert SC.vgram_layout(sc, n, drow, 1)[0] == 1


def test_wander():
    """The offsets move the phase by 2 to 4 turns (and a curvature of up to one more span's worth)
    to either side over every case's own rows, for every instance."""
    for n in sorted({n for c in CASES for n in c.ns if n >= 63}):
        for k in range(5):
            full, _ = RC.approx_full(n, k, RC.Opt("use_pulse_numbers", False, True))
            full = full - RC.delta_pulse_numbers()[:n]
            assert 3.0 <= full.max() - full.min() <= 13.0, (n, k, full.min(), full.max())
            assert abs(full).max() <= 9.0, (n, k)


def test_nearest_margin():
    """No pre-rounding phase near a half-integer (approximately; exactly in the GPU test), and
    the `nearest` branch really wraps: rows on both sides of a wrap in every case of >= 63 rows."""
    for c in CASES:
        for n in c.ns:
            for k in range(c.ninst):
                for o in RC.OPTIONS:
                    if o.track != "nearest":
                        continue
                    scale = RC.tile_scale(o) if c.flow == "tiles" else 1.0
                    full, x = RC.approx_full(n, k, o, scale)
                    assert np.min(np.abs(x + 0.5 - np.round(x + 0.5))) > 1e-7, (c.name, n, k, o.name)
                    if n >= 63:
                        assert len(set(np.floor(x + 0.5))) >= 3, (c.name, n, k, o.name)


def _ratio(r, sigma, U, phi):
    """r^T N^-1 r / r^T C^-1 r in float64 (columns normalised as ld_util.ld_woodbury_chi2 does)."""
    w = 1 / sigma ** 2
    s = np.sqrt(np.sum(U * U * w[:, None], axis=0))
    Un = U / s
    Sigma = Un.T @ (Un * w[:, None]) + np.diag(1 / (phi * s * s))
    d = Un.T @ (w * r)
    rNr = np.sum(w * r * r)
    return rNr / (rNr - d @ np.linalg.solve(Sigma, d))


@pytest.mark.parametrize("c", [c for c in CASES if c.flow == "tiles"], ids=lambda c: c.name)
def test_gls_condition(c):
    """r^T N^-1 r / chi2 of the approximate residuals stays below 5 (the GPU test asserts <= 10
    on the device's): cancellation does not eat the GLS bar."""
    from pint_amd.engine import build_layout
    from pint_amd.noise import scaled_sigma_us
    n = c.ns[0]
    toas = host_toas(n)
    for o in RC.OPTIONS:
        m = RC.model_of(c, o.phoff, n)
        lay = build_layout(m, toas, track_mode=o.track, subtract_mean=o.sub, use_weighted_mean=o.wm)
        sigma = scaled_sigma_us(m, toas) * 1e-6
        t = np.asarray(toas.tdbld, dtype=np.float64) * 86400.0
        f = np.asarray(lay.red_freq, dtype=np.float64)
        U = np.zeros((n, 2 * len(f)))
        U[:, ::2] = np.sin(2 * np.pi * t[:, None] * f)
        U[:, 1::2] = np.cos(2 * np.pi * t[:, None] * f)
        phi = np.asarray(lay.red_phi, dtype=np.float64)
        if not o.phoff:
            U = np.concatenate([U, np.ones((n, 1))], axis=1)
            phi = np.concatenate([phi, [1e40]])
        F0 = float(m.F0.value)
        for k in range(c.ninst):
            full, _ = RC.approx_full(n, k, o, RC.tile_scale(o))
            if o.mean:
                w = 1 / sigma ** 2 if o.wm else np.ones(n)
                full = full - np.sum(w * full) / np.sum(w)
            ratio = _ratio(full / F0, sigma, U, phi)
            assert 1 <= ratio <= 5, (o.name, k, ratio)
