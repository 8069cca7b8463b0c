"""The device-resident ensemble sampler (pint_ens_init / pint_ens_run, pint_amd/sampler.py) on the GPU.

* One-step parity against an independent twin written here (its own Philox from test_sampler_host, its
  own draw mapping, proposals in exact rational arithmetic): for every step t of a 25-step resident run
  the twin takes the device's stored state at t - 1, forms the draws, partners and proposals, gets lnq
  from the target's existing lnposterior_batch (given the proposal's (hi, lo) pairs, so that it evaluates
  what the device evaluated), decides, and compares with the chain at t.  Bars: an accepted proposal
  within 1e-30 of the parameter's magnitude of the exact value; its stored lnprob within 1e-9 of the
  twin's; decisions identical, except that a decision whose twin margin |log u - log ratio| is below
  1e-9 may be skipped, at most once per test (expected count over 25 x 130 decisions: ~1e-5).  The
  chain is drained in chunks of 8 steps, so 25 steps cross three chunk boundaries.
* The resident and the host-stepped mode from the same seed and start; determinism and resume;
  rejections (outside the prior: evaluated at the base values, never flagged; flagged by the device:
  counted and never accepted).
* Statistics: the chain's mean and standard deviation of NGC6440E's five parameters against the WLS
  fit's values and uncertainties, at bars set by the chain's own effective sample size, with conditions
  (ESS, acceptance) that a stuck chain cannot meet.
* MCMCFitter.fit_toas: a loose check of the top layer.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_sampler_host import np_philox

pytestmark = pytest.mark.gpu
LD = np.longdouble
M32 = 0xFFFFFFFF


# -- the twin ------------------------------------------------------------------------------------------
def twin_draws(seed, w, t, half, nother, a):
    r = np_philox([w, t & M32, t >> 32, half], [seed & M32, seed >> 32])
    u_z = ((((r[1] << 32) | r[0]) >> 11) + 0.5) * 2.0 ** -53
    s = (a - 1.0) * u_z + 1.0
    return s * s / a, (r[2] * nother) >> 32, (r[3] + 0.5) * 2.0 ** -32


def frac(pair):
    return Fraction(float(pair[0])) + Fraction(float(pair[1]))


def to_pair(fr):
    hi = float(fr)
    return hi, float(fr - Fraction(hi))


def replay(target, p0, pairs, lnprob, seed, a=2.0):
    """Check every decision of a resident run (pairs (T, W, d, 2), lnprob (T, W)) from the start p0
    ((W, d, 2)); returns (decisions, accepted, skipped)."""
    T, W, d, _ = pairs.shape
    h = W // 2
    prev, lnp_prev = p0, np.asarray(target.lnposterior_batch(np.ascontiguousarray(p0)))
    skipped = accepted = 0
    for t in range(T):
        for half in (0, 1):
            other = prev if half == 0 else pairs[t]  # (the second half moves against the first half's new state)
            dr = [twin_draws(seed, half * h + i, t, half, h, a) for i in range(h)]
            exact = [[frac(other[(1 - half) * h + j, c]) + Fraction(z) * (frac(prev[half * h + i, c]) -
                                                                        frac(other[(1 - half) * h + j, c]))
                      for c in range(d)] for i, (z, j, _) in enumerate(dr)]
            prop = np.array([[to_pair(y) for y in row] for row in exact])
            with np.errstate(invalid="ignore"):
                lnq = np.asarray(target.lnposterior_batch(np.ascontiguousarray(prop)), dtype=np.float64)
            for i, (z, j, u) in enumerate(dr):
                w = half * h + i
                dev_acc = not np.array_equal(pairs[t, w], prev[w])
                margin = math.log(u) - ((d - 1) * math.log(z) + lnq[i] - lnp_prev[w]) if np.isfinite(lnq[i]) else np.inf
                if abs(margin) < 1e-9:
                    skipped += 1
                else:
                    assert dev_acc == (margin < 0), (t, w, margin, lnq[i], lnp_prev[w])
                if dev_acc:
                    accepted += 1
                    for c in range(d):
                        mag = max(abs(frac(prev[w, c])), abs(frac(other[(1 - half) * h + j, c])))
                        assert abs(frac(pairs[t, w, c]) - exact[i][c]) <= mag * Fraction(1, 10 ** 30), (t, w, c)
                    assert abs(lnprob[t, w] - lnq[i]) <= 1e-9, (t, w, lnprob[t, w], lnq[i])
                else:
                    assert lnprob[t, w] == lnp_prev[w]
        prev, lnp_prev = pairs[t], lnprob[t]
    assert skipped <= 1
    return 2 * h * T, accepted, skipped


def ball(pts, W, seed, width=0.2):
    """W starting positions (longdouble) around the mean of a fixture's points, width x their scatter."""
    c, s = pts.mean(axis=0), pts.astype(np.float64).std(axis=0)
    return c + (width * s * np.random.default_rng(seed).standard_normal((W, pts.shape[1]))).astype(LD)


def nb_target(name="bayes_nb"):
    from test_bayesian import bayes, _pts
    bt, z, meta, perm = bayes(name)
    return bt, _pts(z, "pts", perm)


def photon_target():
    """photon_geo with F0 and A1 left at the default unbounded prior, and the PHASE column."""
    import photon_util
    from pint_amd import PhotonTiming
    model, toas, z, meta = photon_util.load("photon_geo")
    info = {k: v for k, v in meta["prior_info"].items() if k not in ("F0", "A1")}
    pt = PhotonTiming(model, toas, z["tmpl"], weights=z.get("weights"), prior_info=info)
    return pt, photon_util.points(pt, z, meta)


@pytest.mark.parametrize("case,W", [("bayes_nb", 4), ("bayes_nb", 6), ("bayes_nb", 130), ("bayes_wb", 6), ("photon", 6)])
def test_one_step_parity(case, W):
    from pint_amd import EnsembleSampler
    from pint_amd.sampler import split_pairs
    target, pts = photon_target() if case == "photon" else nb_target(case)
    try:
        if case == "photon":
            assert target.param_labels[-1] == "PHASE"
        pos = ball(pts, W, seed=W)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (fewer than 2 nparams walkers, on purpose)
            s = EnsembleSampler(target, W, seed=20 + W, resident=True, chunk=8)
        s.run_mcmc(pos, 25)
        pairs, lnprob = s.get_chain_pairs(), s.get_log_prob()
        assert pairs.shape == (25, W, target.nparams, 2) and np.all(np.isfinite(lnprob))
        n, acc, skipped = replay(target, split_pairs(pos), pairs, lnprob, 20 + W)
        print(f"{case} W={W}: {n} decisions, {acc} accepted, {skipped} skipped")
        assert 0 < acc < n
        assert int(round(float(np.sum(s.acceptance_fraction)) * 25)) == acc
        s.close()
    finally:
        target.close()


def test_both_modes_agree():
    """resident=True and resident=False from the same seed and start: the same decisions and positions."""
    import warnings
    from pint_amd import EnsembleSampler
    from pint_amd.sampler import split_pairs
    target, pts = nb_target()
    try:
        pos = ball(pts, 6, seed=1)
        out = []
        for resident in (True, False):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                s = EnsembleSampler(target, 6, seed=77, resident=resident, chunk=8)
            assert s.resident is resident
            s.run_mcmc(pos, 25)
            out.append((s.get_chain_pairs(), s.get_log_prob(), s.acceptance_fraction))
            s.close()
        (pd, ld, ad), (ph, lh, ah) = out
        x0 = split_pairs(pos)[None]
        moved = lambda p: np.any(p != np.concatenate([x0, p[:-1]]), axis=(2, 3))  # noqa: E731  (T, W): accepted
        same = np.all(moved(pd) == moved(ph), axis=1)
        upto = 25 if same.all() else int(np.argmin(same))
        print(f"the two modes agree over {upto} of 25 steps")
        assert upto >= 10
        if upto < 25:  # only at a decision on the edge: the margin of the first differing walker
            t = upto
            w = int(np.argmax(np.any(pd[t] != ph[t], axis=(1, 2))))
            half, d = w // 3, target.nparams
            z, _, u = twin_draws(77, w, t, half, 3, 2.0)
            lnq = ld[t, w] if ld[t, w] != ld[t - 1, w] else lh[t, w]
            assert abs(math.log(u) - ((d - 1) * math.log(z) + lnq - ld[t - 1, w])) < 1e-9
        for t in range(upto):
            for w in range(6):
                for c in range(target.nparams):
                    a, b = frac(pd[t, w, c]), frac(ph[t, w, c])
                    assert abs(a - b) <= abs(a) * Fraction(1, 10 ** 30)
        assert np.max(np.abs(ld[:upto] - lh[:upto])) <= 1e-9
        if upto == 25:
            assert np.array_equal(ad, ah)
    finally:
        target.close()


def test_gls_target_is_host_stepped():
    import warnings
    from test_bayesian_gls import bayes, _pts
    from pint_amd import EnsembleSampler
    bt, z, meta, perm = bayes("bayes_gls_red")
    try:
        with pytest.raises(NotImplementedError):
            EnsembleSampler(bt, 6, resident=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            s = EnsembleSampler(bt, 6, seed=3)
        assert s.resident is False
        s.run_mcmc(ball(_pts(z, "pts", perm), 6, seed=3), 5)
        pairs, lp = s.get_chain_pairs(), s.get_log_prob()
        again = bt.lnposterior_batch(np.ascontiguousarray(pairs.reshape(-1, bt.nparams, 2))).reshape(lp.shape)
        assert np.all(np.isfinite(lp)) and np.max(np.abs(lp - again)) <= 1e-9
        assert np.any(s.acceptance_fraction > 0)
    finally:
        bt.close()


def test_determinism_and_resume():
    from pint_amd import EnsembleSampler
    target, pts = nb_target()
    try:
        pos = ball(pts, 40, seed=9)

        def run(seed, parts):
            s = EnsembleSampler(target, 40, seed=seed, resident=True, chunk=8)
            s.run_mcmc(pos, parts[0])
            for n in parts[1:]:
                # (the target is used in between: the sampler installs its batch again)
                target.lnposterior_batch(pts[:5])
                s.run_mcmc(None, n)
            out = s.get_chain_pairs(), s.get_log_prob(), s.acceptance_fraction
            s.close()
            return out
        a, b, c, d = run(5, [25]), run(5, [25]), run(5, [10, 15]), run(6, [25])
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        for x, y in zip(a, c):
            assert np.array_equal(x, y)
        assert not np.array_equal(a[0], d[0])
    finally:
        target.close()


def test_prior_box_rejections():
    """A box in four parameters with the walkers started near its two ends: about half the first
    proposals fall outside it.  No stored sample is outside, every stored lnprob is finite, and nothing
    is flagged (the marked walkers ran at the base values)."""
    from test_bayesian import load
    from pint_amd import BayesianTiming, EnsembleSampler
    from pint_amd import sampler as S
    bt0, pts = nb_target()
    labels = list(bt0.param_labels)
    bt0.close()
    W = 40
    pos = ball(pts, W, seed=4)
    model, toas, z, meta = load("bayes_nb")
    info = dict(meta["prior_info"])
    rng = np.random.default_rng(5)
    mid, sd = pts.mean(axis=0), pts.astype(np.float64).std(axis=0)
    box = {}
    for p in ("F0", "A1", "TASC", "RAJ"):
        c = labels.index(p)
        half = LD(0.2 * sd[c])
        pos[:, c] = mid[c] + half * (rng.choice([-1.0, 1.0], W) * rng.uniform(0.6, 0.99, W)).astype(LD)
        box[c] = (float(mid[c] - half), float(mid[c] + half))
        info[p] = {"distr": "uniform", "pmin": box[c][0], "pmax": box[c][1]}
    bt = BayesianTiming(model, toas, prior_info=info)
    try:
        assert list(bt.param_labels) == labels
        s = EnsembleSampler(bt, W, seed=8, resident=True)
        s.run_mcmc(pos, 20)
        # the first half-step's proposals, from the sampler's own twin of the draws
        x = S.split_pairs(pos)
        u_z, idx, _ = S.draws(8, np.arange(W // 2), 0, 0, W // 2)
        xj = x[W // 2 + idx]
        yh, _ = S.propose(x[:W // 2, :, 0], x[:W // 2, :, 1], xj[:, :, 0], xj[:, :, 1], S.stretch(2.0, u_z)[:, None])
        out = np.zeros(W // 2, dtype=bool)
        for c, (lo, hi) in box.items():
            out |= (yh[:, c] < lo) | (yh[:, c] > hi)
        print(f"{out.mean():.2f} of the first proposals outside the box")
        assert 0.2 <= out.mean() <= 0.8
        chain, lp = s.get_chain(), s.get_log_prob()
        for c, (lo, hi) in box.items():
            assert np.all((chain[:, :, c] >= lo) & (chain[:, :, c] <= hi))
        assert np.all(np.isfinite(lp)) and np.all(s.n_flagged == 0)
        first = np.any(s.get_chain_pairs()[0, :W // 2] != x[:W // 2], axis=(1, 2))
        assert not np.any(first & out)  # none of the outside proposals was accepted
        assert 0 < s.acceptance_fraction.mean() < 1
        s.close()
    finally:
        bt.close()


def test_flagged_proposals_are_counted_and_rejected():
    """ECC walkers spread below 1 under a prior that allows ECC up to 2: the proposals beyond 1 are
    flagged by the device, counted in n_flagged and never accepted."""
    from golden_util import load as gload
    from test_bayesian import _par
    from pint_amd import BayesianTiming, EnsembleSampler, get_model
    _, toas, _, _ = gload("pta_dd")
    par = "\n".join(l for l in _par("pta_dd").splitlines() if not l.startswith(("TNRed", "TNRED"))) + "\n"
    model = get_model(par)
    model.free_params = ["F0", "ECC"]
    f0 = LD(model.F0.value)
    bt = BayesianTiming(model, toas, prior_info={"F0": {"distr": "uniform", "pmin": float(f0) - 1e-9, "pmax": float(f0) + 1e-9},
                                                 "ECC": {"distr": "uniform", "pmin": 0.0, "pmax": 2.0}})
    try:
        labels = list(bt.param_labels)
        W = 16
        rng = np.random.default_rng(3)
        pos = np.empty((W, 2), dtype=LD)
        pos[:, labels.index("F0")] = f0 + LD(1e-12) * rng.standard_normal(W)
        pos[:, labels.index("ECC")] = rng.uniform(0.6, 0.95, W)
        s = EnsembleSampler(bt, W, seed=2, resident=True)
        s.run_mcmc(pos, 12)
        ecc, lp = s.get_chain()[:, :, labels.index("ECC")], s.get_log_prob()
        print(f"flagged {int(s.n_flagged.sum())}, accepted {int(round(s.acceptance_fraction.sum() * 12))} of {12 * W}")
        assert s.n_flagged.sum() > 0
        assert np.all(ecc < 1.0) and np.all(np.isfinite(lp))
        s.close()
    finally:
        bt.close()


# -- statistics ------------------------------------------------------------------------------------------
_NGC = {}


def ngc_fit():
    """NGC6440E, its WLS fit run to convergence (values, uncertainties) and a BayesianTiming with uniform
    priors +- 50 sigma around it: made once, shared, not changed."""
    if not _NGC:
        from golden_util import load as gload
        from pint_amd import BayesianTiming, WLSFitter
        model, toas, _, _ = gload("ngc6440e")
        f = WLSFitter(toas, model)
        f.fit_toas(maxiter=6)
        m = f.model
        names = list(m.free_params)
        val = np.array([LD(m[p].value) for p in names], dtype=LD)
        sig = np.array([float(m[p].uncertainty_value) for p in names])
        info = {p: {"distr": "uniform", "pmin": float(v) - 50 * s, "pmax": float(v) + 50 * s} for p, v, s in zip(names, val, sig)}
        bt = BayesianTiming(m, toas, prior_info=info)
        _NGC.update(model=m, toas=toas, names=names, val=val, sig=sig, bt=bt)
    return _NGC


def test_chain_statistics_against_the_wls_fit():
    """W = 64, 300 burn-in + 1500 kept steps from get_initial_pos (errfact 0.1).  Per parameter
    |mean - fit| < 4 sigma / sqrt(ESS) and |std / sigma - 1| < 4 / sqrt(2 ESS) + 2 % (the model's
    non-linearity), ESS = 64 x 1500 / tau with tau from integrated_time on the kept chain; and so that a
    stuck chain cannot pass by inflating its own bar: ESS >= 400 for every parameter, acceptance
    fraction within 0.2-0.8."""
    from pint_amd import EnsembleSampler, integrated_time
    g = ngc_fit()
    bt, names, val, sig = g["bt"], g["names"], g["val"], g["sig"]
    order = [names.index(p) for p in bt.param_labels]
    val, sig = val[order], sig[order]
    s = EnsembleSampler(bt, 64, seed=2024, resident=True)
    pos = s.get_initial_pos(list(bt.param_labels), val, sig, 0.1)
    s.run_mcmc(pos, 1800)
    kept = (s.get_chain(longdouble=True, discard=300) - val).astype(np.float64) / sig  # in units of the fit's sigma
    tau = integrated_time(kept)
    ess = 64 * 1500 / tau
    acc = float(np.mean(s.acceptance_fraction))
    mean, std = kept.reshape(-1, len(val)).mean(axis=0), kept.reshape(-1, len(val)).std(axis=0)
    for p, t, e, m, sd in zip(bt.param_labels, tau, ess, mean, std):
        print(f"{p}: tau {t:.1f}, ESS {e:.0f}, mean {m:+.4f} sigma (bar {4 / np.sqrt(e):.4f}), std/sigma {sd:.4f} "
              f"(bar {4 / np.sqrt(2 * e) + 0.02:.4f})")
    print(f"acceptance fraction {acc:.3f}")
    s.close()
    assert np.all(ess >= 400)
    assert 0.2 <= acc <= 0.8
    assert np.all(np.abs(mean) < 4 / np.sqrt(ess))
    assert np.all(np.abs(std - 1) < 4 / np.sqrt(2 * ess) + 0.02)


def test_mcmc_fitter():
    """The top layer: the model ends within 0.5 sigma of the WLS fit in every parameter, its
    uncertainties within 25 % of the fit's (200 steps, W = 32)."""
    import copy
    from pint_amd import MCMCFitter
    g = ngc_fit()
    model = copy.deepcopy(g["model"])
    f = MCMCFitter(g["toas"], model, nwalkers=32, seed=1)
    try:
        assert f.sampler.resident
        post = f.fit_toas(maxiter=200)
        assert np.isfinite(post) and post == f.maxpost and abs(post - f.lnposterior(f.maxpost_fitvals)) < 1e-4
        for p, v, sg in zip(g["names"], g["val"], g["sig"]):
            dv = float(LD(model[p].value) - v) / sg
            ru = float(model[p].uncertainty_value) / sg
            print(f"{p}: {dv:+.3f} sigma from the fit, uncertainty x {ru:.3f}")
            assert abs(dv) < 0.5 and abs(ru - 1) < 0.25
    finally:
        f.sampler.close()
        f.target.close()
