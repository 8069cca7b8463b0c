"""The photon-event likelihood (reference ``src/pint/scripts/event_optimize.py``): Gaussian templates,
the template likelihood of photon phases and its scan over a phase offset, and PhotonTiming -- what the
reference's ``emcee_fitter`` evaluates one parameter vector at a time, here for N points per call on
the device.

The likelihood of photon phases phi_i with weights w_i under a binned template T (Pletsch & Clark 2015,
eq. 2) is

    lnL(phs) = sum_i log(w_i T((phi_i + phs) mod 1) + 1 - w_i)          (sum_i log T(.) without weights)

with T = np.interp(x, arange(L) / L, template, right=template[0]): linear between the bins' nodes and
the constant template[0] beyond the last node.  A sampler moves the timing parameters and the offset
PHASE; each point needs a fresh model phase for every photon.  PhotonTiming keeps the pulsar resident
on the device (one Session), installs the N points with pint_set_points, evaluates them, and the
likelihood pass (pint_point_photon_lnlike) or the trigonometric sums of the H-test
(pint_point_photon_trig) consume the phases where they are: only N (or N x offsets) doubles come back.

Out of scope: FITS and spacecraft-orbit loading, analytic LCTemplate primitives and energy-dependent
templates, the emcee driver itself (``lnposterior_batch`` is emcee's ``vectorize=True`` callable),
fftfit (``marginalize_over_phase(fftfit=True)`` is refused) and plots.
"""
from __future__ import annotations

import copy

import numpy as np

from . import _lib as L
from .pointbatch import PointBatch

LD = np.longdouble
FWHM_PER_SIGMA = 2.35482  # (the reference's rounding of 2 sqrt(2 ln 2))


def gaussian_profile(N: int, phase: float, fwhm: float):
    """A Gaussian pulse of unit integrated flux sampled at the N phases j / N: centred on
    ``phase`` (mod 1), taken at the nearest image of every bin, and zero beyond 20 sigma."""
    sigma = fwhm / FWHM_PER_SIGMA
    mean = phase % 1.0
    x = np.arange(N, dtype=np.float64) / float(N)
    # each bin's image nearest to the peak: one turn down for bins more than half a turn above it, one
    # turn up for bins more than half a turn below it (at most one of the two applies to a mean in [0, 1))
    x = x - (x > mean + 0.5) + (x < mean - 0.5)
    z = (x - mean) / sigma
    norm = sigma * np.sqrt(2 * np.pi)
    with np.errstate(under="ignore"):
        return np.where(np.abs(z) < 20.0, np.exp(-0.5 * z ** 2.0) / norm, 0.0)


def read_gaussfitfile(gaussfitfile, proflen: int):
    """The template of ``proflen`` bins of a Gaussian-fit file (pygaussfit.py's output: lines
    ``phasN = value +/- err``, ``amplN = ...``, ``fwhmN = ...``): the components summed, the strongest
    one moved to phase 0.  A path or an open text file."""
    lines = gaussfitfile.readlines() if hasattr(gaussfitfile, "readlines") else open(gaussfitfile).readlines()
    vals = {"phas": [], "ampl": [], "fwhm": []}
    for line in lines:
        key = line.lstrip()[:4]
        if key in vals:
            vals[key].append(float(line.split()[2]))
    if not (len(vals["phas"]) == len(vals["ampl"]) == len(vals["fwhm"])):
        raise ValueError(f"Number of phases, amplitudes, and FWHMs are not the same in '{gaussfitfile}'!")
    ph, am, fw = (np.asarray(vals[k]) for k in ("phas", "ampl", "fwhm"))
    order = np.argsort(am)[::-1]
    ph, am, fw = ph[order], am[order], fw[order]
    if len(ph):
        ph = (ph - ph[0]) % 1
    template = np.zeros(proflen, dtype=np.float64)
    for p, a, f in zip(ph, am, fw):
        template += a * gaussian_profile(proflen, p, f)
    return template


def profile_likelihood(phs, xvals, phases, template, weights):
    """lnL of the phases shifted by phs (the module docstring's expression) on the host."""
    x = np.asarray(phases).astype(np.float64) + np.float64(phs)
    x %= 1
    probs = np.interp(x, xvals, template, right=template[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(probs).sum() if weights is None else np.log(weights * probs + 1.0 - weights).sum()


def _scan_offsets(lophs, hiphs, resolution):
    return np.arange(lophs, hiphs, resolution)


def bins_of_offset(offset, nbin):
    """marginalize_over_phase's first result: a phase offset as a shift in template bins, counted the
    other way round (offset 0 -> nbin, offset -> 1 gives 0)."""
    return nbin - offset * nbin


def marginalize_over_phase(phases, template, weights=None, resolution=1.0 / 1024, minimize=True, fftfit=False,
                           showplot=False, lophs=0.0, hiphs=1.0):
    """The phase offset (in template bins, ``L - offset L``) that maximises the template likelihood of
    the phases, and that likelihood: a scan of arange(lophs, hiphs, resolution), refined with
    scipy.optimize.minimize within +-0.03 of a 1/64 scan when ``minimize``."""
    if fftfit:
        raise NotImplementedError("marginalize_over_phase(fftfit=True): fftfit is not built")
    if showplot:
        raise NotImplementedError("marginalize_over_phase(showplot=True): plots are not built")
    template = np.asarray(template, dtype=np.float64)
    L_ = len(template)
    xtemp = np.arange(L_) * 1.0 / L_
    if minimize:
        import scipy.optimize as op
        phs, _ = marginalize_over_phase(phases, template, weights, resolution=1.0 / 64, minimize=False)
        phs = 1.0 - phs / L_
        res = op.minimize(lambda p: -profile_likelihood(p[0], xtemp, phases, template, weights), [phs],
                          bounds=[[phs - 0.03, phs + 0.03]])
        return bins_of_offset(res["x"], L_), -res["fun"]
    # the scan is profile_likelihood at every offset (for phases in [0, 1) and offsets in [0, 1) its
    # mod 1 is the reference's "subtract 1 above 1": both leave 1.0 itself to the template's right value)
    offsets = _scan_offsets(lophs, hiphs, resolution)
    lnl = np.array([profile_likelihood(d, xtemp, phases, template, weights) for d in offsets])
    best = int(np.argmax(lnl))
    return bins_of_offset(offsets[best], L_), lnl[best]


class PhotonTiming(PointBatch):
    """lnprior, lnlikelihood and lnposterior of a timing model, photon TOAs and a binned template, and
    the H-test and the phase scan of many points at once.

    model : the timing model; a deep copy is kept, its values are the base values of every batch.
    toas : the photons (get_event_TOAs, or any TOAs); with an AbsPhase component in the model the photon
        phase is relative to the TZR TOA, as model.phase(toas) takes it.
    template : the template's values at the phases j / len(template), at most 4096 bins; None: only
        the H-test (htest_batch) and the phases are available.
    weights : one per photon, or None.
    prior_info : as for BayesianTiming; supersedes the priors set on the model's parameters.
    phs, phserr : the starting value and scale of PHASE (fitvals / fiterrs, as emcee_fitter keeps them).

    param_labels are the model's free parameters with a slot in the device table, then "PHASE";
    PHASE is uniform on [0, 1] (emcee_fitter.lnprior).  Unlike BayesianTiming the timing parameters may
    keep the default unbounded prior: the reference's event sampler accepts it (log-prior 0).
    """

    def __init__(self, model, toas, template, weights=None, prior_info=None, phs=0.0, phserr=0.03):
        from .engine import build_layout
        self.model = copy.deepcopy(model)
        self.toas = toas
        self.template = None if template is None else np.ascontiguousarray(template, dtype=np.float64)
        if self.template is not None and (self.template.ndim != 1 or not 1 <= self.template.size <= L.MAX_TEMPLATE):
            raise ValueError(f"the template must hold 1..{L.MAX_TEMPLATE} bins, got {self.template.shape}")
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if self.weights is not None and self.weights.shape != (toas.ntoas,):
            raise ValueError(f"weights must have one value per photon ({toas.ntoas}), got {self.weights.shape}")
        self._apply_prior_info(prior_info)
        free = list(self.model.free_params)
        frozen = copy.deepcopy(self.model)  # (the table's entries do not depend on what is free)
        frozen.free_params = []
        slots = build_layout(frozen, toas, track_mode="nearest", use_gls_basis=False).offsets
        for p in free:
            if p not in slots:
                raise NotImplementedError(f"free parameter {p} has no slot in the device table: it cannot be sampled")
        self.lay = build_layout(self.model, toas, track_mode="nearest", use_gls_basis=False)
        self.param_labels = free + ["PHASE"]
        self.params = [self.model[p] for p in free]
        self.nparams = len(self.param_labels)
        self._timing = list(enumerate(free))
        self.abs_phase = "AbsPhase" in self.model.components
        self.fitkeys = list(self.param_labels)
        val = lambda p: LD(0) if self.model[p].value is None else LD(self.model[p].value)  # noqa: E731
        self.fitvals = np.array([val(p) for p in free] + [LD(phs)], dtype=LD)
        unc = lambda p: getattr(self.model[p], "uncertainty_value", None)  # noqa: E731
        self.fiterrs = np.array([np.nan if unc(p) is None else float(unc(p)) for p in free] + [float(phserr)])
        self._base_values = self.fitvals
        self._dev = None

    def _device(self):
        if self._dev is None:
            from .engine import Session, pack_table
            s = Session()
            try:
                s.set_timing_mask(0)
                lay = s.add(self.lay)
                s.set_photons(lay, self.weights, self.template, self.abs_phase)
                self._table0 = pack_table(lay, self.model)
            except Exception:
                s.close()
                raise
            self._dev = s
        return self._dev

    def _extra_point_bytes(self):
        return 8.0 * (2 * L.MAX_PHOTON_HARM + 2)

    # -- prior -------------------------------------------------------------------------
    def lnprior_batch(self, params):
        """The parameters' log-priors, and PHASE uniform on [0, 1]: -inf outside (and where any
        parameter's prior is -inf or NaN)."""
        v = self._points(params, True)
        total = self._lnprior_sum(v)
        ph = np.asarray(v[:, -1], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            bad = np.isnan(total) | (ph > 1.0) | (ph < 0.0)
        return np.where(bad, -np.inf, total)

    # -- device passes -----------------------------------------------------------------
    def _run(self, v, width, fn):
        """fn(session, chunk of points) -> (chunk, width) for every chunk of v; a point the device flags
        (pint_inst_status) is NaN."""
        s = self._device()
        out = np.empty((v.shape[0], width))
        chunk = self._chunk(v.shape[0])
        for c0 in range(0, v.shape[0], chunk):
            vc = v[c0:c0 + chunk]
            flagged = self._eval_points(s, vc)
            got = np.array(fn(s, vc), dtype=np.float64).reshape(vc.shape[0], width)
            if flagged:
                got[s.inst_status() != 0] = np.nan
            out[c0:c0 + chunk] = got
        return out

    def _need_template(self):
        if self.template is None:
            raise ValueError("this PhotonTiming has no template: only htest_batch and get_event_phases are available")

    def lnlikelihood_batch(self, params):
        """The template log-likelihood of every point at its own PHASE, (N,)."""
        self._need_template()
        v = self._points(params, True)
        return self._run(v, 1, lambda s, vc: s.point_photon_lnlike(np.asarray(vc[:, -1], dtype=np.float64)))[:, 0]

    def lnlikelihood(self, params):
        return float(self.lnlikelihood_batch(self._points(params, False))[0])

    def lnposterior_batch(self, params):
        """lnprior + lnlikelihood of every point, (N,): -inf where the prior is not finite (such a point
        runs at the base values in the batch), NaN where the device flags the point."""
        v = self._points(params, True)
        lp = self.lnprior_batch(v)
        ok = np.isfinite(lp)
        if not ok.all():
            v = v.copy()
            v[~ok] = self._base_values.astype(v.dtype)
        with np.errstate(invalid="ignore"):
            return np.where(ok, lp + self.lnlikelihood_batch(v), -np.inf)

    def lnposterior(self, params):
        return float(self.lnposterior_batch(self._points(params, False))[0])

    __call__ = lnposterior_batch

    def htest_batch(self, params, m=20, c=4):
        """(H, Z^2): the (weighted) H statistic (N,) and the Z^2_k for k = 1..m (N, m) of every point's
        photon phases, from the device's trigonometric sums (PHASE does not enter)."""
        from . import eventstats as es
        m = int(m)
        v = self._points(params, True)
        sums = self._run(v, 2 * m + 2, lambda s, vc: s.point_photon_trig(m))
        if self.weights is None:
            return es.hm(None, m, c, sums=sums), es.z2m(None, m, sums=sums)
        return es.hmw(None, None, m, c, sums=sums), es.z2mw(None, None, m, sums=sums)

    def phase_scan(self, params, resolution=1.0 / 1024):
        """marginalize_over_phase(minimize=False) of every point: (offset in template bins (N,), the
        largest log-likelihood (N,), the scan (N, nphs)) over the offsets arange(0, 1, resolution);
        PHASE does not enter.  One evaluation per point serves all its offsets."""
        self._need_template()
        d = _scan_offsets(0.0, 1.0, resolution)
        if not 1 <= d.size <= L.MAX_PHOTON_PHS:
            raise ValueError(f"resolution {resolution}: {d.size} offsets per point (1..{L.MAX_PHOTON_PHS})")
        v = self._points(params, True)
        scan = self._run(v, d.size, lambda s, vc: s.point_photon_lnlike(np.tile(d, (vc.shape[0], 1))))
        Lb = self.template.size
        with np.errstate(invalid="ignore"):
            best = np.array([np.argmax(r) for r in scan])
        return bins_of_offset(d[best], Lb), scan[np.arange(len(scan)), best], scan

    def get_event_phases(self, params=None):
        """The photon phases in [0, 1) (float64): model.phase(toas).frac % 1 at the base values (n,), or
        at every point of ``params`` (N, n).  This reads 16 B per photon and point back from the device:
        the batch methods above do not."""
        v = self._base_values[None, :] if params is None else self._points(params, np.ndim(params) == 2)
        s = self._device()
        out = np.empty((v.shape[0], self.lay.n))
        chunk = self._chunk(v.shape[0])
        for c0 in range(0, v.shape[0], chunk):
            vc = v[c0:c0 + chunk]
            flagged = self._eval_points(s, vc)
            hi, lo, _, _ = s.read_eval()
            for k in range(vc.shape[0]):
                # the integer parts first (hi - floor(hi) is exact in float64, and integers do not enter
                # the fraction of a difference): the sum hi + lo of a phase of ~3e10 cycles would be rounded
                # to the longdouble's ulp there, 3.5e-9 cycles
                h, l = LD(hi[k] - np.floor(hi[k])), LD(lo[k])
                a, b = (h[:-1] - h[-1], l[:-1] - l[-1]) if self.abs_phase else (h[:-1], l[:-1])
                d = a + b
                f = (d - np.floor(d)).astype(np.float64)
                out[c0 + k] = np.where(f >= 1.0, np.nextafter(1.0, 0.0), f)
            if flagged:
                out[c0:c0 + chunk][s.inst_status() != 0] = np.nan
        return out[0] if params is None or np.ndim(params) == 1 else out
