"""BayesianTiming (reference ``src/pint/bayesian.py``): the pulsar-timing log-likelihood, prior
and posterior for posterior sampling (MCMC, nested sampling), evaluated in batches on the device.

The reference evaluates one parameter vector per call by rebuilding a Residuals object.  A
sampler wants many independent points per step, so every method here has a batch form that takes
an ``(N, nparams)`` array and returns ``(N,)`` float64; the scalar forms are the batch forms at
N = 1.  ``lnposterior_batch`` works directly as emcee's ``vectorize=True`` callable.

One pulsar stays resident on the device (one Session per object).  A batch installs its N points
as instances with pint_set_points (each point replaces the table entries of every free timing
parameter; a batch of the same N as the last one only forms new tables), runs the evaluation and
the residual pass as grid_chisq does, and then one likelihood pass (pint_point_lnlike) in which
every point scales the TOA errors with its own EFAC / EQUAD (and the DM errors with its own
DMEFAC / DMEQUAD), takes its own weighted mean, and forms

    lnL = -chi2_toa / 2 - sum log sigma_i  [- chi2_dm / 2 - sum log sigma_dm,i  (wideband)]

(bayesian.py:202-252).  Priors and the prior transform are column-wise scipy on the host.

Differences from the reference, all of them documented in DESIGN.md section 4: a NaN log-prior
counts as -inf (the reference's ``in (np.nan, -np.inf)`` test never matches a computed NaN);
``lnposterior`` of a point the device cannot evaluate (e.g. ECC >= 1 under an allowing prior) is
NaN instead of an exception; free parameters must have a slot in the device table or be
EFAC / EQUAD / DMEFAC / DMEQUAD.  The correlated-noise (GLS) likelihood is refused as in the
reference unless ``correlated_noise=True`` is given.

With ``correlated_noise=True`` a model with ECORR, PLRedNoise or PLDMNoise takes the marginalised
likelihood of ``Residuals.lnlikelihood`` (residuals.py:567-716),

    lnL = -r^T C^-1 r / 2 - log det C / 2,   C = N + U Phi U^T,

in one more device pass (pint_point_lnlike_gls) in which every point has its own N (EFAC / EQUAD),
its own ECORR variance per epoch and its own Fourier prior variances (TNREDAMP / TNREDGAM or
RNAMP / RNIDX, TNDMAMP / TNDMGAM), beside its own timing parameters.
"""
from __future__ import annotations

import copy
from typing import Optional

import numpy as np

from .pointbatch import PointBatch

LD = np.longdouble
WHITE = ("EFAC", "EQUAD", "DMEFAC", "DMEQUAD")
RED = ("TNREDAMP", "TNREDGAM", "RNAMP", "RNIDX")
DMN = ("TNDMAMP", "TNDMGAM")
FYR = 1 / 3.16e7  # (noise_model.py powerlaw)
RN_FAC = (86400.0 * 365.24 * 1e6) / (2.0 * np.pi * np.sqrt(3.0))  # RNAMP -> amplitude (noise_model.py:761-768)


def _base(name: str) -> str:
    return name.rstrip("0123456789")


def _pl_scale(amp, gam: float) -> float:
    """powerlaw's factor without the frequencies, amp^2 / 12 / pi^2 fyr^(gam - 3), in the scalar
    types and the order of noise.red_noise_freqs_weights; an overflow gives IEEE's result."""
    try:
        return float(amp ** 2 / 12.0 / np.pi ** 2 * FYR ** (gam - 3))
    except (OverflowError, ZeroDivisionError, ValueError):
        a, g = np.float64(amp), np.float64(gam)
        return float(a ** 2 / 12.0 / np.pi ** 2 * np.float64(FYR) ** (g - 3))


def _rowpow(ff: np.ndarray, e: np.ndarray) -> np.ndarray:
    """(N, len(ff)): ff ** e[k] per row, with the bits of the array-by-scalar power ``ff ** e[k]``:
    numpy's power loop, but for the exponents that ``**`` hands to another loop (square, reciprocal,
    square root, identity, ones), which go through ``**`` row by row."""
    out = np.power(ff[None, :], e[:, None])
    for k in np.nonzero(np.isin(e, (2.0, -1.0, 0.5, 1.0, 0.0)))[0]:
        out[k] = ff ** float(e[k])
    return out


class BayesianTiming(PointBatch):
    """lnprior, prior_transform, lnlikelihood and lnposterior of a timing model and TOAs.

    model : the timing model; a deep copy is kept, its values are the base values of every batch.
    toas : the TOAs (narrowband or wideband).
    use_pulse_numbers : track pulse numbers instead of the nearest integer; TOAs without pulse
        numbers get them from the initial model's phase (TOAs.compute_pulse_numbers).
    prior_info : {name: {"distr": "uniform", "pmin": .., "pmax": ..} or {"distr": "normal",
        "mu": .., "sigma": ..}}; supersedes the priors set on the model's parameters.
    correlated_noise : accept a model with ECORR, PLRedNoise or PLDMNoise and evaluate the marginalised
        likelihood (``likelihood_method == "gls"``); ECORR, TNREDAMP, TNREDGAM (or RNAMP, RNIDX), TNDMAMP
        and TNDMGAM may then be free beside the timing parameters and EFAC / EQUAD.  A model without
        correlated noise takes the white-noise path either way.
    """

    def __init__(self, model, toas, use_pulse_numbers=False, prior_info=None, correlated_noise=False):
        self.model = copy.deepcopy(model)
        self.toas = toas
        if use_pulse_numbers:
            pn = toas.get_pulse_numbers()
            if pn is None or np.any(np.isnan(pn)):
                toas.compute_pulse_numbers(self.model)
        self.track_mode = "use_pulse_numbers" if use_pulse_numbers else "nearest"
        self.is_wideband = toas.is_wideband()
        self.param_labels = self.model.free_params
        self.params = [self.model[p] for p in self.param_labels]
        self.nparams = len(self.param_labels)
        self._apply_prior_info(prior_info)
        self.correlated_noise = bool(correlated_noise)
        self._validate_priors()
        self.likelihood_method = self._decide_likelihood_method()
        self._plan()
        self._dev = None

    # -- construction ------------------------------------------------------------------
    def _decide_likelihood_method(self):
        m = self.model
        if not m.has_correlated_errors:
            return "wls"
        if not self.correlated_noise:
            raise NotImplementedError("GLS likelihood for correlated noise is not yet implemented.")
        if self.is_wideband:
            raise NotImplementedError("The correlated-noise likelihood of wideband TOAs is not implemented.")
        for n in ("TNREDC", "TNDMC"):
            if n in self.param_labels:
                raise NotImplementedError(f"{n} (the number of Fourier modes) cannot be a free parameter.")
        if (not m.has_time_correlated_errors and "PhaseOffset" in m.components
                and "PHOFF" not in self.param_labels):
            # (residuals.py:595-599: _calc_ecorr_chi2 asserts that PHOFF is free)
            raise NotImplementedError("ECORR without time-correlated noise and with a PhaseOffset needs PHOFF "
                                      "to be a free parameter (Residuals._calc_ecorr_chi2).")
        return "gls"

    def _plan(self):
        """Host layout of the pulsar and the split of the free parameters into table entries
        (timing parameters) and white-noise parameters; the white-noise classes."""
        from .engine import build_layout
        from .noisefit import white_noise_classes
        m = self.model
        gls = self.likelihood_method == "gls"
        self.lay = build_layout(m, self.toas, track_mode=self.track_mode, use_gls_basis=gls)
        self._timing = [(j, p) for j, p in enumerate(self.param_labels) if p in self.lay.offsets]
        col = {p: j for j, p in enumerate(self.param_labels)}
        for p in self.param_labels:
            if p in self.lay.offsets or (m[p].kind == "mask" and _base(p) in WHITE):
                continue
            if gls and ((m[p].kind == "mask" and _base(p) == "ECORR") or p in RED or p in DMN):
                continue
            raise NotImplementedError(f"free parameter {p} has no slot in the device table and is not a white-noise "
                                      f"parameter (EFAC, EQUAD, DMEFAC, DMEQUAD): it cannot be sampled")
        self._base_values = np.array([LD(0) if m[p].value is None else LD(m[p].value) for p in self.param_labels], dtype=LD)

        def classes(efac, equad):
            ptr, idx, cef, ceq = white_noise_classes(m, self.toas, efac, equad)
            # per class: its EFACs and EQUADs as (column of the sample array, or -1 and the fixed value)
            ref = lambda n: (col.get(n, -1), float(m[n].value))  # noqa: E731
            return ptr, idx, [[ref(n) for n in c] for c in cef], [[ref(n) for n in c] for c in ceq]
        self._cls = classes("EFAC", "EQUAD")
        self._dmcls = classes("DMEFAC", "DMEQUAD") if self.is_wideband else None
        if gls:
            self._plan_gls(col)

    def _plan_gls(self, col):
        """The sources of the correlated components' prior variances: per ECORR epoch its parameter,
        per Fourier component its amplitude and index, each as (column of the sample array, or -1
        and the fixed value)."""
        m, lay = self.model, self.lay
        ref = lambda n: (col.get(n, -1), float(m[n].value))  # noqa: E731
        self._ones = "PHOFF" not in self.param_labels  # (residuals.py:583-585)
        if 2 * lay.nred + self._ones > 128:
            raise NotImplementedError(f"{2 * lay.nred + self._ones} columns 2 (TNREDC + TNDMC) + the offset column: "
                                      f"the device pass takes at most 128")
        self._ep = [ref(n) for n in (lay.ep_param if getattr(lay, "nep", 0) else [])]
        self._four = []  # (first mode, modes, "tn" | "rn", amplitude, index)
        nr = lay.spec.dmn0 if lay.nred else 0
        if "PLRedNoise" in m.components:
            tn = "TNREDAMP" in m and m["TNREDAMP"].value is not None and m["TNREDGAM"].value is not None
            for n in (("RNAMP", "RNIDX") if tn else ("TNREDAMP", "TNREDGAM")):
                if n in self.param_labels:
                    raise NotImplementedError(f"free parameter {n}: the model's red noise is given by "
                                              f"{'TNREDAMP / TNREDGAM' if tn else 'RNAMP / RNIDX'}")
            a, g = ("TNREDAMP", "TNREDGAM") if tn else ("RNAMP", "RNIDX")
            self._four.append((0, nr, "tn" if tn else "rn", ref(a), ref(g)))
        if "PLDMNoise" in m.components:
            self._four.append((nr, lay.nred - nr, "tn", ref("TNDMAMP"), ref("TNDMGAM")))
        f = np.asarray(lay.red_freq, dtype=np.longdouble) if lay.nred else np.zeros(0, dtype=np.longdouble)
        ff = np.zeros(2 * lay.nred)  # (float64, as red_noise_freqs_weights forms it)
        ff[::2] = f
        ff[1::2] = f
        self._ff = ff

    def _ep_phi(self, v):
        """(N, nep): the ECORR variance (s^2) of every epoch per point (EcorrNoise.get_noise_weights)."""
        out = np.empty((v.shape[0], len(self._ep)))
        for e, (j, fixed) in enumerate(self._ep):
            out[:, e] = (np.asarray(v[:, j], dtype=np.float64) * 1e-6) ** 2 if j >= 0 else (fixed * 1e-6) ** 2
        return out

    def _four_phi(self, v):
        """(N, 2 nmodes): the prior variances of the Fourier modes per point, PLRedNoise then
        PLDMNoise: noise.red_noise_freqs_weights / dm_noise_freqs_weights' expression, operation by
        operation (the scalar powers by the same libm calls), so that it gives their bits."""
        N = v.shape[0]
        out = np.empty((N, len(self._ff)))
        val = lambda r: np.asarray(v[:, r[0]], dtype=np.float64) if r[0] >= 0 else np.full(N, r[1])  # noqa: E731
        with np.errstate(all="ignore"):
            for k0, nm, kind, ra, rg in self._four:
                a, g = val(ra), val(rg)
                if kind == "tn":  # (red_noise_params / dm_noise_params: Python floats)
                    amp = [float(np.float64(10.0) ** np.float64(x)) if abs(x) > 300 else 10.0 ** float(x) for x in a]
                    gam = g
                else:  # (a float over numpy's float64 factor)
                    amp = [float(x) / RN_FAC for x in a]
                    gam = -1.0 * g
                ff = self._ff[2 * k0:2 * (k0 + nm)]
                c = np.array([_pl_scale(x, float(y)) for x, y in zip(amp, gam)])
                out[:, 2 * k0:2 * (k0 + nm)] = c[:, None] * _rowpow(ff, -gam) * ff[0]
        return out

    def _device(self):
        """The resident Session with the pulsar, its wideband data and its noise classes."""
        if self._dev is None:
            from .engine import Session, pack_table
            s = Session()
            try:
                s.set_timing_mask(0)
                lay = s.add(self.lay)
                s.set_noise_classes(lay, self._cls[0], self._cls[1], self.toas.get_errors())
                if self.is_wideband:
                    s.set_wideband(lay)
                    s.set_dm_noise_classes(lay, self._dmcls[0], self._dmcls[1], self.toas.get_dm_errors())
                self._table0 = pack_table(lay, self.model)
            except Exception:
                s.close()
                raise
            self._dev = s
        return self._dev

    # -- prior (lnprior, lnprior_batch and the argument check: PointBatch) ----------------
    def prior_transform_batch(self, cube):
        """Points of the unit hypercube mapped to the prior distribution, (N, nparams) float64."""
        c = np.asarray(cube, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != self.nparams:
            raise IndexError(f"The number of input parameters ({c.shape[-1] if c.ndim else 0}) should be the same "
                             f"as the number of free parameters ({self.nparams}).")
        return np.column_stack([np.asarray(p.prior.ppf(np.ascontiguousarray(c[:, j])), dtype=np.float64)
                                for j, p in enumerate(self.params)]) if self.nparams else np.zeros_like(c)

    def prior_transform(self, cube):
        return self.prior_transform_batch(np.asarray(cube, dtype=np.float64)[None, :])[0]

    # -- likelihood --------------------------------------------------------------------
    @staticmethod
    def _qf(v, cls):
        """(N, ncls, 2): Q^2 = the sum of the class's EQUAD^2, F = the product of its EFACs, per point."""
        _, _, cef, ceq = cls
        out = np.empty((v.shape[0], len(cef), 2))
        val = lambda r: np.asarray(v[:, r[0]], dtype=np.float64) if r[0] >= 0 else r[1]  # noqa: E731
        for c in range(len(cef)):
            q2 = np.zeros(v.shape[0])
            for r in ceq[c]:
                q2 = q2 + val(r) ** 2
            f = np.ones(v.shape[0])
            for r in cef[c]:
                f = f * val(r)
            out[:, c, 0], out[:, c, 1] = q2, f
        return out

    def _extra_point_bytes(self):
        if self.likelihood_method == "gls":  # (class, epoch and Fourier values, outputs)
            return 8.0 * (2 * len(self._cls[2]) + len(self._ep) + len(self._ff) + 4)
        return 0.0

    def lnlikelihood_terms_batch(self, params):
        """(N, 5) of every point; a point the device flags (pint_inst_status) is NaN.
        likelihood_method "wls": lnL, chi2_toa, sum log sigma_toa (s), chi2_dm, sum log sigma_dm (SI, as
        the reference takes it).  "gls": lnL, chi2 = r^T C^-1 r, log det C / 2, log det Sigma, 0."""
        v = self._points(params, True)
        s = self._device()
        out = np.empty((v.shape[0], 5))
        chunk = self._chunk(v.shape[0])
        for c0 in range(0, v.shape[0], chunk):
            vc = v[c0:c0 + chunk]
            flagged = self._eval_points(s, vc)
            if self.likelihood_method == "gls":
                if flagged:
                    bad = s.inst_status() != 0
                g4 = s.point_lnlike_gls(self._qf(vc, self._cls), self._ep_phi(vc) if self._ep else None,
                                        self._four_phi(vc) if len(self._ff) else None, self._ones)
                got = np.zeros((vc.shape[0], 5))
                got[:, :4] = g4
                st = s.inst_status()  # (Sigma not positive definite: already NaN; read to clear)
                got[st != 0] = np.nan
                if flagged:
                    got[bad] = np.nan
            else:
                got = s.point_lnlike(self._qf(vc, self._cls), self._qf(vc, self._dmcls) if self.is_wideband else None)
                got = np.array(got, dtype=np.float64)
                if flagged:
                    got[s.inst_status() != 0] = np.nan
            out[c0:c0 + chunk] = got
        return out

    def lnlikelihood_batch(self, params):
        """The log-likelihood of every point, (N,) (bayesian.py:163-187 at each row)."""
        return self.lnlikelihood_terms_batch(params)[:, 0].copy()

    def lnlikelihood(self, params):
        return float(self.lnlikelihood_batch(self._points(params, False))[0])

    def lnposterior_batch(self, params):
        """lnprior + lnlikelihood of every point, (N,): -inf where the prior is not finite (such a
        point runs at the base values in the batch, so nothing invalid is evaluated on its
        account), NaN where the prior is finite and the device flags the point."""
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
