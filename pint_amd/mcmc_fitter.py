"""MCMCFitter (reference ``src/pint/mcmc_fitter.py``, its fitting layer): sample the posterior of a
timing model with the EnsembleSampler and leave the model at the maximum-posterior sample, the
uncertainties from the chain.  The ``phaseogram`` plots and the reference's template classes are not
part of this module (PhotonTiming takes a binned template).
"""
from __future__ import annotations

import numpy as np

from .sampler import EnsembleSampler

LD = np.longdouble


class MCMCFitter:
    """MCMCFitter(toas, model, target=None, nwalkers=None, seed=0, prior_info=None, priorerrfact=50.0).

    target : a PointBatch to sample (a PhotonTiming, or a BayesianTiming made by the caller); None: a
        BayesianTiming of (model, toas).  A free parameter without a proper prior then gets a uniform
        one, its value +- priorerrfact x its uncertainty (prior_info supersedes it).
    nwalkers : default 2 nparams + 2, at least 4 (even).
    """

    def __init__(self, toas, model, target=None, nwalkers=None, seed=0, prior_info=None, priorerrfact=50.0,
                 resident=None):
        self.toas, self.model = toas, model
        if target is None:
            from .bayesian import BayesianTiming
            from .pointbatch import _is_unbounded
            info = {}
            for p in model.free_params:
                par = model[p]
                if _is_unbounded(par.prior):
                    u = par.uncertainty_value
                    if not u:
                        raise ValueError(f"free parameter {p} has neither a proper prior nor an uncertainty to make one from")
                    v = float(par.value)
                    info[p] = {"distr": "uniform", "pmin": v - priorerrfact * u, "pmax": v + priorerrfact * u}
            info.update(prior_info or {})
            target = BayesianTiming(model, toas, prior_info=info)
        self.target = target
        self.fitkeys = list(target.param_labels)
        self.n_fit_params = len(self.fitkeys)
        self.fitvals = np.array(getattr(target, "fitvals", target._base_values), dtype=LD)
        errs = getattr(target, "fiterrs", None)
        if errs is None:
            errs = [np.nan if target.model[p].uncertainty_value is None else float(target.model[p].uncertainty_value)
                    for p in self.fitkeys]
        self.fiterrs = np.asarray(errs, dtype=np.float64)
        if nwalkers is None:
            nwalkers = max(4, 2 * self.n_fit_params + 2)
        self.sampler = EnsembleSampler(target, nwalkers, seed=seed, resident=resident)
        self.maxpost = -np.inf
        self.maxpost_fitvals = self.fitvals.copy()
        self.method = "MCMC"

    def lnposterior(self, theta):
        return self.target.lnposterior(theta)

    def fit_toas(self, maxiter=100, pos=None, errfact=0.1):
        """maxiter steps of the sampler from pos (default: the sampler's ball around the model's values,
        the uncertainties x errfact wide).  The model ends at the maximum-posterior sample, its
        uncertainties are the chain's standard deviations after the first quarter; returns the
        log-posterior there."""
        s = self.sampler
        if pos is None:
            if not np.all(np.isfinite(self.fiterrs)):
                raise ValueError("the starting ball needs an uncertainty of every fitted parameter")
            toas = self.toas
            mjds = None if toas is None else np.asarray(toas.get_mjds(), dtype=np.float64)
            kw = {} if mjds is None else {"minMJD": float(mjds.min()), "maxMJD": float(mjds.max())}
            pos = s.get_initial_pos(self.fitkeys, self.fitvals, self.fiterrs, errfact, **kw)
        n0 = len(s.get_log_prob())
        s.run_mcmc(pos, maxiter)
        lnp = s.get_log_prob()[n0:]
        if lnp.size:
            chain = s.get_chain(longdouble=True)[n0:]
            t, w = np.unravel_index(int(np.argmax(lnp)), lnp.shape)
            if lnp[t, w] > self.maxpost:
                self.maxpost = float(lnp[t, w])
                self.maxpost_fitvals = chain[t, w].copy()
            # (the offsets from one sample in longdouble, then rounded: F0's scatter is 1e-13 of its value)
            off = (chain[len(chain) // 4:] - self.maxpost_fitvals).astype(np.float64)
            self.chain_std = np.std(off.reshape(-1, self.n_fit_params), axis=0)
        model_keys = [k for k in self.fitkeys if k in self.model]
        self.model.set_param_values({k: self.maxpost_fitvals[self.fitkeys.index(k)] for k in model_keys})
        if lnp.size:
            for k in model_keys:
                self.model[k].uncertainty_value = float(self.chain_std[self.fitkeys.index(k)])
        return self.maxpost
