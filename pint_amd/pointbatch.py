"""The point plumbing shared by the batched samplers' targets (BayesianTiming, PhotonTiming): priors
from prior_info, the (N, nparams) argument check, the factorised log-prior and the prior transform,
the chunk size of a batch, the installation and evaluation of a chunk of points on the resident
Session, and the Session's lifetime.

A subclass sets, before it uses any of this: ``model`` (its own copy), ``param_labels``, ``params`` (the
model's Parameter objects whose priors are sampled, the first len(params) columns of a sample array),
``nparams`` (the columns of a sample array), ``lay`` (build_layout's), ``_timing`` ([(column, name)] of
the free parameters with a slot in the device table), ``_table0`` (pack_table's base table, once the
Session exists) and ``_dev`` (None until _device() makes the Session).
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .priors import Prior, UniformUnboundedRV

LD = np.longdouble
EVAL_ERRORS = (L.PINT_E_KEPLER, L.PINT_E_PARAM)


def _is_unbounded(prior) -> bool:
    rv = prior._rv
    return isinstance(rv, UniformUnboundedRV) or isinstance(getattr(rv, "dist", None), UniformUnboundedRV)


class PairPoints(np.ndarray):
    """Points given as (hi, lo) pairs of doubles: a longdouble array (hi + lo rounded to its 64 bits)
    that keeps the pairs themselves in ``pairs`` (float64, the array's shape + (2,)).  A double-double
    value -- an ensemble sampler's walker -- carries ~106 bits, and the device table takes both halves:
    Session.set_points hands on the pairs as they are.  Everything else (priors, noise parameters)
    reads the rounded value.  Indexing and copies keep the pairs in step; assignment writes the
    assigned values' own pairs."""

    def __new__(cls, pairs):
        pairs = np.array(pairs, dtype=np.float64)
        v = np.atleast_1d(pairs[..., 0].astype(LD) + pairs[..., 1].astype(LD))
        # a reader that rounds to double must get hi, the pair's own rounding: where the sum's 64 bits
        # end on a tie that would round away from it, the neighbour towards hi (one longdouble ulp)
        off = v.astype(np.float64) != pairs[..., 0]
        if np.any(off):
            v[off] = np.nextafter(v[off], pairs[..., 0][off].astype(LD))
        obj = np.ascontiguousarray(v.reshape(pairs.shape[:-1])).view(cls)
        obj.pairs = pairs
        return obj

    def __array_finalize__(self, obj):
        self.pairs = None

    def __getitem__(self, idx):
        r = super().__getitem__(idx)
        if isinstance(r, PairPoints) and self.pairs is not None:
            r.pairs = self.pairs[idx]
        return r

    def __setitem__(self, idx, value):
        super().__setitem__(idx, value)
        if self.pairs is not None:
            v = np.asarray(value, dtype=LD)
            hi = v.astype(np.float64)
            self.pairs[idx] = getattr(value, "pairs", None) if getattr(value, "pairs", None) is not None else \
                np.stack([hi, (v - hi.astype(LD)).astype(np.float64)], axis=-1)

    def copy(self, order="C"):
        r = super().copy(order)
        r.pairs = None if self.pairs is None else self.pairs.copy()
        return r


class PointBatch:
    # -- construction ------------------------------------------------------------------
    def _apply_prior_info(self, prior_info):
        from scipy.stats import norm, uniform
        if prior_info is None:
            return
        for par, info in prior_info.items():
            distr = info["distr"]
            if distr == "uniform":
                self.model[par].prior = Prior(uniform(info["pmin"], info["pmax"] - info["pmin"]))
            elif distr == "normal":
                self.model[par].prior = Prior(norm(info["mu"], info["sigma"]))
            else:
                raise NotImplementedError("Only uniform and normal distributions are supported in prior_info.")

    def _validate_priors(self):
        for p in self.params:
            if _is_unbounded(p.prior):
                raise NotImplementedError(f"Unbounded uniform priors are not supported. (param : {p.name})")

    def close(self):
        if getattr(self, "_dev", None) is not None:
            self._dev.close()
            self._dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- arguments ---------------------------------------------------------------------
    def _points(self, params, batch):
        if isinstance(params, PairPoints):
            v = params
        elif batch and isinstance(params, np.ndarray) and params.ndim == 3 and params.shape[1:] == (self.nparams, 2):
            v = PairPoints(params)  # (N, nparams, 2): (hi, lo) pairs
        else:
            v = np.asarray(params)
        if v.dtype != LD:
            v = v.astype(np.float64)
        if not batch:
            if v.ndim != 1 or len(v) != self.nparams:
                raise IndexError(f"The number of input parameters ({len(params)}) should be the same "
                                 f"as the number of free parameters ({self.nparams}).")
            return v[None, :]
        if v.ndim != 2 or v.shape[1] != self.nparams:
            raise IndexError(f"The number of input parameters ({v.shape[-1] if v.ndim else 0}) should be the same "
                             f"as the number of free parameters ({self.nparams}).")
        return v

    # -- prior -------------------------------------------------------------------------
    def _lnprior_sum(self, v):
        """The sum of the parameters' log-priors over the first len(self.params) columns, (N,)."""
        total = np.zeros(v.shape[0])
        with np.errstate(invalid="ignore", divide="ignore"):
            for j, p in enumerate(self.params):
                total = total + np.asarray(p.prior_pdf(np.ascontiguousarray(v[:, j]), logpdf=True), dtype=np.float64)
        return total

    def lnprior_batch(self, params):
        """The factorised log-prior of every point, (N,); -inf where any parameter's is -inf or NaN."""
        total = self._lnprior_sum(self._points(params, True))
        return np.where(np.isnan(total), -np.inf, total)

    def lnprior(self, params):
        return float(self.lnprior_batch(self._points(params, False))[0])

    # -- batches -----------------------------------------------------------------------
    def _extra_point_bytes(self) -> float:
        return 0.0

    def _chunk(self, n):
        from .gridutils import GRID_BATCH_BYTES
        lay = self.lay
        per_pt = 8.0 * (lay.n * (lay.K + 12) + 64 * (lay.K + 2) ** 2) + self._extra_point_bytes()
        return int(max(1, min(n, GRID_BATCH_BYTES // per_pt)))

    def _eval_points(self, s, vc) -> bool:
        """Install the chunk vc of points as the Session's instances and evaluate them; True when the
        device flagged some point (pint_inst_status tells which)."""
        s.set_points(self.lay, self._table0, [p for _, p in self._timing], vc[:, [j for j, _ in self._timing]])
        try:
            s.eval(False)
        except L.PintError as e:
            if e.code not in EVAL_ERRORS:
                raise
            return True
        return False
