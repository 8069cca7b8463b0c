"""Prior probability densities of single timing-model parameters (reference
``src/pint/models/priors.py``), on ``scipy.stats``.

A :class:`Prior` wraps a frozen ``scipy.stats`` distribution and evaluates it at plain numbers
in the parameter's par-file unit: ``pdf`` / ``logpdf`` take a scalar or an array, ``ppf`` is the
prior transform of a unit-cube coordinate.  Host code only: priors are cheap, column-wise
numpy / scipy work beside the batched device likelihood (``pint_amd.bayesian``).

The distributions carry the reference's names and meanings:

* ``UniformUnboundedRV()``  -- density 1 everywhere (an improper "no prior"; every parameter's
  default, and refused by ``BayesianTiming`` on a free parameter);
* ``UniformBoundedRV(lo, hi)`` -- uniform on [lo, hi], 0 outside;
* ``GaussianBoundedRV(loc, scale, lower_bound, upper_bound)`` -- the normal density inside the
  bounds and 0 outside (as in the reference, the density is not renormalised over the bounds: a
  sampler needs it only up to a constant);
* ``RandomInclinationPrior()`` -- the density of sin i for an orbit orientation drawn uniformly
  in cos i: p(x) = x / sqrt(1 - x^2) on [0, 1].
"""
from __future__ import annotations

import numpy as np
from scipy.stats import rv_continuous, uniform


def _as_float(value):
    """A scalar as a Python float, an array as float64 (longdouble values are rounded: scipy's
    distributions work in double precision)."""
    if isinstance(value, np.ndarray) and value.ndim > 0:
        return value.astype(np.float64)
    return float(value)


class Prior:
    """A prior density on one parameter: ``Prior(rv)`` with ``rv`` a frozen ``scipy.stats``
    distribution (all shape, location and scale parameters fixed)."""

    def __init__(self, rv):
        self._rv = rv

    def pdf(self, value):
        return self._rv.pdf(_as_float(value))

    def logpdf(self, value):
        return self._rv.logpdf(_as_float(value))

    def ppf(self, q):
        """The value at cumulative probability q (the prior transform of a unit-cube coordinate)."""
        return self._rv.ppf(_as_float(q))

    def __repr__(self):
        rv = self._rv
        name = getattr(getattr(rv, "dist", rv), "name", type(rv).__name__)
        return f"Prior({name}, args={getattr(rv, 'args', ())}, kwds={getattr(rv, 'kwds', {})})"


class UniformUnboundedRV(rv_continuous):
    """Density 1 on the whole real line (no prior at all); not normalisable, so it has no ppf."""

    def _pdf(self, x):
        return np.ones(np.shape(x), dtype=np.float64)

    def _logpdf(self, x):
        return np.zeros(np.shape(x), dtype=np.float64)


def UniformBoundedRV(lower_bound, upper_bound):
    """Uniform between the two bounds, 0 outside (a frozen ``scipy.stats.uniform``)."""
    return uniform(lower_bound, upper_bound - lower_bound)


class _StandardNormalOnInterval(rv_continuous):
    """exp(-x^2 / 2) / sqrt(2 pi) on the support [a, b], 0 outside it."""

    def _pdf(self, x):
        return np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def GaussianBoundedRV(loc=0.0, scale=1.0, lower_bound=-np.inf, upper_bound=np.inf):
    """A normal density of mode ``loc`` and width ``scale`` kept between the two bounds (0
    outside), as a frozen distribution."""
    gen = _StandardNormalOnInterval(name="bounded_gaussian", a=(lower_bound - loc) / scale, b=(upper_bound - loc) / scale)
    return gen(loc=loc, scale=scale)


class RandomInclinationPrior(rv_continuous):
    """p(sin i) for cos i uniform: x / sqrt(1 - x^2) on [0, 1]."""

    def __init__(self, **kwargs):
        kwargs.update(a=0, b=1)
        super().__init__(**kwargs)

    def _pdf(self, x):
        return x / np.sqrt(1.0 - x * x)

    def _logpdf(self, x):
        return np.log(x) - 0.5 * np.log1p(-x * x)

    def _cdf(self, x):
        return 1.0 - np.sqrt(1.0 - x * x)

    def _ppf(self, q):
        return np.sqrt(1.0 - (1.0 - q) ** 2)
