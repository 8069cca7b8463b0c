"""EnsembleSampler: Goodman & Weare's affine-invariant stretch move in the red/blue half-ensemble
form (what the reference's ``pint.sampler.EmceeSampler`` gets from emcee), for the batched posteriors
of this package (any ``PointBatch``: BayesianTiming, PhotonTiming).

Two modes that run the same algorithm on the same random numbers:

* resident (``pint_ens_init`` / ``pint_ens_run``): walkers, proposals, priors, the accept test and the
  chain live on the device; per half-step the library enqueues propose -> tables -> evaluation ->
  likelihood -> accept and nothing crosses to the host between steps.  Targets: BayesianTiming with
  ``likelihood_method == "wls"`` (narrowband or wideband) and PhotonTiming with a template.
* host-stepped: a numpy loop over ``target.lnposterior_batch``; works for every target, the
  correlated-noise (GLS) likelihood included.

The walkers are double-double (hi, lo) pairs in both modes; a proposal y = x_j + z (x_k - x_j) is
formed in double-double, so that a parameter known to 1e-13 (F0) is not quantised by the move.  The
random numbers are Philox4x32-10 blocks keyed by the seed and counted by (walker, step, half)
(csrc/ensemble.hpp): a chain is a function of the seed, the start and the step
numbers, ``run_mcmc(p, 10); run_mcmc(None, 15)`` gives the bits of ``run_mcmc(p, 25)``.

Unlike emcee a proposal the model cannot be evaluated at (NaN: ECC >= 1 under an allowing prior)
is rejected and counted (``n_flagged``), not raised; the halves are the first and the second
nwalkers / 2 walkers (emcee shuffles them each step).
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib as L

LD = np.longdouble
U32 = np.uint32
U64 = np.uint64


# -- Philox4x32-10 and the draws (the twin of csrc/ensemble.hpp) ---------------------------------------
def philox4x32_10(ctr, key):
    """ctr (n, 4) and key (2,) or (n, 2), uint32 -> (n, 4) uint32."""
    c = [np.array(ctr[:, i], dtype=U64) for i in range(4)]
    key = np.asarray(key, dtype=U64)
    k = [key[..., 0].copy(), key[..., 1].copy()]
    m32 = U64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c[0], U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + U64(0x9E3779B9)) & m32, (k[1] + U64(0xBB67AE85)) & m32]
    return np.stack(c, axis=1).astype(U32)


def draws(seed, walkers, step, half, nother):
    """(u_z, partner index, u_acc) of the walkers' moves at a step and half."""
    w = np.asarray(walkers, dtype=U64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step)
    ctr = np.stack([w, np.full_like(w, step & 0xFFFFFFFF), np.full_like(w, step >> 32), np.full_like(w, half)], axis=1)
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=U64)).astype(U64)
    m = ((r[:, 1] << U64(32)) | r[:, 0]) >> U64(11)
    u_z = (m.astype(np.float64) + 0.5) * 2.0 ** -53
    idx = ((r[:, 2] * U64(nother)) >> U64(32)).astype(np.int64)
    u_acc = (r[:, 3].astype(np.float64) + 0.5) * 2.0 ** -32
    return u_z, idx, u_acc


def stretch(a, u):
    t = (a - 1.0) * u + 1.0
    return t * t / a


# -- double-double in numpy (dd.hpp's operations, the same roundings) ----------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _two_prod(a, b):
    """p = fl(a b) and the exact a b - p (Dekker's split: what fma(a, b, -p) gives)."""
    p = a * b

    def split(x):
        t = 134217729.0 * x
        h = t - (t - x)
        return h, x - h
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ah, al, bh, bl):
    sh, sl = _two_sum(ah, bh)
    th, tl = _two_sum(al, bl)
    sh, sl = _quick_two_sum(sh, sl + th)
    return _quick_two_sum(sh, sl + tl)


def dd_mul_d(ah, al, b):
    ph, pl = _two_prod(ah, b)
    return _quick_two_sum(ph, pl + al * b)


def propose(xk_hi, xk_lo, xj_hi, xj_lo, z):
    """y = x_j + z (x_k - x_j) in double-double (ens_propose)."""
    th, tl = dd_add(xk_hi, xk_lo, -xj_hi, -xj_lo)
    mh, ml = dd_mul_d(th, tl, z)
    return dd_add(xj_hi, xj_lo, mh, ml)


def split_pairs(pos):
    """(…, 2) float64 (hi, lo) pairs of a float64 or longdouble array."""
    v = np.asarray(pos)
    if v.dtype != LD:
        v = v.astype(np.float64)
    out = np.empty(v.shape + (2,))
    out[..., 0] = v
    out[..., 1] = (v - out[..., 0].astype(LD)) if v.dtype == LD else 0.0
    return out


# -- what the device needs to know of a target --------------------------------------------------------
def prior_table(target):
    """(nparams, ENS_PRIOR_W): the device's prior table of the target's parameters (csrc/ensemble.hpp);
    NotImplementedError naming the parameter whose prior it cannot hold."""
    import math
    from .priors import UniformUnboundedRV
    tab = np.zeros((target.nparams, L.ENS_PRIOR_W))
    for j, p in enumerate(target.params):
        rv = p.prior._rv
        dist = getattr(rv, "dist", rv)
        args, kw = getattr(rv, "args", ()), getattr(rv, "kwds", {})
        loc = float(args[0]) if len(args) > 0 else float(kw.get("loc", 0.0))
        scale = float(args[1]) if len(args) > 1 else float(kw.get("scale", 1.0))
        name = getattr(dist, "name", None)
        if isinstance(dist, UniformUnboundedRV):
            tab[j, 0] = L.ENS_PRIOR_FLAT
        elif name == "uniform" and len(args) + len(kw) <= 2 and scale > 0:
            tab[j, :4] = L.ENS_PRIOR_UNIFORM, loc, scale, math.log(scale)
        elif name == "norm" and len(args) + len(kw) <= 2 and scale > 0:
            tab[j, :5] = L.ENS_PRIOR_NORMAL, loc, scale, math.log(scale), math.log(math.sqrt(2.0 * math.pi))
        elif name == "bounded_gaussian" and scale > 0:
            tab[j] = L.ENS_PRIOR_BNORMAL, loc, scale, math.log(scale), float(dist.a), float(dist.b)
        else:
            raise NotImplementedError(f"the prior of {p.name} ({p.prior!r}) has no form in the device's prior table: "
                                      f"use resident=False")
    for j in range(len(target.params), target.nparams):  # (PhotonTiming's PHASE)
        tab[j, 0] = L.ENS_PRIOR_PHASE
    return tab


def class_map(target):
    """(imap, fmap) of pint_ens_init: the EFAC / EQUAD entries of the target's noise classes."""
    ptrs, cols, vals = [], [], []
    sets = [getattr(target, "_cls", None), getattr(target, "_dmcls", None)]
    counts = []
    for cls in sets:
        n = 0 if cls is None else len(cls[2])
        counts.append(n)
        for which in (2, 3):  # EFACs, then EQUADs
            ptr = [len(cols)]
            for c in range(n):
                for col, fixed in cls[which][c]:
                    cols.append(col)
                    vals.append(fixed if col < 0 else 0.0)
                ptr.append(len(cols))
            ptrs.append(ptr)
    imap = np.array(counts + [len(cols)] + [x for p in ptrs for x in p] + cols, dtype=np.int32)
    return imap, np.array(vals + [0.0], dtype=np.float64)


def resident_kind(target):
    """PINT_ENS_* of a target the device sampler takes, else None."""
    from .bayesian import BayesianTiming
    from .event_optimize import PhotonTiming
    if isinstance(target, BayesianTiming) and target.likelihood_method == "wls":
        return L.ENS_WLS
    if isinstance(target, PhotonTiming) and target.template is not None:
        return L.ENS_PHOTON
    return None


class EnsembleSampler:
    """EnsembleSampler(target, nwalkers, seed=0, a=2.0, resident=None).

    target : a PointBatch (BayesianTiming, PhotonTiming).
    nwalkers : even, at least 4; fewer than 2 nparams walkers cannot span the space (emcee refuses
        that by default; here it is a warning).
    seed : the Philox key.   a : the stretch scale (> 1).
    resident : True the device path (NotImplementedError if the target or one of its priors has no
        resident form), False the host-stepped mode, None the device path where the target has one.
    chunk : steps between two drains of the device's chain (None: chosen from the sizes).
    """

    def __init__(self, target, nwalkers, seed=0, a=2.0, resident=None, chunk=None):
        nwalkers = int(nwalkers)
        if nwalkers < 4 or nwalkers % 2:
            raise ValueError(f"nwalkers must be even and at least 4, got {nwalkers}")
        if not float(a) > 1.0:
            raise ValueError("the stretch scale a must be > 1")
        self.target, self.nwalkers, self.ndim = target, nwalkers, int(target.nparams)
        if nwalkers < 2 * self.ndim:
            warnings.warn(f"{nwalkers} walkers for {self.ndim} parameters: fewer than twice the dimension, the "
                          f"ensemble cannot span the space well", RuntimeWarning, stacklevel=2)
        self.seed, self.a = int(seed), float(a)
        kind = resident_kind(target)
        if resident is None:
            resident = kind is not None
            if resident:
                try:
                    prior_table(target)
                except NotImplementedError:
                    resident = False
        elif resident:
            if kind is None:
                raise NotImplementedError("this target has no device-resident likelihood (the correlated-noise likelihood "
                                          "and a PhotonTiming without a template are host-stepped): use resident=False")
            prior_table(target)
        self.resident, self._kind = bool(resident), kind
        self.chunk = 0 if chunk is None else int(chunk)
        self._live = False
        self.reset()

    # -- state ---------------------------------------------------------------------------
    def reset(self):
        """Forget the chain, the counters and the walkers; the next run_mcmc needs a start, and its
        first step is step 0 again."""
        self._close_device()
        self.iteration = 0
        self._hi, self._lo, self._lnp = [], [], []
        self._x = self._xlnp = None
        self._nacc = np.zeros(self.nwalkers, dtype=np.int64)
        self._nflag = np.zeros(self.nwalkers, dtype=np.int64)
        self._cnt0 = (0, 0)

    def _close_device(self):
        if getattr(self, "_live", False):
            s = self.target._dev
            if s is not None and s.ctx:
                s.L.pint_ens_close(s.ctx)
            self._live = False

    def close(self):
        self._close_device()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- running -------------------------------------------------------------------------
    def _install(self):
        """The half-ensemble's batch on the target's Session (a call that finds it resident only forms
        tables): pint_set_points through the Session, which keeps its own view of the batch in step."""
        t = self.target
        s = t._device()
        cols = [j for j, _ in t._timing]
        base = np.tile(np.asarray(t._base_values, dtype=LD)[cols], (self.nwalkers // 2, 1))
        s.set_points(t.lay, t._table0, [p for _, p in t._timing], base)
        return s

    def _start_device(self, pairs):
        t = self.target
        self._close_device()
        s = self._install()
        cols = np.array([j for j, _ in t._timing], dtype=np.int32)
        base = np.ascontiguousarray(split_pairs(np.asarray(t._base_values, dtype=LD)))
        prior = np.ascontiguousarray(prior_table(t))
        imap, fmap = class_map(t)
        pos = np.ascontiguousarray(pairs)
        phase_col = self.ndim - 1 if self._kind == L.ENS_PHOTON else -1
        s._check(s.L.pint_ens_init(s.ctx, self._kind, self.nwalkers, self.ndim, len(cols), L.ptr(cols, C.c_int32),
                                   L.ptr(base), L.ptr(prior), phase_col, imap.size, L.ptr(imap, C.c_int32), L.ptr(fmap),
                                   C.c_uint64(self.seed & (2 ** 64 - 1)), self.a, self.chunk, self.iteration, L.ptr(pos)))
        self._live = True
        self._cnt0 = (self._nacc.copy(), self._nflag.copy())

    def _run_device(self, nsteps):
        s = self._install()
        s._check(s.L.pint_ens_run(s.ctx, int(nsteps)))
        W, d = self.nwalkers, self.ndim
        hi, lo, lp = np.empty((nsteps, W, d)), np.empty((nsteps, W, d)), np.empty((nsteps, W))
        cnt, st = np.empty(2 * W, dtype=np.int32), np.empty(2 * W * d + W)
        s._check(s.L.pint_ens_read(s.ctx, L.ptr(hi), L.ptr(lo), L.ptr(lp), L.ptr(cnt, C.c_int32), L.ptr(st)))
        self._nacc = self._cnt0[0] + cnt[:W]
        self._nflag = self._cnt0[1] + cnt[W:]
        self._x = np.stack([st[:W * d].reshape(W, d), st[W * d:2 * W * d].reshape(W, d)], axis=-1)
        self._xlnp = st[2 * W * d:].copy()
        return hi, lo, lp

    def _lnpost_pairs(self, pairs):
        with np.errstate(invalid="ignore"):
            return np.asarray(self.target.lnposterior_batch(np.ascontiguousarray(pairs)), dtype=np.float64)

    def _run_host(self, nsteps):
        W, d, h = self.nwalkers, self.ndim, self.nwalkers // 2
        x, lnp = self._x, self._xlnp
        hi, lo, lp = np.empty((nsteps, W, d)), np.empty((nsteps, W, d)), np.empty((nsteps, W))
        for r in range(nsteps):
            for half in (0, 1):
                me = np.arange(half * h, half * h + h)
                u_z, idx, u_acc = draws(self.seed, me, self.iteration + r, half, h)
                z = stretch(self.a, u_z)
                xj = x[(1 - half) * h + idx]
                yh, yl = propose(x[me, :, 0], x[me, :, 1], xj[:, :, 0], xj[:, :, 1], z[:, None])
                y = np.stack([yh, yl], axis=-1)
                lnq = self._lnpost_pairs(y)
                nan = np.isnan(lnq)
                self._nflag[me[nan]] += 1
                with np.errstate(invalid="ignore"):
                    acc = ~nan & (np.log(u_acc) < (d - 1) * np.log(z) + lnq - lnp[me])
                x[me[acc]] = y[acc]
                lnp[me[acc]] = lnq[acc]
                self._nacc[me[acc]] += 1
            hi[r], lo[r], lp[r] = x[:, :, 0], x[:, :, 1], lnp
        return hi, lo, lp

    def run_mcmc(self, pos, nsteps, thin_by=1):
        """nsteps (x thin_by) more steps, every thin_by-th stored.  pos: (nwalkers, nparams) float64 or
        longdouble, or None to go on from the last state.  Returns the last state (positions as
        longdouble, log-posteriors)."""
        nsteps, thin_by = int(nsteps), int(thin_by)
        if nsteps < 0 or thin_by < 1:
            raise ValueError("nsteps must be >= 0 and thin_by >= 1")
        if pos is None:
            if self._x is None:
                raise ValueError("no walkers yet: the first run_mcmc needs initial positions")
            if self.resident and not self._live:
                self._start_device(self._x)
        else:
            p = np.asarray(pos)
            if p.shape != (self.nwalkers, self.ndim):
                raise ValueError(f"pos must be ({self.nwalkers}, {self.ndim}), got {p.shape}")
            pairs = split_pairs(p)
            if self.resident:
                try:
                    self._start_device(pairs)
                except L.PintError as e:
                    if e.code == L.PINT_E_INVALID and "finite log-posterior" in str(e):
                        raise ValueError(str(e)) from None
                    raise
                self._x, self._xlnp = pairs, None
            else:
                lnp = self._lnpost_pairs(pairs)
                if not np.all(np.isfinite(lnp)):
                    raise ValueError(f"the initial position of walker {int(np.argmin(np.isfinite(lnp)))} has no finite "
                                     f"log-posterior")
                self._x, self._xlnp = pairs.copy(), lnp
        total = nsteps * thin_by
        if total:
            hi, lo, lp = (self._run_device if self.resident else self._run_host)(total)
            self.iteration += total
            keep = slice(thin_by - 1, None, thin_by)
            self._hi.append(hi[keep])
            self._lo.append(lo[keep])
            self._lnp.append(lp[keep])
        return self.get_last_sample()

    # -- results -------------------------------------------------------------------------
    def _cat(self, parts, tail):
        return np.concatenate(parts, axis=0) if parts else np.empty((0, self.nwalkers) + tail)

    @staticmethod
    def _cut(a, flat, discard, thin):
        a = a[int(discard)::int(thin)]
        return a.reshape((-1,) + a.shape[2:]) if flat else a

    def get_chain(self, flat=False, discard=0, thin=1, longdouble=False):
        """(steps, nwalkers, nparams): float64 (hi + lo rounded) or longdouble (the pair)."""
        hi, lo = self._cat(self._hi, (self.ndim,)), self._cat(self._lo, (self.ndim,))
        c = hi.astype(LD) + lo.astype(LD) if longdouble else hi + lo
        return self._cut(c, flat, discard, thin)

    def get_chain_pairs(self, discard=0, thin=1):
        """(steps, nwalkers, nparams, 2): the walkers' (hi, lo) pairs, nothing rounded."""
        c = np.stack([self._cat(self._hi, (self.ndim,)), self._cat(self._lo, (self.ndim,))], axis=-1)
        return c[int(discard)::int(thin)]

    def get_log_prob(self, flat=False, discard=0, thin=1):
        return self._cut(self._cat(self._lnp, ()), flat, discard, thin)

    @property
    def acceptance_fraction(self):
        return self._nacc / max(self.iteration, 1)

    @property
    def n_flagged(self):
        """Per walker, the proposals the model could not be evaluated at (rejected)."""
        return self._nflag.copy()

    def chains_to_dict(self, names):
        c = self.get_chain()
        if len(names) != self.ndim:
            raise ValueError(f"{len(names)} names for {self.ndim} parameters")
        return {n: c[:, :, i] for i, n in enumerate(names)}

    def get_initial_pos(self, fitkeys, fitvals, fiterrs, errfact, rng=None, **kw):
        """get_initial_pos (below) for this sampler's walkers; rng defaults to the sampler's seed."""
        return get_initial_pos(fitkeys, fitvals, fiterrs, errfact, self.nwalkers, self.seed if rng is None else rng, **kw)

    def get_last_sample(self):
        if self._x is None:
            return None
        if self.resident and self._xlnp is None:  # (started, no step yet)
            s = self.target._device()
            W, d = self.nwalkers, self.ndim
            st = np.empty(2 * W * d + W)
            s._check(s.L.pint_ens_read(s.ctx, None, None, None, None, L.ptr(st)))
            self._xlnp = st[2 * W * d:].copy()
        return self._x[:, :, 0].astype(LD) + self._x[:, :, 1].astype(LD), self._xlnp.copy()


def get_initial_pos(fitkeys, fitvals, fiterrs, errfact, nwalkers, rng=None, **kw):
    """A ball of nwalkers starting positions around fitvals, fiterrs x errfact wide (the reference's
    EmceeSampler.get_initial_pos), with its special cases: GLPH_1 uniform in [-0.5, 0.5]; GLEP_1 uniform
    in [minMJD + 100, maxMJD - 100]; SINI and PHASE uniform in [0, 1]; M2 uniform in [0.1, 0.6]; E, ECC,
    PX, A1 = |value + error x normal| (the full error), E and ECC reflected below 1; pos[0] = fitvals.
    rng: a numpy Generator or a seed."""
    fitkeys = list(fitkeys)
    if len(fitkeys) != len(fitvals):
        raise ValueError(f"Number of keys does ({len(fitkeys)}) not match number of values ({len(fitvals)})!")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    ld = np.asarray(fitvals).dtype == LD
    vals = np.asarray(fitvals, dtype=LD if ld else np.float64)
    errs = np.asarray(fiterrs, dtype=np.float64)
    n = len(vals)
    pos = vals[None, :] + (errs * float(errfact))[None, :] * rng.standard_normal((nwalkers, n))
    uniform = {"GLPH_1": (-0.5, 0.5), "SINI": (0.0, 1.0), "M2": (0.1, 0.6), "PHASE": (0.0, 1.0)}
    for param in ("GLPH_1", "GLEP_1", "SINI", "M2", "E", "ECC", "PX", "A1", "PHASE"):
        if param not in fitkeys:
            continue
        i = fitkeys.index(param)
        if param == "GLEP_1":
            if kw.get("minMJD") is None or kw.get("maxMJD") is None:
                raise ValueError("minMJD or maxMJD is None for glep_1 param")
            sv = rng.uniform(kw["minMJD"] + 100, kw["maxMJD"] - 100, nwalkers)
        elif param in uniform:
            sv = rng.uniform(*uniform[param], nwalkers)
        else:
            sv = np.abs(vals[i] + errs[i] * rng.standard_normal(nwalkers))
            if param in ("E", "ECC"):
                sv = np.where(sv > 1.0, 1.0 - (sv - 1.0), sv)
        pos[:, i] = sv
    pos[0] = vals
    return pos


def integrated_time(chain, c=5):
    """The integrated autocorrelation time of every parameter of a chain (steps, nwalkers, nparams) --
    or (steps, nwalkers), (steps,) --, as emcee estimates it: the FFT autocorrelation function of each
    walker, averaged over the walkers, tau(M) = 2 sum_{t <= M} rho(t) - 1 at Sokal's window, the smallest
    M with M >= c tau(M)."""
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None, None]
    elif x.ndim == 2:
        x = x[:, :, None]
    n, nw, nd = x.shape
    nfft = 1 << (2 * n - 1).bit_length()
    tau = np.empty(nd)
    for k in range(nd):
        f = np.zeros(n)
        for w in range(nw):
            y = x[:, w, k] - np.mean(x[:, w, k])
            ft = np.fft.rfft(y, nfft)
            acf = np.fft.irfft(ft * np.conj(ft), nfft)[:n]
            f += acf / acf[0] if acf[0] > 0 else 0.0
        f /= nw
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(n) < c * taus
        win = int(np.argmin(m)) if not m.all() else n - 1
        tau[k] = taus[win]
    return tau
