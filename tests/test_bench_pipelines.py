"""bench.timed_steps' pipeline logic on the host (no GPU): a stand-in session records the
order of enqueues and retirements.  Checks that steps go round-robin over the pipelines, that
a pipeline's slot is retired before it is reused and every step is retired by the end, that
the trial times each candidate twice and keeps the fastest, and that a fixed count is used
as given."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class FakeSession:
    """The Session calls timed_steps makes; each 'step' costs `cost` seconds of host sleep
    divided by the number of pipelines the run uses (a stand-in for overlap)."""

    log = []

    def __init__(self, name, nslot):
        self.name, self.nslot = name, nslot
        self.next, self.pending = 0, []
        self.enqueued = self.retired = 0

    def save_tables(self):
        pass

    def set_lazy(self, on):
        assert on

    def set_timing_mask(self, m):
        pass

    def set_timing_every(self, k):
        pass

    def timing(self):
        return [0.0] * 8

    def fit_step_enqueue(self, restore=True, lam=1.0):
        assert len(self.pending) < self.nslot, "enqueue into a slot whose step was never checked"
        sl = self.next
        self.next = (sl + 1) % self.nslot
        self.pending.append(sl)
        self.enqueued += 1
        FakeSession.log.append(("enq", self.name))
        return sl, None, None, None

    def check_step(self, sl):
        assert self.pending and self.pending[0] == sl, "steps retired out of order"
        self.pending.pop(0)
        self.retired += 1


@pytest.fixture
def bench_mod(monkeypatch):
    import bench
    from pint_amd import _lib as L
    from pint_amd import engine
    monkeypatch.setattr(engine, "Session", FakeSession)  # (timed_steps' isinstance check)
    FakeSession.log = []
    return bench, L.NSLOT


def test_round_robin_and_every_step_retired(bench_mod):
    bench, nslot = bench_mod
    ss = [FakeSession("a", nslot), FakeSession("b", nslot)]
    dt, _, _, _, mode, p = bench.timed_steps(ss, 21, 3, lambda: None, lambda v: v, graph="0", gram_pass=False,
                                             pipes=2)
    assert (mode, p) == ("direct", 2)
    for s in ss:
        assert s.enqueued == s.retired and not s.pending
    timed = [n for k, n in FakeSession.log[-21:]]
    assert timed == [("a", "b")[i % 2] for i in range(21)]


def test_fixed_pipeline_count_uses_the_first_sessions(bench_mod):
    bench, nslot = bench_mod
    ss = [FakeSession("a", nslot), FakeSession("b", nslot)]
    _, _, _, _, _, p = bench.timed_steps(ss, 10, 2, lambda: None, lambda v: v, graph="0", gram_pass=False, pipes=1)
    assert p == 1
    assert [n for _, n in FakeSession.log[-10:]] == ["a"] * 10


def test_trial_keeps_the_fastest_candidate(bench_mod, monkeypatch):
    bench, nslot = bench_mod
    ss = [FakeSession("a", nslot), FakeSession("b", nslot)]
    clock = {"t": 0.0}

    def fake_clock():
        return clock["t"]

    orig = FakeSession.fit_step_enqueue

    def enq(self, restore=True, lam=1.0):
        # two pipelines: half the cost per step
        npipe = 2 if any(s.pending for s in ss if s is not self) else 1
        clock["t"] += 1.0 / npipe
        return orig(self, restore, lam)

    monkeypatch.setattr(FakeSession, "fit_step_enqueue", enq)
    monkeypatch.setattr(bench.time, "perf_counter", fake_clock)
    _, _, _, _, mode, p = bench.timed_steps(ss, 40, 2, lambda: None, lambda v: v, graph="0", gram_pass=False,
                                            pipes="auto")
    assert (mode, p) == ("direct", 2)


def test_on_timed_gets_the_last_timed_step(bench_mod):
    """The hook runs once, after the timed steps, with the session of the last timed step
    (step 20 of 21 over two pipelines: the first) and what that step handed out."""
    bench, nslot = bench_mod
    ss = [FakeSession("a", nslot), FakeSession("b", nslot)]
    seen = []
    bench.timed_steps(ss, 21, 3, lambda: None, lambda v: v, graph="0", gram_pass=False, pipes=2,
                      on_timed=lambda s, outs: seen.append((s.name, outs, s.enqueued, s.retired)))
    assert len(seen) == 1
    name, outs, enq, ret = seen[0]
    assert name == "a" and outs == (None, None, None)
    assert enq == ret  # every step retired before the outputs are read


def test_dump_outputs_files_and_seeded_sample(bench_mod, tmp_path, monkeypatch):
    import numpy as np
    from pint_amd.engine import SplitView
    bench, _ = bench_mod
    rng = np.random.default_rng(1)
    offk, offc = np.array([0, 3, 8]), np.array([0, 4, 20])
    dp, er, cov = rng.normal(size=8), rng.normal(size=8), rng.normal(size=20)
    cl, c2 = rng.normal(size=2), rng.normal(size=2)
    outs = ((SplitView(dp, offk), SplitView(er, offk), SplitView(cov, offc, [(2, 2), (4, 4)]), cl), None, c2)
    bench.dump_outputs(str(tmp_path / "d"), None, outs)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["chi2", "chi2_linearised", "covariances", "errors", "steps"]
    for k, ref in (("steps", dp), ("errors", er), ("covariances", cov), ("chi2_linearised", cl), ("chi2", c2)):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], ref)
    # over the budget: every array cut to the same seeded sample on every call, within it
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 20)
    for d in ("e", "f"):
        bench.dump_outputs(str(tmp_path / d), None, outs)
    e = {f: np.load(tmp_path / "e" / f) for f in os.listdir(tmp_path / "e")}
    f = {f: np.load(tmp_path / "f" / f) for f in os.listdir(tmp_path / "f")}
    assert sum(v.nbytes for v in e.values()) <= 8 * 20
    assert all(np.array_equal(e[k], f[k]) for k in e)
    assert np.array_equal(e["chi2.npy"], c2) and set(e["covariances.npy"]) <= set(cov)
