"""What WaveX and DMWaveX cost the headline workload: the bench's 68-pulsar
x 10k-TOA PTA with --nharm WaveX and --nharm DMWaveX harmonics (n / T_span, every amplitude free
and non-zero) added to every pulsar against the same PTA without them, timed by the bench's own
step loop (bench.timed_steps: one GLSFitter.fit_toas(maxiter=1) of every pulsar per step), the two
batches alternating.  The WaveX batch has 4 x nharm more compact timing columns per pulsar in the
Gram and runs k_wavex after each of the step's evaluations.

How many harmonics fit beside the bench's shape is set by the fit kernels, not by k_wavex: a
bench pulsar has 100 DMX bins, up to 22 other timing columns and 60 red-noise columns, and the
DMX-eliminated solve keeps its dense block and the DMX coupling in LDS (SD_MAXBLK: at 100 bins a
dense block of at most 96 columns), so 3 + 3 harmonics (12 columns) is what the step comparison
can carry; the 10-45 harmonics of a wavex_setup par file come *instead of* PLRedNoise and DMX.
The kernel's own time is therefore measured apart, on evaluations alone, at --nharm-kernel
(15 + 15; the Gram's 255-column cap, GMAXKP, bounds it beside 100 DMX bins and 60 Fourier columns).

k_wavex's own time: the device time of the evaluation with the fit layout's design matrix
(pint_last_timing slot 4, which ends after k_wavex / k_glitch and before the residual pass) of the
WaveX batch less that of the plain batch, both with the fused residual pass off and the red-noise
columns stored in M (PINT_OPT_VGRAM 0: with this many timing columns the WaveX batch leaves the
generated-Fourier path anyway), so that the two run the same evaluation kernels on the same
columns and differ by k_wavex and by the evaluation's zero fill of the new columns (which k_wavex
then overwrites); median of --evals evaluations.  --kernel-only skips the
step loops.

Per row and evaluation with the design matrix k_wavex reads 8 doubles (tdb, delay, phase, radio
frequency, velocity) and the harmonics' table (block-uniform, cached) and writes 3 doubles and 2 K
doubles of columns per component: with 15 + 15 harmonics 88 B + 480 B = 0.57 kB per row; it
evaluates 15 + 15 sincospi (one per harmonic, for the delay and its two columns), about 30 x ~60 =
2 k FP64 operations.

    python3 scripts/diag/wavex_cost.py [--steps 100] [--reps 3] [--npsr 68] [--nharm 3] [--nharm-kernel 15]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T_SPAN = 3652.0


def wavex_lines(nharm):
    out = "WXEPOCH 54900\n"
    for stem, amp in (("WX", 1e-7), ("DMWX", 1e-5)):
        for k in range(1, nharm + 1):
            out += (f"{stem}FREQ_{k:04d} {k / T_SPAN!r}\n{stem}SIN_{k:04d} {amp / k!r} 1\n"
                    f"{stem}COS_{k:04d} {-0.7 * amp / k!r} 1\n")
    return out


def eval_ms(items, evals):
    """Median device ms of the evaluation with the fit layout's design matrix, fused residual pass off."""
    from pint_amd.engine import Session, pack_table
    s = Session(device=int(os.environ.get("LOCAL_RANK", "0")))
    s.set_efuse(False)
    s.set_vgram(False)
    lays = s.add_all(items)
    s.set_instances([(l, pack_table(l, m)) for l, (m, _) in zip(lays, items)])
    s.set_timing_mask(1 << 4)
    ms = []
    for _ in range(evals + 3):
        s.eval(want_M=Session.FIT)
        s.L.pint_sync(s.ctx)
        ms.append(float(s.timing()[4]))
    rows = sum(l.n + 1 for l in lays)
    s.close()
    return float(np.median(ms[3:])), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--npsr", type=int, default=68)
    ap.add_argument("--ntoas", type=int, default=10000)
    ap.add_argument("--nharm", type=int, default=3)
    ap.add_argument("--nharm-kernel", type=int, default=15)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    from bench import pipelines, timed_steps
    from pint_amd import get_model
    from pint_amd import simulation as sim
    idx = list(range(args.npsr))
    plain = [sim.pta_model(i) for i in idx]
    wavex = [get_model(sim.pta_par(i, sim.pta_kind(i)) + wavex_lines(args.nharm)) for i in idx]
    batches = {"plain": sim.make_pta(ntoas=args.ntoas, indices=idx, models=plain),
               "wavex": sim.make_pta(ntoas=args.ntoas, indices=idx, models=wavex)}
    ms = {k: [] for k in batches}
    for rep in range(0 if args.kernel_only else args.reps):
        for name, items in batches.items():
            ss, lays = pipelines(items, 2)
            dt = timed_steps(ss, args.steps, args.warmup, lambda: None, lambda v: v, graph="0", gram_pass=False,
                             pipes="auto")[0]
            for s in ss:
                s.close()
            ms[name].append(round(dt / args.steps * 1e3, 4))
            print(f"rep {rep} {name}: {ms[name][-1]} ms/step (K max {max(l.K for l in lays)})", file=sys.stderr, flush=True)
    wavex_k = [get_model(sim.pta_par(i, sim.pta_kind(i)) + wavex_lines(args.nharm_kernel)) for i in idx]
    batches["wavex"] = sim.make_pta(ntoas=args.ntoas, indices=idx, models=wavex_k)
    ev = {name: eval_ms(items, args.evals) for name, items in batches.items()}
    k_ms = ev["wavex"][0] - ev["plain"][0]
    rows = ev["wavex"][1]
    print(json.dumps({"npsr": args.npsr, "ntoas": args.ntoas, "steps": args.steps, "nharm": args.nharm,
                      "nharm_kernel": args.nharm_kernel,
                      "ms_per_step": ms, "median": {k: float(np.median(v)) for k, v in ms.items() if v},
                      "eval_with_M_device_ms": {k: v[0] for k, v in ev.items()}, "k_wavex_ms": k_ms,
                      "rows": rows, "k_wavex_ns_per_row": k_ms * 1e6 / rows}))


if __name__ == "__main__":
    main()
