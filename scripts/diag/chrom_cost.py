"""What the chromatic pass costs, after wavex_cost.py's kernel measurement: the
bench's 68-pulsar x 10k-TOA PTA with ChromaticCM (CM free, TNCHROMIDX 2.6) and --nharm CMWaveX
harmonics (n / T_span, every amplitude free and non-zero) on every pulsar against the same PTA
without them.

The pass's own time: the device time of the evaluation with the fit layout's design matrix
(pint_last_timing slot 4, which ends after k_wavex / k_glitch and before the residual pass) of the
chromatic batch less that of the plain batch, both with the fused residual pass off and the
red-noise columns stored in M (PINT_OPT_VGRAM 0), so that the two run the same evaluation kernels
on the same columns and differ by k_wavex<true> and by the evaluation's zero fill of the new
columns (which the pass then overwrites); median of --evals evaluations.

Per row and evaluation with the design matrix the pass reads 8 doubles (tdb, delay, phase, radio
frequency, velocity) and the table (block-uniform, cached) and writes 3 doubles and 1 + 2 K doubles
of columns: with 1 + 15 that is 88 B + 248 B per row, beside 248 B of zeros from the evaluation;
it evaluates one pow and 15 sincospi.

    python3 scripts/diag/chrom_cost.py [--npsr 68] [--nharm 15] [--evals 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T_SPAN = 3652.0


def chrom_lines(nharm):
    out = "CM 0.05 1\nTNCHROMIDX 2.6\n"
    for k in range(1, nharm + 1):
        out += (f"CMWXFREQ_{k:04d} {k / T_SPAN!r}\nCMWXSIN_{k:04d} {0.02 / k!r} 1\n"
                f"CMWXCOS_{k:04d} {-0.014 / k!r} 1\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npsr", type=int, default=68)
    ap.add_argument("--ntoas", type=int, default=10000)
    ap.add_argument("--nharm", type=int, default=15)
    ap.add_argument("--evals", type=int, default=20)
    args = ap.parse_args()
    from wavex_cost import eval_ms
    from pint_amd import get_model
    from pint_amd import simulation as sim
    idx = list(range(args.npsr))
    plain = [sim.pta_model(i) for i in idx]
    chrom = [get_model(sim.pta_par(i, sim.pta_kind(i)) + chrom_lines(args.nharm)) for i in idx]
    batches = {"plain": sim.make_pta(ntoas=args.ntoas, indices=idx, models=plain),
               "chromatic": sim.make_pta(ntoas=args.ntoas, indices=idx, models=chrom)}
    ev = {name: eval_ms(items, args.evals) for name, items in batches.items()}
    k_ms = ev["chromatic"][0] - ev["plain"][0]
    rows = ev["chromatic"][1]
    print(json.dumps({"npsr": args.npsr, "ntoas": args.ntoas, "ncm": 1, "nharm": args.nharm,
                      "eval_with_M_device_ms": {k: v[0] for k, v in ev.items()}, "k_chrom_ms": k_ms,
                      "rows": rows, "k_chrom_ns_per_row": k_ms * 1e6 / rows}))


if __name__ == "__main__":
    main()
