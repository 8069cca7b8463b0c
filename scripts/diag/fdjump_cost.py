"""What the FDJump / FDJumpDM pass costs, after chrom_cost.py's measurement: the
bench's 68-pulsar x 10k-TOA PTA with three FDJUMPs (FD1JUMP and FD2JUMP on the 800 MHz band,
FD1JUMP on the 1200 MHz band) and one FDJUMPDM (the 1600 MHz band), all free and selected by
frequency range, on every pulsar against the same PTA without them.

The pass's own time: the device time of the evaluation with the fit layout's design matrix
(pint_last_timing slot 4, which ends after k_wavex / k_fdjump / k_glitch and before the residual
pass) of the FDJump batch less that of the plain batch, both with the fused residual pass off and
the red-noise columns stored in M (PINT_OPT_VGRAM 0), so that the two run the same evaluation
kernels on the same columns and differ by k_fdjump and by the evaluation's zero fill of the four
new columns (which the pass then overwrites); median of --evals evaluations.

Per row and evaluation with the design matrix the pass reads 8 doubles (tdb, delay, phase, radio
frequency, velocity), two mask words and the table (block-uniform, cached) and writes 3 doubles
and 4 doubles of columns: 88 B + 16 B + 32 B per row, beside 32 B of zeros from the evaluation; it
evaluates one log.

    python3 scripts/diag/fdjump_cost.py [--npsr 68] [--evals 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FDJ_LINES = ("FD1JUMP freq 700 900 2e-5 1\nFD2JUMP freq 700 900 4e-5 1\nFD1JUMP freq 1100 1300 1e-5 1\n"
             "FDJUMPDM freq 1500 1700 3e-4 1\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npsr", type=int, default=68)
    ap.add_argument("--ntoas", type=int, default=10000)
    ap.add_argument("--evals", type=int, default=20)
    args = ap.parse_args()
    from wavex_cost import eval_ms
    from pint_amd import get_model
    from pint_amd import simulation as sim
    idx = list(range(args.npsr))
    plain = [sim.pta_model(i) for i in idx]
    fdj = [get_model(sim.pta_par(i, sim.pta_kind(i)) + FDJ_LINES) for i in idx]
    batches = {"plain": sim.make_pta(ntoas=args.ntoas, indices=idx, models=plain),
               "fdjump": sim.make_pta(ntoas=args.ntoas, indices=idx, models=fdj)}
    selected = [len(t.select_mask(m[p].key, m[p].key_value)) for m, t in batches["fdjump"][:1]
                for p in m.fdjump_params() + m.fdjumpdm_params()]
    ev = {name: eval_ms(items, args.evals) for name, items in batches.items()}
    k_ms = ev["fdjump"][0] - ev["plain"][0]
    rows = ev["fdjump"][1]
    print(json.dumps({"npsr": args.npsr, "ntoas": args.ntoas, "nfdjump": 3, "nfdjumpdm": 1,
                      "selected_rows_first_pulsar": selected,
                      "eval_with_M_device_ms": {k: v[0] for k, v in ev.items()}, "k_fdjump_ms": k_ms,
                      "rows": rows, "k_fdjump_ns_per_row": k_ms * 1e6 / rows}))


if __name__ == "__main__":
    main()
