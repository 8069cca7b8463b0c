"""The residual pass swept over row counts, options and launch paths, against an exact reference.

Every fit, every Residuals, every grid point and every Woodbury chi2 goes through the residual
pass: five implementations of one arithmetic (k_resid1<256> + k_resid2<256>, their one-wave
forms, k_resid12, the first half fused into the evaluation's blocks, the second half deferred
into k_gram_v), three options (track mode, subtract_mean, use_weighted_mean) and the Woodbury
trig tiles of k_resid2.  The cases (resid_cases.py) are prefixes of one fake TOA set of 16 257
rows at the geocentre with two sigma classes a factor 10 apart and +-1, +-2 turns of
delta_pulse_number on a tenth of the rows; every instance's table has F0 and F1 offset so that
the phase residual wanders by 2 to 4 turns to either side over the case's own rows (`nearest`
really wraps, the pulse-number residuals are O(1) turns).  Every case runs the eight option sets
of resid_cases.OPTIONS (track mode x (weighted mean, unweighted mean, no mean), and the model
with a free PHOFF in both track modes), one pulsar layout each, in one session.

The reference is the operation restated from the device's own evaluation outputs
(Session.read_eval: phase hi, lo and the Taylor frequency, n + 1 rows), the layout's pulse
numbers, delta_pulse_number and scaled sigma:

  full_i  exactly, in rational arithmetic (fractions.Fraction of the doubles; longdouble cannot
          hold a 1e11-turn phase to better than 1e-8): (phase_i - phase_TZR + dpn_i) - pn_i, or
          in `nearest` mode x - floor(x + 1/2), x relative to row 0 only when the mean is
          subtracted (oracle/pint_oracle.py::residuals).  Asserted: no row's x lies within 1e-9
          of a half-integer.
  mean, subtraction, division by the Taylor frequency: longdouble.
  WLS chi2: longdouble, from the device's own time residuals.
  GLS chi2: ld_util.ld_woodbury_chi2 on the device's own time residuals, the Fourier columns
          ld_util.host_fourier, a column of ones (prior 1e40) unless PHOFF is free.

Bars, eps = 2^-52 (derived, not tuned; the run prints every case's worst value per bar):
  (a) phase residual before the mean (the option sets without one): |d| <= 2 eps max(|full_i|,
      2^-54): the double-double chain, far below eps, and one rounding.
  (b) mean-subtracted phase residual: |d| <= 32 eps sum w |full| / sum w + 2 eps |p_i|: no path
      adds more than ~21 roundings in series (4 rows per thread, an 8-level tree, one strided
      partial, a second 8-level tree), then two products and one division.
  (c) time residual: the phase bar / F + eps |rt_i|.
  (d) WLS chi2: 1e-13 relative (positive terms, depth below 40 roundings).
  (e) GLS chi2 after eval(False): 1e-9 relative with r^T N^-1 r / chi2 <= 10 asserted
      (test_shape_sweep's bar (d)); resid_cases.tile_scale chooses the offsets so that it holds.
  (f) the fit flow: debug_gram()'s r^T N^-1 r entry (the residuals k_gram_v staged itself, from
      its own mean) against longdouble on the residuals read back, 1e-12 relative.

Session.resid_path() is asserted against the case's mask after the evaluation and after the
reads, and the phases of each model and table, read back with every option set, must not depend
on the options; test_every_path_was_run asserts the union of the masks.

Measured on an MI355X (130 cases x 8 option sets, all within their bars; (a)-(c) as the worst row's
error / bar, (d)-(f) relative):
                                              bar     measured, worst case
  (a) phase residual before the mean, err / bar 1       2.5e-01  (defer_n16256)
  (b) mean-subtracted phase residual, err / bar 1       1.7e-01  (small_tiles_n129_x5)
  (c) time residual, err / bar                  1       3.2e-01  (defer_n16257_not)
  (d) WLS chi2                                  1e-13   3.0e-16  (r256_n1025)
  (e) GLS chi2 after eval(False)                1e-9    3.1e-16  (small_tiles_n64_x3)
  (f) k_gram_v's r^T N^-1 r                     1e-12   1.7e-15  (defer_n16257_not)
The one rounding of (a) shows as 0.25 = eps / 2 over 2 eps; the mean's roundings stay below a fifth
of bar (b).  The hand-made mutations this sweep was checked against (each fails at least 22
cases): `+ dpn` dropped in the evaluation's fused first half, in k_resid1 and in k_resid12; lw for
lw * lw in k_resid12 and in the fused first half; d0 taken with subtract_mean off in k_resid1;
EF_ROWS for EF_ROWS + 1 in the `own` test of the evaluation's last lanes; c8 / s8 swapped in the
tile staging (nred >= 8 at n >= 257, nred >= 9 at n = 65); the fourth term of the four-wave tile
sum dropped (n >= 257).

Per case (path: Session.resid_path() after the reads):
  case                         path                       worst per bar
  small_n1_x1_r12              r12                        a 1.6e-01 b       - c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x1_r1r2             r1<64>+r2<64>              a 1.6e-01 b       - c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x3_r12              r12                        a 1.6e-01 b 1.0e-05 c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x3_r1r2             r1<64>+r2<64>              a 1.6e-01 b 1.0e-05 c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x4_r12              r12                        a 1.8e-01 b 1.0e-05 c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x4_r1r2             r1<64>+r2<64>              a 1.8e-01 b 1.0e-05 c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x5_r12              r12                        a 1.8e-01 b 1.0e-05 c 1.9e-01 d 2.0e-16 e       - f       -
  small_n1_x5_r1r2             r1<64>+r2<64>              a 1.8e-01 b 1.0e-05 c 1.9e-01 d 2.0e-16 e       - f       -
  small_n2_x1_r12              r12                        a 2.3e-01 b 3.0e-02 c 1.5e-01 d 1.3e-16 e       - f       -
  small_n2_x1_r1r2             r1<64>+r2<64>              a 2.3e-01 b 3.0e-02 c 1.5e-01 d 1.3e-16 e       - f       -
  small_n2_x3_r12              r12                        a 2.3e-01 b 3.0e-02 c 1.5e-01 d 1.3e-16 e       - f       -
  small_n2_x3_r1r2             r1<64>+r2<64>              a 2.3e-01 b 3.0e-02 c 1.5e-01 d 1.3e-16 e       - f       -
  small_n2_x4_r12              r12                        a 2.3e-01 b 3.0e-02 c 1.5e-01 d 1.5e-16 e       - f       -
  small_n2_x4_r1r2             r1<64>+r2<64>              a 2.3e-01 b 3.0e-02 c 1.5e-01 d 1.5e-16 e       - f       -
  small_n2_x5_r12              r12                        a 2.3e-01 b 3.0e-02 c 1.5e-01 d 2.8e-16 e       - f       -
  small_n2_x5_r1r2             r1<64>+r2<64>              a 2.3e-01 b 3.0e-02 c 1.5e-01 d 2.8e-16 e       - f       -
  small_n63_x1_r12             r12                        a 2.4e-01 b 2.5e-02 c 2.8e-01 d 1.0e-16 e       - f       -
  small_n63_x1_r1r2            r1<64>+r2<64>              a 2.4e-01 b 2.5e-02 c 2.8e-01 d 1.0e-16 e       - f       -
  small_n63_x3_r12             r12                        a 2.4e-01 b 3.2e-02 c 2.9e-01 d 2.7e-16 e       - f       -
  small_n63_x3_r1r2            r1<64>+r2<64>              a 2.4e-01 b 3.2e-02 c 2.9e-01 d 2.7e-16 e       - f       -
  small_n63_x4_r12             r12                        a 2.4e-01 b 3.2e-02 c 2.9e-01 d 2.7e-16 e       - f       -
  small_n63_x4_r1r2            r1<64>+r2<64>              a 2.4e-01 b 3.2e-02 c 2.9e-01 d 2.7e-16 e       - f       -
  small_n63_x5_r12             r12                        a 2.4e-01 b 3.9e-02 c 2.9e-01 d 2.7e-16 e       - f       -
  small_n63_x5_r1r2            r1<64>+r2<64>              a 2.4e-01 b 3.9e-02 c 2.9e-01 d 2.7e-16 e       - f       -
  small_n64_x1_r12             r12                        a 2.4e-01 b 2.4e-02 c 2.9e-01 d 1.4e-16 e       - f       -
  small_n64_x1_r1r2            r1<64>+r2<64>              a 2.4e-01 b 2.4e-02 c 2.9e-01 d 1.4e-16 e       - f       -
  small_n64_x3_r12             r12                        a 2.4e-01 b 2.9e-02 c 2.9e-01 d 1.8e-16 e       - f       -
  small_n64_x3_r1r2            r1<64>+r2<64>              a 2.4e-01 b 2.9e-02 c 2.9e-01 d 1.8e-16 e       - f       -
  small_n64_x4_r12             r12                        a 2.4e-01 b 3.1e-02 c 2.9e-01 d 1.8e-16 e       - f       -
  small_n64_x4_r1r2            r1<64>+r2<64>              a 2.4e-01 b 3.1e-02 c 2.9e-01 d 1.8e-16 e       - f       -
  small_n64_x5_r12             r12                        a 2.4e-01 b 3.1e-02 c 3.0e-01 d 1.8e-16 e       - f       -
  small_n64_x5_r1r2            r1<64>+r2<64>              a 2.4e-01 b 3.1e-02 c 3.0e-01 d 1.8e-16 e       - f       -
  small_n65_x1_r12             r12                        a 2.3e-01 b 3.0e-02 c 2.8e-01 d 9.5e-17 e       - f       -
  small_n65_x1_r1r2            r1<64>+r2<64>              a 2.3e-01 b 3.0e-02 c 2.8e-01 d 9.5e-17 e       - f       -
  small_n65_x3_r12             r12                        a 2.5e-01 b 3.4e-02 c 2.8e-01 d 1.7e-16 e       - f       -
  small_n65_x3_r1r2            r1<64>+r2<64>              a 2.5e-01 b 3.4e-02 c 2.8e-01 d 1.7e-16 e       - f       -
  small_n65_x4_r12             r12                        a 2.5e-01 b 3.9e-02 c 2.8e-01 d 1.7e-16 e       - f       -
  small_n65_x4_r1r2            r1<64>+r2<64>              a 2.5e-01 b 3.9e-02 c 2.8e-01 d 1.7e-16 e       - f       -
  small_n65_x5_r12             r12                        a 2.5e-01 b 3.9e-02 c 2.8e-01 d 2.1e-16 e       - f       -
  small_n65_x5_r1r2            r1<64>+r2<64>              a 2.5e-01 b 3.9e-02 c 2.8e-01 d 2.1e-16 e       - f       -
  small_n128_x1_r12            r12                        a 2.3e-01 b 3.0e-02 c 2.6e-01 d 1.4e-16 e       - f       -
  small_n128_x1_r1r2           r1<64>+r2<64>              a 2.3e-01 b 3.0e-02 c 2.6e-01 d 1.4e-16 e       - f       -
  small_n128_x3_r12            r12                        a 2.4e-01 b 3.3e-02 c 2.9e-01 d 1.4e-16 e       - f       -
  small_n128_x3_r1r2           r1<64>+r2<64>              a 2.4e-01 b 3.3e-02 c 2.9e-01 d 1.4e-16 e       - f       -
  small_n128_x4_r12            r12                        a 2.4e-01 b 3.7e-02 c 3.0e-01 d 1.4e-16 e       - f       -
  small_n128_x4_r1r2           r1<64>+r2<64>              a 2.4e-01 b 3.7e-02 c 3.0e-01 d 1.4e-16 e       - f       -
  small_n128_x5_r12            r12                        a 2.4e-01 b 5.6e-02 c 3.0e-01 d 1.4e-16 e       - f       -
  small_n128_x5_r1r2           r1<64>+r2<64>              a 2.4e-01 b 5.6e-02 c 3.0e-01 d 1.4e-16 e       - f       -
  small_n129_x1_r12            r12                        a 2.3e-01 b 4.4e-02 c 2.8e-01 d 1.1e-16 e       - f       -
  small_n129_x1_r1r2           r1<64>+r2<64>              a 2.3e-01 b 4.4e-02 c 2.8e-01 d 1.1e-16 e       - f       -
  small_n129_x3_r12            r12                        a 2.3e-01 b 6.8e-02 c 2.8e-01 d 1.2e-16 e       - f       -
  small_n129_x3_r1r2           r1<64>+r2<64>              a 2.3e-01 b 6.8e-02 c 2.8e-01 d 1.2e-16 e       - f       -
  small_n129_x4_r12            r12                        a 2.4e-01 b 6.8e-02 c 2.8e-01 d 1.2e-16 e       - f       -
  small_n129_x4_r1r2           r1<64>+r2<64>              a 2.4e-01 b 6.8e-02 c 2.8e-01 d 1.2e-16 e       - f       -
  small_n129_x5_r12            r12                        a 2.4e-01 b 6.8e-02 c 2.9e-01 d 1.2e-16 e       - f       -
  small_n129_x5_r1r2           r1<64>+r2<64>              a 2.4e-01 b 6.8e-02 c 2.9e-01 d 1.2e-16 e       - f       -
  small_n255_x1_r12            r12                        a 2.4e-01 b 5.6e-02 c 3.0e-01 d 1.3e-16 e       - f       -
  small_n255_x1_r1r2           r1<64>+r2<64>              a 2.4e-01 b 5.6e-02 c 3.0e-01 d 1.3e-16 e       - f       -
  small_n255_x3_r12            r12                        a 2.4e-01 b 6.3e-02 c 3.0e-01 d 2.0e-16 e       - f       -
  small_n255_x3_r1r2           r1<64>+r2<64>              a 2.4e-01 b 6.3e-02 c 3.0e-01 d 2.0e-16 e       - f       -
  small_n255_x4_r12            r12                        a 2.5e-01 b 6.3e-02 c 3.0e-01 d 2.0e-16 e       - f       -
  small_n255_x4_r1r2           r1<64>+r2<64>              a 2.5e-01 b 6.3e-02 c 3.0e-01 d 2.0e-16 e       - f       -
  small_n255_x5_r12            r12                        a 2.5e-01 b 6.3e-02 c 3.0e-01 d 2.0e-16 e       - f       -
  small_n255_x5_r1r2           r1<64>+r2<64>              a 2.5e-01 b 6.3e-02 c 3.0e-01 d 2.0e-16 e       - f       -
  small_n256_x1_r12            r12                        a 2.4e-01 b 4.5e-02 c 3.0e-01 d 1.6e-16 e       - f       -
  small_n256_x1_r1r2           r1<64>+r2<64>              a 2.4e-01 b 4.5e-02 c 3.0e-01 d 1.6e-16 e       - f       -
  small_n256_x3_r12            r12                        a 2.4e-01 b 4.7e-02 c 3.1e-01 d 1.6e-16 e       - f       -
  small_n256_x3_r1r2           r1<64>+r2<64>              a 2.4e-01 b 4.7e-02 c 3.1e-01 d 1.6e-16 e       - f       -
  small_n256_x4_r12            r12                        a 2.5e-01 b 4.7e-02 c 3.1e-01 d 1.6e-16 e       - f       -
  small_n256_x4_r1r2           r1<64>+r2<64>              a 2.5e-01 b 4.7e-02 c 3.1e-01 d 1.6e-16 e       - f       -
  small_n256_x5_r12            r12                        a 2.5e-01 b 4.9e-02 c 3.1e-01 d 1.7e-16 e       - f       -
  small_n256_x5_r1r2           r1<64>+r2<64>              a 2.5e-01 b 4.9e-02 c 3.1e-01 d 1.7e-16 e       - f       -
  small_tiles_n64_x3           r1<64>+r2<64>+tiles        a 2.4e-01 b 1.1e-01 c 2.7e-01 d 2.2e-16 e 3.1e-16 f       -
  small_tiles_n129_x5          r1<64>+r2<64>+tiles        a 2.4e-01 b 1.7e-01 c 3.1e-01 d 1.7e-16 e 2.1e-16 f       -
  small_tiles_n255_x1          r1<64>+r2<64>+tiles        a 2.4e-01 b 9.7e-02 c 2.7e-01 d 2.2e-16 e 2.3e-16 f       -
  small_tiles_n256_x4          r1<64>+r2<64>+tiles        a 2.5e-01 b 1.4e-01 c 3.2e-01 d 1.5e-16 e 2.1e-16 f       -
  r256_n257                    r1<256>+r2<256>            a 2.5e-01 b 6.3e-02 c 2.8e-01 d 2.1e-16 e       - f       -
  r256_n1023                   r1<256>+r2<256>            a 2.5e-01 b 4.8e-02 c 2.9e-01 d 1.7e-16 e       - f       -
  r256_n1024                   r1<256>+r2<256>            a 2.5e-01 b 5.9e-02 c 3.0e-01 d 1.4e-16 e       - f       -
  r256_n1025                   r1<256>+r2<256>            a 2.5e-01 b 5.5e-02 c 3.1e-01 d 3.0e-16 e       - f       -
  r256_n2049                   r1<256>+r2<256>            a 2.5e-01 b 5.1e-02 c 3.1e-01 d 1.5e-16 e       - f       -
  efused_n257                  efused+r2<256>             a 2.5e-01 b 5.2e-02 c 2.8e-01 d 2.1e-16 e       - f       -
  efused_n253                  efused+r2<256>             a 2.4e-01 b 5.0e-02 c 2.8e-01 d 1.3e-16 e       - f       -
  efused_n254                  efused+r2<256>             a 2.4e-01 b 4.5e-02 c 3.1e-01 d 2.2e-16 e       - f       -
  efused_n255                  efused+r2<256>             a 2.4e-01 b 5.6e-02 c 3.0e-01 d 1.5e-16 e       - f       -
  efused_n508                  efused+r2<256>             a 2.4e-01 b 4.3e-02 c 2.8e-01 d 2.3e-16 e       - f       -
  efused_n509                  efused+r2<256>             a 2.5e-01 b 5.0e-02 c 3.1e-01 d 1.3e-16 e       - f       -
  efused_mixed                 efused+r2<256>             a 2.5e-01 b 5.0e-02 c 3.1e-01 d 2.2e-16 e       - f       -
  r256_mixed                   r1<256>+r2<256>            a 2.5e-01 b 5.0e-02 c 3.1e-01 d 2.2e-16 e       - f       -
  tiles_n65_nred1_efused       efused+r2<256>+tiles       a 2.3e-01 b 6.5e-02 c 2.3e-01 d 1.4e-16 e 1.9e-16 f       -
  tiles_n65_nred1_unfused      r1<64>+r2<64>+tiles        a 2.3e-01 b 6.5e-02 c 2.3e-01 d 2.4e-16 e 2.6e-16 f       -
  tiles_n65_nred7_efused       efused+r2<256>+tiles       a 2.3e-01 b 6.5e-02 c 2.3e-01 d 1.4e-16 e 1.8e-16 f       -
  tiles_n65_nred7_unfused      r1<64>+r2<64>+tiles        a 2.3e-01 b 6.5e-02 c 2.3e-01 d 2.4e-16 e 2.6e-16 f       -
  tiles_n65_nred8_efused       efused+r2<256>+tiles       a 2.3e-01 b 6.5e-02 c 2.3e-01 d 1.4e-16 e 1.8e-16 f       -
  tiles_n65_nred8_unfused      r1<64>+r2<64>+tiles        a 2.3e-01 b 6.5e-02 c 2.3e-01 d 2.4e-16 e 2.6e-16 f       -
  tiles_n65_nred9_efused       efused+r2<256>+tiles       a 2.3e-01 b 6.5e-02 c 2.3e-01 d 1.4e-16 e 1.8e-16 f       -
  tiles_n65_nred9_unfused      r1<64>+r2<64>+tiles        a 2.3e-01 b 6.5e-02 c 2.3e-01 d 2.4e-16 e 2.4e-16 f       -
  tiles_n65_nred31_efused      efused+r2<256>+tiles       a 2.3e-01 b 6.5e-02 c 2.3e-01 d 1.4e-16 e 1.5e-16 f       -
  tiles_n65_nred31_unfused     r1<64>+r2<64>+tiles        a 2.3e-01 b 6.5e-02 c 2.3e-01 d 2.4e-16 e 2.1e-16 f       -
  tiles_n65_nred63_efused      efused+r2<256>+tiles       a 2.3e-01 b 6.5e-02 c 2.3e-01 d 1.4e-16 e 1.9e-16 f       -
  tiles_n65_nred63_unfused     r1<64>+r2<64>+tiles        a 2.3e-01 b 6.5e-02 c 2.3e-01 d 2.4e-16 e 2.0e-16 f       -
  tiles_n257_nred1_efused      efused+r2<256>+tiles       a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.2e-16 f       -
  tiles_n257_nred1_unfused     r1<256>+r2<256>+tiles      a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.2e-16 f       -
  tiles_n257_nred7_efused      efused+r2<256>+tiles       a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.8e-16 f       -
  tiles_n257_nred7_unfused     r1<256>+r2<256>+tiles      a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.7e-16 f       -
  tiles_n257_nred8_efused      efused+r2<256>+tiles       a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.2e-16 f       -
  tiles_n257_nred8_unfused     r1<256>+r2<256>+tiles      a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.2e-16 f       -
  tiles_n257_nred9_efused      efused+r2<256>+tiles       a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.0e-16 f       -
  tiles_n257_nred9_unfused     r1<256>+r2<256>+tiles      a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.0e-16 f       -
  tiles_n257_nred31_efused     efused+r2<256>+tiles       a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.2e-16 f       -
  tiles_n257_nred31_unfused    r1<256>+r2<256>+tiles      a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.1e-16 f       -
  tiles_n257_nred63_efused     efused+r2<256>+tiles       a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.8e-16 f       -
  tiles_n257_nred63_unfused    r1<256>+r2<256>+tiles      a 2.5e-01 b 1.3e-01 c 2.8e-01 d 2.0e-16 e 2.7e-16 f       -
  tiles_n1025_nred1_efused     efused+r2<256>+tiles       a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.4e-16 f       -
  tiles_n1025_nred1_unfused    r1<256>+r2<256>+tiles      a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.4e-16 f       -
  tiles_n1025_nred7_efused     efused+r2<256>+tiles       a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.3e-16 f       -
  tiles_n1025_nred7_unfused    r1<256>+r2<256>+tiles      a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.3e-16 f       -
  tiles_n1025_nred8_efused     efused+r2<256>+tiles       a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.2e-16 f       -
  tiles_n1025_nred8_unfused    r1<256>+r2<256>+tiles      a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.2e-16 f       -
  tiles_n1025_nred9_efused     efused+r2<256>+tiles       a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 1.9e-16 f       -
  tiles_n1025_nred9_unfused    r1<256>+r2<256>+tiles      a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 1.9e-16 f       -
  tiles_n1025_nred31_efused    efused+r2<256>+tiles       a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.5e-16 f       -
  tiles_n1025_nred31_unfused   r1<256>+r2<256>+tiles      a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.5e-16 f       -
  tiles_n1025_nred63_efused    efused+r2<256>+tiles       a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.5e-16 f       -
  tiles_n1025_nred63_unfused   r1<256>+r2<256>+tiles      a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 2.5e-16 f       -
  tiles_n1025_nred64_kwdot     efused+r2<256>             a 2.5e-01 b 1.6e-01 c 2.8e-01 d 2.3e-16 e 1.9e-16 f       -
  defer_n1025                  efused+r2<256>+deferred    a 2.5e-01 b 4.5e-02 c 3.1e-01 d 2.8e-16 e       - f 4.5e-16
  defer_n1025_unfused          r1<256>+r2<256>+deferred   a 2.5e-01 b 4.5e-02 c 3.1e-01 d 1.8e-16 e       - f 4.5e-16
  defer_n16256                 efused+r2<256>+deferred    a 2.5e-01 b 7.0e-02 c 3.1e-01 d 6.7e-17 e       - f 1.4e-15
  defer_n16257_not             efused+r2<256>             a 2.5e-01 b 7.8e-02 c 3.2e-01 d 1.4e-16 e       - f 1.7e-15
"""
from fractions import Fraction

import numpy as np
import pytest

import resid_cases as RC
from ld_util import LD, host_fourier, ld_woodbury_chi2

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CASES = RC.cases()
RAN = {}       # case name -> (mask after the evaluation, mask after the reads)
WORST = {}     # bar -> (worst value, case)
_PREFIX = {}
_FOUR = {}


@pytest.fixture(scope="module")
def toas_all():
    from pint_amd.simulation import make_fake_toas_batch
    base = RC.model_of(RC.RCase("base", (RC.N_ALL,), 0), False)
    t = make_fake_toas_batch([RC.toa_spec(base)])[0]
    assert t.ntoas == RC.N_ALL and t.get_pulse_numbers() is not None
    t.arrays["delta_pulse_number"] = RC.delta_pulse_numbers()
    return t


def prefix(toas, n):
    if n not in _PREFIX:
        _PREFIX[n] = toas if n == toas.ntoas else toas[np.arange(n)]
    return _PREFIX[n]


def to_ld(fr):
    """A Fraction to longdouble, correctly to ~1e-32 relative (two doubles)."""
    hi = float(fr)
    return LD(hi) + LD(float(fr - Fraction(hi)))


def exact_rel(hi, lo, dpn):
    """phase_i - phase_TZR + dpn_i, exactly."""
    tz = Fraction(float(hi[-1])) + Fraction(float(lo[-1]))
    return [Fraction(float(h)) + Fraction(float(l)) - tz + Fraction(float(d)) for h, l, d in zip(hi[:-1], lo[:-1], dpn)]


def exact_full(rel, pn, o):
    """(full_i in longdouble, the smallest distance of a pre-rounding phase to a half-integer)."""
    if o.track == "use_pulse_numbers":
        return np.array([to_ld(r - Fraction(float(p))) for r, p in zip(rel, pn)], dtype=LD), None
    half = Fraction(1, 2)
    x = [r - rel[0] for r in rel] if o.mean else rel
    fl = [(v + half).__floor__() for v in x]
    margin = min(min(v + half - f, f + 1 - (v + half)) for v, f in zip(x, fl))
    return np.array([to_ld(v - f) for v, f in zip(x, fl)], dtype=LD), float(margin)


def fourier(lay, toas, n, nred):
    if (n, nred) not in _FOUR:
        _FOUR[(n, nred)] = host_fourier(lay, toas)
    return _FOUR[(n, nred)]


def over(err, bar):
    """max err / bar; a zero bar (one row with its own mean subtracted: exactly 0) allows no error."""
    err, bar = np.atleast_1d(err), np.atleast_1d(bar)
    q = np.where(err == 0, LD(0), err / np.where(bar > 0, bar, LD(1)))
    return float(np.max(np.where((bar > 0) | (err == 0), q, np.inf)))


def note(bar, v, name):
    if bar not in WORST or v > WORST[bar][0]:
        WORST[bar] = (v, name)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_resid(c, toas_all, monkeypatch):
    from pint_amd.engine import Session, build_layout
    monkeypatch.setenv("PINT_RESID12", "1" if c.resid12 else "0")
    monkeypatch.setenv("PINT_NSPLIT", "1")
    assert RC.predict_mask(c) == (c.mask, c.mask_read)
    tiles, fit = c.flow == "tiles", c.flow == "fit"
    worst = dict(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, f=0.0)
    masks = set()
    rels = {}
    s = Session()
    try:
        s.set_small(c.small)
        s.set_efuse(c.efuse)
        for o in RC.OPTIONS:
            scale = RC.tile_scale(o) if tiles else 1.0
            lays, insts = [], []
            for n in c.ns:
                t = prefix(toas_all, n)
                lay = s.add(build_layout(RC.model_of(c, o.phoff, n), t, track_mode=o.track, subtract_mean=o.sub,
                                         use_weighted_mean=o.wm))
                assert (lay.spec.track_pn, lay.spec.subtract_mean, lay.spec.weighted_mean) == \
                    (int(o.track == "use_pulse_numbers"), int(o.mean), int(o.wm))
                assert lay.nred == c.nred
                lays.append(lay)
                insts += [(lay, RC.table_of(lay, n, k, scale)) for k in range(c.ninst)]
            s.set_instances(insts)
            gls = g_rr = None
            if fit:
                s.eval(Session.FIT)
                assert s.n_vgram() == len(insts)
                m0 = s.resid_path()
                s.fit_step(1)
                g_rr = [G[lay.K, lay.K] for (G, _), (lay, _) in zip(s.debug_gram(), insts)]
            else:
                s.eval(True)
                if tiles:
                    s.fit_step(1)
                    assert s.wfuse() == (c.nred <= 63)
                    s.eval(False)
                m0 = s.resid_path()
            assert m0 == c.mask, (o.name, RC.mask_names(m0), RC.mask_names(c.mask))
            tr, pr, c2 = s.read_resids()
            m1 = s.resid_path()
            assert m1 == c.mask | c.mask_read, (o.name, RC.mask_names(m1))
            if tiles:
                gls = s.chi2_gls()
            hi, lo, ft, _ = s.read_eval()
            masks.add((m0, m1))
            for j, (lay, _) in enumerate(insts):
                n, t = lay.n, lay.toas
                key = (o.phoff, scale, j)
                if key not in rels:  # the phases do not depend on the residual options
                    rels[key] = (hi[j].copy(), lo[j].copy(), exact_rel(hi[j], lo[j], t.arrays["delta_pulse_number"]))
                assert np.array_equal(rels[key][0], hi[j]) and np.array_equal(rels[key][1], lo[j]), o.name
                full, margin = exact_full(rels[key][2], t.get_pulse_numbers(), o)
                assert margin is None or margin > 1e-9, (o.name, j, margin)
                sig = np.asarray(lay.sigma_us * 1e-6, dtype=LD)
                F = np.asarray(ft[j][:n], dtype=LD)
                w = 1 / (sig * sig) if o.wm else np.ones(n, dtype=LD)
                if o.mean:
                    p = full - np.sum(w * full) / np.sum(w)
                    bar = 32 * EPS * np.sum(w * np.abs(full)) / np.sum(w) + 2 * EPS * np.abs(p)
                else:
                    p = full
                    bar = 2 * EPS * np.maximum(np.abs(full), LD(2.0) ** -54)
                rt = p / F
                ep = over(np.abs(np.asarray(pr[j], dtype=LD) - p), bar)
                et = over(np.abs(np.asarray(tr[j], dtype=LD) - rt), bar / np.abs(F) + EPS * np.abs(rt))
                worst["b" if o.mean else "a"] = max(worst["b" if o.mean else "a"], ep)
                worst["c"] = max(worst["c"], et)
                z = np.asarray(tr[j], dtype=LD) / sig
                rNr = np.sum(z * z)
                worst["d"] = max(worst["d"], over(abs(LD(c2[j]) - rNr), rNr))
                if g_rr is not None:
                    worst["f"] = max(worst["f"], over(abs(LD(g_rr[j]) - rNr), rNr))
                if gls is not None:
                    U, ph = fourier(lay, t, n, c.nred), np.asarray(lay.red_phi, dtype=LD)
                    if not o.phoff:
                        U = np.concatenate([U, np.ones((n, 1), dtype=LD)], axis=1)
                        ph = np.concatenate([ph, [LD(1e40)]])
                    ref, rNr2 = ld_woodbury_chi2(tr[j], sig, U, ph)
                    assert rNr2 / ref <= 10, (o.name, j, float(rNr2 / ref))
                    worst["e"] = max(worst["e"], float(abs(LD(gls[j]) / ref - 1)))
    finally:
        s.close()
    print(f"{c.name:<28} {RC.mask_names(c.mask | c.mask_read):<26} " +
          " ".join(f"{k} {v:.1e}" if v else f"{k}       -" for k, v in worst.items()))
    for k, v in worst.items():
        note(k, v, c.name)
    RAN[c.name] = (c.mask, c.mask | c.mask_read)
    assert masks == {(c.mask, c.mask | c.mask_read)}
    assert worst["a"] <= 1 and worst["b"] <= 1 and worst["c"] <= 1
    assert worst["d"] <= 1e-13
    assert worst["e"] <= 1e-9
    assert worst["f"] <= 1e-12


def test_every_path_was_run():
    """The union of the masks that ran (each asserted per case) holds all eight bits, every case
    ran, and each pairing of a first half with a second half that the dispatcher can choose."""
    assert sorted(RAN) == sorted(c.name for c in CASES)
    union = 0
    for _, m in RAN.values():
        union |= m
    print("worst per bar: " + ", ".join(f"({k}) {v:.1e} [{n}]" for k, (v, n) in sorted(WORST.items())))
    print("paths run: " + RC.mask_names(union))
    assert union == 255, RC.mask_names(union)
    seen = {m for m, _ in RAN.values()}
    for m in (RC.R12, RC.R1_64 | RC.R2_64, RC.R1_64 | RC.R2_64 | RC.TILES, RC.R1_256 | RC.R2_256,
              RC.R1_256 | RC.R2_256 | RC.TILES, RC.EFUSED | RC.R2_256, RC.EFUSED | RC.R2_256 | RC.TILES,
              RC.EFUSED | RC.DEFERRED, RC.R1_256 | RC.DEFERRED):
        assert m in seen, RC.mask_names(m)
