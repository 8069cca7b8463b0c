"""Gram and solve kernel instantiations swept over widths, against a longdouble reference.

pint_fit_step picks its kernels from the padded width of the normal equations; the fixtures
reach a few widths only.  Every case here is a synthetic model of an exact width
(shape_cases.py) on one of four fake TOA sets (n = 300, 530, 1100, and 1100 in four-frequency
epochs for ECORR; made once), with the residuals replaced by a seeded N(0, sigma_i) vector.
n = 530 is just over GS_MAXN = 512 and no multiple of 64; n = 1100 leaves a ragged last chunk.
Per case:

(a) Session.last_plan() equals the plan shape_cases.predict_plan derives from the widths, so a
    case cannot stop exercising its instantiation unnoticed; test_every_target_was_run asserts
    the union of the plans that ran.
(b) debug_gram() against [M | F | r]^T N^-1 [M | F | r] in longdouble: the timing columns M
    from a full-layout read_designmatrix() of a separate session without the generated-Fourier
    path, the Fourier columns F = sin / cos(2 pi f_k t) evaluated in longdouble on the host
    (the stored ones are checked against them to 5e-13: a column error d moves a normalised
    Gram entry by at most sqrt(2) d).  Bar |dA_ij| <= 1e-12 sqrt(D_i D_j) and 1e-12 relative
    on the column sums of squares; the FP64 accumulation bound n eps
    sqrt(D_i D_j) is 1.2e-13 at n = 1100.
(c) step, errors and covariance against a longdouble solve and inverse of the device's own
    normalised system, built element for element as the solve kernels form it.  Bar e_dev <=
    max(1e-9 sigma, 3 e_ref), e_ref the error of a float64 LAPACK Cholesky solve of the same
    system against the longdouble one; every case is built so that e_ref <= 1e-7 sigma
    (asserted), while an indexing error moves the step by O(1) sigma.
(d) chi2_gls() against the longdouble Woodbury form on the same residuals, 1e-9 relative, with
    r^T N^-1 r / chi2 <= 10 asserted so that cancellation does not eat the bar.

Unreachable by the layout rules (shape_cases.vgram_keys_reachable; pint_set_instances):
k_gram_v<1, 6>, <1, 7> and <2, 7> (keys 6, 7, 17): the Fourier tiles number ceil(nred / 8) <= 4
beside R row tiles.  The w8 rule's `nbs_sig <= 9` clause of k_solve_dmx cannot decide: a fused
Sigma of 10 blocks needs nred >= 72, whose dense block has more than 8 column blocks already.
SD_MAXBLK = 76 is not reached as a block count that runs: its only layout within n rows, 8
dense x 5 DMX blocks, needs 164,608 bytes of LDS and falls back to the general solve on the
LDS rule; 75 blocks (10 x 2) is the largest that runs (dmx_blk75_*), 77 (11 x 1) falls back
on SD_MAXBLK.  Full-layout GLS systems of K >= 197 are beyond k_solve's LDS: the Gram's T = 7,
8, 9 run as WLS steps.  The ECORR variants k_gram<T, ch, true> run for T = 2 and 3 on the TOA
set of four-frequency epochs (multi_freqs_in_epoch), against the same Gram with the ECORR
block eliminated in longdouble.

Measured on an MI355X (98 cases, all within their bars; the run prints every case's line):
                                  bar                 measured, worst case
  stored Fourier columns          5e-13               1.9e-15
  Gram, |dA_ij| / sqrt(D_i D_j)   1e-12               1.8e-14 (8.1e-14 with ECORR eliminated)
  column sums of squares          1e-12               5.3e-15
  step (sigma)                    max(1e-9, 3 e_ref)  2.8e-12   (e_ref up to 3.2e-12)
  errors (relative)               max(1e-9, 3 s_ref)  1.2e-12   (s_ref up to 1.9e-12)
  covariance (sigma_i sigma_j)    max(1e-9, 3 c_ref)  2.3e-12   (c_ref up to 3.8e-12)
  GLS chi2 (relative)             1e-9                2.5e-16
  post-fit chi2 (nred 63, 64)     1e-9                8.8e-17

Per case (plan: Gram / N-splits / solve / Sigma; Gram Tn = k_gram<n>, s = k_gram_s, vK = k_gram_v
key K, vb its binned body; dmxN = k_solve_dmx<N>; solve_K197 is refused before any launch):
  case                         K plan                              Gram     step    e_ref   errors      cov     chi2
  solve_K4                     4 T1/1/lanes4/side4             1.1e-14  3.1e-16  1.2e-16  1.6e-16  1.7e-16  1.6e-17
  solve_K5                     5 T1/1/lanes8/side4             1.1e-14  4.0e-16  8.6e-16  2.3e-16  2.8e-16  1.6e-17
  solve_K8                     8 T1/1/lanes8/side4             1.1e-14  3.3e-15  1.5e-15  4.9e-15  1.0e-14  1.6e-17
  solve_K9                     9 T1/1/blk1/side4               1.1e-14  2.7e-16  1.6e-15  1.5e-15  3.1e-15  1.6e-17
  grams_Kp16                  12 s/1/blk1/side4                1.5e-15  2.6e-15  1.1e-15  1.2e-15  2.8e-15  2.1e-16
  solve_K15                   15 T1/1/blk1/side4               1.1e-14  5.8e-15  4.8e-15  7.3e-15  1.4e-14  2.3e-17
  vg_R1_nred0                 15 v1vb/1/dmx8/-                 1.2e-15  2.0e-15  1.0e-15  6.9e-16  1.1e-15        -
  vg_R1_nred0_novb            15 v1/1/dmx8/-                   1.2e-15  2.0e-15  1.0e-15  6.9e-16  1.1e-15        -
  solve_K16                   16 T1/1/blk1/side4               1.1e-14  1.3e-14  1.7e-14  1.5e-14  2.9e-14  2.3e-17
  solve_K17                   17 T1/1/blk1/side4               1.1e-14  4.3e-15  5.4e-15  6.7e-15  1.3e-14  2.3e-17
  vg_R1_nred1                 17 v2vb/1/dmx8/fused             1.2e-15  5.1e-15  1.3e-15  3.0e-15  5.9e-15  1.6e-17
  vg_R1_nred1_novb            17 v2/1/dmx8/fused               1.2e-15  5.1e-15  1.3e-15  3.0e-15  5.9e-15  1.6e-17
  vg_R2_nred0                 26 v12vb/1/dmx8/-                1.2e-15  9.6e-16  1.0e-15  3.4e-16  6.3e-16        -
  vg_R2_nred0_novb            26 v12/1/dmx8/-                  1.2e-15  2.2e-15  5.0e-16  1.9e-15  3.7e-15        -
  solve_K31                   31 T1/1/blk1/side4               1.1e-14  1.4e-12  2.8e-12  2.9e-13  6.2e-13  2.3e-17
  grams_Kp32                  31 s/1/blk1/side4                1.5e-15  1.9e-13  3.4e-13  5.6e-14  1.1e-13  2.2e-16
  vg_R1_nred8                 31 v2vb/1/dmx8/fused             1.2e-15  1.6e-14  6.7e-15  9.6e-15  1.9e-14  4.2e-17
  vg_R1_nred8_novb            31 v2/1/dmx8/fused               1.2e-15  1.6e-14  6.7e-15  9.6e-15  1.9e-14  4.2e-17
  solve_K32                   32 T1/1/blk1/side4               1.1e-14  2.5e-12  3.2e-12  5.8e-13  1.2e-12  2.3e-17
  solve_K33                   33 T1/1/blk4/side4               1.1e-14  1.8e-12  1.8e-12  7.1e-13  1.4e-12  2.3e-17
  vg_R3_nred0                 39 v23vb/1/dmx8/-                1.2e-15  1.2e-15  1.3e-15  4.9e-16  1.2e-15        -
  vg_R3_nred0_novb            39 v23/1/dmx8/-                  1.2e-15  1.9e-15  7.1e-16  1.1e-15  2.1e-15        -
  vg_R2_nred8                 42 v13vb/1/dmx8/fused            1.2e-15  2.3e-14  2.9e-14  1.8e-14  3.5e-14  4.2e-17
  vg_R2_nred8_novb            42 v13/1/dmx8/fused              1.2e-15  3.5e-14  5.4e-15  3.6e-14  7.2e-14  4.2e-17
  vg_R2_wt21                  46 v13vb/1/dmx8/fused            1.2e-15  1.2e-13  1.8e-13  3.0e-13  5.9e-13  4.2e-17
  vg_R2_wt21_novb             46 v13/1/dmx8/fused              1.2e-15  1.2e-13  1.8e-13  3.0e-13  5.9e-13  4.2e-17
  vg_R1_nred16                47 v3vb/1/dmx8/fused             1.2e-15  1.6e-14  1.7e-14  9.5e-15  1.9e-14  1.1e-16
  vg_R1_nred16_novb           47 v3/1/dmx8/fused               1.2e-15  1.6e-14  1.7e-14  9.5e-15  1.9e-14  1.1e-16
  vg_R3_nred8                 55 v24vb/1/dmx8/fused            1.2e-15  1.6e-14  5.7e-15  2.3e-14  4.6e-14  4.2e-17
  vg_R3_nred8_novb            55 v24/1/dmx8/fused              1.2e-15  3.2e-14  1.6e-14  3.5e-14  7.1e-14  4.2e-17
  vg_R2_nred16                58 v14vb/1/dmx8/fused            1.2e-15  2.3e-14  2.8e-14  1.8e-14  3.6e-14  1.1e-16
  vg_R2_nred16_novb           58 v14/1/dmx8/fused              1.2e-15  3.5e-14  9.7e-15  3.6e-14  7.2e-14  1.1e-16
  vg_R2_nred16_ns3            58 v3vb/3/dmx8/fused             6.7e-16  7.7e-15  1.1e-14  1.2e-14  2.4e-14  1.0e-17
  vg_R2_nred16_ns5            58 v3vb/5/dmx8/fused             5.1e-16  3.5e-15  7.0e-15  1.4e-15  4.6e-15  1.1e-16
  vg_R3_wt37                  62 v24vb/1/dmx8/fused            1.2e-15  6.2e-13  2.5e-12  1.2e-12  2.3e-12  4.2e-17
  vg_R3_wt37_novb             62 v24/1/dmx8/fused              1.2e-15  6.2e-13  2.5e-12  1.2e-12  2.3e-12  4.2e-17
  vg_R1_nred24                63 v4vb/1/dmx8/fused             1.2e-15  1.6e-14  1.1e-14  9.5e-15  1.9e-14  1.1e-16
  vg_R3_wt40                  63 v24vb/1/dmx8/fused            1.2e-15  2.8e-12  2.7e-12  9.2e-13  1.8e-12  4.2e-17
  vg_R1_nred24_novb           63 v4/1/dmx8/fused               1.2e-15  1.6e-14  1.1e-14  9.5e-15  1.9e-14  1.1e-16
  vg_R3_wt40_novb             63 v24/1/dmx8/fused              1.2e-15  2.8e-12  2.7e-12  9.2e-13  1.8e-12  4.2e-17
  vg_R3_nred16                71 v25vb/1/dmx8/fused            1.2e-15  1.6e-14  5.1e-15  2.3e-14  4.6e-14  1.1e-16
  vg_R3_nred16_novb           71 v25/1/dmx8/fused              1.2e-15  3.2e-14  6.0e-15  3.5e-14  7.1e-14  1.1e-16
  vg_R2_nred24                74 v15vb/1/dmx8/fused            1.2e-15  2.3e-14  3.3e-14  1.8e-14  3.6e-14  1.1e-16
  vg_R2_nred24_novb           74 v15/1/dmx8/fused              1.2e-15  3.5e-14  3.4e-15  3.6e-14  7.2e-14  1.1e-16
  vg_R1_nred31                77 v5vb/1/dmx8/fused             1.2e-15  1.6e-14  1.7e-14  9.5e-15  1.9e-14  3.5e-17
  vg_R1_nred31_novb           77 v5/1/dmx8/fused               1.2e-15  1.6e-14  1.7e-14  9.5e-15  1.9e-14  3.5e-17
  gram_Kp80                   79 T1/1/blk4/side4               1.8e-14  1.3e-14  7.9e-15  2.1e-14  4.3e-14  2.0e-16
  solve_K80                   80 T2/1/blk4/side4               1.1e-14  1.2e-14  2.1e-14  6.3e-15  1.3e-14  2.9e-17
  solve_K81                   81 T2/1/blk16/side4              1.1e-14  6.0e-15  1.5e-15  5.3e-15  1.1e-14  2.9e-17
  vg_R2_nred30                86 v16vb/1/dmx8/fused            1.2e-15  2.3e-14  2.7e-14  1.8e-14  3.6e-14  8.9e-17
  vg_R2_nred30_novb           86 v16/1/dmx8/fused              1.2e-15  3.5e-14  4.0e-15  3.6e-14  7.2e-14  8.9e-17
  vg_R3_nred24                87 v26vb/1/dmx8/fused            1.2e-15  1.6e-14  6.0e-15  2.3e-14  4.6e-14  1.1e-16
  vg_R3_nred24_novb           87 v26/1/dmx8/fused              1.2e-15  3.2e-14  7.5e-15  3.5e-14  7.1e-14  1.1e-16
  vg_R2_nred31                88 v16vb/1/dmx8/fused            1.2e-15  2.3e-14  2.8e-14  1.8e-14  3.6e-14  3.5e-17
  vg_R2_nred31_novb           88 v16/1/dmx8/fused              1.2e-15  3.5e-14  3.2e-15  3.6e-14  7.3e-14  3.5e-17
  gram_Kp96                   90 T2/1/blk16/side4              1.8e-14  2.5e-15  1.1e-14  1.9e-14  3.8e-14  2.0e-16
  vg_off_nred32               90 T1/1/dmx8/fused               1.1e-14  4.0e-14  4.3e-15  3.0e-14  6.0e-14  2.2e-17
  sigma_nred39                90 T2/1/blk16/side4              1.8e-14  1.3e-14  3.6e-14  1.2e-14  2.5e-14  2.5e-16
  sigma_nred40                92 T2/1/blk16/side16             1.8e-14  1.3e-14  8.4e-15  1.5e-14  3.1e-14  7.8e-17
  solve_K95                   95 T2/1/blk16/side4              1.1e-14  3.1e-15  6.7e-15  5.1e-15  1.1e-14  2.9e-17
  solve_K96                   96 T2/1/blk16/side4              1.1e-14  1.0e-14  1.3e-14  7.1e-15  1.4e-14  2.9e-17
  vg_R3_nred31               101 v27/1/dmx8/fused              1.2e-15  3.2e-14  6.1e-15  3.5e-14  7.1e-14  3.5e-17
  vg_R3_nred31_novb          101 v27/1/dmx8/fused              1.2e-15  3.2e-14  6.1e-15  3.5e-14  7.1e-14  3.5e-17
  gram_Kp112                 111 T2/1/blk16/side4              1.8e-14  1.2e-14  6.9e-15  2.3e-14  4.6e-14  2.0e-16
  ecorr_Kp112                111 T2+ecorr/1/blk16/side4        8.1e-14  2.2e-15  2.7e-15  8.2e-16  1.2e-15  1.9e-16
  gram_Kp128                 120 T3/1/blk16/side4              1.8e-14  5.2e-15  4.5e-15  7.3e-15  1.4e-14  2.0e-16
  gram_Kp144                 143 T3/1/blk16/side4              1.8e-14  1.4e-14  1.5e-14  2.3e-14  4.5e-14  2.0e-16
  ecorr_Kp144                143 T3+ecorr/1/blk16/side4        8.1e-14  1.5e-15  2.3e-15  5.3e-15  1.0e-14  1.9e-16
  gram_Kp144_ns3             143 T3/3/blk16/side4              5.6e-15  4.4e-15  1.3e-14  3.0e-14  6.0e-14  2.0e-16
  gram_Kp144_ns5             143 T3/5/blk16/side4              2.4e-15  8.0e-15  9.5e-15  2.1e-14  4.1e-14  2.0e-16
  dmx_nbd8_d0                144 T3/1/dmx8/fused               1.8e-14  8.0e-15  2.0e-14  2.5e-15  5.6e-15  6.5e-17
  dmx_nbd8_d2                144 T3/1/dmx8/fused/schur/defer   1.8e-14  8.0e-15  2.0e-14  2.5e-15  5.6e-15  6.5e-17
  dmx_nbd8_d2_noschur        144 T3/1/dmx8/fused/defer         1.8e-14  8.0e-15  2.0e-14  2.5e-15  5.6e-15  6.5e-17
  dmx_nbd9_d0                145 T3/1/dmx16/fused              1.8e-14  1.6e-14  6.5e-15  8.7e-15  1.7e-14  6.5e-17
  dmx_nbd9_d2                145 T3/1/dmx16/fused/schur/defer  1.8e-14  1.6e-14  6.5e-15  8.7e-15  1.7e-14  6.5e-17
  dmx_nbd9_d2_noschur        145 T3/1/dmx16/fused/defer        1.8e-14  1.6e-14  6.5e-15  8.7e-15  1.7e-14  6.5e-17
  wfuse_nred63               154 T3/1/dmx16/fused              1.8e-14  1.3e-14  3.6e-15  2.3e-14  4.5e-14  7.7e-17
  wfuse_nred64               156 T3/1/dmx16/fused              1.8e-14  1.3e-14  4.1e-15  2.3e-14  4.5e-14  2.1e-16
  gram_Kp160                 159 T4/1/blk16/side16             1.8e-14  2.6e-15  6.4e-15  2.1e-14  4.2e-14  7.8e-17
  dmx_blk75_nbs9_d0          166 T4/1/dmx16/fused              1.8e-14  1.7e-14  4.9e-15  3.4e-14  6.9e-14  8.6e-17
  dmx_blk75_nbs9_d2          166 T4/1/dmx16/fused/schur/defer  1.8e-14  1.7e-14  4.9e-15  3.4e-14  6.9e-14  8.6e-17
  dmx_blk75_nbs9_d2_noschur  166 T4/1/dmx16/fused/defer        1.8e-14  1.7e-14  4.9e-15  3.4e-14  6.9e-14  8.6e-17
  dmx_nbs10_d0               174 T4/1/dmx16/fused              1.8e-14  1.7e-14  4.1e-15  3.5e-14  6.8e-14  8.3e-17
  dmx_nbs10_d2               174 T4/1/dmx16/fused/schur/defer  1.8e-14  1.7e-14  4.1e-15  3.5e-14  6.8e-14  8.3e-17
  dmx_nbs10_d2_noschur       174 T4/1/dmx16/fused/defer        1.8e-14  1.7e-14  4.1e-15  3.5e-14  6.8e-14  8.3e-17
  dmx_blk76_lds              178 T3/1/blk16/side16             1.8e-14  3.0e-14  1.7e-14  3.7e-14  7.3e-14  6.2e-17
  dmx_blk77                  186 T5/1/blk16/side16             1.8e-14  1.8e-15  3.4e-15  4.1e-15  7.5e-15  1.6e-16
  gram_Kp192                 191 T5/1/blk16/side16             1.8e-14  5.8e-15  1.2e-14  2.3e-15  4.2e-15  6.5e-17
  solve_K192                 192 T6/1/blk16/side16             1.8e-14  1.4e-14  1.8e-14  4.8e-14  9.6e-14  6.5e-17
  sigma_nred95               192 T6/1/blk16/side16             1.8e-14  1.7e-15  9.6e-16  1.4e-15  1.9e-15  1.2e-16
  solve_K193                 193 T6/1/column/side16            1.8e-14  3.0e-15  1.4e-14  2.6e-14  5.3e-14  6.5e-17
  sigma_nred96               194 T6/1/column/in-solve          1.8e-14  2.4e-15  1.8e-15  1.3e-15  1.7e-15  7.2e-17
  solve_K196                 196 T6/1/column/side4             1.8e-14  5.2e-15  5.1e-15  1.3e-14  2.6e-14  2.0e-16
  solve_K197_fit             197 T2/1/dmx8/fused               1.8e-14  3.5e-14  3.5e-14  1.1e-13  2.1e-13  2.0e-16
  gram_Kp224                 223 T7/1/blk16/-    (WLS)         1.8e-14  1.4e-15  1.7e-15  5.0e-16  1.1e-15        -
  gram_Kp240                 239 T8/1/blk16/-    (WLS)         1.8e-14  1.9e-15  2.0e-15  5.4e-16  1.6e-15        -
  gram_Kp256                 255 T9/1/blk16/-    (WLS)         1.8e-14  1.8e-15  2.5e-15  6.4e-16  1.7e-15        -
"""
import numpy as np
import pytest

import shape_cases as SC
from ld_util import LD, chol64, host_fourier, ld_gram, ld_woodbury_chi2, step_errors  # noqa: F401  (chol64: test_wideband_sweep.py imports it from here)

pytestmark = pytest.mark.gpu

CASES = sorted(SC.cases(), key=lambda c: c.K)  # narrow to wide
RAN = {}      # case name -> the plan that ran
_REF = {}     # reference design matrices by model


@pytest.fixture(scope="module")
def toa_sets():
    from pint_amd.simulation import make_fake_toas_batch
    base = SC.model_of(SC.Case("base", 8, SC.BASE_NDMX, 30))
    specs = [dict(model=base, start=SC.MJD0, end=SC.MJD1, ntoas=n, freq=[800, 1200, 1600, 2000], obs="geocenter",
                  error_us=0.5, add_noise=True, seed=100 + n) for n in (300, 530, 1100)]
    # epochs of four TOAs, flagged -f fake so that the cases' ECORR selects them
    specs.append(dict(specs[-1], multi_freqs_in_epoch=True, flags={"f": "fake"}, seed=99))
    toas = make_fake_toas_batch(specs)
    sets = {}
    for name, t in zip(("n300", "n530", "n1100", "e1100"), toas):
        rng = np.random.default_rng(t.ntoas)
        sets[name] = (t, rng.standard_normal(t.ntoas))
    return sets


def reference(c, toas):
    """(M | F in longdouble, sigma in s, phi) of the case's model: stored full-layout design
    matrix of a session without k_gram_v, its Fourier columns replaced by the host's."""
    key = (c.ntim, c.ndmx, c.nred, c.dmx_free, c.toas, c.ecorr)
    if key in _REF:
        return _REF[key]
    from pint_amd.engine import Session, build_layout, pack_table
    from pint_amd.noise import scaled_sigma_us
    model = SC.model_of(c)
    s = Session()
    try:
        s.set_vgram(False)
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.eval(want_M=True)
        M = np.array(s.read_designmatrix()[0], dtype=LD)
    finally:
        s.close()
    ncol = len(lay.columns)
    assert (ncol, lay.nred, lay.K) == (c.ncol, c.nred, c.K), (lay.columns, lay.nred)
    phi = None
    if c.nred:
        F = host_fourier(lay, toas)
        dF = float(np.max(np.abs(M[:, ncol:] - F)))
        print(f"{c.name}: stored Fourier columns vs host longdouble {dF:.2e}")
        assert dF <= 5e-13
        M[:, ncol:] = F
        phi = np.asarray(lay.red_phi, dtype=LD)
    sigma = np.asarray(scaled_sigma_us(model, toas), dtype=LD) * LD(1e-6)
    ep = None
    if c.ecorr:  # the epochs as the host forms them (noise.ecorr_epochs): TOA lists and ECORR^2
        assert lay.nep >= toas.ntoas // 8, lay.nep
        ep = [(lay.ep_idx[lay.ep_ptr[e]:lay.ep_ptr[e + 1]], LD(lay.ep_phi[e])) for e in range(lay.nep)]
    _REF[key] = (M, sigma, phi, ep)
    return _REF[key]


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_shape(c, toa_sets, monkeypatch):
    from pint_amd import _lib
    from pint_amd.engine import Session, build_layout, pack_table
    monkeypatch.setenv("PINT_NSPLIT", str(c.nsplit))
    toas, z = toa_sets[c.toas]
    M, sigma, phi, ep = reference(c, toas)
    r = np.asarray(z * sigma, dtype=np.float64)
    want = SC.predict_plan(c, toas.ntoas, toas.arrays["mjd_float"])
    s = Session()
    try:
        s.set_vgram(c.vgram)
        s.set_vbin(c.vbin)
        lay = s.add(build_layout(SC.model_of(c), toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.set_cov_defer(c.cov_defer)
        s.set_schur(c.schur)
        s.eval(want_M=Session.FIT if c.layout == "fit" else True)
        s.debug_set_resids([r])
        if c.refused:
            with pytest.raises(_lib.PintError) as e:
                s.fit_step(c.mode)
            assert e.value.code == _lib.PINT_E_INVALID and "normal matrix too large" in str(e.value)
            assert s.last_plan() == want  # nothing launched
            RAN[c.name] = dict(want, refused=True)
            return
        s.fit_step(c.mode)
        plan = s.last_plan()
        assert plan == want, {k: (plan[k], want[k]) for k in plan if plan[k] != want[k]}
        G, colsq = s.debug_gram()[0]
        dp, er, cov, _ = s.read_step()
        dp, er, cov = np.array(dp[0]), np.array(er[0]), np.array(cov[0])
        c2 = s.chi2_gls()[0] if (c.mode == 1 and c.nred) else None
        post = None
        if c.postfit:
            assert s.wfuse() == (c.nred <= 63)
            s.eval(False)
            post = (np.array(s.read_resids()[0][0]), s.chi2_gls()[0])
    finally:
        s.close()
    K, ncol = c.K, c.ncol
    # (b) Gram
    Gref, csref = ld_gram(M, r, sigma)
    if ep is not None:
        # the ECORR block eliminated (diagonal: disjoint epochs): - sum_e s_e s_e^T / D_e with
        # s_e = sum_{i in e} w_i [M | r]_i, D_e = 1 / ECORR^2 + sum_{i in e} w_i
        Xw = np.concatenate([M, np.asarray(r, dtype=LD)[:, None]], axis=1) / (sigma * sigma)[:, None]
        for idx, ph_e in ep:
            se = Xw[idx].sum(axis=0)
            Gref = Gref - np.outer(se, se) / (1 / ph_e + np.sum(1 / (sigma[idx] * sigma[idx])))
    D = np.sqrt(np.diag(Gref))
    eg = float(np.max(np.abs(G - Gref) / np.outer(D, D)))
    ec = float(np.max(np.abs(colsq / csref - 1)))
    # (c) step, errors, covariance: the device's own normalised system
    e_dev, e_ref, s_dev, s_ref, c_dev, c_ref = step_errors(G, colsq, K, ncol, c.mode, lay.red_phi, dp, er, cov)
    line = (f"{c.name}: K {K} n {toas.ntoas} gram {eg:.1e} colsq {ec:.1e} step {e_dev:.1e} (ref {e_ref:.1e}) "
            f"errs {s_dev:.1e} (ref {s_ref:.1e}) cov {c_dev:.1e} (ref {c_ref:.1e})")
    # (d) GLS chi2
    e2 = None
    if c2 is not None:
        E = np.zeros((toas.ntoas, len(ep or [])), dtype=LD)
        for e, (idx, _) in enumerate(ep or []):
            E[idx, e] = 1
        U = np.concatenate([M[:, ncol:], E, np.ones((toas.ntoas, 1), dtype=LD)], axis=1)
        ph = np.concatenate([phi, [p for _, p in (ep or [])], [LD(1e40)]])
        ref2, rNr = ld_woodbury_chi2(r, sigma, U, ph)
        assert rNr / ref2 <= 10
        e2 = float(abs(c2 / ref2 - 1))
        line += f" chi2 {e2:.1e}"
    ep = None
    if post is not None:
        refp, rNr = ld_woodbury_chi2(post[0], sigma, U, ph)
        assert rNr / refp <= 10, (rNr, refp)
        ep = float(abs(post[1] / refp - 1))
        line += f" post-fit chi2 {ep:.1e}"
    sol = plan["solve"] if plan["solve"] != "none" else f"dmx{plan['solve_dmx_waves']}"
    print(line + f" | gram {plan['gram_T'] or plan['gram_v'] or 'small'} nsplit {plan['nsplit']} solve {sol} "
          f"sigma {'fused' if plan['fuse_sigma'] else ('side%d' % plan['sigma_waves'] if plan['side_sigma'] else ('in-solve' if plan['do_sigma'] else '-'))}"
          f" schur {int(plan['schur'])} defer {int(plan['cov_deferred'])}")
    RAN[c.name] = plan
    assert eg <= 1e-12 and ec <= 1e-12
    assert e_ref <= 1e-7
    assert e_dev <= max(1e-9, 3 * e_ref)
    assert s_dev <= max(1e-9, 3 * s_ref)
    assert c_dev <= max(1e-9, 3 * c_ref)
    assert e2 is None or e2 <= 1e-9
    assert ep is None or ep <= 1e-9


def test_every_target_was_run():
    """The union of the plans that ran (each asserted equal to its prediction) covers every
    instantiation and switch the sweep was written for; no case may be skipped."""
    assert sorted(RAN) == sorted(c.name for c in CASES)
    plans = list(RAN.values())

    def seen(f):
        return {f(p) for p in plans}
    assert set(range(1, 10)) <= {T for p in plans for T in p["gram_T"]}
    assert any(p["gram_s"] for p in plans)
    assert len({p["gram_T"] for p in plans if p["gram_ecorr"]}) >= 2
    keys = {kv for p in plans for kv in p["gram_v"]}
    for k in SC.vgram_keys_reachable():
        assert (k, False) in keys, k
        assert k % 10 > 6 or (k, True) in keys, k
    assert {1, 3, 5} <= seen(lambda p: p["nsplit"])
    assert {"lanes4", "lanes8", "blk1", "blk4", "blk16", "column"} <= seen(lambda p: p["solve"])
    assert {8, 16} <= seen(lambda p: p["solve_dmx_waves"])
    assert {4, 16} <= seen(lambda p: p["sigma_waves"])
    for f in ("fuse_sigma", "side_sigma", "do_sigma", "schur", "cov_deferred", "greduce", "dmx_rows"):
        assert seen(lambda p: p[f]) == {False, True}, f
    assert any(p.get("refused") for p in plans)
    # fall-backs of the DMX-eliminated solve: compact layout through the general solve
    assert any(p["dmx_rows"] and p["solve"] == "blk16" for p in plans)
