/*
 * pint_amd.h — C-ABI of libpint_hip.so, the MI355X (gfx950) implementation of PINT's
 * fit-and-residual hot path.
 *
 * The reference (Jackson-D-Taylor/PINT, pure Python) has no FFI; every entry point below
 * replaces a Python call on the hot path, cited as reference file:line.  Plain pointers
 * and sizes only: caller-owned host buffers, library-owned device buffers, int status
 * codes (0 = ok) and pint_last_error() for a message.  One context per host thread; each
 * context owns one HIP stream on one device.
 *
 * Data model (see DESIGN.md "Data layout in HBM"):
 *   - a *pulsar* is a packed SoA TOA set (N rows + 1 TZR row) plus a ModelSpec
 *     (structure: which components, column map, table offsets);
 *   - an *instance* is one parameter table (doubles, every parameter a double-double
 *     hi/lo pair, in the reference's par-file units) bound to a pulsar.  A batch of
 *     instances (grid points, PTA pulsars, downhill trial states) is evaluated by one
 *     launch sequence.
 */
#ifndef PINT_AMD_H
#define PINT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------------- */
#define PINT_OK 0
#define PINT_E_INVALID 1      /* bad argument / shape / unsupported model feature    */
#define PINT_E_HIP 2          /* HIP runtime error                                    */
#define PINT_E_NOT_PD 3       /* normal matrix not positive definite (LinAlgError)    */
#define PINT_E_KEPLER 4       /* Kepler iteration did not converge / ECC outside [0,1)*/
#define PINT_E_PARAM 5        /* invalid model parameter region (InvalidModelParameters)*/
#define PINT_E_SIGMA 6        /* Woodbury Sigma = Phi^-1 + U^T N^-1 U not positive definite */

/* ---- limits -------------------------------------------------------------------- */
#define PINT_MAX_COLS 320     /* design-matrix columns incl. Offset                   */
#define PINT_MAX_F 16
#define PINT_MAX_DMK 10
#define PINT_MAX_FD 10
#define PINT_MAX_JUMP 64
#define PINT_MAX_GLITCH 64    /* glitches per model (the JUMP cap; J0537-6910 has more than 32) */
#define PINT_MAX_WAVEX 128    /* WaveX harmonics, and DMWaveX harmonics, per model (wavex_setup par files
                                 carry 10-45 per component); CMWaveX harmonics too                   */
#define PINT_MAX_CM 16        /* ChromaticCM Taylor terms CM, CM1, ... per model                        */
#define PINT_MAX_ADDED_DELAY 1.0 /* s: the largest |WaveX + DMWaveX + ChromaticCM + CMWaveX| delay of a row
                                 for which the phase moved to it holds 1e-12 cycle (k_wavex); a model
                                 beyond it fails with PINT_E_PARAM.  The same bound, on its own, for
                                 |FDJump + FDJumpDM| (k_fdjump)                                        */
#define PINT_MAX_FDJUMP 64    /* FDJump parameters, and FDJumpDM parameters, per model: one 64-bit mask
                                 word per row and family                                               */
#define PINT_FDJUMP_MAX_INDEX 20 /* the largest FD index p of FD{p}JUMP{q} (fdjump.py:12)                */
#define PINT_MAX_PW 64        /* PiecewiseSpindown pieces per model (the glitch cap)                    */
#define PINT_MAX_WAVE 128     /* Wave terms WAVE1 ... WAVEn per model                                   */
#define PINT_MAX_IFUNC 1024   /* IFunc control points per model (tempo2's own limit is 1000)            */

/* ---- per-TOA packed input (reference TOAs.table columns
 *      toa.py:2320 tdbld, :2385-2439 posvels, freq, error, mjd_float, pulse_number) ---- */
typedef struct {
    int32_t n;                      /* TOAs, excluding the TZR row                      */
    const double *tdb_hi, *tdb_lo;  /* n+1: exact double-double split of longdouble tdbld (days) */
    const double *freq_mhz;         /* n+1                                              */
    const double *sigma_s;          /* n: scaled TOA uncertainty (s), noise_model.py:159 */
    const double *pos_km;           /* (n+1)*3 ssb_obs_pos (row-major xyz)              */
    const double *vel_kms;          /* (n+1)*3 ssb_obs_vel                              */
    const double *sun_km;           /* (n+1)*3 obs_sun_pos                              */
    const double *pulse_number;     /* n (NaN-free when track_mode=pulse numbers)       */
    const double *delta_pn;         /* n+1 delta_pulse_number                           */
    const uint32_t *flags;          /* n+1 bit0: barycentric obs, bit1: all ssb_obs_pos != 0 */
    const uint64_t *jump_mask;      /* n+1 bit k: JUMP k selects this TOA               */
    const int32_t *dmx_a, *dmx_b;   /* n+1 DMX bin indices (-1 none; two allow overlap) */
    const double *planet_km;        /* (n+1)*15 obs_<planet>_pos for jupiter, saturn, venus,
                                       uranus, neptune (toa.py:2403-2433); read only when
                                       spec.shapiro == 2, may be NULL otherwise             */
    const int32_t *dmx_x;           /* DMX bins beyond a TOA's first two (any number may overlap,
                                       dispersion_model.py:659-678): n+2 offsets into this array,
                                       then the bin indices; NULL when no TOA has more than two */
} pint_toas_t;

/* The same per-TOA input as the TOA table's own columns (n rows each, no TZR row) plus the TZR
 * TOA's values and the DMX ranges: the library forms the n+1-row pint_toas_t itself (the TZR
 * row appended, flags, DMX bins) -- the host packing of engine.pack_toas in native code. */
typedef struct {
    int32_t n;
    const double *tdb_hi, *tdb_lo;  /* n                                                  */
    const double *freq_mhz;         /* n                                                  */
    const double *pos_km;           /* n*3 ssb_obs_pos; vel_kms, sun_km likewise          */
    const double *vel_kms;
    const double *sun_km;
    const double *delta_pn;         /* n, or NULL (zeros)                                 */
    const double *mjd;              /* n float MJDs: the DMX ranges select on them (toa_select.py:101) */
    const uint8_t *is_bary;         /* n: barycentric observatory                         */
    const double *sigma_us;         /* n: scaled TOA uncertainty (us), noise_model.py:159  */
    const double *pulse_number;     /* n, or NULL (zeros)                                 */
    const uint64_t *jump_mask;      /* n+1, or NULL (no JUMPs)                            */
    const double *planet_km;        /* (n+1)*15 as in pint_toas_t, or NULL               */
    double tzr[15];                 /* the TZR TOA: tdb_hi, tdb_lo, freq_mhz, pos[3], vel[3], sun[3],
                                       delta_pn, mjd, is_bary (0/1)                      */
    int32_t ndmx;                   /* DMX ranges in parameter order (DMXR1_k, DMXR2_k)   */
    const double *dmx_r1, *dmx_r2;
} pint_toa_cols_t;

/* Form the pint_toas_t of `cols` into caller buffers (host only, no device): out->n and every
 * n+1 (n for sigma_s, pulse_number) array pointer must be set; dmx_x receives the overflow CSR
 * of TOAs in three or more bins when dmx_x_cap holds it.  Returns that CSR's length (0: none,
 * out->dmx_x set to NULL; larger than dmx_x_cap: nothing written to dmx_x, call again), or a
 * negative status.  Bit-identical to engine.pack_toas. */
int64_t pint_pack_toas(const pint_toa_cols_t *cols, pint_toas_t *out, int32_t *dmx_x, int64_t dmx_x_cap);

/* ---- model structure ------------------------------------------------------------ */
/* column kinds for the design matrix (timing_model.py:2073 designmatrix)              */
enum {
    PINT_COL_OFFSET = 0, PINT_COL_F = 1, PINT_COL_LON = 2, PINT_COL_LAT = 3,
    PINT_COL_PMLON = 4, PINT_COL_PMLAT = 5, PINT_COL_PX = 6, PINT_COL_DM = 7,
    PINT_COL_DMX = 8, PINT_COL_FD = 9, PINT_COL_JUMP = 10, PINT_COL_BIN = 11,
    PINT_COL_ZERO = 12,     /* a parameter without a delay (DMJUMP, dispersion_model.py:797) */
    PINT_COL_NESW = 13,     /* NE_SW: d_delay_d_ne_sw = DMconst * solar_wind_geometry / bfreq^2
                               (solar_wind_dispersion.py:404-412), d_dm_d_ne_sw = the geometry (:394) */
    PINT_COL_GLITCH = 14,   /* a Glitch parameter: col_index = 7 * glitch + PINT_GL_*; -d_phase_d_p / F0
                               on the TOAs the glitch acts on, 0 elsewhere (glitch.py:234-344); a timing
                               column like any other (its wideband DM rows are zero)                 */
    PINT_COL_WX = 15,       /* WXSIN_ / WXCOS_: col_index = 2 k + (0 sin, 1 cos), k the harmonic's position
                               in ascending index; d_delay_d_p = sin / cos (2 pi WXFREQ_k (tdb - WXEPOCH)),
                               the accumulated delay NOT subtracted (wavex.py:382-396); col_toff the
                               amplitude's table slot                                                */
    PINT_COL_DMWX = 16,     /* DMWXSIN_ / DMWXCOS_: the same indexing; d_dm_d_p = sin / cos (2 pi
                               DMWXFREQ_k (tdb - DMWXEPOCH)), times DMconst / bfreq^2 (dmwavex.py:373-387) */
    PINT_COL_CM = 17,       /* CM, CM1, ...: col_index = the Taylor order k; d_delay_d_p = DMconst
                               bfreq^(-TNCHROMIDX) dt^k / k!, dt years since CMEPOCH
                               (chromatic_model.py:64-90, :250-270)                                   */
    PINT_COL_CMWX = 18,     /* CMWXSIN_ / CMWXCOS_: col_index = 2 k + (0 sin, 1 cos); d_cm_d_p = sin / cos
                               (2 pi CMWXFREQ_k (tdb - CMWXEPOCH)), times DMconst bfreq^(-TNCHROMIDX)
                               (cmwavex.py:373-387)                                                   */
    PINT_COL_FDJUMP = 19,   /* FD{p}JUMP{q}: col_index = the parameter's place in pint_set_fdjump's block
                               (ascending p), also its bit in the row masks; d_delay_d_p = y^p on the
                               rows its mask selects, 0 elsewhere (fdjump.py:177-193)                  */
    PINT_COL_FDJUMPDM = 20, /* FDJUMPDM{q}: col_index = the place in the FDJumpDM block and the mask bit;
                               d_delay_d_p = -DMconst / bfreq^2 on the selected rows
                               (dispersion_model.py:877-884, :99-109)                                  */
    PINT_COL_PW = 21        /* PWPH_ / PWF0_ / PWF1_ / PWF2_: col_index = 4 * piece + (0 PH, 1 F0, 2 F1, 3 F2),
                               piece = the place in pint_set_phase_terms' block; -(1, dt, dt^2 / 2,
                               dt^3 / 6) / F0 on the rows inside the piece's window, exactly 0 outside
                               (piecewise.py:237-253)                                                 */
};
/* the parameters of one PiecewiseSpindown piece, in the order of its 7 table slots
 * (piecewise.py:130-138 pwsol_prop) */
enum {
    PINT_PW_EP = 0, PINT_PW_START, PINT_PW_STOP, PINT_PW_PH, PINT_PW_F0, PINT_PW_F1, PINT_PW_F2,
    PINT_PW_NPAR
};
/* the parameters of one glitch, in the order of its 7 table slots (glitch.py:130-138 glitch_prop) */
enum {
    PINT_GL_EP = 0, PINT_GL_PH, PINT_GL_F0, PINT_GL_F1, PINT_GL_F2, PINT_GL_F0D, PINT_GL_TD,
    PINT_GL_NPAR
};
/* binary parameter ids (stand_alone_psr_binaries/binary_generic.py, ELL1_model.py, DD_model.py,
 * ELL1H_model.py (H3, H4, STIGMA), DDK_model.py (KIN, KOM), DDS_model.py (SHAPMAX), DDH_model.py (H3,
 * STIGMA), ELL1k_model.py (OMDOT, LNEDOT)) */
enum {
    PINT_B_PB = 0, PINT_B_PBDOT, PINT_B_XPBDOT, PINT_B_A1, PINT_B_A1DOT, PINT_B_ECC,
    PINT_B_EDOT, PINT_B_T0, PINT_B_OM, PINT_B_OMDOT, PINT_B_M2, PINT_B_SINI, PINT_B_GAMMA,
    PINT_B_DR, PINT_B_DTH, PINT_B_A0, PINT_B_B0, PINT_B_TASC, PINT_B_EPS1, PINT_B_EPS2,
    PINT_B_EPS1DOT, PINT_B_EPS2DOT, PINT_B_H3, PINT_B_H4, PINT_B_STIGMA, PINT_B_KIN, PINT_B_KOM,
    PINT_B_NPAR0,                        /* the length of spec.o_bin                                   */
    PINT_B_SHAPMAX = PINT_B_NPAR0, PINT_B_LNEDOT,   /* their slots: PINT_SPEC_O_BINX(spec, id)          */
    PINT_B_NPAR,
    PINT_B_FB0 = PINT_B_NPAR             /* FBn: PINT_B_FB0 + n, n < PINT_MAX_FB; its slot: PINT_SPEC_O_FB(spec)
                                            + 2 n.  A PINT_COL_BIN column like the others: d orbits / d FBn =
                                            tt0^(n+1) / (n+1)! (times 2 pi into Phi / M) and d pbprime / d FBn =
                                            -pbprime^2 tt0^n / n!, carried through the chains of the PB column
                                            (binary_orbits.py:205-231), per 1 / s^(n+1), the par unit            */
};
#define PINT_MAX_FB 20                   /* orbital-frequency terms FB0 .. FB19 per pulsar                  */
/* binary models (spec.binary).
 * dds (DDS_model.py): DD with SINI = 1 - exp(-SHAPMAX) wherever DD uses SINI; d SINI / d SHAPMAX =
 *   exp(-SHAPMAX), no other parameter moves SINI.  SHAPMAX (dimensionless) must be > -log 2.
 * ddh (DDH_model.py, Freire & Wex 2010): DD with SINI = 2 s / (1 + s^2) and T_sun M2 = H3 / s^3,
 *   s = STIGMA > 0, H3 in s; the exact DD Shapiro delay -2 (H3 / s^3) log(logNum), not ELL1H's
 *   harmonic sum.  d delayS / d H3 = -2 log(logNum) / s^3; d delayS / d STIGMA = 6 H3 / s^4
 *   log(logNum) - 2 H3 / s^3 (-dSINI/ds X) / logNum, X = sin w (cos E - e) + sqrt(1 - e^2) cos w
 *   sin E, dSINI/ds = 2 / (1 + s^2) - 4 s^2 / (1 + s^2)^2 (the reference's column carries a stray
 *   1 / T_sun; this is the correct one).
 * ell1k (ELL1k_model.py, Susobhanan et al. 2018): ELL1 without EPS1DOT / EPS2DOT / EDOT; with dt =
 *   t - TASC, eps1 = (1 + LNEDOT dt)(EPS1 cos(OMDOT dt) + EPS2 sin(OMDOT dt)), eps2 = (1 + LNEDOT
 *   dt)(EPS2 cos(OMDOT dt) - EPS1 sin(OMDOT dt)); OMDOT deg / yr, LNEDOT 1 / yr.  The Roemer delay
 *   is the first-order a1 (sin Phi + (eps2 sin 2 Phi - eps1 (cos 2 Phi + 3)) / 2), with d Dre / d eps1
 *   = -a1 (cos 2 Phi + 3) / 2 and d Dre / d eps2 = a1 sin 2 Phi / 2; Drep, Drepp, their partials and
 *   the Shapiro delay are ELL1's.  d eps2 / d EPS2 = +d eps1 / d EPS1 (the reference has the
 *   opposite sign; this is the correct one).
 * A dds / ddh row whose Shapiro argument logNum is <= 0 sets PINT_E_KEPLER like a failed Kepler
 * solve.
 * The orbital-frequency orbit (binary_orbits.py:158-239 OrbitFBX; ELL1, ELL1H, DD and BT): when
 * PINT_SPEC_NFB(spec) > 0 the orbit is orbits = sum_n FBn tt0^(n+1) / (n+1)! (double-double), the
 * period pbprime = 1 / sum_n FBn tt0^n / n! and its rate pbdot = -pbprime^2 sum_{n>=1} FBn tt0^(n-1) /
 * (n-1)! wherever the model uses pb() and pbdot(); PB is absent (o_bin[PINT_B_PB] = -1), PBDOT and
 * XPBDOT are ignored and their columns are zero.  T0 (DD, BT): d orbits / d T0 = -1 / pbprime per
 * second, d pbprime / d T0 = -pbdot (the reference's column is zero; this is the correct one).  A row
 * whose orbital frequency is not positive sets PINT_E_KEPLER.  Such a pulsar's rows are evaluated by
 * a kernel build of their own (block kinds PINT_BLK_FB_*), never by the builds of the period form. */
enum { PINT_BIN_NONE = 0, PINT_BIN_ELL1 = 1, PINT_BIN_DD = 2, PINT_BIN_ELL1H = 3, PINT_BIN_BT = 4, PINT_BIN_DDK = 5,
       PINT_BIN_DDS = 6, PINT_BIN_DDH = 7, PINT_BIN_ELL1K = 8,
       PINT_NBIN = 9,
       /* block kinds of the evaluation past the binary models: the FBn form of ELL1, DD, ELL1H, BT */
       PINT_BLK_FB_ELL1 = 9, PINT_BLK_FB_DD = 10, PINT_BLK_FB_ELL1H = 11, PINT_BLK_FB_BT = 12,
       PINT_NBLK = 13 };

typedef struct {
    int32_t nf;             /* spin terms F0..F{nf-1}                                   */
    int32_t astrometry;     /* 0 none, 1 equatorial (RAJ/DECJ), 2 ecliptic (ELONG/ELAT) */
    int32_t shapiro;        /* SolarSystemShapiro: 0 absent, 1 the Sun, 2 the Sun and the
                               PLANET_SHAPIRO planets (solar_system_shapiro.py:105-117)    */
    int32_t ndm;            /* DispersionDM taylor terms (0 = component absent)         */
    int32_t ndmx;           /* DMX bins                                                 */
    int32_t binary;         /* PINT_BIN_*: 0 none, 1 ELL1, 2 DD, 3 ELL1H, 4 BT, 5 DDK,
                               6 DDS, 7 DDH, 8 ELL1k                                    */
    int32_t nfd;            /* FD terms                                                 */
    int32_t njump;          /* phase JUMPs                                              */
    int32_t track_pn;       /* 1: use_pulse_numbers, 0: nearest  (residuals.py:133-149) */
    int32_t subtract_mean;  /* residuals.py:124                                         */
    int32_t weighted_mean;
    int32_t ncol;           /* design-matrix columns incl. Offset                      */
    int32_t nred;           /* PLRedNoise modes (2*nred Fourier columns), 0 = none     */
    int32_t tstride;        /* doubles per instance parameter table                    */
    /* table offsets (doubles; each parameter is a dd pair at [off], [off+1]); -1 absent */
    int32_t o_F, o_PEPOCH, o_lon, o_lat, o_pmlon, o_pmlat, o_px, o_POSEPOCH;
    int32_t o_DM, o_DMEPOCH, o_DMX, o_FD, o_JUMP, o_bin[PINT_B_NPAR0];
    int32_t o_PHOFF;        /* PhaseOffset: table slot of PHOFF (-1 none); the TOAs' phase gets
                               -PHOFF, the TZR TOA's does not (phase_offset.py offset_phase)    */
    int32_t wb_noones;      /* 1: the Woodbury chi2 has no offset column of ones (PHOFF free,
                               residuals.py:583-585); the ECORR-only Sherman-Morrison chi2 of
                               :591-636 is this form with the ECORR basis alone             */
    int32_t ell1h;          /* ELL1H Shapiro form (binary_ell1.py:383-405): 1 H3 alone (Eq. 19,
                               stigma 0), 2 H3 + H4 (Eq. 19, stigma = H4/H3), 3 H3 + STIGMA
                               (exact, Eq. 29); 0 otherwise                                 */
    int32_t nharms;         /* ELL1H: last harmonic of Eq. 19 (NHARMS; max(NHARMS, 7) with H4) */
    int32_t dmn0;           /* first PLDMNoise mode among the nred Fourier modes (= nred: none);
                               modes >= dmn0 are scaled by (1400 MHz / f_bary)^2 per TOA
                               (noise_model.py:443-540 PLDMNoise.get_noise_basis)           */
    int32_t k96;            /* DDK: 1 = Kopeikin (1996) proper-motion terms on a1, omega and i
                               (K96, the reference default; DDK_model.py:157-349), 0 = off */
    int32_t o_DMJUMP;       /* DispersionJump: table slot of the first DMJUMP (-1 none); they
                               offset the modelled DM values only (dispersion_model.py:724-795) */
    int32_t ndmjump;        /* DMJUMPs (<= 64; bit k of the per-TOA DMJUMP mask selects DMJUMP k+1) */
    double obliquity;       /* rad, ecliptic models (pulsar_ecliptic.py OBL[ECL])       */
    double red_f0;          /* red-noise fundamental 1/T (Hz), noise_model.py:847       */
    int32_t o_NE_SW;        /* SolarWindDispersion, SWM 0: table slot of NE_SW (cm^-3; -1 absent, or
                               present, zero and frozen: the reference's delay is then zeros,
                               solar_wind_dispersion.py:388-392).  DM_sw = NE_SW * AU^2 rho /
                               (r sin rho) in pc, rho = pi - the pulsar-observatory-Sun angle
                               (:356-360, astrometry.py:114-150; Edwards et al. 2006 eq. 29-30);
                               its delay joins the sum after the Solar-system Shapiro delay and
                               before DispersionDM (timing_model.py DEFAULT_ORDER)              */
    int32_t o_GLITCH;       /* Glitch: table slot of the first glitch's block (-1 none).  Glitch k has 7
                               dd pairs at o_GLITCH + 14 k, in PINT_GL_* order and par units (GLEP MJD,
                               GLPH cycles, GLF0 Hz, GLF1 Hz/s, GLF2 Hz/s^2, GLF0D Hz, GLTD d).  With
                               dt = (tdb - GLEP) 86400 s - delay (the model's total delay), on the rows
                               with dt > 0 the phase gains GLPH + dt (GLF0 + dt GLF1 / 2 + dt^2 GLF2 / 6)
                               + GLF0D tau (1 - exp(-dt / tau)), tau = GLTD 86400 s, the last term only
                               when GLF0D != 0 (glitch.py:193-232); the TZR TOA like any TOA.  Glitch
                               registers no phase_derivs_wrt_delay (only spindown.py:85 does), so the
                               chain factor of the delay columns is unchanged                      */
    int32_t nglitch;        /* glitches (<= PINT_MAX_GLITCH), in ascending index                  */
    int32_t rsv_[3];        /* rsv_[id - PINT_B_NPAR0] = 1 + the table slot of binary parameter id for
                               the ids past o_bin (PINT_B_SHAPMAX, PINT_B_LNEDOT), 0 = absent: read
                               with PINT_SPEC_O_BINX.  Kept in the reserve, biased by one, so that
                               every field keeps its offset and a model without them keeps its spec
                               bytes (all-zero reserve).  rsv_[2]: the FBn block, nfb << 24 | (1 + the
                               table slot of FB0), 0 = the period form: nfb dd pairs FB0 .. FB{nfb-1},
                               contiguous and ascending; read with PINT_SPEC_NFB / PINT_SPEC_O_FB.
                               pint_add_pulsar returns -PINT_E_INVALID for nfb outside 1..PINT_MAX_FB, a
                               block outside the table, a binary model other than ELL1, ELL1H, DD, BT,
                               or a PB slot beside it                                               */
    int32_t col_kind[PINT_MAX_COLS];
    int32_t col_index[PINT_MAX_COLS];
    int32_t col_toff[PINT_MAX_COLS];  /* table offset of the column's parameter (-1: Offset) */
} pint_spec_t;

/* table slot of binary parameter id >= PINT_B_NPAR0 (-1 absent) */
#define PINT_SPEC_O_BINX(spec, id) ((spec).rsv_[(id) - PINT_B_NPAR0] - 1)
/* the FBn block: the number of terms (0: the period form) and the table slot of FB0 (-1 absent) */
#define PINT_SPEC_NFB(spec) ((int)((uint32_t)(spec).rsv_[2] >> 24))
#define PINT_SPEC_O_FB(spec) ((int)((uint32_t)(spec).rsv_[2] & 0xffffffu) - 1)
#define PINT_SPEC_FB(o_fb, nfb) ((int32_t)(((uint32_t)(nfb) << 24) | (uint32_t)((o_fb) + 1)))

/* ---- context -------------------------------------------------------------------- */
typedef struct pint_ctx pint_ctx;

/* One context per host thread; it owns one HIP stream on `device`. */
pint_ctx *pint_ctx_create(int device);
void pint_ctx_destroy(pint_ctx *ctx);
const char *pint_last_error(pint_ctx *ctx);

/* Instance buffers are drawn from a process-wide cache per device and returned to it by
 * pint_set_instances / pint_ctx_destroy; this hands every idle cached buffer back to the
 * HIP runtime (no reference counterpart: device memory management). */
void pint_release_cache(void);
int pint_device_count(void);
/* Pipeline slots of pint_step_end / pint_check_step, fixed when the library is built
 * (-DPINT_NSLOT, default 4): the host's slot bookkeeping must use this value. */
int pint_nslot(void);

/* Upload one pulsar (packed TOAs + model structure); returns its id >= 0, or -status.
 * Replaces the TOAs.table hand-off of get_model_and_toas (model_builder.py:859) and the
 * param-independent noise bases: red_freq[2*nred] are the PLRedNoise Fourier frequencies
 * as double-double pairs (hi[nred] then lo[nred]: the reference keeps them longdouble)
 * (noise_model.py:847 get_rednoise_freqs), red_phi[2*nred] their weights
 * (noise_model.py:780 get_noise_weights).  The library copies everything it needs. */
int pint_add_pulsar(pint_ctx *ctx, const pint_toas_t *toas, const pint_spec_t *spec,
                    const double *red_freq, const double *red_phi);
/* pint_add_pulsar from the TOA table's columns (pint_pack_toas into the context's scratch). */
int pint_add_pulsar_cols(pint_ctx *ctx, const pint_toa_cols_t *cols, const pint_spec_t *spec,
                         const double *red_freq, const double *red_phi);
/* WaveX / DMWaveX (wavex.py, dmwavex.py) of pulsar `psr`: the Fourier-series delay components,
 * described beside the spec (pint_spec_t keeps its layout).  Each component has one table block
 * of its harmonics in ascending index, three dd pairs per harmonic -- FREQ (1/d), SIN, COS (s;
 * pc cm^-3 for DMWaveX) -- at o_wx / o_dmwx (table slots, -1 for none), nwx / ndmwx harmonics
 * (<= PINT_MAX_WAVEX), and its epoch (WXEPOCH / DMWXEPOCH, MJD) in the dd pair just before the
 * block, at o - 2.  Both delays follow the binary's (timing_model.py DEFAULT_ORDER; dmwavex
 * sorts after everything), on every evaluation row, the TZR row included:
 *   WaveX    sum_k WXSIN_k sin a_k + WXCOS_k cos a_k, a_k = 2 pi WXFREQ_k (tdb - WXEPOCH - D),
 *            D the delay accumulated before it in days (wavex.py:365-380);
 *   DMWaveX  DMconst / bfreq^2 times sum_k DMWXSIN_k sin a'_k + DMWXCOS_k cos a'_k,
 *            a'_k = 2 pi DMWXFREQ_k (tdb - DMWXEPOCH) (dmwavex.py:355-371).
 * They run as a kernel of their own (k_wavex) after the evaluation and before the glitch
 * kernel; a batch with either component runs its residual pass unfused.  Call after
 * pint_add_pulsar* and before the first pint_set_instances that uses the pulsar; a model with
 * neither component makes no call. */
int pint_set_wavex(pint_ctx *ctx, int psr, int o_wx, int nwx, int o_dmwx, int ndmwx);
/* ChromaticCM / CMWaveX (chromatic_model.py, cmwavex.py) of pulsar `psr`, described beside the
 * spec like WaveX: delays DMconst bfreq^(-alpha) CM(t) with alpha = TNCHROMIDX, any real number.
 *   ChromaticCM  ncm (1..PINT_MAX_CM) Taylor terms CM, CM1, ... (per yr^k) as dd pairs at table
 *                slot o_cm, then CMEPOCH's pair (MJD; 0 when the model has none) and
 *                TNCHROMIDX's pair: CM(t) = sum_k CMk dt^k / k!, dt years since CMEPOCH;
 *   CMWaveX      ncmwx (<= PINT_MAX_WAVEX) harmonics in a block at o_cmwx laid out as a WaveX
 *                block (FREQ, SIN, COS; CMWXEPOCH's pair at o_cmwx - 2): CM(t) = sum_k CMWXSIN_k
 *                sin a'_k + CMWXCOS_k cos a'_k, a'_k = 2 pi CMWXFREQ_k (tdb - CMWXEPOCH).  Only
 *                beside a ChromaticCM, whose TNCHROMIDX it uses.
 * Both follow WaveX and DMWaveX in the delay sum, in this order, inside the same pass (the
 * chromatic build of k_wavex); a batch without chromatic terms launches what it launched
 * before.  The four delays of a row may sum to at most PINT_MAX_ADDED_DELAY.  Same calling
 * rule as pint_set_wavex; a model with neither component makes no call. */
int pint_set_chromatic(pint_ctx *ctx, int psr, int o_cm, int ncm, int o_cmwx, int ncmwx);
/* FDJump / FDJumpDM (fdjump.py, dispersion_model.py:805-884) of pulsar `psr`, described beside
 * the spec like WaveX: system-dependent delays selected per row by a mask.
 *   FDJump    nfdj (<= PINT_MAX_FDJUMP) values (s) as dd pairs at table slot o_fdj, value k of FD
 *             index fd_index[k] in 1..PINT_FDJUMP_MAX_INDEX, non-decreasing in k; bit k of
 *             mask[r] says that row r is selected by parameter k.  delay = sum_k [bit k] value_k
 *             y^fd_index[k], y = log(bfreq / 1 GHz) when use_log, else bfreq / 1 GHz; a
 *             non-finite y is 0 (fdjump.py:122-175);
 *   FDJumpDM  nfdjdm (<= PINT_MAX_FDJUMP) values (pc cm^-3) at o_fdjdm, bit k of dmmask[r]:
 *             delay = DMconst / bfreq^2 * sum_k [bit k] (-value_k).
 * mask and dmmask have n + 1 entries, the last the TZR TOA's; the library keeps device copies of
 * its own and frees them with the pulsar's other arrays; a family with no parameter may pass a
 * null mask.  Both delays follow WaveX, DMWaveX, ChromaticCM and CMWaveX in the delay sum, in this
 * order, in a pass of their own (k_fdjump, after k_wavex and before k_glitch); a batch without
 * them launches what it launched before.  The two delays of a row may sum to at most
 * PINT_MAX_ADDED_DELAY.  Wideband DM data with either is refused (pint_set_wideband).  Same
 * calling rule as pint_set_wavex; a model with neither component makes no call. */
int pint_set_fdjump(pint_ctx *ctx, int psr, int o_fdj, int nfdj, const int32_t *fd_index, int use_log,
                    const uint64_t *mask, int o_fdjdm, int nfdjdm, const uint64_t *dmmask);
/* PiecewiseSpindown, Wave and IFunc (piecewise.py, wave.py, ifunc.py) of pulsar `psr`: three
 * phase components, each added to a row's phase at the row's total delay, described beside the
 * spec like WaveX.
 *   PiecewiseSpindown  npw (<= PINT_MAX_PW) pieces at table slot o_pw, PINT_PW_NPAR dd pairs per
 *             piece in ascending index (PWEP, PWSTART, PWSTOP in MJD; PWPH, PWF0, PWF1, PWF2).  On
 *             the rows with PWSTART <= tdb < PWSTOP (the TOA's own TDB, not the emission time) the
 *             phase gains PWPH + dt (PWF0 + dt PWF1 / 2 + dt^2 PWF2 / 6), dt = (tdb - PWEP) 86400 s
 *             - delay; overlapping pieces both add; columns PINT_COL_PW;
 *   Wave      at o_wave the dd pairs of WAVEEPOCH (MJD) and WAVE_OM (rad / d), then nwave (<=
 *             PINT_MAX_WAVE) pairs of doubles (a_k, b_k) in seconds, k = 1 ... nwave:
 *             phase += F0 sum_k a_k sin(k b) + b_k cos(k b), b = WAVE_OM (tdb - WAVEEPOCH - delay / 86400 s);
 *   IFunc     nifunc (<= PINT_MAX_IFUNC) control points (x_hi + x_lo MJD, non-decreasing; y s) and
 *             the interpolation type sifunc: 2 linear between the points and constant outside them,
 *             0 the reference's piecewise-constant form as it runs (ifunc.py:131-134: y_0 before
 *             x_0, y_{n-1} from x_1 on, y_2 or at x_0 itself y_1 between; needs nifunc >= 3);
 *             phase += F0 times(tdb - delay / 86400 s).  The library keeps device copies of the
 *             three arrays and frees them with the pulsar.
 * Nothing of Wave or IFunc is fittable.  None of the three registers a derivative with respect
 * to the delay, so every other column is unchanged.  The TZR TOA is treated like any TOA.  A pass
 * of its own (k_phase_terms, after k_wavex and k_fdjump, beside k_glitch); a batch without the
 * components launches what it launched before.  Wideband DM data with any of them is refused.
 * A bad count, slot, pointer, order or type returns PINT_E_INVALID and leaves the pulsar as it
 * was.  Same calling rule as pint_set_wavex; a model with none of the three makes no call. */
int pint_set_phase_terms(pint_ctx *ctx, int psr, int o_pw, int npw, int o_wave, int nwave, int sifunc, int nifunc,
                         const double *ifunc_x_hi, const double *ifunc_x_lo, const double *ifunc_y);

/* Bind `ninst` instances (grid points, PTA pulsars, trial states): inst_psr[k] is a
 * pulsar id; `tables` concatenates each instance's parameter table (spec.tstride doubles,
 * dd pairs in par-file units).  Replaces the parameter state of a TimingModel
 * (parameter.py values) for a whole batch. */
int pint_set_instances(pint_ctx *ctx, int ninst, const int32_t *inst_psr, const double *tables);

/* A grid of npts instances of pulsar psr (gridutils.py:166 grid_chisq, :392, :588, :773 -- the
 * reference forms one model copy per point, gridutils.py:72): each point's table is `base`
 * (tstride doubles) with nvar (hi, lo) entries replaced, formed on the device from the base
 * table and the grid axes.  Variable j (table offset var_toff[j]) of point k takes the pair
 * vals_j[((k0 + k) / var_stride[j]) % var_size[j]], vals_j = the var_size[j] (hi, lo) pairs
 * of variable j in `vals` (the variables' pairs concatenated): a meshgrid's axis, or every
 * point's own value (stride 1).  k0: the global index of the first point (a rank's block).
 * Otherwise as pint_set_instances. */
int pint_set_grid(pint_ctx *ctx, int psr, int npts, const double *base, int nvar, const int32_t *var_toff,
                  const int64_t *var_stride, const int64_t *var_size, const double *vals, int64_t k0);
/* npts instances of pulsar psr, each with its own value of any number of parameters (a sampler's
 * walkers, a nested sampler's live points; BayesianTiming's batch): point k's table is `base`
 * (tstride doubles) with the nvar (hi, lo) entries at table offsets var_toff[j] replaced by
 * vals[2 (k nvar + j)], vals[2 (k nvar + j) + 1] -- point-major, npts x nvar pairs.  The tables are
 * formed on the device (k_point_tables: one map lookup per entry, so nvar is bounded by the table
 * alone, 2 nvar <= tstride; offsets must be distinct).  When the pulsar and the point count are
 * those of the resident pint_set_grid / pint_set_points batch, only the tables change -- no host
 * set-up, no instance upload (PINT_QUERY_NREUSE counts such calls).  Otherwise as
 * pint_set_instances. */
int pint_set_points(pint_ctx *ctx, int psr, int npts, const double *base, int nvar, const int32_t *var_toff,
                    const double *vals);
int pint_get_tables(pint_ctx *ctx, double *tables_out);
int pint_set_tables(pint_ctx *ctx, const double *tables);

/* Evaluate delay (timing_model.py:1515), phase (:1548, incl. the TZR phase) and, when
 * want_M, the design matrix (:2073) plus the red-noise basis columns; then residuals
 * (residuals.py:314 calc_phase_resids, :483 calc_time_resids) and the WLS chi2 (:638)
 * for every instance. */
int pint_eval(pint_ctx *ctx, int want_M);  /* want_M: 0 none, 1 full, 2 fit layout */

/* Copy results to caller buffers (any pointer may be NULL).  Residual rows are n_i per
 * instance, eval rows n_i+1 (last = TZR TOA), design matrices n_i x K_i column-major
 * with K_i = ncol + 2*nred.  pint_read_resids in lazy mode only enqueues its copies (pinned
 * buffers, valid after pint_check). */
int pint_read_resids(pint_ctx *ctx, double *time_resid, double *phase_resid, double *chi2_wls);
int pint_read_eval(pint_ctx *ctx, double *phase_hi, double *phase_lo, double *ftaylor, double *delay);
int pint_read_designmatrix(pint_ctx *ctx, double *M);

/* One normal-equations step for every instance on the state of the last pint_eval(1):
 * mode 0 = WLS (fitter.py:1965 WLSFitter / :1282 WLSState.step), mode 1 = GLS
 * (:2104 GLSFitter / :1425 GLSState.step, rank-reduced, full_cov=False).  The GLS mode
 * also factors the Woodbury Sigma used by pint_chi2_gls. */
int pint_fit_step(pint_ctx *ctx, int mode);
/* dpars/errs: (K_i+1) per instance (par units, [0] = Offset; noise coefficients after the
 * ncol timing columns); cov: ncol_i x ncol_i per instance (timing-parameter covariance,
 * fitter.py:2240 parameter_covariance_matrix); chi2_lin: linearised post-step chi2. */
int pint_read_step(pint_ctx *ctx, double *dpars, double *errs, double *cov, double *chi2_lin);

/* tables += lambda[k] * dpars (double-double add): fitter.py:957 take_step_model and
 * :2073-2080 the longdouble parameter update. */
int pint_apply_step(pint_ctx *ctx, const double *lambda_);
/* The same with one lambda for every instance (GLSFitter / WLSFitter take the full step,
 * fitter.py:2254-2263); a kernel argument, no host->device copy. */
int pint_apply_step_uniform(pint_ctx *ctx, double lambda_);
/* pint_fit_step followed by pint_apply_step_uniform(lambda_) (GLSFitter.fit_toas's step and
 * full-step update, fitter.py:2164-2263): when every instance takes the DMX-eliminated solve
 * on the generated-Fourier path the update and the new tables' per-instance constants are
 * formed at the end of the solve kernel, saving the apply launch.  pint_read_step and
 * pint_noise_resids read the step, not the tables, and may follow it. */
int pint_fit_step_apply(pint_ctx *ctx, int mode, double lambda_);

/* Device-resident parameter tables: pint_save_tables snapshots the batch's current tables
 * on the device, pint_restore_tables copies the snapshot back (device->device on the
 * stream), e.g. to start repeated fits from the same initial models without an upload. */
int pint_save_tables(pint_ctx *ctx);
int pint_restore_tables(pint_ctx *ctx);

/* GLS chi2 (Woodbury, residuals.py:567 _calc_gls_chi2 + utils.py:3074 woodbury_dot) of
 * the current residuals, per instance. */
int pint_chi2_gls(pint_ctx *ctx, double *chi2);

/* WLS chi2 (residuals.py:638-667 _calc_wls_chi2: sum (r / sigma_scaled)^2) of the current
 * residuals, per instance -- e.g. of residuals replaced by pint_debug_set_resids (the
 * residual pass reports its own through pint_read_resids). */
int pint_chi2_wls(pint_ctx *ctx, double *chi2);

/* ECORR epochs of pulsar `psr` (replaces EcorrNoise.ecorr_basis_weight_pair,
 * noise_model.py:385-427 + get_ecorr_epochs :808): nep epochs, TOA index lists in CSR form
 * (ep_ptr[nep+1], ep_idx[ep_ptr[nep]]) and the prior variance phi_e = ECORR^2 in s^2.
 * The quantisation block is eliminated by a Schur complement on the device (its normal
 * matrix block is diagonal), so it adds no Gram columns; on the compact layout each epoch
 * then couples to at most one DMX column (else the pulsar takes the full layout).  Call
 * before pint_set_instances.
 * Overlapping epochs: a TOA listed in two epochs (two ECORR parameters whose masks share TOAs)
 * is accepted here, but the block is then not diagonal and the per-epoch elimination is not
 * that model.  Every entry point that rests on it refuses a batch holding such a pulsar with
 * PINT_E_INVALID and a message naming overlapping ECORR epochs, before any launch and with no
 * state changed (deferred work stays deferred, the plan of pint_last_plan is all-zero):
 * pint_fit_step and pint_fit_step_apply in mode 1, pint_fit_step_enqueue, pint_chi2_gls,
 * pint_noise_resids, and the likelihoods pint_noise_lnlike and pint_point_lnlike_gls.  The
 * evaluation, mode 0 steps and the WLS chi2 are not affected. */
int pint_set_ecorr(pint_ctx *ctx, int psr, int nep, const int32_t *ep_ptr, const int32_t *ep_idx,
                   const double *ep_phi);

/* Fit layout of pulsar `psr` (no reference counterpart; for benchmarks/tests):
 * out4 = {compact, Gram columns excl. residual, sparse DMX columns, padded Gram width}.
 * compact = 1 when the DMX columns are kept out of M and the dense Gram (>= 8 free DMX
 * columns, no TOA in two free bins, no TOA in two ECORR epochs, every ECORR epoch's TOAs in at
 * most one free bin -- its elimination then keeps the DMX block diagonal, k_ecorr_dmx):
 * pint_eval(ctx, 2) then writes the compact
 * design matrix, and pint_fit_step forms their Gram rows as bin sums. */
int pint_fit_layout(pint_ctx *ctx, int psr, int32_t *out4);
/* The k_gram_v layout of a pulsar in the current batch: (on the vg path (+2 with the
 * binned DMX x Fourier tile, PINT_OPT_VBIN), DMX slots, LDS width [T | r | slots | F]
 * padded to 16, timing columns of the compact layout). */
int pint_vgram_layout(pint_ctx *ctx, int psr, int32_t *out4);
/* Wideband DM data of pulsar `psr` (n TOAs): the measured DMs pp_dm and their errors pp_dme
 * (the -pp_dm / -pp_dme TOA flags, toa.py:1767-1791), the errors scaled by DMEFAC/DMEQUAD
 * (ScaleDmError.scale_dm_sigma, noise_model.py:291), and each TOA's DMJUMP mask (bit k:
 * DMJUMP k+1 selects it).  All in pc/cm^3.  Replaces WidebandDMResiduals.get_dm_data
 * (residuals.py:1044-1071). */
int pint_set_wideband(pint_ctx *ctx, int psr, const double *pp_dm, const double *pp_dme,
                      const double *dm_sigma, const uint64_t *dmjump_mask);
/* WidebandDMResiduals.calc_resids / calc_chi2 (residuals.py:1000-1031) of every instance
 * whose pulsar has wideband data: pp_dm - total_dm (DispersionDM Taylor series + DMX +
 * DMJUMP, timing_model.py:1593) at the instance's parameters, the mean (weighted by
 * 1/pp_dme^2 unless use_weighted_mean = 0) removed if subtract_mean; chi2 with the scaled
 * errors.  resid_out: the instances' TOA rows concatenated (n per instance, 0 for pulsars
 * without wideband data), chi2_out[ninst] (NaN without wideband data). */
int pint_dm_resids(pint_ctx *ctx, int subtract_mean, int use_weighted_mean, double *resid_out,
                   double *chi2_out);

/* Lazy mode (1): launches return without synchronising or checking the device status;
 * pint_check() synchronises and returns the accumulated status.  In lazy mode
 * pint_set_tables, pint_read_step and pint_chi2_gls only enqueue their copies
 * (pint_read_step on a second stream, overlapped with the kernels that follow): host
 * buffers must stay valid, and outputs are complete, after pint_check().  Use pinned
 * buffers (pint_host_alloc) for the copies to run asynchronously. */
int pint_set_lazy(pint_ctx *ctx, int lazy);
int pint_check(pint_ctx *ctx);

/* Pipelined steps (replaces the per-step pint_check of a lazy-mode loop; no reference
 * counterpart -- the reference's fitters are synchronous).  pint_step_end closes the work
 * enqueued since the previous step_end and returns its slot (0 .. PINT_NSLOT-1) in *slot;
 * launches after it go to the next slot (own status word, timing events, fit-output
 * buffers).  pint_check_step waits for that step only and returns its status, so the host
 * enqueues the next steps while the device runs step k.  At most PINT_NSLOT steps in
 * flight: check slot s before ending the step that reuses it.  Pinned output buffers must
 * be per slot.  In lazy mode pint_read_step / pint_noise_resids(_dm) put their copy-stream
 * work behind the step's last kernel (at pint_step_end or pint_check), not behind the
 * solve. */
#ifndef PINT_NSLOT
#define PINT_NSLOT 4
#endif
int pint_step_end(pint_ctx *ctx, int *slot);
/* One GLSFitter.fit_toas(maxiter=1) step of every instance (fitter.py:2164-2289: the GLS
 * step, full_cov=False noise realisations :2269-2282, the post-fit chi2 it returns) enqueued
 * by a single call, lazy mode only: [pint_restore_tables when restore], pint_eval(2),
 * pint_fit_step_apply(mode = 1, lambda_), pint_read_step(dpars, errs, cov, chi2lin),
 * pint_noise_resids(noise_red, noise_ecorr), pint_noise_resids_dm(noise_dm), pint_eval(0),
 * pint_chi2_gls(chi2), pint_step_end(slot).  NULL outputs are skipped; pinned buffers
 * (pint_host_alloc), complete after pint_check_step(*slot). */
int pint_fit_step_enqueue(pint_ctx *ctx, int restore, int mode, double lambda_, double *dpars, double *errs,
                          double *cov, double *chi2lin, double *noise_red, double *noise_ecorr, double *noise_dm,
                          double *chi2, int *slot);
int pint_check_step(pint_ctx *ctx, int slot);
/* Engine options (no reference counterpart): PINT_OPT_BLOCKED_SOLVE = 1 (default) solves
 * the normal equations with the blocked FP64-MFMA kernel, 0 with the column-by-column
 * LDS kernel (used by the tests to cross-check the two).  PINT_OPT_VGRAM = 1 (default)
 * generates the PLRedNoise Fourier columns inside the Gram and Woodbury kernels of the
 * compact fit layout (never stored in M) and fuses the DMX bin sums into the Gram; 0
 * keeps them in M (the tests cross-check the two).  Takes effect at pint_set_instances. */
#define PINT_OPT_BLOCKED_SOLVE 1
#define PINT_OPT_VGRAM 2
/* PINT_OPT_TIMING_MASK: bit k enables timing slot k of pint_last_timing (default 0xff).
 * Every HIP timing event costs device time (~5 us each), so a timed run enables only the
 * slots it reports. */
#define PINT_OPT_TIMING_MASK 3
/* PINT_OPT_TIMING_EVERY k (default 1): the Gram kernels' timing events (slot 6) ride on
 * every k-th pint_fit_step only; the other steps carry no events.  The slot then reads 0
 * after an unsampled step. */
#define PINT_OPT_TIMING_EVERY 8
/* PINT_OPT_REFINE = 1 (default): a normal-equations solve whose condition estimate
 * max diag(A) * max diag(A^-1) exceeds 1e8 gets one pass of iterative refinement with a
 * double-double residual (the explicit L^-1 of the blocked solves otherwise loses ~cond(L)
 * digits that LAPACK's cho_solve keeps); 0 skips it (grid points: their post-fit chi2 is
 * second order in a step error along the weak directions). */
#define PINT_OPT_REFINE 4
/* PINT_OPT_VBIN = 1 (default): k_gram_v forms the DMX bins' Fourier entries from one binned
 * trig tile per k-step (the accumulator holds an even and an odd bin) instead of the DMX-slot
 * row tiles x Fourier columns; pulsars whose aligned 4-row groups hold more than two bins
 * (or two of one parity) leave the vg path.  Takes effect at pint_set_instances. */
#define PINT_OPT_VBIN 5
/* PINT_OPT_WBFIT = 1: pint_fit_step adds the wideband DM rows (pint_set_wideband) of every
 * compact-layout instance to its normal equations (WidebandTOAFitter.fit_toas,
 * fitter.py:2465-2637: design matrix [M_toa | F; M_dm | 0], residuals [r; pp_dm - DM]);
 * default 0.  With it set pint_fit_step returns PINT_E_INVALID, before any launch, when the
 * design matrix is in the full layout (pint_eval want_M = 1) or a pulsar with wideband data is
 * not on the compact DMX layout (pint_fit_layout): the DM rows would be left out. */
#define PINT_OPT_WBFIT 6
/* PINT_OPT_COV_DEFER (default 1, env PINT_COV_DEFER): the covariance of the DMX-eliminated
 * solve is formed by pint_read_step (k_cov_dmx, several workgroups per instance, on the copy
 * stream) instead of inside the solve: 0 never, 1 for batches of >= 16 instances, 2 always.
 * Same values bit for bit; takes effect at the next pint_fit_step. */
#define PINT_OPT_COV_DEFER 7
/* PINT_OPT_SCHUR = 1 (default): for deferred solves (PINT_OPT_COV_DEFER) the DMX-eliminated
 * solve's build phase -- column norms, S = A_dd, U = A_dx D^-1/2, S -= U U^T, b'_d -- runs as
 * k_schur, one workgroup per (block of S, instance), before the one-workgroup-per-instance
 * solve; 0 keeps it inside the solve.  Same operations in the same order: same bits. */
#define PINT_OPT_SCHUR 9
/* PINT_OPT_SMALL = 1 (default): instances of at most 32 padded columns and 512 rows (a
 * grid's points) take k_gram_s (a wave per instance, applies from the next
 * pint_set_instances) and the one-wave k_solve_blk (four instances per workgroup); 0 keeps
 * them on the 16-wave Gram and the 4-wave solve (the tests cross-check the two). */
#define PINT_OPT_SMALL 10
/* PINT_OPT_LA_CHOL = 1 (default, env PINT_LA_CHOL): the DMX-eliminated solve factors its
 * dense block with look-ahead (the next diagonal block factored beside the current trailing
 * update, L^-1's block rows beside the panels); 0 runs the plain blocked order.  The same
 * operations in the same order per block: the same bits. */
#define PINT_OPT_LA_CHOL 11
/* PINT_OPT_EFUSE = 1 (default, env PINT_EFUSE): batches off the small-instance path evaluate
 * 254 rows per block plus row 0 and the TZR row, and form the phase residuals and their
 * weighted sums there (the residual pass's first half, no k_resid1 launch); applies from the
 * next pint_set_instances. */
#define PINT_OPT_EFUSE 12
/* PINT_OPT_LANE_SOLVE = 1 (default, env PINT_LANE_SOLVE): small-instance batches (the
 * PINT_OPT_SMALL path) whose normal equations have at most 8 columns are solved with one
 * lane per instance (64 instances per wave) instead of one wave per instance. */
#define PINT_OPT_LANE_SOLVE 13
/* PINT_OPT_SPIN_EVAL = 1 (default, env PINT_SPIN_EVAL): a pint_set_grid batch whose points
 * differ in spin frequencies or glitch parameters only (isolated model, no red-noise basis) evaluates its rows'
 * delays and astrometric geometry once, on the first point, for the evaluation with the
 * design matrix that precedes the first fit step; each point then runs the spin part only.
 * The same bits as the full evaluation. */
#define PINT_OPT_SPIN_EVAL 14
/* PINT_OPT_SOLVE_W8 = 1 (default, env PINT_SOLVE_W8): the DMX-eliminated solve runs 8 waves
 * per instance (256 VGPRs per lane) when its dense block has at most 8 16-column blocks,
 * else 16.  The same operations per element: the same bits. */
#define PINT_OPT_SOLVE_W8 15
int pint_set_option(pint_ctx *ctx, int key, int value);
/* The SVD path of the fitters for degenerate normal equations (WLSState.step,
 * fitter.py:1282-1359: singular values of the whitened normalised M below threshold * s_max
 * dropped; GLSFitter fitter.py:2196-2230: SVD of mtcm when Cholesky fails), on the Gram of
 * the last pint_fit_step(mode), threshold[i] per instance: eigendecomposition of the normalised normal matrix (Jacobi,
 * on the device).  Replaces the outputs pint_read_step returns.  ndeg[i] = dropped
 * directions of instance i (<= PINT_EIG_MAXDEG); degvec[(i * PINT_EIG_MAXDEG + d) *
 * degstride + k] their components over the instance's fit columns, scaled to max |.| = 1,
 * smallest singular value first (degstride >= the widest instance's column count). */
#define PINT_EIG_MAXDEG 8
int pint_solve_eig(pint_ctx *ctx, int mode, const double *threshold, int32_t *ndeg, double *degvec,
                   int degstride);

/* Likelihood normalisation per instance, Residuals.calc_chi2(lognorm=True)
 * (residuals.py:567-589, :638-667): gls != 0 gives logdet(C)/2 of the last pint_chi2_gls
 * (C = N + U Phi U^T, U = [F, ECORR, 1], utils.py:3074 woodbury_dot), gls == 2 the same
 * for a correlated-noise model whose basis has no columns (U = [1]), gls == 0 gives
 * sum_i log sigma_i (s).  lnlikelihood = -(chi2/2 + lognorm). */
int pint_lognorm(pint_ctx *ctx, int gls, double *out);

/* HIP-graph capture of a launch sequence (lazy mode only).  Everything the calls between
 * pint_capture_begin and pint_capture_end enqueue (kernels, the copies to and from the
 * caller's pinned buffers, the side-stream work) becomes one graph; pint_graph_launch
 * replays it with one launch.  Device buffers and host pointers are fixed at capture, so a
 * replay re-runs the same batch on whatever those buffers hold (e.g. new parameter tables
 * written into the same pinned buffer).  One graph per pipeline slot (pint_step_end): a
 * capture belongs to the slot current at pint_capture_end (its outputs, status word and
 * pinned buffers), and pint_graph_launch replays the current slot's graph, so captured steps
 * pipeline two deep like enqueued ones.  pint_set_instances discards the graphs. */
int pint_capture_begin(pint_ctx *ctx);
int pint_capture_end(pint_ctx *ctx);
int pint_graph_launch(pint_ctx *ctx);
/* Introspection: PINT_QUERY_NVGRAM = 1 returns the number of instances of the current batch
 * on the generated-Fourier path, PINT_QUERY_NSPLIT = 2 the Gram's N-split count (row blocks
 * per instance), PINT_QUERY_NSPINEVAL = 3 the number of evaluations of this context that took
 * the shared head of a spin-only grid (PINT_OPT_SPIN_EVAL); negative status on error. */
#define PINT_QUERY_NVGRAM 1
#define PINT_QUERY_NSPLIT 2
#define PINT_QUERY_NSPINEVAL 3
#define PINT_QUERY_WFUSE 4      /* 1: the batch's residual pass forms the post-fit Woodbury dots (k_resid2
                                   tiles): every noise basis a PLRedNoise series of at most 63 modes */
#define PINT_QUERY_NREUSE 5     /* pint_set_grid / pint_set_points calls of this context that kept the resident
                                   batch (same pulsar, point count and options) and only formed new tables */
#define PINT_QUERY_NPLGLS 6     /* k_point_lnl_gls launches of this context (pint_point_lnlike_gls): a call refused
                                   before any launch leaves it unchanged */
#define PINT_QUERY_RESID_PATH 7 /* PINT_RESID_* bits: what the last pint_eval's residual pass launched or left
                                   pending (a later flush of the deferred second half adds its k_resid2 bit) */
#define PINT_RESID_EFUSED 1     /* first half in the evaluation's blocks */
#define PINT_RESID_R1_64 2      /* k_resid1<64> */
#define PINT_RESID_R1_256 4     /* k_resid1<256> */
#define PINT_RESID_R12 8        /* k_resid12 */
#define PINT_RESID_R2_64 16     /* k_resid2<64> */
#define PINT_RESID_R2_256 32    /* k_resid2<256> */
#define PINT_RESID_TILES 64     /* k_resid2 formed the Woodbury trig tiles */
#define PINT_RESID_DEFERRED 128 /* second half left to k_gram_v (or to the first reader of the residuals) */
#define PINT_QUERY_EVAL_PATH 8  /* PINT_EVALP_* bits: what the last pint_eval launched before its residual pass */
#define PINT_EVALP_PREP 1           /* k_prep formed the per-instance constants */
#define PINT_EVALP_PREP_LANES 2     /* k_prep_lanes did (a batch of small tables) */
#define PINT_EVALP_PREP_RESTORE 4   /* ... and whichever ran copied the pint_save_tables snapshot back first */
#define PINT_EVALP_SNAPSHOT 8       /* the evaluation read the snapshot and its constants and wrote them back
                                       (pint_restore_tables without a k_prep launch) */
#define PINT_EVALP_SW_GEOM 16       /* k_sw_geom (a solar-wind model in the batch) */
#define PINT_EVALP_SPIN 32          /* a spin-only grid's shared head and spin part instead of the block launches */
#define PINT_EVALP_MERGED 64        /* one launch for the isolated, ELL1 and DD blocks (k_eval_mix) */
#define PINT_EVALP_MERGED_BUDGET 128 /* ... at a fixed register budget (k_eval_mix_w) */
#define PINT_EVALP_KIND_BUDGET 256  /* some block kind's own launch ran a build at a fixed register budget */
#define PINT_QUERY_EVAL_KINDS 9 /* bit t set: block kind t (PINT_BIN_*, PINT_BLK_FB_*; PINT_NBLK bits) got a launch
                                   of its own in the last pint_eval */
int pint_query(pint_ctx *ctx, int key);
/* The launch plan of the last pint_fit_step (host bookkeeping, no reference counterpart): which
 * kernel instantiations the call enqueued, as the dispatcher chose them from the batch's padded
 * widths.  The tests assert it, so that a case written for one instantiation cannot stop
 * exercising it unnoticed when a threshold moves.  A pint_fit_step that refuses its batch
 * (PINT_E_INVALID before any launch) leaves an all-zero plan. */
#define PINT_PLAN_MAXVKEY 18
enum { PINT_PLAN_SOLVE_NONE = 0, PINT_PLAN_SOLVE_LANES4, PINT_PLAN_SOLVE_LANES8, PINT_PLAN_SOLVE_BLK1,
       PINT_PLAN_SOLVE_BLK4, PINT_PLAN_SOLVE_BLK16, PINT_PLAN_SOLVE_COLUMN };
typedef struct {
    int32_t gram_t_mask;    /* bit T: k_gram<T> launched (T = 1..9 upper tiles per wave)          */
    int32_t gram_ecorr;     /* the ECORR variants k_gram<T, ch, true> ran                        */
    int32_t gram_s;         /* k_gram_s ran                                                      */
    int32_t nvkey;          /* k_gram_v launches; vkey[i] = 10 (R - 1) + C, vkey_vb[i] the vb body */
    int32_t vkey[PINT_PLAN_MAXVKEY];
    int32_t vkey_vb[PINT_PLAN_MAXVKEY];
    int32_t nsplit;         /* Gram row blocks per instance                                      */
    int32_t greduce, dmx_rows, dmx, ecorr_dmx, wb_gram;  /* k_greduce, k_dmx_rows, k_dmx, k_ecorr_dmx, k_wb_gram ran */
    int32_t solve;          /* PINT_PLAN_SOLVE_*: the general solve kernel                       */
    int32_t solve_dmx_waves;/* k_solve_dmx<NW>: 0 (not launched), 8 or 16                        */
    int32_t fuse_sigma;     /* Woodbury Sigma factored in k_solve_dmx's grid                     */
    int32_t side_sigma;     /* ... by k_sigma on the side stream                                 */
    int32_t do_sigma;       /* ... inside k_solve                                                */
    int32_t sigma_waves;    /* k_sigma<NW>: 0, 4 or 16                                           */
    int32_t schur;          /* k_schur ran in front of k_solve_dmx                               */
    int32_t cov_deferred;   /* the covariance is left to k_cov_dmx at the read                   */
} pint_plan_t;
int pint_last_plan(pint_ctx *ctx, pint_plan_t *out);
/* Page-locked host memory for the output buffers (hipHostMalloc); NULL on failure. */
void *pint_host_alloc(size_t bytes);
void pint_host_free(void *p);
/* Introspection for tests: 0 Gram partials, 1 column sums of squares, 2 Woodbury factor
 * (L^-1, packed lower). */
int pint_debug_read(pint_ctx *ctx, int which, double *out);
/* Stage-wise parity introspection (SURVEY.md 8(a) parity definition 2; no reference
 * counterpart -- these expose the intermediate arrays of fitter.py:2164-2202):
 * pint_debug_gram writes, per instance, the assembled unnormalised normal matrix
 * [M | r]^T N^-1 [M | r] of the last pint_fit_step ((K_i+1)^2, original column order,
 * residual last; ECORR block eliminated, or with pre_ecorr != 0 its Schur term
 * sum_e s_e s_e^T / D_e added back) followed by M's K_i unweighted column sums of
 * squares (utils.py:2879 normalize_designmatrix).  pint_debug_set_resids replaces every
 * instance's time residuals (n_i each) by the caller's, so that pint_fit_step and
 * pint_chi2_gls run on e.g. the reference's own residual arrays. */
int pint_debug_gram(pint_ctx *ctx, int pre_ecorr, double *out);
int pint_debug_set_resids(pint_ctx *ctx, const double *time_resid);

/* The normalisation of the last pint_fit_step's design matrix, the reference fitters' `fac`
 * / `norm` squared (utils.py:2879 normalize_designmatrix; fitter.py:1320-1343 WLS,
 * fitter.py:2164-2176 GLS): per instance K_i values at the same K_i+1 stride as
 * pint_read_step's dpars.  mode 1: the unweighted column sums of squares of [M | F];
 * mode 0: the diagonal of the whitened normal matrix M^T N^-1 M.  Synchronous. */
int pint_read_norms(pint_ctx *ctx, int mode, double *out);

/* Per-instance status bits (1 << PINT_E_*) raised by evaluations since the last call, one
 * int32 per instance; reading clears them.  The batch status returned by pint_eval/
 * pint_check names the first error of any instance; this names the instances, so one
 * invalid grid point or trial state fails alone (fitter.py:926-935 InvalidModelParameters,
 * gridutils.py:89-106 NaN per point). */
int pint_inst_status(pint_ctx *ctx, int32_t *out);

/* Noise realisations of the last pint_fit_step(mode=1), n_i per instance (either pointer
 * may be NULL): red = F a (PLRedNoise basis times its fitted coefficients), ecorr = the
 * ECORR epoch coefficients back-substituted from the eliminated block, per TOA.  Replaces
 * Residuals.noise_resids as GLSFitter.fit_toas (fitter.py:2270-2282) and
 * DownhillGLSFitter.fit_toas (:1582-1605) set it. */
int pint_noise_resids(pint_ctx *ctx, double *red, double *ecorr);
/* The PLDMNoise realisation of the same step (its modes times (1400 MHz / f_bary)^2), n_i per
 * instance: Residuals.noise_resids["pl_DM_noise"] (zeros for pulsars without PLDMNoise).  In
 * lazy mode it is enqueued on the copy stream like pint_noise_resids (dm valid after
 * pint_check / pint_check_step; the next evaluation with M waits for it). */
int pint_noise_resids_dm(pint_ctx *ctx, double *dm);

/* Device time (ms, HIP events on the streams the kernels run on) of the last launches, 8
 * values: [0] eval (no design matrix), [1] resid, [2] ecorr + Gram + partial reduction,
 * [3] solve, [4] eval with design matrix, [5] Woodbury chi2, [6] the Gram kernels alone
 * (k_gram / k_gram_v), [7] the Gram partial reduction (k_greduce). */
int pint_last_timing(pint_ctx *ctx, double *ms8);
int pint_sync(pint_ctx *ctx);

/* ---- noise-parameter fitting ------------------------------------------
 * DownhillFitter._fit_noise (fitter.py:1230-1273) maximises the likelihood over the free
 * EFAC/EQUAD/ECORR/red-noise parameters with the residuals of the current timing model held
 * fixed (fitter.py:1239-1247: one Residuals object, only its model's noise values change).
 *
 * pint_set_resids replaces every instance's time residuals (n_i each, s): the fixed
 * residuals of such a fit (= pint_debug_set_resids).
 * pint_set_sigma replaces pulsar psr's scaled TOA uncertainties (s) in place
 * (ScaleToaError.scale_toa_sigma, noise_model.py:159, at trial EFAC/EQUAD values) and
 * pint_set_noise_weights its noise-basis prior variances (PLRedNoise 2 nred, ECORR nep; s^2;
 * either NULL), for a Woodbury likelihood (pint_fit_step(ctx,1) + pint_chi2_gls +
 * pint_lognorm(ctx,1)) at trial noise parameters of a model with time-correlated noise. */
int pint_set_resids(pint_ctx *ctx, const double *time_resid);
int pint_set_sigma(pint_ctx *ctx, int psr, const double *sigma_s);
int pint_set_noise_weights(pint_ctx *ctx, int psr, const double *red_phi, const double *ep_phi);
/* White-noise classes of pulsar psr: its TOAs grouped by the set of EFAC/EQUAD masks that
 * select them, CSR (cls_ptr[ncls+1], cls_idx[n]; every TOA in exactly one class), with the
 * raw TOA uncertainties sigma0_us[n] (us).  A class's scaled variance is
 * N_i = (sigma0_i^2 + Q^2) F^2, Q^2 = sum of its EQUAD^2, F = product of its EFACs. */
int pint_set_noise_classes(pint_ctx *ctx, int psr, int ncls, const int32_t *cls_ptr, const int32_t *cls_idx,
                           const double *sigma0_us);
/* Log-likelihood of the current (fixed) residuals of every instance at trial noise
 * parameters, one device pass: Residuals.lnlikelihood (residuals.py:713) with
 * kind[k] = 0 diagonal N (_calc_wls_chi2, :638), 1 N + ECORR blocks by Sherman-Morrison
 * (_calc_ecorr_chi2, :591; PHOFF free), 2 as 1 plus the 1e40 offset column of
 * _calc_gls_chi2 (:583-587).  cls_qf: (Q^2 [us^2], F) per class, instances' classes
 * concatenated; ep_w: ECORR variance (s^2) per epoch of the batch (NULL when no instance
 * has kind > 0 and epochs).  out3[3k] = lnL, [3k+1] = chi2, [3k+2] = logdet(C)/2.
 * Gradients (kinds 0 and 1; either pointer may be NULL): cls_g[2c] = sum_{i in c} N_i
 * dlnL/dN_i, cls_g[2c+1] = sum_{i in c} dlnL/dN_i (s^-2), ep_g[e] = dlnL/dw_e (s^-2) --
 * the chain-rule pieces of Residuals.d_lnlikelihood_d_param (residuals.py:718-828):
 * dlnL/dEFAC_p = sum_{c ∋ p} 2 cls_g[2c] / EFAC_p, dlnL/dEQUAD_p = sum_{c ∋ p}
 * 2 EQUAD_p F_c^2 1e-12 cls_g[2c+1], dlnL/dECORR_p = sum_{e of p} 2 ECORR_p 1e-12 ep_g[e]. */
int pint_noise_lnlike(pint_ctx *ctx, const int32_t *kind, const double *cls_qf, const double *ep_w, double *out3,
                      double *cls_g, double *ep_g);

/* ---- posterior sampling (bayesian.py BayesianTiming) ---------------------------------------
 * The white-noise log-likelihood of many points at once, every point with its own timing
 * parameters (pint_set_points) and its own EFAC / EQUAD / DMEFAC / DMEQUAD values.
 *
 * pint_set_dm_noise_classes: the DM-side twin of pint_set_noise_classes for a pulsar with
 * wideband DM data (after pint_set_wideband): its TOAs grouped by the set of DMEFAC / DMEQUAD
 * masks that select them, CSR, with the raw -pp_dme errors dme0[n] (pc/cm^3).  A class's scaled DM
 * error is sqrt(dme0_i^2 + Q^2) F, Q^2 the sum of its DMEQUAD^2, F the product of its DMEFACs
 * (ScaleDmError.scale_dm_sigma, noise_model.py:291).
 *
 * pint_point_lnlike, after pint_eval(ctx, 0): for every instance k, with its own (Q^2 [us^2], F) per
 * TOA class in cls_qf and (Q^2 [(pc/cm^3)^2], F) per DM class in dmcls_qf (the instances' classes
 * concatenated; dmcls_qf NULL when no pulsar of the batch has wideband data),
 *   out[5k]     lnL = -chi2_toa / 2 - sum log sigma_toa - chi2_dm / 2 - sum log sigma_dm
 *               (bayesian.py:202-252 _wls_nb_lnlikelihood / _wls_wb_lnlikelihood),
 *   out[5k + 1] chi2_toa, the time residuals over the point's scaled errors, the weighted mean
 *               taken with the point's own errors (unless the model has a PhaseOffset),
 *   out[5k + 2] sum_i log sigma_i, sigma in seconds,
 *   out[5k + 3] chi2_dm of pp_dm - (DM series + DMX + DMJUMP + NE_SW), no mean removed,
 *   out[5k + 4] sum_i log sigma_dm,i with sigma_dm in m^-2 (the reference takes the SI value of
 *               the pc/cm^3 errors: log(3.0856775814913673e22) per TOA more than in pc/cm^3);
 * the last two are 0 without wideband data.  ncls_tot / ndmcls_tot: the number of (Q^2, F) pairs
 * in each array.  PINT_E_INVALID with a message, before any launch, when a pulsar of the batch has
 * no classes (pint_set_noise_classes), has wideband data but no DM classes or dmcls_qf is NULL, or a
 * count is not the batch's sum of classes.  Lazy mode: only enqueued (cls_qf, dmcls_qf and out must
 * stay valid until pint_check), like pint_chi2_wls.  A zero or negative scaled error gives what
 * IEEE arithmetic gives the reference's expressions (infinities and NaNs), never an error. */
int pint_set_dm_noise_classes(pint_ctx *ctx, int psr, int ncls, const int32_t *cls_ptr, const int32_t *cls_idx,
                              const double *dme0);
int pint_point_lnlike(pint_ctx *ctx, int64_t ncls_tot, const double *cls_qf, int64_t ndmcls_tot,
                      const double *dmcls_qf, double *out);

/* pint_point_lnlike_gls, after pint_eval(ctx, 0) like pint_point_lnlike: the marginalised
 * correlated-noise log-likelihood of every instance k (Residuals.calc_chi2(lognorm=True),
 * residuals.py:567-716, utils.py:3074 woodbury_dot), every instance with its own values:
 *   cls_qf    (Q^2 [us^2], F) per TOA class, as for pint_point_lnlike: N_i = (sigma0_i^2 + Q^2) F^2 1e-12 s^2;
 *   ep_phi    one prior variance (s^2) per ECORR epoch of the pulsar (pint_set_ecorr's order);
 *   four_phi  the 2 nred prior variances (s^2) of the Fourier modes, PLRedNoise then PLDMNoise
 *             (sin, cos per mode), the order of the pulsar's red_phi;
 *   ones      1: the offset column of ones with Phi = 1e40 is appended (residuals.py:583-585, PHOFF
 *             not free), 0: not (PHOFF free; the ECORR-only form of _calc_ecorr_chi2 is this case).
 * With r the time residuals (the point's own weighted mean removed, none with a PhaseOffset),
 * U = [Fourier columns | PLDMNoise columns times the row's (1400 MHz / f_bary)^2 | ECORR epoch
 * indicators | ones], b = U^T N^-1 r and Sigma = Phi^-1 + U^T N^-1 U,
 *   out[4k]     lnL = -chi2 / 2 - logdet C / 2,
 *   out[4k + 1] chi2 = r^T N^-1 r - b^T Sigma^-1 b,
 *   out[4k + 2] logdet C / 2 = (sum log N_i + sum log Phi_j + logdet Sigma) / 2,
 *   out[4k + 3] logdet Sigma.
 * The Fourier modes of each component must be the harmonics 1, 2, ... of the pulsar's first mode
 * (get_rednoise_freqs' linspace(1/T, n/T, n)): the columns are rotations of the stored e^{i theta}.
 * Where Sigma is not positive definite (cho_factor raises in the reference) the instance's four
 * outputs are NaN and its PINT_E_SIGMA bit is raised (pint_inst_status); other instances are not
 * affected.  Zero or NaN variances give what IEEE arithmetic gives the expressions above.
 * ncls_tot / nep_tot / nphi_tot: the number of (Q^2, F) pairs, epoch variances and Fourier variances
 * passed.  PINT_E_INVALID with a message, before any launch (PINT_QUERY_NPLGLS unchanged), when a
 * pulsar of the batch has no noise classes, has wideband DM data (the wideband correlated likelihood
 * is not implemented), has overlapping ECORR epochs or more than 128 columns 2 nred + ones, or a
 * count is not the batch's sum.  Lazy mode: only enqueued (the arrays and out must stay valid until
 * pint_check). */
int pint_point_lnlike_gls(pint_ctx *ctx, int64_t ncls_tot, const double *cls_qf, int64_t nep_tot,
                          const double *ep_phi, int64_t nphi_tot, const double *four_phi, int ones, double *out);

/* ---- photon events (scripts/event_optimize.py, eventstats.py) --------------------------------
 * The rows of a pulsar taken as photons: after pint_eval(ctx, 0) the absolute phase of every row of
 * every instance is on the device, and the two calls below consume it as photon phases
 *   phi_i = frac(phase_i)  (abs_phase 0)   or   frac(phase_i - phase_TZR)  (abs_phase 1)
 * -- the reference's model.phase(toas, abs_phase=...).frac % 1 --, the fraction d - floor(d) taken in
 * double-double, rounded to a double and kept in [0, 1).
 *
 * pint_set_photons: the pulsar's photon data, beside its spec (calling rule of pint_set_wavex, at any
 * time after pint_add_pulsar; a second call replaces the data).  weights: n doubles (the pulsar's
 * row count), or NULL for unweighted data.  tmpl: nbin doubles, 1 <= nbin <= PINT_MAX_TEMPLATE, the
 * template at the phases j / nbin; or NULL with nbin 0 for no template (only the trig sums are then
 * available).  The library keeps device copies and frees them with the context.  PINT_E_INVALID with a
 * message for a bad pulsar, abs_phase, count or pointer; the pulsar's previous data stay in force.
 *
 * pint_point_photon_lnlike: for every instance k and each of its nphs (1..PINT_MAX_PHOTON_PHS) phase
 * offsets phs[k nphs + j],
 *   out[k nphs + j] = sum_i log(w_i T(x_ij) + 1 - w_i)   (sum_i log T(x_ij) without weights),
 *   x_ij = (phi_i + phs[k nphs + j]) mod 1 formed in doubles (event_optimize.py:143-145),
 *   T(x) = np.interp(x, arange(L) / L, tmpl, right=tmpl[0]): linear between the nodes j / L and
 *          (j + 1) / L for j < L - 1, and the constant tmpl[0] for x > (L - 1) / L -- a step at the last
 *          node, not an interpolation back to bin 0.
 * One offset per instance is emcee_fitter.lnposterior's likelihood; many offsets at one point are
 * marginalize_over_phase's scan at the cost of one evaluation.  A non-positive argument of the log
 * gives what IEEE arithmetic gives the reference (-inf, NaN) for that output only.
 *
 * pint_point_photon_trig: for every instance k and m (1..PINT_MAX_PHOTON_HARM) harmonics, 2 m + 2
 * doubles:
 *   out[k (2m + 2) + 2 (j - 1)]     = sum_i w_i cos(2 pi j phi_i),
 *   out[k (2m + 2) + 2 (j - 1) + 1] = sum_i w_i sin(2 pi j phi_i),   j = 1..m,
 *   then sum_i w_i and sum_i w_i^2  (w = 1 without weights):
 * the sums z2m, z2mw, hm, hmw and em_four are made of.
 *
 * Both: every output has the same bits on every run and whatever the batch around the instance
 * (fixed-order sums, no floating-point atomics); batches of several pulsars work, each with its own
 * data.  PINT_E_INVALID with a message, before any launch, when a pulsar of the batch has no photon
 * data (or no template, for the likelihood), a count is out of range, or the batch was not evaluated (no pint_eval since pint_set_instances /
 * pint_set_grid / pint_set_points / pint_set_tables, an applied step or pint_restore_tables).  Lazy
 * mode: only enqueued (phs and out must stay valid until pint_check), like pint_point_lnlike. */
#define PINT_MAX_TEMPLATE 4096     /* template bins: the table sits in LDS beside the reduction scratch */
#define PINT_MAX_PHOTON_PHS 1024   /* phase offsets per instance and call */
#define PINT_MAX_PHOTON_HARM 64    /* harmonics of the trig sums */
int pint_set_photons(pint_ctx *ctx, int psr, int abs_phase, const double *weights, int nbin, const double *tmpl);
int pint_point_photon_lnlike(pint_ctx *ctx, int nphs, const double *phs, double *out);
int pint_point_photon_trig(pint_ctx *ctx, int m, double *out);

/* ---- polycos (polycos.py; reference src/pint/polycos.py) --------------------------------------
 * tempo's piecewise polynomial phase predictor.  An entry (tmid, span, rphase, f0, coeffs) gives, with
 * dt = (t - tmid) 1440 minutes,
 *   phase(t) = rphase + 60 f0 dt + sum_i coeffs[i] dt^i,
 *   freq(t)  = f0 + (sum_i i coeffs[i] dt^(i-1)) / 60,   fdot(t) = (sum_i i (i-1) coeffs[i] dt^(i-2)) / 3600.
 * Every value that the reference keeps in longdouble crosses this interface as a (hi, lo) pair of
 * doubles with hi = (double)v, lo = (double)(v - hi), and the device works on pairs in double-double.
 * All five calls return when their outputs are complete (they synchronise, lazy mode or not).
 *
 * pint_polyco_fit: after pint_eval(ctx, 0), on instance inst whose rows are, per segment, nnode node
 * rows then the segment's mid-point row (so n = nseg (nnode + 1)), the TZR row last.  Per segment:
 *   rphase = phi(mid) - phi(TZR), split into an integer and a fraction in [-1/2, 1/2) (a pair);
 *   y_j = (phi(node_j) - phi(mid)) - 60 F0 dt_j in double-double, rounded to a double, with
 *         dt_j = dt_hi[s nnode + j] + dt_lo[...] minutes and F0 = f0_hi + f0_lo;
 *   coeffs[s ncoeff + i]: the least-squares polynomial of degree ncoeff - 1 through (dt_hi_j, y_j), by
 *         Householder QR of the Vandermonde matrix in dt / max |dt| (not by normal equations);
 *   rms[s]: the root mean square of the nnode residuals of that fit (cycles).
 * An output pointer may be NULL (not read back).  The result also stays on the device for
 * pint_set_polycos to adopt.  1 <= ncoeff <= PINT_MAX_POLYCO_COEFF, ncoeff <= nnode <=
 * PINT_MAX_POLYCO_NODES, else PINT_E_INVALID with a message before any launch; so for a batch that
 * was not evaluated or an instance of another row count.
 * pint_polyco_fit_host: the same kernel on phases given as host arrays of pairs, nseg (nnode + 1) + 1
 * rows in that order (the TZR row last).
 *
 * pint_set_polycos: the table used by the two calls below, nent entries sorted by t_start
 * (PINT_E_INVALID otherwise), ncoeff coefficients each (an entry with fewer: padded with zeros).
 * hdr: PINT_PC_NF fields of nent doubles each, field-major, in the order tmid hi, lo; t_start hi, lo;
 * t_stop hi, lo; rphase integer; rphase fraction hi, lo; f0 hi, lo.  c_hi, c_lo: nent x ncoeff.  Both
 * NULL: the coefficients and rphase of the last pint_polyco_fit are adopted on the device (nent and
 * ncoeff must be that fit's; the rphase fields of hdr are ignored).  A refused call leaves the previous
 * table in force.
 *
 * pint_polyco_eval: n times as pairs.  The entry of a time is found as the reference's find_entry does
 * (count(t_start < t) - 1 == count(t_stop < t), compared exactly on pairs: a time on a boundary
 * belongs to the earlier entry).  want: bit 0 the absolute phase as out_int (an integer as a double)
 * and out_frac (in [-1/2, 1/2)), bit 1 out_freq (Hz), bit 2 out_fdot (Hz/s); arrays not asked for may
 * be NULL.  A time that no entry covers gets NaN in every output and is counted in *n_uncovered.
 *
 * pint_polyco_trig: C_1, S_1, ..., C_m, S_m, sum w, sum w^2 of the polyco phases of the n times (w: n
 * weights or NULL), m in 1..PINT_MAX_PHOTON_HARM, in the layout of pint_point_photon_trig.  Computed
 * by a grid whose size depends on n only, each workgroup's partial sums added in index order: the
 * output's bits depend on the inputs only.  Uncovered times add nothing and are counted. */
#define PINT_MAX_POLYCO_COEFF 16
#define PINT_MAX_POLYCO_NODES 64
#define PINT_PC_NF 11
int pint_polyco_fit(pint_ctx *ctx, int inst, int nseg, int nnode, int ncoeff, const double *dt_hi, const double *dt_lo,
                    double f0_hi, double f0_lo, double *coeffs, double *rph_int, double *rph_frac_hi,
                    double *rph_frac_lo, double *rms);
int pint_polyco_fit_host(pint_ctx *ctx, int nseg, int nnode, int ncoeff, const double *ph_hi, const double *ph_lo,
                         const double *dt_hi, const double *dt_lo, double f0_hi, double f0_lo, double *coeffs,
                         double *rph_int, double *rph_frac_hi, double *rph_frac_lo, double *rms);
int pint_set_polycos(pint_ctx *ctx, int nent, int ncoeff, const double *hdr, const double *c_hi, const double *c_lo);
int pint_polyco_eval(pint_ctx *ctx, int64_t n, const double *t_hi, const double *t_lo, int want, double *out_int,
                     double *out_frac, double *out_freq, double *out_fdot, int64_t *n_uncovered);
int pint_polyco_trig(pint_ctx *ctx, int64_t n, const double *t_hi, const double *t_lo, const double *w, int m,
                     double *out, int64_t *n_uncovered);

/* ---- ensemble sampler (sampler.py EnsembleSampler) ---------------------------------------------
 * Goodman & Weare's affine-invariant stretch move in the red/blue half-ensemble form, resident on
 * the device: the nwalkers walkers (double-double positions), their log-posteriors, the proposals,
 * the priors, the accept test and the chain all stay there; per half-step the library enqueues
 *   k_ens_propose -> k_point_tables -> pint_eval's launches (residual pass included) ->
 *   k_point_lnl (or k_photon_lnl) -> k_ens_accept
 * on the context's stream, with no host copy and no synchronisation between steps.  The random
 * numbers are Philox4x32-10 blocks keyed by the seed and counted by (walker, step, half)
 * (csrc/ensemble.hpp): a chain depends on the seed, the start and the step
 * numbers only, and has the same bits on every run.
 *
 * pint_ens_init: the resident batch must be pint_set_points' with nwalkers / 2 points of one pulsar
 * (the walkers of one half are its instances; their values are overwritten), nvar variables whose
 * column in a walker's position is var_col[j].  kind PINT_ENS_WLS: the white-noise likelihood of
 * pint_point_lnlike, narrowband or wideband; PINT_ENS_PHOTON: pint_point_photon_lnlike at one phase
 * offset, the walker's column phase_col.  base_vals: nparams (hi, lo) pairs evaluated in place of a
 * proposal whose prior is not finite (nothing invalid runs on its account; it is rejected).  prior:
 * nparams rows of 6 doubles (kind, p0..p4: csrc/ensemble.hpp).  The class map tells which columns are
 * the EFACs and EQUADs of every noise class: imap = ncls, ndmcls, nent, then ef_ptr[ncls + 1],
 * eq_ptr[ncls + 1], dmef_ptr[ndmcls + 1], dmeq_ptr[ndmcls + 1] (ranges of entries) and ent_col[nent]
 * (a column, or -1: the fixed value fmap[e]); Q^2 of a class is the sum of its EQUAD entries' squares,
 * F the product of its EFAC entries, in entry order.  chunk: steps between two drains of the chain
 * (0: chosen from the sizes).  step0: the number of the first step (the Philox counter continues a
 * chain from there).  pos: nwalkers x nparams (hi, lo) pairs; their log-posteriors are evaluated
 * through the same launches, and PINT_E_INVALID is returned if one is not finite.
 * pint_ens_run: nsteps more steps; synchronises once per chunk, to drain the chain and to read the
 * status word (flagged proposals -- Kepler, added delay -- are rejections counted per walker, not
 * errors).  pint_ens_read: of the last pint_ens_run, chain_hi / chain_lo [nsteps][nwalkers][nparams]
 * and lnprob [nsteps][nwalkers]; counters: accepted[nwalkers] then flagged[nwalkers] since
 * pint_ens_init; state: the current positions hi[nwalkers][nparams], lo[...], then lnprob[nwalkers].
 * Any pointer may be NULL.  pint_ens_close frees the sampler (so does pint_ctx_destroy). */
#define PINT_ENS_WLS 0
#define PINT_ENS_PHOTON 1
int pint_ens_init(pint_ctx *ctx, int kind, int nwalkers, int nparams, int nvar, const int32_t *var_col,
                  const double *base_vals, const double *prior, int phase_col, int nimap, const int32_t *imap,
                  const double *fmap, uint64_t seed, double a, int chunk, int64_t step0, const double *pos);
int pint_ens_run(pint_ctx *ctx, int64_t nsteps);
int pint_ens_read(pint_ctx *ctx, double *chain_hi, double *chain_lo, double *lnprob, int32_t *counters, double *state);
int pint_ens_close(pint_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
