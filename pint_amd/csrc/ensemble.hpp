// ensemble.hpp — the pieces of the affine-invariant ensemble sampler (Goodman & Weare's stretch
// move in the red/blue half-ensemble form, k_ens_propose / k_ens_accept) that a host program can
// check without a device: the counter-based random numbers, the mapping from one random block to
// a walker's three draws, the stretch factor, the double-double proposal and the log-priors.
// Host + device functions in the style of dd.hpp; DESIGN.md section 4 states the same layout, and
// the tests' numpy twin mirrors it.
#pragma once
#include <stdint.h>
#include "dd.hpp"

// ---- Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3") --------
struct ens_u4 {
    uint32_t v[4];
};

PD ens_u4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    ens_u4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// ---- the draws of one walker's move ------------------------------------------------------------
// key = (seed's low word, seed's high word); counter = (walker, step's low word, step's high word,
// half): one block per walker, step and half, so a chain is a pure function of the seed and its
// start -- reproducible, resumable at any step, and checkable from the host.
//   u_z   = (((r1 << 32 | r0) >> 11) + 0.5) 2^-53      53 bits, in (0, 1)
//   idx   = (r2 * nother) >> 32                        the partner among the nother walkers of the
//                                                      complementary half, with replacement
//   u_acc = (r3 + 0.5) 2^-32                           32 bits, in (0, 1)
struct ens_draw {
    double u_z, u_acc;
    int idx;
};

PD ens_draw ens_draws(uint64_t seed, uint32_t walker, uint64_t step, uint32_t half, int nother) {
    const ens_u4 r = philox4x32_10(walker, (uint32_t)step, (uint32_t)(step >> 32), half, (uint32_t)seed,
                                   (uint32_t)(seed >> 32));
    ens_draw d;
    const uint64_t m = (((uint64_t)r.v[1] << 32) | r.v[0]) >> 11;
    d.u_z = ((double)m + 0.5) * 0x1p-53;  // (m + 0.5 is exact: m < 2^53)
    d.idx = (int)(((uint64_t)r.v[2] * (uint64_t)(uint32_t)nother) >> 32);
    d.u_acc = ((double)r.v[3] + 0.5) * 0x1p-32;
    return d;
}

// the stretch factor z = ((a - 1) u + 1)^2 / a of the density g(z) ~ 1 / sqrt(z) on [1 / a, a]
PD double ens_stretch(double a, double u) {
    DD_NOCONTRACT
    const double t = (a - 1.0) * u + 1.0;
    return t * t / a;
}

// the proposal y = x_j + z (x_k - x_j): x_k the walker, x_j its partner
PD dd ens_propose(dd xk, dd xj, double z) { return dd_add(xj, dd_mul_d(dd_sub(xk, xj), z)); }

// ---- log-priors ----------------------------------------------------------------------------------
// One row of ENS_PRIOR_W doubles per parameter: the kind, then p[0..4].  Each kind follows the
// operations of the scipy.stats distribution that prior_info (or the model) gives the host, on the
// parameter's value rounded to double, so that the host's lnprior_batch is reproduced to rounding.
//   FLAT     0
//   UNIFORM  y = (x - p0) / p1, 0 <= y <= 1: 0 - p2 (p2 = log p1), else -inf       (uniform(loc, scale))
//   NORMAL   y = (x - p0) / p1: (-y^2 / 2 - p3) - p2 (p3 = log sqrt(2 pi))          (norm(mu, sigma))
//   PHASE    0 <= x <= 1: 0, else -inf
//   BNORMAL  y as NORMAL, p3 <= y <= p4: log(exp(-y^2 / 2) / sqrt(2 pi)) - p2, else -inf  (GaussianBoundedRV)
// A NaN value gives -inf (the host counts a NaN log-prior as -inf).
#define ENS_PRIOR_W 6
#define ENS_PRIOR_FLAT 0
#define ENS_PRIOR_UNIFORM 1
#define ENS_PRIOR_NORMAL 2
#define ENS_PRIOR_PHASE 3
#define ENS_PRIOR_BNORMAL 4

PD double ens_lnprior(const double* row, double x) {
    DD_NOCONTRACT
    const int kind = (int)row[0];
    const double* p = row + 1;
    const double ninf = -INFINITY;
    if (x != x) return ninf;
    if (kind == ENS_PRIOR_FLAT) return 0.0;
    if (kind == ENS_PRIOR_PHASE) return (x >= 0.0 && x <= 1.0) ? 0.0 : ninf;
    const double y = (x - p[0]) / p[1];
    if (kind == ENS_PRIOR_UNIFORM) return (y >= 0.0 && y <= 1.0) ? 0.0 - p[2] : ninf;
    if (kind == ENS_PRIOR_NORMAL) return (-(y * y) / 2.0 - p[3]) - p[2];
    if (kind == ENS_PRIOR_BNORMAL)
        return (y >= p[3] && y <= p[4]) ? log(exp(-0.5 * y * y) / sqrt(2.0 * 3.141592653589793)) - p[2] : ninf;
    return ninf;  // (an unknown kind never accepts: pint_ens_init refuses it first)
}
