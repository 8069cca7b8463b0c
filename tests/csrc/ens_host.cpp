// A host program over csrc/ensemble.hpp for tests/test_sampler_host.py: it reads commands from its
// standard input and prints the header's results, doubles as C99 hex floats (exact).
//   philox c0 c1 c2 c3 k0 k1                    (hex words)       -> four hex words
//   draw seed walker step half nother           (decimal)         -> u_z idx u_acc z(a = 2) z(a = 1.5)
//   prop xk_hi xk_lo xj_hi xj_lo z              (hex floats)      -> y_hi y_lo
//   prior kind p0 p1 p2 p3 p4 x                 (hex floats)      -> the log-prior
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ensemble.hpp"

int main() {
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "philox")) {
            unsigned c[4], k[2];
            if (scanf("%x %x %x %x %x %x", &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) != 6) return 2;
            const ens_u4 r = philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
            printf("%08x %08x %08x %08x\n", r.v[0], r.v[1], r.v[2], r.v[3]);
        } else if (!strcmp(cmd, "draw")) {
            unsigned long long seed, step;
            unsigned walker, half;
            int nother;
            if (scanf("%llu %u %llu %u %d", &seed, &walker, &step, &half, &nother) != 5) return 2;
            const ens_draw d = ens_draws(seed, walker, step, half, nother);
            printf("%a %d %a %a %a\n", d.u_z, d.idx, d.u_acc, ens_stretch(2.0, d.u_z), ens_stretch(1.5, d.u_z));
        } else if (!strcmp(cmd, "prop")) {
            double v[5];
            for (double& x : v)
                if (scanf("%la", &x) != 1) return 2;
            const dd y = ens_propose(dd_make(v[0], v[1]), dd_make(v[2], v[3]), v[4]);
            printf("%a %a\n", y.hi, y.lo);
        } else if (!strcmp(cmd, "prior")) {
            double row[ENS_PRIOR_W], x;
            for (double& r : row)
                if (scanf("%la", &r) != 1) return 2;
            if (scanf("%la", &x) != 1) return 2;
            printf("%a\n", ens_lnprior(row, x));
        } else {
            return 2;
        }
    }
    return 0;
}
