/* norm3 (rt_device.hpp): the fused square root + three quotients against sqrt() and `/`; host-only model.
 * The device's v_rsq_f64 seed is modelled as RN(1/sqrt(s)) * (1 + d), |d| <= 2^-B uniformly at random
 * (and at both ends of the interval every 8th vector); B comes from the command line.  Vectors: random
 * directions at magnitudes 2^-250 .. 2^250, near-unit vectors (the output of a previous normalisation)
 * and vectors with one component 2^-500 times the others.
 * gcc -O2 -ffp-contract=off norm3_check.c -lm && ./a.out 5000000 18 */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
static uint64_t st = 88172645463325252ull;
static uint64_t rnd(void) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static double uni(void) { return (double)(rnd() >> 11) * 0x1p-53; }          /* [0,1) */
static double sym(void) { return 2.0 * uni() - 1.0; }                         /* [-1,1) */
/* sqrt_core: the refinement of the compiler's FP64 square root, same order */
static double sqrt_core(double s, double y, double* hh) {
    double g = s * y, h = y * 0.5;
    double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    double d = fma(-g, g, s);
    g = fma(d, h, g);
    d = fma(-g, g, s);
    *hh = h;
    return fma(d, h, g);
}
static int same(double a, double b) { return !memcmp(&a, &b, 8); }
int main(int argc, char** argv) {
    long n = argc > 1 ? atol(argv[1]) : 5000000;
    int B = argc > 2 ? atoi(argv[2]) : 18;
    int newton = argc > 3 ? atoi(argv[3]) : 1;   /* 0: y = h + h without the Newton step */
    const double dmax = ldexp(1.0, -B);
    long badL = 0, badq = 0, nq = 0;
    double worst_y = 0.0;
    for (long i = 0; i < n; ++i) {
        double v[3];
        for (int k = 0; k < 3; ++k) v[k] = sym();
        switch (i % 3) {
        case 0: { double m = ldexp(1.0, (int)(rnd() % 501) - 250); for (int k = 0; k < 3; ++k) v[k] *= m; break; }
        case 1: { double l = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); for (int k = 0; k < 3; ++k) v[k] /= l; break; }
        default: v[rnd() % 3] *= 0x1p-500; break;
        }
        const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        if (!(s >= 0x1p-600 && s <= 0x1p600 && fabs(v[0]) >= 0x1p-600 && fabs(v[1]) >= 0x1p-600 && fabs(v[2]) >= 0x1p-600))
            continue;   /* the device takes today's path */
        const double d = (i & 7) == 0 ? dmax : (i & 7) == 1 ? -dmax : sym() * dmax;
        const double seed = (1.0 / sqrt(s)) * (1.0 + d);
        double h;
        const double L = sqrt_core(s, seed, &h);
        const double y0 = h + h;
        const double y = newton ? fma(y0, fma(-L, y0, 1.0), y0) : y0;
        const double Lr = sqrt(s);
        if (!same(L, Lr)) { if (badL < 5) printf("L s=%a got %a want %a\n", s, L, Lr); ++badL; }
        const double ey = fabs(fma(y, Lr, -1.0));
        if (ey > worst_y) worst_y = ey;
        for (int k = 0; k < 3; ++k) {
            double q = v[k] * y;
            const double r = fma(-L, q, v[k]);
            q = fma(r, y, q);
            ++nq;
            if (!same(q, v[k] / Lr)) { if (badq < 5) printf("q a=%a L=%a got %a want %a\n", v[k], Lr, q, v[k] / Lr); ++badq; }
        }
    }
    printf("n=%ld seed error <= 2^-%d newton=%d: L mismatches %ld, quotient mismatches %ld of %ld, max |y*L - 1| = %.3g (2^%.1f)\n",
           n, B, newton, badL, badq, nq, worst_y, log2(worst_y));
    return badL || badq;
}
