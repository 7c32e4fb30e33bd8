/* spec_skips (rt_device.hpp, RT_SPEC_SKIP): one lit (sample, light) of shade()'s point-light pass 2 evaluated
 * twice in host double arithmetic, today's way and with the specular term left out where the device leaves it
 * out; the colour E = combine(E0, combine(Ed, Es)) has to be bit-equal whenever the skip condition holds, and the
 * clamped r.v it replaces has to be +-0 there.  Host-only; no FMA contraction, as the host and device builds.
 * Cases (i % 8):
 *   0, 1  random unit n, wi, wo; exponents: integers 0..1023, non-integers, negatives
 *   2     near-unit n, wi, wo (each scaled by 1 + t, |t| <= 1e-3)
 *   3     u = rv.wo steered to t * 2^-40, t in [-4, 4] or exactly +-1 margin: both sides of the margin
 *   4     n = 0, the inside-at-origin hits: rv = -wi
 *   5     |wi| < 1, the clamped near-light case, down to lengths where normalized() takes its fallback
 *   6     ks = 0 or shininess = 0
 *   7     a NaN in one component of n, wi, wo or in the shininess
 * gcc -O2 -ffp-contract=off spec_skip_check.c -lm && ./a.out 50000000 */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
static uint64_t st = 88172645463325252ull;
static uint64_t rnd(void) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static double uni(void) { return (double)(rnd() >> 11) * 0x1p-53; }          /* [0,1) */
static double sym(void) { return 2.0 * uni() - 1.0; }                         /* [-1,1) */
typedef struct { double x, y, z; } V3;
static double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 normalized(V3 v) {   /* Dir3::normalized */
    const double L = sqrt(dot3(v, v));
    if (L > 1e-6) { V3 r = {v.x / L, v.y / L, v.z / L}; return r; }
    V3 f = {0.0, 1.0, 0.0};
    return f;
}
static V3 unit(void) {
    for (;;) {
        V3 v = {sym(), sym(), sym()};
        const double s = dot3(v, v);
        if (s > 0.01 && s <= 1.0) return normalized(v);
    }
}
static V3 scale(V3 v, double t) { V3 r = {v.x * t, v.y * t, v.z * t}; return r; }
static V3 cross(V3 a, V3 b) { V3 r = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; return r; }
/* pow_spec: the unnormalised double-double for integer exponents 0..1023, libm otherwise */
static double pow_spec(double x, double y) {
    const int k = (int)y;
    if (!(y >= 0.0 && y < 1024.0 && (double)k == y)) return pow(x, y);
    if (k == 0) return 1.0;
    const int top = 31 - __builtin_clz(k);
    double h = x, l = 0.0;
    for (int i = top - 1; i >= 0; --i) {
        double p = h * h;
        l = fma(h + h, l, fma(h, h, -p));
        h = p;
        if ((k >> i) & 1) { p = h * x; l = fma(l, x, fma(h, x, -p)); h = p; }
    }
    return h + l;
}
static int spec_skips(V3 rv, double s, V3 wo, double shin) {
    const int loop = shin > 0.0 && shin < 1024.0 && (double)(int)shin == shin;   /* 1 .. 1023: pow_spec's loop */
    return loop && s >= 0x1p-20 && s <= 4.0 && dot3(rv, wo) <= -0x1p-40;
}
static V3 combine(V3 a, V3 b) {
    V3 r = {1.0 - (1.0 - a.x) * (1.0 - b.x), 1.0 - (1.0 - a.y) * (1.0 - b.y), 1.0 - (1.0 - a.z) * (1.0 - b.z)};
    return r;
}
static double exponent(void) {
    switch (rnd() % 8) {
    case 0: return 12.5;
    case 1: return 64.0 * uni();              /* a non-integer */
    case 2: return -(double)(rnd() % 8) - 0.5 * (double)(rnd() % 2);   /* <= 0 */
    case 3: return (double)(rnd() % 1024);
    default: return (double)(1 + rnd() % 32);  /* the scenes' own range */
    }
}
int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 50000000;
    const double NaN = nan("");
    long cases[8] = {0}, skips[8] = {0}, bad = 0, bad_zero = 0, bad_guard = 0, near_in = 0, near_out = 0;
    for (long i = 0; i < n; ++i) {
        const int kind = (int)(i % 8);
        V3 nn = unit(), wi = unit(), wo = unit();
        double shin = exponent(), ks = 0.05 + uni();
        /* a lit light has n.wi > 0 (kind 4 sets n = 0 afterwards, kind 7 may break it with a NaN) */
        if (dot3(nn, wi) <= 0.0) nn = scale(nn, -1.0);
        switch (kind) {
        case 2:
            nn = scale(nn, 1.0 + 1e-3 * sym()), wi = scale(wi, 1.0 + 1e-3 * sym()), wo = scale(wo, 1.0 + 1e-3 * sym());
            break;
        case 4: nn.x = nn.y = nn.z = 0.0; break;
        case 5: wi = scale(wi, (i & 8) ? uni() : ldexp(1.0, -(int)(rnd() % 40))); break;
        case 6:
            if (i & 8) ks = 0.0; else shin = (i & 16) ? 0.0 : -0.0;
            break;
        case 7: {
            double* f[10] = {&nn.x, &nn.y, &nn.z, &wi.x, &wi.y, &wi.z, &wo.x, &wo.y, &wo.z, &shin};
            *f[rnd() % 10] = NaN;
            break;
        }
        default: break;
        }
        const double ndw = dot3(nn, wi);
        const V3 rv = {2.0 * ndw * nn.x - wi.x, 2.0 * ndw * nn.y - wi.y, 2.0 * ndw * nn.z - wi.z};
        const double s = dot3(rv, rv);
        if (kind == 3) {   /* wo = a unit vector across rv, moved along rv so that rv.wo = t 2^-40 */
            const V3 p = normalized(cross(rv, unit()));
            const int m = (int)(rnd() % 4);
            const double t = m == 0 ? -1.0 : m == 1 ? 1.0 : 4.0 * sym();
            const double c = t * 0x1p-40 / s;
            wo.x = p.x + c * rv.x, wo.y = p.y + c * rv.y, wo.z = p.z + c * rv.z;
            if (i & 8) wo = normalized(wo);
            if (fabs(dot3(rv, wo)) <= 0x1p-38) { if (dot3(rv, wo) <= -0x1p-40) ++near_in; else ++near_out; }
        }
        /* the rest of the lane's light: Ed, IL and the colour so far, all in [0, 1.5) */
        const V3 IL = {3.0 * uni(), 3.0 * uni(), 3.0 * uni()};
        const V3 Ed = {0.4 * uni() * IL.x, 0.4 * uni() * IL.y, 0.4 * uni() * IL.z};
        const V3 E0 = {uni(), uni(), uni()};
        /* today's text */
        V3 EsA = {0.0, 0.0, 0.0};
        double rdotv = 0.0;
        if (ks > 0.0) {
            const V3 rr = normalized(rv);
            rdotv = fmax(0.0, dot3(rr, wo));
            const double spec = pow_spec(rdotv, shin) * ks;
            EsA.x = IL.x * spec, EsA.y = IL.y * spec, EsA.z = IL.z * spec;
        }
        const V3 A = combine(E0, combine(Ed, EsA));
        /* with the skip */
        V3 EsB = {0.0, 0.0, 0.0};
        int skip = 0;
        if (ks > 0.0) {
            skip = spec_skips(rv, s, wo, shin);
            if (!skip) EsB = EsA;   /* (the same operations on the same values) */
        }
        const V3 B = combine(E0, combine(Ed, EsB));
        ++cases[kind];
        if (!skip) continue;
        ++skips[kind];
        if (memcmp(&A, &B, sizeof A)) {
            if (bad < 5) printf("E differs: kind %d rv=(%a %a %a) wo=(%a %a %a) shin=%a\n", kind, rv.x, rv.y, rv.z, wo.x, wo.y, wo.z, shin);
            ++bad;
        }
        if (!(rdotv == 0.0) || !(EsA.x == 0.0 && EsA.y == 0.0 && EsA.z == 0.0)) {
            if (bad_zero < 5) printf("skipped, but r.v = %a, Es = (%a %a %a): kind %d shin=%a\n", rdotv, EsA.x, EsA.y, EsA.z, kind, shin);
            ++bad_zero;
        }
        /* the guards: only at an integer exponent 1 .. 1023, never where normalized() falls back or with a NaN about */
        if (!(shin >= 1.0 && shin <= 1023.0 && floor(shin) == shin) || !(sqrt(s) > 1e-6) || kind == 7 || s != s) {
            if (bad_guard < 5) printf("skipped against a guard: kind %d s=%a shin=%a\n", kind, s, shin);
            ++bad_guard;
        }
    }
    static const char* names[8] = {"unit", "unit", "near-unit", "margin", "n = 0", "|wi| < 1", "ks / shin = 0", "NaN"};
    for (int k = 0; k < 8; ++k) printf("kind %d %-14s cases %10ld  skipped %10ld\n", k, names[k], cases[k], skips[k]);
    printf("margin cases with |u| <= 2^-38: %ld skipped side, %ld kept side\n", near_in, near_out);
    printf("n=%ld: E mismatches %ld, non-zero skipped terms %ld, guard violations %ld\n", n, bad, bad_zero, bad_guard);
    /* the cases must have exercised what they are for */
    const int covered = skips[0] > 0 && skips[2] > 0 && skips[3] > 0 && skips[4] > 0 && skips[5] > 0 && near_in > 0 &&
                        near_out > 0 && skips[7] == 0;
    if (!covered) printf("coverage: a case kind never skipped (or a NaN case did)\n");
    return (bad || bad_zero || bad_guard || !covered) ? 1 : 0;
}
