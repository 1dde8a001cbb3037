// Stand-alone driver of csrc/fmt_f6.h for tests/test_fmt_f6_host.py: every token against snprintf("%f") over the hard list of the BVH
// writer's tests and a seeded stream of float64 values (random sign and mantissa, binary exponent uniform in -40 .. 39), and the refused
// values (NaN, +-inf, |x| >= 1e12) reported as refused with nothing written.  Each token is formatted into an exactly sized heap buffer,
// so a byte too many is the address sanitizer's to report.  Usage: fmt_f6_main <seed> <count>.  Prints "checked <n> tokens, <r> refusals".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../mocha_sigasia2023_amd/csrc/fmt_f6.h"

static long long g_bad = 0, g_checked = 0, g_refused = 0;

static void check(double x) {
    char want[400];
    const int wn = snprintf(want, sizeof want, "%f", x);
    const fmt_f6::Fixed f = fmt_f6::to_fixed(x);
    ++g_checked;
    if (f.len < 1 || f.len > fmt_f6::MAX_TOKEN) {
        if (++g_bad < 20) printf("MISMATCH %a: length %d, want \"%s\"\n", x, f.len, want);
        return;
    }
    unsigned char* got = (unsigned char*)malloc((size_t)f.len);
    const int gn = fmt_f6::format(x, got);
    if (gn != wn || memcmp(got, want, (size_t)wn) != 0)
        if (++g_bad < 20) printf("MISMATCH %a: got \"%.*s\", want \"%s\"\n", x, gn, (const char*)got, want);
    free(got);
}

static void refused(double x) {
    unsigned char* guard = (unsigned char*)malloc(1);
    guard[0] = 0xA5;
    ++g_refused;
    if (fmt_f6::format(x, guard) != 0 || fmt_f6::to_fixed(x).len != 0 || guard[0] != 0xA5)
        if (++g_bad < 20) printf("NOT REFUSED %a\n", x);
    free(guard);
}

static unsigned long long g_state;
static unsigned long long next64() {                          // splitmix64
    unsigned long long z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: fmt_f6_main <seed> <count>\n"); return 2; }
    g_state = strtoull(argv[1], nullptr, 10);
    const long long count = atoll(argv[2]);

    std::vector<double> hard = {0.0, 5e-7, 4.9e-7, 5.1e-7, 1e-9, 5e-324, 0.9999995, 0.9999994999, 9.9999995, 99999.9999995, 999999.9999995,
                                nextafter(1e12, 0.0), 2.2250738585072014e-308, 1.5, 0.5, 2.5e-6, 3.5e-6};
    for (int k = 7; k <= 20; ++k) {
        const double p = ldexp(1.0, k);
        for (double j : {1.0, 3.0, 5.0, p + 1.0, 3.0 * p - 1.0}) hard.push_back(j / p);
    }
    double d = 7.25;                                          // one value of every integer-digit count 1 .. 12
    for (int n = 1; n <= 12; ++n, d = d * 10.0 + 0.0000005) hard.push_back(d);
    for (int n = 1; n <= 9; ++n) hard.push_back(pow(10.0, n) - 0.0000004);        // 9.9999996, 99.9999996, ...: carries into a new digit
    for (double x : hard) { check(x); check(-x); }

    // the two ties the writer's tests name: half-even, not half-up
    unsigned char t[fmt_f6::MAX_TOKEN];
    if (fmt_f6::format(1.0 / 128, t) != 8 || memcmp(t, "0.007812", 8)) { ++g_bad; printf("MISMATCH 1/128\n"); }
    if (fmt_f6::format(3.0 / 128, t) != 8 || memcmp(t, "0.023438", 8)) { ++g_bad; printf("MISMATCH 3/128\n"); }
    if (fmt_f6::format(-0.0, t) != 9 || memcmp(t, "-0.000000", 9)) { ++g_bad; printf("MISMATCH -0.0\n"); }

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double x : {inf, nan, 1e12, nextafter(1e12, inf), 1e13, 1e300, std::numeric_limits<double>::max()}) { refused(x); refused(-x); }

    for (long long i = 0; i < count; ++i) {
        const unsigned long long r = next64(), q = next64();
        const unsigned long long mant = r & 0xfffffffffffffull;
        const unsigned long long ex = 1023 - 40 + q % 80;     // 2^-40 .. 2^39
        const unsigned long long bits = (q >> 63) << 63 | ex << 52 | mant;
        double x;
        memcpy(&x, &bits, sizeof x);
        if (fabs(x) < 1e12) check(x); else refused(x);        // the top of the 2^39 binade lies above 1e12
    }
    printf("checked %lld tokens, %lld refusals\n", g_checked, g_refused);
    return g_bad ? 1 : 0;
}
