// "%f" of a float64, in integers, for the host and the device: the correctly rounded six-decimal expansion, ties to even - what the
// reference's BVH writer emits for every number (motion/bvh.py:215-222, Python's "%f").  No HIP header: g++ compiles this file alone.
//
// A finite x = +-m 2^e (m < 2^53; a denormal is e = -1074 without the hidden bit).  |x| 10^6 = P 2^(e+6) exactly, P = m 15625 < 2^67 held
// in two 64-bit words.  With s = -(e+6):  N = P >> s, plus one when the shifted-out remainder is above half, or exactly half with N odd.
// The token is [-] (the sign BIT: -0.0 and -1e-9 print "-0.000000"), the digits of N / 10^6 (at least one), '.', the six digits of
// N % 10^6.  Admitted: finite, |x| < 1e12.  Then s >= 7, N < 10^18 fits a uint64 and the token has at most 20 bytes (sign + 12 + 7);
// nothing rounds up past 10^12 (the float64 spacing there is 1.2e-4).  NaN, +-inf and |x| >= 1e12 are refused: the length is 0.
// A carry into a new digit (9.9999995 -> 10.000000) comes out of counting the digits of N AFTER rounding.  The only divisions are by
// the constants 10^6 and 10^9 (multiply-high) and by 10 on 32-bit pieces; nothing keeps an array, so nothing goes to scratch.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__) || defined(__CUDACC__)
#define FMT_F6_HD __host__ __device__
#else
#define FMT_F6_HD
#endif

namespace fmt_f6 {

constexpr int MAX_TOKEN = 20;                                 // bytes, without the space the BVH writer puts behind it

struct Fixed {
    uint64_t n;                                               // round(|x| 10^6), ties to even
    int neg;                                                  // the sign bit
    int len;                                                  // bytes of the token, 0 = refused
};

FMT_F6_HD inline uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

FMT_F6_HD inline uint64_t bits_of(double x) {
    union { double d; uint64_t u; } v;
    v.d = x;
    return v.u;
}

// decimal digits of ip < 10^12, at least one
FMT_F6_HD inline int int_digits(uint64_t ip) {
    int d = 1;
    uint64_t p = 10;
    while (d < 12 && ip >= p) { ++d; p *= 10; }
    return d;
}

FMT_F6_HD inline Fixed to_fixed(double x) {
    const uint64_t u = bits_of(x), a = u & 0x7fffffffffffffffull;
    Fixed r;
    r.n = 0; r.neg = (int)(u >> 63); r.len = 0;
    if (a >= 0x426d1a94a2000000ull) return r;                // |x| >= 1e12 (bit patterns of non-negative doubles are ordered), inf, NaN
    const unsigned ex = (unsigned)(a >> 52);
    const uint64_t frac = a & 0xfffffffffffffull;
    const uint64_t m = ex ? frac | (1ull << 52) : frac;
    const int s = 1069 - (int)(ex ? ex : 1u);                 // -(e + 6), e = max(ex, 1) - 1075: 7 .. 1068
    const uint64_t lo = m * 15625ull, hi = mulhi64(m, 15625ull);      // hi < 8
    uint64_t n;
    bool above, tie;
    if (s < 64) {
        n = (lo >> s) | (hi << (64 - s));
        const uint64_t rem = lo & ((1ull << s) - 1), half = 1ull << (s - 1);
        above = rem > half; tie = rem == half;
    } else if (s == 64) {
        n = hi;
        above = lo > (1ull << 63); tie = lo == (1ull << 63);
    } else if (s < 128) {
        const int t = s - 64;                                 // 1 .. 63
        n = hi >> t;
        const uint64_t rem = hi & ((1ull << t) - 1), half = 1ull << (t - 1);
        above = rem > half || (rem == half && lo != 0); tie = rem == half && lo == 0;
    } else {
        n = 0; above = false; tie = false;                    // P < 2^67 is below half of 2^s
    }
    n += (above || (tie && (n & 1))) ? 1 : 0;
    r.n = n;
    r.len = r.neg + int_digits(n / 1000000ull) + 7;
    return r;
}

// the token of an admitted value at out[0 .. f.len): digits from the last to the first
FMT_F6_HD inline void put(const Fixed f, unsigned char* out) {
    const uint64_t ip = f.n / 1000000ull;
    uint32_t fr = (uint32_t)(f.n - ip * 1000000ull);
    unsigned char* p = out + f.len;
    for (int i = 0; i < 6; ++i) { *--p = (unsigned char)('0' + fr % 10u); fr /= 10u; }
    *--p = '.';
    const uint32_t top = (uint32_t)(ip / 1000000000ull);      // < 1000
    uint32_t low = (uint32_t)(ip - (uint64_t)top * 1000000000ull);
    if (top == 0) {
        do { *--p = (unsigned char)('0' + low % 10u); low /= 10u; } while (low);
    } else {
        for (int i = 0; i < 9; ++i) { *--p = (unsigned char)('0' + low % 10u); low /= 10u; }
        uint32_t t = top;
        do { *--p = (unsigned char)('0' + t % 10u); t /= 10u; } while (t);
    }
    if (f.neg) *--p = '-';
}

// host and tests: the token of x at out (room for MAX_TOKEN bytes), its length, 0 = refused and nothing written
FMT_F6_HD inline int format(double x, unsigned char* out) {
    const Fixed f = to_fixed(x);
    if (f.len) put(f, out);
    return f.len;
}

}  // namespace fmt_f6
