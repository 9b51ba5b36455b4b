// gsf_text.hpp -- step 7 of main_process_gui as bytes: the TUM rows np.savetxt writes (ref :1091-1092, :1098-1101).
//
// np.savetxt formats every field with Python's '%.{p}f' (p = 3, 6, 8): the EXACT binary value of the double rounded to p decimals,
// ties to even, '-' whenever the sign bit is set (-0.0 and negatives that round to zero print -0.000000), 'nan' for a NaN of either
// sign, 'inf' / '-inf'.  Here every digit is decided on the bit pattern with integer arithmetic only -- no floating-point operation
// rounds anything -- so the g++ build of this header (tests/host_text_harness.cpp) and the gfx950 build (gsf_text.hip) agree by
// construction.  Covered range: finite |x| < 2^63 (every stamp, UTM coordinate, degree and quaternion of a run); a larger finite value
// is reported (FixedField::kind == FIX_RANGE) and its track is left to the host writer.
#pragma once
#include <stdint.h>
#include "gsf_math.hpp"

namespace gsf {

enum { FIX_FINITE = 0, FIX_NAN = 1, FIX_INF = 2, FIX_RANGE = 3 };
enum { TUM_COLS = 8, TUM_MAX_ROW = 8 * 29 + 8 };   // a field is at most '-' + 19 integer digits + '.' + 8 decimals

// x = (-1)^neg (ip + frac / 10^p), frac already rounded
struct FixedField {
    uint64_t ip;
    uint32_t frac;
    int32_t kind;
    int32_t neg;
    int32_t len;     // bytes of the printed field
};

GSF_HD uint32_t pow10_u32(int p)
{
    uint32_t r = 1;
    for (int k = 0; k < p; ++k) r *= 10u;
    return r;
}

GSF_HD uint32_t pow5_u32(int p)
{
    uint32_t r = 1;
    for (int k = 0; k < p; ++k) r *= 5u;
    return r;
}

GSF_HD int decimal_digits(uint64_t v)       // digits of v (1 for 0), v < 10^19
{
    int n = 1;
    uint64_t t = 10;
    while (n < 19 && v >= t) { t *= 10; ++n; }
    return n;
}

// '%.{p}f' % x as (sign, integer part, p-digit fraction), p <= 9
GSF_HD FixedField fixed_decompose(double x, int p)
{
    const uint64_t bits = __builtin_bit_cast(uint64_t, x);
    FixedField f;
    f.ip = 0; f.frac = 0; f.kind = FIX_FINITE; f.neg = (int32_t)(bits >> 63);
    const int be = (int)((bits >> 52) & 0x7ff);
    uint64_t m = bits & ((1ull << 52) - 1);
    if (be == 0x7ff) {
        f.kind = m ? FIX_NAN : FIX_INF;
        f.len = (m ? 3 : 3 + f.neg);
        if (m) f.neg = 0;
        return f;
    }
    int e = -1074;                              // subnormal (or zero): x = m * 2^-1074
    if (be) { m |= 1ull << 52; e = be - 1075; }
    if (e >= 11) {                              // m >= 2^52, so x >= 2^63
        f.kind = FIX_RANGE; f.len = 0;
        return f;
    }
    const uint32_t scale = pow10_u32(p);
    if (e >= 0) {
        f.ip = m << e;
    } else {
        const int k = -e;                       // x = m / 2^k
        f.ip = k < 64 ? m >> k : 0;
        const uint64_t mf = k < 64 ? m & ((1ull << k) - 1) : m;      // fraction = mf / 2^k exactly
        uint32_t q;
        if (k <= p) {                           // frac * 10^p = mf * 5^p * 2^(p-k): an integer, nothing to round
            q = (uint32_t)((mf * pow5_u32(p)) << (p - k));
        } else {
            const int s = k - p;                // frac * 10^p = mf * 5^p / 2^s; mf * 5^p < 2^53 * 5^9 < 2^74
            if (s > 74) {
                q = 0;                          // below half of the last place (and never equal to it)
            } else {
                const unsigned __int128 prod = (unsigned __int128)mf * pow5_u32(p);
                const unsigned __int128 qq = prod >> s;
                const unsigned __int128 r = prod - (qq << s), half = (unsigned __int128)1 << (s - 1);
                q = (uint32_t)qq;
                if (r > half || (r == half && (q & 1u))) ++q;       // ties to even
            }
        }
        if (q >= scale) { q -= scale; ++f.ip; }                     // 9.9999999 -> 10.000000
        f.frac = q;
    }
    f.len = f.neg + decimal_digits(f.ip) + 1 + p;
    return f;
}

// writes the f.len bytes of a FIX_FINITE / FIX_NAN / FIX_INF field
template <typename Out>
GSF_HD void fixed_write(const FixedField& f, int p, Out* dst)
{
    if (f.kind == FIX_NAN) { dst[0] = 'n'; dst[1] = 'a'; dst[2] = 'n'; return; }
    int o = 0;
    if (f.neg) dst[o++] = '-';
    if (f.kind == FIX_INF) { dst[o] = 'i'; dst[o + 1] = 'n'; dst[o + 2] = 'f'; return; }
    const int nd = f.len - f.neg - 1 - p;
    int w = o + nd - 1;
    uint64_t v = f.ip;
    while (v >= (1ull << 32)) { dst[w--] = (Out)('0' + (int)(v % 10u)); v /= 10u; }
    uint32_t v32 = (uint32_t)v;
    do { dst[w--] = (Out)('0' + (int)(v32 % 10u)); v32 /= 10u; } while (v32);
    o += nd;
    dst[o++] = '.';
    uint32_t q = f.frac;
    for (int k = p - 1; k >= 0; --k) { dst[o + k] = (Out)('0' + (int)(q % 10u)); q /= 10u; }
}

// ---- the two TUM formats (GSF_TUM_UTM / GSF_TUM_WGS84 of include/gsf.h)
// UTM   (ref :1091-1092): fmt ['%.6f'] + ['%.6f']*3 + ['%.8f']*4,              header "timestamp x y z qx qy qz qw (UTM)"
// WGS84 (ref :1098-1101): fmt ['%.6f'] + ['%.8f','%.8f','%.3f'] + ['%.8f']*4, header "timestamp lon lat alt qx qy qz qw (WGS84)"
// np.savetxt joins the fields with ' ', ends every row with '\n' and writes comments + header + '\n' first (comments='').
GSF_HD int tum_precision(int format, int c)
{
    return format == 1 ? (c == 0 ? 6 : (c == 3 ? 3 : 8)) : (c < 4 ? 6 : 8);
}

GSF_HD const char* tum_header(int format)
{
    return format == 1 ? "timestamp lon lat alt qx qy qz qw (WGS84)\n" : "timestamp x y z qx qy qz qw (UTM)\n";
}

GSF_HD int tum_header_len(int format) { return format == 1 ? 42 : 34; }

// the fields of row i of (ts[P], xyz[P][3], quat[P][4])
GSF_HD void tum_row_values(const double* ts, const double* xyz, const double* quat, int64_t i, double v[TUM_COLS])
{
    v[0] = ts[i];
    v[1] = xyz[i * 3]; v[2] = xyz[i * 3 + 1]; v[3] = xyz[i * 3 + 2];
    v[4] = quat[i * 4]; v[5] = quat[i * 4 + 1]; v[6] = quat[i * 4 + 2]; v[7] = quat[i * 4 + 3];
}

// THE length routine of both passes: decomposes the row's fields and returns its bytes (7 separators and the newline included);
// out_of_range is set when a field is finite with |x| >= 2^63 (the row's length is then meaningless)
GSF_HD int tum_row_len(int format, const double v[TUM_COLS], FixedField f[TUM_COLS], bool& out_of_range)
{
    int len = TUM_COLS;
#pragma unroll
    for (int c = 0; c < TUM_COLS; ++c) {
        f[c] = fixed_decompose(v[c], tum_precision(format, c));
        out_of_range |= f[c].kind == FIX_RANGE;
        len += f[c].len;
    }
    return len;
}

// writes the row whose fields tum_row_len decomposed
template <typename Out>
GSF_HD void tum_row_write(int format, const FixedField f[TUM_COLS], Out* dst)
{
    int o = 0;
#pragma unroll
    for (int c = 0; c < TUM_COLS; ++c) {
        fixed_write(f[c], tum_precision(format, c), dst + o);
        o += f[c].len;
        dst[o++] = (Out)(c + 1 < TUM_COLS ? ' ' : '\n');
    }
}

}  // namespace gsf
