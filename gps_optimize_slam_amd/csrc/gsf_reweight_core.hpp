// gsf_reweight_core.hpp -- robust smoothing (gsf_ekf_smooth_reweighted_dev): the rule of one reweighting round, plain host/device C++
// (definitions: include/gsf.h, "robust smoothing").  ekf_smooth_kernel<SMOOTH_REWEIGHTED> (gsf_smooth.hip) calls it per lane;
// tests/host_harness_reweight.cpp compiles it with g++ and compares it with the restatement of tests/reweight_ref.py bit for bit.
//
//  * the residual of a used row against the SMOOTHED track, relative to init_pos: res = (z - init_pos) - (xr + e).  Nothing of UTM size
//    meets anything of residual size in it;
//  * u^2 = sum_c res_c^2 / v_c with the caller's GIVEN variances, three divisions summed left to right;
//  * the weight: Huber w = 1 for u^2 <= c2, else sqrt(c2 / u^2); Cauchy w = 1 / (1 + u^2 / c2).  Both are continuous in u^2;
//  * the effective variance of the next solve, min(v / w, WVAR_MAX): w = 0 (u^2 = inf) gives WVAR_MAX, and v <= v / w, so a usable
//    variance stays usable and no row changes its availability between the solves;
//  * the fixed point: a weight equal BIT FOR BIT to the one its solve used.
// Every statement is one operation or a sum of finished terms: -ffp-contract=on in the kernel's unit finds nothing to fuse here, so the
// device forms what g++ -ffp-contract=off forms (division and square root are correctly rounded on both).
#pragma once
#include "gsf_weighted_core.hpp"

namespace gsf {

enum : int32_t { REWEIGHT_HUBER = 0, REWEIGHT_CAUCHY = 1 };              // GSF_REWEIGHT_* (include/gsf.h)
constexpr int32_t REWEIGHT_MAX_ROUNDS = 32;

// what the entry checks of its three scalars: c2 finite and > 0 (false for NaN), a known loss, 0 <= rounds <= 32
GSF_HD bool reweight_args_ok(const int32_t loss, const double c2, const int32_t rounds)
{
    const bool c2_ok = c2 > 0.0 && c2 < __builtin_huge_val();
    return c2_ok && (loss == REWEIGHT_HUBER || loss == REWEIGHT_CAUCHY) && rounds >= 0 && rounds <= REWEIGHT_MAX_ROUNDS;
}

// one axis of the residual.  zr = z - init_pos (the forward pass's expression), xr = the filtered position relative to init_pos,
// e = the smoother's correction (0 where no later fix reaches the row)
GSF_HD double reweight_residual(const double zr, const double xr, const double e)
{
    const double xs = xr + e;
    return zr - xs;
}

GSF_HD double reweight_u2(const double r0, const double r1, const double r2, const double v0, const double v1, const double v2)
{
    const double s0 = r0 * r0, s1 = r1 * r1, s2 = r2 * r2;
    const double q0 = s0 / v0, q1 = s1 / v1, q2 = s2 / v2;
    const double q01 = q0 + q1;
    return q01 + q2;
}

GSF_HD double reweight_weight(const int32_t loss, const double u2, const double c2)
{
    if (loss == REWEIGHT_CAUCHY) {
        const double t = u2 / c2;
        const double d = 1.0 + t;
        return 1.0 / d;
    }
    const double t = c2 / u2;                                             // (u2 = 0: not taken below)
    const double w = sqrt(t);
    return u2 <= c2 ? 1.0 : w;                                            // a NaN u2 gives NaN
}

// the variance a solve runs with; a quotient that is no number below WVAR_MAX gives WVAR_MAX
GSF_HD double reweight_var(const double v, const double w)
{
    const double q = v / w;
    return q < WVAR_MAX ? q : WVAR_MAX;
}

GSF_HD bool reweight_same_bits(const double a, const double b)
{
    unsigned long long ua, ub;
    __builtin_memcpy(&ua, &a, 8); __builtin_memcpy(&ub, &b, 8);
    return ua == ub;
}

}  // namespace gsf
