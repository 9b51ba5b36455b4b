// Test-only host build of gps_optimize_slam_amd/csrc/gsf_wave_route.hpp (which build of the wave-level EKF kernels runs for a call),
// compiled with g++ by tests/test_wave_route_host.py and compared with a Python restatement.
#include <cstdint>
#include "../gps_optimize_slam_amd/csrc/gsf_wave_route.hpp"

extern "C" {

int hr_early_chunks() { return GSF_EARLY_CHUNKS; }
int hr_tail_full() { return gsf::WAVE_TAIL_FULL; }
// the family codes in the order ONE, DUO, EARLY, BIG, BLOCK
void hr_families(int32_t* f)
{
    f[0] = gsf::WAVE_ONE; f[1] = gsf::WAVE_DUO; f[2] = gsf::WAVE_EARLY; f[3] = gsf::WAVE_BIG; f[4] = gsf::WAVE_BLOCK;
}

// n calls, nine int64 each: block_kernel, duo_kernel, early_variances, tail_scan_stages, pipeline, xy, ragged, B, N
// -> four int32 each: family, tail, nch, pv_stride
void hr_route(const int64_t* in, int64_t n, int32_t* out)
{
    for (int64_t i = 0; i < n; ++i) {
        const int64_t* v = in + 9 * i;
        const gsf::WaveRoute r = gsf::wave_route(gsf::WaveRouteIn{ (int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0, v[5] != 0, v[6] != 0, v[7], v[8] });
        out[4 * i] = r.family; out[4 * i + 1] = r.tail; out[4 * i + 2] = r.nch; out[4 * i + 3] = r.pv_stride;
    }
}

// the noise-layout predicate on (P0[3], Q[3], R[3]) of the position axes
int hr_xy(const double* P0, const double* Q, const double* R)
{
    gsf::EkfConfig k{};
    for (int i = 0; i < 3; ++i) { k.P0[i] = P0[i]; k.Qps[i] = Q[i]; k.Rm[i] = R[i]; }
    return gsf::wave_xy_layout(k) ? 1 : 0;
}

}  // extern "C"
