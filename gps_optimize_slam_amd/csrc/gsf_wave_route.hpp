// gsf_wave_route.hpp -- which build of the wave-level EKF kernels runs for a call: ONE table, pure host code (no HIP include; compiled with
// g++ into tests/host_route_harness.cpp and checked on the CPU by tests/test_wave_route_host.py).  Five kernel families implement one
// contract and give the same bits, so the choice may depend on the batch size and still a shard of a batch produces the bits of the whole
// batch.  launch_ekf_wave (gsf_ekf_wave.hip) launches what wave_route() says; whoever tunes a bound or adds a build edits this file.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "gsf_ekf_core.hpp"

namespace gsf {
// TAILNS of a kernel instance: the stages the scans of the track's LAST chunk run.  The launcher picks the instance from the track
// length (wave_tail_stages), so the kernel itself carries no test: TAILNS = 6 is the kernel without sized scans, for any length;
// WAVE_TAIL_FULL says that the length is a multiple of 64, i.e. that EVERY chunk is a full one (six stages, no partial chunk at all).
constexpr int WAVE_TAIL_FULL = 7;
GSF_HD int wave_tail_stages(const int64_t N)
{
    if (N <= 0) return 6;
    const int last = (int)((N - 1) & 63);                                 // last active lane of the last chunk
    return last == 63 ? WAVE_TAIL_FULL : (last < 16 ? 4 : (last < 32 ? 5 : 6));
}

// x and y share their (P0, Q, R) and z does not (the default CONFIG): the builds with that choice of scans compiled in (AXMODE 1)
inline bool wave_xy_layout(const EkfConfig& k)
{
    return k.P0[1] == k.P0[0] && k.Qps[1] == k.Qps[0] && k.Rm[1] == k.Rm[0] && !(k.P0[2] == k.P0[0] && k.Qps[2] == k.Qps[0] && k.Rm[2] == k.Rm[0]);
}

// Where the early-variance build is taken without being asked for: 1 000..1 024 tracks of 256..384 poses.  The bounds come from a sweep
// of plain bench runs with the option at 0 and at 1 (HISTORY.md, "Early variances", holds every figure): below 1 000 tracks nothing was
// gained (the launch does not fill the chip and does not end with a wave that gained); at 1 000 tracks lengths below 256 poses gained
// 0.05-0.13 us, at or inside the run-to-run spread; 1 000 and 1 024 tracks gained 0.17-0.55 us over 256..384 poses; 1 536 tracks gained at
// 271 poses but were measured at that length only.  Everything outside the measured wins stays on the one-wave kernel.
#ifndef GSF_EARLY_AUTO_RULE
#define GSF_EARLY_AUTO_RULE(B_, N_) ((B_) >= 1000 && (B_) <= 1024 && (N_) >= 256 && (N_) <= 384)
#endif
// How many chunks' variances the early-variance build forms early (never the last chunk's).  Measured at 1 000 x 271, plain bench, us per
// step: parent 17.38, one chunk 16.94, two 17.65, three 18.86, all five 18.8 (HISTORY.md, "Early variances").
#ifndef GSF_EARLY_CHUNKS
#define GSF_EARLY_CHUNKS 1
#endif

// the families: gsf_ekf_wave.hip (ONE, DUO), gsf_ekf_wave_early.hip (EARLY), gsf_ekf_wave_big.hip (BIG), gsf_ekf_block.hip (BLOCK, opt-in)
enum WaveFamily : int { WAVE_ONE, WAVE_DUO, WAVE_EARLY, WAVE_BIG, WAVE_BLOCK };
struct WaveRouteIn {
    int block_kernel, duo_kernel, early_variances, tail_scan_stages;      // the context's options (gsf_set_option)
    bool pipeline, xy, ragged;   // fused K2+K3+K4 (else K4 alone); wave_xy_layout() of the call's noise; the batch comes with offsets (then N is 0)
    int64_t B, N;
};
struct WaveRoute {
    WaveFamily family;
    bool pipeline, xy;           // as given: with the fields below, the template arguments of the build
    int tail;                    // 4, 5, 6 or WAVE_TAIL_FULL: the TAILNS of ONE, DUO and EARLY
    int nch;                     // chunks of a track, ceil(N / 64): EARLY's build is keyed by it (2..6), BLOCK runs a wave for each
    int pv_stride;               // poses the LDS variance table holds: DUO the whole track (N rounded up to even), EARLY its early chunks; else 0
};

inline WaveRoute wave_route(const WaveRouteIn& in)
{
    const int64_t B = in.B, N = in.N;
    WaveRoute r{ WAVE_ONE, in.pipeline, in.xy, 6, (int)((N + 63) / 64), 0 };
    // the build with sized scans (gsf_set_option "tail_scan_stages"), uniform track length only: a ragged batch has no single last-chunk length
    // (and BIG has no registers for a second instance of the chunk body: it would spill at three waves per SIMD).  Same bits from every build.
    if (in.tail_scan_stages != 0 && !in.ragged) r.tail = wave_tail_stages(N);
    const bool multi = !in.ragged && N > 64;                              // equal lengths, more than one chunk: every build but ONE and BIG needs both
    // Short tracks of the fused pipeline under the default noise layout: the one-wave build that forms the FIRST chunk's variances while
    // the track's rows are still in flight, so that this chunk runs without its Moebius scans (gsf_ekf_wave_early.hip: one round of six
    // chunks).  gsf_set_option "early_variances": -1 automatic, 0 never, 1 always where the build applies (a forced two-wave build goes
    // first; the automatic two-wave range, B <= 256, comes before the automatic rule).
    const bool early_applies = in.pipeline && in.xy && multi && N <= 384 && B <= 2048;
    // Small batches of the fused pipeline: two waves per trajectory (see ekf_wave_duo_kernel).  gsf_set_option "duo_kernel": -1 automatic,
    // 0 never, 1 always.  Measured with the polar-iteration fit (pipeline, N = 271; tools/duo_sweep.py): 15.5 vs 17.8 us at 256 tracks,
    // 19.4 vs 18.9 us at 512, 20.9 vs 19.5 us at 1 000 (every SIMD then holds a main wave and the helper only competes with it)
    // -- automatic = up to 256 tracks.  The four-trajectory-per-block form of round 2 (main and helper of a trajectory forced onto
    // one SIMD) lost its edge with the shorter fit (20.2 vs 19.5 us at 1 000) and lives in tools/experiments/ now.
    const bool duo_applies = in.pipeline && multi && N <= 640, duo_auto = in.duo_kernel == -1 && B <= 256;
    // ---- the precedence, once.  First: tracks of 65..1024 poses, one workgroup per trajectory, one wave per chunk (gsf_ekf_block.hip), only
    // when asked for (gsf_set_option "block_kernel" = 1).  The choice depends on N and the layout only, never on B.
    if (in.block_kernel == 1 && multi && N <= 1024) r.family = WAVE_BLOCK;
    else if (early_applies && in.early_variances == 1 && in.duo_kernel != 1) r.family = WAVE_EARLY;
    else if (duo_applies && (in.duo_kernel == 1 || duo_auto)) r.family = WAVE_DUO;
    else if (early_applies && in.early_variances == -1 && GSF_EARLY_AUTO_RULE(B, N)) r.family = WAVE_EARLY;
    // up to 2 048 waves (two per SIMD) the build with inlined cold blocks costs no occupancy; same arithmetic, same bits
    else if (B > 2048) r.family = WAVE_BIG;
    if (r.family == WAVE_DUO) r.pv_stride = (int)((N + 1) & ~(int64_t)1);
    if (r.family == WAVE_EARLY) r.pv_stride = 64 * (GSF_EARLY_CHUNKS < r.nch - 1 ? GSF_EARLY_CHUNKS : r.nch - 1);   // the kernel's NE chunks
    return r;
}

// EKF noise sweep (gsf_noise_sweep.hip): how many of a call's K candidates one wave takes.  A wave reads its track's chunk once (89 B per
// pose) and runs its candidates one after the other on it, so a larger group means fewer reads of the same rows and a smaller one more
// waves.  The chip has 256 CUs x 4 SIMDs; the kernel's registers leave room for two waves on a SIMD, so 2 048 waves fill it.  Automatic
// (forced == 0): the candidates are split into just enough groups to reach 2 048 waves -- groups = ceil(2048 / B), at most K -- of equal
// size, at most 64 (one lane holds the carry of one candidate).  One track with K = 64: 64 waves of one candidate each; 1 000 tracks with
// K = 64: 3 groups of 22, 22 and 20; 2 048 tracks or more: one group of up to 64.  gsf_set_option "noise_sweep_group" 1..64 forces the
// size.  A candidate's arithmetic does not depend on its group (one code path, a run-time loop), so every choice gives the same bits.
constexpr int64_t SWEEP_FILL_WAVES = 2048;
inline int sweep_group(const int64_t B, const int K, const int forced)
{
    if (K <= 0) return 1;
    int kc;
    if (forced > 0) kc = forced;
    else {
        const int64_t want = B > 0 ? (SWEEP_FILL_WAVES + B - 1) / B : SWEEP_FILL_WAVES;   // groups per track that fill the chip
        const int groups = (int)(want < K ? want : K);
        kc = (K + groups - 1) / groups;
    }
    if (kc > 64) kc = 64;
    if (kc > K) kc = K;
    return kc < 1 ? 1 : kc;
}

// A run-time value as a compile-time one: f(std::integral_constant<int, V>) for the first V of the list that equals v, the LAST one when
// none does.  How the launchers turn a route into template arguments (nested: one lift per argument).
template <int V, int... Vs, class F> inline auto wave_lift(const int v, F&& f)
{
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : wave_lift<Vs...>(v, f);
}
}  // namespace gsf
