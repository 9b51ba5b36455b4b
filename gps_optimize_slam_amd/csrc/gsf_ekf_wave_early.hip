// gsf_ekf_wave_early.hip -- the fused pipeline's one-wave kernel for SHORT tracks (64 < N <= 384, equal lengths, the default noise layout)
// with the variances of its first chunk(s) computed EARLY: while the input burst of the fit is in flight.
//
// The one-wave kernel (gsf_ekf_wave.hip) asks for the track's rows and then issues nothing until they are back; its chunk loop then runs
// the two Moebius scans of the variance recursion in every chunk.  That recursion depends on the stamps and on which fixes are used --
// nine of the ~70 bytes per pose the burst moves.  This build
//   1. requests the stamps and mask bytes of EVERY chunk first, then chunk after chunk the fix and the SLAM position, then chunk 0's
//      quaternions (vmcnt retires loads in issue order and nothing is stored before the chunk loop: a use of chunk k's registers waits for
//      chunk k alone; the stamps are back ~3 000 cycles ahead of the last column);
//   2. waits for stamps and mask bytes ALONE and takes a set mask byte to mean a usable fix (true of every row the generator, the loaders
//      and time_align_kernel produce; a NaN fix under a set mask byte is the reference's demotion quirk, see 4);
//   3. runs the local scans of the first GSF_EARLY_CHUNKS chunks side by side in one basic block, applies the carried variance chunk after
//      chunk and writes P_f, P_p and the gain of their poses into LDS, in the layout of the two-wave kernel's helper but for the y rows:
//      y repeats x (AXMODE 1), so they are neither written nor read and the chunk loop copies x in registers.  Only what fits the
//      shadow of the burst is done here: a chunk's scans are ~1 400-1 700 cycles of issue, and every cycle past the arrival of the rows
//      delays the fit by as much as the chunk loop gains (all chunks early: +1.3 us; HISTORY.md, "Early variances");
//  2b. chooses the rows of the fit (the reference's rule, ref :973-998) from the same stamps and mask bytes, still in the shadow: the
//      per-lane compares here, the wave-uniform decisions in gsf_rows_rule.hpp (first gap, V[:k], duration limit, both fall-backs as
//      decisions on popcounts -- no second pass).  One lane mask per chunk comes out, the count, the row flag, and dep_end: the rows whose
//      validity the choice depends on;
//   4. sums the fit's moments chunk by chunk AS THE CHUNKS ARRIVE, under those masks, and forms each chunk's exact validity mask from its
//      fix.  Under the reference's rule a chunk in front of dep_end whose exact mask is not the assumed one (a NaN under a set byte;
//      wave-uniform, rare) drops the sums: the one-wave kernel's pass, fit_moments_reference_rows, runs unchanged on the held rows.  Chunks
//      behind dep_end (behind the gap's row of a track that fits its first segment) are not waited for.  Under "every valid row" nothing is
//      assumed or chosen: the exact masks, then one block of sums, as in the one-wave kernel's pass.  The closed form (fit_from_partials) is the one-wave kernel's.  A miss in
//      an early chunk forms that part of the table again from memory, with the NaN test, wave-uniformly;
//   5. runs wave_serial_chunks<PIPELINE, PREVAR = true, ..., PVCHUNKS, REGCHUNKS = NCH>: the first chunks read the table as the two-wave
//      kernel's main wave does, the chunks behind them run their scans as the one-wave kernel does.  The kernel's type carries the number of
//      chunks, so the chunks are NCH straight-line instances of the ONE chunk body (c0 = 64 k a constant, L = 63 but for the last chunk: the
//      lane masks built from them fold), and chunk k + 1 takes its stamp, mask byte, SLAM position and fix from the registers of 1, not
//      from memory again (12 loads and the address arithmetic of five arrays per chunk).  Only the quaternion
//      of chunk k + 1 is requested in chunk k (four loads, one address); the last chunk requests nothing.  The registers hold what memory
//      holds: nothing writes them after 2 (the fall-back pass of 4 reads them), and the idle lanes of a short last chunk hold the last row
//      by il[] of 1, which is load_chunk's clamp.  The carried-outage patch reads stamps from memory and the LDS ring as before.
// No load may stay pending on a rare path of 2b or 4: where paths meet the wave would wait for it with vmcnt(0), i.e. for the whole burst.
// Single stamps and the shift of a track whose first valid row is not row 0 therefore come out of the registers (v_readlane), not from memory.
// One wave per block: no barrier, no wait on another wave; a wave's LDS operations complete in order.
// Same functions on the same operands in the same order as the one-wave kernel -- the guarantee the two-wave build gives -- so every
// output byte is the same.  The builds are OVERLOADS of ekf_wave_kernel<PIPELINE, SMALLBATCH, AXMODE> (the build travels in the
// argument's type, as WaveArgsTail does), keyed by the number of chunks and by the sizing of the last chunk's scans.
// The table holds the early chunks only: 9 x 64 x GSF_EARLY_CHUNKS x 8 bytes of dynamic LDS, 4.5 KB for one chunk.
#include "gsf_wave_common.hpp"
#include "gsf_rows_rule.hpp"

using namespace gsf;

namespace {

static_assert(GSF_ROWS_ROUND == 6, "the early-variance build hands the fit passes ONE round of six chunks");

// (GSF_EARLY_CHUNKS, how many chunks' variances are formed early: gsf_wave_route.hpp, with the bounds of this build)
template <int NCH, int TAILNS> struct WaveArgsEarly { WaveArgs a; int pv_stride; };

template <bool PIPELINE, int AXMODE, int NCH, int TAILNS>
__device__ __forceinline__ void wave_early_body(const WaveArgs& a, const EkfConfig& cfg, const int pv_stride, const int64_t b, const int lane)
{
    static_assert(PIPELINE && AXMODE == 1 && NCH >= 2 && NCH <= 6, "fused pipeline, x and y share their noise, two to six chunks");
    constexpr int NE = GSF_EARLY_CHUNKS < NCH - 1 ? GSF_EARLY_CHUNKS : NCH - 1;   // chunks whose variances are formed early: full ones, never the last
    extern __shared__ double gsf_pv[];
    GSF_STAMP(0);
    const int64_t N = a.N, base = b * N;                                  // equal lengths: 64 (NCH - 1) < N <= 64 NCH (the launcher's choice of build)
    int Ni = (int)N;
    asm volatile("" : "+s"(Ni));
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;

    // ---- 1. the whole track is ONE round of the fit's row pass: requested here, in the order in which it is needed
    int stride = pv_stride; double cPx = cfg.P0[0], cPz = cfg.P0[2];      // (fetched here, with the other kernel arguments: see 3)
    asm volatile("" : "+s"(stride), "+s"(cPx), "+s"(cPz));
    int rows_mode = a.rows.mode, rows_ms = a.rows.min_samples; double rows_gap = a.rows.max_gap, rows_dur = a.rows.max_dur;   // (the row rule's, for 2b)
    asm volatile("" : "+s"(rows_mode), "+s"(rows_ms), "+s"(rows_gap), "+s"(rows_dur));
    RoundRows<6> rr;
    int il[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) { const int i = 64 * k + lane; il[k] = (k < NCH - 1 || i < Ni) ? i : Ni - 1; }
    uint8_t vb[NCH];                                                      // (widened below the last request: the conversion is a use, and a use waits)
#pragma unroll
    for (int k = 0; k < NCH; ++k) { rr.pt[k] = tsb[il[k]]; vb[k] = valb[il[k]]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {                                       // chunk after chunk: the fix, then the SLAM position (a use of chunk k waits for chunk k alone)
        rr.pz[k][0] = gpsb[il[k] * 3]; rr.pz[k][1] = gpsb[il[k] * 3 + 1]; rr.pz[k][2] = gpsb[il[k] * 3 + 2];
        rr.pa[k][0] = posb[il[k] * 3]; rr.pa[k][1] = posb[il[k] * 3 + 1]; rr.pa[k][2] = posb[il[k] * 3 + 2];
        __builtin_amdgcn_sched_barrier(0);
    }
    // chunk 0 of the chunk loop: its stamp, position, fix and mask byte ARE the round's first chunk; only the quaternion is its own
    ChunkIn nxt;
    nxt.q = Quat{ __builtin_nontemporal_load(&quatb[il[0] * 4]), __builtin_nontemporal_load(&quatb[il[0] * 4 + 1]),
                  __builtin_nontemporal_load(&quatb[il[0] * 4 + 2]), __builtin_nontemporal_load(&quatb[il[0] * 4 + 3]) };
#pragma unroll
    for (int k = NCH; k < 6; ++k) {                                       // (chunks past the end of the track, as the passes' own loads leave them)
        rr.pa[k][0] = rr.pa[k][1] = rr.pa[k][2] = 0.0; rr.pz[k][0] = rr.pz[k][1] = rr.pz[k][2] = 0.0; rr.pt[k] = 0.0; rr.pv[k] = 0u;
    }
    __builtin_amdgcn_sched_barrier(0);                                   // ... and stay requested HERE: nothing below is scheduled above them

    // ---- 2. stamps and mask bytes have arrived (the columns behind them are still in flight)
    // (each byte has ONE use, its widening, which then folds into the load; and the widened value is opaque from here on.  Left transparent, the
    // compiler compared the raw byte in one place and widened it in another, the widening became an instruction right behind the byte's load,
    // and the wave waited for that load before it had requested the other columns.)
#pragma unroll
    for (int k = 0; k < NCH; ++k) { uint32_t w = vb[k]; asm volatile("" : "+v"(w) :: "memory"); rr.pv[k] = w; }
#pragma unroll
    for (int k = 0; k < NCH; ++k) asm volatile("" :: "v"(rr.pt[k]) : "memory");
    GSF_STAMP(14);                                                       // stamps and mask bytes have arrived
    double dt[NE]; bool stepping[NE], spec[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {                                        // (full chunks, all of them: NE < NCH)
        stepping[k] = (64 * k + lane) != 0;
        const double c_t = (k == 0) ? lane_bcast(rr.pt[0], 0) : lane_bcast(rr.pt[k - 1], 63);
        dt[k] = fmax(1e-6, rr.pt[k] - prev_lane(c_t, rr.pt[k]));         // ref :865
        spec[k] = stepping[k] && rr.pv[k] != 0u;                          // the fix is taken to be usable (ref :867-869 without the NaN test)
    }

    // ---- 3. the local scans of the first NE chunks, side by side (2 NE independent chains; a lone wave issues a DPP-move + FMA chain every
    // 7.4 cycles alone and every 4.5 with four chains beside it, tools/ubench/ilp.hip); then the carry, chunk after chunk; the table goes to LDS.
    // (The constants of the block are fetched in front of it and pinned: left alone, the register allocator re-fetched them from the kernel
    // arguments in front of every scan, a dozen scalar-cache round trips with nothing to cover them.)
    double qx = cfg.Qps[0], rx = cfg.Rm[0], qz = cfg.Qps[2], rz = cfg.Rm[2];
    asm volatile("" : "+s"(qx), "+s"(rx), "+s"(qz), "+s"(rz));
    Moebius mx[NE], mz[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        mx[k] = variance_scan<6>(qx, rx, dt[k], stepping[k], spec[k]);
        mz[k] = variance_scan<6>(qz, rz, dt[k], stepping[k], spec[k]);
    }
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int i = 64 * k + lane;
        const AxisVar vx = variance_finish(mx[k], qx, rx, dt[k], cPx);
        const AxisVar vz = variance_finish(mz[k], qz, rz, dt[k], cPz);
        gsf_pv[0 * stride + i] = vx.Pf; gsf_pv[1 * stride + i] = vx.Pm; gsf_pv[2 * stride + i] = vx.kg;
        gsf_pv[6 * stride + i] = vz.Pf; gsf_pv[7 * stride + i] = vz.Pm; gsf_pv[8 * stride + i] = vz.kg;
        cPx = lane_bcast(vx.Pf, 63); cPz = lane_bcast(vz.Pf, 63);
    }
    __builtin_amdgcn_sched_barrier(0);
    GSF_STAMP(13);                                                       // variance table written (the timing tools run five-chunk tracks: 13 is free there)

    // ---- 2b. the row choice (ref :973-998) from stamps and mask bytes, under the assumption of 2: which rows the fit sums, as one lane mask
    // per chunk, before a row has been summed -- the fall-backs of the rule are decisions on popcounts (gsf_rows_rule.hpp), not second passes
    u64 av[6];                                                            // rows of the track whose mask byte is set
#pragma unroll
    for (int k = 0; k < 6; ++k) av[k] = k < NCH ? (mask_first(Ni - 64 * k) & mask_nonzero(rr.pv[k])) : 0ull;
    int k0, l0;
    const bool anyv = rows_first_valid<6>(av, k0, l0), first0 = (av[0] & 1ull) != 0ull;   // (the usual track: its very first row is valid)
    const int i0 = anyv ? 64 * k0 + l0 : 0;
    RowsChoice<6> ch;
    if (rows_mode != 0) {                                                 // wave-uniform
        // single stamps come out of the registers that hold them (the row is wave-uniform: a v_readlane), never from memory: a load on this
        // path would make the wave wait for the whole burst (vmcnt retires in order), and for a round trip of its own on top
        const auto stamp_at = [&](const int i) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < NCH; ++k) if ((i >> 6) == k) t = lane_bcast(rr.pt[k], i & 63);
            return t;
        };
        double tfirst = lane_bcast(rr.pt[0], 0);
        if (!first0) { asm volatile("" ::: "memory"); tfirst = stamp_at(i0); }   // (a real branch, not if-conversion)
        const double max_gap = rows_gap, tlim = tfirst + rows_dur;   // segment_start_time + max_dur (:989-990)
        u64 graw[6], le[6]; double tb = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (k < NCH) {
                const double tp = prev_lane(tb, rr.pt[k]);                // stamp of row i - 1
                tb = lane_bcast(rr.pt[k], 63);
                graw[k] = mask_gt(rr.pt[k] - tp, max_gap); le[k] = mask_le(rr.pt[k], tlim);
            } else { graw[k] = 0ull; le[k] = 0ull; }
        }
        rows_rule_choose<6>(av, graw, le, Ni, rows_ms, max_gap, stamp_at, ch);
    } else {                                                              // every valid row: nothing to choose
        ch.nT = 0; ch.rows_flag = 0; ch.row_end = Ni; ch.nF = 0; ch.dep_end = Ni;
#pragma unroll
        for (int k = 0; k < 6; ++k) { ch.mo[k] = av[k]; ch.nT += __popcll(av[k]); }
    }
    GSF_STAMP(15);                                                       // the rows of the fit are chosen

    // ---- 4. the fit: chunk k is summed when chunk k is back (vmcnt retires loads in the order of 1).  Its fix gives its exact validity mask.
    // Every valid row (rows mode 0): those masks ARE the rows summed, nothing was assumed (one block, see there).  The reference's rule: the chunk is summed
    // under the mask of 2b; where the exact mask differs from the assumed one in a chunk the choice depends on, the sums are dropped and the
    // one-wave kernel's pass runs on the held rows, unchanged.  Rows behind dep_end -- behind the gap's row, when the fit takes the first
    // segment -- cannot change the choice (gsf_rows_rule.hpp) and are not waited for: a NaN there is the chunk loop's business alone.
    // Same expressions, same order of additions over the chunks, same shifts, the count from the same popcounts as those passes: same bits.
    nxt.t = rr.pt[0]; nxt.v = rr.pv[0];
    Vec3 p0; Quat q0; int32_t fit = 0;
    rr.nearly = NE;
    u64 miss = 0ull;                                                     // rows of the early chunks on which the assumption of 2 does not hold
    double sums[17], bs_[3]; int32_t rows_flag = ch.rows_flag;
    const double as0 = lane_bcast(rr.pa[0][0], 0), as1 = lane_bcast(rr.pa[0][1], 0), as2 = lane_bcast(rr.pa[0][2], 0);   // pose 0 sits in lane 0
    double Sa0 = 0, Sa1 = 0, Sa2 = 0, Sb0 = 0, Sb1 = 0, Sb2 = 0, Saa = 0;
    double Sab[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    double bs0 = lane_bcast(rr.pz[0][0], 0), bs1 = lane_bcast(rr.pz[0][1], 0), bs2 = lane_bcast(rr.pz[0][2], 0);
    int nsum = 0; u64 bad = 0ull;
#define GSF_EARLY_SUM(k_, o_)                                                                                                                      \
    {                                                                                                                                              \
        const double a0 = o_ ? rr.pa[k_][0] - as0 : 0.0, a1 = o_ ? rr.pa[k_][1] - as1 : 0.0, a2 = o_ ? rr.pa[k_][2] - as2 : 0.0;                  \
        const double b0 = o_ ? rr.pz[k_][0] - bs0 : 0.0, b1 = o_ ? rr.pz[k_][1] - bs1 : 0.0, b2 = o_ ? rr.pz[k_][2] - bs2 : 0.0;                  \
        Sa0 += a0; Sa1 += a1; Sa2 += a2; Sb0 += b0; Sb1 += b1; Sb2 += b2;                                                                        \
        Saa += a0 * a0 + a1 * a1 + a2 * a2;                                                                                                       \
        Sab[0] += a0 * b0; Sab[1] += a0 * b1; Sab[2] += a0 * b2;                                                                                  \
        Sab[3] += a1 * b0; Sab[4] += a1 * b1; Sab[5] += a1 * b2;                                                                                  \
        Sab[6] += a2 * b0; Sab[7] += a2 * b1; Sab[8] += a2 * b2;                                                                                  \
    }
    if (rows_mode != 0) {
        if (!first0) {                                                    // the first valid row is not row 0: the GNSS-side shift (:988)
            asm volatile("" ::: "memory");                               // (a real branch, not if-conversion)
            bs0 = bs1 = bs2 = 0.0;
#pragma unroll
            for (int k = 0; k < NCH; ++k)                                 // (from the registers that hold the row: its chunk alone is waited for)
                if (anyv && (i0 >> 6) == k) { bs0 = lane_bcast(rr.pz[k][0], i0 & 63); bs1 = lane_bcast(rr.pz[k][1], i0 & 63); bs2 = lane_bcast(rr.pz[k][2], i0 & 63); }
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (k < NE || 64 * k < ch.dep_end) {                          // wave-uniform
                const u64 exk = av[k] & mask_not_nan(rr.pz[k][0]) & mask_not_nan(rr.pz[k][1]) & mask_not_nan(rr.pz[k][2]);
                bad |= av[k] & ~exk;
                if (k < NE) miss |= av[k] & ~exk & ~(k == 0 ? 1ull : 0ull);
                if (k == NCH - 1) GSF_STAMP(1);                           // the last chunk's fix has arrived
            }
            nsum += __popcll(ch.mo[k]);
            if (ch.mo[k] != 0ull) {                                       // wave-uniform (a track with a gap sums its first segment only)
                const bool o = __builtin_amdgcn_inverse_ballot_w64(ch.mo[k]);
                GSF_EARLY_SUM(k, o)
            }
        }
    } else {
        // every valid row: nothing was assumed and nothing is chosen -- the exact masks of all chunks, then one straight block of sums, as the
        // one-wave kernel's pass has it.  (Summed chunk by chunk as the rule's path does, this mode measured 0.16-0.3 us SLOWER than the
        // parent: HISTORY.md, "Early rows".)
        u64 mok[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            mok[k] = av[k] & mask_not_nan(rr.pz[k][0]) & mask_not_nan(rr.pz[k][1]) & mask_not_nan(rr.pz[k][2]);
            if (k < NE) miss |= av[k] & ~mok[k] & ~(k == 0 ? 1ull : 0ull);
        }
        GSF_STAMP(1);                                                     // the rows have arrived
        if ((mok[0] & 1ull) == 0ull) {                                    // the first valid row is not row 0
            asm volatile("" ::: "memory");                               // (a real branch, not if-conversion)
            u64 ex[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) ex[k] = k < NCH ? mok[k] : 0ull;
            int ke, le_;
            const bool have = rows_first_valid<6>(ex, ke, le_);
            bs0 = bs1 = bs2 = 0.0;
#pragma unroll
            for (int k = 0; k < NCH; ++k)
                if (have && ke == k) { bs0 = lane_bcast(rr.pz[k][0], le_); bs1 = lane_bcast(rr.pz[k][1], le_); bs2 = lane_bcast(rr.pz[k][2], le_); }
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const bool o = __builtin_amdgcn_inverse_ballot_w64(mok[k]);
            nsum += __popcll(mok[k]);
            GSF_EARLY_SUM(k, o)
        }
    }
#undef GSF_EARLY_SUM
    sums[0] = (double)nsum;                                               // (wave-uniform: the count of the rows summed, from the masks)
    sums[1] = Sa0; sums[2] = Sa1; sums[3] = Sa2; sums[4] = Sb0; sums[5] = Sb1; sums[6] = Sb2; sums[7] = Saa;
#pragma unroll
    for (int k = 0; k < 9; ++k) sums[8 + k] = Sab[k];
    bs_[0] = bs0; bs_[1] = bs1; bs_[2] = bs2;
    if (bad != 0ull) {
        // a NaN fix under a set mask byte where the choice looks (wave-uniform, rare): the one-wave kernel's pass, unchanged, on the held rows
        asm volatile("" ::: "memory");                                   // (a real branch, not if-conversion)
        fit_moments_reference_rows<6, true>(a, b, base, N, lane, as0, as1, as2, sums, bs_, rows_flag, &rr, &miss);
    }
    GSF_STAMP(2);
    nxt.p = Vec3{ rr.pa[0][0], rr.pa[0][1], rr.pa[0][2] };
    nxt.z = Vec3{ rr.pz[0][0], rr.pz[0][1], rr.pz[0][2] };
    {
        const double as_[3] = { as0, as1, as2 };
        const Quat qraw0 = lane_bcast(nxt.q, 0);                          // pose 0's quaternion as stored: requested last, used after the closed form
        if (!fit_from_partials(a, b, base, N, lane, sums, as_, bs_, qraw0, p0, q0, fit, rows_flag, true)) return;   // (fit None, bad pose-0 quaternion: the table is never read)
    }
    if (miss != 0ull) {
        // a NaN fix under a set mask byte in the first NE chunks (wave-uniform, rare): their part of the table again, from memory, with the
        // NaN test -- the flags, the dt and the variance_chunk() of the chunk loop, as the two-wave kernel's helper forms them
        asm volatile("" ::: "memory");                                   // (a real branch, not if-conversion)
        double cP0 = cfg.P0[0], cP1 = cfg.P0[1], cP2 = cfg.P0[2], c_t = tsb[0];
#pragma nounroll
        for (int k = 0; k < NE; ++k) {
            const int i = 64 * k + lane;                                  // (full chunks: every lane holds a pose of the track)
            const double t = tsb[i], z0 = gpsb[i * 3], z1 = gpsb[i * 3 + 1], z2 = gpsb[i * 3 + 2];
            const bool step = i != 0, avail = step && valb[i] != 0 && !(isnan(z0) || isnan(z1) || isnan(z2));   // ref :867-869
            const double dtk = fmax(1e-6, t - prev_lane(c_t, t));       // ref :865
            AxisVar v0, v1, v2;
            variance_chunk<6>(cfg, 0, -1, dtk, step, avail, cP0, cP1, cP2, v0, v1, v2);   // (AXMODE 1: y repeats x, z has its own scan)
            gsf_pv[0 * stride + i] = v0.Pf; gsf_pv[1 * stride + i] = v0.Pm; gsf_pv[2 * stride + i] = v0.kg;
            gsf_pv[6 * stride + i] = v2.Pf; gsf_pv[7 * stride + i] = v2.Pm; gsf_pv[8 * stride + i] = v2.kg;
            cP0 = lane_bcast(v0.Pf, 63); cP1 = lane_bcast(v1.Pf, 63); cP2 = lane_bcast(v2.Pf, 63); c_t = lane_bcast(t, 63);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    // one wave per block: its LDS operations complete in order, no barrier
    GSF_STAMP(6);

    // ---- 5. the chunk loop: its first NE chunks as the two-wave kernel's main wave runs them, the rest as the one-wave kernel does
    wave_serial_chunks<PIPELINE, true, true, 1, AXMODE, TAILNS, NE, NCH>(a, cfg, b, lane, base, N, p0, q0, fit, nxt, gsf_pv, stride, 0, nullptr, &rr);
}

#define GSF_WAVE_EARLY_KERNEL(C_, T_)                                                                                                 \
    template <bool PIPELINE, bool SMALLBATCH, int AXMODE>                                                                             \
    __global__ __launch_bounds__(64, 1) void ekf_wave_kernel(WaveArgsEarly<C_, T_> w, EkfConfig cfg)                                  \
    {                                                                                                                                 \
        static_assert(SMALLBATCH, "a small-batch build");                                                                             \
        wave_early_body<PIPELINE, AXMODE, C_, T_>(w.a, cfg, w.pv_stride, (int64_t)blockIdx.x, (int)threadIdx.x);                      \
    }
#define GSF_WAVE_EARLY_KERNELS(C_) GSF_WAVE_EARLY_KERNEL(C_, 4) GSF_WAVE_EARLY_KERNEL(C_, 5) GSF_WAVE_EARLY_KERNEL(C_, 6) GSF_WAVE_EARLY_KERNEL(C_, WAVE_TAIL_FULL)
GSF_WAVE_EARLY_KERNELS(2)
GSF_WAVE_EARLY_KERNELS(3)
GSF_WAVE_EARLY_KERNELS(4)
GSF_WAVE_EARLY_KERNELS(5)
GSF_WAVE_EARLY_KERNELS(6)
#undef GSF_WAVE_EARLY_KERNELS
#undef GSF_WAVE_EARLY_KERNEL

}  // namespace

namespace gsf {

// fused pipeline, x and y sharing their noise and z not, equal lengths, 64 < N <= 384: wave_route()'s EARLY, taken as it comes
int launch_ekf_wave_early(gsf_ctx* ctx, const WaveRoute& r, const WaveArgs& a, const EkfConfig& k)
{
    GSF_REQUIRE(a.B > 0 && a.B <= 0x7fffffff, "B out of range for one launch");
    WaveArgs e = a; e.init_pos = nullptr; e.init_quat = nullptr;           // the fit gives the initial pose
    const size_t lds = (size_t)r.pv_stride * 9 * sizeof(double);
    wave_lift<2, 3, 4, 5, 6>(r.nch, [&](auto c) { wave_lift<4, 5, WAVE_TAIL_FULL, 6>(r.tail, [&](auto tl) {
        hipLaunchKernelGGL((ekf_wave_kernel<true, true, 1>), dim3((unsigned)a.B), dim3(64), lds, ctx->stream,
                           WaveArgsEarly<decltype(c)::value, decltype(tl)::value>{ e, r.pv_stride }, k); }); });
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

const char* wave_early_build_info() { return GSF_TU_BUILD_INFO("gsf_ekf_wave_early.hip"); }

}  // namespace gsf
