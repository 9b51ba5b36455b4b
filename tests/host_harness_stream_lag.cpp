// TEST-ONLY stand-alone program: compiles gsf_stream_lag_core.hpp (and with it gsf_stream_core.hpp, gsf_ekf_core.hpp, gsf_smooth_core.hpp) with
// g++ and drives a stream of B tracks with a fixed-lag smoother through a list of append calls exactly as gsf_stream_lag.hip does --
// stream_append_track() under LagPark per track, then lag_backpass_track() per track -- while
//   * running the SAME calls through stream_append_track() under the no-op policy on a second state and ring, and counting every byte of the
//     plain outputs, reports, state and ring in which the two differ (the superset claim: must be 0);
//   * mirroring every track's smoothed rows from ring_spos / ring_svar after each call, and counting the times a row below an
//     n_smooth_final reported earlier changed its bits or the count moved back (must be 0);
//   * recording per call and track: n_total, status, smooth_from, n_smooth_final, "the three new rings are byte for byte what they were",
//     the segment's spos_out / svar_out / sflags_out rows, and the mirrored rows [smooth_from, n_total) (final and provisional) as they
//     stand after the call;
//   * writing the mirrored smoothed tracks and the raw bytes of the three rings at the end.
// State and rings start as NaN garbage.  usage: host_harness_stream_lag job.bin result.bin, flat float64 files whose layout
// tests/stream_lag_ref.py writes and reads.  tests/test_stream_lag_host.py builds and runs it, once more under
// -fsanitize=address,undefined.  Exit status 0 and a line "OK ..." when the job ran.  Never shipped, never loaded by the package.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_stream_lag_core.hpp"

using namespace gsf;

static bool read_all(const char* path, std::vector<double>& v)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / 8);
    const size_t got = v.empty() ? 0 : fread(v.data(), 8, v.size(), f);
    fclose(f);
    return got == v.size();
}

static bool same_bits(const double* a, const double* b, size_t n) { return n == 0 || memcmp(a, b, n * 8) == 0; }
template <class T> static bool same_vec(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s job.bin result.bin\n", argv[0]); return 2; }
    std::vector<double> in;
    if (!read_all(argv[1], in) || in.size() < 24) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    size_t at = 0;
    auto take = [&](size_t n) { const double* p = in.data() + at; at += n; return p; };
    const double* hdr = take(6);
    const int64_t B = (int64_t)hdr[0], cap = (int64_t)hdr[1], ncalls = (int64_t)hdr[2], P = (int64_t)hdr[3], lag = (int64_t)hdr[5];
    EkfConfig cfg;
    { const double* c = take(18); for (int i = 0; i < 7; ++i) { cfg.P0[i] = c[i]; cfg.Qps[i] = c[7 + i]; } for (int i = 0; i < 3; ++i) cfg.Rm[i] = c[14 + i]; cfg.yaw_thr_rad = c[17]; }
    cfg.sharp_turn_steps = (int32_t)hdr[4]; cfg._pad = 0;
    if (B < 1 || cap < 1 || ncalls < 0 || P < 0 || lag < 1 || lag > STREAM_LAG_MAX) return 2;
    const size_t need = 24 + (size_t)B * 7 + (size_t)B + 1 + (size_t)P * 12 + (size_t)ncalls * (size_t)B;
    if (in.size() != need) { fprintf(stderr, "job has %zu numbers, expected %zu\n", in.size(), need); return 2; }
    const double* init_pos = take((size_t)B * 3); const double* init_quat = take((size_t)B * 4);
    std::vector<int64_t> off((size_t)B + 1);
    { const double* o = take((size_t)B + 1); for (int64_t b = 0; b <= B; ++b) off[b] = (int64_t)o[b]; }
    const double* ts = take((size_t)P); const double* pos = take((size_t)P * 3); const double* quat = take((size_t)P * 4); const double* gps = take((size_t)P * 3);
    std::vector<uint8_t> valid((size_t)P + 1);
    { const double* v = take((size_t)P); for (int64_t i = 0; i < P; ++i) valid[i] = v[i] != 0.0; }
    const double* calls = take((size_t)ncalls * (size_t)B);

    const double garbage = NAN;
    // the stream with a lag, and the plain stream beside it
    std::vector<double> sf((size_t)B * STREAM_F64, garbage), rt((size_t)B * cap, garbage), rp((size_t)B * cap * 3, garbage), rq((size_t)B * cap * 4, garbage);
    std::vector<int64_t> si((size_t)B * STREAM_I64, (int64_t)0x7ff8dead7ff8deadll);
    std::vector<double> rl((size_t)B * cap * STREAM_LAG_F64, garbage), rs((size_t)B * cap * 3, garbage), rv((size_t)B * cap * 3, garbage);
    for (int64_t b = 0; b < B; ++b) stream_open_track(sf.data(), si.data(), B, b, cap, init_pos, init_quat);
    std::vector<double> sf_p = sf, rt_p = rt, rp_p = rp, rq_p = rq;
    std::vector<int64_t> si_p = si;
    std::vector<int64_t> cursor((size_t)B, 0), reported_final((size_t)B, 0);
    std::vector<std::vector<double>> mirror((size_t)B);                  // rows of 6: spos, svar
    std::vector<double> out;
    long violations = 0, superset_diff = 0, appended = 0;

    for (int64_t c = 0; c < ncalls; ++c) {
        const double* call = calls + c * B;
        const std::vector<double> rl0 = rl, rs0 = rs, rv0 = rv;
        std::vector<int64_t> so((size_t)B + 1, 0);
        for (int64_t b = 0; b < B; ++b) {
            const int64_t m = (int64_t)call[b];
            if (m < 0 || cursor[b] + m > off[b + 1] - off[b]) { fprintf(stderr, "call %ld takes more rows than track %ld has\n", (long)c, (long)b); return 2; }
            so[b + 1] = so[b] + m;
        }
        const size_t T = (size_t)so[B];
        std::vector<double> sts(T + 1), sp(T * 3 + 1), sq(T * 4 + 1), sg(T * 3 + 1);
        std::vector<double> po(T * 3 + 1, 0.0), qo(T * 4 + 1, 0.0), co(T * 7 + 1, 0.0), po_p = po, qo_p = qo, co_p = co;
        std::vector<double> spo(T * 3 + 1, 0.0), svo(T * 3 + 1, 0.0);
        std::vector<uint8_t> sv(T + 1), sfl(T + 1, 0xee);
        for (int64_t b = 0; b < B; ++b)
            for (int64_t j = 0; j < so[b + 1] - so[b]; ++j) {
                const int64_t s = off[b] + cursor[b] + j, d = so[b] + j;
                sts[d] = ts[s]; sv[d] = valid[s];
                for (int k = 0; k < 3; ++k) { sp[d * 3 + k] = pos[s * 3 + k]; sg[d * 3 + k] = gps[s * 3 + k]; }
                for (int k = 0; k < 4; ++k) sq[d * 4 + k] = quat[s * 4 + k];
            }
        const StreamSeg g{ sts.data(), sp.data(), sq.data(), sg.data(), sv.data(), po.data(), qo.data(), co.data() };
        const StreamSeg g_p{ sts.data(), sp.data(), sq.data(), sg.data(), sv.data(), po_p.data(), qo_p.data(), co_p.data() };
        const LagOut lo_{ spo.data(), svo.data(), sfl.data() };
        std::vector<double> rep, rows, tail;
        for (int64_t b = 0; b < B; ++b) {
            const int64_t m = so[b + 1] - so[b];
            const LagPark park{ rl.data() + b * cap * STREAM_LAG_F64, lag };
            const StreamReport r = stream_append_track(cfg, sf.data(), si.data(), B, b, cap, rt.data(), rp.data(), rq.data(), g, so[b], m, park);
            const bool taken = !(r.status & (STREAM_FULL | STREAM_BAD_STATE));
            int64_t from = 0, fin = 0;
            lag_backpass_track(rl.data() + b * cap * STREAM_LAG_F64, rs.data() + b * cap * 3, rv.data() + b * cap * 3, cap, lag,
                               taken ? r.n_total - m : r.n_total, taken ? m : -1, lo_, so[b], m, from, fin);
            // the plain stream: it may take a segment that the lag's capacity rule refuses, so it is fed only what the other took
            if (taken) {
                const StreamReport q = stream_append_track(cfg, sf_p.data(), si_p.data(), B, b, cap, rt_p.data(), rp_p.data(), rq_p.data(), g_p, so[b], m);
                superset_diff += (q.n_total != r.n_total) + (q.n_final != r.n_final) + (q.revised_from != r.revised_from) + (q.status != r.status);
                cursor[b] += m; appended += m;
            }
            if (taken) {                                                 // the consumer of the smoothed rows
                std::vector<double>& mr = mirror[b];
                const int64_t n = r.n_total, n_before = n - m;
                mr.resize((size_t)n * 6, 0.0);
                for (int64_t i = (n - cap > 0 ? n - cap : 0); i < n; ++i) {
                    double row[6];
                    for (int k = 0; k < 3; ++k) { row[k] = rs[(b * cap + i % cap) * 3 + k]; row[3 + k] = rv[(b * cap + i % cap) * 3 + k]; }
                    if (i < n_before && i < reported_final[b] && !same_bits(row, mr.data() + i * 6, 6)) ++violations;
                    if (i >= from || i >= n_before) memcpy(mr.data() + i * 6, row, sizeof row);
                }
                if (fin < reported_final[b] || from != reported_final[b]) ++violations;   // the count never moves back, and a call starts where the last ended
                reported_final[b] = fin;
            }
            bool same = same_bits(rl.data() + b * cap * STREAM_LAG_F64, rl0.data() + b * cap * STREAM_LAG_F64, (size_t)cap * STREAM_LAG_F64) &&
                        same_bits(rs.data() + b * cap * 3, rs0.data() + b * cap * 3, (size_t)cap * 3) && same_bits(rv.data() + b * cap * 3, rv0.data() + b * cap * 3, (size_t)cap * 3);
            const double w[5] = { (double)r.n_total, (double)r.status, (double)from, (double)fin, same ? 1.0 : 0.0 };
            rep.insert(rep.end(), w, w + 5);
            for (int64_t j = 0; j < m; ++j) {
                const int64_t d = so[b] + j;
                for (int k = 0; k < 3; ++k) rows.push_back(spo[d * 3 + k]);
                for (int k = 0; k < 3; ++k) rows.push_back(svo[d * 3 + k]);
                rows.push_back((double)sfl[d]);
            }
            // rows [smooth_from, n_total) as the ring holds them now (a refused track: none)
            const int64_t n_now = taken ? r.n_total : from;
            tail.push_back((double)(n_now - from));
            for (int64_t i = from; i < n_now; ++i) tail.insert(tail.end(), mirror[b].begin() + i * 6, mirror[b].begin() + i * 6 + 6);
        }
        // the superset claim: state, ring and the plain outputs (the rows of the segments that were taken: the plain stream never saw the others)
        superset_diff += !same_vec(sf, sf_p) + !same_vec(si, si_p) + !same_vec(rt, rt_p) + !same_vec(rp, rp_p) + !same_vec(rq, rq_p);
        for (int64_t b = 0; b < B; ++b) {
            const bool taken = !((int64_t)rep[b * 5 + 1] & (STREAM_FULL | STREAM_BAD_STATE));
            if (!taken) continue;
            const int64_t a = so[b], m = so[b + 1] - so[b];
            superset_diff += !same_bits(po.data() + a * 3, po_p.data() + a * 3, (size_t)m * 3) + !same_bits(qo.data() + a * 4, qo_p.data() + a * 4, (size_t)m * 4) +
                             !same_bits(co.data() + a * 7, co_p.data() + a * 7, (size_t)m * 7);
        }
        out.insert(out.end(), rep.begin(), rep.end());
        out.insert(out.end(), rows.begin(), rows.end());
        out.insert(out.end(), tail.begin(), tail.end());
    }
    out.push_back((double)violations);
    out.push_back((double)superset_diff);
    for (int64_t b = 0; b < B; ++b) {
        out.push_back((double)(mirror[b].size() / 6));
        out.insert(out.end(), mirror[b].begin(), mirror[b].end());
    }
    out.insert(out.end(), rl.begin(), rl.end());
    out.insert(out.end(), rs.begin(), rs.end());
    out.insert(out.end(), rv.begin(), rv.end());
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("OK %ld tracks, cap %ld, lag %ld, %ld calls, %ld poses appended, %ld finality violations, %ld superset differences\n", (long)B, (long)cap, (long)lag,
           (long)ncalls, appended, violations, superset_diff);
    return 0;
}
