// TEST-ONLY stand-alone program: compiles gsf_stream_core.hpp (and with it gsf_ekf_core.hpp) with g++ and drives a stream of B tracks through
// a list of calls exactly as gsf_stream.hip does -- stream_open_track() per (re-)opened track, stream_append_track() per track of an append --
// while playing the consumer the contract is written for: it mirrors every track's rows from the ring after each call and records
//   * per call and track: n_total, n_final, revised_from, status, the smallest index below the call's first new pose whose bits changed
//     (-1: none) and whether the track's state and ring bytes are the same as before the call;
//   * the rows of every segment (pos, quat, cov) as the call left them;
//   * the number of times a row below an n_final reported earlier changed its bits (must be 0);
//   * the mirrored tracks at the end.
// State and ring start as NaN garbage.  usage: host_harness_stream job.bin result.bin, both flat float64 files whose layout
// tests/stream_ref.py writes and reads.  tests/test_stream_host.py builds and runs it, once more under -fsanitize=address,undefined.
// Exit status 0 and a line "OK ..." when the job ran.  Never shipped, never loaded by the package.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_stream_core.hpp"

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

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s job.bin result.bin\n", argv[0]); return 2; }
    std::vector<double> in;
    if (!read_all(argv[1], in) || in.size() < 23) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    size_t at = 0;
    auto take = [&](size_t n) { const double* p = in.data() + at; at += n; return p; };
    const double* hdr = take(5);
    const int64_t B = (int64_t)hdr[0], cap = (int64_t)hdr[1], ncalls = (int64_t)hdr[2], P = (int64_t)hdr[3];
    EkfConfig cfg;
    { const double* c = take(18); for (int i = 0; i < 7; ++i) { cfg.P0[i] = c[i]; cfg.Qps[i] = c[7 + i]; } for (int i = 0; i < 3; ++i) cfg.Rm[i] = c[14 + i]; cfg.yaw_thr_rad = c[17]; }
    cfg.sharp_turn_steps = (int32_t)hdr[4]; cfg._pad = 0;
    if (B < 1 || cap < 1 || ncalls < 0 || P < 0) return 2;
    const size_t need = 23 + (size_t)B * 7 + (size_t)B + 1 + (size_t)P * 12 + (size_t)ncalls * (1 + (size_t)B);
    if (in.size() != need) { fprintf(stderr, "job has %zu numbers, expected %zu\n", in.size(), need); return 2; }
    const double* init_pos = take((size_t)B * 3); const double* init_quat = take((size_t)B * 4);
    std::vector<int64_t> off((size_t)B + 1);
    { const double* o = take((size_t)B + 1); for (int64_t b = 0; b <= B; ++b) off[b] = (int64_t)o[b]; }
    const double* ts = take((size_t)P); const double* pos = take((size_t)P * 3); const double* quat = take((size_t)P * 4); const double* gps = take((size_t)P * 3);
    std::vector<uint8_t> valid((size_t)P + 1);
    { const double* v = take((size_t)P); for (int64_t i = 0; i < P; ++i) valid[i] = v[i] != 0.0; }
    const double* calls = take((size_t)ncalls * (1 + (size_t)B));

    const double garbage = NAN;
    std::vector<double> sf((size_t)B * STREAM_F64, garbage), rt((size_t)B * cap, garbage), rp((size_t)B * cap * 3, garbage), rq((size_t)B * cap * 4, garbage);
    std::vector<int64_t> si((size_t)B * STREAM_I64, (int64_t)0x7ff8dead7ff8deadll);
    std::vector<int64_t> cursor((size_t)B, 0), reported_final((size_t)B, 0);
    std::vector<std::vector<double>> mirror((size_t)B);                  // rows of 8: t, pos, quat
    std::vector<double> out;
    long violations = 0, appended = 0;

    for (int64_t c = 0; c < ncalls; ++c) {
        const double* call = calls + c * (1 + B);
        const int type = (int)call[0];
        const std::vector<double> sf0 = sf, rt0 = rt, rp0 = rp, rq0 = rq;
        const std::vector<int64_t> si0 = si;
        std::vector<double> rep((size_t)B * 6, -1.0), rows;
        if (type == 1) {                                                 // re-open the marked tracks
            for (int64_t b = 0; b < B; ++b)
                if (call[1 + b] != 0.0) { stream_open_track(sf.data(), si.data(), B, b, cap, init_pos, init_quat); cursor[b] = 0; reported_final[b] = 0; mirror[b].clear(); }
        } else if (type == 2) {                                          // a state of another layout version
            for (int64_t b = 0; b < B; ++b)
                if (call[1 + b] != 0.0) si[SI_VERSION * B + b] = 99;
        } else {
            // the segment arrays of this call: each track's next rows, packed
            std::vector<int64_t> so((size_t)B + 1, 0);
            for (int64_t b = 0; b < B; ++b) {
                int64_t m = (int64_t)call[1 + b];
                if (cursor[b] + m > off[b + 1] - off[b]) { fprintf(stderr, "call %ld takes more rows than track %ld has\n", (long)c, (long)b); return 2; }
                so[b + 1] = so[b] + m;
            }
            const size_t T = (size_t)so[B];
            std::vector<double> sts(T + 1), sp(T * 3 + 1), sq(T * 4 + 1), sg(T * 3 + 1), po(T * 3 + 1, 0.0), qo(T * 4 + 1, 0.0), co(T * 7 + 1, 0.0);
            std::vector<uint8_t> sv(T + 1);
            for (int64_t b = 0; b < B; ++b)
                for (int64_t j = 0; j < so[b + 1] - so[b]; ++j) {
                    const int64_t s = off[b] + cursor[b] + j, d = so[b] + j;
                    sts[d] = ts[s]; sv[d] = valid[s];
                    for (int k = 0; k < 3; ++k) { sp[d * 3 + k] = pos[s * 3 + k]; sg[d * 3 + k] = gps[s * 3 + k]; }
                    for (int k = 0; k < 4; ++k) sq[d * 4 + k] = quat[s * 4 + k];
                }
            const StreamSeg g{ sts.data(), sp.data(), sq.data(), sg.data(), sv.data(), po.data(), qo.data(), co.data() };
            for (int64_t b = 0; b < B; ++b) {
                const int64_t m = so[b + 1] - so[b];
                const int64_t n_before = si0[SI_VERSION * B + b] == STREAM_LAYOUT_VERSION ? si0[SI_NTOTAL * B + b] : 0;
                const StreamReport r = stream_append_track(cfg, sf.data(), si.data(), B, b, cap, rt.data(), rp.data(), rq.data(), g, so[b], m);
                double* w = rep.data() + b * 6;
                w[0] = (double)r.n_total; w[1] = (double)r.n_final; w[2] = (double)r.revised_from; w[3] = (double)r.status;
                const bool taken = !(r.status & (STREAM_FULL | STREAM_BAD_STATE));
                if (taken) { cursor[b] += m; appended += m; }
                // the consumer: mirror what the ring holds, note what changed below the first new pose
                int64_t min_changed = -1;
                if (taken) {
                    std::vector<double>& mr = mirror[b];
                    const int64_t n = r.n_total;
                    mr.resize((size_t)n * 8, 0.0);
                    for (int64_t i = (n - cap > 0 ? n - cap : 0); i < n; ++i) {
                        double t; Vec3 p; Quat q;
                        stream_gather_row(rt.data() + b * cap, rp.data() + b * cap * 3, rq.data() + b * cap * 4, cap, n, i, t, p, q);
                        const double row[8] = { t, p.x, p.y, p.z, q.x, q.y, q.z, q.w };
                        if (i < n_before && !same_bits(row, mr.data() + i * 8, 8)) {
                            if (min_changed < 0) min_changed = i;
                            if (i < reported_final[b]) ++violations;
                        }
                        memcpy(mr.data() + i * 8, row, sizeof row);
                    }
                    if (r.n_final < reported_final[b]) ++violations;     // n_final never moves back
                    reported_final[b] = r.n_final;
                }
                w[4] = (double)min_changed;
                for (int64_t j = 0; j < m; ++j) {
                    const int64_t d = so[b] + j;
                    for (int k = 0; k < 3; ++k) rows.push_back(po[d * 3 + k]);
                    for (int k = 0; k < 4; ++k) rows.push_back(qo[d * 4 + k]);
                    for (int k = 0; k < 7; ++k) rows.push_back(co[d * 7 + k]);
                }
            }
        }
        for (int64_t b = 0; b < B; ++b) {                                // state and ring bytes of the track as before the call?
            bool same = same_bits(rt.data() + b * cap, rt0.data() + b * cap, (size_t)cap) && same_bits(rp.data() + b * cap * 3, rp0.data() + b * cap * 3, (size_t)cap * 3) &&
                        same_bits(rq.data() + b * cap * 4, rq0.data() + b * cap * 4, (size_t)cap * 4);
            for (int k = 0; k < STREAM_F64; ++k) same = same && same_bits(&sf[k * B + b], &sf0[k * B + b], 1);
            for (int k = 0; k < STREAM_I64; ++k) same = same && si[k * B + b] == si0[k * B + b];
            rep[b * 6 + 5] = same ? 1.0 : 0.0;
        }
        out.insert(out.end(), rep.begin(), rep.end());
        out.insert(out.end(), rows.begin(), rows.end());
    }
    out.push_back((double)violations);
    for (int64_t b = 0; b < B; ++b) {
        out.push_back((double)(mirror[b].size() / 8));
        out.insert(out.end(), mirror[b].begin(), mirror[b].end());
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("OK %ld tracks, cap %ld, %ld calls, %ld poses appended, %ld finality violations\n", (long)B, (long)cap, (long)ncalls, appended, violations);
    return 0;
}
