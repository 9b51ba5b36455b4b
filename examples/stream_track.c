/* examples/stream_track.c -- a plain C99 consumer of the streaming fusion (include/gsf.h, "streaming fusion"): one track fused in three
 * appends, with the bookkeeping a live consumer does -- keep the rows an append returns, fetch the rows it revised, trust rows below n_final.
 * The stream's entries take device pointers, so the program owns its device memory through three calls of the HIP runtime (link -lamdhip64).
 *
 *   stream_track IN OUT [cap]
 *
 * IN:  int64 N, then ts[N] f64, pos[N*3] f64, quat[N*4] f64 (x y z w), gps[N*3] f64 (NaN = no fix), valid[N] u8, init_pos[3], init_quat[4] f64
 *      -- one track as main_process_gui holds it after its time alignment, and its Sim3-transformed pose 0 (EKFGPSSLAM.py:1005-1008).
 * OUT: pos_out[N*3], quat_out[N*4] f64 = the track as the consumer holds it after the third append; n_total[3], n_final[3],
 *      revised_from[3] i64 and status[3] i32 = what each append reported.  Default CONFIG (:22-71); cap: rows of history (default 256).
 * Exit code 0, or 1 with the library's message on stderr.  tests/test_stream_c_consumer.py builds it with gcc and compares with one whole-track fuse.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gsf.h"

static int fail(const char *what)
{
    char msg[512];
    gsf_last_error(msg, (int)sizeof msg);
    fprintf(stderr, "stream_track: %s: %s\n", what, msg);
    return 1;
}

/* The three HIP runtime calls a binding needs to own device memory (libamdhip64; hip/hip_runtime_api.h declares them, with enums where this
   file says int).  Synchronous copies; kind 1 = host to device, 2 = device to host. */
extern int hipMalloc(void **ptr, size_t bytes);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);

static int hipfail(const char *what)
{
    fprintf(stderr, "stream_track: %s failed\n", what);
    return 1;
}

static void *dalloc(size_t bytes)
{
    void *p = NULL;
    if (hipMalloc(&p, bytes ? bytes : 8) || !p) { fprintf(stderr, "stream_track: hipMalloc failed\n"); exit(1); }
    return p;
}

static void *upload(const void *host, size_t bytes)
{
    void *p = dalloc(bytes);
    if (bytes && hipMemcpy(p, host, bytes, 1)) { fprintf(stderr, "stream_track: hipMemcpy failed\n"); exit(1); }
    return p;
}

static void *xread(FILE *f, size_t bytes)
{
    void *p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "stream_track: short input\n"); exit(2); }
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: stream_track IN OUT [cap]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t N;
    if (fread(&N, sizeof N, 1, f) != 1 || N < 0) { fprintf(stderr, "stream_track: bad header\n"); return 2; }
    const size_t P = (size_t)N;
    double *ts = xread(f, P * 8), *pos = xread(f, P * 24), *quat = xread(f, P * 32), *gps = xread(f, P * 24);
    uint8_t *valid = xread(f, P);
    double *init_pos = xread(f, 24), *init_quat = xread(f, 32);
    fclose(f);
    const int64_t cap = argc > 3 ? atoll(argv[3]) : 256;

    gsf_ekf_config cfg;                                    /* EKFGPSSLAM.py:24-29, :68-69 */
    memset(&cfg, 0, sizeof cfg);
    {
        const double p0[7] = { 0.1, 0.1, 0.1, 0.01, 0.01, 0.01, 0.01 }, q[7] = { 0.1, 0.1, 0.7, 0.01, 0.01, 0.01, 0.01 }, r[3] = { 0.2, 0.2, 0.2 };
        memcpy(cfg.initial_cov_diag, p0, sizeof p0); memcpy(cfg.process_noise_diag, q, sizeof q); memcpy(cfg.meas_noise_diag, r, sizeof r);
        cfg.sharp_turn_yaw_rate_threshold_deg_per_sec = 45.0;
        cfg.default_ekf_transition_steps_on_sharp_turn = 0;
    }
    if (gsf_device_count() < 1) { fprintf(stderr, "stream_track: no HIP device (there is no CPU fallback)\n"); return 1; }
    gsf_ctx *ctx = NULL;
    if (gsf_create(0, &ctx)) return fail("gsf_create");
    if (cap < 1) { fprintf(stderr, "stream_track: cap must be at least 1\n"); return 2; }

    /* the whole stream lives in device buffers this program owns: two opaque state arrays and the history ring; beside them the track
       (uploaded once here; a live consumer uploads each segment as it arrives), the outputs and the marks of a call */
    double *d_sf = dalloc(GSF_STREAM_F64 * 8), *d_rt = dalloc((size_t)cap * 8), *d_rp = dalloc((size_t)cap * 24), *d_rq = dalloc((size_t)cap * 32);
    int64_t *d_si = dalloc(GSF_STREAM_I64 * 8), *d_marks = dalloc(6 * 8);         /* seg[2], n_total, n_final, revised_from, (gather) lo */
    int32_t *d_status = dalloc(8);
    double *d_ts = upload(ts, P * 8), *d_pos = upload(pos, P * 24), *d_quat = upload(quat, P * 32), *d_gps = upload(gps, P * 24);
    uint8_t *d_valid = upload(valid, P);
    double *d_ip = upload(init_pos, 24), *d_iq = upload(init_quat, 32), *d_po = dalloc(P * 24), *d_qo = dalloc(P * 32);
    double *po = malloc(P * 24 + 8), *qo = malloc(P * 32 + 8);
    if (!po || !qo) { fprintf(stderr, "stream_track: out of memory\n"); return 2; }
    if (gsf_stream_open_dev(ctx, 1, cap, d_ip, d_iq, NULL, d_sf, d_si)) return fail("gsf_stream_open_dev");

    int64_t n_total[3], n_final[3], revised_from[3];
    int32_t status[3];
    int64_t have = 0;
    for (int k = 0; k < 3; ++k) {
        const int64_t lo = have, hi = k == 2 ? N : (N * (k + 1)) / 3;
        int64_t marks[6] = { 0, 0, 0, 0, 0, 0 };
        marks[1] = hi - lo;                                /* seg_offsets of the one track */
        if (hipMemcpy(d_marks, marks, 16, 1)) return hipfail("hipMemcpy");
        if (gsf_stream_append_dev(ctx, &cfg, 1, cap, d_sf, d_si, d_rt, d_rp, d_rq, d_ts + lo, d_pos + lo * 3, d_quat + lo * 4, d_gps + lo * 3,
                                  d_valid + lo, d_marks, d_po + lo * 3, d_qo + lo * 4, NULL, d_marks + 2, d_marks + 3, d_marks + 4, d_status))
            return fail("gsf_stream_append_dev");
        if (gsf_synchronize(ctx)) return fail("gsf_synchronize");
        if (hipMemcpy(marks, d_marks, sizeof marks, 2) || hipMemcpy(&status[k], d_status, 4, 2)) return hipfail("hipMemcpy");
        n_total[k] = marks[2]; n_final[k] = marks[3]; revised_from[k] = marks[4];
        if (status[k] & GSF_STREAM_FULL) {                 /* the open outage and this segment do not fit the ring: nothing was taken */
            fprintf(stderr, "stream_track: append %d refused (GSF_STREAM_FULL): run with a larger cap than %lld\n", k, (long long)cap);
            return 1;
        }
        if (revised_from[k] < lo) {                        /* an RTS back-pass rewrote rows of an earlier append: fetch them from the ring */
            const int64_t from = revised_from[k];
            marks[0] = 0; marks[1] = lo - from; marks[5] = from;
            if (hipMemcpy(d_marks, marks, sizeof marks, 1)) return hipfail("hipMemcpy");
            if (gsf_stream_gather_dev(ctx, 1, cap, d_si, d_rt, d_rp, d_rq, d_marks + 5, d_marks, NULL, d_po + from * 3, d_qo + from * 4))
                return fail("gsf_stream_gather_dev");
        }
        have = n_total[k];
        printf("append %d: %lld poses held, rows [0, %lld) final, rows from %lld written, status %d\n", k, (long long)n_total[k], (long long)n_final[k],
               (long long)revised_from[k], (int)status[k]);
    }
    if (gsf_synchronize(ctx)) return fail("gsf_synchronize");
    if (hipMemcpy(po, d_po, P * 24, 2) || hipMemcpy(qo, d_qo, P * 32, 2)) return hipfail("hipMemcpy");
    {
        void *all[] = { d_sf, d_rt, d_rp, d_rq, d_si, d_marks, d_status, d_ts, d_pos, d_quat, d_gps, d_valid, d_ip, d_iq, d_po, d_qo };
        for (size_t a = 0; a < sizeof all / sizeof all[0]; ++a) hipFree(all[a]);
    }
    gsf_destroy(ctx);

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(po, 8, P * 3, f); fwrite(qo, 8, P * 4, f);
    fwrite(n_total, 8, 3, f); fwrite(n_final, 8, 3, f); fwrite(revised_from, 8, 3, f); fwrite(status, 4, 3, f);
    fclose(f);
    printf("%s\nstreamed %lld poses in three appends through a ring of %lld rows\n", gsf_version(), (long long)N, (long long)cap);
    free(ts); free(pos); free(quat); free(gps); free(valid); free(init_pos); free(init_quat); free(po); free(qo);
    return 0;
}
