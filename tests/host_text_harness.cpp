// Test-only host build of gps_optimize_slam_amd/csrc/gsf_text.hpp (the TUM text routine gsf_text.hip runs on the device), compiled
// with g++ by tests/test_tum_text_host.py and compared with Python's '%.{p}f' byte for byte.
#include <cstdint>
#include "../gps_optimize_slam_amd/csrc/gsf_text.hpp"

extern "C" {

// '%.{p}f' % x[i] into out[i * stride ...]; lens[i] = its bytes, or -1 for a finite |x| >= 2^63 (left to the host writer)
void ht_fixed(const double* x, int64_t n, int p, char* out, int64_t stride, int64_t* lens)
{
    for (int64_t i = 0; i < n; ++i) {
        const gsf::FixedField f = gsf::fixed_decompose(x[i], p);
        if (f.kind == gsf::FIX_RANGE) { lens[i] = -1; continue; }
        gsf::fixed_write(f, p, out + i * stride);
        lens[i] = f.len;
    }
}

// rows (n, 8): lens[i] = tum_row_len (or -1 when the row holds a finite |x| >= 2^63)
void ht_row_lens(int format, const double* rows, int64_t n, int64_t* lens)
{
    for (int64_t i = 0; i < n; ++i) {
        gsf::FixedField f[gsf::TUM_COLS];
        bool big = false;
        const int len = gsf::tum_row_len(format, rows + i * 8, f, big);
        lens[i] = big ? -1 : len;
    }
}

// header + rows as np.savetxt writes them into out (sized from ht_row_lens); returns the bytes written
int64_t ht_rows_text(int format, const double* rows, int64_t n, char* out)
{
    const char* h = gsf::tum_header(format);
    int64_t o = 0;
    for (int k = 0; k < gsf::tum_header_len(format); ++k) out[o++] = h[k];
    for (int64_t i = 0; i < n; ++i) {
        gsf::FixedField f[gsf::TUM_COLS];
        bool big = false;
        const int len = gsf::tum_row_len(format, rows + i * 8, f, big);
        gsf::tum_row_write(format, f, out + o);
        o += len;
    }
    return o;
}

}  // extern "C"
