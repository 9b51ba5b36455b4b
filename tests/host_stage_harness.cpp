// Test-only host build of gps_optimize_slam_amd/csrc/gsf_stage_plan.hpp (where gsf::Staging puts the arrays of a host-pointer call),
// compiled with g++ by tests/test_stage_plan_host.py and compared with a Python restatement.  With -DHS_MAIN it is a stand-alone
// program that checks the same properties itself (built under -fsanitize=address,undefined by the same test).
#include <cstdint>
#include "../gps_optimize_slam_amd/csrc/gsf_stage_plan.hpp"

extern "C" {

int hs_max_blocks() { return gsf::STAGE_MAX_BLOCKS; }

// n arrays (bytes, kind, host != 0) declared in order, then laid out.  off[0 .. min(n, table)): the offsets; plan[4] = in_end, d2h_lo,
// d2h_hi, cap.  Returns the number of arrays the table refused (0 unless n exceeds it).
int hs_plan(const int64_t* bytes, const int32_t* kind, const uint8_t* host, int n, int64_t* off, int64_t* plan)
{
    gsf::StageTable t;
    int refused = 0;
    for (int i = 0; i < n; ++i)
        if (t.add((size_t)bytes[i], kind[i], host[i] != 0) < 0) ++refused;
    const gsf::StagePlan p = gsf::stage_plan(t.b, t.n);
    for (int i = 0; i < t.n; ++i) off[i] = (int64_t)t.b[i].off;
    plan[0] = (int64_t)p.in_end; plan[1] = (int64_t)p.d2h_lo; plan[2] = (int64_t)p.d2h_hi; plan[3] = (int64_t)p.cap;
    return refused;
}

}  // extern "C"

#ifdef HS_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

static int check(const std::vector<int64_t>& bytes, const std::vector<int32_t>& kind, const std::vector<uint8_t>& host)
{
    const int n = (int)bytes.size(), m = n < gsf::STAGE_MAX_BLOCKS ? n : gsf::STAGE_MAX_BLOCKS;
    std::vector<int64_t> off((size_t)m);                                       // exactly the table's worth: a write past it is caught
    int64_t plan[4];
    if (hs_plan(bytes.data(), kind.data(), host.data(), n, off.data(), plan) != n - m) return 1;
    int64_t end = 0, in_end = 0;
    for (int i = 0; i < m; ++i) {
        if (off[i] % 256) return 2;
        if (off[i] + bytes[i] > end) end = off[i] + bytes[i];
        if (kind[i] == gsf::STAGE_IN && off[i] + bytes[i] > in_end) in_end = off[i] + bytes[i];
        for (int j = 0; j < m; ++j) {
            if (j != i && bytes[i] && bytes[j] && off[i] < off[j] + bytes[j] && off[j] < off[i] + bytes[i]) return 3;
            if (kind[i] == gsf::STAGE_IN && kind[j] != gsf::STAGE_IN && off[i] + bytes[i] > off[j]) return 4;
        }
        if (kind[i] == gsf::STAGE_OUT && host[i] && bytes[i] && (off[i] < plan[1] || off[i] + bytes[i] > plan[2])) return 5;
    }
    if (plan[0] != in_end || plan[3] != end) return 6;
    return 0;
}

int main()
{
    uint64_t s = 88172645463325252ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int it = 0; it < 5000; ++it) {
        const int n = (int)(next() % (unsigned)(gsf::STAGE_MAX_BLOCKS + 3));
        std::vector<int64_t> bytes((size_t)n); std::vector<int32_t> kind((size_t)n); std::vector<uint8_t> host((size_t)n);
        for (int i = 0; i < n; ++i) {
            const uint64_t r = next();
            bytes[(size_t)i] = (r & 7) == 0 ? 0 : (int64_t)((r >> 8) % ((r & 8) ? 5000000 : 700));
            kind[(size_t)i] = (int32_t)((r >> 40) % 3); host[(size_t)i] = (uint8_t)((r >> 48) & 1);
        }
        const int rc = check(bytes, kind, host);
        if (rc) { printf("list %d: property %d fails\n", it, rc); return 1; }
    }
    printf("stage plan: 5000 lists ok\n");
    return 0;
}
#endif
