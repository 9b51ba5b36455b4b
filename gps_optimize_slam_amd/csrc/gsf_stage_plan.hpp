// gsf_stage_plan.hpp -- where the arrays of a host-pointer call lie in the staging arena (gsf::Staging, gsf_internal.hpp).  A pure function
// of the declared arrays: nothing from HIP is included, so g++ compiles it as it stands (tests/host_stage_harness.cpp) and the layout is
// checked without a device.  Nothing else computes an offset into the arena.
#pragma once
#include <stddef.h>

namespace gsf {

enum StageKind { STAGE_IN = 0, STAGE_OUT = 1, STAGE_TMP = 2 };

struct StageBlock {
    size_t bytes;
    int kind;        // StageKind
    bool host;       // host-backed: an input that is copied in / an output that is copied back (a caller's array, bytes > 0)
    size_t off;      // <- stage_plan: a multiple of STAGE_ALIGN
};

struct StagePlan {
    size_t in_end;           // end of the last input: [0, in_end) crosses in one H2D copy (0: no inputs)
    size_t d2h_lo, d2h_hi;   // [d2h_lo, d2h_hi) holds every host-backed output and comes back in one D2H copy (equal: none)
    size_t cap;              // end of the last block: the arena must hold this much
};

constexpr size_t STAGE_ALIGN = 256;
constexpr int STAGE_MAX_BLOCKS = 48;   // the ragged whole run declares about forty
// the arrays one call declares, in a table inside the object (no heap on this path)
struct StageTable {
    StageBlock b[STAGE_MAX_BLOCKS];
    int n = 0;
    int add(size_t bytes, int kind, bool host)   // index of the new block, or -1 when the table is full (nothing is written then)
    {
        if (n >= STAGE_MAX_BLOCKS) return -1;
        b[n] = StageBlock{ bytes, kind, host && bytes > 0, 0 };
        return n++;
    }
};

// All inputs first, in the order declared, then the outputs and temporaries in the order declared; every block on a STAGE_ALIGN boundary.
inline StagePlan stage_plan(StageBlock* b, int n)
{
    StagePlan p{ 0, 0, 0, 0 };
    size_t end = 0;
    bool any_out = false;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n; ++i) {
            if ((b[i].kind == STAGE_IN) != (pass == 0)) continue;
            b[i].off = (end + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1);
            end = b[i].off + b[i].bytes;
            if (pass == 0) p.in_end = end;
            else if (b[i].kind == STAGE_OUT && b[i].host) {
                if (!any_out) { any_out = true; p.d2h_lo = b[i].off; }
                p.d2h_hi = end;
            }
        }
    p.cap = end;
    return p;
}

}  // namespace gsf
