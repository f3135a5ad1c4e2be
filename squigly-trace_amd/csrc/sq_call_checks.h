// sq_call_checks.h — host code only: what the entry points of all three libraries check the same way before they touch the device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sq_error.h"

// A HIP runtime call whose failure is the entry point's: sets the message and returns 1.  (Expands where it is used: the file that
// uses it includes the HIP runtime.)
#define SQ_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return sq_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
// A device buffer as an entry point was given it.  p = NULL: not given, and it overlaps nothing.
struct NamedRange { const char* name; const void* p; size_t bytes; };
// The check every entry point makes of its device buffers: no two of r may overlap.  twins = pairs of indices (i < j) that may share
// memory when they start at the same address; note = what the message says behind "overlap".
static inline int refuse_overlaps(const NamedRange* r, int count, const char* note = "", const int (*twins)[2] = nullptr, int n_twins = 0) {
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j) {
            if (!r[i].p || !r[j].p || !ranges_overlap(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) continue;
            bool allowed = false;
            for (int t = 0; t < n_twins; ++t) allowed = allowed || (twins[t][0] == i && twins[t][1] == j && r[i].p == r[j].p);
            if (!allowed) return sq_set_error("%s and %s overlap%s", r[i].name, r[j].name, note);
        }
    return 0;
}
