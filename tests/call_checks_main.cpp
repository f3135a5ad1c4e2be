// call_checks_main.cpp — the overlap check of csrc/sq_call_checks.h as a stand-alone host program (tests/test_call_checks.py):
//   g++ -std=c++17 -fsanitize=address,undefined tests/call_checks_main.cpp
// Addresses are made up and never dereferenced.  Prints one line per case: the return value and the message.
#include <cstdio>
#include <cstring>

#include "../squigly-trace_amd/csrc/sq_call_checks.h"

static const void* at(uintptr_t a) { return (const void*)a; }

static void say(const char* what, int rc) { std::printf("%s: %d %s\n", what, rc, rc ? sq_error_buffer() : ""); }

int main() {
    // disjoint, and touching end to start
    const NamedRange apart[3] = { { "a", at(0x1000), 0x100 }, { "b", at(0x1100), 0x100 }, { "c", at(0x3000), 1 } };
    say("touching", refuse_overlaps(apart, 3));
    // one byte shared; the first offending pair in index order is the one named
    const NamedRange shared[3] = { { "a", at(0x1000), 0x101 }, { "b", at(0x1100), 0x100 }, { "c", at(0x11ff), 1 } };
    say("one byte", refuse_overlaps(shared, 3));
    const NamedRange inside[2] = { { "big", at(0x1000), 0x1000 }, { "small", at(0x1800), 4 } };
    say("inside", refuse_overlaps(inside, 2));
    // NULL = not given: overlaps nothing, whatever its size says
    const NamedRange absent[3] = { { "a", at(0x1000), 0x100 }, { "none", nullptr, (size_t)-1 }, { "nil", nullptr, 0x2000 } };
    say("null", refuse_overlaps(absent, 3));
    // the denoiser's call: d_out == d_color and d_out_var == d_var may share memory, from the same start only
    const char* note = " (only d_out == d_color and d_out_var == d_var may share memory)";
    const int twins[2][2] = { { 0, 5 }, { 1, 6 } };
    const size_t n = 64;
    NamedRange dn[8] = { { "d_color", at(0x10000), 12 * n }, { "d_var", at(0x20000), 4 * n }, { "d_tri", at(0x30000), 4 * n },
                         { "d_normal", at(0x40000), 12 * n }, { "d_point", at(0x50000), 12 * n }, { "d_out", at(0x10000), 12 * n },
                         { "d_out_var", at(0x20000), 4 * n }, { "d_work", at(0x60000), 64 * n } };
    say("both aliases", refuse_overlaps(dn, 8, note, twins, 2));
    say("aliases not allowed", refuse_overlaps(dn, 8));
    dn[5].p = at(0x10000 + 12);                       // d_out one pixel into d_color
    say("shifted alias", refuse_overlaps(dn, 8, note, twins, 2));
    dn[5].p = at(0x70000); dn[6].p = at(0x10000);     // d_out_var on d_color: same start, but not a pair that may
    say("wrong pair", refuse_overlaps(dn, 8, note, twins, 2));
    dn[6].p = nullptr; dn[1].p = nullptr;             // no variance at all
    say("no variance", refuse_overlaps(dn, 8, note, twins, 2));
    say("pair test", ranges_overlap(at(0x1000), 0, at(0x1000), 0x10) ? 1 : 0);   // an empty range at another's start overlaps nothing
    return 0;
}
