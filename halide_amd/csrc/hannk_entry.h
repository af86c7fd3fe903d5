// hannk_entry.h — what the entry points of apps/hannk's op library share on the host side (hannk_conv.hip, hannk_nn.hip): the lanes-1
// types of their argument tables and the constraint checks in the reference's words.
#pragma once

#include "hlmi_internal.h"

namespace hlmi {
namespace hannk_entry {

// The tables state every type with lanes = 1 (L), as the reference's metadata does (ConvOp::filter_type hands arguments[2].type to the
// buffer it allocates); a buffer may come with lanes 0 (this library's other callers) or 1 (Halide::Runtime::Buffer): own_lanes().
constexpr uint32_t L1 = 1u << 16;
inline Arg L(Arg a) {
    a.type |= L1;
    return a;
}
template<int N>
void own_lanes(BufArg (&args)[N]) {
    for (BufArg &a : args)
        if (a.buf && (buf_type_abi(a.buf) >> 16) <= 1) a.type = (a.type & 0xffffu) | (buf_type_abi(a.buf) & L1);
}
inline int blocks_ok(void *uc, const char *what, long threads, unsigned *blocks) {
    const long n = (threads + 255) / 256;
    if (n > 0x7fffffffL) return report(uc, halide_error_code_buffer_extents_too_large, "%s: %ld workgroups exceed one launch", what, n);
    *blocks = (unsigned)n;
    return 0;
}

// "<buffer>.stride.<d> is a multiple of m", in the words of the reference's constraint (stride == stride / m * m)
inline void check_stride_multiple(void *uc, const char *buffer, const halide_buffer_t *b, int d, int m) {
    char what[64], expect[96];
    snprintf(what, sizeof what, "%s.stride.%d", buffer, d);
    snprintf(expect, sizeof expect, "%s.stride.%d / %d * %d", buffer, d, m, m);
    const int s = b->dim[d].stride;
    check_equal(uc, what, s, expect, s - ((s % m) + m) % m);   // Halide's division rounds toward -inf
}
inline void check_dim(void *uc, const char *buffer, const halide_buffer_t *b, int d, const int *min, const int *extent, const int *stride) {
    char what[64], expect[32];
    const int *want[3] = {stride, min, extent};
    const int have[3] = {b->dim[d].stride, b->dim[d].min, b->dim[d].extent};
    const char *field[3] = {"stride", "min", "extent"};
    for (int k = 0; k < 3; k++) {
        if (!want[k]) continue;
        snprintf(what, sizeof what, "%s.%s.%d", buffer, field[k], d);
        snprintf(expect, sizeof expect, "%d", *want[k]);
        check_equal(uc, what, have[k], expect, *want[k]);
    }
}
}  // namespace hannk_entry
}  // namespace hlmi
