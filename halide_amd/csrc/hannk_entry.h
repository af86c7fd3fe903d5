// hannk_entry.h — what the entry points of apps/hannk's op library share on the host side (hannk_conv.hip, hannk_nn.hip, hannk_program.hip): the lanes-1
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
// check_shape for a buffer whose dimension 0 may have any stride (the generator's dim(0).set_stride(Expr())): the same extents and
// sizes, recorded under the same name, with the stride constraint taken out
inline void check_shape_any_stride0(void *uc, const BufArg &a) {
    halide_dimension_t dims[4];
    halide_buffer_t copy = *a.buf;
    const int nd = std::min(a.buf->dimensions, 4);
    for (int d = 0; d < nd; d++) dims[d] = a.buf->dim[d];
    if (nd > 0) dims[0].stride = 1;
    copy.dim = dims;
    const BufArg b = {a.name, &copy, a.type, a.dims, a.is_output};
    check_shape(uc, b);
}
// the no_bounds_query ops: an unallocated buffer is checked like any other, its type first (check_type_and_dims would take it
// for a query and rewrite the type)
inline int check_unallocated_types(void *uc, const BufArg *args, int n) {
    for (int i = 0; i < n; i++)
        if (!buffer_is_real(args[i].buf) && buf_type_abi(args[i].buf) != args[i].type) {
            char t0[16], t1[16];
            return report(uc, halide_error_code_bad_type, "%s buffer %s has type %s but type of the buffer passed in is %s", args[i].is_output ? "Output" : "Input",
                          args[i].name, type_name(args[i].type, t0), type_name(buf_type_abi(args[i].buf), t1));
        }
    return 0;
}
// ... and after every other check has passed, its missing host pointer ends the call (asserts_host_non_null): before anything is
// allocated for it
inline int check_unallocated_host(void *uc, const BufArg *args, int n) {
    for (int i = 0; i < n; i++)
        if (!buffer_is_real(args[i].buf)) {
            if (int r = checks_done(uc)) return r;
            return report(uc, halide_error_code_host_is_null, "%s buffer %s host pointer is null", args[i].is_output ? "Output" : "Input", args[i].name);
        }
    return 0;
}
inline long elem_offset(const halide_buffer_t *b, int d, long coord) { return (coord - b->dim[d].min) * (long)b->dim[d].stride; }
}  // namespace hannk_entry
}  // namespace hlmi
