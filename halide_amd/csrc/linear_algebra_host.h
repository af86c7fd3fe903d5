// linear_algebra_host.h — the host-side checks that linear_algebra.hip (f32) and linear_algebra_f64.hip (f64) share: alignment,
// overlap of byte ranges (by each buffer's own element size), the pinned shapes, derived extents, limits and bounds-query answers.
#pragma once

#include "hlmi_internal.h"

namespace hlmi {
namespace la_host {

inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }
// a matrix whose every column starts on 16 bytes: `per16` elements fill 16 bytes
inline bool aligned16(const void *p, long col_stride, int per16) { return aligned16(p) && col_stride % per16 == 0; }

inline uintptr_t elem_bytes(const halide_buffer_t *b) { return (b->type.bits + 7) / 8; }

// elements from a buffer's first to one past its last, 0 for an empty one (dimension 0 has stride 1)
inline uintptr_t span_elems(const halide_buffer_t *b) {
    uintptr_t n = 1;
    for (int d = 0; d < b->dimensions; d++) {
        if (b->dim[d].extent <= 0) return 0;
        n += (uintptr_t)(b->dim[d].extent - 1) * (uintptr_t)b->dim[d].stride;
    }
    return n;
}

inline bool same_layout(const halide_buffer_t *a, const halide_buffer_t *b) {
    if (a->dimensions != b->dimensions) return false;
    for (int d = 0; d < a->dimensions; d++)
        if (a->dim[d].extent != b->dim[d].extent || a->dim[d].stride != b->dim[d].stride) return false;
    return true;
}

// mat_mul.hip's overlap() for any shape: do the byte ranges of a and b meet, in host or in device memory.  With `exact_ok`, a that IS
// b — the same first element and the same layout, the call every wrapper of halide_blas.h makes — does not count.
inline bool overlap(const halide_buffer_t *a, const halide_buffer_t *b, bool exact_ok) {
    if (a == b) return !exact_ok;
    const uintptr_t na = elem_bytes(a) * span_elems(a), nb = elem_bytes(b) * span_elems(b);
    auto hit = [&](uintptr_t pa, uintptr_t pb) {
        if (!pa || !pb || !na || !nb) return false;
        if (exact_ok && pa == pb && same_layout(a, b)) return false;
        return pa < pb + nb && pb < pa + na;
    };
    return hit((uintptr_t)a->host, (uintptr_t)b->host) || hit((uintptr_t)a->device, (uintptr_t)b->device);
}

// records: min == 0, extent == the named value, and for a matrix a column stride that keeps columns apart
inline void pin(void *uc, const BufArg &a, int d, int extent, const char *extent_name) {
    char what[40], expect[64];
    snprintf(what, sizeof what, "%s.min.%d", a.name, d);
    check_equal(uc, what, a.buf->dim[d].min, "0", 0);
    snprintf(what, sizeof what, "%s.extent.%d", a.name, d);
    check_equal(uc, what, a.buf->dim[d].extent, extent_name, extent);
    if (d == 1) {
        snprintf(what, sizeof what, "%s.stride.1", a.name);
        snprintf(expect, sizeof expect, "max(%s.stride.1, %s.extent.0)", a.name, a.name);
        check_equal(uc, what, a.buf->dim[1].stride, expect, std::max(a.buf->dim[1].stride, a.buf->dim[0].extent));
    }
}

// an extent the call derives its sizes from: the first of `cands` (buffer, dimension) that is real or, in a query, shaped; else 0
struct Cand {
    const halide_buffer_t *b;
    int d;
};
inline int derive(std::initializer_list<Cand> cands) {
    for (const Cand &c : cands)
        if (c.b && buffer_known(c.b)) return c.b->dim[c.d].extent;
    return 0;
}

inline int limit(void *uc, const char *entry, const char *what, int v, int max) {
    if (v >= 0 && v <= max) return 0;
    return report(uc, halide_error_code_constraint_violated, "Constraint violated: %s %s (%d) must be 0 .. %d", entry, what, v, max);
}

inline void answer1(halide_buffer_t *b, int n) {
    const int mins[1] = {0}, ext[1] = {n};
    answer_query(b, mins, ext);
}
inline void answer2(halide_buffer_t *b, int w, int h) {
    const int mins[2] = {0, 0}, ext[2] = {w, h};
    answer_query(b, mins, ext);
}

// null, type, dimensionality; returns 1 for a bounds query (the caller answers it), < 0 for an error
inline int prologue(void *uc, const BufArg *args, int n) {
    int r = check_not_null(uc, args, n);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, n))) return r;
    return any_bounds_query(args, n) ? 1 : 0;
}

}  // namespace la_host
}  // namespace hlmi
