// hannk_move.hip — the data movement apps/hannk's interpreter does in plain C++ rather than through a generator (interpreter/ops.cpp):
//   hlmi_hannk_copy_from   Halide::Runtime::Buffer::copy_from on two buffers of any strides: TRANSPOSE, SPACE_TO_DEPTH / DEPTH_TO_SPACE,
//                          the copying half of CONCATENATION and SPLIT are this one call on re-viewed buffers
//   hlmi_hannk_gather      GatherOp::execute with batch_dims == 0 as one launch
// Library extensions in C linkage: no argument table, no _argv, no _metadata.
//
// copy_from, host side: intersect the two boxes, drop extent-1 dimensions, turn negative dst strides round, sort by dst stride, merge what
// is contiguous on both sides; then the plan (move_plan below, hlmi_debug_hannk_move_plan) picks one of
//   hannk_cf_rows        dimension 0 has stride 1 on both sides and is at least 16 bytes long: 16 bytes per lane where both addresses and
//                        the row's end allow, element by element in every other lane
//   hannk_cf_transpose   dimension 0 has stride 1 in dst, another dimension has stride 1 in src, both at least TR_MIN long, elements of 2, 4 or
//                        8 bytes: a tile goes through LDS, loaded along src's stride-1 dimension and stored along dst's.  1-byte elements
//                        go to the general kernel: at 1024 x 1024 the tile measured 8.3 us against its 8.0 (2 bytes: 8.5 against 8.9,
//                        4 bytes: 8.7 against 9.6)
//   hannk_cf_general     one thread per element, consecutive lanes along dst's innermost dimension; what hlmi_hannk_general forces
// The LDS tile of hannk_cf_transpose is tile[TILE][TILE + PAD] elements; a wave writes one row (consecutive addresses) and reads one
// column, a stride of (TILE + PAD) * sizeof(T) bytes between lanes: 2 bytes 64 + 2 (33 dwords), 4 bytes 64 + 1 (65 dwords): odd dword
// strides, the 32 lanes of a group on 32 different banks; 8 bytes 32 + 1 (66 dwords): ds_read_b64 banks over 64, lane l on banks 2 l
// and 2 l + 1.  scripts/model/lds_banks.py on these addresses: tests/test_hannk_move.py.
#include "hannk_entry.h"

namespace hlmi {
namespace {
using namespace hannk_entry;

constexpr int MOVE_MAX_RANK = 8;
constexpr int TR_MIN = 16;   // below this many elements along either tile edge most of a tile's lanes idle: the general kernel
enum { MOVE_EMPTY = 0, MOVE_ROWS = 1, MOVE_TRANSPOSE = 2, MOVE_GENERAL = 3 };

struct CopyGeom {
    const uint8_t *src;   // the element of the box's first corner, on either side
    uint8_t *dst;
    int n;                // dimensions after merging (at least 1)
    int e[MOVE_MAX_RANK];
    long ss[MOVE_MAX_RANK], ds[MOVE_MAX_RANK];   // in elements
};

template<typename T>
__global__ __launch_bounds__(256) void hannk_cf_general(CopyGeom g, long total) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    long so = 0, dof = 0;
#pragma unroll
    for (int d = 0; d < MOVE_MAX_RANK; d++) {
        if (d < g.n) {
            const long c = i % g.e[d];
            i /= g.e[d];
            so += c * g.ss[d], dof += c * g.ds[d];
        }
    }
    reinterpret_cast<T *>(g.dst)[dof] = reinterpret_cast<const T *>(g.src)[so];
}

// a lane: 16 bytes of one row (dimension 0, stride 1 on both sides)
template<typename T>
__global__ __launch_bounds__(256) void hannk_cf_rows(CopyGeom g, long row_bytes, long total) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long nch = (row_bytes + 15) / 16;
    const long b0 = (i % nch) * 16;
    i /= nch;
    long so = 0, dof = 0;
#pragma unroll
    for (int d = 1; d < MOVE_MAX_RANK; d++) {
        if (d < g.n) {
            const long c = i % g.e[d];
            i /= g.e[d];
            so += c * g.ss[d], dof += c * g.ds[d];
        }
    }
    const uint8_t *pi = g.src + so * (long)sizeof(T) + b0;
    uint8_t *po = g.dst + dof * (long)sizeof(T) + b0;
    const int n = (int)min(16L, row_bytes - b0);
    if (n == 16 && (((uintptr_t)pi | (uintptr_t)po) & 15) == 0) {
        *reinterpret_cast<uint4 *>(po) = *reinterpret_cast<const uint4 *>(pi);
    } else {
        for (int k = 0; k < n / (int)sizeof(T); k++) reinterpret_cast<T *>(po)[k] = reinterpret_cast<const T *>(pi)[k];
    }
}

// dimension 0 = a (dst stride 1), dimension 1 = b (src stride 1); a workgroup: one TILE x TILE tile of one (a, b) plane
template<typename T, int TILE, int PAD>
__global__ __launch_bounds__(256) void hannk_cf_transpose(CopyGeom g, int tiles_a, int tiles_b) {
    __shared__ T tile[TILE][TILE + PAD];
    constexpr int ROWS = 256 / TILE;
    long blk = blockIdx.x;
    const int a0 = (int)(blk % tiles_a) * TILE;
    blk /= tiles_a;
    const int b0 = (int)(blk % tiles_b) * TILE;
    blk /= tiles_b;
    long so = 0, dof = 0;
#pragma unroll
    for (int d = 2; d < MOVE_MAX_RANK; d++) {
        if (d < g.n) {
            const long c = blk % g.e[d];
            blk /= g.e[d];
            so += c * g.ss[d], dof += c * g.ds[d];
        }
    }
    const T *ps = reinterpret_cast<const T *>(g.src) + so;
    T *pd = reinterpret_cast<T *>(g.dst) + dof;
    const int tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
    for (int j = ty; j < TILE; j += ROWS) {   // lanes along b
        const int a = a0 + j, b = b0 + tx;
        if (a < g.e[0] && b < g.e[1]) tile[j][tx] = ps[a * g.ss[0] + b];
    }
    __syncthreads();
    for (int j = ty; j < TILE; j += ROWS) {   // lanes along a
        const int a = a0 + tx, b = b0 + j;
        if (a < g.e[0] && b < g.e[1]) pd[b * g.ds[1] + a] = tile[tx][j];
    }
}

// ---------------------------------------------------------------------------------------------------------------- gather
struct GatherGeom {
    const uint8_t *src;
    const int32_t *idx;
    uint8_t *dst;
    int *flag;              // set to 1 by a lane whose index lies outside the source
    int n;                  // dst's rank
    int axis, k;            // dst dimensions axis .. axis + k - 1 are the position in `indices`
    int e[MOVE_MAX_RANK];   // dst's extents
    long ds[MOVE_MAX_RANK];
    long ss[MOVE_MAX_RANK]; // the source's stride for the dst dimension (not read for the k index dimensions)
    long is[2];             // strides of `indices`
    int axis_min, axis_extent;
    long axis_stride;       // of the source's dimension `axis`
};
template<typename T>
__global__ __launch_bounds__(256) void hannk_gather_kernel(GatherGeom g, long total) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    long so = 0, dof = 0, io = 0;
#pragma unroll
    for (int d = 0; d < MOVE_MAX_RANK; d++) {
        if (d < g.n) {
            const long c = i % g.e[d];
            i /= g.e[d];
            dof += c * g.ds[d];
            if (d >= g.axis && d < g.axis + g.k) io += c * g.is[d - g.axis];
            else so += c * g.ss[d];
        }
    }
    const long at = (long)g.idx[io] - g.axis_min;
    if (at < 0 || at >= g.axis_extent) {   // nothing of this slice is written
        atomicOr(g.flag, 1);
        return;
    }
    reinterpret_cast<T *>(g.dst)[dof] = reinterpret_cast<const T *>(g.src)[so + at * g.axis_stride];
}

// ---------------------------------------------------------------------------------------------------------------- host: the plan
struct MovePlan {
    int kernel;   // MOVE_*
    int rank;     // dimensions left after dropping and merging (0: one element)
    int b;        // MOVE_TRANSPOSE: the dimension with src stride 1 (moved to position 1 in g)
    long total;   // elements
    long soff, doff;   // the box's first corner, in elements from each buffer's first element
    CopyGeom g;
};
// 0, or -8 when distinct indices of dst alias through a stride of 0: the one overlap that is looked for.  Any other self-overlap of dst
// (strides (1, 1), a row stride below the row's extent) passes, and the lanes that share an element race: the caller's error, as with
// Buffer::copy_from itself.
int move_plan(const halide_buffer_t *src, const halide_buffer_t *dst, int es, bool general, MovePlan &p) {
    p = MovePlan{};
    CopyGeom &g = p.g;
    int n = 0;
    p.total = 1;
    bool empty = false;
    for (int d = 0; d < dst->dimensions; d++) {
        const halide_dimension_t &s = src->dim[d], &t = dst->dim[d];
        const long lo = std::max(s.min, t.min), hi = std::min((long)s.min + s.extent, (long)t.min + t.extent);
        if (hi <= lo) {
            empty = true;
            continue;
        }
        p.soff += (lo - s.min) * (long)s.stride, p.doff += (lo - t.min) * (long)t.stride;
        if (hi - lo == 1) continue;
        if (t.stride == 0) return -8;
        g.e[n] = (int)(hi - lo), g.ss[n] = s.stride, g.ds[n] = t.stride;
        if (g.ds[n] < 0) {   // walk the dimension from its other end: every dst stride positive
            p.soff += (g.e[n] - 1) * g.ss[n], p.doff += (g.e[n] - 1) * g.ds[n];
            g.ss[n] = -g.ss[n], g.ds[n] = -g.ds[n];
        }
        p.total *= g.e[n];
        n++;
    }
    if (empty) {
        p.kernel = MOVE_EMPTY, p.total = 0;
        return 0;
    }
    for (int i = 1; i < n; i++)   // by dst stride, then by src stride
        for (int j = i; j > 0 && (g.ds[j] < g.ds[j - 1] || (g.ds[j] == g.ds[j - 1] && g.ss[j] < g.ss[j - 1])); j--) {
            std::swap(g.e[j], g.e[j - 1]), std::swap(g.ss[j], g.ss[j - 1]), std::swap(g.ds[j], g.ds[j - 1]);
        }
    int m = 0;
    for (int d = 1; d < n; d++) {
        const long ext = (long)g.e[m] * g.e[d];
        if (g.ds[d] == g.ds[m] * g.e[m] && g.ss[d] == g.ss[m] * g.e[m] && ext < (1L << 31)) {
            g.e[m] = (int)ext;
        } else {
            m++;
            g.e[m] = g.e[d], g.ss[m] = g.ss[d], g.ds[m] = g.ds[d];
        }
    }
    p.rank = n == 0 ? 0 : m + 1;
    if (n == 0) g.e[0] = 1, g.ss[0] = 1, g.ds[0] = 1;
    g.n = std::max(p.rank, 1);
    p.kernel = MOVE_GENERAL;
    if (general || p.rank == 0 || g.ds[0] != 1) return 0;
    if (g.ss[0] == 1) {
        if ((long)g.e[0] * es >= 16) p.kernel = MOVE_ROWS;
        return 0;
    }
    if (es < 2 || g.e[0] < TR_MIN) return 0;   // 1-byte tiles did not beat the general kernel (above)
    for (int d = 1; d < g.n; d++)
        if (g.ss[d] == 1 && g.e[d] >= TR_MIN) {
            p.kernel = MOVE_TRANSPOSE, p.b = d;
            for (int j = d; j > 1; j--) std::swap(g.e[j], g.e[j - 1]), std::swap(g.ss[j], g.ss[j - 1]), std::swap(g.ds[j], g.ds[j - 1]);
            break;
        }
    return 0;
}

int elem_size(const halide_buffer_t *b) { return (int)((buf_type_abi(b) >> 8) & 0xffu) / 8 * std::max<int>(buf_type_abi(b) >> 16, 1); }
bool size_ok(int es) { return es == 1 || es == 2 || es == 4 || es == 8; }

// null -12, element size -3, rank -43: the order and codes of the generated entry points
int move_protocol(void *uc, const BufArg *args, int n, const char *what) {
    if (int r = check_not_null(uc, args, n)) return r;
    const int es = elem_size(args[0].buf);
    if (!size_ok(es)) return report(uc, halide_error_code_bad_type, "%s: elements of %d bytes are not supported", what, es);
    const halide_buffer_t *out = args[n - 1].buf;
    if (elem_size(out) != es)
        return report(uc, halide_error_code_bad_type, "%s: %s has elements of %d bytes but %s has elements of %d bytes", what, args[n - 1].name,
                      elem_size(out), args[0].name, es);
    return 0;
}
int check_aligned(void *uc, const char *what, const BufArg &a, int es) {
    if (a.buf->device % es) return report(uc, halide_error_code_constraint_violated, "%s: %s is not aligned to its element size", what, a.name);
    return 0;
}
// every offset of a buffer stays inside 2^31 elements, as check_shape asks of the generated entry points' buffers
int check_span(void *uc, const char *what, const BufArg &a) {
    long span = 0;
    for (int d = 0; d < a.buf->dimensions; d++) {
        const halide_dimension_t &t = a.buf->dim[d];
        if (t.extent < 0) return report(uc, halide_error_code_buffer_extents_negative, "%s: %s has a negative extent in dimension %d", what, a.name, d);
        span += (long)std::max(t.extent - 1, 0) * std::abs((long)t.stride);
    }
    if (span >= (1L << 31)) return report(uc, halide_error_code_buffer_allocation_too_large, "%s: %s spans more than 2^31 - 1 elements", what, a.name);
    return 0;
}
bool dst_covered(const halide_buffer_t *src, const halide_buffer_t *dst) {
    for (int d = 0; d < dst->dimensions; d++)
        if (src->dim[d].min > dst->dim[d].min || (long)src->dim[d].min + src->dim[d].extent < (long)dst->dim[d].min + dst->dim[d].extent) return false;
    return true;
}

template<typename T>
int launch_copy(void *uc, hipStream_t stream, const MovePlan &p) {
    const CopyGeom &g = p.g;
    unsigned blocks;
    if (p.kernel == MOVE_ROWS) {
        const long row_bytes = (long)g.e[0] * (long)sizeof(T), total = (row_bytes + 15) / 16 * (p.total / g.e[0]);
        if (int r = blocks_ok(uc, "hannk_copy_from", total, &blocks)) return r;
        HLMI_LAUNCH(uc, "hannk_cf_rows", stream, hannk_cf_rows<T>, dim3(blocks), dim3(256), 0, g, row_bytes, total);
    } else if (p.kernel == MOVE_TRANSPOSE) {
        if constexpr (sizeof(T) > 1) {   // the plan sends no 1-byte copy here
            constexpr int TILE = sizeof(T) == 8 ? 32 : 64, PAD = sizeof(T) == 2 ? 2 : 1;
            const int ta = (g.e[0] + TILE - 1) / TILE, tb = (g.e[1] + TILE - 1) / TILE;
            const long nblk = (long)ta * tb * (p.total / g.e[0] / g.e[1]);
            if (nblk > 0x7fffffffL) return report(uc, halide_error_code_buffer_extents_too_large, "hannk_copy_from: %ld workgroups exceed one launch", nblk);
            constexpr auto kernel = hannk_cf_transpose<T, TILE, PAD>;
            HLMI_LAUNCH(uc, "hannk_cf_transpose", stream, kernel, dim3((unsigned)nblk), dim3(256), 0, g, ta, tb);
        }
    } else {
        if (int r = blocks_ok(uc, "hannk_copy_from", p.total, &blocks)) return r;
        HLMI_LAUNCH(uc, "hannk_cf_general", stream, hannk_cf_general<T>, dim3(blocks), dim3(256), 0, g, p.total);
    }
    return 0;
}

template<bool GENERAL>
int copy_from_entry(const halide_buffer_t *src, halide_buffer_t *dst) {
    void *uc = nullptr;
    const BufArg args[2] = {{"src", const_cast<halide_buffer_t *>(src), 0, 0, false}, {"dst", dst, 0, 0, true}};
    int r = move_protocol(uc, args, 2, "hannk_copy_from");
    if (r) return r;
    const int es = elem_size(src);
    if (src->dimensions != dst->dimensions || dst->dimensions > MOVE_MAX_RANK || dst->dimensions < 0)
        return report(uc, halide_error_code_bad_dimensions, "hannk_copy_from: src has %d dimensions and dst has %d (equal, at most %d)", src->dimensions,
                      dst->dimensions, MOVE_MAX_RANK);
    if ((r = check_span(uc, "hannk_copy_from", args[0])) || (r = check_span(uc, "hannk_copy_from", args[1]))) return r;
    MovePlan p;
    if (move_plan(src, dst, es, GENERAL, p))
        return report(uc, halide_error_code_constraint_violated, "hannk_copy_from: distinct indices of dst share an element (a stride of 0)");
    if (p.kernel == MOVE_EMPTY) return 0;
    if ((r = check_unallocated_host(uc, args, 2))) return r;
    DeviceCtx ctx;
    if ((r = acquire_device(uc, &ctx)) || (r = input_to_device(uc, ctx, args[0]))) return r;
    // a dst that the copy writes only in part keeps the rest of what its host side holds
    if (dst->host && (dst->device == 0 || (dst->flags & halide_buffer_flag_host_dirty)) && !dst_covered(src, dst)) {
        const BufArg keep = {"dst", dst, 0, 0, false};
        if ((r = input_to_device(uc, ctx, keep))) return r;
    }
    if ((r = output_on_device(uc, ctx, args[1])) || (r = check_aligned(uc, "hannk_copy_from", args[0], es)) ||
        (r = check_aligned(uc, "hannk_copy_from", args[1], es)))
        return r;
    p.g.src = dev_ptr<uint8_t>(src) + p.soff * es, p.g.dst = dev_ptr<uint8_t>(dst) + p.doff * es;
    timing_note_bytes(2.0 * (double)p.total * es);
    switch (es) {
    case 1: r = launch_copy<uint8_t>(uc, ctx.stream, p); break;
    case 2: r = launch_copy<uint16_t>(uc, ctx.stream, p); break;
    case 4: r = launch_copy<uint32_t>(uc, ctx.stream, p); break;
    default: r = launch_copy<uint64_t>(uc, ctx.stream, p); break;
    }
    if (r) return r;
    mark_output_written(dst);
    return 0;
}

template<typename T>
int launch_gather(void *uc, hipStream_t stream, const GatherGeom &g, long total) {
    unsigned blocks;
    if (int r = blocks_ok(uc, "hannk_gather", total, &blocks)) return r;
    HLMI_LAUNCH(uc, "hannk_gather", stream, hannk_gather_kernel<T>, dim3(blocks), dim3(256), 0, g, total);
    return 0;
}

int gather_entry(const halide_buffer_t *src, const halide_buffer_t *indices, int axis, halide_buffer_t *dst) {
    void *uc = nullptr;
    const BufArg args[3] = {{"src", const_cast<halide_buffer_t *>(src), 0, 0, false},
                            {"indices", const_cast<halide_buffer_t *>(indices), T_I32, 0, false},
                            {"dst", dst, 0, 0, true}};
    int r = move_protocol(uc, args, 3, "hannk_gather");
    if (r) return r;
    const int es = elem_size(src);
    if ((buf_type_abi(indices) & 0xffffu) != T_I32) return report(uc, halide_error_code_bad_type, "hannk_gather: indices must be int32");
    const int k = std::max(indices->dimensions, 1);   // a scalar index is one index (ops.cpp:1127-1130)
    if (indices->dimensions < 0 || indices->dimensions > 2 || src->dimensions < 1 || dst->dimensions != src->dimensions + indices->dimensions - 1 ||
        dst->dimensions + (indices->dimensions == 0) > MOVE_MAX_RANK)
        return report(uc, halide_error_code_bad_dimensions, "hannk_gather: src has %d dimensions, indices %d and dst %d", src->dimensions, indices->dimensions,
                      dst->dimensions);
    if (axis < 0 || axis >= src->dimensions) return report(uc, halide_error_code_constraint_violated, "hannk_gather: axis %d is not a dimension of src", axis);
    if ((r = check_span(uc, "hannk_gather", args[0])) || (r = check_span(uc, "hannk_gather", args[1])) || (r = check_span(uc, "hannk_gather", args[2]))) return r;
    // dst as the kernel sees it: a scalar index gives it a dimension of extent 1 at `axis`
    GatherGeom g = {};
    g.n = src->dimensions + k - 1, g.axis = axis, g.k = k;
    long total = 1;
    for (int d = 0; d < g.n; d++) {
        const bool index_dim = d >= axis && d < axis + k;
        int want = 0;
        if (index_dim && indices->dimensions == 0) {
            g.e[d] = 1, g.ds[d] = 0, g.is[0] = 0;
            continue;
        }
        const halide_dimension_t &t = dst->dim[indices->dimensions == 0 && d > axis ? d - 1 : d];
        if (index_dim) {
            want = indices->dim[d - axis].extent, g.is[d - axis] = indices->dim[d - axis].stride;
        } else {
            const halide_dimension_t &s = src->dim[d < axis ? d : d - k + 1];
            want = s.extent, g.ss[d] = s.stride;
        }
        if (t.extent != want) return report(uc, halide_error_code_constraint_violated, "hannk_gather: dst has extent %d where %d is expected", t.extent, want);
        if (t.stride == 0 && t.extent > 1) return report(uc, halide_error_code_constraint_violated, "hannk_gather: distinct indices of dst share an element");
        g.e[d] = t.extent, g.ds[d] = t.stride;
        total *= t.extent;
    }
    g.axis_min = src->dim[axis].min, g.axis_extent = src->dim[axis].extent, g.axis_stride = src->dim[axis].stride;
    if (total == 0) return 0;
    // indices the host holds (a model's constant) are checked here; indices that live on the device by the kernel's flag, read back
    // after the launch: the one host synchronisation
    const bool host_indices = indices->host && !(indices->flags & halide_buffer_flag_device_dirty);
    bool bad = false;
    if (host_indices) {
        const int e0 = indices->dimensions > 0 ? indices->dim[0].extent : 1, e1 = indices->dimensions > 1 ? indices->dim[1].extent : 1;
        const long s0 = indices->dimensions > 0 ? indices->dim[0].stride : 0, s1 = indices->dimensions > 1 ? indices->dim[1].stride : 0;
        for (int j = 0; j < e1; j++)
            for (int i = 0; i < e0; i++) {
                const long at = (long)reinterpret_cast<const int32_t *>(indices->host)[i * s0 + j * s1] - g.axis_min;
                bad |= at < 0 || at >= g.axis_extent;
            }
    }
    if ((r = check_unallocated_host(uc, args, 3))) return r;
    DeviceCtx ctx;
    if ((r = acquire_device(uc, &ctx)) || (r = input_to_device(uc, ctx, args[0])) || (r = input_to_device(uc, ctx, args[1]))) return r;
    if (dst->host && (dst->device == 0 || (dst->flags & halide_buffer_flag_host_dirty)) && bad) {   // the slices left out keep what the host side holds
        const BufArg keep = {"dst", dst, 0, 0, false};
        if ((r = input_to_device(uc, ctx, keep))) return r;
    }
    if ((r = output_on_device(uc, ctx, args[2])) || (r = check_aligned(uc, "hannk_gather", args[0], es)) || (r = check_aligned(uc, "hannk_gather", args[1], 4)) ||
        (r = check_aligned(uc, "hannk_gather", args[2], es)))
        return r;
    void *flag = nullptr;
    if ((r = get_workspace(uc, ctx, sizeof(int), &flag))) return r;
    g.src = dev_ptr<uint8_t>(src), g.idx = dev_ptr<int32_t>(indices), g.dst = dev_ptr<uint8_t>(dst), g.flag = (int *)flag;
    HLMI_HIP(uc, hipMemsetAsync(flag, 0, sizeof(int), ctx.stream));
    timing_note_bytes(2.0 * (double)total * es);
    switch (es) {
    case 1: r = launch_gather<uint8_t>(uc, ctx.stream, g, total); break;
    case 2: r = launch_gather<uint16_t>(uc, ctx.stream, g, total); break;
    case 4: r = launch_gather<uint32_t>(uc, ctx.stream, g, total); break;
    default: r = launch_gather<uint64_t>(uc, ctx.stream, g, total); break;
    }
    if (r) return r;
    mark_output_written(dst);
    if (!host_indices) {
        int seen = 0;
        HLMI_HIP(uc, hipMemcpyAsync(&seen, flag, sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
        HLMI_HIP(uc, hipStreamSynchronize(ctx.stream));
        bad = seen != 0;
    }
    if (bad) return report(uc, halide_error_code_constraint_violated, "hannk_gather: an index lies outside [%d, %d): its slice of dst was not written",
                           g.axis_min, g.axis_min + g.axis_extent);
    return 0;
}

}  // namespace
}  // namespace hlmi

extern "C" int hlmi_hannk_copy_from(const halide_buffer_t *src, halide_buffer_t *dst) { return hlmi::copy_from_entry<false>(src, dst); }
extern "C" int hlmi_hannk_gather(const halide_buffer_t *src, const halide_buffer_t *indices, int axis, halide_buffer_t *dst) {
    return hlmi::gather_entry(src, indices, axis, dst);
}

int hlmi::hannk_copy_general(const char *name, void **argv) {
    if (!strcmp(name, "hannk_copy_from")) return copy_from_entry<true>((const halide_buffer_t *)argv[0], (halide_buffer_t *)argv[1]);
    if (!strcmp(name, "hannk_gather"))   // its one kernel is the general one
        return gather_entry((const halide_buffer_t *)argv[0], (const halide_buffer_t *)argv[1], *(const int *)argv[2], (halide_buffer_t *)argv[3]);
    return -1;
}

extern "C" int hlmi_debug_hannk_move_plan(const halide_buffer_t *src, const halide_buffer_t *dst, int32_t general, int32_t *out) {
    if (!src || !dst || !out || src->dimensions != dst->dimensions || dst->dimensions > hlmi::MOVE_MAX_RANK || dst->dimensions < 0) return -1;
    const int es = hlmi::elem_size(dst);
    if (!hlmi::size_ok(es)) return -1;
    hlmi::MovePlan p;
    if (int r = hlmi::move_plan(src, dst, es, general != 0, p)) return r;
    out[0] = p.kernel, out[1] = p.rank;
    return 0;
}
