// hannk_program.hip — the elementwise programs and the data movers of apps/hannk's op library (apps/hannk/halide/elementwise_generator.cpp:112-229,
// copy_generator.cpp, fill_generator.cpp, depthwise_conv_generator.cpp:244-270), C++-mangled in namespace hannk as the reference builds them:
//   hannk::elementwise_5xuint8_1xuint8, hannk::elementwise_5xint16_1xuint8int16, hannk::copy_uint8_uint8, hannk::fill_uint8,
//   hannk::upsample_channels_uint8, each with _argv and _metadata (include/aot/halide/<name>.h).
//
// The contract is integer throughout (the instruction rule elementwise_op and its approx_* helpers are in hannk_math.h).
//   elementwise  slot -i-1 = i16(input_i(x, y)), slot 0 = 0, instruction n (from 0) writes slot n + 1 = elementwise_op(op, slot arg1, slot
//                arg2, arg3, arg4); output i of k = saturating_cast(type_i, slot n - k + i + 1)
//   copy         out(c, x, y, b) = c inside the input's dimension 0 ? in(c, x, y, b) : u8(pad_value)
//   fill         out = value
//   upsample     out(c, x, y, b) = in(c / factor, x, y, b), Halide's division (c / 0 == 0)
//
// The program is read on the host once per call (the host copy if it is current, else a small device-to-host copy), validated (an operand
// of an instruction with opcode 1 .. 10 outside [-5, n] is refused: no kernel indexes outside the slots) and passed to the kernels by value;
// the instruction loop and every operand index are wave-uniform.
//
// Kernels (each op: a default plan and the general kernel, one thread per output with the loops as written, behind hlmi_hannk_general):
//   hannk_prog_table    a u8 program that names at most one input is a function of one byte: every workgroup runs the interpreter
//                       once over the 256 byte values (slots in LDS) and applies the table, 16 bytes per lane where the addresses allow;
//                       the default for large outputs (ew_plan)
//   hannk_prog_interp   a lane owns two adjacent elements, the slots of its pair packed in one dword: slot-major, lane-minor in LDS (one
//                       conflict-free dword per lane and access), or in registers reached through wave-uniform selects.  Neither layout
//                       measured ahead of hannk_prog_general (DESIGN.md §5.14 has the timings): reached through HLMI_HANNK_EW_PLAN only
//   hannk_prog_general  one thread per output, the slots a private array the compiler keeps in registers (no scratch): the default for
//                       every other program
//   hannk_rows16        copy of equal channels, the 3 -> 4 channel pad and fill: rows merged as far as the strides allow, 16 bytes per
//                       lane where the addresses allow, bytes otherwise
//   hannk_upsample16    16 output channels of one pixel per lane; a factor that is a multiple of 4 splats a byte into a dword
//
// Host path: every entry point reads top to bottom: check arguments -> bounds query (upsample) -> device and buffers -> empty output ->
// plan -> launch -> mark_output_written.
#include "hlmi_internal.h"
#include "hannk_entry.h"
#include "hannk_math.h"

using namespace hlmi;

namespace {

using namespace hlmi::hannk_math;
using namespace hlmi::hannk_entry;

// ---------------------------------------------------------------------------------------------------------------- elementwise programs
struct EwProgram {
    int32_t n;                               // instructions, <= EW_MAX_INSTRUCTIONS
    int16_t w[EW_MAX_INSTRUCTIONS * 5];      // op, arg1, arg2, arg3, arg4; the operands of a Noop are 0
};
struct ProgGeom {
    const void *in[EW_INPUTS];   // input i's element at the output's (x_min, y_min); a stride-0 input: at (its own x_min, y_min)
    long in_s0[EW_INPUTS], in_s1[EW_INPUTS];   // in_s0: 0 or 1
    uint8_t *out0;
    int16_t *out1;               // the i16 variant's second output
    long o0_s1, o1_s1;
    int W, H;
};
template<bool I16>
__device__ __forceinline__ int32_t prog_load(const void *p, long at) {
    return I16 ? (int32_t)((const int16_t *)p)[at] : (int32_t)((const uint8_t *)p)[at];
}
__device__ __forceinline__ int32_t sat_u8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one thread per output, the slots in a private array indexed as the program says
template<bool I16>
__global__ __launch_bounds__(256) void hannk_prog_general(ProgGeom g, EwProgram pr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.W * g.H) return;
    const int x = (int)(i % g.W);
    const long y = i / g.W;
    int32_t s[EW_SLOTS];   // slot k at s[k + EW_INPUTS]
    for (int k = 0; k < EW_INPUTS; k++) s[EW_INPUTS - 1 - k] = prog_load<I16>(g.in[k], y * g.in_s1[k] + x * g.in_s0[k]);
    s[EW_INPUTS] = 0;
    for (int n = 0; n < pr.n; n++) {
        const int16_t *w = pr.w + 5 * n;
        s[EW_INPUTS + n + 1] = elementwise_op(w[0], s[EW_INPUTS + w[1]], s[EW_INPUTS + w[2]], w[3], w[4]);
    }
    if (I16) {
        g.out0[y * g.o0_s1 + x] = (uint8_t)sat_u8(s[EW_INPUTS + pr.n - 1]);
        g.out1[y * g.o1_s1 + x] = (int16_t)s[EW_INPUTS + pr.n];
    } else {
        g.out0[y * g.o0_s1 + x] = (uint8_t)sat_u8(s[EW_INPUTS + pr.n]);
    }
}

// ---- the slots of a lane's element pair, one packed dword per slot
__device__ __forceinline__ void unpack2(uint32_t d, int32_t (&v)[2]) { v[0] = (int32_t)(int16_t)(d & 0xffffu), v[1] = (int32_t)d >> 16; }
__device__ __forceinline__ uint32_t pack2(const int32_t (&v)[2]) { return ((uint32_t)v[0] & 0xffffu) | ((uint32_t)v[1] << 16); }
struct SlotsLds {   // slot k of thread t at lds[(k + EW_INPUTS) * 256 + t]: a column no other lane touches, so no barrier orders it
    uint32_t *col;
    __device__ __forceinline__ uint32_t get(int k) const { return col[(k + EW_INPUTS) * 256]; }
    __device__ __forceinline__ void set(int k, uint32_t v) { col[(k + EW_INPUTS) * 256] = v; }
};
struct SlotsReg {   // every index below is a compile-time constant after unrolling: the array stays in registers
    uint32_t s[EW_SLOTS];
    __device__ __forceinline__ uint32_t get(int k) const {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < EW_SLOTS; j++) v = j == k + EW_INPUTS ? s[j] : v;
        return v;
    }
    __device__ __forceinline__ void set(int k, uint32_t v) {
#pragma unroll
        for (int j = 0; j < EW_SLOTS; j++) s[j] = j == k + EW_INPUTS ? v : s[j];
    }
};
template<typename S>
__device__ __forceinline__ void run_program(S &sl, const EwProgram &pr) {
    for (int n = 0; n < pr.n; n++) {
        const int16_t *w = pr.w + 5 * n;
        const int op = w[0], arg3 = w[3], arg4 = w[4];
        int32_t a[2], b[2], r[2];
        unpack2(sl.get(w[1]), a);
        unpack2(sl.get(w[2]), b);
#pragma unroll
        for (int e = 0; e < 2; e++) r[e] = elementwise_op(op, a[e], b[e], arg3, arg4);
        sl.set(n + 1, pack2(r));
    }
}

template<bool I16, bool LDS>
__global__ __launch_bounds__(256) void hannk_prog_interp(ProgGeom g, EwProgram pr) {
    __shared__ uint32_t lds[LDS ? EW_SLOTS * 256 : 1];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int npair = (g.W + 1) / 2;
    if (i >= (long)npair * g.H) return;   // (no barrier in this kernel)
    const int x0 = (int)(i % npair) * 2;
    const long y = i / npair;
    const bool two = x0 + 1 < g.W;
    typename std::conditional<LDS, SlotsLds, SlotsReg>::type sl;
    if constexpr (LDS) {
        sl.col = lds + threadIdx.x;
    } else {
#pragma unroll
        for (int j = 0; j < EW_SLOTS; j++) sl.s[j] = 0;
    }
#pragma unroll
    for (int k = 0; k < EW_INPUTS; k++) {
        const long at = y * g.in_s1[k] + x0 * g.in_s0[k];
        int32_t v[2];
        v[0] = prog_load<I16>(g.in[k], at);
        v[1] = g.in_s0[k] == 0 ? v[0] : two ? prog_load<I16>(g.in[k], at + 1) : 0;
        sl.set(-k - 1, pack2(v));
    }
    sl.set(0, 0u);
    run_program(sl, pr);
    int32_t o0[2], o1[2];
    unpack2(sl.get(I16 ? pr.n - 1 : pr.n), o0);
    uint8_t *p0 = g.out0 + y * g.o0_s1 + x0;
    p0[0] = (uint8_t)sat_u8(o0[0]);
    if (two) p0[1] = (uint8_t)sat_u8(o0[1]);
    if (I16) {
        unpack2(sl.get(pr.n), o1);
        int16_t *p1 = g.out1 + y * g.o1_s1 + x0;
        p1[0] = (int16_t)o1[0];
        if (two) p1[1] = (int16_t)o1[1];
    }
}

// the u8 program as a byte table: `which` is the one input the program names
struct TableGeom {
    const uint8_t *in;   // as ProgGeom::in[which]
    uint8_t *out;
    long in_s0, in_s1, o_s1;
    int W, H;
    int which;
    int iters;           // 16-byte chunks a lane takes, 256 lanes apart
};
__global__ __launch_bounds__(256) void hannk_prog_table(TableGeom g, EwProgram pr) {
    __shared__ uint32_t lds[EW_SLOTS * 256];
    __shared__ uint8_t table[256];
    {
        SlotsLds sl;
        sl.col = lds + threadIdx.x;
        for (int k = -EW_INPUTS; k <= 0; k++) sl.set(k, k == -g.which - 1 ? threadIdx.x : 0u);
        run_program(sl, pr);
        int32_t o[2];
        unpack2(sl.get(pr.n), o);
        table[threadIdx.x] = (uint8_t)sat_u8(o[0]);
    }
    __syncthreads();
    const int nch = (g.W + 15) / 16;
    const long total = (long)nch * g.H;
    for (int it = 0; it < g.iters; it++) {
        const long i = ((long)blockIdx.x * g.iters + it) * 256 + threadIdx.x;
        if (i >= total) break;
        const int x0 = (int)(i % nch) * 16;
        const long y = i / nch;
        const uint8_t *pi = g.in + y * g.in_s1 + x0 * g.in_s0;
        uint8_t *po = g.out + y * g.o_s1 + x0;
        if (x0 + 16 <= g.W && g.in_s0 == 1 && (((uintptr_t)pi | (uintptr_t)po) & 15) == 0) {
            const uint4 t = *reinterpret_cast<const uint4 *>(pi);
            const uint32_t vi[4] = {t.x, t.y, t.z, t.w};
            uint32_t vo[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                vo[k] = (uint32_t)table[vi[k] & 0xffu] | ((uint32_t)table[(vi[k] >> 8) & 0xffu] << 8) | ((uint32_t)table[(vi[k] >> 16) & 0xffu] << 16) |
                        ((uint32_t)table[vi[k] >> 24] << 24);
            *reinterpret_cast<uint4 *>(po) = make_uint4(vo[0], vo[1], vo[2], vo[3]);
        } else {
            const int n = min(16, g.W - x0);
            for (int k = 0; k < n; k++) po[k] = table[pi[k * g.in_s0]];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- copy, fill
// Rows: dimension 0 and every further dimension that follows it without a gap (in both buffers) are one row of L units; up to three
// dimensions stay outside.  MODE: what a unit is
enum { ROWS_COPY = 0, ROWS_PAD34 = 1, ROWS_FILL = 2 };
struct RowsGeom {
    const uint8_t *in;   // the input element of the output's first (copy: the rows are bytes; pad34: pixels of 3 bytes)
    uint8_t *out;
    long L;              // copy, fill: bytes per row; pad34: pixels per row
    int e[3];            // the outer extents (1 where merged)
    long is[3], os[3];
    uint32_t value;      // fill's value, pad34's fourth channel
};
template<int MODE>
__global__ __launch_bounds__(256) void hannk_rows16(RowsGeom g) {
    constexpr int UNITS = MODE == ROWS_PAD34 ? 4 : 16;   // units of a lane's 16 output bytes
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nch = (g.L + UNITS - 1) / UNITS;
    if (i >= nch * g.e[0] * g.e[1] * g.e[2]) return;
    const long u0 = (i % nch) * UNITS;
    long r = i / nch;
    const int r0 = (int)(r % g.e[0]);
    r /= g.e[0];
    const int r1 = (int)(r % g.e[1]), r2 = (int)(r / g.e[1]);
    uint8_t *po = g.out + r0 * g.os[0] + r1 * g.os[1] + r2 * g.os[2] + u0 * (MODE == ROWS_PAD34 ? 4 : 1);
    const uint8_t *pi = MODE == ROWS_FILL ? nullptr : g.in + r0 * g.is[0] + r1 * g.is[1] + r2 * g.is[2] + u0 * (MODE == ROWS_PAD34 ? 3 : 1);
    const int n = (int)min((long)UNITS, g.L - u0);
    const bool whole = n == UNITS && ((uintptr_t)po & 15) == 0;
    if (MODE == ROWS_FILL) {
        const uint32_t v = g.value * 0x01010101u;
        if (whole) *reinterpret_cast<uint4 *>(po) = make_uint4(v, v, v, v);
        else
            for (int k = 0; k < n; k++) po[k] = (uint8_t)g.value;
    } else if (MODE == ROWS_COPY) {
        if (whole && ((uintptr_t)pi & 15) == 0) *reinterpret_cast<uint4 *>(po) = *reinterpret_cast<const uint4 *>(pi);
        else
            for (int k = 0; k < n; k++) po[k] = pi[k];
    } else {
        if (whole && ((uintptr_t)pi & 3) == 0) {
            const uint32_t a = reinterpret_cast<const uint32_t *>(pi)[0], b = reinterpret_cast<const uint32_t *>(pi)[1], c = reinterpret_cast<const uint32_t *>(pi)[2];
            const uint32_t v = g.value << 24;
            *reinterpret_cast<uint4 *>(po) = make_uint4((a & 0xffffffu) | v, (a >> 24) | ((b & 0xffffu) << 8) | v, (b >> 16) | ((c & 0xffu) << 16) | v, (c >> 8) | v);
        } else {
            for (int k = 0; k < n; k++) {
                po[4 * k] = pi[3 * k], po[4 * k + 1] = pi[3 * k + 1], po[4 * k + 2] = pi[3 * k + 2];
                po[4 * k + 3] = (uint8_t)g.value;
            }
        }
    }
}
struct MoveGeom {   // the general kernels of copy, fill and upsample_channels
    const uint8_t *in;   // input element (its own c_min; the output's x_min, y_min, b_min)
    uint8_t *out;
    int ext[4];
    long is[4], os[4];
    int c_off;           // copy: output.min(0) - input.min(0); upsample: output.min(0)
    int c_in;            // copy: the input's extent 0; upsample: the input's min 0
    int param;           // copy: u8(pad_value); fill: value; upsample: factor
};
// Halide's integer division (div_imp, src/IROperator.h:290-310): rounds toward -inf for a positive divisor, the remainder is never negative, x / 0 == 0
__host__ __device__ inline int halide_div(int a, int b) {
    if (b == 0) return 0;
    const long d = b < 0 ? -(long)b : (long)b;
    long q = a / d;
    if (a % d < 0) q--;   // floor(a / |b|)
    return (int)(b < 0 ? -q : q);
}
enum { MOVE_COPY = 0, MOVE_FILL = 1, MOVE_UPSAMPLE = 2 };
template<int OP>
__global__ __launch_bounds__(256) void hannk_move_general(MoveGeom g) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.ext[0] * g.ext[1] * g.ext[2] * g.ext[3]) return;
    int o[4];
    long ooff = 0, ioff = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        o[d] = (int)(i % g.ext[d]);
        i /= g.ext[d];
        ooff += o[d] * g.os[d];
        if (d > 0) ioff += o[d] * g.is[d];
    }
    int v;
    if (OP == MOVE_FILL) {
        v = g.param;
    } else if (OP == MOVE_COPY) {
        const long ci = (long)o[0] + g.c_off;
        v = ci >= 0 && ci < g.c_in ? g.in[ioff + ci] : g.param;
    } else {
        v = g.in[ioff + (long)(halide_div(o[0] + g.c_off, g.param) - g.c_in)];
    }
    g.out[ooff] = (uint8_t)v;
}
// a lane: output channels c0 .. c0 + 15 of one pixel
__global__ __launch_bounds__(256) void hannk_upsample16(MoveGeom g) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int nch = (g.ext[0] + 15) / 16;
    if (i >= (long)nch * g.ext[1] * g.ext[2] * g.ext[3]) return;
    const int c0 = (int)(i % nch) * 16;
    i /= nch;
    long ooff = c0, ioff = 0;
#pragma unroll
    for (int d = 1; d < 4; d++) {
        const int od = (int)(i % g.ext[d]);
        i /= g.ext[d];
        ooff += od * g.os[d], ioff += od * g.is[d];
    }
    const uint8_t *pi = g.in + ioff;
    uint8_t *po = g.out + ooff;
    const int n = min(16, g.ext[0] - c0);
    const bool splat = g.param != 0 && g.param % 4 == 0 && (c0 + g.c_off) % 4 == 0;   // a quad of channels never straddles a multiple of the factor
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (4 * k >= n) {
            v[k] = 0;
        } else if (splat) {
            v[k] = (uint32_t)pi[halide_div(c0 + 4 * k + g.c_off, g.param) - g.c_in] * 0x01010101u;
        } else {
            v[k] = 0;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (4 * k + j < n) v[k] |= (uint32_t)pi[halide_div(c0 + 4 * k + j + g.c_off, g.param) - g.c_in] << (8 * j);
        }
    }
    if (n == 16 && ((uintptr_t)po & 15) == 0) {
        *reinterpret_cast<uint4 *>(po) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < n; k++) po[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    }
}

// the debug hook's kernel: fn as hlmi_debug_hannk_program_approx
__host__ __device__ inline int32_t program_approx(int fn, int width, int32_t x, int32_t q, int32_t q_x) {
    if (width == 16) {
        return fn == 0 ? approx_log2pm1_exp2<16>(q, x, 1, q_x) : fn == 1 ? approx_log2pm1_exp2<16>(q, x, -1, q_x) : fn == 2 ? approx_logistic<16>(q, x, q_x) :
                                                                                                                             approx_tanh<16>(q, x, q_x);
    }
    return fn == 0 ? approx_log2pm1_exp2<32>(q, x, 1, q_x) : fn == 1 ? approx_log2pm1_exp2<32>(q, x, -1, q_x) : fn == 2 ? approx_logistic<32>(q, x, q_x) :
                                                                                                                         approx_tanh<32>(q, x, q_x);
}
__global__ __launch_bounds__(256) void dbg_hannk_program_approx(int fn, int width, const int32_t *__restrict__ x, const int32_t *__restrict__ q,
                                                                const int32_t *__restrict__ q_x, size_t n, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = program_approx(fn, width, x[i], q[i], q_x[i]);
}

// ---------------------------------------------------------------------------------------------------------------- host: tables
const ArgTable ew_u8_table("elementwise_5xuint8_1xuint8",
                           {L(in_buf("inputs_0", T_U8, 2)), L(in_buf("inputs_1", T_U8, 2)), L(in_buf("inputs_2", T_U8, 2)), L(in_buf("inputs_3", T_U8, 2)),
                            L(in_buf("inputs_4", T_U8, 2)), L(in_buf("program", T_I16, 2)), L(out_buf("output", T_U8, 2))});
// a Func with a Tuple value: one output buffer per component, named <func>.<i> (src/Function.cpp:729-735); the metadata keeps the dot
// (src/CodeGen_C.cpp:874-879), the header's parameter is _output_0_buffer (:1089)
const ArgTable ew_i16_table("elementwise_5xint16_1xuint8int16",
                            {L(in_buf("inputs_0", T_I16, 2)), L(in_buf("inputs_1", T_I16, 2)), L(in_buf("inputs_2", T_I16, 2)), L(in_buf("inputs_3", T_I16, 2)),
                             L(in_buf("inputs_4", T_I16, 2)), L(in_buf("program", T_I16, 2)), L(out_buf("output.0", T_U8, 2)), L(out_buf("output.1", T_I16, 2))});
const ArgTable copy_table("copy_uint8_uint8", {L(in_buf("input", T_U8, 4)), L(scalar_i32("pad_value")), L(out_buf("output", T_U8, 4))});
const ArgTable fill_table("fill_uint8", {L(scalar_u8("value")), L(out_buf("output", T_U8, 4))});
const ArgTable upsample_table("upsample_channels_uint8", {L(in_buf("input", T_U8, 4)), L(scalar_i32("factor")), L(out_buf("output", T_U8, 4))});

// ---------------------------------------------------------------------------------------------------------------- host: elementwise
// program(k, n), k in 0 .. 4, n in 0 .. count - 1, read on the host once per call: the host copy where it is current, else the buffer
// goes through the input protocol (which orders the stream behind its producer) and is fetched behind a stream synchronisation.
// `count` <= EW_MAX_INSTRUCTIONS; the checks have pinned the layout: element (k, n) at 5 n + k
int read_program(void *uc, const DeviceCtx *ctx, const BufArg &arg, int count, EwProgram *pr) {
    halide_buffer_t *b = arg.buf;
    pr->n = count;
    if (count == 0) return 0;
    if (b->host && !(b->flags & halide_buffer_flag_device_dirty)) {
        memcpy(pr->w, b->host, (size_t)count * 5 * sizeof(int16_t));
        return 0;
    }
    if (int r = input_to_device(uc, *ctx, arg)) return r;
    HLMI_HIP(uc, hipStreamSynchronize(ctx->stream));
    HLMI_HIP(uc, hipMemcpy(pr->w, dev_ptr<int16_t>(b), (size_t)count * 5 * sizeof(int16_t), hipMemcpyDeviceToHost));
    return 0;
}
bool program_on_host(const halide_buffer_t *b) { return b->host && !(b->flags & halide_buffer_flag_device_dirty); }
// This library's own refusal (the reference promises the range with unsafe_promise_clamped and checks nothing): instruction n may read
// the inputs, the constant and the slots written before it.  The operands of the other opcodes are not read: zeroed.
int validate_program(void *uc, EwProgram *pr) {
    for (int n = 0; n < pr->n; n++) {
        int16_t *w = pr->w + 5 * n;
        if (w[0] < 1 || w[0] > 10) {
            w[0] = w[1] = w[2] = 0;
            continue;
        }
        for (int k = 1; k <= 2; k++)
            if (w[k] < -EW_INPUTS || w[k] > n)
                return report(uc, halide_error_code_constraint_violated, "Constraint violated: program(%d, %d) (%d) is a slot in [-%d, %d]", k, n, w[k], EW_INPUTS, n);
    }
    return 0;
}
// the one input a program names: -1 none, 0 .. 4 that one, -2 several
int program_single_input(const EwProgram &pr) {
    int which = -1;
    for (int n = 0; n < pr.n; n++)
        for (int k = 1; k <= 2; k++) {
            const int a = pr.w[5 * n + k];
            if (a >= 0) continue;
            if (which >= 0 && which != -a - 1) return -2;
            which = -a - 1;
        }
    return which;
}

// ---- the plan.  A u8 program that names at most one input runs as a byte table where the output has at least EW_TABLE_MIN_OUTPUTS
// elements: every workgroup pays 256 runs of the program for its table, which measured level with the general kernel at 65 536 elements
// (6.5 - 7.2 against 6.6 us) and ahead from 262 144 (6.6 against 7.3 us; 8.1 against 22.7 us at 2.4 M).  Everything else runs on the
// one-thread-per-output kernel: the interpreter kernel with two elements per lane measured level with it on large outputs and behind
// it on small ones with either slot layout (the LSTM program on 2048 x 2048: 111.8 us with LDS slots, 175.7 us with register slots,
// 111.4 us general; on 32 x 2048: 14.3, 19.1 and 10.4 us), so it is reached through the switch only.
// HLMI_HANNK_EW_PLAN forces the choice: 0 the general kernel, 1 the table wherever the program allows it, 2 the interpreter kernel with
// LDS slots, 3 with register slots.
constexpr long EW_TABLE_MIN_OUTPUTS = 4 * 256L * 256;
enum class EwKernel { general, table, interp_lds, interp_reg };
EwKernel ew_plan(bool i16, int single_input, long outputs, std::optional<int> sw) {
    const bool table_ok = !i16 && single_input != -2;
    if (sw) {
        switch (*sw) {
        case 0: return EwKernel::general;
        case 1: return table_ok ? EwKernel::table : EwKernel::general;
        case 2: return EwKernel::interp_lds;
        case 3: return EwKernel::interp_reg;
        default: break;
        }
    }
    return table_ok && outputs >= EW_TABLE_MIN_OUTPUTS ? EwKernel::table : EwKernel::general;
}

template<bool I16, bool GENERAL>
int elementwise_entry(halide_buffer_t *const (&in)[EW_INPUTS], halide_buffer_t *program, halide_buffer_t *out0, halide_buffer_t *out1) {
    void *uc = nullptr;
    constexpr int NB = I16 ? 8 : 7, OUT0 = 6;
    const ArgTable &table = I16 ? ew_i16_table : ew_u8_table;
    BufArg args[NB];
    if constexpr (I16) table.bufs(args, {in[0], in[1], in[2], in[3], in[4], program, out0, out1});
    else table.bufs(args, {in[0], in[1], in[2], in[3], in[4], program, out0});
    own_lanes(args);
    int r = check_not_null(uc, args, NB);
    // built with no_bounds_query, as add and mul: an unallocated buffer is checked like any other and ends the call with -34
    if (r || (r = check_unallocated_types(uc, args, NB)) || (r = check_type_and_dims(uc, args, NB))) return r;
    const halide_dimension_t *od = out0->dim, *pd = program->dim;
    // ---- constraints (elementwise_generator.cpp:212, :226-227; a secondary output: src/AddImageChecks.cpp:520-549)
    for (int k = 0; k < EW_INPUTS; k++) check_shape_any_stride0(uc, args[k]);
    const int zero = 0, five = 5, one = 1;
    check_dim(uc, "program", program, 0, &zero, &five, &one);
    check_dim(uc, "program", program, 1, &zero, nullptr, &five);
    check_shape(uc, args[EW_INPUTS]);
    check_shape(uc, args[OUT0]);
    if (I16) {
        check_shape(uc, args[OUT0 + 1]);
        for (int d = 0; d < 2; d++) {
            char what[32], expect[32];
            snprintf(what, sizeof what, "output.1.min.%d", d), snprintf(expect, sizeof expect, "output.0.min.%d", d);
            check_equal(uc, what, out1->dim[d].min, expect, od[d].min);
            snprintf(what, sizeof what, "output.1.extent.%d", d), snprintf(expect, sizeof expect, "output.0.extent.%d", d);
            check_equal(uc, what, out1->dim[d].extent, expect, od[d].extent);
        }
    }
    // ---- regions: every input is loaded into its slot whatever the program reads
    const bool empty = od[0].extent <= 0 || od[1].extent <= 0;
    if (!empty)
        for (int k = 0; k < EW_INPUTS; k++)
            for (int d = 0; d < 2; d++) check_covers(uc, args[k], d, od[d].min, od[d].extent);
    const std::optional<int> sw_plan = env_int("HLMI_HANNK_EW_PLAN");
    if ((r = check_unallocated_host(uc, args, NB)) || (r = checks_done(uc))) return r;
    // ---- the program: read and refused before anything is uploaded where the host holds it
    const int count = pd[1].extent;
    EwProgram pr = {};
    bool have_program = false;
    if (count <= EW_MAX_INSTRUCTIONS && program_on_host(program)) {
        if ((r = read_program(uc, nullptr, args[EW_INPUTS], count, &pr)) || (r = validate_program(uc, &pr))) return r;
        have_program = true;
    }
    DeviceCtx ctx;
    BufArg io[NB - 1];   // the program stays where it is: read_program
    for (int k = 0, j = 0; k < NB; k++)
        if (k != EW_INPUTS) io[j++] = args[k];
    if ((r = to_device(uc, &ctx, io, NB - 1))) return r;
    // the specialisations (elementwise_generator.cpp:211-216): each input's dimension 0 has stride 1 or 0; anything else is specialize_fail
    for (int k = 0; k < EW_INPUTS; k++)
        if (in[k]->dim[0].stride != 0 && in[k]->dim[0].stride != 1)
            return report(uc, halide_error_code_specialize_fail, "A schedule specialized with specialize_fail() was chosen: Input dimension 0 must have stride 0 or 1.");
    // scratch.bound_extent(u, 5 + 20 + 1) (:219-221): slots -5 .. 20 (src/AllocationBoundsInference.cpp:112-120)
    if (count > EW_MAX_INSTRUCTIONS)
        return report(uc, halide_error_code_explicit_bounds_too_small, "Bounds given for u in scratch (from %d to %d) do not cover required region (from %d to %d)",
                      -EW_INPUTS, EW_MAX_INSTRUCTIONS, -EW_INPUTS, count);
    if (!have_program && ((r = read_program(uc, &ctx, args[EW_INPUTS], count, &pr)) || (r = validate_program(uc, &pr)))) return r;
    if (empty) {
        mark_output_written(out0);
        if (I16) mark_output_written(out1);
        return 0;
    }
    ProgGeom g = {};
    g.W = od[0].extent, g.H = od[1].extent;
    bool dense = true;   // rows that follow each other without a gap in every buffer are one long row
    for (int k = 0; k < EW_INPUTS; k++) {
        const halide_dimension_t *d = in[k]->dim;
        g.in_s0[k] = d[0].stride, g.in_s1[k] = d[1].stride;
        const long esz = I16 ? 2 : 1;
        const long off = (d[0].stride ? elem_offset(in[k], 0, od[0].min) : 0) + elem_offset(in[k], 1, od[1].min);
        g.in[k] = dev_ptr<uint8_t>(in[k]) + off * esz;
        dense = dense && d[0].stride == 1 && d[1].stride == g.W;
    }
    g.out0 = dev_ptr<uint8_t>(out0), g.o0_s1 = od[1].stride;
    dense = dense && g.o0_s1 == g.W;
    if (I16) {
        g.out1 = dev_ptr<int16_t>(out1), g.o1_s1 = out1->dim[1].stride;
        dense = dense && g.o1_s1 == g.W;
    }
    if (dense && (long)g.W * g.H < (1L << 31)) g.W *= g.H, g.H = 1;
    const int single = program_single_input(pr);
    const long outputs = (long)g.W * g.H;
    const EwKernel k = GENERAL ? EwKernel::general : ew_plan(I16, single, outputs, sw_plan);
    timing_note_bytes((double)outputs * (I16 ? 3 + 2 * EW_INPUTS : k == EwKernel::table ? 2 : 1 + EW_INPUTS));
    unsigned blocks;
    const char *name = table.md.name;
    if (k == EwKernel::general) {
        if ((r = blocks_ok(uc, name, outputs, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_prog_general", ctx.stream, hannk_prog_general<I16>, dim3(blocks), dim3(256), 0, g, pr);
    } else if (k == EwKernel::table) {
        if constexpr (!I16) {
            TableGeom t = {};
            t.which = std::max(single, 0);
            t.in = (const uint8_t *)g.in[t.which], t.out = g.out0;
            t.in_s0 = g.in_s0[t.which], t.in_s1 = g.in_s1[t.which], t.o_s1 = g.o0_s1, t.W = g.W, t.H = g.H;
            // every workgroup builds the table (256 runs of the program): a lane takes up to 8 chunks where that still leaves four
            // workgroups for every compute unit
            const long chunks = (long)((g.W + 15) / 16) * g.H;
            t.iters = (int)std::min<long>(8, std::max<long>(1, chunks / (256L * 1024)));
            if ((r = blocks_ok(uc, name, (chunks + t.iters - 1) / t.iters, &blocks))) return r;
            HLMI_LAUNCH(uc, "hannk_prog_table", ctx.stream, hannk_prog_table, dim3(blocks), dim3(256), 0, t, pr);
        }
    } else {
        if ((r = blocks_ok(uc, name, (long)((g.W + 1) / 2) * g.H, &blocks))) return r;
        if (k == EwKernel::interp_lds) HLMI_LAUNCH(uc, "hannk_prog_interp", ctx.stream, (hannk_prog_interp<I16, true>), dim3(blocks), dim3(256), 0, g, pr);
        else HLMI_LAUNCH(uc, "hannk_prog_interp", ctx.stream, (hannk_prog_interp<I16, false>), dim3(blocks), dim3(256), 0, g, pr);
    }
    mark_output_written(out0);
    if (I16) mark_output_written(out1);
    return 0;
}
template<bool GENERAL>
int ew_u8_entry(halide_buffer_t *i0, halide_buffer_t *i1, halide_buffer_t *i2, halide_buffer_t *i3, halide_buffer_t *i4, halide_buffer_t *program,
                halide_buffer_t *output) {
    return elementwise_entry<false, GENERAL>({i0, i1, i2, i3, i4}, program, output, nullptr);
}
template<bool GENERAL>
int ew_i16_entry(halide_buffer_t *i0, halide_buffer_t *i1, halide_buffer_t *i2, halide_buffer_t *i3, halide_buffer_t *i4, halide_buffer_t *program,
                 halide_buffer_t *output0, halide_buffer_t *output1) {
    return elementwise_entry<true, GENERAL>({i0, i1, i2, i3, i4}, program, output0, output1);
}

// ---------------------------------------------------------------------------------------------------------------- host: copy, fill
// rows of `unit_out` (`unit_in`) bytes per unit: merge x, y, b into the row while each follows without a gap in both buffers
void merge_rows(RowsGeom &g, const halide_dimension_t *od, const halide_dimension_t *id, long L, long unit_out, long unit_in, int first_dim) {
    g.L = L;
    int k = 0;
    bool merging = true;
    for (int d = first_dim; d < 4; d++) {
        if (merging && od[d].stride == g.L * unit_out && (!id || id[d].stride == g.L * unit_in) && g.L * od[d].extent < (1L << 31)) {
            g.L *= od[d].extent;
            continue;
        }
        merging = false;
        g.e[k] = od[d].extent, g.os[k] = od[d].stride, g.is[k] = id ? id[d].stride : 0, k++;
    }
    for (; k < 3; k++) g.e[k] = 1, g.os[k] = 0, g.is[k] = 0;
}
template<int MODE>
int launch_rows(void *uc, const char *name, hipStream_t stream, const RowsGeom &g) {
    const long units = MODE == ROWS_PAD34 ? 4 : 16;
    unsigned blocks;
    if (int r = blocks_ok(uc, name, ((g.L + units - 1) / units) * g.e[0] * g.e[1] * g.e[2], &blocks)) return r;
    HLMI_LAUNCH(uc, "hannk_rows16", stream, hannk_rows16<MODE>, dim3(blocks), dim3(256), 0, g);
    return 0;
}
void move_geom(MoveGeom &g, const halide_buffer_t *input, const halide_buffer_t *output) {
    for (int d = 0; d < 4; d++) {
        g.ext[d] = output->dim[d].extent, g.os[d] = output->dim[d].stride;
        g.is[d] = input ? input->dim[d].stride : 0;
    }
    g.out = dev_ptr<uint8_t>(output);
    if (input) {
        g.in = dev_ptr<uint8_t>(input);
        for (int d = 1; d < 4; d++) g.in += elem_offset(input, d, output->dim[d].min);
    }
}
template<int OP>
int launch_move_general(void *uc, const char *name, hipStream_t stream, const MoveGeom &g) {
    unsigned blocks;
    if (int r = blocks_ok(uc, name, (long)g.ext[0] * g.ext[1] * g.ext[2] * g.ext[3], &blocks)) return r;
    HLMI_LAUNCH(uc, "hannk_move_general", stream, hannk_move_general<OP>, dim3(blocks), dim3(256), 0, g);
    return 0;
}
bool empty4(const halide_buffer_t *b) { return b->dim[0].extent <= 0 || b->dim[1].extent <= 0 || b->dim[2].extent <= 0 || b->dim[3].extent <= 0; }
bool fits_int(const halide_buffer_t *b) { return (long)b->dim[0].extent * b->dim[1].extent < (1L << 31); }

// ---- copy, fill and upsample_channels take their 16-byte kernel wherever the layout allows it: it measured ahead of or level with the
// one-thread-per-output kernel at every size (equal-channel copy of 32 x 56^2 x 8: 6.5 against 7.3 us, fill: 6.4 against 6.7 us, both
// launch-bound; the 3 -> 4 pad of 32 x 224^2: 7.1 against 27.3 us).  HLMI_HANNK_MOVE_VECTOR = 0 forces the general kernel.
bool move_vector(bool general, std::optional<int> forced) { return !general && forced.value_or(1) != 0; }

// ---- the plan of a copy: equal channels (same min and extent in dimension 0) are rows of bytes; the interleaved 3 -> 4 channel pad
// (PadOp's special case) rows of pixels; any other channel window goes to the one-thread-per-output kernel, whose select per byte is the
// contract itself.
template<bool GENERAL>
int copy_entry(halide_buffer_t *input, int32_t pad_value, halide_buffer_t *output) {
    void *uc = nullptr;
    BufArg args[2];
    copy_table.bufs(args, {input, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 2);
    // no_bounds_query, as add and mul
    if (r || (r = check_unallocated_types(uc, args, 2)) || (r = check_type_and_dims(uc, args, 2))) return r;
    const halide_dimension_t *id = input->dim, *od = output->dim;
    check_shape(uc, args[0]);
    check_shape(uc, args[1]);
    const bool empty = empty4(output);
    // dimension 0 is clamped into the input (constant_exterior, copy_generator.cpp:21-22): only x, y, b can be out of bounds; an input
    // without channels is never read
    const bool reads = !empty && id[0].extent > 0;
    if (reads)
        for (int d = 1; d < 4; d++) check_covers(uc, args[0], d, od[d].min, od[d].extent);
    const std::optional<int> sw_vector = env_int("HLMI_HANNK_MOVE_VECTOR");
    if ((r = check_unallocated_host(uc, args, 2))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    const bool vector = move_vector(GENERAL, sw_vector);
    const uint32_t pad = (uint8_t)pad_value;   // cast(input_.type(), pad_value_): wraps
    const int C = od[0].extent;
    timing_note_bytes((double)od[1].extent * od[2].extent * od[3].extent * (C + std::min(C, std::max(id[0].extent, 0))));
    const bool same_c = reads && id[0].min == od[0].min && id[0].extent == C;
    const bool pad34 = reads && id[0].min == od[0].min && id[0].extent == 3 && C == 4 && id[1].stride == 3 && od[1].stride == 4 && fits_int(output);
    if (vector && (same_c || pad34)) {
        RowsGeom g = {};
        g.out = dev_ptr<uint8_t>(output), g.in = dev_ptr<uint8_t>(input), g.value = pad;
        for (int d = 1; d < 4; d++) g.in += elem_offset(input, d, od[d].min);
        if (same_c) {
            merge_rows(g, od, id, C, 1, 1, 1);
            r = launch_rows<ROWS_COPY>(uc, "copy_uint8_uint8", ctx.stream, g);
        } else {
            merge_rows(g, od, id, od[1].extent, 4, 3, 2);
            r = launch_rows<ROWS_PAD34>(uc, "copy_uint8_uint8", ctx.stream, g);
        }
    } else {
        MoveGeom g = {};
        move_geom(g, reads ? input : nullptr, output);
        g.c_off = reads ? od[0].min - id[0].min : 0, g.c_in = reads ? id[0].extent : 0, g.param = (int)pad;
        r = launch_move_general<MOVE_COPY>(uc, "copy_uint8_uint8", ctx.stream, g);
    }
    if (r) return r;
    mark_output_written(output);
    return 0;
}

// fill_uint8 is built with no_bounds_query no_asserts: the reference checks nothing.  What memory safety needs is kept: a null or
// unallocated buffer, its type and dimensions, and the shape checks that keep every offset inside 2^31 elements.
template<bool GENERAL>
int fill_entry(uint8_t value, halide_buffer_t *output) {
    void *uc = nullptr;
    BufArg args[1];
    fill_table.bufs(args, {output});
    own_lanes(args);
    int r = check_not_null(uc, args, 1);
    if (r || (r = check_unallocated_types(uc, args, 1)) || (r = check_type_and_dims(uc, args, 1))) return r;
    const halide_dimension_t *od = output->dim;
    check_shape(uc, args[0]);
    const std::optional<int> sw_vector = env_int("HLMI_HANNK_MOVE_VECTOR");
    if ((r = check_unallocated_host(uc, args, 1))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 1))) return r;
    if (empty4(output)) {
        mark_output_written(output);
        return 0;
    }
    timing_note_bytes((double)od[0].extent * od[1].extent * od[2].extent * od[3].extent);
    if (move_vector(GENERAL, sw_vector)) {
        RowsGeom g = {};
        g.out = dev_ptr<uint8_t>(output), g.value = value;
        merge_rows(g, od, nullptr, od[0].extent, 1, 1, 1);
        r = launch_rows<ROWS_FILL>(uc, "fill_uint8", ctx.stream, g);
    } else {
        MoveGeom g = {};
        move_geom(g, nullptr, output);
        g.param = value;
        r = launch_move_general<MOVE_FILL>(uc, "fill_uint8", ctx.stream, g);
    }
    if (r) return r;
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: upsample_channels
template<bool GENERAL>
int upsample_entry(halide_buffer_t *input, int32_t factor, halide_buffer_t *output) {
    void *uc = nullptr;
    BufArg args[2];
    upsample_table.bufs(args, {input, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 2);
    if (r || (r = check_type_and_dims(uc, args, 2))) return r;
    halide_dimension_t *id = input->dim, *od = output->dim;
    // the input's channels: c / factor is monotone in c (either way for a negative factor)
    const int ca = halide_div(od[0].min, factor), cb = halide_div(od[0].min + std::max(od[0].extent, 1) - 1, factor);
    const int clo = std::min(ca, cb), chi = std::max(ca, cb);
    if (any_bounds_query(args, 2)) {
        // dimension 3 is shared (require_same_min_extent, depthwise_conv_generator.cpp:259); a query output keeps c, x, y as given
        const int imin[4] = {clo, od[1].min, od[2].min, od[3].min}, iext[4] = {chi - clo + 1, od[1].extent, od[2].extent, od[3].extent};
        const int omin[4] = {od[0].min, od[1].min, od[2].min, id[3].min}, oext[4] = {od[0].extent, od[1].extent, od[2].extent, id[3].extent};
        answer_query(input, imin, iext);
        answer_query(output, omin, oext);
        return 0;
    }
    check_dim(uc, "output", output, 3, &id[3].min, &id[3].extent, nullptr);
    if ((r = check_shapes(uc, args, 2))) return r;
    const bool empty = empty4(output);
    if (!empty) {
        check_covers(uc, args[0], 0, clo, chi - clo + 1);
        for (int d = 1; d < 3; d++) check_covers(uc, args[0], d, od[d].min, od[d].extent);
    }
    const std::optional<int> sw_vector = env_int("HLMI_HANNK_MOVE_VECTOR");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    MoveGeom g = {};
    move_geom(g, input, output);
    g.c_off = od[0].min, g.c_in = id[0].min, g.param = factor;
    const double px = (double)od[1].extent * od[2].extent * od[3].extent;
    timing_note_bytes(px * (od[0].extent + (chi - clo + 1)));
    if (move_vector(GENERAL, sw_vector)) {
        unsigned blocks;
        if ((r = blocks_ok(uc, "upsample_channels_uint8", (long)((od[0].extent + 15) / 16) * od[1].extent * od[2].extent * od[3].extent, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_upsample16", ctx.stream, hannk_upsample16, dim3(blocks), dim3(256), 0, g);
    } else if ((r = launch_move_general<MOVE_UPSAMPLE>(uc, "upsample_channels_uint8", ctx.stream, g))) {
        return r;
    }
    mark_output_written(output);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- the entry points
#define HLMI_HANNK_ENTRY(name, table)                                             \
    int name##_argv(void **a) { return ::hlmi::argv_call(name, a); }              \
    const halide_filter_metadata_t *name##_metadata() { return &(table).md; }
namespace hannk {

int elementwise_5xuint8_1xuint8(halide_buffer_t *inputs_0, halide_buffer_t *inputs_1, halide_buffer_t *inputs_2, halide_buffer_t *inputs_3,
                                halide_buffer_t *inputs_4, halide_buffer_t *program, halide_buffer_t *output) {
    return ew_u8_entry<false>(inputs_0, inputs_1, inputs_2, inputs_3, inputs_4, program, output);
}
int elementwise_5xint16_1xuint8int16(halide_buffer_t *inputs_0, halide_buffer_t *inputs_1, halide_buffer_t *inputs_2, halide_buffer_t *inputs_3,
                                     halide_buffer_t *inputs_4, halide_buffer_t *program, halide_buffer_t *output_0, halide_buffer_t *output_1) {
    return ew_i16_entry<false>(inputs_0, inputs_1, inputs_2, inputs_3, inputs_4, program, output_0, output_1);
}
int copy_uint8_uint8(halide_buffer_t *input, int32_t pad_value, halide_buffer_t *output) { return copy_entry<false>(input, pad_value, output); }
int fill_uint8(uint8_t value, halide_buffer_t *output) { return fill_entry<false>(value, output); }
int upsample_channels_uint8(halide_buffer_t *input, int32_t factor, halide_buffer_t *output) { return upsample_entry<false>(input, factor, output); }
HLMI_HANNK_ENTRY(elementwise_5xuint8_1xuint8, ew_u8_table)
HLMI_HANNK_ENTRY(elementwise_5xint16_1xuint8int16, ew_i16_table)
HLMI_HANNK_ENTRY(copy_uint8_uint8, copy_table)
HLMI_HANNK_ENTRY(fill_uint8, fill_table)
HLMI_HANNK_ENTRY(upsample_channels_uint8, upsample_table)

}  // namespace hannk
#undef HLMI_HANNK_ENTRY

int hlmi::hannk_program_general(const char *name, void **argv) {
    if (!strcmp(name, "elementwise_5xuint8_1xuint8")) return argv_call(ew_u8_entry<true>, argv);
    if (!strcmp(name, "elementwise_5xint16_1xuint8int16")) return argv_call(ew_i16_entry<true>, argv);
    if (!strcmp(name, "copy_uint8_uint8")) return argv_call(copy_entry<true>, argv);
    if (!strcmp(name, "fill_uint8")) return argv_call(fill_entry<true>, argv);
    if (!strcmp(name, "upsample_channels_uint8")) return argv_call(upsample_entry<true>, argv);
    return hannk_copy_general(name, argv);   // copy_from and gather
}

// x, q, q_x, out: host pointers to n elements.  One launch.
extern "C" int hlmi_debug_hannk_program_approx(int fn, const int32_t *x, const int32_t *q, const int32_t *q_x, size_t n, int32_t width, int32_t *out) {
    if (fn < 0 || fn > 3 || !x || !q || !q_x || !out || n == 0 || (n + 255) / 256 > 0x7fffffffu || (width != 16 && width != 32)) return -1;
    for (size_t i = 0; i < n; i++)
        if (x[i] < -32768 || x[i] > 32767 || q[i] < 0 || q[i] > 15 || q_x[i] < 0 || q_x[i] > 15) return -1;
    void *d[4] = {nullptr, nullptr, nullptr, nullptr};
    const int32_t *src[3] = {x, q, q_x};
    int rc = 0;
    for (int i = 0; i < 4 && !rc; i++)
        if (hipMalloc(&d[i], 4 * n) != hipSuccess) rc = -2;
    for (int i = 0; i < 3 && !rc; i++)
        if (hipMemcpy(d[i], src[i], 4 * n, hipMemcpyHostToDevice) != hipSuccess) rc = -3;
    if (!rc) {
        hipLaunchKernelGGL(dbg_hannk_program_approx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (int)width, (const int32_t *)d[0], (const int32_t *)d[1],
                           (const int32_t *)d[2], n, (int32_t *)d[3]);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d[3], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
    }
    for (int i = 0; i < 4; i++)
        if (d[i]) (void)hipFree(d[i]);
    return rc;
}
