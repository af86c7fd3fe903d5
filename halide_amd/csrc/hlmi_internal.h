// hlmi_internal.h — shared plumbing between the runtime slice and the per-pipeline host shims.
// Nothing here is exported; the exported C ABI is declared in include/hlmi_runtime.h and
// include/hlmi_pipelines.h.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <optional>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include <utility>

#include "hlmi_pipelines.h"
#include "hlmi_runtime.h"

namespace hlmi {

// ---------------------------------------------------------------------------------------------
// errors: format a message, hand it to halide_error() (default handler aborts, like the reference's
// posix_error_handler.cpp:9-21) and return the code so callers can `return report(...)`.
int report(void *uc, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
int hip_failed(void *uc, hipError_t e, const char *what);  // -> halide_error_code_gpu_device_error

#define HLMI_HIP(uc, call)                                           \
    do {                                                             \
        hipError_t e__ = (call);                                     \
        if (e__ != hipSuccess) return ::hlmi::hip_failed(uc, e__, #call); \
    } while (0)

// ---------------------------------------------------------------------------------------------
// ABI helpers
constexpr uint32_t type_abi(int code, int bits) { return (uint32_t)code | ((uint32_t)bits << 8); }
constexpr uint32_t T_U8 = type_abi(1, 8), T_I8 = type_abi(0, 8), T_U16 = type_abi(1, 16), T_I16 = type_abi(0, 16),
                   T_I32 = type_abi(0, 32), T_U32 = type_abi(1, 32), T_F32 = type_abi(2, 32), T_F64 = type_abi(2, 64);
inline uint32_t buf_type_abi(const halide_buffer_t *b) {
    uint32_t v;
    memcpy(&v, &b->type, 4);
    return v;
}
const char *type_name(uint32_t abi, char tmp[16]);

// internal helpers that need no entry in the dynamic symbol table: the C ABI is what the library exports
#define HLMI_LOCAL __attribute__((visibility("hidden")))

struct BufArg {
    const char *name;
    halide_buffer_t *buf;
    uint32_t type;  // required element type (type_abi)
    int dims;       // required dimensionality
    bool is_output;
};

// ---------------------------------------------------------------------------------------------
// The argument table: the ONE place an entry point describes its arguments, one line each, in signature order.  The metadata
// RunGen reads (layout: src/runtime/HalideRuntime.h:1937-1975; contents as emitted by src/CodeGen_C.cpp:760-912), the BufArg
// array of the checks below, lens_blur's scalar ranges and the Python caller's argtypes all come from it.
struct Arg {
    const char *name;
    int32_t kind;       // halide_argument_kind_*
    uint32_t type;      // type_abi
    int32_t dims;       // 0 for scalars
    int n_est;          // buffers: 2 * dims (min, extent) estimates given, or 0
    int64_t est[8];
    unsigned has;       // scalars: bit DEF / MIN / MAX / EST set = sv[that] given
    halide_scalar_value_t sv[4];
    enum { DEF, MIN, MAX, EST };
    // stored as the argument's own type (lanes aside): a float, a double, a uint8, an int16, a uint16, a uint32, otherwise an int32
    Arg &set(int which, double v) {
        has |= 1u << which;
        const uint32_t t = type & 0xffffu;
        if (t == T_F32) sv[which].u.f32 = (float)v;
        else if (t == T_F64) sv[which].u.f64 = v;
        else if (t == T_U8) sv[which].u.u8 = (uint8_t)v;
        else if (t == T_I16) sv[which].u.i16 = (int16_t)v;
        else if (t == T_U16) sv[which].u.u16 = (uint16_t)v;
        else if (t == T_U32) sv[which].u.u32 = (uint32_t)v;
        else sv[which].u.i32 = (int32_t)v;
        return *this;
    }
    double get(int which) const {
        const uint32_t t = type & 0xffffu;
        return t == T_F32 ? (double)sv[which].u.f32 : t == T_F64 ? sv[which].u.f64 : t == T_U8 ? (double)sv[which].u.u8 :
               t == T_I16 ? (double)sv[which].u.i16 : t == T_U16 ? (double)sv[which].u.u16 : t == T_U32 ? (double)sv[which].u.u32 :
                            (double)sv[which].u.i32;
    }
    Arg &def(double v) { return set(DEF, v); }
    Arg &range(double lo, double hi) { return set(MIN, lo).set(MAX, hi); }
    Arg &estimate(double v) { return set(EST, v); }
};
// `est`: {min0, extent0, min1, extent1, ...} of the generator's set_estimates, or nothing where it declares none (ArgTable's
// constructor refuses a line whose count is neither 0 nor 2 * dims)
inline Arg make_arg(const char *name, int32_t kind, uint32_t type, int dims, std::initializer_list<int64_t> est = {}) {
    Arg a = {name, kind, type, dims, (int)est.size(), {}, 0, {}};
    std::copy_n(est.begin(), std::min<size_t>(est.size(), 8), a.est);
    return a;
}
inline Arg in_buf(const char *name, uint32_t type, int dims, std::initializer_list<int64_t> est = {}) {
    return make_arg(name, halide_argument_kind_input_buffer, type, dims, est);
}
inline Arg out_buf(const char *name, uint32_t type, int dims, std::initializer_list<int64_t> est = {}) {
    return make_arg(name, halide_argument_kind_output_buffer, type, dims, est);
}
inline Arg scalar_f32(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_F32, 0); }
inline Arg scalar_f64(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_F64, 0); }
inline Arg scalar_i32(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_I32, 0); }
inline Arg scalar_u8(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_U8, 0); }
inline Arg scalar_i16(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_I16, 0); }
inline Arg scalar_u16(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_U16, 0); }
inline Arg scalar_u32(const char *name) { return make_arg(name, halide_argument_kind_input_scalar, T_U32, 0); }

// One entry point's table and everything RunGen's structs point into, built once from the table and never per call.  Initialised
// dynamically (the pointers lead into the object itself), which no consumer can observe: tests/cpp/rungen_registration.cpp calls
// <name>_metadata() from a static initialiser of the EXECUTABLE, which runs after those of the library it links, and hlmi_rungen
// comes in through dlopen, which returns after them.
// The storage fits the table: three arrays of `n` entries made by the constructor and never resized, so the pointers RunGen's
// structs hold into them stay valid for the life of the table (resnet50 has 269 lines, most tables two or three).
struct HLMI_LOCAL ArgTable {
    int n = 0;
    using EstPtrs = const int64_t *[8];
    const std::unique_ptr<Arg[]> spec;
    const std::unique_ptr<halide_filter_argument_t[]> args;
    const std::unique_ptr<EstPtrs[]> est_ptrs;
    halide_filter_metadata_t md;   // version 1, kTargetString, `name`
    ArgTable(const char *name, std::initializer_list<Arg> table) : ArgTable(name, table.begin(), table.size()) {}
    ArgTable(const char *name, const Arg *table, size_t count);   // a table built at run time (resnet50's: generated names)
    ArgTable(const ArgTable &) = delete;   // (nor moved: args and md point into *this)
    // the same arguments under another entry point's name (the resize variants of one element type)
    halide_filter_metadata_t named(const char *name) const { return {md.version, md.num_arguments, md.arguments, md.target, name}; }
    // the table's buffer arguments, in table order, bound to the pointers the entry point received
    template<int N>
    void bufs(BufArg (&out)[N], halide_buffer_t *const (&ptrs)[N]) const {
        for (int i = 0, k = 0; i < n && k < N; i++) {
            const Arg &a = spec[i];
            if (a.kind != halide_argument_kind_input_scalar) out[k] = {a.name, ptrs[k], a.type, a.dims, a.kind == halide_argument_kind_output_buffer}, k++;
        }
    }
};

// <name>_argv from the signature of <name>: a pointer parameter takes a[i], any other parameter type P takes *(P *)a[i]
// (src/CodeGen_C.cpp:688-694), so the casts cannot disagree with the signature.
template<typename... P, size_t... I>
int argv_call(int (*fn)(P...), void **a, std::index_sequence<I...>) {
    auto arg = [](auto *tag, void *p) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if constexpr (std::is_pointer<T>::value) return (T)p;
        else return *(T *)p;
    };
    return fn(arg((P *)nullptr, a[I])...);
}
template<typename... P>
int argv_call(int (*fn)(P...), void **a) { return argv_call(fn, a, std::index_sequence_for<P...>{}); }

// The exported companions of entry point `name`: <name>_argv and <name>_metadata (`md`: a halide_filter_metadata_t, usually
// table.md), and with HLMI_ENTRY_AUTO also <name>_auto_schedule, a second name for the same function (the reference's drivers
// link both objects; an alias needs its target defined, which it is in the host pass only).
#define HLMI_ENTRY(name, md)                                                       \
    extern "C" int name##_argv(void **a) { return ::hlmi::argv_call(name, a); }    \
    extern "C" const halide_filter_metadata_t *name##_metadata(void) { return &(md); }
#if defined(__HIP_DEVICE_COMPILE__)
#define HLMI_ENTRY_AUTO(name, md) HLMI_ENTRY(name, md)
#else
#define HLMI_ENTRY_AUTO(name, md) \
    HLMI_ENTRY(name, md)          \
    extern "C" __typeof__(name) name##_auto_schedule __attribute__((alias(#name)));
#endif

// ---------------------------------------------------------------------------------------------
// The entry prologue.  The reference emits its argument checks in a fixed order (src/AddImageChecks.cpp:716-760,
// reverse of the prepend order; buffers in the order of a std::map keyed by buffer name, i.e. alphabetical):
//   0. null buffer arguments, in signature order                       (src/UnpackBuffers.cpp:148)          -12
//   1. scalar parameter ranges                                           (src/AddParameterChecks.cpp)         -9 / -10
//   2. bounds-query mode: rewrite the query buffers, return 0            (:709-713)
//   3. per buffer: type, then dimensionality                             (asserts_type_checks, :329-347)      -3 / -43
//   4. per buffer, per dimension: stride / min / extent constraints      (asserts_constrained, :621-645)      -8
//   5. per buffer, per dimension: required region, then extent >= 0      (asserts_required, :414-418, :466-470) -4 / -28
//   6. per buffer, per dimension: |extent * stride| and the running product of extents <= 2^31 - 1
//                                                                        (dims_no_overflow_asserts, :436-462) -5 / -6
//   7. host pointer alignment (set_host_alignment)                       (asserts_host_alignment, :688-692)   -24
//   8. host pointers                                                     (asserts_host_non_null, :648-655)    -34
// The pipelines call the check_* helpers below in whatever order is convenient for them; failures of phases 4-7 are
// not reported on the spot but RECORDED with their (phase, buffer rank, dimension, kind) key, and the one the
// reference would have hit first is reported by checks_done() — which acquire_device() calls, so no kernel is ever
// enqueued with unchecked arguments.  tests/test_entry_protocol.py pins the codes and the order.
// An entry point fills its BufArg array from its table (ArgTable::bufs), runs the checks in its own order — check_shapes and
// check_scalar_ranges are the loops several of them share — and ends the prologue with to_device().
// step 0; also (re)starts the recording for this call and ranks the buffers by name
int check_not_null(void *uc, const BufArg *args, int n);
// step 2 (src/AddImageChecks.cpp:315-318, HalideRuntime.h:1851-1853)
bool any_bounds_query(const BufArg *args, int n);
// step 3, reported immediately (everything after it indexes dim[]).  In bounds-query mode the reference skips the
// type check and rewrites type and dimensions of the query buffers (BufferBuilder, :478-494): here a query buffer gets
// its type rewritten too, but a wrong dimensionality stays an error (-43) — writing dim[] entries the caller did not
// provide is not something a drop-in should copy.
int check_type_and_dims(void *uc, const BufArg *args, int n);
// steps 4-6 for one buffer: dim[0].stride == 1 (src/Parameter.cpp:30-35), extents >= 0, sizes < 2^31.  Always
// returns 0 (recorded).
int check_shape(void *uc, const BufArg &a);
HLMI_LOCAL int check_shapes(void *uc, const BufArg *args, int n);   // every buffer, in array order
// step 1: the min / max the table's scalar lines declare, if any; `values` are the scalars the entry point received, in table
// order like ArgTable::bufs' pointers
HLMI_LOCAL int check_scalar_ranges(void *uc, const ArgTable &t, std::initializer_list<double> values);
// step 5: [min, min+extent) of dimension d must cover [req_min, req_min+req_extent)
// (src/AddImageChecks.cpp:393-418 -> halide_error_access_out_of_bounds).  Always returns 0 (recorded).
int check_covers(void *uc, const BufArg &a, int d, int req_min, int req_extent);
// step 4, a pinned constraint "<buffer>.<field>.<dim> == expect" (halide_error_constraint_violated,
// src/runtime/errors.cpp:104); `what` must start with the buffer's name.  Always returns 0 (recorded).
int check_equal(void *uc, const char *what, int val, const char *expect_what, int expect);
// step 7: the buffer's host pointer is a multiple of `alignment` bytes (halide_error_unaligned_host_ptr, src/runtime/errors.cpp:187);
// a null host pointer passes (0 % alignment == 0) and is step 8's business.  Always returns 0 (recorded).
HLMI_LOCAL int check_host_aligned(void *uc, const BufArg &a, int alignment);
// report the recorded failure the reference would have hit first (0 if none) and forget the rest
int checks_done(void *uc);
// bounds-query answer: rewrite dim[] to a dense planar shape (stride[0]=1) — only if `buf` is itself
// a query buffer (host==NULL && device==0), as the reference does (AddImageChecks.cpp:480-497).
void answer_query(halide_buffer_t *buf, const int *mins, const int *extents);

// ---------------------------------------------------------------------------------------------
// device context
struct DeviceCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    // Held from acquire_device() until the context goes out of scope at the end of the entry point: calls that share
    // a (device, stream) — and therefore its scratch arena — enqueue their launches one call at a time, so that stream
    // order alone makes the shared arena safe when several host threads call pipelines concurrently (the reference's
    // generated code is re-entrant, test/generator/gpu_multi_context_threaded_aottest.cpp).  Threads that want their
    // calls to overlap on the GPU use distinct streams (halide_hip_set_stream).
    std::unique_lock<std::recursive_mutex> call_lock;
};
// choose device (halide_set_gpu_device / HL_GPU_DEVICE / 0), hipSetDevice, choose stream.
// Fails with -29 when no gfx950 device is usable: there is NO CPU fallback.
// `lock` = take the stream's call lock (pipeline entry points do; copies, syncs and allocations do not: they never
// touch the scratch arena, and holding the lock across a blocking wait would stall every other caller of the stream).
// Reports the failure recorded by the check_* helpers first, if there is one.
int acquire_device(void *uc, DeviceCtx *ctx, bool lock = true);
// scratch arena owned by (device, stream); contents valid until the next call that asks for a
// workspace on the same stream (stream order makes reuse across back-to-back calls safe).
int get_workspace(void *uc, const DeviceCtx &ctx, size_t bytes, void **ptr);

// dirty-flag protocol for pipeline arguments (src/InjectHostDevBufferCopies.cpp:197-217,285-304)
int input_to_device(void *uc, const DeviceCtx &ctx, const BufArg &a);
int output_on_device(void *uc, const DeviceCtx &ctx, const BufArg &a);
// acquire_device, then input_to_device for every input and output_on_device for every output, each in array order
HLMI_LOCAL int to_device(void *uc, DeviceCtx *ctx, const BufArg *args, int n);
void mark_output_written(halide_buffer_t *buf);  // device_dirty = 1, host_dirty = 0
// A number that changes whenever the device contents of `buf` may have changed through this runtime (upload of a
// host-dirty buffer, use as a pipeline output or copy target, re-allocation); unique across allocations, so
// (device handle, version) identifies contents.  0 = memory this runtime does not own (wrapped native pointers: their
// owner can rewrite them behind our back) — callers must not cache anything derived from such a buffer.
uint64_t buffer_version(const halide_buffer_t *buf);
// compute units a launch on `stream` is sized for (a frame-queue stream of halide_hip_partition_stream: its 1 / nparts share)
int stream_cu_count(int device, hipStream_t stream);

// Bounds-query helpers.  A buffer takes part in deriving the other buffers' regions when it is real (host or device set) or,
// in query mode, when the caller gave it a shape: RunGen's queries pass EVERY buffer with host == device == 0 — outputs shaped
// by --output_extents / the estimates / the first input, inputs shaped as loaded (tools/RunGen.h:1212-1250) — and Halide's
// bounds inference takes the outputs' shapes as the request whether or not they are allocated.
inline bool buffer_is_real(const halide_buffer_t *b) { return !(b->host == nullptr && b->device == 0); }
inline bool buffer_has_shape(const halide_buffer_t *b) {
    for (int d = 0; d < b->dimensions; d++)
        if (b->dim[d].extent <= 0) return false;
    return b->dimensions > 0;
}
inline bool buffer_known(const halide_buffer_t *b) { return buffer_is_real(b) || buffer_has_shape(b); }

// ---- events across streams.  The special stream handles (NULL, hipStreamLegacy — which callers on torch's default stream pass
// to halide_hip_set_stream — and hipStreamPerThread) launch kernels fine, but they are not safe partners for events in ROCm
// 7.2: an event RECORDED on hipStreamLegacy crashes the next hipStreamWaitEvent on it (scripts/legacy_event_probe.py), and
// one recorded on the NULL handle and waited for from several host threads at once threw std::bad_variant_access inside the
// runtime (tests/test_torch_ops.py followed by tests/test_threads.py).  So no event ever names a special stream: work on one
// is waited for on the host, which leaves the event in its "nothing pending" state.
inline bool stream_is_special(hipStream_t s) { return s == nullptr || s == hipStreamLegacy || s == hipStreamPerThread; }
// "everything enqueued on `producer` so far" as an event other streams can wait for
inline hipError_t record_done(hipEvent_t ev, hipStream_t producer) {
    if (stream_is_special(producer)) return hipStreamSynchronize(producer == hipStreamLegacy ? nullptr : producer);
    return hipEventRecord(ev, producer);
}
// whatever is enqueued on `consumer` from now on happens after `ev`
inline hipError_t wait_done(hipStream_t consumer, hipEvent_t ev) {
    if (stream_is_special(consumer)) return hipEventSynchronize(ev);
    return hipStreamWaitEvent(consumer, ev, 0);
}
// timing events only (never waited for by a stream): hipStreamLegacy is the NULL stream
inline hipStream_t event_stream(hipStream_t s) { return s == hipStreamLegacy ? nullptr : s; }

template<typename T>
inline T *dev_ptr(const halide_buffer_t *b) { return reinterpret_cast<T *>((uintptr_t)b->device); }

// ---- cache of derived device data: small results of a producing launch that are a function of a key only (the remap table of
// local_laplacian, the set-up block of camera_pipe, the re-ordered bf16 filter of conv_layer_bf16), kept in memory of their own
// so that a call with a known key skips the launch.  One instance per pipeline, each with its own lock and a fixed number of
// slots, least recently used replaced first.  An entry is read by the launches of every call that hits it, on whatever stream
// that call runs: the entry therefore remembers its reader streams, and whoever re-fills or evicts the entry first records an
// event behind everything those streams hold and orders its own stream behind all of them (or waits for the whole device where
// a stream is a caller's, which may be gone by then).  DESIGN.md section 1 has the invariants.
constexpr int DERIVED_SLOTS = 8, DERIVED_READERS = 4;
constexpr size_t DERIVED_KEY_BYTES = 96;
struct DerivedEntry {
    unsigned char key[DERIVED_KEY_BYTES];
    size_t key_bytes = 0;          // 0: matches nothing
    int device = -1;
    size_t bytes = 0;
    void *ptr = nullptr;
    hipStream_t stream = nullptr;  // stream the producer ran on
    hipEvent_t ready = nullptr;    // recorded behind the producer
    struct Reader {
        hipStream_t s = nullptr;
        hipEvent_t done = nullptr;
        bool live = false;
    } readers[DERIVED_READERS];
    bool overflow = false;         // more reader streams than slots: fall back to a device-wide wait
    int pins = 0;                  // calls between their cache hit and the enqueue of their last reading launch: not evictable meanwhile
    uint64_t used = 0;
};
struct DerivedCache {
    const int capacity;            // slots in use, <= DERIVED_SLOTS
    std::mutex mu;
    DerivedEntry slots[DERIVED_SLOTS];
    uint64_t clock = 0;
    explicit DerivedCache(int n) : capacity(n) {}
};
// A use of an entry by one call.  A cache HIT pins its entry (not evictable, not re-fillable) and lets go of the cache lock at
// once — concurrent callers (the per-device workers of hlmi_run_batch, multi-stream hosts) enqueue their launches side by side;
// done() — called after the last launch that reads `ptr` has been enqueued — takes the lock again for a moment, records this
// stream as a reader and unpins.  A MISS keeps the lock from the choice of the slot until done(): the entry is being (re)filled.
struct DerivedUse {
    void *ptr = nullptr;             // null: not cached — the caller produces into memory of its own (its workspace)
    bool fill = true;                // the caller has to enqueue the producing launch on its stream first, then call filled()
    void filled(hipStream_t s);      // the producer has been enqueued on s
    void done(hipStream_t s);        // every launch of this call that reads ptr has been enqueued on s
    ~DerivedUse();                   // the call bailed out between derived_acquire() and done()

    std::unique_lock<std::mutex> lock;   // (which also keeps a use from being copied)
    DerivedCache *cache = nullptr;
    DerivedEntry *entry = nullptr;
    bool pinned = false;
};
// `key` is compared as `key_bytes` (<= DERIVED_KEY_BYTES) opaque bytes: callers zero their key struct first and put the device in it.
// !cacheable, or every slot pinned by a concurrent call: nothing is touched, use->ptr == nullptr and use->fill.
int derived_acquire(void *uc, const DeviceCtx &ctx, DerivedCache &c, const void *key, size_t key_bytes, size_t bytes, bool cacheable,
                    DerivedUse *use);

// ---------------------------------------------------------------------------------------------
// optional per-kernel HIP-event timing (include/hlmi_runtime.h: hlmi_kernel_timing_*)
bool timing_enabled();
void timing_begin(const char *name, hipStream_t s);
void timing_end(hipStream_t s);
// declares the ALGORITHMIC bytes (compulsory reads + writes) of the next timed launch of this thread
void timing_note_bytes(double bytes);
struct ScopedKernelTimer {
    hipStream_t s;
    bool on;
    ScopedKernelTimer(const char *name, hipStream_t stream) : s(stream), on(timing_enabled()) {
        if (on) timing_begin(name, s);
    }
    ~ScopedKernelTimer() {
        if (on) timing_end(s);
    }
};
// Run-time switches (HLMI_*): two helpers so that every switch reads the same way.  env_int: unset or empty = nullopt (the caller's
// default), otherwise atoi of the value.  env_flag: env_int(name).value_or(0) != 0 — set and non-zero = on, unset / empty / "0" = off.
// Read at every call (a getenv, ~100 ns): the parity tests flip switches inside one process to reach the alternative paths.
HLMI_LOCAL std::optional<int> env_int(const char *name);   // hidden: the library's exported symbols stay as they were
bool env_flag(const char *name);
// launch + error check; kernel errors surface as -23 (device_run_failed)
int launch_failed(void *uc, const char *kernel);
// measurement only (hlmi_kernel_timing_only): while a launch name is selected every OTHER launch is skipped, so that a
// caller can run one kernel of a chain back to back (its inputs are whatever earlier, complete calls left in the workspace)
bool launch_selected(const char *name);
#define HLMI_LAUNCH(uc, name, stream, kernel, grid, block, shmem, ...)                      \
    do {                                                                                    \
        if (!::hlmi::launch_selected(name)) break;                                          \
        ::hlmi::ScopedKernelTimer t__(name, stream);                                        \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                \
        if (hipGetLastError() != hipSuccess) return ::hlmi::launch_failed(uc, name);        \
    } while (0)

// Run-time flags to template arguments, once: calls f(std::true_type / std::false_type ...) — one per flag, in order — and returns
// what it returns.  f is a generic lambda that names the kernel instantiation (`kernel<A.value, B.value>`); all 2^n are instantiated.
// HLMI_LAUNCH inside f returns from f on a failed launch, so f ends in `return 0` and the caller forwards the code.  Host only.
template<typename F>
int with_flags(F &&f) { return f(); }
template<typename F, typename... Bs>
int with_flags(F &&f, bool b, Bs... rest) {
    return b ? with_flags([&](auto... t) { return f(std::true_type{}, t...); }, rest...)
             : with_flags([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}

// ---------------------------------------------------------------------------------------------
extern const char *const kTargetString;  // "x86-64-linux-hip-gfx950" (canonical-style target string)

// conv_layer.hip: argument table and protocol shared by conv_layer and conv_layer_bf16; the table's estimates are those of an
// N x W x H output with 128 -> 128 channels
HLMI_LOCAL ArgTable conv_arg_table(const char *name, int w, int h, int n);
int conv_check_args(void *uc, BufArg *args, int *CI, int *CO, int *W, int *H, int *N, bool *query);

// resize.hip: the named resize variant ("resize_cubic_uint8_down", ...) on its general two-launch path whatever the sizes, for the
// tests (fused == general bit for bit) and for bench_apps.py (fused is not slower).  Per call: no mode is kept anywhere.
extern "C" int hlmi_resize_general(const char *variant, halide_buffer_t *input, float scale_factor, halide_buffer_t *output);

// gaussian_blur.hip: the named blur ("gaussian_blur_direct", "gaussian_blur_3_2_8", ...) with its blur passes on the path that
// has no size conditions (every tap read from global memory with its clamp), for the tests (tiled == general bit for bit) and for
// bench_apps.py.  Per call: no mode is kept anywhere.
extern "C" int hlmi_gaussian_blur_general(const char *variant, halide_buffer_t *input, float sigma, int32_t trunc, halide_buffer_t *output);

// linear_blur.hip: "linear_blur" or "simple_blur" as the unfused composition (to_linear over the required region into the scratch
// arena, one thread per output with nine clamped taps from global memory, to_srgb in place: three launches, one for simple_blur),
// for the tests (fused == general bit for bit) and for bench_apps.py.  linear_blur does not read width and height.  Per call: no
// mode is kept anywhere.
extern "C" int hlmi_linear_blur_general(const char *name, halide_buffer_t *input, int32_t width, int32_t height, halide_buffer_t *output);

// wavelet.hip: "haar_x", "inverse_haar_x", "daubechies_x" or "inverse_daubechies_x" with one thread per output and every tap a
// clamped scalar load from global memory, for the tests (default == general bit for bit) and for bench_apps.py.  Per call: no mode
// is kept anywhere.
extern "C" int hlmi_wavelet_general(const char *name, halide_buffer_t *in, halide_buffer_t *out);

// reaction_diffusion.hip: "reaction_diffusion_init" (reads `out`), "reaction_diffusion_update" (state, mouse_x, mouse_y, frame, out),
// "reaction_diffusion_render" (state, render) or "run" (hlmi_reaction_diffusion_run's arguments, out = new_state) with one thread per
// output, every tap a clamped load from global memory and, for "run", one launch per step and a separate render, for the tests
// (default == general bit for bit) and for bench_apps.py.  Arguments a name does not read are ignored.  Per call: no mode is kept.
extern "C" int hlmi_reaction_diffusion_general(const char *name, halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame, int32_t steps,
                                               halide_buffer_t *out, halide_buffer_t *render);

// compositing.hip: the same call with one thread per pixel and byte loads, written from the operator table of hlmi_pipelines.h, for
// the tests (default == general bit for bit) and for bench_apps.py.  Per call: no mode is kept anywhere.
extern "C" int hlmi_compositing_general(halide_buffer_t *layer_rgba_0, halide_buffer_t *layer_rgba_1, halide_buffer_t *layer_rgba_2,
                                        halide_buffer_t *layer_rgba_3, halide_buffer_t *layer_rgba_4, halide_buffer_t *layer_rgba_5,
                                        halide_buffer_t *ops, halide_buffer_t *output);
// compositing.hip, test hook: fn 0 = the device's normalise quotient of (numerator a[i], alpha b[i]) before the saturation, fn 1 =
// the device's scale16(a[i], b[i]); host pointers to n elements.  Returns 0, < 0 = HIP error.
extern "C" int hlmi_debug_compositing(int fn, const uint16_t *a, const uint8_t *b, uint16_t *out, size_t n);

// hexagon_benchmarks.hip: "conv3x3a16", "conv3x3a32", "dilate3x3", "median3x3", "gaussian5x5" or "sobel" with one thread per output
// pixel and its 9 (25) clamped taps read from global memory, the arithmetic in the contract's own types, for the tests (default ==
// general bit for bit) and for bench_apps.py.  `mask` is read by the two conv3x3 filters only and may be null for the others.  Per
// call: no mode is kept anywhere.
extern "C" int hlmi_hexagon_benchmarks_general(const char *name, halide_buffer_t *input, halide_buffer_t *mask, halide_buffer_t *output);

// mat_mul.hip: the generator instantiated at another `size` (1 .. 8192; mat_mul is hlmi_mat_mul_sized(1024, ...)): the same shim,
// plan and rules, every buffer [0, size) x [0, size).  -8 for a size outside the range.
extern "C" int hlmi_mat_mul_sized(int32_t size, halide_buffer_t *A, halide_buffer_t *B, halide_buffer_t *out);
// mat_mul.hip: the same call with one thread per output running a plain fmaf loop, for the tests (default == general bit for bit)
// and for bench_apps.py.  Per call: no mode is kept anywhere.
extern "C" int hlmi_mat_mul_general(int32_t size, halide_buffer_t *A, halide_buffer_t *B, halide_buffer_t *out);

// linear_algebra.hip (body: general_entry of linear_algebra_core.h): the named entry point ("halide_sdot", "halide_sgemm_transA", ...) with one thread per output running the chain
// as written, for the tests (default == general bit for bit) and for bench_apps.py.  p0 .. p3: the entry point's buffers in its own
// order, the unused trailing ones null; a and b are read where the entry point has them.  Per call: no mode is kept anywhere.
extern "C" int hlmi_linear_algebra_general(const char *name, float a, float b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                                           halide_buffer_t *p3);
// linear_algebra_f64.hip: the same general_entry for the twelve f64 entry points ("halide_ddot", "halide_dgemm_transA", ...)
extern "C" int hlmi_linear_algebra_general_f64(const char *name, double a, double b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                                               halide_buffer_t *p3);

// fft.hip: the fft generator instantiated at other sizes and gains (fft_forward_c2c is hlmi_fft2d(0, 16, 16, 1 / 256, ...)): the same
// shim, plan and rules.  kind: 0 c2c forward, 1 c2c inverse, 2 r2c, 3 c2r; N0, N1 in 2 .. 4096 with radix factors 8, 6, 4, 2 only, both
// even for r2c and c2r; -8 for any other size.
extern "C" int hlmi_fft2d(int32_t kind, int32_t N0, int32_t N1, float gain, halide_buffer_t *input, halide_buffer_t *output);
// fft.hip: the same call with one thread per 1-D line (per zipped column pair), every pass in full through the scratch arena, for the
// tests (default == general bit for bit) and for bench_apps.py.  Per call: no mode is kept anywhere.
extern "C" int hlmi_fft2d_general(int32_t kind, int32_t N0, int32_t N1, float gain, halide_buffer_t *input, halide_buffer_t *output);
// fft.hip: the host function behind every twiddle table (the checker builds its tables with it too), radix_factor and the size predicate
extern "C" void hlmi_fft_twiddles(int32_t n, int32_t sign, float gain, float *out);
extern "C" int hlmi_fft_radix_factor(int32_t N, int32_t *R);
extern "C" int hlmi_fft_size_ok(int32_t N);

// resnet50.hip: the same call in argv form (269 halide_buffer_t *) with every convolution on the one-thread-per-output kernel, for the
// tests (default == general bit for bit) and for scripts/resnet50_times.py.  Per call: no mode is kept anywhere.
extern "C" int hlmi_resnet50_general(void **argv);
// resnet50.hip: ONE convolution layer of any shape through the network's plan predicate and kernels.  input [CI, W, H], weights
// [CO, KW, KH, CI], the four per-channel vectors [CO], output (and residual) [CO, OW, OH] with compute_shape's extents; every min 0 (-8).
// mode: 0 the raw chain, 1 normalise and scale, 2 + ReLU, 3 + residual + ReLU; residual is looked at in mode 3 only and may be null
// otherwise.  general_only != 0: the one-thread-per-output kernel.
extern "C" int hlmi_debug_resnet50_layer(halide_buffer_t *input, halide_buffer_t *weights, halide_buffer_t *gamma, halide_buffer_t *beta, halide_buffer_t *mu,
                                         halide_buffer_t *sig, halide_buffer_t *residual, int32_t stride, int32_t pad, int32_t mode, int32_t general_only,
                                         halide_buffer_t *output);
// resnet50.hip: the max pool (k x k window) and the tail (mean over W x H, fc with weights [N, C] and bias [N], softmax) at any size
extern "C" int hlmi_debug_resnet50_maxpool(halide_buffer_t *input, int32_t k, int32_t stride, int32_t pad, halide_buffer_t *output);
extern "C" int hlmi_debug_resnet50_tail(halide_buffer_t *input, halide_buffer_t *fc_weights, halide_buffer_t *fc_bias, halide_buffer_t *output);
// resnet50.hip, the batched siblings (resnet50_batch is a library extension: the reference has no such generator).  The whole call on the
// general kernel; the layer hook over N images, input [CI, W, H, N], residual and output [CO, OW, OH, N], with `variant` 0 = the plan's
// choice, 1 = the general kernel, 2 = the 64 x 64 MFMA tile, 3 = the 64 x 128 one, anything else -8; the pool hook [C, W, H, N] ->
// [C, OW, OH, N]; the tail hook [C, W, H, N] -> [classes, N].
extern "C" int hlmi_resnet50_batch_general(void **argv);
extern "C" int hlmi_debug_resnet50_layer_batch(halide_buffer_t *input, halide_buffer_t *weights, halide_buffer_t *gamma, halide_buffer_t *beta,
                                               halide_buffer_t *mu, halide_buffer_t *sig, halide_buffer_t *residual, int32_t stride, int32_t pad, int32_t mode,
                                               int32_t variant, halide_buffer_t *output);
extern "C" int hlmi_debug_resnet50_maxpool_batch(halide_buffer_t *input, int32_t k, int32_t stride, int32_t pad, halide_buffer_t *output);
extern "C" int hlmi_debug_resnet50_tail_batch(halide_buffer_t *input, halide_buffer_t *fc_weights, halide_buffer_t *fc_bias, halide_buffer_t *output);
// resnet50.hip, no device needed: the 57 launches of the first run of a batch of n_images >= 1 images (min(n_images, *chunk) of them) as steps[57][5] = (launch: 0
// resnet50_conv_mfma, 1 resnet50_conv_general, 2 resnet50_maxpool, 3 resnet50_avgpool, 4 resnet50_fc, 5 resnet50_softmax, 6
// resnet50_conv_mfma_wide; grid x; grid y; tile co; tile pixels) and *chunk = the images per run in force.  Returns the step count.
extern "C" int hlmi_debug_resnet50_batch_plan(int32_t n_images, int32_t general_only, int32_t *chunk, int32_t *steps);

// hannk_conv.hip: the named entry point of apps/hannk's op library ("tile_conv_filter_uint8", "conv_u8_u8_u8", "conv_u8_u8_i16",
// "depthwise_conv_uint8", "depthwise_conv_broadcast_uint8", "depthwise_conv_shallow_uint8") in argv form with one thread per output running the contract's loops as
// written, for the tests (default == general byte for byte) and for bench_apps.py.  -1 for an unknown name.  Per call: no mode is
// kept anywhere.
extern "C" int hlmi_hannk_general(const char *name, void **argv);
// hannk_conv.hip, test hook: the device's epilogue alone on host arrays of n elements: fn 0 = quantize_i16 (out: int16_t[n]; zero, lo
// and hi are not read), fn 1 = quantize_and_relu_u8 (out: uint8_t[n]).  Returns 0, < 0 = HIP error.
extern "C" int hlmi_debug_hannk_quantize(int fn, const int32_t *acc, size_t n, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi,
                                         void *out);
// hannk_conv.hip: what conv_*'s plan chooses for `npix` output pixels, `channels` output channels and `quads` = fw * fh * ci / 4 on
// `cus` compute units with aligned operands: out = {1 if the MFMA kernel runs, k splits (1 = none), wave tiles}.  The switch
// HLMI_HANNK_SPLIT_K (unset = the plan's choice, n >= 1 = that many splits where the k blocks allow) is read like in a call.
extern "C" int hlmi_debug_hannk_conv_plan(int64_t npix, int32_t channels, int32_t quads, int32_t cus, int32_t *out);

// hannk_nn.hip: the seven further ops of the library ("average_pool_uint8", "max_pool_uint8", "mean_uint8", "add_uint8_uint8",
// "mul_uint8_uint8_uint8", "softmax_uint8", "l2_normalization_uint8") with one thread per output: what hlmi_hannk_general forwards
// the names it does not know to.  -1 for an unknown name.
HLMI_LOCAL int hannk_nn_general(const char *name, void **argv);
// hannk_nn.hip, test hook: the device's approx_* helpers (hannk_math.h) alone over host arrays of n int32 arguments, one launch.
// fn 0 = approx_log2(q, x, q_x, Int(bits)), 1 = approx_exp2(q, x, q_x, Int(bits)) of an i32 x, 2 = approx_reciprocal(q, x, Int(bits)),
// 3 = approx_reciprocal_sqrt(q, x, Int(bits)); bits is 16 or 32; out: int32_t[n].  Returns 0, -1 = bad argument, < -1 = HIP error.
extern "C" int hlmi_debug_hannk_approx(int fn, int32_t q, const int32_t *x, size_t n, int32_t q_x, int32_t bits, int32_t *out);

// hannk_program.hip: the elementwise programs and the data movers ("elementwise_5xuint8_1xuint8", "elementwise_5xint16_1xuint8int16",
// "copy_uint8_uint8", "fill_uint8", "upsample_channels_uint8") with one thread per output: what hannk_nn_general forwards the names it
// does not know to.  -1 for an unknown name.
HLMI_LOCAL int hannk_program_general(const char *name, void **argv);
// hannk_program.hip, test hook: the device's approx_log2p1_exp2 (fn 0), approx_log2m1_exp2 (1), approx_logistic (2) and approx_tanh (3)
// of hannk_math.h in Int(16), over host arrays of n elements: x the i16 argument, q the result's precision, q_x the argument's, each as
// int32; width 16 or 32 is the width of the count q_x; out: int32_t[n].  One launch.  Returns 0, -1 = bad argument,
// < -1 = HIP error.
extern "C" int hlmi_debug_hannk_program_approx(int fn, const int32_t *x, const int32_t *q, const int32_t *q_x, size_t n, int32_t width, int32_t *out);

// hannk_move.hip: the movement the interpreter does with Buffer::copy_from, as library extensions without argument table, _argv or _metadata.
// hlmi_hannk_copy_from: Halide::Runtime::Buffer::copy_from: same rank (<= 8) and element size (1, 2, 4, 8 bytes), the intersection of the two
// boxes, any strides on either side.  A dst whose distinct indices share an element through a stride of 0 is refused (-8); no other
// overlap of dst with itself (strides (1, 1), a row stride below the row's extent) is looked for: such a dst is the caller's error and its
// elements end up holding any one of the values written to them.  hlmi_hannk_gather: GatherOp::execute with batch_dims == 0, indices int32 of
// rank 0 .. 2; an index outside the source's dimension `axis` leaves its slice of dst unwritten and the call returns -8.
extern "C" int hlmi_hannk_copy_from(const halide_buffer_t *src, halide_buffer_t *dst);
extern "C" int hlmi_hannk_gather(const halide_buffer_t *src, const halide_buffer_t *indices, int axis, halide_buffer_t *dst);
// "hannk_copy_from" (argv: src, dst) and "hannk_gather" (argv: src, indices, &axis, dst) with one thread per element: what hannk_program_general
// forwards the names it does not know to.  -1 for an unknown name.
HLMI_LOCAL int hannk_copy_general(const char *name, void **argv);
// hannk_move.hip, no device needed: what copy_from's plan chooses for two buffers (only type, dimensions and dim[] are read): out = {kernel:
// 0 nothing to copy, 1 rows, 2 transposing, 3 general; dimensions left after dropping and merging}.  general != 0: as under hlmi_hannk_general.
// Returns 0, -1 = bad argument, -8 = dst aliases itself.
extern "C" int hlmi_debug_hannk_move_plan(const halide_buffer_t *src, const halide_buffer_t *dst, int32_t general, int32_t *out);

inline int floor_div(int a, int b) {  // b > 0 ; Halide integer division rounds toward -inf (src/IR.h:145-166)
    int q = a / b, r = a % b;
    return (r != 0 && r < 0) ? q - 1 : q;
}

}  // namespace hlmi
