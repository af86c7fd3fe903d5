// hlmi_random.h — Halide::random_float / random_int restated once, for host and device: a pure integer hash of its argument list
// (src/Random.cpp:14-98; paths relative to the reference).
//   rng32(x)       = (C2 x + C1) x + C0 in uint32, a permutation polynomial                          src/Random.cpp:15-17, 59-62
//   random_int(e)  = r = rng32(e[0]); r = rng32(r + e[i]) for every further argument; r ^ (r >> 16)  src/Random.cpp:66-90
//   random_float   = bits((127 << 23) | (r >> 9)) - 1.0f, clamped to [0, 1]                           src/Random.cpp:92-98
// The argument list of a call is [seed if given, call id, definition tag, the definition's free variables in REVERSE order]:
// random_float(seed) makes Call::random {seed, id} with id = random_number_counter++ (src/IROperator.cpp:2873-2889), and the
// Func definition that holds the call appends [free variables ..., tag] reversed (LowerRandom, src/Random.cpp:105-137) with tag =
// random_variable_counter++ (src/Function.cpp:640 for a pure definition, :883 for an update, whose free variables are its remaining
// pure arguments and its reduction variables, :866-882).  Both counters restart per compiled module (src/Module.cpp:865, 932).
// A pipeline that calls random_float keeps its (id, tag) pairs in ONE named table beside its kernels; the arguments are folded in
// with random_begin / random_next in list order and finished with random_float_end.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HLMI_HD __host__ __device__ __forceinline__
#else
#define HLMI_HD inline
#endif

namespace hlmi {
namespace rnd {

constexpr uint32_t C0 = 576942909u, C1 = 1121052041u, C2 = 1040796640u;

HLMI_HD uint32_t rng32(uint32_t x) { return (C2 * x + C1) * x + C0; }
HLMI_HD uint32_t random_begin(uint32_t e0) { return rng32(e0); }
HLMI_HD uint32_t random_next(uint32_t r, uint32_t e) { return rng32(r + e); }
HLMI_HD uint32_t random_int_end(uint32_t r) { return r ^ (r >> 16); }
HLMI_HD float random_float_end(uint32_t r) {
    const uint32_t bits = (127u << 23) | (random_int_end(r) >> 9);
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(bits);
#else
    memcpy(&f, &bits, 4);
#endif
    f = f - 1.0f;
    const float m = f < 1.0f ? f : 1.0f;   // clamp(v, 0, 1) = max(min(v, 1), 0): never active, kept as written
    return m > 0.0f ? m : 0.0f;
}

}  // namespace rnd
}  // namespace hlmi
