// ddgi_device.h — device-side math for the DDGI kernels (gfx950).
//
// Every function restates the reference GLSL with the same per-component
// evaluation order as the CPU oracle (oracle/ddgi_oracle.cpp), so that with
// -ffp-contract=off and ark_fmath.h the HIP path is bit-exact against it.
// Reference citations are on each function.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ark_fmath.h"
#include "../../include/ark_ddgi.h"
#include "ddgi_types.h"
#include "shading_math.h"

namespace ark {
namespace dev {

// fp16 storage (RNE, NaN canonicalised to 0x7e00 like the oracle)
__device__ __forceinline__ uint16_t f32_to_f16(float f)
{
    // The empty asm makes the fp32 value opaque: without it the backend may fuse
    // the producing fmul/fma with the conversion (v_mad_mix* rounds the exact
    // product to f16 once), which differs from fp32-then-f16 on fp16 ties.
    asm volatile("" : "+v"(f));
    if (f != f) return 0x7e00u;
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
}
__device__ __forceinline__ float f16_to_f32(uint16_t h) { return static_cast<float>(__builtin_bit_cast(_Float16, h)); }

} // namespace dev
} // namespace ark
