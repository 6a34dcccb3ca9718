// refl_denoise_host.h — the host side of the reflection denoiser passes
// (ark_ddgi_rt_reflections_denoise): the entry's argument checks and a serial restatement of
// the four passes that walks the image tile by tile and lane by lane through refl_denoise.h,
// the functions the kernels call. Host only, no HIP (also built on its own, tests/cpp).
#pragma once

#include <stdint.h>

#include "../../include/ark_ddgi.h"
#include "refl_denoise.h"

namespace ark {
namespace refl {

// What ark_ddgi_rt_reflections_denoise refuses about a descriptor of the right struct_size
// (null: nothing): a non-finite matrix or scalar, z_near == z_far, width * height >= 2^28,
// and, unless the image is empty, a null plane, a plane that is not aligned to its texel
// (8 bytes RGBA16F, 4 bytes otherwise) and two planes whose byte ranges overlap. The
// pointers are compared, never followed.
const char* descProblem(const ArkReflDenoiseDesc& d);

Args argsOf(const ArkReflDenoiseDesc& d);

// The passes over host planes, whole image each, in the node's order.
void hostHistoryCopy(const Args& a, bool firstCopy);
void hostReproject(const Args& a);
void hostPrefilter(const Args& a);
void hostResolveTemporal(const Args& a);

// ark_ddgi_rt_reflections_denoise with host pointers. Returns 0, or -1 for what descProblem refuses.
int hostDenoise(const ArkReflDenoiseDesc& d);

} // namespace refl
} // namespace ark
