// refl_denoise_test.cpp — csrc/refl_denoise_host.cpp on its own (tests/test_refl_denoise_sanitizers.py
// builds both with -fsanitize=address,undefined): the host restatement of the reflection
// denoiser passes over random planes at 1 x 1, 1 x 97, 8 x 8, 9 x 7 and 29 x 19, a first
// frame and a following one, motion vectors and ray lengths that send the reprojection UVs
// far outside [0, 1] (the repeat wrap, the slow path's texel coordinates), an all-sky
// plane, inf and NaN radiance, and the refusals. Every plane lies between guard words,
// which must survive. It also prints the error of exp and pow(x, 512) against glibc.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "refl_denoise.h"
#include "refl_denoise_host.h"
#include "../../include/ark_ddgi_debug.h"

using namespace ark;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++failures;                                      \
        }                                                    \
    } while (0)

static const float kIdentity[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
// a perspective-like inverse projection (w = 1 - 0.9 z) and a previous view shifted sideways
static const float kUnproject[16] = { 0.6f, 0, 0, 0, 0, 0.4f, 0, 0, 0, 0, 0, -0.9f, 0, 0, -1, 1 };
static const float kPrevView[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.05f, -0.02f, 0, 1 };
static const float kPrevProj[16] = { 1.6f, 0, 0, 0, 0, 2.4f, 0, 0, 0, 0, -1.001f, -1, 0, 0, -0.1001f, 0 };

constexpr size_t kGuard = 4; // 8-byte words before and after every plane

template<class T>
struct Plane {
    std::vector<uint64_t> store;
    size_t count = 0;
    void init(size_t n, T fill)
    {
        count = n;
        store.assign(2 * kGuard + (n * sizeof(T) + 7) / 8, 0xa5a5a5a5a5a5a5a5ull);
        for (size_t i = 0; i < n; ++i) data()[i] = fill;
    }
    T* data() { return reinterpret_cast<T*>(store.data() + kGuard); }
    bool guardsIntact() const
    {
        for (size_t i = 0; i < kGuard; ++i)
            if (store[i] != 0xa5a5a5a5a5a5a5a5ull || store[store.size() - 1 - i] != 0xa5a5a5a5a5a5a5a5ull) return false;
        // the tail of the last word past the plane's bytes
        const unsigned char* b = reinterpret_cast<const unsigned char*>(store.data() + kGuard);
        for (size_t i = count * sizeof(T); i < (store.size() - 2 * kGuard) * 8; ++i)
            if (b[i] != 0xa5) return false;
        return true;
    }
};

struct Case {
    uint32_t w = 0, h = 0;
    Plane<uint16_t> radiance, normalVelocity, radianceHistory, normalHistory, depthHistory, reprojected, average, resolved, temporal;
    Plane<float> depth, variance, numSamples;
    Plane<uint8_t> material;

    void init(uint32_t W, uint32_t H, uint32_t seed, bool allSky, float wildMotion)
    {
        w = W, h = H;
        const size_t n = static_cast<size_t>(W) * H, tiles = static_cast<size_t>((W + 7) / 8) * ((H + 7) / 8);
        radiance.init(4 * n, 0), normalVelocity.init(4 * n, 0), material.init(4 * n, 0), depth.init(n, 0.0f);
        radianceHistory.init(4 * n, 0), normalHistory.init(4 * n, 0), depthHistory.init(4 * n, 0), reprojected.init(4 * n, 0), average.init(4 * tiles, 0);
        variance.init(n, 0.0f), numSamples.init(n, 0.0f), resolved.init(4 * n, 0), temporal.init(4 * n, 0);
        refill(seed, allSky, wildMotion);
    }
    // new inputs, the written planes stay (a following frame)
    void refill(uint32_t seed, bool allSky, float wildMotion)
    {
        std::mt19937 rng(seed);
        std::uniform_real_distribution<float> u01(0.0f, 1.0f);
        const size_t n = static_cast<size_t>(w) * h;
        for (size_t p = 0; p < n; ++p) {
            depth.data()[p] = allSky || u01(rng) < 0.1f ? 1.0f : 0.9f + 0.0995f * u01(rng);
            const float kind = u01(rng);
            const float len = kind < 0.3f ? 0.1f * u01(rng) : kind < 0.6f ? 50.0f * u01(rng) : kind < 0.8f ? -5.0f * u01(rng) : 1.0e4f * wildMotion * (u01(rng) - 0.5f);
            for (int c = 0; c < 3; ++c) radiance.data()[4 * p + c] = refl::f2h(4.0f * u01(rng));
            radiance.data()[4 * p + 3] = refl::f2h(len);
            normalVelocity.data()[4 * p] = refl::f2h(0.6f * (u01(rng) - 0.5f));
            normalVelocity.data()[4 * p + 1] = refl::f2h(0.6f * (u01(rng) - 0.5f));
            // mostly sub-pixel motion; with wildMotion some UVs land tens of images away, on either side
            const float m = u01(rng) < 0.5f ? 0.01f : 40.0f * wildMotion;
            normalVelocity.data()[4 * p + 2] = refl::f2h(m * (u01(rng) - 0.5f));
            normalVelocity.data()[4 * p + 3] = refl::f2h(m * (u01(rng) - 0.5f));
            const float r = u01(rng);
            material.data()[4 * p] = r < 0.1f ? 0 : r < 0.7f ? static_cast<uint8_t>(150.0f * u01(rng)) : r < 0.85f ? 160 : 230;
        }
        if (n >= 3) {
            radiance.data()[4 * (n / 2)] = 0x7c00;         // +inf
            radiance.data()[4 * (n / 3) + 1] = 0x7e00;     // NaN
            radiance.data()[4 * (n - 1) + 3] = 0x7e00;     // a NaN ray length
        }
    }
    ArkReflDenoiseDesc desc(uint32_t flags)
    {
        ArkReflDenoiseDesc d {};
        d.struct_size = sizeof(d);
        d.width = w, d.height = h, d.flags = flags;
        d.no_tracing_roughness = 0.6f, d.temporal_stability = 0.7f;
        std::memcpy(d.world_from_view, kIdentity, 64);
        std::memcpy(d.view_from_projection, kUnproject, 64);
        std::memcpy(d.previous_frame_view_from_world, kPrevView, 64);
        std::memcpy(d.previous_frame_projection_from_view, kPrevProj, 64);
        d.z_near = 0.1f, d.z_far = 100.0f;
        d.radiance = radiance.data(), d.depth = depth.data(), d.material = material.data(), d.normal_velocity = normalVelocity.data();
        d.radiance_history = radianceHistory.data(), d.normal_history = normalHistory.data(), d.depth_history = depthHistory.data();
        d.reprojected = reprojected.data(), d.average_radiance = average.data(), d.variance = variance.data(), d.num_samples = numSamples.data();
        d.resolved = resolved.data(), d.temporal_accumulation = temporal.data();
        return d;
    }
    bool guardsIntact() const
    {
        return radiance.guardsIntact() && normalVelocity.guardsIntact() && material.guardsIntact() && depth.guardsIntact() && radianceHistory.guardsIntact() &&
               normalHistory.guardsIntact() && depthHistory.guardsIntact() && reprojected.guardsIntact() && average.guardsIntact() && variance.guardsIntact() &&
               numSamples.guardsIntact() && resolved.guardsIntact() && temporal.guardsIntact();
    }
};

static void sequences()
{
    const uint32_t sizes[5][2] = { { 1, 1 }, { 1, 97 }, { 8, 8 }, { 9, 7 }, { 29, 19 } };
    for (const auto& s : sizes)
        for (int variant = 0; variant < 3; ++variant) { // plain, wild reprojection UVs, all sky
            Case c;
            c.init(s[0], s[1], 100u * s[0] + s[1] + 7u * variant, variant == 2, variant == 1 ? 1.0f : 0.0f);
            ArkReflDenoiseDesc d = c.desc(ARK_REFL_DENOISE_FIRST_FRAME);
            CHECK(ark_ddgi_debug_refl_denoise_host(&d) == ARK_DDGI_OK, "%ux%u/%d: first frame refused", s[0], s[1], variant);
            // the first historyCopy ran: after the frame the history holds this frame's roughness
            const size_t n = static_cast<size_t>(s[0]) * s[1];
            size_t wrong = 0, glossy = 0, unwritten = 0;
            for (size_t p = 0; p < n; ++p) {
                const float r = static_cast<float>(c.material.data()[4 * p]) / 255.0f;
                wrong += c.depthHistory.data()[4 * p + 1] != refl::f2h(r);
                if (r < 0.6f) {
                    ++glossy;
                    unwritten += c.numSamples.data()[p] == 0.0f; // reproject stores at least 1
                } else {
                    wrong += c.numSamples.data()[p] != 0.0f || c.variance.data()[p] != 0.0f; // untouched
                }
            }
            CHECK(wrong == 0 && unwritten == 0, "%ux%u/%d: %zu wrong, %zu of %zu glossy unwritten", s[0], s[1], variant, wrong, unwritten, glossy);
            for (uint32_t f = 1; f < 3; ++f) {
                c.refill(1000u * f + s[0], variant == 2, variant == 1 ? 1.0f : 0.0f);
                d = c.desc(0);
                CHECK(ark_ddgi_debug_refl_denoise_host(&d) == ARK_DDGI_OK, "%ux%u/%d frame %u refused", s[0], s[1], variant, f);
            }
            d = c.desc(ARK_REFL_DENOISE_DISABLED);
            CHECK(ark_ddgi_debug_refl_denoise_host(&d) == ARK_DDGI_OK, "disabled refused");
            CHECK(std::memcmp(c.resolved.data(), c.radiance.data(), n * 8) == 0, "%ux%u/%d: disabled is not a copy", s[0], s[1], variant);
            CHECK(c.guardsIntact(), "%ux%u/%d: a guard word was written", s[0], s[1], variant);
        }
}

static void refusals()
{
    Case c;
    c.init(9, 7, 3, false, 0.0f);
    ArkReflDenoiseDesc d = c.desc(0);
    CHECK(ark_ddgi_debug_refl_denoise_check_desc(&d) == ARK_DDGI_OK, "a good descriptor is refused");
    CHECK(ark_ddgi_debug_refl_denoise_check_desc(nullptr) == ARK_DDGI_E_INVALID_ARGUMENT, "null descriptor");
    auto refused = [&](const char* what, auto&& change) {
        ArkReflDenoiseDesc e = c.desc(0);
        change(e);
        CHECK(ark_ddgi_debug_refl_denoise_check_desc(&e) == ARK_DDGI_E_INVALID_ARGUMENT && ark_ddgi_debug_refl_denoise_host(&e) == ARK_DDGI_E_INVALID_ARGUMENT, "%s accepted", what);
    };
    refused("struct_size", [](ArkReflDenoiseDesc& e) { e.struct_size -= 8; });
    refused("null radiance", [](ArkReflDenoiseDesc& e) { e.radiance = nullptr; });
    refused("null depth", [](ArkReflDenoiseDesc& e) { e.depth = nullptr; });
    refused("null average", [](ArkReflDenoiseDesc& e) { e.average_radiance = nullptr; });
    refused("null temporal", [](ArkReflDenoiseDesc& e) { e.temporal_accumulation = nullptr; });
    refused("alias out/out", [](ArkReflDenoiseDesc& e) { e.resolved = e.temporal_accumulation; });
    refused("alias in/out", [](ArkReflDenoiseDesc& e) { e.radiance_history = const_cast<uint16_t*>(e.radiance); });
    refused("overlap", [](ArkReflDenoiseDesc& e) { e.num_samples = e.variance + 5; });
    refused("misaligned", [](ArkReflDenoiseDesc& e) { e.resolved += 1; });
    refused("NaN matrix", [](ArkReflDenoiseDesc& e) { e.previous_frame_projection_from_view[5] = NAN; });
    refused("inf matrix", [](ArkReflDenoiseDesc& e) { e.world_from_view[0] = INFINITY; });
    refused("NaN threshold", [](ArkReflDenoiseDesc& e) { e.no_tracing_roughness = NAN; });
    refused("inf stability", [](ArkReflDenoiseDesc& e) { e.temporal_stability = INFINITY; });
    refused("NaN z_far", [](ArkReflDenoiseDesc& e) { e.z_far = NAN; });
    refused("z_near == z_far", [](ArkReflDenoiseDesc& e) { e.z_far = e.z_near; });
    refused("unknown flag", [](ArkReflDenoiseDesc& e) { e.flags = 4; });
    refused("2^28 pixels", [](ArkReflDenoiseDesc& e) { e.width = 1u << 14, e.height = 1u << 14; });
    // an empty image: OK, nothing touched, planes not looked at
    ArkReflDenoiseDesc e = c.desc(0);
    e.width = 0;
    e.resolved = nullptr;
    CHECK(ark_ddgi_debug_refl_denoise_host(&e) == ARK_DDGI_OK, "empty image refused");
}

static void knownAnswers()
{
    float in[256] = { 29.0f }, out[4];
    CHECK(ark_ddgi_debug_refl_denoise_kat(ARK_REFL_KAT_ROUND_UP8, in, 1, out, 1) == ARK_DDGI_OK && out[0] == 37.0f, "RoundUp8(29) = %g", out[0]);
    CHECK(refl::roundUp8(32) == 32 && refl::roundUp8(0) == 0 && refl::roundUp8(1) == 9, "RoundUp8");
    // fp16 both ways over every half
    for (uint32_t h = 0; h < 0x10000u; ++h) {
        const float f = refl::h2f(static_cast<uint16_t>(h));
        const uint16_t back = refl::f2h(f);
        const bool nan = (h & 0x7c00u) == 0x7c00u && (h & 0x3ffu);
        if (back != (nan ? 0x7e00u : h)) {
            CHECK(false, "half %04x -> %g -> %04x", h, f, back);
            break;
        }
    }
    CHECK(refl::f2h(65519.9f) == 0x7bff && refl::f2h(65520.0f) == 0x7c00 && refl::f2h(0x1p-25f) == 0 && refl::f2h(0x1.000002p-25f) == 1 && refl::f2h(1.00048828125f) == 0x3c00 &&
              refl::f2h(1.00146484375f) == 0x3c02,
          "f2h rounding");
}

// exp(x) = exp2f_(x log2 e) and pow(x, 512) = powf_ against glibc's double results, in fp32 ulps
static void libmError()
{
    auto ulps = [](float got, double want) {
        const float w = static_cast<float>(want);
        if (got == w) return 0.0;
        const float step = std::fabs(std::nextafterf(w, INFINITY) - w);
        return step > 0.0f ? std::fabs((static_cast<double>(got) - want) / step) : 0.0;
    };
    double worstExp = 0.0, worstPow = 0.0;
    for (int i = 0; i <= 200000; ++i) {
        const float x = -20.0f * static_cast<float>(i) / 200000.0f; // every exp argument of the passes is <= 0
        worstExp = std::fmax(worstExp, ulps(refl::expf_(x), std::exp(static_cast<double>(x))));
    }
    for (int i = 0; i <= 200000; ++i) {
        const float x = 0.9f + 0.1f * static_cast<float>(i) / 200000.0f; // below 0.9 the result is under 1e-23
        worstPow = std::fmax(worstPow, ulps(ark::powf_(x, 512.0f), std::pow(static_cast<double>(x), 512.0)));
    }
    std::printf("exp on [-20, 0]: max error %.2f ulp (fp32) against glibc\n", worstExp);
    std::printf("pow(x, 512) on [0.9, 1]: max error %.2f ulp (fp32) against glibc\n", worstPow);
    CHECK(worstExp < 32.0 && worstPow < 256.0, "exp / pow far from glibc: %.2f, %.2f ulp", worstExp, worstPow);
}

int main()
{
    sequences();
    refusals();
    knownAnswers();
    libmError();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
