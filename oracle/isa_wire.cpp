// TEST INFRASTRUCTURE ONLY -- the instruction yardstick of the wire casts.
//
// The wire form's 16-bit casts are defined by six x86 operations (see the
// header of stg_oracle.cpp's wire section).  Each function below applies ONE
// of them element-wise to whole arrays and nothing else: no block / tail rule,
// no flags, no arithmetic of its own.  The rule that says which position takes
// which operation is composed in Python (oracle.py: IsaWire), so this file
// shares no conversion logic with stg_oracle.cpp or csrc/wire_dev.h -- what
// the CPU executes is the definition.
//
// The vector forms take n % 8 == 0 elements (callers pad); the scalar forms
// take any n.  Built with the oracle's flags (-O3 -march=broadwell: F16C, AVX2).
#include <immintrin.h>
#include <stddef.h>
#include <stdint.h>

#define ISA_API extern "C" __attribute__((visibility("default")))

// vcvtps2ph ymm -> xmm, imm8 = 0: round to nearest even, MXCSR.RC ignored
ISA_API void isa_cvtps_ph(const float *src, uint16_t *dst, size_t n) {
    for (size_t i = 0; i < n; i += 8) {
        const __m128i h = _mm256_cvtps_ph(_mm256_loadu_ps(src + i), 0);
        _mm_storeu_si128(reinterpret_cast<__m128i *>(dst + i), h);
    }
}

// vcvtph2ps xmm -> ymm
ISA_API void isa_cvtph_ps(const uint16_t *src, float *dst, size_t n) {
    for (size_t i = 0; i < n; i += 8) {
        const __m256 f = _mm256_cvtph_ps(_mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i)));
        _mm256_storeu_ps(dst + i, f);
    }
}

// packssdw: two vectors of four int32 -> eight int16, signed saturation
ISA_API void isa_packs_epi32(const uint32_t *src, uint16_t *dst, size_t n) {
    for (size_t i = 0; i < n; i += 8) {
        const __m128i lo = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i));
        const __m128i hi = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i + 4));
        _mm_storeu_si128(reinterpret_cast<__m128i *>(dst + i), _mm_packs_epi32(lo, hi));
    }
}

// vpmovsxwd: eight int16 -> eight int32, sign extension
ISA_API void isa_cvtepi16_epi32(const uint16_t *src, uint32_t *dst, size_t n) {
    for (size_t i = 0; i < n; i += 8) {
        const __m256i w = _mm256_cvtepi16_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i)));
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(dst + i), w);
    }
}

// vcvttss2si r32 and a 16-bit store.  The intrinsic, not a C cast: a cast in a
// loop may be vectorised into a saturating pack, which is another operation.
ISA_API void isa_cvttss_si32_lo16(const float *src, uint16_t *dst, size_t n) {
    for (size_t i = 0; i < n; ++i) dst[i] = static_cast<uint16_t>(_mm_cvttss_si32(_mm_load_ss(src + i)));
}

// (float) of a uint16_t: zero extension, then an exact int32 -> float
ISA_API void isa_u16_to_f32(const uint16_t *src, float *dst, size_t n) {
    for (size_t i = 0; i < n; ++i) dst[i] = static_cast<float>(src[i]);
}
