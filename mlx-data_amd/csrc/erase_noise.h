// erase_noise.h -- the noise of Random Erasing (mxd_erase; DESIGN.md section
// 2): Philox4x32-10, the four standard normals of one Philox call, and the
// casts to the 16-bit element types.  One statement for both sides: the erase
// kernel (erase.hip) and the CPU statement (erase.cpp, mxd_erase_apply)
// include this header and so run the same operations in the same order.
//
// Float contract: integer / bit operations and float32 add, multiply, divide
// and sqrt only, each correctly rounded and none fused (both sides compile
// with -ffp-contract=off, and the pragma below says so again).  No libm or
// OCML call: ln and sincos(2 pi u) are written out here.  Every int -> float
// conversion is of a value below 2^24 and so exact.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MXD_EN_HD __host__ __device__ inline
#else
#define MXD_EN_HD inline
#endif

#pragma clang fp contract(off)

namespace mxd {
namespace noise {

MXD_EN_HD uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
MXD_EN_HD float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }

// Philox4x32-10 (Salmon et al., SC'11): counter c[0..3], key k[0..1] -> four
// words in c.
MXD_EN_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1, c[3] = (uint32_t)p0;
    c[0] = n0, c[2] = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// -2 ln u for u = (2k + 1) 2^-24, k = w >> 9: u = m 2^e with m in
// (sqrt(1/2), sqrt(2)], ln u = e ln 2 + 2 atanh(s), s = (m - 1) / (m + 1)
// (m - 1 is exact; |s| < 0.1716, the series is cut behind s^9: 7e-10).
// ln 2 is split so that e * kLn2Hi is exact for |e| <= 24.
MXD_EN_HD float neg2_ln(uint32_t w) {
  const float u = (float)(2u * (w >> 9) + 1u) * 5.9604644775390625e-8f;  // 2^-24: exact
  const uint32_t b = bits_of(u);
  int e = (int)(b >> 23) - 127;
  uint32_t mb = (b & 0x007fffffu) | 0x3f800000u;  // m in [1, 2)
  if (mb > 0x3fb504f3u) mb -= 0x00800000u, e += 1;  // above sqrt(2): m / 2
  const float m = float_of(mb);
  const float s = (m - 1.0f) / (m + 1.0f);
  const float t = s * s;
  float p = 0.22222222f;  // 2/9
  p = p * t + 0.2857143f;  // 2/7
  p = p * t + 0.4f;        // 2/5
  p = p * t + 0.6666667f;  // 2/3
  p = p * t + 2.0f;
  const float lnm = p * s;
  const float fe = (float)e;
  const float kLn2Hi = 0.693145751953125f, kLn2Lo = 1.42860677e-6f;  // hi: 16 bits
  const float ln = fe * kLn2Hi + (fe * kLn2Lo + lnm);
  return ln * -2.0f;
}

// (cos, sin)(2 pi u) for u = (2k + 1) 2^-24, k = w >> 9.  The angle is a
// dyadic rational, so the octant reduction is exact: 8u = o + r 2^-21 with
// octant o = k >> 20 and r = (2k + 1) mod 2^21 (odd, never 0); odd octants
// take the mirrored 2^21 - r.  a = r 2^-21 * pi/4 lies in (0, pi/4), where
// both series are cut below 2e-9.
MXD_EN_HD void sincos_2pi(uint32_t w, float* cs, float* sn) {
  const uint32_t k = w >> 9;
  const uint32_t o = k >> 20;
  uint32_t r = (2u * k + 1u) & 0x1fffffu;
  if (o & 1u) r = 0x200000u - r;
  const float a = ((float)r * 4.76837158203125e-7f) * 0.78539816339744831f;  // r 2^-21 exact, then pi/4
  const float t = a * a;
  float ps = 2.7557319e-6f;        // 1/9!
  ps = ps * t + -1.98412698e-4f;   // 1/7!
  ps = ps * t + 8.33333333e-3f;    // 1/5!
  ps = ps * t + -0.16666667f;      // 1/3!
  const float s = a + a * (ps * t);
  float pc = -2.755732e-7f;        // 1/10!
  pc = pc * t + 2.48015873e-5f;    // 1/8!
  pc = pc * t + -1.38888889e-3f;   // 1/6!
  pc = pc * t + 4.16666667e-2f;    // 1/4!
  pc = pc * t + -0.5f;
  const float c = 1.0f + pc * t;
  const bool swap = ((o + 1u) >> 1) & 1u;
  const float ca = swap ? s : c, sa = swap ? c : s;
  *cs = ((o + 2u) >> 2) & 1u ? -ca : ca;
  *sn = o >> 2 ? -sa : sa;
}

// The four normals of the words w[0..3] (Box-Muller): (z0, z1) from w0, w1,
// (z2, z3) from w2, w3.
MXD_EN_HD void normals4(const uint32_t (&w)[4], float (&z)[4]) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float rad = __builtin_sqrtf(neg2_ln(w[2 * h]));
    float c, s;
    sincos_2pi(w[2 * h + 1], &c, &s);
    z[2 * h] = rad * c, z[2 * h + 1] = rad * s;
  }
}

// PIXEL noise: the normals of elements x = 4 xq .. 4 xq + 3 of row y, channel
// c, box b under the image's seed.
MXD_EN_HD void pixel_normals(uint32_t seed0, uint32_t seed1, uint32_t b, uint32_t c, uint32_t y, uint32_t xq,
                             float (&z)[4]) {
  uint32_t w[4] = {xq, y, c, b};
  philox4x32_10(w, seed0, seed1);
  normals4(w, z);
}

// COLOR noise: the normals of box b's channels (the fourth is not used).
MXD_EN_HD void color_normals(uint32_t seed0, uint32_t seed1, uint32_t b, float (&z)[4]) {
  uint32_t w[4] = {0u, 0u, 0u, 0x100u + b};
  philox4x32_10(w, seed0, seed1);
  normals4(w, z);
}

// float32 -> bfloat16 bits, round to nearest even (finite values).
MXD_EN_HD uint32_t to_bf16(float v) {
  const uint32_t f = bits_of(v);
  if ((f & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (f + 0x7fffu + ((f >> 16) & 1u)) >> 16;
}

// float32 -> float16 bits, round to nearest even (subnormal results through
// one float32 addition whose rounding is the half's).
MXD_EN_HD uint32_t to_f16(float v) {
  uint32_t f = bits_of(v);
  const uint32_t sign = f & 0x80000000u;
  f ^= sign;
  const uint32_t magic = ((127u - 15u) + (23u - 10u) + 1u) << 23;
  uint32_t o;
  if (f >= ((127u + 16u) << 23)) {
    o = f > (255u << 23) ? 0x7e00u : 0x7c00u;
  } else if (f < (113u << 23)) {
    o = bits_of(float_of(f) + float_of(magic)) - magic;
  } else {
    const uint32_t odd = (f >> 13) & 1u;
    f += ((15u - 127u) << 23) + 0xfffu;
    f += odd;
    o = f >> 13;
  }
  return o | (sign >> 16);
}

// Element kinds of an erase (the call's element type).
enum Elem : int32_t { kElemU8 = 0, kElemF32 = 1, kElemF16 = 2, kElemBF16 = 3 };

// A float as the bits of an element of kind `elem` (not kElemU8).
MXD_EN_HD uint32_t elem_bits(float v, int elem) {
  return elem == kElemF32 ? bits_of(v) : elem == kElemF16 ? to_f16(v) : to_bf16(v);
}

}  // namespace noise
}  // namespace mxd
