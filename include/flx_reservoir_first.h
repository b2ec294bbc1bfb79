/*
 * flx_reservoir_first.h — does the reservoir take the FIRST light it weighs?  (fragment:400-433, reservoirPick in csrc/flx_device.h.)
 *
 * Before its loop over the lights the shader draws n0 = noise(seed, randomVec.z, randomVec.w, BIAS).  Of n0, .z and .w are
 * never read, .x feeds only the draw in front of a SECOND light, and .y — lastRandomY — enters one comparison per light:
 *     C = (abs(lastRandomY) * totalWeight <= weight).
 * For the first light of positive strength totalWeight = 0.0f + weight == weight =: w exactly (w = length(colorForLight) is a
 * square root: +0 or above, +inf, or NaN; never -0), so C = (|y| * w <= w) with
 *     a = (randomVec.z * 12.9898f + randomVec.w * 78.233f) + 59.0f * (BIAS + seed * PHI)      the f32 operations of noise(), in its order
 *     y = flx_fract(flx_sin(a) * 43758.5453f) * 2.0f - 1.0f.
 * What C needs of y:
 *   - flx_sin(a) is NaN if and only if !(|a| <= 2^20) (flx_rem_pio2: NaN, an infinity or a magnitude above 2^20); then y is NaN,
 *     |y| * w is NaN and C is FALSE whatever w is.
 *   - Otherwise flx_sin(a) lies in [-1, 1], its product with 43758.5453f is finite, flx_fract of a finite float lies in [0, 1]
 *     (x - floor(x) rounds to 1.0f at most), and y = fract * 2 - 1 is finite with |y| <= 1.  Then:
 *       w NaN            |y| * w is NaN: C is FALSE.
 *       0 <= w < +inf    the real product |y| w lies in [0, w]; rounding to nearest is monotone and both ends are floats, so
 *                        RN(|y| w) lies in [0, w] too: C is TRUE.  This takes in w == 0 (0 <= 0) and a denormal w in either flush
 *                        mode: flushed, the product is 0 <= w (or 0 <= 0 where w itself is read as 0).
 *       w == +inf        |y| * inf is +inf for y != 0 (TRUE) and NaN for y == 0 (FALSE): C depends on y, and the sine is taken
 *                        as before.  Rare (a light's strength over (1 + distance)^2 must overflow), so behind a branch.
 * So C = (|a| <= 2^20) && (w < +inf), with the lanes of w == +inf computing y: an f32 range check in place of two sines in double
 * (~164 vector instructions a shade, 58 of them f64).  The rule holds for the first light WEIGHED; the kernels use it where the
 * scene has ONE light — with more, the draw's .x and .y feed the next light's draw and every value is needed.
 *
 * tests/test_reservoir_first_cpu.py holds flx_first_light_taken against the literal expression on the host.
 * Plain C99, also valid C++ / HIP, like flx_math.h.
 */
#ifndef FLX_RESERVOIR_FIRST_H
#define FLX_RESERVOIR_FIRST_H

#include "flx_math.h"

#define FLX_NOISE_PHI 1.61803398874989484820459f      /* fragment:5 */

/* the argument of the sine behind noise(random_seed, nx, ny, seed).y, by noise()'s own f32 operations (fragment:119-121) */
FLX_HD float flx_noise_y_arg(float random_seed, float nx, float ny, float seed) {
  float d = nx * 12.9898f + ny * 78.233f;
  float k = seed + random_seed * FLX_NOISE_PHI;
  return d + 59.0f * k;
}
/* noise(...).y from that argument */
FLX_HD float flx_noise_y_from_arg(float a) { return flx_fract(flx_sin(a) * 43758.5453f) * 2.0f - 1.0f; }

/* the literal test of fragment:426 for the first light weighed (totalWeight == weight == w) */
FLX_HD int flx_first_light_taken_literal(float a, float w) {
  float y = flx_noise_y_from_arg(a);
  return flx_abs(y) * w <= w;
}
/* ... and the same boolean without the sine (the derivation above) */
FLX_HD int flx_first_light_taken(float a, float w) {
  if (!(flx_abs(a) <= 1048576.0f)) return 0;
  if (w == flx_inff()) {
#if defined(__HIP_DEVICE_COMPILE__)
    /* the sine stays behind this branch: to the compiler it is free of side effects and, in reservoirPick, invariant in the loop over the lights — without this it
     * computes the sine in front of the loop, for every lane, and selects afterwards (seen in the ISA: the rule then saves one of the two sines, not both) */
    asm volatile("" : "+v"(a));
#endif
    return flx_first_light_taken_literal(a, w);
  }
  return w < flx_inff();
}

#endif /* FLX_RESERVOIR_FIRST_H */
