/* tests/test_reservoir_first_cpu.py compiles and runs this: include/flx_reservoir_first.h's rule — does the reservoir take the first light it weighs, told from
 * the sine's ARGUMENT and the weight — against the literal flx_abs(y) * w <= w with y from flx_sin, on the host.  It prints what it checked and how often the two
 * disagreed, and exits with 1 if they ever did.  TEST INFRASTRUCTURE ONLY. */
#include <float.h>
#include <stdio.h>
#include <stdlib.h>

#include "flx_reservoir_first.h"

static unsigned long long checked, disagreed, taken, slow;

static void hold(float a, float w) {
  const int want = flx_first_light_taken_literal(a, w), got = flx_first_light_taken(a, w);
  checked++;
  taken += (unsigned long long)(want != 0);
  slow += (unsigned long long)(w == flx_inff() && flx_abs(a) <= 1048576.0f);
  if ((want != 0) != (got != 0)) {
    if (disagreed < 20ull) printf("DISAGREE a=%a (0x%08x) w=%a (0x%08x): literal %d, rule %d\n", (double)a, flx_f2u(a), (double)w, flx_f2u(w), want, got);
    disagreed++;
  }
}

static uint32_t lcg_state = 0x2545f491u;
static uint32_t lcg(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float unit(void) { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }      /* [0, 1) */

int main(void) {
  const float weights[] = { 0.0f, flx_u2f(1u) /* the smallest denormal */, 1.0f, FLT_MAX, flx_u2f(0x7f800000u) /* +inf */, flx_u2f(0x7fc00000u) /* NaN */,
                            flx_u2f(0x00800000u) /* the smallest normal */, flx_u2f(0x007fffffu) /* the largest denormal */, 3.0e-5f, 0.37f, 1.0e30f };
  const int nw = (int)(sizeof weights / sizeof weights[0]);
  /* 1. the argument on both sides of +-2^20, float by float, and the values that are no numbers */
  const uint32_t edge = flx_f2u(1048576.0f);
  for (int sign = 0; sign < 2; sign++)
    for (int d = -4096; d <= 4096; d++) {
      const float a = flx_u2f((uint32_t)((int32_t)edge + d) | ((uint32_t)sign << 31));
      for (int k = 0; k < nw; k++) hold(a, weights[k]);
    }
  {
    const float odd[] = { flx_u2f(0x7fc00000u), flx_u2f(0xffc00000u), flx_u2f(0x7f800001u), flx_u2f(0x7f800000u), flx_u2f(0xff800000u), FLT_MAX, -FLT_MAX, 0.0f, -0.0f,
                          flx_u2f(1u), flx_u2f(0x80000001u), 1.0f, -1.0f, 3.14159274f, 6.28318548f, 1.57079637f, 2097152.0f, -2097152.0f, 1048575.9375f, -1048575.9375f };
    for (unsigned i = 0; i < sizeof odd / sizeof odd[0]; i++)
      for (int k = 0; k < nw; k++) hold(odd[i], weights[k]);
  }
  /* 2. arguments where the sine is 0 or close to it (whole multiples of pi, rounded): y == 0 is what decides a weight of +inf */
  for (int m = -3000; m <= 3000; m++) {
    const float a = (float)((double)m * 3.14159265358979323846);
    for (int d = -2; d <= 2; d++) {
      const float b = flx_u2f((uint32_t)((int32_t)flx_f2u(a) + d));
      for (int k = 0; k < nw; k++) hold(b, weights[k]);
    }
  }
  /* 3. random draws as the shading makes them: (z, w) in [-1, 1], the frame's seed, the argument by noise()'s own operations; seeds up to 30 000 take the argument
   * across 2^20 (59 x 1.618 x 10 984 = 2^20.  Among them 11 500 and 20 000, the seeds of tests/test_shade_shortcuts_gpu.py) */
  unsigned long long random_triples = 0;
  for (int i = 0; i < 200000; i++) {
    const float z = unit() * 2.0f - 1.0f, w2 = unit() * 2.0f - 1.0f;
    float seed;
    switch (i & 7) {
      case 0: seed = 11500.0f; break;
      case 1: seed = 20000.0f; break;
      case 2: seed = unit() * 30000.0f; break;
      case 3: seed = 10934.0f + unit() * 100.0f; break;      /* around the crossing itself */
      case 4: seed = (float)(lcg() % 1000u); break;
      default: seed = unit() * 100.0f; break;
    }
    const float a = flx_noise_y_arg(seed, z, w2, FLX_BIAS);
    float wt;
    switch ((i >> 3) % 6) {
      case 0: wt = weights[(i >> 6) % nw]; break;
      case 1: wt = unit() * 1.0e-40f; break;                  /* denormal weights */
      case 2: wt = unit() * 1.0e38f * 3.4f; break;            /* up to FLT_MAX and, rounded, beyond: +inf */
      default: wt = unit() * unit() * 4.0f; break;
    }
    hold(a, wt);
    random_triples++;
  }
  printf("checked %llu pairs (%llu random triples): the literal test is true in %llu, takes the sine in the rule's slow branch in %llu; disagreements %llu\n", checked,
         random_triples, taken, slow, disagreed);
  return disagreed == 0ull ? 0 : 1;
}
