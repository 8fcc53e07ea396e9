// xv_draws.h — the draw constructions of the on-device task samplers, stated once on top of philox.h: what a Philox call
// becomes (two uniforms, a 53-bit key, an fp64 Box-Muller pair, an exponential, an integer) and the index counter layout.
// The host states the same in xenoverse_amd/host_draws.py, the oracle's C independently.  The samplers
// are built with -ffp-contract=off: every expression below is evaluated as written, which is what makes task k the same
// bits whatever the batch.
#pragma once
#include <cmath>

#include "philox.h"

constexpr double XV_TWO_PI = 6.283185307179586;

struct xv_u2 {
  double a, b;
};
// the two uniforms of a call: words 0,1 and words 2,3
__device__ __forceinline__ xv_u2 xv_pair(const xv_u32x4& w) { return xv_u2{xv_u53(w.x, w.y), xv_u53(w.z, w.w)}; }
// the fp64 Box-Muller pair of a call: radius from the first uniform (1 - u in (0, 1]), angle from the second
__device__ __forceinline__ void xv_normal2(const xv_u2& u, double* zc, double* zs) {
  const double r = sqrt(-2.0 * log(1.0 - u.a));
  const double ang = XV_TWO_PI * u.b;
  *zc = r * cos(ang);
  *zs = r * sin(ang);
}
__device__ __forceinline__ double xv_expo(double u) { return -log(1.0 - u); }
__device__ __forceinline__ int xv_floor_int(double u, int m) { return (int)floor(u * (double)m); }
// the 53-bit integer of two words (xv_u53's numerator) and its uniform
__device__ __forceinline__ uint64_t xv_k53(uint32_t a, uint32_t b) { return ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6); }
__device__ __forceinline__ double xv_k53_u(uint64_t k53) { return (double)k53 * (1.0 / 9007199254740992.0); }
// the index layout: counter = {index lo, index hi, sub, purpose | tick << 8}, key = seed; tick below 2^24
__device__ __forceinline__ xv_u32x4 xv_index_draw(uint64_t seed, uint64_t index, uint32_t tick, uint32_t purpose,
                                                  uint32_t sub) {
  return xv_philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), sub, (purpose & 0xFFu) | (tick << 8), (uint32_t)seed,
                          (uint32_t)(seed >> 32));
}
