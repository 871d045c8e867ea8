// The noise of a seeded request (gfx950): a counter-based generator, so that a request's noise is a pure function of (seed, purpose, step, element
// index within the request) -- never of its row in a batch, of its neighbours or of launch geometry.  Philox4x32-10 with the Random123 constants;
//   key     = (seed low, seed high)
//   counter = (q low, q high, step, domain),  q = idx >> 2, idx the element's index in the request's OWN [C, h, w] tensor
// and element idx takes normal idx & 3 of the four that group q yields.  Used in registers by the NOISY step (scheduler_step.hip) and to fill
// tensors (noise.hip); tests/noise_ref.py restates it in numpy.  Including files are built without FMA contraction (Makefile), like step_math.h's.
#pragma once
#include "common.h"
#include "../../include/mxdenoise.h"

#pragma clang fp contract(off)

namespace mx {

// the integer half: the four output words of group q
__device__ __forceinline__ void philox4x32_10(unsigned long long seed, unsigned long long q, unsigned step, unsigned domain, unsigned (&w)[4]) {
  unsigned c0 = (unsigned)q, c1 = (unsigned)(q >> 32), c2 = step, c3 = domain;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// two words -> two normals (Box-Muller): u in (0, 1) and the angle t2 in (0, 2) half turns are exact in fp32, so neither log(0) nor an angle of a
// whole turn occurs
__device__ __forceinline__ void normal_pair(unsigned wa, unsigned wb, float& za, float& zb) {
  const float u = (float)(2u * (wa >> 9) + 1u) * 0x1p-24f;
  const float t2 = (float)(2u * (wb >> 9) + 1u) * 0x1p-23f;
  const float r = sqrtf(-2.0f * logf(u));
  float sn, cs;
  sincospif(t2, &sn, &cs);
  za = r * cs;
  zb = r * sn;
}

// THE noise function: the four N(0, 1) values of group q of (seed, step, domain)
__device__ __forceinline__ void noise_group(unsigned long long seed, unsigned step, unsigned domain, unsigned long long q, float (&z)[4]) {
  unsigned w[4];
  philox4x32_10(seed, q, step, domain, w);
  normal_pair(w[0], w[1], z[0], z[1]);
  normal_pair(w[2], w[3], z[2], z[3]);
}

// the normals of V consecutive elements from `within` (the first one's index in its request): one group per four elements when V is a multiple of 4
// (`within` is then one too: the vector paths), the element's own lane of its group when V == 1
template <int V>
__device__ __forceinline__ void noise_elems(unsigned long long seed, unsigned step, unsigned domain, long within, float (&z)[V]) {
  static_assert(V == 1 || V % 4 == 0, "a vector holds whole groups");
  if constexpr (V == 1) {
    float g[4];
    noise_group(seed, step, domain, (unsigned long long)within >> 2, g);
    const int lane = (int)(within & 3);
    z[0] = lane == 0 ? g[0] : lane == 1 ? g[1] : lane == 2 ? g[2] : g[3];
  } else {
#pragma unroll
    for (int k = 0; k < V / 4; ++k) {
      float g[4];
      noise_group(seed, step, domain, ((unsigned long long)within >> 2) + k, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[4 * k + i] = g[i];
    }
  }
}

}  // namespace mx
