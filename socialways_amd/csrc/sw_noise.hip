// sw_noise.hip - the counter-based device noise stream: uniform z as a pure function of (seed, domain, step, draw, row, column).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the standard constants.
//   key     = (seed low word, seed high word)
//   counter = (row, draw, step, column block + 256 * domain), column block = column >> 2
//   the four output words are the columns 4b .. 4b+3 of column block b; uniform = float(word >> 8) * 2^-24: exact, in
//   [0, 1), the 24-bit grid of torch.rand.
// No state anywhere: any rank, chunk or tile produces exactly its rows, in any order, with the same bits.
#include "sw_common.h"
#include "../../include/socialways_hip.h"

#define SW_PHILOX_M0 0xD2511F53u
#define SW_PHILOX_M1 0xCD9E8D57u
#define SW_PHILOX_W0 0x9E3779B9u
#define SW_PHILOX_W1 0xBB67AE85u
#define SW_NOISE_MAXCOLS 1024      // 256 column blocks: the domain sits above them in counter word 3

struct sw_u4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ sw_u4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(SW_PHILOX_M0, c0), l0 = SW_PHILOX_M0 * c0;
    const uint32_t h1 = __umulhi(SW_PHILOX_M1, c2), l1 = SW_PHILOX_M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += SW_PHILOX_W0;
    k1 += SW_PHILOX_W1;
  }
  return sw_u4{c0, c1, c2, c3};
}

// One thread per (step, draw, row, 4-column block) = one float4 of `out`; thread f owns out[4f .. 4f+3] (ld % 4 == 0, so the
// float4s of a row are consecutive and a wave stores 1 KB of consecutive memory).  Blocks past `cols` are the zero padding.
__global__ __launch_bounds__(256) void noise_uniform_kernel(uint32_t k0, uint32_t k1, uint32_t domain, uint32_t step0,
                                                            uint32_t draw0, uint32_t n_draws, uint32_t row0, uint32_t rows,
                                                            uint32_t cols, uint32_t ld4, uint32_t total, float* __restrict__ out) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= total) return;
  const uint32_t r = f / ld4, b = f - r * ld4;
  const uint32_t q = r / rows, i = r - q * rows;
  const uint32_t t = q / n_draws, k = q - t * n_draws;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const uint32_t c = 4u * b;
  if (c < cols) {
    const sw_u4 x = philox4x32_10(row0 + i, draw0 + k, step0 + t, b + 256u * domain, k0, k1);
    const float s = 5.9604644775390625e-8f;      // 2^-24
    v[0] = (float)(x.x >> 8) * s;
    v[1] = c + 1u < cols ? (float)(x.y >> 8) * s : 0.f;
    v[2] = c + 2u < cols ? (float)(x.z >> 8) * s : 0.f;
    v[3] = c + 3u < cols ? (float)(x.w >> 8) * s : 0.f;
  }
  st4(out + (size_t)f * 4, v);
}

extern "C" int sw_noise_uniform(unsigned long long seed, int domain, unsigned step0, int n_steps, unsigned draw0, int n_draws,
                                unsigned row0, int rows, int cols, int ld, float* out, void* stream) {
  if (domain < 0 || domain > 1 || cols < 1 || cols > SW_NOISE_MAXCOLS || ld < cols || (ld & 3)) return SW_EARG;
  if (!out || ((uintptr_t)out & 15)) return SW_EARG;
  if (n_steps < 1 || n_draws < 1 || rows < 1) return SW_EARG;
  const unsigned long long lim = 1ull << 32;      // counter words are 32 bits: no index may wrap into another's range
  if ((unsigned long long)row0 + (unsigned long long)rows > lim || (unsigned long long)draw0 + (unsigned long long)n_draws > lim ||
      (unsigned long long)step0 + (unsigned long long)n_steps > lim)
    return SW_EARG;
  // the kernel indexes float4s with 32 bits (and the grid's x extent is a signed int)
  const unsigned long long ld4 = (unsigned long long)ld / 4;
  const unsigned long long per_step = (unsigned long long)n_draws * (unsigned long long)rows;      // < 2^62
  if (per_step > 0x7fffffffull / ld4 || per_step * ld4 > 0x7fffffffull / (unsigned long long)n_steps) return SW_ESHAPE;
  const uint32_t total = (uint32_t)(per_step * ld4 * (unsigned long long)n_steps);
  SW_LAUNCH(noise_uniform_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, (uint32_t)seed,
            (uint32_t)(seed >> 32), (uint32_t)domain, (uint32_t)step0, (uint32_t)draw0, (uint32_t)n_draws, (uint32_t)row0,
            (uint32_t)rows, (uint32_t)cols, (uint32_t)ld4, total, out);
  SW_CHECK_LAUNCH("noise_uniform_kernel");
  return SW_OK;
}
