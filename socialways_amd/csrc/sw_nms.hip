// sw_nms.hip - diverse top-M of K sampled futures: greedy non-maximum suppression in score order, per agent or per scene
// (a joint future = draw k of every agent of the scene), with the share of the K draws that every kept mode stands for.
// A selection, not arithmetic: the only floating-point work is the distance between two draws; everything that is
// written out is a draw index, an integer count or one integer ratio.  Does not depend on the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include <stdint.h>

#define SW_NMS_MAXK 4096
#define NMS_NONE 0x7fffffff

// d_a(k, c): inv_ss * the distance between draws k and c of batch row `row` - at the last step (metric 0) or its mean over
// the Tp steps, summed over t ascending (metric 1)
__device__ __forceinline__ float nms_dist(const float* __restrict__ pos, int pstride, int B, int Tp, int metric, float inv_ss,
                                          int k, int c, int row) {
  const float* pk = pos + ((size_t)k * B + row) * Tp * pstride;
  const float* pc = pos + ((size_t)c * B + row) * Tp * pstride;
  float sum = 0.f;
  for (int t = metric ? 0 : Tp - 1; t < Tp; ++t) {
    const float2 x = *reinterpret_cast<const float2*>(pk + (size_t)t * pstride);
    const float2 y = *reinterpret_cast<const float2*>(pc + (size_t)t * pstride);
    const float dx = x.x - y.x, dy = x.y - y.y;
    sum += sqrtf(dx * dx + dy * dy);
  }
  return inv_ss * (metric ? sum / (float)Tp : sum);
}

// ---- the greedy loop (definition in include/socialways_hip.h) ---------------------------------------------------------------
//   One wave per group, four groups per workgroup.  Lane l owns the draws k = l, l + 64, ...: their group score s_g(k) and
//   their assignment (-1 = alive) sit in the wave's LDS slice and only the owner touches them inside the loop.  A pick is a
//   wave reduction on (score, lowest k); every lane then reads the pick's positions from one address and walks the agents
//   of the group sequentially for each of its alive draws - leaving at the first agent farther than the radius - so the
//   scene size has no lane boundary.  The picks are kept in LDS for the leftover draws, which compare their D_g to every
//   pick.  The counts per mode are M integer wave reductions over the assignments; they take over the score slice, which
//   is dead by then.  One writer per output element, no atomics.  LDS per wave: 6 * roundup(K, 8) + 2 * roundup(M, 8)
//   bytes (scores fp32, assignments and picks int16: K, M <= 4096), 128 KB per workgroup at the largest K.
__global__ __launch_bounds__(256) void sample_nms_kernel(const float* __restrict__ pos, int pstride,
                                                          const float* __restrict__ score, const int* __restrict__ scene_off,
                                                          int G, int B, int K, int Tp, int M, int metric, float inv_ss,
                                                          float radius, const float* __restrict__ err,
                                                          const int* __restrict__ best, int* __restrict__ order,
                                                          int* __restrict__ count, float* __restrict__ weight,
                                                          int* __restrict__ assign, float* __restrict__ per_row) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int Kp = (K + 7) & ~7, Mp = (M + 7) & ~7;
  unsigned char* slice = nms_lds + (size_t)wave * (6 * Kp + 2 * Mp);
  float* s = reinterpret_cast<float*>(slice);
  short* asg = reinterpret_cast<short*>(slice + 4 * Kp);
  short* pick = reinterpret_cast<short*>(slice + 6 * Kp);
  const bool live = (int)blockIdx.x * 4 + wave < G;        // a wave past the last group repeats it and does not store
  const int g = live ? (int)blockIdx.x * 4 + wave : G - 1;
  int s0 = g, n = 1;
  if (scene_off) {
    const int s1 = scene_off[g + 1];
    s0 = scene_off[g];
    n = (s0 >= 0 && s1 >= s0 && s1 <= B) ? s1 - s0 : 0;    // offsets outside the batch: read nothing
  }
  const float INF = __builtin_inff();

  for (int k = lane; k < K; k += 64) {
    float v = INF;
    for (int a = 0; a < n; ++a) v = fminf(v, score[(size_t)k * B + s0 + a]);
    s[k] = v;
    asg[k] = -1;
  }

  int np = 0;                                               // picks so far (wave-uniform)
  for (int m = 0; m < M; ++m) {
    float bs = 0.f;
    int bk = NMS_NONE;
    for (int k = lane; k < K; k += 64)                      // ascending k and a strict >: the lowest k of equal scores
      if (asg[k] < 0 && (bk == NMS_NONE || s[k] > bs)) {
        bs = s[k];
        bk = k;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o);
      const int ok = __shfl_xor(bk, o);
      if (ok != NMS_NONE && (bk == NMS_NONE || os > bs || (os == bs && ok < bk))) {
        bs = os;
        bk = ok;
      }
    }
    const int c = __builtin_amdgcn_readfirstlane(bk);
    if (c == NMS_NONE) break;                               // nothing alive
    pick[m] = (short)c;                                     // every lane writes the value it reads back later
    for (int k = lane; k < K; k += 64) {
      if (asg[k] >= 0) continue;
      bool in = true;                                       // D_g(k, c) <= radius: every agent within the radius
      if (k != c)
        for (int a = 0; a < n && in; ++a) in = nms_dist(pos, pstride, B, Tp, metric, inv_ss, k, c, s0 + a) <= radius;
      if (in) asg[k] = (short)m;
    }
    if (lane == 0 && live) order[(size_t)g * M + m] = c;
    np = m + 1;
  }

  for (int k = lane; k < K; k += 64) {                      // leftovers (np == M only): the nearest pick, the lowest m of equals
    if (asg[k] >= 0) continue;
    float bd = INF;
    int bm = 0;
    for (int m = 0; m < np; ++m) {
      const int c = pick[m];
      float D = 0.f;
      for (int a = 0; a < n; ++a) D = fmaxf(D, nms_dist(pos, pstride, B, Tp, metric, inv_ss, k, c, s0 + a));
      if (D < bd) {
        bd = D;
        bm = m;
      }
    }
    asg[k] = (short)bm;
  }
  if (live) {
    for (int k = lane; k < K; k += 64) assign[(size_t)g * K + k] = asg[k];
    for (int m = np + lane; m < M; m += 64) {
      order[(size_t)g * M + m] = -1;
      weight[(size_t)g * M + m] = 0.f;
    }
    if (lane == 0) count[g] = np;
  }
  __syncthreads();                                          // the scores are dead: their slice takes the counts
  for (int m = 0; m < np; ++m) {
    int c = 0;
    for (int k = lane; k < K; k += 64) c += asg[k] == m ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    s[m] = __int_as_float(c);
    if (lane == 0 && live) weight[(size_t)g * M + m] = (float)c / (float)K;
  }
  if (!per_row) return;
  __syncthreads();                                          // assignments and counts are read across lanes from here
  if (!live) return;
  const float2* e = reinterpret_cast<const float2*>(err);
  for (int a = lane; a < n; a += 64) {
    const int row = s0 + a;
    const float2 e0 = e[(size_t)pick[0] * B + row];
    float ma = e0.x, mf = e0.y;
    for (int m = 1; m < np; ++m) {
      const float2 em = e[(size_t)pick[m] * B + row];
      ma = fminf(ma, em.x);
      mf = fminf(mf, em.y);
    }
    const int kb = best ? best[row] : -1;
    float w = 0.f, mi = 0.f;
    if (kb >= 0 && kb < K) {
      const int mb = asg[kb];
      w = (float)__float_as_int(s[mb]) / (float)K;
      mi = (float)mb;
    }
    float* p = per_row + (size_t)row * 6;
    p[0] = e0.x; p[1] = e0.y; p[2] = ma; p[3] = mf; p[4] = w; p[5] = mi;
  }
}

extern "C" int sw_sample_nms(const float* pos, int pstride, const float* score, const int* scene_off, int S, int B, int K,
                             int Tp, int M, int metric, float inv_ss, float radius, const float* err, const int* best,
                             int* order, int* count, float* weight, int* assign, float* per_row, void* stream) {
  if (!sw_paths_ok(pos, pstride, nullptr, 0)) return SW_EARG;
  if (!score || !order || !count || !weight || !assign || B < 0 || K < 1 || M < 1 || M > K || Tp < 1) return SW_EARG;
  if ((metric != 0 && metric != 1) || !(radius >= 0.f) || !(inv_ss > 0.f)) return SW_EARG;
  if ((per_row && !err) || (scene_off && S < 0) || ((uintptr_t)err & 7)) return SW_EARG;      // errors are read as float2
  if (K > SW_NMS_MAXK) return SW_ESHAPE;
  const int G = scene_off ? S : B;
  if (B == 0 || G == 0) return SW_OK;
  const int lds = 4 * (6 * ((K + 7) & ~7) + 2 * ((M + 7) & ~7));
  static int have = 0;
  if (int rc = sw_set_lds((const void*)sample_nms_kernel, lds, have)) return rc;
  SW_LAUNCH(sample_nms_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), lds, (hipStream_t)stream, pos, pstride, score, scene_off,
            G, B, K, Tp, M, metric, inv_ss, radius, err, best, order, count, weight, assign, per_row);
  SW_CHECK_LAUNCH("sample_nms_kernel");
  return SW_OK;
}
