// sw_clearance_grad.hip - the scene-clearance penalty of the generator loss and its gradient: per pair of agents of a
// scene and per segment phi = max(0, 1 - |c|^2 / d0^2)^2 of the closest approach c that sw_scene_clearance measures
// (sc_segment_at: sc_segment's arithmetic), differentiated by hand.  Plain VALU work, block-diagonal per scene, independent
// of the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include <math.h>
#include <stdint.h>

#define CG_MAX_TILES 8         // grid.y at most: the 64-agent tiles of a scene are dealt round robin over it

// ---- gradient (definition in include/socialways_hip.h) -------------------------------------------------------------------
//   One wave per (scene, tile of 64 agents): blockIdx.x = scene, the scene's tiles a0 = 64 * blockIdx.y, + 64 * gridDim.y,
//   ..; a block whose first tile lies past the scene leaves at once (the host does not know the scene sizes).  Lane al owns
//   agent a0 + al: the SC_TC + 1 points of its path of the current time chunk and the SC_TC + 1 gradient accumulators of
//   those points sit in registers, the paths of a tile of up to 64 partners in LDS (the lane's own points when the partner
//   tile is its tile).  The lane walks partner tiles, partners and segments in ascending order; segment j of the chunk adds
//   k tau c to the accumulator of its end point j + 1 and k (1 - tau) c to that of its start point j, k = -4 u / d0^2.  A
//   point on a chunk boundary ends one chunk and starts the next: its dpos row takes two += of this lane, in that order.
//   One owner per dpos row, loss[a] and count[a], no atomics, nothing read across scenes: two calls give the same bits, and
//   a scene's outputs do not depend on the rest of the batch.  A lane stores the rows of a chunk only if one of the chunk's
//   (partner, segment)s was active (|c|^2 < d0^2): otherwise they are not touched.  Lanes past n compute on clamped indices
//   and do not store.  The pair (a, a) is computed like any other and masked by a select.
__global__ __launch_bounds__(64) void clearance_grad_kernel(const float* __restrict__ pos, int pstride,
                                                            const float* __restrict__ start, int sstride,
                                                            const int* __restrict__ scene_off, int Tp, float d02,
                                                            float inv_d02, float scale, float* __restrict__ dpos, int dstride,
                                                            float* __restrict__ loss, int* __restrict__ count) {
  __shared__ float2 tile[64 * SC_NP];
  const int s0 = scene_off[blockIdx.x], n = scene_off[blockIdx.x + 1] - s0;
  if ((int)blockIdx.y * 64 >= n) return;                   // uniform: in front of every barrier (n <= 0 included)
  const int lane = threadIdx.x;
  const int first = start ? 1 : 0;                         // points in front of pos row 0
  const int NS = Tp - 1 + first;                           // segments of a path

  for (int a0 = blockIdx.y * 64; a0 < n; a0 += 64 * gridDim.y) {
    const int a = a0 + lane, ac = a < n ? a : n - 1;
    const size_t row = (size_t)s0 + ac;
    float phi = 0.f;
    int cnt = 0;
    for (int t0 = 0; t0 < NS; t0 += SC_TC) {
      const int nseg = NS - t0 < SC_TC ? NS - t0 : SC_TC;
      float2 own[SC_NP], g[SC_NP];
      sc_load_own(own, pos, pstride, start, sstride, row, s0 + ac, Tp, t0, nseg);
#pragma unroll
      for (int p = 0; p < SC_NP; ++p) g[p] = float2{0.f, 0.f};
      int hit = 0;                                         // active (partner, segment)s of this chunk
      for (int b0 = 0; b0 < n; b0 += 64) {
        const int nb = n - b0 < 64 ? n - b0 : 64;
        const int bc = b0 + lane < n ? b0 + lane : n - 1;
        __syncthreads();                                   // the previous tile has been read
        sc_stage_row(tile + lane * SC_NP, own, b0 == a0, pos, pstride, start, sstride, (size_t)s0 + bc, s0 + bc, Tp, t0, nseg);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
          const float2* q = tile + b * SC_NP;              // one address for the wave: a broadcast read
          const bool other = b0 + b != a;
          const float2 q0 = q[0];
          float rx = own[0].x - q0.x, ry = own[0].y - q0.y;      // r0 of the first segment
          float pphi = 0.f;                                // the pair's phi over this chunk: summed apart, then added
#pragma unroll
          for (int j = 0; j < SC_TC; ++j) {
            if (j < nseg) {                                // uniform
              float tau, cx, cy;
              sc_segment_at(own[j + 1], q[j + 1], rx, ry, tau, cx, cy);
              const float cc = cx * cx + cy * cy;
              const bool on = other && cc < d02;
              const float u = on ? fmaxf(1.f - cc * inv_d02, 0.f) : 0.f;
              const float k = -4.f * u * inv_d02;
              const float wx = on ? k * cx : 0.f, wy = on ? k * cy : 0.f;
              g[j + 1].x += tau * wx;
              g[j + 1].y += tau * wy;
              g[j].x += (1.f - tau) * wx;
              g[j].y += (1.f - tau) * wy;
              pphi += u * u;
              hit += on ? 1 : 0;
            }
          }
          phi += pphi;
        }
      }
      cnt += hit;
      if (a < n && hit) {
#pragma unroll
        for (int p = 0; p < SC_NP; ++p) {
          const int r = t0 + p - first;                    // dpos row of point p: the start point is data and has none
          if (p <= nseg && r >= 0) {
            float2* d = reinterpret_cast<float2*>(dpos + ((size_t)(s0 + a) * Tp + r) * dstride);
            float2 v = *d;
            v.x += scale * g[p].x;
            v.y += scale * g[p].y;
            *d = v;
          }
        }
      }
    }
    if (a < n) {
      if (loss) loss[s0 + a] = 0.5f * phi;
      if (count) count[s0 + a] = cnt;
    }
  }
}

extern "C" int sw_clearance_grad(const float* pos, int pstride, const float* start, int sstride, const int* scene_off, int S,
                                 int B, int Tp, float d0, float scale, float* dpos, int dstride, float* loss, int* count,
                                 void* stream) {
  float d02, inv_d02;
  if (!sw_paths_ok(pos, pstride, start, sstride) || !sw_penalty_dist(d0, d02, inv_d02) || !isfinite(scale)) return SW_EARG;
  if (!scene_off || !dpos || S < 0 || B < 0 || Tp < 1) return SW_EARG;
  if ((dstride != 2 && dstride != 4) || ((uintptr_t)dpos & 7)) return SW_EARG;       // rows are written as float2
  if (B == 0 || S == 0) return SW_OK;
  const int tiles = (B + 63) / 64;                         // no scene has more
  SW_LAUNCH(clearance_grad_kernel, dim3((unsigned)S, (unsigned)(tiles < CG_MAX_TILES ? tiles : CG_MAX_TILES)), dim3(64), 0,
            (hipStream_t)stream, pos, pstride, start, sstride, scene_off, Tp, d02, inv_d02, scale, dpos, dstride, loss, count);
  SW_CHECK_LAUNCH("clearance_grad_kernel");
  return SW_OK;
}
