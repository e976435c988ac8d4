// sw_wall_grad.hip - the wall-clearance penalty of the generator loss and its gradient: per (path segment, wall) pair
// phi = max(0, 1 - |c|^2 / dw^2)^2 of the closest approach c that sw_path_walls measures (wl_closest of sw_wall_dev.h and
// nothing else), differentiated by the envelope formula of the WALLS section of include/socialways_hip.h.  Plain VALU work,
// independent of the hidden size and of the scenes: a path owns its pairs alone.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include "sw_wall_dev.h"
#include <math.h>
#include <stdint.h>

#define WG_THREADS 256
#define WG_WAVES (WG_THREADS / 64)

struct WgArgs {
  const float* pos;
  const float* start;
  const int* len;
  const float* walls;
  int pstride, sstride, dstride, B, Tp, NS, front, M;
  long long R;                 // K * B paths
  float dw2, inv_dw2, scale;
};

// ---- gradient (definition in include/socialways_hip.h) -------------------------------------------------------------------
//   The mapping of path_walls_kernel: one 256-thread workgroup per 64 paths, a lane owns a path - the same one in each of the
//   four waves - and wave w takes the wall slice w, w + 4, ..; the walls sit in LDS and are read as the wave-uniform partner,
//   the lane's SC_TC + 1 points of the current time chunk and the SC_TC + 1 gradient accumulators of those points in
//   registers.  A wave walks its walls, then the chunk's segments, in ascending order; segment j adds k s c to the
//   accumulator of its end point j + 1 and k (1 - s) c to that of its start point j, k = -4 u / dw^2, every contribution
//   through a select (a segment behind the path's length, NaN included, reaches nothing).  Waves 1 .. 3 leave their partial
//   sums in LDS and wave 0 adds them to its own in the order 1, 2, 3, then makes the one read-modify-write of the chunk's
//   dpos rows - only if one of the chunk's (segment, wall)s was counted, and only of the points a counted segment can reach.
//   A point on a chunk boundary ends one chunk and starts the next: its row takes two += of the same thread, in chunk order.
//   One owner per dpos row, loss[r] and count[r], no atomics; the order of the additions depends on (Tp, M) only: two calls
//   give the same bits and a path's outputs do not depend on the rest of the batch.  Lanes behind the last path walk it again
//   and store nothing.
__global__ __launch_bounds__(WG_THREADS) void wall_grad_kernel(WgArgs A, float* __restrict__ dpos, float* __restrict__ loss,
                                                               int* __restrict__ count) {
  __shared__ float4 wl[WL_MAX];
  __shared__ float2 part[WG_WAVES - 1][SC_NP][64];
  __shared__ float f_phi[WG_WAVES - 1][64];
  __shared__ int f_hit[WG_WAVES - 1][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  wl_stage(wl, A.walls, A.M, tid, WG_THREADS);
  __syncthreads();

  const long long r = (long long)blockIdx.x * 64 + lane;
  const size_t row = (size_t)(r < A.R ? r : A.R - 1);
  const int agent = (int)(row % (size_t)A.B);
  const int lim_all = A.len ? sc_len(A.len, agent, A.Tp, 1 - A.front) : A.NS;      // countable segments of the path
  float phi = 0.f;
  int cnt = 0;
  for (int t0 = 0; t0 < A.NS; t0 += SC_TC) {
    const int nsg = A.NS - t0 < SC_TC ? A.NS - t0 : SC_TC;
    float2 own[SC_NP], g[SC_NP];
    sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, row, agent, A.Tp, t0, nsg);
#pragma unroll
    for (int p = 0; p < SC_NP; ++p) g[p] = float2{0.f, 0.f};
    const int lim = lim_all - t0;                            // countable segments of the path in this chunk (<= 0: none)
    int hit = 0;                                             // counted (segment, wall)s of this wave in this chunk
    for (int m = wave; m < A.M; m += WG_WAVES) {             // uniform within the wave
      const float4 w = wl[m];
      float wphi = 0.f;                                      // the wall's phi over this chunk: summed apart, then added
#pragma unroll
      for (int j = 0; j < SC_TC; ++j) {
        if (j < nsg) {                                       // uniform
          float s, cx, cy, cc;
          wl_closest(own[j], own[j + 1], w, s, cx, cy, cc);
          const bool on = j < lim && cc < A.dw2;
          const float u = on ? fmaxf(1.f - cc * A.inv_dw2, 0.f) : 0.f;
          const float k = -4.f * u * A.inv_dw2;
          const float wx = k * cx, wy = k * cy;
          g[j + 1].x += on ? s * wx : 0.f;
          g[j + 1].y += on ? s * wy : 0.f;
          g[j].x += on ? (1.f - s) * wx : 0.f;
          g[j].y += on ? (1.f - s) * wy : 0.f;
          wphi += u * u;
          hit += on ? 1 : 0;
        }
      }
      phi += wphi;
    }
    if (wave) {
#pragma unroll
      for (int p = 0; p < SC_NP; ++p) part[wave - 1][p][lane] = g[p];
      f_hit[wave - 1][lane] = hit;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < WG_WAVES - 1; ++w) hit += f_hit[w][lane];
      cnt += hit;
      if (r < A.R && hit) {
#pragma unroll
        for (int p = 0; p < SC_NP; ++p) {
          const int dr = t0 + p - A.front;                   // dpos row of point p: the start point is data and has none
          if (p <= nsg && p <= lim && dr >= 0) {
            float2 a = g[p];
#pragma unroll
            for (int w = 0; w < WG_WAVES - 1; ++w) {
              const float2 b = part[w][p][lane];
              a.x += b.x;
              a.y += b.y;
            }
            float2* d = reinterpret_cast<float2*>(dpos + ((size_t)r * A.Tp + dr) * A.dstride);
            float2 v = *d;
            v.x += A.scale * a.x;
            v.y += A.scale * a.y;
            *d = v;
          }
        }
      }
    }
    __syncthreads();                                         // the partials have been read
  }
  if (wave) f_phi[wave - 1][lane] = phi;
  __syncthreads();
  if (wave == 0 && r < A.R) {
#pragma unroll
    for (int w = 0; w < WG_WAVES - 1; ++w) phi += f_phi[w][lane];
    if (loss) loss[r] = phi;
    if (count) count[r] = cnt;
  }
}

extern "C" int sw_wall_grad(const float* pos, int pstride, const float* start, int sstride, const int* len, int K, int B,
                            int Tp, const float* walls, int M, float dw, float scale, float* dpos, int dstride, float* loss,
                            int* count, void* stream) {
  float dw2, inv_dw2;
  if (!sw_paths_ok(pos, pstride, start, sstride) || !sw_penalty_dist(dw, dw2, inv_dw2) || !isfinite(scale)) return SW_EARG;
  if (!dpos || (M > 0 && !walls) || K < 1 || B < 0 || Tp < 1 || M < 0) return SW_EARG;
  if ((dstride != 2 && dstride != 4) || ((uintptr_t)dpos & 7)) return SW_EARG;       // rows are written as float2
  if (M > SW_WALLS_MAX) return SW_ESHAPE;
  if (B == 0) return SW_OK;
  const long long R = (long long)K * B;
  if ((R + 63) / 64 > 0x7fffffffLL) return SW_EARG;
  WgArgs A = {};
  A.pos = pos; A.start = start; A.len = len; A.walls = walls;
  A.pstride = pstride; A.sstride = sstride; A.dstride = dstride; A.B = B; A.Tp = Tp; A.M = M; A.R = R;
  A.front = start ? 1 : 0;                                   // points in front of pos row 0
  A.NS = Tp - 1 + A.front;                                   // segments of a path
  A.dw2 = dw2; A.inv_dw2 = inv_dw2; A.scale = scale;
  SW_LAUNCH(wall_grad_kernel, dim3((unsigned)((R + 63) / 64)), dim3(WG_THREADS), 0, (hipStream_t)stream, A, dpos, loss, count);
  SW_CHECK_LAUNCH("wall_grad_kernel");
  return SW_OK;
}
