// sw_walls.hip - the clearance of paths (the K draws, the true futures, ego plans) to a static map of line segments: per
// (draw, agent) path the smallest distance to any wall over its counted segments, the frame at which the first segment closer
// than `dist` ends and the number of (segment, wall) pairs closer than it.  The segment-against-wall arithmetic is
// sw_wall_dev.h's; the points of a path are sw_scene_dev.h's.  Does not depend on the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include "sw_wall_dev.h"
#include <stdint.h>

#define PW_THREADS 256
#define PW_WAVES (PW_THREADS / 64)

struct PwArgs {
  const float* pos;
  const float* start;
  const int* len;
  const float* walls;
  int pstride, sstride, B, Tp, NS, first, M;
  long long R;                 // K * B paths
  float inv_ss, dist;
};

// ---- the clearance of 64 paths (definitions in include/socialways_hip.h) ----------------------------------------------------
//   One 256-thread workgroup per 64 paths.  A lane owns a path, the same one in each of the four waves, and wave w takes the
//   wall slice w, w + 4, w + 8 ...: a chunk of plans (few paths, many walls) still fills its waves, and a chunk of draws has
//   R / 64 workgroups of four waves.  The walls sit in LDS and are read as the wave-uniform partner (every lane the same
//   address: a broadcast); the lane's own SC_TC + 1 points sit in registers (sc_load_own), longer paths in time chunks.  What
//   a lane accumulates is a minimum and two integers; the four waves leave theirs in LDS and wave 0 folds them in the order
//   0 .. 3.  No atomics: two calls give the same bits.
__global__ __launch_bounds__(PW_THREADS) void path_walls_kernel(PwArgs A, float* __restrict__ clear, int* __restrict__ first,
                                                                int* __restrict__ nseg) {
  __shared__ float4 wl[WL_MAX];
  __shared__ unsigned f_min[PW_WAVES][64];
  __shared__ int f_first[PW_WAVES][64], f_n[PW_WAVES][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  wl_stage(wl, A.walls, A.M, tid, PW_THREADS);
  __syncthreads();

  const long long r = (long long)blockIdx.x * 64 + lane;
  const size_t row = (size_t)(r < A.R ? r : A.R - 1);        // lanes behind the last path walk it again and write nothing
  const int agent = (int)(row % (size_t)A.B);
  const int lim_all = A.len ? sc_len(A.len, agent, A.Tp, A.first) : A.NS;
  float mn = __builtin_inff();
  int tf = 0x7fffffff, ns = 0;
  for (int t0 = 0; t0 < A.NS; t0 += SC_TC) {
    const int nsg = A.NS - t0 < SC_TC ? A.NS - t0 : SC_TC;
    float2 own[SC_NP];
    sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, row, agent, A.Tp, t0, nsg);
    const int lim = lim_all - t0;                            // countable segments of the path in this chunk (<= 0: none)
    for (int m = wave; m < A.M; m += PW_WAVES) {             // uniform within the wave
      const float4 w = wl[m];
#pragma unroll
      for (int j = 0; j < SC_TC; ++j) {
        if (j < nsg) {                                       // uniform
          float s, cx, cy, cc;
          wl_closest(own[j], own[j + 1], w, s, cx, cy, cc);
          const bool on = j < lim;
          mn = on ? fminf(mn, cc) : mn;
          const bool hit = on && sqrtf(cc) * A.inv_ss < A.dist;
          ns += hit ? 1 : 0;
          tf = hit ? min(tf, t0 + j + A.first) : tf;
        }
      }
    }
  }
  f_min[wave][lane] = __float_as_uint(mn);
  f_first[wave][lane] = tf;
  f_n[wave][lane] = ns;
  __syncthreads();
  if (wave == 0 && r < A.R) {
    mn = __uint_as_float(f_min[0][lane]);
#pragma unroll
    for (int w = 1; w < PW_WAVES; ++w) {
      mn = fminf(mn, __uint_as_float(f_min[w][lane]));
      tf = min(tf, f_first[w][lane]);
      ns += f_n[w][lane];
    }
    clear[r] = sqrtf(mn) * A.inv_ss;
    first[r] = tf == 0x7fffffff ? -1 : tf;
    nseg[r] = ns;
  }
}

extern "C" int sw_path_walls(const float* pos, int pstride, const float* start, int sstride, const int* len, int K, int B,
                             int Tp, const float* walls, int M, float inv_ss, float dist, float* clear, int* first, int* nseg,
                             void* stream) {
  if (!sw_paths_ok(pos, pstride, start, sstride) || !clear || !first || !nseg || (M > 0 && !walls)) return SW_EARG;
  if (K < 1 || B < 0 || Tp < 1 || M < 0 || !(inv_ss > 0.f) || !(dist >= 0.f)) return SW_EARG;
  if (M > SW_WALLS_MAX) return SW_ESHAPE;
  if (B == 0) return SW_OK;
  const long long R = (long long)K * B;
  if ((R + 63) / 64 > 0x7fffffffLL) return SW_EARG;
  PwArgs A = {};
  A.pos = pos; A.start = start; A.len = len; A.walls = walls;
  A.pstride = pstride; A.sstride = sstride; A.B = B; A.Tp = Tp; A.M = M; A.R = R;
  A.first = start ? 0 : 1;
  A.NS = Tp - A.first;
  A.inv_ss = inv_ss; A.dist = dist;
  SW_LAUNCH(path_walls_kernel, dim3((unsigned)((R + 63) / 64)), dim3(PW_THREADS), 0, (hipStream_t)stream, A, clear, first, nseg);
  SW_CHECK_LAUNCH("path_walls_kernel");
  return SW_OK;
}
