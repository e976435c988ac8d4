// sw_scene.hip - scene-level evaluation of K sampled futures: the clearance of every agent against the other agents of
// its scene (closest approach of two linearly moving points, per segment, clamped to the segment) and the per-scene
// reduction to joint min ADE / FDE and collision rates.  Plain VALU work, block-diagonal per scene like the social block;
// neither kernel depends on the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include <stdint.h>

// ---- clearance, dense and with ragged futures (definitions in include/socialways_hip.h) ----------------------------------
//   One wave per (scene, group of 64 / n_pad draws); blockIdx.x = scene * K + group, groups past the scene's last one
//   leave at once (the host does not know the scene sizes).  Lane (kk, al) owns clear[k0 + kk][agent a0 + al]: its own
//   SC_TC + 1 points sit in registers, the paths of a tile of up to 64 partner agents sit in LDS (one row per lane, the
//   lane's own points when the partner tile is its tile), and the lane walks partners x segments taking the minimum of
//   the squared distance - one owner per output, no atomics.  Scenes above 64 agents loop over agent tiles on both sides,
//   longer futures over time chunks.  Lanes past n or K compute on clamped indices and do not store.
//   LEN: a length per agent.  Agent a has va = len[a] - (start ? 0 : 1) countable segments (len clamped into 1 .. Tp); the
//   segment of pair (a, b) with global index j counts if j < min(va, vb).  The partner's count travels with its tile (tlen,
//   written between the tile's two barriers).  r0 advances through every segment and only the minimum is gated, by a
//   select: the countable segments are a prefix, so whatever the padding holds - NaN included - never reaches one.  All
//   lengths n: the bits of the dense kernel on the paths cut to n frames (same chunk boundaries, same segment arithmetic;
//   min is exact).  Without LEN there is no tlen, len is not read and the minimum is not gated.
template <bool LEN>
__global__ __launch_bounds__(64) void scene_clearance_kernel(const float* __restrict__ pos, int pstride,
                                                             const float* __restrict__ start, int sstride,
                                                             const int* __restrict__ scene_off,
                                                             const int* __restrict__ len, int B, int K, int Tp,
                                                             float inv_ss, float* __restrict__ clear) {
  __shared__ float2 tile[64 * SC_NP + (LEN ? 32 : 0)];    // LEN: the 64 counts of the tile's agents behind its points
  int* tlen = reinterpret_cast<int*>(tile + 64 * SC_NP);
  const int s = blockIdx.x / K, g = blockIdx.x - s * K;
  const int s0 = scene_off[s], n = scene_off[s + 1] - s0;
  const int lg = sc_log2_pad(n), n_pad = 1 << lg;
  const int k0 = g * (64 >> lg);
  if (k0 >= K || n <= 0) return;                           // uniform: in front of every barrier
  const int lane = threadIdx.x, al = lane & (n_pad - 1), kk = lane >> lg;
  const int k = k0 + kk, kc = k < K ? k : K - 1;
  const int first = start ? 0 : 1;                         // future frame at which segment 0 ends
  const int NS = Tp - first;                               // segments of a path
  const float INF = __builtin_inff();
  const float2* mine = tile + (size_t)(kk << lg) * SC_NP;  // the partner rows of this lane's draw
  const int* mlen = tlen + (kk << lg);

  for (int a0 = 0; a0 < n; a0 += n_pad) {
    const int a = a0 + al, ac = a < n ? a : n - 1;
    const size_t row = (size_t)kc * B + s0 + ac;
    int va = 0;
    if constexpr (LEN) va = sc_len(len, s0 + ac, Tp, first);
    float best = INF;
    for (int t0 = 0; t0 < NS; t0 += SC_TC) {
      const int nseg = NS - t0 < SC_TC ? NS - t0 : SC_TC;
      float2 own[SC_NP];
      sc_load_own(own, pos, pstride, start, sstride, row, s0 + ac, Tp, t0, nseg);
      for (int b0 = 0; b0 < n; b0 += n_pad) {
        const int nb = n - b0 < n_pad ? n - b0 : n_pad;
        const int bc = b0 + al < n ? b0 + al : n - 1;
        __syncthreads();                                   // the previous tile has been read
        sc_stage_row(tile + lane * SC_NP, own, b0 == a0, pos, pstride, start, sstride, (size_t)kc * B + s0 + bc, s0 + bc, Tp,
                     t0, nseg);
        if constexpr (LEN) tlen[lane] = b0 == a0 ? va : sc_len(len, s0 + bc, Tp, first);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
          const auto q = [row = mine + b * SC_NP](int p) { return row[p]; };
          int lim = 0;                                     // countable segments of the pair in this chunk (<= 0: none)
          if constexpr (LEN) lim = min(va, mlen[b]) - t0;
          float m = INF;
          SC_CHUNK(LEN, own, q, nseg, lim, m);
          best = (b0 + b == a) ? best : fminf(best, m);
        }
      }
    }
    if (a < n && k < K) clear[(size_t)k * B + s0 + a] = sqrtf(best) * inv_ss;
  }
}

// both entries: the dense launch without lengths
extern "C" int sw_scene_clearance_len(const float* pos, int pstride, const float* start, int sstride, const int* scene_off,
                                      const int* len, int S, int B, int K, int Tp, float inv_ss, float* clear, void* stream) {
  if (!sw_paths_ok(pos, pstride, start, sstride)) return SW_EARG;
  if (!scene_off || !clear || S < 0 || B < 0 || K < 1 || Tp < 1 || !(inv_ss > 0.f)) return SW_EARG;
  if ((long long)S * K > 0x7fffffffLL) return SW_EARG;
  if (B == 0 || S == 0) return SW_OK;
  if (len) {
    SW_LAUNCH_AS("scene_clearance_len_kernel", scene_clearance_kernel<true>, dim3((unsigned)(S * K)), dim3(64), 0,
                 (hipStream_t)stream, pos, pstride, start, sstride, scene_off, len, B, K, Tp, inv_ss, clear);
    SW_CHECK_LAUNCH("scene_clearance_len_kernel");
  } else {
    SW_LAUNCH_AS("scene_clearance_kernel", scene_clearance_kernel<false>, dim3((unsigned)(S * K)), dim3(64), 0,
                 (hipStream_t)stream, pos, pstride, start, sstride, scene_off, len, B, K, Tp, inv_ss, clear);
    SW_CHECK_LAUNCH("scene_clearance_kernel");
  }
  return SW_OK;
}

extern "C" int sw_scene_clearance(const float* pos, int pstride, const float* start, int sstride, const int* scene_off,
                                  int S, int B, int K, int Tp, float inv_ss, float* clear, void* stream) {
  return sw_scene_clearance_len(pos, pstride, start, sstride, scene_off, nullptr, S, B, K, Tp, inv_ss, clear, stream);
}

// ---- per-scene reduction -------------------------------------------------------------------------------------------------
//   One wave per scene, four scenes per workgroup, lanes laid out as in the clearance kernel: 64 / n_pad draws side by
//   side, each over the scene's agents.  Per draw the agent sums and minima are folded with an xor butterfly inside the
//   draw's lanes, every lane keeps the running result of the draws it saw (k ascending, strict <: the first k wins), and
//   a second butterfly folds the draw groups, the lower k winning a tie.  Fixed order throughout: two calls, same bits.
struct ScAcc {
  float sade, sfde, cbest, cmin;     // min_k sade, min_k sfde, sclear at kbest, min_k sclear
  int kbest, ndraw, nagent;          // first k of min sade, colliding draws, colliding (k, a)
};
__device__ __forceinline__ void sc_fold(ScAcc& x, float sade, float sfde, float cbest, float cmin, int kbest, int ndraw,
                                        int nagent) {
  if (sade < x.sade || (sade == x.sade && kbest < x.kbest)) {
    x.sade = sade;
    x.kbest = kbest;
    x.cbest = cbest;
  }
  x.sfde = fminf(x.sfde, sfde);
  x.cmin = fminf(x.cmin, cmin);
  x.ndraw += ndraw;
  x.nagent += nagent;
}

__global__ __launch_bounds__(256) void scene_reduce_kernel(const float* __restrict__ err, const float* __restrict__ clear,
                                                           const int* __restrict__ scene_off, int S, int B, int K,
                                                           float coll_dist, float* __restrict__ per_scene,
                                                           int* __restrict__ best) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;
  const int s0 = scene_off[s], n = scene_off[s + 1] - s0;
  if (n <= 0) return;
  const int lg = sc_log2_pad(n), n_pad = 1 << lg;
  const int lane = threadIdx.x & 63, al = lane & (n_pad - 1), kk = lane >> lg;
  const float INF = __builtin_inff();
  const bool pairs = clear != nullptr && n > 1;
  const float inv_n = 1.f / (float)n;
  ScAcc acc = {INF, INF, INF, INF, 0x7fffffff, 0, 0};
  for (int k = kk; k < K; k += 64 >> lg) {                 // the draws of this lane group, ascending
    float sa = 0.f, sf = 0.f, cm = INF;
    int cnt = 0;
    for (int a = al; a < n; a += n_pad) {
      const float2 e = reinterpret_cast<const float2*>(err)[(size_t)k * B + s0 + a];
      sa += e.x;
      sf += e.y;
      if (pairs) {
        const float c = clear[(size_t)k * B + s0 + a];
        cm = fminf(cm, c);
        cnt += c < coll_dist ? 1 : 0;
      }
    }
    for (int w = 1; w < n_pad; w <<= 1) {                  // within the draw's lanes: every lane ends with the total
      sa += __shfl_xor(sa, w);
      sf += __shfl_xor(sf, w);
      cm = fminf(cm, __shfl_xor(cm, w));
      cnt += __shfl_xor(cnt, w);
    }
    sc_fold(acc, sa * inv_n, sf * inv_n, cm, cm, k, cm < coll_dist ? 1 : 0, cnt);
  }
  for (int w = n_pad; w < 64; w <<= 1) {                   // across the draw groups
    const float sade = __shfl_xor(acc.sade, w), sfde = __shfl_xor(acc.sfde, w), cbest = __shfl_xor(acc.cbest, w),
                cmin = __shfl_xor(acc.cmin, w);
    const int kbest = __shfl_xor(acc.kbest, w), ndraw = __shfl_xor(acc.ndraw, w), nagent = __shfl_xor(acc.nagent, w);
    sc_fold(acc, sade, sfde, cbest, cmin, kbest, ndraw, nagent);
  }
  if (lane == 0) {
    float* o = per_scene + (size_t)s * 6;
    o[0] = acc.sade;
    o[1] = acc.sfde;
    o[2] = pairs ? (float)acc.ndraw / (float)K : 0.f;
    o[3] = pairs && acc.cbest < coll_dist ? 1.f : 0.f;
    o[4] = pairs ? acc.cmin : INF;
    o[5] = pairs ? (float)acc.nagent / ((float)K * (float)n) : 0.f;
    if (best) best[s] = acc.kbest;
  }
}

extern "C" int sw_scene_reduce(const float* err, const float* clear, const int* scene_off, int S, int B, int K,
                               float coll_dist, float* per_scene, int* best, void* stream) {
  if (!err || !scene_off || !per_scene || S < 0 || B < 0 || K < 1 || ((uintptr_t)err & 7)) return SW_EARG;
  if (B == 0 || S == 0) return SW_OK;
  SW_LAUNCH(scene_reduce_kernel, dim3((S + 3) / 4), dim3(256), 0, (hipStream_t)stream, err, clear, scene_off, S, B, K,
            coll_dist, per_scene, best);
  SW_CHECK_LAUNCH("scene_reduce_kernel");
  return SW_OK;
}
