// sw_scene_dev.h - the device pieces sw_scene.hip, sw_compose.hip and sw_clearance_grad.hip share: the points of a path,
// the closest approach of two linearly moving points within one segment, the lane layout of a scene, and the walk over the
// pairs of a scene (the chunk of a pair, a lane's own points, the partner tile).  sw_scene.hip and sw_compose.hip form a
// clearance from these and nothing else, so a clearance of sw_scene_compose carries the bits sw_scene_clearance gives the
// same two paths.  Behind them, the host part: the two argument checks every entry point of the family makes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define SC_TC 16               // segments per time chunk: a lane keeps the SC_TC + 1 points of its own path in registers
#define SC_NP (SC_TC + 1)

// Lanes of a wave for a scene of n agents: n_pad = 64 above 32 agents, else the next power of two; the wave then holds
// 64 / n_pad draws k side by side (lane = kk * n_pad + agent), so a chunk of 8-agent scenes fills its lanes with 8 draws.
__device__ __forceinline__ int sc_log2_pad(int n) {
  if (n > 32) return 6;
  int lg = 0;
  while ((1 << lg) < n) ++lg;
  return lg;
}

// point p of the path of (row = k * B + agent): the start point in front of the Tp positions when there is one
__device__ __forceinline__ float2 sc_point(const float* __restrict__ pos, int pstride, const float* __restrict__ start,
                                           int sstride, size_t row, int agent, int Tp, int p) {
  if (start) {
    if (p == 0) return float2{start[(size_t)agent * sstride], start[(size_t)agent * sstride + 1]};
    p -= 1;
  }
  return *reinterpret_cast<const float2*>(pos + (row * Tp + p) * pstride);
}

// One segment: (rx, ry) = r0 on entry, the next segment's r0 on exit; m = min(m, squared closest approach).  The
// reciprocal is the hardware's (1 ulp): tau only places the point on the segment, its error moves the distance by
// |dv| * 2^-23 at most.  dd = 0 (no relative motion) takes tau = 0 whatever the reciprocal returned.
__device__ __forceinline__ void sc_segment(float2 pa, float2 pb, float& rx, float& ry, float& m) {
  const float ex = pa.x - pb.x, ey = pa.y - pb.y;
  const float dx = ex - rx, dy = ey - ry;
  const float dd = dx * dx + dy * dy, rd = rx * dx + ry * dy;
  float tau = -rd * __builtin_amdgcn_rcpf(dd);
  tau = dd > 0.f ? fminf(fmaxf(tau, 0.f), 1.f) : 0.f;
  const float cx = rx + tau * dx, cy = ry + tau * dy;
  m = fminf(m, cx * cx + cy * cy);
  rx = ex;
  ry = ey;
}

// sc_segment that hands back where the closest approach lies instead of folding a minimum: tau and c = r0 + tau dv, by
// sc_segment's arithmetic (the same reciprocal, the same clamp, tau = 0 at dd = 0), so |c|^2 carries the bits sc_segment
// would have folded.  tau minimises |r0 + tau dv|^2 over [0, 1]: d|c|^2 / d(r1) = 2 tau c and d|c|^2 / d(r0) = 2 (1 - tau) c
// (sw_clearance_grad.hip).  (rx, ry) = r0 on entry, the next segment's r0 on exit.
__device__ __forceinline__ void sc_segment_at(float2 pa, float2 pb, float& rx, float& ry, float& tau, float& cx, float& cy) {
  const float ex = pa.x - pb.x, ey = pa.y - pb.y;
  const float dx = ex - rx, dy = ey - ry;
  const float dd = dx * dx + dy * dy, rd = rx * dx + ry * dy;
  tau = -rd * __builtin_amdgcn_rcpf(dd);
  tau = dd > 0.f ? fminf(fmaxf(tau, 0.f), 1.f) : 0.f;
  cx = rx + tau * dx;
  cy = ry + tau * dy;
  rx = ex;
  ry = ey;
}

// sc_segment whose minimum is gated by a select: r0 advances, m moves only when `on` - whatever the segment holds, NaN
// included, reaches nothing when it does not count
__device__ __forceinline__ void sc_segment_if(bool on, float2 pa, float2 pb, float& rx, float& ry, float& m) {
  float mm = m;
  sc_segment(pa, pb, rx, ry, mm);
  m = on ? mm : m;
}

// countable segments of an agent with ragged futures: len clamped into 1 .. Tp, first = the frame at which segment 0 ends
__device__ __forceinline__ int sc_len(const int* __restrict__ len, int agent, int Tp, int first) {
  return min(max(len[agent], 1), Tp) - first;
}

// ---- the pair walk: agent tiles x time chunks of SC_TC segments x partner tiles x partners x segments -------------------
// The chunk of one pair: m = min(m, squared closest approach) over its nseg segments, in ascending order.  own = the lane's
// points t0 .. t0 + nseg of the chunk, q(p) = the partner's point t0 + p (an LDS row, or wherever it lies).  GATED: r0
// advances through every segment and only segment j < lim folds (sc_segment_if); else all of them do (sc_segment; lim is
// not evaluated).  Whole groups of four segments without a branch between them, the tail guarded.
// A macro, not a function: behind a function boundary - partner by functor or by pointer, own by reference or by pointer,
// r0 and m in the caller or in the callee - the dense clearance kernel's groups come out of the scheduler one s_nop longer
// (62 instructions for 61), 1.5 - 1.9 % of the launch on 64-agent scenes (profiles/scene_walk_resource_usage.txt).
#define SC_CHUNK_SEG_(GATED, j, own, q, lim, rx, ry, m)                                  \
  do {                                                                                   \
    if constexpr (GATED) sc_segment_if((j) < (lim), (own)[(j) + 1], q((j) + 1), rx, ry, m); \
    else sc_segment((own)[(j) + 1], q((j) + 1), rx, ry, m);                              \
  } while (0)
#define SC_CHUNK(GATED, own, q, nseg, lim, m)                                            \
  do {                                                                                   \
    const float2 q0_ = q(0);                                                             \
    float rx_ = (own)[0].x - q0_.x, ry_ = (own)[0].y - q0_.y; /* r0 of the first segment */ \
    _Pragma("unroll") for (int t4_ = 0; t4_ < SC_TC; t4_ += 4) {                         \
      if (t4_ + 4 <= (nseg)) {                                                           \
        _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) SC_CHUNK_SEG_(GATED, t4_ + u_, own, q, lim, rx_, ry_, m); \
      } else {                                                                           \
        _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_)                                 \
          if (t4_ + u_ < (nseg)) SC_CHUNK_SEG_(GATED, t4_ + u_, own, q, lim, rx_, ry_, m); \
      }                                                                                  \
    }                                                                                    \
  } while (0)

// the lane's own points of the chunk at t0 into registers (zeros behind the chunk's last point)
__device__ __forceinline__ void sc_load_own(float2 (&own)[SC_NP], const float* __restrict__ pos, int pstride,
                                            const float* __restrict__ start, int sstride, size_t row, int agent, int Tp,
                                            int t0, int nseg) {
#pragma unroll
  for (int p = 0; p < SC_NP; ++p)
    own[p] = p <= nseg ? sc_point(pos, pstride, start, sstride, row, agent, Tp, t0 + p) : float2{0.f, 0.f};
}

// One lane's row of the partner tile: its own points when the partner tile is its tile (same), else the chunk's points of
// (brow, bagent), which the caller has clamped into the scene.  The caller puts a barrier in front (the previous tile has
// been read) and one behind, both outside every lane-dependent condition; `same` is the same in every lane.
__device__ __forceinline__ void sc_stage_row(float2* trow, const float2 (&own)[SC_NP], bool same,
                                             const float* __restrict__ pos, int pstride, const float* __restrict__ start,
                                             int sstride, size_t brow, int bagent, int Tp, int t0, int nseg) {
  if (same) {
#pragma unroll
    for (int p = 0; p < SC_NP; ++p) trow[p] = own[p];
  } else {
#pragma unroll
    for (int p = 0; p < SC_NP; ++p)
      if (p <= nseg) trow[p] = sc_point(pos, pstride, start, sstride, brow, bagent, Tp, t0 + p);
  }
}

// ---- host: what the entry points of the family (scene clearance and its gradient, composition, suppression, plan risk and
// refinement, the wall calls) check of their arguments, each once ----------------------------------------------------------
// Are pos and start readable as paths of float2: pos there, its rows 2 or 4 floats apart and on an 8-byte boundary, and a
// start - when there is one - with rows at least 2 floats apart?
static inline bool sw_paths_ok(const float* pos, int pstride, const float* start, int sstride) {
  return pos && (pstride == 2 || pstride == 4) && !((uintptr_t)pos & 7) && !(start && sstride < 2);
}
// Is d a usable penalty distance: finite and > 0, and d^2 and 1 / d^2 fp32 numbers?  Hands both back.
static inline bool sw_penalty_dist(float d, float& d2, float& inv_d2) {
  d2 = d * d;
  inv_d2 = 1.f / d2;
  return d > 0.f && isfinite(d) && d2 > 0.f && isfinite(d2) && isfinite(inv_d2);
}
