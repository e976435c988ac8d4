// sw_scene_dev.h - the device pieces sw_scene.hip and sw_compose.hip share: the points of a path, the closest approach
// of two linearly moving points within one segment, and the lane layout of a scene.  Both files form a clearance from
// these and nothing else, so a clearance of sw_scene_compose carries the bits sw_scene_clearance gives the same two paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

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
