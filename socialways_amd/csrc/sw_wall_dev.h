// sw_wall_dev.h - the device piece sw_walls.hip and sw_plan_refine.hip share: the closest approach of a point that moves
// linearly through one segment to a static wall (a line segment; a zero-length one is a post), by the five candidates of
// include/socialways_hip.h in their fixed order.  Both kernels form a wall distance from this function and nothing else, so
// the same two geometries give the same bits in both.
#pragma once
#include <hip/hip_runtime.h>

#define WL_MAX SW_WALLS_MAX    // walls of a call: 16 bytes each in LDS

__device__ __forceinline__ float wl_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// the walls of a call into LDS (w0.x, w0.y, w1.x, w1.y); the caller puts the barrier behind
__device__ __forceinline__ void wl_stage(float4* dst, const float* __restrict__ walls, int M, int tid, int nthreads) {
  for (int m = tid; m < M; m += nthreads) dst[m] = float4{walls[4 * m], walls[4 * m + 1], walls[4 * m + 2], walls[4 * m + 3]};
}

// p0 -> p1 against the wall w = (w0, w1): s = where on the path segment the closest approach lies, (cx, cy) = c = the path
// point minus the wall point there, cc = |c|^2.  A later candidate replaces the best one only by a strictly smaller |c|^2;
// NaN compares false and replaces nothing.  The reciprocals are the hardware's (1 ulp), as in sc_segment: u and s only place
// a point on a segment.
__device__ __forceinline__ void wl_closest(float2 p0, float2 p1, float4 w, float& s, float& cx, float& cy, float& cc) {
  const float fx = w.z - w.x, fy = w.w - w.y;                // f = w1 - w0
  const float ex = p1.x - p0.x, ey = p1.y - p0.y;            // e = p1 - p0
  const float ff = fx * fx + fy * fy, ee = ex * ex + ey * ey;
  const float rf = __builtin_amdgcn_rcpf(ff), re = __builtin_amdgcn_rcpf(ee);
  const float ax = p0.x - w.x, ay = p0.y - w.y;              // p0 - w0
  const float bx = p1.x - w.x, by = p1.y - w.y;              // p1 - w0
  const float hx = p0.x - w.z, hy = p0.y - w.w;              // p0 - w1
  // 1: s = 0, p0 against the wall
  float u = ff > 0.f ? wl_clamp01((ax * fx + ay * fy) * rf) : 0.f;
  cx = ax - u * fx;
  cy = ay - u * fy;
  cc = cx * cx + cy * cy;
  s = 0.f;
  // 2: s = 1, p1 against the wall
  u = ff > 0.f ? wl_clamp01((bx * fx + by * fy) * rf) : 0.f;
  float tx = bx - u * fx, ty = by - u * fy, tc = tx * tx + ty * ty;
  bool lt = tc < cc;
  s = lt ? 1.f : s; cx = lt ? tx : cx; cy = lt ? ty : cy; cc = lt ? tc : cc;
  // 3: the end w0 against the path
  float t = ee > 0.f ? wl_clamp01(-(ax * ex + ay * ey) * re) : 0.f;
  tx = ax + t * ex; ty = ay + t * ey; tc = tx * tx + ty * ty;
  lt = tc < cc;
  s = lt ? t : s; cx = lt ? tx : cx; cy = lt ? ty : cy; cc = lt ? tc : cc;
  // 4: the end w1 against the path
  t = ee > 0.f ? wl_clamp01(-(hx * ex + hy * ey) * re) : 0.f;
  tx = hx + t * ex; ty = hy + t * ey; tc = tx * tx + ty * ty;
  lt = tc < cc;
  s = lt ? t : s; cx = lt ? tx : cx; cy = lt ? ty : cy; cc = lt ? tc : cc;
  // 5: a proper crossing: both pairs of cross products have strictly opposite signs
  const float d1 = fx * ay - fy * ax, d2 = fx * by - fy * bx;      // f x (p0 - w0), f x (p1 - w0)
  const float d3 = ey * ax - ex * ay, d4 = ey * hx - ex * hy;      // e x (w0 - p0), e x (w1 - p0)
  const bool cross = ((d1 < 0.f && d2 > 0.f) || (d1 > 0.f && d2 < 0.f)) && ((d3 < 0.f && d4 > 0.f) || (d3 > 0.f && d4 < 0.f));
  lt = cross && 0.f < cc;
  t = d1 * __builtin_amdgcn_rcpf(d1 - d2);
  s = lt ? t : s; cx = lt ? 0.f : cx; cy = lt ? 0.f : cy; cc = lt ? 0.f : cc;
}
