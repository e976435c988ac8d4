// sw_wall_grid.hip - sw_path_walls and sw_wall_grad for maps that do not fit LDS: the walls stay in global memory under a
// uniform grid of cells (socialways_amd.WallGrid), and a path segment visits only the walls listed in the cells its
// bounding box, inflated by `reach`, touches - each of them once.  The pair arithmetic is wl_closest of sw_wall_dev.h and
// nothing else, the decisions are the flat kernels' expressions, the points of a path are sw_scene_dev.h's: a pair that both
// forms visit gives the same bits in both.  The definition is the GRID section of include/socialways_hip.h.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include "sw_wall_dev.h"
#include <math.h>
#include <stdint.h>

#define WQ_THREADS 64          // one wave per workgroup: a lane owns a path, nothing crosses lanes
#define WQ_MAX_CELLS (1 << 20)

struct WqGrid {
  const float4* walls;         // [M] (w0.x, w0.y, w1.x, w1.y)
  const int* cell_ptr;         // [nx ny + 1]
  const int* cell_walls;       // [cell_ptr[nx ny]] wall indices, ascending within a cell
  const int4* wall_cells;      // [M] (ix0, iy0, ix1, iy1): the cells that list the wall
  int nx, ny;
  float x0, y0, inv_cell, reach;
};

// ---- the cells of one axis a segment asks about --------------------------------------------------------------------------------
//   Exact: floor((lo - reach - org) / cell) .. floor((hi + reach - org) / cell).  fp32 forms c = ((lo - reach) - org) * inv_cell
//   with three roundings and inv_cell = fl(1 / cell); with u = 2^-24, t1 = lo - reach, t2 = t1 - org:
//     |c - exact| <= (u |t1| + u |t2|) / cell + 2 u |c|  <=  4 u |c| + u |org| / cell            (|t1| <= |t2| + |org|).
//   The range is widened by SLACK (|c| + |org| inv_cell) with SLACK = 8 u = 2^-21 - twice the bound, which also covers the
//   float64 rounding of the builder's own floor() at a wall that lies on a cell line.  A cell too many costs a list walk and
//   changes no output (the visit-once rule); a cell too few would lose a pair.
//   The clamps come BEFORE the conversion: fmaxf / fminf return the operand that is not NaN.  c is first held inside
//   +-WQ_CMAX (2^22, beyond every grid), so that an infinite or overflowing c stays finite under the slack (inf - inf would be
//   NaN) and a NaN c becomes -WQ_CMAX: a NaN bound gives 0 | -1 (an empty range), a coordinate of +-1e30 or +-inf n | n - 1 on
//   its side; q0 lies in 0 .. n, q1 in -1 .. n - 1, and the loop q0 .. q1 indexes inside the grid or not at all.  n <= 2^20 is
//   exact in fp32.
#define WQ_SLACK 0x1p-21f
#define WQ_CMAX 0x1p22f
__device__ __forceinline__ void wq_axis(float a, float b, float org, float inv_cell, float reach, int n, int& q0, int& q1) {
  const float bias = fabsf(org) * inv_cell;
  const float c0 = fminf(fmaxf(((fminf(a, b) - reach) - org) * inv_cell, -WQ_CMAX), WQ_CMAX);
  const float c1 = fminf(fmaxf(((fmaxf(a, b) + reach) - org) * inv_cell, -WQ_CMAX), WQ_CMAX);
  const float f0 = floorf(c0 - WQ_SLACK * (fabsf(c0) + bias)), f1 = floorf(c1 + WQ_SLACK * (fabsf(c1) + bias));
  q0 = (int)fminf(fmaxf(f0, 0.f), (float)n);
  q1 = (int)fminf(fmaxf(f1, -1.f), (float)(n - 1));
}

// The walk of one counted segment p0 -> p1: the cells of its query range row-major, a cell's list in ascending order, a wall
// only in the first cell its own range shares with the query's.  VISIT(w) sees every wall within reach exactly once.
// A list is read WQ_BATCH entries at a time - the indices, then their ranges and walls, are independent loads in flight
// together (an entry behind the list's end reads the last one again and is not visited); one entry at a time the walk is a chain
// of two dependent global loads per pair and nothing else of the lane's wave hides it.  The order of the visits is unchanged.
#define WQ_BATCH 4
#define WQ_WALK(G, p0, p1, VISIT)                                                                    \
  do {                                                                                               \
    int qx0_, qx1_, qy0_, qy1_;                                                                      \
    wq_axis((p0).x, (p1).x, (G).x0, (G).inv_cell, (G).reach, (G).nx, qx0_, qx1_);                    \
    wq_axis((p0).y, (p1).y, (G).y0, (G).inv_cell, (G).reach, (G).ny, qy0_, qy1_);                    \
    for (int iy_ = qy0_; iy_ <= qy1_; ++iy_)                                                         \
      for (int ix_ = qx0_; ix_ <= qx1_; ++ix_) {                                                     \
        const int c_ = iy_ * (G).nx + ix_;                                                           \
        const int e1_ = (G).cell_ptr[c_ + 1];                                                        \
        for (int e_ = (G).cell_ptr[c_]; e_ < e1_; e_ += WQ_BATCH) {                                  \
          int m_[WQ_BATCH];                                                                          \
          int4 wc_[WQ_BATCH];                                                                        \
          float4 w_[WQ_BATCH];                                                                       \
          _Pragma("unroll") for (int b_ = 0; b_ < WQ_BATCH; ++b_) m_[b_] = (G).cell_walls[min(e_ + b_, e1_ - 1)]; \
          _Pragma("unroll") for (int b_ = 0; b_ < WQ_BATCH; ++b_) {                                  \
            wc_[b_] = (G).wall_cells[m_[b_]];                                                        \
            w_[b_] = (G).walls[m_[b_]];                                                              \
          }                                                                                          \
          _Pragma("unroll") for (int b_ = 0; b_ < WQ_BATCH; ++b_)                                    \
            if (e_ + b_ < e1_ && ix_ == max(wc_[b_].x, qx0_) && iy_ == max(wc_[b_].y, qy0_)) VISIT(w_[b_]); \
        }                                                                                            \
      }                                                                                              \
  } while (0)

struct PwgArgs {
  const float* pos;
  const float* start;
  const int* len;
  int pstride, sstride, B, Tp, NS, first;
  long long R;                 // K * B paths
  float inv_ss, dist, reach2;
};

// ---- the clearance of 64 paths -----------------------------------------------------------------------------------------------
//   The mapping of path_walls_kernel without its wall slices: a lane owns a path, its SC_TC + 1 points of a time chunk in
//   registers, and walks the chunk's segments in ascending order, each through WQ_WALK; a segment behind the path's length is
//   skipped, whatever it holds.  No LDS, no barrier, no atomics: a lane is the one owner of clear[r], first[r], nseg[r].
__global__ __launch_bounds__(WQ_THREADS) void path_walls_grid_kernel(PwgArgs A, WqGrid G, float* __restrict__ clear,
                                                                     int* __restrict__ first, int* __restrict__ nseg) {
  const long long r = (long long)blockIdx.x * WQ_THREADS + threadIdx.x;
  if (r >= A.R) return;                                      // lanes behind the last path write nothing
  const size_t row = (size_t)r;
  const int agent = (int)(row % (size_t)A.B);
  const int lim_all = A.len ? sc_len(A.len, agent, A.Tp, A.first) : A.NS;
  float mn = __builtin_inff();
  int tf = 0x7fffffff, ns = 0;
  for (int t0 = 0; t0 < A.NS; t0 += SC_TC) {
    const int nsg = A.NS - t0 < SC_TC ? A.NS - t0 : SC_TC;
    float2 own[SC_NP];
    sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, row, agent, A.Tp, t0, nsg);
    const int lim = lim_all - t0;                            // countable segments of the path in this chunk (<= 0: none)
#pragma unroll
    for (int j = 0; j < SC_TC; ++j) {
      if (j < nsg && j < lim) {
#define PWG_VISIT(w)                                                       \
  do {                                                                     \
    float s, cx, cy, cc;                                                   \
    wl_closest(own[j], own[j + 1], w, s, cx, cy, cc);                      \
    mn = fminf(mn, cc);                                                    \
    const bool hit = sqrtf(cc) * A.inv_ss < A.dist;                        \
    ns += hit ? 1 : 0;                                                     \
    tf = hit ? min(tf, t0 + j + A.first) : tf;                             \
  } while (0)
        WQ_WALK(G, own[j], own[j + 1], PWG_VISIT);
#undef PWG_VISIT
      }
    }
  }
  clear[r] = mn < A.reach2 ? sqrtf(mn) * A.inv_ss : __builtin_inff();
  first[r] = tf == 0x7fffffff ? -1 : tf;
  nseg[r] = ns;
}

struct WggArgs {
  const float* pos;
  const float* start;
  const int* len;
  int pstride, sstride, dstride, B, Tp, NS, front;
  long long R;                 // K * B paths
  float dw2, inv_dw2, scale;
};

// ---- the penalty and its gradient ----------------------------------------------------------------------------------------------
//   The mapping of wall_grad_kernel without its wall slices: a lane owns a path, the SC_TC + 1 points of a time chunk and as
//   many gradient accumulators in registers.  Segments ascend; within a segment the walls come in WQ_WALK's order; segment j
//   adds k s c to the accumulator of its end point j + 1 and k (1 - s) c to that of its start point j, k = -4 u / dw^2, through
//   selects.  phi is summed per segment, then added.  One read-modify-write of the chunk's dpos rows, as in wall_grad_kernel:
//   only if one of the chunk's pairs was counted, and only of the points a counted segment can reach.  The order of every
//   sum depends on the path, the map and the grid alone: two calls give the same bits, and a path does not see its batch.
__global__ __launch_bounds__(WQ_THREADS) void wall_grad_grid_kernel(WggArgs A, WqGrid G, float* __restrict__ dpos,
                                                                    float* __restrict__ loss, int* __restrict__ count) {
  const long long r = (long long)blockIdx.x * WQ_THREADS + threadIdx.x;
  if (r >= A.R) return;
  const size_t row = (size_t)r;
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
    const int lim = lim_all - t0;
    int hit = 0;                                             // counted (segment, wall)s of this chunk
#pragma unroll
    for (int j = 0; j < SC_TC; ++j) {
      if (j < nsg && j < lim) {
        float sphi = 0.f;                                    // the segment's phi: summed apart, then added
#define WGG_VISIT(w)                                                       \
  do {                                                                     \
    float s, cx, cy, cc;                                                   \
    wl_closest(own[j], own[j + 1], w, s, cx, cy, cc);                      \
    const bool on = cc < A.dw2;                                            \
    const float u = on ? fmaxf(1.f - cc * A.inv_dw2, 0.f) : 0.f;           \
    const float k = -4.f * u * A.inv_dw2;                                  \
    const float wx = k * cx, wy = k * cy;                                  \
    g[j + 1].x += on ? s * wx : 0.f;                                       \
    g[j + 1].y += on ? s * wy : 0.f;                                       \
    g[j].x += on ? (1.f - s) * wx : 0.f;                                   \
    g[j].y += on ? (1.f - s) * wy : 0.f;                                   \
    sphi += u * u;                                                         \
    hit += on ? 1 : 0;                                                     \
  } while (0)
        WQ_WALK(G, own[j], own[j + 1], WGG_VISIT);
#undef WGG_VISIT
        phi += sphi;
      }
    }
    cnt += hit;
    if (hit) {
#pragma unroll
      for (int p = 0; p < SC_NP; ++p) {
        const int dr = t0 + p - A.front;                     // dpos row of point p: the start point is data and has none
        if (p <= nsg && p <= lim && dr >= 0) {
          float2* d = reinterpret_cast<float2*>(dpos + ((size_t)r * A.Tp + dr) * A.dstride);
          float2 v = *d;
          v.x += A.scale * g[p].x;
          v.y += A.scale * g[p].y;
          *d = v;
        }
      }
    }
  }
  if (loss) loss[r] = phi;
  if (count) count[r] = cnt;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// What both entries check of the grid (nothing behind the pointers: the builder validated what they hold): -> SW_OK | SW_EARG
static int wq_grid_ok(const float* walls, int M, const int* cell_ptr, const int* cell_walls, const int* wall_cells, int nx,
                      int ny, float x0, float y0, float inv_cell, float reach, float& reach2) {
  reach2 = reach * reach;
  if (M < 0 || !cell_ptr || (M > 0 && (!walls || !cell_walls || !wall_cells))) return SW_EARG;
  if (((uintptr_t)walls & 15) || ((uintptr_t)wall_cells & 15)) return SW_EARG;       // read as float4 / int4
  if (nx < 1 || ny < 1 || (long long)nx * ny > WQ_MAX_CELLS) return SW_EARG;
  if (!isfinite(x0) || !isfinite(y0) || !(inv_cell > 0.f) || !isfinite(inv_cell)) return SW_EARG;
  if (!(reach > 0.f) || !isfinite(reach) || !(reach2 > 0.f) || !isfinite(reach2)) return SW_EARG;
  return SW_OK;
}
// Is the distance d (in the walls' coordinates) below reach by the relative margin 1e-5?
static inline bool wq_within(double d, float reach) { return d <= (double)reach * (1.0 - 1e-5); }

static WqGrid wq_grid(const float* walls, const int* cell_ptr, const int* cell_walls, const int* wall_cells, int nx, int ny,
                      float x0, float y0, float inv_cell, float reach) {
  WqGrid G = {};
  G.walls = reinterpret_cast<const float4*>(walls); G.cell_ptr = cell_ptr; G.cell_walls = cell_walls;
  G.wall_cells = reinterpret_cast<const int4*>(wall_cells);
  G.nx = nx; G.ny = ny; G.x0 = x0; G.y0 = y0; G.inv_cell = inv_cell; G.reach = reach;
  return G;
}

extern "C" int sw_path_walls_grid(const float* pos, int pstride, const float* start, int sstride, const int* len, int K, int B,
                                  int Tp, const float* walls, int M, const int* cell_ptr, const int* cell_walls,
                                  const int* wall_cells, int nx, int ny, float x0, float y0, float inv_cell, float reach,
                                  float inv_ss, float dist, float* clear, int* first, int* nseg, void* stream) {
  float reach2;
  if (!sw_paths_ok(pos, pstride, start, sstride) || !clear || !first || !nseg) return SW_EARG;
  if (K < 1 || B < 0 || Tp < 1 || !(inv_ss > 0.f) || !(dist >= 0.f)) return SW_EARG;
  if (wq_grid_ok(walls, M, cell_ptr, cell_walls, wall_cells, nx, ny, x0, y0, inv_cell, reach, reach2) != SW_OK) return SW_EARG;
  if (!wq_within((double)dist / (double)inv_ss, reach)) return SW_EARG;
  if (B == 0) return SW_OK;
  const long long R = (long long)K * B;
  if ((R + WQ_THREADS - 1) / WQ_THREADS > 0x7fffffffLL) return SW_EARG;
  PwgArgs A = {};
  A.pos = pos; A.start = start; A.len = len;
  A.pstride = pstride; A.sstride = sstride; A.B = B; A.Tp = Tp; A.R = R;
  A.first = start ? 0 : 1;
  A.NS = Tp - A.first;
  A.inv_ss = inv_ss; A.dist = dist; A.reach2 = reach2;
  const WqGrid G = wq_grid(walls, cell_ptr, cell_walls, wall_cells, nx, ny, x0, y0, inv_cell, reach);
  SW_LAUNCH(path_walls_grid_kernel, dim3((unsigned)((R + WQ_THREADS - 1) / WQ_THREADS)), dim3(WQ_THREADS), 0,
            (hipStream_t)stream, A, G, clear, first, nseg);
  SW_CHECK_LAUNCH("path_walls_grid_kernel");
  return SW_OK;
}

extern "C" int sw_wall_grad_grid(const float* pos, int pstride, const float* start, int sstride, const int* len, int K, int B,
                                 int Tp, const float* walls, int M, const int* cell_ptr, const int* cell_walls,
                                 const int* wall_cells, int nx, int ny, float x0, float y0, float inv_cell, float reach, float dw,
                                 float scale, float* dpos, int dstride, float* loss, int* count, void* stream) {
  float dw2, inv_dw2, reach2;
  if (!sw_paths_ok(pos, pstride, start, sstride) || !sw_penalty_dist(dw, dw2, inv_dw2) || !isfinite(scale)) return SW_EARG;
  if (!dpos || K < 1 || B < 0 || Tp < 1) return SW_EARG;
  if ((dstride != 2 && dstride != 4) || ((uintptr_t)dpos & 7)) return SW_EARG;       // rows are written as float2
  if (wq_grid_ok(walls, M, cell_ptr, cell_walls, wall_cells, nx, ny, x0, y0, inv_cell, reach, reach2) != SW_OK) return SW_EARG;
  if (!wq_within((double)dw, reach)) return SW_EARG;
  if (B == 0) return SW_OK;
  const long long R = (long long)K * B;
  if ((R + WQ_THREADS - 1) / WQ_THREADS > 0x7fffffffLL) return SW_EARG;
  WggArgs A = {};
  A.pos = pos; A.start = start; A.len = len;
  A.pstride = pstride; A.sstride = sstride; A.dstride = dstride; A.B = B; A.Tp = Tp; A.R = R;
  A.front = start ? 1 : 0;                                   // points in front of pos row 0
  A.NS = Tp - 1 + A.front;                                   // segments of a path
  A.dw2 = dw2; A.inv_dw2 = inv_dw2; A.scale = scale;
  const WqGrid G = wq_grid(walls, cell_ptr, cell_walls, wall_cells, nx, ny, x0, y0, inv_cell, reach);
  SW_LAUNCH(wall_grad_grid_kernel, dim3((unsigned)((R + WQ_THREADS - 1) / WQ_THREADS)), dim3(WQ_THREADS), 0,
            (hipStream_t)stream, A, G, dpos, loss, count);
  SW_CHECK_LAUNCH("wall_grad_grid_kernel");
  return SW_OK;
}
