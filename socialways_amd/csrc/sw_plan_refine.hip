// sw_plan_refine.hip - gradient descent on the expected clearance penalty of candidate ego paths against the K sampled
// futures of a scene, every iteration inside one launch: per (query, plan) the penalty of sw_clearance_grad against every
// (draw, agent) path, averaged over the draws (the draws of different agents are independent given the observations), plus a
// tracking and a smoothness term - and, in the instance with walls, the penalty of the plan's own segments against a static
// map of line segments (sw_wall_dev.h).  The segment arithmetic is sw_scene_dev.h's; the lane layout is sw_plan_risk.hip's.
// Does not depend on the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include "sw_wall_dev.h"
#include <math.h>
#include <stdint.h>

#define RF_MAXK 4096
#define RF_MAXT 1024
#define RF_MAXIT 1024
#define RF_THREADS 256
#define RF_WAVES (RF_THREADS / 64)

struct RfArgs {
  const float* pos;
  const float* start;
  const int* scene_off;
  const int* len;
  const float* plans;
  const float* plan_start;
  const int* q_scene;
  const int* q_ego;
  int pstride, sstride, S, B, K, Tp, P;
  int Kb, APB;                 // draws and agents of a lane batch (Kb * APB <= 256)
  int n_iter;
  float inv_ss, d02, inv_d02, inv_K, lr, wt2, ws2, cap, cap2;      // wt2 = 2 w_track, ws2 = 2 w_smooth, cap = max_move d0
  // the instance with walls only
  const float* walls;
  int M, NSL, NW;              // walls, wall slices (NSL * Tp <= 256, or 1), walls of a slice = ceil(M / NSL)
  float dw2, inv_dw2, ww;      // ww = w_wall d0^2 / dw^2
};

// LDS of a workgroup: three rows of Tp + 2 points (X0, and X twice: an iteration reads one and writes the other) and one row
// of partial gradients per wave, each with a slot behind its last point that takes the stores of idle lanes; then 4 floats
// for the block sums.
__host__ __device__ constexpr int rf_row(int Tp) { return Tp + 2; }
__host__ __device__ constexpr int rf_lds_bytes(int Tp) { return 8 * (3 + RF_WAVES) * rf_row(Tp) + 16; }
// With walls, behind that (rounded up to 16 bytes): the M walls, then per (wall slice, plan segment) the shares of the
// segment's two end points in the slice's wall gradient - two arrays of NSL * Tp float2, each with a slot behind its last
// element that takes the stores of idle threads.
__host__ __device__ constexpr int rf_wall_slices(int Tp) { return Tp < RF_THREADS ? RF_THREADS / Tp : 1; }
__host__ __device__ constexpr int rf_wall_off(int Tp) { return (rf_lds_bytes(Tp) + 15) & ~15; }
__host__ __device__ constexpr int rf_lds_bytes_walls(int Tp, int M) { return rf_wall_off(Tp) + 16 * M + 2 * 8 * (rf_wall_slices(Tp) * Tp + 1); }

// acc_i = x_{i+1} - 2 x_i + x_{i-1} for 1 <= i <= Tp - 1, else 0: clamped reads, the value selected afterwards
__device__ __forceinline__ float2 rf_acc(const float2* x, int i, int Tp) {
  const int ic = min(max(i, 1), Tp > 1 ? Tp - 1 : 1);
  const float2 a = x[ic - 1], b = x[ic], c = x[ic + 1 <= Tp ? ic + 1 : Tp];
  const bool on = i >= 1 && i <= Tp - 1;
  return float2{on ? c.x - 2.f * b.x + a.x : 0.f, on ? c.y - 2.f * b.y + a.y : 0.f};
}

// The sum of v over the 64 lanes of a wave, in every lane: the DPP reduction (neighbours inside a quad, row shifts by 4 and 8,
// then the row broadcasts 15 and 31; a lane without a source adds 0) leaves the total in lane 63, which is read back as a
// scalar.  VALU only - a __shfl_xor butterfly goes through the LDS crossbar (ds_bpermute_b32), and with 2 (SC_TC + 1) sums per
// chunk and sixteen waves on a CU that crossbar was what the evaluation waited for.  The order of the additions is fixed.
// Every lane of the wave must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float rf_dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float rf_wave_sum(float v) {
  v = rf_dpp_add<0xb1, 0xf>(v);                              // quad_perm:[1,0,3,2]
  v = rf_dpp_add<0x4e, 0xf>(v);                              // quad_perm:[2,3,0,1]
  v = rf_dpp_add<0x114, 0xf>(v);                             // row_shr:4
  v = rf_dpp_add<0x118, 0xf>(v);                             // row_shr:8: lane 15 of every row holds the row's sum
  v = rf_dpp_add<0x142, 0xa>(v);                             // row_bcast:15 into rows 1 and 3
  v = rf_dpp_add<0x143, 0xc>(v);                             // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- the refinement of one plan (definitions in include/socialways_hip.h) ---------------------------------------------------
//   One 256-thread workgroup per (query, plan).  A lane owns a (agent, draw) pair, laid out as in plan_risk_kernel (lane =
//   al * Kb + kk, Kb = min(K, 256), 256 / Kb agents per batch); larger scenes loop over agent groups, more than 256 draws over
//   draw groups.  The lane's own SC_TC + 1 points sit in registers; when the scene is one lane batch and the path one time
//   chunk they are loaded once and stay there across all iterations.  An EVALUATION walks the lane's path against the current
//   X (read from LDS, every lane the same address): per segment the arithmetic of clearance_grad_kernel, the two end points'
//   shares into the lane's SC_TC + 1 accumulators, every contribution gated by a select.  Per chunk the accumulators are
//   summed over the wave (rf_wave_sum: every lane gets the same sum, taken in a fixed order), lane p keeps the sum of
//   point p and ALL lanes add what they keep to the wave's row in LDS - idle lanes to the slot behind the row: no memory
//   operation under a lane-dependent branch inside the iteration loop.  A point on a chunk boundary takes two such adds, in
//   program order.  Behind a barrier a thread per waypoint adds the waves' rows 0 .. 3 in that order, clears them, adds the
//   quadratic terms, caps the step and writes the other copy of X; a second barrier ends the iteration.  There are
//   n_iter + 1 evaluations: the first also gives the costs of X0, the last only the costs of the result.  Every barrier sits in
//   uniform control flow; there is no early exit at all - a query without agents runs the loops over no lanes' worth of work.
//   WALLS (sw_plan_refine_walls; the instance without is sw_plan_refine's and carries none of this): every evaluation also
//   walks the plan's OWN segments against the walls, staged in LDS once.  Tp is usually 12 and M tens to hundreds, so the work
//   item is a (wall slice c, plan segment s) pair, item = c * Tp + s over the workgroup's threads, NSL = 256 / Tp slices (1
//   above 256 steps, the threads then loop over the segments); slice c takes the walls c, c + NSL, ... in ascending order,
//   every item ceil(M / NSL) of them with the index clamped and the contribution selected, so the trip count is uniform.  The
//   item writes the two end points' shares of its slice to LDS (an idle thread to the slot behind); behind the barrier the
//   thread of waypoint t adds, slices ascending, the share of segment t-1's second end and of segment t's first end.
template <bool WALLS>
__global__ __launch_bounds__(RF_THREADS) void plan_refine_kernel(RfArgs A, float* __restrict__ out, float* __restrict__ cost,
                                                                 float* __restrict__ moved) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x / A.P;
  const int Tp = A.Tp, ROW = rf_row(Tp), TRASH = Tp + 1;

  float2* x0 = reinterpret_cast<float2*>(rf_lds);
  float2* xc = x0 + ROW;                                     // the current X
  float2* xn = xc + ROW;                                     // the next one
  float2* gw = xn + ROW;                                     // RF_WAVES rows
  float* red = reinterpret_cast<float*>(gw + RF_WAVES * ROW);
  float2* gmine = gw + wave * ROW;
  float4* wl = reinterpret_cast<float4*>(rf_lds + rf_wall_off(Tp));      // WALLS only
  const int NIT = WALLS ? A.NSL * Tp : 0;                    // (slice, segment) items; slot NIT takes the idle stores
  float2* wg0 = reinterpret_cast<float2*>(wl + (WALLS ? A.M : 0));
  float2* wg1 = wg0 + NIT + 1;

  const int sc = A.q_scene[q];
  int s0 = 0, n = 0;
  if (sc >= 0 && sc < A.S) {
    const int b0 = A.scene_off[sc], b1 = A.scene_off[sc + 1];
    if (b0 >= 0 && b1 >= b0 && b1 <= A.B) {                  // offsets outside the batch: read nothing
      s0 = b0;
      n = b1 - b0;
    }
  }
  const int ego = A.q_ego ? A.q_ego[q] : -1;

  const float2* gplan = reinterpret_cast<const float2*>(A.plans) + (size_t)blockIdx.x * Tp;
  const float2 pstart = float2{A.plan_start[(size_t)q * 2], A.plan_start[(size_t)q * 2 + 1]};
  for (int i = tid; i < ROW; i += RF_THREADS) {
    const float2 g0 = gplan[(i < 1 ? 1 : i <= Tp ? i : Tp) - 1];
    const float2 v = i == 0 ? pstart : g0;
    x0[i] = v;
    xc[i] = v;
    xn[i] = v;
  }
  for (int i = tid; i < RF_WAVES * ROW; i += RF_THREADS) gw[i] = float2{0.f, 0.f};
  if constexpr (WALLS) wl_stage(wl, A.walls, A.M, tid, RF_THREADS);
  __syncthreads();

  const int al = tid / A.Kb, kk = tid - al * A.Kb;
  const bool resident = Tp <= SC_TC && n > 0 && n <= A.APB && A.K <= A.Kb;      // uniform
  float2 own[SC_NP];
  if (resident) {
    const int arow = s0 + (al < n ? al : n - 1);
    sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, (size_t)(kk < A.K ? kk : A.K - 1) * A.B + arow, arow, Tp, 0, Tp);
  }

  for (int it = 0;; ++it) {
    // ---- evaluation: the penalty of xc and its gradient into the waves' rows ------------------------------------------------
    float phi = 0.f;
    for (int a0 = 0; a0 < n; a0 += A.APB) {
      const int a = a0 + al, ac = a < n ? a : n - 1;
      const int arow = s0 + ac;
      const int va = A.len ? sc_len(A.len, arow, Tp, 0) : Tp;      // countable segments of the agent
      for (int k0 = 0; k0 < A.K; k0 += A.Kb) {
        const int k = k0 + kk, kc = k < A.K ? k : A.K - 1;
        const bool valid = al < A.APB && a < n && k < A.K && arow != ego;
        const size_t row = (size_t)kc * A.B + arow;
        for (int t0 = 0; t0 < Tp; t0 += SC_TC) {
          const int nseg = Tp - t0 < SC_TC ? Tp - t0 : SC_TC;
          if (!resident) sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, row, arow, Tp, t0, nseg);
          float2 g[SC_NP];
#pragma unroll
          for (int p = 0; p < SC_NP; ++p) g[p] = float2{0.f, 0.f};
          const float2* xq = xc + t0;
          const float2 q0 = xq[0];
          float rx = own[0].x - q0.x, ry = own[0].y - q0.y;  // r0 of the chunk's first segment
          const int lim = va - t0;                           // countable segments of the pair in this chunk (<= 0: none)
          float cphi = 0.f;                                  // the chunk's phi: summed apart, then added
#pragma unroll
          for (int j = 0; j < SC_TC; ++j) {
            if (j < nseg) {                                  // uniform
              float tau, cx, cy;
              sc_segment_at(own[j + 1], xq[j + 1], rx, ry, tau, cx, cy);
              const float cc = cx * cx + cy * cy;
              const bool on = valid && j < lim && cc < A.d02;
              const float u = fmaxf(1.f - cc * A.inv_d02, 0.f);
              const float wx = 4.f * u * cx, wy = 4.f * u * cy;
              g[j + 1].x += on ? tau * wx : 0.f;
              g[j + 1].y += on ? tau * wy : 0.f;
              g[j].x += on ? (1.f - tau) * wx : 0.f;
              g[j].y += on ? (1.f - tau) * wy : 0.f;
              cphi += on ? u * u : 0.f;
            }
          }
          phi += cphi;
          float2 keep = float2{0.f, 0.f};                    // lane p: the wave's sum of point p of the chunk
#pragma unroll
          for (int p = 0; p < SC_NP; ++p) {
            if (p <= nseg) {                                 // uniform
              const float vx = rf_wave_sum(g[p].x), vy = rf_wave_sum(g[p].y);
              keep.x = lane == p ? vx : keep.x;
              keep.y = lane == p ? vy : keep.y;
            }
          }
          float2* slot = gmine + (lane <= nseg ? t0 + lane : TRASH);
          float2 acc = *slot;
          acc.x += keep.x;
          acc.y += keep.y;
          *slot = acc;
        }
      }
    }

    float wphi = 0.f;
    if constexpr (WALLS) {
      // ---- the walls: item (c, s) = segment s of xc against the walls of slice c -------------------------------------------
      for (int ib = 0; ib < NIT; ib += RF_THREADS) {
        const int i = ib + tid, ic = i < NIT ? i : NIT - 1;
        const int c = ic / Tp, s = ic - c * Tp;
        const float2 p0 = xc[s], p1 = xc[s + 1];
        float2 g0 = float2{0.f, 0.f}, g1 = float2{0.f, 0.f};
        for (int jw = 0; jw < A.NW; ++jw) {                  // uniform
          const int m = c + jw * A.NSL, mc = m < A.M ? m : A.M - 1;
          float sw_, cx, cy, cc;
          wl_closest(p0, p1, wl[mc], sw_, cx, cy, cc);
          const bool on = i < NIT && m < A.M && cc < A.dw2;
          const float u = fmaxf(1.f - cc * A.inv_dw2, 0.f);
          const float wx = -4.f * u * cx, wy = -4.f * u * cy;
          g1.x += on ? sw_ * wx : 0.f;
          g1.y += on ? sw_ * wy : 0.f;
          g0.x += on ? (1.f - sw_) * wx : 0.f;
          g0.y += on ? (1.f - sw_) * wy : 0.f;
          wphi += on ? u * u : 0.f;
        }
        const int slot = i < NIT ? i : NIT;                  // slot NIT is write-only: whatever the idle threads leave there is never read
        wg0[slot] = g0;
        wg1[slot] = g1;
      }
    }

    const bool first = it == 0, last = it == A.n_iter;       // uniform
    if (first || last) {
      // the costs of xc: pen | trk / d0^2 | smo / d0^2, and the largest displacement
      float trk = 0.f, smo = 0.f, far = 0.f;
      for (int tb = 0; tb < Tp; tb += RF_THREADS) {
        const int t = tb + tid + 1, tc = t <= Tp ? t : Tp;
        const bool on = t <= Tp;
        const float2 x = xc[tc], xo = x0[tc];
        const float dx = x.x - xo.x, dy = x.y - xo.y;
        const float2 ac = rf_acc(xc, tc, Tp);
        const float d2 = dx * dx + dy * dy;
        trk += on ? d2 : 0.f;
        smo += on ? ac.x * ac.x + ac.y * ac.y : 0.f;
        far = on ? fmaxf(far, d2) : far;
      }
      const float pen = sw_block_sum(phi, red) * A.inv_K;
      trk = sw_block_sum(trk, red) * A.inv_d02;
      smo = sw_block_sum(smo, red) * A.inv_d02;
      constexpr int NC = WALLS ? 4 : 3;
      float wpen = 0.f;
      if constexpr (WALLS) wpen = sw_block_sum(wphi, red);
      float* c = cost + (size_t)blockIdx.x * (2 * NC);
      if (first && tid == 0) {
        c[0] = pen; c[1] = trk; c[2] = smo;
        if constexpr (WALLS) c[3] = wpen;
      }
      if (last) {
        far = sw_block_max(far, red);
        if (tid == 0) {
          c[NC] = pen; c[NC + 1] = trk; c[NC + 2] = smo;
          if constexpr (WALLS) c[NC + 3] = wpen;
          moved[blockIdx.x] = sqrtf(far) * A.inv_ss;
        }
        break;
      }
    }
    __syncthreads();                                         // the waves' rows are complete

    // ---- update: a thread per waypoint ------------------------------------------------------------------------------------
    for (int tb = 0; tb < Tp; tb += RF_THREADS) {
      const int t = tb + tid + 1, tc = t <= Tp ? t : Tp;
      float gx = 0.f, gy = 0.f;
#pragma unroll
      for (int w = 0; w < RF_WAVES; ++w) {                   // waves 0 .. 3 in order
        const float2 v = gw[w * ROW + tc];
        gx += v.x;
        gy += v.y;
        gw[w * ROW + (t <= Tp ? t : TRASH)] = float2{0.f, 0.f};      // its owner clears the column; what an idle thread read goes nowhere
      }
      const float2 x = xc[tc], xo = x0[tc];
      const float2 am = rf_acc(xc, tc - 1, Tp), a0 = rf_acc(xc, tc, Tp), ap = rf_acc(xc, tc + 1, Tp);
      float sx, sy;
      if constexpr (WALLS) {
        float hx = 0.f, hy = 0.f;                            // the wall gradient of waypoint tc, slices ascending
        const bool inner = tc < Tp;                          // segment tc exists: its first end is waypoint tc
        const int s1 = inner ? tc : Tp - 1;
        for (int c = 0; c < A.NSL; ++c) {
          const float2 v1 = wg1[c * Tp + tc - 1], v0 = wg0[c * Tp + s1];
          hx += v1.x;
          hy += v1.y;
          hx += inner ? v0.x : 0.f;
          hy += inner ? v0.y : 0.f;
        }
        // the wall term LAST, behind the sum the instance without walls forms: a wall gradient of 0 leaves that sum's bits
        sx = A.lr * ((gx * A.inv_K + A.wt2 * (x.x - xo.x) + A.ws2 * (am.x - 2.f * a0.x + ap.x)) + A.ww * hx);
        sy = A.lr * ((gy * A.inv_K + A.wt2 * (x.y - xo.y) + A.ws2 * (am.y - 2.f * a0.y + ap.y)) + A.ww * hy);
      } else {
        sx = A.lr * (gx * A.inv_K + A.wt2 * (x.x - xo.x) + A.ws2 * (am.x - 2.f * a0.x + ap.x));
        sy = A.lr * (gy * A.inv_K + A.wt2 * (x.y - xo.y) + A.ws2 * (am.y - 2.f * a0.y + ap.y));
      }
      const float n2 = sx * sx + sy * sy;
      const float sc_ = n2 > A.cap2 ? A.cap / sqrtf(n2) : 1.f;
      sx = n2 > A.cap2 ? sx * sc_ : sx;
      sy = n2 > A.cap2 ? sy * sc_ : sy;
      xn[t <= Tp ? t : TRASH] = float2{x.x - sx, x.y - sy};
    }
    float2* sw = xc;
    xc = xn;
    xn = sw;
    __syncthreads();
  }

  float2* o = reinterpret_cast<float2*>(out) + (size_t)blockIdx.x * Tp;
  for (int i = tid; i < Tp; i += RF_THREADS) o[i] = xc[i + 1];
}

// the argument checks and the launch of both entry points; walls == NULL with M < 0: the instance without walls
static int rf_run(const float* pos, int pstride, const float* start, int sstride, const int* scene_off, const int* len, int S,
                  int B, int K, int Tp, const float* plans, const float* plan_start, const int* q_scene, const int* q_ego, int Q,
                  int P, float inv_ss, float d0, int n_iter, float lr, float w_track, float w_smooth, float max_move,
                  const float* walls, int M, float dw, float w_wall, float* out, float* cost, float* moved, void* stream) {
  const bool with_walls = M >= 0;
  float d02, inv_d02, dw2 = 1.f, inv_dw2 = 1.f;
  if (!start || !sw_paths_ok(pos, pstride, start, sstride) || !sw_penalty_dist(d0, d02, inv_d02)) return SW_EARG;
  if (!scene_off || !plan_start || !q_scene || !out || !cost || !moved) return SW_EARG;
  if (!plans || ((uintptr_t)plans & 7)) return SW_EARG;                              // plans are read as float2
  if (S < 0 || B < 0 || Q < 0 || K < 1 || Tp < 1 || P < 1 || !(inv_ss > 0.f)) return SW_EARG;
  if (n_iter < 0 || n_iter > RF_MAXIT) return SW_EARG;
  const float par[4] = {lr, w_track, w_smooth, max_move};
  for (float v : par)
    if (!(v >= 0.f) || !isfinite(v)) return SW_EARG;
  if (with_walls) {
    if (M > 0 && !walls) return SW_EARG;
    if (!sw_penalty_dist(dw, dw2, inv_dw2) || !(w_wall >= 0.f) || !isfinite(w_wall) || !isfinite(w_wall * (d02 / dw2))) return SW_EARG;
  }
  if (K > RF_MAXK || Tp > RF_MAXT) return SW_ESHAPE;
  if (with_walls && M > SW_WALLS_MAX) return SW_ESHAPE;
  if (Q == 0) return SW_OK;
  if ((long long)Q * P > 0x7fffffffLL) return SW_EARG;
  RfArgs A = {};
  A.pos = pos; A.start = start; A.scene_off = scene_off; A.len = len; A.plans = plans; A.plan_start = plan_start;
  A.q_scene = q_scene; A.q_ego = q_ego;
  A.pstride = pstride; A.sstride = sstride; A.S = S; A.B = B; A.K = K; A.Tp = Tp; A.P = P;
  A.Kb = K < RF_THREADS ? K : RF_THREADS;
  A.APB = RF_THREADS / A.Kb;
  A.n_iter = n_iter;
  A.inv_ss = inv_ss; A.d02 = d02; A.inv_d02 = inv_d02; A.inv_K = 1.f / (float)K;
  A.lr = lr; A.wt2 = 2.f * w_track; A.ws2 = 2.f * w_smooth;
  A.cap = max_move * d0;
  A.cap2 = A.cap * A.cap;                                    // +inf for a huge max_move: no step is capped
  if (!with_walls) {
    const int lds = rf_lds_bytes(Tp);                        // 57 472 bytes at Tp = 1024: inside the default limit
    SW_LAUNCH_AS("plan_refine_kernel", plan_refine_kernel<false>, dim3((unsigned)(Q * P)), dim3(RF_THREADS), lds,
                 (hipStream_t)stream, A, out, cost, moved);
    SW_CHECK_LAUNCH("plan_refine_kernel");
    return SW_OK;
  }
  A.walls = walls; A.M = M;
  A.NSL = rf_wall_slices(Tp);
  A.NW = (M + A.NSL - 1) / A.NSL;
  A.dw2 = dw2; A.inv_dw2 = inv_dw2; A.ww = w_wall * (d02 / dw2);
  static_assert(rf_lds_bytes_walls(RF_MAXT, SW_WALLS_MAX) <= 160 * 1024, "the largest plan and map fit the LDS of a CU");
  const int lds = rf_lds_bytes_walls(Tp, M);                 // 90 256 bytes at Tp = 1024, M = 1024
  if (lds > 160 * 1024) return SW_ESHAPE;
  static int have = 0;
  if (int rc = sw_set_lds((const void*)plan_refine_kernel<true>, lds, have)) return rc;
  SW_LAUNCH_AS("plan_refine_walls_kernel", plan_refine_kernel<true>, dim3((unsigned)(Q * P)), dim3(RF_THREADS), lds,
               (hipStream_t)stream, A, out, cost, moved);
  SW_CHECK_LAUNCH("plan_refine_walls_kernel");
  return SW_OK;
}

extern "C" int sw_plan_refine(const float* pos, int pstride, const float* start, int sstride, const int* scene_off,
                              const int* len, int S, int B, int K, int Tp, const float* plans, const float* plan_start,
                              const int* q_scene, const int* q_ego, int Q, int P, float inv_ss, float d0, int n_iter, float lr,
                              float w_track, float w_smooth, float max_move, float* out, float* cost, float* moved,
                              void* stream) {
  return rf_run(pos, pstride, start, sstride, scene_off, len, S, B, K, Tp, plans, plan_start, q_scene, q_ego, Q, P, inv_ss, d0,
                n_iter, lr, w_track, w_smooth, max_move, nullptr, -1, 0.f, 0.f, out, cost, moved, stream);
}

extern "C" int sw_plan_refine_walls(const float* pos, int pstride, const float* start, int sstride, const int* scene_off,
                                    const int* len, int S, int B, int K, int Tp, const float* plans, const float* plan_start,
                                    const int* q_scene, const int* q_ego, int Q, int P, float inv_ss, float d0, int n_iter,
                                    float lr, float w_track, float w_smooth, float max_move, const float* walls, int M,
                                    float dw, float w_wall, float* out, float* cost, float* moved, void* stream) {
  if (M < 0) return SW_EARG;
  return rf_run(pos, pstride, start, sstride, scene_off, len, S, B, K, Tp, plans, plan_start, q_scene, q_ego, Q, P, inv_ss, d0,
                n_iter, lr, w_track, w_smooth, max_move, walls, M, dw, w_wall, out, cost, moved, stream);
}
