// sw_plan_risk.hip - the risk of candidate ego paths against the K sampled futures of a scene: per (query, plan) the
// closest approach of the plan to every (draw, agent) path, reduced to per-agent conflict counts, their product over the
// scene's agents (the draws of different agents are independent given the observations), the index-paired count, the first
// conflicting frame and the smallest clearance.  The only floating-point work in front of the final product is the segment
// arithmetic of sw_scene.hip (sw_scene_dev.h); everything accumulated across lanes is an integer or a minimum.  Does not
// depend on the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include <stdint.h>

#define SW_RISK_MAXK 4096
#define PR_THREADS 256
#define PR_TILE 64             // plans of a workgroup at most
#define PR_LDS_MAX 65536       // two workgroups per CU
#define PR_FILL 512            // workgroups that fill the device (256 CUs, two each)
#define PR_TILE_MIN 8          // plans of a tile at least (unless P is smaller): a tile reloads the paths of its scene

struct PrArgs {
  const float* pos;
  const float* start;
  const int* scene_off;
  const int* len;
  const float* plans;
  const float* plan_start;
  const int* plan_len;
  const int* q_scene;
  const int* q_ego;
  int pstride, sstride, S, B, K, Tp, NS, first, P;
  int PT, NT;                  // plans per tile, tiles per query
  int Kb, APB, HS, KW;         // draws and agents of a lane batch (Kb * APB <= 256), stride of a plan's h row, words of its draw mask
  float inv_ss, coll;
};

// LDS of a workgroup, per plan of its tile: ST: the NS + 1 points of the plan; then the bits of the smallest squared
// approach, the first conflicting frame, KW words of draw bits and HS per-agent counts of the agent group at hand.
__host__ __device__ inline long long pr_plan_bytes(bool st, int NS, int KW, int HS) {
  return (st ? 8LL * (NS + 1) : 0LL) + 8 + 4LL * KW + 4LL * HS;
}

// ---- the risk of the plans of one tile (definitions in include/socialways_hip.h) -------------------------------------------
//   One 256-thread workgroup per (query, tile of up to 64 plans; 8 .. 64 so that the launch has some 512 workgroups).  A lane owns a (agent, draw) pair: the draws of an agent
//   sit side by side (lane = al * Kb + kk, Kb = min(K, 256), 256 / Kb agents per batch), so a chunk of 8-agent scenes at
//   K = 20 fills 160 lanes with the whole scene; larger scenes loop over agent groups, more than 256 draws over draw groups.
//   The lane's own SC_TC + 1 points sit in registers (sc_load_own, loaded once when the path is one time chunk) and it walks
//   plans x segments with the plan as the wave-uniform partner, read from LDS (every lane the same address) or, when a tile
//   does not fit, from where it lies.  r0 advances through every segment; with lengths the fold is a select.  Per segment the
//   lane tests sqrtf(m) * inv_ss < coll_dist itself, which gives the first conflicting frame; a path conflicts iff a segment
//   does.  Conflicting lanes add to the plan's per-agent count, set the draw's bit and lower the first frame with integer LDS
//   atomics, every lane lowers the plan's minimum (the bits of a non-negative float order as unsigned integers): none of
//   these depends on the order of arrival.  Behind an agent group thread p folds the group's counts of plan p, agents
//   ascending: the product, and the worst agent by a strict >.  No barrier inside the plan loop.
template <bool LEN, bool ST>
__global__ __launch_bounds__(PR_THREADS) void plan_risk_kernel(PrArgs A, float* __restrict__ risk,
                                                               float* __restrict__ clear_min, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pr_lds[];
  const int tid = threadIdx.x;
  const int q = blockIdx.x / A.NT, p0 = (blockIdx.x - q * A.NT) * A.PT;
  const int np = A.P - p0 < A.PT ? A.P - p0 : A.PT;
  const float INF = __builtin_inff();
  const int NP = A.NS + 1;

  const int sc = A.q_scene[q];
  int s0 = 0, n = 0;
  if (sc >= 0 && sc < A.S) {
    const int b0 = A.scene_off[sc], b1 = A.scene_off[sc + 1];
    if (b0 >= 0 && b1 >= b0 && b1 <= A.B) {                  // offsets outside the batch: read nothing
      s0 = b0;
      n = b1 - b0;
    }
  }
  const size_t out0 = (size_t)q * A.P + p0;
  if (n == 0) {                                              // uniform: in front of every barrier
    if (tid < np) {
      risk[out0 + tid] = 0.f;
      clear_min[out0 + tid] = INF;
      int* o = counts + (out0 + tid) * 4;
      o[0] = 0; o[1] = -1; o[2] = -1; o[3] = 0;
    }
    return;
  }
  const int ego = A.q_ego ? A.q_ego[q] : -1;

  float2* pl = reinterpret_cast<float2*>(pr_lds);
  unsigned* minm = reinterpret_cast<unsigned*>(pr_lds + (ST ? (size_t)8 * NP * A.PT : 0));
  int* tfirst = reinterpret_cast<int*>(minm + A.PT);
  unsigned* mask = reinterpret_cast<unsigned*>(tfirst + A.PT);
  int* hcnt = reinterpret_cast<int*>(mask + (size_t)A.PT * A.KW);

  const float2* gplan = reinterpret_cast<const float2*>(A.plans) + out0 * A.Tp;
  float2 pstart = float2{0.f, 0.f};
  if (A.plan_start) pstart = float2{A.plan_start[(size_t)q * 2], A.plan_start[(size_t)q * 2 + 1]};
  const auto gpoint = [=](int p, int pt) {                   // point pt of plan p of the tile, where it lies
    if (A.plan_start) {
      if (pt == 0) return pstart;
      pt -= 1;
    }
    return gplan[(size_t)p * A.Tp + pt];
  };

  for (int i = tid; i < np; i += PR_THREADS) {
    minm[i] = __float_as_uint(INF);
    tfirst[i] = 0x7fffffff;
  }
  for (int i = tid; i < np * A.KW; i += PR_THREADS) mask[i] = 0u;
  for (int i = tid; i < np * A.HS; i += PR_THREADS) hcnt[i] = 0;
  if (ST)
    for (int i = tid; i < np * NP; i += PR_THREADS) {
      const int p = i / NP;
      pl[i] = gpoint(p, i - p * NP);
    }
  __syncthreads();

  int vp = A.NS;                                             // countable segments of the plans of this query
  if (LEN && A.plan_len) vp = min(max(A.plan_len[q], 1), A.Tp) - A.first;
  const int al = tid / A.Kb, kk = tid - al * A.Kb;
  const bool single = A.NS <= SC_TC;                         // one time chunk: the lane's points are loaded once per batch
  float prod = 1.f;                                          // thread p: the running product of plan p, its worst agent
  int worst = -1, worst_h = 0;

  for (int a0 = 0; a0 < n; a0 += A.APB) {
    const int a = a0 + al, ac = a < n ? a : n - 1;
    const int arow = s0 + ac;
    int va = A.NS;
    if (LEN && A.len) va = sc_len(A.len, arow, A.Tp, A.first);
    const int lim_all = min(va, vp);
    for (int k0 = 0; k0 < A.K; k0 += A.Kb) {
      const int k = k0 + kk, kc = k < A.K ? k : A.K - 1;
      const bool valid = al < A.APB && a < n && k < A.K && arow != ego;
      const size_t row = (size_t)kc * A.B + arow;
      float2 own[SC_NP];
      if (single) sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, row, arow, A.Tp, 0, A.NS);
      for (int p = 0; p < np; ++p) {
        const float2* prow = pl + (size_t)p * NP;
        float m = INF;
        int tf = -1;                                         // the frame at which this pair's first conflicting segment ends
        for (int t0 = 0; t0 < A.NS; t0 += SC_TC) {
          const int nseg = A.NS - t0 < SC_TC ? A.NS - t0 : SC_TC;
          if (!single) sc_load_own(own, A.pos, A.pstride, A.start, A.sstride, row, arow, A.Tp, t0, nseg);
          const auto pq = [=](int pt) { return ST ? prow[t0 + pt] : gpoint(p, t0 + pt); };
          const float2 q0 = pq(0);
          float rx = own[0].x - q0.x, ry = own[0].y - q0.y;  // r0 of the chunk's first segment
          const int lim = lim_all - t0;                      // countable segments of the pair in this chunk (<= 0: none)
#pragma unroll
          for (int j = 0; j < SC_TC; ++j) {
            if (j < nseg) {
              float mj = INF;
              sc_segment(own[j + 1], pq(j + 1), rx, ry, mj);
              const bool on = !LEN || j < lim;
              m = on ? fminf(m, mj) : m;
              const bool hit = on && sqrtf(mj) * A.inv_ss < A.coll;
              tf = (hit && tf < 0) ? t0 + j + A.first : tf;
            }
          }
        }
        if (valid) {
          const unsigned mb = __float_as_uint(m);
          if (mb < minm[p]) atomicMin(&minm[p], mb);
          if (tf >= 0) {
            atomicAdd(&hcnt[p * A.HS + al], 1);
            atomicOr(&mask[p * A.KW + (k >> 5)], 1u << (k & 31));
            atomicMin(&tfirst[p], tf);
          }
        }
      }
    }
    __syncthreads();                                         // the counts of this agent group are complete
    if (tid < np) {
      const int na = n - a0 < A.APB ? n - a0 : A.APB;
      for (int b = 0; b < na; ++b) {
        const int h = hcnt[tid * A.HS + b];
        if (h) {                                             // h = 0: f = 1, the product keeps its bits
          prod *= (float)(A.K - h) / (float)A.K;
          hcnt[tid * A.HS + b] = 0;
          if (h > worst_h) {
            worst_h = h;
            worst = s0 + a0 + b;
          }
        }
      }
    }
    __syncthreads();
  }

  if (tid < np) {
    int draws = 0;
    for (int w = 0; w < A.KW; ++w) draws += __popc(mask[tid * A.KW + w]);
    risk[out0 + tid] = 1.f - prod;
    clear_min[out0 + tid] = sqrtf(__uint_as_float(minm[tid])) * A.inv_ss;
    int* o = counts + (out0 + tid) * 4;
    o[0] = draws;
    o[1] = tfirst[tid] == 0x7fffffff ? -1 : tfirst[tid];
    o[2] = worst;
    o[3] = worst_h;
  }
}

template <bool LEN, bool ST>
static int pr_launch(const PrArgs& A, int Q, int lds, float* risk, float* clear_min, int* counts, hipStream_t stream) {
  static int have = 0;                                       // one per instance
  if (int rc = sw_set_lds((const void*)plan_risk_kernel<LEN, ST>, lds, have)) return rc;
  SW_LAUNCH_AS("plan_risk_kernel", (plan_risk_kernel<LEN, ST>), dim3((unsigned)(Q * A.NT)), dim3(PR_THREADS), lds, stream, A, risk,
               clear_min, counts);
  SW_CHECK_LAUNCH("plan_risk_kernel");
  return SW_OK;
}

extern "C" int sw_plan_risk(const float* pos, int pstride, const float* start, int sstride, const int* scene_off,
                            const int* len, int S, int B, int K, int Tp, const float* plans, const float* plan_start,
                            const int* plan_len, const int* q_scene, const int* q_ego, int Q, int P, float inv_ss,
                            float coll_dist, float* risk, float* clear_min, int* counts, void* stream) {
  if (!sw_paths_ok(pos, pstride, start, sstride) || !scene_off || !q_scene || !risk || !clear_min || !counts) return SW_EARG;
  if (!plans || ((uintptr_t)plans & 7)) return SW_EARG;                              // plans are read as float2
  if ((start == nullptr) != (plan_start == nullptr)) return SW_EARG;                 // a start point on both sides or on neither
  if (S < 0 || B < 0 || Q < 0 || K < 1 || Tp < 1 || P < 1 || !(inv_ss > 0.f) || !(coll_dist >= 0.f)) return SW_EARG;
  if (K > SW_RISK_MAXK) return SW_ESHAPE;
  if (Q == 0) return SW_OK;
  PrArgs A = {};
  A.pos = pos; A.start = start; A.scene_off = scene_off; A.len = len; A.plans = plans; A.plan_start = plan_start;
  A.plan_len = plan_len; A.q_scene = q_scene; A.q_ego = q_ego;
  A.pstride = pstride; A.sstride = sstride; A.S = S; A.B = B; A.K = K; A.Tp = Tp; A.P = P;
  A.first = start ? 0 : 1;
  A.NS = Tp - A.first;
  A.Kb = K < PR_THREADS ? K : PR_THREADS;
  A.APB = PR_THREADS / A.Kb;
  A.HS = A.APB | 1;                                          // odd: the folding threads, a plan each, fall on different banks
  A.KW = (K + 31) / 32;
  A.inv_ss = inv_ss; A.coll = coll_dist;
  bool st = true;
  long long fit = PR_LDS_MAX / pr_plan_bytes(true, A.NS, A.KW, A.HS);
  if (fit < 1) {                                             // not one plan fits: the plans are read where they lie
    st = false;
    fit = PR_LDS_MAX / pr_plan_bytes(false, A.NS, A.KW, A.HS);
  }
  A.PT = (int)(fit < PR_TILE ? fit : PR_TILE);
  if (A.PT > P) A.PT = P;
  const int tiles = (PR_FILL + Q - 1) / Q;                   // few queries: smaller tiles, down to PR_TILE_MIN plans, fill the device
  const int spread = (P + tiles - 1) / tiles < PR_TILE_MIN ? PR_TILE_MIN : (P + tiles - 1) / tiles;
  if (A.PT > spread) A.PT = spread;
  A.NT = (P + A.PT - 1) / A.PT;
  if ((long long)Q * A.NT > 0x7fffffffLL) return SW_EARG;
  const int lds = (int)(A.PT * pr_plan_bytes(st, A.NS, A.KW, A.HS));
  const bool gated = len || plan_len;
  hipStream_t hs = (hipStream_t)stream;
  if (gated) return st ? pr_launch<true, true>(A, Q, lds, risk, clear_min, counts, hs) : pr_launch<true, false>(A, Q, lds, risk, clear_min, counts, hs);
  return st ? pr_launch<false, true>(A, Q, lds, risk, clear_min, counts, hs) : pr_launch<false, false>(A, Q, lds, risk, clear_min, counts, hs);
}
