// sw_compose.hip - a collision-free joint future of a scene put together from the per-agent draws: per scene one draw per
// agent, the draws the score prefers, moved to other draws until no two chosen paths come closer than coll_dist (or no
// move helps).  A selection: the only floating-point work is the clearance of two paths, with the segment arithmetic of
// sw_scene.hip (sw_scene_dev.h); everything written out is a draw index, an integer count or such a clearance.  Does not
// depend on the hidden size.
#include "../../include/socialways_hip.h"
#include "sw_common.h"
#include "sw_scene_dev.h"
#include <stdint.h>

#define SW_COMPOSE_MAXK 4096
#define CMP_HEAD 64            // bytes in front of everything else: the integers the four waves exchange
#define CMP_CAND 8192          // bytes for the candidate paths of the agent a sweep is at, a batch at a time
#define CMP_LDS_MAX 65536      // two workgroups per CU

struct CmpArgs {
  const float* pos;
  const float* start;
  const float* score;
  const int* len;
  int pstride, sstride, B, K, Tp, NS, first;
  float inv_ss, coll;
};

__device__ __forceinline__ int cmp_len(const CmpArgs& A, int row) {           // countable segments of an agent
  return A.len ? sc_len(A.len, row, A.Tp, A.first) : A.NS;
}

// sel0: the draw with the highest score, the lowest k of equal ones (ascending k, strict >)
__device__ __forceinline__ int cmp_top(const CmpArgs& A, int row) {
  float bs = A.score[row];
  int bk = 0;
  for (int k = 1; k < A.K; ++k) {
    const float v = A.score[(size_t)k * A.B + row];
    if (v > bs) {
      bs = v;
      bk = k;
    }
  }
  return bk;
}

// (conf, -score, j) lexicographically: is x in front of y
__device__ __forceinline__ bool cmp_before(int xc, float xs, int xj, int yc, float ys, int yj) {
  return xc < yc || (xc == yc && (xs > ys || (xs == ys && xj < yj)));
}

// The scene of one workgroup.  ST: its selected paths sit in LDS (sp, rows of NPs float2) and so does the selection
// (csel); else csel is the scene's part of the output and a partner's path is read where it lies.
template <bool ST>
struct CmpScene {
  const CmpArgs& A;
  int s0, n, lg, NPs;
  int* csel;               // [n] the selection as it stands (LDS or global; read behind a barrier after every change)
  float2* sp;
  float2* cand;            // rows of NPs float2: the batch of candidate paths of one agent

  __device__ __forceinline__ float2 partner(int b, size_t brow, int p) const {
    if (ST) return sp[b * NPs + p];
    return sc_point(A.pos, A.pstride, A.start, A.sstride, brow, s0 + b, A.Tp, p);
  }

  // Draw j of agent a against the selected draws of the others, by the n_pad lanes of a group (bl = lane in the group;
  // every lane of the wave is in here): cnt = conf_a(j), m = the smallest squared approach, in every lane of the group.
  // Lane bl walks the partners bl, bl + n_pad, ...; per partner the time chunks of sw_scene.hip with the lane's own points
  // in registers, r0 advancing through every segment and the minimum gated by the pair's length.  The lane's own
  // points are copies of the same floats wherever they come from: CUR - j is sel[a], whose path a staged scene holds; else
  // row `slot` of the candidate batch, or (slot < 0) global memory.  The count is a population count of the group's part
  // of the wave's ballot; the minimum (MIN: the caller wants it) an xor butterfly.
  template <bool CUR, bool MIN>
  __device__ __forceinline__ void eval(int a, int j, int slot, int bl, int& cnt, float& mn) const {
    const int n_pad = 1 << lg;
    const float INF = __builtin_inff();
    const unsigned long long gmask =
        lg == 6 ? ~0ull : ((1ull << n_pad) - 1ull) << (((threadIdx.x & 63) >> lg) << lg);      // the lanes of this group
    const size_t row = (size_t)j * A.B + s0 + a;
    const int va = cmp_len(A, s0 + a);
    int count = 0;
    float best = INF;
    for (int b0 = 0; b0 < n; b0 += n_pad) {
      const int b = b0 + bl, bc = b < n ? b : n - 1;
      const bool other = b < n && b != a;
      const int lim = min(va, cmp_len(A, s0 + bc));
      const size_t brow = ST ? 0 : (size_t)csel[bc] * A.B + s0 + bc;
      float m = INF;
      for (int t0 = 0; t0 < A.NS; t0 += SC_TC) {
        const int nseg = A.NS - t0 < SC_TC ? A.NS - t0 : SC_TC;
        float2 own[SC_NP];
#pragma unroll
        for (int p = 0; p < SC_NP; ++p)
          own[p] = p > nseg ? float2{0.f, 0.f}
                   : (ST && CUR) ? sp[a * NPs + t0 + p]
                   : (!CUR && slot >= 0) ? cand[slot * NPs + t0 + p]
                                         : sc_point(A.pos, A.pstride, A.start, A.sstride, row, s0 + a, A.Tp, t0 + p);
        const auto q = [&](int p) { return partner(bc, brow, t0 + p); };
        SC_CHUNK(true, own, q, nseg, lim - t0, m);          // lim - t0: the pair's countable segments in this chunk (<= 0: none)
      }
      count += __popcll(__ballot(other && sqrtf(m) * A.inv_ss < A.coll) & gmask);
      best = other ? fminf(best, m) : best;
    }
    if (MIN)
      for (int w = 1; w < n_pad; w <<= 1) best = fminf(best, __shfl_xor(best, w));
    cnt = count;
    mn = best;
  }

  __device__ __forceinline__ void stage(int a, int j) const {      // the path of (j, a) into row a of the staged scene
    const int NP = A.NS + 1;
    for (int p = threadIdx.x; p < NP; p += 256)
      sp[a * NPs + p] = sc_point(A.pos, A.pstride, A.start, A.sstride, (size_t)j * A.B + s0 + a, s0 + a, A.Tp, p);
  }
};

// sum of v over the workgroup, in every thread (integers: no order to fix)
__device__ __forceinline__ int cmp_block_sum(int v, int* xch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                           // the previous exchange has been read
  if ((threadIdx.x & 63) == 0) xch[threadIdx.x >> 6] = v;
  __syncthreads();
  return xch[0] + xch[1] + xch[2] + xch[3];
}

// conflicting pairs of the selection as it stands; with `clear`, also the clearance of every agent.  A group per agent.
template <bool ST>
__device__ __forceinline__ int cmp_pairs(const CmpScene<ST>& C, int* xch, float* __restrict__ clear) {
  const int n_pad = 1 << C.lg, groups = 256 >> C.lg;
  const int gid = threadIdx.x >> C.lg, bl = threadIdx.x & (n_pad - 1);
  int sum = 0;
  for (int a0 = 0; a0 < C.n; a0 += groups) {
    const int a = a0 + gid, ac = a < C.n ? a : C.n - 1;
    int cnt;
    float m;
    C.template eval<true, true>(ac, C.csel[ac], -1, bl, cnt, m);
    if (a < C.n && bl == 0) {
      sum += cnt;
      if (clear) clear[C.s0 + a] = sqrtf(m) * C.A.inv_ss;
    }
  }
  return cmp_block_sum(sum, xch) >> 1;                       // every conflicting pair was counted from both sides
}

template <bool ST>
__device__ __forceinline__ void cmp_scene(const CmpArgs& A, int s, int s0, int n, int sweeps, unsigned char* lds,
                                          const float* __restrict__ err, int* sel, int* __restrict__ sel0,
                                          float* __restrict__ clear, int* __restrict__ per_scene,
                                          float* __restrict__ per_row) {
  int* xch = reinterpret_cast<int*>(lds);                    // [0..3] sums, [4..15] the waves' candidates
  CmpScene<ST> C{A, s0, n, sc_log2_pad(n), (A.NS + 1) | 1, sel + s0, nullptr, reinterpret_cast<float2*>(lds + CMP_HEAD)};
  if (ST) {
    C.csel = reinterpret_cast<int*>(lds + CMP_HEAD + CMP_CAND);
    C.sp = reinterpret_cast<float2*>(lds + CMP_HEAD + CMP_CAND + ((4 * n + 15) & ~15));
  }
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n_pad = 1 << C.lg, groups = 256 >> C.lg, gid = tid >> C.lg, bl = tid & (n_pad - 1);
  const int NP = A.NS + 1;
  const int CB = CMP_CAND / (8 * C.NPs);                    // candidates per batch; 0: a path does not fit, read where it lies

  for (int a = tid; a < n; a += 256) {
    const int k = cmp_top(A, s0 + a);
    C.csel[a] = k;
    if (sel0) sel0[s0 + a] = k;
  }
  __syncthreads();
  if (ST) {
    for (int i = tid; i < n * NP; i += 256) {
      const int b = i / NP, p = i - b * NP;
      C.sp[b * C.NPs + p] = sc_point(A.pos, A.pstride, A.start, A.sstride, (size_t)C.csel[b] * A.B + s0 + b, s0 + b, A.Tp, p);
    }
    __syncthreads();
  }
  const int pairs0 = cmp_pairs(C, xch, nullptr);

  int swept = 0;
  for (int sw = 0; sw < sweeps && pairs0 > 0; ++sw) {        // everything that steers this loop is the same in every thread
    bool changed = false;
    for (int a = 0; a < n; ++a) {
      const int cur_j = C.csel[a];
      int cur;
      float m;
      C.template eval<true, false>(a, cur_j, -1, bl, cur, m);      // every group the same work: no exchange needed
      if (cur == 0) continue;
      int bc = 0x7fffffff, bj = 0x7fffffff;                  // the candidates of this group, then of the wave
      float bs = 0.f;
      for (int jb = 0; jb < A.K; jb += CB > 0 ? CB : A.K) {  // a batch of candidate paths into LDS with one round of loads
        const int nb = CB > 0 && A.K - jb > CB ? CB : A.K - jb;
        if (CB > 0) {
          __syncthreads();                                   // the previous batch has been read
          for (int i = tid; i < nb * NP; i += 256) {
            const int jj = i / NP, p = i - jj * NP;
            C.cand[jj * C.NPs + p] = sc_point(A.pos, A.pstride, A.start, A.sstride, (size_t)(jb + jj) * A.B + s0 + a, s0 + a, A.Tp, p);
          }
          __syncthreads();
        }
        for (int j0 = 0; j0 < nb; j0 += groups) {
          const int jj = j0 + gid, jc = jj < nb ? jj : nb - 1, j = jb + jj;
          int cnt;
          C.template eval<false, false>(a, jb + jc, CB > 0 ? jc : -1, bl, cnt, m);
          const float sc = A.score[(size_t)(jb + jc) * A.B + s0 + a];
          if (jj < nb && cmp_before(cnt, sc, j, bc, bs, bj)) {
            bc = cnt;
            bs = sc;
            bj = j;
          }
        }
      }
      for (int w = n_pad; w < 64; w <<= 1) {
        const int oc = __shfl_xor(bc, w), oj = __shfl_xor(bj, w);
        const float os = __shfl_xor(bs, w);
        if (cmp_before(oc, os, oj, bc, bs, bj)) {
          bc = oc;
          bs = os;
          bj = oj;
        }
      }
      __syncthreads();                                       // the previous exchange has been read
      if (lane == 0) {
        xch[4 + 3 * wave] = bc;
        xch[5 + 3 * wave] = __float_as_int(bs);
        xch[6 + 3 * wave] = bj;
      }
      __syncthreads();
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int oc = xch[4 + 3 * w], oj = xch[6 + 3 * w];
        const float os = __int_as_float(xch[5 + 3 * w]);
        if (cmp_before(oc, os, oj, bc, bs, bj)) {
          bc = oc;
          bs = os;
          bj = oj;
        }
      }
      if (bc < cur) {                                        // a strict gain only: the pair count falls with every change
        if (tid == 0) C.csel[a] = bj;
        if (ST) C.stage(a, bj);
        changed = true;
        __syncthreads();
      }
    }
    if (!changed) break;
    ++swept;
  }

  const int pairs1 = cmp_pairs(C, xch, clear);
  int moved = 0;
  for (int a = tid; a < n; a += 256) {
    const int row = s0 + a, k0 = cmp_top(A, row), k1 = C.csel[a];
    if (ST) sel[row] = k1;
    moved += k1 != k0 ? 1 : 0;
    if (per_row) {
      const float2 e0 = reinterpret_cast<const float2*>(err)[(size_t)k0 * A.B + row];
      const float2 e1 = reinterpret_cast<const float2*>(err)[(size_t)k1 * A.B + row];
      float* p = per_row + (size_t)row * 4;
      p[0] = e0.x; p[1] = e0.y; p[2] = e1.x; p[3] = e1.y;
    }
  }
  moved = cmp_block_sum(moved, xch);
  if (tid == 0) {
    int* o = per_scene + (size_t)s * 4;
    o[0] = pairs0; o[1] = pairs1; o[2] = moved; o[3] = swept;
  }
}

// ---- the composition (definition in include/socialways_hip.h) ----------------------------------------------------------------
//   One 256-thread workgroup per scene: the agents are visited one after the other, and a change must be seen by the next.
//   The selected path of every agent is staged in LDS (rows of Tp + 1 points, padded to an odd count so that the lanes of
//   a group, one partner each, fall on different banks) and rewritten when its agent moves; a scene whose rows do not fit
//   reads them from global memory through the selection, which then lives in the output array.  The unit of work is (agent
//   a, draw j): a group of n_pad lanes (sc_log2_pad: a power of two up to 64) walks the partners, one or more per lane;
//   its integer conflict count is a population count of the wave's ballot, its minimum an xor butterfly.  For the agent a
//   sweep visits, every group first evaluates the selected draw, whose own points the staged scene holds too - the same
//   work in all groups, so nobody waits for the result.  Only an agent in conflict looks at its K candidates: the
//   workgroup copies their paths into LDS, 8 KB at a time (one round of global loads per batch; a path longer than that is
//   read where it lies), and spreads them over the 256 / n_pad groups; their best (conf, -score, j) is folded inside the
//   wave by an xor butterfly and across the four waves through 12 integers in LDS.  The pair counts and the clearances are
//   one more pass with a group per agent.  One writer per output element, integer sums, no atomics.
__global__ __launch_bounds__(256) void scene_compose_kernel(CmpArgs A, const int* __restrict__ scene_off, int sweeps,
                                                            int lds_bytes, const float* __restrict__ err, int* sel,
                                                            int* __restrict__ sel0, float* __restrict__ clear,
                                                            int* __restrict__ per_scene, float* __restrict__ per_row) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cmp_lds[];
  const int s = blockIdx.x;
  const int s0 = scene_off[s], s1 = scene_off[s + 1];
  const int n = (s0 >= 0 && s1 >= s0 && s1 <= A.B) ? s1 - s0 : 0;      // offsets outside the batch: read nothing
  if (n == 0) {                                              // uniform: in front of every barrier
    if (threadIdx.x < 4) per_scene[(size_t)s * 4 + threadIdx.x] = 0;
    return;
  }
  const long long need = CMP_HEAD + CMP_CAND + (((long long)4 * n + 15) & ~15LL) + (long long)8 * n * ((A.NS + 1) | 1);
  if (need <= lds_bytes)
    cmp_scene<true>(A, s, s0, n, sweeps, cmp_lds, err, sel, sel0, clear, per_scene, per_row);
  else
    cmp_scene<false>(A, s, s0, n, sweeps, cmp_lds, err, sel, sel0, clear, per_scene, per_row);
}

extern "C" int sw_scene_compose(const float* pos, int pstride, const float* start, int sstride, const float* score,
                                const int* scene_off, const int* len, int S, int B, int K, int Tp, float inv_ss,
                                float coll_dist, int sweeps, const float* err, int* sel, int* sel0, float* clear,
                                int* per_scene, float* per_row, void* stream) {
  if (!sw_paths_ok(pos, pstride, start, sstride) || !score || !scene_off || !sel || !clear || !per_scene) return SW_EARG;
  if (S < 0 || B < 0 || K < 1 || Tp < 1 || sweeps < 1 || !(inv_ss > 0.f) || !(coll_dist >= 0.f)) return SW_EARG;
  if ((per_row && !err) || ((uintptr_t)err & 7)) return SW_EARG;                     // errors are read as float2
  if (K > SW_COMPOSE_MAXK) return SW_ESHAPE;
  if (B == 0 || S == 0) return SW_OK;
  const int first = start ? 0 : 1;
  const CmpArgs A = {pos, start, score, len, pstride, sstride, B, K, Tp, Tp - first, first, inv_ss, coll_dist};
  const long long all = CMP_HEAD + CMP_CAND + (((long long)4 * B + 15) & ~15LL) + (long long)8 * B * ((A.NS + 1) | 1);
  const int lds = all < CMP_LDS_MAX ? (int)all : CMP_LDS_MAX;                       // a scene has at most B agents
  static int have = 0;
  if (int rc = sw_set_lds((const void*)scene_compose_kernel, lds, have)) return rc;
  SW_LAUNCH(scene_compose_kernel, dim3((unsigned)S), dim3(256), lds, (hipStream_t)stream, A, scene_off, sweeps, lds, err, sel,
            sel0, clear, per_scene, per_row);
  SW_CHECK_LAUNCH("scene_compose_kernel");
  return SW_OK;
}
