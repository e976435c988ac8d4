// sw_wgrad_dev.h - device code of the grouped split-K weight-gradient GEMM (see sw_wgrad.hip): the per-job body of
// wgrad_partial_kernel.
#pragma once
#include <type_traits>
#include "sw_common.h"
#include "sw_wgrad.h"
#ifndef SW_WG_DEPTH
#define SW_WG_DEPTH 4
#endif
#ifndef SW_WG_DEPTH5
#define SW_WG_DEPTH5 2
#endif
#ifndef SW_WG_DEPTH_TAIL
#define SW_WG_DEPTH_TAIL SW_WG_DEPTH
#endif
#ifndef SW_WG_PEEL      // 1: a slice's last partial trip runs only its live groups (wg_run); 0: whole trips, the rest zeros
#define SW_WG_PEEL 1
#endif

// Timing experiment (-DSW_WG_STAMP, tools/build_variant.sh): wall-clock marks inside a job, kept in registers by the first
// lane of the workgroup and written out by wgrad_partial_kernel.  mk[0] job found (record fetched), [1] descriptors built,
// [2] first group arrived, [3] loop left, [4] LDS sum done, [5] stores issued.  Nothing of it exists in a default build.
#ifdef SW_WG_STAMP
#define WG_MARKS_ARG , unsigned long long (&mk)[6]
#define WG_MARKS_PASS , mk
#define WG_MARK(i) mk[i] = wall_clock64()
#else
#define WG_MARKS_ARG
#define WG_MARKS_PASS
#define WG_MARK(i) ((void)0)
#endif

#define SW_WG_RLD 72   // LDS row stride of a wave's 64 x (<= 69) block: 64 act columns + tail segment + ones, rounded up
                       // to 16 bytes (a lane's consecutive columns go out, and the four slices come back, as b128 / b64)
static_assert(SW_WG_RLD % 4 == 0 && SW_WG_RLD >= 69, "16-byte LDS rows that hold 64 + 4 + 1 columns");
static_assert(2 * 4 * 64 * SW_WG_RLD * 4 <= 160 * 1024, "two workgroups per CU must fit the 160 KB of LDS");

// Bounded operand loads: a wave reads its row slice through one buffer descriptor per operand.  The descriptor's range
// ends on the slice's last row boundary, so a row beyond it - prefetch overrun, the padding of the last 4-row group - comes
// back as zeros from the hardware's range check, and a row in front of the base (byte offset wrapped past 2^32) does too:
// no row clamp, no 64-bit address, no 0/1 mask factor.
typedef __amdgpu_buffer_rsrc_t wg_rsrc;
// `base` and `bytes` must be wave-uniform TO THE COMPILER (formed from kernel arguments and readfirstlane values): a
// descriptor it cannot prove uniform gets every load wrapped in a serialising loop over the lanes' values
__device__ __forceinline__ wg_rsrc wg_make_rsrc(const float* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
// NV consecutive floats at byte offset `off` as ONE vector load (dword / dwordx2 / dwordx3 / dwordx4)
// (each component goes through a scalar of its own: __builtin_bit_cast applied to a vector ELEMENT reads component 0)
template <int NV>
__device__ __forceinline__ void wg_ldv(float (&v)[NV], wg_rsrc rs, unsigned off) {
  unsigned u[NV];
  if constexpr (NV == 4) {
    const auto q = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    u[0] = q[0]; u[1] = q[1]; u[2] = q[2]; u[3] = q[3];
  } else if constexpr (NV == 3) {
    const auto q = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)off, 0, 0);
    u[0] = q[0]; u[1] = q[1]; u[2] = q[2];
  } else if constexpr (NV == 2) {
    const auto q = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0);
    u[0] = q[0]; u[1] = q[1];
  } else {
    u[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = __uint_as_float(u[i]);
}

// Tiles per lane vector: the smallest t with 16 t >= n and n % t == 0 (every lane's vector is then wholly live or wholly
// dead: no partial lane), t in {1, 2, 4} for delta columns, {1, 2, 3, 4} for act columns; 0 = no such t (the host
// rejects the problem: SW_ESHAPE - cannot happen for the layer widths of this model, all multiples of 4 or <= 16)
__host__ __device__ inline int wg_tiles(int n, bool allow3) {
  if (n <= 16) return 1;
  for (int t = (n + 15) >> 4; t <= 4; ++t)
    if ((t != 3 || allow3) && n % t == 0) return t;
  return 0;
}

// One wave = one job: a 64 x (<= 69) output block of one column block of one problem over one row slice, accumulated
// in NA x (KR + XT) MFMA tiles.  MFMA K dimension = rows (4 per instruction: lane group lg = row r0 + lg).
//
// Operand loads are VECTOR loads: lane ln fetches the NA consecutive delta columns n0 + NA ln .. and the KR consecutive
// act columns KR ln .. of its row - a 16-lane group reads one contiguous 64 NA / 64 KR-byte piece of the row - and
// feeds component i to MFMA tile i.  Tile i therefore covers the columns {NA m + i}: a permutation of the output rows /
// columns among the tiles, undone where the block is written out (`mine`).  (Round 1 loaded one dword per tile and
// lane: 9 load instructions of 64-byte pieces per 20 MFMAs; the waves waited 58 % of their cycles.)  The summation
// order of every output element - its rows, 4 per MFMA, in slice order - is unchanged: bit-identical results.
//   NA = min(4, tiles of 16 delta columns in this block), KR = tiles of real act columns (1..4),
//   XT = 1: one more k-tile holding the tail segment (act2, K2 columns) and / or the ones column at lanes ln = 0..
// Branch-free streaming body: loads are unconditional and bounded by the operand's descriptor (rows outside the slice read
// zero); the pipeline registers hold RAW loaded values (arithmetic attached to a load would sit in front of the loop's back
// edge and drain the pipeline once per DEPTH groups).
// rbeg / rend must be wave-uniform to the compiler (wg_job passes them through readfirstlane).  Rows below row0 have no
// `act` operand: its descriptor starts at row max(rbeg, row0) - `abase` itself may lie IN FRONT of the allocation (the LSTM
// problem passes h_{t-1} as "the act row one time step earlier") and is never dereferenced below that row.
template <int NA, int KR, int K2, int ONES, int DSCALE = 1>
__device__ __forceinline__ void wg_run(const float* __restrict__ dbase, const float* __restrict__ abase, int ldd, int lda,
                                       int rbeg, int rend, int acol, int bcol, int lg, int ln,
                                       float* __restrict__ mine,
                                       const float* __restrict__ abase2, int lda2, int row0, int xoff WG_MARKS_ARG) {
  constexpr int KT = KR, XC = K2 + ONES;
  // 4-row groups in flight (swept on the GPU at 8 waves per CU)
  constexpr int DEPTH = (K2 > 0 ? SW_WG_DEPTH_TAIL : SW_WG_DEPTH) * DSCALE;
  float a[DEPTH][NA], b[DEPTH][KT];
  f32x4 xq[DEPTH];
  // One descriptor per operand: the slice's rows [rbeg, rend) - for `act` [max(rbeg, row0), rend) -, ending on a row
  // boundary (a lane's vector lies inside its row: no load straddles the end).  Byte offsets are 32-bit (the host rejects
  // a problem whose slices could span 2^31 bytes); a lane's offset advances by one add per group.
  const int abeg = K2 > 0 ? max(rbeg, row0) : rbeg, aend = max(abeg, rend);
  const wg_rsrc drs = wg_make_rsrc(dbase + (size_t)rbeg * ldd, (unsigned)(rend - rbeg) * (unsigned)ldd * 4u);
  const wg_rsrc ars = wg_make_rsrc(abase + (size_t)abeg * lda, (unsigned)(aend - abeg) * (unsigned)lda * 4u);
  const wg_rsrc xrs = wg_make_rsrc(abase2 + (size_t)rbeg * lda2, (unsigned)(rend - rbeg) * (unsigned)lda2 * 4u);
  // rows below row0 start at a NEGATIVE row of the act descriptor: the unsigned offset wraps out of range -> zeros
  unsigned doff = (unsigned)(lg * ldd + acol) * 4u, aoff = (unsigned)((rbeg - abeg + lg) * lda + bcol) * 4u;
  unsigned xoff2 = (unsigned)(lg * lda2) * 4u;
  const unsigned dstep = 16u * (unsigned)ldd, astep = 16u * (unsigned)lda, xstep = 16u * (unsigned)lda2;
  WG_MARK(1);
  auto load = [&](float (&av)[NA], float (&bv)[KT], f32x4& xv) {     // the next 4-row group of the slice
    wg_ldv<NA>(av, drs, doff);
    doff += dstep;
    wg_ldv<KR>(bv, ars, aoff);
    aoff += astep;
    if constexpr (K2 > 0) {
      float x4[4];
      wg_ldv<4>(x4, xrs, xoff2);                                      // the row's tail columns (same address for 16 lanes)
      xv = f32x4{x4[0], x4[1], x4[2], x4[3]};
      xoff2 += xstep;
    }
  };
#pragma unroll
  for (int q = 0; q < DEPTH - 1; ++q) load(a[q], b[q], xq[q]);
  asm volatile("" ::: "memory");   // the first DEPTH - 1 groups are on their way before anything that does not feed an address
  // The tail segment (K2 = 4 columns of act2: the LSTM's x_t) and the ones column (bias gradient) do NOT get an MFMA
  // tile of their own - it would carry 5 (or 1) useful columns of 16, a fifth of the LSTM problem's matrix work -:
  // the lane that holds delta[row][n] multiplies it with the row's 4 x values / adds it up on the VALU, which runs
  // beside the matrix pipe; the per-row-group partial sums meet in two lane shuffles at the end of the slice.
  f32x4 acc[NA][KT];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[i][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float xacc[NA][XC > 0 ? XC : 1];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int c = 0; c < (XC > 0 ? XC : 1); ++c) xacc[i][c] = 0.f;
  }
  // No masks at all.  Rows outside [rbeg, rend) load zeros (a zero delta row kills its products, its tail columns and its
  // ones column), rows below row0 a zero act row.  There are no COLUMN masks either: a lane beyond the block's live delta /
  // act columns (clamped to the last live ones) only feeds output rows / columns that are never written out - an MFMA
  // output element mixes nothing but its own row and column.  (Peeling the interior into a branch of its own was
  // measured 1.8 x slower: memory operations under a branch cost the exact vmcnt bookkeeping, see DESIGN.md.  The peeled
  // END of a slice below holds no memory operation: the generator's LSTM jobs at the metric shape - 45 groups, 3 of 48
  // were zeros - 28.1 -> 26.8 us, profiles/wgrad_fixed_ab.txt.)
  auto consume = [&](int q) {           // q is a constant after unrolling
#pragma unroll
    for (int i = 0; i < NA; ++i) asm volatile("" : "+v"(a[q][i]));   // group q is first touched here
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) asm volatile("" : "+v"(b[q][kt]));
    if constexpr (K2 > 0) asm volatile("" : "+v"(xq[q]));
#pragma unroll
    for (int i = 0; i < NA; ++i) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        acc[i][kt] = SW_MFMA(a[q][i], b[q][kt], acc[i][kt]);
      }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      if constexpr (K2 > 0) {
#pragma unroll
        for (int c = 0; c < K2; ++c) xacc[i][c] = fmaf(a[q][i], xq[q][c], xacc[i][c]);
      }
      if constexpr (ONES) xacc[i][K2] += a[q][i];
    }
  };
#if SW_WG_PEEL
  // Whole trips of DEPTH groups, then the slice's last 1 .. DEPTH - 1 groups WITHOUT loads: they are already in flight, and
  // what the full trip would fetch and multiply beyond them is zeros.  The group count is wave-uniform; the branches hold
  // no memory operation, so every path sees the same loads in the same order (the vector-memory counter rule).
  const int groups = (rend - rbeg + 3) >> 2, whole = groups / DEPTH, rest = groups - whole * DEPTH;
  for (int t = 0; t < whole; ++t) {
#else
  for (int r = rbeg; r < rend; r += 4 * DEPTH) {
#endif
#pragma unroll
    for (int q = 0; q < DEPTH; ++q) {
      load(a[(q + DEPTH - 1) % DEPTH], b[(q + DEPTH - 1) % DEPTH], xq[(q + DEPTH - 1) % DEPTH]);
      asm volatile("" ::: "memory");   // the loads are issued HERE (DEPTH - 1 groups ahead), not sunk to their uses
      consume(q);
#ifdef SW_WG_STAMP
#if SW_WG_PEEL
      if (q == 0 && t == 0) WG_MARK(2);
#else
      if (q == 0 && r == rbeg) WG_MARK(2);
#endif
#endif
    }
  }
#if SW_WG_PEEL
#pragma unroll
  for (int q = 0; q < DEPTH - 1; ++q) {
    if (q < rest) consume(q);
  }
#endif
  WG_MARK(3);
  // tile (i, kt) element (m = 4 lg + r, n = ln)  =  output row NA m + i, act column KR n + kt
  // A lane's KR columns are consecutive and wholly live or wholly dead (K % KR == 0): one b128 / b64 write per output row
  // where KR is 4 / 2 (the row stride and KR ln keep it aligned)
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* o = mine + (NA * (4 * lg + r) + i) * SW_WG_RLD + KR * ln;
      if (KR * ln < xoff) {                                                                  // xoff = K: live columns only
        if constexpr (KR == 4) {
          *reinterpret_cast<float4*>(o) = float4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
        } else if constexpr (KR == 2) {
          *reinterpret_cast<float2*>(o) = float2{acc[i][0][r], acc[i][1][r]};
        } else {
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) o[kt] = acc[i][kt][r];
        }
      }
    }
  }
  // extra columns xoff + c of output row NA ln + i: sum of the four row groups (lanes ln, ln + 16, ln + 32, ln + 48)
  if constexpr (XC > 0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      float xv[XC];
#pragma unroll
      for (int c = 0; c < XC; ++c) {
        float v = xacc[i][c];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        xv[c] = v;
      }
      float* o = mine + (NA * ln + i) * SW_WG_RLD + xoff;
      if (lg == 0) {
        if constexpr (K2 == 4) {                        // the tail sits behind K = 64 columns: aligned
          *reinterpret_cast<float4*>(o) = float4{xv[0], xv[1], xv[2], xv[3]};
          if constexpr (ONES) o[4] = xv[4];
        } else {
#pragma unroll
          for (int c = 0; c < XC; ++c) o[c] = xv[c];
        }
      }
    }
  }
}

// One workgroup-job = 4 waves = 4 consecutive row slices of one output block (summed through LDS at the end); every
// wave streams independently (no LDS, no barriers in the loop).  `red` = 4 x 64 x SW_WG_RLD floats of LDS.
#define SW_WG_RED_FLOATS (4 * 64 * SW_WG_RLD)
template <int DSCALE = 1>
__device__ __forceinline__ void wg_job(const WgBatch& batch, const int (&keys)[SW_WG_MAXP], float* __restrict__ ws, int job,
                                       float* red WG_MARKS_ARG) {
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  // Job start = two dependent scalar round trips: the search keys (fetched by the caller, wg_keys), then the GEMM part of
  // the problem's record in one clause - it carries everything a job used to derive with divisions and loops
  // (WgProblem: cases, rows_per, nbmul).
  const int p = wg_find(keys, job);
  const WgProblem& Q = batch.p[p];
  struct {
    const float *delta, *act, *act2;
    size_t ws_off;
    int ldd, lda, lda2, row0, R, N, K, job0, cases, rows_per, nbmul, ldp;
  } P = {Q.delta, Q.act,  Q.act2, Q.ws_off, Q.ldd, Q.lda,   Q.lda2,     Q.row0,
         Q.R,     Q.N,    Q.K,    Q.job0,   Q.cases, Q.rows_per, Q.nbmul, Q.ldp};
  WG_PIN(P.delta); WG_PIN(P.act); WG_PIN(P.act2); WG_PIN(P.ws_off);
  WG_PIN(P.ldd); WG_PIN(P.lda); WG_PIN(P.lda2); WG_PIN(P.row0); WG_PIN(P.R); WG_PIN(P.N); WG_PIN(P.K); WG_PIN(P.job0);
  WG_PIN(P.cases); WG_PIN(P.rows_per); WG_PIN(P.nbmul); WG_PIN(P.ldp);
  WG_MARK(0);
  const int j = job - P.job0;
  const int NB = P.cases >> 16;         // 64-row output blocks
  const int sg = (int)(((unsigned)j * (unsigned)P.nbmul) >> 16), nb = j - sg * NB;
  const int s = sg * 4 + wave;          // this wave's row slice (may be empty)
  const int N = P.N, K = P.K;
  const int n0 = nb * 64;
  const int Nb = min(64, N - n0);                       // live delta columns of this block
  const int cs = (nb == NB - 1 ? P.cases >> 8 : P.cases) & 255;   // ((NA * 8 + KR) * 2 + tail) * 2 + ones
  const int NA = cs >> 5;                               // delta tiles
  const int KR = (cs >> 2) & 7;                         // real act tiles
  const int rows_per = P.rows_per;
  // the slice bounds feed the buffer descriptors: wave-uniform, and through readfirstlane the compiler knows it
  const int rbeg = __builtin_amdgcn_readfirstlane(min(P.R, s * rows_per));
  const int rend = __builtin_amdgcn_readfirstlane(min(P.R, rbeg + rows_per));
  // the lane's NA delta columns n0 + NA ln + i and KR act columns KR ln + kt; bases clamped into the row, dead
  // components masked
  const int acol = n0 + max(0, min(NA * ln, Nb - NA));
  const int bcol = max(0, min(KR * ln, K - KR));
  float* mine = red + wave * 64 * SW_WG_RLD;
  // extra columns on the VALU: a tail segment of exactly 4 columns (K2; only next to K = 64) and / or the ones column
#define WG_CASE(na, kr, k2, on)                                                                                     \
  case ((na * 8 + kr) * 2 + (k2 ? 1 : 0)) * 2 + on:                                                                 \
    wg_run<na, kr, k2, on, DSCALE>(P.delta, P.act, P.ldd, P.lda, rbeg, rend, acol, bcol, lg, ln,                      \
                                   mine, P.act2 ? P.act2 : P.delta, P.act2 ? P.lda2 : P.ldd, P.row0, K WG_MARKS_PASS); \
    break;
#define WG_CASES(na)                                                                                                \
  WG_CASE(na, 1, 0, 0) WG_CASE(na, 2, 0, 0) WG_CASE(na, 3, 0, 0) WG_CASE(na, 4, 0, 0)                               \
  WG_CASE(na, 1, 0, 1) WG_CASE(na, 2, 0, 1) WG_CASE(na, 3, 0, 1) WG_CASE(na, 4, 0, 1)                               \
  WG_CASE(na, 4, 4, 0) WG_CASE(na, 4, 4, 1)
  switch (cs) {
    WG_CASES(1) WG_CASES(2) WG_CASES(4)
  }
#undef WG_CASES
#undef WG_CASE
  sw_barrier();
  // one partial per workgroup (4 row slices summed): ws[ws_off + (sg*N + n)*ldp + k], ldp = Kc rounded up to 4 floats.
  // A thread sums one 16-byte chunk of a row at a time: 4 b128 LDS reads, one 16-byte store.  (The <= 3 columns between
  // Kc and ldp carry whatever the LDS held: the reduction never reads them.)
  const int ldp = P.ldp, c4 = ldp >> 2;
  float* out = ws + P.ws_off + ((size_t)sg * N + n0) * ldp;
  // chunk c = rr * c4 + cq: rr = c / c4 through a float reciprocal, exact here: c < 64 * 18 + 256, c4 <= 18, so
  // (c + 0.5) / c4 stays >= 1 / 36 away from an integer, far beyond the 2^-22 relative error of rcp and the product
  const float rc4 = __builtin_amdgcn_rcpf((float)c4);
  const float4* r0 = reinterpret_cast<const float4*>(red);
  constexpr int S4 = 64 * SW_WG_RLD / 4;
  for (int c = threadIdx.x; c < Nb * c4; c += SW_THREADS) {
    const int rr = (int)(((float)c + 0.5f) * rc4), cq = c - rr * c4;
    const int o = rr * (SW_WG_RLD / 4) + cq;
    const float4 v0 = r0[o], v1 = r0[o + S4], v2 = r0[o + 2 * S4], v3 = r0[o + 3 * S4];
    float4 v;
    v.x = (v0.x + v1.x) + (v2.x + v3.x);
    v.y = (v0.y + v1.y) + (v2.y + v3.y);
    v.z = (v0.z + v1.z) + (v2.z + v3.z);
    v.w = (v0.w + v1.w) + (v2.w + v3.w);
    reinterpret_cast<float4*>(out)[rr * c4 + cq] = v;
#ifdef SW_WG_STAMP
    if (c == (int)threadIdx.x) WG_MARK(4);      // the first chunk's sum: its four LDS reads have come back
#endif
  }
  WG_MARK(5);
}
