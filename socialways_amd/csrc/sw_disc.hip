// sw_disc.hip - Discriminator.forward (reference train.py:294-309) and its backward:
//   LSTM(4->64) over the observed 4-d track, FC 64->32->32 on its last output, FC 4Tp->32->32 on
//   the flattened (predicted or real) future, classifier 64->32->1 (raw LSGAN score) and the
//   InfoGAN latent-code head 64->32->2.
// One workgroup per 16-agent tile.  The observation encoding does not depend on the future
// branch, so the fake and the real branch of a D update (train.py:482,487) share ONE LSTM pass:
// `nb` branches are evaluated per call.
#include "../../include/socialways_hip.h"
#include "sw_lstm_dev.h"
#include "sw_wgrad.h"
#include "sw_wgrad_dev.h"
#include <cstdlib>
#ifdef SW_PHASE_STAMPS
__device__ long long sw_disc_stamps[16];
#define SW_STAMP(k) do { __builtin_amdgcn_sched_barrier(0); long long _t = clock64(); if (blockIdx.x == 0 && threadIdx.x == 0) sw_disc_stamps[k] += _t - _tprev; _tprev = _t; __builtin_amdgcn_sched_barrier(0); } while (0)
#define SW_STAMP_INIT long long _tprev = clock64()
extern "C" int sw_debug_disc_stamps(long long* out, int reset) {
  if (reset) { long long z[16] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(sw_disc_stamps), z, sizeof(z)); }
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sw_disc_stamps), 16 * sizeof(long long));
}
#else
#define SW_STAMP(k)
#define SW_STAMP_INIT
#endif

#define SW_DSTAMP(k) SW_STAMP(k)
#define SW_DSTAMP_INIT SW_STAMP_INIT
#include "sw_disc_dev.h"

__global__ __launch_bounds__(SW_THREADS, 2) void disc_fwd_kernel(
    const float* __restrict__ obsv, int To, int x_mode, const float* __restrict__ pred_a,
    const float* __restrict__ pred_b, int nb, const float* __restrict__ d_w, int B, int Tp, float* __restrict__ label_a, float* __restrict__ label_b,
    float* __restrict__ code_a, float* __restrict__ code_b, float* __restrict__ dsave, int save_lstm, int split,
    float* __restrict__ w_snap, int fuse, DiscLoss gl, float* __restrict__ dpred_out, const float* __restrict__ dimg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  disc_fwd_tile(smem, blockIdx.x, gridDim.x, obsv, To, x_mode, pred_a, pred_b, nb, d_w, B, Tp, label_a, label_b, code_a, code_b, dsave,
                save_lstm, split, w_snap, fuse, gl, dpred_out, dimg);
}

// The forward pass over RAGGED observation histories (sw_disc_fwd_ragged, sw_disc_dpred_ragged): disc_fwd_tile with the
// ragged observation loop.  A kernel of its own with obs_len as the last argument; disc_fwd_kernel keeps its code.
__global__ __launch_bounds__(SW_THREADS, 2) void disc_fwd_ragged_kernel(
    const float* __restrict__ obsv, int To, int x_mode, const float* __restrict__ pred_a,
    const float* __restrict__ pred_b, int nb, const float* __restrict__ d_w, int B, int Tp, float* __restrict__ label_a, float* __restrict__ label_b,
    float* __restrict__ code_a, float* __restrict__ code_b, float* __restrict__ dsave, int save_lstm, int split,
    float* __restrict__ w_snap, int fuse, DiscLoss gl, float* __restrict__ dpred_out, const float* __restrict__ dimg,
    const int* __restrict__ obs_len) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  disc_fwd_tile<true>(smem, blockIdx.x, gridDim.x, obsv, To, x_mode, pred_a, pred_b, nb, d_w, B, Tp, label_a, label_b, code_a, code_b,
                      dsave, save_lstm, split, w_snap, fuse, gl, dpred_out, dimg, obs_len);
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
#define SW_SPLIT_MAX_WGS 256   // CUs of an MI355X: splitting only pays while the launch leaves some of them idle

__global__ __launch_bounds__(SW_THREADS, 2) void disc_bwd_kernel(
    const float* __restrict__ d_w, const float* __restrict__ dsave, const float* __restrict__ dlabel_a,
    const float* __restrict__ dlabel_b, const float* __restrict__ dcode_a, const float* __restrict__ dcode_b, int nb,
    int B, int To, int Tp, int want_w, float* __restrict__ ddelta, float* __restrict__ dpred_a,
    float* __restrict__ dpred_b, DiscLoss gl, const float* __restrict__ dimg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const HeadLdsB L = head_lds_b(Tp, 0);
  float* dgbuf = smem + L.pe0T;  // [2][16][260], aliasing the prediction heads' images / deltas (dead when the BPTT starts)
  const swp::Disc O = swp::disc(Tp);
  const DSave ds = dsave_layout(B, To, Tp, nb);
  const DDelta dd = ddelta_layout(B, To, Tp, nb);
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int u0 = wave * 16;
  const int a0 = blockIdx.x * SW_TILE;
  const int b = min(a0 + ln, B - 1);
  const bool live = (a0 + ln) < B;
  const int K4 = 4 * Tp;

  SW_STAMP_INIT;
  // saved activations the head backward needs (post-lrelu c1 | l1, q1 per branch, o1): requested now, they arrive
  // under the weight staging instead of one L2 round trip in front of every head layer.  Unconditional loads (every
  // wave fetches a valid row, waves 2, 3 do not use q1 / o1): see the BPTT loop below.
  const int m0h = 16 * (wave & 1);
  f32x4 pc1[2], pq1[2], po1;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const size_t kb = (size_t)min(k, nb - 1) * B + b;
    pc1[k] = ld4(dsave + (wave < 2 ? ds.c1 : ds.l1) + kb * 32 + m0h + 4 * lg);
    pq1[k] = ld4(dsave + ds.q1 + kb * 32 + m0h + 4 * lg);
  }
  po1 = ld4(dsave + ds.o1 + (size_t)b * 32 + m0h + 4 * lg);
  // ... and the inputs of the loss gradients (forward outputs label / code_hat, z, the label targets): requested here,
  // not where the head backward starts (a global round trip of its own behind the staging barrier).  Element e of the
  // [16][LD16] delta tiles this thread fills, plus the per-agent values of the reported sums; unconditional loads.
  float hl[2][2], hc[2][2], hz[2], htg[2], rl[2], rc[2], rz[2];
  {
    const float* zsrc = gl.on ? gl.z : dsave;            // no GAN mode: any readable address, the value is unused
    const float* tsrc = gl.on ? gl.targets : dsave;
    htg[0] = tsrc[gl.on ? gl.t0 : 0];
    htg[1] = tsrc[gl.on ? gl.t1 : 0];
    const float* dl1 = nb > 1 ? dlabel_b : dlabel_a;
    const float* dc1p = nb > 1 ? dcode_b : dcode_a;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = min((int)threadIdx.x + SW_THREADS * e, 16 * LD16 - 1);
      const int a = i / LD16, c1 = min(i - a * LD16, 1);
      const int bb = min(a0 + a, B - 1);
      hl[e][0] = dlabel_a[bb];
      hl[e][1] = dl1[bb];
      hc[e][0] = dcode_a[(size_t)bb * 2 + c1];
      hc[e][1] = dc1p[(size_t)bb * 2 + c1];
      hz[e] = zsrc[(size_t)bb * SW_Z + c1];
    }
    const int bb = min(a0 + ln, B - 1);
    rl[0] = dlabel_a[bb];
    rl[1] = dl1[bb];
    rc[0] = dcode_a[(size_t)bb * 2];
    rc[1] = dcode_a[(size_t)bb * 2 + 1];
    rz[0] = zsrc[(size_t)bb * SW_Z];
    rz[1] = zsrc[(size_t)bb * SW_Z + 1];
  }
  for (int i = threadIdx.x; i < 16 * LD32; i += blockDim.x) smem[L.docode + i] = 0.f;
  // the eight transposed head matrices: with the registered images ONE contiguous block in the LDS layout of this kernel
  // (a float4 copy, no zero fill, no scalar scatter); from the weights every global load is issued before the zero fill
  disc_stage_headT(smem, L, true, d_w, O, K4, dimg, true, [&] {
    stage_zero(smem + L.of0T, L.dlab - L.of0T);  // transposed images are zero padded
    sw_barrier();
  });

  for (int k = 0; k < nb; ++k) {
    float* dpred = k == 0 ? dpred_a : dpred_b;
    sw_barrier();
    if (k == 0) SW_STAMP(8);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = threadIdx.x + SW_THREADS * e;
      if (i < 16 * LD16) {
        const int a = i / LD16, cc = i - a * LD16;
        const int bb = min(a0 + a, B - 1);
        const float xl = k == 0 ? hl[e][0] : hl[e][1], xc = k == 0 ? hc[e][0] : hc[e][1];
        float vl, vc;
        if (gl.on) {  // LSGAN / InfoGAN loss gradients formed here from the forward outputs (train.py:484-494, 512-523)
          const float tgt = k == 0 ? htg[0] : htg[1];
          vl = cc == 0 ? 2.0f * (xl - tgt) * gl.g_label : 0.f;
          vc = (k == 0 && cc < 2) ? 2.0f * (xc - hz[e]) * gl.g_code : 0.f;
        } else {
          vl = cc == 0 ? xl : 0.f;
          vc = cc < 2 ? xc : 0.f;
        }
        smem[L.dlab + i] = vl;
        smem[L.dcod + i] = vc;
        if (want_w && a0 + a < B && cc < 4) {
          ddelta[dd.dlab + ((size_t)k * B + bb) * 4 + cc] = vl;
          ddelta[dd.dcod + ((size_t)k * B + bb) * 4 + cc] = vc;
        }
      }
    }
    if (gl.on && gl.loss_part && wave == 3 && k < 2) {  // the reported MSE sums of this tile (train.py:484-488, 512-516)
      const bool lv = lane < 16 && a0 + lane < B;
      const float e = (k == 0 ? rl[0] : rl[1]) - (k == 0 ? htg[0] : htg[1]);
      float sl = lv ? e * e : 0.f, sc = 0.f;
      if (k == 0 && lv) {
        const float c0 = rc[0] - rz[0], c1 = rc[1] - rz[1];
        sc = c0 * c0 + c1 * c1;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        sl += __shfl_xor(sl, o);
        sc += __shfl_xor(sc, o);
      }
      if (lane == 0) {
        gl.loss_part[(size_t)blockIdx.x * 3 + (k == 0 ? 0 : 2)] = sl;
        if (k == 0) gl.loss_part[(size_t)blockIdx.x * 3 + 1] = sc;
      }
    }
    sw_barrier();
    // dc1 = (cl1^T dlabel) * lrelu'(c1)  (waves 0,1) ; dl1 = (la1^T dcode) * lrelu'(l1)  (waves 2,3)
    {
      int m0 = 16 * (wave & 1);
      bool cls = wave < 2;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_mm_rt(smem + (cls ? L.cl1T : L.la1T) + (m0 + ln) * LD16 + 4 * lg,
                       smem + (cls ? L.dlab : L.dcod) + ln * LD16 + 4 * lg, 1, acc);
      const f32x4 a = k == 0 ? pc1[0] : pc1[1];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = sw_lrelu_grad(a[r], acc[r]);
      st4(smem + (cls ? L.dc1 : L.dl1) + ln * LD32 + m0 + 4 * lg, acc);
      if (want_w && live) st4(ddelta + (cls ? dd.dc1 : dd.dl1) + ((size_t)k * B + b) * 32 + m0 + 4 * lg, acc);
    }
    sw_barrier();
    // dboth = cl0^T dc1 + la0^T dl1   (wave w: rows 16w..)
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_mm_rt(smem + L.cl0T + (u0 + ln) * LD32 + 4 * lg, smem + L.dc1 + ln * LD32 + 4 * lg, 2, acc);
      acc = tile_mm_rt(smem + L.la0T + (u0 + ln) * LD32 + 4 * lg, smem + L.dl1 + ln * LD32 + 4 * lg, 2, acc);
      st4(smem + L.dboth + ln * LD64 + u0 + 4 * lg, acc);
      if (wave < 2) {  // observation-code half: summed over branches
        float* p = smem + L.docode + ln * LD32 + u0 + 4 * lg;
        st4(p, ld4(p) + acc);
      } else if (want_w && live) {
        st4(ddelta + dd.dpcode + ((size_t)k * B + b) * 32 + (u0 - 32) + 4 * lg, acc);
      }
    }
    sw_barrier();
    // dq1 = (pe1^T dpcode) * lrelu'(q1)   (waves 0,1)
    if (wave < 2) {
      int m0 = 16 * wave;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_mm_rt(smem + L.pe1T + (m0 + ln) * LD32 + 4 * lg, smem + L.dboth + ln * LD64 + 32 + 4 * lg, 2, acc);
      const f32x4 a = k == 0 ? pq1[0] : pq1[1];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = sw_lrelu_grad(a[r], acc[r]);
      st4(smem + L.dq1 + ln * LD32 + m0 + 4 * lg, acc);
      if (want_w && live) st4(ddelta + dd.dq1 + ((size_t)k * B + b) * 32 + m0 + 4 * lg, acc);
    }
    sw_barrier();
    // dpred = pe0^T dq1   (4Tp rows)
    if (dpred) {
      for (int mt = wave; mt * 16 < K4; mt += 4) {
        int m0 = 16 * mt;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile_mm_rt(smem + L.pe0T + (m0 + ln) * LD32 + 4 * lg, smem + L.dq1 + ln * LD32 + 4 * lg, 2, acc);
        if (live && m0 + 4 * lg < K4) st4(dpred + (size_t)b * K4 + m0 + 4 * lg, acc);
      }
    }
  }
  if (!want_w) return;
  sw_barrier();
  SW_STAMP(9);
  // ---- observation path: of1, of0, LSTM BPTT -------------------------------------------------
  if (live && wave < 2) st4(ddelta + dd.docode + (size_t)b * 32 + u0 + 4 * lg, ld4(smem + L.docode + ln * LD32 + u0 + 4 * lg));
  f32x4 dh = disc_obs_bwd_tail(smem + L.of1T, smem + L.of0T, smem + L.docode, smem + L.do1, po1, ddelta + dd.do1 + (size_t)b * 32, live);
  f32x4 dc = {0.f, 0.f, 0.f, 0.f};
  LstmWT WT;
  lstm_load_whhT(WT, dimg, swdimg::OP_WHHT, d_w + O.whh, wave, lane);
  // the BPTT over the saved rows (sw_lstm_dev.h): c_{-1} = 0, padding lanes of the last tile store to the trash row
  const LstmBptt S{dsave + ds.act + (size_t)b * 384 + u0 + 4 * lg, nullptr, dgbuf, ddelta + dd.dgates + (size_t)a0 * 256,
                   ddelta + dd.trash, a0, B};
  lstm_bptt_rows<false>(WT, S, To, dh, dc, SwNop{}, [&](int k) { SW_STAMP(k); });
}

// ---------------------------------------------------------------------------------------------
// One discriminator UPDATE pass in ONE launch (train.py:476-495): forward of D on the fake and the real branch, the LSGAN /
// InfoGAN loss gradients (per-agent local: means over the batch, scale known up front) and the whole backward down to the
// delta rows the weight-gradient GEMM contracts over.  One workgroup per 16-agent tile; the two-launch form costs a launch,
// a second prologue and the round trip of the gates / every head activation through the save buffer.  The two branches share the observation encoding; their heads run
// SIDE BY SIDE on the two wave pairs (waves 0, 1: fake; 2, 3: real) - a head layer is 2 row tiles, so the pair that used
// to idle now carries the other branch - forward and backward.  Rows for the weight gradients (saved activations, deltas)
// are written exactly where sw_disc_fwd / sw_disc_bwd put them.  Needs the registered weight images (sw_disc_images).
// ---------------------------------------------------------------------------------------------
namespace {
struct UpdLds {
  int hbuf, hw, bias, hwT, x, q1, both, c1, l1, o1, total;          // forward carve
  int dlab, dcod, dc1, dl1, dboth, docode, do1, dend;                // deltas: alias the forward head weights (dead by then)
  int ldp;
  HeadLds F;      // offsets of the forward head weights (relative to 0: add hw - F.of0)
  HeadLdsB T;     // offsets of the transposed block (relative to T.of0T: add hwT)
};
__host__ __device__ inline UpdLds upd_lds(int Tp) {
  UpdLds U;
  U.F = head_lds(Tp, 0);
  U.T = head_lds_b(Tp, 0);
  U.ldp = U.F.ldp;
  int o = 0;
  U.hbuf = o; o += 2 * 16 * SW_HLD;
  U.hw = o; o += U.F.bias - U.F.of0;          // of0 | of1 | pe0 | pe1 | cl0 | la0 | cl1 | la1 (row-major, padded)
  U.bias = o; o += 8 * 32;
  U.hwT = o; o += U.T.dlab - U.T.of0T;        // the transposed block of the images (HeadLdsB layout)
  U.x = o; o += 2 * 16 * U.ldp;
  U.q1 = o; o += 2 * 16 * LD32;
  U.both = o; o += 2 * 16 * LD64;
  U.c1 = o; o += 2 * 16 * LD32;
  U.l1 = o; o += 2 * 16 * LD32;
  U.o1 = o; o += 16 * LD32;
  U.total = o;
  int d = U.hw;
  U.dlab = d; d += 2 * 16 * LD16;
  U.dcod = d; d += 2 * 16 * LD16;
  U.dc1 = d; d += 2 * 16 * LD32;
  U.dl1 = d; d += 2 * 16 * LD32;
  U.dboth = d; d += 2 * 16 * LD64;
  U.docode = d; d += 16 * LD32;
  U.do1 = d; d += 16 * LD32;
  U.dend = d;
  return U;
}
}  // namespace

// RAGGED (sw_disc_update_ragged): the observation pass starts row b at step s = To - obs_len[b] (clamped, obs_start) and
// keeps the zero state in front of it by a SELECT on the cell's result - the values lstm_obs_loop<0, SAVE_ROWS, true> leaves
// (sw_lstm_dev.h), its products per step included: the recurrent product stays on step 0.  Zero gates with zero c_t, c_{t-1}
// give zero gate gradients and dc_{t-1} = 0, so everything behind the observation pass - heads, loss gradients, BPTT - is
// the dense code.  A template parameter with obs_len as the LAST argument, as disc_score_kernel.  There is no precomputed
// observation pass for ragged rows (obs_pre = 0).
template <bool RAGGED>
__global__ __launch_bounds__(SW_THREADS) void disc_update_kernel(
    const float* __restrict__ obsv, int To, const float* __restrict__ pred_a, const float* __restrict__ pred_b,
    const float* __restrict__ d_w, int B, int Tp, float* __restrict__ label_a, float* __restrict__ label_b,
    float* __restrict__ code_a, float* __restrict__ code_b, float* __restrict__ dsave, int obs_pre, float* __restrict__ w_snap,
    DiscLoss gl, float* __restrict__ ddelta, const float* __restrict__ dimg, const int* __restrict__ obs_len) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const UpdLds U = upd_lds(Tp);
  const HeadLds& F = U.F;
  const HeadLdsB& T = U.T;
  const swp::Disc O = swp::disc(Tp);
  const DSave ds = dsave_layout(B, To, Tp, 2);
  const DDelta dd = ddelta_layout(B, To, Tp, 2);
  float* hbuf = smem + U.hbuf;
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int u0 = wave * 16, br = wave >> 1, wp = wave & 1;       // br: the branch this wave's pair owns, wp: wave in pair
  const int a0 = blockIdx.x * SW_TILE;
  const int b = min(a0 + ln, B - 1);
  const bool live = (a0 + ln) < B;
  const int K4 = 4 * Tp, ldp = U.ldp;
  float* hw = smem + U.hw - F.of0;      // forward head matrices and bias slots at their HeadLds offsets
  float* hwT = smem + U.hwT - T.of0T;   // transposed head matrices at their HeadLdsB offsets

  // ---- prologue: every global load first --------------------------------------------------------------------------
  float xpre[2][4];       // prediction rows of both branches (Tp <= 12 here)
  disc_xpre_load(xpre, pred_a, pred_b, a0, B, K4, ldp);
  const float tg0 = gl.targets[gl.t0], tg1 = gl.targets[gl.t1];
  const float z0 = gl.z[(size_t)b * SW_Z], z1 = gl.z[(size_t)b * SW_Z + 1];
  LstmW W;
  if (!obs_pre) disc_obs_operands(W, d_w, O, dimg);
  if (w_snap)   // deepcopy(D) of train.py:499: the weights this pass runs with
    for (int i = blockIdx.x * SW_THREADS + threadIdx.x; i < O.n; i += gridDim.x * SW_THREADS) w_snap[i] = d_w[i];
  disc_stage_heads(hw, F, d_w, O, K4, true);
  disc_stage_headT(hwT, T, true, nullptr, O, K4, dimg, false);   // the image block: one float4 copy (zero padding included)
  // prediction rows into LDS (zero padded) and into the save buffer (rows of the pe0 weight gradient)
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    disc_xpre_put(xpre, kk == 1, smem + U.x + kk * 16 * ldp, dsave + ds.px + (size_t)kk * B * K4, a0, B, K4, ldp);
  f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};
  disc_seed_h(hbuf, obs_pre, dsave + ds.act, To, B, b);
  sw_barrier();
  // The usual horizon (8 observed steps, train.py:44): the gates and cell states of the eight steps STAY IN REGISTERS
  // (160 of the 512 a wave owns at one wave per SIMD) for the BPTT below - only h (the operand of the LSTM's weight
  // gradient) and the step's input go to memory: a sixth of the saved bytes, no row loads in the BPTT.
  const bool reg8 = !obs_pre && To == 8;
  f32x4 sg[8][4], sc[8];
  int s0 = 0;             // RAGGED: the step this lane's row starts at (requested here: it arrives under the staging above)
  if constexpr (RAGGED) {
    __builtin_assume(obs_len != nullptr);
    s0 = obs_start(obs_len, b, To, 0);
  }
  if (reg8) {
    // lstm_obs_loop (sw_lstm_dev.h, with what it keeps) unrolled, the steps' gates and cell states left in sg / sc; only the
    // h row and the input go to dsave.  Dense: step 0 from h = 0 without recurrent products.  RAGGED: every lane computes
    // every step (W_hh h on step 0 too: exact zeros) and selects the zero state in front of its start, so sg[t] / sc[t] and
    // what goes to dsave hold SELECTED zeros there.  The stores stay unconditional.
    float xa, xq;
    if constexpr (RAGGED) obs_x4_load_from(obsv, b, 0, s0, 8, lg, xa, xq);
    else obs_x4_load(obsv, b, 0, 8, lg, xa, xq);
    asm volatile("" : "+v"(xa), "+v"(xq));
    float* hrow_g = dsave + ds.act + (size_t)b * 384 + 320 + u0 + 4 * lg;
    float* xrow = dsave + ds.x4s + (size_t)b * 4 + lg;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      float xb = xa - (lg >= 2 ? xq : 0.f);
      if constexpr (RAGGED) obs_x4_load_from(obsv, b, t + 1 < 8 ? t + 1 : 7, s0, 8, lg, xa, xq);
      else obs_x4_load(obsv, b, t + 1 < 8 ? t + 1 : 7, 8, lg, xa, xq);
      const float* hrow = &hbuf[(t & 1) * 16 * SW_HLD + ln * SW_HLD + 4 * lg];
      if (!RAGGED && t == 0) lstm_cell<false>(W, xb, hrow, sg[t], c, h);   // (unrolled: no branch)
      else lstm_cell(W, xb, hrow, sg[t], c, h);
      if constexpr (RAGGED) {
        const bool on = t >= s0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          c[r] = on ? c[r] : 0.f;
          h[r] = on ? h[r] : 0.f;
#pragma unroll
          for (int g = 0; g < 4; ++g) sg[t][g][r] = on ? sg[t][g][r] : 0.f;
        }
        xb = on ? xb : 0.f;
      }
      sc[t] = c;
      st4(&hbuf[((t + 1) & 1) * 16 * SW_HLD + ln * SW_HLD + u0 + 4 * lg], h);
      st4g(hrow_g, h);
      *xrow = xb;
      hrow_g += (size_t)B * 384;
      xrow += (size_t)B * 4;
      sw_barrier();
      asm volatile("" : "+v"(xa), "+v"(xq));
    }
  } else if (!obs_pre) {
    lstm_obs_loop<0, SAVE_ROWS, RAGGED>(W, hbuf, obsv, To, B, b, s0, false, c, h, dsave + ds.act, dsave + ds.x4s);
  }
  const float* hlast = &hbuf[(To & 1) * 16 * SW_HLD];

  // ---- observation fc (waves 0, 1) -> both[0 | 1][:, 0:32] --------------------------------------------------------------
  const f32x4 o1reg = disc_obs_fc(hw, F, hlast, smem + U.o1, dsave + ds.o1 + (size_t)b * 32, live, smem + U.both, 2);
  // ---- prediction heads, the two branches side by side: wave pair br, wave wp of the pair ------------------------------
  float* xb_ = smem + U.x + br * 16 * ldp;
  float* q1_ = smem + U.q1 + br * 16 * LD32;
  float* both_ = smem + U.both + br * 16 * LD64;
  float* c1_ = smem + U.c1 + br * 16 * LD32;
  float* l1_ = smem + U.l1 + br * 16 * LD32;
  const size_t kb = (size_t)br * B + b;
  f32x4 q1reg, c1reg, l1reg;
  {   // q1 = lrelu(pe0 x + b): row tile wp
    const int m0 = 16 * wp;
    f32x4 acc = ld4(smem + U.bias + 2 * 32 + m0 + 4 * lg);
    acc = tile_mm_rt(hw + F.pe0 + (m0 + ln) * ldp + 4 * lg, xb_ + ln * ldp + 4 * lg, (ldp - 4) / 16, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = sw_lrelu(acc[r]);
    q1reg = acc;
    st4(q1_ + ln * LD32 + m0 + 4 * lg, acc);
    if (live) st4(dsave + ds.q1 + kb * 32 + m0 + 4 * lg, acc);
  }
  sw_barrier();
  {   // pred_code = pe1 q1 + b -> both[br][:, 32:64]
    // (of0 / of1 are dead behind the barrier above: the dlab | dcod delta tiles that alias them are zeroed here - only
    //  their columns 0 / 0..1 are written later)
    stage_zero(smem + U.dlab, U.dc1 - U.dlab);
    const int m0 = 16 * wp;
    f32x4 acc = ld4(smem + U.bias + 3 * 32 + m0 + 4 * lg);
    acc = tile_mm_rt(hw + F.pe1 + (m0 + ln) * LD32 + 4 * lg, q1_ + ln * LD32 + 4 * lg, 2, acc);
    st4(both_ + ln * LD64 + 32 + m0 + 4 * lg, acc);
  }
  sw_barrier();
  {   // both codes saved (wave wp: columns 32 wp ..), then c1 = lrelu(cl0 both + b), l1 = lrelu(la0 both + b): row tile wp each
    if (live) {
      st4(dsave + ds.both + kb * 64 + 32 * wp + 4 * lg, ld4(both_ + ln * LD64 + 32 * wp + 4 * lg));
      st4(dsave + ds.both + kb * 64 + 32 * wp + 16 + 4 * lg, ld4(both_ + ln * LD64 + 32 * wp + 16 + 4 * lg));
    }
    const int m0 = 16 * wp;
    f32x4 ac = ld4(smem + U.bias + 4 * 32 + m0 + 4 * lg), al = ld4(smem + U.bias + 5 * 32 + m0 + 4 * lg);
    ac = tile_mm_rt(hw + F.cl0 + (m0 + ln) * LD64 + 4 * lg, both_ + ln * LD64 + 4 * lg, 4, ac);
    al = tile_mm_rt(hw + F.la0 + (m0 + ln) * LD64 + 4 * lg, both_ + ln * LD64 + 4 * lg, 4, al);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ac[r] = sw_lrelu(ac[r]);
      al[r] = sw_lrelu(al[r]);
    }
    c1reg = ac;
    l1reg = al;
    st4(c1_ + ln * LD32 + m0 + 4 * lg, ac);
    st4(l1_ + ln * LD32 + m0 + 4 * lg, al);
    if (live) {
      st4(dsave + ds.c1 + kb * 32 + m0 + 4 * lg, ac);
      st4(dsave + ds.l1 + kb * 32 + m0 + 4 * lg, al);
    }
  }
  sw_barrier();     // every reader of the forward head matrices up to la0 is done: the delta tiles overwrite them from here on
  // ---- label = cl1 c1 + b (wave wp = 0), code_hat = la1 l1 + b (wp = 1); loss gradients (train.py:484-494) + reported sums
  {
    const bool cls = wp == 0;
    f32x4 acc = ld4(smem + U.bias + (cls ? 6 : 7) * 32 + 4 * lg);
    acc = tile_mm_rt(hw + (cls ? F.cl1 : F.la1) + ln * LD32 + 4 * lg, (cls ? c1_ : l1_) + ln * LD32 + 4 * lg, 2, acc);
    float* label = br == 0 ? label_a : label_b;
    float* code = br == 0 ? code_a : code_b;
    float sl = 0.f;
    if (lg == 0) {
      if (cls) {
        if (live) label[b] = acc[0];
        const float e = acc[0] - (br == 0 ? tg0 : tg1);
        const float g = 2.0f * e * gl.g_label;
        smem[U.dlab + br * 16 * LD16 + ln * LD16] = g;
        if (live) st4(ddelta + dd.dlab + kb * 4, f32x4{g, 0.f, 0.f, 0.f});
        sl = live ? e * e : 0.f;
      } else {
        if (live) { code[(size_t)b * 2] = acc[0]; code[(size_t)b * 2 + 1] = acc[1]; }
        const float e0 = acc[0] - z0, e1 = acc[1] - z1;
        const float g0 = br == 0 ? 2.0f * e0 * gl.g_code : 0.f, g1 = br == 0 ? 2.0f * e1 * gl.g_code : 0.f;   // info term: fake branch only
        smem[U.dcod + br * 16 * LD16 + ln * LD16] = g0;
        smem[U.dcod + br * 16 * LD16 + ln * LD16 + 1] = g1;
        if (live) st4(ddelta + dd.dcod + kb * 4, f32x4{g0, g1, 0.f, 0.f});
        sl = live ? e0 * e0 + e1 * e1 : 0.f;
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sl += __shfl_xor(sl, o);
    if (gl.loss_part && lane == 0) {
      if (cls) gl.loss_part[(size_t)blockIdx.x * 3 + (br == 0 ? 0 : 2)] = sl;
      else if (br == 0) gl.loss_part[(size_t)blockIdx.x * 3 + 1] = sl;
    }
  }
  sw_barrier();
  // ---- backward of the heads, branches side by side ------------------------------------------------------------------
  float* dlab_ = smem + U.dlab + br * 16 * LD16;
  float* dcod_ = smem + U.dcod + br * 16 * LD16;
  float* dc1_ = smem + U.dc1 + br * 16 * LD32;
  float* dl1_ = smem + U.dl1 + br * 16 * LD32;
  float* dboth_ = smem + U.dboth + br * 16 * LD64;
  {   // dc1 = (cl1^T dlabel) * lrelu'(c1), dl1 = (la1^T dcode) * lrelu'(l1): row tile wp each
    const int m0 = 16 * wp;
    f32x4 ac = {0.f, 0.f, 0.f, 0.f}, al = ac;
    ac = tile_mm_rt(hwT + T.cl1T + (m0 + ln) * LD16 + 4 * lg, dlab_ + ln * LD16 + 4 * lg, 1, ac);
    al = tile_mm_rt(hwT + T.la1T + (m0 + ln) * LD16 + 4 * lg, dcod_ + ln * LD16 + 4 * lg, 1, al);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ac[r] = sw_lrelu_grad(c1reg[r], ac[r]);
      al[r] = sw_lrelu_grad(l1reg[r], al[r]);
    }
    st4(dc1_ + ln * LD32 + m0 + 4 * lg, ac);
    st4(dl1_ + ln * LD32 + m0 + 4 * lg, al);
    if (live) {
      st4(ddelta + dd.dc1 + kb * 32 + m0 + 4 * lg, ac);
      st4(ddelta + dd.dl1 + kb * 32 + m0 + 4 * lg, al);
    }
  }
  sw_barrier();
  {   // dboth = cl0^T dc1 + la0^T dl1 (64 rows): row tiles 2 wp, 2 wp + 1
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m0 = 16 * (2 * wp + q);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_mm_rt(hwT + T.cl0T + (m0 + ln) * LD32 + 4 * lg, dc1_ + ln * LD32 + 4 * lg, 2, acc);
      acc = tile_mm_rt(hwT + T.la0T + (m0 + ln) * LD32 + 4 * lg, dl1_ + ln * LD32 + 4 * lg, 2, acc);
      st4(dboth_ + ln * LD64 + m0 + 4 * lg, acc);
      if (wp == 1 && live) st4(ddelta + dd.dpcode + kb * 32 + (m0 - 32) + 4 * lg, acc);   // the prediction-code half
    }
  }
  sw_barrier();
  {   // dq1 = (pe1^T dpcode) * lrelu'(q1): row tile wp (only the weight gradient needs it: D updates want no d/dpred)
    const int m0 = 16 * wp;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = tile_mm_rt(hwT + T.pe1T + (m0 + ln) * LD32 + 4 * lg, dboth_ + ln * LD64 + 32 + 4 * lg, 2, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = sw_lrelu_grad(q1reg[r], acc[r]);
    if (live) st4(ddelta + dd.dq1 + kb * 32 + m0 + 4 * lg, acc);
  }
  if (wave < 2) {   // observation-code half summed over the branches (fixed order), then do1 = (of1^T docode) * lrelu'(o1)
    const int m0 = 16 * wave;
    const f32x4 v = ld4(smem + U.dboth + ln * LD64 + m0 + 4 * lg) + ld4(smem + U.dboth + 16 * LD64 + ln * LD64 + m0 + 4 * lg);
    st4(smem + U.docode + ln * LD32 + m0 + 4 * lg, v);
    if (live) st4(ddelta + dd.docode + (size_t)b * 32 + m0 + 4 * lg, v);
  }
  sw_barrier();
  // ---- observation backward: do1, dh_T = of0^T do1, then the BPTT (sw_lstm_dev.h: c_{-1} = 0, padding rows to the trash row)
  f32x4 dh = disc_obs_bwd_tail(hwT + T.of1T, hwT + T.of0T, smem + U.docode, smem + U.do1, o1reg, ddelta + dd.do1 + (size_t)b * 32, live);
  f32x4 dc = {0.f, 0.f, 0.f, 0.f};
  LstmWT WT;
  lstm_load_whhT(WT, dimg, swdimg::OP_WHHT, nullptr, wave, lane);
  // the dgates tiles [2][16][SW_GLD] lie over the prediction heads' transposed images (dead now)
  const LstmBptt S{dsave + ds.act + (size_t)b * 384 + u0 + 4 * lg, nullptr, hwT + T.pe0T, ddelta + dd.dgates + (size_t)a0 * 256,
                   ddelta + dd.trash, a0, B};
  // (both paths: a barrier in front of the first step - every wave has read of0T / do1; the dgates tiles start behind
  //  of0T / of1T, kept for symmetry with disc_bwd)
  if (reg8) {        // the eight steps' gates / cell states are in registers: no row traffic at all
    sw_barrier();
#pragma unroll
    for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(WT.whhT[j]));
#pragma unroll
    for (int t = 7; t >= 1; --t) lstm_bptt_step<false, false, true>(WT, S, t, sg[t], sc[t], sc[t - 1], dh, dc);
    f32x4 c_1 = {0.f, 0.f, 0.f, 0.f};   // c_{-1} = 0
    lstm_bptt_step<false, false, false>(WT, S, 0, sg[0], sc[0], c_1, dh, dc);
    return;
  }
  lstm_bptt_rows<false>(WT, S, To, dh, dc, SwNop{}, [](int k) {
    if (k == 10) sw_barrier();   // behind the request of the first rows
  });
}

static int g_disc_fwd_lds = 0;   // dynamic-LDS limit of disc_fwd_kernel (plain + fused launches, sw_set_lds)

size_t sw_dsave_floats(int B, int To, int Tp, int nb) { return dsave_layout(B, To, Tp, nb).total; }
size_t sw_ddelta_floats(int B, int To, int Tp, int nb) { return ddelta_layout(B, To, Tp, nb).total; }

static int g_disc_fwd_ragged_lds = 0;   // ... of disc_fwd_ragged_kernel

// sw_disc_fwd and sw_disc_fwd_ragged: one set of checks, one grid rule; the dense entry launches the dense kernel
static int disc_fwd_launch(bool ragged, const float* obsv, int To, int x_mode, const int* obs_len, const float* const* pred4, int nb,
                           const float* d_w, int B, int Tp, float* const* label, float* const* code, float* dsave,
                           int save_lstm, float* w_snapshot, void* stream) {
  if (!obsv || !pred4 || !d_w || !label || !code || nb < 1 || nb > SW_DISC_MAXB || B < 0 || To < 1 || Tp < 1 ||
      (x_mode != 0 && x_mode != 1) || (x_mode == 0 && To < 2) || save_lstm < 0 || save_lstm > 2 || (save_lstm == 2 && !dsave))
    return SW_EARG;
  if (ragged && save_lstm == 2) return SW_EARG;   // no precomputed observation pass for ragged rows
  for (int k = 0; k < nb; ++k)
    if (!pred4[k] || !label[k] || !code[k]) return SW_EARG;
  if (Tp > 64) return SW_ESHAPE;
  if (B == 0) return SW_OK;
  int lds = head_lds(Tp, 2 * 16 * SW_HLD + 1280).total * 4;
  if (lds > 163840) return SW_ESHAPE;
  if (int rc = ragged ? sw_set_lds((const void*)disc_fwd_ragged_kernel, lds, g_disc_fwd_ragged_lds)
                      : sw_set_lds((const void*)disc_fwd_kernel, lds, g_disc_fwd_lds))
    return rc;
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  const int split = (nb == 2 && 2 * tiles <= SW_SPLIT_MAX_WGS) ? 1 : 0;   // idle CUs: one workgroup per (tile, branch)
  if (ragged) {
    SW_LAUNCH(disc_fwd_ragged_kernel, dim3(split ? 2 * tiles : tiles), dim3(SW_THREADS), lds, (hipStream_t)stream,
                       obsv, To, x_mode, pred4[0], nb > 1 ? pred4[1] : nullptr, nb, d_w, B, Tp, label[0],
                       nb > 1 ? label[1] : nullptr, code[0], nb > 1 ? code[1] : nullptr, dsave, save_lstm, split, w_snapshot, 0, DiscLoss{}, nullptr,
                       sw_disc_images_for(d_w, Tp).img, obs_len);
    SW_CHECK_LAUNCH("disc_fwd_ragged_kernel");
    return SW_OK;
  }
  SW_LAUNCH(disc_fwd_kernel, dim3(split ? 2 * tiles : tiles), dim3(SW_THREADS), lds, (hipStream_t)stream,
                     obsv, To, x_mode, pred4[0], nb > 1 ? pred4[1] : nullptr, nb, d_w, B, Tp, label[0],
                     nb > 1 ? label[1] : nullptr, code[0], nb > 1 ? code[1] : nullptr, dsave, save_lstm, split, w_snapshot, 0, DiscLoss{}, nullptr,
                     sw_disc_images_for(d_w, Tp).img);
  SW_CHECK_LAUNCH("disc_fwd_kernel");
  return SW_OK;
}
extern "C" int sw_disc_fwd(const float* obsv, int To, int x_mode, const float* const* pred4, int nb,
                           const float* d_w, int B, int Tp, float* const* label, float* const* code, float* dsave,
                           int save_lstm, float* w_snapshot, void* stream) {
  return disc_fwd_launch(false, obsv, To, x_mode, nullptr, pred4, nb, d_w, B, Tp, label, code, dsave, save_lstm, w_snapshot, stream);
}
extern "C" int sw_disc_fwd_ragged(const float* obsv, int To, int x_mode, const int* obs_len, const float* const* pred4, int nb,
                                  const float* d_w, int B, int Tp, float* const* label, float* const* code, float* dsave,
                                  int save_lstm, float* w_snapshot, void* stream) {
  return disc_fwd_launch(true, obsv, To, x_mode, obs_len, pred4, nb, d_w, B, Tp, label, code, dsave, save_lstm, w_snapshot, stream);
}

// Generator phase in ONE launch: forward of D on (obsv, pred_hat) and the backward of its prediction heads down to
// d(g_loss)/d(pred_hat) (train.py:510-523, 538): no saves, no second prologue, activations stay in LDS.
// sw_disc_dpred and sw_disc_dpred_ragged: one set of checks; the dense entry launches the dense kernel
static int disc_dpred_launch(bool ragged, const float* obsv, int To, int x_mode, const int* obs_len, const float* pred4,
                             const float* d_w, int B, int Tp, const float* targets, int t_idx, const float* z, float g_label,
                             float g_code, float* dpred4, float* label, float* code, float* loss_part, void* stream) {
  if (!obsv || !pred4 || !d_w || !targets || !z || !dpred4 || B < 0 || To < 1 || Tp < 1 || t_idx < 0 ||
      (x_mode != 0 && x_mode != 1) || (x_mode == 0 && To < 2))
    return SW_EARG;
  if (Tp > 64) return SW_ESHAPE;
  if (B == 0) return SW_OK;
  const int lds = disc_dpred_lds(Tp);
  if (lds > 163840) return SW_ESHAPE;
  if (int rc = ragged ? sw_set_lds((const void*)disc_fwd_ragged_kernel, lds, g_disc_fwd_ragged_lds)
                      : sw_set_lds((const void*)disc_fwd_kernel, lds, g_disc_fwd_lds))
    return rc;
  DiscLoss gl{targets, z, t_idx, t_idx, g_label, g_code, 1, loss_part};
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  if (ragged) {
    SW_LAUNCH(disc_fwd_ragged_kernel, dim3(tiles), dim3(SW_THREADS), lds, (hipStream_t)stream, obsv, To, x_mode, pred4,
                       (const float*)nullptr, 1, d_w, B, Tp, label, (float*)nullptr, code, (float*)nullptr, (float*)nullptr, 0, 0,
                       (float*)nullptr, 1, gl, dpred4, sw_disc_images_for(d_w, Tp).img, obs_len);
    SW_CHECK_LAUNCH("disc_fwd_ragged_kernel");
    return SW_OK;
  }
  SW_LAUNCH(disc_fwd_kernel, dim3(tiles), dim3(SW_THREADS), lds, (hipStream_t)stream, obsv, To, x_mode, pred4,
                     (const float*)nullptr, 1, d_w, B, Tp, label, (float*)nullptr, code, (float*)nullptr, (float*)nullptr, 0, 0,
                     (float*)nullptr, 1, gl, dpred4, sw_disc_images_for(d_w, Tp).img);
  SW_CHECK_LAUNCH("disc_fwd_kernel");
  return SW_OK;
}
extern "C" int sw_disc_dpred(const float* obsv, int To, int x_mode, const float* pred4, const float* d_w, int B, int Tp,
                             const float* targets, int t_idx, const float* z, float g_label, float g_code,
                             float* dpred4, float* label, float* code, float* loss_part, void* stream) {
  return disc_dpred_launch(false, obsv, To, x_mode, nullptr, pred4, d_w, B, Tp, targets, t_idx, z, g_label, g_code, dpred4, label, code,
                           loss_part, stream);
}
extern "C" int sw_disc_dpred_ragged(const float* obsv, int To, int x_mode, const int* obs_len, const float* pred4, const float* d_w,
                                    int B, int Tp, const float* targets, int t_idx, const float* z, float g_label, float g_code,
                                    float* dpred4, float* label, float* code, float* loss_part, void* stream) {
  return disc_dpred_launch(true, obsv, To, x_mode, obs_len, pred4, d_w, B, Tp, targets, t_idx, z, g_label, g_code, dpred4, label, code,
                           loss_part, stream);
}

// ---------------------------------------------------------------------------------------------
// Scoring K sampled futures per agent (sw_disc_score): the discriminator-side twin of dec_sample_fwd_kernel.  Workgroup
// (tile, k-group) runs the observation LSTM and the observation fc of its 16-agent tile ONCE, then the prediction heads
// for every draw of its k-range, reading row k B + a of pred4 in place: two draws per pass, side by side on the two wave
// pairs (waves 0, 1: draw k; 2, 3: draw k + 1 - a head layer is 2 row tiles, as in disc_update_kernel).  Every row goes
// through the tile_mm_rt chains of disc_fwd_tile in its order, so score / code carry the bits of sw_disc_fwd(nb = 1) on
// that draw.  Nothing is saved, every output element has one owner.
// ---------------------------------------------------------------------------------------------
namespace {
struct ScoreLds {
  HeadLds F;                            // forward head matrices, bias slots, o1 (at their HeadLds offsets)
  int x, q1, both, c1, l1, total;       // two draw tiles each
};
__host__ __device__ inline ScoreLds score_lds(int Tp) {
  ScoreLds S;
  S.F = head_lds(Tp, 2 * 16 * SW_HLD);
  int o = S.F.o1 + 16 * LD32;
  // the prediction rows and q1 lie over of0 / of1 (their only readers, the observation fc, are done by then)
  if (2 * 16 * S.F.ldp <= 32 * LD64) S.x = S.F.of0;
  else { S.x = o; o += 2 * 16 * S.F.ldp; }
  S.q1 = S.F.of1;                       // 32 * LD32 = 2 x [16][LD32]
  S.both = o; o += 2 * 16 * LD64;
  S.c1 = o; o += 2 * 16 * LD32;
  S.l1 = o; o += 2 * 16 * LD32;
  S.total = o;
  return S;
}
}  // namespace

// RAGGED: the observation pass starts row b at step To - obs_len[b] (lstm_obs_loop<., ., true>); everything behind it is the
// same code.  A template parameter with obs_len as the LAST argument: the dense instance keeps its argument layout.
template <bool RAGGED>
__global__ __launch_bounds__(SW_THREADS) void disc_score_kernel(
    const float* __restrict__ obsv, int To, int x_mode, const float* __restrict__ pred4, const float* __restrict__ d_w, int B, int K,
    int Tp, float* __restrict__ score, float* __restrict__ code, int tiles, int kgroups, const float* __restrict__ dimg,
    const int* __restrict__ obs_len) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* hbuf = smem;                   // [2][16][SW_HLD]
  const ScoreLds S = score_lds(Tp);
  const HeadLds& F = S.F;
  const swp::Disc O = swp::disc(Tp);
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int br = wave >> 1, wp = wave & 1;              // br: the draw slot this wave's pair owns, wp: wave in the pair
  const int kg = blockIdx.x / tiles;
  const int a0 = (blockIdx.x - kg * tiles) * SW_TILE;
  const int k_lo = (int)(((long long)kg * K) / kgroups), k_hi = (int)(((long long)(kg + 1) * K) / kgroups);
  const int b = min(a0 + ln, B - 1);
  const bool live = (a0 + ln) < B;
  const int K4 = 4 * Tp, ldp = F.ldp;
  const size_t draw = (size_t)B * K4;                    // floats of one draw of pred4

  // the first two draws' prediction rows are requested now (longer horizons than Tp = 12 load in place)
  const bool x_pre = 16 * ldp <= 4 * SW_THREADS;
  float xpre[2][4];
  disc_xpre_load(xpre, pred4 + (size_t)k_lo * draw, pred4 + (size_t)min(k_lo + 1, k_hi - 1) * draw, a0, B, K4, ldp);
  LstmW W;
  disc_obs_operands(W, d_w, O, dimg);
  disc_stage_heads(smem, F, d_w, O, K4, 32 * (ldp >> 2) <= 2 * SW_THREADS);
  f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};   // h0 = c0 = 0 (train.py:296-297)
  disc_seed_h(hbuf, false, nullptr, To, B, b);
  sw_barrier();
  lstm_obs_pass<RAGGED>(x_mode, false, W, hbuf, obsv, To, B, b, RAGGED ? obs_start(obs_len, b, To, x_mode) : 0, c, h, nullptr, nullptr);
  // observation fc (waves 0, 1) -> both[0 | 1][:, 0:32]
  disc_obs_fc(smem, F, &hbuf[(To & 1) * 16 * SW_HLD], smem + F.o1, nullptr, live, smem + S.both, 2);

  float* x_ = smem + S.x + br * 16 * ldp;
  float* q1_ = smem + S.q1 + br * 16 * LD32;
  float* both_ = smem + S.both + br * 16 * LD64;
  float* c1_ = smem + S.c1 + br * 16 * LD32;
  float* l1_ = smem + S.l1 + br * 16 * LD32;
  const int m0 = 16 * wp;
  for (int k = k_lo; k < k_hi; k += 2) {
    const int k1 = min(k + 1, k_hi - 1);                 // an odd tail: slot 1 repeats draw k and stores nothing
    sw_barrier();                                        // the observation fc / the previous pair are done with these tiles
    if (x_pre) {
#pragma unroll
      for (int s = 0; s < 2; ++s) disc_xpre_put(xpre, s == 1, smem + S.x + s * 16 * ldp, nullptr, a0, B, K4, ldp);
      if (k + 2 < k_hi)                                  // the next pair's rows arrive under this pair's heads
        disc_xpre_load(xpre, pred4 + (size_t)(k + 2) * draw, pred4 + (size_t)min(k + 3, k_hi - 1) * draw, a0, B, K4, ldp);
    } else {
      for (int i = threadIdx.x; i < 2 * 16 * ldp; i += SW_THREADS) {
        const int s = i / (16 * ldp), r = i - s * 16 * ldp;
        const int a = r / ldp, cc = r - a * ldp;
        smem[S.x + i] = cc < K4 ? pred4[(size_t)(s ? k1 : k) * draw + (size_t)min(a0 + a, B - 1) * K4 + cc] : 0.f;
      }
    }
    sw_barrier();
    {   // q1 = lrelu(pe0 x + b): row tile wp
      f32x4 acc = ld4(smem + F.bias + 2 * 32 + m0 + 4 * lg);
      acc = tile_mm_rt(smem + F.pe0 + (m0 + ln) * ldp + 4 * lg, x_ + ln * ldp + 4 * lg, (ldp - 4) / 16, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = sw_lrelu(acc[r]);
      st4(q1_ + ln * LD32 + m0 + 4 * lg, acc);
    }
    sw_barrier();
    {   // pred_code = pe1 q1 + b -> both[br][:, 32:64]
      f32x4 acc = ld4(smem + F.bias + 3 * 32 + m0 + 4 * lg);
      acc = tile_mm_rt(smem + F.pe1 + (m0 + ln) * LD32 + 4 * lg, q1_ + ln * LD32 + 4 * lg, 2, acc);
      st4(both_ + ln * LD64 + 32 + m0 + 4 * lg, acc);
    }
    sw_barrier();
    {   // c1 = lrelu(cl0 both + b), l1 = lrelu(la0 both + b): row tile wp each
      f32x4 ac = ld4(smem + F.bias + 4 * 32 + m0 + 4 * lg), al = ld4(smem + F.bias + 5 * 32 + m0 + 4 * lg);
      ac = tile_mm_rt(smem + F.cl0 + (m0 + ln) * LD64 + 4 * lg, both_ + ln * LD64 + 4 * lg, 4, ac);
      al = tile_mm_rt(smem + F.la0 + (m0 + ln) * LD64 + 4 * lg, both_ + ln * LD64 + 4 * lg, 4, al);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ac[r] = sw_lrelu(ac[r]);
        al[r] = sw_lrelu(al[r]);
      }
      st4(c1_ + ln * LD32 + m0 + 4 * lg, ac);
      st4(l1_ + ln * LD32 + m0 + 4 * lg, al);
    }
    sw_barrier();
    {   // score = cl1 c1 + b (wave wp = 0), code_hat = la1 l1 + b (wp = 1)
      const bool cls = wp == 0;
      f32x4 acc = ld4(smem + F.bias + (cls ? 6 : 7) * 32 + 4 * lg);
      acc = tile_mm_rt(smem + (cls ? F.cl1 : F.la1) + ln * LD32 + 4 * lg, (cls ? c1_ : l1_) + ln * LD32 + 4 * lg, 2, acc);
      if (lg == 0 && live && k + br < k_hi) {
        const size_t r = (size_t)(k + br) * B + b;
        if (cls) score[r] = acc[0];
        else if (code) { code[r * 2] = acc[0]; code[r * 2 + 1] = acc[1]; }
      }
    }
  }
}

// The k-groups of a scoring launch: every group repeats the observation pass of its tile (8 LSTM steps against 2 head
// passes per draw pair), so groups are added only while the launch leaves CUs idle, and never below one draw pair each.
static int disc_score_kgroups(int tiles, int K) {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = SW_SPLIT_MAX_WGS;
    cus = n;
  }
  const int by_cu = cus / tiles, by_k = (K + 1) / 2;
  const int g = by_cu < by_k ? by_cu : by_k;
  return g < 1 ? 1 : g;
}

// sw_disc_score and sw_disc_score_ragged: one set of checks, one grid rule; the dense entry launches the dense kernel
static int disc_score_launch(bool ragged, const float* obsv, int To, int x_mode, const int* obs_len, const float* pred4,
                             const float* d_w, int B, int K, int Tp, float* score, float* code, void* stream) {
  if (!obsv || !pred4 || !d_w || !score || K < 1 || B < 0 || To < 1 || Tp < 1 || (x_mode != 0 && x_mode != 1) ||
      (x_mode == 0 && To < 2))
    return SW_EARG;
  if (Tp > 64) return SW_ESHAPE;
  if (B == 0) return SW_OK;
  const int lds = score_lds(Tp).total * 4;
  if (lds > 163840) return SW_ESHAPE;
  static int have = 0, have_ragged = 0;
  if (int rc = ragged ? sw_set_lds((const void*)disc_score_kernel<true>, lds, have_ragged)
                      : sw_set_lds((const void*)disc_score_kernel<false>, lds, have))
    return rc;
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  const int kgroups = disc_score_kgroups(tiles, K);
  if ((long long)tiles * kgroups > 0x7fffffffLL) return SW_ESHAPE;
  const float* dimg = sw_disc_images_for(d_w, Tp).img;
  if (ragged)
    SW_LAUNCH(disc_score_kernel<true>, dim3((unsigned)(tiles * kgroups)), dim3(SW_THREADS), lds, (hipStream_t)stream, obsv, To, x_mode,
              pred4, d_w, B, K, Tp, score, code, tiles, kgroups, dimg, obs_len);
  else
    SW_LAUNCH(disc_score_kernel<false>, dim3((unsigned)(tiles * kgroups)), dim3(SW_THREADS), lds, (hipStream_t)stream, obsv, To, x_mode,
              pred4, d_w, B, K, Tp, score, code, tiles, kgroups, dimg, (const int*)nullptr);
  SW_CHECK_LAUNCH("disc_score_kernel");
  return SW_OK;
}
extern "C" int sw_disc_score(const float* obsv, int To, int x_mode, const float* pred4, const float* d_w, int B, int K, int Tp,
                             float* score, float* code, void* stream) {
  return disc_score_launch(false, obsv, To, x_mode, nullptr, pred4, d_w, B, K, Tp, score, code, stream);
}
extern "C" int sw_disc_score_ragged(const float* obsv, int To, int x_mode, const int* obs_len, const float* pred4, const float* d_w,
                                    int B, int K, int Tp, float* score, float* code, void* stream) {
  return disc_score_launch(true, obsv, To, x_mode, obs_len, pred4, d_w, B, K, Tp, score, code, stream);
}

extern "C" int sw_disc_dpred_supported(int Tp) { return Tp >= 1 && Tp <= 64 && disc_dpred_lds(Tp) <= 163840 ? 1 : 0; }

// the weight-gradient problems of a discriminator pass over its saved / delta rows (dW = delta^T act per layer)
static int disc_wgrad_problems(WgBatch& wb, const float* dsave, float* ddelta, int nb, int B, int To, int Tp, float* d_d_w) {
  const swp::Disc O = swp::disc(Tp);
  const DSave ds = dsave_layout(B, To, Tp, nb);
  const DDelta dd = ddelta_layout(B, To, Tp, nb);
  const int R = nb * B, K4 = 4 * Tp;
  int rc_add = 0;
  // LSTM: dW_hh over rows t >= 1 against h_{t-1}; dW_ih / biases over all rows against x4
  rc_add |= wg_add_tail(wb, ddelta + dd.dgates, 256, dsave + ds.act + 320 - (ptrdiff_t)B * 384, 384, To * B, 256, 64,
                        d_d_w + O.whh, 64, dsave + ds.x4s, 4, 4, d_d_w + O.wih, 4, B /*h_{t-1}: rows t >= 1*/,
                        d_d_w + O.bih, d_d_w + O.bhh, 0);
  rc_add |= wg_add(wb, ddelta + dd.do1, 32, dsave + ds.act + (size_t)(To - 1) * B * 384 + 320, 384, B, 32, 64, d_d_w + O.of0w,
                   64, d_d_w + O.of0b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.docode, 32, dsave + ds.o1, 32, B, 32, 32, d_d_w + O.of1w, 32, d_d_w + O.of1b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.dq1, 32, dsave + ds.px, K4, R, 32, K4, d_d_w + O.pe0w, K4, d_d_w + O.pe0b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.dpcode, 32, dsave + ds.q1, 32, R, 32, 32, d_d_w + O.pe1w, 32, d_d_w + O.pe1b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.dc1, 32, dsave + ds.both, 64, R, 32, 64, d_d_w + O.cl0w, 64, d_d_w + O.cl0b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.dlab, 4, dsave + ds.c1, 32, R, 1, 32, d_d_w + O.cl1w, 32, d_d_w + O.cl1b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.dl1, 32, dsave + ds.both, 64, R, 32, 64, d_d_w + O.la0w, 64, d_d_w + O.la0b, nullptr, 0);
  rc_add |= wg_add(wb, ddelta + dd.dcod, 4, dsave + ds.l1, 32, R, 2, 32, d_d_w + O.la1w, 32, d_d_w + O.la1b, nullptr, 0);
  return rc_add ? SW_ESHAPE : SW_OK;
}

static int disc_bwd_impl(const float* d_w, const float* dsave, const float* const* dlabel, const float* const* dcode,
                         int nb, int B, int To, int Tp, float* ddelta, float* d_d_w, float* const* dpred4,
                         float* wgrad_ws, void* stream, DiscLoss gl, const WgAdam& adam = WgAdam()) {
  if (!d_w || !dsave || !dlabel || !dcode || nb < 1 || nb > SW_DISC_MAXB || B < 0 || To < 1 || Tp < 1) return SW_EARG;
  for (int k = 0; k < nb; ++k)
    if (!dlabel[k] || !dcode[k]) return SW_EARG;
  if (d_d_w && (!ddelta || !wgrad_ws)) return SW_EARG;
  if (Tp > 64) return SW_ESHAPE;
  if (B == 0) return SW_OK;
  int lds = head_lds_b(Tp, 0).total * 4;
  if (lds > 163840) return SW_ESHAPE;
  static int have = 0;
  if (int rc = sw_set_lds((const void*)disc_bwd_kernel, lds, have)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  WgBatch wb;
  if (d_d_w)
    if (int rc = disc_wgrad_problems(wb, dsave, ddelta, nb, B, To, Tp, d_d_w)) return rc;
  SW_LAUNCH(disc_bwd_kernel, dim3(tiles), dim3(SW_THREADS), lds, st, d_w, dsave,
                     dlabel[0], nb > 1 ? dlabel[1] : nullptr, dcode[0], nb > 1 ? dcode[1] : nullptr, nb, B, To, Tp,
                     d_d_w ? 1 : 0, ddelta, dpred4 ? dpred4[0] : nullptr, (dpred4 && nb > 1) ? dpred4[1] : nullptr, gl,
                     sw_disc_images_for(d_w, Tp).img);
  SW_CHECK_LAUNCH("disc_bwd_kernel");
  if (!d_d_w) return SW_OK;
  WgAdam ad = adam;
  return wg_launch_adam(wb, wgrad_ws, ad, st);
}

// The Adam update riding in the weight-gradient reduction (none without adam_w); D's registered images follow it element by element
static WgAdam disc_adam(float* w, float* m, float* v, const float* step, float* g, double lr, double beta1, double beta2, double eps,
                        int Tp) {
  WgAdam ad;
  if (!w) return ad;
  ad.w = w; ad.m = m; ad.v = v; ad.g0 = g; ad.step = step;
  ad.lr = lr; ad.beta1 = beta1; ad.beta2 = beta2; ad.eps = eps;
  const DiscImages di = sw_disc_images_for(w, Tp);
  ad.img = const_cast<float*>(di.img);
  ad.tab = di.tab;
  return ad;
}

// Can sw_disc_update run this pass (else: sw_disc_fwd + sw_disc_bwd_gan*)?  Built in round 3 for the shapes that leave CUs
// idle (<= 128 tiles); measured in round 4 at 160 .. 2 048 tiles: one workgroup per CU without the round trip of the gates
// through the save buffer beats the two launches at two workgroups per CU by 1-5 % of the step everywhere.
extern "C" int sw_disc_update_supported(const float* d_w, int B, int To, int Tp) {
  if (!d_w || B < 1 || To < 1 || Tp < 1 || Tp > 12) return 0;
  if (!sw_disc_images_for(d_w, Tp).img) return 0;
  return upd_lds(Tp).total * 4 <= 163840 ? 1 : 0;
}
// One discriminator update pass (train.py:476-495) in ONE launch + its weight-gradient GEMM (+ the Adam update when
// adam_w = d_w): what sw_disc_fwd(nb = 2, x_mode 0, save_lstm 1 | 2) followed by sw_disc_bwd_gan[_adam] computes, to the
// same buffers.  obs_pre = 1: the observation-LSTM rows are already in dsave (sw_dec_rollout_fwd_aux).  Requires
// sw_disc_update_supported() (SW_ESHAPE otherwise).
// sw_disc_update and sw_disc_update_ragged: one set of checks, one grid rule; the dense entry launches the dense instance
static int disc_update_launch(bool ragged, const float* obsv, int To, const int* obs_len, const float* const* pred4, const float* d_w,
                              int B, int Tp, float* const* label, float* const* code, float* dsave, int obs_pre, float* w_snapshot,
                              const float* targets, int t0, int t1, const float* z, float g_label, float g_code, float* ddelta,
                              float* d_d_w, float* wgrad_ws, float* loss_part, float* adam_w, float* adam_m, float* adam_v,
                              const float* adam_step, double lr, double beta1, double beta2, double eps, void* stream) {
  if (!obsv || !pred4 || !pred4[0] || !pred4[1] || !d_w || !label || !label[0] || !label[1] || !code || !code[0] || !code[1] ||
      !dsave || !targets || !z || !ddelta || !d_d_w || !wgrad_ws || t0 < 0 || t1 < 0 || To < 2)
    return SW_EARG;
  if (ragged && !obs_len) return SW_EARG;
  if (adam_w && (!adam_m || !adam_v || !adam_step || adam_w != d_w)) return SW_EARG;
  if (B == 0) return SW_OK;
  if (!sw_disc_update_supported(d_w, B, To, Tp)) return SW_ESHAPE;
  const int lds = upd_lds(Tp).total * 4;
  static int have = 0, have_ragged = 0;
  if (int rc = ragged ? sw_set_lds((const void*)disc_update_kernel<true>, lds, have_ragged)
                      : sw_set_lds((const void*)disc_update_kernel<false>, lds, have))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const DiscImages di = sw_disc_images_for(d_w, Tp);
  DiscLoss gl{targets, z, t0, t1, g_label, g_code, 1, loss_part};
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  WgBatch wb;
  if (int rc = disc_wgrad_problems(wb, dsave, ddelta, 2, B, To, Tp, d_d_w)) return rc;
  // (both instances are timed as "disc_update_kernel": SW_LAUNCH_AS)
  if (ragged)
    SW_LAUNCH_AS("disc_update_kernel", disc_update_kernel<true>, dim3(tiles), dim3(SW_THREADS), lds, st, obsv, To, pred4[0], pred4[1],
                 d_w, B, Tp, label[0], label[1], code[0], code[1], dsave, 0, w_snapshot, gl, ddelta, di.img, obs_len);
  else
    SW_LAUNCH_AS("disc_update_kernel", disc_update_kernel<false>, dim3(tiles), dim3(SW_THREADS), lds, st, obsv, To, pred4[0], pred4[1],
                 d_w, B, Tp, label[0], label[1], code[0], code[1], dsave, obs_pre ? 1 : 0, w_snapshot, gl, ddelta, di.img,
                 (const int*)nullptr);
  SW_CHECK_LAUNCH("disc_update_kernel");
  WgAdam ad = disc_adam(adam_w, adam_m, adam_v, adam_step, d_d_w, lr, beta1, beta2, eps, Tp);
  return wg_launch_adam(wb, wgrad_ws, ad, st);
}
extern "C" int sw_disc_update(const float* obsv, int To, const float* const* pred4, const float* d_w, int B, int Tp,
                              float* const* label, float* const* code, float* dsave, int obs_pre, float* w_snapshot,
                              const float* targets, int t0, int t1, const float* z, float g_label, float g_code, float* ddelta,
                              float* d_d_w, float* wgrad_ws, float* loss_part, float* adam_w, float* adam_m, float* adam_v,
                              const float* adam_step, double lr, double beta1, double beta2, double eps, void* stream) {
  return disc_update_launch(false, obsv, To, nullptr, pred4, d_w, B, Tp, label, code, dsave, obs_pre, w_snapshot, targets, t0, t1, z,
                            g_label, g_code, ddelta, d_d_w, wgrad_ws, loss_part, adam_w, adam_m, adam_v, adam_step, lr, beta1, beta2,
                            eps, stream);
}
// ... over RAGGED observation histories: what sw_disc_fwd_ragged(nb = 2, x_mode 0, save_lstm 1) followed by
// sw_disc_bwd_gan[_adam] computes, to the same buffers, bit for bit.  Row b holds clamp(obs_len[b], 2, To) valid frames
// right-aligned in obsv.  sw_disc_update's arguments without obs_pre: ragged rows have no precomputed observation pass.
extern "C" int sw_disc_update_ragged(const float* obsv, int To, const int* obs_len, const float* const* pred4, const float* d_w, int B,
                                     int Tp, float* const* label, float* const* code, float* dsave, float* w_snapshot,
                                     const float* targets, int t0, int t1, const float* z, float g_label, float g_code,
                                     float* ddelta, float* d_d_w, float* wgrad_ws, float* loss_part, float* adam_w, float* adam_m,
                                     float* adam_v, const float* adam_step, double lr, double beta1, double beta2, double eps,
                                     void* stream) {
  return disc_update_launch(true, obsv, To, obs_len, pred4, d_w, B, Tp, label, code, dsave, 0, w_snapshot, targets, t0, t1, z, g_label,
                            g_code, ddelta, d_d_w, wgrad_ws, loss_part, adam_w, adam_m, adam_v, adam_step, lr, beta1, beta2, eps, stream);
}

extern "C" int sw_disc_bwd(const float* d_w, const float* dsave, const float* const* dlabel,
                           const float* const* dcode, int nb, int B, int To, int Tp, float* ddelta, float* d_d_w,
                           float* const* dpred4, float* wgrad_ws, void* stream) {
  DiscLoss gl{};
  gl.on = 0;
  gl.loss_part = nullptr;
  return disc_bwd_impl(d_w, dsave, dlabel, dcode, nb, B, To, Tp, ddelta, d_d_w, dpred4, wgrad_ws, stream, gl);
}

extern "C" int sw_disc_bwd_gan_adam(const float* d_w, const float* dsave, const float* const* label,
                                    const float* const* code, const float* targets, int t0, int t1, const float* z,
                                    float g_label, float g_code, int nb, int B, int To, int Tp, float* ddelta,
                                    float* d_d_w, float* const* dpred4, float* wgrad_ws, float* loss_part,
                                    float* adam_w, float* adam_m, float* adam_v, const float* adam_step, double lr,
                                    double beta1, double beta2, double eps, void* stream) {
  if (!targets || !z || t0 < 0 || t1 < 0) return SW_EARG;
  if (adam_w && (!adam_m || !adam_v || !adam_step || !d_d_w || adam_w != d_w)) return SW_EARG;
  DiscLoss gl{targets, z, t0, t1, g_label, g_code, 1, loss_part};
  const WgAdam ad = disc_adam(adam_w, adam_m, adam_v, adam_step, d_d_w, lr, beta1, beta2, eps, Tp);
  return disc_bwd_impl(d_w, dsave, label, code, nb, B, To, Tp, ddelta, d_d_w, dpred4, wgrad_ws, stream, gl, ad);
}
extern "C" int sw_disc_bwd_gan(const float* d_w, const float* dsave, const float* const* label,
                               const float* const* code, const float* targets, int t0, int t1, const float* z,
                               float g_label, float g_code, int nb, int B, int To, int Tp, float* ddelta,
                               float* d_d_w, float* const* dpred4, float* wgrad_ws, float* loss_part, void* stream) {
  return sw_disc_bwd_gan_adam(d_w, dsave, label, code, targets, t0, t1, z, g_label, g_code, nb, B, To, Tp, ddelta, d_d_w,
                              dpred4, wgrad_ws, loss_part, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, stream);
}

// ---- derived images of the discriminator's weights (swdimg, sw_common.h) --------------------------------------------
extern "C" int sw_disc_image_floats(int Tp) {
  if (Tp < 1 || Tp > 64) return SW_EARG;
  return swdimg::HEADT + head_lds_b(Tp, 0).dlab;
}
// tab[2 i], tab[2 i + 1] = image offsets of packed float i (or -1); host memory, sw_param_count(SW_GRP_DISC, Tp) pairs
extern "C" int sw_disc_image_table(int Tp, int* tab) {
  if (Tp < 1 || Tp > 64 || !tab) return SW_EARG;
  const swp::Disc O = swp::disc(Tp);
  const HeadLdsB L = head_lds_b(Tp, 0);
  for (int i = 0; i < 2 * O.n; ++i) tab[i] = -1;
  for (int R = 0; R < 256; ++R)
    for (int C = 0; C < 64; ++C) {
      const int i = O.whh + R * 64 + C;
      tab[2 * i] = sw_op_at(swdimg::OP_WHH, R, C);
      tab[2 * i + 1] = sw_op_at(swdimg::OP_WHHT, C, R);
    }
  auto head = [&](int w_off, int M, int K, int img_off, int ld) {   // XT[c][r] = X[r][c]
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < K; ++c) tab[2 * (w_off + r * K + c)] = swdimg::HEADT + img_off + c * ld + r;
  };
  head(O.of0w, 32, 64, L.of0T, LD32);
  head(O.of1w, 32, 32, L.of1T, LD32);
  head(O.pe0w, 32, 4 * Tp, L.pe0T, LD32);
  head(O.pe1w, 32, 32, L.pe1T, LD32);
  head(O.cl0w, 32, 64, L.cl0T, LD32);
  head(O.la0w, 32, 64, L.la0T, LD32);
  head(O.cl1w, 1, 32, L.cl1T, LD16);
  head(O.la1w, 2, 32, L.la1T, LD16);
  return SW_OK;
}
static thread_local const float* g_dimg_w = nullptr;     // per host thread, like the generator's registration (sw_misc.hip)
static thread_local DiscImages g_dimg;
static thread_local int g_dimg_tp = 0;
DiscImages sw_disc_images_for(const float* d_w, int Tp) {
  return (g_dimg.img && d_w == g_dimg_w && Tp == g_dimg_tp) ? g_dimg : DiscImages();
}
void sw_disc_images_register(const float* d_w, const float* img, const int* tab, int Tp) {
  g_dimg_w = d_w; g_dimg.img = img; g_dimg.tab = tab; g_dimg_tp = Tp;
}
__global__ __launch_bounds__(256) void disc_images_kernel(const float* __restrict__ d_w, float* __restrict__ img,
                                                           const int* __restrict__ tab, int n) {
  disc_images_scatter(d_w, img, tab, n, blockIdx.x, gridDim.x);
}
// Scatter the packed weights d_w into img (sw_disc_image_floats(Tp) floats, ZERO-FILLED by the caller once: padding is
// never written) through the device copy `tab` of sw_disc_image_table(Tp), and register the images for d_w: until the
// registration is dropped - sw_disc_images(NULL, NULL, NULL, 0, NULL) - sw_disc_fwd / sw_disc_dpred / sw_disc_bwd* called with
// these weights read the images, and sw_disc_bwd_gan_adam keeps them current while it updates the weights.  Whoever
// changes the weights by other means re-scatters or drops the registration.
extern "C" int sw_disc_images(const float* d_w, float* img, const int* tab, int Tp, void* stream) {
  if (!img) {
    sw_disc_images_register(nullptr, nullptr, nullptr, 0);
    return SW_OK;
  }
  if (!d_w || !tab || Tp < 1 || Tp > 64) return SW_EARG;
  SW_LAUNCH(disc_images_kernel, dim3(16), dim3(256), 0, (hipStream_t)stream, d_w, img, tab, swp::disc(Tp).n);
  SW_CHECK_LAUNCH("disc_images_kernel");
  sw_disc_images_register(d_w, img, tab, Tp);
  return SW_OK;
}
