// sw_lstm.hip - EncoderLstm over a whole sequence (reference train.py:245-269 as used by
// predict() train.py:397-404) and its BPTT.  One workgroup per 16-agent tile, 4 waves, W_hh in
// registers, h exchanged through a double-buffered 4 KB LDS tile: one barrier per time step.
#include "../../include/socialways_hip.h"
#include "sw_lstm_dev.h"
#include <cstdlib>

// XMODE 0: x = positions [B][T][2] (4-d state formed on the fly); 1: x = [B][T][4].  ACT / Y / X4S: which per-step
// rows are stored.  RAGGED (sw_enc_lstm_fwd_ragged*): row b runs its last obs_len[b] steps from the zero state (obs_len
// the LAST argument, as in disc_score_kernel; those launches pass no h0 / c0 / y and add no z-pull workgroups).  All of
// them are template parameters so that the step loop (lstm_obs_loop, sw_lstm_dev.h) has NO conditional memory operation.
template <int XMODE, bool ACT, bool Y, bool X4S, bool RAGGED>
__global__ __launch_bounds__(SW_THREADS) void enc_lstm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ enc_w, const float* __restrict__ h0,
    const float* __restrict__ c0, int B, int T, float* __restrict__ hT, float* __restrict__ cT,
    float* __restrict__ y, float* __restrict__ act, float* __restrict__ x4s, int t0, const float* __restrict__ aux_src,
    float* __restrict__ aux_dst, long long aux_n, const float* __restrict__ gimg, const int* __restrict__ obs_len) {
  // The FIRST workgroups of the grid only copy aux_src -> aux_dst (the training step pulls z out of its pinned host slot
  // here).  128 tiles leave half of the CUs idle for the whole latency-bound kernel: the PCIe read is free.  With more
  // tiles than CUs (dense crowds: 4 MB of z) the copy must START with the kernel - workgroups are dispatched in index
  // order; appended behind the tiles (round 3) they began when the last round of tiles did and the 4 MB then took
  // longer than that round: 113 -> 173 us - and keep several reads per thread in flight (PCIe round trips).
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  const int extra = RAGGED ? 0 : (int)gridDim.x - tiles;   // (the ragged launches: tiles only, zero initial state)
  if ((int)blockIdx.x < extra) {
    sw_z_pull<SW_THREADS, 4>(aux_src, aux_dst, aux_n, extra);
    return;
  }
  // h exchange between the waves: with ACT the whole saved row of a step is assembled in LDS (lstm_put_act_tile) and its
  // h columns are the next step's B operand; without, a plain [16][68] h tile
  constexpr int HS = ACT ? SW_ALD : SW_HLD, HO = ACT ? 320 : 0;
  __shared__ __attribute__((aligned(16))) float hbuf[2][SW_TILE * HS];
  __shared__ __attribute__((aligned(16))) float wx_lds[256 * 4];
  __shared__ __attribute__((aligned(16))) float bx_lds[256];
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int u0 = wave * 16;
  const int a0 = ((int)blockIdx.x - extra) * SW_TILE;
  const int b = min(a0 + ln, B - 1);
  LstmW W;
  lstm_load_enc(W, gimg, enc_w, wx_lds, bx_lds, wave, lane);
  const int s = RAGGED ? obs_start(obs_len, b, T, XMODE) : 0;
  // initial state
  f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};
  if (!RAGGED && h0) h = ld4(h0 + (size_t)b * 64 + u0 + 4 * lg);
  if (!RAGGED && c0) c = ld4(c0 + (size_t)b * 64 + u0 + 4 * lg);
  st4(&hbuf[0][ln * HS + HO + u0 + 4 * lg], h);
  sw_barrier();
  if (!gimg) lstm_load_wx(W, wx_lds, bx_lds, u0, ln, lg);

  float* yrow = Y ? y + (size_t)b * T * 64 + u0 + 4 * lg : nullptr;
  lstm_obs_loop<XMODE, ACT ? SAVE_TILE : SAVE_NONE, RAGGED, X4S>(
      W, hbuf[0], x, T, B, b, s, h0 != nullptr, c, h, act, x4s, a0, t0, [&](const f32x4& hn) {
        if constexpr (Y) {
          st4(yrow, hn);
          yrow += 64;
        }
      });
  st4(hT + (size_t)b * 64 + u0 + 4 * lg, h);
  st4(cT + (size_t)b * 64 + u0 + 4 * lg, c);
}

// ---- round-5 pilot: the same kernel on EIGHT waves (two per SIMD), weights split 8 ways -----------------------------
// The r4 verdict's lever for the register-resident serial kernels.  Wave w owns hidden units 8w .. 8w+7 of all four gates
// as two row tiles (swimg::OP_WHH8: a lane's result registers hold i, f | g, o of the same two units, so the cell update
// stays lane-local): 34 instead of 68 matrix instructions per wave and step, 32 instead of 64 weight registers, the saved
// row assembled in the same LDS tile.  Training-step instance only (positions in, saved rows + inputs out, weight images
// registered); selected by SW_ENC8=1.  Measured against the 4-wave kernel in DESIGN section 9 (round 5).
__global__ __launch_bounds__(512) void enc_lstm_fwd8_kernel(
    const float* __restrict__ x, const float* __restrict__ h0, const float* __restrict__ c0, int B, int T,
    float* __restrict__ hT, float* __restrict__ cT, float* __restrict__ act, float* __restrict__ x4s, int t0,
    const float* __restrict__ aux_src, float* __restrict__ aux_dst, long long aux_n, const float* __restrict__ gimg) {
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  const int extra = (int)gridDim.x - tiles;
  if ((int)blockIdx.x < extra) {      // z's pull out of the pinned slot, as in enc_lstm_fwd_kernel
    sw_z_pull<512, 2>(aux_src, aux_dst, aux_n, extra);
    return;
  }
  __shared__ __attribute__((aligned(16))) float hbuf[2][SW_TILE * SW_ALD];
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int ub = 8 * wave + 2 * lg;                 // this lane's two units (result rows 4 lg + r: gate r >> 1, unit ub + (r & 1))
  const int a0 = ((int)blockIdx.x - extra) * SW_TILE;
  const int b = min(a0 + ln, B - 1);
  f32x4 whh[2][4], bias[2];
  float wx[2];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
#pragma unroll
    for (int j = 0; j < 4; ++j) whh[tl][j] = SW_OP_LD(gimg, swimg::OP_WHH8, (size_t)wave * 2 + tl, j, lane);
    const int rowA = (2 * tl + ((ln & 3) >> 1)) * 64 + 8 * wave + 2 * (ln >> 2) + (ln & 1);   // A row of lane ln
    wx[tl] = gimg[swimg::WX + rowA * 4 + lg];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[tl][r] = gimg[swimg::BX + (2 * tl + (r >> 1)) * 64 + ub + (r & 1)];
  }
  float2 c = {0.f, 0.f}, h = {0.f, 0.f};
  if (h0) h = *reinterpret_cast<const float2*>(h0 + (size_t)b * 64 + ub);
  if (c0) c = *reinterpret_cast<const float2*>(c0 + (size_t)b * 64 + ub);
  *reinterpret_cast<float2*>(&hbuf[0][ln * SW_ALD + 320 + ub]) = h;
  sw_barrier();
  float xa, xq = 0.f;
  obs_x4_load(x, b, 0, T, lg, xa, xq);
  asm volatile("" : "+v"(xa), "+v"(xq));
  float* xrow = x4s + ((size_t)t0 * B + b) * 4 + lg;
  auto step = [&](int t, auto hp) {
    const float xb = xa - (lg >= 2 ? xq : 0.f);
    obs_x4_load(x, b, min(t + 1, T - 1), T, lg, xa, xq);
    f32x4 acc0 = SW_MFMA(wx[0], xb, bias[0]), acc1 = SW_MFMA(wx[1], xb, bias[1]);
    if constexpr (decltype(hp)::value) {     // (false: the step starts from h = 0 - neither the h tile nor W_hh is touched)
      const float* hrow = &hbuf[t & 1][ln * SW_ALD + 320 + 4 * lg];
      f32x4 bq[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bq[j] = ld4(hrow + 16 * j);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc0 = SW_MFMA(whh[0][j][r], bq[j][r], acc0);
          acc1 = SW_MFMA(whh[1][j][r], bq[j][r], acc1);
        }
    }
    float2 gi, gf, gg, go;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float i_ = sw_sigmoid(acc0[e]), f_ = sw_sigmoid(acc0[2 + e]), g_ = sw_tanh(acc1[e]), o_ = sw_sigmoid(acc1[2 + e]);
      const float cp = e ? c.y : c.x;
      const float cn = fmaf(f_, cp, i_ * g_);
      const float hn = o_ * sw_tanh(cn);
      if (e) { gi.y = i_; gf.y = f_; gg.y = g_; go.y = o_; c.y = cn; h.y = hn; }
      else   { gi.x = i_; gf.x = f_; gg.x = g_; go.x = o_; c.x = cn; h.x = hn; }
    }
    float* row = &hbuf[(t + 1) & 1][ln * SW_ALD + ub];
    *reinterpret_cast<float2*>(row) = gi;
    *reinterpret_cast<float2*>(row + 64) = gf;
    *reinterpret_cast<float2*>(row + 128) = gg;
    *reinterpret_cast<float2*>(row + 192) = go;
    *reinterpret_cast<float2*>(row + 256) = c;
    *reinterpret_cast<float2*>(row + 320) = h;
    *xrow = xb;
    xrow += (size_t)B * 4;
    sw_barrier();
    {   // the saved rows of the step: 16 agents x 96 float4, three per thread, 1 KB of consecutive memory per wave instruction
      float* rows_t = act + (size_t)(t0 + t) * B * 384;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int f = k * 512 + (int)threadIdx.x, a = f / 96, c4 = f - a * 96;
        const f32x4 v = ld4(&hbuf[(t + 1) & 1][a * SW_ALD + 4 * c4]);
        st4g(rows_t + (size_t)min(a0 + a, B - 1) * 384 + 4 * c4, v);
      }
    }
    asm volatile("" : "+v"(xa), "+v"(xq));
  };
  if (h0) step(0, std::true_type{});       // step 0 peeled, as in enc_lstm_fwd_kernel
  else step(0, std::false_type{});
  for (int t = 1; t < T; ++t) step(t, std::true_type{});
  *reinterpret_cast<float2*>(hT + (size_t)b * 64 + ub) = h;
  *reinterpret_cast<float2*>(cT + (size_t)b * 64 + ub) = c;
}

// BPTT over the saved rows (lstm_bptt_rows, sw_lstm_dev.h): dy (DY, a template parameter: no conditional load in the
// loop) joins dh in front of every step's cell backward.
template <bool DY>
__global__ __launch_bounds__(SW_THREADS) void enc_lstm_bwd_kernel(
    const float* __restrict__ whh, const float* __restrict__ act, const float* __restrict__ c0,
    const float* __restrict__ dhT, const float* __restrict__ dcT, const float* __restrict__ dy, int B, int T,
    int t0, float* __restrict__ dgates, float* __restrict__ dh0, float* __restrict__ dc0, const float* __restrict__ gimg,
    const float* __restrict__ aux_src, float* __restrict__ aux_dst, const float* __restrict__ aux_mask, long long aux_n) {
  // (the masked copy of the training step's D.load(backup) when the decode BPTT launch - its usual place - reads D's weights)
  if (sw_aux_masked_copy(B, aux_src, aux_dst, aux_mask, aux_n)) return;
  __shared__ __attribute__((aligned(16))) float dgbuf[2][SW_TILE * SW_GLD];
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int u0 = wave * 16;
  const int a0 = blockIdx.x * SW_TILE;
  const int b = min(a0 + ln, B - 1);
  LstmWT W;
  lstm_load_whhT(W, gimg, swimg::OP_WHHT, whh, wave, lane);   // W_hh^T of this step (operand-layout image when there is one)
  // optional inputs are read unconditionally from a selected address (a load under a branch costs the exact vmcnt
  // bookkeeping of everything behind it) and zeroed afterwards
  const float* act_b = act + ((size_t)t0 * B + b) * 384 + u0 + 4 * lg;
  f32x4 dh = ld4(dhT ? dhT + (size_t)b * 64 + u0 + 4 * lg : act_b);
  f32x4 dc = ld4(dcT ? dcT + (size_t)b * 64 + u0 + 4 * lg : act_b);
  if (!dhT) dh = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!dcT) dc = f32x4{0.f, 0.f, 0.f, 0.f};
  // c_{-1} of the sequence start: the row in front of t0, c0 or zero
  const float* cstart = t0 > 0 ? act_b - (size_t)B * 384 + 256 : c0 ? c0 + (size_t)b * 64 + u0 + 4 * lg : nullptr;
  const LstmBptt S{act_b, cstart, dgbuf[0], dgates + ((size_t)t0 * B + a0) * 256, nullptr, a0, B};
  const float* dyp = DY ? dy + ((size_t)b * T + T - 1) * 64 + u0 + 4 * lg : nullptr;
  lstm_bptt_rows<true>(W, S, T, dh, dc, [&](f32x4& d) {
    if constexpr (DY) {
      d += ld4(dyp);
      dyp -= 64;
    }
  });
  if (dh0) st4(dh0 + (size_t)b * 64 + u0 + 4 * lg, dh);
  if (dc0) st4(dc0 + (size_t)b * 64 + u0 + 4 * lg, dc);
}

// get_traj_4d (train.py:130-138) as a standalone op for the module-level API.
__global__ void traj4d_kernel(const float* __restrict__ obsv, const float* __restrict__ pred, int B, int To,
                              int Tp, float* __restrict__ o4, float* __restrict__ p4) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int n_o = B * To, n_p = pred ? B * Tp : 0;
  if (i < n_o) {
    int b = i / To, t = i - b * To;
    f32x4 v;
    v[0] = obs_x4(obsv, b, t, To, 0);
    v[1] = obs_x4(obsv, b, t, To, 1);
    v[2] = obs_x4(obsv, b, t, To, 2);
    v[3] = obs_x4(obsv, b, t, To, 3);
    st4(o4 + (size_t)i * 4, v);
  } else if (i < n_o + n_p) {
    int k = i - n_o, b = k / Tp, t = k - b * Tp;
    const float* p = pred + ((size_t)b * Tp + t) * 2;
    const float* q = t == 0 ? obsv + ((size_t)b * To + To - 1) * 2 : p - 2;
    f32x4 v = {p[0], p[1], p[0] - q[0], p[1] - q[1]};
    st4(p4 + (size_t)k * 4, v);
  }
}

extern "C" int sw_traj_4d(const float* obsv, const float* pred, int B, int To, int Tp, float* obsv4,
                          float* pred4, void* stream) {
  if (!obsv || !obsv4 || B < 0 || To < 2 || (pred && (!pred4 || Tp < 1))) return SW_EARG;
  if (B == 0) return SW_OK;
  int n = B * To + (pred ? B * Tp : 0);
  SW_LAUNCH(traj4d_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, obsv, pred, B,
                     To, Tp, obsv4, pred4);
  SW_CHECK_LAUNCH("traj4d_kernel");
  return SW_OK;
}

// The instance of enc_lstm_fwd_kernel for what is asked for, launched on tiles + extra workgroups under the name it is
// timed as (SW_LAUNCH_AS).  The ragged entry points reach four instances: x_mode x (nothing saved | act + x4s).
static int enc_fwd_launch(const char* name, const float* x, int x_mode, const float* enc_w, const float* h0, const float* c0, int B,
                          int T, float* hT, float* cT, float* y, float* act, float* x4s, int t0, const float* aux_src,
                          float* aux_dst, long long aux_n, int extra, const float* gimg, bool ragged, const int* obs_len,
                          void* stream) {
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
#define SW_ENC_FWD(XM, A, Y_, X4, RG)                                                                                    \
  SW_LAUNCH_AS(name, (enc_lstm_fwd_kernel<XM, A, Y_, X4, RG>), dim3(tiles + extra), dim3(SW_THREADS), 0, (hipStream_t)stream, \
               x, enc_w, h0, c0, B, T, hT, cT, y, act, x4s, t0, aux_src, aux_dst, aux_n, gimg, obs_len)
  switch ((ragged ? 16 : 0) | (x_mode ? 8 : 0) | (act ? 4 : 0) | (y ? 2 : 0) | (x4s ? 1 : 0)) {
    case 0: SW_ENC_FWD(0, false, false, false, false); break;
    case 1: SW_ENC_FWD(0, false, false, true, false); break;
    case 2: SW_ENC_FWD(0, false, true, false, false); break;
    case 3: SW_ENC_FWD(0, false, true, true, false); break;
    case 4: SW_ENC_FWD(0, true, false, false, false); break;
    case 5: SW_ENC_FWD(0, true, false, true, false); break;
    case 6: SW_ENC_FWD(0, true, true, false, false); break;
    case 7: SW_ENC_FWD(0, true, true, true, false); break;
    case 8: SW_ENC_FWD(1, false, false, false, false); break;
    case 9: SW_ENC_FWD(1, false, false, true, false); break;
    case 10: SW_ENC_FWD(1, false, true, false, false); break;
    case 11: SW_ENC_FWD(1, false, true, true, false); break;
    case 12: SW_ENC_FWD(1, true, false, false, false); break;
    case 13: SW_ENC_FWD(1, true, false, true, false); break;
    case 14: SW_ENC_FWD(1, true, true, false, false); break;
    case 15: SW_ENC_FWD(1, true, true, true, false); break;
    case 16: SW_ENC_FWD(0, false, false, false, true); break;
    case 16 + 5: SW_ENC_FWD(0, true, false, true, true); break;
    case 16 + 8: SW_ENC_FWD(1, false, false, false, true); break;
    case 16 + 13: SW_ENC_FWD(1, true, false, true, true); break;
    default: return SW_EARG;   // (not reached: the ragged entry points check their outputs)
  }
#undef SW_ENC_FWD
  SW_CHECK_LAUNCH(name);
  return SW_OK;
}

extern "C" int sw_enc_lstm_fwd_aux(const float* x, int x_mode, const float* enc_w, const float* h0,
                                   const float* c0, int B, int T, float* hT, float* cT, float* y, float* act,
                                   float* x4s, int t0, const float* aux_src, float* aux_dst, long long aux_n,
                                   void* stream) {
  if (!x || !enc_w || !hT || !cT || B < 0 || T < 1 || t0 < 0 || (x_mode != 0 && x_mode != 1)) return SW_EARG;
  if (aux_n < 0 || (aux_n & 3) || (aux_n > 0 && (!aux_src || !aux_dst))) return SW_EARG;
  if (x_mode == 0 && T < 2) return SW_ESHAPE;  // the observation velocity rule needs 2 points
  if (B == 0) return SW_OK;
  const float* gimg = sw_gen_images_for(enc_w, nullptr);
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  int extra = aux_n > 0 ? (int)((aux_n / 4 + SW_THREADS - 1) / SW_THREADS) : 0;
  if (extra > 64) extra = 64;
  // the 8-wave kernel (bit-identical results): per step -7.5 % when every tile has a CU to itself (m1: 1.67 -> 1.54 us per
  // step), +3.5 % once tiles queue for CUs (c4) - used up to one tile per CU; SW_ENC8=0 / 1 forces either kernel
  static const int enc8_env = getenv("SW_ENC8") ? atoi(getenv("SW_ENC8")) : -1;
  const bool enc8 = enc8_env >= 0 ? enc8_env != 0 : tiles <= 256;
  if (enc8 && gimg && x_mode == 0 && act && x4s && !y) {
    SW_LAUNCH(enc_lstm_fwd8_kernel, dim3(tiles + extra), dim3(512), 0, (hipStream_t)stream, x, h0, c0, B, T, hT, cT, act, x4s, t0,
              aux_src, aux_dst, aux_n, gimg);
    SW_CHECK_LAUNCH("enc_lstm_fwd8_kernel");
    return SW_OK;
  }
  return enc_fwd_launch("enc_lstm_fwd_kernel", x, x_mode, enc_w, h0, c0, B, T, hT, cT, y, act, x4s, t0, aux_src, aux_dst, aux_n,
                        extra, gimg, false, nullptr, stream);
}
extern "C" int sw_enc_lstm_fwd(const float* x, int x_mode, const float* enc_w, const float* h0,
                               const float* c0, int B, int T, float* hT, float* cT, float* y, float* act,
                               float* x4s, int t0, void* stream) {
  return sw_enc_lstm_fwd_aux(x, x_mode, enc_w, h0, c0, B, T, hT, cT, y, act, x4s, t0, nullptr, nullptr, 0, stream);
}

// Ragged observation histories: row b runs its last obs_len[b] steps (lstm_obs_loop<., ., true>, sw_lstm_dev.h) - the RAGGED
// instances of enc_lstm_fwd_kernel from the zero state, on a grid of tiles only (no z pull: the ragged step copies z itself).
// The inference form saves nothing ...
extern "C" int sw_enc_lstm_fwd_ragged(const float* x, int x_mode, const float* enc_w, const int* obs_len, int B, int T,
                                      float* hT, float* cT, void* stream) {
  if (!x || !enc_w || !hT || !cT || B < 0 || T < 1 || (x_mode != 0 && x_mode != 1) || (x_mode == 0 && T < 2)) return SW_EARG;
  if (B == 0) return SW_OK;
  return enc_fwd_launch("enc_lstm_fwd_ragged_kernel", x, x_mode, enc_w, nullptr, nullptr, B, T, hT, cT, nullptr, nullptr, nullptr,
                        0, nullptr, nullptr, 0, 0, sw_gen_images_for(enc_w, nullptr), true, obs_len, stream);
}
// ... the training form the saved rows + inputs of enc_lstm_fwd_kernel<., true, false, true> at t0 = 0, zeros in front of a
// row's start.
extern "C" int sw_enc_lstm_fwd_ragged_save(const float* x, int x_mode, const float* enc_w, const int* obs_len, int B, int T,
                                           float* hT, float* cT, float* act, float* x4s, void* stream) {
  if (!x || !enc_w || !hT || !cT || !act || !x4s || B < 0 || T < 1 || (x_mode != 0 && x_mode != 1) || (x_mode == 0 && T < 2))
    return SW_EARG;
  if (B == 0) return SW_OK;
  return enc_fwd_launch("enc_lstm_fwd_ragged_save_kernel", x, x_mode, enc_w, nullptr, nullptr, B, T, hT, cT, nullptr, act, x4s,
                        0, nullptr, nullptr, 0, 0, sw_gen_images_for(enc_w, nullptr), true, obs_len, stream);
}

extern "C" int sw_enc_lstm_bwd_aux(const float* enc_w, const float* act, const float* c0, const float* dhT,
                                   const float* dcT, const float* dy, int B, int T, int t0, float* dgates,
                                   float* dh0, float* dc0, const float* aux_src, float* aux_dst, const float* aux_mask,
                                   long long aux_n, void* stream) {
  if (!enc_w || !act || !dgates || B < 0 || T < 1 || t0 < 0) return SW_EARG;
  if (aux_n < 0 || (aux_n > 0 && (!aux_src || !aux_dst || !aux_mask))) return SW_EARG;
  if (B == 0) return SW_OK;
  const float* gimg = sw_gen_images_for(enc_w, nullptr);
  const int tiles = (B + SW_TILE - 1) / SW_TILE;
  int extra = aux_n > 0 ? (int)((aux_n + SW_THREADS - 1) / SW_THREADS) : 0;
  if (extra > 64) extra = 64;
  if (dy)
    SW_LAUNCH(enc_lstm_bwd_kernel<true>, dim3(tiles + extra), dim3(SW_THREADS), 0, (hipStream_t)stream, enc_w + swp::ENC_WHH, act, c0,
              dhT, dcT, dy, B, T, t0, dgates, dh0, dc0, gimg, aux_src, aux_dst, aux_mask, aux_n);
  else
    SW_LAUNCH(enc_lstm_bwd_kernel<false>, dim3(tiles + extra), dim3(SW_THREADS), 0, (hipStream_t)stream, enc_w + swp::ENC_WHH, act, c0,
              dhT, dcT, dy, B, T, t0, dgates, dh0, dc0, gimg, aux_src, aux_dst, aux_mask, aux_n);
  SW_CHECK_LAUNCH("enc_lstm_bwd_kernel");
  return SW_OK;
}
extern "C" int sw_enc_lstm_bwd(const float* enc_w, const float* act, const float* c0, const float* dhT,
                               const float* dcT, const float* dy, int B, int T, int t0, float* dgates,
                               float* dh0, float* dc0, void* stream) {
  return sw_enc_lstm_bwd_aux(enc_w, act, c0, dhT, dcT, dy, B, T, t0, dgates, dh0, dc0, nullptr, nullptr, nullptr, 0, stream);
}
