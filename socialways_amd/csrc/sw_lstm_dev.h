// sw_lstm_dev.h - the time-unrolled LSTM cell shared by the encoder, decode-loop and
// discriminator kernels (reference: nn.LSTM in EncoderLstm train.py:254,268 and Discriminator
// train.py:278,299; gate order i,f,g,o, c' = f c + i g, h' = o tanh(c')).
//
// A workgroup = 4 waves owns a tile of 16 agents.  Wave w owns hidden units [16w, 16w+16) of all
// four gates, so the cell update is lane-local.  W_hh lives in registers for the whole kernel
// (64 VGPRs/lane); the 4-d input goes through a 256x4 input matrix Wx which for the encoder is
// the composition W_ih * W_embed (no non-linearity sits between embed and the LSTM,
// train.py:266-268), for the discriminator W_ih itself.
#pragma once
#include <type_traits>
#include "sw_common.h"

#define SW_HLD 68    // LDS row stride of a 64-wide h tile
#define SW_GLD 260   // LDS row stride of a 256-wide dgates tile

struct LstmW {
  f32x4 whh[4][4];  // [gate][j] = Whh[gate*64 + u0 + ln][16j + 4lg .. +3]
  float wx[4];      // Wx[gate*64 + u0 + ln][lg]
  f32x4 bias[4];    // rows gate*64 + u0 + 4lg + r
};

// Cooperative prologue: every thread computes one row of the input matrix / bias into LDS
// (wx_lds[256][4], bx_lds[256]); caller must __syncthreads() afterwards.
//   composed (encoder): Wx = Wih * We, bx = Wih * be + bih + bhh
//   direct (discriminator): Wx = Wih (256x4), bx = bih + bhh
__device__ __forceinline__ void lstm_prep_rows(const float* We, const float* be, const float* Wih,
                                               const float* bih, const float* bhh, bool composed,
                                               float* wx_lds, float* bx_lds) {
  int row = threadIdx.x;  // 256 threads = 256 gate rows
  if (composed) {
    // the whole W_ih row first (16 independent float4 loads: ONE L2 round trip, not one per k-step),
    // W_embed / b_embed are tiny and L1-resident after the first touch
    f32x4 w[16];
    const float* wr = Wih + (size_t)row * 64;
#pragma unroll
    for (int e = 0; e < 16; ++e) w[e] = ld4(wr + 4 * e);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, ab = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      f32x4 bq = ld4(be + 4 * e);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 em = ld4(We + (4 * e + q) * 4);
        a0 = fmaf(w[e][q], em[0], a0);
        a1 = fmaf(w[e][q], em[1], a1);
        a2 = fmaf(w[e][q], em[2], a2);
        a3 = fmaf(w[e][q], em[3], a3);
        ab = fmaf(w[e][q], bq[q], ab);
      }
    }
    wx_lds[row * 4 + 0] = a0;
    wx_lds[row * 4 + 1] = a1;
    wx_lds[row * 4 + 2] = a2;
    wx_lds[row * 4 + 3] = a3;
    bx_lds[row] = ab + bih[row] + bhh[row];
  } else {
    f32x4 w = ld4(Wih + row * 4);
    wx_lds[row * 4 + 0] = w[0];
    wx_lds[row * 4 + 1] = w[1];
    wx_lds[row * 4 + 2] = w[2];
    wx_lds[row * 4 + 3] = w[3];
    bx_lds[row] = bih[row] + bhh[row];
  }
}

// W_hh rows straight from global memory: issued at the very top of a kernel so the loads overlap the
// LDS staging of the other weights; the composed input matrix / bias come from LDS after the barrier.
__device__ __forceinline__ void lstm_load_whh(LstmW& W, const float* Whh, int u0, int ln, int lg) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float* wr = Whh + (size_t)(g * 64 + u0 + ln) * 64 + 4 * lg;
#pragma unroll
    for (int j = 0; j < 4; ++j) W.whh[g][j] = ld4(wr + 16 * j);
  }
}
__device__ __forceinline__ void lstm_load_wx(LstmW& W, const float* wx_lds, const float* bx_lds, int u0, int ln, int lg) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    W.wx[g] = wx_lds[(g * 64 + u0 + ln) * 4 + lg];
    W.bias[g] = ld4(bx_lds + g * 64 + u0 + 4 * lg);
  }
}

// The generator's LSTM weights from the image buffer of the step (swimg, sw_common.h): W_hh as an operand-layout image
// (a wave's load instruction = 1 KB of consecutive memory; the row-per-lane loads of lstm_load_whh touch 64 cache lines
// per instruction), the composed input matrix and bias straight into their registers - no LDS staging, no barrier.
__device__ __forceinline__ void lstm_load_img(LstmW& W, const float* __restrict__ gimg, int wave, int lane) {
  const int ln = lane & 15, lg = lane >> 4, u0 = wave * 16;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) W.whh[g][j] = SW_OP_LD(gimg, swimg::OP_WHH, (size_t)4 * g + wave, j, lane);
    W.wx[g] = gimg[swimg::WX + (g * 64 + u0 + ln) * 4 + lg];
    W.bias[g] = ld4(gimg + swimg::BX + g * 64 + u0 + 4 * lg);
  }
}
// The encoder's operands: from the images of the step (gimg), or from the weights - W_hh straight into its registers, the
// composed Wx | bx through LDS (then the caller: sw_barrier(), if (!gimg) lstm_load_wx).
__device__ __forceinline__ void lstm_load_enc(LstmW& W, const float* gimg, const float* enc_w,
                                              float* wx_lds, float* bx_lds, int wave, int lane) {
  if (gimg) {   // weight images of this step, derived once by the staging launch (swimg, sw_common.h)
    lstm_load_img(W, gimg, wave, lane);
  } else {
    lstm_load_whh(W, enc_w + swp::ENC_WHH, wave * 16, lane & 15, lane >> 4);
    lstm_prep_rows(enc_w + swp::ENC_EMB_W, enc_w + swp::ENC_EMB_B, enc_w + swp::ENC_WIH, enc_w + swp::ENC_BIH,
                   enc_w + swp::ENC_BHH, true, wx_lds, bx_lds);
  }
}

// The products of one cell step for NB 16-agent tiles: acc[k][g] = Wx x_k + b + W_hh h_k (pre-activation rows of gate g),
// every W_hh operand issued against the NB h tiles in turn.  xb[k] = x4[agent ln][component lg] of tile k;
// hrow[k] = &h_lds_k[ln*ld + 4*lg] (previous h).  HP = false: the step starts from h = 0 - W_hh h adds exact zeros, so
// neither the 64 recurrent products nor the read of the (zeroed) h tile are issued: acc = Wx x + b.
template <int NB, bool HP = true>
__device__ __forceinline__ void lstm_products(const LstmW& W, const float (&xb)[NB], const float* const (&hrow)[NB],
                                              f32x4 (&acc)[NB][4]) {
  f32x4 b[NB][4];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    if constexpr (HP) {
#pragma unroll
      for (int j = 0; j < 4; ++j) b[k][j] = ld4(hrow[k] + 16 * j);   // one LDS round trip for the whole step
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[k][g] = SW_MFMA(W.wx[g], xb[k], W.bias[g]);
  }
  if constexpr (HP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int k = 0; k < NB; ++k) acc[k][g] = SW_MFMA(W.whh[g][j][r], b[k][j][r], acc[k][g]);
        }
      }
    }
  }
}

// The elementwise part of a cell step on the pre-activation gates acc[].  On return gate[] holds the post-activation
// gates i,f,g,o, c the new cell state, h the new h.
__device__ __forceinline__ void lstm_gates(const f32x4 acc[4], f32x4 gate[4], f32x4& c, f32x4& h) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float i = sw_sigmoid(acc[0][r]);
    float f = sw_sigmoid(acc[1][r]);
    float g = sw_tanh(acc[2][r]);
    float o = sw_sigmoid(acc[3][r]);
    float cn = fmaf(f, c[r], i * g);
    gate[0][r] = i;
    gate[1][r] = f;
    gate[2][r] = g;
    gate[3][r] = o;
    c[r] = cn;
    h[r] = o * sw_tanh(cn);
  }
}

// One cell step of NB tiles: the products, then the gate step per tile.  On return gate[k] holds tile k's post-activation
// gates i,f,g,o, c[k] its new cell state, h[k] its new h.
template <int NB>
__device__ __forceinline__ void lstm_cell(const LstmW& W, const float (&xb)[NB], const float* const (&hrow)[NB],
                                          f32x4 (&gate)[NB][4], f32x4 (&c)[NB], f32x4 (&h)[NB]) {
  f32x4 acc[NB][4];
  lstm_products<NB>(W, xb, hrow, acc);
#pragma unroll
  for (int k = 0; k < NB; ++k) lstm_gates(acc[k], gate[k], c[k], h[k]);
}
// ... of one tile: xb = x4[agent ln][component lg]; hrow = &h_lds[ln*SW_HLD + 4*lg] (previous h; HP = false: h = 0, not read).
template <bool HP = true>
__device__ __forceinline__ void lstm_cell(const LstmW& W, float xb, const float* hrow, f32x4 gate[4],
                                          f32x4& c, f32x4& h) {
  f32x4 acc[1][4];
  lstm_products<1, HP>(W, {xb}, {hrow}, acc);
  lstm_gates(acc[0], gate, c, h);
}

// Backward of one cell step (elementwise part).  In: dh, dc (gradients w.r.t. h_t, c_t), saved
// gates/c_t/c_{t-1}.  Out: dgate[] = gradients w.r.t. the four PRE-activation gate rows, dc :=
// gradient w.r.t. c_{t-1}.
__device__ __forceinline__ void lstm_cell_bwd(const f32x4 gate[4], f32x4 ct, f32x4 cprev, f32x4 dh,
                                              f32x4& dc, f32x4 dgate[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float i = gate[0][r], f = gate[1][r], g = gate[2][r], o = gate[3][r];
    float tc = sw_tanh(ct[r]);
    float d_o = dh[r] * tc;
    float dct = fmaf(dh[r] * o, 1.0f - tc * tc, dc[r]);
    dgate[0][r] = dct * g * i * (1.0f - i);
    dgate[1][r] = dct * cprev[r] * f * (1.0f - f);
    dgate[2][r] = dct * i * (1.0f - g * g);
    dgate[3][r] = d_o * o * (1.0f - o);
    dc[r] = dct * f;
  }
}

// The dgates rows of a BPTT step go to memory FROM THE LDS TILE the step builds anyway ([16 agents][SW_GLD]), behind the
// step's barrier and one agent per store instruction: a wave writes 4 agents' rows, lane l the l-th float4 of the 256-float
// row - 1 KB of consecutive memory per instruction (8 full cache lines).  Stored from the MFMA result registers a lane
// holds 4 units of one agent, i.e. an instruction scatters sixteen 64-byte pieces over sixteen rows - half-line writes,
// which the store path charges for: at the dense-crowd shape the dgates stores were a third of disc_bwd (round 3,
// SW_EXP_NOSTORE).  Rows beyond agent B-1 (padding of the last tile) go to `trash` (16 x 256 floats).
__device__ __forceinline__ void lstm_store_dgates_tile(const float* dgtile, float* __restrict__ rows /*row of agent a0*/,
                                                       float* __restrict__ trash, int a0, int B, int wave, int lane) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int a = 4 * wave + q;
    const f32x4 v = ld4(dgtile + a * SW_GLD + 4 * lane);
    // trash == nullptr: the padding rows of the tile are exact replicas of agent B-1 (every load of the kernel is clamped
    // to it) and are stored over its row - the same values to the same place
    float* dst = (a0 + a < B) ? rows + (size_t)a * 256 + 4 * lane
                 : trash      ? trash + a * 256 + 4 * lane
                              : rows + (size_t)(B - 1 - a0) * 256 + 4 * lane;
    st4g(dst, v);
  }
}

// Forward counterpart: the saved row of an LSTM step (gates i f g o | c | h = 384 floats per agent) is assembled in an LDS
// tile [16 agents][SW_ALD] - whose h columns double as the B operand of the next step's products - and written out behind
// the step's barrier, a wave storing 4 agents' rows as six 1 KB instructions of consecutive memory.
#define SW_ALD 388   // LDS row stride of a 384-wide saved row
__device__ __forceinline__ void lstm_put_act_tile(float* tile, const f32x4 gate[4], f32x4 c, f32x4 h, int ln, int lg, int u0) {
  float* row = tile + ln * SW_ALD + u0 + 4 * lg;
#pragma unroll
  for (int g = 0; g < 4; ++g) st4(row + g * 64, gate[g]);
  st4(row + 256, c);
  st4(row + 320, h);
}
__device__ __forceinline__ void lstm_store_act_tile(const float* tile, float* __restrict__ rows_t /*row of agent 0 at this step*/,
                                                    int a0, int B, int wave, int lane) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int f = k * 64 + lane, q = f / 96, c4 = f - q * 96;      // float4 c4 of agent 4 wave + q
    const int a = 4 * wave + q;
    const f32x4 v = ld4(tile + a * SW_ALD + 4 * c4);
    st4g(rows_t + (size_t)min(a0 + a, B - 1) * 384 + 4 * c4, v);     // padding rows: replicas of agent B-1, same values
  }
}

// W_hh^T in registers for dh_{t-1} = W_hh^T dgates: whhT[j][r] = Whh[16j + 4lg + r][u0 + ln].
struct LstmWT {
  f32x4 whhT[16];
};
__device__ __forceinline__ void lstm_load_wT(LstmWT& W, const float* Whh, int u0, int ln, int lg) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) W.whhT[j][r] = Whh[(size_t)(16 * j + 4 * lg + r) * 64 + u0 + ln];
  }
}
// dgrow = &dg_lds[ln*SW_GLD + 4*lg]
__device__ __forceinline__ f32x4 lstm_dh_prev(const LstmWT& W, const float* dgrow) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  f32x4 b[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = ld4(dgrow + 16 * j);
#pragma unroll
  for (int j = 0; j < 16; j += 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      a0 = SW_MFMA(W.whhT[j][r], b[j][r], a0);
      a1 = SW_MFMA(W.whhT[j + 1][r], b[j + 1][r], a1);
    }
  }
  return a0 + a1;
}
// W_hh^T from its operand-layout image d of img (16 contiguous 1 KB loads per wave) or, without an image, from the
// weights Whh (Whh == nullptr: the image is always there)
__device__ __forceinline__ void lstm_load_whhT(LstmWT& W, const float* img, const OpImage d, const float* Whh, int wave, int lane) {
  if (img || !Whh) {
#pragma unroll
    for (int j = 0; j < 16; ++j) W.whhT[j] = SW_OP_LD(img, d, (size_t)wave, j, lane);
  } else {
    lstm_load_wT(W, Whh, wave * 16, lane & 15, lane >> 4);
  }
}

// ---- the BPTT over saved rows (enc_lstm_bwd_kernel, disc_bwd_kernel, disc_update_kernel) ------------------------------
// Per step: elementwise gate gradients (lane-local) -> dgates tile in LDS -> dgates rows to HBM (for the deferred
// weight-gradient GEMM) -> dh_{t-1} = W_hh^T dgates on the matrix cores.  As in enc_lstm_fwd the loop body has NO
// conditional memory operation (the boundary steps are peeled, padding lanes of the last tile are replicas of agent B-1
// and store the same values or go to `trash`): with conditional loads / stores the compiler waited for everything in
// flight (s_waitcnt vmcnt(0)) behind every step's barrier - the dgates rows just stored included.
struct LstmBptt {
  const float* act;     // saved row of the lane's agent at step 0 (column u0 + 4 lg); one step = B * 384 floats
  const float* cstart;  // c_{-1} of the sequence start (same column), or nullptr: zero
  float* tile;          // [2][16][SW_GLD] dgates tiles in LDS
  float* dg;            // dgates row of agent a0 at step 0; one step = B * 256 floats
  float* trash;         // see lstm_store_dgates_tile
  int a0, B;
};
__device__ __forceinline__ int lstm_bptt_bound(const LstmBptt& S) { return S.B; }   // rows a0 .. bound-1 are the tile's
// ... of a tile that holds ONE SCENE inside the batch (the scene-per-workgroup launch): B stays the time-major stride, the
// rows end at `bound`, so that a scene never stores into its neighbour's rows
struct LstmBpttScene : LstmBptt {
  int bound;
};
__device__ __forceinline__ int lstm_bptt_bound(const LstmBpttScene& S) { return S.bound; }
struct SwNop {
  template <class... A> __device__ void operator()(A&&...) const {}
};
// The rows of step t: gates and c_t, c_{t-1} from the row in front (HP) or, at the sequence start, from cstart (one load
// from a selected address, zeroed afterwards: a load under a branch costs the exact vmcnt bookkeeping of everything behind it)
template <bool HP>
__device__ __forceinline__ void lstm_bptt_load(const LstmBptt& S, int t, f32x4 (&gate)[4], f32x4& ct, f32x4& cprev) {
  const size_t tstep = (size_t)S.B * 384;
  const float* row = S.act + (size_t)t * tstep;
#pragma unroll
  for (int q = 0; q < 4; ++q) gate[q] = ld4(row + q * 64);
  ct = ld4(row + 256);
  if constexpr (HP) {
    cprev = ld4(row - tstep + 256);
  } else {
    cprev = ld4(S.cstart ? S.cstart : row + 256);
    if (!S.cstart) cprev = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
// One step t on the rows in gate / ct / cprev, dh and dc carried.  PF: the rows of step t-1 (HP: with a row in front) are
// requested right behind the last use of step t's, into the same registers (rolling prefetch, DESIGN section 3 "one
// register set"); NX: dh_{t-1} is formed.  stamp(k): the phase stamps 12-14 of disc_bwd (SW_PHASE_STAMPS).
template <bool PF, bool HP, bool NX, class Stamp = SwNop, class St = LstmBptt>
__device__ __forceinline__ void lstm_bptt_step(const LstmWT& W, const St& S, int t, f32x4 (&gate)[4], f32x4& ct,
                                               f32x4& cprev, f32x4& dh, f32x4& dc, Stamp stamp = {}) {
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  f32x4 dgate[4];
  lstm_cell_bwd(gate, ct, cprev, dh, dc, dgate);
  if constexpr (PF) {
    lstm_bptt_load<HP>(S, t - 1, gate, ct, cprev);
    asm volatile("" ::: "memory");
  }
  float* tile = S.tile + (t & 1) * 16 * SW_GLD;
  float* dgl = tile + ln * SW_GLD + 16 * wave + 4 * lg;
#pragma unroll
  for (int g = 0; g < 4; ++g) st4(dgl + g * 64, dgate[g]);
  stamp(12);
  sw_barrier();
  lstm_store_dgates_tile(tile, S.dg + (size_t)t * S.B * 256, S.trash, S.a0, lstm_bptt_bound(S), wave, lane);
  stamp(13);
  if constexpr (NX) dh = lstm_dh_prev(W, tile + ln * SW_GLD + 4 * lg);
  // the prefetched rows are not touched before the matrix products above have been issued
  if constexpr (PF) asm volatile("" : "+v"(gate[0]), "+v"(gate[1]), "+v"(gate[2]), "+v"(gate[3]), "+v"(ct), "+v"(cprev));
  stamp(14);
}
// The whole BPTT of T steps: the first rows, steps T-1 .. 2 in a loop, the peeled steps 1 and 0 (DH0: dh of step 0 too, for
// dh0).  pre(dh) runs in front of every step's cell backward.  Every load issued so far (the first rows, W_hh^T) is waited
// for in front of the loop: a loop header with an unknown count of pending operations gets s_waitcnt vmcnt(0), which every
// step then pays as the round trip of the dgates rows it has just stored.  stamp(k): called at points 10-14 (the phase
// stamps of disc_bwd; disc_update puts its barrier at 10, behind the request of the first rows).
template <bool DH0, class Pre = SwNop, class Stamp = SwNop, class St = LstmBptt>
__device__ __forceinline__ void lstm_bptt_rows(LstmWT& W, const St& S, int T, f32x4& dh, f32x4& dc, Pre pre = {},
                                               Stamp stamp = {}) {
  f32x4 gate[4], ct, cprev;
  if (T > 1) lstm_bptt_load<true>(S, T - 1, gate, ct, cprev);
  else lstm_bptt_load<false>(S, 0, gate, ct, cprev);
  stamp(10);
  pre(dh);
  asm volatile("" : "+v"(gate[0]), "+v"(gate[1]), "+v"(gate[2]), "+v"(gate[3]), "+v"(ct), "+v"(cprev), "+v"(dh));
#pragma unroll
  for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(W.whhT[j]));
  for (int t = T - 1; t >= 2; --t) {
    lstm_bptt_step<true, true, true>(W, S, t, gate, ct, cprev, dh, dc, stamp);
    pre(dh);
  }
  if (T > 1) {
    lstm_bptt_step<true, false, true>(W, S, 1, gate, ct, cprev, dh, dc, stamp);
    pre(dh);
  }
  lstm_bptt_step<false, false, DH0>(W, S, 0, gate, ct, cprev, dh, dc, stamp);
  stamp(11);
}

// x4[agent][t][comp] for the observation rule of get_traj_4d (train.py:131-133): v_0 := v_1, as two raw loads
// (a, q) with x = a - (comp >= 2 ? q : 0).  Branch-free and split from the arithmetic on purpose: memory operations
// under lane-dependent branches make the compiler lose count of what is in flight (it then waits for everything,
// s_waitcnt vmcnt(0)), and arithmetic on a prefetched value gets scheduled right behind its load.
__device__ __forceinline__ void obs_x4_load(const float* pos, int b, int t, int T, int comp, float& a, float& q) {
  const float* p = pos + (size_t)b * T * 2;
  const int c = comp & 1, tt = t == 0 ? 1 : t;
  const bool vel = comp >= 2;
  a = p[(vel ? tt : t) * 2 + c];
  q = p[(vel ? tt - 1 : t) * 2 + c];
}
__device__ __forceinline__ float obs_x4(const float* pos, int b, int t, int T, int comp) {
  float a, q;
  obs_x4_load(pos, b, t, T, comp, a, q);
  return a - (comp >= 2 ? q : 0.f);
}

// ---- ragged observation histories (sw_enc_lstm_fwd_ragged*, sw_disc_*_ragged) -----------------------------------------
// Row b of x holds n = obs_len[b] valid frames RIGHT-ALIGNED in its T columns: its LSTM starts from the zero state at step
// s = T - n, the columns in front of s are padding that is never read.  n is clamped on the device into 2 .. T for positions
// (the velocity rule needs two points), 1 .. T for 4-d input; obs_len == nullptr: every row starts at 0.
__device__ __forceinline__ int obs_start(const int* __restrict__ obs_len, int b, int T, int xmode) {
  const int n = obs_len ? min(max(obs_len[b], xmode == 0 ? 2 : 1), T) : T;
  return T - n;
}
// obs_x4_load for a row that starts at step s: t is clamped to >= s and the first-frame rule v_s := v_{s+1} sits at s
// (get_traj_4d on the valid frames alone); s = 0 is obs_x4_load.  Branch-free like it.
__device__ __forceinline__ void obs_x4_load_from(const float* pos, int b, int t, int s, int T, int comp, float& a, float& q) {
  const float* p = pos + (size_t)b * T * 2;
  const int c = comp & 1, te = max(t, s), tt = te == s ? s + 1 : te;
  const bool vel = comp >= 2;
  a = p[(vel ? tt : te) * 2 + c];
  q = p[(vel ? tt - 1 : te) * 2 + c];
}

// ---- THE forward time loop of the 64-unit LSTM over an observed track -------------------------------------------------
// (enc_lstm_fwd_kernel and, through lstm_obs_pass below, every observation pass of the discriminator) for the 16-agent tile
// of agent row b (clamped), W loaded, c / h the initial state with h already in hbuf[0].  One step: fetch the next input,
// cell, [select the zero state], h into the LDS tile, [save the row], barrier.
//   XMODE   0: x = positions [B][T][2], the 4-d state formed on the fly; 1: x = [B][T][4]
//   SAVE    what step t leaves at act + ((t0 + t) B + b) 384 = gates i|f|g|o [256], c [64], h [64] (t0: the encoder's first
//           row; the index itself is an argument, not an offset of act: the tile stores keep their 32-bit row arithmetic):
//           SAVE_NONE  nothing; hbuf is [2][16][SW_HLD]
//           SAVE_ROWS  the row straight from the registers (act = row 0 of step 0)
//           SAVE_TILE  through the LDS row tile: hbuf is [2][16][SW_ALD], its h columns (320 ..) are the next step's
//                      operand, and the rows leave behind the step's barrier as 1 KB stores (a0 = the tile's first agent)
//   X4S     the step's 4-d input goes to x4s + ((t0 + t) B + b) 4 (with every saving form; the encoder also asks for it alone)
//   RAGGED  false: step 0 is peeled and, unless hp0 (the caller passed an initial h: a UNIFORM run-time branch whose two
//           sides issue the same global loads and stores in the same order), issues only Wx x + b - from h = 0 neither the
//           recurrent products nor the read of hbuf[0] (lstm_products with HP = false).
//           true: a start step s per lane (obs_start) FROM THE ZERO STATE.  Every lane computes the cell on every step -
//           step 0 keeps its full products: a lane may start anywhere - with the input index clamped to >= s, so that the
//           cell runs on finite values and nothing of the padding is loaded, and a lane in front of its start SELECTS the
//           zero state instead of the cell's result.  From s on the lane's agent sees exactly the operands of the T - s
//           step run on its valid frames (an agent is one column of the products): h_T / c carry the bits of the dense
//           loop on the truncated buffer.  A saving form stores the SELECTED row and input - zeros in front of s - so that
//           the dense BPTT and weight-gradient kernels give the ragged gradients as they are (zero gates with zero c_t,
//           c_{t-1}: zero dgates, dc_{t-1} = 0).  Selected, never computed from the padding: 0 * NaN would poison the GEMM.
//   post(h) runs per step behind the LDS store of h (the encoder's y rows).
// What every form keeps:
//   - the loop body has NO memory operation under a lane- or wave-dependent branch: everything that differs between the
//     forms is `if constexpr`.  With run-time conditions the compiler loses count of what is in flight and waits for
//     everything (s_waitcnt vmcnt(0)) in front of every step's barrier: one store round trip per step;
//   - the first input is waited for in front of the loop header (the asm anchor), which must see no pending load on any
//     path in;
//   - the input of step t+1 is fetched while step t computes (the last step re-fetches its own: no conditional load) and
//     is not touched before the step's barrier (the second anchor);
//   - stores are unconditional, their VALUES are selected; all four waves hold the same x_t and all store it;
//   - padding lanes of the last tile are exact replicas of agent B-1 (every load is clamped to it) and store the same
//     values to the same rows;
//   - on return h_T sits in hbuf[T & 1].
enum { SAVE_NONE = 0, SAVE_ROWS = 1, SAVE_TILE = 2 };
template <int XMODE, int SAVE, bool RAGGED, bool X4S = SAVE != SAVE_NONE, class Post = SwNop>
__device__ __forceinline__ void lstm_obs_loop(const LstmW& W, float* hbuf, const float* __restrict__ x, int T, int B, int b, int s,
                                              bool hp0, f32x4& c, f32x4& h, float* __restrict__ act, float* __restrict__ x4s,
                                              int a0 = 0, int t0 = 0, Post post = {}) {
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int u0 = wave * 16;
  constexpr int HS = SAVE == SAVE_TILE ? SW_ALD : SW_HLD, HO = SAVE == SAVE_TILE ? 320 : 0;
  float xa, xq = 0.f;
  auto load_x = [&](int t) {
    if constexpr (RAGGED) {
      if constexpr (XMODE == 0) obs_x4_load_from(x, b, t, s, T, lg, xa, xq);
      else xa = x[((size_t)b * T + max(t, s)) * 4 + lg];
    } else {
      if constexpr (XMODE == 0) obs_x4_load(x, b, t, T, lg, xa, xq);
      else xa = x[((size_t)b * T + t) * 4 + lg];
    }
  };
  load_x(0);
  asm volatile("" : "+v"(xa), "+v"(xq));
  float* arow = SAVE == SAVE_ROWS ? act + ((size_t)t0 * B + b) * 384 + u0 + 4 * lg : nullptr;
  float* xrow = X4S ? x4s + ((size_t)t0 * B + b) * 4 + lg : nullptr;
  auto step = [&](int t, auto hp) {
    float xb = XMODE == 0 ? xa - (lg >= 2 ? xq : 0.f) : xa;
    load_x(min(t + 1, T - 1));
    f32x4 gate[4];
    lstm_cell<decltype(hp)::value>(W, xb, &hbuf[(t & 1) * 16 * HS + ln * HS + HO + 4 * lg], gate, c, h);
    if constexpr (RAGGED) {
      const bool on = t >= s;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        c[r] = on ? c[r] : 0.f;
        h[r] = on ? h[r] : 0.f;
      }
      if constexpr (SAVE != SAVE_NONE) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) gate[g][r] = on ? gate[g][r] : 0.f;
      }
      if constexpr (X4S) xb = on ? xb : 0.f;
    }
    float* hnext = hbuf + ((t + 1) & 1) * 16 * HS;
    if constexpr (SAVE == SAVE_TILE) lstm_put_act_tile(hnext, gate, c, h, ln, lg, u0);
    else st4(&hbuf[((t + 1) & 1) * 16 * HS + ln * HS + u0 + 4 * lg], h);
    post(h);
    if constexpr (SAVE == SAVE_ROWS) {
#pragma unroll
      for (int g = 0; g < 4; ++g) st4g(arow + g * 64, gate[g]);
      st4g(arow + 256, c);
      st4g(arow + 320, h);
      arow += (size_t)B * 384;
    }
    if constexpr (X4S) {
      *xrow = xb;
      xrow += (size_t)B * 4;
    }
    sw_barrier();
    if constexpr (SAVE == SAVE_TILE) lstm_store_act_tile(hnext, act + (size_t)(t0 + t) * B * 384, a0, B, wave, lane);
    asm volatile("" : "+v"(xa), "+v"(xq));
  };
  if constexpr (RAGGED) {
    for (int t = 0; t < T; ++t) step(t, std::true_type{});
  } else {
    if (hp0) step(0, std::true_type{});
    else step(0, std::false_type{});
    for (int t = 1; t < T; ++t) step(t, std::true_type{});
  }
}
// The observation pass of the discriminator (FROM THE ZERO STATE: c = h = 0, hbuf[0] zeroed; train.py:296-297): the run-time
// x_mode and `save` (rows straight from the registers, or nothing) to the instantiation, chosen once in front of the loop.
// s: the lane's start step (obs_start; RAGGED only).
template <bool RAGGED>
__device__ __forceinline__ void lstm_obs_pass(int x_mode, bool save, const LstmW& W, float* hbuf, const float* __restrict__ x,
                                              int T, int B, int b, int s, f32x4& c, f32x4& h, float* __restrict__ act,
                                              float* __restrict__ x4s) {
  if (x_mode == 0) {
    if (save) lstm_obs_loop<0, SAVE_ROWS, RAGGED>(W, hbuf, x, T, B, b, s, false, c, h, act, x4s);
    else lstm_obs_loop<0, SAVE_NONE, RAGGED>(W, hbuf, x, T, B, b, s, false, c, h, act, x4s);
  } else {
    if (save) lstm_obs_loop<1, SAVE_ROWS, RAGGED>(W, hbuf, x, T, B, b, s, false, c, h, act, x4s);
    else lstm_obs_loop<1, SAVE_NONE, RAGGED>(W, hbuf, x, T, B, b, s, false, c, h, act, x4s);
  }
}

// Observation LSTM of the discriminator (train.py:296-299) for the 16-agent tile at a0, leaving the rows its
// backward needs (see lstm_obs_loop).  It exists as a function so that idle workgroups of ANOTHER launch can run it
// (the first D pass of a step does not depend on the generator: sw_dec_rollout_fwd_aux).
// smem: [2][16][SW_HLD] h tiles | [256][4] Wx | [256] bx  (2 * 16 * SW_HLD + 1280 floats).
__device__ __forceinline__ void disc_obs_lstm_tile(float* smem, const float* __restrict__ obsv, int To, int x_mode,
                                                   const float* wih, const float* whh, const float* bih, const float* bhh,
                                                   int B, int a0, float* __restrict__ act, float* __restrict__ x4s) {
  float* hbuf = smem;
  float* wx_lds = smem + 2 * 16 * SW_HLD;
  float* bx_lds = wx_lds + 1024;
  const int lane = sw_lane(), wave = sw_wave(), ln = lane & 15, lg = lane >> 4;
  const int u0 = wave * 16;
  const int b = min(a0 + ln, B - 1);
  LstmW W;
  lstm_load_whh(W, whh, u0, ln, lg);
  lstm_prep_rows(nullptr, nullptr, wih, bih, bhh, false, wx_lds, bx_lds);
  f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};
  st4(&hbuf[ln * SW_HLD + u0 + 4 * lg], h);
  sw_barrier();
  lstm_load_wx(W, wx_lds, bx_lds, u0, ln, lg);
  lstm_obs_pass<false>(x_mode, true, W, hbuf, obsv, To, B, b, 0, c, h, act, x4s);
}
