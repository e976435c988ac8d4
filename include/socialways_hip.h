/* socialways_hip.h - C ABI of the MI355X (gfx950) Social Ways hot path.
 *
 * The reference (crowdbotp/socialways) has no FFI of its own: its hot path is the Python call
 * surface of train.py.  This header is the boundary UNDER that surface: every
 * entry point below replaces the stock-PyTorch ops one reference function dispatches to, and the
 * Python glue in socialways_amd/ (same class / function names as the reference) calls exactly
 * these symbols through ctypes.  INTEGRATION.md shows the binding a maintainer of the reference
 * would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (int32 for scene offsets), 16-byte
 *     aligned; the caller owns all memory (the library never allocates);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 ok, -1 bad argument, -2 unsupported shape, -3 HIP error (sw_last_error());
 *   - "packed" weight buffers hold the tensors of the reference module's state_dict() in key
 *     order, row-major, each tensor starting on a 4-float boundary (sw_param_offset() is the
 *     authority; only Discriminator.classifier.2.bias (1 float) introduces padding);
 *   - B = agents in the packed batch, H = 64 hidden, Z = 32 noise, To / Tp = obs / pred length,
 *     scene_off = int32[S+1] prefix offsets of the scenes ("sub_batches" of train.py:446-461).
 *   - time-major workspaces ("gsave", "dsave", "*delta*") are opaque to the caller except for
 *     their sizes, which sw_workspace_floats() returns.
 */
#ifndef SOCIALWAYS_HIP_H
#define SOCIALWAYS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SW_OK 0
#define SW_EARG -1
#define SW_ESHAPE -2
#define SW_EHIP -3

#define SW_H 64
#define SW_Z 32

/* parameter groups for sw_param_offset / sw_param_count */
enum { SW_GRP_ENC = 0, SW_GRP_EMB = 1, SW_GRP_ATT = 2, SW_GRP_DEC = 3, SW_GRP_DISC = 4 };

/* workspace ids for sw_workspace_floats */
enum {
  SW_WS_GSAVE = 0,   /* generator forward saves (LSTM acts, x4, decoder acts, attention weights) */
  SW_WS_GDELTA = 1,  /* generator backward deltas                                                */
  SW_WS_DSAVE = 2,   /* discriminator forward saves (per call, nb pred branches)                 */
  SW_WS_DDELTA = 3,  /* discriminator backward deltas                                            */
  SW_WS_WGRAD = 4,   /* split-K partials of the weight-gradient GEMMs                            */
  SW_WS_PAIRS = 5    /* per-pair rows of the social block backward (P pairs)                     */
};

int sw_version(void);
const char* sw_last_error(void);

/* Packed-weight layout: number of floats of group `grp` and the float offset of its `idx`-th
 * state_dict tensor (Tp only matters for SW_GRP_DISC: pred_encoder.0.weight is (32, 4*Tp)). */
int sw_param_count(int grp, int Tp);
int sw_param_offset(int grp, int idx, int Tp);
int sw_param_tensors(int grp);
size_t sw_workspace_floats(int ws_id, int B, int To, int Tp, int nb, long long P);

/* ---- get_traj_4d (train.py:130-138) ------------------------------------------------------- */
int sw_traj_4d(const float* obsv /*[B,To,2]*/, const float* pred /*[B,Tp,2] or NULL*/, int B, int To,
               int Tp, float* obsv4 /*[B,To,4]*/, float* pred4 /*[B,Tp,4] or NULL*/, void* stream);

/* ---- EncoderLstm (train.py:245-269): Linear(4->64) + LSTM(64->64), time-unrolled ----------- */
/* x_mode 0: `x` = positions [B,T,2], the 4-d state is formed on the fly with the OBSERVATION rule
 * of get_traj_4d; x_mode 1: `x` = 4-d states [B,T,4].  h0/c0 NULL = zeros (predict(), :399-401).
 * y/act/x4s may be NULL.  act = [t0+T][B][384] rows (i f g o | c | h), x4s = [..][B][4]; the
 * kernel writes rows t0 .. t0+T-1.                                                             */
int sw_enc_lstm_fwd(const float* x, int x_mode, const float* enc_w, const float* h0, const float* c0,
                    int B, int T, float* hT, float* cT, float* y /*[B,T,64]*/, float* act,
                    float* x4s, int t0, void* stream);
/* Same, plus an auxiliary copy aux_src -> aux_dst (aux_n floats, multiple of 4; aux_src may be host-pinned memory)
 * done by extra workgroups of the same launch: the LSTM kernel is latency-bound and leaves CUs idle, so the
 * training step fetches z from its pinned slot here instead of in a kernel of its own.                        */
int sw_enc_lstm_fwd_aux(const float* x, int x_mode, const float* enc_w, const float* h0, const float* c0, int B, int T,
                        float* hT, float* cT, float* y, float* act, float* x4s, int t0, const float* aux_src,
                        float* aux_dst, long long aux_n, void* stream);
/* The inference form (zero initial state, nothing saved) for RAGGED observation histories.  `x` stays the dense buffer,
 * RIGHT-ALIGNED: row a has n_a = obs_len[a] valid frames in columns s_a = T - n_a .. T-1, 2 <= n_a <= T for positions
 * (x_mode 0), 1 <= n_a <= T for 4-d input (x_mode 1); the columns in front of s_a are padding.  obs_len: int32 [B] on
 * the device, NULL = every row has T frames.  Row a's state is zero until step s_a, steps s_a .. T-1 run the cell on the
 * 4-d states get_traj_4d gives for the valid frames alone (x_t = (p_t, p_t - p_{t-1}) for t > s_a, (p_s, p_{s+1} - p_s)
 * at s_a): hT[a] / cT[a] are, bit for bit, what sw_enc_lstm_fwd returns for the [1, n_a, .] buffer of the valid frames,
 * with and without registered generator images (sw_gen_images).  The padding is never read: no output bit depends on
 * it, NaN / Inf included.  An obs_len outside its range is clamped into it on the device (no out-of-bounds read, no
 * host sync).  The step loop keeps the shape of the dense kernel - every lane computes every step and selects the zero
 * state in front of its start, no conditional memory operation, one uniform barrier per step: it is the RAGGED instance
 * of the kernel sw_enc_lstm_fwd launches (one loop, csrc/sw_lstm_dev.h lstm_obs_loop), on a grid of tiles only.
 * SW_EARG before any device call: x, enc_w, hT or cT NULL, B < 0, T < 1, x_mode not 0 / 1, T < 2 with x_mode 0.
 * B == 0: SW_OK without a launch.                                                                                       */
int sw_enc_lstm_fwd_ragged(const float* x, int x_mode, const float* enc_w, const int* obs_len /*[B] int32 or NULL = all T*/,
                           int B, int T, float* hT /*[B,64]*/, float* cT /*[B,64]*/, void* stream);
/* The TRAINING form of sw_enc_lstm_fwd_ragged: the same ragged pass (x right-aligned, obs_len int32 [B] on the device or
 * NULL = every row has T frames, clamped on the device into 2 .. T for positions / 1 .. T for 4-d input, zero initial state,
 * the padding never read) that also leaves the rows the backward needs, in the layout of sw_enc_lstm_fwd(..., act, x4s,
 * t0 = 0): act = [T][B][384] rows (i f g o | c | h), x4s = [T][B][4].  For row a with s_a = T - obs_len[a]:
 *   steps t >= s_a: act[t][a], x4s[t][a], hT[a], cT[a] are, bit for bit, what sw_enc_lstm_fwd saves / returns at step
 *                   t - s_a of the [1, n_a, .] buffer of the valid frames, with and without registered generator images;
 *   steps t <  s_a: act[t][a] and x4s[t][a] are all-zero bits - SELECTED zeros, never values computed from the padding.
 * With these rows the dense backward gives the ragged gradients as it is: sw_enc_lstm_bwd* forms zero dgates rows in
 * front of s_a (i = g = o = 0, c_t = c_{t-1} = 0) and takes c_{s-1} = h_{s-1} = 0 as the initial state at s_a, and the
 * weight-gradient sums (sw_gen_wgrad*) get zero dgates against zero inputs there.  The step loop keeps the shape of the
 * dense kernel (every lane computes every step, unconditional stores of selected values, one barrier per step, the saved
 * row assembled in the LDS row tile): the RAGGED instance of the kernel sw_enc_lstm_fwd(..., act, x4s) launches.  No
 * auxiliary copy: the caller moves z itself.
 * SW_EARG before any device call: x, enc_w, hT, cT, act or x4s NULL, B < 0, T < 1, x_mode not 0 / 1, T < 2 with x_mode 0.
 * B == 0: SW_OK without a launch.                                                                                       */
int sw_enc_lstm_fwd_ragged_save(const float* x, int x_mode, const float* enc_w, const int* obs_len /*[B] int32 or NULL = all T*/,
                                int B, int T, float* hT /*[B,64]*/, float* cT /*[B,64]*/, float* act /*[T,B,384]*/,
                                float* x4s /*[T,B,4]*/, void* stream);
/* BPTT over rows t0+T-1 .. t0 of `act`; dhT/dcT = gradient w.r.t. the final state (dcT may be
 * NULL); dy optional [B,T,64].  Writes dgates rows [t][B][256]; dh0/dc0 optional outputs.       */
int sw_enc_lstm_bwd(const float* enc_w, const float* act, const float* c0, const float* dhT,
                    const float* dcT, const float* dy, int B, int T, int t0, float* dgates,
                    float* dh0, float* dc0, void* stream);

/* ---- SocialFeatures + EmbedSocialFeatures + AttentionPooling (train.py:153-241), fused,
 *      block-diagonal: only in-scene pairs are formed (identical math) -------- */
/* Scenes of up to SW_AMAX = 64 agents run one workgroup per scene (scores in LDS).  Larger scenes are
 * listed by the caller as blocks of 16 query agents, big_blocks = int32 [NB][8] records
 *   { scene, i0, partial row base of the block, partial row base of its scene, blocks in the scene,
 *     block index in the scene, 0, 0 }
 * (partial rows: 132 floats each, sum over big scenes of blocks*agents rows - used by the backward), and
 * run as row-block kernels with an online softmax; wh_ws (132 B floats) receives W h + b [B,64], then
 * v = W3^T (W h + b) [B,64] and c = <b3, W h + b> [B] - what the attention needs of the embedder's last layer fc.4
 * (weight W3, bias b3), which is never run per pair; ml [B,2] the softmax statistics (running max, normaliser)
 * the backward needs.  Amax = largest scene NOT in big_blocks.                                         */
int sw_social_pool_fwd(const float* obsv /*[B,To,2]*/, int To, const float* h /*[B,64]*/,
                       const int* scene_off, int S, int B, int Amax /*<= 64*/,
                       const float* emb_w, const float* att_w, float* S_out /*[B,64]*/,
                       float* attn /*[B,64] softmax weights (row i, column j_local) or NULL*/,
                       const int* big_blocks /*or NULL*/, int NB, float* wh_ws, float* ml /*or NULL*/, void* stream);
/* the same with an auxiliary copy aux_dst[0..aux_n) = aux_src[0..aux_n) (floats, aux_n % 4 == 0) done by extra
 * workgroups of the launch (the captured training step pulls z out of its pinned host slot here)          */
int sw_social_pool_fwd_aux(const float* obsv, int To, const float* h, const int* scene_off, int S, int B, int Amax,
                           const float* emb_w, const float* att_w, float* S_out, float* attn, const int* big_blocks,
                           int NB, float* wh_ws, float* ml, const float* aux_src, float* aux_dst, long long aux_n,
                           void* stream);
/* dense SocialFeatures (train.py:229-241) for the reference's module-level API on small batches */
int sw_social_features(const float* x4_last /*[B,4]*/, int B, float* feat /*[B,B,3]*/, void* stream);
/* EmbedSocialFeatures.forward on R rows of 3 features -> [R,64]; AttentionPooling.forward on a
 * dense (B,B,64) embedding tensor (only the in-scene blocks are read).                           */
int sw_embed_features(const float* feat /*[R,3]*/, long long R, const float* emb_w, float* out /*[R,64]*/,
                      void* stream);
int sw_attention_pool_dense(const float* f /*[B,B,64]*/, const float* h /*[B,64]*/, const int* scene_off,
                            int S, int B, const float* att_w, float* S_out /*[B,64]*/, void* stream);
/* ---- backward passes of the STAND-ALONE sub-modules (the reference's modules are ordinary nn.Modules: a user may
 *      compose AttentionPooling / EmbedSocialFeatures / EncoderLstm / DecoderFC differently from predict() and
 *      back-propagate through them, train.py:153-189, 245-269, 320-335).  Not on the training step's path. ------- */
/* y[r][n] (+)= bias[n] + sum_k x[r][k] w[k*w_rs + n*w_cs]  (w or w^T by the strides; bias may be NULL)              */
int sw_rows_gemm(const float* x, int ldx, const float* w, int w_rs, int w_cs, const float* bias, long long R, int K, int N,
                 float* y, int ldy, int accumulate, void* stream);
/* dW[N][K] (+)= delta^T act, db[N] (+)= column sums of delta (db may be NULL): one problem of the grouped weight-gradient
 * GEMM; wgrad_ws = sw_workspace_floats(SW_WS_WGRAD, ...) floats.  N <= 256; ldd, lda multiples of 4.               */
int sw_linear_wgrad(const float* delta, int ldd, const float* act, int lda, int R, int N, int K, float* dW, int ldw,
                    float* db, float* wgrad_ws, int accumulate, void* stream);
/* EmbedSocialFeatures backward on R rows: recomputes the MLP, leaves rows = h2 [R,64] | dh2 [R,64] | h1 [R,32] | dh1 [R,32] |
 * feat4 [R,4] (196 R floats) for sw_linear_wgrad (dout x h2, dh2 x h1, dh1 x feat4) and dfeat [R,3] (or NULL).        */
int sw_embed_features_bwd(const float* feat /*[R,3]*/, long long R, const float* emb_w, const float* dout /*[R,64]*/,
                          float* rows, float* dfeat, void* stream);
/* AttentionPooling on a dense (B,B,64) embedding tensor, ANY scene size (one workgroup per agent): wh = W h + b [B,64]
 * (sw_rows_gemm), attn [B,B] receives a_ij inside the scene blocks.  Backward: dsig [B,B] scratch, df [B,B,64] (or
 * NULL; zero outside the scene blocks on entry), dwh [B,64] = dL/d(Wh), dh [B,64] = sum_i a_ij dS_i (the caller adds
 * W^T dwh and forms dW, db from dwh and h).                                                                        */
int sw_attention_dense_fwd(const float* f, const float* h, const float* wh, const int* scene_off, int S, int B, float* attn,
                           float* S_out, void* stream);
int sw_attention_dense_bwd(const float* f, const float* h, const float* wh, const float* attn, const float* dS,
                           const int* scene_off, int S, int B, float* dsig, float* df, float* dwh, float* dh, void* stream);
/* Weight gradients of EncoderLstm over T steps from state (h0 or NULL = zeros): act / x4s as sw_enc_lstm_fwd left them,
 * dgates from sw_enc_lstm_bwd; tmp = 2048 floats.  Writes the whole packed gradient buffer d_enc_w.                 */
int sw_enc_lstm_wgrad(const float* enc_w, const float* act, const float* x4s, const float* h0, const float* dgates, int B,
                      int T, float* d_enc_w, float* wgrad_ws, float* tmp, void* stream);
/* Weight gradients of DecoderFC on one batch = a Tp = 1 rollout (gsave / gdelta of sw_dec_rollout_fwd / _bwd called
 * with this To and Tp = 1) with its inputs h, s (NULL = zeros), z; tmp = 2048 floats.  Writes the whole d_dec_w.   */
int sw_dec_fc_wgrad(const float* dec_w, const float* gsave, const float* gdelta, const float* h, const float* s,
                    const float* z, int B, int To, float* d_dec_w, float* wgrad_ws, float* tmp, void* stream);

/* ... and dz [B,32] = dL/dz of that rollout (predict() never needs it: z is data, train.py:473)                    */
int sw_dec_fc_dz(const float* dec_w, const float* gdelta, int B, int To, float* dz, void* stream);

/* pair_off = int64[S+1] prefix sums of n_s^2 over scenes with n_s > 1 (single-agent scenes own no
 * pair rows), P = pair_off[S].  dh is accumulated into.  d_emb_w / d_att_w are overwritten.
 * pair_ws holds sw_workspace_floats(SW_WS_PAIRS, ...) floats.                                    */
/* Host-side handle carrying weight-gradient problems from one call to a later launch (the grouped GEMM launches
 * are occupancy-bound: one launch per backward pass beats one per module).  Not thread-safe per handle.     */
typedef struct sw_wgrad_batch sw_wgrad_batch;
sw_wgrad_batch* sw_wgrad_batch_new(void);
void sw_wgrad_batch_free(sw_wgrad_batch* h);

int sw_social_pool_bwd(const float* obsv, int To, const float* h, const int* scene_off,
                       const long long* pair_off, int S, int B, int Amax, long long P,
                       const float* emb_w, const float* att_w, const float* attn, const float* dS,
                       float* dh, float* d_emb_w, float* d_att_w, float* pair_ws, float* wgrad_ws,
                       /* scenes above 64 agents (see sw_social_pool_fwd): the forward's big_blocks, wh_ws, ml, its
                        * output S_pool, and big_part_ws = 132 floats per partial row (blocks*agents rows per scene) */
                       const int* big_blocks /*or NULL*/, int NB, const float* wh_ws, const float* ml,
                       const float* S_pool, float* big_part_ws,
                       sw_wgrad_batch* defer /*NULL: reduce the weight gradients now; else leave the problems in the
                                               handle for the next sw_gen_wgrad on the same workspace*/,
                       void* stream);

/* sw_social_pool_bwd's per-pair-rows form followed by sw_enc_lstm_bwd_aux (dy, c0, dh0, dc0 NULL, t0 = 0) in ONE launch of a
 * workgroup per scene that keeps dh_T + its social gradient on chip: the same dgates rows, pair rows, agent rows and deferred
 * weight-gradient problems as the two launches; dhT is read, not updated.  For layouts in which every scene has at most 16
 * agents (Amax <= 16, no big_blocks), S <= sw_scene_wg_max_scenes(), and on which the two launches take the rows form
 * (0 < P < sw_social_rows_max_pairs() * S); SW_ESHAPE otherwise (the caller then issues the two launches).  scene_off must
 * tile [0, B).  aux_*: the masked copy of sw_enc_lstm_bwd_aux.                                                          */
int sw_scene_wg_max_scenes(void);
int sw_social_rows_max_pairs(void);
int sw_social_enc_bwd(const float* obsv, int To, const float* h, const int* scene_off, const long long* pair_off, int S, int B,
                      int Amax, long long P, const float* emb_w, const float* att_w, const float* attn, const float* dS,
                      const float* dhT, const float* dcT, float* d_emb_w, float* d_att_w, float* pair_ws, float* wgrad_ws,
                      const float* enc_w, const float* act, float* dgates, const float* aux_src, float* aux_dst,
                      const float* aux_mask, long long aux_n, sw_wgrad_batch* defer, void* stream);

/* ---- predict() decode loop (train.py:415-432): DecoderFC + position integration + the
 *      re-fed EncoderLstm step, Tp times, one persistent kernel (one workgroup per 16-agent tile; with the
 *      step's weight images registered and more than 256 tiles: per two tiles, the same body issuing every
 *      register-resident weight operand against both - the same results bit for bit) ------------------- */
int sw_dec_rollout_fwd(const float* obsv /*[B,To,2]*/, int To, const float* z /*[B,32]*/,
                       const float* S_pool /*[B,64] or NULL = zeros*/, const float* hT, const float* cT,
                       const float* enc_w, const float* dec_w, int B, int Tp,
                       float* pred4 /*[B,Tp,4]*/, float* h_end, float* c_end /*[B,64] or NULL*/,
                       float* gsave /*or NULL*/,
                       /* optional ADE/FDE partial sums of train.py:546-551, one triple per 16-agent tile
                        * (summed by the caller): { sum err / Tp, sum err[:, -1], sum err^2 },
                        * err = |(p_hat - gt) * inv_ss|; NULL to skip */
                       const float* gt /*[B,Tp,2]*/, float inv_ss, float* ade_part /*[ceil(B/16)][3]*/,
                       void* stream);
/* Same, plus (d_w, dsave non-NULL) the observation LSTM of Discriminator.forward (train.py:296-299) on the same
 * positions `obsv` with the packed D weights d_w, run by ceil(B/16) extra workgroups of the launch: the first D
 * pass of a training step (train.py:476-482) does not depend on the generator, and the rollout leaves CUs idle
 * for batches below ~2000 agents.  The LSTM rows land in `dsave` where sw_disc_fwd(save_lstm = 1) would put
 * them; the following sw_disc_fwd(obsv, x_mode = 0, same B / To / d_w, save_lstm = 2) reads them instead of
 * recomputing.                                                                                             */
int sw_dec_rollout_fwd_aux(const float* obsv, int To, const float* z, const float* S_pool, const float* hT,
                           const float* cT, const float* enc_w, const float* dec_w, int B, int Tp, float* pred4,
                           float* h_end, float* c_end, float* gsave, const float* gt, float inv_ss, float* ade_part,
                           const float* d_w /*or NULL*/, float* dsave /*or NULL*/, void* stream);
/* The SAMPLING form of the decode loop: K rollouts of B encoded agents in one launch (test(), train.py:563-616).
 * ROW ORDER: K*B rows, row r = k*B + a (k-major: copy k of agent a - the order of preds_our).  PER ROW: z and the
 * outputs.  PER AGENT (read at a = r % B, never replicated): obsv, S_pool, hT, cT, gt.  Row r equals row r of
 * sw_dec_rollout_fwd on inputs replicated K times, bit for bit.
 *   pred4  [K*B,Tp,4] or NULL (metrics only);
 *   err    [K*B][2] or NULL (needs gt): per row { mean over t of |(p_hat - gt) * inv_ss|, the same norm at step Tp-1 }
 *          (train.py:587, 602-607).  pred4 == NULL && err == NULL is SW_EARG.
 * Both tile forms of sw_dec_rollout_fwd (two tiles per workgroup above 256 tiles needs registered images).       */
int sw_dec_sample_fwd(const float* obsv /*[B,To,2]*/, int To, const float* z /*[K*B,32]*/,
                      const float* S_pool /*[B,64] or NULL = zeros*/, const float* hT, const float* cT /*[B,64]*/,
                      const float* enc_w, const float* dec_w, int B, int K, int Tp, float* pred4, const float* gt /*[B,Tp,2]*/,
                      float inv_ss, float* err, void* stream);
/* sw_dec_sample_fwd with RAGGED FUTURES: gt stays the dense [B,Tp,2] buffer, left-aligned; pred_len [B] int32 (read per
 * agent at a = r % B, like gt) gives the valid frames of row a, 1 .. Tp, the columns behind them are padding that no output
 * depends on (NaN included: selects, not products).  With e_t = |(p_hat_t - gt_t) * inv_ss| and n = pred_len[a]:
 *   err [K*B][2] = { (e_0 + .. + e_{n-1}) / (float)n, e_{n-1} }, summed over t ascending in fp32 as the dense launch sums:
 *                  a row of length n carries the bits of sw_dec_sample_fwd called with Tp = n on the first n frames of gt.
 * The rollout is untouched: every row runs all Tp steps and pred4 is the dense launch's bit for bit.  Errors are formed in
 * the launch (pred4 == NULL: no trajectory leaves the kernel).  The kernel clamps n into 1 .. Tp, so a bad device-side
 * length neither divides by zero nor reads past the row.  pred_len == NULL, or err == NULL (nothing for the lengths to
 * say): sw_dec_sample_fwd itself.  Checked before the device is touched: everything sw_dec_sample_fwd checks, with the
 * same codes.  Both tile forms; one owner per output, fixed order: two calls give the same bits.                     */
int sw_dec_sample_fwd_plen(const float* obsv /*[B,To,2]*/, int To, const float* z /*[K*B,32]*/,
                           const float* S_pool /*[B,64] or NULL = zeros*/, const float* hT, const float* cT /*[B,64]*/,
                           const float* enc_w, const float* dec_w, int B, int K, int Tp, float* pred4,
                           const float* gt /*[B,Tp,2]*/, const int* pred_len /*[B] int32 or NULL*/, float inv_ss, float* err,
                           void* stream);
/* Best-of-K reduction of err [K][B][2] (sw_dec_sample_fwd): per_agent [B][4] = { mean_k ADE, mean_k FDE, min_k ADE,
 * min_k FDE }, best [B] (int32, or NULL) = the k of the smallest ADE, the lowest k on ties.  Sums run over k ascending
 * in fp32 (s = s + e_k, then s / K): deterministic.  Sums over agents are the caller's (test() keeps them in float64). */
int sw_sample_reduce(const float* err /*[K,B,2]*/, int B, int K, float* per_agent /*[B,4]*/, int* best /*[B] or NULL*/,
                     void* stream);
/* Ranking of the K draws of every agent by a score (sw_disc_score; any [K,B] score works): order [B,M] int32,
 * order[a][m] = the draw with the (m+1)-th HIGHEST score of agent a - for the raw LSGAN score higher is more realistic
 * (targets 0 = generated, 1 = real; the optimal D is monotone in the density ratio).  Equal scores: the lowest k first,
 * as in sw_sample_reduce; the order is that of a stable descending sort.  1 <= M <= K <= 4096 (SW_ESHAPE above).
 * With err (the row errors [K,B,2] of sw_dec_sample_fwd), per_agent [B,5] = { ADE of order[a][0], FDE of order[a][0],
 * min over the top M of ADE, min over the top M of FDE, the 0-based rank of draw best[a] in the full descending order:
 * the number of k with score[k] > score[best], or == and k < best }.  best [B] = the min-ADE draw of sw_sample_reduce;
 * NULL (or an index outside 0 .. K-1): column 4 is 0.  per_agent needs err (SW_EARG).  Columns 0-3 are selections and
 * column 4 an integer count: no rounding anywhere, one owner per agent, two calls give the same bits.  Scores are
 * expected to be ordered (no NaN).                                                                                  */
int sw_sample_rank(const float* score /*[K,B]*/, const float* err /*[K,B,2] or NULL*/, const int* best /*[B] or NULL*/,
                   int B, int K, int M, int* order /*[B,M]*/, float* per_agent /*[B,5] or NULL*/, void* stream);
/* SCENE-LEVEL metrics of K joint draws (draw k of a scene = draw k of every agent in it).  B agents in S scenes,
 * scene_off [S+1] int32 prefix offsets (scene s = agents scene_off[s] .. scene_off[s+1]-1).
 *
 * sw_scene_clearance: clear [K,B], clear[k][a] = inv_ss * the closest approach of agent a to any other agent of its
 * scene in draw k; +inf for a single-agent scene or a path without segments.  The path of (k, a) is P_0 = start[a]
 * (when start != NULL), then pos[k][a][0 .. Tp-1]: Tp segments with start, Tp - 1 without.  Within a segment both agents
 * move linearly: r0 = P_{t-1}(a) - P_{t-1}(b), dv = (P_t(a) - P_t(b)) - r0, tau = clamp(-(r0.dv) / (dv.dv), 0, 1)
 * (0 when dv.dv = 0), distance |r0 + tau dv| - two agents that swap places inside a segment have distance 0.
 *   pos    [K,B,Tp,pstride], pstride 2 or 4 floats (x, y first; pred4 of sw_dec_sample_fwd has 4), 8-byte aligned;
 *   start  [B,sstride] or NULL, x, y first, sstride >= 2 (the last observed step of obsv [B,To,2]: obsv + 2*(To-1),
 *          sstride 2*To);  inv_ss > 0.
 * Plain trajectories in, so the same launch serves sampled futures, the ground truth (K = 1) and anything else.  Any
 * scene size: up to 32 agents a wave holds 64 / n_pad draws side by side, above 64 it loops over agent tiles.  Each
 * clear[k][a] has one owner (no atomics): deterministic.                                                           */
int sw_scene_clearance(const float* pos, int pstride, const float* start /*or NULL*/, int sstride, const int* scene_off,
                       int S, int B, int K, int Tp, float inv_ss, float* clear /*[K,B]*/, void* stream);
/* sw_scene_clearance with a LENGTH per agent: len [B] int32, the valid future frames of agent a, 1 .. Tp (clamped into
 * that range by the kernel), in every draw k; pos stays [K,B,Tp,pstride], left-aligned, and what lies behind a row's length
 * is padding no output depends on (NaN included).  A collision needs both agents present: in the clearance of pair (a, b)
 * the segment that ENDS at future frame t counts only if t < min(len[a], len[b]); segments run from t = 0 with a start
 * point, else from t = 1.  An agent for which no segment counts against any partner has clearance +inf, like a
 * single-agent scene.  r0 of a pair advances through every segment; only the minimum is gated.  All lengths n: the bits of
 * sw_scene_clearance on the paths cut to n frames.  len == NULL (= all Tp): sw_scene_clearance itself.  Checked before the
 * device is touched: everything sw_scene_clearance checks.  One owner per clear[k][a], no atomics: deterministic.    */
int sw_scene_clearance_len(const float* pos, int pstride, const float* start /*or NULL*/, int sstride, const int* scene_off,
                           const int* len /*[B] int32 or NULL*/, int S, int B, int K, int Tp, float inv_ss,
                           float* clear /*[K,B]*/, void* stream);
/* SCENE-CLEARANCE PENALTY of the generator loss and its gradient with respect to the positions: the training-side
 * counterpart of sw_scene_clearance - the same closest approach, squashed and differentiated.  B agents in S scenes
 * (scene_off as above), all fp32.  The path of agent a is P_a[0] = start[a] (when start != NULL), then pos[a][0 .. Tp-1]:
 * Tp segments with start, Tp - 1 without.  For two agents a != b of one scene and segment s (from point s-1 to point s):
 *   r0 = P_a[s-1] - P_b[s-1],  r1 = P_a[s] - P_b[s],  dv = r1 - r0,
 *   tau = clamp(-(r0.dv) / (dv.dv), 0, 1), tau = 0 when dv.dv = 0      (the arithmetic of sw_scene_clearance),
 *   c = r0 + tau dv,  u = max(0, 1 - |c|^2 / d0^2),  phi = u^2.
 * The penalty of the batch is the sum over scenes, pairs a < b and segments of phi.  tau minimises |r0 + tau dv|^2 over
 * [0, 1], so d|c|^2 / dP_a[s] = 2 tau c and d|c|^2 / dP_a[s-1] = 2 (1 - tau) c, and with d phi / d|c|^2 = -2 u / d0^2
 *   g_a[s] = sum over b != a of [ -(4 u_s / d0^2) tau_s c_s - (4 u_{s+1} / d0^2) (1 - tau_{s+1}) c_{s+1} ]
 * (the second term absent at the last point).  phi is C1 at the threshold |c| = d0 (u reaches 0 there, and g with it); g
 * is continuous across both clamps of tau (inside, c is orthogonal to dv; at a clamp the formula holds with the clamped tau),
 * finite everywhere, and exactly 0 where c = 0 - coincident agents are not pushed apart: a saddle of measure zero.  Its only
 * discontinuity is at dv.dv = 0, where tau = 0 is the definition.
 *   pos    [B,Tp,pstride], pstride 2 or 4 floats (x, y first), 8-byte aligned;  start [B,sstride] or NULL, sstride >= 2;
 *   d0 > 0 and finite, in the units of pos;  scale finite;
 *   dpos   [B,Tp,dstride], dstride 2 or 4, 8-byte aligned: dpos[a][t][0:2] += scale * g of the point pos[a][t]; components
 *          2 and 3 of a 4-float row are neither read nor written.  With start, P[0] is data and takes no gradient; without,
 *          pos[a][0] takes its share as the r0 end of segment 1;
 *   loss   [B] or NULL: loss[a] = 1/2 * the sum over b != a and s of phi - unscaled, the agent's share: the sum over a of
 *          loss[a] is the penalty;   count [B] int32 or NULL: the number of (b, s) with |c|^2 < d0^2.
 * STORES ARE SKIPPED, not +0: per agent and chunk of 16 segments, the dpos rows of the chunk are read and written only if
 * one of its (b, s) has |c|^2 < d0^2.  An agent whose every |c|^2 >= d0^2, and any agent of a single-agent scene, leaves
 * its dpos rows bit for bit as they were (loss 0, count 0).  Rows outside every scene are not written.
 * One wave per (scene, tile of 64 agents), one owner per dpos row, loss[a] and count[a], partners then segments in ascending
 * order, no atomics: two calls give the same bits, and a scene's outputs do not depend on the other scenes of the batch.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, dpos, scene_off; S < 0; B < 0; Tp < 1; d0 <= 0
 * or not finite (or d0^2 or 1 / d0^2 outside fp32's range); scale not finite; pstride or dstride not 2 or 4; pos or dpos off their
 * 8-byte alignment; start with sstride < 2.  B == 0 or S == 0: SW_OK without a launch.                                 */
int sw_clearance_grad(const float* pos, int pstride, const float* start /*or NULL*/, int sstride, const int* scene_off,
                      int S, int B, int Tp, float d0, float scale, float* dpos /*[B,Tp,dstride], += */, int dstride,
                      float* loss /*[B] or NULL*/, int* count /*[B] or NULL*/, void* stream);
/* sw_scene_reduce: with sade[k][s] / sfde[k][s] = the mean over the scene's agents of err[k][a][0] / [1] and
 * sclear[k][s] = the minimum over them of clear[k][a],
 *   per_scene [S,6] = { min_k sade, min_k sfde, share of k with sclear < coll_dist, 1 if draw kbest collides else 0,
 *                       min_k sclear, mean over (k, a in s) of [clear[k][a] < coll_dist] },
 *   best [S] (int32, or NULL) = kbest = the first k that attains min_k sade.
 * clear == NULL, and every single-agent scene: columns 2, 3, 5 are 0 and column 4 is +inf.  Fixed summation order: two
 * calls give the same bits.                                                                                          */
int sw_scene_reduce(const float* err /*[K,B,2]*/, const float* clear /*[K,B] or NULL*/, const int* scene_off, int S, int B,
                    int K, float coll_dist, float* per_scene /*[S,6]*/, int* best /*[S] or NULL*/, void* stream);
/* DIVERSE top-M of K draws: greedy non-maximum suppression in score order, and the share of the K draws behind every kept
 * mode.  A GROUP is a scene (scene_off [S+1] as above: its rows scene_off[s] .. scene_off[s+1]-1, G = S groups) or, with
 * scene_off == NULL, a single row (G = B).  All fp32:
 *   d_a(j,k)  between draws j and k of row a: metric 0 ("fde") inv_ss * the Euclidean distance at step Tp-1; metric 1 ("ade")
 *             inv_ss * the mean over the Tp steps of that distance (summed over t ascending, divided by Tp);
 *   D_g(j,k)  = the maximum over the rows a of group g of d_a(j,k): two joint futures are one mode only if every agent agrees;
 *   s_g(k)    = the minimum over the rows of g of score[k][a]: a joint future is as realistic as its least realistic agent.
 * Both are selections: no sum over agents, no order dependence (over no rows: s_g = +inf, D_g = 0).  The loop: all K draws
 * start alive; for m = 0 .. M-1, unless none is alive, the pick c_m is the alive draw with the largest s_g (the lowest k of
 * equal ones), and every alive k with D_g(k, c_m) <= radius - c_m among them - is removed with assign[k] = m.  count[g] =
 * the number of picks.  Draws that are still alive then (only with count == M) get assign[k] = the m with the smallest
 * D_g(k, c_m), the lowest m of equal ones.
 *   pos     [K,B,Tp,pstride], pstride 2 or 4 floats, x and y first (pred4 of sw_dec_sample_fwd, read where it lies), 8-byte
 *           aligned;  score [K,B] (sw_disc_score; ordered, no NaN);  1 <= M <= K <= 4096;  inv_ss > 0;  radius >= 0 in the
 *           units of inv_ss * distance;
 *   order   [G,M] int32: c_m, -1 from count[g] on;   count [G] int32;   assign [G,K] int32;
 *   weight  [G,M]: #{k : assign[k] == m} / K, one integer-to-float division, 0 from count[g] on; every row sums to 1;
 *   per_row [B,6] or NULL, needs err [K,B,2] (the row errors of sw_dec_sample_fwd, 8-byte aligned): for row a of group g
 *           { ADE of draw c_0, FDE of draw c_0, min over the picks of ADE, of FDE, weight[g][assign[g][best[a]]],
 *           (float) assign[g][best[a]] } - best [B] int32 = the min-ADE draw of sw_sample_reduce; NULL or an index outside
 *           0 .. K-1: columns 4 and 5 are 0.  Rows outside every scene are not written.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, score, order, count, weight, assign; B < 0;
 * K < 1; M < 1 or M > K; Tp < 1; pstride not 2 or 4; metric not 0 or 1; radius < 0 or NaN; inv_ss <= 0 or NaN; per_row without
 * err; scene_off with S < 0; pos or err off their 8-byte alignment.  SW_ESHAPE: K > 4096.  B == 0 (or no scenes): SW_OK
 * without a launch.  One wave per group, one writer per output element, no atomics: two calls give the same bits.
 * LDS per workgroup: 4 * (6 * roundup(K, 8) + 2 * roundup(M, 8)) bytes, 131 072 at K = M = 4096.                        */
int sw_sample_nms(const float* pos, int pstride, const float* score /*[K,B]*/, const int* scene_off /*[S+1] or NULL*/, int S,
                  int B, int K, int Tp, int M, int metric, float inv_ss, float radius, const float* err /*[K,B,2] or NULL*/,
                  const int* best /*[B] or NULL*/, int* order /*[G,M]*/, int* count /*[G]*/, float* weight /*[G,M]*/,
                  int* assign /*[G,K]*/, float* per_row /*[B,6] or NULL*/, void* stream);
/* COMPOSED joint future of a scene: one draw PER AGENT.  Given the observations the K draws of different agents are
 * independent (the social block runs once, on the observations; row (k, a) of the rollout reads z[k][a] and the encoding of
 * agent a alone), so every tuple (k_a) of per-agent draws is as much a joint sample as the diagonal (k, .., k) that
 * sw_scene_clearance / sw_scene_reduce look at.  Per scene this picks the tuple the score prefers, moved away from it only
 * where two chosen paths would come closer than coll_dist.  All fp32; agents a, b are rows of one scene (scene_off as above).
 *   path of (k, a)   as in sw_scene_clearance: start[a] first when start != NULL, then pos[k][a][0 .. Tp-1];
 *   c(a,j; b,k)      = sqrtf(m) * inv_ss, m = the minimum over the countable segments of the squared closest approach of
 *                    path (j, a) to path (k, b), each segment with the arithmetic of sw_scene_clearance operation for
 *                    operation (r0, dv, tau = clamp(-(r0.dv) / (dv.dv), 0, 1), 0 when dv.dv = 0, |r0 + tau dv|^2).  With len
 *                    [B] int32 (clamped into 1 .. Tp) the segment that ends at future frame t counts only while
 *                    t < min(len[a], len[b]) - the rule of sw_scene_clearance_len; what lies behind a length, NaN included,
 *                    reaches nothing.  +inf when no segment counts.  Exactly symmetric: c(a,j; b,k) = c(b,k; a,j);
 *   conflict         c < coll_dist, the comparison sw_scene_reduce applies to clear.
 * The selection, per scene, its agents a = 0 .. n-1 in ascending row order:
 *   sel0[a] = the draw with the highest score[k][a], the lowest k of equal ones (order[a][0] of sw_sample_rank); sel = sel0;
 *   conf_a(j) = the number of agents b != a of the scene with c(a,j; b,sel[b]) in conflict;
 *   up to `sweeps` sweeps; in a sweep, for a = 0 .. n-1 in order: if conf_a(sel[a]) == 0 nothing happens; else with j* = the
 *   draw that minimises (conf_a(j), -score[j][a], j) lexicographically, sel[a] = j* if conf_a(j*) < conf_a(sel[a]) - seen by
 *   the agents after a in the same sweep - and sel[a] stays otherwise.  Every change lowers the number of conflicting pairs
 *   of the scene by at least one, so the loop ends; it stops after the first sweep in which nothing changed.
 * Outputs:  sel [B] int32, sel0 [B] int32 (or NULL);
 *   clear [B]        clear[a] = the minimum over b != a of c(a,sel[a]; b,sel[b]), +inf in a single-agent scene: the bits of
 *                    sw_scene_clearance(_len) with K = 1 on the selected paths;
 *   per_scene [S,4]  int32 { conflicting pairs under sel0, conflicting pairs under sel, agents with sel != sel0, sweeps in
 *                    which some agent changed };
 *   per_row [B,4]    or NULL, needs err [K,B,2] (the row errors of sw_dec_sample_fwd, 8-byte aligned):
 *                    { ADE, FDE of draw sel0[a], ADE, FDE of draw sel[a] }.
 * Rows outside every scene are not written; a scene whose offsets leave 0 .. B reads nothing and has per_scene 0.  Scores are
 * expected to be ordered (no NaN).  coll_dist == 0 admits no conflict: sel == sel0.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, score, scene_off, sel, clear, per_scene; S < 0;
 * B < 0; K < 1; Tp < 1; sweeps < 1; pstride not 2 or 4; pos or err off their 8-byte alignment; start with sstride < 2;
 * inv_ss <= 0 or NaN; coll_dist < 0 or NaN; per_row without err.  SW_ESHAPE: K > 4096.  B == 0 or S == 0: SW_OK without a
 * launch.  One 256-thread workgroup per scene, any scene size and any Tp; one writer per output element, integer conflict
 * counts, no atomics: two calls give the same bits.  The n^2 K^2 table of clearances is never formed.
 * LDS per workgroup: min(8 256 + roundup(4 B, 16) + 8 B ((Tp + [start != NULL]) | 1), 65 536) bytes - 8 192 for a batch of one
 * agent's candidate paths, the rest for the selection and the selected paths of a scene (at most B agents); a scene whose
 * paths do not fit reads them from global memory instead.                                                            */
int sw_scene_compose(const float* pos, int pstride, const float* start /*or NULL*/, int sstride,
                     const float* score /*[K,B]*/, const int* scene_off /*[S+1]*/, const int* len /*[B] or NULL*/,
                     int S, int B, int K, int Tp, float inv_ss, float coll_dist, int sweeps,
                     const float* err /*[K,B,2] or NULL*/,
                     int* sel /*[B]*/, int* sel0 /*[B] or NULL*/, float* clear /*[B]*/,
                     int* per_scene /*[S,4]*/, float* per_row /*[B,4] or NULL*/, void* stream);
/* PLAN RISK: candidate ego paths - paths that are NOT rows of pos - scored against the K sampled futures of a scene: how
 * likely is a plan to come closer than coll_dist to somebody?  pos, start, scene_off, len, inv_ss and the path of (k, a) are
 * exactly as in sw_scene_clearance_len.  The draws are open-loop: the pedestrians do not react to the plan.  A QUERY q names
 * a scene q_scene[q] (int32), an ego row q_ego[q] to leave out - an ABSOLUTE row of the batch; q_ego == NULL, -1 or a row
 * outside the scene leaves nobody out - and P candidate plans: plan (q, p) is plan_start[q] first when there is a start point
 * (plan_start != NULL iff start != NULL), then plans[q][p][0 .. Tp-1] (x, y; 8-byte aligned).  Several queries may name one
 * scene; leave-one-out is Q = B.  All fp32; "agent a" below is a row of the scene other than the ego row.
 *   d(q,p; k,a; t)   = sqrtf(m) * inv_ss, m = the squared closest approach of plan (q, p) and path (k, a) within the segment
 *                    that ENDS at future frame t, with the arithmetic of sw_scene_clearance operation for operation: r0 = the
 *                    agent's point minus the plan's point at the segment's first end, r1 the same at its second end,
 *                    dv = r1 - r0, tau = clamp(-(r0.dv) / (dv.dv), 0, 1), 0 when dv.dv = 0, m = |r0 + tau dv|^2; r0 advances
 *                    through every segment.  Segments run from t = 0 with a start point, else from t = 1.  The segment counts
 *                    only while t < min(len[a], plan_len[q]), both clamped into 1 .. Tp, NULL meaning Tp; what lies behind a
 *                    length, NaN included, reaches nothing (the minimum is gated by a select).
 *   c(q,p; k,a)      = the minimum over the counted segments of d, +inf when none counts.  A conflict is c < coll_dist, the
 *                    fp32 comparison sw_scene_reduce makes; sqrtf and the multiplication are monotone, so a path conflicts
 *                    iff one of its counted segments has d < coll_dist.
 *   h_a(q,p)         = the number of draws k in which path (k, a) conflicts with plan (q, p), 0 .. K.
 * Outputs, per (q, p):
 *   clear_min        = the minimum over the agents a and the draws k of c; +inf with no other agent or no counted segment;
 *   counts[0]        = the number of draws k in which SOME agent's draw k conflicts: the index-paired estimate of the risk is
 *                    counts[0] / K;
 *   counts[1]        = the frame t at which the earliest conflicting counted segment over all (a, k) ends, -1 if none;
 *   counts[2]        = the absolute row a with the largest h_a, the lowest row of equal ones, -1 if every h_a is 0;
 *   counts[3]        = that row's h_a (0 if none);
 *   risk             = 1 - prod over the agents a of f_a, f_a = (float)(K - h_a) / (float)K: one fp32 IEEE division per agent,
 *                    fp32 products taken over the agents in ascending row order starting from 1.0f (a factor f_a = 1 leaves the
 *                    bits as they are), one fp32 subtraction.  Given the observations the draws of different agents are
 *                    independent (see sw_scene_compose), so the product is the share of ALL K^n tuples of per-agent draws in
 *                    which the plan hits somebody; the index-paired counts[0] / K looks
 *                    at K of them.  risk is exactly 0 when every h_a is 0, exactly 1 when some h_a = K, and within
 *                    2 (n + 1) 2^-24 of the exact product otherwise (n divisions, n - 1 products and one subtraction on
 *                    values in [0, 1]: a rounding bound).
 * A query whose scene index lies outside 0 .. S-1 or whose offsets leave 0 .. B reads nothing and writes risk 0, clear_min
 * +inf, counts {0, -1, -1, 0}; so does a scene without rows.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, scene_off, plans, q_scene, risk, clear_min,
 * counts; plan_start NULL with start non-NULL or the other way round; S, B or Q < 0; K, Tp or P < 1; pstride not 2 or 4; pos
 * or plans off their 8-byte alignment; start with sstride < 2; inv_ss <= 0 or NaN; coll_dist < 0 or NaN.  SW_ESHAPE: K > 4096.
 * Q == 0: SW_OK without a launch.
 * One 256-thread workgroup per (query, tile of up to 64 plans - fewer with few queries, so that the launch fills the device);
 * a lane owns an (agent, draw) pair and walks the tile's plans.
 * One writer per output element; what is accumulated across lanes is an integer (counts, bit masks, the first frame) or a
 * minimum, through LDS integer atomics whose result does not depend on the order: two calls give the same bits.  LDS per
 * workgroup: at most 65 536 bytes - per plan of the tile 8 (Tp + [start != NULL]) for its points, 8, 4 ceil(K / 32) and
 * 4 ((256 / min(K, 256)) | 1); the tile shrinks until it fits, and a plan that does not fit alone is read where it lies.   */
int sw_plan_risk(const float* pos, int pstride, const float* start /*or NULL*/, int sstride,
                 const int* scene_off /*[S+1]*/, const int* len /*[B] or NULL*/, int S, int B, int K, int Tp,
                 const float* plans /*[Q,P,Tp,2]*/, const float* plan_start /*[Q,2]; NULL iff start == NULL*/,
                 const int* plan_len /*[Q] or NULL*/, const int* q_scene /*[Q]*/, const int* q_ego /*[Q] or NULL*/,
                 int Q, int P, float inv_ss, float coll_dist,
                 float* risk /*[Q,P]*/, float* clear_min /*[Q,P]*/, int* counts /*[Q,P,4]*/, void* stream);
/* PLAN REFINEMENT: the question behind sw_plan_risk turned round - not "how likely is this plan to run into somebody" but
 * "which plan near it is not": n_iter steps of gradient descent on the expected clearance penalty of a plan against the K
 * sampled futures of a scene, all inside one launch.  pos, start, scene_off, len, inv_ss, the path of (k, a), the queries
 * (q_scene, q_ego: which rows of which scene count as "agent a") and the layout of plans / plan_start are exactly as in
 * sw_plan_risk, except that a start point is REQUIRED on both sides (start and plan_start non-NULL) and that there is no
 * plan_len.  The draws are open-loop: the pedestrians do not react to the plan.  All fp32.
 * For one (query q, plan p) the WAYPOINTS are X = (x_1 .. x_T), T = Tp, x_t = plans[q][p][t-1] on entry (X0, kept); x_0 =
 * plan_start[q] is data and never moves.  The pedestrian path of (k, a) is A_0 = start[a], A_s = pos[k][a][s-1].  The objective:
 *   J(X) = pen(X) + (w_track / d0^2) trk(X) + (w_smooth / d0^2) smo(X),
 *   pen(X) = (1 / K) * sum over the agents a of the query, the draws k < K and the segments s = 1 .. min(T, len[a]) of phi,
 *            (len clamped into 1 .. Tp, NULL meaning Tp) with, for segment s (from point s-1 to point s),
 *              r0 = A_{s-1} - x_{s-1},  r1 = A_s - x_s  (pedestrian minus plan),  dv = r1 - r0,
 *              tau = clamp(-(r0.dv) / (dv.dv), 0, 1), tau = 0 when dv.dv = 0     (the arithmetic of sw_scene_clearance),
 *              c = r0 + tau dv,  u = max(0, 1 - |c|^2 / d0^2),  phi = u^2        (the penalty of sw_clearance_grad);
 *   trk(X) = sum over t = 1 .. T of |x_t - x0_t|^2;
 *   smo(X) = sum over t = 1 .. T-1 of |acc_t|^2,  acc_t = x_{t+1} - 2 x_t + x_{t-1}  (acc_1 reads x_0; none for T = 1).
 * Given the observations the draws of different agents are independent (sw_scene_compose), so pen is the expectation of the
 * penalty over all K^n joint futures.  Its gradient (tau minimises |r0 + tau dv|^2 over [0, 1], see sw_clearance_grad; the
 * sign turns because r is pedestrian minus plan):
 *   d phi / d x_s = (4 u / d0^2) tau c,   d phi / d x_{s-1} = (4 u / d0^2) (1 - tau) c   (nothing for x_0);
 *   d trk / d x_t = 2 (x_t - x0_t);   d smo / d x_t = 2 (acc_{t-1} - 2 acc_t + acc_{t+1}),  acc_i = 0 outside 1 .. T-1.
 * One ITERATION, all waypoints at once from the same X:
 *   step_t = lr d0^2 dJ/dx_t = lr [ (1 / K) sum of 4 u {tau | 1 - tau} c  +  2 w_track (x_t - x0_t)  +  2 w_smooth (acc_{t-1} - 2 acc_t + acc_{t+1}) ];
 *   if |step_t| > max_move d0:  step_t = step_t * (max_move d0 / |step_t|);      x_t = x_t - step_t.
 * Descent moves the plan away from the pedestrians.  With this scaling lr, w_track, w_smooth and max_move are dimensionless;
 * on the quadratic part alone the iteration is stable for lr (2 w_track + 32 w_smooth) < 2 (the acceleration operator's largest
 * eigenvalue is 16) and free of overshoot below 1; not checked here: the Python layers refuse what is not stable.
 * Outputs, per (q, p), after n_iter iterations:
 *   out   [Q,P,Tp,2]  the refined waypoints;  n_iter = 0 copies plans bit for bit;
 *   cost  [Q,P,2,3]   { pen, trk / d0^2, smo / d0^2 } of X0 (row 0; trk is exactly 0) and of the refined plan (row 1),
 *                     unweighted; with n_iter = 0 the two rows carry the same bits;
 *   moved [Q,P]       inv_ss * the largest |x_t - x0_t| over t.
 * Gating is by select: the ego row, segments behind len[a] and whatever they hold - NaN included - reach no output.  A query
 * whose scene index lies outside 0 .. S-1 or whose offsets leave 0 .. B, and a scene with nobody but the ego, take no penalty
 * (pen = 0); the quadratic terms still act.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, start, scene_off, plans, plan_start, q_scene,
 * out, cost, moved; S, B or Q < 0; K, Tp or P < 1; pstride not 2 or 4; pos or plans off their 8-byte alignment; sstride < 2;
 * inv_ss <= 0 or NaN; n_iter outside 0 .. 1024; d0 <= 0 or not finite (or d0^2 or 1 / d0^2 outside fp32's range); lr,
 * w_track, w_smooth or max_move negative or not finite.  SW_ESHAPE: K > 4096 or Tp > 1024.  Q == 0: SW_OK without a launch.
 * One 256-thread workgroup per (query, plan); a lane owns an (agent, draw) pair as in sw_plan_risk and keeps its path in
 * registers across the iterations when the scene is one lane batch and the path one time chunk; X, X0 and the per-wave
 * partial gradients live in LDS (56 (Tp + 2) + 16 bytes).  Every sum across lanes is taken in a fixed order (a fixed tree inside
 * the wave, then waves 0 .. 3) and there are no atomics: two calls give the same bits, and the result of a (query, plan)
 * does not depend on the other queries, plans or scenes of the batch.                                                   */
int sw_plan_refine(const float* pos, int pstride, const float* start /*[B,sstride]*/, int sstride,
                   const int* scene_off /*[S+1]*/, const int* len /*[B] or NULL*/, int S, int B, int K, int Tp,
                   const float* plans /*[Q,P,Tp,2]*/, const float* plan_start /*[Q,2]*/, const int* q_scene /*[Q]*/,
                   const int* q_ego /*[Q] or NULL*/, int Q, int P, float inv_ss, float d0, int n_iter, float lr,
                   float w_track, float w_smooth, float max_move,
                   float* out /*[Q,P,Tp,2]*/, float* cost /*[Q,P,2,3]*/, float* moved /*[Q,P]*/, void* stream);
/* WALLS: the static map of a recording - walls, kerbs, benches - as M line segments, one set per call (one recording has one
 * map).  walls [M,2,2] fp32 holds the segments [w0, w1] in the coordinates of the trajectories and plans (normalised ones);
 * inv_ss turns a distance into the units of `dist`, as everywhere else.  M = 0 is allowed (walls may then be NULL); a wall of
 * zero length is a post; M <= SW_WALLS_MAX, so that the set fits LDS (16 bytes per wall) next to what the refinement holds.
 * CLOSEST APPROACH of a moving point to a wall within one segment: the path point moves linearly from p0 to p1, the wall is
 * static.  e = p1 - p0, f = w1 - w0, a x b = a.x b.y - a.y b.x.  Five candidates (s, c) - s in [0, 1] the place on the path
 * segment, c the path point minus the wall point - tried in this order; the first is the best so far, a later one replaces
 * the best only if its |c|^2 is STRICTLY smaller (a NaN compares false and replaces nothing):
 *   1. s = 0:  c = p0 - (w0 + u f),  u = clamp((p0 - w0).f / |f|^2, 0, 1), u = 0 when |f|^2 = 0;
 *   2. s = 1:  the same with p1;
 *   3. the end w0 against the path:  s = clamp((w0 - p0).e / |e|^2, 0, 1), s = 0 when |e|^2 = 0,  c = p0 + s e - w0;
 *   4. the end w1 likewise;
 *   5. a proper crossing:  d1 = f x (p0 - w0), d2 = f x (p1 - w0), d3 = e x (w0 - p0), d4 = e x (w1 - p0); if d1, d2 have
 *      strictly opposite signs and d3, d4 have strictly opposite signs:  c = 0, |c|^2 = 0, s = d1 / (d1 - d2).
 * Touching and collinear contact reach distance 0 through candidates 1 - 4.  The reciprocals of |f|^2, |e|^2 and d1 - d2 are
 * the hardware's (1 ulp), as in sw_scene_clearance: u and s only place a point on a segment.
 * PENALTY of a (path segment, wall) pair at the distance dw:  u = max(0, 1 - |c|^2 / dw^2),  phi = u^2, counted where
 * |c|^2 < dw^2.  By the envelope argument of sw_clearance_grad (the candidate's free parameter minimises |c|^2):
 *   d phi / d p1 = -(4 u / dw^2) s c,    d phi / d p0 = -(4 u / dw^2) (1 - s) c.
 * phi is C1 at |c| = dw and the gradient is finite everywhere.  It is exactly 0 where the path crosses the wall (c = 0):
 * descent cannot undo a crossing - crossings are reported (sw_path_walls), not repaired.  Where two candidates tie - a path
 * parallel to a wall - |c|^2 is unique but s is not: the order above decides which end point takes the gradient, while the
 * sum over both end points, -(4 u / dw^2) c, does not depend on it.  This discontinuity is the twin of the "pair without
 * relative motion" one (tau = 0 when dv.dv = 0).                                                                         */
#define SW_WALLS_MAX 1024
/* PATH WALLS: the clearance of R = K B paths to the walls in one launch.  pos, pstride, start, sstride, the path of (k, a) and
 * len are as in sw_scene_clearance_len: with a start point (start != NULL) the path has Tp segments and segment j (from point
 * j to point j + 1) ends at future frame j, without one Tp - 1 segments and segment j ends at frame j + 1; a segment counts
 * only while its frame t < len[a] (clamped into 1 .. Tp, NULL meaning Tp), and what lies behind a length, NaN included,
 * reaches nothing (every contribution is gated by a select).  Per path (k, a), over its counted segments and all M walls:
 *   clear [K,B]        inv_ss * sqrtf(the smallest |c|^2); +inf with M = 0 or nothing counted;
 *   first [K,B] int32  the frame at which the first segment with a wall closer than dist ends, -1 if none;
 *   nseg  [K,B] int32  the number of (segment, wall) pairs closer than dist.
 * "Closer" is the fp32 comparison sqrtf(|c|^2) * inv_ss < dist, as in sw_plan_risk.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, clear, first, nseg, or walls with M > 0; K < 1;
 * B < 0; Tp < 1; M < 0; pstride not 2 or 4; pos off its 8-byte alignment; start with sstride < 2; inv_ss <= 0 or NaN; dist < 0
 * or NaN.  SW_ESHAPE: M > SW_WALLS_MAX.  B == 0: SW_OK without a launch.
 * One 256-thread workgroup per 64 paths: a lane owns a path, its points in registers; the four waves take the wall slices
 * w, w + 4, ... of the same 64 paths, the walls read from LDS as the wave-uniform partner.  What is accumulated is a minimum
 * and two integers, folded over the waves in the order 0 .. 3; no atomics: two calls give the same bits.                  */
int sw_path_walls(const float* pos, int pstride, const float* start /*[B,sstride] or NULL*/, int sstride,
                  const int* len /*[B] or NULL*/, int K, int B, int Tp, const float* walls /*[M,2,2]*/, int M,
                  float inv_ss, float dist, float* clear /*[K,B]*/, int* first /*[K,B]*/, int* nseg /*[K,B]*/, void* stream);
/* PLAN REFINEMENT WITH WALLS: sw_plan_refine with one more term in the objective,
 *   J(X) = pen(X) + (w_track / d0^2) trk(X) + (w_smooth / d0^2) smo(X) + w_wall wal(X),
 *   wal(X) = the sum over the plan's segments s = 1 .. T (from x_{s-1} to x_s; x_0 = plan_start is data) and the M walls of
 *            phi at the distance dw (WALLS above) - no 1 / K: the walls are certain.
 * The iteration is sw_plan_refine's with the wall gradient inside the step,
 *   step_t = lr [ (1 / K) sum 4 u {tau | 1 - tau} c  +  w_wall (d0^2 / dw^2) sum over the walls of -4 u_w ( s c of segment t
 *            + (1 - s) c of segment t + 1 )  +  2 w_track (x_t - x0_t)  +  2 w_smooth (acc_{t-1} - 2 acc_t + acc_{t+1}) ],
 * capped at max_move d0 as before; the wall term is added last, to the sum sw_plan_refine forms.  The stability rule is unchanged: the wall term is bounded and not quadratic.
 * cost is [Q,P,2,4]: the three columns of sw_plan_refine, then wal, unweighted.  n_iter = 0 returns the plans' bits; M = 0
 * returns, bit for bit, what sw_plan_refine returns in out, moved and the first three cost columns, and wal = 0.
 * Checked before the device is touched: everything sw_plan_refine checks, and SW_EARG: M < 0; walls NULL with M > 0; dw <= 0
 * or not finite (or dw^2 or 1 / dw^2 outside fp32's range); w_wall negative or not finite, or w_wall d0^2 / dw^2 not
 * finite.  SW_ESHAPE: M > SW_WALLS_MAX.
 * The same kernel as sw_plan_refine, instantiated with the wall evaluation: per iteration the workgroup's threads take
 * (wall slice, plan segment) pairs - 256 / Tp slices, a slice the walls c, c + 256 / Tp, ... - and the slices are added in
 * ascending order: every sum in a fixed order, no atomics, two calls give the same bits, a plan's result independent of
 * the rest of the batch.  LDS: sw_plan_refine's, rounded up to 16, + 16 M + 16 (max(256 / Tp, 1) Tp + 1) bytes - 90 256 at
 * Tp = 1024, M = 1024, inside the 160 KB of a CU.                                                                        */
int sw_plan_refine_walls(const float* pos, int pstride, const float* start /*[B,sstride]*/, int sstride,
                         const int* scene_off /*[S+1]*/, const int* len /*[B] or NULL*/, int S, int B, int K, int Tp,
                         const float* plans /*[Q,P,Tp,2]*/, const float* plan_start /*[Q,2]*/, const int* q_scene /*[Q]*/,
                         const int* q_ego /*[Q] or NULL*/, int Q, int P, float inv_ss, float d0, int n_iter, float lr,
                         float w_track, float w_smooth, float max_move, const float* walls /*[M,2,2]*/, int M, float dw,
                         float w_wall, float* out /*[Q,P,Tp,2]*/, float* cost /*[Q,P,2,4]*/, float* moved /*[Q,P]*/,
                         void* stream);
/* WALL PENALTY of the generator loss and its gradient with respect to the positions: the training-side counterpart of
 * sw_path_walls, as sw_clearance_grad is that of sw_scene_clearance.  R = K B paths against the M walls of the call, all fp32.
 * Paths, segments and the gating by len are those of sw_path_walls: with a start point (start != NULL) the path of (k, a) has
 * Tp segments, without one Tp - 1; a segment counts only while its frame t < len[a] (clamped into 1 .. Tp, NULL meaning Tp),
 * and what lies behind a length, NaN included, reaches nothing (every contribution goes through a select).
 * Per counted (segment, wall) pair: (s, c, |c|^2) are those of the CLOSEST APPROACH above (one device function, shared with
 * sw_path_walls and sw_plan_refine_walls) and nothing else;  u = max(0, 1 - |c|^2 / dw^2),  phi = u^2;  the pair is COUNTED
 * where |c|^2 < dw^2.  dw is in the units of pos, like d0 of sw_clearance_grad.
 *   dpos   [K,B,Tp,dstride], dstride 2 or 4, 8-byte aligned:  dpos[r][t][0:2] += scale * g_t,
 *            g_t = sum over the walls of [ -(4 u / dw^2) s c of the segment that ends at point t
 *                                          -(4 u / dw^2) (1 - s) c of the segment that starts at point t ]
 *          (each over counted pairs only).  With start, the start point is data and takes nothing; without, pos[.][0] takes
 *          the (1 - s) share of segment 1.  Components 2 and 3 of a 4-float row are neither read nor written;
 *   pos    [K,B,Tp,pstride], pstride 2 or 4 floats (x, y first), 8-byte aligned;  start [B,sstride] or NULL, sstride >= 2;
 *   loss   [K,B] or NULL: loss[r] = the sum of phi over the path's counted pairs, unscaled - no 1/2: a path owns its pairs alone;
 *   count  [K,B] int32 or NULL: the number of counted pairs.
 * phi is C1 at |c| = dw, the gradient finite everywhere and exactly 0 where the path crosses the wall (c = 0); where two
 * candidates tie the order of the candidates decides which end point takes the gradient (WALLS above).
 * STORES ARE SKIPPED, not +0: per path and chunk of 16 segments, the dpos rows of the chunk are read and written only if one
 * of its (segment, wall)s is counted, and then only the rows of points a counted segment can reach (none behind len).  A
 * path with count == 0 leaves its dpos rows bit for bit as they were, and so does every path when M = 0: M = 0 returns SW_OK,
 * writes loss 0 and count 0 and touches no dpos.
 * One 256-thread workgroup per 64 paths, a lane per path, the four waves taking the wall slices w, w + 4, ..; a wave adds its
 * walls, then the chunk's segments, in ascending order, the waves' partial sums are added in the order 0 .. 3 and wave 0 makes
 * the one read-modify-write of a chunk's rows (the point two chunks share: twice by the same thread, in chunk order).  One
 * owner per dpos row, loss[r] and count[r], no atomics; the order in which a point's contributions are added depends on
 * (Tp, M) only, never on K, B or the grid: two calls give the same bits, and a path's outputs do not depend on the rest of
 * the batch.  LDS: 16 KB of walls + 3 * 64 * 17 * 8 bytes of partial sums + 1.5 KB.
 * Checked before the device is touched - SW_EARG: a NULL pointer among pos, dpos, or walls with M > 0; K < 1; B < 0; Tp < 1;
 * M < 0; dw <= 0 or not finite (or dw^2 or 1 / dw^2 outside fp32's range); scale not finite; pstride or dstride not 2 or 4;
 * pos or dpos off their 8-byte alignment; start with sstride < 2.  SW_ESHAPE: M > SW_WALLS_MAX.  B == 0: SW_OK without a
 * launch.                                                                                                                */
int sw_wall_grad(const float* pos, int pstride, const float* start /*[B,sstride] or NULL*/, int sstride,
                 const int* len /*[B] or NULL*/, int K, int B, int Tp, const float* walls /*[M,2,2]*/, int M,
                 float dw, float scale, float* dpos /*[K,B,Tp,dstride], += */, int dstride,
                 float* loss /*[K,B] or NULL*/, int* count /*[K,B] or NULL*/, void* stream);
/* GRID: sw_path_walls and sw_wall_grad for a map of any size - M has no cap but int32 - whose walls stay in global memory under
 * a uniform grid (socialways_amd.WallGrid builds and validates it on the host): nx x ny square cells of edge 1 / inv_cell, cell
 * (ix, iy) covering [x0 + ix cell, x0 + (ix + 1) cell) x [y0 + iy cell, ...), nx ny <= 2^20;
 *   wall_cells [M,4] int32   (ix0, iy0, ix1, iy1): the cell range of wall m's bounding box, clamped into the grid;
 *   cell_ptr [nx ny + 1], cell_walls [cell_ptr[nx ny]] int32: cell c = iy nx + ix lists cell_walls[cell_ptr[c] .. cell_ptr[c + 1])
 *              = the walls whose range holds (ix, iy) - wall m is listed in EVERY cell of its range - in ascending order;
 *   reach      the largest distance, in the coordinates of the walls, a call may ask about.
 * Paths, segments, start, the gating by len, the thresholds and the outputs are those of the flat entries; the pair arithmetic
 * is the CLOSEST APPROACH above and nothing else, the decisions are the flat kernels' expressions |c|^2 < dw^2 and
 * sqrtf(|c|^2) * inv_ss < dist.  What differs is which pairs are looked at:
 * QUERY RANGE of a counted segment p0 -> p1: the cell range of its bounding box inflated by reach,
 *   floor((min(p0.x, p1.x) - reach - x0) / cell) .. floor((max(p0.x, p1.x) + reach - x0) / cell), likewise in y, formed in fp32
 *   as c = ((v -+ reach) - x0) * inv_cell and widened by the slack 2^-21 (|c| + |x0| inv_cell) on either side - twice the bound
 *   4 u |c| + u |x0| / cell, u = 2^-24, of the three roundings and of inv_cell - c itself held inside +-2^22 before the slack, so that it stays finite - then clamped to 0 .. nx - 1; empty when it
 *   lies wholly outside the grid or a bound is NaN.  The clamps come before the float-to-int conversion: NaN or huge points
 *   index nothing out of range.  The cells are walked row-major (iy outer, ix inner), a cell's list in ascending order.
 * VISIT-ONCE RULE: wall m is visited in cell (ix, iy) only if ix == max(wall_cells[m].ix0, qx0) and iy == max(wall_cells[m].iy0,
 *   qy0) - the first cell of the intersection of the two ranges.  A wall within reach of the segment has a bounding box that
 *   meets the inflated box of the segment, so the two ranges intersect and their first common cell lists the wall: every pair
 *   with |c|^2 < reach^2 is visited exactly once, no pair twice, whatever the cell size.
 * REFUSED (SW_EARG): dw, or dist / inv_ss, that is not <= reach (1 - 1e-5); the margin covers the rounding of the square root
 *   and the product, so that every pair a decision can count is a visited one.
 * OUTPUTS: nseg, first and count are the flat entries' numbers.  loss and dpos are the flat entries' sums over the same counted
 *   pairs in another fixed order - segments ascending, within a segment the walls in the order of the walk, phi summed per
 *   segment and then added - so they agree with the flat entries to rounding, not bit for bit.  The one documented difference is
 *   clear: inv_ss * sqrtf(the smallest visited |c|^2) if that is below reach^2, else +inf - it does not depend on the cells -
 *   where the flat call reports the distance to the nearest wall however far.  Stores are skipped as in sw_wall_grad.
 * A lane owns a path, its points and gradient accumulators of a time chunk in registers; walls are read from global memory as
 * float4 (walls and wall_cells on 16-byte boundaries); no LDS, no barrier, no atomics, one owner per output row: two calls give
 * the same bits and a path's outputs do not depend on the rest of the batch.  Every loop is bounded by the clamped ranges and
 * by cell_ptr; what the index arrays hold is the builder's to validate.
 * Checked before the device is touched - SW_EARG: everything the flat entry refuses of its other arguments; M < 0; cell_ptr
 * NULL; walls, cell_walls or wall_cells NULL with M > 0; walls or wall_cells off a 16-byte boundary; nx or ny < 1 or
 * nx ny > 2^20; x0, y0 not finite; inv_cell not finite or <= 0; reach (or its square) not finite or <= 0; the refusal above.
 * M = 0 is legal (a 1 x 1 grid with an empty list).  B == 0: SW_OK without a launch.                                          */
int sw_path_walls_grid(const float* pos, int pstride, const float* start /*[B,sstride] or NULL*/, int sstride,
                       const int* len /*[B] or NULL*/, int K, int B, int Tp, const float* walls /*[M,2,2]*/, int M,
                       const int* cell_ptr /*[nx ny + 1]*/, const int* cell_walls /*[L]*/, const int* wall_cells /*[M,4]*/,
                       int nx, int ny, float x0, float y0, float inv_cell, float reach,
                       float inv_ss, float dist, float* clear /*[K,B]*/, int* first /*[K,B]*/, int* nseg /*[K,B]*/, void* stream);
int sw_wall_grad_grid(const float* pos, int pstride, const float* start /*[B,sstride] or NULL*/, int sstride,
                      const int* len /*[B] or NULL*/, int K, int B, int Tp, const float* walls /*[M,2,2]*/, int M,
                      const int* cell_ptr /*[nx ny + 1]*/, const int* cell_walls /*[L]*/, const int* wall_cells /*[M,4]*/,
                      int nx, int ny, float x0, float y0, float inv_cell, float reach,
                      float dw, float scale, float* dpos /*[K,B,Tp,dstride], += */, int dstride,
                      float* loss /*[K,B] or NULL*/, int* count /*[K,B] or NULL*/, void* stream);
int sw_dec_rollout_bwd(const float* dpred4 /*[B,Tp,4]*/, const float* enc_w, const float* dec_w,
                       const float* gsave, int B, int To, int Tp, float* gdelta,
                       float* dhT, float* dcT, float* dS_pool /*[B,64]*/, void* stream);
/* Same, plus an auxiliary masked copy aux_dst[i] = aux_mask[i] > 0 ? aux_src[i] : aux_dst[i] (aux_n floats) done by
 * extra workgroups of the launch (idle CUs): the training step's D.load(backup) (train.py:541-542).          */
int sw_dec_rollout_bwd_aux(const float* dpred4, const float* enc_w, const float* dec_w, const float* gsave, int B,
                           int To, int Tp, float* gdelta, float* dhT, float* dcT, float* dS_pool,
                           const float* aux_src, float* aux_dst, const float* aux_mask, long long aux_n, void* stream);
/* weight gradients of the whole generator rollout (encoder + decoder) from gsave/gdelta.
 * part 0 = all; 1 = what dec_rollout_bwd produced (decoder layers + LSTM rows t >= To); 2 = LSTM rows
 * t < To (after enc_lstm_bwd) accumulated onto part 1, then the embed / W_ih split.  Parts 1 and 2
 * may run on different streams with different `wgrad_ws`; `tmp` (2048 floats) links them.        */
int sw_gen_wgrad(const float* enc_w, const float* dec_w, const float* gsave, const float* gdelta, const float* z,
                 const float* S_pool, int B, int To, int Tp, float* d_enc_w, float* d_dec_w, int part,
                 float* wgrad_ws, float* tmp /*[2048]*/,
                 sw_wgrad_batch* pending /*or NULL: problems deferred by sw_social_pool_bwd join this launch*/,
                 void* stream);
/* sw_gen_wgrad(part 0) that ALSO applies the generator's Adam update (train.py:539 `predictor_optimizer.step()`,
 * torch's fused Adam restated like sw_disc_bwd_gan_adam): every generator gradient is finished either by the
 * reduction of the grouped GEMM or by the composition kernel behind it, and the thread that finishes an element
 * updates exp_avg / exp_avg_sq / the weight.  adam_w / adam_m / adam_v / adam_g = the packed weight, moment and
 * gradient buffers of the WHOLE generator (adam_n floats each, one layout; enc_w, dec_w, d_enc_w, d_dec_w and the
 * pending problems' outputs point into them); adam_step = device scalar, 1-based index of the update.  Needs
 * the weight images of this step (sw_gen_images / sw_stage_step_img: the compositions read their step-start
 * snapshot while live weights are overwritten), else SW_EARG.  Single process only: a data-parallel job
 * all-reduces between gradient and update.                                                                */
int sw_gen_wgrad_adam(const float* enc_w, const float* dec_w, const float* gsave, const float* gdelta,
                      const float* z, const float* S_pool, int B, int To, int Tp, float* d_enc_w, float* d_dec_w,
                      float* wgrad_ws, float* tmp /*[2048]*/, sw_wgrad_batch* pending /*or NULL*/, float* adam_w,
                      float* adam_m, float* adam_v, const float* adam_g, long long adam_n, const float* adam_step,
                      double lr, double beta1, double beta2, double eps, void* stream);

/* ---- Discriminator.forward (train.py:294-309) for nb prediction branches sharing one
 *      observation encoding (fake / real of the same batch) ----------------------------------- */
/* x_mode 0: obsv = positions [B,To,2] (4-d state formed on the fly); 1: obsv = obsv_4d [B,To,4].   */
int sw_disc_fwd(const float* obsv, int To, int x_mode, const float* const* pred4 /*nb x [B,Tp,4]*/,
                int nb, const float* d_w, int B, int Tp, float* const* label /*nb x [B,1]*/,
                float* const* code /*nb x [B,2]*/, float* dsave /*or NULL*/,
                int save_lstm /*0: head activations only - enough for a backward that wants d/dpred only; 1: + the
                                LSTM rows; 2: the LSTM rows are ALREADY in dsave (sw_dec_rollout_fwd_aux): the
                                observation LSTM is not run again, h_T is read from them*/,
                float* w_snapshot /*or NULL: receives a copy of d_w (sw_param_count floats) - deepcopy(D), train.py:499*/,
                void* stream);
/* dlabel/dcode: nb x gradients of the loss w.r.t. label / code.  d_d_w NULL = skip weight grads
 * (generator phase), dpred4[k] NULL = skip input grad of branch k.                              */
int sw_disc_bwd(const float* d_w, const float* dsave, const float* const* dlabel,
                const float* const* dcode, int nb, int B, int To, int Tp, float* ddelta,
                float* d_d_w, float* const* dpred4, float* wgrad_ws, void* stream);

/* Same backward with the LSGAN / InfoGAN loss gradients formed inside the kernel from the forward
 * outputs: dlabel_k = 2 (label_k - targets[t_k]) g_label, dcode_0 = 2 (code_0 - z[:, :2]) g_code,
 * dcode_1 = 0 (train.py:484-494, 512-523) - no separate loss kernel on the critical path.          */
int sw_disc_bwd_gan(const float* d_w, const float* dsave, const float* const* label,
                    const float* const* code, const float* targets, int t0, int t1, const float* z /*[B,32]*/,
                    float g_label, float g_code, int nb, int B, int To, int Tp, float* ddelta,
                    float* d_d_w, float* const* dpred4, float* wgrad_ws,
                    float* loss_part /*[ceil(B/16)][3] or NULL: per-tile sums {(label_0-t0)^2, (code_0-z)^2,
                                       (label_1-t1)^2}, the reported MSE terms; column 2 untouched if nb == 1*/,
                    void* stream);
/* The same with the discriminator's Adam update (train.py:384-385: lr, betas, eps; no weight decay) applied by the
 * kernel that finishes the gradients: every discriminator parameter is an output of that reduction, so its thread
 * updates exp_avg, exp_avg_sq and the weight right there - operation for operation torch's fused Adam
 * (fused_adam_utils.cuh) - and the optimizer's own launch disappears.  adam_w must be d_w (the packed weights the pass
 * just read: all of its readers are behind kernel boundaries), adam_m / adam_v the packed moments, adam_step a device
 * scalar holding the 1-based index of this update.  adam_w = NULL: plain sw_disc_bwd_gan.  Single process only: data
 * parallel ranks all-reduce the gradients between this call and their optimizer step.                             */
int sw_disc_bwd_gan_adam(const float* d_w, const float* dsave, const float* const* label, const float* const* code,
                         const float* targets, int t0, int t1, const float* z, float g_label, float g_code, int nb,
                         int B, int To, int Tp, float* ddelta, float* d_d_w, float* const* dpred4, float* wgrad_ws,
                         float* loss_part, float* adam_w, float* adam_m, float* adam_v, const float* adam_step,
                         double lr, double beta1, double beta2, double eps, void* stream);

/* ---- one discriminator UPDATE pass in one launch (train.py:476-495): sw_disc_fwd(nb = 2: fake, real; x_mode 0;
 *      save_lstm = obs_pre ? 2 : 1; w_snapshot) + sw_disc_bwd_gan[_adam](no d/dpred) fused per 16-agent tile - forward,
 *      LSGAN / InfoGAN loss gradients, backward, the two branches' heads side by side on the two wave pairs - followed by
 *      the weight-gradient GEMM (and the Adam update when adam_w = d_w).  Same buffers, same rows, same arguments as the
 *      two calls.  sw_disc_update_supported() says whether this (d_w with registered images - sw_disc_images -,
 *      Tp <= 12; any B) can run; SW_ESHAPE otherwise.                                                                */
int sw_disc_update_supported(const float* d_w, int B, int To, int Tp);
int sw_disc_update(const float* obsv /*[B,To,2]*/, int To, const float* const* pred4 /*2 x [B,Tp,4]*/, const float* d_w, int B,
                   int Tp, float* const* label, float* const* code, float* dsave, int obs_pre, float* w_snapshot /*or NULL*/,
                   const float* targets, int t0, int t1, const float* z, float g_label, float g_code, float* ddelta,
                   float* d_d_w, float* wgrad_ws, float* loss_part /*or NULL*/, float* adam_w /*or NULL*/, float* adam_m,
                   float* adam_v, const float* adam_step, double lr, double beta1, double beta2, double eps, void* stream);
/*      sw_disc_update_ragged = sw_disc_update over RAGGED observation histories: what sw_disc_fwd_ragged(nb = 2, x_mode 0,
 *      save_lstm 1) followed by sw_disc_bwd_gan[_adam] computes, into the same buffers, bit for bit.  Row b holds
 *      clamp(obs_len[b], 2, To) valid frames right-aligned in obsv; the padding is never read.  sw_disc_update's arguments
 *      without obs_pre (ragged rows have no precomputed observation pass), obs_len (B int32, device) behind To; a NULL
 *      obs_len is SW_EARG, a shape outside sw_disc_update_supported() SW_ESHAPE.                                       */
int sw_disc_update_ragged(const float* obsv /*[B,To,2]*/, int To, const int* obs_len /*[B]*/, const float* const* pred4, const float* d_w,
                          int B, int Tp, float* const* label, float* const* code, float* dsave, float* w_snapshot /*or NULL*/,
                          const float* targets, int t0, int t1, const float* z, float g_label, float g_code, float* ddelta,
                          float* d_d_w, float* wgrad_ws, float* loss_part /*or NULL*/, float* adam_w /*or NULL*/, float* adam_m,
                          float* adam_v, const float* adam_step, double lr, double beta1, double beta2, double eps, void* stream);

/* ---- generator phase in one launch (train.py:510-523, 538): D forward on (obsv, pred_hat) fused with the backward of
 *      its prediction heads: dpred4 = d(g_loss)/d(pred_hat) with g_loss = mse(label, targets[t_idx]) +
 *      w mse(code, z[:, :2]) expressed through g_label = 1/B_global, g_code = w/(2 B_global).  No saves; label / code /
 *      loss_part ([ceil(B/16)][3]: columns 0, 1 = per-tile sums of the squared errors) are optional outputs.
 *      LDS per workgroup: the forward carve behind the observation LSTM's tiles plus the backward's transposed head
 *      images and delta tiles, 4 352 B more per 4 steps of Tp: 146 688 B at Tp = 12, 159 744 B at Tp = 24, 164 096 B at
 *      Tp = 25 - over the 163 840 B limit, so this and sw_dec_rollout_bwd_dfuse return SW_ESHAPE for Tp = 25 .. 64.
 *      sw_disc_dpred_supported(Tp) says whether they run; otherwise sw_disc_fwd + sw_disc_bwd_gan (nb = 1, dpred4) give
 *      the same d/dpred and loss sums.                                                                              */
int sw_disc_dpred_supported(int Tp);
int sw_disc_dpred(const float* obsv, int To, int x_mode, const float* pred4 /*[B,Tp,4]*/, const float* d_w, int B, int Tp,
                  const float* targets, int t_idx, const float* z /*[B,32]*/, float g_label, float g_code,
                  float* dpred4 /*[B,Tp,4]*/, float* label /*[B,1] or NULL*/, float* code /*[B,2] or NULL*/,
                  float* loss_part /*or NULL*/, void* stream);

/* ---- Discriminator.forward on K sampled futures per agent in one launch: the scoring twin of sw_dec_sample_fwd.
 *      ROW ORDER: K*B rows, row r = k*B + a (the layout of sw_dec_sample_fwd's pred4).  PER ROW: pred4, score, code.
 *      PER AGENT (read at a, never replicated): obsv - positions [B,To,2] (x_mode 0) or obsv_4d [B,To,4] (x_mode 1).
 *        score [K*B]          the raw LSGAN score (higher = more realistic);
 *        code  [K*B,2] or NULL  the InfoGAN head's estimate of the latent code z[:, :2] behind the draw.
 *      score[k*B + a] / code[k*B + a] are the bits sw_disc_fwd(nb = 1) writes to label[a] / code[a] given
 *      pred4 + k*B*Tp*4, with and without registered weight images (sw_disc_images): every row passes through the same
 *      product chains in the same order.  Grid: ceil(B/16) tiles x k-groups workgroups; a workgroup runs the observation
 *      LSTM and fc of its tile ONCE and the prediction heads for the draws of its k-range, two draws side by side on
 *      its two wave pairs.  Every k-group repeats the observation pass, so their number is chosen from what is
 *      there - min(CUs of the device / tiles, ceil(K/2)), at least 1: a small chunk fills the chip, a large one runs the
 *      LSTM once per tile.  No save buffers, no atomics, one owner per output: deterministic.
 *      SW_EARG: a NULL pointer (code may be NULL), K < 1, B < 0, To < 1, Tp < 1, x_mode not 0 / 1, To < 2 with x_mode 0;
 *      SW_ESHAPE: Tp > 64.  B == 0: SW_OK without a launch.  LDS per workgroup: 89 600 B at Tp = 12, 149 504 B at 64.   */
int sw_disc_score(const float* obsv, int To, int x_mode, const float* pred4 /*[K*B,Tp,4]*/, const float* d_w, int B, int K,
                  int Tp, float* score /*[K*B]*/, float* code /*[K*B,2] or NULL*/, void* stream);

/* sw_disc_score with the ragged observation pass of sw_enc_lstm_fwd_ragged: obsv right-aligned, obs_len int32 [B] on the
 * device (2 <= n <= To for positions, 1 <= n <= To for obsv_4d; clamped on the device; the padding is never read), row a's
 * observation LSTM starts from the zero state at step To - obs_len[a].  score[k*B + a] / code[k*B + a] are the bits
 * sw_disc_score gives agent a on the [1, n_a, .] buffer of its valid frames and its draws.  Same grid and k-group rule,
 * same LDS, same argument checks, same behaviour with and without sw_disc_images; a kernel of its own (sw_disc_score's
 * is unchanged).  obs_len == NULL: every row has To frames - sw_disc_score's bits.                                       */
int sw_disc_score_ragged(const float* obsv, int To, int x_mode, const int* obs_len /*[B] int32 or NULL = all To*/,
                         const float* pred4 /*[K*B,Tp,4]*/, const float* d_w, int B, int K, int Tp, float* score /*[K*B]*/,
                         float* code /*[K*B,2] or NULL*/, void* stream);

/* ---- the discriminator's training passes over RAGGED observation histories ---------------------------------------------
 * sw_disc_fwd / sw_disc_dpred with obs_len [B] (int32 on the device, NULL = every row has To frames; clamped on the device
 * into 2 .. To for positions, 1 .. To for obsv_4d) between x_mode and pred4: obsv is right-aligned, row a's observation
 * LSTM runs from the zero state over its obs_len[a] valid frames alone and the padding is never read.  label / code /
 * dpred4 / the saved head activations of agent a carry the bits of the dense entry on the [1, n_a, .] buffer of its valid
 * frames (an agent is one column of every product).  The LSTM rows of the save buffer (save_lstm = 1) follow
 * sw_enc_lstm_fwd_ragged_save: the dense entry's bits from step To - n_a on, all-zero rows and inputs in front of it, so
 * sw_disc_bwd* run on the buffer unchanged and give the ragged gradients.  Same grid rule, LDS, argument checks and
 * behaviour with and without sw_disc_images as the dense entries; a kernel of its own (disc_fwd_kernel is unchanged).
 * sw_disc_fwd_ragged takes save_lstm 0 or 1 only: 2 is SW_EARG, there is no precomputed observation pass for ragged rows.
 * sw_disc_dpred_ragged needs sw_disc_dpred_supported(Tp) like sw_disc_dpred (SW_ESHAPE otherwise).
 * B == 0: SW_OK without a launch.                                                                                          */
int sw_disc_fwd_ragged(const float* obsv, int To, int x_mode, const int* obs_len /*[B] int32 or NULL = all To*/,
                       const float* const* pred4 /*nb x [B,Tp,4]*/, int nb, const float* d_w, int B, int Tp,
                       float* const* label /*nb x [B,1]*/, float* const* code /*nb x [B,2]*/, float* dsave /*or NULL*/,
                       int save_lstm /*0 or 1*/, float* w_snapshot /*or NULL*/, void* stream);
int sw_disc_dpred_ragged(const float* obsv, int To, int x_mode, const int* obs_len /*[B] int32 or NULL = all To*/,
                         const float* pred4 /*[B,Tp,4]*/, const float* d_w, int B, int Tp, const float* targets, int t_idx,
                         const float* z /*[B,32]*/, float g_label, float g_code, float* dpred4 /*[B,Tp,4]*/,
                         float* label /*[B,1] or NULL*/, float* code /*[B,2] or NULL*/, float* loss_part /*or NULL*/,
                         void* stream);

/* ---- LSGAN + InfoGAN losses of train.py:484-494 / 512-523 and their gradients -------------- */
/* t_a = targets[ia], t_b = targets[ib] (read on the device, so a captured hipGraph sees new values).
 * out_sums[3] = { sum (label_a - t_a)^2, sum (code_a - z[:, :2])^2, sum (label_b - t_b)^2 } over the
 * B local rows (label_b may be NULL).  Gradients (any may be NULL):
 *   dlabel_x = 2 (label_x - t_x) g_label,  dcode_a = 2 (code_a - z) g_code,  dcode_b = 0
 * with g_label = 1/B_global and g_code = loss_info_w / (2 B_global) for a mean over the global
 * batch (data-parallel ranks pass the GLOBAL batch size so summed gradients are exact).
 * `scratch` (3*SW_RED_BLOCKS floats, optional): with it, large batches are reduced by up to
 * SW_RED_BLOCKS workgroups and a fixed-order second stage; NULL keeps the one-workgroup path.   */
#define SW_RED_BLOCKS 64
int sw_gan_loss(const float* label_a, const float* targets /*device [>=2]: label-noise scalars*/, int ia,
                const float* code_a, const float* z /*[B,32]*/, const float* label_b, int ib, int B,
                float g_label, float g_code, float* out_sums /*[3]*/, float* dlabel_a, float* dcode_a,
                float* dlabel_b, float* dcode_b, float* scratch /*[3*SW_RED_BLOCKS] or NULL*/, void* stream);

/* ---- optional L2 term of the generator loss (train.py:512,525-526; the "variety" term as written in
 *      train.py:527-536 is the same expression restricted to one agent row):
 *      dpred4[b][t][0:2] += scale * (pred4_hat[b][t][0:2] - gt[b][t][:]) for rows b in [row0,row1).
 *      L2: rows [0,B), scale = loss_l2_w / (B_global * Tp).  Called after sw_disc_bwd_gan wrote dpred4. */
int sw_l2_grad(const float* pred4_hat /*[B,Tp,4]*/, const float* gt /*[B,Tp,2]*/, int B, int Tp, int row0, int row1,
               float scale, float* dpred4 /*[B,Tp,4]*/, void* stream);

/* ---- variety loss with its INTENDED semantics (train.py:527-536 is buggy as written - see SURVEY 0.x / DESIGN):
 *      K rollouts with independent z folded into one batch (copy k = rows [k*B,(k+1)*B)); per agent the copy with
 *      the smallest mean squared error receives dpred4[k*B+b][t][0:2] += scale * (p_hat - p), scale =
 *      loss_l2_w / (B_global * Tp).  kmin [B] (int32) / l2min [B] (the per-agent minimum, for the reported loss)
 *      may be NULL.  K <= 64 (SW_ESHAPE above).                                                              */
int sw_variety_grad(const float* pred4_hat_K /*[K*B,Tp,4]*/, const float* gt /*[B,Tp,2]*/, int K, int B, int Tp,
                    float scale, float* dpred4_K /*[K*B,Tp,4]*/, int* kmin, float* l2min, void* stream);

/* ---- toy statistics (calc_statistics.py:7-66): the O(K^2) distance loops of compute_1nn /
 *      compute_wasserstein.  D[k][i][j] = mean over t in [t0,T) of ||a[i][k][t] - b[j][k][t]||.        */
int sw_traj_dist(const float* a /*[Na,nPed,T,2]*/, const float* b /*[Nb,nPed,T,2]*/, int Na, int Nb, int nPed, int T,
                 int t0, float* D /*[nPed,Na,Nb]*/, void* stream);

/* ---- input staging of a hipGraph-replayed step, one kernel with fixed arguments.  `slot` = host-pinned
 *      (device-mapped) words the host rewrites before each replay: [0,1] device pointer of obsv (B,To,2),
 *      [2,3] device pointer of pred (B,Tp,2), [4] zeros_val, [5] ones_val, [6] / [7] number of D / G Adam
 *      updates applied so far, [8..] z (B*32).
 *      Writes the static buffers of the graph: tracks, real future as (p,v) rows (train.py:135-137),
 *      label-noise scalars, z (z_dst may be NULL: fetched elsewhere) and (steps_dst != NULL) the 1-based Adam step indices of this step's
 *      n_d_updates discriminator updates followed by the generator update. -------------------------- */
#define SW_STAGE_HEADER 8
int sw_stage_step(const float* slot, int B, int To, int Tp, float* obsv_dst /*[B,To,2]*/, float* pred_dst /*[B,Tp,2]*/,
                  float* pred4_dst /*[B,Tp,4]*/, float* targets_dst /*[2]*/, float* z_dst /*[B,32]*/,
                  float* steps_dst /*[n_d_updates+1] or NULL*/, int n_d_updates, void* stream);

/* ---- derived weight images of the generator.  Every workgroup of the encoder / decode launches needs the composed input
 *      matrix W_ih W_embed (train.py:266-268: no non-linearity between embed and the LSTM), fc4 . fc3 and every weight
 *      matrix (transposed in the backward pass) as MFMA A operands.  sw_gen_images derives them ONCE into img
 *      (sw_gen_image_floats() floats) - the compositions, a step-start snapshot of the raw weights behind them, and
 *      OPERAND-LAYOUT images (a wave's operand load = 1 KB of consecutive memory instead of 64 cache-line accesses) -
 *      and REGISTERS them for (enc_w, dec_w) and, when given, for the social block's (emb_w, att_w): until the
 *      registration is dropped, sw_enc_lstm_fwd*, sw_dec_rollout_fwd*, sw_dec_rollout_bwd*, sw_social_pool_fwd/bwd
 *      called with these weight buffers load the images instead of deriving / gathering per workgroup (same values bit
 *      for bit).  The images are valid while the weights are unchanged: the caller drops the registration -
 *      sw_gen_images(NULL, NULL, NULL, NULL, NULL, NULL) - before it updates them.  Registrations (these and
 *      sw_disc_images') are per HOST THREAD: register, launch and drop on the thread that steps the trainer.
 *      sw_stage_step_img = sw_stage_step whose launch derives and registers the images as well (no extra launch).   */
int sw_gen_image_floats(void);
int sw_gen_images(const float* enc_w, const float* dec_w, const float* emb_w /*or NULL*/, const float* att_w /*or NULL*/,
                  float* img, void* stream);
int sw_stage_step_img(const float* slot, int B, int To, int Tp, float* obsv_dst, float* pred_dst, float* pred4_dst,
                      float* targets_dst, float* z_dst, float* steps_dst, int n_d_updates, const float* enc_w,
                      const float* dec_w, const float* emb_w /*or NULL*/, const float* att_w /*or NULL*/, float* img,
                      /* d_img != NULL: the launch also scatters and registers the discriminator's images (sw_disc_images) */
                      const float* d_w /*or NULL*/, float* d_img /*or NULL*/, const int* d_tab /*or NULL*/, void* stream);
/*      sw_stage_step_zdev = sw_stage_step_img for a caller whose z (train.py:473) already lives in device memory
 *      (z_device = 1): slot words [8,9] then hold the device pointer of z (B,32) instead of its values, z_dst is required
 *      and filled from there - no PCIe read of z inside the step (4 MB at 32 768 agents).                               */
int sw_stage_step_zdev(const float* slot, int B, int To, int Tp, float* obsv_dst, float* pred_dst, float* pred4_dst,
                       float* targets_dst, float* z_dst, float* steps_dst, int n_d_updates, const float* enc_w,
                       const float* dec_w, const float* emb_w, const float* att_w, float* img, const float* d_w, float* d_img,
                       const int* d_tab, int z_device, void* stream);

/*      sw_stage_step_ragged = sw_stage_step_zdev for a captured step over RAGGED observation histories, with a slot layout
 *      of its own: words [0..7] as above, [8,9] the device pointer of z when z_device = 1, [10,11] the device pointer of this
 *      step's obs_len (B int32, contiguous), z values from word SW_STAGE_HEADER_RAGGED on when z_device = 0.  It writes what
 *      sw_stage_step_zdev writes and obs_len_dst[i] = clamp(obs_len[i], 2, To), the static buffer the graph's ragged kernels
 *      read.  z_dst and obs_len_dst are required (SW_EARG): the ragged encoder launch pulls no z, so this launch fills z
 *      in both z modes.                                                                                                   */
#define SW_STAGE_HEADER_RAGGED 12
int sw_stage_step_ragged(const float* slot, int B, int To, int Tp, float* obsv_dst, float* pred_dst, float* pred4_dst,
                         float* targets_dst, float* z_dst, float* steps_dst, int n_d_updates, const float* enc_w,
                         const float* dec_w, const float* emb_w, const float* att_w, float* img, const float* d_w, float* d_img,
                         const int* d_tab, int z_device, int* obs_len_dst /*[B]*/, void* stream);

/* ---- derived weight images of the DISCRIMINATOR (Discriminator.forward, train.py:294-309, as the kernels consume it):
 *      MFMA A-operand images of lstm.weight_hh and its transpose, and the eight head matrices transposed and zero-padded
 *      exactly as the backward kernels keep them in LDS (their prologue becomes one contiguous copy).  D's weights change
 *      three times per training step (two Adam updates, D.load(backup)), so the images are maintained element-wise through
 *      a table: sw_disc_image_table(Tp, tab) fills HOST memory with 2 ints per packed float (sw_param_count(SW_GRP_DISC, Tp)
 *      pairs): its image offsets, -1 = none.  sw_disc_images(d_w, img, tab_device, Tp, stream) scatters the whole packed
 *      buffer into img (sw_disc_image_floats(Tp) floats, ZERO-FILLED by the caller once - padding is never written) and
 *      REGISTERS (img, tab) for d_w: until the registration is dropped - sw_disc_images(NULL, NULL, NULL, 0, NULL) -
 *      sw_disc_fwd / sw_disc_dpred / sw_disc_bwd* called with these weights and this Tp read the images, and
 *      sw_disc_bwd_gan_adam / sw_adam_packed keep them current while they update the weights.  Whoever changes the
 *      weights by other means re-scatters or drops the registration.  Same values bit for bit either way.           */
int sw_disc_image_floats(int Tp);
int sw_disc_image_table(int Tp, int* tab_host);
int sw_disc_images(const float* d_w, float* img, const int* tab, int Tp, void* stream);

/* ---- GENERIC-WIDTH path: the per-layer pieces from which socialways_amd/generic.py runs the same model for any
 *      `--hidden-size` (train.py:42-44, 76-81: encoder / social-feature / discriminator widths H, noise H/2) and any
 *      latent-code count (train.py:65).  The fused kernels above hold a 64-unit layer per workgroup in registers and are
 *      the path of every BASELINE config; H > 64 or n_latent_code != 2 run layer by layer through these entry points
 *      plus sw_rows_gemm / sw_linear_wgrad - same mathematics, launch-bound.  All buffers row-major fp32.        */
/* nn.LSTM cell, element-wise part: pre [B][4H] = gate pre-activations (i | f | g | o blocks); gates receives the
 * activated gates, c / h [B][H] the new state; c_prev NULL = zeros.  Backward: dpre [B][4H], dc_prev [B][H] from
 * dh / dc (either may be NULL = zeros).                                                                       */
int sw_lstm_point_fwd(const float* pre, const float* c_prev, int B, int H, float* gates, float* c, float* h, void* stream);
int sw_lstm_point_bwd(const float* gates, const float* c, const float* c_prev, const float* dh, const float* dc, int B,
                      int H, float* dpre, float* dc_prev, void* stream);
/* kind 0: ReLU, 1: LeakyReLU(0.2) (train.py:181-188, 280-292, 324-328); the backward takes the activated values */
int sw_act_fwd(const float* x, long long n, int kind, float* y, void* stream);
int sw_act_bwd(const float* y, const float* dy, long long n, int kind, float* dx, void* stream);
/* sum over an [R][C] block of (a - b)^2 (b NULL: the scalar target[target_idx], read on the device) into out_sum[0]
 * (or NULL), and da = gscale (a - b) (or NULL): the pieces of nn.MSELoss and its gradient (train.py:484-494, 512-523) */
int sw_sqdiff(const float* a, int lda, const float* b, int ldb, const float* target, int target_idx, long long R, int C,
              float gscale, float* out_sum, float* da, int ldda, void* stream);
/* SocialFeatures (train.py:208-241) on the ordered in-scene pairs only: feat [P][4] = (dist, bearing, dca, 0) at row
 * pair_off[s] + i_local n + j_local (pair_off as for sw_social_pool_bwd); x4_last [B][4] = last observed (p, v)   */
int sw_pair_features(const float* x4_last, const int* scene_off, const long long* pair_off, int S, float* feat, void* stream);
/* AttentionPooling (train.py:153-175) on pair rows f [P][F] with wh = W h + b [B][F], h [B][H]: attn [P] receives the
 * softmax weights, S_out [B][H] the pooled states.  Backward: dsig [P] scratch, df [P][F] (or NULL), dwh [B][F] =
 * dL/d(wh), dh [B][H] = sum_i a_ij dS_i (the caller adds the W^T dwh term and forms dW, db).                    */
int sw_attn_pairs_fwd(const float* f, const float* wh, const float* h, const int* scene_off, const long long* pair_off, int S,
                      int B, int F, int H, float* attn, float* S_out, void* stream);
int sw_attn_pairs_bwd(const float* f, const float* wh, const float* h, const float* attn, const float* dS, const int* scene_off,
                      const long long* pair_off, int S, int B, int F, int H, float* dsig, float* df, float* dwh, float* dh,
                      void* stream);

/* ---- Adam on a packed buffer (train.py:379-385: lr, betas, eps; no weight decay), torch's fused Adam restated operation
 *      by operation (the arithmetic of sw_disc_bwd_gan_adam / sw_gen_wgrad_adam as a kernel of its own): the optimizer
 *      step of data-parallel ranks, whose gradients pass through an all-reduce first.  step = device scalar, 1-based
 *      index of the update.  disc_Tp > 0: w is the packed Discriminator and its registered images (sw_disc_images)
 *      follow the update; 0 otherwise.                                                                          */
int sw_adam_packed(float* w, const float* g, float* m, float* v, long long n, const float* step, double lr, double beta1,
                   double beta2, double eps, int disc_Tp, void* stream);

/* sw_enc_lstm_bwd with the masked copy of sw_dec_rollout_bwd_aux (dst[i] = mask[i] > 0 ? src[i] : dst[i]) done by extra
 * workgroups of the launch                                                                                            */
int sw_enc_lstm_bwd_aux(const float* enc_w, const float* act, const float* c0, const float* dhT, const float* dcT,
                        const float* dy, int B, int T, int t0, float* dgates, float* dh0, float* dc0, const float* aux_src,
                        float* aux_dst, const float* aux_mask, long long aux_n, void* stream);
/* sw_disc_dpred (generator phase of train.py:510-523: D forward on obsv [B,To,2] / pred4 + the backward of its prediction
 * heads, loss gradients formed in the kernel, per-tile loss sums to loss_part) and sw_dec_rollout_bwd in ONE launch: the
 * pass is tile-local and the decode BPTT of the same 16 agents is its only consumer.  dpred4 [B,Tp,4] = scratch that
 * receives d(g_loss)/d(pred4).  Same results as the two calls, bit for bit.  The LDS of the D pass is sw_disc_dpred's
 * (159 744 B at Tp = 24, 164 096 B at Tp = 25): SW_ESHAPE wherever sw_disc_dpred_supported(Tp) is 0.                  */
int sw_dec_rollout_bwd_dfuse(const float* obsv, const float* pred4, const float* d_w, const float* targets, int t_idx,
                             const float* z, float g_label, float g_code, float* loss_part, float* dpred4, const float* enc_w,
                             const float* dec_w, const float* gsave, int B, int To, int Tp, float* gdelta, float* dhT, float* dcT,
                             float* dS_pool, void* stream);

/* ---- WIDE path (socialways_amd/wide.py, csrc/sw_wide.hip): the model at hidden sizes H > 64, H % 32 == 0 (WideTrainer.supports; train.py:42-44,
 *      76-81) as one launch per LSTM step and per decoder / head layer over all agents, explicit backward, deferred
 *      weight gradients.  Replaces, per call, the stock-PyTorch ops behind nn.Linear / nn.LSTM / nn.LeakyReLU / nn.ReLU of
 *      train.py:153-335 (forward and autograd backward).  All buffers row-major fp32, row strides in floats.            */
/* y[r][n] = epi(sum_k x[r][k] w[n][k] + bias[n] + cin[r][n]; aux[r][n]); x element (r,k) at x + r*x_rs + k*x_cs, w element
 * (n,k) at w + n*w_rs + k*w_cs; epi 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 / 4: multiply by ReLU' / LeakyReLU'(0.2) taken from
 * the sign of aux (the layer's saved activation).  bias / cin / aux may be NULL.                                         */
int sw_wide_gemm(const float* x, long long x_rs, int x_cs, const float* w, long long w_rs, int w_cs, const float* bias,
                 const float* cin, int cin_ld, const float* aux, int aux_ld, long long R, int K, int N, float* y, int y_ld, int epi,
                 void* stream);
/* one nn.LSTM step on all B agents: pre = Wx x4 + b1 (+ b2) + Whh h_prev (Wx [4H][4], Whh [4H][H], gate blocks i f g o),
 * gates [B][4H] = activated gates, c_out / h_out the new state (h also to h_out2 if given); h_prev / c_prev NULL = zeros */
int sw_wide_lstm_fwd(const float* x4, int x_ld, const float* h_prev, int hp_ld, const float* c_prev, const float* Wx,
                     const float* b1, const float* b2, const float* Whh, int B, int H, float* gates, float* c_out, float* h_out,
                     int h_ld, float* h_out2, int h2_ld, void* stream);
/* its backward: dh = dh_ext + dh_ext2 + dg_next WhhT^T (WhhT [H][4H]; any of the three may be NULL), cell backward with the
 * saved gates / c / c_prev -> dgates [B][4H] (pre-activation gradients) and dc_out [B][H]                               */
int sw_wide_lstm_bwd(const float* dh_ext, int dhe_ld, const float* dh_ext2, int dhe2_ld, const float* dg_next, const float* WhhT,
                     const float* gates, const float* c, const float* c_prev, const float* dc_in, int B, int H, float* dgates,
                     float* dc_out, void* stream);
/* last decoder layer + integration of a decode step (train.py:330, 422-424): v = a3 W4^T + b4 (W4 [2][D3]), p += v,
 * pred4_i[b*pred_ld] = x4_tm[b*4] = (p, v).  Backward of the step: dx4 = dg WxT^T (dg [B][H4] = dgates of the re-fed encoder
 * step or NULL, WxT [4][H4]), dp_run += dpred.p + dx4.p, dv[b] = (dpred.v + dx4.v + dp_run, 0, 0), dz3 [B][D3] = dv W4       */
int sw_wide_out_fwd(const float* a3, int D3, const float* W4, const float* b4, float* p, int B, float* pred4_i, int pred_ld,
                    float* x4_tm, void* stream);
int sw_wide_out_bwd(const float* dpred4_i, int pred_ld, const float* dg, const float* WxT, int H4, float* dp_run, int B, float* dv,
                    const float* W4, int D3, float* dz3, void* stream);
/* out[r][c] = sum_t in[t*t_stride + r*in_ld + c] */
int sw_wide_sum_steps(const float* in, long long t_stride, int in_ld, int T, long long R, int C, float* out, int out_ld,
                      void* stream);
/* transposed copies of ntab matrices of one packed buffer: tab (device, ntab x {src offset, rows, cols, dst offset} int32, in
 * floats), total_tiles = sum over the matrices of ceil(rows/32) ceil(cols/32); dst[dst_off + c*rows + r] = src[src_off + r*cols + c] */
int sw_wide_transpose(const float* src, const int* tab, int ntab, int total_tiles, float* dst, void* stream);
/* MFMA operand images of ntab matrices of one packed buffer (tab: device, ntab x {src offset, R, K, dst offset, transposed,
 * 0} int32; the image of Mx [R][K] - M or, transposed, M^T of M [K][R] - holds the float4 Mx[16t + (l & 15)][16j + 4(l >> 4)..]
 * at dst offset + ((t K/16 + j) 64 + l) 4); total_float4 = sum of R K / 4                                              */
int sw_wide_opimage(const float* src, const int* tab, int ntab, long long total_float4, float* dst, void* stream);
/* LSTM SEQUENCE kernels (hidden sizes 64 and 128: sw_wide_lstm_seq_supported): T steps of sw_wide_lstm_fwd / _bwd in one
 * launch per 16-agent tile, W_hh / W_hh^T register-resident from their operand images.  x4 [T][B][4], gates [T][B][4H],
 * cs [T][B][H], hs [T+1][B][H] (slab 0 = h_0, c_0 = 0), h_last2 = optional second copy of h_T.  Backward: dh_ext (+ dh_ext2)
 * = gradient w.r.t. h_{T-1} from outside, dg_init [B][4H] = dgates of the step behind the sequence or NULL, dc_init [B][H]
 * = gradient w.r.t. c_{T-1} from that step or NULL; writes dgates [T][B][4H].                                          */
int sw_wide_lstm_seq_supported(int H);
int sw_wide_lstm_seq_fwd(const float* x4, const float* Wx, const float* b1, const float* b2, const float* whh_img, int B, int H, int T,
                         float* gates, float* cs, float* hs, float* h_last2, int h2_ld, void* stream);
int sw_wide_lstm_seq_bwd(const float* dh_ext, int dhe_ld, const float* dh_ext2, int dhe2_ld, const float* dg_init, const float* dc_init,
                         const float* whhT_img, const float* gates, const float* cs, int B, int H, int T, float* dgates, void* stream);
/* the decode loop of predict() (train.py:415-432) at 128 hidden units (sw_wide_dec_loop_supported) as ONE launch per 16-agent
 * tile, streaming the operand images of W1[:, :H], W2, W3 and W_hh per step: replaces Tp x {3 sw_wide_gemm, sw_wide_out_fwd,
 * sw_wide_lstm_fwd}.  u [B][2.5H] = W1[:, H:] [S; z] + b1; p0 = last observed positions; leaves a1 / a2 / a3 [Tp][B][.],
 * pred4 [B][Tp][4], x4 rows To.., gates / cs rows To.., hs rows To + 1.., h into cat[i + 1][:, :H] (row stride 2.5H).    */
int sw_wide_dec_loop_supported(int H);
int sw_wide_dec_loop_fwd(const float* w1h_img, const float* w2_img, const float* w3_img, const float* whh_img, const float* u,
                         const float* b2, const float* b3, const float* W4, const float* b4, const float* Wx, const float* bx1,
                         const float* bx2, const float* p0, int p0_ld, float* a1, float* a2, float* a3, float* pred4, float* x4,
                         float* gates, float* cs, float* hs, float* cat, int B, int H, int To, int Tp, void* stream);
/* ... and its backward (data gradients; Tp x {sw_wide_lstm_bwd, sw_wide_out_bwd, 3 sw_wide_gemm} in one launch): images of W_hh^T,
 * W3^T, W2^T, W1[:, :H]^T and of Wx^T zero-padded to 16 rows; leaves dgates rows To.., dv / dz3 / dz2 / dz1 [Tp][B][.], the gradient
 * w.r.t. h_{To-1} from decode step 0 (dhcat_out) and w.r.t. c_{To-1} (dc_out), both [B][H].                              */
int sw_wide_dec_loop_bwd(const float* whhT_img, const float* w3T_img, const float* w2T_img, const float* w1hT_img,
                         const float* wxT_img, const float* W4, const float* dpred4, const float* a1, const float* a2,
                         const float* gates, const float* cs, float* dgates, float* dv, float* dz3, float* dz2, float* dz1,
                         float* dhcat_out, float* dc_out, int B, int H, int To, int Tp, void* stream);
/* the heads of the discriminator (train.py:280-292, 300-309) for all agents and both future branches in ONE launch per
 * direction (instead of nine / seven sw_wide_gemm launches): p = 52 host values in the order {6 operand images (forward: of0,
 * of1, pe0, pe1, cl0, la0; backward: their transposes), 6 biases, cl1 weight, cl1 bias, la1 weight, la1 bias, hT [B][H], px
 * [nb B][4Tp], outputs o1, q1, both, c1, l1, label, code, inputs dlab [nb B][4], dcod [nb B][nlp], deltas dc1, dl1, dboth, dq1,
 * docode, do1, dhT, dpx, then B, H, 4Tp, nb, nl, nlp, need_obs, want_dpred, then the loss block of the forward launch: loss
 * (0 / 1), target index of branch 0 / 1, row stride of z, the two gradient scales (as the bit patterns of doubles), targets,
 * z, part [tiles][3]}: with loss = 1 the forward launch also forms the LSGAN / info-loss gradients dlab / dcod (train.py:484-494,
 * 512-523) and each tile's sums of squares {branch-0 label, branch-0 code_hat, branch-1 label}.                        */
int sw_wide_disc_heads_supported(int H, int K4, int nl);
int sw_wide_disc_heads_fwd(const long long* p, void* stream);
int sw_wide_disc_heads_bwd(const long long* p, void* stream);
/* n weight-gradient problems dW[N][K] = delta^T act, db = column sums (desc: n x {delta, ldd, act, lda, R, N, K, dW, ldw, db}
 * as 64-bit host values) through the grouped split-K GEMM; wgrad_ws = sw_workspace_floats(SW_WS_WGRAD, ...) floats       */
int sw_wide_wgrad(const long long* desc, int n, float* wgrad_ws, void* stream);

/* ---- A two-hop gradient all-reduce over peer-mapped exchange buffers (csrc/sw_comm.hip) - the data-parallel step's
 *      alternative to `torch.distributed.all_reduce` on RCCL (3 flat buckets of 112 / 112 / 344 KB per step; the
 *      reference itself is single-process, train.py has no counterpart).  Every rank allocates ONE exchange buffer
 *      (sw_comm_alloc, sw_comm_bytes(world, max_floats) bytes, zero-filled device memory), exports it (sw_comm_ipc_export:
 *      a 64-byte hipIpc handle the host passes to the peers by any means), imports the peers' (sw_comm_ipc_import) and then
 *      calls sw_allreduce_direct with the `world` buffer addresses as mapped in ITS process (its own at [rank]): grad[0..n)
 *      becomes the element-wise sum over the ranks, every element summed in rank order by one rank (replicas receive
 *      identical bits).  Collective: every rank must issue the same sequence of calls (same n); asynchronous on `stream`,
 *      capturable in a hipGraph.  A peer that never arrives is given up after SW_COMM_TIMEOUT_S seconds (environment,
 *      default 30) instead of hanging the device: the rank whose wait timed out publishes nothing from it (its peers time
 *      out in turn), writes neither the gradient nor - in the _adam form - the weights for those elements, every later call
 *      on its buffer returns at once, and sw_comm_status (which synchronises the device) reports 1.  The caller makes the
 *      status collective before it trusts the results (trainer.train_epoch).  world <= 16.                                 */
long long sw_comm_bytes(int world, long long max_floats);
int sw_comm_alloc(long long bytes, void** ptr);
int sw_comm_free(void* ptr);
int sw_comm_ipc_export(void* ptr, void* handle64 /* 64 bytes out */);
int sw_comm_ipc_import(const void* handle64, void** ptr);
int sw_comm_ipc_close(void* ptr);
int sw_comm_status(const void* own_buf, int* status /* 0 ok, 1 a wait timed out */);
int sw_allreduce_direct(void* const* peer_bufs /* [world] */, int rank, int world, long long max_floats, float* grad,
                        long long n, void* stream);
/* ... and with the optimizer step behind it in the same launch: every rank applies Adam (sw_adam_packed's arithmetic, same
 * arguments; disc_Tp > 0: the packed weights are a Discriminator's and its registered images follow) to its replica from
 * the reduced gradient while it copies it out.  Interoperates with sw_allreduce_direct on other ranks (a rank without rows
 * in a batch exchanges zeros and updates separately). */
int sw_allreduce_direct_adam(void* const* peer_bufs, int rank, int world, long long max_floats, float* grad, long long n,
                             float* w, float* m, float* v, const float* step, double lr, double beta1, double beta2,
                             double eps, int disc_Tp, void* stream);

/* ---- ADE/FDE partial sums of train.py:546-551:
 *      out[3] = { sum_{b,t} err / Tp, sum_b err[:, -1], sum_{b,t} err^2 },  err = |(p_hat - p) / ss|   */
int sw_ade_fde(const float* pred4 /*[B,Tp,4]*/, const float* gt /*[B,Tp,2]*/, int B, int Tp, float inv_ss,
               float* out /*[3]*/, float* scratch /*[3*SW_RED_BLOCKS] or NULL*/, void* stream);

/* ---- the counter-based device noise stream (csrc/sw_noise.hip; train.py:473 / :584 draw z ~ U[0,1) from torch's CPU generator,
 *      which stays the default): every z value is a pure function of (seed, domain, step, draw, row, column), so any rank,
 *      chunk or tile produces exactly its rows in one launch, evaluation repeats call to call and a checkpoint that carries
 *      {seed, step} continues the same stream.  Philox4x32-10, standard constants (multipliers 0xD2511F53 / 0xCD9E8D57, key
 *      increments 0x9E3779B9 / 0xBB67AE85): key = (seed low, seed high 32 bits), counter = (row, draw, step,
 *      (column >> 2) + 256 domain); the four output words are columns 4b .. 4b+3 of column block b; value =
 *      float(word >> 8) * 2^-24 - exact, in [0, 1), torch.rand's 24-bit grid.  domain 0 = training, 1 = evaluation / sampling.
 *        out[((t n_draws + k) rows + i) ld + j] = the value at (step0 + t, draw0 + k, row0 + i, j) for j < cols, 0 for
 *        cols <= j < ld (the zero padding to the kernels' SW_Z noise columns comes out of the same launch).
 *      One thread per (row, 4-column block), one 16-byte store each; no LDS, no atomics, no host synchronisation, no
 *      allocation: capturable in a hipGraph.  Checked before any device call - SW_EARG: domain outside 0 .. 1, cols outside
 *      1 .. 1024, ld < cols or ld % 4, out NULL or not 16-byte aligned, a count below 1, row0 + rows / draw0 + n_draws /
 *      step0 + n_steps past 2^32; SW_ESHAPE: n_steps n_draws rows ld / 4 above 2^31 - 1 (the kernel's 32-bit float4 index). */
int sw_noise_uniform(unsigned long long seed, int domain, unsigned step0, int n_steps, unsigned draw0, int n_draws,
                     unsigned row0, int rows, int cols, int ld, float* out /*[n_steps][n_draws][rows][ld]*/, void* stream);

/* ==== MEASUREMENT SECTION - not part of the product surface (the drop-in boundary ends above this line; tests/test_abi.py
 *      checks the two lists separately).  sw_kernel_timing(1): every kernel launch of the library is bracketed by two HIP
 *      events on its own stream (never inside a graph capture) until sw_kernel_timing(0); sw_kernel_timing_read(buf, cap)
 *      waits for the device and writes one line "kernel calls total_us" per kernel, returning the bytes needed.
 *      sw_debug_spin queues a kernel that occupies the stream for ~us microseconds (queued in front of a timed sequence it
 *      lets the host run ahead, so the event intervals hold no launch gaps).  bench.py's roofline pass is their only caller. */
int sw_kernel_timing(int on);
int sw_kernel_timing_read(char* buf, int cap);
int sw_debug_spin(double us, void* stream);

#ifdef __cplusplus
}
#endif
#endif
