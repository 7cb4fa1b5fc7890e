/*
 * st2.h -- C ABI of libst2_hip.so, the MI355X (gfx950) kernel library behind the
 * StyleTTS 2 text->waveform hot path (style-diffusion sampler, AdaIN acoustic decoder,
 * iSTFTNet / HiFi-GAN vocoder).
 *
 * The reference (yl4579/StyleTTS2) has no FFI of its own: the hot path is a chain of
 * torch ATen ops issued from nn.Module.forward.  Each entry point
 * below therefore replaces one *class* of ATen calls; the reference call sites it stands
 * in for are cited per function (paths relative to the reference tree).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated otherwise; the caller owns
 *     all memory; nothing is allocated or freed inside the library (one exception: the 64-byte
 *     host-mapped status word of st2_status(), allocated once per process);
 *   - tensors are row-major "NCL": element (b, c, l) of tensor t lives at
 *     t + b * t_bs + c * t_cs + l   (strides in ELEMENTS; bs = batch, cs = channel);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is
 *     stream-ordered and asynchronous; no entry point synchronises;
 *   - return value: 0 on success, non-zero on error; st2_last_error() gives the message
 *     of the last failing call on this thread.  No C++ exception crosses the ABI;
 *   - devices: every entry point works on the CURRENT HIP device of the calling thread; per-kernel settings
 *     (dynamic LDS limits, co-residency capacities, the autotuner's table) are kept per device ordinal, so one
 *     process may drive several GPUs.  The measurement hooks (st2_conv_timing*, st2_conv_tune*) are process-wide
 *     and meant for one driving thread.
 */
#ifndef ST2_H
#define ST2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST2_ABI_VERSION 23

/* ---- library ---------------------------------------------------------------------- */
int st2_abi_version(void);
const char* st2_last_error(void);
/* Fills name (<= cap bytes) with the gcnArchName of device `dev`, returns CU count or <0. */
int st2_device_info(int dev, char* name, int cap);

/* ---- sticky device-side status --------------------------------------------------------------------------------- *
 * Conditions a kernel can only detect on the device are OR-ed into ONE process-wide status word that lives in
 * host-mapped (pinned) memory -- the single allocation this library makes, 64 bytes, on the first call that needs
 * it -- so the host reads it without a device synchronisation; a bit is visible once the kernel that raised it has
 * completed.  Bits:
 *   ST2_STATUS_F16_RANGE     an operand of a split-f16 conv exceeded the f16 range after scaling (|x * x_scale| >
 *                            65504) and was clamped to +-65504 (st2_act_split, st2_conv1d_f16s): the result is finite
 *                            but not the fp32 conv's; re-run that layer with a smaller x_scale or on st2_conv1d.  A NaN
 *                            operand raises the same bit (ABI 18: the clamp maps it to -65504);
 *   ST2_STATUS_LSTM_TIMEOUT  a bounded spin of st2_lstm_bidir_coop expired (a group's workgroups were not
 *                            co-resident in time): the outputs of that call are invalid;
 *                            (st2_lstm_bidir_coop called directly; the launch plans use st2_lstm_bidir_coop_recovering, which
 *                            repairs the call in-stream and raises ST2_STATUS_LSTM_RECOVERED instead);
 *   ST2_STATUS_DURATION_SUM  a row of the durations handed to st2_expand_by_durations does not sum to T (caller-supplied
 *                            durations with a wrong `total_frames`): frames past the sum repeat the last phoneme.
 *   ST2_STATUS_FRAME_CAPACITY  (added under ABI 23, additive) a row of the durations handed to st2_frames_from_durations
 *                            sums to more than the capacity T_cap: its frame count was clamped to T_cap and the row is
 *                            synthesised TRUNCATED to its first T_cap frames (st2_expand_by_durations_len then raises
 *                            ST2_STATUS_DURATION_SUM for the same row).  Both bits mean "this row is not its solo run;
 *                            retry with a larger capacity"; every other row of the batch is unaffected.
 * st2_status(clear != 0) returns the word and atomically clears it.  Returns < 0 if no HIP device is usable. */
#define ST2_STATUS_F16_RANGE 1
#define ST2_STATUS_LSTM_TIMEOUT 2
#define ST2_STATUS_DURATION_SUM 4
#define ST2_STATUS_LSTM_RECOVERED 8  /* informational: a cooperative BiLSTM group timed out and st2_lstm_bidir_coop_recovering
                                        re-ran the call on the single-CU kernel -- the outputs are VALID, latency was lost */
#define ST2_STATUS_FRAME_CAPACITY 16 /* informational-but-reported: a row was truncated to the caller's frame capacity */
int st2_status(int clear);

/* ---- fused Conv1d (implicit GEMM on v_mfma_f32_32x32x2_f32, exact fp32) ------------ *
 * y[b,co,l] = epi( bias[co] + sum_{ci,t} W[co,ci,t] * pro(x)[b,ci, l + t*dil - pad_left] )
 * with zero padding applied AFTER the prologue, stride 1.
 * Replaces: F.conv1d behind every weight-normed nn.Conv1d on the path
 *   Modules/istftnet.py:68-74 (AdaINResBlock1 convs1/convs2), :445-448 (AdainResBlk1d),
 *   :319-322,364 (ConvTranspose1d via its polyphase form, see st2_convt_interleave),
 *   :377 (conv_post), Modules/hifigan.py:65-74,292-294,344, models.py:255-263,
 *   and nn.Linear / 1x1 Conv1d of the denoiser, Modules/diffusion/modules.py:256-261,
 *   484-490,317-324 (tokens laid out channel-major so a Linear is a k=1 conv).
 */
enum st2_prologue {
  ST2_PRO_NONE = 0,
  ST2_PRO_LEAKY = 1,        /* x>=0 ? x : slope*x                       istftnet.py:360,376 */
  ST2_PRO_ADAIN_LEAKY = 2,  /* leaky((1+g)*(x-mean)*rstd + b)           istftnet.py:441-447 */
  ST2_PRO_ADAIN_SNAKE = 3,  /* u=(1+g)*(x-mean)*rstd+b; u+sin(a u)^2/a  istftnet.py:68-72   */
  ST2_PRO_SNAKE = 4,        /* x + sin(a x)^2 / a                       hifigan.py:329,343  */
  ST2_PRO_COLNORM = 5       /* (x-mean[b,l])*rstd[b,l]*G[b,c]+Bt[b,c]   modules.py:18-38,556 */
};
enum st2_epilogue_act {
  ST2_ACT_NONE = 0,
  ST2_ACT_GELU = 1,     /* exact erf GELU                                modules.py:484-490 */
  ST2_ACT_EXP_SIN = 2,  /* rows < act_split: exp, rows >= act_split: sin istftnet.py:378-379 */
  ST2_ACT_TANH = 3,     /*                                               hifigan.py:345     */
  ST2_ACT_LEAKY = 4,    /* leaky(act_slope)                                                  */
  ST2_ACT_GELU_TANH = 5 /* 0.5 x (1 + tanh(sqrt(2/pi)(x + 0.044715 x^3))): HF "gelu_new", the ALBERT FFN of PL-BERT
                           (Utils/PLBERT/util.py:19-20 -> transformers AlbertConfig.hidden_act)               */
};

typedef struct st2_conv_desc {
  /* geometry */
  int32_t B, C_in, C_out, L_in, L_out, ks, dil, pad_left;
  /* input */
  const float* x; int64_t x_bs; int32_t x_cs;
  /* weights packed K-major: wt[(ci*ks + t) * w_ld + co], w_ld >= C_out, w_ld % 4 == 0 */
  const float* wt; int32_t w_ld;
  const float* bias;                 /* [C_out] or NULL */
  /* output */
  float* y; int64_t y_bs; int32_t y_cs;
  /* prologue */
  int32_t pro;                       /* enum st2_prologue */
  float slope;                       /* LEAKY / ADAIN_LEAKY */
  const float* stats;                /* ADAIN_*: [B][C_in][2] = (mean, rstd); COLNORM: [B][L_in][2] */
  const float* gamma; const float* beta;  /* ADAIN_*: gamma[b*gb_bs + c]; the kernel applies (1+gamma)
                                             COLNORM: G = gamma[b*gb_bs+c] (+1 if gamma_plus_one) */
  int64_t gb_bs; int32_t gamma_plus_one;
  const float* alpha;                /* SNAKE modes: [C_in] */
  /* epilogue: v = acc + bias; v += res; v += res2; v /= div; v = act(v) */
  const float* res;  int64_t res_bs;  int32_t res_cs;  int32_t res_shift;  /* reads res[b,co,l>>res_shift] */
  const float* res2; int64_t res2_bs; int32_t res2_cs;
  float div;                         /* 1.0f = none */
  int32_t act; int32_t act_split; float act_slope;
  /* st2_conv1d_f16s only: split-f16 packed weights (see below); ignored by st2_conv1d */
  const void* wq; int32_t wq_co_pad; int32_t wq_cin_pad;
  float x_scale;                     /* power of two applied to pro(x) before the hi/lo split (by rule 8 after a normalising
                                        prologue, else 1; per layer after st2_calibrate) */
  float out_scale;                   /* applied to the accumulator first: 1 / (x_scale * weight scale), or 1 / x_scale
                                        when w_row_scale carries the per-row weight scales */
  const float* w_row_scale;          /* [wq_co_pad] or NULL: 1 / (per-output-row weight scale); the accumulator of row co
                                        is multiplied by out_scale * w_row_scale[co] (both powers of two: exact) */
  /* st2_conv1d_xs only: pre-activated, pre-split input planes written by st2_act_split (x/pro/stats/... unused) */
  const void* xs; int32_t xs_cg; int32_t xs_lp; int32_t xs_halo;
  /* st2_conv1d_xs only, optional: per-tile InstanceNorm partial sums of the STORED output,
     part[((b*C_out + co)*part_nt + l/128)*2 + {0,1}] = (sum, sum of squares) of (y - shift) over the 128 columns of that tile,
     shift = the tile's first stored value y[b][co][128*(l/128)], itself stored at part[B*C_out*part_nt*2 + (b*C_out + co)*part_nt +
     l/128]: the buffer holds B*C_out*part_nt*3 floats (see st2_stats_finalize) */
  float* part; int32_t part_nt;
  /* st2_conv1d_xs only (ABI v20): columns per partial-sum slot, 0 = 128.  A small-grid launch (fewer workgroups than CUs: one
     utterance) runs 128 x 64 or 128 x 32 tiles and emits its sums per 64 / 32 columns: the caller asks
     st2_conv1d_xs_part_cols(d) BEFORE sizing `part` (part_nt >= ceil(L_out / part_cols)) and passes the answer here; a caller
     that leaves it 0 keeps the 128-column tiles and the 128-column slots.  st2_stats_finalize sums whatever slots there are. */
  int32_t part_cols;
  /* st2_conv1d_f16s only, optional: workspace for split-K launches.  A layer whose grid leaves most of the chip idle and
     whose k loop is long (C_in >= 8 chunks, < 128 workgroups: the 1024 -> 2048 Linears of the denoiser over the ~100
     tokens of one utterance) runs as up to 8 K slices per tile + a fixed-order reduction that applies the epilogue; the
     split is a function of the geometry alone (every plan picks the same one: results are reproducible bit for bit) and
     needs st2_conv1d_f16s_splitk_bytes(d) bytes here (the slices are stored in the accumulator layout of whole tiles: ksplit * B *
     padded C_out * padded L_out * 4).  NULL / too small = no split. */
  void* splitk_ws; int64_t splitk_ws_bytes;
  /* ABI v23, optional: per-row lengths of a ragged batch (int32 [B] on the device, NULL = every row is L_in / L_out long).
     x_len[b] (st2_conv1d_f16s): row b of the input ends at x_len[b] <= L_in -- positions past it are the conv's zero padding
     AFTER the prologue (a select: whatever the memory holds there is ignored).  The xs path gets the same from
     st2_act_split_len.  y_len[b] (both kernels): row b of the output ends at y_len[b] <= L_out -- tiles wholly past it exit
     before doing any work, nothing is stored at or past it, and the epilogue's partial sums cover only its columns
     (st2_stats_finalize_len).  Outputs past y_len[b] are left as the memory held them.  Values above L_in / L_out are
     clamped.  st2_conv1d (the exact-fp32 kernel) does not implement them and rejects a descriptor that sets either. */
  const int32_t* x_len; const int32_t* y_len;
} st2_conv_desc;

int st2_conv1d(const st2_conv_desc* d, void* stream);

/* ---- fused Conv1d on the f16 matrix pipe, fp32-class accuracy ("f16 hi/lo split") ---- *
 * Same contract, prologues and epilogues as st2_conv1d.
 * Each operand v is carried as f16 hi + f16 lo of v*scale and the product is evaluated as
 * hi*hi + hi*lo + lo*hi by three v_mfma_f32_32x32x16_f16 into one fp32 accumulator (the dropped lo*lo
 * term is 2^-22 relative).  Through the whole decoder the waveform differs from an fp64 evaluation by
 * 2.6e-7 RMS, the fp32 ATen path by 2.4e-7; the rate ceiling is 5.3x that of the exact-fp32 MFMA.
 * Weights are pre-split once per load (the d.wt field is unused):
 *   wq[((ci/16 * ks + t) * 2 + (ci%16)/8) * wq_co_pad + co][16 halves] = hi[0..7] | lo[0..7]
 *   over the 8 channels ci..ci+7 of W[co, ., t] * w_scale[co], zero padded to wq_cin_pad input channels
 *   (a multiple of st2_conv1d_f16s_chunk(ks)) and wq_co_pad rows (a multiple of
 *   st2_conv1d_f16s_co_block(C_out)); w_scale[co] is the power of two that puts max_{ci,t}|W[co]| in [2^13, 2^14)
 *   (per OUTPUT ROW, so a checkpoint whose rows differ by many octaves keeps every row's lo halves in the normal
 *   f16 range; d.w_row_scale = 1 / w_scale[co]).  Operands are clamped to the f16 range (ST2_STATUS_F16_RANGE).
 * Replaces the same reference call sites as st2_conv1d (decoder / vocoder convolutions, denoiser Linears). */
int st2_conv1d_f16s(const st2_conv_desc* d, void* stream);
/* Bytes of d.splitk_ws the launch described by *d would use (0 = this geometry is not split): the caller allocates that
 * much (any alignment >= 16) and sets d.splitk_ws / d.splitk_ws_bytes before calling st2_conv1d_f16s. */
int64_t st2_conv1d_f16s_splitk_bytes(const st2_conv_desc* d);
int st2_conv1d_f16s_chunk(int ks);        /* input-channel padding granule of the packed weight */
int st2_conv1d_f16s_co_block(int C_out);  /* output-channel padding granule of the packed weight */
/* Measurement hook (process-wide): which build of the fused kernel a launch takes.  0 (default) = by rule: the
 * warp-specialised persistent build (512-thread workgroups, one per CU: four waves stage + activate the input, four issue
 * the MFMAs; bitwise the same results) for AdaIN + Snake convs with k = 3, C_out <= 64 and at least 512 tiles, the one-role
 * build otherwise; 1 = one-role build always; 2 = warp-specialised for every layer it can run (k = 3 / 7 / 11, C_out <= 64). */
void st2_conv1d_f16s_set_variant(int variant);
/* Measurement hook (process-wide): the depth of the split-K rule -- at most `max_slices` K slices per tile (1..32), each of at
 * least `min_chunks` input-channel chunks (1..16); out-of-range values restore the default (8, 4).  Every plan of a process sees
 * the same rule (results stay reproducible within the process); the default is what the tests and the bench run. */
void st2_conv1d_f16s_set_splitk(int max_slices, int min_chunks);
/* sizeof(st2_conv_desc) as the library was compiled: lets a binding verify its struct mirror. */
int st2_sizeof_conv_desc(void);

/* ---- activation pass + pure MFMA conv ("xs" path) -------------------------------------------------------------- *
 * The fused prologue of st2_conv1d_f16s costs ~40 VALU instructions per staged element inside the MFMA kernel.  The
 * xs path runs it ONCE per element in an HBM-bound pass instead and hands the conv pre-split f16 operands:
 *
 *   st2_act_split:  xs[b][plane][cg][pos][e] (f16; plane 0 = hi, 1 = lo; 16-byte slots of 8 channels) =
 *                   split( x_scale * pro(x)[b][cg*8 + e][pos - halo] ),  zero for pos - halo outside [0, L) and for
 *                   channels >= C.  Same prologue arithmetic (op for op) as st2_conv1d_f16s.  cg in [0, xs_cg),
 *                   pos in [0, Lp); xs_cg*8 >= C rounded up to st2_conv1d_f16s_chunk(ks) of the consuming conv.
 *                   gb_seg > 0 (ST2_PRO_COLNORM only): the gamma / beta row of position l is l / gb_seg instead of the
 *                   batch index b -- the token-merged view [1][C][B*N] of B utterances of N tokens whose LayerNorm
 *                   affine is per utterance (the multispeaker denoiser's AdaLayerNorm, Modules/diffusion/modules.py:
 *                   104-118), so that their q / kv projections run as ONE GEMM over B*N columns.
 *   st2_conv1d_xs:  same GEMM, weights (d.wq ...) and epilogue as st2_conv1d_f16s on those planes: chunks are staged
 *                   global -> LDS as plain 16-byte copies, no per-element arithmetic in the MFMA kernel.  Requires
 *                   pad_left <= xs_halo and Lp large enough for the last tile (checked).  If d.part != NULL the
 *                   epilogue also emits per-128-column partial (sum, sumsq) of the stored output so the next
 *                   layer's InstanceNorm statistics need no extra read of the tensor:
 *   st2_stats_finalize: stats[row] = (mean, 1/sqrt(var+eps)) from part[row][nt][2] (fp64, fixed order), rows = B*C.
 *                   ABI v20: the partial sums are SHIFTED -- slot i holds (sum, sum of squares) of (y - shift_i) over its
 *                   columns, shift_i = the slot's first stored value, written by the producer behind the sums (part = float2
 *                   [rows][nt], then float [rows][nt]); the finaliser combines the slots with Chan's formula (cols = columns
 *                   per slot: d.part_cols or 128 for the convs, 1024 for st2_convt_interleave_stats).  Unshifted E[x^2] - mean^2 from fp32
 *                   partial sums loses rstd of a channel whose mean dominates its variance (|mean| / std = 100: 1e-4 relative,
 *                   three decades above the reference's two-pass fp32 reduction).
 * Replaces the same reference call sites as st2_conv1d_f16s + st2_instnorm_stats. */
int st2_act_split(const float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L,
                  int32_t pro, float slope, const float* stats, const float* gamma, const float* beta, int64_t gb_bs,
                  int32_t gb_seg, int32_t gamma_plus_one, const float* alpha, float x_scale,
                  void* xs, int32_t xs_cg, int32_t Lp, int32_t halo, void* stream);
int st2_conv1d_xs(const st2_conv_desc* d, void* stream);
/* Ragged rows (ABI v23): as st2_act_split, with row b ending at len[b] <= L (int32 [B] on the device; NULL = L): positions at or
 * past it are written as zeros after the prologue; values above L are clamped.  Not defined for ST2_PRO_COLNORM. */
int st2_act_split_len(const float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L,
                      int32_t pro, float slope, const float* stats, const float* gamma, const float* beta, int64_t gb_bs,
                      int32_t gb_seg, int32_t gamma_plus_one, const float* alpha, float x_scale,
                      void* xs, int32_t xs_cg, int32_t Lp, int32_t halo, const int32_t* len, void* stream);
/* Columns per partial-sum slot (128, 64 or 32) the launch described by *d would use when its caller opts into the small-grid
 * builds (d.part_cols): a function of the geometry alone -- every plan gets the same answer, results are reproducible bit for
 * bit.  k = 3 / 7 / 11 launches of up to three utterances: 32 below ~100 tiles of 128 x 128, 64 up to ~900 (k = 3) / 340 (k = 7,
 * 11); 128 otherwise (y is bitwise the same either way: st2_conv1d_xs_impl.h). */
int st2_conv1d_xs_part_cols(const st2_conv_desc* d);
/* ---- the conv launch rule (added under ABI 23, additive; host-only: launches nothing, never touches the GPU) ------- *
 * How ONE split-f16 convolution is issued.  Both host routines that issue them -- conv() of the C++ plans and ops.conv1d of
 * the per-kernel Python plans -- ask here and do what the answer says, so a layer is routed, scaled and sized the same way by
 * both (the plans are held bitwise equal).  Reads B, C_in, C_out, L_in, L_out, ks, pad_left and pro of *d.
 *   route         ST2_CONV_ROUTE_XS (st2_act_split + st2_conv1d_xs) when pad_left <= xs_halo, L_in >= xs_min_l, the conv has a
 *                 prologue or C_in >= 64 (the split pass is then cheap next to the conv), and not prefer_fused; else
 *                 ST2_CONV_ROUTE_FUSED (st2_conv1d_f16s).  force_fused != 0 (the contract tests' selector) = fused always.
 *   prefer_fused  1: a prologue and C_in <= 64, or ks <= 3 and C_in <= 128 -- the xs pair of such a layer is HBM-bound (20
 *                 against 12 bytes per element), the fused kernel wins whatever the length (measured per layer at B = 32).
 *   x_scale       the operand scale by rule: 8 after a normalising prologue (ADAIN_LEAKY, ADAIN_SNAKE, COLNORM), else 1; a
 *                 calibrated per-layer value (st2_calibrate) overrides it.
 *   xs_min_l      256: shorter rows stay on the fused kernel (an xs row is >= 640 slots).
 *   xs_*          the split planes of THIS input, filled on either route (st2_act_split can be driven on any layer):
 *                 xs_cg = C_in rounded up to 32, in groups of 8; xs_lp = slots per row = xs_halo + (L_in + 1 rounded up to the
 *                 widest conv tile, 512) + 96 for the last tile's taps; xs_halo = 32 zero columns in front of every row (>= the
 *                 largest pad_left on the path); xs_bytes = B * 2 * xs_cg * xs_lp * 16.
 *   part_*        want_stats != 0: the partial-sum layout of the output's InstanceNorm statistics -- part_cols columns per slot
 *                 (st2_conv1d_xs_part_cols(d) on the xs route, to be passed as d.part_cols; 128 on the fused route, whose
 *                 d.part_cols stays 0), part_nt = ceil(L_out / part_cols) slots, part_floats = B * C_out * part_nt * 3.  All 0
 *                 without want_stats.
 *   splitk_bytes  fused route without statistics: st2_conv1d_f16s_splitk_bytes(d); else 0.
 * Returns non-zero (with the error text set) for gb_seg > 0 on the fused route: the per-segment affine exists in
 * st2_act_split only. */
enum st2_conv_route { ST2_CONV_ROUTE_XS = 0, ST2_CONV_ROUTE_FUSED = 1 };
typedef struct st2_conv_plan {
  int32_t route;         /* enum st2_conv_route */
  int32_t prefer_fused;
  float x_scale;
  int32_t xs_cg, xs_lp, xs_halo, xs_min_l;
  int64_t xs_bytes;
  int32_t part_cols, part_nt;
  int64_t part_floats;
  int64_t splitk_bytes;
} st2_conv_plan;
int st2_conv_launch_plan(const st2_conv_desc* d, int32_t want_stats, int32_t gb_seg, int32_t force_fused, st2_conv_plan* plan);
int st2_stats_finalize(const float* part, int32_t rows, int32_t nt, int32_t L, float eps, float* stats, int32_t cols, void* stream);
/* Ragged rows (ABI v23): row r covers len[r / len_div] <= L columns (len int32 on the device, NULL = L; len_div = channels per
 * batch item).  Slots wholly past that end are not read; the last one counts only its valid columns. */
int st2_stats_finalize_len(const float* part, int32_t rows, int32_t nt, int32_t L, float eps, float* stats, int32_t cols,
                           const int32_t* len, int32_t len_div, void* stream);

/* ---- small direct Conv1d (any stride, tiny C_in): noise convs, F0/N down-convs ------ *
 * y[b,co,l] = bias[co] + sum_{ci,t} w[co,ci,t] * x[b,ci, l*stride + t - pad]   (plain OIK weights)
 * Replaces: Modules/istftnet.py:332-339,361 (noise_convs), :486-488,511-512 (F0_conv/N_conv),
 *           Modules/hifigan.py:296-303,330, models.py:464-465 (F0_proj/N_proj).
 */
int st2_conv1d_direct(const float* x, int64_t x_bs, int32_t x_cs,
                      const float* w, const float* bias,
                      float* y, int64_t y_bs, int32_t y_cs,
                      int32_t B, int32_t C_in, int32_t C_out, int32_t L_in, int32_t L_out,
                      int32_t ks, int32_t stride, int32_t pad, void* stream);
/* Ragged rows (ABI v23): row b of the input ends (zero padding) at x_len[b] <= L_in, outputs at or past y_len[b] are written as
 * exact zeros (int32 [B] on the device; either may be NULL). */
int st2_conv1d_direct_len(const float* x, int64_t x_bs, int32_t x_cs, const float* w, const float* bias,
                          float* y, int64_t y_bs, int32_t y_cs, int32_t B, int32_t C_in, int32_t C_out, int32_t L_in,
                          int32_t L_out, int32_t ks, int32_t stride, int32_t pad, const int32_t* x_len,
                          const int32_t* y_len, void* stream);

/* ---- polyphase split of a strided Conv1d input (kernel = 2*stride, the noise_convs of both vocoders) -------- *
 * xp[b][ci*stride + r][u] = x[b][ci][u*stride + r - pad]  for u in [0,Lu), r in [0,stride); 0 outside [0,L_in).
 * With weights.polyphase_strided_conv() the strided conv becomes a stride-1, k=2 st2_conv1d over C*stride
 * channels (L_out = Lu - 1) on the matrix pipe.
 * Replaces the im2col inside F.conv1d(stride=s): Modules/istftnet.py:332-336,361, Modules/hifigan.py:296-300,330. */
int st2_phase_split(const float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L_in,
                    int32_t stride, int32_t pad, float* xp, int64_t p_bs, int32_t p_cs, int32_t Lu, void* stream);

/* ---- InstanceNorm1d statistics ------------------------------------------------------ *
 * stats[b][c] = (mean, 1/sqrt(biased_var + eps)) over l in [0,L).  fp64 accumulation in a
 * fixed tree order (bitwise reproducible).  Replaces nn.InstanceNorm1d inside AdaIN1d,
 * Modules/istftnet.py:15-25.
 */
int st2_instnorm_stats(const float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L,
                       float eps, float* stats /* [B][C][2] */, void* stream);
/* Ragged rows (ABI v23): row b covers its first len[b] <= L columns (int32 [B] on the device, NULL = L), reduced in an order
 * that does not depend on the row's address. */
int st2_instnorm_stats_len(const float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L,
                           float eps, float* stats, const int32_t* len, void* stream);

/* LayerNorm statistics over the CHANNEL axis of an NCL tensor: stats[b][l] = (mean, rstd) over c.
 * Replaces F.layer_norm's reduction, Modules/diffusion/modules.py:18-38,556-557. */
int st2_colnorm_stats(const float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L,
                      float eps, float* stats /* [B][L][2] */, void* stream);

/* ---- style FC: h[b][j] = act(bias[j] + sum_k s[b][k] * wt[k*J + j])  (all AdaIN fc's of a module
 * concatenated along j; act is an st2_epilogue_act, NONE or GELU).  Replaces the per-AdaIN nn.Linear,
 * Modules/istftnet.py:19,22-24, and the per-utterance mapping MLPs of the denoiser,
 * Modules/diffusion/modules.py:333-357,363-384. */
int st2_style_fc(const float* s, int32_t B, int32_t K, const float* wt, const float* bias,
                 int32_t J, int32_t act, float* h, void* stream);

/* ---- ConvTranspose1d finishing pass ------------------------------------------------- *
 * phases[b][r*C + co][q] (q in [0,Lq)) is the polyphase GEMM output of st2_conv1d;
 * out[b,co,l] = bias[co] + phases[b][((l+pad)%s)*C + co][(l+pad)/s] + add[b,co,l]
 * for l in [0,L_raw); if reflect_left the result is shifted right by one sample and
 * out[.,.,0] = value at raw index 1 (nn.ReflectionPad1d((1,0))).  L_out = L_raw + reflect_left.
 * Columns q >= Lq read as 0 (the transposed conv's zero padding); 0 <= pad, 1 <= stride <= 64 (anything else is refused).
 * Replaces: Modules/istftnet.py:364-368 (ups[i], reflection_pad, + x_source),
 *           Modules/hifigan.py:333-334.
 */
int st2_convt_interleave(const float* phases, int64_t p_bs, int32_t p_cs, int32_t Lq,
                         const float* bias, const float* add, int64_t a_bs, int32_t a_cs,
                         float* out, int64_t o_bs, int32_t o_cs,
                         int32_t B, int32_t C, int32_t stride, int32_t pad, int32_t L_raw,
                         int32_t reflect_left, void* stream);

/* Same, additionally emitting per-tile InstanceNorm partial sums of the stored output (tiles of 1024 positions):
 * part[((b*C + co)*part_nt + l/1024)*2 + {0,1}] = (sum, sum of squares) of (out - shift), shift = out[b][co][1024*(l/1024)] stored at
 * part[B*C*part_nt*2 + (b*C + co)*part_nt + l/1024] (B*C*part_nt*3 floats in all); part may be NULL.  Feed to
 * st2_stats_finalize: the AdaIN that follows the up-sampling needs no pass over the tensor. */
int st2_convt_interleave_stats(const float* phases, int64_t p_bs, int32_t p_cs, int32_t Lq,
                               const float* bias, const float* add, int64_t a_bs, int32_t a_cs,
                               float* out, int64_t o_bs, int32_t o_cs,
                               int32_t B, int32_t C, int32_t stride, int32_t pad, int32_t L_raw,
                               int32_t reflect_left, float* part, int32_t part_nt, void* stream);
/* Ragged rows (ABI v23): row b has q_len[b] <= Lq phase columns (the rest is the transposed conv's zero padding) and
 * out_len[b] <= L_raw + reflect_left outputs; tiles wholly past out_len[b] exit, partial sums cover only its columns, outputs
 * past out_len[b] are left as the memory held them (st2_stats_finalize_len with len_div = C).  Both int32 [B] on the device,
 * both NULL or both set. */
int st2_convt_interleave_stats_len(const float* phases, int64_t p_bs, int32_t p_cs, int32_t Lq,
                                   const float* bias, const float* add, int64_t a_bs, int32_t a_cs,
                                   float* out, int64_t o_bs, int32_t o_cs,
                                   int32_t B, int32_t C, int32_t stride, int32_t pad, int32_t L_raw,
                                   int32_t reflect_left, float* part, int32_t part_nt, const int32_t* q_len,
                                   const int32_t* out_len, void* stream);
/* Positions per partial-sum slot of the two entries above (1024; added under ABI 23, host-only): part_nt >= ceil(L_out / this), and the `cols`
 * their sums go to st2_stats_finalize with. */
int st2_convt_interleave_part_cols(void);

/* ---- AdaIN + LeakyReLU + depthwise ConvTranspose1d(k3,s2,p1,op1) ("pool") ------------ *
 * Replaces Modules/istftnet.py:441-444 with upsample=True (weights w[c][3], bias[c]). */
int st2_adain_leaky_pool(const float* x, int64_t x_bs, int32_t x_cs,
                         const float* stats, const float* gamma, const float* beta, int64_t gb_bs,
                         float slope, const float* w, const float* bias,
                         float* y, int64_t y_bs, int32_t y_cs,
                         int32_t B, int32_t C, int32_t L, void* stream);
/* Ragged rows (ABI v23): row b of the input ends (zero padding) at len[b] <= L; 2 * len[b] outputs are written, the rest of
 * the row is left as the memory held it. */
int st2_adain_leaky_pool_len(const float* x, int64_t x_bs, int32_t x_cs,
                             const float* stats, const float* gamma, const float* beta, int64_t gb_bs,
                             float slope, const float* w, const float* bias,
                             float* y, int64_t y_bs, int32_t y_cs,
                             int32_t B, int32_t C, int32_t L, const int32_t* len, void* stream);

/* ---- harmonic source (SineGen + SourceModuleHnNSF) ---------------------------------- *
 * f0 [B][F] frame-rate F0 (Hz), U samples per frame, H harmonics (9).
 * noise [B][F*U][H] standard normal draws (the reference's randn_like, istftnet.py:242).
 * lin_w [H], lin_b [1]: l_linear.  out [B][F*U] = tanh(linear(sine_waves)).
 * phase_scratch: [B][H][F] floats.  Bit-faithful to ATen-CPU op order.
 * Replaces Modules/istftnet.py:141-247,283-297,352-354 (identical code hifigan.py:112-268).
 */
int st2_har_source(const float* f0, int32_t B, int32_t F, int32_t U, int32_t H,
                   const float* noise, const float* lin_w, const float* lin_b,
                   float sine_amp, float noise_std, float voiced_threshold, float sample_rate,
                   float* phase_scratch, float* out, void* stream);
/* Ragged rows (ABI v23): row b holds f_len[b] <= F frames (int32 [B] on the device, NULL = F) in the [B][F] / [B][F*U][H] /
 * [B][F*U] layouts: its phase prefix sums, its interpolation boundary and the noise it reads end there; out is exactly 0 from
 * f_len[b] * U on. */
int st2_har_source_len(const float* f0, int32_t B, int32_t F, int32_t U, int32_t H,
                       const float* noise, const float* lin_w, const float* lin_b,
                       float sine_amp, float noise_std, float voiced_threshold, float sample_rate,
                       float* phase_scratch, float* out, const int32_t* f_len, void* stream);

/* ---- STFT of the harmonic source (n_fft = win = N, hop, periodic Hann, center/reflect) *
 * har[b][k][m] = |X_k|, har[b][N/2+1+k][m] = atan2(Im, Re), k in [0,N/2], m in [0, L/hop].
 * Replaces Modules/istftnet.py:91-97,355-357. */
int st2_stft_mag_phase(const float* x, int32_t B, int32_t L, int32_t n_fft, int32_t hop,
                       float* har, int64_t har_bs, int32_t har_cs, void* stream);
/* Ragged rows (ABI v23): row b is len[b] <= L samples of a row of L, reflect-padded at its own end; frames m > len[b] / hop
 * are exact zeros.  len[b] is clamped to n_fft / 2 + 1 .. L (the reflection needs more samples than n_fft / 2, as
 * torch's reflect pad does): a shorter row gives the result of its first n_fft / 2 + 1 samples. */
int st2_stft_mag_phase_len(const float* x, int32_t B, int32_t L, int32_t n_fft, int32_t hop,
                           float* har, int64_t har_bs, int32_t har_cs, const int32_t* len, void* stream);

/* ---- iSTFT synthesis: spec/phase [B][N/2+1][M] each (spec = exp(.), phase = sin(.) already
 * applied by the conv_post epilogue) -> wave [B][hop*(M-1)].
 * Replaces Modules/istftnet.py:99-104,380. */
int st2_istft(const float* sp, int64_t sp_bs, int32_t sp_cs, int32_t B, int32_t M,
              int32_t n_fft, int32_t hop, float* wave, int64_t wave_bs, void* stream);
/* Ragged rows (ABI v23): row b has m_len[b] (2..M) frames: it emits hop * (m_len[b] - 1) samples normalised by the window sum
 * of that length, and exact zeros up to hop * (M - 1). */
int st2_istft_len(const float* sp, int64_t sp_bs, int32_t sp_cs, int32_t B, int32_t M,
                  int32_t n_fft, int32_t hop, float* wave, int64_t wave_bs, const int32_t* m_len, void* stream);
/* Per-row lengths of a ragged batch (ABI v23): out[i][b] = (coef[3i] * f_b + coef[3i + 1]) / coef[3i + 2] for i < n <= 16,
 * f_b = frames[b] clamped to 1..T_max (integer arithmetic, floor division; coef on the HOST, copied at launch; frames / out
 * int32 on the device). */
int st2_ragged_lengths(const int32_t* frames, int32_t B, int32_t T_max, int32_t n, const int32_t* coef, int32_t* out,
                       void* stream);

/* ---- denoiser helpers (tokens channel-major: x[b][c][n]) ------------------------------ */
/* Multi-head attention without mask: q,k,v [B][H*D][N] -> o [B][H*D][N], softmax(q^T k * scale) v.
 * Replaces Modules/diffusion/modules.py:523-535. */
int st2_attention(const float* q, const float* k, const float* v, int64_t bs, int32_t cs,
                  float* o, int64_t o_bs, int32_t o_cs,
                  int32_t B, int32_t H, int32_t D, int32_t N, float scale, void* stream);

/* Same with key padding: keys m >= key_len[b] are excluded from the softmax of every query of utterance b (the HF
 * additive -inf attention mask of a right-padded batch, Utils/PLBERT/util.py:8-11 -> AlbertAttention); key_len may be
 * NULL (= st2_attention).  key_len: int32 [B] on the device, every entry >= 1. */
int st2_attention_keylen(const float* q, const float* k, const float* v, int64_t bs, int32_t cs,
                         float* o, int64_t o_bs, int32_t o_cs,
                         int32_t B, int32_t H, int32_t D, int32_t N, float scale, const int32_t* key_len, void* stream);

/* ---- LayerNorm over channels, applied: y[b,c,l] = act( (x[b,c,l] - mean[b,l]) * rstd[b,l] * G[b,c] + Bt[b,c] ),
 * G = gamma[b*gb_bs + c] (+1 if gamma_plus_one), stats [B][L][2] from st2_colnorm_stats; act NONE or LEAKY(slope);
 * positions l >= len[b] are written as 0 when len != NULL (the masked_fill_ after each block of the text encoders).
 * Replaces nn.LayerNorm / AdaLayerNorm applications whose result is needed as a tensor (residual inputs): ALBERT
 * post-LN blocks, models.py:270-282,308-312 (TextEncoder), :418-438,547-556 (DurationEncoder). */
int st2_colnorm_apply(const float* x, int64_t x_bs, int32_t x_cs, const float* stats, const float* gamma,
                      const float* beta, int64_t gb_bs, int32_t gamma_plus_one, int32_t act, float slope,
                      const int32_t* len, float* y, int64_t y_bs, int32_t y_cs,
                      int32_t B, int32_t C, int32_t L, void* stream);

/* ---- bidirectional LSTM recurrence (hidden size H = 256) ------------------------------------- *
 * G [B][2*4H][N]: input projections W_ih x_t + b_ih + b_hh for both directions (rows 0..4H-1 forward,
 * 4H..8H-1 reverse; PyTorch gate order i,f,g,o), produced by st2_conv1d (k=1).  whh_t [2][H][4H] is
 * W_hh transposed per direction.  lengths [B] int32 (NULL = all N): packed-sequence semantics, outputs
 * beyond the length are zero; a device length is clamped to 0..N where it is read (both kernels), so a bad value
 * gives an all-zero or a full row, never an access outside the row.  Y [B][2H][N] (rows 0..H-1 forward h_t, H..2H-1 reverse).
 * Replaces nn.LSTM(bidirectional=True) + pack/pad: models.py:300,314-327 (TextEncoder),
 * :450,523-528,545-566 (duration LSTM / DurationEncoder), :453,498 (shared F0/N LSTM). */
int st2_lstm_bidir(const float* G, int64_t g_bs, int32_t g_cs, const float* whh_t, const int32_t* lengths,
                   int32_t B, int32_t H, int32_t N, float* Y, int64_t y_bs, int32_t y_cs, void* stream);

/* Cooperative form of the same recurrence: W_hh stays in registers, split over 8 workgroups (CUs) per group of up to
 * 8 utterances of one direction, which exchange the new hidden state once per step through `scratch` (agent-scope
 * release/acquire on a monotonic counter).  ~5x lower latency per step than st2_lstm_bidir, same results up to fp32
 * summation order.  `scratch` (256-byte aligned, >= st2_lstm_coop_scratch_bytes(B) bytes, contents irrelevant) is
 * zeroed and used by the call; scratch[0..3] holds an int32 status afterwards (0 = ok, 1 = a bounded spin timed out
 * and the outputs are invalid).  st2_lstm_coop_scratch_bytes returns 0 when B is too large for one co-resident
 * launch (B > 48): use st2_lstm_bidir. */
int64_t st2_lstm_coop_scratch_bytes(int32_t B);
/* Hand-off variant (process-wide): 2 (default) = the data is the flag: every new hidden value travels as ONE 8-byte
 * agent-scope store {step tag, value} and the consumers re-read their granules until every tag matches -- one fabric
 * round trip per step, no counter, no cache maintenance; 0 = plain stores/loads bracketed by agent-scope release /
 * acquire fences around a monotonic counter (three round trips); 1 = sc1 atomic stores/loads + the counter.
 * A time-out also raises ST2_STATUS_LSTM_TIMEOUT in st2_status().  st2_lstm_bidir_coop refuses (returns non-zero)
 * when the device cannot hold the launch's workgroups co-resident (occupancy query): use st2_lstm_bidir then. */
int st2_lstm_coop_set_exchange(int mode);
/* Polls a waiting workgroup makes before it gives up (process-wide; <= 0 restores the default of 2^22, seconds).
 * Tests set 1 to provoke ST2_STATUS_LSTM_TIMEOUT. */
int st2_lstm_coop_set_spin_limit(int polls);
/* Measurement hook (process-wide): utterances per cooperative group, 1 / 2 / 4 / 8; 0 (default) = chosen from the batch
 * size (4 up to 32 utterances, 8 up to 48); < 0 = no cooperative launches (st2_lstm_coop_scratch_bytes returns 0, the
 * plans take st2_lstm_bidir).  Smaller blocks trade CUs for less mat-vec work per step and workgroup. */
int st2_lstm_coop_set_block(int utterances);
int st2_lstm_bidir_coop(const float* G, int64_t g_bs, int32_t g_cs, const float* whh_t, const int32_t* lengths,
                        int32_t B, int32_t H, int32_t N, float* Y, int64_t y_bs, int32_t y_cs,
                        void* scratch, int64_t scratch_bytes, void* stream);
/* The same launch with its safety net (ABI v20; what every launch plan issues): the single-CU kernel of st2_lstm_bidir is
 * queued behind the cooperative launch in a CONDITIONAL form -- every workgroup reads scratch[0] and leaves when it is 0 (a
 * few microseconds); when a group was not co-resident in time (another queue held its CUs) it re-runs the whole call into
 * the same Y.  The outputs are then the single-CU kernel's (same results up to fp32 summation order), ST2_STATUS_LSTM_TIMEOUT
 * is NOT raised and ST2_STATUS_LSTM_RECOVERED is.  Same refusal behaviour as st2_lstm_bidir_coop (nothing launched); legal
 * under stream capture. */
int st2_lstm_bidir_coop_recovering(const float* G, int64_t g_bs, int32_t g_cs, const float* whh_t, const int32_t* lengths,
                                   int32_t B, int32_t H, int32_t N, float* Y, int64_t y_bs, int32_t y_cs,
                                   void* scratch, int64_t scratch_bytes, void* stream);

/* generic fused elementwise helpers used by the sampler / denoiser glue */
/* y[b][c][n] = x[b][c][n] + v[b][c]  (x = x + mapping, modules.py:152,394) */
int st2_add_chanvec(const float* x, int64_t x_bs, int32_t x_cs, const float* v, int64_t v_bs,
                    float* y, int64_t y_bs, int32_t y_cs, int32_t B, int32_t C, int32_t N, void* stream);
/* m[b][c] = mean_n x[b][c][n]  (modules.py:155,397) */
int st2_mean_tokens(const float* x, int64_t x_bs, int32_t x_cs, float* m, int64_t m_bs,
                    int32_t B, int32_t C, int32_t N, void* stream);
/* Same over the first len[b] tokens only (int32 [B] on the device, NULL = all N): a right-padded batch then gives
 * every utterance the result of its own un-padded run (the reference runs one utterance at a time,
 * Demo/Inference_LJSpeech.ipynb:268-290). */
int st2_mean_tokens_len(const float* x, int64_t x_bs, int32_t x_cs, float* m, int64_t m_bs,
                        int32_t B, int32_t C, int32_t N, const int32_t* len, void* stream);
/* four[b] = [t, sin(t w_j 2 pi) (j < H2), cos(t w_j 2 pi) (j < H2)], out [B][1 + 2*H2]: LearnedPositionalEmbedding of the
 * denoiser's time input t = c_noise (Modules/diffusion/modules.py:657-671; op order ((t*w)*2)*pi in fp32). */
int st2_time_features(float t, const float* w, int32_t H2, int32_t B, float* out, void* stream);
/* y[b][e][n] = emb[b][n][e]  (b*e_bs + n*E + e): token-major embedding -> channel-major rows of a [B][.][N] tensor
 * (y points at the first destination row); e_bs = 0 broadcasts one [N][E] table (the fixed embedding of the
 * classifier-free-guidance branch, modules.py:412-423) over the batch.  Replaces rearrange / cat, modules.py:388-393. */
int st2_tokens_to_channels(const float* e, int64_t e_bs, int32_t B, int32_t N, int32_t E, float* y, int64_t y_bs,
                           int32_t y_cs, void* stream);
/* y[b][c][n] = x[b*x_bs + c] for n < N  (the noisy style vector repeated over the tokens, modules.py:388-390) */
int st2_broadcast_cols(const float* x, int64_t x_bs, float* y, int64_t y_bs, int32_t y_cs, int32_t B, int32_t C,
                       int32_t N, void* stream);
/* strided NCL copy y[b][c][l] = x[b][c][l] (channel slices of concatenation buffers, tap points) */
int st2_copy_ncl(const float* x, int64_t x_bs, int32_t x_cs, float* y, int64_t y_bs, int32_t y_cs, int32_t B, int32_t C,
                 int32_t L, void* stream);

/* y[b][e][n] = n < len[b] ? (table[tokens[b][n]][e] + add[e]) + pos[n][e] : 0  (tokens int64 [B][N], table [V][E]; add [E]
 * and pos [>= N][E] optional; len int32 [B] or NULL; token ids outside [0, V) contribute 0): nn.Embedding + transpose +
 * masked_fill of TextEncoder.forward (models.py:302-306), and -- with add = token-type row 0, pos = the position table --
 * the embedding sum of the ALBERT model behind PL-BERT (Utils/PLBERT/util.py:6-12; HF AlbertEmbeddings). */
int st2_embed_tokens(const int64_t* tokens, int32_t B, int32_t N, const float* table, int32_t V, int32_t E,
                     const float* add, const float* pos, const int32_t* len, float* y, int64_t y_bs, int32_t y_cs,
                     void* stream);
/* x[b][c][l] = 0 for l >= len[b] (int32 [B] on the device): the masked_fill_ the reference applies after every block of
 * the text-side modules (models.py:308-312, 547-556). */
int st2_mask_tail(float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t L, const int32_t* len, void* stream);

/* ---- duration head and alignment expansion (the notebooks' glue between predictor and decoder) ----------------- *
 * st2_duration_head: x [B][K][N] channel-major output of the duration BiLSTM, w [J][K] / bias [J] = duration_proj
 * (models.py:450-451); dur[b][n] (int64) = max(1, round(sum_j sigmoid(w_j . x[b,:,n] + bias_j))), 0 for n >= len[b]
 * (len NULL = no padding), + `tail` frames on token len[b]-1 (5 in the LJSpeech notebook, 0 in the LibriTTS one);
 * dsum (optional, [B][N]) receives the un-rounded sums.  Replaces Demo/Inference_LJSpeech.ipynb:296-301.
 * st2_expand_by_durations: y[b][c][t] = x[b][c][idx(b,t)], idx = the phoneme whose frames cover t (every row of dur
 * sums to T; N <= 512); shift = 1 applies the HiFi-GAN one-frame right shift of Demo/Inference_LibriTTS.ipynb:306-319.
 * Replaces the one-hot alignment matrix + matmul, Demo/Inference_LJSpeech.ipynb:303-312. */
int st2_duration_head(const float* x, int64_t x_bs, int32_t x_cs, const float* w, const float* bias, int32_t B,
                      int32_t K, int32_t J, int32_t N, const int32_t* len, int32_t tail, int64_t* dur, float* dsum,
                      void* stream);
int st2_expand_by_durations(const float* x, int64_t x_bs, int32_t x_cs, const int64_t* dur, int32_t B, int32_t C,
                            int32_t N, int32_t T, int32_t shift, float* y, int64_t y_bs, int32_t y_cs, void* stream);
/* Ragged rows (ABI v23): row b's durations sum to len[b] <= T (int32 [B] on the device, NULL = T); columns from len[b] on
 * are exact zeros. */
int st2_expand_by_durations_len(const float* x, int64_t x_bs, int32_t x_cs, const int64_t* dur, int32_t B, int32_t C,
                                int32_t N, int32_t T, int32_t shift, float* y, int64_t y_bs, int32_t y_cs, const int32_t* len,
                                void* stream);

/* ---- sync-free synthesis: device frame counts and packed PCM (added under ABI 23, additive: two kernel-level entry
 * points, no new backend-table slot, no struct change) ------------------------------------------------------------- *
 * A caller that states a frame CAPACITY T_cap (the longest utterance it accepts) needs no host read of the predicted
 * durations: the frame counts stay on the device from the duration head to the packed samples.
 *
 * st2_frames_from_durations: frames[b] = clamp(sum_{n < len[b]} dur[b][n], 1, T_cap)  (dur int64 [B][N], N <= 512; len int32
 * [B] on the device, clamped to 0..N, NULL = N; frames int32 [B]).  A row whose sum exceeds T_cap raises
 * ST2_STATUS_FRAME_CAPACITY; that row is then synthesised truncated to its first T_cap frames (st2_expand_by_durations_len
 * clamps the same way and raises ST2_STATUS_DURATION_SUM).  One launch, no allocation, no synchronisation.  NULL dur /
 * frames, B <= 0, N <= 0, N > 512 or T_cap <= 0 return non-zero before any launch. */
int st2_frames_from_durations(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, int32_t T_cap, int32_t* frames,
                              void* stream);

/* st2_wave_pack: the valid samples of a ragged batch of waveforms as ONE contiguous buffer.  Row b (at wave + b * w_bs,
 * w_bs >= samples_per_frame * T_cap) contributes n_b = max(0, samples_per_frame * f_b - trim) samples, f_b = frames[b]
 * clamped to 0..T_cap (a row of no frames contributes nothing); offsets (int64 [B + 1], device) receives the exclusive prefix sum of n_b,
 * offsets[B] the total; out[offsets[b] + i] = cvt(wave[b][i]) for i < n_b:
 *   ST2_PACK_F32  a bit copy (out is float);
 *   ST2_PACK_S16  (int16_t) rint(clamp(x, -1, 1) * 32767.0f), round-to-nearest-even; a NaN sample gives 0 (out is int16_t).
 * `out_capacity` is in SAMPLES: nothing at or past min(offsets[B], out_capacity) is written (offsets still describes the
 * untruncated layout), and nothing of `wave` at or past samples_per_frame * f_b is read -- the ragged decoder's tails may
 * hold anything.  trim: samples dropped from every row's end (the notebooks' HiFi-GAN tail).  Two launches (scan, move), no
 * allocation, no synchronisation; the move stores 16 bytes per lane on the aligned body of every row and peels head and
 * tail.  Bad arguments (NULL wave / frames / out / offsets, B <= 0 or > 65535, T_cap <= 0, samples_per_frame <= 0, trim < 0,
 * out_capacity < 0, unknown fmt, w_bs too small) return non-zero before any launch. */
enum st2_pack_format { ST2_PACK_F32 = 0, ST2_PACK_S16 = 1 };
int st2_wave_pack(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                  int32_t samples_per_frame, int32_t trim, int32_t fmt, void* out, int64_t out_capacity, int64_t* offsets,
                  void* stream);

/* ---- output sample rates and G.711 in the packed hand-over (added under ABI 23, additive: one kernel-level entry point, no
 * new backend-table slot, no struct change; st2_wave_pack and its format codes are untouched) -------------------------- *
 * st2_wave_resample_pack: st2_wave_pack with a rational polyphase resampler in it.  U = up, D = down, K = taps_per_phase,
 * taps fp32 [U][K] on the device.  Row b has n_b = max(0, samples_per_frame * f_b - trim) input samples (f_b = frames[b]
 * clamped to 0..T_cap: st2_wave_pack's rule) and m_b = (n_b U + D - 1) div D output samples; offsets (int64 [B + 1], device)
 * receives the exclusive prefix sum of m_b.  For j < m_b, with c = (j D) div U and p = (j D) mod U,
 *     y[j] = sum_{k = 0}^{K - 1} taps[p][k] * x_b[c - (K - 1) div 2 + k],      x_b[i] = 0 for i < 0 or i >= n_b,
 * accumulated in fp32 with fmaf, k ascending -- the result does not depend on how the kernel tiles a row.  The zero is a
 * SELECT: nothing of `wave` at or past n_b is read (the ragged decoder's tails may hold NaN bit patterns).
 * out[offsets[b] + j] = cvt(y[j]):
 *   ST2_PCM_F32   y (out is float);
 *   ST2_PCM_S16   st2_wave_pack's 16-bit rule: (int16_t) rint(clamp(y, -1, 1) * 32767.0f), NaN -> 0 (out is int16_t);
 *   ST2_PCM_ULAW / ST2_PCM_ALAW   ITU-T G.711 of that 16-bit sample, one byte each (out is uint8_t).
 * `out_capacity` is in output SAMPLES: nothing at or past min(offsets[B], out_capacity) is written (offsets still describes
 * the untruncated layout).  Two launches (scan, move), no allocation, no synchronisation; one workgroup per (tile of output
 * samples, row) stages the phase table and the tile's input span in static LDS (63 KiB) and stores 16 bytes per lane on the
 * aligned body of the destination, head and tail peeled.  Returns non-zero before any launch on: every condition of
 * st2_wave_pack; NULL taps; up / down outside 1..1024; taps_per_phase outside 1..512; unknown fmt; out misaligned for its
 * sample type; a table that leaves no room in LDS for a 16-sample tile. */
enum st2_pcm_format { ST2_PCM_F32 = 0, ST2_PCM_S16 = 1, ST2_PCM_ULAW = 2, ST2_PCM_ALAW = 3 };
int st2_wave_resample_pack(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                           int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                           int32_t taps_per_phase, int32_t fmt, void* out, int64_t out_capacity, int64_t* offsets, void* stream);

/* ---- passages: breaks behind the rows of the packed hand-over (added under ABI 23, additive: one kernel-level entry point, no
 * new backend-table slot, no struct change) ------------------------------------------------------ *
 * st2_wave_pack_gaps: st2_wave_pack / st2_wave_resample_pack with g_b samples of silence behind row b -- the rows of a batch
 * as the sentences of one passage, with SSML's <break> / <s> / <p> between them, in the hand-over's own rate and format.
 *   m_b   the row's sample count by the wrapped entry's rule.  taps != NULL: st2_wave_resample_pack's m_b = (n_b U + D - 1)
 *         div D.  taps == NULL: the caller passes up == down == 1 and fmt ST2_PCM_F32 or ST2_PCM_S16 (the codes of
 *         ST2_PACK_F32 / ST2_PACK_S16), m_b = st2_wave_pack's n_b and its move kernel does the work.
 *   g_b = clamp(gaps[b], 0, gap_cap), in OUTPUT samples; gaps int32 [B] on the device (a negative value gives 0).  gaps ==
 *         NULL or gap_cap == 0: no gaps, and the call IS the wrapped entry (its two launches, its bytes).
 *   offsets[b] = sum_{i < b} (m_i + g_i) (int64 [B + 1], device; 64-bit sums); offsets[B] the total, the last row's gap included.
 *   out[offsets[b] + j], j < m_b: byte for byte what the wrapped entry writes for that row (its move kernel, unchanged).
 *   out[offsets[b] + m_b + j] = cvt(0.0f), j < g_b: what the format's encoder gives for a zero sample -- 0.0f, 0, or the G.711
 *         mu-law / A-law code of 0 (0xFF / 0xD5: silence is not byte 0 there).
 * Nothing at or past min(offsets[B], out_capacity) is written (the bound may fall inside a gap), every element below it is
 * written exactly once, and nothing of `wave` at or past a row's valid samples is read.  Three launches (gap-aware scan, move,
 * fill), no allocation, no synchronisation: legal under stream capture.  The fill is one workgroup per (chunk, row), its grid
 * sized by gap_cap and its work by g_b (a workgroup whose chunk lies past its gap's end leaves at once); it stores 16 bytes
 * per lane on the aligned body of the gap and peels head and tail.  Returns non-zero before any launch on: every refusal of the
 * entry it wraps; gap_cap < 0; taps == NULL together with up / down != 1 or a G.711 format; gaps misaligned for int32. */
int st2_wave_pack_gaps(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                       int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                       int32_t taps_per_phase, int32_t fmt /* st2_pcm_format */, const int32_t* gaps, int32_t gap_cap,
                       void* out, int64_t out_capacity, int64_t* offsets, void* stream);

/* ---- loudness-normalised hand-over: BS.1770 level and per-row gain (added under ABI 23, additive: two kernel-level entry
 * points and a size helper, no new backend-table slot, no struct change, no new sticky status bit) -- *
 * st2_wave_level: per-row integrated loudness (ITU-R BS.1770-4) and sample peak of a ragged batch at the model rate, and the
 * per-row linear gain that brings the row to a target loudness without passing a peak ceiling.
 *  1. Valid samples.  Row b has x[0 .. n_b), n_b = max(0, samples_per_frame * f_b - trim), f_b = frames[b] clamped to 0..T_cap
 *     (st2_wave_pack's rule); nothing of `wave` at or past n_b is read.  A non-finite sample counts as 0.
 *  2. K-weighting: two biquads in cascade from zero state at x[0], in fp64 -- the high shelf and the high pass of BS.1770-4,
 *     their coefficients derived on the host in double for `sample_rate` from the analog prototypes by the bilinear transform
 *     (at 48 kHz the standard's table).
 *  3. Blocks.  The hop is h = sample_rate / 10 samples; e_j = sum y^2 over hop j; block k covers four hops, z_k = (e_k + ... +
 *     e_{k+3}) / (4 h), for every k with (k + 4) h <= n_b.  A row with n_b < 4 h has one block, the whole row: z_0 = sum y^2 / n_b;
 *     a row with n_b = 0 has none.  l_k = -0.691 + 10 log10 z_k.
 *  4. Gates.  Absolute: l_k > -70.  Relative: l_k > -0.691 + 10 log10(mean of z over the absolutely gated blocks) - 10.
 *     L_b = -0.691 + 10 log10(mean of z over the blocks that pass both); -inf if none does.
 *  5. Gain.  peak_b = max |x| over the valid, finite samples;  g_b = min(10^((target[b] - L_b) / 20), 10^(max_gain_db / 20),
 *     ceiling / peak_b) in fp64, rounded once to fp32; exactly 1.0f where target[b] is NaN (the row is left alone), where
 *     L_b = -inf or where peak_b = 0.
 *  6. Report.  level[b] = {L_b, peak_b, g_b, number of blocks that passed both gates}, four fp32 values (level fp32 [B][4]).
 * A lane of the measuring kernel starts its fp64 chain from zero state W = 4 ceil(0.032 sample_rate) samples early (or at the
 * row's first sample, then exactly): a block's energy is off by at most 2 T peak_b / sqrt(z_k) relative, T = 1.2e-12 -- 7.0e-9
 * for a block above the absolute gate of a row that peaks at full scale.  Sums are made in a fixed order without atomics: a
 * row's four values depend neither on the tiling nor on the row's place in the batch, bit for bit.
 * `workspace` (8-byte aligned, st2_wave_level_workspace_bytes(B, T_cap, samples_per_frame, sample_rate) bytes; 0 for an
 * argument <= 0 or a rate that is no multiple of 10) holds the fp64 hop energies [B][ceil(samples_per_frame T_cap / h)] and the
 * hops' peaks.  Two launches (hop energies and peaks; gates and gain), no allocation, no synchronisation, no host read: legal
 * under stream capture.  Returns non-zero before any launch on: every geometry refusal of st2_wave_pack (NULL wave / frames,
 * B <= 0 or > 65535, T_cap <= 0, samples_per_frame <= 0, trim < 0, w_bs too small); NULL target / level / workspace; a workspace
 * that is too small or misaligned; sample_rate <= 0 or not a multiple of 10, or so high that a hop does not fit LDS; ceiling
 * outside (0, 1]; max_gain_db outside [0, 60]; wave / target / level misaligned for float.
 *
 * st2_wave_pack_level: st2_wave_pack_gaps with the gain in its moves.  level == NULL: the call IS st2_wave_pack_gaps, its
 * launches and its bytes.  Otherwise every valid input sample of row b becomes fl32(x * level[b][2]) -- one fp32 multiply as
 * the sample is loaded, before anything else the move does -- so that the packed output is exactly what st2_wave_pack_gaps
 * writes for the input fl32(x * g_b); gaps stay the format's silence code and sample counts do not change.  Returns non-zero
 * before any launch on every refusal of st2_wave_pack_gaps and on a level misaligned for float.
 *
 * st2_wave_level_ex: st2_wave_level with a true-peak ceiling and / or one gain per passage (additive under ABI 23).  It takes
 * st2_wave_level's arguments and, behind the stream, `taps` (fp32 [up][taps_per_phase] on the device; NULL = sample peaks) and
 * `start` (int32 [B] on the device; NULL = every row its own group).  With both NULL the call IS st2_wave_level: its two
 * launches, its bytes, its refusals under its name.
 *  True peak (ITU-R BS.1770-4 Annex 2: the peak of the signal oversampled to at least 192 kHz -- up = 8 at 24 kHz).  With
 *     U = up, K = taps_per_phase and the row's cleaned samples x (rule 1; x = 0 in front of the row and at or past n_b),
 *         y[j] = sum_{k = 0}^{K - 1} taps[j mod U][k] * x[j div U - (K - 1) div 2 + k]      for j in [0, U n_b)
 *     -- st2_wave_resample_pack's sum with down = 1, the same fp32 fmaf chain from 0, k ascending -- and
 *         tp_b = max(peak_b, max_j |y[j]|);   tp_b = 0 for an empty or all-zero row.
 *     The sample peak stays in the maximum: phase 0 of a table whose cutoff lies below Nyquist is not the identity, and the
 *     reading must never fall below st2_wave_level's.  tp_b takes peak_b's place in rule 5, and level[b][1] reports it.  A
 *     maximum does not depend on order: tp_b depends neither on the tiling nor on the row's place in the batch, bit for bit.
 *     Limit of the measurement: a steady sine of frequency f reads at least cos(pi f / (U sample_rate)) of its crest (0.9952
 *     at a quarter of the rate with U = 8), less the table's passband ripple; content in the table's transition band (with
 *     the package's table: 0.85 to 1.0 of Nyquist, 10.2 to 12 kHz) is attenuated by the table and under-read.  The peak is the
 *     model-rate signal's: what a resampling hand-over or a G.711 conversion adds behind it is not covered.
 *  Passage scope.  A group is a row with start[b] != 0 and the rows with start[b] == 0 behind it; row 0 begins a group
 *     whatever its flag.  The group's blocks are the blocks of its rows, each row's by rule 3 from zero filter state at its own
 *     x[0], in row order; blocks never span two rows.  Both gates and L run over that one list; the peak (sample or true) is
 *     the maximum over the group's rows; the target is the group's first row's (NaN = the whole group is left alone).  Every row
 *     of the group gets the same four values {L_group, peak_group, g_group, blocks passed in the group}, bit for bit; a group
 *     of one row is st2_wave_level's row, bit for bit.
 * With `taps` one launch more, between the two: one workgroup per (hop, row) stages the table and the hop's span (K - 1 samples
 * of halo) in LDS, every lane makes all U phases of its input positions, and one lane folds the hop's maximum into the hop's
 * peak slot -- the workspace is st2_wave_level's (st2_wave_level_ex_workspace_bytes forwards).  Returns non-zero before any
 * launch, under its own name, on: every refusal of st2_wave_level; with `taps`, up outside 1..1024, taps_per_phase outside
 * 1..512, a table that does not fit LDS beside one hop, taps misaligned for float; start misaligned for int32. */
int64_t st2_wave_level_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame, int32_t sample_rate);
int st2_wave_level(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                   int32_t trim, int32_t sample_rate, const float* target /* fp32 [B], device */, double ceiling,
                   double max_gain_db, float* level /* fp32 [B][4], device */, void* workspace, int64_t workspace_bytes,
                   void* stream);
int st2_wave_pack_level(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                        int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                        int32_t taps_per_phase, int32_t fmt /* st2_pcm_format */, const int32_t* gaps, int32_t gap_cap,
                        void* out, int64_t out_capacity, int64_t* offsets, void* stream, const float* level);
int64_t st2_wave_level_ex_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame, int32_t sample_rate);
int st2_wave_level_ex(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                      int32_t trim, int32_t sample_rate, const float* target, double ceiling, double max_gain_db, float* level,
                      void* workspace, int64_t workspace_bytes, void* stream, const float* taps /* fp32 [up][taps_per_phase] */,
                      int32_t up, int32_t taps_per_phase, const int32_t* start /* int32 [B], device */);

/* ---- look-ahead peak limiter of the hand-over (added under ABI 23, additive: one kernel-level entry point and two helpers, no
 * new backend-table slot, no struct change, no new sticky status bit) ---------------------------------- *
 * st2_wave_limit: the rows of st2_wave_level_ex, driven above the ceiling by up to drive_db and brought back under it by a
 * zero-phase gain that is a sliding minimum (the hold) under an FIR smoother.  It takes what st2_wave_level_ex took -- the same
 * wave, frames, trim, target, ceiling (c below), max_gain_db, start and taps [U = up][K = taps_per_phase], NULL as there -- and
 * the `level` table that call wrote (read, never modified), drive_db in [0, 24], a half window W in samples, 1..1024, and `win`,
 * fp32 [2 W + 1] on the device, non-negative and summing to 1.  Row b's valid samples are st2_wave_level's rule 1: x[0 .. n_b),
 * cleaned (a non-finite sample counts as 0).
 *  1. Drive gain.  g'_b = min(10^((t - L) / 20), 10^(max_gain_db / 20), 10^(drive_db / 20) * c / peak) in fp64, rounded once to
 *     fp32; L = level[b][0] and peak = level[b][1] as they stand there in fp32, t the target of the first row of b's group
 *     (start as in st2_wave_level_ex; NULL = every row its own group).  Where t is NaN, L = -inf or peak = 0 the row is LEFT
 *     ALONE: its valid samples are copied bit for bit, NaN payloads intact, and limit[b] = {1, 1}.  drive_db bounds how deep
 *     the limiter ever digs: q >= 10^(-drive_db / 20) up to rounding wherever `peak` covers the envelope.
 *  2. Envelope.  e[i] = |x[i]|; with taps, e[i] = max(|x[i]|, max_{p < U} |y[U i + p]|), y st2_wave_level_ex's interpolation
 *     (the same fp32 fmaf chain from 0, k ascending).
 *  3. Required gain.  r[i] = min(1, c / (e[i] g'_b)) evaluated in fp64 and rounded once to fp32; 1 where e[i] = 0 and 1 for i
 *     outside [0, n_b).
 *  4. Hold.  m[j] = min_{|d| <= W} r[j + d].
 *  5. Smooth.  s[i] = 1 - sum_{k = 0}^{2 W} win[k] * (1 - m[i - W + k]): 1 - m in fp32, the sum an fp32 fmaf chain from 0, k
 *     ascending, the last difference in fp32.  Every window of m that s[i] reads contains i, so s[i] <= r[i] up to the rounding
 *     of sum win; q[i] = min(s[i], r[i]) makes that exact.
 *  6. Output.  out[i] = fl32(fl32(x[i] * g'_b) * q[i]) for i in [0, n_b), fp32 in wave's layout (row stride w_bs); nothing at or
 *     past n_b is written.  limit[b] = {g'_b, min_i q[i]} (fp32 [B][2]; 1 for a row without samples).
 * Every output sample is a function of the 4 W + 1 samples around it and a minimum does not depend on order: a row's output and
 * its two numbers depend neither on the tiling nor on the row's place in the batch, bit for bit.
 * `workspace` (float-aligned, st2_wave_limit_workspace_bytes(B, T_cap, samples_per_frame) bytes; 0 for an argument <= 0) begins
 * with r as fp32 [B][samples_per_frame T_cap] (entries [0, n_b) of a row that is not left alone), followed by the tiles' minima
 * and the rows' gains.  st2_wave_limit_tile(): the samples of a tile.  Four launches (gain; envelope and r; hold, smoother and
 * product; the rows' minima), no allocation, no synchronisation, no host read: legal under stream capture.  Returns non-zero
 * before any launch on: every refusal of st2_wave_level_ex about geometry (NULL wave / frames, B <= 0 or > 65535, T_cap <= 0,
 * samples_per_frame <= 0, trim < 0, w_bs too small), ceiling, max_gain_db and, with taps, the table; NULL or misaligned level /
 * target / out / limit / win / workspace, misaligned taps / start; out overlapping wave; a workspace that is too small; W outside
 * 1..1024; drive_db outside [0, 24]; a tile whose halo does not fit LDS. */
int32_t st2_wave_limit_tile(void);
int64_t st2_wave_limit_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame);
int st2_wave_limit(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                   int32_t trim, const float* target /* fp32 [B], device */, double ceiling, double max_gain_db,
                   const float* level /* fp32 [B][4] of st2_wave_level(_ex) */, const float* taps /* fp32 [up][taps_per_phase] */,
                   int32_t up, int32_t taps_per_phase, const int32_t* start /* int32 [B], device */, double drive_db, int32_t W,
                   const float* win /* fp32 [2 W + 1], device */, float* out, float* limit /* fp32 [B][2], device */,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* ---- edges: lead and tail silence trimmed on the way out (added under ABI 23, additive: two kernel-level entry points and two
 * helpers, no new backend-table slot, no struct change, no new sticky status bit) ------------------------ *
 * st2_wave_edges: the way out's counterpart of st2_clip_ingest's trim.  It takes st2_wave_level's geometry (wave, w_bs, frames,
 * B, T_cap, samples_per_frame, trim) and, all on the device and read by the kernels -- a captured launch serves any values --
 * top_db fp32 [B], keep int32 [B][2] (samples of lead and of tail to keep outside the detected bounds) and ramp fp32 [F],
 * F in 0..4096 (NULL with F = 0), rising and non-negative; it writes `out`, fp32 in wave's layout (row stride w_bs), not
 * overlapping wave, and edges int32 [B][2].
 *  1. Valid samples.  Row b's valid samples are st2_wave_level's rule 1: x[0 .. n_b), n_b = max(0, frames[b] * samples_per_frame
 *     - trim), frames clamped to 0..T_cap.  A non-finite sample counts as 0 for the measurement.
 *  2. Detection.  Rule 3 of st2_clip_ingest, verbatim, over the row's n_b samples with top_db[b]: 2048-sample frames with hop
 *     512, centred and zero-padded, f = 0 .. n_b div 512; e_f = max(sum / 2048, 1e-10) from the sums of squares of the row's
 *     512-sample blocks -- every block by one wave, lane l the samples l, l + 64, ... ascending by fmaf from 0, the 64 partial
 *     sums by a butterfly; e_f = ((s[f - 2] + s[f - 1]) + (s[f] + s[f + 1])) / 2048 in fp32 --; frame f is non-silent iff
 *     e_f > max_f e_f * (float) 10^(-top_db / 10) (the power in double, rounded once), the maximal frame whatever the rounding.
 *     start = 512 * the first non-silent frame, end = min(n_b, 512 * (the last one + 1)).  The row is LEFT ALONE (start = 0,
 *     end = n_b) where top_db[b] is NaN or <= 0 or the row is empty; an all-zero row has every frame at the floor, so every
 *     frame is the maximal one and the rule itself gives start = 0, end = n_b.
 *  3. Pads.  head = max(0, start - max(0, keep[b][0])), stop = min(n_b, end + max(0, keep[b][1])), count = stop - head, in
 *     integers (64-bit inside: no keep overflows).
 *  4. Move and fade.  out[b][i] = x[head + i] for i < count, the bits copied, NaN payloads included, except inside a fade: with
 *     F > 0 and f = min(F, count div 2) the first f samples are multiplied by ramp[i] only if head > 0, the last f by
 *     ramp[count - 1 - i] only if stop < n_b, each one fp32 multiply (f + f <= count: no sample takes both).  Nothing at or past
 *     out[b][count] is written.
 *  5. Result.  edges[b] = {head, count}.
 *  6. Independence.  The block sums have one fixed order, the maximum and the first / last frame do not depend on order, and
 *     the move accumulates nothing: a row's output and its two numbers depend neither on the tiling nor on the row's place in
 *     the batch, bit for bit.
 * `workspace` (float-aligned, st2_wave_edges_workspace_bytes(B, T_cap, samples_per_frame) bytes; 0 for an argument <= 0) holds
 * the block sums, fp32 [B][4 ceil(samples_per_frame T_cap / tile)].  st2_wave_edges_tile(): the samples of a tile of the sums'
 * launch.  Three launches (block sums; per row the maximum, the bounds and the pads; the move), no atomics, no allocation, no
 * synchronisation, no host read: legal under stream capture.  Returns non-zero before any launch on: NULL wave / frames, B <= 0
 * or > 65535, T_cap <= 0, samples_per_frame <= 0, trim < 0, a row at capacity beyond the int32 edges, w_bs too small; NULL
 * top_db / keep / out / edges / workspace; F outside 0..4096 or F > 0 with a NULL ramp; wave / top_db / out / ramp / workspace
 * misaligned for float, frames / keep / edges for int32; out overlapping wave; a workspace that is too small. */
int32_t st2_wave_edges_tile(void);
int64_t st2_wave_edges_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame);
int st2_wave_edges(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                   int32_t trim, const float* top_db /* fp32 [B], device */, const int32_t* keep /* int32 [B][2], device */,
                   const float* ramp /* fp32 [F], device */, int32_t F, float* out, int32_t* edges /* int32 [B][2], device */,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* st2_token_marks_edges: st2_token_marks for rows that st2_wave_edges cut before they were packed.  It takes st2_token_marks's
 * arguments and, in front of the stream, `edges` (int32 [B][2] on the device, {head, count} as st2_wave_edges wrote them; a
 * negative entry counts as 0).  The boundaries are st2_token_marks's, by the one boundary rule; with s = min(samples_per_frame *
 * bound[b][n], n_smp) as there, marks[b][n] = (clamp(s - head, 0, count) * up + down - 1) div down: a token that lies in the
 * removed lead sits at 0, one in the removed tail at the row's end, and marks[b][N] is still the row's packed sample count,
 * ceil(count up / down).  bound_out is st2_token_marks's, in decoder frames of the uncut row.  One launch.  Returns non-zero
 * before any launch on every refusal of st2_token_marks and on a NULL or misaligned edges. */
int st2_token_marks_edges(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* frames, int32_t T_cap,
                          int32_t shift, int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, int32_t* marks,
                          int32_t* bound_out, const int32_t* edges /* int32 [B][2], device */, void* stream);

/* ---- breaks: silence spliced into a row at token spans (added under ABI 23, additive: two kernel-level entry points and one
 * helper, no new backend-table slot, no struct change, no new sticky status bit) ------------------------- *
 * st2_wave_breaks: a pause INSIDE a row.  It takes st2_wave_edges's geometry (wave, w_bs, frames, B, T_cap, samples_per_frame,
 * trim) and its ramp (fp32 [F], F in 0..4096, NULL with F = 0), and, on the device and read by the kernels, pos int32 [B][N + 1]
 * (the tokens' boundaries in samples of THIS row: st2_token_marks(_edges) at up = down = 1) and brk int32 [B][N] (samples of
 * silence wanted inside token n; <= 0 = none); max_break is a host number, the most silence one row takes, and sizes the grids.
 * It writes `out` (fp32, row stride o_bs >= samples_per_frame T_cap + max_break, not overlapping wave), ins int32 [B][N], cuts
 * int32 [B][N] and breaks int32 [B][2].
 *  1. Valid samples.  Row b's valid samples are st2_wave_level's rule 1: x[0 .. n_b).  A non-finite sample counts as 0 for the
 *     measurement only.  The boundaries are q[0] = 0, q[N] = n_b, q[i] = clamp(pos[b][i], 0, n_b) otherwise, then made monotone
 *     by a running maximum, q[i] = max(q[i - 1], q[i]); token n's span is [q[n], q[n + 1]).
 *  2. Block energies.  s[k] is the sum of squares of the row's samples [64 k, 64 k + 64), zeros at and past n_b: lane l of a
 *     wave squares sample 64 k + l (one fp32 multiply), and the 64 squares are folded by a butterfly, t[l] += t[l ^ off] for
 *     off = 32, 16, ..., 1 in fp32.  The window energy is e_k = s[k - 1] + s[k] in fp32: 128 samples, 5.3 ms.
 *  3. Cut.  For token n with a break and span [p0, p1) the candidates are the k with 64 (k - 1) >= p0 and 64 (k + 1) <= p1; the
 *     cut is c = 64 k for the smallest e_k, the smallest such k among equal ones.  Without a candidate (a span that holds no
 *     aligned window, or an empty one) c = (p0 + p1) div 2.  p0 <= c <= p1, so the cuts of a row do not decrease.
 *  4. Cap.  In token order, with w_n = max(brk[b][n], 0): ins[b][n] = min(w_n, max_break - the silence inserted in front of
 *     token n) (the sum of the w in 64 bits).  ins[b][n] = 0 -- nothing asked for, or the cap reached -- makes no cut:
 *     cuts[b][n] = -1 and no fade; else cuts[b][n] = c.
 *  5. Move, fade and fill.  The m cuts of the row divide it into m + 1 segments (a segment between two equal cuts is empty).
 *     Every segment is copied, bit for bit, NaN payloads included, to its place plus the silence in front of it, and ins[b][n]
 *     samples of +0.0f follow cut n.  With f = min(F, (a segment's length) div 2), the last f samples of a segment that ends
 *     at a cut are multiplied by ramp[0 .. f) counted back from the cut, the first f samples of a segment that starts at one by
 *     ramp[0 .. f) counted from it: one fp32 multiply each, f + f <= the length, so no sample takes two.  The row's own ends
 *     are not faded (that is st2_wave_edges's).  count' = n_b + the silence inserted; nothing at or past out[b][count'] is
 *     written.  A row without a break is a bit copy of its n_b samples.
 *  6. Result.  breaks[b] = {count', the silence inserted}.
 *  7. Independence.  The block sums have one fixed order, the minimum and its tie rule do not depend on order, the scan is in
 *     integers and the move accumulates nothing: a row's output and its numbers depend neither on the tiling nor on the row's
 *     place in the batch, bit for bit.
 * `workspace` (float-aligned, st2_wave_breaks_workspace_bytes(B, T_cap, samples_per_frame, N) bytes; 0 for an argument <= 0 or
 * N > 512) holds the block sums and one segment table per row.  Three launches (block sums; per row the boundaries, the cap,
 * the cuts and the table; the move), no atomics, no allocation, no synchronisation, no host read: legal under stream capture.
 * Returns non-zero before any launch on every refusal of st2_wave_edges that applies (NULL wave / frames / out / workspace, bad
 * geometry, trim < 0, w_bs too small, F outside 0..4096 or F > 0 with a NULL ramp, misaligned wave / out / ramp / workspace or
 * frames, out overlapping wave, a workspace that is too small) and on: NULL or misaligned pos / brk / ins / cuts / breaks; N
 * outside 1..512; max_break < 0; o_bs too small; a row at capacity with max_break beyond the int32 counts. */
int64_t st2_wave_breaks_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame, int32_t N);
int st2_wave_breaks(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                    int32_t trim, const int32_t* pos /* int32 [B][N + 1], device */, const int32_t* brk /* int32 [B][N], device */,
                    int32_t N, int32_t max_break, const float* ramp /* fp32 [F], device */, int32_t F, float* out, int64_t o_bs,
                    int32_t* ins /* int32 [B][N], device */, int32_t* cuts /* int32 [B][N], device */,
                    int32_t* breaks /* int32 [B][2], device */, void* workspace, int64_t workspace_bytes, void* stream);
/* st2_token_marks_breaks: the timing marks of rows that st2_wave_breaks spliced silence into.  pos and ins as that entry read and
 * wrote them (a negative entry counts as 0): marks[b][n] = min(((pos[b][n] + sum_{m < n} ins[b][m]) * up + down - 1) div down,
 * INT32_MAX), in 64 bits, n = 0 .. N.  Token n's own break lies inside [marks[b][n], marks[b][n + 1]), and with pos[b][N] = n_b
 * marks[b][N] is the row's packed sample count, ceil(count' up / down).  One launch, one wave per row.  Returns non-zero before
 * the launch on a NULL or misaligned pos / ins / marks, B <= 0, N outside 1..512, up or down outside 1..1024. */
int st2_token_marks_breaks(const int32_t* pos, const int32_t* ins, int32_t B, int32_t N, int32_t up, int32_t down,
                           int32_t* marks /* int32 [B][N + 1], device */, void* stream);

/* ---- dynamics: a speech compressor in the hand-over (added under ABI 23, additive: one kernel-level entry point and three
 * helpers, no new backend-table slot, no struct change, no new sticky status bit) ------------------------ *
 * st2_wave_dynamics: the dynamic range of a row reduced by a feed-forward compressor with a soft knee, instant attack under a
 * zero-phase look-ahead, and a release that is linear in dB.  It takes st2_wave_edges's geometry (wave, w_bs, frames, B, T_cap,
 * samples_per_frame, trim) and, on the device and read by the kernels, params fp32 [B][4] = {threshold_db, slope, knee_db,
 * makeup_db} with slope = 1 - 1 / ratio; the kernels clamp slope to [0, 1], knee_db to [0, 40] and makeup_db to [-24, 24].  A
 * NaN in any of the four, or a threshold that is not finite, means the row is left alone.  Host numbers: the half window A in
 * blocks of 64 samples, 0..64; win fp32 [2 A + 1] on the device, non-negative weights that sum to 1 (NULL with A = 0, where the
 * smoother is the identity); the release rho > 0 in dB per block.  It writes `out` (fp32, row stride o_bs, not overlapping
 * wave), dyn fp32 [B][2] and the workspace.  With T, slope, Wk, makeup the row's clamped parameters as fp64:
 *  1. Valid samples.  st2_wave_level's rule 1: x[0 .. n_b).  A row that is left alone, or whose n_b = 0, is copied bit for bit,
 *     NaN payloads intact, and its dyn[b] = {0, 0}.
 *  2. Block sums.  st2_wave_breaks's rule 2, bit for bit and by the same kernel: s[k], k = 0 .. K - 1, K = ceil(n_b / 64); a
 *     non-finite sample counts as 0, zeros past n_b.  A sum that overflowed to +inf counts as FLT_MAX.
 *  3. Detector.  E[k] = fl32(fl32(s[k - 1] + s[k]) + s[k + 1]), a missing neighbour as 0, +inf as FLT_MAX; L[k] =
 *     10 log10((double)E[k] / 192) in fp64, -inf at E[k] = 0: a centred RMS over 192 samples, 8 ms.  The first block and the
 *     last, partial one are divided by 192 like the others: the edges of a row read up to 4.8 dB low, and never high.
 *  4. Static curve, fp64, o = L[k] - T: c[k] = 0 where 2 o <= -Wk; c[k] = (slope * (u * u)) / (2 Wk) with u = o + Wk / 2 where
 *     |2 o| < Wk; c[k] = slope * o otherwise (the soft knee of Giannoulis, Massberg and Reiss, JAES 2012).  c >= 0.
 *  5. Release.  g[k] = max_{m <= k} (c[m] - (k - m) rho), evaluated as g[k] = P[k] - fl64(k * rho) with P the running maximum
 *     of z[m] = c[m] + fl64(m * rho): one fp64 multiply and one add each, and a maximum has no rounding, so no result depends
 *     on how the scan is cut.
 *  6. Attack.  The hold m[k] = max_{|d| <= A} g[k + d], entries outside 0 .. K - 1 absent; the smoother d[k] = sum_j win[j]
 *     m[k - A + j] as the fp64 chain d = d + fl64((double)win[j] * m[.]) from 0 with j ascending, an entry outside the row
 *     taking the nearest valid one; d'[k] = max(d[k], g[k]).  Every window d[k] reads contains k, so no block is ever reduced
 *     by less than the release envelope -- and so the static curve -- asks.
 *  7. Gain per block.  lin[k] = fl32(10^((makeup - d'[k]) / 20)), pow in fp64, rounded once.
 *  8. Gain per sample, fp32: linear between the block centres 64 k + 31.5.  For sample i between the centres of blocks k and
 *     k + 1, t = (2 (i - 64 k) - 63) / 128 (exact) and gain = fmaf(t, lin[k + 1] - lin[k], lin[k]); in front of the first
 *     centre gain = lin[0], behind the last gain = lin[K - 1].  out[i] = fl32(x[i] * gain) on the valid samples, with x itself:
 *     a NaN stays a NaN.  Nothing at or past out[b][n_b] is written.
 *  9. Result.  dyn[b] = {max_k d'[k], the number of blocks with d'[k] > 0}, both as fp32: a maximum and a count, no sum across
 *     samples, no atomics.  A row's output and its two numbers depend neither on the tiling nor on the row's place in the
 *     batch, bit for bit.
 * A row whose level never reaches T - Wk / 2, with makeup = 0, has lin = 1 everywhere and comes out bit for bit; slope = 0 is
 * the identity times the make-up gain.  Everything is fixed but the last ulp of log10 and pow.
 * `workspace` (float-aligned, st2_wave_dynamics_workspace_bytes(B, T_cap, samples_per_frame) bytes; 0 for an argument <= 0)
 * begins with lin fp32 [B][Kcap], then s fp32 [B][Kcap], Kcap = ceil(samples_per_frame T_cap / 64); entries at or past a row's
 * K are not written.  st2_wave_dynamics_tile(): the samples of a tile of the apply launch; st2_wave_dynamics_chunk(): the
 * blocks of a chunk of the per-row launch.  Three launches (block sums; per row rules 3 to 7 and 9; apply), no atomics, no
 * allocation, no synchronisation, no host read: legal under stream capture.
 * Returns non-zero before any launch on every refusal of st2_wave_edges about the geometry (NULL wave / frames, bad B / T_cap /
 * samples_per_frame, trim < 0, a row too long for int32, w_bs too small) and on: o_bs too small; NULL params / out / dyn /
 * workspace; A outside 0..64; win NULL with A > 0; rho not finite or <= 0; a pointer that is not aligned to 4 bytes; out
 * overlapping wave; a workspace that is too small. */
int32_t st2_wave_dynamics_tile(void);
int32_t st2_wave_dynamics_chunk(void);
int64_t st2_wave_dynamics_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame);
int st2_wave_dynamics(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                      int32_t trim, const float* params /* fp32 [B][4], device */, int32_t A,
                      const float* win /* fp32 [2 A + 1], device */, double rho, float* out, int64_t o_bs,
                      float* dyn /* fp32 [B][2], device */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- volume: per-request and per-token gain envelopes in the hand-over (added under ABI 23, additive: one kernel-level entry
 * point and one helper, no new backend-table slot, no struct change, no new sticky status bit) --------- *
 * st2_wave_volume: SSML's <prosody volume=> and the loudness of <emphasis> -- one gain in dB per row and one per token, smoothed
 * on the 64-sample grid and applied as st2_wave_dynamics applies its gain.  It takes st2_wave_edges's geometry (wave, w_bs,
 * frames, B, T_cap, samples_per_frame, trim) and, on the device and read by the kernels:
 *   pos      int32 [B][N + 1]: the tokens' boundaries in samples of THIS row, not decreasing (what st2_wave_breaks is given, or
 *            st2_token_marks_breaks's marks at up = down = 1 for rows that entry spliced silence into); N in 1..512;
 *   lengths  int32 [B] or NULL: the rows' token counts, Nb = clamp(lengths[b], 0, N); NULL = N;
 *   db       fp32 [B] or NULL: row b's gain in dB;       tok_db  fp32 [B][N] or NULL: token n's gain in dB, on top of the row's.
 * Host numbers: the half window A in blocks of 64 samples, 0..64, and win fp32 [2 A + 1] on the device (the limiter's window,
 * non-negative weights that sum to 1); win is NULL if and only if A = 0.  It writes `out` (fp32, row stride o_bs, not overlapping
 * wave), vol fp32 [B][2] and the workspace.  With n = n_b the row's valid samples (st2_wave_level's rule 1) and K = ceil(n / 64):
 *  1. Cleaning.  clean(v) = 0 for a NaN, else min(max(v, -60), +20), in fp32: -inf is -60, +inf is +20.  A NULL table is 0.
 *  2. Wanted gain per block.  For block k, c = min(64 k + 32, n - 1); idx is the largest i in [0, Nb) with pos[b][i] <= c, or 0
 *     if there is none (a binary search: where pos decreases, whichever of its candidates the search meets) -- so a token of no
 *     samples is skipped, and of several boundaries at one sample the last token owns what follows.  d[k] =
 *     min(max((double)clean(db[b]) + (double)clean(tok_db[b][idx]), -60), +20); with Nb = 0 the token term is 0.
 *  3. Smoothing, fp64: acc = 0; for j = -A .. A in order acc = acc + fl64((double)win[j + A] * (d[clamp(k + j, 0, K - 1)] -
 *     d[k])); e[k] = d[k] + acc.  A stretch of equal d wider than the window gives e = d exactly, d = 0 all around e = 0.
 *  4. Gain per block.  lin[k] = 0.0f where e[k] <= -60 (SSML's "silent"), else fl32(10^(e[k] / 20)), pow in fp64, rounded once;
 *     e = 0 gives exactly 1.0f.
 *  5. Gain per sample: st2_wave_dynamics's rule 8, bit for bit -- linear between the block centres 64 k + 31.5, block indices
 *     clamped to [0, K - 1], gain = fmaf(t, lin[ka + 1] - lin[ka], lin[ka]) with t = (2 (i - 64 ka) - 63) / 128, out[i] =
 *     fl32(x[i] * gain) with x itself.
 *  6. Kept words.  Samples 4 v .. 4 v + 3 of a row lie between the same two block centres; where both of those gains are exactly
 *     1.0f the samples are moved as 32-bit words, NaN payloads as they are.  Every 0 dB stretch of a row keeps its bits, and
 *     a call whose tables are all 0 (or NULL) is a bit copy of the valid samples.
 *  7. Nothing at or past out[b][n] is written.
 *  8. Report.  vol[b] = {max |out[b][i]| over i < n with a NaN ignored as by fmaxf, 0 for an empty row; the number of k < K with
 *     lin[k] != 1.0f, as fp32}: a maximum and a count of integers, so no bit depends on how the reduction is cut, and a row's
 *     output and its two numbers depend neither on the tiling nor on the row's place in the batch.
 * Everything is fixed but the last ulp of pow.
 * `workspace` (float-aligned, st2_wave_volume_workspace_bytes(B, T_cap, samples_per_frame) bytes; 0 for an argument <= 0) begins
 * with lin fp32 [B][Kcap], Kcap = ceil(samples_per_frame T_cap / 64) (entries at or past a row's K are not written); the
 * partials of the report follow.  Three launches (gains per (256 blocks, row); apply per (4096 samples, row); the report per
 * row), no atomics, no allocation, no synchronisation, no host read: legal under stream capture.
 * Returns non-zero before any launch on every refusal of st2_wave_dynamics about the geometry, out, the workspace and the window
 * (NULL wave / frames, bad B / T_cap / samples_per_frame, trim < 0, a row too long for int32, w_bs or o_bs too small, A outside
 * 0..64, win NULL with A > 0, out overlapping wave, a workspace that is too small) and on: win given with A = 0; NULL pos / out /
 * vol / workspace; N outside 1..512; a pointer that is not aligned to 4 bytes. */
int64_t st2_wave_volume_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame);
int st2_wave_volume(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap, int32_t samples_per_frame,
                    int32_t trim, const int32_t* pos /* int32 [B][N + 1], device */, const int32_t* lengths /* int32 [B] or NULL */,
                    int32_t N, const float* db /* fp32 [B] or NULL, device */, const float* tok_db /* fp32 [B][N] or NULL, device */,
                    int32_t A, const float* win /* fp32 [2 A + 1], device */, float* out, int64_t o_bs,
                    float* vol /* fp32 [B][2], device */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- per-request seeds: counter-based noise drawn on the device (added under ABI 23, additive: one kernel-level entry point,
 * no new backend-table slot, no struct change, no new sticky status bit) ----------------------------- *
 * st2_noise_fill: the model's randomness -- the sampler's start noise, its per-step draws, the harmonic source's draws -- from one
 * int64 seed per row.  A plain-C host needs no generator of its own: it fills the `noise` / `step_noise` of st2_front_args and the
 * `noise` of st2_decoder_forward(_ragged) with this entry, on the stream the plans run on.
 * Values.  Element i of noise stream s of a row with seed k is output (i mod 4) of the four values made from
 *     Philox4x32-10(counter = (i div 4, 0, s, 0), key = (lo32(k), hi32(k))),    k read as uint64
 * (Random123's generator: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds).  A row's
 * values depend on its seed, the stream id and i alone: not on B, not on the row's place in the batch, not on n.
 *   ST2_NOISE_BITS    the four 32-bit words x0 .. x3 themselves, as their bit pattern (for tests and callers that want integers);
 *   ST2_NOISE_NORMAL  fp32 standard normals, pairwise from (x0, x1) and (x2, x3): with u1 = ((x >> 8) + 0.5) 2^-24,
 *                     r = sqrt(-2 ln u1) and a = 2 ((x' >> 8) 2^-24) -- exact in fp32 -- the pair is (r cos(pi a), r sin(pi a));
 *                     |z| <= 5.89.  Full-precision logf / sqrtf / sincospif; within 8 2^-24 max(1, |z|) of the fp64 value.
 * Stream ids: ST2_NOISE_SAMPLER the sampler's start noise [B][256]; ST2_NOISE_STEP + j the draws of sampler step j;
 * ST2_NOISE_SINE the harmonic source's [B][F U][9].
 * Layout.  out[s][b][i] at out + s * s_stride + b * b_stride + i (strides in elements) for s < S, b < B, written with noise stream
 * stream0 + s under seeds[b] (int64 [B], device: read by the kernel, so a captured launch serves any seeds), for i in
 * [0, min(n, counts[b] * per_count)) -- counts int32 [B] on the device, a negative one counting as 0 -- or [0, n) where counts
 * is NULL.  Nothing else is written: padding between rows and a row's tail past its count stay as they are.  (The source noise
 * of a ragged batch: counts = the frame counts, per_count = U * 9; st2_har_source_len reads no further.)
 * One launch, one thread per counter, 16-byte stores where the row's base is 16-byte aligned and 4-byte stores elsewhere; no
 * allocation, no synchronisation: legal under stream capture.  n = 0 is a successful no-op.  Returns non-zero before any launch
 * on: NULL seeds / out; B or S outside 1..65535; n < 0 or n >= 2^34 (i div 4 is the counter's first word); an unknown kind;
 * stream0 + S - 1 past 2^32 - 1; B > 1 with b_stride < n (or >= 2^40); S > 1 with s_stride < (B - 1) b_stride + n; counts with
 * per_count <= 0; seeds / out / counts misaligned for its element. */
enum st2_noise_kind { ST2_NOISE_NORMAL = 0, ST2_NOISE_BITS = 1 };
#define ST2_NOISE_SAMPLER 0u
#define ST2_NOISE_STEP 1u
#define ST2_NOISE_SINE 0x10000u
int st2_noise_fill(const int64_t* seeds, int32_t B, uint32_t stream0, int32_t S, int32_t kind /* st2_noise_kind */, float* out,
                   int64_t s_stride, int64_t b_stride, int64_t n, const int32_t* counts, int64_t per_count, void* stream);

/* ---- fit to duration: per-request frame targets apportioned on the device (added under ABI 23, additive: one kernel-level
 * entry point, no new backend-table slot, no struct change, no new sticky status bit -- the flag column of `report` carries
 * what a status bit would) ------------------------------------------------------------------------- *
 * st2_durations_fit: rewrites every row of the integer durations (int64 [B][N], N <= 512, as the duration head or a caller made
 * them) to a stated total of frames, between the front and st2_frames_from_durations.  Everything that takes its timing from
 * the durations -- the frame counts, the expansion, the timing marks, the per-token prosody spans -- follows with no change.
 * All integer arithmetic; a row's result depends on that row alone.
 *   len     int32 [B] or NULL: the rows' token counts, clamped to 0..N; NULL = N.
 *   target  int32 [B]: the frame targets; <= 0 leaves the row alone.
 *   hold    uint8 [B][N] or NULL: non-zero = this token keeps its duration.  NULL = no token is held.
 *   out     int64 [B][N]; may be dur itself (in place), must not overlap it otherwise.
 *   report  int32 [B][4] or NULL: {S, T', flag, number of tokens n < n_b with out[n] != dur[n]} per row.
 * Per row b, with n_b the clamped length:
 *   1. target[b] <= 0: all N entries of out equal dur's; report {S, S, 0, 0}, S as in step 2.
 *   2. v_n = max(dur[n], 1) for n < n_b, S = sum of min(v_n, 2^31) (a term is saturated so that no caller-made duration wraps
 *      the sum; S <= 2^31 - 1 is exact either way), reported as min(S, 2^31 - 1).  In a fitted row the entries n >= n_b of out
 *      are 0, as the duration head writes them.  n_b = 0: the row is all zeros, report {0, 0, 2, 0}.  S > 2^31 - 1: the row
 *      is copied as in step 1, report {2^31 - 1, 2^31 - 1, 3, 0}.
 *   3. Held tokens: base_n = v_n, m_n = 0.  Free tokens: base_n = 1, m_n = v_n - 1 -- no token drops under one frame; the
 *      excess over that frame is what stretches and shrinks.  lo = sum of base_n.
 *   4. lo > T_cap: the row is copied as in step 1, report {S, S, 3, 0}.  Else T' = min(max(target[b], lo), T_cap) and
 *      flag = 0 if T' == target[b], else 1: the target was infeasible and the nearest feasible total was taken.
 *   5. R = T' - lo, M = sum of m_n.  M = 0 (every free token is one frame long): m_n = 1 for the free tokens, M = their count.
 *      No free token at all: the row is copied as in step 1, report {S, S, 2, 0}.
 *   6. Largest remainders: q_n = floor(R m_n / M), r_n = (R m_n) mod M, K = R - sum of q_n; the K tokens with m_n > 0 that
 *      have the largest r_n, ties to the LOWER index, get one frame more: out[n] = base_n + q_n + [extra].  (R m_n < 2^62.)
 *   7. report[b] = {S, T', flag, changed}.
 * Then: the row sums to T' exactly; T' = target wherever lo <= target <= T_cap; T' = S returns the row's v_n; held tokens
 * are unchanged; among free tokens dur[a] < dur[b] implies out[a] <= out[b].
 * One launch, one workgroup of 256 threads per row, at most two tokens per thread, read into registers before anything is
 * written (in place is legal); block sums in a fixed order; a token's rank is a count over the row's (r, -index) keys in LDS.
 * No atomics, no allocation, no synchronisation: legal under stream capture.  len, target and hold are read by the kernel: a
 * captured launch serves any of them.  Returns non-zero before any launch on: NULL dur / target / out; B outside 1..65535;
 * N outside 1..512; T_cap <= 0; dur / out not 8-byte aligned, len / target / report not 4-byte aligned. */
int st2_durations_fit(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* target, const uint8_t* hold,
                      int32_t T_cap, int64_t* out, int32_t* report, void* stream);

/* ---- reference clips at a client's rate and in G.711 (added under ABI 23, additive: one kernel-level entry point and its
 * size helper, no new backend-table slot, no struct change, no new sticky status bit) ---------------------------------- *
 * st2_clip_ingest: the way in of a zero-shot request.  src holds B rows of N_cap samples (row b at
 * src + b * src_bs samples) in format fmt; n (int32 [B], device) their sample counts.  U = up, D = down, K = taps_per_phase,
 * taps fp32 [U][K] on the device, U / D = 24000 / rate reduced.
 *  1. Decode.  Row b has n_b = clamp(n[b], 0, N_cap) samples; nothing of src at or past n_b is read.  ST2_PCM_F32 as it is;
 *     ST2_PCM_S16 v / 32768; ST2_PCM_ULAW / ST2_PCM_ALAW the ITU-T G.711 16-bit value of the byte, / 32768 (all exact in fp32).
 *  2. Resample: st2_wave_resample_pack's rule.  m_b = min(L_cap, (n_b U + D - 1) div D) and, with c = (j D) div U and
 *     p = (j D) mod U,  r_b[j] = sum_{k < K} taps[p][k] * x_b[c - (K - 1) div 2 + k],  x_b = 0 outside [0, n_b) by select, in
 *     fp32 with fmaf, k ascending: a sample depends neither on the tiling nor on the row's place in the batch.  U = D = K = 1
 *     is the decode alone.
 *  3. Trim: librosa.effects.trim(y, top_db, ref = max, frame_length 2048, hop_length 512) with centred, zero-padded frames.
 *     Frame f = 0 .. m_b div 512 covers r_b[512 f - 1024, 512 f + 1024), zeros outside [0, m_b); e_f = max(sum r^2 / 2048,
 *     1e-10); frame f is non-silent iff e_f > max_f e_f * 10^(-top_db / 10).  With f0 / f1 the first / last non-silent frame:
 *     start = 512 f0, end = min(m_b, 512 (f1 + 1)).  A frame is the sum of four 512-sample block sums, each made once in a fixed
 *     order (no atomics).  An all-zero row keeps its whole length.  top_db <= 0: start = 0, end = m_b.
 *  4. Minimum length.  If end - start < L_min: end = min(m_b, start + L_min), then start = max(0, end - L_min).
 *  5. Hand-over.  wave[b][i] = r_b[start + i] for i < end - start (row b at wave + b * w_bs, w_bs >= L_cap and a multiple of 4,
 *     wave 16-byte aligned); nothing at or past wave[b][end - start] is written.  len[b] = end - start; start[b] (may be NULL)
 *     the cut; flags[b] (may be NULL): bit 0 -- (n_b U + D - 1) div D > L_cap, the row was truncated to the capacity; bit 1 --
 *     the minimum-length rule moved a bound, or the row is still shorter than L_min.
 * `work` (16-byte aligned, st2_clip_ingest_work_bytes(B, L_cap) bytes; 0 for B or L_cap <= 0) holds the untrimmed 24 kHz rows
 * and the block sums.  Three launches (resample + block sums, bounds, gather), no allocation, no synchronisation, no host
 * read.  Returns non-zero before any launch on: NULL src / n / taps / wave / len / work; B outside 1..65535; N_cap or L_cap
 * <= 0; w_bs < L_cap or not a multiple of 4; src_bs < N_cap with B > 1; up / down outside 1..1024; taps_per_phase outside
 * 1..512; unknown fmt; L_min < 0 or > L_cap; a NaN top_db; work_bytes too small; src misaligned for its sample type (taps / n
 * / len for theirs, wave / work for 16 bytes); a table that leaves no room in LDS (63 KiB) for a 512-sample tile. */
int64_t st2_clip_ingest_work_bytes(int32_t B, int32_t L_cap);
int st2_clip_ingest(const void* src, int64_t src_bs, const int32_t* n, int32_t B, int32_t N_cap, int32_t fmt, int32_t up,
                    int32_t down, const float* taps, int32_t taps_per_phase, float top_db, int32_t L_min, float* wave,
                    int64_t w_bs, int32_t L_cap, int32_t* len, int32_t* start, int32_t* flags, void* work, int64_t work_bytes,
                    void* stream);

/* ---- reference-audio style path (compute_style, Demo/Inference_LibriTTS.ipynb:100-111) ------------------------- *
 * The mel front-end (meldataset.py:58-66: torchaudio MelSpectrogram(n_mels 80, n_fft 2048, win 1200, hop 300) ->
 * (log(1e-5 + mel) + 4) / 4) and StyleEncoder (models.py:139-164) run on the conv kernels above: the windowed DFT is a
 * k=1 conv [2*(n_fft/2+1)][n_win] over the frame columns, the mel filter bank a k=1 conv [n_mels][n_fft/2+1], every
 * Conv2d a Conv1d over the width with its kernel rows stacked along the channels (feature maps are stored (h, c, w):
 * element (b,h,c,w) at x + b*x_bs + h*x_hs + c*x_cs + w, so three consecutive rows ARE the 3C-channel input).  These
 * entry points are the remaining non-GEMM steps.
 *   st2_stft_frames:    frames[b][c][m] = wave[b][reflect(m*hop + c - shift)], c < n_win, m < L/hop + 1: the frame
 *                       columns of torch.stft(center=True, pad_mode="reflect") restricted to the taps where the window
 *                       (zero padded to n_fft) is non-zero; shift = n_fft/2 - (n_fft - n_win)/2.
 *   st2_power_spectrum: p[b][k][m] = y[b][k][m]^2 + y[b][K+k][m]^2 (stacked real / imaginary DFT rows).
 *   st2_log_norm:       x = (log(eps + x) - mean) / std in place.
 *   st2_dwconv3x3s2:    depthwise Conv2d(C, C, 3, stride 2, padding 1, groups C), w [C][3][3]: LearnedDownSample('half'),
 *                       models.py:27-42; output map (H-1)/2+1 x (W-1)/2+1.
 *   st2_avgpool2x2:     DownSample('half'), models.py:72-75: replicate the last column of an odd width, 2x2 average;
 *                       H even; output H/2 x (W+1)/2. */
int st2_stft_frames(const float* wave, int64_t w_bs, int32_t B, int32_t L, int32_t n_win, int32_t hop, int32_t shift,
                    float* frames, int64_t f_bs, int32_t f_cs, void* stream);
int st2_power_spectrum(const float* y, int64_t y_bs, int32_t y_cs, int32_t B, int32_t K, int32_t M, float* p,
                       int64_t p_bs, int32_t p_cs, void* stream);
int st2_log_norm(float* x, int64_t n, float eps, float mean, float stdv, void* stream);
int st2_dwconv3x3s2(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, const float* w, const float* bias,
                    int32_t B, int32_t C, int32_t H, int32_t W, float* y, int64_t y_bs, int64_t y_hs, int32_t y_cs,
                    void* stream);
int st2_avgpool2x2(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, int32_t B, int32_t C, int32_t H, int32_t W,
                   float* y, int64_t y_bs, int64_t y_hs, int32_t y_cs, void* stream);

/* out[i] = a*x[i] + b*y[i] + c*z[i] (z may be NULL): sampler updates, sampler.py:184-208,497-510 */
int st2_axpbypcz(const float* x, float a, const float* y, float b, const float* z, float c,
                 float* out, int64_t n, void* stream);

/* ================================================================================================================ *
 * Module-level entry points: one call per reference nn.Module.forward.                          *
 *                                                                                                                      *
 * An engine handle holds one model's packed weights on one device.  The launch plans behind                            *
 *   st2_decoder_forward  ==  Decoder.forward            Modules/istftnet.py:499-528 / Modules/hifigan.py:446-475        *
 *   st2_sampler_run      ==  DiffusionSampler.forward   Modules/diffusion/sampler.py:573-586 (ADPM2 :497-519, KDiffusion *
 *                            :184-208, Transformer1d / StyleTransformer1d Modules/diffusion/modules.py:283-427, 40-185)  *
 * live in C++ (styletts2_amd/csrc/st2_engine.hip): a host in any language synthesises with these calls and nothing    *
 * else.  Memory: the engine owns ONE device allocation for its packed weights (st2_finalize_weights); every forward    *
 * call works inside a caller-owned workspace (size from the *_workspace_bytes query for the same shape), allocates     *
 * nothing, never synchronises and is legal under hipStreamBeginCapture after one eager call of the same shape.         *
 * ================================================================================================================ */
typedef struct st2_engine st2_engine;

typedef struct st2_model_config {
  /* decoder: models.py:617-633, Configs/config.yml:49-57 (istftnet) / Configs/config_libritts.yml:49-55 (hifigan) */
  int32_t decoder_kind;            /* 0 = istftnet, 1 = hifigan */
  int32_t dim_in;                  /* hidden_dim: asr channels (512) */
  int32_t style_dim;               /* acoustic style width (128) */
  int32_t upsample_initial_channel;
  int32_t n_upsamples;  int32_t upsample_rates[4];  int32_t upsample_kernel_sizes[4];
  int32_t n_resblock_kernels;  int32_t resblock_kernel_sizes[4];  int32_t resblock_dilations[4][3];
  int32_t gen_istft_n_fft, gen_istft_hop;   /* istftnet only */
  /* style denoiser: models.py:643-669, Configs/config.yml:66-83 */
  int32_t multispeaker;            /* 0 = Transformer1d (LayerNorm), 1 = StyleTransformer1d (AdaLayerNorm on `features`) */
  int32_t dn_layers, dn_heads, dn_head_features, dn_multiplier;
  int32_t dn_channels;             /* style vector width = 2 * style_dim (256) */
  int32_t dn_embedding;            /* PL-BERT hidden size (768) */
  int32_t dn_context_features;     /* width of `features` (256), multispeaker only */
  int32_t dn_max_length;           /* fixed-embedding table length (512) */
  /* prosody predictor: models.py:440-466, Configs/config.yml `hidden_dim` */
  int32_t pred_hidden;             /* d_hid of ProsodyPredictor (512); 0 = predictor not used */
  /* PL-BERT: Utils/PLBERT/config.yml model_params (an HF AlbertConfig; widths are read from the weights' shapes) */
  int32_t bert_layers;             /* num_hidden_layers (12; ALBERT: one shared weight set); 0 = PL-BERT not used */
  float bert_ln_eps;               /* layer_norm_eps (1e-12) */
} st2_model_config;

int st2_create(const st2_model_config* cfg, st2_engine** out);
int st2_destroy(st2_engine* e);
/* Hands one parameter to the engine (copied): `name` = the reference state_dict key below the module, prefixed by
 * "decoder." / "denoiser." (the Transformer's keys, i.e. `diffusion.unet.*` without that prefix), with weight-norm
 * pairs FOLDED by the caller: `X.weight` = weight_g * weight_v / ||weight_v|| (norm over all dims but 0; dim 0 of a
 * ConvTranspose1d is C_in), replacing X.weight_g / X.weight_v.  `data` is a HOST pointer to fp32, C-contiguous. */
int st2_load_weights(st2_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* Packs everything loaded so far (split-f16 conv layouts, polyphase ConvTranspose / strided-conv forms, concatenated
 * AdaIN fc matrix) and uploads it in one device allocation.  which: bit 0 = decoder, bit 1 = denoiser, bit 2 = prosody
 * predictor (names prefixed "predictor."), bit 3 = text encoder ("text_encoder."), bit 4 = PL-BERT ("bert.", the HF
 * AlbertModel keys) with the `bert_encoder` Linear ("bert_encoder.weight" / ".bias") when it was loaded, bit 5 = the
 * reference-audio style encoders ("style_encoder." / "predictor_encoder.", whichever were loaded; spectral-norm triples
 * folded by the caller: X.weight = weight_orig / (u . (W_mat v)), replacing X.weight_orig / weight_u / weight_v).
 * Synchronous; call once after the last st2_load_weights (again after loading new weights). */
int st2_finalize_weights(st2_engine* e, int32_t which);

/* Optional tap points (NULL = not wanted): device buffers the forward copies intermediates into, for parity work. */
typedef struct st2_decoder_taps {
  float* encode;       /* [B][1024][T]                                       istftnet.py:510 */
  float* front;        /* [B][512][2T]   decoder front = generator input      istftnet.py:513-524 */
  float* har_source;   /* [B][600T]      tanh(l_linear(sine waves))           istftnet.py:352-354 */
  float* har;          /* istftnet [B][n_fft+2][120T+1] |STFT| ++ angle; hifigan: unused (== har_source) */
  float* stage[4];     /* generator stage outputs [B][C_i][L_i]               istftnet.py:359-375 */
  float* spec_phase;   /* istftnet [B][n_fft+2][120T+1] after exp / sin        istftnet.py:378-379 */
} st2_decoder_taps;

int64_t st2_decoder_workspace_bytes(st2_engine* e, int32_t B, int32_t T);
/* wave[B][600*T] = Decoder(asr[B][dim_in][T], F0[B][2T], N[B][2T], s[B][style_dim]).  `sine_noise` [B][600T][9] are
 * the standard-normal draws of SineGen (istftnet.py:242; the reference draws them inside forward); `har_inject`
 * (optional) replaces the harmonic-source features with the caller's (tap-point protocol): istftnet
 * [B][n_fft+2][120T+1], hifigan [B][600T].  All pointers are device pointers, tensors contiguous. */
int st2_decoder_forward(st2_engine* e, const float* asr, const float* f0, const float* n, const float* s,
                        const float* sine_noise, const float* har_inject, int32_t B, int32_t T, float* wave,
                        void* workspace, int64_t workspace_bytes, const st2_decoder_taps* taps, void* stream);
/* Ragged batch (ABI v23): row b is an utterance of frames[b] (int32 [B] on the device, each in 1..T_max) frames in the T_max
 * layout above (asr [B][dim_in][T_max], F0 / N [B][2 T_max], sine_noise [B][600 T_max][9], har_inject istftnet
 * [B][n_fft+2][120 T_max+1] zero past 120 frames[b] + 1 columns, hifigan [B][600 T_max] zero past 600 frames[b]).  Row b of
 * wave [B][600 T_max] equals st2_decoder_forward of that utterance alone at T = frames[b] (every convolution sees the zero
 * padding of the row's own end, every InstanceNorm / AdaIN reduces over the row's own columns) and is exactly 0 from
 * 600 frames[b] on.  Inputs past a row's end are never used (NaN there is harmless).  frames[b] outside 1..T_max is clamped
 * there (not checked: that would need a host read).  Workspace: st2_decoder_workspace_bytes(B, T_max).  Taps: not supported
 * (must be NULL).  Same stream / graph-capture contract. */
int st2_decoder_forward_ragged(st2_engine* e, const float* asr, const float* f0, const float* n, const float* s,
                               const float* sine_noise, const float* har_inject, const int32_t* frames, int32_t B,
                               int32_t T_max, float* wave, void* workspace, int64_t workspace_bytes,
                               const st2_decoder_taps* taps, void* stream);

/* Per-step scalars of the ADPM2 loop, all input independent (sampler.py:184-191, 490-495): for step i (sigma_i ->
 * sigma_{i+1}) row i of `table` holds 11 doubles
 *   [0..3]  c_skip, c_out, c_in, c_noise at sigma_i        [4..7]  the same at sigma_mid
 *   [8]     (sigma_mid - sigma_i) / sigma_i                [9]     (sigma_down - sigma_i) / sigma_mid      [10] sigma_up
 * A Python host fills it with the reference's own torch / python-float arithmetic (bit-faithful to the reference);
 * st2_sampler_table does the same with libm for other hosts (KarrasSchedule sigma_min / sigma_max / rho, sampler.py:
 * 328-337; ADPM2 rho = 1).  sigma0 = sigmas[0] (x_0 = sigma0 * noise). */
#define ST2_SAMPLER_TABLE_COLS 11
int st2_sampler_table(int32_t steps, double sigma_min, double sigma_max, double rho, double sigma_data, double* table,
                      double* sigma0);
int64_t st2_sampler_workspace_bytes(st2_engine* e, int32_t B, int32_t N, int32_t steps, double embedding_scale);
/* out[B][C] = DiffusionSampler(noise[B][C], embedding[B][N][E], features[B][Fc] or NULL, num_steps = steps,
 * embedding_scale).  step_noise [steps-1][B][C] are the per-step randn_like draws (sampler.py:509); `lengths` (int32
 * [B] on the device, or NULL) = token counts of a right-padded batch; step_taps (optional) [steps-1][B][C] receives x
 * after every step. */
int st2_sampler_run(st2_engine* e, const float* noise, const float* embedding, const float* features,
                    const float* step_noise, const int32_t* lengths, int32_t B, int32_t N, int32_t steps,
                    double embedding_scale, const double* table, double sigma0, float* out, void* workspace,
                    int64_t workspace_bytes, float* step_taps, void* stream);

/* Alignment expansion + ProsodyPredictor.F0Ntrain (Demo/Inference_LJSpeech.ipynb:303-311, models.py:497-510), i.e. what
 * sits between the duration predictor and Decoder.forward:
 *   asr[B][dim_in][T]  = t_en[B][dim_in][N] expanded by `durations` (int64 [B][N], rows summing to T),
 *   (f0, n)[B][2T]     = F0Ntrain(d expanded the same way, s),  d_cm [B][pred_hidden + style_dim][N] = the duration
 *                        encoder's output channel-major, s [B][style_dim] the prosodic style;
 * shift = 1 applies the HiFi-GAN one-frame right shift (Demo/Inference_LibriTTS.ipynb:306-319).  Same memory / stream
 * contract as st2_decoder_forward; its outputs are exactly that call's inputs. */
int64_t st2_prosody_workspace_bytes(st2_engine* e, int32_t B, int32_t N, int32_t T);
int st2_prosody_forward(st2_engine* e, const float* d_cm, const float* t_en, const int64_t* durations, const float* s,
                        int32_t B, int32_t N, int32_t T, int32_t shift, float* asr, float* f0, float* n, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* Ragged batch (ABI v23): as st2_prosody_forward with T = T_max, row b's durations summing to frames[b] (int32 [B] on the
 * device, 1..T_max).  Row b equals st2_prosody_forward of that utterance alone at T = frames[b]; asr is exactly 0 from
 * frames[b] on, f0 / n from 2 frames[b] on.  Workspace: st2_prosody_workspace_bytes(B, N, T_max). */
int st2_prosody_forward_ragged(st2_engine* e, const float* d_cm, const float* t_en, const int64_t* durations,
                               const float* s, const int32_t* frames, int32_t B, int32_t N, int32_t T_max, int32_t shift,
                               float* asr, float* f0, float* n, void* workspace, int64_t workspace_bytes, void* stream);

/* TextEncoder.forward (models.py:284-345): tokens int64 [B][N] (id 0 = pad), lengths int32 [B] or NULL ->
 * t_en [B][dim_in][N]: Embedding -> depth x [weight-norm Conv1d k5 -> LayerNorm over channels -> LeakyReLU(0.2) -> mask] ->
 * BiLSTM.  Weights: "text_encoder.*" with the weight-norm pairs folded (st2_finalize_weights bit 3). */
int64_t st2_text_workspace_bytes(st2_engine* e, int32_t B, int32_t N);
int st2_text_forward(st2_engine* e, const int64_t* tokens, const int32_t* lengths, int32_t B, int32_t N, float* t_en,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* DurationEncoder.forward + the duration head (models.py:536-569, 450-451; Demo/Inference_LJSpeech.ipynb:294-301): from
 * d_en [B][pred_hidden][N] (bert_encoder's output, channel-major) and the prosodic style s [B][style_dim] to
 *   d_cm [B][pred_hidden + style_dim][N]  the duration encoder's output (channel-major; st2_prosody_forward's input),
 *   durations int64 [B][N] (may be NULL)  max(1, round(sum sigmoid(duration_proj(lstm(d))))), 0 at pad tokens, + `tail`
 *                                         frames on every utterance's last token (5 in the LJSpeech notebook).
 * `lengths` (int32 [B] on the device, or NULL) = token counts of a right-padded batch (packed-sequence BiLSTMs, masked
 * LayerNorm outputs).  Weights: "predictor.text_encoder.*", "predictor.lstm.*", "predictor.duration_proj.linear_layer.*"
 * (st2_finalize_weights bit 2 packs them with the rest of the predictor when they were loaded). */
int64_t st2_duration_workspace_bytes(st2_engine* e, int32_t B, int32_t N);
int st2_duration_forward(st2_engine* e, const float* d_en, const float* s, const int32_t* lengths, int32_t B, int32_t N,
                         int32_t tail, float* d_cm, int64_t* durations, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* PL-BERT forward (Utils/PLBERT/util.py:6-12: HF AlbertModel(...).last_hidden_state): tokens int64 [B][N], lengths int32
 * [B] or NULL (valid keys of a right-padded batch = the attention mask of utils.py:42-46 `length_to_mask`) ->
 * hidden_cm [B][hidden][N], the last hidden state CHANNEL-major (transpose of the reference's [B][N][hidden]).
 * Token-merged storage inside ([C][B*N]): every Linear is one k = 1 split-f16 conv over B*N columns (q|k|v fused), the
 * embedding LayerNorm rides in the mapping conv's prologue, gelu_new in the FFN conv's epilogue.  Weights: "bert.*"
 * (st2_finalize_weights bit 4); cfg.bert_layers / bert_ln_eps. */
int64_t st2_bert_workspace_bytes(st2_engine* e, int32_t B, int32_t N);
int st2_bert_forward(st2_engine* e, const int64_t* tokens, const int32_t* lengths, int32_t B, int32_t N, float* hidden_cm,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* Everything the notebooks' `inference` cell does between the phoneme ids and the alignment (Demo/Inference_LJSpeech.ipynb:
 * 268-301, Demo/Inference_LibriTTS.ipynb:258-305; LFinference's style carry-over, Inference_LJSpeech.ipynb:409-446) in ONE
 * call: text encoder, PL-BERT, bert_encoder, the style-diffusion sampler (ADPM2 over st2_sampler_table's rows), the style
 * mixing, the duration encoder and (when `durations` is given) the duration head.
 *   s_pred  = sampler(noise, embedding = bert, features = ref_s)            [B][2*style_dim]
 *   s_pred  = t * s_prev + (1 - t) * s_pred                                 when s_prev != NULL
 *             (carry != 0: the B rows are CONSECUTIVE SENTENCES of one passage and row k's s_prev is row k-1's mixed s_pred_out;
 *             row 0 takes `s_prev` [1][2*style_dim] or nothing.  The passage is sequential in this vector only, so its text
 *             encoder / PL-BERT / sampler / duration stages run as ONE right-padded batch and the carry-over as a row scan
 *             of elementwise kernels between them: every row equals the sentence-by-sentence LFinference loop's)
 *   ref | s = s_pred[:, :style_dim] | s_pred[:, style_dim:]
 *   ref     = alpha * ref + (1 - alpha) * ref_s[:, :style_dim];  s = beta * s + (1 - beta) * ref_s[:, style_dim:]   (ref_s)
 * All pointers are device memory; NULL = absent where marked optional.  Needs every weight group of bits 1-4 finalized.
 * Same memory / stream / graph-capture contract as st2_decoder_forward; the outputs feed st2_prosody_forward (after the
 * host has read the frame counts off `durations`) and st2_decoder_forward (`ref`). */
typedef struct st2_front_args {
  const int64_t* tokens;     /* [B][N] */
  const int32_t* lengths;    /* [B] or NULL */
  const float* noise;        /* [B][2*style_dim] */
  const float* step_noise;   /* [steps-1][B][2*style_dim] */
  const float* ref_s;        /* [B][2*style_dim]: reference style (multispeaker models), or NULL */
  const float* s_prev;       /* [B][2*style_dim]: previous sentence's s_pred_out (long-form), or NULL */
  int32_t B, N, steps;
  int32_t tail;              /* frames added to every utterance's last token (5 in the LJSpeech notebook) */
  double embedding_scale;
  const double* table;       /* HOST: st2_sampler_table(steps, ...) rows */
  double sigma0;
  double alpha, beta, t;     /* style mixing weights (0.3 / 0.7 / 0.7 in the notebooks) */
  float* t_en;               /* out [B][dim_in][N] */
  float* d_cm;               /* out [B][pred_hidden + style_dim][N] */
  float* s;                  /* out [B][style_dim]  prosodic style */
  float* ref;                /* out [B][style_dim]  acoustic style (the decoder's `s`) */
  float* s_pred_out;         /* out [B][2*style_dim] = ref | s after mixing (the next sentence's s_prev), or NULL */
  int64_t* durations;        /* out [B][N], or NULL when the caller supplies its own durations */
  int32_t carry;             /* != 0: rows = consecutive sentences, style carried from row k-1 to row k (see above); ABI v21 */
} st2_front_args;
int st2_sizeof_front_args(void);
int64_t st2_front_workspace_bytes(st2_engine* e, const st2_front_args* a);
int st2_front_forward(st2_engine* e, const st2_front_args* a, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- per-request controls (added under ABI 23, additive: kernel-level entry points and one plan-level twin, no new
 * backend-table slot, no change to an existing struct or signature) ------------------------------------------------ *
 * What a request brings as a SETTING is a device row of fp32 [B], like its lengths are, so that one batch -- and one recorded
 * graph -- serves any mix of requests.  A NULL row keeps the behaviour without it.  Rows are CLAMPED WHERE THEY ARE READ (a
 * bad device value gives a clamped row, never a fault or a host read); hosts validate what they upload.
 *
 *   speed     dur[b][n] = max(1, rint(total[b][n] / speed[b])), total = the fp32 sigmoid sum of st2_duration_head: one
 *             correctly rounded fp32 division behind the unchanged reduction, rint = round-half-even, 0 at pad tokens, `tail`
 *             added afterwards, unscaled.  Clamped to [0.25, 4]; NaN -> 1.  x / 1 is exact: speed 1 gives st2_duration_head's
 *             bits.
 *   alpha, beta, t   the style mixing weights of st2_front_args with row b's own value.  Clamped to [0, 1]; NaN -> the
 *             call's scalar.  The complement of a weight is (float)(1.0 - (double)w) and a mix is `v = a x; v += b y` (no
 *             FMA), which is st2_axpbypcz's arithmetic: a row whose weight equals a scalar representable in fp32 gives the
 *             bits of the scalar call.
 *   f0_scale  F0[b][l] *= f0_scale[b] for l < 2 T_b.  Clamped to [0.5, 2]; NaN -> 1.
 *   n_shift   N[b][l] += n_shift[b] for l < 2 T_b (N is a log-energy: a shift is a gain).  Clamped to [-2, 2]; NaN -> 0; a
 *             shift of 0 keeps x itself (-0.0 survives).
 *
 * st2_duration_head_rate: st2_duration_head with `speed` (fp32 [B], device, not NULL).  Same reduction order; dsum (optional)
 * receives the un-scaled sums.
 * st2_style_mix_rows: the style mixing of st2_front_forward as ONE launch.  s_pred [B][2 style_dim] = the sampler's output;
 * s_prev ([B][2 style_dim], or [1][2 style_dim] with carry != 0), ref_s [B][2 style_dim], t / alpha / beta (fp32 [B]) may each
 * be NULL; a NULL weight row means the scalar t0 / alpha0 / beta0 (validated: in [0, 1]).  Outputs ref, s [B][style_dim] and
 * (optional) s_pred_out [B][2 style_dim] = ref | s.  carry != 0: the rows are consecutive sentences of one passage and row k's
 * s_prev is row k-1's mixed result (row 0 takes s_prev or nothing): ONE workgroup per 256 channels walks the rows, one channel
 * per thread.  Same arithmetic, in the same order, as the st2_axpbypcz / st2_copy_ncl launches of the front plan it replaces.
 * st2_prosody_controls: in place over f0, n [B][L] (row stride bs, L = 2 T of st2_prosody_forward[_ragged]'s outputs);
 * frames (int32 [B], device, or NULL = every row is L long) bounds row b at 2 * frames[b] (clamped to 0..L): nothing at or past
 * it is read or written, and a workgroup whose chunk lies there leaves at once.  A NULL f0_scale / n_shift leaves that curve
 * alone; both NULL launches nothing.  One operation per element, never fused.
 * All three: one launch, no allocation, no synchronisation, legal under stream capture; bad arguments return non-zero before
 * any launch. */
int st2_duration_head_rate(const float* x, int64_t x_bs, int32_t x_cs, const float* w, const float* bias, int32_t B,
                           int32_t K, int32_t J, int32_t N, const int32_t* len, int32_t tail, const float* speed,
                           int64_t* dur, float* dsum, void* stream);
int st2_style_mix_rows(const float* s_pred, const float* s_prev, const float* ref_s, const float* t, const float* alpha,
                       const float* beta, double t0, double alpha0, double beta0, int32_t B, int32_t style_dim,
                       int32_t carry, float* ref, float* s, float* s_pred_out, void* stream);
int st2_prosody_controls(float* f0, float* n, int64_t bs, int32_t B, int32_t L, const float* f0_scale,
                         const float* n_shift, const int32_t* frames, void* stream);

/* st2_front_forward with per-row controls.  A NULL `ctl`, or one whose four members are NULL, issues exactly the launches of
 * st2_front_forward.  With any of alpha / beta / t the style mixing is ONE st2_style_mix_rows launch (also in carry mode: the
 * row scan runs inside it instead of as 5 B launches); with speed the duration head is st2_duration_head_rate (`durations`
 * must then be non-NULL: there is nothing to scale otherwise).  With a non-empty `ctl` the scalar a->t / alpha / beta must lie
 * in [0, 1] (they are what a NaN row falls back to).  Workspace: st2_front_workspace_bytes(a) suffices.  The CPU
 * backends of st2_debug_set_backend have no slot for the two kernels: a non-empty `ctl` is refused while one is installed. */
typedef struct st2_controls {
  const float *speed, *alpha, *beta, *t;  /* each fp32 [B] on the device, or NULL */
} st2_controls;
int st2_sizeof_controls(void);
int st2_front_forward_ctl(st2_engine* e, const st2_front_args* a, const st2_controls* ctl, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- timing marks and per-token prosody controls (added under ABI 23, additive: kernel-level entry points, one plan-level
 * entry and one new struct; no new backend-table slot, no change to an existing struct or signature) -- *
 * Both rest on ONE rule: where a token lies in the decoder frames of its row.
 *
 * The boundary rule.  Row b has durations dur[b][0..N) (int64, non-negative, N <= 512), n_b tokens (len[b] clamped to 0..N,
 * NULL = N) and T_b frames (frames[b] clamped to 0..T_cap, NULL = T_cap).  With
 *     c[n] = min(T_cap, sum_{m < min(n, n_b)} dur[b][m])                       (a 64-bit sum that saturates)
 * -- st2_expand_by_durations_len's cum[n - 1] for every n <= n_b; tokens at or past n_b hold 0 wherever len is given, the
 * duration head writes that -- bound[b][n], n = 0..N, is the first frame t in [0, T_b] whose token index idx(b, t) of the
 * expansion is >= n:
 *     bound[0] = 0;   bound[n] = min(T_b, c[n] == 0 ? 0 : c[n] + shift)  for 1 <= n <= N - 1;   bound[N] = T_b
 * (shift = 1: the HiFi-GAN one-frame right shift; the last token owns whatever the durations leave over, as the expansion's
 * idx = min(lo, N - 1) does).  Monotone by construction; a row truncated to T_cap (ST2_STATUS_FRAME_CAPACITY) gets T_b for
 * every token that fell off, and so do pad tokens.
 *
 * st2_token_marks: marks (int32 [B][N + 1]) = row-relative sample positions in the PACKED stream of st2_wave_pack (up = down =
 * 1) / st2_wave_resample_pack (U = up, D = down).  With n_smp = max(0, samples_per_frame * T_b - trim) and
 * s = min(samples_per_frame * bound[b][n], n_smp):   marks[b][n] = (s U + D - 1) div D,   the first output sample at or after
 * the boundary's time under the resampler's c = (j D) div U.  Hence marks[b][N] = offsets[b + 1] - offsets[b] exactly, and
 * token n of row b is packed[offsets[b] + marks[b][n] : offsets[b] + marks[b][n + 1]].  bound_out (int32 [B][N + 1], optional)
 * receives bound, in frames.  All intermediates are 64-bit.  One launch, one wave per row, no allocation, no synchronisation,
 * legal under stream capture.  Returns non-zero before any launch on: NULL dur / marks; B, N, T_cap or samples_per_frame
 * <= 0; N > 512; up or down outside 1..1024; trim < 0; a row at capacity whose ceil(samples_per_frame T_cap U / D) samples do
 * not fit int32. */
int st2_token_marks(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* frames, int32_t T_cap,
                    int32_t shift, int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, int32_t* marks,
                    int32_t* bound_out, void* stream);

/* Per-token controls: fp32 [B][N] device rows, clamped where they are read like the per-row controls above.
 *   tok_speed     dur[b][n] = max(1, rint(total[b][n] / r)), r = clamp(clamp(speed[b]) * clamp(tok_speed[b][n])): ONE fp32
 *                 product in front of st2_duration_head_rate's one division; every clamp is to [0.25, 4], NaN -> 1, a NULL speed
 *                 row is 1.  1 * 1 and x / 1 are exact: neutral keeps st2_duration_head's bits.
 *   tok_f0_scale  F0[b][l] *= tok_f0_scale[b][idx(b, l div 2)] for l < 2 T_b.  Clamped to [0.5, 2]; NaN -> 1.
 *   tok_n_shift   N[b][l] += tok_n_shift[b][idx(b, l div 2)] for l < 2 T_b.  Clamped to [-2, 2]; NaN -> 0; a shift of 0 keeps x
 *                 itself.
 * idx(b, t) is st2_expand_by_durations_len's for the same dur / shift: the values are stepwise at the token boundaries
 * (nothing is smoothed across them).
 * st2_duration_head_rate_tok: st2_duration_head_rate with tok_speed (not NULL) and an optional speed.
 * st2_prosody_controls_tok: st2_prosody_controls with token rows; L = 2 T must be even, dur int64 [B][N], N <= 512.  Workgroup
 * (1024 columns, row) rebuilds the prefix sum in LDS as the expansion does, searches once per frame, applies one operation
 * per element (never fused) and leaves at once at or past 2 T_b, where nothing is read or written.  A NULL row leaves that curve
 * alone; both NULL launches nothing.
 * Both: one launch, no allocation, no synchronisation, legal under stream capture; bad arguments return non-zero before any
 * launch. */
int st2_duration_head_rate_tok(const float* x, int64_t x_bs, int32_t x_cs, const float* w, const float* bias, int32_t B,
                               int32_t K, int32_t J, int32_t N, const int32_t* len, int32_t tail, const float* speed,
                               const float* tok_speed, int64_t* dur, float* dsum, void* stream);
int st2_prosody_controls_tok(float* f0, float* n, int64_t bs, int32_t B, int32_t L, const int64_t* dur, int32_t N,
                             int32_t shift, const float* tok_f0_scale, const float* tok_n_shift, const int32_t* frames,
                             void* stream);

/* Intonation (added under ABI 23): a request's pitch RANGE and pitch CONTOUR, applied in place to the
 * prosody predictor's F0 curve (fp32 [B][L], row stride bs, L = 2 T_cap even) in front of st2_prosody_controls[_tok].  Row b
 * has T_b = clamp(frames[b], 0, L / 2) frames (L / 2 without frames) and len_b = 2 T_b columns; nothing at or past len_b is read
 * or written.
 *  1. Voiced.  Column l < len_b is voiced iff f0[l] is finite and f0[l] > voiced_hz (the harmonic source's rule).  n_v = their
 *     number, m = (sum over them of log2((double)f0[l])) / n_v in fp64.  A row with n_v = 0 is left alone, bit for bit.
 *  2. Range.  r_b = range[b] clamped to [0, 4]; NaN or a NULL row = 1.  q = tok_range[b][idx(b, l div 2)] clamped to [0, 4], NaN
 *     = 1 (NULL: 1), idx the token of st2_prosody_controls_tok for the same dur / shift.  r = min(r_b * q, 4) in fp32.
 *  3. Contour.  contour is fp32 [B][K][2], 0 <= K <= 8, of points (p, v): p a position as a share of the row's own frames, v an
 *     offset in semitones.  A point with a NaN p or v is unused; p is clamped to [0, 1] and then raised to the largest used p in
 *     front of it, v is clamped to [-24, 24].  At frame t, x = (t + 0.5) / T_b in fp64 and j = the number of used points with
 *     p <= x: c = the first v for j = 0, the last v for j = the number of used points, and otherwise
 *     c = v[j-1] + (v[j] - v[j-1]) * ((x - p[j-1]) / (p[j] - p[j-1])) in fp64 in that order: coincident points are a step.  No
 *     used point: c = 0.
 *  4. Output.  A voiced column with r == 1.0f and c == 0.0 keeps its bits.  Any other voiced column becomes
 *     fl32(min(max(exp2((m + (double)r * (log2 f0 - m)) + c / 12.0), lo_hz), hi_hz)).  Unvoiced columns keep their bits; as
 *     lo_hz > voiced_hz, a voiced column stays voiced.
 *  5. pitch (fp32 [B][4] or NULL) = {exp2(m) in Hz, n_v, the smallest and the largest output over the voiced columns};
 *     {NaN, 0, NaN, NaN} for n_v = 0.
 * Everything is fixed but the last ulp of fp64 log2 / exp2 and the order of the fp64 sum.  One launch, one workgroup of 256
 * threads per row, no atomics, no allocation, no synchronisation, no host read: legal under stream capture.  range, tok_range,
 * contour (or K = 0) and pitch all absent: returns 0 without a launch; pitch alone: the launch measures and writes no f0.
 * Returns non-zero before any launch on: NULL f0; B outside 1..65535; L <= 0 or odd; bs < L with B > 1; tok_range without dur;
 * N outside 1..512 with tok_range; K outside 0..8; NULL contour with K > 0; voiced_hz outside (0, 1000]; not voiced_hz < lo_hz
 * < hi_hz <= 20000. */
int st2_pitch_shape(float* f0, int64_t bs, int32_t B, int32_t L, const int32_t* frames, const float* range,
                    const float* tok_range, const int64_t* dur, int32_t N, int32_t shift, const float* contour, int32_t K,
                    float voiced_hz, float lo_hz, float hi_hz, float* pitch /* [B][4] or NULL */, void* stream);

/* st2_front_forward_ctl with a per-token rate: tok->speed (fp32 [B][N], device) makes the duration head
 * st2_duration_head_rate_tok (`durations` must then be non-NULL).  A NULL `tok`, or one whose member is NULL, is
 * st2_front_forward_ctl, which is this call with NULL.  Refused while a debug backend is installed, as `ctl` is. */
typedef struct st2_token_controls {
  const float* speed;  /* fp32 [B][N] on the device, or NULL */
} st2_token_controls;
int st2_sizeof_token_controls(void);
int st2_front_forward_tok(st2_engine* e, const st2_front_args* a, const st2_controls* ctl, const st2_token_controls* tok,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* StyleEncoder.forward (models.py:139-164; `compute_style`, Demo/Inference_LibriTTS.ipynb:100-111): mel [B][80][T] (the
 * normalised log-mel of the reference recording, T >= 80 frames) -> style [B][style_dim].  which = 0: `style_encoder`
 * (acoustic half of ref_s), 1: `predictor_encoder` (prosodic half); ref_s = cat(which 0, which 1).  Conv2d layers run as
 * split-f16 Conv1d over the width with their kernel rows stacked along the channels (maps stored (h, c, w)), the
 * depthwise stride-2 conv and the 2x2 average as st2_dwconv3x3s2 / st2_avgpool2x2.  The mel itself is five kernel-level
 * calls (st2_stft_frames, st2_conv1d with the windowed-DFT matrix, st2_power_spectrum, st2_conv1d with the filter bank,
 * st2_log_norm: styletts2_amd/style.py mel_spectrogram_engine).  Same memory / stream contract as st2_decoder_forward. */
int64_t st2_style_workspace_bytes(st2_engine* e, int32_t which, int32_t B, int32_t n_mels, int32_t T);
int st2_style_forward(st2_engine* e, int32_t which, const float* mel, int32_t B, int32_t n_mels, int32_t T, float* style,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- length-aware reference-audio style path (additive under ABI 23) ------------------------------------- *
 * A batch of B reference clips of unequal length in one [B][L_cap] buffer: row b of every result equals the clip processed
 * alone at its own length.  Masking is a select throughout: nothing at or past a row's own end is ever used, those
 * positions may hold NaN bit patterns.  Lengths are int32 [B] on the device and are CLAMPED where they are read (a caller's
 * bad length gives a wrong row, never a read or a store outside the buffers the capacities size).
 *
 *   st2_stft_frames_len  st2_stft_frames with the reflection about the row's own [0, L_b), L_b = len[b] clamped to
 *                        [L_min, L]; frame columns at or past M_b = L_b / hop + 1 are exact zeros, so the windowed-DFT and
 *                        filter-bank convs behind it need no lengths.  m_len (int32 [B], may be NULL) receives M_b.
 *   st2_log_norm_len     st2_log_norm on rows x[b][c][0 .. M), columns at or past len[b] written as exact 0.
 *   st2_dwconv3x3s2_len / st2_avgpool2x2_len   the maps of clip b are w_len[b] <= W wide (clamped to 1 .. W): zero padding /
 *                        the odd-width replicate at the row's own end, outputs [0, (w_len[b] + 1) / 2); outputs past that
 *                        width are left as the memory held them.
 *   st2_style_lengths    one launch: every per-row length of st2_style_forward_ragged from mel_len [B] (clamped to
 *                        [T_min, T_cap]).  With W_0 = mel_len and W_{i+1} = (W_i + 1) / 2 the table holds, in this order,
 *                        W_i[b] for i = 0 .. stages (B entries each), W_stages[b] - 4 (B entries), then for i = 0 .. stages
 *                        the per-stacked-row table of the H >> i high map: B ((H >> i) + 2) - 2 entries, entry r = W_i[b]
 *                        when padded row r + 1 of the [B][(H >> i) + 2] stack is an image row of clip b, 0 when it is one
 *                        of the zero rows between clips (a "seam": the conv tiles of that row exit without storing).
 *                        st2_style_lengths_count returns the number of entries (-1 on bad arguments). */
int st2_stft_frames_len(const float* wave, int64_t w_bs, int32_t B, int32_t L, int32_t n_win, int32_t hop, int32_t shift,
                        float* frames, int64_t f_bs, int32_t f_cs, const int32_t* len, int32_t L_min, int32_t* m_len,
                        void* stream);
int st2_log_norm_len(float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t M, float eps, float mean, float stdv,
                     const int32_t* len, void* stream);
int st2_dwconv3x3s2_len(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, const float* w, const float* bias, int32_t B,
                        int32_t C, int32_t H, int32_t W, float* y, int64_t y_bs, int64_t y_hs, int32_t y_cs,
                        const int32_t* w_len, void* stream);
int st2_avgpool2x2_len(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, int32_t B, int32_t C, int32_t H, int32_t W,
                       float* y, int64_t y_bs, int64_t y_hs, int32_t y_cs, const int32_t* w_len, void* stream);
int64_t st2_style_lengths_count(int32_t B, int32_t H, int32_t stages);
int st2_style_lengths(const int32_t* mel_len, int32_t B, int32_t T_min, int32_t T_cap, int32_t H, int32_t stages, int32_t* out,
                      void* stream);
/* StyleEncoder.forward on a ragged batch: mel [B][80][T_cap], row b valid on its first mel_len[b] frames (int32 [B] on the
 * device, clamped to [80, T_cap]) -> style [B][style_dim], row b as st2_style_forward gives it for that clip alone.  Every
 * Conv2d is ONE launch over the B (h + 2) - 2 stacked rows of the padded [B][h + 2][c][w] maps with per-row x_len / y_len
 * (seam rows: 0), so the number of launches does not depend on B; the split-K decision of each conv is the one the per-clip
 * launch of st2_style_forward takes, so a batch whose rows are all T_cap long gives st2_style_forward's bits.  No host read,
 * no allocation: legal under stream capture. */
int64_t st2_style_workspace_bytes_ragged(st2_engine* e, int32_t which, int32_t B, int32_t n_mels, int32_t T_cap);
int st2_style_forward_ragged(st2_engine* e, int32_t which, const float* mel, const int32_t* mel_len, int32_t B, int32_t n_mels,
                             int32_t T_cap, float* style, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- measurement hook (bench.py's roofline leg) ------------------------------------------------------------------- *
 * st2_conv_timing(1) clears and starts, (0) stops recording a HIP event pair around every st2_conv1d_xs launch (C_in >=
 * 64, L_out >= 256) on its launch stream, whichever plan issues it.  st2_conv_timing_read (after stopping) waits for the
 * events and fills rows of 6 doubles {ks, C_in, C_out, L_out, B, milliseconds}; returns the number of launches recorded
 * (rows may be NULL to count), < 0 on error.  Not thread safe; not legal under stream capture. */
int st2_conv_timing(int enable);
int st2_conv_timing_read(double* rows, int32_t cap_rows);

/* ---- start-up autotuner of st2_conv1d_xs (ABI v19) ---------------------------------------------------------------- *
 * A launch of st2_conv1d_xs exists in several BUILDS that issue the same products in the same order and share one
 * epilogue -- results are bitwise identical (tests/test_ops_gpu.py) --: 128 x 128 tiles at 3 workgroups / CU or 128 x 256
 * tiles at 2 (k = 3, 7, 11), in dispatch order or XCD-aware tile order (launches with 2 / 4 / 8 output row blocks: every XCD keeps
 * ONE row block's weights in its L2).  Which is fastest depends on the shape AND on the box by a few percent (and, before
 * round 4's row-end fix of the epilogue, by up to 1.75 x on the C = 256 / L = 8 000 layers of Modules/istftnet.py:358-375),
 * so a serving process measures at start-up:
 *   st2_conv_tune(1)   every FIRST launch of a shape class (device, ks, C_in, C_out, L_out, B) on a non-capturing stream
 *                      times its candidate builds (1 warm-up + 3 x 2 launches each, round-robin, output into a scratch tensor the
 *                      library allocates for the duration of tuning mode -- the one exception to "no allocation" besides
 *                      the status word; the caller's tensors are only read) and records the winner; the call then runs it;
 *   st2_conv_tune(0)   leaves tuning mode (frees the scratch); recorded classes keep their build, others follow the rule;
 *   st2_conv_tune(-1)  also forgets the current device's table.
 * st2_conv_tune_set pins (variant >= 0: bit 0 = 128 x 256 tiles, bit 1 = XCD-aware order) or
 * erases (variant = -1) one class on the current device; st2_conv_tune_read fills rows of 24 doubles {ks, C_in, C_out,
 * L_out, B, device, chosen variant, n candidates, (variant, ms / launch) x 8} for the current device and returns the number
 * of classes (rows may be NULL to count).  Tuning synchronises the stream it measures on; the table is guarded by a mutex and
 * the measurement runs outside it (other threads keep launching, on the rule's build for a class while it is being measured).
 * Tuning mode allocates and waits on events: it must not overlap a stream capture anywhere in the process (a global-mode
 * capture on another stream would be invalidated) -- tune first, record graphs afterwards.  A class is keyed without the
 * dilation: the three dilations of a resblock share one measurement (they differ in halo columns only). */
int st2_conv_tune(int mode);
int st2_conv_tune_set(int32_t ks, int32_t C_in, int32_t C_out, int32_t L_out, int32_t B, int32_t variant);
int st2_conv_tune_read(double* rows, int32_t cap_rows);

/* ---- operand-range telemetry, both ends (ABI v20; debug: allocates, synchronises; not for the serving path) ------------------ *
 * The split-f16 convs carry u = x_scale * pro(x) as f16 hi + lo.  The format has two ends: above 65504 the kernels clamp
 * (ST2_STATUS_F16_RANGE); below ~2^-3 the lo half becomes a subnormal f16 and the operand keeps an ABSOLUTE error of 2^-25
 * instead of 2^-22 relative -- a layer whose scaled input sits at 1e-3 is 100 x less precise than fp32 although nothing
 * overflows.  Where a checkpoint puts each layer (Snake alpha, weight-norm gains, GELU / LeakyReLU outputs are free,
 * Modules/istftnet.py:27-62) is what this hook reports: between st2_debug_headroom(1) and (0) every st2_act_split /
 * st2_conv1d_f16s launch also measures the planes it produced; st2_debug_headroom_read fills rows of ST2_HEADROOM_COLS doubles
 *   [0] kind (0 = activation pass of the xs path, 1 = prologue of the fused conv)   [1] prologue   [2] B  [3] C_in  [4] L
 *   [5] x_scale   [6] max |u|   [7] max |u| / 65504 (>= 1: clamped)
 *   [8] relative RMS error the split adds to the operand: sqrt(sum ulp(lo)^2 / 12 / sum u^2) (fp32 storage itself: 3.4e-8;
 *       every element's lo normal: ~4e-8)
 *   [9] share of the operand's energy carried by elements whose lo half is subnormal or zero
 *   [10] conv site (st2_calibration_read index) when an engine plan issued the launch, else -1   [11] that engine (identity)
 * in launch order and returns their number.  tools/headroom_report.py prints the table for a checkpoint.
 * A ragged launch (st2_act_split_len's len, st2_conv_desc.x_len) is measured over each row's valid columns on both routes: the
 * columns at and past a row's end are the conv's zero padding, so what memory holds there (a longer earlier batch, a NaN) enters
 * neither the maximum nor a sum and raises no status bit; [4] stays the launch's L.  Elements with hi = lo = 0 enter no sum, and a
 * launch without any other element reports [8] = [9] = 0.  Launches under stream capture are not recorded. */
#define ST2_HEADROOM_COLS 12
int st2_debug_headroom(int enable);
int st2_debug_headroom_read(double* rows, int32_t cap_rows);

/* ---- per-layer operand scales (ABI v20) ------------------------------------------------------------------------------------ *
 * Every F.conv1d / nn.Linear of the reference is fp32 (Modules/istftnet.py:68-74,376-377, Modules/diffusion/modules.py:
 * 484-490).  The split-f16 convs match that over the whole fp32 range only if each conv's input is scaled into the part of
 * the f16 range where both halves are normal numbers.  By rule (no calibration) x_scale is 8 after a normalising prologue and
 * 1 otherwise -- right for O(1) tensors, up to 500 x less precise than fp32 for a layer whose input sits at 1e-4.  A serving
 * process therefore calibrates once per checkpoint:
 *     st2_debug_headroom(1);  one or more forward calls on representative inputs;  st2_debug_headroom(0);
 *     st2_calibrate(e, 3, &clamped);            (repeat the three lines while clamped > 0: at most twice)
 * Every conv site of the engine (= every split-f16 packed weight, in packing order) that was launched gets
 *     x_scale = 2^floor(log2(2^(16 - margin_bits) / max |pro(x)|))     (margin_bits = 3: max |u| in (4096, 8192])
 * from the largest operand any of its launches produced (a PL-BERT weight runs 12 times, a denoiser weight once per
 * evaluation: the maximum counts); the clamp and the status bit stay as the safety net for inputs beyond 2^margin_bits x the
 * calibration's.  Scales are powers of two -- the accumulator is rescaled exactly -- and live in the engine: every later
 * forward (eager or captured; capture AFTER calibrating, the scale is a kernel argument) uses them; results stay
 * reproducible bit for bit for a given table.  Returns the number of sites set (< 0 on error).
 *   st2_calibration_read   rows of ST2_CALIBRATION_COLS doubles {C_in, C_out, ks, x_scale (0 = by rule), max |pro(x)| seen};
 *                          returns the number of sites (rows may be NULL to count);
 *   st2_calibration_site_name   the reference state_dict key the site's weight was packed from;
 *   st2_calibration_write  installs a table (n = number of sites, entries 0 or a power of two; n = 0 clears): how rank 0's
 *                          calibration reaches the other ranks and how a table saved beside a checkpoint is restored;
 *   st2_calibration_scale  the formula above for one value (0 for max_abs <= 0).
 * st2_calibrate ACCUMULATES: a site's maximum is the largest over every recorded call since the table was last cleared, and sites whose
 * operand does not come out of a normalising prologue (free-ranging: F0 in Hz, stage outputs, FFN intermediates) get two more bits
 * of headroom than margin_bits (ABI v22).  st2_finalize_weights CLEARS the table (ABI v22; v20-21 kept it for an unchanged conv
 * layout): scales belong to the weights they were measured on.
 * Accumulation NEVER NARROWS a site: where a non-zero scale is already there, st2_calibrate keeps min(that scale, the scale computed
 * from the accumulated maximum).  This is the rule chosen for tables installed by st2_calibration_write, which carry scales only
 * (the maxima behind them do not travel: column 4 restarts at 0 and then reports what was seen SINCE the write): the installed scale
 * is itself the record of what the site must hold, so calibrating further on a quieter input leaves it alone and a louder one
 * lowers it, exactly as on the process that measured the table.  To start over, clear first (st2_calibration_write with n = 0). */
#define ST2_CALIBRATION_COLS 5
int st2_calibrate(st2_engine* e, int32_t margin_bits, int32_t* n_clamped);
int st2_calibration_read(st2_engine* e, double* rows, int32_t cap_rows);
int st2_calibration_site_name(st2_engine* e, int32_t site, char* name, int32_t cap);
int st2_calibration_write(st2_engine* e, const float* scales, int32_t n);
float st2_calibration_scale(float max_abs, int32_t margin_bits);

/* ---- box probe (ABI v19; diagnostic: allocates and frees its own device buffers, synchronises the device) ----------- *
 * Writes a JSON object (NUL terminated, <= cap bytes; 4 KB is enough) of micro-measurements of the current device:
 * device properties, sustained matrix-pipe clock and TFLOP/s of a bare v_mfma_f32_32x32x16_f16 loop on random / all-zero
 * operands, dependent-load latency and weight-stream bandwidth for working sets of 0.75 ... 64 MB (level >= 1: also 512
 * MB), a 512 MB HBM copy, and where the 2 048 workgroups of a 2-per-CU launch run (CUs / XCDs seen, workgroups per CU).
 * Takes ~0.5 s; bench.py puts it into its JSON line (`box.probe`) so that a run on a box nobody can log into still says
 * what the box gives the conv path.  No reference call site: measurement only. */
int st2_probe_box(char* json, int32_t cap, int32_t level);

/* ---- CU health probe (ABI v19; diagnostic: allocates ~0.9 GB for its duration, synchronises the device) --------------- *
 * Runs an instrumented copy of the conv kernel (per-workgroup cycle stamps + HW_ID) on the launch class that separated
 * the box classes of rounds 1-3 (k = 7, C = 256, L = 8 000, 128 x 256 tiles), reports as JSON when every XCD finished and the
 * CUs whose median epilogue takes > 3 x the chip's median, finds their CU-mask bits by measurement (8-workgroup probes on
 * single-bit-masked streams: bit i belongs to XCD i % 8) and returns in mask_out (mask_words >= 8 words) the CU mask of the
 * device WITHOUT them and their number in *n_excluded (0 = nothing slow, mask = all CUs).  It is how round 4 found that the
 * "slow CUs" of the slow box class were the row-end tiles of the launch -- since the epilogue fix it
 * reads 0 on every box seen -- and it stays as the check that finds a genuinely degraded CU.  Takes ~0.1 s. */
int st2_probe_cu_health(char* json, int32_t cap, uint32_t* mask_out, int32_t mask_words, int32_t* n_excluded);

/* Matrix-pipe load generator for the co-residency canaries (ABI v22).  Round 6 traced "the BiLSTM returns other bits while
 * narrow-tile convs run on another queue" to the hardware: on gfx950 a packed-f32 VALU op whose op_sel takes the HIGH dword of
 * src1 for the low result lane (`v_pk_fma_f32 ... op_sel:[0,1,0]`) returns a wrong low half in lanes 48-63 while ANOTHER wave of the
 * CU issues MFMAs in certain cadences (tools/simd_hazard_repro.hip).  The library no longer contains that
 * encoding (tools/check_isa.py gates every build); this entry point launches the cadences that provoked it, so that tests and a
 * serving process's start-up check can run ANY kernel of the path next to them and demand bitwise the idle result:
 *   kind 0  v_mfma_f32_16x16x32_f16, one dependent chain per wave (hit rate ~90-100 % on the old BiLSTM kernels)
 *   kind 1  v_mfma_f32_32x32x16_f16 in isolated dependent groups of three with LDS reads between them (what a one-accumulator
 *           32-column conv tile issues per k-step)
 *   kind 2  v_mfma_f32_16x16x32_f16, four independent chains per wave
 * `workgroups` x 4 waves, `iters` MFMA groups per wave (720 / 400: ~60-100 us per launch); nothing is read or written; asynchronous
 * on `stream`.  Returns non-zero on bad arguments. */
int st2_probe_mfma_stream(int32_t kind, int32_t workgroups, int32_t iters, void* stream);

/* ---- CU-partitioned streams (ABI v17) ---------------------------------------------------------------------------- *
 * A HIP stream whose kernels may only be placed on the compute units whose bit is set in `mask` (n_words x 32 bits, bit i
 * = CU i in the driver's numbering, which deals consecutive bits out round-robin over the 8 XCDs and their shader
 * engines: the low 64 bits are 8 CUs of every XCD).  The two-stage pipeline (front of batch k+1 under the decoder of
 * batch k) uses a pair of complementary masks so that the latency-bound front kernels -- among them the spin-waiting
 * cooperative BiLSTM groups -- own their CUs instead of competing with 12 000-workgroup convs for slots.
 * st2_stream_destroy waits for the stream's work.  The handle is a hipStream_t. */
int st2_stream_create_cu_mask(const uint32_t* mask, int32_t n_words, void** stream);
int st2_stream_destroy(void* stream);

/* ---- testing hook ---------------------------------------------------------------------------------------------- *
 * Replaces the kernel / memory entry points the launch plans call by the caller's (an array of ST2_BACKEND_ENTRIES,
 * ST2_BACKEND_ENTRIES_RAGGED or ST2_BACKEND_ENTRIES_V22 function pointers in the order of `enum st2_backend_slot`: a shorter
 * table leaves the later slots on their HIP kernels; NULL restores the HIP kernels).  tests/ uses it to run the
 * C++ plans on HOST memory against per-kernel CPU contracts, i.e. to validate plan wiring, packing and workspace
 * aliasing without a GPU.  Never used by the product path. */
enum st2_backend_slot {
  ST2_BE_CONV1D_F16S = 0, ST2_BE_CONV1D_XS, ST2_BE_ACT_SPLIT, ST2_BE_STATS_FINALIZE, ST2_BE_CONV1D_DIRECT,
  ST2_BE_PHASE_SPLIT, ST2_BE_INSTNORM_STATS, ST2_BE_COLNORM_STATS, ST2_BE_STYLE_FC, ST2_BE_CONVT_INTERLEAVE_STATS,
  ST2_BE_ADAIN_LEAKY_POOL, ST2_BE_HAR_SOURCE, ST2_BE_STFT_MAG_PHASE, ST2_BE_ISTFT, ST2_BE_ATTENTION_KEYLEN,
  ST2_BE_ADD_CHANVEC, ST2_BE_MEAN_TOKENS_LEN, ST2_BE_AXPBYPCZ, ST2_BE_TIME_FEATURES, ST2_BE_TOKENS_TO_CHANNELS,
  ST2_BE_BROADCAST_COLS, ST2_BE_COPY_NCL, ST2_BE_EXPAND_BY_DURATIONS,
  ST2_BE_LSTM_BIDIR,  /* st2_lstm_bidir's arguments with (void* scratch, int64_t scratch_bytes) inserted before `stream` */
  ST2_BE_COLNORM_APPLY, ST2_BE_DURATION_HEAD, ST2_BE_MASK_TAIL, ST2_BE_EMBED_TOKENS, ST2_BE_DWCONV3X3S2, ST2_BE_AVGPOOL2X2,
  ST2_BE_DEV_ALLOC,   /* void* (*)(int64_t bytes) */
  ST2_BE_DEV_FREE,    /* void (*)(void*) */
  ST2_BE_UPLOAD,      /* int (*)(void* dst, const void* src, int64_t bytes): synchronous host -> device copy */
  ST2_BACKEND_ENTRIES_V22,  /* a table of this many entries (ABI <= 22) leaves the slots below on their HIP kernels */
  /* ABI v23: the length-aware entry points of the ragged decoder / prosody plans */
  ST2_BE_ACT_SPLIT_LEN = ST2_BACKEND_ENTRIES_V22, ST2_BE_INSTNORM_STATS_LEN, ST2_BE_STATS_FINALIZE_LEN,
  ST2_BE_CONV1D_DIRECT_LEN, ST2_BE_ADAIN_LEAKY_POOL_LEN, ST2_BE_CONVT_INTERLEAVE_STATS_LEN, ST2_BE_HAR_SOURCE_LEN,
  ST2_BE_STFT_MAG_PHASE_LEN, ST2_BE_ISTFT_LEN, ST2_BE_RAGGED_LENGTHS, ST2_BE_EXPAND_BY_DURATIONS_LEN,
  ST2_BACKEND_ENTRIES_RAGGED,  /* a table of this many entries leaves the slots below on their HIP kernels */
  /* the length-aware entry points of the ragged style plan (st2_style_forward_ragged) */
  ST2_BE_DWCONV3X3S2_LEN = ST2_BACKEND_ENTRIES_RAGGED, ST2_BE_AVGPOOL2X2_LEN, ST2_BE_STYLE_LENGTHS,
  ST2_BACKEND_ENTRIES
};
int st2_debug_set_backend(void* const* table, int32_t entries);

#ifdef __cplusplus
}
#endif
#endif /* ST2_H */
