/* wfl_asr.h — C ABI of libwfl_asr_hip.so, the MI355X (gfx950) implementation of the WFL-ASR labeling hot path.
 *
 * The reference (usamireko/WFL-ASR) has no plugin / operator / FFI layer: its hot path sits behind plain Python
 * callables.  This header is therefore the build's own boundary; every entry point names the
 * reference interface it replaces so a maintainer can bind it from the reference's Python (ctypes stub in
 * INTEGRATION.md).  Conventions:
 *   - plain pointers and sizes only; all tensor pointers are DEVICE pointers unless the name ends in `_host`;
 *   - the caller owns every buffer (PyTorch-ROCm allocations are fine: pass tensor.data_ptr());
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued on it and nothing here synchronises the device;
 *   - return value 0 = ok, negative = error (wfl_last_error() gives the text); no exceptions cross the ABI;
 *   - one model handle per process per GPU; a handle is not re-entrant.  A model lives on the HIP device that was current
 *     when wfl_finalize ran (wfl_device()); every later call must be made with that device current and with buffers and
 *     stream of that device (checked: a mismatch is an error, not a cross-device access).
 */
#ifndef WFL_ASR_H
#define WFL_ASR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wfl_model wfl_model;

#define WFL_ENC_WHISPER 0
#define WFL_ENC_WAVLM 1
#define WFL_ENC_NONE 2     /* no encoder: the hidden states are a power mel spectrogram (model.py:82-91, 149-150) */

#define WFL_ABI_VERSION 2

/* Architecture = what /root/reference/model.py:54-146 reads from config.yaml plus the HF encoder config it
 * fetches by name (model.py:69-70, 74-80).  All int32, 64 slots, zero-initialise then fill. */
typedef struct wfl_arch {
  int32_t abi_version;       /* WFL_ABI_VERSION */
  int32_t encoder_type;      /* WFL_ENC_* */
  int32_t d_model;
  int32_t enc_layers;
  int32_t enc_heads;
  int32_t enc_ffn;
  int32_t n_mels;            /* whisper: 80 | 128 */
  int32_t max_positions;     /* whisper: encoder frames (1500); mel frames = 2x */
  /* head (model.py:96-142) */
  int32_t num_classes;       /* len(phonemes.txt) */
  int32_t o_id;              /* class index of "O" */
  int32_t num_languages;
  int32_t lang_emb_dim;
  int32_t enable_bilstm;
  int32_t bilstm_layers;
  int32_t n_conformer;
  int32_t conformer_heads;
  int32_t conformer_ff_expansion;
  int32_t conformer_kernel;
  int32_t enable_dilated;
  int32_t dilated_depth;
  int32_t dilated_kernel;
  /* wavlm (HF WavLMConfig) */
  int32_t wavlm_n_conv;              /* 7 */
  int32_t wavlm_conv_dim[8];
  int32_t wavlm_conv_kernel[8];
  int32_t wavlm_conv_stride[8];
  int32_t wavlm_group_norm;          /* 1: feat_extract_norm == "group" */
  int32_t wavlm_conv_bias;
  int32_t wavlm_stable_layer_norm;
  int32_t wavlm_pos_conv_kernel;
  int32_t wavlm_pos_conv_groups;
  int32_t wavlm_num_buckets;
  int32_t wavlm_max_distance;
  int32_t wavlm_do_normalize;
  int32_t fp8_weights;               /* 1: the Whisper encoder layers' q|k|v, out_proj, fc1, fc2 weights are kept as OCP e4m3 with one
                                        fp32 scale per output channel (BASELINE configs[4]); 0: bf16 */
  int32_t mel_hop;                   /* WFL_ENC_NONE: hop of the mel front-end = int(frame_duration * sample_rate) (model.py:88): 160 or
                                        320 when mel_sample_rate is 0, any hop >= 1 when it is set (160 and 320 have kernels of their own,
                                        every other hop runs the general one); d_model = n_mels = the hidden width (model.py:91) */
  int32_t precision;                 /* 0: bf16 operands (default).  1 ("model.precision: high", round 3): every GEMM, the attention's two
                                        products and the BiLSTM recurrence (hidden size <= 256 per direction) run as three bf16 MFMA passes
                                        over split operands -- A_hi W_hi + A_hi W_lo + A_lo W_hi, summed in fp32 -- with every activation
                                        carried as a bf16 pair hi + lo: the reference's tag indices at ~2.7x the forward time; the
                                        workspace doubles (wfl_workspace_bytes) */
  int32_t fp8_activations;           /* fp8_weights models only ("model.activation_dtype", round 4): how the four GEMM inputs of every encoder
                                        layer are carried.
                                        0: bf16 -- the e4m3 weights are converted in registers, bf16 MFMA;
                                        3: e4m3 PAIRS hi + lo (eight significant bits, what a bf16 operand carries) on the block-scaled
                                           fp8 MFMA v_mfma_scale_f32_16x16x128_f8f6f4: lo rides in the same instruction with a 2^-4 block
                                           scale.  Both hold the reference's arithmetic on the fp8-rounded checkpoint (logits within
                                           0.13 / 0.022);
                                        2: ONE e4m3 value per activation on the same MFMA: the fastest form, and 5-9 % of the raw tag
                                           decisions then differ from that reference (three mantissa bits) -- an explicit opt-in;
                                        1: round 3's form of 2 on the non-scaled fp8 MFMA (kept for A/B runs). */
  int32_t mel_sample_rate;           /* WFL_ENC_NONE: data.sample_rate of the model, 8000 .. 192000 Hz, with any mel_hop >= 1.  0 (a caller
                                        that predates the field): 16 kHz, mel_hop 160 or 320 only, as before.  The HTK mel bank spans
                                        0 .. rate // 2 Hz over the 201 STFT bins, as torchaudio's MelSpectrogram defaults; the caller feeds
                                        audio at this rate (wfl_forward's wav) */
  int32_t reserved[5];
} wfl_arch;

const char* wfl_last_error(void);
int32_t wfl_abi_version(void);

/* Replaces BIOPhonemeTagger.__init__ (model.py:55-146): builds an empty model for `arch`. */
int32_t wfl_create(const wfl_arch* arch, wfl_model** out);
void wfl_destroy(wfl_model* m);

/* Replaces nn.Module.load_state_dict(strict=True) as called at /root/reference/infer.py:206-207: call once per
 * state-dict tensor with the reference's own key names (fp32 host data; `num_batches_tracked` is ignored). */
int32_t wfl_load_tensor(wfl_model* m, const char* name, const float* data_host, const int64_t* shape, int32_t ndim);

/* Strict key check + weight packing (q/k/v packing and scaling, BatchNorm fold into the k=31 conv, conv weights to
 * tap-major GEMM form, GLU row interleave, language-bias table, bf16 conversion, upload).  After this the model
 * is immutable.  Missing or unexpected keys are an error, as with strict loading. */
int32_t wfl_finalize(wfl_model* m);

/* HIP device ordinal the weights were uploaded to by wfl_finalize (-1 before). */
int32_t wfl_device(const wfl_model* m);

/* The language ids WFL_LANG_AVERAGE averages over: the reference loops over the ids listed in langs.txt
 * (/root/reference/infer.py:147-156, 266-276), which may be a subset of the embedding rows.  Default: every id
 * 0 .. num_languages-1.  ids_host: n host int32, each in [0, num_languages). */
int32_t wfl_set_average_languages(wfl_model* m, const int32_t* ids_host, int32_t n);

/* Output frames for L input samples per clip (Whisper: always max_positions; WavLM: conv arithmetic; WFL_ENC_NONE:
 * 1 + L / mel_hop, the centred STFT's frame count, 0 when L <= 200). */
int32_t wfl_num_frames(const wfl_model* m, int32_t L);
int64_t wfl_workspace_bytes(const wfl_model* m, int32_t B, int32_t L);

/* lang_mode for wfl_forward */
#define WFL_LANG_NONE 0     /* forward(lang_id=None): skip lang_proj (model.py:176) */
#define WFL_LANG_IDS 1      /* lang_id[B] given */
#define WFL_LANG_AVERAGE 2  /* infer.py:146-156 / 266-276: every language id, mean of logits and of offsets
                               (the encoder runs once; only the head depends on the language) */

/* Replaces BIOPhonemeTagger.forward (model.py:148-194) + decode_predictions (196-198) + the softmax/threshold
 * half of suppress_low_confidence (infer.py:86-96) for a batch of clips.
 *   wav        [B][ldw] fp32 samples (16 kHz; WFL_ENC_NONE: mel_sample_rate), L valid columns; lens (optional, [B] int32) marks shorter clips
 *   ids        [B][T] int32  argmax class, or o_id where max prob < threshold
 *   argmax     [B][T] int32  raw argmax                      (optional)
 *   maxprob    [B][T] fp32   max softmax probability
 *   offsets    [B][T][2] fp32 sigmoid sub-frame offsets
 *   logits     [B][T][C] fp32                                (optional)
 *   hidden     [B][T][d] fp32 encoder output                 (optional, parity tests; WFL_ENC_NONE: the mel power, d = n_mels)
 *   lens with WavLM / WFL_ENC_NONE (whose input the reference never pads): clip b is treated as lens[b] samples long through the whole
 *   forward -- its own waveform / GroupNorm statistics, conv frame counts, attention keys, positional-conv padding and backward-LSTM
 *   start -- and comes out bit for bit as if it were labelled alone; frames behind its own count are tagged o_id with probability 0.
 *   With Whisper, lens only says where a clip's samples end inside the 30 s window (the encoder always sees 1500 frames).
 *   status     [1] int32 (device, optional): 0, or a bit mask of device-side errors of THIS forward (bit 0: an
 *              inter-workgroup wait of the BiLSTM recurrence timed out; bit 1, fp8_activations only: an e4m3 activation saturated
 *              at its scale or was NaN -- the tags are invalid either way).  Written by the last kernel
 *              of the forward, so it can ride in the same D2H copy as the tags.
 */
int32_t wfl_forward(wfl_model* m, const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L,
                    const int32_t* lang_id, int32_t lang_mode, float threshold, void* workspace,
                    int64_t workspace_bytes, int32_t* ids, int32_t* argmax, float* maxprob, float* offsets,
                    float* logits, float* hidden, int32_t* status, void* stream);

/* The two halves of wfl_forward, for callers that work on the encoder output in between -- the reference's training-time
 * validation forward pads / truncates hidden_states to max_label_len frames before the head (model.py:166-174).
 *   wfl_encode: model.py:149-161 (feature extractor + encoder) -> hidden [B][T][d] fp32, T = wfl_num_frames(L).
 *   wfl_head:   model.py:176-194 + the tag decision on hidden [B][T][d] fp32 with ANY T >= 1 (outputs as wfl_forward);
 *               workspace size from wfl_head_workspace_bytes(B, T). */
int32_t wfl_encode(wfl_model* m, const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, void* workspace,
                   int64_t workspace_bytes, float* hidden, void* stream);
int64_t wfl_head_workspace_bytes(const wfl_model* m, int32_t B, int32_t T);
int32_t wfl_head(wfl_model* m, const float* hidden, int32_t B, int32_t T, const int32_t* lang_id, int32_t lang_mode,
                 float threshold, void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* argmax, float* maxprob,
                 float* offsets, float* logits, int32_t* status, void* stream);

/* Synchronise `stream` and report the device-side error word of the last forward run on this workspace (same bits as
 * `status`: every kernel of a forward ORs into one word that the forward clears when it starts).  Optional; 0 = ok.
 * B, L: those of that forward (the word's place in the workspace follows the plan).  A workspace no forward has run on holds
 * whatever its allocator left there: zero it once, or call this only after a forward. */
int32_t wfl_check(wfl_model* m, void* workspace, int64_t workspace_bytes, int32_t B, int32_t L, void* stream);

/* ---- single stages, exported for unit parity tests and profiling ---- */

/* Replaces WhisperFeatureExtractor.__call__ at model.py:153-154 (HF feature_extraction_whisper.py:135-168).
 * out [B][n_mels][2*max_positions] fp32, the reference's layout.  wav and out must not be null and L must be at least 1 (B > 0,
 * ldw >= L), as for wfl_forward: anything else is an error status and nothing is launched.  lens[b] may be 0 (the clip is silence). */
int32_t wfl_logmel(wfl_model* m, const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L,
                   float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* bf16 MFMA GEMM with fused epilogue on frame rows (see csrc/common.h for the row layout):
 *   C[row(b,t)][n] = res + alpha * act( sum_k A[m][k] W[n][k] + bias[n] )      m = b*P + t, stored iff t < T
 * A, W, C(bf16 unless out_f32), res are bf16; K % 64 == 0, N % 128 == 0; k is split into taps of `cin` channels
 * `tap_stride` elements apart (cin >= K: one contiguous run).  glu: W rows interleaved (16 a | 16 gate). */
int32_t wfl_op_gemm(const void* A, int64_t lda, int32_t cin, int64_t tap_stride, const void* W, int32_t M, int32_t N,
                    int32_t K, int32_t n_valid, int32_t P, int32_t T, void* C, int64_t ldc, int64_t c_lead,
                    int32_t c_pitch, const float* bias, const void* res, int64_t ldres, float alpha, int32_t act,
                    int32_t glu, int32_t out_f32, void* stream);

/* The same Linear / Conv1d in the exact-label mode (`model.precision: high`; /root/reference/model.py:18-19, 26, 31-37, 131, 140 and
 * HF modeling_whisper.py:309-354, 391-407 computed to fp32-like accuracy so that infer.py:86-96 yields the reference's tag indices):
 * operands and results are bf16 PAIRS hi + lo (hi = bf16(x), lo = bf16(x - hi)), and
 *   out = res_hi + res_lo + alpha * act( A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T + bias ),   C = bf16(out), C_lo = bf16(out - C).
 * W3 is [N][3 K] bf16 with rows [W_hi | W_hi | W_lo]; A_lo has A_hi's leading dimension and tap layout (both inside one allocation);
 * K is the layer's K (a whole number of `cin`-channel taps), K % 32 == 0, N % 256 == 0 for the MFMA kernels' fast forms. */
int32_t wfl_op_gemm_split(const void* A_hi, const void* A_lo, int64_t lda, int32_t cin, int64_t tap_stride, const void* W3, int32_t M,
                          int32_t N, int32_t K, int32_t n_valid, int32_t P, int32_t T, void* C, void* C_lo, int64_t ldc,
                          int64_t c_lead, int32_t c_pitch, const float* bias, const void* res, const void* res_lo, int64_t ldres,
                          float alpha, int32_t act, int32_t glu, void* stream);

/* LayerNorm folded into the GEMM that consumes it (HF modeling_whisper.py:384-385, 401-402; model.py:18, 45):
 *   C = act( rstd_m * (A W'^T - mean_m * ln_s) + bias ),  W' = gamma o W (bf16), ln_s[n] = sum_k W'[n][k], bias = b + W beta;
 * mean / rstd are the statistics of row m of A over its K columns, computed inside the kernel.  M >= 2048, N % 256 == 0. */
int32_t wfl_op_gemm_ln(const void* A, int64_t lda, const void* W, int32_t M, int32_t N, int32_t K, int32_t n_valid, int32_t P,
                       int32_t T, void* C, int64_t ldc, int64_t c_lead, int32_t c_pitch, const float* bias, const float* ln_s,
                       float ln_eps, int32_t act, void* stream);

/* One GEMM launch with every optional field of csrc/common.h's GemmArgs passed through (null / 0 = absent), for per-mode parity tests:
 *   v      = sa(m) * w8_scale[n] * sum_k a(m, k) W[n][k]             (sa, w8_scale: 1 when absent)
 *   v      = rstd_m * (v - mean_m * ln_s[n])                          with ln_s (W = gamma o W, bias = b + W beta; see wfl_op_gemm_ln)
 *   v      = act( v + bias[n] + clip_bias[clip_idx[b]][n] ) + pos[t][n]
 *   out    = res (+ res_lo) + alpha * v       (no res: out = v);      out_f32 + acc_f32: out += C
 *   C      = bf16(out) (fp32 with out_f32),  c_lo = bf16(out - C);    stored iff t < T, t < clip_T[b] and n < n_valid
 *   W        bf16 [N][K], or -- w8_scale given -- OCP e4m3 bytes [N][K] with one fp32 scale per output channel
 *   a8 == 1  A holds e4m3 bytes too (lda in bytes, one tap); sa(m) = a8_scale[a8_lead + m], or a8_static when a8_scale is null;
 *            needs w8_scale.  (The block-scaled forms a8 == 2, 3 stay with wfl_op_gemm_mx.)
 *   c8       with a8: instead of C, e4m3(out * c8_inv_scale) bytes (ldc8 per row, C's row mapping); a stored element that saturates
 *            (|out| * c8_inv_scale > 448) or is NaN is stored clamped and ORs 2 into *status
 *   stats_out  (residual launches of the streaming kernel, N <= 1024) per C row r and 256-column tile j, the sum and the sum of squares
 *            of the bf16 values stored in C: stats_out[(r * 4 + j) * 2 + {0, 1}]
 *   stats_in   with ln_s: mean_m / rstd_m from a producer's stats_out -- row stats_lead + m, its first stats_nsl (1 .. 4) tile slots
 *            added up, over K columns -- instead of from the A row itself
 *   pos [>= T][ldpos] bf16, clip_bias [rows][clip_ld] fp32 with clip_idx [clips] int32, clip_T [clips] int32.
 * *kernel_id (optional) receives the kernel that ran: 1 / 5 the streaming kernel (192- / 256-row tiles), 2 / 3 gemm256, 4 the 128-tile
 * kernel, 6 the streaming kernel's conv mode, 7 its fp8 forms; 0 when nothing was launched.
 * What the dispatch would pass over without a word is an error status and nothing is launched: struct_bytes != sizeof(wfl_gemm_ex_args),
 * res_lo without res, c8 without a8, a8 outside {0, 1} or without w8_scale, stats_in without ln_s, acc_f32 without out_f32, and
 * stats_out / stats_in on a launch the streaming kernel does not take (no other kernel reads or writes them). */
typedef struct wfl_gemm_ex_args {
  int64_t struct_bytes;       /* sizeof(wfl_gemm_ex_args) */
  const void* A; int64_t lda; int64_t tap_stride; int32_t cin; int32_t a8;          /* as wfl_op_gemm (cin <= 0: K) */
  const void* W; const float* w8_scale; const float* a8_scale; int64_t a8_lead; float a8_static;
  int32_t M, N, K, n_valid, P, T, c_pitch;
  void* C; void* c_lo; int64_t ldc; int64_t c_lead;
  const float* bias; const float* clip_bias; const int32_t* clip_idx; const int32_t* clip_T; int32_t clip_ld; int32_t act;
  const void* res; const void* res_lo; int64_t ldres; float alpha; int32_t glu; int32_t out_f32; int32_t acc_f32;
  const void* pos; int64_t ldpos;
  const float* ln_s; float ln_eps; int32_t stats_nsl; float* stats_out; const float* stats_in; int64_t stats_lead;
  void* c8; int64_t ldc8; float c8_inv_scale; int32_t reserved;
  int32_t* status;            /* -> GemmArgs::err */
} wfl_gemm_ex_args;
int32_t wfl_op_gemm_ex(const wfl_gemm_ex_args* args, int32_t* kernel_id, void* stream);

/* softmax(q k^T) v per (clip, head); QK rows hold [q | k] (q pre-scaled by hd^-1/2 * log2 e), V rows (ld = ldv, same row
 * indexing) hold v; normally all three are columns of one packed q|k|v projection output. */
int32_t wfl_op_attention(const void* QK, int64_t ldqk, int64_t lead, const void* V, int64_t ldv, void* O, int64_t ldo, int32_t B,
                         int32_t T, int32_t P, int32_t heads, int32_t d, void* stream);

/* The same attention with every optional field of csrc/common.h's AttnArgs passed through (null = absent):
 *   bias [heads][2T-1] fp32 + gate [B][heads][T] fp32   WavLM's gated relative position bias (HF modeling_wavlm.py:167-180), in log2 units:
 *                                                       score(q, k) += gate[b][h][q] * bias[h][k - q + T - 1]; head_dim 32 / 64
 *   clip_T [B]                                          valid frames per clip: keys and queries >= clip_T[b] do not exist, their rows of O
 *                                                       are not written; bias and gate stay laid out for the batch-wide T
 *   QK_lo, V_lo (both or neither)                       `model.precision: high`: the operands' low halves, same layout; head_dim 32 / 64
 *                                                       (with or without bias), 128, 256
 *   O_lo                                                the context's low half, bf16(o - O)
 *   O8 (+ O8_lo), ldo8, o8_scale, status                instead of O: e4m3(o * o8_scale) bytes (+ e4m3(16 (o * o8_scale - hi))); an element
 *                                                       that saturates is stored as +-448 and ORs 2 into *status; head_dim 64, no bias,
 *                                                       no QK_lo / V_lo / O_lo
 * A combination attention.hip has no kernel for is an error status: nothing is launched. */
int32_t wfl_op_attention_ex(const void* QK, const void* QK_lo, int64_t ldqk, int64_t lead, const void* V, const void* V_lo, int64_t ldv,
                            void* O, void* O_lo, int64_t ldo, int32_t B, int32_t T, int32_t P, int32_t heads, int32_t d, const float* bias,
                            const float* gate, const int32_t* clip_T, void* O8, void* O8_lo, int64_t ldo8, float o8_scale, int32_t* status,
                            void* stream);

/* WavLM's relative position table (HF modeling_wavlm.py:243-271, gathered once per forward):
 *   table[h][delta + T - 1] = rel_emb[bucket_of_delta[delta + max_t - 1]][h],  delta = key - query in [-(T-1), T-1];  T <= max_t.
 * rel_emb [buckets][heads] fp32, bucket_of_delta [2 max_t - 1] int32, table [heads][2T-1] fp32. */
int32_t wfl_op_relpos_table(const float* rel_emb, const int32_t* bucket_of_delta, int32_t max_t, int32_t heads, int32_t T, float* table,
                            void* stream);

/* The gate of that bias (HF modeling_wavlm.py:167-180): with (ga, gb) = sigmoid((w8 x_head + b8).view(2, 4).sum(-1)),
 *   gate[b][h][t] = ga * (gb * cst[h] - 1) + 2.
 * x (+ x_lo when given) bf16 frame rows, head h at column h * hd; w8 [8][hd], b8 [8], cst [heads] fp32; hd % 8 == 0, hd <= 128. */
int32_t wfl_op_relpos_gate(const void* x, const void* x_lo, int64_t ldx, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t heads,
                           int32_t hd, const float* w8, const float* b8, const float* cst, float* gate, void* stream);

/* Frame rows x [R][d] -> xg [groups][R][64]: channels g * cpg .. + cpg of every valid frame (t < T, and < clip_T[b] when given), zero in
 * the padding channels and in every other row: the positional conv's operand.  cpg % 8 == 0, cpg <= 64, groups * cpg == d. */
int32_t wfl_op_regroup(const void* x, int32_t d, int32_t groups, int32_t cpg, int64_t R, int64_t lead, int32_t B, int32_t P, int32_t T,
                       const int32_t* clip_T, void* xg, void* stream);

/* Waveform statistics of Wav2Vec2FeatureExtractor's do_normalize (csrc/wavlm.hip): stats[2b] = sum, stats[2b + 1] = sum of squares of
 * the first lens[b] (null: L) samples of clip b, accumulated in float64 in a fixed order.  wav [B][ldw] fp32, stats [2 B] double. */
int32_t wfl_op_wav_stats(const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, double* stats, void* stream);

/* Frames per clip at every level of a conv stack without padding: t = clamp(lens[b], 0, L), below min_len no frames at any level, then
 * per level t <- t >= kernel[i] ? (t - kernel[i]) / stride[i] + 1 : 0; out[i * B + b].  lens and out are device arrays, kernel and
 * stride HOST arrays of n entries, 1 <= n <= 8, stride > 0.  (kernel 0, stride hop, min_len 201: the mel front-end's 1 + len / hop.) */
int32_t wfl_op_clip_frames(const int32_t* lens, int32_t B, int32_t L, int32_t n, const int32_t* kernel, const int32_t* stride,
                           int32_t min_len, int32_t* out, void* stream);

/* Level 0 of WavLM's feature encoder (csrc/wavlm.hip; HF modeling_wavlm.py:675-744): every field of csrc/common.h's Conv0Args.
 *   x = (wav - mean) / sqrt(var + 1e-7) from wstats (wfl_op_wav_stats' output over the clip's own lens[b] samples; null: x = wav),
 *   y[t][c] = sum_j w[c][j] x[5 t + j]   (k = 10, stride 5, no padding; T0 frames, a clip with lens has (lens[b] - 10) / 5 + 1, none below 10)
 *   group_norm != 0: out = gelu(gamma (y - mean_c) rstd_c + beta), statistics per (clip, channel) over the clip's own frames, eps 1e-5.
 *                    The conv bias is NOT read in this mode: per-channel GroupNorm removes a per-channel constant.  Needs `scratch`:
 *                    16-byte aligned, wfl_op_conv0_scratch_bytes(B, T0, C) bytes, overwritten.
 *   group_norm == 0: out = gelu(LayerNorm_C(y + bias)), eps 1e-5 (bias null: none); scratch is not used.
 * out (+ out_lo = bf16(value - out) when given): bf16 frame rows of C channels, row lead + b P + t; rows at t >= the clip's own frame
 * count are not written.  w [C][10], bias / gamma / beta [C] fp32.  C % 8 == 0, C <= 512, 0 < T0 <= (L - 10) / 5 + 1, P >= T0;
 * lens[b] <= L is the caller's to keep.  An argument error is an error status and nothing is launched. */
int64_t wfl_op_conv0_scratch_bytes(int32_t B, int32_t T0, int32_t C);
int32_t wfl_op_conv0(const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, const double* wstats, const float* w,
                     const float* bias, const float* gamma, const float* beta, int32_t C, int32_t T0, void* out, void* out_lo,
                     int64_t lead, int32_t P, int32_t group_norm, void* scratch, int64_t scratch_bytes, void* stream);

/* WavLM's positional convolution on regrouped rows (csrc/posconv.hip; HF modeling_wavlm.py:48-90):
 *   out = res (+ res_lo) + gelu( grouped conv1d(x, taps, padding taps / 2)[..., :-1] + bias ),  out_lo = bf16(out - bf16(out)) when given.
 * w [groups][64][ldw] bf16, element (o, tap * 64 + c), zero beyond cpg in o and c -- all 64 rows of a group are read; bias [groups][64] fp32;
 * res / out rows of `ld` channels, group g at column g * cpg.  groups <= 16, cpg % 8 == 0, taps even in 4 .. 128, ldw >= 64 taps,
 * lead >= taps / 2 and at least taps / 2 zero rows between clips.  A shape the kernel does not take is an error status. */
int32_t wfl_op_posconv(const void* xg, int64_t R, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t groups, int32_t cpg, int32_t taps,
                       const void* w, int64_t ldw, const float* bias, const void* res, const void* res_lo, void* out, void* out_lo,
                       int64_t ld, const int32_t* clip_T, void* stream);

/* LayerNorm with everything csrc/norm.hip's launcher takes: input and output as bf16 pairs (x_lo, y_lo: optional), statistics over the
 * first n_div channels (0: C; the columns beyond carry zeros and gamma = beta = 0), exact-erf GELU after the affine (gelu != 0), per-clip
 * frame counts (rows t >= clip_T[b] are left alone).  y may be x. */
int32_t wfl_op_layernorm_act(const void* x, const void* x_lo, int64_t ldx, void* y, void* y_lo, int64_t ldy, const float* gamma,
                             const float* beta, float eps, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t C, int32_t n_div,
                             int32_t gelu, const int32_t* clip_T, void* stream);

/* y1 = LN1(x), y2 = LN2(y1) in one pass over the rows, bit for bit what two wfl_op_layernorm_act launches write.  y2 may be x; y1 may
 * be neither x nor y2. */
int32_t wfl_op_layernorm_pair(const void* x, const void* x_lo, void* y1, void* y1_lo, void* y2, void* y2_lo, int64_t ld, const float* gamma1,
                              const float* beta1, const float* gamma2, const float* beta2, float eps, int64_t lead, int32_t B, int32_t P,
                              int32_t T, int32_t C, int32_t n_div, const int32_t* clip_T, void* stream);

/* fp8 x fp8 GEMM on the block-scaled MFMA (csrc/gemm_mx.hip, round 4; the encoder GEMMs of an fp8-weight model, HF modeling_whisper.py:
 * 309-354, 391-407 via /root/reference/model.py:155-156):
 *   C[row(b,t)][n] = res + alpha * act( w_scale[n] * sa(m) * sum_k a(m, k) W8[n][k] + bias[n] )
 * W8 [N][K] OCP e4m3 bytes; a(m, k) = A8[m][k] (e4m3 bytes, lda bytes per row), or A8[m][k] + A8_lo[m][k] / 16 when A8_lo is given
 * (an e4m3 PAIR: lo = e4m3(16 (x / sa - hi))); sa(m) = a_scale[m] or a_static when a_scale is null.  N % 256 == 0, K % 128 == 0, K >= 512.
 * res / res_lo / c_lo are bf16 rows with C's leading dimension and row mapping.
 * Output: bf16 rows C (+ the low half c_lo with a residual), or -- c8 given -- e4m3(out * c8_inv_scale) into c8 and, c8_lo given, the
 * remainder e4m3(16 (out * c8_inv_scale - hi)) into c8_lo (ldc8 bytes per row); a stored element that saturates or is NaN ORs 2 into
 * *status (elements that are not stored -- rows t >= T -- are not judged). */
int32_t wfl_op_gemm_mx(const void* A8, const void* A8_lo, int64_t lda, const void* W8, const float* w_scale, const float* a_scale,
                       float a_static, int32_t M, int32_t N, int32_t K, int32_t P, int32_t T, void* C, int64_t ldc, int64_t c_lead,
                       int32_t c_pitch, const float* bias, const void* res, const void* res_lo, void* c_lo, float alpha, int32_t act,
                       void* c8, void* c8_lo, int64_t ldc8, float c8_inv_scale, int32_t* status, void* stream);

/* Frame rows -> e4m3 with one fp32 scale per row (row maximum -> 448), optionally LayerNorm(gamma, beta, eps) first (gamma null: plain
 * quantisation) and optionally as a PAIR (y8_lo given: e4m3(16 (x / scale - hi))): the producers of gemm_mx's frame operand
 * (csrc/norm.hip rows_fp8_kernel; HF modeling_whisper.py:384, 399).  x (+ x_lo when given) are bf16 rows, C % 8 == 0, C <= 2048. */
int32_t wfl_op_rows_fp8(const void* x, int64_t ldx, const void* x_lo, const float* gamma, const float* beta, float eps, int64_t lead,
                        int32_t B, int32_t P, int32_t T, int32_t C, void* y8, void* y8_lo, int64_t ldy8, float* scale, void* stream);

int32_t wfl_op_layernorm(const void* x, int64_t ldx, void* y, int64_t ldy, const float* gamma, const float* beta,
                         float eps, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t C, void* stream);

/* softmax max-prob / argmax / threshold over fp32 logits rows (infer.py:86-96). */
int32_t wfl_op_tag_decide(const float* logits, int64_t ldl, int32_t rows, int32_t C, float threshold, int32_t o_id,
                          int32_t* ids, int32_t* argmax, float* maxprob, void* stream);

/* One BiLSTM layer's recurrence (csrc/lstm.hip; nn.LSTM at model.py:104-111 behind its input projection), every field of csrc/common.h's
 * LstmArgs:   gates_t = gx_t + W_hh h_(t-1),  c_t = f c_(t-1) + i g,  h_t = o tanh(c_t),  zero initial state, both directions in one launch.
 *   gx      fp32 frame rows (row lead + b P + t, ldgx floats per row): the input projection x W_ih^T + b_ih + b_hh of both directions,
 *           column dir * 4H + 4 * unit + gate (gate 0 .. 3 = i, f, g, o; dir 0 forward, 1 backward)
 *   out     bf16 frame rows (same row mapping, ldo per row): column dir * H + unit.  Rows t >= T (>= clip_T[b] when given), the rows
 *           between clips and the columns beyond 2H are not written.  A clip's rows do not depend on the other clips of the batch.
 *   whh     wfl_op_lstm_pack_whh's hi output on the device, packed for the U passed here
 *   whh_lo + out_lo (both or neither)   `model.precision: high`: W_hh and h as bf16 pairs hi + lo, three MFMA passes; out_lo = bf16(h - out)
 *   clip_T  [B] int32 on the device or null: frames per clip, 0 <= clip_T[b] <= T; the backward direction of clip b starts at its own last frame
 *   U       hidden units per workgroup: a multiple of 8, at most 32, dividing H, H / U <= 64; <= 0: the default for H
 *   exchange   device scratch through which the workgroups of a direction hand h to each other, 16-byte aligned, at least
 *           wfl_op_lstm_exchange_bytes(H, B) bytes; the launch clears it itself, so any content may be passed and it may be reused
 *   status  device error word, required: a hand-off wait that gives up ORs 1 into it (the output is invalid then); never cleared here
 * H is one of 32, 64, 128, 192, 256, 384, 512, 640.  ldgx % 4 == 0, ldgx >= 8H, ldo % 8 == 0, ldo >= 2H, P >= T >= 1, B >= 1.  Anything
 * else is an error status with a wfl_last_error() text, and nothing is launched.
 * wfl_op_lstm_pack_whh (host only): weight_hh of both directions, [2][4H][H] fp32 in PyTorch's row order (blocks i | f | g | o of H rows)
 * -> the slice-major [2][H / U][4U][H] bf16 high halves (row 4 * u_local + gate of slice unit / U) and, lo_host not null, the low halves
 * bf16(w - hi) in the same layout.  The model loader packs with this function. */
int64_t wfl_op_lstm_exchange_bytes(int32_t H, int32_t B);
int32_t wfl_op_lstm_pack_whh(const float* whh_host, int32_t H, int32_t U, uint16_t* hi_host, uint16_t* lo_host);
int32_t wfl_op_lstm(const float* gx, int64_t ldgx, const void* whh, const void* whh_lo, void* out, void* out_lo, int64_t ldo,
                    int64_t lead, int32_t B, int32_t T, int32_t P, int32_t H, int32_t U, const int32_t* clip_T,
                    void* exchange, int64_t exchange_bytes, int32_t* status, void* stream);

/* Per-kernel timing hook for bench.py's roofline: when enabled, wfl_forward brackets every GEMM launch with
 * hipEvents on `stream`.  wfl_gemm_profile_read synchronises on them and returns, per GEMM kernel variant
 * (key = act | glu<<2 | out_f32<<3 | res<<4 | kernel<<5 | ln_fold<<8 | stats<<10, one template instantiation = one
 * rocprof kernel name), the launch
 * count, summed milliseconds and summed algorithmic FLOPs (2 * valid_rows * n_valid * K) since the last reset. */
int32_t wfl_gemm_profile_enable(wfl_model* m, int32_t on);
int32_t wfl_gemm_profile_read(wfl_model* m, int32_t max_variants, int32_t* keys, int64_t* launches, double* total_ms,
                              double* total_flops, int32_t* n_variants, int32_t reset);

/* ---- host-side label logic (no device access): thresholded ids + offsets of one clip -> segments -> .lab text.
 * Replaces the per-frame Python of /root/reference/utils.py:10-81, 148-186 and the scipy median filter call at
 * /root/reference/infer.py:170-171, 298-299; bit-exact with them (times are doubles computed in the same order).
 *   kind[c] : 0 the "O" tag, 1 "B-x", 2 "I-x", 3 anything else (ignored);  phon[c] : phoneme index of tag c (-1 for "O")
 *   merge mode : 0 none, 1 right, 2 left, 3 previous (config postprocess.merge_segments)
 * wfl_host_decode_bio returns the number of segments (-3 when max_segments was too small, -4 when a run closes at a frame
 * beyond the n_off offsets rows, where the reference raises IndexError), wfl_host_merge_segments the
 * new count (in place), wfl_host_format_lab the number of bytes the text needs (written only if it fits in cap). */
int32_t wfl_host_median_filter(const int32_t* ids, int32_t n, int32_t size, int32_t* out);
int32_t wfl_host_decode_bio(const int32_t* ids, int32_t T, const float* offsets, int32_t n_off, const int32_t* kind,
                            const int32_t* phon, int32_t n_labels, double frame_duration, double* seg_start,
                            double* seg_end, int32_t* seg_ph, int32_t max_segments);
int32_t wfl_host_merge_segments(double* start, double* end, int32_t* ph, int32_t n, int32_t mode);
int64_t wfl_host_format_lab(const double* start, const double* end, const int32_t* ph, int32_t n,
                            const char* const* names, int32_t n_names, char* out, int64_t cap);

/* ---- audio ingest on the host (replaces soundfile.read + the float64 peak normalisation of /root/reference/infer.py:217-218,
 * 234-235 for 16-bit/24-bit/32-bit/float WAV files with 1 or 2 channels): decode, mono mix, audio / (max|audio| + 1e-8) in
 * float64, stored as float32 -- bit-identical to wfl-asr_amd/audio.py.  status: 0 ok, 1 unsupported encoding, 2 more than two
 * channels, 3 longer than cap samples (n_samples = the length), 4 cannot open.  The sample rate is reported, not converted.
 * wfl_host_load_wavs fills rows out + i * ld of a batch buffer with `threads` worker threads. */
int32_t wfl_host_load_wav(const char* path, float* out, int64_t cap, int32_t* n_samples, int32_t* sample_rate);
int32_t wfl_host_load_wavs(const char* const* paths, int32_t n, float* out, int64_t ld, int64_t cap, int32_t* n_samples,
                           int32_t* sample_rates, int32_t* status, int32_t threads);

/* The general ingest path of ONE file (replaces /root/reference/infer.py:217-220 soundfile.read + torchaudio resample, 234-235
 * whole-clip peak normalisation, 237-244 + 19-28 split_audio for clips longer than chunk_samples, 114-115 per-chunk
 * re-normalisation): rows out + r * ld receive the float32 work items, lens[r] their lengths.  Resampling = torchaudio's sinc /
 * Hann algorithm restated (parity with torchaudio UNPINNED: library absent).  Status as wfl_host_load_wav, 5 = more than max_rows
 * chunks (n_rows = the count needed, nothing written). */
int32_t wfl_host_load_wav_chunks(const char* path, int32_t target_sr, int64_t chunk_samples, float* out, int64_t ld, int32_t max_rows,
                                 int32_t* n_rows, int32_t* lens, int32_t* sample_rate);

/* ---- audio ingest on the GPU (round 3): a file that is not at the model's rate no longer costs host cores.
 * wfl_host_read_pcm16 copies the 16-bit PCM samples of `n` WAV files as they are (interleaved, 1 or 2 channels) into rows
 * out + i * ld of a (pinned) int16 buffer -- status 0 ok, 1 not 16-bit PCM, 2 more than two channels, 3 more than cap_samples values,
 * 4 cannot open.  wfl_resample_pcm16 (device pointers, one HIP stream) turns B such rows of ONE sample rate into float32 rows ready
 * for wfl_forward: decode ((l + r) / 2 for two channels), band-limited sinc resampling to new_sr -- torchaudio.functional.resample's
 * published algorithm in float64 (/root/reference/infer.py:217-220; parity with torchaudio UNPINNED: library absent), bit-identical to
 * wfl_host_load_wav_chunks -- and whole-clip peak normalisation x / (max|x| + 1e-8) in float64 (infer.py:234-235).  Row b of `out`
 * receives min(ceil(len_b * new_sr / orig_sr), out_cap) samples followed by zeros up to out_cap; clips that come out longer than
 * out_cap (= 30 s: they would be cut into chunks) belong to wfl_host_load_wav_chunks.  orig_sr == new_sr is taken (round 4): no
 * resampling, as torchaudio returns such a waveform as it is -- decode and normalisation only. */
int32_t wfl_host_read_pcm16(const char* const* paths, int32_t n, int16_t* out, int64_t ld, int64_t cap_samples, int32_t* n_frames,
                            int32_t* channels, int32_t* sample_rates, int32_t* status, int32_t threads);
int64_t wfl_resample_workspace_bytes(int32_t B, int32_t out_cap);
int32_t wfl_resample_pcm16(const int16_t* pcm, int64_t ld_in, const int32_t* n_in, const int32_t* channels, int32_t B, int32_t orig_sr,
                           int32_t new_sr, float* out, int64_t ld_out, int32_t out_cap, void* workspace, int64_t workspace_bytes,
                           void* stream);

/* ---- boundary-snapping features on the GPU (round 3; /root/reference/correct_label.py:15-24, the step the
 * reference's notebook runs after inference): for B clips of up to L samples at 16 kHz (device pointers, one HIP stream),
 *   flux[b][t]    spectral flux of |librosa.stft(y, n_fft=512, hop_length=160)| (flux[b][0] = 0),
 *   mfcc[b][c][t] librosa.feature.mfcc(y, sr=16000, n_mfcc=13, hop_length=160): n_fft 2048, 128 Slaney mel bands, dB with top_db 80,
 *                 orthonormal DCT-II,
 * t < F = 1 + L / 160.  mel_w [128][1025] and dct [13][128] are the caller's (wfl-asr_amd/correct_label.py builds them; its numpy
 * restatement of the same features is what tests hold this to).  Restated from librosa's documented definitions: parity with librosa
 * itself is UNPINNED (library absent, the reference holds no fixtures). */
int64_t wfl_boundary_workspace_bytes(int32_t B, int32_t L);
int32_t wfl_boundary_features(const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, const float* mel_w,
                              const float* dct, float* flux, float* mfcc, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Viterbi forced alignment on the GPU (`postprocess.align: viterbi`; wfl-asr_amd/align.py).  Replaces, for files that come with a
 * transcript, the greedy in-order string match of /root/reference/infer.py:30-60 over the freely decoded segments (read at 193, 210-215;
 * applied at 312-319) by a search over the frame logits that spells exactly the transcript, in order, one contiguous run per token.
 * Clip b has T = n_frames_host[b] logits rows (row frame_off_host[b] + t, ld ldl, C <= 1024 fp32 columns) and N = n_tok_host[b] tokens
 * (tok_cls rows tok_off_host[b] ..).  Emissions e_t(c) = z[t][c] - logsumexp z[t][.];  token k has 1..4 alternatives (B_j, I_j)
 * (tok_cls[k][j][0..1], -1 -1 = unused), EB_t(k) = max_j e_t(B_j), EI_t(k) = max_j e_t(I_j); EG_t = max over gap_cls[b][0..7] (-1 = unused,
 * at least one).  States G_0, B_0, I_0, G_1, ..., B_{N-1}, I_{N-1}, G_N (G_k = 3k, B_k = 3k + 1, I_k = 3k + 2):
 *     G_k <- {G_k, I_{k-1}, B_{k-1}}    B_k <- {G_k, I_{k-1}, B_{k-1}}    I_k <- {I_k, B_k}        (the first listed wins an exact tie)
 *     start G_0 | B_0, end G_N | I_{N-1} | B_{N-1} (in that order of preference): every token gets >= 1 frame, gaps may be empty.
 * Outputs (device): ids[t] the class on the path (a B frame: the B_j of its arg-max alternative, an I frame: the I_j of its arg-max
 * alternative, a gap frame: o_id), tok[t] = k on B_k / I_k frames and -1 in gaps (same rows as the logits); score[b] the path's sum of
 * e_t (fp32; the search itself decides on the raw logits); status[b]: 0 ok, 1 infeasible (T < N), 2 N above 4096, 4 a class id out of
 * range or no gap class.  A clip with status != 0 gets ids = o_id, tok = -1, score 0.  Clips are independent (one workgroup each): a
 * clip aligned alone equals the same clip inside any batch, bit for bit.  Arguments are checked on the host (negative return): C in
 * 1 .. 1024, o_id in range, ldl >= C, counts and offsets >= 0, non-null pointers, workspace large enough.
 * Workspace: 2-bit backpointers, per clip round_up(T * words(N), 64) 4-byte words, words(N) = 64 (N <= 127), 256 (N <= 1023),
 * 512 (N <= 2047), 1024 (N <= 4096); 0 for a clip with T < N or N > 4096.  wfl_align_workspace_bytes returns that sum in bytes. */
int64_t wfl_align_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                  const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls, const int32_t* gap_cls, int32_t n_clips,
                  void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream);

/* ---- wfl_align inside per-token start windows (`postprocess.align_draft`; wfl-asr_amd/align.py).  wfl_align's arguments plus tok_win
 * (device), [total tokens][2] int32 = (lo, hi), rows as tok_cls: a path is accepted only if, for every token k, the frame t (0-based
 * inside the clip) at which it is in B_k -- the frame where the token opens -- satisfies lo_k <= t <= hi_k (inclusive).  That is
 * EB_t(k) = -inf outside the window; transitions, tie order, start and end states, the other emissions, the renormalisation and the
 * workspace (wfl_align_workspace_bytes) are wfl_align's, and with every window (0, INT32_MAX) so is every output, bit for bit.  The ends of
 * tokens carry no window: an end is not a state event of this lattice.
 * status[b]: wfl_align's codes, 1 now meaning "no path satisfies the windows": T < N, a window with lo > hi, a window at or beyond T,
 * windows that cannot be met in order (the host rule e_k = max(lo_k, e_{k-1} + 1) <= min(hi_k, T - 1), e_{-1} = -1, predicts it exactly).
 * Such a clip gets ids = o_id, tok = -1, score 0; its backpointers are never walked.  A null tok_win with any token present is a host-side
 * -1. */
int32_t wfl_align_windowed(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                           const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, void* workspace, int64_t workspace_bytes,
                           int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream);

/* ---- wfl_align with a minimum duration per token (`postprocess.min_duration`; wfl-asr_amd/align.py).  wfl_align_windowed's arguments
 * (tok_win may be null: no windows) plus tok_min (device), [total tokens] int32, rows as tok_cls: token k occupies at least D_k =
 * tok_min[k] frames, 1 <= D_k <= 8 (0.16 s on the 20 ms clock).  A run of token k is frame 1 in B_k, frames 2 .. D_k - 1 in the chain
 * states H_k^2 .. H_k^{D_k-1}, and every later frame in I_k:
 *     H_k^2(t) = B_k(t-1) + EI_t(k)
 *     H_k^j(t) = H_k^{j-1}(t-1) + EI_t(k)
 *     I_k(t)   = max{ I_k(t-1), X_k(t-1) } + EI_t(k)      X_k = H_k^{D_k-1} for D_k >= 3, B_k for D_k <= 2; I_k first on a tie
 * The token is left from I_k alone, towards G_{k+1} or B_{k+1}; where D_k == 1 also from B_k, as in wfl_align.  End states G_N | I_{N-1},
 * and B_{N-1} only when D_{N-1} == 1.  Chain frames emit the token's I classes and are written to ids / tok exactly as I_k frames are, so
 * the tag string stays BIO-legal and every token keeps one contiguous run, now of at least D_k frames.  G, B, the windows (on EB alone),
 * the other emissions, the tie order, the renormalisation and the workspace (wfl_align_workspace_bytes: the chain needs no backpointer
 * bits) are wfl_align_windowed's, and with every D_k == 1 so is every output, bit for bit (of wfl_align with a null tok_win).
 * status[b]: wfl_align's codes; 1 "no path": T < N, sum of D_k > T, or windows and durations that cannot both be met (the host rule
 * e_k = max(lo_k, e_{k-1} + D_{k-1}) <= hi_k, e_{N-1} + D_{N-1} <= T predicts it); 4 also for a D_k outside 1 .. 8.  Such a clip gets
 * ids = o_id, tok = -1, score 0.  A null tok_min with any token present is a host-side -1. */
int32_t wfl_align_min_duration(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                               const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                               const int32_t* tok_win, const int32_t* tok_min, const int32_t* gap_cls, int32_t n_clips, void* workspace,
                               int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream);

/* ---- wfl_align with optional tokens: a path may leave out a token the user marked (`postprocess.optional_tokens`; wfl-asr_amd/align.py).
 * wfl_align_windowed's arguments (tok_win may be null: no windows) plus tok_opt (device), [total tokens] int32 0 | 1, rows as tok_cls,
 * and skip_penalty = lambda >= 0 in nats.  The lattice gains skip arcs only, no epsilon moves:
 *     B_k <- {G_k, I_{k-1}, B_{k-1}, G_{k-1} - lambda, I_{k-2} - lambda, B_{k-2} - lambda}     (the first listed wins an exact tie)
 * the last three only where tok_opt[k-1] == 1 (I_{k-2}, B_{k-2} also need k >= 2).  G_k and I_k are entered as in wfl_align: a gap in
 * front of a skipped token k - 1 stays in G_{k-1} until B_k opens, there is no G_{k-1} -> G_k arc, so every labelling is exactly one path
 * and at most one token is skipped between two kept ones.  Start: the virtual frame -1 sits in G_0, so with tok_opt[0] == 1 and N >= 2
 * frame 0 may also be B_1, at -lambda.  End: G_N | I_{N-1} | B_{N-1}, and where tok_opt[N-1] == 1 | G_{N-1} - lambda | I_{N-2} - lambda |
 * B_{N-2} - lambda.  Windows mask EB alone and a skipped token's window is never consulted: an optional token with an empty window
 * (lo > hi) is a token that must be skipped.  With every flag 0 every output is wfl_align's (null tok_win) or wfl_align_windowed's, bit
 * for bit, for any lambda.
 * Outputs: ids, tok as wfl_align's (a skipped token never appears in tok); skipped[k] (device, [total tokens] int32) 1 for a token the
 * path left out, else 0; score[b] the path's sum of e_t minus lambda times its skipped tokens.  status[b]: wfl_align's codes; 1 "no
 * path": fewer frames than N minus, over every maximal run of optional tokens, ceil(run / 2) (and T >= 1), or windows that cannot be met;
 * 4 also for a flag other than 0 | 1.  A clip with status != 0 gets ids = o_id, tok = -1, skipped = 0, score 0; its backpointers are never
 * walked.  Host-side negative returns as wfl_align's, and: a null tok_opt or skipped with any token present, a negative, infinite or NaN
 * skip_penalty.
 * Workspace: wfl_align's words (2 bits G, 3 bits B, 1 bit I per slot and frame: the same 6), but a clip with T < N may have a path here
 * and keeps its round_up(T * words(N), 64) words.  wfl_align_optional_workspace_bytes returns that sum: wfl_align_workspace_bytes' own
 * figure for every batch whose clips all have T >= N. */
int64_t wfl_align_optional_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_optional(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                           const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* tok_opt, float skip_penalty,
                           void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* skipped,
                           int32_t* status, void* stream);

/* ---- wfl_align over a transcript GRAPH: pronunciation variants, several spellings of a stretch of the transcript, chosen jointly by the
 * search (`postprocess.transcript_variants`; wfl-asr_amd/align.py, csrc/align_graph.hip).  Clip b has N = n_slots_host[b] slots in
 * topological order (rows slot_off_host[b] .. of tok_cls, slot_pred, slot_final and taken).  Slot k carries tok_cls exactly as a wfl_align
 * token does, a predecessor list slot_pred[k][0..7] (int32, the used entries first: -1 = START, -2 = unused, otherwise a clip-local slot
 * j with k - 255 <= j < k) and slot_final[k] in {0, 1}.  States G_k, B_k, I_k per slot and one end gap G_end:
 *     m_k(t)   = max{ G_k, then for p in pred(k) in list order: I_p, B_p }  of frame t - 1      (the first listed wins an exact tie)
 *     G_k(t)   = m_k(t) + EG_t        B_k(t) = m_k(t) + EB_t(k)        I_k(t) = max{I_k, B_k}(t-1) + EI_t(k)
 *     G_end(t) = max{ G_end, then for final f in slot order: I_f, B_f }(t-1) + EG_t
 *     start: frame 0 is G_k or B_k of a slot that lists START (G_end when N == 0)
 *     end:   G_end | I_f | B_f over the final slots, in that order
 * Emissions, gap classes, the decisions on the raw logits, the renormalisation every 16 frames and the meaning of score are wfl_align's.
 * With pred(k) = {k - 1}, START for slot 0 and slot N - 1 alone final this is wfl_align's lattice state for state (G_k its G_k, G_end its
 * G_N), and ids, tok and status are wfl_align's.
 * Outputs (device): ids and tok per frame as wfl_align writes them, tok the clip-local slot or -1 in a gap; score[b]; taken[k] ([total
 * slots] int32) 1 for a slot the path visits, else 0.  status[b]: 0 ok; 1 no path (the best end state is -inf, found as the windowed
 * kernels find it: every way through the graph needs more frames than T, or no slot lists START); 2 N > 2047; 4 a bad class or no gap
 * class, a slot without a predecessor, a predecessor >= k, < -2 or more than 255 slots back, a used entry behind an unused one, a
 * slot_final other than 0 | 1, N > 0 and no final slot.  A clip with status != 0 gets ids = o_id, tok = -1, taken = 0, score 0; its
 * backpointers are never walked.  Clips are independent (one workgroup each): a clip aligned alone equals the same clip inside any
 * batch, bit for bit.  Host-side negative returns as wfl_align's, and: a null slot_pred, slot_final or taken with any slot present.
 * Workspace: 8 bits per slot and frame (4 the choice of m_k, 1 I_k's, 1 "X_k = max{I_k, B_k} was B_k") in wfl_align's words per thread,
 * and one word per frame for G_end's choice: per clip round_up(T * (words(N) + 1), 64) 4-byte words, words(N) = 64 (N <= 127), 256
 * (N <= 1023), 512 (N <= 2047); 0 for a clip with T == 0 or N > 2047.  wfl_align_graph_workspace_bytes returns that sum in bytes. */
int64_t wfl_align_graph_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_slots_host, int32_t n_clips);
int32_t wfl_align_graph(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                        const int32_t* n_frames_host, const int32_t* slot_off_host, const int32_t* n_slots_host, const int32_t* tok_cls,
                        const int32_t* gap_cls, int32_t n_clips, const int32_t* slot_pred, const int32_t* slot_final, void* workspace,
                        int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* taken, int32_t* status, void* stream);

/* ---- wfl_align with filler tokens: a token that matches anything, for a stretch of audio the transcript does not spell
 * (`postprocess.filler_token`; wfl-asr_amd/align.py).  wfl_align_windowed's arguments (tok_win may be null: no windows) plus tok_fill
 * (device), [total tokens] int32 0 | 1, rows as tok_cls, and filler_penalty = phi >= 0 in nats per frame.  The states, arcs and tie rules
 * are wfl_align's; only the emission of a flagged token differs:
 *     EB_t(k) = EI_t(k) = max_{0 <= c < C} z_t[c] - phi        where tok_fill[k] == 1
 * the maximum over ALL classes, the gap classes included, so a frame goes to a filler instead of a neighbouring token only where that
 * token's class is more than phi below the frame's best class.  Windows mask EB of a filler like any token's.  A flagged token's tok_cls
 * row must still hold one valid pair (the host writes (o_id, o_id)); it is never read for emissions.  With every flag 0 every output is
 * wfl_align's (null tok_win) or wfl_align_windowed's, bit for bit, for any phi.
 * Outputs: in a filler's frames tok[t] = k and ids[t] is the frame's first arg-max class over all C (the lowest index on a tie);
 * everywhere else ids, tok as wfl_align's; score[b] = sum e_t - sum lse_t as wfl_align's.  status[b]: wfl_align's codes (1: T < N, or
 * windows no path meets; 2 over the cap); 4 also for a flag other than 0 | 1.  A clip with status != 0 gets ids = o_id, tok = -1, score 0.
 * Host-side negative returns as wfl_align's, and: a null tok_fill with any token present, a negative, infinite or NaN filler_penalty.
 * Workspace: wfl_align's own figure (wfl_align_filler_workspace_bytes returns wfl_align_workspace_bytes' sum). */
int64_t wfl_align_filler_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_filler(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                         const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                         const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* tok_fill, float filler_penalty,
                         void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status,
                         void* stream);

/* ---- wfl_align with a duration prior per token: an explicit-duration (semi-Markov) Viterbi search (`postprocess.duration_prior`;
 * wfl-asr_amd/align.py viterbi_align_duration_prior, csrc/align_duration_prior.hip).  wfl_align_windowed's arguments up to n_clips
 * (tok_win may be null: no windows), then the prior: dur (device), [n_rows][D + 1] fp32, 1 <= D <= 32 -- columns 0 .. D - 1 are
 * L(1) .. L(D), column D is `tail`; every entry finite or -inf, never NaN or +inf, tail <= 0 or -inf (the caller's contract, as for
 * wfl_decode_bigram's trans) -- and tok_dur (device), [total tokens] int32, rows as tok_cls: the row of token k, -1 for no prior
 * (L = 0, tail = 0).  A run of d frames of token k (one B frame, d - 1 I frames) with row r adds
 *     L_k(d) = dur[r][d-1]                          1 <= d <= D
 *            = dur[r][D-1] + (d - D) * dur[r][D]    d >  D
 * to the path's score (gaps carry no prior), so hard minimum and maximum durations are rows with -inf entries.  Frame by frame, every
 * quantity of frame t - 1 on the right:
 *     Ent_k(t) = max(G_k(t-1), X_{k-1}(t-1))          Ent_0(0) = 0, every other Ent_k(0) = -inf; G first on a tie
 *     G_k(t)   = Ent_k(t) + EG_t
 *     R_k^1(t) = Ent_k(t) + EB_t(k)                   (EB through the window where tok_win is given)
 *     R_k^j(t) = R_k^{j-1}(t-1) + EI_t(k)             2 <= j <= D: a run of exactly j frames, prior not yet added
 *     Y_k(t)   = max(Y_k(t-1), R_k^D(t-1) + L_k(D)) + EI_t(k) + tail_k      a run longer than D; Y first on a tie
 *     X_k(t)   = max(max_j R_k^j(t) + L_k(j), Y_k(t))      frame t is the last frame of token k; shortest j first, Y last on a tie
 *     end      = max(G_N(T-1), X_{N-1}(T-1))          G first
 * Emissions, alternatives, gap classes and windows are wfl_align_windowed's; the search decides on the raw logits and no expression
 * forms inf - inf.  Outputs: ids and tok as wfl_align's (a run's first frame carries its arg-max alternative's B class, every later
 * frame that frame's arg-max alternative's I class); score[b] the path's sum of e_t plus the sum of L_k(d_k).  status[b]: wfl_align's
 * codes; 1 "no path of finite score": T < N, or the table or the windows forbid every path; 2 N above 4096; 4 also a tok_dur outside
 * -1 .. n_rows - 1.  A clip with status != 0 gets ids = o_id, tok = -1, score 0 and does not disturb its batch; one workgroup per clip,
 * a clip aligned alone equals the same clip inside any batch, bit for bit.  Host-side negative returns: wfl_align's, and a null tok_dur
 * with any token present, a null dur with n_rows > 0, n_rows < 0, D outside 1 .. 32, a workspace that is too small.
 * Workspace: one backpointer byte per token slot and frame, and the history of the D run scores of every slot where the workgroup's LDS
 * does not hold it: per clip, in 4-byte words (0 for a clip with T < N, T = 0 or N > 4096),
 *     round_up_64(T * words(N)) + ring(N, D),   words(N) = 64 (N <= 127), 256 (N <= 1023), 512 (N <= 2047), 1536 (N <= 4096),
 *     ring(N, D) = 0 for N <= 511; round_up_64(slots(N) * D) where D > 23 (N <= 1023), D > 9 (N <= 2047), D > 1 (N <= 4096), else 0,
 *     slots(N) = 1024 (N <= 1023), 2048 (N <= 2047), 4608 (N <= 4096). */
int64_t wfl_align_duration_prior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips, int32_t D);
int32_t wfl_align_duration_prior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                 const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                 const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                 const int32_t* tok_dur, const float* dur, int32_t n_rows, int32_t D, void* workspace,
                                 int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream);

/* ---- Posteriors of a Viterbi alignment by forward-backward on the GPU (`postprocess.align_scores`; wfl-asr_amd/align.py).  No
 * counterpart in the reference, which reports no confidence for its string match.  The lattice, emissions EB / EI / EG, start and end
 * states, caps (C <= 1024, N <= 4096) and argument conventions are wfl_align's.  The weight of a path is exp(sum_t e_t(state_t));
 * alpha_t(s) / beta_t(s) are the log-sums of the weights of the path prefixes ending in / suffixes leaving s at frame t over wfl_align's
 * transitions:
 *     logZ = log sum over all accepted paths,        gamma_t(s) = exp(alpha_t(s) + beta_t(s) - logZ).
 * tok (device) is wfl_align's output for the same clips (row frame_off_host[b] + t).  Outputs (device):
 *   logz[b]        logZ of the clip (fp32);
 *   tok_post[k]    (rows tok_off_host[b] + k) the mean over the frames t with tok[t] == k of gamma_t(B_k) + gamma_t(I_k): the posterior
 *                  occupancy of the run Viterbi chose, in [0, 1] (clamped to 1 from above);
 *   start_mean[k], start_sd[k]   mean and standard deviation, in frames, of the token's start frame: a path visits B_k in exactly one
 *                  frame, so gamma_.(B_k) is that frame's posterior distribution (sum_t gamma_t(B_k) = 1; the moments are divided by the
 *                  computed sum, which is 1 up to rounding).  start_mean is relative to the first frame with tok[t] == k (Viterbi's
 *                  start); the moments are accumulated about that frame, in double;
 *   status[b]      wfl_align's codes (0 ok, 1 infeasible, 2 N above 4096, 4 a class id out of range or no gap class), and 8: tok does not
 *                  contain every token 0 .. N - 1 or holds a value outside -1 .. N - 1 (not a path of this lattice).  A clip with
 *                  status != 0 gets logz = 0 and tok_post = start_mean = start_sd = 0.
 * One workgroup per clip: a clip scored alone equals the same clip inside any batch, bit for bit.  fp32 log-domain states, renormalised
 * every 16 frames (offsets in double).  Arguments are checked on the host as wfl_align checks its own (negative return).
 * Workspace: the alpha lattice is not stored.  Per clip, in 4-byte words, round_up_64 of
 *     round_up_64(T) + round_up_64(2 nblk) + (nblk + 128) * 3 * slots(N),   nblk = ceil(T / 128),
 * (the frames' log-sum-exp, alpha checkpoints every 128 frames with their offsets, one recomputed 128-frame block of alpha);
 * slots(N) = 128 (N <= 127), 512 (N <= 511), 1024 (N <= 1023), 2048 (N <= 2047), 4608 (above); 0 for T = 0.  13.7 MB at T = 15000,
 * N = 4096.  wfl_align_posterior_workspace_bytes returns the sum in bytes. */
int64_t wfl_align_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                            const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                            const int32_t* gap_cls, int32_t n_clips, const int32_t* tok, void* workspace, int64_t workspace_bytes,
                            float* logz, float* tok_post, float* start_mean, float* start_sd, int32_t* status, void* stream);

/* ---- wfl_align_posterior over the windowed lattice of wfl_align_windowed: the same tok_win (device, [total tokens][2] = (lo, hi)), the
 * same mask EB_t(k) = -inf outside [lo_k, hi_k] in alpha and in beta, so logZ sums and gamma normalises over exactly the paths the
 * windowed search chose among.  Workspace and outputs are wfl_align_posterior's (bit for bit with every window open); every token's
 * start distribution lies inside its window, a token with lo == hi has start_sd 0.  status[b] adds: 8 also when a token's first frame
 * in tok lies outside its window (such a tok is not a path of this lattice), 1 also when no path satisfies the windows (logZ = -inf).
 * A null tok_win with any token present is a host-side -1. */
int32_t wfl_align_posterior_windowed(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                     const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                     const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                     const int32_t* tok, void* workspace, int64_t workspace_bytes, float* logz, float* tok_post,
                                     float* start_mean, float* start_sd, int32_t* status, void* stream);

/* ---- wfl_align_posterior over the minimum-duration lattice of wfl_align_min_duration (`postprocess.duration_scores`;
 * wfl-asr_amd/align.py duration_posteriors).  wfl_align_posterior_windowed's arguments (tok_win may be null: no windows) plus tok_min
 * (device, [total tokens] int32, 1 <= D_k <= 8), the table the search was given; tok is wfl_align_min_duration's output.  The sums run
 * over that search's expanded states, B_k, H_k^2 .. H_k^{D_k-1} (emitting EI) and I_k per token:
 *     alpha: G_k and B_k are entered from G_k, I_{k-1}, and from B_{k-1} only where D_{k-1} == 1; H_k^2 from B_k, H_k^j from H_k^{j-1};
 *            I_k from I_k and from X_k (H_k^{D_k-1} for D_k >= 3, B_k for D_k <= 2).  End states G_N | I_{N-1}, B_{N-1} only for D == 1.
 *     beta:  beta_{t-1}(I_k) = lse(beta_t(I_k) + EI_t(k), beta_t(G_{k+1}) + EG_t, beta_t(B_{k+1}) + EB_t(k+1)); beta_{t-1}(B_k) is that
 *            value where D_k == 1, beta_t(I_k) + EI_t(k) where D_k == 2, beta_t(H_k^2) + EI_t(k) above; beta_{t-1}(H_k^j) =
 *            beta_t(H_k^{j+1}) + EI_t(k), the last chain state going to I_k: a delay line per token, the mirror of alpha's chain.
 * Outputs as wfl_align_posterior's: logz[b] the log weight of every path that meets the durations (and the windows); tok_post[k] the
 * mean over the frames of Viterbi's run of the posterior of being in ANY state of token k (B_k, its chain, I_k); start_mean / start_sd
 * from gamma(B_k).  A path in B_k at frame t is in H_k^j at t + j - 1, so gamma_t(H_k^j) = gamma_{t-j+1}(B_k) and the chain's occupancy
 * is taken from gamma(B_k): the recomputed block holds G, B, I alone, only the checkpoints hold the chain.  With every D_k == 1 the
 * outputs are wfl_align_posterior's (wfl_align_posterior_windowed's).
 * status[b]: 2 over the cap; 1 T < N, or no path meets durations and windows (logZ = -inf); 4 a bad class or a D_k outside 1 .. 8;
 * 8 tok is not a path of this lattice: a token missing, a token opening outside its window, or a run shorter than its D_k.  1 comes
 * before 8: a clip without any path is status 1 whatever tok holds (wfl_align_min_duration writes tok = -1 for it).  A clip with
 * status != 0 gets zeros.  A null tok_min with any token present is a host-side -1.
 * Workspace: wfl_align_posterior's with checkpoints of 9 instead of 3 floats per slot: per clip, in 4-byte words, round_up_64 of
 *     round_up_64(T) + round_up_64(2 nblk) + (9 nblk + 3 * 128) * slots(N),   nblk = ceil(T / 128). */
int64_t wfl_align_min_duration_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_min_duration_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                         const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                         const int32_t* tok_cls, const int32_t* tok_win, const int32_t* tok_min, const int32_t* gap_cls,
                                         int32_t n_clips, const int32_t* tok, void* workspace, int64_t workspace_bytes, float* logz,
                                         float* tok_post, float* start_mean, float* start_sd, int32_t* status, void* stream);

/* ---- wfl_align_posterior over the skip lattice of wfl_align_optional (`postprocess.optional_scores`; wfl-asr_amd/align.py
 * optional_posteriors).  wfl_align_posterior_windowed's arguments (tok_win may be null: no windows) plus tok_opt and skip_penalty =
 * lambda, the table and the penalty the search was given; tok is wfl_align_optional's output.  A path weighs
 * exp(sum_t e_t - lambda * its skipped tokens), emissions normalised per frame as in wfl_align_posterior.  With
 * in_k(t) = lse(alpha_{t-1}(G_k), alpha_{t-1}(I_{k-1}), alpha_{t-1}(B_{k-1})):
 *     alpha_t(G_k) = EG_t + in_k(t),    alpha_t(I_k) as wfl_align_posterior's,
 *     alpha_t(B_k) = EB_t(k) + lse(in_k(t), in_{k-1}(t) - lambda where tok_opt[k-1]);
 *     beta_{t-1}(G_k) = lse(beta_t(G_k) + EG_t, beta_t(B_k) + EB_t(k), beta_t(B_{k+1}) + EB_t(k+1) - lambda where tok_opt[k]),
 *     beta_{t-1}(B_k) = beta_{t-1}(I_k) = lse(wfl_align_posterior's three, beta_t(B_{k+2}) + EB_t(k+2) - lambda where tok_opt[k+1]);
 * start and end states are wfl_align_optional's (where tok_opt[N-1]: also G_{N-1}, I_{N-2}, B_{N-2}, each at -lambda).  Windows mask EB
 * wherever it is gathered; a skipped token's window is never consulted.
 * Outputs (device, float32; the per-token ones rows as tok_cls):
 *   keep_post[k]   sum_t gamma_t(B_k), clamped to [0, 1].  Every labelling is exactly one path and a path enters B_k at most once, so
 *                  this is the posterior probability that token k is present (on wfl_align_posterior's lattice: the constant 1);
 *   tok_post[k]    as wfl_align_posterior's, the occupancy of the run Viterbi gave the token; 0 for a token tok does not hold;
 *   start_mean[k], start_sd[k]   moments of gamma_.(B_k) divided by their sum, i.e. conditional on the token being kept: relative to
 *                  Viterbi's start for a token tok holds, to frame 0 for one it does not; zeros where the sum is 0;
 *   logz[b]        log of the summed weight of every path of the skip lattice, wfl_align_posterior's convention.
 * status[b]: wfl_align_posterior's codes; 1 "no path": too few frames (wfl_align_optional's rule) or windows that cannot be met
 * (logZ = -inf, never a NaN); 4 also for a flag other than 0 | 1; 8 tok is not a path of this lattice: a value outside -1 .. N - 1, a
 * missing token that is not optional, two adjacent tokens both missing, a kept token that opens outside its window.  1 comes before 8:
 * a clip without any path is status 1 whatever tok holds (wfl_align_optional writes tok = -1 for it).  A clip with status != 0 gets zeros.  Host-side negative returns as wfl_align_optional's (a null tok_opt, a negative, infinite or NaN
 * skip_penalty), and a null keep_post with any token present.
 * Workspace: wfl_align_posterior's layout and figure (a clip with 0 < T < N, which may have a path here, has its floats there too).
 * With every flag 0 the outputs are wfl_align_posterior's (wfl_align_posterior_windowed's) up to rounding and keep_post is 1. */
int64_t wfl_align_optional_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_optional_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                     const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                     const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                     const int32_t* tok_opt, float skip_penalty, const int32_t* tok, void* workspace,
                                     int64_t workspace_bytes, float* logz, float* keep_post, float* tok_post, float* start_mean,
                                     float* start_sd, int32_t* status, void* stream);

/* ---- wfl_align_posterior over the filler lattice of wfl_align_filler (`postprocess.filler_scores`; wfl-asr_amd/align.py
 * filler_posteriors).  wfl_align_posterior_windowed's arguments (tok_win may be null: no windows) plus tok_fill and filler_penalty =
 * phi, the table and the penalty the search was given; tok is wfl_align_filler's output.  States, arcs, start and end states and the
 * recurrences are wfl_align_posterior's, emissions normalised per frame (z - lse) as there; the one difference is that a flagged token
 * emits
 *     EB_t(k) = EI_t(k) = (max_c z_t[c] - lse_t) - phi,     the maximum over all C classes, as in the search;
 * windows mask EB of a filler like any token's.  A path weighs exp(sum_t e_t): every frame of a filler carries -phi.
 * Outputs (device, float32; the per-token ones rows as tok_cls):
 *   logz[b], tok_post[k], start_mean[k], start_sd[k]   as wfl_align_posterior_windowed defines them; for a filler tok_post is the mean
 *                  over Viterbi's run of gamma_t(B_k) + gamma_t(I_k), the posterior that those frames belong to the filler;
 *   end_mean[k], end_sd[k]   for EVERY token: with last[k] the last frame tok gives token k and
 *                      omega_t(k) = exp(lse(alpha_t(B_k), alpha_t(I_k)) + leave_k(t+1) - logZ),
 *                      leave_k(t+1) = lse(beta_{t+1}(G_{k+1}) + EG_{t+1}, beta_{t+1}(B_{k+1}) + EB_{t+1}(k+1))   for t < T - 1
 *                                     (the B term absent for k = N - 1; EB masked by the window),
 *                                   = 0 for k = N - 1 and -inf for k < N - 1 at t = T - 1,
 *                  the posterior that token k's run ends on frame t: mean and standard deviation of t - last[k] under omega_.(k) divided
 *                  by its own sum, accumulated in double; zeros where the sum is 0.  omega is summed from alpha and leave directly (no
 *                  difference of gammas), and leave crosses the boundaries of the checkpointed sweep with beta.
 * status[b]: wfl_align_posterior_windowed's codes: 2 over the cap; 1 T < N, or windows no path meets (logZ = -inf, never a NaN); 4 a bad
 * class, and also a flag other than 0 | 1; 8 tok is not a path of this lattice.  1 comes before 8: a clip without any path is status 1
 * whatever tok holds (wfl_align_filler writes tok = -1 for it).  A clip with status != 0 gets zeros in all seven outputs.
 * Host-side negative returns as wfl_align_posterior_windowed's, and: a null tok_fill, end_mean or end_sd with any token present; a
 * negative, infinite or NaN filler_penalty; a workspace that is too small.
 * The row maximum is taken once per frame, in the pass that takes the log-sum-exp, and kept in the workspace: inside the frame loops a
 * thread reads one value per frame and never scans a logits row.  A clip without a flag skips all of it.
 * Workspace: wfl_align_posterior's and the filler emission of every frame behind it: per clip, in 4-byte words (0 for T = 0),
 *     round_up_64(T) + round_up_64(2 nblk) + 3 (nblk + 128) * slots(N) + round_up_64(T),   nblk = ceil(T / 128);
 * the end moments' sums live in registers.  With every flag 0, logz, tok_post, start_mean and start_sd are wfl_align_posterior's
 * (wfl_align_posterior_windowed's) up to rounding, for any phi. */
int64_t wfl_align_filler_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_filler_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                   const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                   const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                   const int32_t* tok_fill, float filler_penalty, const int32_t* tok, void* workspace,
                                   int64_t workspace_bytes, float* logz, float* tok_post, float* start_mean, float* start_sd,
                                   float* end_mean, float* end_sd, int32_t* status, void* stream);

/* ---- Posteriors over the explicit-duration lattice of wfl_align_duration_prior (`postprocess.duration_prior_scores`;
 * wfl-asr_amd/align.py duration_prior_posteriors, csrc/align_duration_prior_posterior.hip).  The arguments up to D are
 * wfl_align_duration_prior's, under the same table contract (every entry finite or -inf, never NaN; tail <= 0 or -inf; 1 <= D <= 32);
 * tok is that search's output for the same clips.  Emissions EB / EI / EG are wfl_align_posterior's (z_t - lse_t, EB through the window
 * where tok_win is given), L_k(d) and tail_k the search's, and a path weighs exp(sum_t e_t + sum_k L_k(d_k)).  Forward, the search's
 * recurrence with log-sum-exp for max:
 *     ent_k(t)  = lse(aG_k(t-1), aX_{k-1}(t-1))                ent_0(0) = 0, every other ent_k(0) = -inf
 *     aG_k(t)   = ent_k(t) + EG_t
 *     aR_k^1(t) = ent_k(t) + EB_t(k);    aR_k^j(t) = aR_k^{j-1}(t-1) + EI_t(k)     2 <= j <= D
 *     aY_k(t)   = lse(aY_k(t-1), aR_k^D(t-1) + L_k(D)) + EI_t(k) + tail_k
 *     aX_k(t)   = lse(aR_k^1(t) + L_k(1), .., aR_k^D(t) + L_k(D), aY_k(t))          frame t is the last frame of token k
 *     logZ      = lse(aG_N(T-1), aX_{N-1}(T-1))
 * Backward: bE_k(t) stands for beta(G_k) and beta(X_{k-1}) (the same successors); W_k^j(t) is the suffix weight when frame t is the
 * j-th frame of a run of token k, V_k(t) when the run is already longer than D:
 *     bE_N(T-1) = 0, every other bE_k(T-1) = -inf;   the terms "at t+1" are absent at t = T - 1
 *     V_k(t)    = lse(bE_{k+1}(t), EI_{t+1}(k) + tail_k + V_k(t+1))
 *     W_k^j(t)  = lse(L_k(j) + bE_{k+1}(t), EI_{t+1}(k) + W_k^{j+1}(t+1))   1 <= j < D;      W_k^D(t) = L_k(D) + V_k(t)
 *     bE_k(t-1) = lse(bE_k(t) + EG_t, EB_t(k) + W_k^1(t))                    (second term absent for k = N)
 *     start_k(t) = exp(ent_k(t) + EB_t(k) + W_k^1(t) - logZ),     end_k(t) = exp(aX_k(t) + bE_{k+1}(t) - logZ)
 *     occ_k(t)   = sum_{s <= t} start_k(s) - sum_{e < t} end_k(e)            the posterior that frame t belongs to token k
 * Outputs (device, float32; the per-token ones rows as tok_cls), with [first_k, last_k] the frames tok gives token k:
 *   logz[b]        logZ; the fp32 rounding residue of the frames' log-sum-exp is given back in double, as in wfl_align_posterior;
 *   tok_post[k]    the mean of occ_k(t) over first_k .. last_k, clamped to [0, 1]; accumulated in double by the thread that owns the
 *                  token as  sum_s start_k(s) #{t in run: t >= s} - sum_e end_k(e) #{t in run: t > e};
 *   start_mean[k], start_sd[k]   moments of t - first_k under start_k(.) divided by its own sum (wfl_align_posterior's definition);
 *   end_mean[k], end_sd[k]       moments of t - last_k under end_k(.) divided by its own sum (wfl_align_filler_posterior's); zeros where
 *                  the sum is 0.
 * status[b]: wfl_align_posterior_windowed's codes: 2 N above 4096; 1 T < N, or table and windows leave no path (logZ = -inf; never a
 * NaN in any output); 4 a bad class, or a tok_dur outside -1 .. n_rows - 1; 8 tok is not a path of this lattice: a value outside
 * -1 .. N - 1, a token missing, twice or out of order, a token opening outside its window, a run whose length d has L_k(d) = -inf.
 * 1 comes before 8.  A clip with status != 0 gets zeros in all six float outputs and does not disturb its batch; one workgroup per
 * clip, a clip scored alone equals the same clip inside any batch, bit for bit.
 * Host-side negative returns: wfl_align_duration_prior's, and a null tok while any frame is present, a null per-token output while any
 * token is present, a workspace that is too small.  Nothing is launched after a refusal.
 * Workspace.  Alpha is never stored per frame: a checkpoint of G, X, Y and the D ring entries of every slot every 128 frames, and one
 * block of 128 frames of (aR^1, aX), the two values of alpha that meet beta.  The two rings (alpha's aR^1 .. aR^D, beta's W^1 .. W^D;
 * D floats per slot each) live in the workgroup's LDS where they fit beside its other areas, alpha's first, and in the workspace where
 * they do not.  With eight or nine slots per thread (N > 1023) the seven double sums of every slot and the two ends of its run are kept
 * in the workspace as well, not in registers.  Per clip, in 4-byte words (0 for T = 0), with nblk = ceil(T / 128):
 *     round_up_64(T) + round_up_64(2 nblk) + nblk (3 + D) slots(N) + 256 slots(N) + sums(N)
 *         + (2 - lds_rings(N, D)) round_up_64(slots(N) D),
 *     slots(N) = 128 (N <= 127), 512 (N <= 511), 1024 (N <= 1023), 2048 (N <= 2047), 4608 (above);   sums(N) = 16 slots(N) for
 *     N > 1023, else 0;   lds_rings(N, D) = min(2, floor(room(N) / (4 slots(N) D))),   room(N) = 148992, 112128, 99840, 75264, 9728
 *     bytes in that order
 * (so N <= 127 keeps both rings in LDS at every D; N <= 511 both up to D = 27, one above; N <= 1023 both up to D = 12, one up to
 * D = 24, none above; N <= 2047 both up to D = 4, one up to D = 9, none above; above that none at any D). */
int64_t wfl_align_duration_prior_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips,
                                                           int32_t D);
int32_t wfl_align_duration_prior_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                           const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                           const int32_t* tok_dur, const float* dur, int32_t n_rows, int32_t D, const int32_t* tok,
                                           void* workspace, int64_t workspace_bytes, float* logz, float* tok_post, float* start_mean,
                                           float* start_sd, float* end_mean, float* end_sd, int32_t* status, void* stream);

/* ---- Expected run-length counts over the same explicit-duration lattice: the E-step of a duration prior's re-estimation from audio and
 * transcripts alone (wfl-asr_amd/align.py duration_prior_expected_counts, `python -m wfl_asr_amd.adapt_durations`; the counts
 * instantiations of csrc/align_duration_prior_posterior.hip).  The arguments are wfl_align_duration_prior_posterior's without tok: the
 * sums run over all paths, no search is needed.  With d_k the length of token k's run under the path posterior, outputs (device, float32):
 *   logz[b]          as wfl_align_duration_prior_posterior's;
 *   dur_post[k][j]   (rows as tok_cls, D + 1 columns: the layout of a table row)
 *                      j = 0 .. D - 2   P(d_k = j + 1)
 *                      j = D - 1        P(d_k >= D)
 *                      j = D            E[max(d_k - D, 0)]
 *                    the statistics wfl-asr_amd/durations.py estimate() counts in .lab files (c[d], c_ge, excess).
 * The posterior that token k opens at frame t and lasts exactly d < D frames is
 *     p_k(t, d) = exp(aR_k^1(t) + L_k(d) + Q_k^{t+d-1}(t) - logZ)
 *     Q_k^e(t)  = EI_{t+1}(k) + .. + EI_e(k) + bE_{k+1}(e),    Q_k^t(t) = bE_{k+1}(t),    Q_k^e(t-1) = EI_t(k) + Q_k^e(t)
 * (a third ring of D - 1 floats per slot carried by the backward sweep beside W, renormalised with it and part of beta's maximum), and
 *     P(d_k = d)         = sum_t p_k(t, d)                                     d < D, only where start_k(t) != 0 in fp32: p <= start
 *     P(d_k >= D)        = sum_t exp(aR_k^D(t) + L_k(D) + V_k(t) - logZ)       frame t the D-th frame of the run: once per such run
 *     E[max(d_k - D, 0)] = sum_t exp(aY_k(t) + V_k(t) - logZ)                  frame t in the tail: once per frame past the D-th
 * each a sum of non-negative terms in double by the thread that owns the token; nothing is formed as a difference.  An entry the table
 * forbids (L = -inf) is exactly 0.0; at D = 1 there is no ring and column 0 is P(d >= 1).  A token with tok_dur -1 is computed like any
 * other, with L = 0 and tail 0.
 * status[b]: wfl_align_duration_prior_posterior's codes without 8.  A clip with status != 0 gets zeros in logz and in its dur_post rows
 * and does not disturb its batch; a clip alone equals the same clip inside any batch, bit for bit.  Host-side negative returns:
 * wfl_align_duration_prior's, a null dur_post while any token is present, a workspace that is too small.
 * Workspace, per clip in 4-byte words (0 for T = 0), in the notation of wfl_align_duration_prior_posterior_workspace_bytes:
 *     round_up_64(T) + round_up_64(2 nblk) + nblk (3 + D) slots(N) + 384 slots(N) + 2 (D + 1) slots(N)
 *         + (2 - min(2, r)) round_up_64(slots(N) D) + (r < 3 ? round_up_64(slots(N) (D - 1)) : 0)
 * (the block holds aR^1, aY and aR^D, three floats per slot and frame; the D + 1 double sums of a slot are always in the workspace),
 * r = count_rings(N, D) how many of alpha's ring, W and Q, in that order, fit room(N): 3 where slots(N) (3 D - 1) words fit, else 2 where
 * 2 slots(N) D fit, else 1 where slots(N) D fit, else 0 -- N <= 127: 3 at every D; N <= 511: 3 up to D = 18, 2 up to 27, 1 above;
 * N <= 1023: 3 up to D = 8, 2 up to 12, 1 up to 24, 0 above; N <= 2047: 3 up to D = 3, 2 at D = 4, 1 up to 9, 0 above; above that 0. */
int64_t wfl_align_duration_prior_counts_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips,
                                                        int32_t D);
int32_t wfl_align_duration_prior_counts(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                        const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                        const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                        const int32_t* tok_dur, const float* dur, int32_t n_rows, int32_t D, void* workspace,
                                        int64_t workspace_bytes, float* logz, float* dur_post, int32_t* status, void* stream);

/* ---- Single-edit scores of an aligned transcript (`postprocess.align_edits`; wfl-asr_amd/align.py, csrc/align_edits.hip).  No
 * counterpart in the reference.  The arguments are wfl_align_posterior_windowed's without tok; tok_win may be null: the unwindowed
 * lattice.  sub_cls (device, [n_sub][2] int32 = (B class, I class)) is a table of P = n_sub substitutes, 0 <= P <= 512.  With logZ(.)
 * what wfl_align_posterior / wfl_align_posterior_windowed return for a transcript, outputs (device):
 *   logz[b]          logZ of the clip's transcript as written (wfl_align_posterior's logz);
 *   edits[k][p]      (rows tok_off_host[b] + k, P + 1 fp32 columns) for p < P: logZ(the transcript whose token k has the single alternative
 *                    sub_cls[p]; everything else, k's window included, unchanged) - logZ(transcript);
 *   edits[k][P]      logZ(the transcript without token k and without its window) - logZ(transcript).
 *                    A log likelihood ratio: positive when the edited transcript explains the audio better; -inf when the edited
 *                    transcript has no path (windows).  If token k has exactly one alternative and it is row p, edits[k][p] is 0 up to
 *                    rounding;
 *   status[b]        wfl_align_posterior's codes without 8: 0 ok, 1 infeasible (T < N, or no path satisfies the windows), 2 N above
 *                    4096, 4 a class id out of range or no gap class -- and 4 for EVERY clip when a class id of sub_cls is out of range.
 *                    A clip with status != 0 gets logz = 0 and zeros in its edits rows.
 * The sums run over all boundaries, not Viterbi's: one forward and one backward sweep of the clip (one workgroup per clip, fp32 log
 * domain renormalised every 16 frames, per-frame offsets in double) leave, per frame and token, the mass that may enter the token, the
 * mass that follows it and the next token's entry; then one wave per (token, 64 substitutes) runs the N P chains of T steps.  Clips are
 * independent: a clip scored alone equals the same clip inside any batch, bit for bit.
 * Workspace per clip, in 4-byte words (every part rounded up to 64; 0 for T = 0), W = round_up_64(min(N, 4096)):
 *     64 + T + 2 (T + 1) + 2 T + (T + 1) W + 2 T W
 * about 3 N T floats: 5.3 MB for 1500 frames and 300 tokens, 740 MB at T = 15000, N = 4096.  wfl_align_edits_workspace_bytes returns the
 * sum in bytes.  Arguments are checked on the host as wfl_align checks its own (negative return). */
int64_t wfl_align_edits_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_edits(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                        const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                        const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* sub_cls, int32_t n_sub,
                        void* workspace, int64_t workspace_bytes, float* logz, float* edits, int32_t* status, void* stream);

/* ---- Single-insertion scores of an aligned transcript (`postprocess.align_insertions`; wfl-asr_amd/align.py, csrc/align_edits.hip):
 * the third single edit beside wfl_align_edits' substitution and deletion.  No counterpart in the reference.  The arguments are
 * wfl_align_edits' (tok_win may be null; sub_cls holds P = n_sub substitutes, 0 <= P <= 512).  A clip of N tokens has N + 1 places:
 * place j lies in front of token j, place N behind the last token; N = 0 is a legal clip with one place.  Outputs (device):
 *   logz[b]          wfl_align_posterior's (wfl_align_posterior_windowed's) logz of the transcript as written, as wfl_align_edits';
 *   ins[row][p]      (P fp32 columns) logZ(the transcript with a token whose single alternative is sub_cls[p] inserted at place j, the
 *                    new token without a window, every other token with its own) - logZ(transcript).  -inf when the longer transcript
 *                    has no path: every entry of a clip with T = N, and whatever the neighbours' windows leave no frame for;
 *   status[b]        wfl_align_edits' codes.  A clip with status != 0 gets logz = 0 and zeros in its rows.
 * Rows: clip b owns the N_b + 1 rows tok_off_host[b] + b + j, j = 0 .. N_b, of a buffer of (total tokens + n_clips) rows.  This rests
 * on the clips' token ranges lying in clip order (tok_off_host[b + 1] >= tok_off_host[b] + n_tok_host[b]), as pack_clips lays them out.
 * The sweeps are wfl_align_edits' (the same kernel, instantiated with planes one slot wider); then one wave per (place, 64
 * substitutes) runs the (N + 1) P chains.  Clips are independent, bit for bit.  N = 4096 is legal.
 * Workspace per clip, in 4-byte words (every part rounded up to 64; 0 for T = 0), W = round_up_64(min(N, 4096) + 1):
 *     64 + T + 2 (T + 1) + 2 T + (T + 1) W + T W
 * wfl_align_insertions_workspace_bytes returns the sum in bytes.  Arguments are checked on the host as wfl_align_edits checks its own;
 * ins may be null only when n_sub is 0. */
int64_t wfl_align_insertions_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips);
int32_t wfl_align_insertions(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                             const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                             const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* sub_cls, int32_t n_sub,
                             void* workspace, int64_t workspace_bytes, float* logz, float* ins, int32_t* status, void* stream);

/* ---- BIO-grammar Viterbi decode of clips WITHOUT a transcript on the GPU (`postprocess.decode: viterbi`; wfl-asr_amd/decode.py).
 * Stands beside the reference's free decode, infer.py:86-96, 164-174, 293-302 (per-frame argmax, confidence threshold, median filter
 * over the ids, then the BIO decoder), which knows nothing of the grammar it decodes.  Clip b has T = n_frames_host[b] logits rows (row
 * frame_off_host[b] + t, ld ldl, C fp32 columns).  pairs (device) holds n_pairs phonemes as (B class, I class or -1); o_id is the O
 * class; every other class is never chosen.  A legal path is a class per frame with every I-p directly preceded by B-p or I-p; B-* and
 * O may follow anything; the clip starts after a virtual O frame.  The path maximises
 *     sum_t z[t][c_t] - lambda * (runs opened),     a run is opened by every B-p frame and by every O frame whose predecessor is not O.
 * With d the previous frame's state scores, a = argmax d (the lowest class id wins a tie) and best = d[a]:
 *     O   : z + (d[O] >= best - lambda ? d[O] : best - lambda)      B-p : z + best - lambda
 *     I-p : z + (d[I-p] >= d[B-p] ? d[I-p] : d[B-p])                end state: the argmax of the last frame, lowest id on a tie.
 * threshold > 0: a frame whose largest softmax probability (fp32) is below it can only be O.  lambda >= 0 is in nats.
 * Outputs (device): ids[t] the path's class (same rows as the logits); score[b] the path's objective minus sum_t logsumexp z[t][.]
 * (fp32; the search decides on the raw logits); status[b]: 0 ok, 2 C above 1024, 4 a class id of `pairs` outside [0, C) or a class used
 * twice (o_id included).  A clip with status != 0 gets ids = o_id and score 0; T = 0 is ok and writes no ids.  One wave per clip: a clip
 * decoded alone equals the same clip inside any batch, bit for bit.  fp32 state scores, renormalised every 16 frames (offset in double).
 * Arguments are checked on the host (negative return): C >= 1, o_id in range, ldl >= C, counts and offsets >= 0, lambda and threshold
 * >= 0, non-null pointers, workspace large enough.
 * Workspace, per clip with T > 0, in 4-byte words: round_up_64(T (2 S + 1)) + 2 round_up_64(T)  (backpointers: 2 S words of I-p bits
 * and one word a | O's bit << 16 per frame; the frames' log-sum-exp; their forced flags), S = 2 (n_pairs <= 128), 4 (<= 256),
 * 8 (<= 512), 16 (<= 1024); 0 above.  wfl_decode_workspace_bytes returns the sum in bytes (28 bytes per frame at n_pairs <= 128). */
int64_t wfl_decode_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs);
int32_t wfl_decode(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                   int32_t n_clips, const int32_t* pairs, int32_t n_pairs, float lambda, float threshold, void* workspace,
                   int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status, void* stream);

/* ---- Posteriors of a BIO-grammar decode by forward-backward on the GPU (`postprocess.decode_scores`; wfl-asr_amd/decode.py).  No
 * counterpart in the reference, which reports no confidence for its free decode.  Classes, virtual start, forced frames, caps and
 * argument conventions are wfl_decode's: the states are O, B-p, I-p of `pairs` (every other class is never on a path), the clip follows
 * a virtual O frame, a frame whose largest softmax probability (fp32, the same pre-pass arithmetic) is below threshold > 0 can only be O,
 * any state may end the clip.  The weight of a legal path is exp(sum_t z[t][c_t] - lambda * runs opened), the runs counted as wfl_decode
 * counts them; as transitions:  into O from O: 0;  into O from anything else: -lambda;  into any B-q from anything: -lambda;  into I-p
 * from B-p or I-p only: 0.  Then
 *     logZ = log sum of the weights of all legal paths,      gamma_t(c) = posterior that the path is in class c at frame t.
 * ids (device) is the path wfl_decode returned for the same clips and rows.  Outputs (device, fp32):
 *   logz[b]       logZ of the clip;
 *   post[t]       (same rows as the logits) for ids[t] in {B-p, I-p}: gamma_t(B-p) + gamma_t(I-p), the posterior that frame t belongs to
 *                 phoneme p at all; for ids[t] == O: gamma_t(O).  In [0, 1], clamped to 1 from above;
 *   cls_post[t]   gamma_t(ids[t]), the posterior of the exact class: on the first frame of a run, that a run of p opens exactly here.
 *                 cls_post[t] <= post[t];
 *   status[b]     wfl_decode's codes (0 ok, 2 C above 1024, 4 a class id of `pairs` outside [0, C) or a class used twice), and 8: ids
 *                 holds a class that is never chosen, an I-p that does not follow B-p / I-p, or a non-O class on a forced frame (not a
 *                 path of this grammar).  A clip with status != 0 gets logz = 0 and post = cls_post = 0; T = 0 is ok, logz 0, and
 *                 writes nothing per frame.
 * One wave per clip: a clip scored alone equals the same clip inside any batch, bit for bit.  Scaled linear-domain fp32 states
 * (emissions exp(z - row maximum), every frame rescaled by a power of two, the exponents summed in an integer); a posterior that
 * underflows fp32 is reported as 0.  An O emission counts as at least 2^-60 of its frame's largest (the row maximum over all C
 * classes) and lambda as at most 60 ln 2 (41.6 nats), which keeps every sum inside fp32's exponent range.  Neither moves a posterior by
 * more than 1e-18 while the frame's largest logit belongs to a class that carries mass there or O lies within 41.6 nats of it; on a
 * frame whose largest logit is a class outside the grammar, or an I-q no path can reach, more than 41.6 nats above O, O is lifted
 * against the B / I states and the frame's posterior leans towards O.  Arguments are checked on the host as wfl_decode checks its own
 * (negative return).
 * Workspace: the alpha lattice is not stored.  Per clip with T > 0, in 4-byte words: round_up_64(3 T) + 3 round_up_64(T)  (per frame
 * alpha on the path's own phoneme and the scale exponent; the path's (pair, kind); the row maximum; the forced flag), whatever n_pairs
 * <= 1024; 0 above.  wfl_decode_posterior_workspace_bytes returns the sum in bytes (24 bytes per frame). */
int64_t wfl_decode_posterior_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs);
int32_t wfl_decode_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                             const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, float lambda,
                             float threshold, const int32_t* ids, void* workspace, int64_t workspace_bytes, float* logz, float* post,
                             float* cls_post, int32_t* status, void* stream);

/* ---- BIO-grammar Viterbi decode with a phone-bigram prior on the GPU (`postprocess.phoneme_bigram`; wfl-asr_amd/decode.py,
 * wfl-asr_amd/phonotactics.py).  No counterpart in the reference.  Clips, logits, pairs, o_id, threshold, ids, score and the argument
 * checks are wfl_decode's; so are the states, the legality rule, the forced-to-O rule and the virtual O frame before frame 0.  Symbols:
 * 0 is O, 1 + p is phoneme p of `pairs`; N = n_pairs + 1.  trans (device) is an [N][N] fp32 table, rows the PREVIOUS symbol, entries
 * finite or -inf (a forbidden succession), never NaN or +inf, every trans[p][O] finite (so every clip has a path); trans[O][O] is never
 * read.  The path maximises
 *     sum_t z[t][c_t] + sum over opened runs trans[previous symbol][opened symbol],
 * a run being opened by every B-q frame and by every O frame whose predecessor is not O; the previous symbol of a frame in B-p or I-p is
 * p, of a frame in O it is O; O after O and I-q after B-q / I-q cost nothing.  With end[O] = d[O], end[p] = max(d[B-p], d[I-p]):
 *     B-q : z + max_s (end[s] + trans[s][q])     O : z + max(d[O], max_{p != O} (end[p] + trans[p][O]))     I-q : z + max(d[I-q], d[B-q])
 * The lowest predecessor symbol wins a tie; of a symbol's two states I-p wins a tie against B-p; the end state is the best symbol of the
 * last frame, the lowest on a tie.  With trans identically -lambda the objective is wfl_decode's.
 * status[b]: 0 ok; 2 C above 1024 or N above WFL_DECODE_BIGRAM_MAX_SYMBOLS (O + 191 phonemes: the table, 144 KiB of fp32 at the cap,
 * stays in one CU's LDS for the whole clip); 4 a bad class table, as wfl_decode.  A clip with status != 0 gets ids = o_id and score 0.
 * One workgroup per clip: a clip decoded alone equals the same clip inside any batch, bit for bit.  fp32 state scores, renormalised every
 * 16 frames (offset in double).
 * Workspace, per clip with T > 0, in 4-byte words: round_up_64(T ceil(N / 2)) + 2 round_up_64(T)  (per frame and symbol 16 bits: the
 * winning predecessor symbol | the I bit << 8 | O's bit << 9; the frames' log-sum-exp; their forced flags); 0 above the symbol cap. */
#define WFL_DECODE_BIGRAM_MAX_SYMBOLS 192
int64_t wfl_decode_bigram_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs);
int32_t wfl_decode_bigram(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                          const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, const float* trans,
                          float threshold, void* workspace, int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status,
                          void* stream);

/* ---- Posteriors of a phone-bigram decode by forward-backward on the GPU (`postprocess.bigram_scores`; wfl-asr_amd/decode.py).  The
 * sum-product counterpart of wfl_decode_bigram, as wfl_decode_posterior is wfl_decode's.  Clips, logits, pairs, o_id, threshold, trans,
 * the symbols (0 is O, 1 + p is phoneme p; N = n_pairs + 1), the states, the legality rule, the forced-to-O rule and the virtual O frame
 * are wfl_decode_bigram's; ids, logz, post, cls_post and what they mean are wfl_decode_posterior's.  The weight of a legal path is
 *     exp(sum_t z[t][c_t] + sum over opened runs trans[previous symbol][opened symbol]),
 * the runs counted as wfl_decode_bigram counts them; any state may end the clip.  With W = exp(trans) (-inf -> 0), e a frame's emissions,
 * end[O] = alpha(O), end[p] = alpha(B-p) + alpha(I-p) of the previous frame, and primes for the next frame:
 *     forward    B-q' = e(B-q) sum_s end[s] W[s][q]     O' = e(O) (alpha(O) + sum_{p != O} end[p] W[p][O])     I-q' = e(I-q) (alpha(B-q) + alpha(I-q))
 *     backward   u[O] = e'(O) beta'(O),  u[q] = e'(B-q) beta'(B-q);     beta(O) = u[O] + sum_{q >= 1} W[O][q] u[q];
 *                beta(B-p) = beta(I-p) = sum_{q >= 0} W[p][q] u[q] + e'(I-p) beta'(I-p);     beta at T - 1 = 1.
 * With trans identically -lambda every output equals wfl_decode_posterior's at that lambda.
 * status[b]: 0 ok; 2 C above 1024 or N above WFL_DECODE_BIGRAM_MAX_SYMBOLS; 4 a bad class table, as wfl_decode; 8 ids is not a path of
 * this grammar: a class that is never chosen, an I-p that does not follow B-p / I-p, a non-O class on a forced frame, or a run opened
 * through a succession whose trans entry is -inf (wfl_decode_bigram never returns such a path).  A clip with status != 0 gets logz = 0
 * and post = cls_post = 0; T = 0 is ok, logz 0, and writes nothing per frame.
 * One workgroup per clip: a clip scored alone equals the same clip inside any batch, bit for bit.  The table stays in one CU's LDS for
 * the whole clip as linear weights.  Scaled linear-domain fp32 states (emissions exp(z - row maximum), every frame rescaled by a power
 * of two taken from the previous frame's largest state, the exponents summed in an integer); a posterior that underflows fp32 is
 * reported as 0.  Guards: an O emission counts as at least 2^-60 of its frame's largest (the row maximum over all C classes), as for
 * wfl_decode_posterior, with the same consequence on a frame whose largest logit lies outside the grammar more than 41.6 nats above
 * O; a finite trans entry is clamped to +-60 ln 2 (+-41.6 nats), -inf is exactly weight 0.  Together they keep every sum inside fp32's
 * exponent range whatever the logits, the table and the clip's length.
 * Arguments are checked on the host as wfl_decode_bigram checks its own (negative return); trans may be null only when no clip is scored.
 * Workspace: wfl_decode_posterior's.  Per clip with T > 0, in 4-byte words: round_up_64(3 T) + 3 round_up_64(T)  (per frame alpha on
 * the path's own phoneme and the scale exponent; the path's (pair, kind); the row maximum; the forced flag); 0 above the symbol cap.
 * wfl_decode_bigram_posterior_workspace_bytes returns the sum in bytes (24 bytes per frame). */
int64_t wfl_decode_bigram_posterior_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs);
int32_t wfl_decode_bigram_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                    const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs,
                                    const float* trans, float threshold, const int32_t* ids, void* workspace, int64_t workspace_bytes,
                                    float* logz, float* post, float* cls_post, int32_t* status, void* stream);

/* ---- Expected successions of a phone-bigram decode on the GPU: one Baum-Welch E-step over the grammar of wfl_decode_bigram, to adapt
 * the bigram to audio without labels (`python -m wfl_asr_amd.adapt_bigram`; wfl-asr_amd/decode.py).  Clips, logits, pairs, o_id,
 * threshold, trans, the symbols, the states, the legality rule, the forced-to-O rule, the virtual O frame, the path weights, W, the
 * recurrences, the guards and logz are wfl_decode_bigram_posterior's; there is no path argument.  With end_{-1} = (1, 0, ...),
 * u_t[O] = e_t(O) beta_t(O), u_t[q] = e_t(B-q) beta_t(B-q):
 *     counts[b][s][q] = (1 / Z) sum_{t = 0 .. T-1} end_{t-1}[s] W[s][q] u_t[q]     for (s, q) != (O, O);     counts[b][O][O] = 0
 * the expected number of runs of symbol q opened directly after symbol s under the path distribution wfl_decode_bigram maximises over,
 * the runs counted as the search counts them.  counts (device, fp32) holds one [N][N] table per clip, rows the PREVIOUS symbol; every
 * entry is >= 0, an entry whose trans is -inf is exactly 0, column q >= 1 sums to sum_t gamma_t(B-q).
 * status[b]: 0 ok; 2 C above 1024 or N above WFL_DECODE_BIGRAM_MAX_SYMBOLS; 4 a bad class table.  A clip with status != 0 gets logz = 0
 * and an all-zero table; so does T = 0, with status 0.  logz, counts and status must not be null when n_clips > 0.
 * One workgroup per clip: a clip alone equals the same clip inside any batch, bit for bit.  The sums are kept in registers for the
 * whole clip, in fp32 (a frame adds at most 1 to the table).  A frame's share is end W u times the constant 2^(exponents) / Z: that
 * constant is formed in double, clamped to 2^126 and applied to end first, so no intermediate is inf or NaN whatever the logits and the
 * table; the clamp acts only where every product of the frame has left fp32's normal range, which reports as 0 as a posterior does.
 * Workspace, per clip with T > 0, in 4-byte words: round_up_64(T (N + 1)) + 2 round_up_64(T)  (per frame the scaled vector end_{t-1} and
 * its exponent; the row maximum; the forced flag): 4 (N + 3) bytes per frame, 11.7 MB for 15 000 frames at the cap; 0 above the cap. */
int64_t wfl_decode_bigram_counts_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs);
int32_t wfl_decode_bigram_counts(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                 const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, const float* trans,
                                 float threshold, void* workspace, int64_t workspace_bytes, float* logz, float* counts, int32_t* status,
                                 void* stream);

/* ---- BIO-grammar Viterbi decode with a phone-bigram prior AND a duration prior per phoneme on the GPU: the free decode as an
 * explicit-duration (semi-Markov) search (`postprocess.decode_duration_prior`; wfl-asr_amd/decode.py, wfl-asr_amd/durations.py).  No
 * counterpart in the reference.  Clips, logits, pairs, o_id, trans, threshold, ids, score, the symbols (0 is O, 1 + p is phoneme p;
 * N = n_pairs + 1), the states, the legality rule, the forced-to-O rule, the virtual O frame before frame 0 and "any state may end the
 * clip" are wfl_decode_bigram's.  sym_dur (device), [n_pairs] int32: the row of `dur` of phoneme p, -1 for no prior.  dur (device) is
 * wfl_align_duration_prior's table, [n_rows][D + 1] fp32, 1 <= D <= 32: columns L(1) .. L(D), then the per-frame `tail`; entries finite
 * or -inf, never NaN or +inf; tail <= 0 or -inf.  A run of phoneme q is one B-q frame and then zero or more I-q frames (exactly one frame
 * for a phoneme without an I class); B-q after B-q / I-q opens a new run of q.  The path maximises
 *     sum_t z[t][c_t] + sum over opened runs trans[previous symbol][opened symbol] + sum over phoneme runs L_q(d),
 *     L_q(d) = dur[r][d - 1] for d <= D,  dur[r][D - 1] + (d - D) dur[r][D] for d > D,  r = sym_dur[q - 1];  L = 0 for r = -1.
 * O runs carry no prior; the run in progress at the clip's last frame ends there and pays its L.  Frame by frame, everything of frame
 * t - 1 on the right, for phoneme q (zB, zI its B and I logits; -inf on a forced frame, zI -inf without an I class):
 *     In_q(t)  = max_s (end_s(t-1) + trans[s][q])                                the lowest s on a tie
 *     R_q^1(t) = In_q(t) + zB_t(q)
 *     R_q^j(t) = R_q^{j-1}(t-1) + zI_t(q)             2 <= j <= D
 *     Y_q(t)   = max(Y_q(t-1), R_q^D(t-1) + L_q(D)) + zI_t(q) + tail_q           Y first on a tie
 *     end_q(t) = max(max_j R_q^j(t) + L_q(j), Y_q(t))                            the shortest j first, Y last on a tie
 *     O        : z + max(d[O], max_{p != O} (end_p(t-1) + trans[p][O]))          wfl_decode_bigram's line
 * -inf only ever adds: no expression forms inf - inf.  The end state is the best `end` of the last frame, the lowest symbol on a tie.
 * score[b] is the objective minus the frames' log-sum-exp.  With every sym_dur = -1, or an all-zero table, the objective is
 * wfl_decode_bigram's.
 * status[b]: 0 ok; 2 C above 1024 or N above WFL_DECODE_BIGRAM_MAX_SYMBOLS (whatever D); 4 a bad class table, as wfl_decode, or a sym_dur
 * outside -1 .. n_rows - 1.  All-O is always a path, so there is no status 1.  A clip with status != 0 gets ids = o_id and score 0.
 * Host-side errors (negative return) are wfl_decode_bigram's, and: a null sym_dur with n_pairs > 0 and frames present, a null dur with
 * n_rows > 0, n_rows < 0, D outside 1 .. 32, a workspace below wfl_decode_duration_workspace_bytes.
 * One workgroup per clip: a clip decoded alone equals the same clip inside any batch, bit for bit.  fp32 scores; every 16 frames the
 * largest end[] is taken off every state and every entry of the run history (offset in double), and a history entry is at most D
 * frames old, so nothing grows with the clip's length.
 * Workspace, per clip with T > 0, in 4-byte words: round_up_64(T ceil(N / 2)) + H + 2 round_up_64(T)  (per frame and symbol 16 bits:
 * the winning predecessor symbol | the winning duration 1 .. D, D + 1 for the tail, << 8 | the tail's stay / enter bit << 14 | O's bit
 * << 15; H; the frames' log-sum-exp; their forced flags).  H holds the run history and the symbols' rows of dur where one CU's LDS does
 * not hold them beside the trans table: with HS = round_up_64(N), H = 0 when
 *     16 ceil(max(4 N N, 128 ceil(N / 2)) / 16) + 8448 + 4 (2 D + 1) HS <= 163840 - 4416
 * (every D at N <= 141; at the cap of 192 symbols D = 1 only), else H = round_up_64((2 D + 1) HS).  0 above the symbol cap;
 * wfl_decode_duration_workspace_bytes returns -1 for D outside 1 .. 32. */
int64_t wfl_decode_duration_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs, int32_t D);
int32_t wfl_decode_duration(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                            const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, const float* trans,
                            const int32_t* sym_dur, const float* dur, int32_t n_rows, int32_t D, float threshold, void* workspace,
                            int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status, void* stream);

/* ---- Posteriors of a duration-prior decode by forward-backward on the GPU (`postprocess.decode_duration_scores`;
 * wfl-asr_amd/decode.py).  The sum-product counterpart of wfl_decode_duration, as wfl_decode_bigram_posterior is wfl_decode_bigram's: a
 * semi-Markov forward-backward over the BIO grammar.  Clips, logits, pairs, o_id, trans, sym_dur, dur, n_rows, D, threshold, the
 * symbols, the states, the legality rule, the forced-to-O rule, the virtual O frame, "any state may end the clip", L_q(d) with its
 * tail and "the run in progress at the last frame ends there and pays its L" are wfl_decode_duration's; ids (the path
 * wfl_decode_duration returned for the same clips), logz, post, cls_post and what they mean are wfl_decode_posterior's.  The weight of
 * a legal path is
 *     exp(sum_t z[t][c_t] + sum over opened runs trans[previous symbol][opened symbol] + sum over phoneme runs L_q(d)).
 * With W = exp(trans), W[O][O] = 1, lambda_q(j) = exp(L_q(j)), tau_q = exp(tail_q) (-inf -> exactly 0; all 1 for a phoneme without a
 * row), e a frame's emissions (e(B) = e(I) = 0 on a forced frame, e(I) = 0 without an I class), everything of frame t - 1 on the right
 * and end(-1) = (1, 0, ...):
 *     forward    In_q(t) = sum_s end_s(t-1) W[s][q];    R_q^1(t) = e_t(B-q) In_q(t);    R_q^j(t) = e_t(I-q) R_q^{j-1}(t-1)  2 <= j <= D
 *                Y_q(t) = e_t(I-q) tau_q (Y_q(t-1) + lambda_q(D) R_q^D(t-1));    end_q(t) = sum_j lambda_q(j) R_q^j(t) + Y_q(t)
 *                O(t) = e_t(O) sum_s end_s(t-1) W[s][O]   (end_O = O);    Z = sum_s end_s(T-1)
 *     backward   bE_q(t): the suffix weight after a run of q ends at t; Wr_q^j(t): when t is the j-th frame of a run; V_q(t): inside the
 *                tail.  At T - 1: bO = bE = V = 1, Wr^j = lambda(j).    u_t[O] = e_t(O) bO(t),  u_t[q] = e_t(B-q) Wr_q^1(t)
 *                (bO, bE_1 .. bE_P)(t-1) = W u_t;    V_q(t-1) = bE_q(t-1) + e_t(I-q) tau_q V_q(t)
 *                Wr_q^j(t-1) = lambda_q(j) bE_q(t-1) + e_t(I-q) Wr_q^{j+1}(t)  j < D;    Wr_q^D(t-1) = lambda_q(D) V_q(t-1)
 * logz[b] = log Z.  For ids[t] in {B-p, I-p}: post[t] = (sum_j R_p^j(t) Wr_p^j(t) + Y_p(t) V_p(t)) / Z, the posterior that frame t
 * belongs to phoneme p at all; for ids[t] = O: post[t] = O(t) bO(t) / Z.  cls_post[t] is the posterior of the exact class: on a B frame
 * R^1 Wr^1 / Z (a run opens exactly here), on an I frame the j >= 2 terms plus the tail term, on O post.  0 <= cls_post <= post <= 1.
 * With every sym_dur = -1, or an all-zero table, every output equals wfl_decode_bigram_posterior's.
 * status[b]: 0 ok; 2 C above 1024 or N above WFL_DECODE_BIGRAM_MAX_SYMBOLS (whatever D); 4 a bad class table, or a sym_dur outside
 * -1 .. n_rows - 1; 8 ids is not a path of this grammar: wfl_decode_bigram_posterior's cases, or a phoneme run of ids whose length has
 * L = -inf, the run the clip ends in included (wfl_decode_duration never returns such a path).  A clip with status != 0 gets logz = 0
 * and post = cls_post = 0; T = 0 is ok, logz 0, and writes nothing per frame.  Host-side errors (negative return) are
 * wfl_decode_duration's and wfl_decode_bigram_posterior's.
 * One workgroup per clip: a clip scored alone equals the same clip inside any batch, bit for bit.  Scaled linear-domain fp32 states,
 * every frame rescaled by a power of two taken from the largest value alive in the previous frame -- the states, the tail states and
 * every entry of the run history, not the states alone: under a hard minimum a history entry does not show in the states for D - 1
 * frames -- the exponents summed in integers; the posteriors are sums of non-negative products added in double.  Guards: an O emission
 * counts as at least 2^-60 of its frame's largest, finite entries of trans, and finite lambda and tau, are clamped to +-60 ln 2; no
 * intermediate is inf or NaN whatever the logits, the tables and the clip's length.  What is below 2^-122 of its frame's largest alive
 * value underflows and is reported as 0.
 * Workspace, per clip with T > 0, in 4-byte words: round_up_64(T (D + 2)) + round_up_64(T) + H + 2 round_up_64(T)  (per frame the run
 * history, the tail state and the scale exponent of the path's own symbol; the path's (pair, kind); H; the row maxima; the forced
 * flags).  H holds the run history and the symbols' rows of dur where one CU's LDS does not hold them beside the trans table: with
 * HS = round_up_64(N), H = 0 when
 *     16 ceil(4 N (N | 1) / 16) + 6912 + 4 (2 D + 1) HS <= 163840 - 4608
 * (every D at N <= 159; at the cap of 192 symbols D <= 2), else H = round_up_64((2 D + 1) HS).  0 above the symbol cap;
 * wfl_decode_duration_posterior_workspace_bytes returns -1 for D outside 1 .. 32. */
int64_t wfl_decode_duration_posterior_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs, int32_t D);
int32_t wfl_decode_duration_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                      const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs,
                                      const float* trans, const int32_t* sym_dur, const float* dur, int32_t n_rows, int32_t D,
                                      float threshold, const int32_t* ids, void* workspace, int64_t workspace_bytes, float* logz,
                                      float* post, float* cls_post, int32_t* status, void* stream);

/* ---- Expected run lengths and successions of a duration-prior decode on the GPU: one E-step over the explicit-duration grammar of
 * wfl_decode_duration, to learn the free decode's duration prior (and its bigram) from audio without labels
 * (`python -m wfl_asr_amd.adapt_decode_durations`; wfl-asr_amd/decode.py).  Clips, logits, pairs, o_id, trans, sym_dur, dur, n_rows, D,
 * threshold, the symbols, the states, the legality rule, the forced-to-O rule, the virtual O frame, "any state may end the clip",
 * L_q(d) with its tail, "the run in progress at the last frame ends there and pays its L", the path weight, W, lambda, tau, the
 * recurrences (R, Y, end, bE, bO, Wr, V, u), the guards and clamps and logz are wfl_decode_duration_posterior's; there is no path
 * argument: the sums run over every legal path.  Outputs (device, fp32):
 *     succ[b][s][q] = (1 / Z) sum_t end_s(t-1) W[s][q] u_t[q]    (s, q) != (O, O);  succ[b][O][O] = 0
 * one [N][N] table per clip, rows the PREVIOUS symbol: wfl_decode_bigram_counts' table on this grammar; an entry whose trans is -inf is
 * exactly 0.  dur_counts[b][p][j], [n_pairs][D + 1] per clip, indexed by phoneme SYMBOL p (not by table row; the host adds symbols
 * that share a row), in the layout of a row of dur:
 *     j = 0 .. D - 2   (1 / Z) sum_t R_p^{j+1}(t) lambda_p(j+1) bE_p(t)    expected runs of p of exactly j + 1 frames (t: the last frame)
 *     j = D - 1        (1 / Z) sum_t R_p^D(t) lambda_p(D) V_p(t)            expected runs of D frames or more (t: the D-th frame)
 *     j = D            (1 / Z) sum_t Y_p(t) V_p(t)                          expected frames past the D-th
 * At the last frame bE = V = 1: a run the clip cuts off counts with its cut length, as the search charges it.  Every entry is a sum of
 * non-negative products (nothing is formed as a difference); an entry the table forbids (lambda = 0; tau = 0 for j = D) is exactly 0.0; a
 * phoneme without a row (sym_dur = -1) is counted like any other, lambda = tau = 1.  At D = 1 column 0 is the number of runs.
 * Identities, by construction: sum_{j <= D-1} dur_counts[p][j] = sum_s succ[s][1 + p] (every run is opened once);
 * sum_{j <= D-2} (j + 1) dc[p][j] + D dc[p][D-1] + dc[p][D] is the posterior number of frames of p, and those summed over p are <= T;
 * with every sym_dur = -1, or an all-zero table, succ and logz are wfl_decode_bigram_counts'; dur_counts[p][.] and succ are the partial
 * derivatives of log Z with respect to p's row of dur and to trans, which is why they are the E-step.
 * status[b]: 0 ok; 2 C above 1024 or N above WFL_DECODE_BIGRAM_MAX_SYMBOLS (whatever D); 4 a bad class table, or a sym_dur outside
 * -1 .. n_rows - 1.  A clip with status != 0 gets logz = 0 and all-zero tables; so does T = 0, with status 0.  Host-side errors
 * (negative return) are wfl_decode_duration_posterior's, and a null logz, succ, status or (n_pairs > 0) dur_counts when n_clips > 0.
 * One workgroup per clip: a clip alone equals the same clip inside any batch, bit for bit.  Three sweeps: forward and backward as in
 * wfl_decode_duration_posterior (succ is summed in the backward sweep, in registers, fp32, a frame adds at most 1), then the owner
 * thread of each phoneme walks forward again over its recorded R^1, bE and V and adds the run-length shares, in double.  A frame's
 * share is multiplied by 2^(exponents) / Z formed in double and clamped to 2^126; no intermediate is inf or NaN whatever the logits,
 * the tables and the clip's length.
 * Workspace, per clip with T > 0, in 4-byte words: round_up_64(T (4 N + 2)) + H + 2 round_up_64(T)  (per frame the scaled end(t-1),
 * R^1(t), bE(t), V(t) of every symbol and the two scale exponents; H; the row maxima; the forced flags).  H holds the run history,
 * the symbols' rows of dur and the (D + 1) double sums per symbol where one CU's LDS does not hold them beside the trans table: with
 * HS = round_up_64(N), H = 0 when
 *     16 ceil(4 N (N | 1) / 16) + 6912 + 4 (4 D + 3) HS <= 163840 - 4608
 * (every D at N <= 128; at N = 141 D <= 22; never at the cap of 192 symbols), else H = round_up_64((4 D + 3) HS).  0 above the symbol cap;
 * wfl_decode_duration_counts_workspace_bytes returns -1 for D outside 1 .. 32. */
int64_t wfl_decode_duration_counts_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs, int32_t D);
int32_t wfl_decode_duration_counts(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                   const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs,
                                   const float* trans, const int32_t* sym_dur, const float* dur, int32_t n_rows, int32_t D,
                                   float threshold, void* workspace, int64_t workspace_bytes, float* logz, float* succ,
                                   float* dur_counts, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
