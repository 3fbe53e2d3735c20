// Model handle, weight packing and the forward schedule behind the C ABI of include/wfl_asr.h.
//
// This file is the native replacement for BIOPhonemeTagger (/root/reference/model.py:54-201): it owns the packed
// bf16 weights in HBM, lays the caller's workspace out as frame-row buffers (common.h) and enqueues the kernel
// sequence of one batched forward on the caller's HIP stream.  No torch types, no allocation and no
// synchronisation inside wfl_forward (graph-capturable).
#include "common.h"
#include "../../include/wfl_asr.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

// ---- launchers defined in the kernel translation units
int wfl_launch_logmel(const LogmelArgs& a, bf16_t* out, long ldo, long lead, int P, float* ref_out, hipStream_t s, bf16_t* out_lo = nullptr);
int wfl_launch_precise_finish(const PreciseFinishArgs& a, hipStream_t s);
int wfl_launch_melpower(const LogmelArgs& a, int hop, bf16_t* out, long ldo, long lead, int P, int split, int shift, hipStream_t s);

int wfl_launch_tag_decide(const TagArgs& a, hipStream_t s);
int wfl_launch_f32_to_rows(const float* in, bf16_t* x, long ldx, long lead, int B, int P, int T, int C, hipStream_t s, int split,
                           int shift, bf16_t* x_lo = nullptr);

int wfl_launch_lstm(LstmArgs a, void* exchange, hipStream_t s);

int wfl_launch_wav_stats(const float* wav, long ldw, int B, int L, double* stats, hipStream_t s, const int* lens = nullptr);
int wfl_launch_conv0(const Conv0Args& a, int group_norm, hipStream_t s);
int wfl_launch_clip_frames(const int* lens, int B, int L, int n, const int* kernel, const int* stride, int min_len, int* out, hipStream_t s);
int wfl_launch_posconv(const PosConvArgs& a, hipStream_t s);
int wfl_launch_regroup(const bf16_t* x, int d, int groups, int cpg, long R, long lead, int B, int P, int T, bf16_t* xg, hipStream_t s,
                       const int* clip_T = nullptr);
int wfl_launch_relpos_gate(const bf16_t* x, long ldx, long lead, int B, int P, int T, int heads, int hd, const float* w8,
                           const float* b8, const float* cst, float* gate, hipStream_t s, const bf16_t* x_lo = nullptr);
int wfl_launch_relpos_table(const float* rel_emb, const int* bucket_of_delta, int max_t, int heads, int T, float* table, hipStream_t s);
int wfl_launch_layernorm_act(const bf16_t* x, long ldx, bf16_t* y, long ldy, const float* g, const float* b, float eps, long lead,
                             int B, int P, int T, int C, int gelu, hipStream_t s, const bf16_t* x_lo = nullptr, bf16_t* y_lo = nullptr,
                             int n_div = 0, const int* clip_T = nullptr);
int wfl_launch_layernorm_pair(const bf16_t* x, const bf16_t* x_lo, bf16_t* y1, bf16_t* y1_lo, bf16_t* y2, bf16_t* y2_lo, long ld,
                              const float* g1, const float* b1, const float* g2, const float* b2, float eps, long lead, int B, int P,
                              int T, int C, int n_div, const int* clip_T, hipStream_t s);
int wfl_lstm_units_per_wg(int H);
long wfl_lstm_exchange_bytes(int H, int B);
bool wfl_lstm_split_precision_supported(int H);
bool wfl_lstm_hidden_supported(int H);
int wfl_launch_rows_fp8(const bf16_t* x, long ldx, const bf16_t* x_lo, const float* g, const float* b, float eps, long lead, int B, int P,
                        int T, int C, unsigned char* y8, long ldy8, float* scale, hipStream_t s, unsigned char* y8_lo = nullptr);          // norm.hip
int wfl_launch_axpy(float* dst, const float* src, long n, float alpha, int init, hipStream_t s);
int wfl_launch_zero_halo_multi(const ZeroMulti& z, hipStream_t s);
int wfl_launch_rows_to_f32(const bf16_t* x, long ldx, long lead, int B, int P, int T, int C, float* out, hipStream_t s, int split,
                           int shift, const bf16_t* x_lo = nullptr);

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int wfl_fail(int code, const char* msg) { return fail(code, msg); }   // (common.h: other translation units' ABI errors)
#define HIPCHK(x)                                                                            \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) return fail(-10, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

static inline uint16_t f32_to_bf16_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

static inline long round_up(long x, long m) { return (x + m - 1) / m * m; }

static std::string lstm_hidden_refusal(int H) {
  return "BiLSTM hidden size " + std::to_string(H) + " is not supported (32, 64, 128, 192, 256, 384, 512 or 640 per direction)";
}

// the launcher's rules for the slice width (wfl_launch_lstm): a multiple of 8, at most 32, dividing H, at most 64 slices per direction
static bool lstm_units_ok(int H, int U) { return U >= 8 && U % 8 == 0 && U <= 32 && H % U == 0 && H / U <= 64; }

// nn.LSTM's weight_hh of both directions -> the recurrence kernel's operand (lstm.hip): slice-major [dir][slice][4 * u_local + gate][H],
// so that the workgroup of slice s reads one contiguous 4U x H block whose rows hold the four gates of a unit side by side.
int32_t wfl_op_lstm_pack_whh(const float* whh_host, int32_t H, int32_t U, uint16_t* hi_host, uint16_t* lo_host) {
  if (!whh_host || !hi_host) return fail(-1, "wfl_op_lstm_pack_whh: null argument");
  if (!wfl_lstm_hidden_supported(H)) return fail(-4, "wfl_op_lstm_pack_whh: " + lstm_hidden_refusal(H));
  if (U <= 0) U = wfl_lstm_units_per_wg(H);
  if (!lstm_units_ok(H, U)) return fail(-1, "wfl_op_lstm_pack_whh: U must be a multiple of 8, at most 32, divide H and leave at most 64 slices");
  const int G = H / U;
  for (int dir = 0; dir < 2; ++dir)
    for (int u = 0; u < H; ++u)
      for (int gate = 0; gate < 4; ++gate) {
        const size_t src = (size_t)dir * 4 * H + (size_t)gate * H + u;       // PyTorch's row order: blocks i | f | g | o of H rows
        const int sl = u / U, ul = u % U;
        const size_t wrow = ((size_t)(dir * G + sl) * 4 * U) + 4 * ul + gate;
        for (int k = 0; k < H; ++k) {
          const float x = whh_host[src * H + k];
          const uint16_t hb = f32_to_bf16_bits(x);
          const uint32_t u32 = (uint32_t)hb << 16;
          float xh;
          memcpy(&xh, &u32, 4);
          hi_host[wrow * H + k] = hb;
          if (lo_host) lo_host[wrow * H + k] = f32_to_bf16_bits(x - xh);
        }
      }
  return 0;
}
#define WAVLM_MAX_T 4096   // frames per clip the relative-position bucket table covers (81 s of audio)

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  long numel() const { long n = 1; for (auto s : shape) n *= s; return n; }
};

// A packed Linear / Conv-as-GEMM operand
struct Lin {
  bf16_t* W = nullptr;   // [N][K] padded
  float* bias = nullptr; // [N] padded (may be null)
  int N = 0, K = 0, n_valid = 0;
  float* ln_s = nullptr; // set on a LayerNorm-folded operand: s[n] = sum_k W'[n][k] (gemm_stream.hip), bias = b + W beta
  float* w8 = nullptr;   // set on an fp8 operand: W holds OCP e4m3 bytes [N][K], w8[n] = the row's scale (GemmArgs::w8_scale)
  bf16_t* W_lo = nullptr; // "model.precision: high": bf16(w - bf16(w)), same layout as W (precise.hip)
  bf16_t* W3 = nullptr;   //   and the one-launch form's operand [N][3 K]: rows [W_hi | W_hi | W_lo] (GemmArgs::tap_wrap)
};
struct LNp { float* g = nullptr; float* b = nullptr; };

struct EncLayer { LNp ln1, ln2; Lin qkv, out, fc1, fc2, qkv_ln, fc1_ln; };   // *_ln: the LayerNorm in front folded in
struct WavlmLayer { LNp ln1, ln2; Lin qkv, out, fc1, fc2, fc1_ln; float *w8 = nullptr, *b8 = nullptr, *cst = nullptr; };
struct ConfLayer {
  LNp ff1_ln, ff2_ln, ln1, ln2;
  Lin ff1_a, ff1_b, ff2_a, ff2_b, qkv, out, pw1, conv, pw2, ff1_a_ln, ff2_a_ln;
};

// GEMM launches are timed per kernel variant (template instantiation), keyed act | glu<<2 | out_f32<<3 | res<<4 | kernel id<<5
// | LayerNorm-fold mode<<8 | statistics-emitting epilogue<<10
struct GemmProf {
  long launches[2048] = {0};
  double flops[2048] = {0};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  std::vector<int> key;
};

struct wfl_model {
  wfl_arch a{};
  bool finalized = false;
  int device = -1;                   // HIP device the weights live on (current device at wfl_finalize)
  std::vector<int> avg_langs;        // WFL_LANG_AVERAGE: the ids averaged over (default: all)
  std::map<std::string, HostTensor> host;
  std::vector<void*> dev_allocs;
  // geometry
  int halo = 16;
  // `encoder_type: none` (WFL_ENC_NONE): the hidden width dv = n_mels (80) is no multiple of the 64 columns / supported head sizes
  // the kernels are built for, so every d-wide tensor of the head lives in d >= dv columns (a.d_model is rewritten to d at
  // wfl_create), valid channel c in column c + (c >= dv/2 ? d/2 - dv/2 : 0) -- the two halves a BiLSTM writes -- and zeros elsewhere;
  // pad_head_state() moves the checkpoint's tensors into that layout, LayerNorm divides by dv.  dv == d for every other model.
  int dv = 0;
  // Conformer attention: head size the attention kernels are built for (32 .. 640) at or above d / conformer_heads, and the width
  // heads * that of its q | k | v and context rows.  Whisper-tiny's 192 (384 / 2 heads) runs as 256: the q | k | v projection writes
  // zero columns behind every head (QKp / ATTp buffers of the plan), out_proj skips them.  Equal to d for every BASELINE config.
  int conf_hd = 0, conf_da = 0;
  int pad_split() const { return dv == a.d_model ? a.d_model : dv / 2; }
  int pad_shift() const { return dv == a.d_model ? 0 : a.d_model / 2 - dv / 2; }
  // whisper front-end tables
  float *Wc = nullptr, *Ws = nullptr, *mel_w = nullptr;
  int *mel_lo = nullptr, *mel_cnt = nullptr;
  int mel_maxw = 0;
  Lin conv1, conv2;
  bf16_t* pos = nullptr;
  bf16_t* pos_lo = nullptr;     // precision high: what the table's bf16 rounding left behind
  std::vector<EncLayer> enc;
  LNp enc_ln;
  // wavlm
  float *conv0_w = nullptr, *conv0_b = nullptr;
  LNp conv0_norm;
  std::vector<Lin> fconv;            // feature-encoder layers 1..n-1 as GEMMs
  std::vector<LNp> fconv_ln;         // "layer" checkpoints: LayerNorm after every conv
  LNp fp_ln;
  Lin fp_proj;
  std::vector<Lin> posconv;          // one GEMM per group over [rows][64]-regrouped channels
  LNp wenc_ln;
  std::vector<WavlmLayer> wl;
  float* rel_emb = nullptr;          // [num_buckets][heads]
  int* bucket_of_delta = nullptr;    // [2*WAVLM_MAX_T - 1]
  // head
  Lin lang;
  float* lang_table = nullptr;    // [num_languages][d]
  std::vector<Lin> lstm_in;       // per layer: both directions' input projection, rows [dir][unit][gate]
  std::vector<bf16_t*> lstm_whh;  // per layer: [2][G][4U][H]
  std::vector<bf16_t*> lstm_whh_lo;   // precision high: the same slices' low halves (null entries where the recurrence stays bf16)
  int lstm_U = 0;
  std::vector<ConfLayer> conf;
  std::vector<Lin> dil;
  Lin cls, off1;
  Lin cls_lo, cls_hi2;             // split-precision classifier: W - bf16(W), and [bf16(W) | bf16(W)] for the [hi | lo] input taps
  Lin cls3;                        //   and the one-launch form [W_hi | W_hi | W_lo] against the tap segments [h_hi | h_lo | h_hi] (GemmArgs::tap_wrap)
  float *off_w2 = nullptr, *off_b2 = nullptr;
  // profiling
  bool prof_on = false;
  GemmProf prof;
  size_t prof_used = 0;
};

const char* wfl_last_error(void) { return g_err.c_str(); }
int32_t wfl_abi_version(void) { return WFL_ABI_VERSION; }

int32_t wfl_create(const wfl_arch* arch, wfl_model** out) {
  if (!arch || !out) return fail(-1, "wfl_create: null argument");
  if (arch->abi_version != WFL_ABI_VERSION) return fail(-1, "wfl_create: ABI version mismatch");
  const wfl_arch& a = *arch;
  if (a.encoder_type != WFL_ENC_WHISPER && a.encoder_type != WFL_ENC_WAVLM && a.encoder_type != WFL_ENC_NONE)
    return fail(-1, "unknown encoder_type");
  const bool none = a.encoder_type == WFL_ENC_NONE;
  int d_pad = a.d_model;
  if (none) {
    // model.py:82-91: hidden_size = n_mels; the head runs at that width
    if (a.n_mels <= 0 || a.d_model != a.n_mels) return fail(-1, "encoder_type none: d_model must equal n_mels");
    if (a.mel_sample_rate == 0) {          // a caller that names no rate: 16 kHz with the two Toeplitz hops, as before the field existed
      if (a.mel_hop != 160 && a.mel_hop != 320)
        return fail(-1, "encoder_type none: without mel_sample_rate the mel front-end is built for hop 160 and 320 (frame_duration 0.01 / "
                        "0.02 s at 16 kHz); set mel_sample_rate for any other hop");
    } else {
      if (a.mel_sample_rate < 8000 || a.mel_sample_rate > 192000)
        return fail(-1, "encoder_type none: mel_sample_rate must be 8000 .. 192000 Hz (or 0: 16 kHz, hop 160 / 320)");
      if (a.mel_hop < 1) return fail(-1, "encoder_type none: mel_hop must be >= 1 (int(frame_duration * sample_rate))");
    }
    if (a.d_model % 2 && a.enable_bilstm) return fail(-1, "encoder_type none: odd n_mels with a BiLSTM");
    if (a.n_conformer > 0) {
      if (a.conformer_heads <= 0 || a.d_model % a.conformer_heads) return fail(-1, "bad conformer_heads");
      d_pad = 0;
      for (int hd : {32, 64, 128, 256}) {
        const int dp = hd * a.conformer_heads;
        if (hd >= a.d_model / a.conformer_heads && dp % 64 == 0) { d_pad = dp; break; }
      }
      if (!d_pad) return fail(-1, "encoder_type none: n_mels / conformer_heads above 256 is not supported");
    } else {
      d_pad = (int)round_up(a.d_model, 64);
    }
  } else {
    if (a.d_model <= 0 || a.d_model % 64) return fail(-1, "d_model must be a positive multiple of 64");
    if (a.enc_heads <= 0 || a.d_model % a.enc_heads) return fail(-1, "enc_heads must divide d_model");
  }
  if (!none && a.enc_layers <= 0) return fail(-1, "enc_layers must be positive");
  if (a.num_classes <= 0 || a.o_id < 0 || a.o_id >= a.num_classes) return fail(-1, "bad num_classes / o_id");
  if (a.n_conformer > 0 && (a.conformer_heads <= 0 || a.d_model % a.conformer_heads)) return fail(-1, "bad conformer_heads");
  if (a.n_conformer > 0 && a.conformer_kernel % 2 == 0) return fail(-1, "even conformer_kernel_size is not supported");
  int conf_hd = 0;
  if (a.n_conformer > 0) {
    const int hd = d_pad / a.conformer_heads;
    for (int v : {32, 64, 128, 256, 384, 512, 640})
      if (!conf_hd && v >= hd) conf_hd = v;
    if (!conf_hd) return fail(-1, "conformer head size " + std::to_string(hd) + " (d_model / conformer_heads) is above 640");
  }
  if (a.enable_dilated && a.dilated_kernel % 2 == 0) return fail(-1, "even dilated_conv_kernel is not supported");
  if (a.fp8_weights && (a.encoder_type != WFL_ENC_WHISPER || a.d_model % 256 || a.enc_ffn % 256))
    return fail(-1, "fp8_weights: Whisper encoders with d_model and ffn multiples of 256 only");
  if (a.fp8_activations && !a.fp8_weights) return fail(-1, "fp8_activations needs fp8_weights");
  if (a.fp8_activations < 0 || a.fp8_activations > 3) return fail(-1, "fp8_activations: 0 (bf16), 1 / 2 (e4m3) or 3 (e4m3 pairs)");
  if (a.precision && a.fp8_weights) return fail(-1, "precision = 1 (three-pass bf16 pairs) and fp8_weights contradict each other");
  wfl_model* m = new wfl_model();
  m->a = a;
  m->dv = a.d_model;
  m->a.d_model = d_pad;
  m->conf_hd = conf_hd;
  m->conf_da = conf_hd * (a.n_conformer > 0 ? a.conformer_heads : 0);
  int pad = 1;
  if (a.n_conformer > 0) pad = std::max(pad, a.conformer_kernel / 2);
  if (a.enable_dilated)
    for (int i = 0; i < a.dilated_depth; ++i) pad = std::max(pad, (1 << i) * (a.dilated_kernel - 1) / 2);
  if (a.encoder_type == WFL_ENC_WAVLM) {
    if (a.wavlm_n_conv < 2 || a.wavlm_n_conv > 8 || a.wavlm_conv_kernel[0] != 10 || a.wavlm_conv_stride[0] != 5) {
      delete m;
      return fail(-1, "WavLM feature encoder: layer 0 must be k=10 s=5 (all released checkpoints)");
    }
    for (int i = 1; i < a.wavlm_n_conv; ++i)
      if (a.wavlm_conv_stride[i] != 2 || a.wavlm_conv_dim[i] != a.wavlm_conv_dim[0] || a.wavlm_conv_dim[i] % 8 || a.wavlm_conv_dim[i] > 512) {
        delete m;
        return fail(-1, "WavLM feature encoder: layers 1.. must be stride 2 with one common width <= 512");
      }
    if (a.wavlm_pos_conv_kernel % 2 || a.d_model % a.wavlm_pos_conv_groups || a.d_model / a.wavlm_pos_conv_groups > 64 ||
        (a.d_model / a.wavlm_pos_conv_groups) % 8) {
      delete m;
      return fail(-1, "WavLM positional conv: even kernel and d_model/groups a multiple of 8, <= 64");
    }
    pad = std::max(pad, a.wavlm_pos_conv_kernel / 2);
  }
  m->halo = (int)round_up(pad + 1, 8);
  *out = m;
  return 0;
}

void wfl_destroy(wfl_model* m) {
  if (!m) return;
  for (void* p : m->dev_allocs) (void)hipFree(p);
  for (auto& e : m->prof.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  delete m;
}

int32_t wfl_load_tensor(wfl_model* m, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
  if (!m || !name || (!data && ndim > 0)) return fail(-1, "wfl_load_tensor: null argument");
  if (m->finalized) return fail(-1, "wfl_load_tensor: model already finalized");
  HostTensor t;
  long n = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
  if (data) t.data.assign(data, data + n);
  m->host[name] = std::move(t);
  return 0;
}

// ------------------------------------------------------------------------------------------------ packing helpers
namespace {

struct Packer {
  wfl_model* m;
  std::set<std::string> used;
  std::string err;

  const HostTensor* get(const std::string& name, std::initializer_list<int64_t> shape) {
    auto it = m->host.find(name);
    if (it == m->host.end()) { if (err.empty()) err = "missing key in state_dict: " + name; return nullptr; }
    std::vector<int64_t> want(shape);
    if (it->second.shape != want) {
      if (err.empty()) {
        err = "size mismatch for " + name + ": got [";
        for (auto s : it->second.shape) err += std::to_string(s) + ",";
        err += "] expected [";
        for (auto s : want) err += std::to_string(s) + ",";
        err += "]";
      }
      return nullptr;
    }
    used.insert(name);
    return &it->second;
  }

  template <class T>
  T* upload(const std::vector<T>& v) {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(v.size() * sizeof(T), 16)) != hipSuccess) { if (err.empty()) err = "hipMalloc failed"; return nullptr; }
    m->dev_allocs.push_back(d);
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
      if (err.empty()) err = "hipMemcpy failed";
      return nullptr;
    }
    return (T*)d;
  }

  // rows[n][k] fp32 (n_valid x k_valid) -> padded bf16 [N][K] + fp32 bias [N]
  Lin pack(const std::vector<float>& rows, int n_valid, int k_valid, const std::vector<float>* bias) {
    Lin L;
    L.n_valid = n_valid;
    L.N = (int)round_up(n_valid, 128);
    L.K = (int)round_up(k_valid, 64);
    std::vector<uint16_t> w((size_t)L.N * L.K, 0);
    for (int n = 0; n < n_valid; ++n)
      for (int k = 0; k < k_valid; ++k) w[(size_t)n * L.K + k] = f32_to_bf16_bits(rows[(size_t)n * k_valid + k]);
    L.W = (bf16_t*)upload(w);
    if (m->a.precision) {                      // the weights' low halves for the split-precision passes (precise.hip)
      std::vector<uint16_t> wl((size_t)L.N * L.K, 0);
      for (int n = 0; n < n_valid; ++n)
        for (int k = 0; k < k_valid; ++k) {
          const float x = rows[(size_t)n * k_valid + k];
          const uint32_t u = (uint32_t)w[(size_t)n * L.K + k] << 16;
          float xh;
          memcpy(&xh, &u, 4);
          wl[(size_t)n * L.K + k] = f32_to_bf16_bits(x - xh);
        }
      L.W_lo = (bf16_t*)upload(wl);
      std::vector<uint16_t> w3((size_t)L.N * 3 * L.K);
      for (int n = 0; n < L.N; ++n) {
        memcpy(&w3[((size_t)n * 3 + 0) * L.K], &w[(size_t)n * L.K], (size_t)L.K * 2);
        memcpy(&w3[((size_t)n * 3 + 1) * L.K], &w[(size_t)n * L.K], (size_t)L.K * 2);
        memcpy(&w3[((size_t)n * 3 + 2) * L.K], &wl[(size_t)n * L.K], (size_t)L.K * 2);
      }
      L.W3 = (bf16_t*)upload(w3);
    }
    std::vector<float> b((size_t)L.N, 0.f);
    if (bias) for (int n = 0; n < n_valid; ++n) b[n] = (*bias)[n];
    L.bias = upload(b);
    return L;
  }

  // OCP e4m3 (fn) encode, round to nearest even, saturating at 448: nearest entry of the 127 non-negative code points
  static uint8_t e4m3_encode(float x) {
    static float tab[127];
    static bool init = false;
    if (!init) {
      for (int b = 0; b < 127; ++b) {
        const int e = b >> 3, mnt = b & 7;
        tab[b] = e == 0 ? (float)mnt / 8.0f * 0.015625f : (1.0f + (float)mnt / 8.0f) * std::ldexp(1.0f, e - 7);
      }
      init = true;
    }
    const uint8_t sign = std::signbit(x) ? 0x80 : 0;
    const float a = std::fabs(x);
    if (!(a == a)) return 0x7F;
    if (a >= 448.0f) return sign | 126;
    int lo = 0, hi = 126;                       // tab[lo] <= a < tab[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tab[mid] <= a) lo = mid; else hi = mid; }
    const float dl = a - tab[lo], dh = tab[hi] - a;
    const int pick = dl < dh ? lo : (dh < dl ? hi : ((lo & 1) ? hi : lo));
    return sign | (uint8_t)pick;
  }
  static float e4m3_decode(uint8_t b) {
    const int e = (b >> 3) & 15, mnt = b & 7;
    const float v = e == 0 ? (float)mnt / 8.0f * 0.015625f : (1.0f + (float)mnt / 8.0f) * std::ldexp(1.0f, e - 7);
    return (b & 0x80) ? -v : v;
  }

  // rows[n][k] fp32 -> e4m3 bytes [N][K] (padded) + per-row fp32 scale (row max -> 448) + fp32 bias [N]
  Lin pack8(const std::vector<float>& rows, int n_valid, int k_valid, const std::vector<float>* bias) {
    Lin L;
    L.n_valid = n_valid;
    L.N = (int)round_up(n_valid, 256);
    L.K = (int)round_up(k_valid, 64);
    std::vector<uint8_t> w((size_t)L.N * L.K, 0);
    std::vector<float> sc((size_t)L.N, 1.0f);
    for (int n = 0; n < n_valid; ++n) {
      float mx = 0.f;
      for (int k = 0; k < k_valid; ++k) mx = std::max(mx, std::fabs(rows[(size_t)n * k_valid + k]));
      const float scale = mx > 0.f ? mx / 448.0f : 1.0f;
      sc[n] = scale;
      for (int k = 0; k < k_valid; ++k) w[(size_t)n * L.K + k] = e4m3_encode(rows[(size_t)n * k_valid + k] / scale);
    }
    L.W = (bf16_t*)upload(w);
    L.w8 = upload(sc);
    std::vector<float> b((size_t)L.N, 0.f);
    if (bias) for (int n = 0; n < n_valid; ++n) b[n] = (*bias)[n];
    L.bias = upload(b);
    return L;
  }
  Lin linear8(const std::string& p, int out_f, int in_f) {
    const HostTensor* w = get(p + ".weight", {out_f, in_f});
    const HostTensor* b = get(p + ".bias", {out_f});
    if (!w || !b) return Lin();
    return pack8(w->data, out_f, in_f, &b->data);
  }

  // LayerNorm(gamma, beta) folded into the Linear that consumes it (gemm_stream.hip): W' = gamma o W rounded to bf16,
  // s[n] = sum_k W'[n][k] over the ROUNDED weights (what the MFMA multiplies), bias' = bias + W beta.
  Lin pack_ln(const std::vector<float>& rows, int n_valid, int k_valid, const std::vector<float>* bias, const std::string& ln_name) {
    const HostTensor* g = get(ln_name + ".weight", {k_valid});
    const HostTensor* b = get(ln_name + ".bias", {k_valid});
    if (!g || !b) return Lin();
    std::vector<float> wf((size_t)n_valid * k_valid), bf(n_valid), sv;
    for (int n = 0; n < n_valid; ++n) {
      double acc = bias ? (*bias)[n] : 0.0;
      for (int k = 0; k < k_valid; ++k) {
        const float w = rows[(size_t)n * k_valid + k];
        wf[(size_t)n * k_valid + k] = w * g->data[k];
        acc += (double)w * b->data[k];
      }
      bf[n] = (float)acc;
    }
    Lin L = pack(wf, n_valid, k_valid, &bf);
    sv.assign((size_t)L.N, 0.f);
    for (int n = 0; n < n_valid; ++n) {
      double acc = 0.0;
      for (int k = 0; k < k_valid; ++k) {
        const uint32_t u = (uint32_t)f32_to_bf16_bits(wf[(size_t)n * k_valid + k]) << 16;
        float r;
        memcpy(&r, &u, 4);
        acc += r;
      }
      sv[n] = (float)acc;
    }
    L.ln_s = upload(sv);
    return L;
  }
  Lin linear_ln(const std::string& p, int out_f, int in_f, const std::string& ln_name) {
    const HostTensor* w = get(p + ".weight", {out_f, in_f});
    const HostTensor* b = get(p + ".bias", {out_f});
    if (!w || !b) return Lin();
    return pack_ln(w->data, out_f, in_f, &b->data, ln_name);
  }

  Lin linear(const std::string& p, int out_f, int in_f, bool has_bias = true) {
    const HostTensor* w = get(p + ".weight", {out_f, in_f});
    const HostTensor* b = has_bias ? get(p + ".bias", {out_f}) : nullptr;
    if (!w || (has_bias && !b)) return Lin();
    return pack(w->data, out_f, in_f, has_bias ? &b->data : nullptr);
  }

  // Conv1d weight [cout][cin][k] -> tap-major rows [cout][k*cin]; optional per-output-channel scale/shift (BN fold)
  Lin conv(const std::string& p, int cout, int cin, int k, const std::vector<float>* scale = nullptr,
           const std::vector<float>* shift = nullptr, bool has_bias = true) {
    const HostTensor* w = get(p + ".weight", {cout, cin, k});
    const HostTensor* b = has_bias ? get(p + ".bias", {cout}) : nullptr;
    if (!w || (has_bias && !b)) return Lin();
    std::vector<float> rows((size_t)cout * k * cin), bias(cout, 0.f);
    for (int co = 0; co < cout; ++co) {
      const float sc = scale ? (*scale)[co] : 1.f;
      for (int ci = 0; ci < cin; ++ci)
        for (int j = 0; j < k; ++j) rows[((size_t)co * k + j) * cin + ci] = w->data[((size_t)co * cin + ci) * k + j] * sc;
      float bv = has_bias ? b->data[co] : 0.f;
      bias[co] = bv * sc + (shift ? (*shift)[co] : 0.f);
    }
    return pack(rows, cout, k * cin, &bias);
  }

  LNp ln(const std::string& p, int d) {
    LNp r;
    const HostTensor* g = get(p + ".weight", {d});
    const HostTensor* b = get(p + ".bias", {d});
    if (!g || !b) return r;
    r.g = upload(g->data);
    r.b = upload(b->data);
    return r;
  }
};

// Slaney mel filter bank, as HF audio_utils.py:638-729 with feature_extraction_whisper.py:97-105's arguments
// (0..8000 Hz, 201 bins, norm="slaney", mel_scale="slaney"); float64 then rounded to fp32 like the reference.
// htk = true: torchaudio.functional.melscale_fbanks(n_freqs = 201, 0, sr / 2, n_mels, sr, norm = None, mel_scale = "htk"), the bank
// behind torchaudio.transforms.MelSpectrogram's defaults (/root/reference/model.py:85-90): m = 2595 log10(1 + f / 700), plain
// triangles of height 1.
static void build_mel(int n_mels, std::vector<int>& lo, std::vector<int>& cnt, std::vector<float>& w, int& maxw, bool htk = false,
                      double fmax = 8000.0) {
  const int nf = 201;
  auto hz2mel = [htk](double f) {
    if (htk) return 2595.0 * std::log10(1.0 + f / 700.0);
    return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0;
  };
  auto mel2hz = [htk](double mm) {
    if (htk) return 700.0 * (std::pow(10.0, mm / 2595.0) - 1.0);
    return mm >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (mm - 15.0)) : 200.0 * mm / 3.0;
  };
  const double m0 = hz2mel(0.0), m1 = hz2mel(fmax);
  std::vector<double> ff(n_mels + 2);
  for (int i = 0; i < n_mels + 2; ++i) ff[i] = mel2hz(m0 + (m1 - m0) * i / (n_mels + 1));
  std::vector<std::vector<float>> fb(n_mels, std::vector<float>(nf, 0.f));
  for (int k = 0; k < nf; ++k) {
    const double f = fmax * k / (nf - 1);
    for (int i = 0; i < n_mels; ++i) {
      const double down = (f - ff[i]) / (ff[i + 1] - ff[i]);
      const double up = (ff[i + 2] - f) / (ff[i + 2] - ff[i + 1]);
      const double v = std::max(0.0, std::min(down, up)) * (htk ? 1.0 : 2.0 / (ff[i + 2] - ff[i]));
      fb[i][k] = (float)v;
    }
  }
  lo.assign(n_mels, 0);
  cnt.assign(n_mels, 0);
  maxw = 1;
  for (int i = 0; i < n_mels; ++i) {
    int a = nf, b = -1;
    for (int k = 0; k < nf; ++k)
      if (fb[i][k] != 0.f) { a = std::min(a, k); b = std::max(b, k); }
    if (b >= a) { lo[i] = a; cnt[i] = b - a + 1; maxw = std::max(maxw, cnt[i]); }
  }
  w.assign((size_t)n_mels * maxw, 0.f);
  for (int i = 0; i < n_mels; ++i)
    for (int j = 0; j < cnt[i]; ++j) w[(size_t)i * maxw + j] = fb[i][lo[i] + j];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ finalize
// STFT front-end tables: Hann-folded DFT matrix (periodic Hann as torch.hann_window(400)) + the sparse mel bank
static void build_frontend_tables(wfl_model* m, Packer& P, bool htk, double fmax) {
  // folded about n = 200 (see logmel.hip): row j-1 <-> sample j = 1..200; Wc[200] carries the factor 1/2
  std::vector<float> wc((size_t)200 * 224, 0.f), ws((size_t)200 * 224, 0.f);
  for (int j = 1; j <= 200; ++j) {
    const double hann = 0.5 - 0.5 * std::cos(2.0 * M_PI * j / 400.0);
    const double fold = j == 200 ? 0.5 : 1.0;
    for (int k = 0; k <= 200; ++k) {
      const int nk = (int)(((long)j * k) % 400);
      const double ang = 2.0 * M_PI * nk / 400.0;
      wc[(size_t)(j - 1) * 224 + k] = (float)(fold * hann * std::cos(ang));
      ws[(size_t)(j - 1) * 224 + k] = (float)(-hann * std::sin(ang));
    }
  }
  m->Wc = P.upload(wc);
  m->Ws = P.upload(ws);
  std::vector<int> lo, cnt;
  std::vector<float> w;
  build_mel(m->a.n_mels, lo, cnt, w, m->mel_maxw, htk, fmax);
  m->mel_lo = P.upload(lo);
  m->mel_cnt = P.upload(cnt);
  m->mel_w = P.upload(w);
}

// `encoder_type: none`: move the head's checkpoint tensors (width dv) into the padded channel layout (width d, see wfl_model::dv).
// Rows / columns that carry no channel are zero, so every padded activation column stays exactly zero through Linear, Conv1d,
// GELU / ReLU / GLU, LayerNorm (gamma = beta = 0), eval-mode BatchNorm (scale 0), attention (zero q, k, v columns) and the LSTM
// (zero gates: i = f = o = 1/2, g = 0, so c = h = 0).
static void pad_head_state(wfl_model* m, Packer& P) {
  const wfl_arch& a = m->a;
  const int dv = m->dv, d = a.d_model, e = a.lang_emb_dim;
  if (dv == d) return;
  const int split = m->pad_split(), shift = m->pad_shift();
  auto pi = [&](int c) { return c + (c >= split ? shift : 0); };
  std::vector<int> PI(dv), ID_C(a.num_classes), ID2(2);
  for (int c = 0; c < dv; ++c) PI[c] = pi(c);
  for (int c = 0; c < a.num_classes; ++c) ID_C[c] = c;
  ID2[0] = 0; ID2[1] = 1;
  auto ident = [](int n) { std::vector<int> v(n); for (int i = 0; i < n; ++i) v[i] = i; return v; };
  // tensor [rows][cols][taps] (taps = 1: a matrix; cols = 0: a vector) -> [n_out][k_out][taps]
  auto move = [&](const std::string& name, const std::vector<int>& rmap, int n_out, const std::vector<int>& cmap, int k_out, int taps,
                  float fill = 0.f) {
    auto it = m->host.find(name);
    if (it == m->host.end()) return;                  // finalize_head reports the missing key
    HostTensor& t = it->second;
    std::vector<int64_t> want{(int64_t)rmap.size()};
    if (!cmap.empty()) want.push_back((int64_t)cmap.size());
    if (taps > 1 || t.shape.size() == 3) want.push_back(taps);
    if (t.shape != want) {
      if (P.err.empty()) {
        P.err = "size mismatch for " + name + ": got [";
        for (auto v : t.shape) P.err += std::to_string(v) + ",";
        P.err += "] expected [";
        for (auto v : want) P.err += std::to_string(v) + ",";
        P.err += "]";
      }
      return;
    }
    HostTensor o;
    const int kin = cmap.empty() ? 1 : (int)cmap.size(), kout = cmap.empty() ? 1 : k_out;
    o.data.assign((size_t)n_out * kout * taps, fill);
    for (size_t r = 0; r < rmap.size(); ++r)
      for (int c = 0; c < kin; ++c)
        for (int j = 0; j < taps; ++j)
          o.data[((size_t)rmap[r] * kout + (cmap.empty() ? 0 : cmap[c])) * taps + j] = t.data[((size_t)r * kin + c) * taps + j];
    o.shape.push_back(n_out);
    if (!cmap.empty()) o.shape.push_back(k_out);
    if (t.shape.size() == 3) o.shape.push_back(taps);
    t = std::move(o);
  };
  const std::vector<int> none;
  {                                                   // lang_proj: [dv][dv + e]: hidden columns through pi, embedding columns behind them
    std::vector<int> cm(dv + e);
    for (int c = 0; c < dv; ++c) cm[c] = pi(c);
    for (int c = 0; c < e; ++c) cm[dv + c] = d + c;
    move("lang_proj.weight", PI, d, cm, d + e, 1);
    move("lang_proj.bias", PI, d, none, 0, 1);
  }
  if (a.enable_bilstm) {
    const int Hv = dv / 2, Hp = d / 2;
    std::vector<int> gm(4 * Hv);
    for (int g = 0; g < 4; ++g)
      for (int u = 0; u < Hv; ++u) gm[g * Hv + u] = g * Hp + u;
    for (int layer = 0; layer < a.bilstm_layers; ++layer)
      for (int dir = 0; dir < 2; ++dir) {
        const std::string suf = "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
        move("bilstm.weight_ih" + suf, gm, 4 * Hp, PI, d, 1);          // layer 0 reads the hidden states, deeper ones [fwd | bwd]: both pi
        move("bilstm.weight_hh" + suf, gm, 4 * Hp, ident(Hv), Hp, 1);
        move("bilstm.bias_ih" + suf, gm, 4 * Hp, none, 0, 1);
        move("bilstm.bias_hh" + suf, gm, 4 * Hp, none, 0, 1);
      }
  }
  const int x = a.conformer_ff_expansion, kk = a.conformer_kernel;
  for (int i = 0; i < a.n_conformer; ++i) {
    const std::string p = "conformer_layers." + std::to_string(i) + ".";
    const int hv = dv / a.conformer_heads, hp = d / a.conformer_heads;
    std::vector<int> hm(dv), qm(3 * dv), gl(2 * dv);
    for (int c = 0; c < dv; ++c) hm[c] = (c / hv) * hp + c % hv;             // per-head padding of the attention's channel axis
    for (int b = 0; b < 3; ++b)
      for (int c = 0; c < dv; ++c) qm[b * dv + c] = b * d + hm[c];
    for (int c = 0; c < dv; ++c) { gl[c] = pi(c); gl[dv + c] = d + pi(c); }   // GLU: value half | gate half
    for (const char* ff : {"ff1", "ff2"}) {
      const std::string q = p + ff + ".net.";
      move(q + "0.weight", PI, d, none, 0, 1);
      move(q + "0.bias", PI, d, none, 0, 1);
      move(q + "1.weight", ident(dv * x), d * x, PI, d, 1);
      move(q + "1.bias", ident(dv * x), d * x, none, 0, 1);
      move(q + "4.weight", PI, d, ident(dv * x), d * x, 1);
      move(q + "4.bias", PI, d, none, 0, 1);
    }
    move(p + "self_attn.in_proj_weight", qm, 3 * d, PI, d, 1);
    move(p + "self_attn.in_proj_bias", qm, 3 * d, none, 0, 1);
    move(p + "self_attn.out_proj.weight", PI, d, hm, d, 1);
    move(p + "self_attn.out_proj.bias", PI, d, none, 0, 1);
    for (const char* ln : {"ln1", "ln2"}) {
      move(p + ln + ".weight", PI, d, none, 0, 1);
      move(p + ln + ".bias", PI, d, none, 0, 1);
    }
    move(p + "conv.0.weight", gl, 2 * d, PI, d, 1);
    move(p + "conv.0.bias", gl, 2 * d, none, 0, 1);
    move(p + "conv.2.weight", PI, d, PI, d, kk);
    move(p + "conv.2.bias", PI, d, none, 0, 1);
    move(p + "conv.3.weight", PI, d, none, 0, 1);
    move(p + "conv.3.bias", PI, d, none, 0, 1);
    move(p + "conv.3.running_mean", PI, d, none, 0, 1);
    move(p + "conv.3.running_var", PI, d, none, 0, 1, 1.0f);
    move(p + "conv.5.weight", PI, d, PI, d, 1);
    move(p + "conv.5.bias", PI, d, none, 0, 1);
  }
  if (a.enable_dilated)
    for (int i = 0; i < a.dilated_depth; ++i) {
      const std::string p = "dilated_conv_stack." + std::to_string(2 * i);
      move(p + ".weight", PI, d, PI, d, a.dilated_kernel);
      move(p + ".bias", PI, d, none, 0, 1);
    }
  move("classifier.weight", ID_C, a.num_classes, PI, d, 1);
  move("boundary_offset_head.0.weight", PI, d, PI, d, 3);
  move("boundary_offset_head.0.bias", PI, d, none, 0, 1);
  move("boundary_offset_head.2.weight", ID2, 2, PI, d, 1);
}

static int finalize_whisper(wfl_model* m, Packer& P) {
  const wfl_arch& a = m->a;
  const int d = a.d_model, hd = d / a.enc_heads;
  build_frontend_tables(m, P, false, 8000.0);
  m->conv1 = P.conv("encoder.conv1", d, a.n_mels, 3);
  m->conv2 = P.conv("encoder.conv2", d, d, 3);
  if (const HostTensor* pe = P.get("encoder.embed_positions.weight", {a.max_positions, d})) {
    std::vector<uint16_t> pb(pe->data.size());
    for (size_t i = 0; i < pb.size(); ++i) pb[i] = f32_to_bf16_bits(pe->data[i]);
    m->pos = (bf16_t*)P.upload(pb);
    if (a.precision) {
      for (size_t i = 0; i < pb.size(); ++i) {
        const uint32_t u = (uint32_t)pb[i] << 16;
        float xh;
        memcpy(&xh, &u, 4);
        pb[i] = f32_to_bf16_bits(pe->data[i] - xh);
      }
      m->pos_lo = (bf16_t*)P.upload(pb);
    }
  }
  const float qs = (float)(std::pow((double)hd, -0.5) * 1.4426950408889634);   // hd^-1/2 * log2(e)
  m->enc.resize(a.enc_layers);
  for (int i = 0; i < a.enc_layers; ++i) {
    const std::string p = "encoder.layers." + std::to_string(i) + ".";
    EncLayer& L = m->enc[i];
    L.ln1 = P.ln(p + "self_attn_layer_norm", d);
    L.ln2 = P.ln(p + "final_layer_norm", d);
    const HostTensor* wq = P.get(p + "self_attn.q_proj.weight", {d, d});
    const HostTensor* bq = P.get(p + "self_attn.q_proj.bias", {d});
    const HostTensor* wk = P.get(p + "self_attn.k_proj.weight", {d, d});
    const HostTensor* wv = P.get(p + "self_attn.v_proj.weight", {d, d});
    const HostTensor* bv = P.get(p + "self_attn.v_proj.bias", {d});
    if (wq && bq && wk && wv && bv) {
      std::vector<float> rows((size_t)3 * d * d), bias((size_t)3 * d, 0.f);
      for (size_t j = 0; j < (size_t)d * d; ++j) {
        rows[j] = wq->data[j] * qs;
        rows[(size_t)d * d + j] = wk->data[j];
        rows[(size_t)2 * d * d + j] = wv->data[j];
      }
      for (int j = 0; j < d; ++j) { bias[j] = bq->data[j] * qs; bias[2 * d + j] = bv->data[j]; }
      if (a.fp8_weights) {
        L.qkv = P.pack8(rows, 3 * d, d, &bias);
      } else {
        L.qkv = P.pack(rows, 3 * d, d, &bias);
        L.qkv_ln = P.pack_ln(rows, 3 * d, d, &bias, p + "self_attn_layer_norm");
      }
    }
    if (a.fp8_weights) {
      // fp8 weights (BASELINE configs[4]): the four big operands of every layer as e4m3 + per-channel scale; no LayerNorm folding
      // (its gamma would have to go into the quantised tensor), the LayerNorm kernel feeds the plain fp8 GEMM
      L.out = P.linear8(p + "self_attn.out_proj", d, d);
      L.fc1 = P.linear8(p + "fc1", a.enc_ffn, d);
      L.fc2 = P.linear8(p + "fc2", d, a.enc_ffn);
    } else {
      L.out = P.linear(p + "self_attn.out_proj", d, d);
      L.fc1 = P.linear(p + "fc1", a.enc_ffn, d);
      L.fc1_ln = P.linear_ln(p + "fc1", a.enc_ffn, d, p + "final_layer_norm");
      L.fc2 = P.linear(p + "fc2", d, a.enc_ffn);
    }
  }
  m->enc_ln = P.ln("encoder.layer_norm", d);
  return 0;
}

static int finalize_wavlm(wfl_model* m, Packer& P) {
  const wfl_arch& a = m->a;
  const int d = a.d_model, hd = d / a.enc_heads, C = a.wavlm_conv_dim[0], nconv = a.wavlm_n_conv;
  const bool group = a.wavlm_group_norm != 0, cbias = a.wavlm_conv_bias != 0;
  const std::string fe = "encoder.feature_extractor.conv_layers.";
  if (const HostTensor* w0 = P.get(fe + "0.conv.weight", {C, 1, 10})) m->conv0_w = P.upload(w0->data);
  if (cbias)
    if (const HostTensor* b0 = P.get(fe + "0.conv.bias", {C})) m->conv0_b = P.upload(b0->data);
  m->conv0_norm = P.ln(fe + "0.layer_norm", C);
  for (int i = 1; i < nconv; ++i) {
    m->fconv.push_back(P.conv(fe + std::to_string(i) + ".conv", C, C, a.wavlm_conv_kernel[i], nullptr, nullptr, cbias));
    if (!group) m->fconv_ln.push_back(P.ln(fe + std::to_string(i) + ".layer_norm", C));
  }
  m->fp_ln = P.ln("encoder.feature_projection.layer_norm", C);
  m->fp_proj = P.linear("encoder.feature_projection.projection", d, C);
  // positional conv: weight = g * v / ||v||, norm over dims (0, 1) per tap (weight_norm dim=2); HF modeling_wavlm.py:48-90
  {
    const int G = a.wavlm_pos_conv_groups, cpg = d / G, K = a.wavlm_pos_conv_kernel;
    const std::string pc = "encoder.encoder.pos_conv_embed.conv.";
    const HostTensor* g0 = P.get(pc + "parametrizations.weight.original0", {1, 1, K});
    const HostTensor* v = P.get(pc + "parametrizations.weight.original1", {d, cpg, K});
    const HostTensor* pb = P.get(pc + "bias", {d});
    if (g0 && v && pb) {
      std::vector<double> nrm(K, 0.0);
      for (int o = 0; o < d; ++o)
        for (int c = 0; c < cpg; ++c)
          for (int k = 0; k < K; ++k) { const double x = v->data[((size_t)o * cpg + c) * K + k]; nrm[k] += x * x; }
      for (int k = 0; k < K; ++k) nrm[k] = std::sqrt(nrm[k]);
      for (int gi = 0; gi < G; ++gi) {
        // rows = the group's cpg output channels, k index = tap * 64 + channel (channels padded to 64)
        std::vector<float> rows((size_t)cpg * K * 64, 0.f), bias(cpg);
        for (int o = 0; o < cpg; ++o) {
          const int oc = gi * cpg + o;
          bias[o] = pb->data[oc];
          for (int c = 0; c < cpg; ++c)
            for (int k = 0; k < K; ++k)
              rows[((size_t)o * K + k) * 64 + c] = (float)(g0->data[k] * v->data[((size_t)oc * cpg + c) * K + k] / nrm[k]);
        }
        m->posconv.push_back(P.pack(rows, cpg, K * 64, &bias));
      }
    }
  }
  m->wenc_ln = P.ln("encoder.encoder.layer_norm", d);
  const float qs = (float)(std::pow((double)hd, -0.5) * 1.4426950408889634);
  m->wl.resize(a.enc_layers);
  for (int i = 0; i < a.enc_layers; ++i) {
    const std::string p = "encoder.encoder.layers." + std::to_string(i) + ".";
    WavlmLayer& L = m->wl[i];
    L.ln1 = P.ln(p + "layer_norm", d);
    L.ln2 = P.ln(p + "final_layer_norm", d);
    const HostTensor* wq = P.get(p + "attention.q_proj.weight", {d, d});
    const HostTensor* bq = P.get(p + "attention.q_proj.bias", {d});
    const HostTensor* wk = P.get(p + "attention.k_proj.weight", {d, d});
    const HostTensor* bk = P.get(p + "attention.k_proj.bias", {d});
    const HostTensor* wv = P.get(p + "attention.v_proj.weight", {d, d});
    const HostTensor* bv = P.get(p + "attention.v_proj.bias", {d});
    if (wq && bq && wk && bk && wv && bv) {
      std::vector<float> rows((size_t)3 * d * d), bias((size_t)3 * d);
      for (size_t j = 0; j < (size_t)d * d; ++j) {
        rows[j] = wq->data[j] * qs;
        rows[(size_t)d * d + j] = wk->data[j];
        rows[(size_t)2 * d * d + j] = wv->data[j];
      }
      for (int j = 0; j < d; ++j) { bias[j] = bq->data[j] * qs; bias[d + j] = bk->data[j]; bias[2 * d + j] = bv->data[j]; }
      L.qkv = P.pack(rows, 3 * d, d, &bias);
    }
    L.out = P.linear(p + "attention.out_proj", d, d);
    L.fc1 = P.linear(p + "feed_forward.intermediate_dense", a.enc_ffn, d);
    // (stable layers: final_layer_norm could fold into fc1 like Whisper's; measured on cfg3 it costs more in the residual GEMM's
    //  statistics epilogue -- four 256-column tiles at d = 1024 -- and the folded fc1 than the LayerNorm launch it saves:
    //  GEMM family +1.2 ms, LayerNorm -0.84 ms per 64 x 10 s step.  Set WFL_WAVLM_LN_FOLD=1 to try it.)
    if (a.wavlm_stable_layer_norm && getenv("WFL_WAVLM_LN_FOLD") && atoi(getenv("WFL_WAVLM_LN_FOLD")))
      L.fc1_ln = P.linear_ln(p + "feed_forward.intermediate_dense", a.enc_ffn, d, p + "final_layer_norm");
    L.fc2 = P.linear(p + "feed_forward.output_dense", d, a.enc_ffn);
    if (const HostTensor* w8 = P.get(p + "attention.gru_rel_pos_linear.weight", {8, hd})) L.w8 = P.upload(w8->data);
    if (const HostTensor* b8 = P.get(p + "attention.gru_rel_pos_linear.bias", {8})) L.b8 = P.upload(b8->data);
    if (const HostTensor* cst = P.get(p + "attention.gru_rel_pos_const", {1, a.enc_heads, 1, 1})) L.cst = P.upload(cst->data);
    if (i == 0) {
      if (const HostTensor* re = P.get(p + "attention.rel_attn_embed.weight", {a.wavlm_num_buckets, a.enc_heads})) {
        std::vector<float> scaled(re->data);
        for (auto& x : scaled) x *= 1.4426950408889634f;           // scores live in the log2 domain
        m->rel_emb = P.upload(scaled);
      }
    }
  }
  // relative-position buckets (HF modeling_wavlm.py:243-271), float32 arithmetic like torch
  {
    std::vector<int> bod(2 * WAVLM_MAX_T - 1);
    const int nb = a.wavlm_num_buckets / 2, max_exact = nb / 2;
    for (int delta = -(WAVLM_MAX_T - 1); delta <= WAVLM_MAX_T - 1; ++delta) {
      int bkt = delta > 0 ? nb : 0;
      const int ad = delta < 0 ? -delta : delta;
      if (ad < max_exact) bkt += ad;
      else {
        const float v = std::log((float)ad / (float)max_exact) / (float)std::log((double)a.wavlm_max_distance / max_exact) * (float)(nb - max_exact);
        int large = max_exact + (int)v;
        if (large > nb - 1) large = nb - 1;
        bkt += large;
      }
      bod[delta + WAVLM_MAX_T - 1] = bkt;
    }
    m->bucket_of_delta = P.upload(bod);
  }
  return 0;
}

static int finalize_head(wfl_model* m, Packer& P) {
  const wfl_arch& a = m->a;
  const int d = a.d_model, e = a.lang_emb_dim;
  // language conditioning: cat(h, emb) @ W^T + b  ==  h @ W[:, :d]^T + (W[:, d:] @ emb + b)   (model.py:176-180)
  const HostTensor* emb = P.get("lang_emb.weight", {a.num_languages, e});
  const HostTensor* lw = P.get("lang_proj.weight", {d, d + e});
  const HostTensor* lb = P.get("lang_proj.bias", {d});
  if (emb && lw && lb) {
    std::vector<float> rows((size_t)d * d), table((size_t)std::max(a.num_languages, 1) * d, 0.f);
    for (int n = 0; n < d; ++n) {
      for (int k = 0; k < d; ++k) rows[(size_t)n * d + k] = lw->data[(size_t)n * (d + e) + k];
      for (int l = 0; l < a.num_languages; ++l) {
        double acc = lb->data[n];
        for (int k = 0; k < e; ++k) acc += (double)lw->data[(size_t)n * (d + e) + d + k] * emb->data[(size_t)l * e + k];
        table[(size_t)l * d + n] = (float)acc;
      }
    }
    m->lang = P.pack(rows, d, d, nullptr);
    m->lang_table = P.upload(table);
  }
  if (a.enable_bilstm) {
    // nn.LSTM(d, d/2, num_layers, bidirectional): model.py:104-111.  Gate rows i|f|g|o (blocks of H) are reordered
    // unit-major / gate-minor for the recurrence kernel (lstm.hip); b_ih + b_hh fold into the projection bias.
    const int H = d / 2;
    m->lstm_U = wfl_lstm_units_per_wg(H);
    if ((m->lstm_U <= 0 || !wfl_lstm_hidden_supported(H)) && P.err.empty()) P.err = lstm_hidden_refusal(H);
    for (int layer = 0; layer < a.bilstm_layers && P.err.empty(); ++layer) {
      const int din = d;      // layer 0: encoder width d; deeper layers: 2H = d
      std::vector<float> rows((size_t)8 * H * din), bias((size_t)8 * H), whh_f((size_t)2 * 4 * H * H);
      std::vector<uint16_t> whh((size_t)2 * 4 * H * H), whh_lo((size_t)2 * 4 * H * H);
      for (int dir = 0; dir < 2; ++dir) {
        const std::string suf = "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
        const HostTensor* wih = P.get("bilstm.weight_ih" + suf, {4 * H, din});
        const HostTensor* whh_t = P.get("bilstm.weight_hh" + suf, {4 * H, H});
        const HostTensor* bih = P.get("bilstm.bias_ih" + suf, {4 * H});
        const HostTensor* bhh = P.get("bilstm.bias_hh" + suf, {4 * H});
        if (!wih || !whh_t || !bih || !bhh) break;
        for (int u = 0; u < H; ++u)
          for (int gate = 0; gate < 4; ++gate) {
            const int src = gate * H + u;
            const size_t dst = (size_t)dir * 4 * H + 4 * u + gate;
            memcpy(&rows[dst * din], &wih->data[(size_t)src * din], sizeof(float) * din);
            bias[dst] = bih->data[src] + bhh->data[src];
          }
        memcpy(&whh_f[(size_t)dir * 4 * H * H], whh_t->data.data(), sizeof(float) * 4 * H * H);
      }
      if (!P.err.empty()) break;
      if (wfl_op_lstm_pack_whh(whh_f.data(), H, m->lstm_U, whh.data(), whh_lo.data())) { P.err = g_err; break; }
      m->lstm_in.push_back(P.pack(rows, 8 * H, din, &bias));
      m->lstm_whh.push_back((bf16_t*)P.upload(whh));
      m->lstm_whh_lo.push_back((a.precision && wfl_lstm_split_precision_supported(H)) ? (bf16_t*)P.upload(whh_lo) : nullptr);
    }
  }
  m->conf.resize(a.n_conformer);
  const int x = a.conformer_ff_expansion, kk = a.conformer_kernel;
  for (int i = 0; i < a.n_conformer; ++i) {
    const std::string p = "conformer_layers." + std::to_string(i) + ".";
    ConfLayer& C = m->conf[i];
    C.ff1_ln = P.ln(p + "ff1.net.0", d);
    C.ff1_a = P.linear(p + "ff1.net.1", d * x, d);
    C.ff1_a_ln = P.linear_ln(p + "ff1.net.1", d * x, d, p + "ff1.net.0");
    C.ff1_b = P.linear(p + "ff1.net.4", d, d * x);
    C.ff2_ln = P.ln(p + "ff2.net.0", d);
    C.ff2_a = P.linear(p + "ff2.net.1", d * x, d);
    C.ff2_a_ln = P.linear_ln(p + "ff2.net.1", d * x, d, p + "ff2.net.0");
    C.ff2_b = P.linear(p + "ff2.net.4", d, d * x);
    const HostTensor* iw = P.get(p + "self_attn.in_proj_weight", {3 * d, d});
    const HostTensor* ib = P.get(p + "self_attn.in_proj_bias", {3 * d});
    if (iw && ib) {
      const int hd = m->dv / a.conformer_heads;              // (the true head size; padded columns are zero)
      const float qs = (float)(std::pow((double)hd, -0.5) * 1.4426950408889634);
      std::vector<float> rows(iw->data), bias(ib->data);
      for (size_t j = 0; j < (size_t)d * d; ++j) rows[j] *= qs;
      for (int j = 0; j < d; ++j) bias[j] *= qs;
      const int da = m->conf_da, hp = m->conf_hd, hv = d / a.conformer_heads;
      if (da == d) {
        C.qkv = P.pack(rows, 3 * d, d, &bias);
      } else {                                               // head h's rows move to [h * hp, h * hp + hv) of each da-wide block
        std::vector<float> prow((size_t)3 * da * d, 0.f), pbias((size_t)3 * da, 0.f);
        for (int b3 = 0; b3 < 3; ++b3)
          for (int c = 0; c < d; ++c) {
            const size_t dst = (size_t)b3 * da + (c / hv) * hp + c % hv;
            memcpy(&prow[dst * d], &rows[((size_t)b3 * d + c) * d], sizeof(float) * d);
            pbias[dst] = bias[(size_t)b3 * d + c];
          }
        C.qkv = P.pack(prow, 3 * da, d, &pbias);
      }
    }
    if (m->conf_da == d) {
      C.out = P.linear(p + "self_attn.out_proj", d, d);
    } else {
      const HostTensor* ow = P.get(p + "self_attn.out_proj.weight", {d, d});
      const HostTensor* ob = P.get(p + "self_attn.out_proj.bias", {d});
      if (ow && ob) {
        const int da = m->conf_da, hp = m->conf_hd, hv = d / a.conformer_heads;
        std::vector<float> prow((size_t)d * da, 0.f);
        for (int n = 0; n < d; ++n)
          for (int c = 0; c < d; ++c) prow[(size_t)n * da + (c / hv) * hp + c % hv] = ow->data[(size_t)n * d + c];
        C.out = P.pack(prow, d, da, &ob->data);
      }
    }
    C.ln1 = P.ln(p + "ln1", d);
    C.ln2 = P.ln(p + "ln2", d);
    // pointwise conv d -> 2d followed by GLU: interleave rows in groups of 16 (a | gate)
    const HostTensor* pw = P.get(p + "conv.0.weight", {2 * d, d, 1});
    const HostTensor* pb = P.get(p + "conv.0.bias", {2 * d});
    if (pw && pb) {
      std::vector<float> rows((size_t)2 * d * d), bias((size_t)2 * d);
      for (int gidx = 0; gidx < d / 16; ++gidx)
        for (int r = 0; r < 16; ++r) {
          const int ca = gidx * 16 + r, cg = d + gidx * 16 + r;
          const int ra = gidx * 32 + r, rg = gidx * 32 + 16 + r;
          memcpy(&rows[(size_t)ra * d], &pw->data[(size_t)ca * d], sizeof(float) * d);
          memcpy(&rows[(size_t)rg * d], &pw->data[(size_t)cg * d], sizeof(float) * d);
          bias[ra] = pb->data[ca];
          bias[rg] = pb->data[cg];
        }
      C.pw1 = P.pack(rows, 2 * d, d, &bias);
    }
    // dense k-tap conv with eval-mode BatchNorm folded in: y = (conv(x) - mean) * g / sqrt(var + eps) + beta
    const HostTensor* bw = P.get(p + "conv.3.weight", {d});
    const HostTensor* bb = P.get(p + "conv.3.bias", {d});
    const HostTensor* bm = P.get(p + "conv.3.running_mean", {d});
    const HostTensor* bvar = P.get(p + "conv.3.running_var", {d});
    if (m->host.count(p + "conv.3.num_batches_tracked")) P.used.insert(p + "conv.3.num_batches_tracked");
    if (bw && bb && bm && bvar) {
      std::vector<float> sc(d), sh(d);
      for (int c = 0; c < d; ++c) {
        sc[c] = bw->data[c] / std::sqrt(bvar->data[c] + 1e-5f);
        sh[c] = bb->data[c] - bm->data[c] * sc[c];
      }
      C.conv = P.conv(p + "conv.2", d, d, kk, &sc, &sh);
    }
    C.pw2 = P.conv(p + "conv.5", d, d, 1);
  }
  if (a.enable_dilated) {
    for (int i = 0; i < a.dilated_depth; ++i)
      m->dil.push_back(P.conv("dilated_conv_stack." + std::to_string(2 * i), d, d, a.dilated_kernel));
  }
  m->cls = P.linear("classifier", a.num_classes, d);
  // The classifier runs in split precision (its inputs are the residual stream's hi + lo halves, its weights hi + lo):
  // logits = [h_hi | h_lo] . [W_hi | W_hi]^T + h_hi . W_lo^T + b, three bf16 MFMA passes summed in fp32 -- 0.4 % of the forward's FLOPs
  // for a logit error a plain bf16 pass would double (tests/study_quant.py).
  if (const HostTensor* cw = P.get("classifier.weight", {a.num_classes, d})) {
    std::vector<float> lo((size_t)a.num_classes * d), hi2((size_t)a.num_classes * 2 * d), w3((size_t)a.num_classes * 3 * d);
    for (int n = 0; n < a.num_classes; ++n)
      for (int k = 0; k < d; ++k) {
        const float w = cw->data[(size_t)n * d + k];
        const uint32_t u = (uint32_t)f32_to_bf16_bits(w) << 16;
        float wh;
        memcpy(&wh, &u, 4);
        lo[(size_t)n * d + k] = w - wh;
        hi2[(size_t)n * 2 * d + k] = wh;
        hi2[(size_t)n * 2 * d + d + k] = wh;
        w3[(size_t)n * 3 * d + k] = wh;
        w3[(size_t)n * 3 * d + d + k] = wh;
        w3[(size_t)n * 3 * d + 2 * d + k] = w - wh;
      }
    const HostTensor* cb = P.get("classifier.bias", {a.num_classes});
    m->cls_lo = P.pack(lo, a.num_classes, d, nullptr);
    if (cb) m->cls_hi2 = P.pack(hi2, a.num_classes, 2 * d, &cb->data);
    if (cb && d % 64 == 0) m->cls3 = P.pack(w3, a.num_classes, 3 * d, &cb->data);
  }
  m->off1 = P.conv("boundary_offset_head.0", d, d, 3);
  const HostTensor* w2 = P.get("boundary_offset_head.2.weight", {2, d, 1});
  const HostTensor* b2 = P.get("boundary_offset_head.2.bias", {2});
  if (w2 && b2) {
    m->off_w2 = P.upload(w2->data);
    m->off_b2 = P.upload(b2->data);
  }
  return 0;
}

int32_t wfl_finalize(wfl_model* m) {
  if (!m) return fail(-1, "wfl_finalize: null model");
  if (m->finalized) return fail(-1, "wfl_finalize: already finalized");
  // a hidden size the recurrence has no kernel for is refused here, by name, and not by the first forward (before any device call)
  if (m->a.enable_bilstm && !wfl_lstm_hidden_supported(m->a.d_model / 2)) return fail(-2, "wfl_finalize: " + lstm_hidden_refusal(m->a.d_model / 2));
  Packer P{m};
  if (hipGetDevice(&m->device) != hipSuccess) return fail(-10, "wfl_finalize: hipGetDevice failed");
  if (m->a.encoder_type == WFL_ENC_WHISPER) finalize_whisper(m, P);
  else if (m->a.encoder_type == WFL_ENC_WAVLM) finalize_wavlm(m, P);
  else {
    // MelSpectrogram(f_min = 0, f_max = float(sample_rate // 2)): torchaudio's default f_max and melscale_fbanks' bin grid
    // linspace(0, sample_rate // 2, 201) both use the integer half
    const int sr = m->a.mel_sample_rate ? m->a.mel_sample_rate : 16000;
    build_frontend_tables(m, P, true, (double)(sr / 2));
    pad_head_state(m, P);
  }
  if (P.err.empty()) finalize_head(m, P);
  if (!P.err.empty()) return fail(-2, "wfl_finalize: " + P.err);
  for (auto& kv : m->host)
    if (!P.used.count(kv.first)) return fail(-2, "wfl_finalize: unexpected key in state_dict: " + kv.first);
  m->host.clear();
  m->avg_langs.clear();
  for (int i = 0; i < m->a.num_languages; ++i) m->avg_langs.push_back(i);
  m->finalized = true;
  return 0;
}

int32_t wfl_device(const wfl_model* m) { return m ? m->device : -1; }

int32_t wfl_set_average_languages(wfl_model* m, const int32_t* ids_host, int32_t n) {
  if (!m || !m->finalized) return fail(-1, "wfl_set_average_languages: model not finalized");
  if (!ids_host || n <= 0) return fail(-1, "wfl_set_average_languages: empty id list");
  for (int i = 0; i < n; ++i)
    if (ids_host[i] < 0 || ids_host[i] >= m->a.num_languages) return fail(-1, "wfl_set_average_languages: id out of range");
  m->avg_langs.assign(ids_host, ids_host + n);
  return 0;
}

// Every entry point that touches the device: the model's device must be the current one (a handle on GPU 1 driven with GPU 0
// current would dereference GPU-1 weight pointers from GPU-0 kernels).
static int check_device(const wfl_model* m, const char* who) {
  int d = -1;
  if (hipGetDevice(&d) != hipSuccess) return fail(-10, std::string(who) + ": hipGetDevice failed");
  if (d != m->device)
    return fail(-11, std::string(who) + ": the model lives on HIP device " + std::to_string(m->device) + " but device " +
                         std::to_string(d) + " is current (call hipSetDevice / torch.cuda.set_device first)");
  return 0;
}

// ------------------------------------------------------------------------------------------------ workspace plan
namespace {

// The bf16 activation buffers of the workspace: frame rows [lead | B clips of P rows, the first T of each its frames | tail].
// make_plan declares each of them once, as an ActBuf of Plan::bufs; the Runner reads offsets, geometry and low halves from there.
enum Buf { BUF_X, BUF_Y, BUF_ATT, BUF_QK, BUF_FF, BUF_MEL, BUF_C1, BUF_ENC2, BUF_QKP, BUF_ATTP, BUF_FA, BUF_FB, BUF_XG, BUF_COUNT };

struct ActBuf {
  long off, bytes;      // 0 bytes: not allocated for this model
  int width;            // elements per row
  int lead, P, T;       // row geometry (FA / FB: of level 0 / level 1, the first level each of them holds)
  long tail;            // rows behind the last clip's pitch that the halo kernel clears
  long lo;              // byte offset of the low half, -1: none.  Default mode: X and Y have one (the residual stream, GemmArgs::res_lo);
                        // "model.precision: high": every buffer, lo_delta bytes further on
  long span;            // a pointer less than `span` bytes behind `off` names this buffer (Runner::lo_idx).  Default mode: one row of
                        // X / Y, i.e. a column offset is allowed and a row offset is not; precision high: the whole buffer
};

struct Plan {
  int B, L, T, P, lead, tail;
  int T2, P2, lead2;            // whisper stem input rows (mel frames)
  long R, R2;
  int d, ffw;
  // wavlm feature-encoder levels: level i = output of conv layer i (frames T_i, pitch P_i = P * 2^(n-1-i), lead 8)
  int nlev, Tl[8], Pl[8], leadl[8];
  long Rl[8];
  ActBuf bufs[BUF_COUNT];
  // byte offsets of the single-use slots
  long stats, raw, clipmax, logits, logits2, offs2, gx, lstm_x;
  long gate, rtab, wstats, cstats, cpart, err, clipT, total;
  long X8, FF8, rs8;            // fp8 activations (fp8_weights models): e4m3 rows [R][d], [R][ffw], fp32 row scales [R]
  long X8lo, FF8lo;             //   and their lo planes (e4m3 pairs, gemm_mx.hip)
  long lo_delta, hp32;          // "model.precision: high": every activation buffer has its low half lo_delta bytes further on (a twin of
  long hp32_floats;             //   the whole activation area); hp32 = the fp32 sums of the three passes, [rows][columns]
  int da;                       // Conformer attention width (wfl_model::conf_da); QKp / ATTp exist when it differs from d
};

static int wavlm_frames(const wfl_arch& a, int L) {
  long t = L;
  for (int i = 0; i < a.wavlm_n_conv; ++i) {
    if (t < a.wavlm_conv_kernel[i]) return 0;
    t = (t - a.wavlm_conv_kernel[i]) / a.wavlm_conv_stride[i] + 1;
  }
  return (int)t;
}

// T_frames > 0: a head-only plan over that many frames per clip (wfl_head): no encoder-side buffers.
static Plan make_plan(const wfl_model* m, int B, int L, int T_frames = 0) {
  const wfl_arch& a = m->a;
  const bool whisper = a.encoder_type == WFL_ENC_WHISPER;
  Plan p{};
  p.B = B; p.L = L;
  const bool none = a.encoder_type == WFL_ENC_NONE;
  p.T = T_frames > 0 ? T_frames : (whisper ? a.max_positions : (none ? 1 + L / a.mel_hop : wavlm_frames(a, L)));
  p.P = (int)round_up(p.T + m->halo, 8);
  p.lead = m->halo;
  p.tail = 256;
  p.T2 = 2 * p.T; p.P2 = 2 * p.P; p.lead2 = 8;
  p.R = p.lead + (long)B * p.P + p.tail;
  p.R2 = p.lead2 + (long)B * p.P2 + 2 * p.tail;
  p.d = a.d_model;
  p.ffw = std::max(a.enc_ffn, a.d_model * std::max(a.conformer_ff_expansion, 1));
  long off = 0;
  auto take = [&](long bytes) { long o = off; off = round_up(off + bytes, 256); return o; };
  // the only writer of Plan::bufs: one call per buffer, in allocation order (lo and span follow below, once the low halves are placed)
  auto take_buf = [&](Buf b, long bytes, int width, int lead, int P, int T, long tail) {
    p.bufs[b] = {take(bytes), bytes, width, lead, P, T, tail, -1, 0};
  };
  auto take_rows = [&](Buf b, int width) { take_buf(b, p.R * width * 2, width, p.lead, p.P, p.T, p.tail); };   // the main geometry
  if (T_frames > 0) {
  } else if (whisper) {
    take_buf(BUF_MEL, p.R2 * a.n_mels * 2 + 1024, a.n_mels, p.lead2, p.P2, p.T2, 2 * p.tail);
    take_buf(BUF_C1, p.R2 * p.d * 2, p.d, p.lead2, p.P2, p.T2, 2 * p.tail);
    p.raw = take((long)B * p.T2 * a.n_mels * 4);
  } else if (none) {
    p.raw = take((long)B * p.T * a.n_mels * 4);        // the mel power = the hidden states, fp32 [B][T][n_mels]
  } else {
    const int n = a.wavlm_n_conv, C = a.wavlm_conv_dim[0];
    p.nlev = n;
    long t = L;
    for (int i = 0; i < n; ++i) {
      t = t >= a.wavlm_conv_kernel[i] ? (t - a.wavlm_conv_kernel[i]) / a.wavlm_conv_stride[i] + 1 : 0;
      p.Tl[i] = (int)t;
    }
    for (int i = n - 1; i >= 0; --i) {
      p.Pl[i] = i == n - 1 ? p.P : p.Pl[i + 1] * 2;
      p.leadl[i] = i == n - 1 ? p.lead : 8;
      p.Rl[i] = p.leadl[i] + (long)B * p.Pl[i] + p.tail;
    }
    take_buf(BUF_FA, p.Rl[0] * C * 2, C, p.leadl[0], p.Pl[0], p.Tl[0], p.tail);   // levels 0, 2, 4, 6
    take_buf(BUF_FB, p.Rl[1] * C * 2, C, p.leadl[1], p.Pl[1], p.Tl[1], p.tail);   // levels 1, 3, 5
    take_buf(BUF_XG, (long)a.wavlm_pos_conv_groups * p.R * 64 * 2, 64, p.lead, p.P, p.T, p.tail);   // per group: R rows of 64 channels
    p.gate = take((long)B * a.enc_heads * p.T * 4);
    p.rtab = take((long)a.enc_heads * (2L * p.T + 1) * 4);
    p.wstats = take((long)B * 2 * 8);
    p.cstats = take((long)B * C * 2 * 8);
    p.cpart = take(a.wavlm_group_norm ? (long)B * ((p.Tl[0] + 511) / 512) * C * 2 * 4 : 16);   // GroupNorm partials per 512-step block
  }
  take_rows(BUF_X, p.d);
  take_rows(BUF_Y, p.d);
  const long Xlo = take(p.R * p.d * 2);                 // low halves of the residual stream (GemmArgs::res_lo)
  const long Ylo = take(p.R * p.d * 2);
  take_rows(BUF_ATT, p.d);
  take_rows(BUF_QK, 3 * p.d);                           // packed q | k | v rows
  take_rows(BUF_FF, p.ffw);
  p.da = m->conf_da > 0 ? m->conf_da : p.d;
  if (p.da != p.d) {
    take_rows(BUF_QKP, 3 * p.da);
    take_rows(BUF_ATTP, p.da);
  }
  if (a.fp8_weights && T_frames <= 0) {
    p.X8 = take(p.R * (long)p.d);
    p.FF8 = take(p.R * (long)p.ffw);
    p.rs8 = take(p.R * 4L);
    p.X8lo = take(p.R * (long)p.d);
    p.FF8lo = take(p.R * (long)p.ffw);
  }
  p.stats = take(p.R * 4L * 2 * 4);                     // per row, per 256-column tile (<= 4): (sum, sum of squares)
  take_rows(BUF_ENC2, p.d);
  p.clipmax = take((long)B * 4);
  p.logits = take((long)B * p.T * round_up(a.num_classes, 4) * 4);      // (rows of a multiple of four floats when the caller does not ask for them)
  p.logits2 = take((long)B * p.T * a.num_classes * 4);
  p.offs2 = take((long)B * p.T * 2 * 4);
  p.gx = p.lstm_x = 0;
  if (a.enable_bilstm) {
    p.gx = take(p.R * 4L * p.d * 4);                       // fp32 [rows][8H]
    p.lstm_x = take(wfl_lstm_exchange_bytes(p.d / 2, B));
  }
  p.clipT = take(8L * B * 4);                            // per-clip frame counts per front-end level (ragged batches), [level][B]
  p.err = take(256);                                     // the forward's device-side error word
  if (a.precision) {
    p.lo_delta = round_up(off, 256);
    off = 2 * p.lo_delta;                                // the twin
    long rows = std::max(p.R2, p.R);
    for (int i = 1; i < p.nlev; ++i) rows = std::max(rows, p.Rl[i]);                       // (WavLM: the feature encoder's levels are GEMM outputs too)
    const long cols = std::max<long>(std::max<long>(3L * std::max(p.d, p.da), 2L * p.ffw), 1024);
    p.hp32_floats = rows * cols;
    p.hp32 = take(p.hp32_floats * 4);
    for (ActBuf& b : p.bufs)
      if (b.bytes) { b.lo = b.off + p.lo_delta; b.span = b.bytes; }
  } else {
    p.bufs[BUF_X].lo = Xlo;
    p.bufs[BUF_Y].lo = Ylo;
    p.bufs[BUF_X].span = p.bufs[BUF_Y].span = (long)p.d * 2;
  }
  p.total = off;
  return p;
}

}  // namespace

int32_t wfl_num_frames(const wfl_model* m, int32_t L) {
  if (!m) return -1;
  if (m->a.encoder_type == WFL_ENC_NONE) return L > 200 ? 1 + L / m->a.mel_hop : 0;    // (reflect padding needs L > n_fft / 2)
  return m->a.encoder_type == WFL_ENC_WHISPER ? m->a.max_positions : wavlm_frames(m->a, L);
}

int64_t wfl_workspace_bytes(const wfl_model* m, int32_t B, int32_t L) {
  if (!m || B <= 0) return -1;
  return make_plan(m, B, L).total;
}

// ------------------------------------------------------------------------------------------------ forward
namespace {

// Keys of the non-GEMM kernel families in the launch profile (wfl_gemm_profile_read; GEMM variants have keys below 2040)
enum { PROF_ATTENTION = 2040, PROF_LSTM = 2041, PROF_LOGMEL = 2042, PROF_LAYERNORM = 2043, PROF_POSCONV = 2044 };

// One Runner::gemm() call: C = epilogue(A W^T + b) over the rows, with the options the caller names.
struct GemmRows { int M, P, T; };                              // M = B * P rows; the first T of every P are a clip's frames
struct GemmOut { void* C; long ldc, c_lead; int c_pitch; };    // row b * P + t of the product goes to row c_lead + b * c_pitch + t of C
struct GemmOpts {
  int act = WFL_ACT_NONE;
  const bf16_t* res = nullptr;  // residual: C = res + alpha * act(A W^T + b)
  long ldres = 0;
  float alpha = 1.f;
  int cin = 0;                  // > 0: K holds K / cin taps of cin channels, tap_stride elements apart (GemmArgs::cin)
  long tap_stride = 0;
  bool glu = false;
  bool out_f32 = false;
  const bf16_t* pos = nullptr;  // positional table [T][ldpos], added after the activation
  long ldpos = 0;
  const float* clip_bias = nullptr;   // per-clip bias rows clip_bias[clip_idx[b] * clip_ld + n]
  const int* clip_idx = nullptr;
  int clip_ld = 0;
  bool want_stats = false;      // a residual launch that feeds a LayerNorm-folded GEMM: emit the row statistics if this launch can
  bool lo_out = false;          // the output is a residual-stream tensor: keep its low half
  bool acc_f32 = false;         // (fp32 output) add to what is there
  double flops = -1.0;          // >= 0: algorithmic FLOPs to book instead of 2 M N K
  int tap_wrap = 0;             // K holds three tap segments (GemmArgs::tap_wrap / seg_off)
  long seg_off = 0;
  // fp8 activations (GemmArgs::a8): the A operand is e4m3 bytes with these scales ...
  int a8 = 0;                   // 0 off, 1 gemm_stream A8, 2 / 3 gemm_mx single / pair
  const float* a8_scale = nullptr;
  float a8_static = 1.f;
  const unsigned char* a8_lo = nullptr;     // pair input (a8 == 3)
  // ... and the output goes out as e4m3 too (gemm_mx.hip: c8_lo for a pair)
  unsigned char* c8 = nullptr;
  unsigned char* c8_lo = nullptr;
  long ldc8 = 0;
  float c8_inv = 1.f;
  bool stats_in = false;        // (ln_gemm) a folded operand reads the statistics the last residual launch left behind
};

struct Runner {
  wfl_model* m;
  Plan p;
  char* ws;
  hipStream_t s;
  int rc = 0;

  bf16_t* act(Buf b) const { return (bf16_t*)(ws + p.bufs[b].off); }
  // the first frame row of rows `width` elements wide in the main geometry / of a buffer in its own
  template <class T> T* rows(T* ptr, long width) const { return ptr + (long)p.lead * width; }
  bf16_t* rows(Buf b) const { return act(b) + (long)p.bufs[b].lead * p.bufs[b].width; }
  // Ragged batches (WavLM / mel front-ends with per-clip lengths): clipT = [B] frames of every clip at the encoder's rate,
  // levelT[i] = the same at level i of the WavLM conv stack (both in the workspace, written by clip_frames_kernel); null otherwise.
  // Every kernel that stores frame rows skips rows t >= clipT[b]; the shared buffers are zeroed whole at the start of the forward,
  // so those rows stay zero like the halo rows do, and what a clip sees is exactly what it sees when it is labelled alone.
  const int* clipT = nullptr;
  const int* levelT[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int* clip_T_for(int P) const {
    if (!clipT) return nullptr;
    if (P == p.P) return clipT;
    for (int i = 0; i < p.nlev; ++i) if (p.Pl[i] == P) return levelT[i];
    return nullptr;
  }
  // Residual stream hi + lo (common.h, GemmArgs::res_lo): X and Y have low halves; lo_ok says whether the low half of the
  // tensor currently held in X / Y is valid (a kernel that writes only the high half invalidates it).
  // "model.precision: high" (precise.hip): EVERY activation buffer has a low half, lo_delta bytes further on, and lo_ok tracks the
  // buffers whose producer wrote it (one flag per Buf).  Which pointers name a buffer, and where its low half lies: ActBuf::span, lo
  bool precise() const { return m->a.precision != 0 && p.lo_delta > 0; }
  bool lo_ok[BUF_COUNT] = {};
  int lo_idx(const void* ptr) const {               // the buffer `ptr` names, or -1 (a buffer without a low half has no span)
    const long o = (const char*)ptr - ws;
    for (int i = 0; i < BUF_COUNT; ++i)
      if (o >= p.bufs[i].off && o < p.bufs[i].off + p.bufs[i].span) return i;
    return -1;
  }
  bf16_t* lo_of(const void* ptr) const {
    const int i = lo_idx(ptr);
    return i < 0 ? nullptr : (bf16_t*)((char*)ptr + (p.bufs[i].lo - p.bufs[i].off));
  }
  const bf16_t* lo_in(const void* ptr) const { const int i = lo_idx(ptr); return (i >= 0 && lo_ok[i]) ? lo_of(ptr) : nullptr; }
  void mark_lo(const void* ptr, bool valid) { const int i = lo_idx(ptr); if (i >= 0) lo_ok[i] = valid; }   // the producer of `ptr` did / did not write its low half
  // LayerNorm statistics left behind by the last residual GEMM (gemm_stream.hip, STATS): valid for the rows of `stats_for`
  const void* stats_for = nullptr;
  int stats_nsl = 0;

  GemmOut out(void* C, long ldc) const { return {C, ldc, p.lead, p.P}; }        // rows in the main geometry

  // What every launch of a Linear / Conv-as-GEMM has in common; the callers below set what differs (operand halves, W_lo / W3, the
  // fp32 accumulator, the fp8 and LayerNorm-fold fields)
  GemmArgs gemm_args(const bf16_t* A, long lda, const Lin& W, const GemmRows& r, const GemmOut& c, const GemmOpts& o) const {
    GemmArgs g{};
    g.A = A; g.lda = lda;
    g.cin = o.cin > 0 ? o.cin : W.K; g.tap_stride = o.tap_stride;
    g.W = W.W; g.M = r.M; g.N = W.N; g.K = W.K; g.n_valid = W.n_valid;
    g.P = r.P; g.T = r.T; g.clip_T = clip_T_for(r.P);
    g.C = c.C; g.ldc = c.ldc; g.c_lead = c.c_lead; g.c_pitch = c.c_pitch;
    g.bias = W.bias; g.clip_bias = o.clip_bias; g.clip_idx = o.clip_idx; g.clip_ld = o.clip_ld;
    g.res = o.res; g.ldres = o.ldres; g.alpha = o.alpha;
    g.pos = o.pos; g.ldpos = o.ldpos;
    g.act = o.act; g.glu = o.glu ? 1 : 0; g.out_f32 = o.out_f32 ? 1 : 0;
    g.ln_eps = 1e-5f;
    return g;
  }
  // One pass of a product summed in fp32: A W^T alone -- no bias, no epilogue -- of the same taps
  static GemmOpts partial_product(const GemmOpts& o) { return {.cin = o.cin, .tap_stride = o.tap_stride, .out_f32 = true}; }

  void gemm(const bf16_t* A, long lda, const Lin& W, const GemmRows& r, const GemmOut& c, const GemmOpts& o = {}) {
    if (rc) return;
    if (precise() && !o.out_f32 && !W.w8 && !o.a8 && W.W_lo) {
      gemm_precise(A, lda, W, r, c, o);
      return;
    }
    bool acc_f32 = o.acc_f32;
    if (precise() && o.out_f32 && !acc_f32 && o.act == WFL_ACT_NONE && W.W_lo && !W.w8 && !o.glu && !o.res && !o.pos && !o.clip_bias &&
        !W.ln_s && o.tap_wrap == 0) {
      // fp32 output (the BiLSTM's input projection): the two correction passes first -- A_hi W_lo^T, then A_lo W_hi^T added to it, no
      // bias -- and the plain launch below adds A_hi W_hi^T + b to them (which books the product: these two are not timed)
      const bf16_t* A_lo = lo_in(A);
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !A_lo) break;
        GemmArgs g = gemm_args(pass == 1 ? A_lo : A, lda, W, r, c, partial_product(o));
        g.W = pass == 0 ? W.W_lo : W.W; g.bias = nullptr; g.acc_f32 = pass;
        const int e = wfl_launch_gemm(g, s);
        if (e) { rc = fail(e, "gemm launch failed (precision high, fp32 output, pass " + std::to_string(pass) + ")"); return; }
      }
      acc_f32 = true;
    }
    GemmArgs g = gemm_args(A, lda, W, r, c, o);
    g.ln_s = W.ln_s;
    g.w8_scale = W.w8;
    if (W.ln_s && o.stats_in) { g.stats_in = (const float*)(ws + p.stats); g.stats_nsl = stats_nsl; g.stats_lead = p.lead; }
    g.tap_wrap = o.tap_wrap; g.seg_off = o.seg_off;
    g.acc_f32 = (o.out_f32 && acc_f32) ? 1 : 0;
    if (o.a8) {
      g.a8 = o.a8; g.a8_lo = o.a8_lo; g.a8_scale = o.a8_scale; g.a8_lead = p.lead; g.a8_static = o.a8_static;
      g.c8 = o.c8; g.c8_lo = o.c8_lo; g.ldc8 = o.ldc8; g.c8_inv_scale = o.c8_inv;
      g.err = (unsigned*)(ws + p.err);
    }
    if (!o.out_f32 && !o.glu && (o.res || o.lo_out)) g.c_lo = lo_of(c.C);
    if (o.res) g.res_lo = lo_in(o.res);
    if (!o.out_f32) mark_lo(c.C, g.c_lo != nullptr);
    if (c.C == stats_for) stats_for = nullptr;                     // the rows they describe are being overwritten
    // want_stats is a request: a launch that cannot emit the statistics runs without them, and the consumer's LayerNorm stays a kernel
    if (o.want_stats && o.res && !o.out_f32 && !o.glu && o.act == WFL_ACT_NONE && c.ldc == p.d && W.n_valid == p.d && c.c_lead == p.lead &&
        c.c_pitch == p.P && r.P == p.P && ln_fold_mode() == 1 && !W.w8) {
      g.stats_out = (float*)(ws + p.stats);
      if (wfl_gemm_stream_takes(g)) { stats_for = c.C; stats_nsl = W.N / 256; }
      else g.stats_out = nullptr;
    }
    launch_timed(g, o.flops >= 0.0 ? o.flops : 2.0 * (double)(r.M / r.P) * r.T * (double)W.n_valid * (double)W.K, "");
  }

  // "model.precision: high": the same Linear / Conv1d as three bf16 passes over split operands, summed in fp32, then the layer's
  // epilogue as its own kernel (precise.hip).  A's low half is used when its producer wrote it (lo_ok).  Both halves of the output are
  // always kept and the FLOPs of the passes are booked as they are: o.want_stats, o.lo_out and o.flops are not read.
  void gemm_precise(const bf16_t* A, long lda, const Lin& W, const GemmRows& r, const GemmOut& c, const GemmOpts& o) {
    void* const C = c.C;
    if (C == stats_for) stats_for = nullptr;
    const int B = r.M / r.P;
    const bf16_t* A_lo = lo_in(A);
    // One launch instead of three + the finish kernel, whenever the operand has its low half and the fused epilogues can do what the
    // layer needs: K' = 3 K with the weights packed [W_hi | W_hi | W_lo] against the taps [A_hi | A_lo | A_hi] (GemmArgs::tap_wrap; the
    // low half of A is lo_delta away), the accumulator never leaves the registers, the epilogue writes hi AND lo.  WFL_PRECISE_FUSED=0
    // keeps the three-launch form (A/B runs); the positional-table launch (the Whisper stem's conv2) joined it in round 4 (below).
    static int fused_on = -1;
    if (fused_on < 0) { const char* e = getenv("WFL_PRECISE_FUSED"); fused_on = e ? atoi(e) : 1; }
    static int pos_fused = -1;                          // WFL_PRECISE_POS_FUSED=0: the table launch in the three-launch form (A/B runs)
    if (pos_fused < 0) { const char* e = getenv("WFL_PRECISE_POS_FUSED"); pos_fused = e ? atoi(e) : 1; }
    if (fused_on && W.W3 && A_lo && lo_of(C)) {
      GemmArgs g = gemm_args(A, lda, W, r, c, o);
      g.tap_wrap = W.K / g.cin; g.seg_off = (long)(A_lo - A);
      g.W = W.W3; g.K = 3 * W.K;
      g.res_lo = o.res ? lo_in(o.res) : nullptr;
      g.c_lo = lo_of(C);
      // the positional-table launch (the Whisper stem's conv2): one launch too when the slice-by-slice walk takes it -- its epilogue adds
      // the table as a pair; any other kernel would drop the low half, so those shapes keep the three-launch form below
      if (o.pos) g.pos_lo = (o.pos == m->pos) ? m->pos_lo : nullptr;
      if (!o.pos || (pos_fused && g.pos_lo && !o.glu && wfl_gemm256_tri_takes(g) && !wfl_gemm_stream_takes(g))) {
        mark_lo(C, true);
        launch_timed(g, 3.0 * 2.0 * (double)B * r.T * (double)W.n_valid * (double)W.K, "precision high, one-launch form: ");
        return;
      }
    }
    if ((long)r.M * W.N > p.hp32_floats) { rc = fail(-1, "precision high: the fp32 accumulator is too small for this launch"); return; }
    float* acc = (float*)(ws + p.hp32);
    for (int pass = 0; pass < 3; ++pass) {
      if (pass == 2 && !A_lo) break;
      GemmArgs g = gemm_args(pass == 2 ? A_lo : A, lda, W, r, {acc, W.N, 0, r.P}, partial_product(o));
      g.W = pass == 1 ? W.W_lo : W.W; g.n_valid = W.N; g.bias = nullptr; g.acc_f32 = pass > 0 ? 1 : 0;
      if (!launch_timed(g, 2.0 * (double)B * r.T * (double)W.n_valid * (double)W.K, "precision high, pass " + std::to_string(pass) + ": "))
        return;
    }
    PreciseFinishArgs f{};
    f.acc = acc; f.ld_acc = W.N; f.B = B; f.P = r.P; f.T = r.T;
    f.glu = o.glu ? 1 : 0;
    f.n_out = o.glu ? W.n_valid / 2 : W.n_valid;
    f.bias = W.bias; f.clip_bias = o.clip_bias; f.clip_idx = o.clip_idx; f.clip_ld = o.clip_ld;
    f.act = o.act; f.alpha = o.alpha; f.pos = o.pos; f.ldpos = o.ldpos;
    f.pos_lo = (o.pos && o.pos == m->pos) ? m->pos_lo : nullptr;
    f.res = o.res; f.res_lo = o.res ? lo_in(o.res) : nullptr; f.ldres = o.ldres;
    f.out = (bf16_t*)C; f.out_lo = lo_of(C); f.ldc = c.ldc; f.c_lead = c.c_lead; f.c_pitch = c.c_pitch;
    f.clip_T = clip_T_for(r.P);
    mark_lo(C, f.out_lo != nullptr);
    if (f.n_out % 8) { rc = fail(-1, "precision high: output width must be a multiple of 8"); return; }
    const int e = wfl_launch_precise_finish(f, s);
    if (e) rc = fail(e, "precise_finish launch failed");
  }

  // WFL_LN_FOLD: 1 (default) fold a LayerNorm into the GEMM that consumes it whenever the GEMM that produced its input left
  // the row statistics behind; 2 fold always, summing the statistics inside the consumer (slower: tools/gemm_lab.py qkvLN);
  // 0 never (LayerNorm kernel + plain GEMM).
  static int ln_fold_mode() {
    static int mode = -1;
    if (mode < 0) { const char* e = getenv("WFL_LN_FOLD"); mode = e ? atoi(e) : 1; }
    return mode;
  }
  // y = act(LayerNorm(x) W^T + b)
  void ln_gemm(const bf16_t* x, bf16_t* scratch, const LNp& w, const Lin& plain, const Lin& folded, int M, void* C, long ldc,
               int act) {
    if (rc) return;
    const int mode = (m->dv != p.d || precise()) ? 0 : ln_fold_mode();   // (the folded form divides by K: not for a zero-padded width;
                                                                          //  precision high: the LayerNorm kernel writes hi + lo)
    if (folded.ln_s && (mode == 2 || (mode == 1 && stats_for == x))) {
      GemmArgs g{};
      g.M = M; g.N = folded.N; g.K = folded.K; g.cin = folded.K; g.n_valid = folded.n_valid; g.act = act; g.ln_s = folded.ln_s;
      if (mode == 1) { g.stats_in = (const float*)(ws + p.stats); g.stats_nsl = stats_nsl; }
      if (wfl_gemm_stream_takes(g)) {
        gemm(rows(x, p.d), p.d, folded, {M, p.P, p.T}, out(C, ldc), {.act = act, .stats_in = mode == 1});
        return;
      }
    }
    ln(x, scratch, w);
    gemm(rows(scratch, p.d), p.d, plain, {M, p.P, p.T}, out(C, ldc), {.act = act});
  }

  // lo_out: the output is (or may become) a residual-stream tensor -- keep its low half; the input's low half is read when valid
  void ln(const bf16_t* x, bf16_t* y, const LNp& w, bool lo_out = false) {
    if (rc) return;
    if (y == stats_for) stats_for = nullptr;
    const bf16_t* x_lo = lo_in(x);
    bf16_t* y_lo = (lo_out || precise()) ? lo_of(y) : nullptr;
    mark_lo(y, y_lo != nullptr);
    prof_begin();
    const int r = wfl_launch_layernorm_act(x, p.d, y, p.d, w.g, w.b, 1e-5f, p.lead, p.B, p.P, p.T, p.d, 0, s, x_lo, y_lo, m->dv, clipT);
    prof_end(PROF_LAYERNORM, 0.0);
    if (r) rc = fail(r, "layernorm launch failed");
  }

  // y1 = LN_w1(x) kept as a residual-stream tensor (hi + lo), y2 = LN_w2(y1): what ln(x, y1, w1, true); ln(y1, y2, w2) compute, bit for
  // bit, in one launch and one pass over the rows (norm.hip, layernorm_pair_kernel).  y2 may be x.
  void ln_pair(const bf16_t* x, bf16_t* y1, const LNp& w1, bf16_t* y2, const LNp& w2) {
    if (rc) return;
    if (y1 == stats_for || y2 == stats_for) stats_for = nullptr;
    const bf16_t* x_lo = lo_in(x);
    bf16_t* y1_lo = lo_of(y1);
    bf16_t* y2_lo = precise() ? lo_of(y2) : nullptr;
    mark_lo(y1, y1_lo != nullptr);
    mark_lo(y2, y2_lo != nullptr);
    prof_begin();
    const int r = wfl_launch_layernorm_pair(x, x_lo, y1, y1_lo, y2, y2_lo, p.d, w1.g, w1.b, w2.g, w2.b, 1e-5f, p.lead, p.B, p.P, p.T, p.d,
                                            m->dv, clipT, s);
    prof_end(PROF_LAYERNORM, 0.0);
    if (r) rc = fail(r, "layernorm launch failed");
  }

  // Timing hook: prof_begin() takes the next event pair (created on demand) and records its first event, prof_end() records the second
  // and books the launch under its key -- a GEMM variant's (launch_timed) or a PROF_* family's
  hipEvent_t prof_e1 = nullptr;
  void prof_begin() {
    prof_e1 = nullptr;
    if (!m->prof_on || rc) return;
    if (m->prof_used >= m->prof.ev.size()) {
      hipEvent_t a_, b_;
      if (hipEventCreate(&a_) != hipSuccess || hipEventCreate(&b_) != hipSuccess) { rc = fail(-10, "hipEventCreate"); return; }
      m->prof.ev.push_back({a_, b_});
    }
    (void)hipEventRecord(m->prof.ev[m->prof_used].first, s);
    prof_e1 = m->prof.ev[m->prof_used].second;
    ++m->prof_used;
  }
  void prof_end(int key, double flops) {
    if (!prof_e1) return;
    (void)hipEventRecord(prof_e1, s);
    m->prof.key.push_back(key);
    m->prof.launches[key] += 1;
    m->prof.flops[key] += flops;
    prof_e1 = nullptr;
  }
  // wfl_launch_gemm, timed and booked under the key of the kernel variant that took it (GemmProf); false, and rc set, when it failed
  bool launch_timed(const GemmArgs& g, double flops, const std::string& what) {
    prof_begin();
    if (rc) return false;
    const int e = wfl_launch_gemm(g, s);
    prof_end((g.act & 3) | (g.glu ? 4 : 0) | (g.out_f32 ? 8 : 0) | (g.res ? 16 : 0) | ((g_wfl_gemm_kernel_id & 7) << 5) |
             ((g.ln_s ? (g.stats_in ? 2 : 1) : 0) << 8) | (g.stats_out ? 1024 : 0), flops);
    if (e) rc = fail(e, "gemm launch failed (" + what + std::to_string(e) + ")");
    return !e;
  }

  // padded: the Conformer attention at width p.da != p.d (head size rounded up to a built one): q | k | v rows in QKp, context in ATTp
  void attn(int heads, const float* bias = nullptr, const float* gate = nullptr, bool padded = false, unsigned char* o8 = nullptr,
            long ldo8 = 0, float o8_scale = 1.f, unsigned char* o8_lo = nullptr) {
    if (rc) return;
    AttnArgs a{};
    a.bias = bias; a.gate = gate;
    a.O8 = o8; a.O8_lo = o8_lo; a.ldo8 = ldo8; a.o8_scale = o8_scale;
    a.err = (unsigned*)(ws + p.err);
    bf16_t* ctx = act(padded ? BUF_ATTP : BUF_ATT);
    if (precise() && !o8) {                               // the context's low half for the out-projection's third pass
      a.O_lo = lo_of(ctx);
      mark_lo(ctx, a.O_lo != nullptr);
    }
    const int w = padded ? p.da : p.d;
    bf16_t* qk = act(padded ? BUF_QKP : BUF_QK);
    static const bool split_attn = std::getenv("WFL_SPLIT_ATTN") == nullptr;       // (set to anything: bf16 q, k, v, P in precision high -- A/B runs)
    if (precise() && !o8 && split_attn)
      if (const bf16_t* ql = lo_in(qk)) { a.QK_lo = ql; a.V_lo = ql + 2 * w; }     // q | k | v as hi + lo (their projection wrote both halves)
    a.QK = qk; a.ldqk = 3 * w; a.lead = p.lead; a.V = qk + 2 * w; a.ldv = 3 * w; a.O = ctx; a.ldo = w;
    a.B = p.B; a.T = p.T; a.P = p.P; a.heads = heads; a.d = w;
    a.clip_T = clipT;
    prof_begin();
    const int r = wfl_launch_attention(a, s);
    prof_end(PROF_ATTENTION, 4.0 * (double)p.B * p.T * (double)p.T * (double)p.d);
    if (r) rc = fail(r, "attention launch failed (" + std::to_string(r) + "; head_dim " + std::to_string(w / heads) + ")");
  }

  ZeroMulti zm{};
  void zero_add(Buf b, bool lo_half) {               // the halo rows of a buffer (of its low half); queued, zero_flush() launches once
    const ActBuf& a = p.bufs[b];
    const int k = zm.n++;
    zm.buf[k] = ws + (lo_half ? a.lo : a.off); zm.ld_bytes[k] = (long)a.width * 2; zm.lead[k] = a.lead; zm.P[k] = a.P; zm.T[k] = a.T;
    zm.tail_rows[k] = (long)(a.P - a.T) + a.tail;
  }
  void zero_flush() {
    if (rc || zm.n == 0) return;
    zm.B = p.B;
    const int r = wfl_launch_zero_halo_multi(zm, s);
    zm.n = 0;
    if (r) rc = fail(r, "zero_halo launch failed");
  }

  void zero(bf16_t* b, long ld_elems, long lead, int P, int T, long tail) {
    if (rc) return;
    // `tail` = rows behind the last clip's pitch; the kernel counts from the last clip's last valid frame
    const int r = wfl_launch_zero_halo(b, ld_elems * 2, lead, p.B, P, T, (long)(P - T) + tail, s);
    if (r) rc = fail(r, "zero_halo launch failed");
  }
};

}  // namespace

static int run_logmel(wfl_model* m, const Plan& p, char* ws, const float* wav, long ldw, const int* lens, float* ref_out,
                      hipStream_t s) {
  LogmelArgs a{};
  a.wav = wav; a.ldw = ldw; a.lens = lens; a.L = p.L; a.B = p.B;
  a.n_frames = p.T2; a.n_samples = p.T2 * 160; a.n_mels = m->a.n_mels;
  a.Wc = m->Wc; a.Ws = m->Ws; a.mel_lo = m->mel_lo; a.mel_cnt = m->mel_cnt; a.mel_w = m->mel_w; a.mel_maxw = m->mel_maxw;
  a.raw = (float*)(ws + p.raw); a.clipmax = (unsigned*)(ws + p.clipmax);
  const ActBuf& mel = p.bufs[BUF_MEL];
  return wfl_launch_logmel(a, (bf16_t*)(ws + mel.off), mel.width, mel.lead, mel.P, ref_out, s, mel.lo >= 0 ? (bf16_t*)(ws + mel.lo) : nullptr);
}

int32_t wfl_logmel(wfl_model* m, const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, float* out,
                   void* workspace, int64_t workspace_bytes, void* stream) {
  if (!m || !m->finalized) return fail(-1, "wfl_logmel: model not finalized");
  if (m->a.encoder_type != WFL_ENC_WHISPER) return fail(-1, "wfl_logmel: not a Whisper model");
  // (L == 0 would make the staging loads of logmel_power_kernel clamp their index to L - 1 = -1: rejected here, as wfl_forward does)
  if (!wav || !out) return fail(-1, "wfl_logmel: null wav or out");
  if (B <= 0 || L <= 0 || ldw < L) return fail(-1, "wfl_logmel: bad shape (B > 0, L > 0, ldw >= L)");
  if (int r = check_device(m, "wfl_logmel")) return r;
  const Plan p = make_plan(m, B, L);
  if (workspace_bytes < p.total) return fail(-1, "wfl_logmel: workspace too small");
  const int r = run_logmel(m, p, (char*)workspace, wav, ldw, lens, out, (hipStream_t)stream);
  return r ? fail(r, "logmel launch failed") : 0;
}

// The opening steps of every forward: the workspace and frame-count checks (`who` = the entry point, for its messages), then the halo
// rows of the buffers every stage shares (cheap; keeps the layout invariant independent of the workspace's history) and the forward's
// error word.
static int begin_forward(Runner& R, const char* who, int64_t workspace_bytes, bool with_encoder) {
  const Plan& p = R.p;
  if (!R.ws || workspace_bytes < p.total) return fail(-1, std::string(who) + ": workspace too small");
  if (p.T <= 0) return fail(-1, std::string(who) + ": clip too short for the encoder");
  // QKp / ATTp: a padded Conformer head size only; mel / c1: the Whisper stem (a head-only plan has neither)
  for (int lo_half = 0; lo_half <= (R.precise() ? 1 : 0); ++lo_half) {   // the low halves' halo rows are taps of the split-precision convolutions too
    for (Buf b : {BUF_X, BUF_Y, BUF_ATT, BUF_QK, BUF_FF, BUF_QKP, BUF_ATTP, BUF_MEL, BUF_C1})
      if (p.bufs[b].bytes && (with_encoder || (b != BUF_MEL && b != BUF_C1))) R.zero_add(b, lo_half != 0);
    // the first launch clears the error word (a kernel, not a memset node: graph replay)
    R.zm.err_word = lo_half ? nullptr : (unsigned*)(R.ws + p.err);
    R.zero_flush();
  }
  // a zero-padded width (encoder_type none): the front-end / wfl_head write only the valid columns of the Y rows
  if (!R.rc && R.m->dv != p.d && wfl_launch_fill_i32((int*)R.act(BUF_Y), p.bufs[BUF_Y].bytes / 4, 0, R.s)) return fail(-3, "fill launch failed");
  return R.rc;
}

// Ragged batches: every row of the buffers the stages share starts at zero (begin_forward zeroed their halo rows only); producers skip
// the rows behind a clip's own frame count, so those stay zero for the whole forward -- for the convolutions' taps and the positional
// conv's padding they are the same zeros the halo rows are.
static int zero_shared_buffers(Runner& R) {
  const Plan& p = R.p;
  for (int lo_half = 0; lo_half <= (R.precise() ? 1 : 0); ++lo_half)       // ... and their low halves
    for (Buf b : {BUF_X, BUF_Y, BUF_ATT, BUF_QK, BUF_FF, BUF_QKP, BUF_ATTP}) {
      const ActBuf& a = p.bufs[b];
      if (!a.bytes) continue;
      if (int r = wfl_launch_fill_i32((int*)(R.ws + (lo_half ? a.lo : a.off)), a.bytes / 4, 0, R.s)) return fail(r, "fill launch failed");
    }
  return 0;
}

// Feature extractor + encoder (model.py:149-161): leaves the encoder output in the Y rows.
static int run_encoder(Runner& R, const float* wav, int64_t ldw, const int32_t* lens) {
  wfl_model* m = R.m;
  const wfl_arch& a = m->a;
  const Plan& p = R.p;
  const int B = p.B, L = p.L, d = p.d;
  const long Mrows = (long)B * p.P;
  const GemmRows rows{(int)Mrows, p.P, p.T};
  bf16_t *X = R.act(BUF_X), *Y = R.act(BUF_Y), *ATT = R.act(BUF_ATT), *QK = R.act(BUF_QK), *FF = R.act(BUF_FF);
  if (a.encoder_type == WFL_ENC_WHISPER) {
    // ---- Whisper encoder (HF modeling_whisper.py:618-642)
    R.prof_begin();
    const int r = run_logmel(m, p, R.ws, wav, ldw, lens, nullptr, R.s);
    R.prof_end(PROF_LOGMEL, 0.96e9 * (double)B * (a.n_mels / 80.0));
    if (r) return fail(r, "logmel launch failed");
    if (R.precise()) R.lo_ok[BUF_MEL] = true;                // (the log-mel kernel wrote the features' low half)
    bf16_t* mel = R.act(BUF_MEL);
    bf16_t* c1 = R.act(BUF_C1);
    // conv1 k3 p1: frame t reads mel rows t-1..t+1 = 3*n_mels contiguous channels
    R.gemm(mel + (long)(p.lead2 - 1) * a.n_mels, a.n_mels, m->conv1, {B * p.P2, p.P2, p.T2}, {c1, d, p.lead2, p.P2}, {.act = WFL_ACT_GELU});
    // conv2 k3 s2 p1: frame t reads c1 rows 2t-1..2t+1; pitch(c1) = 2 * pitch(X) makes it one flat GEMM with lda = 2d
    // (lo_out: the residual stream starts here)
    R.gemm(c1 + (long)(p.lead2 - 1) * d, 2 * d, m->conv2, rows, R.out(X, d), {.act = WFL_ACT_GELU, .pos = m->pos, .ldpos = d, .lo_out = true});
    // fp8 x fp8 (BASELINE configs[4]; WFL_FP8_ACT=0: fp8 weights with bf16 activations, round 2's form): every GEMM operand of a layer
    // is e4m3 -- LayerNorm outputs and the attention context with one scale per row (norm.hip), fc1's GELU output straight from its
    // epilogue with a fixed scale -- and the four GEMMs run on v_mfma_f32_16x16x32_fp8_fp8 (gemm_stream.hip, A8)
    // Round 4: e4m3 activations are an explicit opt-in (wfl_arch::fp8_activations, "model.activation_dtype: fp8"); the default for an
    // fp8-weight model is bf16 activations, which holds the reference's arithmetic on the fp8-rounded checkpoint.  WFL_FP8_ACT=0 / 1
    // overrides either way (A/B runs).
    static int fp8_act_env = -2;
    if (fp8_act_env == -2) { const char* e = getenv("WFL_FP8_ACT"); fp8_act_env = e ? atoi(e) : -1; }
    const int fp8_act = fp8_act_env >= 0 ? fp8_act_env : a.fp8_activations;
    const bool act8 = a.fp8_weights && fp8_act && p.X8 > 0 && p.ffw == a.enc_ffn;
    // fp8_act: 1 single e4m3 activations on gemm_stream's non-scaled fp8 MFMA (round 3); 2 the same on the block-scaled K = 128 MFMA
    // (gemm_mx.hip, twice the rate); 3 e4m3 PAIRS hi + lo on that MFMA -- eight significant bits per activation, the parity of bf16
    // activations at the fp8 MFMA's price per pass
    const bool pair8 = fp8_act == 3;
    const int a8_mode = fp8_act == 1 ? 1 : (pair8 ? 3 : 2);
    for (int i = 0; act8 && i < a.enc_layers; ++i) {
      const EncLayer& L_ = m->enc[i];
      unsigned char* X8 = (unsigned char*)(R.ws + p.X8);
      unsigned char* FF8 = (unsigned char*)(R.ws + p.FF8);
      unsigned char* X8lo = pair8 ? (unsigned char*)(R.ws + p.X8lo) : nullptr;
      unsigned char* FF8lo = pair8 ? (unsigned char*)(R.ws + p.FF8lo) : nullptr;
      float* rs8 = (float*)(R.ws + p.rs8);
      // fixed scales of the two operands whose producer cannot see a whole row: single e4m3 stores e4m3(8 x) (|x| <= 56, normal numbers
      // down to 2^-9); a pair carries eight significant bits, so e4m3(4 x) + lo covers |x| <= 112 down to 2^-13.  A value beyond the
      // range sets bit 1 of the status word (GemmArgs::err / AttnArgs::err): never a silent clip.
      const float ff_scale = pair8 ? 4.0f : 8.0f;
      const float att_scale = pair8 ? 4.0f : 8.0f;
      auto rows8 = [&](const bf16_t* x, const bf16_t* x_lo, const LNp* w) {
        if (R.rc) return;
        R.prof_begin();
        const int r = wfl_launch_rows_fp8(x, d, x_lo, w ? w->g : nullptr, w ? w->b : nullptr, 1e-5f, p.lead, B, p.P, p.T, d, X8, d, rs8, R.s, X8lo);
        R.prof_end(PROF_LAYERNORM, 0.0);
        if (r) R.rc = fail(r, "rows_fp8 launch failed");
      };
      // the e4m3 operand of the next launch: one scale per row (rows8) or a fixed one, and the plane of the pairs' low halves
      auto in8 = [&](const float* row_scale, float stat, const unsigned char* lo_plane) {
        return GemmOpts{.a8 = a8_mode, .a8_scale = row_scale, .a8_static = stat, .a8_lo = lo_plane};
      };
      const unsigned char* X8lo_rows = X8lo ? R.rows(X8lo, d) : nullptr;
      const bf16_t* X8_rows = (const bf16_t*)R.rows(X8, d);
      rows8(X, R.lo_in(X), &L_.ln1);
      R.gemm(X8_rows, d, L_.qkv, rows, R.out(QK, 3 * d), in8(rs8, 1.f, X8lo_rows));
      // the attention context leaves the attention kernel as e4m3 (a pair in mode 3) with a fixed scale (head_dim 64; other head sizes:
      // bf16, then quantised per row): a context row is a convex combination of value rows, |x| <= max |v|
      GemmOpts o;
      if (d / a.enc_heads == 64) {
        R.attn(a.enc_heads, nullptr, nullptr, false, X8, d, att_scale, X8lo);
        o = in8(nullptr, 1.0f / att_scale, X8lo_rows);
      } else {
        R.attn(a.enc_heads);
        rows8(ATT, nullptr, nullptr);
        o = in8(rs8, 1.f, X8lo_rows);
      }
      o.res = X; o.ldres = d;
      R.gemm(X8_rows, d, L_.out, rows, R.out(X, d), o);
      rows8(X, R.lo_in(X), &L_.ln2);
      o = in8(rs8, 1.f, X8lo_rows);
      o.act = WFL_ACT_GELU;
      o.c8 = FF8; o.c8_lo = FF8lo; o.ldc8 = p.ffw; o.c8_inv = ff_scale;
      R.gemm(X8_rows, d, L_.fc1, rows, R.out(FF, p.ffw), o);
      o = in8(nullptr, 1.0f / ff_scale, FF8lo ? R.rows(FF8lo, p.ffw) : nullptr);
      o.res = X; o.ldres = d;
      R.gemm((const bf16_t*)R.rows(FF8, p.ffw), p.ffw, L_.fc2, rows, R.out(X, d), o);
    }
    for (int i = 0; !act8 && i < a.enc_layers; ++i) {
      const EncLayer& L_ = m->enc[i];
      R.ln_gemm(X, Y, L_.ln1, L_.qkv, L_.qkv_ln, (int)Mrows, QK, 3 * d, WFL_ACT_NONE);
      R.attn(a.enc_heads);
      // want_stats: for the folded fc1, then for the next layer's folded q|k|v (the final LayerNorm is a kernel)
      R.gemm(R.rows(ATT, d), d, L_.out, rows, R.out(X, d), {.res = X, .ldres = d, .want_stats = true});
      R.ln_gemm(X, Y, L_.ln2, L_.fc1, L_.fc1_ln, (int)Mrows, FF, p.ffw, WFL_ACT_GELU);
      R.gemm(R.rows(FF, p.ffw), p.ffw, L_.fc2, rows, R.out(X, d), {.res = X, .ldres = d, .want_stats = i + 1 < a.enc_layers});
    }
    R.ln(X, Y, m->enc_ln, true);   // encoder output in Y (with lang_id None it is the head's residual stream)
  } else if (a.encoder_type == WFL_ENC_NONE) {
    // ---- no encoder: hidden = MelSpectrogram(wav).transpose(1, 2) (model.py:149-150).  Like WavLM input it is never padded by the
    // reference: one clip length per call.
    if (lens) {                                        // (every clip keeps its own frame count: Runner::clipT)
      int* ct = (int*)(R.ws + p.clipT);
      const int k0 = 0, s0 = a.mel_hop;
      const int cr = wfl_launch_clip_frames(lens, B, L, 1, &k0, &s0, 201, ct, R.s);
      if (cr) return fail(cr, "clip_frames launch failed");
      R.clipT = ct;
      if (int zr = zero_shared_buffers(R)) return zr;
    }
    if (L <= 200) return fail(-1, "wfl_forward: encoder_type none needs more than 200 samples (reflect padding of the STFT)");
    LogmelArgs la{};
    la.wav = wav; la.ldw = ldw; la.lens = lens; la.L = L; la.B = B;
    la.n_frames = p.T; la.n_samples = L; la.n_mels = a.n_mels;
    la.Wc = m->Wc; la.Ws = m->Ws; la.mel_lo = m->mel_lo; la.mel_cnt = m->mel_cnt; la.mel_w = m->mel_w; la.mel_maxw = m->mel_maxw;
    la.raw = (float*)(R.ws + p.raw); la.clipmax = nullptr;
    R.prof_begin();
    const int r = wfl_launch_melpower(la, a.mel_hop, Y, d, p.lead, p.P, m->pad_split(), m->pad_shift(), R.s);
    R.prof_end(PROF_LOGMEL, 0.0);
    if (r) return fail(r, "mel launch failed");
    R.lo_ok[BUF_Y] = false;
    if (R.precise()) {                                 // the fp32 mel power once more, as hi + lo rows
      const int r2 = wfl_launch_f32_to_rows(la.raw, Y, d, p.lead, B, p.P, p.T, a.n_mels, R.s, m->pad_split(), m->pad_shift(), R.lo_of(Y));
      if (r2) return fail(r2, "f32_to_rows launch failed");
      R.lo_ok[BUF_Y] = true;
    }
  } else {
    // ---- WavLM (HF modeling_wavlm.py:1032-1088).  The reference never pads WavLM input: with `lens` every clip keeps its own sample
    // and frame counts through the whole forward (Runner::clipT), i.e. what it gets when it is labelled alone.
    if (lens) {
      int* ct = (int*)(R.ws + p.clipT);
      const int cr = wfl_launch_clip_frames(lens, B, L, p.nlev, a.wavlm_conv_kernel, a.wavlm_conv_stride, 0, ct, R.s);
      if (cr) return fail(cr, "clip_frames launch failed");
      for (int i = 0; i < p.nlev; ++i) R.levelT[i] = ct + (long)i * B;
      R.clipT = R.levelT[p.nlev - 1];
      if (int zr = zero_shared_buffers(R)) return zr;
    }
    if (p.T > WAVLM_MAX_T) return fail(-1, "wfl_forward: clip too long for the WavLM relative-position table");
    const int C = a.wavlm_conv_dim[0], n = p.nlev;
    bf16_t* F[2] = {R.act(BUF_FA), R.act(BUF_FB)};
    double* wstats = nullptr;
    if (a.wavlm_do_normalize) {
      wstats = (double*)(R.ws + p.wstats);
      const int r = wfl_launch_wav_stats(wav, ldw, B, L, wstats, R.s, lens);
      if (r) return fail(r, "wav_stats launch failed");
    }
    // Rows that are not valid frames of a level are zeroed before the level is produced (the two buffers alternate
    // between levels; a K-padded conv GEMM may read a few channels past the last valid frame).
    const bool pairs = R.precise();                    // precision high: the feature extractor's rows as bf16 pairs too
    R.zero(F[0], C, p.leadl[0], p.Pl[0], p.Tl[0], p.tail);
    if (pairs) R.zero(R.lo_of(F[0]), C, p.leadl[0], p.Pl[0], p.Tl[0], p.tail);
    if (R.rc) return R.rc;
    {
      Conv0Args c{};
      if (pairs) { c.out_lo = R.lo_of(F[0]); R.lo_ok[BUF_FA] = c.out_lo != nullptr; }
      c.wav = wav; c.ldw = ldw; c.L = L; c.wstats = wstats; c.w = m->conv0_w; c.bias = m->conv0_b;
      c.gamma = m->conv0_norm.g; c.beta = m->conv0_norm.b; c.B = B; c.T0 = p.Tl[0]; c.C = C; c.lens = lens;
      c.cstats = (double*)(R.ws + p.cstats); c.cpart = (float*)(R.ws + p.cpart); c.out = F[0]; c.lead = p.leadl[0]; c.P = p.Pl[0];
      const int r = wfl_launch_conv0(c, a.wavlm_group_norm, R.s);
      if (r) return fail(r, "conv0 launch failed");
    }
    for (int i = 1; i < n; ++i) {
      // conv k, stride 2, no padding: output frame t reads input rows 2t .. 2t+k-1 = k*C contiguous channels, lda = 2C
      const bf16_t* in = F[(i - 1) & 1] + (long)p.leadl[i - 1] * C;
      bf16_t* out = F[i & 1];
      const bool group = a.wavlm_group_norm != 0;
      R.zero(out, C, p.leadl[i], p.Pl[i], p.Tl[i], p.tail);
      if (pairs) R.zero(R.lo_of(out), C, p.leadl[i], p.Pl[i], p.Tl[i], p.tail);
      R.gemm(in, 2 * C, m->fconv[i - 1], {B * p.Pl[i], p.Pl[i], p.Tl[i]}, {out, C, p.leadl[i], p.Pl[i]},
             {.act = group ? WFL_ACT_GELU : WFL_ACT_NONE});
      if (!group && !R.rc) {
        const int r = wfl_launch_layernorm_act(out, C, out, C, m->fconv_ln[i - 1].g, m->fconv_ln[i - 1].b, 1e-5f, p.leadl[i], B,
                                               p.Pl[i], p.Tl[i], C, 1, R.s, R.lo_in(out), pairs ? R.lo_of(out) : nullptr, 0, R.levelT[i]);
        if (r) return fail(r, "layernorm launch failed");
      }
    }
    if (R.rc) return R.rc;
    bf16_t* feats = F[(n - 1) & 1];                    // level n-1 has the main geometry (lead, P, T)
    {
      const int r = wfl_launch_layernorm_act(feats, C, feats, C, m->fp_ln.g, m->fp_ln.b, 1e-5f, p.lead, B, p.P, p.T, C, 0, R.s, R.lo_in(feats),
                                             pairs ? R.lo_of(feats) : nullptr, 0, R.clipT);
      if (r) return fail(r, "layernorm launch failed");
    }
    R.gemm(R.rows(feats, C), C, m->fp_proj, rows, R.out(X, d), {.lo_out = true});
    // positional conv: x + GELU(grouped conv k, pad k/2, last step dropped), one contiguous-tap GEMM per group
    {
      const int G = a.wavlm_pos_conv_groups, cpg = d / G, K = a.wavlm_pos_conv_kernel;
      bf16_t* XG = R.act(BUF_XG);
      if (!R.rc) {
        int r = wfl_launch_regroup(X, d, G, cpg, p.R, p.lead, B, p.P, p.T, XG, R.s, R.clipT);
        R.lo_ok[BUF_XG] = false;
        if (!r && pairs && R.lo_in(X)) {                 // the low halves in the same layout: the per-group GEMMs' third pass
          r = wfl_launch_regroup(R.lo_in(X), d, G, cpg, p.R, p.lead, B, p.P, p.T, R.lo_of(XG), R.s, R.clipT);
          R.lo_ok[BUF_XG] = true;
        }
        if (r) return fail(r, "regroup launch failed");
      }
      // all groups in one tap-stationary launch (posconv.hip); WFL_POSCONV_GEMM=1 keeps rounds 1-2's GEMM per group (A/B runs)
      static int as_gemm = -1;
      if (as_gemm < 0) { const char* e = getenv("WFL_POSCONV_GEMM"); as_gemm = e && atoi(e) ? 1 : 0; }
      int taken = 1;
      if (!as_gemm && !pairs && !R.rc && G <= 16) {      // (precision high: the GEMM per group, three passes each)
        PosConvArgs pc{};
        pc.xg = XG; pc.R = p.R; pc.lead = p.lead; pc.B = B; pc.P = p.P; pc.T = p.T; pc.groups = G; pc.cpg = cpg; pc.taps = K;
        for (int gi = 0; gi < G; ++gi) { pc.w[gi] = m->posconv[gi].W; pc.bias[gi] = m->posconv[gi].bias; }
        pc.ldw = m->posconv[0].K;
        pc.res = X; pc.res_lo = R.lo_in(X); pc.out = Y; pc.out_lo = R.lo_of(Y); pc.ld = d;
        pc.clip_T = R.clipT;
        R.prof_begin();
        taken = wfl_launch_posconv(pc, R.s);
        R.prof_end(PROF_POSCONV, 2.0 * (double)B * p.T * (double)d * (double)cpg * (double)K);
        if (taken < 0) return fail(taken, "posconv launch failed");
        if (taken == 0) { R.lo_ok[BUF_Y] = true; R.stats_for = nullptr; }
      }
      for (int gi = 0; gi < G && taken == 1; ++gi)
        R.gemm(XG + ((long)gi * p.R + p.lead - K / 2) * 64, 64, m->posconv[gi], rows, R.out(Y + gi * cpg, d),
               {.act = WFL_ACT_GELU, .res = X + gi * cpg, .ldres = d});
    }
    bf16_t *H = Y, *S = X;                             // current hidden states / scratch
    const bool stable = a.wavlm_stable_layer_norm != 0;
    if (!stable) { R.ln(H, S, m->wenc_ln, true); std::swap(H, S); }
    float* gate = (float*)(R.ws + p.gate);
    float* rtab = (float*)(R.ws + p.rtab);
    if (!R.rc) {
      const int r = wfl_launch_relpos_table(m->rel_emb, m->bucket_of_delta, WAVLM_MAX_T, a.enc_heads, p.T, rtab, R.s);
      if (r) return fail(r, "relpos_table launch failed");
    }
    const int hd = d / a.enc_heads;
    for (int i = 0; i < a.enc_layers && !R.rc; ++i) {
      const WavlmLayer& L_ = m->wl[i];
      bf16_t* A_in = H;                                // what the attention block sees
      if (stable) { R.ln(H, S, L_.ln1); A_in = S; }
      if (R.rc) break;
      int r = wfl_launch_relpos_gate(A_in, d, p.lead, B, p.P, p.T, a.enc_heads, hd, L_.w8, L_.b8, L_.cst, gate, R.s, R.lo_in(A_in));
      if (r) return fail(r, "relpos_gate launch failed");
      R.gemm(R.rows(A_in, d), d, L_.qkv, rows, R.out(QK, 3 * d));
      R.attn(a.enc_heads, rtab, gate);
      if (stable) {
        // x = x + attn; x = x + FFN(LN(x))
        R.gemm(R.rows(ATT, d), d, L_.out, rows, R.out(H, d), {.res = H, .ldres = d, .want_stats = L_.fc1_ln.ln_s != nullptr});
        R.ln_gemm(H, S, L_.ln2, L_.fc1, L_.fc1_ln, (int)Mrows, FF, p.ffw, WFL_ACT_GELU);
        R.gemm(R.rows(FF, p.ffw), p.ffw, L_.fc2, rows, R.out(H, d), {.res = H, .ldres = d});
      } else {
        // x = LN(x + attn); x = LN_final(x + FFN(x))
        R.gemm(R.rows(ATT, d), d, L_.out, rows, R.out(S, d), {.res = H, .ldres = d});
        R.ln(S, H, L_.ln1, true);
        R.gemm(R.rows(H, d), d, L_.fc1, rows, R.out(FF, p.ffw), {.act = WFL_ACT_GELU});
        R.gemm(R.rows(FF, p.ffw), p.ffw, L_.fc2, rows, R.out(S, d), {.res = H, .ldres = d});
        R.ln(S, H, L_.ln2, true);
      }
    }
    if (stable) { R.ln(H, S, m->wenc_ln, true); std::swap(H, S); }
    if (H != Y && !R.rc) {                             // the head expects the encoder output in Y
      R.stats_for = nullptr;
      if (wfl_launch_copy16(Y, H, p.R * d * 2, R.s)) return fail(-3, "copy launch failed");
      if (R.lo_in(H) && wfl_launch_copy16(R.lo_of(Y), R.lo_of(H), p.R * d * 2, R.s)) return fail(-3, "copy launch failed");
      R.lo_ok[BUF_Y] = R.lo_in(H) != nullptr;
    }
  }
  return R.rc;
}

// The encoder output as the caller sees it: compact fp32 [B][T][hidden_size]
static int emit_hidden(Runner& R, float* hidden) {
  const wfl_model* m = R.m;
  const Plan& p = R.p;
  if (m->a.encoder_type == WFL_ENC_NONE)           // the mel power itself, before its rounding into the bf16 rows
    return wfl_launch_axpy(hidden, (const float*)(R.ws + p.raw), (long)p.B * p.T * m->a.n_mels, 1.f, 1, R.s);
  // (the default build hands out the high halves only: wfl_head rounds its input to bf16 again, and bf16(hi + lo) is not always hi --
  //  lo can round up to exactly half a unit of hi -- which would cost wfl_encode + wfl_head == wfl_forward its bit-exactness)
  return wfl_launch_rows_to_f32(R.act(BUF_Y), p.d, p.lead, p.B, p.P, p.T, m->dv, hidden, R.s, m->pad_split(), m->pad_shift(),
                                R.precise() ? R.lo_in(R.act(BUF_Y)) : nullptr);
}

// Head (model.py:176-194) + tag decision on the encoder output in the Y rows.
static int run_head(Runner& R, const int32_t* lang_id, int32_t lang_mode, float threshold, int32_t* ids, int32_t* argmax,
                    float* maxprob, float* offsets, float* logits, int32_t* status) {
  wfl_model* m = R.m;
  const wfl_arch& a = m->a;
  const Plan& p = R.p;
  const int B = p.B, d = p.d;
  const long Mrows = (long)B * p.P;
  const GemmRows rows{(int)Mrows, p.P, p.T};
  bf16_t *X = R.act(BUF_X), *Y = R.act(BUF_Y), *ATT = R.act(BUF_ATT), *QK = R.act(BUF_QK), *FF = R.act(BUF_FF);
  // ---- head (model.py:176-194); with WFL_LANG_AVERAGE it runs once per language on the same encoder output
  const int n_pass = lang_mode == WFL_LANG_AVERAGE ? (int)m->avg_langs.size() : 1;
  float* lg = logits ? logits : (float*)(R.ws + p.logits);
  bf16_t* ENC = Y;
  // the head needs Y as scratch: keep the encoder output in ATT when more than one pass reads it
  if (n_pass > 1) {
    ENC = R.act(BUF_ENC2);
    if (wfl_launch_copy16(ENC, Y, p.R * d * 2, R.s)) return fail(-3, "copy launch failed");
    if (R.precise()) {                                   // ... and its low half
      const bool have_lo = R.lo_in(Y) != nullptr && R.lo_of(ENC) != nullptr;
      if (have_lo && wfl_launch_copy16(R.lo_of(ENC), R.lo_of(Y), p.R * d * 2, R.s)) return fail(-3, "copy launch failed");
      R.mark_lo(ENC, have_lo);
    }
  }
  int* lang_dev = nullptr;
  for (int pass = 0; pass < n_pass; ++pass) {
    bf16_t* H;      // current activation
    bf16_t* S;      // scratch of the same shape
    if (lang_mode == WFL_LANG_NONE) {
      H = Y; S = X;
    } else {
      const int* idx = lang_id;
      if (lang_mode == WFL_LANG_AVERAGE) {
        // clip_idx = this pass's language id for every clip: reuse the clipmax slot region (B ints) as a constant index vector
        lang_dev = (int*)(R.ws + p.clipmax);
        const int fr = wfl_launch_fill_i32(lang_dev, B, m->avg_langs[pass], R.s);
        if (fr) return fail(fr, "fill launch failed");
        idx = lang_dev;
      }
      R.gemm(R.rows(ENC, d), d, m->lang, rows, R.out(X, d),
             {.clip_bias = m->lang_table, .clip_idx = idx, .clip_ld = d, .lo_out = true});
      H = X; S = Y;
    }
    if (a.enable_bilstm) {
      const int Hh = d / 2;
      float* GX = (float*)(R.ws + p.gx);
      for (int layer = 0; layer < a.bilstm_layers; ++layer) {
        R.gemm(R.rows(H, d), d, m->lstm_in[layer], rows, R.out(GX, 8 * Hh), {.out_f32 = true});
        if (R.rc) return R.rc;
        LstmArgs la{};
        la.gx = GX; la.ldgx = 8 * Hh; la.whh = m->lstm_whh[layer]; la.out = S; la.ldo = d; la.lead = p.lead;
        la.B = B; la.T = p.T; la.P = p.P; la.H = Hh; la.U = m->lstm_U;
        la.error = (unsigned*)(R.ws + p.err);
        la.clip_T = R.clipT;
        R.stats_for = nullptr;
        // the recurrence writes plain bf16 rows -- or, precision high with H <= 256, h as a bf16 pair like every other activation
        const bool split = R.precise() && m->lstm_whh_lo[layer] != nullptr && R.lo_of(S) != nullptr;
        if (split) { la.whh_lo = m->lstm_whh_lo[layer]; la.out_lo = R.lo_of(S); }
        R.mark_lo(S, split);
        R.prof_begin();
        const int lr = wfl_launch_lstm(la, R.ws + p.lstm_x, R.s);
        R.prof_end(PROF_LSTM, 2.0 * (double)B * p.T * 2.0 * 4.0 * (double)Hh * (double)Hh);
        if (lr) return fail(lr, lr == -5 ? "BiLSTM: hidden size too large (more than 64 slice workgroups per direction)"
                                          : "lstm launch failed (" + std::to_string(lr) + ")");
        std::swap(H, S);
      }
    }
    for (int i = 0; i < a.n_conformer; ++i) {
      const ConfLayer& C = m->conf[i];
      // x = x + 0.5 * FF1(x)
      R.ln_gemm(H, S, C.ff1_ln, C.ff1_a, C.ff1_a_ln, (int)Mrows, FF, p.ffw, WFL_ACT_GELU);
      R.gemm(R.rows(FF, p.ffw), p.ffw, C.ff1_b, rows, R.out(H, d), {.res = H, .ldres = d, .alpha = 0.5f});
      // x = LN1(x + MHA(x))
      if (p.da == d) {
        R.gemm(R.rows(H, d), d, C.qkv, rows, R.out(QK, 3 * d));
        R.attn(a.conformer_heads);
        R.gemm(R.rows(ATT, d), d, C.out, rows, R.out(S, d), {.res = H, .ldres = d});
      } else {
        R.gemm(R.rows(H, d), d, C.qkv, rows, R.out(R.act(BUF_QKP), 3 * p.da));
        R.attn(a.conformer_heads, nullptr, nullptr, true);
        R.gemm(R.rows(BUF_ATTP), p.da, C.out, rows, R.out(S, d), {.res = H, .ldres = d});
      }
      // ... and LN2(x) for the conv module in the same pass: x = x + pw2(GELU(BN(conv_k(GLU(pw1(LN2(x)))))))
      R.ln_pair(S, H, C.ln1, S, C.ln2);
      R.gemm(R.rows(S, d), d, C.pw1, rows, R.out(ATT, d), {.glu = true});
      // dense k-tap conv: taps are adjacent rows (cin = d, tap stride = one row) -> the streaming GEMM's tap-stationary mode
      R.gemm(ATT + (long)(p.lead - a.conformer_kernel / 2) * d, d, C.conv, rows, R.out(S, d),
             {.act = WFL_ACT_GELU, .cin = d, .tap_stride = d});
      // want_stats: for the folded ff2, then for the next block's folded ff1
      R.gemm(R.rows(S, d), d, C.pw2, rows, R.out(H, d), {.res = H, .ldres = d, .want_stats = true});
      // x = x + 0.5 * FF2(x)
      R.ln_gemm(H, S, C.ff2_ln, C.ff2_a, C.ff2_a_ln, (int)Mrows, FF, p.ffw, WFL_ACT_GELU);
      R.gemm(R.rows(FF, p.ffw), p.ffw, C.ff2_b, rows, R.out(H, d),
             {.res = H, .ldres = d, .alpha = 0.5f, .want_stats = i + 1 < a.n_conformer});
    }
    if (a.enable_dilated) {
      for (int i = 0; i < a.dilated_depth; ++i) {
        const int dil = 1 << i, pad = dil * (a.dilated_kernel - 1) / 2;
        R.gemm(H + (long)(p.lead - pad) * d, d, m->dil[i], rows, R.out(S, d), {.act = WFL_ACT_RELU, .cin = d, .tap_stride = (long)dil * d});
        std::swap(H, S);
      }
    }
    float* lg_pass = (n_pass > 1 && pass > 0) ? (float*)(R.ws + p.logits2) : lg;
    // (the internal logits buffer has rows of a multiple of four floats: the fp32 epilogue then stores 16 bytes at a time instead of
    //  141 single floats per row; the caller's own buffer and the language-averaging passes keep the compact layout)
    const long ldlg = (!logits && n_pass == 1) ? round_up(a.num_classes, 4) : a.num_classes;
    // classifier in split precision: h_hi . W_lo^T first, then [h_hi | h_lo] . [W_hi | W_hi]^T + b added to it in fp32 (the two
    // input halves are taps one buffer apart; without a valid low half the second pass is the plain K = d one)
    static const bool cls_one = std::getenv("WFL_CLS_TWO_LAUNCHES") == nullptr;       // (A/B hook: rounds 2-3's two-launch form)
    const bf16_t* hlo = R.lo_in(H);
    const bf16_t* Hrows = R.rows(H, d);
    const GemmOut lg_out{lg_pass, ldlg, 0, p.T};                    // compact rows: no halo
    const double cls_flops = 2.0 * (double)B * p.T * (double)a.num_classes * (double)d;
    if (hlo && m->cls3.W && cls_one) {
      // one launch (round 3): K' = 3 d over the tap segments [h_hi | h_lo | h_hi] against [W_hi | W_hi | W_lo], bias once, the sum never
      // leaves the accumulators
      R.gemm(Hrows, d, m->cls3, rows, lg_out, {.cin = d, .out_f32 = true, .flops = cls_flops, .tap_wrap = 1, .seg_off = (long)(hlo - H)});
    } else {
      R.gemm(Hrows, d, m->cls_lo, rows, lg_out, {.out_f32 = true, .flops = 0.0});       // (the product is booked once, below)
      if (hlo)
        R.gemm(Hrows, d, m->cls_hi2, rows, lg_out,
               {.cin = d, .tap_stride = (long)(hlo - H), .out_f32 = true, .acc_f32 = true, .flops = cls_flops});
      else
        R.gemm(Hrows, d, m->cls, rows, lg_out, {.out_f32 = true, .acc_f32 = true, .flops = cls_flops});
    }
    R.gemm(H + (long)(p.lead - 1) * d, d, m->off1, rows, R.out(S, d), {.act = WFL_ACT_GELU, .cin = d, .tap_stride = d});
    if (R.rc) return R.rc;
    TagArgs t{};
    t.rows = B * p.T; t.C = a.num_classes; t.threshold = threshold; t.o_id = a.o_id;
    t.ids = ids; t.argmax = argmax; t.maxprob = maxprob;
    t.hid = S; t.hid_lo = R.lo_in(S); t.ldh = d; t.lead = p.lead; t.P = p.P; t.T = p.T; t.d = d; t.w2 = m->off_w2; t.b2 = m->off_b2;
    t.clip_T = R.clipT; t.Tmax = p.T;
    if (n_pass == 1) {
      t.logits = lg; t.ldl = ldlg; t.offsets = offsets;
      t.status_src = (const unsigned*)(R.ws + p.err); t.status_dst = status;
      const int r = wfl_launch_tag_decide(t, R.s);
      if (r) return fail(r, "tag_decide launch failed");
    } else {
      // offsets of this pass only; logits are decided after the mean
      t.logits = nullptr;
      t.offsets = pass == 0 ? offsets : (float*)(R.ws + p.offs2);
      int r = wfl_launch_tag_decide(t, R.s);
      if (r) return fail(r, "tag_decide launch failed");
      const float w = 1.0f / (float)n_pass;
      const long nl = (long)B * p.T * a.num_classes, no = (long)B * p.T * 2;
      if (pass == 0) {
        r = wfl_launch_axpy(lg, lg, nl, w, 1, R.s);
        if (!r) r = wfl_launch_axpy(offsets, offsets, no, w, 1, R.s);
      } else {
        r = wfl_launch_axpy(lg, (float*)(R.ws + p.logits2), nl, w, 0, R.s);
        if (!r) r = wfl_launch_axpy(offsets, (float*)(R.ws + p.offs2), no, w, 0, R.s);
      }
      if (r) return fail(r, "axpy launch failed");
      if (pass == n_pass - 1) {
        TagArgs f{};
        f.logits = lg; f.ldl = a.num_classes; f.rows = B * p.T; f.C = a.num_classes; f.threshold = threshold;
        f.o_id = a.o_id; f.ids = ids; f.argmax = argmax; f.maxprob = maxprob;
        f.clip_T = R.clipT; f.Tmax = p.T;
        f.status_src = (const unsigned*)(R.ws + p.err); f.status_dst = status;
        r = wfl_launch_tag_decide(f, R.s);
        if (r) return fail(r, "tag_decide launch failed");
      }
    }
  }
  return R.rc;
}

static int check_forward_args(const wfl_model* m, const char* who, int32_t B, const int32_t* lang_id, int32_t lang_mode,
                              const int32_t* ids, const float* maxprob, const float* offsets) {
  if (!ids || !maxprob || !offsets) return fail(-1, std::string(who) + ": ids, maxprob and offsets are required");
  if (B <= 0) return fail(-1, std::string(who) + ": bad batch size");
  if (lang_mode == WFL_LANG_IDS && !lang_id) return fail(-1, std::string(who) + ": lang_id missing");
  if (lang_mode == WFL_LANG_AVERAGE && m->avg_langs.empty()) return fail(-1, std::string(who) + ": no languages to average");
  if (lang_mode < WFL_LANG_NONE || lang_mode > WFL_LANG_AVERAGE) return fail(-1, std::string(who) + ": bad lang_mode");
  return 0;
}

int32_t wfl_forward(wfl_model* m, const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L,
                    const int32_t* lang_id, int32_t lang_mode, float threshold, void* workspace, int64_t workspace_bytes,
                    int32_t* ids, int32_t* argmax, float* maxprob, float* offsets, float* logits, float* hidden,
                    int32_t* status, void* stream) {
  if (!m || !m->finalized) return fail(-1, "wfl_forward: model not finalized");
  if (!wav || B <= 0 || L <= 0 || ldw < L) return fail(-1, "wfl_forward: bad input shape");
  if (int r = check_forward_args(m, "wfl_forward", B, lang_id, lang_mode, ids, maxprob, offsets)) return r;
  if (int r = check_device(m, "wfl_forward")) return r;
  Runner R{m, make_plan(m, B, L), (char*)workspace, (hipStream_t)stream};
  if (int r = begin_forward(R, "wfl_forward", workspace_bytes, true)) return r;
  if (int r = run_encoder(R, wav, ldw, lens)) return r;
  if (hidden) {
    const int r = emit_hidden(R, hidden);
    if (r) return fail(r, "rows_to_f32 launch failed");
  }
  return run_head(R, lang_id, lang_mode, threshold, ids, argmax, maxprob, offsets, logits, status);
}

int32_t wfl_encode(wfl_model* m, const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, void* workspace,
                   int64_t workspace_bytes, float* hidden, void* stream) {
  if (!m || !m->finalized) return fail(-1, "wfl_encode: model not finalized");
  if (!wav || !hidden || B <= 0 || L <= 0 || ldw < L) return fail(-1, "wfl_encode: bad argument");
  if (int r = check_device(m, "wfl_encode")) return r;
  Runner R{m, make_plan(m, B, L), (char*)workspace, (hipStream_t)stream};
  if (int r = begin_forward(R, "wfl_encode", workspace_bytes, true)) return r;
  if (int r = run_encoder(R, wav, ldw, lens)) return r;
  const int r = emit_hidden(R, hidden);
  return r ? fail(r, "rows_to_f32 launch failed") : 0;
}

int64_t wfl_head_workspace_bytes(const wfl_model* m, int32_t B, int32_t T) {
  if (!m || B <= 0 || T <= 0) return -1;
  return make_plan(m, B, 0, T).total;
}

int32_t wfl_head(wfl_model* m, const float* hidden, int32_t B, int32_t T, const int32_t* lang_id, int32_t lang_mode,
                 float threshold, void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* argmax, float* maxprob,
                 float* offsets, float* logits, int32_t* status, void* stream) {
  if (!m || !m->finalized) return fail(-1, "wfl_head: model not finalized");
  if (!hidden || T <= 0) return fail(-1, "wfl_head: bad argument");
  if (int r = check_forward_args(m, "wfl_head", B, lang_id, lang_mode, ids, maxprob, offsets)) return r;
  if (int r = check_device(m, "wfl_head")) return r;
  Runner R{m, make_plan(m, B, 0, T), (char*)workspace, (hipStream_t)stream};
  const Plan& p = R.p;
  if (int r = begin_forward(R, "wfl_head", workspace_bytes, false)) return r;
  const int r = wfl_launch_f32_to_rows(hidden, R.act(BUF_Y), p.d, p.lead, B, p.P, p.T, m->dv, R.s, m->pad_split(), m->pad_shift(),
                                       R.precise() ? R.lo_of(R.act(BUF_Y)) : nullptr);
  if (r) return fail(r, "f32_to_rows launch failed");
  if (R.precise()) R.lo_ok[BUF_Y] = true;
  return run_head(R, lang_id, lang_mode, threshold, ids, argmax, maxprob, offsets, logits, status);
}

int32_t wfl_check(wfl_model* m, void* workspace, int64_t workspace_bytes, int32_t B, int32_t L, void* stream) {
  if (!m || !m->finalized || !workspace) return fail(-1, "wfl_check: bad argument");
  if (int r = check_device(m, "wfl_check")) return r;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  const Plan p = make_plan(m, B, L);
  if (workspace_bytes < p.total) return fail(-1, "wfl_check: workspace too small");
  unsigned err = 0;
  HIPCHK(hipMemcpy(&err, (char*)workspace + p.err, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (err & 1u) return fail(-20, "BiLSTM recurrence: an inter-workgroup wait timed out (results of the last forward are invalid)");
  if (err & 2u) return fail(-22, "fp8 activations: a value did not fit e4m3 at its scale (results of the last forward are invalid; run this "
                                 "checkpoint with bf16 activations)");
  if (err) return fail(-21, "device-side error word " + std::to_string(err));
  return 0;
}

// ------------------------------------------------------------------------------------------------ single-op exports
int32_t wfl_op_gemm_mx(const void* A8, const void* A8_lo, int64_t lda, const void* W8, const float* w_scale, const float* a_scale,
                       float a_static, int32_t M, int32_t N, int32_t K, int32_t P, int32_t T, void* C, int64_t ldc, int64_t c_lead,
                       int32_t c_pitch, const float* bias, const void* res, const void* res_lo, void* c_lo, float alpha, int32_t act,
                       void* c8, void* c8_lo, int64_t ldc8, float c8_inv_scale, int32_t* status, void* stream) {
  GemmArgs g{};
  g.A = (const bf16_t*)A8; g.a8_lo = (const unsigned char*)A8_lo; g.a8 = A8_lo ? 3 : 2; g.lda = lda; g.cin = K; g.W = (const bf16_t*)W8;
  g.w8_scale = w_scale; g.a8_scale = a_scale; g.a8_static = a_static; g.a8_lead = 0;
  g.M = M; g.N = N; g.K = K; g.n_valid = N; g.P = P; g.T = T; g.C = C; g.ldc = ldc; g.c_lead = c_lead; g.c_pitch = c_pitch;
  g.bias = bias; g.res = (const bf16_t*)res; g.res_lo = (const bf16_t*)res_lo; g.c_lo = (bf16_t*)c_lo; g.ldres = ldc; g.alpha = alpha; g.act = act;
  g.c8 = (unsigned char*)c8; g.c8_lo = (unsigned char*)c8_lo; g.ldc8 = ldc8; g.c8_inv_scale = c8_inv_scale; g.err = (unsigned*)status;
  if (!A8 || !W8 || !w_scale || (!C && !c8) || M <= 0 || P <= 0 || P % 8) return fail(-1, "wfl_op_gemm_mx: bad argument");
  const int r = wfl_launch_gemm_mx(g, (hipStream_t)stream);
  return r ? fail(r == 1 ? -1 : r, "wfl_op_gemm_mx: shape or argument not taken by gemm_mx.hip (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_rows_fp8(const void* x, int64_t ldx, const void* x_lo, const float* gamma, const float* beta, float eps, int64_t lead,
                        int32_t B, int32_t P, int32_t T, int32_t C, void* y8, void* y8_lo, int64_t ldy8, float* scale, void* stream) {
  const int r = wfl_launch_rows_fp8((const bf16_t*)x, ldx, (const bf16_t*)x_lo, gamma, beta, eps, lead, B, P, T, C, (unsigned char*)y8, ldy8,
                                    scale, (hipStream_t)stream, (unsigned char*)y8_lo);
  return r ? fail(r, "wfl_op_rows_fp8: invalid arguments or launch failure") : 0;
}

int32_t wfl_op_gemm(const void* A, int64_t lda, int32_t cin, int64_t tap_stride, const void* W, int32_t M, int32_t N,
                    int32_t K, int32_t n_valid, int32_t P, int32_t T, void* C, int64_t ldc, int64_t c_lead, int32_t c_pitch,
                    const float* bias, const void* res, int64_t ldres, float alpha, int32_t act, int32_t glu,
                    int32_t out_f32, void* stream) {
  GemmArgs g{};
  g.A = (const bf16_t*)A; g.lda = lda; g.cin = cin > 0 ? cin : K; g.tap_stride = tap_stride;
  g.W = (const bf16_t*)W; g.M = M; g.N = N; g.K = K; g.n_valid = n_valid; g.P = P; g.T = T;
  g.C = C; g.ldc = ldc; g.c_lead = c_lead; g.c_pitch = c_pitch; g.bias = bias;
  g.res = (const bf16_t*)res; g.ldres = ldres; g.alpha = alpha; g.act = act; g.glu = glu; g.out_f32 = out_f32;
  const int r = wfl_launch_gemm(g, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_gemm: invalid arguments or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_gemm_ln(const void* A, int64_t lda, const void* W, int32_t M, int32_t N, int32_t K, int32_t n_valid, int32_t P,
                       int32_t T, void* C, int64_t ldc, int64_t c_lead, int32_t c_pitch, const float* bias, const float* ln_s,
                       float ln_eps, int32_t act, void* stream) {
  if (!ln_s) return fail(-1, "wfl_op_gemm_ln: ln_s is required");
  GemmArgs g{};
  g.A = (const bf16_t*)A; g.lda = lda; g.cin = K; g.tap_stride = 0;
  g.W = (const bf16_t*)W; g.M = M; g.N = N; g.K = K; g.n_valid = n_valid; g.P = P; g.T = T;
  g.C = C; g.ldc = ldc; g.c_lead = c_lead; g.c_pitch = c_pitch; g.bias = bias; g.alpha = 1.f; g.act = act;
  g.ln_s = ln_s; g.ln_eps = ln_eps;
  const int r = wfl_launch_gemm(g, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_gemm_ln: shape not supported by the LayerNorm-folding kernel or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_gemm_split(const void* A_hi, const void* A_lo, int64_t lda, int32_t cin, int64_t tap_stride, const void* W3, int32_t M,
                          int32_t N, int32_t K, int32_t n_valid, int32_t P, int32_t T, void* C, void* C_lo, int64_t ldc, int64_t c_lead,
                          int32_t c_pitch, const float* bias, const void* res, const void* res_lo, int64_t ldres, float alpha,
                          int32_t act, int32_t glu, void* stream) {
  if (!A_hi || !A_lo || !W3 || !C || !C_lo) return fail(-1, "wfl_op_gemm_split: null argument");
  if (K <= 0 || (cin > 0 && K % cin)) return fail(-1, "wfl_op_gemm_split: K must be a whole number of taps");
  GemmArgs g{};
  g.A = (const bf16_t*)A_hi; g.lda = lda; g.cin = cin > 0 ? cin : K; g.tap_stride = tap_stride;
  g.tap_wrap = K / g.cin; g.seg_off = (long)((const bf16_t*)A_lo - (const bf16_t*)A_hi);
  g.W = (const bf16_t*)W3; g.M = M; g.N = N; g.K = 3 * K; g.n_valid = n_valid; g.P = P; g.T = T;
  g.C = C; g.c_lo = (bf16_t*)C_lo; g.ldc = ldc; g.c_lead = c_lead; g.c_pitch = c_pitch; g.bias = bias;
  g.res = (const bf16_t*)res; g.res_lo = res ? (const bf16_t*)res_lo : nullptr; g.ldres = ldres; g.alpha = alpha; g.act = act; g.glu = glu;
  g.ln_eps = 1e-5f;
  const int r = wfl_launch_gemm(g, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_gemm_split: invalid arguments or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_gemm_ex(const wfl_gemm_ex_args* x, int32_t* kernel_id, void* stream) {
  if (kernel_id) *kernel_id = 0;
  if (!x || x->struct_bytes != (int64_t)sizeof(wfl_gemm_ex_args)) return fail(-1, "wfl_op_gemm_ex: struct_bytes is not the size of wfl_gemm_ex_args");
  if (!x->A || !x->W || (!x->C && !x->c8)) return fail(-1, "wfl_op_gemm_ex: null argument");
  // (fields the dispatch would pass over without a word)
  if (x->res_lo && !x->res) return fail(-1, "wfl_op_gemm_ex: res_lo without res");
  if (x->a8 != 0 && x->a8 != 1) return fail(-1, "wfl_op_gemm_ex: a8 is 0 or 1 here (2 / 3: wfl_op_gemm_mx)");
  if (x->a8 && !x->w8_scale) return fail(-1, "wfl_op_gemm_ex: a8 without w8_scale");
  if (x->c8 && !x->a8) return fail(-1, "wfl_op_gemm_ex: c8 without a8");
  if (x->stats_in && !x->ln_s) return fail(-1, "wfl_op_gemm_ex: stats_in without ln_s");
  if (x->acc_f32 && !x->out_f32) return fail(-1, "wfl_op_gemm_ex: acc_f32 without out_f32");
  if (x->clip_bias && !x->clip_idx) return fail(-1, "wfl_op_gemm_ex: clip_bias without clip_idx");
  GemmArgs g{};
  g.A = (const bf16_t*)x->A; g.lda = x->lda; g.cin = x->cin > 0 ? x->cin : x->K; g.tap_stride = x->tap_stride;
  g.W = (const bf16_t*)x->W; g.M = x->M; g.N = x->N; g.K = x->K; g.n_valid = x->n_valid; g.P = x->P; g.T = x->T;
  g.C = x->C; g.c_lo = (bf16_t*)x->c_lo; g.ldc = x->ldc; g.c_lead = x->c_lead; g.c_pitch = x->c_pitch;
  g.bias = x->bias; g.clip_bias = x->clip_bias; g.clip_idx = x->clip_idx; g.clip_ld = x->clip_ld; g.clip_T = x->clip_T;
  g.res = (const bf16_t*)x->res; g.res_lo = (const bf16_t*)x->res_lo; g.ldres = x->ldres; g.alpha = x->alpha;
  g.act = x->act; g.glu = x->glu; g.out_f32 = x->out_f32; g.acc_f32 = x->acc_f32;
  g.pos = (const bf16_t*)x->pos; g.ldpos = x->ldpos;
  g.ln_s = x->ln_s; g.ln_eps = x->ln_eps; g.stats_out = x->stats_out; g.stats_in = x->stats_in; g.stats_nsl = x->stats_nsl;
  g.stats_lead = x->stats_lead;
  g.w8_scale = x->w8_scale; g.a8 = x->a8; g.a8_scale = x->a8_scale; g.a8_lead = x->a8_lead; g.a8_static = x->a8_static;
  g.c8 = (unsigned char*)x->c8; g.ldc8 = x->ldc8; g.c8_inv_scale = x->c8_inv_scale; g.err = (unsigned*)x->status;
  // only the streaming kernel writes or reads row statistics: gemm256 / the 128-tile kernel would run and ignore them
  if ((g.stats_out || g.stats_in) && !wfl_gemm_stream_takes(g))
    return fail(-4, "wfl_op_gemm_ex: stats_out / stats_in on a launch the streaming kernel does not take");
  g_wfl_gemm_kernel_id = 0;
  const int r = wfl_launch_gemm(g, (hipStream_t)stream);
  if (r) return fail(r, "wfl_op_gemm_ex: invalid arguments, a combination no kernel takes, or launch failure (" + std::to_string(r) + ")");
  if (kernel_id) *kernel_id = g_wfl_gemm_kernel_id;
  return 0;
}

int32_t wfl_op_attention(const void* QK, int64_t ldqk, int64_t lead, const void* V, int64_t ldv, void* O, int64_t ldo, int32_t B, int32_t T,
                         int32_t P, int32_t heads, int32_t d, void* stream) {
  AttnArgs a{};
  a.QK = (const bf16_t*)QK; a.ldqk = ldqk; a.lead = lead; a.V = (const bf16_t*)V; a.ldv = ldv; a.O = (bf16_t*)O; a.ldo = ldo;
  a.B = B; a.T = T; a.P = P; a.heads = heads; a.d = d;
  const int r = wfl_launch_attention(a, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_attention: invalid arguments, unsupported head_dim or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_attention_ex(const void* QK, const void* QK_lo, int64_t ldqk, int64_t lead, const void* V, const void* V_lo, int64_t ldv,
                            void* O, void* O_lo, int64_t ldo, int32_t B, int32_t T, int32_t P, int32_t heads, int32_t d, const float* bias,
                            const float* gate, const int32_t* clip_T, void* O8, void* O8_lo, int64_t ldo8, float o8_scale, int32_t* status,
                            void* stream) {
  if (!QK || !V || (!O && !O8)) return fail(-1, "wfl_op_attention_ex: null argument");
  if (!QK_lo != !V_lo) return fail(-1, "wfl_op_attention_ex: QK_lo and V_lo go together");
  if ((O_lo && !O) || (O8_lo && !O8)) return fail(-1, "wfl_op_attention_ex: a low half without its high half");
  if (B <= 0 || T <= 0 || heads <= 0 || d % heads) return fail(-1, "wfl_op_attention_ex: empty batch or d not a whole number of heads");
  // (fields the dispatch would pass over without a word: the fp8 context has no split-precision or bf16-low-half form, the split kernels
  //  exist for four head sizes)
  if (O8 && (QK_lo || O_lo)) return fail(-4, "wfl_op_attention_ex: the fp8 context takes no QK_lo / V_lo / O_lo");
  if (QK_lo && d / heads != 32 && d / heads != 64 && d / heads != 128 && d / heads != 256)
    return fail(-4, "wfl_op_attention_ex: split precision at head_dim 32, 64, 128, 256 only");
  AttnArgs a{};
  a.QK = (const bf16_t*)QK; a.ldqk = ldqk; a.lead = lead; a.V = (const bf16_t*)V; a.ldv = ldv; a.O = (bf16_t*)O; a.ldo = ldo;
  a.B = B; a.T = T; a.P = P; a.heads = heads; a.d = d;
  a.bias = bias; a.gate = gate; a.clip_T = clip_T; a.O_lo = (bf16_t*)O_lo; a.QK_lo = (const bf16_t*)QK_lo; a.V_lo = (const bf16_t*)V_lo;
  a.O8 = (unsigned char*)O8; a.O8_lo = (unsigned char*)O8_lo; a.ldo8 = ldo8; a.o8_scale = o8_scale; a.err = (unsigned*)status;
  const int r = wfl_launch_attention(a, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_attention_ex: invalid arguments, a combination attention.hip has no kernel for, or launch failure (" +
                         std::to_string(r) + ")") : 0;
}

int32_t wfl_op_relpos_table(const float* rel_emb, const int32_t* bucket_of_delta, int32_t max_t, int32_t heads, int32_t T, float* table,
                            void* stream) {
  if (!rel_emb || !bucket_of_delta || !table || heads <= 0 || T <= 0) return fail(-1, "wfl_op_relpos_table: bad argument");
  const int r = wfl_launch_relpos_table(rel_emb, bucket_of_delta, max_t, heads, T, table, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_relpos_table: T > max_t or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_relpos_gate(const void* x, const void* x_lo, int64_t ldx, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t heads,
                           int32_t hd, const float* w8, const float* b8, const float* cst, float* gate, void* stream) {
  if (!x || !w8 || !b8 || !cst || !gate || B <= 0 || T <= 0 || heads <= 0 || hd <= 0) return fail(-1, "wfl_op_relpos_gate: bad argument");
  const int r = wfl_launch_relpos_gate((const bf16_t*)x, ldx, lead, B, P, T, heads, hd, w8, b8, cst, gate, (hipStream_t)stream,
                                       (const bf16_t*)x_lo);
  return r ? fail(r, "wfl_op_relpos_gate: head_dim or leading dimension not taken, or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_regroup(const void* x, int32_t d, int32_t groups, int32_t cpg, int64_t R, int64_t lead, int32_t B, int32_t P, int32_t T,
                       const int32_t* clip_T, void* xg, void* stream) {
  if (!x || !xg || groups <= 0 || cpg <= 0 || R <= 0 || B <= 0 || P <= 0) return fail(-1, "wfl_op_regroup: bad argument");
  const int r = wfl_launch_regroup((const bf16_t*)x, d, groups, cpg, R, lead, B, P, T, (bf16_t*)xg, (hipStream_t)stream, clip_T);
  return r ? fail(r, "wfl_op_regroup: channel split not taken or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_wav_stats(const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, double* stats, void* stream) {
  if (!wav || !stats) return fail(-1, "wfl_op_wav_stats: null argument");
  if (B <= 0 || L <= 0 || ldw < L) return fail(-1, "wfl_op_wav_stats: bad shape (B > 0, L > 0, ldw >= L)");
  const int r = wfl_launch_wav_stats(wav, ldw, B, L, stats, (hipStream_t)stream, lens);
  return r ? fail(r, "wfl_op_wav_stats: launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_clip_frames(const int32_t* lens, int32_t B, int32_t L, int32_t n, const int32_t* kernel, const int32_t* stride,
                           int32_t min_len, int32_t* out, void* stream) {
  if (!lens || !kernel || !stride || !out) return fail(-1, "wfl_op_clip_frames: null argument");
  if (B <= 0 || L < 0) return fail(-1, "wfl_op_clip_frames: bad shape (B > 0, L >= 0)");
  if (n < 1 || n > 8) return fail(-1, "wfl_op_clip_frames: 1 .. 8 levels");
  for (int i = 0; i < n; ++i)
    if (kernel[i] < 0 || stride[i] <= 0) return fail(-1, "wfl_op_clip_frames: kernel >= 0 and stride > 0 at every level");
  const int r = wfl_launch_clip_frames(lens, B, L, n, kernel, stride, min_len, out, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_clip_frames: launch failure (" + std::to_string(r) + ")") : 0;
}

// scratch of wfl_op_conv0's group mode: cstats [B][C][2] double, then cpart [B][time blocks of 512 frames][C][2] float
int64_t wfl_op_conv0_scratch_bytes(int32_t B, int32_t T0, int32_t C) {
  if (B <= 0 || T0 <= 0 || C <= 0) return 0;
  const int64_t nblk = ((int64_t)T0 + 511) / 512;
  return (int64_t)B * C * 2 * (int64_t)sizeof(double) + (int64_t)B * nblk * C * 2 * (int64_t)sizeof(float);
}

int32_t wfl_op_conv0(const float* wav, int64_t ldw, const int32_t* lens, int32_t B, int32_t L, const double* wstats, const float* w,
                     const float* bias, const float* gamma, const float* beta, int32_t C, int32_t T0, void* out, void* out_lo,
                     int64_t lead, int32_t P, int32_t group_norm, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!wav || !w || !gamma || !beta || !out) return fail(-1, "wfl_op_conv0: null argument");
  if (B <= 0 || L < 10 || ldw < L) return fail(-1, "wfl_op_conv0: bad shape (B > 0, L >= 10, ldw >= L)");
  if (C <= 0 || C % 8 || C > 512) return fail(-1, "wfl_op_conv0: C a multiple of 8, at most 512");
  if (T0 <= 0 || T0 > (L - 10) / 5 + 1 || P < T0 || lead < 0) return fail(-1, "wfl_op_conv0: 0 < T0 <= (L - 10) / 5 + 1, P >= T0, lead >= 0");
  Conv0Args c{};
  c.wav = wav; c.ldw = ldw; c.L = L; c.wstats = wstats; c.w = w; c.bias = bias; c.gamma = gamma; c.beta = beta;
  c.B = B; c.T0 = T0; c.C = C; c.lens = lens;
  c.out = (bf16_t*)out; c.out_lo = (bf16_t*)out_lo; c.lead = lead; c.P = P;
  if (group_norm) {
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < wfl_op_conv0_scratch_bytes(B, T0, C))
      return fail(-1, "wfl_op_conv0: group mode needs 16-byte aligned scratch of wfl_op_conv0_scratch_bytes(B, T0, C)");
    c.cstats = (double*)scratch;
    c.cpart = (float*)((char*)scratch + (size_t)B * C * 2 * sizeof(double));
  }
  const int r = wfl_launch_conv0(c, group_norm, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_conv0: launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_posconv(const void* xg, int64_t R, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t groups, int32_t cpg, int32_t taps,
                       const void* w, int64_t ldw, const float* bias, const void* res, const void* res_lo, void* out, void* out_lo,
                       int64_t ld, const int32_t* clip_T, void* stream) {
  if (!xg || !w || !bias || !res || !out || R <= 0 || B <= 0 || P <= 0) return fail(-1, "wfl_op_posconv: bad argument");
  if (groups <= 0 || groups > 16) return fail(-1, "wfl_op_posconv: 1 .. 16 groups");
  PosConvArgs pc{};
  pc.xg = (const bf16_t*)xg; pc.R = R; pc.lead = lead; pc.B = B; pc.P = P; pc.T = T; pc.groups = groups; pc.cpg = cpg; pc.taps = taps;
  for (int gi = 0; gi < groups; ++gi) { pc.w[gi] = (const bf16_t*)w + (long)gi * 64 * ldw; pc.bias[gi] = bias + gi * 64; }
  pc.ldw = ldw;
  pc.res = (const bf16_t*)res; pc.res_lo = (const bf16_t*)res_lo; pc.out = (bf16_t*)out; pc.out_lo = (bf16_t*)out_lo; pc.ld = ld;
  pc.clip_T = clip_T;
  const int r = wfl_launch_posconv(pc, (hipStream_t)stream);
  if (r == 1) return fail(-1, "wfl_op_posconv: shape not taken by posconv.hip (cpg % 8, even taps 4 .. 128, ldw >= 64 taps, lead >= taps / 2)");
  return r ? fail(r, "wfl_op_posconv: launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_layernorm_act(const void* x, const void* x_lo, int64_t ldx, void* y, void* y_lo, int64_t ldy, const float* gamma,
                             const float* beta, float eps, int64_t lead, int32_t B, int32_t P, int32_t T, int32_t C, int32_t n_div,
                             int32_t gelu, const int32_t* clip_T, void* stream) {
  if (!x || !y || !gamma || !beta || B <= 0 || T <= 0) return fail(-1, "wfl_op_layernorm_act: bad argument");
  const int r = wfl_launch_layernorm_act((const bf16_t*)x, ldx, (bf16_t*)y, ldy, gamma, beta, eps, lead, B, P, T, C, gelu, (hipStream_t)stream,
                                         (const bf16_t*)x_lo, (bf16_t*)y_lo, n_div, clip_T);
  return r ? fail(r, "wfl_op_layernorm_act: invalid arguments or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_layernorm_pair(const void* x, const void* x_lo, void* y1, void* y1_lo, void* y2, void* y2_lo, int64_t ld, const float* gamma1,
                              const float* beta1, const float* gamma2, const float* beta2, float eps, int64_t lead, int32_t B, int32_t P,
                              int32_t T, int32_t C, int32_t n_div, const int32_t* clip_T, void* stream) {
  if (!x || !y1 || !y2 || !gamma1 || !beta1 || !gamma2 || !beta2 || B <= 0 || T <= 0) return fail(-1, "wfl_op_layernorm_pair: bad argument");
  const int r = wfl_launch_layernorm_pair((const bf16_t*)x, (const bf16_t*)x_lo, (bf16_t*)y1, (bf16_t*)y1_lo, (bf16_t*)y2, (bf16_t*)y2_lo, ld,
                                          gamma1, beta1, gamma2, beta2, eps, lead, B, P, T, C, n_div, clip_T, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_layernorm_pair: invalid arguments, aliased y1 or launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_op_layernorm(const void* x, int64_t ldx, void* y, int64_t ldy, const float* gamma, const float* beta, float eps,
                         int64_t lead, int32_t B, int32_t P, int32_t T, int32_t C, void* stream) {
  const int r = wfl_launch_layernorm((const bf16_t*)x, ldx, (bf16_t*)y, ldy, gamma, beta, eps, lead, B, P, T, C, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_layernorm: invalid arguments or launch failure") : 0;
}

int32_t wfl_op_tag_decide(const float* logits, int64_t ldl, int32_t rows, int32_t C, float threshold, int32_t o_id, int32_t* ids,
                          int32_t* argmax, float* maxprob, void* stream) {
  if (!logits || !ids || !maxprob) return fail(-1, "wfl_op_tag_decide: null argument");
  TagArgs t{};
  t.logits = logits; t.ldl = ldl; t.rows = rows; t.C = C; t.threshold = threshold; t.o_id = o_id;
  t.ids = ids; t.argmax = argmax; t.maxprob = maxprob;
  const int r = wfl_launch_tag_decide(t, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_tag_decide: launch failure") : 0;
}

int64_t wfl_op_lstm_exchange_bytes(int32_t H, int32_t B) {
  if (!wfl_lstm_hidden_supported(H) || B < 1) return fail(-1, "wfl_op_lstm_exchange_bytes: " + (B < 1 ? std::string("B < 1") : lstm_hidden_refusal(H)));
  return wfl_lstm_exchange_bytes(H, B);
}

int32_t wfl_op_lstm(const float* gx, int64_t ldgx, const void* whh, const void* whh_lo, void* out, void* out_lo, int64_t ldo, int64_t lead,
                    int32_t B, int32_t T, int32_t P, int32_t H, int32_t U, const int32_t* clip_T, void* exchange, int64_t exchange_bytes,
                    int32_t* status, void* stream) {
  if (!gx || !whh || !out || !exchange || !status) return fail(-1, "wfl_op_lstm: null argument (gx, whh, out, exchange and status are required)");
  if (!whh_lo != !out_lo) return fail(-1, "wfl_op_lstm: whh_lo and out_lo go together");
  if (!wfl_lstm_hidden_supported(H)) return fail(-4, "wfl_op_lstm: " + lstm_hidden_refusal(H));
  if (U <= 0) U = wfl_lstm_units_per_wg(H);
  if (!lstm_units_ok(H, U)) return fail(-1, "wfl_op_lstm: U must be a multiple of 8, at most 32, divide H and leave at most 64 slices");
  if (B < 1 || T < 1 || P < T || lead < 0) return fail(-1, "wfl_op_lstm: bad shape (B >= 1, T >= 1, P >= T, lead >= 0)");
  if (ldgx % 4 || ldgx < 8L * H) return fail(-1, "wfl_op_lstm: ldgx must be a multiple of 4 and at least 8 H");
  if (ldo % 8 || ldo < 2L * H) return fail(-1, "wfl_op_lstm: ldo must be a multiple of 8 and at least 2 H");
  // the kernel's access widths: 16-byte gx, W_hh and granule loads, 4-byte stores of two hidden values
  if ((((uintptr_t)gx | (uintptr_t)whh | (uintptr_t)whh_lo | (uintptr_t)exchange) & 15) || (((uintptr_t)out | (uintptr_t)out_lo) & 3))
    return fail(-1, "wfl_op_lstm: gx, whh, whh_lo and exchange must be 16-byte aligned, out and out_lo 4-byte aligned");
  if (exchange_bytes < wfl_lstm_exchange_bytes(H, B))
    return fail(-1, "wfl_op_lstm: exchange_bytes is below wfl_op_lstm_exchange_bytes(H, B) = " + std::to_string(wfl_lstm_exchange_bytes(H, B)));
  LstmArgs la{};
  la.gx = gx; la.ldgx = ldgx; la.whh = (const bf16_t*)whh; la.whh_lo = (const bf16_t*)whh_lo; la.out = (bf16_t*)out; la.out_lo = (bf16_t*)out_lo;
  la.ldo = ldo; la.lead = lead; la.B = B; la.T = T; la.P = P; la.H = H; la.U = U; la.error = (unsigned*)status; la.clip_T = clip_T;
  const int r = wfl_launch_lstm(la, exchange, (hipStream_t)stream);
  return r ? fail(r, "wfl_op_lstm: launch failure (" + std::to_string(r) + ")") : 0;
}

int32_t wfl_gemm_profile_enable(wfl_model* m, int32_t on) {
  if (!m) return fail(-1, "null model");
  m->prof_on = on != 0;
  return 0;
}

int32_t wfl_gemm_profile_read(wfl_model* m, int32_t max_variants, int32_t* keys, int64_t* launches, double* total_ms,
                              double* total_flops, int32_t* n_variants, int32_t reset) {
  if (!m || !keys || !launches || !total_ms || !total_flops || !n_variants) return fail(-1, "wfl_gemm_profile_read: null argument");
  std::vector<double> ms(2048, 0.0);
  for (size_t i = 0; i < m->prof_used; ++i) {
    HIPCHK(hipEventSynchronize(m->prof.ev[i].second));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, m->prof.ev[i].first, m->prof.ev[i].second));
    ms[m->prof.key[i]] += t;
  }
  int n = 0;
  for (int k = 0; k < 2048 && n < max_variants; ++k)
    if (m->prof.launches[k]) {
      keys[n] = k; launches[n] = m->prof.launches[k]; total_ms[n] = ms[k]; total_flops[n] = m->prof.flops[k];
      ++n;
    }
  *n_variants = n;
  if (reset) {
    memset(m->prof.launches, 0, sizeof(m->prof.launches));
    memset(m->prof.flops, 0, sizeof(m->prof.flops));
    m->prof.key.clear();
    m->prof_used = 0;
  }
  return 0;
}
