// Viterbi forced alignment of a phoneme transcript over the frame logits of a clip (wfl_align, include/wfl_asr.h).
//
// Replaces the greedy string match of /root/reference/infer.py:30-60 (run at 193, 210-215, 312-319) when the caller asks for
// `postprocess.align: viterbi`: the search spells exactly the transcript, in order, one contiguous run of frames per token.
//
// States of a clip with N tokens: G_0, B_0, I_0, G_1, ..., B_{N-1}, I_{N-1}, G_N  (G_k = 3k, B_k = 3k+1, I_k = 3k+2, G_N = 3N).
//   G_k <- {G_k, I_{k-1}, B_{k-1}}     B_k <- {G_k, I_{k-1}, B_{k-1}}     I_k <- {I_k, B_k}       (first listed wins a tie)
//   start G_0 | B_0, end G_N | I_{N-1} | B_{N-1}; emission of G: max over the gap classes, of B_k / I_k: max over the token's
//   alternatives' B / I classes.  The decisions are taken on the raw logits (the per-frame log-sum-exp is common to every state);
//   it is subtracted only for the clip's score.
//
// One workgroup per clip; clips are independent, so a clip aligned alone equals the same clip in a batch bit for bit.
//   Forward pass: thread i owns the R consecutive token slots k = i R .. i R + R - 1 (all three states of each, slot N holds G_N
//   alone) in registers.  Only the first slot's G and B need the previous frame's B and I of token k - 1, i.e. the last slot of
//   thread i - 1: one float2 per thread goes through LDS, one barrier per frame.  The logits rows reach LDS in stages of F rows
//   (F C <= NT PR values), loaded into registers one stage ahead, so a frame's gathers (the token's classes and the gap classes)
//   are LDS reads.  Every 16 frames the block's maximum state score is subtracted from all states (and added to a double), so
//   the fp32 state scores never grow with T.
//   Backpointers: 2 bits per state per frame (the index of the chosen predecessor), WPT words per thread per frame.
//   Backtrace: from frame t in state s = 3k + j, frame t - 1 is in token k or k - 1, so ALIGN_W frames need the backpointer words
//   of at most ALIGN_W / R + 2 threads: the block loads such a window into LDS in one go and thread 0 walks ALIGN_W frames out of
//   LDS, T / ALIGN_W memory round trips in all.  The per-frame states go to `tok`, then every thread turns its frames into
//   (class id, token) and adds up its frames' log-sum-exp for the score.
#include "common.h"
#include "wfl_asr.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int ALIGN_MAX_TOKENS = 4096;
constexpr int ALIGN_MAX_CLASSES = 1024;
constexpr int ALIGN_W = 32;                 // backtrace window, frames
constexpr int ALIGN_CLIPS_PER_LAUNCH = 64;  // the clip table travels in the kernel arguments
constexpr int ALIGN_NGAP = 8;

struct AlignClip {
  long frame_off;  // first logits row of the clip
  long bp_off;     // backpointer words of the clip in the workspace
  int T, tok_off, N, clip;
};

struct AlignLaunch {
  const float* logits;
  long ldl;
  int C, o_id;
  const int* tok_cls;  // [total tokens][4][2]
  const int* gap_cls;  // [n_clips][8]
  unsigned* bp;
  int* ids;
  int* tok;
  float* score;
  int* status;
  int n;
  AlignClip clip[ALIGN_CLIPS_PER_LAUNCH];
};

template <int NT, int R>
struct Cfg {
  static constexpr int WPT = (6 * R + 31) / 32;          // backpointer words per thread per frame
  static constexpr int PR = NT >= 512 ? 8 : 16;          // staged logits values per thread
  static constexpr int NW = NT / 64;
  static constexpr int WIN = ALIGN_W * (ALIGN_W / R + 2) * WPT;
  static constexpr int OFF_ALT = 2 * NT * PR * 4;                  // ring: two stages of NT PR floats
  static constexpr int OFF_XCH = OFF_ALT + NT * R * 16;            // alternatives: one int4 (B | I << 16, -1 unused) per slot
  static constexpr int OFF_WMAX = OFF_XCH + 2 * NT * 8;            // neighbour exchange: [2][NT] float2
  static constexpr int OFF_RED = OFF_WMAX + 64;                    // per-wave maxima (renormalisation)
  static constexpr int OFF_WIN = OFF_RED + 8 * 16;                 // per-wave double sums
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int LDS = OFF_MISC + 64;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NT, int R>
__global__ __launch_bounds__(NT) void align_kernel(AlignLaunch a) {
  using K = Cfg<NT, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  float2* xch = (float2*)(lds + K::OFF_XCH);
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  unsigned* win = (unsigned*)(lds + K::OFF_WIN);
  int* misc = (int*)(lds + K::OFF_MISC);
  float* fin = (float*)(misc + 4);

  const AlignClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = cl.T, N = cl.N, C = a.C;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  int* ids = a.ids + cl.frame_off;
  int* tokp = a.tok + cl.frame_off;
  const float NEG = -INFINITY;

  int st = 0;
  if (N > NT * R - 1 || N > ALIGN_MAX_TOKENS) st = 2;
  else if (T < N) st = 1;
  int g[ALIGN_NGAP];
  if (st == 0) {
    if (tid == 0) misc[0] = 0;
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = tid * R + r;
      int4 v = make_int4(-1, -1, -1, -1);          // the used alternatives first
      if (k < N) {
        const int* tc = a.tok_cls + (long)(cl.tok_off + k) * 8;
        int n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = tc[2 * j], i = tc[2 * j + 1];
          if (b == -1 && i == -1) continue;                        // an unused alternative
          if (b < 0 || b >= C || i < 0 || i >= C) { bad = true; continue; }
          const int pk = b | (i << 16);
          if (n == 0) v.x = pk; else if (n == 1) v.y = pk; else if (n == 2) v.z = pk; else v.w = pk;
          ++n;
        }
        if (n == 0) bad = true;
      }
      alt[k] = v;
    }
    int ng = 0;
#pragma unroll
    for (int j = 0; j < ALIGN_NGAP; ++j) {
      g[j] = a.gap_cls[(long)cl.clip * ALIGN_NGAP + j];
      if (g[j] == -1) continue;
      if (g[j] < 0 || g[j] >= C) { bad = true; g[j] = -1; }
      else ++ng;
    }
    if (ng == 0) bad = true;
    if (bad) misc[0] = 1;
    __syncthreads();
    if (misc[0]) st = 4;
  }
  if (st != 0 || T == 0) {
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = st; }
    return;
  }

  // ---- forward pass
  const int F = min(32, NT * K::PR / C);       // rows per stage (C <= ALIGN_MAX_CLASSES <= NT PR: F >= 1)
  const int SE = F * C;
  int rc[K::PR];                               // (row << 16 | column) of this thread's staged values inside a stage, -1 none
#pragma unroll
  for (int i = 0; i < K::PR; ++i) {
    const int e = tid + i * NT;
    rc[i] = e < SE ? ((e / C) << 16) | (e % C) : -1;
  }
  float pre[K::PR];
  auto load_stage = [&](int c) {
    const int t0 = c * F;
#pragma unroll
    for (int i = 0; i < K::PR; ++i) {
      const int row = t0 + (rc[i] >> 16);
      pre[i] = (rc[i] >= 0 && row < T) ? Z[(long)row * a.ldl + (rc[i] & 0xffff)] : 0.f;
    }
  };
  auto store_stage = [&](int c) {
    float* h = ring + (c & 1) * NT * K::PR;
#pragma unroll
    for (int i = 0; i < K::PR; ++i)
      if (rc[i] >= 0) h[tid + i * NT] = pre[i];
  };

  float G[R], B[R], I[R];
#pragma unroll
  for (int r = 0; r < R; ++r) G[r] = B[r] = I[r] = NEG;
  if (tid == 0) G[0] = 0.f;                    // a virtual frame -1 in G_0: frame 0 starts in G_0 or B_0
  xch[NT + tid] = make_float2(NEG, NEG);
  load_stage(0);
  store_stage(0);
  load_stage(1);
  __syncthreads();

  int4 av[R];                                   // this thread's slots' alternatives, for the whole forward pass
#pragma unroll
  for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  unsigned* bp = a.bp + cl.bp_off;
  double acc = 0.0;                            // what the renormalisations subtracted
  float sub = 0.f;
  int c = 0, tin = 0;
  for (int t = 0; t < T; ++t, ++tin) {
    if (tin == F) {
      ++c;
      tin = 0;
      store_stage(c);
      __syncthreads();
      load_stage(c + 1);
    }
    const float* row = ring + (c & 1) * NT * K::PR + tin * C;
    float eg = NEG;
#pragma unroll
    for (int j = 0; j < ALIGN_NGAP; ++j)
      if (g[j] >= 0) eg = fmaxf(eg, row[g[j]]);
    float2 nb = tid > 0 ? xch[((t + 1) & 1) * NT + tid - 1] : make_float2(NEG, NEG);
    nb.x -= sub;
    nb.y -= sub;
    unsigned bits[K::WPT];
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bits[w] = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {         // descending: slot r - 1's previous-frame values are still in place
      const int k = tid * R + r;
      const float pB1 = r ? B[r > 0 ? r - 1 : 0] : nb.x;
      const float pI1 = r ? I[r > 0 ? r - 1 : 0] : nb.y;
      float m = G[r];
      unsigned cg = 0;
      if (pI1 > m) { m = pI1; cg = 1; }
      if (pB1 > m) { m = pB1; cg = 2; }
      float mi = I[r];
      unsigned ci = 0;
      if (B[r] > mi) { mi = B[r]; ci = 1; }
      float eb = NEG, ei = NEG;
      if (k < N) {
        const int p[4] = {av[r].x, av[r].y, av[r].z, av[r].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (p[j] < 0) break;
          eb = fmaxf(eb, row[p[j] & 0xffff]);
          ei = fmaxf(ei, row[p[j] >> 16]);
        }
      }
      G[r] = k <= N ? m + eg : NEG;
      B[r] = m + eb;
      I[r] = mi + ei;
      bits[(6 * r) >> 5] |= cg << ((6 * r) & 31);
      bits[(6 * r + 2) >> 5] |= cg << ((6 * r + 2) & 31);
      bits[(6 * r + 4) >> 5] |= ci << ((6 * r + 4) & 31);
    }
    xch[(t & 1) * NT + tid] = make_float2(B[R - 1], I[R - 1]);
    unsigned* bw = bp + ((long)t * NT + tid) * K::WPT;
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bw[w] = bits[w];
    const bool renorm = (t & 15) == 15;
    if (renorm) {
      float lm = NEG;
#pragma unroll
      for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(G[r], fmaxf(B[r], I[r])));
      lm = wave_max(lm);
      if (lane == 0) wmax[wave] = lm;
    }
    __syncthreads();
    sub = 0.f;
    if (renorm) {
      float M = wmax[0];
#pragma unroll
      for (int w = 1; w < K::NW; ++w) M = fmaxf(M, wmax[w]);
#pragma unroll
      for (int r = 0; r < R; ++r) { G[r] -= M; B[r] -= M; I[r] -= M; }
      sub = M;
      acc += (double)M;
    }
  }

  // ---- the best end state
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    if (k == N) fin[0] = G[r];
    if (k == N - 1) { fin[1] = I[r]; fin[2] = B[r]; }
  }
  __syncthreads();
  float best = 0.f;
  if (tid == 0) {
    best = fin[0];
    int s = 3 * N;
    if (N >= 1) {
      if (fin[1] > best) { best = fin[1]; s = 3 * N - 1; }
      if (fin[2] > best) { best = fin[2]; s = 3 * N - 2; }
    }
    misc[1] = s;
  }
  __syncthreads();

  // ---- backtrace, ALIGN_W frames per window
  int s = misc[1];
  for (int thi = T - 1; thi >= 1;) {
    const int tlo = max(1, thi - ALIGN_W + 1);
    const int nf = thi - tlo + 1;
    const int k_hi = min(max(s / 3, 0), N);
    const int k_lo = max(0, k_hi - nf);
    const int th_lo = k_lo / R, th_hi = k_hi / R;
    const int nw = (th_hi - th_lo + 1) * K::WPT;
    for (int e = tid; e < nf * nw; e += NT) {
      const int f = e / nw, w = e - f * nw;
      win[e] = bp[((long)(tlo + f) * NT + th_lo) * K::WPT + w];
    }
    __syncthreads();
    if (tid == 0) {
      for (int t = thi; t >= tlo; --t) {
        tokp[t] = s;
        const int k = s / 3, j = s - 3 * k;
        const int th = k / R, r = k - th * R;
        const int pos = 2 * (3 * r + j);
        const int wi = (t - tlo) * nw + (th - th_lo) * K::WPT + (pos >> 5);
        const unsigned ch = (wi >= 0 && wi < nf * nw) ? (win[wi] >> (pos & 31)) & 3u : 0u;
        s = j == 2 ? s - (int)ch : 3 * k - (int)ch;
        s = max(s, 0);
      }
      misc[1] = s;
    }
    __syncthreads();
    s = misc[1];
    thi = tlo - 1;
  }
  if (tid == 0) tokp[0] = s;
  __syncthreads();

  // ---- states -> (class id, token); the score's per-frame log-sum-exp
  double lsum = 0.0;
  for (int t = tid; t < T; t += NT) {
    const float* z = Z + (long)t * a.ldl;
    float m = z[0];
    for (int q = 1; q < C; ++q) m = fmaxf(m, z[q]);
    float se = 0.f;
    for (int q = 0; q < C; ++q) se += __expf(z[q] - m);
    lsum += (double)m + log((double)se);
    const int sv = tokp[t];
    const int k = sv / 3, j = sv - 3 * k;
    int id = a.o_id, tk = -1;
    if (j != 0 && k < N) {
      const int4 v = alt[k];
      const int p[4] = {v.x, v.y, v.z, v.w};
      float bv = NEG;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (p[q] < 0) break;
        const int col = j == 2 ? p[q] >> 16 : p[q] & 0xffff;
        const float x = z[col];
        if (q == 0 || x > bv) { bv = x; id = col; }
      }
      tk = k;
    }
    ids[t] = id;
    tokp[t] = tk;
  }
  lsum = wave_sum(lsum);
  if (lane == 0) red[wave] = lsum;
  __syncthreads();
  if (tid == 0) {
    double ls = 0.0;
    for (int w = 0; w < K::NW; ++w) ls += red[w];
    a.score[cl.clip] = (float)((double)best + acc - ls);
    a.status[cl.clip] = 0;
  }
}

// configuration by token count: (threads, slots per thread); NT R - 1 >= N
constexpr int kCfgMaxN[5] = {127, 511, 1023, 2047, ALIGN_MAX_TOKENS};
constexpr int kCfgWords[5] = {64 * Cfg<64, 2>::WPT, 256 * Cfg<256, 2>::WPT, 256 * Cfg<256, 4>::WPT, 256 * Cfg<256, 8>::WPT,
                              512 * Cfg<512, 9>::WPT};
static_assert(64 * 2 - 1 >= 127 && 256 * 2 - 1 >= 511 && 256 * 4 - 1 >= 1023 && 256 * 8 - 1 >= 2047 && 512 * 9 - 1 >= 4096, "slots");

int cfg_of(int N) {
  for (int c = 0; c < 5; ++c)
    if (N <= kCfgMaxN[c]) return c;
  return -1;
}

long clip_words(int T, int N) {
  const int c = cfg_of(N);
  if (c < 0 || T < N || T <= 0) return 0;
  return ((long)T * kCfgWords[c] + 63) / 64 * 64;      // (256-byte aligned)
}

template <int NT, int R>
int launch_cfg(const AlignLaunch& a, hipStream_t s) {
  auto k = align_kernel<NT, R>;
  constexpr int lds = Cfg<NT, R>::LDS;
  static WflOncePerDevice attr_once;
  if (attr_once.need()) {
    if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
      return wfl_fail(-2, "wfl_align: cannot reserve the kernel's LDS");
  }
  hipLaunchKernelGGL(k, dim3(a.n), dim3(NT), lds, s, a);
  return hipGetLastError() == hipSuccess ? 0 : wfl_fail(-3, "wfl_align: launch failed");
}

int launch(int cfg, const AlignLaunch& a, hipStream_t s) {
  switch (cfg) {
    case 0: return launch_cfg<64, 2>(a, s);
    case 1: return launch_cfg<256, 2>(a, s);
    case 2: return launch_cfg<256, 4>(a, s);
    case 3: return launch_cfg<256, 8>(a, s);
    default: return launch_cfg<512, 9>(a, s);
  }
}

}  // namespace

extern "C" {

int64_t wfl_align_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  if (n_clips < 0 || (n_clips > 0 && (!n_frames_host || !n_tok_host))) return -1;
  int64_t words = 0;
  for (int b = 0; b < n_clips; ++b) {
    if (n_frames_host[b] < 0 || n_tok_host[b] < 0) return -1;
    words += clip_words(n_frames_host[b], n_tok_host[b]);
  }
  return words * 4;
}

int32_t wfl_align(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                  const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls, const int32_t* gap_cls, int32_t n_clips,
                  void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  if (C < 1 || C > ALIGN_MAX_CLASSES) return wfl_fail(-1, "wfl_align: C must be 1 .. 1024");
  if (o_id < 0 || o_id >= C) return wfl_fail(-1, "wfl_align: o_id out of range");
  if (ldl < C) return wfl_fail(-1, "wfl_align: ldl < C");
  if (n_clips < 0) return wfl_fail(-1, "wfl_align: n_clips < 0");
  if (n_clips == 0) return 0;
  if (!frame_off_host || !n_frames_host || !tok_off_host || !n_tok_host)
    return wfl_fail(-1, "wfl_align: null host array");
  const int64_t need = wfl_align_workspace_bytes(n_frames_host, n_tok_host, n_clips);
  if (need < 0) return wfl_fail(-1, "wfl_align: negative frame or token count");
  bool any_tok = false, any_frame = false;
  for (int b = 0; b < n_clips; ++b) {
    if (frame_off_host[b] < 0 || tok_off_host[b] < 0) return wfl_fail(-1, "wfl_align: negative offset");
    any_tok |= n_tok_host[b] > 0;
    any_frame |= n_frames_host[b] > 0;
  }
  if (!score || !status || !gap_cls || (any_tok && !tok_cls) || (any_frame && (!logits || !ids || !tok)))
    return wfl_fail(-1, "wfl_align: null device pointer");
  if (workspace_bytes < need || (need > 0 && !workspace))
    return wfl_fail(-1, "wfl_align: workspace too small (wfl_align_workspace_bytes)");
  hipStream_t s = (hipStream_t)stream;
  AlignLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.tok_cls = tok_cls; a.gap_cls = gap_cls;
  a.bp = (unsigned*)workspace; a.ids = ids; a.tok = tok; a.score = score; a.status = status;
  long off = 0;
  std::vector<AlignClip> by_cfg[5];
  for (int b = 0; b < n_clips; ++b) {
    const int T = n_frames_host[b], N = n_tok_host[b];
    int cfg = cfg_of(N);
    if (cfg < 0) cfg = 0;                       // over the cap: the kernel reports status 2
    by_cfg[cfg].push_back(AlignClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b});
    off += clip_words(T, N);
  }
  for (int cfg = 0; cfg < 5; ++cfg) {
    for (size_t i = 0; i < by_cfg[cfg].size(); i += ALIGN_CLIPS_PER_LAUNCH) {
      a.n = (int)std::min<size_t>(ALIGN_CLIPS_PER_LAUNCH, by_cfg[cfg].size() - i);
      for (int j = 0; j < a.n; ++j) a.clip[j] = by_cfg[cfg][i + j];
      const int rc = launch(cfg, a, s);
      if (rc) return rc;
    }
  }
  return 0;
}

}  // extern "C"
