// The forced-alignment lattice of wfl_align (csrc/align.hip, the max-product search), wfl_align_posterior (csrc/align_posterior.h,
// the sum-product sweeps) and wfl_align_edits (csrc/align_edits.hip: the same sweeps once more, kept per frame, and from them the
// score of every single substitution and deletion of the transcript, and wfl_align_insertions beside it: of every single insertion),
// defined ONCE: a change made here reaches all of them, so the posterior and the edit scores always speak of the lattice the search
// ran on.  The sweeps themselves follow the same rule: the max-product step is csrc/align.hip's own, and the sum-product sweeps --
// alpha, beta, their renormalisation, the per-frame log-sum-exp, logZ -- are written once in csrc/lattice_sums.h, on the pieces below,
// for post_kernel and edits_fb_kernel both (csrc/align.hip does not include that header).
//
//   device  caps and constants, the per-clip record, the wave reductions, the (threads, slots per thread) configurations and their
//           dispatch, the shared part of the LDS layout, lattice setup (status 0 / 1 / 2 / 4, the alternatives in LDS, the gap classes in
//           registers), the staged logits ring, the emission gathers, the start-window mask of the windowed entries (win_mask: ONE mask
//           for the search and for both sweeps of the sums), the minimum-duration chain of wfl_align_min_duration (chain_out / chain_shift:
//           the search and alpha) and its mirror for beta (chain_in / chain_shift_back: wfl_align_min_duration_posterior), the two
//           halves of the block-maximum renormalisation, the end states
//   host    the argument checks the ABI entries share, "group the clips by configuration, hand out workspace offsets, launch at most
//           64 clips at a time", and the launch that reserves a kernel's dynamic LDS once per device
//
// The BIO-grammar decodes (csrc/decode.hip, csrc/decode_bigram.hip, csrc/decode_posterior.hip) are a different search, the classes as
// states; what they share lives in csrc/bio_grammar.h.  From here that header takes the class cap, the clips-per-launch constant, round64,
// wave_max / wave_sum and the host's fail, check_workspace, launch_clips and reserve_lds, nothing of the lattice.
#pragma once
#include "common.h"

#include <math.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace lattice {

constexpr int MAX_TOKENS = 4096;
constexpr int MAX_CLASSES = 1024;
constexpr int NGAP = 8;               // gap classes per clip
constexpr int CLIPS_PER_LAUNCH = 64;  // the clip table travels in the kernel arguments
constexpr int RENORM = 16;            // frames between two renormalisations of the state scores
constexpr int FMAX = 32;              // staged logits rows per stage, at most

struct LatClip {
  long frame_off;  // first logits row of the clip
  long ws_off;     // the clip's workspace, in the kernel's 4-byte units
  int T, tok_off, N, clip;
};

__host__ __device__ constexpr long round64(long x) { return (x + 63) / 64 * 64; }

static __device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

static __device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- configurations by token count: (threads NT, slots per thread R), NT R - 1 >= N.  Thread i owns the token slots i R .. i R + R - 1.
template <int NT_, int R_>
struct Shape {
  static constexpr int NT = NT_, R = R_;
};
constexpr int NCFG = 5;
constexpr int kCfgMaxN[NCFG] = {127, 511, 1023, 2047, MAX_TOKENS};
static_assert(64 * 2 - 1 >= 127 && 256 * 2 - 1 >= 511 && 256 * 4 - 1 >= 1023 && 256 * 8 - 1 >= 2047 && 512 * 9 - 1 >= MAX_TOKENS, "slots");

// f(Shape<NT, R>()) of configuration `cfg`
template <class F>
auto dispatch_cfg(int cfg, F&& f) {
  switch (cfg) {
    case 0: return f(Shape<64, 2>());
    case 1: return f(Shape<256, 2>());
    case 2: return f(Shape<256, 4>());
    case 3: return f(Shape<256, 8>());
    default: return f(Shape<512, 9>());
  }
}

// the smallest configuration that holds N tokens; NCFG: N is over the cap (each caller has its own rule for that)
inline int cfg_of(int N) {
  for (int c = 0; c < NCFG; ++c)
    if (N <= kCfgMaxN[c]) return c;
  return NCFG;
}

// ---- LDS both kernels lay out the same way: [ring: two stages of NT PR floats] [alt: one int4 per slot] [X bytes of the kernel's own: its
// neighbour exchange] [per-wave maxima] [per-wave double sums] [the kernel's own, from OFF_OWN on]
template <int NT, int R, int X>
struct LdsBase {
  static constexpr int PR = NT >= 512 ? 8 : 16;  // staged logits values per thread
  static constexpr int NW = NT / 64;
  static constexpr int OFF_ALT = 2 * NT * PR * 4;
  static constexpr int OFF_X = OFF_ALT + NT * R * 16;
  static constexpr int OFF_WMAX = OFF_X + X;
  static constexpr int OFF_RED = OFF_WMAX + 64;
  static constexpr int OFF_OWN = OFF_RED + 8 * 16;
};

// ---- a token's alternatives: up to 4 (B class, I class) pairs, packed B | I << 16 into one int4, the used ones first, -1 unused
template <class F>
static __device__ __forceinline__ void for_each_alt(const int4& v, F f) {   // f(index, B class, I class)
  const int p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] < 0) break;
    f(j, p[j] & 0xffff, p[j] >> 16);
  }
}

// emission of a token's B and I states / of a gap state on a staged row: the maximum over the alternatives / over the gap classes
static __device__ __forceinline__ void tok_emission(const float* row, const int4& v, float& eb, float& ei) {
  eb = -INFINITY;
  ei = -INFINITY;
  for_each_alt(v, [&](int, int b, int i) {
    eb = fmaxf(eb, row[b]);
    ei = fmaxf(ei, row[i]);
  });
}

static __device__ __forceinline__ float gap_emission(const float* row, const int (&g)[NGAP]) {
  float eg = -INFINITY;
#pragma unroll
  for (int j = 0; j < NGAP; ++j)
    if (g[j] >= 0) eg = fmaxf(eg, row[g[j]]);
  return eg;
}

// ---- start windows (wfl_align_windowed, wfl_align_posterior_windowed): token k may open, i.e. be in B_k, only at a frame lo <= t <= hi
// (int32, inclusive; lo > hi: never).  That is EB_t(k) = -inf outside the window, and THE mask is win_mask: the max-product step, alpha
// and both gathers of beta go through it, so the search and the sums run on one lattice.  The table has 36 KB at the cap and the largest
// posterior configuration has no such LDS left, so every thread keeps the windows of its own R slots in registers (load_windows); the
// backward sweep takes the next thread's first slot as well (load_window).
constexpr int WIN_OPEN_HI = 0x7fffffff;

static __device__ __forceinline__ float win_mask(float eb, int t, const int2& w) { return (t >= w.x && t <= w.y) ? eb : -INFINITY; }

static __device__ __forceinline__ int2 load_window(const int* tok_win, int tok_off, int k, int N) {   // slots past the tokens: open
  const int* p = tok_win + (long)(tok_off + k) * 2;
  return k < N ? make_int2(p[0], p[1]) : make_int2(0, WIN_OPEN_HI);
}

template <int R>
static __device__ __forceinline__ void load_windows(const int* tok_win, int tok_off, int N, int2 (&w)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) w[r] = load_window(tok_win, tok_off, threadIdx.x * R + r, N);
}

// ---- minimum durations (wfl_align_min_duration): token k occupies at least D_k frames, 1 <= D_k <= MAX_MIN_FRAMES.  A run is frame 1 in
// B_k, frames 2 .. D_k - 1 in the chain states H_k^2 .. H_k^{D_k - 1} (which emit EI as I_k does), every later frame in I_k, and the
// token is left from I_k alone (from B_k as well where D_k == 1).  The chain of a slot is MAX_MIN_FRAMES - 2 floats in registers,
// h[j] = H^{j + 2}, -inf where the token's D_k has no such state.  Every step is an unrolled select on D_k: no register array is
// indexed dynamically.
constexpr int MAX_MIN_FRAMES = 8;
constexpr int CHAIN = MAX_MIN_FRAMES - 2;

static __device__ __forceinline__ int load_min(const int* tok_min, int tok_off, int k, int N) {   // slots past the tokens: 1
  return k < N ? tok_min[tok_off + k] : 1;
}

// X_k of the frame before: what I_k may be entered from, H_k^{D_k - 1} for D_k >= 3, B_k itself for D_k <= 2
static __device__ __forceinline__ float chain_out(float b, const float (&h)[CHAIN], int d) {
  float x = b;
#pragma unroll
  for (int j = 0; j < CHAIN; ++j) x = d == j + 3 ? h[j] : x;
  return x;
}

// one frame: H^2 <- B + EI, H^j <- H^{j-1} + EI (b and h of the frame before), the states D_k does not reach stay -inf
static __device__ __forceinline__ void chain_shift(float (&h)[CHAIN], float b, float ei, int d) {
#pragma unroll
  for (int j = CHAIN - 1; j >= 1; --j) h[j] = j + 3 <= d ? h[j - 1] + ei : -INFINITY;
  h[0] = 3 <= d ? b + ei : -INFINITY;
}

// ---- the chain seen from behind (wfl_align_min_duration_posterior's beta): a delay line per slot, the mirror of h[].  c[e - 1] is beta of
// the chain state that is e frames before I_k, e = 1 .. MAX_MIN_FRAMES - 1: H_k^j sits at e = D_k - j, B_k itself at e = D_k - 1.  The
// shift needs no select on D_k (the entries past D_k - 1 are never read); the one select is chain_in, where B_k is read.
constexpr int CHAIN_BACK = MAX_MIN_FRAMES - 1;

// beta(B_k) of a frame: beta(I_k) of that frame where D_k == 1 (the same successors), the delay line's entry D_k - 1 elsewhere
static __device__ __forceinline__ float chain_in(float bi, const float (&c)[CHAIN_BACK], int d) {
  float b = bi;
#pragma unroll
  for (int j = 0; j < CHAIN_BACK; ++j) b = d == j + 2 ? c[j] : b;
  return b;
}

// one frame back: beta_{t-1} of the state in front of I_k is beta_t(I_k) + EI_t, of every other chain state beta_t of its successor + EI_t
static __device__ __forceinline__ void chain_shift_back(float (&c)[CHAIN_BACK], float bi, float ei) {
#pragma unroll
  for (int j = CHAIN_BACK - 1; j >= 1; --j) c[j] = c[j - 1] + ei;
  c[0] = bi + ei;
}

// ---- lattice setup of a clip -> status: 2 over the cap (of the ABI or of this configuration), 1 fewer frames than tokens, 4 a class id
// out of range / a token without alternative / no gap class, 0: alt[] (LDS, visible to the block) and g[] (-1 unused) hold the lattice.
// `flag`: one LDS word.  The status is the same in every thread.  ANY_T (wfl_align_optional alone, whose paths may skip tokens): fewer
// frames than tokens is no status here, only "tokens and no frame" is; the search itself finds a clip without path.
template <int NT, int R, bool ANY_T = false>
static __device__ __forceinline__ int lattice_setup(const LatClip& cl, int C, const int* tok_cls, const int* gap_cls, int4* alt, int* flag,
                                                    int (&g)[NGAP]) {
  const int tid = threadIdx.x, N = cl.N;
  if (N > NT * R - 1 || N > MAX_TOKENS) return 2;
  if (ANY_T ? (cl.T == 0 && N > 0) : cl.T < N) return 1;
  if (tid == 0) *flag = 0;
  __syncthreads();
  bool bad = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    int4 v = make_int4(-1, -1, -1, -1);
    if (k < N) {
      const int* tc = tok_cls + (long)(cl.tok_off + k) * 8;   // [4][2]
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
  for (int j = 0; j < NGAP; ++j) {
    g[j] = gap_cls[(long)cl.clip * NGAP + j];
    if (g[j] == -1) continue;
    if (g[j] < 0 || g[j] >= C) { bad = true; g[j] = -1; }
    else ++ng;
  }
  if (ng == 0) bad = true;
  if (bad) *flag = 1;
  __syncthreads();
  return *flag ? 4 : 0;
}

// ---- the logits rows of a clip, staged through the LDS ring: stage c = rows c F .. c F + F - 1 (F C <= NT PR values), loaded into
// registers one stage ahead of its store, so a frame's gathers are LDS reads
template <int NT, int PR>
struct LogitStages {
  const float* Z;
  long ldl;
  int T, C, F;
  float* ring;
  int rc[PR];     // (row << 16 | column) of this thread's staged values inside a stage, -1 none
  float pre[PR];

  __device__ __forceinline__ LogitStages(const float* Z_, long ldl_, int T_, int C_, float* ring_)
      : Z(Z_), ldl(ldl_), T(T_), C(C_), F(min(FMAX, NT * PR / C_)), ring(ring_) {   // (C <= MAX_CLASSES <= NT PR: F >= 1)
    const int SE = F * C;
#pragma unroll
    for (int i = 0; i < PR; ++i) {
      const int e = threadIdx.x + i * NT;
      rc[i] = e < SE ? ((e / C) << 16) | (e % C) : -1;
    }
  }
  __device__ __forceinline__ void load(int c, bool exists = true) {   // exists: false for a stage in front of the clip (backward sweeps)
    const int t0 = c * F;
#pragma unroll
    for (int i = 0; i < PR; ++i) {
      const int row = t0 + (rc[i] >> 16);
      pre[i] = (rc[i] >= 0 && exists && row < T) ? Z[(long)row * ldl + (rc[i] & 0xffff)] : 0.f;
    }
  }
  __device__ __forceinline__ void store(int c) {
    float* h = ring + (c & 1) * NT * PR;
#pragma unroll
    for (int i = 0; i < PR; ++i)
      if (rc[i] >= 0) h[threadIdx.x + i * NT] = pre[i];
  }
  __device__ __forceinline__ const float* row(int c, int tin) const { return ring + (c & 1) * NT * PR + tin * C; }
};

// ---- renormalisation by the block's maximum state score, around the frame's ONE barrier (which stays in the caller, shared with the
// neighbour exchange): renorm_publish(this thread's maximum) before it, M = renorm_max() after it.  What to do with an M of -inf is the
// caller's choice.
static __device__ __forceinline__ void renorm_publish(float lm, float* wmax) {
  lm = wave_max(lm);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = lm;
}

template <int NW>
static __device__ __forceinline__ float renorm_max(const float* wmax) {
  float M = wmax[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) M = fmaxf(M, wmax[w]);
  return M;
}

// ---- the end states of the last frame to LDS: fin[0] = G_N, fin[1] = I_{N-1}, fin[2] = B_{N-1} (the last two only for N >= 1)
template <int R>
static __device__ __forceinline__ void publish_end_states(int N, const float (&G)[R], const float (&B)[R], const float (&I)[R], float* fin) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = threadIdx.x * R + r;
    if (k == N) fin[0] = G[r];
    if (k == N - 1) { fin[1] = I[r]; fin[2] = B[r]; }
  }
}

// =================================================================================================================== host side
inline int fail(const char* fn, int code, const char* what) { return wfl_fail(code, (std::string(fn) + ": " + what).c_str()); }

inline int check_workspace(const char* fn, int64_t need, const void* workspace, int64_t workspace_bytes) {
  if (workspace_bytes < need || (need > 0 && !workspace))
    return fail(fn, -1, (std::string("workspace too small (") + fn + "_workspace_bytes)").c_str());
  return 0;
}

// bytes of a ragged batch's workspace, words(T, N) 4-byte units per clip; -1: a null array or a negative count
template <class Words>
int64_t clips_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips, Words words) {
  if (n_clips < 0 || (n_clips > 0 && (!n_frames_host || !n_tok_host))) return -1;
  int64_t sum = 0;
  for (int b = 0; b < n_clips; ++b) {
    if (n_frames_host[b] < 0 || n_tok_host[b] < 0) return -1;
    sum += words(n_frames_host[b], n_tok_host[b]);
  }
  return sum * 4;
}

// the arguments wfl_align and wfl_align_posterior share (`need`: the function's own workspace_bytes of the batch).  any_tok / any_frame
// come back for the caller's check of its device pointers.
inline int check_clip_args(const char* fn, int C, int o_id, int64_t ldl, const int64_t* frame_off_host, const int32_t* n_frames_host,
                           const int32_t* tok_off_host, const int32_t* n_tok_host, int n_clips, int64_t need, bool& any_tok,
                           bool& any_frame) {
  if (C < 1 || C > MAX_CLASSES) return fail(fn, -1, "C must be 1 .. 1024");
  if (o_id < 0 || o_id >= C) return fail(fn, -1, "o_id out of range");
  if (ldl < C) return fail(fn, -1, "ldl < C");
  if (n_clips < 0) return fail(fn, -1, "n_clips < 0");
  if (n_clips == 0) return 0;
  if (!frame_off_host || !n_frames_host || !tok_off_host || !n_tok_host) return fail(fn, -1, "null host array");
  if (need < 0) return fail(fn, -1, "negative frame or token count");
  any_tok = any_frame = false;
  for (int b = 0; b < n_clips; ++b) {
    if (frame_off_host[b] < 0 || tok_off_host[b] < 0) return fail(fn, -1, "negative offset");
    any_tok |= n_tok_host[b] > 0;
    any_frame |= n_frames_host[b] > 0;
  }
  return 0;
}

// Clips into a.clip[] by group, the workspace offsets handed out in clip order, at most CLIPS_PER_LAUNCH clips per launch.
//   make(b, ws_off, clip&, group&) fills clip b's record and its group (< NG) and returns the clip's workspace units
//   fire(group, a) launches a.n clips, -> 0 or the error
template <int NG, class Launch, class Make, class Fire>
int launch_clips(Launch& a, int n_clips, Make make, Fire fire) {
  using Clip = std::decay_t<decltype(a.clip[0])>;
  std::vector<Clip> by_group[NG];
  long off = 0;
  for (int b = 0; b < n_clips; ++b) {
    Clip c;
    int group = 0;
    off += make(b, off, c, group);
    by_group[group].push_back(c);
  }
  for (int gi = 0; gi < NG; ++gi) {
    for (size_t i = 0; i < by_group[gi].size(); i += CLIPS_PER_LAUNCH) {
      a.n = (int)std::min<size_t>(CLIPS_PER_LAUNCH, by_group[gi].size() - i);
      for (int j = 0; j < a.n; ++j) a.clip[j] = by_group[gi][i + j];
      const int rc = fire(gi, a);
      if (rc) return rc;
    }
  }
  return 0;
}

// LDS bytes of dynamic LDS for KERNEL, reserved once per device
template <auto KERNEL, int LDS>
int reserve_lds(const char* fn) {
  static_assert(LDS <= 160 * 1024, "LDS");
  static WflOncePerDevice attr_once;
  if (attr_once.need()) {
    if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess)
      return fail(fn, -2, "cannot reserve the kernel's LDS");
  }
  return 0;
}

// one workgroup of NT threads per clip of `a`, LDS bytes of dynamic LDS
template <auto KERNEL, int NT, int LDS, class Launch>
int launch_cfg(const char* fn, const Launch& a, hipStream_t s) {
  if (const int rc = reserve_lds<KERNEL, LDS>(fn)) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(a.n), dim3(NT), LDS, s, a);
  return hipGetLastError() == hipSuccess ? 0 : fail(fn, -3, "launch failed");
}

}  // namespace lattice
