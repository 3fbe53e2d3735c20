// Viterbi forced alignment of a phoneme transcript over the frame logits of a clip (wfl_align, include/wfl_asr.h).
//
// Replaces the greedy string match of the reference's infer.py:30-60 (run at 193, 210-215, 312-319) when the caller asks for
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
//
// The lattice itself -- caps, configurations, the shared LDS layout, setup and status codes, the logits stage ring, emissions, the
// renormalisation halves, and the host side of a ragged batch -- is csrc/lattice.h, shared with csrc/align_posterior.hip.  Here: the
// max-product recursion, the backpointers and the backtrace.
//
// wfl_align_windowed is the same kernel instantiated with WIN: every token's EB passes through lattice.h's win_mask (the token may open
// only inside its window), and a clip whose best end state is -inf -- no path satisfies the windows -- reports status 1 before the
// backtrace.  The unwindowed instantiation holds none of it.
#include "lattice.h"
#include "wfl_asr.h"

namespace {

using namespace lattice;

constexpr int ALIGN_W = 32;                 // backtrace window, frames

struct AlignLaunch {
  const float* logits;
  long ldl;
  int C, o_id;
  const int* tok_cls;  // [total tokens][4][2]
  const int* gap_cls;  // [n_clips][8]
  unsigned* bp;        // LatClip::ws_off: the clip's backpointer words
  int* ids;
  int* tok;
  float* score;
  int* status;
  int n;
  LatClip clip[CLIPS_PER_LAUNCH];
  const int* tok_win;  // [total tokens][2] = (lo, hi), the windowed kernels alone (last: the other fields stay where they were)
};

template <int NT, int R>
struct Cfg : LdsBase<NT, R, 2 * NT * 8> {                // its own between alt and wmax: the neighbour exchange, [2][NT] float2
  static constexpr int WPT = (6 * R + 31) / 32;          // backpointer words per thread per frame
  static constexpr int WIN = ALIGN_W * (ALIGN_W / R + 2) * WPT;
  static constexpr int OFF_WIN = Cfg::OFF_OWN;           // the backtrace window
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int LDS = OFF_MISC + 64;
};

// WIN: the start windows of wfl_align_windowed (lattice.h win_mask); false is wfl_align's kernel, instruction for instruction
template <int NT, int R, bool WIN>
__global__ __launch_bounds__(NT) void align_kernel(AlignLaunch a) {
  using K = Cfg<NT, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  float2* xch = (float2*)(lds + K::OFF_X);
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  unsigned* win = (unsigned*)(lds + K::OFF_WIN);
  int* misc = (int*)(lds + K::OFF_MISC);
  float* fin = (float*)(misc + 4);

  const LatClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = cl.T, N = cl.N, C = a.C;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  int* ids = a.ids + cl.frame_off;
  int* tokp = a.tok + cl.frame_off;
  const float NEG = -INFINITY;

  int g[NGAP];
  const int st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
  if (st != 0 || T == 0) {
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = st; }
    return;
  }

  // ---- forward pass
  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;

  float G[R], B[R], I[R];
#pragma unroll
  for (int r = 0; r < R; ++r) G[r] = B[r] = I[r] = NEG;
  if (tid == 0) G[0] = 0.f;                    // a virtual frame -1 in G_0: frame 0 starts in G_0 or B_0
  xch[NT + tid] = make_float2(NEG, NEG);
  stage.load(0);
  stage.store(0);
  stage.load(1);
  __syncthreads();

  int4 av[R];                                   // this thread's slots' alternatives, for the whole forward pass
#pragma unroll
  for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  int2 wn[WIN ? R : 1];                         // this thread's slots' start windows, in registers
  if constexpr (WIN) load_windows<R>(a.tok_win, cl.tok_off, N, wn);
  unsigned* bp = a.bp + cl.ws_off;
  double acc = 0.0;                            // what the renormalisations subtracted
  float sub = 0.f;
  int c = 0, tin = 0;
  for (int t = 0; t < T; ++t, ++tin) {
    if (tin == F) {
      ++c;
      tin = 0;
      stage.store(c);
      __syncthreads();
      stage.load(c + 1);
    }
    const float* row = stage.row(c, tin);
    const float eg = gap_emission(row, g);
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
      if (k < N) tok_emission(row, av[r], eb, ei);
      if constexpr (WIN) eb = win_mask(eb, t, wn[r]);
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
    const bool renorm = (t & (RENORM - 1)) == RENORM - 1;
    if (renorm) {
      float lm = NEG;
#pragma unroll
      for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(G[r], fmaxf(B[r], I[r])));
      renorm_publish(lm, wmax);
    }
    __syncthreads();                           // the neighbour exchange and the renormalisation share it
    sub = 0.f;
    if (renorm) {
      // (taken as it is; the posterior sweeps replace an M of -inf by 0.  Windows never make it -inf here: G_0 has no window and a
      // finite emission at every frame, so it is finite at every frame and M with it)
      const float M = renorm_max<K::NW>(wmax);
#pragma unroll
      for (int r = 0; r < R; ++r) { G[r] -= M; B[r] -= M; I[r] -= M; }
      sub = M;
      acc += (double)M;
    }
  }

  // ---- the best end state
  publish_end_states<R>(N, G, B, I, fin);
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
    if constexpr (WIN) misc[2] = best == NEG;
  }
  __syncthreads();
  if constexpr (WIN) {
    if (misc[2]) {                              // no path opens every token inside its window: status 1, the backpointers never walked
      for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
      if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 1; }
      return;
    }
  }

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
      float bv = NEG;
      for_each_alt(alt[k], [&](int q, int b, int i) {      // the arg-max alternative's class, the first on a tie
        const int col = j == 2 ? i : b;
        const float x = z[col];
        if (q == 0 || x > bv) { bv = x; id = col; }
      });
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

// backpointer words of a clip.  Over the cap, with fewer frames than tokens or with no frame the kernel stops at its status: no words.
long clip_words(int T, int N) {
  const int c = cfg_of(N);
  if (c == NCFG || T < N || T <= 0) return 0;
  const int per_frame = dispatch_cfg(c, [](auto sh) { return decltype(sh)::NT * Cfg<decltype(sh)::NT, decltype(sh)::R>::WPT; });
  return round64((long)T * per_frame);      // (256-byte aligned)
}

}  // namespace

extern "C" {

int64_t wfl_align_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_words);
}

}  // extern "C"

namespace {

// wfl_align (WIN false) and wfl_align_windowed: one host path
template <bool WIN>
int align_batch(const char* fn, const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, void* workspace, int64_t workspace_bytes, int32_t* ids,
                int32_t* tok, float* score, int32_t* status, void* stream) {
  const int64_t need = wfl_align_workspace_bytes(n_frames_host, n_tok_host, n_clips);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc || n_clips == 0) return rc;
  if (!score || !status || !gap_cls || (any_tok && (!tok_cls || (WIN && !tok_win))) || (any_frame && (!logits || !ids || !tok)))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  AlignLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok_win = tok_win;
  a.bp = (unsigned*)workspace; a.ids = ids; a.tok = tok; a.score = score; a.status = status;
  return launch_clips<NCFG>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_tok_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b};
        cfg = cfg_of(N) < NCFG ? cfg_of(N) : 0;   // over the cap: every kernel reports status 2 before it touches the workspace; the smallest
        return clip_words(T, N);
      },
      [&](int cfg, const AlignLaunch& a) {
        return dispatch_cfg(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          return launch_cfg<align_kernel<NT, R, WIN>, NT, Cfg<NT, R>::LDS>(fn, a, s);
        });
      });
}

}  // namespace

extern "C" {

int32_t wfl_align(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                  const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls, const int32_t* gap_cls, int32_t n_clips,
                  void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  return align_batch<false>("wfl_align", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls, nullptr,
                            gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status, stream);
}

int32_t wfl_align_windowed(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                           const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, void* workspace, int64_t workspace_bytes,
                           int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  return align_batch<true>("wfl_align_windowed", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                           tok_win, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status, stream);
}

}  // extern "C"
