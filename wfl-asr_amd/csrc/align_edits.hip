// Single-edit scores of an aligned transcript (wfl_align_edits, include/wfl_asr.h): per token k the log likelihood ratio of replacing it
// by each of P substitutes, and of deleting it, against the transcript as written -- logZ(edited transcript) - logZ(transcript), the
// sums running over ALL boundaries of the lattice of wfl_align (csrc/lattice.h), with the start windows where given.  The reference has
// no counterpart.
//
// Nothing of the lattice is run again per edit.  With alpha / beta of csrc/align_posterior.hip (same states, same recurrences):
//   A_k(t) = lse(alpha_{t-1}(G_k), alpha_{t-1}(I_{k-1}), alpha_{t-1}(B_{k-1}))   what may enter token k at frame t: the forward step's `in`
//            (t = 0: 0 for k = 0, -inf otherwise; t = T: what ends the clip in front of token k)
//   E_k(t) = beta_t(G_{k+1})                       what follows token k when frame t is its last: G_{k+1} has the successors of I_k
//                                                  other than I_k itself, so this is beta(B_k) without the stay in I_k
//   D_k(t) = EB_t(k) + beta_t(B_k)                 token k opens at t, and everything after
//   substitute p for k:  r_p(t) = lse(A_k(t) + EB_t(p) [k's window], r_p(t-1) + EI_t(p)),   logZ_p(k) = lse_t(r_p(t) + E_k(t))
//   delete k:            k < N - 1: lse_t(A_k(t) + D_{k+1}(t));   k = N - 1: A_k(T)
// (proved against the definition by enumeration of edited transcripts in tests/test_align_edits_cpu.py).
//
// Phase 1, edits_fb_kernel: one workgroup per clip, configurations, slot ownership, staging, neighbour exchange and renormalisation as
// post_kernel, and the very same sweeps: both kernels run alpha and beta of csrc/lattice_sums.h (this one with the windows held at run
// time and without the minimum-duration chain; A_k(t) reaches it through alpha_frame's hook).  Its own are the substitute-table check,
// the planes and the offsets.  One forward and one backward sweep, no checkpoints: the planes A [T + 1][W], E [T][W], D [T][W] (W = round_up_64(N) floats a row) go to the workspace with, per frame, the
// double offsets that alpha's and beta's renormalisations have subtracted so far (an absolute fp32 alpha of a long clip has no
// resolution left).  A null tok_win is every window open.
// Phase 2, edits_chain_kernel: one wave per (token, 64 substitutes), lanes over p: N P independent chains of T steps, two lae2 a step.
// A_k(t), E_k(t), the offsets and the frame's log-sum-exp are wave-uniform loads, the two logits of a lane's pair are gathered from the
// frame's row; frames are taken four at a time so that the loads of a group are in flight together.  r is carried in fp32 relative to
// alpha's offset of its frame; the sum over t is a running (maximum, sum) in double, and so is the difference to logZ.  The wave of a
// token's first 64 substitutes also forms the deletion column, lanes over t.  Frames before max(k, lo_k) and after
// min(T - 1 - (N - 1 - k), hi_{k+1} - 1) contribute exact zeros (A / the window, E) and are skipped; nothing else is.
// Cost: phase 1 two sweeps of the lattice, phase 2 N P T chain steps (measured: tools/align_edits_bench.py).
//
// Single insertions (wfl_align_insertions) are the third edit, from the same two sweeps and the same chain.  Place j = 0 .. N lies in
// front of token j (j = N: behind the last token); a token [p] inserted there has no window, its neighbours keep theirs:
//   F_j(t) = beta_t(G_j)                           what follows a token that ends at t in front of token j (E_{j-1}(t) for j >= 1)
//   insert p at j:  r_p(t) = lse(A_j(t) + EB_t(p), r_p(t-1) + EI_t(p)),   logZ_p(j) = lse_t(r_p(t) + F_j(t))
// (proved against the definition in tests/test_align_insertions_cpu.py).  Phase 1 is edits_fb_kernel<NT, R, true>: planes
// round64(N + 1) wide, A with slot N, F = beta(G_k) for k = 0 .. N in E's place, no D.  Phase 2 is insertions_chain_kernel, one wave
// per (place, 64 substitutes) on the chain of edits_chain_kernel (edit_chain): (N + 1) P chains and no deletion column.  Frames before
// j and after min(T - 1 - (N - j), hi_j - 1) contribute exact zeros and are skipped; nothing else is.
#include "lattice_sums.h"
#include "wfl_asr.h"

namespace {

using namespace lattice;

constexpr int MAX_SUB = 512;               // substitutes per call
constexpr int CHAIN_WAVES = 4;             // waves per workgroup of phase 2
constexpr int CHAIN_U = 4;                 // frames whose loads are in flight together

struct EditLaunch {
  const float* logits;
  long ldl;
  int C;
  const int* tok_cls;  // [total tokens][4][2]
  const int* gap_cls;  // [n_clips][8]
  const int* tok_win;  // [total tokens][2] = (lo, hi); null: every window open
  const int* sub_cls;  // [P][2] = (B class, I class)
  int P;
  float* ws;           // LatClip::ws_off: the clip's workspace, in floats
  float* logz;
  float* edits;        // [total tokens][P + 1]; the insertions: [total tokens + n_clips][P], clip b's rows from tok_off + b
  int* status;
  int n;
  LatClip clip[CLIPS_PER_LAUNCH];
};

// a clip's workspace in floats: [logZ (double) : 64] [lse: round64(T)] [offA (double): T + 1] [offB (double): T] [A: (T + 1) W] [E: T W]
// [D: T W], every part rounded up to 64.  ins (the insertions): W = round64(N + 1), E holds F (slot k in column k), and there is no D
struct EditLayout {
  long W, lse, offa, offb, A, E, D, total;
  __host__ __device__ EditLayout(int T, int N, bool ins = false) {
    W = round64(N + (ins ? 1 : 0));
    lse = 64;
    offa = lse + round64(T);
    offb = offa + round64(2L * (T + 1));
    A = offb + round64(2L * T);
    E = A + round64((long)(T + 1) * W);
    D = E + round64((long)T * W);
    total = ins ? D : D + round64((long)T * W);
  }
};

template <int NT, int R>
struct ECfg : LdsBase<NT, R, 2 * 2 * NT * 8> {                     // its own between alt and wmax: the two neighbour exchanges
  static constexpr int OFF_XF = ECfg::OFF_X;                       // forward neighbour exchange: [2][NT] float2
  static constexpr int OFF_XB = OFF_XF + 2 * NT * 8;               // backward neighbour exchange
  static constexpr int OFF_LRING = ECfg::OFF_OWN;                  // staged rows' log-sum-exp
  static constexpr int OFF_MISC = OFF_LRING + 2 * FMAX * 4;
  static constexpr int LDS = OFF_MISC + 64;
};

// ---- phase 1: the sweeps of the transcript's own lattice -> A, E, D, the offsets, logZ; INS: A with slot N, F in E's place, no D
template <int NT, int R, bool INS = false>
__global__ __launch_bounds__(NT) void edits_fb_kernel(EditLaunch a) {
  using K = ECfg<NT, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  float2* xf = (float2*)(lds + K::OFF_XF);
  float2* xb = (float2*)(lds + K::OFF_XB);
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  float* lring = (float*)(lds + K::OFF_LRING);
  int* misc = (int*)(lds + K::OFF_MISC);
  float* fin = (float*)(misc + 4);

  const LatClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = cl.T, N = cl.N, C = a.C, P = a.P;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  const float NEG = -INFINITY;

  // the substitute table first: a class id out of range is status 4 for every clip
  if (tid == 0) misc[1] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += NT) {
    const int b = a.sub_cls[2 * p], i = a.sub_cls[2 * p + 1];
    if (b < 0 || b >= C || i < 0 || i >= C) misc[1] = 1;
  }
  __syncthreads();
  int g[NGAP];
  int st = misc[1] ? 4 : lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
  int2 wn[R];                                  // this thread's slots' start windows, and the next thread's first slot's
  int2 wnn = make_int2(0, WIN_OPEN_HI);
#pragma unroll
  for (int r = 0; r < R; ++r) wn[r] = make_int2(0, WIN_OPEN_HI);
  if (a.tok_win && st == 0) {
    load_windows<R>(a.tok_win, cl.tok_off, N, wn);
    wnn = load_window(a.tok_win, cl.tok_off, (tid + 1) * R, N);
  }
  auto refuse = [&](int code, float fill = 0.f) {   // zeros and the status, as every entry of the lattice
    const long n = INS ? (long)(N + 1) * P : (long)N * (P + 1);
    float* e = INS ? a.edits + (long)(cl.tok_off + cl.clip) * P : a.edits + (long)cl.tok_off * (P + 1);
    for (long q = tid; q < n; q += NT) e[q] = fill;
    if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = code; }
  };
  if (st != 0 || T == 0) {
    refuse(st, INS && st == 0 ? NEG : 0.f);    // (no frame and no token: a legal clip, and no frame for an inserted token)
    return;
  }

  const EditLayout lay(T, N, INS);
  const long W = lay.W;
  float* ws = a.ws + cl.ws_off;
  float* lse = ws + lay.lse;
  double* offa = (double*)(ws + lay.offa);
  double* offb = (double*)(ws + lay.offb);
  float* pA = ws + lay.A;
  float* pE = ws + lay.E;
  [[maybe_unused]] float* pD = ws + lay.D;

  // ---- the per-frame log-sum-exp, in fp32 for the sweeps; what its rounding loses, in double for logZ
  const double lres = frame_lse<NT>(tid, Z, a.ldl, T, C, lse, red);

  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;
  float pre_l = 0.f;
  int pre_t = -1;                              // (no token ring here)
  auto load_stage = [&](int c) { stage_load<false>(tid, stage, c, lse, nullptr, pre_l, pre_t); };
  auto store_stage = [&](int c) { stage_store<false>(tid, stage, c, lring, nullptr, pre_l, pre_t); };

  int4 av[R];                                   // this thread's slots' alternatives
#pragma unroll
  for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  const int4 avn = tid + 1 < NT ? alt[(tid + 1) * R] : make_int4(-1, -1, -1, -1);   // the next thread's first slot

  // ---- the forward sweep: A_k(t) is the step's `in`, relative to what alpha's renormalisations subtracted before frame t
  // (lattice_sums.h with WIN, the windows being held at run time and open where there are none, and without MIND)
  NoChain no;
  float G[R], B[R], I[R];
#pragma unroll
  for (int r = 0; r < R; ++r) G[r] = B[r] = I[r] = NEG;
  if (tid == 0) G[0] = 0.f;                    // a virtual frame -1 in G_0: frame 0 starts in G_0 or B_0
  double acc = 0.0;
  float sub = 0.f;
  {
    alpha_to_right<NT, R, false>(tid, xf, 1, B, I, no.D);
    int c = 0, tin = 0;
    stage_start(0, 1, load_stage, store_stage);
    for (int t = 0; t < T; ++t, ++tin) {
      if (tin == F) {
        ++c;
        tin = 0;
        stage_enter(c, 1, load_stage, store_stage);
      }
      if (tid == 0) offa[t] = acc;
      alpha_frame<NT, R, true, false>(tid, stage.row(c, tin), lring[(c & 1) * FMAX + tin], g, av, N, t, xf, wmax, sub, acc, G, B, I, no.H, no.D, wn, [&](int, int k, float in) {
        if (k < N || (INS && k == N)) pA[(long)t * W + k] = in;
      });
    }
    // row T of A: what ends the clip in front of token k (the deletion of the last token reads A_{N-1}(T)); no insertion reads it
    if constexpr (!INS) {
      const float2 nb = alpha_from_left<NT>(tid, xf, T, sub);
      if (tid == 0) offa[T] = acc;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (tid * R + r < N) pA[(long)T * W + tid * R + r] = alpha_enter<R, false>(r, G, B, I, nb, no.D);
    }
  }
  publish_end_states<R>(N, G, B, I, fin);
  __syncthreads();
  if (tid == 0) red[0] = end_logz<true>(fin, N, acc);   // -inf: no path opens every token inside its window
  __syncthreads();
  const double logZ = red[0];                  // on the fp32 log-sum-exps; the clip's logZ is logZ - lres
  if (logZ == -INFINITY) {                     // status 1 and zeros, as every clip with a status
    refuse(1);
    return;
  }

  // ---- the backward sweep: E_k(t) = beta_t(G_{k+1}), D_k(t) = EB_t(k) + beta_t(B_k), relative to what beta's renormalisations
  // subtracted before frame t (counting down)
  float bG[R], bX[R];                          // beta(G_k), beta(B_k) = beta(I_k)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    bG[r] = k == N ? 0.f : NEG;
    bX[r] = k == N - 1 ? 0.f : NEG;
  }
  beta_to_left<NT, R, false>(tid, xb, T, bG, bX, no.C, no.D);
  double accb = 0.0;
  float subb = 0.f;
  {
    int c = (T - 1) / F, tin = (T - 1) - c * F;
    stage_start(c, -1, load_stage, store_stage);
    for (int t = T - 1; t >= 0; --t, --tin) {
      if (tin < 0) {
        --c;
        tin = F - 1;
        stage_enter(c, -1, load_stage, store_stage);
      }
      float eg, eb[R], ei[R], ebn;
      beta_emissions<NT, R, true>(tid, stage.row(c, tin), lring[(c & 1) * FMAX + tin], g, av, avn, N, t, wn, wnn, eg, eb, ei, ebn);
      if (tid == 0) offb[t] = accb;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = tid * R + r;
        if constexpr (INS) {
          if (k <= N) pE[(long)t * W + k] = bG[r];
        } else {
          if (k < N) pD[(long)t * W + k] = bX[r] + eb[r];
          if (k >= 1 && k <= N) pE[(long)t * W + k - 1] = bG[r];
        }
      }
      if (t == 0) break;
      beta_frame<NT, R, false>(tid, N, t, eg, eb, ei, ebn, xb, wmax, subb, accb, bG, bX, no.B, no.C, no.D);
    }
  }
  if (tid == 0) {
    *(double*)ws = logZ;
    a.logz[cl.clip] = (float)(logZ - lres);
    a.status[cl.clip] = 0;
  }
}

// ---- phase 2: the edit recursions
// a running log-sum-exp in double: (maximum, sum of exp(v - maximum))
struct RunLse {
  double m = -INFINITY, s = 0.0;
  __device__ __forceinline__ void add(double v) {
    if (v > m) {                               // (v = -inf never gets here, nor a NaN)
      s = s * (double)__expf((float)(m - v)) + 1.0;
      m = v;
    } else if (v > -INFINITY) {
      s += (double)__expf((float)(v - m));
    }
  }
  __device__ __forceinline__ double value() const { return s > 0.0 ? m + log(s) : -INFINITY; }
};

// one lane's chain of substitute p over the frames t0 .. t1: r(t) = lse(A(t) + EB_t(p) [the window wk], r(t-1) + EI_t(p)) ->
// lse_t(r(t) + E(t)), absolute.  pA / pE: the column of the token (edits) or of the place (insertions, wk open), W floats a row.
__device__ __forceinline__ double edit_chain(const EditLaunch& a, const float* Z, const float* lse, const double* offa, const double* offb,
                                             const float* pA, const float* pE, long W, int t0, int t1, int2 wk, int p) {
  const float NEG = -INFINITY;
  const int cb = a.sub_cls[2 * p], ci = a.sub_cls[2 * p + 1];
  float r = NEG;
  double oprev = 0.0;
  RunLse acc;
  for (int tb = t0; tb <= t1; tb += CHAIN_U) {
    float Ak[CHAIN_U], Ek[CHAIN_U], lk[CHAIN_U], zb[CHAIN_U], zi[CHAIN_U];
    double oa[CHAIN_U], ob[CHAIN_U];
#pragma unroll
    for (int u = 0; u < CHAIN_U; ++u) {        // (a group's tail reads frame t1 again, and does not use it)
      const int t = min(tb + u, t1);
      Ak[u] = pA[(long)t * W];
      Ek[u] = pE[(long)t * W];
      lk[u] = lse[t];
      oa[u] = offa[t];
      ob[u] = offb[t];
      zb[u] = Z[(long)t * a.ldl + cb];
      zi[u] = Z[(long)t * a.ldl + ci];
    }
#pragma unroll
    for (int u = 0; u < CHAIN_U; ++u) {
      const int t = tb + u;
      if (t > t1) break;
      const float d = (float)(oa[u] - oprev);              // r of frame t - 1 was relative to that frame's offset
      oprev = oa[u];
      const float enter = win_mask(Ak[u] + (zb[u] - lk[u]), t, wk);
      r = lae2(enter, (r - d) + (zi[u] - lk[u]));
      acc.add((double)(r + Ek[u]) + (oa[u] + ob[u]));
    }
  }
  return acc.value();
}

__global__ __launch_bounds__(CHAIN_WAVES * 64) void edits_chain_kernel(EditLaunch a) {
  const LatClip cl = a.clip[blockIdx.y];
  const int T = cl.T, N = cl.N, P = a.P;
  const int chunks = max(1, (P + 63) / 64);
  const int lane = threadIdx.x & 63;
  // (wave-uniform by construction; saying so lets the per-frame values of the token travel as scalars)
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * CHAIN_WAVES + (threadIdx.x >> 6)));
  if (w >= N * chunks || a.status[cl.clip] != 0 || T == 0) return;
  const int k = w / chunks, chunk = w - k * chunks;
  const EditLayout lay(T, N);
  const long W = lay.W;
  const float* ws = a.ws + cl.ws_off;
  const double logZ = *(const double*)ws;
  const float* lse = ws + lay.lse;
  const double* offa = (const double*)(ws + lay.offa);
  const double* offb = (const double*)(ws + lay.offb);
  const float* pA = ws + lay.A + k;
  const float* pE = ws + lay.E + k;
  const float* pD = ws + lay.D + k + 1;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  float* out = a.edits + (long)(cl.tok_off + k) * (P + 1);
  const float NEG = -INFINITY;

  int2 wk = make_int2(0, WIN_OPEN_HI), wk1 = wk;
  if (a.tok_win) {
    wk = load_window(a.tok_win, cl.tok_off, k, N);
    wk1 = load_window(a.tok_win, cl.tok_off, k + 1, N);
  }
  // before t0 nothing can have entered token k (k tokens in front of it, its window); after t1 nothing can follow it (N - 1 - k
  // tokens behind it, the next token's window): exact zeros
  const int t0 = max(k, wk.x);
  const int t1 = min(T - 1 - (N - 1 - k), k + 1 < N ? max(min(wk1.y, T), 0) - 1 : T - 1);

  const int p = chunk * 64 + lane;
  if (p < P) out[p] = (float)(edit_chain(a, Z, lse, offa, offb, pA, pE, W, t0, t1, wk, p) - logZ);

  if (chunk == 0) {                            // the deletion column, lanes over t
    double v;
    if (k == N - 1) {
      v = (double)pA[(long)T * W] + offa[T];
    } else {
      RunLse acc;
      for (int t = k + lane; t < T; t += 64) acc.add((double)(pA[(long)t * W] + pD[(long)t * W]) + (offa[t] + offb[t]));
      double M = acc.m;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) M = fmax(M, __shfl_xor(M, o));
      const double s = wave_sum(acc.s > 0.0 ? acc.s * exp(acc.m - M) : 0.0);
      v = s > 0.0 ? M + log(s) : -INFINITY;
    }
    if (lane == 0) out[P] = (float)(v - logZ);
  }
}

// the insertions' phase 2: one wave per (place j, 64 substitutes); A's column j with F's column j, no window on the entry
__global__ __launch_bounds__(CHAIN_WAVES * 64) void insertions_chain_kernel(EditLaunch a) {
  const LatClip cl = a.clip[blockIdx.y];
  const int T = cl.T, N = cl.N, P = a.P;
  const int chunks = (P + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * CHAIN_WAVES + (threadIdx.x >> 6)));
  if (w >= (N + 1) * chunks || a.status[cl.clip] != 0 || T == 0) return;
  const int j = w / chunks, chunk = w - j * chunks;
  const EditLayout lay(T, N, true);
  const float* ws = a.ws + cl.ws_off;
  const double logZ = *(const double*)ws;
  // a token needs a frame at or after j (j tokens in front of it); nothing follows it after T - 1 - (N - j) (N - j tokens behind it)
  // or from token j's last start on: exact zeros
  int hi = T;
  if (a.tok_win && j < N) hi = max(min(load_window(a.tok_win, cl.tok_off, j, N).y, T), 0);
  const int t1 = min(T - 1 - (N - j), hi - 1);
  const int p = chunk * 64 + lane;
  if (p < P)
    a.edits[(long)(cl.tok_off + cl.clip + j) * P + p] =
        (float)(edit_chain(a, a.logits + cl.frame_off * a.ldl, ws + lay.lse, (const double*)(ws + lay.offa), (const double*)(ws + lay.offb),
                           ws + lay.A + j, ws + lay.E + j, lay.W, j, t1, make_int2(0, WIN_OPEN_HI), p) - logZ);
}

// over the cap the kernel reports status 2; such a clip is sized (and launched) as the cap's configuration, as the posterior's
int edit_cfg(int N) { return std::min(cfg_of(N), NCFG - 1); }

long clip_floats(int T, int N) {
  if (T <= 0) return 0;
  return EditLayout(T, std::min(N, MAX_TOKENS)).total;     // (a multiple of 64: 256-byte aligned)
}

long clip_floats_ins(int T, int N) {
  if (T <= 0) return 0;
  return EditLayout(T, std::min(N, MAX_TOKENS), true).total;
}

// the two entries: INS false wfl_align_edits, true wfl_align_insertions (`edits`: its ins)
template <bool INS>
int run_edits(const char* fn, const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
              const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
              const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* sub_cls, int32_t n_sub, void* workspace,
              int64_t workspace_bytes, float* logz, float* edits, int32_t* status, void* stream) {
  const int64_t need = clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, INS ? clip_floats_ins : clip_floats);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc) return rc;
  if (n_sub < 0 || n_sub > MAX_SUB) return fail(fn, -1, "n_sub must be 0 .. 512");
  if (n_clips == 0) return 0;
  // (the insertions have a row for every clip, tokens or none, and no column without a substitute)
  const bool no_out = INS ? (n_sub > 0 && !edits) : (any_tok && !edits);
  if (!logz || !status || !gap_cls || (n_sub > 0 && !sub_cls) || (any_tok && !tok_cls) || no_out || (any_frame && !logits))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  EditLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok_win = tok_win; a.sub_cls = sub_cls;
  a.P = n_sub; a.ws = (float*)workspace; a.logz = logz; a.edits = edits; a.status = status;
  return launch_clips<NCFG>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_tok_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b};
        cfg = edit_cfg(N);
        return INS ? clip_floats_ins(T, N) : clip_floats(T, N);
      },
      [&](int cfg, const EditLaunch& a) {
        const int rc = dispatch_cfg(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          return launch_cfg<edits_fb_kernel<NT, R, INS>, NT, ECfg<NT, R>::LDS>(fn, a, s);
        });
        if (rc) return rc;
        int waves = 0;                         // of the launch's largest transcript; a clip with fewer leaves its surplus at once
        for (int j = 0; j < a.n; ++j)
          if (a.clip[j].N <= MAX_TOKENS)
            waves = std::max(waves, INS ? (a.clip[j].N + 1) * ((a.P + 63) / 64) : a.clip[j].N * std::max(1, (a.P + 63) / 64));
        if (waves == 0) return 0;
        hipLaunchKernelGGL(INS ? insertions_chain_kernel : edits_chain_kernel, dim3((waves + CHAIN_WAVES - 1) / CHAIN_WAVES, a.n),
                           dim3(CHAIN_WAVES * 64), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : fail(fn, -3, "launch failed");
      });
}

}  // namespace

extern "C" {

int64_t wfl_align_edits_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_floats);
}

int32_t wfl_align_edits(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                        const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                        const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* sub_cls, int32_t n_sub,
                        void* workspace, int64_t workspace_bytes, float* logz, float* edits, int32_t* status, void* stream) {
  return run_edits<false>("wfl_align_edits", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls, tok_win,
                          gap_cls, n_clips, sub_cls, n_sub, workspace, workspace_bytes, logz, edits, status, stream);
}

int64_t wfl_align_insertions_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_floats_ins);
}

int32_t wfl_align_insertions(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                             const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                             const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* sub_cls, int32_t n_sub,
                             void* workspace, int64_t workspace_bytes, float* logz, float* ins, int32_t* status, void* stream) {
  return run_edits<true>("wfl_align_insertions", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                         tok_win, gap_cls, n_clips, sub_cls, n_sub, workspace, workspace_bytes, logz, ins, status, stream);
}

}  // extern "C"
