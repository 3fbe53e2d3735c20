// The sum-product sweeps over the forced-alignment lattice of csrc/lattice.h, written ONCE for the kernels that run them: post_kernel
// (csrc/align_posterior.h: the per-token posteriors, with start windows and with the minimum-duration chain) and edits_fb_kernel
// (csrc/align_edits.hip: the planes of the single-edit scores).  A lattice variant that is written into alpha and beta here is
// written for both.  csrc/align.hip, the max-product search, does not include this header: its step stays its own.
//
// Pieces, in the order a kernel uses them (recurrences: the head of align_posterior.h):
//   lae2 / lae3                        log-sum-exp of two / three log-domain values
//   frame_lse                          the per-frame log-sum-exp of the logits, fp32 for the sweeps, its rounding residue in double
//   stage_load / stage_store           the staged logits ring of lattice.h with its side rings: the rows' log-sum-exp, and their Viterbi token
//   stage_start / stage_enter          a sweep's walk over the stages, one stage ahead, in either direction
//   alpha_to_right / alpha_from_left   the forward neighbour exchange;  alpha_enter: what may enter token k (edits' A_k(t))
//   alpha_frame                        one frame of alpha over a thread's R slots, with the frame's barrier and the renormalisation
//   end_logz                           logZ from the published end states
//   beta_to_left, beta_emissions, beta_frame                  the same for beta
// WIN: EB passes through win_mask (windows in registers; a kernel that holds its windows at run time instantiates WIN and loads open
// windows where it has none).  MIND: the minimum-duration chain, H beside G, B, I for alpha and the delay line bC for beta; without it
// the chain arguments are arrays of one element that nothing reads (NoChain).  Every piece takes the kernel's own `tid`: a thread index
// read again inside the pieces costs post_kernel a register.
// OPT: the skip arcs of wfl_align_optional (include/wfl_asr.h), never with MIND: B_k is also entered from what may enter token k - 1,
// at -lam, where token k - 1 is optional.  Everything of it stands under `if constexpr (OPT)`; the wider neighbour exchanges are the
// *_opt siblings of the exchange pieces, and the flags travel as a bit mask per thread (SkipArcs).
// FILL: the filler emission of wfl_align_filler (include/wfl_asr.h), never with MIND or OPT: a flagged token emits EB = EI = ef, the
// frame's (largest logit - log-sum-exp) - phi, which frame_lse keeps per frame beside lse[]; the flags travel as a bit mask per thread
// (bit r: this thread's slot r, bit R: the next thread's first slot), and beta_frame hands out what leaves every token (leave).
// Everything of it stands under `if constexpr (FILL)`.
#pragma once
#include "lattice.h"

namespace lattice {

// log(exp a + exp b [+ exp c]); -inf in, -inf out (v_exp_f32 / v_log_f32)
static __device__ __forceinline__ float lae2(float a, float b) {
  const float m = fmaxf(a, b);
  const float ms = m == -INFINITY ? 0.f : m;
  return ms + __logf(__expf(a - ms) + __expf(b - ms));
}

static __device__ __forceinline__ float lae3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float ms = m == -INFINITY ? 0.f : m;
  return ms + __logf(__expf(a - ms) + __expf(b - ms) + __expf(c - ms));
}

// ---- the per-frame log-sum-exp of the logits (double, expf) -> lse[T] in fp32, for the sweeps; returns what the fp32 rounding loses,
// summed over the clip in double (the same in every thread): it is common to every path and goes back into logZ.  red: a double per wave.
// (a thread per row; a wave per row with coalesced loads and wave reductions was measured 4 % slower for the whole posterior kernel)
// FILL: fem[t] = (the row's maximum - lse[t]) - phi as well, what a filler emits at frame t; fem null: a clip without a filler, nothing more
template <int NT, bool FILL = false>
static __device__ __forceinline__ double frame_lse(const int tid, const float* Z, long ldl, int T, int C, float* lse, double* red,
                                                   float* fem = nullptr, float phi = 0.f) {
  double lres = 0.0;
  for (int t = tid; t < T; t += NT) {
    const float* z = Z + (long)t * ldl;
    float m = z[0];
    for (int q = 1; q < C; ++q) m = fmaxf(m, z[q]);
    double se = 0.0;
    for (int q = 0; q < C; ++q) se += (double)expf(z[q] - m);
    const double ld = (double)m + log(se);
    const float lf = (float)ld;
    lse[t] = lf;
    if constexpr (FILL) {
      if (fem) fem[t] = (m - lf) - phi;
    }
    lres += ld - (double)lf;
  }
  lres = wave_sum(lres);
  if ((tid & 63) == 0) red[tid >> 6] = lres;
  __syncthreads();                             // (and the block sees lse[])
  lres = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) lres += red[w];
  return lres;
}

// ---- staging of the logits rows (rows: lattice.h LogitStages) with their log-sum-exp and, TOK, their Viterbi token, through two side
// rings of 2 FMAX words: stage c into registers (pre_l, pre_t beside rows' own), and from there into the rings.  The kernel keeps
// pre_l / pre_t as plain locals beside its LogitStages, as both kernels always did, and wraps the pair in two lambdas of (c).
// A sweep runs one stage ahead of its frames in either direction: stage_start before its first frame, stage_enter when it crosses into
// stage c; step = +1 forward, -1 backward (down to a stage -1 in front of the clip, which loads nothing).
template <bool TOK, class Rows>
static __device__ __forceinline__ void stage_load(const int tid, Rows& rows, int c, const float* lse, const int* tokp, float& pre_l, int& pre_t) {
  const int F = rows.F;
  rows.load(c, c >= 0);
  const bool in = tid < F && c >= 0 && c * F + tid < rows.T;
  pre_l = in ? lse[c * F + tid] : 0.f;
  if constexpr (TOK) pre_t = in ? tokp[c * F + tid] : -1;
}

template <bool TOK, class Rows>
static __device__ __forceinline__ void stage_store(const int tid, Rows& rows, int c, float* lring, int* tring, float pre_l, int pre_t) {
  rows.store(c);
  if (tid < rows.F) {
    lring[(c & 1) * FMAX + tid] = pre_l;
    if constexpr (TOK) tring[(c & 1) * FMAX + tid] = pre_t;
  }
}

template <class Load, class Store>
static __device__ __forceinline__ void stage_start(int c, int step, Load load, Store store) {
  __syncthreads();                             // the ring's last readers are done
  load(c);
  store(c);
  load(c + step);
  __syncthreads();
}

template <class Load, class Store>
static __device__ __forceinline__ void stage_enter(int c, int step, Load load, Store store) {
  store(c);
  __syncthreads();
  load(c + step);
}

// ---- alpha.  Thread i hands (alpha(B), alpha(I)) of its last slot to thread i + 1 through xf[2][NT], by the parity of the frame.
// (with durations the left token is left from its I alone where its D > 1: B is masked by its owner, as in csrc/align.hip)
template <int NT, int R, bool MIND>
static __device__ __forceinline__ void alpha_to_right(const int tid, float2* xf, int t, const float (&B)[R], const float (&I)[R], const int (&dm)[MIND ? R : 1]) {
  float b = B[R - 1];
  if constexpr (MIND) b = dm[R - 1] > 1 ? -INFINITY : b;
  xf[(t & 1) * NT + tid] = make_float2(b, I[R - 1]);
}

// what thread i - 1 published for frame t - 1, less what that frame's renormalisation subtracted after it was published
template <int NT>
static __device__ __forceinline__ float2 alpha_from_left(const int tid, const float2* xf, int t, float sub) {
  float2 nb = tid > 0 ? xf[((t + 1) & 1) * NT + tid - 1] : make_float2(-INFINITY, -INFINITY);
  nb.x -= sub;
  nb.y -= sub;
  return nb;
}

// lse(alpha_{t-1}(G_k), alpha_{t-1}(I_{k-1}), alpha_{t-1}(B_{k-1})) of slot r: what may enter token k at frame t
template <int R, bool MIND>
static __device__ __forceinline__ float alpha_enter(int r, const float (&G)[R], const float (&B)[R], const float (&I)[R], float2 nb,
                                                    const int (&dm)[MIND ? R : 1]) {
  float pB1 = r ? B[r > 0 ? r - 1 : 0] : nb.x;
  if constexpr (MIND) {
    if (r && dm[r > 0 ? r - 1 : 0] > 1) pB1 = -INFINITY;
  }
  const float pI1 = r ? I[r > 0 ? r - 1 : 0] : nb.y;
  return lae3(G[r], pI1, pB1);
}

// ---- OPT.  The flags of the tokens a thread's recurrences look at, and the penalty: bit j of `om` = "token tid R + j - 1 is optional",
// j = 0 .. R + 1 (a slot outside 0 .. N - 1: 0).  Alpha asks for token k - 1 (bit r), beta for tokens k and k + 1 (bits r + 1, r + 2).
// Without OPT a kernel hands over SkipArcs() and nothing reads it.
struct SkipArcs {
  unsigned om = 0;
  float lam = 0.f;
  __device__ __forceinline__ bool opt(int j) const { return (om >> j) & 1u; }
};

template <int R>
static __device__ __forceinline__ SkipArcs load_skip_arcs(const int tid, const int* tok_opt, int tok_off, int N, float lam) {
  SkipArcs sk;
  sk.lam = lam;
#pragma unroll
  for (int j = 0; j < R + 2; ++j) {
    const int k = tid * R + j - 1;
    if (k >= 0 && k < N && tok_opt[tok_off + k] != 0) sk.om |= 1u << j;
  }
  return sk;
}

// the forward exchange with skip arcs: what csrc/align.hip's OPT search exchanges, [2][XF_OPT][NT] floats -- B, I, G of the thread's last
// slot, B, I of the one before it (every configuration has R >= 2).  All five carry the same `sub`.
constexpr int XF_OPT = 5;
struct LeftOpt {
  float2 nb;           // (alpha(B), alpha(I)) of slot R - 1, as alpha_from_left's
  float G1, B2, I2;    // alpha(G) of slot R - 1, alpha(B), alpha(I) of slot R - 2
};

template <int NT, int R>
static __device__ __forceinline__ void alpha_to_right_opt(const int tid, float* xf, int t, const float (&G)[R], const float (&B)[R], const float (&I)[R]) {
  static_assert(R >= 2, "the widened exchange takes a thread's last TWO slots");
  float* xq = xf + (t & 1) * XF_OPT * NT + tid;
  xq[0] = B[R - 1];
  xq[NT] = I[R - 1];
  xq[2 * NT] = G[R - 1];
  xq[3 * NT] = B[R - 2];
  xq[4 * NT] = I[R - 2];
}

template <int NT>
static __device__ __forceinline__ LeftOpt alpha_from_left_opt(const int tid, const float* xf, int t, float sub) {
  LeftOpt l;
  l.nb = make_float2(-INFINITY, -INFINITY);
  l.G1 = l.B2 = l.I2 = -INFINITY;
  if (tid > 0) {
    const float* xp = xf + ((t + 1) & 1) * XF_OPT * NT + tid - 1;
    l.nb = make_float2(xp[0], xp[NT]);
    l.G1 = xp[2 * NT];
    l.B2 = xp[3 * NT];
    l.I2 = xp[4 * NT];
  }
  l.nb.x -= sub;
  l.nb.y -= sub;
  l.G1 -= sub;
  l.B2 -= sub;
  l.I2 -= sub;
  return l;
}

// the chain arguments of a kernel that runs the sweeps without MIND: one element each, which nothing reads
struct NoChain {
  float H[1][CHAIN], C[1][CHAIN_BACK], B[1];
  int D[1];
};

struct NoHook {
  __device__ __forceinline__ void operator()(int, int, float) const {}
};

// one frame t of alpha over this thread's slots, from the staged row and its log-sum-exp l: the neighbour's values in, the recurrences,
// this thread's last slot out, the frame's ONE barrier (the neighbour exchange and the renormalisation share it) and, every RENORM
// frames, the renormalisation: the block's maximum of G, B, I (with the chain as without) leaves every state and goes to acc; sub is
// what the neighbour's values of this frame, published before the barrier, still carry.  Every state -inf (or a NaN): nothing is
// subtracted (wfl_align's search takes M as it is).  hook(r, k, in) sees alpha_enter of every slot.
// (Frame and tail are ONE function on purpose: as two, with sub going into one by value and out of the other by reference, post_kernel
// needs a register more and wfl_align_posterior_windowed was measured 0.4 to 0.8 % slower; profiles/sumproduct_sweeps_ab.txt.)
// OPT: xf is the [2][XF_OPT][NT] exchange, and B_k is also entered from in_{k-1} - lam where token k - 1 is optional: the slot
// below's alpha_enter, taken before that slot is written (of slot 0: from the left thread's G[R-1], I[R-2], B[R-2]).
// FILL: a slot whose bit of fm is set emits ef for B and I (B still through its window).
template <int NT, int R, bool WIN, bool MIND, class Hook = NoHook, bool OPT = false, bool FILL = false>
static __device__ __forceinline__ void alpha_frame(const int tid, const float* row, float l, const int (&g)[NGAP], const int4 (&av)[R], int N, int t, float2* xf,
                                                   float* wmax, float& sub, double& acc, float (&G)[R], float (&B)[R], float (&I)[R], float (&H)[MIND ? R : 1][CHAIN],
                                                   const int (&dm)[MIND ? R : 1], const int2 (&wn)[WIN ? R : 1], Hook hook = Hook(),
                                                   const SkipArcs sk = SkipArcs(), const unsigned fm = 0, const float ef = 0.f) {
  static_assert(!(OPT && MIND), "no skip arcs in the minimum-duration lattice");
  static_assert(!(FILL && (MIND || OPT)), "no filler emission in the minimum-duration and skip lattices");
  const float eg = gap_emission(row, g) - l;
  float2 nb;
  float inl = -INFINITY, inr = -INFINITY;      // OPT: alpha_enter of the slot below (of the left thread's last slot), of this slot
  if constexpr (OPT) {
    const LeftOpt lf = alpha_from_left_opt<NT>(tid, (const float*)xf, t, sub);
    nb = lf.nb;
    inl = lae3(lf.G1, lf.I2, lf.B2);
    inr = alpha_enter<R, MIND>(R - 1, G, B, I, nb, dm);
  } else {
    nb = alpha_from_left<NT>(tid, xf, t, sub);
  }
#pragma unroll
  for (int r = R - 1; r >= 0; --r) {           // descending: slot r - 1's previous-frame values are still in place
    const int k = tid * R + r;
    float in;
    float inb;                                 // what B_k is entered from
    if constexpr (OPT) {
      in = inr;
      inr = r ? alpha_enter<R, MIND>(r > 0 ? r - 1 : 0, G, B, I, nb, dm) : inl;
      inb = sk.opt(r) ? lae2(in, inr - sk.lam) : in;
    } else {
      in = alpha_enter<R, MIND>(r, G, B, I, nb, dm);
      inb = in;
    }
    float x = B[r];                            // what I_k is entered from
    if constexpr (MIND) x = chain_out(B[r], H[r], dm[r]);
    const float ii = lae2(I[r], x);
    hook(r, k, in);
    float eb = -INFINITY, ei = -INFINITY;
    if (k < N) {
      tok_emission(row, av[r], eb, ei);
      eb -= l;
      ei -= l;
      if constexpr (FILL) {
        if ((fm >> r) & 1u) eb = ei = ef;
      }
      if constexpr (WIN) eb = win_mask(eb, t, wn[r]);
    }
    G[r] = k <= N ? in + eg : -INFINITY;
    if constexpr (MIND) chain_shift(H[r], B[r], ei, dm[r]);
    B[r] = inb + eb;
    I[r] = ii + ei;
  }
  if constexpr (OPT) alpha_to_right_opt<NT, R>(tid, (float*)xf, t, G, B, I);
  else alpha_to_right<NT, R, MIND>(tid, xf, t, B, I, dm);
  const bool renorm = (t & (RENORM - 1)) == RENORM - 1;
  if (renorm) {
    float lm = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(G[r], fmaxf(B[r], I[r])));
    renorm_publish(lm, wmax);
  }
  __syncthreads();
  sub = 0.f;
  if (renorm) {
    float M = renorm_max<NT / 64>(wmax);
    if (!(M > -INFINITY)) M = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) { G[r] -= M; B[r] -= M; I[r] -= M; }
    if constexpr (MIND) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < CHAIN; ++j) H[r][j] -= M;
    }
    sub = M;
    acc += (double)M;
  }
}

// logZ on the fp32 log-sum-exps, by thread 0 after publish_end_states and a barrier: lse(fin[]) + what alpha's renormalisations took.
// INF_RULE: no path at all (windows, durations) is -inf and not the NaN of the formula
template <bool INF_RULE>
static __device__ __forceinline__ double end_logz(const float* fin, int N, double acc) {
  const int ne = N >= 1 ? 3 : 1;
  double m = -INFINITY;
  for (int i = 0; i < ne; ++i) m = fmax(m, (double)fin[i]);
  double s = 0.0;
  for (int i = 0; i < ne; ++i) s += exp((double)fin[i] - m);
  if (INF_RULE && m == -INFINITY) return -INFINITY;
  return m + log(s) + acc;
}

// the same over the skip lattice: where token N - 1 is optional (last), the ends that skip it as well, each at -lam --
// fin[3] = G_{N-1}, fin[4] = I_{N-2}, fin[5] = B_{N-2} (the last two only for N >= 2).  No path at all is -inf.
static __device__ __forceinline__ double end_logz_opt(const float* fin, int N, double acc, bool last, float lam) {
  double v[6];
  int ne = 0;
  v[ne++] = (double)fin[0];
  if (N >= 1) { v[ne++] = (double)fin[1]; v[ne++] = (double)fin[2]; }
  if (N >= 1 && last) {
    v[ne++] = (double)fin[3] - (double)lam;
    if (N >= 2) { v[ne++] = (double)fin[4] - (double)lam; v[ne++] = (double)fin[5] - (double)lam; }
  }
  double m = -INFINITY;
  for (int i = 0; i < ne; ++i) m = fmax(m, v[i]);
  if (m == -INFINITY) return -INFINITY;
  double s = 0.0;
  for (int i = 0; i < ne; ++i) s += exp(v[i] - m);
  return m + log(s) + acc;
}

// ---- beta.  bG = beta(G_k), bX = beta(I_k) (= beta(B_k) without durations; with them beta(B_k) comes out of the slot's delay line bC).
// Thread i hands (beta(G), beta(B)) of its first slot to thread i - 1 through xb[2][NT].
template <int NT, int R, bool MIND>
static __device__ __forceinline__ void beta_to_left(const int tid, float2* xb, int t, const float (&bG)[R], const float (&bX)[R],
                                                    const float (&bC)[MIND ? R : 1][CHAIN_BACK], const int (&dm)[MIND ? R : 1]) {
  float b = bX[0];
  if constexpr (MIND) b = chain_in(bX[0], bC[0], dm[0]);
  xb[(t & 1) * NT + tid] = make_float2(bG[0], b);
}

// the backward exchange with skip arcs, [2][XB_OPT][NT] floats: beta(G), beta(B) of the thread's first slot and beta(B) of its second
constexpr int XB_OPT = 3;
template <int NT, int R>
static __device__ __forceinline__ void beta_to_left_opt(const int tid, float* xb, int t, const float (&bG)[R], const float (&bX)[R]) {
  static_assert(R >= 2, "the widened exchange takes a thread's first TWO slots");
  float* xq = xb + (t & 1) * XB_OPT * NT + tid;
  xq[0] = bG[0];
  xq[NT] = bX[0];
  xq[2 * NT] = bX[1];
}

// the emissions of frame t that beta_{t-1} needs: the gap's, EB / EI of this thread's slots, and EB of the next thread's first slot
// (avn, wnn), which this thread gathers itself from the staged row
// OPT: EB of the next thread's SECOND slot as well (avn2, wnn2 -> ebn2): a skip arc over the next thread's first token ends there
// FILL: flagged slots emit ef (fm bit r: this thread's slot r, bit R: the next thread's first slot)
template <int NT, int R, bool WIN, bool OPT = false, bool FILL = false>
static __device__ __forceinline__ void beta_emissions(const int tid, const float* row, float l, const int (&g)[NGAP], const int4 (&av)[R], const int4& avn, int N,
                                                      int t, const int2 (&wn)[WIN ? R : 1], const int2& wnn, float& eg, float (&eb)[R],
                                                      float (&ei)[R], float& ebn, const int4& avn2 = int4(), const int2& wnn2 = int2(),
                                                      float* ebn2 = nullptr, const unsigned fm = 0, const float ef = 0.f) {
  eg = gap_emission(row, g) - l;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    eb[r] = ei[r] = -INFINITY;
    if (tid * R + r < N) {
      tok_emission(row, av[r], eb[r], ei[r]);
      eb[r] -= l;
      ei[r] -= l;
      if constexpr (FILL) {
        if ((fm >> r) & 1u) eb[r] = ei[r] = ef;
      }
      if constexpr (WIN) eb[r] = win_mask(eb[r], t, wn[r]);
    }
  }
  ebn = -INFINITY;
  if ((tid + 1) * R < N && tid + 1 < NT) {
    float ein;
    tok_emission(row, avn, ebn, ein);
    ebn -= l;
    if constexpr (FILL) {
      if ((fm >> R) & 1u) ebn = ef;
    }
    if constexpr (WIN) ebn = win_mask(ebn, t, wnn);
  }
  if constexpr (OPT) {
    float e2 = -INFINITY;
    if ((tid + 1) * R + 1 < N && tid + 1 < NT) {
      float ein;
      tok_emission(row, avn2, e2, ein);
      e2 -= l;
      if constexpr (WIN) e2 = win_mask(e2, t, wnn2);
    }
    *ebn2 = e2;
  }
}

// one frame back, beta_t -> beta_{t-1}, over this thread's slots: the neighbour's values in, the recurrences, this thread's first slot
// out, the step's barrier and, where t is a multiple of RENORM, beta's renormalisation (as alpha_frame's).  bB (MIND): beta_t(B_k) of
// every slot, chain_in of the state before this call.
// OPT: xb is the [2][XB_OPT][NT] exchange; G_k also goes to B_{k+1} where token k is optional, B_k / I_k to B_{k+2} where token k + 1
// is, each at -lam.  vB[j] = beta_t(B) + EB_t of slot j, j = 0 .. R + 1 (the next thread's first two behind this thread's own), of frame t.
// FILL: leave[r] = lse(beta_t(G_{k+1}) + EG_t, beta_t(B_{k+1}) + EB_t(k+1)), what follows token k's last frame -- two of the three
// terms of beta_{t-1}(B_k), summed first and on their own; it comes back on the scale of beta_{t-1} (this call's renormalisation taken
// off it as well), so the caller's one offset serves both.
template <int NT, int R, bool MIND, bool OPT = false, bool FILL = false>
static __device__ __forceinline__ void beta_frame(const int tid, int N, int t, float eg, const float (&eb)[R], const float (&ei)[R], float ebn, float2* xb,
                                                  float* wmax, float& subb, double& accb, float (&bG)[R], float (&bX)[R], const float (&bB)[MIND ? R : 1],
                                                  float (&bC)[MIND ? R : 1][CHAIN_BACK], const int (&dm)[MIND ? R : 1], float ebn2 = 0.f,
                                                  const SkipArcs sk = SkipArcs(), float* leave = nullptr) {
  static_assert(!(OPT && MIND), "no skip arcs in the minimum-duration lattice");
  static_assert(!(FILL && (MIND || OPT)), "no filler emission in the minimum-duration and skip lattices");
  float2 nb;
  float vB[OPT ? R + 2 : 1];
  if constexpr (OPT) {
    nb = make_float2(-INFINITY, -INFINITY);
    float nX1 = -INFINITY;
    if (tid + 1 < NT) {
      const float* xp = (const float*)xb + ((t + 1) & 1) * XB_OPT * NT + tid + 1;
      nb = make_float2(xp[0], xp[NT]);
      nX1 = xp[2 * NT];
    }
    nb.x -= subb;
    nb.y -= subb;
    nX1 -= subb;
#pragma unroll
    for (int r = 0; r < R; ++r) vB[r] = bX[r] + eb[r];
    vB[R] = nb.y + ebn;
    vB[R + 1] = nX1 + ebn2;
  } else {
    nb = tid + 1 < NT ? xb[((t + 1) & 1) * NT + tid + 1] : make_float2(-INFINITY, -INFINITY);
    nb.x -= subb;
    nb.y -= subb;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {                // ascending: slot r + 1's values of frame t are still in place
    const int k = tid * R + r;
    if constexpr (OPT) {
      const float nG = r + 1 < R ? bG[r + 1 < R ? r + 1 : 0] : nb.x;
      float x = lae3(bX[r] + ei[r], nG + eg, vB[r + 1]);
      if (sk.opt(r + 2)) x = lae2(x, vB[r + 2] - sk.lam);
      float y = lae2(bG[r] + eg, vB[r]);
      if (sk.opt(r + 1)) y = lae2(y, vB[r + 1] - sk.lam);
      bG[r] = k <= N ? y : -INFINITY;
      bX[r] = k < N ? x : -INFINITY;
      continue;
    }
    const float nG = r + 1 < R ? bG[r + 1 < R ? r + 1 : 0] : nb.x;
    float nX = r + 1 < R ? bX[r + 1 < R ? r + 1 : 0] : nb.y;
    if constexpr (MIND) nX = r + 1 < R ? bB[r + 1 < R ? r + 1 : 0] : nb.y;   // the next token is entered through its B
    const float nE = r + 1 < R ? eb[r + 1 < R ? r + 1 : 0] : ebn;
    float x;
    if constexpr (FILL) {
      const float lv = lae2(nG + eg, nX + nE);
      leave[r] = k < N ? lv : -INFINITY;
      x = lae2(bX[r] + ei[r], lv);
    } else {
      x = lae3(bX[r] + ei[r], nG + eg, nX + nE);
    }
    float bb = bX[r];
    if constexpr (MIND) bb = bB[r];
    const float y = lae2(bG[r] + eg, bb + eb[r]);
    if constexpr (MIND) chain_shift_back(bC[r], bX[r], ei[r]);
    bG[r] = k <= N ? y : -INFINITY;
    bX[r] = k < N ? x : -INFINITY;
  }
  if constexpr (OPT) beta_to_left_opt<NT, R>(tid, (float*)xb, t, bG, bX);
  else beta_to_left<NT, R, MIND>(tid, xb, t, bG, bX, bC, dm);
  const bool renorm = (t & (RENORM - 1)) == 0;
  if (renorm) {
    float lm = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(bG[r], bX[r]));
    renorm_publish(lm, wmax);
  }
  __syncthreads();
  subb = 0.f;
  if (renorm) {
    float M = renorm_max<NT / 64>(wmax);
    if (!(M > -INFINITY)) M = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) { bG[r] -= M; bX[r] -= M; }
    if constexpr (FILL) {
#pragma unroll
      for (int r = 0; r < R; ++r) leave[r] -= M;
    }
    if constexpr (MIND) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < CHAIN_BACK; ++j) bC[r][j] -= M;
    }
    subb = M;
    accb += (double)M;
  }
}


}  // namespace lattice
