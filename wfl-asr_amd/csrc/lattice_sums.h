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
template <int NT>
static __device__ __forceinline__ double frame_lse(const int tid, const float* Z, long ldl, int T, int C, float* lse, double* red) {
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
template <int NT, int R, bool WIN, bool MIND, class Hook = NoHook>
static __device__ __forceinline__ void alpha_frame(const int tid, const float* row, float l, const int (&g)[NGAP], const int4 (&av)[R], int N, int t, float2* xf,
                                                   float* wmax, float& sub, double& acc, float (&G)[R], float (&B)[R], float (&I)[R], float (&H)[MIND ? R : 1][CHAIN],
                                                   const int (&dm)[MIND ? R : 1], const int2 (&wn)[WIN ? R : 1], Hook hook = Hook()) {
  const float eg = gap_emission(row, g) - l;
  const float2 nb = alpha_from_left<NT>(tid, xf, t, sub);
#pragma unroll
  for (int r = R - 1; r >= 0; --r) {           // descending: slot r - 1's previous-frame values are still in place
    const int k = tid * R + r;
    const float in = alpha_enter<R, MIND>(r, G, B, I, nb, dm);
    float x = B[r];                            // what I_k is entered from
    if constexpr (MIND) x = chain_out(B[r], H[r], dm[r]);
    const float ii = lae2(I[r], x);
    hook(r, k, in);
    float eb = -INFINITY, ei = -INFINITY;
    if (k < N) {
      tok_emission(row, av[r], eb, ei);
      eb -= l;
      ei -= l;
      if constexpr (WIN) eb = win_mask(eb, t, wn[r]);
    }
    G[r] = k <= N ? in + eg : -INFINITY;
    if constexpr (MIND) chain_shift(H[r], B[r], ei, dm[r]);
    B[r] = in + eb;
    I[r] = ii + ei;
  }
  alpha_to_right<NT, R, MIND>(tid, xf, t, B, I, dm);
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

// ---- beta.  bG = beta(G_k), bX = beta(I_k) (= beta(B_k) without durations; with them beta(B_k) comes out of the slot's delay line bC).
// Thread i hands (beta(G), beta(B)) of its first slot to thread i - 1 through xb[2][NT].
template <int NT, int R, bool MIND>
static __device__ __forceinline__ void beta_to_left(const int tid, float2* xb, int t, const float (&bG)[R], const float (&bX)[R],
                                                    const float (&bC)[MIND ? R : 1][CHAIN_BACK], const int (&dm)[MIND ? R : 1]) {
  float b = bX[0];
  if constexpr (MIND) b = chain_in(bX[0], bC[0], dm[0]);
  xb[(t & 1) * NT + tid] = make_float2(bG[0], b);
}

// the emissions of frame t that beta_{t-1} needs: the gap's, EB / EI of this thread's slots, and EB of the next thread's first slot
// (avn, wnn), which this thread gathers itself from the staged row
template <int NT, int R, bool WIN>
static __device__ __forceinline__ void beta_emissions(const int tid, const float* row, float l, const int (&g)[NGAP], const int4 (&av)[R], const int4& avn, int N,
                                                      int t, const int2 (&wn)[WIN ? R : 1], const int2& wnn, float& eg, float (&eb)[R],
                                                      float (&ei)[R], float& ebn) {
  eg = gap_emission(row, g) - l;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    eb[r] = ei[r] = -INFINITY;
    if (tid * R + r < N) {
      tok_emission(row, av[r], eb[r], ei[r]);
      eb[r] -= l;
      ei[r] -= l;
      if constexpr (WIN) eb[r] = win_mask(eb[r], t, wn[r]);
    }
  }
  ebn = -INFINITY;
  if ((tid + 1) * R < N && tid + 1 < NT) {
    float ein;
    tok_emission(row, avn, ebn, ein);
    ebn -= l;
    if constexpr (WIN) ebn = win_mask(ebn, t, wnn);
  }
}

// one frame back, beta_t -> beta_{t-1}, over this thread's slots: the neighbour's values in, the recurrences, this thread's first slot
// out, the step's barrier and, where t is a multiple of RENORM, beta's renormalisation (as alpha_frame's).  bB (MIND): beta_t(B_k) of
// every slot, chain_in of the state before this call.
template <int NT, int R, bool MIND>
static __device__ __forceinline__ void beta_frame(const int tid, int N, int t, float eg, const float (&eb)[R], const float (&ei)[R], float ebn, float2* xb,
                                                  float* wmax, float& subb, double& accb, float (&bG)[R], float (&bX)[R], const float (&bB)[MIND ? R : 1],
                                                  float (&bC)[MIND ? R : 1][CHAIN_BACK], const int (&dm)[MIND ? R : 1]) {
  float2 nb = tid + 1 < NT ? xb[((t + 1) & 1) * NT + tid + 1] : make_float2(-INFINITY, -INFINITY);
  nb.x -= subb;
  nb.y -= subb;
#pragma unroll
  for (int r = 0; r < R; ++r) {                // ascending: slot r + 1's values of frame t are still in place
    const int k = tid * R + r;
    const float nG = r + 1 < R ? bG[r + 1 < R ? r + 1 : 0] : nb.x;
    float nX = r + 1 < R ? bX[r + 1 < R ? r + 1 : 0] : nb.y;
    if constexpr (MIND) nX = r + 1 < R ? bB[r + 1 < R ? r + 1 : 0] : nb.y;   // the next token is entered through its B
    const float nE = r + 1 < R ? eb[r + 1 < R ? r + 1 : 0] : ebn;
    const float x = lae3(bX[r] + ei[r], nG + eg, nX + nE);
    float bb = bX[r];
    if constexpr (MIND) bb = bB[r];
    const float y = lae2(bG[r] + eg, bb + eb[r]);
    if constexpr (MIND) chain_shift_back(bC[r], bX[r], ei[r]);
    bG[r] = k <= N ? y : -INFINITY;
    bX[r] = k < N ? x : -INFINITY;
  }
  beta_to_left<NT, R, MIND>(tid, xb, t, bG, bX, bC, dm);
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
