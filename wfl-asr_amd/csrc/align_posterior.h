// Forward-backward over the forced-alignment lattice of wfl_align: per-token posteriors of a Viterbi path (wfl_align_posterior,
// include/wfl_asr.h).  The sum-product twin of csrc/align.hip; the reference has no counterpart (it reports no confidence for its
// string match).
//
// Lattice, emissions, start / end states and caps are wfl_align's, and so is their code: csrc/lattice.h holds the caps, the
// configurations, the shared LDS layout, lattice setup with its status codes, the logits stage ring, the emission gathers, the
// renormalisation halves and the host side of a ragged batch.  csrc/lattice_sums.h holds the sum-product sweeps -- one frame of alpha
// and of beta over a thread's slots, their renormalisation, the per-frame log-sum-exp, the staged ring's side rings, logZ -- which
// csrc/align_edits.hip runs as well.  Here is what is this kernel's own: the status-8 check of `tok`, the checkpoints and the block
// buffer, the gammas and the per-token moments.  States G_k = 3k, B_k = 3k + 1, I_k = 3k + 2:
//   alpha_t(G_k) = EG_t + lse(alpha_{t-1}(G_k), alpha_{t-1}(I_{k-1}), alpha_{t-1}(B_{k-1}))      alpha_t(B_k): the same sum + EB_t(k)
//   alpha_t(I_k) = EI_t(k) + lse(alpha_{t-1}(I_k), alpha_{t-1}(B_k))
//   beta_{t-1}(G_k) = lse(beta_t(G_k) + EG_t, beta_t(B_k) + EB_t(k))
//   beta_{t-1}(B_k) = beta_{t-1}(I_k) = lse(beta_t(I_k) + EI_t(k), beta_t(G_{k+1}) + EG_t, beta_t(B_{k+1}) + EB_t(k+1))
//   logZ = lse(alpha_{T-1}(G_N), alpha_{T-1}(I_{N-1}), alpha_{T-1}(B_{N-1})),   gamma_t(s) = exp(alpha_t(s) + beta_t(s) - logZ).
// beta of B_k and I_k are equal (same successors), so the backward sweep carries two values per token.
//
// One workgroup per clip, configurations and slot ownership from lattice.h: thread i owns the token slots i R .. i R + R - 1 in
// registers.  Per frame one float2 crosses between neighbouring threads through LDS, one barrier per frame: the forward sweep takes
// (alpha(B), alpha(I)) of the last slot of thread i - 1, the backward sweep (beta(G), beta(B)) of the first slot of thread i + 1 (the
// emission of that slot's B state is gathered by thread i itself, from the staged row).  Every per-token output is accumulated by
// the thread that owns the token; no reduction over the block per frame.  Every 16 frames the block's maximum is subtracted from the
// states (alpha and beta separately) and added to a double, so the fp32 log-domain values never grow with T.
//
// Memory: the alpha lattice is never stored.  Sweep 1 runs forward over the clip and keeps a checkpoint of the registers every
// POST_W frames; then, block by block from the last one, sweep 2 recomputes the block's POST_W frames of alpha from its checkpoint
// into a block buffer and sweep 3 walks beta down the block, combining.  Every thread reads back only what it wrote itself.
// Workspace per clip: lse[T] | checkpoints' offsets | checkpoints | one block (wfl_align_posterior_workspace_bytes).
//
// wfl_align_posterior_windowed is the same kernel instantiated with WIN: EB passes through lattice.h's win_mask wherever it is gathered --
// alpha, beta's own slots, and the next thread's first slot (ebn) -- with the windows of a thread's slots (and of that one slot) in
// registers; a tok that opens a token outside its window is status 8, logZ = -inf status 1.
//
// wfl_align_min_duration_posterior is the kernel instantiated with MIND (with and without WIN): the sums over the lattice of
// wfl_align_min_duration.  Alpha carries lattice.h's chain beside G, B, I (chain_out / chain_shift, as the search), beta a delay line per
// slot (chain_in / chain_shift_back): beta(B_k) differs from beta(I_k) there, bX is beta(I_k) and beta(B_k) comes out of the line.  The
// block buffer stays at G, B, I: gamma_t(H_k^j) = gamma_{t-j+1}(B_k), so the chain's share of a run's occupancy is gamma_t(B_k) times
// the overlap of [t, t + D_k - 2] with the run; only the checkpoints hold the chain (PCfg::SM).  A D_k outside 1 .. 8 is status 4, a run
// shorter than its D_k status 8, and a clip without any path status 1 before its tok is judged.
//
// wfl_align_optional_posterior is the kernel instantiated with OPT (with and without WIN, never with MIND): the sums over the skip
// lattice of wfl_align_optional, a path weighing exp(sum_t e_t - lambda * its skipped tokens).  With in_k(t) = alpha_enter of token k,
//   alpha_t(B_k) = EB_t(k) + lse(in_k(t), in_{k-1}(t) - lambda where tok_opt[k-1])                       (G_k, I_k as above)
//   beta_{t-1}(G_k) gains beta_t(B_{k+1}) + EB_t(k+1) - lambda where tok_opt[k], beta_{t-1}(B_k) = beta_{t-1}(I_k) gains
//   beta_t(B_{k+2}) + EB_t(k+2) - lambda where tok_opt[k+1]; where tok_opt[N-1] the ends G_{N-1}, I_{N-2}, B_{N-2} count at -lambda.
// The exchanges widen to five floats forward (the search's: B, I, G of the last slot, B, I of the one before) and three backward
// (beta(G), beta(B) of slot 0, beta(B) of slot 1; EB of that second slot is gathered by the reader: avn2, wnn2), still one barrier per
// frame.  Every labelling is one path and a path enters B_k at most once, so m0 = sum_t gamma_t(B_k) is the posterior that token k is
// present: keep_post.  A tok that misses a token that is not optional, or two neighbours, is status 8 -- after sweep 1, as with
// durations: a clip without any path is status 1 first.
//
// wfl_align_filler_posterior is the kernel instantiated with FILL (with and without WIN, never with MIND or OPT): the sums over the
// lattice of wfl_align_filler.  States and arcs are wfl_align_posterior's; a flagged token emits EB = EI = (max_c z_t[c] - lse_t) - phi.
// frame_lse, which takes every row's maximum anyway, keeps that value per frame in the clip's workspace (fem[T], behind the block
// buffer); it travels through the stage rings beside the log-sum-exp (fring), so a frame of either sweep reads one float and never
// scans a row.  A clip without a flag (the same in every thread) computes, stages and reads none of it.  New here as well: the moments
// of every token's END.  omega_t(k) = exp(lse(alpha_t(B_k), alpha_t(I_k)) + leave_k(t+1) - logZ), leave_k(t+1) what follows the token
// at frame t + 1 -- beta_frame hands it out (two of the three terms of beta_t(B_k)) on the scale of beta_t, and it is CARRIED into the
// next iteration of the backward loop, where alpha_t is in hand: so it crosses the boundary of a recomputed block like beta itself
// (alpha of frame t_lo - 1 is not in the block that produced leave(t_lo)).  At T - 1 leave is 0 for token N - 1 and -inf elsewhere:
// beta's own start values.  The last frame of every Viterbi run comes through first[] as with durations.
//
// The per-frame log-sum-exp of the logits is computed once (double, expf), stored in fp32 and subtracted from the gathered logits;
// what the fp32 rounding of it loses is summed in double and given back to logZ (it is common to every path).
//
// This header holds the kernel and the host path every entry shares.  csrc/align_posterior.hip instantiates wfl_align_posterior and
// wfl_align_posterior_windowed from it, csrc/align_min_duration_posterior.hip the kernels with the minimum-duration chain (MIND) -- a
// translation unit of its own because those are compiled without the SLP vectoriser (build.py), which must not reach the others.
// csrc/align_optional_posterior.hip instantiates the kernels with the skip arcs (OPT), so that the other objects keep their code.
// csrc/align_filler_posterior.hip instantiates the kernels with the filler emission (FILL), for the same reason.
// Everything here is in an unnamed namespace: each of the files has its own copy, and instantiates only its own kernels.
#pragma once
#include "lattice_sums.h"
#include "wfl_asr.h"

#include <limits.h>

namespace {

using namespace lattice;

constexpr int POST_W = 128;                // frames per recomputed block (a multiple of the renormalisation period)
static_assert(POST_W % RENORM == 0, "a block ends on a renormalisation");

struct PostLaunch {
  const float* logits;
  long ldl;
  int C;
  const int* tok_cls;  // [total tokens][4][2]
  const int* gap_cls;  // [n_clips][8]
  const int* tok;      // wfl_align's output, same rows as the logits
  float* ws;           // LatClip::ws_off: the clip's workspace, in floats
  float* logz;
  float* tok_post;
  float* start_mean;
  float* start_sd;
  int* status;
  int n;
  LatClip clip[CLIPS_PER_LAUNCH];
  const int* tok_win;  // [total tokens][2] = (lo, hi), the windowed kernels alone (last: the other fields stay where they were)
  const int* tok_min;  // [total tokens] D_k, the minimum-duration kernels alone
};

// a clip's workspace in floats: [lse: round64(T)] [checkpoint offsets: round64(2 nblk)] [checkpoints: nblk SC] [block: POST_W S]
// SC: a checkpoint's floats -- S, and with minimum durations the chain states of every slot as well (PCfg::SM)
struct PostLayout {
  long ckacc, ckpt, blk, total;
  int nblk;
  __host__ __device__ PostLayout(int T, long SC, long S) {
    nblk = (T + POST_W - 1) / POST_W;
    ckacc = round64(T);
    ckpt = ckacc + round64(2L * nblk);
    blk = ckpt + (long)nblk * SC;
    total = blk + (long)POST_W * S;
  }
};

// the kernel arguments of wfl_align_optional_posterior: PostLaunch (which stays the record it was for the other entries) and, behind
// it, the optional tokens
struct PostLaunchOpt : PostLaunch {
  const int* tok_opt;  // [total tokens] 0 | 1
  float* keep_post;    // [total tokens]
  float lambda;        // the skip penalty, nats
};

// the kernel arguments of wfl_align_filler_posterior: PostLaunch and, behind it, the filler tokens and the end moments
struct PostLaunchFill : PostLaunch {
  const int* tok_fill;  // [total tokens] 0 | 1
  float* end_mean;      // [total tokens]
  float* end_sd;        // [total tokens]
  float phi;            // the filler penalty, nats per frame
};

// OPT: the exchanges of the skip lattice, [2][XF_OPT][NT] and [2][XB_OPT][NT] floats instead of [2][NT] float2 each
// FILL: one side ring more, the staged rows' filler emission, behind everything else
template <int NT, int R, bool OPT = false, bool FILL = false>
struct PCfg : LdsBase<NT, R, NT * R * 4 + (OPT ? 2 * (XF_OPT + XB_OPT) * NT * 4 : 2 * 2 * NT * 8)> {   // its own between alt and wmax: first[] and the two neighbour exchanges
  static constexpr long S = (long)NT * R * 3;            // floats of one frame's alpha (and of one checkpoint)
  static constexpr long SM = (long)NT * R * (3 + CHAIN); // floats of one checkpoint with the minimum-duration chain
  static constexpr int OFF_FIRST = PCfg::OFF_X;                    // first frame of every token's Viterbi run
  static constexpr int OFF_XF = OFF_FIRST + NT * R * 4;            // forward neighbour exchange: [2][NT] float2
  static constexpr int OFF_XB = OFF_XF + (OPT ? 2 * XF_OPT * NT * 4 : 2 * NT * 8);   // backward neighbour exchange
  static constexpr int OFF_OFFA = PCfg::OFF_OWN;                   // alpha's offset of every frame of the block (double)
  static constexpr int OFF_LRING = OFF_OFFA + POST_W * 8;          // staged rows' log-sum-exp
  static constexpr int OFF_TRING = OFF_LRING + 2 * FMAX * 4;       // staged rows' Viterbi token
  static constexpr int OFF_MISC = OFF_TRING + 2 * FMAX * 4;
  static constexpr int OFF_FRING = OFF_MISC + 64;                  // FILL: staged rows' filler emission
  static constexpr int LDS = OFF_FRING + (FILL ? 2 * FMAX * 4 : 0);
};

// WIN: the start windows of wfl_align_posterior_windowed (lattice.h win_mask); false is wfl_align_posterior's kernel
// MIND: the minimum durations of wfl_align_min_duration_posterior (lattice.h chain_*); false leaves the two kernels above without a
// trace of the chain (lattice_sums.h takes both as template values)
// OPT: the skip arcs of wfl_align_optional_posterior (lattice_sums.h OPT), never with MIND; keep_post[k] = sum_t gamma_t(B_k), the
// posterior of the paths that hold token k (a path enters B_k at most once).  Without OPT the kernels keep their arguments (PostLaunch)
// and their code; only their names carry one template value more.
// FILL: the filler emission of wfl_align_filler_posterior (lattice_sums.h FILL), never with MIND or OPT, and the end moments
// end_mean / end_sd of every token.  Without FILL the kernels keep their arguments and their code.
template <int NT, int R, bool WIN, bool MIND, bool OPT, bool FILL = false>
__global__ __launch_bounds__(NT) void post_kernel(
    std::conditional_t<OPT, PostLaunchOpt, std::conditional_t<FILL, PostLaunchFill, PostLaunch>> a) {
  static_assert(!(OPT && MIND), "no skip arcs in the minimum-duration lattice");
  static_assert(!(FILL && (MIND || OPT)), "no filler emission in the minimum-duration and skip lattices");
  using K = PCfg<NT, R, OPT, FILL>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  int* first = (int*)(lds + K::OFF_FIRST);
  float2* xf = (float2*)(lds + K::OFF_XF);
  float2* xb = (float2*)(lds + K::OFF_XB);
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  double* offa = (double*)(lds + K::OFF_OFFA);
  float* lring = (float*)(lds + K::OFF_LRING);
  int* tring = (int*)(lds + K::OFF_TRING);
  int* misc = (int*)(lds + K::OFF_MISC);
  float* fin = (float*)(misc + 4);

  const LatClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = cl.T, N = cl.N, C = a.C;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  const int* tokp = a.tok + cl.frame_off;
  const float NEG = -INFINITY;

  int g[NGAP];
  int st;
  SkipArcs sk;
  unsigned fm = 0;                             // FILL: bit r = "this thread's slot r is a filler", bit R = the next thread's first slot
  bool anyfill = false;                        // FILL: the clip has a filler (the same in every thread)
  if constexpr (FILL) {
    // the clip's flags, as csrc/align.hip's FILL search judges them: a value other than 0 | 1 is status 4, after setup's 2 and 1
    if (tid == 0) { misc[2] = 0; misc[3] = 0; }
    __syncthreads();
    bool any = false, badf = false;
    for (int k = tid; k < N; k += NT) {
      const int f = a.tok_fill[cl.tok_off + k];
      any |= f != 0;
      badf |= f != 0 && f != 1;
    }
    if (any) misc[2] = 1;
    if (badf) misc[3] = 1;
    __syncthreads();
    anyfill = misc[2] != 0;
    const bool bad_flag = misc[3] != 0;
    __syncthreads();                            // (lattice_setup writes misc[0])
    st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
    if (st == 0 && bad_flag) st = 4;
    if (st == 0) {
#pragma unroll
      for (int r = 0; r <= R; ++r) {
        const int k = tid * R + r;
        if (k < N && (r < R || tid + 1 < NT) && a.tok_fill[cl.tok_off + k] != 0) fm |= 1u << r;
      }
    }
  } else if constexpr (OPT) {
    // the clip's flags first, as csrc/align.hip's OPT search judges them: a value other than 0 | 1 is status 4; a clip without any flag
    // and with fewer frames than tokens is wfl_align_posterior's status 1, whatever its classes are
    if (tid == 0) { misc[2] = 0; misc[3] = 0; }
    __syncthreads();
    bool any = false, badf = false;
    for (int k = tid; k < N; k += NT) {
      const int f = a.tok_opt[cl.tok_off + k];
      any |= f != 0;
      badf |= f != 0 && f != 1;
    }
    if (any) misc[2] = 1;
    if (badf) misc[3] = 1;
    __syncthreads();
    const bool none = misc[2] == 0, bad_flag = misc[3] != 0;
    __syncthreads();                            // (lattice_setup writes misc[0])
    if (N <= NT * R - 1 && N <= MAX_TOKENS && T < N && none) st = 1;
    else st = lattice_setup<NT, R, true>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
    if (st == 0 && bad_flag) st = 4;
    if (st == 0) sk = load_skip_arcs<R>(tid, a.tok_opt, cl.tok_off, N, a.lambda);
  } else {
    st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
  }
  int2 wn[WIN ? R : 1];                        // this thread's slots' start windows, in registers, and the next thread's first slot's
  int2 wnn = make_int2(0, WIN_OPEN_HI);
  int2 wnn2 = make_int2(0, WIN_OPEN_HI);       // OPT: and its second slot's
  if constexpr (WIN) {
    if (st == 0) {
      load_windows<R>(a.tok_win, cl.tok_off, N, wn);
      wnn = load_window(a.tok_win, cl.tok_off, (tid + 1) * R, N);
      if constexpr (OPT) wnn2 = load_window(a.tok_win, cl.tok_off, (tid + 1) * R + 1, N);
    }
  }
  int dm[MIND ? R : 1];                        // this thread's slots' minimum durations, in registers
  int fst[(MIND || FILL) ? R : 1], lst[(MIND || FILL) ? R : 1];    // first and last frame of their Viterbi runs (FILL: the end moments' origin)
  // with durations a tok that is no path is reported only after sweep 1: a clip that has no path at all is status 1 first (the search
  // writes tok = -1 for such a clip, and its status is the one to pass on)
  bool notpath = false;
  if constexpr (MIND) {
    if (st == 0) {                             // (the same in every thread).  A D_k outside 1 .. MAX_MIN_FRAMES: status 4
      if (tid == 0) misc[3] = 0;
      __syncthreads();
      bool bad = false;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        dm[r] = load_min(a.tok_min, cl.tok_off, tid * R + r, N);
        if (dm[r] < 1 || dm[r] > MAX_MIN_FRAMES) bad = true;
      }
      if (bad) misc[3] = 1;
      __syncthreads();
      if (misc[3]) st = 4;
    }
  }
  if (st == 0 && T > 0) {
    // the first frame of every token's Viterbi run; a tok that is not a path of this lattice (a token missing, a value out of range)
#pragma unroll
    for (int r = 0; r < R; ++r) first[tid * R + r] = INT_MAX;
    __syncthreads();                           // (and every thread has read setup's flag before this phase may raise it again)
    bool bad = false;
    for (int t = tid; t < T; t += NT) {
      const int k = tokp[t];
      if (k < -1 || k >= N) bad = true;
      else if (k >= 0 && (t == 0 || tokp[t - 1] != k)) atomicMin(&first[k], t);
    }
    if (bad) misc[0] = 1;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (tid * R + r < N) {
        const int f = first[tid * R + r];
        if constexpr (OPT) {
          // a token tok does not hold: a path only where it is optional and the next one is held (one skip between two kept tokens);
          // its window is never consulted
          if (f == INT_MAX) {
            if (!sk.opt(r + 1) || (tid * R + r + 1 < N && first[tid * R + r + 1] == INT_MAX)) misc[0] = 1;
          } else if constexpr (WIN) {
            if (f < wn[r].x || f > wn[r].y) misc[0] = 1;
          }
        } else {
          if (f == INT_MAX) misc[0] = 1;
          if constexpr (WIN) {
            if (f < wn[r].x || f > wn[r].y) misc[0] = 1;   // a token opens outside its window: not a path of this lattice either
          }
        }
      }
    __syncthreads();
    if (misc[0]) {
      if constexpr (MIND || OPT || FILL) notpath = true;   // (OPT, FILL: the search writes tok = -1 for a clip without path, too: 1 comes before 8)
      else st = 8;
    }
    if constexpr (MIND || FILL) {
      // the last frame of every run, through the same LDS words (the chain's share of a run's occupancy needs both ends before the
      // backward sweep reaches the run); a run shorter than its D_k is not a path of this lattice
      if (st == 0 && !notpath) {               // (the same in every thread; misc[0] is still 0)
#pragma unroll
        for (int r = 0; r < R; ++r) fst[r] = tid * R + r < N ? first[tid * R + r] : 0;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) first[tid * R + r] = -1;
        __syncthreads();
        for (int t = tid; t < T; t += NT) {
          const int k = tokp[t];
          if (k >= 0 && (t == T - 1 || tokp[t + 1] != k)) atomicMax(&first[k], t);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
          lst[r] = tid * R + r < N ? first[tid * R + r] : 0;
          if constexpr (MIND) {
            if (tid * R + r < N && lst[r] - fst[r] + 1 < dm[r]) misc[0] = 1;
          }
        }
        if constexpr (MIND) {
          __syncthreads();
          if (misc[0]) notpath = true;
        }
      }
    }
  }
  if (st != 0 || T == 0) {
    for (int k = tid; k < N; k += NT) {
      a.tok_post[cl.tok_off + k] = 0.f;
      a.start_mean[cl.tok_off + k] = 0.f;
      a.start_sd[cl.tok_off + k] = 0.f;
      if constexpr (OPT) a.keep_post[cl.tok_off + k] = 0.f;
      if constexpr (FILL) { a.end_mean[cl.tok_off + k] = 0.f; a.end_sd[cl.tok_off + k] = 0.f; }
    }
    if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = st; }
    return;
  }

  const PostLayout lay(T, MIND ? K::SM : K::S, K::S);
  constexpr long SC = MIND ? K::SM : K::S;     // floats of a checkpoint
  float* ws = a.ws + cl.ws_off;
  float* lse = ws;
  double* ckacc = (double*)(ws + lay.ckacc);
  float* ckpt = ws + lay.ckpt;
  float* blk = ws + lay.blk;

  // the thread index lattice_sums.h's pieces get.  Measured, five alternating rounds against the build before the pieces were shared
  // (profiles/sumproduct_sweeps_ab.txt): handed `tid`, the 256 x 2 kernel with the chain is 0.6 to 0.8 % slower and the one with
  // windows alone level; handed a fresh read in every piece, the other way round.  Same value, another schedule; each gets its own.
  auto me = [&]() -> int {
    if constexpr (MIND) return threadIdx.x;
    else return tid;
  };

  // ---- the per-frame log-sum-exp, in fp32 for the sweeps; what its rounding loses, in double for logZ
  // FILL: and the filler emission of every frame, behind the block buffer; a clip without a filler has none
  float* fem = nullptr;
  float* fring = nullptr;
  if constexpr (FILL) {
    if (anyfill) fem = ws + lay.total;
    fring = (float*)(lds + K::OFF_FRING);
  }
  double lres;
  if constexpr (FILL) lres = frame_lse<NT, true>(me(), Z, a.ldl, T, C, lse, red, fem, a.phi);
  else lres = frame_lse<NT>(me(), Z, a.ldl, T, C, lse, red);

  // ---- staging of the logits rows, with their log-sum-exp and Viterbi token (the backward sweep runs one stage ahead as well)
  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;
  float pre_l = 0.f;
  int pre_t = -1;
  float pre_f = 0.f;                           // FILL: the stage's filler emissions, beside pre_l
  auto load_stage = [&](int c) {
    stage_load<true>(me(), stage, c, lse, tokp, pre_l, pre_t);
    if constexpr (FILL) {
      if (anyfill) pre_f = (tid < F && c >= 0 && c * F + tid < T) ? fem[c * F + tid] : 0.f;
    }
  };
  auto store_stage = [&](int c) {
    stage_store<true>(me(), stage, c, lring, tring, pre_l, pre_t);
    if constexpr (FILL) {
      if (anyfill && tid < F) fring[(c & 1) * FMAX + tid] = pre_f;
    }
  };
  auto filler_emission = [&](int c, int tin) -> float {   // FILL: what a filler emits at the staged frame; one LDS read
    if constexpr (FILL) {
      if (anyfill) return fring[(c & 1) * FMAX + tin];
    }
    return 0.f;
  };

  int4 av[R];                                   // this thread's slots' alternatives
#pragma unroll
  for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  const int4 avn = tid + 1 < NT ? alt[(tid + 1) * R] : make_int4(-1, -1, -1, -1);   // the next thread's first slot
  int4 avn2 = make_int4(-1, -1, -1, -1);                                            // OPT: and its second
  if constexpr (OPT) {
    if (tid + 1 < NT) avn2 = alt[(tid + 1) * R + 1];
  }

  // ---- the forward sweep over frames t0 .. t1 - 1, from the clip's start (t0 = 0) or from checkpoint t0 / POST_W
  float G[R], B[R], I[R];
  float H[MIND ? R : 1][CHAIN];                // the chain states H^2 .. H^{MAX_MIN_FRAMES - 1} of every slot (alpha)
  double acc = 0.0;                            // what alpha's renormalisations subtracted
  auto forward = [&](int t0, int t1, bool keep) {
    if (t0 == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) G[r] = B[r] = I[r] = NEG;
      if constexpr (MIND) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < CHAIN; ++j) H[r][j] = NEG;
      }
      if (tid == 0) G[0] = 0.f;                // a virtual frame -1 in G_0: frame 0 starts in G_0 or B_0
      acc = 0.0;
    } else {
      const float* ck = ckpt + (long)(t0 / POST_W) * SC;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        G[r] = ck[(r * 3 + 0) * NT + tid];
        B[r] = ck[(r * 3 + 1) * NT + tid];
        I[r] = ck[(r * 3 + 2) * NT + tid];
      }
      if constexpr (MIND) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < CHAIN; ++j) H[r][j] = ck[(R * 3 + r * CHAIN + j) * NT + tid];
      }
      acc = ckacc[t0 / POST_W];
    }
    if constexpr (OPT) alpha_to_right_opt<NT, R>(me(), (float*)xf, t0 + 1, G, B, I);
    else alpha_to_right<NT, R, MIND>(me(), xf, t0 + 1, B, I, dm);
    float sub = 0.f;
    int c = t0 / F, tin = t0 - c * F;
    stage_start(c, 1, load_stage, store_stage);
    for (int t = t0; t < t1; ++t, ++tin) {
      if (tin == F) {
        ++c;
        tin = 0;
        stage_enter(c, 1, load_stage, store_stage);
      }
      if constexpr (FILL)
        alpha_frame<NT, R, WIN, MIND, NoHook, false, true>(me(), stage.row(c, tin), lring[(c & 1) * FMAX + tin], g, av, N, t, xf, wmax, sub, acc, G, B, I, H, dm,
                                                           wn, NoHook(), SkipArcs(), fm, filler_emission(c, tin));
      else if constexpr (OPT)
        alpha_frame<NT, R, WIN, MIND, NoHook, true>(me(), stage.row(c, tin), lring[(c & 1) * FMAX + tin], g, av, N, t, xf, wmax, sub, acc, G, B, I, H, dm, wn,
                                                    NoHook(), sk);
      else
        alpha_frame<NT, R, WIN, MIND>(me(), stage.row(c, tin), lring[(c & 1) * FMAX + tin], g, av, N, t, xf, wmax, sub, acc, G, B, I, H, dm, wn);
      if (keep) {                              // the block's alpha, for the backward sweep of the same thread
        float* o = blk + (long)(t - t0) * K::S;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          o[(r * 3 + 0) * NT + tid] = G[r];
          o[(r * 3 + 1) * NT + tid] = B[r];
          o[(r * 3 + 2) * NT + tid] = I[r];
        }
        if (tid == 0) offa[t - t0] = acc;
      } else if ((t + 1) % POST_W == 0 && t + 1 < T) {   // (a block ends on a renormalisation: sub is spent)
        float* o = ckpt + (long)((t + 1) / POST_W) * SC;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          o[(r * 3 + 0) * NT + tid] = G[r];
          o[(r * 3 + 1) * NT + tid] = B[r];
          o[(r * 3 + 2) * NT + tid] = I[r];
        }
        if constexpr (MIND) {
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < CHAIN; ++j) o[(R * 3 + r * CHAIN + j) * NT + tid] = H[r][j];
        }
        if (tid == 0) ckacc[(t + 1) / POST_W] = acc;
      }
    }
  };

  // ---- sweep 1: alpha over the whole clip, checkpoints, logZ
  forward(0, T, false);
  publish_end_states<R>(N, G, B, I, fin);
  if constexpr (MIND) {                         // B_{N-1} ends the clip only where D_{N-1} == 1 (the thread that published it)
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (tid * R + r == N - 1 && dm[r] > 1) fin[2] = NEG;
  }
  if constexpr (OPT) {                          // the ends that skip token N - 1: fin[3] = G_{N-1}, fin[4] = I_{N-2}, fin[5] = B_{N-2}
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = tid * R + r;
      if (k == N - 1) fin[3] = G[r];
      if (k == N - 2) { fin[4] = I[r]; fin[5] = B[r]; }
    }
  }
  __syncthreads();
  if constexpr (OPT) {                          // -inf: too few frames for the tokens that may not be skipped, or windows that cannot be met
    if (tid == 0) red[0] = end_logz_opt(fin, N, acc, N >= 1 && a.tok_opt[cl.tok_off + (N >= 1 ? N - 1 : 0)] != 0, sk.lam);
  } else {
    if (tid == 0) red[0] = end_logz<WIN || MIND || FILL>(fin, N, acc);   // -inf: no path opens every token inside its window (meets every duration)
  }
  __syncthreads();                             // (ckacc[] of thread 0 is visible to the block as well)
  const double logZ = red[0];                  // on the fp32 log-sum-exps; the clip's logZ is logZ - lres
  if constexpr (WIN || MIND || OPT || FILL) {   // (FILL without windows: a penalty that takes every path to -inf)
    if (logZ == -INFINITY || ((MIND || OPT || FILL) && notpath)) {   // status 1 (with durations, skip arcs or fillers 8: paths exist, tok is none of them) and zeros
      int code = 1;
      if constexpr (MIND || OPT || FILL) {
        if (logZ != -INFINITY) code = 8;
      }
      for (int k = tid; k < N; k += NT) {
        a.tok_post[cl.tok_off + k] = 0.f;
        a.start_mean[cl.tok_off + k] = 0.f;
        a.start_sd[cl.tok_off + k] = 0.f;
        if constexpr (OPT) a.keep_post[cl.tok_off + k] = 0.f;
        if constexpr (FILL) { a.end_mean[cl.tok_off + k] = 0.f; a.end_sd[cl.tok_off + k] = 0.f; }
      }
      if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = code; }
      return;
    }
  }

  // ---- sweeps 2 and 3, block by block from the end
  float bG[R], bX[R];                          // beta(G_k), beta(B_k) = beta(I_k)
  // with durations bX is beta(I_k) alone and beta(B_k) comes out of the slot's delay line (lattice.h chain_in): bB, of the frame in hand
  float bC[MIND ? R : 1][CHAIN_BACK], bB[MIND ? R : 1];
  int f0[R], cnt[R];
  double occ[R], m0[R], m1[R], m2[R];
  // FILL: what follows token k after the frame in hand (leave_k(t + 1), on beta_t's scale), carried from the iteration before --
  // across block boundaries too -- and the end moments' sums
  float lv[FILL ? R : 1];
  double e0[FILL ? R : 1], e1[FILL ? R : 1], e2[FILL ? R : 1];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    bG[r] = k == N ? 0.f : NEG;
    bX[r] = k == N - 1 ? 0.f : NEG;
    if constexpr (MIND || FILL) f0[r] = fst[r];
    else f0[r] = k < N ? first[k] : 0;
    if constexpr (FILL) {                       // at T - 1 only token N - 1 ends, into the clip's end
      lv[r] = k == N - 1 ? 0.f : NEG;
      e0[r] = e1[r] = e2[r] = 0.0;
    }
    if constexpr (OPT) {
      // where token N - 1 is optional the clip also ends in G_{N-1}, I_{N-2}, B_{N-2}, at -lam; a token tok does not hold has its
      // start moments about frame 0
      if (sk.opt(r + 1) && k == N - 1) bG[r] = -sk.lam;
      if (sk.opt(r + 2) && k == N - 2) bX[r] = -sk.lam;
      if (f0[r] == INT_MAX) f0[r] = 0;
    }
    cnt[r] = 0;
    occ[r] = m0[r] = m1[r] = m2[r] = 0.0;
  }
  if constexpr (MIND) {                         // no chain state ends the clip, and B_{N-1} only where D_{N-1} == 1
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < CHAIN_BACK; ++j) bC[r][j] = NEG;
  }
  if constexpr (OPT) beta_to_left_opt<NT, R>(me(), (float*)xb, T, bG, bX);
  else beta_to_left<NT, R, MIND>(me(), xb, T, bG, bX, bC, dm);
  double accb = 0.0;                           // what beta's renormalisations subtracted
  float subb = 0.f;
  for (int j = lay.nblk - 1; j >= 0; --j) {
    const int t_lo = j * POST_W, t_hi = min(T, t_lo + POST_W) - 1;
    forward(t_lo, t_hi + 1, true);
    int c = t_hi / F, tin = t_hi - c * F;
    stage_start(c, -1, load_stage, store_stage);
    float an[R][3], ac[R][3];
    auto load_alpha = [&](int f) {
      const float* o = blk + (long)f * K::S;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        an[r][0] = o[(r * 3 + 0) * NT + tid];
        an[r][1] = o[(r * 3 + 1) * NT + tid];
        an[r][2] = o[(r * 3 + 2) * NT + tid];
      }
    };
    load_alpha(t_hi - t_lo);
    for (int t = t_hi; t >= t_lo; --t, --tin) {
      if (tin < 0) {
        --c;
        tin = F - 1;
        stage_enter(c, -1, load_stage, store_stage);
      }
      const float* row = stage.row(c, tin);
      const float l = lring[(c & 1) * FMAX + tin];
      const int tk = tring[(c & 1) * FMAX + tin];
#pragma unroll
      for (int r = 0; r < R; ++r) { ac[r][0] = an[r][0]; ac[r][1] = an[r][1]; ac[r][2] = an[r][2]; }
      if (t > t_lo) load_alpha(t - 1 - t_lo);  // one frame ahead of its use
      // gamma_t of this thread's tokens
      const double cst = offa[t - t_lo] + accb - logZ;
      if constexpr (MIND) {
#pragma unroll
        for (int r = 0; r < R; ++r) bB[r] = chain_in(bX[r], bC[r], dm[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = tid * R + r;
        if (k < N) {
          float bb = bX[r];
          if constexpr (MIND) bb = bB[r];
          const float gb = __expf((float)((double)ac[r][1] + (double)bb + cst));
          const float gi = __expf((float)((double)ac[r][2] + (double)bX[r] + cst));
          const double d = (double)(t - f0[r]);
          m0[r] += (double)gb;
          m1[r] += (double)gb * d;
          m2[r] += (double)gb * d * d;
          if constexpr (FILL) {
            // omega_t(k): in B_k or I_k at t and out of the token at t + 1 (summed as two terms, no difference of gammas)
            const double dl = (double)lv[r] + cst;
            const float w = __expf((float)((double)ac[r][1] + dl)) + __expf((float)((double)ac[r][2] + dl));
            const double de = (double)(t - lst[r]);
            e0[r] += (double)w;
            e1[r] += (double)w * de;
            e2[r] += (double)w * de * de;
          }
          if constexpr (MIND) {
            // gamma_t(H_k^j) = gamma_{t-j+1}(B_k): a path in B_k at t is in the token's B / chain states at t .. t + max(D_k - 2, 0),
            // so gamma_t(B_k) counts once for every such frame inside Viterbi's run -- the block buffer needs no chain
            const int ov = min(t + max(dm[r] - 2, 0), lst[r]) - max(t, f0[r]) + 1;
            double add = (double)gb * (double)max(ov, 0);
            if (tk == k) { add += (double)gi; ++cnt[r]; }
            occ[r] += add;
          } else {
            if (tk == k) { occ[r] += (double)gb + (double)gi; ++cnt[r]; }
          }
        }
      }
      if (t == 0) break;
      // beta_{t-1}
      float eg, eb[R], ei[R], ebn;
      if constexpr (FILL) {
        beta_emissions<NT, R, WIN, false, true>(me(), row, l, g, av, avn, N, t, wn, wnn, eg, eb, ei, ebn, int4(), int2(), nullptr, fm, filler_emission(c, tin));
        beta_frame<NT, R, MIND, false, true>(me(), N, t, eg, eb, ei, ebn, xb, wmax, subb, accb, bG, bX, bB, bC, dm, 0.f, SkipArcs(), lv);
      } else if constexpr (OPT) {
        float ebn2;
        beta_emissions<NT, R, WIN, true>(me(), row, l, g, av, avn, N, t, wn, wnn, eg, eb, ei, ebn, avn2, wnn2, &ebn2);
        beta_frame<NT, R, MIND, true>(me(), N, t, eg, eb, ei, ebn, xb, wmax, subb, accb, bG, bX, bB, bC, dm, ebn2, sk);
      } else {
        beta_emissions<NT, R, WIN>(me(), row, l, g, av, avn, N, t, wn, wnn, eg, eb, ei, ebn);
        beta_frame<NT, R, MIND>(me(), N, t, eg, eb, ei, ebn, xb, wmax, subb, accb, bG, bX, bB, bC, dm);
      }
    }
  }

  // ---- per-token outputs, by the thread that owns the token
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    if (k < N) {
      const double mean = m0[r] > 0.0 ? m1[r] / m0[r] : 0.0;
      const double var = m0[r] > 0.0 ? m2[r] / m0[r] - mean * mean : 0.0;
      a.tok_post[cl.tok_off + k] = cnt[r] > 0 ? fminf((float)(occ[r] / (double)cnt[r]), 1.f) : 0.f;
      a.start_mean[cl.tok_off + k] = (float)mean;
      a.start_sd[cl.tok_off + k] = (float)sqrt(fmax(var, 0.0));
      if constexpr (OPT) a.keep_post[cl.tok_off + k] = fminf(fmaxf((float)m0[r], 0.f), 1.f);
      if constexpr (FILL) {
        const double em = e0[r] > 0.0 ? e1[r] / e0[r] : 0.0;
        const double ev = e0[r] > 0.0 ? e2[r] / e0[r] - em * em : 0.0;
        a.end_mean[cl.tok_off + k] = (float)em;
        a.end_sd[cl.tok_off + k] = (float)sqrt(fmax(ev, 0.0));
      }
    }
  }
  if (tid == 0) {
    a.logz[cl.clip] = (float)(logZ - lres);
    a.status[cl.clip] = 0;
  }
}

// over the cap the kernel reports status 2; such a clip is sized (and launched) as the cap's configuration, so the workspace need is
// monotone in N -- wfl_align instead gives it no workspace, its words being zero for every clip it does not search
int post_cfg(int N) { return std::min(cfg_of(N), NCFG - 1); }

long clip_floats(int T, int N) {
  if (T <= 0) return 0;
  const long S = dispatch_cfg(post_cfg(N), [](auto sh) { return PCfg<decltype(sh)::NT, decltype(sh)::R>::S; });
  return round64(PostLayout(T, S, S).total);  // (256-byte aligned)
}

// with fillers: wfl_align_posterior's floats and, behind them, the filler emission of every frame
long clip_floats_fill(int T, int N) {
  if (T <= 0) return 0;
  return clip_floats(T, N) + round64(T);
}

// with minimum durations: the checkpoints hold the chain as well, the block does not (post_kernel's note at occ)
long clip_floats_min(int T, int N) {
  if (T <= 0) return 0;
  return dispatch_cfg(post_cfg(N), [T](auto sh) {
    using K = PCfg<decltype(sh)::NT, decltype(sh)::R>;
    return round64(PostLayout(T, K::SM, K::S).total);
  });
}

}  // namespace

namespace {

// wfl_align_posterior (WIN false), wfl_align_posterior_windowed and wfl_align_min_duration_posterior (MIND, with or without windows): one
// host path
// and wfl_align_optional_posterior (OPT, with or without windows; tok_opt, skip_penalty and keep_post are its alone)
// and wfl_align_filler_posterior (FILL, with or without windows; tok_fill, filler_penalty, end_mean and end_sd are its alone)
template <bool WIN, bool MIND, bool OPT = false, bool FILL = false>
int posterior_batch(const char* fn, const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                    const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                    const int32_t* tok_win, const int32_t* tok_min, const int32_t* gap_cls, int32_t n_clips, const int32_t* tok,
                    void* workspace, int64_t workspace_bytes, float* logz, float* tok_post, float* start_mean, float* start_sd,
                    int32_t* status, void* stream, const int32_t* tok_opt = nullptr, float skip_penalty = 0.f, float* keep_post = nullptr,
                    const int32_t* tok_fill = nullptr, float filler_penalty = 0.f, float* end_mean = nullptr, float* end_sd = nullptr) {
  const int64_t need = FILL   ? wfl_align_filler_posterior_workspace_bytes(n_frames_host, n_tok_host, n_clips)
                       : OPT  ? wfl_align_optional_posterior_workspace_bytes(n_frames_host, n_tok_host, n_clips)
                       : MIND ? wfl_align_min_duration_posterior_workspace_bytes(n_frames_host, n_tok_host, n_clips)
                              : wfl_align_posterior_workspace_bytes(n_frames_host, n_tok_host, n_clips);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc || n_clips == 0) return rc;
  if (OPT && !(skip_penalty >= 0.f && skip_penalty <= 3.0e38f)) return fail(fn, -1, "skip_penalty must be a finite number >= 0");
  if (FILL && !(filler_penalty >= 0.f && filler_penalty <= 3.0e38f)) return fail(fn, -1, "filler_penalty must be a finite number >= 0");
  if (!logz || !status || !gap_cls ||
      (any_tok && (!tok_cls || (WIN && !tok_win) || (MIND && !tok_min) || (OPT && (!tok_opt || !keep_post)) ||
                   (FILL && (!tok_fill || !end_mean || !end_sd)) || !tok_post || !start_mean || !start_sd)) ||
      (any_frame && (!logits || !tok)))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::conditional_t<OPT, PostLaunchOpt, std::conditional_t<FILL, PostLaunchFill, PostLaunch>> a{};
  if constexpr (OPT) { a.tok_opt = tok_opt; a.keep_post = keep_post; a.lambda = skip_penalty; }
  if constexpr (FILL) { a.tok_fill = tok_fill; a.end_mean = end_mean; a.end_sd = end_sd; a.phi = filler_penalty; }
  a.logits = logits; a.ldl = ldl; a.C = C; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok = tok; a.tok_win = tok_win; a.tok_min = tok_min;
  a.ws = (float*)workspace; a.logz = logz; a.tok_post = tok_post; a.start_mean = start_mean; a.start_sd = start_sd; a.status = status;
  return launch_clips<NCFG>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_tok_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b};
        cfg = post_cfg(N);
        return FILL ? clip_floats_fill(T, N) : MIND ? clip_floats_min(T, N) : clip_floats(T, N);
      },
      [&](int cfg, const auto& a) {
        return dispatch_cfg(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          return launch_cfg<post_kernel<NT, R, WIN, MIND, OPT, FILL>, NT, PCfg<NT, R, OPT, FILL>::LDS>(fn, a, s);
        });
      });
}

}  // namespace
