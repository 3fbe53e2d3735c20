// Forward-backward over the explicit-duration lattice of wfl_align_duration_prior: per-token posteriors of a search under a duration
// prior (wfl_align_duration_prior_posterior, include/wfl_asr.h).  The sum-product twin of csrc/align_duration_prior.hip, and the first
// lattice here that is not first-order Markov: csrc/lattice_sums.h's alpha_frame / beta_frame cannot be instantiated for it, so the two
// sweeps below are this file's own.  What IS shared: csrc/lattice.h (configurations, setup and status, the logits stage ring, the
// emissions, the window mask, the renormalisation halves, the ragged batch) and, of csrc/lattice_sums.h, lae2, frame_lse and the stage
// walk.  A path weighs exp(sum_t e_t + sum_k L_k(d_k)); emissions from z_t - lse_t, L and tail the search's table rows.
//
// Forward (everything of frame t - 1 on the right; the search's recurrence, max -> log-sum-exp):
//   ent_k(t)  = lse(aG_k(t-1), aX_{k-1}(t-1))                     ent_0(0) = 0, every other ent_k(0) = -inf
//   aG_k(t)   = ent_k(t) + EG_t
//   aR_k^1(t) = ent_k(t) + EB_t(k);   aR_k^j(t) = aR_k^{j-1}(t-1) + EI_t(k)      2 <= j <= D
//   aY_k(t)   = lse(aY_k(t-1), aR_k^D(t-1) + L_k(D)) + EI_t(k) + tail_k
//   aX_k(t)   = lse(aR_k^1(t) + L_k(1), .., aR_k^D(t) + L_k(D), aY_k(t))         frame t is the LAST frame of token k
//   logZ      = lse(aG_N(T-1), aX_{N-1}(T-1))
// aX is max-then-sum: one pass shifts the ring and takes the maximum, a second sums D + 1 exponentials, one logarithm.
//
// Backward.  beta(G_k) and beta(X_{k-1}) have the same successors: bE_k(t).  W_k^j(t): the suffix weight when frame t is the j-th frame
// of a run of token k; V_k(t): the same inside the tail.
//   V_k(t)    = lse(bE_{k+1}(t), EI_{t+1}(k) + tail_k + V_k(t+1))
//   W_k^j(t)  = lse(L_k(j) + bE_{k+1}(t), EI_{t+1}(k) + W_k^{j+1}(t+1))   j < D;        W_k^D(t) = L_k(D) + V_k(t)
//   bE_k(t-1) = lse(bE_k(t) + EG_t, EB_t(k) + W_k^1(t))
// V and W of frame t need bE_{k+1} of the SAME frame, of the right thread's first slot for a thread's last slot.  So an iteration of the
// backward loop first makes V(t), W(t) from the bE(t) that the iteration before published (and from EI_{t+1}, kept in registers), then
// the gammas of frame t, then bE(t-1), which it publishes: one float through LDS and the frame's one barrier, shared with the
// renormalisation.  W^j(t) is made from W^{j+1}(t+1), so the ring entry (j - t) mod D stays in its word: the ring updates in place.
//
// Posteriors, accumulated in double by the thread that owns the token, straight from the gammas:
//   start_k(t) = exp(aR_k^1(t) + W_k^1(t) - logZ),      end_k(t) = exp(aX_k(t) + bE_{k+1}(t) - logZ)
//   occ_k(t)   = sum_{s <= t} start_k(s) - sum_{e < t} end_k(e);     tok_post the mean of occ over the search's run [first, last]:
//   sum_s start(s) #{t in run: t >= s} - sum_e end(e) #{t in run: t > e}, over the run's length.  No running sum crosses a block.
//
// Memory, as csrc/align_posterior.h: alpha is never stored per frame.  Sweep 1 runs forward and checkpoints its state every POST_W
// frames -- G, X, Y and the D ring entries of every slot; then, block by block from the last, the block's alpha is recomputed from its
// checkpoint into the block buffer -- aR^1 and aX alone, two floats per slot and frame: nothing else of alpha meets beta -- and beta
// walks down the block.  Both rings (alpha's aR^1 .. aR^D indexed by the run's start frame mod D, beta's W) are D floats per slot, entry
// (q, r) of thread i at word (q R + r) NT + i: a thread touches its own words only.  They live in LDS behind the kernel's other areas
// where they fit the CU's 160 KiB, alpha's first, and in the clip's workspace (L2-resident) where they do not: rings_in_lds().
// The table is read through the caches (at most 33 floats per row, every lane of a frame the same few rows).
//
// Every RENORM frames the block's maximum over G, X, Y and the ring (bE, V and the ring) is taken off all of them, alpha and beta
// separately, into a double: nothing is summed over the clip in fp32, a ring entry is at most D frames old.
//
// The counts side (wfl_align_duration_prior_counts; dpp_kernel's CNT = true): the same three sweeps without tok, and per token the
// posterior distribution of its run's length in the layout of a table row -- P(d = 1) .. P(d = D - 1), P(d >= D), E[max(d - D, 0)].
// The posterior that token k opens at t and lasts exactly d < D frames:
//   p_k(t, d) = exp(aR_k^1(t) + L_k(d) + Q_k^{t+d-1}(t) - logZ)
//   Q_k^e(t)  = EI_{t+1}(k) + .. + EI_e(k) + bE_{k+1}(e)   e = t .. t + D - 2;   Q_k^t(t) = bE_{k+1}(t),  Q_k^e(t-1) = EI_t(k) + Q_k^e(t)
// Q is beta's third ring, D - 1 floats per slot, entry e in word e mod (D - 1), updated in place (the entry of frame t takes the word
// of the one D - 1 frames later), renormalised with W and part of beta's maximum.  W^1(t) is the log-sum of L(d) + Q^{t+d-1}(t) over
// d < D joined with the D / tail term: p(t, d) <= start(t), and a start gamma of 0 skips the D - 1 exponentials.  The two tail
// statistics are sums of non-negative terms as well, no differences: P(d >= D) = sum_t exp(aR^D(t) + L(D) + V(t) - logZ), frame t the
// D-th frame of the run, and E[max(d - D, 0)] = sum_t exp(aY(t) + V(t) - logZ), frame t in the tail; so the block buffer holds
// (aR^1, aY, aR^D), three floats per slot and frame.  The D + 1 double sums of a slot live in the clip's workspace.  Up to three rings
// go to LDS, alpha's, W, Q in that order: count_rings_in_lds().  What is the posterior side's alone: tok, first[] / last[], the run
// validation, the seven moment sums; its instantiations are the code they were before the switch.
#include "lattice_sums.h"
#include "wfl_asr.h"

#include <limits.h>

namespace {

using namespace lattice;

constexpr int POST_W = 128;                 // frames per recomputed block
static_assert(POST_W % RENORM == 0, "a block ends on a renormalisation");
constexpr int MAX_D = 32;
constexpr int LDS_CAP = 160 * 1024;
constexpr double COUNT_SHIFT = 64 * 0.69314718055994530942;   // 64 ln 2: the scale of the counts side's gammas

struct DppLaunch {
  const float* logits;
  long ldl;
  int C;
  const int* tok_cls;  // [total tokens][4][2]
  const int* gap_cls;  // [n_clips][8]
  const int* tok_win;  // [total tokens][2], or null
  const int* tok_dur;  // [total tokens] row of `dur`, -1 none
  const float* dur;    // [n_rows][D + 1]
  int n_rows, D;
  const int* tok;      // the search's output (the counts side: null, never read)
  float* ws;           // LatClip::ws_off: the clip's workspace, in floats
  float* logz;
  float* tok_post;     // (the counts side: dur_post [total tokens][D + 1]; the four below unused)
  float* start_mean;
  float* start_sd;
  float* end_mean;
  float* end_sd;
  int* status;
  int n;
  LatClip clip[CLIPS_PER_LAUNCH];
};

template <int NT, int R>
struct CfgDpp : LdsBase<NT, R, 2 * NT * R * 4 + 4 * NT * 4> {   // its own between alt and wmax: first[], last[], the two exchanges
  static constexpr long SLOTS = (long)NT * R;
  static constexpr int OFF_FIRST = CfgDpp::OFF_X;                 // first frame of every token's run in tok
  static constexpr int OFF_LAST = OFF_FIRST + NT * R * 4;         // and its last
  static constexpr int OFF_XF = OFF_LAST + NT * R * 4;            // forward neighbour exchange: [2][NT] float
  static constexpr int OFF_XB = OFF_XF + 2 * NT * 4;              // backward neighbour exchange: [2][NT] float
  static constexpr int OFF_OFFA = CfgDpp::OFF_OWN;                // alpha's offsets of every frame of the block (double): [2][POST_W]
  static constexpr int OFF_LRING = OFF_OFFA + 2 * POST_W * 8;     // staged rows' log-sum-exp
  static constexpr int OFF_MISC = OFF_LRING + 2 * FMAX * 4;
  static constexpr int OFF_RING = OFF_MISC + 64;                  // the rings that fit
  static_assert(OFF_RING % 16 == 0 && OFF_RING <= LDS_CAP, "LDS");
  static constexpr long ring_words(int D) { return SLOTS * D; }
  static constexpr int rings_in_lds(int D) {
    const long n = (LDS_CAP - OFF_RING) / (ring_words(D) * 4);
    return n >= 2 ? 2 : (int)n;
  }
  static constexpr int MAX_RINGS = rings_in_lds(1), MIN_RINGS = rings_in_lds(32);   // what any D of 1 .. 32 can ask for
  static constexpr int lds_bytes(int D) { return OFF_RING + rings_in_lds(D) * (int)ring_words(D) * 4; }
  static constexpr long ckpt_floats(int D) { return SLOTS * (3 + D); }   // G, X, Y and the ring of every slot
  static constexpr long BLK = SLOTS * 2;                                 // aR^1 and aX of every slot, one frame
  // the seven double sums of every slot (occ, three start moments, three end moments) and the two ends of its run: in registers up
  // to four slots per thread; with eight or nine they would spill inside the frame loop, so those configurations keep them in the
  // clip's workspace, every thread its own words, touched only in the frames where a gamma of the slot is not 0 -- and their start
  // windows in LDS, in the words of first[] and last[] once tok has been judged
  static constexpr bool ACC_MEM = R >= 8;
  static constexpr long ACC = ACC_MEM ? SLOTS * (7 * 2 + 2) : 0;         // floats
  // ---- the counts side (wfl_align_duration_prior_counts): a third ring, beta's Q, D - 1 floats per slot, placed behind the other two
  static constexpr long qring_words(int D) { return SLOTS * (D - 1); }
  static constexpr int count_rings_in_lds(int D) {                       // alpha's, W, Q, in that order: how many of them fit
    const long room = (LDS_CAP - OFF_RING) / 4, rw = ring_words(D);
    return 2 * rw + qring_words(D) <= room ? 3 : 2 * rw <= room ? 2 : rw <= room ? 1 : 0;
  }
  static constexpr int COUNT_MAX_RINGS = count_rings_in_lds(1), COUNT_MIN_RINGS = count_rings_in_lds(32);
  static constexpr int count_lds_bytes(int D) {
    const int n = count_rings_in_lds(D);
    return OFF_RING + (int)((n >= 2 ? 2 : n) * ring_words(D) + (n >= 3 ? qring_words(D) : 0)) * 4;
  }
  static constexpr long COUNT_BLK = SLOTS * 3;                            // aR^1, aY and aR^D of every slot, one frame
  static constexpr long count_acc(int D) { return SLOTS * (D + 1) * 2; }  // a row of D + 1 double sums per slot, always in the workspace
};

// a clip's workspace in floats: [lse: round64(T)] [checkpoint offsets: round64(2 nblk)] [checkpoints: nblk SC] [block: POST_W BLK]
// [the sums where they are not in registers: ACC] [alpha's ring: round64(RW) unless in LDS] [beta's ring: the same]
// [the counts side's Q ring: round64(RQ) unless in LDS; RQ = 0 on the posterior side]
struct DppLayout {
  long ckacc, ckpt, blk, sums, ringf, ringb, ringq, total;
  int nblk;
  __host__ __device__ DppLayout(int T, long SC, long BLK, long ACC, long RW, int in_lds, long RQ = 0) {
    nblk = (T + POST_W - 1) / POST_W;
    ckacc = round64(T);
    ckpt = ckacc + round64(2L * nblk);
    blk = ckpt + (long)nblk * SC;
    sums = blk + (long)POST_W * BLK;
    ringf = sums + ACC;
    ringb = ringf + (in_lds >= 1 ? 0 : round64(RW));
    ringq = ringb + (in_lds >= 2 ? 0 : round64(RW));
    total = ringq + (in_lds >= 3 ? 0 : round64(RQ));
  }
};

// HL: how many of the rings are in LDS (0 | 1: alpha's | 2: beta's W as well | 3, the counts side alone: its Q too)
// CNT: false the posteriors of wfl_align_duration_prior_posterior (tok, first / last, the run validation, the seven moment sums);
// true the expected length counts of wfl_align_duration_prior_counts (no tok; the Q ring and a histogram row per slot), which writes
// its dur_post through the launch's tok_post pointer
template <int NT, int R, int HL, bool CNT>
__global__ __launch_bounds__(NT) void dpp_kernel(DppLaunch a) {
  using K = CfgDpp<NT, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  int* first = (int*)(lds + K::OFF_FIRST);
  int* last = (int*)(lds + K::OFF_LAST);
  float* xf = (float*)(lds + K::OFF_XF);
  float* xb = (float*)(lds + K::OFF_XB);
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  double* offa = (double*)(lds + K::OFF_OFFA);
  float* lring = (float*)(lds + K::OFF_LRING);
  int* misc = (int*)(lds + K::OFF_MISC);
  float* fin = (float*)(misc + 4);

  const LatClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = cl.T, N = cl.N, C = a.C, D = a.D, D1 = a.D + 1;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  const int* tokp = a.tok + cl.frame_off;      // (CNT: never read)
  const float NEG = -INFINITY;

  auto zeros = [&](int code) {
    if constexpr (CNT) {
      for (long w = tid; w < (long)N * D1; w += NT) a.tok_post[(long)cl.tok_off * D1 + w] = 0.f;
    } else for (int k = tid; k < N; k += NT) {
      a.tok_post[cl.tok_off + k] = 0.f;
      a.start_mean[cl.tok_off + k] = 0.f;
      a.start_sd[cl.tok_off + k] = 0.f;
      a.end_mean[cl.tok_off + k] = 0.f;
      a.end_sd[cl.tok_off + k] = 0.f;
    }
    if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = code; }
  };

  int g[NGAP];
  int st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
  int row[R];                                   // this thread's slots' table rows (-1: no prior; slots past the tokens too)
#pragma unroll
  for (int r = 0; r < R; ++r) row[r] = -1;
  if (st == 0) {                                // (the same in every thread).  A row outside -1 .. n_rows - 1: status 4
    if (tid == 0) misc[3] = 0;
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = tid * R + r;
      if (k < N) row[r] = a.tok_dur[cl.tok_off + k];
      if (row[r] < -1 || row[r] >= a.n_rows) bad = true;
    }
    if (bad) misc[3] = 1;
    __syncthreads();
    if (misc[3]) st = 4;
  }
  if (st != 0 || T == 0) {
    zeros(st);
    return;
  }

  // entry j (0 .. D) of the row at word `lb`; `has` false: 0, and nothing is loaded (a table may have no row at all)
  // (an unsigned 32-bit offset from the table's uniform base -- the host refuses a table of 2^31 values or more -- so that no slot
  // keeps a 64-bit address of its row in registers; the rings' words below the same)
  auto Ld = [&](int lb, bool has, int j) -> float { return has ? a.dur[(unsigned)(lb + j)] : 0.f; };

  constexpr bool AM = K::ACC_MEM;
  int2 wn[R];                                   // the start windows; a null tok_win: open
#pragma unroll
  for (int r = 0; r < R; ++r) wn[r] = make_int2(0, WIN_OPEN_HI);
  if (a.tok_win) load_windows<R>(a.tok_win, cl.tok_off, N, wn);

  // ---- the run of every token in tok; a tok that is no path of this lattice is reported after sweep 1 (status 1 comes first)
  int fst[R], lst[R];
  bool notpath;
  const long SC = K::ckpt_floats(D);
  const DppLayout lay = CNT ? DppLayout(T, SC, K::COUNT_BLK, K::count_acc(D), K::ring_words(D), HL, K::qring_words(D))
                            : DppLayout(T, SC, K::BLK, K::ACC, K::ring_words(D), HL);
  constexpr int BW = CNT ? 3 : 2;               // floats per slot and frame of the block buffer
  float* ws = a.ws + cl.ws_off;
  // (what a thread keeps for itself in the workspace lies together, thread by thread: one base address and immediate offsets, where
  // an interleaved layout makes the compiler keep an address per slot in registers)
  double* gsum = (double*)(ws + lay.sums) + tid * (7 * R);             // ACC_MEM: sum i of slot r at gsum[7 r + i]
  int* gends = (int*)(ws + lay.sums + K::SLOTS * 14) + tid * (2 * R);  // and its (first, last) at gends[2 r], gends[2 r + 1]
  double* hsum = (double*)(ws + lay.sums) + tid * (R * D1);            // CNT: entry j of slot r's row at hsum[r D1 + j]
  if constexpr (CNT) {                          // no tok to judge: the windows go to their LDS words at once (a thread's own words)
    if constexpr (AM) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        first[r * NT + tid] = wn[r].x;
        last[r * NT + tid] = wn[r].y;
      }
    }
    notpath = false;
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) { first[tid * R + r] = INT_MAX; last[tid * R + r] = -1; }
    __syncthreads();                            // (and every thread has read misc[3] before misc[0] is raised)
    bool bad = false;
    for (int t = tid; t < T; t += NT) {
      const int k = tokp[t];
      if (k < -1 || k >= N) { bad = true; continue; }
      if (k < 0) continue;
      if (t == 0 || tokp[t - 1] != k) atomicMin(&first[k], t);
      if (t == T - 1 || tokp[t + 1] != k) atomicMax(&last[k], t);
    }
    if (bad) misc[0] = 1;
    __syncthreads();
    bad = false;
    for (int t = tid; t < T; t += NT) {         // a token with two runs
      const int k = tokp[t];
      if (k >= 0 && k < N && (t == 0 || tokp[t - 1] != k) && first[k] != t) bad = true;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = tid * R + r;
      fst[r] = lst[r] = 0;
      if (k < N) {
        const int f = first[k], l = last[k];
        fst[r] = f;
        lst[r] = l;
        if (f == INT_MAX) { bad = true; continue; }                       // a token missing
        if (k + 1 < N && first[k + 1] <= l) bad = true;                   // out of order
        if (f < wn[r].x || f > wn[r].y) bad = true;                       // opens outside its window
        const bool has = row[r] >= 0;
        const int lb = max(row[r], 0) * D1;
        const int d = l - f + 1;
        if (d <= D ? Ld(lb, has, d - 1) == NEG : (Ld(lb, has, D - 1) == NEG || Ld(lb, has, D) == NEG)) bad = true;   // a forbidden length
      }
    }
    if (bad) misc[0] = 1;
    __syncthreads();
    notpath = misc[0] != 0;
    if constexpr (AM) {                         // (every thread is past its reads of first[] and last[])
#pragma unroll
      for (int r = 0; r < R; ++r) {
        gends[2 * r] = fst[r];
        gends[2 * r + 1] = lst[r];
        first[r * NT + tid] = wn[r].x;
        last[r * NT + tid] = wn[r].y;
      }
    }
  }
  auto window = [&](int r) -> int2 {
    if constexpr (AM) return make_int2(first[r * NT + tid], last[r * NT + tid]);
    else return wn[r];
  };

  const int nblk = (T + POST_W - 1) / POST_W;
  float* lse = ws;
  double* ckacc = (double*)(ws + lay.ckacc);
  float* ckpt = ws + lay.ckpt;
  float* blk = ws + lay.blk;
  float* lrings = (float*)(lds + K::OFF_RING);
  // a ring's entry (q, r): in LDS word (q R + r) NT + tid (a wave's lanes on consecutive banks), in the workspace word (tid D + q) R + r
  float* fring = HL >= 1 ? lrings : ws + lay.ringf;                                   // alpha's ring
  float* bring = HL >= 2 ? lrings + K::ring_words(D) : ws + lay.ringb;                // beta's
  auto fi = [&](int q, int r) -> unsigned {
    if constexpr (HL >= 1) return (q * R + r) * NT + tid;
    else return (tid * D + q) * R + r;
  };
  auto bi = [&](int q, int r) -> unsigned {
    if constexpr (HL >= 2) return (q * R + r) * NT + tid;
    else return (tid * D + q) * R + r;
  };
  // CNT: beta's Q ring, DQ = D - 1 words per slot, entry e (the run's last frame) in word e mod DQ
  const int DQ = D - 1;
  float* qring = HL >= 3 ? lrings + 2 * K::ring_words(D) : ws + lay.ringq;
  auto qi = [&](int q, int r) -> unsigned {
    if constexpr (HL >= 3) return (q * R + r) * NT + tid;
    else return (tid * DQ + q) * R + r;
  };
  auto each_q = [&](auto&& f) {
    for (int q = 0; q < DQ; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) f(qi(q, r));
  };
  // f(word) over every entry of this thread's part of a ring
  auto each_f = [&](auto&& f) {
    for (int q = 0; q < D; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) f(fi(q, r), q, r);
  };
  auto each_b = [&](auto&& f) {
    for (int q = 0; q < D; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) f(bi(q, r), q, r);
  };

  // (summed now and parked in LDS until the clip's last line: left to the compiler, the per-wave terms wait in registers, or in
  // scratch, across all three sweeps)
  double* lres = (double*)(misc + 8);
  {
    const double v = frame_lse<NT>(tid, Z, a.ldl, T, C, lse, red);
    if (tid == 0) *lres = v;
  }

  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;
  float pre_l = 0.f;
  int pre_t = -1;
  auto load_stage = [&](int c) { stage_load<false>(tid, stage, c, lse, nullptr, pre_l, pre_t); };
  auto store_stage = [&](int c) { stage_store<false>(tid, stage, c, lring, nullptr, pre_l, pre_t); };

  constexpr bool AVR = NT < 512;                // (512 x 9: the alternatives stay in LDS)
  int4 av[AVR ? R : 1];
  if constexpr (AVR) {
#pragma unroll
    for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  }
  auto emissions = [&](const float* rowz, float l, int r, int k, int t, float& eb, float& ei) {
    if constexpr (AVR) tok_emission(rowz, av[r], eb, ei);
    else tok_emission(rowz, alt[k], eb, ei);
    eb -= l;
    ei -= l;
    eb = win_mask(eb, t, window(r));
  };

  // ---- the forward sweep over frames t0 .. t1 - 1, from the clip's start (t0 = 0) or from checkpoint t0 / POST_W
  float G[R], X[R], Y[R];
  double acc = 0.0;                             // what alpha's renormalisations subtracted
  auto forward = [&](int t0, int t1, bool keep) {
    if (t0 == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) G[r] = X[r] = Y[r] = NEG;
      if (tid == 0) G[0] = 0.f;                 // a virtual frame -1 in G_0: ent_0(0) = 0
      each_f([&](unsigned w, int, int) { fring[w] = NEG; });
      acc = 0.0;
    } else {
      const float* ck = ckpt + (long)(t0 / POST_W) * SC;        // [thread][slot](G, X, Y), then [thread][q][slot] the ring
      const float* cs = ck + tid * (3 * R);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        G[r] = cs[r * 3 + 0];
        X[r] = cs[r * 3 + 1];
        Y[r] = cs[r * 3 + 2];
      }
      const float* cr = ck + 3 * K::SLOTS + tid * D * R;
      each_f([&](unsigned w, int q, int r) { fring[w] = cr[q * R + r]; });
      acc = ckacc[t0 / POST_W];
    }
    xf[((t0 + 1) & 1) * NT + tid] = X[R - 1];
    float sub = 0.f;
    int c = t0 / F, tin = t0 - c * F;
    int p = t0 % D;                             // t mod D
    stage_start(c, 1, load_stage, store_stage);
    for (int t = t0; t < t1; ++t, ++tin) {
      if (tin == F) {
        ++c;
        tin = 0;
        stage_enter(c, 1, load_stage, store_stage);
      }
      const float* rowz = stage.row(c, tin);
      const float l = lring[(c & 1) * FMAX + tin];
      const float eg = gap_emission(rowz, g) - l;
      const float nb = (tid > 0 ? xf[((t + 1) & 1) * NT + tid - 1] : NEG) - sub;
      // aR^1 goes to the block buffer as it is made, on the scale of BEFORE this frame's renormalisation (offa[0][]), aX after it, on
      // the scale of after (offa[1][]): no aR^1 stays in a register across the slots
      float* o = blk + (long)(t - t0) * (K::SLOTS * BW) + tid * (BW * R);   // [thread][slot](aR^1, aX), CNT: (aR^1, aY, aR^D)
      if (keep && tid == 0) offa[t - t0] = acc;
#pragma unroll
      for (int r = R - 1; r >= 0; --r) {        // descending: slot r - 1's previous-frame X is still in place
        const int k = tid * R + r;
        const float pX = r ? X[r > 0 ? r - 1 : 0] : nb;
        const float ent = lae2(G[r], pX);
        G[r] = k <= N ? ent + eg : NEG;
        if (k < N) {
          float eb, ei;
          emissions(rowz, l, r, k, t, eb, ei);
          const bool has = row[r] >= 0;
          const int lb = max(row[r], 0) * D1;
          // Y: stay, or enter from the run that is D frames old (the ring entry this frame's opening replaces)
          const float old = fring[fi(p, r)];
          Y[r] = (lae2(Y[r], old + Ld(lb, has, D - 1)) + ei) + Ld(lb, has, D);
          const float r1 = ent + eb;
          fring[fi(p, r)] = r1;
          if (keep) o[r * BW + 0] = r1;
          // pass 1: the runs that began at t - j + 1 gain EI_t; the maximum of the D + 1 candidates
          float m = fmaxf(r1 + Ld(lb, has, 0), Y[r]);
          for (int j = 2; j <= D; ++j) {
            int q = p - (j - 1);
            q = q < 0 ? q + D : q;
            const float v = fring[fi(q, r)] + ei;
            fring[fi(q, r)] = v;
            m = fmaxf(m, v + Ld(lb, has, j - 1));
          }
          // pass 2: D + 1 exponentials, one logarithm (-inf only ever adds: ms is finite)
          const float ms = m == NEG ? 0.f : m;
          float s = __expf(Y[r] - ms);
#pragma unroll 2
          for (int j = 1; j <= D; ++j) {
            int q = p - (j - 1);
            q = q < 0 ? q + D : q;
            s += __expf((fring[fi(q, r)] + Ld(lb, has, j - 1)) - ms);
          }
          X[r] = ms + __logf(s);
        }
      }
      p = p + 1 == D ? 0 : p + 1;
      xf[(t & 1) * NT + tid] = X[R - 1];
      const bool renorm = (t & (RENORM - 1)) == RENORM - 1;
      if (renorm) {
        float lm = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(G[r], fmaxf(X[r], Y[r])));
        each_f([&](unsigned w, int, int) { lm = fmaxf(lm, fring[w]); });
        renorm_publish(lm, wmax);
      }
      __syncthreads();                          // the neighbour exchange and the renormalisation share it
      sub = 0.f;
      if (renorm) {
        float M = renorm_max<K::NW>(wmax);
        if (!(M > NEG)) M = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) { G[r] -= M; X[r] -= M; Y[r] -= M; }
        each_f([&](unsigned w, int, int) { fring[w] -= M; });
        sub = M;
        acc += (double)M;
      }
      if (keep) {                               // what of the block's alpha meets beta, for the backward sweep of the same thread
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if constexpr (CNT) {                  // (p is (t + 1) mod D by now: the word of the run that is D frames old, aR^D(t))
            o[r * BW + 1] = Y[r];
            o[r * BW + 2] = fring[fi(p, r)];
          } else {
            o[r * BW + 1] = X[r];
          }
        }
        if (tid == 0) offa[POST_W + t - t0] = acc;
      } else if ((t + 1) % POST_W == 0 && t + 1 < T) {   // (a block ends on a renormalisation: sub is spent)
        float* o = ckpt + (long)((t + 1) / POST_W) * SC;
        float* os = o + tid * (3 * R);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          os[r * 3 + 0] = G[r];
          os[r * 3 + 1] = X[r];
          os[r * 3 + 2] = Y[r];
        }
        float* orr = o + 3 * K::SLOTS + tid * D * R;
        each_f([&](unsigned w, int q, int r) { orr[q * R + r] = fring[w]; });
        if (tid == 0) ckacc[(t + 1) / POST_W] = acc;
      }
    }
  };

  // ---- sweep 1: alpha over the whole clip, checkpoints, logZ
  forward(0, T, false);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    if (k == N) fin[0] = G[r];
    if (k == N - 1) fin[1] = X[r];
  }
  __syncthreads();
  if (tid == 0) {
    const double e0 = (double)fin[0], e1 = N >= 1 ? (double)fin[1] : -INFINITY;
    const double m = fmax(e0, e1);
    red[0] = m == -INFINITY ? -INFINITY : m + log(exp(e0 - m) + exp(e1 - m)) + acc;
  }
  __syncthreads();                              // (ckacc[] of thread 0 is visible to the block as well)
  const double logZ = red[0];                   // on the fp32 log-sum-exps; the clip's logZ is logZ - lres
  if (logZ == -INFINITY || notpath) {           // no path at all: 1; paths, and tok is none of them: 8
    zeros(logZ == -INFINITY ? 1 : 8);
    return;
  }

  // ---- sweeps 2 and 3, block by block from the end
  float bE[R], V[R], eip[R];                    // bE_k, V_k; EI of the frame behind the one in hand
  double sums[AM ? 1 : R][7];                   // occ, m0, m1, m2, e0, e1, e2 of every slot (ACC_MEM: in the workspace, gsum[(r * 7 + i) NT])
#pragma unroll
  for (int r = 0; r < R; ++r) {
    bE[r] = tid * R + r == N ? 0.f : NEG;
    V[r] = NEG;
    eip[r] = 0.f;
    if constexpr (CNT) {
      for (int j = 0; j < D1; ++j) hsum[r * D1 + j] = 0.0;
    } else {
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        if constexpr (AM) gsum[r * 7 + i] = 0.0;
        else sums[r][i] = 0.0;
      }
    }
  }
  each_b([&](unsigned w, int, int) { bring[w] = NEG; });
  if constexpr (CNT) each_q([&](unsigned w) { qring[w] = NEG; });
  int pq = DQ > 0 ? (T - 1) % DQ : 0;           // CNT: t mod DQ, the word of Q^t(t)
  xb[(T & 1) * NT + tid] = bE[0];
  double accb = 0.0;                            // what beta's renormalisations subtracted
  float subb = 0.f;
  int pb = (D - (T - 1) % D) % D;               // (-t) mod D: the word of W^D(t); W^j(t) sits in word (pb + j) mod D
  for (int j = nblk - 1; j >= 0; --j) {
    const int t_lo = j * POST_W, t_hi = min(T, t_lo + POST_W) - 1;
    forward(t_lo, t_hi + 1, true);
    int c = t_hi / F, tin = t_hi - c * F;
    stage_start(c, -1, load_stage, store_stage);
    for (int t = t_hi; t >= t_lo; --t, --tin) {
      if (tin < 0) {
        --c;
        tin = F - 1;
        stage_enter(c, -1, load_stage, store_stage);
      }
      const float nbE = (tid + 1 < NT ? xb[((t + 1) & 1) * NT + tid + 1] : NEG) - subb;     // bE(t) of the next thread's first slot
      const double cst1 = offa[t - t_lo] + accb - logZ, cst = offa[POST_W + t - t_lo] + accb - logZ;     // for aR^1, for aX
      const float* ab = blk + (long)(t - t_lo) * (K::SLOTS * BW) + tid * (BW * R);
      float W1[R];
      const int q1 = pb + 1 >= D ? pb + 1 - D : pb + 1;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = tid * R + r;
        W1[r] = NEG;
        if (k < N) {
          const float nE = r + 1 < R ? bE[r + 1 < R ? r + 1 : 0] : nbE;
          const bool has = row[r] >= 0;
          const int lb = max(row[r], 0) * D1;
          const float ep = eip[r];
          // V(t), W(t) from bE_{k+1}(t) and V(t+1), W(t+1); at T - 1 the latter are -inf and ep is 0
          V[r] = lae2(nE, (ep + Ld(lb, has, D)) + V[r]);
          for (int jj = 1; jj < D; ++jj) {
            int q = pb + jj;
            q = q >= D ? q - D : q;
            bring[bi(q, r)] = lae2(Ld(lb, has, jj - 1) + nE, ep + bring[bi(q, r)]);
          }
          bring[bi(pb, r)] = Ld(lb, has, D - 1) + V[r];
          W1[r] = bring[bi(q1, r)];
          // the gammas of frame t
          if constexpr (CNT) {
            // Q(t) from bE_{k+1}(t) and Q(t+1): the run that ends on t takes the word of the one that ended on t + D - 1
            for (int q = 0; q < DQ; ++q)
              if (q != pq) qring[qi(q, r)] = ep + qring[qi(q, r)];
            if (DQ > 0) qring[qi(pq, r)] = nE;
            double* h = hsum + r * D1;
            // The counts' gammas are formed 2^64 times their size and the row is scaled back in double at the end: an fp32
            // exponential is 0 below 2^-126 (or a denormal of a few bits), and a length that takes 1e-40 of the mass in each of a
            // thousand frames is still an output fp32 can write; on this scale a term counts down to 2^-190.  (A posterior is at
            // most 1: 2^64 times it is far inside fp32.)
            const double c1 = cst1 + COUNT_SHIFT, c2 = cst + COUNT_SHIFT;
            // a run of exactly d < D frames from t: p(t, d) <= start(t), so a start gamma of 0 has nothing to add
            if (__expf((float)((double)ab[r * BW + 0] + (double)W1[r] + c1)) != 0.f) {
              int q = pq;
              for (int d = 1; d < D; ++d) {
                const float pd = __expf((float)((double)ab[r * BW + 0] + (double)(Ld(lb, has, d - 1) + qring[qi(q, r)]) + c1));
                if (pd != 0.f) h[d - 1] += (double)pd;
                q = q + 1 == DQ ? 0 : q + 1;
              }
            }
            // frame t as the D-th frame of a run (every run of D frames or more has exactly one), and as a frame of the tail
            const float gd = __expf((float)((double)ab[r * BW + 2] + (double)(Ld(lb, has, D - 1) + V[r]) + c2));
            const float gy = __expf((float)((double)ab[r * BW + 1] + (double)V[r] + c2));
            if (gd != 0.f) h[D - 1] += (double)gd;
            if (gy != 0.f) h[D] += (double)gy;
            continue;
          }
          const float gs = __expf((float)((double)ab[r * 2 + 0] + (double)W1[r] + cst1));
          const float ge = __expf((float)((double)ab[r * 2 + 1] + (double)nE + cst));
          // occ summed over the run [f, l]: a start at s counts for the run's frames >= s, an end at e against those > e
          auto add = [&](int f, int l, auto&& to) {
            const double ds = (double)(t - f), de = (double)(t - l);
            const int ns = max(l - max(t, f) + 1, 0);
            const int ne = max(l - max(t + 1, f) + 1, 0);
            to(0, (double)gs * (double)ns - (double)ge * (double)ne);
            to(1, (double)gs);
            to(2, (double)gs * ds);
            to(3, (double)gs * ds * ds);
            to(4, (double)ge);
            to(5, (double)ge * de);
            to(6, (double)ge * de * de);
          };
          if constexpr (AM) {
            if (gs != 0.f || ge != 0.f)
              add(gends[2 * r], gends[2 * r + 1], [&](int i, double v) { gsum[r * 7 + i] += v; });
          } else {
            add(fst[r], lst[r], [&](int i, double v) { sums[r][i] += v; });
          }
        }
      }
      pb = pb + 1 == D ? 0 : pb + 1;            // (-(t - 1)) mod D
      pq = pq == 0 ? max(DQ - 1, 0) : pq - 1;   // (t - 1) mod DQ
      if (t == 0) break;
      // bE(t - 1)
      const float* rowz = stage.row(c, tin);
      const float l = lring[(c & 1) * FMAX + tin];
      const float eg = gap_emission(rowz, g) - l;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = tid * R + r;
        float eb = NEG, ei = NEG;
        if (k < N) emissions(rowz, l, r, k, t, eb, ei);
        eip[r] = ei;
        bE[r] = k <= N ? lae2(bE[r] + eg, eb + W1[r]) : NEG;
      }
      xb[(t & 1) * NT + tid] = bE[0];
      const bool renorm = (t & (RENORM - 1)) == 0;
      if (renorm) {
        float lm = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(bE[r], V[r]));
        each_b([&](unsigned w, int, int) { lm = fmaxf(lm, bring[w]); });
        if constexpr (CNT) each_q([&](unsigned w) { lm = fmaxf(lm, qring[w]); });
        renorm_publish(lm, wmax);
      }
      __syncthreads();
      subb = 0.f;
      if (renorm) {
        float M = renorm_max<K::NW>(wmax);
        if (!(M > NEG)) M = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) { bE[r] -= M; V[r] -= M; }
        each_b([&](unsigned w, int, int) { bring[w] -= M; });
        if constexpr (CNT) each_q([&](unsigned w) { qring[w] -= M; });
        subb = M;
        accb += (double)M;
      }
    }
  }

  // ---- per-token outputs, by the thread that owns the token
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    if constexpr (CNT) {
      if (k < N)
        for (int j = 0; j < D1; ++j) a.tok_post[(long)(cl.tok_off + k) * D1 + j] = (float)ldexp(hsum[r * D1 + j], -64);
      continue;
    }
    if (k < N) {
      double sm[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        if constexpr (AM) sm[i] = gsum[r * 7 + i];
        else sm[i] = sums[r][i];
      }
      const double mean = sm[1] > 0.0 ? sm[2] / sm[1] : 0.0;
      const double var = sm[1] > 0.0 ? sm[3] / sm[1] - mean * mean : 0.0;
      const double em = sm[4] > 0.0 ? sm[5] / sm[4] : 0.0;
      const double ev = sm[4] > 0.0 ? sm[6] / sm[4] - em * em : 0.0;
      int f = fst[r], l = lst[r];
      if constexpr (AM) { f = gends[2 * r]; l = gends[2 * r + 1]; }
      const double po = sm[0] / (double)(l - f + 1);
      a.tok_post[cl.tok_off + k] = fminf(fmaxf((float)po, 0.f), 1.f);
      a.start_mean[cl.tok_off + k] = (float)mean;
      a.start_sd[cl.tok_off + k] = (float)sqrt(fmax(var, 0.0));
      a.end_mean[cl.tok_off + k] = (float)em;
      a.end_sd[cl.tok_off + k] = (float)sqrt(fmax(ev, 0.0));
    }
  }
  if (tid == 0) {
    a.logz[cl.clip] = (float)(logZ - *lres);
    a.status[cl.clip] = 0;
  }
}

// over the cap the kernel reports status 2; such a clip is sized (and launched) as the cap's configuration (csrc/align_posterior.h)
int dpp_cfg(int N) { return std::min(cfg_of(N), NCFG - 1); }

long clip_floats(int T, int N, int D, bool counts = false) {
  if (T <= 0) return 0;
  return dispatch_cfg(dpp_cfg(N), [&](auto sh) {
    using K = CfgDpp<decltype(sh)::NT, decltype(sh)::R>;
    if (counts)
      return round64(DppLayout(T, K::ckpt_floats(D), K::COUNT_BLK, K::count_acc(D), K::ring_words(D), K::count_rings_in_lds(D),
                               K::qring_words(D)).total);
    return round64(DppLayout(T, K::ckpt_floats(D), K::BLK, K::ACC, K::ring_words(D), K::rings_in_lds(D)).total);
  });
}

// the launches of both entries: the clips by configuration, each with the ring placement its D reaches
template <bool CNT>
int launch_all(const char* fn, DppLaunch& a, int n_clips, const int64_t* frame_off_host, const int32_t* n_frames_host,
               const int32_t* tok_off_host, const int32_t* n_tok_host, int D, hipStream_t s) {
  return launch_clips<NCFG>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_tok_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b};
        cfg = dpp_cfg(N);
        return clip_floats(T, N, D, CNT);
      },
      [&](int cfg, DppLaunch& a) {
        return dispatch_cfg(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          using K = CfgDpp<NT, R>;
          constexpr int HI = CNT ? K::COUNT_MAX_RINGS : K::MAX_RINGS, LO = CNT ? K::COUNT_MIN_RINGS : K::MIN_RINGS;
          auto launch = [&](auto hl_tag) {
            constexpr int HL = decltype(hl_tag)::value;
            if constexpr (HL <= HI && HL >= LO) {                          // (only the placements some D reaches are instantiated)
              if (const int rc = reserve_lds<dpp_kernel<NT, R, HL, CNT>, LDS_CAP>(fn)) return rc;     // (the most any D asks for)
              hipLaunchKernelGGL((dpp_kernel<NT, R, HL, CNT>), dim3(a.n), dim3(NT), CNT ? K::count_lds_bytes(D) : K::lds_bytes(D), s, a);
              return hipGetLastError() == hipSuccess ? 0 : fail(fn, -3, "launch failed");
            } else {
              return fail(fn, -3, "no such ring placement");
            }
          };
          const int hl = CNT ? K::count_rings_in_lds(D) : K::rings_in_lds(D);
          if (hl == 3) return launch(std::integral_constant<int, 3>());
          if (hl == 2) return launch(std::integral_constant<int, 2>());
          if (hl == 1) return launch(std::integral_constant<int, 1>());
          return launch(std::integral_constant<int, 0>());
        });
      });
}

}  // namespace

extern "C" {

int64_t wfl_align_duration_prior_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips,
                                                           int32_t D) {
  if (D < 1 || D > MAX_D) return -1;
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, [D](int T, int N) { return clip_floats(T, N, D); });
}

int32_t wfl_align_duration_prior_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                           const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                           const int32_t* tok_dur, const float* dur, int32_t n_rows, int32_t D, const int32_t* tok,
                                           void* workspace, int64_t workspace_bytes, float* logz, float* tok_post, float* start_mean,
                                           float* start_sd, float* end_mean, float* end_sd, int32_t* status, void* stream) {
  const char* fn = "wfl_align_duration_prior_posterior";
  if (D < 1 || D > MAX_D) return fail(fn, -1, "D must be 1 .. 32");
  if (n_rows < 0) return fail(fn, -1, "n_rows < 0");
  const int64_t need = wfl_align_duration_prior_posterior_workspace_bytes(n_frames_host, n_tok_host, n_clips, D);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc) return rc;
  if (n_rows > 0 && !dur) return fail(fn, -1, "null dur with n_rows > 0");
  if ((int64_t)n_rows * (D + 1) > INT_MAX) return fail(fn, -1, "a table of 2^31 values or more");
  if (n_clips == 0) return 0;
  if (any_tok && !tok_dur) return fail(fn, -1, "null tok_dur");
  if (!logz || !status || !gap_cls ||
      (any_tok && (!tok_cls || !tok_post || !start_mean || !start_sd || !end_mean || !end_sd)) || (any_frame && (!logits || !tok)))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  DppLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok_win = tok_win;
  a.tok_dur = tok_dur; a.dur = dur; a.n_rows = n_rows; a.D = D; a.tok = tok;
  a.ws = (float*)workspace; a.logz = logz; a.tok_post = tok_post; a.start_mean = start_mean; a.start_sd = start_sd;
  a.end_mean = end_mean; a.end_sd = end_sd; a.status = status;
  return launch_all<false>(fn, a, n_clips, frame_off_host, n_frames_host, tok_off_host, n_tok_host, D, (hipStream_t)stream);
}

int64_t wfl_align_duration_prior_counts_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips,
                                                        int32_t D) {
  if (D < 1 || D > MAX_D) return -1;
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, [D](int T, int N) { return clip_floats(T, N, D, true); });
}

int32_t wfl_align_duration_prior_counts(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                        const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                        const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                        const int32_t* tok_dur, const float* dur, int32_t n_rows, int32_t D, void* workspace,
                                        int64_t workspace_bytes, float* logz, float* dur_post, int32_t* status, void* stream) {
  const char* fn = "wfl_align_duration_prior_counts";
  if (D < 1 || D > MAX_D) return fail(fn, -1, "D must be 1 .. 32");
  if (n_rows < 0) return fail(fn, -1, "n_rows < 0");
  const int64_t need = wfl_align_duration_prior_counts_workspace_bytes(n_frames_host, n_tok_host, n_clips, D);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc) return rc;
  if (n_rows > 0 && !dur) return fail(fn, -1, "null dur with n_rows > 0");
  if ((int64_t)n_rows * (D + 1) > INT_MAX) return fail(fn, -1, "a table of 2^31 values or more");
  if (n_clips == 0) return 0;
  if (any_tok && !tok_dur) return fail(fn, -1, "null tok_dur");
  if (!logz || !status || !gap_cls || (any_tok && (!tok_cls || !dur_post)) || (any_frame && !logits))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  DppLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok_win = tok_win;
  a.tok_dur = tok_dur; a.dur = dur; a.n_rows = n_rows; a.D = D;
  a.ws = (float*)workspace; a.logz = logz; a.tok_post = dur_post; a.status = status;
  return launch_all<true>(fn, a, n_clips, frame_off_host, n_frames_host, tok_off_host, n_tok_host, D, (hipStream_t)stream);
}

}  // extern "C"
