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
// renormalisation halves, and the host side of a ragged batch -- is csrc/lattice.h, shared with csrc/align_posterior.h.  Here: the
// max-product recursion, the backpointers and the backtrace.
//
// wfl_align_windowed is the same kernel instantiated with WIN: every token's EB passes through lattice.h's win_mask (the token may open
// only inside its window), and a clip whose best end state is -inf -- no path satisfies the windows -- reports status 1 before the
// backtrace.  The unwindowed instantiation holds none of it.
//
// wfl_align_min_duration is the kernel instantiated with MIND (with and without WIN): token k occupies at least D_k frames, by the chain
// states of lattice.h (chain_out / chain_shift), kept in registers beside G, B and I.  A chain frame has one predecessor, so it needs no
// backpointer: the bits stay 6 per slot and frame, and the I_k bit "entered" now means "from X_k", the chain's last state.  The backtrace
// then knows the D_k - 2 frames before it to be chain frames of token k (written as I_k frames) and the one before those to be B_k, whose
// G / B bits it reads there.  The B that a token's successor sees -- inside a thread, through the exchange, and as an end state -- is
// -inf where D_k > 1: the token is left from I_k alone.
//
// wfl_align_optional is the kernel instantiated with OPT (with and without WIN, never with MIND): where token k - 1 is optional, B_k is
// also entered from G_{k-1}, I_{k-2} and B_{k-2}, each minus the skip penalty, after the three arcs above (which win a tie).  G and I are
// entered as before, so a labelling is one path and at most one token is skipped between two kept ones.  B_k's choice takes 3 bits, I_k's
// its 1: still 6 per slot and frame (2 G, 3 B, 1 I), the same words.  Slot 0 of a thread needs B, I, G of the left thread's last slot and
// B, I of the one before it, slot 1 the first two: the exchange carries those five floats per thread (CfgOpt, R >= 2 everywhere), and
// the renormalisation's `sub` applies to all five.  A frame of the backtrace may step back two tokens, so its LDS window holds the words
// of 2 ALIGN_W / R + 2 threads.  The ends that skip token N - 1 are G_{N-1}, I_{N-2}, B_{N-2} minus the penalty, after the usual three.
// `skipped` is filled with 1 for the clip's tokens once a path is known to exist, and the last pass stores 0 from every frame that
// carries a token.  A clip may now have a path with fewer frames than tokens, so it has backpointer words then too
// (wfl_align_optional_workspace_bytes; wfl_align's figure wherever T >= N), and "no path" is found as the windowed kernels find it.
//
// wfl_align_filler is the kernel instantiated with FILL (with and without WIN, never with MIND or OPT): the states, arcs and tie rules
// are wfl_align's, only the emission of a flagged token differs -- EB = EI = the frame's largest logit over all C classes minus the filler
// penalty.  Once per stage of the logits ring the block computes that value for every staged row (groups of lanes share a row in LDS; one
// more barrier per stage) into [2][FMAX] floats (CfgFill), so a frame reads one LDS float; a clip without a flag skips it.  The last pass
// already scans all C classes per frame for the log-sum-exp and tracks the first arg-max there: a filler frame's id.  The backpointers,
// the backtrace and the workspace are wfl_align's own.
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
  const int* tok_min;  // [total tokens] D_k, the minimum-duration kernels alone
};

template <int NT, int R>
struct Cfg : LdsBase<NT, R, 2 * NT * 8> {                // its own between alt and wmax: the neighbour exchange, [2][NT] float2
  static constexpr int WPT = (6 * R + 31) / 32;          // backpointer words per thread per frame
  static constexpr int WIN = ALIGN_W * (ALIGN_W / R + 2) * WPT;
  static constexpr int OFF_WIN = Cfg::OFF_OWN;           // the backtrace window
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int LDS = OFF_MISC + 64;
};

// wfl_align_optional's layout: the exchange carries XN floats per thread, [2][XN][NT], and a frame of the backtrace may step back two
// tokens, so ALIGN_W frames need the words of 2 ALIGN_W / R + 2 threads.  The same words per thread: 2 bits G, 3 bits B, 1 bit I.
constexpr int XN = 5;                       // B, I, G of the thread's last slot, B, I of the one before it
template <int NT, int R>
struct CfgOpt : LdsBase<NT, R, 2 * XN * NT * 4> {
  static_assert(R >= 2, "the widened exchange takes a thread's last TWO slots");
  static constexpr int WPT = Cfg<NT, R>::WPT;
  static constexpr int WIN = ALIGN_W * (2 * ALIGN_W / R + 2) * WPT;
  static constexpr int OFF_WIN = CfgOpt::OFF_OWN;
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int LDS = OFF_MISC + 64;
};

// the kernel arguments of wfl_align_optional: AlignLaunch (which stays the record it was for the other entries) and the optional tokens
struct AlignLaunchOpt : AlignLaunch {
  const int* tok_opt;  // [total tokens] 0 | 1
  int* skipped;        // [total tokens]
  float lambda;        // the skip penalty, nats
};

// wfl_align_filler's layout: Cfg's, and in front of the backtrace window the filler emission of every staged frame -- the row's maximum
// over all C classes minus the penalty -- [2][FMAX] floats, one half per stage of the ring
template <int NT, int R>
struct CfgFill : LdsBase<NT, R, 2 * NT * 8> {
  static constexpr int WPT = Cfg<NT, R>::WPT;
  static constexpr int WIN = Cfg<NT, R>::WIN;
  static constexpr int OFF_FILL = CfgFill::OFF_OWN;
  static constexpr int OFF_WIN = OFF_FILL + 2 * FMAX * 4;
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int LDS = OFF_MISC + 64;
};

// the kernel arguments of wfl_align_filler: AlignLaunch and the filler tokens
struct AlignLaunchFill : AlignLaunch {
  const int* tok_fill;  // [total tokens] 0 | 1
  float phi;            // the filler penalty, nats per frame
};

// WIN: the start windows of wfl_align_windowed (lattice.h win_mask); false is wfl_align's kernel, instruction for instruction
// MIND: the minimum durations of wfl_align_min_duration (lattice.h chain_*); false leaves the two kernels above as they were
// OPT: the skip arcs of wfl_align_optional (B_k also from G_{k-1}, I_{k-2}, B_{k-2} where token k - 1 is optional); false leaves the
// kernels above as they were.  Never with MIND.
// FILL: the filler tokens of wfl_align_filler (EB = EI = the frame's largest logit minus the penalty where the token is flagged); false
// leaves the kernels above as they were.  Never with MIND or OPT.
template <int NT, int R, bool WIN, bool MIND, bool OPT, bool FILL = false>
__global__ __launch_bounds__(NT) void align_kernel(
    std::conditional_t<OPT, AlignLaunchOpt, std::conditional_t<FILL, AlignLaunchFill, AlignLaunch>> a) {
  static_assert(!(OPT && MIND), "no skip arcs in the minimum-duration lattice");
  static_assert(!(FILL && (MIND || OPT)), "no filler emission in the minimum-duration and skip lattices");
  using K = std::conditional_t<OPT, CfgOpt<NT, R>, std::conditional_t<FILL, CfgFill<NT, R>, Cfg<NT, R>>>;
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
  int st;
  unsigned fm = 0;                              // FILL: bit r = "this thread's slot r is a filler"
  bool anyfill = false;                         // FILL: the clip has a filler (the same in every thread)
  unsigned om = 0;                              // OPT: bit r = "token k - 1 is optional", k this thread's slot r: B_k has skip arcs
  if constexpr (OPT) {
    // the clip's flags, before anything else: a value other than 0 | 1 is status 4; a clip without any flag and with fewer frames than
    // tokens is wfl_align's status 1, whatever its classes are
    if (tid == 0) { misc[2] = 0; misc[3] = 0; }
    __syncthreads();
    bool any = false, bad = false;
    for (int k = tid; k < N; k += NT) {
      const int f = a.tok_opt[cl.tok_off + k];
      any |= f != 0;
      bad |= f != 0 && f != 1;
    }
    if (any) misc[2] = 1;
    if (bad) misc[3] = 1;
    __syncthreads();
    const bool none = misc[2] == 0, badf = misc[3] != 0;
    __syncthreads();                            // (lattice_setup writes misc[0]; misc[2] is written again at the end states)
    if (N <= NT * R - 1 && N <= MAX_TOKENS && T < N && none) st = 1;
    else st = lattice_setup<NT, R, true>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
    if (st == 0 && badf) st = 4;
    if (st == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k1 = tid * R + r - 1;        // (never below 0 or past the tokens: such a slot has no skip arc)
        if (k1 >= 0 && k1 < N && a.tok_opt[cl.tok_off + k1] != 0) om |= 1u << r;
      }
    }
  } else if constexpr (FILL) {
    // the clip's flags, as OPT reads its own: a value other than 0 | 1 is status 4 (after wfl_align's 2 and 1); a clip without any flag
    // never computes a row maximum
    if (tid == 0) { misc[2] = 0; misc[3] = 0; }
    __syncthreads();
    bool any = false, bad = false;
    for (int k = tid; k < N; k += NT) {
      const int f = a.tok_fill[cl.tok_off + k];
      any |= f != 0;
      bad |= f != 0 && f != 1;
    }
    if (any) misc[2] = 1;
    if (bad) misc[3] = 1;
    __syncthreads();
    anyfill = misc[2] != 0;
    const bool badf = misc[3] != 0;
    __syncthreads();                            // (lattice_setup writes misc[0]; misc[2] is written again at the end states)
    st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
    if (st == 0 && badf) st = 4;
    if (st == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = tid * R + r;
        if (k < N && a.tok_fill[cl.tok_off + k] != 0) fm |= 1u << r;
      }
    }
  } else {
    st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
  }
  int dm[MIND ? R : 1];                         // this thread's slots' minimum durations, in registers
  if constexpr (MIND) {
    if (st == 0) {                              // (the same in every thread).  A D_k outside 1 .. MAX_MIN_FRAMES: status 4
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
  if (st != 0 || T == 0) {
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    if constexpr (OPT) {
      for (int k = tid; k < N; k += NT) a.skipped[cl.tok_off + k] = 0;
    }
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = st; }
    return;
  }

  // ---- forward pass
  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;
  float a_phi = 0.f;                           // FILL: the penalty
  if constexpr (FILL) a_phi = a.phi;

  float G[R], B[R], I[R];
#pragma unroll
  for (int r = 0; r < R; ++r) G[r] = B[r] = I[r] = NEG;
  float H[MIND ? R : 1][CHAIN];                // the chain states H^2 .. H^{MAX_MIN_FRAMES - 1} of every slot
  if constexpr (MIND) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < CHAIN; ++j) H[r][j] = NEG;
  }
  if (tid == 0) G[0] = 0.f;                    // a virtual frame -1 in G_0: frame 0 starts in G_0 or B_0 (OPT: or, skipping token 0, B_1)
  float* xo = (float*)xch;                     // OPT: [2][XN][NT]
  float lam = 0.f;
  if constexpr (OPT) {
    lam = a.lambda;
#pragma unroll
    for (int j = 0; j < XN; ++j) xo[(XN + j) * NT + tid] = NEG;
  } else {
    xch[NT + tid] = make_float2(NEG, NEG);
  }
  stage.load(0);
  stage.store(0);
  stage.load(1);
  __syncthreads();
  // FILL: the filler emission of every row of a stage, once per stage and behind a barrier of its own: FG threads share a row (FG the
  // largest power of two <= NT / F, at most a wave: 8 at C = 141), each takes every FG-th class of it in LDS and log2(FG) exchanges
  // inside the group end it, so no thread scans a whole row and the frame loop reads one float per frame.  A clip without a filler
  // (the same in every thread) does none of it.
  float* fem = nullptr;
  if constexpr (FILL) fem = (float*)(lds + K::OFF_FILL);
  int FG = 1;
  if constexpr (FILL) {
    FG = 64;
    while (FG * F > NT) FG >>= 1;               // (F <= FMAX = 32 <= NT / 2: FG >= 2; a group never straddles a wave)
  }
  auto fill_stage = [&](int cs) {
    const int f = tid / FG, sub = tid - f * FG;
    float mx = NEG;
    if (f < F) {
      const float* rw = stage.row(cs, f);
      for (int q = sub; q < C; q += FG) mx = fmaxf(mx, rw[q]);
    }
    for (int o = FG >> 1; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (f < F && sub == 0) fem[(cs & 1) * FMAX + f] = mx - a_phi;
    __syncthreads();
  };
  if constexpr (FILL) {
    if (anyfill) fill_stage(0);
  }

  // this thread's slots' alternatives, for the whole forward pass.  (512 x 9 with the chain: 4 R registers too many, it would spill --
  // that one configuration reads them from LDS every frame)
  constexpr bool AVR = !(MIND && NT >= 512);
  int4 av[AVR ? R : 1];
  if constexpr (AVR) {
#pragma unroll
    for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  }
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
      if constexpr (FILL) {
        if (anyfill) fill_stage(c);
      }
    }
    const float* row = stage.row(c, tin);
    const float eg = gap_emission(row, g);
    float ef = 0.f;                             // FILL: what a filler emits at this frame
    if constexpr (FILL) {
      if (anyfill) ef = fem[(c & 1) * FMAX + tin];
    }
    float2 nb;
    float nG1 = NEG, nB2 = NEG, nI2 = NEG;      // OPT: G of the left thread's last slot, B and I of the slot before it
    if constexpr (OPT) {
      const float* xp = xo + ((t + 1) & 1) * XN * NT + tid - 1;
      nb = tid > 0 ? make_float2(xp[0], xp[NT]) : make_float2(NEG, NEG);
      if (tid > 0) { nG1 = xp[2 * NT]; nB2 = xp[3 * NT]; nI2 = xp[4 * NT]; }
      nG1 -= sub;
      nB2 -= sub;
      nI2 -= sub;
    } else {
      nb = tid > 0 ? xch[((t + 1) & 1) * NT + tid - 1] : make_float2(NEG, NEG);
    }
    nb.x -= sub;
    nb.y -= sub;
    unsigned bits[K::WPT];
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bits[w] = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {         // descending: slot r - 1's previous-frame values are still in place
      const int k = tid * R + r;
      float pB1 = r ? B[r > 0 ? r - 1 : 0] : nb.x;
      if constexpr (MIND) {                    // the left token is left from its I alone where its D > 1 (nb.x: masked by its owner)
        if (r && dm[r > 0 ? r - 1 : 0] > 1) pB1 = NEG;
      }
      const float pI1 = r ? I[r > 0 ? r - 1 : 0] : nb.y;
      float m = G[r];
      unsigned cg = 0;
      if (pI1 > m) { m = pI1; cg = 1; }
      if (pB1 > m) { m = pB1; cg = 2; }
      float mb = m;                            // B_k: G_k's three, then the skip arcs over token k - 1
      unsigned cb = cg;
      if constexpr (OPT) {
        if ((om >> r) & 1u) {
          const float sG = (r ? G[r > 0 ? r - 1 : 0] : nG1) - lam;
          const float sI = (r >= 2 ? I[r > 1 ? r - 2 : 0] : r == 1 ? nb.y : nI2) - lam;
          const float sB = (r >= 2 ? B[r > 1 ? r - 2 : 0] : r == 1 ? nb.x : nB2) - lam;
          if (sG > mb) { mb = sG; cb = 3; }
          if (sI > mb) { mb = sI; cb = 4; }
          if (sB > mb) { mb = sB; cb = 5; }
        }
      }
      float mi = I[r];
      unsigned ci = 0;
      float x = B[r];                          // what I_k is entered from
      if constexpr (MIND) x = chain_out(B[r], H[r], dm[r]);
      if (x > mi) { mi = x; ci = 1; }
      float eb = NEG, ei = NEG;
      if (k < N) {
        if constexpr (AVR) tok_emission(row, av[r], eb, ei);
        else tok_emission(row, alt[k], eb, ei);
      }
      if constexpr (FILL) {
        if ((fm >> r) & 1u) eb = ei = ef;
      }
      if constexpr (WIN) eb = win_mask(eb, t, wn[r]);
      G[r] = k <= N ? m + eg : NEG;
      if constexpr (MIND) chain_shift(H[r], B[r], ei, dm[r]);
      if constexpr (OPT) B[r] = mb + eb;
      else B[r] = m + eb;
      I[r] = mi + ei;
      bits[(6 * r) >> 5] |= cg << ((6 * r) & 31);
      if constexpr (OPT) {                     // 2 bits G, 3 bits B, 1 bit I: no field straddles a word (6 r + 2 .. 6 r + 4 never holds bit 32)
        bits[(6 * r + 2) >> 5] |= cb << ((6 * r + 2) & 31);
        bits[(6 * r + 5) >> 5] |= ci << ((6 * r + 5) & 31);
      } else {
        bits[(6 * r + 2) >> 5] |= cg << ((6 * r + 2) & 31);
        bits[(6 * r + 4) >> 5] |= ci << ((6 * r + 4) & 31);
      }
    }
    if constexpr (OPT) {
      float* xq = xo + (t & 1) * XN * NT + tid;
      xq[0] = B[R - 1];
      xq[NT] = I[R - 1];
      xq[2 * NT] = G[R - 1];
      xq[3 * NT] = B[R - 2];
      xq[4 * NT] = I[R - 2];
    } else if constexpr (MIND) xch[(t & 1) * NT + tid] = make_float2(dm[R - 1] > 1 ? NEG : B[R - 1], I[R - 1]);
    else xch[(t & 1) * NT + tid] = make_float2(B[R - 1], I[R - 1]);
    unsigned* bw = bp + ((long)t * NT + tid) * K::WPT;
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bw[w] = bits[w];
    const bool renorm = (t & (RENORM - 1)) == RENORM - 1;
    if (renorm) {
      float lm = NEG;
#pragma unroll
      for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(G[r], fmaxf(B[r], I[r])));
      if constexpr (MIND) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < CHAIN; ++j) lm = fmaxf(lm, H[r][j]);
      }
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

  // ---- the best end state
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
    if (tid == 0) misc[3] = N >= 1 ? a.tok_opt[cl.tok_off + N - 1] : 0;
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
    if constexpr (OPT) {
      if (N >= 1 && misc[3]) {
        if (fin[3] - lam > best) { best = fin[3] - lam; s = 3 * N - 3; }
        if (N >= 2) {
          if (fin[4] - lam > best) { best = fin[4] - lam; s = 3 * N - 4; }
          if (fin[5] - lam > best) { best = fin[5] - lam; s = 3 * N - 5; }
        }
      }
    }
    misc[1] = s;
    if constexpr (WIN || MIND || OPT) misc[2] = best == NEG;
  }
  __syncthreads();
  if constexpr (WIN || MIND || OPT) {
    if (misc[2]) {                              // no path meets every window and duration (OPT: or too few frames): status 1, the
      for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }            // backpointers never walked
      if constexpr (OPT) {
        for (int k = tid; k < N; k += NT) a.skipped[cl.tok_off + k] = 0;
      }
      if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 1; }
      return;
    }
  }
  if constexpr (OPT) {                          // every token skipped, until a frame of the path carries it (the last pass, behind barriers)
    for (int k = tid; k < N; k += NT) a.skipped[cl.tok_off + k] = 1;
  }

  // ---- backtrace, ALIGN_W frames per window
  int s = misc[1];
  int chain = 0;                                // thread 0: chain frames of the run still to walk; a run's opening may straddle windows
  for (int thi = T - 1; thi >= 1;) {
    const int tlo = max(1, thi - ALIGN_W + 1);
    const int nf = thi - tlo + 1;
    const int k_hi = min(max(s / 3, 0), N);
    const int k_lo = max(0, k_hi - (OPT ? 2 * nf : nf));      // (OPT: a frame may step back two tokens)
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
        if constexpr (MIND) {
          if (chain > 0) {                      // frame t is a chain frame (written as I_k); the frame before the chain is B_k
            if (--chain == 0) s -= 1;
            continue;
          }
        }
        const int k = s / 3, j = s - 3 * k;
        const int th = k / R, r = k - th * R;
        const int pos = OPT ? 6 * r + (j == 0 ? 0 : j == 1 ? 2 : 5) : 2 * (3 * r + j);
        const unsigned field = OPT ? (j == 0 ? 3u : j == 1 ? 7u : 1u) : 3u;
        const int wi = (t - tlo) * nw + (th - th_lo) * K::WPT + (pos >> 5);
        const unsigned ch = (wi >= 0 && wi < nf * nw) ? (win[wi] >> (pos & 31)) & field : 0u;
        if constexpr (MIND) {
          if (j == 2 && ch == 1 && k < N) {     // I_k entered at t: from B_k for D_k <= 2, else through D_k - 2 chain frames
            const int d = a.tok_min[cl.tok_off + k];
            if (d >= 3) { chain = d - 2; continue; }
          }
        }
        s = j == 2 ? s - (int)ch : 3 * k - (int)ch;      // (OPT: B_k's 3, 4, 5 are G_{k-1}, I_{k-2}, B_{k-2} = 3 k - 3, - 4, - 5)
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
    int am = 0;                                 // FILL: the first arg-max class over all C, a filler frame's id
    if constexpr (FILL) {
      for (int q = 1; q < C; ++q)
        if (z[q] > m) { m = z[q]; am = q; }
    } else {
      for (int q = 1; q < C; ++q) m = fmaxf(m, z[q]);
    }
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
      if constexpr (FILL) {
        if (a.tok_fill[cl.tok_off + k] != 0) id = am;
      }
    }
    ids[t] = id;
    tokp[t] = tk;
    if constexpr (OPT) {
      if (tk >= 0) a.skipped[cl.tok_off + tk] = 0;
    }
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

// the same for wfl_align_optional: a clip with fewer frames than tokens may still have a path (it skips tokens), so it has its words
long clip_words_opt(int T, int N) {
  const int c = cfg_of(N);
  if (c == NCFG || T <= 0) return 0;
  const int per_frame = dispatch_cfg(c, [](auto sh) { return decltype(sh)::NT * Cfg<decltype(sh)::NT, decltype(sh)::R>::WPT; });
  return round64((long)T * per_frame);      // (wfl_align's own figure wherever T >= N)
}

}  // namespace

extern "C" {

int64_t wfl_align_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_words);
}

int64_t wfl_align_optional_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_words_opt);
}

int64_t wfl_align_filler_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_words);      // (the same backpointer words: wfl_align's own figure)
}

}  // extern "C"

namespace {

// wfl_align (WIN false), wfl_align_windowed, wfl_align_min_duration (MIND, with or without windows), wfl_align_optional (OPT, with or
// without windows; tok_opt, skipped and skip_penalty are its alone) and wfl_align_filler (FILL, with or without windows; tok_fill and
// filler_penalty are its alone): one host path
template <bool WIN, bool MIND, bool OPT = false, bool FILL = false>
int align_batch(const char* fn, const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                const int32_t* tok_win, const int32_t* tok_min, const int32_t* gap_cls, int32_t n_clips, void* workspace,
                int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream,
                const int32_t* tok_opt = nullptr, float skip_penalty = 0.f, int32_t* skipped = nullptr, const int32_t* tok_fill = nullptr,
                float filler_penalty = 0.f) {
  const int64_t need = OPT ? wfl_align_optional_workspace_bytes(n_frames_host, n_tok_host, n_clips)
                           : wfl_align_workspace_bytes(n_frames_host, n_tok_host, n_clips);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc) return rc;
  if (OPT && !(skip_penalty >= 0.f && skip_penalty <= 3.0e38f)) return fail(fn, -1, "skip_penalty must be a finite number >= 0");
  if (FILL && !(filler_penalty >= 0.f && filler_penalty <= 3.0e38f)) return fail(fn, -1, "filler_penalty must be a finite number >= 0");
  if (n_clips == 0) return 0;
  if (!score || !status || !gap_cls ||
      (any_tok && (!tok_cls || (WIN && !tok_win) || (MIND && !tok_min) || (OPT && (!tok_opt || !skipped)) || (FILL && !tok_fill))) ||
      (any_frame && (!logits || !ids || !tok)))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::conditional_t<OPT, AlignLaunchOpt, std::conditional_t<FILL, AlignLaunchFill, AlignLaunch>> a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok_win = tok_win; a.tok_min = tok_min;
  a.bp = (unsigned*)workspace; a.ids = ids; a.tok = tok; a.score = score; a.status = status;
  if constexpr (OPT) { a.tok_opt = tok_opt; a.skipped = skipped; a.lambda = skip_penalty; }
  if constexpr (FILL) { a.tok_fill = tok_fill; a.phi = filler_penalty; }
  return launch_clips<NCFG>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_tok_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b};
        cfg = cfg_of(N) < NCFG ? cfg_of(N) : 0;   // over the cap: every kernel reports status 2 before it touches the workspace; the smallest
        return OPT ? clip_words_opt(T, N) : clip_words(T, N);
      },
      [&](int cfg, const auto& a) {
        return dispatch_cfg(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          using K = std::conditional_t<OPT, CfgOpt<NT, R>, std::conditional_t<FILL, CfgFill<NT, R>, Cfg<NT, R>>>;
          return launch_cfg<align_kernel<NT, R, WIN, MIND, OPT, FILL>, NT, K::LDS>(fn, a, s);
        });
      });
}

}  // namespace

extern "C" {

int32_t wfl_align(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                  const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls, const int32_t* gap_cls, int32_t n_clips,
                  void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  return align_batch<false, false>("wfl_align", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                                   nullptr, nullptr, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status, stream);
}

int32_t wfl_align_windowed(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                           const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, void* workspace, int64_t workspace_bytes,
                           int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  return align_batch<true, false>("wfl_align_windowed", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host,
                                  tok_cls, tok_win, nullptr, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status, stream);
}

int32_t wfl_align_min_duration(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                               const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                               const int32_t* tok_win, const int32_t* tok_min, const int32_t* gap_cls, int32_t n_clips, void* workspace,
                               int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  const char* fn = "wfl_align_min_duration";
  return tok_win ? align_batch<true, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls, tok_win,
                                           tok_min, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status, stream)
                 : align_batch<false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                                            nullptr, tok_min, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status, stream);
}

int32_t wfl_align_optional(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                           const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                           const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* tok_opt, float skip_penalty,
                           void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* skipped,
                           int32_t* status, void* stream) {
  const char* fn = "wfl_align_optional";
  return tok_win ? align_batch<true, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                                                  tok_win, nullptr, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score, status,
                                                  stream, tok_opt, skip_penalty, skipped)
                 : align_batch<false, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host,
                                                   tok_cls, nullptr, nullptr, gap_cls, n_clips, workspace, workspace_bytes, ids, tok, score,
                                                   status, stream, tok_opt, skip_penalty, skipped);
}

int32_t wfl_align_filler(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                         const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                         const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips, const int32_t* tok_fill, float filler_penalty,
                         void* workspace, int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status,
                         void* stream) {
  const char* fn = "wfl_align_filler";
  return tok_win ? align_batch<true, false, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host,
                                                         tok_cls, tok_win, nullptr, gap_cls, n_clips, workspace, workspace_bytes, ids, tok,
                                                         score, status, stream, nullptr, 0.f, nullptr, tok_fill, filler_penalty)
                 : align_batch<false, false, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host,
                                                          tok_cls, nullptr, nullptr, gap_cls, n_clips, workspace, workspace_bytes, ids, tok,
                                                          score, status, stream, nullptr, 0.f, nullptr, tok_fill, filler_penalty);
}

}  // extern "C"
