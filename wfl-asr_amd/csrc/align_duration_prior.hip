// Viterbi forced alignment with a duration prior per token (wfl_align_duration_prior, include/wfl_asr.h): an explicit-duration
// (semi-Markov) search over the transcript.  A run of d frames of token k adds L_k(d) to the path's score, L a row of the caller's table
// `dur` ([n_rows][D + 1] fp32: L(1) .. L(D), then the per-frame `tail` of every frame past D), so a hard minimum or maximum duration is a
// row with -inf entries.  Token k uses row tok_dur[k]; -1: no prior (L = 0, tail = 0).
//
// Frame by frame (everything of frame t - 1 on the right):
//   Ent_k(t) = max(G_k(t-1), X_{k-1}(t-1))                         G first on a tie
//   G_k(t)   = Ent_k(t) + EG_t
//   R_k^1(t) = Ent_k(t) + EB_t(k)                                  (EB through lattice.h's win_mask where tok_win is given)
//   R_k^j(t) = R_k^{j-1}(t-1) + EI_t(k)          2 <= j <= D       a run of exactly j frames, prior not yet added
//   Y_k(t)   = (max(Y_k(t-1), R_k^D(t-1) + L_k(D)) + EI_t(k)) + tail_k      a run longer than D; Y first on a tie
//   X_k(t)   = max(max_j R_k^j(t) + L_k(j), Y_k(t))                frame t is the LAST frame of token k; shortest j first, Y last
//   end      = max(G_N(T-1), X_{N-1}(T-1))                         G first
// -inf entries only ever add, so no expression forms inf - inf.
//
// One workgroup per clip on the pieces of csrc/lattice.h (the configurations, setup and status, the logits ring, the emissions, the
// window mask, the renormalisation halves, the host's ragged batch); thread i owns the token slots i R .. i R + R - 1 and keeps their
// G, X and Y in registers.  Only X of the left thread's last slot crosses threads: one float per thread through LDS and the frame's
// ONE barrier, shared with the renormalisation.
//
// The history R_k^1 .. R_k^D is a ring of D floats per slot, indexed by the run's start frame modulo D: frame t first reads the entry
// t mod D (the run that began at t - D, i.e. R^D(t-1), what Y is entered from), overwrites it with R^1(t), and adds EI_t to the other
// D - 1.  Nothing is summed over the clip: an entry is at most D frames old, and every RENORM frames the block's maximum is taken off
// the ring's entries as it is off G, X and Y, so the fp32 scores never grow with T.  Entry (q, r) of thread i is word (q R + r) NT + i:
// a thread touches its own words only (no barrier) and a wave's lanes touch consecutive ones (no bank conflict, coalesced).  The ring
// lives in LDS behind the kernel's other areas where NT R D floats fit the CU's 160 KiB beside them, and in the clip's workspace
// (L2-resident) where they do not: hist_in_lds().  The table sits in LDS where it has at most TAB_FLOATS values, else it is read
// through the caches.
//
// Backpointers: one byte per slot and frame -- bit 0 Ent's choice (G_k | X_{k-1}; G_k(t) and R_k^1(t) share it), bit 1 Y's (stay |
// enter), bits 2 .. 7 X's winning duration 1 .. D, D + 1 for Y.  The backtrace is csrc/align.hip's: ALIGN_W frames of the words of at
// most ALIGN_W / R + 2 threads go to LDS at once and thread 0 walks them; a frame steps back one token at most.  From "frame t ends
// token k" it reads the duration j <= D and knows the next j frames (the last of them B_k, where Ent's bit is read) without another
// look; for a tail it follows Y's bits to the frame that entered Y, then D frames.
#include "lattice.h"
#include "wfl_asr.h"

namespace {

using namespace lattice;

constexpr int ALIGN_W = 32;                 // backtrace window, frames
constexpr int MAX_D = 32;                   // the table's longest explicit duration, frames
constexpr int TAB_FLOATS = 4096;            // the table is staged in LDS up to this many values (124 rows at D = 32)
constexpr int LDS_CAP = 160 * 1024;
constexpr int JU = 8;                       // ring entries of a slot in flight together

struct DurLaunch {
  const float* logits;
  long ldl;
  int C, o_id;
  const int* tok_cls;  // [total tokens][4][2]
  const int* gap_cls;  // [n_clips][8]
  unsigned* ws;        // LatClip::ws_off: the clip's backpointer words, then its history ring where LDS does not hold it
  int* ids;
  int* tok;
  float* score;
  int* status;
  int n;
  LatClip clip[CLIPS_PER_LAUNCH];
  const int* tok_win;  // [total tokens][2] = (lo, hi), or null
  const int* tok_dur;  // [total tokens] row of `dur`, -1 none
  const float* dur;    // [n_rows][D + 1]
  int n_rows, D;
};

template <int NT, int R>
struct CfgDur : LdsBase<NT, R, 2 * NT * 4> {             // its own between alt and wmax: the neighbour exchange, [2][NT] float
  static constexpr int WPT = (8 * R + 31) / 32;          // backpointer words per thread per frame: a byte per slot
  static constexpr int WIN = ALIGN_W * (ALIGN_W / R + 2) * WPT;
  static constexpr int OFF_WIN = CfgDur::OFF_OWN;        // the backtrace window
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int OFF_TAB = OFF_MISC + 64;          // the table, where it fits
  static constexpr int OFF_HIST = OFF_TAB + TAB_FLOATS * 4;
  static_assert(OFF_HIST % 16 == 0 && OFF_HIST <= LDS_CAP, "LDS");
  static constexpr long hist_words(int D) { return (long)NT * R * D; }
  static constexpr bool hist_in_lds(int D) { return OFF_HIST + hist_words(D) * 4 <= LDS_CAP; }
  static constexpr int lds_bytes(int D) { return OFF_HIST + (hist_in_lds(D) ? (int)hist_words(D) * 4 : 0); }
};

// WIN: the start windows (lattice.h win_mask); HL: the history ring is in LDS, else in the clip's workspace
template <int NT, int R, bool WIN, bool HL>
__global__ __launch_bounds__(NT) void dur_kernel(DurLaunch a) {
  using K = CfgDur<NT, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  float* xch = (float*)(lds + K::OFF_X);
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  unsigned* win = (unsigned*)(lds + K::OFF_WIN);
  int* misc = (int*)(lds + K::OFF_MISC);
  float* fin = (float*)(misc + 4);
  float* ltab = (float*)(lds + K::OFF_TAB);
  float* lhist = (float*)(lds + K::OFF_HIST);

  const LatClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = cl.T, N = cl.N, C = a.C, D = a.D, D1 = a.D + 1;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  int* ids = a.ids + cl.frame_off;
  int* tokp = a.tok + cl.frame_off;
  const float NEG = -INFINITY;

  int g[NGAP];
  int st = lattice_setup<NT, R>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);
  int row[R];                                   // this thread's slots' table rows, in registers (-1: no prior; slots past the tokens too)
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
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = st; }
    return;
  }

  // ---- the table and the history ring
  const bool TL = (long)a.n_rows * D1 <= TAB_FLOATS;
  if (TL)
    for (int e = tid; e < a.n_rows * D1; e += NT) ltab[e] = a.dur[e];
  const float* gtab = a.dur;
  unsigned* bp = a.ws + cl.ws_off;
  float* ghist = (float*)(bp + round64((long)T * NT * K::WPT));
  float* hist = (HL ? lhist : ghist) + tid;     // entry (q, r): hist[(q R + r) NT]
  for (int e = 0; e < D * R; ++e) hist[(long)e * NT] = NEG;

  // ---- forward pass
  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;
  float G[R], X[R], Y[R];
#pragma unroll
  for (int r = 0; r < R; ++r) G[r] = X[r] = Y[r] = NEG;
  if (tid == 0) G[0] = 0.f;                    // a virtual frame -1 in G_0: Ent_0(0) = 0
  xch[NT + tid] = NEG;
  stage.load(0);
  stage.store(0);
  stage.load(1);
  __syncthreads();

  constexpr bool AVR = NT < 512;               // (512 x 9: the alternatives stay in LDS, the registers go to G, X, Y and the rows)
  int4 av[AVR ? R : 1];
  if constexpr (AVR) {
#pragma unroll
    for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  }
  int2 wn[WIN ? R : 1];
  if constexpr (WIN) load_windows<R>(a.tok_win, cl.tok_off, N, wn);
  double acc = 0.0;                            // what the renormalisations subtracted
  float sub = 0.f;
  int c = 0, tin = 0, p = 0;                   // p = t mod D
  for (int t = 0; t < T; ++t, ++tin) {
    if (tin == F) {
      ++c;
      tin = 0;
      stage.store(c);
      __syncthreads();
      stage.load(c + 1);
    }
    const float* rowz = stage.row(c, tin);
    const float eg = gap_emission(rowz, g);
    const float nb = (tid > 0 ? xch[((t + 1) & 1) * NT + tid - 1] : NEG) - sub;
    unsigned bits[K::WPT];
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bits[w] = 0;
    // the frame's slots, once for the table in LDS and once for the table behind the caches: each path loads from ONE address space
    // (a pointer chosen at run time would make every table read a flat load)
    auto slots = [&](auto tl) {
      // entry j (0 .. D) of the row at word `base`; `has` false: 0.  The load is unconditional (row 0 stands in; a table of more than
      // TAB_FLOATS values has a row 0) and the choice a select, so a slot's loads are never behind a divergent branch
      auto L = [&](long base, bool has, int j) -> float {
        float v;
        if constexpr (decltype(tl)::value) v = ltab[(int)base + j];
        else v = gtab[base + j];
        return has ? v : 0.f;
      };
#pragma unroll
      for (int r = R - 1; r >= 0; --r) {         // descending: slot r - 1's previous-frame X is still in place
        const int k = tid * R + r;
        const float pX = r ? X[r > 0 ? r - 1 : 0] : nb;
        float ent = G[r];
        unsigned cg = 0;
        if (pX > ent) { ent = pX; cg = 1; }
        G[r] = k <= N ? ent + eg : NEG;
        unsigned byte = cg;
        if (k < N) {
          float eb, ei;
          if constexpr (AVR) tok_emission(rowz, av[r], eb, ei);
          else tok_emission(rowz, alt[k], eb, ei);
          if constexpr (WIN) eb = win_mask(eb, t, wn[r]);
          const bool has = row[r] >= 0;          // no row: L = 0, tail = 0 (the loads go to row 0 and are dropped)
          const long lb = (long)max(row[r], 0) * D1;
          float* h = hist + (long)r * NT;
          const long qs = (long)R * NT;          // words between two ring entries of a slot
          // Y: stay, or enter from the run that is D frames old (the ring entry this frame's opening replaces)
          const float old = h[p * qs];
          const float yc = old + L(lb, has, D - 1);
          float ym = Y[r];
          if (yc > ym) { ym = yc; byte |= 2u; }
          Y[r] = (ym + ei) + L(lb, has, D);
          const float r1 = ent + eb;
          h[p * qs] = r1;
          float x = r1 + L(lb, has, 0);
          unsigned dw = 1;
          // the runs that began at t - j + 1, j = 2 .. D, JU at a time and without a branch: the ring entries and the table entries of
          // a group are loaded before any of the group is stored, so the loads are in flight together (entry by entry, every load
          // waits for the one before it).  A j past D reads and rewrites the entry just written, and its candidate is -inf.
          for (int j0 = 2; j0 <= D; j0 += JU) {
            float hv[JU], lv[JU];
#pragma unroll
            for (int u = 0; u < JU; ++u) {
              const int j = min(j0 + u, D);
              int q = p - (j - 1);
              q = q < 0 ? q + D : q;
              q = j0 + u <= D ? q : p;
              hv[u] = h[q * qs];
              lv[u] = L(lb, has, j - 1);
            }
#pragma unroll
            for (int u = 0; u < JU; ++u) {
              const int j = min(j0 + u, D);
              const bool in = j0 + u <= D;
              int q = p - (j - 1);
              q = q < 0 ? q + D : q;
              q = in ? q : p;
              const float v = in ? hv[u] + ei : r1;
              h[q * qs] = v;
              const float cand = in ? v + lv[u] : NEG;
              if (cand > x) { x = cand; dw = j; }
            }
          }
          if (Y[r] > x) { x = Y[r]; dw = D1; }
          X[r] = x;
          byte |= dw << 2;
        }
        bits[(8 * r) >> 5] |= byte << ((8 * r) & 31);
      }
    };
    if (TL) slots(std::true_type());
    else slots(std::false_type());
    p = p + 1 == D ? 0 : p + 1;
    xch[(t & 1) * NT + tid] = X[R - 1];
    unsigned* bw = bp + ((long)t * NT + tid) * K::WPT;
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bw[w] = bits[w];
    const bool renorm = (t & (RENORM - 1)) == RENORM - 1;
    if (renorm) {
      float lm = NEG;
#pragma unroll
      for (int r = 0; r < R; ++r) lm = fmaxf(lm, fmaxf(G[r], fmaxf(X[r], Y[r])));
      renorm_publish(lm, wmax);
    }
    __syncthreads();                           // the neighbour exchange and the renormalisation share it
    sub = 0.f;
    if (renorm) {
      // (G_0 has no prior and no window and a finite emission at every frame: M is finite)
      const float M = renorm_max<K::NW>(wmax);
#pragma unroll
      for (int r = 0; r < R; ++r) { G[r] -= M; X[r] -= M; Y[r] -= M; }
      for (int e = 0; e < D * R; ++e) hist[(long)e * NT] -= M;      // the ring's entries too: this thread's own words
      sub = M;
      acc += (double)M;
    }
  }

  // ---- the best end state: G_N, then X_{N-1}
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid * R + r;
    if (k == N) fin[0] = G[r];
    if (k == N - 1) fin[1] = X[r];
  }
  __syncthreads();
  float best = 0.f;
  if (tid == 0) {
    best = fin[0];
    int k = N, cnt = -2;
    if (N >= 1 && fin[1] > best) { best = fin[1]; k = N - 1; cnt = 0; }
    misc[1] = k;
    misc[2] = best == NEG;
    misc[3] = cnt;
  }
  __syncthreads();
  if (misc[2]) {                                // the table, the windows or the frame count forbid every path: status 1
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 1; }
    return;
  }

  // ---- backtrace, ALIGN_W frames per window.  Thread 0's walker: token (or gap) k, and cnt = -2 frame t is in G_k | -1 frame t is a
  // tail frame of token k (Y) | 0 frame t is the last frame of token k, its run not yet read | j >= 1 frame t and the j - 1 before it
  // are the rest of a run of token k, the last of them B_k
  int k = misc[1];
  int cnt = misc[3];
  for (int thi = T - 1; thi >= 1;) {
    const int tlo = max(1, thi - ALIGN_W + 1);
    const int nf = thi - tlo + 1;
    const int k_hi = min(max(k, 0), N);
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
        const int th = k / R, r = k - th * R;
        const int wi = (t - tlo) * nw + (th - th_lo) * K::WPT + ((8 * r) >> 5);
        const unsigned b = (wi >= 0 && wi < nf * nw) ? (win[wi] >> ((8 * r) & 31)) & 0xffu : 0u;
        if (cnt == -2) {                        // a gap frame: it stayed in G_k, or token k - 1 ended the frame before
          tokp[t] = 3 * k;
          if ((b & 1u) && k > 0) { k -= 1; cnt = 0; }
          continue;
        }
        if (cnt == 0) {                         // the run that ends here: j <= D frames, or a tail
          const int dw = (int)(b >> 2);
          cnt = dw > D ? -1 : max(dw, 1);
        }
        if (cnt == -1) {                        // a tail frame: Y stayed, or it was entered from the D frames before
          tokp[t] = 3 * k + 2;
          if (b & 2u) cnt = D;
          continue;
        }
        if (cnt > 1) {
          tokp[t] = 3 * k + 2;
          --cnt;
          continue;
        }
        tokp[t] = 3 * k + 1;                    // B_k: opened from G_k, or behind token k - 1
        if ((b & 1u) && k > 0) { k -= 1; cnt = 0; }
        else cnt = -2;
      }
      misc[1] = k;
    }
    __syncthreads();
    k = misc[1];
    thi = tlo - 1;
  }
  if (tid == 0) tokp[0] = cnt == -2 ? 3 * k : 3 * k + 1;      // (frame 0 of a run is its B frame)
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
    const int kk = sv / 3, j = sv - 3 * kk;
    int id = a.o_id, tk = -1;
    if (j != 0 && kk < N) {
      float bv = NEG;
      for_each_alt(alt[kk], [&](int q, int b, int i) {      // the arg-max alternative's class, the first on a tie
        const int col = j == 2 ? i : b;
        const float x = z[col];
        if (q == 0 || x > bv) { bv = x; id = col; }
      });
      tk = kk;
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

// workspace words of a clip: its backpointer bytes, and the history ring where this configuration's LDS does not hold it at this D.
// Over the cap, with fewer frames than tokens or with no frame the kernel stops at its status: no words.
long clip_words(int T, int N, int D) {
  const int c = cfg_of(N);
  if (c == NCFG || T < N || T <= 0) return 0;
  return dispatch_cfg(c, [&](auto sh) {
    using K = CfgDur<decltype(sh)::NT, decltype(sh)::R>;
    return round64((long)T * decltype(sh)::NT * K::WPT) + (K::hist_in_lds(D) ? 0 : round64(K::hist_words(D)));
  });
}

}  // namespace

extern "C" {

int64_t wfl_align_duration_prior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips, int32_t D) {
  if (D < 1 || D > MAX_D) return -1;
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, [D](int T, int N) { return clip_words(T, N, D); });
}

int32_t wfl_align_duration_prior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                 const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                 const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                 const int32_t* tok_dur, const float* dur, int32_t n_rows, int32_t D, void* workspace,
                                 int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* status, void* stream) {
  const char* fn = "wfl_align_duration_prior";
  if (D < 1 || D > MAX_D) return fail(fn, -1, "D must be 1 .. 32");
  if (n_rows < 0) return fail(fn, -1, "n_rows < 0");
  const int64_t need = wfl_align_duration_prior_workspace_bytes(n_frames_host, n_tok_host, n_clips, D);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, tok_off_host, n_tok_host, n_clips, need, any_tok, any_frame);
  if (rc) return rc;
  if (n_rows > 0 && !dur) return fail(fn, -1, "null dur with n_rows > 0");
  if (n_clips == 0) return 0;
  if (any_tok && !tok_dur) return fail(fn, -1, "null tok_dur");
  if (!score || !status || !gap_cls || (any_tok && !tok_cls) || (any_frame && (!logits || !ids || !tok)))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  DurLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.tok_win = tok_win;
  a.tok_dur = tok_dur; a.dur = dur; a.n_rows = n_rows; a.D = D;
  a.ws = (unsigned*)workspace; a.ids = ids; a.tok = tok; a.score = score; a.status = status;
  return launch_clips<NCFG>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_tok_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, tok_off_host[b], N, b};
        cfg = cfg_of(N) < NCFG ? cfg_of(N) : 0;   // over the cap: the kernel reports status 2 before it touches the workspace; the smallest
        return clip_words(T, N, D);
      },
      [&](int cfg, DurLaunch& a) {
        return dispatch_cfg(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          using K = CfgDur<NT, R>;
          auto launch = [&](auto win_tag, auto hl_tag) {
            constexpr bool WIN = decltype(win_tag)::value, HL = decltype(hl_tag)::value;
            if (const int rc = reserve_lds<dur_kernel<NT, R, WIN, HL>, LDS_CAP>(fn)) return rc;     // (the most any D asks for)
            hipLaunchKernelGGL((dur_kernel<NT, R, WIN, HL>), dim3(a.n), dim3(NT), K::lds_bytes(D), s, a);
            return hipGetLastError() == hipSuccess ? 0 : fail(fn, -3, "launch failed");
          };
          const std::true_type yes;
          const std::false_type no;
          if (K::hist_in_lds(D)) return tok_win ? launch(yes, yes) : launch(no, yes);
          return tok_win ? launch(yes, no) : launch(no, no);
        });
      });
}

}  // extern "C"
