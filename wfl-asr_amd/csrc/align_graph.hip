// Viterbi forced alignment of a transcript GRAPH over the frame logits of a clip (wfl_align_graph, include/wfl_asr.h): pronunciation
// variants, `postprocess.transcript_variants`.  Every other lattice of the family is a chain; this one is a small DAG.
//
// A clip has N slots in topological order.  Slot k carries a token's alternatives (tok_cls, as wfl_align's), up to 8 predecessors
// (START, or a slot 1 .. 255 places in front of it) and a `final` flag.  States G_k, B_k, I_k per slot and one end gap G_end:
//   m_k(t)   = max{ G_k, then for p in pred(k) in list order: I_p, B_p } of frame t - 1          (the first listed wins an exact tie)
//   G_k(t)   = m_k(t) + EG_t     B_k(t) = m_k(t) + EB_t(k)     I_k(t) = max{I_k, B_k}(t - 1) + EI_t(k)
//   G_end(t) = max{ G_end, then for final f in slot order: I_f, B_f }(t - 1) + EG_t
//   start: frame 0 is G_k or B_k of a slot that lists START (G_end when N == 0); end: G_end | I_f | B_f over the final slots, in that order
// With pred(k) = {k - 1}, START for slot 0 and slot N - 1 alone final this is wfl_align's lattice state for state (G_end its G_N), and the
// same floats are added and compared in the same order: ids, tok and status are wfl_align's.
//
// One workgroup per clip; thread i owns the slots i R .. i R + R - 1 in registers, slot N holds G_end alone, as in csrc/align.hip.  What is
// new is the predecessor gather, in place of that kernel's one-float2 neighbour exchange:
//   every thread publishes per owned slot the exit score X_k = max{I_k, B_k} (I wins a tie) into a double-buffered [2][NT R] float array
//   in LDS -- slot k at (k mod R) NT + k / R, so the lanes of a wave write, and on a chain read, consecutive words -- and after the
//   frame's ONE barrier reads X of its slots' predecessors by index.  "I_p, then B_p" of the definition is X_p: which of the two it was
//   is a bit the OWNER of p stores with its own backpointers of that frame (the exit bit), so the gather moves one float per arc.
//   The predecessors of a slot are packed as eight byte distances k - p (0: unused) into two words, in registers for the frame loop and
//   in LDS for the backtrace.  START needs no distance: it matters at frame 0 alone, where every other candidate is -inf, so it is a
//   flag per slot.  The final slots stand as a list in LDS; the thread that owns slot N scans it each frame (a transcript's last
//   frontier: a handful), preferring G_end, then the lowest slot, and keeps its choice in one word per frame beside the backpointers.
//   Backpointers: 8 bits per slot and frame -- 4 the choice of m_k (0: G_k, j + 1: the j-th packed predecessor), shared by G_k and B_k,
//   1 I_k's (0: I_k, 1: B_k), 1 the exit bit (X_k was B_k) -- in the same words per thread as wfl_align's 6.
//   Backtrace: thread 0 walks GRAPH_W frames out of an LDS window that holds, for GRAPH_W + 1 frames, the words of the threads that
//   255 + GRAPH_W slots span below the current one, and the end words.  A frame may step back up to 255 slots, so a run of long jumps can
//   leave that window: a word outside it is read from memory instead, which costs time, never the result.
// The lattice's shared pieces -- LatClip, the configurations, the logits ring, the emissions, the renormalisation halves, the host side
// of a ragged batch -- are csrc/lattice.h's.  csrc/align.hip and its kernels are untouched.
#include "lattice.h"
#include "wfl_asr.h"

namespace {

using namespace lattice;

constexpr int GRAPH_W = 32;          // backtrace window, frames
constexpr int MAX_SLOTS = 2047;      // slots per clip: Shape<256, 8> with slot N for G_end
constexpr int MAX_PRED = 8;          // predecessors per slot
constexpr int MAX_SPAN = 255;        // a predecessor is at most this many slots back: a distance fits a byte
constexpr int NCFG_GRAPH = 4;        // lattice.h's configurations up to Shape<256, 8>
static_assert(kCfgMaxN[NCFG_GRAPH - 1] == MAX_SLOTS && 256 * 8 - 1 >= MAX_SLOTS, "the cap is the largest power-of-two configuration's");

struct GraphLaunch {
  const float* logits;
  long ldl;
  int C, o_id;
  const int* tok_cls;     // [total slots][4][2]
  const int* gap_cls;     // [n_clips][8]
  const int* slot_pred;   // [total slots][8]
  const int* slot_final;  // [total slots]
  unsigned* bp;           // LatClip::ws_off: T NT WPT backpointer words, then T end words
  int* ids;
  int* tok;
  float* score;
  int* taken;             // [total slots]
  int* status;
  int n;
  LatClip clip[CLIPS_PER_LAUNCH];
};

// LDS: lattice.h's base with X = the exit scores [2][NT R]; then the packed predecessors (two words per slot), the list of final slots,
// the backtrace window and a few words
template <int NT, int R>
struct CfgGraph : LdsBase<NT, R, 2 * NT * R * 4> {
  static_assert((R & (R - 1)) == 0, "slot -> X index by shift and mask");
  static constexpr int LOG_R = R == 2 ? 1 : R == 4 ? 2 : 3;
  static constexpr int WPT = (8 * R + 31) / 32;                                      // backpointer words per thread per frame
  static constexpr int SPAN = (MAX_SPAN + GRAPH_W) / R + 2 < NT ? (MAX_SPAN + GRAPH_W) / R + 2 : NT;   // threads of the window
  static constexpr int ROW = SPAN * WPT + 1;                                         // a frame of the window: those words and the end word
  static constexpr int WIN = (GRAPH_W + 1) * ROW;
  static constexpr int OFF_PRED = CfgGraph::OFF_OWN;
  static constexpr int OFF_FIN = OFF_PRED + NT * R * 8;
  static constexpr int OFF_WIN = OFF_FIN + NT * R * 4;
  static constexpr int OFF_MISC = OFF_WIN + WIN * 4;
  static constexpr int LDS = OFF_MISC + 128;
};
// at the cap: ring 32 KB + alternatives 32 KB + X 16 KB + predecessors 16 KB + finals 8 KB + window 9.7 KB + a few words = 114 KB
static_assert(CfgGraph<256, 8>::OFF_OWN == 2 * 256 * 16 * 4 + 2048 * 16 + 2 * 2048 * 4 + 64 + 128 &&
                  CfgGraph<256, 8>::LDS == CfgGraph<256, 8>::OFF_OWN + 2048 * 8 + 2048 * 4 + 33 * (37 * 2 + 1) * 4 + 128 &&
                  CfgGraph<256, 8>::LDS <= 160 * 1024,
              "LDS at the cap");
static_assert(CfgGraph<64, 2>::WPT == 1 && CfgGraph<256, 4>::WPT == 1 && CfgGraph<256, 8>::WPT == 2, "wfl_align's words per thread");

template <int NT, int R>
__global__ __launch_bounds__(NT) void align_graph_kernel(GraphLaunch a) {
  using K = CfgGraph<NT, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* ring = (float*)lds;
  int4* alt = (int4*)(lds + K::OFF_ALT);
  float* X = (float*)(lds + K::OFF_X);                // [2][NT R]
  float* wmax = (float*)(lds + K::OFF_WMAX);
  double* red = (double*)(lds + K::OFF_RED);
  uint2* pk = (uint2*)(lds + K::OFF_PRED);           // [NT R] eight byte distances, the used ones first
  int* flist = (int*)(lds + K::OFF_FIN);             // the final slots, in no order
  unsigned* win = (unsigned*)(lds + K::OFF_WIN);
  int* misc = (int*)(lds + K::OFF_MISC);             // 0 lattice_setup's flag, 1 the walk's state, 2 bad graph, 3 finals, 4 no path
  float* fin = (float*)(misc + 8);

  const LatClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = cl.T, N = cl.N, C = a.C;
  const float* Z = a.logits + cl.frame_off * a.ldl;
  int* ids = a.ids + cl.frame_off;
  int* tokp = a.tok + cl.frame_off;
  int* taken = a.taken + cl.tok_off;
  const float NEG = -INFINITY;
  auto xi = [](int k) { return (k & (R - 1)) * NT + (k >> K::LOG_R); };   // slot -> its place in a half of X

  // ---- the lattice: the classes (lattice.h), then the graph.  Status 2 before 4 before 1.
  int g[NGAP];
  uint2 pw[R];                                  // this thread's slots' packed predecessors
  unsigned sf = 0;                              // bit r: slot r lists START
  int st;
  if (tid == 0) { misc[2] = 0; misc[3] = 0; }
  if (N > MAX_SLOTS) st = 2;
  else st = lattice_setup<NT, R, true>(cl, C, a.tok_cls, a.gap_cls, alt, misc, g);   // (ANY_T: "no path" is the search's to find)
  if (st == 0) {
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = tid * R + r;
      uint2 w = make_uint2(0u, 0u);
      if (k < N) {
        const int* sp = a.slot_pred + (long)(cl.tok_off + k) * MAX_PRED;
        int used = 0, nd = 0;
        bool ended = false;
#pragma unroll
        for (int j = 0; j < MAX_PRED; ++j) {
          const int p = sp[j];
          if (p == -2) { ended = true; continue; }
          if (ended) { bad = true; continue; }            // a used entry behind an unused one
          ++used;
          if (p == -1) { sf |= 1u << r; continue; }
          if (p < -2 || p >= k || k - p > MAX_SPAN) { bad = true; continue; }
          const unsigned d = (unsigned)(k - p);
          if (nd < 4) w.x |= d << (8 * nd);
          else w.y |= d << (8 * (nd - 4));
          ++nd;
        }
        if (used == 0) bad = true;
        const int f = a.slot_final[cl.tok_off + k];
        if (f == 1) flist[atomicAdd(&misc[3], 1)] = k;    // (at most N entries)
        else if (f != 0) bad = true;
      }
      pk[k] = w;
      pw[r] = w;
    }
    if (N == 0 && tid == 0) sf = 1u;                      // no slot: frame 0 is G_end
    if (bad) misc[2] = 1;
    __syncthreads();
    if (misc[2] || (N > 0 && misc[3] == 0)) st = 4;
  }
  if (st != 0 || T == 0) {
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    for (int k = tid; k < N; k += NT) taken[k] = 0;
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = st; }
    return;
  }
  const int nfin = misc[3];
  const int own_t = N >> K::LOG_R, own_r = N & (R - 1);   // the thread and register slot of G_end

  // ---- forward pass
  LogitStages<NT, K::PR> stage(Z, a.ldl, T, C, ring);
  const int F = stage.F;
  float G[R], B[R], I[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    G[r] = B[r] = I[r] = NEG;
    X[r * NT + tid] = NEG;
    X[NT * R + r * NT + tid] = NEG;
  }
  stage.load(0);
  stage.store(0);
  stage.load(1);
  __syncthreads();
  int4 av[R];
#pragma unroll
  for (int r = 0; r < R; ++r) av[r] = alt[tid * R + r];
  unsigned* bp = a.bp + cl.ws_off;
  unsigned* endbp = bp + (long)T * NT * K::WPT;
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
    const float* Xp = X + ((t + 1) & 1) * NT * R;          // the frame before
    float ge = NEG;                                        // G_end's way in from a final slot: the best X_f, the lowest f on a tie
    int gef = 0;                                           // f + 1, 0: none
    if (tid == own_t) {
      for (int i = 0; i < nfin; ++i) {
        const int f = flist[i];
        const float x = Xp[xi(f)] - sub;
        if (x > ge || (x == ge && gef != 0 && f + 1 < gef)) { ge = x; gef = f + 1; }
      }
    }
    unsigned bits[K::WPT];
#pragma unroll
    for (int w = 0; w < K::WPT; ++w) bits[w] = 0;
    float xo[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = tid * R + r;
      float m = G[r];
      unsigned cg = 0;
      const unsigned long long pq = ((unsigned long long)pw[r].y << 32) | pw[r].x;
#pragma unroll
      for (int j = 0; j < MAX_PRED; ++j) {
        const int d = (int)((pq >> (8 * j)) & 255u);
        if (d == 0) break;
        const float x = Xp[xi(k - d)] - sub;
        if (x > m) { m = x; cg = j + 1; }
      }
      if (tid == own_t && r == own_r) {
        if (ge > m) m = ge;
        else gef = 0;
        endbp[t] = (unsigned)gef;
      }
      if (t == 0 && ((sf >> r) & 1u)) m = 0.f;             // the virtual frame -1 sits in START
      float mi = I[r];
      unsigned ci = 0;
      if (B[r] > mi) { mi = B[r]; ci = 1; }
      float eb = NEG, ei = NEG;
      if (k < N) tok_emission(row, av[r], eb, ei);
      G[r] = k <= N ? m + eg : NEG;
      B[r] = m + eb;
      I[r] = mi + ei;
      const unsigned xb = B[r] > I[r] ? 1u : 0u;           // the exit bit: X_k is B_k
      xo[r] = xb ? B[r] : I[r];
      bits[(8 * r) >> 5] |= (cg | (ci << 4) | (xb << 5)) << ((8 * r) & 31);
    }
    float* Xc = X + (t & 1) * NT * R;
#pragma unroll
    for (int r = 0; r < R; ++r) Xc[r * NT + tid] = xo[r];
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
    __syncthreads();                           // the gather and the renormalisation share it
    sub = 0.f;
    if (renorm) {
      // a graph whose every path is shorter than t frames can leave every state -inf: nothing to subtract then (the clip ends as status 1)
      const float M = renorm_max<K::NW>(wmax);
      if (M > NEG) {
#pragma unroll
        for (int r = 0; r < R; ++r) { G[r] -= M; B[r] -= M; I[r] -= M; }
        sub = M;
        acc += (double)M;
      }
    }
  }

  // ---- the best end state: G_end, then the final slots' exits in slot order
  if (tid == own_t) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r == own_r) fin[0] = G[r];
  }
  __syncthreads();
  float best = 0.f;
  if (tid == 0) {
    const float* Xc = X + ((T - 1) & 1) * NT * R;
    best = fin[0];
    int s = 3 * N;
    float bx = NEG;
    int bf = -1;
    for (int i = 0; i < nfin; ++i) {
      const int f = flist[i];
      const float x = Xc[xi(f)] - sub;
      if (x > bx || (x == bx && bf >= 0 && f < bf)) { bx = x; bf = f; }
    }
    if (bf >= 0 && bx > best) {
      best = bx;
      const unsigned w = bp[((long)(T - 1) * NT + (bf >> K::LOG_R)) * K::WPT + ((8 * (bf & (R - 1))) >> 5)];
      s = 3 * bf + (((w >> (((8 * (bf & (R - 1))) & 31) + 5)) & 1u) ? 1 : 2);
    }
    misc[1] = s;
    misc[4] = best == NEG;
  }
  __syncthreads();
  if (misc[4]) {                                // no path: status 1, the backpointers never walked
    for (int t = tid; t < T; t += NT) { ids[t] = a.o_id; tokp[t] = -1; }
    for (int k = tid; k < N; k += NT) taken[k] = 0;
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 1; }
    return;
  }
  for (int k = tid; k < N; k += NT) taken[k] = 0;         // until a frame of the path carries the slot (the last pass, behind barriers)

  // ---- backtrace, GRAPH_W frames per window
  int s = misc[1];
  for (int thi = T - 1; thi >= 1;) {
    const int flo = max(0, thi - GRAPH_W);
    const int nf = thi - flo + 1;                               // <= GRAPH_W + 1 frames: a step reads frame t and frame t - 1
    const int th_hi = min(min(max(s / 3, 0), N) >> K::LOG_R, NT - 1);
    const int th_lo = max(0, th_hi - (K::SPAN - 1));
    const int nw = (th_hi - th_lo + 1) * K::WPT, rowlen = nw + 1;
    for (int e = tid; e < nf * rowlen; e += NT) {
      const int f = e / rowlen, w = e - f * rowlen;
      win[e] = w < nw ? bp[((long)(flo + f) * NT + th_lo) * K::WPT + w] : endbp[flo + f];
    }
    __syncthreads();
    if (tid == 0) {
      // slot k's 8 bits of frame t, out of the window or, outside it, out of memory
      auto slot_bits = [&](int t, int k) -> unsigned {
        const int th = k >> K::LOG_R, pos = 8 * (k & (R - 1));
        const unsigned w = (t >= flo && th >= th_lo && th <= th_hi) ? win[(t - flo) * rowlen + (th - th_lo) * K::WPT + (pos >> 5)]
                                                                    : bp[((long)t * NT + th) * K::WPT + (pos >> 5)];
        return (w >> (pos & 31)) & 255u;
      };
      for (int t = thi; t > flo; --t) {
        tokp[t] = s;
        const int k = s / 3, j = s - 3 * k;
        int p = -1;                                             // the slot left at frame t - 1, if any
        if (k >= N) {
          const int e = (int)win[(t - flo) * rowlen + nw];
          if (e > 0) p = min(e - 1, N - 1);
        } else {
          const unsigned b = slot_bits(t, k);
          if (j == 2) {
            s -= (int)((b >> 4) & 1u);
          } else {
            const int cg = (int)(b & 15u);
            if (cg == 0) {
              s = 3 * k;
            } else {
              const uint2 w = pk[k];
              const unsigned long long pq = ((unsigned long long)w.y << 32) | w.x;
              p = max(k - (int)((pq >> (8 * ((cg - 1) & 7))) & 255u), 0);
            }
          }
        }
        if (p >= 0) s = 3 * p + (((slot_bits(t - 1, p) >> 5) & 1u) ? 1 : 2);
      }
      misc[1] = s;
    }
    __syncthreads();
    s = misc[1];
    thi = flo;
  }
  if (tid == 0) tokp[0] = s;
  __syncthreads();

  // ---- states -> (class id, slot); the score's per-frame log-sum-exp
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
      taken[k] = 1;
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

template <class F>
auto dispatch_graph(int cfg, F&& f) {
  switch (cfg) {
    case 0: return f(Shape<64, 2>());
    case 1: return f(Shape<256, 2>());
    case 2: return f(Shape<256, 4>());
    default: return f(Shape<256, 8>());
  }
}

// backpointer and end words of a clip.  Over the cap or with no frame the kernel stops at its status: no words.
long graph_words(int T, int N) {
  const int c = cfg_of(N);
  if (c >= NCFG_GRAPH || T <= 0) return 0;
  const int per_frame = dispatch_graph(c, [](auto sh) { return decltype(sh)::NT * CfgGraph<decltype(sh)::NT, decltype(sh)::R>::WPT; });
  return round64((long)T * (per_frame + 1));
}

}  // namespace

extern "C" {

int64_t wfl_align_graph_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_slots_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_slots_host, n_clips, graph_words);
}

int32_t wfl_align_graph(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                        const int32_t* n_frames_host, const int32_t* slot_off_host, const int32_t* n_slots_host, const int32_t* tok_cls,
                        const int32_t* gap_cls, int32_t n_clips, const int32_t* slot_pred, const int32_t* slot_final, void* workspace,
                        int64_t workspace_bytes, int32_t* ids, int32_t* tok, float* score, int32_t* taken, int32_t* status, void* stream) {
  const char* fn = "wfl_align_graph";
  const int64_t need = wfl_align_graph_workspace_bytes(n_frames_host, n_slots_host, n_clips);
  bool any_tok = false, any_frame = false;
  int rc = check_clip_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, slot_off_host, n_slots_host, n_clips, need, any_tok, any_frame);
  if (rc) return rc;
  if (n_clips == 0) return 0;
  if (!score || !status || !gap_cls || (any_tok && (!tok_cls || !slot_pred || !slot_final || !taken)) ||
      (any_frame && (!logits || !ids || !tok)))
    return fail(fn, -1, "null device pointer");
  if ((rc = check_workspace(fn, need, workspace, workspace_bytes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  GraphLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.tok_cls = tok_cls; a.gap_cls = gap_cls; a.slot_pred = slot_pred;
  a.slot_final = slot_final; a.bp = (unsigned*)workspace; a.ids = ids; a.tok = tok; a.score = score; a.taken = taken; a.status = status;
  return launch_clips<NCFG_GRAPH>(
      a, n_clips,
      [&](int b, long off, LatClip& c, int& cfg) {
        const int T = n_frames_host[b], N = n_slots_host[b];
        c = LatClip{(long)frame_off_host[b], off, T, slot_off_host[b], N, b};
        cfg = cfg_of(N) < NCFG_GRAPH ? cfg_of(N) : 0;   // over the cap: status 2 before the kernel touches anything; the smallest
        return graph_words(T, N);
      },
      [&](int cfg, const auto& a) {
        return dispatch_graph(cfg, [&](auto sh) {
          constexpr int NT = decltype(sh)::NT, R = decltype(sh)::R;
          return launch_cfg<align_graph_kernel<NT, R>, NT, CfgGraph<NT, R>::LDS>(fn, a, s);
        });
      });
}

}  // extern "C"
