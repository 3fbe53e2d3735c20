// BIO-grammar Viterbi decode with a phone-bigram prior AND a duration prior per phoneme (wfl_decode_duration, include/wfl_asr.h): the
// free decode as an explicit-duration (semi-Markov) search.  Symbols, states, legality, forced frames, the virtual O frame and the
// N x N max-plus step over the table `trans` are wfl_decode_bigram's (csrc/decode_bigram.hip); a run of d frames of phoneme q adds
// L_q(d), L the row sym_dur[q - 1] of the caller's table `dur` ([n_rows][D + 1] fp32: L(1) .. L(D), then the per-frame `tail` of every
// frame past D; wfl_align_duration_prior's layout), -1: no prior (L = 0, tail = 0).  O runs carry no prior.
//
// Frame by frame (everything of frame t - 1 on the right), for phoneme q:
//   In_q(t)  = max_s (end_s(t-1) + W[s][q])                                 the lowest s on a tie (the bigram kernel's product)
//   R_q^1(t) = In_q(t) + zB_t(q)
//   R_q^j(t) = R_q^{j-1}(t-1) + zI_t(q)            2 <= j <= D              a run of exactly j frames, prior not yet added
//   Y_q(t)   = (max(Y_q(t-1), R_q^D(t-1) + L_q(D)) + zI_t(q)) + tail_q      a run longer than D; Y first on a tie
//   end_q(t) = max(max_j R_q^j(t) + L_q(j), Y_q(t))                         frame t is the LAST frame of a run of q; shortest j first, Y last
//   O        : z + max(d[O], max_{p != O} (end_p(t-1) + W[p][O]))           wfl_decode_bigram's line
// -inf entries only ever add, so no expression forms inf - inf.
//
// Two kernels.  bio::pre_kernel (csrc/bio_grammar.h) writes the frames' log-sum-exp and forced flags.  duration_chain_kernel, ONE WORKGROUP
// of 256 threads per clip, is the bigram chain kernel -- the table in LDS, four predecessor slices, thread q owns symbol q, two barriers
// per frame -- plus, in the owner, the run history, Y, the D-way maximum and a wider backpointer.  The D adds and compares sit on the
// serial chain between the two barriers; the N x N product does not.
//
// The history R_q^1 .. R_q^D is a ring of D floats per symbol, indexed by the run's start frame modulo D: frame t first reads entry
// t mod D (the run that began at t - D, i.e. R^D(t-1), what Y is entered from), overwrites it with R^1(t), and adds zI_t to the other
// D - 1.  An entry is at most D frames old and every 16 frames the maximum of end[] is taken off the ring's entries as it is off d[O]
// and Y (in the same pass that adds zI: no extra sweep), the offset carried in a double: nothing grows with T.  Entry j of symbol q is
// word j HS + q, HS = round_up_64(N): a thread touches its own words only (no barrier) and a wave's lanes touch consecutive ones (no
// bank conflict, coalesced).  Behind the ring, in the same layout, lies the symbol's own row of `dur` (D + 1 words, zeros for no prior),
// so the owner's table reads are conflict-free too.  Both areas, (2 D + 1) HS floats, live in LDS behind the kernel's other areas where
// they fit the CU's 160 KiB beside the N x N table, and in the clip's workspace (L2-resident) where they do not: hist_in_lds().  At 141
// symbols every D <= 32 fits; at the cap of 192 symbols only D = 1 does.  Never in scratch: the ring is addressed memory, not a register
// array under a run-time index (profiles/decode_duration_resources.txt).
//
// Backpointers, 16 bits per symbol and frame as wfl_decode_bigram's: bits 0 .. 7 the winning predecessor symbol of In_q(t), bits 8 .. 13
// end_q(t)'s winning duration 1 .. D, D + 1 for Y, bit 14 Y's choice (stay | enter); O keeps its predecessor and bit 15 (opened | stayed).
// Backtrace: thread 0 over windows of BIGRAM_W frames staged into the LDS the table no longer needs.  From "frame t ends a run of q with
// duration j" it knows the next j frames without another look; for a tail it follows Y's bits to the entering frame, then D frames.  The
// predecessor is read at the run's B frame.
#include "bigram_sumproduct.h"

namespace {

using lattice::MAX_CLASSES;

using bio::NO_CLASS;
using DurClip = bio::Clip;

using bigram_sp::JT;
using bigram_sp::MAX_SYMBOLS;
using bigram_sp::NT;
using bigram_sp::NW;
constexpr int G = 8;                         // frames per emission group
constexpr int BIGRAM_W = 32;                 // backtrace window, frames
constexpr int MAX_D = 32;                    // the table's longest explicit duration, frames
constexpr int JU = 8;                        // ring entries of a symbol in flight together
constexpr int LDS_CAP = 160 * 1024;
static_assert(MAX_SYMBOLS <= 256, "8-bit predecessors");
static_assert(MAX_D + 1 < 64, "6-bit durations");

struct DurationLaunch : bio::Launch {
  const float* trans;    // [N][N], rows the previous symbol
  const int* sym_dur;    // [n_pairs] row of `dur`, -1 none
  const float* dur;      // [n_rows][D + 1]
  int n_rows, D;
  int* ids;
  float* score;
};

// dynamic LDS, in bytes: [table N N floats, later the backtrace window] [partial values NW x MAX_SYMBOLS] [partial predecessors, same]
// [end MAX_SYMBOLS] [B class, I class per symbol] [the ring and the symbols' rows of dur, (2 D + 1) HS floats, where they fit]
__host__ __device__ inline int bp_words(int N) { return (N + 1) / 2; }
__host__ __device__ inline int table_bytes(int N) {
  const int t = N * N * 4, w = BIGRAM_W * bp_words(N) * 4;
  return ((t > w ? t : w) + 15) / 16 * 16;
}
constexpr int FIXED_BYTES = (2 * NW + 3) * MAX_SYMBOLS * 4;
constexpr int STATIC_BYTES = (MAX_CLASSES + MAX_CLASSES / 32 + BIGRAM_W + 16) * 4;   // the kernel's __shared__ variables, rounded up
constexpr int MAX_DYN_LDS = LDS_CAP - STATIC_BYTES;
static_assert(MAX_SYMBOLS * MAX_SYMBOLS * 4 + FIXED_BYTES <= MAX_DYN_LDS, "LDS of one CU");

__host__ __device__ inline int hist_stride(int N) { return (N + 63) / 64 * 64; }
__host__ __device__ inline long hist_words(int N, int D) { return (long)(2 * D + 1) * hist_stride(N); }
__host__ __device__ inline bool hist_in_lds(int N, int D) { return table_bytes(N) + FIXED_BYTES + hist_words(N, D) * 4 <= MAX_DYN_LDS; }
inline int lds_bytes(int N, int D) { return table_bytes(N) + FIXED_BYTES + (hist_in_lds(N, D) ? (int)hist_words(N, D) * 4 : 0); }

// head of a clip's workspace, in words: the backpointers, 16 bits per symbol and frame, then the ring and the rows where LDS does not
// hold them
struct DurHead {
  int N, D;
  __host__ __device__ long bp(int T) const { return lattice::round64((long)T * bp_words(N)); }
  __host__ __device__ long operator()(int T) const { return bp(T) + (hist_in_lds(N, D) ? 0 : lattice::round64(hist_words(N, D))); }
};

// HL: the ring and the rows are in LDS, else in the clip's workspace
template <bool HL>
__global__ __launch_bounds__(NT) void duration_chain_kernel(DurationLaunch a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];
  __shared__ int wout[BIGRAM_W];
  __shared__ int sh_q, sh_cnt;

  const DurClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = cl.T, C = a.C, o_id = a.o_id, N = a.n_pairs + 1, D = a.D, D1 = a.D + 1;
  const int NPW = bp_words(N), NP2 = 2 * NPW;   // backpointer words / 16-bit records per frame
  const int HS = hist_stride(N);
  const float NEG = -INFINITY;
  int* ids = a.ids + cl.frame_off;

  float* tab = (float*)lds;
  float* pv = (float*)(lds + table_bytes(N));   // [NW][MAX_SYMBOLS]
  int* pa = (int*)(pv + NW * MAX_SYMBOLS);      // [NW][MAX_SYMBOLS]
  float* endv = (float*)(pa + NW * MAX_SYMBOLS);
  int* symB = (int*)(endv + MAX_SYMBOLS);
  int* symI = symB + MAX_SYMBOLS;

  // ---- the class table: thread p owns phoneme p here (one slot per thread); a bad one is status 4
  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, C, o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) {
    if (tid == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }
  // thread q >= 1 owns phoneme q - 1 from here on; its row of dur, outside -1 .. n_rows - 1: status 4
  const bool owner = tid < N;
  int row = -1;
  if (owner && tid > 0) row = a.sym_dur[tid - 1];
  if (__syncthreads_or((row < -1 || row >= a.n_rows) ? 1 : 0)) { bio::refuse<NT>(a, cl, 4); return; }

  if (tid < a.n_pairs) { symB[tid + 1] = cB[0]; symI[tid + 1] = cI[0]; }
  if (tid == 0) { symB[0] = o_id; symI[0] = NO_CLASS; }
  for (int e = tid; e < N * N; e += NT) tab[e] = e == 0 ? NEG : a.trans[e];
  if (tid < MAX_SYMBOLS) endv[tid] = tid == 0 ? 0.f : NEG;   // the virtual O frame
  __syncthreads();

  unsigned* bpw = a.ws + cl.ws_off;
  unsigned short* bp = (unsigned short*)bpw;
  const DurHead head{N, D};
  const float* lse = (const float*)(bpw + bio::tail_stat(head(T)));
  const unsigned* forced = bpw + bio::tail_forced(head(T), T);
  const float* Z = a.logits + cl.frame_off * a.ldl;

  // ---- the ring (entry j: h[j HS]) and this symbol's row of dur (L(j): lr[(j - 1) HS], the tail lr[D HS]): the thread's own words
  float* h;
  if constexpr (HL) h = (float*)(lds + table_bytes(N) + FIXED_BYTES) + tid;
  else h = (float*)(bpw + head.bp(T)) + tid;
  float* lr = h + (long)D * HS;
  if (owner) {
    for (int j = 0; j < D; ++j) h[j * HS] = NEG;
    for (int j = 0; j < D1; ++j) lr[j * HS] = row >= 0 ? a.dur[(long)row * D1 + j] : 0.f;
  }

  // ---- thread q < N owns symbol q: d0 = d[O] (q = 0); Y, the ring and end for a phoneme
  const int myB = owner ? symB[tid] : o_id, myI = owner ? symI[tid] : NO_CLASS;
  const bool hasI = myI != NO_CLASS;
  const int col0 = myB, col1 = hasI ? myI : o_id;  // (a state that does not exist reads O's column and is masked to -inf)
  float d0 = 0.f, Y = NEG;

  float z0[G], z1[G];
  unsigned fc[G];
  auto load_group = [&](int t0, float (&o0)[G], float (&o1)[G], unsigned (&of)[G]) {
#pragma unroll
    for (int f = 0; f < G; ++f) {
      const int t = min(t0 + f, T - 1);          // (the tail of the last group re-reads the last row; it is never used)
      const float* z = Z + (long)t * a.ldl;
      o0[f] = z[col0];
      o1[f] = z[col1];
      of[f] = forced[t];
    }
  };
  load_group(0, z0, z1, fc);

  // this thread's predecessor slice and targets
  const int NS = (N + NW - 1) / NW;
  const int s_lo = min(wv * NS, N), s_hi = min(s_lo + NS, N);
  int tq[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) tq[j] = min(lane + 64 * j, N - 1);   // (a lane past N repeats the last target; nobody reads its partial)
  const int nj = (N + 63) / 64;
  double acc = 0.0;                               // what the renormalisations subtracted (the same in every thread)
  int p = 0;                                      // t mod D

  for (int t0 = 0; t0 < T; t0 += G) {
    float n0[G], n1[G];
    unsigned nf[G];
    if (t0 + G < T) load_group(t0 + G, n0, n1, nf);
#pragma unroll
    for (int f = 0; f < G; ++f) {
      const int t = t0 + f;
      if (t < T) {                                // (uniform)
        float sub = 0.f;
        if ((t & 15) == 0 && t > 0) {             // every wave finds the same maximum of end[]; O is finite on every frame, so it is
          float m = NEG;
#pragma unroll
          for (int j = 0; j < JT; ++j) m = fmaxf(m, endv[tq[j]]);
          sub = lattice::wave_max(m);
          acc += (double)sub;
          d0 -= sub;
          Y -= sub;                               // (the ring's entries lose it where they are read, below)
        }
        // partial maxima over this wave's predecessors
        float bv[JT];
        int ba[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) { bv[j] = NEG; ba[j] = s_lo; }
#pragma unroll 4
        for (int s = s_lo; s < s_hi; ++s) {
          const float e = endv[s] - sub;
          const float* trow = tab + s * N;
#pragma unroll
          for (int j = 0; j < JT; ++j) {
            if (j < nj) {                         // (uniform)
              const float v = e + trow[tq[j]];
              if (v > bv[j]) { bv[j] = v; ba[j] = s; }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < JT; ++j) {
          if (j < nj) { pv[wv * MAX_SYMBOLS + tq[j]] = bv[j]; pa[wv * MAX_SYMBOLS + tq[j]] = ba[j]; }
        }
        __syncthreads();
        if (owner) {
          float in = pv[tid];
          int arg = pa[tid];
#pragma unroll
          for (int w = 1; w < NW; ++w) {
            const float v = pv[w * MAX_SYMBOLS + tid];
            if (v > in) { in = v; arg = pa[w * MAX_SYMBOLS + tid]; }
          }
          const bool frc = fc[f] != 0;
          unsigned rec = (unsigned)arg;
          if (tid == 0) {
            const bool obit = !(d0 >= in);
            d0 = z0[f] + (obit ? in : d0);
            rec |= obit ? 1u << 15 : 0u;
            endv[0] = d0;
          } else {
            const float zb = frc ? NEG : z0[f];
            const float zi = (frc || !hasI) ? NEG : z1[f];
            // Y: stay, or enter from the run that is D frames old (the ring entry this frame's opening replaces)
            const float old = h[p * HS] - sub;
            const float yc = old + lr[(D - 1) * HS];
            float ym = Y;
            if (yc > ym) { ym = yc; rec |= 1u << 14; }
            Y = (ym + zi) + lr[D * HS];
            const float r1 = in + zb;
            h[p * HS] = r1;
            float x = r1 + lr[0];
            unsigned dw = 1;
            // the runs that began at t - j + 1, j = 2 .. D, JU at a time and without a branch: the ring entries and the row's entries of
            // a group are loaded before any of the group is stored, so the loads are in flight together.  A j past D reads and rewrites
            // the entry just written, and its candidate is -inf.
            for (int j0 = 2; j0 <= D; j0 += JU) {
              float hv[JU], lv[JU];
#pragma unroll
              for (int u = 0; u < JU; ++u) {
                const int j = min(j0 + u, D);
                int q = p - (j - 1);
                q = q < 0 ? q + D : q;
                q = j0 + u <= D ? q : p;
                hv[u] = h[q * HS];
                lv[u] = lr[(j - 1) * HS];
              }
#pragma unroll
              for (int u = 0; u < JU; ++u) {
                const int j = min(j0 + u, D);
                const bool inside = j0 + u <= D;
                int q = p - (j - 1);
                q = q < 0 ? q + D : q;
                q = inside ? q : p;
                const float v = inside ? (hv[u] - sub) + zi : r1;
                h[q * HS] = v;
                const float cand = inside ? v + lv[u] : NEG;
                if (cand > x) { x = cand; dw = (unsigned)j; }
              }
            }
            if (Y > x) { x = Y; dw = (unsigned)D1; }
            rec |= dw << 8;
            endv[tid] = x;
          }
          bp[(long)t * NP2 + tid] = (unsigned short)rec;
        }
        p = p + 1 == D ? 0 : p + 1;
        __syncthreads();
      }
    }
    if (t0 + G < T) {
#pragma unroll
      for (int f = 0; f < G; ++f) { z0[f] = n0[f]; z1[f] = n1[f]; fc[f] = nf[f]; }
    }
  }

  // ---- the end state: the best symbol of the last frame, the lowest on a tie; its last frame ends a run
  __threadfence_block();
  __syncthreads();                               // also: the backpointers are read back below, and the table is no longer needed
  float best = endv[0];
  int q = 0;
  for (int s = 1; s < N; ++s)
    if (endv[s] > best) { best = endv[s]; q = s; }
  int cnt = 0;
  __syncthreads();

  // ---- backtrace, BIGRAM_W frames per window.  Thread 0's walker: symbol q, and for a phoneme cnt = 0 frame t is the last frame of a
  // run, not yet read | -1 frame t is a tail frame (Y) | j >= 1 frame t and the j - 1 before it are the rest of a run, the last of them B-q
  unsigned* win = (unsigned*)lds;
  const unsigned short* win16 = (const unsigned short*)lds;
  for (int thi = T - 1; thi >= 0;) {
    const int tlo = max(0, thi - BIGRAM_W + 1);
    const int nfr = thi - tlo + 1;
    for (int e = tid; e < nfr * NPW; e += NT) win[e] = bpw[(long)tlo * NPW + e];
    __syncthreads();
    if (tid == 0) {
      for (int t = thi; t >= tlo; --t) {
        const unsigned r = win16[(t - tlo) * NP2 + q];
        int s = -1;                               // the symbol the run was opened from; -1: the path stays inside its symbol
        if (q == 0) {
          wout[t - tlo] = o_id;
          if ((r >> 15) & 1u) s = (int)(r & 0xffu);
        } else {
          if (cnt == 0) {                         // the run that ends here: j <= D frames, or a tail
            const int dw = (int)((r >> 8) & 63u);
            cnt = dw > D ? -1 : max(dw, 1);
          }
          if (cnt == -1) {                        // a tail frame: Y stayed, or it was entered from the D frames before
            wout[t - tlo] = symI[q];
            if ((r >> 14) & 1u) cnt = D;
          } else if (cnt > 1) {
            wout[t - tlo] = symI[q];
            --cnt;
          } else {                                // B-q: the run was opened from the record's predecessor
            wout[t - tlo] = symB[q];
            s = (int)(r & 0xffu);
          }
        }
        if (s >= 0) {
          q = s < N ? s : 0;
          cnt = 0;
        }
      }
      sh_q = q;
      sh_cnt = cnt;
    }
    __syncthreads();
    q = sh_q;
    cnt = sh_cnt;
    if (tid < nfr) ids[tlo + tid] = wout[tid];
    __syncthreads();
    thi = tlo - 1;
  }

  // ---- the score: the objective minus the frames' log-sum-exp
  if (wv == 0) {
    double ls = 0.0;
    for (int t = lane; t < T; t += 64) ls += (double)lse[t];
    ls = lattice::wave_sum(ls);
    if (lane == 0) {
      a.score[cl.clip] = (float)((double)best + acc - ls);
      a.status[cl.clip] = 0;
    }
  }
}

}  // namespace

extern "C" {

int64_t wfl_decode_duration_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs, int32_t D) {
  if (D < 1 || D > MAX_D) return -1;
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, n_pairs + 1 > MAX_SYMBOLS, DurHead{n_pairs + 1, D});
}

int32_t wfl_decode_duration(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                            const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, const float* trans,
                            const int32_t* sym_dur, const float* dur, int32_t n_rows, int32_t D, float threshold, void* workspace,
                            int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status, void* stream) {
  const char* fn = "wfl_decode_duration";
  if (D < 1 || D > MAX_D) return lattice::fail(fn, -1, "D must be 1 .. 32");
  if (n_rows < 0) return lattice::fail(fn, -1, "n_rows < 0");
  if (n_rows > 0 && !dur) return lattice::fail(fn, -1, "null dur with n_rows > 0");
  bool any_frame;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!score || !status || (n_pairs > 0 && !pairs) || (any_frame && (!logits || !ids))) return lattice::fail(fn, -1, "null device pointer");
  if (any_frame && n_pairs > 0 && !sym_dur) return lattice::fail(fn, -1, "null sym_dur");
  // over the symbol cap: status 2, as over the class cap; the table is read only when the clips are searched
  const int N = n_pairs + 1;
  bool over;
  if (bigram_sp::table_missing(trans, any_frame, C, n_pairs, over)) return lattice::fail(fn, -1, "null device pointer");
  auto a = bio::launch_of<DurationLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.trans = trans; a.sym_dur = sym_dur; a.dur = dur; a.n_rows = n_rows; a.D = D; a.ids = ids; a.score = score;
  return bio::run<true>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, DurHead{N, D},
                        [&](const DurationLaunch& a, hipStream_t s) {
                          if (hist_in_lds(N, D)) {
                            if (const int rc = lattice::reserve_lds<duration_chain_kernel<true>, MAX_DYN_LDS>(fn)) return rc;
                            hipLaunchKernelGGL(duration_chain_kernel<true>, dim3(a.n), dim3(NT), lds_bytes(N, D), s, a);
                          } else {
                            if (const int rc = lattice::reserve_lds<duration_chain_kernel<false>, MAX_DYN_LDS>(fn)) return rc;
                            hipLaunchKernelGGL(duration_chain_kernel<false>, dim3(a.n), dim3(NT), lds_bytes(N, D), s, a);
                          }
                          return 0;
                        });
}

}  // extern "C"
