// BIO-grammar Viterbi decode with a phone-bigram prior (wfl_decode_bigram, include/wfl_asr.h): wfl_decode's states, legality rule, forced
// frames and virtual O frame, but every opened run costs W[previous symbol][opened symbol] instead of one flat lambda.  Symbols: 0 is O,
// 1 + p is phoneme p of `pairs`; N = n_pairs + 1 <= MAX_SYMBOLS.  With end[O] = d[O], end[p] = max(d[B-p], d[I-p]) of the previous frame:
//     B-q : z + max_s (end[s] + W[s][q])      O : z + max(d[O], max_{p != O} (end[p] + W[p][O]))      I-q : z + max(d[I-q], d[B-q])
// so a frame is a max-plus product of the N x N table with end[]: decode_chain_kernel's one wave-wide maximum does not carry over.
//
// Two kernels.  bio::pre_kernel: the frames' log-sum-exp and forced-to-O flags (csrc/bio_grammar.h, as everything this entry shares with
// wfl_decode and wfl_decode_posterior; this file holds the chain kernel, its backpointer words and LDS layout, and the entry's own
// checks).  bigram_chain_kernel, ONE WORKGROUP of 256 threads per clip:
//   - the table lives in LDS for the whole clip (N N floats, 144 KiB at the cap), row = previous symbol, so the 64 lanes of a wave read
//     consecutive words of one row: no bank conflict; W[O][O] is stored as -inf (O after O costs nothing and is decided apart)
//   - wave w takes the predecessors [w NS, (w + 1) NS), NS = ceil(N / 4); lane l the targets l, l + 64, l + 128.  Ascending s and a strict
//     compare: the lowest predecessor wins a tie.  The four partial (value, predecessor) per target go through LDS, one barrier
//   - thread q < N owns symbol q: both states in registers, combines the four partials in slice order, updates, stores the frame's
//     backpointer (predecessor symbol | I bit << 8 | O bit << 9, 16 bits) and publishes end[q] for the next frame, second barrier
//   - the owner's emissions are gathered one group of D frames ahead into registers; no transcendental sits on the chain
//   - every 16 frames the maximum of end[] is subtracted from all states and carried in a double (wfl_decode's scheme)
// Backtrace: thread 0 walks windows of BIGRAM_W frames of backpointers staged into the LDS the table no longer needs.  The state a
// run was opened from is the better of the predecessor symbol's two states; that is the I bit of the same frame's record.
#include "bigram_sumproduct.h"

namespace {

using lattice::MAX_CLASSES;

using bio::NO_CLASS;
using BigramClip = bio::Clip;

// the workgroup's shape is the sum-product chain's (csrc/bigram_sumproduct.h): NT threads per clip, NW predecessor slices, JT targets per lane
using bigram_sp::JT;
using bigram_sp::MAX_SYMBOLS;
using bigram_sp::NT;
using bigram_sp::NW;
constexpr int D = 8;                         // frames per emission group
constexpr int BIGRAM_W = 32;                 // backtrace window, frames
static_assert(MAX_SYMBOLS <= 256, "8-bit predecessors");

struct BigramLaunch : bio::Launch {
  const float* trans;  // [N][N], rows the previous symbol
  int* ids;
  float* score;
};

// head of a clip's workspace, in words: the backpointers, 16 bits per symbol and frame
__host__ __device__ inline int bp_words(int N) { return (N + 1) / 2; }
struct BpWords {
  int N;
  __host__ __device__ long operator()(int T) const { return lattice::round64((long)T * bp_words(N)); }
};

// dynamic LDS, in bytes: [table N N floats, later the backtrace window] [partial values NW x MAX_SYMBOLS] [partial predecessors, same]
// [end MAX_SYMBOLS] [B class, I class per symbol]
__host__ __device__ inline int table_bytes(int N) {
  const int t = N * N * 4, w = BIGRAM_W * bp_words(N) * 4;
  return ((t > w ? t : w) + 15) / 16 * 16;
}
constexpr int FIXED_BYTES = (2 * NW + 3) * MAX_SYMBOLS * 4;
inline int lds_bytes(int N) { return table_bytes(N) + FIXED_BYTES; }
constexpr int MAX_LDS = (MAX_SYMBOLS * MAX_SYMBOLS + (2 * NW + 3) * MAX_SYMBOLS) * 4;
static_assert(MAX_LDS + (MAX_CLASSES + MAX_CLASSES / 32 + BIGRAM_W + 16) * 4 <= 160 * 1024, "LDS of one CU");

__global__ __launch_bounds__(NT) void bigram_chain_kernel(BigramLaunch a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];
  __shared__ int wout[BIGRAM_W];
  __shared__ int sh_q, sh_i;

  const BigramClip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = cl.T, C = a.C, o_id = a.o_id, N = a.n_pairs + 1;
  const int NPW = bp_words(N), NP2 = 2 * NPW;   // backpointer words / 16-bit records per frame
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
  if (tid < a.n_pairs) { symB[tid + 1] = cB[0]; symI[tid + 1] = cI[0]; }
  if (tid == 0) { symB[0] = o_id; symI[0] = NO_CLASS; }
  for (int e = tid; e < N * N; e += NT) tab[e] = e == 0 ? NEG : a.trans[e];
  if (tid < MAX_SYMBOLS) endv[tid] = tid == 0 ? 0.f : NEG;   // the virtual O frame
  __syncthreads();

  // ---- thread q < N owns symbol q: d0 = d[O] (q = 0) or d[B-q], d1 = d[I-q]
  const bool owner = tid < N;
  const int myB = owner ? symB[tid] : o_id, myI = owner ? symI[tid] : NO_CLASS;
  const bool hasI = myI != NO_CLASS;
  const int col0 = myB, col1 = hasI ? myI : o_id;  // (a state that does not exist reads O's column and is masked to -inf)
  float d0 = tid == 0 ? 0.f : NEG, d1 = NEG;

  unsigned* bpw = a.ws + cl.ws_off;
  unsigned short* bp = (unsigned short*)bpw;
  const float* lse = (const float*)(bpw + bio::tail_stat(BpWords{N}(T)));
  const unsigned* forced = bpw + bio::tail_forced(BpWords{N}(T), T);
  const float* Z = a.logits + cl.frame_off * a.ldl;

  float z0[D], z1[D];
  unsigned fc[D];
  auto load_group = [&](int t0, float (&o0)[D], float (&o1)[D], unsigned (&of)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
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

  for (int t0 = 0; t0 < T; t0 += D) {
    float n0[D], n1[D];
    unsigned nf[D];
    if (t0 + D < T) load_group(t0 + D, n0, n1, nf);
#pragma unroll
    for (int f = 0; f < D; ++f) {
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
          d1 -= sub;
        }
        // partial maxima over this wave's predecessors
        float bv[JT];
        int ba[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) { bv[j] = NEG; ba[j] = s_lo; }
#pragma unroll 4
        for (int s = s_lo; s < s_hi; ++s) {
          const float e = endv[s] - sub;
          const float* row = tab + s * N;
#pragma unroll
          for (int j = 0; j < JT; ++j) {
            if (j < nj) {                         // (uniform)
              const float v = e + row[tq[j]];
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
            rec |= obit ? 1u << 9 : 0u;
            endv[0] = d0;
          } else {
            const bool ibit = !hasI || !(d1 >= d0);
            const float from = ibit ? d0 : d1;
            d1 = from + ((frc || !hasI) ? NEG : z1[f]);
            d0 = in + (frc ? NEG : z0[f]);
            rec |= ibit ? 1u << 8 : 0u;
            endv[tid] = fmaxf(d0, d1);
          }
          bp[(long)t * NP2 + tid] = (unsigned short)rec;
        }
        __syncthreads();
      }
    }
    if (t0 + D < T) {
#pragma unroll
      for (int f = 0; f < D; ++f) { z0[f] = n0[f]; z1[f] = n1[f]; fc[f] = nf[f]; }
    }
  }

  // ---- the end state: the best symbol of the last frame, the lowest on a tie; of its two states I when d[I] >= d[B]
  if (owner) pa[tid] = (hasI && d1 >= d0) ? 1 : 0;
  __threadfence_block();
  __syncthreads();                               // also: the backpointers are read back below, and the table is no longer needed
  float best = endv[0];
  int q = 0;
  for (int s = 1; s < N; ++s)
    if (endv[s] > best) { best = endv[s]; q = s; }
  int isI = q ? pa[q] : 0;
  __syncthreads();

  // ---- backtrace, BIGRAM_W frames per window
  unsigned* win = (unsigned*)lds;
  const unsigned short* win16 = (const unsigned short*)lds;
  for (int thi = T - 1; thi >= 0;) {
    const int tlo = max(0, thi - BIGRAM_W + 1);
    const int nfr = thi - tlo + 1;
    for (int e = tid; e < nfr * NPW; e += NT) win[e] = bpw[(long)tlo * NPW + e];
    __syncthreads();
    if (tid == 0) {
      for (int t = thi; t >= tlo; --t) {
        wout[t - tlo] = q == 0 ? o_id : (isI ? symI[q] : symB[q]);
        const unsigned short* rec = win16 + (t - tlo) * NP2;
        const unsigned r = rec[q];
        int s = -1;                               // the symbol the run was opened from; -1: the state stays inside its symbol
        if (q == 0) {
          if ((r >> 9) & 1u) s = (int)(r & 0xffu);
        } else if (isI) {
          if ((r >> 8) & 1u) isI = 0;
        } else {
          s = (int)(r & 0xffu);
        }
        if (s >= 0) {
          q = s < N ? s : 0;
          isI = q ? !((rec[q] >> 8) & 1u) : 0;
        }
      }
      sh_q = q;
      sh_i = isI;
    }
    __syncthreads();
    q = sh_q;
    isI = sh_i;
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

int64_t wfl_decode_bigram_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs) {
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, n_pairs + 1 > MAX_SYMBOLS, BpWords{n_pairs + 1});
}

int32_t wfl_decode_bigram(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                          const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, const float* trans,
                          float threshold, void* workspace, int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status,
                          void* stream) {
  const char* fn = "wfl_decode_bigram";
  bool any_frame;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!score || !status || (n_pairs > 0 && !pairs) || (any_frame && (!logits || !ids))) return lattice::fail(fn, -1, "null device pointer");
  // over the symbol cap: status 2, as over the class cap; the table is read only when the clips are searched
  const int N = n_pairs + 1;
  const bool over = N > MAX_SYMBOLS;
  if (any_frame && !trans && !bio::refused_status(C, n_pairs, over)) return lattice::fail(fn, -1, "null device pointer");
  auto a = bio::launch_of<BigramLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.trans = trans; a.ids = ids; a.score = score;
  return bio::run<true>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, BpWords{N},
                        [&](const BigramLaunch& a, hipStream_t s) {
                          if (const int rc = lattice::reserve_lds<bigram_chain_kernel, MAX_LDS>(fn)) return rc;
                          hipLaunchKernelGGL(bigram_chain_kernel, dim3(a.n), dim3(NT), lds_bytes(N), s, a);
                          return 0;
                        });
}

}  // extern "C"
