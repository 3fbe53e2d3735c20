// The BIO grammar over the classes themselves, as the five decode entries see it -- wfl_decode (csrc/decode.hip, the max-product search
// under a flat penalty), wfl_decode_bigram (csrc/decode_bigram.hip, the same search under a phone-bigram table), wfl_decode_posterior
// (csrc/decode_posterior.hip, the sum-product sweeps under the flat penalty) and wfl_decode_bigram_posterior
// (csrc/decode_bigram_posterior.hip, the sum-product sweeps under the table); wfl_decode_bigram_counts (csrc/decode_bigram_counts.hip, the
// same sweeps summed into expected successions) is the fifth; wfl_decode_duration (csrc/decode_duration.hip, the bigram search with a
// duration prior per phoneme) and wfl_decode_duration_posterior (csrc/decode_duration_posterior.hip, the sum-product sweeps under that
// prior) use the same pieces as they are -- defined ONCE: a change made here reaches all of them, so a
// posterior always scores the grammar and the forced frames its search ran on.  A .hip file keeps its chain kernel, the head of its workspace and its
// own fields of the launch struct; everything else of an entry is here, but for what only some entries share: the path posteriors'
// csrc/path_posterior.h and the bigram sum-product chain's csrc/bigram_sumproduct.h.
//
//   device  the per-clip record and the launch fields every kernel takes, a clip's workspace ([the kernel's head] [a statistic per
//           frame] [a forced flag per frame]), a frame's row maximum / sum of exponentials and its forced-to-O rule, the ONE pre-pass
//           kernel that writes them, what a refused clip looks like (per output shape) and the ONE fill kernel, the class table in LDS
//           and registers with its validation (status 4), the logZ tail of the three sum-product kernels
//   host    the slot configurations by n_pairs and their dispatch, the launch struct's common fields (launch_of), the argument checks
//           the ABI entries share, the status a whole call is refused with, the *_workspace_bytes rule, and the driver of an entry
//           after its own pointer checks: workspace check, clip records, fill or pre-pass + chain launches
//
// From csrc/lattice.h (the alignment kernels' header) come the class cap, the clips-per-launch constant, round64, the wave reductions
// and the host's clip-table batching, workspace check, error strings and once-per-device LDS reservation.
#pragma once
#include "lattice.h"

namespace bio {

using lattice::CLIPS_PER_LAUNCH;
using lattice::MAX_CLASSES;
using lattice::round64;

constexpr int NO_CLASS = 0x7fffffff;

struct Clip {
  long frame_off;  // first logits row of the clip
  long ws_off;     // the clip's words in the workspace
  int T, clip;
};

// what the kernels of all five entries take; an entry's launch struct is this plus its own fields, passed by value
struct Launch {
  const float* logits;
  long ldl;
  int C, o_id;
  const int* pairs;  // [n_pairs][2]: B class, I class or -1
  int n_pairs;
  float threshold;
  unsigned* ws;
  int* status;
  int n, fill_status;
  Clip clip[CLIPS_PER_LAUNCH];
};

// (host) an entry's launch struct L with the fields the ABI hands every entry; ws, fill_status and the clips are run()'s
template <class L>
L launch_of(const float* logits, long ldl, int C, int o_id, const int* pairs, int n_pairs, float threshold, int* status) {
  L a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.pairs = pairs; a.n_pairs = n_pairs; a.threshold = threshold; a.status = status;
  return a;
}

// ---- workspace of a clip, in words: [head: the kernel's own, `head` words, a multiple of 64] [a float per frame: its log-sum-exp or
// its row maximum] [forced flag per frame], the last two rounded up to 64 words.  tail_stat / tail_forced: where the last two begin
__host__ __device__ inline long tail_stat(long head) { return head; }
__host__ __device__ inline long tail_forced(long head, int T) { return head + round64(T); }
inline long clip_words(long head, int T) { return T > 0 ? tail_forced(head, T) + round64(T) : 0; }

// ---- the wave-per-clip kernels' configurations: S slots per lane (lane l owns the phonemes l, l + 64, ...), D frames per group of
// emissions in flight.  slots_of -> S, 0: more phonemes than the class cap allows
inline int slots_of(int n_pairs) {
  for (int s = 2; s <= 16; s *= 2)
    if (n_pairs <= 64 * s) return s;
  return 0;
}

template <int S_, int D_>
struct Slots {
  static constexpr int S = S_, D = D_;
};

// f(Slots<S, D>()) of the configuration with S slots
template <class F>
auto dispatch_slots(int S, F&& f) {
  switch (S) {
    case 2: return f(Slots<2, 16>());
    case 4: return f(Slots<4, 8>());
    case 8: return f(Slots<8, 4>());
    default: return f(Slots<16, 2>());
  }
}

// ---- a frame's statistics, by one wave (every lane gets both): m = the row's maximum, se = sum_c exp(z[c] - m).
// log-sum-exp = m + logf(se); the largest softmax probability = exp(m - lse) = 1 / se.
static __device__ __forceinline__ void frame_stats(const float* z, int C, int lane, float& m, float& se) {
  m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(z[c] - m);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o);
}

// a frame whose largest softmax probability is below the threshold can only be O
static __device__ __forceinline__ unsigned forced_to_o(float se, float threshold) {
  return (threshold > 0.f && 1.f / se < threshold) ? 1u : 0u;
}

// ---- the pre-pass: per frame its statistic (LSE: the log-sum-exp, else the row maximum) and its forced-to-O flag, behind the head
// head(T) of the clip's workspace.  grid (ceil(max T / 4), clips), 4 waves per block, one wave per frame.
template <class L, class Head, bool LSE>
__global__ __launch_bounds__(256) void pre_kernel(L a, Head head) {
  const Clip cl = a.clip[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= cl.T) return;
  const float* z = a.logits + (cl.frame_off + t) * a.ldl;
  float m, se;
  frame_stats(z, a.C, lane, m, se);
  if (lane == 0) {
    unsigned* w = a.ws + cl.ws_off;
    ((float*)(w + tail_stat(head(cl.T))))[t] = LSE ? m + logf(se) : m;
    w[tail_forced(head(cl.T), cl.T) + t] = forced_to_o(se, a.threshold);
  }
}

// ---- the end of a sum-product kernel, by one wave: logZ = log of the scaled sum, its exponent KA, and what the emissions left out (the
// row maxima; O's logit on a forced frame); status 0
template <class L>
static __device__ __forceinline__ void write_logz(const L& a, const Clip& cl, int lane, const float* Z, const float* rowmax,
                                                  const unsigned* forced, double zsum, long KA) {
  double ls = 0.0;
  for (int t = lane; t < cl.T; t += 64) ls += forced[t] ? (double)Z[(long)t * a.ldl + a.o_id] : (double)rowmax[t];
  ls = lattice::wave_sum(ls);
  if (lane == 0) {
    a.logz[cl.clip] = (float)(log(zsum) + (double)KA * 0.69314718055994530942 + ls);
    a.status[cl.clip] = 0;
  }
}

// ---- what a clip that is not searched / scored looks like, written by a block of NT threads; the shape is chosen by the outputs the
// launch struct has.  A search (ids, score): O everywhere, score 0.  A posterior (logz, post, cls_post): zeros.  Expected successions
// (logz, counts [clips][N][N]): logz 0 and an all-zero table.  Expected run lengths: below.
template <int NT, class L>
static __device__ __forceinline__ auto refuse(const L& a, const Clip& cl, int status) -> decltype((void)a.score) {
  int* ids = a.ids + cl.frame_off;
  for (int t = threadIdx.x; t < cl.T; t += NT) ids[t] = a.o_id;
  if (threadIdx.x == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = status; }
}

template <int NT, class L>
static __device__ __forceinline__ auto refuse(const L& a, const Clip& cl, int status) -> decltype((void)a.post) {
  for (int t = threadIdx.x; t < cl.T; t += NT) a.post[cl.frame_off + t] = a.cls_post[cl.frame_off + t] = 0.f;
  if (threadIdx.x == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = status; }
}

template <int NT, class L>
static __device__ __forceinline__ auto refuse(const L& a, const Clip& cl, int status) -> decltype((void)a.counts) {
  const long nn = (long)(a.n_pairs + 1) * (a.n_pairs + 1);
  float* c = a.counts + cl.clip * nn;
  for (long e = threadIdx.x; e < nn; e += NT) c[e] = 0.f;
  if (threadIdx.x == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = status; }
}

// expected run lengths (logz, succ [clips][N][N], dur_counts [clips][n_pairs][D + 1]): logz 0 and two all-zero tables
template <int NT, class L>
static __device__ __forceinline__ auto refuse(const L& a, const Clip& cl, int status) -> decltype((void)a.dur_counts) {
  const long nn = (long)(a.n_pairs + 1) * (a.n_pairs + 1), nd = (long)a.n_pairs * (a.D + 1);
  float* c = a.succ + cl.clip * nn;
  float* d = a.dur_counts + cl.clip * nd;
  for (long e = threadIdx.x; e < nn; e += NT) c[e] = 0.f;
  for (long e = threadIdx.x; e < nd; e += NT) d[e] = 0.f;
  if (threadIdx.x == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = status; }
}

// the clips of a call that is refused as a whole (refused_status): one wave per clip
template <class L>
__global__ __launch_bounds__(64) void fill_kernel(L a) {
  refuse<64>(a, a.clip[blockIdx.x], a.fill_status);
}

// ---- the class table, by a workgroup of NT threads: every class at most once, all inside [0, C).  Thread i owns the phonemes i,
// i + NT, ... (S slots).  Fills info[] (LDS, MAX_CLASSES ints: class -> pair | kind << 16, kind 0 O, 1 B, 2 I; -1 never chosen) and this
// thread's clsB[] / clsI[] (NO_CLASS: no such state); `used`: MAX_CLASSES / 32 LDS words.  -> true, in every thread of the block, when
// the table is bad: status 4.
template <int S, int NT>
static __device__ __forceinline__ bool class_table(const int* pairs, int n_pairs, int C, int o_id, unsigned* used, int* info, int (&clsB)[S],
                                                   int (&clsI)[S]) {
  const int tid = threadIdx.x;
  if (tid < MAX_CLASSES / 32) used[tid] = 0;
  for (int c = tid; c < MAX_CLASSES; c += NT) info[c] = -1;
  __syncthreads();
  if (tid == 0) { used[o_id >> 5] = 1u << (o_id & 31); info[o_id] = 0; }
  __syncthreads();
  bool bad = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int p = tid + NT * s;
    clsB[s] = clsI[s] = NO_CLASS;
    if (p < n_pairs) {
      const int b = pairs[2 * p], i = pairs[2 * p + 1];
      if (b < 0 || b >= C) bad = true;
      else if (atomicOr(&used[b >> 5], 1u << (b & 31)) & (1u << (b & 31))) bad = true;
      else { clsB[s] = b; info[b] = p | (1 << 16); }
      if (i != -1) {
        if (i < 0 || i >= C) bad = true;
        else if (atomicOr(&used[i >> 5], 1u << (i & 31)) & (1u << (i & 31))) bad = true;
        else { clsI[s] = i; info[i] = p | (2 << 16); }
      }
    }
  }
  __syncthreads();
  if constexpr (NT == 64) return __any(bad);   // (one wave)
  else return __syncthreads_or(bad ? 1 : 0) != 0;
}

// =================================================================================================================== host side
// the status every clip of a call gets without a search: 2 over the class cap, 4 more pairs than classes (then one is used twice or out
// of range), 2 over a cap of the entry's own; 0: the clips are searched
inline int refused_status(int C, int n_pairs, bool over_own_cap = false) {
  return C > MAX_CLASSES ? 2 : (n_pairs > C ? 4 : (over_own_cap ? 2 : 0));
}

// the arguments the five entries share -> 0 or the error.  any_frame comes back for the caller's check of its device pointers (only
// when n_clips > 0).
inline int check_args(const char* fn, int C, int o_id, int64_t ldl, const int64_t* frame_off_host, const int32_t* n_frames_host, int n_clips,
                      int n_pairs, float lambda, float threshold, bool& any_frame) {
  any_frame = false;
  if (C < 1) return lattice::fail(fn, -1, "C < 1");
  if (o_id < 0 || o_id >= C) return lattice::fail(fn, -1, "o_id out of range");
  if (ldl < C) return lattice::fail(fn, -1, "ldl < C");
  if (n_clips < 0 || n_pairs < 0) return lattice::fail(fn, -1, "negative count");
  if (!(lambda >= 0.f) || !(threshold >= 0.f)) return lattice::fail(fn, -1, "lambda and threshold must be >= 0");
  if (n_clips == 0) return 0;
  if (!frame_off_host || !n_frames_host) return lattice::fail(fn, -1, "null host array");
  for (int b = 0; b < n_clips; ++b) {
    if (frame_off_host[b] < 0 || n_frames_host[b] < 0) return lattice::fail(fn, -1, "negative offset or frame count");
    any_frame |= n_frames_host[b] > 0;
  }
  return 0;
}

// what a *_workspace_bytes entry returns: head(T) the entry's head words of a clip; nothing_searched: n_pairs is over a cap, the call
// will be refused and needs no workspace.  -1: a null array or a negative count
template <class Head>
int64_t workspace_bytes(const int32_t* n_frames_host, int n_clips, int n_pairs, bool nothing_searched, Head head) {
  if (n_clips < 0 || n_pairs < 0 || (n_clips > 0 && !n_frames_host)) return -1;
  int64_t words = 0;
  for (int b = 0; b < n_clips; ++b) {
    if (n_frames_host[b] < 0) return -1;
    if (!nothing_searched) words += clip_words(head(n_frames_host[b]), n_frames_host[b]);
  }
  return words * 4;
}

// An entry from its own pointer checks on (check_args has passed, n_clips > 0).  `a` holds everything but ws, fill_status and the
// clips.  A refused call (refused_status; over_own_cap: a cap of the entry's own) fills its clips; otherwise the workspace is checked
// and every launch of at most CLIPS_PER_LAUNCH clips is the pre-pass (LSE: see pre_kernel) and chain(a, stream) -> 0 or the error,
// the entry's chain kernel.
template <bool LSE, class L, class Head, class Chain>
int run(const char* fn, L& a, bool over_own_cap, const int64_t* frame_off_host, const int32_t* n_frames_host, int n_clips, void* workspace,
        int64_t workspace_bytes_given, void* stream, Head head, Chain chain) {
  const int fill = refused_status(a.C, a.n_pairs, over_own_cap);
  const int64_t need = fill ? 0 : workspace_bytes(n_frames_host, n_clips, a.n_pairs, false, head);
  if (const int rc = lattice::check_workspace(fn, need, workspace, workspace_bytes_given)) return rc;
  hipStream_t s = (hipStream_t)stream;
  a.ws = (unsigned*)workspace;
  a.fill_status = fill;
  return lattice::launch_clips<1>(           // one group: the clips in their order
      a, n_clips,
      [&](int b, long off, Clip& c, int&) {
        c = Clip{(long)frame_off_host[b], off, n_frames_host[b], b};
        return fill ? 0 : clip_words(head(c.T), c.T);
      },
      [&](int, const L& a) {
        if (fill) {
          hipLaunchKernelGGL(fill_kernel<L>, dim3(a.n), dim3(64), 0, s, a);
        } else {
          int max_t = 0;
          for (int j = 0; j < a.n; ++j) max_t = std::max(max_t, a.clip[j].T);
          if (max_t > 0) {
            hipLaunchKernelGGL((pre_kernel<L, Head, LSE>), dim3((max_t + 3) / 4, a.n), dim3(256), 0, s, a, head);
            if (hipGetLastError() != hipSuccess) return lattice::fail(fn, -3, "launch failed");
          }
          if (const int rc = chain(a, s)) return rc;
        }
        return hipGetLastError() == hipSuccess ? 0 : lattice::fail(fn, -3, "launch failed");
      });
}

}  // namespace bio
