// The BIO grammar over the classes themselves, as wfl_decode (csrc/decode.hip, the max-product search) and wfl_decode_posterior
// (csrc/decode_posterior.hip, the sum-product sweeps) see it, defined ONCE: a change made here reaches both kernels, so the posterior
// always scores a path of the grammar the search ran on.
//
//   device  the per-clip record, a frame's row maximum / sum of exponentials and its forced-to-O rule (the pre-pass arithmetic), the
//           class table in LDS and registers with its validation (status 4)
//   host    the slot configuration by n_pairs, the argument checks the two ABI entries share, the status a whole call is refused with
//
// From csrc/lattice.h (the alignment kernels' header) come the class cap, the clips-per-launch constant, round64, wave_sum and the
// host's clip-table batching and workspace check.
#pragma once
#include "lattice.h"

namespace bio {

using lattice::MAX_CLASSES;

constexpr int NO_CLASS = 0x7fffffff;

struct Clip {
  long frame_off;  // first logits row of the clip
  long ws_off;     // the clip's words in the workspace
  int T, clip;
};

// slots per lane: lane l owns the phonemes l, l + 64, ...; 0: more phonemes than the class cap allows
inline int slots_of(int n_pairs) {
  for (int s = 2; s <= 16; s *= 2)
    if (n_pairs <= 64 * s) return s;
  return 0;
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

// ---- the class table of a one-wave workgroup: every class at most once, all inside [0, C).  Fills info[] (LDS, MAX_CLASSES ints:
// class -> pair | kind << 16, kind 0 O, 1 B, 2 I; -1 never chosen) and this lane's clsB[] / clsI[] (NO_CLASS: no such state); `used`:
// MAX_CLASSES / 32 LDS words.  -> true (in every lane) when the table is bad: status 4.
template <int S>
static __device__ __forceinline__ bool class_table(const int* pairs, int n_pairs, int C, int o_id, unsigned* used, int* info, int (&clsB)[S],
                                                   int (&clsI)[S]) {
  const int lane = threadIdx.x;
  if (lane < MAX_CLASSES / 32) used[lane] = 0;
  for (int c = lane; c < MAX_CLASSES; c += 64) info[c] = -1;
  __syncthreads();
  if (lane == 0) { used[o_id >> 5] = 1u << (o_id & 31); info[o_id] = 0; }
  __syncthreads();
  bool bad = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int p = lane + 64 * s;
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
  return __any(bad);
}

// =================================================================================================================== host side
// the status every clip of a call gets without a search: 2 over the class cap, 4 more pairs than classes (then one is used twice or out
// of range); 0: the clips are searched
inline int refused_status(int C, int n_pairs) { return C > MAX_CLASSES ? 2 : (n_pairs > C ? 4 : 0); }

// the arguments wfl_decode and wfl_decode_posterior share -> 0 or the error.  any_frame comes back for the caller's check of its
// device pointers (only when n_clips > 0).
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

}  // namespace bio
