// BIO-grammar Viterbi decode of the frame logits of clips WITHOUT a transcript (wfl_decode, include/wfl_asr.h).
//
// Replaces, when the caller asks for `postprocess.decode: viterbi`, the per-frame argmax + median filter of the reference's free
// decode (infer.py:86-96, 164-174, 293-302): the path is a class per frame in which every I-p directly follows B-p or I-p, and it
// maximises  sum_t z[t][c_t] - lambda * (runs opened).  States are the classes themselves.  With d the previous frame's scores,
// a = argmax d (lowest id on a tie), best = d[a]:
//     O   : z + (d[O] >= best - lambda ? d[O] : best - lambda)        B-p : z + best - lambda
//     I-p : z + (d[I-p] >= d[B-p] ? d[I-p] : d[B-p])
// Frame 0 follows a virtual O frame (d[O] = 0, every other state -inf).  A frame whose largest softmax probability is below the
// threshold can only be O (every other emission is -inf there).
//
// Two kernels.  bio::pre_kernel (csrc/bio_grammar.h), one wave per frame, fully parallel: the frame's log-sum-exp and its forced-to-O
// flag, so no transcendental sits on the serial chain.  decode_chain_kernel, ONE WAVE per clip: lane l owns the phonemes l, l + 64, ... (S slots,
// both states of each in registers), so the I-p update is lane-local, and the only cross-lane work of a frame is one
// max-with-index reduction over the 64 lanes (DPP inside a row of 16, two __shfl_xor across rows); its result feeds O and every B-p.
// There is no LDS exchange and no barrier in the frame loop.  The logits are gathered through the per-lane class ids one group of D
// frames ahead, into registers.  Every 16 frames `best` is subtracted from all states and carried in a double (the scheme of
// align.hip), so the fp32 scores do not grow with T.
// Backpointers: per frame 2 S words of I-p bits (one __ballot per slot), and one word a | (O's bit << 16).  Backtrace: lane 0 walks
// windows of DECODE_W frames that the wave stages into LDS.
// This file holds the chain kernel, its backpointer words (the head of a clip's workspace) and the entry's own pointer checks.
// Everything wfl_decode shares with wfl_decode_bigram and wfl_decode_posterior lives in csrc/bio_grammar.h: the clip record and the
// common launch fields, the workspace tail, the pre-pass and fill kernels, the class table, the slot dispatch, the argument checks and
// the host driver of an entry.
#include "bio_grammar.h"
#include "wfl_asr.h"

namespace {

using lattice::MAX_CLASSES;

using bio::NO_CLASS;
using DecodeClip = bio::Clip;

constexpr int DECODE_W = 32;                 // backtrace window, frames

struct DecodeLaunch : bio::Launch {
  float lambda;
  int* ids;
  float* score;
};

// head of a clip's workspace, in words: the backpointers, 2 S + 1 per frame
struct BpWords {
  int S;
  __host__ __device__ long operator()(int T) const { return lattice::round64((long)T * (2 * S + 1)); }
};

// (value, class) ordered by value, then by the LOWER class id: max-combine of one lane's pair with another's
__device__ __forceinline__ void take_better(float& v, int& c, float ov, int oc) {
  if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
}

template <int CTRL>
__device__ __forceinline__ void dpp_step(float& v, int& c) {
  const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
  const int oc = __builtin_amdgcn_update_dpp(0, c, CTRL, 0xf, 0xf, false);
  take_better(v, c, ov, oc);
}

// every lane gets the wave's best (value, class).  Each step merges two groups that already agree inside themselves.
__device__ __forceinline__ void wave_best(float& v, int& c) {
  dpp_step<0xB1>(v, c);    // quad_perm [1,0,3,2]
  dpp_step<0x4E>(v, c);    // quad_perm [2,3,0,1]
  dpp_step<0x141>(v, c);   // row_half_mirror: the other quad of the 8
  dpp_step<0x140>(v, c);   // row_mirror: the other 8 of the 16
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float ov = __shfl_xor(v, o);
    const int oc = __shfl_xor(c, o);
    take_better(v, c, ov, oc);
  }
}

template <int S, int D>
__global__ __launch_bounds__(64) void decode_chain_kernel(DecodeLaunch a) {
  constexpr int WPF = 2 * S + 1;              // backpointer words per frame
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];    // class -> pair | kind << 16 (kind 0 O, 1 B, 2 I); -1 never chosen
  __shared__ unsigned win[DECODE_W * WPF];
  __shared__ int wout[DECODE_W];
  __shared__ int sh_s;

  const DecodeClip cl = a.clip[blockIdx.x];
  const int lane = threadIdx.x;
  const int T = cl.T, C = a.C, o_id = a.o_id;
  const float NEG = -INFINITY;
  int* ids = a.ids + cl.frame_off;

  // ---- the class table: every class at most once, all inside [0, C)
  int clsB[S], clsI[S];
  if (bio::class_table<S, 64>(a.pairs, a.n_pairs, C, o_id, used, info, clsB, clsI)) { bio::refuse<64>(a, cl, 4); return; }
  if (T == 0) {
    if (lane == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }

  unsigned* bp = a.ws + cl.ws_off;
  const float* lse = (const float*)(bp + bio::tail_stat(BpWords{S}(T)));
  const unsigned* forced = bp + bio::tail_forced(BpWords{S}(T), T);
  const float* Z = a.logits + cl.frame_off * a.ldl;
  int colB[S], colI[S];                        // a state that does not exist reads O's column and is masked to -inf
#pragma unroll
  for (int s = 0; s < S; ++s) {
    colB[s] = clsB[s] != NO_CLASS ? clsB[s] : o_id;
    colI[s] = clsI[s] != NO_CLASS ? clsI[s] : o_id;
  }

  // ---- forward pass: groups of D frames, the next group's logits in flight while this one is computed
  float zb[D][S], zi[D][S], zo[D];
  unsigned fc[D];
  auto load_group = [&](int t0, float (&ob)[D][S], float (&oi)[D][S], float (&oo)[D], unsigned (&of)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = min(t0 + f, T - 1);        // (the tail of the last group re-reads the last row; it is never used)
      const float* z = Z + (long)t * a.ldl;
      oo[f] = z[o_id];
      of[f] = forced[t];
#pragma unroll
      for (int s = 0; s < S; ++s) { ob[f][s] = z[colB[s]]; oi[f][s] = z[colI[s]]; }
    }
  };
  load_group(0, zb, zi, zo, fc);

  float dO = 0.f, dB[S], dI[S];
#pragma unroll
  for (int s = 0; s < S; ++s) dB[s] = dI[s] = NEG;
  double acc = 0.0;                            // what the renormalisations subtracted
  const float lambda = a.lambda;

  for (int t0 = 0; t0 < T; t0 += D) {
    float nb[D][S], ni[D][S], no[D];
    unsigned nf[D];
    if (t0 + D < T) load_group(t0 + D, nb, ni, no, nf);
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = t0 + f;
      if (t < T) {                             // (uniform)
        float bv = NEG;
        int bc = NO_CLASS;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          take_better(bv, bc, dB[s], clsB[s]);
          take_better(bv, bc, dI[s], clsI[s]);
        }
        wave_best(bv, bc);
        take_better(bv, bc, dO, o_id);         // O is finite on every frame, so best is
        if ((t & 15) == 0 && t > 0) {
          acc += (double)bv;
          dO -= bv;
#pragma unroll
          for (int s = 0; s < S; ++s) { dB[s] -= bv; dI[s] -= bv; }
          bv = 0.f;
        }
        const float sw = bv - lambda;
        const bool frc = fc[f] != 0;
        const bool obit = !(dO >= sw);
        dO = zo[f] + (obit ? sw : dO);
        unsigned w = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const bool ibit = !(dI[s] >= dB[s]);
          const float eb = (frc || clsB[s] == NO_CLASS) ? NEG : zb[f][s];
          const float ei = (frc || clsI[s] == NO_CLASS) ? NEG : zi[f][s];
          const float from = ibit ? dB[s] : dI[s];
          dI[s] = from + ei;
          dB[s] = sw + eb;
          const unsigned long long m = __ballot(ibit);
          if (lane == 2 * s) w = (unsigned)m;
          if (lane == 2 * s + 1) w = (unsigned)(m >> 32);
        }
        if (lane == 2 * S) w = (unsigned)bc | (obit ? 1u << 16 : 0u);
        if (lane < WPF) bp[(long)t * WPF + lane] = w;
      }
    }
    if (t0 + D < T) {
#pragma unroll
      for (int f = 0; f < D; ++f) {
        zo[f] = no[f];
        fc[f] = nf[f];
#pragma unroll
        for (int s = 0; s < S; ++s) { zb[f][s] = nb[f][s]; zi[f][s] = ni[f][s]; }
      }
    }
  }

  // ---- the end state: argmax of the last frame, lowest id on a tie
  float best = NEG;
  int cur = NO_CLASS;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    take_better(best, cur, dB[s], clsB[s]);
    take_better(best, cur, dI[s], clsI[s]);
  }
  wave_best(best, cur);
  take_better(best, cur, dO, o_id);
  __threadfence_block();
  __syncthreads();                             // the backpointers this wave wrote are read back below

  // ---- backtrace, DECODE_W frames per window
  for (int thi = T - 1; thi >= 0;) {
    const int tlo = max(0, thi - DECODE_W + 1);
    const int nfr = thi - tlo + 1;
    for (int e = lane; e < nfr * WPF; e += 64) win[e] = bp[(long)tlo * WPF + e];
    __syncthreads();
    if (lane == 0) {
      int s = cur;
      for (int t = thi; t >= tlo; --t) {
        wout[t - tlo] = s;
        const unsigned* rec = win + (t - tlo) * WPF;
        const int in = info[s];
        const unsigned aw = rec[2 * S];
        const int kind = in < 0 ? 0 : in >> 16;
        int prev;
        if (kind == 2) {
          const int p = in & 0xffff;
          const unsigned bit = (rec[2 * (p >> 6) + ((p & 63) >> 5)] >> (p & 31)) & 1u;
          prev = bit ? a.pairs[2 * p] : s;
        } else if (kind == 1) {
          prev = (int)(aw & 0xffffu);
        } else {
          prev = (aw >> 16) & 1u ? (int)(aw & 0xffffu) : o_id;
        }
        s = (prev >= 0 && prev < C && info[prev] >= 0) ? prev : o_id;
      }
      sh_s = s;
    }
    __syncthreads();
    cur = sh_s;
    if (lane < nfr) ids[tlo + lane] = wout[lane];
    __syncthreads();
    thi = tlo - 1;
  }

  // ---- the score: the objective minus the frames' log-sum-exp
  double ls = 0.0;
  for (int t = lane; t < T; t += 64) ls += (double)lse[t];
  ls = lattice::wave_sum(ls);
  if (lane == 0) {
    a.score[cl.clip] = (float)((double)best + acc - ls);
    a.status[cl.clip] = 0;
  }
}

}  // namespace

extern "C" {

int64_t wfl_decode_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs) {
  const int S = bio::slots_of(n_pairs);
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, S == 0, BpWords{S});
}

int32_t wfl_decode(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                   int32_t n_clips, const int32_t* pairs, int32_t n_pairs, float lambda, float threshold, void* workspace,
                   int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status, void* stream) {
  const char* fn = "wfl_decode";
  bool any_frame;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, lambda, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!score || !status || (n_pairs > 0 && !pairs) || (any_frame && (!logits || !ids))) return lattice::fail(fn, -1, "null device pointer");
  auto a = bio::launch_of<DecodeLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.lambda = lambda; a.ids = ids; a.score = score;
  const int S = bio::slots_of(n_pairs);
  return bio::run<true>(fn, a, false, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, BpWords{S},
                        [&](const DecodeLaunch& a, hipStream_t s) {
                          bio::dispatch_slots(S, [&](auto c) {
                            hipLaunchKernelGGL((decode_chain_kernel<decltype(c)::S, decltype(c)::D>), dim3(a.n), dim3(64), 0, s, a);
                          });
                          return 0;
                        });
}

}  // extern "C"
