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
// Two kernels.  decode_pre_kernel, one wave per frame, fully parallel: the frame's log-sum-exp and its forced-to-O flag, so no
// transcendental sits on the serial chain.  decode_chain_kernel, ONE WAVE per clip: lane l owns the phonemes l, l + 64, ... (S slots,
// both states of each in registers), so the I-p update is lane-local, and the only cross-lane work of a frame is one
// max-with-index reduction over the 64 lanes (DPP inside a row of 16, two __shfl_xor across rows); its result feeds O and every B-p.
// There is no LDS exchange and no barrier in the frame loop.  The logits are gathered through the per-lane class ids one group of D
// frames ahead, into registers.  Every 16 frames `best` is subtracted from all states and carried in a double (the scheme of
// align.hip), so the fp32 scores do not grow with T.
// Backpointers: per frame 2 S words of I-p bits (one __ballot per slot), and one word a | (O's bit << 16).  Backtrace: lane 0 walks
// windows of DECODE_W frames that the wave stages into LDS.
// What wfl_decode_posterior (csrc/decode_posterior.hip) scores this search's paths with lives in csrc/bio_grammar.h: the clip record,
// the slot configurations, the pre-pass arithmetic, the class table and its validation, the host's argument checks.  From
// csrc/lattice.h (the alignment kernels' header) come only the class cap, the clips-per-launch constant, round64, wave_sum and the
// host's clip-table batching and workspace check; the kernels here share nothing with the lattice.
#include "bio_grammar.h"
#include "wfl_asr.h"

namespace {

using lattice::CLIPS_PER_LAUNCH;
using lattice::MAX_CLASSES;
using lattice::round64;

using bio::NO_CLASS;
using bio::slots_of;
using DecodeClip = bio::Clip;

constexpr int DECODE_W = 32;                 // backtrace window, frames

struct DecodeLaunch {
  const float* logits;
  long ldl;
  int C, o_id;
  const int* pairs;  // [n_pairs][2]: B class, I class or -1
  int n_pairs;
  float lambda, threshold;
  unsigned* ws;
  int* ids;
  float* score;
  int* status;
  int n, fill_status;
  DecodeClip clip[CLIPS_PER_LAUNCH];
};

// workspace of a clip, in words: [backpointers T (2 S + 1)] [lse T] [forced T], each rounded up to 64 words
__host__ __device__ inline long off_lse(int T, int S) { return round64((long)T * (2 * S + 1)); }
__host__ __device__ inline long off_forced(int T, int S) { return off_lse(T, S) + round64(T); }
inline long clip_words(int T, int S) { return T > 0 ? off_forced(T, S) + round64(T) : 0; }

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

// ---- per frame: log-sum-exp and the forced-to-O flag.  grid (ceil(max T / 4), clips), 4 waves per block, one wave per frame.
__global__ __launch_bounds__(256) void decode_pre_kernel(DecodeLaunch a, int S) {
  const DecodeClip cl = a.clip[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= cl.T) return;
  const float* z = a.logits + (cl.frame_off + t) * a.ldl;
  float m, se;
  bio::frame_stats(z, a.C, lane, m, se);
  if (lane == 0) {
    unsigned* w = a.ws + cl.ws_off;
    ((float*)(w + off_lse(cl.T, S)))[t] = m + logf(se);
    w[off_forced(cl.T, S) + t] = bio::forced_to_o(se, a.threshold);
  }
}

// ---- clips that cannot be decoded (C over the cap, more pairs than classes): O everywhere, score 0, the status
__global__ __launch_bounds__(64) void decode_fill_kernel(DecodeLaunch a) {
  const DecodeClip cl = a.clip[blockIdx.x];
  int* ids = a.ids + cl.frame_off;
  for (int t = threadIdx.x; t < cl.T; t += 64) ids[t] = a.o_id;
  if (threadIdx.x == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = a.fill_status; }
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
  if (bio::class_table<S>(a.pairs, a.n_pairs, C, o_id, used, info, clsB, clsI)) {
    for (int t = lane; t < T; t += 64) ids[t] = o_id;
    if (lane == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 4; }
    return;
  }
  if (T == 0) {
    if (lane == 0) { a.score[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }

  unsigned* bp = a.ws + cl.ws_off;
  const float* lse = (const float*)(bp + off_lse(T, S));
  const unsigned* forced = bp + off_forced(T, S);
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

int launch_chain(int S, const DecodeLaunch& a, hipStream_t s) {
  switch (S) {
    case 2: hipLaunchKernelGGL((decode_chain_kernel<2, 16>), dim3(a.n), dim3(64), 0, s, a); break;
    case 4: hipLaunchKernelGGL((decode_chain_kernel<4, 8>), dim3(a.n), dim3(64), 0, s, a); break;
    case 8: hipLaunchKernelGGL((decode_chain_kernel<8, 4>), dim3(a.n), dim3(64), 0, s, a); break;
    default: hipLaunchKernelGGL((decode_chain_kernel<16, 2>), dim3(a.n), dim3(64), 0, s, a); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : wfl_fail(-3, "wfl_decode: launch failed");
}

}  // namespace

extern "C" {

int64_t wfl_decode_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs) {
  if (n_clips < 0 || n_pairs < 0 || (n_clips > 0 && !n_frames_host)) return -1;
  const int S = slots_of(n_pairs);
  int64_t words = 0;
  for (int b = 0; b < n_clips; ++b) {
    if (n_frames_host[b] < 0) return -1;
    if (S) words += clip_words(n_frames_host[b], S);
  }
  return words * 4;
}

int32_t wfl_decode(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host, const int32_t* n_frames_host,
                   int32_t n_clips, const int32_t* pairs, int32_t n_pairs, float lambda, float threshold, void* workspace,
                   int64_t workspace_bytes, int32_t* ids, float* score, int32_t* status, void* stream) {
  bool any_frame;
  if (const int rc = bio::check_args("wfl_decode", C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, lambda, threshold, any_frame))
    return rc;
  if (n_clips == 0) return 0;
  if (!score || !status || (n_pairs > 0 && !pairs) || (any_frame && (!logits || !ids)))
    return wfl_fail(-1, "wfl_decode: null device pointer");
  // over the class cap: status 2; more pairs than classes (then one is used twice or out of range): status 4
  const int fill = bio::refused_status(C, n_pairs);
  const int S = fill ? 0 : slots_of(n_pairs);
  const int64_t need = fill ? 0 : wfl_decode_workspace_bytes(n_frames_host, n_clips, n_pairs);
  if (const int rc = lattice::check_workspace("wfl_decode", need, workspace, workspace_bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  DecodeLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.pairs = pairs; a.n_pairs = n_pairs; a.lambda = lambda;
  a.threshold = threshold; a.ws = (unsigned*)workspace; a.ids = ids; a.score = score; a.status = status; a.fill_status = fill;
  return lattice::launch_clips<1>(           // one group: the clips in their order
      a, n_clips,
      [&](int b, long off, DecodeClip& c, int&) {
        c = DecodeClip{(long)frame_off_host[b], off, n_frames_host[b], b};
        return fill ? 0 : clip_words(c.T, S);
      },
      [&](int, const DecodeLaunch& a) {
        if (fill) {
          hipLaunchKernelGGL(decode_fill_kernel, dim3(a.n), dim3(64), 0, s, a);
          return hipGetLastError() == hipSuccess ? 0 : wfl_fail(-3, "wfl_decode: launch failed");
        }
        int max_t = 0;
        for (int j = 0; j < a.n; ++j) max_t = std::max(max_t, a.clip[j].T);
        if (max_t > 0) {
          hipLaunchKernelGGL(decode_pre_kernel, dim3((max_t + 3) / 4, a.n), dim3(256), 0, s, a, S);
          if (hipGetLastError() != hipSuccess) return wfl_fail(-3, "wfl_decode: launch failed");
        }
        return launch_chain(S, a, s);
      });
}

}  // extern "C"
