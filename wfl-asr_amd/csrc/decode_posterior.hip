// Forward-backward over the BIO grammar of wfl_decode: per-frame posteriors of a decoded path (wfl_decode_posterior, include/wfl_asr.h).
//
// The sum-product counterpart of csrc/decode.hip over the same states (the classes O, B-p, I-p of `pairs`; every other class is never on
// a path), the same virtual O frame in front of the clip, the same forced frames (largest softmax probability below the threshold: only
// O) and the same penalty.  The weight of a legal path is exp(sum_t z[t][c_t] - lambda * runs opened); in transition terms, with
// w = exp(-lambda):   into O from O: 1    into O from anything else: w    into any B-q from anything: w    into I-p from B-p / I-p: 1.
// Any state may end the clip.
//     logZ = log sum of the weights of all legal paths,      gamma_t(c) = posterior that the path is in class c at frame t.
// With e the frame's emissions, tot the sum of all states of the previous frame (alpha) and primes for the next frame (beta):
//     forward    O'   = e(O) (O + w (tot - O))          B-p' = e(B-p) w tot          I-p' = e(I-p) (I-p + B-p)
//     backward   SB = sum_q e'(B-q) beta'(B-q),  wO = e'(O) beta'(O)
//                beta(O) = wO + w SB          beta(B-p) = beta(I-p) = w (wO + SB) + e'(I-p) beta'(I-p)          beta at T - 1 = 1
// Outputs per frame, for the class ids[t] of the path wfl_decode returned: post = gamma(B-p) + gamma(I-p) of the path's phoneme (gamma(O)
// on an O frame), cls_post = gamma(ids[t]).
//
// Execution shape of the search: bio::pre_kernel (csrc/bio_grammar.h, the search's own pre-pass, here leaving the row maximum in place
// of the log-sum-exp), one wave per frame, fully parallel; decode_post_chain_kernel, ONE WAVE per clip, lane l owning the phonemes l, l + 64, ... (S slots,
// both states of each in registers), so the I-p update is lane-local and the only cross-lane work of a frame is ONE wave sum in each
// direction (DPP inside a row of 16, the four row sums through v_readlane).  No LDS exchange, no barrier in the frame loops.
//
// Arithmetic: scaled linear domain.  e = exp(z - row maximum) is formed when a group of D frames is loaded, one group ahead of the chain,
// so the chain holds no transcendental: a frame is a handful of multiply-adds, the wave sum and a rescale by a power of two taken from the
// exponent of that sum (exact; the exponents add up in an integer, so the scale costs no rounding however long the clip).  On a forced
// frame every path is in O, so O's emission is factored out (taken as 1, its logit added to logZ).  Two guards keep the sums inside
// fp32's exponent range whatever the logits: an O emission is at least 2^-60 of its frame's maximum and w at least 2^-60 (41.6 nats).
// The maximum is the row's, over ALL C classes.  While it belongs to a class that carries mass at that frame, or O lies within 41.6 nats
// of it, the floors move no posterior by more than 1e-18.  On a frame whose largest logit is a class outside the grammar (or an I-q no
// path can reach there) AND stands more than 41.6 nats above O, O is lifted against the B / I states, which keep their true size: that
// frame's posterior leans towards O.  A state smaller than 2^-126 of its frame's sum underflows: its posterior is reported 0.
//
// The alpha lattice is not stored.  The outputs need alpha only on the path's own phoneme: the forward sweep's owning lane writes
// (alpha(B-p), alpha(I-p), scale exponent) -- (alpha(O), 0, exponent) on an O frame -- three words per frame; the backward sweep reads them
// a group ahead and the owning lane multiplies them with its beta (in double, with logZ's mantissa and the three exponents).
// Before the sweeps the wave checks in parallel that ids is a path of the grammar (status 8) and leaves class -> (pair, kind) per frame.
// Workspace per clip, in words: [alpha records 3 T] [pair | kind << 16 per frame T] [row maxima T] [forced flags T], each rounded up to 64;
// the first two are this file's head, the last two the tail of csrc/bio_grammar.h.  That header holds everything this entry shares with
// wfl_decode and wfl_decode_bigram, csrc/path_posterior.h what it shares with wfl_decode_bigram_posterior (the path's launch fields, this
// head, the per-frame path check, the records' loads, gamma); this file holds the chain kernel's frame.
#include "path_posterior.h"
#include "wfl_asr.h"

namespace {

using bio::NO_CLASS;
using lattice::MAX_CLASSES;
struct HeadWords : bio::PathHead {};   // (a type of this file: bio::pre_kernel<L, HeadWords, LSE> keeps its name)

struct PostLaunch : bio::PathLaunch {
  float lambda;
};

constexpr float TINY = 0x1p-60f;   // floor of an O emission and of exp(-lambda)

// ---- every lane gets the wave's sum.  Each DPP step adds two groups that already agree inside themselves (a + b == b + a bit for bit),
// so the 16 lanes of a row end with the same row sum; the four row sums are read through SGPRs.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float wave_total(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);   // row_half_mirror: the other quad of the 8
  v = dpp_add<0x140>(v);   // row_mirror: the other 8 of the 16
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

// x = f 2^e, f in [1, 2): e into `ex`, -> 2^-e (x is positive and normal, see the guards in the header comment)
__device__ __forceinline__ float unscale(float x, int& ex) {
  const int be = __builtin_amdgcn_readfirstlane((__float_as_int(x) >> 23) & 0xff);
  ex = be - 127;
  return __int_as_float((254 - be) << 23);
}

template <int S, int D>
__global__ __launch_bounds__(64) void decode_post_chain_kernel(PostLaunch a) {
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];    // class -> pair | kind << 16 (kind 0 O, 1 B, 2 I); -1 never chosen

  const bio::Clip cl = a.clip[blockIdx.x];
  const int lane = threadIdx.x;
  const int T = cl.T, C = a.C, o_id = a.o_id;
  float* post = a.post + cl.frame_off;
  float* cls_post = a.cls_post + cl.frame_off;

  int clsB[S], clsI[S];
  if (bio::class_table<S, 64>(a.pairs, a.n_pairs, C, o_id, used, info, clsB, clsI)) { bio::refuse<64>(a, cl, 4); return; }
  if (T == 0) {
    if (lane == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }

  unsigned* w0 = a.ws + cl.ws_off;
  float* rec = (float*)w0;                                     // [T][3]: alpha(B-p) or alpha(O), alpha(I-p) or 0, scale exponent
  int* sel = (int*)(w0 + bio::off_sel(T));
  const float* rowmax = (const float*)(w0 + bio::tail_stat(HeadWords{}(T)));
  const unsigned* forced = w0 + bio::tail_forced(HeadWords{}(T), T);
  const float* Z = a.logits + cl.frame_off * a.ldl;

  // ---- is ids a path of this grammar?  Every frame on its own; any run may be opened here.
  bool bad = false;
  for (int t = lane; t < T; t += 64)
    bad |= bio::path_step_bad(a.ids + cl.frame_off, t, C, o_id, info, forced, sel, [](int, int) { return false; });
  if (__any(bad)) { bio::refuse<64>(a, cl, 8); return; }
  __threadfence_block();
  __syncthreads();                                             // sel[] is read back by every lane below

  int colB[S], colI[S];                                        // a state that does not exist reads O's column and gets emission 0
  unsigned hasB = 0, hasI = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    colB[s] = clsB[s] != NO_CLASS ? clsB[s] : o_id;
    colI[s] = clsI[s] != NO_CLASS ? clsI[s] : o_id;
    if (clsB[s] != NO_CLASS) hasB |= 1u << s;
    if (clsI[s] != NO_CLASS) hasI |= 1u << s;
  }
  const float w = fmaxf(expf(-a.lambda), TINY);

  // a group of D frames from t0 on: the raw logits, the row maxima, the forced flags, the path's (pair, kind)
  auto load_group = [&](int t0, float (&ob)[D][S], float (&oi)[D][S], float (&oo)[D], float (&om)[D], unsigned (&of)[D], int (&os)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = min(t0 + f, T - 1);        // (the tail of the last group re-reads the last row; it is never used)
      const float* z = Z + (long)t * a.ldl;
      oo[f] = z[o_id];
      om[f] = rowmax[t];
      of[f] = forced[t];
      os[f] = sel[t];
#pragma unroll
      for (int s = 0; s < S; ++s) { ob[f][s] = z[colB[s]]; oi[f][s] = z[colI[s]]; }
    }
  };
  // ... turned into emissions in place, off the chain
  auto to_emissions = [&](float (&ob)[D][S], float (&oi)[D][S], float (&oo)[D], const float (&om)[D], const unsigned (&of)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const bool frc = of[f] != 0;
      oo[f] = frc ? 1.f : fmaxf(expf(oo[f] - om[f]), TINY);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        ob[f][s] = (frc || !((hasB >> s) & 1u)) ? 0.f : expf(ob[f][s] - om[f]);
        oi[f][s] = (frc || !((hasI >> s) & 1u)) ? 0.f : expf(oi[f][s] - om[f]);
      }
    }
  };

  float eb[D][S], ei[D][S], eo[D], mx[D];
  unsigned fc[D];
  int sl[D];

  // ================================================================================================================ forward sweep
  float aO = 1.f, aB[S], aI[S];                // the virtual O frame
#pragma unroll
  for (int s = 0; s < S; ++s) aB[s] = aI[s] = 0.f;
  long KA = 0;                                 // true alpha = a 2^KA
  load_group(0, eb, ei, eo, mx, fc, sl);
  to_emissions(eb, ei, eo, mx, fc);
  for (int t0 = 0; t0 < T; t0 += D) {
    float nb[D][S], ni[D][S], no[D], nm[D];
    unsigned nf[D];
    int ns[D];
    const bool more = t0 + D < T;
    if (more) load_group(t0 + D, nb, ni, no, nm, nf, ns);
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = t0 + f;
      if (t < T) {                             // (uniform)
        float both[S], part[S];                // both: what I-p continues from
#pragma unroll
        for (int s = 0; s < S; ++s) part[s] = both[s] = aB[s] + aI[s];
#pragma unroll
        for (int h = S / 2; h >= 1; h >>= 1)
#pragma unroll
          for (int s = 0; s < h; ++s) part[s] += part[s + h];
        const float tot = aO + wave_total(part[0]);
        int ex;
        const float sc = unscale(tot, ex);
        KA += ex;
        const float wts = w * tot * sc;
        aO = eo[f] * ((aO + w * (tot - aO)) * sc);
#pragma unroll
        for (int s = 0; s < S; ++s) {
          aI[s] = (ei[f][s] * both[s]) * sc;
          aB[s] = eb[f][s] * wts;
        }
        // the path's own phoneme, by the lane that owns it
        const int se = __builtin_amdgcn_readfirstlane(sl[f]);
        const int slot = (se & 0xffff) >> 6;
        float x0 = aO, x1 = 0.f;
        if (se >> 16) {
#pragma unroll
          for (int s = 0; s < S; ++s)
            if (slot == s) { x0 = aB[s]; x1 = aI[s]; }
        }
        if (lane == (se & 63)) {
          float* r = rec + 3L * t;
          r[0] = x0;
          r[1] = x1;
          r[2] = __int_as_float((int)KA);      // (the low 32 bits: the backward sweep needs only differences of exponents)
        }
      }
    }
    if (more) {
      to_emissions(nb, ni, no, nm, nf);
#pragma unroll
      for (int f = 0; f < D; ++f) {
        eo[f] = no[f];
        sl[f] = ns[f];
#pragma unroll
        for (int s = 0; s < S; ++s) { eb[f][s] = nb[f][s]; ei[f][s] = ni[f][s]; }
      }
    }
  }
  // Z = Zm 2^KA, every state may end the clip
  float zsum = 0.f;
  {
    float part[S];
#pragma unroll
    for (int s = 0; s < S; ++s) part[s] = aB[s] + aI[s];
#pragma unroll
    for (int h = S / 2; h >= 1; h >>= 1)
#pragma unroll
      for (int s = 0; s < h; ++s) part[s] += part[s + h];
    zsum = aO + wave_total(part[0]);
  }
  const double inv_zm = 1.0 / (double)zsum;
  const int ka_end = (int)KA;
  __threadfence_block();
  __syncthreads();                             // the records this wave wrote are read back below

  // =============================================================================================================== backward sweep
  float bO = 1.f, bX[S];                       // beta(B-p) = beta(I-p): the same successors
#pragma unroll
  for (int s = 0; s < S; ++s) bX[s] = 1.f;
  int KB = 0;                                  // true beta = b 2^KB (low 32 bits)
  float r0[D], r1[D], r2[D];
  const int tl = (T - 1) / D * D;              // the last group
  load_group(tl, eb, ei, eo, mx, fc, sl);
  bio::load_rec(rec, tl, T, r0, r1, r2);
  to_emissions(eb, ei, eo, mx, fc);
  for (int t0 = tl; t0 >= 0; t0 -= D) {
    float nb[D][S], ni[D][S], no[D], nm[D], n0[D], n1[D], n2[D];
    unsigned nf[D];
    int ns[D];
    const bool more = t0 > 0;
    if (more) {
      load_group(t0 - D, nb, ni, no, nm, nf, ns);
      bio::load_rec(rec, t0 - D, T, n0, n1, n2);
    }
#pragma unroll
    for (int f = D - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T) {                             // (uniform)
        // gamma of the path's class at t, by the owning lane
        const int se = __builtin_amdgcn_readfirstlane(sl[f]);
        const int slot = (se & 0xffff) >> 6, kind = se >> 16;
        float bs = bO;
        if (kind) {
#pragma unroll
          for (int s = 0; s < S; ++s)
            if (slot == s) bs = bX[s];
        }
        if (lane == (se & 63)) bio::write_gamma(r0[f], r1[f], r2[f], kind, bs, inv_zm, KB, ka_end, post + t, cls_post + t);
        if (t > 0) {
          float part[S], pI[S];
#pragma unroll
          for (int s = 0; s < S; ++s) {
            part[s] = eb[f][s] * bX[s];
            pI[s] = ei[f][s] * bX[s];
          }
#pragma unroll
          for (int h = S / 2; h >= 1; h >>= 1)
#pragma unroll
            for (int s = 0; s < h; ++s) part[s] += part[s + h];
          const float SB = wave_total(part[0]);
          const float wO = eo[f] * bO;
          const float cm = wO + SB;
          int ex;
          const float sc = unscale(cm, ex);
          KB += ex;
          bO = (wO + w * SB) * sc;
          const float base = w * cm * sc;
#pragma unroll
          for (int s = 0; s < S; ++s) bX[s] = base + pI[s] * sc;
        }
      }
    }
    if (more) {
      to_emissions(nb, ni, no, nm, nf);
#pragma unroll
      for (int f = 0; f < D; ++f) {
        eo[f] = no[f];
        sl[f] = ns[f];
        r0[f] = n0[f];
        r1[f] = n1[f];
        r2[f] = n2[f];
#pragma unroll
        for (int s = 0; s < S; ++s) { eb[f][s] = nb[f][s]; ei[f][s] = ni[f][s]; }
      }
    }
  }

  // ---- logZ: the mantissa, the exponents, and what the emissions left out (the row maxima; O's logit on a forced frame)
  bio::write_logz(a, cl, lane, Z, rowmax, forced, (double)zsum, KA);
}

}  // namespace

extern "C" {

int64_t wfl_decode_posterior_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs) {
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, bio::slots_of(n_pairs) == 0, HeadWords{});
}

int32_t wfl_decode_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                             const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, float lambda,
                             float threshold, const int32_t* ids, void* workspace, int64_t workspace_bytes, float* logz, float* post,
                             float* cls_post, int32_t* status, void* stream) {
  const char* fn = "wfl_decode_posterior";
  bool any_frame;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, lambda, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (bio::path_pointer_missing(logits, pairs, n_pairs, ids, logz, post, cls_post, status, any_frame))
    return lattice::fail(fn, -1, "null device pointer");
  auto a = bio::launch_of<PostLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.lambda = lambda; a.ids = ids; a.logz = logz; a.post = post; a.cls_post = cls_post;
  const int S = bio::slots_of(n_pairs);
  return bio::run<false>(fn, a, false, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, HeadWords{},
                         [&](const PostLaunch& a, hipStream_t s) {
                           bio::dispatch_slots(S, [&](auto c) {
                             hipLaunchKernelGGL((decode_post_chain_kernel<decltype(c)::S, decltype(c)::D>), dim3(a.n), dim3(64), 0, s, a);
                           });
                           return 0;
                         });
}

}  // extern "C"
