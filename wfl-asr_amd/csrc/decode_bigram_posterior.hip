// Forward-backward over the BIO grammar of wfl_decode_bigram: per-frame posteriors of a path decoded under a phone-bigram table
// (wfl_decode_bigram_posterior, include/wfl_asr.h).
//
// The sum-product counterpart of csrc/decode_bigram.hip: its symbols (0 is O, 1 + p is phoneme p of `pairs`, N = n_pairs + 1 <=
// MAX_SYMBOLS), its states, legality rule, forced frames, virtual O frame in front of the clip and its table `trans` ([N][N], rows the
// previous symbol, finite or -inf, trans[O][O] never read: O after O costs nothing).  The weight of a legal path is
//     exp(sum_t z[t][c_t] + sum over opened runs trans[previous symbol][opened symbol]),
// the runs counted as the search counts them (every B-q frame, and every O frame whose predecessor is not O).  Any state may end the
// clip.  With W = exp(trans) (-inf -> 0), e the frame's emissions, end[O] = alpha(O), end[p] = alpha(B-p) + alpha(I-p) of the previous
// frame and primes for the next frame (beta):
//     forward    B-q' = e(B-q) sum_s end[s] W[s][q]       O' = e(O) (alpha(O) + sum_{p != O} end[p] W[p][O])
//                I-q' = e(I-q) (alpha(B-q) + alpha(I-q))
//     backward   u[O] = e'(O) beta'(O),  u[q] = e'(B-q) beta'(B-q)
//                beta(O) = u[O] + sum_{q >= 1} W[O][q] u[q]
//                beta(B-p) = beta(I-p) = sum_{q >= 0} W[p][q] u[q] + e'(I-p) beta'(I-p)                beta at T - 1 = 1
// W[O][O] is staged as 1, so O is a symbol like any other in both products: a frame is one matrix-vector product with the table, by
// columns going forward and by rows going backward.  Outputs are wfl_decode_posterior's: logZ; per frame, for the class ids[t] of the
// path, post = gamma(B-p) + gamma(I-p) of the path's phoneme (gamma(O) on an O frame) and cls_post = gamma(ids[t]).  With trans
// identically -lambda everything equals wfl_decode_posterior at that lambda.
//
// Two kernels.  bio::pre_kernel (csrc/bio_grammar.h, as everything this entry shares with the other decode entries; row maxima, as for
// wfl_decode_posterior).  bigram_post_chain_kernel, ONE WORKGROUP of 256 threads per clip, the shape of the search:
//   - the table lives in LDS for the whole clip as LINEAR weights, row = previous symbol, ROW STRIDE LD = N | 1 words (odd).  Forward, wave
//     w takes the predecessors [w NS, (w + 1) NS), NS = ceil(N / 4), lane l the targets l, l + 64, l + 128: the lanes read consecutive
//     words of one row.  Backward, wave w takes the successors [w NS, (w + 1) NS) and lane l the rows l, l + 64, l + 128: the lanes read
//     words LD apart, and an odd stride visits each of the 64 banks once.  Neither sweep has a systematic bank conflict; a transposed
//     copy would not fit (148 KiB at the cap)
//   - the four partial sums per symbol go through LDS, one barrier; thread q < N owns symbol q (both states in registers), adds the four
//     in a fixed order, updates, publishes end[q] (backward: u[q]) for the next frame, second barrier
//   - the owner's emissions exp(z - row maximum) are formed one group of D frames ahead: no transcendental sits on the chain
//   - scale: every wave takes the largest of the PREVIOUS frame's published end[] (u[]), the same value in every wave, and multiplies
//     the vector by the power of two that brings it into [1, 2) as it reads it; the exponents add up in an integer, so the scale costs
//     no rounding however long the clip and needs no barrier of its own
// Guards, as wfl_decode_posterior's: an O emission is at least 2^-60 of its frame's row maximum (over ALL C classes), and a forced
// frame factors O's logit into logZ (every path is in O there).  Here also: a finite table entry is clamped to +-60 ln 2 = +-41.6 nats
// on the linear side (W in [2^-60, 2^60]); -inf is exactly 0.  With the vector's largest entry in [1, 2) a product is at most 2^61, a
// sum of N of them 2^69, and O's state at least 2^-120 of the scale: every sum stays inside fp32 whatever the logits and the table.
// While the row maximum belongs to a class that carries mass at that frame, or O lies within 41.6 nats of it, and the table's finite
// entries lie within +-41.6, the guards move no posterior by more than 1e-18; otherwise the frame leans towards O as described at
// wfl_decode_posterior.  A state smaller than 2^-126 of its frame's largest underflows: its posterior is reported 0.
//
// The alpha lattice is not stored: the forward sweep's owner thread of the path's symbol writes (alpha(B-p) or alpha(O), alpha(I-p) or
// 0, scale exponent) per frame, the backward sweep reads them a group ahead and the owner multiplies them with its beta in double.
// Before the sweeps the workgroup checks in parallel that ids is a path of the grammar (status 8): a class of the table, I-p only after
// B-p / I-p, O on a forced frame, and no run opened through a succession whose W is 0.  Workspace per clip, in words: [alpha records
// 3 T] [pair | kind << 16 per frame T] [row maxima T] [forced flags T], each rounded up to 64: wfl_decode_posterior's.
//
// The chain itself -- LDS layout, staging, owner columns, emissions, the frame of either sweep, logZ -- is csrc/bigram_sumproduct.h's,
// shared with csrc/decode_bigram_counts.hip; what this entry shares with wfl_decode_posterior is csrc/path_posterior.h's.  This file
// keeps the path check's succession test, the loops over the groups, the records and gamma.
#include "bigram_sumproduct.h"
#include "path_posterior.h"

namespace {

using namespace bigram_sp;
using lattice::MAX_CLASSES;
struct HeadWords : bio::PathHead {};   // (a type of this file: bio::pre_kernel<L, HeadWords, LSE> keeps its name)

struct BigramPostLaunch : bio::PathLaunch {
  const float* trans;  // [N][N], rows the previous symbol
};

__global__ __launch_bounds__(NT) void bigram_post_chain_kernel(BigramPostLaunch a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];    // class -> pair | kind << 16 (kind 0 O, 1 B, 2 I); -1 never chosen

  const bio::Clip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = cl.T, N = a.n_pairs + 1;
  float* post = a.post + cl.frame_off;
  float* cls_post = a.cls_post + cl.frame_off;
  Chain<JT> ch(lds, tid, tid >> 6, T, N, (N + 63) / 64);

  // ---- the class table: thread p owns phoneme p here (one slot per thread); a bad one is status 4
  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, a.C, a.o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) {
    if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }
  ch.stage(a.trans, a.n_pairs, a.o_id, cB[0], cI[0]);

  unsigned* w0 = a.ws + cl.ws_off;
  float* rec = (float*)w0;                                     // [T][3]: alpha(B-p) or alpha(O), alpha(I-p) or 0, scale exponent
  int* sel = (int*)(w0 + bio::off_sel(T));
  const unsigned* forced = w0 + bio::tail_forced(HeadWords{}(T), T);

  // ---- is ids a path of this grammar?  Every frame on its own; here also: a run (every B-q frame, every O frame after a phoneme) is
  // opened only through a succession the table allows
  bool bad = false;
  for (int t = tid; t < T; t += NT)
    bad |= bio::path_step_bad(a.ids + cl.frame_off, t, a.C, a.o_id, info, forced, sel, [&](int in, int pin) {
      const int sy = (in >> 16) ? (in & 0xffff) + 1 : 0, psy = (pin >> 16) ? (pin & 0xffff) + 1 : 0;
      return ((in >> 16) == 1 || psy != 0) && !(ch.tab[psy * ch.LD + sy] > 0.f);
    });
  if (__syncthreads_or(bad ? 1 : 0)) { bio::refuse<NT>(a, cl, 8); return; }
  __threadfence_block();
  __syncthreads();                                             // sel[] is read back by every thread below

  ch.own(a.logits + cl.frame_off * a.ldl, a.ldl, (const float*)(w0 + bio::tail_stat(HeadWords{}(T))), forced);
  Group g;
  int sl[D];                                                   // the path's (pair, kind) of the group's frames
  const auto owns = [&](int se) { return tid == ((se >> 16) ? (se & 0xffff) + 1 : 0); };

  // ================================================================================================================ forward sweep
  ch.start_forward();
  ch.load_group(0, g, [&](int f, int t) { sl[f] = sel[t]; });
  ch.to_emissions(g);
  for (int t0 = 0; t0 < T; t0 += D) {
    Group n;
    int ns[D];
    const bool more = t0 + D < T;
    if (more) ch.load_group(t0 + D, n, [&](int f, int t) { ns[f] = sel[t]; });
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = t0 + f;
      if (t < T)                                 // (uniform)
        ch.forward_frame(g.e0[f], g.e1[f], [](float) {}, [&] {
          if (owns(sl[f])) {                     // the path's own symbol, by the thread that owns it
            float* r = rec + 3L * t;
            r[0] = ch.x0;
            r[1] = ch.x1;
            r[2] = __int_as_float((int)ch.KA);   // (the low 32 bits: the backward sweep needs only differences of exponents)
          }
        });
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
#pragma unroll
      for (int f = 0; f < D; ++f) sl[f] = ns[f];
    }
  }
  ch.end_forward();

  // =============================================================================================================== backward sweep
  float r0[D], r1[D], r2[D];
  const int tl = (T - 1) / D * D;                // the last group
  ch.load_group(tl, g, [&](int f, int t) { sl[f] = sel[t]; });
  bio::load_rec(rec, tl, T, r0, r1, r2);
  ch.to_emissions(g);
  for (int t0 = tl; t0 >= 0; t0 -= D) {
    Group n;
    float m0[D], m1[D], m2[D];
    int ns[D];
    const bool more = t0 > 0;
    if (more) {
      ch.load_group(t0 - D, n, [&](int f, int t) { ns[f] = sel[t]; });
      bio::load_rec(rec, t0 - D, T, m0, m1, m2);
    }
#pragma unroll
    for (int f = D - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        // gamma of the path's class at t, by the thread that owns its symbol
        if (owns(sl[f])) bio::write_gamma(r0[f], r1[f], r2[f], sl[f] >> 16, ch.bX, ch.inv_zm, ch.KB, ch.ka_end, post + t, cls_post + t);
        if (t > 0) {                             // (uniform)
          float pI, acc[JT];
          const float sc = ch.backward_publish(g.e0[f], g.e1[f], pI);
#pragma unroll
          for (int j = 0; j < JT; ++j) acc[j] = 0.f;
#pragma unroll 4
          for (int q = ch.s_lo; q < ch.s_hi; ++q) {
            const float u = ch.endv[q] * sc;
            const float* col = ch.tab + q;
#pragma unroll
            for (int j = 0; j < JT; ++j)
              if (j < ch.nj) acc[j] = fmaf(col[ch.tq[j] * ch.LD], u, acc[j]);   // (uniform)
          }
          ch.backward_update(acc, pI, sc);
        }
      }
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
#pragma unroll
      for (int f = 0; f < D; ++f) {
        sl[f] = ns[f];
        r0[f] = m0[f];
        r1[f] = m1[f];
        r2[f] = m2[f];
      }
    }
  }
  ch.write_logz(a, cl);
}

}  // namespace

extern "C" {

int64_t wfl_decode_bigram_posterior_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs) {
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, n_pairs + 1 > MAX_SYMBOLS, HeadWords{});
}

int32_t wfl_decode_bigram_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                    const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs,
                                    const float* trans, float threshold, const int32_t* ids, void* workspace, int64_t workspace_bytes,
                                    float* logz, float* post, float* cls_post, int32_t* status, void* stream) {
  const char* fn = "wfl_decode_bigram_posterior";
  bool any_frame, over;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (bio::path_pointer_missing(logits, pairs, n_pairs, ids, logz, post, cls_post, status, any_frame) ||
      table_missing(trans, any_frame, C, n_pairs, over))
    return lattice::fail(fn, -1, "null device pointer");
  auto a = bio::launch_of<BigramPostLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.trans = trans; a.ids = ids; a.logz = logz; a.post = post; a.cls_post = cls_post;
  return bio::run<false>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, HeadWords{},
                         [&](const BigramPostLaunch& a, hipStream_t s) {
                           if (const int rc = lattice::reserve_lds<bigram_post_chain_kernel, MAX_LDS>(fn)) return rc;
                           hipLaunchKernelGGL(bigram_post_chain_kernel, dim3(a.n), dim3(NT), lds_bytes(n_pairs + 1), s, a);
                           return 0;
                         });
}

}  // extern "C"
