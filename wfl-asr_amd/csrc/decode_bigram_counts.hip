// Expected successions under the BIO grammar of wfl_decode_bigram: one Baum-Welch E-step over the phone-bigram table
// (wfl_decode_bigram_counts, include/wfl_asr.h).
//
// Symbols, states, legality, forced frames, the virtual O frame in front of the clip, the table `trans`, W = exp(trans) with W[O][O]
// staged as 1, the forward and backward recurrences, the guards and the scaling are those of csrc/decode_bigram_posterior.hip: that
// file's header comment is the definition, and what the two chain kernels share is csrc/bigram_sumproduct.h.  With end_{-1} = (1, 0, ...),
// u_t[O] = e_t(O) beta_t(O), u_t[q] = e_t(B-q) beta_t(B-q) and Z the summed weight of every legal path:
//     counts[s][q] = (1 / Z) sum_{t = 0 .. T-1} end_{t-1}[s] W[s][q] u_t[q]      for (s, q) != (O, O);     counts[O][O] = 0
// the expected number of runs of q opened directly after symbol s, the runs counted as the search counts them (every B-q frame, and
// every O frame whose predecessor is not O).  Column q sums to sum_t gamma_t(B-q); a forbidden succession (W = 0) is exactly 0.
//
// Two kernels.  bio::pre_kernel (csrc/bio_grammar.h; row maxima).  bigram_counts_chain_kernel<J>, ONE WORKGROUP of 256 threads per
// clip, the shape of bigram_post_chain_kernel (table in LDS once per clip as linear weights, odd row stride; four wave slices of the
// summed-over symbols; an owner thread per symbol; emissions a group of D frames ahead; the power-of-two scale from the previous frame's
// published vector):
//   - forward: unchanged, except for what it records: per frame t the WHOLE vector the frame starts from, a_t[s] = end_{t-1}[s] scaled
//     by that frame's power of two (largest entry in [1, 2)), N words written by the owners, and the exponent KA_t in word N
//   - backward: wave w takes the successors [w NS, (w + 1) NS), lane l the rows l, l + 64, l + 128, as in the posterior kernel.  The
//     row-wise product already forms p = W[s][q] u_t[q] (u scaled: largest in [1, 2)); the succession's share of frame t is
//     p a_t[s] c_t with the frame's constant c_t = 2^(KA_t + KB_{t-1} - KA_end) / zsum.  A thread keeps its J x NS tile of sums in
//     REGISTERS for the whole clip (3 x 48 = 144 at the cap; LDS has no room beside the 145 KiB table) and stores it once at the end.
//     The tile must be indexed at compile time: the kernel is instantiated for J = 1, 2, 3 lane groups (N <= 64, 128, 192), the loop
//     over a wave's successors fully unrolled to 16 J and predicated (uniform).  a_t (J values per lane) and KA_t are loaded a group of
//     frames ahead
//   - frame 0 has only row O (end_{-1}): the owner of q forms W[O][q] u_0[q] / Z in double after the loop; it is added to row O as the
//     tile is stored, where [O][O] is set to 0
// Range of the frame constant.  Every share p a c is at most 1 (the shares of a frame sum to gamma_t(O) + sum_q gamma_t(B-q) <= 1),
// but c alone is not bounded: it is large exactly when every product of the frame is small.  c is formed in double (ldexp of 1 / zsum,
// zsum in [1, 2^78)) and brought to fp32 clamped to 2^126; it is applied to a FIRST: v = a c < 2 x 2^126 is finite, p = W u <= 2^60 x 2
// is finite, and v p is the share itself, <= 1 up to rounding, whenever the clamp is not active.  The clamp is active only when
// c > 2^126, i.e. when every p a of the frame is below 2^-126: those products have left fp32's normal range already (the posterior
// kernel reports such states as 0), and the clamp makes the share smaller, never larger.  A small c only underflows v towards 0, an
// absolute error below 2^-126 x 2^61.  No factor is inf or NaN for any logits and any table inside the clamps, so W = 0 gives an exact
// 0 and every entry is >= 0.  The running sums are fp32: a frame adds at most 1, a clip of T frames at most T.
//
// Workspace per clip, in words: [a_t and KA_t: T (N + 1)] [row maxima T] [forced flags T], each rounded up to 64.
//
// This file keeps what the kernel records, its register tile and the loop that fills it, frame 0 and the stores; every other line of
// the chain is a call into csrc/bigram_sumproduct.h.
#include "bigram_sumproduct.h"

namespace {

using namespace bigram_sp;
using lattice::MAX_CLASSES;
using lattice::round64;

struct BigramCountsLaunch : bio::Launch {
  const float* trans;  // [N][N], rows the previous symbol
  float *logz, *counts;
};

// head of a clip's workspace, in words: per frame the scaled vector it starts from and the scale exponent
struct HeadWords {
  int N;
  __host__ __device__ long operator()(int T) const { return round64((long)T * (N + 1)); }
};

template <int J>
__global__ __launch_bounds__(NT) void bigram_counts_chain_kernel(BigramCountsLaunch a) {
  constexpr int NSM = 16 * J;                    // successors of a wave, at most: ceil(64 J / 4)
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];

  const bio::Clip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = cl.T, N = a.n_pairs + 1, LDR = N + 1;
  Chain<J> ch(lds, tid, __builtin_amdgcn_readfirstlane(tid >> 6), T, N, J);

  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, a.C, a.o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) { bio::refuse<NT>(a, cl, 0); return; }            // (zeros, status 0)
  ch.stage(a.trans, a.n_pairs, a.o_id, cB[0], cI[0]);

  const HeadWords head{N};
  unsigned* w0 = a.ws + cl.ws_off;
  float* rec = (float*)w0;                                     // [T][N + 1]: a_t[0 .. N), KA_t
  ch.own(a.logits + cl.frame_off * a.ldl, a.ldl, (const float*)(w0 + bio::tail_stat(head(T))), w0 + bio::tail_forced(head(T), T));
  const int ns = ch.s_hi - ch.s_lo;
  Group g;

  // ================================================================================================================ forward sweep
  ch.start_forward();
  ch.load_group(0, g);
  ch.to_emissions(g);
  for (int t0 = 0; t0 < T; t0 += D) {
    Group n;
    const bool more = t0 + D < T;
    if (more) ch.load_group(t0 + D, n);
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = t0 + f;
      if (t < T)                                 // (uniform)
        ch.forward_frame(g.e0[f], g.e1[f], [&](float sc) {
          // what this frame starts from, for the backward sweep: the scaled vector and its exponent
          float* r = rec + (long)t * LDR;
          if (ch.owner) r[tid] = ch.endv[tid] * sc;
          if (tid == 0) r[N] = __int_as_float((int)ch.KA);   // (the low 32 bits: only differences of exponents are needed)
        }, [] {});
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
    }
  }
  ch.end_forward();

  // =============================================================================================================== backward sweep
  float tile[J][NSM];                            // this thread's sums: rows tq[j], successors s_lo + qi
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int qi = 0; qi < NSM; ++qi) tile[j][qi] = 0.f;
  float ra[J][D];
  int rk[D];
  auto load_rec = [&](int t0, float (&oa)[J][D], int (&ok)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const float* r = rec + (long)min(t0 + f, T - 1) * LDR;
#pragma unroll
      for (int j = 0; j < J; ++j) oa[j][f] = r[ch.tq[j]];
      ok[f] = __float_as_int(r[N]);
    }
  };
  const int tl = (T - 1) / D * D;                // the last group
  ch.load_group(tl, g);
  load_rec(tl, ra, rk);
  ch.to_emissions(g);
  for (int t0 = tl; t0 >= 0; t0 -= D) {
    Group n;
    float ma[J][D];
    int mk[D];
    const bool more = t0 > 0;
    if (more) {
      ch.load_group(t0 - D, n);
      load_rec(t0 - D, ma, mk);
    }
#pragma unroll
    for (int f = D - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T && t > 0)                        // (uniform; frame 0 follows the loop)
        ch.backward_frame(g.e0[f], g.e1[f], [&](float sc, float (&acc)[J]) {
          // the frame's constant, formed in double and clamped (see the header): applied to a_t first
          const int sh = rk[f] + ch.KB - ch.ka_end;   // (wraps to the true, small difference)
          const float c = (float)fmin(ldexp(ch.inv_zm, sh), 0x1p126);
          float v[J];
#pragma unroll
          for (int j = 0; j < J; ++j) {
            v[j] = ra[j][f] * c;
            acc[j] = 0.f;
          }
#pragma unroll
          for (int qi = 0; qi < NSM; ++qi) {
            if (qi < ns) {                       // (uniform)
              const float u = ch.endv[ch.s_lo + qi] * sc;
              const float* col = ch.tab + ch.s_lo + qi;
#pragma unroll
              for (int j = 0; j < J; ++j) {
                const float p = col[ch.tq[j] * ch.LD] * u;
                acc[j] += p;
                tile[j][qi] = fmaf(v[j], p, tile[j][qi]);
              }
            }
          }
        });
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
#pragma unroll
      for (int f = 0; f < D; ++f) {
        rk[f] = mk[f];
#pragma unroll
        for (int j = 0; j < J; ++j) ra[j][f] = ma[j][f];
      }
    }
  }

  // ---- frame 0 starts from the virtual O frame (end_{-1} = (1, 0, ...), KA_0 = 0): row O alone, W[O][q] u_0[q] / Z, by q's owner
  if (ch.owner) {
    double gq = ldexp((double)ch.tab[tid] * (double)g.e0[0] * (double)ch.bX * ch.inv_zm, ch.KB - ch.ka_end);
    gq = gq >= 0.0 ? fmin(gq, 1.0) : 0.0;        // (a NaN of an overflowed clip is reported as 0)
    ch.endv[tid] = (float)gq;                    // (u[] was last read before frame 1's second barrier)
  }
  __syncthreads();
  float* cnt = a.counts + (long)cl.clip * N * N;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int s = ch.lane + 64 * j;
#pragma unroll
    for (int qi = 0; qi < NSM; ++qi) {
      if (qi < ns && s < N) {
        const int q = ch.s_lo + qi;
        float x = tile[j][qi];
        if (s == 0) x = q == 0 ? 0.f : x + ch.endv[q];   // O after O is no succession
        cnt[(long)s * N + q] = x;
      }
    }
  }
  ch.write_logz(a, cl);
}

template <int J>
int launch_chain(const char* fn, const BigramCountsLaunch& a, hipStream_t s) {
  if (const int rc = lattice::reserve_lds<bigram_counts_chain_kernel<J>, MAX_LDS>(fn)) return rc;
  hipLaunchKernelGGL(bigram_counts_chain_kernel<J>, dim3(a.n), dim3(NT), lds_bytes(a.n_pairs + 1), s, a);
  return 0;
}

}  // namespace

extern "C" {

int64_t wfl_decode_bigram_counts_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs) {
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, n_pairs + 1 > MAX_SYMBOLS, HeadWords{n_pairs + 1});
}

int32_t wfl_decode_bigram_counts(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                 const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs, const float* trans,
                                 float threshold, void* workspace, int64_t workspace_bytes, float* logz, float* counts, int32_t* status,
                                 void* stream) {
  const char* fn = "wfl_decode_bigram_counts";
  bool any_frame, over;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!logz || !counts || !status || (n_pairs > 0 && !pairs) || (any_frame && !logits) || table_missing(trans, any_frame, C, n_pairs, over))
    return lattice::fail(fn, -1, "null device pointer");
  const int N = n_pairs + 1;
  auto a = bio::launch_of<BigramCountsLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.trans = trans; a.logz = logz; a.counts = counts;
  return bio::run<false>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, HeadWords{N},
                         [&](const BigramCountsLaunch& a, hipStream_t s) {
                           return N <= 64 ? launch_chain<1>(fn, a, s) : (N <= 128 ? launch_chain<2>(fn, a, s) : launch_chain<3>(fn, a, s));
                         });
}

}  // extern "C"
