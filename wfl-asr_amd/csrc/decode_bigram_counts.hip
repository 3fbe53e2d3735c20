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
#include "bigram_sumproduct.h"

namespace {

using namespace bigram_sp;
using bio::NO_CLASS;
using lattice::MAX_CLASSES;
using lattice::round64;

constexpr int D = 8;                         // frames per emission group

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
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = cl.T, C = a.C, o_id = a.o_id, N = a.n_pairs + 1, LD = row_stride(N), LDR = N + 1;

  float* tab = (float*)lds;
  float* pv = (float*)(lds + table_bytes(N));   // [NW][MAX_SYMBOLS]
  float* endv = pv + NW * MAX_SYMBOLS;          // end[] going forward, u[] going backward
  int* symB = (int*)(endv + MAX_SYMBOLS);
  int* symI = symB + MAX_SYMBOLS;

  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, C, o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) { bio::refuse<NT>(a, cl, 0); return; }            // (zeros, status 0)
  if (tid < a.n_pairs) { symB[tid + 1] = cB[0]; symI[tid + 1] = cI[0]; }
  if (tid == 0) { symB[0] = o_id; symI[0] = NO_CLASS; }
  stage_table(a.trans, N, tab);
  if (tid < MAX_SYMBOLS) endv[tid] = tid == 0 ? 1.f : 0.f;   // the virtual O frame
  __syncthreads();

  const HeadWords head{N};
  unsigned* w0 = a.ws + cl.ws_off;
  float* rec = (float*)w0;                                     // [T][N + 1]: a_t[0 .. N), KA_t
  const float* rowmax = (const float*)(w0 + bio::tail_stat(head(T)));
  const unsigned* forced = w0 + bio::tail_forced(head(T), T);
  const float* Z = a.logits + cl.frame_off * a.ldl;

  // ---- thread q < N owns symbol q: x0 = O's state (q = 0) or B-q's, x1 = I-q's (0 for O and for a phoneme without an I class)
  const bool owner = tid < N;
  const int myB = owner ? symB[tid] : o_id, myI = owner ? symI[tid] : NO_CLASS;
  const bool hasI = myI != NO_CLASS;
  const int col0 = myB, col1 = hasI ? myI : o_id;              // (a state that does not exist reads O's column and gets emission 0)

  auto load_group = [&](int t0, float (&o0)[D], float (&o1)[D], float (&om)[D], unsigned (&of)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = min(t0 + f, T - 1);          // (the tail of the last group re-reads the last row; it is never used)
      const float* z = Z + (long)t * a.ldl;
      o0[f] = z[col0];
      o1[f] = z[col1];
      om[f] = rowmax[t];
      of[f] = forced[t];
    }
  };
  auto to_emissions = [&](float (&o0)[D], float (&o1)[D], const float (&om)[D], const unsigned (&of)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const bool frc = of[f] != 0;
      const float x = expf(o0[f] - om[f]);
      o0[f] = tid == 0 ? (frc ? 1.f : fmaxf(x, W_MIN)) : (frc ? 0.f : x);
      o1[f] = (frc || !hasI) ? 0.f : expf(o1[f] - om[f]);
    }
  };

  // this wave's slice of the summed-over symbols and this lane's output symbols
  const int NS = (N + NW - 1) / NW;
  const int s_lo = min(wv * NS, N), s_hi = min(s_lo + NS, N), ns = s_hi - s_lo;
  int tq[J];
#pragma unroll
  for (int j = 0; j < J; ++j) tq[j] = min(lane + 64 * j, N - 1);   // (a lane past N repeats the last symbol and writes nothing)
  const float* mine = pv + tid;

  float e0[D], e1[D], mx[D];
  unsigned fc[D];

  // ================================================================================================================ forward sweep
  float x0 = tid == 0 ? 1.f : 0.f, x1 = 0.f;     // the virtual O frame
  long KA = 0;                                   // true alpha = x 2^KA (the same in every thread)
  load_group(0, e0, e1, mx, fc);
  to_emissions(e0, e1, mx, fc);
  for (int t0 = 0; t0 < T; t0 += D) {
    float n0[D], n1[D], nm[D];
    unsigned nf[D];
    const bool more = t0 + D < T;
    if (more) load_group(t0 + D, n0, n1, nm, nf);
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) m = fmaxf(m, endv[tq[j]]);
        int ex;
        const float sc = unscale(wave_largest(m), ex);
        KA += ex;
        // what this frame starts from, for the backward sweep: the scaled vector and its exponent
        float* r = rec + (long)t * LDR;
        if (owner) r[tid] = endv[tid] * sc;
        if (tid == 0) r[N] = __int_as_float((int)KA);   // (the low 32 bits: only differences of exponents are needed)
        float acc[J];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = 0.f;
#pragma unroll 4
        for (int s = s_lo; s < s_hi; ++s) {
          const float e = endv[s] * sc;
          const float* row = tab + s * LD;
#pragma unroll
          for (int j = 0; j < J; ++j) acc[j] = fmaf(e, row[tq[j]], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (lane + 64 * j < N) pv[wv * MAX_SYMBOLS + lane + 64 * j] = acc[j];
        __syncthreads();
        if (owner) {
          const float in = (mine[0] + mine[MAX_SYMBOLS]) + (mine[2 * MAX_SYMBOLS] + mine[3 * MAX_SYMBOLS]);
          const float both = (x0 + x1) * sc;     // what I-q continues from
          x1 = e1[f] * both;                     // (O: e1 is 0)
          x0 = e0[f] * in;
          endv[tid] = x0 + x1;
        }
        __syncthreads();
      }
    }
    if (more) {
      to_emissions(n0, n1, nm, nf);
#pragma unroll
      for (int f = 0; f < D; ++f) { e0[f] = n0[f]; e1[f] = n1[f]; }
    }
  }
  // Z = zsum 2^KA, every state may end the clip (every thread computes the same sum)
  double zs = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < N) zs += (double)endv[lane + 64 * j];
  const double zsum = lattice::wave_sum(zs);
  const double inv_zm = 1.0 / zsum;
  const int ka_end = (int)KA;
  __threadfence_block();
  __syncthreads();                               // the records are read back below, and end[] becomes u[]

  // =============================================================================================================== backward sweep
  float tile[J][NSM];                            // this thread's sums: rows tq[j], successors s_lo + qi
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int qi = 0; qi < NSM; ++qi) tile[j][qi] = 0.f;
  float bX = 1.f;                                // beta(O), or beta(B-q) = beta(I-q): the same successors
  int KB = 0;                                    // true beta = b 2^KB (low 32 bits)
  float ra[J][D];
  int rk[D];
  auto load_rec = [&](int t0, float (&oa)[J][D], int (&ok)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const float* r = rec + (long)min(t0 + f, T - 1) * LDR;
#pragma unroll
      for (int j = 0; j < J; ++j) oa[j][f] = r[tq[j]];
      ok[f] = __float_as_int(r[N]);
    }
  };
  const int tl = (T - 1) / D * D;                // the last group
  load_group(tl, e0, e1, mx, fc);
  load_rec(tl, ra, rk);
  to_emissions(e0, e1, mx, fc);
  for (int t0 = tl; t0 >= 0; t0 -= D) {
    float n0[D], n1[D], nm[D], ma[J][D];
    unsigned nf[D];
    int mk[D];
    const bool more = t0 > 0;
    if (more) {
      load_group(t0 - D, n0, n1, nm, nf);
      load_rec(t0 - D, ma, mk);
    }
#pragma unroll
    for (int f = D - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T && t > 0) {                      // (uniform; frame 0 follows the loop)
        float pI = 0.f;
        if (owner) {
          endv[tid] = e0[f] * bX;                // u[q]
          pI = e1[f] * bX;
        }
        __syncthreads();
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) m = fmaxf(m, endv[tq[j]]);
        int ex;
        const float sc = unscale(wave_largest(m), ex);
        KB += ex;
        // the frame's constant, formed in double and clamped (see the header): applied to a_t first
        const int sh = rk[f] + KB - ka_end;      // (wraps to the true, small difference)
        const float c = (float)fmin(ldexp(inv_zm, sh), 0x1p126);
        float v[J], acc[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
          v[j] = ra[j][f] * c;
          acc[j] = 0.f;
        }
        // partial sums over this wave's successors: lane l holds the rows l, l + 64, l + 128
#pragma unroll
        for (int qi = 0; qi < NSM; ++qi) {
          if (qi < ns) {                         // (uniform)
            const float u = endv[s_lo + qi] * sc;
            const float* col = tab + s_lo + qi;
#pragma unroll
            for (int j = 0; j < J; ++j) {
              const float p = col[tq[j] * LD] * u;
              acc[j] += p;
              tile[j][qi] = fmaf(v[j], p, tile[j][qi]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (lane + 64 * j < N) pv[wv * MAX_SYMBOLS + lane + 64 * j] = acc[j];
        __syncthreads();
        if (owner) bX = ((mine[0] + mine[MAX_SYMBOLS]) + (mine[2 * MAX_SYMBOLS] + mine[3 * MAX_SYMBOLS])) + pI * sc;
      }
    }
    if (more) {
      to_emissions(n0, n1, nm, nf);
#pragma unroll
      for (int f = 0; f < D; ++f) {
        e0[f] = n0[f];
        e1[f] = n1[f];
        rk[f] = mk[f];
#pragma unroll
        for (int j = 0; j < J; ++j) ra[j][f] = ma[j][f];
      }
    }
  }

  // ---- frame 0 starts from the virtual O frame (end_{-1} = (1, 0, ...), KA_0 = 0): row O alone, W[O][q] u_0[q] / Z, by q's owner
  if (owner) {
    double g = ldexp((double)tab[tid] * (double)e0[0] * (double)bX * inv_zm, KB - ka_end);
    g = g >= 0.0 ? fmin(g, 1.0) : 0.0;           // (a NaN of an overflowed clip is reported as 0)
    endv[tid] = (float)g;                        // (u[] was last read before frame 1's second barrier)
  }
  __syncthreads();
  float* cnt = a.counts + (long)cl.clip * N * N;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int s = lane + 64 * j;
#pragma unroll
    for (int qi = 0; qi < NSM; ++qi) {
      if (qi < ns && s < N) {
        const int q = s_lo + qi;
        float x = tile[j][qi];
        if (s == 0) x = q == 0 ? 0.f : x + endv[q];   // O after O is no succession
        cnt[(long)s * N + q] = x;
      }
    }
  }

  // ---- logZ: the mantissa, the exponents, and what the emissions left out (the row maxima; O's logit on a forced frame)
  if (wv == 0) {
    double ls = 0.0;
    for (int t = lane; t < T; t += 64) ls += forced[t] ? (double)Z[(long)t * a.ldl + o_id] : (double)rowmax[t];
    ls = lattice::wave_sum(ls);
    if (lane == 0) {
      a.logz[cl.clip] = (float)(log(zsum) + (double)KA * 0.69314718055994530942 + ls);
      a.status[cl.clip] = 0;
    }
  }
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
  bool any_frame;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!logz || !counts || !status || (n_pairs > 0 && !pairs) || (any_frame && !logits)) return lattice::fail(fn, -1, "null device pointer");
  // over the symbol cap: status 2, as over the class cap; the table is read only when the clips are scored
  const int N = n_pairs + 1;
  const bool over = N > MAX_SYMBOLS;
  if (any_frame && !trans && !bio::refused_status(C, n_pairs, over)) return lattice::fail(fn, -1, "null device pointer");
  BigramCountsLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.pairs = pairs; a.n_pairs = n_pairs; a.threshold = threshold; a.status = status;
  a.trans = trans; a.logz = logz; a.counts = counts;
  return bio::run<false>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, HeadWords{N},
                         [&](const BigramCountsLaunch& a, hipStream_t s) {
                           return N <= 64 ? launch_chain<1>(fn, a, s) : (N <= 128 ? launch_chain<2>(fn, a, s) : launch_chain<3>(fn, a, s));
                         });
}

}  // extern "C"
