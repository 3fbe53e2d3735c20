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
#include "bigram_sumproduct.h"

namespace {

using namespace bigram_sp;   // the workgroup's shape, the table in LDS, the scale: shared with csrc/decode_bigram_counts.hip
using bio::NO_CLASS;
using lattice::MAX_CLASSES;
using lattice::round64;

constexpr int D = 8;                         // frames per emission group

struct BigramPostLaunch : bio::Launch {
  const float* trans;  // [N][N], rows the previous symbol
  const int* ids;
  float *logz, *post, *cls_post;
};

// head of a clip's workspace, in words: the alpha records, then the path's (pair, kind) per frame
__host__ __device__ inline long off_sel(int T) { return round64(3L * T); }
struct HeadWords {
  __host__ __device__ long operator()(int T) const { return off_sel(T) + round64(T); }
};

__global__ __launch_bounds__(NT) void bigram_post_chain_kernel(BigramPostLaunch a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];    // class -> pair | kind << 16 (kind 0 O, 1 B, 2 I); -1 never chosen

  const bio::Clip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = cl.T, C = a.C, o_id = a.o_id, N = a.n_pairs + 1, LD = row_stride(N);
  const int* ids = a.ids + cl.frame_off;
  float* post = a.post + cl.frame_off;
  float* cls_post = a.cls_post + cl.frame_off;

  float* tab = (float*)lds;
  float* pv = (float*)(lds + table_bytes(N));   // [NW][MAX_SYMBOLS]
  float* endv = pv + NW * MAX_SYMBOLS;          // end[] going forward, u[] going backward
  int* symB = (int*)(endv + MAX_SYMBOLS);
  int* symI = symB + MAX_SYMBOLS;

  // ---- the class table: thread p owns phoneme p here (one slot per thread); a bad one is status 4
  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, C, o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) {
    if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }
  if (tid < a.n_pairs) { symB[tid + 1] = cB[0]; symI[tid + 1] = cI[0]; }
  if (tid == 0) { symB[0] = o_id; symI[0] = NO_CLASS; }
  stage_table(a.trans, N, tab);
  if (tid < MAX_SYMBOLS) endv[tid] = tid == 0 ? 1.f : 0.f;   // the virtual O frame
  __syncthreads();

  unsigned* w0 = a.ws + cl.ws_off;
  float* rec = (float*)w0;                                     // [T][3]: alpha(B-p) or alpha(O), alpha(I-p) or 0, scale exponent
  int* sel = (int*)(w0 + off_sel(T));
  const float* rowmax = (const float*)(w0 + bio::tail_stat(HeadWords{}(T)));
  const unsigned* forced = w0 + bio::tail_forced(HeadWords{}(T), T);
  const float* Z = a.logits + cl.frame_off * a.ldl;

  // ---- is ids a path of this grammar?  Every frame on its own: a class of the table, I-p only after B-p / I-p, O on a forced frame,
  // and a run (every B-q frame, every O frame after a phoneme) opened only through a succession the table allows.
  bool bad = false;
  for (int t = tid; t < T; t += NT) {
    const int c = ids[t];
    const int in = (c >= 0 && c < C) ? info[c] : -1;
    const int pc = t ? ids[t - 1] : o_id;
    const int pin = (pc >= 0 && pc < C) ? info[pc] : -1;
    if (in < 0) bad = true;
    else if (pin >= 0) {                                       // (a bad previous class is found at its own frame)
      const int kind = in >> 16, pkind = pin >> 16;
      const int sy = kind ? (in & 0xffff) + 1 : 0, psy = pkind ? (pin & 0xffff) + 1 : 0;
      if (kind == 2) {
        if (pkind == 0 || psy != sy) bad = true;
      } else if (kind == 1 || psy != 0) {
        if (!(tab[psy * LD + sy] > 0.f)) bad = true;
      }
    }
    if (in > 0 && forced[t]) bad = true;                       // (in == 0 is O)
    sel[t] = in < 0 ? 0 : in;
  }
  if (__syncthreads_or(bad ? 1 : 0)) { bio::refuse<NT>(a, cl, 8); return; }
  __threadfence_block();
  __syncthreads();                                             // sel[] is read back by every thread below

  // ---- thread q < N owns symbol q: x0 = O's state (q = 0) or B-q's, x1 = I-q's (0 for O and for a phoneme without an I class)
  const bool owner = tid < N;
  const int myB = owner ? symB[tid] : o_id, myI = owner ? symI[tid] : NO_CLASS;
  const bool hasI = myI != NO_CLASS;
  const int col0 = myB, col1 = hasI ? myI : o_id;              // (a state that does not exist reads O's column and gets emission 0)

  // a group of D frames from t0 on: the raw logits, the row maxima, the forced flags, the path's (pair, kind)
  auto load_group = [&](int t0, float (&o0)[D], float (&o1)[D], float (&om)[D], unsigned (&of)[D], int (&os)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = min(t0 + f, T - 1);          // (the tail of the last group re-reads the last row; it is never used)
      const float* z = Z + (long)t * a.ldl;
      o0[f] = z[col0];
      o1[f] = z[col1];
      om[f] = rowmax[t];
      of[f] = forced[t];
      os[f] = sel[t];
    }
  };
  // ... turned into emissions in place, off the chain
  auto to_emissions = [&](float (&o0)[D], float (&o1)[D], const float (&om)[D], const unsigned (&of)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const bool frc = of[f] != 0;
      const float x = expf(o0[f] - om[f]);
      o0[f] = tid == 0 ? (frc ? 1.f : fmaxf(x, W_MIN)) : (frc ? 0.f : x);
      o1[f] = (frc || !hasI) ? 0.f : expf(o1[f] - om[f]);
    }
  };

  // this thread's slice of the summed-over symbols and its output symbols
  const int NS = (N + NW - 1) / NW;
  const int s_lo = min(wv * NS, N), s_hi = min(s_lo + NS, N);
  int tq[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) tq[j] = min(lane + 64 * j, N - 1);   // (a lane past N repeats the last symbol and writes nothing)
  const int nj = (N + 63) / 64;
  const float* mine = pv + tid;

  float e0[D], e1[D], mx[D];
  unsigned fc[D];
  int sl[D];

  // ================================================================================================================ forward sweep
  float x0 = tid == 0 ? 1.f : 0.f, x1 = 0.f;     // the virtual O frame
  long KA = 0;                                   // true alpha = x 2^KA (the same in every thread)
  load_group(0, e0, e1, mx, fc, sl);
  to_emissions(e0, e1, mx, fc);
  for (int t0 = 0; t0 < T; t0 += D) {
    float n0[D], n1[D], nm[D];
    unsigned nf[D];
    int ns[D];
    const bool more = t0 + D < T;
    if (more) load_group(t0 + D, n0, n1, nm, nf, ns);
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < JT; ++j) m = fmaxf(m, endv[tq[j]]);
        int ex;
        const float sc = unscale(wave_largest(m), ex);
        KA += ex;
        // partial sums over this wave's predecessors
        float acc[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[j] = 0.f;
#pragma unroll 4
        for (int s = s_lo; s < s_hi; ++s) {
          const float e = endv[s] * sc;
          const float* row = tab + s * LD;
#pragma unroll
          for (int j = 0; j < JT; ++j)
            if (j < nj) acc[j] = fmaf(e, row[tq[j]], acc[j]);   // (uniform)
        }
#pragma unroll
        for (int j = 0; j < JT; ++j)
          if (lane + 64 * j < N) pv[wv * MAX_SYMBOLS + lane + 64 * j] = acc[j];
        __syncthreads();
        if (owner) {
          const float in = (mine[0] + mine[MAX_SYMBOLS]) + (mine[2 * MAX_SYMBOLS] + mine[3 * MAX_SYMBOLS]);
          const float both = (x0 + x1) * sc;     // what I-q continues from
          x1 = e1[f] * both;                     // (O: e1 is 0)
          x0 = e0[f] * in;
          endv[tid] = x0 + x1;
          // the path's own symbol, by the thread that owns it
          const int se = sl[f];
          if (tid == ((se >> 16) ? (se & 0xffff) + 1 : 0)) {
            float* r = rec + 3L * t;
            r[0] = x0;
            r[1] = x1;
            r[2] = __int_as_float((int)KA);      // (the low 32 bits: the backward sweep needs only differences of exponents)
          }
        }
        __syncthreads();
      }
    }
    if (more) {
      to_emissions(n0, n1, nm, nf);
#pragma unroll
      for (int f = 0; f < D; ++f) { e0[f] = n0[f]; e1[f] = n1[f]; sl[f] = ns[f]; }
    }
  }
  // Z = zsum 2^KA, every state may end the clip (every thread computes the same sum)
  double zs = 0.0;
#pragma unroll
  for (int j = 0; j < JT; ++j)
    if (lane + 64 * j < N) zs += (double)endv[lane + 64 * j];
  const double zsum = lattice::wave_sum(zs);
  const double inv_zm = 1.0 / zsum;
  const int ka_end = (int)KA;
  __threadfence_block();
  __syncthreads();                               // the records are read back below, and end[] becomes u[]

  // =============================================================================================================== backward sweep
  float bX = 1.f;                                // beta(O), or beta(B-q) = beta(I-q): the same successors
  int KB = 0;                                    // true beta = b 2^KB (low 32 bits)
  float r0[D], r1[D], r2[D];
  auto load_rec = [&](int t0, float (&o0)[D], float (&o1)[D], float (&o2)[D]) {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const float* r = rec + 3L * min(t0 + f, T - 1);
      o0[f] = r[0];
      o1[f] = r[1];
      o2[f] = r[2];
    }
  };
  const int tl = (T - 1) / D * D;                // the last group
  load_group(tl, e0, e1, mx, fc, sl);
  load_rec(tl, r0, r1, r2);
  to_emissions(e0, e1, mx, fc);
  for (int t0 = tl; t0 >= 0; t0 -= D) {
    float n0[D], n1[D], nm[D], m0[D], m1[D], m2[D];
    unsigned nf[D];
    int ns[D];
    const bool more = t0 > 0;
    if (more) {
      load_group(t0 - D, n0, n1, nm, nf, ns);
      load_rec(t0 - D, m0, m1, m2);
    }
#pragma unroll
    for (int f = D - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        // gamma of the path's class at t, by the thread that owns its symbol
        const int se = sl[f];
        const int kind = se >> 16;
        if (tid == (kind ? (se & 0xffff) + 1 : 0)) {
          const int sh = __float_as_int(r2[f]) + KB - ka_end;            // (wraps to the true, small difference)
          const double k = ldexp((double)bX * inv_zm, sh);
          double gp = (double)(r0[f] + r1[f]) * k, gc = (double)(kind == 2 ? r1[f] : r0[f]) * k;
          gp = gp >= 0.0 ? fmin(gp, 1.0) : 0.0;                          // (a NaN of an overflowed clip is reported as 0)
          gc = gc >= 0.0 ? fmin(gc, 1.0) : 0.0;
          post[t] = (float)gp;
          cls_post[t] = (float)gc;
        }
        if (t > 0) {                             // (uniform)
          float pI = 0.f;
          if (owner) {
            endv[tid] = e0[f] * bX;              // u[q]
            pI = e1[f] * bX;
          }
          __syncthreads();
          float m = 0.f;
#pragma unroll
          for (int j = 0; j < JT; ++j) m = fmaxf(m, endv[tq[j]]);
          int ex;
          const float sc = unscale(wave_largest(m), ex);
          KB += ex;
          // partial sums over this wave's successors: lane l holds the rows l, l + 64, l + 128
          float acc[JT];
#pragma unroll
          for (int j = 0; j < JT; ++j) acc[j] = 0.f;
#pragma unroll 4
          for (int q = s_lo; q < s_hi; ++q) {
            const float u = endv[q] * sc;
            const float* col = tab + q;
#pragma unroll
            for (int j = 0; j < JT; ++j)
              if (j < nj) acc[j] = fmaf(col[tq[j] * LD], u, acc[j]);     // (uniform)
          }
#pragma unroll
          for (int j = 0; j < JT; ++j)
            if (lane + 64 * j < N) pv[wv * MAX_SYMBOLS + lane + 64 * j] = acc[j];
          __syncthreads();
          if (owner) bX = ((mine[0] + mine[MAX_SYMBOLS]) + (mine[2 * MAX_SYMBOLS] + mine[3 * MAX_SYMBOLS])) + pI * sc;
        }
      }
    }
    if (more) {
      to_emissions(n0, n1, nm, nf);
#pragma unroll
      for (int f = 0; f < D; ++f) {
        e0[f] = n0[f];
        e1[f] = n1[f];
        sl[f] = ns[f];
        r0[f] = m0[f];
        r1[f] = m1[f];
        r2[f] = m2[f];
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
  bool any_frame;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!logz || !status || (n_pairs > 0 && !pairs) || (any_frame && (!logits || !ids || !post || !cls_post)))
    return lattice::fail(fn, -1, "null device pointer");
  // over the symbol cap: status 2, as over the class cap; the table is read only when the clips are scored
  const int N = n_pairs + 1;
  const bool over = N > MAX_SYMBOLS;
  if (any_frame && !trans && !bio::refused_status(C, n_pairs, over)) return lattice::fail(fn, -1, "null device pointer");
  BigramPostLaunch a{};
  a.logits = logits; a.ldl = ldl; a.C = C; a.o_id = o_id; a.pairs = pairs; a.n_pairs = n_pairs; a.threshold = threshold; a.status = status;
  a.trans = trans; a.ids = ids; a.logz = logz; a.post = post; a.cls_post = cls_post;
  return bio::run<false>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, HeadWords{},
                         [&](const BigramPostLaunch& a, hipStream_t s) {
                           if (const int rc = lattice::reserve_lds<bigram_post_chain_kernel, MAX_LDS>(fn)) return rc;
                           hipLaunchKernelGGL(bigram_post_chain_kernel, dim3(a.n), dim3(NT), lds_bytes(N), s, a);
                           return 0;
                         });
}

}  // extern "C"
