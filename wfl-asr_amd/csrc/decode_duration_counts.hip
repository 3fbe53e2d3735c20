// Expected run lengths and successions over the explicit-duration BIO grammar of wfl_decode_duration: one E-step of an EM that learns
// the free decode's duration prior (and its bigram) from audio without labels (wfl_decode_duration_counts, include/wfl_asr.h).
//
// The lattice, the tables, the recurrences, the guards and the "largest value alive" scale are csrc/decode_duration_posterior.hip's:
// that file's header comment is the definition, its notation (In, R, Y, end, bE, bO, Wr, V, u, W, lambda, tau) is used here, and its two
// frame functions are repeated here with what the sums need added.  There is no path: the sums run over every legal path.
//     succ[s][q]      = (1 / Z) sum_t end_s(t-1) W[s][q] u_t[q]                     (s, q) != (O, O);  succ[O][O] = 0
//     dur_counts[p][j] = (1 / Z) sum_t R_p^{j+1}(t) lambda_p(j+1) bE_p(t)          j = 0 .. D - 2: runs of exactly j + 1 frames, t the last
//     dur_counts[p][D-1] = (1 / Z) sum_t R_p^D(t) lambda_p(D) V_p(t)               runs of D frames or more, t the D-th frame
//     dur_counts[p][D]   = (1 / Z) sum_t Y_p(t) V_p(t)                             frames past the D-th
// At the last frame bE = V = 1: a run the clip cuts off counts with its cut length, as the search charges it.
//
// Two kernels.  bio::pre_kernel (row maxima, forced flags).  duration_counts_chain_kernel<J, HL>, ONE WORKGROUP of 256 threads per clip,
// on bigram_sumproduct.h's Chain as duration_post_chain_kernel uses it, in THREE sweeps:
//   forward    the posterior kernel's frame.  Records per frame t: a_t[s] = end_s(t-1) scaled as the frame's products read it (N words, by
//              the owners), R_q^1(t) (N words, by the owners) and the exponent KA_t
//   backward   the posterior kernel's frame.  Records per frame t: bE_q(t), V_q(t) (2 N words, by the owners) and the exponent KB_t.  The
//              row-wise product forms p = W[s][q] u_t[q]; the succession's share of the frame is a_t[s] p c_t with
//              c_t = 2^(KA_t + KB_{t-1} - KA_end) / zsum: csrc/decode_bigram_counts.hip's register tile, J x 16 J fp32 sums per thread kept
//              for the whole clip, indexed at compile time (the kernel is instantiated for J = 1, 2, 3 lane groups), a frame adds at most
//              1; frame 0 (row O alone) by the owners after the loop
//   counting   END-INDEXED, forward again, by the owner threads alone: no product over the table, no barrier, no exchange.  The owner
//              recomputes its ring R^1 .. R^D and Y from the recorded R^1(t), the recorded exponents (the scale of frame t is
//              2^-(KA_t - KA_{t-1} - KS), the power of two the forward sweep used) and the frame's e(I), exactly as the forward sweep
//              did, and adds R^j(t) lambda(j) bE(t) c'_t (j < D), R^D(t) lambda(D) V(t) c'_t and Y(t) V(t) c'_t with
//              c'_t = 2^(KA_t + KB_t - KA_end) / zsum.  The start-indexed alternative (a third ring Q in the backward sweep, R^D and Y
//              recorded) puts D more LDS round trips per symbol and frame on the barrier-bound chain; here they run off it
//              (DESIGN section 4 has both budgets)
// The (D + 1) sums of a symbol are indexed by the run-time age j: they are addressed memory, DOUBLE, behind the ring and the rows --
// column j of symbol q at double j HS + q -- in LDS where ring, rows and sums fit and in the clip's workspace where they do not
// (store_in_lds).  Only the owner thread of a symbol touches its ring and sums: no atomics.  They are never a register array; the
// kernel uses no scratch (profiles/decode_duration_counts_resources.txt).
// Range.  c_t and c'_t are formed in double (ldexp of 1 / zsum) and clamped to 2^126 as in the bigram counts kernel.  The succession's
// share applies c to a first (a < 2^-3).  A duration share is formed entirely in double: R < 2^65, lambda bE and lambda V < 2^125 (the
// posterior kernel's bounds), c <= 2^126, so the product is below 2^316 and finite; where the clamp is not active it is the share
// itself, at most 1 up to rounding; where it is active every product of the frame has left fp32's range and the share only gets
// smaller.  lambda = 0 (and tau = 0 for the excess) gives an exact 0.0; every term is >= 0.
//
// Workspace per clip with T > 0, in 4-byte words: [records round_up_64(T (4 N + 2))] [ring, rows and sums round_up_64((4 D + 3) HS) where
// LDS does not hold them] [row maxima round_up_64(T)] [forced flags round_up_64(T)].
#include "bigram_sumproduct.h"

namespace {

using bigram_sp::Chain;
using bigram_sp::Group;
using bigram_sp::MAX_SYMBOLS;
using bigram_sp::NT;
using bigram_sp::NW;
using bigram_sp::W_MAX;
using bigram_sp::W_MIN;
using lattice::MAX_CLASSES;
constexpr int GF = bigram_sp::D;             // frames per emission group
constexpr int MAX_D = 32;                    // the table's longest explicit duration, frames
constexpr int JU = 8;                        // ring entries of a symbol in flight together
constexpr int KS = 4;                        // the scaled largest alive value lies in [2^-KS, 2^(1-KS))
constexpr float CK = 0x1p-4f;
constexpr int LDS_CAP = 160 * 1024;

struct DurCountsLaunch : bio::Launch {
  const float* trans;    // [N][N], rows the previous symbol
  const int* sym_dur;    // [n_pairs] row of `dur`, -1 none
  const float* dur;      // [n_rows][D + 1]
  int n_rows, D;
  float *logz, *succ, *dur_counts;
};

// dynamic LDS, in bytes: [the chain's areas, bigram_sp::lds_bytes(N)] [alive MAX_SYMBOLS] [Y / V (O: its state) MAX_SYMBOLS] [the ring D HS
// floats, the symbols' rows (D + 1) HS floats, the sums (D + 1) HS doubles, where they fit]
constexpr int EXTRA_BYTES = 2 * MAX_SYMBOLS * 4;
constexpr int STATIC_BYTES = (MAX_CLASSES + MAX_CLASSES / 32 + 96) * 4;   // the kernel's __shared__ variables as declared, rounded up
constexpr int MAX_DYN_LDS = LDS_CAP - STATIC_BYTES;
static_assert(bigram_sp::MAX_LDS + EXTRA_BYTES <= MAX_DYN_LDS, "LDS of one CU");

__host__ __device__ inline int fixed_bytes(int N) { return bigram_sp::table_bytes(N) + bigram_sp::FIXED_BYTES + EXTRA_BYTES; }
__host__ __device__ inline int hist_stride(int N) { return (N + 63) / 64 * 64; }
__host__ __device__ inline long hist_words(int N, int D) { return (long)(2 * D + 1) * hist_stride(N); }                  // ring and rows
__host__ __device__ inline long store_words(int N, int D) { return hist_words(N, D) + 2L * (D + 1) * hist_stride(N); }   // ... and sums
__host__ __device__ inline bool store_in_lds(int N, int D) { return fixed_bytes(N) + store_words(N, D) * 4 <= MAX_DYN_LDS; }
inline int lds_bytes(int N, int D) { return fixed_bytes(N) + (store_in_lds(N, D) ? (int)store_words(N, D) * 4 : 0); }

// head of a clip's workspace, in words
struct DurCountsHead {
  int N, D;
  __host__ __device__ long store(int T) const { return lattice::round64((long)T * (4 * N + 2)); }
  __host__ __device__ long operator()(int T) const { return store(T) + (store_in_lds(N, D) ? 0 : lattice::round64(store_words(N, D))); }
};

// J: lane groups of output symbols (N <= 64 J).  HL: the ring, the rows and the sums are in LDS, else in the clip's workspace
template <int J, bool HL>
__global__ __launch_bounds__(NT) void duration_counts_chain_kernel(DurCountsLaunch a) {
  constexpr int NSM = 16 * J;                    // successors of a wave, at most: ceil(64 J / 4)
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];

  const bio::Clip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = cl.T, N = a.n_pairs + 1, D = a.D, D1 = a.D + 1;
  const int HS = hist_stride(N);
  const long LDR = 4L * N + 2;                   // a frame's record: a[N], R^1[N], bE[N], V[N], KA, KB
  Chain<J> ch(lds, tid, wv, T, N, J);

  // ---- the class table: thread p owns phoneme p here (one slot per thread); a bad one is status 4
  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, a.C, a.o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) { bio::refuse<NT>(a, cl, 0); return; }            // (zeros, status 0)
  // thread q >= 1 owns phoneme q - 1 from here on; its row of dur, outside -1 .. n_rows - 1: status 4
  const bool owner = tid < N;
  int row = -1;
  if (owner && tid > 0) row = a.sym_dur[tid - 1];
  if (__syncthreads_or((row < -1 || row >= a.n_rows) ? 1 : 0)) { bio::refuse<NT>(a, cl, 4); return; }

  unsigned* w0 = a.ws + cl.ws_off;
  const DurCountsHead head{N, D};
  float* rec = (float*)w0;                                     // [T][4 N + 2]
  const unsigned* forced = w0 + bio::tail_forced(head(T), T);
  float* alive = (float*)(lds + fixed_bytes(N) - EXTRA_BYTES);
  float* pub = alive + MAX_SYMBOLS;
  float* ring;                                                 // slot j of symbol q: ring[j HS + q]
  if constexpr (HL) ring = pub + MAX_SYMBOLS;
  else ring = (float*)(w0 + head.store(T));

  // ---- the ring (all 0) and this symbol's row as linear weights: the thread's own words.  O's column stays 0 in every sweep
  float* h = ring + tid;
  float* lr = h + (long)D * HS;                                // lambda_q(j): lr[(j - 1) HS], tau_q: lr[D HS]
  double* ac = (double*)(ring + hist_words(N, D)) + tid;       // the sums of column j: ac[j HS]
  int jl = 0;                                                  // the last age at which a run of this symbol can still end
  if (owner) {
    for (int j = 0; j < D; ++j) h[j * HS] = 0.f;
    for (int j = 0; j < D1; ++j) {
      const float L = row >= 0 ? a.dur[(long)row * D1 + j] : 0.f;
      const float w = tid == 0 ? 0.f : (L == -INFINITY ? 0.f : fminf(fmaxf(expf(L), W_MIN), W_MAX));
      lr[j * HS] = w;
      ac[j * HS] = 0.0;
      if (j < D && w > 0.f) jl = j + 1;
    }
  }
  if (tid < MAX_SYMBOLS) { alive[tid] = tid == 0 ? 1.f : 0.f; pub[tid] = 0.f; }
  ch.stage(a.trans, a.n_pairs, a.o_id, cB[0], cI[0]);          // (ends in a barrier)

  ch.own(a.logits + cl.frame_off * a.ldl, a.ldl, (const float*)(w0 + bio::tail_stat(head(T))), forced);
  const int ns = ch.s_hi - ch.s_lo;
  const float lam1 = owner ? lr[0] : 0.f, lamD = owner ? lr[(D - 1) * HS] : 0.f, tau = owner ? lr[D * HS] : 0.f;
  // every wave takes the largest alive value (the same in every wave) -> the power of two that brings it into [1, 2); CK does the rest
  const auto scale = [&](int& ex) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) m = fmaxf(m, alive[ch.tq[j]]);
    return bigram_sp::unscale(bigram_sp::wave_largest(m), ex);
  };

  Group g;

  // ================================================================================================================ forward sweep
  float Y = 0.f;
  long KA = 0;                                                 // true value = stored 2^KA (the same in every thread)
  int p = 0;                                                   // t mod D
  ch.load_group(0, g);
  ch.to_emissions(g);
  for (int t0 = 0; t0 < T; t0 += GF) {
    Group n;
    const bool more = t0 + GF < T;
    if (more) ch.load_group(t0 + GF, n);
#pragma unroll
    for (int f = 0; f < GF; ++f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        int ex;
        const float sc = scale(ex);
        KA += ex + KS;
        float* r = rec + (long)t * LDR;
        // what this frame starts from, for the succession sums: the scaled vector as the products read it, and its exponent
        if (owner) r[tid] = (ch.endv[tid] * sc) * CK;
        if (tid == 0) r[4 * N] = __int_as_float((int)KA);      // (the low 32 bits: only differences of exponents are needed)
        float acc[J];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = 0.f;
#pragma unroll 4
        for (int s = ch.s_lo; s < ch.s_hi; ++s) {
          const float e = (ch.endv[s] * sc) * CK;
          const float* trow = ch.tab + s * ch.LD;
#pragma unroll
          for (int j = 0; j < J; ++j) acc[j] = fmaf(e, trow[ch.tq[j]], acc[j]);
        }
        ch.exchange(acc);
        if (owner) {
          const float in = ch.summed();
          const float e0 = g.e0[f], e1 = g.e1[f];
          if (tid == 0) {
            const float x = e0 * in;
            ch.endv[0] = x;
            pub[0] = x;
            alive[0] = x;
          } else {
            const float eIk = e1 * CK;
            const float old = h[p * HS] * sc;    // R^D(t-1): the run that is D frames old, what the tail is entered from
            Y = (e1 * tau) * ((Y * sc + lamD * old) * CK);
            const float r1 = jl >= 1 ? e0 * in : 0.f;
            h[p * HS] = r1;
            r[N + tid] = r1;                     // the counting sweep rebuilds the ring from it
            float end = lam1 * r1, mx = r1;
            for (int j0 = 2; j0 <= D; j0 += JU) {
              float hv[JU], lv[JU];
#pragma unroll
              for (int u = 0; u < JU; ++u) {
                const int j = min(j0 + u, D);
                int q = p - (j - 1);
                q = q < 0 ? q + D : q;
                q = j0 + u <= D ? q : p;
                hv[u] = h[q * HS];
                lv[u] = lr[(j - 1) * HS];
              }
#pragma unroll
              for (int u = 0; u < JU; ++u) {
                const int j = min(j0 + u, D);
                const bool inside = j0 + u <= D;
                int q = p - (j - 1);
                q = q < 0 ? q + D : q;
                q = inside ? q : p;
                const float v = inside ? (j <= jl ? (hv[u] * sc) * eIk : 0.f) : r1;
                h[q * HS] = v;
                if (inside) {
                  end = fmaf(lv[u], v, end);
                  mx = fmaxf(mx, v);
                }
              }
            }
            end += Y;
            ch.endv[tid] = end;
            pub[tid] = Y;
            alive[tid] = fmaxf(fmaxf(mx, end), Y);
          }
        }
        p = p + 1 == D ? 0 : p + 1;
        __syncthreads();
      }
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
    }
  }
  // Z = zsum 2^KA: any state may end the clip (every wave computes the same sum)
  double zsum = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < N) zsum += (double)ch.endv[lane + 64 * j];
  zsum = lattice::wave_sum(zsum);
  const double inv_z = zsum > 0.0 ? 1.0 / zsum : 0.0;
  const int ka_end = (int)KA;
  __threadfence_block();
  __syncthreads();                               // the records are read back from here on; end[] becomes u[], the ring Wr

  // =============================================================================================================== backward sweep
  float tile[J][NSM];                            // this thread's succession sums: rows tq[j], successors s_lo + qi
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int qi = 0; qi < NSM; ++qi) tile[j][qi] = 0.f;
  float bX = 1.f, V = 1.f, w1 = lam1;            // bO (q = 0) or bE_q; the tail; Wr^1 of the current frame
  int KB = 0;
  p = (T - 1) % D;
  if (owner) {
    float mx = 1.f;
    if (tid > 0) {
      int q = p;
      for (int j = 0; j < D; ++j) {              // Wr^(j+1)(T-1) = lambda(j + 1), in the slot of the run that began at T - 1 - j
        const float v = lr[j * HS];
        h[q * HS] = v;
        mx = fmaxf(mx, v);
        q = q == 0 ? D - 1 : q - 1;
      }
    }
    pub[tid] = 1.f;
    alive[tid] = mx;
  }
  float ra[J][GF];                               // a_t of this lane's rows and KA_t, a group of frames ahead
  int rk[GF];
  const auto also = [&](float (&oa)[J][GF], int (&ok)[GF]) {
    return [&](int f, int t) {
      const float* r = rec + (long)t * LDR;
#pragma unroll
      for (int j = 0; j < J; ++j) oa[j][f] = r[ch.tq[j]];
      ok[f] = __float_as_int(r[4 * N]);
    };
  };
  const int tl = (T - 1) / GF * GF;              // the last group
  ch.load_group(tl, g, also(ra, rk));
  ch.to_emissions(g);
  for (int t0 = tl; t0 >= 0; t0 -= GF) {
    Group n;
    float ma[J][GF];
    int mk[GF];
    const bool more = t0 > 0;
    if (more) ch.load_group(t0 - GF, n, also(ma, mk));
#pragma unroll
    for (int f = GF - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        // what the counting sweep multiplies frame t's ring with: bE(t), V(t) and their exponent
        float* r = rec + (long)t * LDR;
        if (owner && tid > 0) {
          r[2 * N + tid] = bX;
          r[3 * N + tid] = V;
        }
        if (tid == 0) r[4 * N + 1] = __int_as_float(KB);
        if (t > 0) {                             // (uniform)
          const float e0 = g.e0[f], e1 = g.e1[f];
          if (owner) ch.endv[tid] = e0 * (tid == 0 ? bX : w1);  // u[q]
          __syncthreads();
          int ex;
          const float sc = scale(ex);
          KB += ex + KS;
          // the frame's constant, formed in double and clamped (see the header): applied to a_t first
          const int sh = rk[f] + KB - ka_end;    // (wraps to the true, small difference)
          const float c = (float)fmin(ldexp(inv_z, sh), 0x1p126);
          float v[J], acc[J];
#pragma unroll
          for (int j = 0; j < J; ++j) {
            v[j] = ra[j][f] * c;
            acc[j] = 0.f;
          }
#pragma unroll
          for (int qi = 0; qi < NSM; ++qi) {
            if (qi < ns) {                       // (uniform)
              const float u = (ch.endv[ch.s_lo + qi] * sc) * CK;
              const float* col = ch.tab + ch.s_lo + qi;
#pragma unroll
              for (int j = 0; j < J; ++j) {
                const float pr = col[ch.tq[j] * ch.LD] * u;
                acc[j] += pr;
                tile[j][qi] = fmaf(v[j], pr, tile[j][qi]);
              }
            }
          }
          ch.exchange(acc);
          if (owner) {
            bX = ch.summed();
            if (tid == 0) {
              pub[0] = bX;
              alive[0] = bX;
            } else {
              const float eIk = e1 * CK;
              V = bX + (e1 * tau) * ((V * sc) * CK);
              const float wD = lamD * V;         // Wr^D(t-1), into the slot Wr^1(t) leaves
              float mx = fmaxf(fmaxf(bX, V), wD);
              for (int j0 = 1; j0 < D; j0 += JU) {
                float hv[JU], lv[JU];
#pragma unroll
                for (int u = 0; u < JU; ++u) {
                  const int j = min(j0 + u, D - 1);
                  int q = p - j;
                  q = q < 0 ? q + D : q;
                  q = j0 + u < D ? q : p;
                  hv[u] = h[q * HS];
                  lv[u] = lr[(j - 1) * HS];
                }
#pragma unroll
                for (int u = 0; u < JU; ++u) {
                  const int j = min(j0 + u, D - 1);
                  const bool inside = j0 + u < D;
                  int q = p - j;
                  q = q < 0 ? q + D : q;
                  q = inside ? q : p;
                  const float x = inside ? fmaf(lv[u], bX, (hv[u] * sc) * eIk) : wD;
                  h[q * HS] = x;
                  if (inside) mx = fmaxf(mx, x);
                  if (j0 + u == 1) w1 = x;
                }
              }
              h[p * HS] = wD;
              if (D == 1) w1 = wD;
              pub[tid] = V;
              alive[tid] = mx;
            }
          }
          p = p == 0 ? D - 1 : p - 1;
        }
      }
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
#pragma unroll
      for (int f = 0; f < GF; ++f) {
        rk[f] = mk[f];
#pragma unroll
        for (int j = 0; j < J; ++j) ra[j][f] = ma[j][f];
      }
    }
  }

  // ---- frame 0 starts from the virtual O frame (end_{-1} = (1, 0, ...), KA_0's products are W[O][q] alone): row O, by q's owner
  __syncthreads();                               // (u[] of frame 1 has been read by every wave)
  if (owner) {
    const double k = fmin(ldexp(inv_z, KB - ka_end), 0x1p126);
    double gq = (double)ch.tab[tid] * (double)g.e0[0] * (double)(tid == 0 ? bX : w1) * k;
    gq = gq >= 0.0 ? fmin(gq, 1.0) : 0.0;
    ch.endv[tid] = (float)gq;
  }
  __threadfence_block();
  __syncthreads();                               // (and the backward records are written)
  float* cnt = a.succ + (long)cl.clip * N * N;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int s = lane + 64 * j;
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

  // =============================================================================================================== counting sweep
  // forward again, the owner of a phoneme alone with its ring: no barrier from here on
  if (owner && tid > 0) {
    for (int j = 0; j < D; ++j) h[j * HS] = 0.f;
    Y = 0.f;
    p = 0;
    int kprev = 0;                               // KA_{t-1}
    float q1[GF], qe[GF], qv[GF];
    int qa[GF], qb[GF];
    const auto mine = [&](float (&o1)[GF], float (&oe)[GF], float (&ov)[GF], int (&oa)[GF], int (&ob)[GF]) {
      return [&](int f, int t) {
        const float* r = rec + (long)t * LDR;
        o1[f] = r[N + tid];
        oe[f] = r[2 * N + tid];
        ov[f] = r[3 * N + tid];
        oa[f] = __float_as_int(r[4 * N]);
        ob[f] = __float_as_int(r[4 * N + 1]);
      };
    };
    ch.load_group(0, g, mine(q1, qe, qv, qa, qb));
    ch.to_emissions(g);
    for (int t0 = 0; t0 < T; t0 += GF) {
      Group n;
      float n1[GF], ne[GF], nv[GF];
      int na[GF], nb[GF];
      const bool more = t0 + GF < T;
      if (more) ch.load_group(t0 + GF, n, mine(n1, ne, nv, na, nb));
#pragma unroll
      for (int f = 0; f < GF; ++f) {
        const int t = t0 + f;
        if (t < T) {
          const int ex = qa[f] - kprev - KS;     // the forward sweep's power of two of this frame
          kprev = qa[f];
          const float sc = __int_as_float((127 - ex) << 23);
          const double c = fmin(ldexp(inv_z, qa[f] + qb[f] - ka_end), 0x1p126);
          const double cb = c * (double)qe[f], cv = c * (double)qv[f];
          const float e1 = g.e1[f];
          const float eIk = e1 * CK;
          const float old = h[p * HS] * sc;
          Y = (e1 * tau) * ((Y * sc + lamD * old) * CK);
          const float r1 = q1[f];
          h[p * HS] = r1;
          ac[0] += ((double)r1 * (double)lam1) * (D == 1 ? cv : cb);
          for (int j0 = 2; j0 <= D; j0 += JU) {
            float hv[JU], lv[JU];
            double av[JU];
#pragma unroll
            for (int u = 0; u < JU; ++u) {
              const int j = min(j0 + u, D);
              int q = p - (j - 1);
              q = q < 0 ? q + D : q;
              q = j0 + u <= D ? q : p;
              hv[u] = h[q * HS];
              lv[u] = lr[(j - 1) * HS];
              av[u] = ac[(j - 1) * HS];
            }
#pragma unroll
            for (int u = 0; u < JU; ++u) {
              const int j = min(j0 + u, D);
              const bool inside = j0 + u <= D;
              int q = p - (j - 1);
              q = q < 0 ? q + D : q;
              q = inside ? q : p;
              const float x = inside ? (j <= jl ? (hv[u] * sc) * eIk : 0.f) : r1;
              h[q * HS] = x;
              if (inside) ac[(j - 1) * HS] = av[u] + ((double)x * (double)lv[u]) * (j == D ? cv : cb);
            }
          }
          ac[D * HS] += (double)Y * cv;
          p = p + 1 == D ? 0 : p + 1;
        }
      }
      if (more) {
        ch.to_emissions(n);
        g.take(n);
#pragma unroll
        for (int f = 0; f < GF; ++f) {
          q1[f] = n1[f]; qe[f] = ne[f]; qv[f] = nv[f]; qa[f] = na[f]; qb[f] = nb[f];
        }
      }
    }
    float* dc = a.dur_counts + ((long)cl.clip * a.n_pairs + (tid - 1)) * D1;
    for (int j = 0; j < D1; ++j) dc[j] = (float)ac[j * HS];
  }
  if (wv == 0) bio::write_logz(a, cl, lane, ch.Z, ch.rowmax, forced, fmax(zsum, 1e-300), KA);
}

template <int J>
int launch_chain(const char* fn, const DurCountsLaunch& a, hipStream_t s) {
  const int N = a.n_pairs + 1;
  if (store_in_lds(N, a.D)) {
    if (const int rc = lattice::reserve_lds<duration_counts_chain_kernel<J, true>, MAX_DYN_LDS>(fn)) return rc;
    hipLaunchKernelGGL((duration_counts_chain_kernel<J, true>), dim3(a.n), dim3(NT), lds_bytes(N, a.D), s, a);
  } else {
    if (const int rc = lattice::reserve_lds<duration_counts_chain_kernel<J, false>, MAX_DYN_LDS>(fn)) return rc;
    hipLaunchKernelGGL((duration_counts_chain_kernel<J, false>), dim3(a.n), dim3(NT), lds_bytes(N, a.D), s, a);
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t wfl_decode_duration_counts_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs, int32_t D) {
  if (D < 1 || D > MAX_D) return -1;
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, n_pairs + 1 > MAX_SYMBOLS, DurCountsHead{n_pairs + 1, D});
}

int32_t wfl_decode_duration_counts(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                   const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs,
                                   const float* trans, const int32_t* sym_dur, const float* dur, int32_t n_rows, int32_t D,
                                   float threshold, void* workspace, int64_t workspace_bytes, float* logz, float* succ,
                                   float* dur_counts, int32_t* status, void* stream) {
  const char* fn = "wfl_decode_duration_counts";
  if (D < 1 || D > MAX_D) return lattice::fail(fn, -1, "D must be 1 .. 32");
  if (n_rows < 0) return lattice::fail(fn, -1, "n_rows < 0");
  if (n_rows > 0 && !dur) return lattice::fail(fn, -1, "null dur with n_rows > 0");
  bool any_frame, over;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (!logz || !succ || !status || (n_pairs > 0 && (!pairs || !dur_counts)) || (any_frame && !logits) ||
      bigram_sp::table_missing(trans, any_frame, C, n_pairs, over))
    return lattice::fail(fn, -1, "null device pointer");
  if (any_frame && n_pairs > 0 && !sym_dur) return lattice::fail(fn, -1, "null sym_dur");
  const int N = n_pairs + 1;
  auto a = bio::launch_of<DurCountsLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.trans = trans; a.sym_dur = sym_dur; a.dur = dur; a.n_rows = n_rows; a.D = D;
  a.logz = logz; a.succ = succ; a.dur_counts = dur_counts;
  return bio::run<false>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, DurCountsHead{N, D},
                         [&](const DurCountsLaunch& a, hipStream_t s) {
                           return N <= 64 ? launch_chain<1>(fn, a, s) : (N <= 128 ? launch_chain<2>(fn, a, s) : launch_chain<3>(fn, a, s));
                         });
}

}  // extern "C"
