// Forward-backward over the explicit-duration BIO grammar of wfl_decode_duration: per-frame posteriors of a path decoded under a
// phone-bigram table AND a duration prior per phoneme (wfl_decode_duration_posterior, include/wfl_asr.h).
//
// The sum-product counterpart of csrc/decode_duration.hip, as csrc/decode_bigram_posterior.hip is csrc/decode_bigram.hip's: its symbols,
// states, legality rule, forced frames, virtual O frame, "any state may end the clip", its tables `trans`, `dur` and `sym_dur`, and
// L_q(d) with its tail.  The weight of a legal path is
//     exp(sum_t z[t][c_t] + sum over opened runs trans[previous symbol][opened symbol] + sum over phoneme runs L_q(d)),
// the run in progress at the last frame ends there and pays its L.  With W = exp(trans) (W[O][O] = 1), lambda_q(j) = exp(L_q(j)),
// tau_q = exp(tail_q) (-inf -> 0; all 1 for a phoneme without a row), e the frame's emissions, everything of frame t - 1 on the right:
//     forward    In_q(t)  = sum_s end_s(t-1) W[s][q]                          end(-1) = (1, 0, ...)
//                R_q^1(t) = e_t(B-q) In_q(t);    R_q^j(t) = e_t(I-q) R_q^{j-1}(t-1)   2 <= j <= D
//                Y_q(t)   = e_t(I-q) tau_q (Y_q(t-1) + lambda_q(D) R_q^D(t-1))
//                end_q(t) = sum_j lambda_q(j) R_q^j(t) + Y_q(t);    O(t) = e_t(O) In_O(t);    Z = sum_s end_s(T-1)
//     backward   bE_q(t): after a run of q has ended at t; Wr_q^j(t): t is the j-th frame of a run; V_q(t): inside the tail.
//                At T - 1: bO = bE = V = 1, Wr^j = lambda(j).    u_t[O] = e_t(O) bO(t),  u_t[q] = e_t(B-q) Wr_q^1(t)
//                (bO, bE_1 .. bE_P)(t-1) = W u_t;    V_q(t-1) = bE_q(t-1) + e_t(I-q) tau_q V_q(t)
//                Wr_q^j(t-1) = lambda_q(j) bE_q(t-1) + e_t(I-q) Wr_q^{j+1}(t)  j < D;    Wr_q^D(t-1) = lambda_q(D) V_q(t-1)
// Outputs are wfl_decode_posterior's: logZ; for the class ids[t] of the path, post = (sum_j R_p^j Wr_p^j + Y_p V_p) / Z (O(t) bO(t) / Z on
// an O frame) and cls_post = R^1 Wr^1 / Z on a B frame, the other terms on an I frame.  Both are sums of non-negative products, added in
// double; post is formed as cls_post + the rest, so cls_post <= post holds by construction.
//
// Two kernels.  bio::pre_kernel (csrc/bio_grammar.h; row maxima).  duration_post_chain_kernel, ONE WORKGROUP of 256 threads per clip:
// the chain of csrc/bigram_sumproduct.h -- Chain's LDS carve-up, staging, owner columns, wave slices, emission groups one group ahead,
// exchange and logZ are used as they are; the two frame functions are this file's, because the owner's update and the vector the scale
// is taken from differ (below).  Chain itself is not changed: the two kernels that use it keep their objects.
//
// The run history R^1 .. R^D and, going backward, Wr^1 .. Wr^D are the search's ring: D floats per symbol, entry of the run that began
// at frame s in slot s mod D, word slot HS + q (HS = round_up_64(N)), the symbol's row of linear lambda(1 .. D), tau behind it in the
// same layout.  Going forward, frame t reads slot t mod D (R^D(t-1), what Y is entered from), overwrites it with R^1(t) and multiplies
// the others by e_t(I); going backward, slot t mod D holds Wr^1(t) and becomes Wr^D(t-1).  A slot means the same run in both sweeps, so
// the backward ring takes the forward ring's words once the forward sweep is done.  Ring and rows, (2 D + 1) HS floats, live in LDS
// behind the chain's areas where they fit the CU's 160 KiB, and in the clip's workspace where they do not (hist_in_lds).  The ring is
// addressed memory, never a register array under a run-time index; the kernel uses no scratch
// (profiles/decode_duration_posterior_resources.txt).
//
// The alpha lattice is not stored.  After every forward frame wave 3 copies the ring column of the path's symbol, its Y (O's state on
// an O frame) and the scale exponent into the clip's record, D + 2 words per frame, lane j word j: the copy runs beside the next
// frame's products, off the owner's chain.  Going backward the same lanes read the records a group ahead, multiply them with the
// backward ring's column and V (bO) in double, and lane 0 writes the two posteriors.
//
// Scale.  Every owner publishes, beside end[q] (backward: u[q]), the largest value ALIVE in it: forward max(end, Y, the ring's
// entries), backward max(bE or bO, V, the ring's entries).  Every wave takes the largest of that vector and multiplies what it reads of
// the previous frame by the power of two that brings that largest into [2^-4, 2^-3); the exponents add up in integers.  end[] alone
// (Chain::scale) is not enough here: under a hard minimum of D frames a ring entry whose lambda(j) is 0 does not show in end[] and
// would outgrow the scale by 2^60 per frame while O sits on its floor.  A forward ring entry that can no longer end (lambda(j') = 0 for
// every j' from its age on) is set to 0, so a dead run cannot hold the scale either; backward such an entry is 0 by the recurrence.
// Guards, bigram_sumproduct.h's: an O emission is at least 2^-60 of its frame's row maximum, a finite table entry is clamped to
// [2^-60, 2^60], and so is a finite lambda or tau here; -inf is exactly 0.  Emissions are <= 1.  Bound, with S < 2^-3 the scaled largest:
//     In, bE < N 2^60 S < 2^65,   R^1 < 2^65,   lambda R^1 and lambda bE < 2^125,   Y, V < 2^60 (S + 2^60 S) < 2^118,
//     end < 2^125 + 31 2^57 + 2^118 < 2^126,   Wr < 2^125 + 2^-3
// so every sum stays inside fp32 whatever the logits, the tables and the clip's length, no product is inf and no inf meets a 0.  What
// is smaller than 2^-122 of its frame's largest alive value underflows: its posterior is reported as 0.  (That includes a state below
// a run that is alive but later proves impossible; the guards and this range are what a shared scale in fp32 can carry.)
//
// Before the sweeps the workgroup checks that ids is a path (status 8): wfl_decode_bigram_posterior's per-frame check, and then per
// phoneme run of ids that its length d has lambda(d) > 0 (d > D: lambda(D) > 0 and tau > 0), the run the clip ends in included.
// Workspace per clip with T > 0, in 4-byte words: [records round_up_64(T (D + 2))] [pair | kind << 16 per frame round_up_64(T)] [ring and
// rows round_up_64((2 D + 1) HS) where LDS does not hold them] [row maxima round_up_64(T)] [forced flags round_up_64(T)].
#include "bigram_sumproduct.h"
#include "path_posterior.h"

namespace {

using bigram_sp::Chain;
using bigram_sp::Group;
using bigram_sp::JT;
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
static_assert(MAX_D + 2 <= 64, "a record is written by one wave, a word per lane");

struct DurPostLaunch : bio::PathLaunch {
  const float* trans;    // [N][N], rows the previous symbol
  const int* sym_dur;    // [n_pairs] row of `dur`, -1 none
  const float* dur;      // [n_rows][D + 1]
  int n_rows, D;
};

// dynamic LDS, in bytes: [the chain's areas, bigram_sp::lds_bytes(N)] [alive MAX_SYMBOLS] [Y / V (O: its state) MAX_SYMBOLS] [the ring and
// the symbols' rows, (2 D + 1) HS floats, where they fit]
constexpr int EXTRA_BYTES = 2 * MAX_SYMBOLS * 4;
constexpr int STATIC_BYTES = (MAX_CLASSES + MAX_CLASSES / 32 + 96) * 4;   // the kernel's __shared__ variables (4480 bytes), rounded up
constexpr int MAX_DYN_LDS = LDS_CAP - STATIC_BYTES;
static_assert(bigram_sp::MAX_LDS + EXTRA_BYTES <= MAX_DYN_LDS, "LDS of one CU");

__host__ __device__ inline int fixed_bytes(int N) { return bigram_sp::table_bytes(N) + bigram_sp::FIXED_BYTES + EXTRA_BYTES; }
__host__ __device__ inline int hist_stride(int N) { return (N + 63) / 64 * 64; }
__host__ __device__ inline long hist_words(int N, int D) { return (long)(2 * D + 1) * hist_stride(N); }
__host__ __device__ inline bool hist_in_lds(int N, int D) { return fixed_bytes(N) + hist_words(N, D) * 4 <= MAX_DYN_LDS; }
inline int lds_bytes(int N, int D) { return fixed_bytes(N) + (hist_in_lds(N, D) ? (int)hist_words(N, D) * 4 : 0); }

// head of a clip's workspace, in words
struct DurPostHead {
  int N, D;
  __host__ __device__ long sel(int T) const { return lattice::round64((long)T * (D + 2)); }
  __host__ __device__ long ring(int T) const { return sel(T) + lattice::round64(T); }
  __host__ __device__ long operator()(int T) const { return ring(T) + (hist_in_lds(N, D) ? 0 : lattice::round64(hist_words(N, D))); }
};

// HL: the ring and the rows are in LDS, else in the clip's workspace
template <bool HL>
__global__ __launch_bounds__(NT) void duration_post_chain_kernel(DurPostLaunch a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned used[MAX_CLASSES / 32];
  __shared__ int info[MAX_CLASSES];    // class -> pair | kind << 16 (kind 0 O, 1 B, 2 I); -1 never chosen

  const bio::Clip cl = a.clip[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = cl.T, N = a.n_pairs + 1, D = a.D, D1 = a.D + 1, D2 = a.D + 2;
  const int HS = hist_stride(N);
  float* post = a.post + cl.frame_off;
  float* cls_post = a.cls_post + cl.frame_off;
  Chain<JT> ch(lds, tid, wv, T, N, (N + 63) / 64);

  // ---- the class table: thread p owns phoneme p here (one slot per thread); a bad one is status 4
  int cB[1], cI[1];
  if (bio::class_table<1, NT>(a.pairs, a.n_pairs, a.C, a.o_id, used, info, cB, cI)) { bio::refuse<NT>(a, cl, 4); return; }
  if (T == 0) {
    if (tid == 0) { a.logz[cl.clip] = 0.f; a.status[cl.clip] = 0; }
    return;
  }
  // thread q >= 1 owns phoneme q - 1 from here on; its row of dur, outside -1 .. n_rows - 1: status 4
  const bool owner = tid < N;
  int row = -1;
  if (owner && tid > 0) row = a.sym_dur[tid - 1];
  if (__syncthreads_or((row < -1 || row >= a.n_rows) ? 1 : 0)) { bio::refuse<NT>(a, cl, 4); return; }

  unsigned* w0 = a.ws + cl.ws_off;
  const DurPostHead head{N, D};
  float* rec = (float*)w0;                                     // [T][D + 2]: the ring column, Y (O: its state), the scale exponent
  int* sel = (int*)(w0 + head.sel(T));
  const unsigned* forced = w0 + bio::tail_forced(head(T), T);
  float* alive = (float*)(lds + fixed_bytes(N) - EXTRA_BYTES);
  float* pub = alive + MAX_SYMBOLS;
  float* ring;                                                 // slot j of symbol q: ring[j HS + q]
  if constexpr (HL) ring = pub + MAX_SYMBOLS;
  else ring = (float*)(w0 + head.ring(T));
  const float* rows = ring + (long)D * HS;                     // lambda_q(j): rows[(j - 1) HS + q], tau_q: rows[D HS + q]

  // ---- the ring (all 0) and this symbol's row as linear weights: the thread's own words.  O's column stays 0 in both sweeps
  float* h = ring + tid;
  float* lr = h + (long)D * HS;
  int jl = 0;                                                  // the last age at which a run of this symbol can still end
  if (owner) {
    for (int j = 0; j < D; ++j) h[j * HS] = 0.f;
    for (int j = 0; j < D1; ++j) {
      const float L = row >= 0 ? a.dur[(long)row * D1 + j] : 0.f;
      const float w = tid == 0 ? 0.f : (L == -INFINITY ? 0.f : fminf(fmaxf(expf(L), W_MIN), W_MAX));
      lr[j * HS] = w;
      if (j < D && w > 0.f) jl = j + 1;
    }
  }
  if (tid < MAX_SYMBOLS) { alive[tid] = tid == 0 ? 1.f : 0.f; pub[tid] = 0.f; }
  ch.stage(a.trans, a.n_pairs, a.o_id, cB[0], cI[0]);          // (ends in a barrier)

  // ---- is ids a path of this grammar?  wfl_decode_bigram_posterior's check of every frame on its own ...
  bool bad = false;
  for (int t = tid; t < T; t += NT)
    bad |= bio::path_step_bad(a.ids + cl.frame_off, t, a.C, a.o_id, info, forced, sel, [&](int in, int pin) {
      const int sy = (in >> 16) ? (in & 0xffff) + 1 : 0, psy = (pin >> 16) ? (pin & 0xffff) + 1 : 0;
      return ((in >> 16) == 1 || psy != 0) && !(ch.tab[psy * ch.LD + sy] > 0.f);
    });
  __threadfence_block();
  if (__syncthreads_or(bad ? 1 : 0)) { bio::refuse<NT>(a, cl, 8); return; }
  // ... and every phoneme run's length, by the thread of the run's last frame: d = min(frames, D + 1)
  for (int t = tid; t < T; t += NT) {
    const int se = sel[t];
    if ((se >> 16) == 0 || (t + 1 < T && (sel[t + 1] >> 16) == 2)) continue;
    int d = 1;
    for (int u = t; (sel[u] >> 16) == 2 && d <= D; --u) ++d;
    const float* lq = rows + (se & 0xffff) + 1;
    bad |= d <= D ? !(lq[(d - 1) * HS] > 0.f) : !(lq[(D - 1) * HS] > 0.f && lq[D * HS] > 0.f);
  }
  if (__syncthreads_or(bad ? 1 : 0)) { bio::refuse<NT>(a, cl, 8); return; }

  ch.own(a.logits + cl.frame_off * a.ldl, a.ldl, (const float*)(w0 + bio::tail_stat(head(T))), forced);
  const float lam1 = owner ? lr[0] : 0.f, lamD = owner ? lr[(D - 1) * HS] : 0.f, tau = owner ? lr[D * HS] : 0.f;
  const bool copier = wv == NW - 1 && lane < D2;               // the lanes that write and read the records
  const auto symbol_of = [](int se) { return (se >> 16) ? (se & 0xffff) + 1 : 0; };
  // every wave takes the largest alive value (the same in every wave) -> the power of two that brings it into [1, 2); CK does the rest
  const auto scale = [&](int& ex) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < JT; ++j) m = fmaxf(m, alive[ch.tq[j]]);
    return bigram_sp::unscale(bigram_sp::wave_largest(m), ex);
  };
  // frame t's record of the path's symbol, by the copier lanes, while the ring holds frame t
  const auto copy_record = [&](int t, int se, long ka) {
    if (copier) {
      const int sy = symbol_of(se);
      const float v = lane < D ? ring[lane * HS + sy] : (lane == D ? pub[sy] : __int_as_float((int)ka));
      rec[(long)t * D2 + lane] = v;
    }
  };

  Group g;
  int sl[GF];                                                  // the path's (pair, kind) of the group's frames

  // ================================================================================================================ forward sweep
  float Y = 0.f;
  long KA = 0;                                                 // true value = stored 2^KA (the same in every thread)
  int p = 0;                                                   // t mod D
  int prev_se = 0;
  ch.load_group(0, g, [&](int f, int t) { sl[f] = sel[t]; });
  ch.to_emissions(g);
  for (int t0 = 0; t0 < T; t0 += GF) {
    Group n;
    int ns[GF];
    const bool more = t0 + GF < T;
    if (more) ch.load_group(t0 + GF, n, [&](int f, int t) { ns[f] = sel[t]; });
#pragma unroll
    for (int f = 0; f < GF; ++f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        int ex;
        const float sc = scale(ex);
        if (t > 0) copy_record(t - 1, prev_se, KA);
        KA += ex + KS;
        float acc[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[j] = 0.f;
#pragma unroll 4
        for (int s = ch.s_lo; s < ch.s_hi; ++s) {
          const float e = (ch.endv[s] * sc) * CK;
          const float* trow = ch.tab + s * ch.LD;
#pragma unroll
          for (int j = 0; j < JT; ++j)
            if (j < ch.nj) acc[j] = fmaf(e, trow[ch.tq[j]], acc[j]);   // (uniform)
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
            float end = lam1 * r1, mx = r1;
            // the runs that began at t - j + 1, j = 2 .. D, JU at a time: the loads of a group are in flight together.  A j past D reads
            // and rewrites the entry just written
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
        prev_se = sl[f];
        __syncthreads();
      }
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
#pragma unroll
      for (int f = 0; f < GF; ++f) sl[f] = ns[f];
    }
  }
  copy_record(T - 1, prev_se, KA);
  // Z = zsum 2^KA: any state may end the clip (every wave computes the same sum)
  double zsum = 0.0;
#pragma unroll
  for (int j = 0; j < JT; ++j)
    if (lane + 64 * j < N) zsum += (double)ch.endv[lane + 64 * j];
  zsum = lattice::wave_sum(zsum);
  const double inv_z = zsum > 0.0 ? 1.0 / zsum : 0.0;
  const int ka_end = (int)KA;
  __threadfence_block();
  __syncthreads();                               // the records are read back from here on; end[] becomes u[], the ring Wr

  // =============================================================================================================== backward sweep
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
  float rr[GF];                                  // the copier lanes' words of the group's records
  const auto also = [&](int (&s)[GF], float (&r)[GF]) {
    return [&](int f, int t) {
      s[f] = sel[t];
      r[f] = copier ? rec[(long)t * D2 + lane] : 0.f;
    };
  };
  // gamma of the path's class at t from its record and the backward ring's column, by wave NW - 1 in double
  const auto gamma = [&](int t, int se, float r, int kb) {
    if (wv == NW - 1) {
      const int sy = symbol_of(se), kind = se >> 16;
      double pr = 0.0;
      if (lane < D) pr = (double)r * (double)ring[lane * HS + sy];
      else if (lane == D) pr = (double)r * (double)pub[sy];
      const int ka = __shfl(__float_as_int(r), D1);
      const double first = __shfl(pr, p);                       // the run that opens at t: slot t mod D
      const double rest = lattice::wave_sum(lane == p ? 0.0 : pr);
      if (lane == 0) {
        const double k = ldexp(inv_z, ka + kb - ka_end);        // (the exponents wrap to the true, small difference)
        const double c = kind == 1 ? first : (kind == 2 ? rest : first + rest);
        double gc = c * k, gp = gc + (first + rest - c) * k;
        gc = gc >= 0.0 ? fmin(gc, 1.0) : 0.0;
        gp = gp >= 0.0 ? fmin(gp, 1.0) : 0.0;
        post[t] = (float)gp;
        cls_post[t] = (float)gc;
      }
    }
  };
  const int tl = (T - 1) / GF * GF;              // the last group
  ch.load_group(tl, g, also(sl, rr));
  ch.to_emissions(g);
  for (int t0 = tl; t0 >= 0; t0 -= GF) {
    Group n;
    int ns[GF];
    float nr[GF];
    const bool more = t0 > 0;
    if (more) ch.load_group(t0 - GF, n, also(ns, nr));
#pragma unroll
    for (int f = GF - 1; f >= 0; --f) {
      const int t = t0 + f;
      if (t < T) {                               // (uniform)
        if (t > 0) {                             // (uniform)
          const float e0 = g.e0[f], e1 = g.e1[f];
          if (owner) ch.endv[tid] = e0 * (tid == 0 ? bX : w1);  // u[q]
          __syncthreads();
          int ex;
          const float sc = scale(ex);
          gamma(t, sl[f], rr[f], KB);
          KB += ex + KS;
          float acc[JT];
#pragma unroll
          for (int j = 0; j < JT; ++j) acc[j] = 0.f;
#pragma unroll 4
          for (int q = ch.s_lo; q < ch.s_hi; ++q) {
            const float u = (ch.endv[q] * sc) * CK;
            const float* col = ch.tab + q;
#pragma unroll
            for (int j = 0; j < JT; ++j)
              if (j < ch.nj) acc[j] = fmaf(col[ch.tq[j] * ch.LD], u, acc[j]);   // (uniform)
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
              // Wr^j(t-1), j = 1 .. D - 1, in the slot of the run that began at t - j; a j past D - 1 rewrites slot t mod D
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
                  const float v = inside ? fmaf(lv[u], bX, (hv[u] * sc) * eIk) : wD;
                  h[q * HS] = v;
                  if (inside) mx = fmaxf(mx, v);
                  if (j0 + u == 1) w1 = v;
                }
              }
              h[p * HS] = wD;
              if (D == 1) w1 = wD;
              pub[tid] = V;
              alive[tid] = mx;
            }
          }
          p = p == 0 ? D - 1 : p - 1;
        } else {
          __syncthreads();
          gamma(0, sl[f], rr[f], KB);
        }
      }
    }
    if (more) {
      ch.to_emissions(n);
      g.take(n);
#pragma unroll
      for (int f = 0; f < GF; ++f) {
        sl[f] = ns[f];
        rr[f] = nr[f];
      }
    }
  }
  if (wv == 0) bio::write_logz(a, cl, lane, ch.Z, ch.rowmax, forced, fmax(zsum, 1e-300), KA);
}

}  // namespace

extern "C" {

int64_t wfl_decode_duration_posterior_workspace_bytes(const int32_t* n_frames_host, int32_t n_clips, int32_t n_pairs, int32_t D) {
  if (D < 1 || D > MAX_D) return -1;
  return bio::workspace_bytes(n_frames_host, n_clips, n_pairs, n_pairs + 1 > MAX_SYMBOLS, DurPostHead{n_pairs + 1, D});
}

int32_t wfl_decode_duration_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                      const int32_t* n_frames_host, int32_t n_clips, const int32_t* pairs, int32_t n_pairs,
                                      const float* trans, const int32_t* sym_dur, const float* dur, int32_t n_rows, int32_t D,
                                      float threshold, const int32_t* ids, void* workspace, int64_t workspace_bytes, float* logz,
                                      float* post, float* cls_post, int32_t* status, void* stream) {
  const char* fn = "wfl_decode_duration_posterior";
  if (D < 1 || D > MAX_D) return lattice::fail(fn, -1, "D must be 1 .. 32");
  if (n_rows < 0) return lattice::fail(fn, -1, "n_rows < 0");
  if (n_rows > 0 && !dur) return lattice::fail(fn, -1, "null dur with n_rows > 0");
  bool any_frame, over;
  if (const int rc = bio::check_args(fn, C, o_id, ldl, frame_off_host, n_frames_host, n_clips, n_pairs, 0.f, threshold, any_frame)) return rc;
  if (n_clips == 0) return 0;
  if (bio::path_pointer_missing(logits, pairs, n_pairs, ids, logz, post, cls_post, status, any_frame) ||
      bigram_sp::table_missing(trans, any_frame, C, n_pairs, over))
    return lattice::fail(fn, -1, "null device pointer");
  if (any_frame && n_pairs > 0 && !sym_dur) return lattice::fail(fn, -1, "null sym_dur");
  const int N = n_pairs + 1;
  auto a = bio::launch_of<DurPostLaunch>(logits, ldl, C, o_id, pairs, n_pairs, threshold, status);
  a.trans = trans; a.sym_dur = sym_dur; a.dur = dur; a.n_rows = n_rows; a.D = D;
  a.ids = ids; a.logz = logz; a.post = post; a.cls_post = cls_post;
  return bio::run<false>(fn, a, over, frame_off_host, n_frames_host, n_clips, workspace, workspace_bytes, stream, DurPostHead{N, D},
                         [&](const DurPostLaunch& a, hipStream_t s) {
                           if (hist_in_lds(N, D)) {
                             if (const int rc = lattice::reserve_lds<duration_post_chain_kernel<true>, MAX_DYN_LDS>(fn)) return rc;
                             hipLaunchKernelGGL(duration_post_chain_kernel<true>, dim3(a.n), dim3(NT), lds_bytes(N, D), s, a);
                           } else {
                             if (const int rc = lattice::reserve_lds<duration_post_chain_kernel<false>, MAX_DYN_LDS>(fn)) return rc;
                             hipLaunchKernelGGL(duration_post_chain_kernel<false>, dim3(a.n), dim3(NT), lds_bytes(N, D), s, a);
                           }
                           return 0;
                         });
}

}  // extern "C"
