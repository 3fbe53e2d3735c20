// The sum-product chain over the phone-bigram grammar, written ONCE for the two kernels that run it -- bigram_post_chain_kernel
// (csrc/decode_bigram_posterior.hip, the posteriors of a path; its header comment is the definition of the recurrences, the guards and
// the scaling) and bigram_counts_chain_kernel (csrc/decode_bigram_counts.hip, the expected successions).  A guard, a scale rule or a
// forced-frame rule changed here is changed for both.  The grammar, the pre-pass, the logZ tail and the host driver are
// csrc/bio_grammar.h's.  duration_post_chain_kernel (csrc/decode_duration_posterior.hip, the posteriors under a duration prior) uses
// Chain's carve-up, stage, own, load_group / to_emissions, exchange / summed, unscale and wave_largest as they are and writes its own
// two frames: its owner carries a run history, and its scale is taken from everything alive in the owners, not from end[] alone.
//
// Pieces, in the order a kernel uses them:
//   the workgroup's shape (also that of csrc/decode_bigram.hip, the max-product search, which takes the four constants from here and
//   keeps its own staging and slices: its object is the one it was), the LDS layout, stage_table, wave_largest, unscale
//   Chain<J>          a clip's chain, J lane groups of output symbols: the LDS carve-up, stage (symbols, table, virtual O frame), own
//                     (owner columns, wave slice, tq[J]), load_group / to_emissions (a Group of D frames, one group ahead of the chain),
//                     forward_frame, end_forward (zsum, inv_zm, ka_end), backward_publish / backward_update (together: backward_frame),
//                     write_logz
// A kernel keeps its launch struct, its workspace head, the loops over the groups and what it records: forward_frame calls
// before(sc) ahead of the products (the counts kernel's scaled vector and KA_t) and after() behind the owner's update (the posterior
// kernel's record of the path's symbol).  The backward frame's row-wise products are the kernel's own loop (the posterior kernel's fmaf
// chain and the counts kernel's product shared with its register tile round differently), between backward_publish and
// backward_update or, as one call, handed to backward_frame as products(sc, acc).  The posterior kernel calls the two halves: with its
// loop inside a callable it was measured 1.4 % slower at N = 192 (profiles/bigram_sumproduct_ab.txt).  nj: the lane groups in use; a
// kernel instantiated per J passes the constant J and the predicate folds away.  There is no run-time switch on the chain.
#pragma once
#include "bio_grammar.h"
#include "wfl_asr.h"

namespace bigram_sp {

constexpr int MAX_SYMBOLS = WFL_DECODE_BIGRAM_MAX_SYMBOLS;
constexpr int NT = 256;                      // threads per clip
constexpr int NW = NT / 64;                  // slices of the summed-over symbols
constexpr int JT = (MAX_SYMBOLS + 63) / 64;  // output symbols per lane
static_assert(MAX_SYMBOLS <= NT, "one owner thread per symbol");

constexpr float W_MIN = 0x1p-60f;   // floor of an O emission and of a finite table entry
constexpr float W_MAX = 0x1p60f;    // ceiling of a table entry

// dynamic LDS, in bytes: [table N rows of LD floats] [partial sums NW x MAX_SYMBOLS] [end / u MAX_SYMBOLS] [B class, I class per symbol]
__host__ __device__ inline int row_stride(int N) { return N | 1; }
__host__ __device__ inline int table_bytes(int N) { return (N * row_stride(N) * 4 + 15) / 16 * 16; }
constexpr int FIXED_BYTES = (NW + 3) * MAX_SYMBOLS * 4;
inline int lds_bytes(int N) { return table_bytes(N) + FIXED_BYTES; }
constexpr int MAX_LDS = (MAX_SYMBOLS * (MAX_SYMBOLS | 1) * 4 + 15) / 16 * 16 + FIXED_BYTES;
static_assert(MAX_LDS + (lattice::MAX_CLASSES + lattice::MAX_CLASSES / 32 + 16) * 4 <= 160 * 1024, "LDS of one CU");

// the table as linear weights: -inf is exactly 0, a finite entry is clamped to [2^-60, 2^60], O after O is 1
static __device__ __forceinline__ void stage_table(const float* trans, int N, float* tab) {
  const int LD = row_stride(N);
  for (int e = threadIdx.x; e < N * N; e += NT) {
    const float v = trans[e];
    const float w = e == 0 ? 1.f : (v == -INFINITY ? 0.f : fminf(fmaxf(expf(v), W_MIN), W_MAX));
    tab[(e / N) * LD + e % N] = w;
  }
}

// ---- every lane gets the wave's maximum: DPP inside a row of 16, the four row maxima through SGPRs
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)));
}

__device__ __forceinline__ float wave_largest(float v) {
  v = dpp_max<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_max<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_max<0x141>(v);   // row_half_mirror: the other quad of the 8
  v = dpp_max<0x140>(v);   // row_mirror: the other 8 of the 16
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// x = f 2^e, f in [1, 2): e into `ex`, -> 2^-e.  The exponent is kept inside the normal range, so a vector that is all zero (a table
// without a finite way into O: refused by the Python layer) stays zero instead of turning into NaN.
__device__ __forceinline__ float unscale(float x, int& ex) {
  int be = __builtin_amdgcn_readfirstlane((__float_as_int(x) >> 23) & 0xff);
  be = min(max(be, 1), 253);
  ex = be - 127;
  return __int_as_float((254 - be) << 23);
}

constexpr int D = 8;                         // frames per emission group

// a group of D frames of the owner's emissions: raw logits, row maxima and forced flags until to_emissions
struct Group {
  float e0[D], e1[D], mx[D];
  unsigned fc[D];
  __device__ __forceinline__ void take(const Group& n) {
#pragma unroll
    for (int f = 0; f < D; ++f) { e0[f] = n.e0[f]; e1[f] = n.e1[f]; }
  }
};

struct Nothing {
  template <class... A>
  __device__ __forceinline__ void operator()(A...) const {}
};

template <int J>
struct Chain {
  const int tid, lane, wv, T, N, LD, nj;
  float *tab, *pv, *endv;                        // the table; partial sums [NW][MAX_SYMBOLS]; end[] going forward, u[] going backward
  int *symB, *symI;
  const float *Z, *rowmax, *mine;
  const unsigned* forced;
  long ldl;
  int o_id;
  bool owner, hasI;                              // thread q < N owns symbol q
  int col0, col1;                                // its logits columns: O (q = 0) or B-q, and I-q
  int s_lo, s_hi, tq[J];                         // the wave's slice of the summed-over symbols, the lane's output symbols
  float x0, x1;                                  // forward: O's state (q = 0) or B-q's, I-q's (0 for O and without an I class)
  long KA;                                       // true alpha = x 2^KA (the same in every thread)
  float bX;                                      // backward: beta(O), or beta(B-q) = beta(I-q): the same successors
  int KB;                                        // true beta = b 2^KB (low 32 bits)
  double zsum, inv_zm;                           // Z = zsum 2^KA
  int ka_end;

  // the LDS carve-up
  __device__ __forceinline__ Chain(unsigned char* lds, int tid, int wv, int T, int N, int nj)
      : tid(tid), lane(tid & 63), wv(wv), T(T), N(N), LD(row_stride(N)), nj(nj) {
    tab = (float*)lds;
    pv = (float*)(lds + table_bytes(N));
    endv = pv + NW * MAX_SYMBOLS;
    symB = (int*)(endv + MAX_SYMBOLS);
    symI = symB + MAX_SYMBOLS;
  }

  // the symbols' classes (this thread's phoneme: cB, cI of bio::class_table), the table and the virtual O frame, into LDS
  __device__ __forceinline__ void stage(const float* trans, int n_pairs, int o_id_, int cB, int cI) {
    o_id = o_id_;
    if (tid < n_pairs) { symB[tid + 1] = cB; symI[tid + 1] = cI; }
    if (tid == 0) { symB[0] = o_id; symI[0] = bio::NO_CLASS; }
    stage_table(trans, N, tab);
    if (tid < MAX_SYMBOLS) endv[tid] = tid == 0 ? 1.f : 0.f;
    __syncthreads();
  }

  // the owner's columns of the clip's logits Z, the wave's slice, the lane's output symbols
  __device__ __forceinline__ void own(const float* Z_, long ldl_, const float* rowmax_, const unsigned* forced_) {
    Z = Z_; ldl = ldl_; rowmax = rowmax_; forced = forced_;
    owner = tid < N;
    const int myB = owner ? symB[tid] : o_id, myI = owner ? symI[tid] : bio::NO_CLASS;
    hasI = myI != bio::NO_CLASS;
    col0 = myB;
    col1 = hasI ? myI : o_id;                    // (a state that does not exist reads O's column and gets emission 0)
    const int NS = (N + NW - 1) / NW;
    s_lo = min(wv * NS, N);
    s_hi = min(s_lo + NS, N);
#pragma unroll
    for (int j = 0; j < J; ++j) tq[j] = min(lane + 64 * j, N - 1);   // (a lane past N repeats the last symbol and writes nothing)
    mine = pv + tid;
  }

  // a group of D frames from t0 on: the raw logits, the row maxima, the forced flags; also(f, t): what else the kernel loads per frame
  template <class Also = Nothing>
  __device__ __forceinline__ void load_group(int t0, Group& g, Also also = Also()) const {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const int t = min(t0 + f, T - 1);          // (the tail of the last group re-reads the last row; it is never used)
      const float* z = Z + (long)t * ldl;
      g.e0[f] = z[col0];
      g.e1[f] = z[col1];
      g.mx[f] = rowmax[t];
      g.fc[f] = forced[t];
      also(f, t);
    }
  }
  // ... turned into emissions in place, off the chain
  __device__ __forceinline__ void to_emissions(Group& g) const {
#pragma unroll
    for (int f = 0; f < D; ++f) {
      const bool frc = g.fc[f] != 0;
      const float x = expf(g.e0[f] - g.mx[f]);
      g.e0[f] = tid == 0 ? (frc ? 1.f : fmaxf(x, W_MIN)) : (frc ? 0.f : x);
      g.e1[f] = (frc || !hasI) ? 0.f : expf(g.e1[f] - g.mx[f]);
    }
  }

  // every wave takes the largest of the published vector (the same value in every wave) -> the power of two that brings it into [1, 2)
  __device__ __forceinline__ float scale(int& ex) const {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) m = fmaxf(m, endv[tq[j]]);
    return unscale(wave_largest(m), ex);
  }
  // the four partial sums per symbol through LDS, one barrier, added by the owner in a fixed order
  __device__ __forceinline__ void exchange(const float (&acc)[J]) const {
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (lane + 64 * j < N) pv[wv * MAX_SYMBOLS + lane + 64 * j] = acc[j];
    __syncthreads();
  }
  __device__ __forceinline__ float summed() const {
    return (mine[0] + mine[MAX_SYMBOLS]) + (mine[2 * MAX_SYMBOLS] + mine[3 * MAX_SYMBOLS]);
  }

  __device__ __forceinline__ void start_forward() {
    x0 = tid == 0 ? 1.f : 0.f;                   // the virtual O frame
    x1 = 0.f;
    KA = 0;
  }
  // one frame forward with the emissions (e0, e1): scale, this wave's partial products by columns, exchange, the owner's update, end[]
  template <class Before, class After>
  __device__ __forceinline__ void forward_frame(float e0, float e1, Before before, After after) {
    int ex;
    const float sc = scale(ex);
    KA += ex;
    before(sc);
    float acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0.f;
#pragma unroll 4
    for (int s = s_lo; s < s_hi; ++s) {
      const float e = endv[s] * sc;
      const float* row = tab + s * LD;
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (j < nj) acc[j] = fmaf(e, row[tq[j]], acc[j]);   // (uniform)
    }
    exchange(acc);
    if (owner) {
      const float in = summed();
      const float both = (x0 + x1) * sc;         // what I-q continues from
      x1 = e1 * both;                            // (O: e1 is 0)
      x0 = e0 * in;
      endv[tid] = x0 + x1;
      after();
    }
    __syncthreads();
  }
  // Z = zsum 2^KA, every state may end the clip (every thread computes the same sum); beta at T - 1 = 1
  __device__ __forceinline__ void end_forward() {
    double zs = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (lane + 64 * j < N) zs += (double)endv[lane + 64 * j];
    zsum = lattice::wave_sum(zs);
    inv_zm = 1.0 / zsum;
    ka_end = (int)KA;
    __threadfence_block();
    __syncthreads();                             // the kernel's records are read back from here on, and end[] becomes u[]
    bX = 1.f;
    KB = 0;
  }

  // one frame backward, from t to t - 1, with frame t's emissions (e0, e1), in two halves round the kernel's own loop over this wave's
  // partial products by rows (the successors [s_lo, s_hi), lane l the rows tq[]): publish u and scale -> sc; then exchange, the owner's beta
  __device__ __forceinline__ float backward_publish(float e0, float e1, float& pI) {
    pI = 0.f;
    if (owner) {
      endv[tid] = e0 * bX;                       // u[q]
      pI = e1 * bX;
    }
    __syncthreads();
    int ex;
    const float sc = scale(ex);
    KB += ex;
    return sc;
  }
  __device__ __forceinline__ void backward_update(const float (&acc)[J], float pI, float sc) {
    exchange(acc);
    if (owner) bX = summed() + pI * sc;
  }
  // ... or as one call round products(sc, acc)
  template <class Products>
  __device__ __forceinline__ void backward_frame(float e0, float e1, Products products) {
    float pI, acc[J];
    const float sc = backward_publish(e0, e1, pI);
    products(sc, acc);
    backward_update(acc, pI, sc);
  }

  // logZ and status 0, by wave 0
  template <class L>
  __device__ __forceinline__ void write_logz(const L& a, const bio::Clip& cl) const {
    if (wv == 0) bio::write_logz(a, cl, lane, Z, rowmax, forced, zsum, KA);
  }
};

// ---- host: the entry's checks of the symbol cap and of the table pointer (over: status 2, as over the class cap; the table is read only
// when the clips are scored) -> true: the table is needed and null
inline bool table_missing(const float* trans, bool any_frame, int C, int n_pairs, bool& over) {
  over = n_pairs + 1 > MAX_SYMBOLS;
  return any_frame && !trans && !bio::refused_status(C, n_pairs, over);
}

}  // namespace bigram_sp
