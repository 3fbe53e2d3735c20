// What the two sum-product chain kernels over the phone-bigram grammar share -- bigram_post_chain_kernel (csrc/decode_bigram_posterior.hip,
// the posteriors of a path) and bigram_counts_chain_kernel (csrc/decode_bigram_counts.hip, the expected successions) -- defined ONCE: the
// workgroup's shape, the table in LDS as clamped linear weights with its odd row stride, and the power-of-two scale of a frame's vector.
// The grammar, the pre-pass and the host driver are csrc/bio_grammar.h's.
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

}  // namespace bigram_sp
