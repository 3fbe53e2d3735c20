// What the two entries that score a decoded path share -- wfl_decode_posterior (csrc/decode_posterior.hip) and
// wfl_decode_bigram_posterior (csrc/decode_bigram_posterior.hip) -- defined ONCE: the launch fields of the path and its outputs, the head
// of a clip's workspace, the per-frame part of the check that ids is a path, the alpha records read back a group ahead, and gamma of the
// path's class from a record and the owner's beta.  The sweeps are each file's own.  wfl_decode_duration_posterior
// (csrc/decode_duration_posterior.hip) takes the launch fields, path_step_bad and path_pointer_missing from here; its records, its
// workspace head and its gamma are its own (a record there is a ring column, not two states).
#pragma once
#include "bio_grammar.h"

namespace bio {

struct PathLaunch : Launch {
  const int* ids;
  float *logz, *post, *cls_post;
};

// head of a clip's workspace, in words: the alpha records (alpha(B-p) or alpha(O), alpha(I-p) or 0, scale exponent per frame), then the
// path's pair | kind << 16 per frame, each rounded up to 64
__host__ __device__ inline long off_sel(int T) { return round64(3L * T); }
struct PathHead {
  __host__ __device__ long operator()(int T) const { return off_sel(T) + round64(T); }
};

// ---- is ids[t] a step of a path?  A class of the table, I-p only after B-p / I-p, O on a forced frame; opens(in, pin) -> true when the
// grammar at hand refuses the run that frame t opens (in, pin: info[] of the class and of the previous one, kind 0 or 1 in `in`).  A
// previous class outside the table is found at its own frame.  Leaves sel[t] = pair | kind << 16.  -> true: not a path (status 8)
template <class Opens>
static __device__ __forceinline__ bool path_step_bad(const int* ids, int t, int C, int o_id, const int* info, const unsigned* forced, int* sel,
                                                     Opens opens) {
  const int c = ids[t], pc = t ? ids[t - 1] : o_id;
  const int in = (c >= 0 && c < C) ? info[c] : -1;
  const int pin = (pc >= 0 && pc < C) ? info[pc] : -1;
  bool bad = in < 0;
  if (in >= 0 && pin >= 0) bad = (in >> 16) == 2 ? ((pin >> 16) == 0 || (pin & 0xffff) != (in & 0xffff)) : opens(in, pin);
  if (in > 0 && forced[t]) bad = true;                         // (in == 0 is O)
  sel[t] = in < 0 ? 0 : in;
  return bad;
}

// ---- the alpha records of the D frames from t0 on
template <int D>
static __device__ __forceinline__ void load_rec(const float* rec, int t0, int T, float (&o0)[D], float (&o1)[D], float (&o2)[D]) {
#pragma unroll
  for (int f = 0; f < D; ++f) {
    const float* r = rec + 3L * min(t0 + f, T - 1);
    o0[f] = r[0];
    o1[f] = r[1];
    o2[f] = r[2];
  }
}

// ---- gamma of the path's class from its record (r0, r1, r2) and the owner's beta b 2^KB, in double: *post = gamma(B-p) + gamma(I-p)
// (gamma(O) on an O frame), *cls_post = gamma of the class itself (kind 2: I)
static __device__ __forceinline__ void write_gamma(float r0, float r1, float r2, int kind, float b, double inv_zm, int KB, int ka_end,
                                                   float* post, float* cls_post) {
  const int sh = __float_as_int(r2) + KB - ka_end;             // (wraps to the true, small difference)
  const double k = ldexp((double)b * inv_zm, sh);
  double gp = (double)(r0 + r1) * k, gc = (double)(kind == 2 ? r1 : r0) * k;
  gp = gp >= 0.0 ? fmin(gp, 1.0) : 0.0;                        // (a NaN of an overflowed clip is reported as 0)
  gc = gc >= 0.0 ? fmin(gc, 1.0) : 0.0;
  *post = (float)gp;
  *cls_post = (float)gc;
}

// (host) the device pointers both entries need
inline bool path_pointer_missing(const float* logits, const int* pairs, int n_pairs, const int* ids, const float* logz, const float* post,
                                 const float* cls_post, const int* status, bool any_frame) {
  return !logz || !status || (n_pairs > 0 && !pairs) || (any_frame && (!logits || !ids || !post || !cls_post));
}

}  // namespace bio
