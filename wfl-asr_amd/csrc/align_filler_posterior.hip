// wfl_align_filler_posterior (include/wfl_asr.h): csrc/align_posterior.h's kernel with the filler emission of wfl_align_filler (FILL),
// with and without start windows, and the end moments of every token.  A translation unit of its own, as
// csrc/align_optional_posterior.hip is: the objects of the other entries of that header keep the code they had.
#include "align_posterior.h"

// wfl_align_posterior's floats and round64(T) more per clip: the filler emission of every frame (clip_floats_fill)
extern "C" int64_t wfl_align_filler_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_floats_fill);
}

extern "C" {

int32_t wfl_align_filler_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                   const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                   const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                   const int32_t* tok_fill, float filler_penalty, const int32_t* tok, void* workspace,
                                   int64_t workspace_bytes, float* logz, float* tok_post, float* start_mean, float* start_sd,
                                   float* end_mean, float* end_sd, int32_t* status, void* stream) {
  const char* fn = "wfl_align_filler_posterior";
  return tok_win ? posterior_batch<true, false, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host,
                                                             n_tok_host, tok_cls, tok_win, nullptr, gap_cls, n_clips, tok, workspace,
                                                             workspace_bytes, logz, tok_post, start_mean, start_sd, status, stream,
                                                             nullptr, 0.f, nullptr, tok_fill, filler_penalty, end_mean, end_sd)
                 : posterior_batch<false, false, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host,
                                                              n_tok_host, tok_cls, nullptr, nullptr, gap_cls, n_clips, tok, workspace,
                                                              workspace_bytes, logz, tok_post, start_mean, start_sd, status, stream,
                                                              nullptr, 0.f, nullptr, tok_fill, filler_penalty, end_mean, end_sd);
}

}  // extern "C"
