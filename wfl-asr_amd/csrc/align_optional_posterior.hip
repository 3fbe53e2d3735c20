// wfl_align_optional_posterior (include/wfl_asr.h): csrc/align_posterior.h's kernel with the skip arcs of wfl_align_optional (OPT), with
// and without start windows.  A translation unit of its own, as csrc/align_min_duration_posterior.hip is: the objects of the other
// entries of that header keep the code they had.
#include "align_posterior.h"

// PostLayout as wfl_align_posterior's: a clip with 0 < T < N has its floats there already, and may have a path here
extern "C" int64_t wfl_align_optional_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_floats);
}

extern "C" {

int32_t wfl_align_optional_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                     const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                     const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                     const int32_t* tok_opt, float skip_penalty, const int32_t* tok, void* workspace,
                                     int64_t workspace_bytes, float* logz, float* keep_post, float* tok_post, float* start_mean,
                                     float* start_sd, int32_t* status, void* stream) {
  const char* fn = "wfl_align_optional_posterior";
  return tok_win ? posterior_batch<true, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host,
                                                      tok_cls, tok_win, nullptr, gap_cls, n_clips, tok, workspace, workspace_bytes, logz,
                                                      tok_post, start_mean, start_sd, status, stream, tok_opt, skip_penalty, keep_post)
                 : posterior_batch<false, false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host,
                                                       tok_cls, nullptr, nullptr, gap_cls, n_clips, tok, workspace, workspace_bytes, logz,
                                                       tok_post, start_mean, start_sd, status, stream, tok_opt, skip_penalty, keep_post);
}

}  // extern "C"
