// wfl_align_posterior and wfl_align_posterior_windowed (include/wfl_asr.h): the entries of csrc/align_posterior.h's kernel without
// minimum durations.  wfl_align_min_duration_posterior is csrc/align_min_duration_posterior.hip.
#include "align_posterior.h"

extern "C" int64_t wfl_align_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host, int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_floats);
}

extern "C" {

int32_t wfl_align_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                            const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host, const int32_t* tok_cls,
                            const int32_t* gap_cls, int32_t n_clips, const int32_t* tok, void* workspace, int64_t workspace_bytes,
                            float* logz, float* tok_post, float* start_mean, float* start_sd, int32_t* status, void* stream) {
  return posterior_batch<false, false>("wfl_align_posterior", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host,
                                       n_tok_host, tok_cls, nullptr, nullptr, gap_cls, n_clips, tok, workspace, workspace_bytes, logz,
                                       tok_post, start_mean, start_sd, status, stream);
}

int32_t wfl_align_posterior_windowed(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                     const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                     const int32_t* tok_cls, const int32_t* tok_win, const int32_t* gap_cls, int32_t n_clips,
                                     const int32_t* tok, void* workspace, int64_t workspace_bytes, float* logz, float* tok_post,
                                     float* start_mean, float* start_sd, int32_t* status, void* stream) {
  return posterior_batch<true, false>("wfl_align_posterior_windowed", logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host,
                                      n_tok_host, tok_cls, tok_win, nullptr, gap_cls, n_clips, tok, workspace, workspace_bytes, logz,
                                      tok_post, start_mean, start_sd, status, stream);
}

}  // extern "C"
