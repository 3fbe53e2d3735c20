// wfl_align_min_duration_posterior (include/wfl_asr.h): csrc/align_posterior.h's kernel with the minimum-duration chain (MIND), with and
// without start windows.  Compiled without the SLP vectoriser (build.py): with it, the chain's shifts and renormalisations become
// packed-f32 adds that take the high half of a register pair into the low lane, which the build refuses on gfx950.
#include "align_posterior.h"

extern "C" int64_t wfl_align_min_duration_posterior_workspace_bytes(const int32_t* n_frames_host, const int32_t* n_tok_host,
                                                                    int32_t n_clips) {
  return clips_workspace_bytes(n_frames_host, n_tok_host, n_clips, clip_floats_min);
}

extern "C" {

int32_t wfl_align_min_duration_posterior(const float* logits, int64_t ldl, int32_t C, int32_t o_id, const int64_t* frame_off_host,
                                         const int32_t* n_frames_host, const int32_t* tok_off_host, const int32_t* n_tok_host,
                                         const int32_t* tok_cls, const int32_t* tok_win, const int32_t* tok_min, const int32_t* gap_cls,
                                         int32_t n_clips, const int32_t* tok, void* workspace, int64_t workspace_bytes, float* logz,
                                         float* tok_post, float* start_mean, float* start_sd, int32_t* status, void* stream) {
  const char* fn = "wfl_align_min_duration_posterior";
  return tok_win ? posterior_batch<true, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                                               tok_win, tok_min, gap_cls, n_clips, tok, workspace, workspace_bytes, logz, tok_post,
                                               start_mean, start_sd, status, stream)
                 : posterior_batch<false, true>(fn, logits, ldl, C, o_id, frame_off_host, n_frames_host, tok_off_host, n_tok_host, tok_cls,
                                                nullptr, tok_min, gap_cls, n_clips, tok, workspace, workspace_bytes, logz, tok_post,
                                                start_mean, start_sd, status, stream);
}

}  // extern "C"
