// soft_nms_images.h -- soft_nms.hip's two launches with the image on the grid, for the library's own callers
// (ssad_soft_nms / ssad_box_voting pass images = 1, detect_batch.hip passes its N).  Every per-image array is
// addressed as base + image * n (the top_* arrays of the voting as base + image * m).  The arguments are the public
// entries' and were checked by the caller; `live` holds images * n words (the scores of segments longer than
// SSAD_SOFT_NMS_LDS_CAP).  Not exported.
#pragma once

#include <hip/hip_runtime.h>

int ssad_soft_nms_images(const float* boxes, const float* scores, const int* cls, int n, int images, int C, int method,
                         float sigma, float Nt, float score_thresh, unsigned long long* keys_out, int* pick_rank_out,
                         unsigned* live, hipStream_t stream);
int ssad_box_voting_images(const float* top_boxes, const int* top_cls, int m, const float* boxes, const float* scores,
                           const int* cls, int n, int images, float vote_thresh, int scoring_method, float beta,
                           unsigned long long* keys_inout, float* voted_boxes_out, hipStream_t stream);
