// detect.hip -- RetinaNet inference post-processing on the device (row f4, second
// half): what detectron/lib/core/test_retinanet.py:108-206 does in numpy for one
// image -- per level: scores above the threshold, the pre_nms_topn best, anchor
// decode (utils/boxes.py:150-190), rescale and clip (:132-147); then per-class
// greedy NMS (utils/cython_nms.pyx:37-92, suppression at IoU >= thresh, +1 box
// convention) and the dets_per_im best survivors, sorted by score.
//
// Pipeline (all on the caller's stream, no host round trip):
//   1. one 64-bit key per (level, anchor, class, y, x):
//        [63:61] level order | [60:29] score bits (0 when not a candidate) | [28:0] ~index
//      and, per level, the pre_nms_topn LARGEST keys: a radix select (eight 8-bit passes: histogram of the
//      digit among the keys that match the prefix found so far, then the digit in which the k-th largest
//      lies) gives the k-th largest key exactly (keys are unique), a compaction collects the keys >= it, a
//      rank sort orders those <= topn keys;
//   2. decode the <= levels * pre_nms_topn survivors to boxes;
//   3. order them by (class, score descending) -- rank sort;
//   4. 64 x 64 suppression bit-matrix for same-class pairs, then one workgroup per
//      class walks its segment in score order (the serial part of greedy NMS);
//   5. order the survivors by score (rank sort), emit the first dets_per_im.
// ssad_retinanet_detect_ex (core/test.py:779-797) may replace step 4 by Soft-NMS and add bounding-box voting before
// step 5: both are soft_nms.hip's and write the same survivor words.
// Score ties are broken by element index (the reference's argpartition / argsort
// leave them unspecified).  Every kernel is this file's: rounds 1-5 sorted with rocPRIM's radix sort through
// hipCUB (the whole 8.6 M-key array of an image for the top 1000 per level); the rank sort is O(n^2) comparisons
// on n = levels x topn <= 65 535 keys, exact and stable, a few microseconds at the reference's n = 5000.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssad_kernels.h"
#include "detect_common.h"     // the decode, the rank sort and stages 3-5, shared with detect_batch.hip

namespace {

struct DArgs {
  const float* prob[SSAD_MAX_LEVELS];     // [1][A*C][H][W]
  const float* delta[SSAD_MAX_LEVELS];    // [1][A*4][H][W]; class_specific: [1][A*4*C][H][W]
  const double* cells;                    // [levels][A][4]
  int H[SSAD_MAX_LEVELS], W[SSAD_MAX_LEVELS];
  long long estart[SSAD_MAX_LEVELS + 1];  // first element of each level in the key array
  int levels, A, C, k_min;
  float th, th_last, nms_thresh, scale, xform_clip;
  int topn, dets_per_im, im_h, im_w;
  int n;                                  // levels * topn candidate slots
  int class_specific;                     // RETINANET.CLASS_SPECIFIC_BBOX: channel a * 4 * C + 4 * cls + k
};

__device__ __forceinline__ int level_of(const DArgs& p, long long e) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < SSAD_MAX_LEVELS; ++i)
    if (i < p.levels && e >= p.estart[i]) l = i;
  return l;
}

__global__ __launch_bounds__(kT) void det_keys_kernel(const DArgs p, unsigned long long* keys) {
  const long long total = p.estart[p.levels];
  for (long long e = (long long)blockIdx.x * kT + threadIdx.x; e < total;
       e += (long long)gridDim.x * kT) {
    const int l = level_of(p, e);
    const long long idx = e - p.estart[l];
    const float s = p.prob[l][idx];
    const float th = l == p.levels - 1 ? p.th_last : p.th;
    const unsigned long long sb = s > th ? (unsigned long long)__float_as_uint(s) : 0ull;
    // descending sort: level 0 first, higher score first, lower index first
    keys[e] = ((unsigned long long)(7 - l) << 61) | (sb << 29) |
              (unsigned long long)((~(unsigned)idx) & 0x1fffffffu);
  }
}

// ---- top-k per level: radix select -------------------------------------------------------------------------------
struct SelState {
  unsigned long long prefix[SSAD_MAX_LEVELS];   // the bits of the k-th largest key found so far
  int want[SSAD_MAX_LEVELS];                    // its rank among the keys that match the prefix (1 = largest)
  int k[SSAD_MAX_LEVELS];                       // min(topn, elements of the level)
  int count[SSAD_MAX_LEVELS];                   // compaction cursor
};

__global__ void det_select_init_kernel(const DArgs p, SelState* st, unsigned* hist, unsigned long long* sel) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < SSAD_MAX_LEVELS) {
    const long long E = t < p.levels ? p.estart[t + 1] - p.estart[t] : 0;
    const int k = (int)(E < p.topn ? E : p.topn);
    st->prefix[t] = 0; st->want[t] = k; st->k[t] = k; st->count[t] = 0;
  }
  if (t < SSAD_MAX_LEVELS * 256) hist[t] = 0;
  for (int i = t; i < p.n; i += gridDim.x * blockDim.x) sel[i] = 0;   // slots past a level's k: key 0 = "not a candidate"
}

// histogram of digit (key >> shift) & 255 over the keys of level blockIdx.y whose bits above the digit equal the prefix
__global__ __launch_bounds__(kT) void det_select_hist_kernel(const DArgs p, const unsigned long long* keys,
                                                             const SelState* st, unsigned* hist, int shift) {
  __shared__ unsigned h[256];
  const int l = blockIdx.y;
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long prefix = st->prefix[l];
  const long long lo = p.estart[l], hi = p.estart[l + 1];
  for (long long e = lo + (long long)blockIdx.x * kT + threadIdx.x; e < hi; e += (long long)gridDim.x * kT) {
    const unsigned long long key = keys[e];
    const bool match = shift >= 56 || ((key ^ prefix) >> (shift + 8)) == 0;
    if (match) atomicAdd(&h[(unsigned)(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[l * 256 + threadIdx.x], h[threadIdx.x]);
}

// the digit in which the wanted key lies; one thread per level
__global__ void det_select_pick_kernel(int levels, SelState* st, unsigned* hist, int shift) {
  const int l = threadIdx.x;
  if (l >= levels) return;
  int want = st->want[l];
  if (st->k[l] > 0) {
    for (int d = 255; d >= 0; --d) {
      const int c = (int)hist[l * 256 + d];
      if (want <= c) { st->prefix[l] |= (unsigned long long)d << shift; break; }
      want -= c;
    }
    st->want[l] = want;
  }
  for (int d = 0; d < 256; ++d) hist[l * 256 + d] = 0;
}

// the keys >= the k-th largest, in arrival order (exactly k of them: keys are unique)
__global__ __launch_bounds__(kT) void det_select_compact_kernel(const DArgs p, const unsigned long long* keys,
                                                                SelState* st, unsigned long long* sel) {
  const int l = blockIdx.y;
  if (st->k[l] == 0) return;
  const unsigned long long kth = st->prefix[l];
  const long long lo = p.estart[l], hi = p.estart[l + 1];
  for (long long e = lo + (long long)blockIdx.x * kT + threadIdx.x; e < hi; e += (long long)gridDim.x * kT) {
    const unsigned long long key = keys[e];
    if (key >= kth) {
      const int slot = atomicAdd(&st->count[l], 1);
      if (slot < p.topn) sel[(long long)l * p.topn + slot] = key;
    }
  }
}

// slot = l * topn + r: the r-th best element of level l
__global__ __launch_bounds__(kT) void det_decode_kernel(const DArgs p,
                                                        const unsigned long long* keys,
                                                        float* boxes, float* scores,
                                                        unsigned long long* ckeys, int* cvals) {
  const int slot = blockIdx.x * kT + threadIdx.x;
  if (slot >= p.n) return;
  const int l = slot / p.topn;
  cvals[slot] = slot;
  // keys[slot]: the level's r-th largest key (0 past its last element)
  det_decode_candidate(keys[slot], slot, l, p.H[l], p.W[l], p.A, p.C, p.k_min, p.cells, p.delta[l], p.class_specific,
                       p.xform_clip, p.scale, p.im_h, p.im_w, boxes + (long long)slot * 4, scores + slot, ckeys + slot);
}

struct Plan {
  long long total;
  int n, words;
  size_t sort1, sort2, sort3;
};

int make_plan(int levels, int A, int C, const int* H, const int* W, int topn, Plan* p,
              long long* estart) {
  if (levels < 1 || levels > SSAD_MAX_LEVELS || A < 1 || C < 1 || C > 0x7fff || topn < 1)
    return SSAD_E_BADARG;
  long long t = 0;
  for (int l = 0; l < levels; ++l) {
    if (H[l] < 0 || W[l] < 0) return SSAD_E_BADARG;
    const long long e = (long long)A * C * H[l] * W[l];
    if (e >= (1LL << 29)) return SSAD_E_BADARG;      // 29 index bits in the key
    estart[l] = t;
    t += e;
  }
  for (int l = levels; l <= SSAD_MAX_LEVELS; ++l) estart[l] = t;
  if ((long long)levels * topn > 0xffff) return SSAD_E_BADARG;   // 16 slot bits in the class key
  p->total = t;
  p->n = levels * topn;
  p->words = (p->n + 63) / 64;
  // (sort1: the selection's state + histograms; the former radix-sort scratch sizes stay in the plan as zero)
  p->sort1 = al(sizeof(SelState)) + al(SSAD_MAX_LEVELS * 256 * sizeof(unsigned));
  p->sort2 = p->sort3 = 0;
  return 0;
}

}  // namespace

extern "C" {

size_t ssad_retinanet_detect_workspace_bytes(int levels, int A, int C, const int* H_host,
                                             const int* W_host, int pre_nms_topn) {
  Plan p;
  long long es[SSAD_MAX_LEVELS + 1];
  if (make_plan(levels, A, C, H_host, W_host, pre_nms_topn, &p, es)) return 0;
  size_t tmp = p.sort1 > p.sort2 ? p.sort1 : p.sort2;
  if (p.sort3 > tmp) tmp = p.sort3;
  const size_t n = (size_t)p.n;
  const size_t ks = (size_t)p.total > n ? (size_t)p.total : n;       // keys_s holds the levels' top-k (n slots) too
  return al((size_t)p.total * 8) + al(ks * 8) + al(tmp) + al(n * 16) + al(n * 4) + 2 * al(n * 8) +
         2 * al(n * 4) + al(n * 16) + al(n * 4) + al(n * 4) + al(n * (size_t)p.words * 8) +
         2 * al(n * 8);
}

}  // extern "C"

namespace {

// the body of ssad_retinanet_detect and ssad_retinanet_detect_ex; post == nullptr (or greedy without voting) makes
// the launches ssad_retinanet_detect has always made
int detect_body(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, float nms_thresh, int dets_per_im,
    float im_scale, int im_height, int im_width, float bbox_xform_clip, float* dets_out,
    int* count_out, void* workspace, size_t workspace_bytes, ssad_stream_t stream,
    const ssad_detect_post* post, int class_specific) {
  Plan pl;
  DArgs a;
  const int rc = make_plan(levels, A, C, H_host, W_host, pre_nms_topn, &pl, a.estart);
  if (rc) return rc;
  if (!cls_prob_host || !box_pred_host || !cell_anchors || !dets_out || !count_out ||
      dets_per_im < 1 || dets_per_im > pl.n || !(im_scale > 0.0f) || check_post(post) ||
      (class_specific != 0 && class_specific != 1))
    return SSAD_E_BADARG;
  if (post_is_plain(post)) post = nullptr;
  const size_t need = ssad_retinanet_detect_ex_workspace_bytes(levels, A, C, H_host, W_host,
                                                               pre_nms_topn, post);
  if (!workspace || workspace_bytes < need) return SSAD_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < SSAD_MAX_LEVELS; ++l) {
    a.prob[l] = l < levels ? cls_prob_host[l] : nullptr;
    a.delta[l] = l < levels ? box_pred_host[l] : nullptr;
    a.H[l] = l < levels ? H_host[l] : 0;
    a.W[l] = l < levels ? W_host[l] : 0;
  }
  a.cells = cell_anchors;
  a.levels = levels; a.A = A; a.C = C; a.k_min = k_min;
  a.th = inference_th; a.th_last = 0.0f;        // test_retinanet.py:136: level k_max uses 0.0
  a.nms_thresh = nms_thresh; a.scale = im_scale; a.xform_clip = bbox_xform_clip;
  a.topn = pre_nms_topn; a.dets_per_im = dets_per_im; a.im_h = im_height; a.im_w = im_width;
  a.n = pl.n;
  a.class_specific = class_specific;
  const size_t n = (size_t)pl.n;
  char* w = (char*)workspace;
  auto take = [&](size_t b) { char* r = w; w += al(b); return r; };
  unsigned long long* keys = (unsigned long long*)take((size_t)pl.total * 8);
  unsigned long long* keys_s = (unsigned long long*)take(((size_t)pl.total > n ? (size_t)pl.total : n) * 8);
  size_t tmp_bytes = pl.sort1 > pl.sort2 ? pl.sort1 : pl.sort2;
  if (pl.sort3 > tmp_bytes) tmp_bytes = pl.sort3;
  void* tmp = take(tmp_bytes);
  float* boxes = (float*)take(n * 16);
  float* scores = (float*)take(n * 4);
  unsigned long long* ckeys = (unsigned long long*)take(n * 8);
  unsigned long long* ckeys_s = (unsigned long long*)take(n * 8);
  int* cvals = (int*)take(n * 4);
  int* cvals_s = (int*)take(n * 4);
  float* sboxes = (float*)take(n * 16);
  float* sscores = (float*)take(n * 4);
  int* scls = (int*)take(n * 4);
  unsigned long long* mask = (unsigned long long*)take(n * (size_t)pl.words * 8);
  unsigned long long* fkeys = (unsigned long long*)take(n * 8);
  unsigned long long* fkeys_s = (unsigned long long*)take(n * 8);
  int* pick_rank = nullptr;
  void* soft_ws = nullptr;
  float* voted = nullptr;
  if (post) {
    pick_rank = (int*)take(n * 4);
    soft_ws = take(ssad_soft_nms_workspace_bytes(pl.n));
    voted = (float*)take(n * 16);
  }

  if (pl.total > 0) {
    long long blocks = (pl.total + kT - 1) / kT;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(det_keys_kernel, dim3((unsigned)blocks), dim3(kT), 0, s, a, keys);
  }
  // top-k per level: keys_s[l * topn + r] = the level's r-th largest key
  {
    SelState* st = (SelState*)tmp;
    unsigned* hist = (unsigned*)((char*)tmp + al(sizeof(SelState)));
    unsigned long long* sel = fkeys;             // scratch until the NMS scan claims it (stream order)
    hipLaunchKernelGGL(det_select_init_kernel, dim3(8), dim3(kT), 0, s, a, st, hist, sel);
    if (pl.total > 0) {
      long long per = (pl.total / levels + kT - 1) / kT;
      if (per > 512) per = 512;
      if (per < 1) per = 1;
      for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(det_select_hist_kernel, dim3((unsigned)per, (unsigned)levels), dim3(kT), 0, s, a, keys, st, hist, shift);
        hipLaunchKernelGGL(det_select_pick_kernel, dim3(1), dim3(64), 0, s, levels, st, hist, shift);
      }
      hipLaunchKernelGGL(det_select_compact_kernel, dim3((unsigned)per, (unsigned)levels), dim3(kT), 0, s, a, keys, st, sel);
    }
    hipLaunchKernelGGL(det_rank_sort_kernel, dim3((unsigned)((pre_nms_topn + kT - 1) / kT), (unsigned)levels), dim3(kT), 0, s,
                       sel, (const int*)nullptr, pre_nms_topn, 1, keys_s, (int*)nullptr);
  }
  const int nb = (pl.n + kT - 1) / kT;
  hipLaunchKernelGGL(det_decode_kernel, dim3(nb), dim3(kT), 0, s, a, keys_s, boxes, scores, ckeys,
                     cvals);
  hipLaunchKernelGGL(det_rank_sort_kernel, dim3((unsigned)nb, 1), dim3(kT), 0, s, ckeys, cvals, pl.n, 0, ckeys_s, cvals_s);
  hipLaunchKernelGGL(det_gather_kernel, dim3(nb), dim3(kT), 0, s, pl.n, ckeys_s, cvals_s, boxes,
                     scores, sboxes, sscores, scls);
  if (!post || post->nms_method == SSAD_NMS_GREEDY) {
    // greedy: suppression at ovr >= nms_thresh, decided ahead in the bit-matrix
    hipLaunchKernelGGL(det_nms_mask_kernel, dim3(pl.words, pl.words), dim3(64), 0, s, pl.n, pl.words,
                       sboxes, scls, nms_thresh, mask);
    (void)hipMemsetAsync(fkeys, 0, n * 8, s);
    hipLaunchKernelGGL(det_nms_scan_kernel, dim3(C), dim3(kT), (size_t)pl.words * 8, s, pl.n, pl.words,
                       C, scls, sscores, mask, fkeys);
  } else {
    // Soft-NMS (its "hard" decays to 0 at ov > nms_thresh and retires below score_thresh): the same fkeys words
    const int rs = ssad_soft_nms(sboxes, sscores, scls, pl.n, C, post->nms_method, post->sigma, nms_thresh,
                                 post->score_thresh, fkeys, pick_rank, soft_ws,
                                 ssad_soft_nms_workspace_bytes(pl.n), stream);
    if (rs) return rs;
  }
  const float* out_boxes = sboxes;
  if (post && post->vote) {
    // every survivor votes before the final sort: a scoring method may change the order and the cut
    const int rv = ssad_box_voting(sboxes, scls, pl.n, sboxes, sscores, scls, pl.n, C, post->vote_thresh,
                                   post->scoring_method, post->beta, fkeys, voted, stream);
    if (rv) return rv;
    out_boxes = voted;
  }
  hipLaunchKernelGGL(det_rank_sort_kernel, dim3((unsigned)nb, 1), dim3(kT), 0, s, fkeys, (const int*)nullptr, pl.n, 1, fkeys_s,
                     (int*)nullptr);
  hipLaunchKernelGGL(det_emit_kernel, dim3((dets_per_im + kT - 1) / kT), dim3(kT), 0, s, pl.n,
                     dets_per_im, fkeys_s, out_boxes, scls, dets_out, count_out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t ssad_retinanet_detect_ex_workspace_bytes(int levels, int A, int C, const int* H_host, const int* W_host,
                                                int pre_nms_topn, const ssad_detect_post* post) {
  const size_t base = ssad_retinanet_detect_workspace_bytes(levels, A, C, H_host, W_host, pre_nms_topn);
  if (base == 0 || check_post(post)) return 0;
  return post_is_plain(post) ? base : base + post_bytes((size_t)levels * pre_nms_topn);
}

int ssad_retinanet_detect(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, float nms_thresh, int dets_per_im,
    float im_scale, int im_height, int im_width, float bbox_xform_clip, float* dets_out,
    int* count_out, void* workspace, size_t workspace_bytes, ssad_stream_t stream) {
  return detect_body(cls_prob_host, box_pred_host, cell_anchors, levels, A, C, k_min, H_host, W_host, inference_th,
                     pre_nms_topn, nms_thresh, dets_per_im, im_scale, im_height, im_width, bbox_xform_clip, dets_out,
                     count_out, workspace, workspace_bytes, stream, nullptr, 0);
}

int ssad_retinanet_detect_ex(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, float nms_thresh, int dets_per_im,
    float im_scale, int im_height, int im_width, float bbox_xform_clip, float* dets_out,
    int* count_out, void* workspace, size_t workspace_bytes, ssad_stream_t stream,
    const ssad_detect_post* post) {
  return detect_body(cls_prob_host, box_pred_host, cell_anchors, levels, A, C, k_min, H_host, W_host, inference_th,
                     pre_nms_topn, nms_thresh, dets_per_im, im_scale, im_height, im_width, bbox_xform_clip, dets_out,
                     count_out, workspace, workspace_bytes, stream, post, 0);
}

int ssad_retinanet_detect_class_specific(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, float nms_thresh, int dets_per_im,
    float im_scale, int im_height, int im_width, float bbox_xform_clip, float* dets_out,
    int* count_out, void* workspace, size_t workspace_bytes, ssad_stream_t stream,
    const ssad_detect_post* post, int class_specific_bbox) {
  return detect_body(cls_prob_host, box_pred_host, cell_anchors, levels, A, C, k_min, H_host, W_host, inference_th,
                     pre_nms_topn, nms_thresh, dets_per_im, im_scale, im_height, im_width, bbox_xform_clip, dets_out,
                     count_out, workspace, workspace_bytes, stream, post, class_specific_bbox);
}

}  // extern "C"
