// detect_batch.hip -- detect.hip's post-processing for N images in one call (ssad_retinanet_detect_batch), and the
// detections-to-ground-truth step behind it (ssad_detections_to_gt: the teacher's pseudo-labels for the labeller).
//
// detect.hip writes one 64-bit key per score and selects each level's pre_nms_topn largest from the whole key array.
// Here the scores are read once and only the candidates (score > threshold) become keys:
//   1. candidate pass, one launch over all (image, level) segments: 16-byte loads, the threshold test, and the
//      survivors appended to the segment's list of `cap` keys through one counter per segment (wave ballot, one
//      atomic per wave).  A slot at or beyond cap is not written; the counter still counts it;
//   2. one workgroup per list: the min(count, cap) keys' topn largest (radix select in LDS histograms when the list
//      is longer than topn, as detect.hip's, then a rank sort in LDS), key 0 in the slots behind them; the image's
//      overflow word is set when count > cap;
//   3. detect.hip's stages 2-5 (detect_common.h) with the image on the grid, the decode with per-image scale / size.
// The keys are detect.hip's ([63:61] level order | [60:29] score bits | [28:0] ~index within the image's level), they
// are unique, and every later stage orders them itself: the arrival order in a list does not reach the result.
//
// ssad_retinanet_detect_batch_ex adds the per-image entries' remaining options:
//   - cls_is_logits: step 1 reads the softmax head's logits [N][A*(C+1)][H][W] instead (detb_candidates_logits_kernel):
//     a lane holds one cell's C+1 logits in registers, softmax_cell.h's arithmetic -- group_softmax_kernel's, so the
//     same bits -- makes its probabilities, and the foreground classes above the threshold are appended under the
//     index they would have in the background-dropped [A*C][H][W] tensor.  The probabilities are never written;
//   - Soft-NMS in place of the bit-matrix and the scan, and box voting before the final sort: soft_nms.hip's two
//     kernels with the image on their grid (soft_nms_images.h), one launch each for the whole batch.

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "ssad_kernels.h"
#include "detect_common.h"
#include "softmax_cell.h"
#include "soft_nms_images.h"

namespace {

constexpr int kTopT = 1024;      // threads of a top-k workgroup
constexpr int kCandIters = 8;    // 16-byte loads per lane the candidate pass aims at (sizes its grid)
constexpr int kCandMaxBlocks = 2048;   // per (image, level)

struct BGeom {
  const float* prob[SSAD_MAX_LEVELS];     // [N][A*C][H][W]; from logits: [N][A*(C+1)][H][W]
  const float* delta[SSAD_MAX_LEVELS];    // [N][A*4][H][W]; class_specific: [N][A*4*C][H][W]
  const double* cells;                    // [levels][A][4]
  int H[SSAD_MAX_LEVELS], W[SSAD_MAX_LEVELS];
  int E[SSAD_MAX_LEVELS];                 // A*C*H*W: the scores of one image on the level (< 2^29)
  int bstart[SSAD_MAX_LEVELS + 1];        // candidate pass: the level's first workgroup along grid x
  int levels, A, C, k_min;
  float th, th_last, xform_clip;
  int topn, cap, n, class_specific;       // n = levels * topn candidate slots per image
};

struct BImages {
  float scale[SSAD_DETECT_BATCH_MAX_IMAGES];
  int im_h[SSAD_DETECT_BATCH_MAX_IMAGES], im_w[SSAD_DETECT_BATCH_MAX_IMAGES];
};

// The whole wave calls this; the lanes with c append their key to the list.  True (for the whole wave) when the list
// was full before this call: the counter is then above cap, the image's rows are the caller's to redo, and the wave
// may leave the rest of its share unread -- on dense maps that spares most of the atomics on one counter.
__device__ __forceinline__ bool push_candidates(bool c, float score, int idx, unsigned long long level_bits,
                                                int* counter, unsigned long long* list, int cap) {
  const unsigned long long m = __ballot(c);
  if (m == 0) return false;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, leader);
  if (c) {
    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
    if (slot >= 0 && slot < cap)
      list[slot] = level_bits | ((unsigned long long)__float_as_uint(score) << 29) |
                   (unsigned long long)((~(unsigned)idx) & 0x1fffffffu);
  }
  return base >= cap;
}

// grid (sum of the levels' workgroups, N): a workgroup belongs to one (image, level)
__global__ __launch_bounds__(kT) void detb_candidates_kernel(const BGeom g, int* counts, unsigned long long* cand) {
  const int img = blockIdx.y;
  int l = 0;
#pragma unroll
  for (int i = 1; i < SSAD_MAX_LEVELS; ++i)
    if (i < g.levels && (int)blockIdx.x >= g.bstart[i]) l = i;
  const int blk = blockIdx.x - g.bstart[l], nblk = g.bstart[l + 1] - g.bstart[l];
  const int E = g.E[l];
  const float* s = g.prob[l] + (long long)img * E;
  const float th = l == g.levels - 1 ? g.th_last : g.th;
  const int seg = img * g.levels + l;
  int* counter = counts + seg;
  unsigned long long* list = cand + (long long)seg * g.cap;
  const unsigned long long lb = (unsigned long long)(7 - l) << 61;
  // [0, head) scalars up to the first 16-byte boundary, nvec float4, then the scalar tail
  int head = (int)(((16u - (unsigned)((uintptr_t)s & 15u)) & 15u) >> 2);
  if (head > E) head = E;
  const int nvec = (E - head) >> 2;
  const float4* v = (const float4*)(s + head);
  for (int v0 = blk * kT; v0 < nvec; v0 += nblk * kT) {          // uniform trip count: every wave votes as a whole
    const int i = v0 + threadIdx.x;
    const bool in = i < nvec;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in) q = v[i];
    const bool c0 = in && q.x > th, c1 = in && q.y > th, c2 = in && q.z > th, c3 = in && q.w > th;   // NaN: false
    if (__ballot(c0 || c1 || c2 || c3) == 0) continue;
    const int e = head + 4 * i;
    if (push_candidates(c0, q.x, e, lb, counter, list, g.cap) || push_candidates(c1, q.y, e + 1, lb, counter, list, g.cap) ||
        push_candidates(c2, q.z, e + 2, lb, counter, list, g.cap) || push_candidates(c3, q.w, e + 3, lb, counter, list, g.cap))
      break;
  }
  if (blk == 0 && threadIdx.x < 64) {                             // at most 3 + 3 scalars, the first wave
    const int t = threadIdx.x, tail0 = head + 4 * nvec;
    int e = -1;
    if (t < 3) { if (t < head) e = t; }
    else if (t < 6) { if (tail0 + (t - 3) < E) e = tail0 + (t - 3); }
    const float x = e >= 0 ? s[e] : 0.0f;
    push_candidates(e >= 0 && x > th, x, e, lb, counter, list, g.cap);
  }
}

// The candidate pass on the softmax head's logits; same grid, a workgroup belongs to one (image, level).  Work item
// = the softmax kernels': (anchor of the image, chunk of kT positions), one lane = one cell, whose C + 1 logits come
// plane by plane at stride H*W (coalesced across the lanes, non-temporal: nobody reads them again).  bstart gives the
// level min(items, kCandMaxBlocks) workgroups.  The wave stays whole around every vote: a lane past the plane's end
// loads the plane's last cell and takes part with c = false.
template <bool FAST, int CMAX>
__global__ __launch_bounds__(kT) void detb_candidates_logits_kernel(const BGeom g, int* counts,
                                                                    unsigned long long* cand) {
  const int img = blockIdx.y;
  int l = 0;
#pragma unroll
  for (int i = 1; i < SSAD_MAX_LEVELS; ++i)
    if (i < g.levels && (int)blockIdx.x >= g.bstart[i]) l = i;
  const int blk = blockIdx.x - g.bstart[l], nblk = g.bstart[l + 1] - g.bstart[l];
  const int C = g.C, K = g.C + 1;                                 // foreground classes; logits of a cell
  const unsigned hw = (unsigned)(g.H[l] * g.W[l]);
  const int chunks = (int)((hw + kT - 1) / kT), items = g.A * chunks;
  const float* x = g.prob[l] + (size_t)img * g.A * K * hw;
  const float th = l == g.levels - 1 ? g.th_last : g.th;
  const int seg = img * g.levels + l;
  int* counter = counts + seg;
  unsigned long long* list = cand + (long long)seg * g.cap;
  const unsigned long long lb = (unsigned long long)(7 - l) << 61;
  for (int item = blk; item < items; item += nblk) {              // uniform in the workgroup
    const int a = item / chunks;
    const unsigned pos = (unsigned)(item - a * chunks) * kT + threadIdx.x;
    const bool in = pos < hw;
    float v[CMAX];
    load_cell<CMAX, true>(x + (size_t)a * K * hw, hw, in ? pos : hw - 1, K, -FLT_MAX, v);
    softmax_cell<FAST, CMAX>(v);
    // nearly every cell has no foreground class above the threshold: one vote for the cell-wave first
    bool any = false;
#pragma unroll
    for (int c = 1; c < CMAX; ++c) any = any || (c < K && v[c] > th);          // NaN: false
    if (__ballot(in && any) == 0) continue;
    const int e0 = a * C * (int)hw + (int)pos;                    // class 1's index in the [A*C][H][W] tensor
    bool full = false;
#pragma unroll
    for (int c = 1; c < CMAX; ++c) {
      if (c < K && !full)                                         // wave-uniform
        full = push_candidates(in && v[c] > th, v[c], e0 + (c - 1) * (int)hw, lb, counter, list, g.cap);
    }
    if (full) break;
  }
}

// grid (levels, N), kTopT threads, topn * 8 bytes of dynamic LDS: out[seg][0 .. topn) = the list's largest keys in
// descending order, 0 behind them
__global__ __launch_bounds__(kTopT) void detb_topk_kernel(const int* counts, const unsigned long long* cand, int cap,
                                                          int topn, unsigned long long* out, int* overflow) {
  extern __shared__ unsigned long long sel[];       // [topn]
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_want, s_cnt;
  const int seg = blockIdx.y * gridDim.x + blockIdx.x;
  const int counted = counts[seg];
  const int len = counted < cap ? counted : cap;    // bounded by what was counted, never beyond the list
  const unsigned long long* keys = cand + (long long)seg * cap;
  out += (long long)seg * topn;
  const int t = threadIdx.x;
  if (t == 0) {
    if (counted > cap) atomicOr(overflow + blockIdx.y, 1);
    s_prefix = 0; s_want = topn; s_cnt = 0;
  }
  const int k = len < topn ? len : topn;
  __syncthreads();
  if (len > topn) {
    // the topn-th largest key, digit by digit (keys are unique, so exactly topn keys are >= it)
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      for (int i = t; i < len; i += kTopT) {
        const unsigned long long key = keys[i];
        if (shift >= 56 || ((key ^ prefix) >> (shift + 8)) == 0) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (t == 0) {
        int want = s_want;
        for (int d = 255; d >= 0; --d) {
          const int c = (int)hist[d];
          if (want <= c) { s_prefix = prefix | ((unsigned long long)d << shift); break; }
          want -= c;
        }
        s_want = want;
      }
      __syncthreads();
    }
  }
  const unsigned long long kth = s_prefix;          // 0 when the whole list is taken
  for (int i = t; i < len; i += kTopT) {
    const unsigned long long key = keys[i];
    if (key >= kth) {
      const int slot = atomicAdd(&s_cnt, 1);
      if (slot < topn) sel[slot] = key;
    }
  }
  __syncthreads();
  for (int i = t; i < k; i += kTopT) {
    const unsigned long long mine = sel[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += sel[j] > mine ? 1 : 0;
    out[rank] = mine;
  }
  for (int r = k + t; r < topn; r += kTopT) out[r] = 0;       // "not a candidate"
}

// grid (slots / kT, N); slot = l * topn + r: the r-th best element of the image's level l
__global__ __launch_bounds__(kT) void detb_decode_kernel(const BGeom g, const BImages im, const unsigned long long* keys,
                                                         float* boxes, float* scores, unsigned long long* ckeys,
                                                         int* cvals) {
  const int slot = blockIdx.x * kT + threadIdx.x;
  if (slot >= g.n) return;
  const int img = blockIdx.y;
  const int l = slot / g.topn;
  const long long o = (long long)img * g.n + slot;
  const long long per_image = (long long)g.A * 4 * (g.class_specific ? g.C : 1) * g.H[l] * g.W[l];
  cvals[o] = slot;
  det_decode_candidate(keys[o], slot, l, g.H[l], g.W[l], g.A, g.C, g.k_min, g.cells, g.delta[l] + img * per_image,
                       g.class_specific, g.xform_clip, im.scale[img], im.im_h[img], im.im_w[img], boxes + o * 4,
                       scores + o, ckeys + o);
}

// one workgroup per image: the rows r < counts[img] with score >= thresh, in order, the first Gmax of them
__global__ __launch_bounds__(kT) void dets_to_gt_kernel(const float* dets, const int* counts, const float* im_scale,
                                                        int dets_per_im, float thresh, int Gmax, float* gt_boxes,
                                                        int* gt_classes, int* gt_counts) {
  __shared__ int wave_total[kT / 64];
  __shared__ int s_base;
  const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int c = counts[img];
  c = c < 0 ? 0 : (c > dets_per_im ? dets_per_im : c);
  const float* d = dets + (long long)img * dets_per_im * 6;
  float* gb = gt_boxes + (long long)img * Gmax * 4;
  int* gc = gt_classes + (long long)img * Gmax;
  const float scale = im_scale[img];
  if (t == 0) s_base = 0;
  __syncthreads();
  for (int r0 = 0; r0 < c; r0 += kT) {
    const int r = r0 + t;
    const bool keep = r < c && d[(long long)r * 6 + 4] >= thresh;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int pos = s_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wave_total[w];
    if (keep && pos < Gmax) {
#pragma unroll
      for (int j = 0; j < 4; ++j) gb[(long long)pos * 4 + j] = __fmul_rn(d[(long long)r * 6 + j], scale);
      gc[pos] = (int)d[(long long)r * 6 + 5];
    }
    __syncthreads();
    if (t == 0) {
      int sum = s_base;
      for (int w = 0; w < kT / 64; ++w) sum += wave_total[w];
      s_base = sum;
    }
    __syncthreads();
  }
  const int kept = s_base < Gmax ? s_base : Gmax;
  if (t == 0) gt_counts[img] = kept;
  for (int g = kept + t; g < Gmax; g += kT) {
#pragma unroll
    for (int j = 0; j < 4; ++j) gb[(long long)g * 4 + j] = 0.0f;
    gc[g] = 0;
  }
}

struct BPlan {
  int n, words;
  size_t counts, cand, slots;    // byte sizes (unaligned) of the counters, the lists, and one n-slot int32 array x N
};

// the geometry checks of detect.hip's make_plan and the batch's own; fills E (may be null)
int batch_plan(int N, int levels, int A, int C, const int* H, const int* W, int topn, int cap, BPlan* p, int* E) {
  if (N < 1 || N > SSAD_DETECT_BATCH_MAX_IMAGES || !H || !W) return SSAD_E_BADARG;
  if (levels < 1 || levels > SSAD_MAX_LEVELS || A < 1 || C < 1 || C > 0x7fff || topn < 1)
    return SSAD_E_BADARG;
  if (topn > SSAD_DETECT_BATCH_MAX_TOPN || cap < topn) return SSAD_E_BADARG;
  for (int l = 0; l < levels; ++l) {
    if (H[l] < 0 || W[l] < 0) return SSAD_E_BADARG;
    const long long e = (long long)A * C * H[l] * W[l];
    if (e >= (1LL << 29)) return SSAD_E_BADARG;      // 29 index bits in the key
    if (E) E[l] = (int)e;
  }
  if ((long long)levels * topn > 0xffff) return SSAD_E_BADARG;   // 16 slot bits in the class key
  p->n = levels * topn;
  p->words = (p->n + 63) / 64;
  // the int offsets of the kernels: lists (N * n * words stays below 2^31 for every N and topn admitted above)
  if ((long long)N * levels * cap >= (1LL << 31)) return SSAD_E_BADARG;
  p->counts = (size_t)N * levels * 4;
  p->cand = (size_t)N * levels * cap * 8;
  p->slots = (size_t)N * p->n * 4;
  return 0;
}

size_t batch_bytes(const BPlan& p) {
  // counters, lists, keys_s | boxes, scores, ckeys x 2, cvals x 2, sboxes, sscores, scls | mask | fkeys x 2
  return al(p.counts) + al(p.cand) + al(p.slots * 2) + al(p.slots * 4) + al(p.slots) + 2 * al(p.slots * 2) +
         2 * al(p.slots) + al(p.slots * 4) + 2 * al(p.slots) + al(p.slots * 2 * (size_t)p.words) + 2 * al(p.slots * 2);
}

// what the options add behind batch_bytes: pick ranks, the scores of long Soft-NMS segments and the voted boxes of
// all N images, carved below as three arrays of N * n slots (al(N * x) <= N * al(x))
size_t batch_post_bytes(int N, const BPlan& p) { return (size_t)N * post_bytes((size_t)p.n); }

bool logit_classes_ok(int C) { return C + 1 >= kMinClasses && C + 1 <= kMaxClasses; }

// the body of ssad_retinanet_detect_batch and ssad_retinanet_detect_batch_ex; post == nullptr (or greedy without
// voting) and cls_is_logits == 0 make the launches ssad_retinanet_detect_batch has always made
int detect_batch_body(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int N, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, int candidate_cap, float nms_thresh,
    int dets_per_im, const float* im_scale_host, const int* im_height_host, const int* im_width_host,
    float bbox_xform_clip, int class_specific, float* dets_out, int* counts_out, int* overflow_out,
    void* workspace, size_t workspace_bytes, ssad_stream_t stream, const ssad_detect_post* post, int cls_is_logits) {
  BPlan pl;
  BGeom g;
  const int rc = batch_plan(N, levels, A, C, H_host, W_host, pre_nms_topn, candidate_cap, &pl, g.E);
  if (rc) return rc;
  if (!cls_prob_host || !box_pred_host || !cell_anchors || !im_scale_host || !im_height_host || !im_width_host ||
      !dets_out || !counts_out || !overflow_out || dets_per_im < 1 || dets_per_im > pl.n ||
      (class_specific != 0 && class_specific != 1) || check_post(post) || (cls_is_logits != 0 && cls_is_logits != 1) ||
      (cls_is_logits && !logit_classes_ok(C)))
    return SSAD_E_BADARG;
  if (post_is_plain(post)) post = nullptr;
  BImages im;
  for (int i = 0; i < SSAD_DETECT_BATCH_MAX_IMAGES; ++i) {
    if (i < N && !(im_scale_host[i] > 0.0f)) return SSAD_E_BADARG;
    im.scale[i] = i < N ? im_scale_host[i] : 1.0f;
    im.im_h[i] = i < N ? im_height_host[i] : 0;
    im.im_w[i] = i < N ? im_width_host[i] : 0;
  }
  for (int l = 0; l < levels; ++l)
    if (!cls_prob_host[l] || !box_pred_host[l]) return SSAD_E_BADARG;
  if (!workspace || workspace_bytes < batch_bytes(pl) + (post ? batch_post_bytes(N, pl) : 0)) return SSAD_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int blocks = 0;
  for (int l = 0; l < SSAD_MAX_LEVELS; ++l) {
    g.prob[l] = l < levels ? cls_prob_host[l] : nullptr;
    g.delta[l] = l < levels ? box_pred_host[l] : nullptr;
    g.H[l] = l < levels ? H_host[l] : 0;
    g.W[l] = l < levels ? W_host[l] : 0;
    if (l >= levels) g.E[l] = 0;
    g.bstart[l] = blocks;
    long long b;
    if (cls_is_logits)     // one workgroup per (anchor, chunk of kT cells) item (an empty level gets none)
      b = (long long)A * (((long long)g.H[l] * g.W[l] + kT - 1) / kT);
    else                   // one workgroup per kT * kCandIters float4
      b = ((long long)g.E[l] + (long long)kT * 4 * kCandIters - 1) / ((long long)kT * 4 * kCandIters);
    if (b > kCandMaxBlocks) b = kCandMaxBlocks;
    blocks += (int)b;
  }
  g.bstart[SSAD_MAX_LEVELS] = blocks;
  g.cells = cell_anchors;
  g.levels = levels; g.A = A; g.C = C; g.k_min = k_min;
  g.th = inference_th; g.th_last = 0.0f;          // test_retinanet.py:136: level k_max uses 0.0
  g.xform_clip = bbox_xform_clip;
  g.topn = pre_nms_topn; g.cap = candidate_cap; g.n = pl.n; g.class_specific = class_specific;

  char* w = (char*)workspace;
  auto take = [&](size_t b) { char* r = w; w += al(b); return r; };
  int* counts = (int*)take(pl.counts);
  unsigned long long* cand = (unsigned long long*)take(pl.cand);
  unsigned long long* keys_s = (unsigned long long*)take(pl.slots * 2);
  float* boxes = (float*)take(pl.slots * 4);
  float* scores = (float*)take(pl.slots);
  unsigned long long* ckeys = (unsigned long long*)take(pl.slots * 2);
  unsigned long long* ckeys_s = (unsigned long long*)take(pl.slots * 2);
  int* cvals = (int*)take(pl.slots);
  int* cvals_s = (int*)take(pl.slots);
  float* sboxes = (float*)take(pl.slots * 4);
  float* sscores = (float*)take(pl.slots);
  int* scls = (int*)take(pl.slots);
  unsigned long long* mask = (unsigned long long*)take(pl.slots * 2 * (size_t)pl.words);
  unsigned long long* fkeys = (unsigned long long*)take(pl.slots * 2);
  unsigned long long* fkeys_s = (unsigned long long*)take(pl.slots * 2);
  int* pick_rank = nullptr;
  unsigned* live = nullptr;
  float* voted = nullptr;
  if (post) {
    pick_rank = (int*)take(pl.slots);
    live = (unsigned*)take(pl.slots);
    voted = (float*)take(pl.slots * 4);
  }

  (void)hipMemsetAsync(counts, 0, pl.counts, s);                 // the call zeroes its own counters
  (void)hipMemsetAsync(overflow_out, 0, (size_t)N * 4, s);
  if (blocks > 0) {
    if (cls_is_logits)
      LAUNCH_BY_CLASSES(detb_candidates_logits_kernel, C + 1, dim3((unsigned)blocks, (unsigned)N), dim3(kT), 0, s, g,
                        counts, cand);
    else
      hipLaunchKernelGGL(detb_candidates_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(kT), 0, s, g, counts, cand);
  }
  hipLaunchKernelGGL(detb_topk_kernel, dim3((unsigned)levels, (unsigned)N), dim3(kTopT), (size_t)pre_nms_topn * 8, s,
                     counts, cand, candidate_cap, pre_nms_topn, keys_s, overflow_out);
  const unsigned nb = (unsigned)((pl.n + kT - 1) / kT), un = (unsigned)N;
  hipLaunchKernelGGL(detb_decode_kernel, dim3(nb, un), dim3(kT), 0, s, g, im, keys_s, boxes, scores, ckeys, cvals);
  hipLaunchKernelGGL(det_rank_sort_kernel, dim3(nb, un), dim3(kT), 0, s, ckeys, cvals, pl.n, 0, ckeys_s, cvals_s);
  hipLaunchKernelGGL(det_gather_kernel, dim3(nb, un), dim3(kT), 0, s, pl.n, ckeys_s, cvals_s, boxes, scores, sboxes,
                     sscores, scls);
  if (!post || post->nms_method == SSAD_NMS_GREEDY) {
    hipLaunchKernelGGL(det_nms_mask_kernel, dim3(pl.words, pl.words, un), dim3(64), 0, s, pl.n, pl.words, sboxes, scls,
                       nms_thresh, mask);
    (void)hipMemsetAsync(fkeys, 0, pl.slots * 2, s);
    hipLaunchKernelGGL(det_nms_scan_kernel, dim3((unsigned)C, un), dim3(kT), (size_t)pl.words * 8, s, pl.n, pl.words, C,
                       scls, sscores, mask, fkeys);
  } else {
    // Soft-NMS, one workgroup per (class, image): the same fkeys words (detect.hip's detect_body)
    const int rs = ssad_soft_nms_images(sboxes, sscores, scls, pl.n, N, C, post->nms_method, post->sigma, nms_thresh,
                                        post->score_thresh, fkeys, pick_rank, live, s);
    if (rs) return rs;
  }
  const float* out_boxes = sboxes;
  if (post && post->vote) {
    // every survivor votes before the final sort; beta is 1 where it is no exponent, as ssad_box_voting passes it
    const int m = post->scoring_method;
    const bool exponent = m == SSAD_VOTE_TEMP_AVG || m == SSAD_VOTE_GENERALIZED_AVG || m == SSAD_VOTE_QUASI_SUM;
    const int rv = ssad_box_voting_images(sboxes, scls, pl.n, sboxes, sscores, scls, pl.n, N, post->vote_thresh, m,
                                          exponent ? post->beta : 1.0f, fkeys, voted, s);
    if (rv) return rv;
    out_boxes = voted;
  }
  hipLaunchKernelGGL(det_rank_sort_kernel, dim3(nb, un), dim3(kT), 0, s, fkeys, (const int*)nullptr, pl.n, 1, fkeys_s,
                     (int*)nullptr);
  hipLaunchKernelGGL(det_emit_kernel, dim3((unsigned)((dets_per_im + kT - 1) / kT), un), dim3(kT), 0, s, pl.n,
                     dets_per_im, fkeys_s, out_boxes, scls, dets_out, counts_out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t ssad_retinanet_detect_batch_workspace_bytes(int N, int levels, int A, int C, const int* H_host,
                                                   const int* W_host, int pre_nms_topn, int candidate_cap) {
  BPlan p;
  if (batch_plan(N, levels, A, C, H_host, W_host, pre_nms_topn, candidate_cap, &p, nullptr)) return 0;
  return batch_bytes(p);
}

int ssad_retinanet_detect_batch(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int N, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, int candidate_cap, float nms_thresh,
    int dets_per_im, const float* im_scale_host, const int* im_height_host, const int* im_width_host,
    float bbox_xform_clip, int class_specific, float* dets_out, int* counts_out, int* overflow_out,
    void* workspace, size_t workspace_bytes, ssad_stream_t stream) {
  return detect_batch_body(cls_prob_host, box_pred_host, cell_anchors, N, levels, A, C, k_min, H_host, W_host,
                           inference_th, pre_nms_topn, candidate_cap, nms_thresh, dets_per_im, im_scale_host,
                           im_height_host, im_width_host, bbox_xform_clip, class_specific, dets_out, counts_out,
                           overflow_out, workspace, workspace_bytes, stream, nullptr, 0);
}

size_t ssad_retinanet_detect_batch_ex_workspace_bytes(int N, int levels, int A, int C, const int* H_host,
                                                      const int* W_host, int pre_nms_topn, int candidate_cap,
                                                      const ssad_detect_post* post) {
  BPlan p;
  if (batch_plan(N, levels, A, C, H_host, W_host, pre_nms_topn, candidate_cap, &p, nullptr) || check_post(post))
    return 0;
  return batch_bytes(p) + (post_is_plain(post) ? 0 : batch_post_bytes(N, p));
}

int ssad_retinanet_detect_batch_ex(
    const float* const* cls_prob_host, const float* const* box_pred_host,
    const double* cell_anchors, int N, int levels, int A, int C, int k_min, const int* H_host,
    const int* W_host, float inference_th, int pre_nms_topn, int candidate_cap, float nms_thresh,
    int dets_per_im, const float* im_scale_host, const int* im_height_host, const int* im_width_host,
    float bbox_xform_clip, int class_specific, float* dets_out, int* counts_out, int* overflow_out,
    void* workspace, size_t workspace_bytes, ssad_stream_t stream, const ssad_detect_post* post, int cls_is_logits) {
  return detect_batch_body(cls_prob_host, box_pred_host, cell_anchors, N, levels, A, C, k_min, H_host, W_host,
                           inference_th, pre_nms_topn, candidate_cap, nms_thresh, dets_per_im, im_scale_host,
                           im_height_host, im_width_host, bbox_xform_clip, class_specific, dets_out, counts_out,
                           overflow_out, workspace, workspace_bytes, stream, post, cls_is_logits);
}

int ssad_detections_to_gt(const float* dets, const int* counts, const float* im_scale, int N, int dets_per_im,
                          float score_thresh, int Gmax, float* gt_boxes, int* gt_classes, int* gt_counts,
                          ssad_stream_t stream) {
  if (!dets || !counts || !im_scale || !gt_boxes || !gt_classes || !gt_counts || N < 1 || dets_per_im < 1 || Gmax < 1)
    return SSAD_E_BADARG;
  hipLaunchKernelGGL(dets_to_gt_kernel, dim3((unsigned)N), dim3(kT), 0, (hipStream_t)stream, dets, counts, im_scale,
                     dets_per_im, score_thresh, Gmax, gt_boxes, gt_classes, gt_counts);
  return (int)hipGetLastError();
}

}  // extern "C"
