// detect_common.h -- what detect.hip (one image per call) and detect_batch.hip (N images per call) share: the
// candidate decode, the rank sort and stages 3-5 of detect.hip's pipeline.  Every kernel below takes its image from
// the grid (the dimension named at the kernel) and addresses per-image arrays of n = levels * topn slots; the
// single-image launches leave that dimension at 1.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssad_kernels.h"

namespace {

constexpr int kT = 256;

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// what the post-processing options add behind the greedy path's workspace, per image of n slots: pick ranks,
// Soft-NMS's own workspace, the voted boxes
size_t post_bytes(size_t n) { return al(n * 4) + al(ssad_soft_nms_workspace_bytes((int)n)) + al(n * 16); }

bool post_is_plain(const ssad_detect_post* post) {
  return !post || (post->nms_method == SSAD_NMS_GREEDY && !post->vote);
}

int check_post(const ssad_detect_post* post) {
  if (!post) return 0;
  if (post->nms_method < SSAD_NMS_GREEDY || post->nms_method > SSAD_NMS_SOFT_GAUSSIAN) return SSAD_E_BADARG;
  if (post->nms_method != SSAD_NMS_GREEDY && !(post->sigma > 0.0f)) return SSAD_E_BADARG;
  if (post->vote) {
    const int m = post->scoring_method;
    if (m < SSAD_VOTE_ID || m > SSAD_VOTE_QUASI_SUM) return SSAD_E_BADARG;
    if ((m == SSAD_VOTE_TEMP_AVG || m == SSAD_VOTE_GENERALIZED_AVG || m == SSAD_VOTE_QUASI_SUM) &&
        !(post->beta > 0.0f))
      return SSAD_E_BADARG;
  }
  return 0;
}

// Rank sort of `segs` segments of seg_len keys each (blockIdx.y = segment): out[rank] = key, rank = the number of keys
// that precede it (descending: larger first; ascending: smaller first; equal keys in index order -- stable).  vals
// (may be null) travel with their keys.  O(seg_len^2) comparisons through LDS tiles.
__global__ __launch_bounds__(kT) void det_rank_sort_kernel(const unsigned long long* in, const int* vals_in, int seg_len,
                                                           int descending, unsigned long long* out, int* vals_out) {
  __shared__ unsigned long long tile[kT];
  const long long base = (long long)blockIdx.y * seg_len;
  const int i = blockIdx.x * kT + threadIdx.x;
  const unsigned long long mine = i < seg_len ? in[base + i] : 0;
  int rank = 0;
  for (int j0 = 0; j0 < seg_len; j0 += kT) {
    const int j = j0 + threadIdx.x;
    tile[threadIdx.x] = j < seg_len ? in[base + j] : 0;
    __syncthreads();
    const int m = seg_len - j0 < kT ? seg_len - j0 : kT;
    for (int u = 0; u < m; ++u) {
      const unsigned long long o = tile[u];
      const bool before = descending ? (o > mine) : (o < mine);
      rank += (before || (o == mine && j0 + u < i)) ? 1 : 0;
    }
    __syncthreads();
  }
  if (i < seg_len) {
    out[base + rank] = mine;
    if (vals_in) vals_out[base + rank] = vals_in[base + i];
  }
}

// One candidate slot of an image: `key` is its level's r-th largest key (0 past the level's last candidate), delta
// the image's box deltas of level l.  Writes the box (4 floats), the score and the class-order key of the slot.
__device__ __forceinline__ void det_decode_candidate(unsigned long long key, int slot, int l, int H, int W, int A, int C,
                                                     int k_min, const double* cells, const float* delta,
                                                     int class_specific, float xform_clip, float scale, int im_h,
                                                     int im_w, float* bo, float* score, unsigned long long* ckey) {
  const unsigned sb = (unsigned)((key >> 29) & 0xffffffffull);
  if (sb == 0) {                                   // not a candidate
    *ckey = ~0ull;                                 // sorts last
    *score = 0.0f;
    return;
  }
  const int idx = (int)((~(unsigned)key) & 0x1fffffffu);
  const int HW = H * W;
  const int x = idx % W, y = (idx / W) % H;
  const int ac = idx / HW;                         // a * C + cls
  const int a = ac / C, cls = ac - a * C;
  const float stride = (float)(1 << (k_min + l));
  const double* c = cells + ((long long)l * A + a) * 4;
  // boxes = float32([x, y, x, y]) * stride; boxes += cell_anchor (float64 add, float32 store)
  const float bx = __fmul_rn((float)x, stride), by = __fmul_rn((float)y, stride);
  const float b0 = (float)((double)bx + c[0]), b1 = (float)((double)by + c[1]);
  const float b2 = (float)((double)bx + c[2]), b3 = (float)((double)by + c[3]);
  // class-agnostic: channels 4a .. 4a+3; class-specific: the box of (anchor, class), the layout the training loss
  // addresses (retinanet.py:140-151)
  const long long ch = class_specific ? (long long)a * 4 * C + 4 * cls : (long long)a * 4;
  const float* d = delta + ch * HW + (long long)y * W + x;
  const float dx = d[0], dy = d[HW], dw = fminf(d[2 * HW], xform_clip),
              dh = fminf(d[3 * HW], xform_clip);
  const float w = __fadd_rn(__fsub_rn(b2, b0), 1.0f), h = __fadd_rn(__fsub_rn(b3, b1), 1.0f);
  const float cx = __fadd_rn(b0, __fmul_rn(0.5f, w)), cy = __fadd_rn(b1, __fmul_rn(0.5f, h));
  const float pcx = __fadd_rn(__fmul_rn(dx, w), cx), pcy = __fadd_rn(__fmul_rn(dy, h), cy);
  const float pw = __fmul_rn(expf(dw), w), ph = __fmul_rn(expf(dh), h);
  float o0 = __fsub_rn(pcx, __fmul_rn(0.5f, pw));
  float o1 = __fsub_rn(pcy, __fmul_rn(0.5f, ph));
  float o2 = __fsub_rn(__fadd_rn(pcx, __fmul_rn(0.5f, pw)), 1.0f);
  float o3 = __fsub_rn(__fadd_rn(pcy, __fmul_rn(0.5f, ph)), 1.0f);
  o0 = __fdiv_rn(o0, scale); o1 = __fdiv_rn(o1, scale);
  o2 = __fdiv_rn(o2, scale); o3 = __fdiv_rn(o3, scale);
  const float xm = (float)(im_w - 1), ym = (float)(im_h - 1);
  o0 = fmaxf(fminf(o0, xm), 0.0f); o1 = fmaxf(fminf(o1, ym), 0.0f);
  o2 = fmaxf(fminf(o2, xm), 0.0f); o3 = fmaxf(fminf(o3, ym), 0.0f);
  bo[0] = o0; bo[1] = o1; bo[2] = o2; bo[3] = o3;
  *score = __uint_as_float(sb);
  // ascending sort: class, then score descending, then slot
  *ckey = ((unsigned long long)cls << 48) | ((unsigned long long)(~sb) << 16) |
          (unsigned long long)(slot & 0xffff);
}

// gather boxes / scores / classes into class-sorted order (blockIdx.y = image)
__global__ __launch_bounds__(kT) void det_gather_kernel(int n, const unsigned long long* skeys,
                                                        const int* svals, const float* boxes,
                                                        const float* scores, float* sboxes,
                                                        float* sscores, int* scls) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const long long im = (long long)blockIdx.y * n;
  const unsigned long long k = skeys[im + i];
  const int slot = svals[im + i];
  scls[im + i] = k == ~0ull ? -1 : (int)(k >> 48);
  sscores[im + i] = scores[im + slot];
#pragma unroll
  for (int j = 0; j < 4; ++j) sboxes[(im + i) * 4 + j] = boxes[(im + slot) * 4 + j];
}

// cython_nms.pyx:72-79, float32
__device__ __forceinline__ bool suppresses(const float* a, float aarea, const float* b, float barea,
                                           float thresh) {
  const float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]);
  const float xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
  const float w = fmaxf(0.0f, __fadd_rn(__fsub_rn(xx2, xx1), 1.0f));
  const float h = fmaxf(0.0f, __fadd_rn(__fsub_rn(yy2, yy1), 1.0f));
  const float inter = __fmul_rn(w, h);
  const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(aarea, barea), inter));
  return ovr >= thresh;
}

__device__ __forceinline__ float box_area(const float* b) {
  return __fmul_rn(__fadd_rn(__fsub_rn(b[2], b[0]), 1.0f), __fadd_rn(__fsub_rn(b[3], b[1]), 1.0f));
}

// mask[i][bj] bit t: box i suppresses box bj*64+t (same class, later in score order); blockIdx.z = image
__global__ __launch_bounds__(64) void det_nms_mask_kernel(int n, int words, const float* sboxes,
                                                          const int* scls, float thresh,
                                                          unsigned long long* mask) {
  __shared__ float jb[64][4];
  __shared__ int jc[64];
  const long long im = (long long)blockIdx.z * n;
  sboxes += im * 4; scls += im; mask += im * words;
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int t = threadIdx.x;
  const int j = bj * 64 + t;
  if (j < n) {
#pragma unroll
    for (int q = 0; q < 4; ++q) jb[t][q] = sboxes[(long long)j * 4 + q];
    jc[t] = scls[j];
  } else {
    jc[t] = -2;
  }
  __syncthreads();
  const int i = bi * 64 + t;
  if (i >= n) return;
  const int ci = scls[i];
  unsigned long long bits = 0;
  if (ci >= 0) {
    float ib[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ib[q] = sboxes[(long long)i * 4 + q];
    const float ia = box_area(ib);
    for (int u = 0; u < 64; ++u) {
      const int jj = bj * 64 + u;
      if (jj > i && jc[u] == ci && suppresses(ib, ia, jb[u], box_area(jb[u]), thresh))
        bits |= 1ull << u;
    }
  }
  mask[(long long)i * words + bj] = bits;
}

// one workgroup per (class, image = blockIdx.y): greedy walk of the class segment in score order
__global__ __launch_bounds__(kT) void det_nms_scan_kernel(int n, int words, int C, const int* scls,
                                                          const float* sscores,
                                                          const unsigned long long* mask,
                                                          unsigned long long* fkeys) {
  extern __shared__ unsigned long long remv[];
  __shared__ int seg[2];
  const long long im = (long long)blockIdx.y * n;
  scls += im; sscores += im; mask += im * words; fkeys += im;
  const int cls = blockIdx.x;
  for (int w = threadIdx.x; w < words; w += kT) remv[w] = 0;
  if (threadIdx.x == 0) {
    // segment of this class in the class-sorted arrays (binary searches)
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; const int c = scls[m]; if (c >= 0 && c < cls) lo = m + 1; else hi = m; }
    seg[0] = lo;
    hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; const int c = scls[m]; if (c >= 0 && c <= cls) lo = m + 1; else hi = m; }
    seg[1] = lo;
  }
  __syncthreads();
  const int s = seg[0], e = seg[1];
  for (int i = s; i < e; ++i) {
    const bool removed = (remv[i >> 6] >> (i & 63)) & 1ull;      // uniform read
    __syncthreads();
    if (!removed) {
      for (int w = threadIdx.x + (i >> 6); w < words; w += kT) remv[w] |= mask[(long long)i * words + w];
      if (threadIdx.x == 0)   // descending sort key: score, then earlier position first
        fkeys[i] = ((unsigned long long)__float_as_uint(sscores[i]) << 32) |
                   (unsigned long long)(~(unsigned)i);
    } else if (threadIdx.x == 0) {
      fkeys[i] = 0;
    }
    __syncthreads();
  }
  (void)C;
}

// blockIdx.y = image: out [images][dets_per_im][6], count [images]
__global__ __launch_bounds__(kT) void det_emit_kernel(int n, int dets_per_im,
                                                      const unsigned long long* fsorted,
                                                      const float* sboxes, const int* scls,
                                                      float* out, int* count) {
  const long long im = (long long)blockIdx.y * n;
  fsorted += im; sboxes += im * 4; scls += im;
  out += (long long)blockIdx.y * dets_per_im * 6; count += blockIdx.y;
  const int r = blockIdx.x * kT + threadIdx.x;
  if (r == 0) {
    int c = 0;
    while (c < dets_per_im && c < n && fsorted[c] != 0) ++c;
    *count = c;
  }
  if (r >= dets_per_im || r >= n) return;
  const unsigned long long k = fsorted[r];
  float* o = out + (long long)r * 6;
  if (k == 0) { for (int j = 0; j < 6; ++j) o[j] = 0.0f; return; }
  const int i = (int)(~(unsigned)k);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = sboxes[(long long)i * 4 + j];
  o[4] = __uint_as_float((unsigned)(k >> 32));
  o[5] = (float)(scls[i] + 1);                  // class ids are 1-based in the output
}

}  // namespace
