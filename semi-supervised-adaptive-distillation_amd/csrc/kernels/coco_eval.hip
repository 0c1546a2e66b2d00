// COCO box evaluation (detectron/lib/datasets/vid_eval.py: evaluateImg :236-318, accumulate :320-425) for gfx950.
// The contract of every entry point is in include/ssad_kernels.h.
//
// coco_match_kernel   one 64-lane workgroup per (image, category) cell.  The lanes first rank the cell's detections
//                     (score descending, equal scores in slot order) into LDS, then lane p = a * T + t walks them
//                     against the cell's ground truths on its own: 40 independent, serial greedy walks over shared
//                     boxes with the reference's defaults.  IoUs are recomputed in the walk (a few flops), the matched
//                     flags of a walk are one byte per ground truth in the workspace, so a cell may hold any number.
// coco_cells_kernel   per (category, area range): non-ignored ground truths over all images, and "any evaluated cell".
// coco_accumulate_kernel   per (category, maxDets entry) one workgroup, lane p one (area range, threshold): a forward
//                     pass for the tp / fp totals, then one backward pass that undoes the cumulative sums element by
//                     element while it carries the right-to-left maximum of the precision and hands it to every recall
//                     threshold whose searchsorted(rc, thr, 'left') position it is passing.  Nothing of length nd is
//                     stored.
//
// Every comparison that decides a match or a position is a float64 comparison of values the reference computes with
// one rounding per operation: no contraction into fused multiply-adds in this file.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssad_kernels.h"

namespace {

constexpr int kT = 64;

// score -> key with the order of the reference's argsort(-score): larger score = larger key, -0.0 == +0.0,
// and a total order whatever the bits (a NaN ranks last), so the ranks of a cell are always a permutation
__device__ inline unsigned long long score_key(double s) {
  if (s != s) return 0ull;
  const long long b = __double_as_longlong(s + 0.0);
  return b < 0 ? ~(unsigned long long)b : ((unsigned long long)b | 0x8000000000000000ull);
}

__device__ inline double box_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw,
                                 double gh, bool crowd) {
  const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (!(w > 0.0) || !(h > 0.0)) return 0.0;
  const double i = w * h;
  const double da = dw * dh;
  const double u = crowd ? da : da + gw * gh - i;
  return i / u;
}

__global__ __launch_bounds__(kT) void coco_add_kernel(const float* boxes, int box_stride, const float* scores,
                                                      int score_stride, const float* cls1, int cls_stride,
                                                      const int* cats, int n, int cap, int K, double* det_xywh,
                                                      double* det_score, int* det_cat, int* bad_count) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= cap) return;
  if (j >= n) {
    det_cat[j] = -1;
    return;
  }
  const float* b = boxes + (size_t)j * box_stride;
  const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  const float w = x2 - x1 + 1.0f, h = y2 - y1 + 1.0f;
  det_xywh[4 * j + 0] = (double)x1;
  det_xywh[4 * j + 1] = (double)y1;
  det_xywh[4 * j + 2] = (double)w;
  det_xywh[4 * j + 3] = (double)h;
  det_score[j] = (double)scores[(size_t)j * score_stride];
  int c = cats ? cats[j] : (int)cls1[(size_t)j * cls_stride] - 1;
  if (c < 0 || c >= K) {
    atomicAdd(bad_count, 1);
    c = -1;
  }
  det_cat[j] = c;
}

__global__ __launch_bounds__(kT) void coco_match_kernel(
    int K, int cap, const double* __restrict__ det_xywh, const double* __restrict__ det_score,
    const int* __restrict__ det_cat, const double* __restrict__ gt_xywh, const double* __restrict__ gt_area,
    const unsigned char* __restrict__ gt_crowd, const int* __restrict__ gt_cell_off,
    const double* __restrict__ iou_thrs, int T, const double* __restrict__ area_rng, int A, int max_det, int relax,
    int* __restrict__ det_rank, int* __restrict__ dt_match, unsigned char* __restrict__ dt_ignore,
    int* __restrict__ cell_npig, unsigned char* __restrict__ cell_eval, unsigned char* __restrict__ gtm) {
  __shared__ int s_idx[SSAD_COCO_EVAL_MAX_DETS];
  __shared__ int s_kept, s_all;
  const int tid = threadIdx.x;
  const int cell = blockIdx.x;
  const int img = cell / K, k = cell - img * K;
  const int g0 = gt_cell_off[cell], g1 = gt_cell_off[cell + 1];
  const size_t base = (size_t)img * cap;
  if (tid == 0) s_kept = s_all = 0;
  __syncthreads();
  for (int j = tid; j < cap; j += kT) {
    if (det_cat[base + j] != k) continue;
    const unsigned long long mine = score_key(det_score[base + j]);
    int r = 0;
    for (int i = 0; i < cap; ++i) {
      if (det_cat[base + i] != k) continue;
      const unsigned long long other = score_key(det_score[base + i]);
      r += (other > mine) || (other == mine && i < j);
    }
    atomicAdd(&s_all, 1);
    if (r < max_det) {
      s_idx[r] = j;
      det_rank[base + j] = r;
      atomicAdd(&s_kept, 1);
    }
  }
  __syncthreads();
  const int D = s_kept;
  if (tid == 0) cell_eval[cell] = (g1 > g0 || s_all > 0) ? 1 : 0;
  if (g1 == g0 && D == 0) {
    for (int a = tid; a < A; a += kT) cell_npig[(size_t)cell * A + a] = 0;
    return;
  }
  const int AT = A * T;
  for (int p = tid; p < AT; p += kT) {
    const int a = p / T, t = p - a * T;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = fmin(iou_thrs[t], 1 - 1e-10);
    int npig = 0;
    for (int g = g0; g < g1; ++g) {
      gtm[(size_t)g * AT + p] = 0;
      const double ga = gt_area[g];
      npig += !(gt_crowd[g] || ga < lo || ga > hi);
    }
    if (t == 0) cell_npig[(size_t)cell * A + a] = npig;
    for (int d = 0; d < D; ++d) {
      const int j = s_idx[d];
      const double* db = det_xywh + (base + j) * 4;
      const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
      double iou = thr;
      int m = -1;
      for (int pass = 0; pass < 2; ++pass) {
        // an ignored ground truth behind a regular match ends the walk (:284-285)
        if (pass == 1 && m >= 0) break;
        for (int g = g0; g < g1; ++g) {
          const bool crowd = gt_crowd[g] != 0;
          const double ga = gt_area[g];
          const int ign = (crowd || ga < lo || ga > hi) ? 1 : 0;
          if (ign != pass) continue;
          if (gtm[(size_t)g * AT + p] && !crowd) continue;
          const double* gb = gt_xywh + (size_t)g * 4;
          const double gx = gb[0], gy = gb[1], gw = gb[2], gh = gb[3];
          double tiou = iou;
          if (relax) tiou = fmin(iou, (1.0 * gw * gh) / ((gw + 10.0) * (gh + 10.0)));
          const double v = box_iou(dx, dy, dw, dh, gx, gy, gw, gh, crowd);
          if (v < tiou) continue;
          iou = v;
          m = g;
        }
      }
      const size_t o = (base + j) * AT + p;
      if (m >= 0) {
        const double ga = gt_area[m];
        dt_match[o] = m - g0 + 1;
        dt_ignore[o] = (gt_crowd[m] || ga < lo || ga > hi) ? 1 : 0;
        gtm[(size_t)m * AT + p] = 1;
      } else {
        const double da = dw * dh;
        dt_match[o] = 0;
        dt_ignore[o] = (da < lo || da > hi) ? 1 : 0;
      }
    }
  }
}

__global__ __launch_bounds__(kT) void coco_cells_kernel(int I, int K, int A, const int* __restrict__ cell_npig,
                                                        const unsigned char* __restrict__ cell_eval,
                                                        long long* __restrict__ cat_npig, int* __restrict__ cat_eval) {
  const int idx = blockIdx.x * kT + threadIdx.x;
  if (idx >= K * (A + 1)) return;
  const int k = idx / (A + 1), a = idx - k * (A + 1);
  if (a < A) {
    long long s = 0;
    for (int i = 0; i < I; ++i) s += cell_npig[((size_t)i * K + k) * A + a];
    cat_npig[k * A + a] = s;
  } else {
    int any = 0;
    for (int i = 0; i < I; ++i) any |= cell_eval[(size_t)i * K + k];
    cat_eval[k] = any;
  }
}

__global__ __launch_bounds__(kT) void coco_accumulate_kernel(
    int K, int A, int T, int M, int R, const int* __restrict__ max_dets, const long long* __restrict__ perm,
    const long long* __restrict__ seg, const double* __restrict__ det_score, const int* __restrict__ det_rank,
    const int* __restrict__ dt_match, const unsigned char* __restrict__ dt_ignore,
    const long long* __restrict__ cat_npig, const int* __restrict__ cat_eval, const double* __restrict__ rec_thrs,
    double* __restrict__ precision, double* __restrict__ scores, double* __restrict__ recall) {
  const int k = blockIdx.x, mi = blockIdx.y;
  const int md = max_dets[mi];
  const long long s0 = seg[k], s1 = seg[k + 1];
  const int AT = A * T;
  const double eps = 2.220446049250313e-16;   // np.spacing(1)
  for (int p = threadIdx.x; p < AT; p += kT) {
    const int a = p / T, t = p - a * T;
    // element (t, r, k, a, mi) of [T][R][K][A][M], r varying
    const size_t o0 = (((size_t)t * R * K + k) * A + a) * M + mi;
    const size_t ostep = (size_t)K * A * M;
    const size_t orec = (((size_t)t * K + k) * A + a) * M + mi;
    const long long npig = cat_npig[k * A + a];
    if (!cat_eval[k] || npig == 0) {
      for (int r = 0; r < R; ++r) precision[o0 + r * ostep] = scores[o0 + r * ostep] = -1.0;
      recall[orec] = -1.0;
      continue;
    }
    long long tp = 0, fp = 0, nd = 0;
    for (long long i = s0; i < s1; ++i) {
      const long long slot = perm[i];
      if ((unsigned)det_rank[slot] >= (unsigned)md) continue;   // cut or empty (-1) too
      const size_t o = (size_t)slot * AT + p;
      const bool mt = dt_match[o] != 0, ig = dt_ignore[o] != 0;
      tp += mt && !ig;
      fp += !mt && !ig;
      ++nd;
    }
    const double dn = (double)npig;
    const double rc_last = (double)tp / dn;
    recall[orec] = nd ? rc_last : 0.0;
    int r = R - 1;
    // thresholds above the last recall (all of them without detections): position past the end
    while (r >= 0 && (nd == 0 || !(rc_last >= rec_thrs[r]))) {
      precision[o0 + r * ostep] = 0.0;
      scores[o0 + r * ostep] = 0.0;
      --r;
    }
    double pm = -1.0;
    long long left = nd;
    for (long long i = s1 - 1; i >= s0 && r >= 0; --i) {
      const long long slot = perm[i];
      if ((unsigned)det_rank[slot] >= (unsigned)md) continue;   // cut or empty (-1) too
      const size_t o = (size_t)slot * AT + p;
      const bool mt = dt_match[o] != 0, ig = dt_ignore[o] != 0;
      const double pr = (double)tp / ((double)fp + (double)tp + eps);
      if (pr > pm) pm = pr;
      tp -= mt && !ig;
      fp -= !mt && !ig;
      --left;
      // every remaining threshold is <= this element's recall; it sits here if the recall before is below it
      const double rc_prev = (double)tp / dn;
      const double sc = det_score[slot];
      while (r >= 0 && (left == 0 || rec_thrs[r] > rc_prev)) {
        precision[o0 + r * ostep] = pm;
        scores[o0 + r * ostep] = sc;
        --r;
      }
    }
  }
}

inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int ssad_coco_eval_add(const float* boxes_xyxy, int box_stride, const float* scores, int score_stride,
                       const float* cls1_f32, int cls_stride, const int* cats_i32, int n, int cap, int K, int image,
                       double* det_xywh, double* det_score, int* det_cat, int* bad_count, ssad_stream_t stream) {
  if (n < 0 || cap <= 0 || n > cap || K <= 0 || image < 0 || !det_xywh || !det_score || !det_cat || !bad_count)
    return SSAD_E_BADARG;
  if (n > 0 && (!boxes_xyxy || !scores || (!cls1_f32 && !cats_i32) || box_stride < 4 || score_stride < 1 ||
                (!cats_i32 && cls_stride < 1)))
    return SSAD_E_BADARG;
  const size_t base = (size_t)image * cap;
  hipLaunchKernelGGL(coco_add_kernel, dim3((cap + kT - 1) / kT), dim3(kT), 0, (hipStream_t)stream, boxes_xyxy,
                     box_stride, scores, score_stride, cls1_f32, cls_stride, cats_i32, n, cap, K,
                     det_xywh + base * 4, det_score + base, det_cat + base, bad_count);
  return (int)hipGetLastError();
}

size_t ssad_coco_eval_match_workspace_bytes(long long G, int A, int T) {
  if (G < 0 || A <= 0 || T <= 0) return 0;
  return al((size_t)G * A * T + 1);
}

int ssad_coco_eval_match(int I, int K, int cap, const double* det_xywh, const double* det_score, const int* det_cat,
                         const double* gt_xywh, const double* gt_area, const unsigned char* gt_crowd,
                         const int* gt_cell_off, long long G, const double* iou_thrs, int T, const double* area_rng,
                         int A, int max_det, int small_box_relax, int* det_rank, int* dt_match,
                         unsigned char* dt_ignore, int* cell_npig, unsigned char* cell_eval, void* workspace,
                         size_t workspace_bytes, ssad_stream_t stream) {
  if (I <= 0 || K <= 0 || cap <= 0 || T <= 0 || A <= 0 || G < 0 || max_det <= 0 ||
      max_det > SSAD_COCO_EVAL_MAX_DETS || (long long)I * K >= (1ll << 31) - 1 || G >= (1ll << 31))
    return SSAD_E_BADARG;
  if (!det_xywh || !det_score || !det_cat || !gt_cell_off || !iou_thrs || !area_rng || !det_rank || !dt_match ||
      !dt_ignore || !cell_npig || !cell_eval || (G > 0 && (!gt_xywh || !gt_area || !gt_crowd)))
    return SSAD_E_BADARG;
  if (workspace_bytes < ssad_coco_eval_match_workspace_bytes(G, A, T) || !workspace) return SSAD_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(det_rank, 0xff, (size_t)I * cap * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(coco_match_kernel, dim3(I * K), dim3(kT), 0, s, K, cap, det_xywh, det_score, det_cat, gt_xywh,
                     gt_area, gt_crowd, gt_cell_off, iou_thrs, T, area_rng, A, max_det, small_box_relax, det_rank,
                     dt_match, dt_ignore, cell_npig, cell_eval, (unsigned char*)workspace);
  return (int)hipGetLastError();
}

size_t ssad_coco_eval_accumulate_workspace_bytes(int K, int A) {
  if (K <= 0 || A <= 0) return 0;
  return al((size_t)K * A * sizeof(long long)) + al((size_t)K * sizeof(int));
}

int ssad_coco_eval_accumulate(int I, int K, int cap, int A, int T, int M, int R, const int* max_dets,
                              const long long* perm, long long n_perm, const long long* seg, const double* det_score,
                              const int* det_rank, const int* dt_match, const unsigned char* dt_ignore,
                              const int* cell_npig, const unsigned char* cell_eval, const double* rec_thrs,
                              double* precision, double* scores, double* recall, void* workspace,
                              size_t workspace_bytes, ssad_stream_t stream) {
  if (I <= 0 || K <= 0 || cap <= 0 || A <= 0 || T <= 0 || M <= 0 || M > 65535 || R <= 0 ||
      n_perm != (long long)I * cap)
    return SSAD_E_BADARG;
  if (!max_dets || !perm || !seg || !det_score || !det_rank || !dt_match || !dt_ignore || !cell_npig || !cell_eval ||
      !rec_thrs || !precision || !scores || !recall)
    return SSAD_E_BADARG;
  if (workspace_bytes < ssad_coco_eval_accumulate_workspace_bytes(K, A) || !workspace) return SSAD_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  long long* cat_npig = (long long*)workspace;
  int* cat_eval = (int*)((char*)workspace + al((size_t)K * A * sizeof(long long)));
  hipLaunchKernelGGL(coco_cells_kernel, dim3((K * (A + 1) + kT - 1) / kT), dim3(kT), 0, s, I, K, A, cell_npig,
                     cell_eval, cat_npig, cat_eval);
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3(K, M), dim3(kT), 0, s, K, A, T, M, R, max_dets, perm, seg, det_score,
                     det_rank, dt_match, dt_ignore, cat_npig, cat_eval, rec_thrs, precision, scores, recall);
  return (int)hipGetLastError();
}

}  // extern "C"
