// soft_nms.hip -- the two post-processing options of the reference's test path (detectron/lib/core/test.py:779-797)
// on the device: Soft-NMS (utils/cython_nms.pyx:98-203 behind utils/boxes.py:321-338; hard, linear, gaussian) and
// bounding-box voting (utils/boxes.py:262-311, IoU of utils/cython_bbox.pyx:32-72).  Both work on the class-sorted
// candidate arrays of detect.hip (boxes [n][4], scores [n], cls [n] ascending, -1 in the empty trailing slots) and on
// its 64-bit survivor keys, so its rank sort and emit kernel serve them unchanged.
//
// Soft-NMS is not the greedy kernel with other weights: every pick changes the scores that decide the next pick, so
// no suppression bit-matrix can be computed ahead.  One workgroup per class keeps the segment's boxes and CURRENT
// scores in LDS (20 bytes a candidate, up to SSAD_SOFT_NMS_LDS_CAP = 1024 of them = 20 KiB; longer segments keep the
// scores in the global workspace and read the boxes where they lie) and repeats: arg-max of the live scores -> the
// pick; one pass of every thread over its own candidates (j = thread, thread + 256, ...) that decays them against the
// pick and gathers the next arg-max on the way.  One barrier a pick.  The definition is free of the reference's swap
// bookkeeping (see include/ssad_kernels.h); it is the reference's result whenever no two current scores tie at a
// pick, and among equal scores the lower position goes first.  Worst case -- all n candidates in one class, none
// retired -- the walk is n serial picks of n / 256 candidates a thread.
//
// Both kernels take the image from the grid (blockIdx.y) and address every per-image array as base + image * n, so
// a minibatch's classes share one launch (detect_batch.hip); the single-image entries launch one image.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssad_kernels.h"
#include "soft_nms_images.h"

// The scores must come out as the reference's float32 arithmetic rounds them, one operation at a time.  hipcc
// contracts a * b + c into an FMA by default, and the __fmul_rn / __fadd_rn of the HIP headers do not stop it (their
// bodies are plain operators that carry the contraction flag with them): nothing in this file is contracted, and
// the four helpers below are its rounded operations.
#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kCap = SSAD_SOFT_NMS_LDS_CAP;
constexpr unsigned kDead = 0xffffffffu;      // score word of a picked / retired candidate (no score: a NaN pattern)

typedef unsigned long long u64;

__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rn_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_div(float a, float b) { return a / b; }    // IEEE division (hipcc's default)

// float bits -> unsigned that orders like the float (negative scores included), and back
__device__ __forceinline__ unsigned ordered(unsigned b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ unsigned unordered(unsigned o) { return o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu); }

// arg-max key of a live candidate: never 0 (position < 2^32 - 1); larger score first, then the lower position
__device__ __forceinline__ u64 pick_key(unsigned score_bits, int pos) {
  return ((u64)ordered(score_bits) << 32) | (u64)(~(unsigned)pos);
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), d, 64), lo = __shfl_xor((unsigned)v, d, 64);
    const u64 o = ((u64)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// every thread gets the maximum over the workgroup; `slot` is one of two buffers used in turn, so one barrier is
// enough: a buffer is rewritten two calls later, after the barrier of the call in between
__device__ __forceinline__ u64 block_max(u64 v, u64* slot) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) { const u64 o = slot[w]; v = o > v ? o : v; }
  return v;
}

__device__ __forceinline__ float area_of(const float* b) {
  return rn_mul(rn_add(rn_sub(b[2], b[0]), 1.0f), rn_add(rn_sub(b[3], b[1]), 1.0f));
}

// the class's segment [seg[0], seg[1]) of the class-sorted arrays; thread 0 searches, the caller synchronises
__device__ __forceinline__ void find_segment(const int* cls, int n, int c, int* seg) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; const int v = cls[m]; if (v >= 0 && v < c) lo = m + 1; else hi = m; }
  seg[0] = lo;
  hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; const int v = cls[m]; if (v >= 0 && v <= c) lo = m + 1; else hi = m; }
  seg[1] = lo;
}

// bx: the segment's boxes, sc: its current score words (LDS or global; a thread touches only its own words of sc)
__device__ __forceinline__ void soft_nms_walk(const float* bx, unsigned* sc, int s, int L, int method, float sigma,
                                              float nt, float thresh, u64* keys, int* rank_out, u64 (*wmax)[kWaves]) {
  const int t = threadIdx.x;
  u64 local = 0;
  for (int j = t; j < L; j += kT) { const u64 k = pick_key(sc[j], j); local = k > local ? k : local; }
  int rank = 0;
  for (;;) {
    const u64 best = block_max(local, wmax[rank & 1]);      // (the barrier also publishes the LDS boxes on round 0)
    if (best == 0) break;                                   // nothing live: uniform
    const int p = (int)(~(unsigned)best);
    if ((p & (kT - 1)) == t) {                              // the pick's owner records and retires it
      sc[p] = kDead;
      keys[s + p] = ((u64)unordered((unsigned)(best >> 32)) << 32) | (u64)(~(unsigned)(s + p));
      rank_out[s + p] = rank;
    }
    ++rank;
    float tb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) tb[q] = bx[(long long)p * 4 + q];
    const float ta = area_of(tb);
    local = 0;
    for (int j = t; j < L; j += kT) {
      const unsigned bits = sc[j];
      if (bits == kDead) continue;
      float sj = __uint_as_float(bits);
      const float* cb = bx + (long long)j * 4;
      // cython_nms.pyx:166-172
      const float iw = rn_add(rn_sub(fminf(tb[2], cb[2]), fmaxf(tb[0], cb[0])), 1.0f);
      if (iw > 0.0f) {
        const float ih = rn_add(rn_sub(fminf(tb[3], cb[3]), fmaxf(tb[1], cb[1])), 1.0f);
        if (ih > 0.0f) {
          const float inter = rn_mul(iw, ih);
          const float ov = rn_div(inter, rn_sub(rn_add(ta, area_of(cb)), inter));
          float w;
          if (method == SSAD_NMS_SOFT_LINEAR) w = ov > nt ? rn_sub(1.0f, ov) : 1.0f;
          else if (method == SSAD_NMS_SOFT_GAUSSIAN) w = expf(rn_div(-rn_mul(ov, ov), sigma));
          else w = ov > nt ? 0.0f : 1.0f;
          sj = rn_mul(w, sj);
          if (sj < thresh) {                                // :191 -- tested only where a weight was applied
            sc[j] = kDead;
            keys[s + j] = 0;
            rank_out[s + j] = -1;
            continue;
          }
          sc[j] = __float_as_uint(sj);
        }
      }
      const u64 k = pick_key(__float_as_uint(sj), j);
      local = k > local ? k : local;
    }
  }
}

__global__ __launch_bounds__(kT) void soft_nms_kernel(int n, const float* boxes, const float* scores, const int* cls,
                                                      int method, float sigma, float nt, float thresh, u64* keys,
                                                      int* rank_out, unsigned* live) {
  {
    const long long im = (long long)blockIdx.y * n;             // this image's arrays
    boxes += im * 4; scores += im; cls += im; keys += im; rank_out += im; live += im;
  }
  __shared__ float lbox[kCap * 4];
  __shared__ unsigned lsc[kCap];
  __shared__ u64 wmax[2][kWaves];
  __shared__ int seg[2];
  if (threadIdx.x == 0) find_segment(cls, n, blockIdx.x, seg);
  __syncthreads();
  const int s = seg[0], L = seg[1] - seg[0];
  if (L == 0) return;
  if (L <= kCap) {
    for (int j = threadIdx.x; j < L; j += kT) {
      lsc[j] = __float_as_uint(scores[s + j]);
#pragma unroll
      for (int q = 0; q < 4; ++q) lbox[j * 4 + q] = boxes[(long long)(s + j) * 4 + q];
    }
    soft_nms_walk(lbox, lsc, s, L, method, sigma, nt, thresh, keys, rank_out, wmax);
  } else {
    for (int j = threadIdx.x; j < L; j += kT) live[s + j] = __float_as_uint(scores[s + j]);
    soft_nms_walk(boxes + (long long)s * 4, live + s, s, L, method, sigma, nt, thresh, keys, rank_out, wmax);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// one wave per top detection; blockIdx.y = image
__global__ __launch_bounds__(64) void box_voting_kernel(int m, const float* top_boxes, const int* top_cls,
                                                        const float* boxes, const float* scores, const int* cls, int n,
                                                        float vote_thresh, int scoring, float beta, u64* keys,
                                                        float* voted) {
  const int k = blockIdx.x;
  if (k >= m) return;
  {
    const long long tm = (long long)blockIdx.y * m, im = (long long)blockIdx.y * n;
    top_boxes += tm * 4; top_cls += tm; keys += tm; voted += tm * 4;
    boxes += im * 4; scores += im; cls += im;
  }
  const u64 key = keys[k];
  const int c = top_cls[k];
  if (key == 0 || c < 0) return;                              // uniform
  int seg[2];
  find_segment(cls, n, c, seg);                               // every lane the same search
  float tb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) tb[q] = top_boxes[(long long)k * 4 + q];
  const float ta = area_of(tb);
  const float inv_beta = 1.0f / beta;
  float sw = 0.0f, sb[4] = {0.0f, 0.0f, 0.0f, 0.0f}, cnt = 0.0f, siou = 0.0f, spiou = 0.0f, sgen = 0.0f, stemp = 0.0f;
  for (int j = seg[0] + (int)threadIdx.x; j < seg[1]; j += 64) {
    const float* cb = boxes + (long long)j * 4;
    // cython_bbox.pyx:52-72 (0 where the boxes do not meet)
    float ov = 0.0f;
    const float iw = rn_add(rn_sub(fminf(tb[2], cb[2]), fmaxf(tb[0], cb[0])), 1.0f);
    if (iw > 0.0f) {
      const float ih = rn_add(rn_sub(fminf(tb[3], cb[3]), fmaxf(tb[1], cb[1])), 1.0f);
      if (ih > 0.0f) {
        const float inter = rn_mul(iw, ih);
        ov = rn_div(inter, rn_sub(rn_add(ta, area_of(cb)), inter));
      }
    }
    if (!(ov >= vote_thresh)) continue;
    const float w = scores[j];
    sw += w;
    cnt += 1.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) sb[q] += w * cb[q];
    if (scoring == SSAD_VOTE_IOU_AVG) { siou += ov; spiou += w * ov; }
    else if (scoring == SSAD_VOTE_GENERALIZED_AVG) sgen += powf(w, beta);
    else if (scoring == SSAD_VOTE_TEMP_AVG) {
      const float q1 = 1.0f - w, mx = fmaxf(w, q1);
      const float a = powf(w / mx, inv_beta), b = powf(q1 / mx, inv_beta);
      stemp += a / (a + b);
    }
  }
  sw = wave_sum(sw); cnt = wave_sum(cnt);
#pragma unroll
  for (int q = 0; q < 4; ++q) sb[q] = wave_sum(sb[q]);
  siou = wave_sum(siou); spiou = wave_sum(spiou); sgen = wave_sum(sgen); stemp = wave_sum(stemp);
  if (threadIdx.x != 0) return;
  float* out = voted + (long long)k * 4;
  if (cnt == 0.0f) {                                          // a foreign top box that met nothing: left as it is
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = tb[q];
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) out[q] = sb[q] / sw;
  float score;
  switch (scoring) {
    case SSAD_VOTE_AVG: score = sw / cnt; break;
    case SSAD_VOTE_IOU_AVG: score = spiou / siou; break;
    case SSAD_VOTE_GENERALIZED_AVG: score = powf(sgen / cnt, inv_beta); break;
    case SSAD_VOTE_QUASI_SUM: score = sw / powf(cnt, beta); break;
    case SSAD_VOTE_TEMP_AVG: score = stemp / cnt; break;
    default: return;                                          // SSAD_VOTE_ID
  }
  keys[k] = ((u64)__float_as_uint(score) << 32) | (key & 0xffffffffull);
}

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int ssad_soft_nms_images(const float* boxes, const float* scores, const int* cls, int n, int images, int C, int method,
                         float sigma, float Nt, float score_thresh, unsigned long long* keys_out, int* pick_rank_out,
                         unsigned* live, hipStream_t s) {
  // the empty trailing slots belong to no class: no workgroup writes them
  (void)hipMemsetAsync(keys_out, 0, (size_t)images * n * 8, s);
  (void)hipMemsetAsync(pick_rank_out, 0xff, (size_t)images * n * 4, s);
  hipLaunchKernelGGL(soft_nms_kernel, dim3((unsigned)C, (unsigned)images), dim3(kT), 0, s, n, boxes, scores, cls,
                     method, sigma, Nt, score_thresh, keys_out, pick_rank_out, live);
  return (int)hipGetLastError();
}

int ssad_box_voting_images(const float* top_boxes, const int* top_cls, int m, const float* boxes, const float* scores,
                           const int* cls, int n, int images, float vote_thresh, int scoring_method, float beta,
                           unsigned long long* keys_inout, float* voted_boxes_out, hipStream_t s) {
  hipLaunchKernelGGL(box_voting_kernel, dim3((unsigned)m, (unsigned)images), dim3(64), 0, s, m, top_boxes, top_cls,
                     boxes, scores, cls, n, vote_thresh, scoring_method, beta, keys_inout, voted_boxes_out);
  return (int)hipGetLastError();
}

extern "C" {

size_t ssad_soft_nms_workspace_bytes(int n) { return n > 0 ? al((size_t)n * 4) : 0; }

int ssad_soft_nms(const float* boxes, const float* scores, const int* cls, int n, int C, int method, float sigma,
                  float Nt, float score_thresh, unsigned long long* keys_out, int* pick_rank_out, void* workspace,
                  size_t workspace_bytes, ssad_stream_t stream) {
  if (n < 0 || C < 1 || method < SSAD_NMS_SOFT_HARD || method > SSAD_NMS_SOFT_GAUSSIAN || !(sigma > 0.0f))
    return SSAD_E_BADARG;
  if (n == 0) return 0;
  if (!boxes || !scores || !cls || !keys_out || !pick_rank_out) return SSAD_E_BADARG;
  if (!workspace || workspace_bytes < ssad_soft_nms_workspace_bytes(n)) return SSAD_E_WORKSPACE;
  return ssad_soft_nms_images(boxes, scores, cls, n, 1, C, method, sigma, Nt, score_thresh, keys_out, pick_rank_out,
                              (unsigned*)workspace, (hipStream_t)stream);
}

int ssad_box_voting(const float* top_boxes, const int* top_cls, int m, const float* boxes, const float* scores,
                    const int* cls, int n, int C, float vote_thresh, int scoring_method, float beta,
                    unsigned long long* keys_inout, float* voted_boxes_out, ssad_stream_t stream) {
  if (m < 0 || n < 0 || C < 1 || scoring_method < SSAD_VOTE_ID || scoring_method > SSAD_VOTE_QUASI_SUM)
    return SSAD_E_BADARG;
  const bool exponent = scoring_method == SSAD_VOTE_TEMP_AVG || scoring_method == SSAD_VOTE_GENERALIZED_AVG ||
                        scoring_method == SSAD_VOTE_QUASI_SUM;
  if (exponent && !(beta > 0.0f)) return SSAD_E_BADARG;
  if (m == 0) return 0;
  if (!top_boxes || !top_cls || !keys_inout || !voted_boxes_out || (n > 0 && (!boxes || !scores || !cls)))
    return SSAD_E_BADARG;
  return ssad_box_voting_images(top_boxes, top_cls, m, boxes, scores, cls, n, 1, vote_thresh, scoring_method,
                                exponent ? beta : 1.0f, keys_inout, voted_boxes_out, (hipStream_t)stream);
}

}  // extern "C"
