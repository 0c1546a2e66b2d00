// softmax_focal.hip -- GroupSpatialSoftmax (+Gradient) and SoftmaxFocalLoss (+Gradient) for
// gfx950 (MI355X): the RETINANET.SOFTMAX classification head.
//
// What the reference does (caffe2/modules/detectron/group_spatial_softmax_op.cu:26-87,
// softmax_focal_loss_op.cu:26-140): one thread per cell (image, anchor, y, x) walks the C class
// planes three times (max, exp + store, re-read + divide + store), a second kernel gathers the
// labelled probability into a full-size `losses_` temp, math::Sum reduces it in one block and
// math::Scale touches the scalar.  The gradient op writes a per-cell weight buffer, a second
// kernel reads it back once per logit, and math::Scale re-reads and re-writes all of dX.  The
// softmax gradient is a copy, a sum kernel, a subtract kernel and a Mul over the whole tensor.
//
// What this file does: ONE thread per cell too, but a workgroup takes 256 consecutive positions of
// ONE (image, anchor) slab: adjacent lanes = adjacent x, so every class plane is read and written
// as 256-byte wave rows, and the address of class c is a wave-uniform (scalar) base plus the
// lane's 32-bit position -- one address register per lane instead of a 64-bit pair per class.
// The cell's C values live in REGISTERS between the passes: each logit / probability leaves HBM
// once per kernel and each result is written once.  C is a run-time value (2..128); the register file is addressed statically by unrolling
// the class loops to a compile-time bound CMAX (16 / 48 / 96 / 128, the smallest that holds C)
// (registers past C hold a neutral value), so nothing is indexed dynamically and nothing spills.  C = 81
// runs the CMAX = 96 instance.  The labelled probability is picked up by a compare in the store
// loop, not by a gather.
//
// The loss is summed per thread in double, per workgroup by a wave shuffle tree, and per level by
// a second tiny launch that adds the workgroup partials in index order (the two-launch pattern of
// focal_fwd_kernel + distill_finalize_kernel): no float atomics, no arrival counters, and the bits
// do not depend on timing.  A level's workgroup count depends on that level's shape alone, so a
// five-level call and five one-level calls produce the same bits.
//
// A training step needs neither P nor a device-side dloss: softmax_focal_fused_kernel is the forward and the
// backward kernel joined at the cell's registers (logits read once, dX written once, the same reduction).
//
// All offsets are 64-bit: N*A*C*H*W may exceed 2^31.

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "ssad_kernels.h"
#include "softmax_cell.h"     // exp_f, load_cell, softmax_cell, LAUNCH_BY_CLASSES: shared with detect_batch.hip

namespace {

constexpr int kThreads = 256;
constexpr int kLevelBlocks = 1024;   // workgroups (= partial slots) per level: 4 waves per SIMD on 256 CUs

template <bool FAST> __device__ __forceinline__ float log_f(float v) {
  if constexpr (FAST) return __logf(v); else return logf(v);
}

// Work item = (slab, chunk): 256 consecutive positions of one (image, anchor) plane group.
struct Geometry {
  long long items;       // slabs * chunks
  unsigned hw;           // H * W  (< 2^31)
  unsigned chunks;       // ceil(hw / 256)
};

struct Level {
  const float* x;        // logits (forward) -- unused by the gradient
  const int32_t* g;      // labels, one per cell
  float* p;              // probabilities: written by the forward, read by the gradient; fused: written, or null
  float* out;            // forward: the scalar loss; gradient and fused: dX (finalize: the scalar loss)
  Geometry geo;
  int block_start;       // first blockIdx.x of this level
  int blocks;            // workgroups of this level
};

struct Args {
  Level lv[SSAD_MAX_LEVELS];
  int n_levels;
  int C;
  float gamma, alpha, scale;
};

__device__ __forceinline__ int find_level(const Args& a, int bid) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < SSAD_MAX_LEVELS; ++i)
    if (i < a.n_levels && bid >= a.lv[i].block_start) l = i;
  return l;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Sum over the 256-thread workgroup; result valid in thread 0.
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double wsum[kThreads / 64];
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) wsum[wid] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) t += wsum[i];
  }
  return t;
}

// item -> slab (wave-uniform) and this lane's position in the plane; false past the plane's end
__device__ __forceinline__ bool locate(const Geometry& G, long long item, long long* slab, unsigned* pos) {
  *slab = item / G.chunks;
  *pos = (unsigned)(item - *slab * G.chunks) * kThreads + threadIdx.x;
  return *pos < G.hw;
}

// (1 - p)^gamma and (1 - p)^(gamma - 1); gamma == 2 and gamma == 1 are multiplies.  Once per cell.
__device__ __forceinline__ void pow_pair(float omp, float gamma, float& pg, float& pgm1) {
  if (gamma == 2.0f) { pg = omp * omp; pgm1 = omp; }
  else if (gamma == 1.0f) { pg = omp; pgm1 = 1.0f; }
  else { pg = powf(omp, gamma); pgm1 = powf(omp, gamma - 1.0f); }
}

// ---- GroupSpatialSoftmax -------------------------------------------------------

// y = softmax over each cell's C classes.  drop: write classes 1..C-1 only, as N x (A*(C-1)) x H x W
// (the layout RetinanetDetector reads; core/test_retinanet.py:123-124 slices the background away).
template <bool FAST, int CMAX>
__global__ __launch_bounds__(kThreads) void group_softmax_kernel(
    const float* __restrict__ x, float* __restrict__ y, const Geometry G, int C, int drop) {
  const unsigned hw = G.hw;
  for (long long item = blockIdx.x; item < G.items; item += gridDim.x) {
    long long slab;
    unsigned pos;
    if (!locate(G, item, &slab, &pos)) continue;
    float v[CMAX];
    load_cell<CMAX, true>(x + (size_t)slab * C * hw, hw, pos, C, -FLT_MAX, v);
    softmax_cell<FAST, CMAX>(v);
    if (drop) {
      float* __restrict__ o = y + (size_t)slab * (C - 1) * hw;
#pragma unroll
      for (int c = 1; c < CMAX; ++c) if (c < C) (o + (size_t)(c - 1) * hw)[pos] = v[c];
    } else {
      float* __restrict__ o = y + (size_t)slab * C * hw;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) if (c < C) (o + (size_t)c * hw)[pos] = v[c];
    }
  }
}

// dX = Y * (dY - sum_c Y dY) per cell (.cu:59-87 + the Copy and the Mul of RunOnDevice): Y and dY
// of the cell are both held in registers, so each is read once and dX is written once.
template <int CMAX>
__global__ __launch_bounds__(kThreads) void group_softmax_grad_kernel(
    const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx, const Geometry G, int C) {
  const unsigned hw = G.hw;
  for (long long item = blockIdx.x; item < G.items; item += gridDim.x) {
    long long slab;
    unsigned pos;
    if (!locate(G, item, &slab, &pos)) continue;
    const size_t off = (size_t)slab * C * hw;
    float yv[CMAX], dv[CMAX];
    load_cell<CMAX, true>(y + off, hw, pos, C, 0.0f, yv);
    load_cell<CMAX, true>(dy + off, hw, pos, C, 0.0f, dv);
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) s += yv[c] * dv[c];
    float* __restrict__ o = dx + off;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) if (c < C) (o + (size_t)c * hw)[pos] = (dv[c] - s) * yv[c];
  }
}

// ---- SoftmaxFocalLoss -------------------------------------------------------------

// All levels in one launch: P = softmax(X) written once, the cell's loss
//   -(1 - p_label)^gamma * log(max(p_label, FLT_MIN)) * z,   z = [label == 0](1 - alpha)/Np + [label >= 1] alpha/Np
// (.cu:59-85) summed into one double per workgroup.  A label outside [-1, C) finds no class and is
// scored with p = 0 (the reference reads out of bounds there).
template <bool FAST, int CMAX>
__global__ __launch_bounds__(kThreads) void softmax_focal_fwd_kernel(
    const Args args, const float* __restrict__ fg_num, double* __restrict__ partials) {
  const Level& L = args.lv[find_level(args, blockIdx.x)];
  const int lb = blockIdx.x - L.block_start;
  const int C = args.C;
  const unsigned hw = L.geo.hw;
  const float np = fmaxf(fg_num[0], 1.0f);
  const float z_bg = (1.0f - args.alpha) / np, z_fg = args.alpha / np;
  double acc = 0.0;
  for (long long item = lb; item < L.geo.items; item += L.blocks) {
    long long slab;
    unsigned pos;
    if (!locate(L.geo, item, &slab, &pos)) continue;
    const size_t off = (size_t)slab * C * hw;
    const int label = (L.g + (size_t)slab * hw)[pos];
    float v[CMAX];
    load_cell<CMAX, true>(L.x + off, hw, pos, C, -FLT_MAX, v);
    softmax_cell<FAST, CMAX>(v);
    float* __restrict__ o = L.p + off;
    float pl = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) (o + (size_t)c * hw)[pos] = v[c];
      pl = (c == label) ? v[c] : pl;
    }
    if (label >= 0) {
      float pg, pgm1;
      pow_pair(1.0f - pl, args.gamma, pg, pgm1);
      const float z = label == 0 ? z_bg : z_fg;
      acc += (double)(-(pg * log_f<FAST>(fmaxf(pl, FLT_MIN))) * z);
    }
  }
  const double t = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// One workgroup per level: the level's partials in index order, then the float multiply by scale
// (math::Scale on one element, .cu:192-193).
__global__ __launch_bounds__(kThreads) void softmax_focal_finalize_kernel(
    const Args args, const double* __restrict__ partials) {
  const Level& L = args.lv[blockIdx.x];
  double v = 0.0;
  for (int i = threadIdx.x; i < L.blocks; i += kThreads) v += partials[L.block_start + i];
  const double t = block_sum(v);
  if (threadIdx.x == 0) L.out[0] = (float)t * args.scale;
}

// The reference's weight kernel, gradient kernel and math::Scale (.cu:88-140, 238-240) in one pass
// over P:  dX = scale * dloss * w * ([c == label] - P),
//   w = (-(1 - p)^gamma + gamma (1 - p)^(gamma - 1) p log(max(p, FLT_MIN))) * z,  p = P[label],
// and 0 for an ignored cell (label < 0), whose probabilities are not read.
template <bool FAST, int CMAX>
__global__ __launch_bounds__(kThreads) void softmax_focal_bwd_kernel(
    const Args args, const float* __restrict__ fg_num, const float* __restrict__ dloss, int dloss_stride) {
  const int level = find_level(args, blockIdx.x);
  const Level& L = args.lv[level];
  const int lb = blockIdx.x - L.block_start;
  const int C = args.C;
  const unsigned hw = L.geo.hw;
  const float np = fmaxf(fg_num[0], 1.0f);
  const float z_bg = (1.0f - args.alpha) / np, z_fg = args.alpha / np;
  const float dl = dloss[(size_t)level * dloss_stride];
  const float gamma = args.gamma, scale = args.scale;
  for (long long item = lb; item < L.geo.items; item += L.blocks) {
    long long slab;
    unsigned pos;
    if (!locate(L.geo, item, &slab, &pos)) continue;
    const size_t off = (size_t)slab * C * hw;
    const int label = (L.g + (size_t)slab * hw)[pos];
    float* __restrict__ o = L.out + off;
    if (label < 0) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c) if (c < C) (o + (size_t)c * hw)[pos] = 0.0f;
      continue;
    }
    float v[CMAX];
    load_cell<CMAX, false>(L.p + off, hw, pos, C, 0.0f, v);
    float pl = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) pl = (c == label) ? v[c] : pl;
    float pg, pgm1;
    pow_pair(1.0f - pl, gamma, pg, pgm1);
    const float z = label == 0 ? z_bg : z_fg;
    const float w = (-pg + gamma * pgm1 * pl * log_f<FAST>(fmaxf(pl, FLT_MIN))) * z;
    const float k = dl * w;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) (o + (size_t)c * hw)[pos] = (k * ((c == label ? 1.0f : 0.0f) - v[c])) * scale;
    }
  }
}

// Loss and dX of a training step in ONE pass over the logits (the forward and the backward kernel above, joined at
// the cell's registers): inside a step dloss is a constant and nobody reads P, so the logits are read once, dX is
// written once, and P goes to memory only for a level that has a P pointer.  Same formulas, same order of the
// operations as the pair; L.out is dX here and the level's loss is written by the finalize launch.  An ignored
// cell is computed like any other (straight-line code: its label matches no class) and selected away at the store,
// so a NaN in its logits reaches neither dX nor the loss.
template <bool FAST, int CMAX>
__global__ __launch_bounds__(kThreads) void softmax_focal_fused_kernel(
    const Args args, const float* __restrict__ fg_num, const float dl, double* __restrict__ partials) {
  const Level& L = args.lv[find_level(args, blockIdx.x)];
  const int lb = blockIdx.x - L.block_start;
  const int C = args.C;
  const unsigned hw = L.geo.hw;
  const float np = fmaxf(fg_num[0], 1.0f);
  const float z_bg = (1.0f - args.alpha) / np, z_fg = args.alpha / np;
  const float gamma = args.gamma, scale = args.scale;
  const bool want_p = L.p != nullptr;           // wave-uniform
  double acc = 0.0;
  for (long long item = lb; item < L.geo.items; item += L.blocks) {
    long long slab;
    unsigned pos;
    if (!locate(L.geo, item, &slab, &pos)) continue;
    const size_t off = (size_t)slab * C * hw;
    const int label = (L.g + (size_t)slab * hw)[pos];
    float v[CMAX];
    load_cell<CMAX, true>(L.x + off, hw, pos, C, -FLT_MAX, v);
    softmax_cell<FAST, CMAX>(v);
    float pl = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) pl = (c == label) ? v[c] : pl;
    if (want_p) {
      float* __restrict__ po = L.p + off;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) if (c < C) (po + (size_t)c * hw)[pos] = v[c];
    }
    const bool live = label >= 0;
    float pg, pgm1;
    pow_pair(1.0f - pl, gamma, pg, pgm1);
    const float z = label == 0 ? z_bg : z_fg;
    const float lg = log_f<FAST>(fmaxf(pl, FLT_MIN));
    if (live) acc += (double)(-(pg * lg) * z);
    const float w = (-pg + gamma * pgm1 * pl * lg) * z;
    const float k = dl * w;
    float* __restrict__ o = L.out + off;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      const float d = (k * ((c == label ? 1.0f : 0.0f) - v[c])) * scale;
      if (c < C) (o + (size_t)c * hw)[pos] = live ? d : 0.0f;
    }
  }
  const double t = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// ---- host side ---------------------------------------------------------------

bool classes_ok(int C) { return C >= kMinClasses && C <= kMaxClasses; }

// N x (A*C) x H x W -> work items; false for a non-positive extent or a plane of 2^31 positions or more
bool geometry(int N, int A, int H, int W, Geometry* G) {
  if (N <= 0 || A <= 0 || H <= 0 || W <= 0) return false;
  const long long hw = (long long)H * W;
  if (hw >= (1LL << 31) - kThreads) return false;
  G->hw = (unsigned)hw;
  G->chunks = (unsigned)((hw + kThreads - 1) / kThreads);
  G->items = (long long)N * A * G->chunks;
  return true;
}

int grid_for(long long items, int cap) { return (int)(items < cap ? items : cap); }

// Level table of the focal loss: validates, assigns each level min(items, kLevelBlocks) workgroups (a
// function of that level alone).
int build_args(const ssad_softmax_focal_level* lv, int n_levels, const ssad_focal_params* P, bool backward,
               Args* out, int* total_blocks, bool fused = false) {
  if (!lv || !P || n_levels < 0 || n_levels > SSAD_MAX_LEVELS) return SSAD_E_BADARG;
  if (!classes_ok(P->num_classes) || !(P->scale >= 0.0f)) return SSAD_E_BADARG;
  Args& a = *out;
  a.n_levels = n_levels;
  a.C = P->num_classes;
  a.gamma = P->gamma; a.alpha = P->alpha; a.scale = P->scale;
  int start = 0;
  for (int l = 0; l < n_levels; ++l) {
    const ssad_softmax_focal_level& s = lv[l];
    // (the fused pass writes P only where a level has a P pointer)
    if (!s.labels || (!s.prob && !fused) || !s.out || (!backward && !s.logits)) return SSAD_E_BADARG;
    if (s.D <= 0 || s.D % P->num_classes != 0) return SSAD_E_BADARG;
    Level& L = a.lv[l];
    if (!geometry(s.N, s.D / P->num_classes, s.H, s.W, &L.geo)) return SSAD_E_BADARG;
    L.x = s.logits; L.g = s.labels; L.p = s.prob; L.out = s.out;
    L.block_start = start;
    L.blocks = grid_for(L.geo.items, kLevelBlocks);
    start += L.blocks;
  }
  for (int l = n_levels; l < SSAD_MAX_LEVELS; ++l) {
    a.lv[l] = Level{nullptr, nullptr, nullptr, nullptr, Geometry{0, 1, 1}, start, 0};
  }
  *total_blocks = start;
  return 0;
}

}  // namespace

extern "C" {

int ssad_group_spatial_softmax(const float* x, float* y, int N, int A, int C, int H, int W, int drop_background,
                               ssad_stream_t stream) {
  Geometry G;
  if (!x || !y || !classes_ok(C) || !geometry(N, A, H, W, &G)) return SSAD_E_BADARG;
  const int grid = grid_for(G.items, 4 * kLevelBlocks);
  LAUNCH_BY_CLASSES(group_softmax_kernel, C, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x, y, G, C,
                    drop_background ? 1 : 0);
  return (int)hipGetLastError();
}

int ssad_group_spatial_softmax_grad(const float* y, const float* dy, float* dx, int N, int A, int C, int H, int W,
                                    ssad_stream_t stream) {
  Geometry G;
  if (!y || !dy || !dx || !classes_ok(C) || !geometry(N, A, H, W, &G)) return SSAD_E_BADARG;
  const int grid = grid_for(G.items, 4 * kLevelBlocks);
  hipStream_t s = (hipStream_t)stream;
  if (C <= 16) hipLaunchKernelGGL(group_softmax_grad_kernel<16>, dim3(grid), dim3(kThreads), 0, s, y, dy, dx, G, C);
  else if (C <= 48) hipLaunchKernelGGL(group_softmax_grad_kernel<48>, dim3(grid), dim3(kThreads), 0, s, y, dy, dx, G, C);
  else if (C <= 96) hipLaunchKernelGGL(group_softmax_grad_kernel<96>, dim3(grid), dim3(kThreads), 0, s, y, dy, dx, G, C);
  else hipLaunchKernelGGL(group_softmax_grad_kernel<128>, dim3(grid), dim3(kThreads), 0, s, y, dy, dx, G, C);
  return (int)hipGetLastError();
}

size_t ssad_softmax_focal_loss_workspace_bytes(int n_levels) {
  if (n_levels < 1) n_levels = 1;
  if (n_levels > SSAD_MAX_LEVELS) n_levels = SSAD_MAX_LEVELS;
  return sizeof(double) * kLevelBlocks * (size_t)n_levels;
}

int ssad_softmax_focal_loss_forward(const ssad_softmax_focal_level* levels_host, int n_levels, const float* fg_num,
                                    const ssad_focal_params* params_host, void* workspace, size_t workspace_bytes,
                                    ssad_stream_t stream) {
  Args a;
  int blocks = 0;
  const int rc = build_args(levels_host, n_levels, params_host, false, &a, &blocks);
  if (rc) return rc;
  if (!fg_num) return SSAD_E_BADARG;
  if (n_levels == 0) return 0;
  if (!workspace || workspace_bytes < sizeof(double) * (size_t)blocks) return SSAD_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)workspace;
  LAUNCH_BY_CLASSES(softmax_focal_fwd_kernel, a.C, dim3(blocks), dim3(kThreads), 0, s, a, fg_num, partials);
  hipLaunchKernelGGL(softmax_focal_finalize_kernel, dim3(n_levels), dim3(kThreads), 0, s, a,
                     (const double*)partials);
  return (int)hipGetLastError();
}

int ssad_softmax_focal_loss_backward(const ssad_softmax_focal_level* levels_host, int n_levels, const float* fg_num,
                                     const float* dloss, int dloss_stride, const ssad_focal_params* params_host,
                                     ssad_stream_t stream) {
  Args a;
  int blocks = 0;
  const int rc = build_args(levels_host, n_levels, params_host, true, &a, &blocks);
  if (rc) return rc;
  if (!fg_num || !dloss || dloss_stride < 0) return SSAD_E_BADARG;
  if (n_levels == 0) return 0;
  LAUNCH_BY_CLASSES(softmax_focal_bwd_kernel, a.C, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, fg_num,
                    dloss, dloss_stride);
  return (int)hipGetLastError();
}

size_t ssad_softmax_focal_loss_fused_workspace_bytes(int n_levels) {
  return ssad_softmax_focal_loss_workspace_bytes(n_levels);
}

int ssad_softmax_focal_loss_fused(const ssad_softmax_focal_level* levels_host, int n_levels, const float* fg_num,
                                  float dloss, const ssad_focal_params* params_host, float* losses, void* workspace,
                                  size_t workspace_bytes, ssad_stream_t stream) {
  Args a;
  int blocks = 0;
  const int rc = build_args(levels_host, n_levels, params_host, false, &a, &blocks, true);
  if (rc) return rc;
  if (!fg_num || !losses) return SSAD_E_BADARG;
  if (n_levels == 0) return 0;
  if (!workspace || workspace_bytes < sizeof(double) * (size_t)blocks) return SSAD_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)workspace;
  LAUNCH_BY_CLASSES(softmax_focal_fused_kernel, a.C, dim3(blocks), dim3(kThreads), 0, s, a, fg_num, dloss, partials);
  Args fin = a;                  // the finalize launch writes out[0]: level l's loss is losses[l]
  for (int l = 0; l < n_levels; ++l) fin.lv[l].out = losses + l;
  hipLaunchKernelGGL(softmax_focal_finalize_kernel, dim3(n_levels), dim3(kThreads), 0, s, fin,
                     (const double*)partials);
  return (int)hipGetLastError();
}

}  // extern "C"
