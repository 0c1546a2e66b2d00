// softmax_cell.h -- one cell's group softmax in registers, and the dispatch by class count: what softmax_focal.hip's
// kernels and detect_batch.hip's candidate pass from logits share.  Both files instantiate the same templates through
// the same macro, so a given class count runs the same CMAX instance and the same FAST choice in both, and a
// probability computed in either carries the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdlib.h>

namespace {

constexpr int kMinClasses = 2;
constexpr int kMaxClasses = 128;

template <bool FAST> __device__ __forceinline__ float exp_f(float v) {
  if constexpr (FAST) return __expf(v); else return expf(v);
}

// ---- the cell in registers ---------------------------------------------------
// `base` (wave-uniform) points at class 0 of the slab; class c is hw floats further and the lane's
// cell `pos` floats into the plane.  The register indices are compile-time constants.  Registers
// c >= C hold a neutral value (-FLT_MAX before a softmax: exp underflows to exactly 0, so the max and
// the class-order sum keep their bits; 0 elsewhere), which keeps the arithmetic straight-line; only
// the stores are guarded, by a wave-uniform `c < C`.

template <int CMAX, bool NT>
__device__ __forceinline__ void load_cell(const float* __restrict__ base, unsigned hw, unsigned pos, int C,
                                          float fill, float (&v)[CMAX]) {
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    // classes past C re-read the last plane (a scalar clamp, no branch) and take `fill`
    const float* __restrict__ plane = base + (size_t)(c < C ? c : C - 1) * hw;
    float t;
    if constexpr (NT) t = __builtin_nontemporal_load(plane + pos);
    else t = plane[pos];
    v[c] = c < C ? t : fill;
  }
}

// v <- softmax(v) as the reference's three loops (.cu:36-55): max, exp(x - max) with the sum in
// class order, divide.  The fast path multiplies by one reciprocal instead of C divisions.
template <bool FAST, int CMAX>
__device__ __forceinline__ void softmax_cell(float (&v)[CMAX]) {
  float m = -FLT_MAX;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) m = fmaxf(m, v[c]);
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) { v[c] = exp_f<FAST>(v[c] - m); s += v[c]; }
  if constexpr (FAST) {
    const float inv = __frcp_rn(s);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) v[c] *= inv;
  } else {
#pragma unroll
    for (int c = 0; c < CMAX; ++c) v[c] = v[c] / s;
  }
}

// ---- host side ---------------------------------------------------------------

bool accurate_math() {
  static const bool v = [] {
    const char* e = getenv("SSAD_ACCURATE_MATH");
    return e && e[0] == '1';
  }();
  return v;
}

// KERNEL<FAST, CMAX> for the smallest CMAX that holds C
#define LAUNCH_BY_CLASSES(KERNEL, C_, ...)                                                  \
  do {                                                                                      \
    if (!accurate_math()) {                                                                 \
      if ((C_) <= 16) hipLaunchKernelGGL((KERNEL<true, 16>), __VA_ARGS__);                  \
      else if ((C_) <= 48) hipLaunchKernelGGL((KERNEL<true, 48>), __VA_ARGS__);             \
      else if ((C_) <= 96) hipLaunchKernelGGL((KERNEL<true, 96>), __VA_ARGS__);             \
      else hipLaunchKernelGGL((KERNEL<true, 128>), __VA_ARGS__);                            \
    } else {                                                                                \
      if ((C_) <= 16) hipLaunchKernelGGL((KERNEL<false, 16>), __VA_ARGS__);                 \
      else if ((C_) <= 48) hipLaunchKernelGGL((KERNEL<false, 48>), __VA_ARGS__);            \
      else if ((C_) <= 96) hipLaunchKernelGGL((KERNEL<false, 96>), __VA_ARGS__);            \
      else hipLaunchKernelGGL((KERNEL<false, 128>), __VA_ARGS__);                           \
    }                                                                                       \
  } while (0)

}  // namespace
