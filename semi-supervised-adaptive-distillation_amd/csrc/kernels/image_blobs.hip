// image_blobs.hip -- the `data` and `teacher/data` input blobs built on the device from
// decoded uint8 images: what the reference does on the host, per image and once per network
// (detectron/lib/roi_data/minibatch.py:102-134, detectron/lib/utils/blob.py:40-106):
//   preprocess_im    t = ((float)u8 / div - mean[c]) / std[c]            (blob.py:70-75)
//   cv2.resize       float INTER_LINEAR with fx = fy = im_scale          (blob.py:102-103)
//   im_list_to_blob  zero padding to the blob size, HWC -> NCHW          (blob.py:40-68)
// The host uploads the packed uint8 HWC BGR pixels once; one launch writes both blobs.
//
// Definition (written from cv2's algorithm; cv2 itself is not part of this project's tests):
// element (n, c, y, x) of a blob [N][3][Hb][Wb] is +0.0f for y >= oh or x >= ow, otherwise
//   fxd = (x + 0.5) * (1.0 / s) - 0.5 in double (two roundings, never an FMA), fx = (float)fxd,
//   sx = floorf(fx), ax = fx - sx; sx < 0 -> (0, 0); sx >= w - 1 -> (w - 1, 0); sx1 = min(sx + 1, w - 1)
// (rows alike with h), a flipped image reads source column w - 1 - col, and
//   out = (1 - ay) * ((1 - ax) * t00 + ax * t01) + ay * ((1 - ax) * t10 + ax * t11)   in float.
//
// Two launches per call:
//  * image_tables_kernel (tiny): the [norm][channel][256] table of every value a tap can take,
//    computed with the exact expression above (true divisions), and per image the column entries
//    (source column after the flip, its right neighbour, ax) for every x < Wb and the row entries
//    for every y < Hb.  Every entry is clamped into the image, for padding coordinates too, so
//    whatever the main kernel reads through them lies inside the source buffer.
//  * image_blobs_kernel: a thread owns four consecutive x of one row for the three channels of
//    both blobs: six 16-byte stores, coalesced; the 6 KB tap table sits in LDS, so the inner loop
//    has no division and the taps stay bit-exact; padding is written here (the destination needs
//    no memset), a quad that straddles ow selects per element.  Measured at config 3's input:
//    2.75 x the time of a plain fill of the same 220 MB, so not write-bound; what bounds it has
//    not been identified, no counter run was made (profiles/image_blobs.md).
// The per-image sizes reach both kernels by value (hence SSAD_IMAGE_BLOBS_MAX_BATCH); the
// launcher validates all of them before the first launch.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssad_kernels.h"

namespace {

constexpr int kT = 256;
constexpr int kQuadsPerThread = 4;      // one table fill serves 1024 quads
constexpr int kLut = 3 * 256;           // tap values of one blob

struct IBImage {
  long long offset;                // first byte of the image in src
  double inv_scale;                // 1.0 / s
  int h, w, oh, ow;
  int flipped, pad_;
};

struct IBArgs {
  IBImage img[SSAD_IMAGE_BLOBS_MAX_BATCH];
  const unsigned char* src;
  float* out[2];
  float div[2], mean[2][3], std_[2][3];
  int N, Hb, Wb, n_norms;
  // workspace
  float* lut;                      // [2][3][256]
  int* col0; int* col1; float* ax; // [N][Wb] each
  int* row0; int* row1; float* ay; // [N][Hb] each
};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// One axis of the resize: destination coordinate i -> (source index, its neighbour, weight).
__device__ inline void axis_entry(int i, double inv_scale, int len, int* s0, int* s1, float* a) {
  const double fd = __dsub_rn(__dmul_rn((double)i + 0.5, inv_scale), 0.5);
  const float f = (float)fd;
  const float fl = floorf(f);
  int s = 0;
  float w = 0.0f;
  if (fl >= (float)(len - 1)) {    // also +Inf
    s = len - 1;
  } else if (fl >= 0.0f) {
    s = (int)fl;
    w = f - fl;
  }
  *s0 = s;
  *s1 = s + 1 < len ? s + 1 : len - 1;
  *a = w;
}

__global__ __launch_bounds__(kT) void image_tables_kernel(const IBArgs a) {
  int i = blockIdx.x * kT + threadIdx.x;
  const int n_lut = a.n_norms * kLut;
  if (i < n_lut) {
    const int k = i / kLut, c = (i / 256) % 3, v = i & 255;
    const float t = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, a.div[k]), a.mean[k][c]), a.std_[k][c]);
    a.lut[i] = t;
    return;
  }
  i -= n_lut;
  if (i < a.N * a.Wb) {
    const int n = i / a.Wb, x = i - n * a.Wb;
    const IBImage& im = a.img[n];
    int s0, s1;
    float w;
    axis_entry(x, im.inv_scale, im.w, &s0, &s1, &w);
    a.col0[i] = im.flipped ? im.w - 1 - s0 : s0;
    a.col1[i] = im.flipped ? im.w - 1 - s1 : s1;
    a.ax[i] = w;
    return;
  }
  i -= a.N * a.Wb;
  if (i < a.N * a.Hb) {
    const int n = i / a.Hb, y = i - n * a.Hb;
    const IBImage& im = a.img[n];
    axis_entry(y, im.inv_scale, im.h, &a.row0[i], &a.row1[i], &a.ay[i]);
  }
}

template <int NB>
__global__ __launch_bounds__(kT) void image_blobs_kernel(const IBArgs a) {
  __shared__ float lut[NB * kLut];
  for (int i = threadIdx.x; i < NB * kLut / 4; i += kT)
    reinterpret_cast<float4*>(lut)[i] = reinterpret_cast<const float4*>(a.lut)[i];
  __syncthreads();
  const int Wq = a.Wb >> 2;
  const int total = a.N * a.Hb * Wq;               // < 2^31 / 12 (launcher)
  const size_t plane = (size_t)a.Hb * a.Wb;
  const int first = blockIdx.x * (kT * kQuadsPerThread) + threadIdx.x;
#pragma unroll 1
  for (int it = 0; it < kQuadsPerThread; ++it) {
    const int q = first + it * kT;
    if (q >= total) return;
    const int xq = q % Wq, row = q / Wq;           // row = n * Hb + y
    const int n = row / a.Hb, y = row - n * a.Hb;
    const int x0 = xq << 2;
    const long long offset = a.img[n].offset;
    const int w = a.img[n].w, oh = a.img[n].oh, ow = a.img[n].ow;
    const size_t o = (size_t)n * 3 * plane + (size_t)y * a.Wb + x0;
    float res[NB][3][4];
    if (y >= oh || x0 >= ow) {
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j) res[k][c][j] = 0.0f;
    } else {
      const int ci = n * a.Wb + x0;
      const int4 c0 = *reinterpret_cast<const int4*>(a.col0 + ci);
      const int4 c1 = *reinterpret_cast<const int4*>(a.col1 + ci);
      const float4 axv = *reinterpret_cast<const float4*>(a.ax + ci);
      const float ay = a.ay[row];
      const unsigned char* p0 = a.src + offset + (long long)a.row0[row] * w * 3;
      const unsigned char* p1 = a.src + offset + (long long)a.row1[row] * w * 3;
      const int c0s[4] = {c0.x, c0.y, c0.z, c0.w};
      const int c1s[4] = {c1.x, c1.y, c1.z, c1.w};
      const float axs[4] = {axv.x, axv.y, axv.z, axv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long b0 = 3LL * c0s[j], b1 = 3LL * c1s[j];
        const float ax = axs[j];
        const bool inside = x0 + j < ow;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int u00 = p0[b0 + c], u01 = p0[b1 + c], u10 = p1[b0 + c], u11 = p1[b1 + c];
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const float* t = lut + (k * 3 + c) * 256;
            const float top = (1.0f - ax) * t[u00] + ax * t[u01];
            const float bot = (1.0f - ax) * t[u10] + ax * t[u11];
            const float v = (1.0f - ay) * top + ay * bot;
            res[k][c][j] = inside ? v : 0.0f;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(a.out[k] + o + c * plane) =
            make_float4(res[k][c][0], res[k][c][1], res[k][c][2], res[k][c][3]);
  }
}

// 0 when the shape is unsupported
size_t plan_bytes(int N, int Hb, int Wb) {
  if (N < 1 || N > SSAD_IMAGE_BLOBS_MAX_BATCH || Hb < 1 || Wb < 4 || (Wb & 3)) return 0;
  if ((unsigned long long)N * 3 * (unsigned long long)Hb * (unsigned long long)Wb >= (1ull << 31)) return 0;
  return align256(2 * kLut * sizeof(float)) + 3 * align256((size_t)N * Wb * 4) + 3 * align256((size_t)N * Hb * 4);
}

}  // namespace

extern "C" {

size_t ssad_image_blobs_workspace_bytes(int N, int Hb, int Wb) { return plan_bytes(N, Hb, Wb); }

int ssad_image_blobs(const unsigned char* src, size_t src_bytes, const long long* offset_host,
                     const int* h_host, const int* w_host, const int* out_h_host, const int* out_w_host,
                     const double* scale_host, const int* flipped_host, int N, int Hb, int Wb,
                     const ssad_image_norm* norms_host, int n_norms, void* workspace,
                     size_t workspace_bytes, ssad_stream_t stream) {
  if (!src || !offset_host || !h_host || !w_host || !out_h_host || !out_w_host || !scale_host ||
      !flipped_host || !norms_host)
    return SSAD_E_BADARG;
  if (n_norms != 1 && n_norms != 2) return SSAD_E_BADARG;
  const size_t need = plan_bytes(N, Hb, Wb);
  if (!need) return SSAD_E_BADARG;
  IBArgs a;
  for (int k = 0; k < n_norms; ++k) {
    const ssad_image_norm& nm = norms_host[k];
    if (!nm.out || ((uintptr_t)nm.out & 15)) return SSAD_E_BADARG;     // 16-byte stores
    if (!(nm.div != 0.0f) || !isfinite(nm.div)) return SSAD_E_BADARG;
    a.out[k] = nm.out;
    a.div[k] = nm.div;
    for (int c = 0; c < 3; ++c) {
      if (!(nm.std[c] != 0.0f) || !isfinite(nm.std[c]) || !isfinite(nm.mean[c])) return SSAD_E_BADARG;
      a.mean[k][c] = nm.mean[c];
      a.std_[k][c] = nm.std[c];
    }
  }
  if (n_norms == 1) {
    a.out[1] = nullptr;
    a.div[1] = 1.0f;
    for (int c = 0; c < 3; ++c) { a.mean[1][c] = 0.0f; a.std_[1][c] = 1.0f; }
  }
  for (int n = 0; n < N; ++n) {
    const int h = h_host[n], w = w_host[n], oh = out_h_host[n], ow = out_w_host[n];
    const long long off = offset_host[n];
    const double s = scale_host[n];
    if (h < 1 || w < 1 || oh < 1 || ow < 1 || oh > Hb || ow > Wb) return SSAD_E_BADARG;
    if (!(s > 0.0) || !isfinite(s)) return SSAD_E_BADARG;
    // offset + 3 h w <= src_bytes, without overflow: h w < 2^62
    if (off < 0 || (unsigned long long)off > src_bytes) return SSAD_E_BADARG;
    if ((unsigned long long)h * (unsigned long long)w > (src_bytes - (unsigned long long)off) / 3)
      return SSAD_E_BADARG;
    IBImage& im = a.img[n];
    im.offset = off; im.inv_scale = 1.0 / s;
    im.h = h; im.w = w; im.oh = oh; im.ow = ow;
    im.flipped = flipped_host[n] != 0; im.pad_ = 0;
  }
  for (int n = N; n < SSAD_IMAGE_BLOBS_MAX_BATCH; ++n) a.img[n] = IBImage{0, 1.0, 1, 1, 1, 1, 0, 0};
  if (!workspace || ((uintptr_t)workspace & 15)) return SSAD_E_BADARG;
  if (workspace_bytes < need) return SSAD_E_WORKSPACE;
  a.src = src; a.N = N; a.Hb = Hb; a.Wb = Wb; a.n_norms = n_norms;
  char* p = (char*)workspace;
  a.lut = (float*)p; p += align256(2 * kLut * sizeof(float));
  const size_t cb = align256((size_t)N * Wb * 4), rb = align256((size_t)N * Hb * 4);
  a.col0 = (int*)p; p += cb;
  a.col1 = (int*)p; p += cb;
  a.ax = (float*)p; p += cb;
  a.row0 = (int*)p; p += rb;
  a.row1 = (int*)p; p += rb;
  a.ay = (float*)p;
  hipStream_t s = (hipStream_t)stream;
  const int entries = n_norms * kLut + N * (Wb + Hb);
  hipLaunchKernelGGL(image_tables_kernel, dim3((entries + kT - 1) / kT), dim3(kT), 0, s, a);
  const int quads = N * Hb * (Wb >> 2);
  const dim3 grid((quads + kT * kQuadsPerThread - 1) / (kT * kQuadsPerThread));
  if (n_norms == 2)
    hipLaunchKernelGGL(image_blobs_kernel<2>, grid, dim3(kT), 0, s, a);
  else
    hipLaunchKernelGGL(image_blobs_kernel<1>, grid, dim3(kT), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
