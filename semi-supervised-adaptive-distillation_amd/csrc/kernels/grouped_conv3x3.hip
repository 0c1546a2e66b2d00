// grouped_conv3x3.hip -- grouped 3x3 convolution (pad 1, stride 1 or 2), NCHW fp32, forward:
// ResNeXt's cardinality-64 bottleneck layer (detectron/lib/modeling/ResNet.py:247-258 with
// RESNETS.NUM_GROUPS = 64, WIDTH_PER_GROUP = 4, STRIDE_1X1 = False, i.e. BASELINE config 5's
// X-101-64x4d teacher; reference algorithm caffe2/operators/conv_op_impl.h:93-98,126-173: the groups
// are independent convolutions over contiguous channel blocks).
//
//   y[n][g*cg + m][oy][ox] = act( bias + sum_{c < cg} sum_{ky,kx} w[g*cg + m][c][ky][kx]
//                                                       * x[n][g*cg + c][oy*s + ky - 1][ox*s + kx - 1] )
//
// cg = channels per group = 4, 8, 16, 32 at res2..res5.  Design for gfx950: per group the layer is a
// [cg x 9cg] . [9cg x pixels] product -- M = 16 of `v_mfma_f32_16x16x4_f32` is exactly a res4 group (23
// of the 33 layers).  A wave owns one group and rows of 16 output pixels:
//  * the filter is packed once (ssad_grouped_conv3x3_pack_filter; the teacher is frozen) into MFMA
//    operand order [group][row tile][step][lane], so a wave fetches its 9cg/4 A operands with
//    coalesced loads and keeps them in REGISTERS for all its rows.  Reduction order k = tap * cg + c:
//    four consecutive k share their tap, so in the fully unrolled loop the tap is a compile-time
//    constant and the channel is (constant + lane / 16);
//  * the input tile of the workgroup's channels ((rows*s + 2) x (16*s + 2) per channel, zero outside
//    the image) is staged once in LDS; a B operand is then ONE ds_read_b32 with an immediate offset
//    ((c0 * plane + ky * pitch + kx) * 4) on a per-lane base -- no address arithmetic in the loop;
//  * bias and ReLU in registers.  One workgroup = 4 waves = 8 output rows x 16 columns of GPW
//    neighbouring groups (4 at cg = 4, 2 at cg = 8, else 1): narrow groups would otherwise give a
//    workgroup too little to do (measured 0.77 -> see DESIGN.md 3.6 for res2's layer).
// Groups narrower than 16 channels leave MFMA rows idle (res2: cg = 4, res3: cg = 8 -- seven small
// layers); cg = 32 uses two row tiles.  cg = 64 (X-101-32x8d's res5) has a kernel of its own, further down.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssad_kernels.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kThreads = 256;
constexpr int TR = 8, TC = 16;             // output tile: rows x columns

struct GArgs {
  const float* x;
  const float* wp;          // packed filter
  const float* bias;
  float* y;
  int N, C, H, W, OH, OW, G, relu;
  int tiles_x, tiles_y, gblocks;
};

template <int CG>
struct Geo {
  static constexpr int MT = CG > 16 ? CG / 16 : 1;          // 16-row MFMA tiles per group
  static constexpr int KS = 9 * CG / 4;                     // MFMA steps (K = 9 cg, 4 per step)
  static constexpr int GPW = CG == 4 ? 4 : (CG == 8 ? 2 : 1);   // groups per workgroup
};

// packed[g][t][s][lane] = w[g*CG + t*16 + (lane & 15)][(4s % CG) + lane / 16][tap = 4s / CG] (0 past CG rows)
template <int CG>
__global__ __launch_bounds__(256) void grouped_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int G) {
  constexpr int MT = Geo<CG>::MT, KS = Geo<CG>::KS;
  const long long total = (long long)G * MT * KS * 64;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    long long r = e >> 6;
    const int s = (int)(r % KS); r /= KS;
    const int t = (int)(r % MT);
    const int g = (int)(r / MT);
    const int m = t * 16 + (lane & 15), k0 = 4 * s, tap = k0 / CG, c = (k0 % CG) + (lane >> 4);
    out[e] = (m < CG) ? w[(((long long)g * CG + m) * CG + c) * 9 + tap] : 0.0f;
  }
}

template <int CG, int S>
__global__ __launch_bounds__(kThreads) void grouped_conv3x3_kernel(const GArgs a) {
  constexpr int MT = Geo<CG>::MT, KS = Geo<CG>::KS, GPW = Geo<CG>::GPW;
  constexpr int CH = CG * GPW;                       // channels staged per workgroup
  constexpr int IR = (TR - 1) * S + 3, IC = (TC - 1) * S + 3;     // input tile rows / columns
  constexpr int CP = IC + 1;                         // row pitch
  constexpr int PLANE = IR * CP;
  constexpr int ROWS = TR * GPW / 4;                 // output rows per wave
  __shared__ float tile[CH * PLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x; b /= a.tiles_x;
  const int ty = b % a.tiles_y; b /= a.tiles_y;
  const int gb = b % a.gblocks, n = b / a.gblocks;
  const int gi = wave % GPW, g = gb * GPW + gi;
  const int oy0 = ty * TR, ox0 = tx * TC;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

  // ---- the wave's filter: 9cg/4 (x MT) coalesced loads, kept in registers ----
  float wr[MT][KS];
  {
    const float* wp = a.wp + (long long)(g < a.G ? g : 0) * MT * KS * 64 + lane;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int s = 0; s < KS; ++s) wr[t][s] = wp[(t * KS + s) * 64];
  }

  // ---- stage the workgroup's input channels (zero outside the image / past the last group) ----
  const int ch0 = gb * CH;
  const float* xg = a.x + ((long long)n * a.C + ch0) * a.H * a.W;
  for (int e = tid; e < CH * IR * IC; e += kThreads) {
    const int c = e / (IR * IC), r = (e / IC) % IR, q = e % IC;
    const int iy = iy0 + r, ix = ix0 + q;
    float v = 0.0f;
    if (ch0 + c < a.C && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = xg[((long long)c * a.H + iy) * a.W + ix];
    tile[c * PLANE + r * CP + q] = v;
  }
  __syncthreads();
  if (g >= a.G) return;

  // ---- rows of 16 output pixels ----
#pragma unroll 1
  for (int rr = 0; rr < ROWS; ++rr) {
    const int r = wave / GPW + (4 / GPW) * rr;
    const float* base = tile + (gi * CG + kk) * PLANE + (r * S) * CP + j * S;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k0 = 4 * s, tap = k0 / CG, c0 = k0 % CG;
      const float bv = base[c0 * PLANE + (tap / 3) * CP + (tap % 3)];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[t][s], bv, acc[t], 0, 0, 0);
    }
    const int oy = oy0 + r, ox = ox0 + j;
    if (oy < a.OH && ox < a.OW) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = t * 16 + kk * 4 + q;          // C/D layout of 16x16x4: row = 4 * (lane / 16) + q
          if (m < CG) {
            const int ch = g * CG + m;
            float v = acc[t][q] + (a.bias ? a.bias[ch] : 0.0f);
            if (a.relu) v = fmaxf(v, 0.0f);
            a.y[(((long long)n * a.C + ch) * a.OH + oy) * a.OW + ox] = v;
          }
        }
    }
  }
}

template <int CG>
int launch(GArgs a, int stride, hipStream_t s) {
  a.gblocks = (a.G + Geo<CG>::GPW - 1) / Geo<CG>::GPW;
  const long long blocks = (long long)a.N * a.gblocks * a.tiles_y * a.tiles_x;
  if (blocks >= (1LL << 31)) return SSAD_E_BADARG;
  const dim3 grid((unsigned)blocks);
  if (stride == 1) hipLaunchKernelGGL((grouped_conv3x3_kernel<CG, 1>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((grouped_conv3x3_kernel<CG, 2>), grid, dim3(kThreads), 0, s, a);
  return (int)hipGetLastError();
}

// ---- groups of 64 channels (ResNeXt-101-32x8d's res5: 2048 channels in 32 groups) ----
// The design above does not stretch to cg = 64: MT * 9cg/4 = 576 filter registers per wave, and a stride-2 halo
// of all 64 channels is 148 KB.  Here one workgroup is one group's 8 x 16 output tile and each of the four waves
// owns ONE 16-row tile of the group's 64 output channels and walks all eight pixel rows:
//  * the input is staged in chunks of 16 channels at stride 1 (13 KB) and of 8 at stride 2 (8 x 17 x 33 floats =
//    18 KB) and the reduction runs chunk-major, k = (chunk, tap, channel in chunk); the eight rows' accumulators
//    (32 registers) live across the chunks.  The sum order therefore differs from the narrower widths' (fp32
//    round-off only);
//  * the chunk loop is software-pipelined through registers: a thread stages the same one (stride 1) or three
//    (stride 2) halo positions of every channel of a chunk, fetches the NEXT chunk's floats and its A operands
//    (coalesced, from the same packed order as above, s = tap * 16 + c / 4) before the current chunk's MFMAs and
//    writes them to the one LDS buffer after them.  Eight channels at stride 2 because 3 x 16 staged floats, their
//    addresses and two sets of 36 A operands do not fit 256 registers at two workgroups per CU;
//  * two pixel rows share each A operand: two independent accumulator chains, so the 40-cycle dependent latency
//    of 16x16x4 never stalls its 32-cycle issue (a single chain, as in the cg <= 16 path, loses a fifth);
//  * ds_read_b32 banks are (address / 4) % 32 within a 32-lane half, i.e. lanes (j, kk) and (j, kk + 1): at
//    stride 1 the 16 columns take 16 consecutive banks, so PLANE % 32 == 16 puts kk + 1 on the other 16; at
//    stride 2 they take the even banks, so an odd PLANE puts kk + 1 on the odd ones.  Both are conflict-free.
template <int S>
struct Geo64 {
  static constexpr int CK = S == 1 ? 16 : 8, NCK = 64 / CK, KC = 9 * CK / 4;      // chunk channels, chunks, steps per chunk
  static constexpr int IR = (TR - 1) * S + 3, IC = (TC - 1) * S + 3, CP = IC;
  static constexpr int PLANE = S == 1 ? (IR * CP + 15) / 32 * 32 + 16 : ((IR * CP) | 1);
  static_assert(PLANE >= IR * CP && PLANE % 32 != 0, "plane pitch");
  static_assert(CK * PLANE * 4 <= 64 * 1024, "static LDS");
};

template <int S>
__global__ __launch_bounds__(kThreads, 2) void grouped_conv3x3_cg64_kernel(const GArgs a) {
  typedef Geo64<S> Q;
  constexpr int CG = 64, CK = Q::CK, KC = Q::KC, IR = Q::IR, IC = Q::IC, CP = Q::CP, PLANE = Q::PLANE;
  __shared__ float tile[CK * PLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;      // wave = the group's 16-row tile
  const int j = lane & 15, kk = lane >> 4;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x; b /= a.tiles_x;
  const int ty = b % a.tiles_y; b /= a.tiles_y;
  const int g = b % a.G, n = b / a.G;
  const int oy0 = ty * TR, ox0 = tx * TC;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

  const float* wp = a.wp + ((long long)g * 4 + wave) * (9 * CG / 4) * 64 + lane;
  const float* xg = a.x + ((long long)n * a.C + (long long)g * CG) * a.H * a.W;
  const float* base = tile + kk * PLANE + j * S;

  f32x4 acc[TR / 2][2];
#pragma unroll
  for (int rp = 0; rp < TR / 2; ++rp) acc[rp][0] = acc[rp][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Software pipeline over the chunks: the next chunk's input (SLOTS x CK floats per thread) and A operands are
  // fetched into registers BEFORE the current chunk's MFMAs and written to the one LDS buffer after them, so their
  // latency hides behind the arithmetic of the same workgroup.
  // A thread stages the same SLOTS halo positions of every channel of a chunk: their addresses and bounds are
  // worked out once, a channel is a uniform step of H * W, and the LDS offset of (channel, position) is immediate.
  constexpr int NPOS = IR * IC, SLOTS = (NPOS + kThreads - 1) / kThreads;
  float pre[SLOTS][CK], wr[KC];
  long long goff[SLOTS];
  int loff[SLOTS];
  bool inside[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int pos = tid + k * kThreads, r = pos / IC, p = pos % IC;
    const int iy = iy0 + r, ix = ix0 + p;
    inside[k] = pos < NPOS && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    goff[k] = (long long)iy * a.W + ix;
    loff[k] = pos < NPOS ? r * CP + p : -1;
  }
  const long long HW = (long long)a.H * a.W;
  auto fetch = [&](int q) {
    const float* xq = xg + (long long)q * CK * HW;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
#pragma unroll
      for (int c = 0; c < CK; ++c) pre[k][c] = inside[k] ? xq[c * HW + goff[k]] : 0.0f;    // zero outside the image
  };
  // the chunk's A operands: step (tap, i) is packed step tap * 16 + q * CK / 4 + i
  auto fetch_w = [&](float* dst, int q) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int i = 0; i < CK / 4; ++i) dst[tap * (CK / 4) + i] = wp[(tap * 16 + q * (CK / 4) + i) * 64];
  };
  fetch_w(wr, 0);
  fetch(0);

#pragma unroll 1
  for (int q = 0; q < Q::NCK; ++q) {
    // ---- channels q * CK .. of the group: registers -> LDS ----
    if (q) __syncthreads();                        // every wave has read the previous chunk
#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
      if (loff[k] >= 0) {
#pragma unroll
        for (int c = 0; c < CK; ++c) tile[c * PLANE + loff[k]] = pre[k][c];
      }
    __syncthreads();
    float wn[KC];
    if (q + 1 < Q::NCK) {                          // uniform
      fetch(q + 1);
      fetch_w(wn, q + 1);
    } else {
#pragma unroll
      for (int k = 0; k < KC; ++k) wn[k] = wr[k];
    }

    // ---- pairs of pixel rows: one A operand, two accumulator chains ----
#pragma unroll
    for (int rp = 0; rp < TR / 2; ++rp) {
      if (oy0 + 2 * rp >= a.OH) continue;          // wave-uniform: rows below the map
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int i = 0; i < CK / 4; ++i) {
          const int off = 4 * i * PLANE + (tap / 3) * CP + (tap % 3);
          const float b0 = base[off + (2 * rp * S) * CP];
          const float b1 = base[off + ((2 * rp + 1) * S) * CP];
          acc[rp][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[tap * (CK / 4) + i], b0, acc[rp][0], 0, 0, 0);
          acc[rp][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[tap * (CK / 4) + i], b1, acc[rp][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) wr[k] = wn[k];
  }

  const int ox = ox0 + j;
  if (ox >= a.OW) return;
#pragma unroll
  for (int rp = 0; rp < TR / 2; ++rp)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int oy = oy0 + 2 * rp + h;
      if (oy >= a.OH) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = g * CG + wave * 16 + kk * 4 + e;     // C/D layout of 16x16x4: row = 4 * (lane / 16) + e
        float v = acc[rp][h][e] + (a.bias ? a.bias[ch] : 0.0f);
        if (a.relu) v = fmaxf(v, 0.0f);
        a.y[(((long long)n * a.C + ch) * a.OH + oy) * a.OW + ox] = v;
      }
    }
}

int launch64(GArgs a, int stride, hipStream_t s) {
  a.gblocks = a.G;
  const long long blocks = (long long)a.N * a.G * a.tiles_y * a.tiles_x;
  if (blocks >= (1LL << 31)) return SSAD_E_BADARG;
  const dim3 grid((unsigned)blocks);
  if (stride == 1) hipLaunchKernelGGL((grouped_conv3x3_cg64_kernel<1>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((grouped_conv3x3_cg64_kernel<2>), grid, dim3(kThreads), 0, s, a);
  return (int)hipGetLastError();
}

template <int CG>
int pack(const float* w, float* out, int G, hipStream_t s) {
  const long long total = (long long)G * Geo<CG>::MT * Geo<CG>::KS * 64;
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL((grouped_pack_kernel<CG>), dim3(blocks), dim3(256), 0, s, w, out, G);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

long long ssad_grouped_conv3x3_filter_floats(int C, int group) {
  if (C < 1 || group < 1 || C % group) return -1;
  const int cg = C / group;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return -1;
  return (long long)group * (cg > 16 ? cg / 16 : 1) * (9 * cg / 4) * 64;
}

int ssad_grouped_conv3x3_pack_filter(const float* w, int C, int group, float* packed, ssad_stream_t stream) {
  if (!w || !packed || ssad_grouped_conv3x3_filter_floats(C, group) < 0) return SSAD_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  switch (C / group) {
    case 4: return pack<4>(w, packed, group, s);
    case 8: return pack<8>(w, packed, group, s);
    case 16: return pack<16>(w, packed, group, s);
    case 32: return pack<32>(w, packed, group, s);
    default: return pack<64>(w, packed, group, s);
  }
}

int ssad_grouped_conv3x3_forward(const float* x, const float* packed, const float* bias, int N, int C, int H,
                                 int W, int group, int stride, int relu, float* y, ssad_stream_t stream) {
  if (!x || !packed || !y || N < 0 || H < 1 || W < 1) return SSAD_E_BADARG;
  if (ssad_grouped_conv3x3_filter_floats(C, group) < 0) return SSAD_E_BADARG;   // widths other than 4/8/16/32/64
  if (stride != 1 && stride != 2) return SSAD_E_BADARG;
  GArgs a;
  a.x = x; a.wp = packed; a.bias = bias; a.y = y;
  a.N = N; a.C = C; a.H = H; a.W = W; a.G = group; a.relu = relu;
  a.OH = (H - 1) / stride + 1; a.OW = (W - 1) / stride + 1;      // pad 1, kernel 3
  a.tiles_y = (a.OH + TR - 1) / TR; a.tiles_x = (a.OW + TC - 1) / TC;
  a.gblocks = 0;
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  switch (C / group) {
    case 4: return launch<4>(a, stride, s);
    case 8: return launch<8>(a, stride, s);
    case 16: return launch<16>(a, stride, s);
    case 32: return launch<32>(a, stride, s);
    default: return launch64(a, stride, s);
  }
}

}  // extern "C"
