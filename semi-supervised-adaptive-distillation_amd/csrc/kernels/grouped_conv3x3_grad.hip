// grouped_conv3x3_grad.hip -- the two gradients of the grouped 3x3 convolution of grouped_conv3x3.hip (pad 1, stride 1
// or 2, NCHW fp32, cg = C / group in {4, 8, 16, 32, 64}): what a trained ResNeXt body needs of its 33 grouped layers
// (detectron/lib/modeling/ResNet.py:247-258; reference algorithm conv_op_impl.h:451-500,524-560, group by group).
//
// Data gradient   dx[n][g cg + c][iy][ix] = sum_m sum_(ky,kx) w[g cg + m][c][ky][kx] dy[n][g cg + m][oy][ox],
//                 oy s + ky - 1 = iy, ox s + kx - 1 = ix.
//   The filter is packed once into the FORWARD kernel's operand order of the per-group transposed, tap-flipped filter
//   (rows = the group's input channels c, reduction k = tap' * cg + m, tap' = 8 - tap), so at stride 1 the product is
//   the forward product on dy.  One kernel for every width: a workgroup is one 8 x 16 tile of dx for 4 / MT groups, a
//   wave owns ONE 16-row tile of one group's channels and walks all the tile's rows (independent accumulator chains
//   behind one A operand); the reduction channels are staged in LDS in chunks of min(cg, 16) -- the A operands of a
//   chunk (9 * 16 / 4 = 36 registers at most) are fetched per chunk with coalesced loads, so 32- and 64-wide groups
//   need no more registers than 16-wide ones.
//   Stride 2 uses the per-parity tap subsets: dx(2 hy + py, 2 hx + px) reads only the taps whose parity matches --
//   1, 2, 2 and 4 of the nine for (py, px) = (0,0), (0,1), (1,0), (1,1) -- so the nine taps are each multiplied once
//   per 2 x 2 dx pixels, a quarter of the work of the forward product on a zero-upsampled dy, and a non-finite filter
//   tap reaches only the parity class the definition gives it.  A wave holds the four parities of a 4 x 16 patch of
//   the half-resolution grid (16 accumulators); the staged dy tile is (4 + 1) x (16 + 1) per channel.
//   Every dx element is written (with pad 1 every position has a contributing tap; the mask epilogue writes zeros).
//
// Filter gradient dw[g cg + m][c][ky][kx] = sum_n sum_(oy,ox) dy[n][g cg + m][oy][ox] x[n][g cg + c][oy s + ky - 1][..]
//   Per group a [cg x P] . [P x 9cg] product with the pixels as the reduction index: `v_mfma_f32_16x16x4_f32` with
//   A = dy (16 output channels x 4 pixels) and B = the shifted x (4 pixels x 16 (tap, channel) columns), both read
//   from LDS tiles staged like the forward kernel's (dy 8 x 16 pixels, x with its halo).  A wave owns one group (cg
//   <= 16), one (row tile, 16-channel column chunk) pair (cg = 32) or one row tile of a column chunk (cg = 64) and
//   keeps its <= 9 accumulator tiles in registers over a contiguous range of pixel tiles.  No float atomics: the
//   ranges' partial sums go to the workspace and a second launch adds them in range order, so the result is the same
//   bits on every run.  Rows below the map are skipped and columns right of it are multiplied as zero ON THE X SIDE
//   too: a padded output pixel must not carry an x value (a NaN, say) into a tap the definition does not connect.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssad_kernels.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TC = 16;                                  // tile columns (MFMA N)

int group_width(int C, int group) {
  if (C < 1 || group < 1 || C % group) return 0;
  const int cg = C / group;
  return (cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64) ? cg : 0;
}

// ------------------------------------------------------------------------------------------------------------------
// data gradient
// ------------------------------------------------------------------------------------------------------------------
template <int CG>
struct DGeo {
  static constexpr int CK = CG < 16 ? CG : 16, NCK = CG / CK;       // reduction channels per staged chunk, chunks
  static constexpr int MT = CG > 16 ? CG / 16 : 1;                  // 16-row tiles per group
  static constexpr int GPW = 4 / MT;                                // groups per workgroup: a wave per (group, row tile)
  static constexpr int KC = 9 * CK / 4, KS = 9 * CG / 4;            // MFMA steps per chunk / per group
};

struct DArgs {
  const float* dy;
  const float* wp;
  const float* mask;
  float* dx;
  int N, C, H, W, OH, OW, G;
  int tiles_x, tiles_y, gblocks;
};

// packed[g][t][s][lane] = w[g*CG + m][c][8 - tap], c = t*16 + (lane & 15), tap = 4s / CG, m = (4s % CG) + lane / 16
template <int CG>
__global__ __launch_bounds__(256) void grouped_pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ out, int G) {
  constexpr int MT = DGeo<CG>::MT, KS = DGeo<CG>::KS;
  const long long total = (long long)G * MT * KS * 64;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    long long r = e >> 6;
    const int s = (int)(r % KS); r /= KS;
    const int t = (int)(r % MT);
    const int g = (int)(r / MT);
    const int c = t * 16 + (lane & 15), k0 = 4 * s, tap = k0 / CG, m = (k0 % CG) + (lane >> 4);
    out[e] = (c < CG) ? w[(((long long)g * CG + m) * CG + c) * 9 + (8 - tap)] : 0.0f;
  }
}

template <int CG, int S>
__global__ __launch_bounds__(256) void grouped_dgrad_kernel(const DArgs a) {
  typedef DGeo<CG> Q;
  constexpr int CK = Q::CK, NCK = Q::NCK, MT = Q::MT, GPW = Q::GPW, KC = Q::KC, KS = Q::KS;
  constexpr int TR = S == 1 ? 8 : 4;                    // rows of the (stride 2: half-resolution) grid per tile
  constexpr int IR = S == 1 ? TR + 2 : TR + 1, IC = S == 1 ? TC + 2 : TC + 1, CP = IC;     // staged dy tile
  constexpr int PLANE = (IR * CP + 15) / 32 * 32 + 16;  // % 32 == 16: lanes (j, kk) and (j, kk + 1) on distinct banks
  constexpr int NPAR = S * S;
  static_assert(PLANE >= IR * CP && GPW * CK * PLANE * 4 <= 64 * 1024, "static LDS");
  __shared__ float tile[GPW * CK * PLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x; b /= a.tiles_x;
  const int ty = b % a.tiles_y; b /= a.tiles_y;
  const int gb = b % a.gblocks, n = b / a.gblocks;
  const int gi = wave / MT, t = wave % MT, g = gb * GPW + gi;
  const bool active = g < a.G;
  // stride 1: the tile's dx rows ty*TR.. need dy rows from one above; stride 2: half-grid rows hy need dy rows hy, hy + 1
  const int oy0 = ty * TR - (S == 1 ? 1 : 0), ox0 = tx * TC - (S == 1 ? 1 : 0);
  const int ch0 = gb * GPW * CG;
  const float* dyn = a.dy + (long long)n * a.C * a.OH * a.OW;
  const float* wp = a.wp + ((long long)(active ? g : 0) * MT + t) * KS * 64 + lane;
  const float* base = tile + (gi * CK + kk) * PLANE + j;

  f32x4 acc[TR][NPAR];
#pragma unroll
  for (int r = 0; r < TR; ++r)
#pragma unroll
    for (int p = 0; p < NPAR; ++p) acc[r][p] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int q = 0; q < NCK; ++q) {
    if (q) __syncthreads();                            // every wave has read the previous chunk
    for (int e = tid; e < GPW * CK * IR * IC; e += 256) {
      const int sc = e / (IR * IC), r = (e / IC) % IR, p = e % IC;
      const int ch = ch0 + (sc / CK) * CG + q * CK + (sc % CK);
      const int oy = oy0 + r, ox = ox0 + p;
      float v = 0.0f;                                  // zero outside the map / past the last group
      if (ch < a.C && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW) v = dyn[((long long)ch * a.OH + oy) * a.OW + ox];
      tile[sc * PLANE + r * CP + p] = v;
    }
    __syncthreads();
    if (!active) continue;                             // wave-uniform; the barriers above are still reached
    float wr[KC];                                      // the chunk's A operands: packed step tap * CG/4 + q * CK/4 + i
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int i = 0; i < CK / 4; ++i) wr[tap * (CK / 4) + i] = wp[(tap * (CG / 4) + q * (CK / 4) + i) * 64];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;            // of the flipped filter: original tap (2 - ky, 2 - kx)
      // stride 1: dx(iy, ix) reads dy(iy + ky - 1, ix + kx - 1).  stride 2: dx(2hy + py, 2hx + px) takes the original
      // row tap 1 at py = 0 (dy row hy) and 0, 2 at py = 1 (dy rows hy + 1, hy), i.e. flipped ky = 1 | 2, 0.
      const int par = S == 1 ? 0 : (ky != 1) * 2 + (kx != 1);
      const int dr = S == 1 ? ky : (ky == 2), dc = S == 1 ? kx : (kx == 2);
#pragma unroll
      for (int i = 0; i < CK / 4; ++i)
#pragma unroll
        for (int r = 0; r < TR; ++r) {
          const float bv = base[4 * i * PLANE + (r + dr) * CP + dc];
          acc[r][par] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[tap * (CK / 4) + i], bv, acc[r][par], 0, 0, 0);
        }
    }
  }
  if (!active) return;

#pragma unroll
  for (int r = 0; r < TR; ++r)
#pragma unroll
    for (int p = 0; p < NPAR; ++p) {
      const int iy = S == 1 ? ty * TR + r : 2 * (ty * TR + r) + p / 2;
      const int ix = S == 1 ? tx * TC + j : 2 * (tx * TC + j) + p % 2;
      if (iy >= a.H || ix >= a.W) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = t * 16 + kk * 4 + e;             // C/D layout of 16x16x4: row = 4 * (lane / 16) + e
        if (m < CG) {
          const long long o = (((long long)n * a.C + g * CG + m) * a.H + iy) * a.W + ix;
          float v = acc[r][p][e];
          if (a.mask && a.mask[o] <= 0.0f) v = 0.0f;   // ReluGradient of the in-place ReLU below
          a.dx[o] = v;
        }
      }
    }
}

template <int CG>
int launch_dgrad(DArgs a, int stride, hipStream_t s) {
  constexpr int TR1 = 8, TR2 = 4;
  a.tiles_y = (a.OH + (stride == 1 ? TR1 : TR2) - 1) / (stride == 1 ? TR1 : TR2);
  a.tiles_x = (a.OW + TC - 1) / TC;
  a.gblocks = (a.G + DGeo<CG>::GPW - 1) / DGeo<CG>::GPW;
  const long long blocks = (long long)a.N * a.gblocks * a.tiles_y * a.tiles_x;
  if (blocks >= (1LL << 31)) return SSAD_E_BADARG;
  const dim3 grid((unsigned)blocks);
  if (stride == 1) hipLaunchKernelGGL((grouped_dgrad_kernel<CG, 1>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((grouped_dgrad_kernel<CG, 2>), grid, dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

template <int CG>
int pack_dgrad(const float* w, float* out, int G, hipStream_t s) {
  const long long total = (long long)G * DGeo<CG>::MT * DGeo<CG>::KS * 64;
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL((grouped_pack_dgrad_kernel<CG>), dim3(blocks), dim3(256), 0, s, w, out, G);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// filter gradient
// ------------------------------------------------------------------------------------------------------------------
template <int CG>
struct WGeo {
  static constexpr int CC = CG < 16 ? CG : 16;                      // input channels per column chunk
  static constexpr int NQ = 9 * CC, NT = (NQ + 15) / 16;            // (tap, channel) columns of a chunk, 16-column tiles
  static constexpr int NW = CG == 16 ? 2 : 4;                       // waves per workgroup
  static constexpr int GPW = CG <= 8 ? 4 : (CG == 16 ? 2 : 1);      // groups per workgroup
  static constexpr int QB = CG == 64 ? 4 : 1;                       // column chunks that are workgroups of their own
  static constexpr int XCH = CG == 64 ? 16 : GPW * CG, DCH = GPW * CG;   // staged channels of x / of dy
};
constexpr int kWgradTarget = 1024;                                  // workgroups aimed at (4 per CU)

struct WArgs {
  const float* x;
  const float* dy;
  float* ws;
  int N, C, H, W, OH, OW, G;
  int tiles_x, tiles_y, gblocks, split;
  long long tiles, elems;
};

template <int CG, int S>
__global__ __launch_bounds__(WGeo<CG>::NW * 64) void grouped_wgrad_kernel(const WArgs a) {
  typedef WGeo<CG> Q;
  constexpr int CC = Q::CC, NQ = Q::NQ, NT = Q::NT, NW = Q::NW, GPW = Q::GPW, QB = Q::QB, XCH = Q::XCH, DCH = Q::DCH;
  constexpr int TR = S == 1 ? 8 : 4;                                // output rows per pixel tile
  constexpr int IR = (TR - 1) * S + 3, IC = (TC - 1) * S + 3, CP = IC;
  constexpr int XPLANE = (IR * CP) | 1, DPLANE = TR * TC + 2;
  static_assert((XCH * XPLANE + DCH * DPLANE) * 4 <= 64 * 1024, "static LDS");
  __shared__ float xt[XCH * XPLANE];
  __shared__ float dt[DCH * DPLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, k = lane >> 4;
  int b = blockIdx.x;
  const int qb = b % QB; b /= QB;
  const int gb = b % a.gblocks, sp = b / a.gblocks;
  // the wave's group, 16-row tile of output channels and 16-channel column chunk
  const int gi = CG <= 16 ? wave : 0, t = CG == 32 ? (wave & 1) : (CG == 64 ? wave : 0);
  const int q = CG == 32 ? (wave >> 1) : (CG == 64 ? qb : 0);
  const int g = gb * GPW + gi;
  const bool active = g < a.G;
  const int xbase = CG <= 16 ? gi * CG : (CG == 32 ? q * 16 : 0);   // first staged x channel of the wave's columns
  const int dbase = CG <= 16 ? gi * CG : t * 16;                    // first staged dy channel of the wave's rows
  const int xch0 = gb * GPW * CG + (CG == 64 ? qb * 16 : 0), dch0 = gb * GPW * CG;

  const bool avalid = j < CG;                                       // A row = output channel (idle rows at cg < 16)
  const int aoff = (dbase + (avalid ? j : 0)) * DPLANE + k;
  int boff[NT];
  bool bvalid[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int qq = ct * 16 + j, tap = qq / CC, c = qq % CC;         // B column = (tap, input channel)
    bvalid[ct] = qq < NQ;
    boff[ct] = bvalid[ct] ? (xbase + c) * XPLANE + (tap / 3) * CP + (tap % 3) + k * S : 0;
  }
  f32x4 acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long t0 = a.tiles * sp / a.split, t1 = a.tiles * (sp + 1) / a.split;
  const long long HW = (long long)a.H * a.W, OP = (long long)a.OH * a.OW;
#pragma unroll 1
  for (long long tt = t0; tt < t1; ++tt) {
    const int tx = (int)(tt % a.tiles_x);
    const int ty = (int)((tt / a.tiles_x) % a.tiles_y);
    const long long n = tt / ((long long)a.tiles_x * a.tiles_y);
    const int oy0 = ty * TR, ox0 = tx * TC, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    __syncthreads();                                                // every wave has read the previous tile
    const float* xn = a.x + n * a.C * HW;
    for (int e = tid; e < XCH * IR * IC; e += NW * 64) {
      const int c = e / (IR * IC), r = (e / IC) % IR, p = e % IC;
      const int iy = iy0 + r, ix = ix0 + p;
      float v = 0.0f;
      if (xch0 + c < a.C && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = xn[(long long)(xch0 + c) * HW + (long long)iy * a.W + ix];
      xt[c * XPLANE + r * CP + p] = v;
    }
    const float* dn = a.dy + n * a.C * OP;
    for (int e = tid; e < DCH * TR * TC; e += NW * 64) {
      const int c = e / (TR * TC), r = (e / TC) % TR, p = e % TC;
      const int oy = oy0 + r, ox = ox0 + p;
      float v = 0.0f;
      if (dch0 + c < a.C && oy < a.OH && ox < a.OW) v = dn[(long long)(dch0 + c) * OP + (long long)oy * a.OW + ox];
      dt[c * DPLANE + r * TC + p] = v;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
      if (oy0 + r >= a.OH) continue;                                // wave-uniform: rows below the map
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float av = avalid ? dt[aoff + r * TC + ks * 4] : 0.0f;
        const bool pv = ox0 + ks * 4 + k < a.OW;                    // pixels right of the map carry no x
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const float xv = xt[boff[ct] + r * S * CP + ks * 4 * S];
          const float bv = (pv && bvalid[ct]) ? xv : 0.0f;
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[ct], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;

  float* out = a.ws + (long long)sp * a.elems;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int qq = ct * 16 + j, tap = qq / CC, c = q * 16 + qq % CC;
    if (qq >= NQ) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = t * 16 + k * 4 + e;                             // C/D layout of 16x16x4: row = 4 * (lane / 16) + e
      if (m < CG) out[(((long long)g * CG + m) * CG + c) * 9 + tap] = acc[ct][e];
    }
  }
}

// dw[e] = partial 0 + partial 1 + ... in that order
__global__ __launch_bounds__(256) void grouped_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                    long long elems, int split) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < elems; e += (long long)gridDim.x * blockDim.x) {
    float s = ws[e];
    for (int p = 1; p < split; ++p) s += ws[(long long)p * elems + e];
    dw[e] = s;
  }
}

// fills tiles / split / gblocks of the geometry; false when the kernels refuse it
bool wgrad_plan(int N, int C, int H, int W, int group, int stride, WArgs* a) {
  const int cg = group_width(C, group);
  if (!cg || N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return false;
  a->N = N; a->C = C; a->H = H; a->W = W; a->G = group;
  a->OH = (H - 1) / stride + 1; a->OW = (W - 1) / stride + 1;
  const int tr = stride == 1 ? 8 : 4;
  a->tiles_y = (a->OH + tr - 1) / tr; a->tiles_x = (a->OW + TC - 1) / TC;
  a->tiles = (long long)N * a->tiles_y * a->tiles_x;
  const int gpw = cg <= 8 ? 4 : (cg == 16 ? 2 : 1);
  a->gblocks = (group + gpw - 1) / gpw;
  const long long per_range = (long long)a->gblocks * (cg == 64 ? 4 : 1);
  const long long want = kWgradTarget / per_range > 1 ? kWgradTarget / per_range : 1;
  a->split = (int)(a->tiles < want ? a->tiles : want);
  a->elems = (long long)C * cg * 9;
  return per_range * a->split < (1LL << 31);
}

template <int CG>
int launch_wgrad(const WArgs& a, int stride, hipStream_t s) {
  const dim3 grid((unsigned)((long long)a.split * a.gblocks * WGeo<CG>::QB)), block(WGeo<CG>::NW * 64);
  if (stride == 1) hipLaunchKernelGGL((grouped_wgrad_kernel<CG, 1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((grouped_wgrad_kernel<CG, 2>), grid, block, 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

long long ssad_grouped_conv3x3_dgrad_filter_floats(int C, int group) {
  const int cg = group_width(C, group);
  if (!cg) return -1;
  return (long long)group * (cg > 16 ? cg / 16 : 1) * (9 * cg / 4) * 64;
}

int ssad_grouped_conv3x3_pack_filter_dgrad(const float* w, int C, int group, float* packed, ssad_stream_t stream) {
  if (!w || !packed || !group_width(C, group)) return SSAD_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  switch (C / group) {
    case 4: return pack_dgrad<4>(w, packed, group, s);
    case 8: return pack_dgrad<8>(w, packed, group, s);
    case 16: return pack_dgrad<16>(w, packed, group, s);
    case 32: return pack_dgrad<32>(w, packed, group, s);
    default: return pack_dgrad<64>(w, packed, group, s);
  }
}

int ssad_grouped_conv3x3_dgrad(const float* dy, const float* packed, const float* relu_x, int N, int C, int H, int W,
                               int group, int stride, float* dx, ssad_stream_t stream) {
  if (!group_width(C, group) || (stride != 1 && stride != 2) || N < 1 || H < 1 || W < 1) return SSAD_E_BADARG;
  if (!dy || !packed || !dx) return SSAD_E_BADARG;
  DArgs a;
  a.dy = dy; a.wp = packed; a.mask = relu_x; a.dx = dx;
  a.N = N; a.C = C; a.H = H; a.W = W; a.G = group;
  a.OH = (H - 1) / stride + 1; a.OW = (W - 1) / stride + 1;
  a.tiles_x = a.tiles_y = a.gblocks = 0;
  hipStream_t s = (hipStream_t)stream;
  switch (C / group) {
    case 4: return launch_dgrad<4>(a, stride, s);
    case 8: return launch_dgrad<8>(a, stride, s);
    case 16: return launch_dgrad<16>(a, stride, s);
    case 32: return launch_dgrad<32>(a, stride, s);
    default: return launch_dgrad<64>(a, stride, s);
  }
}

size_t ssad_grouped_conv3x3_wgrad_workspace_bytes(int N, int C, int H, int W, int group, int stride) {
  WArgs a;
  if (!wgrad_plan(N, C, H, W, group, stride, &a)) return 0;
  return (size_t)a.split * (size_t)a.elems * sizeof(float);
}

int ssad_grouped_conv3x3_wgrad(const float* x, const float* dy, int N, int C, int H, int W, int group, int stride,
                               float* dw, void* workspace, size_t workspace_bytes, ssad_stream_t stream) {
  WArgs a;
  if (!wgrad_plan(N, C, H, W, group, stride, &a)) return SSAD_E_BADARG;
  if (!x || !dy || !dw || !workspace) return SSAD_E_BADARG;
  if (workspace_bytes < (size_t)a.split * (size_t)a.elems * sizeof(float)) return SSAD_E_BADARG;
  a.x = x; a.dy = dy; a.ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  switch (C / group) {
    case 4: rc = launch_wgrad<4>(a, stride, s); break;
    case 8: rc = launch_wgrad<8>(a, stride, s); break;
    case 16: rc = launch_wgrad<16>(a, stride, s); break;
    case 32: rc = launch_wgrad<32>(a, stride, s); break;
    default: rc = launch_wgrad<64>(a, stride, s); break;
  }
  if (rc) return rc;
  const int blocks = (int)((a.elems + 255) / 256 < 2048 ? (a.elems + 255) / 256 : 2048);
  hipLaunchKernelGGL(grouped_wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)a.ws, dw, a.elems, a.split);
  return (int)hipGetLastError();
}

}  // extern "C"
