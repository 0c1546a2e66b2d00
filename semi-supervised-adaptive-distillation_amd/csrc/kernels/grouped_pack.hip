// grouped_pack.hip -- both packed copies of every trained grouped 3x3 filter in one launch.
//
// A trained ResNeXt layer needs its filter [C][cg][3][3] (cg = C / group in {4, 8, 16, 32, 64}) twice after every
// update: in the forward kernel's MFMA operand order (grouped_conv3x3.hip, grouped_pack_kernel) and in the data
// gradient's (grouped_conv3x3_grad.hip, grouped_pack_dgrad_kernel: per group transposed, taps flipped).  As per-layer
// launches that is 60 kernels of a few microseconds for an X-101's 30 trained layers, a serial chain at the head of every
// step; here the whole table travels in the kernel arguments (as ssad_transpose_filters and ssad_f16_pack_filters do) and
// a workgroup finds its entry from a prefix table of block counts.
//
// Both orders have the same shape, [group][MT = max(cg / 16, 1)][KS = 9 cg / 4][64 lanes]; element e = ((g MT + t) KS + s)
// 64 + lane, with r = t 16 + (lane & 15), k0 = 4 s, tap = k0 / cg, q = k0 % cg + lane / 16, holds
//   forward        w[g cg + r][q][tap]        (0 for r >= cg)
//   data gradient  w[g cg + q][r][8 - tap]    (0 for r >= cg)
// -- pure copies, so the result is the same bits as the per-layer launchers' for every width.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssad_kernels.h"

namespace {

constexpr int kThreads = 256;

struct GroupedPackTable {
  ssad_grouped_pack_entry e[SSAD_MAX_GROUPED_PACK_ENTRIES];
  int block_start[SSAD_MAX_GROUPED_PACK_ENTRIES + 1];
  int n;
};

// workgroups of an entry: one thread per element of a pack; the size (and the verdict on the widths: < 0) is the
// forward file's own function -- both orders have that many elements
long long entry_blocks(const ssad_grouped_pack_entry& e) {
  const long long n = ssad_grouped_conv3x3_filter_floats(e.C, e.group);
  return n < 0 ? -1 : (n + kThreads - 1) / kThreads;
}

__global__ __launch_bounds__(kThreads) void grouped_pack_multi_kernel(const GroupedPackTable t) {
  int k = 0;
  for (int j = 1; j < t.n; ++j) k += (int)blockIdx.x >= t.block_start[j];
  const ssad_grouped_pack_entry en = t.e[k];
  const int cg = en.C / en.group;
  const int MT = cg > 16 ? cg / 16 : 1, KS = 9 * cg / 4;
  const long long total = (long long)en.group * MT * KS * 64;
  const long long e = (long long)((int)blockIdx.x - t.block_start[k]) * kThreads + threadIdx.x;
  if (e >= total) return;
  const int lane = (int)(e & 63);
  long long r = e >> 6;
  const int s = (int)(r % KS); r /= KS;
  const int tt = (int)(r % MT);
  const int g = (int)(r / MT);
  const int row = tt * 16 + (lane & 15), k0 = 4 * s, tap = k0 / cg, q = (k0 % cg) + (lane >> 4);
  const float* __restrict__ w = en.w;
  const bool live = row < cg;
  if (en.pf) en.pf[e] = live ? w[(((long long)g * cg + row) * cg + q) * 9 + tap] : 0.0f;
  if (en.pd) en.pd[e] = live ? w[(((long long)g * cg + q) * cg + row) * 9 + (8 - tap)] : 0.0f;
}

}  // namespace

extern "C" {

int ssad_grouped_conv3x3_pack_filters(const ssad_grouped_pack_entry* entries, int n_entries, ssad_stream_t stream) {
  if (n_entries <= 0 || !entries) return SSAD_E_BADARG;
  // the whole table is checked before the first chunk is launched: a bad entry leaves every output untouched
  long long chunk_blocks = 0;                      // of the launch the entry belongs to: a grid holds < 2^31
  for (int i = 0; i < n_entries; ++i) {
    const ssad_grouped_pack_entry& e = entries[i];
    const long long nb = entry_blocks(e);
    if (!e.w || (!e.pf && !e.pd) || nb < 0) return SSAD_E_BADARG;
    chunk_blocks = (i % SSAD_MAX_GROUPED_PACK_ENTRIES ? chunk_blocks : 0) + nb;
    if (chunk_blocks >= (1LL << 31)) return SSAD_E_BADARG;
  }
  for (int base = 0; base < n_entries; base += SSAD_MAX_GROUPED_PACK_ENTRIES) {
    const int cnt = n_entries - base < SSAD_MAX_GROUPED_PACK_ENTRIES ? n_entries - base : SSAD_MAX_GROUPED_PACK_ENTRIES;
    GroupedPackTable t;
    long long blocks = 0;
    t.n = cnt;
    for (int i = 0; i < SSAD_MAX_GROUPED_PACK_ENTRIES; ++i) {
      t.e[i] = i < cnt ? entries[base + i] : ssad_grouped_pack_entry{nullptr, nullptr, nullptr, 0, 1};
      t.block_start[i] = (int)blocks;
      if (i < cnt) blocks += entry_blocks(t.e[i]);
    }
    t.block_start[SSAD_MAX_GROUPED_PACK_ENTRIES] = (int)blocks;
    hipLaunchKernelGGL(grouped_pack_multi_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, t);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
