// wino_launch.h -- the host side the two Winograd engines share (conv3x3_winograd.hip: F(2x2), conv3x3_winograd24.hip:
// F(2x4)): the level and work-item records their kernels read, the staging geometry rule, the plan of one pass over a
// level table and the F(2x2) engine's split-tail decision.  Host code and plain data only: every kernel, and every
// constant only a kernel reads, stays in its .hip file.  Internal, not exported.
#ifndef SSAD_WINO_LAUNCH_H_
#define SSAD_WINO_LAUNCH_H_

#include <stdlib.h>

#include "conv_internal.h"
#include "ssad_kernels.h"

namespace ssad_wino {

constexpr int PR = 8, PC = 16;     // output patch rows / cols
constexpr int SP = 8;              // sub-patch edge (output pixels)
constexpr int BM = 128;            // output channels per workgroup
constexpr int KC = 16;             // input channels per chunk
constexpr int ZNT = 256;           // work items per workgroup in the LDS list
constexpr int kBlock = 512;
constexpr int kNoSub = 1 << 24;    // WTile::y0 of an absent partner
constexpr unsigned kOOBOff = 0x80000000u;

struct WLevel {
  const float* x;
  float* y;
  const float* aux;                // SSAD_CONV_MASK_AUX: the forward output whose sign masks y (fused ReluGradient)
  const float* packed;
  const float* bias;
  int N, H, W;
  int tiles_x, tiles_y;            // 8 x 16 patches per row / column of one image
  int block_start;                 // first patch of this level
  int sub_x, sub_y;                // 8 x 8 sub-patches per row / column of one image, two per work item
  int pair_start;                  // first pair of this level
};

// One work item: two 8 x 8-pixel sub-patches of one level, each with its own image and origin; y0 = kNoSub marks an
// absent partner.
struct WTile {
  int l, mb;
  int n[2], y0[2], x0[2];
};

constexpr long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// Staging geometry per level: 8 x 16 patches where they tile the map exactly or the 8 x 8 sub-patches would not save
// pixels (a patch stages 18 columns where two sub-patches stage 20: ~4 % faster per computed pixel), sub-patch pairs
// where they save at least 4 % of them.  SSAD_WINO_PAIRS=0 / 1 forces one geometry for every level (read once).
inline bool level_wants_pairs(int H, int W) {
  static const int geom = [] { const char* e = getenv("SSAD_WINO_PAIRS"); return (e && *e) ? atoi(e) : -1; }();
  if (geom >= 0) return geom != 0;
  const long long by_patch = ceil_div(W, PC) * ceil_div(H, PR) * 128;
  const long long by_sub = ceil_div(W, SP) * ceil_div(H, SP) * 64;
  return by_sub * 100 <= by_patch * 96;
}

// What both launchers refuse before anything is launched.  (The F(2x4) launcher refuses some flag combinations on top;
// those lines are its own.)
inline int check_levels(const ssad_conv_level* lv, int n_levels, const float* packed, int Cout, int Cin, int flags) {
  if (n_levels < 1 || n_levels > SSAD_MAX_CONV_PROBLEMS || Cout <= 0 || Cin <= 0) return SSAD_E_BADARG;
  for (int l = 0; l < n_levels; ++l) {
    if (!(lv[l].packed ? lv[l].packed : packed)) return SSAD_E_BADARG;
    if (lv[l].N < 0 || lv[l].H < 0 || lv[l].W < 0) return SSAD_E_BADARG;
    if ((long long)lv[l].N * lv[l].H * lv[l].W * (Cin > Cout ? Cin : Cout) >= (1LL << 29)) return SSAD_E_BADARG;
    if ((flags & SSAD_CONV_MASK_AUX) && !lv[l].aux) return SSAD_E_BADARG;
  }
  return 0;
}

// One pass over a level table: the non-empty levels staged as sub-patch pairs (use_pairs) or as 8 x 16 patches.
struct Pass {
  int rc;                  // SSAD_E_BADARG: a count does not fit 31 bits
  int nl;                  // levels of this pass (0: nothing to launch)
  long long blocks, pairs; // 8 x 16 patches / sub-patch pairs of those levels
  long long total;         // work items: (pairs or blocks) x mblocks
  long long grid;          // persistent workgroups: one per CU, more only where a list of ZNT items would overflow
};

// `out` (SSAD_MAX_CONV_PROBLEMS records, or nullptr for a count that launches nothing): the pass's levels first, in table
// order, the rest zeroed.  A level's own filter comes with its own bias; the others take `packed` and `bias`.
inline Pass plan_pass(const ssad_conv_level* lv, int n_levels, const float* packed, const float* bias, bool use_pairs,
                      int mblocks, int cus, WLevel* out) {
  Pass p{0, 0, 0, 0, 0, 0};
  for (int l = 0; l < n_levels; ++l) {
    if ((long long)lv[l].N * lv[l].H * lv[l].W == 0) continue;
    if (level_wants_pairs(lv[l].H, lv[l].W) != use_pairs) continue;
    WLevel L{};
    L.x = lv[l].x; L.y = lv[l].y; L.aux = lv[l].aux;
    L.packed = lv[l].packed ? lv[l].packed : packed;
    L.bias = lv[l].packed ? lv[l].bias : bias;
    L.N = lv[l].N; L.H = lv[l].H; L.W = lv[l].W;
    L.tiles_x = (int)ceil_div(L.W, PC); L.tiles_y = (int)ceil_div(L.H, PR);
    L.block_start = (int)p.blocks;
    p.blocks += (long long)L.N * L.tiles_x * L.tiles_y;
    L.sub_x = (int)ceil_div(L.W, SP); L.sub_y = (int)ceil_div(L.H, SP);
    L.pair_start = (int)p.pairs;
    p.pairs += ((long long)L.N * L.sub_x * L.sub_y + 1) / 2;
    if (out) out[p.nl] = L;
    ++p.nl;
    if (p.blocks >= (1LL << 31)) { p.rc = SSAD_E_BADARG; return p; }
  }
  if (out)
    for (int l = p.nl; l < SSAD_MAX_CONV_PROBLEMS; ++l) out[l] = WLevel{};
  p.total = (use_pairs ? p.pairs : p.blocks) * mblocks;
  if (p.total >= (1LL << 31)) { p.rc = SSAD_E_BADARG; return p; }
  p.grid = p.total < cus ? p.total : cus;
  if (p.grid * ZNT < p.total) p.grid = ceil_div(p.total, ZNT);
  return p;
}

// ---- the F(2x2) engine's split tail (wino_conv_z_kernel's header) -------------------------------------------------
// Units per tail item (1 = no split): the largest power of two p with  p <= 8,  tail * p <= grid,  p | chunks  and
// chunks / p >= 2.  *full = items of the whole rounds, *tail = items of the partial round.
inline int split_plan(long long total, int chunks, int cus, long long* full, long long* tail) {
  *full = (total / cus) * cus;
  *tail = total - *full;
  int p = 1;
  while (*tail > 0 && p * 2 <= 8 && *tail * (p * 2) <= cus && chunks % (p * 2) == 0 && chunks / (p * 2) >= 2) p *= 2;
  return p;
}

struct Tail {
  int parts;               // units per item of the partial round; 0: the launch is not split
  long long full, tail;    // items of the whole rounds (the main launch, none if 0) / of the partial round
};

// The items of the last, partial round are cut along the reduction into `parts` units each and run as a launch of
// their own, `tail * parts` workgroups, behind the full rounds.  Taken when the partial round is at most half full
// (parts >= 2), never for the half-block kernels, never where the grid is longer than one workgroup per CU.
// setting (ssad_conv_wino_split_tail) 0: never; 1: only launches WITHOUT a full round -- there the units replace the
// launch, no second kernel; 2, or 1 with SSAD_CONV_SPLIT_TAIL in `flags`: also the partial round behind full rounds.
// What this cannot know is whether the launcher gets its scratch: if that allocation fails the launcher runs the
// unsplit launch instead, and a launch count made from this decision is one too high for a tail behind full rounds.
inline Tail plan_split_tail(long long total, int chunks, int cus, int setting, int flags, bool half) {
  if (setting && (flags & SSAD_CONV_SPLIT_TAIL)) setting = 2;
  const Tail unsplit{0, total, 0};
  if (!setting || half || total > (long long)cus * ZNT) return unsplit;
  long long full = 0, tail = 0;
  const int p = split_plan(total, chunks, cus, &full, &tail);
  if (p < 2 || (setting < 2 && full > 0)) return unsplit;
  return Tail{p, full, tail};
}

}  // namespace ssad_wino

#endif  // SSAD_WINO_LAUNCH_H_
