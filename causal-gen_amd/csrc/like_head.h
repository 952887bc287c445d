// What the fused likelihood head (dgauss_head_*_kernel, csrc/likelihood.hip) shares with the units whose launches it replaces:
// the split geometry of the generic weight-gradient kernel (wgrad_kernel, csrc/wgrad.hip) -- it writes the same split-K
// partials, so it walks the same splits -- and the question which kernel cgen_conv2d picks for a head conv (csrc/conv.hip).
#pragma once
#include "common.h"

namespace cgen {

// Does cgen_conv2d serve this f16 call with conv_tile_kernel<h16, 1, 1> in ONE K-step (a 1x1 conv of at most 32 input channels
// whose output the 16-byte epilogues of conv_px / conv_ws cannot write)?  That is the arithmetic the fused head repeats: one
// v_mfma_f32_16x16x32 from zero, the bias added in f32, one rounding.
bool conv_is_tile_1x1_onestep(const cgen_conv_args* a);

#define WG_PK 64   // pixels per K-step of a workgroup
#define WG_MAXT 9  // taps per workgroup

static inline int wgrad_ntc(int co) { return co <= 16 ? 1 : (co <= 32 ? 2 : 4); }

static inline void wgrad_geometry(int P, int co, int ci_chunks, int ks, int& nsplit, int& pps) {
  const int ntc = wgrad_ntc(co);
  const int tiles = ci_chunks * ceil_div(co, ntc * 16) * ceil_div(ks * ks, WG_MAXT);
  int want = ceil_div(2048, tiles);
  int maxs = ceil_div(P, 4 * WG_PK);
  nsplit = want < 1 ? 1 : (want > maxs ? maxs : want);
  if (nsplit < 1) nsplit = 1;
  pps = (ceil_div(P, nsplit) + WG_PK - 1) / WG_PK * WG_PK;
  nsplit = ceil_div(P, pps);
}

}  // namespace cgen
