// The split-K reduce in its tiled form (the per-element original, wred_kernel of csrc/conv.hip, stays behind cgen_wgrad_reduce_ref as
// the executable definition of the sum order):
//   wred_kernel_tiled   split-K partials -> flat OIHW gradient.  A workgroup owns a TILE of a site (a block of partial rows), sums it --
//                      deep sites with the four split chains dealt to different lanes --, and writes the OIHW gradient from LDS in runs.
#include "common.h"

namespace cgen {

#define WRED_T 2048       // elements of a tile that needs one LDS word per sum (at most four splits, or the plain split order)
#define WRED_T_DEEP 1024  // elements of a tile that keeps its four chain sums in LDS (more than four splits)

template <int VW>
__device__ __forceinline__ void wred_load(const float* q, float* t) {
  if (VW == 4) { const f32x4_t v = __builtin_nontemporal_load((const f32x4_t*)q); t[0] = v[0]; t[1 % VW] = v[1]; t[2 % VW] = v[2]; t[3 % VW] = v[3]; }
  else t[0] = __builtin_nontemporal_load(q);
}

// One split chain of VW consecutive partial elements: splits c, c + step, ... < nsplit added in that order to 0.f -- the order
// wred_kernel adds them to b[c] (its batches of sixteen and four only put loads in flight; the additions are in split order).
template <int VW>
__device__ __forceinline__ void wred_chain(const float* p, size_t stride, int c, int step, int nsplit, float* out) {
  float acc[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) acc[e] = 0.f;
  int sp = c;
  for (; sp + 7 * step < nsplit; sp += 8 * step) {  // eight loads in flight
    float t[8][VW];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wred_load<VW>(p + (size_t)(sp + j * step) * stride, t[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[e] += t[j][e];
  }
  for (; sp < nsplit; sp += step) {
    float v[VW];
    wred_load<VW>(p + (size_t)sp * stride, v);
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < VW; ++e) out[e] = acc[e];
}

// tile element l = (row, col): row = (a - a0) * taps + t, col = b - b0; its partial sits at ((a0 * taps + row) * inner + b0 + col)
template <int VW>
__device__ __forceinline__ void wred_tile_sums(const cgen_wred_item& it, float* sm, int n, bool deep) {
  const int ngroups = n / VW;
  const size_t stride = (size_t)it.split_stride;
  const float* base = it.partial + ((size_t)it.a0 * it.taps * it.inner + it.b0);
  if (it.nsplit <= 4) {  // a thread holds all of a group's splits: two groups, up to eight loads, in flight
    for (int u0 = threadIdx.x; u0 < ngroups; u0 += 2 * 256) {
      float t[2][4][VW];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int l = (u0 + 256 * j) * VW;
        if (l < n) {
          const int row = (int)((unsigned)l / (unsigned)it.nb), col = l - row * it.nb;
          const float* q = base + (size_t)row * it.inner + col;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < it.nsplit) wred_load<VW>(q + (size_t)c * stride, t[j][c]);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int l = (u0 + 256 * j) * VW;
        if (l < n) {
#pragma unroll
          for (int e = 0; e < VW; ++e) {
            float r;
            if (it.vec) {  // chains c = split: b[c] = 0 + split c, then (b0 + b1) + (b2 + b3)
              float b[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) { b[c] = 0.f; if (c < it.nsplit) b[c] += t[j][c][e]; }
              r = (b[0] + b[1]) + (b[2] + b[3]);
            } else {
              r = 0.f;
#pragma unroll
              for (int c = 0; c < 4; ++c) if (c < it.nsplit) r += t[j][c][e];
            }
            sm[l + e] = r;
          }
        }
      }
    }
    return;
  }
  if (!deep) {  // plain split order: one chain per group
    for (int u = threadIdx.x; u < ngroups; u += 256) {
      const int l = u * VW, row = (int)((unsigned)l / (unsigned)it.nb), col = l - row * it.nb;
      float a[VW];
      wred_chain<VW>(base + (size_t)row * it.inner + col, stride, 0, 1, it.nsplit, a);
#pragma unroll
      for (int e = 0; e < VW; ++e) sm[l + e] = a[e];
    }
    return;
  }
  // the four chains of a group go to different lanes (chain-major: a wave load is 1 KB of one split) and meet in LDS
  const int units = 4 * ngroups;
  for (int u = threadIdx.x; u < units; u += 256) {
    const int c = (int)((unsigned)u / (unsigned)ngroups), l = (u - c * ngroups) * VW;
    const int row = (int)((unsigned)l / (unsigned)it.nb), col = l - row * it.nb;
    float a[VW];
    wred_chain<VW>(base + (size_t)row * it.inner + col, stride, c, 4, it.nsplit, a);
#pragma unroll
    for (int e = 0; e < VW; ++e) sm[c * n + l + e] = a[e];
  }
}

__global__ __launch_bounds__(256) void wred_kernel_tiled(const cgen_wred_item* items) {
  __shared__ float sm[4 * WRED_T_DEEP];
  const cgen_wred_item it = items[blockIdx.x];
  const float us = it.unscale == 0.f ? 1.f : it.unscale;
  if (it.kind == 1) {  // bias gradient of channels b0 .. b0 + nb: plain split order, as wred_kernel
    for (int e = threadIdx.x; e < it.nb; e += 256) {
      const float* p = it.partial + it.b0 + e;
      float acc = 0.f;
      int sp = 0;
      for (; sp + 16 <= it.nsplit; sp += 16) {
        float t[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) t[c] = p[(size_t)(sp + c) * it.split_stride];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc += t[c];
      }
      for (; sp < it.nsplit; ++sp) acc += p[(size_t)sp * it.split_stride];
      float* g = it.grad + it.b0 + e;
      *g = it.accumulate ? *g + acc * us : acc * us;
    }
    return;
  }
  // vec: wred_kernel's 16-byte path -- chains c = split mod 4, combined as (b0 + b1) + (b2 + b3); otherwise one chain in plain split order
  const bool deep = it.vec && it.nsplit > 4;
  const int n = it.na * it.taps * it.nb;
  if (n <= 0 || n > (deep ? WRED_T_DEEP : WRED_T) || it.nb <= 0 || it.taps <= 0 || (it.v4 && (it.nb & 3))) return;  // (not a tile of plan_wred_items)
  if (it.v4) wred_tile_sums<4>(it, sm, n, deep); else wred_tile_sums<1>(it, sm, n, deep);
  __syncthreads();
  // the gradient goes out in OIHW order: runs of nb * taps (layout 0: one per a = co) or na * taps (layout 1: one per b = co) floats
  const int run = (it.layout == 1 ? it.na : it.nb) * it.taps;
  for (int m = threadIdx.x; m < n; m += 256) {
    const int q = (int)((unsigned)m / (unsigned)run), r = m - q * run;
    const int x = (int)((unsigned)r / (unsigned)it.taps), tt = r - x * it.taps;
    int l;
    size_t o;
    if (it.layout == 1) {  // q = co - b0, x = ci - a0, partial tap = taps - 1 - tt
      l = (x * it.taps + (it.taps - 1 - tt)) * it.nb + q;
      o = ((size_t)(it.b0 + q) * it.ci_total + it.a0) * it.taps + r;
    } else {  // q = co - a0, x = ci - b0
      l = (q * it.taps + tt) * it.nb + x;
      o = ((size_t)(it.a0 + q) * it.ci_total + it.b0) * it.taps + r;
    }
    const float s = deep ? (sm[l] + sm[n + l]) + (sm[2 * n + l] + sm[3 * n + l]) : sm[l];
    it.grad[o] = it.accumulate ? it.grad[o] + s * us : s * us;
  }
}

}  // namespace cgen

using namespace cgen;

extern "C" int cgen_wgrad_reduce_tiles(const cgen_wred_item* items, int32_t nitems, cgen_stream_t stream) {
  if (nitems <= 0) return CGEN_OK;
  CGEN_REQUIRE(items, "cgen_wgrad_reduce_tiles: null table");
  hipLaunchKernelGGL(wred_kernel_tiled, dim3(nitems), dim3(256), 0, (hipStream_t)stream, items);
  return check_launch("cgen_wgrad_reduce_tiles");
}
