// The multi-tensor kernels of a training step: weight re-imaging and the split-K reduce of the weight gradients.
//   wprep_kernel        OIHW f32 -> weight images (cgen_weight_prep)
//   wred_kernel         split-K partials -> flat OIHW gradient, one element group per thread.  Stays behind cgen_wgrad_reduce_ref as the
//                       executable definition of the sum order
//   wred_kernel_tiled   the same sums, bit for bit.  A workgroup owns a TILE of a site (a block of partial rows), sums it -- deep sites
//                       with the four split chains dealt to different lanes --, and writes the OIHW gradient from LDS in runs.
#include "common.h"

namespace cgen {

typedef f32x4_t f32x4;  // (wred_kernel's spelling)

// ============================================================================= multi-tensor weight prep / reduce
#define MT_CHUNK 1024  // elements per block

__global__ __launch_bounds__(256) void wprep_kernel(const cgen_wprep_desc* descs, const int* csite, const int* cidx) {
  // image row r, column k:  k = tap * ctot8 + c  with c running over the segments at 8-channel granularity
  const cgen_wprep_desc d = descs[csite[blockIdx.x]];
  const int taps = d.ks * d.ks;
  const int64_t base = (int64_t)cidx[blockIdx.x] * MT_CHUNK;
  int ctot8 = 0;
  if (d.mode == 0) { for (int s = 0; s < d.nseg; ++s) ctot8 += (d.seg_c[s] + 7) & ~7; }
  else ctot8 = (d.co + 7) & ~7;
  if (d.mode >= 8) {  // fragment-ordered images of the fused default Block (csrc/block4.hip; layout in include/cgen_hip.h)
    for (int i = threadIdx.x; i < MT_CHUNK; i += 256) {
      const int64_t o = base + i;
      if (o >= d.numel) break;
      const int frag = (int)(o >> 9), w = (int)(o & 511), ln = w >> 3, e = w & 7;
      const int r32 = ln & 31, kg = ln >> 5;
      const int q = (int)((uint32_t)frag / (uint32_t)d.k_pad), r = frag - q * d.k_pad;
      // channel (inside its 32-row block) that fragment row r32 carries.  Phase 3 (modes 12 / 13): the lane (pixel, kg) of the accumulator
      // tile ends up with 16 consecutive channels, 16 kg ..; phases 0-2 (modes 8-11): with HW = half the block's real channels (the
      // bottleneck rounded up to 8: 4, 8, 12 or 16), channels HW kg .. + HW in its first HW accumulators -- no lane idles on padding
      const int kgr = (r32 >> 2) & 1, jr = (r32 & 3) + 4 * (r32 >> 3);
      int perm = 16 * kgr + jr;
      if (d.mode <= 11) {
        const int bw = (d.mode == 8 || d.mode == 10) ? d.co : d.ci_total;  // bottleneck width
        const int mbq = d.mode <= 9 ? q : q / 9;
        const int hw = min(32, ((bw + 7) & ~7) - 32 * mbq) / 2;
        perm = jr < hw ? hw * kgr + jr : 1 << 20;
      }
      float v = 0.f;
      if (d.mode <= 9) {  // phase 0: frag = (32-row block * chunks + chunk) * 2 + step; a lane's K = 32 chunk + 16 step + 8 kg + e
        const int row = 32 * q + perm, kc = 32 * (r >> 1) + 16 * (r & 1) + 8 * kg + e;
        if (d.mode == 8) {
          if (row < d.co) {
            int cc = kc, off = 0, ci = -1;
            for (int s = 0; s < d.nseg; ++s) {  // (every segment padded to whole 32-channel chunks)
              const int c32 = (d.seg_c[s] + 31) & ~31;
              if (cc < c32) { if (cc < d.seg_c[s]) ci = off + cc; break; }
              cc -= c32; off += d.seg_c[s];
            }
            if (ci >= 0) v = d.src[(int64_t)row * d.ci_total + ci];
          }
        } else if (row < d.ci_total && kc < d.co) {
          v = d.src[(int64_t)kc * d.ci_total + row];
        }
      } else if (d.mode <= 11) {  // 3x3: frag = ((32-row block * 9 + tap) * groups + 16-channel group); k_pad = groups
        const int tap = q % 9, row = 32 * (q / 9) + perm, k = 16 * r + 8 * kg + e;
        if (d.mode == 10) { if (row < d.co && k < d.ci_total) v = d.src[((int64_t)row * d.ci_total + k) * 9 + tap]; }
        else if (row < d.ci_total && k < d.co) v = d.src[((int64_t)k * d.ci_total + row) * 9 + (8 - tap)];
      } else {  // phase 3: frag = 32-row block * groups + 16-channel group of the bottleneck; k_pad = groups
        const int row = 32 * q + perm, k = 16 * r + 8 * kg + e;
        if (d.mode == 12) { if (row < d.co && k < d.ci_total) v = d.src[(int64_t)row * d.ci_total + k]; }
        else if (row < d.seg_c[0] && k < d.co) v = d.src[(int64_t)k * d.ci_total + d.seg_off + row];
      }
      ((h16_t*)d.dst)[o] = f2h(v);
    }
    return;
  }
  if (d.mode >= 6) {  // 16-row images of the row-streaming Block instance: frag = tap * chunks + q (k_pad = chunks)
    for (int i = threadIdx.x; i < MT_CHUNK; i += 256) {
      const int64_t o = base + i;
      if (o >= d.numel) break;
      const int frag = (int)(o >> 9), w = (int)(o & 511), ln = w >> 3, e = w & 7;
      const int row = ln & 15, kc = 8 * (ln >> 4) + e;
      const int tap = (int)((uint32_t)frag / (uint32_t)d.k_pad), q = frag - tap * d.k_pad, c = 32 * q + kc;
      float v = 0.f;
      if (d.mode == 6) { if (row < d.co && c < d.ci_total) v = d.src[((int64_t)row * d.ci_total + c) * 9 + tap]; }
      else if (row < d.ci_total && c < d.co) v = d.src[((int64_t)c * d.ci_total + row) * 9 + (8 - tap)];
      ((h16_t*)d.dst)[o] = f2h(v);
    }
    return;
  }
  if (d.mode >= 2) {  // fragment-ordered images of the fused Block kernel (csrc/block.hip; layout in include/cgen_hip.h)
    for (int i = threadIdx.x; i < MT_CHUNK; i += 256) {
      const int64_t o = base + i;
      if (o >= d.numel) break;
      int frag = (int)(o >> 9);
      const int w = (int)(o & 511), ln = w >> 3, e = w & 7;
      const int r32 = ln & 31, kg = ln >> 5;
      int row = 16 * ((r32 >> 2) & 1) + (r32 & 3) + 4 * (r32 >> 3);  // channel (inside its 32-block) that fragment row r32 carries
      float v = 0.f;
      if (d.mode <= 3) {  // phase A: frag = (32-row block * chunks + chunk) * 18 + kk; k_pad = fragments per 32-row block (0: one block)
        if (d.k_pad > 0) { const int mb = (int)((uint32_t)frag / (uint32_t)d.k_pad); frag -= mb * d.k_pad; row += 32 * mb; }
        const int j = (int)((uint32_t)frag / 18u), kk = frag - j * 18, half = kk >= 9 ? 1 : 0, tap = kk - 9 * half;  // (a wave's nine fragments are contiguous)
        const int kc = 32 * j + 16 * half + 8 * kg + e;  // position on the concatenated input axis (segments in whole chunks)
        if (d.mode == 2) {
          if (row < d.co) {
            int cc = kc, off = 0, ci = -1;
            for (int s = 0; s < d.nseg; ++s) {  // (every segment padded to whole 32-channel chunks)
              const int c32 = (d.seg_c[s] + 31) & ~31;
              if (cc < c32) { if (cc < d.seg_c[s]) ci = off + cc; break; }
              cc -= c32; off += d.seg_c[s];
            }
            if (ci >= 0) v = d.src[((int64_t)row * d.ci_total + ci) * 9 + tap];
          }
        } else if (row < d.ci_total && kc < d.co) {
          v = d.src[((int64_t)kc * d.ci_total + row) * 9 + (8 - tap)];
        }
      } else {  // phase B: frag = pair * k_pad + K16-step
        const int pair = (int)((uint32_t)frag / (uint32_t)d.k_pad), ks16 = frag - pair * d.k_pad;
        const int k = 16 * ks16 + 8 * kg + e;
        const int bw = d.mode == 4 ? d.ci_total : d.co;  // bottleneck width (a multiple of 8)
        const int tap = (int)((uint32_t)k / (uint32_t)bw), c = k - tap * bw;
        const int och = pair * 32 + row;
        if (tap < 9) {
          if (d.mode == 4) { if (och < d.co) v = d.src[((int64_t)och * d.ci_total + c) * 9 + tap]; }
          else if (och < d.seg_c[0]) v = d.src[((int64_t)c * d.ci_total + d.seg_off + och) * 9 + (8 - tap)];
        }
      }
      ((h16_t*)d.dst)[o] = f2h(v);
    }
    return;
  }
  for (int i = threadIdx.x; i < MT_CHUNK; i += 256) {
    const int64_t o = base + i;
    if (o >= d.numel) break;
    // (32-bit unsigned index arithmetic: an image has < 2^31 elements -- the 64-bit division cost ~100 instructions per element
    //  and the launch was 0.2 ms at the head of every step's critical path)
    const uint32_t o32 = (uint32_t)o;
    const int r = (int)(o32 / (uint32_t)d.k_pad);
    const int k = (int)(o32 - (uint32_t)r * (uint32_t)d.k_pad);
    const int tap = (int)((uint32_t)k / (uint32_t)ctot8), c = k - tap * ctot8;
    float v = 0.f;
    if (tap < taps) {
      if (d.mode == 0) {  // forward image: r = co
        if (r < d.co) {
          int cc = c, off = 0, ci = -1;
          for (int s = 0; s < d.nseg; ++s) {
            const int c8 = (d.seg_c[s] + 7) & ~7;
            if (cc < c8) { if (cc < d.seg_c[s]) ci = off + cc; break; }
            cc -= c8; off += d.seg_c[s];
          }
          if (ci >= 0) v = d.src[((int64_t)r * d.ci_total + ci) * taps + tap];
        }
      } else {  // dgrad image of one segment: r = local ci, c = co, taps flipped
        if (r < d.seg_c[0] && c < d.co) v = d.src[((int64_t)c * d.ci_total + d.seg_off + r) * taps + (taps - 1 - tap)];
      }
    }
    if (d.dtype == CGEN_F32) ((float*)d.dst)[o] = v; else ((h16_t*)d.dst)[o] = f2h(v);
  }
}

__global__ __launch_bounds__(256) void wred_kernel(const cgen_wred_desc* descs, const int* csite, const int* cidx) {
  // Threads walk the PARTIAL layout [co][tap][ci] (what the wgrad kernels wrote), 4 consecutive ci per thread, so the
  // nsplit-deep reads are coalesced 16-byte streams; the sum is scattered into the OIHW gradient (1/nsplit of the bytes).
  const cgen_wred_desc d = descs[csite[blockIdx.x]];
  const int taps = d.ks * d.ks;
  const float us = d.unscale == 0.f ? 1.f : d.unscale;  // 1 / loss scale of the f16 engine (a power of two: exact)
  const int nw = d.co * d.ci_total * taps;  // < 2^31 (checked on the host)
  const int s0 = cidx[blockIdx.x] * MT_CHUNK + threadIdx.x * 4;
  if (s0 >= d.numel) return;
  if (s0 < nw) {
    const bool vec = (nw & 3) == 0 && (((uintptr_t)d.partial_w) & 15) == 0;  // (16-byte loads of 4 consecutive partial elements: any layout)
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    const int cnt = min(4, nw - s0);
    if (vec) {
      const float4* src = (const float4*)(d.partial_w + s0);
      const size_t stride = (size_t)nw / 4;
      // four independent chains of streaming (non-temporal) 16-byte loads: the partials are read exactly once; the sum order
      // ((c0 + c1) + (c2 + c3)) over splits dealt round-robin is fixed => deterministic
      float4 b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      int sp = 0;
      // sixteen loads in flight per thread first: a thread walks its element's splits alone, and the streaming weight-gradient kernel
      // leaves up to 144 of them (192^2 layers) -- at four per round trip the final reduce was 36 dependent HBM latencies long
      // (0.15 ms at the end of every step for 108 MB).  The order of the additions is the one below: bit-identical sums.
      for (; sp + 16 <= d.nsplit; sp += 16) {
        f32x4 t[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) t[c] = __builtin_nontemporal_load((const f32x4*)(src + (size_t)(sp + c) * stride));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int c = 0; c < 4; ++c) { b[c].x += t[4 * u + c][0]; b[c].y += t[4 * u + c][1]; b[c].z += t[4 * u + c][2]; b[c].w += t[4 * u + c][3]; }
      }
      for (; sp + 4 <= d.nsplit; sp += 4) {
        float4 v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 t = __builtin_nontemporal_load((const f32x4*)(src + (size_t)(sp + c) * stride));  // one global_load_dwordx4 nt
          v[c] = make_float4(t[0], t[1], t[2], t[3]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) { b[c].x += v[c].x; b[c].y += v[c].y; b[c].z += v[c].z; b[c].w += v[c].w; }
      }
      for (int c = 0; sp < d.nsplit; ++sp, ++c) {
        const float4 v0 = src[(size_t)sp * stride];
        b[c].x += v0.x; b[c].y += v0.y; b[c].z += v0.z; b[c].w += v0.w;
      }
      a[0] = (b[0].x + b[1].x) + (b[2].x + b[3].x); a[1] = (b[0].y + b[1].y) + (b[2].y + b[3].y);
      a[2] = (b[0].z + b[1].z) + (b[2].z + b[3].z); a[3] = (b[0].w + b[1].w) + (b[2].w + b[3].w);
    } else {
      for (int e = 0; e < cnt; ++e) {
        float acc = 0.f;
        for (int sp = 0; sp < d.nsplit; ++sp) acc += d.partial_w[(size_t)sp * nw + s0 + e];
        a[e] = acc;
      }
    }
    for (int e = 0; e < cnt; ++e) {
      const unsigned sidx = (unsigned)(s0 + e);
      size_t o;
      if (d.layout == 1) {  // [ci][flipped tap][co] (the streaming kernel with grad_out as its shifted operand, csrc/wgrad3.hip)
        const unsigned r = sidx / (unsigned)d.co, co = sidx - r * d.co;
        const unsigned ci = r / (unsigned)taps, ft = r - ci * taps;
        o = ((size_t)co * d.ci_total + ci) * taps + (taps - 1 - ft);
      } else {
        const unsigned r = sidx / (unsigned)d.ci_total, ci = sidx - r * d.ci_total;
        const unsigned co = r / (unsigned)taps, tap = r - co * taps;
        o = ((size_t)co * d.ci_total + ci) * taps + tap;
      }
#ifdef WRED_ABL_NOSCATTER  // (ablation build, wrong results: the sums go out in partial order, coalesced)
      o = sidx;
#endif
      d.grad_w[o] = d.accumulate ? d.grad_w[o] + a[e] * us : a[e] * us;
    }
  }
  if (d.grad_b && s0 + 3 >= nw) {  // elements nw .. numel-1 are the bias gradient: this thread's (up to four) sums run side by side --
    // one after the other they were 4 x nsplit / 16 dependent round trips on the one thread that owns them, the end of the launch
    int co4[4];
    bool ok4[4];
    float acc4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int o = s0 + e; ok4[e] = o >= nw && o < d.numel; co4[e] = ok4[e] ? o - nw : 0; }
    int sp = 0;
    for (; sp + 16 <= d.nsplit; sp += 16) {  // (loads first, additions in split order: the same sums as a plain loop)
      float t[4][16];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 16; ++c) t[e][c] = d.partial_b[(size_t)(sp + c) * d.co + co4[e]];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 16; ++c) acc4[e] += t[e][c];
    }
    for (; sp < d.nsplit; ++sp)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc4[e] += d.partial_b[(size_t)sp * d.co + co4[e]];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ok4[e]) d.grad_b[co4[e]] = d.accumulate ? d.grad_b[co4[e]] + acc4[e] * us : acc4[e] * us;
  }
}

// ============================================================================= the split-K reduce in its tiled form
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

extern "C" int cgen_weight_prep(const cgen_wprep_desc* descs, const int32_t* csite, const int32_t* cidx, int32_t nchunks,
                                cgen_stream_t stream) {
  if (nchunks <= 0) return CGEN_OK;
  CGEN_REQUIRE(descs && csite && cidx, "cgen_weight_prep: null table");
  hipLaunchKernelGGL(wprep_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, descs, csite, cidx);
  return check_launch("cgen_weight_prep");
}

extern "C" int cgen_wgrad_reduce(const cgen_wred_desc* descs, const int32_t* csite, const int32_t* cidx, int32_t nchunks,
                                 cgen_stream_t stream) {
  if (nchunks <= 0) return CGEN_OK;
  CGEN_REQUIRE(descs && csite && cidx, "cgen_wgrad_reduce: null table");
  hipLaunchKernelGGL(wred_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, descs, csite, cidx);
  return check_launch("cgen_wgrad_reduce");
}

// These names keep the per-element kernels reachable as the reference of the tiled form below.
extern "C" int cgen_weight_prep_ref(const cgen_wprep_desc* descs, const int32_t* csite, const int32_t* cidx, int32_t nchunks,
                                    cgen_stream_t stream) {
  return cgen_weight_prep(descs, csite, cidx, nchunks, stream);
}

extern "C" int cgen_wgrad_reduce_ref(const cgen_wred_desc* descs, const int32_t* csite, const int32_t* cidx, int32_t nchunks,
                                     cgen_stream_t stream) {
  return cgen_wgrad_reduce(descs, csite, cidx, nchunks, stream);
}

extern "C" int cgen_wgrad_reduce_tiles(const cgen_wred_item* items, int32_t nitems, cgen_stream_t stream) {
  if (nitems <= 0) return CGEN_OK;
  CGEN_REQUIRE(items, "cgen_wgrad_reduce_tiles: null table");
  hipLaunchKernelGGL(wred_kernel_tiled, dim3(nitems), dim3(256), 0, (hipStream_t)stream, items);
  return check_launch("cgen_wgrad_reduce_tiles");
}
