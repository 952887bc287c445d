// Weight gradient of the implicit-GEMM convolution for gfx950 (MI355X): cgen_conv2d_wgrad, cgen_conv2d_wgrad_plan and the batch
// plan / run (cgen_conv2d_wgrad_batch_*), which also drive the streaming kernel of csrc/wgrad3.hip.  Split-K partials out; the
// reduce to the OIHW gradient is csrc/multitensor.hip's.  GEMM view and shared kit: csrc/conv.hip, csrc/conv_shared.h.
//   wgrad_kernel<T,NTC>           generic weight gradient (f32 MFMA)
//   wgrad_tile_kernel / wgrad_tile_batched_kernel<NCF,NJW,KS> / wgrad_tile_mega_kernel   bf16 weight gradient with LDS transpose
//                                 reads; the batched forms run the workgroups of many problems in one launch
#include <algorithm>
#include <vector>

#include "conv_shared.h"
#include "wgrad3.h"
#include "like_head.h"

namespace cgen {

// ============================================================================= weight gradient
// dW[co][tap][ci] = sum_px G[px][co] * act(X)[px + tap][ci]          (f32 MFMA 16x16x4 for both storage dtypes)
// Workgroup tile: (16*NTC output channels) x (32 input channels) x (<= 9 taps) x one pixel split.
// (WG_PK = 64 pixels per K-step, WG_MAXT = 9 taps, and the split geometry: like_head.h)

struct WgP {
  int N, H, W, KS, pad, nseg, act, Co, P, taps, ci_total, nsplit, pix_per_split, n_tapgroups, n_cichunks;
  View seg[CGEN_MAX_SEG];
  int seg_off[CGEN_MAX_SEG];
  int seg_vec[CGEN_MAX_SEG];
  int seg_chunk0[CGEN_MAX_SEG + 1];  // first 32-wide chunk index of each segment
  View gout;
  int gout_vec;
  float* pw;
  float* pb;
};

template <typename T, int NTC>
__global__ __launch_bounds__(256) void wgrad_kernel(WgP p) {
  constexpr int COT = NTC * 16;
  constexpr int LDG = COT + 16;  // stride == 16 (mod 32) -> conflict-free b32 fragment reads
  constexpr int LDX = 32 + 16;
  constexpr int NPAIR = NTC * 2;                 // (co-frag, ci-frag) pairs
  constexpr int KW = NPAIR >= 4 ? 1 : 4 / NPAIR; // K-ways across waves
  constexpr int PPW = NPAIR >= 4 ? NPAIR / 4 : 1;
  constexpr int G = 16 / sizeof(T);
  __shared__ float Gs[WG_PK * LDG];
  __shared__ float Xs[WG_PK * LDX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x;
  const int chunk = blockIdx.y;  // global 32-wide ci chunk
  const int co_tile = blockIdx.z / p.n_tapgroups, tg = blockIdx.z % p.n_tapgroups;
  const int co_base = co_tile * COT;
  const int t0 = tg * WG_MAXT;
  const int ntap = min(WG_MAXT, p.taps - t0);
  int s = 0;
  while (s + 1 < p.nseg && chunk >= p.seg_chunk0[s + 1]) ++s;
  const int c0 = (chunk - p.seg_chunk0[s]) * 32;
  const View sv = p.seg[s];

  const int px0 = sp * p.pix_per_split;
  const int px1 = min(p.P, px0 + p.pix_per_split);

  f32x4 acc[WG_MAXT][PPW];
#pragma unroll
  for (int t = 0; t < WG_MAXT; ++t)
#pragma unroll
    for (int q = 0; q < PPW; ++q) acc[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  const int kpart = (KW > 1) ? (wave / NPAIR) : 0;
  const int pair0 = (KW > 1) ? (wave % NPAIR) : wave * PPW;

  for (int pc = px0; pc < px1; pc += WG_PK) {
    __syncthreads();
    // ---- gradient tile Gs[64][COT] (f32)
    for (int g = tid; g < WG_PK * COT / 4; g += 256) {
      const int r = g / (COT / 4), cg = (g % (COT / 4)) * 4;
      const int m = pc + r, co = co_base + cg;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (m < px1 && co < p.Co) {
        const int n = m / (p.H * p.W);
        const int rr = m - n * p.H * p.W;
        const int y = rr / p.W, x = rr - y * p.W;
        const T* src = vptr<T>(p.gout, n, y, x) + co;
        if (p.gout_vec && co + 4 <= p.Co) {
          ld4<T>(src, v);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (co + e < p.Co) v[e] = Elem<T>::ld(src + e);
        }
      }
      *(float4*)(Gs + r * LDG + cg) = make_float4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int tt = 0; tt < WG_MAXT; ++tt) {
      if (tt < ntap) {
        const int tap = t0 + tt;
        const int dy = tap / p.KS - p.pad, dx = tap % p.KS - p.pad;
        if (tt > 0) __syncthreads();
        // ---- activation tile Xs[64][32] for this tap
        for (int g = tid; g < WG_PK * 32 / G; g += 256) {
          const int r = g / (32 / G), cg = (g % (32 / G)) * G;
          const int m = pc + r, cs = c0 + cg;
          float v[G];
#pragma unroll
          for (int e = 0; e < G; ++e) v[e] = 0.f;
          if (m < px1 && cs < sv.c) {
            const int n = m / (p.H * p.W);
            const int rr = m - n * p.H * p.W;
            const int y = rr / p.W + dy, x = rr % p.W + dx;
            if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
              const T* src = vptr<T>(sv, n, y, x) + cs;
              if (p.seg_vec[s] && cs + G <= sv.c) {
                Pack<T, G> tmp;
                tmp.v4 = *(const uint4*)src;
#pragma unroll
                for (int e = 0; e < G; ++e) v[e] = act_fwd(p.act, Elem<T>::ld(&tmp.e[e]));
              } else {
#pragma unroll
                for (int e = 0; e < G; ++e) if (cs + e < sv.c) v[e] = act_fwd(p.act, Elem<T>::ld(src + e));
              }
            }
          }
#pragma unroll
          for (int e = 0; e < G; e += 4) *(float4*)(Xs + r * LDX + cg + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
        }
        __syncthreads();
        if (tt == 0 && p.pb && chunk == 0 && tg == 0 && tid < COT) {
          float a = 0.f;
          for (int r = 0; r < WG_PK; ++r) a += Gs[r * LDG + tid];
          bsum += a;
        }
        // ---- MFMA: D[co][ci] += G^T[co][px] * X[px][ci]
        const int kq0 = kpart * (WG_PK / 4 / KW), kq1 = kq0 + WG_PK / 4 / KW;
#pragma unroll
        for (int q = 0; q < PPW; ++q) {
          const int pr = pair0 + q;
          const int cf = pr >> 1, jf = pr & 1;
          for (int k4 = kq0; k4 < kq1; ++k4) {
            const int prow = k4 * 4 + (lane >> 4);
            const float a = Gs[prow * LDG + cf * 16 + (lane & 15)];
            const float b = Xs[prow * LDX + jf * 16 + (lane & 15)];
            acc[tt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tt][q], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- write partials (K-ways are combined through LDS in a fixed order)
  __syncthreads();
  float* red = Gs;  // reuse (>= 64*32 floats)
#pragma unroll
  for (int tt = 0; tt < WG_MAXT; ++tt) {
    if (tt < ntap) {
#pragma unroll
      for (int q = 0; q < PPW; ++q) {
        f32x4 v = acc[tt][q];
        if (KW > 1) {
          // waves with kpart > 0 publish, kpart == 0 sums in kpart order
          for (int kp = 1; kp < KW; ++kp) {
            __syncthreads();
            if (kpart == kp) *(f32x4*)(red + ((wave % NPAIR) * 64 + lane) * 4) = v;
            __syncthreads();
            if (kpart == 0) {
              const f32x4 o = *(const f32x4*)(red + ((wave % NPAIR) * 64 + lane) * 4);
              v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
            }
          }
        }
        if (kpart == 0) {
          const int pr = pair0 + q;
          const int cf = pr >> 1, jf = pr & 1;
          const int ci = c0 + jf * 16 + (lane & 15);
          if (ci < sv.c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int co = co_base + cf * 16 + (lane >> 4) * 4 + e;
              if (co < p.Co)
                p.pw[(((size_t)sp * p.Co + co) * p.taps + (t0 + tt)) * p.ci_total + p.seg_off[s] + ci] = v[e];
            }
          }
        }
      }
    }
  }
  if (p.pb && chunk == 0 && tg == 0 && tid < COT && co_base + tid < p.Co) p.pb[(size_t)sp * p.Co + co_base + tid] = bsum;
}

// ============================================================================= weight gradient, tiled / streaming (bf16)
// dW[co][tap][ci] = sum_px G[px][co] * act(X)[px + tap][ci] with the PIXEL axis as the MFMA K dimension.
// Both operands live in HBM with channels contiguous, so K (pixels) is strided: the fragments are assembled with the
// gfx950 LDS transpose read ds_read_b64_tr_b16 (4 pixels x 16 channels -> each lane gets 4 consecutive-K values of its
// channel) straight from NHWC tiles in LDS -- no explicit transposes.
// A persistent workgroup owns the whole [16*NCF co] x [taps x cwin ci] gradient slab in MFMA accumulators
// (output-stationary) and streams 8x16 pixel tiles through LDS by global->LDS DMA: every activation / gradient element
// is read from HBM exactly once per (co range, ci window).  2 workgroups per CU: one's DMA wait overlaps the other's MFMAs.
//
#define WG2_MAXACC 24  // accumulator fragments per wave (96 VGPRs)

struct Wg2P {
  int N, H, W, KS, nseg, act, Co, taps, ci_total, ctot8;
  View seg[CGEN_MAX_SEG];
  int seg_koff[CGEN_MAX_SEG];  // 8-granular concat offsets
  int seg_off[CGEN_MAX_SEG];   // real channel offsets in the OIHW gradient
  View gout;
  float* pw;
  float* pb;
  int tiles_x, tiles_y, ntiles, nsplit, tiles_per_split;
  int cwin, cog;  // channel window, co columns staged per workgroup (16*NCF)
  int dbg;        // ablation mask (CGEN_WG2_DBG): 1 skip DMA, 2 skip activation pass, 4 skip MFMA loop
  unsigned long long* stamps;  // optional (CGEN_WG2_STAMPS): per-phase cycle stamps of workgroup 0
  PixTile xt, gt;
  FastDiv d_tx, d_ty;
  int variant, dbuf;  // ncf * 2 + (KS == 3): which body the all-variant kernel runs for this problem; dbuf: two tile buffers (the next tile's DMA flies under this tile's MFMAs)
};

typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ h16x8 tr_pair(const char* p0, const char* p1, const bool plain = false) {
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
  if (plain) {  // ablation (CGEN_WG2_DBG & 8): ordinary 8-byte LDS reads instead of the transposing ones (wrong math, same traffic)
    union { s16x4 h[2]; h16x8 v; } u;
    u.h[0] = *(const s16x4*)p0; u.h[1] = *(const s16x4*)p1;
    return u.v;
  }
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)p1);
  union { s16x4 h[2]; h16x8 v; } u;
  u.h[0] = lo; u.h[1] = hi;
  return u.v;
}

template <int NCF, int NJW, int KS>
__device__ __forceinline__ void wgrad_tile_body(const Wg2P& p, const int bid_x, const int bid_y, const int bid_z) {
  typedef h16_t T;
  constexpr int G = 8;
  constexpr int HALO = KS / 2, HH = TILE_H + 2 * HALO, HW = TILE_W + 2 * HALO;
  constexpr int TAPS = KS * KS;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* gbl_ptr;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bufbytes = p.xt.bytes + p.gt.bytes;  // one tile buffer: activation halo tile, then the gradient tile
  const bool dbuf = p.dbuf != 0;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sp = bid_x;
  const int cA = bid_y * p.cwin;
  const int cw = min(p.cwin, p.ctot8 - cA);      // multiple of 8
  const int cw16 = (cw + 15) & ~15;
  const int cgrp = cw16 >> 4;
  const int njf = TAPS * cgrp;                   // (tap, 16-channel group) fragments of this window
  const int co_base = bid_z * (NCF * 16);
  const int t_begin = sp * p.tiles_per_split, t_end = min(p.ntiles, t_begin + p.tiles_per_split);

  f32x4 acc[NCF][NJW];
  f32x4 accb[NCF];
#pragma unroll
  for (int a = 0; a < NCF; ++a) {
    accb[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJW; ++j) acc[a][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bool do_bias = p.pb != nullptr && bid_y == 0 && wave == 0;
  const unsigned long long t_entry = __builtin_readcyclecounter();

  // ---- per-lane DMA constants (identical for every piece of every tile)
  // activation tile: lane -> (pixel xl inside the piece, channel group) -> segment / channel / element offset
  const int xl = fdiv(lane, p.xt.d_gpr), xcg = lane - xl * p.xt.gpr;
  int x_si = 0, x_off = 0;
  bool x_lane = xl < p.xt.ppp && xcg * G < cw16, x_data = false;
  {
    const int c = cA + xcg * G;
#pragma unroll
    for (int k = 1; k < CGEN_MAX_SEG; ++k) x_si += (k < p.nseg && c >= p.seg_koff[k]) ? 1 : 0;
    View sv = p.seg[0];
    int koff = p.seg_koff[0];
#pragma unroll
    for (int k = 1; k < CGEN_MAX_SEG; ++k)
      if (x_si == k) { sv = p.seg[k]; koff = p.seg_koff[k]; }
    const int cs = c - koff;
    x_data = x_lane && xcg * G < cw && cs < sv.c;
    x_off = (int)(xl * sv.sw) + cs;
  }
  // gradient tile
  const int gl = fdiv(lane, p.gt.d_gpr), gcg = lane - gl * p.gt.gpr;
  const bool g_lane = gl < p.gt.ppp && gcg * G < p.cog;
  const bool g_data = g_lane && co_base + gcg * G < p.Co;
  const int g_off = (int)(gl * p.gout.sw) + co_base + gcg * G;
  const int xpieces = p.xt.rows * p.xt.ppr, gpieces = p.gt.rows * p.gt.ppr;

  LaneTile LX, LG;
  {
    LX.xl = xl; LX.lane = x_lane; LX.data = x_data;
    LX.sh = (int)p.seg[0].sh; LX.swp = (int)(p.seg[0].sw * p.xt.ppp);
#pragma unroll
    for (int k = 1; k < CGEN_MAX_SEG; ++k)
      if (x_si == k) { LX.sh = (int)p.seg[k].sh; LX.swp = (int)(p.seg[k].sw * p.xt.ppp); }
    LG.xl = gl; LG.lane = g_lane; LG.data = g_data;
    LG.sh = (int)p.gout.sh; LG.swp = (int)(p.gout.sw * p.gt.ppp);
  }
  auto issue_tile = [&](int t, char* Xb, char* Gb) {
    const int b1 = fdiv(t, p.d_tx), tx = t - b1 * p.tiles_x;
    const int n = fdiv(b1, p.d_ty), ty = b1 - n * p.tiles_y;
    const int y0 = ty * TILE_H, x0 = tx * TILE_W;
    const T* my_org = vptr32<T>(p.seg[0], n, y0 - HALO, x0 - HALO);  // this lane's segment
    if (p.nseg > 1) {
      if (x_si == 1) my_org = vptr32<T>(p.seg[1], n, y0 - HALO, x0 - HALO);
      if (x_si == 2) my_org = vptr32<T>(p.seg[2], n, y0 - HALO, x0 - HALO);
      if (x_si == 3) my_org = vptr32<T>(p.seg[3], n, y0 - HALO, x0 - HALO);
    }
    dma_tile<T>(p.xt, LX, my_org + x_off, Xb, wave, max(0, HALO - y0), min(HH, p.H + HALO - y0), max(0, HALO - x0), min(HW, p.W + HALO - x0));
    dma_tile<T>(p.gt, LG, vptr32<T>(p.gout, n, y0, x0) + g_off, Gb, wave, 0, min(TILE_H, p.H - y0), 0, min(TILE_W, p.W - x0));
  };
  // in-place activation of the staged halo tile: every lane re-visits the groups it DMA'd (same piece mapping)
  auto act_pass = [&](char* Xb) { act_pieces<T>(Xb, wave, lane, xpieces, p.act); };

  // lane geometry of the transpose reads: group g = k-block, t = 4r + q supplies (pixel r of the read, channels 4q..4q+3)
  const int g = lane >> 4, t16 = lane & 15, r = t16 >> 2, qd = t16 & 3;
  const int krow = g >> 1, kx = (g & 1) * 8 + r;  // this lane's FIRST read inside a 2-row K-step: pixel (row, x); second: x + 4
  // tile-independent LDS byte offsets of this lane's two reads per (tap, channel group) fragment
  int xo0[NJW], xo1[NJW];
  int jtap[NJW], jcb[NJW];  // (tap, first channel of the 16-channel group) of fragment j of this wave; wave-uniform
  {
    int tapw = wave / cgrp, gw = wave - tapw * cgrp;  // fragment jf = wave + 4j  ->  (tap, group), walked incrementally
#pragma unroll
    for (int j = 0; j < NJW; ++j) {
      const int tap = tapw < TAPS ? tapw : TAPS - 1;  // waves short of a fragment compute a duplicate that is never written out
      const int cb = tapw < TAPS ? gw * 16 : 0;
      jtap[j] = tap; jcb[j] = cb;
      const int dy = tap / KS, dx = tap % KS;
      xo0[j] = pix_off(p.xt, krow + dy, kx + dx) + (cb + qd * 4) * 2;
      xo1[j] = pix_off(p.xt, krow + dy, kx + dx + 4) + (cb + qd * 4) * 2;
      gw += 4;
      while (gw >= cgrp) { gw -= cgrp; ++tapw; }
    }
  }
  const int nj_eff = (njf + 3) >> 2;  // fragments per wave, the same for all four waves
  const int go0 = pix_off(p.gt, krow, kx) + qd * 8, go1 = pix_off(p.gt, krow, kx + 4) + qd * 8;
  h16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (h16n_t)1.0f;

  const bool stamp = p.stamps != nullptr && bid_x == 0 && bid_y == 0 && bid_z == 0 && tid == 0;
#ifdef CGEN_WG2_ABLATE
  const bool plain_rd = (p.dbg & 8) != 0, no_mfma = (p.dbg & 16) != 0;
#else
  constexpr bool plain_rd = false;
#endif
  int nst = 0;
#define WG2_STAMP() do { if (stamp && nst < 60) p.stamps[nst++] = __builtin_readcyclecounter(); } while (0)
  if (stamp) p.stamps[nst++] = t_entry;
  WG2_STAMP();
  // One tile: activation pass + MFMAs on the buffer `cur` while (double-buffered problems) the DMA of tile t + 1 fills `nxt`.
  // Two things keep that DMA in flight: (1) `cur` / `nxt` are __restrict__ -- hipcc tracks an LDS-DMA as a pending LDS write
  // and, without alias information, puts s_waitcnt vmcnt(0) in front of the next LDS read; (2) the barrier between the
  // activation pass and the MFMAs is a bare lgkmcnt(0) + s_barrier: __syncthreads() drains vmcnt as well.
  auto tile_step = [&](char* __restrict__ cur, char* __restrict__ nxt, const int t) {
    if (dbuf && t + 1 < t_end && !(p.dbg & 1)) issue_tile(t + 1, nxt, nxt + p.xt.bytes);
    WG2_STAMP();
    char* Xb = cur;
    char* Gb = cur + p.xt.bytes;
    if (p.act != CGEN_ACT_NONE && !(p.dbg & 2)) {
      act_pass(Xb);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    WG2_STAMP();
    if (!(p.dbg & 4)) {
      // fragments are processed in chunks of CH: all transpose reads of a chunk are issued before its MFMAs (one LDS
      // latency per chunk instead of per fragment); the chunk test is wave-uniform and identical for the four waves
      constexpr int CH = (NJW % 4 == 0) ? 4 : 3;
#pragma unroll
      for (int ks = 0; ks < TILE_H / 2; ++ks) {
        h16x8 af[NCF];
        const char* gk = Gb + ks * 2 * p.gt.rowbytes;
#pragma unroll
        for (int a = 0; a < NCF; ++a) af[a] = tr_pair(gk + go0 + a * 32, gk + go1 + a * 32, plain_rd);
        if (do_bias) {
#pragma unroll
          for (int a = 0; a < NCF; ++a) accb[a] = mfma_h16(af[a], ones, accb[a], 0, 0, 0);
        }
        const char* xk = Xb + ks * 2 * p.xt.rowbytes;
#pragma unroll
        for (int j0 = 0; j0 < NJW; j0 += CH) {
          if (j0 < nj_eff) {
            h16x8 bfv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) bfv[u] = tr_pair(xk + xo0[j0 + u], xk + xo1[j0 + u], plain_rd);
#pragma unroll
            for (int u = 0; u < CH; ++u)
#pragma unroll
              for (int a = 0; a < NCF; ++a) {
#ifdef CGEN_WG2_ABLATE  // (tools/coexec_probe.py, CGEN_WG2_DBG & 16): keep the LDS reads alive without the matrix instruction
                if (no_mfma) {
                  union { h16x8 v; float f[4]; } ua, ub;
                  ua.v = af[a]; ub.v = bfv[u];
                  acc[a][j0 + u][0] += ua.f[0] + ub.f[0]; acc[a][j0 + u][1] += ua.f[1] + ub.f[1];
                  acc[a][j0 + u][2] += ua.f[2] + ub.f[2]; acc[a][j0 + u][3] += ua.f[3] + ub.f[3];
                  continue;
                }
#endif
                acc[a][j0 + u] = mfma_h16(af[a], bfv[u], acc[a][j0 + u], 0, 0, 0);
              }
          }
        }
      }
    }
    WG2_STAMP();
  };
  if (!(p.dbg & 1) && t_begin < t_end) issue_tile(t_begin, smem, smem + p.xt.bytes);
  int cur = 0;
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();  // hipcc waits vmcnt(0) here: tile t has landed; and every wave is done reading the other buffer
    WG2_STAMP();
    tile_step(smem + cur * bufbytes, smem + (cur ^ 1) * bufbytes, t);
    if (dbuf) {
      cur ^= 1;
    } else if (t + 1 < t_end) {  // single buffer (the tile pair is too big for two): fetch the next tile once this one is consumed
      __syncthreads();
      if (!(p.dbg & 1)) issue_tile(t + 1, smem, smem + p.xt.bytes);
    }
  }
  __syncthreads();  // (the batched kernels start the next problem's DMA right away)

  // ---- write the partial slab straight from the accumulators.  Lane (g, t16) of fragment (a, j) holds
  // D[co = a*16 + 4g + e][ci = cb_j + t16]: 16 consecutive input channels = one 64-byte run per (co, tap).  Everything
  // but a per-lane constant is wave-uniform, so a store costs no address arithmetic: what made this tail expensive
  // before was 64-bit index math per store, not the stores.
  {
    // this lane's real input-channel index for fragment j (8-granular concat index -> segment -> OIHW channel), -1: padding
    const int cl = cA + t16;
    float* pw_lane = p.pw + ((size_t)sp * p.Co + co_base + g * 4) * TAPS * p.ci_total;
#pragma unroll
    for (int j = 0; j < NJW; ++j) {
      const int jf = wave + 4 * j;
      if (jf < njf) {
        const int c = cl + jcb[j];
        int sidx = 0;
#pragma unroll
        for (int k = 1; k < CGEN_MAX_SEG; ++k) sidx += (k < p.nseg && c >= p.seg_koff[k]) ? 1 : 0;
        int koff = p.seg_koff[0], segc = p.seg[0].c, soff = p.seg_off[0];
#pragma unroll
        for (int k = 1; k < CGEN_MAX_SEG; ++k)
          if (sidx == k) { koff = p.seg_koff[k]; segc = p.seg[k].c; soff = p.seg_off[k]; }
        const int cs = c - koff;
        const bool cv = jcb[j] + t16 < cw && cs < segc;
        float* col = pw_lane + jtap[j] * p.ci_total + soff + cs;
#pragma unroll
        for (int a = 0; a < NCF; ++a)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cv && co_base + a * 16 + g * 4 + e < p.Co) col[(size_t)(a * 16 + e) * TAPS * p.ci_total] = acc[a][j][e];
      }
    }
  }
  if (do_bias && (lane & 15) == 0) {
#pragma unroll
    for (int a = 0; a < NCF; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = co_base + a * 16 + (lane >> 4) * 4 + e;
        if (co < p.Co) p.pb[(size_t)sp * p.Co + co] = accb[a][e];
      }
  }
  WG2_STAMP();
  if (stamp) p.stamps[63] = nst;
#undef WG2_STAMP
}

template <int NCF, int NJW, int KS>
__global__ __launch_bounds__(256, 2) void wgrad_tile_kernel(Wg2P p) {
  wgrad_tile_body<NCF, NJW, KS>(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Horizontally batched form: ONE launch runs the workgroups of many independent weight-gradient problems of the same
// kernel variant.  The engine defers all weight gradients of a step to the end of the backward pass, where they are
// independent; most of them (everything below 48x48) fill a fraction of the CUs with one or two tiles per workgroup,
// i.e. they are latency chains.  Packed into one grid, every CU always holds workgroups of *some* problem.
// blocks[b] = {problem, split, channel window, co range}; problems are read through a uniform pointer (scalar loads).
template <int NCF, int NJW, int KS>
__global__ __launch_bounds__(256, 2) void wgrad_tile_batched_kernel(const Wg2P* __restrict__ probs, const int4* __restrict__ blocks, const int nblocks) {
  // gridDim.x < nblocks: a resident set of workgroups walks the block list (the engine caps the grid when the launch
  // runs in the background of the backward chain, so that the chain's kernels always find free CUs)
  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int4 bi = blocks[b];
    // BY VALUE: through a reference into global memory hipcc must re-read every field after each barrier / store (it cannot
    // prove the table is not written), and every such s_load waits on lgkmcnt, i.e. on all LDS traffic in flight
    const Wg2P p = probs[__builtin_amdgcn_readfirstlane(bi.x)];
    wgrad_tile_body<NCF, NJW, KS>(p, __builtin_amdgcn_readfirstlane(bi.y), __builtin_amdgcn_readfirstlane(bi.z),
                                  __builtin_amdgcn_readfirstlane(bi.w));
    __syncthreads();
  }
}

// All variants in ONE launch: a flush of the deferred weight gradients used to be up to 14 dependent launches (one per
// variant and LDS class), each with its own tail and, in the background of the backward chain, each a barrier packet on
// the side queue -- the rocprofv3 timeline showed the chain being dispatched only every ~60 us while those packets waited
// on each other.  Here every workgroup walks the common block list and runs the body its problem asks for.
__global__ __launch_bounds__(256, 2) void wgrad_tile_mega_kernel(const Wg2P* __restrict__ probs, const int4* __restrict__ blocks, const int nblocks) {
  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int4 bi = blocks[b];
    const Wg2P p = probs[__builtin_amdgcn_readfirstlane(bi.x)];  // by value (see the batched kernel)
    const int bx = __builtin_amdgcn_readfirstlane(bi.y), by = __builtin_amdgcn_readfirstlane(bi.z), bz = __builtin_amdgcn_readfirstlane(bi.w);
    switch (p.variant) {
      case 2: wgrad_tile_body<1, 16, 1>(p, bx, by, bz); break;
      case 3: wgrad_tile_body<1, 16, 3>(p, bx, by, bz); break;
      case 4: wgrad_tile_body<2, 12, 1>(p, bx, by, bz); break;
      case 5: wgrad_tile_body<2, 12, 3>(p, bx, by, bz); break;
      case 8: wgrad_tile_body<4, 6, 1>(p, bx, by, bz); break;
      case 9: wgrad_tile_body<4, 6, 3>(p, bx, by, bz); break;
      case 12: wgrad_tile_body<6, 4, 1>(p, bx, by, bz); break;
      case 13: wgrad_tile_body<6, 4, 3>(p, bx, by, bz); break;
      case 16: wgrad_tile_body<8, 3, 1>(p, bx, by, bz); break;
      case 33: wgrad_tile_body<1, 16, 7>(p, bx, by, bz); break;
      case 34: wgrad_tile_body<2, 16, 7>(p, bx, by, bz); break;
      case 36: wgrad_tile_body<2, 16, 1>(p, bx, by, bz); break;
      case 37: wgrad_tile_body<2, 16, 3>(p, bx, by, bz); break;
      default: wgrad_tile_body<8, 3, 3>(p, bx, by, bz); break;
    }
    __syncthreads();
  }
}

struct Wg2Geom { int ncf, njw, cwin, nsplit, tps, ntiles, tiles_x, tiles_y, n_cwin, n_co, dbuf; PixTile xt, gt; size_t lds; };

// returns false when the shape is not served by the tiled kernel
static bool wgrad2_geometry(int N, int H, int W, int co, int ctot8, int ks, Wg2Geom& g) {
  // tiny images waste most of a tile, but the packed launch still beats the generic kernel -- down to 1x1 images (round 2): the
  // 21 generic launches of ukbb192's 1x1-resolution layers sat in the exposed tail of the step (0.21 ms); packed: 16.89 vs 17.1 ms
  static const int min_hw = env_int("CGEN_WG2_MINHW", 1);
  if (!(ks == 1 || ks == 3 || ks == 7) || H < min_hw || W < min_hw) return false;
  const int taps = ks * ks;
  const int halo = ks / 2;
  g.ncf = co <= 16 ? 1 : (co <= 32 ? 2 : (co <= 64 ? 4 : (co <= 96 ? 6 : 8)));
  g.njw = g.ncf == 1 ? 16 : WG2_MAXACC / g.ncf;
  // The widest co block is not always the cheapest slab: the accumulators cap (co block) x (input-channel window), and every
  // window re-reads the gradient tile while every co block re-reads the input tile.  Pick the block width that moves the
  // fewest bytes per tile position (32 -> 160 @ 3x3: 128 + 32 co x two 16-channel windows = 151 KB; three 64-co blocks with
  // one 32-channel window = 82 KB).  A narrower block must save >= 10 %: it also means more LDS fragment reads per MFMA.
  static const int ncf_search = env_int("CGEN_WG2_NCF_SEARCH", 1);
  if (ncf_search && ks != 7) {
    // (co-block width in 16-column units, accumulator fragments per wave): the five standard slabs, plus a taller two-block
    // slab (32 fragments) that holds 112 input channels of a 3x3 conv in one window -- 96 -> 24 needs no second pass
    static const int cand[6][2] = {{1, 16}, {2, 12}, {2, 16}, {4, 6}, {6, 4}, {8, 3}};
    static const int tall = env_int("CGEN_WG2_TALL", 1);
    const int halo_ = ks / 2, c16_ = pad_to(ctot8, 16), co8 = pad_to(co, 8);
    const long xpix = (long)(TILE_H + 2 * halo_) * (TILE_W + 2 * halo_), gpix = (long)TILE_H * TILE_W;
    long best = -1, base = -1;
    int best_ncf = g.ncf, best_njw = g.njw;
    for (int k = 0; k < 6; ++k) {
      const int ncf = cand[k][0], njw = cand[k][1];
      if (ncf > g.ncf || (njw == 16 && ncf == 2 && !tall)) continue;
      const int mg = (4 * njw) / taps;
      if (mg < 1) continue;
      int cw = std::min(mg * 16, c16_);
      const PixTile gt = mk_pixtile(ncf * 16, 2, TILE_H, TILE_W);
      for (; cw >= 16; cw -= 16) {
        const PixTile xt = mk_pixtile(cw, 2, TILE_H + 2 * halo_, TILE_W + 2 * halo_);
        if (gt.ppp >= 1 && xt.ppp >= 1 && xt.bytes + gt.bytes <= 78 * 1024) break;
      }
      if (cw < 16) continue;
      const long n_cw = ceil_div(ctot8, cw), n_co = ceil_div(co, ncf * 16);
      const long bytes = n_co * n_cw * (xpix * std::min(cw, ctot8) * 2 + gpix * std::min(ncf * 16, co8) * 2);
      if (ncf == g.ncf && njw == g.njw) base = bytes;
      if (best < 0 || bytes < best) { best = bytes; best_ncf = ncf; best_njw = njw; }
    }
    static const int ncf_pct = env_int("CGEN_WG2_NCF_PCT", 90);
    if (base > 0 && (best_ncf != g.ncf || best_njw != g.njw) && best * 100 <= base * ncf_pct) {
      g.ncf = best_ncf;
      g.njw = best_njw;
    }
  }
  if (ks == 7) {  // the 7x7 stem (Cin <= 8: ONE 16-channel group, 49 taps -> 49 fragments = 13 per wave): at most 32 co columns per workgroup
    if (ctot8 > 16) return false;
    g.ncf = co <= 16 ? 1 : 2;
    g.njw = 16;
  }
  g.n_co = ceil_div(co, g.ncf * 16);
  int maxgrp = (4 * g.njw) / taps;  // 16-channel groups per window that fit the accumulators
  if (maxgrp < 1) return false;
  int cwin = maxgrp * 16;
  const int c16 = pad_to(ctot8, 16);
  if (cwin > c16) cwin = c16;
  g.gt = mk_pixtile(g.ncf * 16, 2, TILE_H, TILE_W);
  for (;; cwin -= 16) {  // LDS budget: two workgroups per CU
    if (cwin < 16) return false;
    g.xt = mk_pixtile(cwin, 2, TILE_H + 2 * halo, TILE_W + 2 * halo);
    if (g.gt.ppp >= 1 && g.xt.ppp >= 1 && g.xt.bytes + g.gt.bytes <= 78 * 1024) break;
  }
  if (g.gt.ppp < 1) return false;
  {  // equal windows: 96 channels as 48 + 48 rather than 80 + 16 -- same passes over the gradient tile, a smaller input tile
     // (which may make room for the second tile buffer) and workgroups of equal length.  Measured: the packed launches alone
     // 4.00 -> 3.88 ms, the STEP 1940 -> 1928 img/s (three interleaved pairs) -- off.
    static const int balance = env_int("CGEN_WG2_BALANCE", 0);
    const int nwin = ceil_div(ctot8, cwin);
    const int bal = pad_to(ceil_div(ctot8, nwin), 16);
    if (balance && nwin > 1 && bal < cwin) {
      cwin = bal;
      g.xt = mk_pixtile(cwin, 2, TILE_H + 2 * halo, TILE_W + 2 * halo);
    }
  }
  g.lds = (size_t)g.xt.bytes + g.gt.bytes;
  // two tile buffers where they fit next to a second workgroup on the CU: the next tile's DMA runs under this tile's MFMAs
  // (ablation on ukbb192: DMA-only 2.1 ms, MFMA-only ~1.6 ms, both 4.6 ms with one buffer -- the two phases did not overlap)
  static const int dbuf_on = env_int("CGEN_WG2_DBUF", 1);
  g.dbuf = (dbuf_on && 2 * g.lds <= 78 * 1024) ? 1 : 0;
  if (g.dbuf) g.lds *= 2;
  g.cwin = cwin;
  g.n_cwin = ceil_div(ctot8, cwin);
  g.tiles_x = ceil_div(W, TILE_W); g.tiles_y = ceil_div(H, TILE_H);
  g.ntiles = N * g.tiles_x * g.tiles_y;
  static const int want_total = env_int("CGEN_WG2_WANT", 32);  // (round 2: 160 -> 64 -> 32 workgroups per problem; with 16 tiles per workgroup: split-K partials 945 -> 429 MB per ukbb192 step, 1779 -> 1930 img/s overall)
  // workgroups per problem: the batched launch packs all problems of a step into one grid, so a problem need not fill
  // the chip by itself -- fewer, longer workgroups mean fewer split-K partials (measured optimum on MI355X: ~160 / >= 4 tiles)
  int want = ceil_div(want_total, g.n_cwin * g.n_co);
  {  // bound the split-K partials of one conv (they are written and re-read by cgen_wgrad_reduce)
    const char* e = getenv("CGEN_WG2_PARTIAL_MB");
    const long cap = (e ? atol(e) : 4096) << 20;  // off by default: capping costs more wgrad time than it saves in the reduce
    const long wbytes = 4L * co * taps * ctot8;
    const int maxs = (int)(cap / (wbytes > 0 ? wbytes : 1));
    if (want > maxs) want = maxs;
  }
  if (want < 1) want = 1;
  g.tps = ceil_div(g.ntiles, want);
  // long workgroups: the packed launch fills the chip whatever a single problem does, and every split costs a partial slab
  // (12 tiles per workgroup halves the split-K partials of ukbb192, 1.8 -> 0.94 GB per step, +1.7 %); the batch-256 32x32
  // models measured 1-2 % better with 4
  static const int min_tps_env = env_int("CGEN_WG2_MINTPS", 0);
  const int min_tps = min_tps_env > 0 ? min_tps_env : (N <= 64 ? 16 : 4);
  if (g.tps < min_tps && g.ntiles >= min_tps) g.tps = min_tps;
  g.nsplit = ceil_div(g.ntiles, g.tps);
  return true;
}

template <int NCF, int NJW>
static void launch_wgrad2_ks(const Wg2P& p, const Wg2Geom& g, hipStream_t st) {
  dim3 grid(g.nsplit, g.n_cwin, g.n_co), block(256);
  if (p.KS == 7) {
    if constexpr (NJW == 16 && NCF <= 2) {
      static bool once7 = false;
      if (!once7) { (void)hipFuncSetAttribute((const void*)wgrad_tile_kernel<NCF, 16, 7>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once7 = true; }
      hipLaunchKernelGGL((wgrad_tile_kernel<NCF, 16, 7>), grid, block, g.lds, st, p);
    }
    return;
  }
  if (p.KS == 3) {
    static bool once3 = false;
    if (!once3) { (void)hipFuncSetAttribute((const void*)wgrad_tile_kernel<NCF, NJW, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once3 = true; }
    hipLaunchKernelGGL((wgrad_tile_kernel<NCF, NJW, 3>), grid, block, g.lds, st, p);
  } else {
    static bool once1 = false;
    if (!once1) { (void)hipFuncSetAttribute((const void*)wgrad_tile_kernel<NCF, NJW, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once1 = true; }
    hipLaunchKernelGGL((wgrad_tile_kernel<NCF, NJW, 1>), grid, block, g.lds, st, p);
  }
}

template <typename T>
static int launch_wgrad(const WgP& p, const int ntc, hipStream_t st) {
  dim3 grid(p.nsplit, p.n_cichunks, ceil_div(p.Co, ntc * 16) * p.n_tapgroups), block(256);
  if (ntc == 1) hipLaunchKernelGGL((wgrad_kernel<T, 1>), grid, block, 0, st, p);
  else if (ntc == 2) hipLaunchKernelGGL((wgrad_kernel<T, 2>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((wgrad_kernel<T, 4>), grid, block, 0, st, p);
  return check_launch("cgen_conv2d_wgrad");
}

}  // namespace cgen

using namespace cgen;

static int count_chunks(const cgen_view* seg, int nseg) {
  int c = 0;
  for (int s = 0; s < nseg; ++s) c += (seg[s].c + 31) / 32;
  return c;
}

static int ctot8_of(const int32_t* seg_c, int nseg) {
  int c = 0;
  for (int s = 0; s < nseg; ++s) c += pad_to(seg_c[s], 8);
  return c;
}

// can the streaming tiled kernel serve this call?
static bool wgrad_tiled_ok(const cgen_wgrad_args* a, Wg2Geom& g) {
  if (a->dtype != CGEN_F16 || getenv("CGEN_WGRAD_GENERIC")) return false;
  if (!dma_clean(a->gout, 2)) return false;
  int segc[CGEN_MAX_SEG];
  for (int s = 0; s < a->nseg; ++s) {
    if (!dma_clean(a->seg[s], 2)) return false;
    segc[s] = a->seg[s].c;
  }
  // the kernel does its address arithmetic in 32 bits: every view must span less than 2^31 bytes (tile overhang included)
  auto fits = [&](const cgen_view& v) {
    const int64_t ext = (int64_t)a->n * v.sn + (int64_t)(a->h + TILE_H + a->ks) * v.sh + (int64_t)(a->w + TILE_W + a->ks) * v.sw + v.c;
    return ext * 2 < ((int64_t)1 << 31);
  };
  if (!fits(a->gout)) return false;
  for (int s = 0; s < a->nseg; ++s)
    if (!fits(a->seg[s])) return false;
  return wgrad2_geometry(a->n, a->h, a->w, a->gout.c, ctot8_of(segc, a->nseg), a->ks, g);
}

// Wg2P + geometry of one problem for the tiled bf16 kernel (false: not eligible, the caller uses the generic kernel)
static bool build_wg2(const cgen_wgrad_args* a, Wg2P& q, Wg2Geom& g) {
  if (!wgrad_tiled_ok(a, g)) return false;
  memset(&q, 0, sizeof(q));
  q.N = a->n; q.H = a->h; q.W = a->w; q.KS = a->ks; q.nseg = a->nseg; q.act = a->act; q.Co = a->gout.c; q.taps = a->ks * a->ks;
  int k8 = 0, o2 = 0;
  for (int s = 0; s < a->nseg; ++s) {
    q.seg[s] = mk(a->seg[s]); q.seg_koff[s] = k8; q.seg_off[s] = o2;
    k8 += pad_to(a->seg[s].c, 8); o2 += a->seg[s].c;
  }
  for (int s = a->nseg; s < CGEN_MAX_SEG; ++s) q.seg_koff[s] = 1 << 30;
  q.ci_total = o2;
  q.ctot8 = k8;
  q.gout = mk(a->gout);
  q.pw = a->partial_w; q.pb = a->partial_b;
  q.tiles_x = g.tiles_x; q.tiles_y = g.tiles_y; q.ntiles = g.ntiles; q.nsplit = g.nsplit; q.tiles_per_split = g.tps;
  q.cwin = g.cwin; q.cog = g.ncf * 16; q.xt = g.xt; q.gt = g.gt;
  q.d_tx = mk_fastdiv(g.tiles_x); q.d_ty = mk_fastdiv(g.tiles_y);
  q.variant = a->ks == 7 ? 32 + g.ncf : (g.ncf == 2 && g.njw == 16 ? 36 + (a->ks == 3 ? 1 : 0) : g.ncf * 2 + (a->ks == 3 ? 1 : 0));
  q.dbuf = g.dbuf;
  q.dbg = env_int("CGEN_WG2_DBG", 0);
  return true;
}

template <int NCF, int NJW>
static void launch_wgrad2_batched(int ks, const Wg2P* probs, const int4* blocks, int nblocks, int grid, size_t lds, hipStream_t st) {
  if (ks == 3) {
    static bool once3 = false;
    if (!once3) { (void)hipFuncSetAttribute((const void*)wgrad_tile_batched_kernel<NCF, NJW, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once3 = true; }
    hipLaunchKernelGGL((wgrad_tile_batched_kernel<NCF, NJW, 3>), dim3(grid), dim3(256), lds, st, probs, blocks, nblocks);
  } else {
    static bool once1 = false;
    if (!once1) { (void)hipFuncSetAttribute((const void*)wgrad_tile_batched_kernel<NCF, NJW, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once1 = true; }
    hipLaunchKernelGGL((wgrad_tile_batched_kernel<NCF, NJW, 1>), dim3(grid), dim3(256), lds, st, probs, blocks, nblocks);
  }
}

extern "C" int cgen_conv2d_wgrad_batch_plan(const cgen_wgrad_args* args, int32_t count, void* blob_host, int64_t capacity, int64_t* blob_bytes,
                                            cgen_wgrad_batch_launch* launches, int32_t max_launches, int32_t* n_launches, int32_t* eligible) {
  CGEN_REQUIRE(args && count >= 0 && blob_bytes && n_launches && eligible, "cgen_conv2d_wgrad_batch_plan: null args");
  struct Item { int idx; Wg2P q; Wg2Geom g; int key; long cost; };
  std::vector<Item> items;
  struct Item3 { int idx; Wg3Plan g; };
  std::vector<Item3> items3;  // problems of the streaming kernel (csrc/wgrad3.hip): their own launch, table and block list
  for (int i = 0; i < count; ++i) {
    Item it;
    it.idx = i;
    eligible[i] = 0;
    if (args[i].dtype != CGEN_F16 || !args[i].partial_w) continue;
    {
      Item3 i3;
      i3.idx = i;
      if (wg3_plan(&args[i], i3.g)) {
        if (i3.g.nsplit_total != args[i].nsplit) continue;
        eligible[i] = 1;
        items3.push_back(i3);
        continue;
      }
    }
    if (!build_wg2(&args[i], it.q, it.g)) continue;
    if (it.g.nsplit != args[i].nsplit) continue;
    eligible[i] = 1;
    // one launch per (variant, kernel size, LDS class): a big-LDS problem must not lower everyone's occupancy
    it.key = (it.g.ncf * 4 + (args[i].ks == 3 ? 1 : 0)) * 2 + (it.g.lds > 40 * 1024 ? 1 : 0);
    it.cost = (long)it.g.nsplit * it.g.n_cwin * it.g.n_co * it.g.tps;
    if (blob_host && getenv("CGEN_WG2_PLAN_DEBUG"))
      fprintf(stderr, "wg2 plan: %dx%dx%d ks%d ctot8 %3d co %3d | ncf %d cwin %3d n_cwin %d n_co %d | tiles %5d tps %3d nsplit %3d | lds %6zu dbuf %d | tile-visits %ld\n",
              args[i].n, args[i].h, args[i].w, args[i].ks, it.q.ctot8, it.q.Co, it.g.ncf, it.g.cwin, it.g.n_cwin, it.g.n_co, it.g.ntiles, it.g.tps,
              it.g.nsplit, it.g.lds, it.g.dbuf, (long)it.g.ntiles * it.g.n_cwin * it.g.n_co);
    items.push_back(it);
  }
  static const bool mega = [] { const char* e = getenv("CGEN_WGRAD_MEGA"); return !e || atoi(e) != 0; }();
  if (!mega) {  // the per-variant launches have no 7x7 instance: the stem goes to the caller's single launch
    std::vector<Item> keep;
    for (auto& it : items) { if (args[it.idx].ks == 7 || (it.g.ncf == 2 && it.g.njw == 16)) eligible[it.idx] = 0; else keep.push_back(it); }
    items.swap(keep);
  }
  if (mega) {  // one launch for everything: longest blocks first (the resident workgroups take them round robin)
    for (auto& it : items) {
      it.key = 0;
      it.cost = (long)it.g.tps * it.g.ncf * std::min(it.g.cwin, it.q.ctot8) * it.q.taps;
      // (a block's length is its DMA bytes, not its FLOPs: 1933 -> 1940 img/s in three interleaved pairs)
      static const int by_bytes = env_int("CGEN_WG2_SORT_BYTES", 1);
      if (by_bytes) it.cost = (long)it.g.tps * (long)(it.g.xt.bytes + it.g.gt.bytes);
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.key != b.key ? a.key < b.key : a.cost > b.cost; });
  const int64_t probs_bytes = pad_to((int)(items.size() * sizeof(Wg2P)), 256);
  int64_t nblocks_total = 0;
  for (auto& it : items) nblocks_total += (int64_t)it.g.nsplit * it.g.n_cwin * it.g.n_co;
  const int64_t old_bytes = pad_to((int)(probs_bytes + nblocks_total * (int64_t)sizeof(int4)), 256);
  // streaming-kernel section: [Wg3P table][one int4 per workgroup], longest blocks first
  std::stable_sort(items3.begin(), items3.end(), [](const Item3& a, const Item3& b) { return a.g.block_bytes > b.g.block_bytes; });
  const int64_t probs3_bytes = pad_to((int)(items3.size() * sizeof(Wg3P)), 256);
  int64_t nblocks3 = 0;
  for (auto& it : items3) nblocks3 += it.g.nblocks;
  *blob_bytes = old_bytes + (items3.empty() ? 0 : probs3_bytes + nblocks3 * (int64_t)sizeof(int4));
  int nl = 0;
  for (size_t i = 0; i < items.size(); ++i)
    if (i == 0 || items[i].key != items[i - 1].key) ++nl;
  if (!items3.empty()) ++nl;
  *n_launches = nl;
  if (!blob_host) return CGEN_OK;  // size query
  CGEN_REQUIRE(capacity >= *blob_bytes && launches && max_launches >= nl, "cgen_conv2d_wgrad_batch_plan: buffers too small");
  memset(blob_host, 0, (size_t)*blob_bytes);
  Wg2P* probs = (Wg2P*)blob_host;
  int4* blocks = (int4*)((char*)blob_host + probs_bytes);
  int64_t b = 0;
  int li = -1;
  for (size_t i = 0; i < items.size(); ++i) {
    const Item& it = items[i];
    probs[i] = it.q;
    if (i == 0 || it.key != items[i - 1].key) {
      ++li;
      launches[li].ncf = mega ? 0 : it.g.ncf; launches[li].ks = args[it.idx].ks; launches[li].lds_bytes = 0; launches[li].nblocks = 0;
      launches[li].blocks_offset = probs_bytes + b * (int64_t)sizeof(int4);
    }
    if ((int32_t)it.g.lds > launches[li].lds_bytes) launches[li].lds_bytes = (int32_t)it.g.lds;
    for (int z = 0; z < it.g.n_co; ++z)
      for (int y = 0; y < it.g.n_cwin; ++y)
        for (int x = 0; x < it.g.nsplit; ++x) { blocks[b] = make_int4((int)i, x, y, z); ++b; }
    launches[li].nblocks += it.g.nsplit * it.g.n_cwin * it.g.n_co;
  }
  if (!items3.empty()) {
    // The block list interleaves the problems: block k of every problem before block k + 1 of any (each problem's blocks are
    // equally long; problems sorted longest first), so the resident workgroups start on the long problems and the tail is short.
    Wg3P* probs3 = (Wg3P*)((char*)blob_host + old_bytes);
    int4* blocks3 = (int4*)((char*)blob_host + old_bytes + probs3_bytes);
    ++li;
    launches[li].ncf = -3; launches[li].ks = (int32_t)items3.size(); launches[li].lds_bytes = 0; launches[li].nblocks = (int32_t)nblocks3;
    launches[li].blocks_offset = old_bytes + probs3_bytes;
    int64_t b3 = 0;
    int maxb = 0;
    for (size_t i = 0; i < items3.size(); ++i) {
      probs3[i] = items3[i].g.q;
      probs3[i].pw = args[items3[i].idx].partial_w; probs3[i].pb = args[items3[i].idx].partial_b;
      if ((int32_t)items3[i].g.lds > launches[li].lds_bytes) launches[li].lds_bytes = (int32_t)items3[i].g.lds;
      maxb = std::max(maxb, items3[i].g.nblocks);
    }
    // Block order = start order (the final flush launches one workgroup per block, the background flush walks the list with a
    // resident set): LONGEST FIRST over all blocks, by estimated duration -- bytes over the rate the problem's image side streams at
    // (tools/bench_wgrad3.py batch: >= 96^2 ~4 TB/s, 48^2 ~3, 24^2 ~1.4, 12^2 and below ~0.9).  The first version dealt the
    // problems round-robin (block k of every problem, k = 0, 1, ...): the list then ENDED with blocks 30..63 of the dozen 192^2
    // problems alone, ~300 of the longest blocks on a half-empty chip, and the launch took 2.5 ms whatever the kernel's speed.
    if (getenv("CGEN_WG3_ORDER") && atoi(getenv("CGEN_WG3_ORDER")) == 0) {
      for (int k = 0; k < maxb; ++k)
        for (size_t i = 0; i < items3.size(); ++i) {
          const Wg3P& q3 = items3[i].g.q;
          if (k < items3[i].g.nblocks) { const int w = k / q3.nsplit; blocks3[b3] = make_int4((int)i, k % q3.nsplit, w % q3.n_pwin, w / q3.n_pwin); ++b3; }
        }
    } else {
      struct Ord { double cost; int i, k; };
      std::vector<Ord> ord;
      ord.reserve((size_t)nblocks3);
      for (size_t i = 0; i < items3.size(); ++i) {
        const Wg3P& q3 = items3[i].g.q;
        const int side = std::min(q3.H, q3.W);
        const double slow = side >= 96 ? 1.0 : side >= 48 ? 1.35 : side >= 24 ? 2.9 : 4.5;
        // the last split of a problem may be short: tiles of split s
        for (int k = 0; k < items3[i].g.nblocks; ++k) {
          const int sp = k % q3.nsplit;
          const int nt = std::min(q3.tps, q3.ntiles - sp * q3.tps);
          ord.push_back({(double)items3[i].g.block_bytes * slow * (double)nt / (double)q3.tps, (int)i, k});
        }
      }
      std::stable_sort(ord.begin(), ord.end(), [](const Ord& a, const Ord& b) { return a.cost > b.cost; });
      for (const Ord& o : ord) {
        const Wg3P& q3 = items3[o.i].g.q;
        const int w = o.k / q3.nsplit;
        blocks3[b3] = make_int4(o.i, o.k % q3.nsplit, w % q3.n_pwin, w / q3.n_pwin); ++b3;
      }
    }
  }
  return CGEN_OK;
}

extern "C" int cgen_conv2d_wgrad_batch_run(const void* blob_dev, const cgen_wgrad_batch_launch* launches, int32_t n_launches, int32_t max_workgroups,
                                           cgen_stream_t stream) {
  CGEN_REQUIRE(blob_dev && (launches || n_launches == 0) && n_launches >= 0, "cgen_conv2d_wgrad_batch_run: null args");
  hipStream_t st = (hipStream_t)stream;
  const Wg2P* probs = (const Wg2P*)blob_dev;
  for (int i = 0; i < n_launches; ++i) {
    const cgen_wgrad_batch_launch& l = launches[i];
    if (l.nblocks <= 0) continue;
    const int4* blocks = (const int4*)((const char*)blob_dev + l.blocks_offset);
    const int grid = max_workgroups > 0 ? std::min(l.nblocks, max_workgroups) : l.nblocks;
    switch (l.ncf) {
      case -3: {  // streaming kernel: l.ks problems, their table right in front of the block list
        const int64_t probs3_bytes = pad_to((int)(l.ks * sizeof(Wg3P)), 256);
        wg3_launch_mega((const Wg3P*)((const char*)blob_dev + l.blocks_offset - probs3_bytes), blocks, l.nblocks, grid, (size_t)l.lds_bytes, st);
        break;
      }
      case 0: {
        static bool once = false;
        if (!once) { (void)hipFuncSetAttribute((const void*)wgrad_tile_mega_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once = true; }
        hipLaunchKernelGGL(wgrad_tile_mega_kernel, dim3(grid), dim3(256), (size_t)l.lds_bytes, st, probs, blocks, l.nblocks);
        break;
      }
      case 1: launch_wgrad2_batched<1, 16>(l.ks, probs, blocks, l.nblocks, grid, (size_t)l.lds_bytes, st); break;
      case 2: launch_wgrad2_batched<2, 12>(l.ks, probs, blocks, l.nblocks, grid, (size_t)l.lds_bytes, st); break;
      case 4: launch_wgrad2_batched<4, 6>(l.ks, probs, blocks, l.nblocks, grid, (size_t)l.lds_bytes, st); break;
      case 6: launch_wgrad2_batched<6, 4>(l.ks, probs, blocks, l.nblocks, grid, (size_t)l.lds_bytes, st); break;
      case 8: launch_wgrad2_batched<8, 3>(l.ks, probs, blocks, l.nblocks, grid, (size_t)l.lds_bytes, st); break;
      default: return cgen::fail(CGEN_EINVAL, "cgen_conv2d_wgrad_batch_run: bad variant %d", l.ncf);
    }
  }
  return check_launch("cgen_conv2d_wgrad_batch_run");
}

// The launch decision, made ONCE per call: cgen_conv2d_wgrad launches from this record, cgen_conv2d_wgrad_plan and
// cgen_conv2d_wgrad_plan_record report it.  Host code: nothing is dereferenced.
struct WgradDecision {
  int kind, nsplit;  // kind as cgen_conv2d_wgrad_plan names it: 0 generic, 1 tiled, 2 / 3 streaming (partial layout 0 / 1)
  Wg3Plan g3;        // kinds 2, 3
  Wg2P q2;           // kind 1
  Wg2Geom g2;
  WgP p;             // kind 0
  int ntc, esz;
};

static void wgrad_decide(const cgen_wgrad_args* a, WgradDecision& d) {
  if (wg3_plan(a, d.g3)) {  // streaming kernel of round 5 (csrc/wgrad3.hip) where it serves the shape
    d.kind = 2 + d.g3.q.layout;
    d.nsplit = d.g3.nsplit_total;
    return;
  }
  if (build_wg2(a, d.q2, d.g2)) {  // tiled bf16 kernel when the shape allows it
    d.kind = 1;
    d.nsplit = d.g2.nsplit;
    return;
  }
  d.kind = 0;
  d.esz = a->dtype == CGEN_F32 ? 4 : 2;
  WgP& p = d.p;
  memset(&p, 0, sizeof(p));
  p.N = a->n; p.H = a->h; p.W = a->w; p.KS = a->ks; p.pad = a->ks / 2; p.nseg = a->nseg; p.act = a->act;
  p.Co = a->gout.c; p.P = a->n * a->h * a->w; p.taps = a->ks * a->ks;
  int off = 0, ch = 0;
  for (int s = 0; s < a->nseg; ++s) {
    p.seg[s] = mk(a->seg[s]);
    p.seg_off[s] = off;
    p.seg_vec[s] = vec16_ok(a->seg[s], d.esz);
    p.seg_chunk0[s] = ch;
    off += a->seg[s].c;
    ch += (a->seg[s].c + 31) / 32;
  }
  p.seg_chunk0[a->nseg] = ch;
  p.ci_total = off;
  p.n_cichunks = ch;
  p.n_tapgroups = ceil_div(p.taps, WG_MAXT);
  wgrad_geometry(p.P, p.Co, (p.ci_total + 31) / 32, p.KS, p.nsplit, p.pix_per_split);
  d.nsplit = p.nsplit;
  d.ntc = wgrad_ntc(p.Co);
  p.gout = mk(a->gout);
  {
    const int q = 4 * d.esz;
    p.gout_vec = ((uintptr_t)a->gout.p % q == 0) && ((a->gout.sn * d.esz) % q == 0) && ((a->gout.sh * d.esz) % q == 0) && ((a->gout.sw * d.esz) % q == 0);
  }
  p.pw = a->partial_w; p.pb = a->partial_b;
}

extern "C" int cgen_conv2d_wgrad_plan(const cgen_wgrad_args* a, int32_t* tiled_out) {
  if (!a || a->nseg < 1 || a->nseg > CGEN_MAX_SEG) return 0;
  WgradDecision d;
  wgrad_decide(a, d);
  if (tiled_out) *tiled_out = d.kind;
  return d.nsplit;
}

extern "C" int cgen_conv2d_wgrad_plan_record(const cgen_wgrad_args* a, int32_t* out) {
  if (!a || a->nseg < 1 || a->nseg > CGEN_MAX_SEG) return 0;
  WgradDecision d;
  wgrad_decide(a, d);
  if (out) {
    for (int i = 0; i < CGEN_WGRAD_PLAN_INTS; ++i) out[i] = 0;
    out[0] = d.kind; out[1] = d.nsplit;
    if (d.kind == 0) {
      const WgP& p = d.p;
      int mask = 0;
      for (int s = 0; s < p.nseg; ++s) mask |= (p.seg_vec[s] ? 1 : 0) << s;
      out[2] = a->dtype; out[3] = d.ntc; out[4] = p.n_cichunks; out[5] = p.n_tapgroups; out[6] = p.pix_per_split;
      out[7] = p.gout_vec; out[8] = mask; out[9] = p.pb ? 1 : 0;
    } else if (d.kind == 1) {
      const Wg2Geom& g = d.g2;
      out[2] = g.ncf; out[3] = g.njw; out[4] = d.q2.KS; out[5] = g.cwin; out[6] = g.n_cwin; out[7] = g.n_co; out[8] = g.ntiles;
      out[9] = g.tps; out[10] = g.dbuf; out[11] = (int32_t)g.lds; out[12] = d.q2.variant;
    }
  }
  return d.nsplit;
}

extern "C" int cgen_conv2d_wgrad(const cgen_wgrad_args* a, cgen_stream_t stream) {
  CGEN_REQUIRE(a && a->partial_w, "cgen_conv2d_wgrad: null args");
  CGEN_REQUIRE(a->dtype == CGEN_F32 || a->dtype == CGEN_F16, "cgen_conv2d_wgrad: bad dtype");
  CGEN_REQUIRE(a->nseg >= 1 && a->nseg <= CGEN_MAX_SEG && a->gout.p && a->gout.c > 0, "cgen_conv2d_wgrad: bad args");
  WgradDecision d;
  wgrad_decide(a, d);
  // geometry must match what the caller sized the partial buffer with
  CGEN_REQUIRE(d.nsplit == a->nsplit, "cgen_conv2d_wgrad: nsplit %d != expected %d", a->nsplit, d.nsplit);
  hipStream_t st = (hipStream_t)stream;
  if (d.kind >= 2) {
    wg3_launch_single(d.g3, st);
    return check_launch("cgen_conv2d_wgrad(stream)");
  }
  if (d.kind == 1) {
    Wg2P& q = d.q2;
    const Wg2Geom& g = d.g2;
    { const char* e = getenv("CGEN_WG2_STAMPS"); q.stamps = e ? (unsigned long long*)strtoull(e, nullptr, 0) : nullptr; }
    switch (g.ncf) {
      case 1: launch_wgrad2_ks<1, 16>(q, g, st); break;
      case 2: if (a->ks == 7 || g.njw == 16) launch_wgrad2_ks<2, 16>(q, g, st); else launch_wgrad2_ks<2, 12>(q, g, st); break;
      case 4: launch_wgrad2_ks<4, 6>(q, g, st); break;
      case 6: launch_wgrad2_ks<6, 4>(q, g, st); break;
      default: launch_wgrad2_ks<8, 3>(q, g, st); break;
    }
    return check_launch("cgen_conv2d_wgrad(tile)");
  }
  return a->dtype == CGEN_F32 ? launch_wgrad<float>(d.p, d.ntc, st) : launch_wgrad<h16_t>(d.p, d.ntc, st);
}
