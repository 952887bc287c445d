// Backward latent tail of a stochastic decoder layer in ONE launch (binary16): include/cgen_hip.h, cgen_latent_tail_bwd.
// (Its forward mirror image, cgen_latent_tail_fwd, is the second half of this file.)
//
// What it replaces ran as a strict chain of four launches per layer -- the two data gradients of z_feat_proj, the data gradient
// of z_proj (accumulating into grad(z)) and the reparameterisation backward that reads grad(z) back, with the residual copy into
// grad(p_feat) as its rider: four load -> compute -> store round trips for three 1x1 GEMMs with K <= 192 and a formula.
// Here the chain is ONE round trip:
//   * all convs are 1x1 and every view is linear in pixels, so the problem is [P pixels] x [channels]; a lane of an
//     MFMA 16x16x32 B operand is 8 consecutive channels of one pixel = one 16-byte global load, so the gradient tiles go from
//     memory straight into registers (no LDS staging, no barrier per tile) and every load of a tile -- GEMM operands AND
//     epilogue operands -- is requested up front, in one batch;
//   * the weight slab of the workgroup's output rows is composed in LDS once per launch from the data-gradient images
//     cgen_weight_prep writes anyway; rows are permuted inside each 32-row block as in conv_px_kernel, so a lane ends up with
//     8 CONSECUTIVE output channels of its pixel: the reparam body (latent_bodies.inc) applies to the accumulators as is and
//     every result leaves as one 16-byte store (by default after the roundings the four launches applied on the way: ORDER below);
//   * gridDim.y splits the output rows: part 0 owns g_z (K = g_f.c + C, never stored) and runs the reparam epilogue, parts
//     1.. own LT_NP 32-channel blocks of g_pfeat each (K = g_f.c; the identity G_h -> g_pfeat is an add in the epilogue).
// Both entry points also take a DETERMINISTIC layer (z = p_loc; called without q_loc / q_ls): DET instances of the same bodies,
// kernels of their own (latent_tail_det1_bwd_kernel: one workgroup row, C <= 64; latent_tail_det_bwd_kernel; latent_tail_det_fwd_kernel).
#include <stdlib.h>

#include "common.h"
#include "latent_bodies.inc"

#ifdef CGEN_NO_SETPRIO
#define CGEN_SETPRIO() do {} while (0)
#else
#define CGEN_SETPRIO() __builtin_amdgcn_s_setprio(3)
#endif

namespace cgen {

#define LT_MAXKF 6   // K-steps of 32 channels per gradient tensor the widest instance holds: C, g_f.c <= 192
#define LT_NP 2      // 32-channel blocks of g_pfeat per workgroup
#define LT_PX 64     // pixels per tile: 16 per wave

__device__ uint4 g_lt_zero[1];  // 16 bytes of zeros: the address an absent or out-of-range epilogue operand is loaded from

struct LtP {
  int P, hw, Z, C, Cf;
  int nks_f, nks_h;      // K-steps over G_f / G_h
  int ntiles;
  int krow_f, krow_p;    // row lengths of the z_feat_proj / z_proj data-gradient images
  int s_gh, s_gf, s_gz, s_ql, s_qs, s_pl, s_ps, s_z, s_op, s_oq;  // pixel strides (elements)
  const h16_t *g_h, *g_f, *gz_in, *q_loc, *q_ls, *p_loc, *p_ls, *z;
  h16_t *out_p, *out_q;
  const h16_t *img_fz, *img_fp, *img_pz;
  const float *coef, *chan_scale;
  int coef_stride, acc_q, acc_p;
  float logt;
};

__device__ __forceinline__ uint4 lt_ld(const h16_t* base, int off, bool ok) {
  // unconditional load from a selected address (vmcnt is in order: a skipped load would change every later wait count)
  return *(const uint4*)(ok ? (const void*)(base + off) : (const void*)g_lt_zero);
}
__device__ __forceinline__ h16x8 lt_frag(uint4 v) {
  union { uint4 u; h16x8 h; } c;
  c.u = v;
  return c.h;
}

__device__ __forceinline__ float lt_r16(float v) { return h2f(f2h(v)); }  // what a binary16 store followed by a load leaves of v
// the partial sums of the small-image conv kernel's four waves, added in its order: ((w0 + w1) + w2) + w3
template <int NPART>
__device__ __forceinline__ f32x4_t lt_sum(const f32x4_t (&a)[NPART][2], int h) {
  f32x4_t v = a[0][h];
#pragma unroll
  for (int w = 1; w < NPART; ++w) { v[0] += a[w][h][0]; v[1] += a[w][h][1]; v[2] += a[w][h][2]; v[3] += a[w][h][3]; }
  return v;
}

// ORDER -- the arithmetic between the MFMAs and the stores (cgen_latent_tail_bwd_args.parity):
//   0: one f32 sum per output over all its terms, one rounding (closest to exact);
//   1 / 2: what the four launches compute, bit for bit: every GEMM summed on its own in the order of the data-gradient kernel that
//      serves the shape (1: conv_px, K-steps in sequence; 2: conv_smallp, K-step i in partial i % 4, the partials added in wave
//      order) and rounded to binary16 wherever that path stores a tensor: grad(z) after each of its two writers, grad(p_feat) before
//      the residual is added.
// ---- part 0: g_z = [W_f[:, :Z]^T | W_p[:, :Z]^T] [G_f ; G_h] (+ gz_in) in registers, then the reparam / KL backward
// DET: the layer is deterministic (z = p_loc; no reparam entry, no posterior): g_z IS grad(p_loc), the p_ls channels of out_p leave as
// zeros (nobody else writes them: the launch owns the whole 2Z + C pixel) and nothing of the reparam operands is loaded.
template <int MAXKF, bool ACC, int ORDER, bool DET = false>
__device__ __forceinline__ void lt_run_z(const LtP& p, char* smem) {
  static_assert(!(DET && ACC), "the deterministic tail does not accumulate");
  constexpr int NPART = ORDER == 2 ? 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int nks = p.nks_f + p.nks_h, K = nks * 32, ldw = K + 8, Kf = p.nks_f * 32;
  const int ch = fg * 8;            // this lane's z channels ch .. ch + 8
  const bool live = ch < p.Z;       // (lane groups past Z hold the zero rows of the 32-row block)
  const bool has_gz = ACC && p.gz_in != nullptr;

  uint4 xf[MAXKF], xh[MAXKF], ql, qs, pl, ps, zv, gzi, pq1, pq2, pp1, pp2;
  int px = 0;
  bool ok = false;
  auto request = [&](int t) {
    px = t * LT_PX + wave * 16 + fr;
    const bool inside = px < p.P;
    const int pc = inside ? px : p.P - 1;  // (a lane past the last pixel multiplies the last pixel again; nothing of it is stored)
    ok = inside && live;
#pragma unroll
    for (int i = 0; i < MAXKF; ++i) {
      if (i < p.nks_f) xf[i] = *(const uint4*)(p.g_f + (pc * p.s_gf + i * 32 + ch));
    }
#pragma unroll
    for (int i = 0; i < MAXKF; ++i) {
      if (i < p.nks_h) xh[i] = *(const uint4*)(p.g_h + (pc * p.s_gh + i * 32 + ch));
    }
    if constexpr (!DET) {
      ql = lt_ld(p.q_loc, pc * p.s_ql + ch, ok); qs = lt_ld(p.q_ls, pc * p.s_qs + ch, ok);
      pl = lt_ld(p.p_loc, pc * p.s_pl + ch, ok); ps = lt_ld(p.p_ls, pc * p.s_ps + ch, ok);
      zv = lt_ld(p.z, pc * p.s_z + ch, ok);
    }
    if constexpr (ACC) {  // (the instance without them keeps 20 registers fewer: one more workgroup per CU)
      gzi = lt_ld(p.gz_in, pc * p.s_gz + ch, ok && has_gz);
      pq1 = lt_ld(p.out_q, pc * p.s_oq + ch, ok && p.acc_q); pq2 = lt_ld(p.out_q, pc * p.s_oq + p.Z + ch, ok && p.acc_q);
      pp1 = lt_ld(p.out_p, pc * p.s_op + ch, ok && p.acc_p); pp2 = lt_ld(p.out_p, pc * p.s_op + p.Z + ch, ok && p.acc_p);
    }
  };
  int t = (int)blockIdx.x;
  request(t);
  // ---- weight slab, once: LDS row h * 16 + j holds z channel (j >> 2) * 8 + h * 4 + (j & 3) (zeros past Z): MFMA h then leaves
  // channels 8 fg + 4 h + {0..3} in lane group fg.  Columns [0, Kf) from z_feat_proj's image, [Kf, K) from z_proj's.
  {
    const int gpr = K >> 3;
    for (int g = tid; g < 32 * gpr; g += 256) {
      const int r = g / gpr, k = (g - r * gpr) * 8;
      const int h = r >> 4, j = r & 15, c = (j >> 2) * 8 + h * 4 + (j & 3);
      const h16_t* src = k < Kf ? p.img_fz + (c * p.krow_f + k) : p.img_pz + (c * p.krow_p + (k - Kf));
      *(uint4*)(smem + (r * ldw + k) * 2) = lt_ld(src, 0, c < p.Z);
    }
  }
  __syncthreads();
  const char* a_base = smem + (fr * ldw + fg * 8) * 2;
  const char* a_base_h = a_base + Kf * 2;
  for (;;) {
    f32x4_t aF[NPART][2], aH[NPART][2];
#pragma unroll
    for (int w = 0; w < NPART; ++w) aF[w][0] = aF[w][1] = aH[w][0] = aH[w][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MAXKF; ++i) {
      if (i < p.nks_f) {  // (uniform)
        const h16x8 b = lt_frag(xf[i]);
        aF[i % NPART][0] = mfma_h16(*(const h16x8*)(a_base + i * 64), b, aF[i % NPART][0], 0, 0, 0);
        aF[i % NPART][1] = mfma_h16(*(const h16x8*)(a_base + (16 * ldw) * 2 + i * 64), b, aF[i % NPART][1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXKF; ++i) {
      if (i < p.nks_h) {  // (uniform; ORDER 0 goes on with the one sum)
        const h16x8 b = lt_frag(xh[i]);
        f32x4_t(&a)[2] = ORDER == 0 ? aF[0] : aH[i % NPART];
        a[0] = mfma_h16(*(const h16x8*)(a_base_h + i * 64), b, a[0], 0, 0, 0);
        a[1] = mfma_h16(*(const h16x8*)(a_base_h + (16 * ldw) * 2 + i * 64), b, a[1], 0, 0, 0);
      }
    }
    if (ok) {
      float gz[8], fql[8], fqs[8], fpl[8], fps[8], fz[8], o1[8], o2[8], o3[8], o4[8], tp[8];
      if (has_gz) unpack8(gzi, tp);
      if constexpr (ORDER == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { gz[e] = aF[0][0][e]; gz[4 + e] = aF[0][1][e]; }
        if (has_gz) {
#pragma unroll
          for (int e = 0; e < 8; ++e) gz[e] += tp[e];
        }
      } else {
        const f32x4_t f0 = lt_sum<NPART>(aF, 0), f1 = lt_sum<NPART>(aF, 1), h0 = lt_sum<NPART>(aH, 0), h1 = lt_sum<NPART>(aH, 1);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float zf = e < 4 ? f0[e & 3] : f1[e & 3], zh = e < 4 ? h0[e & 3] : h1[e & 3];
          if (p.nks_f) gz[e] = lt_r16(zh + (has_gz ? lt_r16(zf + tp[e]) : lt_r16(zf)));  // z_feat_proj's data gradient wrote grad(z), z_proj's added to it
          else gz[e] = has_gz ? lt_r16(zh + tp[e]) : lt_r16(zh);
        }
      }
      if constexpr (DET) {  // grad(p_loc) = g_z (already rounded as the launches round it), grad(p_ls) = 0
        *(uint4*)(p.out_p + (px * p.s_op + ch)) = pack8(gz);
        *(uint4*)(p.out_p + (px * p.s_op + p.Z + ch)) = make_uint4(0, 0, 0, 0);
      } else {
        unpack8(ql, fql); unpack8(qs, fqs); unpack8(pl, fpl); unpack8(ps, fps); unpack8(zv, fz);
        const int b = px / p.hw;
        const float k0 = p.coef[(int64_t)b * p.coef_stride];
        reparam_kl_bwd_vec8_math(k0, p.chan_scale, ch, p.logt, true, fql, fqs, fpl, fps, gz, fz, o1, o2, o3, o4);
        if (ACC && p.acc_q) {
          unpack8(pq1, tp);
#pragma unroll
          for (int e = 0; e < 8; ++e) o1[e] += tp[e];
          unpack8(pq2, tp);
#pragma unroll
          for (int e = 0; e < 8; ++e) o2[e] += tp[e];
        }
        if (ACC && p.acc_p) {
          unpack8(pp1, tp);
#pragma unroll
          for (int e = 0; e < 8; ++e) o3[e] += tp[e];
          unpack8(pp2, tp);
#pragma unroll
          for (int e = 0; e < 8; ++e) o4[e] += tp[e];
        }
        *(uint4*)(p.out_q + (px * p.s_oq + ch)) = pack8(o1);
        *(uint4*)(p.out_q + (px * p.s_oq + p.Z + ch)) = pack8(o2);
        *(uint4*)(p.out_p + (px * p.s_op + ch)) = pack8(o3);
        *(uint4*)(p.out_p + (px * p.s_op + p.Z + ch)) = pack8(o4);
      }
    }
    t += (int)gridDim.x;
    if (t >= p.ntiles) break;
    request(t);
  }
}

// ---- parts 1..: g_pfeat[32 (pr0 + pr) ..] = G_h + W_f[:, Z:]^T G_f for LT_NP 32-channel blocks
template <int MAXKF, bool ACC, int ORDER>
__device__ __forceinline__ void lt_run_p(const LtP& p, char* smem) {
  constexpr int NPART = ORDER == 2 ? 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int nks = p.nks_f, K = nks * 32, ldw = K + 8;
  const int c0 = ((int)blockIdx.y - 1) * (LT_NP * 32) + fg * 8;  // this lane's channels c0 + 32 pr .. + 8
  const int o0 = 2 * p.Z + c0;

  uint4 xf[MAXKF], gh[LT_NP], pv[LT_NP];
  int px = 0;
  bool ok[LT_NP];
  auto request = [&](int t) {
    px = t * LT_PX + wave * 16 + fr;
    const bool inside = px < p.P;
    const int pc = inside ? px : p.P - 1;
#pragma unroll
    for (int i = 0; i < MAXKF; ++i) {
      if (i < nks) xf[i] = *(const uint4*)(p.g_f + (pc * p.s_gf + i * 32 + fg * 8));
    }
#pragma unroll
    for (int pr = 0; pr < LT_NP; ++pr) {
      ok[pr] = inside && c0 + pr * 32 < p.C;  // (C is a multiple of 32: a block is inside or outside as a whole)
      gh[pr] = lt_ld(p.g_h, pc * p.s_gh + c0 + pr * 32, ok[pr]);
      if constexpr (ACC) pv[pr] = lt_ld(p.out_p, pc * p.s_op + o0 + pr * 32, ok[pr] && p.acc_p);
    }
  };
  int t = (int)blockIdx.x;
  request(t);
  // ---- weight slab, once: LDS row pr * 32 + h * 16 + j holds p_feat channel 32 (pr0 + pr) + (j >> 2) * 8 + h * 4 + (j & 3)
  {
    const int gpr = K >> 3, cb = ((int)blockIdx.y - 1) * (LT_NP * 32);
    for (int g = tid; g < LT_NP * 32 * gpr; g += 256) {
      const int r = g / gpr, k = (g - r * gpr) * 8;
      const int pr = r >> 5, h = (r >> 4) & 1, j = r & 15, c = cb + pr * 32 + (j >> 2) * 8 + h * 4 + (j & 3);
      *(uint4*)(smem + (r * ldw + k) * 2) = lt_ld(p.img_fp, c * p.krow_f + k, c < p.C);
    }
  }
  __syncthreads();
  const char* a_base = smem + (fr * ldw + fg * 8) * 2;
  for (;;) {
    f32x4_t acc[LT_NP][NPART][2];
#pragma unroll
    for (int pr = 0; pr < LT_NP; ++pr)
#pragma unroll
      for (int w = 0; w < NPART; ++w) acc[pr][w][0] = acc[pr][w][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MAXKF; ++i) {
      if (i < nks) {  // (uniform)
        const h16x8 b = lt_frag(xf[i]);
#pragma unroll
        for (int pr = 0; pr < LT_NP; ++pr)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            acc[pr][i % NPART][h] = mfma_h16(*(const h16x8*)(a_base + ((pr * 32 + h * 16) * ldw) * 2 + i * 64), b, acc[pr][i % NPART][h], 0, 0, 0);
      }
    }
#pragma unroll
    for (int pr = 0; pr < LT_NP; ++pr) {
      if (!ok[pr]) continue;
      float v[8], tp[8];
      const bool accp = ACC && p.acc_p;
      const f32x4_t s0 = lt_sum<NPART>(acc[pr], 0), s1 = lt_sum<NPART>(acc[pr], 1);
      unpack8(gh[pr], v);
      if (accp) unpack8(pv[pr], tp);
      if constexpr (ORDER == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += e < 4 ? s0[e & 3] : s1[e & 3];
        if (accp) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += tp[e];
        }
      } else if (nks) {  // z_feat_proj's data gradient wrote (or added to) grad(p_feat), then the residual's copy of G_h was added
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = e < 4 ? s0[e & 3] : s1[e & 3];
          v[e] += accp ? lt_r16(f + tp[e]) : lt_r16(f);
        }
      } else if (accp) {  // no z_feat_proj: G_h is copied (its bits kept) or added
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += tp[e];
      }
      *(uint4*)(p.out_p + (px * p.s_op + o0 + pr * 32)) = pack8(v);
    }
    t += (int)gridDim.x;
    if (t >= p.ntiles) break;
    request(t);
  }
}

// MAXKF: K-steps per gradient tensor the kernel is compiled for (the fragments live in registers): 4 serves C, g_f.c <= 128 --
// ukbb192's layers of 24x24 and above -- 6 the widest.  ACC: out_p / out_q are accumulated into or gz_in is present; the previous
// values are five more epilogue operands in registers.  Without them the sequential orders fit 128 registers (four workgroups
// per CU, which the grid below counts on), with them 168 (three); the four-partial order (small images: few workgroups) two.
template <int MAXKF, bool ACC, int ORDER>
__global__ __launch_bounds__(256, ORDER == 2 ? 2 : (ACC ? 3 : 4)) void latent_tail_bwd_kernel(LtP p) {
  CGEN_SETPRIO();  // the chain's waves win issue arbitration over background weight-gradient waves on the same SIMD
  extern __shared__ __attribute__((aligned(16))) char lt_smem[];
  if (blockIdx.y == 0) lt_run_z<MAXKF, ACC, ORDER>(p, lt_smem);
  else lt_run_p<MAXKF, ACC, ORDER>(p, lt_smem);
}

// ---- the deterministic layer with C, g_f.c <= 64 (every preset's) in ONE workgroup row: g_z and g_pfeat from the same fragments.
// The two-row split reads both gradient tensors once per row and writes each half of a pixel's 2Z + C channels at another time; here a
// wave loads its 16 pixels of G_f and G_h once -- K-step pr of G_h IS the epilogue operand of g_pfeat's block pr (lane group fg holds
// channels 32 pr + 8 fg .. + 8 either way) -- and stores the whole pixel.  LDS: the z slab [32][K_z + 8], then the p_feat slab
// [32 nb][K_f + 8].  Same sums, same roundings as lt_run_z<DET> / lt_run_p.
#define LT_DK 2  // K-steps per gradient tensor (and 32-channel blocks of g_pfeat) of the one-row instance
template <int ORDER>
__device__ __forceinline__ void lt_run_det1(const LtP& p, char* smem) {
  static_assert(ORDER == 0 || ORDER == 1, "the sequential orders only");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int Kf = p.nks_f * 32, K = Kf + p.nks_h * 32, ldz = K + 8, ldp = Kf + 8, nb = p.nks_h;
  const int ch = fg * 8;
  const bool live = ch < p.Z;
  char* smem_p = smem + 32 * ldz * 2;

  uint4 xf[LT_DK], xh[LT_DK];
  int px = 0;
  bool inside = false;
  auto request = [&](int t) {
    px = t * LT_PX + wave * 16 + fr;
    inside = px < p.P;
    const int pc = inside ? px : p.P - 1;  // (a lane past the last pixel multiplies the last pixel again; nothing of it is stored)
#pragma unroll
    for (int i = 0; i < LT_DK; ++i) {
      if (i < p.nks_f) xf[i] = *(const uint4*)(p.g_f + (pc * p.s_gf + i * 32 + ch));
    }
#pragma unroll
    for (int i = 0; i < LT_DK; ++i) {
      if (i < p.nks_h) xh[i] = *(const uint4*)(p.g_h + (pc * p.s_gh + i * 32 + ch));
    }
  };
  int t = (int)blockIdx.x;
  request(t);
  {  // the two slabs, once: rows permuted as in lt_run_z / lt_run_p
    const int gz = K >> 3, gp = Kf >> 3;
    for (int g = tid; g < 32 * gz; g += 256) {
      const int r = g / gz, k = (g - r * gz) * 8;
      const int h = r >> 4, j = r & 15, c = (j >> 2) * 8 + h * 4 + (j & 3);
      const h16_t* src = k < Kf ? p.img_fz + (c * p.krow_f + k) : p.img_pz + (c * p.krow_p + (k - Kf));
      *(uint4*)(smem + (r * ldz + k) * 2) = lt_ld(src, 0, c < p.Z);
    }
    for (int g = tid; g < nb * 32 * gp; g += 256) {
      const int r = g / gp, k = (g - r * gp) * 8;
      const int pr = r >> 5, h = (r >> 4) & 1, j = r & 15, c = pr * 32 + (j >> 2) * 8 + h * 4 + (j & 3);
      *(uint4*)(smem_p + (r * ldp + k) * 2) = *(const uint4*)(p.img_fp + (c * p.krow_f + k));  // (c < C: nb blocks of 32)
    }
  }
  __syncthreads();
  const char* az = smem + (fr * ldz + fg * 8) * 2;
  const char* azh = az + Kf * 2;
  const char* ap = smem_p + (fr * ldp + fg * 8) * 2;
  for (;;) {
    f32x4_t aF[2], aH[2], aP[LT_DK][2];
    aF[0] = aF[1] = aH[0] = aH[1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < LT_DK; ++pr) aP[pr][0] = aP[pr][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < LT_DK; ++i) {
      if (i < p.nks_f) {  // (uniform)
        const h16x8 b = lt_frag(xf[i]);
        aF[0] = mfma_h16(*(const h16x8*)(az + i * 64), b, aF[0], 0, 0, 0);
        aF[1] = mfma_h16(*(const h16x8*)(az + (16 * ldz) * 2 + i * 64), b, aF[1], 0, 0, 0);
#pragma unroll
        for (int pr = 0; pr < LT_DK; ++pr) {
          if (pr < nb) {  // (uniform)
            aP[pr][0] = mfma_h16(*(const h16x8*)(ap + ((pr * 32) * ldp) * 2 + i * 64), b, aP[pr][0], 0, 0, 0);
            aP[pr][1] = mfma_h16(*(const h16x8*)(ap + ((pr * 32 + 16) * ldp) * 2 + i * 64), b, aP[pr][1], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < LT_DK; ++i) {
      if (i < p.nks_h) {  // (uniform; ORDER 0 goes on with the one sum)
        const h16x8 b = lt_frag(xh[i]);
        f32x4_t(&a)[2] = ORDER == 0 ? aF : aH;
        a[0] = mfma_h16(*(const h16x8*)(azh + i * 64), b, a[0], 0, 0, 0);
        a[1] = mfma_h16(*(const h16x8*)(azh + (16 * ldz) * 2 + i * 64), b, a[1], 0, 0, 0);
      }
    }
    if (inside) {
      h16_t* o = p.out_p + px * p.s_op;
      if (live) {  // grad(p_loc) = g_z, grad(p_ls) = 0
        float gz[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float zf = e < 4 ? aF[0][e & 3] : aF[1][e & 3], zh = e < 4 ? aH[0][e & 3] : aH[1][e & 3];
          if constexpr (ORDER == 0) gz[e] = zf;
          else gz[e] = p.nks_f ? lt_r16(zh + lt_r16(zf)) : lt_r16(zh);  // z_feat_proj's data gradient wrote grad(p_loc), z_proj's added to it
        }
        *(uint4*)(o + ch) = pack8(gz);
        *(uint4*)(o + p.Z + ch) = make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int pr = 0; pr < LT_DK; ++pr) {
        if (pr < nb) {  // grad(p_feat) = G_h + W_f[:, Z:]^T G_f; without z_feat_proj G_h's bits
          float v[8];
          unpack8(xh[pr], v);
          if (p.nks_f) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float f = e < 4 ? aP[pr][0][e & 3] : aP[pr][1][e & 3];
              v[e] += ORDER == 0 ? f : lt_r16(f);
            }
          }
          *(uint4*)(o + 2 * p.Z + pr * 32 + ch) = pack8(v);
        }
      }
    }
    t += (int)gridDim.x;
    if (t >= p.ntiles) break;
    request(t);
  }
}
template <int ORDER>
__global__ __launch_bounds__(256, 4) void latent_tail_det1_bwd_kernel(LtP p) {
  CGEN_SETPRIO();
  extern __shared__ __attribute__((aligned(16))) char lt_smem[];
  lt_run_det1<ORDER>(p, lt_smem);
}

// The deterministic layer's wider instances (cgen_latent_tail_bwd without q_loc / q_ls): the two bodies above, nothing accumulated, the
// sequential orders only (lt_reject declines the small-image shapes).  Instances of their own: the stochastic ones keep their code.
template <int MAXKF, int ORDER>
__global__ __launch_bounds__(256, 4) void latent_tail_det_bwd_kernel(LtP p) {
  CGEN_SETPRIO();
  extern __shared__ __attribute__((aligned(16))) char lt_smem[];
  if (blockIdx.y == 0) lt_run_z<MAXKF, false, ORDER, true>(p, lt_smem);
  else lt_run_p<MAXKF, false, ORDER>(p, lt_smem);
}

// ----------------------------------------------------------------------------- host
static int lt_smallp_maxp() {
  static const int v = [] { const char* e = getenv("CGEN_SMALLP_MAXP"); return e ? atoi(e) : 6000; }();
  return v;
}
static bool lt_conv_knob_set() {  // a knob that changes which kernel cgen_conv2d serves a 1x1 conv with
  return getenv("CGEN_CONV_NO_PX") || getenv("CGEN_CONV_NO_SMALLP") || getenv("CGEN_CONV_GENERIC") || getenv("CGEN_PX_MODE") ||
         getenv("CGEN_SMALLP_MAXP_LONGK") || getenv("CGEN_SMALLP_LONGK");
}
static bool lt_is_det(const cgen_latent_tail_bwd_args* a) { return !a->q_loc.p && !a->q_ls.p; }

// the deterministic form: out_p alone is written; only the conv_px order is built
static const char* lt_reject_det(const cgen_latent_tail_bwd_args* a) {
  if (a->gz_in.p || a->p_loc.p || a->p_ls.p || a->z.p || a->out_q.p) return "a reparam view without q_loc / q_ls";
  if (a->acc_p || a->acc_q) return "the deterministic tail does not accumulate";
  if ((int64_t)a->n * a->h * a->w <= lt_smallp_maxp() || a->h < 5 || a->w < 5) return "a shape of the small-image conv";
  if (lt_conv_knob_set()) return "a conv dispatch knob is set";
  return nullptr;
}

static const char* lt_reject(const cgen_latent_tail_bwd_args* a) {
  if (!a) return "null args";
  if (a->dtype != CGEN_F16) return "binary16 only";
  if (a->n < 1 || a->h < 1 || a->w < 1) return "empty problem";
  const int Z = a->z_dim, C = a->c;
  const bool det = lt_is_det(a);
  if (det) {
    if (const char* why = lt_reject_det(a)) return why;
  }
  if (Z != 8 && Z != 16) return "z_dim must be 8 or 16";
  if (C < 32 || C % 32 != 0 || C > 32 * LT_MAXKF) return "C must be a multiple of 32, at most 192";
  const int Cf = a->g_f.p ? a->g_f.c : 0;
  if (a->g_f.p && (Cf < 32 || Cf % 32 != 0 || Cf > 32 * LT_MAXKF)) return "g_f.c must be a multiple of 32, at most 192";
  const int64_t P = (int64_t)a->n * a->h * a->w;
  if (P >= (1ll << 31) / 2) return "too many pixels";
  struct { const cgen_view* v; int c; bool need; } vs[] = {
      {&a->g_h, C, true},     {&a->g_f, Cf, false},  {&a->gz_in, Z, false}, {&a->q_loc, Z, !det},         {&a->q_ls, Z, !det},
      {&a->p_loc, Z, !det},   {&a->p_ls, Z, !det},   {&a->z, Z, !det},      {&a->out_p, 2 * Z + C, true}, {&a->out_q, 2 * Z, !det}};
  for (auto& e : vs) {
    const cgen_view& v = *e.v;
    if (!v.p) {
      if (e.need) return "a required view is absent";
      continue;
    }
    if (v.c != e.c) return "a view has the wrong channel count";
    if (!vec16_ok(v, 2)) return "a view is not 16-byte clean";
    if (v.sw < v.c) return "pixel stride below the channel count";
    if (v.sh != (int64_t)a->w * v.sw || v.sn != (int64_t)a->h * v.sh) return "a view is not linear in pixels";
    if ((P * v.sw + v.c) * 2 >= (1ll << 31)) return "a view spans 2^31 bytes or more";
  }
  if (!a->img_pz || (a->g_f.p && (!a->img_fz || !a->img_fp))) return "a weight image is absent";
  if (((uintptr_t)a->img_pz | (uintptr_t)a->img_fz | (uintptr_t)a->img_fp) % 16) return "a weight image is not 16-byte aligned";
  if (det) return nullptr;
  if (!a->coef) return "kl coefficient absent";
  if (a->coef_stride < 0) return "negative coef_stride";
  return nullptr;
}

}  // namespace cgen

extern "C" int cgen_latent_tail_bwd_supported(const cgen_latent_tail_bwd_args* a) { return cgen::lt_reject(a) == nullptr ? 1 : 0; }

extern "C" int cgen_latent_tail_bwd(const cgen_latent_tail_bwd_args* a, cgen_stream_t stream) {
  using namespace cgen;
  if (const char* why = lt_reject(a)) return fail(CGEN_EUNSUPPORTED, "cgen_latent_tail_bwd: %s", why);
  LtP p;
  memset(&p, 0, sizeof(p));
  p.P = a->n * a->h * a->w; p.hw = a->h * a->w; p.Z = a->z_dim; p.C = a->c; p.Cf = a->g_f.p ? a->g_f.c : 0;
  p.nks_f = p.Cf / 32; p.nks_h = p.C / 32;
  p.ntiles = (p.P + LT_PX - 1) / LT_PX;
  p.krow_f = (p.Cf + 31) / 32 * 32 + 32; p.krow_p = (p.C + 31) / 32 * 32 + 32;
  p.s_gh = (int)a->g_h.sw; p.s_gf = (int)a->g_f.sw; p.s_gz = (int)a->gz_in.sw;
  p.s_ql = (int)a->q_loc.sw; p.s_qs = (int)a->q_ls.sw; p.s_pl = (int)a->p_loc.sw; p.s_ps = (int)a->p_ls.sw; p.s_z = (int)a->z.sw;
  p.s_op = (int)a->out_p.sw; p.s_oq = (int)a->out_q.sw;
  p.g_h = (const h16_t*)a->g_h.p; p.g_f = (const h16_t*)a->g_f.p; p.gz_in = (const h16_t*)a->gz_in.p;
  p.q_loc = (const h16_t*)a->q_loc.p; p.q_ls = (const h16_t*)a->q_ls.p; p.p_loc = (const h16_t*)a->p_loc.p; p.p_ls = (const h16_t*)a->p_ls.p;
  p.z = (const h16_t*)a->z.p; p.out_p = (h16_t*)a->out_p.p; p.out_q = (h16_t*)a->out_q.p;
  p.img_fz = (const h16_t*)a->img_fz; p.img_fp = (const h16_t*)a->img_fp; p.img_pz = (const h16_t*)a->img_pz;
  p.coef = a->coef; p.chan_scale = a->chan_scale; p.coef_stride = a->coef_stride; p.acc_q = a->acc_q ? 1 : 0; p.acc_p = a->acc_p ? 1 : 0;
  p.logt = a->logt;
  // LDS: the larger of the two slabs ([32][K_z + 8] for part 0, [32 LT_NP][K_f + 8] for the others), at most 25 KiB
  const int kz = (p.nks_f + p.nks_h) * 32, kf = p.nks_f * 32;
  const size_t lds_z = (size_t)32 * (kz + 8) * 2, lds_p = (size_t)LT_NP * 32 * (kf + 8) * 2;
  const size_t lds = lds_z > lds_p ? lds_z : lds_p;
  const int parts = 1 + (p.C / 32 + LT_NP - 1) / LT_NP;
  // parity: the order the four launches sum in at this shape -- cgen_conv2d hands a 1x1 conv over few pixels (or a side below 5
  // that the caller cannot present as rows of 16 pixels) to conv_smallp_kernel, everything else here to conv_px_kernel
  const int smallp_maxp = lt_smallp_maxp();
  const bool by_side = (a->h < 5 || a->w < 5) && (p.P % 16 != 0 || p.P < 256);
  const int order = !a->parity ? 0 : (p.P <= smallp_maxp || by_side) ? 2 : 1;
  // persistent over pixel tiles: as many workgroups as are resident at once (256 CUs), every part the same share
  const bool small = p.nks_f <= 4 && p.nks_h <= 4, accum = p.acc_q || p.acc_p || p.gz_in != nullptr;
  const int resident = (order == 2 ? 512 : accum ? 768 : 1024) / parts;
  const int rounds = (p.ntiles + resident - 1) / resident;
  const int gx = (p.ntiles + rounds - 1) / rounds;  // every workgroup the same number of tiles: no half-empty last round
  const dim3 grid(gx, parts), block(256);
  if (lt_is_det(a)) {  // (lt_reject: order is 0 or 1, nothing accumulates)
    if (p.nks_f <= LT_DK && p.nks_h <= LT_DK) {  // one workgroup row: four workgroups per CU, every one the same number of tiles
      const size_t lds1 = (size_t)32 * (kz + 8) * 2 + (size_t)p.nks_h * 32 * (kf + 8) * 2;
      const int rounds1 = (p.ntiles + 1023) / 1024;
      const dim3 grid1((p.ntiles + rounds1 - 1) / rounds1);
      if (order == 0) hipLaunchKernelGGL((latent_tail_det1_bwd_kernel<0>), grid1, block, lds1, (hipStream_t)stream, p);
      else hipLaunchKernelGGL((latent_tail_det1_bwd_kernel<1>), grid1, block, lds1, (hipStream_t)stream, p);
      return check_launch("cgen_latent_tail_bwd(det)");
    }
#define LT_DET(KF_) do { if (order == 0) hipLaunchKernelGGL((latent_tail_det_bwd_kernel<KF_, 0>), grid, block, lds, (hipStream_t)stream, p); \
                         else hipLaunchKernelGGL((latent_tail_det_bwd_kernel<KF_, 1>), grid, block, lds, (hipStream_t)stream, p); } while (0)
    if (small) LT_DET(4); else LT_DET(LT_MAXKF);
#undef LT_DET
    return check_launch("cgen_latent_tail_bwd(det)");
  }
#define LT_LAUNCH(KF_, ACC_, ORD_) hipLaunchKernelGGL((latent_tail_bwd_kernel<KF_, ACC_, ORD_>), grid, block, lds, (hipStream_t)stream, p)
#define LT_ORDER(KF_, ACC_) do { if (order == 0) LT_LAUNCH(KF_, ACC_, 0); else if (order == 1) LT_LAUNCH(KF_, ACC_, 1); else LT_LAUNCH(KF_, ACC_, 2); } while (0)
  if (small) { if (accum) LT_ORDER(4, true); else LT_ORDER(4, false); }
  else { if (accum) LT_ORDER(LT_MAXKF, true); else LT_ORDER(LT_MAXKF, false); }
#undef LT_ORDER
#undef LT_LAUNCH
  return check_launch("cgen_latent_tail_bwd");
}

// ============================================================================= forward latent tail (cgen_latent_tail_fwd)
// What it replaces ran as three launches per layer: reparam_kl_fwd writes z, the 1x1 conv z_proj reads it back (with pa; bias + h +
// p_feat in its epilogue), the 1x1 conv z_feat_proj reads it and p_feat again.  Here:
//   * a tile is ONE KL chunk -- LAT_CHUNK / Z pixels of one sample, 256 threads with reparam_kl_fwd_vec8_item's thread -> element
//     mapping -- so the KL partials keep their geometry and block_sum_256 its summation order;
//   * z leaves as one 16-byte store per thread AND goes to an LDS tile, from which the MFMA pixel operand's z lanes are read; every
//     other operand lane (pa / p_feat: 8 consecutive channels of one pixel) is a 16-byte global load straight into registers,
//     requested together with the epilogue operands (h, p_feat) before the reparam math;
//   * gridDim.y splits the output channels into LF_NP 32-channel blocks: rows [0, parts_p) own h' (K = [z | pa], one or two
//     K-steps), the rest own zf (K = [z | p_feat]).  Every row recomputes z in registers from q_loc, q_ls and the same Philox
//     counters; only row 0 reads p_loc / p_ls, stores z and the KL partial;
//   * persistent over tiles: the row's weight slab goes to LDS once (rows permuted inside each 32-row block as in conv_px_kernel:
//     a lane ends up with 8 consecutive output channels of its pixel, one 16-byte store per result);
//   * ORDER 1 / 2: the summation order of conv_px_kernel / conv_smallp_kernel, whichever cgen_conv2d picks for the shape.
namespace cgen {

#define LF_NP 2     // 32-channel output blocks per workgroup
#define LF_MAXKP 2  // K-steps of z_proj: Z + ceil8(ctx) <= 64
#define LF_MAXKF 7  // K-steps of z_feat_proj: Z + C <= 208

struct LfP {
  int hw, per, chunks, ntiles, C, Cf, ctx8, parts_p;
  int nks_p, nks_f, krow_p, krow_f;
  int s_ql, s_qs, s_pl, s_ps, s_pf, s_eps, s_h, s_z, s_ho, s_zf, pa_sn, pa_sw;  // pixel strides (elements); pa: sample and pixel stride
  const h16_t *q_loc, *q_ls, *p_loc, *p_ls, *p_feat, *eps, *h_in, *pa;
  h16_t *z, *h_out, *zf;
  const h16_t *img_p, *img_f;
  const float *bias_p, *bias_f;
  const uint64_t* rng;
  uint32_t stream_id;
  float logt;
  float* kl_part;
  int kl_stride;
};

// ROLE_P: this workgroup row computes h' (z_proj), else zf (z_feat_proj).  `part`: its index among the rows of its role.
// DET: the layer is deterministic (z = p_loc, a channel slice of the prior Block's output): the z lanes of K-step 0 are 16-byte global
// loads like every other operand lane, and everything tied to the KL chunk is absent -- no reparam, no z tile in LDS, no z store, no KL
// partial, no barrier per tile.  (A tile keeps the chunk's LAT_CHUNK / Z pixels of one sample: pa is addressed per sample.)
template <int ZD, int MAXK, int ORDER, bool ROLE_P, bool DET = false>
__device__ __forceinline__ void lf_run(const LfP& p, char* smem, const int part) {
  constexpr int TP = LAT_CHUNK / ZD;  // pixels per tile
  constexpr int NF = TP / 64;         // 16-pixel fragments per wave and tile: 2 (Z = 16) or 4 (Z = 8), taken two at a time
  constexpr int CG = ZD / 8;          // 8-channel groups per pixel
  constexpr int ZLD = ZD + 8;         // row of the z tile in LDS (elements)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int nks = ROLE_P ? p.nks_p : p.nks_f, K = nks * 32, ldw = K + 8;
  const int krow = ROLE_P ? p.krow_p : p.krow_f, Co = ROLE_P ? p.C : p.Cf;
  const int s1c = ROLE_P ? p.ctx8 : p.C;  // channels of the second input segment (pa is zero padded to ctx8)
  const h16_t* img = ROLE_P ? p.img_p : p.img_f;
  const float* bias = ROLE_P ? p.bias_p : p.bias_f;
  h16_t* outp = ROLE_P ? p.h_out : p.zf;
  const int s_out = ROLE_P ? p.s_ho : p.s_zf;
  const int co_base = part * (LF_NP * 32), ch0 = co_base + fg * 8;
  const bool first = ROLE_P && part == 0;  // the row that owns z and the KL partial
  float* sm = (float*)smem;
  char* zt = smem + 16;
  char* wsl = DET ? smem : zt + TP * ZLD * 2;
  uint64_t seed = 0, off = 0;
  if constexpr (!DET) {
    if (!p.eps) { seed = p.rng[0]; off = p.rng[1]; }
  }

  uint4 ql, qs, pl, ps, ev, xb[2][MAXK], eh[ROLE_P ? 2 : 1][LF_NP], ep[ROLE_P ? 2 : 1][LF_NP];
  int b = 0, chunk = 0, e0 = 0, gpx = 0, xb_b = 0, xb_chunk = 0, opx[2];
  bool live = false, okf[2];
  // the reparam operands of this thread's element group (8 channels of one pixel) of tile t
  auto request_z = [&](int t) {
    b = t / p.chunks; chunk = t - b * p.chunks;
    e0 = chunk * LAT_CHUNK + tid * 8;
    live = e0 < p.per;
    gpx = b * p.hw + chunk * TP + (live ? tid / CG : 0);  // (a thread past the sample's end reads the tile's first pixel; nothing of it is kept)
    const int ch = (tid % CG) * 8;
    ql = *(const uint4*)(p.q_loc + (gpx * p.s_ql + ch)); qs = *(const uint4*)(p.q_ls + (gpx * p.s_qs + ch));
    pl = lt_ld(p.p_loc, gpx * p.s_pl + ch, first); ps = lt_ld(p.p_ls, gpx * p.s_ps + ch, first);
    ev = lt_ld(p.eps, gpx * p.s_eps + ch, p.eps != nullptr);
  };
  // the GEMM and epilogue operands of fragments 2 g and 2 g + 1 of this wave: pixel operand lane (fr, fg) of K-step i = channels
  // i * 32 + fg * 8 .. + 8 of [z | segment 1] (each padded to 8, as cgen_conv2d concatenates) of the fragment's pixel fr
  // (of tile (xb_b, xb_chunk): by then request_z may already have moved on to the next tile)
  auto request_x = [&](int g) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int lp = xb_chunk * TP + (wave * NF + g * 2 + f) * 16 + fr;  // pixel inside the sample
      okf[f] = lp < p.hw;
      const int pc = okf[f] ? lp : xb_chunk * TP;
      opx[f] = xb_b * p.hw + pc;
#pragma unroll
      for (int i = 0; i < MAXK; ++i) {
        if (i < nks) {  // (uniform)
          const int c = i * 32 + fg * 8 - ZD;
          const bool s1 = c >= 0 && c < s1c;
          if constexpr (DET) {  // (one load from a selected address: the lanes whose part of K-step 0 is z read p_loc)
            const bool zl = i == 0 && c < 0;
            const h16_t* s1p = ROLE_P ? p.pa + (xb_b * p.pa_sn + pc * p.pa_sw + c) : p.p_feat + (opx[f] * p.s_pf + c);
            xb[f][i] = lt_ld(zl ? p.p_loc + (opx[f] * p.s_pl + fg * 8) : s1p, 0, zl || s1);
          } else if constexpr (ROLE_P) xb[f][i] = lt_ld(p.pa, xb_b * p.pa_sn + pc * p.pa_sw + c, s1);
          else xb[f][i] = lt_ld(p.p_feat, opx[f] * p.s_pf + c, s1);
        }
      }
      if constexpr (ROLE_P) {
#pragma unroll
        for (int pr = 0; pr < LF_NP; ++pr) {
          const bool okc = ch0 + pr * 32 < Co;  // (Co is a multiple of 32: a block is inside or outside as a whole)
          eh[f][pr] = lt_ld(p.h_in, opx[f] * p.s_h + ch0 + pr * 32, okc);
          ep[f][pr] = lt_ld(p.p_feat, opx[f] * p.s_pf + ch0 + pr * 32, okc);
        }
      }
    }
  };
  int t = (int)blockIdx.x;
  if constexpr (DET) { b = t / p.chunks; chunk = t - b * p.chunks; }
  else request_z(t);
  xb_b = b; xb_chunk = chunk;
  request_x(0);
  // ---- weight slab, once: LDS row pr * 32 + h * 16 + j holds output channel co_base + pr * 32 + (j >> 2) * 8 + h * 4 + (j & 3): MFMA h of
  // block pr then leaves channels 8 fg + 4 h + {0..3} of the block in lane group fg
  {
    const int gpr = K >> 3;
    for (int g = tid; g < LF_NP * 32 * gpr; g += 256) {
      const int r = g / gpr, k = (g - r * gpr) * 8;
      const int pr = r >> 5, h = (r >> 4) & 1, j = r & 15, c = co_base + pr * 32 + (j >> 2) * 8 + h * 4 + (j & 3);
      *(uint4*)(wsl + (r * ldw + k) * 2) = lt_ld(img, c * krow + k, c < Co);
    }
  }
  f32x4_t binit[LF_NP][2];  // the bias of this lane's channels: conv_px's initial accumulator value, conv_smallp's first epilogue term
#pragma unroll
  for (int pr = 0; pr < LF_NP; ++pr)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int co = ch0 + pr * 32 + h * 4;
      const float4 bb = *(const float4*)((bias && co + 4 <= Co) ? (const void*)(bias + co) : (const void*)g_lt_zero);
      binit[pr][h] = (f32x4_t){bb.x, bb.y, bb.z, bb.w};
    }
  const char* a_base = wsl + (fr * ldw + fg * 8) * 2;
  if constexpr (DET) __syncthreads();  // the slab is visible (the stochastic form's first tile barrier does this)
  for (;;) {
    // ---- reparameterise: z to memory (row 0) and to the LDS tile, the KL partial of the chunk (row 0)
    if constexpr (!DET) {
      float fql[8], fqs[8], fpl[8], fps[8], fe[8], fz[8];
      unpack8(ql, fql); unpack8(qs, fqs); unpack8(pl, fpl); unpack8(ps, fps);
      if (p.eps) unpack8(ev, fe);
      else reparam_eps8(seed, off, p.stream_id, (uint64_t)b * p.per + e0, fe);
      float kl_acc = reparam_kl_fwd_vec8_math(p.logt, fql, fqs, fpl, fps, fe, fz);
      if (!live) kl_acc = 0.f;
      const uint4 zv = live ? pack8(fz) : make_uint4(0, 0, 0, 0);
      *(uint4*)(zt + ((tid / CG) * ZLD + (tid % CG) * 8) * 2) = zv;
      if (first) {
        if (live) *(uint4*)(p.z + (gpx * p.s_z + (tid % CG) * 8)) = zv;
        const float tot = block_sum_256(kl_acc, sm);  // (two barriers: the z tile is visible behind them)
        if (tid == 0) p.kl_part[(int64_t)b * p.kl_stride + chunk] = tot;
      } else {
        __syncthreads();
      }
    }
    // the next tile's reparam operands are requested now: they arrive under this tile's MFMAs and stores
    t += (int)gridDim.x;
    const bool more = t < p.ntiles;
    if constexpr (DET) { b = t / p.chunks; chunk = t - b * p.chunks; }
    else if (more) request_z(t);
#pragma unroll
    for (int g = 0; g < NF / 2; ++g) {
      if (g > 0) request_x(g);
      if (!DET && fg < CG) {  // this lane's part of K-step 0 is z
#pragma unroll
        for (int f = 0; f < 2; ++f) xb[f][0] = *(const uint4*)(zt + (((wave * NF + g * 2 + f) * 16 + fr) * ZLD + fg * 8) * 2);
      }
      f32x4_t acc[LF_NP][2][2];  // [block][MFMA h][fragment]
      if constexpr (ORDER == 1) {  // conv_px: the bias is the initial value, the K-steps accumulate in sequence
#pragma unroll
        for (int pr = 0; pr < LF_NP; ++pr)
#pragma unroll
          for (int h = 0; h < 2; ++h) acc[pr][h][0] = acc[pr][h][1] = binit[pr][h];
#pragma unroll
        for (int i = 0; i < MAXK; ++i) {
          if (i < nks) {  // (uniform)
#pragma unroll
            for (int pr = 0; pr < LF_NP; ++pr)
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const h16x8 aq = *(const h16x8*)(a_base + ((pr * 32 + h * 16) * ldw) * 2 + i * 64);
                acc[pr][h][0] = mfma_h16(aq, lt_frag(xb[0][i]), acc[pr][h][0], 0, 0, 0);
                acc[pr][h][1] = mfma_h16(aq, lt_frag(xb[1][i]), acc[pr][h][1], 0, 0, 0);
              }
          }
        }
      } else {  // conv_smallp: K-step i belongs to wave i % 4's partial sum; the partials are added in wave order, then the bias
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          f32x4_t part_[LF_NP][2][2];
#pragma unroll
          for (int pr = 0; pr < LF_NP; ++pr)
#pragma unroll
            for (int h = 0; h < 2; ++h) part_[pr][h][0] = part_[pr][h][1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int i = w; i < MAXK; i += 4) {
            if (i < nks) {  // (uniform)
#pragma unroll
              for (int pr = 0; pr < LF_NP; ++pr)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                  const h16x8 aq = *(const h16x8*)(a_base + ((pr * 32 + h * 16) * ldw) * 2 + i * 64);
                  part_[pr][h][0] = mfma_h16(aq, lt_frag(xb[0][i]), part_[pr][h][0], 0, 0, 0);
                  part_[pr][h][1] = mfma_h16(aq, lt_frag(xb[1][i]), part_[pr][h][1], 0, 0, 0);
                }
            }
          }
#pragma unroll
          for (int pr = 0; pr < LF_NP; ++pr)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int f = 0; f < 2; ++f) {
                if (w == 0) acc[pr][h][f] = part_[pr][h][f];
                else { acc[pr][h][f][0] += part_[pr][h][f][0]; acc[pr][h][f][1] += part_[pr][h][f][1]; acc[pr][h][f][2] += part_[pr][h][f][2]; acc[pr][h][f][3] += part_[pr][h][f][3]; }
              }
        }
      }
      // ---- epilogue straight from the accumulators, cgen_conv2d's order: (+ bias) + res1 (h) + res2 (p_feat), one rounding
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int pr = 0; pr < LF_NP; ++pr) {
          if (!(okf[f] && ch0 + pr * 32 < Co)) continue;
          float v[8], tp[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = acc[pr][0][f][e]; v[4 + e] = acc[pr][1][f][e]; }
          if (ORDER != 1 && bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] += binit[pr][0][e]; v[4 + e] += binit[pr][1][e]; }
          }
          if constexpr (ROLE_P) {
            unpack8(eh[f][pr], tp);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += tp[e];
            unpack8(ep[f][pr], tp);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += tp[e];
          }
          *(uint4*)(outp + (opx[f] * s_out + ch0 + pr * 32)) = pack8(v);
        }
    }
    if (!more) break;
    if constexpr (!DET) __syncthreads();  // every wave is done reading the z tile before the next one overwrites it
    xb_b = b; xb_chunk = chunk;
    request_x(0);
  }
}

// ZD: latent channels; MAXKF: K-steps of z_feat_proj the instance is compiled for (the pixel fragments live in registers): 5 serves
// C <= 128 at Z = 16 -- ukbb192's layers of 24x24 and above -- 7 the widest; ORDER as above.  The sequential order is the large
// layers': three workgroups per CU (168 registers; at 128 it spills), which the grid below counts on -- at two per CU a 48x48 layer
// was five serial round trips per workgroup, 30 us where the three launches' main chain took 27; the four-partial order (few
// pixels, one round anyway) keeps its second accumulator set and two per CU.
template <int ZD, int MAXKF, int ORDER>
__global__ __launch_bounds__(256, ORDER == 1 ? 3 : 2) void latent_tail_fwd_kernel(LfP p) {
  CGEN_SETPRIO();  // the chain's waves win issue arbitration over background weight-gradient waves on the same SIMD
  extern __shared__ __attribute__((aligned(16))) char lf_smem[];
  if ((int)blockIdx.y < p.parts_p) lf_run<ZD, LF_MAXKP, ORDER, true>(p, lf_smem, (int)blockIdx.y);
  else lf_run<ZD, MAXKF, ORDER, false>(p, lf_smem, (int)blockIdx.y - p.parts_p);
}

// The deterministic layer's instances (cgen_latent_tail_fwd without q_loc / q_ls): conv_px's order only (lf_reject declines the
// small-image shapes).  Instances of their own: the stochastic ones keep their code.
template <int ZD, int MAXKF>
__global__ __launch_bounds__(256, 3) void latent_tail_det_fwd_kernel(LfP p) {
  CGEN_SETPRIO();
  extern __shared__ __attribute__((aligned(16))) char lf_smem[];
  if ((int)blockIdx.y < p.parts_p) lf_run<ZD, LF_MAXKP, 1, true, true>(p, lf_smem, (int)blockIdx.y);
  else lf_run<ZD, MAXKF, 1, false, true>(p, lf_smem, (int)blockIdx.y - p.parts_p);
}

static inline int lf_pad(int v, int m) { return (v + m - 1) / m * m; }
static bool lf_is_det(const cgen_latent_tail_fwd_args* a) { return !a->q_loc.p && !a->q_ls.p; }

static const char* lf_reject(const cgen_latent_tail_fwd_args* a) {
  if (!a) return "null args";
  if (a->dtype != CGEN_F16) return "binary16 only";
  if (a->n < 1 || a->h < 1 || a->w < 1) return "empty problem";
  const int Z = a->z_dim, C = a->c;
  if (Z != 8 && Z != 16) return "z_dim must be 8 or 16";
  if (C < 32 || C % 32 != 0 || C > 192) return "C must be a multiple of 32, at most 192";
  const int Cf = a->zf.p ? a->zf.c : 0;
  if (a->zf.p && (Cf < 32 || Cf % 32 != 0 || Cf > 192)) return "zf.c must be a multiple of 32, at most 192";
  if (a->ctx < 1 || Z + lf_pad(a->ctx, 8) > 32 * LF_MAXKP) return "z_proj's K is more than two K-steps";
  if (a->h_in_rem || a->h_out_rem) return "remainder planes are not served";
  const int64_t P = (int64_t)a->n * a->h * a->w;
  if (P >= (1ll << 31) / 2) return "too many pixels";
  // which kernel cgen_conv2d serves the two convs with must be the same for both and known from the shape alone
  if ((a->h < 5 || a->w < 5) && P > lt_smallp_maxp()) return "an image side below 5 with more pixels than the small-image conv takes";
  if (lt_conv_knob_set()) return "a conv dispatch knob is set";
  const bool det = lf_is_det(a);  // z = p_loc: only h_out and zf are written; only the conv_px order is built
  if (det) {
    if (a->p_ls.p || a->eps.p || a->z.p) return "a reparam view without q_loc / q_ls";
    if (P <= lt_smallp_maxp() || a->h < 5 || a->w < 5) return "a shape of the small-image conv";
  }
  struct { const cgen_view* v; int c; bool need; } vs[] = {
      {&a->q_loc, Z, !det}, {&a->q_ls, Z, !det}, {&a->p_loc, Z, true}, {&a->p_ls, Z, !det}, {&a->p_feat, C, true}, {&a->h_in, C, true},
      {&a->eps, Z, false},  {&a->z, Z, !det},    {&a->h_out, C, true}, {&a->zf, Cf, false}};
  for (auto& e : vs) {
    const cgen_view& v = *e.v;
    if (!v.p) {
      if (e.need) return "a required view is absent";
      continue;
    }
    if (v.c != e.c) return "a view has the wrong channel count";
    if (!vec16_ok(v, 2)) return "a view is not 16-byte clean";
    if (v.sw < v.c) return "pixel stride below the channel count";
    if (v.sh != (int64_t)a->w * v.sw || v.sn != (int64_t)a->h * v.sh) return "a view is not linear in pixels";
    if ((P * v.sw + v.c) * 2 >= (1ll << 31)) return "a view spans 2^31 bytes or more";
  }
  {
    const cgen_view& v = a->pa;
    const int c8 = lf_pad(a->ctx, 8);
    if (!v.p || v.c != a->ctx) return "pa is absent or has the wrong channel count";
    if (!vec16_ok(v, 2)) return "pa is not 16-byte clean";
    if (a->ctx % 8 != 0 && v.cpad < c8) return "pa is not zero padded to 8 channels";
    const bool constant = v.sh == 0 && v.sw == 0, linear = v.sw >= c8 && v.sh == (int64_t)a->w * v.sw && v.sn == (int64_t)a->h * v.sh;
    if (!constant && !linear) return "pa is neither spatially constant nor linear in pixels";
    if (v.sn < 0 || ((int64_t)a->n * v.sn + P * v.sw + c8) * 2 >= (1ll << 31)) return "pa spans 2^31 bytes or more";
  }
  if (!a->img_p || (a->zf.p && !a->img_f)) return "a weight image is absent";
  if (((uintptr_t)a->img_p | (uintptr_t)a->img_f | (uintptr_t)a->bias_p | (uintptr_t)a->bias_f) % 16) return "a weight image or bias is not 16-byte aligned";
  if (det) return nullptr;
  if (!a->eps.p && !a->rng) return "neither eps nor rng";
  if (!a->kl_part || a->kl_stride < ceil_div((int64_t)a->h * a->w * Z, LAT_CHUNK)) return "kl_part absent or kl_stride below the chunk count";
  return nullptr;
}

}  // namespace cgen

extern "C" int cgen_latent_tail_fwd_supported(const cgen_latent_tail_fwd_args* a) { return cgen::lf_reject(a) == nullptr ? 1 : 0; }

extern "C" int cgen_latent_tail_fwd(const cgen_latent_tail_fwd_args* a, cgen_stream_t stream) {
  using namespace cgen;
  if (const char* why = lf_reject(a)) return fail(CGEN_EUNSUPPORTED, "cgen_latent_tail_fwd: %s", why);
  LfP p;
  memset(&p, 0, sizeof(p));
  const int Z = a->z_dim, P = a->n * a->h * a->w;
  p.hw = a->h * a->w; p.per = p.hw * Z; p.chunks = ceil_div(p.per, LAT_CHUNK); p.ntiles = a->n * p.chunks;
  p.C = a->c; p.Cf = a->zf.p ? a->zf.c : 0; p.ctx8 = lf_pad(a->ctx, 8);
  p.nks_p = ceil_div(Z + p.ctx8, 32); p.nks_f = p.Cf ? ceil_div(Z + p.C, 32) : 0;
  p.krow_p = lf_pad(Z + p.ctx8, 32) + 32; p.krow_f = lf_pad(Z + p.C, 32) + 32;
  p.parts_p = ceil_div(p.C / 32, LF_NP);
  const int parts = p.parts_p + ceil_div(p.Cf / 32, LF_NP);
  p.s_ql = (int)a->q_loc.sw; p.s_qs = (int)a->q_ls.sw; p.s_pl = (int)a->p_loc.sw; p.s_ps = (int)a->p_ls.sw; p.s_pf = (int)a->p_feat.sw;
  p.s_eps = (int)a->eps.sw; p.s_h = (int)a->h_in.sw; p.s_z = (int)a->z.sw; p.s_ho = (int)a->h_out.sw; p.s_zf = (int)a->zf.sw;
  p.pa_sn = (int)a->pa.sn; p.pa_sw = (int)a->pa.sw;
  p.q_loc = (const h16_t*)a->q_loc.p; p.q_ls = (const h16_t*)a->q_ls.p; p.p_loc = (const h16_t*)a->p_loc.p; p.p_ls = (const h16_t*)a->p_ls.p;
  p.p_feat = (const h16_t*)a->p_feat.p; p.eps = (const h16_t*)a->eps.p; p.h_in = (const h16_t*)a->h_in.p; p.pa = (const h16_t*)a->pa.p;
  p.z = (h16_t*)a->z.p; p.h_out = (h16_t*)a->h_out.p; p.zf = (h16_t*)a->zf.p;
  p.img_p = (const h16_t*)a->img_p; p.img_f = (const h16_t*)a->img_f; p.bias_p = a->bias_p; p.bias_f = a->bias_f;
  p.rng = a->rng; p.stream_id = a->stream_id; p.logt = a->logt; p.kl_part = a->kl_part; p.kl_stride = a->kl_stride;
  // LDS: 16 bytes for the block sum, the z tile [LAT_CHUNK / Z][Z + 8], the larger of the two roles' slabs [32 LF_NP][K + 8]: at most 38 KiB
  const int kmax = (p.nks_p > p.nks_f ? p.nks_p : p.nks_f) * 32;
  const size_t lds = 16 + (size_t)(LAT_CHUNK / Z) * (Z + 8) * 2 + (size_t)LF_NP * 32 * (kmax + 8) * 2;
  // the order cgen_conv2d sums in at this shape (launch_conv): conv_smallp_kernel takes few pixels and sides below 5 (which lf_reject
  // admits only with few pixels), conv_px_kernel every other 1x1 conv with a short K
  const int order = (P <= lt_smallp_maxp() || a->h < 5 || a->w < 5) ? 2 : 1;
  // persistent over tiles: as many workgroups as are resident at once (three or two per CU, 256 CUs), every one the same number of tiles
  const int resident = (order == 1 ? 768 : 512) / parts;  // (parts <= 6)
  const int rounds = (p.ntiles + resident - 1) / resident;
  const int gx = (p.ntiles + rounds - 1) / rounds;
  const dim3 grid(gx, parts), block(256);
  const bool small = p.nks_f <= 5;
  if (lf_is_det(a)) {  // (lf_reject: order is 1; LDS holds the slab alone)
    const size_t lds_det = (size_t)LF_NP * 32 * (kmax + 8) * 2;
#define LF_DET(Z_, KF_) hipLaunchKernelGGL((latent_tail_det_fwd_kernel<Z_, KF_>), grid, block, lds_det, (hipStream_t)stream, p)
    if (Z == 16) { if (small) LF_DET(16, 5); else LF_DET(16, LF_MAXKF); }
    else { if (small) LF_DET(8, 5); else LF_DET(8, LF_MAXKF); }
#undef LF_DET
    return check_launch("cgen_latent_tail_fwd(det)");
  }
#define LF_LAUNCH(Z_, KF_, ORD_) hipLaunchKernelGGL((latent_tail_fwd_kernel<Z_, KF_, ORD_>), grid, block, lds, (hipStream_t)stream, p)
#define LF_ORDER(Z_, KF_) do { if (order == 1) LF_LAUNCH(Z_, KF_, 1); else LF_LAUNCH(Z_, KF_, 2); } while (0)
  if (Z == 16) { if (small) LF_ORDER(16, 5); else LF_ORDER(16, LF_MAXKF); }
  else { if (small) LF_ORDER(8, 5); else LF_ORDER(8, LF_MAXKF); }
#undef LF_ORDER
#undef LF_LAUNCH
  return check_launch("cgen_latent_tail_fwd");
}
