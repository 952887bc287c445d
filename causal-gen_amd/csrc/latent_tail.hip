// Backward latent tail of a stochastic decoder layer in ONE launch (binary16): include/cgen_hip.h, cgen_latent_tail_bwd.
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
template <int MAXKF, bool ACC, int ORDER>
__device__ __forceinline__ void lt_run_z(const LtP& p, char* smem) {
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
    ql = lt_ld(p.q_loc, pc * p.s_ql + ch, ok); qs = lt_ld(p.q_ls, pc * p.s_qs + ch, ok);
    pl = lt_ld(p.p_loc, pc * p.s_pl + ch, ok); ps = lt_ld(p.p_ls, pc * p.s_ps + ch, ok);
    zv = lt_ld(p.z, pc * p.s_z + ch, ok);
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

// ----------------------------------------------------------------------------- host
static const char* lt_reject(const cgen_latent_tail_bwd_args* a) {
  if (!a) return "null args";
  if (a->dtype != CGEN_F16) return "binary16 only";
  if (a->n < 1 || a->h < 1 || a->w < 1) return "empty problem";
  const int Z = a->z_dim, C = a->c;
  if (Z != 8 && Z != 16) return "z_dim must be 8 or 16";
  if (C < 32 || C % 32 != 0 || C > 32 * LT_MAXKF) return "C must be a multiple of 32, at most 192";
  const int Cf = a->g_f.p ? a->g_f.c : 0;
  if (a->g_f.p && (Cf < 32 || Cf % 32 != 0 || Cf > 32 * LT_MAXKF)) return "g_f.c must be a multiple of 32, at most 192";
  const int64_t P = (int64_t)a->n * a->h * a->w;
  if (P >= (1ll << 31) / 2) return "too many pixels";
  struct { const cgen_view* v; int c; bool need; } vs[] = {
      {&a->g_h, C, true},     {&a->g_f, Cf, false},  {&a->gz_in, Z, false}, {&a->q_loc, Z, true},         {&a->q_ls, Z, true},
      {&a->p_loc, Z, true},   {&a->p_ls, Z, true},   {&a->z, Z, true},      {&a->out_p, 2 * Z + C, true}, {&a->out_q, 2 * Z, true}};
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
  static const int smallp_maxp = [] { const char* e = getenv("CGEN_SMALLP_MAXP"); return e ? atoi(e) : 6000; }();
  const bool by_side = (a->h < 5 || a->w < 5) && (p.P % 16 != 0 || p.P < 256);
  const int order = !a->parity ? 0 : (p.P <= smallp_maxp || by_side) ? 2 : 1;
  // persistent over pixel tiles: as many workgroups as are resident at once (256 CUs), every part the same share
  const bool small = p.nks_f <= 4 && p.nks_h <= 4, accum = p.acc_q || p.acc_p || p.gz_in != nullptr;
  const int resident = (order == 2 ? 512 : accum ? 768 : 1024) / parts;
  const int rounds = (p.ntiles + resident - 1) / resident;
  const int gx = (p.ntiles + rounds - 1) / rounds;  // every workgroup the same number of tiles: no half-empty last round
  const dim3 grid(gx, parts), block(256);
#define LT_LAUNCH(KF_, ACC_, ORD_) hipLaunchKernelGGL((latent_tail_bwd_kernel<KF_, ACC_, ORD_>), grid, block, lds, (hipStream_t)stream, p)
#define LT_ORDER(KF_, ACC_) do { if (order == 0) LT_LAUNCH(KF_, ACC_, 0); else if (order == 1) LT_LAUNCH(KF_, ACC_, 1); else LT_LAUNCH(KF_, ACC_, 2); } while (0)
  if (small) { if (accum) LT_ORDER(4, true); else LT_ORDER(4, false); }
  else { if (accum) LT_ORDER(LT_MAXKF, true); else LT_ORDER(LT_MAXKF, false); }
#undef LT_ORDER
#undef LT_LAUNCH
  return check_launch("cgen_latent_tail_bwd");
}
