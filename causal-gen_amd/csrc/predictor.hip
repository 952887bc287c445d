// Anticausal predictors of the parent SCMs (pgm/layers.py CNN in eval mode + flow_pgm.py model_anticausal likelihoods):
// forward (per-sample, per-variable -log p, optional head outputs) and input gradient, for counterfactual fine-tuning's
// aux_loss (dscm.py:78-88).  One workgroup per image runs every head of the PGM in turn; the activation stack of a head lives
// in LDS (fused path, 32x32 presets: 88 KiB at C = 1, 96 KiB at C = 3) or in a caller-owned global workspace (larger images).
// The convolutions are VALU FMA loops: at B = 256 the whole morphomnist forward is ~2 GMAC, the launch is latency-bound.
//
// Backward recomputes the head's forward, then walks back IN PLACE: the gradient of a layer's output overwrites that layer's
// post-activation once its LeakyReLU mask has been read (LeakyReLU keeps the sign, so the post-activation is the mask).  The
// heads' contributions to dx are added in head order by the same thread per element: no atomics, bit-identical reruns.
#include <float.h>

#include "common.h"

namespace cgen {
namespace {

constexpr int PNT = 512;                                // threads per workgroup (8 waves)
constexpr float PRED_EPS = 1.1920928955078125e-07f;     // torch clamp_probs: finfo(float32).eps
constexpr float PRED_LOGIT_MAX = 15.942384719848633f;   // logit(1 - eps): Bernoulli(probs=sigmoid(z)) sees clamp(z, -L, L)
constexpr float LEAK = 0.01f;
constexpr int HS_FEAT = 0, HS_HID = 288, HS_OUT = 544, HS_GOUT = 560, HS_TOTAL = 576;  // head scratch (floats): 8w + ctx <= 260

struct PredGeo {
  int c, r, w, s1, h1, pool, p, h2, h4, h6;
  int64_t a1, ap, a2, a3, a4, a5, a6, total;
};

__host__ __device__ inline PredGeo pred_geo(const cgen_pred_head& hd) {
  PredGeo g;
  g.c = hd.c; g.r = hd.res; g.w = hd.width;
  g.s1 = hd.res > 64 ? 2 : 1;
  g.h1 = (hd.res - 1) / g.s1 + 1;  // 7x7, pad 3
  g.pool = hd.res > 32;
  g.p = g.pool ? g.h1 / 2 : g.h1;
  g.h2 = (g.p - 1) / 2 + 1;  // 3x3, pad 1, stride 2
  g.h4 = (g.h2 - 1) / 2 + 1;
  g.h6 = (g.h4 - 1) / 2 + 1;
  const int64_t w = g.w;
  int64_t o = 0;
  g.a1 = o; o += w * g.h1 * g.h1;
  g.ap = o; o += g.pool ? w * g.p * g.p : 0;
  g.a2 = o; o += 2 * w * g.h2 * g.h2;
  g.a3 = o; o += 2 * w * g.h2 * g.h2;
  g.a4 = o; o += 4 * w * g.h4 * g.h4;
  g.a5 = o; o += 4 * w * g.h4 * g.h4;
  g.a6 = o; o += 8 * w * g.h6 * g.h6;
  g.total = (o + 3) & ~(int64_t)3;
  return g;
}

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : LEAK * v; }
__device__ __forceinline__ float lrelu_d(float post) { return post > 0.f ? 1.f : LEAK; }

// out[co][p] = lrelu(bias[co] + sum_{ci,ky,kx} wt[co][ci][ky][kx] * in[ci][oy*S-K/2+ky][ox*S-K/2+kx]); COB output channels per
// thread, pixels on the lanes (padded to whole waves so that the channel group, and with it the weight address, is wave-uniform)
template <int K, int COB>
__device__ void conv_fwd(const float* in, int cin, int hin, float* out, int cout, int hout, int S, const float* __restrict__ wt,
                         const float* __restrict__ bias) {
  const int hw = hout * hout, hwp = (hw + 63) & ~63, ng = cout / COB;
  for (int t = threadIdx.x; t < ng * hwp; t += PNT) {
    const int g = __builtin_amdgcn_readfirstlane(t / hwp), p = t - g * hwp;
    if (p >= hw) continue;
    const int oy = p / hout, ox = p - oy * hout, iy0 = oy * S - K / 2, ix0 = ox * S - K / 2;
    float acc[COB];
#pragma unroll
    for (int j = 0; j < COB; ++j) acc[j] = bias[g * COB + j];
    for (int ci = 0; ci < cin; ++ci) {
      const float* ip = in + (int64_t)ci * hin * hin;
      const float* wp = wt + ((int64_t)g * COB * cin + ci) * K * K;
#pragma unroll 1  // (unrolling both taps puts K*K*COB weight loads in flight: 248 VGPRs and scratch)
      for (int ky = 0; ky < K; ++ky) {
        const int iy = iy0 + ky;
        if (iy < 0 || iy >= hin) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ix0 + kx;
          if (ix < 0 || ix >= hin) continue;
          const float v = ip[iy * hin + ix];
#pragma unroll
          for (int j = 0; j < COB; ++j) acc[j] = fmaf(wp[(int64_t)j * cin * K * K + ky * K + kx], v, acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < COB; ++j) out[(int64_t)(g * COB + j) * hw + p] = lrelu(acc[j]);
  }
}

// Data gradient of conv_fwd: gi[ci][iy][ix] = sum_{co,ky,kx : iy = oy*S-K/2+ky, ix = ...} wt[co][ci][ky][kx] * gout[co][oy][ox]
// (gout = gradient of the PRE-activation).  MODE 0: dst holds the input's post-activation; it becomes gi * lrelu'(dst).
// MODE 1: dst = gi (the input is a max-pool output: no activation).  MODE 2: dst = gi (first) or dst += gi (global dx).
template <int K, int CIB, int MODE>
__device__ void conv_bwd(const float* gout, int cout, int hout, float* dst, int cin, int hin, int S, const float* __restrict__ wt,
                         bool first) {
  const int hw = hin * hin, hwp = (hw + 63) & ~63, ng = cin / CIB;
  for (int t = threadIdx.x; t < ng * hwp; t += PNT) {
    const int g = __builtin_amdgcn_readfirstlane(t / hwp), p = t - g * hwp;
    if (p >= hw) continue;
    const int iy = p / hin, ix = p - iy * hin;
    float acc[CIB];
#pragma unroll
    for (int j = 0; j < CIB; ++j) acc[j] = 0.f;
    for (int co = 0; co < cout; ++co) {
      const float* gp = gout + (int64_t)co * hout * hout;
      const float* wp = wt + ((int64_t)co * cin + g * CIB) * K * K;
#pragma unroll 1  // (unrolling both taps puts K*K*COB weight loads in flight: 248 VGPRs and scratch)
      for (int ky = 0; ky < K; ++ky) {
        const int ty = iy + K / 2 - ky;
        if (ty < 0 || ty % S) continue;
        const int oy = ty / S;
        if (oy >= hout) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int tx = ix + K / 2 - kx;
          if (tx < 0 || tx % S) continue;
          const int ox = tx / S;
          if (ox >= hout) continue;
          const float gv = gp[oy * hout + ox];
#pragma unroll
          for (int j = 0; j < CIB; ++j) acc[j] = fmaf(wp[(int64_t)j * K * K + ky * K + kx], gv, acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CIB; ++j) {
      float* d = dst + (int64_t)(g * CIB + j) * hw + p;
      if (MODE == 0) *d = acc[j] * lrelu_d(*d);
      else if (MODE == 1 || first) *d = acc[j];
      else *d += acc[j];
    }
  }
}

// MaxPool2d(2, 2): the first maximum of the window in row-major order (what torch selects)
__device__ __forceinline__ int pool_argmax(const float* a, int h1, int py, int px) {
  const float* r0 = a + (2 * py) * h1 + 2 * px;
  float best = r0[0];
  int k = 0;
  if (r0[1] > best) { best = r0[1]; k = 1; }
  if (r0[h1] > best) { best = r0[h1]; k = 2; }
  if (r0[h1 + 1] > best) k = 3;
  return k;
}

__device__ void maxpool_fwd(const float* a1, int c, int h1, float* ap, int p) {
  for (int t = threadIdx.x; t < c * p * p; t += PNT) {
    const int ch = t / (p * p), q = t - ch * p * p, py = q / p, px = q - py * p;
    const float* a = a1 + (int64_t)ch * h1 * h1;
    const int k = pool_argmax(a, h1, py, px);
    ap[t] = a[(2 * py + (k >> 1)) * h1 + 2 * px + (k & 1)];
  }
}

// a1 (post-activation) <- d/d pre-activation of the 7x7 conv, from gp = d/d pool output; each window is owned by one thread
__device__ void maxpool_bwd(float* a1, int c, int h1, const float* gp, int p) {
  for (int t = threadIdx.x; t < c * h1 * h1; t += PNT) {  // rows / columns no window covers (odd h1)
    const int q = t % (h1 * h1), y = q / h1, x = q - y * h1;
    if (y >= 2 * p || x >= 2 * p) a1[t] = 0.f;
  }
  for (int t = threadIdx.x; t < c * p * p; t += PNT) {
    const int ch = t / (p * p), q = t - ch * p * p, py = q / p, px = q - py * p;
    float* a = a1 + (int64_t)ch * h1 * h1;
    const int k = pool_argmax(a, h1, py, px);
    const float g = gp[t];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float* d = a + (2 * py + (e >> 1)) * h1 + 2 * px + (e & 1);
      *d = e == k ? g * lrelu_d(*d) : 0.f;
    }
  }
}

}  // namespace

// -log p(obs | head outputs o) of one sample (flow_pgm.py model_anticausal) and, if d != NULL, its gradient w.r.t. o.
// The one place the likelihoods live: the forward and the backward launches both call it.
__device__ float pred_nll(const cgen_pred_head& hd, const float* o, const float* obs, float* d) {
  if (hd.kind == CGEN_PRED_NORMAL) {
    const float raw = o[0], loc = hd.tanh_loc ? tanhf(raw) : raw, ls = o[1];
    float sc, dsc;
    if (hd.std_fixed > 0.f) { sc = hd.std_fixed; dsc = 0.f; }
    else if (ls > 20.f) { sc = ls; dsc = 1.f; }  // F.softplus threshold 20
    else { sc = log1pf(expf(ls)); dsc = 1.f / (1.f + expf(-ls)); }
    const float z = (obs[0] - loc) / sc;
    if (d) {
      const float dloc = -z / sc;
      d[0] = hd.tanh_loc ? dloc * (1.f - loc * loc) : dloc;
      d[1] = (1.f - z * z) / sc * dsc;
    }
    return 0.5f * z * z + logf(sc) + 0.91893853320467274f;
  }
  if (hd.kind == CGEN_PRED_CATEGORICAL) {
    int k = 0;
    float m = o[0], vk = obs[0];
    for (int j = 1; j < hd.nout; ++j) {
      m = fmaxf(m, o[j]);
      if (obs[j] > vk) { vk = obs[j]; k = j; }
    }
    float s = 0.f;
    for (int j = 0; j < hd.nout; ++j) s += expf(o[j] - m);
    const float pk = expf(o[k] - m) / s;
    const bool sat = pk < PRED_EPS || pk > 1.f - PRED_EPS;  // clamp_probs: constant there, zero gradient
    if (d)
      for (int j = 0; j < hd.nout; ++j) d[j] = sat ? 0.f : expf(o[j] - m) / s - (j == k ? 1.f : 0.f);
    if (pk < PRED_EPS) return -logf(PRED_EPS);
    if (pk > 1.f - PRED_EPS) return -logf(1.f - PRED_EPS);
    return logf(s) - (o[k] - m);
  }
  // Bernoulli(probs=sigmoid(z)): binary_cross_entropy_with_logits at the clamped logit
  const float z = o[0], zc = fminf(fmaxf(z, -PRED_LOGIT_MAX), PRED_LOGIT_MAX), v = obs[0];
  if (d) d[0] = (z > -PRED_LOGIT_MAX && z < PRED_LOGIT_MAX) ? 1.f / (1.f + expf(-zc)) - v : 0.f;
  return fmaxf(zc, 0.f) - zc * v + log1pf(expf(-fabsf(zc)));
}

namespace {

struct PredArgs {
  cgen_pred_head hd[CGEN_PRED_MAX_HEADS];
  int32_t nheads, n;
  const float* x;
  float* ws;
  int64_t ws_img, lds_x;
  float* terms;
  float* outs;
  const float* coef;
  float* dx;
};

template <bool BWD, bool GWS>
__global__ __launch_bounds__(PNT) void predictor_kernel(PredArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pred_lds[];
  __shared__ float hs[HS_TOTAL];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cx = a.hd[0].c, R = a.hd[0].res;
  const int64_t xs = (int64_t)cx * R * R;
  const float* xg = a.x + (int64_t)b * xs;
  const float* X;
  float* base;
  if (GWS) {
    X = xg;
    base = a.ws + (int64_t)b * a.ws_img;
  } else {
    for (int64_t i = tid; i < xs; i += PNT) pred_lds[i] = xg[i];
    X = pred_lds;
    base = pred_lds + a.lds_x;
  }
  __syncthreads();
  float* feat = hs + HS_FEAT;
  float* hid = hs + HS_HID;
  float* out = hs + HS_OUT;
  float* gout = hs + HS_GOUT;
  for (int h = 0; h < a.nheads; ++h) {
    const cgen_pred_head& hd = a.hd[h];
    const PredGeo g = pred_geo(hd);
    const int w = g.w;
    float *A1 = base + g.a1, *Ap = base + g.ap, *A2 = base + g.a2, *A3 = base + g.a3, *A4 = base + g.a4, *A5 = base + g.a5,
          *A6 = base + g.a6;
    const float* P = g.pool ? Ap : A1;
    // ---- trunk
    conv_fwd<7, 8>(X, cx, R, A1, w, g.h1, g.s1, hd.w[0], hd.b[0]);
    __syncthreads();
    if (g.pool) {
      maxpool_fwd(A1, w, g.h1, Ap, g.p);
      __syncthreads();
    }
    conv_fwd<3, 8>(P, w, g.p, A2, 2 * w, g.h2, 2, hd.w[1], hd.b[1]);
    __syncthreads();
    conv_fwd<3, 8>(A2, 2 * w, g.h2, A3, 2 * w, g.h2, 1, hd.w[2], hd.b[2]);
    __syncthreads();
    conv_fwd<3, 8>(A3, 2 * w, g.h2, A4, 4 * w, g.h4, 2, hd.w[3], hd.b[3]);
    __syncthreads();
    conv_fwd<3, 8>(A4, 4 * w, g.h4, A5, 4 * w, g.h4, 1, hd.w[4], hd.b[4]);
    __syncthreads();
    conv_fwd<3, 8>(A5, 4 * w, g.h4, A6, 8 * w, g.h6, 2, hd.w[5], hd.b[5]);
    __syncthreads();
    // ---- spatial mean, context, fc
    const int nf = 8 * w, hw6 = g.h6 * g.h6;
    for (int c = tid; c < nf + hd.ctx; c += PNT) {
      if (c < nf) {
        float s = 0.f;
        for (int q = 0; q < hw6; ++q) s += A6[c * hw6 + q];
        feat[c] = s / (float)hw6;
      } else {
        feat[c] = hd.y[(int64_t)b * hd.ctx + (c - nf)];
      }
    }
    __syncthreads();
    const int nin = nf + hd.ctx;
    for (int j = tid; j < nf; j += PNT) {
      const float* wr = hd.w[6] + (int64_t)j * nin;
      float s = hd.b[6][j];
      for (int i = 0; i < nin; ++i) s = fmaf(wr[i], feat[i], s);
      hid[j] = lrelu(s);
    }
    __syncthreads();
    if (tid < hd.nout) {
      const float* wr = hd.w[7] + (int64_t)tid * nf;
      float s = hd.b[7][tid];
      for (int j = 0; j < nf; ++j) s = fmaf(wr[j], hid[j], s);
      out[tid] = s;
    }
    __syncthreads();
    if (!BWD) {
      if (tid == 0) {
        if (a.terms) a.terms[(int64_t)b * a.nheads + h] = pred_nll(hd, out, hd.obs + (int64_t)b * hd.obs_stride, nullptr);
        if (a.outs)
          for (int o = 0; o < hd.nout; ++o) a.outs[((int64_t)h * a.n + b) * CGEN_PRED_MAX_OUT + o] = out[o];
      }
      __syncthreads();
      continue;
    }
    // ---- backward: loss -> fc -> mean -> trunk -> dx
    if (tid == 0) {
      pred_nll(hd, out, hd.obs + (int64_t)b * hd.obs_stride, gout);
      const float cf = a.coef[0];
      for (int o = 0; o < hd.nout; ++o) gout[o] *= cf;
    }
    __syncthreads();
    for (int j = tid; j < nf; j += PNT) {
      float s = 0.f;
      for (int o = 0; o < hd.nout; ++o) s = fmaf(hd.w[7][(int64_t)o * nf + j], gout[o], s);
      hid[j] = s * lrelu_d(hid[j]);
    }
    __syncthreads();
    for (int i = tid; i < nf; i += PNT) {
      float s = 0.f;
      for (int j = 0; j < nf; ++j) s = fmaf(hd.w[6][(int64_t)j * nin + i], hid[j], s);
      feat[i] = s / (float)hw6;
    }
    __syncthreads();
    for (int t = tid; t < nf * hw6; t += PNT) A6[t] = feat[t / hw6] * lrelu_d(A6[t]);
    __syncthreads();
    conv_bwd<3, 8, 0>(A6, 8 * w, g.h6, A5, 4 * w, g.h4, 2, hd.w[5], false);
    __syncthreads();
    conv_bwd<3, 8, 0>(A5, 4 * w, g.h4, A4, 4 * w, g.h4, 1, hd.w[4], false);
    __syncthreads();
    conv_bwd<3, 8, 0>(A4, 4 * w, g.h4, A3, 2 * w, g.h2, 2, hd.w[3], false);
    __syncthreads();
    conv_bwd<3, 8, 0>(A3, 2 * w, g.h2, A2, 2 * w, g.h2, 1, hd.w[2], false);
    __syncthreads();
    if (g.pool) {
      conv_bwd<3, 8, 1>(A2, 2 * w, g.h2, Ap, w, g.p, 2, hd.w[1], false);
      __syncthreads();
      maxpool_bwd(A1, w, g.h1, Ap, g.p);
    } else {
      conv_bwd<3, 8, 0>(A2, 2 * w, g.h2, A1, w, g.h1, 2, hd.w[1], false);
    }
    __syncthreads();
    conv_bwd<7, 1, 2>(A1, w, g.h1, a.dx + (int64_t)b * xs, cx, R, g.s1, hd.w[0], h == 0);
    __syncthreads();
  }
}

// loss[0] = sum of terms[0..count): per-thread strided partials, then a fixed tree (same order on every run)
__global__ __launch_bounds__(256) void pred_sum_kernel(const float* terms, int64_t count, float* loss) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < count; i += 256) s += terms[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0];
}

constexpr int64_t PRED_LDS_MAX = 160 * 1024 - HS_TOTAL * 4 - 1024;

int pred_validate(const char* fn, const cgen_pred_head* heads, int nheads, int n, const float* x, bool need_obs) {
  CGEN_REQUIRE(heads && nheads >= 1 && nheads <= CGEN_PRED_MAX_HEADS, "%s: need 1..%d head records", fn, CGEN_PRED_MAX_HEADS);
  CGEN_REQUIRE(n >= 1 && x, "%s: bad batch or null image", fn);
  for (int h = 0; h < nheads; ++h) {
    const cgen_pred_head& hd = heads[h];
    CGEN_REQUIRE(hd.c >= 1 && hd.c <= 4 && hd.res >= 8 && hd.res <= 512, "%s: head %d: unsupported input shape (%d, %d, %d)", fn, h,
                 hd.c, hd.res, hd.res);
    CGEN_REQUIRE(hd.c == heads[0].c && hd.res == heads[0].res, "%s: head %d: input shape differs from head 0", fn, h);
    CGEN_REQUIRE(hd.width >= 8 && hd.width <= 32 && hd.width % 8 == 0, "%s: head %d: unsupported width %d (8, 16, 24 or 32)", fn, h,
                 hd.width);
    CGEN_REQUIRE(hd.kind == CGEN_PRED_NORMAL || hd.kind == CGEN_PRED_CATEGORICAL || hd.kind == CGEN_PRED_BERNOULLI,
                 "%s: head %d: unknown variable kind %d", fn, h, hd.kind);
    const int want = hd.kind == CGEN_PRED_NORMAL ? 2 : hd.kind == CGEN_PRED_BERNOULLI ? 1 : -1;
    CGEN_REQUIRE(hd.nout >= 1 && hd.nout <= CGEN_PRED_MAX_OUT && (want < 0 ? hd.nout >= 2 : hd.nout == want),
                 "%s: head %d: %d outputs do not fit variable kind %d", fn, h, hd.nout, hd.kind);
    CGEN_REQUIRE(hd.ctx >= 0 && hd.ctx <= 4 && (hd.ctx > 0) == (hd.y != nullptr), "%s: head %d: context mismatch (ctx %d, y %s)", fn, h,
                 hd.ctx, hd.y ? "set" : "null");
    for (int i = 0; i < 8; ++i)
      CGEN_REQUIRE(hd.w[i] && hd.b[i], "%s: head %d: null weight pointer (layer %d)", fn, h, i);
    if (need_obs)
      CGEN_REQUIRE(hd.obs && hd.obs_stride >= (hd.kind == CGEN_PRED_CATEGORICAL ? hd.nout : 1), "%s: head %d: null obs or bad obs_stride",
                   fn, h);
    CGEN_REQUIRE(hd.kind != CGEN_PRED_NORMAL || hd.std_fixed >= 0.f, "%s: head %d: negative std_fixed", fn, h);
  }
  return CGEN_OK;
}

int64_t pred_ws(const cgen_pred_head* heads, int nheads) {
  int64_t m = 0;
  for (int h = 0; h < nheads; ++h) {
    const int64_t t = pred_geo(heads[h]).total;
    if (t > m) m = t;
  }
  return m;
}

int64_t pred_lds_x(const cgen_pred_head* heads) { return ((int64_t)heads[0].c * heads[0].res * heads[0].res + 3) & ~(int64_t)3; }

bool pred_fused_ok(const cgen_pred_head* heads, int nheads) {
  for (int h = 0; h < nheads; ++h)
    if (pred_geo(heads[h]).pool) return false;
  return (pred_lds_x(heads) + pred_ws(heads, nheads)) * 4 <= PRED_LDS_MAX;
}

template <bool BWD>
int pred_launch(const char* fn, PredArgs& p, const cgen_pred_head* heads, cgen_stream_t stream) {
  if (p.ws) {
    hipLaunchKernelGGL((predictor_kernel<BWD, true>), dim3(p.n), dim3(PNT), 0, (hipStream_t)stream, p);
  } else {
    CGEN_REQUIRE(pred_fused_ok(heads, p.nheads), "%s: the fused path does not take these heads (%dx%dx%d, LDS %lld bytes): pass a workspace",
                 fn, heads[0].c, heads[0].res, heads[0].res, (long long)((pred_lds_x(heads) + pred_ws(heads, p.nheads)) * 4));
    const size_t lds = (size_t)(p.lds_x + p.ws_img) * 4;
    // (exactly what this launch needs: the kernel also has static LDS, so 160 KiB would be refused)
    const hipError_t ae = hipFuncSetAttribute((const void*)predictor_kernel<BWD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ae != hipSuccess) {
      (void)hipGetLastError();  // not sticky: the message below is the error
      return fail(CGEN_ELAUNCH, "%s: cannot raise the dynamic LDS limit to %zu bytes: %s", fn, lds, hipGetErrorString(ae));
    }
    hipLaunchKernelGGL((predictor_kernel<BWD, false>), dim3(p.n), dim3(PNT), lds, (hipStream_t)stream, p);
  }
  return check_launch(fn);
}

int pred_args(PredArgs& p, const cgen_pred_head* heads, int nheads, int n, const float* x, float* ws) {
  memset(&p, 0, sizeof(p));
  for (int h = 0; h < nheads; ++h) p.hd[h] = heads[h];
  p.nheads = nheads; p.n = n; p.x = x; p.ws = ws;
  p.ws_img = pred_ws(heads, nheads);
  p.lds_x = pred_lds_x(heads);
  return CGEN_OK;
}

}  // namespace
}  // namespace cgen

using namespace cgen;

extern "C" int cgen_predictor_supported(const cgen_pred_head* heads, int32_t nheads) {
  if (!heads || nheads < 1 || nheads > CGEN_PRED_MAX_HEADS) return 0;
  for (int h = 0; h < nheads; ++h)
    if (heads[h].c < 1 || heads[h].res < 8 || heads[h].width < 8 || heads[h].width > 32 || heads[h].width % 8) return 0;
  return pred_fused_ok(heads, nheads) ? 1 : 0;
}

extern "C" int cgen_predictor_workspace(const cgen_pred_head* heads, int32_t nheads, int64_t* floats_per_image) {
  CGEN_REQUIRE(floats_per_image, "cgen_predictor_workspace: null output");
  CGEN_REQUIRE(heads && nheads >= 1 && nheads <= CGEN_PRED_MAX_HEADS, "cgen_predictor_workspace: need 1..%d head records",
               CGEN_PRED_MAX_HEADS);
  for (int h = 0; h < nheads; ++h)
    CGEN_REQUIRE(heads[h].res >= 8 && heads[h].width >= 8, "cgen_predictor_workspace: head %d: unsupported shape", h);
  *floats_per_image = pred_ws(heads, nheads);
  return CGEN_OK;
}

extern "C" int cgen_predictor_fwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, float* terms,
                                  float* outs, float* loss, cgen_stream_t stream) {
  int rc = pred_validate("cgen_predictor_fwd", heads, nheads, n, x, terms != nullptr);
  if (rc) return rc;
  CGEN_REQUIRE(terms || outs, "cgen_predictor_fwd: nothing to write (terms and outs are null)");
  CGEN_REQUIRE(!loss || terms, "cgen_predictor_fwd: loss needs terms");
  PredArgs p;
  pred_args(p, heads, nheads, n, x, ws);
  p.terms = terms; p.outs = outs;
  rc = pred_launch<false>("cgen_predictor_fwd", p, heads, stream);
  if (rc || !loss) return rc;
  hipLaunchKernelGGL(pred_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, (int64_t)n * nheads, loss);
  return check_launch("cgen_predictor_fwd (sum)");
}

extern "C" int cgen_predictor_bwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws,
                                  const float* coef_dev, float* dx, cgen_stream_t stream) {
  int rc = pred_validate("cgen_predictor_bwd", heads, nheads, n, x, true);
  if (rc) return rc;
  CGEN_REQUIRE(coef_dev && dx, "cgen_predictor_bwd: null coef_dev or dx");
  PredArgs p;
  pred_args(p, heads, nheads, n, x, ws);
  p.coef = coef_dev; p.dx = dx;
  return pred_launch<true>("cgen_predictor_bwd", p, heads, stream);
}
