// Anticausal predictors of the parent SCMs (pgm/layers.py CNN in eval mode + flow_pgm.py model_anticausal likelihoods):
// forward (per-sample, per-variable -log p, optional head outputs) and input gradient, for counterfactual fine-tuning's
// aux_loss (dscm.py:78-88).  Three placements.  Fused and workspace: one workgroup per image runs every head of the PGM in turn;
// the activation stack of a head lives in LDS (fused path, 32x32 presets: 88 KiB at C = 1, 96 KiB at C = 3) or in a caller-owned
// global workspace.  The convolutions are VALU FMA loops: at B = 256 the whole morphomnist forward is ~2 GMAC, the launch is
// latency-bound.  Tiled (second half of this file): one launch per layer over (tile x channel group x image x head), for the
// large images whose 32 workgroups would leave the chip idle.  Training mode (batch-statistic BatchNorm, parameter gradients) is
// predictor_train.inc, included at the end of this file: it shares the geometry, the likelihoods and the tiled data gradients.
// The scalar head that sees no image (pgm/layers.py MLP, encoder_a) is trained by predictor_mlp.inc, included after it: it
// shares the Normal likelihood.
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

// ============================================================================ tiled placement
// The same network, one launch per LAYER: the grid of a launch covers (output tile x channel group x image x head), so that a
// batch of 32 large images occupies the chip.  Activations are NCHW f32 planes in a caller-owned workspace, one pred_geo stack
// per (image, head) at ws + (b * nheads + h) * total; all heads have the same width, hence the same geometry.  A workgroup is
// 4 waves: the 64 lanes of a wave are an 8 x 8 patch of pixels, the waves are 4 groups of CT channels.  It stages its input
// tile (with halo) and its weight slice in LDS, chunk of channels by chunk, and keeps NP x NP pixels x CT channels per thread
// in registers.  The max-pool is not a launch: the first 3x3 conv pools the stem's planes while it stages them, and that
// conv's data gradient scatters into the stem's planes in its epilogue (each window is owned by one thread).
namespace {

constexpr int TNT = 256;  // threads per workgroup of the tiled kernels
constexpr int TCH = 8;    // channels staged per chunk (3x3 layers; every channel count is a multiple of 8)

struct TileArgs {
  cgen_pred_head hd[CGEN_PRED_MAX_HEADS];
  int32_t nheads, n;
  const float* x;
  float* ws;
  int64_t per;  // floats per (image, head)
  float* terms;
  float* outs;
  const float* coef;
  float* dx;
};

// LDS row pitch: the smallest p >= n with p % 16 == 8, so that the 4 pixel rows of a 32-lane group fall on distinct banks
__host__ __device__ constexpr int tile_pitch(int n) { return (n + 7) / 16 * 16 + 8; }
__host__ __device__ constexpr int floor_div(int a, int b) { return (a + 64 * b) / b - 64; }

struct TileLayer {
  int cin, cout, hin, hout, s;
  int64_t in, out;
};

// 3x3 layer L = 1..5 (index into the head's w[] / b[]); layer 1 reads the pooled stem where the pool exists
__host__ __device__ inline TileLayer tile_layer(const PredGeo& g, int L) {
  const int w = g.w;
  switch (L) {
    case 1: return {w, 2 * w, g.p, g.h2, 2, g.a1, g.a2};
    case 2: return {2 * w, 2 * w, g.h2, g.h2, 1, g.a2, g.a3};
    case 3: return {2 * w, 4 * w, g.h2, g.h4, 2, g.a3, g.a4};
    case 4: return {4 * w, 4 * w, g.h4, g.h4, 1, g.a4, g.a5};
    default: return {4 * w, 8 * w, g.h4, g.h6, 2, g.a5, g.a6};
  }
}

// channels per thread for a layer of `ch` channels (a multiple of 8): 4 * CT divides ch
inline int tile_ct(int ch) { return ch % 32 == 0 ? 8 : ch % 24 == 0 ? 6 : ch % 16 == 0 ? 4 : 2; }

__device__ __forceinline__ float pool_value(const float* plane, int h1, int py, int px) {
  const int k = pool_argmax(plane, h1, py, px);
  return plane[(2 * py + (k >> 1)) * h1 + 2 * px + (k & 1)];
}

// Forward conv K x K, stride S, pad K/2, + bias + LeakyReLU.  K == 7: the stem (layer 0, reads x); K == 3: layer L.
template <int K, int S, int NP, int CT, bool POOL>
__global__ __launch_bounds__(TNT) void ptile_conv_fwd(TileArgs a, int L) {
  constexpr int KP = (K + 3) & ~3, T = 8 * NP, IT = (T - 1) * S + K, IP = tile_pitch(IT), COW = 4 * CT, CIC = K == 7 ? 4 : TCH;
  __shared__ __attribute__((aligned(16))) float s_in[CIC * IT * IP];
  __shared__ __attribute__((aligned(16))) float s_w[COW * CIC * K * KP];
  const PredGeo g = pred_geo(a.hd[0]);
  TileLayer ly;
  if (K == 7) ly = {g.c, g.w, g.r, g.h1, g.s1, 0, g.a1};
  else ly = tile_layer(g, L);
  const int cin = ly.cin, cout = ly.cout, hin = ly.hin, hout = ly.hout;
  const int ntx = (hout + T - 1) / T, ntiles = ntx * ntx, ncog = (cout + COW - 1) / COW;
  int id = blockIdx.x;
  const int tile = id % ntiles;
  id /= ntiles;
  const int cog = id % ncog, pair = id / ncog, b = pair / a.nheads, h = pair - b * a.nheads;
  const cgen_pred_head& hd = a.hd[h];
  float* base = a.ws + (int64_t)pair * a.per;
  const float* in = K == 7 ? a.x + (int64_t)b * cin * hin * hin : base + ly.in;
  const float* __restrict__ wt = hd.w[L];
  const int tid = threadIdx.x, wave = tid >> 6, ty = (tid >> 3) & 7, tx = tid & 7;
  const int oy0 = (tile / ntx) * T, ox0 = (tile % ntx) * T, iy0 = oy0 * S - K / 2, ix0 = ox0 * S - K / 2;
  const int co0 = cog * COW + wave * CT;
  const int64_t plane = POOL ? (int64_t)g.h1 * g.h1 : (int64_t)hin * hin;
  float acc[CT][NP][NP];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int j = 0; j < NP; ++j) acc[t][i][j] = 0.f;
  for (int c0 = 0; c0 < cin; c0 += CIC) {
    if (c0) __syncthreads();
    for (int idx = tid; idx < CIC * IT * IT; idx += TNT) {
      const int ci = idx / (IT * IT), rem = idx - ci * (IT * IT), r = rem / IT, c = rem - r * IT;
      const int gy = iy0 + r, gx = ix0 + c;
      float v = 0.f;
      if (c0 + ci < cin && gy >= 0 && gy < hin && gx >= 0 && gx < hin) {
        const float* pl = in + (c0 + ci) * plane;
        v = POOL ? pool_value(pl, g.h1, gy, gx) : pl[gy * hin + gx];
      }
      s_in[(ci * IT + r) * IP + c] = v;
    }
    // weights: [co][ci][ky][kx padded to KP]; a co's CIC * K * K floats are contiguous in global memory
    for (int idx = tid; idx < COW * CIC * K * K; idx += TNT) {
      const int j = idx / (CIC * K * K), rem = idx - j * (CIC * K * K), ci = rem / (K * K), tap = rem - ci * (K * K);
      const int ky = tap / K, kx = tap - ky * K, co = cog * COW + j;
      s_w[((j * CIC + ci) * K + ky) * KP + kx] = (co < cout && c0 + ci < cin) ? wt[((int64_t)co * cin + c0 + ci) * (K * K) + tap] : 0.f;
    }
    __syncthreads();
    const int nci = min(CIC, cin - c0);
    for (int ci = 0; ci < nci; ++ci) {
      constexpr int KG = K == 3 ? 3 : 1;  // kernel rows whose inputs are held in registers at a time
#pragma unroll 1
      for (int kg = 0; kg < K; kg += KG) {
        float v[NP][NP][KG][K];
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
          for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int ky = 0; ky < KG; ++ky)
#pragma unroll
              for (int kx = 0; kx < K; ++kx)
                v[i][j][ky][kx] = s_in[(ci * IT + (ty + 8 * i) * S + kg + ky) * IP + (tx + 8 * j) * S + kx];
#pragma unroll
        for (int t = 0; t < CT; ++t) {
          const float* wp = s_w + (((wave * CT + t) * CIC + ci) * K + kg) * KP;
#pragma unroll
          for (int ky = 0; ky < KG; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
              const float wv = wp[ky * KP + kx];
#pragma unroll
              for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int j = 0; j < NP; ++j) acc[t][i][j] = fmaf(wv, v[i][j][ky][kx], acc[t][i][j]);
            }
        }
      }
    }
  }
  float* out = base + ly.out;
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int co = co0 + t;
    if (co >= cout) continue;
    const float bv = hd.b[L][co];
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int oy = oy0 + ty + 8 * i, ox = ox0 + tx + 8 * j;
        if (oy < hout && ox < hout) out[(int64_t)co * hout * hout + oy * hout + ox] = lrelu(acc[t][i][j] + bv);
      }
  }
}

// One output channel's share of the data gradient of a K x K, stride-S conv for the S x S block of input pixels a thread owns:
// gw = the (HI - LO + 1)^2 window of that channel's output gradient around the block, wp = its [K][KP] weights.  Which taps
// reach which pixel of the block is known at compile time, so no lane tests a parity.
template <int K, int S>
struct Gather {
  static constexpr int LO = -((K / 2) / S), HI = (S - 1 + K / 2) / S, GW = HI - LO + 1, KP = (K + 3) & ~3;
  static __device__ __forceinline__ void step(float (&acc)[S][S], const float (&gw)[GW][GW], const float* wp) {
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const float wv = wp[ky * KP + kx];
#pragma unroll
        for (int py = 0; py < S; ++py)
#pragma unroll
          for (int px = 0; px < S; ++px)
            if ((py + K / 2 - ky + S * K) % S == 0 && (px + K / 2 - kx + S * K) % S == 0)
              acc[py][px] = fmaf(wv, gw[floor_div(py + K / 2 - ky, S) - LO][floor_div(px + K / 2 - kx, S) - LO], acc[py][px]);
      }
  }
};

// Data gradient of 3x3 layer L, gather form: a thread owns an S x S block of the layer's INPUT pixels for CT input channels.
// The layer's output planes hold d/d(pre-activation).  MODE 0: the input planes hold the post-activation and become
// gi * lrelu'(post).  MODE 1 (layer 1 behind the pool): gi is the gradient of the pooled plane; the thread scatters it to the
// first maximum of each window of the stem's planes (times lrelu') and zeroes the rest, rows / columns no window covers included.
template <int S, int CT, int MODE>
__global__ __launch_bounds__(TNT) void ptile_conv_bwd(TileArgs a, int L) {
  using G = Gather<3, S>;
  constexpr int K = 3, KP = 4, GT = 8 + G::GW - 1, GP = tile_pitch(GT), CIW = 4 * CT, COC = TCH;
  __shared__ __attribute__((aligned(16))) float s_g[COC * GT * GP];
  __shared__ __attribute__((aligned(16))) float s_w[COC * CIW * K * KP];
  const PredGeo g = pred_geo(a.hd[0]);
  const TileLayer ly = tile_layer(g, L);
  const int cin = ly.cin, cout = ly.cout, hin = ly.hin, hout = ly.hout;
  const int nb = (hin + S - 1) / S, ntx = (nb + 7) / 8, ntiles = ntx * ntx, ncig = (cin + CIW - 1) / CIW;
  int id = blockIdx.x;
  const int tile = id % ntiles;
  id /= ntiles;
  const int cig = id % ncig, pair = id / ncig, h = pair % a.nheads;
  const cgen_pred_head& hd = a.hd[h];
  float* base = a.ws + (int64_t)pair * a.per;
  const float* gout = base + ly.out;
  const float* __restrict__ wt = hd.w[L];
  const int tid = threadIdx.x, wave = tid >> 6, ty = (tid >> 3) & 7, tx = tid & 7;
  const int by0 = (tile / ntx) * 8, bx0 = (tile % ntx) * 8;
  float acc[CT][S][S];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) acc[t][i][j] = 0.f;
  for (int c0 = 0; c0 < cout; c0 += COC) {
    if (c0) __syncthreads();
    for (int idx = tid; idx < COC * GT * GT; idx += TNT) {
      const int co = idx / (GT * GT), rem = idx - co * (GT * GT), r = rem / GT, c = rem - r * GT;
      const int oy = by0 + G::LO + r, ox = bx0 + G::LO + c;
      s_g[(co * GT + r) * GP + c] =
          (c0 + co < cout && oy >= 0 && oy < hout && ox >= 0 && ox < hout) ? gout[(int64_t)(c0 + co) * hout * hout + oy * hout + ox] : 0.f;
    }
    // weights: [co][ci][ky][kx padded]; the CIW * 9 floats of one co are contiguous in global memory
    for (int idx = tid; idx < COC * CIW * 9; idx += TNT) {
      const int co = idx / (CIW * 9), rem = idx - co * (CIW * 9), j = rem / 9, tap = rem - j * 9, ci = cig * CIW + j;
      s_w[((co * CIW + j) * K + tap / 3) * KP + tap % 3] =
          (c0 + co < cout && ci < cin) ? wt[((int64_t)(c0 + co) * cin + ci) * 9 + tap] : 0.f;
    }
    __syncthreads();
    const int nco = min(COC, cout - c0);
    for (int co = 0; co < nco; ++co) {
      float gw[G::GW][G::GW];
#pragma unroll
      for (int r = 0; r < G::GW; ++r)
#pragma unroll
        for (int c = 0; c < G::GW; ++c) gw[r][c] = s_g[(co * GT + ty + r) * GP + tx + c];
#pragma unroll
      for (int t = 0; t < CT; ++t) G::step(acc[t], gw, s_w + ((co * CIW + wave * CT + t) * K) * KP);
    }
  }
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int ci = cig * CIW + wave * CT + t;
    if (ci >= cin) continue;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const int iy = (by0 + ty) * S + i, ix = (bx0 + tx) * S + j;
        if (iy >= hin || ix >= hin) continue;
        const float gi = acc[t][i][j];
        if (MODE == 0) {
          float* d = base + ly.in + (int64_t)ci * hin * hin + iy * hin + ix;
          *d = gi * lrelu_d(*d);
        } else {
          const int h1 = g.h1, p = g.p;
          float* pl = base + g.a1 + (int64_t)ci * h1 * h1;
          const int k = pool_argmax(pl, h1, iy, ix);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float* d = pl + (2 * iy + (e >> 1)) * h1 + 2 * ix + (e & 1);
            *d = e == k ? gi * lrelu_d(*d) : 0.f;
          }
          if (2 * p < h1) {
            if (ix == p - 1) pl[(2 * iy) * h1 + 2 * p] = 0.f, pl[(2 * iy + 1) * h1 + 2 * p] = 0.f;
            if (iy == p - 1) pl[(2 * p) * h1 + 2 * ix] = 0.f, pl[(2 * p) * h1 + 2 * ix + 1] = 0.f;
            if (ix == p - 1 && iy == p - 1) pl[(2 * p) * h1 + 2 * p] = 0.f;
          }
        }
      }
  }
}

// dx = data gradient of the 7x7 stem, summed over the heads IN HEAD ORDER inside the thread that owns the pixel (no atomics).
// The stem's planes hold d/d(pre-activation).  A workgroup owns a (16 S)^2 tile of one image: the 4 waves are 2 x 2 patches of
// 8 x 8 blocks of S x S pixels.
template <int S>
__global__ __launch_bounds__(TNT) void ptile_stem_bwd(TileArgs a) {
  using G = Gather<7, S>;
  constexpr int K = 7, KP = 8, GT = 16 + G::GW - 1, GP = tile_pitch(GT), COC = TCH;
  __shared__ __attribute__((aligned(16))) float s_g[COC * GT * GP];
  __shared__ __attribute__((aligned(16))) float s_w[COC * K * KP];
  const PredGeo g = pred_geo(a.hd[0]);
  const int cx = g.c, R = g.r, w = g.w, h1 = g.h1;
  const int nb = (R + S - 1) / S, ntx = (nb + 15) / 16, ntiles = ntx * ntx;
  const int tile = blockIdx.x % ntiles, b = blockIdx.x / ntiles;
  const int tid = threadIdx.x, wave = tid >> 6, ty = ((tid >> 3) & 7) + 8 * (wave >> 1), tx = (tid & 7) + 8 * (wave & 1);
  const int by0 = (tile / ntx) * 16, bx0 = (tile % ntx) * 16;
  for (int ci = 0; ci < cx; ++ci) {
    float acc[S][S];
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) acc[i][j] = 0.f;
    for (int h = 0; h < a.nheads; ++h) {
      const float* gout = a.ws + ((int64_t)b * a.nheads + h) * a.per + g.a1;
      const float* __restrict__ wt = a.hd[h].w[0];
      for (int c0 = 0; c0 < w; c0 += COC) {
        __syncthreads();
        for (int idx = tid; idx < COC * GT * GT; idx += TNT) {
          const int co = idx / (GT * GT), rem = idx - co * (GT * GT), r = rem / GT, c = rem - r * GT;
          const int oy = by0 + G::LO + r, ox = bx0 + G::LO + c;
          s_g[(co * GT + r) * GP + c] = (oy >= 0 && oy < h1 && ox >= 0 && ox < h1) ? gout[(int64_t)(c0 + co) * h1 * h1 + oy * h1 + ox] : 0.f;
        }
        for (int idx = tid; idx < COC * 49; idx += TNT) {
          const int co = idx / 49, tap = idx - co * 49;
          s_w[(co * K + tap / 7) * KP + tap % 7] = wt[((int64_t)(c0 + co) * cx + ci) * 49 + tap];
        }
        __syncthreads();
        for (int co = 0; co < COC; ++co) {
          float gw[G::GW][G::GW];
#pragma unroll
          for (int r = 0; r < G::GW; ++r)
#pragma unroll
            for (int c = 0; c < G::GW; ++c) gw[r][c] = s_g[(co * GT + ty + r) * GP + tx + c];
          G::step(acc, gw, s_w + co * K * KP);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const int iy = (by0 + ty) * S + i, ix = (bx0 + tx) * S + j;
        if (iy < R && ix < R) a.dx[(((int64_t)b * cx + ci) * R + iy) * R + ix] = acc[i][j];
      }
  }
}

// dot of a global row with an LDS vector by one wave: lanes stride the row, then a fixed xor tree (the same order on every run)
__device__ __forceinline__ float wave_dot(const float* __restrict__ row, const float* v, int n, int lane) {
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s = fmaf(row[i], v[i], s);
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// The tail of one (image, head): spatial mean, context, fc.0 + LeakyReLU, fc.3, pred_nll.  Forward: terms / outs.  Backward:
// the last conv's planes become d/d(pre-activation).
template <bool BWD>
__global__ __launch_bounds__(TNT) void ptile_tail(TileArgs a) {
  __shared__ float hs[HS_TOTAL];
  const int pair = blockIdx.x, b = pair / a.nheads, h = pair - b * a.nheads, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const cgen_pred_head& hd = a.hd[h];
  const PredGeo g = pred_geo(hd);
  float* A6 = a.ws + (int64_t)pair * a.per + g.a6;
  float *feat = hs + HS_FEAT, *hid = hs + HS_HID, *out = hs + HS_OUT, *gout = hs + HS_GOUT;
  const int nf = 8 * g.w, hw6 = g.h6 * g.h6, nin = nf + hd.ctx;
  for (int c = tid; c < nin; c += TNT) {
    if (c < nf) {
      float s = 0.f;
      for (int q = 0; q < hw6; ++q) s += A6[c * hw6 + q];
      feat[c] = s / (float)hw6;
    } else {
      feat[c] = hd.y[(int64_t)b * hd.ctx + (c - nf)];
    }
  }
  __syncthreads();
  for (int j = wave; j < nf; j += TNT / 64) {
    const float s = wave_dot(hd.w[6] + (int64_t)j * nin, feat, nin, lane);
    if (lane == 0) hid[j] = lrelu(s + hd.b[6][j]);
  }
  __syncthreads();
  for (int o = wave; o < hd.nout; o += TNT / 64) {
    const float s = wave_dot(hd.w[7] + (int64_t)o * nf, hid, nf, lane);
    if (lane == 0) out[o] = s + hd.b[7][o];
  }
  __syncthreads();
  if (!BWD) {
    if (tid == 0) {
      if (a.terms) a.terms[(int64_t)b * a.nheads + h] = pred_nll(hd, out, hd.obs + (int64_t)b * hd.obs_stride, nullptr);
      if (a.outs)
        for (int o = 0; o < hd.nout; ++o) a.outs[((int64_t)h * a.n + b) * CGEN_PRED_MAX_OUT + o] = out[o];
    }
    return;
  }
  if (tid == 0) {
    pred_nll(hd, out, hd.obs + (int64_t)b * hd.obs_stride, gout);
    const float cf = a.coef[0];
    for (int o = 0; o < hd.nout; ++o) gout[o] *= cf;
  }
  __syncthreads();
  for (int j = tid; j < nf; j += TNT) {
    float s = 0.f;
    for (int o = 0; o < hd.nout; ++o) s = fmaf(hd.w[7][(int64_t)o * nf + j], gout[o], s);
    hid[j] = s * lrelu_d(hid[j]);
  }
  __syncthreads();
  for (int i = tid; i < nf; i += TNT) {
    float s = 0.f;
    for (int j = 0; j < nf; ++j) s = fmaf(hd.w[6][(int64_t)j * nin + i], hid[j], s);
    feat[i] = s / (float)hw6;
  }
  __syncthreads();
  for (int t = tid; t < nf * hw6; t += TNT) A6[t] = feat[t / hw6] * lrelu_d(A6[t]);
}

// ---- host side of the tiled placement
bool tile_shapes_ok(const cgen_pred_head* heads, int nheads) {
  if (!heads || nheads < 1 || nheads > CGEN_PRED_MAX_HEADS) return false;
  for (int h = 0; h < nheads; ++h) {
    const cgen_pred_head& hd = heads[h];
    if (hd.c < 1 || hd.c > 4 || hd.res < 8 || hd.res > 512 || hd.width < 8 || hd.width > 32 || hd.width % 8) return false;
    if (hd.c != heads[0].c || hd.res != heads[0].res || hd.width != heads[0].width) return false;
  }
  return true;
}

int64_t tile_ws(const cgen_pred_head* heads, int nheads, int n) { return (int64_t)n * nheads * pred_geo(heads[0]).total; }

int tile_validate(const char* fn, const cgen_pred_head* heads, int nheads, int n, const float* x, const float* ws, int64_t ws_floats,
                  bool need_obs) {
  const int rc = pred_validate(fn, heads, nheads, n, x, need_obs);
  if (rc) return rc;
  for (int h = 1; h < nheads; ++h)
    CGEN_REQUIRE(heads[h].width == heads[0].width, "%s: head %d: width %d differs from head 0's %d (the tiled path needs equal widths)", fn,
                 h, heads[h].width, heads[0].width);
  CGEN_REQUIRE(ws, "%s: null workspace", fn);
  const int64_t need = tile_ws(heads, nheads, n);
  CGEN_REQUIRE(ws_floats >= need, "%s: workspace too small: %lld floats, need %lld", fn, (long long)ws_floats, (long long)need);
  CGEN_REQUIRE((int64_t)n * nheads * 4096 < INT32_MAX, "%s: batch %d is too large for one launch", fn, n);
  return CGEN_OK;
}

#define TILE_CT_SWITCH(ct, ...)                    \
  switch (ct) {                                    \
    case 2: { constexpr int CT = 2; __VA_ARGS__; } break; \
    case 4: { constexpr int CT = 4; __VA_ARGS__; } break; \
    case 6: { constexpr int CT = 6; __VA_ARGS__; } break; \
    default: { constexpr int CT = 8; __VA_ARGS__; } break; \
  }

#define TILE_LAUNCH(kern, blocks, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(blocks)), dim3(TNT), 0, st, __VA_ARGS__)

// ---- the plan of a launch: which instance, over how many workgroups.  One host function per launch; the launchers below and
// cgen_predictor_tiled_plan both read it, so what the plan entry reports is what runs.
enum { TILE_FWD = 0, TILE_BWD = 1, TILE_STEM_BWD = 2, TILE_TAIL = 3 };
struct TilePlan {
  int family, K, S, NP, CT, flag, L;  // flag: POOL of a forward conv, MODE of a data gradient, BWD of the tail
  int64_t blocks;
};

// the 7x7 stem: 4 * CT == width, one channel group
inline TilePlan tile_plan_stem(const PredGeo& g, int64_t pairs) {
  const int nt = (g.h1 + 15) / 16;
  return {TILE_FWD, 7, g.s1, 2, tile_ct(g.w), 0, 0, pairs * nt * nt};
}

// 3x3 layer L = 1..5
inline TilePlan tile_plan_fwd(const PredGeo& g, int L, int64_t pairs) {
  const TileLayer ly = tile_layer(g, L);
  const int ct = tile_ct(ly.cout), np = ly.hout > 12 ? 2 : 1, nt = (ly.hout + 8 * np - 1) / (8 * np);
  return {TILE_FWD, 3, ly.s, np, ct, L == 1 && g.pool ? 1 : 0, L, pairs * (ly.cout / (4 * ct)) * nt * nt};
}

inline TilePlan tile_plan_tail(int64_t pairs, bool bwd) { return {TILE_TAIL, 0, 0, 0, 0, bwd ? 1 : 0, 6, pairs}; }

// data gradient of 3x3 layer L
inline TilePlan tile_plan_bwd(const PredGeo& g, int L, int64_t pairs) {
  const TileLayer ly = tile_layer(g, L);
  const int ct = tile_ct(ly.cin), nb = (ly.hin + ly.s - 1) / ly.s, nt = (nb + 7) / 8;
  return {TILE_BWD, 3, ly.s, 0, ct, L == 1 && g.pool ? 1 : 0, L, pairs * (ly.cin / (4 * ct)) * nt * nt};
}

inline TilePlan tile_plan_stem_bwd(const PredGeo& g, int64_t n) {
  const int nb = (g.r + g.s1 - 1) / g.s1, nt = (nb + 15) / 16;
  return {TILE_STEM_BWD, 7, g.s1, 0, 0, 0, 0, n * nt * nt};
}

// every layer of the forward, stem to tail, into the workspace
template <bool BWD>
int tile_forward(const char* fn, const TileArgs& p, hipStream_t st) {
  const PredGeo g = pred_geo(p.hd[0]);
  const int64_t pairs = (int64_t)p.n * p.nheads;
  {
    const TilePlan pl = tile_plan_stem(g, pairs);
    TILE_CT_SWITCH(pl.CT, if (pl.S == 2) TILE_LAUNCH((ptile_conv_fwd<7, 2, 2, CT, false>), pl.blocks, p, 0);
                   else TILE_LAUNCH((ptile_conv_fwd<7, 1, 2, CT, false>), pl.blocks, p, 0));
  }
  for (int L = 1; L <= 5; ++L) {
    const TilePlan pl = tile_plan_fwd(g, L, pairs);
    const int np = pl.NP;
#define TILE_FWD3(S, NP, POOL) TILE_LAUNCH((ptile_conv_fwd<3, S, NP, CT, POOL>), pl.blocks, p, L)
    TILE_CT_SWITCH(pl.CT, if (pl.S == 1) { if (np == 2) TILE_FWD3(1, 2, false); else TILE_FWD3(1, 1, false); }
                   else if (pl.flag) { if (np == 2) TILE_FWD3(2, 2, true); else TILE_FWD3(2, 1, true); }
                   else { if (np == 2) TILE_FWD3(2, 2, false); else TILE_FWD3(2, 1, false); });
#undef TILE_FWD3
  }
  TILE_LAUNCH((ptile_tail<BWD>), tile_plan_tail(pairs, BWD).blocks, p);
  return check_launch(fn);
}

// data gradient of 3x3 layer L into the planes of layer L - 1 (the stem's, through the pool, for L == 1)
void tile_bwd_layer(const TileArgs& p, const PredGeo& g, int L, hipStream_t st) {
  const TilePlan pl = tile_plan_bwd(g, L, (int64_t)p.n * p.nheads);
  TILE_CT_SWITCH(pl.CT, if (pl.S == 1) TILE_LAUNCH((ptile_conv_bwd<1, CT, 0>), pl.blocks, p, L);
                 else if (pl.flag) TILE_LAUNCH((ptile_conv_bwd<2, CT, 1>), pl.blocks, p, L);
                 else TILE_LAUNCH((ptile_conv_bwd<2, CT, 0>), pl.blocks, p, L));
}

// dx from the stem's planes
void tile_bwd_stem(const TileArgs& p, const PredGeo& g, hipStream_t st) {
  const TilePlan pl = tile_plan_stem_bwd(g, p.n);
  if (pl.S == 2) TILE_LAUNCH((ptile_stem_bwd<2>), pl.blocks, p);
  else TILE_LAUNCH((ptile_stem_bwd<1>), pl.blocks, p);
}

int tile_backward(const char* fn, const TileArgs& p, hipStream_t st) {
  const PredGeo g = pred_geo(p.hd[0]);
  for (int L = 5; L >= 1; --L) tile_bwd_layer(p, g, L, st);
  tile_bwd_stem(p, g, st);
  return check_launch(fn);
}

void tile_args(TileArgs& p, const cgen_pred_head* heads, int nheads, int n, const float* x, float* ws) {
  memset(&p, 0, sizeof(p));
  for (int h = 0; h < nheads; ++h) p.hd[h] = heads[h];
  p.nheads = nheads; p.n = n; p.x = x; p.ws = ws;
  p.per = pred_geo(heads[0]).total;
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

extern "C" int cgen_predictor_tiled_supported(const cgen_pred_head* heads, int32_t nheads) { return tile_shapes_ok(heads, nheads) ? 1 : 0; }

extern "C" int cgen_predictor_tiled_workspace(const cgen_pred_head* heads, int32_t nheads, int32_t n, int64_t* floats) {
  CGEN_REQUIRE(floats, "cgen_predictor_tiled_workspace: null output");
  CGEN_REQUIRE(n >= 1, "cgen_predictor_tiled_workspace: bad batch %d", n);
  CGEN_REQUIRE(tile_shapes_ok(heads, nheads), "cgen_predictor_tiled_workspace: the tiled path does not take these heads");
  *floats = tile_ws(heads, nheads, n);
  return CGEN_OK;
}

extern "C" int cgen_predictor_tiled_plan(const cgen_pred_head* heads, int32_t nheads, int32_t n, int32_t* records, int32_t max,
                                         int32_t* count) {
  CGEN_REQUIRE(count, "cgen_predictor_tiled_plan: null count");
  CGEN_REQUIRE(n >= 1 && (int64_t)n * CGEN_PRED_MAX_HEADS * 4096 < INT32_MAX, "cgen_predictor_tiled_plan: bad batch %d", n);
  CGEN_REQUIRE(tile_shapes_ok(heads, nheads), "cgen_predictor_tiled_plan: the tiled path does not take these heads");
  CGEN_REQUIRE(!records || max >= 0, "cgen_predictor_tiled_plan: negative record capacity");
  const PredGeo g = pred_geo(heads[0]);
  const int64_t pairs = (int64_t)n * nheads;
  TilePlan pl[CGEN_PRED_PLAN_LAUNCHES];
  int k = 0;
  pl[k++] = tile_plan_stem(g, pairs);
  for (int L = 1; L <= 5; ++L) pl[k++] = tile_plan_fwd(g, L, pairs);
  pl[k++] = tile_plan_tail(pairs, false);
  for (int L = 5; L >= 1; --L) pl[k++] = tile_plan_bwd(g, L, pairs);
  pl[k++] = tile_plan_stem_bwd(g, n);
  *count = k;
  for (int i = 0; records && i < k && i < max; ++i) {
    int32_t* r = records + (int64_t)i * CGEN_PRED_PLAN_FIELDS;
    r[0] = pl[i].family; r[1] = pl[i].K; r[2] = pl[i].S; r[3] = pl[i].NP; r[4] = pl[i].CT; r[5] = pl[i].flag; r[6] = pl[i].L;
    r[7] = (int32_t)pl[i].blocks;
  }
  return CGEN_OK;
}

extern "C" int cgen_predictor_tiled_fwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws,
                                        int64_t ws_floats, float* terms, float* outs, float* loss, cgen_stream_t stream) {
  int rc = tile_validate("cgen_predictor_tiled_fwd", heads, nheads, n, x, ws, ws_floats, terms != nullptr);
  if (rc) return rc;
  CGEN_REQUIRE(terms || outs, "cgen_predictor_tiled_fwd: nothing to write (terms and outs are null)");
  CGEN_REQUIRE(!loss || terms, "cgen_predictor_tiled_fwd: loss needs terms");
  TileArgs p;
  tile_args(p, heads, nheads, n, x, ws);
  p.terms = terms; p.outs = outs;
  rc = tile_forward<false>("cgen_predictor_tiled_fwd", p, (hipStream_t)stream);
  if (rc || !loss) return rc;
  hipLaunchKernelGGL(pred_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, (int64_t)n * nheads, loss);
  return check_launch("cgen_predictor_tiled_fwd (sum)");
}

extern "C" int cgen_predictor_tiled_bwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws,
                                        int64_t ws_floats, const float* coef_dev, float* dx, cgen_stream_t stream) {
  int rc = tile_validate("cgen_predictor_tiled_bwd", heads, nheads, n, x, ws, ws_floats, true);
  if (rc) return rc;
  CGEN_REQUIRE(coef_dev && dx, "cgen_predictor_tiled_bwd: null coef_dev or dx");
  TileArgs p;
  tile_args(p, heads, nheads, n, x, ws);
  p.coef = coef_dev; p.dx = dx;
  rc = tile_forward<true>("cgen_predictor_tiled_bwd", p, (hipStream_t)stream);
  if (rc) return rc;
  return tile_backward("cgen_predictor_tiled_bwd", p, (hipStream_t)stream);
}

#include "predictor_train.inc"
#include "predictor_mlp.inc"
#include "predictor_resnet.inc"
#include "predictor_resnet_train.inc"
