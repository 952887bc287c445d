// ============================================================================ ChestPGM's anticausal heads (included at the end of predictor.hip)
// pgm/resnet.py ResNet18 with GroupNorm in eval mode, four Linear heads on ONE shared trunk, the likelihoods of flow_pgm.py's
// model_anticausal (pred_nll above) and the input gradient (include/cgen_hip.h, cgen_resnet_*).  f32, NHWC.
// The GEMM-shaped work is the library's own: the stride-1 3x3 convs and the 1x1 stride-2 identity convs are cgen_conv2d (CGEN_F32,
// the latter on a view with doubled strides), the 7x7 stride-2 stem and the three stride-2 3x3 convs are cgen_im2col_strided + a
// 1x1 cgen_conv2d, with cgen_col2im_strided on the way back.  What is new here is everything between the convs:
//   rn_gn_part / rn_gn_final    GroupNorm statistics per (image, group): chunk means and CENTRED sums of squares (two passes over
//                               the chunk), merged over the chunks in chunk order (Chan's update)
//   rn_gn_apply                 y = relu(gn(x) [+ identity | + gn_ds(x_ds)])
//   rn_pool_fwd / rn_pool_bwd   MaxPool2d(3, 2, 1), first maximum in row-major order; the backward recomputes the argmax (gather form)
//   rn_tail_fwd / rn_tail_bwd   spatial mean, the four Linears, pred_nll per head / d loss / d (last feature map)
//   rn_gnb_part / rn_gnb_final  sum(g gamma), sum(g gamma xhat) per (image, group), g masked by the ReLU that followed
//   rn_gnb_apply                dx of the GroupNorm, and the masked g itself for the residual fork
// Lanes own one 16-byte channel quad of a pixel (a group is 1, 2 or 4 quads).  Every sum runs in a fixed order: per-thread over
// its pixels, then over the threads of the group by the group's thread through LDS, then over the chunks by one thread.  No atomics.
// The two launch plans (rn_forward, rn_backward) take an optional RnTrain: the training arms of csrc/predictor_resnet_train.inc
// (Dropout, parameter gradients).  Without it they are the eval plans, launch for launch.
namespace cgen {
namespace {

constexpr int RN_CONVS = CGEN_RESNET_CONVS;
constexpr int RN_CHUNK = 256;      // pixels per partial of the group reductions
constexpr float RN_EPS = 1e-5f;
constexpr int RN_FEAT = 512;
constexpr int RN_TAIL_OUT = 8;     // floats per image of the tail's raw outputs kept for the backward (7 used)
// the heads in the order of terms / outs: sex, race, finding, age
__device__ const int RN_NOUT[4] = {1, 3, 1, 2};
__device__ const int RN_OFF[4] = {0, 1, 4, 5};
__device__ const int RN_KIND[4] = {CGEN_PRED_BERNOULLI, CGEN_PRED_CATEGORICAL, CGEN_PRED_BERNOULLI, CGEN_PRED_NORMAL};

// Where everything lives in the workspace (float offsets, all multiples of 4) for n images of res x res.
struct RnPlan {
  int n, res, h1, hp, hs[4];
  int conv_h[RN_CONVS], conv_c[RN_CONVS], groups[RN_CONVS];
  int64_t raw[RN_CONVS], stat[RN_CONVS];
  int64_t stem_act, pool, a1[8], y[8];
  int64_t col, part, sums, tail_out, g[3];
  int64_t total;
};

inline int rn_half(int h) { return (h - 1) / 2 + 1; }  // 7x7/s2/p3, 3x3/s2/p1 and 1x1/s2 alike
inline int rn_conv1(int k) { return 1 + 2 * k; }
inline int rn_conv2(int k) { return 2 + 2 * k; }
inline int rn_ds(int s) { return 16 + s; }  // s = 1..3
inline bool rn_has_ds(int k) { return k >= 2 && k % 2 == 0; }

void rn_plan(RnPlan& p, int n, int res) {
  p.n = n; p.res = res;
  p.h1 = rn_half(res); p.hp = rn_half(p.h1);
  p.hs[0] = p.hp;
  for (int s = 1; s < 4; ++s) p.hs[s] = rn_half(p.hs[s - 1]);
  p.conv_h[0] = p.h1; p.conv_c[0] = 64;
  for (int k = 0; k < 8; ++k) {
    const int s = k / 2;
    p.conv_h[rn_conv1(k)] = p.conv_h[rn_conv2(k)] = p.hs[s];
    p.conv_c[rn_conv1(k)] = p.conv_c[rn_conv2(k)] = 64 << s;
  }
  for (int s = 1; s < 4; ++s) { p.conv_h[rn_ds(s)] = p.hs[s]; p.conv_c[rn_ds(s)] = 64 << s; }
  int64_t o = 0;
  auto take = [&](int64_t floats) { const int64_t at = o; o += (floats + 3) / 4 * 4; return at; };
  const int64_t N = n;
  int64_t col = N * p.h1 * p.h1 * 56;
  for (int i = 0; i < RN_CONVS; ++i) {
    p.groups[i] = std::min(32, p.conv_c[i] / 4);
    p.raw[i] = take(N * p.conv_h[i] * p.conv_h[i] * p.conv_c[i]);
    p.stat[i] = take(N * p.groups[i] * 2);
  }
  p.stem_act = take(N * p.h1 * p.h1 * 64);
  p.pool = take(N * p.hp * p.hp * 64);
  for (int k = 0; k < 8; ++k) {
    const int s = k / 2;
    const int64_t sz = N * p.hs[s] * p.hs[s] * (64 << s);
    p.a1[k] = take(sz);
    p.y[k] = take(sz);
    if (rn_has_ds(k)) col = std::max(col, N * p.hs[s] * p.hs[s] * 9 * (32 << s));
  }
  p.col = take(col);
  const int64_t chunks = (p.h1 * p.h1 + RN_CHUNK - 1) / RN_CHUNK;
  p.part = take(N * chunks * 32 * 2);
  p.sums = take(N * 32 * 2);
  p.tail_out = take(N * RN_TAIL_OUT);
  for (int i = 0; i < 3; ++i) p.g[i] = take(N * p.h1 * p.h1 * 64);
  p.total = o;
}

// ---------------------------------------------------------------------------- GroupNorm: statistics and their backward mirror
struct RnRed {
  const float* x;      // raw conv output [n][hw][c]
  const float* g;      // backward: gradient w.r.t. the post-ReLU output
  const float* y;      // backward: that output (the ReLU mask is y > 0)
  const float* stat;   // backward: mean, rstd per (image, group)
  const float* gamma;  // backward
  float* part;         // [n][nchunks][G][2]
  int hw, c, cpg, nchunks;
};

// The sum of `v` over the threads of each group, by the group's thread in (pixel slot, quad) order; result in out[group].
__device__ __forceinline__ void rn_group_sum(float v, float* red, float* out, int Q, int PP, int qpg, int G, float scale) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  if (tid < G) {
    float t = 0.f;
    for (int pl = 0; pl < PP; ++pl)
      for (int j = 0; j < qpg; ++j) t += red[pl * Q + tid * qpg + j];
    out[tid] = t * scale;
  }
  __syncthreads();
}

template <bool BWD>
__global__ __launch_bounds__(256) void rn_gn_part(RnRed a) {
  __shared__ float red[256];
  __shared__ float r0[32], r1[32];
  const int tid = threadIdx.x, ch = blockIdx.x, img = blockIdx.y;
  const int Q = a.c >> 2, PP = 256 / Q, q = tid & (Q - 1), pl = tid / Q;
  const int qpg = a.cpg >> 2, G = a.c / a.cpg, grp = q / qpg;
  const int p0 = ch * RN_CHUNK, p1 = min(a.hw, p0 + RN_CHUNK);
  const int64_t base = (int64_t)img * a.hw * Q + q;  // in float4 units; pixel p is at base + p * Q
  const float4* x = (const float4*)a.x + base;
  float* dst = a.part + (((int64_t)img * a.nchunks + ch) * G) * 2;
  if (!BWD) {
    float s = 0.f;
    for (int p = p0 + pl; p < p1; p += PP) {
      const float4 v = x[(int64_t)p * Q];
      s += (v.x + v.y) + (v.z + v.w);
    }
    rn_group_sum(s, red, r0, Q, PP, qpg, G, 1.f / (float)((p1 - p0) * a.cpg));
    const float mean = r0[grp];
    s = 0.f;
    for (int p = p0 + pl; p < p1; p += PP) {
      const float4 v = x[(int64_t)p * Q];
      const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
      s += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    rn_group_sum(s, red, r1, Q, PP, qpg, G, 1.f);
    if (tid < G) { dst[2 * tid] = r0[tid]; dst[2 * tid + 1] = r1[tid]; }
  } else {
    const float4* g = (const float4*)a.g + base;
    const float4* y = (const float4*)a.y + base;
    const float4 gam = ((const float4*)a.gamma)[q];
    const float mean = a.stat[((int64_t)img * G + grp) * 2], rstd = a.stat[((int64_t)img * G + grp) * 2 + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int p = p0 + pl; p < p1; p += PP) {
      const float4 v = x[(int64_t)p * Q], gv = g[(int64_t)p * Q], yv = y[(int64_t)p * Q];
      const float t0 = yv.x > 0.f ? gv.x * gam.x : 0.f, t1 = yv.y > 0.f ? gv.y * gam.y : 0.f;
      const float t2 = yv.z > 0.f ? gv.z * gam.z : 0.f, t3 = yv.w > 0.f ? gv.w * gam.w : 0.f;
      s1 += (t0 + t1) + (t2 + t3);
      s2 += (t0 * ((v.x - mean) * rstd) + t1 * ((v.y - mean) * rstd)) + (t2 * ((v.z - mean) * rstd) + t3 * ((v.w - mean) * rstd));
    }
    rn_group_sum(s1, red, r0, Q, PP, qpg, G, 1.f);
    rn_group_sum(s2, red, r1, Q, PP, qpg, G, 1.f);
    if (tid < G) { dst[2 * tid] = r0[tid]; dst[2 * tid + 1] = r1[tid]; }
  }
}

// One thread per (image, group): the chunks' (mean, centred sum of squares) merged in chunk order -> mean, 1 / sqrt(var + eps)
__global__ __launch_bounds__(256) void rn_gn_final(const float* part, float* stat, int count, int G, int nchunks, int hw, int cpg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int img = i / G, g = i - img * G;
  float cnt = 0.f, mean = 0.f, m2 = 0.f;
  for (int ch = 0; ch < nchunks; ++ch) {
    const float* s = part + (((int64_t)img * nchunks + ch) * G + g) * 2;
    const float nb = (float)((min(hw, (ch + 1) * RN_CHUNK) - ch * RN_CHUNK) * cpg);
    const float delta = s[0] - mean, tot = cnt + nb;
    mean += delta * (nb / tot);
    m2 += s[1] + delta * delta * (cnt * nb / tot);
    cnt = tot;
  }
  stat[2 * i] = mean;
  stat[2 * i + 1] = 1.f / sqrtf(m2 / cnt + RN_EPS);
}

__global__ __launch_bounds__(256) void rn_gnb_final(const float* part, float* sums, int count, int G, int nchunks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int img = i / G, g = i - img * G;
  float s1 = 0.f, s2 = 0.f;
  for (int ch = 0; ch < nchunks; ++ch) {
    const float* s = part + (((int64_t)img * nchunks + ch) * G + g) * 2;
    s1 += s[0];
    s2 += s[1];
  }
  sums[2 * i] = s1;
  sums[2 * i + 1] = s2;
}

// ---------------------------------------------------------------------------- GroupNorm apply (+ identity | + second norm) + ReLU
struct RnApply {
  const float *x, *stat, *gamma, *beta;
  const float* idn;                         // optional: added as it is
  const float *x2, *stat2, *gamma2, *beta2; // optional: the normalised downsample branch
  float* y;
  int hw, c, cpg;
  int64_t total4;  // n * hw * c / 4
};

__device__ __forceinline__ float4 rn_norm4(const float4 v, float mean, float rstd, const float4 ga, const float4 be) {
  float4 o;
  o.x = (v.x - mean) * rstd * ga.x + be.x; o.y = (v.y - mean) * rstd * ga.y + be.y;
  o.z = (v.z - mean) * rstd * ga.z + be.z; o.w = (v.w - mean) * rstd * ga.w + be.w;
  return o;
}

__global__ __launch_bounds__(256) void rn_gn_apply(RnApply a) {
  const int Q = a.c >> 2, qpg = a.cpg >> 2, G = a.c / a.cpg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total4; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & (Q - 1));
    const int64_t pix = i / Q;
    const int img = (int)(pix / a.hw), grp = q / qpg;
    const float* st = a.stat + ((int64_t)img * G + grp) * 2;
    float4 o = rn_norm4(((const float4*)a.x)[i], st[0], st[1], ((const float4*)a.gamma)[q], ((const float4*)a.beta)[q]);
    if (a.idn) {
      const float4 r = ((const float4*)a.idn)[i];
      o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
    }
    if (a.x2) {
      const float* s2 = a.stat2 + ((int64_t)img * G + grp) * 2;
      const float4 r = rn_norm4(((const float4*)a.x2)[i], s2[0], s2[1], ((const float4*)a.gamma2)[q], ((const float4*)a.beta2)[q]);
      o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
    }
    o.x = o.x > 0.f ? o.x : 0.f; o.y = o.y > 0.f ? o.y : 0.f; o.z = o.z > 0.f ? o.z : 0.f; o.w = o.w > 0.f ? o.w : 0.f;
    ((float4*)a.y)[i] = o;
  }
}

struct RnApplyB {
  const float *x, *stat, *gamma, *sums, *g, *y;
  float* dx;      // gradient w.r.t. the raw conv output
  float* gm_out;  // optional: g masked by the ReLU (may be g itself)
  int hw, c, cpg;
  int64_t total4;
  float inv_m;    // 1 / (hw * cpg)
};

__global__ __launch_bounds__(256) void rn_gnb_apply(RnApplyB a) {
  const int Q = a.c >> 2, qpg = a.cpg >> 2, G = a.c / a.cpg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total4; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & (Q - 1));
    const int64_t pix = i / Q;
    const int img = (int)(pix / a.hw), grp = q / qpg;
    const int64_t sg = ((int64_t)img * G + grp) * 2;
    const float mean = a.stat[sg], rstd = a.stat[sg + 1], s1 = a.sums[sg] * a.inv_m, s2 = a.sums[sg + 1] * a.inv_m;
    const float4 v = ((const float4*)a.x)[i], gv = ((const float4*)a.g)[i], yv = ((const float4*)a.y)[i], ga = ((const float4*)a.gamma)[q];
    float4 gm, d;
    gm.x = yv.x > 0.f ? gv.x : 0.f; gm.y = yv.y > 0.f ? gv.y : 0.f; gm.z = yv.z > 0.f ? gv.z : 0.f; gm.w = yv.w > 0.f ? gv.w : 0.f;
    d.x = rstd * (gm.x * ga.x - (s1 + (v.x - mean) * rstd * s2));
    d.y = rstd * (gm.y * ga.y - (s1 + (v.y - mean) * rstd * s2));
    d.z = rstd * (gm.z * ga.z - (s1 + (v.z - mean) * rstd * s2));
    d.w = rstd * (gm.w * ga.w - (s1 + (v.w - mean) * rstd * s2));
    ((float4*)a.dx)[i] = d;
    if (a.gm_out) ((float4*)a.gm_out)[i] = gm;
  }
}

// ---------------------------------------------------------------------------- MaxPool2d(3, 2, 1) on 64 channels
// The window of output (oy, ox) is rows 2 oy - 1 .. 2 oy + 1, columns 2 ox - 1 .. 2 ox + 1 inside the image; the first maximum
// in row-major order wins (strict >, a NaN is taken as torch takes it).
__device__ __forceinline__ bool rn_better(float v, float best) { return v > best || v != v; }

__global__ __launch_bounds__(256) void rn_pool_fwd(const float* in, float* out, int h, int ho, int64_t total4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & 15);
    int64_t r = i >> 4;
    const int ox = (int)(r % ho); r /= ho;
    const int oy = (int)(r % ho);
    const int img = (int)(r / ho);
    const float4* src = (const float4*)in + (int64_t)img * h * h * 16 + q;
    const float ninf = -__builtin_inff();
    float4 b = {ninf, ninf, ninf, ninf};
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = 2 * oy + dy;
      if (yy < 0 || yy >= h) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = 2 * ox + dx;
        if (xx < 0 || xx >= h) continue;
        const float4 v = src[((int64_t)yy * h + xx) * 16];
        if (rn_better(v.x, b.x)) b.x = v.x;
        if (rn_better(v.y, b.y)) b.y = v.y;
        if (rn_better(v.z, b.z)) b.z = v.z;
        if (rn_better(v.w, b.w)) b.w = v.w;
      }
    }
    ((float4*)out)[i] = b;
  }
}

// gin[iy, ix] = sum over the (at most four) windows that hold the pixel and whose recomputed argmax it is, in (oy, ox) order.
__global__ __launch_bounds__(256) void rn_pool_bwd(const float* in, const float* gout, float* gin, int h, int ho, int64_t total4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & 15);
    int64_t r = i >> 4;
    const int ix = (int)(r % h); r /= h;
    const int iy = (int)(r % h);
    const int img = (int)(r / h);
    const float4* src = (const float4*)in + (int64_t)img * h * h * 16 + q;
    const float4* gsrc = (const float4*)gout + (int64_t)img * ho * ho * 16 + q;
    const int me = iy * h + ix;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = iy / 2; oy <= (iy + 1) / 2 && oy < ho; ++oy) {
      for (int ox = ix / 2; ox <= (ix + 1) / 2 && ox < ho; ++ox) {
        const float ninf = -__builtin_inff();
        float4 b = {ninf, ninf, ninf, ninf};
        int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = 2 * oy + dy;
          if (yy < 0 || yy >= h) continue;
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = 2 * ox + dx;
            if (xx < 0 || xx >= h) continue;
            const int at = yy * h + xx;
            const float4 v = src[(int64_t)at * 16];
            if (rn_better(v.x, b.x) || k0 < 0) { b.x = v.x; k0 = at; }
            if (rn_better(v.y, b.y) || k1 < 0) { b.y = v.y; k1 = at; }
            if (rn_better(v.z, b.z) || k2 < 0) { b.z = v.z; k2 = at; }
            if (rn_better(v.w, b.w) || k3 < 0) { b.w = v.w; k3 = at; }
          }
        }
        const float4 gv = gsrc[((int64_t)oy * ho + ox) * 16];
        if (k0 == me) acc.x += gv.x;
        if (k1 == me) acc.y += gv.y;
        if (k2 == me) acc.z += gv.z;
        if (k3 == me) acc.w += gv.w;
      }
    }
    ((float4*)gin)[i] = acc;
  }
}

// ---------------------------------------------------------------------------- the tail: spatial mean, four Linears, pred_nll
struct RnTail {
  const float* y;  // last feature map [n][hw][512]
  int hw;
  const float* fc_w[4];
  const float* fc_b[4];
  const float* obs[4];
  int obs_stride[4];
  const float* ctx;  // age's context column (finding), ctx[b * ctx_stride]
  int ctx_stride;
  float std_fixed;
  float* tail_out;  // [n][RN_TAIL_OUT]
  float* terms;
  float* outs;      // [4][n][CGEN_PRED_MAX_OUT]
  int n;
  const float* coef;
  float* g;         // backward: [n][hw][512]
};

__device__ __forceinline__ cgen_pred_head rn_head(const RnTail& a, int h) {
  cgen_pred_head hd;
  hd.kind = RN_KIND[h]; hd.nout = RN_NOUT[h]; hd.tanh_loc = 0; hd.std_fixed = a.std_fixed;
  return hd;
}

// a fixed tree over the 256 threads' values; every thread gets the sum
__device__ __forceinline__ float rn_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void rn_tail_fwd(RnTail a) {
  __shared__ float feat[RN_FEAT + 1];
  __shared__ float red[256];
  __shared__ float outv[RN_TAIL_OUT];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* y = a.y + (int64_t)b * a.hw * RN_FEAT;
  for (int c = tid; c < RN_FEAT; c += 256) {
    float s = 0.f;
    for (int p = 0; p < a.hw; ++p) s += y[(int64_t)p * RN_FEAT + c];
    feat[c] = s / (float)a.hw;
  }
  if (tid == 0) feat[RN_FEAT] = a.ctx ? a.ctx[(int64_t)b * a.ctx_stride] : 0.f;
  __syncthreads();
  for (int h = 0; h < 4; ++h) {
    const int nin = h == 3 ? RN_FEAT + 1 : RN_FEAT;
    for (int j = 0; j < RN_NOUT[h]; ++j) {
      const float* w = a.fc_w[h] + (int64_t)j * nin;
      float s = 0.f;
      for (int c = tid; c < nin; c += 256) s = fmaf(feat[c], w[c], s);
      const float t = rn_block_sum(s, red);
      if (tid == 0) outv[RN_OFF[h] + j] = t + a.fc_b[h][j];
    }
  }
  __syncthreads();
  if (tid < RN_TAIL_OUT) a.tail_out[(int64_t)b * RN_TAIL_OUT + tid] = tid < 7 ? outv[tid] : 0.f;
  if (tid < 4) {
    const int h = tid;
    if (a.outs)
      for (int j = 0; j < RN_NOUT[h]; ++j) a.outs[((int64_t)h * a.n + b) * CGEN_PRED_MAX_OUT + j] = outv[RN_OFF[h] + j];
    if (a.terms) {
      const cgen_pred_head hd = rn_head(a, h);
      a.terms[(int64_t)b * 4 + h] = pred_nll(hd, outv + RN_OFF[h], a.obs[h] + (int64_t)b * a.obs_stride[h], nullptr);
    }
  }
}

// g[b, p, c] = coef / hw * sum_{head, output} d term / d out * W[output][c], heads and outputs in order
__global__ __launch_bounds__(256) void rn_tail_bwd(RnTail a) {
  __shared__ float gout[RN_TAIL_OUT];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid < 4) {
    const int h = tid;
    const cgen_pred_head hd = rn_head(a, h);
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    pred_nll(hd, a.tail_out + (int64_t)b * RN_TAIL_OUT + RN_OFF[h], a.obs[h] + (int64_t)b * a.obs_stride[h], d);
    const float k = a.coef[0] / (float)a.hw;
    for (int j = 0; j < RN_NOUT[h]; ++j) gout[RN_OFF[h] + j] = d[j] * k;
  }
  __syncthreads();
  for (int c = tid; c < RN_FEAT; c += 256) {
    float s = 0.f;
    for (int h = 0; h < 4; ++h) {
      const int nin = h == 3 ? RN_FEAT + 1 : RN_FEAT;
      for (int j = 0; j < RN_NOUT[h]; ++j) s = fmaf(gout[RN_OFF[h] + j], a.fc_w[h][(int64_t)j * nin + c], s);
    }
    float* g = a.g + (int64_t)b * a.hw * RN_FEAT + c;
    for (int p = 0; p < a.hw; ++p) g[(int64_t)p * RN_FEAT] = s;
  }
}

// ---------------------------------------------------------------------------- host side: validation and the two launch plans
inline int rn_grid(int64_t items) { return (int)std::min<int64_t>((items + 255) / 256, 256 * 16); }

inline cgen_view rn_view(float* p, int h, int c, int cphys = 0) {
  cgen_view v;
  const int64_t cs = cphys ? cphys : c;
  v.p = p; v.sw = cs; v.sh = cs * h; v.sn = cs * h * h; v.c = c; v.cpad = cphys > c ? cphys : 0;
  return v;
}

int rn_validate(const char* who, const cgen_resnet_args* a, int n, const float* x, const char* xname, const float* ws, int64_t ws_floats,
                bool need_obs, RnPlan& p) {
  CGEN_REQUIRE(a, "%s: null args", who);
  CGEN_REQUIRE(n >= 1, "%s: n = %d, need n >= 1", who, n);
  CGEN_REQUIRE(a->res >= 32 && a->res <= 256, "%s: res = %d outside 32..256", who, a->res);
  CGEN_REQUIRE((int64_t)n * rn_half(a->res) * rn_half(a->res) * 64 < (1ll << 31), "%s: n = %d is too many images of res %d", who, n, a->res);
  CGEN_REQUIRE(x, "%s: null %s", who, xname);
  CGEN_REQUIRE(ws && ((uintptr_t)ws % 16) == 0, "%s: ws is null or not 16-byte aligned", who);
  rn_plan(p, n, a->res);
  CGEN_REQUIRE(ws_floats >= p.total, "%s: ws_floats = %lld, too small: need %lld", who, (long long)ws_floats, (long long)p.total);
  for (int i = 0; i < RN_CONVS; ++i) {
    CGEN_REQUIRE(a->img_fwd[i] && a->img_dg[i], "%s: null weight image %d (img_fwd / img_dg)", who, i);
    CGEN_REQUIRE(a->gamma[i] && a->beta[i] && ((uintptr_t)a->gamma[i] % 16) == 0 && ((uintptr_t)a->beta[i] % 16) == 0,
                 "%s: gamma / beta %d null or not 16-byte aligned", who, i);
  }
  for (int h = 0; h < 4; ++h) {
    CGEN_REQUIRE(a->fc_w[h] && a->fc_b[h], "%s: null fc_w / fc_b of head %d", who, h);
    if (need_obs) CGEN_REQUIRE(a->obs[h] && a->obs_stride[h] >= (h == 1 ? 3 : 1), "%s: obs of head %d null or its obs_stride too small", who, h);
  }
  CGEN_REQUIRE(a->ctx && a->ctx_stride >= 1, "%s: null ctx (the finding column of the age head) or ctx_stride < 1", who);
  return CGEN_OK;
}

#define RN_TRY(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

int rn_conv(const RnPlan& p, int h, int ks, cgen_view in, const void* img, cgen_view out, const cgen_view* res1, hipStream_t st) {
  cgen_conv_args c;
  memset(&c, 0, sizeof(c));
  c.dtype = CGEN_F32; c.n = p.n; c.h = h; c.w = h; c.ks = ks; c.nseg = 1; c.act = CGEN_ACT_NONE; c.dact = CGEN_ACT_NONE;
  c.seg[0] = in; c.weight = img; c.out = out;
  if (res1) c.res1 = *res1;
  return cgen_conv2d(&c, st);
}

int rn_stats(const RnPlan& p, int i, float* ws, hipStream_t st) {
  const int hw = p.conv_h[i] * p.conv_h[i], c = p.conv_c[i], G = p.groups[i], nchunks = (hw + RN_CHUNK - 1) / RN_CHUNK;
  RnRed r;
  memset(&r, 0, sizeof(r));
  r.x = ws + p.raw[i]; r.part = ws + p.part; r.hw = hw; r.c = c; r.cpg = c / G; r.nchunks = nchunks;
  hipLaunchKernelGGL(rn_gn_part<false>, dim3(nchunks, p.n), dim3(256), 0, st, r);
  hipLaunchKernelGGL(rn_gn_final, dim3((p.n * G + 255) / 256), dim3(256), 0, st, ws + p.part, ws + p.stat[i], p.n * G, G, nchunks, hw, c / G);
  return check_launch("cgen_resnet (GroupNorm statistics)");
}

// y = relu(gn_i(raw_i) [+ idn | + gn_i2(raw_i2)])
int rn_apply(const RnPlan& p, const cgen_resnet_args* a, int i, const float* idn, int i2, float* y, float* ws, hipStream_t st) {
  const int hw = p.conv_h[i] * p.conv_h[i], c = p.conv_c[i];
  RnApply q;
  memset(&q, 0, sizeof(q));
  q.x = ws + p.raw[i]; q.stat = ws + p.stat[i]; q.gamma = a->gamma[i]; q.beta = a->beta[i]; q.idn = idn;
  if (i2 >= 0) { q.x2 = ws + p.raw[i2]; q.stat2 = ws + p.stat[i2]; q.gamma2 = a->gamma[i2]; q.beta2 = a->beta[i2]; }
  q.y = y; q.hw = hw; q.c = c; q.cpg = c / p.groups[i]; q.total4 = (int64_t)p.n * hw * c / 4;
  hipLaunchKernelGGL(rn_gn_apply, dim3(rn_grid(q.total4)), dim3(256), 0, st, q);
  return check_launch("cgen_resnet (GroupNorm apply)");
}

// GroupNorm i backward: g (w.r.t. the post-ReLU output y) -> dx (w.r.t. raw_i); gm_out (optional) = g masked
int rn_gn_bwd(const RnPlan& p, const cgen_resnet_args* a, int i, const float* g, const float* y, float* dx, float* gm_out, float* ws,
              hipStream_t st) {
  const int hw = p.conv_h[i] * p.conv_h[i], c = p.conv_c[i], G = p.groups[i], nchunks = (hw + RN_CHUNK - 1) / RN_CHUNK;
  RnRed r;
  memset(&r, 0, sizeof(r));
  r.x = ws + p.raw[i]; r.g = g; r.y = y; r.stat = ws + p.stat[i]; r.gamma = a->gamma[i]; r.part = ws + p.part;
  r.hw = hw; r.c = c; r.cpg = c / G; r.nchunks = nchunks;
  hipLaunchKernelGGL(rn_gn_part<true>, dim3(nchunks, p.n), dim3(256), 0, st, r);
  hipLaunchKernelGGL(rn_gnb_final, dim3((p.n * G + 255) / 256), dim3(256), 0, st, ws + p.part, ws + p.sums, p.n * G, G, nchunks);
  RnApplyB q;
  memset(&q, 0, sizeof(q));
  q.x = r.x; q.stat = r.stat; q.gamma = r.gamma; q.sums = ws + p.sums; q.g = g; q.y = y; q.dx = dx; q.gm_out = gm_out;
  q.hw = hw; q.c = c; q.cpg = c / G; q.total4 = (int64_t)p.n * hw * c / 4; q.inv_m = 1.f / (float)(hw * (c / G));
  hipLaunchKernelGGL(rn_gnb_apply, dim3(rn_grid(q.total4)), dim3(256), 0, st, q);
  return check_launch("cgen_resnet (GroupNorm backward)");
}

void rn_tail_args(RnTail& t, const RnPlan& p, const cgen_resnet_args* a, float* ws) {
  memset(&t, 0, sizeof(t));
  t.y = ws + p.y[7]; t.hw = p.hs[3] * p.hs[3];
  for (int h = 0; h < 4; ++h) { t.fc_w[h] = a->fc_w[h]; t.fc_b[h] = a->fc_b[h]; t.obs[h] = a->obs[h]; t.obs_stride[h] = a->obs_stride[h]; }
  t.ctx = a->ctx; t.ctx_stride = a->ctx_stride; t.std_fixed = a->std_fixed; t.tail_out = ws + p.tail_out; t.n = p.n;
}

// the input of block k, its channels and its map size
inline void rn_block_in(const RnPlan& p, int k, int64_t& off, int& cin, int& hin) {
  off = k == 0 ? p.pool : p.y[k - 1];
  const int s = k / 2;
  cin = rn_has_ds(k) ? 32 << s : 64 << s;
  hin = rn_has_ds(k) ? p.hs[s - 1] : p.hs[s];
}

// The training arms of the two plans (csrc/predictor_resnet_train.inc).  tr == nullptr: the eval plans, launch for launch.
struct RnTrain;
int rn_tr_dropout(const RnTrain& tr, const RnPlan& p, int k, float* ws, hipStream_t st);
int rn_tr_unscale(const RnTrain& tr, const RnPlan& p, int k, float* g, hipStream_t st);
int rn_tr_gn(const RnTrain& tr, const RnPlan& p, const cgen_resnet_args* a, int i, const float* g, const float* y, float* ws, hipStream_t st);
int rn_tr_wgrad(const RnTrain& tr, const RnPlan& p, int i, cgen_view seg, const float* gout, float* ws, hipStream_t st);
int rn_tr_tail(const RnTrain& tr, const RnPlan& p, const cgen_resnet_args* a, float* ws, const float* coef, hipStream_t st);
bool rn_tr_wants_dx(const RnTrain& tr);

int rn_forward(const RnPlan& p, const cgen_resnet_args* a, const float* x, float* ws, float* terms, float* outs, hipStream_t st,
               const RnTrain* tr = nullptr) {
  const int n = p.n;
  // stem: patches [n, h1, h1, 49 (+7 zeros)] -> 1x1 conv -> GroupNorm + ReLU -> max pool
  cgen_view xin = rn_view(const_cast<float*>(x), p.res, 1);
  RN_TRY(cgen_im2col_strided(CGEN_F32, n, p.res, p.res, 7, 2, 3, p.h1, p.h1, xin, rn_view(ws + p.col, p.h1, 49, 56), st));
  RN_TRY(rn_conv(p, p.h1, 1, rn_view(ws + p.col, p.h1, 49, 56), a->img_fwd[0], rn_view(ws + p.raw[0], p.h1, 64), nullptr, st));
  RN_TRY(rn_stats(p, 0, ws, st));
  RN_TRY(rn_apply(p, a, 0, nullptr, -1, ws + p.stem_act, ws, st));
  {
    const int64_t total4 = (int64_t)n * p.hp * p.hp * 16;
    hipLaunchKernelGGL(rn_pool_fwd, dim3(rn_grid(total4)), dim3(256), 0, st, ws + p.stem_act, ws + p.pool, p.h1, p.hp, total4);
    RN_TRY(check_launch("cgen_resnet (max pool)"));
  }
  for (int k = 0; k < 8; ++k) {
    const int s = k / 2, c = 64 << s, h = p.hs[s], i1 = rn_conv1(k), i2 = rn_conv2(k);
    int64_t in;
    int cin, hin;
    rn_block_in(p, k, in, cin, hin);
    if (rn_has_ds(k)) {
      RN_TRY(cgen_im2col_strided(CGEN_F32, n, hin, hin, 3, 2, 1, h, h, rn_view(ws + in, hin, cin), rn_view(ws + p.col, h, 9 * cin), st));
      RN_TRY(rn_conv(p, h, 1, rn_view(ws + p.col, h, 9 * cin), a->img_fwd[i1], rn_view(ws + p.raw[i1], h, c), nullptr, st));
    } else {
      RN_TRY(rn_conv(p, h, 3, rn_view(ws + in, h, cin), a->img_fwd[i1], rn_view(ws + p.raw[i1], h, c), nullptr, st));
    }
    RN_TRY(rn_stats(p, i1, ws, st));
    RN_TRY(rn_apply(p, a, i1, nullptr, -1, ws + p.a1[k], ws, st));
    if (tr) RN_TRY(rn_tr_dropout(*tr, p, k, ws, st));
    RN_TRY(rn_conv(p, h, 3, rn_view(ws + p.a1[k], h, c), a->img_fwd[i2], rn_view(ws + p.raw[i2], h, c), nullptr, st));
    RN_TRY(rn_stats(p, i2, ws, st));
    if (rn_has_ds(k)) {
      const int id = rn_ds(s);
      cgen_view even = rn_view(ws + in, hin, cin);  // the even pixels of the block's input: a 1x1 stride-2 conv reads only them
      even.sh *= 2; even.sw *= 2;
      RN_TRY(rn_conv(p, h, 1, even, a->img_fwd[id], rn_view(ws + p.raw[id], h, c), nullptr, st));
      RN_TRY(rn_stats(p, id, ws, st));
      RN_TRY(rn_apply(p, a, i2, nullptr, id, ws + p.y[k], ws, st));
    } else {
      RN_TRY(rn_apply(p, a, i2, ws + in, -1, ws + p.y[k], ws, st));
    }
  }
  RnTail t;
  rn_tail_args(t, p, a, ws);
  t.terms = terms; t.outs = outs;
  hipLaunchKernelGGL(rn_tail_fwd, dim3(n), dim3(256), 0, st, t);
  return check_launch("cgen_resnet (tail)");
}

int rn_backward(const RnPlan& p, const cgen_resnet_args* a, float* ws, const float* coef, float* dx, hipStream_t st,
                const RnTrain* tr = nullptr, const float* x = nullptr) {
  const int n = p.n;
  float* G0 = ws + p.g[0];  // gradient w.r.t. the current block's output
  float* G1 = ws + p.g[1];
  float* G2 = ws + p.g[2];
  RnTail t;
  rn_tail_args(t, p, a, ws);
  t.coef = coef; t.g = G0;
  hipLaunchKernelGGL(rn_tail_bwd, dim3(n), dim3(256), 0, st, t);
  RN_TRY(check_launch("cgen_resnet (tail backward)"));
  if (tr) RN_TRY(rn_tr_tail(*tr, p, a, ws, coef, st));
  for (int k = 7; k >= 0; --k) {
    const int s = k / 2, c = 64 << s, h = p.hs[s], i1 = rn_conv1(k), i2 = rn_conv2(k);
    int64_t in;
    int cin, hin;
    rn_block_in(p, k, in, cin, hin);
    // bn2: G0 -> d raw2 in G1; G0 becomes the masked gradient, which is also the identity branch's
    RN_TRY(rn_gn_bwd(p, a, i2, G0, ws + p.y[k], G1, G0, ws, st));
    if (tr) {  // (every weight gradient reads d raw in G1 before the next rn_gn_bwd overwrites it: one stream, in order)
      RN_TRY(rn_tr_gn(*tr, p, a, i2, G0, ws + p.y[k], ws, st));
      RN_TRY(rn_tr_wgrad(*tr, p, i2, rn_view(ws + p.a1[k], h, c), G1, ws, st));
    }
    RN_TRY(rn_conv(p, h, 3, rn_view(G1, h, c), a->img_dg[i2], rn_view(G2, h, c), nullptr, st));  // -> gradient w.r.t. a1
    if (tr) RN_TRY(rn_tr_unscale(*tr, p, k, G2, st));                                             // (Dropout's 1 / (1 - p))
    RN_TRY(rn_gn_bwd(p, a, i1, G2, ws + p.a1[k], G1, nullptr, ws, st));                           // -> d raw1
    if (tr) RN_TRY(rn_tr_gn(*tr, p, a, i1, G2, ws + p.a1[k], ws, st));
    if (rn_has_ds(k)) {
      const int id = rn_ds(s);
      if (tr) {  // the patches again (the forward's are long overwritten), into col before the data gradient below takes it
        RN_TRY(cgen_im2col_strided(CGEN_F32, n, hin, hin, 3, 2, 1, h, h, rn_view(ws + in, hin, cin), rn_view(ws + p.col, h, 9 * cin), st));
        RN_TRY(rn_tr_wgrad(*tr, p, i1, rn_view(ws + p.col, h, 9 * cin), G1, ws, st));
      }
      RN_TRY(rn_conv(p, h, 1, rn_view(G1, h, c), a->img_dg[i1], rn_view(ws + p.col, h, 9 * cin), nullptr, st));
      RN_TRY(cgen_col2im_strided(CGEN_F32, n, hin, hin, 3, 2, 1, h, h, rn_view(ws + p.col, h, 9 * cin), rn_view(G2, hin, cin), 0, st));
      RN_TRY(rn_gn_bwd(p, a, id, G0, ws + p.y[k], G1, nullptr, ws, st));  // (G0 is masked already: masking again changes nothing)
      if (tr) {
        cgen_view even = rn_view(ws + in, hin, cin);  // as the forward reads it
        even.sh *= 2; even.sw *= 2;
        RN_TRY(rn_tr_gn(*tr, p, a, id, G0, ws + p.y[k], ws, st));
        RN_TRY(rn_tr_wgrad(*tr, p, id, even, G1, ws, st));
      }
      RN_TRY(rn_conv(p, h, 1, rn_view(G1, h, c), a->img_dg[id], rn_view(ws + p.col, h, cin), nullptr, st));
      RN_TRY(cgen_col2im_strided(CGEN_F32, n, hin, hin, 1, 2, 0, h, h, rn_view(ws + p.col, h, cin), rn_view(G2, hin, cin), 1, st));
    } else {
      if (tr) RN_TRY(rn_tr_wgrad(*tr, p, i1, rn_view(ws + in, h, cin), G1, ws, st));
      const cgen_view idn = rn_view(G0, h, c);
      RN_TRY(rn_conv(p, h, 3, rn_view(G1, h, c), a->img_dg[i1], rn_view(G2, h, cin), &idn, st));
    }
    std::swap(G0, G2);
  }
  // G0: gradient w.r.t. the pooled map -> the stem's activation -> its raw conv output -> the patches -> x
  {
    const int64_t total4 = (int64_t)n * p.h1 * p.h1 * 16;
    hipLaunchKernelGGL(rn_pool_bwd, dim3(rn_grid(total4)), dim3(256), 0, st, ws + p.stem_act, G0, G1, p.h1, p.hp, total4);
    RN_TRY(check_launch("cgen_resnet (max pool backward)"));
  }
  RN_TRY(rn_gn_bwd(p, a, 0, G1, ws + p.stem_act, G2, nullptr, ws, st));
  if (tr) {
    RN_TRY(rn_tr_gn(*tr, p, a, 0, G1, ws + p.stem_act, ws, st));
    RN_TRY(cgen_im2col_strided(CGEN_F32, n, p.res, p.res, 7, 2, 3, p.h1, p.h1, rn_view(const_cast<float*>(x), p.res, 1),
                               rn_view(ws + p.col, p.h1, 49, 56), st));
    RN_TRY(rn_tr_wgrad(*tr, p, 0, rn_view(ws + p.col, p.h1, 49, 56), G2, ws, st));
    if (!rn_tr_wants_dx(*tr)) return CGEN_OK;
  }
  RN_TRY(rn_conv(p, p.h1, 1, rn_view(G2, p.h1, 64), a->img_dg[0], rn_view(ws + p.col, p.h1, 49, 56), nullptr, st));
  cgen_view gcol = rn_view(ws + p.col, p.h1, 49, 56);
  gcol.cpad = 0;
  return cgen_col2im_strided(CGEN_F32, n, p.res, p.res, 7, 2, 3, p.h1, p.h1, gcol, rn_view(dx, p.res, 1), 0, st);
}

}  // namespace
}  // namespace cgen

using namespace cgen;

extern "C" int cgen_resnet_workspace(int32_t n, int32_t res, int64_t* floats) {
  CGEN_REQUIRE(floats, "cgen_resnet_workspace: null floats");
  CGEN_REQUIRE(n >= 1, "cgen_resnet_workspace: n = %d, need n >= 1", n);
  CGEN_REQUIRE(res >= 32 && res <= 256, "cgen_resnet_workspace: res = %d outside 32..256", res);
  RnPlan p;
  rn_plan(p, n, res);
  *floats = p.total;
  return CGEN_OK;
}

extern "C" int cgen_resnet_site(int32_t n, int32_t res, int32_t site, int64_t* offset, int32_t* h, int32_t* c) {
  CGEN_REQUIRE(offset && h && c, "cgen_resnet_site: null offset, h or c");
  CGEN_REQUIRE(n >= 1, "cgen_resnet_site: n = %d, need n >= 1", n);
  CGEN_REQUIRE(res >= 32 && res <= 256, "cgen_resnet_site: res = %d outside 32..256", res);
  CGEN_REQUIRE(site >= 0 && site < CGEN_RESNET_SITES, "cgen_resnet_site: site = %d outside 0..%d", site, CGEN_RESNET_SITES - 1);
  RnPlan p;
  rn_plan(p, n, res);
  if (site == 0) { *offset = p.stem_act; *h = p.h1; *c = 64; }
  else if (site == CGEN_RESNET_SITES - 1) { *offset = p.pool; *h = p.hp; *c = 64; }
  else {
    const int k = (site - 1) / 2, s = k / 2;
    *offset = (site - 1) % 2 == 0 ? p.a1[k] : p.y[k];
    *h = p.hs[s]; *c = 64 << s;
  }
  return CGEN_OK;
}

extern "C" int cgen_resnet_fwd(const cgen_resnet_args* a, int32_t n, const float* x, float* ws, int64_t ws_floats, float* terms,
                               float* outs, float* loss, cgen_stream_t stream) {
  RnPlan p;
  int rc = rn_validate("cgen_resnet_fwd", a, n, x, "x", ws, ws_floats, terms != nullptr, p);
  if (rc) return rc;
  CGEN_REQUIRE(terms || outs, "cgen_resnet_fwd: nothing to write (terms and outs are null)");
  CGEN_REQUIRE(!loss || terms, "cgen_resnet_fwd: loss needs terms");
  rc = rn_forward(p, a, x, ws, terms, outs, (hipStream_t)stream);
  if (rc || !loss) return rc;
  hipLaunchKernelGGL(pred_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, (int64_t)n * 4, loss);
  return check_launch("cgen_resnet_fwd (sum)");
}

extern "C" int cgen_resnet_bwd(const cgen_resnet_args* a, int32_t n, float* ws, int64_t ws_floats, const float* coef_dev, float* dx,
                               cgen_stream_t stream) {
  RnPlan p;
  const int rc = rn_validate("cgen_resnet_bwd", a, n, dx, "dx", ws, ws_floats, true, p);
  if (rc) return rc;
  CGEN_REQUIRE(coef_dev, "cgen_resnet_bwd: null coef_dev");
  return rn_backward(p, a, ws, coef_dev, dx, (hipStream_t)stream);
}
