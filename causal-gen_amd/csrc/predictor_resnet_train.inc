// ============================================================================ ChestPGM's anticausal heads, TRAINING (after predictor_resnet.inc)
// cgen_resnet_train_*: the eval plans of predictor_resnet.inc with their training arms switched on (rn_forward / rn_backward take an
// RnTrain).  The GEMM-shaped work is again the library's: cgen_conv2d_wgrad (CGEN_F32: the generic f32-MFMA kernel, split-K partials
// [split][Co][tap][Ci]) and cgen_wgrad_reduce, one pair per conv site, into the OIHW gradient.  What is new here:
//   rn_drop_kernel                 CustomBlock's Dropout on a1[k], in place, or its decisions as bytes; one Philox group per channel quad
//   rn_scale                       g *= 1 / (1 - p) at the a1 sites on the way back (the y > 0 test covers the dropped elements)
//   rn_gnp_part / rn_gnp_final     d gamma, d beta: per-(image, chunk, channel) partials, then one fixed tree per channel quad
//   rn_tail_dout / rn_tail_wgrad   coef * d term / d out per image, and the four Linears' gradients summed over the images in order
//   rn_nan_guard                   a non-finite GroupNorm statistic makes the image's terms NaN (the step's skip predicate reads them)
//   rn_wred_setup                  the reduce's descriptor and chunk tables, written into the workspace by vector stores
// Same conventions as above: a lane owns a channel quad, every sum has a fixed order, no atomics.
namespace cgen {
namespace {

constexpr uint32_t RN_STREAM_DROPOUT = 981u;  // + block k (common.h keeps the list)
constexpr int RN_WRED_CHUNK = 1024;           // elements per workgroup of cgen_wgrad_reduce

struct RnTrain {
  const cgen_resnet_train_args* ta;
  float p, scale;  // scale = 1 / (1 - p)
  bool want_dx;
  // float offsets into the workspace, after the eval plan's
  int64_t wpart, gnpart, dout, descs, csite, cidx, total;
  int maxch;       // chunks of the largest reduce
  int nsplit[RN_CONVS];
};

// the weight-gradient problem of conv site i: map size, kernel size as the library sees it, input channels as it sees them
inline void rn_site_wg(const RnPlan& p, int i, int& h, int& ks, int& ci) {
  h = p.conv_h[i];
  const int c = p.conv_c[i];
  if (i == 0) { ks = 1; ci = 49; return; }
  if (i >= 17) { ks = 1; ci = c / 2; return; }
  const int k = (i - 1) / 2;
  if (i == rn_conv1(k) && rn_has_ds(k)) { ks = 1; ci = 9 * (c / 2); return; }
  ks = 3; ci = c;
}

inline void rn_wg_args(cgen_wgrad_args& w, int n, int h, int ks, cgen_view seg, int co, float* gout) {
  memset(&w, 0, sizeof(w));
  w.dtype = CGEN_F32; w.n = n; w.h = h; w.w = h; w.ks = ks; w.nseg = 1; w.act = CGEN_ACT_NONE;
  w.seg[0] = seg;
  w.gout = rn_view(gout, h, co);
}

void rn_train_plan(RnTrain& t, const RnPlan& p) {
  int64_t o = p.total;
  auto take = [&](int64_t floats) { const int64_t at = o; o += (floats + 3) / 4 * 4; return at; };
  const int64_t N = p.n;
  int64_t wpart = 0, gnpart = 0, maxw = 0;
  for (int i = 0; i < RN_CONVS; ++i) {
    int h, ks, ci;
    rn_site_wg(p, i, h, ks, ci);
    cgen_wgrad_args w;
    rn_wg_args(w, p.n, h, ks, rn_view(nullptr, h, ci), p.conv_c[i], nullptr);
    t.nsplit[i] = cgen_conv2d_wgrad_plan(&w, nullptr);
    const int64_t nw = (int64_t)p.conv_c[i] * ci * ks * ks;
    wpart = std::max(wpart, nw * t.nsplit[i]);
    maxw = std::max(maxw, nw);
    const int64_t chunks = (h * h + RN_CHUNK - 1) / RN_CHUNK;
    gnpart = std::max(gnpart, N * chunks * p.conv_c[i] * 2);
  }
  t.maxch = (int)((maxw + RN_WRED_CHUNK - 1) / RN_WRED_CHUNK);
  t.wpart = take(wpart);
  t.gnpart = take(gnpart);
  t.dout = take(N * RN_TAIL_OUT);
  t.descs = take((int64_t)RN_CONVS * sizeof(cgen_wred_desc) / 4);
  t.csite = take(t.maxch);
  t.cidx = take(t.maxch);
  t.total = o;
}

// ---------------------------------------------------------------------------- Dropout
// The four decisions of channel quad `quad` (counted inside the image's NHWC map) of image `img` in block k.
__device__ __forceinline__ void rn_keep4(uint64_t seed, uint64_t off, int k, int img, uint32_t quad, float p, bool (&keep)[4]) {
  uint32_t r[4];
  Philox::gen(seed, off, RN_STREAM_DROPOUT + (uint32_t)k, ((uint64_t)(uint32_t)img << 32) | quad, r);
#pragma unroll
  for (int e = 0; e < 4; ++e) keep[e] = Philox::u01(r[e]) >= p;
}

// a = keep ? a * scale : 0 in place (BYTES: keep itself, one byte per element, nothing else touched)
template <bool BYTES>
__global__ __launch_bounds__(256) void rn_drop_kernel(float* a, uint8_t* out, const uint64_t* rng, int k, float p, float scale,
                                                      int64_t per4, int64_t total4) {
  const uint64_t seed = rng[0], off = rng[1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int img = (int)(i / per4);
    const uint32_t quad = (uint32_t)(i - (int64_t)img * per4);
    bool keep[4];
    rn_keep4(seed, off, k, img, quad, p, keep);
    if (BYTES) {
      uchar4 b;
      b.x = keep[0]; b.y = keep[1]; b.z = keep[2]; b.w = keep[3];
      ((uchar4*)out)[i] = b;
    } else {
      float4 v = ((const float4*)a)[i];
      v.x = keep[0] ? v.x * scale : 0.f; v.y = keep[1] ? v.y * scale : 0.f;
      v.z = keep[2] ? v.z * scale : 0.f; v.w = keep[3] ? v.w * scale : 0.f;
      ((float4*)a)[i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void rn_scale(float* g, float scale, int64_t total4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    float4 v = ((const float4*)g)[i];
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    ((float4*)g)[i] = v;
  }
}

// ---------------------------------------------------------------------------- GroupNorm parameter gradients
// part[((img * nchunks + chunk) * Q + quad) * 8 + (0..3 | 4..7)] = sum over the chunk's pixels of g_masked | g_masked * xhat of the
// quad's four channels: per thread over its pixels, then over the pixel slots in slot order by the quad's first thread.
__global__ __launch_bounds__(256) void rn_gnp_part(RnRed a) {
  __shared__ float red[8][256];
  const int tid = threadIdx.x, ch = blockIdx.x, img = blockIdx.y;
  const int Q = a.c >> 2, PP = 256 / Q, q = tid & (Q - 1), pl = tid / Q;
  const int qpg = a.cpg >> 2, G = a.c / a.cpg, grp = q / qpg;
  const int p0 = ch * RN_CHUNK, p1 = min(a.hw, p0 + RN_CHUNK);
  const int64_t base = (int64_t)img * a.hw * Q + q;
  const float4 *x = (const float4*)a.x + base, *g = (const float4*)a.g + base, *y = (const float4*)a.y + base;
  const float mean = a.stat[((int64_t)img * G + grp) * 2], rstd = a.stat[((int64_t)img * G + grp) * 2 + 1];
  float4 sb = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f};
  for (int p = p0 + pl; p < p1; p += PP) {
    const float4 v = x[(int64_t)p * Q], gv = g[(int64_t)p * Q], yv = y[(int64_t)p * Q];
    const float m0 = yv.x > 0.f ? gv.x : 0.f, m1 = yv.y > 0.f ? gv.y : 0.f, m2 = yv.z > 0.f ? gv.z : 0.f, m3 = yv.w > 0.f ? gv.w : 0.f;
    sb.x += m0; sb.y += m1; sb.z += m2; sb.w += m3;
    sg.x += m0 * ((v.x - mean) * rstd); sg.y += m1 * ((v.y - mean) * rstd);
    sg.z += m2 * ((v.z - mean) * rstd); sg.w += m3 * ((v.w - mean) * rstd);
  }
  red[0][tid] = sb.x; red[1][tid] = sb.y; red[2][tid] = sb.z; red[3][tid] = sb.w;
  red[4][tid] = sg.x; red[5][tid] = sg.y; red[6][tid] = sg.z; red[7][tid] = sg.w;
  __syncthreads();
  if (tid < Q) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = 0.f;
    for (int s = 0; s < PP; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] += red[e][s * Q + tid];
    float4* dst = (float4*)(a.part + (((int64_t)img * a.nchunks + ch) * Q + tid) * 8);
    dst[0] = make_float4(t[0], t[1], t[2], t[3]);
    dst[1] = make_float4(t[4], t[5], t[6], t[7]);
  }
}

// One workgroup per channel quad: thread t adds partials t, t + 256, ... of the (image, chunk) list in that order, then a fixed tree.
__global__ __launch_bounds__(256) void rn_gnp_final(const float* part, float* ggamma, float* gbeta, int Q, int count) {
  __shared__ float red[8][256];
  const int tid = threadIdx.x, q = blockIdx.x;
  float t[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) t[e] = 0.f;
  for (int i = tid; i < count; i += 256) {
    const float4* s = (const float4*)(part + ((int64_t)i * Q + q) * 8);
    const float4 b = s[0], g = s[1];
    t[0] += b.x; t[1] += b.y; t[2] += b.z; t[3] += b.w;
    t[4] += g.x; t[5] += g.y; t[6] += g.z; t[7] += g.w;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[e][tid] = t[e];
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[e][tid] += red[e][tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    ((float4*)gbeta)[q] = make_float4(red[0][0], red[1][0], red[2][0], red[3][0]);
    ((float4*)ggamma)[q] = make_float4(red[4][0], red[5][0], red[6][0], red[7][0]);
  }
}

// ---------------------------------------------------------------------------- the four Linears
// dout[b][RN_OFF[h] + j] = coef * d term_h[b] / d out_h[b][j]  (what rn_tail_bwd forms, without the spatial mean's 1 / hw)
__global__ __launch_bounds__(256) void rn_tail_dout(RnTail a, float* dout) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n * 4) return;
  const int b = i >> 2, h = i & 3;
  const cgen_pred_head hd = rn_head(a, h);
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  pred_nll(hd, a.tail_out + (int64_t)b * RN_TAIL_OUT + RN_OFF[h], a.obs[h] + (int64_t)b * a.obs_stride[h], d);
  const float k = a.coef[0];
  for (int j = 0; j < RN_NOUT[h]; ++j) dout[(int64_t)b * RN_TAIL_OUT + RN_OFF[h] + j] = d[j] * k;
  if (h == 0) dout[(int64_t)b * RN_TAIL_OUT + 7] = 0.f;
}

struct RnHeadGrads {
  float* gw[4];
  float* gb[4];
};

// One thread per input column c (512 is the age head's `finding`): the pooled feature of each image recomputed as rn_tail_fwd
// computes it, d fc_w[h][j][c] = sum_b dout[b][h, j] * feat[b][c] over the images in order.  The first seven threads: d fc_b.
__global__ __launch_bounds__(64) void rn_tail_wgrad(RnTail a, RnHeadGrads hg, const float* dout) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c <= RN_FEAT) {
    float acc[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[j] = 0.f;
    for (int b = 0; b < a.n; ++b) {
      float f;
      if (c < RN_FEAT) {
        const float* y = a.y + (int64_t)b * a.hw * RN_FEAT + c;
        float s = 0.f;
        for (int p = 0; p < a.hw; ++p) s += y[(int64_t)p * RN_FEAT];
        f = s / (float)a.hw;
      } else {
        f = a.ctx[(int64_t)b * a.ctx_stride];
      }
#pragma unroll
      for (int j = 0; j < 7; ++j) acc[j] = fmaf(dout[(int64_t)b * RN_TAIL_OUT + j], f, acc[j]);
    }
    for (int h = 0; h < 4; ++h) {
      const int nin = h == 3 ? RN_FEAT + 1 : RN_FEAT;
      if (c < nin)
        for (int j = 0; j < RN_NOUT[h]; ++j) hg.gw[h][(int64_t)j * nin + c] = acc[RN_OFF[h] + j];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 7) {
    const int o = threadIdx.x;
    float s = 0.f;
    for (int b = 0; b < a.n; ++b) s += dout[(int64_t)b * RN_TAIL_OUT + o];
    int h = 3;
    while (RN_OFF[h] > o) --h;
    hg.gb[h][o - RN_OFF[h]] = s;
  }
}

// ---------------------------------------------------------------------------- non-finite inputs
// The ReLU of rn_gn_apply maps NaN to 0 where torch's keeps it, so an image with a NaN or an Inf in it would train as a zero
// activation with a finite loss.  Such an image (or such a weight) leaves a non-finite GroupNorm statistic: one workgroup per
// image looks at its 20 x (mean, rstd) lists and turns the image's four terms into NaN, which the step's skip predicate sees.
struct RnGuard {
  int64_t stat[RN_CONVS];
  int groups[RN_CONVS];
};

__global__ __launch_bounds__(256) void rn_nan_guard(RnGuard g, const float* ws, float* terms) {
  const int b = blockIdx.x;
  int bad = 0;
  for (int i = 0; i < RN_CONVS; ++i) {
    const float* s = ws + g.stat[i] + (int64_t)b * g.groups[i] * 2;
    for (int j = threadIdx.x; j < g.groups[i] * 2; j += 256) bad |= !(fabsf(s[j]) <= FLT_MAX);
  }
  if (__syncthreads_or(bad) && threadIdx.x < 4) terms[(int64_t)b * 4 + threadIdx.x] = __int_as_float(0x7fc00000);
}

// ---------------------------------------------------------------------------- the reduce's tables
struct RnWredSetup {
  cgen_wred_desc d[RN_CONVS];
  int maxch;
};

// descs[20], csite[maxch] = 0 (every reduce is launched on ONE site: descs + i), cidx[maxch] = 0, 1, 2, ...
__global__ __launch_bounds__(256) void rn_wred_setup(RnWredSetup s, cgen_wred_desc* descs, int* csite, int* cidx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < RN_CONVS) descs[i] = s.d[i];
  if (i < s.maxch) { csite[i] = 0; cidx[i] = i; }
}

// ---------------------------------------------------------------------------- host side: the arms rn_forward / rn_backward call
int rn_tr_dropout(const RnTrain& tr, const RnPlan& p, int k, float* ws, hipStream_t st) {
  if (tr.p <= 0.f) return CGEN_OK;  // (p = 0: the eval forward, launch for launch)
  const int s = k / 2;
  const int64_t per4 = (int64_t)p.hs[s] * p.hs[s] * (16 << s), total4 = per4 * p.n;
  hipLaunchKernelGGL(rn_drop_kernel<false>, dim3(rn_grid(total4)), dim3(256), 0, st, ws + p.a1[k], (uint8_t*)nullptr, tr.ta->rng, k, tr.p,
                     tr.scale, per4, total4);
  return check_launch("cgen_resnet_train_fwd (dropout)");
}

int rn_tr_unscale(const RnTrain& tr, const RnPlan& p, int k, float* g, hipStream_t st) {
  if (tr.p <= 0.f) return CGEN_OK;
  const int s = k / 2;
  const int64_t total4 = (int64_t)p.n * p.hs[s] * p.hs[s] * (16 << s);
  hipLaunchKernelGGL(rn_scale, dim3(rn_grid(total4)), dim3(256), 0, st, g, tr.scale, total4);
  return check_launch("cgen_resnet_train_bwd (dropout scale)");
}

int rn_tr_gn(const RnTrain& tr, const RnPlan& p, const cgen_resnet_args* a, int i, const float* g, const float* y, float* ws, hipStream_t st) {
  const int hw = p.conv_h[i] * p.conv_h[i], c = p.conv_c[i], G = p.groups[i], nchunks = (hw + RN_CHUNK - 1) / RN_CHUNK;
  RnRed r;
  memset(&r, 0, sizeof(r));
  r.x = ws + p.raw[i]; r.g = g; r.y = y; r.stat = ws + p.stat[i]; r.gamma = a->gamma[i]; r.part = ws + tr.gnpart;
  r.hw = hw; r.c = c; r.cpg = c / G; r.nchunks = nchunks;
  hipLaunchKernelGGL(rn_gnp_part, dim3(nchunks, p.n), dim3(256), 0, st, r);
  hipLaunchKernelGGL(rn_gnp_final, dim3(c / 4), dim3(256), 0, st, ws + tr.gnpart, tr.ta->ggamma[i], tr.ta->gbeta[i], c / 4, p.n * nchunks);
  return check_launch("cgen_resnet_train_bwd (GroupNorm parameter gradients)");
}

int rn_tr_wgrad(const RnTrain& tr, const RnPlan& p, int i, cgen_view seg, const float* gout, float* ws, hipStream_t st) {
  int h, ks, ci;
  rn_site_wg(p, i, h, ks, ci);
  cgen_wgrad_args w;
  rn_wg_args(w, p.n, h, ks, seg, p.conv_c[i], const_cast<float*>(gout));
  w.nsplit = tr.nsplit[i];
  w.partial_w = ws + tr.wpart;
  RN_TRY(cgen_conv2d_wgrad(&w, st));
  const int64_t nw = (int64_t)p.conv_c[i] * ci * ks * ks;
  return cgen_wgrad_reduce((const cgen_wred_desc*)(ws + tr.descs) + i, (const int32_t*)(ws + tr.csite), (const int32_t*)(ws + tr.cidx),
                           (int)((nw + RN_WRED_CHUNK - 1) / RN_WRED_CHUNK), st);
}

// the reduce's tables, d out and the Linears' gradients: the head of the training backward
int rn_tr_tail(const RnTrain& tr, const RnPlan& p, const cgen_resnet_args* a, float* ws, const float* coef, hipStream_t st) {
  RnWredSetup s;
  memset(&s, 0, sizeof(s));
  for (int i = 0; i < RN_CONVS; ++i) {
    int h, ks, ci;
    rn_site_wg(p, i, h, ks, ci);
    cgen_wred_desc& d = s.d[i];
    d.partial_w = ws + tr.wpart; d.grad_w = tr.ta->gw[i];
    d.co = p.conv_c[i]; d.ci_total = ci; d.ks = ks; d.nsplit = tr.nsplit[i];
    d.numel = (int64_t)d.co * ci * ks * ks;  // (no bias: the elements past the weight's are the bias gradient's)
  }
  s.maxch = tr.maxch;
  const int items = std::max(tr.maxch, RN_CONVS);
  hipLaunchKernelGGL(rn_wred_setup, dim3((items + 255) / 256), dim3(256), 0, st, s, (cgen_wred_desc*)(ws + tr.descs), (int*)(ws + tr.csite),
                     (int*)(ws + tr.cidx));
  RnTail t;
  rn_tail_args(t, p, a, ws);
  t.coef = coef;
  hipLaunchKernelGGL(rn_tail_dout, dim3((p.n * 4 + 255) / 256), dim3(256), 0, st, t, ws + tr.dout);
  RnHeadGrads hg;
  for (int h = 0; h < 4; ++h) { hg.gw[h] = tr.ta->gfc_w[h]; hg.gb[h] = tr.ta->gfc_b[h]; }
  hipLaunchKernelGGL(rn_tail_wgrad, dim3((RN_FEAT + 1 + 63) / 64), dim3(64), 0, st, t, hg, ws + tr.dout);
  return check_launch("cgen_resnet_train_bwd (heads)");
}

bool rn_tr_wants_dx(const RnTrain& tr) { return tr.want_dx; }

int rn_train_validate(const char* who, const cgen_resnet_train_args* a, int n, const float* x, const float* ws, int64_t ws_floats,
                      bool grads, RnPlan& p, RnTrain& t) {
  CGEN_REQUIRE(a, "%s: null args", who);
  CGEN_REQUIRE(a->p_dropout >= 0.f && a->p_dropout < 1.f, "%s: p_dropout = %g outside [0, 1)", who, (double)a->p_dropout);
  CGEN_REQUIRE(a->rng, "%s: null rng (the device Philox state {seed, offset})", who);
  RN_TRY(rn_validate(who, &a->net, n, x, "x", ws, ws_floats, true, p));
  rn_train_plan(t, p);
  CGEN_REQUIRE(ws_floats >= t.total, "%s: ws_floats = %lld, too small: need %lld (cgen_resnet_train_workspace)", who, (long long)ws_floats,
               (long long)t.total);
  if (grads) {
    for (int i = 0; i < RN_CONVS; ++i) {
      CGEN_REQUIRE(a->gw[i] && ((uintptr_t)a->gw[i] % 16) == 0, "%s: gw %d (the conv's OIHW gradient) null or not 16-byte aligned", who, i);
      CGEN_REQUIRE(a->ggamma[i] && a->gbeta[i] && ((uintptr_t)a->ggamma[i] % 16) == 0 && ((uintptr_t)a->gbeta[i] % 16) == 0,
                   "%s: ggamma / gbeta %d null or not 16-byte aligned", who, i);
    }
    for (int h = 0; h < 4; ++h)
      CGEN_REQUIRE(a->gfc_w[h] && a->gfc_b[h] && ((uintptr_t)a->gfc_w[h] % 4) == 0 && ((uintptr_t)a->gfc_b[h] % 4) == 0,
                   "%s: gfc_w / gfc_b of head %d null or not 4-byte aligned", who, h);
  }
  t.ta = a; t.p = a->p_dropout; t.scale = 1.f / (1.f - a->p_dropout); t.want_dx = false;
  return CGEN_OK;
}

}  // namespace
}  // namespace cgen

using namespace cgen;

extern "C" int cgen_resnet_train_workspace(int32_t n, int32_t res, int64_t* floats) {
  CGEN_REQUIRE(floats, "cgen_resnet_train_workspace: null floats");
  CGEN_REQUIRE(n >= 1, "cgen_resnet_train_workspace: n = %d, need n >= 1", n);
  CGEN_REQUIRE(res >= 32 && res <= 256, "cgen_resnet_train_workspace: res = %d outside 32..256", res);
  CGEN_REQUIRE((int64_t)n * rn_half(res) * rn_half(res) * 64 < (1ll << 31), "cgen_resnet_train_workspace: n = %d is too many images of res %d", n, res);
  RnPlan p;
  RnTrain t;
  rn_plan(p, n, res);
  rn_train_plan(t, p);
  *floats = t.total;
  return CGEN_OK;
}

extern "C" int cgen_resnet_train_fwd(const cgen_resnet_train_args* a, int32_t n, const float* x, float* ws, int64_t ws_floats, float* terms,
                                     float* outs, float* loss, cgen_stream_t stream) {
  RnPlan p;
  RnTrain t;
  int rc = rn_train_validate("cgen_resnet_train_fwd", a, n, x, ws, ws_floats, false, p, t);
  if (rc) return rc;
  CGEN_REQUIRE(terms, "cgen_resnet_train_fwd: null terms");
  rc = rn_forward(p, &a->net, x, ws, terms, outs, (hipStream_t)stream, &t);
  if (rc) return rc;
  RnGuard g;
  for (int i = 0; i < RN_CONVS; ++i) { g.stat[i] = p.stat[i]; g.groups[i] = p.groups[i]; }
  hipLaunchKernelGGL(rn_nan_guard, dim3(n), dim3(256), 0, (hipStream_t)stream, g, ws, terms);
  if (!loss) return check_launch("cgen_resnet_train_fwd (guard)");
  hipLaunchKernelGGL(pred_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, (int64_t)n * 4, loss);
  return check_launch("cgen_resnet_train_fwd (sum)");
}

extern "C" int cgen_resnet_train_bwd(const cgen_resnet_train_args* a, int32_t n, const float* x, float* ws, int64_t ws_floats,
                                     const float* coef_dev, float* dx, cgen_stream_t stream) {
  RnPlan p;
  RnTrain t;
  const int rc = rn_train_validate("cgen_resnet_train_bwd", a, n, x, ws, ws_floats, true, p, t);
  if (rc) return rc;
  CGEN_REQUIRE(coef_dev, "cgen_resnet_train_bwd: null coef_dev");
  t.want_dx = dx != nullptr;
  return rn_backward(p, &a->net, ws, coef_dev, dx, (hipStream_t)stream, &t, x);
}

extern "C" int cgen_resnet_dropout_keep(const uint64_t* rng, float p_dropout, int32_t n, int32_t res, int32_t block, uint8_t* keep,
                                        cgen_stream_t stream) {
  CGEN_REQUIRE(rng, "cgen_resnet_dropout_keep: null rng");
  CGEN_REQUIRE(keep && ((uintptr_t)keep % 4) == 0, "cgen_resnet_dropout_keep: keep is null or not 4-byte aligned");
  CGEN_REQUIRE(p_dropout >= 0.f && p_dropout < 1.f, "cgen_resnet_dropout_keep: p_dropout = %g outside [0, 1)", (double)p_dropout);
  CGEN_REQUIRE(n >= 1, "cgen_resnet_dropout_keep: n = %d, need n >= 1", n);
  CGEN_REQUIRE(res >= 32 && res <= 256, "cgen_resnet_dropout_keep: res = %d outside 32..256", res);
  CGEN_REQUIRE(block >= 0 && block < 8, "cgen_resnet_dropout_keep: block = %d outside 0..7", block);
  RnPlan p;
  rn_plan(p, n, res);
  const int s = block / 2;
  const int64_t per4 = (int64_t)p.hs[s] * p.hs[s] * (16 << s), total4 = per4 * n;
  hipLaunchKernelGGL(rn_drop_kernel<true>, dim3(rn_grid(total4)), dim3(256), 0, (hipStream_t)stream, (float*)nullptr, keep, rng, block, p_dropout,
                     1.f, per4, total4);
  return check_launch("cgen_resnet_dropout_keep");
}
