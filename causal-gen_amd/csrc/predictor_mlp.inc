// ============================================================================ scalar head, training mode (included at the end of predictor.hip)
// pgm/layers.py MLP (FlowPredictor.encoder_a: age from two scalars) with batch-statistic BatchNorm1d: forward and parameter
// gradients, ONE launch each whatever n (include/cgen_hip.h, cgen_mlp_train_*).  n <= 4096 rows of w <= 64 channels are at most
// 16 M multiply-adds per linear: a single workgroup of 1024 threads owns the whole batch, so that -- the discipline of
// predictor_train.inc -- every reduction over the batch runs inside one workgroup in a fixed order.  No atomics, bit-identical reruns.
//
// Ownership: the threads form G = min(1024 / w, n) row groups of w channels, thread (g, j) = g * w + j owns element j of rows
// b = g, g + G, ...  It alone writes and re-reads its elements of the workspace planes (no cross-thread traffic through global
// memory); a linear layer walks the batch in tiles of G rows whose activations go through LDS; a sum over the batch is per-thread
// over the own rows, then over the G groups in g order by the channel's first thread (col_sum).
namespace cgen {
namespace {

constexpr int MT = 1024;  // threads of the one workgroup

struct MlpArgs {
  cgen_pred_head hd;  // kind NORMAL, tanh_loc, std_fixed, obs, obs_stride: what pred_nll reads
  int32_t n, nin, w, G;
  const float* in[CGEN_MLP_MAX_IN];  // (entries past nin repeat entry 0: read, then multiplied by a zero weight)
  int64_t in_stride[CGEN_MLP_MAX_IN];
  const float *w0, *w3, *w6, *b6;
  const float *gamma[2], *beta[2];
  float *rmean[2], *rvar[2];
  int64_t* nbt[2];
  float *gw0, *gw3, *gw6, *gb6, *ggamma[2], *gbeta[2];
  float *xh1, *xh2;  // [n][w]: raw pre-activations during the forward's statistics, then (z - mean) / std
  float* dh;         // [n][w]: the backward's gradient plane
  float* out;        // [n][2]
  float* invstd;     // [2][w]
  float momentum;
  float* terms;
  float* loss;
  const float* coef;
};

// Sum of `v` over the G row groups, per channel: partials through LDS, added in g order by the channel's first thread; every
// thread gets its channel's sum.  Called by all threads of the workgroup.
__device__ __forceinline__ float col_sum(float v, float* part, float* res, int w, int G, int g, int j, bool active) {
  if (active) part[g * w + j] = v;
  __syncthreads();
  if (active && g == 0) {
    float s = 0.f;
    for (int q = 0; q < G; ++q) s += part[q * w + j];
    res[j] = s;
  }
  __syncthreads();
  return res[j];
}

// BatchNorm L's batch statistics of channel j.  The thread's own elements of `z` hold the raw values and `s` is their sum: the
// mean, then the biased variance about it in a second pass over the own elements; running statistics as nn.BatchNorm1d.
__device__ __forceinline__ void mlp_bn_stats(const MlpArgs& a, int L, const float* z, float s, float* part, float* res, int g, int j,
                                             bool active, float& mean, float& invstd) {
  const int n = a.n, w = a.w, G = a.G;
  mean = col_sum(s, part, res, w, G, g, j, active) / (float)n;
  s = 0.f;
  if (active)
    for (int b = g; b < n; b += G) {
      const float d = z[b * w + j] - mean;
      s = fmaf(d, d, s);
    }
  const float var = col_sum(s, part, res, w, G, g, j, active) / (float)n;
  invstd = 1.f / sqrtf(var + BN_EPS);
  if (active && g == 0) {
    a.invstd[L * w + j] = invstd;
    const float mo = a.momentum;
    a.rmean[L][j] = (1.f - mo) * a.rmean[L][j] + mo * mean;
    a.rvar[L][j] = (1.f - mo) * a.rvar[L][j] + mo * (var * ((float)n / (float)(n - 1)));
    if (j == 0) a.nbt[L][0] += 1;
  }
}

__global__ __launch_bounds__(MT) void pmlp_fwd(MlpArgs a) {
  __shared__ float wt[CGEN_MLP_MAX_WIDTH * CGEN_MLP_MAX_WIDTH];  // mlp.3's weight transposed: wt[i * w + j] = W[j][i]
  __shared__ float a_s[MT];                                      // a tile's activations, [g][channel]
  __shared__ float part[MT];
  __shared__ float res[CGEN_MLP_MAX_WIDTH];
  __shared__ float o_s[2 * (MT / 8)];  // a tile's outputs, [g][2]
  const int tid = threadIdx.x, n = a.n, w = a.w, G = a.G, tiles = (n + G - 1) / G;
  const bool active = tid < G * w;
  const int g = active ? tid / w : 0, j = active ? tid - g * w : 0;

  // mlp.0 on the own rows
  float wk[CGEN_MLP_MAX_IN];
#pragma unroll
  for (int k = 0; k < CGEN_MLP_MAX_IN; ++k) wk[k] = k < a.nin ? a.w0[j * a.nin + k] : 0.f;
  float s = 0.f;
  if (active)
    for (int b = g; b < n; b += G) {
      float z = 0.f;
#pragma unroll
      for (int k = 0; k < CGEN_MLP_MAX_IN; ++k) z = fmaf(wk[k], a.in[k][b * a.in_stride[k]], z);
      a.xh1[b * w + j] = z;
      s += z;
    }
  float mean, invstd;
  mlp_bn_stats(a, 0, a.xh1, s, part, res, g, j, active, mean, invstd);

  // mlp.1 + LeakyReLU into LDS a tile at a time, mlp.3 from there
  for (int e = tid; e < w * w; e += MT) {
    const int jj = e / w, ii = e - jj * w;
    wt[ii * w + jj] = a.w3[e];
  }
  float sc = a.gamma[0][j], sh = a.beta[0][j];
  s = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int b = t * G + g;
    const bool on = active && b < n;
    if (on) {
      const float xh = (a.xh1[b * w + j] - mean) * invstd;
      a.xh1[b * w + j] = xh;
      a_s[tid] = lrelu(fmaf(xh, sc, sh));
    }
    __syncthreads();  // (the first one also publishes wt)
    if (on) {
      float acc = 0.f;
      for (int i = 0; i < w; ++i) acc = fmaf(wt[i * w + j], a_s[g * w + i], acc);
      a.xh2[b * w + j] = acc;
      s += acc;
    }
    __syncthreads();
  }
  mlp_bn_stats(a, 1, a.xh2, s, part, res, g, j, active, mean, invstd);

  // mlp.4 + LeakyReLU, mlp.6 and the likelihood: the group's first thread takes the row
  sc = a.gamma[1][j];
  sh = a.beta[1][j];
  s = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int b = t * G + g;
    const bool on = active && b < n;
    if (on) {
      const float xh = (a.xh2[b * w + j] - mean) * invstd;
      a.xh2[b * w + j] = xh;
      a_s[tid] = lrelu(fmaf(xh, sc, sh));
    }
    __syncthreads();
    if (on && j == 0) {
      float o0 = 0.f, o1 = 0.f;
      for (int i = 0; i < w; ++i) {
        const float v = a_s[g * w + i];
        o0 = fmaf(a.w6[i], v, o0);
        o1 = fmaf(a.w6[w + i], v, o1);
      }
      float* o = o_s + 2 * g;
      o[0] = o0 + a.b6[0];
      o[1] = o1 + a.b6[1];
      a.out[2 * b] = o[0];
      a.out[2 * b + 1] = o[1];
      const float term = pred_nll(a.hd, o, a.hd.obs + (int64_t)b * a.hd.obs_stride, nullptr);
      a.terms[b] = term;
      s += term;
    }
    __syncthreads();
  }
  const float total = col_sum(s, part, res, w, G, g, j, active);  // (channel 0 carries the terms)
  if (tid == 0 && a.loss) a.loss[0] += total;
}

__global__ __launch_bounds__(MT) void pmlp_bwd(MlpArgs a) {
  __shared__ float w3s[CGEN_MLP_MAX_WIDTH * CGEN_MLP_MAX_WIDTH];  // mlp.3's weight as it is, [m][i]
  __shared__ float a_s[MT];                                       // a tile's mlp.1 activations, [g][channel]
  __shared__ float d_s[MT];                                       // a tile's d / d(mlp.3 output), [g][channel]
  __shared__ float part[MT];
  __shared__ float res[CGEN_MLP_MAX_WIDTH];
  __shared__ float o_s[2 * (MT / 8)];
  __shared__ float g_s[2 * (MT / 8)];  // a tile's coef * d nll / d out, [g][2]
  const int tid = threadIdx.x, n = a.n, w = a.w, G = a.G, tiles = (n + G - 1) / G;
  const bool active = tid < G * w;
  const int g = active ? tid / w : 0, j = active ? tid - g * w : 0;
  const float cf = a.coef[0];

  // mlp.6 and the likelihood: d / d out, mlp.6's gradients, dh <- d / d(mlp.4 output)
  const float gm2 = a.gamma[1][j], bt2 = a.beta[1][j], w60 = a.w6[j], w61 = a.w6[w + j];
  float sdy = 0.f, sdx = 0.f, q0 = 0.f, q1 = 0.f, sb0 = 0.f, sb1 = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int b = t * G + g;
    const bool on = active && b < n;
    if (on && j == 0) {
      float* o = o_s + 2 * g;
      float* d = g_s + 2 * g;
      o[0] = a.out[2 * b];
      o[1] = a.out[2 * b + 1];
      pred_nll(a.hd, o, a.hd.obs + (int64_t)b * a.hd.obs_stride, d);
      d[0] *= cf;
      d[1] *= cf;
      sb0 += d[0];
      sb1 += d[1];
    }
    __syncthreads();
    if (on) {
      const float xh = a.xh2[b * w + j], av = lrelu(fmaf(xh, gm2, bt2)), g0 = g_s[2 * g], g1 = g_s[2 * g + 1];
      const float dy = fmaf(w61, g1, w60 * g0) * lrelu_d(av);
      a.dh[b * w + j] = dy;
      sdy += dy;
      sdx = fmaf(dy, xh, sdx);
      q0 = fmaf(g0, av, q0);
      q1 = fmaf(g1, av, q1);
    }
    __syncthreads();
  }
  sdy = col_sum(sdy, part, res, w, G, g, j, active);
  sdx = col_sum(sdx, part, res, w, G, g, j, active);
  q0 = col_sum(q0, part, res, w, G, g, j, active);
  q1 = col_sum(q1, part, res, w, G, g, j, active);
  sb0 = col_sum(sb0, part, res, w, G, g, j, active);  // (channel 0 carries the bias sums)
  sb1 = col_sum(sb1, part, res, w, G, g, j, active);
  if (active && g == 0) {
    a.ggamma[1][j] = sdx;
    a.gbeta[1][j] = sdy;
    a.gw6[j] = q0;
    a.gw6[w + j] = q1;
    if (j == 0) {
      a.gb6[0] = sb0;
      a.gb6[1] = sb1;
    }
  }

  // mlp.4 backward into LDS a tile at a time; mlp.3's weight gradient (each thread owns up to four of its w * w elements and adds
  // the rows in order) and its data gradient; dh <- d / d(mlp.1 output)
  const float k2 = gm2 * a.invstd[w + j], my2 = sdy / (float)n, mx2 = sdx / (float)n;
  const float gm1 = a.gamma[0][j], bt1 = a.beta[0][j];
  for (int e = tid; e < w * w; e += MT) w3s[e] = a.w3[e];
  constexpr int NQ = CGEN_MLP_MAX_WIDTH * CGEN_MLP_MAX_WIDTH / MT;
  float acc[NQ];
  int am[NQ], ai[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = tid + q * MT;
    acc[q] = 0.f;
    am[q] = e / w;
    ai[q] = e - am[q] * w;
  }
  sdy = sdx = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int b = t * G + g;
    const bool on = active && b < n;
    float x1 = 0.f, a1 = 0.f;
    if (on) {
      d_s[tid] = k2 * (a.dh[b * w + j] - my2 - a.xh2[b * w + j] * mx2);
      x1 = a.xh1[b * w + j];
      a1 = lrelu(fmaf(x1, gm1, bt1));
      a_s[tid] = a1;
    }
    __syncthreads();  // (the first one also publishes w3s)
    if (on) {
      float da = 0.f;
#pragma unroll 8
      for (int m = 0; m < w; ++m) da = fmaf(w3s[m * w + j], d_s[g * w + m], da);
      const float dy = da * lrelu_d(a1);
      a.dh[b * w + j] = dy;
      sdy += dy;
      sdx = fmaf(dy, x1, sdx);
    }
    const int rows = n - t * G < G ? n - t * G : G;
#pragma unroll 2
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (am[q] < w) acc[q] = fmaf(d_s[r * w + am[q]], a_s[r * w + ai[q]], acc[q]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (am[q] < w) a.gw3[tid + q * MT] = acc[q];
  sdy = col_sum(sdy, part, res, w, G, g, j, active);
  sdx = col_sum(sdx, part, res, w, G, g, j, active);
  if (active && g == 0) {
    a.ggamma[0][j] = sdx;
    a.gbeta[0][j] = sdy;
  }

  // mlp.1 backward and mlp.0's weight gradient on the own rows
  const float k1 = gm1 * a.invstd[j], my1 = sdy / (float)n, mx1 = sdx / (float)n;
  float ak[CGEN_MLP_MAX_IN];
#pragma unroll
  for (int k = 0; k < CGEN_MLP_MAX_IN; ++k) ak[k] = 0.f;
  if (active)
    for (int b = g; b < n; b += G) {
      const float dz = k1 * (a.dh[b * w + j] - my1 - a.xh1[b * w + j] * mx1);
#pragma unroll
      for (int k = 0; k < CGEN_MLP_MAX_IN; ++k) ak[k] = fmaf(dz, a.in[k][b * a.in_stride[k]], ak[k]);
    }
#pragma unroll
  for (int k = 0; k < CGEN_MLP_MAX_IN; ++k)
    if (k < a.nin) {  // (uniform)
      const float v = col_sum(ak[k], part, res, w, G, g, j, active);
      if (active && g == 0) a.gw0[j * a.nin + k] = v;
    }
}

// ---- host side
int64_t mlp_ws_floats(int n, int w) { return 3 * (int64_t)n * w + 2 * (int64_t)n + 2 * w; }

int mlp_validate(const char* fn, const cgen_mlp_train_head* r, int n, const float* ws, int64_t ws_floats) {
  CGEN_REQUIRE(r, "%s: null head record", fn);
  CGEN_REQUIRE(n >= 2, "%s: n = %d: train-mode BatchNorm needs at least 2 rows", fn, n);
  CGEN_REQUIRE(n <= 4096, "%s: n = %d: one workgroup takes at most 4096 rows", fn, n);
  CGEN_REQUIRE(r->nin >= 1 && r->nin <= CGEN_MLP_MAX_IN, "%s: unsupported number of inputs %d (1..%d)", fn, r->nin, CGEN_MLP_MAX_IN);
  CGEN_REQUIRE(r->width >= 8 && r->width <= CGEN_MLP_MAX_WIDTH && r->width % 8 == 0, "%s: unsupported width %d (a multiple of 8 up to %d)", fn,
               r->width, CGEN_MLP_MAX_WIDTH);
  for (int k = 0; k < r->nin; ++k)
    CGEN_REQUIRE(r->in[k] && r->in_stride[k] >= 0 && r->in_stride[k] < (1 << 16), "%s: null input column %d or bad row stride", fn, k);
  CGEN_REQUIRE(r->obs && r->obs_stride >= 0, "%s: null obs", fn);
  CGEN_REQUIRE(r->w[0] && r->w[1] && r->w[2] && r->bias, "%s: null weight pointer", fn);
  for (int i = 0; i < 2; ++i) {
    CGEN_REQUIRE(r->gamma[i] && r->beta[i] && r->running_mean[i] && r->running_var[i] && r->num_batches_tracked[i],
                 "%s: null BatchNorm pointer (BatchNorm %d)", fn, i);
    CGEN_REQUIRE(r->ggamma[i] && r->gbeta[i], "%s: null BatchNorm gradient pointer (BatchNorm %d)", fn, i);
  }
  CGEN_REQUIRE(r->gw[0] && r->gw[1] && r->gw[2], "%s: null weight gradient pointer", fn);
  CGEN_REQUIRE(r->gb, "%s: null gradient pointer of mlp.6's bias", fn);
  CGEN_REQUIRE(ws, "%s: null workspace", fn);
  const int64_t need = mlp_ws_floats(n, r->width);
  CGEN_REQUIRE(ws_floats >= need, "%s: workspace too small: %lld floats, need %lld", fn, (long long)ws_floats, (long long)need);
  return CGEN_OK;
}

void mlp_args(MlpArgs& p, const cgen_mlp_train_head* r, int n, float* ws) {
  memset(&p, 0, sizeof(p));
  p.hd.kind = CGEN_PRED_NORMAL; p.hd.nout = 2; p.hd.tanh_loc = r->tanh_loc; p.hd.std_fixed = r->std_fixed;
  p.hd.obs = r->obs; p.hd.obs_stride = r->obs_stride;
  const int w = r->width;
  p.n = n; p.nin = r->nin; p.w = w;
  p.G = MT / w < n ? MT / w : n;
  for (int k = 0; k < CGEN_MLP_MAX_IN; ++k) {
    p.in[k] = r->in[k < r->nin ? k : 0];
    p.in_stride[k] = r->in_stride[k < r->nin ? k : 0];
  }
  p.w0 = r->w[0]; p.w3 = r->w[1]; p.w6 = r->w[2]; p.b6 = r->bias;
  p.gw0 = r->gw[0]; p.gw3 = r->gw[1]; p.gw6 = r->gw[2]; p.gb6 = r->gb;
  for (int i = 0; i < 2; ++i) {
    p.gamma[i] = r->gamma[i]; p.beta[i] = r->beta[i]; p.rmean[i] = r->running_mean[i]; p.rvar[i] = r->running_var[i];
    p.nbt[i] = r->num_batches_tracked[i]; p.ggamma[i] = r->ggamma[i]; p.gbeta[i] = r->gbeta[i];
  }
  p.xh1 = ws;
  p.xh2 = p.xh1 + (int64_t)n * w;
  p.dh = p.xh2 + (int64_t)n * w;
  p.out = p.dh + (int64_t)n * w;
  p.invstd = p.out + 2 * (int64_t)n;
}

}  // namespace
}  // namespace cgen

extern "C" int cgen_mlp_train_workspace(const cgen_mlp_train_head* rec, int32_t n, int64_t* floats) {
  const char* fn = "cgen_mlp_train_workspace";
  CGEN_REQUIRE(floats, "%s: null output", fn);
  CGEN_REQUIRE(rec, "%s: null head record", fn);
  CGEN_REQUIRE(n >= 2 && n <= 4096, "%s: n = %d outside 2..4096", fn, n);
  CGEN_REQUIRE(rec->width >= 8 && rec->width <= CGEN_MLP_MAX_WIDTH && rec->width % 8 == 0, "%s: unsupported width %d (a multiple of 8 up to %d)",
               fn, rec->width, CGEN_MLP_MAX_WIDTH);
  *floats = mlp_ws_floats(n, rec->width);
  return CGEN_OK;
}

extern "C" int cgen_mlp_train_fwd(const cgen_mlp_train_head* rec, int32_t n, float* ws, int64_t ws_floats, float momentum, float* terms,
                                  float* loss, cgen_stream_t stream) {
  const char* fn = "cgen_mlp_train_fwd";
  const int rc = mlp_validate(fn, rec, n, ws, ws_floats);
  if (rc) return rc;
  CGEN_REQUIRE(terms, "%s: null terms", fn);
  CGEN_REQUIRE(momentum >= 0.f && momentum <= 1.f, "%s: momentum %g outside [0, 1]", fn, (double)momentum);
  MlpArgs p;
  mlp_args(p, rec, n, ws);
  p.momentum = momentum; p.terms = terms; p.loss = loss;
  hipLaunchKernelGGL(pmlp_fwd, dim3(1), dim3(MT), 0, (hipStream_t)stream, p);
  return check_launch(fn);
}

extern "C" int cgen_mlp_train_bwd(const cgen_mlp_train_head* rec, int32_t n, float* ws, int64_t ws_floats, const float* coef_dev,
                                  cgen_stream_t stream) {
  const char* fn = "cgen_mlp_train_bwd";
  const int rc = mlp_validate(fn, rec, n, ws, ws_floats);
  if (rc) return rc;
  CGEN_REQUIRE(coef_dev, "%s: null coef_dev", fn);
  MlpArgs p;
  mlp_args(p, rec, n, ws);
  p.coef = coef_dev;
  hipLaunchKernelGGL(pmlp_bwd, dim3(1), dim3(MT), 0, (hipStream_t)stream, p);
  return check_launch(fn);
}
