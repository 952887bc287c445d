// ============================================================================ training mode (included at the end of predictor.hip)
// The CNN with batch-statistic BatchNorm: forward, parameter gradients and (optionally) the image gradient, for training the
// anticausal predictors themselves (train_pgm.py sup_epoch).  One launch per layer over the whole batch, on the tiled
// placement's layout: TWO pred_geo stacks per (image, head), `z` (the raw convolutions) and `act` (post-activation, later the
// gradients, walked back in place as the eval backward does).  The data gradients ARE the tiled placement's kernels
// (ptile_conv_bwd / ptile_stem_bwd on the raw weights); everything else is here.  Every reduction over the batch runs inside one
// workgroup, or over per-workgroup partials merged in index order: no atomics, bit-identical reruns.
namespace cgen {
namespace {

constexpr float BN_EPS = 1e-5f;
constexpr int WG_CHUNK = 4096, WG_MAX_SPLIT = 64;  // weight gradient: pixels per workgroup aimed at, most partials per weight

struct TrainArgs {
  cgen_pred_train_head hd[CGEN_PRED_MAX_HEADS];
  int32_t nheads, n;
  const float* x;
  float* act;    // post-activation planes, [pair][per]; the backward turns them into gradients
  float* z;      // pre-BatchNorm planes, same layout
  float* stats;  // [head][2][29 w]: batch mean, then 1 / sqrt(var + eps), of the 7 BatchNorms
  float* tail;   // [head][tail_per]: the tail's per-image rows (TailRows)
  float* part;   // [head][part_per]: partial sums of a split weight gradient
  int64_t per, tail_per, part_per;
  float momentum;
  float* terms;
  float* outs;
  const float* coef;
};

struct TrainLayer {
  int cin, cout, hin, hout, s, pool;
  int64_t in, out, plane;
};

// conv layer L = 0..5; `in` is an offset into the act stack (L >= 1) or unused (L == 0 reads x)
__host__ __device__ inline TrainLayer train_layer(const PredGeo& g, int L) {
  if (L == 0) return {g.c, g.w, g.r, g.h1, g.s1, 0, 0, g.a1, (int64_t)g.r * g.r};
  const TileLayer t = tile_layer(g, L);
  const int pool = L == 1 && g.pool;
  return {t.cin, t.cout, t.hin, t.hout, t.s, pool, t.in, t.out, pool ? (int64_t)g.h1 * g.h1 : (int64_t)t.hin * t.hin};
}

// first channel of BatchNorm i = 0..6 in a head's statistics (widths w, 2w, 2w, 4w, 4w, 8w, 8w)
__host__ __device__ inline int stat_off(int w, int i) {
  return w * (i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 3 : i == 3 ? 5 : i == 4 ? 9 : i == 5 ? 13 : 21);
}

__device__ __forceinline__ float block_bcast_sum(float v, float* sm, float* slot) {
  const float r = block_sum_256(v, sm);
  if (threadIdx.x == 0) *slot = r;
  __syncthreads();
  return *slot;
}

// z[co][p] = sum_{ci,ky,kx} wt[co][ci][ky][kx] * in[ci][oy*S-K/2+ky][ox*S-K/2+kx]: a pixel and 8 output channels per thread,
// pixels on the lanes (the channel group, and with it every weight address, is uniform in the workgroup)
template <int K>
__global__ __launch_bounds__(TNT) void ptrain_conv_fwd(TrainArgs a, int L) {
  constexpr int COB = 8;
  const PredGeo g = pred_geo(a.hd[0].hd);
  const TrainLayer ly = train_layer(g, L);
  const int cin = ly.cin, hin = ly.hin, hout = ly.hout, S = ly.s, hw = hout * hout;
  const int nchunk = (hw + TNT - 1) / TNT, ncog = ly.cout / COB;
  int id = blockIdx.x;
  const int chunk = id % nchunk;
  id /= nchunk;
  const int cog = id % ncog, pair = id / ncog, b = pair / a.nheads, h = pair - b * a.nheads;
  const int p = chunk * TNT + threadIdx.x;
  if (p >= hw) return;
  const float* in = K == 7 ? a.x + (int64_t)b * cin * ly.plane : a.act + (int64_t)pair * a.per + ly.in;
  const float* __restrict__ wt = a.hd[h].hd.w[L];
  const int oy = p / hout, ox = p - oy * hout, iy0 = oy * S - K / 2, ix0 = ox * S - K / 2;
  float acc[COB];
#pragma unroll
  for (int j = 0; j < COB; ++j) acc[j] = 0.f;
  for (int ci = 0; ci < cin; ++ci) {
    const float* ip = in + ci * ly.plane;
    const float* wp = wt + ((int64_t)cog * COB * cin + ci) * K * K;
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
      const int iy = iy0 + ky;
      if (iy < 0 || iy >= hin) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ix0 + kx;
        if (ix < 0 || ix >= hin) continue;
        const float v = (K == 3 && ly.pool) ? pool_value(ip, g.h1, iy, ix) : ip[iy * hin + ix];
#pragma unroll
        for (int j = 0; j < COB; ++j) acc[j] = fmaf(wp[(int64_t)j * cin * K * K + ky * K + kx], v, acc[j]);
      }
    }
  }
  float* out = a.z + (int64_t)pair * a.per + ly.out + (int64_t)cog * COB * hw + p;
#pragma unroll
  for (int j = 0; j < COB; ++j) out[(int64_t)j * hw] = acc[j];
}

// Walks the n * hw values of one channel (value e = b * hw + p of image b) TNT apart without dividing inside the loop
struct ChanIter {
  int b, p, qs, rs, hw;
  __device__ __forceinline__ ChanIter(int start, int hw_) : hw(hw_) {
    b = start / hw_;
    p = start - b * hw_;
    qs = TNT / hw_;
    rs = TNT - qs * hw_;
  }
  __device__ __forceinline__ void next() {
    b += qs;
    p += rs;
    if (p >= hw) { p -= hw; ++b; }
  }
};

// BatchNorm2d of conv layer L in training mode, one workgroup per (channel, head): mean, then the biased variance about that
// mean (second pass over z), the running statistics, then act = lrelu(gamma (z - mean) invstd + beta)
__global__ __launch_bounds__(TNT) void ptrain_bn_fwd(TrainArgs a, int L) {
  __shared__ float sm[4];
  __shared__ float slot[2];
  const PredGeo g = pred_geo(a.hd[0].hd);
  const TrainLayer ly = train_layer(g, L);
  const int c = blockIdx.x % ly.cout, h = blockIdx.x / ly.cout, hw = ly.hout * ly.hout, tid = threadIdx.x, n = a.n;
  const cgen_pred_train_head& hd = a.hd[h];
  const int64_t tot = (int64_t)n * hw, off = ly.out + (int64_t)c * hw, stride = a.nheads * a.per;
  const float* z = a.z + h * a.per + off;
  float s = 0.f;
  for (ChanIter it(tid, hw); it.b < n; it.next()) s += z[it.b * stride + it.p];
  const float mean = block_bcast_sum(s, sm, slot) / (float)tot;
  s = 0.f;
  for (ChanIter it(tid, hw); it.b < n; it.next()) {
    const float d = z[it.b * stride + it.p] - mean;
    s = fmaf(d, d, s);
  }
  const float var = block_bcast_sum(s, sm, slot + 1) / (float)tot;
  const float invstd = 1.f / sqrtf(var + BN_EPS);
  if (tid == 0) {
    float* st = a.stats + (int64_t)h * 58 * g.w + stat_off(g.w, L) + c;
    st[0] = mean;
    st[29 * g.w] = invstd;
    const float mo = a.momentum;
    hd.running_mean[L][c] = (1.f - mo) * hd.running_mean[L][c] + mo * mean;
    hd.running_var[L][c] = (1.f - mo) * hd.running_var[L][c] + mo * (var * ((float)tot / (float)(tot - 1)));
    if (c == 0) hd.num_batches_tracked[L][0] += 1;
  }
  const float sc = hd.gamma[L][c] * invstd, sh = hd.beta[L][c];
  float* act = a.act + h * a.per + off;
  for (ChanIter it(tid, hw); it.b < n; it.next()) {
    const int64_t i = it.b * stride + it.p;
    act[i] = lrelu(fmaf(z[i] - mean, sc, sh));
  }
}

// a head's rows in the tail region: feat [n][8w + 4], hz [n][8w] (fc.0's output), hid [n][8w] (after BatchNorm1d and LeakyReLU),
// dh [n][8w] (backward: d / d hid's pre-activation, then d / d hz), out [n][CGEN_PRED_MAX_OUT] (backward: coef * d nll / d out)
struct TailRows {
  float *feat, *hz, *hid, *dh, *out;
  int nf, fp;
};
__device__ __forceinline__ TailRows tail_rows(const TrainArgs& a, int h, int w) {
  TailRows t;
  t.nf = 8 * w;
  t.fp = t.nf + 4;
  const int64_t n = a.n;
  t.feat = a.tail + (int64_t)h * a.tail_per;
  t.hz = t.feat + n * t.fp;
  t.hid = t.hz + n * t.nf;
  t.dh = t.hid + n * t.nf;
  t.out = t.dh + n * t.nf;
  return t;
}

// Tail, one workgroup per (image, head): feat = [spatial mean of the last planes, y]; hz = fc.0 feat (no bias)
__global__ __launch_bounds__(TNT) void ptrain_tail_fc0(TrainArgs a) {
  __shared__ float feat[HS_HID];
  const int pair = blockIdx.x, b = pair / a.nheads, h = pair - b * a.nheads, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const cgen_pred_head& hd = a.hd[h].hd;
  const PredGeo g = pred_geo(hd);
  const float* A6 = a.act + (int64_t)pair * a.per + g.a6;
  const TailRows t = tail_rows(a, h, g.w);
  const int nf = t.nf, hw6 = g.h6 * g.h6, nin = nf + hd.ctx;
  float* featg = t.feat + (int64_t)b * t.fp;
  float* hz = t.hz + (int64_t)b * nf;
  for (int c = tid; c < nin; c += TNT) {
    float v;
    if (c < nf) {
      float s = 0.f;
      for (int q = 0; q < hw6; ++q) s += A6[c * hw6 + q];
      v = s / (float)hw6;
    } else {
      v = hd.y[(int64_t)b * hd.ctx + (c - nf)];
    }
    feat[c] = v;
    featg[c] = v;
  }
  __syncthreads();
  for (int j = wave; j < nf; j += TNT / 64) {
    const float s = wave_dot(hd.w[6] + (int64_t)j * nin, feat, nin, lane);
    if (lane == 0) hz[j] = s;
  }
}

// BatchNorm1d over the n images + LeakyReLU: a thread per channel walks the images in order; 64 channels per workgroup
__global__ __launch_bounds__(64) void ptrain_tail_bn(TrainArgs a) {
  const int h = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x, n = a.n;
  const cgen_pred_train_head& th = a.hd[h];
  const PredGeo g = pred_geo(th.hd);
  const TailRows t = tail_rows(a, h, g.w);
  const int nf = t.nf;
  if (j >= nf) return;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < n; ++b) s += t.hz[(int64_t)b * nf + j];
  const float mean = s / (float)n;
  s = 0.f;
#pragma unroll 8
  for (int b = 0; b < n; ++b) {
    const float d = t.hz[(int64_t)b * nf + j] - mean;
    s = fmaf(d, d, s);
  }
  const float var = s / (float)n, invstd = 1.f / sqrtf(var + BN_EPS);
  float* st = a.stats + (int64_t)h * 58 * g.w + stat_off(g.w, 6) + j;
  st[0] = mean;
  st[29 * g.w] = invstd;
  const float mo = a.momentum;
  th.running_mean[6][j] = (1.f - mo) * th.running_mean[6][j] + mo * mean;
  th.running_var[6][j] = (1.f - mo) * th.running_var[6][j] + mo * (var * ((float)n / (float)(n - 1)));
  if (j == 0) th.num_batches_tracked[6][0] += 1;
  const float sc = th.gamma[6][j] * invstd, sh = th.beta[6][j];
#pragma unroll 8
  for (int b = 0; b < n; ++b) t.hid[(int64_t)b * nf + j] = lrelu(fmaf(t.hz[(int64_t)b * nf + j] - mean, sc, sh));
}

// fc.3 and the likelihood (forward), or coef * d nll / d out and d / d(hid's pre-activation) (backward): one workgroup per
// (image, head)
template <bool BWD>
__global__ __launch_bounds__(TNT) void ptrain_tail_out(TrainArgs a) {
  __shared__ float hid[HS_HID];
  __shared__ float o_s[CGEN_PRED_MAX_OUT];
  __shared__ float g_s[CGEN_PRED_MAX_OUT];
  const int pair = blockIdx.x, b = pair / a.nheads, h = pair - b * a.nheads, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const cgen_pred_head& hd = a.hd[h].hd;
  const PredGeo g = pred_geo(hd);
  const TailRows t = tail_rows(a, h, g.w);
  const int nf = t.nf;
  float* out = t.out + (int64_t)b * CGEN_PRED_MAX_OUT;
  const float* obs = hd.obs + (int64_t)b * hd.obs_stride;
  if (!BWD) {
    for (int j = tid; j < nf; j += TNT) hid[j] = t.hid[(int64_t)b * nf + j];
    __syncthreads();
    for (int o = wave; o < hd.nout; o += TNT / 64) {
      const float s = wave_dot(hd.w[7] + (int64_t)o * nf, hid, nf, lane);
      if (lane == 0) o_s[o] = s + hd.b[7][o];
    }
    __syncthreads();
    if (tid == 0) {
      a.terms[(int64_t)b * a.nheads + h] = pred_nll(hd, o_s, obs, nullptr);
      for (int o = 0; o < hd.nout; ++o) {
        out[o] = o_s[o];
        if (a.outs) a.outs[((int64_t)h * a.n + b) * CGEN_PRED_MAX_OUT + o] = o_s[o];
      }
    }
    return;
  }
  if (tid < hd.nout) o_s[tid] = out[tid];
  __syncthreads();
  if (tid == 0) {
    pred_nll(hd, o_s, obs, g_s);
    const float cf = a.coef[0];
    for (int o = 0; o < hd.nout; ++o) {
      g_s[o] *= cf;
      out[o] = g_s[o];
    }
  }
  __syncthreads();
  for (int j = tid; j < nf; j += TNT) {
    float s = 0.f;
    for (int o = 0; o < hd.nout; ++o) s = fmaf(hd.w[7][(int64_t)o * nf + j], g_s[o], s);
    t.dh[(int64_t)b * nf + j] = s * lrelu_d(t.hid[(int64_t)b * nf + j]);
  }
}

// BatchNorm1d backward, a thread per channel: dh holds dY; gamma / beta gradients; dh <- d / d hz
__global__ __launch_bounds__(64) void ptrain_tail_bn_bwd(TrainArgs a) {
  const int h = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x, n = a.n;
  const cgen_pred_train_head& th = a.hd[h];
  const PredGeo g = pred_geo(th.hd);
  const TailRows t = tail_rows(a, h, g.w);
  const int nf = t.nf;
  if (j >= nf) return;
  const float* st = a.stats + (int64_t)h * 58 * g.w + stat_off(g.w, 6) + j;
  const float mean = st[0], invstd = st[29 * g.w];
  float sdy = 0.f, sdx = 0.f;
#pragma unroll 8
  for (int b = 0; b < n; ++b) {
    const float dy = t.dh[(int64_t)b * nf + j];
    sdy += dy;
    sdx = fmaf(dy, (t.hz[(int64_t)b * nf + j] - mean) * invstd, sdx);
  }
  th.ggamma[6][j] = sdx;
  th.gbeta[6][j] = sdy;
  const float k = th.gamma[6][j] * invstd, my = sdy / (float)n, mx = sdx / (float)n;
#pragma unroll 8
  for (int b = 0; b < n; ++b) {
    const float xh = (t.hz[(int64_t)b * nf + j] - mean) * invstd;
    t.dh[(int64_t)b * nf + j] = k * (t.dh[(int64_t)b * nf + j] - my - xh * mx);
  }
}

// Weight gradients of the two linears, one workgroup per (row, head), images in order.  Row j < 8w: d fc.0 weight[j][i] =
// sum_b dhz[b][j] feat[b][i].  Row 8w + o: d fc.3 weight[o][j] = sum_b gout[b][o] hid[b][j], and d fc.3 bias[o] = sum_b gout[b][o]
__global__ __launch_bounds__(TNT) void ptrain_tail_fc_wgrad(TrainArgs a) {
  const cgen_pred_train_head& th = a.hd[blockIdx.y];
  const PredGeo g = pred_geo(th.hd);
  const TailRows t = tail_rows(a, blockIdx.y, g.w);
  const int nf = t.nf, nin = nf + th.hd.ctx, n = a.n, row = blockIdx.x;
  if (row < nf) {
    for (int i = threadIdx.x; i < nin; i += TNT) {
      float s = 0.f;
#pragma unroll 8
      for (int b = 0; b < n; ++b) s = fmaf(t.dh[(int64_t)b * nf + row], t.feat[(int64_t)b * t.fp + i], s);
      th.gw[6][(int64_t)row * nin + i] = s;
    }
    return;
  }
  const int o = row - nf;
  if (o >= th.hd.nout) return;
  for (int j = threadIdx.x; j < nf; j += TNT) {
    float s = 0.f, sb = 0.f;
#pragma unroll 8
    for (int b = 0; b < n; ++b) {
      const float gv = t.out[b * CGEN_PRED_MAX_OUT + o];
      s = fmaf(gv, t.hid[(int64_t)b * nf + j], s);
      sb += gv;
    }
    th.gw[7][(int64_t)o * nf + j] = s;
    if (j == 0) th.gb[o] = sb;
  }
}

// the last conv's planes become d / d(its BatchNorm output): one workgroup per (image, head)
__global__ __launch_bounds__(TNT) void ptrain_tail_fc0_dgrad(TrainArgs a) {
  __shared__ float dh[HS_HID];
  __shared__ float df[HS_HID];
  const int pair = blockIdx.x, b = pair / a.nheads, h = pair - b * a.nheads, tid = threadIdx.x;
  const cgen_pred_head& hd = a.hd[h].hd;
  const PredGeo g = pred_geo(hd);
  const TailRows t = tail_rows(a, h, g.w);
  const int nf = t.nf, nin = nf + hd.ctx, hw6 = g.h6 * g.h6;
  float* A6 = a.act + (int64_t)pair * a.per + g.a6;
  for (int j = tid; j < nf; j += TNT) dh[j] = t.dh[(int64_t)b * nf + j];
  __syncthreads();
  for (int i = tid; i < nf; i += TNT) {
    float s = 0.f;
    for (int j = 0; j < nf; ++j) s = fmaf(hd.w[6][(int64_t)j * nin + i], dh[j], s);
    df[i] = s / (float)hw6;
  }
  __syncthreads();
  for (int t2 = tid; t2 < nf * hw6; t2 += TNT) A6[t2] = df[t2 / hw6] * lrelu_d(A6[t2]);
}

// BatchNorm2d backward of conv layer L, one workgroup per (channel, head).  The layer's act planes hold dY = d / d(BatchNorm
// output); they become dZ = gamma invstd (dY - mean(dY) - xhat mean(dY xhat)), the gradient of the raw convolution
__global__ __launch_bounds__(TNT) void ptrain_bn_bwd(TrainArgs a, int L) {
  __shared__ float sm[4];
  __shared__ float slot[2];
  const PredGeo g = pred_geo(a.hd[0].hd);
  const TrainLayer ly = train_layer(g, L);
  const int c = blockIdx.x % ly.cout, h = blockIdx.x / ly.cout, hw = ly.hout * ly.hout, tid = threadIdx.x, n = a.n;
  const cgen_pred_train_head& hd = a.hd[h];
  const int64_t tot = (int64_t)n * hw, off = ly.out + (int64_t)c * hw, stride = a.nheads * a.per;
  const float* z = a.z + h * a.per + off;
  float* dy = a.act + h * a.per + off;
  const float* st = a.stats + (int64_t)h * 58 * g.w + stat_off(g.w, L) + c;
  const float mean = st[0], invstd = st[29 * g.w];
  float s0 = 0.f, s1 = 0.f;
  for (ChanIter it(tid, hw); it.b < n; it.next()) {
    const int64_t i = it.b * stride + it.p;
    const float d = dy[i];
    s0 += d;
    s1 = fmaf(d, (z[i] - mean) * invstd, s1);
  }
  const float sdy = block_bcast_sum(s0, sm, slot), sdx = block_bcast_sum(s1, sm, slot + 1);
  if (tid == 0) {
    hd.ggamma[L][c] = sdx;
    hd.gbeta[L][c] = sdy;
  }
  const float k = hd.gamma[L][c] * invstd, my = sdy / (float)tot, mx = sdx / (float)tot;
  for (ChanIter it(tid, hw); it.b < n; it.next()) {
    const int64_t i = it.b * stride + it.p;
    dy[i] = k * (dy[i] - my - (z[i] - mean) * invstd * mx);
  }
}

// dW[co][ci][ky][kx] = sum_{b,oy,ox} dZ[b][co][oy][ox] * in[b][ci][oy*S-K/2+ky][ox*S-K/2+kx] of conv layer L: one workgroup per
// (slice of the b*oy*ox range, ci, co, head), K*K sums per thread, then a fixed tree.  One slice: straight into the gradient;
// more: into `part`, which ptrain_wgrad_reduce adds up in slice order.  Layer 1 reads the pooled stem on the fly.
template <int K>
__global__ __launch_bounds__(TNT) void ptrain_conv_wgrad(TrainArgs a, int L, int nsplit, int chunk) {
  __shared__ float sm[4];
  const PredGeo g = pred_geo(a.hd[0].hd);
  const TrainLayer ly = train_layer(g, L);
  const int cin = ly.cin, cout = ly.cout, hin = ly.hin, hout = ly.hout, S = ly.s, hw = hout * hout;
  int id = blockIdx.x;
  const int sp = id % nsplit;
  id /= nsplit;
  const int ci = id % cin;
  id /= cin;
  const int co = id % cout, h = id / cout;
  const int64_t tot = (int64_t)a.n * hw, q0 = (int64_t)sp * chunk, q1 = q0 + chunk < tot ? q0 + chunk : tot;
  float acc[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
  ChanIter it((int)q0 + (int)threadIdx.x, hw);
  for (int64_t q = q0 + threadIdx.x; q < q1; q += TNT, it.next()) {
    const int b = it.b, p = it.p, oy = p / hout, ox = p - oy * hout;
    const int64_t pair = (int64_t)b * a.nheads + h;
    const float gv = a.act[pair * a.per + ly.out + (int64_t)co * hw + p];
    const float* ip = (K == 7 ? a.x + (int64_t)b * cin * ly.plane : a.act + pair * a.per + ly.in) + ci * ly.plane;
    const int iy0 = oy * S - K / 2, ix0 = ox * S - K / 2;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = iy0 + ky;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ix0 + kx;
        float v = 0.f;
        if (iy >= 0 && iy < hin && ix >= 0 && ix < hin) v = (K == 3 && ly.pool) ? pool_value(ip, g.h1, iy, ix) : ip[iy * hin + ix];
        acc[ky * K + kx] = fmaf(gv, v, acc[ky * K + kx]);
      }
    }
  }
  const int64_t wi = ((int64_t)co * cin + ci) * K * K;
  float* dst = nsplit == 1 ? a.hd[h].gw[L] + wi : a.part + h * a.part_per + (int64_t)sp * cout * cin * K * K + wi;
#pragma unroll
  for (int t = 0; t < K * K; ++t) {
    const float r = block_sum_256(acc[t], sm);
    if (threadIdx.x == 0) dst[t] = r;
  }
}

__global__ __launch_bounds__(TNT) void ptrain_wgrad_reduce(TrainArgs a, int L, int nsplit, int wcount) {
  const int i = blockIdx.x * TNT + threadIdx.x, h = blockIdx.y;
  if (i >= wcount) return;
  const float* p = a.part + h * a.part_per + i;
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += p[(int64_t)sp * wcount];
  a.hd[h].gw[L][i] = s;
}

// ---- host side
struct TrainPlan {
  PredGeo g;
  int nsplit[6], chunk[6];
  int64_t stack, stats, tail_per, part_per, total;
};

TrainPlan train_plan(const cgen_pred_train_head* heads, int nheads, int n) {
  TrainPlan t;
  t.g = pred_geo(heads[0].hd);
  const int w = t.g.w;
  t.part_per = 0;
  for (int L = 0; L < 6; ++L) {
    const TrainLayer ly = train_layer(t.g, L);
    const int64_t tot = (int64_t)n * ly.hout * ly.hout, k = L == 0 ? 49 : 9;
    int64_t ns = (tot + WG_CHUNK - 1) / WG_CHUNK;
    if (ns > WG_MAX_SPLIT) ns = WG_MAX_SPLIT;
    t.chunk[L] = (int)((tot + ns - 1) / ns);
    t.nsplit[L] = (int)((tot + t.chunk[L] - 1) / t.chunk[L]);
    const int64_t need = t.nsplit[L] > 1 ? (int64_t)t.nsplit[L] * ly.cout * ly.cin * k : 0;
    if (need > t.part_per) t.part_per = need;
  }
  t.part_per = (t.part_per + 3) & ~(int64_t)3;
  t.stack = (int64_t)n * nheads * t.g.total;
  t.stats = (int64_t)nheads * 58 * w;
  t.tail_per = ((int64_t)n * (8 * w + 4 + 3 * 8 * w + CGEN_PRED_MAX_OUT) + 3) & ~(int64_t)3;
  t.total = 2 * t.stack + t.stats + nheads * (t.tail_per + t.part_per);
  return t;
}

bool train_shapes_ok(const cgen_pred_train_head* heads, int nheads) {
  if (!heads || nheads < 1 || nheads > CGEN_PRED_MAX_HEADS) return false;
  cgen_pred_head tmp[CGEN_PRED_MAX_HEADS];
  for (int h = 0; h < nheads; ++h) tmp[h] = heads[h].hd;
  return tile_shapes_ok(tmp, nheads);
}

int train_validate(const char* fn, const cgen_pred_train_head* heads, int nheads, int n, const float* x, const float* ws,
                   int64_t ws_floats) {
  CGEN_REQUIRE(heads && nheads >= 1 && nheads <= CGEN_PRED_MAX_HEADS, "%s: need 1..%d head records", fn, CGEN_PRED_MAX_HEADS);
  cgen_pred_head tmp[CGEN_PRED_MAX_HEADS];
  for (int h = 0; h < nheads; ++h) {
    tmp[h] = heads[h].hd;
    for (int i = 0; i < 7; ++i) tmp[h].b[i] = tmp[h].b[7];  // (only fc.3 has a bias here)
  }
  const int rc = pred_validate(fn, tmp, nheads, n, x, true);
  if (rc) return rc;
  CGEN_REQUIRE(n >= 2, "%s: n = %d: train-mode BatchNorm needs at least 2 images", fn, n);
  for (int h = 0; h < nheads; ++h) {
    const cgen_pred_train_head& t = heads[h];
    CGEN_REQUIRE(t.hd.width == heads[0].hd.width, "%s: head %d: width %d differs from head 0's %d (training needs equal widths)", fn, h,
                 t.hd.width, heads[0].hd.width);
    for (int i = 0; i < 7; ++i) {
      CGEN_REQUIRE(t.gamma[i] && t.beta[i] && t.running_mean[i] && t.running_var[i] && t.num_batches_tracked[i],
                   "%s: head %d: null BatchNorm pointer (BatchNorm %d)", fn, h, i);
      CGEN_REQUIRE(t.ggamma[i] && t.gbeta[i], "%s: head %d: null BatchNorm gradient pointer (BatchNorm %d)", fn, h, i);
    }
    for (int i = 0; i < 8; ++i) CGEN_REQUIRE(t.gw[i], "%s: head %d: null weight gradient pointer (layer %d)", fn, h, i);
    CGEN_REQUIRE(t.gb, "%s: head %d: null gradient pointer of fc.3's bias", fn, h);
  }
  CGEN_REQUIRE(ws, "%s: null workspace", fn);
  const int64_t need = train_plan(heads, nheads, n).total;
  CGEN_REQUIRE(ws_floats >= need, "%s: workspace too small: %lld floats, need %lld", fn, (long long)ws_floats, (long long)need);
  const PredGeo g = pred_geo(heads[0].hd);
  CGEN_REQUIRE((int64_t)n * nheads * 4096 < INT32_MAX && (int64_t)n * g.h1 * g.h1 < INT32_MAX / 2, "%s: batch %d is too large for one launch",
               fn, n);
  return CGEN_OK;
}

void train_args(TrainArgs& p, const TrainPlan& t, const cgen_pred_train_head* heads, int nheads, int n, const float* x, float* ws) {
  memset(&p, 0, sizeof(p));
  for (int h = 0; h < nheads; ++h) p.hd[h] = heads[h];
  p.nheads = nheads; p.n = n; p.x = x;
  p.act = ws;
  p.z = p.act + t.stack;
  p.stats = p.z + t.stack;
  p.tail = p.stats + t.stats;
  p.part = p.tail + nheads * t.tail_per;
  p.per = t.g.total; p.tail_per = t.tail_per; p.part_per = t.part_per;
}

}  // namespace
}  // namespace cgen

extern "C" int cgen_predictor_train_workspace(const cgen_pred_train_head* heads, int32_t nheads, int32_t n, int64_t* floats) {
  CGEN_REQUIRE(floats, "cgen_predictor_train_workspace: null output");
  CGEN_REQUIRE(n >= 2, "cgen_predictor_train_workspace: n = %d: train-mode BatchNorm needs at least 2 images", n);
  CGEN_REQUIRE(train_shapes_ok(heads, nheads), "cgen_predictor_train_workspace: training does not take these heads");
  *floats = train_plan(heads, nheads, n).total;
  return CGEN_OK;
}

extern "C" int cgen_predictor_train_fwd(const cgen_pred_train_head* heads, int32_t nheads, int32_t n, const float* x, float* ws,
                                        int64_t ws_floats, float momentum, float* terms, float* outs, float* loss,
                                        cgen_stream_t stream) {
  const char* fn = "cgen_predictor_train_fwd";
  const int rc = train_validate(fn, heads, nheads, n, x, ws, ws_floats);
  if (rc) return rc;
  CGEN_REQUIRE(terms, "%s: null terms", fn);
  CGEN_REQUIRE(momentum >= 0.f && momentum <= 1.f, "%s: momentum %g outside [0, 1]", fn, (double)momentum);
  const TrainPlan t = train_plan(heads, nheads, n);
  TrainArgs p;
  train_args(p, t, heads, nheads, n, x, ws);
  p.momentum = momentum; p.terms = terms; p.outs = outs;
  hipStream_t st = (hipStream_t)stream;
  const int64_t pairs = (int64_t)n * nheads;
  for (int L = 0; L < 6; ++L) {
    const TrainLayer ly = train_layer(t.g, L);
    const int hw = ly.hout * ly.hout;
    const int64_t blocks = pairs * (ly.cout / 8) * ((hw + TNT - 1) / TNT);
    if (L == 0) TILE_LAUNCH(ptrain_conv_fwd<7>, blocks, p, L);
    else TILE_LAUNCH(ptrain_conv_fwd<3>, blocks, p, L);
    TILE_LAUNCH(ptrain_bn_fwd, nheads * ly.cout, p, L);
  }
  TILE_LAUNCH(ptrain_tail_fc0, pairs, p);
  hipLaunchKernelGGL(ptrain_tail_bn, dim3((8 * t.g.w + 63) / 64, nheads), dim3(64), 0, st, p);
  TILE_LAUNCH(ptrain_tail_out<false>, pairs, p);
  if (loss) hipLaunchKernelGGL(pred_sum_kernel, dim3(1), dim3(256), 0, st, terms, pairs, loss);
  return check_launch(fn);
}

extern "C" int cgen_predictor_train_bwd(const cgen_pred_train_head* heads, int32_t nheads, int32_t n, const float* x, float* ws,
                                        int64_t ws_floats, const float* coef_dev, float* dx, cgen_stream_t stream) {
  const char* fn = "cgen_predictor_train_bwd";
  const int rc = train_validate(fn, heads, nheads, n, x, ws, ws_floats);
  if (rc) return rc;
  CGEN_REQUIRE(coef_dev, "%s: null coef_dev", fn);
  const TrainPlan t = train_plan(heads, nheads, n);
  TrainArgs p;
  train_args(p, t, heads, nheads, n, x, ws);
  p.coef = coef_dev;
  TileArgs q;  // the data gradients are the tiled placement's, on the raw weights and the act stack
  memset(&q, 0, sizeof(q));
  for (int h = 0; h < nheads; ++h) q.hd[h] = heads[h].hd;
  q.nheads = nheads; q.n = n; q.x = x; q.ws = p.act; q.per = p.per; q.dx = dx;
  hipStream_t st = (hipStream_t)stream;
  const int64_t pairs = (int64_t)n * nheads;
  const int nf = 8 * t.g.w;
  TILE_LAUNCH(ptrain_tail_out<true>, pairs, p);
  hipLaunchKernelGGL(ptrain_tail_bn_bwd, dim3((nf + 63) / 64, nheads), dim3(64), 0, st, p);
  hipLaunchKernelGGL(ptrain_tail_fc_wgrad, dim3(nf + CGEN_PRED_MAX_OUT, nheads), dim3(TNT), 0, st, p);
  TILE_LAUNCH(ptrain_tail_fc0_dgrad, pairs, p);
  for (int L = 5; L >= 0; --L) {
    const TrainLayer ly = train_layer(t.g, L);
    TILE_LAUNCH(ptrain_bn_bwd, nheads * ly.cout, p, L);
    const int64_t blocks = (int64_t)nheads * ly.cout * ly.cin * t.nsplit[L];
    if (L == 0) TILE_LAUNCH(ptrain_conv_wgrad<7>, blocks, p, L, t.nsplit[L], t.chunk[L]);
    else TILE_LAUNCH(ptrain_conv_wgrad<3>, blocks, p, L, t.nsplit[L], t.chunk[L]);
    if (t.nsplit[L] > 1) {
      const int wcount = ly.cout * ly.cin * (L == 0 ? 49 : 9);
      hipLaunchKernelGGL(ptrain_wgrad_reduce, dim3((wcount + TNT - 1) / TNT, nheads), dim3(TNT), 0, st, p, L, t.nsplit[L], wcount);
    }
    if (L >= 1) tile_bwd_layer(q, t.g, L, st);  // (after this layer's weight gradient: it overwrites the layer's input planes)
    else if (dx) tile_bwd_stem(q, t.g, st);
  }
  return check_launch(fn);
}
