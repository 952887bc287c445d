// Counterfactual fine-tuning (train_cf.py:140-180, dscm.py:75-88) -- what CfTrainStep adds to the shared step tail:
//   cgen_nonfinite_partial   per-block counts of non-finite head outputs (the reference's check_nan: cf_pixels clamps NaN away)
//   cgen_cf_lagrange         the Lagrangian, its gradient seeds, the multiplier's gradient, the step's gate, the running sums
//   cgen_lagrange_step       AdamW(maximize) on the multiplier, its clamp at 0 and the EMA of the clamped value
// Fixed-order sums, plain vector stores, no atomics: reruns are bit-identical.  Every entry point only enqueues.
#include "common.h"
#include "optim_sched.h"

namespace cgen {

__device__ __forceinline__ bool nonfinite(float v) { return !(fabsf(v) <= 3.402823466e38f); }

// deterministic integer block sum for blockDim.x == 256; result valid in thread 0; `sm` >= 4 ints
__device__ __forceinline__ int block_isum_256(int v, int* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  if (threadIdx.x == 0) r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  return r;
}

// Logical element i of the NHWC view = ((n h + y) w + x) c + ch; element -> (block, thread, iteration) as sumsq_partial_kernel.
template <typename T>
__global__ __launch_bounds__(256) void nonfinite_partial_kernel(View v, uint32_t count, uint32_t h, uint32_t w, uint32_t c,
                                                                int32_t* partial) {
  __shared__ int sm[4];
  int a = 0;
  for (uint64_t i64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; i64 < count; i64 += (uint64_t)gridDim.x * 256) {
    const uint32_t i = (uint32_t)i64;
    const uint32_t pix = i / c, ch = i - pix * c;
    const uint32_t row = pix / w, x = pix - row * w;
    const uint32_t n = row / h, y = row - n * h;
    const T* p = (const T*)v.p + ((int64_t)n * v.sn + (int64_t)y * v.sh + (int64_t)x * v.sw + ch);
    a += nonfinite(Elem<T>::ld(p)) ? 1 : 0;
  }
  const int t = block_isum_256(a, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

struct LagrangeP {
  const float* out3; const float* aux_sum; const float* aux_add; const float* lmbda; const float* beta_dev;
  const int32_t* nonfinite; int n_nonfinite;
  float inv_b, eps, damping, seed_scale, beta;
  float* res; float* coef; float* gsq_slot; float* gate; float* sums;
};

__global__ __launch_bounds__(256) void cf_lagrange_kernel(LagrangeP a) {
  __shared__ int sm[4];
  int cnt = 0;
  for (int i = threadIdx.x; i < a.n_nonfinite; i += 256) cnt += a.nonfinite[i];
  const int nbad = block_isum_256(cnt, sm);
  if (threadIdx.x != 0) return;
  const float elbo = a.out3[0], nll = a.out3[1], kl = a.out3[2];
  const float beta = a.beta_dev ? *a.beta_dev : a.beta;
  float aux = *a.aux_sum;
  if (a.aux_add) aux += *a.aux_add;
  aux *= a.inv_b;
  // (every product rounded on its own, never contracted into an fma: the values the host composition's separate torch ops give)
  const float c = a.eps - elbo;                            // the constraint's slack
  const float w = *a.lmbda - __fmul_rn(a.damping, c);      // d loss / d elbo, the damping term under stop-gradient (dscm.py:80-84)
  const float loss = aux - __fmul_rn(w, c);
  const float g_l = -c;                         // d loss / d lmbda
  const bool bad = nonfinite(loss) || nbad > 0;
  a.res[0] = loss; a.res[1] = aux; a.res[2] = g_l; a.res[3] = w;
  a.coef[0] = __fmul_rn(w, a.seed_scale); a.coef[1] = __fmul_rn(__fmul_rn(w, beta), a.seed_scale); a.coef[2] = beta;
  *a.gsq_slot = g_l * g_l;
  a.gate[0] = loss; a.gate[1] = bad ? __builtin_nanf("") : nll; a.gate[2] = kl;
  if (bad) {
    a.sums[6] += 1.f;
  } else {
    a.sums[0] += loss; a.sums[1] += aux; a.sums[2] += elbo; a.sums[3] += nll; a.sums[4] += kl; a.sums[5] += 1.f;
  }
}

struct LagStepP {
  float* lmbda; float* m; float* v; float* ema; const float* g; const float* state;
  float lr, beta1, beta2, eps, ema_beta;
  int ema_update_after;
};

// The moment updates and bias corrections as adamw_ema_kernel writes them (wd = 0, constant lr), on the NEGATED clipped gradient
// (maximize=True); then the clamp; then the EMA of the clamped value.
__global__ void lagrange_step_kernel(LagStepP a) {
  if (a.state[3] != 0.f) return;  // skipped step: the multiplier, its moments and its EMA untouched
  const float clip = a.state[2];
  const int t0 = (int)a.state[5];
  const float t = (float)(t0 + 1);
  const float bc1 = 1.f - powf(a.beta1, t);
  const float bc2s = sqrtf(1.f - powf(a.beta2, t));
  const float step = a.lr / bc1;
  const float ema_decay = ema_decay_of(t0, a.ema_update_after, a.ema_beta);
  const float g = -(a.g[0] * clip);
  float p = a.lmbda[0];
  float m = a.m[0];
  m = m + (g - m) * (1.f - a.beta1);
  const float v = a.v[0] * a.beta2 + (1.f - a.beta2) * g * g;
  const float denom = sqrtf(v) / bc2s + a.eps;
  p = p - step * (m / denom);
  p = p < 0.f ? 0.f : p;  // lmbda.data.clamp_(min=0); a NaN stays a NaN
  a.lmbda[0] = p; a.m[0] = m; a.v[0] = v;
  if (a.ema) {
    if (ema_decay < 0.f) a.ema[0] = p;
    else { const float e = a.ema[0]; a.ema[0] = e - (e - p) * (1.f - ema_decay); }
  }
}

}  // namespace cgen

using namespace cgen;

extern "C" int cgen_nonfinite_partial(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view v, int32_t* partial, int32_t nblk,
                                      cgen_stream_t stream) {
  CGEN_REQUIRE(dtype == CGEN_F32 || dtype == CGEN_F16, "cgen_nonfinite_partial: dtype %d is neither CGEN_F32 nor CGEN_F16", dtype);
  CGEN_REQUIRE(v.p && partial, "cgen_nonfinite_partial: null view or partial");
  CGEN_REQUIRE(n > 0 && h > 0 && w > 0 && v.c > 0 && nblk > 0 && nblk <= 65535, "cgen_nonfinite_partial: bad sizes (n %d h %d w %d c %d nblk %d)",
               n, h, w, v.c, nblk);
  CGEN_REQUIRE(v.sw >= v.c && v.sh >= 0 && v.sn >= 0, "cgen_nonfinite_partial: the channel stride %lld is below the %d channels",
               (long long)v.sw, v.c);
  const int64_t count = (int64_t)n * h * w * v.c;
  CGEN_REQUIRE(count < ((int64_t)1 << 31), "cgen_nonfinite_partial: %lld elements, the kernel indexes below 2^31", (long long)count);
  const View d = mk(v);
  if (dtype == CGEN_F32)
    hipLaunchKernelGGL(nonfinite_partial_kernel<float>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, d, (uint32_t)count, (uint32_t)h,
                       (uint32_t)w, (uint32_t)v.c, partial);
  else
    hipLaunchKernelGGL(nonfinite_partial_kernel<h16_t>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, d, (uint32_t)count, (uint32_t)h,
                       (uint32_t)w, (uint32_t)v.c, partial);
  return check_launch("cgen_nonfinite_partial");
}

extern "C" int cgen_cf_lagrange(const cgen_cf_lagrange_args* a, cgen_stream_t stream) {
  CGEN_REQUIRE(a, "cgen_cf_lagrange: null args");
  CGEN_REQUIRE(a->out3 && a->aux_sum && a->lmbda, "cgen_cf_lagrange: out3, aux_sum and lmbda are needed");
  CGEN_REQUIRE(a->res && a->coef && a->gsq_slot && a->gate && a->sums, "cgen_cf_lagrange: an output pointer is null");
  CGEN_REQUIRE(a->n_nonfinite >= 0 && (a->n_nonfinite == 0 || a->nonfinite), "cgen_cf_lagrange: %d non-finite counts without their array",
               a->n_nonfinite);
  CGEN_REQUIRE(a->inv_b > 0.f && a->inv_b <= 1.f, "cgen_cf_lagrange: inv_b = %g is not 1 / batch size", (double)a->inv_b);
  CGEN_REQUIRE(a->seed_scale > 0.f, "cgen_cf_lagrange: seed_scale = %g must be positive", (double)a->seed_scale);
  LagrangeP p;
  p.out3 = a->out3; p.aux_sum = a->aux_sum; p.aux_add = a->aux_add; p.lmbda = a->lmbda; p.beta_dev = a->beta_dev;
  p.nonfinite = a->nonfinite; p.n_nonfinite = a->n_nonfinite;
  p.inv_b = a->inv_b; p.eps = a->eps; p.damping = a->damping; p.seed_scale = a->seed_scale; p.beta = a->beta;
  p.res = a->res; p.coef = a->coef; p.gsq_slot = a->gsq_slot; p.gate = a->gate; p.sums = a->sums;
  hipLaunchKernelGGL(cf_lagrange_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("cgen_cf_lagrange");
}

extern "C" int cgen_lagrange_step(const cgen_lagrange_step_args* a, cgen_stream_t stream) {
  CGEN_REQUIRE(a, "cgen_lagrange_step: null args");
  CGEN_REQUIRE(a->lmbda && a->m && a->v && a->g && a->state_dev, "cgen_lagrange_step: lmbda, m, v, g and state_dev are needed");
  CGEN_REQUIRE(a->lr > 0.f, "cgen_lagrange_step: lr = %g must be positive", (double)a->lr);
  CGEN_REQUIRE(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f, "cgen_lagrange_step: betas (%g, %g) outside [0, 1)",
               (double)a->beta1, (double)a->beta2);
  LagStepP p;
  p.lmbda = a->lmbda; p.m = a->m; p.v = a->v; p.ema = a->ema; p.g = a->g; p.state = a->state_dev;
  p.lr = a->lr; p.beta1 = a->beta1; p.beta2 = a->beta2; p.eps = a->eps; p.ema_beta = a->ema_beta; p.ema_update_after = a->ema_update_after;
  hipLaunchKernelGGL(lagrange_step_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p);
  return check_launch("cgen_lagrange_step");
}
