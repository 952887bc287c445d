// Counterfactual evaluation on the device (train_cf.py:63-108 get_metrics, :181-189 the eval branch of cf_epoch;
// train_pgm.py:175-249 eval_epoch): per-variable metric accumulation, exact ROC-AUC, per-image distances.
//   metric_accum_kernel  one workgroup per variable; rows in a fixed thread assignment, f64 partial sums folded in a fixed
//                        order; the AUC rows are compacted in sample order by a block-wide prefix count (no atomics).
//   rocauc_pairs_kernel  Mann-Whitney pair count: a workgroup holds 256 rows in registers (one per thread) and streams tiles
//                        of 256 rows through LDS; a row that must not take part (wrong class, NaN) is replaced by NaN so the
//                        inner loop is two compares and two adds; per-block 64-bit sums go out as INTEGER atomics.
//   image_dist_kernel    one workgroup per image, differences and sums in f64, 16-byte loads on the aligned path.
// Nothing here is MFMA work; every shape is small.  No kernel uses scratch.
#include <math.h>

#include "common.h"

namespace cgen {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// deterministic block sum for blockDim.x == 256; every thread gets the result; `sm` >= 4 doubles
__device__ __forceinline__ double block_sum_256_f64(double v, double* sm) {
  v = wave_sum_f64(v);
  __syncthreads();  // (sm may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }  // false for NaN and +-inf

struct MetricVars {
  cgen_metric_var v[CGEN_METRIC_MAX_VARS];
};

__global__ __launch_bounds__(256) void metric_accum_kernel(MetricVars mv, int n) {
  __shared__ double smd[4];
  __shared__ int wave_cnt[4];
  const cgen_metric_var& v = mv.v[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ncls = v.ncls;
  const bool want_auc = v.scores != nullptr;
  const int64_t base0 = want_auc ? *v.row_count : 0;  // read by every thread before thread 0 rewrites it at the end
  double n_cnt = 0.0, n_ok = 0.0, abs_err = 0.0, n_skip = 0.0, n_over = 0.0;
  int64_t appended = 0;  // valid rows of the chunks done so far (the same in every thread)
  for (int r0 = 0; r0 < n; r0 += 256) {
    const int r = r0 + tid;
    const bool in = r < n;
    const float* p = v.pred + (int64_t)(in ? r : 0) * v.pred_stride;
    const float* t = v.target + (int64_t)(in ? r : 0) * v.target_stride;
    bool valid = in;
    if (in) {
      if (v.kind == CGEN_METRIC_CATEGORICAL) {
        for (int c = 0; c < ncls; ++c) valid = valid && finite_f(p[c]) && finite_f(t[c]);
      } else {
        valid = finite_f(p[0]) && finite_f(t[0]);
      }
      if (!valid) n_skip += 1.0;
    }
    // position of this row among the valid rows of the call, in sample order
    const unsigned long long bal = __ballot(valid);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int wave_off = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wv) wave_off += wave_cnt[w];
      chunk += wave_cnt[w];
    }
    const int64_t slot = base0 + appended + wave_off + before;
    appended += chunk;
    if (!valid) continue;
    n_cnt += 1.0;
    const bool store = want_auc && slot < v.capacity;
    if (want_auc && !store) n_over += 1.0;
    if (v.kind == CGEN_METRIC_BINARY) {
      const float o = p[0];
      const bool lab = t[0] > 0.5f;
      const bool sig = v.transform == CGEN_METRIC_SIGMOID;
      const float score = sig ? 1.0f / (1.0f + expf(-o)) : o;
      const bool hit = sig ? (o > 0.f) : (o > 0.5f);
      if (hit == lab) n_ok += 1.0;
      if (store) {
        v.scores[slot] = score;
        v.labels[slot] = lab ? 1.f : 0.f;
      }
    } else if (v.kind == CGEN_METRIC_CATEGORICAL) {
      int ap = 0, at = 0;
      float mp = p[0], mt = t[0];
      for (int c = 1; c < ncls; ++c) {
        if (p[c] > mp) { mp = p[c]; ap = c; }
        if (t[c] > mt) { mt = t[c]; at = c; }
      }
      if (ap == at) n_ok += 1.0;
      if (store) {
        float* so = v.scores + slot * ncls;
        float* lo = v.labels + slot * ncls;
        if (v.transform == CGEN_METRIC_SOFTMAX) {
          // exp(o - max) / sum in f32, the sum taken pairwise over the row padded with zeros to a power of two -- (e_i + e_{i+8})
          // first, then + 4, + 2, + 1: the order of torch.softmax's row reduction, so that the stored scores are predict()'s to
          // the last bits (an exact sum would sit up to 3 ulp from them: torch's own f32 sum carries that error)
          float e[CGEN_PRED_MAX_OUT];
#pragma unroll
          for (int c = 0; c < CGEN_PRED_MAX_OUT; ++c) e[c] = c < ncls ? expf(p[c] - mp) : 0.f;
          float t8[8], t4[4];
#pragma unroll
          for (int c = 0; c < 8; ++c) t8[c] = e[c] + e[c + 8];
#pragma unroll
          for (int c = 0; c < 4; ++c) t4[c] = t8[c] + t8[c + 4];
          const float s = (t4[0] + t4[2]) + (t4[1] + t4[3]);
#pragma unroll
          for (int c = 0; c < CGEN_PRED_MAX_OUT; ++c)
            if (c < ncls) so[c] = e[c] / s;
        } else {
          for (int c = 0; c < ncls; ++c) so[c] = p[c];
        }
        for (int c = 0; c < ncls; ++c) lo[c] = c == at ? 1.f : 0.f;
      }
    } else {
      const double f = v.transform == CGEN_METRIC_TANH ? tanh((double)p[0]) : (double)p[0];
      const double pv = f * (double)v.pred_scale + (double)v.pred_shift;
      const double tv = (double)t[0] * (double)v.tgt_scale + (double)v.tgt_shift;
      abs_err += fabs(tv - pv) / (double)v.norm;
    }
  }
  const double s_cnt = block_sum_256_f64(n_cnt, smd);
  const double s_ok = block_sum_256_f64(n_ok, smd);
  const double s_err = block_sum_256_f64(abs_err, smd);
  const double s_skip = block_sum_256_f64(n_skip, smd);
  const double s_over = block_sum_256_f64(n_over, smd);
  if (tid == 0) {
    v.acc[CGEN_METRIC_N] += s_cnt;
    v.acc[CGEN_METRIC_CORRECT] += s_ok;
    v.acc[CGEN_METRIC_ABS_ERR] += s_err;
    v.acc[CGEN_METRIC_SKIPPED] += s_skip;
    v.acc[CGEN_METRIC_OVERFLOW] += s_over;
    if (want_auc) {
      const int64_t end = base0 + appended;
      *v.row_count = end < v.capacity ? end : v.capacity;
    }
  }
}

// ----------------------------------------------------------------------------- ROC-AUC
// ws[c * 4 + {0, 1, 2, 3}] = {#(s+ > s-), #(s+ == s-), n+, n-} of column c
__global__ void rocauc_zero_kernel(unsigned long long* ws, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) ws[i] = 0ull;
}

__device__ __forceinline__ unsigned long long block_sum_256_u64(unsigned long long v, unsigned long long* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

#define AUC_TILE 256
__global__ __launch_bounds__(256) void rocauc_pairs_kernel(const float* scores, const float* labels, const int64_t* n_rows_dev,
                                                           int64_t n_rows_max, int64_t stride, unsigned long long* ws) {
  __shared__ __attribute__((aligned(16))) float neg[AUC_TILE];
  __shared__ unsigned long long sm[4];
  int64_t n = *n_rows_dev;
  if (n > n_rows_max) n = n_rows_max;
  const int64_t i0 = (int64_t)blockIdx.x * AUC_TILE;
  if (i0 >= n) return;  // (uniform over the block)
  const int c = blockIdx.z, tid = threadIdx.x;
  const float nanv = __int_as_float(0x7fc00000);
  // this thread's row as a POSITIVE (NaN otherwise: a NaN never compares greater or equal)
  const int64_t i = i0 + tid;
  float si = nanv, li = 0.f;
  if (i < n) {
    si = scores[i * stride + c];
    li = labels[i * stride + c];
  }
  const bool usable = i < n && si == si;
  const bool is_pos = usable && li > 0.5f;
  const float sp = is_pos ? si : nanv;
  uint32_t gt = 0, eq = 0;
  const int64_t ntiles = (n + AUC_TILE - 1) / AUC_TILE;
  for (int64_t jt = blockIdx.y; jt < ntiles; jt += gridDim.y) {
    const int64_t j = jt * AUC_TILE + tid;
    float sj = nanv;
    if (j < n) {
      const float s = scores[j * stride + c];
      sj = labels[j * stride + c] > 0.5f ? nanv : s;  // negatives only
    }
    __syncthreads();
    neg[tid] = sj;
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < AUC_TILE; k += 4) {
      const f32x4_t q = *(const f32x4_t*)&neg[k];  // one broadcast ds_read_b128 for the whole wave
      gt += (uint32_t)(sp > q[0]) + (uint32_t)(sp > q[1]) + (uint32_t)(sp > q[2]) + (uint32_t)(sp > q[3]);
      eq += (uint32_t)(sp == q[0]) + (uint32_t)(sp == q[1]) + (uint32_t)(sp == q[2]) + (uint32_t)(sp == q[3]);
    }
  }
  const unsigned long long bgt = block_sum_256_u64(gt, sm);
  const unsigned long long beq = block_sum_256_u64(eq, sm);
  unsigned long long bpos = 0, bneg = 0;
  if (blockIdx.y == 0) {  // every row tile is counted once
    bpos = block_sum_256_u64(is_pos ? 1ull : 0ull, sm);
    bneg = block_sum_256_u64((usable && !is_pos) ? 1ull : 0ull, sm);
  }
  if (tid == 0) {
    if (bgt) atomicAdd(&ws[c * 4 + 0], bgt);
    if (beq) atomicAdd(&ws[c * 4 + 1], beq);
    if (bpos) atomicAdd(&ws[c * 4 + 2], bpos);
    if (bneg) atomicAdd(&ws[c * 4 + 3], bneg);
  }
}

__global__ void rocauc_finish_kernel(const unsigned long long* ws, int ncls, double* auc) {
  const int c = threadIdx.x;
  if (c >= ncls) return;
  const double gt = (double)ws[c * 4 + 0], eq = (double)ws[c * 4 + 1];
  const double np = (double)ws[c * 4 + 2], nn = (double)ws[c * 4 + 3];
  auc[c] = (np > 0.0 && nn > 0.0) ? (gt + 0.5 * eq) / (np * nn) : __longlong_as_double(0x7ff8000000000000ll);
}

// ----------------------------------------------------------------------------- image distances
template <bool VEC>
__global__ __launch_bounds__(256) void image_dist_kernel(int64_t elems, const float* a, const float* b, float* per_image, double* ws) {
  __shared__ double smd[4];
  const int img = blockIdx.x, tid = threadIdx.x;
  const float* pa = a + (int64_t)img * elems;
  const float* pb = b + (int64_t)img * elems;
  double l1 = 0.0, l2 = 0.0;
  if (VEC) {  // elems % 4 == 0 and both bases 16-byte aligned (checked on the host)
    const int64_t nv = elems >> 2;
    const f32x4_t* va = (const f32x4_t*)pa;
    const f32x4_t* vb = (const f32x4_t*)pb;
#pragma unroll 2
    for (int64_t i = tid; i < nv; i += 256) {
      const f32x4_t x = va[i], y = vb[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double d = (double)x[k] - (double)y[k];
        l1 += fabs(d);
        l2 += d * d;
      }
    }
  } else {
    for (int64_t i = tid; i < elems; i += 256) {
      const double d = (double)pa[i] - (double)pb[i];
      l1 += fabs(d);
      l2 += d * d;
    }
  }
  const double s1 = block_sum_256_f64(l1, smd);
  const double s2 = block_sum_256_f64(l2, smd);
  if (tid == 0) {
    const double m1 = s1 / (double)elems, m2 = s2 / (double)elems;
    ws[2 * img] = m1;
    ws[2 * img + 1] = m2;
    if (per_image) {
      per_image[2 * img] = (float)m1;
      per_image[2 * img + 1] = (float)m2;
    }
  }
}

__global__ __launch_bounds__(256) void image_dist_fold_kernel(int n, const double* ws, double* acc) {
  __shared__ double smd[4];
  double l1 = 0.0, l2 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    l1 += ws[2 * i];
    l2 += ws[2 * i + 1];
  }
  const double s1 = block_sum_256_f64(l1, smd);
  const double s2 = block_sum_256_f64(l2, smd);
  if (threadIdx.x == 0) {
    acc[0] += s1;
    acc[1] += s2;
    acc[2] += (double)n;
  }
}

}  // namespace cgen

using namespace cgen;

extern "C" int cgen_metric_accum(const cgen_metric_var* vars, int32_t nvars, int32_t n, cgen_stream_t stream) {
  CGEN_REQUIRE(vars, "cgen_metric_accum: null vars (the record array)");
  CGEN_REQUIRE(nvars >= 1 && nvars <= CGEN_METRIC_MAX_VARS, "cgen_metric_accum: nvars %d outside 1..%d", nvars, CGEN_METRIC_MAX_VARS);
  CGEN_REQUIRE(n >= 0, "cgen_metric_accum: n %d is negative", n);
  MetricVars mv;
  memset(&mv, 0, sizeof(mv));
  for (int i = 0; i < nvars; ++i) {
    const cgen_metric_var& v = vars[i];
    CGEN_REQUIRE(v.kind == CGEN_METRIC_BINARY || v.kind == CGEN_METRIC_CATEGORICAL || v.kind == CGEN_METRIC_CONTINUOUS,
                 "cgen_metric_accum: variable %d: unknown kind %d", i, v.kind);
    CGEN_REQUIRE(v.ncls >= 1 && v.ncls <= CGEN_PRED_MAX_OUT, "cgen_metric_accum: variable %d: ncls %d outside 1..%d", i, v.ncls,
                 CGEN_PRED_MAX_OUT);
    CGEN_REQUIRE(v.transform >= CGEN_METRIC_NONE && v.transform <= CGEN_METRIC_TANH, "cgen_metric_accum: variable %d: unknown transform %d",
                 i, v.transform);
    const bool fits = v.transform == CGEN_METRIC_NONE || (v.kind == CGEN_METRIC_BINARY && v.transform == CGEN_METRIC_SIGMOID) ||
                      (v.kind == CGEN_METRIC_CATEGORICAL && v.transform == CGEN_METRIC_SOFTMAX) ||
                      (v.kind == CGEN_METRIC_CONTINUOUS && v.transform == CGEN_METRIC_TANH);
    CGEN_REQUIRE(fits, "cgen_metric_accum: variable %d: transform %d does not fit kind %d", i, v.transform, v.kind);
    CGEN_REQUIRE(v.kind == CGEN_METRIC_CATEGORICAL ? v.ncls >= 2 : v.ncls == 1, "cgen_metric_accum: variable %d: ncls %d does not fit kind %d",
                 i, v.ncls, v.kind);
    CGEN_REQUIRE(v.pred && v.target && v.acc, "cgen_metric_accum: variable %d: null pred, target or acc pointer", i);
    CGEN_REQUIRE(v.pred_stride >= v.ncls, "cgen_metric_accum: variable %d: pred_stride %lld < ncls %d", i, (long long)v.pred_stride, v.ncls);
    CGEN_REQUIRE(v.target_stride >= (v.kind == CGEN_METRIC_CATEGORICAL ? v.ncls : 1), "cgen_metric_accum: variable %d: target_stride %lld too small",
                 i, (long long)v.target_stride);
    if (v.kind == CGEN_METRIC_CONTINUOUS) {
      CGEN_REQUIRE(v.norm > 0.f, "cgen_metric_accum: variable %d: norm must be > 0", i);
      CGEN_REQUIRE(!v.scores && !v.labels && !v.row_count, "cgen_metric_accum: variable %d: a continuous variable has no AUC buffers", i);
    } else if (v.scores || v.labels || v.row_count) {
      CGEN_REQUIRE(v.scores && v.labels && v.row_count && v.capacity >= 0,
                   "cgen_metric_accum: variable %d: scores, labels and row_count must be given together, capacity >= 0", i);
    }
    mv.v[i] = v;
  }
  if (n == 0) return CGEN_OK;
  hipLaunchKernelGGL(metric_accum_kernel, dim3(nvars), dim3(256), 0, (hipStream_t)stream, mv, (int)n);
  return check_launch("cgen_metric_accum");
}

extern "C" int cgen_rocauc(const float* scores, const float* labels, const int64_t* n_rows_dev, int64_t n_rows_max, int32_t ncls,
                           int64_t stride, double* auc_out, uint64_t* ws, cgen_stream_t stream) {
  CGEN_REQUIRE(scores && labels && n_rows_dev && auc_out && ws, "cgen_rocauc: null scores, labels, n_rows_dev, auc_out or ws");
  CGEN_REQUIRE(ncls >= 1 && ncls <= CGEN_PRED_MAX_OUT, "cgen_rocauc: ncls %d outside 1..%d", ncls, CGEN_PRED_MAX_OUT);
  CGEN_REQUIRE(stride >= ncls, "cgen_rocauc: stride %lld < ncls %d", (long long)stride, ncls);
  CGEN_REQUIRE(n_rows_max >= 0 && n_rows_max < (1ll << 31), "cgen_rocauc: n_rows_max %lld outside 0..2^31-1", (long long)n_rows_max);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* w = (unsigned long long*)ws;
  hipLaunchKernelGGL(rocauc_zero_kernel, dim3(1), dim3(64), 0, st, w, 4 * ncls);
  const int64_t tiles = (n_rows_max + AUC_TILE - 1) / AUC_TILE;
  if (tiles > 0) {
    // rows x a split of the streamed tiles: enough workgroups to fill the chip at 65536 rows, at most 2^26 compares per counter
    const int64_t split = tiles < 32 ? tiles : 32;
    hipLaunchKernelGGL(rocauc_pairs_kernel, dim3((unsigned)tiles, (unsigned)split, (unsigned)ncls), dim3(256), 0, st, scores, labels,
                       n_rows_dev, n_rows_max, stride, w);
  }
  hipLaunchKernelGGL(rocauc_finish_kernel, dim3(1), dim3(64), 0, st, w, (int)ncls, auc_out);
  return check_launch("cgen_rocauc");
}

extern "C" int cgen_image_dist(int32_t n, int64_t elems_per_image, const float* a, const float* b, float* per_image, double* ws,
                               double* acc, cgen_stream_t stream) {
  CGEN_REQUIRE(a && b && ws, "cgen_image_dist: null a, b or ws");
  CGEN_REQUIRE(n >= 0 && elems_per_image >= 1, "cgen_image_dist: n %d or elems_per_image %lld out of range", n, (long long)elems_per_image);
  if (n == 0) return CGEN_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (elems_per_image % 4 == 0) && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0);
  if (vec)
    hipLaunchKernelGGL(image_dist_kernel<true>, dim3(n), dim3(256), 0, st, elems_per_image, a, b, per_image, ws);
  else
    hipLaunchKernelGGL(image_dist_kernel<false>, dim3(n), dim3(256), 0, st, elems_per_image, a, b, per_image, ws);
  if (acc) hipLaunchKernelGGL(image_dist_fold_kernel, dim3(1), dim3(256), 0, st, (int)n, ws, acc);
  return check_launch("cgen_image_dist");
}
