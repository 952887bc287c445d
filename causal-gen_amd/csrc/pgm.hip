// Parent SCM: log-likelihood of the parents and its parameter gradients (cgen_pgm_nll_fwd / cgen_pgm_nll_fwd_bwd; the reference's
// train_pgm.py sup_epoch with --setup sup_pgm, i.e. -log p(parents) of flow_pgm.py's svi_model).  A few thousand parameters and a
// few hundred rows: launch- and latency-bound, so the whole SCM is two launches.
//
// Launch 1, one workgroup of 256 threads per (64 rows, mechanism): thread (r, q) = (tid & 63, tid >> 6) works on row r.  The root
// and spline mechanisms are one thread per row (wave 0); an MLP layer is split over the four waves, wave q computing outputs
// o = q, q + 4, ... of every row with the layer's weights in LDS.  Per-row arrays live in LDS as [feature][row] with a row stride
// of 65 floats: a wave reading one feature of its 64 rows and 64 threads reading 64 features of one row both touch 32 distinct
// banks.  The backward keeps the pre-activations z_l of every hidden layer, overwrites them in place with d term / d z_l, and
// forms each weight gradient as a sum over the workgroup's rows in row order, one thread per weight.  The spline's knots,
// derivatives and lambdas are derived once per workgroup; a row's gradient with respect to the seven quantities of its bin comes
// from forward-mode dual numbers through the closed-form inverse and log-derivative.  Each workgroup writes its partial sums to
// its own row of the workspace.
// Launch 2 adds those rows in index order, applies the batch-independent chain of the root and spline parameters (softmax /
// softplus / sigmoid / cumsum) and the coefficient, and writes the gradients; one more workgroup sums the terms.
// No atomics, fixed summation orders: reruns are bit-identical.  Every store is plain C++.
// Precision: every buffer, parameter, activation, term and gradient is f32, and so are erff / expf of the activations.  Sums --
// the dot products of a layer, the sums over rows and over workgroups, the softmax normalisers -- and the spline algebra
// accumulate in f64 registers and are rounded to f32 once.  The check this kernel is held to is four times the deviation of
// torch's own f32 CPU run from the f64 density; torch's blocked sums sit at about one f32 rounding of a gradient tensor's largest
// entry, and plain f32 accumulation in row order measured three to eight roundings here (5e-7 against bounds of 2.4e-7..4e-7).
// (The pieces the counterfactual launch of csrc/pgm_cf.hip needs as well -- geometry, activation, normalisation, knots, the MLP
// layer, the record validation -- live in pgm_common.h.)
#include "pgm_common.h"

namespace cgen {

struct PgmP {
  cgen_pgm_mech m[CGEN_PGM_MAX_MECH];
  const float* obs;
  const int64_t* index;
  float* terms;
  float* ws;
  int64_t table_rows;
  int n, ncol, rows, S, W, NH;  // S: floats per workspace row; W / NH: largest hidden width / layer count of any MLP (0 without one)
  int soff[CGEN_PGM_MAX_MECH];  // first slot of a mechanism in a workspace row
};

__host__ __device__ inline int pgm_slots(const cgen_pgm_mech& m) {
  if (m.kind == CGEN_PGM_BERNOULLI) return 1;
  if (m.kind == CGEN_PGM_CATEGORICAL) return m.ncls;
  if (m.kind == CGEN_PGM_SPLINE) return 4 * m.bins + 3;
  int s = 0;
  for (int l = 0; l <= m.nhidden; ++l) s += pgm_out(m, l) * pgm_in(m, l) + pgm_out(m, l);
  return s;
}
static inline int pgm_lds_floats(int W, int NH) {
  const int WM = W > 16 ? W : 16;
  return 128 + (NH + 1) * W * PGM_RS + (W ? WM * WM + WM : 0) + 18 * PGM_RS;
}

// ----------------------------------------------------------------------------- scalar pieces (the forward's are in pgm_common.h)
__device__ __noinline__ float pgm_dact(int act, float z) {
  if (act == CGEN_PGM_GELU) return 0.5f * (1.f + erff(z * CGEN_SQRT1_2)) + z * CGEN_INV_SQRT_2PI * expf(-0.5f * z * z);
  if (act == CGEN_PGM_SIGMOID) {
    const float s = pgm_sigmoid(z);
    return s * (1.f - s);
  }
  return z > 0.f ? 1.f : 0.1f;
}

// forward-mode dual number over the seven quantities of a spline bin: x0, x1, y0, y1, d0, d1, lambda.
// The spline algebra alone runs in f64 registers (its inputs and results are f32 like everything else): in f32 the gradient with
// respect to lambda and the widths cancels by two to three digits (measured on a single row: 2.3e-5 relative, six times the
// deviation of torch's own f32 autograd), and with f64 knots a row is binned as the f64 host density bins it.
struct D7 {
  double v, d[7];
};
__device__ __forceinline__ D7 d7_const(double c) {
  D7 r;
  r.v = c;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = 0.0;
  return r;
}
__device__ __forceinline__ D7 d7_var(double c, int which) {
  D7 r = d7_const(c);
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (k == which) r.d[k] = 1.0;
  return r;
}
__device__ __forceinline__ D7 operator+(const D7& a, const D7& b) {
  D7 r;
  r.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
__device__ __forceinline__ D7 operator-(const D7& a, const D7& b) {
  D7 r;
  r.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
__device__ __forceinline__ D7 operator*(const D7& a, const D7& b) {
  D7 r;
  r.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
__device__ __forceinline__ D7 operator/(const D7& a, const D7& b) {
  D7 r;
  const double ib = 1.0 / b.v;
  r.v = a.v * ib;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * ib;
  return r;
}
__device__ __forceinline__ D7 operator-(const D7& a, double c) { D7 r = a; r.v -= c; return r; }
__device__ __forceinline__ D7 operator-(double c, const D7& a) { return d7_const(c) - a; }
__device__ __forceinline__ D7 d7_sqrt(const D7& a) {
  D7 r;
  r.v = sqrt(a.v);
  const double h = 0.5 / r.v;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = a.d[k] * h;
  return r;
}
__device__ __forceinline__ D7 d7_log(const D7& a) {
  D7 r;
  r.v = log(a.v);
  const double ia = 1.0 / a.v;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.d[k] = a.d[k] * ia;
  return r;
}

// s + c <- s + c + x with the rounding error of the addition kept in c (Knuth's TwoSum: additions only, still f32)
__device__ __forceinline__ void pgm_two_sum(float& s, float& c, float x) {
  const float t = s + x, bp = t - s;
  c += (s - (t - bp)) + (x - bp);
  s = t;
}
// the sum of `count` floats by one workgroup of 256: strided compensated partial sums, a butterfly over each wave, the four waves
// in order.  The loss is a sum of rows * mechanisms terms of either sign; the compensation keeps it at the terms' own accuracy.
__device__ __forceinline__ void pgm_sum_terms(const float* terms, int64_t count, float* out, float* sm8) {
  float s = 0.f, c = 0.f;
  for (int64_t i = threadIdx.x; i < count; i += PGM_T) pgm_two_sum(s, c, terms[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(s, o, 64), oc = __shfl_xor(c, o, 64);
    pgm_two_sum(s, c, os);
    c += oc;
  }
  if ((threadIdx.x & 63) == 0) {
    sm8[2 * (threadIdx.x >> 6)] = s;
    sm8[2 * (threadIdx.x >> 6) + 1] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = sm8[0];
    c = sm8[1];
    for (int w = 1; w < 4; ++w) {
      pgm_two_sum(s, c, sm8[2 * w]);
      c += sm8[2 * w + 1];
    }
    out[0] = s + c;
  }
}

// ----------------------------------------------------------------------------- launch 1: rows
// (one kernel for both entry points, the backward behind a uniform flag: two instantiations would be free to contract the
// forward's arithmetic differently, and loss() must give the bits of step()'s loss)
__global__ __launch_bounds__(PGM_T) void pgm_rows_kernel(const PgmP a) {
  extern __shared__ float sm[];
  const bool BWD = a.ws != nullptr;
  const int mi = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, r = tid & 63, q = tid >> 6;
  const cgen_pgm_mech& M = a.m[mi];
  const int W = a.W, NH = a.NH, WM = W > 16 ? W : 16;
  double* const Misc = (double*)sm;                    // [64] the spline's derived quantities (first: 8-byte aligned)
  float* const Zb = sm + 128;                          // [NH][W][RS] pre-activations, then their gradients
  float* const Ht = Zb + NH * W * PGM_RS;              // [W][RS] activations of the layer whose weight gradient is being formed
  float* const Wb = Ht + W * PGM_RS;                   // one layer's weights and bias
  float* const Dout = Wb + (W ? WM * WM + WM : 0);     // [16][RS] MLP outputs, then their gradients; the spline's per-row partials
  float* const Ctx = Dout + 16 * PGM_RS;               // [2][RS]
  const int row = blk * PGM_R + r;
  const bool valid = row < a.rows;
  const int64_t src = valid ? (a.index ? a.index[row] : (int64_t)row) : 0;
  const bool inrange = src >= 0 && src < a.table_rows;
  const float* orow = a.obs + (inrange ? src : 0) * a.ncol;
  const float poison = inrange ? 0.f : NAN;  // a row the index sends outside the table scores NaN
  auto ld = [&](int c) { return valid ? orow[c] + poison : 0.f; };
  float* const wsrow = BWD ? a.ws + (int64_t)blk * a.S + a.soff[mi] : nullptr;
  float* const term_out = a.terms + (int64_t)row * a.n + mi;
  const int kind = M.kind;

  if (kind == CGEN_PGM_BERNOULLI) {
    if (q != 0) return;
    const float l = M.p[0][0], x = ld(M.col);
    if (valid) *term_out = (float)((double)x * (double)l - (fmax((double)l, 0.0) + log1p(exp(-fabs((double)l)))));
    if (BWD) {
      const float s = wave_sum(valid ? x : 0.f);
      if (r == 0) wsrow[0] = s;
    }
    return;
  }
  if (kind == CGEN_PGM_CATEGORICAL) {
    if (q != 0) return;
    const int nc = M.ncls;
    const float* lg = M.p[0];
    float mx = lg[0];
    for (int j = 1; j < nc; ++j) mx = fmaxf(mx, lg[j]);
    double se = 0.0;
    for (int j = 0; j < nc; ++j) se += exp((double)lg[j] - (double)mx);
    const double lse = (double)mx + log(se);
    double term = 0.0;
    for (int j = 0; j < nc; ++j) {
      const float x = ld(M.col + j);
      term += (double)x * ((double)lg[j] - lse);
      if (BWD) {
        const float s = wave_sum(valid ? x : 0.f);
        if (r == 0) wsrow[j] = s;
      }
    }
    if (valid) *term_out = (float)term;
    return;
  }
  if (kind == CGEN_PGM_SPLINE) {
    const int K = M.bins;
    const float Bd = M.bound;
    double *xk = Misc, *yk = Misc + 9, *dk = Misc + 18, *lam = Misc + 27;
    pgm_spline_tables(M, Misc, tid);
    __syncthreads();
    if (q == 0) {
      const float x = ld(M.col);
      double extra = 0.0, u = x;
      if (M.normalize) u = pgm_normalize_inv(x, extra);
      const bool inside = u > -(double)Bd && u < (double)Bd;
      float term = (float)(-0.5 * u * u - 0.91893853320467274178 + extra);  // outside the bound the spline is the identity
      D7 t = d7_const(0.0);
      int idx = -1;
      if (inside) {
        idx = 0;
        for (int j = 1; j < K; ++j) idx += (u >= yk[j]) ? 1 : 0;
        const D7 X0 = d7_var(xk[idx], 0), X1 = d7_var(xk[idx + 1], 1), Y0 = d7_var(yk[idx], 2), Y1 = d7_var(yk[idx + 1], 3);
        const D7 D0 = d7_var(dk[idx], 4), D1 = d7_var(dk[idx + 1], 5), LM = d7_var(lam[idx], 6);
        const D7 dx = X1 - X0;
        const D7 wb = d7_sqrt(D0 / D1);  // w_a = 1
        const D7 s = (Y1 - Y0) / dx;
        const D7 oml = 1.0 - LM;
        const D7 wc = (LM * D0 + oml * wb * D1) / s;
        const D7 yc = (oml * Y0 + LM * wb * Y1) / (oml + LM * wb);
        D7 th, dydth;
        if (u <= yc.v) {  // the piece left of the interior point
          const D7 a0 = Y0 - u, a1 = (d7_const(u) - yc) * wc;
          th = LM * a0 / (a0 + a1);
          const D7 den = (LM - th) + wc * th;
          dydth = wc * LM * (yc - Y0) / (den * den);
        } else {
          const D7 b0 = wc * (yc - u), b1 = wb * (d7_const(u) - Y1);
          th = (b0 + LM * b1) / (b0 + b1);
          const D7 den = wc * (1.0 - th) + wb * (th - LM);
          dydth = wb * wc * oml * (Y1 - yc) / (den * den);
        }
        const D7 eps = th * dx + X0;
        t = d7_const(-0.5) * eps * eps - d7_log(dydth / dx);
        term = (float)(t.v - 0.91893853320467274178 + extra);
      }
      if (valid) *term_out = term;
      if (BWD) {
        const bool use = valid && inside;
#pragma unroll
        for (int k = 0; k < 7; ++k) Dout[k * PGM_RS + r] = use ? (float)t.d[k] : 0.f;
        Dout[7 * PGM_RS + r] = use ? (float)idx : -1.f;
      }
    }
    if (!BWD) return;
    __syncthreads();
    // slots: x knots [K + 1], y knots [K + 1], derivatives [K + 1], lambdas [K]; a row adds to those of its bin, in row order
    if (tid < 4 * K + 3) {
      const int arr = tid < 3 * (K + 1) ? tid / (K + 1) : 3;
      const int k = tid - arr * (K + 1);
      double s = 0.0;
      for (int rr = 0; rr < PGM_R; ++rr) {
        const int id = (int)Dout[7 * PGM_RS + rr];
        if (id < 0) continue;
        if (k == id) s += Dout[(arr < 3 ? 2 * arr : 6) * PGM_RS + rr];
        if (arr < 3 && k == id + 1) s += Dout[(2 * arr + 1) * PGM_RS + rr];
      }
      wsrow[tid] = (float)s;
    }
    return;
  }

  // ---- AFFINE / GUMBEL_MAX: an MLP of the context
  const int L = M.nhidden, act = M.act, nout = pgm_out(M, L);
  if (q == 0)
    for (int c = 0; c < M.nctx; ++c) Ctx[c * PGM_RS + r] = ld(M.ctx_col[c]);
  for (int l = 0; l <= L; ++l) {
    pgm_layer_stage(M, l, Wb, tid);
    __syncthreads();
    pgm_layer_rows(M, l, Wb, l == 0 ? Ctx : Zb + (l - 1) * W * PGM_RS, l < L ? Zb + l * W * PGM_RS : Dout, r, q);
    __syncthreads();
  }
  if (q == 0) {
    float term;
    if (kind == CGEN_PGM_AFFINE) {
      const double loc = Dout[r], ls = Dout[PGM_RS + r];
      const float x = ld(M.col);
      double extra = 0.0, u = x;
      if (M.normalize) u = pgm_normalize_inv(x, extra);
      const double is = exp(-ls), eps = (u - loc) * is;
      term = (float)(-0.5 * eps * eps - 0.91893853320467274178 - ls + extra);
      if (BWD) {
        Dout[r] = valid ? (float)(eps * is) : 0.f;
        Dout[PGM_RS + r] = valid ? (float)(eps * eps - 1.0) : 0.f;
      }
    } else {
      const float f = ld(M.col);
      const int cls = (f >= 0.f && f < (float)nout) ? (int)f : -1;  // (a NaN or foreign class scores NaN)
      float mx = Dout[r];
      for (int j = 1; j < nout; ++j) mx = fmaxf(mx, Dout[j * PGM_RS + r]);
      double se = 0.0;
      for (int j = 0; j < nout; ++j) se += exp((double)Dout[j * PGM_RS + r] - (double)mx);
      const double lse = (double)mx + log(se);
      term = NAN;
      for (int j = 0; j < nout; ++j) {
        const double lg = Dout[j * PGM_RS + r];
        if (j == cls) term = (float)(lg - lse);
        if (BWD) Dout[j * PGM_RS + r] = !valid ? 0.f : cls < 0 ? NAN : (float)((j == cls ? 1.0 : 0.0) - exp(lg - lse));
      }
    }
    if (valid) *term_out = term;
  }
  if (!BWD) return;
  const float* D = Dout;  // d term / d (output of layer l), [wo][RS]
  for (int l = L; l >= 0; --l) {
    const int wi = pgm_in(M, l), wo = pgm_out(M, l);
    float* Zin = l > 0 ? Zb + (l - 1) * W * PGM_RS : nullptr;
    if (l > 0) {
      for (int i = q; i < wi; i += 4) Ht[i * PGM_RS + r] = pgm_act(act, Zin[i * PGM_RS + r]);
      for (int j = tid; j < wo * wi; j += PGM_T) Wb[j] = M.p[2 * l][j];
    }
    __syncthreads();
    const float* A = l > 0 ? Ht : Ctx;
    float* g = wsrow;
    for (int k = 0; k < l; ++k) g += pgm_out(M, k) * pgm_in(M, k) + pgm_out(M, k);
    for (int j = tid; j < wo * wi; j += PGM_T) {  // one thread per weight, its rows in order
      const int o = j / wi, i = j - o * wi;
      double s = 0.0;
      for (int rr = 0; rr < PGM_R; ++rr) s += (double)D[o * PGM_RS + rr] * (double)A[i * PGM_RS + rr];
      g[j] = (float)s;
    }
    for (int o = tid; o < wo; o += PGM_T) {
      double s = 0.0;
      for (int rr = 0; rr < PGM_R; ++rr) s += (double)D[o * PGM_RS + rr];
      g[wo * wi + o] = (float)s;
    }
    if (l > 0) {
      // d term / d z_{l-1}, in place over z_{l-1}: nobody else reads or writes element (i, r)
      for (int i = q; i < wi; i += 4) {
        double s = 0.0;
        for (int o = 0; o < wo; ++o) s += (double)Wb[o * wi + i] * (double)D[o * PGM_RS + r];
        Zin[i * PGM_RS + r] = (float)(s * (double)pgm_dact(act, Zin[i * PGM_RS + r]));
      }
    }
    __syncthreads();
    D = Zin;
  }
}

// ----------------------------------------------------------------------------- launch 2: add the workgroups' rows, chain, scale
__device__ __forceinline__ double pgm_sum_rows(const float* ws, int nblk, int S, int j) {
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += (double)ws[(int64_t)b * S + j];
  return s;
}

// gradient of softmax-made bin sizes: knot gradients G[0..K] -> unnormalized parameters
__device__ void pgm_knots_bwd(const float* u, const double* G, int K, double bound, double coef, float* out) {
  double mx = u[0];
  for (int j = 1; j < K; ++j) mx = fmax(mx, (double)u[j]);
  double se = 0.0;
  for (int j = 0; j < K; ++j) se += exp((double)u[j] - mx);
  // size m moves the interior knots m + 1 .. K - 1
  double dot = 0.0;
  for (int m = 0; m < K; ++m) {
    double gw = 0.0;
    for (int j = m + 1; j < K; ++j) gw += G[j];
    dot += gw * 2.0 * bound * (exp((double)u[m] - mx) / se);
  }
  for (int m = 0; m < K; ++m) {
    double gw = 0.0;
    for (int j = m + 1; j < K; ++j) gw += G[j];
    const double sft = exp((double)u[m] - mx) / se;
    out[m] = (float)(coef * ((1.0 - (double)PGM_MIN_BIN * K) * sft * (gw * 2.0 * bound - dot)));
  }
}

__global__ __launch_bounds__(PGM_T) void pgm_finish_kernel(const PgmP a, const float* coef_dev, float* loss_sum, int nblk) {
  __shared__ double sm[36];
  __shared__ float sm8[8];
  const int mi = blockIdx.x, tid = threadIdx.x;
  if (mi == a.n) {
    if (blockIdx.y == 0) pgm_sum_terms(a.terms, (int64_t)a.rows * a.n, loss_sum, sm8);
    return;
  }
  const cgen_pgm_mech& M = a.m[mi];
  const double coef = coef_dev[0];
  const float* ws = a.ws + a.soff[mi];
  if (pgm_is_mlp(M.kind)) {
    const int slots = pgm_slots(M);
    for (int j = blockIdx.y * PGM_T + tid; j < slots; j += gridDim.y * PGM_T) {
      const float v = (float)(coef * pgm_sum_rows(ws, nblk, a.S, j));
      int l = 0, base = 0, wi, wo;
      for (;; ++l) {
        wi = pgm_in(M, l);
        wo = pgm_out(M, l);
        if (j < base + wo * wi + wo) break;
        base += wo * wi + wo;
      }
      const int k = j - base;
      if (k < wo * wi) M.g[2 * l][k] = v;
      else M.g[2 * l + 1][k - wo * wi] = v;
    }
    return;
  }
  if (blockIdx.y != 0) return;
  const int slots = pgm_slots(M);
  if (tid < slots) sm[tid] = pgm_sum_rows(ws, nblk, a.S, tid);
  __syncthreads();
  if (tid != 0) return;
  if (M.kind == CGEN_PGM_BERNOULLI) {
    M.g[0][0] = (float)(coef * (sm[0] - (double)a.rows / (1.0 + exp(-(double)M.p[0][0]))));
  } else if (M.kind == CGEN_PGM_CATEGORICAL) {
    const int nc = M.ncls;
    const float* lg = M.p[0];
    double mx = lg[0], tot = 0.0, se = 0.0;
    for (int j = 1; j < nc; ++j) mx = fmax(mx, (double)lg[j]);
    for (int j = 0; j < nc; ++j) {
      se += exp((double)lg[j] - mx);
      tot += sm[j];
    }
    for (int j = 0; j < nc; ++j) M.g[0][j] = (float)(coef * (sm[j] - tot * (exp((double)lg[j] - mx) / se)));
  } else {  // SPLINE
    const int K = M.bins;
    pgm_knots_bwd(M.p[0], sm, K, M.bound, coef, M.g[0]);
    pgm_knots_bwd(M.p[1], sm + (K + 1), K, M.bound, coef, M.g[1]);
    for (int j = 1; j < K; ++j) M.g[2][j - 1] = (float)(coef * (sm[2 * (K + 1) + j] / (1.0 + exp(-(double)M.p[2][j - 1]))));
    for (int j = 0; j < K; ++j) {
      const double sg = 1.0 / (1.0 + exp(-(double)M.p[3][j]));
      M.g[3][j] = (float)(coef * (sm[3 * (K + 1) + j] * (1.0 - 2.0 * (double)PGM_MIN_LAMBDA) * sg * (1.0 - sg)));
    }
  }
}

__global__ __launch_bounds__(PGM_T) void pgm_loss_kernel(const float* terms, int64_t count, float* loss_sum) {
  __shared__ float sm[8];
  pgm_sum_terms(terms, count, loss_sum, sm);
}

// ----------------------------------------------------------------------------- host
static void pgm_fill(PgmP& a, const cgen_pgm_mech* mechs, int n, const float* obs, int ncol, int64_t table_rows, const int64_t* index, int rows,
                     float* terms, float* ws) {
  memset(&a, 0, sizeof(a));
  int S = 0;
  for (int i = 0; i < n; ++i) {
    a.m[i] = mechs[i];
    a.soff[i] = S;
    S += pgm_slots(mechs[i]);
    if (pgm_is_mlp(mechs[i].kind)) {
      if (mechs[i].nhidden > a.NH) a.NH = mechs[i].nhidden;
      for (int l = 0; l < mechs[i].nhidden; ++l)
        if (mechs[i].width[l] > a.W) a.W = mechs[i].width[l];
    }
  }
  a.S = S;
  a.obs = obs; a.index = index; a.terms = terms; a.ws = ws; a.table_rows = table_rows;
  a.n = n; a.ncol = ncol; a.rows = rows;
}

static int pgm_check_batch(const char* who, const float* obs, int ncol, int64_t table_rows, const int64_t* index, int rows, const float* terms,
                           const float* loss_sum) {
  CGEN_REQUIRE(obs, "%s: null obs", who);
  CGEN_REQUIRE(ncol >= 1, "%s: ncol = %d", who, ncol);
  CGEN_REQUIRE(rows >= 1 && rows <= (1 << 24), "%s: rows = %d, 1..2^24 are served", who, rows);
  CGEN_REQUIRE(table_rows >= 1 && (index || table_rows >= rows), "%s: table_rows = %lld does not cover %d rows", who, (long long)table_rows, rows);
  CGEN_REQUIRE(terms, "%s: null terms", who);
  CGEN_REQUIRE(loss_sum, "%s: null loss_sum", who);
  return CGEN_OK;
}

static int pgm_launch_rows(const char* who, const PgmP& a, hipStream_t stream) {
  const size_t lds = (size_t)pgm_lds_floats(a.W, a.NH) * sizeof(float);
  static bool once = false;
  if (!once) {
    const hipError_t e = hipFuncSetAttribute((const void*)pgm_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return fail(CGEN_ELAUNCH, "%s: cannot raise the LDS limit: %s", who, hipGetErrorString(e));
    once = true;
  }
  hipLaunchKernelGGL(pgm_rows_kernel, dim3(ceil_div(a.rows, PGM_R), a.n), dim3(PGM_T), lds, stream, a);
  return check_launch(who);
}

}  // namespace cgen

using namespace cgen;

extern "C" int cgen_pgm_workspace(const cgen_pgm_mech* mechs, int32_t n, int32_t rows, int64_t* bytes) {
  if (int rc = pgm_check("cgen_pgm_workspace", mechs, n, -1, false)) return rc;
  CGEN_REQUIRE(rows >= 1 && rows <= (1 << 24), "cgen_pgm_workspace: rows = %d, 1..2^24 are served", rows);
  CGEN_REQUIRE(bytes, "cgen_pgm_workspace: null output");
  int64_t S = 0;
  for (int i = 0; i < n; ++i) S += pgm_slots(mechs[i]);
  *bytes = (int64_t)ceil_div(rows, PGM_R) * S * (int64_t)sizeof(float);
  return CGEN_OK;
}

extern "C" int cgen_pgm_nll_fwd(const cgen_pgm_mech* mechs, int32_t n, const float* obs, int32_t ncol, int64_t table_rows, const int64_t* index,
                                int32_t rows, float* terms, float* loss_sum, cgen_stream_t stream) {
  const char* who = "cgen_pgm_nll_fwd";
  if (int rc = pgm_check_batch(who, obs, ncol, table_rows, index, rows, terms, loss_sum)) return rc;
  if (int rc = pgm_check(who, mechs, n, ncol, false)) return rc;
  PgmP a;
  pgm_fill(a, mechs, n, obs, ncol, table_rows, index, rows, terms, nullptr);
  if (int rc = pgm_launch_rows(who, a, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(pgm_loss_kernel, dim3(1), dim3(PGM_T), 0, (hipStream_t)stream, (const float*)terms, (int64_t)rows * n, loss_sum);
  return check_launch(who);
}

extern "C" int cgen_pgm_nll_fwd_bwd(const cgen_pgm_mech* mechs, int32_t n, const float* obs, int32_t ncol, int64_t table_rows,
                                    const int64_t* index, int32_t rows, float* terms, float* loss_sum, const float* coef_dev, float* workspace,
                                    int64_t workspace_bytes, cgen_stream_t stream) {
  const char* who = "cgen_pgm_nll_fwd_bwd";
  if (int rc = pgm_check_batch(who, obs, ncol, table_rows, index, rows, terms, loss_sum)) return rc;
  if (int rc = pgm_check(who, mechs, n, ncol, true)) return rc;
  CGEN_REQUIRE(coef_dev, "%s: null coef_dev", who);
  CGEN_REQUIRE(workspace, "%s: null workspace", who);
  PgmP a;
  pgm_fill(a, mechs, n, obs, ncol, table_rows, index, rows, terms, workspace);
  const int nblk = ceil_div(rows, PGM_R);
  CGEN_REQUIRE(workspace_bytes >= (int64_t)nblk * a.S * (int64_t)sizeof(float), "%s: workspace too small (%lld bytes, %lld needed)", who,
               (long long)workspace_bytes, (long long)((int64_t)nblk * a.S * (int64_t)sizeof(float)));
  if (int rc = pgm_launch_rows(who, a, (hipStream_t)stream)) return rc;
  int most = 1;
  for (int i = 0; i < n; ++i)
    if (pgm_is_mlp(mechs[i].kind) && pgm_slots(mechs[i]) > most) most = pgm_slots(mechs[i]);
  const int chunks = ceil_div(most, PGM_T) < 32 ? ceil_div(most, PGM_T) : 32;
  hipLaunchKernelGGL(pgm_finish_kernel, dim3(n + 1, chunks), dim3(PGM_T), 0, (hipStream_t)stream, a, coef_dev, loss_sum, nblk);
  return check_launch(who);
}
