// Parent SCM: what csrc/pgm.hip (log-likelihood and gradients) and csrc/pgm_cf.hip (counterfactual parents) share -- the
// workgroup geometry, the scalar pieces (activation, the [-1, 1] normalisation, the spline's knots and per-bin tables), one
// MLP layer over the rows of a workgroup, and the validation of the mechanism records.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"

namespace cgen {

constexpr int PGM_R = CGEN_PGM_ROWS;  // rows per workgroup
constexpr int PGM_RS = PGM_R + 1;     // row stride of the [feature][row] LDS arrays
constexpr int PGM_T = 256;
#define PGM_MIN_BIN 1e-3f   // pyro Spline: min_bin_width = min_bin_height = min_derivative
#define PGM_MIN_LAMBDA 0.025f

__host__ __device__ inline bool pgm_is_mlp(int kind) { return kind == CGEN_PGM_AFFINE || kind == CGEN_PGM_GUMBEL_MAX; }
__host__ __device__ inline int pgm_in(const cgen_pgm_mech& m, int l) { return l == 0 ? m.nctx : m.width[l - 1]; }
__host__ __device__ inline int pgm_out(const cgen_pgm_mech& m, int l) {
  return l < m.nhidden ? m.width[l] : (m.kind == CGEN_PGM_AFFINE ? 2 : m.ncls);
}

// ----------------------------------------------------------------------------- scalar pieces
__device__ __forceinline__ float pgm_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __noinline__ float pgm_act(int act, float z) {
  if (act == CGEN_PGM_GELU) return 0.5f * z * (1.f + erff(z * CGEN_SQRT1_2));
  if (act == CGEN_PGM_SIGMOID) return pgm_sigmoid(z);
  return z > 0.f ? z : 0.1f * z;
}
// x in [-1, 1] -> u = logit((x + 1) / 2) with the clamp torch's SigmoidTransform applies to f32 data, [FLT_MIN, 1 - FLT_EPSILON];
// extra = -(log 2 + logsigmoid(u) + logsigmoid(-u)).  (x + 1) / 2 is exact in f64; in f32 the sum alone loses up to half the bits of a
// small x, and log p - log(1 - p) cancels around p = 1/2.
__device__ __forceinline__ double pgm_normalize_inv(float x, double& extra) {
  double p = ((double)x + 1.0) * 0.5;
  const double lo = (double)FLT_MIN, hi = 1.0 - (double)FLT_EPSILON;
  p = p < lo ? lo : (p > hi ? hi : p);  // (a NaN stays a NaN)
  const double u = log(p) - log1p(-p);
  extra = -(0.69314718055994530942 - fabs(u) - 2.0 * log1p(exp(-fabs(u))));
  return u;
}

// softmax -> min + (1 - min K) s -> cumsum -> knots on [-bound, bound] (k[0..K]); one thread
__device__ void pgm_knots(const float* u, int K, double bound, double* k) {
  double mx = u[0];
  for (int j = 1; j < K; ++j) mx = fmax(mx, (double)u[j]);
  double se = 0.0;
  for (int j = 0; j < K; ++j) se += exp((double)u[j] - mx);
  double cum = 0.0;
  k[0] = -bound;
  for (int j = 0; j < K; ++j) {
    cum += (double)PGM_MIN_BIN + (1.0 - (double)PGM_MIN_BIN * K) * (exp((double)u[j] - mx) / se);
    k[j + 1] = cum * 2.0 * bound - bound;
  }
  k[K] = bound;
}

// the spline's derived quantities, once per workgroup by threads 0..3 (the caller synchronises): x knots at Misc[0..K], y knots at
// Misc[9..], derivatives at Misc[18..], lambdas at Misc[27..] (Misc: 36 doubles or more)
__device__ __forceinline__ void pgm_spline_tables(const cgen_pgm_mech& M, double* Misc, int tid) {
  const int K = M.bins;
  const float Bd = M.bound;
  double *xk = Misc, *yk = Misc + 9, *dk = Misc + 18, *lam = Misc + 27;
  if (tid == 0) pgm_knots(M.p[0], K, Bd, xk);
  if (tid == 1) pgm_knots(M.p[1], K, Bd, yk);
  if (tid == 2) {
    dk[0] = 1.0;  // linear tails: boundary derivatives 1
    for (int j = 1; j < K; ++j) {
      const double z = M.p[2][j - 1];
      dk[j] = (double)PGM_MIN_BIN + fmax(z, 0.0) + log1p(exp(-fabs(z)));
    }
    dk[K] = 1.0;
  }
  if (tid == 3)
    for (int j = 0; j < K; ++j)
      lam[j] = (1.0 - 2.0 * (double)PGM_MIN_LAMBDA) / (1.0 + exp(-(double)M.p[3][j])) + (double)PGM_MIN_LAMBDA;
}

// ----------------------------------------------------------------------------- one MLP layer over the rows of a workgroup
// Layer l's weights [out][in] and bias [out] into Wb, by all PGM_T threads (the caller synchronises before they are read).
__device__ __forceinline__ void pgm_layer_stage(const cgen_pgm_mech& M, int l, float* Wb, int tid) {
  const int wi = pgm_in(M, l), wo = pgm_out(M, l);
  for (int j = tid; j < wo * wi; j += PGM_T) Wb[j] = M.p[2 * l][j];
  for (int j = tid; j < wo; j += PGM_T) Wb[wo * wi + j] = M.p[2 * l + 1][j];
}
// Thread (r, q) computes outputs o = q, q + 4, ... of row r: out[o][r] = bias[o] + sum_i W[o][i] h(in[i][r]), where `in` holds the
// context (l = 0) or the previous layer's PRE-activations (l > 0, the activation is applied on the way in).  [feature][row] arrays
// with row stride PGM_RS; f64 accumulators, rounded to f32 once.
__device__ __forceinline__ void pgm_layer_rows(const cgen_pgm_mech& M, int l, const float* Wb, const float* in, float* out, int r, int q) {
  const int wi = pgm_in(M, l), wo = pgm_out(M, l), act = M.act;
  double acc[16];  // (f64 accumulators: see the note on precision at the top of pgm.hip)
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = (q + 4 * k < wo) ? (double)Wb[wo * wi + q + 4 * k] : 0.0;
  for (int i = 0; i < wi; ++i) {
    float hf = in[i * PGM_RS + r];
    if (l > 0) hf = pgm_act(act, hf);
    const double h = hf;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (q + 4 * k < wo) acc[k] += (double)Wb[(q + 4 * k) * wi + i] * h;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (q + 4 * k < wo) out[(q + 4 * k) * PGM_RS + r] = (float)acc[k];
}

// ----------------------------------------------------------------------------- host: the mechanism records
// (ncol < 0: a query that does not see the table -- columns and pointers are not looked at)
static int pgm_check(const char* who, const cgen_pgm_mech* mechs, int n, int ncol, bool need_g) {
  CGEN_REQUIRE(mechs, "%s: null mechanism records", who);
  CGEN_REQUIRE(n >= 1 && n <= CGEN_PGM_MAX_MECH, "%s: n = %d mechanisms, 1..%d are served", who, n, CGEN_PGM_MAX_MECH);
  for (int i = 0; i < n; ++i) {
    const cgen_pgm_mech& m = mechs[i];
    CGEN_REQUIRE(m.kind >= CGEN_PGM_BERNOULLI && m.kind <= CGEN_PGM_GUMBEL_MAX, "%s: mechanism %d: unknown kind %d", who, i, m.kind);
    int span = 1, nptr = 1;
    if (m.kind == CGEN_PGM_CATEGORICAL || m.kind == CGEN_PGM_GUMBEL_MAX)
      CGEN_REQUIRE(m.ncls >= 2 && m.ncls <= CGEN_PGM_MAX_CLS, "%s: mechanism %d: ncls = %d, 2..%d are served", who, i, m.ncls, CGEN_PGM_MAX_CLS);
    if (m.kind == CGEN_PGM_CATEGORICAL) span = m.ncls;
    if (m.kind == CGEN_PGM_SPLINE) {
      CGEN_REQUIRE(m.bins >= 2 && m.bins <= CGEN_PGM_MAX_BINS, "%s: mechanism %d: bins = %d, 2..%d are served", who, i, m.bins, CGEN_PGM_MAX_BINS);
      CGEN_REQUIRE(m.bound > 0.f && m.bound <= 3.402823466e38f, "%s: mechanism %d: bound = %g must be positive and finite", who, i, (double)m.bound);
      nptr = 4;
    }
    if (m.kind == CGEN_PGM_SPLINE || m.kind == CGEN_PGM_AFFINE)
      CGEN_REQUIRE(m.normalize == 0 || m.normalize == 1, "%s: mechanism %d: normalize = %d is not a flag", who, i, m.normalize);
    if (pgm_is_mlp(m.kind)) {
      CGEN_REQUIRE(m.nhidden >= 1 && m.nhidden <= CGEN_PGM_MAX_HIDDEN, "%s: mechanism %d: nhidden = %d hidden layers, 1..%d are served", who, i,
                   m.nhidden, CGEN_PGM_MAX_HIDDEN);
      for (int l = 0; l < m.nhidden; ++l)
        CGEN_REQUIRE(m.width[l] >= 1 && m.width[l] <= CGEN_PGM_MAX_WIDTH, "%s: mechanism %d: width[%d] = %d, 1..%d are served", who, i, l,
                     m.width[l], CGEN_PGM_MAX_WIDTH);
      CGEN_REQUIRE(m.act >= CGEN_PGM_LEAKY_RELU && m.act <= CGEN_PGM_SIGMOID, "%s: mechanism %d: unknown act %d", who, i, m.act);
      CGEN_REQUIRE(m.nctx >= 1 && m.nctx <= 2, "%s: mechanism %d: nctx = %d context columns, 1..2 are served", who, i, m.nctx);
      for (int c = 0; c < m.nctx && ncol >= 0; ++c)
        CGEN_REQUIRE(m.ctx_col[c] >= 0 && m.ctx_col[c] < ncol, "%s: mechanism %d: ctx_col[%d] = %d is out of range (ncol = %d)", who, i, c,
                     m.ctx_col[c], ncol);
      nptr = 2 * (m.nhidden + 1);
    }
    if (ncol >= 0)
      CGEN_REQUIRE(m.col >= 0 && m.col + span <= ncol, "%s: mechanism %d: col = %d (+%d) is out of range (ncol = %d)", who, i, m.col, span, ncol);
    for (int k = 0; k < nptr && ncol >= 0; ++k) {
      CGEN_REQUIRE(m.p[k], "%s: mechanism %d: null parameter pointer p[%d]", who, i, k);
      CGEN_REQUIRE(!need_g || m.g[k], "%s: mechanism %d: null gradient pointer g[%d]", who, i, k);
    }
  }
  return CGEN_OK;
}

}  // namespace cgen
