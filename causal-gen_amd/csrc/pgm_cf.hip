// Parent SCM: counterfactual parents (cgen_pgm_counterfactual; the reference's BasePGM.counterfactual, flow_pgm.py:71-108, followed
// by dscm.py's vae_preprocess).  Abduction, action and prediction over the mechanism records of csrc/pgm.hip in ONE launch.
//
// One workgroup of 512 threads per 64 rows: thread (r, q, side) = (tid & 63, (tid >> 6) & 3, tid >> 8) works on row r, waves 0..3
// on the factual context of an MLP and waves 4..7 on the counterfactual one, and the workgroup walks the mechanisms in record
// (topological) order; thread (r, 0, 0) owns row r's scalar work.  The mask is one word for the whole launch, so which mechanisms
// are intervened on, which are touched (in the mask, or with a touched context mechanism) and which MLPs have to run is uniform
// over the grid: every branch around a barrier is taken by all threads alike.  A mechanism's counterfactual value (the first column of its span) goes
// to Val[mechanism][row] in LDS, where later mechanisms read their counterfactual context.  An MLP runs only when something needs
// it -- the factual pass for the noise of a touched mechanism or for `eps`, the counterfactual pass for a touched mechanism -- with
// each layer's weights staged in LDS once and applied to both contexts side by side; the hidden pre-activations ping-pong between
// two [width][row] arrays per context.  After the walk wave w writes columns w, w + 8, ... of its rows of `cf` (the do row's bits
// for a masked mechanism, Val for an MLP mechanism, the observation's bits for everything else) and wave 0 the two parents rows.
// No atomics, no workspace, no RNG (the caller supplies the Gumbel-max uniforms, with cgen_philox_uniform or its own draws); every store is plain C++; reruns are bit-identical.
// Precision follows pgm.hip: buffers and activations f32; dot products, the spline inverse, the affine round trip (eps stays in its
// f64 register between abduction and prediction), the Gumbel algebra and the log-standardisation in f64, rounded to f32 once.
#include "pgm_common.h"

namespace cgen {

struct PgmCfP {
  cgen_pgm_mech m[CGEN_PGM_MAX_MECH];
  cgen_pgm_cf_args a;
  int n, W, ctx;                         // W: largest hidden width of any MLP (0 without one); ctx: floats per parents row
  int ctx_mech[CGEN_PGM_MAX_MECH][2];    // the record whose `col` a context column is
};
constexpr int PGM_CF_T = 2 * PGM_T;  // the factual and the counterfactual half
static_assert(sizeof(PgmCfP) < 4096 - 64, "records and arguments travel by value in a 4 KiB kernel-argument segment");

static inline int pgm_cf_lds_floats(int W) {
  const int WM = W > 16 ? W : 16;
  return 128 + 4 * W * PGM_RS + (W ? WM * WM + WM : 0) + (32 + 4 + CGEN_PGM_MAX_MECH) * PGM_RS;
}

// eps = spline^-1(u) from the tables of pgm_spline_tables: the closed-form inverse of the bin's linear-fractional piece
__device__ __forceinline__ double pgm_spline_inv(const double* Misc, int K, double Bd, double u) {
  const double *xk = Misc, *yk = Misc + 9, *dk = Misc + 18, *lam = Misc + 27;
  if (!(u > -Bd && u < Bd)) return u;  // the identity outside the bound (a NaN stays a NaN)
  int idx = 0;
  for (int j = 1; j < K; ++j) idx += (u >= yk[j]) ? 1 : 0;
  const double x0 = xk[idx], x1 = xk[idx + 1], y0 = yk[idx], y1 = yk[idx + 1], d0 = dk[idx], d1 = dk[idx + 1], lm = lam[idx];
  const double dx = x1 - x0, wb = sqrt(d0 / d1), s = (y1 - y0) / dx;  // w_a = 1
  const double wc = (lm * d0 + (1.0 - lm) * wb * d1) / s;
  const double yc = ((1.0 - lm) * y0 + lm * wb * y1) / ((1.0 - lm) + lm * wb);
  double th;
  if (u <= yc) {
    const double a0 = y0 - u, a1 = (u - yc) * wc;
    th = lm * a0 / (a0 + a1);
  } else {
    const double b0 = wc * (yc - u), b1 = wb * (u - y1);
    th = (b0 + lm * b1) / (b0 + b1);
  }
  return th * dx + x0;
}

// dscm.py ukbb_preprocess of one value
__device__ __forceinline__ float pgm_pre_apply(const cgen_pgm_pre& p, float x) {
  if (p.kind == CGEN_PGM_PRE_COPY) return x;
  double t = ((double)x + 1.0) / 2.0 * ((double)p.hi - (double)p.lo) + (double)p.lo;
  t = t < 1e-12 ? 1e-12 : t;  // (a NaN stays a NaN, as torch's clamp keeps it)
  return (float)((log(t) - (double)p.mu) / (double)p.sd);
}

__global__ __launch_bounds__(PGM_CF_T) void pgm_cf_kernel(const PgmCfP P) {
  extern __shared__ float sm[];
  const cgen_pgm_cf_args& a = P.a;
  const int tid = threadIdx.x, r = tid & 63, q = (tid >> 6) & 3, side = tid >> 8, n = P.n, W = P.W, WM = W > 16 ? W : 16, ncol = a.ncol;
  double* const Misc = (double*)sm;                  // [64] the spline's derived quantities (first: 8-byte aligned)
  float* const ZA = sm + 128;                        // [2][W][RS] hidden pre-activations at the factual context, ping-pong
  float* const ZB = ZA + 2 * W * PGM_RS;             // the same at the counterfactual context
  float* const Wb = ZB + 2 * W * PGM_RS;             // one layer's weights and bias
  float* const DoutA = Wb + (W ? WM * WM + WM : 0);  // [16][RS] MLP outputs at the factual context
  float* const DoutB = DoutA + 16 * PGM_RS;          // and at the counterfactual one
  float* const CtxA = DoutB + 16 * PGM_RS;           // [2][RS]
  float* const CtxB = CtxA + 2 * PGM_RS;             // [2][RS]
  float* const Val = CtxB + 2 * PGM_RS;              // [n][RS] counterfactual value of each mechanism's first column

  uint32_t mask = a.do_mask_dev ? a.do_mask_dev[0] : a.do_mask;
  mask &= (1u << n) - 1u;
  uint32_t touched = 0;
  for (int mi = 0; mi < n; ++mi) {
    uint32_t bit = (mask >> mi) & 1u;
    if (pgm_is_mlp(P.m[mi].kind))
      for (int c = 0; c < P.m[mi].nctx; ++c) bit |= (touched >> P.ctx_mech[mi][c]) & 1u;
    touched |= bit << mi;
  }

  const int row = blockIdx.x * PGM_R + r;
  const bool valid = row < a.rows, own = tid < PGM_R;
  const int64_t src = valid ? (a.index ? a.index[row] : (int64_t)row) : 0;
  const bool inrange = src >= 0 && src < a.table_rows;
  const float* orow = a.obs + (inrange ? src : 0) * ncol;
  bool live = valid && inrange;  // a row an index sends outside its table is NaN in every output; nothing is read out of bounds
  const float* drow = orow;      // (read under a non-zero mask only)
  if (mask) {
    const int64_t dsrc = valid ? (a.do_index ? a.do_index[row] : (int64_t)row) : 0;
    const bool din = dsrc >= 0 && dsrc < a.do_rows;
    drow = a.do_table + (din ? dsrc : 0) * ncol;
    live = live && din;
  }
  auto ldo = [&](int c) { return live ? orow[c] : NAN; };
  auto ldd = [&](int c) { return live ? drow[c] : NAN; };

  for (int mi = 0; mi < n; ++mi) {
    const cgen_pgm_mech& M = P.m[mi];
    const int kind = M.kind;
    const bool inmask = (mask >> mi) & 1u;
    const bool compute = ((touched >> mi) & 1u) && !inmask && pgm_is_mlp(kind);
    const float base = inmask ? ldd(M.col) : ldo(M.col);
    float* const eps_out = (a.eps && valid) ? a.eps + (int64_t)row * n + mi : nullptr;
    float* const val = Val + mi * PGM_RS + r;

    if (kind == CGEN_PGM_SPLINE && a.eps) {
      pgm_spline_tables(M, Misc, tid);
      __syncthreads();
      if (own) {
        const float x = ldo(M.col);
        double extra, u = x;
        if (M.normalize) u = pgm_normalize_inv(x, extra);
        if (eps_out) *eps_out = (float)pgm_spline_inv(Misc, M.bins, (double)M.bound, u);
      }
      __syncthreads();  // (the next spline's tables go to the same place)
    }
    const bool need_f = compute || (kind == CGEN_PGM_AFFINE && a.eps);
    if (!need_f) {
      if (own) {
        *val = base;
        if (eps_out && kind != CGEN_PGM_SPLINE) *eps_out = live ? 0.f : NAN;
      }
      continue;
    }

    // ---- AFFINE / GUMBEL_MAX: the MLP at the factual context and, for a touched mechanism, at the counterfactual one
    const int L = M.nhidden, nout = pgm_out(M, L);
    if (own)
      for (int c = 0; c < M.nctx; ++c) {
        CtxA[c * PGM_RS + r] = ldo(M.ctx_col[c]);
        if (compute) CtxB[c * PGM_RS + r] = Val[P.ctx_mech[mi][c] * PGM_RS + r];  // (written by this very thread)
      }
    for (int l = 0; l <= L; ++l) {
      if (side == 0) pgm_layer_stage(M, l, Wb, tid);
      __syncthreads();
      const int in = ((l - 1) & 1) * W * PGM_RS, out = (l & 1) * W * PGM_RS;
      if (side == 0) pgm_layer_rows(M, l, Wb, l == 0 ? CtxA : ZA + in, l < L ? ZA + out : DoutA, r, q);
      else if (compute) pgm_layer_rows(M, l, Wb, l == 0 ? CtxB : ZB + in, l < L ? ZB + out : DoutB, r, q);
      __syncthreads();
    }
    if (!own) continue;
    float v = base;
    if (kind == CGEN_PGM_AFFINE) {
      const float x = ldo(M.col);
      double extra, u = x;
      if (M.normalize) u = pgm_normalize_inv(x, extra);
      const double eps = (u - (double)DoutA[r]) * exp(-(double)DoutA[PGM_RS + r]);
      if (eps_out) *eps_out = (float)eps;
      if (compute) {
        const double y = (double)DoutB[r] + exp((double)DoutB[PGM_RS + r]) * eps;
        v = M.normalize ? (float)tanh(0.5 * y) : (float)y;  // 2 sigmoid(y) - 1 = tanh(y / 2)
      }
    } else {
      if (eps_out) *eps_out = live ? 0.f : NAN;
      // (compute is set: a Gumbel-max mechanism has no noise to report and runs for a touched row only)
      const float f = ldo(M.col);
      const int cls = (f >= 0.f && f < (float)nout) ? (int)f : -1;  // (a NaN or foreign class gives NaN)
      const float* U = a.uniforms[mi] + (int64_t)(valid ? row : 0) * nout;
      auto gumbel = [&](int j) {
        float uj = U[j];
        if (uj == 0.f) uj = FLT_MIN;
        return -log(-log((double)uj));
      };
      v = NAN;
      if (cls >= 0) {
        const double gk = gumbel(cls), lk = DoutA[cls * PGM_RS + r];
        double level;  // exact: the maximum Z = logsumexp(logits) + a fresh Gumbel; else the reference's g_k - logit_k
        if (a.exact_gumbel) {
          double mx = DoutA[r];
          for (int j = 1; j < nout; ++j) mx = fmax(mx, (double)DoutA[j * PGM_RS + r]);
          double se = 0.0;
          for (int j = 0; j < nout; ++j) se += exp((double)DoutA[j * PGM_RS + r] - mx);
          level = mx + log(se) + gk;
        } else {
          level = gk - lk;
        }
        double best = 0.0;
        int arg = -1;
        bool nan = false;
        for (int j = 0; j < nout; ++j) {
          const double lj = DoutA[j * PGM_RS + r];
          double noise;
          if (a.exact_gumbel)
            noise = (j == cls ? level : -log(exp(-(gumbel(j) + lj)) + exp(-level))) - lj;
          else
            noise = j == cls ? level : -log(exp(-(gumbel(j) + lj)) + exp(-level)) - lj;
          const double score = noise + (double)DoutB[j * PGM_RS + r];
          nan = nan || score != score;
          if (arg < 0 || score > best) {  // the first index wins ties, as argmax does
            best = score;
            arg = j;
          }
        }
        if (!nan) v = (float)arg;
      }
    }
    *val = v;
  }
  __syncthreads();
  if (!valid) return;

  // the counterfactual value of column c of this thread's row
  auto cf_at = [&](int c) {
    float v = orow[c];
    for (int mi = 0; mi < n; ++mi) {
      const cgen_pgm_mech& M = P.m[mi];
      const int span = M.kind == CGEN_PGM_CATEGORICAL ? M.ncls : 1;
      if (c < M.col || c >= M.col + span) continue;
      if ((mask >> mi) & 1u) v = drow[c];
      else if (pgm_is_mlp(M.kind)) v = Val[mi * PGM_RS + r];
      else v = orow[c];
    }
    return v;
  };
  for (int c = tid >> 6; c < ncol; c += PGM_CF_T / 64) a.cf[(int64_t)row * ncol + c] = live ? cf_at(c) : NAN;
  if (!own || (!a.pa && !a.cf_pa)) return;
  int o = 0;
  for (int k = 0; k < a.npre; ++k) {
    const cgen_pgm_pre& p = a.pre[k];
    for (int j = 0; j < p.width; ++j, ++o) {
      if (a.pa) a.pa[(int64_t)row * P.ctx + o] = live ? pgm_pre_apply(p, orow[p.col + j]) : NAN;
      if (a.cf_pa) a.cf_pa[(int64_t)row * P.ctx + o] = live ? pgm_pre_apply(p, cf_at(p.col + j)) : NAN;
    }
  }
}

}  // namespace cgen

using namespace cgen;

extern "C" int cgen_pgm_counterfactual(const cgen_pgm_mech* mechs, int32_t n, const cgen_pgm_cf_args* a, cgen_stream_t stream) {
  const char* who = "cgen_pgm_counterfactual";
  CGEN_REQUIRE(a, "%s: null arguments", who);
  CGEN_REQUIRE(a->obs, "%s: null obs", who);
  CGEN_REQUIRE(a->ncol >= 1, "%s: ncol = %d", who, a->ncol);
  CGEN_REQUIRE(a->rows >= 1 && a->rows <= (1 << 24), "%s: rows = %d, 1..2^24 are served", who, a->rows);
  CGEN_REQUIRE(a->table_rows >= 1 && (a->index || a->table_rows >= a->rows), "%s: table_rows = %lld does not cover %d rows", who,
               (long long)a->table_rows, a->rows);
  CGEN_REQUIRE(a->cf, "%s: null cf", who);
  if (int rc = pgm_check(who, mechs, n, a->ncol, false)) return rc;
  PgmCfP P;
  memset(&P, 0, sizeof(P));
  for (int i = 0; i < n; ++i) {
    const cgen_pgm_mech& m = mechs[i];
    P.m[i] = m;
    for (int k = 0; k < 8; ++k) P.m[i].g[k] = nullptr;  // (not read)
    if (!pgm_is_mlp(m.kind)) continue;
    for (int c = 0; c < m.nctx; ++c) {
      int at = -1;
      for (int j = 0; j < i; ++j)
        if (mechs[j].col == m.ctx_col[c]) at = j;
      CGEN_REQUIRE(at >= 0, "%s: mechanism %d: ctx_col[%d] = %d is not the col of an earlier record (topological order)", who, i, c,
                   m.ctx_col[c]);
      P.ctx_mech[i][c] = at;
    }
    for (int l = 0; l < m.nhidden; ++l)
      if (m.width[l] > P.W) P.W = m.width[l];
    if (m.kind == CGEN_PGM_GUMBEL_MAX) CGEN_REQUIRE(a->uniforms[i], "%s: mechanism %d is GUMBEL_MAX: null uniforms[%d]", who, i, i);
  }
  CGEN_REQUIRE(a->exact_gumbel == 0 || a->exact_gumbel == 1, "%s: exact_gumbel = %d is not a flag", who, a->exact_gumbel);
  if (!a->do_mask_dev)
    CGEN_REQUIRE((a->do_mask >> n) == 0, "%s: do_mask = 0x%x has a bit at or above n = %d", who, a->do_mask, n);
  if (a->do_mask_dev || a->do_mask) {
    CGEN_REQUIRE(a->do_table, "%s: null do_table with an intervention mask", who);
    CGEN_REQUIRE(a->do_rows >= 1 && (a->do_index || a->do_rows >= a->rows), "%s: do_rows = %lld does not cover %d rows", who,
                 (long long)a->do_rows, a->rows);
  }
  CGEN_REQUIRE(a->npre >= 0 && a->npre <= CGEN_PGM_MAX_PRE, "%s: npre = %d preprocess records, 0..%d are served", who, a->npre, CGEN_PGM_MAX_PRE);
  CGEN_REQUIRE((!a->pa && !a->cf_pa) || a->npre >= 1, "%s: npre = 0 with a parents output", who);
  for (int k = 0; k < a->npre; ++k) {
    const cgen_pgm_pre& p = a->pre[k];
    CGEN_REQUIRE(p.kind == CGEN_PGM_PRE_COPY || p.kind == CGEN_PGM_PRE_LOGSTD, "%s: pre[%d]: unknown kind %d", who, k, p.kind);
    CGEN_REQUIRE(p.width >= 1 && p.col >= 0 && (int64_t)p.col + p.width <= a->ncol, "%s: pre[%d]: col = %d (+%d) is out of range (ncol = %d)", who,
                 k, p.col, p.width, a->ncol);
    CGEN_REQUIRE(p.kind != CGEN_PGM_PRE_LOGSTD || (p.sd != 0.f && p.sd == p.sd), "%s: pre[%d]: sd = %g", who, k, (double)p.sd);
    P.ctx += p.width;
  }
  P.a = *a;
  P.n = n;
  const size_t lds = (size_t)pgm_cf_lds_floats(P.W) * sizeof(float);
  static bool once = false;
  if (!once) {
    const hipError_t e = hipFuncSetAttribute((const void*)pgm_cf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return fail(CGEN_ELAUNCH, "%s: cannot raise the LDS limit: %s", who, hipGetErrorString(e));
    once = true;
  }
  hipLaunchKernelGGL(pgm_cf_kernel, dim3(ceil_div(a->rows, PGM_R)), dim3(PGM_CF_T), lds, (hipStream_t)stream, P);
  return check_launch(who);
}
