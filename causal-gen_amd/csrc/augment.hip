// Device-resident input pipeline (include/cgen_hip.h, cgen_batch_augment): row gather from a resident u8 NCHW data set, zero-padded
// random crop, horizontal flip, (v - sub) * mul and the NCHW -> NHWC layout change in ONE launch, with the parents of the same rows
// gathered on the side.  Replaces the reference's per-sample PIL work (src/datasets.py: RandomCrop(padding) + RandomHorizontalFlip),
// the host-to-device copy and trainer.py:16-21.
//
// A bandwidth kernel: 1 byte in, 2-16 bytes out per element.  The grid is (image, chunk of the image): the data set row, the Philox
// draw and every bound below are uniform over a workgroup, so they live in scalar registers and a lane only forms its own pixel
// address.  Source bytes are fetched one per lane at arbitrary alignment (consecutive lanes read consecutive bytes of a row, mirrored
// under a flip); the output goes out as 16-byte stores wherever the view allows it:
//   ROW arm  (out.sw == c, no channel padding): a row of r_w * c elements is contiguous; a lane owns 16 bytes of it, the ragged end of
//            a row (and every row of a view that is not 16-byte aligned) is written element by element;
//   PIX arm  (the engine's own tensors: pixel stride rounded up to 8 channels, or a channel slice of a wider tensor): a lane owns one
//            pixel and writes its max(c, cpad) channels -- the zero padding included -- as whole 16-byte groups when the view is
//            aligned, element by element otherwise.
// cgen_batch_augment_planar is one more instance of the kernel for the consumers that read contiguous f32 NCHW (the anticausal
// predictors): a lane owns one element of [c, r_h, r_w], 4-byte stores, same draws and same per-pixel arithmetic.
#include "common.h"

namespace cgen {

struct AugP {
  int n, c, h0, w0, rh, rw, padx, pady, ctx;
  uint32_t stream_id;
  float p, sub, mul;
  int64_t n_data;
  const uint8_t* data;
  const int64_t* index;
  const uint64_t* rng;
  const int32_t* draws_in;
  int32_t* draws_out;
  const float* pa_data;
  float* pa_out;
};

enum { AUG_ROW = 0, AUG_PIX_VEC = 1, AUG_PIX_SCALAR = 2, AUG_PLANAR = 3 };

template <typename T> union AugPack { T e[16 / sizeof(T)]; uint4 v; };

// everything one image needs, uniform over the workgroup
struct AugDraw {
  const uint8_t* img;  // first byte of the row's image (row 0 for an out-of-range row: never read through)
  int oy, ox, flip;
  bool valid;
};

__device__ __forceinline__ float aug_px(const AugP& a, const AugDraw& d, int ch, int y, int x) {
  const int sx = d.flip > 0 ? a.rw - 1 - x : x;
  const int iy = d.oy + y - a.pady, ix = d.ox + sx - a.padx;
  const bool ok = d.valid && (unsigned)iy < (unsigned)a.h0 && (unsigned)ix < (unsigned)a.w0;
  // (never a load under a condition: an in-range dummy address instead)
  const uint8_t v = d.img[ok ? (ch * a.h0 + iy) * a.w0 + ix : 0];
  return ((ok ? (float)v : 0.f) - a.sub) * a.mul;
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void batch_augment_kernel(AugP a, View out, int chunks, int groups, int tail, int cw) {
  constexpr int E = 16 / sizeof(T);
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int64_t row = a.index[b];
  AugDraw d;
  d.valid = row >= 0 && row < a.n_data;
  const int64_t rowc = d.valid ? row : 0;
  d.img = a.data + rowc * ((int64_t)a.c * a.h0 * a.w0);
  if (a.draws_in) {
    d.oy = a.draws_in[3 * (int64_t)b];
    d.ox = a.draws_in[3 * (int64_t)b + 1];
    d.flip = a.draws_in[3 * (int64_t)b + 2] != 0;
  } else {
    uint32_t r[4];
    Philox::gen(a.rng[0], a.rng[1], a.stream_id, (uint64_t)rowc, r);
    d.oy = (int)__umulhi(r[0], (uint32_t)(a.h0 + 2 * a.pady - a.rh + 1));
    d.ox = (int)__umulhi(r[1], (uint32_t)(a.w0 + 2 * a.padx - a.rw + 1));
    // (u01 rounds its largest argument up to 1.0f: p = 1 must still flip every row)
    d.flip = (Philox::u01(r[2]) < a.p || a.p >= 1.f) ? 1 : 0;
  }
  if (!d.valid) d.oy = d.ox = d.flip = -1;
  if (chunk == 0) {
    if (a.draws_out && threadIdx.x < 3) a.draws_out[3 * (int64_t)b + threadIdx.x] = threadIdx.x == 0 ? d.oy : threadIdx.x == 1 ? d.ox : d.flip;
    if (a.pa_out)
      for (int j = threadIdx.x; j < a.ctx; j += 256) {
        const float v = a.pa_data[rowc * a.ctx + j];
        a.pa_out[(int64_t)b * a.ctx + j] = d.valid ? v : 0.f;
      }
  }
  if (MODE == AUG_ROW) {
    const int per_row = groups + tail;
    const int items = a.rh * per_row;
    for (int i = chunk * 256 + threadIdx.x; i < items; i += chunks * 256) {
      const int y = i / per_row, u = i - y * per_row;
      T* dst = vptr<T>(out, b, y, 0);
      if (u < groups) {
        const int e0 = u * E;
        int x = e0 / a.c, ch = e0 - x * a.c;
        AugPack<T> pk;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          pk.e[e] = Elem<T>::to(aug_px(a, d, ch, y, x));
          if (++ch == a.c) { ch = 0; ++x; }
        }
        *(uint4*)(dst + e0) = pk.v;
      } else {
        const int e0 = groups * E + (u - groups);
        const int x = e0 / a.c, ch = e0 - x * a.c;
        Elem<T>::st(dst + e0, aug_px(a, d, ch, y, x));
      }
    }
  } else if (MODE == AUG_PLANAR) {
    // contiguous [n, c, r_h, r_w]: a lane owns one element, consecutive lanes consecutive pixels of a plane
    const int hw = a.rh * a.rw, items = a.c * hw;
    T* dst = (T*)out.p + (int64_t)b * items;
    for (int i = chunk * 256 + threadIdx.x; i < items; i += chunks * 256) {
      const int ch = i / hw, q = i - ch * hw, y = q / a.rw, x = q - y * a.rw;
      Elem<T>::st(dst + i, aug_px(a, d, ch, y, x));
    }
  } else {
    const int items = a.rh * a.rw;
    for (int i = chunk * 256 + threadIdx.x; i < items; i += chunks * 256) {
      const int y = i / a.rw, x = i - y * a.rw;
      T* dst = vptr<T>(out, b, y, x);
      float v[4];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) v[ch] = aug_px(a, d, ch < a.c ? ch : 0, y, x);  // (channels >= c: a copy of channel 0, never stored)
      if (MODE == AUG_PIX_VEC) {
        AugPack<T> pk;
#pragma unroll
        for (int e = 0; e < E; ++e) pk.e[e] = (e < 4 && e < a.c) ? Elem<T>::to(v[e < 4 ? e : 0]) : (T)0;
        *(uint4*)dst = pk.v;
        for (int g = E; g < cw; g += E) *(uint4*)(dst + g) = make_uint4(0u, 0u, 0u, 0u);
      } else {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < a.c) Elem<T>::st(dst + ch, v[ch]);
        for (int ch = a.c; ch < cw; ++ch) dst[ch] = (T)0;
      }
    }
  }
}

struct AugPlan {
  int mode, groups, tail, cw, chunks, arm;
};

// validation + choice of the kernel instance; nothing is launched from here
static int aug_plan(const cgen_augment_args* a, AugPlan* pl) {
  CGEN_REQUIRE(a, "cgen_batch_augment: null args");
  CGEN_REQUIRE(a->dtype == CGEN_F32 || a->dtype == CGEN_F16, "cgen_batch_augment: bad dtype %d", a->dtype);
  CGEN_REQUIRE(a->data && a->index && a->out.p, "cgen_batch_augment: null data, index or out");
  CGEN_REQUIRE(a->n > 0 && a->n_data > 0, "cgen_batch_augment: empty batch or data set (n %d, n_data %lld)", a->n, (long long)a->n_data);
  CGEN_REQUIRE(a->c >= 1 && a->c <= 4, "cgen_batch_augment: c must be 1..4 (got %d)", a->c);
  CGEN_REQUIRE(a->out.c == a->c, "cgen_batch_augment: out.c %d != c %d", a->out.c, a->c);
  CGEN_REQUIRE(a->h0 > 0 && a->w0 > 0 && a->r_h > 0 && a->r_w > 0 && a->pad_x >= 0 && a->pad_y >= 0, "cgen_batch_augment: bad geometry");
  CGEN_REQUIRE((int64_t)a->c * a->h0 * a->w0 < (1ll << 30) && a->r_h < (1 << 14) && a->r_w < (1 << 14) && a->pad_x < (1 << 14) && a->pad_y < (1 << 14),
               "cgen_batch_augment: image too large");
  CGEN_REQUIRE(a->h0 + 2 * a->pad_y - a->r_h >= 0 && a->w0 + 2 * a->pad_x - a->r_w >= 0,
               "cgen_batch_augment: crop %dx%d larger than the padded image %dx%d", a->r_h, a->r_w, a->h0 + 2 * a->pad_y, a->w0 + 2 * a->pad_x);
  CGEN_REQUIRE(a->hflip_p >= 0.f && a->hflip_p <= 1.f, "cgen_batch_augment: hflip_p %g outside [0, 1]", (double)a->hflip_p);
  CGEN_REQUIRE(a->rng || a->draws_in, "cgen_batch_augment: neither a Philox state nor injected draws");
  CGEN_REQUIRE((a->pa_data != nullptr) == (a->pa_out != nullptr), "cgen_batch_augment: pa_data and pa_out go together");
  CGEN_REQUIRE(!a->pa_data || a->ctx > 0, "cgen_batch_augment: ctx must be > 0 with parents (got %d)", a->ctx);
  const int esz = a->dtype == CGEN_F32 ? 4 : 2, E = 16 / esz;
  const int cw = a->out.cpad > a->c ? a->out.cpad : a->c;
  CGEN_REQUIRE(cw <= 64 && a->out.sw >= cw && a->out.sh >= 0 && a->out.sn >= 0, "cgen_batch_augment: bad out view (sw %lld, cpad %d)",
               (long long)a->out.sw, a->out.cpad);
  pl->cw = cw;
  pl->groups = pl->tail = 0;
  int64_t items;
  if (a->out.sw == a->c && cw == a->c) {
    pl->mode = AUG_ROW;
    const int L = a->r_w * a->c;
    const bool aligned = ((uintptr_t)a->out.p % 16 == 0) && ((a->out.sn * esz) % 16 == 0) && ((a->out.sh * esz) % 16 == 0);
    pl->groups = aligned ? L / E : 0;
    pl->tail = L - pl->groups * E;
    items = (int64_t)a->r_h * (pl->groups + pl->tail);
    pl->arm = pl->groups == 0 ? 2 : pl->tail == 0 ? 0 : 1;
  } else {
    const bool vec = vec16_ok(a->out, esz) && cw % E == 0;
    pl->mode = vec ? AUG_PIX_VEC : AUG_PIX_SCALAR;
    items = (int64_t)a->r_h * a->r_w;
    pl->arm = vec ? 3 : 4;
  }
  int64_t chunks = (items + 255) / 256;
  if (chunks > 256) chunks = 256;
  CGEN_REQUIRE((int64_t)a->n * chunks < (1ll << 31), "cgen_batch_augment: batch too large");
  pl->chunks = (int)chunks;
  return CGEN_OK;
}

}  // namespace cgen

using namespace cgen;

extern "C" int cgen_batch_augment_arm(const cgen_augment_args* a) {
  AugPlan pl;
  const int rc = aug_plan(a, &pl);
  return rc != CGEN_OK ? rc : pl.arm;
}

static void aug_params(AugP& p, const cgen_augment_args* a) {
  p.n = a->n; p.c = a->c; p.h0 = a->h0; p.w0 = a->w0; p.rh = a->r_h; p.rw = a->r_w; p.padx = a->pad_x; p.pady = a->pad_y;
  p.ctx = a->ctx; p.stream_id = a->stream_id; p.p = a->hflip_p; p.sub = a->sub; p.mul = a->mul; p.n_data = a->n_data;
  p.data = (const uint8_t*)a->data; p.index = a->index; p.rng = a->rng; p.draws_in = a->draws_in; p.draws_out = a->draws_out;
  p.pa_data = a->pa_data; p.pa_out = a->pa_out;
}

extern "C" int cgen_batch_augment(const cgen_augment_args* a, cgen_stream_t stream) {
  AugPlan pl;
  const int rc = aug_plan(a, &pl);
  if (rc != CGEN_OK) return rc;
  AugP p;
  aug_params(p, a);
  const dim3 g((unsigned)(a->n * pl.chunks)), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define AUG_LAUNCH(T_, M_) hipLaunchKernelGGL((batch_augment_kernel<T_, M_>), g, blk, 0, st, p, mk(a->out), pl.chunks, pl.groups, pl.tail, pl.cw)
  if (a->dtype == CGEN_F32) {
    if (pl.mode == AUG_ROW) AUG_LAUNCH(float, AUG_ROW); else if (pl.mode == AUG_PIX_VEC) AUG_LAUNCH(float, AUG_PIX_VEC); else AUG_LAUNCH(float, AUG_PIX_SCALAR);
  } else {
    if (pl.mode == AUG_ROW) AUG_LAUNCH(h16_t, AUG_ROW); else if (pl.mode == AUG_PIX_VEC) AUG_LAUNCH(h16_t, AUG_PIX_VEC); else AUG_LAUNCH(h16_t, AUG_PIX_SCALAR);
  }
#undef AUG_LAUNCH
  return check_launch("cgen_batch_augment");
}

extern "C" int cgen_batch_augment_planar(const cgen_augment_args* a, cgen_stream_t stream) {
  const char* fn = "cgen_batch_augment_planar";
  CGEN_REQUIRE(a, "%s: null args", fn);
  CGEN_REQUIRE(a->dtype == CGEN_F32, "%s: the planar output is f32 (dtype %d)", fn, a->dtype);
  CGEN_REQUIRE(a->c >= 1 && a->c <= 4, "%s: c must be 1..4 (got %d)", fn, a->c);
  // everything that is not about the output view is cgen_batch_augment's own check, made on the NHWC view of the same memory
  cgen_augment_args q = *a;
  q.out.sn = (int64_t)a->c * a->r_h * a->r_w; q.out.sh = (int64_t)a->c * a->r_w; q.out.sw = a->c; q.out.cpad = 0;
  AugPlan pl;
  const int rc = aug_plan(&q, &pl);
  if (rc != CGEN_OK) return rc;
  CGEN_REQUIRE(a->out.sn == (int64_t)a->c * a->r_h * a->r_w && a->out.sh == a->r_w && a->out.sw == 1 && a->out.cpad <= a->c,
               "%s: out must be a contiguous [n, c, r_h, r_w] (sn %lld, sh %lld, sw %lld, cpad %d)", fn, (long long)a->out.sn,
               (long long)a->out.sh, (long long)a->out.sw, a->out.cpad);
  int64_t chunks = ((int64_t)a->c * a->r_h * a->r_w + 255) / 256;
  if (chunks > 256) chunks = 256;
  CGEN_REQUIRE((int64_t)a->n * chunks < (1ll << 31), "%s: batch too large", fn);
  AugP p;
  aug_params(p, a);
  hipLaunchKernelGGL((batch_augment_kernel<float, AUG_PLANAR>), dim3((unsigned)(a->n * chunks)), dim3(256), 0, (hipStream_t)stream, p,
                     mk(a->out), (int)chunks, 0, 0, a->c);
  return check_launch(fn);
}
