// The kit shared by the convolution units -- csrc/conv.hip (forward / data gradient) and csrc/wgrad.hip (weight gradient):
// vector types, FastDiv, 4-element and 16-byte-group access, the in-LDS activation pass, the pixel-tile ("row piece") layout
// with its DMA, and the small host helpers both launch sides size things with.  Parameter structs of one unit stay in that unit.
#pragma once
#include "common.h"

#ifdef CGEN_NO_SETPRIO
#define CGEN_SETPRIO() do {} while (0)
#else
#define CGEN_SETPRIO() __builtin_amdgcn_s_setprio(3)
#endif

namespace cgen {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The fast division of fastdiv.h in the sixteen-byte form the conv / weight-gradient kernel arguments and PixTile carry
// (`d` is the divisor itself, `pad` keeps the layout)
struct FastDiv {
  uint32_t mul, shift, d, pad;
};
static inline FastDiv mk_fastdiv(uint32_t d) {
  const Div32 q = mk_div32(d);
  FastDiv f;
  f.mul = q.mul; f.shift = q.shift; f.d = d; f.pad = 0;
  return f;
}
__device__ __forceinline__ int fdiv(int n, const FastDiv& f) { return div32(n, Div32{f.mul, f.shift}); }

// 4-element (16B f32 / 8B bf16) vector access
template <typename T> __device__ __forceinline__ void ld4(const T* p, float (&v)[4]);
template <> __device__ __forceinline__ void ld4<float>(const float* p, float (&v)[4]) {
  const float4 t = *(const float4*)p;
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void ld4<h16_t>(const h16_t* p, float (&v)[4]) {
  const uint2 t = *(const uint2*)p;
  v[0] = h_lo(t.x); v[1] = h_hi(t.x);
  v[2] = h_lo(t.y); v[3] = h_hi(t.y);
}
template <typename T> __device__ __forceinline__ void st4(T* p, const float (&v)[4]);
template <> __device__ __forceinline__ void st4<float>(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void st4<h16_t>(h16_t* p, const float (&v)[4]) {
  uint2 t;
  t.x = f2h_pk(v[0], v[1]);
  t.y = f2h_pk(v[2], v[3]);
  *(uint2*)p = t;
}
template <typename T, int N> union Pack {
  T e[N];
  uint4 v4;
};

static inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// LDS row strides: +8 elements (16 B bf16 / 32 B f32) keeps consecutive rows on distinct 16-byte bank slots
static inline int lds_stride(int width, int esz) {
  int s = width + 8;
  if (((s * esz / 16) & 1) == 0) s += 16 / esz;  // make the stride an odd number of 16-byte slots
  return s;
}

// every element offset of the view (extent n x h x w) fits 32-bit byte arithmetic
static inline bool fits_i32(const View& v, int n, int h, int w) {
  if (!v.p) return true;
  const int64_t ext = (int64_t)n * v.sn + (int64_t)h * v.sh + (int64_t)w * v.sw + v.c;
  return ext * 2 < ((int64_t)1 << 31);
}

// the spatial tile of the tiled kernels of both units: 8 rows x 16 pixels (4 waves, each 2 rows)
#define TILE_H 8
#define TILE_W 16

// 64 bytes of zeros: DMA source for out-of-image / padding groups.  One copy per translation unit: the library is built without
// relocatable device code, and two units defining one external __device__ symbol collide at link time.  `used` keeps it a memory
// object the kernels load from, as the external symbol was: a plain static one is folded to constants and every kernel that reads it
// comes out scheduled differently (conv_ws_kernel with up to 4 more spilled SGPRs).
static __device__ __attribute__((used)) uint4 g_zero16[4];

// in-register activation of one 16-byte group
typedef short s16x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ uint4 act_group(uint4 v, int act) {
  constexpr int G = 16 / sizeof(T);
  Pack<T, G> tv;
  tv.v4 = v;
  if constexpr (sizeof(T) == 2) {
    if (act == CGEN_ACT_RELU) {
      // bf16 ReLU == signed 16-bit max(x, 0) on the raw bits (negative floats have the sign bit set): one v_pk_max_i16
      // per channel pair.  (-0.0 -> +0.0; a NaN with the sign bit set becomes 0, torch keeps it -- not reachable here)
      union { uint32_t u; s16x2 s; } c;
      uint32_t* w = (uint32_t*)&tv.v4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c.u = w[e];
        c.s = __builtin_elementwise_max(c.s, (s16x2){0, 0});
        w[e] = c.u;
      }
      return tv.v4;
    }
    if (act == CGEN_ACT_GELU) {
      return gelu8_fwd_h16(v);
    }
    return v;
  }
#pragma unroll
  for (int e = 0; e < G; ++e) tv.e[e] = Elem<T>::to(act_fwd(act, Elem<T>::ld(&tv.e[e])));
  return tv.v4;
}

// In-place activation of the 1-KiB DMA pieces this wave fetched itself (pieces wave, wave + 4, ...; one 16-byte group per lane).
// Four pieces per round: all four reads are issued before the first write -- the plain `*ptr = act(*ptr)` loop is a chain of
// LDS read -> wait -> math -> write round trips (hipcc may not move a later piece's read above an earlier piece's write: it
// cannot prove they do not alias), ~250 cycles per piece where the weight-gradient kernel's cycle stamps showed 1.3-2.4 k per
// tile in this pass.  Lanes that carry no data hold zeros (or sit in never-read padding slots): act(0) = 0, so no lane mask.
template <typename T>
__device__ __forceinline__ void act_pieces(char* buf, const int wave, const int lane, const int npieces, const int act) {
  char* base = buf + lane * 16;
  int pi = wave;
  for (; pi + 12 < npieces; pi += 16) {
    uint4* p0 = (uint4*)(base + pi * 1024);
    uint4* p1 = (uint4*)(base + (pi + 4) * 1024);
    uint4* p2 = (uint4*)(base + (pi + 8) * 1024);
    uint4* p3 = (uint4*)(base + (pi + 12) * 1024);
    const uint4 v0 = *p0, v1 = *p1, v2 = *p2, v3 = *p3;
    const uint4 r0 = act_group<T>(v0, act), r1 = act_group<T>(v1, act), r2 = act_group<T>(v2, act), r3 = act_group<T>(v3, act);
    *p0 = r0; *p1 = r1; *p2 = r2; *p3 = r3;
  }
  if (pi + 4 < npieces) {  // two left (or three: the third goes below)
    uint4* p0 = (uint4*)(base + pi * 1024);
    uint4* p1 = (uint4*)(base + (pi + 4) * 1024);
    const uint4 v0 = *p0, v1 = *p1;
    const uint4 r0 = act_group<T>(v0, act), r1 = act_group<T>(v1, act);
    *p0 = r0; *p1 = r1;
    pi += 8;
  }
  for (; pi < npieces; pi += 4) {
    uint4* p0 = (uint4*)(base + pi * 1024);
    *p0 = act_group<T>(*p0, act);
  }
}

// LDS pixel-tile layout ("row pieces"): a tile row is cut into 1-KiB pieces of `ppp` pixels x `gpr` 16-byte groups
// (gpr odd => conflict-free fragment reads).  One wave-wide DMA instruction fills one piece, so everything about a piece
// except a per-lane constant is wave-uniform: the per-tile address generation is a few SALU ops + ~6 VALU per piece.
struct PixTile {
  int gpr, ppp, ppr, rows, npx, rowbytes, bytes, pad;
  FastDiv d_gpr, d_ppr, d_ppp;
};
static inline PixTile mk_pixtile(int width_elems, int esz, int rows, int npx) {
  PixTile t;
  int gpr = (width_elems * esz + 15) / 16 + 1;
  if ((gpr & 1) == 0) ++gpr;
  t.gpr = gpr; t.ppp = 64 / gpr; t.rows = rows; t.npx = npx;
  if (t.ppp < 1) {  // pixel wider than one 1-KiB piece: caller must fall back (checks ppp < 1)
    t.ppr = 0; t.rowbytes = 0; t.bytes = 0; t.pad = 0;
    t.d_gpr = mk_fastdiv(1); t.d_ppr = mk_fastdiv(1); t.d_ppp = mk_fastdiv(1);
    return t;
  }
  t.ppr = (npx + t.ppp - 1) / t.ppp;
  t.rowbytes = t.ppr * 1024; t.bytes = rows * t.rowbytes; t.pad = 0;
  t.d_gpr = mk_fastdiv(gpr); t.d_ppr = mk_fastdiv(t.ppr); t.d_ppp = mk_fastdiv(t.ppp);
  return t;
}
// byte offset of pixel (row, x) inside a PixTile
__device__ __forceinline__ int pix_off(const PixTile& t, int row, int x) {
  const int pc = fdiv(x, t.d_ppp);
  return row * t.rowbytes + pc * 1024 + (x - pc * t.ppp) * t.gpr * 16;
}

// ---- lean row-piece DMA of one tile (shared by the persistent kernels).  Everything tile-invariant about a lane lives in
// LaneTile (built once per kernel); per piece the wave spends ~10 VALU + ~12 SALU: the piece walk (hy, pc) is scalar and
// incremental, offsets are 24-bit multiplies, the image box is given in TILE coordinates.
struct LaneTile {
  int xl;       // pixel of this lane inside a piece
  int sh, swp;  // element strides of this lane's source per tile row / per piece (ppp pixels); < 2^24 (dma_clean)
  bool lane;    // lane maps to a slot of the piece
  bool data;    // ... and the slot carries real channels
};
// `org`: this lane's source for (tile row 0, piece 0), lane pixel / channel offset included.  Rows [ry0, ry1) and columns
// [cx0, cx1) of the tile lie inside the image (and inside the tile's own pixel extent); everything else reads zeros.
// `wave` must be wave-uniform (readfirstlane).  No LDS store may sit between two DMAs (hipcc would drain vmcnt).
template <typename T>
__device__ __forceinline__ void dma_tile(const PixTile& xt, const LaneTile& L, const T* org, char* buf, int wave, int ry0, int ry1,
                                         int cx0, int cx1) {
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* gbl_ptr;
  const int npieces = xt.rows * xt.ppr;
  int hy = fdiv(wave, xt.d_ppr), pc = wave - hy * xt.ppr;
  for (int pi = wave; pi < npieces; pi += 4) {
    if (L.lane) {
      const int hx = pc * xt.ppp + L.xl;
      const bool ok = L.data && hy >= ry0 && hy < ry1 && hx >= cx0 && hx < cx1;
      const T* src = ok ? org + (int)(__umul24(hy, L.sh) + __umul24(pc, L.swp)) : (const T*)g_zero16;
      __builtin_amdgcn_global_load_lds((gbl_ptr)src, (lds_ptr)(buf + pi * 1024), 16, 0, 0);
    }
    pc += 4;
    while (pc >= xt.ppr) { pc -= xt.ppr; ++hy; }
  }
}

}  // namespace cgen
