/* cgen_hip.h -- C ABI of libcgen_hip.so: the MI355X (gfx950) kernels behind the HVAE image-mechanism /
 * counterfactual hot path of biomedia-mira/causal-gen.
 *
 * The reference has no FFI layer: its L0 is stock ATen.  Each entry point below replaces the
 * ATen op class(es) the reference dispatches at the cited src/ file:line; the host-side mirror of the
 * reference's Python surface (causal-gen_amd/vae.py, dscm.py, dmol.py) is the only caller.
 *
 * Conventions
 *   - Activations are NHWC *views*: channel stride 1, arbitrary (n,h,w) strides in ELEMENTS.  A channel slice
 *     or a [:res,:res] crop of a bigger tensor is therefore a view, and torch.cat along C is never materialised
 *     (multi-segment inputs).  dtype: CGEN_F32 (exact path: f32 MFMA 16x16x4, bit-level fmaf chains) or
 *     CGEN_F16 (IEEE binary16 storage + v_mfma_f32_16x16x32_f16 / 32x32x16_f16, f32 accumulate; activation GRADIENTS are carried
 *     times a power-of-two loss scale chosen by the caller, and the two kernels that turn them into f32 parameter gradients --
 *     cgen_wgrad_reduce via cgen_wred_desc.unscale, cgen_batch_reduce via its `unscale` argument -- multiply by its inverse).
 *     Parameters/gradients are always f32.
 *   - Ownership: the caller owns every buffer including workspaces; the library never allocates, frees or
 *     synchronises, and keeps no mutable global state (deepcopy / fork / hipGraph-capture safe).
 *   - Every call only enqueues work on `stream` and returns 0, or a negative cgen_status (message via
 *     cgen_last_error()).  Numerical NaNs are data, not errors (trainer.py:71-85 tests for them).
 *   - Thread-safe and re-entrant; cgen_last_error() is thread-local.
 */
#ifndef CGEN_HIP_H
#define CGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cgen_stream_t; /* hipStream_t */

enum cgen_status { CGEN_OK = 0, CGEN_EINVAL = -1, CGEN_ELAUNCH = -2, CGEN_EUNSUPPORTED = -3 };
enum cgen_dtype { CGEN_F32 = 0, CGEN_F16 = 1,
                  /* cgen_conv2d only (ABI 405): CGEN_F32 tensors and weight image, but the tiled kernel forms every product from
                   * SPLIT binary16 operands -- v = hi + lo, three v_mfma_f32_16x16x32_f16 per K-step (hi*hi + hi*lo + lo*hi), f32
                   * accumulate: ~2^-21 relative per product instead of binary16's 2^-11, at a fifth of the f32 MFMA's cycles.  The
                   * inference passes of the f32 engine use it (counterfactual pixels within 1e-3 of the reference, north_star);
                   * shapes the tiled kernel does not take run the exact f32 kernels.  Operands must lie inside binary16's range. */
                  CGEN_F32S = 2 };
enum cgen_act { CGEN_ACT_NONE = 0, CGEN_ACT_RELU = 1, CGEN_ACT_GELU = 2 };

/* NHWC strided view; strides in elements; p == NULL means "absent".
 * cpad (optional, 0 = none): the caller guarantees that channels [c, cpad) of every pixel are readable and hold
 * finite values (zeros); lets the tiled kernels fetch whole 16-byte groups of a ragged-width tensor by LDS-DMA.
 * On an OUTPUT view of cgen_conv2d, cpad > c asks the kernel to write zeros into channels [c, cpad) as well, so that a
 * ragged-width result (e.g. the 4-channel bottleneck of a 16-wide Block) is itself DMA-clean for its consumers. */
typedef struct cgen_view {
  void* p;
  int64_t sn, sh, sw;
  int32_t c;
  int32_t cpad;
} cgen_view;

#define CGEN_MAX_SEG 4

/* ABI version of this header.  cgen_version() of the loaded library must equal it (causal-gen_amd/_lib.py checks): struct layouts,
 * enum values and signatures are only compatible within one version.  cgen_h16_format(): the 16-bit storage format the library was
 * BUILT for -- 0 = IEEE binary16 (default), 1 = bfloat16 (-DCGEN_H16_BF16, an A/B build); CGEN_F16 tensors must be in that format. */
#define CGEN_ABI_VERSION 411
int cgen_version(void);
int cgen_h16_format(void);
const char* cgen_last_error(void);

/* ------------------------------------------------------------------ convolution (K1/K2/K3/K4/K5/K8/K9)
 * out = (bias + conv_{KSxKS, stride 1, pad KS/2}( act(cat_C(seg[0..nseg))) )) * act'(aux) + res1 + res2
 * Replaces aten::convolution (+ the gelu/relu before it, the torch.cat feeding it, the residual adds after it)
 * at vae.py:53-55,61-67,71 (Block), :104-110 (stem), :165,167 (z_proj, z_feat_proj), :176,188 (cat), :78,292-294
 * (adds), :325-333 (likelihood heads), dmol.py:223.  The SAME entry point is the data-gradient kernel:
 * seg = grad_out, weight = the "dgrad image" from cgen_weight_prep, dact/aux = the forward activation and
 * its input, res1 = out (accumulate).  res1/res2 may alias out.
 * weight: image built by cgen_weight_prep: [ceil16(Co)][krow], column k = tap * C8 + c with C8 = sum_s ceil8(C_s)
 * (segments side by side at 8-channel granularity), krow = ceil32(KS*KS*C8) + 32, in `dtype`, zero padded.
 * Remainder planes (CGEN_F16 only; 0 = absent): the residual trunk of the HVAE (vae.py:78, 253, 292-294: ~100 consecutive
 * `h = h + f(h)` updates) is carried as a PAIR of binary16 tensors, value = hi + rem with |rem| <= ulp(hi)/2, so that the sum
 * keeps ~22 significant bits although every conv still reads 16-bit operands (hi alone).  `res1_rem` / `out_rem` are BYTE
 * offsets from res1.p / out.p to a plane of identical layout: the epilogue adds res1 + res1_rem in f32, stores
 * out = rn16(v) and, when out_rem != 0, out_rem = rn16(v - out). */
typedef struct cgen_conv_args {
  int32_t dtype, n, h, w, ks, nseg, act, dact;
  cgen_view seg[CGEN_MAX_SEG];
  const void* weight;
  const float* bias; /* [Co] or NULL */
  cgen_view out;     /* out.c = Co */
  cgen_view aux, res1, res2;
  int64_t out_rem, res1_rem;
} cgen_conv_args;
int cgen_conv2d(const cgen_conv_args* a, cgen_stream_t stream);
/* Which kernel served the calling thread's last cgen_conv2d / cgen_conv2d_pair: "gen", "tile", "px", "ws", "smlp" or "smlp2" (the pair
 * launch); "" before any call.  For tests that pin the dispatch; the string is static. */
const char* cgen_conv2d_last_kernel(void);
/* Two independent convolutions in ONE launch where both are small-image problems of the same kernel instance (f16, 1x1 or 3x3, the
 * <= ~6000-pixel batches of the <= 12x12 layers: conv_smallp, whose launches are latency-bound whatever their size).  In the reference's
 * graph: the data gradients of the posterior and the prior Block's convs of a DecoderBlock (vae.py:240-301), which autograd runs back to
 * back.  Bit-identical to two cgen_conv2d calls; the caller guarantees that neither reads or accumulates into what the other writes. */
int cgen_conv2d_pair_supported(const cgen_conv_args* a, const cgen_conv_args* b);
int cgen_conv2d_pair(const cgen_conv_args* a, const cgen_conv_args* b, cgen_stream_t stream);

/* ------------------------------------------------------------------ fused "light" Block (csrc/block.hip; binary16)
 * Block.forward with version == "light" (vae.py:49-56, 60-71, 73-84) as ONE launch, the bottleneck tensor resident in LDS:
 *   pre_act = 1 (forward):   mid = bias_a + conv3x3(relu(cat_C(seg)))          (pre-activation bottleneck, interior pixels written once)
 *                            o[k].out = o[k].bias + conv3x3(relu(mid)) + o[k].res1
 *   pre_act = 0 (data gradient: aten::convolution_backward x2 + threshold_backward x2, the input part; mid_aux = the forward `mid`):
 *                            mid = conv3x3(seg[0] = grad_out; w_a = fragment image of conv2's dgrad) * relu'(mid_aux)
 *                            o[k].out = conv3x3(mid; o[k].w = fragment image of conv1's dgrad w.r.t. segment k) * relu'(o[k].aux) + o[k].res1
 * nout = 2 serves a Block with two differentiable input segments (the posterior Block: h and the encoder activation).
 * Weight images are FRAGMENT-ORDERED (one contiguous KiB per wave load), built by cgen_weight_prep modes 2-5:
 *   w_a   [sum_s ceil(seg[s].c / 32) chunks][18 K16-steps kk: channel half kk / 9 (channels 16 (kk / 9) .. + 16), tap = kk % 9][64 lanes][8]
 *         (every segment occupies whole 32-channel chunks of the K axis, zero padded; a wave's nine fragments are contiguous)
 *   o[].w [ceil(Co / 32) pairs][ceil(9 b / 16) K16-steps over k = tap * b + c][64 lanes][8]
 *   lane l of a fragment holds row (l & 31) -> channel 16 ((r >> 2) & 1) + (r & 3) + 4 (r >> 3) of the 32-row block, k = 8 (l >> 5) .. + 8.
 * Served: mid.c in {8, 16, 24, 32}, out.c a multiple of 8, up to 3 input segments (each DMA-clean: channels a multiple of 8 or
 * zero padded, cgen_view.cpad), 16-byte aligned views below 2^31 bytes; cgen_block3_supported() answers without launching. */
typedef struct cgen_block3_out {
  const void* w;
  const float* bias;
  cgen_view out, aux, res1;
  int64_t out_rem, res1_rem; /* remainder planes of a residual trunk, as in cgen_conv_args (byte offsets from out.p / res1.p, 0 = none) */
} cgen_block3_out;
typedef struct cgen_block3_args {
  int32_t dtype, n, h, w, nseg, nout, pre_act, reserved;
  cgen_view seg[CGEN_MAX_SEG];
  const void* w_a;
  const float* bias_a;
  cgen_view mid, mid_aux;
  cgen_block3_out o[2];
  const void* w_a16; /* optional (NULL: absent): the first conv's weights as the 16-row image of cgen_weight_prep modes 6 / 7, which the
                      * row-streaming instance (wide images, one input segment of 32 or 64 channels, bottleneck <= 16: the 96x96 and
                      * 192x192 Blocks) reads; without it those shapes run on the tile instance */
  /* The encoder's DOWN Block (vae.py:70-84: out = width_proj(x) + conv(x), then avg_pool2d(out, 2)) in the same launch.  Fields added at
   * the end (additive in ABI 411: every caller zero-initialises the struct); NULL / 0 = the behaviour above.  Row-streaming instance only:
   * with any of them set, cgen_block3_supported answers 0 for everything else (odd H or W, a float down-rate, remainder planes, other
   * widths) and the caller runs the separate launches.
   *   pre_act = 1: w_proj = the FORWARD image (cgen_weight_prep mode 0, row stride proj_krow elements) of a 1x1 conv over the RAW seg[0]
   *                (no ReLU), bias_proj its bias; pool = 2 (required with w_proj).  o[0].res1 must be absent; o[0].out is the POOLED tensor
   *                (n, h / 2, w / 2, Co):  out = avg2x2( rn16( conv3x3(relu(mid)) + bias + rn16(w_proj . seg[0] + bias_proj) ) ), the four
   *                values summed in f32 in the order (0,0) (0,1) (1,0) (1,1) like cgen_avgpool_fwd.  Neither the projected residual nor the
   *                un-pooled output is written.
   *   pre_act = 0: w_proj = the DATA-GRADIENT image (mode 1) of that 1x1 conv, pool = 0:
   *                o[0].out = rn16(conv3x3(mid) * relu'(o[0].aux) + o[0].res1) + w_proj^T . seg[0]   (seg[0] = grad_out at the centre pixel)
   * The 1x1 sums are formed as cgen_conv2d's pixel kernel forms them (v_mfma_f32_16x16x32, 32 channels per step, bias first): on the
   * image sizes that kernel serves (more than 6 000 pixels) the results have the bits of the three launches each way. */
  const void* w_proj;
  const float* bias_proj;
  int32_t proj_krow, pool;
} cgen_block3_args;
int cgen_block3_supported(const cgen_block3_args* a);
int cgen_block3(const cgen_block3_args* a, cgen_stream_t stream);
/* The plan of the single launch (additive in ABI 411: a new symbol).  Host code: no GPU needed.  Returns what cgen_block3_supported
 * returns; when that is non-zero and out != NULL, out[0 .. 23] is the record cgen_block3 launches from (entries not named are 0):
 *   [0] kind: 0 = tile kernel blk3_kernel<PRE, NB, NPG, SM, TH, REM>, 1 = small-image kernel blk3s_kernel<PRE>,
 *             2 = row-streaming kernel blk3r_kernel<PRE, NCH, NB, RES, PROJ, NR>
 *   [1] PRE   [2 .. 6] the template arguments after PRE: tile NB, NPG, SM, TH, REM; rows NCH, NB, RES, PROJ, NR; small: none
 *   [7] ring slots ns, [8] wb_persist (tile)   [9] workgroups   [10] tiles / strips of the launch
 *   [11] s_rows, [12] s_strips, [13] s_nmb (small)   [14] r_rs, [15] r_sx, [16] r_sy, [17] r_res_tile (rows)   [18] LDS bytes */
#define CGEN_BLOCK3_PLAN_INTS 24
int cgen_block3_plan(const cgen_block3_args* a, int32_t* out);
/* Two independent DATA-GRADIENT problems (pre_act = 0) in ONE launch: the backward of a decoder layer's posterior and prior Blocks
 * (vae.py:240-301: both hang off the layer's reparameterisation, neither reads what the other writes).  Each is 100-400 workgroups on
 * 512 resident slots; one launch runs them side by side without a second queue.  Served when both plan to the same kernel instance
 * (same bottleneck width, same widest-output class, no streaming mode, no remainder planes): ask _supported first.  The caller
 * guarantees that neither problem reads or accumulates into a tensor the other one writes. */
int cgen_block3_pair_supported(const cgen_block3_args* a, const cgen_block3_args* b);
int cgen_block3_pair(const cgen_block3_args* a, const cgen_block3_args* b, cgen_stream_t stream);
/* The same entry points take two FORWARD problems (pre_act = 1 on both): a decoder layer's posterior Block (a) and prior Block (b),
 * which today run on two queues.  The two may plan to different kernel instances; the launch runs instance A on the first `na`
 * workgroups and instance B on the rest, each the body of the single launch on its record, so the results have the single launches'
 * bits.  Declined (0, nothing launched): one record pre_act and the other not; different image size or batch; different bottleneck
 * width; a streaming or row-streaming instance, remainder planes or a residual on either record; a combination of instances that
 * is not compiled (csrc/block.hip, b3_fwd_pair_served).
 * cgen_block3_pair_plan: what _supported answers, and when that is 1 the plan in out[0 .. 7] = bottleneck / 8, small-image instance
 * (0 / 1), then per record the phase-B wave split, the tile rows and the workgroups.  Host code: no GPU needed. */
int cgen_block3_pair_plan(const cgen_block3_args* a, const cgen_block3_args* b, int32_t* out);

/* ------------------------------------------------------------------ fused DEFAULT Block (csrc/block4.hip; binary16)
 * Block.forward of the non-"light" version (vae.py:57-71, 73-84: GELU -> 1x1 -> GELU -> 3x3 -> GELU -> 3x3 -> GELU -> 1x1) as ONE launch,
 * the three bottleneck tensors' activated tiles resident in LDS:
 *   fwd = 1:  mid[0] = bias[0] + conv1x1(gelu(cat_C(seg)); w[0]),  mid[1] = bias[1] + conv3x3(gelu(mid[0]); w[1]),
 *             mid[2] = bias[2] + conv3x3(gelu(mid[1]); w[2]),       o[0].out = o[0].bias + conv1x1(gelu(mid[2]); o[0].w) + o[0].res1
 *             (mid[]: pre-activations, written once -- the weight gradients and the backward pass read them; mid_aux absent)
 *   fwd = 0 (data gradient: aten::convolution_backward x4 + gelu_backward x4, the input part; seg[0] = grad_out, nseg = 1;
 *             mid_aux[0..2] = the forward mid[2], mid[1], mid[0]):
 *             mid[0] = conv1x1(seg[0]; w[0] = image of the last conv's transpose) * gelu'(mid_aux[0])       (gradient w.r.t. forward mid[2])
 *             mid[1] = conv3x3(mid[0]; w[1] = flipped transpose of the second 3x3) * gelu'(mid_aux[1])      (... forward mid[1])
 *             mid[2] = conv3x3(mid[1]; w[2] = flipped transpose of the first 3x3) * gelu'(mid_aux[2])       (... forward mid[0])
 *             o[k].out = conv1x1(mid[2]; o[k].w = transpose of the first conv w.r.t. segment k) * gelu'(o[k].aux) + o[k].res1
 *             for up to three differentiable input segments (the posterior Block: h and the encoder activation).
 * Weight images are FRAGMENT-ORDERED (1 KiB = one v_mfma_f32_32x32x16 A operand: lane l holds fragment row r = l & 31, k-group kg = l >> 5),
 * built by cgen_weight_prep modes 8-13; G = ceil(b / 16).  Row permutation, with kr = (r >> 2) & 1 and j = (r & 3) + 4 (r >> 3):
 * o[].w rows carry channel 16 kr + j of their 32-row block (a lane of the accumulator tile ends up with 16 consecutive channels);
 * w[0..2] rows carry channel HW kr + j for j < HW (zero rows otherwise), HW = half of the block's channels after rounding b up to 8
 * (4, 8, 12 or 16): every lane of the post-operation works on real channels whatever the bottleneck width.
 *   w[0]        [ceil(b / 32) row blocks][sum_s ceil(seg[s].c / 32) chunks][2 steps][64 lanes][8]: lane (row, kg), step s, element e
 *               multiplies input channel 32 chunk + 16 s + 8 kg + e (segments in whole chunks, zero padded)
 *   w[1], w[2]  [ceil(b / 32)][9 taps][G][64][8]: k = 16 g + 8 kg + e
 *   o[].w       [ceil(Co / 32)][G][64][8]
 * Served: b <= 48 or 57..64, up to 3 input segments, output widths multiples of 8 (<= 256 forward), every view 16-byte aligned, below 2^31
 * bytes, ragged channel counts zero padded to 8 (cgen_view.cpad); any image size (8 x 16 output tiles).  mid[k].c = mid_aux[k].c = b. */
typedef struct cgen_block4_args {
  int32_t dtype, n, h, w, nseg, nout, fwd, b;
  cgen_view seg[CGEN_MAX_SEG];
  const void* wimg[3]; /* w[0..2] below */
  const float* bias[3];
  cgen_view mid[3], mid_aux[3];
  cgen_block3_out o[3];
} cgen_block4_args;
int cgen_block4_supported(const cgen_block4_args* a);
int cgen_block4(const cgen_block4_args* a, cgen_stream_t stream);
/* The plan of the launch (additive in ABI 411: a new symbol).  Host code: no GPU needed, nothing is dereferenced.  Returns what
 * cgen_block4_supported returns; when that is 1 and out != NULL, out[0 .. 15] is the record cgen_block4 launches from (entries not
 * named are 0):  [0] fwd   [1] NB8 (8-channel groups of the bottleneck: 1 .. 6, or 8 for 57 .. 64 channels)   [2] waves per workgroup
 * (4 or 8)   [3] tiles   [4] workgroups   [5] LDS bytes   [6] xcd_order   [7] tiles_x   [8] tiles_y   [9] phase-0 chunks (nch0):
 * the kernel is blk4_kernel<fwd, NB8, waves>.  cgen_block4_pair_plan: what _pair_supported answers, and blk4_pair_kernel<NB8>'s
 * launch in [1] NB8, [2] = 4, [3] tiles of a, [4] workgroups, [5] LDS bytes, [6] tiles of b. */
#define CGEN_BLOCK4_PLAN_INTS 16
int cgen_block4_plan(const cgen_block4_args* a, int32_t* out);
/* Two independent DATA-GRADIENT problems (fwd = 0) of the same bottleneck class (ceil(b / 8) equal) in ONE launch: the backward of a
 * decoder layer's posterior and prior Blocks (vae.py:240-301).  Bit-identical to two cgen_block4 calls; the caller guarantees that
 * neither problem reads or accumulates into a tensor the other one writes. */
int cgen_block4_pair_supported(const cgen_block4_args* a, const cgen_block4_args* b);
int cgen_block4_pair(const cgen_block4_args* a, const cgen_block4_args* b, cgen_stream_t stream);
int cgen_block4_pair_plan(const cgen_block4_args* a, const cgen_block4_args* b, int32_t* out);

/* Weight gradient (aten::convolution_backward, weight/bias part) as split-K partials:
 *   partial_w[split][Co][KS*KS][Ci_total] (f32), partial_b[split][Co] (f32, may be NULL)
 * with Ci_total = sum_s seg[s].c and nsplit = cgen_conv2d_wgrad_plan(args) (call it with the views filled in).  *tiled_out says
 * which kernel will serve the call and in which layout it leaves partial_w: 0 = generic kernel, 1 = tiled 16-bit (CGEN_F16) kernel,
 * 2 = streaming kernel of round 5 (csrc/wgrad3.hip) -- all three the layout above --, 3 = streaming kernel with grad_out as its
 * shifted operand: partial_w[split][Ci_total][KS*KS - 1 - tap][Co] (pass cgen_wred_desc.layout = 1 to cgen_wgrad_reduce).
 * Deterministic: partials are summed in a fixed order by cgen_wgrad_reduce. */
typedef struct cgen_wgrad_args {
  int32_t dtype, n, h, w, ks, nseg, act, nsplit;
  cgen_view seg[CGEN_MAX_SEG];
  cgen_view gout; /* gout.c = Co */
  float* partial_w;
  float* partial_b;
} cgen_wgrad_args;
int cgen_conv2d_wgrad_plan(const cgen_wgrad_args* a, int32_t* tiled_out);
/* The plan of the launch (additive in ABI 411: a new symbol).  Host code: no GPU needed, nothing is dereferenced.  Returns what
 * cgen_conv2d_wgrad_plan returns (nsplit; 0: bad args, out[] untouched); when out != NULL, out[0 .. 23] is the record
 * cgen_conv2d_wgrad launches from (entries not named are 0):  [0] kind (*tiled_out above)   [1] nsplit, and
 *   kind 0, wgrad_kernel<T, NTC>:  [2] dtype (CGEN_F32 / CGEN_F16)   [3] NTC (1, 2, 4: 16 NTC output channels per workgroup)   [4] 32-wide
 *     input-channel chunks, all segments   [5] tap groups of up to 9 taps   [6] pixels per split   [7] gout_vec (grad_out read four
 *     elements at a time)   [8] bit s: segment s is read 16 bytes at a time   [9] 1: partial_b is written
 *   kind 1, wgrad_tile_kernel<NCF, NJW, KS>:  [2] NCF   [3] NJW   [4] KS   [5] cwin (input channels per window)   [6] windows   [7] blocks
 *     of 16 NCF output channels   [8] 8 x 16 pixel tiles   [9] tiles per split   [10] 1: two tile buffers   [11] LDS bytes
 *     [12] variant, as wgrad_tile_mega_kernel switches on it
 *   kinds 2, 3: nothing more. */
#define CGEN_WGRAD_PLAN_INTS 24
int cgen_conv2d_wgrad_plan_record(const cgen_wgrad_args* a, int32_t* out);
/* Horizontally batched weight gradients.  The weight-gradient launches of a step are independent of each other; most of
 * them fill a fraction of the chip.  `plan` packs every problem the tiled 16-bit (CGEN_F16) kernel serves (eligible[i] = 1; the others
 * go through cgen_conv2d_wgrad) into a host blob: a table of problems followed by one {problem, split, window, co range}
 * record per workgroup, and describes one launch per kernel variant.  Call it with blob_host = NULL to get the sizes.
 * The caller copies the blob to the device ONCE (addresses are stable across steps: the arena is deterministic) and
 * `run` then issues n_launches kernels instead of `count`.  nsplit / partial buffers exactly as cgen_conv2d_wgrad.
 * max_workgroups > 0 caps each launch's grid (a resident set of workgroups walks the records): a batch issued on a side
 * stream in the background of the backward chain must leave CUs free for the chain's kernels; 0 = one workgroup per record. */
typedef struct {
  int32_t ncf, ks, lds_bytes, nblocks;
  int64_t blocks_offset; /* byte offset of this launch's workgroup records inside the blob */
} cgen_wgrad_batch_launch;
int cgen_conv2d_wgrad_batch_plan(const cgen_wgrad_args* args, int32_t count, void* blob_host, int64_t capacity, int64_t* blob_bytes,
                                 cgen_wgrad_batch_launch* launches, int32_t max_launches, int32_t* n_launches, int32_t* eligible);
int cgen_conv2d_wgrad_batch_run(const void* blob_dev, const cgen_wgrad_batch_launch* launches, int32_t n_launches, int32_t max_workgroups,
                               cgen_stream_t);
int cgen_conv2d_wgrad(const cgen_wgrad_args* a, cgen_stream_t stream);

/* Multi-tensor descriptor tables (device memory, built once by the host).  One launch serves every conv site. */
typedef struct cgen_wprep_desc { /* OIHW f32 parameter -> forward image or dgrad image */
  const float* src;
  void* dst;
  int32_t co, ci_total, ks, mode; /* mode 0: fwd image, 1: dgrad image of segment [seg_off, seg_off+seg_c[0]);
                                   * fragment-ordered images of cgen_block3 (src is always the OIHW parameter [co][ci_total][3][3]):
                                   * (1 KiB fragments in v_mfma_f32_32x32x16 A-operand lane order; phase-A images [chunk][channel half][tap])
                                   * 2: w_a of the forward pass (conv1: rows = co, K = the segments' channels),
                                   * 3: w_a of the data gradient (conv2: rows = ci_total, K = co, taps flipped),
                                   * 4: o[].w of the forward pass (conv2: rows = co, K = tap * ci_total + c; k_pad = K16-steps per pair),
                                   * 5: o[].w of the data gradient w.r.t. segment [seg_off, seg_off + seg_c[0]) (conv1: rows = the
                                   *    segment's channels, K = tap * co + c, taps flipped; k_pad = K16-steps per pair)
                                   * 6 / 7: w_a16 of the forward pass / the data gradient -- 1 KiB fragments in v_mfma_f32_16x16x32 A-operand lane
                                   *    order, [tap 0..8][32-channel chunk q][64 lanes][8]: lane l holds row (l & 15) (bottleneck channel, <= 16),
                                   *    k = 32 q + 8 (l >> 4) .. + 8 (6: conv1's input channel; 7: conv2's output channel, taps flipped)
                                   * 8-13: images of cgen_block4 (layouts there): 8 / 9 = w[0] forward (src = the first 1x1 [b][ci_total]; k_pad = 2 x chunks)
                                   *    / data gradient (src = the last 1x1 [co][b]: rows = ci_total, K = co), 10 / 11 = a 3x3 forward / flipped
                                   *    transpose (k_pad = G), 12 = o[].w forward (src = the last 1x1), 13 = o[].w of the data gradient w.r.t. segment
                                   *    [seg_off, seg_off + seg_c[0]) (src = the first 1x1; k_pad = G) */
  int32_t nseg, seg_off;
  int32_t seg_c[CGEN_MAX_SEG];
  int32_t dtype, rows_pad, k_pad, reserved; /* k_pad = krow of the image */
  int64_t numel; /* rows_pad * k_pad */
} cgen_wprep_desc;
int cgen_weight_prep(const cgen_wprep_desc* descs_dev, const int32_t* chunk_site_dev, const int32_t* chunk_index_dev,
                     int32_t nchunks, cgen_stream_t stream);

typedef struct cgen_wred_desc { /* split-K partials -> OIHW f32 gradient (+bias gradient) */
  const float* partial_w;
  const float* partial_b;
  float* grad_w; /* [Co][Ci][KS][KS] */
  float* grad_b; /* [Co] or NULL */
  int32_t co, ci_total, ks, nsplit;
  int32_t accumulate;
  float unscale; /* the sums are multiplied by this (1 / loss scale of the f16 engine); 0 means 1 */
  int32_t layout; /* of partial_w, as reported by cgen_conv2d_wgrad_plan: 0 = [split][Co][tap][Ci], 1 = [split][Ci][KS*KS-1-tap][Co] */
  int32_t reserved;
  int64_t numel; /* co*ci_total*ks*ks + co */
} cgen_wred_desc;
int cgen_wgrad_reduce(const cgen_wred_desc* descs_dev, const int32_t* chunk_site_dev, const int32_t* chunk_index_dev,
                      int32_t nchunks, cgen_stream_t stream);

/* The per-element kernels of the two launches above under names of their own (same tables): they define the image layouts and the
 * order of the sums, and what replaces them is tested against them byte for byte (additive in ABI 411: new symbols only). */
int cgen_weight_prep_ref(const cgen_wprep_desc* descs_dev, const int32_t* chunk_site_dev, const int32_t* chunk_index_dev,
                         int32_t nchunks, cgen_stream_t stream);

/* cgen_wgrad_reduce, tiled (csrc/multitensor.hip; additive in ABI 411: one new struct, new symbols).  One workgroup: a TILE of a
 * site's partials, rows [a0, a0 + na) x every tap, columns [b0, b0 + nb) of the partial layout (layout 0: a = Co, b = Ci, inner = Ci_total; layout 1: a = Ci, b = Co, inner = Co), at most 2048 elements (1024 for a site with more than four splits on the 16-byte path), or
 * (kind 1) the bias gradient of channels [b0, b0 + nb).  The four split chains of cgen_wgrad_reduce go to different lanes and are
 * combined in its order; the sums leave LDS as contiguous runs of the OIHW gradient (nb * taps floats in layout 0, na * taps in layout 1). */
typedef struct cgen_wred_item {
  const float* partial; /* the site's partial_w (kind 0) or partial_b (kind 1) */
  float* grad;          /* the site's grad_w or grad_b */
  int32_t kind, nsplit;
  int32_t split_stride; /* elements between two splits: Co * Ci_total * KS * KS, or Co for the bias */
  int32_t vec;          /* 1: the site takes cgen_wgrad_reduce's 16-byte path (four chains); 0: plain split order */
  int32_t v4;           /* 1: 16-byte loads are possible (inner, b0, nb, split_stride multiples of 4, partial 16-byte aligned) */
  int32_t accumulate;
  float unscale;
  int32_t taps, inner, ci_total, layout;
  int32_t a0, na, b0, nb;
  int32_t reserved;
} cgen_wred_item;
int cgen_wgrad_reduce_tiles(const cgen_wred_item* items_dev, int32_t nitems, cgen_stream_t stream);
int cgen_wgrad_reduce_ref(const cgen_wred_desc* descs_dev, const int32_t* chunk_site_dev, const int32_t* chunk_index_dev,
                          int32_t nchunks, cgen_stream_t stream);

/* ------------------------------------------------------------------ element-wise / data movement
 * aten::avg_pool2d fwd/bwd (vae.py:79-83), upsample_nearest2d (+ learned per-res bias, vae.py:251-262),
 * F.pad / slicing / clone (vae.py:131-133, 241), repeat of bias[1] (vae.py:233), pa_sto scaling (vae.py:244-247),
 * layout + u8->[-1,1] preprocessing (trainer.py:16-21). */
int cgen_avgpool_fwd(int32_t dtype, int32_t n, int32_t ho, int32_t wo, int32_t d, cgen_view in, cgen_view out, cgen_stream_t);
int cgen_avgpool_bwd(int32_t dtype, int32_t n, int32_t ho, int32_t wo, int32_t d, cgen_view gout, cgen_view gin,
                     int32_t accumulate, cgen_stream_t);
/* aten::adaptive_avg_pool2d fwd/bwd for a Block with a float down-rate (vae.py:79-81): output cell o averages
 * [floor(o*in/out), ceil((o+1)*in/out)) along each axis; the backward pass gathers gout / window area. */
int cgen_adaptive_avgpool_fwd(int32_t dtype, int32_t n, int32_t hi, int32_t wi, int32_t ho, int32_t wo, cgen_view in, cgen_view out,
                              cgen_stream_t);
int cgen_adaptive_avgpool_bwd(int32_t dtype, int32_t n, int32_t hi, int32_t wi, int32_t ho, int32_t wo, cgen_view gout, cgen_view gin,
                              int32_t accumulate, cgen_stream_t);
/* out[n,y,x,:] = in[n, floor(y*hi/ho), floor(x*wi/wo), :] + (bias ? bias[y,x,:] : 0); bias is f32 [ho][wo][C] */
int cgen_upsample_fwd(int32_t dtype, int32_t n, int32_t hi, int32_t wi, int32_t ho, int32_t wo, cgen_view in,
                      const float* bias, cgen_view out, cgen_stream_t);
int cgen_upsample_bwd(int32_t dtype, int32_t n, int32_t hi, int32_t wi, int32_t ho, int32_t wo, cgen_view gout,
                      cgen_view gin, int32_t accumulate, cgen_stream_t);
/* out[y,x,c] (+)= unscale * sum_n in[n,y,x,c]  (gradient of a batch-broadcast parameter); out f32 contiguous [h][w][C];
 * unscale = 1 / loss scale of the engine whose 16-bit gradients `in` holds (1 for f32) */
int cgen_batch_reduce(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view in, float* out, int32_t accumulate,
                      float unscale, cgen_stream_t);
/* out[n,y,x,c] = src[y,x,c] (batch broadcast of an f32 [h][w][C] parameter) */
int cgen_batch_broadcast(int32_t dtype, int32_t n, int32_t h, int32_t w, const float* src, cgen_view out, cgen_stream_t);
/* out = alpha*in (+ out if accumulate); channels >= c_from additionally scaled by beta.  in may be absent (fill alpha). */
int cgen_axpby(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view in, cgen_view out, float alpha, float beta,
               int32_t c_from, int32_t accumulate, cgen_stream_t);
/* NCHW (f32 or u8, contiguous) -> NHWC view in `dtype`: out = (in - sub) * mul */
int cgen_nchw_to_nhwc(int32_t src_is_u8, int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w, const void* src,
                      cgen_view out, float sub, float mul, cgen_stream_t);
/* Direct 7x7 stem conv, forward (vae.py:104-110,126: Encoder.stem, Cin 1..4, Cout 16 / 32 / 64): halo tile and the whole
 * weight matrix in LDS, one output pixel x all Cout per thread; weight_oihw / bias are the f32 parameters themselves (the 16-bit
 * engine rounds the weights to the 16-bit storage format on load).  No patch tensor on the forward path; cgen_im2col + the 1x1 weight-gradient
 * kernels remain the backward route. */
int cgen_stem_conv_supported(int32_t dtype, int32_t cin, int32_t ks, int32_t co);
int cgen_stem_conv_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t ks, int32_t co, cgen_view in,
                       const float* weight_oihw, const float* bias, cgen_view out, cgen_stream_t);
/* im2col for the thin-K stem conv (vae.py:104-110): out[n,y,x, c*ks*ks + tap] = in[n, y+dy, x+dx, c], zeros outside the
 * image and in out's padding channels (out.c = in.c*ks*ks, out.cpad = ceil8(out.c)).  The 7x7 stem then runs as a 1x1
 * conv over 49*Ci channels on the MFMA kernels, with the OIHW weight used as the [Co][49*Ci] matrix unchanged. */
int cgen_im2col(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ks, cgen_view in, cgen_view out, cgen_stream_t);
/* General im2col / col2im (config 1, simple_vae.py:38-49: the 5x5/s2/p1 and 3x3/s2/p1 convolutions run as im2col + a
 * 1x1 conv with the OIHW weight used as the [Co][Ci*ks*ks] matrix).  out[n,oy,ox, c*ks*ks + tap] =
 * in[n, oy*stride - pad + dy, ox*stride - pad + dx, c] (zeros outside; channels [out.c, out.cpad) zeroed);
 * col2im is its transpose: gin (+)= scatter of gcol. */
int cgen_im2col_strided(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ks, int32_t stride, int32_t pad, int32_t ho,
                        int32_t wo, cgen_view in, cgen_view out, cgen_stream_t);
int cgen_col2im_strided(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ks, int32_t stride, int32_t pad, int32_t ho,
                        int32_t wo, cgen_view gcol, cgen_view gin, int32_t accumulate, cgen_stream_t);
/* Stand-alone unary ops where an activation cannot be fused into a consumer (simple_vae.py:13 LeakyReLU applied to one
 * segment of a concatenation only; .clamp(min=EPS) on log-scales, :68,97): op = CGEN_ACT_* or CGEN_UNARY_*;
 * bwd: gin (+)= gout * f'(x) */
#define CGEN_UNARY_LEAKY_RELU 3 /* param = negative slope */
#define CGEN_UNARY_CLAMP_MIN 4  /* param = minimum; gradient passes where x >= min */
#define CGEN_UNARY_ADD 5        /* x + param (temperature: logscale + log t) */
int cgen_unary_fwd(int32_t dtype, int32_t op, float param, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view in, cgen_view out,
                   cgen_stream_t);
int cgen_unary_bwd(int32_t dtype, int32_t op, float param, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view x, cgen_view gout,
                   cgen_view gin, int32_t accumulate, cgen_stream_t);
/* NHWC view -> contiguous NCHW f32 */
int cgen_nhwc_to_nchw(int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w, cgen_view in, float* dst, cgen_stream_t);

/* ------------------------------------------------------------------ device-resident input pipeline (ABI 411; csrc/augment.hip)
 * One launch builds an augmented training batch from a data set that lives on the device as u8: row gather, zero-padded random
 * crop, horizontal flip, (v - sub) * mul and the NCHW -> NHWC layout change, written in `dtype`; the parents of the same rows are
 * gathered on the side.  Replaces the reference's per-sample PIL transforms (src/datasets.py: RandomCrop(input_res, padding) +
 * RandomHorizontalFlip(p), Pad(2) for evaluation), the host-to-device copy and trainer.py:16-21.
 *   oy uniform on [0, h0 + 2 pad_y - r_h], ox uniform on [0, w0 + 2 pad_x - r_w]: __umulhi(bits, range + 1) of words 0 / 1 of
 *   Philox(seed, offset, stream_id, idx = index[b]) -- keyed by the DATA SET ROW, so a row's crop at a given state depends neither on
 *   its batch position nor on the data-parallel rank that holds it; flip = u01(word 2) < hflip_p (hflip_p = 1 always flips).
 *   out[b, y, x, ch] = (v - sub) * mul, sx = flip ? r_w - 1 - x : x, iy = oy + y - pad_y, ix = ox + sx - pad_x,
 *   v = data[index[b], ch, iy, ix] inside the image and 0 outside (u8 padding BEFORE normalisation; crop, then flip: torchvision's order).
 * The launch reads the Philox state and never advances it.  Addressing into `data` is 64-bit.  A row with index[b] outside
 * [0, n_data) is never read through: its image is all padding value, its pa_out row zero, its draws_out row (-1, -1, -1).
 * out: cpad > c asks for zeros in channels [c, cpad) as on cgen_conv2d's output view.  16-byte stores wherever the view allows.
 * Capturable: no allocation, no synchronisation, one stream. */
typedef struct cgen_augment_args {
  int32_t dtype;           /* CGEN_F32 or CGEN_F16 (the 16-bit storage format) */
  int32_t n, c, h0, w0;    /* batch size; data set images [n_data, c, h0, w0], c in 1..4 */
  int32_t r_h, r_w;        /* crop (= output) size */
  int32_t pad_x, pad_y;    /* virtual zero padding left/right and top/bottom */
  int32_t ctx;             /* parents per row (with pa_data / pa_out) */
  uint32_t stream_id;      /* Philox stream: no other kernel of a step may use it (the engine passes 980, csrc/common.h) */
  float hflip_p, sub, mul;
  int64_t n_data;
  const void* data;        /* u8 NCHW contiguous */
  const int64_t* index;    /* device int64[n] */
  cgen_view out;           /* NHWC [n, r_h, r_w, c] */
  const uint64_t* rng;     /* device {seed, offset}; may be NULL when draws_in is given */
  const int32_t* draws_in; /* optional device int32[n][3] = (oy, ox, flip): overrides the draws */
  int32_t* draws_out;      /* optional, same shape: the draws used */
  const float* pa_data;    /* optional f32 [n_data][ctx] ... */
  float* pa_out;           /* ... gathered into f32 [n][ctx] */
} cgen_augment_args;
int cgen_batch_augment(const cgen_augment_args* a, cgen_stream_t stream);
/* Which store arm cgen_batch_augment takes for these arguments, without launching (negative cgen_status when they are invalid):
 * 0 = contiguous rows, all 16-byte stores; 1 = contiguous rows, 16-byte stores + element-wise row end; 2 = contiguous rows, element-wise
 * (unaligned view); 3 = one pixel per lane, 16-byte stores (padded pixel stride); 4 = one pixel per lane, element-wise. */
int cgen_batch_augment_arm(const cgen_augment_args* a);
/* The same batch in PLANAR layout (additive in ABI 411): out.p is a contiguous f32 [n, c, r_h, r_w], what the anticausal predictors
 * read (the second transforms.ToTensor-shaped copy the reference's sup_epoch feeds them).  Same arguments, same draws from the same
 * Philox state and the same per-pixel arithmetic as cgen_batch_augment, so the two outputs hold the same values bit for bit.
 * dtype must be CGEN_F32 and the view must say what the memory is: out.c = c, out.sn = c * r_h * r_w, out.sh = r_w, out.sw = 1,
 * no channel padding.  (For c == 1 the NHWC launch writes this very memory.) */
int cgen_batch_augment_planar(const cgen_augment_args* a, cgen_stream_t stream);

/* ------------------------------------------------------------------ latent layer (K10, K16)
 * Fused sample_gaussian + gaussian_kl (vae.py:14-30, 268-269):
 *   z = q_loc + exp(q_ls + logt) * eps ; kl = -.5 + p - q + .5 (e^{2q} + (q_loc-p_loc)^2) e^{-2p}  (p = p_ls+logt, q = q_ls+logt)
 * eps: explicit tensor (parity runs) or NULL => Philox4x32-10 + Box-Muller keyed by rng[0]=seed, rng[1]=offset
 * (device memory, so a captured graph replays fresh noise) and `stream_id`; eps_out (optional) receives it.
 * kl_part[b*kl_stride + chunk] = per-sample partial sums (deterministic two-stage reduction), chunk <
 * cgen_reparam_kl_chunks(h,w,c); the caller lays all layers' chunks of one sample side by side (kl_stride = total). */
int cgen_reparam_kl_chunks(int32_t h, int32_t w, int32_t c);
int cgen_reparam_kl_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view q_loc, cgen_view q_ls,
                        cgen_view p_loc, cgen_view p_ls, cgen_view eps_in, const uint64_t* rng, uint32_t stream_id,
                        float logt, cgen_view z, cgen_view eps_out, float* kl_part, int32_t kl_stride, cgen_stream_t);
/* Backward: gz = d/dz (view, may be absent), kl_coef_dev[b*coef_stride] = d elbo / d kl_sum[b] (device, f32;
 * coef_stride 0 broadcasts one value).  dz/dq_ls = e^{q_ls} eps is taken as (z - q_loc), so eps is not needed.
 * Writes (or accumulates into) the four gradients. */
int cgen_reparam_kl_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view q_loc, cgen_view q_ls,
                        cgen_view p_loc, cgen_view p_ls, cgen_view z, float logt, cgen_view gz,
                        const float* kl_coef_dev, int32_t coef_stride, const float* kl_chan_scale, cgen_view g_q_loc,
                        cgen_view g_q_ls, cgen_view g_p_loc, cgen_view g_p_ls, int32_t acc_q, int32_t acc_p, cgen_stream_t);
/* The same launch carrying a RIDER: extra workgroups copy (ride_acc = 0) or accumulate (1) the [n,h,w,ride_src.c] view
 * ride_src into ride_dst.  In the decoder block  h = z_proj(z, pa) + h + p_feat  (vae.py:279-287) the gradient of the
 * residual p_feat -- a channel slice of the prior Block's output -- is the gradient of h verbatim; it has to land in the
 * prior output's gradient buffer next to the g_p_loc / g_p_ls this kernel writes, and used to be a launch of its own per
 * decoder block.  CGEN_F16 (16-bit storage), every view 16-byte aligned with channel counts in multiples of 8 (CGEN_EINVAL otherwise). */
int cgen_reparam_kl_bwd_rider(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view q_loc, cgen_view q_ls,
                              cgen_view p_loc, cgen_view p_ls, cgen_view z, float logt, cgen_view gz,
                              const float* kl_coef_dev, int32_t coef_stride, const float* kl_chan_scale, cgen_view g_q_loc,
                              cgen_view g_q_ls, cgen_view g_p_loc, cgen_view g_p_ls, int32_t acc_q, int32_t acc_p,
                              cgen_view ride_src, cgen_view ride_dst, int32_t ride_acc, cgen_stream_t);
/* kl_chan_scale (optional, [c]): per-channel multiplier of the KL gradient -- the free-bits mask of this layer.
 *
 * Free bits (kl_free_bits > 0, vae.py:443-449).  S[b*out_stride + ch] = sum_{h,w} KL(q||p)[b,h,w,ch] of one layer
 * (c must divide 256; one deterministic workgroup per sample).  The caller lays the layers' channels side by side. */
int cgen_kl_channel_sums(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view q_loc, cgen_view q_ls,
                         cgen_view p_loc, cgen_view p_ls, float logt, float* out, int32_t out_stride, cgen_stream_t);
/* element-wise KL(q || p) map on flat contiguous f32 arrays, no reduction: the module-level gaussian_kl of vae.py:14-25
 * (-0.5 + p_ls - q_ls + 0.5 * (exp(q_ls)^2 + (q_loc - p_loc)^2) / exp(p_ls)^2; no clamps) */
int cgen_gaussian_kl_map(int64_t count, const float* q_loc, const float* q_ls, const float* p_loc, const float* p_ls,
                         float* out, cgen_stream_t);
/* z = loc + exp(ls + logt) * eps (prior sampling, vae.py:283-286); eps as above */
int cgen_sample_gaussian(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view loc, cgen_view ls,
                         cgen_view eps_in, const uint64_t* rng, uint32_t stream_id, float logt, cgen_view z,
                         cgen_stream_t);
/* Mediator latent z* (vae.py:485-513), q = q_ls+logt, p = p_ls+logt: u=(z-q_loc)/e^{q}; r_loc=a q_loc+(1-a)p_loc;
 * r_var=a^2 e^{2q}+(1-a)^2 e^{2p}; z* = r_loc + sqrt(r_var)*t*u   (t<=0 => no temperature factor).
 * linear_var != 0: r_var = a e^{2q} + (1-a) e^{2p}, the config-1 model's variant (simple_vae.py:383-386) */
int cgen_mediator_mix(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view z, cgen_view q_loc,
                      cgen_view q_ls, cgen_view p_loc, cgen_view p_ls, float alpha, float t, float logt, int32_t linear_var, cgen_view out,
                      cgen_stream_t);

/* ------------------------------------------------------------------ backward latent tail of a decoder layer (additive in ABI 411: new symbols only)
 * One launch (csrc/latent_tail.hip; binary16) for what follows a stochastic decoder layer's conv Block in the backward pass
 * (vae.py:263-300): the data gradients of z_feat_proj w.r.t. z and p_feat, the data gradient of z_proj w.r.t. z, the residual's
 * share of grad(p_feat) and the reparameterisation / KL backward.  With G_h = grad(h') [C channels] and G_f = grad(zf) [g_f.c]:
 *   g_z     = W_p[:, :Z]^T G_h + W_f[:, :Z]^T G_f + gz_in           (in registers, never stored; see `parity`)
 *   g_pfeat = G_h + W_f[:, Z:]^T G_f
 *   g_q_loc, g_q_ls, g_p_loc, g_p_ls: cgen_reparam_kl_bwd's formulas with d/dz = g_z
 *   out_p = [g_p_loc | g_p_ls | g_pfeat]  (2Z + C channels)       out_q = [g_q_loc | g_q_ls]  (2Z channels)
 * acc_p / acc_q: add what out_p / out_q already hold.  g_f.p == NULL: the layer has no z_feat_proj (g_pfeat = G_h); gz_in.p == NULL: none.
 * Weights: the data-gradient images cgen_weight_prep (mode 1) writes -- img_fz / img_fp = the z / p_feat segment of z_feat_proj
 * (rows x (ceil32(g_f.c) + 32)), img_pz = the z segment of z_proj (rows x (ceil32(C) + 32)); img_fz / img_fp are not read without g_f.
 * Served (cgen_latent_tail_bwd_supported() == 1, answered without a GPU): CGEN_F16; Z in {8, 16}; C and g_f.c multiples of 32 up to
 * 192; every view 16-byte aligned, linear in pixels (sn == h * sh, sh == w * sw) and below 2^31 bytes.  Anything else:
 * _supported() == 0 and cgen_latent_tail_bwd returns CGEN_EUNSUPPORTED without launching.
 * The DETERMINISTIC form (q_loc.p == NULL and q_ls.p == NULL; no struct change): the layer takes z = p_loc, so g_z IS grad(p_loc):
 *   out_p = [g_z | 0 | g_pfeat]                                   (the p_ls channels are written as zeros; out_q does not exist)
 * gz_in, p_loc, p_ls, z, out_q must be absent and acc_p / acc_q 0 (it does not accumulate); coef, chan_scale, logt are not read.
 * Only the conv_px order is built (parity 1), so what cgen_conv2d serves with its small-image kernel is declined: n*h*w up to its
 * pixel limit (6000), an image side below 5, or a conv dispatch knob in the environment. */
typedef struct cgen_latent_tail_bwd_args {
  int32_t dtype, n, h, w, z_dim, c;
  int32_t coef_stride, acc_q, acc_p;
  float logt;
  int32_t parity;   /* 0: one f32 sum and ONE binary16 rounding per output; 1: bit for bit what cgen_conv2d (x3) +
                     * cgen_reparam_kl_bwd_rider leave -- each GEMM summed in the order of the kernel cgen_conv2d picks for the
                     * shape and rounded to binary16 where those launches store grad(z) / grad(p_feat) (the engine's default) */
  int32_t reserved;
  cgen_view g_h, g_f, gz_in;            /* [n,h,w,C], [n,h,w,g_f.c] or absent, [n,h,w,Z] or absent */
  cgen_view q_loc, q_ls, p_loc, p_ls, z; /* [n,h,w,Z] each */
  cgen_view out_p, out_q;               /* [n,h,w,2Z + C], [n,h,w,2Z] */
  const void *img_fz, *img_fp, *img_pz;
  const float* coef;       /* kl_coef_dev[b * coef_stride], as in cgen_reparam_kl_bwd */
  const float* chan_scale; /* optional [Z] */
} cgen_latent_tail_bwd_args;
int cgen_latent_tail_bwd_supported(const cgen_latent_tail_bwd_args* a);
int cgen_latent_tail_bwd(const cgen_latent_tail_bwd_args* a, cgen_stream_t stream);

/* ------------------------------------------------------------------ forward latent tail of a decoder layer (additive in ABI 411: new symbols only)
 * One launch (csrc/latent_tail.hip; binary16) for what follows a stochastic decoder layer's prior and posterior Blocks in the
 * forward pass (vae.py:263-300): the reparameterisation + KL and the two 1x1 convs that read z.
 *   z       = rn16(q_loc + exp(q_ls + logt) * eps)                eps: the view, or Philox(rng, stream_id, b * h*w*Z + e) when absent
 *   kl_part[b * kl_stride + chunk]                                cgen_reparam_kl_fwd's partials: same chunks, same summation order
 *   h_out   = rn16(bias_p + W_p [z | pa] + h_in + p_feat)         z_proj: cgen_conv2d with res1 = h_in, res2 = p_feat
 *   zf      = rn16(bias_f + W_f [z | p_feat])                     z_feat_proj; zf.p == NULL: the layer has none
 * z, kl_part, h_out and zf are bit for bit what cgen_reparam_kl_fwd + cgen_conv2d x 2 leave: every GEMM is summed in the order of
 * the kernel cgen_conv2d picks for the shape (conv_px: bias as the initial value, K-steps in sequence; conv_smallp, few pixels:
 * K-step i in partial i % 4, the partials added in wave order, then the bias).
 * Weights: the forward images cgen_weight_prep (mode 0) writes for the two convs -- img_p: C rows x (ceil32(Z + ceil8(ctx)) + 32),
 * img_f: zf.c rows x (ceil32(Z + C) + 32); biases f32, optional.  pa is [n,h,w,ctx], linear in pixels or spatially constant (sh == sw == 0),
 * zero padded to a multiple of 8 channels (cpad).
 * Served (cgen_latent_tail_fwd_supported() == 1, answered without a GPU): CGEN_F16; Z in {8, 16}; C and zf.c multiples of 32 up to
 * 192; Z + ceil8(ctx) <= 64; no remainder planes (h_in_rem == h_out_rem == 0); every view 16-byte aligned, linear in pixels
 * (sn == h * sh, sh == w * sw; pa as above) and below 2^31 bytes; an image side below 5 only up to the small-image conv's pixel limit.
 * Anything else: _supported() == 0 and cgen_latent_tail_fwd returns CGEN_EUNSUPPORTED without launching.
 * The DETERMINISTIC form (q_loc.p == NULL and q_ls.p == NULL; no struct change): the layer takes z = p_loc --
 *   h_out = rn16(bias_p + W_p [p_loc | pa] + h_in + p_feat)       zf = rn16(bias_f + W_f [p_loc | p_feat])
 * with cgen_conv2d x 2's bits; nothing else is written.  p_ls, eps and z must be absent; rng, kl_part, kl_stride, stream_id and logt are
 * not read.  Only the conv_px order is built: n*h*w up to the small-image conv's pixel limit (6000) or an image side below 5 is declined. */
typedef struct cgen_latent_tail_fwd_args {
  int32_t dtype, n, h, w, z_dim, c;     /* c: channels of h_in, h_out and p_feat */
  int32_t ctx;                          /* channels of pa */
  int32_t kl_stride;
  uint32_t stream_id;
  float logt;
  int64_t h_in_rem, h_out_rem;          /* remainder planes of the f16 trunk (cgen_conv_args): not served, must be 0 */
  cgen_view q_loc, q_ls, p_loc, p_ls;   /* [n,h,w,Z] each */
  cgen_view p_feat, h_in;               /* [n,h,w,C] */
  cgen_view pa;                         /* [n,h,w,ctx] */
  cgen_view eps;                        /* [n,h,w,Z] or absent */
  cgen_view z, h_out, zf;               /* outputs: [n,h,w,Z], [n,h,w,C], [n,h,w,zf.c] or absent */
  const void *img_p, *img_f;
  const float *bias_p, *bias_f;
  const uint64_t* rng;                  /* device {seed, offset}, as in cgen_reparam_kl_fwd; needed without eps */
  float* kl_part;
} cgen_latent_tail_fwd_args;
int cgen_latent_tail_fwd_supported(const cgen_latent_tail_fwd_args* a);
int cgen_latent_tail_fwd(const cgen_latent_tail_fwd_args* a, cgen_stream_t stream);

/* ------------------------------------------------------------------ likelihoods (K11-K14) and ELBO
 * Discretised Gaussian (vae.py:352-411).  params view holds [loc(C) | logscale(C) | coeff(3, only C==3)] per pixel
 * (the raw 1x1-conv outputs); x is NHWC.  For C == 3 a params view of >= 9 channels selects vae.py's autoregressive
 * RGB form; a 6-channel view [loc(3) | logscale(3)] selects independent channels (simple_vae.py:103-171, no coeffs).  nll_part[b*nchunk+chunk] = partial sums of -log p over (C,H,W). */
int cgen_like_chunks(int32_t h, int32_t w);
int cgen_dgauss_nll_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, cgen_view x,
                        float* nll_part, cgen_stream_t);
/* g_params = coef_dev[b*coef_stride] * d(sum -log p)/d params */
int cgen_dgauss_nll_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, cgen_view x,
                        const float* coef_dev, int32_t coef_stride, cgen_view g_params, cgen_stream_t);
/* The two 1x1 likelihood heads x_loc / x_logscale (vae.py:325-333) fused with the discretised-Gaussian NLL, for one input
 * channel (C = 1) on the CGEN_F16 path: one launch each way, bit-identical to the launches it stands for.
 *   cgen_dgauss_head_fwd = cgen_conv2d(hin -> params channel 0, img_loc, bias_loc) + cgen_conv2d(hin -> params channel 1, img_ls,
 *     bias_ls) + cgen_dgauss_nll_fwd(params, x -> nll_part): reads hin once.
 *   cgen_dgauss_head_bwd = cgen_dgauss_nll_bwd(-> g_params) + the data gradient of x_logscale into g_h (a store) + the data gradient
 *     of x_loc accumulating on it + cgen_conv2d_wgrad of both heads (partials in the layout and split count of
 *     cgen_conv2d_wgrad_plan, `nsplit`): reads hin, params and x once and writes g_h once.  g_params is optional (p == NULL: the
 *     rounded gradients are used but not stored).
 * img_loc / img_ls: the heads' forward images from cgen_weight_prep (mode 0; row 0 is read); both biases are required.
 * Served (cgen_dgauss_head_supported() == 1, answered without a GPU, looks at dtype, n, h, w, hin, params, x, the images and the
 * biases): CGEN_F16; hin.c 16 or 32, 16-byte aligned; params.c == 2 and x.c == 1; and a shape at which cgen_conv2d serves the two
 * head convs with its halo-tiled kernel in one K-step (h, w >= 5 and more pixels than the small-image kernel takes) and the
 * weight gradients run on the generic kernel's plan.  Anything else: 0, and the entry points return CGEN_EUNSUPPORTED. */
typedef struct cgen_dgauss_head_args {
  int32_t dtype, n, h, w;
  cgen_view hin;
  const void* img_loc;
  const void* img_ls;
  const float* bias_loc;
  const float* bias_ls;
  cgen_view params;
  cgen_view x;
  float* nll_part; /* forward: [n][cgen_like_chunks(h, w)] */
  /* backward only */
  const float* coef_dev; /* as in cgen_dgauss_nll_bwd */
  int32_t coef_stride;
  int32_t nsplit;        /* cgen_conv2d_wgrad_plan of either head's weight gradient */
  cgen_view g_h;
  cgen_view g_params;    /* optional */
  float* partial_w_loc;  /* [nsplit][1][1][hin.c] */
  float* partial_b_loc;  /* [nsplit][1] */
  float* partial_w_ls;
  float* partial_b_ls;
} cgen_dgauss_head_args;
int cgen_dgauss_head_supported(const cgen_dgauss_head_args* a);
int cgen_dgauss_head_fwd(const cgen_dgauss_head_args* a, cgen_stream_t stream);
int cgen_dgauss_head_bwd(const cgen_dgauss_head_args* a, cgen_stream_t stream);
/* DGaussNet.sample (vae.py:413-422): loc (RGB autoregressive on the clamped predicted channels) and exp(logscale + log t),
 * NCHW f32 out.  rng == NULL: return_loc=True (x = clamp(loc)); rng = device (seed, offset): return_loc=False,
 * x = clamp(loc + scale * N(0,1)) with Philox noise of stream `stream_id` */
int cgen_dgauss_sample(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, float logt,
                       const uint64_t* rng, uint32_t stream_id, float* x_nchw, float* scale_nchw, cgen_stream_t);
/* DGaussNet.forward (vae.py:352-386): (loc, logscale) from the heads' outputs `params` = [loc(c) | logscale(c) | coeffs(3 if c == 3)]:
 * logscale = max(ls, -9) + logt; RGB: autoregressive means with tanh coefficients -- on the TRUE pixels `x` (NHWC view, c channels) when
 * given (vae.py:370-377), on the clamped predicted channels when x.p == NULL (vae.py:360-369).  Outputs NCHW f32. */
int cgen_dgauss_params(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, cgen_view x, float logt,
                       float* loc_nchw, float* logscale_nchw, cgen_stream_t stream);
/* Logit-space Gaussian of the config-1 model (simple_vae.py:173-248, GaussNet; x_like = *_gauss).  params = [loc(C) |
 * logscale(C)].  nll: x in [-1,1] -> (x+1)*127.5 + u, u ~ U[0,1) -> logit(./256) -> -log N(.; loc, exp(max(logscale,-9)))
 * (simple_vae.py:215-229; no log-determinant, as the reference).  u: NHWC view of injected uniforms (u.p != NULL), else
 * Philox uniforms from the device (seed, offset) pair `rng`, stream `stream_id`; bwd must be given the same u / rng state.
 * sample (simple_vae.py:231-238): scale = exp(logscale + logt) in both modes, x = loc (+ scale*N(0,1) when rng != NULL)
 * -> sigmoid*256 -> clamp((.-128)/128, -1, 1); NCHW f32 out. */
int cgen_gauss_nll_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, cgen_view x, cgen_view u,
                       const uint64_t* rng, uint32_t stream_id, float* nll_part, cgen_stream_t);
int cgen_gauss_nll_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, cgen_view x, cgen_view u,
                       const uint64_t* rng, uint32_t stream_id, const float* coef_dev, int32_t coef_stride,
                       cgen_view g_params, cgen_stream_t);
int cgen_gauss_sample(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view params, float logt,
                      const uint64_t* rng, uint32_t stream_id, float* x_nchw, float* scale_nchw, cgen_stream_t);
/* Discretised mixture of logistics, 10 mixtures, 3 channels (dmol.py:24-118, 164-215, 121-161). logits: [.,100].
 * nll_fwd / nll_bwd: dtype may be OR-ed with CGEN_DMOL_LOW_BIT for the reference's low_bit = True branch (5-bit pixels: half-bin
 * 1/31 and the mid-bin fallback's log 15.5 instead of 1/255 and log 127.5; dmol.py:52-60, 88-102). */
#define CGEN_DMOL_LOW_BIT 0x100
int cgen_dmol_nll_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view logits, cgen_view x, float* nll_part,
                      cgen_stream_t);
int cgen_dmol_nll_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view logits, cgen_view x,
                      const float* coef_dev, int32_t coef_stride, cgen_view g_logits, cgen_stream_t);
/* mode 0 soft mean, 1 hard (argmax) mean, 2 sample (Gumbel argmax + logistic noise from rng, temperature logt),
 * 10 + k (k = 1..9): top-k mean -- mixtures below the k-th largest logit are switched off and the rest renormalised */
int cgen_dmol_decode(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view logits, int32_t mode,
                     const uint64_t* rng, uint32_t stream_id, float logt, float* x_nchw, float* scale_nchw, cgen_stream_t);
/* Backward of cgen_dmol_decode (same mode numbering; mode 2 replays the forward's rng pair / stream_id / logt, so the caller
 * keeps a copy of the pair the forward launch read): g_x_nchw, g_scale_nchw (nullable) are the f32 NCHW gradients of x and
 * scale; writes all 100 channels of g_logits (zeros included), scaled by gscale.  The hard mean and the sample treat the
 * selected mixture as a constant; the soft and top-k means back-propagate through the softmax over the kept mixtures. */
int cgen_dmol_decode_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view logits, int32_t mode,
                         const uint64_t* rng, uint32_t stream_id, float logt, const float* g_x_nchw,
                         const float* g_scale_nchw, float gscale, cgen_view g_logits, cgen_stream_t);
/* elbo/nll/kl (vae.py:450-457): nll = mean_b( sum(nll_part[b]) / nll_div ), kl = mean_b( sum(kl_part[b]) / kl_div ),
 * out3 = {nll + beta*kl, nll, kl}.  kl_part: [nkl][B] per-sample sums already reduced per layer by the caller's
 * layout: kl_part[b*kl_stride + j], j < kl_count.  beta_dev (optional, device memory) overrides beta, so a captured
 * launch follows trainer.py's beta warm-up without re-capture. */
int cgen_elbo_finalize(int32_t n, const float* nll_part, int32_t nll_count, float nll_div, const float* kl_part,
                       int32_t kl_count, float kl_div, float beta, const float* beta_dev, float* out3, cgen_stream_t);
/* free-bits variant: kl = sum_j max(free_bits, mean_b kl_bc[b*ncol + j]) / kl_div; out3 as above;
 * chan_mask[j] = d max/d mean (1 / 0 / 0.5 on a tie) for cgen_reparam_kl_bwd's kl_chan_scale */
int cgen_elbo_finalize_fb(int32_t n, const float* nll_part, int32_t nll_count, float nll_div, const float* kl_bc, int32_t ncol,
                          float kl_div, float free_bits, float beta, const float* beta_dev, float* out3, float* chan_mask,
                          cgen_stream_t);
/* Backward of the counterfactual pixel step composed with both heads' DGaussNet.sample(h) decodes (dscm.py:52-56 over
 * vae.py:352-385,413-422), for the differentiable counterfactual branch of DSCM.forward (train_cf.py:159-183 fine-tunes the
 * HVAE through it): g_cfx_nchw = d loss / d cf_x (f32 NCHW), gscale = 1 / cf_particles; writes d/d params of the
 * reconstruction head and of the counterfactual head ([loc | logscale | coeffs] NHWC, same layout as the inputs). */
int cgen_cf_dgauss_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, cgen_view rec_params, cgen_view cf_params,
                       cgen_view x, const float* g_cfx_nchw, float gscale, cgen_view g_rec_params, cgen_view g_cf_params,
                       cgen_stream_t);
/* The same over two DmolNet mean decodes (dmol.py:234-245 with return_loc=True; mode 0 / 1 / 10 + k as in cgen_dmol_decode):
 * one launch per particle writes both 100-channel logit gradients (NHWC, same layout as the logits). */
int cgen_cf_dmol_bwd(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t mode, cgen_view rec_logits,
                     cgen_view cf_logits, cgen_view x, const float* g_cfx_nchw, float gscale,
                     cgen_view g_rec_logits, cgen_view g_cf_logits, cgen_stream_t);
/* Counterfactual pixel step (dscm.py:55-63): u=(x-rec_loc)/max(rec_scale,1e-12); cf=clamp(cf_loc+cf_scale*u,-1,1);
 * optional running sums sum_x += cf, sum_x2 += cf^2.  All NCHW f32 contiguous, `count` elements. */
int cgen_cf_pixels(int64_t count, const float* x, const float* rec_loc, const float* rec_scale, const float* cf_loc,
                   const float* cf_scale, float* cf_x, float* sum_x, float* sum_x2, cgen_stream_t);

/* ------------------------------------------------------------------ anticausal predictors (ABI 409, tiled placement 410)
 * The reference's pgm/layers.py CNN in eval mode (conv7x7 -> [maxpool2] -> five 3x3 convs -> spatial mean -> [cat y] -> Linear ->
 * Linear), every BatchNorm folded into the preceding conv / linear as weight scale + bias, followed by the per-variable negative
 * log-likelihood of flow_pgm.py's model_anticausal (Normal with optional tanh on the loc, OneHotCategorical(probs=softmax),
 * Bernoulli(probs=sigmoid); probabilities clamped to [eps, 1-eps] with eps = FLT_EPSILON as torch's clamp_probs does).
 * One record per CNN head; all heads of one call read the same image x (NCHW f32 contiguous, [n, c, res, res]).
 * Fused path (ws == NULL): one workgroup per image keeps the whole activation stack in LDS (cgen_predictor_supported says when).
 * Workspace path (ws != NULL): the same kernel with the activation stack in ws, n * cgen_predictor_workspace() floats.
 * Tiled path (cgen_predictor_tiled_*): one launch per layer whose grid covers (output tile x channel group x image x head), for
 * images whose stack does not fit in LDS; the stacks of all heads of all images live in ws at the same time.  Same records,
 * same terms / outs / loss / dx layouts and meanings as the other two. */
#define CGEN_PRED_MAX_HEADS 4
#define CGEN_PRED_MAX_OUT 16
enum cgen_pred_kind { CGEN_PRED_NORMAL = 0, CGEN_PRED_CATEGORICAL = 1, CGEN_PRED_BERNOULLI = 2 };
typedef struct cgen_pred_head {
  int32_t c, res, width, nout; /* in_shape = (c, res, res), CNN width, num_outputs */
  int32_t ctx;                 /* context_dim: y is [n, ctx] row-major, concatenated after the spatial mean */
  int32_t kind;                /* cgen_pred_kind; NORMAL needs nout == 2, BERNOULLI nout == 1, CATEGORICAL nout >= 2 */
  int32_t tanh_loc;            /* NORMAL: loc = tanh(out[0]) */
  int32_t obs_stride;          /* row stride (floats) of obs */
  float std_fixed;             /* NORMAL: > 0 = constant scale, else softplus(out[1]) */
  int32_t reserved;
  const float* w[8];           /* folded weights: w[0..5] convs [co][ci][k][k]; w[6] fc0 [8w][8w+ctx]; w[7] fc3 [nout][8w] */
  const float* b[8];           /* matching biases [co] */
  const float* y;              /* context, NULL iff ctx == 0 */
  const float* obs;            /* observed value: NORMAL / BERNOULLI 1 float, CATEGORICAL nout floats (one-hot; first max wins) */
} cgen_pred_head;
/* 1 if the fused (LDS) path takes these heads, 0 if not (and for invalid records: the launches say why) */
int cgen_predictor_supported(const cgen_pred_head* heads, int32_t nheads);
/* floats of workspace per image for the workspace path */
int cgen_predictor_workspace(const cgen_pred_head* heads, int32_t nheads, int64_t* floats_per_image);
/* Forward: terms[b*nheads + h] = -log p_h(obs_h[b] | x[b], y_h[b]); outs (optional) [nheads][n][CGEN_PRED_MAX_OUT] = the raw head
 * outputs; loss (optional, f32[1]) = sum of all terms, reduced in a fixed order (bit-identical from run to run). */
int cgen_predictor_fwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, float* terms, float* outs,
                       float* loss, cgen_stream_t);
/* Backward: dx = coef_dev[0] * d(sum of terms)/dx (overwritten, NCHW like x).  The heads' contributions are summed in a fixed
 * order inside each image's workgroup; no atomics.  Recomputes the forward. */
int cgen_predictor_bwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, const float* coef_dev,
                       float* dx, cgen_stream_t);
/* 1 if the tiled path takes these heads: every shape the launches accept (c 1..4, res 8..512, width 8 / 16 / 24 / 32) with the
 * SAME width in every head; 0 otherwise.  Never fails. */
int cgen_predictor_tiled_supported(const cgen_pred_head* heads, int32_t nheads);
/* floats of workspace for n images: n * nheads * (the floats of one head's activation stack, rounded up to a multiple of 4). */
int cgen_predictor_tiled_workspace(const cgen_pred_head* heads, int32_t nheads, int32_t n, int64_t* floats);
/* cgen_predictor_fwd / cgen_predictor_bwd on the tiled path.  ws must hold ws_floats >= cgen_predictor_tiled_workspace() floats; a
 * null or too-small workspace and unequal head widths are rejected before anything is launched.  Every launch goes on `stream`,
 * with no host synchronisation, allocation or read of device data (capturable).  dx is written by the stem's data-gradient
 * launch, which adds the heads' contributions in head order inside one thread per element; reruns are bit-identical and image
 * b's results do not depend on n or on b's position.  The backward recomputes the forward into ws. */
int cgen_predictor_tiled_fwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, int64_t ws_floats,
                             float* terms, float* outs, float* loss, cgen_stream_t);
int cgen_predictor_tiled_bwd(const cgen_pred_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, int64_t ws_floats,
                             const float* coef_dev, float* dx, cgen_stream_t);
/* The plan of the tiled placement's launches (additive in ABI 411: a new symbol).  Host code: no GPU needed, no pointer of a
 * record is dereferenced.  *count = CGEN_PRED_PLAN_LAUNCHES; when records != NULL, the first min(max, *count) records of
 * CGEN_PRED_PLAN_FIELDS int32 each are written, in launch order: the forward call's 7 launches (stem, 3x3 layers 1..5, tail), then
 * the 6 data-gradient launches the backward call adds after the same forward (layers 5..1, then the stem's into dx).  A record is
 *   [0] family: 0 ptile_conv_fwd<K, S, NP, CT, POOL>, 1 ptile_conv_bwd<S, CT, MODE>, 2 ptile_stem_bwd<S>, 3 ptile_tail
 *   [1] K  [2] S  [3] NP  [4] CT  (0 where the kernel has no such parameter)
 *   [5] POOL (family 0), MODE (family 1), 0 otherwise (the tail is reported as the forward call runs it)
 *   [6] layer: 0 the stem, 1..5 the 3x3 layers, 6 the tail
 *   [7] workgroups of the launch
 * The launchers read the same host functions, so the record is what runs.  Shapes as cgen_predictor_tiled_supported. */
#define CGEN_PRED_PLAN_LAUNCHES 13
#define CGEN_PRED_PLAN_FIELDS 8
int cgen_predictor_tiled_plan(const cgen_pred_head* heads, int32_t nheads, int32_t n, int32_t* records, int32_t max, int32_t* count);

/* ------------------------------------------------------------------ anticausal predictors, TRAINING mode (additive in ABI 411)
 * The same CNN with batch-statistic BatchNorm (pgm/layers.py CNN in train mode; train_pgm.py sup_epoch, --setup sup_aux): the
 * forward, the gradient of every parameter and, optionally, of the image.  One launch per layer over the whole batch, on the
 * activation layout of the tiled placement; same shapes as cgen_predictor_tiled_supported.  Per conv layer the forward writes
 * the raw convolution z (no bias, no activation), reduces the per-channel batch mean and BIASED variance over n*h*h in two
 * passes over z (mean first, then sum (z - mean)^2: no cancellation), writes a = lrelu(gamma (z - mean) invstd + beta) and
 * updates running_mean / running_var as nn.BatchNorm2d does (momentum, unbiased variance N / (N - 1), num_batches_tracked += 1).
 * The tail (spatial mean, cat y, fc.0, BatchNorm1d over the n images, LeakyReLU, fc.3, the likelihood) sees all images of a head.
 * A record: `hd` as for the eval paths except that hd.w[0..7] are the RAW weights (six convs, fc.0, fc.3), hd.b[7] is fc.3's
 * bias and hd.b[0..6] are not read; BatchNorm i = 0..5 follows conv i, BatchNorm 6 is fc.1.
 * The backward uses the state the forward left in ws (it does NOT recompute the forward: the running statistics move once per
 * step) and may be run once per forward.  Every gradient is OVERWRITTEN with coef_dev[0] * d(sum of terms)/d(parameter); all
 * reductions run in a fixed order without atomics: reruns are bit-identical.  Every launch goes on `stream`; no host
 * synchronisation, allocation or read of device data (capturable).  n >= 2 (BatchNorm1d needs more than one value per channel). */
typedef struct cgen_pred_train_head {
  cgen_pred_head hd;
  const float* gamma[7];            /* BatchNorm weight */
  const float* beta[7];             /* BatchNorm bias */
  float* running_mean[7];
  float* running_var[7];
  int64_t* num_batches_tracked[7];
  float* gw[8];                     /* gradients of hd.w[0..7] */
  float* gb;                        /* gradient of fc.3's bias */
  float* ggamma[7];
  float* gbeta[7];
} cgen_pred_train_head;
/* floats of workspace for n images: two activation stacks (pre-BatchNorm and post-activation) per (image, head), the batch
 * statistics, the tail's per-image rows and the partial sums of the split weight gradients */
int cgen_predictor_train_workspace(const cgen_pred_train_head* heads, int32_t nheads, int32_t n, int64_t* floats);
/* terms / outs / loss as cgen_predictor_fwd (terms is required); momentum = BatchNorm's (0.1) */
int cgen_predictor_train_fwd(const cgen_pred_train_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, int64_t ws_floats,
                             float momentum, float* terms, float* outs, float* loss, cgen_stream_t);
/* dx (optional, NCHW like x) = coef_dev[0] * d(sum of terms)/dx; same heads, n, x and ws as the forward just run */
int cgen_predictor_train_bwd(const cgen_pred_train_head* heads, int32_t nheads, int32_t n, const float* x, float* ws, int64_t ws_floats,
                             const float* coef_dev, float* dx, cgen_stream_t);

/* ------------------------------------------------------------------ ChestPGM's anticausal heads (additive in ABI 411; csrc/predictor_resnet.inc)
 * pgm/resnet.py ResNet18 with GroupNorm (flow_pgm.py:568-602, 659-703: encoder_s / encoder_r / encoder_f / encoder_a of the mimic
 * PGM) in eval mode -- 7x7/s2 stem, GroupNorm, ReLU, MaxPool2d(3, 2, 1), four stages of two residual blocks (64 / 128 / 256 / 512
 * channels; GroupNorm(min(32, c / 4), c), eps 1e-5; no conv bias; a 1x1/s2 conv + GroupNorm on the identity of the first block of
 * stages 2-4), spatial mean -- run ONCE and followed by the four Linear heads (the reference runs four equal copies of the trunk)
 * and the likelihoods of model_anticausal: Bernoulli(sigmoid) for sex and finding, OneHotCategorical(softmax) over 3 races,
 * Normal(loc, softplus(logscale) or std_fixed) without tanh for age, whose Linear also sees `finding` (513 inputs).
 * f32 NHWC.  x is [n, 1, res, res] f32 contiguous, 32 <= res <= 256, odd sizes included.  Heads, terms and outs are in the order
 * sex, race, finding, age.  Convs, in the order of img_fwd / img_dg / gamma / beta: 0 = stem; 1 + 2k / 2 + 2k = conv1 / conv2 of
 * block k = 0..7; 16 + s = the identity conv of stage s = 1..3.  The weight images are cgen_weight_prep's, CGEN_F32: mode 0
 * (forward) and mode 1 (data gradient) of the OIHW parameter as it is for the stride-1 3x3 convs (ks 3) and the 1x1 convs (ks 1);
 * the stem and conv1 of blocks 2, 4, 6 (stride 2) run on patch tensors (cgen_im2col_strided), so their parameter is imaged as the
 * 1x1 conv [co][ci * ks * ks] that it is there.
 * The forward keeps every raw conv output, every post-ReLU activation and the per-(image, group) mean and 1 / std in ws; the
 * backward reads them (it does NOT recompute the forward) and may run any number of times after a forward with the same n and ws.
 * Every launch goes on `stream`; no allocation, synchronisation or host read of device data (capturable).  All sums run in a fixed
 * order without atomics: reruns are bit-identical, and image b's results do not depend on n or on b's position. */
#define CGEN_RESNET_CONVS 20
#define CGEN_RESNET_SITES 18
typedef struct cgen_resnet_args {
  int32_t res;
  int32_t ctx_stride;                      /* row stride (floats) of ctx */
  float std_fixed;                         /* age: > 0 = constant scale, else softplus(out[1]) */
  int32_t obs_stride[4];                   /* row strides (floats) of obs */
  int32_t reserved;
  const void* img_fwd[CGEN_RESNET_CONVS];
  const void* img_dg[CGEN_RESNET_CONVS];
  const float* gamma[CGEN_RESNET_CONVS];   /* GroupNorm weight / bias, 16-byte aligned */
  const float* beta[CGEN_RESNET_CONVS];
  const float* fc_w[4];                    /* [1][512], [3][512], [1][512], [2][513] */
  const float* fc_b[4];
  const float* obs[4];                     /* sex [n][1], race [n][3] one-hot, finding [n][1], age [n][1]; read only with terms */
  const float* ctx;                        /* finding, the age head's context column: ctx[b * ctx_stride] */
} cgen_resnet_args;
/* floats of workspace for n images of res x res */
int cgen_resnet_workspace(int32_t n, int32_t res, int64_t* floats);
/* Where a post-ReLU activation lives in ws after a forward: NHWC [n, h, h, c] at float offset `offset`.  site 0 = the stem,
 * 1 + 2k / 2 + 2k = relu(bn1) / the output of block k, 17 = the max-pool's output. */
int cgen_resnet_site(int32_t n, int32_t res, int32_t site, int64_t* offset, int32_t* h, int32_t* c);
/* terms (optional) [n][4] = -log p_h(obs_h[b] | x[b]); outs (optional) [4][n][CGEN_PRED_MAX_OUT] = the raw head outputs; loss
 * (optional, needs terms) = the sum of all terms in a fixed order. */
int cgen_resnet_fwd(const cgen_resnet_args* a, int32_t n, const float* x, float* ws, int64_t ws_floats, float* terms, float* outs,
                    float* loss, cgen_stream_t);
/* dx [n, 1, res, res] = coef_dev[0] * d(sum of terms)/dx (overwritten) from the state the forward left in ws. */
int cgen_resnet_bwd(const cgen_resnet_args* a, int32_t n, float* ws, int64_t ws_floats, const float* coef_dev, float* dx,
                    cgen_stream_t);

/* ------------------------------------------------------------------ ChestPGM's anticausal heads, TRAINING (additive in ABI 411; csrc/predictor_resnet_train.inc)
 * The same network with CustomBlock's Dropout(p) after relu(bn1) of each of the eight blocks and every parameter gradient:
 *   a1[k] = keep ? relu(gn(raw)) * (1 / (1 - p)) : 0, keep = (u >= p) with u the Philox4x32-10 uniform of (rng state, stream
 *   981 + k, counter (image << 32 | channel quad of the image's NHWC map), word = channel & 3): an image's mask does not depend on
 *   n.  The forward does NOT advance the state (cgen_rng_advance does, between steps).  p_dropout == 0 launches exactly what
 *   cgen_resnet_fwd launches and leaves the same bits.  Deviation from the reference: it runs the trunk once per head and so
 *   draws four independent masks per step; here the trunk runs once, with one mask.
 * The backward is cgen_resnet_bwd's launch sequence (dx, when asked for, has its bits) with, beside it, per conv site: the f32
 * split-K weight gradient of the library (cgen_conv2d_wgrad + cgen_wgrad_reduce into the OIHW gradient; the stem and the stride-2
 * 3x3 convs as ks-1 problems on patches rebuilt by cgen_im2col_strided, the 1x1/s2 convs on the even-pixel view) and the GroupNorm
 * parameter gradients (per-(image, chunk, channel) partials, then one fixed tree per channel quad); and the four Linears' gradients.
 * Every gradient is OVERWRITTEN with d (coef_dev[0] * sum of terms) / d parameter.
 * An image that leaves a non-finite GroupNorm statistic (a NaN or Inf in x or in a weight) gets NaN for its four terms: the eval
 * kernels' ReLU maps NaN to 0, torch's keeps it, and a training step must see such a batch as the reference sees it.
 * The workspace starts with cgen_resnet_workspace's layout (cgen_resnet_site applies) and is larger.  One stream, no allocation,
 * synchronisation or host read, fixed-order sums without atomics, bit-identical reruns, capturable -- as cgen_resnet_*. */
typedef struct cgen_resnet_train_args {
  cgen_resnet_args net;
  float* gw[CGEN_RESNET_CONVS];      /* OIHW gradient of each conv, 16-byte aligned */
  float* ggamma[CGEN_RESNET_CONVS];  /* GroupNorm weight / bias gradients, 16-byte aligned */
  float* gbeta[CGEN_RESNET_CONVS];
  float* gfc_w[4];                   /* as fc_w / fc_b, 4-byte aligned */
  float* gfc_b[4];
  const uint64_t* rng;               /* device {seed, offset}, what cgen_rng_advance moves */
  float p_dropout;                   /* in [0, 1) */
  int32_t reserved;
} cgen_resnet_train_args;
int cgen_resnet_train_workspace(int32_t n, int32_t res, int64_t* floats);
int cgen_resnet_train_fwd(const cgen_resnet_train_args* a, int32_t n, const float* x, float* ws, int64_t ws_floats, float* terms,
                          float* outs, float* loss, cgen_stream_t);
/* x: the forward's image (the stem's patches are rebuilt from it); dx optional (NULL: the stem's data gradient is not computed). */
int cgen_resnet_train_bwd(const cgen_resnet_train_args* a, int32_t n, const float* x, float* ws, int64_t ws_floats,
                          const float* coef_dev, float* dx, cgen_stream_t);
/* keep [n, h, h, c] (NHWC, one byte per element: 1 = kept) = the decisions the forward takes for block k = 0..7 under this state
 * and p, from the same device function (tests, debugging). */
int cgen_resnet_dropout_keep(const uint64_t* rng, float p_dropout, int32_t n, int32_t res, int32_t block, uint8_t* keep, cgen_stream_t);

/* ------------------------------------------------------------------ scalar predictor head, TRAINING mode (additive in ABI 411; csrc/predictor_mlp.inc)
 * pgm/layers.py MLP in train mode (layers.py:46-59), scored as flow_pgm.py:260-267 scores encoder_a: q(a | b, v) = Normal(MLP(b, v)).
 *   mlp.0 Linear nin -> w (no bias), mlp.1 BatchNorm1d(w), LeakyReLU(0.01), mlp.3 Linear w -> w (no bias), mlp.4 BatchNorm1d(w),
 *   LeakyReLU(0.01), mlp.6 Linear w -> 2 (bias); term[b] = -log Normal(obs[b]; loc, scale) with loc = out[0] (tanh(out[0]) with
 *   tanh_loc) and scale = std_fixed > 0 ? std_fixed : softplus(out[1]): cgen_pred_head's NORMAL kind, the same device function.
 * Both BatchNorms take the mean over the n rows first and then the BIASED variance about that mean in a second pass, and update
 * running_mean / running_var as nn.BatchNorm1d does (momentum, unbiased variance n / (n - 1), num_batches_tracked += 1).
 * Input column k of row b is in[k][b * in_stride[k]]: columns of separate buffers or of one wider row-major table are read in
 * place, in the order torch.cat would put them.  There is no gradient to the inputs (observed parents).
 * Served: 2 <= n <= 4096, 1 <= nin <= CGEN_MLP_MAX_IN, w a multiple of 8 up to CGEN_MLP_MAX_WIDTH, two outputs.
 * LAUNCHES: ONE per direction, whatever n: a single workgroup of 1024 threads owns the whole batch, so every reduction over the
 * batch runs inside it in a fixed order (per-thread sums over rows b = g, g + G, ..., merged in g order).  No atomics; reruns are
 * bit-identical.  Capturable: one stream, no allocation, no synchronisation, no host read of device data.
 * Workspace (floats): 3 * n * w (the two normalised pre-activations and one gradient plane) + 2 * n (the outputs) + 2 * w (1 / std). */
#define CGEN_MLP_MAX_IN 8
#define CGEN_MLP_MAX_WIDTH 64
typedef struct cgen_mlp_train_head {
  int32_t nin, width;               /* num_inputs, hidden width */
  int32_t tanh_loc;                 /* loc = tanh(out[0]) */
  int32_t obs_stride;               /* row stride (floats) of obs */
  float std_fixed;                  /* > 0 = constant scale, else softplus(out[1]) */
  int32_t reserved;
  const float* in[CGEN_MLP_MAX_IN]; /* input columns, in[k][b * in_stride[k]] */
  int64_t in_stride[CGEN_MLP_MAX_IN];
  const float* obs;                 /* observed value, obs[b * obs_stride] */
  const float* w[3];                /* mlp.0 [w][nin], mlp.3 [w][w], mlp.6 [2][w] */
  const float* bias;                /* mlp.6 [2] */
  const float* gamma[2];            /* mlp.1, mlp.4 weight */
  const float* beta[2];             /* mlp.1, mlp.4 bias */
  float* running_mean[2];
  float* running_var[2];
  int64_t* num_batches_tracked[2];
  float* gw[3];                     /* gradients of w[0..2] */
  float* gb;                        /* gradient of bias */
  float* ggamma[2];
  float* gbeta[2];
} cgen_mlp_train_head;
/* floats of workspace for n rows: 3 * n * width + 2 * n + 2 * width */
int cgen_mlp_train_workspace(const cgen_mlp_train_head* rec, int32_t n, int64_t* floats);
/* Forward: terms[b] (required, f32[n]) = the row's term; loss (optional, f32[1]): the sum of the terms, taken in a fixed order, is
 * ADDED to the value already there (a step adds this head to the image heads' sum without a launch of its own; a caller that wants
 * the head's sum alone zeroes it first).  momentum = BatchNorm's (0.1).  Leaves in ws what the backward reads. */
int cgen_mlp_train_fwd(const cgen_mlp_train_head* rec, int32_t n, float* ws, int64_t ws_floats, float momentum, float* terms, float* loss,
                       cgen_stream_t);
/* Backward of the forward just run on the same rec, n and ws (it does not recompute it: the running statistics move once per
 * step): every gradient of rec is OVERWRITTEN with coef_dev[0] * d(sum of terms)/d(parameter). */
int cgen_mlp_train_bwd(const cgen_mlp_train_head* rec, int32_t n, float* ws, int64_t ws_floats, const float* coef_dev, cgen_stream_t);

/* ------------------------------------------------------------------ counterfactual evaluation (additive in ABI 411: new symbols only, no struct, enum value or signature moved)
 * The numbers of the reference's evaluation half, accumulated on the device: train_cf.py:63-108 get_metrics over the predictions
 * the `else` branch of cf_epoch collects (train_cf.py:181-189), and train_pgm.py:175-249 eval_epoch on factual images -- ROC-AUC
 * and accuracy of the binary / categorical predictors, mean absolute error of the continuous ones -- plus the per-image distances
 * behind the composition and reversibility measures.  The reference pulls every batch to the host and calls sklearn.
 * All three calls only enqueue on `stream`: no allocation, no host read of device data, no global state (capturable).  Every
 * result is bit-identical from run to run: sums are reduced in a fixed order in f64, pair counts are 64-bit INTEGER atomics
 * (order-independent); there is no floating-point atomic.  Arguments are checked before anything is launched. */
#define CGEN_METRIC_MAX_VARS 8
#define CGEN_METRIC_ACC 8 /* doubles per accumulator block */
enum cgen_metric_kind { CGEN_METRIC_BINARY = 0, CGEN_METRIC_CATEGORICAL = 1, CGEN_METRIC_CONTINUOUS = 2 };
/* what predict() applies to the raw head output (flow_pgm.py predict: sigmoid / softmax / tanh / nothing) */
enum cgen_metric_transform { CGEN_METRIC_NONE = 0, CGEN_METRIC_SIGMOID = 1, CGEN_METRIC_SOFTMAX = 2, CGEN_METRIC_TANH = 3 };
enum cgen_metric_slot { CGEN_METRIC_N = 0,        /* rows counted */
                        CGEN_METRIC_CORRECT = 1,  /* BINARY / CATEGORICAL: rows predicted right */
                        CGEN_METRIC_ABS_ERR = 2,  /* CONTINUOUS: sum of |target - prediction| / norm */
                        CGEN_METRIC_SKIPPED = 3,  /* rows with a non-finite prediction or target (cf_epoch's NaN `continue`) */
                        CGEN_METRIC_OVERFLOW = 4  /* counted rows that did not fit in the score buffer (left out of the AUC only) */ };
typedef struct cgen_metric_var {
  int32_t kind;          /* cgen_metric_kind */
  int32_t transform;     /* cgen_metric_transform: BINARY NONE / SIGMOID, CATEGORICAL NONE / SOFTMAX, CONTINUOUS NONE / TANH */
  int32_t ncls;          /* columns read: BINARY / CONTINUOUS 1, CATEGORICAL 2..CGEN_PRED_MAX_OUT */
  int32_t reserved;
  const float* pred;     /* [n][pred_stride], ncls columns read: e.g. one head of cgen_predictor_fwd's `outs` in place
                            (pred_stride = CGEN_PRED_MAX_OUT), or any [n, k] tensor */
  int64_t pred_stride;   /* floats, >= ncls */
  const float* target;   /* [n][target_stride]: BINARY 0 / 1, CATEGORICAL a one-hot row of ncls, CONTINUOUS 1 value */
  int64_t target_stride; /* floats, >= ncls (CATEGORICAL) or >= 1 */
  /* CONTINUOUS: |(t * tgt_scale + tgt_shift) - (f(o) * pred_scale + pred_shift)| / norm, in f64 (get_metrics' unnormalisation) */
  float pred_scale, pred_shift, tgt_scale, tgt_shift, norm;
  int32_t reserved2;
  double* acc;           /* [CGEN_METRIC_ACC], indexed by cgen_metric_slot; this call ADDS to it */
  /* AUC (optional, BINARY / CATEGORICAL; all NULL = no AUC): rows are appended in sample order at *row_count.
   * BINARY: score = sigmoid(o) (f32; o itself with NONE), label = t > 0.5.  CATEGORICAL: the softmax row (the row itself with
   * NONE) and the one-hot row.  Row r, column c sits at [r * ncls + c]. */
  float* scores;
  float* labels;
  int64_t capacity;      /* rows the two buffers hold */
  int64_t* row_count;    /* device: rows appended so far (<= capacity) */
} cgen_metric_var;
/* One batch of n samples, one record per variable (1..CGEN_METRIC_MAX_VARS), one launch.  Per sample: BINARY correct iff
 * (o > 0) == (t > 0.5) with SIGMOID -- torch.round(sigmoid(o)) == t including o == 0 -> 0 -- or (p > 0.5) == (t > 0.5) with NONE;
 * CATEGORICAL correct iff argmax(pred) == argmax(target), first maximum wins (train_cf.py:98); CONTINUOUS as above.  A row with
 * a non-finite prediction or target is skipped for that variable; a row beyond `capacity` is dropped from the AUC only. */
int cgen_metric_accum(const cgen_metric_var* vars, int32_t nvars, int32_t n, cgen_stream_t);
/* Exact ROC-AUC per column, (#{s+ > s-} + 0.5 #{s+ == s-}) / (n+ n-) over all positive / negative pairs (what
 * sklearn.metrics.roc_auc_score computes, train_cf.py:73,87,100): a tiled O(n^2) pair count through LDS with 64-bit integer
 * counts -- exact, order-independent, no sort.  scores / labels: [rows][stride], `ncls` columns read (binary: 1; the one-vs-rest
 * macro AUC of train_cf.py:100-105 is the caller's mean over columns); label > 0.5 is a positive; rows with a NaN score are left
 * out.  The row count is min(*n_rows_dev, n_rows_max), read on the device; n_rows_max (host, < 2^31) only sizes the grid.
 * auc_out[ncls] (f64): NaN for a column without a positive or without a negative.  ws: 4 * ncls uint64, zeroed by the call. */
int cgen_rocauc(const float* scores, const float* labels, const int64_t* n_rows_dev, int64_t n_rows_max, int32_t ncls,
                int64_t stride, double* auc_out, uint64_t* ws, cgen_stream_t);
/* Per-image distances of two NCHW f32 batches of n images, elems_per_image floats each (contiguous): L1 = mean |a - b| and
 * L2 = mean (a - b)^2, the differences and sums in f64 throughout.  One workgroup reduces one image in a fixed order (16-byte
 * loads when both bases and the image size allow, else a scalar path) into ws[i] = {L1, L2} (f64 [n][2], required) and, if
 * given, per_image[i] = the same rounded to f32; a second launch folds the n values in a fixed order and ADDS
 * {sum L1, sum L2, n} to acc[3] (optional). */
int cgen_image_dist(int32_t n, int64_t elems_per_image, const float* a, const float* b, float* per_image, double* ws, double* acc,
                    cgen_stream_t);

/* ------------------------------------------------------------------ parent SCM: log-likelihood and its parameter gradients (additive in ABI 411: new symbols and one new struct, nothing moved)
 * train_pgm.py sup_epoch with --setup sup_pgm: -log p(parents) of flow_pgm.py's svi_model under an empty guide.  The SCM is a list
 * of 1..CGEN_PGM_MAX_MECH scalar mechanisms, each scoring one variable of a row-major f32 table obs[rows][ncol] (a one-hot variable
 * is its ncls columns, a class index is one column holding 0, 1, ...).  term[row][mech] = log p(variable | its parents):
 *   BERNOULLI    x l - softplus(l)                                          p[0] = the logit [1]
 *   CATEGORICAL  sum_j x_j log_softmax(l)_j                                 p[0] = the logits [ncls]
 *   SPLINE       Normal(0,1) -> linear rational spline (pyro T.Spline(1, bins, bound, order="linear")): eps = spline^-1(u),
 *                -eps^2/2 - log(2 pi)/2 - log|d spline / d eps|(eps); the identity outside +-bound.
 *                p[0..3] = unnormalized widths [bins], heights [bins], derivatives [bins - 1], lambdas [bins]
 *   AFFINE       (loc, log_scale) = MLP(ctx); eps = (u - loc) exp(-log_scale); -eps^2/2 - log(2 pi)/2 - log_scale
 *   GUMBEL_MAX   log_softmax(MLP(ctx))[class]  (TransformedDistributionGumbelMax.log_prob: the base Gumbel density is not in it)
 * `normalize` (SPLINE, AFFINE): the variable lives in [-1, 1] behind 2 sigmoid(.) - 1: u = logit((x + 1) / 2) with torch's
 * SigmoidTransform clamp [FLT_MIN, 1 - FLT_EPSILON], and the term gets -(log 2 + logsigmoid(u) + logsigmoid(-u)); else u = x.
 * MLP (pyro DenseNN): nctx (1..2) inputs -> width[0..nhidden) (nhidden 1..CGEN_PGM_MAX_HIDDEN, each <= CGEN_PGM_MAX_WIDTH) with
 * `act` between -> 2 outputs (AFFINE) or ncls (GUMBEL_MAX); layer i has p[2 i] = weight [out][in] and p[2 i + 1] = bias [out].
 * g[k] is where the gradient of p[k] goes (a slot of the caller's flat gradient buffer); the forward does not read g.
 * Every buffer is f32 (sums and the spline algebra accumulate in f64 registers and round once).  Both entry points only enqueue on `stream`: no allocation, no host synchronisation, no host read of device
 * data (capturable).  No atomics; every sum runs in a fixed order, so reruns give the same bits.  Arguments are checked before
 * anything is launched and the error names the offending field. */
#define CGEN_PGM_MAX_MECH 8
#define CGEN_PGM_MAX_WIDTH 64
#define CGEN_PGM_MAX_HIDDEN 3
#define CGEN_PGM_MAX_BINS 8
#define CGEN_PGM_MAX_CLS 16
#define CGEN_PGM_ROWS 64 /* rows per workgroup: the workspace holds one row of partial sums per workgroup */
enum cgen_pgm_kind { CGEN_PGM_BERNOULLI = 0, CGEN_PGM_CATEGORICAL = 1, CGEN_PGM_SPLINE = 2, CGEN_PGM_AFFINE = 3, CGEN_PGM_GUMBEL_MAX = 4 };
enum cgen_pgm_act { CGEN_PGM_LEAKY_RELU = 0 /* slope 0.1 */, CGEN_PGM_GELU = 1 /* exact erf */, CGEN_PGM_SIGMOID = 2 };
typedef struct cgen_pgm_mech {
  int32_t kind;       /* cgen_pgm_kind */
  int32_t normalize;  /* 0 / 1 (SPLINE, AFFINE) */
  int32_t col;        /* first column of the variable in obs */
  int32_t ncls;       /* CATEGORICAL, GUMBEL_MAX: 2..CGEN_PGM_MAX_CLS */
  int32_t nctx;       /* AFFINE, GUMBEL_MAX: 1..2 */
  int32_t ctx_col[2]; /* columns of the context, in the order the MLP takes them */
  int32_t nhidden;
  int32_t width[CGEN_PGM_MAX_HIDDEN];
  int32_t act;        /* cgen_pgm_act */
  int32_t bins;       /* SPLINE: 2..CGEN_PGM_MAX_BINS */
  float bound;        /* SPLINE: > 0 */
  const float* p[8];
  float* g[8];
} cgen_pgm_mech;
/* bytes of workspace cgen_pgm_nll_fwd_bwd needs for `rows` rows: ceil(rows / CGEN_PGM_ROWS) rows of one partial sum per
 * parameter-gradient slot (BERNOULLI 1, CATEGORICAL ncls, SPLINE 4 bins + 3, MLP its weights and biases).  A pure query. */
int cgen_pgm_workspace(const cgen_pgm_mech* mechs, int32_t n, int32_t rows, int64_t* bytes);
/* terms[rows][n] and loss_sum[0] = the sum of all terms (one workgroup, strided partial sums and a fixed tree).  Row r of the
 * batch is obs row index[r] (device int64, optional; NULL = row r); an index outside [0, table_rows) makes that row's terms NaN. */
int cgen_pgm_nll_fwd(const cgen_pgm_mech* mechs, int32_t n, const float* obs, int32_t ncol, int64_t table_rows, const int64_t* index,
                     int32_t rows, float* terms, float* loss_sum, cgen_stream_t);
/* the same forward, then g[k] of every mechanism = coef_dev[0] * d(sum of terms)/d(p[k]) (overwritten).  Two launches: one
 * workgroup per (CGEN_PGM_ROWS rows, mechanism) writes its partial sums to a row of `workspace`; the second adds the rows in index
 * order and applies the chain through softmax / softplus / sigmoid / cumsum of the root and spline parameters, which does not
 * depend on the batch.  A parameter no row touches gets an exact 0. */
int cgen_pgm_nll_fwd_bwd(const cgen_pgm_mech* mechs, int32_t n, const float* obs, int32_t ncol, int64_t table_rows, const int64_t* index,
                         int32_t rows, float* terms, float* loss_sum, const float* coef_dev, float* workspace, int64_t workspace_bytes,
                         cgen_stream_t);

/* ------------------------------------------------------------------ parent SCM: counterfactual parents (additive in ABI 411: one new symbol and two new structs, nothing moved)
 * BasePGM.counterfactual (flow_pgm.py:71-108) followed by dscm.py's vae_preprocess: abduction -> action -> prediction over the same
 * mechanism records, in ONE launch.  The records must be in topological order: every ctx_col[i] of a record must be the `col` of
 * an EARLIER record (g[] is not read).  Row r of the batch is obs row index[r]; its intervention values are row do_index[r] of
 * do_table, a table with the same column layout as obs.  A mechanism is TOUCHED if its bit is set in the mask or if any of its
 * context mechanisms is touched.  In record order:
 *   in the mask        its columns (ncls of them for CATEGORICAL) are the do row's columns, bit for bit
 *   not touched        its columns are the observation's, bit for bit (the reference recomputes f(f^-1(obs)) here, which returns
 *                      the observation up to rounding; the copy makes the null intervention exact)
 *   touched AFFINE     eps = (u - loc(ctx_obs)) exp(-log_scale(ctx_obs)), u the un-normalised observation;
 *                      cf = loc(ctx_cf) + exp(log_scale(ctx_cf)) eps, normalised again (2 sigmoid(.) - 1) when `normalize` is set;
 *                      ctx_cf is read from the counterfactual values already produced for the row
 *   touched GUMBEL_MAX noise from the observed class, the logits at ctx_obs and the caller's uniforms (exact_gumbel = 0:
 *                      ArgMaxGumbelMax.inv of layers.py:139-160 as it is; 1: the exact top-down posterior), then the class is
 *                      argmax(noise + logits(ctx_cf)), the first index winning ties; an observed class outside 0..ncls-1 gives NaN
 * BERNOULLI, CATEGORICAL and SPLINE mechanisms have no context: they are only ever copied, and the spline inverse serves eps alone.
 * Columns of the table that belong to no mechanism are copied through from the observation.
 * Precision as above: buffers and activations f32; dot products, the spline algebra and the affine round trip (eps is not
 * rounded between abduction and prediction) in f64 registers, rounded to f32 once.  No RNG, no atomics, no workspace: the launch
 * is a pure function of its inputs and reruns give the same bits.  It only enqueues on the stream (capturable); arguments are
 * checked before the launch and the error names the offending field.  cf, eps, pa and cf_pa must not overlap obs or do_table. */
#define CGEN_PGM_MAX_PRE 8
enum cgen_pgm_pre_kind { CGEN_PGM_PRE_COPY = 0, CGEN_PGM_PRE_LOGSTD = 1 };
/* one entry of the parents vector the HVAE takes (vae_preprocess, in args.parents_x order) */
typedef struct cgen_pgm_pre {
  int32_t col;    /* first column of the variable in the table */
  int32_t width;  /* columns taken (1, or the classes of a one-hot variable); col + width <= ncol */
  int32_t kind;   /* COPY: the columns as they are.  LOGSTD (dscm.py ukbb_preprocess), per column:
                     (log(max((x + 1) / 2 * (hi - lo) + lo, 1e-12)) - mu) / sd, evaluated in f64 */
  float hi, lo;   /* LOGSTD: the variable's range behind the [-1, 1] normalisation */
  float mu, sd;   /* LOGSTD: mean and standard deviation of its logarithm (sd != 0) */
} cgen_pgm_pre;
typedef struct cgen_pgm_cf_args {
  const float* obs;            /* [table_rows][ncol] f32 observations */
  int64_t table_rows;          /* >= 1; >= rows when index is NULL */
  const int64_t* index;        /* device int64 [rows], optional: NULL = row r.  An index outside [0, table_rows) makes every output of that row NaN */
  const float* do_table;       /* [do_rows][ncol] f32 intervention values, same column layout as obs; required when the host mask
                                  is non-zero or do_mask_dev is given (only the columns of masked mechanisms are read) */
  int64_t do_rows;             /* >= 1 with a do_table; >= rows when do_index is NULL */
  const int64_t* do_index;     /* device int64 [rows], optional: NULL = row r of do_table.  With a non-zero mask, an index outside
                                  [0, do_rows) makes every output of that row NaN */
  const uint32_t* do_mask_dev; /* optional device word, read by the kernel INSTEAD of do_mask (a captured graph changes the
                                  intervened variable between replays); bits at or above n are ignored */
  const float* uniforms[CGEN_PGM_MAX_MECH]; /* uniforms[m]: [rows][ncls] f32 in [0, 1) for GUMBEL_MAX mechanism m (batch row r, not
                                  index[r]), drawn by the caller; required for every GUMBEL_MAX record, not read for the others.
                                  A uniform of exactly 0 is replaced by FLT_MIN (its Gumbel would be -inf) */
  float* cf;                   /* [rows][ncol] the counterfactual table */
  float* eps;                  /* optional [rows][n]: the abducted noise of every SPLINE and AFFINE mechanism, touched or not
                                  (infer_exogeneous); 0 for roots and GUMBEL_MAX */
  float* pa;                   /* optional [rows][ctx]: the factual parents as the HVAE takes them, ctx = sum of pre[].width */
  float* cf_pa;                /* optional [rows][ctx]: the counterfactual parents, same layout (pa's bits under an empty mask) */
  int32_t ncol;                /* columns of obs, do_table and cf */
  int32_t rows;                /* 1..2^24 */
  uint32_t do_mask;            /* bit m set: mechanism m is intervened on; a bit at or above n is an error */
  int32_t exact_gumbel;        /* 0 / 1 */
  int32_t npre;                /* 0..CGEN_PGM_MAX_PRE entries of pre[]; >= 1 when pa or cf_pa is given */
  int32_t reserved;            /* 0 */
  cgen_pgm_pre pre[CGEN_PGM_MAX_PRE];
} cgen_pgm_cf_args;
/* One workgroup per CGEN_PGM_ROWS rows walks the mechanisms in order, each MLP's weights staged in LDS once and evaluated at the
 * factual and the counterfactual context of its rows.  Records and arguments travel by value in the kernel-argument segment. */
int cgen_pgm_counterfactual(const cgen_pgm_mech* mechs, int32_t n, const cgen_pgm_cf_args* a, cgen_stream_t);

/* ------------------------------------------------------------------ step tail (K17; trainer.py:67-87, utils.py:178-225)
 * Flat-buffer fused global-norm -> clip -> skip predicate -> AdamW -> EMA.
 * state_dev: f32[8] = {sum_sq, grad_norm, clip_coef, skip_flag, n_skipped, opt_steps, n_skipped_nonfinite, -}.  LambdaLR warm-up, Adam
 * bias correction and the EMA warm-up decay are all derived ON DEVICE from opt_steps (successful steps so far), so
 * the host never reads the skip decision (the reference syncs three times per step).
 * out3 (optional) = {elbo, nll, kl}: NaN nll/kl forces a skip as trainer.py:71-74 does. */
int cgen_sumsq_partial(const float* g, int64_t count, float* partial /*[nblk]*/, int32_t nblk, cgen_stream_t);
int cgen_clip_decide(const float* partial, int32_t nblk, const float* out3, float max_norm, float skip_norm,
                     float* state_dev, cgen_stream_t);
typedef struct cgen_adamw_args {
  float* p; const float* g; float* m; float* v; float* ema; /* ema may be NULL */
  int64_t count;
  float lr, beta1, beta2, eps, wd, ema_beta;
  int32_t warmup_steps, ema_update_after;
  const float* state_dev; /* reads clip_coef, skip_flag, opt_steps */
} cgen_adamw_args;
int cgen_adamw_ema(const cgen_adamw_args* a, cgen_stream_t);
/* opt_steps += 1 unless the step was skipped (run once after all cgen_adamw_ema launches of a step) */
int cgen_step_commit(float* state_dev, cgen_stream_t);
/* cgen_adamw_ema without the LambdaLR warm-up: lr as given on every step (train_cf.py has no scheduler); warmup_steps is ignored. */
int cgen_adamw_ema_const_lr(const cgen_adamw_args* a, cgen_stream_t);

/* ---- counterfactual fine-tuning (train_cf.py:140-180, dscm.py:75-88): what CfTrainStep adds to the tail above (csrc/cf_train.hip).
 * Fixed-order sums, no atomics, bit-identical reruns; every call only enqueues.
 *
 * cgen_nonfinite_partial: partial[b] = number of NaN / +-inf among block b's share of the n*h*w*v.c logical elements of the NHWC
 * view `v` (CGEN_F32 or CGEN_F16; v.sw >= v.c, a padded channel stride is skipped over).  Logical element i = ((n h + y) w + x) c + ch
 * belongs to block (i / 256) % nblk, the assignment of cgen_sumsq_partial.  Fewer than 2^31 elements. */
int cgen_nonfinite_partial(int32_t dtype, int32_t n, int32_t h, int32_t w, cgen_view v, int32_t* partial /*[nblk]*/, int32_t nblk,
                           cgen_stream_t);
/* cgen_cf_lagrange (one workgroup).  With c = eps - elbo, w = lmbda - damping c (the damping term under stop-gradient):
 *   res  = {loss = aux_loss - w c, aux_loss = (aux_sum [+ aux_add]) inv_b, g_lmbda = -c, w}
 *   coef = {w seed_scale, w beta seed_scale, beta}: the engine's likelihood / KL gradient seeds, seed_scale = S / (B dims)
 *   *gsq_slot = g_lmbda^2: the multiplier's slot among the gradient norm's partial sums
 *   gate = {loss, bad ? NaN : nll, kl} for cgen_clip_decide's out3; bad = loss non-finite or any of the n_nonfinite counts > 0
 *   sums = {loss, aux_loss, elbo, nll, kl, n, n_bad, -}: += the step's values and n += 1 unless bad, else n_bad += 1
 * beta is read from beta_dev when that is not NULL. */
typedef struct cgen_cf_lagrange_args {
  const float* out3; const float* aux_sum; const float* aux_add /* may be NULL */; const float* lmbda;
  const float* beta_dev /* may be NULL */; const int32_t* nonfinite; int32_t n_nonfinite;
  float inv_b, eps, damping, seed_scale, beta;
  float* res /*[4]*/; float* coef /*[3]*/; float* gsq_slot; float* gate /*[3]*/; float* sums /*[8]*/;
} cgen_cf_lagrange_args;
int cgen_cf_lagrange(const cgen_cf_lagrange_args* a, cgen_stream_t);
/* cgen_lagrange_step (one thread; train_cf.py:174-177), after the parameters' cgen_adamw_ema launches and before cgen_step_commit:
 * nothing on a skipped step; else AdamW(maximize=True, wd = 0, constant lr) on the gradient -g[0] clip_coef with cgen_adamw_ema's
 * moment updates and bias corrections, then lmbda = max(lmbda, 0), then the EMA of the clamped value with cgen_adamw_ema's decay. */
typedef struct cgen_lagrange_step_args {
  float* lmbda; float* m; float* v; float* ema /* may be NULL */; const float* g; const float* state_dev;
  float lr, beta1, beta2, eps, ema_beta;
  int32_t ema_update_after;
} cgen_lagrange_step_args;
int cgen_lagrange_step(const cgen_lagrange_step_args* a, cgen_stream_t);

/* Philox normal fill (f32 contiguous) -- exposed for tests of the in-kernel generator */
int cgen_philox_normal(float* out, int64_t count, const uint64_t* rng, uint32_t stream_id, cgen_stream_t);
/* Philox uniform fill (f32 contiguous): out[i] = u01(word (i & 3) of the 4 x 32 bits of (seed, offset, stream_id, i >> 2)), with
 * u01(r) = ((r >> 8) + 0.5) 2^-24 -- open at both ends, so log(-log u) is finite.  {seed, offset} are read from `rng` when the
 * kernel runs and are not advanced; plain stores, no atomics: reruns are bit-identical.  count == 0 returns CGEN_OK before any
 * device work.  PgmCounterfactual.run(rng=) fills the Gumbel-max uniforms of cgen_pgm_counterfactual with it, stream id 989 + k
 * for a PGM's k-th Gumbel-max mechanism (989 .. 996 are reserved for that; the table of taken ids is in csrc/common.h). */
int cgen_philox_uniform(float* out, int64_t count, const uint64_t* rng, uint32_t stream_id, cgen_stream_t stream);
/* rng[1] += inc (device-side counter bump so graph replays draw fresh noise) */
int cgen_rng_advance(uint64_t* rng, uint64_t inc, cgen_stream_t);

#ifdef __cplusplus
}
#endif
#endif /* CGEN_HIP_H */
