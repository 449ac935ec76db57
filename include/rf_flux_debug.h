/* rf_flux_debug.h -- measurement and introspection entry points of librf_flux.so.
 *
 * NOT part of the drop-in boundary (include/rf_flux.h): nothing here is needed to run the path, nothing here selects a kernel or
 * changes a result.  bench.py's roofline block, tools/ and the tests use them:
 *   rf_time_gemm*            hipEvent timing of one GEMM descriptor, isolated re-launches
 *   rf_profile_begin / _end  in-sequence per-launch timing of everything the library launches (the `roofline` numbers)
 *   rf_debug_last_*_path     which kernel form the LAST launch of a family took (read-only)
 *   rf_debug_sk_plan, rf_debug_attn_mix_plan   the host-side work plans (pure arithmetic, callable without a GPU)
 *   rf_debug_clock_probe     the shader clock a probed launch saw (rf_gemm_desc.clock_probe / an open profile)
 *   rf_debug_text_attention  one launch of the text / CLIP towers' attention kernels on caller buffers (kernel-level parity tests)
 *   rf_debug_vae_op          one op of the VAE (GroupNorm, 3x3 convolution, upsample, downsample, attention) on caller buffers
 *   rf_debug_workspace_layout, rf_debug_text_workspace_layout   where the regions of an rf_workspace lie (pure arithmetic, callable without a GPU)
 */
#ifndef RF_FLUX_DEBUG_H
#define RF_FLUX_DEBUG_H
#include "rf_flux.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Kernel-level timing hook used by bench.py: time `iters` launches of the dominant GEMM
 * shape with hipEvents on `stream`; returns average microseconds in *us. */
int rf_time_gemm(const rf_gemm_desc* d, int32_t iters, float* us, void* stream);
int rf_time_gemm_w8a8(const rf_gemm_desc* d, int32_t iters, float* us, void* stream);

/* In-sequence timing hook (bench.py's `roofline`): between rf_profile_begin and rf_profile_end every launch site of
 * the library records ONE hipEvent on ITS launch stream in front of its kernel(s); rf_profile_end records a closing
 * event.  A launch's duration is the distance to the next event (kernel + the gap behind it), so the durations are
 * those of the kernels inside the real 57-block sequence (cold operands, real neighbours), not of isolated
 * re-launches, and the per-class sums add up exactly to the wall time between the first and the closing event.
 * rf_profile_end synchronises, then fills, per rf_kernel_class: summed duration (us), launch count and summed
 * algorithmic work (FLOPs: 2MNK per GEMM over all groups and K-segments, 4*S^2*128*heads per attention launch;
 * BYTES read+written for the row kernels).  `dropped` = launches beyond max_launches (not timed).
 * Not thread-safe, single stream, not for use during hipGraph capture; costs one event record per launch while open. */
typedef enum rf_kernel_class {
  RF_KC_GEMM_MAIN = 0,   /* 256x256-tile MFMA GEMM launches (tile-per-block ping-pong loop and stream-K) */
  RF_KC_GEMM_SMALL = 1,  /* 128x128-tile launches (embedders, LoRA down-projections incl. split-K + reduce) */
  RF_KC_ATTN = 2,        /* rf_attention / rf_attention_fwd */
  RF_KC_ROWOP = 3,       /* LayerNorm+modulate, RMSNorm+RoPE, Euler, SiLU, add */
  RF_KC_GEMM_W8 = 4,     /* fp8-weight GEMM launches (rf_gemm_w8a8) */
  RF_KC_QUANT = 5,       /* activation quantisation row kernels of the fp8 path */
  RF_KC_ATTN_BWD = 6,    /* rf_attention_bwd (work = 5 products x 2 S^2 128 per head = 2.5 x the forward's) */
  RF_KC_COUNT = 7
} rf_kernel_class;
int rf_profile_begin(int32_t max_launches);
int rf_profile_end(double* us_sum /*[RF_KC_COUNT]*/, int64_t* launches /*[RF_KC_COUNT]*/,
                   double* work_sum /*[RF_KC_COUNT]*/, int32_t* dropped /* may be NULL */);

/* Read-only introspection (no setter exists: a launch's schedule / kernel travels in ITS descriptor).
 * rf_debug_last_gemm_path: 0 = one tile per workgroup, 1 = split-K, 2 = stream-K / persistent whole tiles.
 * rf_debug_last_attn_path: 1 / 2 / 4 / 5 = kernel version, 6 = v5 split launch, 8 = v5 lagged-max, 9 = its split launch, 10 / 11 = the
 * mixed-size launch of the bounded / lagged-max kernel.  rf_debug_last_attn_bwd_path: the RF_ATTN_BWD_* pair the last backward ran. */
int rf_debug_last_gemm_path(void);
int rf_debug_last_attn_path(void);
int rf_debug_last_attn_bwd_path(void);
/* The stream-K plan `d` would get on a device with num_cus compute units (pure host arithmetic, no launch).  Returns 1 = plan made,
 * 0 = the launch does not qualify, < 0 error.  out (>= 51 ints): [0..4] first K-tile iteration per group (+ total), [5..8] K-tiles per
 * tile per group, then per XCD chunk x < 8: [9+x] first tile, [17+x] whole-tile rounds, [25+x] / [33+x] first / one-past-last iteration
 * of the stream-K region; [41] tiles_n, [42..45] tiles_m per group, [46..49] tile_start per group, [50] total tiles. */
int rf_debug_sk_plan(const rf_gemm_desc* d, int32_t num_cus, int32_t* out);
/* The mixed-size attention launch for S keys x heads on num_cus CUs: out = {256-query workgroups per head, 192-query workgroups per
 * head, 1000 x simulated makespan in units of a 256-query workgroup, plain-grid rounds}. */
int rf_debug_attn_mix_plan(int32_t S, int32_t heads, int32_t num_cus, int32_t* out);
/* which: 0 = the last probed 256x256 GEMM launch, 1 = the last bounded-score attention launch, 2 = the GEMM's epilogue (end of main
 * loop -> stores acknowledged).  mhz = shader clocks per microsecond over workgroup 0's region, us = its duration.  Synchronise first. */
int rf_debug_clock_probe(int which, double* mhz, double* us);
/* One launch of the text / CLIP towers' attention (head_dim 64: T5, CLIP-L text, ViT-L; 80: ViT-H/14) on caller buffers, through the
 * launch code the towers use (same LDS size, grid and instantiation): out = softmax(scale * q.k^T + bias) v per head and sequence, bf16.
 * B sequences of S tokens, each owning S_pad rows (S_pad % 32 == 0, <= 512 keys at head_dim 64, <= 480 at 80): rows of q [.][ldq],
 * k [.][ldk] and out [.][ldo] of sequence z start at z * S_pad, head h in columns h * head_dim ...; vt [heads * head_dim][ldvt] is V
 * transposed (row = channel, column = key) with sequence z's keys at columns z * S_pad.  bias: fp32 [.][S_pad][S_pad] with head stride
 * bias_hs (0 = shared by the heads); it must hold -inf in the key columns >= S and may be NULL only when S == S_pad.  Rows >= S of out
 * are not written; rows / keys >= S of q, k, vt must be finite.  qi: 1 | 4 = 64 | 256 queries per workgroup, 0 = the product's rule
 * (4 when heads * B * ceil(S_pad / 256) >= 256).  Pointers 16-byte aligned, pitches multiples of 8 elements.  Not a switch: it
 * changes nothing about any other launch. */
int rf_debug_text_attention(int32_t head_dim, int32_t qi, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                            const float* bias, int64_t bias_hs, void* out, int64_t ldo, int32_t heads, int32_t B, int32_t S, int32_t S_pad,
                            float scale, void* stream);

/* ONE op of the VAE (csrc/vae.hip) on caller buffers, through the host functions rf_vae_decode / rf_vae_encode run (same grids, same
 * kernel instantiations, same fold / schedule decisions).  Images are zero-halo NHWC bf16 as in rf_flux.h; "compact" = [H*W][C] without
 * the halo.  Every argument is validated before the first HIP call.  Not a switch: it changes nothing about any other launch.
 *   GROUP_NORM  out = [silu](group_norm(in)); in padded [(H+2)(W+2)][C] (its halo is not read), `norm`, `groups`; out compact, or padded
 *               with a zero halo FOLLOWED BY RF_VAE_TAIL_PIXELS zeroed pixels (what a folded convolution behind it may read)
 *   CONV3X3     out = [residual +] conv(in); in padded [..][conv->cin] with a CLEAN zero halo (+ the tail above when it runs folded), out /
 *               residual padded [..][conv->cout]; residual may alias out.  Rows (W+3) .. of out are written: the interior, the halo columns
 *               between (garbage) and, folded, up to fold - 1 pixels of the bottom halo row
 *   UPSAMPLE2X  in padded [(H+2)(W+2)][C] (halo not read) -> out padded [(2H+2)(2W+2)][C], zero halo + zeroed tail as GROUP_NORM
 *   DOWNSAMPLE  3x3 / stride 2 over F.pad(in, (0,1,0,1)): in padded [(H+2)(W+2)][conv->cin] (halo not read), H, W even -> out padded
 *               [(H/2+2)(W/2+2)][conv->cout], rows (W/2+3) .. written as CONV3X3 (conv->w in the plain [cout][3][3][cin] layout)
 *   ATTN_CORE   vae_attn_kernel alone: in = qk [S][1024] (q | k), residual = vt [512][S], out [S][512]; S = H*W, C = 512
 *   ATTN_BLOCK  the mid-block attention in place: out = padded [(H+2)(W+2)][512], x += to_out(attn(group_norm(x))); halo neither read
 *               nor written; `attn`, `groups`; `in` unused
 *   ATTN_CORE and ATTN_BLOCK take S = H*W % 64 == 0 only (the kernel without a key tail); the two ops below take ANY S >= 1 and run that
 *   same kernel when S % 64 == 0, its ragged instantiation (last key tile masked) otherwise.  S_pad = S rounded up to a multiple of 64.
 *   ATTN_CORE_RAGGED   in = qk [S_pad][1024] (q | k), residual = vt [512][S_pad] (row pitch S_pad), out [S][512]; rows S .. of qk and
 *               columns S .. of a vt row may hold anything (NaN included): no result depends on them; neither input is written
 *   ATTN_BLOCK_RAGGED  the contract of ATTN_BLOCK
 * ws == NULL (or ws->base == NULL): returns the workspace bytes the op needs (> 0) instead of running; the workspace's contents on
 * entry do not matter.  Otherwise returns RF_OK or an RF_ERR_* status. */
#define RF_VAE_TAIL_PIXELS 64
typedef enum rf_vae_op {
  RF_VAE_OP_GROUP_NORM = 0, RF_VAE_OP_CONV3X3 = 1, RF_VAE_OP_UPSAMPLE2X = 2, RF_VAE_OP_DOWNSAMPLE = 3, RF_VAE_OP_ATTN_CORE = 4,
  RF_VAE_OP_ATTN_BLOCK = 5, RF_VAE_OP_ATTN_CORE_RAGGED = 6, RF_VAE_OP_ATTN_BLOCK_RAGGED = 7
} rf_vae_op;
typedef struct rf_vae_op_desc {
  int32_t op;                       /* rf_vae_op */
  int32_t H, W, C, groups;          /* INPUT geometry; C: GROUP_NORM / UPSAMPLE2X / ATTN_* (the convolutions carry cin / cout) */
  int32_t silu, compact;            /* GROUP_NORM */
  int32_t _pad;
  const rf_vae_norm* norm;          /* GROUP_NORM */
  const rf_vae_conv* conv;          /* CONV3X3, DOWNSAMPLE */
  const rf_vae_attn* attn;          /* ATTN_BLOCK, ATTN_BLOCK_RAGGED */
  const void* in; void* out; const void* residual;
  const rf_workspace* ws;
} rf_vae_op_desc;
int64_t rf_debug_vae_op(const rf_vae_op_desc* d, void* stream);

/* The regions the engine entry points (rf_double_block_fwd ... rf_flux_denoise_guided) carve out of an rf_workspace of rf_workspace_bytes(dims):
 * out[2 i] = byte offset, out[2 i + 1] = byte length of region i, in this order (14 pairs; n = the pairs `out` has room for, >= 14):
 *   0 xn   1 q   2 k   3 vt   4 att   5 hid   6 lt   7 x   8 sk_flags   9 sk_partials   10 xn8   11 a8   12 s_xn   13 s_a
 * (q, k, vt with their rows / key columns S .. s_pad; length 0 for the four fp8 regions when dims->fp8 == 0).  Regions start on 256-byte
 * boundaries, so up to 255 unused bytes follow each.  sk_flags is the one region whose contents matter on entry (rf_workspace in rf_flux.h).
 * Returns the number of pairs or an RF_ERR_* status; launches nothing, changes no state. */
int rf_debug_workspace_layout(const rf_flux_dims* dims, int64_t* out, int32_t n);
/* The same for a tower workspace (rf_t5_encode, rf_clip_text_encode[_opts], rf_clip_vision_encode[_opts]) of total_bytes = the answer of
 * its rf_*_workspace_bytes query: 2 pairs, 0 sk_flags, 1 sk_partials (the scratch of the towers' stream-K / split-K GEMMs, carved last).
 * The towers zero their flag page themselves on every call. */
int rf_debug_text_workspace_layout(int64_t total_bytes, int64_t* out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RF_FLUX_DEBUG_H */
