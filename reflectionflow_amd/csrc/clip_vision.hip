// CLIP-score verifier on the HIP path: transformers' CLIPModel (clip-vit-large-patch14 layout) applied to what the
// reference's verifier reads -- the candidate's 8-bit PNG (tts/tts_reflectionflow.py:157-170, 345-352) -- and scored against the
// original prompt.  New here: the image preprocessing (8-bit levels -> CLIPImageProcessor's resize / crop / normalise -> im2col patch
// rows), the token assembly row kernel and the fused normalise-and-dot score.  The encoder layers are the text tower's
// (text.hip clip_layers: bf16 MFMA GEMM, attn64_kernel, rf_layernorm_modulate); the attention masks the padded keys (T = 257 tokens
// of ViT-L/14 at 224 live in S_pad = 288 rows; the 577 tokens of ViT-L/14 at 336 in 608, which text.hip's launch site serves with
// attn64_stream_kernel: head dim 64 takes up to 2048 keys, head dim 80 up to 480).  rf_clip_tower_opts picks the head dim (64 | 80: attn64_kernel / attn80_kernel) and the
// activation (quick_gelu | gelu) per call: ViT-H/14 (PickScore, HPSv2, LAION CLIP-H) is hidden 1280 = 16 heads x 80 with erf GELU.
//
// Batch invariance.  The search orders candidates by these scores and a rank scores its own candidates in one call, so a row's value
// must not depend on how many images share the call (tts/search.py: score_batch implementations are row-wise batch-invariant).
//   * every projection runs with rf_gemm_desc.schedule = RF_SCHED_TILE256 and no split-K scratch: dispatch() then launches one
//     256x256 tile per workgroup that walks the WHOLE K range in order (sk_mode() is 0 for TILE256, the split-K branch is 128-tile
//     only), so an output element's K order is fixed whatever M is.  AUTO (the text towers' policy) picks 128 / 256 tiles, split-K
//     or stream-K from M -- i.e. from the batch size;
//   * attn64_kernel's / attn80_kernel's QI variant (picked from heads * B) only regroups query tiles into workgroups: each query row's scores, softmax
//     and PV sums run in the same order in both;
//   * LayerNorm, token assembly, preprocessing and the score are one row / image per thread group.
#include "text_internal.hpp"

namespace rf {

// ---- preprocessing --------------------------------------------------------------------------------------------------------------
// PIL's / torch's antialiased bicubic filter (a = -0.5)
__device__ __forceinline__ float aa_bicubic(float x) {
  const float a = -0.5f;
  x = fabsf(x);
  if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
  return 0.0f;
}

// Source window of output pixel i for an in_size -> in_size / scale resize (PIL's precompute_coeffs, torch's antialias path): taps
// lo .. lo + n - 1, weight of tap j = aa_bicubic((j - center + 0.5) * invscale) / total.
struct AaWin { int lo, n; float center, invscale, total; };
__device__ __forceinline__ AaWin aa_window(int i, float scale, int in_size) {
  AaWin r;
  const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
  r.center = scale * ((float)i + 0.5f);
  r.invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
  r.lo = max((int)(r.center - support + 0.5f), 0);
  r.n = min((int)(r.center + support + 0.5f), in_size) - r.lo;
  r.total = 0.0f;
  for (int j = 0; j < r.n; ++j) r.total += aa_bicubic(((float)(r.lo + j) - r.center + 0.5f) * r.invscale);
  return r;
}
__device__ __forceinline__ float aa_weight(const AaWin& w, int j) {
  return aa_bicubic(((float)(w.lo + j) - w.center + 0.5f) * w.invscale) / w.total;
}

constexpr int CP_MAX_SIDE = 8192;   // source rows are staged whole (3 channels fp32) in LDS: 96 KiB at 8192 pixels
constexpr int CP_MAX_SIZE = 512;    // crop side: a workgroup of 256 threads owns one crop row, a thread NX = 1 (size <= 256) or 2 of its columns

// One workgroup per (crop row y, image): the vertical window's source rows are staged one at a time in LDS as 8-bit levels (fp32),
// thread x filters its crop column horizontally out of LDS, rounds and clips that to 8 bits (PIL's 8-bit resample keeps the horizontal
// pass as an 8-bit image; next to saturated edges the clipped overshoot moves the result by up to 7 levels) and accumulates it with
// the vertical weight; the result is rounded to a level, normalised and scattered to its im2col slot.  Row y = py * patch (ky = 0) also zeroes the K padding of patch row py.
// NX: crop columns per thread (x = tid + 256 n).  The one structural cap on `size` is this mapping (a crop row = one workgroup, its
// horizontal windows and accumulators in registers): NX = 1 is the kernel as it always was (size <= 256, same operations in the same
// order), NX = 2 carries CLIP's 336- and 448-pixel processors, up to CP_MAX_SIZE = 512.  Nothing else depends on size: the LDS holds
// source rows (<= 8192 pixels) and the tap weights are recomputed per tap, there is no table.
template <int NX>
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const bf16_t* __restrict__ img, int64_t s_img, int64_t s_row, int64_t s_pix, int64_t s_ch,
                                                              int H, int W, float a, float b, int newH, int newW, int top, int left, int size,
                                                              int patch, int K_pad, bf16_t* __restrict__ out) {
#pragma clang fp contract(off)   // the levels and the normalisation are the host restatement's fp32 operations, one rounding each
  extern __shared__ float row[];   // [3][span]
  const int y = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x;
  const bf16_t* src = img + (int64_t)bi * s_img;
  const float sy = (float)H / (float)newH, sx = (float)W / (float)newW;
  const AaWin vy = aa_window(top + y, sy, H);
  const AaWin wx0 = aa_window(left, sx, W), wx1 = aa_window(left + size - 1, sx, W);
  const int sx0 = wx0.lo, span = wx1.lo + wx1.n - sx0;   // windows move right with the output pixel: [sx0, sx0 + span) covers the crop
  bool act[NX];
  AaWin wx[NX];
  float acc[NX][3];
#pragma unroll
  for (int n = 0; n < NX; ++n) {
    act[n] = tid + 256 * n < size;
    wx[n] = aa_window(left + (act[n] ? tid + 256 * n : 0), sx, W);
    acc[n][0] = acc[n][1] = acc[n][2] = 0.0f;
  }
  const bool ch_fast = s_ch <= s_pix;
  for (int j = 0; j < vy.n; ++j) {
    const int yy = vy.lo + j;
    __syncthreads();
    for (int idx = tid; idx < 3 * span; idx += 256) {
      int p, c;
      if (ch_fast) { p = idx / 3; c = idx - 3 * p; }
      else { c = idx / span; p = idx - c * span; }
      const float v = bf2f(src[(int64_t)yy * s_row + (int64_t)(sx0 + p) * s_pix + (int64_t)c * s_ch]);
      const float u = fminf(fmaxf(a * v + b, 0.0f), 1.0f);
      row[c * span + p] = rintf(u * 255.0f);                 // the PNG's 8-bit level (numpy's round: half to even)
    }
    __syncthreads();
    const float wy = aa_weight(vy, j);
#pragma unroll
    for (int n = 0; n < NX; ++n) {
      if (act[n]) {
        const float* r = row + (wx[n].lo - sx0);
        float h[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < wx[n].n; ++i) {
          const float w = aa_weight(wx[n], i);
#pragma unroll
          for (int c = 0; c < 3; ++c) h[c] += w * r[c * span + i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[n][c] += wy * rintf(fminf(fmaxf(h[c], 0.0f), 255.0f));   // PIL's 8-bit intermediate image
      }
    }
  }
  const int gp = size / patch, py = y / patch, ky = y - py * patch, pp = patch * patch;
#pragma unroll
  for (int n = 0; n < NX; ++n) {
    if (act[n]) {
      const float MEAN[3] = {0.48145466f, 0.4578275f, 0.40821073f}, STD[3] = {0.26862954f, 0.26130258f, 0.27577711f};
      const int x = tid + 256 * n, px = x / patch, kx = x - px * patch;
      bf16_t* o = out + ((int64_t)bi * gp * gp + (int64_t)py * gp + px) * K_pad + ky * patch + kx;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float l = rintf(fminf(fmaxf(acc[n][c], 0.0f), 255.0f));   // 8-bit resize output
        const float v = l * (1.0f / 255.0f);
        o[c * pp] = f2bf((v - MEAN[c]) / STD[c]);
      }
    }
  }
  if (ky == 0) {
    const int npad = K_pad - 3 * pp;
    for (int idx = tid; idx < gp * npad; idx += 256) {
      const int px = idx / npad, k = 3 * pp + (idx - px * npad);
      out[((int64_t)bi * gp * gp + (int64_t)py * gp + px) * K_pad + k] = f2bf(0.0f);
    }
  }
}

// ---- SiglipImageProcessor: PIL's 8-bit resample, exactly ---------------------------------------------------------------------------
// Pillow's 8-bit resampler is INTEGER arithmetic (Resample.c): per axis the bicubic weights are formed in double, normalised, turned
// into 22-bit fixed-point coefficients (round half away from zero), and a pass gives clip8(((1 << 21) + sum level * coef) >> 22).
// The float filter of clip_preprocess_kernel above differs from it by one level in a few percent of the pixels, so SigLIP's
// preprocessing, which is held to PIL level for level, restates Pillow's own arithmetic -- the arithmetic image_handoff.hip's
// rf_pil_resize_to_vae_input runs from host-built tables, here with the coefficients recomputed per tap in double on the device (no
// table: the entry point has no workspace; +, *, / in double are IEEE on both sides, contraction is off).
__device__ __forceinline__ double pil_bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
struct PilWin { int lo, n; double center, ss, ww; };
__device__ __forceinline__ PilWin pil_window(int i, int in_size, int out_size) {   // precompute_coeffs, one output pixel
#pragma clang fp contract(off)
  PilWin r;
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  r.center = (i + 0.5) * scale;
  r.ss = 1.0 / filterscale;
  r.lo = (int)(r.center - support + 0.5);
  if (r.lo < 0) r.lo = 0;
  int hi = (int)(r.center + support + 0.5);
  if (hi > in_size) hi = in_size;
  r.n = hi - r.lo;
  r.ww = 0.0;
  for (int x = 0; x < r.n; ++x) r.ww += pil_bicubic((x + r.lo - r.center + 0.5) * r.ss);
  return r;
}
__device__ __forceinline__ int pil_coef(const PilWin& w, int x) {   // normalize_coeffs_8bpc of tap x
#pragma clang fp contract(off)
  double k = pil_bicubic((x + w.lo - w.center + 0.5) * w.ss);
  if (w.ww != 0.0) k /= w.ww;
  return k < 0 ? (int)(-0.5 + k * 4194304.0) : (int)(0.5 + k * 4194304.0);
}
__device__ __forceinline__ int pil_clip8(int ss) { return min(max(ss >> 22, 0), 255); }

// clip_preprocess_kernel's structure (one workgroup per output row and image, the vertical window's source rows staged one at a time
// in LDS, thread x owns output columns x + 256 n, im2col scatter, K padding zeroed by the rows with ky == 0) with the arithmetic above:
// both axes go straight to `size`, the horizontal pass of a source row is clipped to 8 bits before the vertical pass accumulates it,
// then (v / 255 - 0.5) / 0.5 in fp32, one rounding to bf16.  The patch convolution is "valid": of the size x size image only the first
// used = (size / patch) * patch rows and columns reach a patch (so400m/14 at 384 px: 27 x 14 = 378), the grid has `used` rows.
template <int NX>
__global__ __launch_bounds__(256) void siglip_preprocess_kernel(const bf16_t* __restrict__ img, int64_t s_img, int64_t s_row, int64_t s_pix, int64_t s_ch,
                                                                int H, int W, float a, float b, int size, int used, int patch, int K_pad,
                                                                bf16_t* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ int lrow[];   // [3][span]
  const int y = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x;
  const bf16_t* src = img + (int64_t)bi * s_img;
  const PilWin vy = pil_window(y, H, size);
  const PilWin wx0 = pil_window(0, W, size), wx1 = pil_window(used - 1, W, size);
  const int sx0 = wx0.lo, span = wx1.lo + wx1.n - sx0;
  bool act[NX];
  PilWin wx[NX];
  int acc[NX][3];
#pragma unroll
  for (int n = 0; n < NX; ++n) {
    act[n] = tid + 256 * n < used;
    wx[n] = pil_window(act[n] ? tid + 256 * n : 0, W, size);
    acc[n][0] = acc[n][1] = acc[n][2] = 1 << 21;
  }
  const bool ch_fast = s_ch <= s_pix;
  for (int j = 0; j < vy.n; ++j) {
    const int yy = vy.lo + j;
    __syncthreads();
    for (int idx = tid; idx < 3 * span; idx += 256) {
      int p, c;
      if (ch_fast) { p = idx / 3; c = idx - 3 * p; }
      else { c = idx / span; p = idx - c * span; }
      const float v = bf2f(src[(int64_t)yy * s_row + (int64_t)(sx0 + p) * s_pix + (int64_t)c * s_ch]);
      const float u = fminf(fmaxf(a * v + b, 0.0f), 1.0f);
      lrow[c * span + p] = (int)rintf(u * 255.0f);                 // the PNG's 8-bit level (numpy's round: half to even)
    }
    __syncthreads();
    const int cy = pil_coef(vy, j);
#pragma unroll
    for (int n = 0; n < NX; ++n) {
      if (act[n]) {
        const int* r = lrow + (wx[n].lo - sx0);
        int h[3] = {1 << 21, 1 << 21, 1 << 21};
        for (int i = 0; i < wx[n].n; ++i) {
          const int k = pil_coef(wx[n], i);
#pragma unroll
          for (int c = 0; c < 3; ++c) h[c] += r[c * span + i] * k;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[n][c] += pil_clip8(h[c]) * cy;   // PIL's 8-bit intermediate image
      }
    }
  }
  const int gp = used / patch, py = y / patch, ky = y - py * patch, pp = patch * patch;
#pragma unroll
  for (int n = 0; n < NX; ++n) {
    if (act[n]) {
      const int x = tid + 256 * n, px = x / patch, kx = x - px * patch;
      bf16_t* o = out + ((int64_t)bi * gp * gp + (int64_t)py * gp + px) * K_pad + ky * patch + kx;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (float)pil_clip8(acc[n][c]) * (1.0f / 255.0f);
        o[c * pp] = f2bf((v - 0.5f) / 0.5f);
      }
    }
  }
  if (ky == 0) {
    const int npad = K_pad - 3 * pp;
    for (int idx = tid; idx < gp * npad; idx += 256) {
      const int px = idx / npad, k = 3 * pp + (idx - px * npad);
      out[((int64_t)bi * gp * gp + (int64_t)py * gp + px) * K_pad + k] = f2bf(0.0f);
    }
  }
}

// ---- token assembly: X[b * S_pad + t] = class + pos[0] (t = 0) | patch row t - 1 + pos[t] (t < T) | 0; D % 8 == 0 ------------------
__global__ __launch_bounds__(256) void clip_tokens_kernel(const bf16_t* __restrict__ P, const bf16_t* __restrict__ cls, const bf16_t* __restrict__ pos,
                                                          bf16_t* __restrict__ X, int np, int S_pad, int n_rows, int D) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d8 = D >> 3;
  if (idx >= (int64_t)n_rows * d8) return;
  const int grow = (int)(idx / d8), c = (int)(idx % d8) * 8;
  const int b = grow / S_pad, t = grow - b * S_pad;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (t <= np) {
    float x[8], p[8];
    unpack8(*(const u32x4*)((t == 0 ? cls : P + ((int64_t)b * np + t - 1) * D) + c), x);
    unpack8(*(const u32x4*)(pos + (int64_t)t * D + c), p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] += p[i];
    v = pack8(x);
  }
  *(u32x4*)(X + (int64_t)grow * D + c) = v;
}

// ---- score: one workgroup per image row, fixed reduction order --------------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_score_kernel(const bf16_t* __restrict__ img, const bf16_t* __restrict__ txt, float logit_scale,
                                                         float* __restrict__ scores, int P) {
  __shared__ float red[3][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* r = img + (int64_t)b * P;
  float ii = 0.0f, tt = 0.0f, it = 0.0f;
  for (int p = tid; p < P; p += 256) {
    const float x = bf2f(r[p]), t = bf2f(txt[p]);
    ii += x * x; tt += t * t; it += x * t;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    ii += __shfl_xor(ii, o); tt += __shfl_xor(tt, o); it += __shfl_xor(it, o);
  }
  if (lane == 0) { red[0][w] = ii; red[1][w] = tt; red[2][w] = it; }
  __syncthreads();
  if (tid == 0) {
    const float si = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const float st = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const float d = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    scores[b] = expf(logit_scale) * (d / (sqrtf(si) * sqrtf(st)));
  }
}

// SigLIP's pairwise sigmoid on clip_score_kernel's reduction (same order, a kernel of its own: clip_score_kernel's results are pinned):
// p = 1 / (1 + exp(-(exp(logit_scale) * cos + logit_bias))), label = p >= threshold
__global__ __launch_bounds__(256) void siglip_score_kernel(const bf16_t* __restrict__ img, const bf16_t* __restrict__ txt, float logit_scale, float logit_bias,
                                                           float threshold, float* __restrict__ scores, int32_t* __restrict__ labels, int P) {
  __shared__ float red[3][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* r = img + (int64_t)b * P;
  float ii = 0.0f, tt = 0.0f, it = 0.0f;
  for (int p = tid; p < P; p += 256) {
    const float x = bf2f(r[p]), t = bf2f(txt[p]);
    ii += x * x; tt += t * t; it += x * t;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    ii += __shfl_xor(ii, o); tt += __shfl_xor(tt, o); it += __shfl_xor(it, o);
  }
  if (lane == 0) { red[0][w] = ii; red[1][w] = tt; red[2][w] = it; }
  __syncthreads();
  if (tid == 0) {
    const float si = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const float st = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const float d = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    const float z = expf(logit_scale) * (d / (sqrtf(si) * sqrtf(st))) + logit_bias;
    const float p = 1.0f / (1.0f + expf(-z));
    scores[b] = p;
    if (labels) labels[b] = p >= threshold ? 1 : 0;
  }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_clip_preprocess(const void* img, int64_t s_img, int64_t s_row, int64_t s_pix, int64_t s_ch, int32_t B, int32_t H, int32_t W, float a,
                                  float b, int32_t size, int32_t patch, void* patches, void* stream) {
  RF_REQUIRE(img && patches, RF_ERR_NULL, "rf_clip_preprocess: NULL tensor");
  RF_REQUIRE(B > 0 && H > 0 && W > 0 && H <= CP_MAX_SIDE && W <= CP_MAX_SIDE, RF_ERR_SHAPE, "rf_clip_preprocess: B=%d H=%d W=%d (sides 1 .. %d)", B, H,
             W, CP_MAX_SIDE);
  RF_REQUIRE(size > 0 && size <= CP_MAX_SIZE && patch > 0 && size % patch == 0, RF_ERR_SHAPE, "rf_clip_preprocess: size=%d patch=%d (size <= %d, %% patch == 0)",
             size, patch, CP_MAX_SIZE);
  RF_REQUIRE(s_row > 0 && s_pix > 0 && s_ch > 0 && (B == 1 || s_img > 0), RF_ERR_SHAPE, "rf_clip_preprocess: strides must be positive");
  // CLIPImageProcessor: shortest edge -> size, long edge int(size * long / short) (transformers' get_resize_output_image_size)
  int newH, newW;
  if (W <= H) { newW = size; newH = (int)((double)size * H / W); }
  else { newH = size; newW = (int)((double)size * W / H); }
  const int top = (newH - size) / 2, left = (newW - size) / 2;
  const int K_pad = (int)round_up(3 * patch * patch, 64);
  static bool attr = false;
  if (!attr) {
    RF_CHECK_HIP(hipFuncSetAttribute((const void*)clip_preprocess_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CP_MAX_SIDE * 4));
    RF_CHECK_HIP(hipFuncSetAttribute((const void*)clip_preprocess_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CP_MAX_SIDE * 4));
    attr = true;
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(RF_KC_ROWOP, (double)B * size * size * 3 * 2, st);
  auto* const kern = size <= 256 ? clip_preprocess_kernel<1> : clip_preprocess_kernel<2>;
  hipLaunchKernelGGL(kern, dim3(size, B), dim3(256), 3 * W * 4, st, (const bf16_t*)img, s_img, s_row, s_pix, s_ch, H, W, a, b, newH,
                     newW, top, left, size, patch, K_pad, (bf16_t*)patches);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

static int vision_check(const rf_clip_vision_weights* w, const rf_clip_tower_opts* o, const char* who) {
  RF_REQUIRE(w && w->layer && w->patch_w && w->class_embed && w->pos_embed && w->pre_ln_scale && w->pre_ln_shift && w->post_ln_scale &&
                 w->post_ln_shift && w->proj && w->mask, RF_ERR_NULL, "%s: weights NULL", who);
  RF_REQUIRE(w->layers > 0 && w->heads > 0 && w->hidden > 0 && w->hidden % 8 == 0 && w->hidden <= 4096 && w->inter > 0 && w->inter % 64 == 0 &&
                 w->proj_dim > 0 && w->proj_dim % 8 == 0, RF_ERR_SHAPE, "%s: layers=%d heads=%d hidden=%d inter=%d proj_dim=%d (need hidden %% 8 == 0, <= 4096, "
             "inter %% 64 == 0, proj_dim %% 8 == 0)", who, w->layers, w->heads, w->hidden, w->inter, w->proj_dim);
  RF_REQUIRE(w->patch > 0 && w->image_size > 0 && w->image_size % w->patch == 0, RF_ERR_SHAPE, "%s: image_size=%d patch=%d", who, w->image_size, w->patch);
  const int g = w->image_size / w->patch, T = g * g + 1;
  // head dim 80: as ever (clip_opts_check below then holds S_pad to the 480 resident keys); head dim 64: the streaming-keys limit
  const int lim = o && o->head_dim == 80 ? TA_MAXS : text_attn_stream_max_keys(64);
  RF_REQUIRE(T <= lim, RF_ERR_SHAPE, "%s: %d tokens > %d", who, T, lim);
  RF_REQUIRE(w->mask_S == (int)round_up(T, 32), RF_ERR_SHAPE, "%s: mask is built for S_pad = %d, %d tokens need %d", who, w->mask_S, T, (int)round_up(T, 32));
  return clip_opts_check(o, w->hidden, w->heads, w->mask_S, who);
}

extern "C" int64_t rf_clip_vision_workspace_bytes_opts(const rf_clip_vision_weights* w, const rf_clip_tower_opts* o, int32_t B) {
  const int rc = vision_check(w, o, "rf_clip_vision_workspace_bytes");
  if (rc != RF_OK) return rc;
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_clip_vision_workspace_bytes: B=%d (1 .. 64)", B);
  const int Dp = (int)round_up(w->hidden, 64);
  return text_sizes(B * w->mask_S, Dp, Dp, w->inter, w->inter).total;
}

extern "C" int64_t rf_clip_vision_workspace_bytes(const rf_clip_vision_weights* w, int32_t B) {
  const int64_t n = rf_clip_vision_workspace_bytes_opts(w, &CLIP_L_OPTS, B);
  return n < 0 ? RF_ERR_SHAPE : n;
}

// CLIPVisionModel + visual_projection: patches [B * np][K_pad] -> image_embeds [B][proj_dim].  Workspace use: the patch GEMM's output
// [B * np][D] lives in QK ([R][2D], R = B * S_pad >= B * np), the post-LN class rows [B][Dp] in AO (Dp = D rounded up to the GEMM's
// K-tile; AO's columns D .. Dp - 1 are zero from text_ctx on: the attention writes D columns per row).
extern "C" int rf_clip_vision_encode_opts(const rf_clip_vision_weights* w, const rf_clip_tower_opts* o, const void* patches, int32_t B,
                                          void* image_embeds, const rf_workspace* ws, void* stream) {
  RF_TRY(vision_check(w, o, "rf_clip_vision_encode"));
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_clip_vision_encode: B=%d (1 .. 64)", B);
  RF_REQUIRE(patches && image_embeds && aligned16(patches) && aligned16(image_embeds), RF_ERR_NULL, "rf_clip_vision_encode: NULL / unaligned tensor");
  const int g = w->image_size / w->patch, np = g * g, T = np + 1, S_pad = w->mask_S, D = w->hidden, F = w->inter, R = B * S_pad;
  const int K_pad = (int)round_up(3 * w->patch * w->patch, 64), Dp = (int)round_up(D, 64);
  hipStream_t st = (hipStream_t)stream;
  TextCtx c;
  RF_TRY(text_ctx(c, text_sizes(R, Dp, Dp, F, F), B, T, S_pad, ws, st, "rf_clip_vision_encode"));
  c.sched = RF_SCHED_TILE256;   // batch invariance: see the file header
  RF_TRY(text_gemm(c, (const bf16_t*)patches, K_pad, w->patch_w, nullptr, B * np, D, K_pad, c.QK, D, RF_EPI_STORE, nullptr));
  {
    ProfScope prof(RF_KC_ROWOP, (double)R * D * 6, st);
    hipLaunchKernelGGL(clip_tokens_kernel, dim3((unsigned)cdiv64((int64_t)R * D / 8, 256)), dim3(256), 0, st, c.QK, (const bf16_t*)w->class_embed,
                       (const bf16_t*)w->pos_embed, c.Xn, np, S_pad, R, D);
    RF_LAUNCH_CHECK();
  }
  RF_TRY(rf_layernorm_modulate(c.Xn, D, c.X, D, R, D, w->pre_ln_scale, w->pre_ln_shift, w->eps, st));   // pre_layrnorm -> residual stream
  RF_TRY(clip_layers(c, w->layer, w->layers, w->heads, D, F, w->mask, w->eps, "rf_clip_vision_encode", *o));
  RF_TRY(rf_layernorm_modulate(c.X, (int64_t)S_pad * D, c.AO, Dp, B, D, w->post_ln_scale, w->post_ln_shift, w->eps, st));   // row 0 of each image
  RF_TRY(text_gemm(c, c.AO, Dp, w->proj, nullptr, B, w->proj_dim, Dp, (bf16_t*)image_embeds, w->proj_dim, RF_EPI_STORE, nullptr));
  return RF_OK;
}

extern "C" int rf_clip_vision_encode(const rf_clip_vision_weights* w, const void* patches, int32_t B, void* image_embeds, const rf_workspace* ws,
                                     void* stream) {
  return rf_clip_vision_encode_opts(w, &CLIP_L_OPTS, patches, B, image_embeds, ws, stream);
}

extern "C" int rf_clip_score(const void* img, const void* txt, float logit_scale, float* scores, int32_t B, int32_t P, void* stream) {
  RF_REQUIRE(img && txt && scores, RF_ERR_NULL, "rf_clip_score: NULL tensor");
  RF_REQUIRE(B > 0 && P > 0, RF_ERR_SHAPE, "rf_clip_score: B=%d P=%d", B, P);
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(RF_KC_ROWOP, (double)(B + 1) * P * 2, st);
  hipLaunchKernelGGL(clip_score_kernel, dim3(B), dim3(256), 0, st, (const bf16_t*)img, (const bf16_t*)txt, logit_scale, scores, P);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

extern "C" int rf_siglip_score(const void* img, const void* txt, float logit_scale, float logit_bias, float threshold, float* scores, int32_t* labels,
                               int32_t B, int32_t P, void* stream) {
  RF_REQUIRE(img && txt && scores, RF_ERR_NULL, "rf_siglip_score: NULL tensor");
  RF_REQUIRE(B > 0 && P > 0, RF_ERR_SHAPE, "rf_siglip_score: B=%d P=%d", B, P);
  RF_REQUIRE(threshold >= 0.0f && threshold <= 1.0f, RF_ERR_SHAPE, "rf_siglip_score: threshold=%g (a probability, 0 .. 1)", (double)threshold);
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(RF_KC_ROWOP, (double)(B + 1) * P * 2, st);
  hipLaunchKernelGGL(siglip_score_kernel, dim3(B), dim3(256), 0, st, (const bf16_t*)img, (const bf16_t*)txt, logit_scale, logit_bias, threshold, scores, labels, P);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

// SiglipImageProcessor on the device: rf_clip_preprocess's input contract and im2col output with SigLIP's pipeline -- 8-bit levels, PIL
// resize((size, size), BICUBIC) of both axes straight to `size` (horizontal pass first, rounded and clipped to 8 bits, then the
// vertical pass; up- and down-scaling), (v / 255 - 0.5) / 0.5, bf16.  siglip_preprocess_kernel: Pillow's integer arithmetic.
extern "C" int rf_siglip_preprocess(const void* img, int64_t s_img, int64_t s_row, int64_t s_pix, int64_t s_ch, int32_t B, int32_t H, int32_t W, float a,
                                    float b, int32_t size, int32_t patch, void* patches, void* stream) {
  RF_REQUIRE(img && patches, RF_ERR_NULL, "rf_siglip_preprocess: NULL tensor");
  RF_REQUIRE(B > 0 && H > 0 && W > 0 && H <= CP_MAX_SIDE && W <= CP_MAX_SIDE, RF_ERR_SHAPE, "rf_siglip_preprocess: B=%d H=%d W=%d (sides 1 .. %d)", B, H,
             W, CP_MAX_SIDE);
  RF_REQUIRE(size > 0 && size <= CP_MAX_SIZE && patch > 0 && patch <= size, RF_ERR_SHAPE, "rf_siglip_preprocess: size=%d patch=%d (patch <= size <= %d)", size,
             patch, CP_MAX_SIZE);
  const int used = size / patch * patch;   // the "valid" patch convolution drops the rest (384 = 27 x 14 + 6)
  RF_REQUIRE(s_row > 0 && s_pix > 0 && s_ch > 0 && (B == 1 || s_img > 0), RF_ERR_SHAPE, "rf_siglip_preprocess: strides must be positive");
  const int K_pad = (int)round_up(3 * patch * patch, 64);
  static bool attr = false;
  if (!attr) {
    RF_CHECK_HIP(hipFuncSetAttribute((const void*)siglip_preprocess_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CP_MAX_SIDE * 4));
    RF_CHECK_HIP(hipFuncSetAttribute((const void*)siglip_preprocess_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CP_MAX_SIDE * 4));
    attr = true;
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(RF_KC_ROWOP, (double)B * size * size * 3 * 2, st);
  auto* const kern = size <= 256 ? siglip_preprocess_kernel<1> : siglip_preprocess_kernel<2>;
  hipLaunchKernelGGL(kern, dim3(used, B), dim3(256), 3 * W * 4, st, (const bf16_t*)img, s_img, s_row, s_pix, s_ch, H, W, a, b, size, used, patch, K_pad,
                     (bf16_t*)patches);
  RF_LAUNCH_CHECK();
  return RF_OK;
}
