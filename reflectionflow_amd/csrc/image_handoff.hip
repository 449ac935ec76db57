// The reflection search's round boundary on the device (tts/runner.py): a decoded candidate -> its PNG's 8-bit levels
// (rf_image_levels), and those levels -> the image `PIL.Image.resize((w, h))` returns, as 8-bit levels and as the zero-halo NHWC
// bf16 buffer rf_vae_encode reads (rf_pil_resize_to_vae_input).  Both restate host arithmetic BIT FOR BIT, so a search gives the
// same files, scores and latents whichever side of the bus the boundary runs on:
//   * levels: diffusers' VaeImageProcessor.postprocess -- x = v / 2 + 0.5, clamp to [0, 1], rint(255 x) in fp32, one rounding each
//     (contraction off);
//   * resize: Pillow's 8-bit resampler (ImagingResample, bicubic a = -0.5 with the filter stretched by the scale when reducing): a
//     horizontal pass into an 8-bit image, then a vertical pass over it, each clip8(((1 << 21) + sum level * coeff) >> 22) with the
//     22-bit integer coefficients Pillow's precompute_coeffs / normalize_coeffs_8bpc give.  The caller builds those tables on the
//     host (flux/image_hip.py pil_resize_tables: doubles, once per (in, out)); the kernels are integer only.  An axis whose size does
//     not change is skipped, as Pillow skips it.  (clip_preprocess_kernel's fp32 form of the same filter is a level off on a fraction
//     of pixels -- fine for a score, not for a path that has to reproduce latents.)
//   * encoder input: bf16(2 (level / 255) - 1) has 256 possible values; they come from a table the caller builds with the torch
//     expression it has to equal (VaeImageProcessor.preprocess + .to(bf16)).
// Launch structure: horizontal pass (source window of 256 output pixels staged in LDS with dword loads) -> 8-bit intermediate in
// caller scratch -> vertical pass (a row is 3 w independent bytes: one dword per lane and tap, fully coalesced) -> halo writer
// (16 B per lane; the halo ring and the pad channels are written as zeros).  B images per launch, nothing synchronises.
#include "common.hpp"

namespace rf {

constexpr int IH_MAX_SIDE = 8192;
constexpr int IH_PREC = 22;   // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ uint32_t clip8(int v) { return (uint32_t)min(max(v >> IH_PREC, 0), 255); }

// ---- decoded image -> 8-bit levels: 4 pixels (12 bytes = 3 dwords) per lane -----------------------------------------------------------
__global__ __launch_bounds__(256) void image_levels_kernel(const bf16_t* __restrict__ img, int64_t s_img, int64_t s_row, int64_t s_pix, int64_t s_ch,
                                                           int H, int W, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)   // postprocess's fp32 operations, one rounding each
  const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
  if (x0 >= W) return;
  const bf16_t* src = img + (int64_t)b * s_img + (int64_t)y * s_row;
  uint8_t* o = out + (((int64_t)b * H + y) * W + x0) * 3;
  const int np = min(4, W - x0);
  uint32_t lv[12];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float x = 0.0f;
      if (p < np) x = bf2f(src[(int64_t)(x0 + p) * s_pix + (int64_t)c * s_ch]) / 2.0f + 0.5f;
      x = fminf(fmaxf(x, 0.0f), 1.0f);
      lv[3 * p + c] = (uint32_t)rintf(x * 255.0f);   // numpy's round: half to even
    }
  }
  if ((W & 3) == 0) {   // the row and x0 are multiples of 4 pixels: 12-byte groups on 4-byte boundaries
#pragma unroll
    for (int d = 0; d < 3; ++d) ((uint32_t*)o)[d] = lv[4 * d] | (lv[4 * d + 1] << 8) | (lv[4 * d + 2] << 16) | (lv[4 * d + 3] << 24);
  } else {
    for (int i = 0; i < 3 * np; ++i) o[i] = (uint8_t)lv[i];
  }
}

// ---- horizontal pass: [B][H][W][3] -> [B][H][w][3] --------------------------------------------------------------------------------
// One workgroup per (256 output pixels, row, image).  The chunk's source window [p0, p1) is staged in LDS by aligned dword loads;
// lane x then filters its pixel out of LDS.  lo / cnt / the chunk window are clamped to the row and to the staging buffer, so no table
// content reaches outside either.  coef is tap-major ([kmax][w]): lanes read consecutive ints.
__global__ __launch_bounds__(256) void pil_resize_h_kernel(const uint8_t* __restrict__ src, int H, int W, int w, const int* __restrict__ lo,
                                                           const int* __restrict__ cnt, const int* __restrict__ coef, int kmax, int cap,
                                                           uint8_t* __restrict__ dst) {
  extern __shared__ uint32_t stage[];   // 3 * cap + 8 bytes; reused for the chunk's output bytes
  const int tid = threadIdx.x, x0 = blockIdx.x * 256, y = blockIdx.y, b = blockIdx.z;
  const int nx = min(256, w - x0), xl = x0 + nx - 1;
  const int p0 = min(max(lo[x0], 0), W);
  const int p1 = min(max(lo[xl] + cnt[xl], p0), min(W, p0 + cap));
  const int64_t total = (int64_t)gridDim.z * H * W * 3;
  const int64_t row = ((int64_t)b * H + y) * W * 3;
  const int64_t s0 = row + 3 * (int64_t)p0, s1 = row + 3 * (int64_t)p1, a0 = s0 & ~(int64_t)3;
  for (int64_t a = a0 + 4 * tid; a < s1; a += 1024) {
    uint32_t v = 0;
    if (a + 4 <= total) v = *(const uint32_t*)(src + a);
    else for (int k = 0; a + k < total; ++k) v |= (uint32_t)src[a + k] << (8 * k);
    stage[(a - a0) >> 2] = v;
  }
  __syncthreads();
  const bool act = tid < nx;
  uint32_t r[3] = {0u, 0u, 0u};
  if (act) {
    const int x = x0 + tid;
    const int l = min(max(lo[x], p0), p1), n = min(max(cnt[x], 0), min(kmax, p1 - l));
    const uint8_t* t = (const uint8_t*)stage + (s0 - a0) + 3 * (l - p0);
    int acc[3] = {1 << (IH_PREC - 1), 1 << (IH_PREC - 1), 1 << (IH_PREC - 1)};
    for (int j = 0; j < n; ++j) {
      const int c = coef[(int64_t)j * w + x];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += (int)t[3 * j + ch] * c;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) r[ch] = clip8(acc[ch]);
  }
  uint8_t* o = dst + (((int64_t)b * H + y) * w + x0) * 3;
  if ((w & 3) == 0) {   // chunk = a multiple of 12 bytes on a 4-byte boundary: regroup through LDS into dword stores
    __syncthreads();
    uint8_t* sb = (uint8_t*)stage;
    if (act) { sb[3 * tid] = (uint8_t)r[0]; sb[3 * tid + 1] = (uint8_t)r[1]; sb[3 * tid + 2] = (uint8_t)r[2]; }
    __syncthreads();
    if (4 * tid < 3 * nx) ((uint32_t*)o)[tid] = stage[tid];
  } else if (act) {
    o[3 * tid] = (uint8_t)r[0]; o[3 * tid + 1] = (uint8_t)r[1]; o[3 * tid + 2] = (uint8_t)r[2];
  }
}

// ---- vertical pass: [B][H][rowbytes] -> [B][h][rowbytes], rowbytes = 3 w: every byte of a row filters on its own -----------------------
__global__ __launch_bounds__(256) void pil_resize_v_kernel(const uint8_t* __restrict__ src, int H, int h, int rowbytes, const int* __restrict__ lo,
                                                           const int* __restrict__ cnt, const int* __restrict__ coef, int kmax,
                                                           uint8_t* __restrict__ dst) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
  if (i >= rowbytes) return;
  const int l = min(max(lo[y], 0), H), n = min(max(cnt[y], 0), min(kmax, H - l));   // wave-uniform
  const uint8_t* s = src + ((int64_t)b * H + l) * rowbytes + i;
  uint8_t* o = dst + ((int64_t)b * h + y) * rowbytes + i;
  int acc[4] = {1 << (IH_PREC - 1), 1 << (IH_PREC - 1), 1 << (IH_PREC - 1), 1 << (IH_PREC - 1)};
  if ((rowbytes & 3) == 0) {
    for (int j = 0; j < n; ++j) {
      const uint32_t v = *(const uint32_t*)(s + (int64_t)j * rowbytes);
      const int c = coef[(int64_t)j * h + y];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += (int)((v >> (8 * k)) & 255u) * c;
    }
    *(uint32_t*)o = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
  } else {
    const int nb = min(4, rowbytes - i);
    for (int j = 0; j < n; ++j) {
      const int c = coef[(int64_t)j * h + y];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nb) acc[k] += (int)s[(int64_t)j * rowbytes + k] * c;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nb) o[k] = (uint8_t)clip8(acc[k]);
  }
}

// ---- levels [B][h][w][3] -> zero-halo NHWC bf16 [(h + 2)][(w + 2)][cpad]: one lane per 8 channels (16 B) of one halo pixel ---------------
__global__ __launch_bounds__(256) void levels_to_halo_kernel(const uint8_t* __restrict__ lv, int h, int w, const uint16_t* __restrict__ lut,
                                                             bf16_t* __restrict__ out, int64_t s_out, int cpad) {
  const int g8 = cpad >> 3, b = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)(h + 2) * (w + 2) * g8) return;
  const int64_t pix = idx / g8;
  const int g = (int)(idx - pix * g8), yy = (int)(pix / (w + 2)), xx = (int)(pix - (int64_t)yy * (w + 2));
  u32x4 v = {0u, 0u, 0u, 0u};
  if (g == 0 && yy >= 1 && yy <= h && xx >= 1 && xx <= w) {
    const uint8_t* p = lv + (((int64_t)b * h + (yy - 1)) * w + (xx - 1)) * 3;
    v[0] = (uint32_t)lut[p[0]] | ((uint32_t)lut[p[1]] << 16);
    v[1] = (uint32_t)lut[p[2]];
  }
  *(u32x4*)(out + (int64_t)b * s_out + pix * cpad + g * 8) = v;
}

// the widest table an in -> out axis can have: Pillow's ksize = 2 * ceil(support) + 1
static int axis_ksize(int in, int out) {
  const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
  return 2 * (int)ceil(2.0 * fs) + 1;
}

}  // namespace rf

using namespace rf;

extern "C" int rf_image_levels(const void* img, int64_t s_img, int64_t s_row, int64_t s_pix, int64_t s_ch, int32_t B, int32_t H, int32_t W, void* levels,
                               void* stream) {
  RF_REQUIRE(img && levels, RF_ERR_NULL, "rf_image_levels: NULL tensor");
  RF_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= IH_MAX_SIDE && W <= IH_MAX_SIDE, RF_ERR_SHAPE, "rf_image_levels: B=%d H=%d W=%d (sides 1 .. %d)", B,
             H, W, IH_MAX_SIDE);
  RF_REQUIRE(s_row > 0 && s_pix > 0 && s_ch > 0 && (B == 1 || s_img > 0), RF_ERR_SHAPE, "rf_image_levels: strides must be positive");
  RF_REQUIRE((reinterpret_cast<uintptr_t>(levels) & 3u) == 0, RF_ERR_ALIGN, "rf_image_levels: levels must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(RF_KC_ROWOP, (double)B * H * W * 3 * 3, st);
  hipLaunchKernelGGL(image_levels_kernel, dim3(cdiv(cdiv(W, 4), 256), H, B), dim3(256), 0, st, (const bf16_t*)img, s_img, s_row, s_pix, s_ch, H, W,
                     (uint8_t*)levels);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

extern "C" int rf_pil_resize_to_vae_input(const void* levels, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w, const int32_t* x_lo,
                                          const int32_t* x_n, const int32_t* x_coef, int32_t kx, const int32_t* y_lo, const int32_t* y_n,
                                          const int32_t* y_coef, int32_t ky, const void* lut, void* scratch, void* out_levels, void* out_halo,
                                          int64_t s_halo, int32_t cin_pad, void* stream) {
  RF_REQUIRE(levels && lut && out_levels && out_halo, RF_ERR_NULL, "rf_pil_resize_to_vae_input: NULL tensor");
  RF_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && h > 0 && w > 0 && H <= IH_MAX_SIDE && W <= IH_MAX_SIDE && h <= IH_MAX_SIDE && w <= IH_MAX_SIDE,
             RF_ERR_SHAPE, "rf_pil_resize_to_vae_input: B=%d %dx%d -> %dx%d (sides 1 .. %d)", B, H, W, h, w, IH_MAX_SIDE);
  const bool do_x = W != w, do_y = H != h;
  RF_REQUIRE(!do_x || (x_lo && x_n && x_coef), RF_ERR_NULL, "rf_pil_resize_to_vae_input: the width changes (%d -> %d) and the x tables are NULL", W, w);
  RF_REQUIRE(!do_y || (y_lo && y_n && y_coef), RF_ERR_NULL, "rf_pil_resize_to_vae_input: the height changes (%d -> %d) and the y tables are NULL", H, h);
  RF_REQUIRE(!do_x || (kx >= 1 && kx <= axis_ksize(W, w)), RF_ERR_SHAPE, "rf_pil_resize_to_vae_input: kx=%d (1 .. %d for %d -> %d)", kx, axis_ksize(W, w), W, w);
  RF_REQUIRE(!do_y || (ky >= 1 && ky <= axis_ksize(H, h)), RF_ERR_SHAPE, "rf_pil_resize_to_vae_input: ky=%d (1 .. %d for %d -> %d)", ky, axis_ksize(H, h), H, h);
  RF_REQUIRE(!(do_x && do_y) || scratch, RF_ERR_NULL, "rf_pil_resize_to_vae_input: both axes change: scratch [B][H][w][3] is needed");
  RF_REQUIRE(cin_pad >= 8 && cin_pad % 8 == 0 && s_halo >= (int64_t)(h + 2) * (w + 2) * cin_pad && s_halo % 8 == 0, RF_ERR_SHAPE,
             "rf_pil_resize_to_vae_input: cin_pad=%d s_halo=%lld (cin_pad %% 8 == 0, s_halo %% 8 == 0, s_halo >= (h + 2)(w + 2) cin_pad)", cin_pad,
             (long long)s_halo);
  RF_REQUIRE(aligned16(out_halo) && (reinterpret_cast<uintptr_t>(levels) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_levels) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(scratch) & 3u) == 0, RF_ERR_ALIGN,
             "rf_pil_resize_to_vae_input: out_halo must be 16-byte, the level images 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(RF_KC_ROWOP, (double)B * ((double)H * W * 3 + (double)(h + 2) * (w + 2) * cin_pad * 2), st);
  const uint8_t* cur = (const uint8_t*)levels;
  if (do_x) {
    // a chunk of 256 output pixels spans at most 255 scale + 2 support + 1 source pixels
    const double scale = (double)W / w, fs = scale < 1.0 ? 1.0 : scale;
    const int cap = (int)(255.0 * scale + 4.0 * fs) + 2;
    const size_t lds = (size_t)3 * cap + 8 < 768 ? 768 : (size_t)3 * cap + 8;   // the staged window; reused for the chunk's 768 output bytes
    RF_REQUIRE(lds <= 65536, RF_ERR_SHAPE, "rf_pil_resize_to_vae_input: %d -> %d needs %zu bytes of LDS per chunk (max 65536)", W, w, lds);
    uint8_t* dst = (uint8_t*)(do_y ? scratch : out_levels);
    hipLaunchKernelGGL(pil_resize_h_kernel, dim3(cdiv(w, 256), H, B), dim3(256), lds, st, cur, H, W, w, x_lo, x_n, x_coef, kx, cap, dst);
    RF_LAUNCH_CHECK();
    cur = dst;
  }
  if (do_y) {
    hipLaunchKernelGGL(pil_resize_v_kernel, dim3(cdiv(cdiv(3 * w, 4), 256), h, B), dim3(256), 0, st, cur, H, h, 3 * w, y_lo, y_n, y_coef, ky,
                       (uint8_t*)out_levels);
    RF_LAUNCH_CHECK();
  } else if (!do_x) {
    RF_CHECK_HIP(hipMemcpyAsync(out_levels, levels, (size_t)B * h * w * 3, hipMemcpyDeviceToDevice, st));   // Pillow returns a copy
  }
  const int64_t lanes = (int64_t)(h + 2) * (w + 2) * (cin_pad / 8);
  hipLaunchKernelGGL(levels_to_halo_kernel, dim3((unsigned)cdiv64(lanes, 256), B), dim3(256), 0, st, (const uint8_t*)out_levels, h, w, (const uint16_t*)lut,
                     (bf16_t*)out_halo, s_halo, cin_pad);
  RF_LAUNCH_CHECK();
  return RF_OK;
}
