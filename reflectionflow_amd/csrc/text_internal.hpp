// Internal interface of text.hip shared with clip_vision.hip (not part of the C ABI): the encoder context over a caller-owned
// workspace, the projection GEMM, the head-dim-64 / -80 attention and the pre-LN CLIP layer loop.  The text towers keep their shape-based
// GEMM policy (TextCtx::sched = RF_SCHED_AUTO); the vision tower pins one schedule for every projection (clip_vision.hip).
#pragma once
#include "common.hpp"

#ifndef RF_TRY
#define RF_TRY(expr)              \
  do {                            \
    int _rc = (expr);             \
    if (_rc != RF_OK) return _rc; \
  } while (0)
#endif

namespace rf {

constexpr int TA_MAXS = 512;     // keys of attn64_kernel
constexpr int TA80_MAXS = 480;   // keys of attn80_kernel (text.hip: K + V^T of a head at head dim 80 within the 160 KiB LDS)
constexpr int TAS_MAXS = 2048;   // keys of attn64_stream_kernel (head dim 64 beyond TA_MAXS): 448 px / 14 needs 1056; a shared fp32 mask of 2048^2 is 16 MiB
constexpr int TAS80_MAXS = 2048;   // keys of attn80_stream_kernel (head dim 80 beyond TA80_MAXS, rf_text_attention80): as at head dim 64
constexpr rf_clip_tower_opts CLIP_L_OPTS = {64, RF_CLIP_ACT_QUICK_GELU};   // the towers of clip-vit-large-patch14: the entry points without opts

struct TextCtx {
  hipStream_t st;
  bf16_t *X, *Xn, *QK, *VT, *AO, *HID, *G, *ones;
  void* sk; int64_t sk_bytes;
  int S, S_pad, B;
  int sched;   // rf_gemm_schedule of every text_gemm launch: RF_SCHED_AUTO = the shape-based policy of text_gemm
};

struct TextSizes { int64_t x, qk, vt, ao, hid, g, total; };
constexpr int64_t TEXT_SK = 4096 + (64ll << 20);

inline TextSizes text_sizes(int rows, int D, int inner, int F, int hid_cols) {   // rows = B * S_pad
  TextSizes z;
  z.x = round_up((int64_t)rows * D * 2, 256);
  z.qk = round_up((int64_t)rows * 2 * inner * 2, 256);
  z.vt = round_up((int64_t)inner * rows * 2, 256);
  z.ao = round_up((int64_t)rows * inner * 2, 256);
  z.hid = round_up((int64_t)rows * hid_cols * 2, 256);
  z.g = round_up((int64_t)rows * F * 2, 256);
  z.total = 2 * z.x + z.qk + z.vt + z.ao + z.hid + z.g + round_up(16384 * 2, 256) + TEXT_SK;
  return z;
}

int text_ctx(TextCtx& c, const TextSizes& z, int B, int S, int S_pad, const rf_workspace* ws, hipStream_t st, const char* who);
int text_gemm(TextCtx& c, const bf16_t* x, int64_t ldx, const void* w, const void* b, int M, int N, int K, bf16_t* y, int64_t ldy, int epi,
              const bf16_t* residual);
int text_attn_max_keys(int head_dim);          // the resident kernels: TA_MAXS | TA80_MAXS; 0 for a head dim without a kernel
int text_attn_stream_max_keys(int head_dim);   // the streaming-keys kernel: TAS_MAXS at head dim 64, 0 elsewhere
int text_attention(TextCtx& c, int head_dim, int heads, int inner, int64_t ld_ao, const float* bias, int64_t bias_hs, float scale);
int clip_layers(TextCtx& c, const rf_clip_layer* layer, int layers, int heads, int D, int F, const float* mask, float eps, const char* who,
                const rf_clip_tower_opts& o, int inner = 0, bool route80 = false);   // inner / route80: the SigLIP towers (siglip.hip)
int clip_act_inplace(int act, bf16_t* x, int64_t n, hipStream_t st);   // rf_clip_act | RF_CLIP_ACT_GELU_TANH over x[0 .. n) in place, n % 8 == 0
int text_embed_rows(TextCtx& c, const void* table, const void* pos, const int32_t* ids, int D, int vocab);
int clip_opts_check(const rf_clip_tower_opts* o, int hidden, int heads, int S_pad, const char* who);

}  // namespace rf
