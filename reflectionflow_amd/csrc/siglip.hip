// SigLIP towers on the HIP path (transformers' SiglipVisionModel / SiglipTextModel; google/siglip-so400m-patch14-384 is hidden 1152 =
// 16 heads x 72 and 729 tokens, and is the vision tower inside NVILA / VILA): the score verifier that can give a LABEL, since the
// pairwise sigmoid is a calibrated probability (rf_siglip_score, clip_vision.hip).  The encoder layers are the CLIP towers'
// (text.hip clip_layers) with the attention width `inner` = 80 heads apart from the hidden width: the binding zero-pads every head
// of d <= 80 channels to 80, which is exact (include/rf_flux.h), and the attention goes through text_attention80_launch: attn80_kernel
// up to 480 keys, attn80_stream_kernel beyond.  New here: token assembly without a class token, the pooling head's probe attention,
// and the host sequences.  Batch invariance as in clip_vision.hip: every GEMM on RF_SCHED_TILE256, everything else one row / image /
// (image, head) per thread group with a fixed order.
#include "text_internal.hpp"

namespace rf {

constexpr rf_clip_tower_opts SIGLIP_OPTS = {80, RF_CLIP_ACT_GELU_TANH};   // never shown to clip_opts_check, which refuses the activation
constexpr int SG_MAXT = 2048;   // tokens of one image / prompt: attn80_stream_kernel's keys, and the probe kernel's score array in LDS

// ---- token assembly: X[b * S_pad + t] = patch row t + pos[t] (t < T) | 0; D % 8 == 0 ------------------------------------------------
__global__ __launch_bounds__(256) void siglip_tokens_kernel(const bf16_t* __restrict__ P, const bf16_t* __restrict__ pos, bf16_t* __restrict__ X, int T,
                                                            int S_pad, int n_rows, int D) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d8 = D >> 3;
  if (idx >= (int64_t)n_rows * d8) return;
  const int grow = (int)(idx / d8), c = (int)(idx % d8) * 8;
  const int b = grow / S_pad, t = grow - b * S_pad;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (t < T) {
    float x[8], p[8];
    unpack8(*(const u32x4*)(P + ((int64_t)b * T + t) * D + c), x);
    unpack8(*(const u32x4*)(pos + (int64_t)t * D + c), p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] += p[i];
    v = pack8(x);
  }
  *(u32x4*)(X + (int64_t)grow * D + c) = v;
}

// ---- probe attention of the pooling head ------------------------------------------------------------------------------------------------
// One workgroup per (head, image): ONE query (the probe's, fp32, 1/sqrt(d) folded in) over T keys at the true head dim d <= 80.
// out[b][h d + c] = sum_t softmax_t(q_h . k[b][t][h d ..]) v[b][t][h d + c].  k, v: bf16 rows of pitch ldk / ldv, image b's token t in
// row b * seq_rows + t, head h in columns h d ...  No MFMA: 2 T d multiply-adds per workgroup.  fp32 throughout, P is not rounded;
// fixed order: thread tid owns keys tid, tid + 256, ...; maxima and sums reduce by xor-shuffles then over the four waves in order;
// in the PV sum wave w owns keys t = w mod 4 and lane c channels c and c + 64, the four partials add as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void siglip_probe_attn_kernel(const float* __restrict__ q, const bf16_t* __restrict__ k, int64_t ldk,
                                                                const bf16_t* __restrict__ v, int64_t ldv, bf16_t* __restrict__ out, int64_t ldo, int d,
                                                                int T, int seq_rows) {
  __shared__ float sc[SG_MAXT];
  __shared__ float qs[80];
  __shared__ float red[4];
  __shared__ float part[4][80];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* kb = k + (int64_t)b * seq_rows * ldk + h * d;
  const bf16_t* vb = v + (int64_t)b * seq_rows * ldv + h * d;
  if (tid < d) qs[tid] = q[h * d + tid];
  __syncthreads();
  float mx = -__builtin_huge_valf();
  for (int t = tid; t < T; t += 256) {
    const bf16_t* kr = kb + (int64_t)t * ldk;
    float s = 0.0f;
    for (int c = 0; c < d; c += 8) {   // d % 8 == 0, rows 16-byte aligned
      float x[8];
      unpack8(*(const u32x4*)(kr + c), x);
#pragma unroll
      for (int i = 0; i < 8; ++i) s = __builtin_fmaf(qs[c + i], x[i], s);
    }
    sc[t] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float l = 0.0f;
  for (int t = tid; t < T; t += 256) {
    const float p = __expf(sc[t] - mx);
    sc[t] = p;
    l += p;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) l += __shfl_xor(l, o);
  if (lane == 0) red[w] = l;
  __syncthreads();
  l = (red[0] + red[1]) + (red[2] + red[3]);
  float a0 = 0.0f, a1 = 0.0f;
  const bool two = lane + 64 < d;
  for (int t = w; t < T; t += 4) {
    const float p = sc[t];
    const bf16_t* vr = vb + (int64_t)t * ldv;
    if (lane < d) a0 = __builtin_fmaf(p, bf2f(vr[lane]), a0);
    if (two) a1 = __builtin_fmaf(p, bf2f(vr[lane + 64]), a1);
  }
  if (lane < d) part[w][lane] = a0;
  if (two) part[w][lane + 64] = a1;
  __syncthreads();
  if (tid < d) out[(int64_t)b * ldo + h * d + tid] = f2bf(((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) / l);
}

static int probe_attention(const float* q, const bf16_t* k, int64_t ldk, const bf16_t* v, int64_t ldv, bf16_t* out, int64_t ldo, int heads, int d, int B,
                           int T, int seq_rows, hipStream_t st) {
  ProfScope prof(RF_KC_ATTN, 4.0 * (double)T * d * heads * B, st);
  hipLaunchKernelGGL(siglip_probe_attn_kernel, dim3(heads, B), dim3(256), 0, st, q, k, ldk, v, ldv, out, ldo, d, T, seq_rows);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

static int siglip_geometry_check(const char* who, int layers, int hidden, int heads, int head_dim, int inter) {
  RF_REQUIRE(layers > 0 && heads > 0 && hidden > 0 && hidden % 8 == 0 && inter > 0 && inter % 64 == 0, RF_ERR_SHAPE,
             "%s: layers=%d heads=%d hidden=%d inter=%d (need hidden %% 8 == 0, inter %% 64 == 0)", who, layers, heads, hidden, inter);
  RF_REQUIRE(head_dim > 0 && head_dim <= 80 && head_dim % 8 == 0 && hidden == heads * head_dim, RF_ERR_SHAPE,
             "%s: hidden=%d heads=%d head_dim=%d (need hidden = heads * head_dim, head_dim %% 8 == 0, <= 80)", who, hidden, heads, head_dim);
  RF_REQUIRE(heads * 80 <= 4096, RF_ERR_SHAPE, "%s: heads=%d: heads * 80 = %d > 4096", who, heads, heads * 80);
  return RF_OK;
}

static int siglip_vision_check(const rf_siglip_vision_weights* w, const char* who) {
  RF_REQUIRE(w && w->layer && w->patch_w && w->patch_b && w->pos_embed && w->post_ln_scale && w->post_ln_shift && w->w_kv && w->b_kv && w->probe_q &&
                 w->w_po && w->b_po && w->hln_scale && w->hln_shift && w->w_hfc1 && w->b_hfc1 && w->w_hfc2 && w->b_hfc2, RF_ERR_NULL, "%s: weights NULL", who);
  RF_TRY(siglip_geometry_check(who, w->layers, w->hidden, w->heads, w->head_dim, w->inter));
  RF_REQUIRE(w->patch > 0 && w->image_size >= w->patch, RF_ERR_SHAPE, "%s: image_size=%d patch=%d", who, w->image_size, w->patch);
  const int g = w->image_size / w->patch;
  const int64_t T = (int64_t)g * g;
  RF_REQUIRE(T <= SG_MAXT, RF_ERR_SHAPE, "%s: %lld tokens > %d", who, (long long)T, SG_MAXT);
  RF_REQUIRE(w->mask_S == (int)round_up(T, 32), RF_ERR_SHAPE, "%s: mask_S=%d, %lld tokens need %d", who, w->mask_S, (long long)T, (int)round_up(T, 32));
  RF_REQUIRE(w->mask || T == w->mask_S, RF_ERR_NULL, "%s: mask NULL with %lld tokens in S_pad = %d rows", who, (long long)T, w->mask_S);
  return RF_OK;
}

static TextSizes siglip_sizes(int R, int hidden, int heads, int inter) {
  const int Dp = (int)round_up(hidden, 64), Ip = (int)round_up(heads * 80, 64);
  return text_sizes(R, Dp, Ip, inter, inter);
}

static int siglip_text_check(const rf_siglip_text_weights* w, int32_t S, const char* who) {
  RF_REQUIRE(w && w->layer && w->tok_embed && w->pos_embed && w->final_ln_scale && w->final_ln_shift && w->head_w && w->head_b, RF_ERR_NULL, "%s: weights NULL",
             who);
  RF_TRY(siglip_geometry_check(who, w->layers, w->hidden, w->heads, w->head_dim, w->inter));
  RF_REQUIRE(w->vocab > 0 && w->proj_dim > 0 && w->proj_dim % 8 == 0, RF_ERR_SHAPE, "%s: vocab=%d proj_dim=%d (proj_dim %% 8 == 0)", who, w->vocab, w->proj_dim);
  RF_REQUIRE(S > 0 && S <= w->max_pos && S <= SG_MAXT, RF_ERR_SHAPE, "%s: S=%d (1 .. min(max_pos = %d, %d))", who, S, w->max_pos, SG_MAXT);
  return RF_OK;
}

}  // namespace rf

using namespace rf;

extern "C" int64_t rf_siglip_vision_workspace_bytes(const rf_siglip_vision_weights* w, int32_t B) {
  const int rc = siglip_vision_check(w, "rf_siglip_vision_workspace_bytes");
  if (rc != RF_OK) return rc;
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_siglip_vision_workspace_bytes: B=%d (1 .. 64)", B);
  return siglip_sizes(B * w->mask_S, w->hidden, w->heads, w->inter).total;
}

// Workspace use beyond clip_layers': the patch GEMM's output [B * T][D] lives in QK ([R][2 inner], inner >= D); after the layers the
// post-layernormed tokens are in Xn [R][Dp], their K | V projections for the pooling head in QK as [R][2 D], the pooled attention
// rows [B][Dp] in AO (zeroed first: its pad columns are a GEMM's K tail), the head's residual [B][D] in X, its LayerNorm in Xn's first
// B rows (same pitch Dp, pad columns still zero), the MLP's hidden rows [B][F] in HID.
extern "C" int rf_siglip_vision_encode(const rf_siglip_vision_weights* w, const void* patches, int32_t B, void* pooled, const rf_workspace* ws, void* stream) {
  const char* who = "rf_siglip_vision_encode";
  RF_TRY(siglip_vision_check(w, who));
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "%s: B=%d (1 .. 64)", who, B);
  RF_REQUIRE(patches && pooled && aligned16(patches) && aligned16(pooled), RF_ERR_NULL, "%s: NULL / unaligned tensor", who);
  const int g = w->image_size / w->patch, T = g * g, S_pad = w->mask_S, D = w->hidden, F = w->inter, R = B * S_pad, I = w->heads * 80;
  const int K_pad = (int)round_up(3 * w->patch * w->patch, 64), Dp = (int)round_up(D, 64);
  hipStream_t st = (hipStream_t)stream;
  TextCtx c;
  RF_TRY(text_ctx(c, siglip_sizes(R, D, w->heads, F), B, T, S_pad, ws, st, who));
  c.sched = RF_SCHED_TILE256;   // batch invariance: see clip_vision.hip's header
  RF_TRY(text_gemm(c, (const bf16_t*)patches, K_pad, w->patch_w, w->patch_b, B * T, D, K_pad, c.QK, D, RF_EPI_STORE, nullptr));
  {
    ProfScope prof(RF_KC_ROWOP, (double)R * D * 6, st);
    hipLaunchKernelGGL(siglip_tokens_kernel, dim3((unsigned)cdiv64((int64_t)R * D / 8, 256)), dim3(256), 0, st, c.QK, (const bf16_t*)w->pos_embed, c.X, T,
                       S_pad, R, D);
    RF_LAUNCH_CHECK();
  }
  RF_TRY(clip_layers(c, w->layer, w->layers, w->heads, D, F, w->mask, w->eps, who, SIGLIP_OPTS, I, true));
  RF_TRY(rf_layernorm_modulate(c.X, D, c.Xn, Dp, R, D, w->post_ln_scale, w->post_ln_shift, w->eps, st));
  // the pooling head
  RF_TRY(text_gemm(c, c.Xn, Dp, w->w_kv, w->b_kv, R, 2 * D, Dp, c.QK, 2 * D, RF_EPI_STORE, nullptr));
  RF_CHECK_HIP(hipMemsetAsync(c.AO, 0, (size_t)B * Dp * 2, st));
  RF_TRY(probe_attention(w->probe_q, c.QK, 2 * D, c.QK + D, 2 * D, c.AO, Dp, w->heads, w->head_dim, B, T, S_pad, st));
  RF_TRY(text_gemm(c, c.AO, Dp, w->w_po, w->b_po, B, D, Dp, c.X, D, RF_EPI_STORE, nullptr));
  RF_TRY(rf_layernorm_modulate(c.X, D, c.Xn, Dp, B, D, w->hln_scale, w->hln_shift, w->eps, st));
  RF_TRY(text_gemm(c, c.Xn, Dp, w->w_hfc1, w->b_hfc1, B, F, Dp, c.HID, F, RF_EPI_STORE, nullptr));
  RF_TRY(clip_act_inplace(RF_CLIP_ACT_GELU_TANH, c.HID, (int64_t)B * F, st));
  RF_TRY(text_gemm(c, c.HID, F, w->w_hfc2, w->b_hfc2, B, D, F, (bf16_t*)pooled, D, RF_EPI_STORE, c.X));
  return RF_OK;
}

extern "C" int64_t rf_siglip_text_workspace_bytes(const rf_siglip_text_weights* w, int32_t B, int32_t S) {
  const int rc = siglip_text_check(w, S, "rf_siglip_text_workspace_bytes");
  if (rc != RF_OK) return rc;
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_siglip_text_workspace_bytes: B=%d (1 .. 64)", B);
  return siglip_sizes(B * (int)round_up(S, 32), w->hidden, w->heads, w->inter).total;
}

extern "C" int rf_siglip_text_encode(const rf_siglip_text_weights* w, const int32_t* ids, int32_t B, int32_t S, void* pooled, const rf_workspace* ws,
                                     void* stream) {
  const char* who = "rf_siglip_text_encode";
  RF_TRY(siglip_text_check(w, S, who));
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "%s: B=%d (1 .. 64)", who, B);
  RF_REQUIRE(ids && pooled && aligned16(pooled), RF_ERR_NULL, "%s: NULL / unaligned tensor", who);
  const int S_pad = (int)round_up(S, 32), D = w->hidden, Dp = (int)round_up(D, 64), F = w->inter, R = B * S_pad, I = w->heads * 80;
  RF_REQUIRE(S == S_pad ? true : (w->mask && w->mask_S == S_pad), RF_ERR_SHAPE, "%s: S=%d needs a padded-keys mask built for S_pad = %d (have %d)", who, S, S_pad,
             w->mask ? w->mask_S : 0);
  hipStream_t st = (hipStream_t)stream;
  TextCtx c;
  RF_TRY(text_ctx(c, siglip_sizes(R, D, w->heads, F), B, S, S_pad, ws, st, who));
  c.sched = RF_SCHED_TILE256;
  RF_TRY(text_embed_rows(c, w->tok_embed, w->pos_embed, ids, D, w->vocab));
  RF_TRY(clip_layers(c, w->layer, w->layers, w->heads, D, F, S == S_pad ? nullptr : w->mask, w->eps, who, SIGLIP_OPTS, I, true));
  RF_TRY(rf_layernorm_modulate(c.X, D, c.Xn, Dp, R, D, w->final_ln_scale, w->final_ln_shift, w->eps, st));
  // head over the LAST token's row of every sequence ("which may be padding": max_length padding is the model's training recipe)
  RF_TRY(text_gemm(c, c.Xn + (int64_t)(S - 1) * Dp, (int64_t)S_pad * Dp, w->head_w, w->head_b, B, w->proj_dim, Dp, (bf16_t*)pooled, w->proj_dim, RF_EPI_STORE,
                   nullptr));
  return RF_OK;
}

// The pooling head's probe attention on caller buffers (a binding's own pooling head; the kernel-level tests): q fp32 [heads * head_dim]; k, v bf16, image b's token t in row
// b * seq_rows + t of pitch ldk / ldv, head h in columns h * head_dim ..; out [B][ldo] bf16.
extern "C" int rf_siglip_probe_attention(const float* q, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo, int32_t heads,
                                               int32_t head_dim, int32_t B, int32_t T, int32_t seq_rows, void* stream) {
  const char* who = "rf_siglip_probe_attention";
  RF_REQUIRE(q && k && v && out, RF_ERR_NULL, "%s: NULL tensor", who);
  RF_REQUIRE(head_dim > 0 && head_dim <= 80 && head_dim % 8 == 0, RF_ERR_SHAPE, "%s: head_dim=%d (a multiple of 8, <= 80)", who, head_dim);
  RF_REQUIRE(heads >= 1 && heads * 80 <= 4096 && B >= 1 && B <= 64, RF_ERR_SHAPE, "%s: heads=%d B=%d (heads * 80 <= 4096, B 1 .. 64)", who, heads, B);
  RF_REQUIRE(T >= 1 && T <= SG_MAXT && seq_rows >= T, RF_ERR_SHAPE, "%s: T=%d seq_rows=%d (1 <= T <= %d, seq_rows >= T)", who, T, seq_rows, SG_MAXT);
  const int64_t D = (int64_t)heads * head_dim;
  RF_REQUIRE(ldk >= D && ldv >= D && ldo >= D && ldk % 8 == 0 && ldv % 8 == 0, RF_ERR_SHAPE, "%s: ldk=%lld ldv=%lld ldo=%lld (>= heads * head_dim = %lld, ldk / ldv %% 8 == 0)",
             who, (long long)ldk, (long long)ldv, (long long)ldo, (long long)D);
  RF_REQUIRE(aligned16(k) && aligned16(v), RF_ERR_ALIGN, "%s: k / v not 16-byte aligned", who);
  return probe_attention(q, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv, (bf16_t*)out, ldo, heads, head_dim, B, T, seq_rows, (hipStream_t)stream);
}
