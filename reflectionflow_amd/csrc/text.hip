// Text encoders of the FLUX pipeline on the HIP path: T5-v1.1 encoder (prompt_embeds) and CLIP text tower
// (pooled_prompt_embeds), reference call site train_flux/flux/generate.py:148-161 -> FluxPipeline.encode_prompt, run per candidate
// and round by tts/tts_reflectionflow.py:286-294.  B sequences of S tokens per call (a rank's candidates of a round: the projections
// then run as ONE GEMM over B * S rows instead of B skinny ones); token ids in, hidden states out; tokenisation is the caller's
// (vocabulary files are host-side data).
//
// Every matrix product is a launch of the bf16 MFMA GEMM that already exists (rf_gemm_bf16): q|k projection, V^T = W_v x^T with the
// operands swapped (the attention kernel wants V transposed), out projection and FFN down-projection with the residual add in the
// epilogue (RF_EPI_GATE_RES, gate of ones), fused wi_0|wi_1 / fc1.  New here:
//   * attn64_kernel: one (head, 64-query block) per workgroup, head dim 64, keys <= 512: the head's K and V^T live in LDS whole
//     (XOR-swizzled K rows, padded + key-permuted V^T rows), S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16 with P kept
//     in registers, full-row softmax in fp32 (no running maximum: the whole row of scores is in registers), additive fp32 bias
//     [heads or 1][S_pad][S_pad] (T5: bucketed relative positions; CLIP: the causal mask; both: -inf on padded keys);
//   * attn80_kernel: the same attention at head dim 80 (the ViT-H/14 towers of PickScore / HPSv2 / LAION CLIP-H), keys <= 480;
//   * attn64_stream_kernel: head dim 64 with 513 .. 2048 keys (ViT-L/14 at 336 px: 577 tokens): K / V^T chunks of 128 keys double-buffered
//     through the LDS, online softmax;
//   * attn80_stream_kernel: the same at head dim 80 with 96-key chunks, up to 2048 keys (SigLIP so400m/14 at 384 px: 729 tokens of
//     head dim 72 zero-padded to 80), reached through rf_text_attention80 and the SigLIP towers (siglip.hip) only;
//   * row kernels (HBM-bound, 16-byte accesses): embedding gather (+ position rows), T5 RMS norm, gelu_new(a) * b, quick_gelu, gelu (erf).
#include "common.hpp"
#include "text_internal.hpp"

namespace rf {

static inline int grid_for(int64_t n, int per_block = 256) { return (int)((n + per_block - 1) / per_block); }

// ---- row kernels -------------------------------------------------------------------------------------------------------------
// out[b * S_pad + i][:] = table[ids[b * S + i]][:] (+ pos[i][:]); rows i >= S of a sequence are zero-filled; D % 8 == 0
__global__ __launch_bounds__(256) void embed_rows_kernel(const bf16_t* __restrict__ table, const bf16_t* __restrict__ pos, const int32_t* __restrict__ ids,
                                                         bf16_t* __restrict__ out, int S, int S_pad, int n_rows, int D, int vocab) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d8 = D >> 3;
  if (idx >= (int64_t)n_rows * d8) return;
  const int grow = (int)(idx / d8), c = (int)(idx % d8) * 8;
  const int b = grow / S_pad, row = grow - b * S_pad;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < S) {
    int id = ids[b * S + row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    v = *(const u32x4*)(table + (int64_t)id * D + c);
    if (pos != nullptr) {
      float a[8], b[8];
      unpack8(v, a);
      unpack8(*(const u32x4*)(pos + (int64_t)row * D + c), b);
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] += b[i];
      v = pack8(a);
    }
  }
  *(u32x4*)(out + (int64_t)grow * D + c) = v;
}

// T5LayerNorm: y = w * x * rsqrt(mean(x^2) + eps), statistics in fp32; one wave per row, D % 8 == 0, D <= 8 * 64 * 8 = 4096
__global__ __launch_bounds__(256) void rms_norm_rows_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w, bf16_t* __restrict__ y, int rows,
                                                            int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bf16_t* xr = x + (int64_t)row * D;
  float v[8][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = (i * 64 + lane) * 8;
    if (c < D) {
      unpack8(*(const u32x4*)(xr + c), v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
  const float r = rsqrtf(ss / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = (i * 64 + lane) * 8;
    if (c < D) {
      float g[8];
      unpack8(*(const u32x4*)(w + c), g);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = g[j] * (v[i][j] * r);
      *(u32x4*)(y + (int64_t)row * D + c) = pack8(v[i]);
    }
  }
}

// T5DenseGatedActDense: out[r][c] = gelu_new(h[r][c]) * h[r][F + c]   (h = [rows][2F] from the fused wi_0 | wi_1 GEMM)
__global__ __launch_bounds__(256) void geglu_rows_kernel(const bf16_t* __restrict__ h, bf16_t* __restrict__ out, int rows, int F) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int f8 = F >> 3;
  if (idx >= (int64_t)rows * f8) return;
  const int row = (int)(idx / f8), c = (int)(idx % f8) * 8;
  float a[8], b[8];
  unpack8(*(const u32x4*)(h + (int64_t)row * 2 * F + c), a);
  unpack8(*(const u32x4*)(h + (int64_t)row * 2 * F + F + c), b);
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = gelu_tanh(a[i]) * b[i];
  *(u32x4*)(out + (int64_t)row * F + c) = pack8(a);
}

// A CLIP tower's MLP activation, in place.  quick_gelu: x * sigmoid(1.702 x).  gelu (transformers' "gelu", the ViT-H towers):
// x * 0.5 * (1 + erf(x / sqrt(2))) in fp32, one rounding to bf16 -- the operation order of torch.nn.functional.gelu on a bf16 tensor.
// gelu_pytorch_tanh (RF_CLIP_ACT_GELU_TANH, the SigLIP towers; the CLIP entry points refuse it): the fc1 GEMM stores acc + bias
// rounded to bf16, this kernel forms gelu_tanh of that in fp32 and rounds to bf16 once -- nn.Linear then F.gelu(approximate="tanh")
// on a bf16 tensor -- rather than the GEMM's RF_EPI_GELU, which would skip the first rounding.
// A row kernel of its own, not a GEMM epilogue: the tower runs once per round, not per step.
template <int ACT>   // rf_clip_act
__global__ __launch_bounds__(256) void clip_act_kernel(bf16_t* __restrict__ x, int64_t n8) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n8) return;
  float a[8];
  unpack8(*(const u32x4*)(x + idx * 8), a);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if constexpr (ACT == RF_CLIP_ACT_GELU) a[i] = a[i] * 0.5f * (1.0f + erff(a[i] * 0.70710678118654752440f));
    else if constexpr (ACT == RF_CLIP_ACT_GELU_TANH) a[i] = gelu_tanh(a[i]);
    else a[i] = a[i] * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * a[i]));
  }
  *(u32x4*)(x + idx * 8) = pack8(a);
}

__global__ __launch_bounds__(256) void fill_bf16_rows_kernel(bf16_t* __restrict__ p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = f2bf(v);
}

// ---- attention, head dim 64, <= 512 keys ----------------------------------------------------------------------------------------
constexpr int TA_NT = TA_MAXS / 16;   // score tiles of 16 keys
static inline int ta_lds_bytes(int S_pad) { return S_pad * 128 + 64 * (S_pad * 2 + 16); }

// q [S_pad][ldq], k [S_pad][ldk] (this head's 64 columns start at head * 64), vt [heads * 64][ldvt] (V transposed: row = channel,
// column = key), bias [.][S_pad][S_pad] fp32 with head stride bias_hs (0: shared by the heads) or NULL, out [S][ldo].
// scores = scale * q.k + bias; S_pad % 32 == 0; rows / keys >= S must be masked by the bias (-inf) and are not written.
// blockIdx.z = sequence: its rows of q / k / out start at z * S_pad, its columns of vt at z * S_pad (out: z * S_pad as well).
template <int QI>   // query tiles per wave: a workgroup stages K / V^T once for 64 * QI queries
__global__ __launch_bounds__(256) void attn64_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                     const bf16_t* __restrict__ vt, int64_t ldvt, const float* __restrict__ bias, int64_t bias_hs,
                                                     bf16_t* __restrict__ out, int64_t ldo, int S, int S_pad, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const kl = smem;                       // K rows: 128 B each, 16-byte chunk c of row r at chunk c ^ (r & 7)
  char* const vl = smem + S_pad * 128;         // V^T rows: pitch S_pad * 2 + 16 B (bank shift of 4 words per row), key slots permuted
  const int vpitch = S_pad * 2 + 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int head = blockIdx.y, qb = blockIdx.x;
  {
    const int64_t r0 = (int64_t)blockIdx.z * S_pad;
    q += r0 * ldq; k += r0 * ldk; vt += r0; out += r0 * ldo;
  }
  // ---- stage the head's K and V^T --------------------------------------------------------------------------------------------
  for (int idx = tid; idx < S_pad * 8; idx += 256) {
    const int r = idx >> 3, c = idx & 7;
    *(u32x4*)(kl + r * 128 + ((c ^ (r & 7)) << 4)) = *(const u32x4*)(k + (int64_t)r * ldk + head * 64 + c * 8);
  }
  // The PV product sums over the 32 keys of a block in ANY order as long as P^T and V^T agree.  A 16x16 score tile leaves keys
  // 4g .. 4g+3 of the tile in lane group g, so the B operand of a 32-key block holds, in its 8 slots of lane group g, keys
  // {4g..4g+3} of the block's first tile and {16+4g .. 16+4g+3} of its second: slot(key) = 8 (key%16 / 4) + 4 (key / 16) + key % 4.
  const int kc = S_pad >> 3;
  for (int idx = tid; idx < 64 * kc; idx += 256) {
    const int d = idx / kc, m = idx - d * kc;
    const u32x4 v = *(const u32x4*)(vt + (int64_t)(head * 64 + d) * ldvt + m * 8);
    const int blk = (m * 8) >> 5, kap = (m * 8) & 31;
    const int tile = kap >> 4, g0 = (kap & 15) >> 2;
    char* dst = vl + d * vpitch + blk * 64;
    u32x2 lo, hi;
    lo[0] = v[0]; lo[1] = v[1]; hi[0] = v[2]; hi[1] = v[3];
    *(u32x2*)(dst + (8 * g0 + 4 * tile) * 2) = lo;
    *(u32x2*)(dst + (8 * (g0 + 1) + 4 * tile) * 2) = hi;
  }
  __syncthreads();
  const int nt = S_pad >> 4;
  const float LOG2E = 1.4426950408889634f;
  const float sl2 = scale * LOG2E;
#pragma unroll 1
  for (int it = 0; it < QI; ++it) {
  // ---- scores: S^T tile t = K[16t .. 16t+15] Q^T: this lane holds keys 16t + 4g + r of query l15 ---------------------------------
  const int q_row = (qb * QI + it) * 64 + w * 16 + l15;
  if ((qb * QI + it) * 64 >= S_pad) break;
  const int q_ld = q_row < S_pad ? q_row : S_pad - 1;
  bf16x8 qf[2];
#pragma unroll
  for (int ds = 0; ds < 2; ++ds) qf[ds] = *(const bf16x8*)(q + (int64_t)q_ld * ldq + head * 64 + ds * 32 + g * 8);
  const float* brow = bias ? bias + head * bias_hs + (int64_t)q_ld * S_pad + 4 * g : nullptr;
  f32x4 s[TA_NT];
  float mx = -__builtin_huge_valf();
#pragma unroll
  for (int t = 0; t < TA_NT; ++t) {
    if (t < nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int r = t * 16 + l15;
#pragma unroll
      for (int ds = 0; ds < 2; ++ds) {
        const bf16x8 kf = *(const bf16x8*)(kl + r * 128 + (((ds * 4 + g) ^ (r & 7)) << 4));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ds], acc, 0, 0, 0);
      }
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (brow) b = *(const f32x4*)(brow + t * 16);
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        acc[r2] = acc[r2] * sl2 + b[r2] * LOG2E;
        mx = fmaxf(mx, acc[r2]);
      }
      s[t] = acc;
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if (!(mx > -__builtin_huge_valf())) mx = 0.f;   // a fully masked (padded) query row: keep the arithmetic finite
  // ---- P = exp2(s - max), row sums, O^T += V^T P^T per 32-key block ------------------------------------------------------------------
  f32x4 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
#pragma unroll
  for (int b = 0; b < TA_NT / 2; ++b) {
    if (2 * b < nt) {
      float p[8];
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        p[r2] = __builtin_amdgcn_exp2f(s[2 * b][r2] - mx);
        p[4 + r2] = __builtin_amdgcn_exp2f(s[2 * b + 1][r2] - mx);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) l += p[i];
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pack8(p));
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 vf = *(const bf16x8*)(vl + (dt * 16 + l15) * vpitch + b * 64 + g * 16);
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[dt], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q_row < S) {
    const float inv = 1.0f / l;
    bf16_t* orow = out + (int64_t)q_row * ldo + head * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      u32x2 v;
      v[0] = pack2(oacc[dt][0] * inv, oacc[dt][1] * inv);
      v[1] = pack2(oacc[dt][2] * inv, oacc[dt][3] * inv);
      *(u32x2*)(orow + dt * 16) = v;
    }
  }
  }   // it
}

// ---- attention, head dim 80 (ViT-H/14 vision tower), keys resident in LDS ------------------------------------------------------------
// Same contract as attn64_kernel (operands, bias, masking, fp32 softmax, fixed reduction order, QI); head dim 80 instead of 64.  It is
// a kernel of its own and not a template over the head dim: attn64_kernel's results are pinned bit for bit (T5, CLIP-L text, ViT-L
// vision), so its source stays untouched.  Decisions (MI355X LDS: 64 banks x 4 B, a ds_read_b128 is served in four 16-lane groups,
// conflict-free when a group's addresses fall on 16 different 16-byte slots of the 256-byte bank row):
//   * QK^T over 80 = 32 + 32 + 16 channels: three v_mfma_f32_16x16x32_bf16.  The third one's operands hold channels 64 .. 79 in
//     lane groups g = 0, 1 and ZEROS in g = 2, 3 (those lanes issue no load at all: nothing is read past the head's 80 columns of q
//     or k).  One instruction shape for the whole kernel and b128 fragment reads only; the half-empty MFMA costs 8 passes per 16
//     keys in a kernel that is bound by staging K / V^T, not by the matrix pipe.
//   * K in LDS: a row is 160 B = 10 chunks of 16 B, so (c ^ (r & 7)) over 8 chunks does not carry over -- and nothing is needed in
//     its place: at the natural pitch of 10 chunks, row r starts at slot 10 r mod 16, which is even and takes 8 values, rows r and
//     r + 8 sharing one.  A lane group reads its 16 rows with g on rows {0-3, 12-15} and g + 1 on rows {4-11} (or the reverse): of
//     two rows 8 apart exactly one carries the + 1, so the 16 addresses fall on 16 different slots, for the two whole k-steps and
//     for the tail alike.  No swizzle, no padding bytes, and the staging copy is linear.  (An odd pitch of 11 chunks is 2-way.)
//   * V^T in LDS: 80 channel rows, key slots permuted as in attn64_kernel; pitch 64 * m bytes with m = S_pad / 32 made ODD (one
//     64-byte block of padding when it is even) and the 16-byte chunk g of a 64-byte key block stored at g ^ swz((d & 15) >> 2),
//     swz = {0, 2, 3, 1}.  Rows d, d + 4, d + 8, d + 12 of a 16-row fragment share a 64-byte quarter of the bank row (m odd: 4 m d mod
//     16 walks the four quarters with d mod 4) and carry g, g ^ 1, g ^ 1, g within a lane group; the swizzle sends them to four
//     different chunks.  (attn64_kernel's pitch S_pad * 2 + 16 is 2-way under the same model.)
//   * PV: 5 output tiles of 16 channels, P in registers.
//   * LDS budget: S_pad * 160 + 80 * 64 * (m | 1) bytes: 92,160 B at S_pad = 288 (257 tokens of ViT-H/14 at 224 px), 153,600 B at
//     S_pad = 480 = TA80_MAXS, the largest multiple of 32 that fits a CU's 160 KiB (512 keys would need 168,960 B).  The CLIP entry
//     points refuse larger towers; attn80_stream_kernel below streams the keys for rf_text_attention80 and the SigLIP towers.
//   * q scale: the binding folds 1/sqrt(80) into the q weights and bias, `scale` is 1.
// tests/test_clip_h_cpu.py restates the three fragment-read address formulas against the bank model.
constexpr int TA80_NT = TA80_MAXS / 16;
static inline int ta80_vpitch(int S_pad) { return 64 * ((S_pad >> 5) | 1); }
static inline int ta80_lds_bytes(int S_pad) { return S_pad * 160 + 80 * ta80_vpitch(S_pad); }
static_assert(TA80_MAXS % 32 == 0 && TA80_MAXS * 160 + 80 * 64 * ((TA80_MAXS / 32) | 1) <= 160 * 1024, "head-dim-80 K + V^T must fit the LDS");

template <int QI>
__global__ __launch_bounds__(256) void attn80_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                     const bf16_t* __restrict__ vt, int64_t ldvt, const float* __restrict__ bias, int64_t bias_hs,
                                                     bf16_t* __restrict__ out, int64_t ldo, int S, int S_pad, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const kl = smem;                       // K rows: 160 B each, as they lie in memory
  char* const vl = smem + S_pad * 160;         // V^T rows: pitch 64 * odd, chunk g of a key block at g ^ swz, key slots permuted
  const int vpitch = 64 * ((S_pad >> 5) | 1);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int head = blockIdx.y, qb = blockIdx.x;
  {
    const int64_t r0 = (int64_t)blockIdx.z * S_pad;
    q += r0 * ldq; k += r0 * ldk; vt += r0; out += r0 * ldo;
  }
  // ---- stage the head's K and V^T --------------------------------------------------------------------------------------------
  for (int idx = tid; idx < S_pad * 10; idx += 256) {
    const int r = idx / 10, c = idx - r * 10;
    *(u32x4*)(kl + idx * 16) = *(const u32x4*)(k + (int64_t)r * ldk + head * 80 + c * 8);
  }
  // key slots of a 32-key block as in attn64_kernel: slot(key) = 8 (key%16 / 4) + 4 (key / 16) + key % 4
  const int kc = S_pad >> 3;
  for (int idx = tid; idx < 80 * kc; idx += 256) {
    const int d = idx / kc, m = idx - d * kc;
    const u32x4 v = *(const u32x4*)(vt + (int64_t)(head * 80 + d) * ldvt + m * 8);
    const int blk = (m * 8) >> 5, kap = (m * 8) & 31;
    const int tile = kap >> 4, g0 = (kap & 15) >> 2;
    const int sw = (0x78 >> (2 * ((d & 15) >> 2))) & 3;
    char* dst = vl + d * vpitch + blk * 64 + 8 * tile;
    u32x2 lo, hi;
    lo[0] = v[0]; lo[1] = v[1]; hi[0] = v[2]; hi[1] = v[3];
    *(u32x2*)(dst + ((g0 ^ sw) << 4)) = lo;
    *(u32x2*)(dst + (((g0 + 1) ^ sw) << 4)) = hi;
  }
  __syncthreads();
  const int nt = S_pad >> 4;
  const float LOG2E = 1.4426950408889634f;
  const float sl2 = scale * LOG2E;
  const int vsw = (0x78 >> (2 * (l15 >> 2))) & 3;   // every V^T fragment row is 16 dt + l15
  const bf16x8 zero8 = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
#pragma unroll 1
  for (int it = 0; it < QI; ++it) {
  // ---- scores: S^T tile t = K[16t .. 16t+15] Q^T: this lane holds keys 16t + 4g + r of query l15 ---------------------------------
  const int q_row = (qb * QI + it) * 64 + w * 16 + l15;
  if ((qb * QI + it) * 64 >= S_pad) break;
  const int q_ld = q_row < S_pad ? q_row : S_pad - 1;
  bf16x8 qf[3];
#pragma unroll
  for (int ds = 0; ds < 2; ++ds) qf[ds] = *(const bf16x8*)(q + (int64_t)q_ld * ldq + head * 80 + ds * 32 + g * 8);
  qf[2] = zero8;
  if (g < 2) qf[2] = *(const bf16x8*)(q + (int64_t)q_ld * ldq + head * 80 + 64 + g * 8);
  const float* brow = bias ? bias + head * bias_hs + (int64_t)q_ld * S_pad + 4 * g : nullptr;
  f32x4 s[TA80_NT];
  float mx = -__builtin_huge_valf();
#pragma unroll
  for (int t = 0; t < TA80_NT; ++t) {
    if (t < nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int r = t * 16 + l15;
#pragma unroll
      for (int ds = 0; ds < 2; ++ds) {
        const bf16x8 kf = *(const bf16x8*)(kl + r * 160 + ((ds * 4 + g) << 4));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ds], acc, 0, 0, 0);
      }
      bf16x8 kf2 = zero8;
      if (g < 2) kf2 = *(const bf16x8*)(kl + r * 160 + ((8 + g) << 4));
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf2, qf[2], acc, 0, 0, 0);
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (brow) b = *(const f32x4*)(brow + t * 16);
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        acc[r2] = acc[r2] * sl2 + b[r2] * LOG2E;
        mx = fmaxf(mx, acc[r2]);
      }
      s[t] = acc;
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if (!(mx > -__builtin_huge_valf())) mx = 0.f;   // a fully masked (padded) query row: keep the arithmetic finite
  // ---- P = exp2(s - max), row sums, O^T += V^T P^T per 32-key block ------------------------------------------------------------------
  f32x4 oacc[5];
#pragma unroll
  for (int dt = 0; dt < 5; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
#pragma unroll
  for (int b = 0; b < TA80_NT / 2; ++b) {
    if (2 * b < nt) {
      float p[8];
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        p[r2] = __builtin_amdgcn_exp2f(s[2 * b][r2] - mx);
        p[4 + r2] = __builtin_amdgcn_exp2f(s[2 * b + 1][r2] - mx);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) l += p[i];
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pack8(p));
#pragma unroll
      for (int dt = 0; dt < 5; ++dt) {
        const bf16x8 vf = *(const bf16x8*)(vl + (dt * 16 + l15) * vpitch + b * 64 + ((g ^ vsw) << 4));
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[dt], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q_row < S) {
    const float inv = 1.0f / l;
    bf16_t* orow = out + (int64_t)q_row * ldo + head * 80 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) {
      u32x2 v;
      v[0] = pack2(oacc[dt][0] * inv, oacc[dt][1] * inv);
      v[1] = pack2(oacc[dt][2] * inv, oacc[dt][3] * inv);
      *(u32x2*)(orow + dt * 16) = v;
    }
  }
  }   // it
}

// ---- attention, head dim 64, keys streamed through the LDS (S_pad <= TAS_MAXS) --------------------------------------------------------
// attn64_kernel's operand contract word for word (q, k [S_pad][ld], vt [heads * 64][ldvt], bias fp32 [.][S_pad][S_pad] with head stride
// bias_hs or NULL, out [S][ldo], scale, S_pad % 32 == 0, blockIdx.z = sequence, rows / keys >= S masked by the bias alone, rows >= S
// not written) for towers with more keys than a CU's LDS holds (ViT-L/14 at 336 px: 577 tokens, S_pad 608).  Decisions:
//   * Chunks of TAS_CK = 128 keys, two LDS buffers.  A buffer is attn64_kernel's image of a 128-key head: K rows of 128 B with the
//     16-byte chunk c of row r at c ^ (r & 7), V^T rows of pitch 2 * 128 + 16 B with the key slots of every 32-key block permuted
//     (slot(key) = 8 (key%16 / 4) + 4 (key / 16) + key % 4); chunk-local rows and blocks, and 128 % 32 == 0, so both formulas are
//     the resident kernel's with S_pad = 128 (V^T fragment reads stay 2-way under the bank model, as there).
//   * LDS budget: 2 x (128 * 128 + 64 * 272) = 67,584 B whatever S_pad is: two workgroups per CU (160 KiB / 66 KiB), i.e. two waves
//     per SIMD, which __launch_bounds__(256, 2) also asks of the register allocator (<= 256 VGPR + AGPR).  256 keys per chunk would
//     be 133,120 B = one workgroup per CU and twice the score registers for half the barriers; with one barrier per chunk and the
//     next chunk's loads in flight the barrier is not what this kernel waits for.
//   * Double buffering: chunk c + 1 is loaded from global memory into registers (4 + 4 x 16 B per thread) BEFORE the MFMAs of chunk
//     c and written to the other buffer after them; one __syncthreads per chunk (buffer (c + 1) & 1 was last read in iteration
//     c - 1, which every wave has left).  The last chunk may be partial (a multiple of 32 keys): loads, LDS writes, score tiles and
//     PV blocks past its keys are skipped by workgroup-uniform tests.
//   * Online softmax in the exp2 domain, per query: running maximum m and running sum l (each lane keeps the partial sum of its own
//     keys, reduced over the four lane groups once at the end, as in the resident kernel).  Per chunk: scores of <= 8 tiles in
//     registers (32 per query tile instead of the resident kernel's 128), chunk maximum over the lane groups, m' = max(m, chunk),
//     alpha = exp2(m - m'), O and l scaled by alpha in fp32, P = exp2(s - m') rounded to bf16 once for the PV MFMA, l += the
//     unrounded P.  While a query has seen only -inf (causal rows ahead of their first key, padded rows) the subtrahend is 0, not
//     -inf: P = exp2(-inf) = 0 and alpha = exp2(-inf - 0) = 0 on a state of zeros.  A chunk of -inf under a finite m gives m' = m,
//     alpha = exp2(0) = 1 exactly and P = 0: the state is unchanged bit for bit.  1 / l is formed only for rows that are written.
//   * QI as in attn64_kernel: a workgroup stages every chunk once for 64 * QI queries; the QI tiles of a wave keep separate states
//     and run the same instructions in the same order as one tile alone, and the multiply-adds that could contract differently are
//     written as fmaf.  No atomics, fixed order: results are bitwise repeatable and depend on neither B nor QI.
constexpr int TAS_CK = 128;                        // keys per chunk
constexpr int TAS_VP = TAS_CK * 2 + 16;            // V^T row pitch of a chunk, bytes
constexpr int TAS_KB = TAS_CK * 128;               // K image of a chunk, bytes
constexpr int TAS_BUF = TAS_KB + 64 * TAS_VP;      // one buffer
constexpr int TAS_LDS = 2 * TAS_BUF;
static_assert(TAS_CK % 32 == 0 && TAS_CK * 8 == 4 * 256 && 64 * (TAS_CK / 8) == 4 * 256, "a thread stages 4 + 4 16-byte pieces of a chunk");
static_assert(2 * TAS_LDS <= 160 * 1024, "two workgroups per CU");

// chunk's K rows and V^T columns -> registers; nk: its keys (0: nothing to load)
__device__ __forceinline__ void tas_fetch(u32x4 (&kr)[4], u32x4 (&vr)[4], const bf16_t* __restrict__ k, int64_t ldk, const bf16_t* __restrict__ vt,
                                          int64_t ldvt, int head, int key0, int nk, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + i * 256;
    const int r = idx >> 3, c = idx & 7;
    if (r < nk) kr[i] = *(const u32x4*)(k + (int64_t)(key0 + r) * ldk + head * 64 + c * 8);
    const int d = idx >> 4, m = idx & 15;
    if (m * 8 < nk) vr[i] = *(const u32x4*)(vt + (int64_t)(head * 64 + d) * ldvt + key0 + m * 8);
  }
}

// registers -> one LDS buffer, in attn64_kernel's images
__device__ __forceinline__ void tas_stash(const u32x4 (&kr)[4], const u32x4 (&vr)[4], char* buf, int nk, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + i * 256;
    const int r = idx >> 3, c = idx & 7;
    if (r < nk) *(u32x4*)(buf + r * 128 + ((c ^ (r & 7)) << 4)) = kr[i];
    const int d = idx >> 4, m = idx & 15;
    if (m * 8 < nk) {
      const int blk = (m * 8) >> 5, kap = (m * 8) & 31;
      const int tile = kap >> 4, g0 = (kap & 15) >> 2;
      char* dst = buf + TAS_KB + d * TAS_VP + blk * 64;
      u32x2 lo, hi;
      lo[0] = vr[i][0]; lo[1] = vr[i][1]; hi[0] = vr[i][2]; hi[1] = vr[i][3];
      *(u32x2*)(dst + (8 * g0 + 4 * tile) * 2) = lo;
      *(u32x2*)(dst + (8 * (g0 + 1) + 4 * tile) * 2) = hi;
    }
  }
}

template <int QI>   // query tiles per wave, as attn64_kernel
__global__ __launch_bounds__(256, 2) void attn64_stream_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                               const bf16_t* __restrict__ vt, int64_t ldvt, const float* __restrict__ bias,
                                                               int64_t bias_hs, bf16_t* __restrict__ out, int64_t ldo, int S, int S_pad, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int head = blockIdx.y, qb = blockIdx.x;
  {
    const int64_t r0 = (int64_t)blockIdx.z * S_pad;
    q += r0 * ldq; k += r0 * ldk; vt += r0; out += r0 * ldo;
  }
  const float NINF = -__builtin_huge_valf();
  const float LOG2E = 1.4426950408889634f;
  const float sl2 = scale * LOG2E;
  // ---- per query tile: Q fragments, bias row, softmax state -----------------------------------------------------------------------
  bf16x8 qf[QI][2];
  const float* brow[QI];
  float mrun[QI], lrun[QI];
  f32x4 oacc[QI][4];
#pragma unroll
  for (int it = 0; it < QI; ++it) {
    const int q_row = (qb * QI + it) * 64 + w * 16 + l15;
    const int q_ld = q_row < S_pad ? q_row : S_pad - 1;
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) qf[it][ds] = *(const bf16x8*)(q + (int64_t)q_ld * ldq + head * 64 + ds * 32 + g * 8);
    brow[it] = bias ? bias + head * bias_hs + (int64_t)q_ld * S_pad + 4 * g : nullptr;
    mrun[it] = NINF;
    lrun[it] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[it][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // ---- chunk 0 -> buffer 0 -----------------------------------------------------------------------------------------------------------
  const int nch = (S_pad + TAS_CK - 1) / TAS_CK;
  u32x4 kr[4], vr[4];
  tas_fetch(kr, vr, k, ldk, vt, ldvt, head, 0, min(TAS_CK, S_pad), tid);
  tas_stash(kr, vr, smem, min(TAS_CK, S_pad), tid);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const int key0 = c * TAS_CK, nk = min(TAS_CK, S_pad - key0);
    const int nk_next = c + 1 < nch ? min(TAS_CK, S_pad - key0 - TAS_CK) : 0;
    tas_fetch(kr, vr, k, ldk, vt, ldvt, head, key0 + TAS_CK, nk_next, tid);   // in flight under this chunk's MFMAs
    const char* const kl = smem + (c & 1) * TAS_BUF;
    const char* const vl = kl + TAS_KB;
    const int nt = nk >> 4;
#pragma unroll
    for (int it = 0; it < QI; ++it) {
      if ((qb * QI + it) * 64 < S_pad) {
        // scores: S^T tile t = K[key0 + 16t ..] Q^T: this lane holds keys key0 + 16t + 4g + r of query l15
        f32x4 s[TAS_CK / 16];
        float cm = NINF;
#pragma unroll
        for (int t = 0; t < TAS_CK / 16; ++t) {
          if (t < nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int r = t * 16 + l15;
#pragma unroll
            for (int ds = 0; ds < 2; ++ds) {
              const bf16x8 kf = *(const bf16x8*)(kl + r * 128 + (((ds * 4 + g) ^ (r & 7)) << 4));
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[it][ds], acc, 0, 0, 0);
            }
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (brow[it]) b = *(const f32x4*)(brow[it] + key0 + t * 16);
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
              acc[r2] = __builtin_fmaf(acc[r2], sl2, b[r2] * LOG2E);
              cm = fmaxf(cm, acc[r2]);
            }
            s[t] = acc;
          }
        }
        cm = fmaxf(cm, __shfl_xor(cm, 16));
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mnew = fmaxf(mrun[it], cm);
        const float msub = mnew > NINF ? mnew : 0.f;               // only -inf so far: keep the arithmetic finite
        const float alpha = __builtin_amdgcn_exp2f(mrun[it] - msub);   // -inf - finite: 0; m unchanged: exp2(0) = 1
        mrun[it] = mnew;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int r2 = 0; r2 < 4; ++r2) oacc[it][dt][r2] *= alpha;
        float ls = 0.f;
#pragma unroll
        for (int b = 0; b < TAS_CK / 32; ++b) {
          if (2 * b < nt) {
            float p[8];
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
              p[r2] = __builtin_amdgcn_exp2f(s[2 * b][r2] - msub);
              p[4 + r2] = __builtin_amdgcn_exp2f(s[2 * b + 1][r2] - msub);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ls += p[i];
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pack8(p));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
              const bf16x8 vf = *(const bf16x8*)(vl + (dt * 16 + l15) * TAS_VP + b * 64 + g * 16);
              oacc[it][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[it][dt], 0, 0, 0);
            }
          }
        }
        lrun[it] = __builtin_fmaf(lrun[it], alpha, ls);
      }
    }
    tas_stash(kr, vr, smem + ((c + 1) & 1) * TAS_BUF, nk_next, tid);
    __syncthreads();
  }
#pragma unroll
  for (int it = 0; it < QI; ++it) {
    const int q_row = (qb * QI + it) * 64 + w * 16 + l15;
    float l = lrun[it];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (q_row < S) {
      const float inv = 1.0f / l;
      bf16_t* orow = out + (int64_t)q_row * ldo + head * 64 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        u32x2 v;
        v[0] = pack2(oacc[it][dt][0] * inv, oacc[it][dt][1] * inv);
        v[1] = pack2(oacc[it][dt][2] * inv, oacc[it][dt][3] * inv);
        *(u32x2*)(orow + dt * 16) = v;
      }
    }
  }
}

// ---- attention, head dim 80, keys streamed through the LDS (S_pad <= TAS80_MAXS) ------------------------------------------------------
// attn80_kernel's operand contract word for word (q, k [S_pad][ld] with head h in columns 80 h .., vt [heads * 80][ldvt], bias fp32
// [.][S_pad][S_pad] with head stride bias_hs or NULL, out [S][ldo], scale, S_pad % 32 == 0, blockIdx.z = sequence, rows / keys >= S
// masked by the bias alone, rows >= S not written) for towers with more than TA80_MAXS = 480 keys: SigLIP so400m/14 at 384 px has 729
// tokens (S_pad 736) of 16 heads x 72 channels, which its binding zero-pads to 80.  Built as attn64_stream_kernel is; decisions:
//   * Chunks of TAS80_CK = 96 keys, two LDS buffers.  A buffer is attn80_kernel's image of a 96-key head: K rows of 160 B as they lie
//     in memory (unswizzled: row r starts at slot 10 r mod 16, conflict-free as argued above attn80_kernel), V^T rows of pitch
//     64 * m bytes with m = 96 / 32 = 3, which is odd WITHOUT a padding block, 16-byte chunk g of a key block at g ^ {0, 2, 3, 1}[(d & 15) >> 2],
//     key slots permuted (slot(key) = 8 (key%16 / 4) + 4 (key / 16) + key % 4).  Both buffers start on a multiple of 256 B, so the
//     fragment-read formulas are the resident kernel's at S_pad = 96 and conflict-free in either buffer.
//   * LDS budget: 2 x (96 * 160 + 80 * 192) = 61,440 B whatever S_pad is: two workgroups per CU (160 KiB / 60 KiB), i.e. two waves
//     per SIMD, as __launch_bounds__(256, 2) asks of the register allocator, like the head-dim-64 streaming kernel.  The alternative,
//     128 keys per chunk, needs m = 4 -> 5 (a padding block), 2 x 46,080 = 92,160 B = ONE workgroup per CU, 8 instead of 6 score
//     tiles in registers per query tile and three quarters of the barriers.  The choice is by that arithmetic: a second workgroup per
//     CU hides one's barrier and softmax under the other's MFMAs, and the QI = 4 instantiation (80 accumulator + 48 Q-fragment
//     registers per lane before any score) has no room for 8 more score registers under a 256-register cap: as it is, the compiler
//     reports 164 VGPRs for QI = 1 and 256 VGPRs plus 14 spilled (60 B of scratch per lane) for QI = 4.  Neither chunk size has been
//     timed against the other.
//   * A chunk is 96 * 10 = 960 16-byte pieces of K and 80 * 12 = 960 of V^T: thread tid moves pieces tid + 256 i, i < 4, of each (the
//     last 64 indices are past the chunk and skipped).  Double buffering, the one barrier per chunk, the partial last chunk (32 or 64
//     keys, skipped by workgroup-uniform tests) and the online softmax with its all--inf conventions are attn64_stream_kernel's
//     (header above), with 5 output tiles and the 32 + 32 + 16 channel split of attn80_kernel: lane groups 2, 3 of the third MFMA
//     hold zeros and load nothing.
//   * QI tiles keep separate states and run one tile's instructions in one tile's order; multiply-adds that could contract
//     differently are fmaf.  No atomics, fixed order: bitwise repeatable, independent of B and QI.
// tests/test_siglip_cpu.py restates the LDS addresses against the bank model; tests/test_siglip_attention_gpu.py holds the parity.
constexpr int TAS80_CK = 96;                         // keys per chunk
constexpr int TAS80_VP = 64 * (TAS80_CK / 32);       // V^T row pitch of a chunk, bytes (m = 3: odd)
constexpr int TAS80_KB = TAS80_CK * 160;             // K image of a chunk, bytes
constexpr int TAS80_BUF = TAS80_KB + 80 * TAS80_VP;  // one buffer
constexpr int TAS80_LDS = 2 * TAS80_BUF;
constexpr int TAS80_NP = TAS80_CK * 10;              // 16-byte pieces of a chunk's K; as many of its V^T
static_assert(TAS80_CK % 32 == 0 && (TAS80_CK / 32) % 2 == 1 && TAS80_NP == 80 * (TAS80_CK / 8) && TAS80_NP <= 4 * 256, "a thread stages <= 4 + 4 pieces");
static_assert(TAS80_BUF % 256 == 0 && TAS80_KB % 256 == 0 && 2 * TAS80_LDS <= 160 * 1024, "bank-aligned images, two workgroups per CU");

// chunk's K rows and V^T columns -> registers; nk: its keys (0: nothing to load)
__device__ __forceinline__ void tas80_fetch(u32x4 (&kr)[4], u32x4 (&vr)[4], const bf16_t* __restrict__ k, int64_t ldk, const bf16_t* __restrict__ vt,
                                            int64_t ldvt, int head, int key0, int nk, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + i * 256;
    const int r = idx / 10, c = idx - r * 10;
    if (idx < nk * 10) kr[i] = *(const u32x4*)(k + (int64_t)(key0 + r) * ldk + head * 80 + c * 8);
    const int d = idx / (TAS80_CK / 8), m = idx - d * (TAS80_CK / 8);
    if (idx < TAS80_NP && m * 8 < nk) vr[i] = *(const u32x4*)(vt + (int64_t)(head * 80 + d) * ldvt + key0 + m * 8);
  }
}

// registers -> one LDS buffer, in attn80_kernel's images
__device__ __forceinline__ void tas80_stash(const u32x4 (&kr)[4], const u32x4 (&vr)[4], char* buf, int nk, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + i * 256;
    if (idx < nk * 10) *(u32x4*)(buf + idx * 16) = kr[i];
    const int d = idx / (TAS80_CK / 8), m = idx - d * (TAS80_CK / 8);
    if (idx < TAS80_NP && m * 8 < nk) {
      const int blk = (m * 8) >> 5, kap = (m * 8) & 31;
      const int tile = kap >> 4, g0 = (kap & 15) >> 2;
      const int sw = (0x78 >> (2 * ((d & 15) >> 2))) & 3;
      char* dst = buf + TAS80_KB + d * TAS80_VP + blk * 64 + 8 * tile;
      u32x2 lo, hi;
      lo[0] = vr[i][0]; lo[1] = vr[i][1]; hi[0] = vr[i][2]; hi[1] = vr[i][3];
      *(u32x2*)(dst + ((g0 ^ sw) << 4)) = lo;
      *(u32x2*)(dst + (((g0 + 1) ^ sw) << 4)) = hi;
    }
  }
}

template <int QI>   // query tiles per wave, as attn80_kernel
__global__ __launch_bounds__(256, 2) void attn80_stream_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                               const bf16_t* __restrict__ vt, int64_t ldvt, const float* __restrict__ bias,
                                                               int64_t bias_hs, bf16_t* __restrict__ out, int64_t ldo, int S, int S_pad, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int head = blockIdx.y, qb = blockIdx.x;
  {
    const int64_t r0 = (int64_t)blockIdx.z * S_pad;
    q += r0 * ldq; k += r0 * ldk; vt += r0; out += r0 * ldo;
  }
  const float NINF = -__builtin_huge_valf();
  const float LOG2E = 1.4426950408889634f;
  const float sl2 = scale * LOG2E;
  const int vsw = (0x78 >> (2 * (l15 >> 2))) & 3;   // every V^T fragment row is 16 dt + l15
  const bf16x8 zero8 = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
  // ---- per query tile: Q fragments, bias row, softmax state -----------------------------------------------------------------------
  bf16x8 qf[QI][3];
  const float* const bbase = bias ? bias + head * bias_hs : nullptr;   // uniform; a lane keeps a 32-bit offset per query tile
  int boff[QI];
  float mrun[QI], lrun[QI];
  f32x4 oacc[QI][5];
#pragma unroll
  for (int it = 0; it < QI; ++it) {
    const int q_row = (qb * QI + it) * 64 + w * 16 + l15;
    const int q_ld = q_row < S_pad ? q_row : S_pad - 1;
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) qf[it][ds] = *(const bf16x8*)(q + (int64_t)q_ld * ldq + head * 80 + ds * 32 + g * 8);
    qf[it][2] = zero8;
    if (g < 2) qf[it][2] = *(const bf16x8*)(q + (int64_t)q_ld * ldq + head * 80 + 64 + g * 8);
    boff[it] = q_ld * S_pad + 4 * g;   // < 2048^2
    mrun[it] = NINF;
    lrun[it] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) oacc[it][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // ---- chunk 0 -> buffer 0 -----------------------------------------------------------------------------------------------------------
  const int nch = (S_pad + TAS80_CK - 1) / TAS80_CK;
  u32x4 kr[4], vr[4];
  tas80_fetch(kr, vr, k, ldk, vt, ldvt, head, 0, min(TAS80_CK, S_pad), tid);
  tas80_stash(kr, vr, smem, min(TAS80_CK, S_pad), tid);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const int key0 = c * TAS80_CK, nk = min(TAS80_CK, S_pad - key0);
    const int nk_next = c + 1 < nch ? min(TAS80_CK, S_pad - key0 - TAS80_CK) : 0;
    tas80_fetch(kr, vr, k, ldk, vt, ldvt, head, key0 + TAS80_CK, nk_next, tid);   // in flight under this chunk's MFMAs
    const char* const kl = smem + (c & 1) * TAS80_BUF;
    const char* const vl = kl + TAS80_KB;
    const int nt = nk >> 4;
#pragma unroll
    for (int it = 0; it < QI; ++it) {
      if ((qb * QI + it) * 64 < S_pad) {
        // scores: S^T tile t = K[key0 + 16t ..] Q^T: this lane holds keys key0 + 16t + 4g + r of query l15
        f32x4 s[TAS80_CK / 16];
        float cm = NINF;
#pragma unroll
        for (int t = 0; t < TAS80_CK / 16; ++t) {
          if (t < nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int r = t * 16 + l15;
#pragma unroll
            for (int ds = 0; ds < 2; ++ds) {
              const bf16x8 kf = *(const bf16x8*)(kl + r * 160 + ((ds * 4 + g) << 4));
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[it][ds], acc, 0, 0, 0);
            }
            bf16x8 kf2 = zero8;
            if (g < 2) kf2 = *(const bf16x8*)(kl + r * 160 + ((8 + g) << 4));
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf2, qf[it][2], acc, 0, 0, 0);
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (bbase) b = *(const f32x4*)(bbase + (boff[it] + key0 + t * 16));
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
              acc[r2] = __builtin_fmaf(acc[r2], sl2, b[r2] * LOG2E);
              cm = fmaxf(cm, acc[r2]);
            }
            s[t] = acc;
          }
        }
        cm = fmaxf(cm, __shfl_xor(cm, 16));
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mnew = fmaxf(mrun[it], cm);
        const float msub = mnew > NINF ? mnew : 0.f;               // only -inf so far: keep the arithmetic finite
        const float alpha = __builtin_amdgcn_exp2f(mrun[it] - msub);   // -inf - finite: 0; m unchanged: exp2(0) = 1
        mrun[it] = mnew;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt)
#pragma unroll
          for (int r2 = 0; r2 < 4; ++r2) oacc[it][dt][r2] *= alpha;
        float ls = 0.f;
#pragma unroll
        for (int b = 0; b < TAS80_CK / 32; ++b) {
          if (2 * b < nt) {
            float p[8];
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
              p[r2] = __builtin_amdgcn_exp2f(s[2 * b][r2] - msub);
              p[4 + r2] = __builtin_amdgcn_exp2f(s[2 * b + 1][r2] - msub);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ls += p[i];
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pack8(p));
#pragma unroll
            for (int dt = 0; dt < 5; ++dt) {
              const bf16x8 vf = *(const bf16x8*)(vl + (dt * 16 + l15) * TAS80_VP + b * 64 + ((g ^ vsw) << 4));
              oacc[it][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[it][dt], 0, 0, 0);
            }
          }
        }
        lrun[it] = __builtin_fmaf(lrun[it], alpha, ls);
      }
    }
    tas80_stash(kr, vr, smem + ((c + 1) & 1) * TAS80_BUF, nk_next, tid);
    __syncthreads();
  }
#pragma unroll
  for (int it = 0; it < QI; ++it) {
    const int q_row = (qb * QI + it) * 64 + w * 16 + l15;
    float l = lrun[it];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (q_row < S) {
      const float inv = 1.0f / l;
      bf16_t* orow = out + (int64_t)q_row * ldo + head * 80 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 5; ++dt) {
        u32x2 v;
        v[0] = pack2(oacc[it][dt][0] * inv, oacc[it][dt][1] * inv);
        v[1] = pack2(oacc[it][dt][2] * inv, oacc[it][dt][3] * inv);
        *(u32x2*)(orow + dt * 16) = v;
      }
    }
  }
}

// ---- host side (TextCtx / TextSizes: text_internal.hpp) ------------------------------------------------------------------------
int text_ctx(TextCtx& c, const TextSizes& z, int B, int S, int S_pad, const rf_workspace* ws, hipStream_t st, const char* who) {
  RF_REQUIRE(ws && ws->base && aligned16(ws->base) && ws->bytes >= z.total, RF_ERR_WORKSPACE, "%s: workspace %lld < required %lld bytes", who,
             (long long)(ws ? ws->bytes : 0), (long long)z.total);
  char* p = (char*)ws->base;
  auto take = [&](int64_t bytes) { char* q = p; p += round_up(bytes, 256); return q; };
  c.st = st; c.S = S; c.S_pad = S_pad; c.B = B; c.sched = RF_SCHED_AUTO;
  c.X = (bf16_t*)take(z.x); c.Xn = (bf16_t*)take(z.x); c.QK = (bf16_t*)take(z.qk); c.VT = (bf16_t*)take(z.vt);
  c.AO = (bf16_t*)take(z.ao); c.HID = (bf16_t*)take(z.hid); c.G = (bf16_t*)take(z.g);
  c.ones = (bf16_t*)take(16384 * 2);
  c.sk = take(TEXT_SK); c.sk_bytes = TEXT_SK;
  hipLaunchKernelGGL(fill_bf16_rows_kernel, dim3(64), dim3(256), 0, st, c.ones, (int64_t)16384, 1.0f);
  RF_CHECK_HIP(hipMemsetAsync(c.sk, 0, 4096, st));                       // stream-K flags: zeroed here on every call, the caller owes nothing
  RF_CHECK_HIP(hipMemsetAsync(c.Xn, 0, (size_t)z.x, st));                // padded rows start finite (zero) and stay finite: they run through
  RF_CHECK_HIP(hipMemsetAsync(c.AO, 0, (size_t)z.ao, st));                // the same norms as real rows; no real row ever reads them (masked keys)
  RF_LAUNCH_CHECK();
  return RF_OK;
}

// y[M x N] = epi(x[M x K] . w[N x K]^T + b) (+ residual)
int text_gemm(TextCtx& c, const bf16_t* x, int64_t ldx, const void* w, const void* b, int M, int N, int K, bf16_t* y, int64_t ldy, int epi,
              const bf16_t* residual) {
  rf_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.N = N; d.num_groups = 1; d.epilogue = residual ? RF_EPI_GATE_RES : epi;
  d.splitk_ws = c.sk; d.splitk_ws_bytes = c.sk_bytes;
  rf_gemm_group& G = d.g[0];
  G.seg[0].A = x; G.seg[0].lda = ldx; G.seg[0].W = w; G.seg[0].ldw = K; G.seg[0].K = K;
  G.bias = b; G.M = M; G.out = y; G.ldo = ldy;
  if (residual) { G.gate = c.ones; G.residual = residual; G.ldr = ldy; }
  if (c.sched != RF_SCHED_AUTO) {   // a caller-pinned schedule (the CLIP vision tower: batch-invariant rows), no split-K scratch
    d.schedule = c.sched; d.splitk_ws = nullptr; d.splitk_ws_bytes = 0;
    return rf_gemm_bf16(&d, c.st);
  }
  // A 512-token prompt is 2 rows of 256-tiles: 32 .. 160 output tiles with 64 .. 160 K-tiles each neither fill the 256 CUs with whole
  // tiles nor suit the 128-tile kernel AUTO picks below 200 tiles (417 TF): stream-K cuts the K-tile iterations evenly over the CUs
  {
    const int64_t t256 = (int64_t)cdiv(M, 256) * cdiv(N, 256);
    if (t256 >= 16 && t256 < 200 && K / 64 >= 16) d.schedule = RF_SCHED_STREAMK;
  }
  return rf_gemm_bf16(&d, c.st);
}

// token (+ position) embedding rows into the residual stream c.X
int text_embed_rows(TextCtx& c, const void* table, const void* pos, const int32_t* ids, int D, int vocab) {
  const int R = c.B * c.S_pad;
  ProfScope prof(RF_KC_ROWOP, (double)R * D * 6, c.st);
  hipLaunchKernelGGL(embed_rows_kernel, dim3(grid_for((int64_t)R * D / 8)), dim3(256), 0, c.st, (const bf16_t*)table, (const bf16_t*)pos, ids, c.X, c.S, c.S_pad,
                     R, D, vocab);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

int text_attn_max_keys(int head_dim) { return head_dim == 64 ? TA_MAXS : head_dim == 80 ? TA80_MAXS : 0; }   // 0: no kernel for that head dim
int text_attn_stream_max_keys(int head_dim) { return head_dim == 64 ? TAS_MAXS : 0; }                      // 0: no streaming kernel

// The one launch site of attn64_kernel / attn80_kernel / attn64_stream_kernel (the towers below, rf_text_attention and
// rf_debug_text_attention): the kernel, LDS size, grid, the dynamic-LDS attribute and the instantiation are decided here and nowhere
// else.  qi: 1 | 4 = that instantiation, 0 = the product's rule.  stream_keys: 0 = the product's rule (the resident kernel up to its key
// limit, at head dim 64 the streaming kernel beyond), 1 = the streaming kernel at any S_pad (head dim 64).
static int text_attention_launch(int head_dim, int qi, int stream_keys, const bf16_t* q, int64_t ldq, const bf16_t* k, int64_t ldk, const bf16_t* vt,
                                 int64_t ldvt, const float* bias, int64_t bias_hs, bf16_t* out, int64_t ldo, int heads, int B, int S, int S_pad,
                                 float scale, hipStream_t st) {
  const bool hd80 = head_dim == 80;
  // a workgroup stages the head's K and V^T (2 x 64 KiB at 512 keys) for its queries: with enough (head, sequence) pairs to fill the
  // CUs it takes 256 queries instead of 64 and stages a quarter as often; regroups query tiles only (batch invariance)
  const bool wide = qi ? qi == 4 : (int64_t)heads * B * cdiv(S_pad, 256) >= 256;
  const dim3 grid(cdiv(S_pad, wide ? 256 : 64), heads, B);
  if (stream_keys || (head_dim == 64 && S_pad > TA_MAXS)) {
    RF_REQUIRE(head_dim == 64, RF_ERR_UNSUPPORTED, "head-dim-%d attention: the streaming-keys kernel exists for head dim 64 only", head_dim);
    RF_REQUIRE(S_pad <= TAS_MAXS, RF_ERR_SHAPE, "head-dim-64 attention: S_pad=%d > %d keys, the limit of the streaming-keys kernel", S_pad, TAS_MAXS);
    static bool sattr = false;
    if (!sattr) {
      RF_CHECK_HIP(hipFuncSetAttribute((const void*)attn64_stream_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, TAS_LDS));
      RF_CHECK_HIP(hipFuncSetAttribute((const void*)attn64_stream_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, TAS_LDS));
      sattr = true;
    }
    ProfScope prof(RF_KC_ATTN, 4.0 * (double)S_pad * S_pad * (double)head_dim * heads * B, st);
    auto* const skern = wide ? attn64_stream_kernel<4> : attn64_stream_kernel<1>;
    hipLaunchKernelGGL(skern, grid, dim3(256), TAS_LDS, st, q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, S, S_pad, scale);
    RF_LAUNCH_CHECK();
    return RF_OK;
  }
  RF_REQUIRE(S_pad <= text_attn_max_keys(head_dim), RF_ERR_SHAPE, "head-dim-%d attention: S_pad=%d > %d keys (K and V^T stay resident in the 160 KiB LDS)",
             head_dim, S_pad, text_attn_max_keys(head_dim));
  const int lds = hd80 ? ta80_lds_bytes(S_pad) : ta_lds_bytes(S_pad);
  static bool attr[2] = {false, false};
  if (!attr[hd80]) {
    const int max_lds = hd80 ? ta80_lds_bytes(TA80_MAXS) : ta_lds_bytes(TA_MAXS);
    RF_CHECK_HIP(hipFuncSetAttribute(hd80 ? (const void*)attn80_kernel<1> : (const void*)attn64_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    RF_CHECK_HIP(hipFuncSetAttribute(hd80 ? (const void*)attn80_kernel<4> : (const void*)attn64_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    attr[hd80] = true;
  }
  ProfScope prof(RF_KC_ATTN, 4.0 * (double)S_pad * S_pad * (double)head_dim * heads * B, st);
  auto* const kern = hd80 ? (wide ? attn80_kernel<4> : attn80_kernel<1>) : (wide ? attn64_kernel<4> : attn64_kernel<1>);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, S, S_pad, scale);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

// The head-dim-80 route with streamed keys, beside the launch site above and taken by rf_text_attention80 and by clip_layers' route80
// (the SigLIP towers) alone (the CLIP entry points,
// rf_text_attention and rf_debug_text_attention keep their refusals at head dim 80): stream_keys = 0 launches attn80_kernel up to
// TA80_MAXS keys -- through text_attention_launch, i.e. the very launch the CLIP towers make -- and attn80_stream_kernel beyond;
// stream_keys = 1 launches attn80_stream_kernel at any S_pad.  qi and the grid as above.
static int text_attention80_launch(int qi, int stream_keys, const bf16_t* q, int64_t ldq, const bf16_t* k, int64_t ldk, const bf16_t* vt, int64_t ldvt,
                                   const float* bias, int64_t bias_hs, bf16_t* out, int64_t ldo, int heads, int B, int S, int S_pad, float scale,
                                   hipStream_t st) {
  if (!stream_keys && S_pad <= TA80_MAXS)
    return text_attention_launch(80, qi, 0, q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, heads, B, S, S_pad, scale, st);
  RF_REQUIRE(S_pad <= TAS80_MAXS, RF_ERR_SHAPE, "head-dim-80 attention: S_pad=%d > %d keys, the limit of the streaming-keys kernel", S_pad, TAS80_MAXS);
  const bool wide = qi ? qi == 4 : (int64_t)heads * B * cdiv(S_pad, 256) >= 256;
  const dim3 grid(cdiv(S_pad, wide ? 256 : 64), heads, B);
  static bool sattr = false;
  if (!sattr) {
    RF_CHECK_HIP(hipFuncSetAttribute((const void*)attn80_stream_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, TAS80_LDS));
    RF_CHECK_HIP(hipFuncSetAttribute((const void*)attn80_stream_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, TAS80_LDS));
    sattr = true;
  }
  ProfScope prof(RF_KC_ATTN, 4.0 * (double)S_pad * S_pad * 80.0 * heads * B, st);
  auto* const skern = wide ? attn80_stream_kernel<4> : attn80_stream_kernel<1>;
  hipLaunchKernelGGL(skern, grid, dim3(256), TAS80_LDS, st, q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, S, S_pad, scale);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

// q | k [R][2 * inner], V^T [inner][R], out [R][ld_ao] (ld_ao = inner, or inner rounded up to the GEMM's K-tile, see clip_layers)
int text_attention(TextCtx& c, int head_dim, int heads, int inner, int64_t ld_ao, const float* bias, int64_t bias_hs, float scale) {
  return text_attention_launch(head_dim, 0, 0, c.QK, (int64_t)2 * inner, c.QK + inner, (int64_t)2 * inner, c.VT, (int64_t)c.B * c.S_pad, bias, bias_hs, c.AO,
                               ld_ao, heads, c.B, c.S, c.S_pad, scale, c.st);
}

// A CLIP tower's activation over x[0 .. n) in place, n % 8 == 0
int clip_act_inplace(int act, bf16_t* x, int64_t n, hipStream_t st) {
  ProfScope prof(RF_KC_ROWOP, (double)n * 4, st);
  auto* const kern = act == RF_CLIP_ACT_GELU ? clip_act_kernel<RF_CLIP_ACT_GELU>
                     : act == RF_CLIP_ACT_GELU_TANH ? clip_act_kernel<RF_CLIP_ACT_GELU_TANH> : clip_act_kernel<RF_CLIP_ACT_QUICK_GELU>;
  hipLaunchKernelGGL(kern, dim3(grid_for(n / 8)), dim3(256), 0, st, x, n / 8);
  RF_LAUNCH_CHECK();
  return RF_OK;
}

// The pre-LN CLIP encoder layers over the residual stream c.X (B sequences of S_pad rows, width D, MLP width F): shared by the text
// tower (causal mask) and the vision tower (padded keys masked).  Every GEMM goes through text_gemm, i.e. c.sched decides the schedule.
// o: head dim (64 | 80) and activation (validated by clip_opts_check).  Dp = D rounded up to the GEMM's 64-element K-tile: the
// operands whose K axis is the hidden width (Xn, AO; the weights, packed by the binding) have row pitch Dp and zeros in columns
// D .. Dp - 1.  Dp == D for every hidden width that is a multiple of 64 (all head-dim-64 towers, ViT-H's 1280): nothing moves there.
// inner: the attention width heads * head_dim where it differs from D (the SigLIP towers: heads of d <= 80 channels zero-padded to 80 by
// the binding, so q | k is [R][2 inner], V^T [inner][R], w_o [D][Ip] with Ip = inner rounded up to the K-tile); 0 = D, the CLIP towers,
// for which every launch below is what it was.  route80: the attention goes through text_attention80_launch (head dim 80, keys
// streamed beyond 480) instead of text_attention; mask may then be NULL when S == S_pad.
int clip_layers(TextCtx& c, const rf_clip_layer* layer, int layers, int heads, int D, int F, const float* mask, float eps, const char* who,
                const rf_clip_tower_opts& o, int inner, bool route80) {
  const int R = c.B * c.S_pad, Dp = (int)round_up(D, 64), I = inner ? inner : D, Ip = (int)round_up(I, 64);
  hipStream_t st = c.st;
  if (Dp != D) RF_CHECK_HIP(hipMemsetAsync(c.Xn, 0, (size_t)R * Dp * 2, st));   // the pad columns of Xn: LayerNorm writes D columns per row
  for (int i = 0; i < layers; ++i) {
    const rf_clip_layer& L = layer[i];
    RF_REQUIRE(L.ln1_scale && L.ln1_shift && L.w_qk && L.b_qk && L.w_v && L.w_o && L.b_o && L.ln2_scale && L.ln2_shift && L.w_fc1 && L.b_fc1 && L.w_fc2 &&
                   L.b_fc2, RF_ERR_NULL, "%s: layer %d has NULL weights", who, i);
    RF_TRY(rf_layernorm_modulate(c.X, D, c.Xn, Dp, R, D, L.ln1_scale, L.ln1_shift, eps, st));
    RF_TRY(text_gemm(c, c.Xn, Dp, L.w_qk, L.b_qk, R, 2 * I, Dp, c.QK, 2 * I, RF_EPI_STORE, nullptr));
    RF_TRY(text_gemm(c, (const bf16_t*)L.w_v, Dp, c.Xn, nullptr, I, R, Dp, c.VT, R, RF_EPI_STORE, nullptr));
    if (route80)
      RF_TRY(text_attention80_launch(0, 0, c.QK, (int64_t)2 * I, c.QK + I, (int64_t)2 * I, c.VT, (int64_t)R, mask, 0, c.AO, Ip, heads, c.B, c.S, c.S_pad, 1.0f, st));
    else
      RF_TRY(text_attention(c, o.head_dim, heads, I, Ip, mask, 0, 1.0f));
    RF_TRY(text_gemm(c, c.AO, Ip, L.w_o, L.b_o, R, D, Ip, c.X, D, RF_EPI_STORE, c.X));
    RF_TRY(rf_layernorm_modulate(c.X, D, c.Xn, Dp, R, D, L.ln2_scale, L.ln2_shift, eps, st));
    RF_TRY(text_gemm(c, c.Xn, Dp, L.w_fc1, L.b_fc1, R, F, Dp, c.HID, F, RF_EPI_STORE, nullptr));
    RF_TRY(clip_act_inplace(o.act, c.HID, (int64_t)R * F, st));
    RF_TRY(text_gemm(c, c.HID, F, L.w_fc2, L.b_fc2, R, D, F, c.X, D, RF_EPI_STORE, c.X));
  }
  return RF_OK;
}

// head dim and activation of a CLIP tower + what they demand of its geometry; S_pad: the keys of one attention call
int clip_opts_check(const rf_clip_tower_opts* o, int hidden, int heads, int S_pad, const char* who) {
  RF_REQUIRE(o, RF_ERR_NULL, "%s: opts NULL", who);
  RF_REQUIRE(o->head_dim == 64 || o->head_dim == 80, RF_ERR_UNSUPPORTED, "%s: head_dim=%d (attention kernels exist for 64 and 80)", who, o->head_dim);
  RF_REQUIRE(o->act == RF_CLIP_ACT_QUICK_GELU || o->act == RF_CLIP_ACT_GELU, RF_ERR_UNSUPPORTED, "%s: act=%d (0 = quick_gelu, 1 = gelu)", who, o->act);
  RF_REQUIRE(heads > 0 && hidden == heads * o->head_dim && hidden <= 4096, RF_ERR_SHAPE, "%s: hidden=%d heads=%d head_dim=%d (need hidden = heads * head_dim <= 4096)",
             who, hidden, heads, o->head_dim);
  if (o->head_dim == 64) {   // beyond the resident kernel's keys the launch site streams them
    RF_REQUIRE(S_pad <= text_attn_stream_max_keys(64), RF_ERR_SHAPE, "%s: S_pad=%d > %d keys, the limit of the streaming-keys attention at head_dim 64", who,
               S_pad, text_attn_stream_max_keys(64));
    return RF_OK;
  }
  const int lim = text_attn_max_keys(o->head_dim);
  RF_REQUIRE(S_pad <= lim, RF_ERR_SHAPE, "%s: S_pad=%d > %d keys, the limit at head_dim %d (K and V^T of a head stay resident in the 160 KiB LDS)", who,
             S_pad, lim, o->head_dim);
  return RF_OK;
}

}  // namespace rf

using namespace rf;

// Where a tower workspace of `total_bytes` (an rf_*_workspace_bytes answer) keeps its GEMM scratch: out = (offset, length) of the
// stream-K flag page, then of the partial tiles.  text_ctx carves it last and zeroes the flag page itself on every call.
extern "C" int rf_debug_text_workspace_layout(int64_t total_bytes, int64_t* out, int32_t n) {
  RF_REQUIRE(out, RF_ERR_NULL, "rf_debug_text_workspace_layout: out NULL");
  RF_REQUIRE(total_bytes > TEXT_SK && n >= 2, RF_ERR_SHAPE, "rf_debug_text_workspace_layout: total_bytes=%lld n=%d (need a tower's size and room for 2 pairs)",
             (long long)total_bytes, n);
  out[0] = total_bytes - TEXT_SK; out[1] = 4096;
  out[2] = total_bytes - TEXT_SK + 4096; out[3] = TEXT_SK - 4096;
  return 2;
}

static int t5_check(const rf_t5_weights* w, int32_t S, const char* who) {
  RF_REQUIRE(w && w->layer && w->embed && w->final_ln, RF_ERR_NULL, "%s: weights NULL", who);
  RF_REQUIRE(w->layers > 0 && w->heads > 0 && w->d_model > 0 && w->d_model % 64 == 0 && w->d_model <= 4096 && w->d_ff > 0 && w->d_ff % 64 == 0,
             RF_ERR_SHAPE, "%s: layers=%d heads=%d d_model=%d d_ff=%d (need d_model %% 64 == 0, <= 4096, d_ff %% 64 == 0)", who, w->layers, w->heads,
             w->d_model, w->d_ff);
  RF_REQUIRE(w->d_kv == 64, RF_ERR_UNSUPPORTED, "%s: the attention kernel is built for d_kv = 64 (got %d)", who, w->d_kv);
  RF_REQUIRE(S > 0 && S <= TA_MAXS, RF_ERR_SHAPE, "%s: S=%d (1 .. %d)", who, S, TA_MAXS);
  return RF_OK;
}

extern "C" int64_t rf_t5_workspace_bytes(const rf_t5_weights* w, int32_t B, int32_t S) {
  if (t5_check(w, S, "rf_t5_workspace_bytes") != RF_OK || B <= 0 || B > 64) return RF_ERR_SHAPE;
  const int S_pad = (int)round_up(S, 32);
  return text_sizes(B * S_pad, w->d_model, w->heads * 64, w->d_ff, 2 * w->d_ff).total;
}

// T5EncoderModel(ids)[0] for B sequences of S tokens: ids [B][S] int32 on the device -> out [B][S][ld_out] bf16 (final RMS norm
// applied).  pos_bias: [heads][S_pad][S_pad] fp32 for S_pad = round_up(S, 32) -- layer 0's bucketed relative-position bias, -inf in
// the columns of padded keys (built once per S by the binding: integer bucketing + one gather).  Internally every sequence owns
// S_pad rows; the projections and the FFN run over all B * S_pad rows at once.
extern "C" int rf_t5_encode(const rf_t5_weights* w, const int32_t* ids, int32_t B, int32_t S, void* out, int64_t ld_out, const rf_workspace* ws,
                            void* stream) {
  RF_TRY(t5_check(w, S, "rf_t5_encode"));
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_t5_encode: B=%d (1 .. 64)", B);
  RF_REQUIRE(ids && out && aligned16(out) && ld_out % 8 == 0 && ld_out >= w->d_model, RF_ERR_NULL, "rf_t5_encode: NULL / unaligned tensor");
  const int S_pad = (int)round_up(S, 32), D = w->d_model, inner = w->heads * 64, F = w->d_ff, R = B * S_pad;
  RF_REQUIRE(w->pos_bias && w->bias_S == S_pad, RF_ERR_SHAPE, "rf_t5_encode: pos_bias is built for S_pad = %d, this call needs %d", w->bias_S, S_pad);
  hipStream_t st = (hipStream_t)stream;
  TextCtx c;
  RF_TRY(text_ctx(c, text_sizes(R, D, inner, F, 2 * F), B, S, S_pad, ws, st, "rf_t5_encode"));
  {
    ProfScope prof(RF_KC_ROWOP, (double)R * D * 4, st);
    hipLaunchKernelGGL(embed_rows_kernel, dim3(grid_for((int64_t)R * D / 8)), dim3(256), 0, st, (const bf16_t*)w->embed, (const bf16_t*)nullptr, ids, c.X, S,
                       S_pad, R, D, w->vocab);
    RF_LAUNCH_CHECK();
  }
  auto rms = [&](const void* g, const bf16_t* x, bf16_t* y) {
    ProfScope prof(RF_KC_ROWOP, (double)R * D * 4, st);
    hipLaunchKernelGGL(rms_norm_rows_kernel, dim3(cdiv(R, 4)), dim3(256), 0, st, x, (const bf16_t*)g, y, R, D, w->eps);
    return hipGetLastError() == hipSuccess ? RF_OK : RF_ERR_HIP;
  };
  for (int i = 0; i < w->layers; ++i) {
    const rf_t5_layer& L = w->layer[i];
    RF_REQUIRE(L.ln0 && L.w_qk && L.w_v && L.w_o && L.ln1 && L.w_wi && L.w_wo, RF_ERR_NULL, "rf_t5_encode: layer %d has NULL weights", i);
    RF_TRY(rms(L.ln0, c.X, c.Xn));
    RF_TRY(text_gemm(c, c.Xn, D, L.w_qk, nullptr, R, 2 * inner, D, c.QK, 2 * inner, RF_EPI_STORE, nullptr));
    RF_TRY(text_gemm(c, (const bf16_t*)L.w_v, D, c.Xn, nullptr, inner, R, D, c.VT, R, RF_EPI_STORE, nullptr));   // V^T = W_v x^T
    RF_TRY(text_attention(c, 64, w->heads, inner, inner, w->pos_bias, (int64_t)S_pad * S_pad, 1.0f));                       // T5: no 1/sqrt(d)
    RF_TRY(text_gemm(c, c.AO, inner, L.w_o, nullptr, R, D, inner, c.X, D, RF_EPI_STORE, c.X));
    RF_TRY(rms(L.ln1, c.X, c.Xn));
    RF_TRY(text_gemm(c, c.Xn, D, L.w_wi, nullptr, R, 2 * F, D, c.HID, 2 * F, RF_EPI_STORE, nullptr));
    {
      ProfScope prof(RF_KC_ROWOP, (double)R * F * 6, st);
      hipLaunchKernelGGL(geglu_rows_kernel, dim3(grid_for((int64_t)R * F / 8)), dim3(256), 0, st, c.HID, c.G, R, F);
      RF_LAUNCH_CHECK();
    }
    RF_TRY(text_gemm(c, c.G, F, L.w_wo, nullptr, R, D, F, c.X, D, RF_EPI_STORE, c.X));
  }
  RF_TRY(rms(w->final_ln, c.X, c.Xn));
  // the real rows of every sequence -> the caller's [B][S][ld_out]
  for (int b = 0; b < B; ++b)
    RF_CHECK_HIP(hipMemcpy2DAsync((char*)out + (int64_t)b * S * ld_out * 2, (size_t)ld_out * 2, c.Xn + (int64_t)b * S_pad * D, (size_t)D * 2, (size_t)D * 2,
                                  (size_t)S, hipMemcpyDeviceToDevice, st));
  return RF_OK;
}

static int clip_check(const rf_clip_weights* w, const rf_clip_tower_opts* o, int32_t S, const char* who) {
  RF_REQUIRE(w && w->layer && w->tok_embed && w->pos_embed && w->final_ln_scale && w->final_ln_shift, RF_ERR_NULL, "%s: weights NULL", who);
  RF_REQUIRE(w->layers > 0 && w->heads > 0 && w->hidden > 0 && w->hidden % 8 == 0 && w->hidden <= 4096 && w->inter > 0 && w->inter % 64 == 0, RF_ERR_SHAPE,
             "%s: layers=%d heads=%d hidden=%d inter=%d (need hidden %% 8 == 0, <= 4096, inter %% 64 == 0)", who, w->layers, w->heads, w->hidden, w->inter);
  RF_REQUIRE(S > 0 && S <= w->max_pos && S <= TA_MAXS, RF_ERR_SHAPE, "%s: S=%d (1 .. min(max_pos = %d, %d))", who, S, w->max_pos, TA_MAXS);
  return clip_opts_check(o, w->hidden, w->heads, (int)round_up(S, 32), who);
}

extern "C" int64_t rf_clip_text_workspace_bytes_opts(const rf_clip_weights* w, const rf_clip_tower_opts* o, int32_t B, int32_t S) {
  const int rc = clip_check(w, o, S, "rf_clip_text_workspace_bytes");
  if (rc != RF_OK) return rc;
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_clip_text_workspace_bytes: B=%d (1 .. 64)", B);
  const int S_pad = (int)round_up(S, 32), Dp = (int)round_up(w->hidden, 64);
  return text_sizes(B * S_pad, Dp, Dp, w->inter, w->inter).total;
}

extern "C" int64_t rf_clip_text_workspace_bytes(const rf_clip_weights* w, int32_t B, int32_t S) {
  const int64_t n = rf_clip_text_workspace_bytes_opts(w, &CLIP_L_OPTS, B, S);
  return n < 0 ? RF_ERR_SHAPE : n;
}

// CLIPTextModel(ids) for B sequences of S tokens: last_hidden_state [B][S][hidden] (final LayerNorm applied; may be NULL) and
// pooler_output [B][hidden] = the final-normed row eos_pos[b] of sequence b (HOST array; the binding finds the positions: argmax(ids)
// for the legacy eos_token_id == 2 config, else the first eos_token_id).  mask: [S_pad][S_pad] fp32, 0 on and below the diagonal,
// -inf above it and in the columns of padded keys.  The binding folds 1/sqrt(head_dim) into w_q / b_q, writes LayerNorm weights as
// (weight - 1, bias) pairs for rf_layernorm_modulate and folds v_proj.bias into the out-projection bias (softmax rows sum to 1).
extern "C" int rf_clip_text_encode_opts(const rf_clip_weights* w, const rf_clip_tower_opts* o, const int32_t* ids, int32_t B, int32_t S,
                                        const int32_t* eos_pos, void* last_hidden, void* pooled, const rf_workspace* ws, void* stream) {
  RF_TRY(clip_check(w, o, S, "rf_clip_text_encode"));
  RF_REQUIRE(B > 0 && B <= 64, RF_ERR_SHAPE, "rf_clip_text_encode: B=%d (1 .. 64)", B);
  RF_REQUIRE(ids && (last_hidden || pooled) && (eos_pos || !pooled), RF_ERR_NULL, "rf_clip_text_encode: NULL tensor");
  if (pooled)
    for (int b = 0; b < B; ++b)
      RF_REQUIRE(eos_pos[b] >= 0 && eos_pos[b] < S, RF_ERR_SHAPE, "rf_clip_text_encode: eos_pos[%d]=%d outside 0 .. %d", b, eos_pos[b], S - 1);
  const int S_pad = (int)round_up(S, 32), D = w->hidden, Dp = (int)round_up(D, 64), F = w->inter, R = B * S_pad;
  RF_REQUIRE(w->mask && w->mask_S == S_pad, RF_ERR_SHAPE, "rf_clip_text_encode: mask is built for S_pad = %d, this call needs %d", w->mask_S, S_pad);
  hipStream_t st = (hipStream_t)stream;
  TextCtx c;
  RF_TRY(text_ctx(c, text_sizes(R, Dp, Dp, F, F), B, S, S_pad, ws, st, "rf_clip_text_encode"));
  {
    ProfScope prof(RF_KC_ROWOP, (double)R * D * 6, st);
    hipLaunchKernelGGL(embed_rows_kernel, dim3(grid_for((int64_t)R * D / 8)), dim3(256), 0, st, (const bf16_t*)w->tok_embed, (const bf16_t*)w->pos_embed,
                       ids, c.X, S, S_pad, R, D, w->vocab);
    RF_LAUNCH_CHECK();
  }
  RF_TRY(clip_layers(c, w->layer, w->layers, w->heads, D, F, w->mask, w->eps, "rf_clip_text_encode", *o));
  RF_TRY(rf_layernorm_modulate(c.X, D, c.Xn, D, R, D, w->final_ln_scale, w->final_ln_shift, w->eps, st));
  for (int b = 0; b < B; ++b) {
    const bf16_t* src = c.Xn + (int64_t)b * S_pad * D;
    if (last_hidden) RF_CHECK_HIP(hipMemcpyAsync((char*)last_hidden + (int64_t)b * S * D * 2, src, (size_t)S * D * 2, hipMemcpyDeviceToDevice, st));
    if (pooled) RF_CHECK_HIP(hipMemcpyAsync((char*)pooled + (int64_t)b * D * 2, src + (int64_t)eos_pos[b] * D, (size_t)D * 2, hipMemcpyDeviceToDevice, st));
  }
  return RF_OK;
}

extern "C" int rf_clip_text_encode(const rf_clip_weights* w, const int32_t* ids, int32_t B, int32_t S, const int32_t* eos_pos, void* last_hidden,
                                   void* pooled, const rf_workspace* ws, void* stream) {
  return rf_clip_text_encode_opts(w, &CLIP_L_OPTS, ids, B, S, eos_pos, last_hidden, pooled, ws, stream);
}

// The activation of the ViT-H towers on its own (tests; a binding that runs an MLP of its own): x[0 .. n) in place, n % 8 == 0
extern "C" int rf_gelu_erf_inplace(void* x, int64_t n, void* stream) {
  RF_REQUIRE(x && aligned16(x), RF_ERR_NULL, "rf_gelu_erf_inplace: NULL / unaligned tensor");
  RF_REQUIRE(n > 0 && n % 8 == 0 && n / 8 / 256 < 0x7fffffffll, RF_ERR_SHAPE, "rf_gelu_erf_inplace: n=%lld (a positive multiple of 8)", (long long)n);
  return clip_act_inplace(RF_CLIP_ACT_GELU, (bf16_t*)x, n, (hipStream_t)stream);
}

// The argument checks of the two entry points below, before any HIP call: head_dim / qi are the caller's to check (their sets differ),
// lim = the most keys that entry point launches at this head dim.
static int text_attention_args_check(const char* who, int32_t head_dim, int lim, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt,
                                     int64_t ldvt, const float* bias, int64_t bias_hs, const void* out, int64_t ldo, int32_t heads, int32_t B, int32_t S,
                                     int32_t S_pad) {
  RF_REQUIRE(S_pad > 0 && S_pad % 32 == 0 && S_pad <= lim, RF_ERR_SHAPE, "%s: S_pad=%d (a multiple of 32, 32 .. %d at head_dim %d)", who, S_pad, lim, head_dim);
  RF_REQUIRE(S >= 1 && S <= S_pad, RF_ERR_SHAPE, "%s: S=%d (1 .. S_pad = %d)", who, S, S_pad);
  RF_REQUIRE(B >= 1 && B <= 64, RF_ERR_SHAPE, "%s: B=%d (1 .. 64)", who, B);
  RF_REQUIRE(heads >= 1 && (int64_t)heads * head_dim <= 4096, RF_ERR_SHAPE, "%s: heads=%d head_dim=%d (need 1 <= heads * head_dim <= 4096)", who, heads, head_dim);
  RF_REQUIRE(q && k && vt && out, RF_ERR_NULL, "%s: q / k / vt / out NULL", who);
  RF_REQUIRE(bias || S == S_pad, RF_ERR_NULL, "%s: bias NULL with S=%d < S_pad=%d (padded keys are masked by the bias alone)", who, S, S_pad);
  RF_REQUIRE(aligned16(q) && aligned16(k) && aligned16(vt) && aligned16(out) && aligned16(bias), RF_ERR_ALIGN, "%s: operand not 16-byte aligned", who);
  RF_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 8 == 0 && bias_hs % 4 == 0, RF_ERR_ALIGN,
             "%s: ldq=%lld ldk=%lld ldvt=%lld ldo=%lld (multiples of 8 elements), bias_hs=%lld (multiple of 4)", who, (long long)ldq, (long long)ldk,
             (long long)ldvt, (long long)ldo, (long long)bias_hs);
  const int64_t inner = (int64_t)heads * head_dim;
  RF_REQUIRE(ldq >= inner && ldk >= inner && ldo >= inner && ldvt >= (int64_t)B * S_pad, RF_ERR_SHAPE,
             "%s: ldq=%lld ldk=%lld ldo=%lld < heads * head_dim = %lld or ldvt=%lld < B * S_pad = %lld", who, (long long)ldq, (long long)ldk, (long long)ldo,
             (long long)inner, (long long)ldvt, (long long)B * S_pad);
  RF_REQUIRE(bias_hs == 0 || bias_hs >= (int64_t)S_pad * S_pad, RF_ERR_SHAPE, "%s: bias_hs=%lld (0 = shared by the heads, else >= S_pad^2 = %lld)", who,
             (long long)bias_hs, (long long)S_pad * S_pad);
  return RF_OK;
}

// One attention launch on caller buffers through the towers' own launch site (tests: parity of attn64_kernel / attn80_kernel at shapes,
// bias forms and scales no tower reaches).  Operands as documented above attn64_kernel; qi: 1 | 4 = that instantiation, 0 = the
// product's rule.  Everything is validated before the first HIP call.
extern "C" int rf_debug_text_attention(int32_t head_dim, int32_t qi, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                                       const float* bias, int64_t bias_hs, void* out, int64_t ldo, int32_t heads, int32_t B, int32_t S, int32_t S_pad,
                                       float scale, void* stream) {
  const char* who = "rf_debug_text_attention";
  RF_REQUIRE(head_dim == 64 || head_dim == 80, RF_ERR_UNSUPPORTED, "%s: head_dim=%d (attention kernels exist for 64 and 80)", who, head_dim);
  RF_REQUIRE(qi == 0 || qi == 1 || qi == 4, RF_ERR_UNSUPPORTED, "%s: qi=%d (instantiations exist for 1 and 4; 0 = the product's rule)", who, qi);
  RF_TRY(text_attention_args_check(who, head_dim, text_attn_max_keys(head_dim), q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, heads, B, S, S_pad));
  return text_attention_launch(head_dim, qi, 0, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)vt, ldvt, bias, bias_hs, (bf16_t*)out, ldo, heads, B,
                               S, S_pad, scale, (hipStream_t)stream);
}

// The head-dim-64 attention of the towers as a product call on caller buffers (a binding that runs its own encoder around it), through
// the same launch site: resident keys up to 512, streamed keys up to 2048.  stream_keys = 1 runs the streaming kernel at any S_pad (a
// per-call choice, nothing process-wide).  Everything is validated before the first HIP call, by the debug entry's checks.
extern "C" int rf_text_attention(int32_t head_dim, int32_t qi, int32_t stream_keys, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt,
                                 int64_t ldvt, const float* bias, int64_t bias_hs, void* out, int64_t ldo, int32_t heads, int32_t B, int32_t S, int32_t S_pad,
                                 float scale, void* stream) {
  const char* who = "rf_text_attention";
  RF_REQUIRE(head_dim == 64, RF_ERR_UNSUPPORTED, "%s: head_dim=%d (head dim 64 only; the streaming-keys kernel has no other)", who, head_dim);
  RF_REQUIRE(qi == 0 || qi == 1 || qi == 4, RF_ERR_UNSUPPORTED, "%s: qi=%d (instantiations exist for 1 and 4; 0 = the product's rule)", who, qi);
  RF_REQUIRE(stream_keys == 0 || stream_keys == 1, RF_ERR_UNSUPPORTED, "%s: stream_keys=%d (0 = resident up to %d keys and streamed beyond, 1 = streamed)", who,
             stream_keys, TA_MAXS);
  RF_TRY(text_attention_args_check(who, head_dim, text_attn_stream_max_keys(head_dim), q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, heads, B, S, S_pad));
  return text_attention_launch(head_dim, qi, stream_keys, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)vt, ldvt, bias, bias_hs, (bf16_t*)out, ldo,
                               heads, B, S, S_pad, scale, (hipStream_t)stream);
}

// rf_text_attention's contract at head dim 80 (a tower whose heads are 80 channels wide, or narrower ones zero-padded to 80 by the
// binding: SigLIP so400m's 72), through text_attention80_launch: resident keys up to 480 (attn80_kernel, the CLIP-H towers' launch),
// streamed keys up to 2048 (attn80_stream_kernel).  stream_keys = 1 runs the streaming kernel at any S_pad.  A symbol of its own, so
// rf_text_attention and the CLIP entry points answer head dim 80 as they always did.  Everything is validated before the first HIP call.
extern "C" int rf_text_attention80(int32_t qi, int32_t stream_keys, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                                   const float* bias, int64_t bias_hs, void* out, int64_t ldo, int32_t heads, int32_t B, int32_t S, int32_t S_pad, float scale,
                                   void* stream) {
  const char* who = "rf_text_attention80";
  RF_REQUIRE(qi == 0 || qi == 1 || qi == 4, RF_ERR_UNSUPPORTED, "%s: qi=%d (instantiations exist for 1 and 4; 0 = the product's rule)", who, qi);
  RF_REQUIRE(stream_keys == 0 || stream_keys == 1, RF_ERR_UNSUPPORTED, "%s: stream_keys=%d (0 = resident up to %d keys and streamed beyond, 1 = streamed)", who,
             stream_keys, TA80_MAXS);
  RF_TRY(text_attention_args_check(who, 80, TAS80_MAXS, q, ldq, k, ldk, vt, ldvt, bias, bias_hs, out, ldo, heads, B, S, S_pad));
  return text_attention80_launch(qi, stream_keys, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)vt, ldvt, bias, bias_hs, (bf16_t*)out, ldo, heads,
                                 B, S, S_pad, scale, (hipStream_t)stream);
}
