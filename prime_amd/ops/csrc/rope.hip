// Rotary position embedding (NeoX half-split / Llama "rotate_half") for
// gfx950. Elementwise + table-lookup: cos/sin are precomputed on HOST
// (guide App. B: on-device trig turns memory-bound into VALU-bound) and
// passed as fp32 tables [S, D/2].
//
// Tensor layout: [B, S, H, D] bf16, treated as rows of length D where
// row -> position = (row / H) % S. Forward and backward share a kernel
// (backward is rotation by -theta: sign = -1).
#include "common.h"

// Every kernel here rotates through rope_rot (common.h).
__global__ void rope_kernel(const bf16* __restrict__ x, bf16* __restrict__ y,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t, int64_t nrows,
                            int H, int S, int D, float sign,
                            int64_t pos_offset,
                            const int* __restrict__ pos_dev) {
  if (pos_dev) pos_offset = *pos_dev;  // hipGraph decode: dynamic position
  const int half = D / 2;  // multiple of 4 (head_dim 64/128)
  const int hv = half / 4;
  const int64_t total = nrows * hv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / hv;
    const int i4 = (int)(idx - row * hv) * 4;  // pair index within half
    const int64_t s = (row / H) % S + pos_offset;
    const bf16x4 x1 = *reinterpret_cast<const bf16x4*>(x + row * D + i4);
    const bf16x4 x2 = *reinterpret_cast<const bf16x4*>(x + row * D + half + i4);
    const f32x4v c = *reinterpret_cast<const f32x4v*>(cos_t + s * half + i4);
    const f32x4v sn = *reinterpret_cast<const f32x4v*>(sin_t + s * half + i4);
    bf16x4 y1, y2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rope_rot(x1.v[j], x2.v[j], c.v[j], sn.v[j], sign, y1.v[j], y2.v[j]);
    *reinterpret_cast<bf16x4*>(y + row * D + i4) = y1;
    *reinterpret_cast<bf16x4*>(y + row * D + half + i4) = y2;
  }
}

PRIME_API int prime_rope(hipStream_t stream, const void* x, void* y,
                         const void* cos_t, const void* sin_t, int64_t nrows,
                         int64_t H, int64_t S, int64_t D, int backward,
                         int64_t pos_offset, const void* pos_dev) {
  if (D % 8 != 0) return hipErrorInvalidValue;
  int64_t total = nrows * (D / 8);
  int grid = prime_grid(total, 256);
  hipLaunchKernelGGL(rope_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)x, (bf16*)y, (const float*)cos_t,
                     (const float*)sin_t, nrows, (int)H, (int)S, (int)D,
                     backward ? -1.f : 1.f, pos_offset, (const int*)pos_dev);
  return (int)hipGetLastError();
}

// Stride-aware forward: reads the H heads of each token from a packed row
// (x + token * in_stride + head_off + h * D, e.g. q or k inside the qkv GEMM
// output) and writes a contiguous [tokens, H, D] result, so no dense copy
// of the strided view is needed first. Same work split and arithmetic as
// rope_kernel.
__global__ void rope_strided_kernel(const bf16* __restrict__ x,
                                    bf16* __restrict__ y,
                                    const float* __restrict__ cos_t,
                                    const float* __restrict__ sin_t,
                                    int64_t nrows, int H, int S, int D,
                                    int64_t in_stride, int64_t head_off,
                                    float sign, int64_t pos_offset) {
  const int half = D / 2;
  const int hv = half / 4;
  const int64_t total = nrows * hv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / hv;
    const int i4 = (int)(idx - row * hv) * 4;
    const int64_t tok = row / H;
    const int h = (int)(row - tok * H);
    const int64_t s = tok % S + pos_offset;
    const bf16* xr = x + tok * in_stride + head_off + (int64_t)h * D;
    const bf16x4 x1 = *reinterpret_cast<const bf16x4*>(xr + i4);
    const bf16x4 x2 = *reinterpret_cast<const bf16x4*>(xr + half + i4);
    const f32x4v c = *reinterpret_cast<const f32x4v*>(cos_t + s * half + i4);
    const f32x4v sn = *reinterpret_cast<const f32x4v*>(sin_t + s * half + i4);
    bf16x4 y1, y2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rope_rot(x1.v[j], x2.v[j], c.v[j], sn.v[j], sign, y1.v[j], y2.v[j]);
    *reinterpret_cast<bf16x4*>(y + row * D + i4) = y1;
    *reinterpret_cast<bf16x4*>(y + row * D + half + i4) = y2;
  }
}

PRIME_API int prime_rope_strided(hipStream_t stream, const void* x, void* y,
                                 const void* cos_t, const void* sin_t,
                                 int64_t nrows, int64_t H, int64_t S,
                                 int64_t D, int64_t in_stride,
                                 int64_t head_off, int64_t pos_offset) {
  if (D % 8 != 0 || in_stride % 4 != 0 || head_off % 4 != 0 || H <= 0 ||
      S <= 0)
    return hipErrorInvalidValue;
  int64_t total = nrows * (D / 8);
  int grid = prime_grid(total, 256);
  hipLaunchKernelGGL(rope_strided_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)x, (bf16*)y, (const float*)cos_t,
                     (const float*)sin_t, nrows, (int)H, (int)S, (int)D,
                     in_stride, head_off, 1.f, pos_offset);
  return (int)hipGetLastError();
}

// Backward of {qkv split, RoPE on q and k}: reads the dense gradients
// dq [M,H,D], dk [M,Hkv,D] (both w.r.t. the ROTATED q/k) and dv [M,Hkv,D],
// un-rotates the q and k heads (sign = -1, as rope_kernel's backward) and
// writes the packed dqkv [M, C] plus its transpose dqkv^T [C, M],
// C = (H + 2 Hkv) * D, which the qkv dW GEMM consumes. Replaces two rope
// launches, a cat and a transpose pass. One block per 64 tokens x one
// head; the transpose goes through a padded LDS tile with 16 B accesses on
// both sides, as transpose_bshd_kernel does.
template <int D>
__global__ __launch_bounds__(256) void qkv_grad_pack_kernel(
    const bf16* __restrict__ dq, const bf16* __restrict__ dk,
    const bf16* __restrict__ dv, bf16* __restrict__ dqkv,
    bf16* __restrict__ dqkvt, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, int64_t M, int H, int Hkv, int S,
    float sign, int64_t pos_offset) {
  constexpr int TPD = D + 8;    // padded LDS row
  constexpr int HALF = D / 2;
  constexpr int UPR = HALF / 8;  // 8-pair units per token row
  __shared__ bf16 tile[64][TPD];
  const int NH = H + 2 * Hkv;
  const int hh = blockIdx.x % NH;
  const int64_t m0 = (int64_t)(blockIdx.x / NH) * 64;
  const int64_t C = (int64_t)NH * D;
  // wave-uniform source select
  const bf16* src;
  int sh, shn;
  bool rot = true;
  if (hh < H) { src = dq; sh = hh; shn = H; }
  else if (hh < H + Hkv) { src = dk; sh = hh - H; shn = Hkv; }
  else { src = dv; sh = hh - H - Hkv; shn = Hkv; rot = false; }
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < (64 * UPR) / 256; ++i) {
    const int un = i * 256 + t;
    const int r = un / UPR, i8 = (un % UPR) * 8;
    const int64_t m = m0 + r;
    const bf16* xr = src + (m * shn + sh) * D;
    const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(xr + i8);
    const bf16x8 x2 = *reinterpret_cast<const bf16x8*>(xr + HALF + i8);
    bf16x8 y1 = x1, y2 = x2;
    if (rot) {
      const int64_t s = m % S + pos_offset;
      const float* cr = cos_t + s * HALF + i8;
      const float* sr = sin_t + s * HALF + i8;
      const f32x4v c0 = *reinterpret_cast<const f32x4v*>(cr);
      const f32x4v c1 = *reinterpret_cast<const f32x4v*>(cr + 4);
      const f32x4v s0 = *reinterpret_cast<const f32x4v*>(sr);
      const f32x4v s1 = *reinterpret_cast<const f32x4v*>(sr + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rope_rot(x1.v[j], x2.v[j], c0.v[j], s0.v[j], sign, y1.v[j], y2.v[j]);
        rope_rot(x1.v[4 + j], x2.v[4 + j], c1.v[j], s1.v[j], sign,
                 y1.v[4 + j], y2.v[4 + j]);
      }
    }
    bf16* orow = dqkv + m * C + (int64_t)hh * D;
    *reinterpret_cast<bf16x8*>(orow + i8) = y1;
    *reinterpret_cast<bf16x8*>(orow + HALF + i8) = y2;
    *reinterpret_cast<bf16x8*>(&tile[r][i8]) = y1;
    *reinterpret_cast<bf16x8*>(&tile[r][HALF + i8]) = y2;
  }
  __syncthreads();
  // transposed store: dqkvt row = hh*D + d, cols = the tile's 64 tokens
#pragma unroll
  for (int i = 0; i < (D * 8) / 256; ++i) {
    const int un = i * 256 + t;
    const int d = un >> 3, s8 = (un & 7) * 8;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.v[j] = tile[s8 + j][d];
    *reinterpret_cast<bf16x8*>(dqkvt + ((int64_t)hh * D + d) * M + m0 + s8) = v;
  }
}

PRIME_API int prime_qkv_grad_pack(hipStream_t stream, const void* dq,
                                  const void* dk, const void* dv, void* dqkv,
                                  void* dqkvt, const void* cos_t,
                                  const void* sin_t, int64_t M, int64_t H,
                                  int64_t Hkv, int64_t S, int64_t D,
                                  int64_t pos_offset) {
  if (M <= 0 || M % 64 != 0 || H <= 0 || Hkv <= 0 || S <= 0 ||
      (D != 64 && D != 128))
    return hipErrorInvalidValue;
  const int64_t grid = (M / 64) * (H + 2 * Hkv);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  if (D == 128)
    hipLaunchKernelGGL((qkv_grad_pack_kernel<128>), dim3((int)grid), dim3(256),
                       0, stream, (const bf16*)dq, (const bf16*)dk,
                       (const bf16*)dv, (bf16*)dqkv, (bf16*)dqkvt,
                       (const float*)cos_t, (const float*)sin_t, M, (int)H,
                       (int)Hkv, (int)S, -1.f, pos_offset);
  else
    hipLaunchKernelGGL((qkv_grad_pack_kernel<64>), dim3((int)grid), dim3(256),
                       0, stream, (const bf16*)dq, (const bf16*)dk,
                       (const bf16*)dv, (bf16*)dqkv, (bf16*)dqkvt,
                       (const float*)cos_t, (const float*)sin_t, M, (int)H,
                       (int)Hkv, (int)S, -1.f, pos_offset);
  return (int)hipGetLastError();
}
