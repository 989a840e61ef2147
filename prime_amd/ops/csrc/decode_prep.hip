// Fused decode-step prep for gfx950 (batched serving path): one launch per
// layer takes the qkv GEMM output of ONE new token per sequence and
//   - rotates q at pos[b]              -> qout [B,H,D]
//   - rotates k at pos[b]              -> kc[b, pos[b]]
//   - copies v                         -> vc[b, pos[b]]
// replacing a split/view, two rope launches and two index_copy_.
//
// qkv [B, (H+2Hkv)*D] bf16, cos/sin [T, D/2] fp32, pos int32 [B] on the
// DEVICE, caches [B,Smax,Hkv,D]. The rotation goes through rope_rot with a
// runtime sign, the same work split as rope_kernel (4 pairs per thread), so
// q and k are bit-identical to prime_rope at pos_offset = pos[b].
// A slot with pos[b] < 0 or pos[b] >= min(Smax, T) is idle: no cache row is
// written for it and its q rows are zeros.
#include "common.h"

__global__ void decode_qkv_append_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ qout,
    bf16* __restrict__ kc, bf16* __restrict__ vc,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos, int64_t nrows, int H, int Hkv, int D,
    int Smax, int T, float sign) {
  const int half = D / 2;  // multiple of 4 (head_dim 64/128)
  const int hv = half / 4;
  const int NH = H + 2 * Hkv;
  const int lim = min(Smax, T);
  const int64_t total = nrows * hv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / hv;  // (b, head of the packed row)
    const int i4 = (int)(idx - row * hv) * 4;
    const int64_t b = row / NH;
    const int hh = (int)(row - b * NH);
    const int p = pos[b];
    const bool live = p >= 0 && p < lim;
    bf16* dst;
    bool rot = true;
    if (hh < H) {
      dst = qout + (b * H + hh) * D;
      if (!live) {
        bf16x4 z;
#pragma unroll
        for (int j = 0; j < 4; ++j) z.v[j] = f2bf(0.f);
        *reinterpret_cast<bf16x4*>(dst + i4) = z;
        *reinterpret_cast<bf16x4*>(dst + half + i4) = z;
        continue;
      }
    } else {
      if (!live) continue;
      const int hk = hh - H;
      if (hk < Hkv) {
        dst = kc + ((b * Smax + p) * Hkv + hk) * D;
      } else {
        dst = vc + ((b * Smax + p) * Hkv + (hk - Hkv)) * D;
        rot = false;
      }
    }
    const bf16* xr = qkv + row * D;
    const bf16x4 x1 = *reinterpret_cast<const bf16x4*>(xr + i4);
    const bf16x4 x2 = *reinterpret_cast<const bf16x4*>(xr + half + i4);
    bf16x4 y1 = x1, y2 = x2;
    if (rot) {
      const f32x4v c =
          *reinterpret_cast<const f32x4v*>(cos_t + (int64_t)p * half + i4);
      const f32x4v sn =
          *reinterpret_cast<const f32x4v*>(sin_t + (int64_t)p * half + i4);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rope_rot(x1.v[j], x2.v[j], c.v[j], sn.v[j], sign, y1.v[j], y2.v[j]);
    }
    *reinterpret_cast<bf16x4*>(dst + i4) = y1;
    *reinterpret_cast<bf16x4*>(dst + half + i4) = y2;
  }
}

PRIME_API int prime_decode_qkv_append(hipStream_t stream, const void* qkv,
                                      void* qout, void* kc, void* vc,
                                      const void* cos_t, const void* sin_t,
                                      const void* pos, int64_t B, int64_t H,
                                      int64_t Hkv, int64_t D, int64_t Smax,
                                      int64_t T) {
  if ((D != 64 && D != 128) || B < 1 || H < 1 || Hkv < 1 || Smax < 1 ||
      T < 1 || Smax > 0x7fffffff || T > 0x7fffffff || !pos)
    return hipErrorInvalidValue;
  const int64_t nrows = B * (H + 2 * Hkv);
  const int grid = prime_grid(nrows * (D / 8), 256);
  hipLaunchKernelGGL(decode_qkv_append_kernel, dim3(grid), dim3(256), 0,
                     stream, (const bf16*)qkv, (bf16*)qout, (bf16*)kc,
                     (bf16*)vc, (const float*)cos_t, (const float*)sin_t,
                     (const int*)pos, nrows, (int)H, (int)Hkv, (int)D,
                     (int)Smax, (int)T, 1.f);
  return (int)hipGetLastError();
}
