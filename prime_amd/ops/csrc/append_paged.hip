// Fused qkv prep + append into a PAGED bf16 KV cache (gfx950): the pass of
// decode_prep.hip (decode_qkv_append / decode_qkv_append_multi /
// prefill_qkv_append) with the destination row taken through the block
// table. For TN new tokens per sequence, token t of slot b
//   - rotates q at p = pos[b] + t          -> qout [B,TN,H,D]
//   - rotates k at p                        -> K pool row e*P + p % P
//   - copies v                              -> V pool row e*P + p % P
// with e = table[b, p / P]. Pools [n_pages, P, Hkv, D], table int32
// [B, max_pages] on the device, Smax = max_pages * P.
//
// Same work split (4 rotated pairs per thread, grid-stride over the packed
// rows) and the same rope_rot as the contiguous kernels: q and the rows
// written are bit-identical to theirs for the same token.
//
// A token is dead, with no pool row written and zero q rows, if pos[b] < 0,
// t >= n_new[b] (n_new == nullptr: one live token), p >= min(Smax, T_rope),
// or its table entry is outside [0, n_pages). An invalid entry is NOT
// clamped: a clamped write would land in someone else's page. The table is
// read only for tokens that pass the other three tests (p < Smax keeps the
// index inside the row).
//
// Compiled without the packed fp32 VALU instructions (ops/build.py,
// NO_PACKED_FP32).
#include "common.h"

__global__ void qkv_append_paged_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ qout,
    bf16* __restrict__ kc, bf16* __restrict__ vc,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos, const int* __restrict__ n_new,
    const int* __restrict__ table, int64_t nrows, int TN, int H, int Hkv,
    int D, int psh, int n_pages, int max_pages, int T, float sign) {
  const int half = D / 2;  // multiple of 4 (head_dim 64/128)
  const int hv = half / 4;
  const int NH = H + 2 * Hkv;
  const int lim = min(max_pages << psh, T);
  const int64_t total = nrows * hv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / hv;  // (b, t, head of the packed row)
    const int i4 = (int)(idx - row * hv) * 4;
    const int64_t bt = row / NH;
    const int hh = (int)(row - bt * NH);
    const int64_t b = bt / TN;
    const int t = (int)(bt - b * TN);
    const int p0 = pos[b];
    const int nb = n_new ? n_new[b] : 1;
    // p0 < lim - t, not p0 + t < lim: no overflow for any p0
    bool live = p0 >= 0 && t < nb && p0 < lim - t;
    const int p = p0 + t;
    int e = -1;
    if (live) {
      e = table[b * max_pages + (p >> psh)];
      live = e >= 0 && e < n_pages;
    }
    bf16* dst;
    bool rot = true;
    if (hh < H) {
      dst = qout + (bt * H + hh) * D;
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
      const int64_t prow = ((int64_t)e << psh) + (p & ((1 << psh) - 1));
      if (hk < Hkv) {
        dst = kc + (prow * Hkv + hk) * D;
      } else {
        dst = vc + (prow * Hkv + (hk - Hkv)) * D;
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

static int append_paged(hipStream_t stream, const void* qkv, void* qout,
                        void* kc, void* vc, const void* cos_t,
                        const void* sin_t, const void* pos, const void* n_new,
                        const void* table, int64_t B, int64_t TN, int64_t H,
                        int64_t Hkv, int64_t D, int64_t P, int64_t n_pages,
                        int64_t max_pages, int64_t T) {
  if ((D != 64 && D != 128) || (P != 64 && P != 128 && P != 256) || B < 1 ||
      TN < 1 || TN > 0x7fffffff || H < 1 || Hkv < 1 || n_pages < 1 ||
      max_pages < 1 || T < 1 || T > 0x7fffffff ||
      max_pages > 0x7fffffff / P || n_pages > 0x7fffffff / P || !pos || !table)
    return hipErrorInvalidValue;
  const int64_t nrows = B * TN * (H + 2 * Hkv);
  const int grid = prime_grid(nrows * (D / 8), 256);
  hipLaunchKernelGGL(qkv_append_paged_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)qkv, (bf16*)qout, (bf16*)kc, (bf16*)vc,
                     (const float*)cos_t, (const float*)sin_t, (const int*)pos,
                     (const int*)n_new, (const int*)table, nrows, (int)TN,
                     (int)H, (int)Hkv, (int)D, P == 64 ? 6 : (P == 128 ? 7 : 8),
                     (int)n_pages, (int)max_pages, (int)T, 1.f);
  return (int)hipGetLastError();
}

// One new token per sequence: qkv [B, (H+2Hkv)*D], qout [B,H,D]. T: rows of
// the cos / sin tables.
PRIME_API int prime_decode_qkv_append_paged(
    hipStream_t stream, const void* qkv, void* qout, void* kc, void* vc,
    const void* cos_t, const void* sin_t, const void* pos, const void* table,
    int64_t B, int64_t H, int64_t Hkv, int64_t D, int64_t P, int64_t n_pages,
    int64_t max_pages, int64_t T) {
  return append_paged(stream, qkv, qout, kc, vc, cos_t, sin_t, pos, nullptr,
                      table, B, 1, H, Hkv, D, P, n_pages, max_pages, T);
}

// TN new tokens per sequence (any TN >= 1): qkv [B,TN,(H+2Hkv)*D], qout
// [B,TN,H,D].
PRIME_API int prime_prefill_qkv_append_paged(
    hipStream_t stream, const void* qkv, void* qout, void* kc, void* vc,
    const void* cos_t, const void* sin_t, const void* pos, const void* n_new,
    const void* table, int64_t B, int64_t TN, int64_t H, int64_t Hkv,
    int64_t D, int64_t P, int64_t n_pages, int64_t max_pages, int64_t T) {
  if (!n_new) return hipErrorInvalidValue;
  return append_paged(stream, qkv, qout, kc, vc, cos_t, sin_t, pos, n_new,
                      table, B, TN, H, Hkv, D, P, n_pages, max_pages, T);
}
