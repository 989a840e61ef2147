// Ragged single-token decode attention for gfx950 (batched serving path)
// over the contiguous bf16 cache: the contract, the split kernel's body and
// the merge are in decode_ragged_common.h; this file is the contiguous row
// policy, its __global__ wrapper and the entry point.
//
// Q [B,H,D], K/V cache [B,Smax,Hkv,D], O [B,H,D], ws fp32
// [B*Hkv, nsplit, G*(D+2)]. D in {64,128}, G in {1,2,4,8}.
#include "decode_ragged_common.h"

// Row rc of chunk c0 of sequence b is cache row c0 + rc of slab b.
struct DrContiguous {
  const bf16 *Kb, *Vb;
  int Smax;
  int64_t row_stride;
  int c0;
  __device__ __forceinline__ void open(int b, int64_t col, int64_t stride, int,
                                       int) {
    row_stride = stride;
    Kb += (int64_t)b * Smax * row_stride + col;
    Vb += (int64_t)b * Smax * row_stride + col;
  }
  __device__ __forceinline__ void begin_chunk(int c, int) { c0 = c; }
  __device__ __forceinline__ int64_t off(int rc) const {
    return (int64_t)(c0 + rc) * row_stride;
  }
  __device__ __forceinline__ void end_chunk() {}
};

template <int D, int G>
__global__ __launch_bounds__(DR_THREADS) void attn_decode_ragged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, float* __restrict__ ws,
    const int* __restrict__ lens, int H, int Hkv, int Smax, int split_rows,
    float scale) {
  dr_body<D, G>(Q, ws, lens, H, Hkv, Smax, split_rows, scale,
                DrContiguous{K, V, Smax, 0, 0});
}

// Chunk length of the online softmax (ops.DECODE_RAGGED_CHUNK mirrors it).
PRIME_API int prime_decode_ragged_chunk(void) { return DR_CHUNK; }

// ws, split_rows: see dr_check_args.
PRIME_API int prime_attn_decode_ragged(hipStream_t stream, const void* Q,
                                       const void* K, const void* V, void* O,
                                       void* ws, const void* lens, int64_t B,
                                       int64_t H, int64_t Hkv, int64_t Smax,
                                       int64_t D, int64_t split_rows,
                                       double scale) {
  if (dr_check_args(B, H, Hkv, Smax, D, split_rows, ws, lens))
    return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  dr_dispatch(D, H / Hkv, [&](auto d, auto g) {
    hipLaunchKernelGGL((attn_decode_ragged_kernel<d(), g()>),
                       dim3((int)(B * Hkv), (int)nsplit), dim3(DR_THREADS), 0,
                       stream, (const bf16*)Q, (const bf16*)K, (const bf16*)V,
                       (float*)ws, (const int*)lens, (int)H, (int)Hkv,
                       (int)Smax, (int)split_rows, (float)scale);
  });
  return dr_launch_merge(stream, ws, O, B, H, Hkv, D, nsplit);
}
