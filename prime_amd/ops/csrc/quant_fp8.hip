// Fused bf16 -> OCP fp8 quantization for the fp8-forward mode: ONE pass
// reads x, writes e4m3 (or e5m2), accumulates the tensor's amax for the
// NEXT step (delayed scaling, TransformerEngine-style), and emits the
// dequant scale _scaled_mm needs — all from device scalars, no host
// round-trip. Replaces the 3-pass torch path (amax reduce + mul + cast):
// the activations quantized per 10B step total ~37 GB, so the saved
// passes are ~9 ms/step of HBM traffic in fp8 mode.
#include "common.h"
#include <hip/hip_fp8.h>

typedef __attribute__((ext_vector_type(8))) short q8_short8;

template <int E5M2>
__global__ __launch_bounds__(256) void quant_fp8_kernel(
    const bf16* __restrict__ x, unsigned char* __restrict__ y,
    const float* __restrict__ amax_prev, float* __restrict__ amax_next,
    float* __restrict__ sinv_out, int64_t n8) {
  // fp8 finite max: e4m3fn 448, e5m2 57344
  const float fmax8 = E5M2 ? 57344.f : 448.f;
  const float prev = fmaxf(*amax_prev, 1e-12f);
  const float s = fmax8 / prev;
  if (blockIdx.x == 0 && threadIdx.x == 0) sinv_out[0] = prev / fmax8;
  float amax = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n8;
       u += stride) {
    const q8_short8 raw = *reinterpret_cast<const q8_short8*>(x + u * 8);
    unsigned long long packed = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = bf2f(reinterpret_cast<const bf16*>(&raw)[j]);
      amax = fmaxf(amax, fabsf(v));
      const float q = fminf(fmaxf(v * s, -fmax8), fmax8);
      unsigned char b;
      if (E5M2) {
        b = __hip_fp8_e5m2(q).__x;
      } else {
        b = __hip_fp8_e4m3(q).__x;
      }
      packed |= (unsigned long long)b << (8 * j);
    }
    *reinterpret_cast<unsigned long long*>(y + u * 8) = packed;
  }
  amax = wave_reduce_max(amax);
  __shared__ float wmax[4];
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wmax[wid] = amax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = wmax[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) m = fmaxf(m, wmax[i]);
    // positive floats compare correctly as unsigned bit patterns
    atomicMax(reinterpret_cast<unsigned*>(amax_next),
              __float_as_uint(m));
  }
}

PRIME_API int prime_quant_fp8(hipStream_t stream, const void* x, void* y,
                              const void* amax_prev, void* amax_next,
                              void* sinv_out, int64_t n, int64_t e5m2) {
  if (n % 8) return hipErrorInvalidValue;
  const int grid = prime_grid(n / 8, 256);
  if (e5m2)
    hipLaunchKernelGGL((quant_fp8_kernel<1>), dim3(grid), dim3(256), 0,
                       stream, (const bf16*)x, (unsigned char*)y,
                       (const float*)amax_prev, (float*)amax_next,
                       (float*)sinv_out, n / 8);
  else
    hipLaunchKernelGGL((quant_fp8_kernel<0>), dim3(grid), dim3(256), 0,
                       stream, (const bf16*)x, (unsigned char*)y,
                       (const float*)amax_prev, (float*)amax_next,
                       (float*)sinv_out, n / 8);
  return (int)hipGetLastError();
}

// Rowwise variant: per-ROW amax + scale (no delayed-scaling state, no
// outlier saturation across tokens). One workgroup per row: pass 1 reads
// the row for its amax (coalesced), pass 2 re-reads (L2-hot — rows are
// 8-256 KB against 4 MiB per-XCD L2) and casts. Emits the per-row
// dequant scale vector torch._scaled_mm consumes as scale_a=[M,1] /
// scale_b=[1,N].
template <int E5M2>
__global__ __launch_bounds__(256) void rowwise_quant_fp8_kernel(
    const bf16* __restrict__ x, unsigned char* __restrict__ y,
    float* __restrict__ sinv_out, int64_t R, int64_t C8) {
  const float fmax8 = E5M2 ? 57344.f : 448.f;
  __shared__ float wmax[4];
  __shared__ float s_shared;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const bf16* row = x + r * C8 * 8;
    float amax = 0.f;
    for (int64_t u = threadIdx.x; u < C8; u += 256) {
      const q8_short8 raw = *reinterpret_cast<const q8_short8*>(row + u * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        amax = fmaxf(amax, fabsf(bf2f(reinterpret_cast<const bf16*>(&raw)[j])));
    }
    amax = wave_reduce_max(amax);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
      float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      m = fmaxf(m, 1e-12f);
      s_shared = fmax8 / m;
      sinv_out[r] = m / fmax8;
    }
    __syncthreads();
    const float s = s_shared;
    unsigned char* orow = y + r * C8 * 8;
    for (int64_t u = threadIdx.x; u < C8; u += 256) {
      const q8_short8 raw = *reinterpret_cast<const q8_short8*>(row + u * 8);
      unsigned long long packed = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float q = fminf(fmaxf(
            bf2f(reinterpret_cast<const bf16*>(&raw)[j]) * s, -fmax8), fmax8);
        const unsigned char b = E5M2 ? __hip_fp8_e5m2(q).__x
                                     : __hip_fp8_e4m3(q).__x;
        packed |= (unsigned long long)b << (8 * j);
      }
      *reinterpret_cast<unsigned long long*>(orow + u * 8) = packed;
    }
    __syncthreads();  // wmax/s_shared reused by the next row
  }
}

PRIME_API int prime_rowwise_quant_fp8(hipStream_t stream, const void* x,
                                      void* y, void* sinv_out, int64_t R,
                                      int64_t C, int64_t e5m2) {
  if (C % 8) return hipErrorInvalidValue;
  // no rows: one idle block, as every other op here (a grid of 0 is a
  // launch error)
  const int grid = prime_grid(R, 1);
  if (e5m2)
    hipLaunchKernelGGL((rowwise_quant_fp8_kernel<1>), dim3(grid), dim3(256),
                       0, stream, (const bf16*)x, (unsigned char*)y,
                       (float*)sinv_out, R, C / 8);
  else
    hipLaunchKernelGGL((rowwise_quant_fp8_kernel<0>), dim3(grid), dim3(256),
                       0, stream, (const bf16*)x, (unsigned char*)y,
                       (float*)sinv_out, R, C / 8);
  return (int)hipGetLastError();
}
