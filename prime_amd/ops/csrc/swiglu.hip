// SwiGLU activation for gfx950: out = silu(gate) * up, with gate/up packed
// as one [R, 2I] tensor (gate = [:, :I], up = [:, I:]) so the preceding
// hipBLASLt GEMM produces both halves in one call.
//
// Memory-bound; bf16x8 vectorized; backward recomputes silu from the saved
// input (no extra activation storage).
#include "common.h"

__device__ __forceinline__ float sigmoidf_(float x) {
  return 1.f / (1.f + __expf(-x));
}

__global__ void swiglu_fwd_kernel(const bf16* __restrict__ gu,
                                  bf16* __restrict__ out, int64_t R, int I) {
  const int iv = I / 8;
  const int64_t total = R * iv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx / iv;
    const int i = (int)(idx - r * iv) * 8;
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(gu + r * 2 * I + i);
    const bf16x8 u = *reinterpret_cast<const bf16x8*>(gu + r * 2 * I + I + i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gf = bf2f(g.v[j]);
      o.v[j] = f2bf(gf * sigmoidf_(gf) * bf2f(u.v[j]));
    }
    *reinterpret_cast<bf16x8*>(out + r * I + i) = o;
  }
}

// Backward element math, shared by swiglu_bwd_kernel and the fused
// dgu + dgu^T kernel below so both produce bit-identical values.
__device__ __forceinline__ void swiglu_bwd8(const bf16x8& g, const bf16x8& u,
                                            const bf16x8& d, bf16x8& dg,
                                            bf16x8& du) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gf = bf2f(g.v[j]);
    const float sg = sigmoidf_(gf);
    const float silu = gf * sg;
    const float df = bf2f(d.v[j]);
    dg.v[j] = f2bf(df * bf2f(u.v[j]) * sg * (1.f + gf * (1.f - sg)));
    du.v[j] = f2bf(df * silu);
  }
}

__global__ void swiglu_bwd_kernel(const bf16* __restrict__ dout,
                                  const bf16* __restrict__ gu,
                                  bf16* __restrict__ dgu, int64_t R, int I) {
  const int iv = I / 8;
  const int64_t total = R * iv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx / iv;
    const int i = (int)(idx - r * iv) * 8;
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(gu + r * 2 * I + i);
    const bf16x8 u = *reinterpret_cast<const bf16x8*>(gu + r * 2 * I + I + i);
    const bf16x8 d = *reinterpret_cast<const bf16x8*>(dout + r * I + i);
    bf16x8 dg, du;
    swiglu_bwd8(g, u, d, dg, du);
    *reinterpret_cast<bf16x8*>(dgu + r * 2 * I + i) = dg;
    *reinterpret_cast<bf16x8*>(dgu + r * 2 * I + I + i) = du;
  }
}

PRIME_API int prime_swiglu_fwd(hipStream_t stream, const void* gu, void* out,
                               int64_t R, int64_t I) {
  if (I % 8 != 0) return hipErrorInvalidValue;
  int grid = prime_grid(R * (I / 8), 256);
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)gu, (bf16*)out, R, (int)I);
  return (int)hipGetLastError();
}

PRIME_API int prime_swiglu_bwd(hipStream_t stream, const void* dout,
                               const void* gu, void* dgu, int64_t R, int64_t I) {
  if (I % 8 != 0) return hipErrorInvalidValue;
  int grid = prime_grid(R * (I / 8), 256);
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)dout, (const bf16*)gu, (bf16*)dgu, R, (int)I);
  return (int)hipGetLastError();
}

// swiglu backward that also emits dgu^T [2I, R]: the gate/up dW GEMM runs
// as NN against dY^T, and re-reading dgu just to transpose it costs a full
// extra pass over the largest activation gradient. One block per 64-row x
// 64-column tile of I; dg/du go out row-major straight from registers and
// transposed through two padded LDS tiles (same scheme as
// transpose_bshd_kernel: 16 B loads and stores in both phases).
#define SWT_TP 72  // padded LDS row: 64 + 8 elems

__global__ __launch_bounds__(256) void swiglu_bwd_t_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ gu,
    bf16* __restrict__ dgu, bf16* __restrict__ dgut, int64_t R, int I) {
  __shared__ bf16 tg[64][SWT_TP];
  __shared__ bf16 tu[64][SWT_TP];
  const int n_ct = I / 64;
  const int ct = blockIdx.x % n_ct;
  const int64_t rt = blockIdx.x / n_ct;
  const int64_t r0 = rt * 64;
  const int c0 = ct * 64;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int un = i * 256 + t;
    const int r = un >> 3, c8 = (un & 7) * 8;
    const int64_t row = r0 + r;
    const bf16x8 g =
        *reinterpret_cast<const bf16x8*>(gu + row * 2 * I + c0 + c8);
    const bf16x8 u =
        *reinterpret_cast<const bf16x8*>(gu + row * 2 * I + I + c0 + c8);
    const bf16x8 d = *reinterpret_cast<const bf16x8*>(dout + row * I + c0 + c8);
    bf16x8 dg, du;
    swiglu_bwd8(g, u, d, dg, du);
    *reinterpret_cast<bf16x8*>(dgu + row * 2 * I + c0 + c8) = dg;
    *reinterpret_cast<bf16x8*>(dgu + row * 2 * I + I + c0 + c8) = du;
    *reinterpret_cast<bf16x8*>(&tg[r][c8]) = dg;
    *reinterpret_cast<bf16x8*>(&tu[r][c8]) = du;
  }
  __syncthreads();
  // transposed store: dgut row = column of I (gate rows, then up rows at
  // +I), dgut cols = the tile's 64 rows
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int un = i * 256 + t;
    const int c = un >> 3, s8 = (un & 7) * 8;
    bf16x8 vg, vu;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      vg.v[j] = tg[s8 + j][c];
      vu.v[j] = tu[s8 + j][c];
    }
    *reinterpret_cast<bf16x8*>(dgut + (int64_t)(c0 + c) * R + r0 + s8) = vg;
    *reinterpret_cast<bf16x8*>(dgut + (int64_t)(I + c0 + c) * R + r0 + s8) = vu;
  }
}

PRIME_API int prime_swiglu_bwd_t(hipStream_t stream, const void* dout,
                                 const void* gu, void* dgu, void* dgut,
                                 int64_t R, int64_t I) {
  if (R <= 0 || I <= 0 || R % 64 != 0 || I % 64 != 0)
    return hipErrorInvalidValue;
  const int64_t grid = (R / 64) * (I / 64);
  if (grid > 0x7fffffff || I > 0x3fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swiglu_bwd_t_kernel, dim3((int)grid), dim3(256), 0,
                     stream, (const bf16*)dout, (const bf16*)gu, (bf16*)dgu,
                     (bf16*)dgut, R, (int)I);
  return (int)hipGetLastError();
}
