// Fused residual-add + RMSNorm for gfx950.
//
//   fwd: s = x + res (new residual stream, written once)
//        y = s * rsqrt(mean(s^2)+eps) * w
//   bwd: ds = ds_res + rmsnorm_dx(dy)   (residual grad fused in)
//
// Replaces the {eager add kernel, separate norm} pair per block side:
// one fewer full read+write pass of the hidden stream per fusion site
// (memory-bound; bf16x8 vectorized like rmsnorm.hip).
//
// Two kernel families compute the same bits:
//   *_kernel       generic: any D % 8 == 0, grid-stride over a row's vectors
//   *_rows_kernel  D <= 8192: a thread keeps its NV = ceil(D/8/256) vectors
//                  of the row in registers, every operand is one 16-byte
//                  load, and the next row's loads are in flight while this
//                  row's reduction sits in its barriers.
// The per-element arithmetic lives in the nrm_* helpers below, with
// contraction off and every fused multiply-add spelled out, so both
// families round identically whatever the surrounding code looks like.
#include "common.h"

// ---- per-element arithmetic, shared by both kernel families -------------
// s element before rounding: one fp32 add (none without a residual)
__device__ __forceinline__ float nrm_add(float x, float r) {
#pragma clang fp contract(off)
  return x + r;
}
// sum of squares: ss = fma(f, f, ss)
__device__ __forceinline__ float nrm_sq_acc(float ss, float f) {
  return __builtin_fmaf(f, f, ss);
}
// y = (s * rstd) * w
__device__ __forceinline__ float nrm_y(float s, float rs, float w) {
#pragma clang fp contract(off)
  return s * rs * w;
}
// dot += ((dy * w) * s) * rstd: three products, then a plain add
__device__ __forceinline__ float nrm_dot_acc(float dot, float d, float w,
                                             float s, float rs) {
#pragma clang fp contract(off)
  return dot + d * w * s * rs;
}
// shat = s * rstd
__device__ __forceinline__ float nrm_shat(float s, float rs) {
#pragma clang fp contract(off)
  return s * rs;
}
// g = rstd * (dy*w - shat*mean_dot), the difference as fma(dy, w, -(shat*mean_dot))
__device__ __forceinline__ float nrm_g(float d, float w, float shat,
                                       float mean_dot, float rs) {
#pragma clang fp contract(off)
  const float t = shat * mean_dot;
  return rs * __builtin_fmaf(d, w, -t);
}
// dw += dy * shat, fused
__device__ __forceinline__ float nrm_dw_acc(float dw, float d, float shat) {
  return __builtin_fmaf(d, shat, dw);
}

// ------------------------------------------------------- generic kernels
__global__ void add_rmsnorm_fwd_kernel(const bf16* __restrict__ x,
                                       const bf16* __restrict__ res,
                                       const bf16* __restrict__ w,
                                       bf16* __restrict__ s_out,
                                       bf16* __restrict__ y,
                                       float* __restrict__ rstd, int64_t R,
                                       int D, float eps) {
  __shared__ float scratch[16];
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;
  const int dvec = D / 8;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + r * D);
    const bf16x8* rr = res ? reinterpret_cast<const bf16x8*>(res + r * D) : nullptr;
    bf16x8* sr = reinterpret_cast<bf16x8*>(s_out + r * D);
    float ss = 0.f;
    for (int i = tid; i < dvec; i += nthr) {
      bf16x8 v = xr[i], o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(v.v[j]);
        if (rr) f = nrm_add(f, bf2f(rr[i].v[j]));
        o.v[j] = f2bf(f);
        ss = nrm_sq_acc(ss, f);
      }
      sr[i] = o;
    }
    ss = block_reduce_sum(ss, scratch);
    const float rs = rsqrtf(ss / (float)D + eps);
    if (tid == 0) rstd[r] = rs;
    bf16x8* yr = reinterpret_cast<bf16x8*>(y + r * D);
    const bf16x8* wv = reinterpret_cast<const bf16x8*>(w);
    for (int i = tid; i < dvec; i += nthr) {
      bf16x8 v = sr[i], wj = wv[i], o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o.v[j] = f2bf(nrm_y(bf2f(v.v[j]), rs, bf2f(wj.v[j])));
      yr[i] = o;
    }
  }
}

// ds = ds_res + rstd*(dy*w - shat*mean(dy*w*shat)) ;
// dw_part[block, :] = sum over the block's rows of dy*shat (summed by the
// caller in a fixed order, see rmsnorm.hip)
__global__ void add_rmsnorm_bwd_kernel(const bf16* __restrict__ dy,
                                       const bf16* __restrict__ ds_res,
                                       const bf16* __restrict__ s,
                                       const bf16* __restrict__ w,
                                       const float* __restrict__ rstd,
                                       bf16* __restrict__ ds_out,
                                       float* __restrict__ dw_part, int64_t R,
                                       int D, float eps) {
  extern __shared__ float lds[];
  float* dw_loc = lds;
  float* scratch = lds + D;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;
  const int dvec = D / 8;
  for (int i = tid; i < D; i += nthr) dw_loc[i] = 0.f;
  __syncthreads();

  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const bf16x8* dyr = reinterpret_cast<const bf16x8*>(dy + r * D);
    const bf16x8* srr = reinterpret_cast<const bf16x8*>(s + r * D);
    const bf16x8* dres = ds_res ? reinterpret_cast<const bf16x8*>(ds_res + r * D) : nullptr;
    const bf16x8* wv = reinterpret_cast<const bf16x8*>(w);
    const float rs = rstd[r];
    float dot = 0.f;
    for (int i = tid; i < dvec; i += nthr) {
      bf16x8 d = dyr[i], sv = srr[i], wj = wv[i];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dot = nrm_dot_acc(dot, bf2f(d.v[j]), bf2f(wj.v[j]), bf2f(sv.v[j]), rs);
    }
    dot = block_reduce_sum(dot, scratch);
    const float mean_dot = dot / (float)D;
    bf16x8* dso = reinterpret_cast<bf16x8*>(ds_out + r * D);
    for (int i = tid; i < dvec; i += nthr) {
      bf16x8 d = dyr[i], sv = srr[i], wj = wv[i], o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float shat = nrm_shat(bf2f(sv.v[j]), rs);
        float g = nrm_g(bf2f(d.v[j]), bf2f(wj.v[j]), shat, mean_dot, rs);
        if (dres) g = nrm_add(g, bf2f(dres[i].v[j]));
        o.v[j] = f2bf(g);
        dw_loc[i * 8 + j] = nrm_dw_acc(dw_loc[i * 8 + j], bf2f(d.v[j]), shat);
      }
      dso[i] = o;
    }
    __syncthreads();
  }
  for (int i = tid; i < D; i += nthr)
    dw_part[(int64_t)blockIdx.x * D + i] = dw_loc[i];
}

// ------------------------------------------- row-in-registers kernels
// 256 threads per row; thread t owns vectors t, t+256, ... (the generic
// kernels' assignment at blockDim 256), NV of them. Only the last can lie
// beyond the row. Loads are not predicated: a thread without a last vector
// loads the row's last one and ignores it, so the loads stay straight-line
// code and the compiler's wait counts stay exact.
template <int NV>
__device__ __forceinline__ bool nrm_owns(int k, int tid, int dvec) {
  return k < NV - 1 || tid + k * 256 < dvec;
}

// Byte offsets of a thread's vectors inside a row, 32 bits each, so that
// every access is row base (scalar) + offset (one register).
template <int NV>
__device__ __forceinline__ void nrm_offsets(int tid, int dvec, unsigned (&off)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = tid + k * 256;
    off[k] = 16u * (unsigned)(k < NV - 1 ? i : min(i, dvec - 1));
  }
}

template <int NV>
__device__ __forceinline__ void nrm_load_row(const bf16* __restrict__ row,
                                             const unsigned (&off)[NV],
                                             bf16x8 (&v)[NV]) {
  const char* p = reinterpret_cast<const char*>(row);
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = *reinterpret_cast<const bf16x8*>(p + off[k]);
}

__device__ __forceinline__ void nrm_store(bf16* __restrict__ row, unsigned off,
                                          const bf16x8& v) {
  *reinterpret_cast<bf16x8*>(reinterpret_cast<char*>(row) + off) = v;
}

// An empty asm the value passes through. In the row loop it keeps w as the
// 4 registers per vector it was loaded into (otherwise the fp32 expansion of
// w is hoisted out of the loop and doubles them). In front of the loop it
// makes the first row's loads land there, so that the wait counts inside
// the loop are those of the steady state (next row's loads, then this
// row's stores) and not the stricter ones of the first trip.
__device__ __forceinline__ void nrm_pin(bf16x8& v) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 u = __builtin_bit_cast(u32x4, v);
  asm volatile("" : "+v"(u));
  v = __builtin_bit_cast(bf16x8, u);
}

// Waves per SIMD the register allocator is held to: up to two vectors per
// thread the whole grid is resident at once (forward 2048 blocks = 8 per
// CU, backward 1024 = 4 per CU), which a larger allocation would break
// into a full round and a tail.
#define NRM_FWD_WAVES(NV) ((NV) <= 2 ? 8 : 4)
#define NRM_BWD_WAVES(NV) ((NV) <= 2 ? 4 : 2)

template <int NV, bool HAS_RES>
__global__ __launch_bounds__(256, NRM_FWD_WAVES(NV)) void add_rmsnorm_fwd_rows_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ res,
    const bf16* __restrict__ w, bf16* __restrict__ s_out, bf16* __restrict__ y,
    float* __restrict__ rstd, int64_t R, int D, float eps) {
  __shared__ float scratch[16];
  const int tid = threadIdx.x;
  const int dvec = D / 8;
  unsigned off[NV];
  nrm_offsets<NV>(tid, dvec, off);
  bf16x8 wj[NV], xv[NV], rv[NV];
  nrm_load_row<NV>(w, off, wj);
  int64_t r = blockIdx.x;
  if (r < R) {
    nrm_load_row<NV>(x + r * D, off, xv);
    if (HAS_RES) nrm_load_row<NV>(res + r * D, off, rv);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      nrm_pin(xv[k]);
      if (HAS_RES) nrm_pin(rv[k]);
      nrm_pin(wj[k]);
    }
  }
  for (; r < R; r += gridDim.x) {
    bf16x8 sv[NV];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) nrm_pin(wj[k]);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      // straight-line: a thread without this vector computes on the copy
      // it loaded and keeps its sum
      const bool own = nrm_owns<NV>(k, tid, dvec);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(xv[k].v[j]);
        if (HAS_RES) f = nrm_add(f, bf2f(rv[k].v[j]));
        sv[k].v[j] = f2bf(f);
        const float acc = nrm_sq_acc(ss, f);
        ss = own ? acc : ss;
      }
    }
    // next row's operands leave now and land during the reduction
    const int64_t rn = r + gridDim.x;
    if (rn < R) {
      nrm_load_row<NV>(x + rn * D, off, xv);
      if (HAS_RES) nrm_load_row<NV>(res + rn * D, off, rv);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (nrm_owns<NV>(k, tid, dvec)) nrm_store(s_out + r * D, off[k], sv[k]);
    ss = block_reduce_sum(ss, scratch);
    const float rs = rsqrtf(ss / (float)D + eps);
    if (tid == 0) rstd[r] = rs;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o.v[j] = f2bf(nrm_y(bf2f(sv[k].v[j]), rs, bf2f(wj[k].v[j])));
      if (nrm_owns<NV>(k, tid, dvec)) nrm_store(y + r * D, off[k], o);
    }
  }
}

// The block's dw partial never leaves the owning thread's registers: a
// thread only ever adds into the columns of its own vectors, row after row
// in the generic kernel's order.
template <int NV, bool HAS_DRES>
__global__ __launch_bounds__(256, NRM_BWD_WAVES(NV)) void add_rmsnorm_bwd_rows_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ ds_res,
    const bf16* __restrict__ s, const bf16* __restrict__ w,
    const float* __restrict__ rstd, bf16* __restrict__ ds_out,
    float* __restrict__ dw_part, int64_t R, int D, float eps) {
  __shared__ float scratch[16];
  const int tid = threadIdx.x;
  const int dvec = D / 8;
  bf16x8 wj[NV], dv[NV], sv[NV], rv[NV];
  float dw[NV][8];
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) dw[k][j] = 0.f;
  unsigned off[NV];
  nrm_offsets<NV>(tid, dvec, off);
  nrm_load_row<NV>(w, off, wj);
  int64_t r = blockIdx.x;
  float rs = 0.f;
  if (r < R) {
    nrm_load_row<NV>(dy + r * D, off, dv);
    nrm_load_row<NV>(s + r * D, off, sv);
    if (HAS_DRES) nrm_load_row<NV>(ds_res + r * D, off, rv);
    rs = rstd[r];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      nrm_pin(dv[k]);
      nrm_pin(sv[k]);
      if (HAS_DRES) nrm_pin(rv[k]);
      nrm_pin(wj[k]);
    }
  }
  for (; r < R; r += gridDim.x) {
    // this row's operands move aside: the prefetch below reuses dv/sv/rv
    bf16x8 dk[NV], sk[NV], rk[NV];
    const float rsr = rs;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) nrm_pin(wj[k]);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const bool own = nrm_owns<NV>(k, tid, dvec);
      dk[k] = dv[k];
      sk[k] = sv[k];
      if (HAS_DRES) rk[k] = rv[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float acc = nrm_dot_acc(dot, bf2f(dk[k].v[j]), bf2f(wj[k].v[j]),
                                      bf2f(sk[k].v[j]), rsr);
        dot = own ? acc : dot;
      }
    }
    const int64_t rn = r + gridDim.x;
    if (rn < R) {
      nrm_load_row<NV>(dy + rn * D, off, dv);
      nrm_load_row<NV>(s + rn * D, off, sv);
      if (HAS_DRES) nrm_load_row<NV>(ds_res + rn * D, off, rv);
      rs = rstd[rn];
    }
    dot = block_reduce_sum(dot, scratch);
    const float mean_dot = dot / (float)D;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      // dw of a vector the thread does not own is never stored
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = bf2f(dk[k].v[j]);
        const float shat = nrm_shat(bf2f(sk[k].v[j]), rsr);
        float g = nrm_g(d, bf2f(wj[k].v[j]), shat, mean_dot, rsr);
        if (HAS_DRES) g = nrm_add(g, bf2f(rk[k].v[j]));
        o.v[j] = f2bf(g);
        dw[k][j] = nrm_dw_acc(dw[k][j], d, shat);
      }
      if (nrm_owns<NV>(k, tid, dvec)) nrm_store(ds_out + r * D, off[k], o);
    }
  }
  float* dwo = dw_part + (int64_t)blockIdx.x * D;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if (!nrm_owns<NV>(k, tid, dvec)) continue;
    f32x4v lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo.v[j] = dw[k][j]; hi.v[j] = dw[k][4 + j]; }
    f32x4v* p = reinterpret_cast<f32x4v*>(dwo + (int64_t)(tid + k * 256) * 8);
    p[0] = lo;
    p[1] = hi;
  }
}

// ------------------------------------------------------------ launchers
static int add_rmsnorm_fwd_generic(hipStream_t stream, const void* x,
                                   const void* res, const void* w, void* s_out,
                                   void* y, void* rstd, int64_t R, int64_t D,
                                   double eps) {
  if (D % 8 != 0) return hipErrorInvalidValue;
  int grid = prime_grid(R, 1);
  hipLaunchKernelGGL(add_rmsnorm_fwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)x, (const bf16*)res, (const bf16*)w,
                     (bf16*)s_out, (bf16*)y, (float*)rstd, R, (int)D,
                     (float)eps);
  return (int)hipGetLastError();
}

static int add_rmsnorm_bwd_generic(hipStream_t stream, const void* dy,
                                   const void* ds_res, const void* s,
                                   const void* w, const void* rstd,
                                   void* ds_out, void* dw_part, int64_t R,
                                   int64_t D, int64_t dw_rows, double eps) {
  if (D % 8 != 0) return hipErrorInvalidValue;
  if (dw_rows < 1 || dw_rows > 1024) return hipErrorInvalidValue;
  int grid = (int)dw_rows;
  size_t lds = (size_t)(D + 16) * sizeof(float);
  if (lds > 160 * 1024 - 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(add_rmsnorm_bwd_kernel, dim3(grid), dim3(256), lds,
                     stream, (const bf16*)dy, (const bf16*)ds_res,
                     (const bf16*)s, (const bf16*)w, (const float*)rstd,
                     (bf16*)ds_out, (float*)dw_part, R, (int)D, (float)eps);
  return (int)hipGetLastError();
}

// vectors per thread of the row kernels, 0: the generic kernels take it
static int nrm_rows_nv(int64_t D) {
  if (D < 8 || D % 8 != 0 || D > 8192) return 0;
  return (int)((D / 8 + 255) / 256);
}

PRIME_API int prime_add_rmsnorm_fwd_generic(hipStream_t stream, const void* x,
                                            const void* res, const void* w,
                                            void* s_out, void* y, void* rstd,
                                            int64_t R, int64_t D, double eps) {
  return add_rmsnorm_fwd_generic(stream, x, res, w, s_out, y, rstd, R, D, eps);
}

PRIME_API int prime_add_rmsnorm_bwd_generic(hipStream_t stream, const void* dy,
                                            const void* ds_res, const void* s,
                                            const void* w, const void* rstd,
                                            void* ds_out, void* dw_part,
                                            int64_t R, int64_t D,
                                            int64_t dw_rows, double eps) {
  return add_rmsnorm_bwd_generic(stream, dy, ds_res, s, w, rstd, ds_out,
                                 dw_part, R, D, dw_rows, eps);
}

PRIME_API int prime_add_rmsnorm_fwd(hipStream_t stream, const void* x,
                                    const void* res, const void* w, void* s_out,
                                    void* y, void* rstd, int64_t R, int64_t D,
                                    double eps) {
  const int nv = nrm_rows_nv(D);
  if (nv == 0)
    return add_rmsnorm_fwd_generic(stream, x, res, w, s_out, y, rstd, R, D, eps);
  const int grid = prime_grid(R, 1);
#define FWD_ROWS(NV, HAS)                                                     \
  hipLaunchKernelGGL((add_rmsnorm_fwd_rows_kernel<NV, HAS>), dim3(grid),      \
                     dim3(256), 0, stream, (const bf16*)x, (const bf16*)res,  \
                     (const bf16*)w, (bf16*)s_out, (bf16*)y, (float*)rstd, R, \
                     (int)D, (float)eps)
#define FWD_ROWS_NV(NV) do { if (res) FWD_ROWS(NV, true); else FWD_ROWS(NV, false); } while (0)
  switch (nv) {
    case 1: FWD_ROWS_NV(1); break;
    case 2: FWD_ROWS_NV(2); break;
    case 3: FWD_ROWS_NV(3); break;
    default: FWD_ROWS_NV(4); break;
  }
#undef FWD_ROWS_NV
#undef FWD_ROWS
  return (int)hipGetLastError();
}

PRIME_API int prime_add_rmsnorm_bwd(hipStream_t stream, const void* dy,
                                    const void* ds_res, const void* s,
                                    const void* w, const void* rstd,
                                    void* ds_out, void* dw_part, int64_t R,
                                    int64_t D, int64_t dw_rows, double eps) {
  const int nv = nrm_rows_nv(D);
  if (nv == 0)
    return add_rmsnorm_bwd_generic(stream, dy, ds_res, s, w, rstd, ds_out,
                                   dw_part, R, D, dw_rows, eps);
  if (dw_rows < 1 || dw_rows > 1024) return hipErrorInvalidValue;
  const int grid = (int)dw_rows;
#define BWD_ROWS(NV, HAS)                                                     \
  hipLaunchKernelGGL((add_rmsnorm_bwd_rows_kernel<NV, HAS>), dim3(grid),      \
                     dim3(256), 0, stream, (const bf16*)dy,                   \
                     (const bf16*)ds_res, (const bf16*)s, (const bf16*)w,     \
                     (const float*)rstd, (bf16*)ds_out, (float*)dw_part, R,   \
                     (int)D, (float)eps)
#define BWD_ROWS_NV(NV) do { if (ds_res) BWD_ROWS(NV, true); else BWD_ROWS(NV, false); } while (0)
  switch (nv) {
    case 1: BWD_ROWS_NV(1); break;
    case 2: BWD_ROWS_NV(2); break;
    case 3: BWD_ROWS_NV(3); break;
    default: BWD_ROWS_NV(4); break;
  }
#undef BWD_ROWS_NV
#undef BWD_ROWS
  return (int)hipGetLastError();
}
