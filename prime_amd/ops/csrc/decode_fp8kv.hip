// fp8 (OCP e4m3fn) KV cache for the ragged batched decode path on gfx950.
//
// Cache format, per (sequence, row, kv head) vector x of D bf16 values:
//   m = max(max|x|, 1e-12), s = 448 / m, sinv = m / 448 (fp32 quotients),
//   byte = e4m3_rne(clamp(x * s, -448, 448)); value = float(byte) * sinv.
// k, v: bytes [B,Smax,Hkv,D]; k_scale, v_scale: fp32 sinv [B,Smax,Hkv]. The
// same convention as rowwise_quant_fp8_kernel (quant_fp8.hip) with a head
// row as the row, so an appended token never re-quantises older rows.
//
// Three entry points:
//  - prime_decode_qkv_append_fp8: decode_qkv_append_kernel's work split (a
//    head row is covered by D/8 consecutive threads, an aligned sub-group of
//    one wave that takes the same branches), q rotated to bf16 as there, k
//    rotated and rounded to bf16 then quantised, v quantised. The row amax
//    is a shuffle reduction inside the sub-group.
//  - prime_kv_store_fp8: prefill store of k, v [B,S,Hkv,D] into rows
//    [pos, pos+S) of a cache [B',Smax,Hkv,D] (D/4 lanes x 8 B per row).
//  - prime_attn_decode_ragged_fp8: attn_decode_ragged_kernel's grid, lens
//    clamp, idle / empty-split rule, workspace layout and index-order merge
//    (decode_ragged.hip), streaming 1-byte elements: K rows in 16 B loads
//    with the score scaled by k_scale[row], P * v_scale[row] into LDS, V rows
//    coalesced at 8 B per lane with no scale handling.
// The e4m3 decode is the gfx950 conversion instruction, which is OCP (not
// fnuz) on this target.
#include "common.h"
#include <hip/hip_fp8.h>

#define DF_CHUNK 256    // keys per online-softmax chunk (= DR_CHUNK)
#define DF_THREADS 256

typedef __attribute__((ext_vector_type(2))) float df_float2;

struct alignas(16) u32x4 { unsigned v[4]; };
struct alignas(8) u32x2 { unsigned v[2]; };

// max over an aligned group of W consecutive lanes (W a power of two <= 64)
template <int W>
__device__ __forceinline__ float group_max(float x) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1)
    x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}

// four e4m3 bytes of clamp(x * s), element j in byte j
__device__ __forceinline__ unsigned quant4_e4m3(const float* x, float s) {
  unsigned w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float q = fminf(fmaxf(x[j] * s, -448.f), 448.f);
    w |= (unsigned)__hip_fp8_e4m3(q).__x << (8 * j);
  }
  return w;
}

// four e4m3 bytes of one dword -> fp32
__device__ __forceinline__ void dec4_e4m3(unsigned w, float* f) {
  const df_float2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const df_float2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo.x; f[1] = lo.y; f[2] = hi.x; f[3] = hi.y;
}

// ------------------------------------------------------------ decode append
template <int D>
__global__ __launch_bounds__(256) void decode_qkv_append_fp8_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ qout,
    unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
    float* __restrict__ ksc, float* __restrict__ vsc,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos, int64_t nrows, int H, int Hkv, int Smax,
    int T, float sign) {
  constexpr int half = D / 2;
  constexpr int hv = half / 4;  // threads per head row: 8 or 16
  const int NH = H + 2 * Hkv;
  const int lim = min(Smax, T);
  const int64_t total = nrows * hv;  // a multiple of hv: groups stay whole
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / hv;  // (b, head of the packed row)
    const int i4 = (int)(idx - row * hv) * 4;
    const int64_t b = row / NH;
    const int hh = (int)(row - b * NH);
    const int p = pos[b];
    const bool live = p >= 0 && p < lim;
    const bool isq = hh < H;
    const bool rot = hh < H + Hkv;
    bf16x4 y1, y2;
#pragma unroll
    for (int j = 0; j < 4; ++j) y1.v[j] = y2.v[j] = f2bf(0.f);
    if (live) {
      const bf16* xr = qkv + row * D;
      y1 = *reinterpret_cast<const bf16x4*>(xr + i4);
      y2 = *reinterpret_cast<const bf16x4*>(xr + half + i4);
      if (rot) {
        const bf16x4 x1 = y1, x2 = y2;
        const f32x4v c =
            *reinterpret_cast<const f32x4v*>(cos_t + (int64_t)p * half + i4);
        const f32x4v sn =
            *reinterpret_cast<const f32x4v*>(sin_t + (int64_t)p * half + i4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          rope_rot(x1.v[j], x2.v[j], c.v[j], sn.v[j], sign, y1.v[j], y2.v[j]);
      }
    }
    // row amax over the hv threads of this head row; every lane of the
    // group is here (same row, same trip count), q rows just discard it
    float f1[4], f2[4];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f1[j] = bf2f(y1.v[j]);
      f2[j] = bf2f(y2.v[j]);
      am = fmaxf(am, fmaxf(fabsf(f1[j]), fabsf(f2[j])));
    }
    am = group_max<hv>(am);
    if (isq) {  // idle slot: zeros
      bf16* dst = qout + (b * H + hh) * D;
      *reinterpret_cast<bf16x4*>(dst + i4) = y1;
      *reinterpret_cast<bf16x4*>(dst + half + i4) = y2;
    } else if (live) {
      const int hk = hh - H;
      const bool isk = hk < Hkv;
      const int64_t orow =
          (b * Smax + p) * Hkv + (isk ? hk : hk - Hkv);
      unsigned char* dst = (isk ? kc : vc) + orow * D;
      const float m = fmaxf(am, 1e-12f);
      const float s = 448.f / m;
      *reinterpret_cast<unsigned*>(dst + i4) = quant4_e4m3(f1, s);
      *reinterpret_cast<unsigned*>(dst + half + i4) = quant4_e4m3(f2, s);
      if (i4 == 0) (isk ? ksc : vsc)[orow] = m / 448.f;
    }
  }
}

PRIME_API int prime_decode_qkv_append_fp8(
    hipStream_t stream, const void* qkv, void* qout, void* kc, void* vc,
    void* k_scale, void* v_scale, const void* cos_t, const void* sin_t,
    const void* pos, int64_t B, int64_t H, int64_t Hkv, int64_t D,
    int64_t Smax, int64_t T) {
  if ((D != 64 && D != 128) || B < 1 || H < 1 || Hkv < 1 || Smax < 1 ||
      T < 1 || Smax > 0x7fffffff || T > 0x7fffffff || !pos || !k_scale ||
      !v_scale)
    return hipErrorInvalidValue;
  const int64_t nrows = B * (H + 2 * Hkv);
  const int grid = prime_grid(nrows * (D / 8), 256);
  if (D == 128)
    hipLaunchKernelGGL((decode_qkv_append_fp8_kernel<128>), dim3(grid),
                       dim3(256), 0, stream, (const bf16*)qkv, (bf16*)qout,
                       (unsigned char*)kc, (unsigned char*)vc, (float*)k_scale,
                       (float*)v_scale, (const float*)cos_t,
                       (const float*)sin_t, (const int*)pos, nrows, (int)H,
                       (int)Hkv, (int)Smax, (int)T, 1.f);
  else
    hipLaunchKernelGGL((decode_qkv_append_fp8_kernel<64>), dim3(grid),
                       dim3(256), 0, stream, (const bf16*)qkv, (bf16*)qout,
                       (unsigned char*)kc, (unsigned char*)vc, (float*)k_scale,
                       (float*)v_scale, (const float*)cos_t,
                       (const float*)sin_t, (const int*)pos, nrows, (int)H,
                       (int)Hkv, (int)Smax, (int)T, 1.f);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ prefill store
// idx -> (tensor k/v, input row, lane of the row); LPR = D/4 lanes per row.
template <int D>
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
    float* __restrict__ ksc, float* __restrict__ vsc, int64_t nrows, int S,
    int Hkv, int Smax, int pos) {
  constexpr int LPR = D / 4;  // 16 or 32: an aligned sub-group of a wave
  const int64_t total = 2 * nrows * LPR;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r2 = idx / LPR;
    const int d4 = (int)(idx - r2 * LPR) * 4;
    const bool isk = r2 < nrows;
    const int64_t r = isk ? r2 : r2 - nrows;  // (b * S + s) * Hkv + h
    const int64_t bs = r / Hkv;
    const int h = (int)(r - bs * Hkv);
    const int64_t b = bs / S;
    const int s_ = (int)(bs - b * S);
    const bf16x4 x4 =
        *reinterpret_cast<const bf16x4*>((isk ? k : v) + r * D + d4);
    float f[4];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = bf2f(x4.v[j]);
      am = fmaxf(am, fabsf(f[j]));
    }
    am = group_max<LPR>(am);
    const float m = fmaxf(am, 1e-12f);
    const int64_t orow = (b * Smax + pos + s_) * Hkv + h;
    *reinterpret_cast<unsigned*>((isk ? kc : vc) + orow * D + d4) =
        quant4_e4m3(f, 448.f / m);
    if (d4 == 0) (isk ? ksc : vsc)[orow] = m / 448.f;
  }
}

// k, v: bf16 [B,S,Hkv,D] contiguous -> rows [pos, pos+S) of the first B
// slots of a cache [B',Smax,Hkv,D], B <= B' (the caller's responsibility:
// the batch stride comes from Smax).
PRIME_API int prime_kv_store_fp8(hipStream_t stream, const void* k,
                                 const void* v, void* kc, void* vc,
                                 void* k_scale, void* v_scale, int64_t B,
                                 int64_t S, int64_t Hkv, int64_t D,
                                 int64_t Smax, int64_t pos) {
  if ((D != 64 && D != 128) || B < 1 || S < 1 || Hkv < 1 || Smax < 1 ||
      Smax > 0x7fffffff || pos < 0 || S > Smax || pos > Smax - S)
    return hipErrorInvalidValue;
  const int64_t nrows = B * S * Hkv;
  const int grid = prime_grid(2 * nrows * (D / 4), 256);
  if (D == 128)
    hipLaunchKernelGGL((kv_store_fp8_kernel<128>), dim3(grid), dim3(256), 0,
                       stream, (const bf16*)k, (const bf16*)v,
                       (unsigned char*)kc, (unsigned char*)vc, (float*)k_scale,
                       (float*)v_scale, nrows, (int)S, (int)Hkv, (int)Smax,
                       (int)pos);
  else
    hipLaunchKernelGGL((kv_store_fp8_kernel<64>), dim3(grid), dim3(256), 0,
                       stream, (const bf16*)k, (const bf16*)v,
                       (unsigned char*)kc, (unsigned char*)vc, (float*)k_scale,
                       (float*)v_scale, nrows, (int)S, (int)Hkv, (int)Smax,
                       (int)pos);
  return (int)hipGetLastError();
}

// --------------------------------------------------------- decode attention
template <int D, int G>
__global__ __launch_bounds__(DF_THREADS) void attn_decode_ragged_fp8_kernel(
    const bf16* __restrict__ Q, const unsigned char* __restrict__ K,
    const unsigned char* __restrict__ V, const float* __restrict__ Ks,
    const float* __restrict__ Vs, float* __restrict__ ws,
    const int* __restrict__ lens, int H, int Hkv, int Smax, int split_rows,
    float scale) {
  constexpr int PART = G * (D + 2);  // floats per (b, kv head, split)
  constexpr int LPR = D / 8;         // lanes per V row (8 B = 8 elements each)
  constexpr int RG = DF_THREADS / LPR;  // V rows per step
  constexpr int NW = DF_THREADS / 64;
  // Unroll depths (VGPR counts and the measured alternatives are in
  // profiles/decode_fp8kv.md): a 16 B K load is 16 elements that decode to
  // 16 fp32 values, and the accumulators are G x 8 floats (G x 4 in the
  // bf16 kernel), so the depths are at most half the bf16 kernel's. G <= 4
  // stays at or under 128 VGPRs (4 waves/SIMD, the bf16 kernel's
  // occupancy); for G = 4 that allows half a row of K in flight, which
  // measured best at the full-machine shape, and a whole row (232-256
  // VGPRs) measured 1.7x slower. G = 8 needs 174 at any depth (2 waves/SIMD).
  constexpr int KU = G >= 8 ? 1 : (G >= 4 ? D / 32 : (G >= 2 ? 2 : 4));  // K loads in flight
  constexpr int VU = G >= 8 ? 2 : (G >= 2 ? 4 : 8);  // V row steps in flight
  const int bk = blockIdx.x;
  const int b = bk / Hkv, hkv = bk - b * Hkv;
  const int sp = blockIdx.y, nsplit = gridDim.y;
  const int t = threadIdx.x;
  const int lane = t & 63, wid = t >> 6;
  const int L = min(max(lens[b], 0), Smax);
  const int r0 = sp * split_rows;
  const int r1 = min(r0 + split_rows, L);
  float* wsp = ws + ((int64_t)bk * nsplit + sp) * PART;

  if (r0 >= r1) {  // block-uniform: empty split (or idle slot)
    for (int i = t; i < PART; i += DF_THREADS)
      wsp[i] = (i >= G * D && i < G * D + G) ? -1e30f : 0.f;
    return;
  }

  __shared__ float q_lds[G * D];
  __shared__ float p_lds[G][DF_CHUNK];
  __shared__ float red_m[NW][G];
  __shared__ float red_s[NW][G];
  __shared__ __attribute__((aligned(16))) float part[RG * D];

  const int64_t row_stride = (int64_t)Hkv * D;  // bytes = elements
  const bf16* qp = Q + ((int64_t)b * H + (int64_t)hkv * G) * D;
  const unsigned char* Kb = K + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const unsigned char* Vb = V + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const float* Ksb = Ks + (int64_t)b * Smax * Hkv + hkv;
  const float* Vsb = Vs + (int64_t)b * Smax * Hkv + hkv;

  for (int i = t; i < G * D; i += DF_THREADS) q_lds[i] = bf2f(qp[i]);
  __syncthreads();

  float m[G], lsum[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -1e30f;
    lsum[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
  }
  const int vr = t / LPR, vd = (t - vr * LPR) * 8;

  for (int c0 = r0; c0 < r1; c0 += DF_CHUNK) {
    const int cn = min(DF_CHUNK, r1 - c0);
    // ---- scores: key c0 + t against the G queries
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = -1e30f;
    float vsc = 0.f;  // dequant factor of V row c0 + t, folded into P
    if (t < cn) {
      const int64_t row = c0 + t;
      const u32x4* kr = reinterpret_cast<const u32x4*>(Kb + row * row_stride);
      const float ksc = Ksb[row * Hkv];
      vsc = Vsb[row * Hkv];
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; ++g) dot[g] = 0.f;
#pragma unroll KU
      for (int j = 0; j < D / 16; ++j) {
        const u32x4 k16 = kr[j];
        float kf[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) dec4_e4m3(k16.v[u], kf + 4 * u);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < 16; ++u)
            dot[g] += q_lds[g * D + j * 16 + u] * kf[u];
      }
      const float sc = ksc * scale;
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = dot[g] * sc;
    }
    // ---- chunk max of each head (all lanes get the wave result)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float x = s[g];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
      if (lane == 0) red_m[wid][g] = x;
    }
    __syncthreads();
    float alpha[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = red_m[0][g];
#pragma unroll
      for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red_m[w][g]);
      const float mnew = fmaxf(m[g], mx);
      alpha[g] = __expf(m[g] - mnew);
      m[g] = mnew;
      const float p = (t < cn) ? __expf(s[g] - mnew) : 0.f;
      // the V phase needs no scale: the row's factor rides on its weight
      p_lds[g][t] = (t < cn) ? p * vsc : 0.f;
      float x = p;  // the running sum keeps the unscaled weight
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
      if (lane == 0) red_s[wid][g] = x;
    }
    __syncthreads();  // p_lds and red_s ready
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float ps = red_s[0][g];
#pragma unroll
      for (int w = 1; w < NW; ++w) ps += red_s[w][g];
      lsum[g] = lsum[g] * alpha[g] + ps;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] *= alpha[g];
    }
    // ---- V rows, coalesced: LPR lanes cover one row, RG rows per step and
    // VU steps of loads issued before their FMAs. A step past the chunk
    // re-reads the chunk's last live row with weight 0, so no row (or
    // scale) at or beyond the length is ever touched.
    for (int l0 = vr; l0 < cn; l0 += RG * VU) {
      u32x2 v8[VU];
#pragma unroll
      for (int k = 0; k < VU; ++k) {
        const int lc = min(l0 + k * RG, cn - 1);
        v8[k] = *reinterpret_cast<const u32x2*>(
            Vb + (int64_t)(c0 + lc) * row_stride + vd);
      }
#pragma unroll
      for (int k = 0; k < VU; ++k) {
        const int l = l0 + k * RG;
        const int lc = min(l, cn - 1);
        float vf[8];
        dec4_e4m3(v8[k].v[0], vf);
        dec4_e4m3(v8[k].v[1], vf + 4);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = (l < cn) ? p_lds[g][lc] : 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[g][j] += p * vf[j];
        }
      }
    }
    __syncthreads();  // p_lds / red_* reused by the next chunk
  }

  // ---- combine the RG row groups in a fixed order, one head at a time
#pragma unroll
  for (int g = 0; g < G; ++g) {
    f32x4v a0, a1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a0.v[j] = acc[g][j];
      a1.v[j] = acc[g][4 + j];
    }
    *reinterpret_cast<f32x4v*>(&part[vr * D + vd]) = a0;
    *reinterpret_cast<f32x4v*>(&part[vr * D + vd + 4]) = a1;
    __syncthreads();
    if (t < D) {
      float o = part[t];
#pragma unroll
      for (int r = 1; r < RG; ++r) o += part[r * D + t];
      wsp[g * D + t] = o;
    }
    if (t == 0) {
      wsp[G * D + g] = m[g];
      wsp[G * D + G + g] = lsum[g];
    }
    __syncthreads();
  }
}

// This file's copy of attn_decode_merge_kernel (decode_ragged.hip): the
// library is one non-RDC compile, so a kernel of another file cannot be
// launched from here. Splits are combined in index order.
__global__ void attn_decode_merge_fp8_kernel(const float* __restrict__ ws,
                                             bf16* __restrict__ O, int H,
                                             int Hkv, int D, int nsplit) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh - b * H;
  const int G = H / Hkv;
  const int hkv = h / G, g = h - hkv * G;
  const int d = threadIdx.x;
  const int part = G * (D + 2);
  const float* base = ws + ((int64_t)b * Hkv + hkv) * nsplit * part;
  float M = -1e30f;
  for (int s = 0; s < nsplit; ++s)
    M = fmaxf(M, base[(int64_t)s * part + G * D + g]);
  float num = 0.f, den = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* ps = base + (int64_t)s * part;
    const float w = __expf(ps[G * D + g] - M);
    den += w * ps[G * D + G + g];
    num += w * ps[g * D + d];
  }
  // every split empty (idle slot): num = den = 0 -> exactly zero
  O[((int64_t)b * H + h) * D + d] = f2bf(num / fmaxf(den, 1e-30f));
}

template <int D, int G>
static void launch_ragged_fp8(hipStream_t stream, const void* Q, const void* K,
                              const void* V, const void* Ks, const void* Vs,
                              void* ws, const void* lens, int B, int H,
                              int Hkv, int Smax, int split_rows, int nsplit,
                              float scale) {
  hipLaunchKernelGGL((attn_decode_ragged_fp8_kernel<D, G>),
                     dim3(B * Hkv, nsplit), dim3(DF_THREADS), 0, stream,
                     (const bf16*)Q, (const unsigned char*)K,
                     (const unsigned char*)V, (const float*)Ks,
                     (const float*)Vs, (float*)ws, (const int*)lens, H, Hkv,
                     Smax, split_rows, scale);
}

template <int D>
static int launch_ragged_fp8_g(int G, hipStream_t stream, const void* Q,
                               const void* K, const void* V, const void* Ks,
                               const void* Vs, void* ws, const void* lens,
                               int B, int H, int Hkv, int Smax, int split_rows,
                               int nsplit, float scale) {
  switch (G) {
    case 1: launch_ragged_fp8<D, 1>(stream, Q, K, V, Ks, Vs, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    case 2: launch_ragged_fp8<D, 2>(stream, Q, K, V, Ks, Vs, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    case 4: launch_ragged_fp8<D, 4>(stream, Q, K, V, Ks, Vs, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    case 8: launch_ragged_fp8<D, 8>(stream, Q, K, V, Ks, Vs, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    default: return hipErrorInvalidValue;
  }
  return hipSuccess;
}

// Same contract as prime_attn_decode_ragged (ws layout, split_rows a
// positive multiple of the chunk chosen from the launch shape only), with
// the cache as e4m3 bytes K/V [B,Smax,Hkv,D] + fp32 k_scale/v_scale
// [B,Smax,Hkv].
PRIME_API int prime_attn_decode_ragged_fp8(
    hipStream_t stream, const void* Q, const void* K, const void* V,
    const void* k_scale, const void* v_scale, void* O, void* ws,
    const void* lens, int64_t B, int64_t H, int64_t Hkv, int64_t Smax,
    int64_t D, int64_t split_rows, double scale) {
  if ((D != 64 && D != 128) || B < 1 || H < 1 || Hkv < 1 || Smax < 1 ||
      H % Hkv != 0 || split_rows < DF_CHUNK || split_rows % DF_CHUNK != 0 ||
      !ws || !lens || !k_scale || !v_scale)
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  if (nsplit > 65535 || B * Hkv > 0x7fffffff || B * H > 0x7fffffff ||
      Smax > 0x7fffffff - split_rows)
    return hipErrorInvalidValue;
  int rc;
  if (D == 128)
    rc = launch_ragged_fp8_g<128>((int)G, stream, Q, K, V, k_scale, v_scale,
                                  ws, lens, (int)B, (int)H, (int)Hkv,
                                  (int)Smax, (int)split_rows, (int)nsplit,
                                  (float)scale);
  else
    rc = launch_ragged_fp8_g<64>((int)G, stream, Q, K, V, k_scale, v_scale, ws,
                                 lens, (int)B, (int)H, (int)Hkv, (int)Smax,
                                 (int)split_rows, (int)nsplit, (float)scale);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(attn_decode_merge_fp8_kernel, dim3((int)(B * H)),
                     dim3((int)D), 0, stream, (const float*)ws, (bf16*)O,
                     (int)H, (int)Hkv, (int)D, (int)nsplit);
  return (int)hipGetLastError();
}
