// Ragged single-token decode attention for gfx950 (batched serving path).
//
// Every sequence of the batch attends to its own number of cache rows:
// lens[b] is an int32 DEVICE vector read inside the kernel (a captured
// graph replays while the lengths change), clamped to [0, Smax] so no value
// can move an address out of the cache. lens[b] == 0 is an idle slot: its
// output row is exactly zero and none of its cache rows is read.
//
// Two kernels, no float atomics:
//  1. attn_decode_ragged_kernel, grid (B*Hkv, nsplit), 256 threads. One
//     workgroup serves all G = H/Hkv query heads of one (b, kv head), so a
//     K/V row is fetched once per kv head, and one fixed row range
//     [sp*split_rows, (sp+1)*split_rows) intersected with [0, lens[b]).
//     Flash-style online softmax over chunks of DR_CHUNK keys: thread t
//     owns key t of the chunk (16 B bf16x8 K reads against the G queries
//     held in LDS as fp32); V rows are read coalesced (D/4 lanes x 8 B per
//     row, 256/(D/4) rows per step, 8 steps in flight). The split writes fp32 partials
//     {o[G][D] unnormalised, m[G], l[G]} to the workspace; an empty split
//     writes neutral partials (o = 0, m = -1e30, l = 0) and reads no cache.
//  2. attn_decode_merge_kernel, grid B*H, D threads: combines the splits in
//     index order (bit-reproducible) and writes bf16.
//
// Q [B,H,D], K/V cache [B,Smax,Hkv,D], O [B,H,D], ws fp32
// [B*Hkv, nsplit, G*(D+2)]. D in {64,128}, G in {1,2,4,8}.
#include "common.h"

#define DR_CHUNK 256    // keys per online-softmax chunk (= block size)
#define DR_THREADS 256

template <int D, int G>
__global__ __launch_bounds__(DR_THREADS) void attn_decode_ragged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, float* __restrict__ ws,
    const int* __restrict__ lens, int H, int Hkv, int Smax, int split_rows,
    float scale) {
  constexpr int PART = G * (D + 2);  // floats per (b, kv head, split)
  constexpr int LPR = D / 4;         // lanes per V row (8 B each)
  constexpr int RG = DR_THREADS / LPR;  // V rows in flight
  constexpr int NW = DR_THREADS / 64;
  // K row chunks in flight per thread: fewer for big groups, whose G
  // accumulators and q operands would otherwise push the VGPR count up
  constexpr int KU = G >= 8 ? 2 : (G >= 4 ? 4 : D / 8);
  constexpr int VU = G >= 4 ? 4 : 8;  // V row steps in flight per thread
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
    for (int i = t; i < PART; i += DR_THREADS)
      wsp[i] = (i >= G * D && i < G * D + G) ? -1e30f : 0.f;
    return;
  }

  __shared__ float q_lds[G * D];
  __shared__ float p_lds[G][DR_CHUNK];
  __shared__ float red_m[NW][G];
  __shared__ float red_s[NW][G];
  __shared__ __attribute__((aligned(16))) float part[RG * D];

  const int64_t row_stride = (int64_t)Hkv * D;
  const bf16* qp = Q + ((int64_t)b * H + (int64_t)hkv * G) * D;
  const bf16* Kb = K + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const bf16* Vb = V + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;

  for (int i = t; i < G * D; i += DR_THREADS) q_lds[i] = bf2f(qp[i]);
  __syncthreads();

  float m[G], lsum[G], acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -1e30f;
    lsum[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[g][j] = 0.f;
  }
  const int vr = t / LPR, vd = (t - vr * LPR) * 4;

  for (int c0 = r0; c0 < r1; c0 += DR_CHUNK) {
    const int cn = min(DR_CHUNK, r1 - c0);
    // ---- scores: key c0 + t against the G queries
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = -1e30f;
    if (t < cn) {
      const bf16x8* kr =
          reinterpret_cast<const bf16x8*>(Kb + (int64_t)(c0 + t) * row_stride);
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; ++g) dot[g] = 0.f;
#pragma unroll KU
      for (int j = 0; j < D / 8; ++j) {
        const bf16x8 kv8 = kr[j];
        float kf[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) kf[u] = bf2f(kv8.v[u]);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < 8; ++u) dot[g] += q_lds[g * D + j * 8 + u] * kf[u];
      }
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = dot[g] * scale;
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
      p_lds[g][t] = p;
      float x = p;
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
      for (int j = 0; j < 4; ++j) acc[g][j] *= alpha[g];
    }
    // ---- V rows, coalesced: LPR lanes cover one row, RG rows per step and
    // VU steps of loads issued before their FMAs (a one-row-at-a-time loop
    // is a chain of dependent loads: latency-bound). A step past the chunk
    // re-reads the chunk's last live row with weight 0, so no row at or
    // beyond the length is ever touched.
    for (int l0 = vr; l0 < cn; l0 += RG * VU) {
      bf16x4 v4[VU];
#pragma unroll
      for (int k = 0; k < VU; ++k) {
        const int lc = min(l0 + k * RG, cn - 1);
        v4[k] = *reinterpret_cast<const bf16x4*>(
            Vb + (int64_t)(c0 + lc) * row_stride + vd);
      }
#pragma unroll
      for (int k = 0; k < VU; ++k) {
        const int l = l0 + k * RG;
        const int lc = min(l, cn - 1);
        float vf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vf[j] = bf2f(v4[k].v[j]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = (l < cn) ? p_lds[g][lc] : 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[g][j] += p * vf[j];
        }
      }
    }
    __syncthreads();  // p_lds / red_* reused by the next chunk
  }

  // ---- combine the RG row groups in a fixed order, one head at a time
#pragma unroll
  for (int g = 0; g < G; ++g) {
    f32x4v a;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.v[j] = acc[g][j];
    *reinterpret_cast<f32x4v*>(&part[vr * D + vd]) = a;
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

__global__ void attn_decode_merge_kernel(const float* __restrict__ ws,
                                         bf16* __restrict__ O, int H, int Hkv,
                                         int D, int nsplit) {
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
static void launch_ragged(hipStream_t stream, const void* Q, const void* K,
                          const void* V, void* ws, const void* lens, int B,
                          int H, int Hkv, int Smax, int split_rows, int nsplit,
                          float scale) {
  hipLaunchKernelGGL((attn_decode_ragged_kernel<D, G>), dim3(B * Hkv, nsplit),
                     dim3(DR_THREADS), 0, stream, (const bf16*)Q,
                     (const bf16*)K, (const bf16*)V, (float*)ws,
                     (const int*)lens, H, Hkv, Smax, split_rows, scale);
}

template <int D>
static int launch_ragged_g(int G, hipStream_t stream, const void* Q,
                           const void* K, const void* V, void* ws,
                           const void* lens, int B, int H, int Hkv, int Smax,
                           int split_rows, int nsplit, float scale) {
  switch (G) {
    case 1: launch_ragged<D, 1>(stream, Q, K, V, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    case 2: launch_ragged<D, 2>(stream, Q, K, V, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    case 4: launch_ragged<D, 4>(stream, Q, K, V, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    case 8: launch_ragged<D, 8>(stream, Q, K, V, ws, lens, B, H, Hkv, Smax, split_rows, nsplit, scale); break;
    default: return hipErrorInvalidValue;
  }
  return hipSuccess;
}

// Chunk length of the online softmax (ops.DECODE_RAGGED_CHUNK mirrors it).
PRIME_API int prime_decode_ragged_chunk(void) { return DR_CHUNK; }

// ws: fp32 [B*Hkv, ceil(Smax/split_rows), (H/Hkv)*(D+2)], caller-provided.
// split_rows: rows per split, a positive multiple of DR_CHUNK, chosen by the
// caller from (B*Hkv, Smax, CU count) only, never from lens.
PRIME_API int prime_attn_decode_ragged(hipStream_t stream, const void* Q,
                                       const void* K, const void* V, void* O,
                                       void* ws, const void* lens, int64_t B,
                                       int64_t H, int64_t Hkv, int64_t Smax,
                                       int64_t D, int64_t split_rows,
                                       double scale) {
  if ((D != 64 && D != 128) || B < 1 || H < 1 || Hkv < 1 || Smax < 1 ||
      H % Hkv != 0 || split_rows < DR_CHUNK || split_rows % DR_CHUNK != 0 ||
      !ws || !lens)
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  if (nsplit > 65535 || B * Hkv > 0x7fffffff || B * H > 0x7fffffff ||
      Smax > 0x7fffffff - split_rows)
    return hipErrorInvalidValue;
  int rc;
  if (D == 128)
    rc = launch_ragged_g<128>((int)G, stream, Q, K, V, ws, lens, (int)B,
                              (int)H, (int)Hkv, (int)Smax, (int)split_rows,
                              (int)nsplit, (float)scale);
  else
    rc = launch_ragged_g<64>((int)G, stream, Q, K, V, ws, lens, (int)B, (int)H,
                             (int)Hkv, (int)Smax, (int)split_rows, (int)nsplit,
                             (float)scale);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3((int)(B * H)),
                     dim3((int)D), 0, stream, (const float*)ws, (bf16*)O,
                     (int)H, (int)Hkv, (int)D, (int)nsplit);
  return (int)hipGetLastError();
}
