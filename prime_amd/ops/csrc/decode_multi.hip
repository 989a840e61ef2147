// Multi-token ragged decode attention for gfx950 (speculative / multi-token
// verification on the batched serving path).
//
// Every sequence brings up to T new tokens. lens[b] is the number of cache
// rows the FIRST new token attends to, n_new[b] the live new tokens; both
// are int32 DEVICE vectors read inside the kernels (graph replay), clamped:
//   L0 = clamp(lens[b], 0, Smax);  n = L0 ? clamp(n_new[b], 0,
//   min(T, Smax - L0 + 1)) : 0.
// Query t < n attends to rows [0, L0 + t); query t >= n gives exact zeros.
// No cache row at or beyond L0 + n - 1 is loaded.
//
// One workgroup (4 waves) owns the M = T*G query rows (row r = t*G + g) of
// one (b, kv head) and one row range [sp*split_rows, (sp+1)*split_rows)
// intersected with [0, L0 + n - 1). The waves split the KEYS: wave w takes
// keys kb = r0 + 32*w + 128*i, so every K/V byte is loaded by one wave.
//
// Per wave and 32-key step, on mfma_f32_16x16x32_bf16:
//   St[key][row] = K . Q^T   A = K row fragment: ONE 16 B global load per
//                            lane and k-step, no LDS. Lane (li, lg) reads
//                            d = lg*(D/4) + ks*8 + j, i.e. D/4 contiguous
//                            elements over its k-steps; Q uses the same
//                            contraction order, staged once per workgroup in
//                            LDS in fragment order.
//   softmax                  the accumulator holds St[key = lg*4 + r][row =
//                            li]: in-register max + __shfl_xor 16, 32.
//   O^T[d][row] = V^T . P^T  the two 16-key score tiles, rounded to bf16,
//                            ARE the B fragment P^T[kidx = lg*8 + j][row =
//                            li] in the key order key = 16*(j>>2) + lg*4 +
//                            (j&3). The mirrored (V^T as A) form keeps the
//                            query row on li in the O accumulator as well,
//                            so the online-softmax rescale needs no shuffle.
//   V                        staged per wave through LDS (16 B stores, row
//                            stride D + 8 elements), read back as 8 narrow
//                            reads per fragment in the same key order.
// The next step's K and V loads are issued before the current MFMAs. Loads
// that poke past the live range re-read its last row (V stays finite under
// weight 0). The causal / tail select runs only in steps that reach rows
// >= min(L0, end of range): a wave-uniform test.
//
// The waves' private (o, m, l) are combined once at the end through LDS in
// wave order; the split writes fp32 partials {o[M][D], m[M], l[M]}; empty
// splits write (0, -1e30, 0) and read no cache. attn_decode_multi_merge
// combines the splits in index order: no float atomics, bit-reproducible.
//
// Q, O [B,T,H,D], K/V cache [B,Smax,Hkv,D], ws fp32 [B*Hkv, nsplit,
// M*(D+2)]. D in {64,128}, G in {1,2,4,8}, 1 <= T <= 8, M <= 64.
//
// This file is compiled without the packed fp32 VALU instructions
// (ops/build.py, NO_PACKED_FP32).
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define DM_THREADS 256
#define DM_WAVES 4
#define DM_WKEYS 32                     // keys per wave and step
#define DM_CHUNK (DM_WAVES * DM_WKEYS)  // keys per workgroup step

// Clamped (L0, n) of slot b, the same in both kernels.
__device__ __forceinline__ void dm_live(const int* __restrict__ lens,
                                        const int* __restrict__ n_new, int b,
                                        int T, int Smax, int& L0, int& n) {
  L0 = min(max(lens[b], 0), Smax);
  n = L0 == 0 ? 0 : min(max(n_new[b], 0), min(T, Smax - L0 + 1));
}

// One step's operands: the two 16-key K fragment sets and the wave's 32 V
// rows. Rows past `last` re-read row `last`.
template <int D>
__device__ __forceinline__ void dm_load_kv(
    const bf16* __restrict__ Kb, const bf16* __restrict__ Vb,
    int64_t row_stride, int kb, int last, int lane, short8 (&kn)[2][D / 32],
    short8 (&vn)[D / 16]) {
  constexpr int LPR = D / 8;
  const int li = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int row = min(kb + 16 * s + li, last);
    const short8* kp = reinterpret_cast<const short8*>(
        Kb + (int64_t)row * row_stride + lg * (D / 4));
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) kn[s][ks] = kp[ks];
  }
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
    const int idx = i * 64 + lane;
    const int row = min(kb + idx / LPR, last);
    vn[i] = *reinterpret_cast<const short8*>(
        Vb + (int64_t)row * row_stride + (idx % LPR) * 8);
  }
}

template <int D, int MT>
__global__ __launch_bounds__(DM_THREADS) void attn_decode_multi_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new, int T, int H,
    int Hkv, int gsh, int Smax, int split_rows, float scale) {
  constexpr int KS = D / 32;    // k-steps of the score MFMA
  constexpr int DT = D / 16;    // 16-wide d tiles of O^T
  constexpr int NV = D / 16;    // 16 B V loads per lane and step
  constexpr int LPR = D / 8;    // lanes covering one V row
  constexpr int VSTR = D + 8;   // LDS V row stride (elements): 4 rows apart
                                // = 64 B mod 256, the four lg groups of a
                                // narrow read land in disjoint banks
  constexpr int MR = MT * 16;   // padded query rows
  constexpr int VW = DM_WKEYS * VSTR;  // elements of one wave's V tile
  static_assert(MR * D * 4 <= DM_WAVES * VW * 2, "o_lds aliases v_lds");
  const int G = 1 << gsh, M = T * G;
  const int PART = M * (D + 2);
  const int bk = blockIdx.x;
  const int b = bk / Hkv, hkv = bk - b * Hkv;
  const int sp = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  int L0, n;
  dm_live(lens, n_new, b, T, Smax, L0, n);
  const int r0 = sp * split_rows;
  const int r1 = n > 0 ? min(r0 + split_rows, L0 + n - 1) : 0;
  float* wsp = ws + ((int64_t)bk * nsplit + sp) * PART;

  if (r0 >= r1) {  // block-uniform: empty split, idle slot or n == 0
    for (int i = tid; i < PART; i += DM_THREADS)
      wsp[i] = (i >= M * D && i < M * D + M) ? -1e30f : 0.f;
    return;
  }

  __shared__ short8 q_lds[MT * KS * 64];  // Q^T fragments, fragment order
  __shared__ __attribute__((aligned(16))) short v_lds[DM_WAVES * VW];
  __shared__ float red_m[DM_WAVES][MR];
  __shared__ float red_l[DM_WAVES][MR];
  float* o_lds = reinterpret_cast<float*>(v_lds);  // after the key loop

  const int64_t row_stride = (int64_t)Hkv * D;
  const bf16* Kb = K + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const bf16* Vb = V + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;

  // ---- Q^T fragments: B[kidx = lg*8 + j][row = li] = Q[row][lg*(D/4) +
  // ks*8 + j]; padded rows (>= M) are zero
  for (int i = tid; i < MT * KS * 64; i += DM_THREADS) {
    const int ln = i & 63, f = i >> 6;
    const int mt = f / KS, ks = f - mt * KS;
    const int row = mt * 16 + (ln & 15);
    short8 x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < M) {
      const int t = row >> gsh, g = row & (G - 1);
      x = *reinterpret_cast<const short8*>(
          Q + (((int64_t)b * T + t) * H + (int64_t)hkv * G + g) * D +
          (ln >> 4) * (D / 4) + ks * 8);
    }
    q_lds[i] = x;
  }
  __syncthreads();

  // first row query (mt, li) may NOT see, within this split
  int lim[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    lim[mt] = min(r1, L0 + ((mt * 16 + li) >> gsh));
  const int lim_min = min(r1, L0);
  const int last = r1 - 1;  // loads past the range re-read this row

  float m[MT], l[MT];
  f32x4 acc[MT][DT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    m[mt] = -1e30f;
    l[mt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[mt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  short* vw = v_lds + wid * VW;  // this wave's V tile
  short8 kn[2][KS], vn[NV];
  int kb = r0 + wid * DM_WKEYS;
  if (kb < r1) dm_load_kv<D>(Kb, Vb, row_stride, kb, last, lane, kn, vn);
  for (; kb < r1; kb += DM_CHUNK) {  // wave-uniform trip count
    short8 kc[2][KS];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) kc[s][ks] = kn[s][ks];
    // V tile to LDS (wave-private: LDS operations of one wave complete in
    // order, so no workgroup barrier is needed around the tile)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = i * 64 + lane;
      *reinterpret_cast<short8*>(vw + (idx / LPR) * VSTR + (idx % LPR) * 8) =
          vn[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (kb + DM_CHUNK < r1)  // prefetch under the compute
      dm_load_kv<D>(Kb, Vb, row_stride, kb + DM_CHUNK, last, lane, kn, vn);

    // ---- scores of the two 16-key tiles against every row tile
    f32x4 sc[2][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      sc[0][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      sc[1][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const short8 qf = q_lds[(mt * KS + ks) * 64 + lane];
        sc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[0][ks], qf,
                                                            sc[0][mt], 0, 0, 0);
        sc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[1][ks], qf,
                                                            sc[1][mt], 0, 0, 0);
      }
    }

    // ---- online softmax in registers; P^T fragments
    const bool masked = kb + DM_WKEYS > lim_min;  // wave-uniform
    short8 pf[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = sc[j >> 2][mt][j & 3] * scale;
      if (masked) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int key = kb + 16 * (j >> 2) + lg * 4 + (j & 3);
          x[j] = key < lim[mt] ? x[j] : -1e30f;
        }
      }
      float mx = x[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) mx = fmaxf(mx, x[j]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m[mt], mx);
      // a row with no visible key yet subtracts 0: exp(-1e30) = 0 exactly
      const float msub = mnew == -1e30f ? 0.f : mnew;
      const float alpha = __expf(m[mt] - mnew);
      m[mt] = mnew;
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __expf(x[j] - msub);
        ps += p;
        const bf16 pb = f2bf(p);
        pf[mt][j] = *reinterpret_cast<const short*>(&pb);
      }
      l[mt] = l[mt] * alpha + ps;  // this lane's keys; lg-reduced at the end
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[mt][dt] *= alpha;
    }

    // ---- O^T += V^T . P^T: A[d = li][kidx = lg*8 + j] from the LDS tile
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      short8 vf;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vf[j] = vw[(16 * (j >> 2) + lg * 4 + (j & 3)) * VSTR + dt * 16 + li];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            vf, pf[mt], acc[mt][dt], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  // ---- combine the waves in wave order
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    l[mt] += __shfl_xor(l[mt], 16, 64);
    l[mt] += __shfl_xor(l[mt], 32, 64);
    if (lg == 0) {
      red_m[wid][mt * 16 + li] = m[mt];
      red_l[wid][mt * 16 + li] = l[mt];
    }
  }
  __syncthreads();  // stats visible; every wave is done with its V tile
  float mall[MT], lall[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = mt * 16 + li;
    float mx = red_m[0][row];
#pragma unroll
    for (int w = 1; w < DM_WAVES; ++w) mx = fmaxf(mx, red_m[w][row]);
    float ls = 0.f;
#pragma unroll
    for (int w = 0; w < DM_WAVES; ++w)
      ls += red_l[w][row] * __expf(red_m[w][row] - mx);
    mall[mt] = mx;
    lall[mt] = ls;
    const float f = __expf(m[mt] - mx);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[mt][dt] *= f;
  }
#pragma unroll
  for (int w = 0; w < DM_WAVES; ++w) {
    if (wid == w) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          f32x4* p = reinterpret_cast<f32x4*>(
              o_lds + (mt * 16 + li) * D + dt * 16 + lg * 4);
          *p = w == 0 ? acc[mt][dt] : *p + acc[mt][dt];
        }
    }
    __syncthreads();
  }
  for (int i = tid; i < M * D; i += DM_THREADS) wsp[i] = o_lds[i];
  if (wid == 0 && lg == 0) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = mt * 16 + li;
      if (row < M) {
        wsp[M * D + row] = mall[mt];
        wsp[M * D + M + row] = lall[mt];
      }
    }
  }
}

// grid B*T*H, D threads: splits combined in index order; dead queries
// (t >= n, idle slots) are written as exact zeros.
__global__ void attn_decode_multi_merge_kernel(
    const float* __restrict__ ws, bf16* __restrict__ O,
    const int* __restrict__ lens, const int* __restrict__ n_new, int T, int H,
    int Hkv, int D, int Smax, int nsplit) {
  const int bth = blockIdx.x;
  const int b = bth / (T * H);
  const int th = bth - b * (T * H);
  const int t = th / H, h = th - t * H;
  const int G = H / Hkv, M = T * G;
  const int hkv = h / G, row = t * G + (h - hkv * G);
  const int d = threadIdx.x;
  int L0, n;
  dm_live(lens, n_new, b, T, Smax, L0, n);
  bf16* o = O + (int64_t)bth * D + d;
  if (t >= n) {
    *o = f2bf(0.f);
    return;
  }
  const int part = M * (D + 2);
  const float* base = ws + ((int64_t)b * Hkv + hkv) * nsplit * part;
  float mx = -1e30f;
  for (int s = 0; s < nsplit; ++s)
    mx = fmaxf(mx, base[(int64_t)s * part + M * D + row]);
  float num = 0.f, den = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* ps = base + (int64_t)s * part;
    const float w = __expf(ps[M * D + row] - mx);
    den += w * ps[M * D + M + row];
    num += w * ps[row * D + d];
  }
  *o = f2bf(num / fmaxf(den, 1e-30f));
}

template <int D, int MT>
static void launch_multi(hipStream_t stream, const void* Q, const void* K,
                         const void* V, void* ws, const void* lens,
                         const void* n_new, int B, int T, int H, int Hkv,
                         int gsh, int Smax, int split_rows, int nsplit,
                         float scale) {
  hipLaunchKernelGGL((attn_decode_multi_kernel<D, MT>), dim3(B * Hkv, nsplit),
                     dim3(DM_THREADS), 0, stream, (const bf16*)Q,
                     (const bf16*)K, (const bf16*)V, (float*)ws,
                     (const int*)lens, (const int*)n_new, T, H, Hkv, gsh, Smax,
                     split_rows, scale);
}

template <int D>
static void launch_multi_mt(int MT, hipStream_t stream, const void* Q,
                            const void* K, const void* V, void* ws,
                            const void* lens, const void* n_new, int B, int T,
                            int H, int Hkv, int gsh, int Smax, int split_rows,
                            int nsplit, float scale) {
  switch (MT) {
    case 1: launch_multi<D, 1>(stream, Q, K, V, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
    case 2: launch_multi<D, 2>(stream, Q, K, V, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
    case 3: launch_multi<D, 3>(stream, Q, K, V, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
    default: launch_multi<D, 4>(stream, Q, K, V, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
  }
}

// Keys per workgroup step (ops.DECODE_MULTI_CHUNK mirrors it).
PRIME_API int prime_decode_multi_chunk(void) { return DM_CHUNK; }

// ws: fp32 [B*Hkv, ceil(Smax/split_rows), T*(H/Hkv)*(D+2)], caller-provided.
// split_rows: a positive multiple of DM_CHUNK chosen from the launch shape
// only, never from lens or n_new.
PRIME_API int prime_attn_decode_ragged_multi(
    hipStream_t stream, const void* Q, const void* K, const void* V, void* O,
    void* ws, const void* lens, const void* n_new, int64_t B, int64_t T,
    int64_t H, int64_t Hkv, int64_t Smax, int64_t D, int64_t split_rows,
    double scale) {
  if ((D != 64 && D != 128) || B < 1 || T < 1 || T > 8 || H < 1 || Hkv < 1 ||
      Smax < 1 || H % Hkv != 0 || split_rows < DM_CHUNK ||
      split_rows % DM_CHUNK != 0 || !ws || !lens || !n_new)
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return hipErrorInvalidValue;
  const int64_t M = T * G;
  if (M > 64) return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  if (nsplit > 65535 || B * Hkv > 0x7fffffff || B * T * H > 0x7fffffff ||
      Smax > 0x7fffffff - split_rows - 8)
    return hipErrorInvalidValue;
  const int gsh = G == 1 ? 0 : (G == 2 ? 1 : (G == 4 ? 2 : 3));
  const int MT = (int)((M + 15) / 16);
  if (D == 128)
    launch_multi_mt<128>(MT, stream, Q, K, V, ws, lens, n_new, (int)B, (int)T,
                         (int)H, (int)Hkv, gsh, (int)Smax, (int)split_rows,
                         (int)nsplit, (float)scale);
  else
    launch_multi_mt<64>(MT, stream, Q, K, V, ws, lens, n_new, (int)B, (int)T,
                        (int)H, (int)Hkv, gsh, (int)Smax, (int)split_rows,
                        (int)nsplit, (float)scale);
  hipLaunchKernelGGL(attn_decode_multi_merge_kernel, dim3((int)(B * T * H)),
                     dim3((int)D), 0, stream, (const float*)ws, (bf16*)O,
                     (const int*)lens, (const int*)n_new, (int)T, (int)H,
                     (int)Hkv, (int)D, (int)Smax, (int)nsplit);
  return (int)hipGetLastError();
}
