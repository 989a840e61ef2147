// Multi-token ragged decode over the fp8 (OCP e4m3fn) KV cache for gfx950:
// the contract of decode_multi.hip (grid, key split over the four waves,
// lens / n_new clamp, empty-split rule, workspace layout, wave-order
// combine, index-order merge) with the cache format of decode_fp8kv.hip
// (k, v bytes [B,Smax,Hkv,D]; k_scale, v_scale fp32 [B,Smax,Hkv], value =
// float(byte) * scale). The values attended to are kv_cache_dequant(cache);
// q, the scores, P and the accumulators are not quantised.
//
// Per wave and 32-key step, on mfma_f32_16x16x32_bf16 with both fragment
// maps of decode_multi.hip:
//   K        lane (li, lg) of key tile s reads the D/4 contiguous BYTES
//            lg*(D/4).. of row kb + 16*s + li (16 B loads: two at D = 128,
//            one at D = 64). The eight bytes at offset ks*8 are k-step ks,
//            the contraction order d = lg*(D/4) + ks*8 + j of the Q^T
//            staging, so q_lds is that of the bf16 kernel. Bytes go to fp32
//            through the conversion instruction (OCP on this target) and to
//            bf16 by keeping the upper 16 bits: every finite e4m3 value,
//            subnormals included, has at most 4 significant bits and an
//            exponent inside the bf16 range, so the lower 16 bits of its
//            fp32 form are zero and no rounding step exists to skip.
//   k_scale  the score accumulator holds St[key = lg*4 + r][row = li], so a
//            lane owns 8 keys per step and multiplies register j by
//            k_scale[key_j] * scale before the mask, max and exp.
//   v_scale  folded into P before rounding: the P^T fragment is
//            bf16(p * v_scale[key_j]) while the running sum keeps the
//            unscaled fp32 p (the rule of the single-token fp8 kernel). The
//            V phase handles no scale. A masked p is exactly 0.
//   V        each wave loads its 32 rows as D/32 16 B loads per lane (a row
//            is D/16 consecutive lanes), decodes the 16 bytes to 16 bf16 and
//            writes them as two 16 B LDS stores into the SAME image the bf16
//            kernel uses (row stride D + 8 elements); fragment reads, PV
//            MFMAs and fences are unchanged.
// The next step's K bytes, V bytes and 16 scales are issued before the
// current MFMAs. Rows and scales past the live range re-read row `last`:
// no K/V row and no scale at or beyond L0 + n - 1 is loaded.
//
// decode_qkv_append_multi_fp8_kernel is decode_qkv_append_multi_kernel's
// token rule (decode_prep.hip) with decode_qkv_append_fp8_kernel's work
// split and quantisation (decode_fp8kv.hip).
//
// The library is one non-RDC link, so dm_live and the merge kernel are
// copied here under their own names. This file is compiled without the
// packed fp32 VALU instructions (ops/build.py, NO_PACKED_FP32).
#include "common.h"
#include <hip/hip_fp8.h>

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef unsigned char u8;

#define DM8_THREADS 256
#define DM8_WAVES 4
#define DM8_WKEYS 32                       // keys per wave and step
#define DM8_CHUNK (DM8_WAVES * DM8_WKEYS)  // = DM_CHUNK of decode_multi.hip

// Clamped (L0, n) of slot b: dm_live of decode_multi.hip.
__device__ __forceinline__ void dm8_live(const int* __restrict__ lens,
                                         const int* __restrict__ n_new, int b,
                                         int T, int Smax, int& L0, int& n) {
  L0 = min(max(lens[b], 0), Smax);
  n = L0 == 0 ? 0 : min(max(n_new[b], 0), min(T, Smax - L0 + 1));
}

// Four e4m3 bytes of one dword -> four bf16 in two dwords (element j of the
// dword in byte j). The upper half of the fp32 IS the bf16 (see the head).
__device__ __forceinline__ void dm8_dec4(unsigned w, unsigned& d0,
                                         unsigned& d1) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  d0 = __builtin_amdgcn_perm(__float_as_uint(lo.y), __float_as_uint(lo.x),
                             0x07060302u);
  d1 = __builtin_amdgcn_perm(__float_as_uint(hi.y), __float_as_uint(hi.x),
                             0x07060302u);
}

// Eight bytes (two dwords) -> one MFMA operand of eight bf16.
__device__ __forceinline__ short8 dm8_dec8(unsigned w0, unsigned w1) {
  u32x4 d;
  unsigned a, b;
  dm8_dec4(w0, a, b);
  d[0] = a; d[1] = b;
  dm8_dec4(w1, a, b);
  d[2] = a; d[3] = b;
  return __builtin_bit_cast(short8, d);
}

// One step's operands: the K bytes of the two 16-key tiles, the wave's 32 V
// rows and the 8 + 8 scales of this lane's score registers. Rows and scales
// past `last` re-read row `last`.
template <int D>
__device__ __forceinline__ void dm8_load(
    const u8* __restrict__ Kb, const u8* __restrict__ Vb,
    const float* __restrict__ Ksb, const float* __restrict__ Vsb,
    int64_t row_stride, int Hkv, int kb, int last, int lane,
    u32x4 (&kn)[2][D / 64], u32x4 (&vn)[D / 32], float (&ksn)[8],
    float (&vsn)[8]) {
  constexpr int LPR = D / 16;  // lanes covering one V row
  const int li = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int row = min(kb + 16 * s + li, last);
    const u32x4* kp = reinterpret_cast<const u32x4*>(
        Kb + (int64_t)row * row_stride + lg * (D / 4));
#pragma unroll
    for (int i = 0; i < D / 64; ++i) kn[s][i] = kp[i];
  }
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int idx = i * 64 + lane;
    const int row = min(kb + idx / LPR, last);
    vn[i] = *reinterpret_cast<const u32x4*>(
        Vb + (int64_t)row * row_stride + (idx % LPR) * 16);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t key = min(kb + 16 * (j >> 2) + lg * 4 + (j & 3), last);
    ksn[j] = Ksb[key * Hkv];
    vsn[j] = Vsb[key * Hkv];
  }
}

// Workgroups per CU (= waves per SIMD) the register allocator is held to:
// the counts each instantiation reaches without scratch (docs/KERNELS.md).
// Left to itself the compiler lands 4-8 registers above the next step at
// D = 128 MT <= 2 and D = 64 MT <= 2.
constexpr int dm8_min_blocks(int D, int MT) {
  return D == 128 ? (MT == 1 ? 3 : (MT == 2 ? 2 : 1))
                  : (MT == 1 ? 4 : (MT == 2 ? 3 : (MT == 3 ? 2 : 1)));
}

template <int D, int MT>
__global__ __launch_bounds__(DM8_THREADS, dm8_min_blocks(D, MT)) void
attn_decode_multi_fp8_kernel(
    const bf16* __restrict__ Q, const u8* __restrict__ K,
    const u8* __restrict__ V, const float* __restrict__ Ks,
    const float* __restrict__ Vs, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new, int T, int H,
    int Hkv, int gsh, int Smax, int split_rows, float scale) {
  constexpr int KS = D / 32;    // k-steps of the score MFMA
  constexpr int DT = D / 16;    // 16-wide d tiles of O^T
  constexpr int NK = D / 64;    // 16 B K loads per lane and key tile
  constexpr int NV = D / 32;    // 16 B V loads per lane and step
  constexpr int LPR = D / 16;   // lanes covering one V row
  constexpr int VSTR = D + 8;   // LDS V row stride (bf16 elements), as in
                                // decode_multi.hip
  constexpr int MR = MT * 16;   // padded query rows
  constexpr int VW = DM8_WKEYS * VSTR;  // elements of one wave's V tile
  static_assert(MR * D * 4 <= DM8_WAVES * VW * 2, "o_lds aliases v_lds");
  const int G = 1 << gsh, M = T * G;
  const int PART = M * (D + 2);
  const int bk = blockIdx.x;
  const int b = bk / Hkv, hkv = bk - b * Hkv;
  const int sp = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  int L0, n;
  dm8_live(lens, n_new, b, T, Smax, L0, n);
  const int r0 = sp * split_rows;
  const int r1 = n > 0 ? min(r0 + split_rows, L0 + n - 1) : 0;
  float* wsp = ws + ((int64_t)bk * nsplit + sp) * PART;

  if (r0 >= r1) {  // block-uniform: empty split, idle slot or n == 0
    for (int i = tid; i < PART; i += DM8_THREADS)
      wsp[i] = (i >= M * D && i < M * D + M) ? -1e30f : 0.f;
    return;
  }

  __shared__ short8 q_lds[MT * KS * 64];  // Q^T fragments, fragment order
  __shared__ __attribute__((aligned(16))) short v_lds[DM8_WAVES * VW];
  __shared__ float red_m[DM8_WAVES][MR];
  __shared__ float red_l[DM8_WAVES][MR];
  float* o_lds = reinterpret_cast<float*>(v_lds);  // after the key loop

  const int64_t row_stride = (int64_t)Hkv * D;  // bytes = elements
  const u8* Kb = K + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const u8* Vb = V + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const float* Ksb = Ks + (int64_t)b * Smax * Hkv + hkv;
  const float* Vsb = Vs + (int64_t)b * Smax * Hkv + hkv;

  // ---- Q^T fragments: B[kidx = lg*8 + j][row = li] = Q[row][lg*(D/4) +
  // ks*8 + j]; padded rows (>= M) are zero
  for (int i = tid; i < MT * KS * 64; i += DM8_THREADS) {
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
  u32x4 kn[2][NK], vn[NV];
  float ksn[8], vsn[8];
  int kb = r0 + wid * DM8_WKEYS;
  if (kb < r1)
    dm8_load<D>(Kb, Vb, Ksb, Vsb, row_stride, Hkv, kb, last, lane, kn, vn,
                ksn, vsn);
  for (; kb < r1; kb += DM8_CHUNK) {  // wave-uniform trip count
    u32x4 kc[2][NK];
    float ksc[8], vsc[8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < NK; ++i) kc[s][i] = kn[s][i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ksc[j] = ksn[j] * scale;
      vsc[j] = vsn[j];
    }
    // V tile to LDS as bf16 (wave-private: LDS operations of one wave
    // complete in order, so no workgroup barrier is needed around the tile)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = i * 64 + lane;
      short* dst = vw + (idx / LPR) * VSTR + (idx % LPR) * 16;
      *reinterpret_cast<short8*>(dst) = dm8_dec8(vn[i][0], vn[i][1]);
      *reinterpret_cast<short8*>(dst + 8) = dm8_dec8(vn[i][2], vn[i][3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (kb + DM8_CHUNK < r1)  // prefetch under the compute
      dm8_load<D>(Kb, Vb, Ksb, Vsb, row_stride, Hkv, kb + DM8_CHUNK, last,
                  lane, kn, vn, ksn, vsn);

    // ---- scores of the two 16-key tiles against every row tile; k-step
    // outermost, so a decoded K fragment lives for MT MFMAs only
    f32x4 sc[2][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      sc[0][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      sc[1][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const short8 k0 = dm8_dec8(kc[0][ks >> 1][(ks & 1) * 2],
                                 kc[0][ks >> 1][(ks & 1) * 2 + 1]);
      const short8 k1 = dm8_dec8(kc[1][ks >> 1][(ks & 1) * 2],
                                 kc[1][ks >> 1][(ks & 1) * 2 + 1]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const short8 qf = q_lds[(mt * KS + ks) * 64 + lane];
        sc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf, sc[0][mt],
                                                            0, 0, 0);
        sc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf, sc[1][mt],
                                                            0, 0, 0);
      }
    }

    // ---- online softmax in registers; P^T fragments carry v_scale
    const bool masked = kb + DM8_WKEYS > lim_min;  // wave-uniform
    short8 pf[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = sc[j >> 2][mt][j & 3] * ksc[j];
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
        ps += p;  // the running sum keeps the unscaled weight
        const bf16 pb = f2bf(p * vsc[j]);
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
    for (int w = 1; w < DM8_WAVES; ++w) mx = fmaxf(mx, red_m[w][row]);
    float ls = 0.f;
#pragma unroll
    for (int w = 0; w < DM8_WAVES; ++w)
      ls += red_l[w][row] * __expf(red_m[w][row] - mx);
    mall[mt] = mx;
    lall[mt] = ls;
    const float f = __expf(m[mt] - mx);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[mt][dt] *= f;
  }
#pragma unroll
  for (int w = 0; w < DM8_WAVES; ++w) {
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
  for (int i = tid; i < M * D; i += DM8_THREADS) wsp[i] = o_lds[i];
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

// This file's copy of attn_decode_multi_merge_kernel (decode_multi.hip).
// grid B*T*H, D threads: splits combined in index order; dead queries
// (t >= n, idle slots) are written as exact zeros.
__global__ void attn_decode_multi_fp8_merge_kernel(
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
  dm8_live(lens, n_new, b, T, Smax, L0, n);
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
static void launch_multi_fp8(hipStream_t stream, const void* Q, const void* K,
                             const void* V, const void* Ks, const void* Vs,
                             void* ws, const void* lens, const void* n_new,
                             int B, int T, int H, int Hkv, int gsh, int Smax,
                             int split_rows, int nsplit, float scale) {
  hipLaunchKernelGGL((attn_decode_multi_fp8_kernel<D, MT>),
                     dim3(B * Hkv, nsplit), dim3(DM8_THREADS), 0, stream,
                     (const bf16*)Q, (const u8*)K, (const u8*)V,
                     (const float*)Ks, (const float*)Vs, (float*)ws,
                     (const int*)lens, (const int*)n_new, T, H, Hkv, gsh, Smax,
                     split_rows, scale);
}

template <int D>
static void launch_multi_fp8_mt(int MT, hipStream_t stream, const void* Q,
                                const void* K, const void* V, const void* Ks,
                                const void* Vs, void* ws, const void* lens,
                                const void* n_new, int B, int T, int H,
                                int Hkv, int gsh, int Smax, int split_rows,
                                int nsplit, float scale) {
  switch (MT) {
    case 1: launch_multi_fp8<D, 1>(stream, Q, K, V, Ks, Vs, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
    case 2: launch_multi_fp8<D, 2>(stream, Q, K, V, Ks, Vs, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
    case 3: launch_multi_fp8<D, 3>(stream, Q, K, V, Ks, Vs, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
    default: launch_multi_fp8<D, 4>(stream, Q, K, V, Ks, Vs, ws, lens, n_new, B, T, H, Hkv, gsh, Smax, split_rows, nsplit, scale); break;
  }
}

// The contract of prime_attn_decode_ragged_multi (ws layout, split_rows a
// positive multiple of the chunk chosen from the launch shape only), with
// the cache as e4m3 bytes K/V [B,Smax,Hkv,D] + fp32 k_scale/v_scale
// [B,Smax,Hkv].
PRIME_API int prime_attn_decode_ragged_multi_fp8(
    hipStream_t stream, const void* Q, const void* K, const void* V,
    const void* k_scale, const void* v_scale, void* O, void* ws,
    const void* lens, const void* n_new, int64_t B, int64_t T, int64_t H,
    int64_t Hkv, int64_t Smax, int64_t D, int64_t split_rows, double scale) {
  if ((D != 64 && D != 128) || B < 1 || T < 1 || T > 8 || H < 1 || Hkv < 1 ||
      Smax < 1 || H % Hkv != 0 || split_rows < DM8_CHUNK ||
      split_rows % DM8_CHUNK != 0 || !ws || !lens || !n_new || !k_scale ||
      !v_scale)
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
    launch_multi_fp8_mt<128>(MT, stream, Q, K, V, k_scale, v_scale, ws, lens,
                             n_new, (int)B, (int)T, (int)H, (int)Hkv, gsh,
                             (int)Smax, (int)split_rows, (int)nsplit,
                             (float)scale);
  else
    launch_multi_fp8_mt<64>(MT, stream, Q, K, V, k_scale, v_scale, ws, lens,
                            n_new, (int)B, (int)T, (int)H, (int)Hkv, gsh,
                            (int)Smax, (int)split_rows, (int)nsplit,
                            (float)scale);
  hipLaunchKernelGGL(attn_decode_multi_fp8_merge_kernel,
                     dim3((int)(B * T * H)), dim3((int)D), 0, stream,
                     (const float*)ws, (bf16*)O, (const int*)lens,
                     (const int*)n_new, (int)T, (int)H, (int)Hkv, (int)D,
                     (int)Smax, (int)nsplit);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ decode append
// max over an aligned group of W consecutive lanes (W a power of two <= 64)
template <int W>
__device__ __forceinline__ float dm8_group_max(float x) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1)
    x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}

// four e4m3 bytes of clamp(x * s), element j in byte j
__device__ __forceinline__ unsigned dm8_quant4(const float* x, float s) {
  unsigned w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float q = fminf(fmaxf(x[j] * s, -448.f), 448.f);
    w |= (unsigned)__hip_fp8_e4m3(q).__x << (8 * j);
  }
  return w;
}

// qkv [B,TN,(H+2Hkv)*D]; token t of slot b is rotated at pos[b] + t and
// quantised into cache row pos[b] + t. A head row is covered by D/8
// consecutive threads, an aligned sub-group of one wave that takes the same
// branches; the row amax is a shuffle reduction inside it.
template <int D>
__global__ __launch_bounds__(256) void decode_qkv_append_multi_fp8_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ qout,
    u8* __restrict__ kc, u8* __restrict__ vc, float* __restrict__ ksc,
    float* __restrict__ vsc, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, const int* __restrict__ pos,
    const int* __restrict__ n_new, int64_t nrows, int TN, int H, int Hkv,
    int Smax, int T, float sign) {
  constexpr int half = D / 2;
  constexpr int hv = half / 4;  // threads per head row: 8 or 16
  const int NH = H + 2 * Hkv;
  const int lim = min(Smax, T);
  const int64_t total = nrows * hv;  // a multiple of hv: groups stay whole
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / hv;  // (b, t, head of the packed row)
    const int i4 = (int)(idx - row * hv) * 4;
    const int64_t bt = row / NH;
    const int hh = (int)(row - bt * NH);
    const int64_t b = bt / TN;
    const int t = (int)(bt - b * TN);
    const int p0 = pos[b];
    // p0 < lim - t, not p0 + t < lim: no overflow for any p0
    const bool live = p0 >= 0 && t < n_new[b] && p0 < lim - t;
    const int p = p0 + t;
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
    am = dm8_group_max<hv>(am);
    if (isq) {  // dead token: zeros
      bf16* dst = qout + (bt * H + hh) * D;
      *reinterpret_cast<bf16x4*>(dst + i4) = y1;
      *reinterpret_cast<bf16x4*>(dst + half + i4) = y2;
    } else if (live) {
      const int hk = hh - H;
      const bool isk = hk < Hkv;
      const int64_t orow = (b * Smax + p) * Hkv + (isk ? hk : hk - Hkv);
      u8* dst = (isk ? kc : vc) + orow * D;
      const float m = fmaxf(am, 1e-12f);
      const float s = 448.f / m;
      *reinterpret_cast<unsigned*>(dst + i4) = dm8_quant4(f1, s);
      *reinterpret_cast<unsigned*>(dst + half + i4) = dm8_quant4(f2, s);
      if (i4 == 0) (isk ? ksc : vsc)[orow] = m / 448.f;
    }
  }
}

static int dm8_append_launch(
    hipStream_t stream, const void* qkv, void* qout, void* kc, void* vc,
    void* k_scale, void* v_scale, const void* cos_t, const void* sin_t,
    const void* pos, const void* n_new, int64_t B, int64_t TN, int64_t H,
    int64_t Hkv, int64_t D, int64_t Smax, int64_t T) {
  const int64_t nrows = B * TN * (H + 2 * Hkv);
  const int grid = prime_grid(nrows * (D / 8), 256);
  if (D == 128)
    hipLaunchKernelGGL((decode_qkv_append_multi_fp8_kernel<128>), dim3(grid),
                       dim3(256), 0, stream, (const bf16*)qkv, (bf16*)qout,
                       (u8*)kc, (u8*)vc, (float*)k_scale, (float*)v_scale,
                       (const float*)cos_t, (const float*)sin_t,
                       (const int*)pos, (const int*)n_new, nrows, (int)TN,
                       (int)H, (int)Hkv, (int)Smax, (int)T, 1.f);
  else
    hipLaunchKernelGGL((decode_qkv_append_multi_fp8_kernel<64>), dim3(grid),
                       dim3(256), 0, stream, (const bf16*)qkv, (bf16*)qout,
                       (u8*)kc, (u8*)vc, (float*)k_scale, (float*)v_scale,
                       (const float*)cos_t, (const float*)sin_t,
                       (const int*)pos, (const int*)n_new, nrows, (int)TN,
                       (int)H, (int)Hkv, (int)Smax, (int)T, 1.f);
  return (int)hipGetLastError();
}

// TN: new tokens per sequence in qkv; T: rows of the cos / sin tables.
PRIME_API int prime_decode_qkv_append_multi_fp8(
    hipStream_t stream, const void* qkv, void* qout, void* kc, void* vc,
    void* k_scale, void* v_scale, const void* cos_t, const void* sin_t,
    const void* pos, const void* n_new, int64_t B, int64_t TN, int64_t H,
    int64_t Hkv, int64_t D, int64_t Smax, int64_t T) {
  if ((D != 64 && D != 128) || B < 1 || TN < 1 || TN > 8 || H < 1 ||
      Hkv < 1 || Smax < 1 || T < 1 || Smax > 0x7fffffff || T > 0x7fffffff ||
      !pos || !n_new || !k_scale || !v_scale)
    return hipErrorInvalidValue;
  return dm8_append_launch(stream, qkv, qout, kc, vc, k_scale, v_scale, cos_t,
                           sin_t, pos, n_new, B, TN, H, Hkv, D, Smax, T);
}

// The same pass for a prefill chunk: any TN >= 1 (the kernel is TN-agnostic;
// the entry above keeps its cap for the verification path).
PRIME_API int prime_prefill_qkv_append_fp8(
    hipStream_t stream, const void* qkv, void* qout, void* kc, void* vc,
    void* k_scale, void* v_scale, const void* cos_t, const void* sin_t,
    const void* pos, const void* n_new, int64_t B, int64_t TN, int64_t H,
    int64_t Hkv, int64_t D, int64_t Smax, int64_t T) {
  if ((D != 64 && D != 128) || B < 1 || TN < 1 || H < 1 || Hkv < 1 ||
      Smax < 1 || T < 1 || Smax > 0x7fffffff || T > 0x7fffffff ||
      TN > 0x7fffffff || !pos || !n_new || !k_scale || !v_scale)
    return hipErrorInvalidValue;
  return dm8_append_launch(stream, qkv, qout, kc, vc, k_scale, v_scale, cos_t,
                           sin_t, pos, n_new, B, TN, H, Hkv, D, Smax, T);
}
