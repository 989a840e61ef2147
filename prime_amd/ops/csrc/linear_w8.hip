// Weight-only fp8 linear for decode-sized batches on gfx950:
//   y[m][n] = bf16(sinv[n] * sum_k x[m][k] * dec(byte[n][k])),  1 <= M <= 64.
// A decode step is a pure weight stream; this kernel reads the weights as
// e4m3 bytes (one per value) with one fp32 scale per output channel.
//
// Format (ops.LinearW8): bytes uint8 [N/16][K/64][64][16]. The 16 bytes of
// lane l = lg*16 + li in tile (nt, kc) are row nt*16 + li, columns kc*64 +
// lg*16 .. +15 of the row-major matrix, so every wave load is one linear,
// fully coalesced 1 KiB. sinv fp32 [N].
//
// Operands, swapped as in decode_multi.hip, on mfma_f32_16x16x32_bf16:
//   A = weight tile    A[n = li][kidx = lg*8 + j]
//   B = x^T            B[kidx = lg*8 + j][m = li]
//   C = y^T            C[n = lg*4 + r][m = li]
// One 16 B weight load per lane feeds two MFMA k-steps per m-tile: lane group
// lg, step s, element j is column kc*64 + lg*16 + s*8 + j, and x uses the
// same contraction order. The bytes are decoded in registers
// (cvt_pk_f32_fp8, then the upper half of each fp32 with one v_perm_b32 per
// pair: exact, a finite e4m3 value has at most 4 significant bits and an
// exponent inside the bf16 range), once, by the only wave that loads them.
//
// Work split: 256 threads. A workgroup owns 64 output rows, one 16-row tile
// per wave, over one K range of the grid (N/64, ksplit). The four waves
// share the x fragments: the workgroup stages x in chunks of 256 columns
// into LDS in fragment order ([kc][mt][s][lane] x 16 B, rows >= M as zeros),
// double-buffered with one barrier per chunk; fragment reads are linear
// ds_read_b128. Chunk c+1's global x loads are issued at the head of chunk
// c and stored to the other buffer at its end.
//
// Weight loads are ordinary tracked register loads in a ring of 8 per wave
// (two chunks ahead), running across the chunk barriers: the barrier orders
// LDS only, and the waits in the body are counted vmcnt(n).
//
// ksplit == 1: the kernel scales, rounds and stores bf16 itself. Otherwise
// it writes fp32 partials [ksplit][M][N] and linear_w8_merge_kernel adds
// them in index order, scales and rounds: no float atomics, two calls are
// bit-identical.
//
// This file is compiled without the packed fp32 VALU instructions
// (ops/build.py, NO_PACKED_FP32).
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

#define LW_THREADS 256
#define LW_ROWS 64     // output rows per workgroup
#define LW_CHUNK 256   // x columns per LDS chunk
#define LW_KC 4        // 64-column weight tiles per chunk
#define LW_RING 8      // weight loads in flight per wave

// Eight e4m3 bytes (two dwords, element j in byte j) -> eight bf16.
__device__ __forceinline__ short8 lw_dec8(unsigned w0, unsigned w1) {
  u32x4 d;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned w = h ? w1 : w0;
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    d[2 * h] = __builtin_amdgcn_perm(__float_as_uint(a.y), __float_as_uint(a.x),
                                     0x07060302u);
    d[2 * h + 1] = __builtin_amdgcn_perm(__float_as_uint(c.y),
                                         __float_as_uint(c.x), 0x07060302u);
  }
  return __builtin_bit_cast(short8, d);
}

// Workgroup barrier that orders LDS traffic only: the weight ring's global
// loads stay in flight across it.
__device__ __forceinline__ void lw_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// This thread's share of one x chunk in fragment order: unit u = i*256 + tid
// is LDS slot u of the chunk image, f = u >> 6 = (kc*MT + mt)*2 + s.
template <int MT>
__device__ __forceinline__ void lw_load_x(const bf16* __restrict__ X, int M,
                                          int K, int k0, int tid,
                                          short8 (&xr)[2 * MT]) {
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) {
    const int u = i * LW_THREADS + tid;
    const int ln = u & 63, f = u >> 6;
    const int s = f & 1, mt = (f >> 1) % MT, kc = (f >> 1) / MT;
    const int row = mt * 16 + (ln & 15);
    // every lane loads (a padded row re-reads row M - 1), so that the
    // number of loads in flight does not depend on a branch
    const short8 v = *reinterpret_cast<const short8*>(
        X + (int64_t)min(row, M - 1) * K + k0 + kc * 64 + (ln >> 4) * 16 +
        s * 8);
    xr[i] = row < M ? v : short8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

template <int MT>
__device__ __forceinline__ void lw_store_x(short8* buf, int tid,
                                           const short8 (&xr)[2 * MT]) {
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) buf[i * LW_THREADS + tid] = xr[i];
}

// One 256-column chunk: H = c & 1 is both the LDS buffer and the half of the
// weight ring that holds the chunk's four tiles.
template <int MT, int H>
__device__ __forceinline__ void lw_chunk(
    const bf16* __restrict__ X, const u32x4* __restrict__ wp, short8* x_lds,
    int M, int K, int k0, int c, int nchunk, int tid, int lane,
    u32x4 (&wr)[LW_RING], f32x4 (&acc)[MT]) {
  constexpr int IMG = LW_KC * MT * 2 * 64;  // short8 slots of one chunk image
  lw_lds_barrier();  // chunk c is visible; buffer H ^ 1 is free
  // Every load below is unconditional: past the end of the range the x
  // chunk and the weight tiles re-read the last ones (cache hits, never
  // used). With a branch around a load the compiler has to assume it was
  // not issued and the waits fall back to vmcnt(0).
  short8 xr[2 * MT];
  lw_load_x<MT>(X, M, K, k0 + min(c + 1, nchunk - 1) * LW_CHUNK, tid, xr);
  const short8* xb = x_lds + H * IMG + lane;
#pragma unroll
  for (int kc = 0; kc < LW_KC; ++kc) {
    const u32x4 w = wr[H * LW_KC + kc];
    const short8 a0 = lw_dec8(w[0], w[1]);
    const short8 a1 = lw_dec8(w[2], w[3]);
    // refill the slot two chunks ahead, after its last use: the load then
    // lands in the slot's own registers and the loop needs no copies of
    // them (a copy of a register in flight is a vmcnt(0))
    __builtin_amdgcn_sched_barrier(0);
    wr[H * LW_KC + kc] =
        wp[(int64_t)min((c + 2) * LW_KC + kc, nchunk * LW_KC - 1) * 64];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const short8 b0 = xb[((kc * MT + mt) * 2 + 0) * 64];
      const short8 b1 = xb[((kc * MT + mt) * 2 + 1) * 64];
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[mt], 0, 0, 0);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[mt], 0, 0, 0);
    }
  }
  lw_store_x<MT>(x_lds + (H ^ 1) * IMG, tid, xr);
}

// grid (N/64, ksplit). Y: bf16 [M][N] when ksplit == 1, else fp32 partials
// [ksplit][M][N].
template <int MT>
__global__ __launch_bounds__(LW_THREADS) void linear_w8_kernel(
    const bf16* __restrict__ X, const unsigned char* __restrict__ W8,
    const float* __restrict__ sinv, void* __restrict__ Y, int M, int N, int K,
    int nchunk) {
  constexpr int IMG = LW_KC * MT * 2 * 64;
  __shared__ short8 x_lds[2 * IMG];
  __builtin_assume(nchunk >= 1);  // keeps the ring's first loads up here
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int sp = blockIdx.y;
  const int k0 = sp * nchunk * LW_CHUNK;  // first column of this K range
  const int nt = blockIdx.x * (LW_ROWS / 16) + wid;

  // tile (nt, kc) is 64 lanes x 16 B; wp is this lane's slot of the range's
  // first tile, tile t of the range sits 64 slots further per t
  const u32x4* wp = reinterpret_cast<const u32x4*>(W8) +
                    ((int64_t)nt * (K / 64) + k0 / 64) * 64 + lane;
  // chunk 0 of x first, then the ring: the LDS store of x then waits on
  // vmcnt(LW_RING) and the weight loads stay in flight
  u32x4 wr[LW_RING];
  {
    short8 xr[2 * MT];
    lw_load_x<MT>(X, M, K, k0, tid, xr);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < LW_RING; ++i)
      wr[i] = wp[(int64_t)min(i, nchunk * LW_KC - 1) * 64];
    __builtin_amdgcn_sched_barrier(0);
    lw_store_x<MT>(x_lds, tid, xr);
  }

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < nchunk; c += 2) {  // block-uniform trip count
    lw_chunk<MT, 0>(X, wp, x_lds, M, K, k0, c, nchunk, tid, lane, wr, acc);
    if (c + 1 < nchunk)
      lw_chunk<MT, 1>(X, wp, x_lds, M, K, k0, c + 1, nchunk, tid, lane, wr,
                      acc);
  }

  // ---- epilogue: acc[mt][r] is y[m = mt*16 + li][n = nrow + r]
  const int nrow = nt * 16 + lg * 4;
  if (gridDim.y == 1) {
    const f32x4 sc = *reinterpret_cast<const f32x4*>(sinv + nrow);
    bf16* y = static_cast<bf16*>(Y);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mt * 16 + li;
      if (m < M) {
        short4v o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bf16 b = f2bf(acc[mt][r] * sc[r]);
          o[r] = *reinterpret_cast<const short*>(&b);
        }
        *reinterpret_cast<short4v*>(y + (int64_t)m * N + nrow) = o;
      }
    }
  } else {
    float* ws = static_cast<float*>(Y) + (int64_t)sp * M * N;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mt * 16 + li;
      if (m < M)
        *reinterpret_cast<f32x4*>(ws + (int64_t)m * N + nrow) = acc[mt];
    }
  }
}

// One thread per four outputs: the splits added in index order, then the
// scale and the rounding.
__global__ __launch_bounds__(256) void linear_w8_merge_kernel(
    const float* __restrict__ ws, const float* __restrict__ sinv,
    bf16* __restrict__ Y, int64_t MN4, int N4, int ksplit) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN4) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(ws) + i;
  f32x4 a = p[0];
  for (int s = 1; s < ksplit; ++s) a += p[(int64_t)s * MN4];
  const f32x4 sc = reinterpret_cast<const f32x4*>(sinv)[i % N4];
  short4v o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bf16 b = f2bf(a[r] * sc[r]);
    o[r] = *reinterpret_cast<const short*>(&b);
  }
  reinterpret_cast<short4v*>(Y)[i] = o;
}

template <int MT>
static void launch_w8(hipStream_t stream, const void* X, const void* W8,
                      const void* sinv, void* out, int M, int N, int K,
                      int ksplit) {
  hipLaunchKernelGGL((linear_w8_kernel<MT>), dim3(N / LW_ROWS, ksplit),
                     dim3(LW_THREADS), 0, stream, (const bf16*)X,
                     (const unsigned char*)W8, (const float*)sinv, out, M, N, K,
                     K / LW_CHUNK / ksplit);
}

// X bf16 [M,K], W8 pre-shuffled bytes, sinv fp32 [N], Y bf16 [M,N].
// ws: fp32 [ksplit,M,N], caller-provided, unused (may be null) when ksplit
// == 1. ksplit divides K/256 and depends on the launch shape only.
PRIME_API int prime_linear_w8(hipStream_t stream, const void* X,
                              const void* W8, const void* sinv, void* Y,
                              void* ws, int64_t M, int64_t N, int64_t K,
                              int64_t ksplit) {
  if (!X || !W8 || !sinv || !Y || M < 1 || M > 64 || N < LW_ROWS ||
      N % LW_ROWS != 0 || K < LW_CHUNK || K % LW_CHUNK != 0 || ksplit < 1 ||
      ksplit > 65535 || (K / LW_CHUNK) % ksplit != 0 || (ksplit > 1 && !ws) ||
      N > 0x7fffffff || K > 0x7fffffff)
    return hipErrorInvalidValue;
  void* out = ksplit == 1 ? Y : ws;
  switch ((int)((M + 15) / 16)) {
    case 1: launch_w8<1>(stream, X, W8, sinv, out, (int)M, (int)N, (int)K, (int)ksplit); break;
    case 2: launch_w8<2>(stream, X, W8, sinv, out, (int)M, (int)N, (int)K, (int)ksplit); break;
    case 3: launch_w8<3>(stream, X, W8, sinv, out, (int)M, (int)N, (int)K, (int)ksplit); break;
    default: launch_w8<4>(stream, X, W8, sinv, out, (int)M, (int)N, (int)K, (int)ksplit); break;
  }
  if (ksplit > 1) {
    const int64_t mn4 = M * N / 4;
    hipLaunchKernelGGL(linear_w8_merge_kernel, dim3((int)((mn4 + 255) / 256)),
                       dim3(256), 0, stream, (const float*)ws,
                       (const float*)sinv, (bf16*)Y, mn4, (int)(N / 4),
                       (int)ksplit);
  }
  return (int)hipGetLastError();
}
