// NHWC weight-gradient (wgrad) kernel on MFMA for gfx950.
//
// Generic form covering conv wgrad AND ConvTranspose wgrad (roles swapped):
//   dW[b, r, s, a] = sum_{n,ho,wo} Y[n,ho,wo,b] * X[n, ho*ST-P+r, wo*ST-P+s, a]
// For conv: Y = grad_out, X = input, dW is the (K,R,S,C)-physical weight grad.
// For convT: Y = input, X = grad_out (the larger map), giving the
// (Ci,R,S,Co)-physical transposed-conv weight grad.
//
// GEMM view per (r,s): (B x A) = Y^T @ X_patch, reduced over all N*HO*WO
// pixels — a huge-K GEMM, split over pixel slabs (grid.z). Every slab STORES
// its fp32 partial into its own workspace plane (no atomics, no pre-zeroing)
// and a combine kernel sums the planes in a fixed order, so the result is
// bitwise-deterministic at any split factor.
//
// Both operands are pixel-major in memory (NHWC), so global loads are
// contiguous 16B channel runs and staging writes are single ds_write_b128s
// into [pix/4][ch/16][4][16] subtiles; the transpose to reduction-axis
// fragments happens IN HARDWARE via ds_read_b64_tr_b16 (gfx950's LDS
// transpose read: a 16-lane group reads one 128-byte [4pix][16ch] block and
// lane c receives column c — semantics pinned by tests/test_tr16_gpu.py).

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PCH = 64;    // pixels per staging chunk
constexpr int THREADS = 256;

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// [pix/4][BT/16][4][16] subtiled LDS image: byte offset of element (pix, ch)
template <int BT>
__device__ __forceinline__ int sub_off(int pix, int ch) {
  return ((pix >> 2) * (BT / 16) + (ch >> 4)) * 128 + (pix & 3) * 32 +
         (ch & 15) * 2;
}

// issue one pair of hardware transpose reads (no wait) for the 8-pixel-run
// fragment of a fixed channel: lane l covers ch (..&15 == l&15), pix pe..pe+7
__device__ __forceinline__ void tr16_issue(const char* tile, int ch, int pe,
                                           int lane, int bt_over_16,
                                           u16x4& lo, u16x4& hi) {
  const unsigned a0 =
      (unsigned)(unsigned long long)tile +
      (unsigned)(((pe >> 2) * bt_over_16 + (ch >> 4)) * 128 + (lane & 15) * 8);
  const unsigned a1 = a0 + (unsigned)(bt_over_16 * 128);
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(a1));
}

__device__ __forceinline__ bf16x8 tr16_combine(u16x4 lo, u16x4 hi) {
  typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
  u16x8 r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, r);
}

// BTB/BTA: channel tiles per side (64 or 128, independent); wave tile
// (BTB/2 x BTA/2), (BTB/32 x BTA/32) fragments per wave.
// yring > 0: Y is physically (N, HO+2r, WO+2r, B) with the logical content
// in the interior — pixel indices stay over the logical HOxWO grid so no
// FLOPs are spent on the ring.
template <int BTB, int BTA>
__global__ __launch_bounds__(THREADS) void conv2d_wgrad_kernel(
    const __bf16* __restrict__ Y,  // (N, HO, WO, B) (+ ring, see above)
    const __bf16* __restrict__ X,  // (N, H, W, A)
    float* __restrict__ ws,        // (sp, B, R, S, A) fp32 slab stores
    int Nb, int HO, int WO, int B, int H, int W, int A, int R, int S,
    int STRIDE, int PAD, int p_per_slab, int yring) {
  __shared__ __align__(16) char lds[PCH * (BTB + BTA) * 2];
  char* yt = lds;                        // [PCH/4][BTB/16][4][16] subtiles
  char* xt = lds + PCH * BTB * 2;        // [PCH/4][BTA/16][4][16] subtiles

  const int at_blocks = (A + BTA - 1) / BTA;
  const int b0 = (blockIdx.x / at_blocks) * BTB;
  const int a0 = (blockIdx.x % at_blocks) * BTA;
  const int r = blockIdx.y / S;
  const int s = blockIdx.y % S;
  const int p_begin = blockIdx.z * p_per_slab;
  const int p_total = Nb * HO * WO;
  const int p_end = min(p_begin + p_per_slab, p_total);

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  constexpr int FRB = BTB / 32;
  constexpr int FRA = BTA / 32;
  const int wm = (wid >> 1) * (BTB / 2);   // wave row (b) base
  const int wn = (wid & 1) * (BTA / 2);    // wave col (a) base

  f32x4 acc[FRB][FRA];
#pragma unroll
  for (int i = 0; i < FRB; ++i)
#pragma unroll
    for (int j = 0; j < FRA; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int SLY = (PCH * BTB / 8) / THREADS;  // Y staging slots/thread
  constexpr int SLX = (PCH * BTA / 8) / THREADS;  // X staging slots/thread
  bf16x8 yreg[SLY], xreg[SLX];

  // T14 pipeline: issue chunk t+1's global loads, MFMA chunk t from LDS,
  // write t+1 after the barrier. Pixel meta is computed inline per staging
  // slot (few int divides, hidden under the loads).
  const int HOp = HO + 2 * yring;
  const int WOp = WO + 2 * yring;
  auto load_chunk = [&](int p0) {
#pragma unroll
    for (int it = 0; it < SLY; ++it) {
      const int slot = it * THREADS + tid;
      const int pix_l = slot / (BTB / 8);
      const int ch0 = (slot % (BTB / 8)) * 8;
      const int pix = p0 + pix_l;
      bf16x8 vy = {};
      if (pix < p_end && b0 + ch0 < B) {
        long yoff = (long)pix * B;
        if (yring > 0) {
          const int n = pix / (HO * WO);
          const int rem = pix - n * (HO * WO);
          const int ho = rem / WO;
          const int wo = rem - ho * WO;
          yoff = (((long)n * HOp + ho + yring) * WOp + wo + yring) * B;
        }
        const __bf16* src = Y + yoff + b0 + ch0;
        if (b0 + ch0 + 8 <= B) {
          vy = *reinterpret_cast<const bf16x8*>(src);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (b0 + ch0 + j < B) vy[j] = src[j];
        }
      }
      yreg[it] = vy;
    }
#pragma unroll
    for (int it = 0; it < SLX; ++it) {
      const int slot = it * THREADS + tid;
      const int pix_l = slot / (BTA / 8);
      const int ch0 = (slot % (BTA / 8)) * 8;
      const int pix = p0 + pix_l;
      bf16x8 vx = {};
      if (pix < p_end) {
        const int n = pix / (HO * WO);
        const int rem = pix - n * (HO * WO);
        const int ho = rem / WO;
        const int wo = rem - ho * WO;
        const int hi = ho * STRIDE - PAD + r;
        const int wi = wo * STRIDE - PAD + s;
        if (hi >= 0 && hi < H && wi >= 0 && wi < W && a0 + ch0 < A) {
          const __bf16* src =
              X + ((long)n * H * W + (long)hi * W + wi) * A + a0 + ch0;
          if (a0 + ch0 + 8 <= A) {
            vx = *reinterpret_cast<const bf16x8*>(src);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (a0 + ch0 + j < A) vx[j] = src[j];
          }
        }
      }
      xreg[it] = vx;
    }
  };

  auto write_chunk = [&]() {
#pragma unroll
    for (int it = 0; it < SLY; ++it) {
      const int slot = it * THREADS + tid;
      const int pix_l = slot / (BTB / 8);
      const int ch0 = (slot % (BTB / 8)) * 8;
      *reinterpret_cast<bf16x8*>(yt + sub_off<BTB>(pix_l, ch0)) = yreg[it];
    }
#pragma unroll
    for (int it = 0; it < SLX; ++it) {
      const int slot = it * THREADS + tid;
      const int pix_l = slot / (BTA / 8);
      const int ch0 = (slot % (BTA / 8)) * 8;
      *reinterpret_cast<bf16x8*>(xt + sub_off<BTA>(pix_l, ch0)) = xreg[it];
    }
  };

  const int nchunks = (p_end - p_begin + PCH - 1) / PCH;
  if (nchunks > 0) {
    load_chunk(p_begin);
    write_chunk();
    if (nchunks > 1) load_chunk(p_begin + PCH);
    __syncthreads();
  }

  for (int t = 0; t < nchunks; ++t) {
    // MFMA: 2 K-steps of 32 pixels
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int pe = kk * 32 + (lane >> 4) * 8;   // pixel base (8-aligned)
      u16x4 alo[FRB], ahi[FRB], blo[FRA], bhi[FRA];
#pragma unroll
      for (int f = 0; f < FRB; ++f)
        tr16_issue(yt, wm + f * 16 + (lane & 15), pe, lane, BTB / 16, alo[f],
                   ahi[f]);
#pragma unroll
      for (int f = 0; f < FRA; ++f)
        tr16_issue(xt, wn + f * 16 + (lane & 15), pe, lane, BTA / 16, blo[f],
                   bhi[f]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 a_frag[FRB], b_frag[FRA];
#pragma unroll
      for (int f = 0; f < FRB; ++f) a_frag[f] = tr16_combine(alo[f], ahi[f]);
#pragma unroll
      for (int f = 0; f < FRA; ++f) b_frag[f] = tr16_combine(blo[f], bhi[f]);
#pragma unroll
      for (int i = 0; i < FRB; ++i)
#pragma unroll
        for (int j = 0; j < FRA; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
    }
    if (t + 1 < nchunks) {
      __syncthreads();
      write_chunk();
      if (t + 2 < nchunks) load_chunk(p_begin + (t + 2) * PCH);
      __syncthreads();
    }
  }

  // epilogue: STORE this slab's partial into its own workspace plane —
  // every (b,r,s,a) element is written by exactly one block per slab, so
  // there are no atomics and no pre-zeroing, and the serial slab walk in
  // wgrad_combine makes the weight gradient bitwise-deterministic at any
  // split factor.
  float* slab = ws + (long)blockIdx.z * B * R * S * A;
#pragma unroll
  for (int j = 0; j < FRA; ++j) {
    const int a = a0 + wn + j * 16 + (lane & 15);
    if (a >= A) continue;
#pragma unroll
    for (int i = 0; i < FRB; ++i) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int b = b0 + wm + i * 16 + (lane >> 4) * 4 + v;
        if (b < B) {
          slab[(((long)b * R + r) * S + s) * A + a] = acc[i][j][v];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// glds-staged wgrad (round 2): for the padded-operand case (PAD==0, every X
// gather in-bounds, Y interior-mapped) staging runs on global_load_lds
// straight into the SAME [pix/4][ch/16][4][16] subtiled images the tr16
// transpose reads consume — the per-lane source address realizes the image
// permutation (16B of one pixel's 8 channels is contiguous in both). Three
// LDS buffers, counted vmcnt, raw barriers (same pipeline as
// conv2d_glds.hip); a ragged tail chunk falls back to masked register
// staging. Pixel decode is shift-only (dispatch gated on power-of-two
// interior HO/WO — every training shape qualifies).

template <int N>
__device__ __forceinline__ void wwaitcnt_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void wbarrier_mem() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ void wglds16(const __bf16* g, char* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)g,
      (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// per-(wave, call, lane) fixed image coordinates: 16B unit index scall ->
// subtiled-image (pix, ch0); every glds-staged side shares the decode
// (BT/16 via shift)
__device__ __forceinline__ void glds_decode(int scall, int bt16_sh, int& pix,
                                            int& ch0) {
  const int sidx = scall >> 3;
  const int inner = scall & 7;
  pix = ((sidx >> bt16_sh) << 2) + (inner >> 1);
  ch0 = ((sidx & ((1 << bt16_sh) - 1)) << 4) + ((inner & 1) << 3);
}

template <int BTB, int BTA>
__global__ __launch_bounds__(THREADS) void conv2d_wgrad_glds_kernel(
    const __bf16* __restrict__ Y, const __bf16* __restrict__ X,
    float* __restrict__ ws, int Nb, int HO, int WO, int B, int H, int W,
    int A, int R, int S, int STRIDE, int p_per_slab, int yring,
    int howo_sh, int wo_sh, const __bf16* __restrict__ X2, int A1) {
  extern __shared__ __align__(16) char wlds[];
  constexpr int YBYTES = PCH * BTB * 2;
  constexpr int XBYTES = PCH * BTA * 2;
  constexpr int SLAB = YBYTES + XBYTES;

  const int at_blocks = (A + BTA - 1) / BTA;
  const int b0 = (blockIdx.x / at_blocks) * BTB;
  const int a0 = (blockIdx.x % at_blocks) * BTA;
  const int r = blockIdx.y / S;
  const int s = blockIdx.y % S;
  const int p_begin = blockIdx.z * p_per_slab;
  const int p_total = Nb * HO * WO;
  const int p_end = min(p_begin + p_per_slab, p_total);

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  constexpr int FRB = BTB / 32;
  constexpr int FRA = BTA / 32;
  const int wm = (wid >> 1) * (BTB / 2);
  const int wn = (wid & 1) * (BTA / 2);
  const int HOp = HO + 2 * yring;
  const int WOp = WO + 2 * yring;

  f32x4 acc[FRB][FRA];
#pragma unroll
  for (int i = 0; i < FRB; ++i)
#pragma unroll
    for (int j = 0; j < FRA; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int YC = YBYTES / 4096;          // glds calls per wave (Y)
  constexpr int XC = XBYTES / 4096;
  constexpr int G = YC + XC;

  constexpr int ybt_sh = BTB == 128 ? 3 : 2;
  constexpr int xbt_sh = BTA == 128 ? 3 : 2;

  auto stage = [&](int p0, int buf) {
    char* yimg = wlds + buf * SLAB;
    char* ximg = yimg + YBYTES;
#pragma unroll
    for (int i = 0; i < YC; ++i) {
      int pixl, ch0;
      glds_decode((wid * YC + i) * 64 + lane, ybt_sh, pixl, ch0);
      const int pix = p0 + pixl;
      const int n = pix >> howo_sh;
      const int rem = pix - (n << howo_sh);
      const int ho = rem >> wo_sh;
      const int wo = rem - (ho << wo_sh);
      const long yoff =
          (((long)n * HOp + ho + yring) * WOp + wo + yring) * B + b0 + ch0;
      wglds16(Y + yoff, yimg + (wid * YC + i) * 1024);
    }
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      int pixl, ch0;
      glds_decode((wid * XC + i) * 64 + lane, xbt_sh, pixl, ch0);
      const int pix = p0 + pixl;
      const int n = pix >> howo_sh;
      const int rem = pix - (n << howo_sh);
      const int ho = rem >> wo_sh;
      const int wo = rem - (ho << wo_sh);
      const int hi = ho * STRIDE + r;     // PAD == 0, in-bounds by contract
      const int wi = wo * STRIDE + s;
      // dual-X (skip-concat elimination): channel picks the source tensor
      const int ach = a0 + ch0;
      const bool second = X2 != nullptr && ach >= A1;
      const __bf16* xsrc = second ? X2 : X;
      const int as = X2 == nullptr ? A : (second ? A - A1 : A1);
      const int al = second ? ach - A1 : ach;
      const long xoff = ((long)n * H * W + (long)hi * W + wi) * as + al;
      wglds16(xsrc + xoff, ximg + (wid * XC + i) * 1024);
    }
  };

  auto mfma_image = [&](const char* yimg, const char* ximg) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int pe = kk * 32 + (lane >> 4) * 8;
      u16x4 alo[FRB], ahi[FRB], blo[FRA], bhi[FRA];
#pragma unroll
      for (int f = 0; f < FRB; ++f)
        tr16_issue(yimg, wm + f * 16 + (lane & 15), pe, lane, BTB / 16,
                   alo[f], ahi[f]);
#pragma unroll
      for (int f = 0; f < FRA; ++f)
        tr16_issue(ximg, wn + f * 16 + (lane & 15), pe, lane, BTA / 16,
                   blo[f], bhi[f]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 a_frag[FRB], b_frag[FRA];
#pragma unroll
      for (int f = 0; f < FRB; ++f) a_frag[f] = tr16_combine(alo[f], ahi[f]);
#pragma unroll
      for (int f = 0; f < FRA; ++f) b_frag[f] = tr16_combine(blo[f], bhi[f]);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < FRB; ++i)
#pragma unroll
        for (int j = 0; j < FRA; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  const int nfull = (p_end - p_begin) / PCH;
  const int tail = (p_end - p_begin) - nfull * PCH;

  if (nfull > 0) stage(p_begin, 0);
  if (nfull > 1) stage(p_begin + PCH, 1);
  if (nfull > 2) stage(p_begin + 2 * PCH, 2);

  for (int t = 0; t < nfull; ++t) {
    const int buf = t % 3;
    // wait until chunk t's own glds completed: with fewer than 3 chunks
    // staged ahead, vmcnt(2G) would pass while chunk t is still in flight
    const int ahead = min(nfull, t + 3) - 1 - t;
    if (ahead >= 2) wwaitcnt_vm<2 * G>();
    else if (ahead == 1) wwaitcnt_vm<G>();
    else wwaitcnt_vm<0>();
    wbarrier_mem();
    mfma_image(wlds + buf * SLAB, wlds + buf * SLAB + YBYTES);
    wbarrier_mem();
    if (t + 3 < nfull) stage(p_begin + (t + 3) * PCH, buf);
  }

  if (tail > 0) {
    // ragged last chunk: masked register staging into buffer 0
    wwaitcnt_vm<0>();
    __syncthreads();
    char* yimg = wlds;
    char* ximg = wlds + YBYTES;
    const int p0 = p_begin + nfull * PCH;
    constexpr int SLY = (PCH * BTB / 8) / THREADS;
    constexpr int SLX = (PCH * BTA / 8) / THREADS;
#pragma unroll
    for (int it = 0; it < SLY; ++it) {
      const int slot = it * THREADS + tid;
      const int pixl = slot / (BTB / 8);
      const int ch0 = (slot % (BTB / 8)) * 8;
      bf16x8 vy = {};
      const int pix = p0 + pixl;
      if (pixl < tail) {
        const int n = pix >> howo_sh;
        const int rem = pix - (n << howo_sh);
        const int ho = rem >> wo_sh;
        const int wo = rem - (ho << wo_sh);
        vy = *reinterpret_cast<const bf16x8*>(
            Y + (((long)n * HOp + ho + yring) * WOp + wo + yring) * B + b0 +
            ch0);
      }
      *reinterpret_cast<bf16x8*>(yimg + sub_off<BTB>(pixl, ch0)) = vy;
    }
#pragma unroll
    for (int it = 0; it < SLX; ++it) {
      const int slot = it * THREADS + tid;
      const int pixl = slot / (BTA / 8);
      const int ch0 = (slot % (BTA / 8)) * 8;
      bf16x8 vx = {};
      const int pix = p0 + pixl;
      if (pixl < tail) {
        const int n = pix >> howo_sh;
        const int rem = pix - (n << howo_sh);
        const int ho = rem >> wo_sh;
        const int wo = rem - (ho << wo_sh);
        const int hi = ho * STRIDE + r;
        const int wi = wo * STRIDE + s;
        const int ach = a0 + ch0;
        const bool second = X2 != nullptr && ach >= A1;
        const __bf16* xsrc = second ? X2 : X;
        const int as = X2 == nullptr ? A : (second ? A - A1 : A1);
        const int al = second ? ach - A1 : ach;
        vx = *reinterpret_cast<const bf16x8*>(
            xsrc + ((long)n * H * W + (long)hi * W + wi) * as + al);
      }
      *reinterpret_cast<bf16x8*>(ximg + sub_off<BTA>(pixl, ch0)) = vx;
    }
    __syncthreads();
    mfma_image(yimg, ximg);
  }

  float* slab = ws + (long)blockIdx.z * B * R * S * A;
#pragma unroll
  for (int j = 0; j < FRA; ++j) {
    const int a = a0 + wn + j * 16 + (lane & 15);
    if (a >= A) continue;
#pragma unroll
    for (int i = 0; i < FRB; ++i) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int b = b0 + wm + i * 16 + (lane >> 4) * 4 + v;
        if (b < B) {
          slab[(((long)b * R + r) * S + s) * A + a] = acc[i][j][v];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Thin-channel wgrad (first encoder conv / last decoder ConvT: A = 1..3).
// The taps are folded into the thin channel axis, so the whole weight
// gradient is ONE GEMM and one pass over Y serves every tap:
//   dW[b, q] = sum_pix Y[pix, b] * Xcol[pix, q],   q = (r*S + s)*A + a < 32
//   Xcol[pix, q] = X[n, ho*ST-PAD+r, wo*ST-PAD+s, a]  (0 out of bounds)
// q is the inner index of the (B,R,S,A) layout: the slab store is
// slab[b*R*S*A + q].
//
// Y side: the glds 3-buffer pipeline of conv2d_wgrad_glds_kernel<64,.>.
// Xcol side: 64 pixels x 32 columns per chunk = 256 slots of (pixel, 8
// consecutive q), one per thread. The thread's eight (r,s,a) triples are
// decoded once; per chunk it issues eight 2-byte buffer loads whose hardware
// range check returns 0 for the out-of-bounds offset we hand to masked
// taps, packs them and writes one 16-byte LDS store into the subtiled image.
//
// vmcnt accounting. The gathers are inline asm so the compiler neither
// drains the glds queue for them nor reorders them; loads retire in order,
// and every iteration issues, in this order,
//   Xg(t+2) [TXG ops, always — a chunk past the end gathers zeros]
//   Ys(t+3) [TYC ops, only if the chunk exists]
// One counted wait per iteration, taken just before X(t+1) is written to
// LDS, retires Ys(t+1) and Xg(t+1) and leaves what was issued after them
// outstanding: [Ys(t+2)], Xg(t+2), [Ys(t+3)] = TXG + TYC*[..] + TYC*[..].

constexpr int TQ = 32;                 // padded tap*channel columns
constexpr int TYBYTES = PCH * 64 * 2;  // Y image per chunk
constexpr int TXBYTES = PCH * TQ * 2;  // Xcol image per chunk
constexpr int TSLAB = TYBYTES + TXBYTES;
constexpr int TYC = TYBYTES / 4096;    // glds calls per wave per chunk
constexpr int TXG = 8;                 // gather loads per thread per chunk

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct XRegs {
  unsigned v[TXG];
};

// wait until at most N vector-memory ops are outstanding; naming the gather
// registers read-write keeps every consumer of them behind the wait
template <int N>
__device__ __forceinline__ void thin_wait(XRegs& x) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(x.v[0]), "+v"(x.v[1]), "+v"(x.v[2]), "+v"(x.v[3]),
                 "+v"(x.v[4]), "+v"(x.v[5]), "+v"(x.v[6]), "+v"(x.v[7])
               : "n"(N)
               : "memory");
}

// retire a chunk that has `later` chunks behind it: leave outstanding the
// TXG gather ops and the Y stages of up to two later chunks that were issued
// after it (see the accounting above). The three-way choice lives INSIDE
// one statement: a branch in C++ lets the compiler copy the still-landing
// gather registers on the way to the wait.
__device__ __forceinline__ void thin_retire(int later, XRegs& x) {
  static_assert(TXG + 2 * TYC == 12 && TXG + TYC == 10 && TXG == 8,
                "wait constants below are spelled out");
  asm volatile(
      "s_cmp_ge_i32 %8, 2\n\t"
      "s_cbranch_scc0 .Lthin_w1_%=\n\t"
      "s_waitcnt vmcnt(12)\n\t"
      "s_branch .Lthin_wd_%=\n"
      ".Lthin_w1_%=:\n\t"
      "s_cmp_eq_u32 %8, 1\n\t"
      "s_cbranch_scc0 .Lthin_w0_%=\n\t"
      "s_waitcnt vmcnt(10)\n\t"
      "s_branch .Lthin_wd_%=\n"
      ".Lthin_w0_%=:\n\t"
      "s_waitcnt vmcnt(8)\n"
      ".Lthin_wd_%=:"
      : "+v"(x.v[0]), "+v"(x.v[1]), "+v"(x.v[2]), "+v"(x.v[3]),
        "+v"(x.v[4]), "+v"(x.v[5]), "+v"(x.v[6]), "+v"(x.v[7])
      : "s"(__builtin_amdgcn_readfirstlane(later))
      : "memory", "scc");
}

__global__ __launch_bounds__(THREADS) void conv2d_wgrad_thin_kernel(
    const __bf16* __restrict__ Y, const __bf16* __restrict__ X,
    float* __restrict__ ws, int Nb, int HO, int WO, int B, int H, int W,
    int A, int R, int S, int STRIDE, int PAD, int p_per_slab, int yring,
    int howo_sh, int wo_sh, int xbytes) {
  __shared__ __align__(16) char tlds[3 * TSLAB];

  const int b0 = blockIdx.x * 64;
  const int p_begin = blockIdx.z * p_per_slab;
  const int p_total = Nb * HO * WO;
  const int p_end = min(p_begin + p_per_slab, p_total);
  const int RSA = R * S * A;

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int HOp = HO + 2 * yring;
  const int WOp = WO + 2 * yring;

  // wave w owns b rows [16w, 16w+16) x all 32 columns: 1 x 2 fragments
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};

  // raw buffer over X: an offset >= xbytes reads as 0
  const unsigned long long xaddr = (unsigned long long)X;
  const i32x4 xrsrc = {(int)(unsigned)xaddr, (int)((xaddr >> 32) & 0xffffu),
                       xbytes, 0x00020000};
  constexpr unsigned XOOB = 0x80000000u;

  // this thread's Xcol slot: pixel tid/4 of the chunk, columns q0..q0+7
  const int xpix = tid >> 2;
  const int q0 = (tid & 3) * 8;
  int xdh[TXG], xdw[TXG], xoff[TXG];
#pragma unroll
  for (int j = 0; j < TXG; ++j) {
    const int q = q0 + j;
    const int rs = q / A;
    const int a = q - rs * A;
    const int r = rs / S;
    const int s = rs - r * S;
    // a padding column never passes the row bound check
    xdh[j] = q < RSA ? r - PAD : -(1 << 24);
    xdw[j] = s - PAD;
    xoff[j] = ((r - PAD) * W + (s - PAD)) * A + a;
  }
  const unsigned xlds =
      (unsigned)(unsigned long long)tlds + TYBYTES + sub_off<TQ>(xpix, q0);

  auto pix_decode = [&](int pix, int& n, int& ho, int& wo) {
    n = pix >> howo_sh;
    const int rem = pix - (n << howo_sh);
    ho = rem >> wo_sh;
    wo = rem - (ho << wo_sh);
  };

  // TXG range-checked 2-byte loads, always issued; !live gathers zeros
  auto gather = [&](int p0, bool live, XRegs& x) {
    int n, ho, wo;
    pix_decode(p0 + xpix, n, ho, wo);
    const int hi0 = ho * STRIDE;
    const int wi0 = wo * STRIDE;
    const int base = ((n * H + hi0) * W + wi0) * A;
#pragma unroll
    for (int j = 0; j < TXG; ++j) {
      const bool ok = live && (unsigned)(hi0 + xdh[j]) < (unsigned)H &&
                      (unsigned)(wi0 + xdw[j]) < (unsigned)W;
      const unsigned voff = ok ? (unsigned)(base + xoff[j]) * 2u : XOOB;
      asm volatile("buffer_load_ushort %0, %1, %2, 0 offen"
                   : "=v"(x.v[j])
                   : "v"(voff), "s"(xrsrc)
                   : "memory");
    }
  };

  auto write_x = [&](int buf, const XRegs& x) {
    const u32x4 w = {x.v[0] | (x.v[1] << 16), x.v[2] | (x.v[3] << 16),
                     x.v[4] | (x.v[5] << 16), x.v[6] | (x.v[7] << 16)};
    asm volatile("ds_write_b128 %0, %1" ::"v"(xlds + buf * TSLAB), "v"(w)
                 : "memory");
  };

  auto stage_y = [&](int p0, int buf) {
    char* yimg = tlds + buf * TSLAB;
#pragma unroll
    for (int i = 0; i < TYC; ++i) {
      int pixl, ch0, n, ho, wo;
      glds_decode((wid * TYC + i) * 64 + lane, 2, pixl, ch0);
      pix_decode(p0 + pixl, n, ho, wo);
      const long yoff =
          (((long)n * HOp + ho + yring) * WOp + wo + yring) * B + b0 + ch0;
      wglds16(Y + yoff, yimg + (wid * TYC + i) * 1024);
    }
  };

  auto mfma_image = [&](int buf) {
    const char* yimg = tlds + buf * TSLAB;
    const char* ximg = yimg + TYBYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int pe = kk * 32 + (lane >> 4) * 8;
      u16x4 alo, ahi, blo[2], bhi[2];
      tr16_issue(yimg, wid * 16 + (lane & 15), pe, lane, 4, alo, ahi);
#pragma unroll
      for (int f = 0; f < 2; ++f)
        tr16_issue(ximg, f * 16 + (lane & 15), pe, lane, TQ / 16, blo[f],
                   bhi[f]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8 a_frag = tr16_combine(alo, ahi);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag, tr16_combine(blo[j], bhi[j]), acc[j], 0, 0, 0);
    }
  };

  const int nfull = (p_end - p_begin) / PCH;
  const int tail = (p_end - p_begin) - nfull * PCH;

  // retire chunk c: its Y glds and its gather have landed after this
  auto retire = [&](int c, XRegs& x) { thin_retire(nfull - 1 - c, x); };

  XRegs xa, xb;
  // iteration t: `cur` holds Xg(t+1) in flight, `nxt` receives Xg(t+2)
  auto step = [&](int t, XRegs& cur, XRegs& nxt) {
    const int buf = t % 3;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // X(t) is in LDS
    wbarrier_mem();
    mfma_image(buf);
    wbarrier_mem();
    gather(p_begin + (t + 2) * PCH, t + 2 < nfull, nxt);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 3 < nfull) stage_y(p_begin + (t + 3) * PCH, buf);
    __builtin_amdgcn_sched_barrier(0);
    retire(t + 1, cur);
    write_x((t + 1) % 3, cur);
  };

  if (nfull > 0) {
    gather(p_begin, true, xb);
    __builtin_amdgcn_sched_barrier(0);
    stage_y(p_begin, 0);
    if (nfull > 1) stage_y(p_begin + PCH, 1);
    __builtin_amdgcn_sched_barrier(0);
    gather(p_begin + PCH, nfull > 1, xa);
    __builtin_amdgcn_sched_barrier(0);
    if (nfull > 2) stage_y(p_begin + 2 * PCH, 2);
    __builtin_amdgcn_sched_barrier(0);
    retire(0, xb);
    write_x(0, xb);
    for (int t = 0; t < nfull; t += 2) {
      step(t, xa, xb);
      if (t + 1 >= nfull) break;
      step(t + 1, xb, xa);
    }
    // the last (zero) gathers are still landing in xa/xb
    thin_wait<0>(xa);
    thin_wait<0>(xb);
  }

  if (tail > 0) {
    // ragged last chunk: masked register staging into buffer 0
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    const int p0 = p_begin + nfull * PCH;
    gather(p0, xpix < tail, xa);
    constexpr int SLY = (PCH * 64 / 8) / THREADS;
#pragma unroll
    for (int it = 0; it < SLY; ++it) {
      const int slot = it * THREADS + tid;
      const int pixl = slot >> 3;
      const int ch0 = (slot & 7) * 8;
      bf16x8 vy = {};
      if (pixl < tail) {
        int n, ho, wo;
        pix_decode(p0 + pixl, n, ho, wo);
        vy = *reinterpret_cast<const bf16x8*>(
            Y + (((long)n * HOp + ho + yring) * WOp + wo + yring) * B + b0 +
            ch0);
      }
      *reinterpret_cast<bf16x8*>(tlds + sub_off<64>(pixl, ch0)) = vy;
    }
    thin_wait<0>(xa);
    write_x(0, xa);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    mfma_image(0);
  }

  float* slab = ws + (long)blockIdx.z * B * RSA;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = j * 16 + (lane & 15);
    if (q >= RSA) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int b = b0 + wid * 16 + (lane >> 4) * 4 + v;
      slab[(long)b * RSA + q] = acc[j][v];
    }
  }
}

// ---------------------------------------------------------------------------
// Single-pass 3x3 wgrad: all nine taps from one staged read of Y and X.
// (stride 1, PAD == 0 over a zero-ringed X, B and A multiples of 64.)
//
// One block owns a 64(b) x 64(a) weight tile for ALL nine taps (grid.x walks
// the tiles, grid.z the pixel slabs). The pixel axis is cut into 32-column
// strips of the output map; a chunk is two output rows of one strip (64
// pixels, two 32-pixel MFMA K-steps), so every map width >= 32 runs the same
// code: 32 -> one strip, 64 -> two, 128 -> four.
//
// X side: each input row of the strip is staged ONCE as three column-shifted
// [32 pix][64 ch] subtiled images (global_load_lds takes a per-lane source
// address, so image s simply reads X[hi][wo0 + pix + s]). Tap (r,s) of
// output row ho is then the plain aligned tr16 read of image s of input row
// ho + r. The row images live in a ring of TP_NR slots: a chunk needs four
// input rows, of which two were staged by the chunk before it, so advancing
// a chunk stages two rows (6 images) and one 64-pixel Y image: 8 KB + 24 KB
// against 9 x 16 KB for the per-tap kernel. The ring restarts (four rows)
// at the first chunk of a slab and of every (image, strip) segment.
//
// Ring size: when chunk k is staged, chunk k-2 has not been computed (4
// rows) and chunk k-1 is in flight; at most one of k-1, k is a restart:
// 4 + 2 + 4 = 10 slots, handed out by a running counter.
//
// Pipeline: Y in 3 buffers, one raw barrier per chunk. At the top of
// iteration t only stage(t+1) was issued after stage(t), and a stage is at
// least TP_G glds calls per wave, so vmcnt(TP_G) retires chunk t (it waits
// for a little more than needed when t+1 is a restart).
//
// Waves: 2 x 2 over the tile, each 32(b) x 32(a) x 9 taps = 36 fragments
// (144 accumulator registers). Per K-step a wave reads 2 Y fragments once
// and 18 X fragments: 40 transpose reads for 36 MFMAs.

constexpr int TPW = 32;                      // strip width, pixels per row image
constexpr int TP_IMG = TPW * 64 * 2;         // one shifted row image, 4 KB
constexpr int TP_ROW = 3 * TP_IMG;           // the three shifts of one row
constexpr int TP_NR = 10;                    // row ring slots
constexpr int TP_Y = PCH * 64 * 2;           // Y image of one chunk, 8 KB
constexpr int TP_LDS = TP_NR * TP_ROW + 3 * TP_Y;  // 144 KB
constexpr int TP_G = 2 * 3 + 2;              // glds calls/wave, steady chunk

template <int OFF>
__device__ __forceinline__ void tr16_issue_at(unsigned addr, u16x4& lo,
                                              u16x4& hi) {
  // the pair of tr16_issue, as immediates off a per-lane base: second half of
  // the 8-pixel run is the next pixel-group row of the 64-channel image
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(lo)
               : "v"(addr), "n"(OFF));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(hi)
               : "v"(addr), "n"(OFF + 4 * 128));
}

// wait until at most N LDS reads are outstanding; naming the fragment
// registers read-write keeps their consumers behind the wait
template <int N>
__device__ __forceinline__ void taps_wait(u16x4& a, u16x4& b, u16x4& c,
                                          u16x4& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d)
               : "n"(N)
               : "memory");
}

__global__ __launch_bounds__(THREADS) void conv2d_wgrad_taps_kernel(
    const __bf16* __restrict__ Y, const __bf16* __restrict__ X,
    const __bf16* __restrict__ X2, float* __restrict__ ws, int HO, int WO,
    int B, int H, int W, int A, int A1, int yring, int nchunks, int cps,
    int seg_sh, int strip_sh) {
  extern __shared__ __align__(16) char plds[];
  char* const ybufs = plds + TP_NR * TP_ROW;

  const int at_blocks = A >> 6;
  const int b0 = (blockIdx.x / at_blocks) * 64;
  const int a0 = (blockIdx.x % at_blocks) * 64;
  const int c_begin = blockIdx.z * cps;
  const int nch = min(c_begin + cps, nchunks) - c_begin;

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int wm = (wid >> 1) * 32;
  const int wn = (wid & 1) * 32;
  const int HOp = HO + 2 * yring;
  const int WOp = WO + 2 * yring;

  // dual-X: the 64-wide a-tile lies wholly in one source (A1 % 64 == 0)
  const bool second = X2 != nullptr && a0 >= A1;
  const __bf16* xsrc = second ? X2 + (a0 - A1) : X + a0;
  const int as = X2 == nullptr ? A : (second ? A - A1 : A1);
  const __bf16* ysrc = Y + b0;

  // per-lane staging offsets (elements), fixed for the whole kernel
  int xl_off[3], yl_off[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = wid * 3 + i;  // 1 KB unit of the 12 KB row: image q/4
    int pixl, ch0;
    glds_decode((q & 3) * 64 + lane, 2, pixl, ch0);
    xl_off[i] = (pixl + (q >> 2)) * as + ch0;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int pixl, ch0;
    glds_decode((wid * 2 + i) * 64 + lane, 2, pixl, ch0);
    yl_off[i] = ((pixl >> 5) * WOp + (pixl & (TPW - 1))) * B + ch0;
  }

  const int seg_mask = (1 << seg_sh) - 1;
  const int strip_mask = (1 << strip_sh) - 1;
  auto restart = [&](int c) { return c == c_begin || (c & seg_mask) == 0; };

  int sctr = 0;  // ring slot the next staged row goes to
  auto stage = [&](int c, int ybuf) {
    const int seg = c >> seg_sh;
    const int n = seg >> strip_sh;
    const int wo0 = (seg & strip_mask) * TPW;
    const int ho0 = (c & seg_mask) * 2;
    const bool fresh = restart(c);
    const int hi0 = fresh ? ho0 : ho0 + 2;
    const int nrows = fresh ? 4 : 2;
    for (int j = 0; j < nrows; ++j) {
      const __bf16* rb = xsrc + ((long)(n * H + hi0 + j) * W + wo0) * as;
      char* l = plds + sctr * TP_ROW + wid * 3 * 1024;
      sctr = sctr + 1 == TP_NR ? 0 : sctr + 1;
#pragma unroll
      for (int i = 0; i < 3; ++i) wglds16(rb + xl_off[i], l + i * 1024);
    }
    const __bf16* yb =
        ysrc + (((long)n * HOp + ho0 + yring) * WOp + wo0 + yring) * B;
    char* l = ybufs + ybuf * TP_Y + wid * 2 * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i) wglds16(yb + yl_off[i], l + i * 1024);
  };

  f32x4 acc[9][2][2];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[tp][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane tr16 base inside a 64-channel image: pixel run (lane>>4)*8,
  // column lane&15 of channel subtile w/16 (fragment f adds 128 B)
  const unsigned lane_rd = (unsigned)((lane >> 4) * 2 * 4 * 128 + (lane & 15) * 8);
  const unsigned yrd = (unsigned)(unsigned long long)ybufs + lane_rd +
                       (unsigned)((wm >> 4) * 128);
  const unsigned xrd = (unsigned)(unsigned long long)plds + lane_rd +
                       (unsigned)((wn >> 4) * 128);

  int cctr = 0;  // ring slot of the first row the next restart chunk reads
  auto compute = [&](int c, int ybuf) {
    const bool fresh = restart(c);
    int slot = fresh ? cctr : (cctr >= 2 ? cctr - 2 : cctr - 2 + TP_NR);
    cctr += fresh ? 4 : 2;
    cctr = cctr >= TP_NR ? cctr - TP_NR : cctr;
    unsigned rowa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rowa[j] = xrd + (unsigned)(slot * TP_ROW);
      slot = slot + 1 == TP_NR ? 0 : slot + 1;
    }
    const unsigned ya = yrd + (unsigned)(ybuf * TP_Y);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      u16x4 ylo[2], yhi[2], xlo[2][2], xhi[2][2];
      // Y image: K-step kk is pixels kk*32.. = pixel-group rows kk*8..
      if (kk == 0) {
        tr16_issue_at<0>(ya, ylo[0], yhi[0]);
        tr16_issue_at<128>(ya, ylo[1], yhi[1]);
      } else {
        tr16_issue_at<8 * 512>(ya, ylo[0], yhi[0]);
        tr16_issue_at<8 * 512 + 128>(ya, ylo[1], yhi[1]);
      }
      tr16_issue_at<0>(rowa[kk], xlo[0][0], xhi[0][0]);
      tr16_issue_at<128>(rowa[kk], xlo[0][1], xhi[0][1]);
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int cur = tp & 1, nxt = cur ^ 1;
        if (tp < 8) {
          // images of tap tp+1: row kk + r, shift s
          const unsigned ra = rowa[kk + (tp + 1) / 3];
          switch ((tp + 1) % 3) {
            case 0:
              tr16_issue_at<0>(ra, xlo[nxt][0], xhi[nxt][0]);
              tr16_issue_at<128>(ra, xlo[nxt][1], xhi[nxt][1]);
              break;
            case 1:
              tr16_issue_at<TP_IMG>(ra, xlo[nxt][0], xhi[nxt][0]);
              tr16_issue_at<TP_IMG + 128>(ra, xlo[nxt][1], xhi[nxt][1]);
              break;
            default:
              tr16_issue_at<2 * TP_IMG>(ra, xlo[nxt][0], xhi[nxt][0]);
              tr16_issue_at<2 * TP_IMG + 128>(ra, xlo[nxt][1], xhi[nxt][1]);
              break;
          }
          if (tp == 0) taps_wait<4>(ylo[0], yhi[0], ylo[1], yhi[1]);
          taps_wait<4>(xlo[cur][0], xhi[cur][0], xlo[cur][1], xhi[cur][1]);
        } else {
          taps_wait<0>(xlo[cur][0], xhi[cur][0], xlo[cur][1], xhi[cur][1]);
        }
        bf16x8 yf[2], xf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          yf[f] = tr16_combine(ylo[f], yhi[f]);
          xf[f] = tr16_combine(xlo[cur][f], xhi[cur][f]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[tp][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                yf[i], xf[j], acc[tp][i][j], 0, 0, 0);
      }
    }
  };

  if (nch > 0) stage(c_begin, 0);
  if (nch > 1) stage(c_begin + 1, 1);
  int ybuf = 0;
  for (int t = 0; t < nch; ++t) {
    if (t + 1 < nch) wwaitcnt_vm<TP_G>();
    else wwaitcnt_vm<0>();
    wbarrier_mem();
    // buffer (t+2)%3 and the slots it takes were last read by chunk t-1
    if (t + 2 < nch) stage(c_begin + t + 2, ybuf >= 1 ? ybuf - 1 : 2);
    compute(c_begin + t, ybuf);
    ybuf = ybuf == 2 ? 0 : ybuf + 1;
  }

  float* slab = ws + (long)blockIdx.z * B * 9 * A;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int a = a0 + wn + j * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int b = b0 + wm + i * 16 + (lane >> 4) * 4 + v;
          slab[((long)b * 9 + tp) * A + a] = acc[tp][i][j][v];
        }
    }
}

// ---------------------------------------------------------------------------
// Row-order all-taps 3x3 wgrad for 64-wide maps: the single-pass kernel above
// with one-row chunks, so that every weight-gradient element is summed in
// exactly the per-tap kernel's order. (stride 1, PAD == 0 over a zero-ringed
// X, WO == 64, B, A1 and A multiples of 64, any yring.)
//
// What fixes the bits. A chunk is 64 consecutive output pixels, which on a
// 64-wide map is one output row; its two MFMA K-steps are columns 0-31 and
// 32-63, lane group lane>>4 holding pixels g*8..g*8+7 of the step; the slabs
// are the per-tap path's (whole rows, because p_per_slab is 64-aligned) and
// each element has one accumulator chain per slab. The tile shape, the wave
// layout and the LDS layout do not enter the sums.
//
// X side: each input row is staged ONCE as three column-shifted
// [64 pix][64 ch] subtiled images (24 KB); tap (r,s) of output row ho is the
// aligned tr16 read of image s of input row ho + r. A chunk needs input rows
// ho..ho+2, two of which the chunks before it staged: in steady state a
// chunk stages one row plus one Y image, 24 KB + 8 KB against 9 x 16 KB.
//
// Segments. The chunks of a slab fall into segments of consecutive rows of
// one image; a segment begins at the slab start and at every image boundary
// and needs three fresh rows there. Each segment runs as a pipeline of its
// own: its first chunk's three rows and Y are staged into ring slots 0..2 /
// Y buffer 0 after a barrier that retires the segment before it, so nothing
// from two segments is ever in flight together. That stall is paid once per
// 64 chunks at most and keeps the ring at RW_NR = 5 slots: at the top of
// iteration t chunk t reads rows t..t+2, chunk t+1's row t+3 is in flight and
// chunk t+2's row t+4 goes to slot (t+4) % 5, which held row t-1, last read
// by chunk t-1 before the barrier. Y rotates through 3 buffers the same way.
//
// vmcnt. Within a segment a wave issues, in this order,
//   S(0) = 3 * RW_XC + YC calls, S(1) = G, [wait_0] S(2) = G, [wait_1] ...
// with G = RW_XC + YC for every chunk but the first. At wait_t the calls
// issued after S(t) are exactly S(t+1) when chunk t+1 exists (S(t+2) follows
// the wait), so vmcnt(G) retires S(t), whatever S(t) itself counted; on the
// segment's last chunk nothing follows and the wait is vmcnt(0). A segment
// therefore ends with no loads outstanding and the next starts from zero:
// there is no steady-after-restart or restart-after-steady mix to count.
//
// Tiles: BTB = 64 is the 64(b) x 64(a) tile of the strip kernel (waves 2 x 2,
// 36 fragments each); BTB = 32 halves the tile in b (waves 1 x 4, each
// 32(b) x 16(a) x 9 taps = 18 fragments) and doubles the blocks for layers
// whose slabs alone do not fill the CUs.

constexpr int RW = 64;                 // map width = pixels per row image
constexpr int RW_IMG = RW * 64 * 2;    // one shifted row image, 8 KB
constexpr int RW_ROW = 3 * RW_IMG;     // the three shifts of one row, 24 KB
constexpr int RW_NR = 5;               // row ring slots
constexpr int RW_XC = RW_ROW / 4096;   // glds calls per wave per row

template <int BTB>
struct RowsCfg {
  static constexpr int YIMG = PCH * BTB * 2;  // Y image of one chunk
  static constexpr int YC = YIMG / 4096;      // glds calls per wave (Y)
  static constexpr int G = RW_XC + YC;        // calls per wave, steady chunk
  static constexpr int LDS = RW_NR * RW_ROW + 3 * YIMG;  // 144 / 132 KB
  static constexpr int XF = BTB / 32;         // X fragments per wave and tap
  static constexpr int YHALF = (BTB / 16) * 128;  // next pixel-group row of Y
};

// tr16 pair at an immediate offset; HALF is the byte distance to the next
// pixel-group row of the image (second half of the 8-pixel run)
template <int OFF, int HALF>
__device__ __forceinline__ void tr16_issue_off(unsigned addr, u16x4& lo,
                                               u16x4& hi) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(lo)
               : "v"(addr), "n"(OFF));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(hi)
               : "v"(addr), "n"(OFF + HALF));
}

template <int N>
__device__ __forceinline__ void rows_wait(u16x4 (&lo)[2], u16x4 (&hi)[2]) {
  taps_wait<N>(lo[0], hi[0], lo[1], hi[1]);
}
template <int N>
__device__ __forceinline__ void rows_wait(u16x4 (&lo)[1], u16x4 (&hi)[1]) {
  asm volatile("s_waitcnt lgkmcnt(%2)"
               : "+v"(lo[0]), "+v"(hi[0])
               : "n"(N)
               : "memory");
}

// the X fragments of tap TP (image TP % 3 of the row at `ra`), K-step KK
template <int XF, int TP, int KK>
__device__ __forceinline__ void rows_issue_x(unsigned ra, u16x4 (&lo)[XF],
                                             u16x4 (&hi)[XF]) {
  constexpr int off = (TP % 3) * RW_IMG + KK * 8 * 512;
  tr16_issue_off<off, 512>(ra, lo[0], hi[0]);
  if constexpr (XF == 2) tr16_issue_off<off + 128, 512>(ra, lo[1], hi[1]);
}

template <int XF>
__device__ __forceinline__ void rows_mma(f32x4 (&acc)[2][XF],
                                         const u16x4 (&ylo)[2],
                                         const u16x4 (&yhi)[2],
                                         const u16x4 (&xlo)[XF],
                                         const u16x4 (&xhi)[XF]) {
  bf16x8 yf[2], xf[XF];
#pragma unroll
  for (int f = 0; f < 2; ++f) yf[f] = tr16_combine(ylo[f], yhi[f]);
#pragma unroll
  for (int f = 0; f < XF; ++f) xf[f] = tr16_combine(xlo[f], xhi[f]);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < XF; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], xf[j],
                                                          acc[i][j], 0, 0, 0);
}

// one 32-pixel K-step of a chunk for all nine taps: the reads of tap tp+1
// are in flight while tap tp multiplies. Each tap issues 2*XF reads and LDS
// reads return in order, so lgkmcnt(2*XF) after issuing tap tp+1 retires tap
// tp (and, at tp == 0, the Y reads issued before it).
template <int BTB, int KK>
__device__ __forceinline__ void rows_kstep(
    unsigned ya, const unsigned (&rowa)[3],
    f32x4 (&acc)[9][2][RowsCfg<BTB>::XF]) {
  using C = RowsCfg<BTB>;
  constexpr int XF = C::XF;
  constexpr int yk = KK * 8 * C::YHALF;  // pixels KK*32.. of the Y image
  u16x4 ylo[2], yhi[2], xlo[2][XF], xhi[2][XF];
  tr16_issue_off<yk, C::YHALF>(ya, ylo[0], yhi[0]);
  tr16_issue_off<yk + 128, C::YHALF>(ya, ylo[1], yhi[1]);
  rows_issue_x<XF, 0, KK>(rowa[0], xlo[0], xhi[0]);
#define RW_TAP(TP)                                                     \
  rows_issue_x<XF, (TP) + 1, KK>(rowa[((TP) + 1) / 3], xlo[((TP) + 1) & 1], \
                                 xhi[((TP) + 1) & 1]);                 \
  if ((TP) == 0) rows_wait<2 * XF>(ylo, yhi);                          \
  rows_wait<2 * XF>(xlo[(TP) & 1], xhi[(TP) & 1]);                     \
  rows_mma<XF>(acc[TP], ylo, yhi, xlo[(TP) & 1], xhi[(TP) & 1]);
  RW_TAP(0) RW_TAP(1) RW_TAP(2) RW_TAP(3) RW_TAP(4) RW_TAP(5) RW_TAP(6)
  RW_TAP(7)
#undef RW_TAP
  rows_wait<0>(xlo[0], xhi[0]);
  rows_mma<XF>(acc[8], ylo, yhi, xlo[0], xhi[0]);
}

template <int BTB>
__global__ __launch_bounds__(THREADS) void conv2d_wgrad_rows_kernel(
    const __bf16* __restrict__ Y, const __bf16* __restrict__ X,
    const __bf16* __restrict__ X2, float* __restrict__ ws, int HO, int B,
    int H, int W, int A, int A1, int yring, int nchunks, int cps, int ho_sh) {
  using C = RowsCfg<BTB>;
  constexpr int XF = C::XF;
  extern __shared__ __align__(16) char rlds[];
  char* const ybufs = rlds + RW_NR * RW_ROW;

  const int at_blocks = A >> 6;
  const int b0 = (blockIdx.x / at_blocks) * BTB;
  const int a0 = (blockIdx.x % at_blocks) * 64;
  const int c_begin = blockIdx.z * cps;
  const int c_end = min(c_begin + cps, nchunks);

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int wm = BTB == 64 ? (wid >> 1) * 32 : 0;
  const int wn = BTB == 64 ? (wid & 1) * 32 : wid * 16;
  const int HOp = HO + 2 * yring;
  const int WOp = RW + 2 * yring;

  // dual-X: the 64-wide a-tile lies wholly in one source (A1 % 64 == 0)
  const bool second = X2 != nullptr && a0 >= A1;
  const __bf16* xsrc = second ? X2 + (a0 - A1) : X + a0;
  const int as = X2 == nullptr ? A : (second ? A - A1 : A1);
  const __bf16* ysrc = Y + b0;

  // per-lane staging offsets (elements), fixed for the whole kernel
  int xl_off[RW_XC], yl_off[C::YC];
#pragma unroll
  for (int i = 0; i < RW_XC; ++i) {
    const int q = wid * RW_XC + i;  // 1 KB unit of the 24 KB row: image q/8
    int pixl, ch0;
    glds_decode((q & 7) * 64 + lane, 2, pixl, ch0);
    xl_off[i] = (pixl + (q >> 3)) * as + ch0;   // column pixl + s <= 65
  }
#pragma unroll
  for (int i = 0; i < C::YC; ++i) {
    int pixl, ch0;
    glds_decode((wid * C::YC + i) * 64 + lane, BTB == 64 ? 2 : 1, pixl, ch0);
    yl_off[i] = pixl * B + ch0;
  }

  auto stage_row = [&](int n, int hi, int slot) {
    const __bf16* rb = xsrc + (long)(n * H + hi) * W * as;
    char* l = rlds + slot * RW_ROW + wid * RW_XC * 1024;
#pragma unroll
    for (int i = 0; i < RW_XC; ++i) wglds16(rb + xl_off[i], l + i * 1024);
  };
  auto stage_y = [&](int n, int ho, int ybuf) {
    const __bf16* yb =
        ysrc + (((long)n * HOp + ho + yring) * WOp + yring) * B;
    char* l = ybufs + ybuf * C::YIMG + wid * C::YC * 1024;
#pragma unroll
    for (int i = 0; i < C::YC; ++i) wglds16(yb + yl_off[i], l + i * 1024);
  };

  f32x4 acc[9][2][XF];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < XF; ++j) acc[tp][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane tr16 bases: pixel run (lane>>4)*8 = two pixel-group rows, column
  // lane&15 of the wave's first channel subtile
  const unsigned yrd = (unsigned)(unsigned long long)ybufs +
                       (unsigned)((lane >> 4) * 2 * C::YHALF +
                                  (lane & 15) * 8 + (wm >> 4) * 128);
  const unsigned xrd = (unsigned)(unsigned long long)rlds +
                       (unsigned)((lane >> 4) * 2 * 512 + (lane & 15) * 8 +
                                  (wn >> 4) * 128);

  const int ho_mask = (1 << ho_sh) - 1;
  int c = c_begin;
  while (c < c_end) {
    const int n = c >> ho_sh;
    const int ho0 = c & ho_mask;
    const int len = min(HO - ho0, c_end - c);
    // the segment before this one ended on vmcnt(0); once every wave has
    // left its last chunk the whole ring is free
    if (c != c_begin) wbarrier_mem();
    stage_row(n, ho0, 0);
    stage_row(n, ho0 + 1, 1);
    stage_row(n, ho0 + 2, 2);
    stage_y(n, ho0, 0);
    if (len > 1) {
      stage_row(n, ho0 + 3, 3);
      stage_y(n, ho0 + 1, 1);
    }
    int s0 = 0;    // ring slot of chunk t's first row
    int snew = 4;  // ring slot chunk t+2's new row goes to
    int ybuf = 0;
    for (int t = 0; t < len; ++t) {
      if (t + 1 < len) wwaitcnt_vm<C::G>();
      else wwaitcnt_vm<0>();
      wbarrier_mem();
      // slot snew and Y buffer (t+2)%3 were last read by chunk t-1
      if (t + 2 < len) {
        stage_row(n, ho0 + t + 4, snew);
        stage_y(n, ho0 + t + 2, ybuf >= 1 ? ybuf - 1 : 2);
      }
      unsigned rowa[3];
      int slot = s0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        rowa[j] = xrd + (unsigned)(slot * RW_ROW);
        slot = slot + 1 == RW_NR ? 0 : slot + 1;
      }
      const unsigned ya = yrd + (unsigned)(ybuf * C::YIMG);
      rows_kstep<BTB, 0>(ya, rowa, acc);
      rows_kstep<BTB, 1>(ya, rowa, acc);
      s0 = s0 + 1 == RW_NR ? 0 : s0 + 1;
      snew = snew + 1 == RW_NR ? 0 : snew + 1;
      ybuf = ybuf == 2 ? 0 : ybuf + 1;
    }
    c += len;
  }

  float* slab = ws + (long)blockIdx.z * B * 9 * A;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int j = 0; j < XF; ++j) {
      const int a = a0 + wn + j * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int b = b0 + wm + i * 16 + (lane >> 4) * 4 + v;
          slab[((long)b * 9 + tp) * A + a] = acc[tp][i][j][v];
        }
    }
}

// ---------------------------------------------------------------------------
// All-taps 3x3 wgrad for 16-wide maps: the strip kernel above with 16-pixel
// row images and four-row chunks, summed in exactly the per-tap kernel's
// order. (stride 1, PAD == 0 over a zero-ringed X, WO == 16, HO a power of
// two >= 8, B, A1 and A multiples of 64, any yring.)
//
// What fixes the bits. A chunk is 64 consecutive output pixels, which on a
// 16-wide map is four output rows of one image (HO is a multiple of 4, so a
// chunk never crosses an image); its two MFMA K-steps are pixels 0-31 (rows
// 0-1) and 32-63 (rows 2-3), lane group g = lane>>4 holding pixels
// g*8..g*8+7 of the step: groups 0-1 the two halves of the step's first row,
// groups 2-3 those of its second. The slabs are the per-tap path's (any chunk
// may start one, also mid-image) and each element has one accumulator chain
// per slab. Tile shape, wave layout and LDS layout do not enter the sums.
//
// X side: each input row is staged ONCE as three column-shifted
// [16 pix][64 ch] subtiled images (2 KB each, 6 KB per row). Tap (r,s) of
// output row ho is the aligned tr16 read of image s of input row ho + r; an
// 8-pixel run is two whole pixel groups of one row image. A chunk reads six
// input rows, of which the chunk before it staged two: a steady chunk stages
// four rows plus one Y image, 24 KB + 8 KB against 9 x 32 KB for the per-tap
// kernel's 128x128 tile. The first chunk of a slab and of every image is a
// restart and stages six rows.
//
// Ring: when chunk k is staged, chunk k-2 is being computed (6 rows) and
// chunk k-1 is in flight (4 or 6 new rows); an image is at least two chunks,
// so at most one of k-1, k is a restart: 6 + 4 + 6 = 16 row slots, handed out
// by a running counter. Y rotates through 3 buffers.
//
// Tiles. BTB = 64: a 64(b) x 64(a) tile, 4 waves, 120 KB of LDS. BTB = 128: a
// 128(b) x 64(a) tile, 8 waves, the same row ring under a 16 KB Y image (144
// KB): the X rows are staged once for twice the b-channels, 24 + 16 KB per
// chunk against 2 x 32 KB, and a CU holds 8 waves instead of 4. It is taken
// wherever B is a multiple of 128 (1.28-1.44x over the 64x64 tile on every
// class of profiles/prof_wgrad_narrow_b512.txt).
//
// vmcnt. At the top of iteration t the only calls a wave issued after
// stage(t) are those of stage(t+1) (stage(t+2) follows the barrier): G = 8 / 5
// (BTB 64 / 128) when chunk t+1 is steady, GR = 11 / 7 when it is a restart,
// none when chunk t is the slab's last. Every wave issues the same number of
// calls per stage. Loads retire in order, so waiting for exactly that count
// retires stage(t) whatever stage(t) itself counted.
//
// Waves: (BTB/32) x 2 over the tile, each 32(b) x 32(a) x 9 taps = 36
// fragments (144 accumulator registers), as in the strip kernel. A K-step
// spans two input rows per tap, so the transpose-read base is per lane group:
// a lane holds the addresses of rows (g>>1)..(g>>1)+4 of the chunk's six,
// which may sit in non-adjacent slots where the ring wraps.

constexpr int NW = 16;                  // map width = pixels per row image
constexpr int NW_IMG = NW * 64 * 2;     // one shifted row image, 2 KB
constexpr int NW_ROW = 3 * NW_IMG;      // the three shifts of one row, 6 KB
constexpr int NW_NR = 16;               // row ring slots
constexpr int NW_RU = NW_ROW / 1024;    // 1 KB glds units per row: 6

template <int BTB>
struct NarrowCfg {
  static constexpr int WAVES = BTB / 16;             // 4 / 8
  static constexpr int NT = WAVES * 64;              // threads per block
  static constexpr int YIMG = PCH * BTB * 2;         // Y image of one chunk
  static constexpr int YC = YIMG / 1024 / WAVES;     // glds calls per wave (Y)
  static constexpr int XS = 4 * NW_RU / WAVES;       // X calls, steady: 6 / 3
  static constexpr int XR = (6 * NW_RU + WAVES - 1) / WAVES;  // restart: 9 / 5
  static constexpr int G = XS + YC;                  // steady chunk: 8 / 5
  static constexpr int GR = XR + YC;                 // restart chunk: 11 / 7
  static constexpr int LDS = NW_NR * NW_ROW + 3 * YIMG;  // 120 / 144 KB
  static constexpr int YHALF = (BTB / 16) * 128;  // next pixel-group row of Y
};

// the X fragments of tap TP (image TP % 3 of the row at `ra`)
template <int TP>
__device__ __forceinline__ void narrow_issue_x(unsigned ra, u16x4 (&lo)[2],
                                               u16x4 (&hi)[2]) {
  constexpr int off = (TP % 3) * NW_IMG;
  tr16_issue_off<off, 512>(ra, lo[0], hi[0]);
  tr16_issue_off<off + 128, 512>(ra, lo[1], hi[1]);
}

// one 32-pixel K-step (two output rows) of a chunk for all nine taps, the
// reads of tap tp+1 in flight while tap tp multiplies (cf. rows_kstep).
// rowa[i]: this lane's input row i of the step, i.e. tap row r reads rowa[r]
template <int BTB, int KK>
__device__ __forceinline__ void narrow_kstep(unsigned ya,
                                             const unsigned* rowa,
                                             f32x4 (&acc)[9][2][2]) {
  constexpr int YHALF = NarrowCfg<BTB>::YHALF;
  constexpr int yk = KK * 8 * YHALF;  // pixels KK*32.. of the Y image
  u16x4 ylo[2], yhi[2], xlo[2][2], xhi[2][2];
  tr16_issue_off<yk, YHALF>(ya, ylo[0], yhi[0]);
  tr16_issue_off<yk + 128, YHALF>(ya, ylo[1], yhi[1]);
  narrow_issue_x<0>(rowa[0], xlo[0], xhi[0]);
#define NW_TAP(TP)                                                          \
  narrow_issue_x<(TP) + 1>(rowa[((TP) + 1) / 3], xlo[((TP) + 1) & 1],       \
                           xhi[((TP) + 1) & 1]);                            \
  if ((TP) == 0) rows_wait<4>(ylo, yhi);                                    \
  rows_wait<4>(xlo[(TP) & 1], xhi[(TP) & 1]);                               \
  rows_mma<2>(acc[TP], ylo, yhi, xlo[(TP) & 1], xhi[(TP) & 1]);
  NW_TAP(0) NW_TAP(1) NW_TAP(2) NW_TAP(3) NW_TAP(4) NW_TAP(5) NW_TAP(6)
  NW_TAP(7)
#undef NW_TAP
  rows_wait<0>(xlo[0], xhi[0]);
  rows_mma<2>(acc[8], ylo, yhi, xlo[0], xhi[0]);
}

template <int BTB>
__global__ __launch_bounds__(NarrowCfg<BTB>::NT) void
conv2d_wgrad_narrow_kernel(
    const __bf16* __restrict__ Y, const __bf16* __restrict__ X,
    const __bf16* __restrict__ X2, float* __restrict__ ws, int HO, int B,
    int H, int W, int A, int A1, int yring, int nchunks, int cps, int img_sh) {
  using C = NarrowCfg<BTB>;
  extern __shared__ __align__(16) char nlds[];
  char* const ybufs = nlds + NW_NR * NW_ROW;

  const int at_blocks = A >> 6;
  const int b0 = (blockIdx.x / at_blocks) * BTB;
  const int a0 = (blockIdx.x % at_blocks) * 64;
  const int c_begin = blockIdx.z * cps;
  const int nch = min(c_begin + cps, nchunks) - c_begin;

  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int wm = (wid >> 1) * 32;
  const int wn = (wid & 1) * 32;
  const int HOp = HO + 2 * yring;
  const int WOp = NW + 2 * yring;

  // dual-X: the 64-wide a-tile lies wholly in one source (A1 % 64 == 0)
  const bool second = X2 != nullptr && a0 >= A1;
  const __bf16* xsrc = second ? X2 + (a0 - A1) : X + a0;
  const int as = X2 == nullptr ? A : (second ? A - A1 : A1);
  const __bf16* ysrc = Y + b0;

  // A stage of nr rows is nr * NW_RU glds units of 1 KB, dealt to the waves
  // in order: unit u is row u/6, image (u%6)/2, pixel half u&1. The 36 units
  // of a restart do not divide by 8 waves: the last wave's calls past the end
  // wrap to units 0..3 and write the bytes wave 0 writes there once more,
  // which keeps the call count the same in every wave.
  auto unit_of = [&](int i, bool fresh) {
    const int u = wid * (fresh ? C::XR : C::XS) + i;
    return u >= 6 * NW_RU ? u - 6 * NW_RU : u;
  };
  // per-lane staging offsets (elements), fixed for the whole kernel
  int xs_off[C::XS], xr_off[C::XR], yl_off[C::YC];
  auto unit_off = [&](int u) {
    const int row = u / NW_RU;
    const int q = u - row * NW_RU;
    int pixl, ch0;
    glds_decode((q & 1) * 64 + lane, 2, pixl, ch0);
    return (row * W + pixl + (q >> 1)) * as + ch0;  // column pixl + s <= 17
  };
#pragma unroll
  for (int i = 0; i < C::XS; ++i) xs_off[i] = unit_off(unit_of(i, false));
#pragma unroll
  for (int i = 0; i < C::XR; ++i) xr_off[i] = unit_off(unit_of(i, true));
#pragma unroll
  for (int i = 0; i < C::YC; ++i) {
    int pixl, ch0;
    glds_decode((wid * C::YC + i) * 64 + lane, BTB == 128 ? 3 : 2, pixl, ch0);
    yl_off[i] = ((pixl >> 4) * WOp + (pixl & (NW - 1))) * B + ch0;
  }

  const int img_mask = (1 << img_sh) - 1;  // chunks per image - 1
  auto restart = [&](int c) { return c == c_begin || (c & img_mask) == 0; };

  int sctr = 0;  // ring slot the next staged row goes to
  // LDS address of unit u of a stage whose first row goes to slot sctr
  auto unit_lds = [&](int u) {
    const int row = u / NW_RU;
    return nlds + ((sctr + row) & (NW_NR - 1)) * NW_ROW +
           (u - row * NW_RU) * 1024;
  };
  auto stage = [&](int c, int ybuf) {
    const int n = c >> img_sh;
    const int ho0 = (c & img_mask) * 4;
    const bool fresh = restart(c);
    const int hi0 = fresh ? ho0 : ho0 + 2;
    const __bf16* rb = xsrc + (long)(n * H + hi0) * W * as;
    if (fresh) {
#pragma unroll
      for (int i = 0; i < C::XR; ++i)
        wglds16(rb + xr_off[i], unit_lds(unit_of(i, true)));
    } else {
#pragma unroll
      for (int i = 0; i < C::XS; ++i)
        wglds16(rb + xs_off[i], unit_lds(unit_of(i, false)));
    }
    sctr = (sctr + (fresh ? 6 : 4)) & (NW_NR - 1);
    const __bf16* yb =
        ysrc + (((long)n * HOp + ho0 + yring) * WOp + yring) * B;
    char* l = ybufs + ybuf * C::YIMG + wid * C::YC * 1024;
#pragma unroll
    for (int i = 0; i < C::YC; ++i) wglds16(yb + yl_off[i], l + i * 1024);
  };

  f32x4 acc[9][2][2];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[tp][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane tr16 bases. Y image: pixel run (lane>>4)*8 = two pixel-group
  // rows. X row image: run ((lane>>4)&1)*8 of the row lane>>5 rows down.
  const int grow = lane >> 5;
  const unsigned yrd = (unsigned)(unsigned long long)ybufs +
                       (unsigned)((lane >> 4) * 2 * C::YHALF +
                                  (lane & 15) * 8 + (wm >> 4) * 128);
  const unsigned xrd = (unsigned)(unsigned long long)nlds +
                       (unsigned)(((lane >> 4) & 1) * 2 * 512 +
                                  (lane & 15) * 8 + (wn >> 4) * 128);

  int cctr = 0;  // ring slot of the first row the next restart chunk reads
  auto compute = [&](int c, int ybuf) {
    const bool fresh = restart(c);
    const int slot0 = fresh ? cctr : (cctr - 2) & (NW_NR - 1);
    cctr = (cctr + (fresh ? 6 : 4)) & (NW_NR - 1);
    // rows grow..grow+4 of the chunk's six
    unsigned rowa[5];
#pragma unroll
    for (int j = 0; j < 5; ++j)
      rowa[j] = xrd +
                (unsigned)(((slot0 + grow + j) & (NW_NR - 1)) * NW_ROW);
    const unsigned ya = yrd + (unsigned)(ybuf * C::YIMG);
    narrow_kstep<BTB, 0>(ya, rowa, acc);
    narrow_kstep<BTB, 1>(ya, rowa + 2, acc);
  };

  if (nch > 0) stage(c_begin, 0);
  if (nch > 1) stage(c_begin + 1, 1);
  int ybuf = 0;
  for (int t = 0; t < nch; ++t) {
    if (t + 1 >= nch) wwaitcnt_vm<0>();
    else if (restart(c_begin + t + 1)) wwaitcnt_vm<C::GR>();
    else wwaitcnt_vm<C::G>();
    wbarrier_mem();
    // buffer (t+2)%3 and the slots it takes were last read by chunk t-1
    if (t + 2 < nch) stage(c_begin + t + 2, ybuf >= 1 ? ybuf - 1 : 2);
    compute(c_begin + t, ybuf);
    ybuf = ybuf == 2 ? 0 : ybuf + 1;
  }

  float* slab = ws + (long)blockIdx.z * B * 9 * A;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int a = a0 + wn + j * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int b = b0 + wm + i * 16 + (lane >> 4) * 4 + v;
          slab[((long)b * 9 + tp) * A + a] = acc[tp][i][j][v];
        }
    }
}

// out[e] (+)= sum over slabs ws[z][e] — serial over z (deterministic).
__global__ __launch_bounds__(256) void wgrad_combine_kernel(
    const float* __restrict__ ws, float* __restrict__ out, int sp, long E,
    int accumulate) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E;
       e += (long)gridDim.x * 256) {
    float t = 0.f;
    for (int z = 0; z < sp; ++z) t += ws[(long)z * E + e];
    out[e] = accumulate ? out[e] + t : t;
  }
}

// Two-level form of the combine for the thin path, whose many slabs
// (sp ~ 1024) over few elements would make the single serial walk visible:
// CGR fixed groups of ceil(sp/CGR) consecutive slabs are summed serially in
// parallel, then the CGR group partials serially (cf. fold_rows_kernel).
// The association order is a function of sp alone.
constexpr int CGR = 32;  // slab groups
constexpr int CEL = 8;   // elements per block
__global__ __launch_bounds__(CGR * CEL) void wgrad_combine2_kernel(
    const float* __restrict__ ws, float* __restrict__ out, int sp, int E,
    int accumulate) {
  __shared__ float part[CGR][CEL];
  const int el = threadIdx.x % CEL;
  const int g = threadIdx.x / CEL;
  const int e = blockIdx.x * CEL + el;
  const int zs = (sp + CGR - 1) / CGR;
  const int z0 = g * zs;
  const int z1 = min(sp, z0 + zs);
  float t = 0.f;
  if (e < E) {
#pragma unroll 8
    for (int z = z0; z < z1; ++z) t += ws[(long)z * E + e];
  }
  part[g][el] = t;
  __syncthreads();
  if (g == 0 && e < E) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CGR; ++k) s += part[k][el];
    out[e] = accumulate ? out[e] + s : s;
  }
}

// (B, A, width) classes auto sends to the strip all-taps kernel: the 32-wide
// ones measured in profiles/prof_wgrad_b512.txt (B 64..128, A 64..256). There
// the result is bitwise the per-tap path's, so training results do not move.
// On wider maps the strip kernel sums in strip order: a different fp32
// rounding of ~1e-6, which a training step amplifies (see ROADMAP), so auto
// never sends them there. 64-wide maps have the row-order kernel instead
// (rows_auto below), whose sums are the per-tap path's bit for bit; 128-wide
// maps stay on the per-tap path.
bool taps_auto(int B, int A, int WO) {
  return B <= 128 && A <= 256 && WO == 32;
}

// (B, A) classes of 64-wide maps auto sends to the row-order all-taps kernel:
// those whose per-call time (kernel plus combine, per-tap slabs, batch 512)
// beat the per-tap path by more than the run-to-run spread in
// profiles/prof_wgrad_rows_b512.txt: the two of the 64-pixel model (c1.1
// 64x64 2.85x, upc5.0 64x(64+64) 2.94x) and the four the 128-pixel model
// reaches (B or A of 128, A up to 128+128: 1.95x-2.97x). Wider channel
// counts on a 64-wide map occur in no model, have not been measured and stay
// on the per-tap path.
bool rows_auto(int B, int A, int WO) {
  return WO == RW && B <= 128 && A <= 256;
}

// (B, A) classes of 16-wide maps auto sends to the narrow all-taps kernel:
// those whose per-call time (kernel plus combine, per-tap slabs, batch 512)
// beat the per-tap path by more than the run-to-run spread in
// profiles/prof_wgrad_narrow_b512.txt, all with 128x64 tiles: the four of the
// 64-pixel model (c3.0 256x128, c3.1 256x256, upc3.0 256x(256+256), upc3.2
// 128x256: 2.11x-2.30x) and the four the 128-pixel model reaches (B 512 or
// 256, A 256 to 512+512: 2.11x-2.44x). Anything else, the 64x64 tile
// included, has not been measured against per-tap under auto's rule and
// stays on the per-tap path.
bool narrow_auto(int B, int A, int WO) {
  if (WO != NW) return false;
  if (B == 128) return A == 256;
  return (B == 256 || B == 512) && 2 * A >= B && A <= 2 * B;
}

// P2PVG_WGRAD_ROWS=pertap keeps auto off the row-order kernel (A/B timing;
// the results are bitwise the same either way)
bool g_wgrad_rows = true;
// P2PVG_WGRAD_NARROW=pertap: the same for the 16-wide narrow kernel
bool g_wgrad_narrow = true;

enum WgradPath { WG_PER_TAP = 0, WG_STRIP = 1, WG_ROWS = 2, WG_NARROW = 3 };

// Path of a 3x3 stride-1 PAD == 0 wgrad over a zero-ringed X (H >= HO + 2,
// W >= WO + 2) with more than 3 input channels. taps: 0 per-tap, 1 strip
// kernel, 2 row-order kernel (3 / 4: with 64x64 / 32x64 tiles forced), 5
// narrow kernel (16-wide maps; 6 / 7: with 64x64 / 128x64 tiles forced), -1
// auto. A required kernel whose geometry is not eligible raises.
WgradPath wgrad_k3_path(int B, int A, int A1, int HO, int WO, int yring,
                        long taps) {
  TORCH_CHECK(taps >= -1 && taps <= 7, "wgrad: taps must be -1..7");
  const bool pow2 = HO > 0 && WO > 0 && ((HO * WO) & (HO * WO - 1)) == 0 &&
                    (WO & (WO - 1)) == 0;
  const bool ch_ok = B > 0 && A1 > 0 && B % 64 == 0 && A1 % 64 == 0 &&
                     A % 64 == 0 && yring >= 0 && pow2;
  const bool strip_ok = ch_ok && WO >= TPW && HO >= 4;
  const bool rows_ok = ch_ok && WO == RW;
  // an image of at least two chunks: what the 16-slot ring is sized for
  const bool narrow_ok = ch_ok && WO == NW && HO >= 8;
  TORCH_CHECK(taps != 1 || strip_ok,
              "wgrad: taps path required but the geometry is not eligible");
  TORCH_CHECK(taps < 2 || taps > 4 || rows_ok,
              "wgrad: row-order taps path required but the geometry is not "
              "eligible");
  TORCH_CHECK(taps < 5 || (narrow_ok && (taps != 7 || B % 128 == 0)),
              "wgrad: narrow taps path required but the geometry is not "
              "eligible");
  if (taps >= 5) return WG_NARROW;
  if (taps >= 2) return WG_ROWS;
  if (taps == 1) return WG_STRIP;
  if (taps == 0) return WG_PER_TAP;
  if (rows_ok && g_wgrad_rows && rows_auto(B, A, WO)) return WG_ROWS;
  if (strip_ok && taps_auto(B, A, WO)) return WG_STRIP;
  if (narrow_ok && g_wgrad_narrow && narrow_auto(B, A, WO)) return WG_NARROW;
  return WG_PER_TAP;
}

// fixed-order combine of the 3x3 slab planes (or accumulate into `acc`)
torch::Tensor wgrad_finish(torch::Tensor ws, c10::optional<torch::Tensor> acc,
                           int sp, int B, int A, long E, hipStream_t stream) {
  torch::Tensor out;
  int accumulate = 0;
  if (acc.has_value()) {
    out = acc.value();
    TORCH_CHECK(out.scalar_type() == torch::kFloat32 &&
                    out.is_non_overlapping_and_dense() && out.numel() == E,
                "wgrad acc: need dense fp32 tensor with B*R*S*A elements");
    accumulate = 1;
  } else {
    if (sp == 1) return ws[0];
    out = torch::empty({B, 3, 3, A}, ws.options());
  }
  const int cgrid = (int)std::min<long>(2048, (E + 255) / 256);
  hipLaunchKernelGGL(wgrad_combine_kernel, dim3(cgrid), dim3(256), 0, stream,
                     ws.data_ptr<float>(), out.data_ptr<float>(), sp, E,
                     accumulate);
  return out;
}

}  // namespace

// auto's use of the row-order kernel on or off (off: P2PVG_WGRAD_ROWS=pertap)
void set_wgrad_rows(bool on) { g_wgrad_rows = on; }
bool wgrad_rows() { return g_wgrad_rows; }
// the same for the 16-wide narrow kernel (off: P2PVG_WGRAD_NARROW=pertap)
void set_wgrad_narrow(bool on) { g_wgrad_narrow = on; }
bool wgrad_narrow() { return g_wgrad_narrow; }

// Host only: the path conv2d_nhwc_wgrad takes for a 3x3 stride-1 PAD == 0
// call over a zero-ringed X of A channels (A1 of them in the first source)
// and a Y of B channels on an HO x WO map: "per_tap", "taps_strip",
// "taps_rows" or "taps_narrow". They give the same bits wherever auto picks
// among them, so this is how a test sees the choice.
std::string conv2d_wgrad_path(long B, long A, long A1, long HO, long WO,
                              long yring, long taps) {
  switch (wgrad_k3_path((int)B, (int)A, (int)A1, (int)HO, (int)WO, (int)yring,
                        taps)) {
    case WG_ROWS: return "taps_rows";
    case WG_NARROW: return "taps_narrow";
    case WG_STRIP: return "taps_strip";
    default: return "per_tap";
  }
}

// Y: channels_last (N,B,HO,WO) bf16; X: channels_last (N,A,H,W) bf16.
// Returns dW (B, R, S, A) fp32. splitp<=0 -> auto. When `acc` is given it
// must be an fp32 tensor whose dense layout is (B,R,S,A) (e.g. the conv
// weight's channels_last .grad): the combine ACCUMULATES into it in place
// and returns it — this is how the framework skips autograd's per-use grad
// accumulation adds entirely (the ~29 uses per weight per step land here).
// thin: -1 picks the thin-channel path when the geometry allows it, 0 never
// takes it, 1 requires it (raises otherwise). taps: the same three values for
// the single-pass all-taps 3x3 strip kernel; 2 requires the row-order
// all-taps kernel (64-wide maps; 3 / 4 the same with 64x64 / 32x64 tiles
// forced, where 2 picks the tile by CU fill); 5 requires the narrow all-taps
// kernel (16-wide maps; 6 / 7 the same with 64x64 / 128x64 tiles forced,
// where 5 takes 128x64 when B is a multiple of 128).
torch::Tensor conv2d_nhwc_wgrad(torch::Tensor Y, torch::Tensor X, long R,
                                long S, long stride, long pad, long splitp,
                                c10::optional<torch::Tensor> acc, long yring,
                                c10::optional<torch::Tensor> X2, long thin,
                                long taps) {
  TORCH_CHECK(Y.is_cuda() && Y.scalar_type() == torch::kBFloat16 &&
                  Y.is_contiguous(at::MemoryFormat::ChannelsLast),
              "Y must be bf16 channels_last GPU");
  TORCH_CHECK(X.is_cuda() && X.scalar_type() == torch::kBFloat16 &&
                  X.is_contiguous(at::MemoryFormat::ChannelsLast),
              "X must be bf16 channels_last GPU");
  const int Nb = Y.size(0), B = Y.size(1);
  const int HO = Y.size(2) - 2 * (int)yring, WO = Y.size(3) - 2 * (int)yring;
  const int A1 = X.size(1);
  const int A = X2.has_value() ? A1 + (int)X2->size(1) : A1;
  const int H = X.size(2), W = X.size(3);
  if (X2.has_value()) {
    TORCH_CHECK(X2->is_cuda() && X2->scalar_type() == torch::kBFloat16 &&
                    X2->is_contiguous(at::MemoryFormat::ChannelsLast) &&
                    X2->size(0) == Nb && X2->size(2) == H &&
                    X2->size(3) == W && A1 % 64 == 0,
                "wgrad: X2 geometry mismatch");
  }
  TORCH_CHECK(X.size(0) == Nb, "batch mismatch");
  const long E = (long)B * R * S * A;

  // prefer 128-wide channel tiles; fall back to 64 when the channel count
  // is not 128-aligned (e.g. dual-X totals like 192) so the glds path's
  // exact-tiling requirement still holds
  const int BTB = (B >= 128 && B % 128 == 0) ? 128 : 64;
  const int BTA = (A >= 128 && A % 128 == 0) ? 128 : 64;
  const int bt = ceil_div(B, BTB), at = ceil_div(A, BTA);
  const int p_total = Nb * HO * WO;
  const bool pow2 = ((HO * WO) & (HO * WO - 1)) == 0 && (WO & (WO - 1)) == 0;

  // thin-channel path: all taps folded into <= 32 GEMM columns, any pad/yring
  const bool thin_ok = !X2.has_value() && R * S * A <= TQ && B % 64 == 0 &&
                       (stride == 1 || stride == 2) && pow2 && HO > 0 &&
                       WO > 0 && pad >= 0 && yring >= 0 &&
                       X.numel() * 2 < (1L << 31);
  TORCH_CHECK(thin != 1 || thin_ok,
              "wgrad: thin path required but the geometry is not eligible");
  const bool use_thin = thin_ok && thin != 0;

  // single-pass all-taps paths: 3x3 stride 1 over a zero-ringed X, 64-aligned
  // channels (each X part); the strip kernel (32-column strips, two-row
  // chunks) or, on 64-wide maps, the row-order kernel (one-row chunks)
  const bool k3_ringed = !use_thin && R == 3 && S == 3 && stride == 1 &&
                         pad == 0 && H >= HO + 2 && W >= WO + 2;
  TORCH_CHECK(taps >= -1 && taps <= 7, "wgrad: taps must be -1..7");
  TORCH_CHECK(taps < 1 || k3_ringed,
              "wgrad: taps path required but the geometry is not eligible");
  const WgradPath path =
      k3_ringed ? wgrad_k3_path(B, A, A1, HO, WO, (int)yring, taps)
                : WG_PER_TAP;
  const bool use_taps = path == WG_STRIP;
  const bool use_rows = path == WG_ROWS;

  int sp = (int)splitp;
  if (sp <= 0) {
    // thin: 36 KB of LDS per block -> 4 blocks per CU resident; ~1024 blocks
    // keep every CU's HBM queue full (one block holds only 24 KB in flight)
    sp = use_thin ? std::max(1, 1024 / (B / 64))
                  : std::max(1, 1024 / std::max(1, bt * at * (int)R * (int)S));
    sp = std::min(sp, ceil_div(p_total, PCH));
  }
  const int p_per_slab =
      ceil_div(ceil_div(p_total, sp), PCH) * PCH;  // chunk-aligned
  sp = ceil_div(p_total, p_per_slab);

  if (use_rows) {
    // per-tap slabs (whole rows: p_per_slab is a multiple of the 64-pixel
    // row) and the per-tap combine; a chunk is one output row, summed in the
    // per-tap kernel's order, so the result is bitwise the per-tap path's.
    // Half tiles when full tiles would leave more than half the CUs idle.
    int ho_sh = 0;
    while ((1 << ho_sh) < HO) ++ho_sh;
    const int tiles64 = (B / 64) * (A / 64);
    const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    const bool half = taps == 4 || (taps != 3 && 2 * tiles64 * sp <= cus);
    auto rws = torch::empty({sp, B, 3, 3, A},
                            Y.options().dtype(torch::kFloat32));
    auto rstream = at::cuda::getCurrentCUDAStream();
#define WGRAD_RLAUNCH(BB)                                                     \
  do {                                                                        \
    static bool cfg = false;                                                  \
    if (!cfg) {                                                               \
      (void)hipFuncSetAttribute(                                              \
          (const void*)&conv2d_wgrad_rows_kernel<BB>,                         \
          hipFuncAttributeMaxDynamicSharedMemorySize, RowsCfg<BB>::LDS);      \
      cfg = true;                                                             \
    }                                                                         \
    hipLaunchKernelGGL(                                                       \
        (conv2d_wgrad_rows_kernel<BB>), dim3((B / BB) * (A / 64), 1, sp),     \
        dim3(THREADS), RowsCfg<BB>::LDS, rstream,                             \
        reinterpret_cast<const __bf16*>(Y.data_ptr()),                        \
        reinterpret_cast<const __bf16*>(X.data_ptr()),                        \
        X2.has_value() ? reinterpret_cast<const __bf16*>(X2->data_ptr())      \
                       : nullptr,                                             \
        rws.data_ptr<float>(), HO, B, H, W, A, A1, (int)yring,                \
        p_total / PCH, p_per_slab / PCH, ho_sh);                              \
  } while (0)
    if (half) WGRAD_RLAUNCH(32);
    else WGRAD_RLAUNCH(64);
#undef WGRAD_RLAUNCH
    return wgrad_finish(rws, acc, sp, B, A, E, rstream);
  }

  if (path == WG_NARROW) {
    // per-tap slabs and combine; a chunk is the per-tap kernel's 64 pixels
    // (four output rows), summed in its order: bitwise the per-tap result
    int img_sh = 0;
    while ((4 << img_sh) < HO) ++img_sh;  // chunks per image
    auto nws = torch::empty({sp, B, 3, 3, A},
                            Y.options().dtype(torch::kFloat32));
    auto nstream = at::cuda::getCurrentCUDAStream();
    const bool wide = taps == 7 || (taps != 6 && B % 128 == 0);
    TORCH_CHECK(!wide || B % 128 == 0,
                "wgrad: 128x64 narrow tiles need B a multiple of 128");
#define WGRAD_NLAUNCH(BB)                                                     \
  do {                                                                        \
    static bool cfg = false;                                                  \
    if (!cfg) {                                                               \
      (void)hipFuncSetAttribute(                                              \
          (const void*)&conv2d_wgrad_narrow_kernel<BB>,                       \
          hipFuncAttributeMaxDynamicSharedMemorySize, NarrowCfg<BB>::LDS);    \
      cfg = true;                                                             \
    }                                                                         \
    hipLaunchKernelGGL(                                                       \
        (conv2d_wgrad_narrow_kernel<BB>), dim3((B / BB) * (A / 64), 1, sp),   \
        dim3(NarrowCfg<BB>::NT), NarrowCfg<BB>::LDS, nstream,                 \
        reinterpret_cast<const __bf16*>(Y.data_ptr()),                        \
        reinterpret_cast<const __bf16*>(X.data_ptr()),                        \
        X2.has_value() ? reinterpret_cast<const __bf16*>(X2->data_ptr())      \
                       : nullptr,                                             \
        nws.data_ptr<float>(), HO, B, H, W, A, A1, (int)yring,                \
        p_total / PCH, p_per_slab / PCH, img_sh);                             \
  } while (0)
    if (wide) WGRAD_NLAUNCH(128);
    else WGRAD_NLAUNCH(64);
#undef WGRAD_NLAUNCH
    return wgrad_finish(nws, acc, sp, B, A, E, nstream);
  }

  if (use_taps) {
    // the slabs are those of the per-tap path (same sp rule, same 64-pixel
    // chunk alignment), and so is the combine. On a 32-wide map a K-step is
    // the same 32 pixels in the same order there and here, so the result is
    // bitwise the per-tap path's; on wider maps the strip order differs.
    int seg_sh = 0, strip_sh = 0;
    while ((2 << seg_sh) < HO) ++seg_sh;          // chunks per (image, strip)
    while ((TPW << strip_sh) < WO) ++strip_sh;    // strips per row
    const int tiles = (B / 64) * (A / 64);
    auto tws = torch::empty({sp, B, 3, 3, A},
                            Y.options().dtype(torch::kFloat32));
    static bool cfg = false;
    if (!cfg) {
      (void)hipFuncSetAttribute((const void*)&conv2d_wgrad_taps_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                TP_LDS);
      cfg = true;
    }
    auto tstream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(
        conv2d_wgrad_taps_kernel, dim3(tiles, 1, sp), dim3(THREADS), TP_LDS,
        tstream, reinterpret_cast<const __bf16*>(Y.data_ptr()),
        reinterpret_cast<const __bf16*>(X.data_ptr()),
        X2.has_value() ? reinterpret_cast<const __bf16*>(X2->data_ptr())
                       : nullptr,
        tws.data_ptr<float>(), HO, WO, B, H, W, A, A1, (int)yring,
        p_total / PCH, p_per_slab / PCH, seg_sh, strip_sh);
    return wgrad_finish(tws, acc, sp, B, A, E, tstream);
  }

  // per-slab planes, written by stores — never zeroed
  auto ws = torch::empty({sp, B, (long)R, (long)S, A},
                         Y.options().dtype(torch::kFloat32));

  dim3 grid(bt * at, (int)(R * S), sp);
  auto stream = at::cuda::getCurrentCUDAStream();

  const bool use_glds = pad == 0 && pow2 && HO > 0 && WO > 0 &&
                        B % BTB == 0 && A % BTA == 0 &&
                        (X2.has_value() || p_total >= 4 * PCH);
  TORCH_CHECK(!X2.has_value() || use_glds,
              "wgrad: dual-X requires the glds-eligible geometry");
  if (use_thin) {
    int howo_sh = 0, wo_sh = 0;
    while ((1 << howo_sh) < HO * WO) ++howo_sh;
    while ((1 << wo_sh) < WO) ++wo_sh;
    hipLaunchKernelGGL(conv2d_wgrad_thin_kernel, dim3(B / 64, 1, sp),
                       dim3(THREADS), 0, stream,
                       reinterpret_cast<const __bf16*>(Y.data_ptr()),
                       reinterpret_cast<const __bf16*>(X.data_ptr()),
                       ws.data_ptr<float>(), Nb, HO, WO, B, H, W, A, (int)R,
                       (int)S, (int)stride, (int)pad, p_per_slab, (int)yring,
                       howo_sh, wo_sh, (int)(X.numel() * 2));
  } else if (use_glds) {
    // PAD==0 means every X gather is in-bounds (padded operand or genuine
    // valid conv): glds 3-buffer pipeline, shift-only pixel decode
    int howo_sh = 0, wo_sh = 0;
    while ((1 << howo_sh) < HO * WO) ++howo_sh;
    while ((1 << wo_sh) < WO) ++wo_sh;
#define WGRAD_GLAUNCH(BB, AA)                                                 \
  do {                                                                        \
    const int shmem = 3 * PCH * (BB + AA) * 2;                                \
    static bool cfg = false;                                                  \
    if (!cfg) {                                                               \
      (void)hipFuncSetAttribute(                                              \
          (const void*)&conv2d_wgrad_glds_kernel<BB, AA>,                     \
          hipFuncAttributeMaxDynamicSharedMemorySize, shmem);                 \
      cfg = true;                                                             \
    }                                                                         \
    hipLaunchKernelGGL((conv2d_wgrad_glds_kernel<BB, AA>), grid,              \
                       dim3(THREADS), shmem, stream,                          \
                       reinterpret_cast<const __bf16*>(Y.data_ptr()),         \
                       reinterpret_cast<const __bf16*>(X.data_ptr()),         \
                       ws.data_ptr<float>(), Nb, HO, WO, B, H, W, A, (int)R,  \
                       (int)S, (int)stride, p_per_slab, (int)yring, howo_sh,  \
                       wo_sh,                                                 \
                       X2.has_value()                                         \
                           ? reinterpret_cast<const __bf16*>(X2->data_ptr())  \
                           : nullptr,                                         \
                       A1);                                                   \
  } while (0)
    if (BTB == 128 && BTA == 128) WGRAD_GLAUNCH(128, 128);
    else if (BTB == 128) WGRAD_GLAUNCH(128, 64);
    else if (BTA == 128) WGRAD_GLAUNCH(64, 128);
    else WGRAD_GLAUNCH(64, 64);
#undef WGRAD_GLAUNCH
  } else {
#define WGRAD_LAUNCH(BB, AA)                                                   \
  hipLaunchKernelGGL((conv2d_wgrad_kernel<BB, AA>), grid, dim3(THREADS), 0,    \
                     stream, reinterpret_cast<const __bf16*>(Y.data_ptr()),    \
                     reinterpret_cast<const __bf16*>(X.data_ptr()),            \
                     ws.data_ptr<float>(), Nb, HO, WO, B, H, W, A, (int)R,     \
                     (int)S, (int)stride, (int)pad, p_per_slab, (int)yring)
  if (BTB == 128 && BTA == 128) WGRAD_LAUNCH(128, 128);
  else if (BTB == 128) WGRAD_LAUNCH(128, 64);
  else if (BTA == 128) WGRAD_LAUNCH(64, 128);
  else WGRAD_LAUNCH(64, 64);
#undef WGRAD_LAUNCH
  }

  torch::Tensor out;
  int accumulate = 0;
  if (acc.has_value()) {
    out = acc.value();
    TORCH_CHECK(out.scalar_type() == torch::kFloat32 &&
                    out.is_non_overlapping_and_dense() && out.numel() == E,
                "wgrad acc: need dense fp32 tensor with B*R*S*A elements");
    accumulate = 1;
  } else {
    if (sp == 1) return ws[0];
    out = torch::empty({B, (long)R, (long)S, A},
                       Y.options().dtype(torch::kFloat32));
  }
  if (use_thin) {
    hipLaunchKernelGGL(wgrad_combine2_kernel, dim3(ceil_div((int)E, CEL)),
                       dim3(CGR * CEL), 0, stream, ws.data_ptr<float>(),
                       out.data_ptr<float>(), sp, (int)E, accumulate);
    return out;
  }
  const int cgrid = (int)std::min<long>(2048, (E + 255) / 256);
  hipLaunchKernelGGL(wgrad_combine_kernel, dim3(cgrid), dim3(256), 0, stream,
                     ws.data_ptr<float>(), out.data_ptr<float>(), sp, E,
                     accumulate);
  return out;
}
