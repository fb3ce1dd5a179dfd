// Fused per-frame SSIM + MSE for evaluation.
//
// For M image pairs (C, H, W) one read of both operands yields
//
//   ssim[m] = mean over C*H*W of the SSIM map of utils/metrics.py::ssim
//             (11x11 gaussian window, sigma 1.5, zero padding 5)
//   mse[m]  = mean over C*H*W of (a - b)^2
//
// The window is separable: g (x) g with the eleven 1-D weights the host passes
// in (the 1-D factor of utils.metrics._gaussian_window). One 256-thread block
// owns one 32x32 output tile of one image and loops over its channels:
//
//   load    42x42 halo tile of a and b -> LDS as fp32 (zeros outside the
//           image: the reference's zero padding); (a-b)^2 of the 32x32 core
//           is accumulated here, from the same loads
//   pass 1  11 taps along x on the 42 halo rows: a, b, a*a, b*b, a*b
//           -> five 42x32 fp32 planes in LDS; a thread makes 4 adjacent
//           columns from 14 inputs read as 16-byte LDS loads
//   pass 2  11 taps along y: a thread makes 4 rows of one column from 14 plane
//           rows (lanes = consecutive columns: conflict-free ds_read_b32),
//           then the SSIM formula, masked to pixels inside the image
//
// LDS: 2 * 42 * 44 * 4 (inputs, row stride 44 keeps 16-byte alignment)
//    + 5 * 42 * 32 * 4 (planes) = 41,664 B -> 3 blocks / 12 waves per CU.
// Pure vector-ALU + LDS work: no MFMA, no atomics.
//
// Reduction (deterministic): shuffle tree per wave, the 4 wave sums folded in
// order by thread 0 -> one partial per (image, tile); a second kernel folds
// an image's partials in tile order and divides by C*H*W.
//
// Addressing: element strides per operand (n, c, h, w), 64-bit throughout, so
// dense NCHW, dense channels_last and any image stride are read in place and
// an image may start beyond element 2^31. Every load is guarded by
// 0 <= y < H and 0 <= x < W, so only elements of the (M, C, H, W) view are
// touched. dtypes fp32 / bf16 / fp16 per operand, converted to fp32 at load.

#include <c10/cuda/CUDAException.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int TILE = 32;              // output tile edge
constexpr int RAD = 5;                // window radius
constexpr int TAPS = 2 * RAD + 1;     // 11
constexpr int IN_T = TILE + 2 * RAD;  // 42: halo tile edge
constexpr int IN_LD = 44;             // halo row stride (floats), 16-B aligned
constexpr int NQ = 5;                 // a, b, a*a, b*b, a*b
constexpr int THREADS = 256;
constexpr int NWAVES = THREADS / WAVE;

struct Taps {
  float w[TAPS];
};
struct Strides {
  long n, c, h, w;
};

enum { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };

template <int DT>
__device__ __forceinline__ float load_f32(const void* __restrict__ p, long i) {
  if constexpr (DT == DT_F32) {
    return static_cast<const float*>(p)[i];
  } else if constexpr (DT == DT_BF16) {
    return __uint_as_float(
        (unsigned)static_cast<const unsigned short*>(p)[i] << 16);
  } else {
    return __half2float(static_cast<const __half*>(p)[i]);
  }
}

template <int DA, int DB>
__global__ __launch_bounds__(THREADS) void frame_metrics_tile_kernel(
    const void* __restrict__ a, const void* __restrict__ b, Strides sa,
    Strides sb, long img0, int C, int H, int W, int tiles_x, int tiles_per_img,
    Taps taps, float c1, float c2,
    float* __restrict__ part_ssim,  // (M * tiles_per_img)
    float* __restrict__ part_sq) {  // (M * tiles_per_img)
  __shared__ __attribute__((aligned(16))) float s_in[2][IN_T * IN_LD];
  __shared__ __attribute__((aligned(16))) float s_mid[NQ][IN_T * TILE];
  __shared__ float s_red[2][NWAVES];

  const int tid = threadIdx.x;
  // a launch covers images img0 .. : the host splits M so that no grid
  // exceeds 2^32 threads
  const long bid = img0 * tiles_per_img + blockIdx.x;
  const long img = bid / tiles_per_img;
  const int tile = (int)(bid - img * tiles_per_img);
  const int ty0 = (tile / tiles_x) * TILE;
  const int tx0 = (tile % tiles_x) * TILE;
  const long base_a = img * sa.n;
  const long base_b = img * sb.n;

  // pass 2 ownership: column vx, rows vy0 .. vy0+3 of the tile
  const int vx = tid & (TILE - 1);
  const int vy0 = (tid >> 5) << 2;

  float acc_ssim = 0.f, acc_sq = 0.f;

  for (int c = 0; c < C; ++c) {
    // ---- load the halo tile (zeros outside the image) ----
    // s_in is last read in pass 1 of the previous channel, which every
    // thread left through the barrier in front of pass 2.
    for (int i = tid; i < IN_T * IN_T; i += THREADS) {
      const int iy = i / IN_T;
      const int ix = i - iy * IN_T;
      const int gy = ty0 - RAD + iy;
      const int gx = tx0 - RAD + ix;
      float va = 0.f, vb = 0.f;
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
        va = load_f32<DA>(a, base_a + c * sa.c + gy * sa.h + gx * sa.w);
        vb = load_f32<DB>(b, base_b + c * sb.c + gy * sb.h + gx * sb.w);
        if ((unsigned)(iy - RAD) < (unsigned)TILE &&
            (unsigned)(ix - RAD) < (unsigned)TILE) {
          const float d = va - vb;
          acc_sq = fmaf(d, d, acc_sq);
        }
      }
      s_in[0][iy * IN_LD + ix] = va;
      s_in[1][iy * IN_LD + ix] = vb;
    }
    __syncthreads();

    // ---- pass 1: 11 taps along x, 4 adjacent columns per thread ----
    for (int i = tid; i < IN_T * (TILE / 4); i += THREADS) {
      const int iy = i >> 3;
      const int x0 = (i & 7) << 2;
      float va[14], vb[14];
      {
        const float* ra = &s_in[0][iy * IN_LD + x0];
        const float* rb = &s_in[1][iy * IN_LD + x0];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const float4 ta = reinterpret_cast<const float4*>(ra)[v];
          const float4 tb = reinterpret_cast<const float4*>(rb)[v];
          va[4 * v + 0] = ta.x; va[4 * v + 1] = ta.y;
          va[4 * v + 2] = ta.z; va[4 * v + 3] = ta.w;
          vb[4 * v + 0] = tb.x; vb[4 * v + 1] = tb.y;
          vb[4 * v + 2] = tb.z; vb[4 * v + 3] = tb.w;
        }
        const float2 ta = reinterpret_cast<const float2*>(ra + 12)[0];
        const float2 tb = reinterpret_cast<const float2*>(rb + 12)[0];
        va[12] = ta.x; va[13] = ta.y;
        vb[12] = tb.x; vb[13] = tb.y;
      }
      float vaa[14], vbb[14], vab[14];
#pragma unroll
      for (int v = 0; v < 14; ++v) {
        vaa[v] = va[v] * va[v];
        vbb[v] = vb[v] * vb[v];
        vab[v] = va[v] * vb[v];
      }
      float o[NQ][4];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[q][j] = 0.f;
#pragma unroll
      for (int k = 0; k < TAPS; ++k) {
        const float w = taps.w[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[0][j] = fmaf(w, va[j + k], o[0][j]);
          o[1][j] = fmaf(w, vb[j + k], o[1][j]);
          o[2][j] = fmaf(w, vaa[j + k], o[2][j]);
          o[3][j] = fmaf(w, vbb[j + k], o[3][j]);
          o[4][j] = fmaf(w, vab[j + k], o[4][j]);
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float4 t;
        t.x = o[q][0]; t.y = o[q][1]; t.z = o[q][2]; t.w = o[q][3];
        reinterpret_cast<float4*>(&s_mid[q][iy * TILE + x0])[0] = t;
      }
    }
    __syncthreads();

    // ---- pass 2: 11 taps along y, 4 rows of one column per thread ----
    float r[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float v[14];
#pragma unroll
      for (int t = 0; t < 14; ++t) v[t] = s_mid[q][(vy0 + t) * TILE + vx];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[q][j] = 0.f;
#pragma unroll
      for (int k = 0; k < TAPS; ++k) {
        const float w = taps.w[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[q][j] = fmaf(w, v[j + k], r[q][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mu_a = r[0][j], mu_b = r[1][j];
      const float mu_a2 = mu_a * mu_a, mu_b2 = mu_b * mu_b;
      const float mu_ab = mu_a * mu_b;
      const float sig_a2 = r[2][j] - mu_a2;
      const float sig_b2 = r[3][j] - mu_b2;
      const float sig_ab = r[4][j] - mu_ab;
      const float num = (2.f * mu_ab + c1) * (2.f * sig_ab + c2);
      const float den = (mu_a2 + mu_b2 + c1) * (sig_a2 + sig_b2 + c2);
      const float s = num / den;
      if (ty0 + vy0 + j < H && tx0 + vx < W) acc_ssim += s;
    }
    // no barrier here: the next load writes s_in only, and the barrier
    // behind it orders this pass 2 before the next pass 1 rewrites s_mid
  }

  // ---- fixed-order block reduction -> one partial per (image, tile) ----
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    acc_ssim += __shfl_down(acc_ssim, off, WAVE);
    acc_sq += __shfl_down(acc_sq, off, WAVE);
  }
  if ((tid & (WAVE - 1)) == 0) {
    s_red[0][tid / WAVE] = acc_ssim;
    s_red[1][tid / WAVE] = acc_sq;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
      s += s_red[0][w];
      q += s_red[1][w];
    }
    part_ssim[bid] = s;
    part_sq[bid] = q;
  }
}

// one thread per image: fold its tile partials in tile order
__global__ __launch_bounds__(THREADS) void frame_metrics_fold_kernel(
    const float* __restrict__ part_ssim, const float* __restrict__ part_sq,
    long M, int tiles_per_img, float count, float* __restrict__ ssim,
    float* __restrict__ mse) {
  const long m = (long)blockIdx.x * THREADS + threadIdx.x;
  if (m >= M) return;
  const float* ps = part_ssim + m * tiles_per_img;
  const float* pq = part_sq + m * tiles_per_img;
  float s = 0.f, q = 0.f;
  for (int t = 0; t < tiles_per_img; ++t) {
    s += ps[t];
    q += pq[t];
  }
  ssim[m] = s / count;
  mse[m] = q / count;
}

int dtype_code(const torch::Tensor& t, const char* name) {
  switch (t.scalar_type()) {
    case torch::kFloat32: return DT_F32;
    case torch::kBFloat16: return DT_BF16;
    case torch::kFloat16: return DT_F16;
    default:
      TORCH_CHECK(false, "frame_metrics: ", name,
                  " must be fp32, bf16 or fp16");
  }
  return -1;
}

Strides strides_of(const torch::Tensor& t, const char* name) {
  Strides s{t.stride(0), t.stride(1), t.stride(2), t.stride(3)};
  TORCH_CHECK(s.n >= 0 && s.c >= 0 && s.h >= 0 && s.w >= 0,
              "frame_metrics: ", name, " has a negative stride");
  return s;
}

}  // namespace

// a, b: (M, C, H, W) strided views (any non-negative element strides), fp32 /
// bf16 / fp16 each, one device. win: the eleven 1-D window weights, fp32 on the
// CPU. Returns {ssim (M) f32, mse (M) f32}.
std::vector<torch::Tensor> frame_metrics(torch::Tensor a, torch::Tensor b,
                                         torch::Tensor win,
                                         double data_range) {
  CHECK_CUDA(a);
  CHECK_CUDA(b);
  TORCH_CHECK(a.device() == b.device(),
              "frame_metrics: a and b must be on one device");
  TORCH_CHECK(a.dim() == 4 && b.dim() == 4 && a.sizes() == b.sizes(),
              "frame_metrics: a and b must be (M,C,H,W) of equal shape");
  TORCH_CHECK(!win.is_cuda() && win.scalar_type() == torch::kFloat32 &&
                  win.dim() == 1 && win.size(0) == TAPS && win.is_contiguous(),
              "frame_metrics: win must be 11 fp32 weights on the CPU");
  TORCH_CHECK(data_range > 0, "frame_metrics: data_range must be > 0");
  const int da = dtype_code(a, "a"), db = dtype_code(b, "b");
  const long M = a.size(0), C = a.size(1), H = a.size(2), W = a.size(3);
  TORCH_CHECK(C >= 1 && H >= 1 && W >= 1,
              "frame_metrics: C, H, W must be >= 1");
  TORCH_CHECK(C * H * W <= (1L << 24),
              "frame_metrics: image too large for an fp32 pixel count");
  const Strides sa = strides_of(a, "a"), sb = strides_of(b, "b");

  auto opts = a.options().dtype(torch::kFloat32);
  auto ssim = torch::empty({M}, opts);
  auto mse = torch::empty({M}, opts);
  if (M == 0) return {ssim, mse};

  const long tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
  const long tiles = tiles_x * tiles_y;
  // a launch may not exceed 2^32 threads: whole images per launch, at most
  // MAX_BLOCKS blocks each (tiles <= 2^14 since C*H*W <= 2^24)
  constexpr long MAX_BLOCKS = (1L << 32) / THREADS - 1;
  const long imgs_per_launch = MAX_BLOCKS / tiles;
  TORCH_CHECK(imgs_per_launch >= 1, "frame_metrics: image too large");
  auto part = torch::empty({2, M * tiles}, opts);
  float* part_ssim = part.data_ptr<float>();
  float* part_sq = part_ssim + M * tiles;

  Taps taps;
  const float* wp = win.data_ptr<float>();
  for (int k = 0; k < TAPS; ++k) taps.w[k] = wp[k];
  const float c1 = (float)((0.01 * data_range) * (0.01 * data_range));
  const float c2 = (float)((0.03 * data_range) * (0.03 * data_range));

  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 block(THREADS);
#define FM_LAUNCH(DA, DB)                                                     \
  for (long m0 = 0; m0 < M; m0 += imgs_per_launch) {                          \
    const long nimg = std::min(imgs_per_launch, M - m0);                      \
    hipLaunchKernelGGL((frame_metrics_tile_kernel<DA, DB>),                   \
                       dim3((unsigned)(nimg * tiles)), block, 0, stream,      \
                       a.data_ptr(), b.data_ptr(), sa, sb, m0, (int)C,        \
                       (int)H, (int)W, (int)tiles_x, (int)tiles, taps, c1,    \
                       c2, part_ssim, part_sq);                               \
    C10_CUDA_KERNEL_LAUNCH_CHECK();                                           \
  }
#define FM_DISPATCH_B(DA)                      \
  switch (db) {                                \
    case DT_F32: FM_LAUNCH(DA, DT_F32); break; \
    case DT_BF16: FM_LAUNCH(DA, DT_BF16); break; \
    default: FM_LAUNCH(DA, DT_F16); break;     \
  }
  switch (da) {
    case DT_F32: FM_DISPATCH_B(DT_F32); break;
    case DT_BF16: FM_DISPATCH_B(DT_BF16); break;
    default: FM_DISPATCH_B(DT_F16); break;
  }
#undef FM_DISPATCH_B
#undef FM_LAUNCH
  hipLaunchKernelGGL(frame_metrics_fold_kernel,
                     dim3((unsigned)((M + THREADS - 1) / THREADS)), block, 0,
                     stream, part_ssim, part_sq, M, (int)tiles,
                     (float)(C * H * W), ssim.data_ptr<float>(),
                     mse.data_ptr<float>());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {ssim, mse};
}
