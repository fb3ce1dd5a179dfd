// MovingMNIST frame synthesis on the device.
//
// The host plans trajectories (DynamicLengthMovingMNIST.plan_batch: the same
// random draws as the CPU dataset) and ships only the plan: idx (B, D) and
// pos (L, B, D, 2) = (sy, sx), int32. This kernel renders the frames:
//
//   out[l, b, 0, y, x] = min(1, sum_{d=0..D-1, in that order}
//                               digits[idx[b,d], y - sy, x - sx]  if inside)
//
// with an fp32 accumulator starting at 0. Sprites are >= 0, so adding 0.f for
// a pixel outside a digit's 32x32 window is bit-identical to skipping it, and
// the left-to-right order over d matches the dataset's slice-adds (it fixes
// the fp32 sum once three or more digits overlap).
//
// Pure write-bandwidth work (batch 256 x 30 frames x 64x64 fp32 = 126 MB out):
// one block per (l, b) image, its D sprites staged in LDS (4 KB each, one
// 16-byte load per thread per sprite), idx/pos block-uniform, every thread
// writes 4 consecutive pixels per 16-byte store. No MFMA, no atomics.
//
// Contract (validated on the host by ops.moving_mnist_render BEFORE launch):
// 0 <= idx < N, 0 <= sy, sx <= S - 32, S % 4 == 0, S >= 36, 1 <= D <= 8.
// Window membership gates every LDS read and every store lands inside the
// (S, S) image of its own block, so the kernel has no clipping path.

#include "common.h"

namespace {

constexpr int SPR = 32;              // sprite edge
constexpr int SPR_ELEMS = SPR * SPR;  // 1024 floats = 4 KB
constexpr int MAX_DIGITS = 8;
constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void moving_mnist_render_kernel(
    const float* __restrict__ digits,  // (N, 32, 32)
    const int* __restrict__ idx,       // (B, D)
    const int* __restrict__ pos,       // (L, B, D, 2): sy, sx
    float* __restrict__ out,           // (L*B, S, S)
    int B, int D, int S) {
  extern __shared__ float spr[];  // D * 1024 floats
  __shared__ int s_sy[MAX_DIGITS];
  __shared__ int s_sx[MAX_DIGITS];

  const long img = blockIdx.x;  // l * B + b
  const int b = (int)(img % B);
  const int tid = threadIdx.x;

  // stage the D sprites: 1024 floats each = one float4 per thread
  for (int d = 0; d < D; ++d) {
    const long sprite = idx[b * D + d];
    const float4 v = reinterpret_cast<const float4*>(
        digits + sprite * SPR_ELEMS)[tid];
    reinterpret_cast<float4*>(spr + d * SPR_ELEMS)[tid] = v;
  }
  if (tid < D) {
    const int* p = pos + (img * D + tid) * 2;
    s_sy[tid] = p[0];
    s_sx[tid] = p[1];
  }
  __syncthreads();

  const int qrow = S >> 2;         // 4-pixel quads per row
  const int nquad = S * qrow;      // per image
  float* __restrict__ o = out + img * (long)S * S;

  for (int q = tid; q < nquad; q += THREADS) {
    const int y = q / qrow;
    const int x0 = (q - y * qrow) << 2;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < D; ++d) {
      const int ry = y - s_sy[d];
      if ((unsigned)ry < (unsigned)SPR) {
        const int rx0 = x0 - s_sx[d];
        const float* row = spr + d * SPR_ELEMS + ry * SPR;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rx = rx0 + j;
          acc[j] += ((unsigned)rx < (unsigned)SPR) ? row[rx] : 0.f;
        }
      }
    }
    float4 v;
    v.x = fminf(acc[0], 1.f);
    v.y = fminf(acc[1], 1.f);
    v.z = fminf(acc[2], 1.f);
    v.w = fminf(acc[3], 1.f);
    reinterpret_cast<float4*>(o)[q] = v;  // S % 4 == 0: 16-byte aligned
  }
}

}  // namespace

// digits (N,32,32) f32, idx (B,D) i32, pos (L,B,D,2) i32, all on one device
// and contiguous -> (L,B,1,S,S) f32. Value ranges are the caller's contract
// (see the header comment); shapes, dtypes and the S / D ranges are checked.
torch::Tensor moving_mnist_render(torch::Tensor digits, torch::Tensor idx,
                                  torch::Tensor pos, long S) {
  CHECK_INPUT(digits);
  CHECK_INPUT(idx);
  CHECK_INPUT(pos);
  TORCH_CHECK(digits.scalar_type() == torch::kFloat32 && digits.dim() == 3 &&
                  digits.size(0) >= 1 && digits.size(1) == SPR &&
                  digits.size(2) == SPR,
              "moving_mnist_render: digits must be (N,32,32) fp32");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(digits.data_ptr()) % 16 == 0,
              "moving_mnist_render: digits must be 16-byte aligned");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.dim() == 2,
              "moving_mnist_render: idx must be (B,D) int32");
  const long B = idx.size(0), D = idx.size(1);
  TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.dim() == 4 &&
                  pos.size(1) == B && pos.size(2) == D && pos.size(3) == 2,
              "moving_mnist_render: pos must be (L,B,D,2) int32");
  TORCH_CHECK(idx.device() == digits.device() &&
                  pos.device() == digits.device(),
              "moving_mnist_render: all inputs must be on one device");
  TORCH_CHECK(D >= 1 && D <= MAX_DIGITS, "moving_mnist_render: 1 <= D <= 8");
  TORCH_CHECK(S % 4 == 0 && S >= 36,
              "moving_mnist_render: image size must be >= 36 and % 4 == 0");
  const long L = pos.size(0);
  auto out = torch::empty({L, B, 1, S, S}, digits.options());
  const long nimg = L * B;
  if (nimg == 0) return out;
  TORCH_CHECK(nimg <= 0x7fffffffL, "moving_mnist_render: too many images");
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(moving_mnist_render_kernel, dim3((unsigned)nimg),
                     dim3(THREADS), (size_t)D * SPR_ELEMS * sizeof(float),
                     stream, digits.data_ptr<float>(), idx.data_ptr<int>(),
                     pos.data_ptr<int>(), out.data_ptr<float>(), (int)B,
                     (int)D, (int)S);
  return out;
}
