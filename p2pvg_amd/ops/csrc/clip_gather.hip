// Batch gather from a device-resident uint8 frame bank.
//
// The decoded dataset stays on the device as bank (N, T, H, W, C) uint8. Per
// batch the host ships only the B clip indices; this kernel gathers, converts
// and lays out the training batch:
//
//   out[l, b, :] = float(bank[idx[b], l, :]) / 255      out (L, B, H, W, C) f32
//
// The quotient is the correctly rounded fp32 division (it has to equal the
// dataset's np.float32(v) / 255.0, and v * (1/255) differs from that for 126
// of the 256 byte values): a plain `/`, which hipcc compiles to the IEEE
// sequence as long as no fast-math flag is given. No reciprocal multiply.
// Each block fills a 256-entry fp32 table in LDS, one such division per
// thread, and converts by lookup: measured 5-13 % faster than sixteen
// divisions per lane (profiles/bair_cache.md).
//
// Pure store-bandwidth work, output bytes = 4x input bytes. A frame is F bytes
// = Q dwords (F % 16 == 0). A lane loads one dword (4 pixel bytes) and stores
// one 16-byte vector, so every load instruction of a wave reads 256 B and
// every store instruction writes 1 KB, both contiguous. A block of 256 lanes
// covers 1024 consecutive dwords of one frame (4 per lane, the loads issued
// before the first store). The frame comes from the block index alone:
// blockIdx.x = b, blockIdx.y = l - l0, blockIdx.z = the 1024-dword chunk.
// Source and destination offsets are 64-bit (the 64 px BAIR bank is 15.9 GB).
// No MFMA, no atomics.
//
// Contract (validated on the host by ops.clip_gather BEFORE launch):
// 0 <= idx < N, 1 <= L <= T, F % 16 == 0, bank contiguous and 16-byte aligned.

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int PER_LANE = 4;                        // dwords per lane
constexpr unsigned CHUNK = THREADS * PER_LANE;     // dwords per block
constexpr long GRID_YZ_MAX = 65535;

__global__ __launch_bounds__(THREADS) void clip_gather_kernel(
    const uint8_t* __restrict__ bank,  // (N, T, F)
    const int* __restrict__ idx,       // (B)
    float* __restrict__ out,           // (L, B, F)
    int l0, int T, unsigned Q) {
  __shared__ float tab[256];  // THREADS == 256: one entry per thread
  tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
  __syncthreads();
  const long b = blockIdx.x;
  const long B = gridDim.x;
  const long l = (long)l0 + blockIdx.y;
  const long clip = idx[b];
  const long F = (long)Q * 4;  // bytes per source frame = floats per output frame
  const uint32_t* __restrict__ src =
      reinterpret_cast<const uint32_t*>(bank + (clip * T + l) * F);
  float4* __restrict__ dst = reinterpret_cast<float4*>(out + (l * B + b) * F);

  const unsigned q0 = blockIdx.z * CHUNK + threadIdx.x;
  uint32_t w[PER_LANE];
#pragma unroll
  for (int i = 0; i < PER_LANE; ++i) {
    const unsigned q = q0 + i * THREADS;
    w[i] = q < Q ? src[q] : 0u;
  }
#pragma unroll
  for (int i = 0; i < PER_LANE; ++i) {
    const unsigned q = q0 + i * THREADS;
    if (q < Q) {
      float4 v;
      v.x = tab[w[i] & 0xffu];
      v.y = tab[(w[i] >> 8) & 0xffu];
      v.z = tab[(w[i] >> 16) & 0xffu];
      v.w = tab[w[i] >> 24];
      dst[q] = v;
    }
  }
}

}  // namespace

// bank (N,T,H,W,C) u8 and idx (B) i32 on one device, contiguous ->
// (L,B,H,W,C) f32. The value range of idx is the caller's contract (see the
// header comment); shapes, dtypes, alignment and the range of L are checked.
torch::Tensor clip_gather(torch::Tensor bank, torch::Tensor idx, long L) {
  CHECK_INPUT(bank);
  CHECK_INPUT(idx);
  TORCH_CHECK(bank.scalar_type() == torch::kUInt8 && bank.dim() == 5,
              "clip_gather: bank must be (N,T,H,W,C) uint8");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.dim() == 1,
              "clip_gather: idx must be (B) int32");
  TORCH_CHECK(idx.device() == bank.device(),
              "clip_gather: bank and idx must be on one device");
  const long N = bank.size(0), T = bank.size(1);
  const long H = bank.size(2), W = bank.size(3), C = bank.size(4);
  const long F = H * W * C;
  TORCH_CHECK(N >= 1 && F >= 16 && F % 16 == 0,
              "clip_gather: N >= 1 and H*W*C a positive multiple of 16 required");
  TORCH_CHECK(L >= 1 && L <= T, "clip_gather: 1 <= L <= T required");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(bank.data_ptr()) % 16 == 0,
              "clip_gather: bank must be 16-byte aligned");
  const long B = idx.size(0);
  auto out = torch::empty({L, B, H, W, C},
                          bank.options().dtype(torch::kFloat32));
  if (B == 0) return out;
  const long Q = F / 4;
  const long chunks = (Q + CHUNK - 1) / CHUNK;
  // HIP limits gridDim.x * blockDim.x to 2^32 threads
  TORCH_CHECK(B <= (1L << 23), "clip_gather: batch too large");
  TORCH_CHECK(T <= 0x7fffffffL, "clip_gather: T too large");
  TORCH_CHECK(chunks <= GRID_YZ_MAX, "clip_gather: frame too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  // grid.y is limited to 65535: longer clips take several launches
  for (long l0 = 0; l0 < L; l0 += GRID_YZ_MAX) {
    const long nl = std::min(GRID_YZ_MAX, L - l0);
    hipLaunchKernelGGL(clip_gather_kernel,
                       dim3((unsigned)B, (unsigned)nl, (unsigned)chunks),
                       dim3(THREADS), 0, stream, bank.data_ptr<uint8_t>(),
                       idx.data_ptr<int>(), out.data_ptr<float>(), (int)l0,
                       (int)T, (unsigned)Q);
    C10_CUDA_KERNEL_LAUNCH_CHECK();
  }
  return out;
}
