// Pose scoring for best-of-N evaluation of skeleton sequences (K20).
//
// gen (T, S, B, J, 3): S generated samples per sequence; ref (T, B, J, 3): the
// ground truth; w = (w0, w1, w2) > 0: per-axis scales. Both operands dense,
// fp32 / bf16 / fp16 each, converted to fp32 exactly at load. A difference is
// formed first, in fp32, and scaled afterwards.
//
//   d               = f32(gen[t,s,b,j,:]) - f32(ref[t,b,j,:])
//   mpjpe[s,t,b]    = (1/J)  sum_j sqrt(sum_a (w_a * d_a)^2)
//   mse[s,t,b]      = (1/3J) sum_{j,a} d_a^2              (unscaled)
//   spread[t,b]     = 1/(P J) sum_{i<j} sum_joint
//                     sqrt(sum_a (w_a * (gen_i - gen_j)_a)^2),  P = S(S-1)/2
//
// pose_metrics: one read of gen and ref, memory-bound. For a fixed (t, s) the
// frames of consecutive b are one contiguous run, in gen and (for that t) in
// ref, so a 256-thread block owns (t, s, nb consecutive b) and works in three
// steps:
//
//   1  element e of the run: lane-consecutive loads of gen and ref, the fp32
//      difference -> LDS. A frame is 3J elements (204 B at J = 17) and only
//      element-aligned, so loads are one element per lane: a wave reads 256
//      contiguous bytes of fp32 per instruction, and no lane strides a frame.
//   2  joint q of the run: its three differences from LDS (lane stride 3
//      dwords, conflict-free) -> scaled length and squared length -> LDS
//   3  frame b: its J lengths and squares summed in joint order by one thread
//
// The tile is TILE_Q = 1024 joints: nb = min(1024 / J, 256) frames, 20 KiB of
// LDS. J > 1024: one frame per block, its joints in chunks of 1024, the
// frame's thread carrying the two sums across chunks (still joint order).
// ref is indexed (t, b) in the kernel: never broadcast in memory.
//
// pose_spread: a block stages the S samples of one t for nb <= 4 consecutive
// b in LDS (per sample one contiguous run of nb*3J elements, placed at an odd
// dword stride so that lanes = consecutive samples hit distinct banks), then
// per frame splits the P unordered pairs over its 256 threads. Pair q is
// (i, (i + k) mod S) with k = q / S + 1, i = q mod S: offsets k = 1 .. S/2
// visit every unordered pair once, consecutive lanes take consecutive i.
// A thread adds its pairs in ascending q (each pair: joints in order), a
// shuffle tree folds a wave, thread 0 adds the four wave sums in order: no
// atomics, and a frame's result does not depend on nb, B or the grid.
// LDS budget: S * stride * 4 <= 56 KiB with stride = (nb*3J) | 1. At nb = 1
// that holds whenever S * J <= SPREAD_MAX_SJ = 4096 (12,288 floats plus at most
// 2,048 of padding), the documented limit: S <= 240 at J = 17. The default
// protocol (S = 100, J = 17) stages nb = 2 frames, 41,200 B, in one launch.
//
// Both: 64-bit offsets; every load is inside a run that ends at or before the
// operand's last element; same inputs, same bits.

#include <c10/cuda/CUDAException.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int NWAVES = THREADS / WAVE;
constexpr int TILE_Q = 1024;             // joints of a pose_metrics tile
constexpr int SPREAD_MAX_NB = 4;         // frames staged per pose_spread block
constexpr long SPREAD_MAX_SJ = 4096;     // largest S * J of pose_spread
constexpr long SPREAD_LDS_FLOATS = 14336;  // 56 KiB

struct Scale {
  float w0, w1, w2;
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

__device__ __forceinline__ float scaled_length(float dx, float dy, float dz,
                                               const Scale& w) {
  const float sx = w.w0 * dx, sy = w.w1 * dy, sz = w.w2 * dz;
  return sqrtf(sx * sx + sy * sy + sz * sz);
}

template <int DG, int DR>
__global__ __launch_bounds__(THREADS) void pose_metrics_kernel(
    const void* __restrict__ gen, const void* __restrict__ ref, long T, long S,
    long B, int J, int nb, long tiles_b, Scale w,
    float* __restrict__ mpjpe,  // (S, T, B)
    float* __restrict__ mse) {  // (S, T, B)
  __shared__ float s_d[3 * TILE_Q];
  __shared__ float s_len[TILE_Q];
  __shared__ float s_sq[TILE_Q];

  const int tid = threadIdx.x;
  const long bid = blockIdx.x;
  const long row = bid / tiles_b;  // t * S + s
  const long b0 = (bid - row * tiles_b) * nb;
  const long t = row / S;
  const long s = row - t * S;
  const int nbt = (int)min((long)nb, B - b0);
  const long F = 3L * J;
  const long g0 = (row * B + b0) * F;
  const long r0 = (t * B + b0) * F;

  float acc_len = 0.f, acc_sq = 0.f;  // of frame b0 + tid
  // one pass unless J > TILE_Q; then nb == 1 and the run is the frame itself,
  // so in both cases chunk element e sits at 3 * j0 + e of the run
  for (int j0 = 0; j0 < J; j0 += TILE_Q) {
    const int jc = min(TILE_Q, J - j0);
    const int nq = nbt * jc;
    for (int e = tid; e < 3 * nq; e += THREADS) {
      const long o = 3L * j0 + e;
      s_d[e] = load_f32<DG>(gen, g0 + o) - load_f32<DR>(ref, r0 + o);
    }
    __syncthreads();
    for (int q = tid; q < nq; q += THREADS) {
      const float dx = s_d[3 * q], dy = s_d[3 * q + 1], dz = s_d[3 * q + 2];
      s_len[q] = scaled_length(dx, dy, dz, w);
      s_sq[q] = dx * dx + dy * dy + dz * dz;
    }
    __syncthreads();
    if (tid < nbt) {
      for (int j = 0; j < jc; ++j) {
        acc_len += s_len[tid * jc + j];
        acc_sq += s_sq[tid * jc + j];
      }
    }
    __syncthreads();  // the next chunk rewrites all three arrays
  }
  if (tid < nbt) {
    const long o = (s * T + t) * B + b0 + tid;
    mpjpe[o] = acc_len / (float)J;
    mse[o] = acc_sq / (float)(3 * J);
  }
}

template <int DG>
__global__ __launch_bounds__(THREADS) void pose_spread_kernel(
    const void* __restrict__ gen, int S, long B, int J, int nb, long tiles_b,
    int ld, Scale w, float count,
    float* __restrict__ spread) {  // (T, B)
  extern __shared__ __attribute__((aligned(16))) float s_pose[];  // S * ld
  __shared__ float s_red[NWAVES];

  const int tid = threadIdx.x;
  const long bid = blockIdx.x;
  const long t = bid / tiles_b;
  const long b0 = (bid - t * tiles_b) * nb;
  const int nbt = (int)min((long)nb, B - b0);
  const int F = 3 * J;
  const int run = nbt * F;  // <= ld

  // stage: sample s = the run of nbt frames at ((t * S + s) * B + b0) * F
  for (int idx = tid; idx < S * run; idx += THREADS) {
    const int s = idx / run;
    const int e = idx - s * run;
    s_pose[s * ld + e] = load_f32<DG>(gen, ((t * S + s) * B + b0) * F + e);
  }
  __syncthreads();

  const int P = S * (S - 1) / 2;
  for (int bl = 0; bl < nbt; ++bl) {
    float acc = 0.f;
    for (int q = tid; q < P; q += THREADS) {
      const int k = q / S;  // offset k + 1
      const int i = q - k * S;
      int j = i + k + 1;
      if (j >= S) j -= S;
      const float* pi = s_pose + i * ld + bl * F;
      const float* pj = s_pose + j * ld + bl * F;
      float sum = 0.f;
      for (int c = 0; c < F; c += 3)
        sum += scaled_length(pi[c] - pj[c], pi[c + 1] - pj[c + 1],
                             pi[c + 2] - pj[c + 2], w);
      acc += sum;
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, WAVE);
    if ((tid & (WAVE - 1)) == 0) s_red[tid / WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
      float total = 0.f;
#pragma unroll
      for (int v = 0; v < NWAVES; ++v) total += s_red[v];
      spread[t * B + b0 + bl] = total / count;
    }
    __syncthreads();  // s_red is rewritten for the next frame
  }
}

int dtype_code(const torch::Tensor& t, const char* op, const char* name) {
  switch (t.scalar_type()) {
    case torch::kFloat32: return DT_F32;
    case torch::kBFloat16: return DT_BF16;
    case torch::kFloat16: return DT_F16;
    default:
      TORCH_CHECK(false, op, ": ", name, " must be fp32, bf16 or fp16");
  }
  return -1;
}

Scale scale_of(double w0, double w1, double w2, const char* op) {
  TORCH_CHECK(w0 > 0 && w1 > 0 && w2 > 0, op, ": axis scales must be > 0");
  return Scale{(float)w0, (float)w1, (float)w2};
}

}  // namespace

long pose_spread_max_sj() { return SPREAD_MAX_SJ; }

// gen (T,S,B,J,3), ref (T,B,J,3): contiguous, fp32 / bf16 / fp16 each, one
// device. Returns {mpjpe (S,T,B) f32, mse (S,T,B) f32}.
std::vector<torch::Tensor> pose_metrics(torch::Tensor gen, torch::Tensor ref,
                                        double w0, double w1, double w2) {
  CHECK_INPUT(gen);
  CHECK_INPUT(ref);
  TORCH_CHECK(gen.device() == ref.device(),
              "pose_metrics: gen and ref must be on one device");
  TORCH_CHECK(gen.dim() == 5 && ref.dim() == 4 && gen.size(4) == 3 &&
                  ref.size(3) == 3,
              "pose_metrics: gen must be (T,S,B,J,3) and ref (T,B,J,3)");
  const long T = gen.size(0), S = gen.size(1), B = gen.size(2),
             J = gen.size(3);
  TORCH_CHECK(ref.size(0) == T && ref.size(1) == B && ref.size(2) == J,
              "pose_metrics: gen and ref differ in T, B or J");
  TORCH_CHECK(J >= 1 && J <= (1L << 22), "pose_metrics: 1 <= J <= 2^22");
  const int dg = dtype_code(gen, "pose_metrics", "gen");
  const int dr = dtype_code(ref, "pose_metrics", "ref");
  const Scale w = scale_of(w0, w1, w2, "pose_metrics");

  auto opts = gen.options().dtype(torch::kFloat32);
  auto mpjpe = torch::empty({S, T, B}, opts);
  auto mse = torch::empty({S, T, B}, opts);
  if (T * S * B == 0) return {mpjpe, mse};

  const long nb = std::max(1L, std::min((long)TILE_Q / J, (long)THREADS));
  const long tiles_b = (B + nb - 1) / nb;
  const long blocks = T * S * tiles_b;
  TORCH_CHECK(blocks < (1L << 31), "pose_metrics: too many frames for a launch");

  auto stream = at::cuda::getCurrentCUDAStream();
#define PM_LAUNCH(DG, DR)                                                     \
  hipLaunchKernelGGL((pose_metrics_kernel<DG, DR>), dim3((unsigned)blocks),   \
                     dim3(THREADS), 0, stream, gen.data_ptr(), ref.data_ptr(), \
                     T, S, B, (int)J, (int)nb, tiles_b, w,                    \
                     mpjpe.data_ptr<float>(), mse.data_ptr<float>())
#define PM_DISPATCH_R(DG)                      \
  switch (dr) {                                \
    case DT_F32: PM_LAUNCH(DG, DT_F32); break; \
    case DT_BF16: PM_LAUNCH(DG, DT_BF16); break; \
    default: PM_LAUNCH(DG, DT_F16); break;     \
  }
  switch (dg) {
    case DT_F32: PM_DISPATCH_R(DT_F32); break;
    case DT_BF16: PM_DISPATCH_R(DT_BF16); break;
    default: PM_DISPATCH_R(DT_F16); break;
  }
#undef PM_DISPATCH_R
#undef PM_LAUNCH
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {mpjpe, mse};
}

// gen (T,S,B,J,3) contiguous, fp32 / bf16 / fp16, S >= 2, S * J <=
// SPREAD_MAX_SJ. Returns spread (T,B) f32.
torch::Tensor pose_spread(torch::Tensor gen, double w0, double w1, double w2) {
  CHECK_INPUT(gen);
  TORCH_CHECK(gen.dim() == 5 && gen.size(4) == 3,
              "pose_spread: gen must be (T,S,B,J,3)");
  const long T = gen.size(0), S = gen.size(1), B = gen.size(2),
             J = gen.size(3);
  TORCH_CHECK(S >= 2, "pose_spread: S >= 2 required");
  TORCH_CHECK(J >= 1 && S * J <= SPREAD_MAX_SJ, "pose_spread: S * J = ", S * J,
              " exceeds ", SPREAD_MAX_SJ);
  const int dg = dtype_code(gen, "pose_spread", "gen");
  const Scale w = scale_of(w0, w1, w2, "pose_spread");

  auto spread = torch::empty({T, B}, gen.options().dtype(torch::kFloat32));
  if (T * B == 0) return spread;

  // the most frames (<= SPREAD_MAX_NB) whose padded samples fit the budget;
  // nb = 1 always does (see the header)
  const long F = 3 * J;
  long nb = std::min((long)SPREAD_MAX_NB, B);
  while (nb > 1 && S * ((nb * F) | 1) > SPREAD_LDS_FLOATS) --nb;
  const long ld = (nb * F) | 1;
  TORCH_CHECK(S * ld <= SPREAD_LDS_FLOATS, "pose_spread: LDS budget exceeded");
  const long tiles_b = (B + nb - 1) / nb;
  const long blocks = T * tiles_b;
  TORCH_CHECK(blocks < (1L << 31), "pose_spread: too many frames for a launch");
  const size_t lds = (size_t)(S * ld) * sizeof(float);
  const float count = (float)(S * (S - 1) / 2 * J);  // < 2^24: exact

  auto stream = at::cuda::getCurrentCUDAStream();
#define PS_LAUNCH(DG)                                                         \
  hipLaunchKernelGGL((pose_spread_kernel<DG>), dim3((unsigned)blocks),        \
                     dim3(THREADS), lds, stream, gen.data_ptr(), (int)S, B,   \
                     (int)J, (int)nb, tiles_b, (int)ld, w, count,             \
                     spread.data_ptr<float>())
  switch (dg) {
    case DT_F32: PS_LAUNCH(DT_F32); break;
    case DT_BF16: PS_LAUNCH(DT_BF16); break;
    default: PS_LAUNCH(DT_F16); break;
  }
#undef PS_LAUNCH
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return spread;
}
