// Shared helpers for the libsrk kernels (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include <type_traits>
#include "../../include/srk.h"

namespace srk {

void set_error(const char* fmt, ...);
// Records the kernel a conv entry point just launched (thread-local; read back through srk_last_kernel_name()) so that
// measurements can name the kernel that actually ran instead of guessing it from the shape.
void note_kernel(const char* fmt, ...);
// A conv launcher whose kernel keeps the running maximum of what it stores (srk_epilogue.y_amax) says so here; read back
// through srk_last_conv_wrote_amax().  Reset by every srk_conv2d_forward call.
void note_amax_written(bool written);
// ... and a launcher that filled srk_epilogue.bn_partial says how many rows (srk_last_conv_bn_partial_rows()).
void note_bn_partial_rows(int rows);

// Environment switches.  env_int / env_str read a variable ONCE per process and answer from a table
// afterwards -- a dispatch must not pay getenv's environment scan -- unless SRK_ENV_LIVE is set when the library is first
// used: the test-suite flips switches between calls of one process (tests/conftest.py sets it).
const char* env_str(const char* name);
int env_int(const char* name, int dflt);
// Ablations and timing probes are patches of a throwaway copy of csrc/ (tools/build_variant.sh), never a
// switch in these kernels.  Not only dead code: a run-time `if (dbg & 4)` around a kernel's MFMA loop and its stores gives
// the compiler's s_waitcnt pass a path on which the stores were never issued, and the waits for loads issued before them
// then assume the worst (k_conv_rowsw: s_waitcnt vmcnt(7..0) instead of vmcnt(15..8) in front of the staging commit =
// every stage waited for the write acknowledgements of its own eight stores).

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return SRK_ERR_LAUNCH;
  }
  return SRK_OK;
}

#define SRK_REQUIRE(cond, ...)          \
  do {                                  \
    if (!(cond)) {                      \
      ::srk::set_error(__VA_ARGS__);    \
      return SRK_ERR_BAD_ARG;           \
    }                                   \
  } while (0)

constexpr int kWave = 64;
typedef float f32x4 __attribute__((ext_vector_type(4)));
// Compute units of the current device (MI355X: 256), asked once per device: grids of the persistent kernels and the
// small- / large-problem thresholds follow the part the library runs on instead of a compile-time constant.
inline int num_cu() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cached[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    n = 256;
  }
  cached[dev].store(n, std::memory_order_relaxed);
  return n;
}
#define kNumCU (::srk::num_cu())
constexpr int kMaxDynLds = 160 * 1024;  // gfx950: 160 KB of LDS per CU, all of it usable by one workgroup

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE property of a kernel.  A kernel that may need more than the
// 64 KB default is launched through launch_lds (below), which owns one `static LdsLimit` per kernel instantiation and
// calls ensure() before launching: the limit is raised to the hardware maximum once per (kernel, device).  Thread-safe (relaxed atomics; a race only repeats an idempotent host call), so the
// main and the autograd threads — or several devices driven from one process — can launch concurrently.
struct LdsLimit {
  static constexpr int kMaxDevices = 64;
  std::atomic<unsigned char> done[kMaxDevices];
  LdsLimit() {
    for (int i = 0; i < kMaxDevices; ++i) done[i].store(0, std::memory_order_relaxed);
  }
  void ensure(const void* fn, size_t lds) {
    if (lds <= 48 * 1024) return;  // under the default limit: nothing to raise
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < kMaxDevices && done[dev].load(std::memory_order_relaxed)) return;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds) != hipSuccess) {
      // (a kernel that also has static LDS cannot take the full 160 KB as dynamic: ask for what this launch needs)
      (void)hipGetLastError();
      (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      return;
    }
    if (dev >= 0 && dev < kMaxDevices) done[dev].store(1, std::memory_order_relaxed);
  }
};

// Launches kernel K with `lds` bytes of dynamic LDS, raising K's limit first where needed.  The kernel is named once, so
// the instantiation whose limit is raised is the one that is launched.
template <auto K, typename... A>
inline void launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
  static LdsLimit lim;  // one per kernel instantiation
  lim.ensure(reinterpret_cast<const void*>(K), lds);
  hipLaunchKernelGGL(K, grid, block, lds, s, args...);
}

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// Blocks of a grid-stride streaming kernel: one per `per_block` items, at least 1, at most `cap`.
inline unsigned grid_for(size_t items, size_t per_block, size_t cap) {
  const size_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// Every pointer on a 16-byte boundary (NULL counts as aligned): the condition of a kernel's 16-byte form.
template <typename... P>
__host__ __device__ __forceinline__ bool aligned16(const P*... p) {
  return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// V consecutive floats as one access: the 4-byte and the 16-byte form of a streaming kernel are one template over V.
// load / store index in units of V floats.
template <int V>
struct Vec;
template <>
struct Vec<4> {
  typedef f32x4 T;
  static __device__ __forceinline__ T load(const float* p, size_t i) { return reinterpret_cast<const T*>(p)[i]; }
  static __device__ __forceinline__ void store(float* p, size_t i, const T& v) { reinterpret_cast<T*>(p)[i] = v; }
  static __device__ __forceinline__ float at(const T& v, int k) { return v[k]; }
  static __device__ __forceinline__ void set(T& v, int k, float x) { v[k] = x; }
};
template <>
struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ T load(const float* p, size_t i) { return p[i]; }
  static __device__ __forceinline__ void store(float* p, size_t i, const T& v) { p[i] = v; }
  static __device__ __forceinline__ float at(const T& v, int) { return v; }
  static __device__ __forceinline__ void set(T& v, int, float x) { v = x; }
};

// Element strides of a [N][C][H][W] tensor in any layout; passed to kernels by value.
struct Strides4 {
  int64_t n, c, h, w;
};
inline Strides4 strides4(const int64_t* s) { return {s[0], s[1], s[2], s[3]}; }

// XCD-aware tile index: hardware deals consecutive block ids round-robin over the 8 XCDs (each with its own L2); this maps
// block `bx` of `nb` to a tile index such that every XCD walks a CONTIGUOUS range of tiles -- neighbouring tiles share
// their halo in ONE L2 instead of fetching it once per L2.  A bijection on [0, nb) for any nb.
__device__ __forceinline__ int xcd_tile_index(int bx, int nb) {
  const int per = nb >> 3, rem = nb & 7;
  const int xcd = bx & 7, idx = bx >> 3;
  return xcd < rem ? xcd * (per + 1) + idx : rem * (per + 1) + (xcd - rem) * per + idx;
}

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [I0, I1)
template <int I0, int I1, typename F>
__device__ __forceinline__ void srk_static_for(F&& f) {
  if constexpr (I0 < I1) {
    f(std::integral_constant<int, I0>{});
    srk_static_for<I0 + 1, I1>(f);
  }
}

// Buffer descriptor over [base, base + bytes) built from wave-uniform values (the readfirstlane makes the uniformity
// provable: no waterfall loop around the accesses); an offset outside the range reads zero and stores nothing.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  void* p = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(p, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// fp32 MFMA, 16 x 16 x 4
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Activation forward on a scalar. `a` is the negative-side slope for PReLU / LeakyReLU.
__device__ __forceinline__ float act_apply(float v, int act, float a) {
  switch (act) {
    case SRK_ACT_RELU: return v > 0.f ? v : 0.f;
    case SRK_ACT_PRELU:
    case SRK_ACT_LRELU: return v > 0.f ? v : a * v;
    case SRK_ACT_TANH: return tanhf(v);
    case SRK_ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    default: return v;
  }
}

// Sum over the 64 lanes of a wave; every lane gets the total.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide sum for blockDim.x == 256 (4 waves). `sm` needs 4 floats. All threads get the total.
__device__ __forceinline__ float block_sum_256(float v, float* sm) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}
__device__ __forceinline__ double block_sum_256_d(double v, double* sm) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// The two halves of a reduction through per-block partials (blocks of 256 threads, `sm` = 4 doubles).
// Tail of a partial kernel: the block's sum of v, stored to *slot by thread 0.
__device__ __forceinline__ void store_block_sum_256_d(double v, double* sm, double* __restrict__ slot) {
  const double tot = block_sum_256_d(v, sm);
  if (threadIdx.x == 0) *slot = tot;
}
// One-block final: the sum of partials[i * stride], i < nparts, in a fixed order (thread t adds i = t, t + 256, ...; then
// the block sum).  All threads get the total.
__device__ __forceinline__ double sum_partials_256_d(const double* __restrict__ partials, int nparts, double* sm,
                                                     int stride = 1) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += partials[(size_t)i * stride];
  return block_sum_256_d(acc, sm);
}

}  // namespace srk

