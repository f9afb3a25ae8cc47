// ModelEMA's update as a multi-tensor step: every floating-point (EMA, model) pair of a model in one launch of model_ema_kernel.
//
// The host cuts every tensor into work items of at most GDRNPP_EMA_TILE elements, one workgroup each.  A pure stream: e and m are read
// once, e is written once, 12 bytes per element, no LDS and no reuse.  A full, 16-byte aligned tile (all but the tail of a large tensor:
// nearly every byte of a detector) takes the straight-line path, four 16-byte loads of each operand in flight per lane before the first
// store; any other item takes the loop, with 16-byte accesses plus a dword tail where both pointers allow them and dword accesses
// where not (views).  The arithmetic per element is the same on every path.
#include <cstddef>

#include "common.hpp"

// elements per work item of the host's plan (hip_lib/net.py EMA_TILE, which tests/test_model_ema_cpu.py holds to this line): such an
// item, 16-byte aligned, takes the straight-line path.  The kernel is correct for any count.
#define GDRNPP_EMA_TILE 8192

namespace {

// the records of the two device tables (include/gdrnpp_hip.h describes them; hip_lib/net.py EMA_TENSOR / EMA_WORK builds them)
struct EmaTensor {
  float* ema;
  const float* model;
  long long numel;
};
struct EmaWork {
  long long start;
  int tensor;
  int count;
};
static_assert(sizeof(EmaTensor) == 24 && offsetof(EmaTensor, ema) == 0 && offsetof(EmaTensor, model) == 8 && offsetof(EmaTensor, numel) == 16,
              "the table layouts are part of the ABI");
static_assert(sizeof(EmaWork) == 16 && offsetof(EmaWork, start) == 0 && offsetof(EmaWork, tensor) == 8 && offsetof(EmaWork, count) == 12,
              "the table layouts are part of the ABI");

constexpr int kTile = GDRNPP_EMA_TILE;
constexpr int kThreads = 256;
constexpr int kBatch = 4;                                  // 16-byte loads of each operand in flight per lane on the full-tile path
static_assert(kTile % (4 * kThreads * kBatch) == 0, "a full tile is a whole number of batches");

// The pointers come out of a table in memory, so the compiler cannot tell that they are global and would use flat accesses: said
// here, they are global_load / global_store.
typedef float vec4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) vec4 gvec4;

// one element of the reference's `v *= d; v += (1.0 - d) * m`: two products and a sum, each rounded on its own (the Makefile's
// -ffp-contract=off holds for the whole file; the intrinsics say it again where it matters)
__device__ __forceinline__ float ema_elem(float e, float m, float d, float omd) { return __fadd_rn(__fmul_rn(e, d), __fmul_rn(omd, m)); }

__device__ __forceinline__ vec4 ema_elem4(vec4 e, vec4 m, float d, float omd) {
  vec4 r;
  r.x = ema_elem(e.x, m.x, d, omd), r.y = ema_elem(e.y, m.y, d, omd), r.z = ema_elem(e.z, m.z, d, omd), r.w = ema_elem(e.w, m.w, d, omd);
  return r;
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) == 0; }

__global__ __launch_bounds__(kThreads) void model_ema_kernel(const EmaTensor* __restrict__ tensors, int n_tensors,
                                                            const EmaWork* __restrict__ work, float d, float omd) {
  const EmaWork w = work[blockIdx.x];
  if (w.tensor < 0 || w.tensor >= n_tensors) return;
  const EmaTensor T = tensors[w.tensor];
  if (w.start < 0 || w.start >= T.numel || w.count <= 0) return;
  const long long left = T.numel - w.start;
  const int count = (long long)w.count > left ? (int)left : w.count;      // an item never leaves its tensor, whatever the table says
  const bool vec = aligned16(T.ema + w.start) && aligned16(T.model + w.start);
  gfloat* e = (gfloat*)(T.ema + w.start);
  const gfloat* m = (const gfloat*)(T.model + w.start);
  gvec4* e4 = (gvec4*)e;                                   // dereferenced only where vec holds
  const gvec4* m4 = (const gvec4*)m;
  const int tid = threadIdx.x;

  if (vec && count == kTile) {
#pragma unroll
    for (int base = 0; base < kTile / 4; base += kThreads * kBatch) {
      vec4 ee[kBatch], mm[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        ee[j] = e4[base + j * kThreads + tid];
        mm[j] = m4[base + j * kThreads + tid];
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) e4[base + j * kThreads + tid] = ema_elem4(ee[j], mm[j], d, omd);
    }
    return;
  }
  int done = 0;
  if (vec) {
    const int n4 = count >> 2;
    for (int i = tid; i < n4; i += kThreads) e4[i] = ema_elem4(e4[i], m4[i], d, omd);
    done = n4 << 2;
  }
  for (int i = done + tid; i < count; i += kThreads) e[i] = ema_elem(e[i], m[i], d, omd);
}

}  // namespace

extern "C" int gdrnpp_model_ema_update(const void* tensors, int n_tensors, const void* work, int n_work, float decay, float one_minus_decay,
                                       void* stream) {
  GDRNPP_REQUIRE(n_tensors >= 0 && n_work >= 0, GDRNPP_EINVAL, "gdrnpp_model_ema_update: negative count");
  if (n_work == 0) return 0;
  GDRNPP_REQUIRE(tensors && work && n_tensors > 0, GDRNPP_EINVAL, "gdrnpp_model_ema_update: work without tables");
  hipLaunchKernelGGL(model_ema_kernel, dim3(n_work), dim3(kThreads), 0, (hipStream_t)stream, (const EmaTensor*)tensors, n_tensors,
                     (const EmaWork*)work, decay, one_minus_decay);
  return gdrnpp::check_launch("gdrnpp_model_ema_update");
}
