// Ranger (RAdam + Lookahead + gradient centralisation) as a multi-tensor step: every tensor of an optimiser in one launch of
// ranger_step_kernel (plus one launch of ranger_long_row_means_kernel when a centralised row is longer than a tile).
//
// The host cuts every tensor into work items of at most GDRNPP_RANGER_TILE elements.  An item of a centralised tensor whose rows fit
// a tile is a run of WHOLE rows: the workgroup stages that piece of the gradient in LDS, one wave per row forms the row sum (fp64,
// lane l adds elements l, l + 64, ... in index order, then a xor butterfly: a fixed order that depends on the row length alone, not on
// the launch), subtracts the mean in place, and the update pass reads the centralised gradient back from LDS: g, p, m, v are each
// read once and p, m, v written once (+ slow on a Lookahead step).  A row longer than a tile gets its mean from the pre-pass kernel
// (one workgroup per row, the same fixed order with 256 partial sums), which reads that row's gradient a second time.
// 16-byte accesses where every pointer of the item allows them, dword accesses otherwise: the arithmetic per element is the same.
#include "common.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int kTile = GDRNPP_RANGER_TILE;
constexpr int kThreads = 512;
constexpr int kMeanThreads = 256;

struct Coef {
  float beta1, beta2, omb1, omb2, eps, alpha, wd_lr, step_lr;
  bool rect, look;
};

__device__ __forceinline__ float fix_nonfinite(float g) {      // torch.nan_to_num(g, nan=0, posinf=1e5, neginf=-1e5)
  if (g != g) return 0.f;
  if (g == __builtin_inff()) return 1.0e5f;
  if (g == -__builtin_inff()) return -1.0e5f;
  return g;
}

// one element of the reference's step(); the Makefile's -ffp-contract=off keeps every product and sum a rounding of its own
__device__ __forceinline__ void ranger_elem(float g, float& p, float& m, float& v, float& s, const Coef& c) {
  v = v * c.beta2 + (c.omb2 * g) * g;
  m = m * c.beta1 + c.omb1 * g;
  if (c.wd_lr != 0.f) p = p + c.wd_lr * p;
  if (c.rect) {
    const float denom = sqrtf(v) + c.eps;
    p = p + c.step_lr * (m / denom);
  } else {
    p = p + c.step_lr * m;
  }
  if (c.look) {
    s = s + c.alpha * (p - s);
    p = s;
  }
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) == 0; }

__global__ __launch_bounds__(kMeanThreads) void ranger_long_row_means_kernel(const gdrnpp_ranger_tensor* __restrict__ tensors,
                                                                             const gdrnpp_ranger_long_row* __restrict__ rows,
                                                                             float* __restrict__ means) {
  __shared__ double part[kMeanThreads];
  const gdrnpp_ranger_long_row r = rows[blockIdx.x];
  const gdrnpp_ranger_tensor& T = tensors[r.tensor];
  const long long L = T.row_len;
  const float* g = T.g + r.row * L;
  const bool fix = (T.flags & GDRNPP_RANGER_NAN_TO_NUM) != 0;
  double s = 0.0;
  for (long long i = threadIdx.x; i < L; i += kMeanThreads) {
    float x = g[i];
    if (fix) x = fix_nonfinite(x);
    s += (double)x;
  }
  const double total = gdrnpp::wave::block_sum_halving<kMeanThreads>(s, part);
  if (threadIdx.x == 0) means[blockIdx.x] = (float)(total / (double)L);
}

template <bool VEC>
__device__ __forceinline__ void update_pass(const gdrnpp_ranger_tensor& T, long long start, int count, const float* g_lds, float mean,
                                            bool fix, const Coef& c) {
  float* __restrict__ p = T.p + start;
  float* __restrict__ m = T.m + start;
  float* __restrict__ v = T.v + start;
  float* __restrict__ s = T.slow + start;      // touched on Lookahead steps only
  float* __restrict__ g = T.g + start;         // read here unless the item was staged; written only with NAN_TO_NUM
  const int tid = threadIdx.x;
  int done = 0;
  if (VEC) {
    const int n4 = count >> 2;
    for (int i = tid; i < n4; i += kThreads) {
      float4 gg;
      if (g_lds) {
        gg = reinterpret_cast<const float4*>(g_lds)[i];
      } else {
        gg = reinterpret_cast<const float4*>(g)[i];
        if (fix) {
          gg.x = fix_nonfinite(gg.x), gg.y = fix_nonfinite(gg.y), gg.z = fix_nonfinite(gg.z), gg.w = fix_nonfinite(gg.w);
          reinterpret_cast<float4*>(g)[i] = gg;
        }
        gg.x -= mean, gg.y -= mean, gg.z -= mean, gg.w -= mean;
      }
      float4 pp = reinterpret_cast<const float4*>(p)[i];
      float4 mm = reinterpret_cast<const float4*>(m)[i];
      float4 vv = reinterpret_cast<const float4*>(v)[i];
      float4 ss = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c.look) ss = reinterpret_cast<const float4*>(s)[i];
      ranger_elem(gg.x, pp.x, mm.x, vv.x, ss.x, c);
      ranger_elem(gg.y, pp.y, mm.y, vv.y, ss.y, c);
      ranger_elem(gg.z, pp.z, mm.z, vv.z, ss.z, c);
      ranger_elem(gg.w, pp.w, mm.w, vv.w, ss.w, c);
      reinterpret_cast<float4*>(p)[i] = pp;
      reinterpret_cast<float4*>(m)[i] = mm;
      reinterpret_cast<float4*>(v)[i] = vv;
      if (c.look) reinterpret_cast<float4*>(s)[i] = ss;
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < count; i += kThreads) {
    float gg;
    if (g_lds) {
      gg = g_lds[i];
    } else {
      gg = g[i];
      if (fix) {
        gg = fix_nonfinite(gg);
        g[i] = gg;
      }
      gg -= mean;
    }
    float pp = p[i], mm = m[i], vv = v[i], ss = c.look ? s[i] : 0.f;
    ranger_elem(gg, pp, mm, vv, ss, c);
    p[i] = pp, m[i] = mm, v[i] = vv;
    if (c.look) s[i] = ss;
  }
}

__global__ __launch_bounds__(kThreads) void ranger_step_kernel(const gdrnpp_ranger_tensor* __restrict__ tensors,
                                                              const gdrnpp_ranger_work* __restrict__ work,
                                                              const float* __restrict__ long_means) {
  __shared__ __attribute__((aligned(16))) float tile[kTile];
  const gdrnpp_ranger_work w = work[blockIdx.x];
  const gdrnpp_ranger_tensor& T = tensors[w.tensor];
  const long long start = w.start;
  const int count = w.count < kTile ? w.count : kTile;      // the tile is never overrun, whatever the table says
  const int flags = T.flags;
  const bool fix = (flags & GDRNPP_RANGER_NAN_TO_NUM) != 0;
  Coef c;
  c.beta1 = T.beta1, c.beta2 = T.beta2, c.omb1 = T.one_minus_beta1, c.omb2 = T.one_minus_beta2, c.eps = T.eps, c.alpha = T.alpha;
  c.wd_lr = T.wd_lr, c.step_lr = T.step_lr;
  c.rect = (flags & GDRNPP_RANGER_RECTIFIED) != 0;
  c.look = (flags & GDRNPP_RANGER_LOOKAHEAD) != 0;

  const int L = T.row_len;
  const bool staged = L > 0 && L <= kTile && w.mean_slot < 0;
  float mean = 0.f;
  if (L > 0 && !staged && w.mean_slot >= 0) mean = long_means[w.mean_slot];

  const float* g_lds = nullptr;
  if (staged) {
    float* __restrict__ g = T.g + start;
    const int tid = threadIdx.x;
    int done = 0;
    if (aligned16(g)) {
      const int n4 = count >> 2;
      for (int i = tid; i < n4; i += kThreads) {
        float4 x = reinterpret_cast<const float4*>(g)[i];
        if (fix) {
          x.x = fix_nonfinite(x.x), x.y = fix_nonfinite(x.y), x.z = fix_nonfinite(x.z), x.w = fix_nonfinite(x.w);
          reinterpret_cast<float4*>(g)[i] = x;
        }
        reinterpret_cast<float4*>(tile)[i] = x;
      }
      done = n4 << 2;
    }
    for (int i = done + tid; i < count; i += kThreads) {
      float x = g[i];
      if (fix) {
        x = fix_nonfinite(x);
        g[i] = x;
      }
      tile[i] = x;
    }
    __syncthreads();
    const int rows = count / L, lane = tid & (gdrnpp::kWave - 1);
    for (int r = tid / gdrnpp::kWave; r < rows; r += kThreads / gdrnpp::kWave) {
      float* row = tile + r * L;
      double s = 0.0;
      for (int i = lane; i < L; i += gdrnpp::kWave) s += (double)row[i];
      const float mu = (float)(gdrnpp::wave::wave_sum_ascending(s) / (double)L);   // every lane receives the same bits
      for (int i = lane; i < L; i += gdrnpp::kWave) row[i] -= mu;
    }
    __syncthreads();
    g_lds = tile;
  }

  bool vec = aligned16(T.p + start) && aligned16(T.m + start) && aligned16(T.v + start);
  if (!staged) vec = vec && aligned16(T.g + start);
  if (c.look) vec = vec && aligned16(T.slow + start);
  if (vec)
    update_pass<true>(T, start, count, g_lds, mean, fix, c);
  else
    update_pass<false>(T, start, count, g_lds, mean, fix, c);
}

}  // namespace

extern "C" int gdrnpp_ranger_step(const gdrnpp_ranger_tensor* tensors, int n_tensors, const gdrnpp_ranger_work* work, int n_work,
                                  const gdrnpp_ranger_long_row* long_rows, int n_long_rows, float* long_means, void* stream) {
  static_assert(sizeof(gdrnpp_ranger_tensor) == 96 && sizeof(gdrnpp_ranger_work) == 24 && sizeof(gdrnpp_ranger_long_row) == 16,
                "the table layouts are part of the ABI");
  GDRNPP_REQUIRE(n_tensors >= 0 && n_work >= 0 && n_long_rows >= 0, GDRNPP_EINVAL, "gdrnpp_ranger_step: negative count");
  if (n_work == 0) return 0;
  GDRNPP_REQUIRE(tensors && work && n_tensors > 0, GDRNPP_EINVAL, "gdrnpp_ranger_step: work without tables");
  GDRNPP_REQUIRE(n_long_rows == 0 || (long_rows && long_means), GDRNPP_EINVAL, "gdrnpp_ranger_step: long rows without their buffers");
  hipStream_t st = (hipStream_t)stream;
  if (n_long_rows > 0) {
    hipLaunchKernelGGL(ranger_long_row_means_kernel, dim3(n_long_rows), dim3(kMeanThreads), 0, st, tensors, long_rows, long_means);
    if (int rc = gdrnpp::check_launch("gdrnpp_ranger_step (row means)")) return rc;
  }
  hipLaunchKernelGGL(ranger_step_kernel, dim3(n_work), dim3(kThreads), 0, st, tensors, work, (const float*)long_means);
  return gdrnpp::check_launch("gdrnpp_ranger_step");
}
