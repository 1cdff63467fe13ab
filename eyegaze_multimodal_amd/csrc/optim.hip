// Optimiser step over the FLAT parameter / gradient buffers (T:221-222, T:401-405):
//   global L2 norm -> clip coefficient (device resident, no host sync) -> AdamW (decoupled weight decay).
// HBM-bound: one pass reads g, p, m, v and writes p, m, v (28 B/param).
#include "common.h"

namespace {

// one block's squared-norm partial (256 threads; the value is returned to thread 0)
__device__ __forceinline__ float sqnorm_block(const float* __restrict__ g, long long n, float* red) {
  float s = 0.f;
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      const f32x4 v = *(const f32x4*)(g + i);
      s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    } else {
      for (long long j = i; j < n; ++j) s += g[j] * g[j];
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, long long n,
                                                             float* __restrict__ partial) {
  __shared__ float red[4];
  const float s = sqnorm_block(g, n, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the n partials -> global norm, clip coefficient and overflow flag of the step state (one block of 256 threads)
__device__ __forceinline__ void clip_coef_block(const float* partial, int n, float max_norm, eg_step_state* st, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float ls = st->scaler_on ? st->loss_scale : 1.0f;
    const float norm = (float)sqrt(red[0]) * (st->grad_scale / ls);
    st->grad_norm = norm;
    float coef = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.0f;
    st->clip_coef = fminf(coef, 1.0f);
    st->found_inf = (st->scaler_on && !(fabsf(norm) <= 3.0e38f)) ? 1u : 0u;   // inf or NaN
  }
}

__global__ void clip_coef_kernel(const float* __restrict__ partial, int n, float max_norm, eg_step_state* st) {
  __shared__ double red[256];
  clip_coef_block(partial, n, max_norm, st, red);
}

// sqnorm_partial_kernel + clip_coef_kernel in one launch: every block leaves its partial, and the block that finishes LAST (a
// device counter tells it; nobody waits for anybody) does clip_coef_kernel's sums over all of them and clears the counter for the
// next launch.  Same thread-to-element map, same partials, same double-precision tree: the state fields get the same bits.
__global__ __launch_bounds__(256) void sqnorm_clip_kernel(const float* __restrict__ g, long long n, float* partial,
                                                          float max_norm, eg_step_state* st, unsigned* counter) {
  __shared__ float red[4];
  __shared__ double dred[256];
  __shared__ bool last_s;
  const float s = sqnorm_block(g, n, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s;
    __threadfence();
    last_s = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last_s) return;
  __threadfence();
  clip_coef_block(partial, (int)gridDim.x, max_norm, st, dred);
  if (threadIdx.x == 0) *counter = 0u;
}

__global__ void set_step_state_kernel(eg_step_state* st, uint32_t seed_lo, uint32_t seed_hi, float lr, float bc1, float bc2,
                                      float grad_scale, int reset_scaler, float init_scale, int use_dev_t) {
  st->seed_lo = seed_lo; st->seed_hi = seed_hi; st->lr = lr; st->bias_corr1 = bc1; st->bias_corr2 = bc2;
  st->grad_scale = grad_scale; st->use_dev_t = (uint32_t)use_dev_t;
  if (reset_scaler) {
    st->scaler_on = reset_scaler == 1 ? 1u : 0u;
    st->loss_scale = reset_scaler == 1 ? init_scale : 1.0f;
    st->found_inf = 0u; st->good_steps = 0u; st->opt_steps = 0u; st->skipped = 0u;
    st->clip_coef = 1.0f; st->grad_norm = 0.0f;
  }
}

__global__ void scaler_update_kernel(eg_step_state* st, float growth, float backoff, int growth_interval) {
  if (st->scaler_on && st->found_inf) {
    st->loss_scale *= backoff;
    st->good_steps = 0u;
    st->skipped += 1u;
    return;
  }
  st->opt_steps += 1u;
  if (!st->scaler_on) return;
  st->good_steps += 1u;
  if ((int)st->good_steps >= growth_interval) {
    st->loss_scale *= growth;
    st->good_steps = 0u;
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long long n,
                                                    float beta1, float beta2, float eps, float wd, float lr_mult,
                                                    const eg_step_state* __restrict__ st) {
  if (st->scaler_on && st->found_inf) return;        // GradScaler.step: non-finite gradients -> no update at all
  float bc1 = st->bias_corr1, bc2 = st->bias_corr2;
  if (st->use_dev_t) {                               // skipped steps do not advance t: the device keeps the count
    const float t = (float)(st->opt_steps + 1u);
    bc1 = 1.0f - powf(beta1, t);
    bc2 = 1.0f - powf(beta2, t);
  }
  const float lr = st->lr * lr_mult, bc2s = sqrtf(bc2);
  const float gs = st->grad_scale * st->clip_coef / (st->scaler_on ? st->loss_scale : 1.0f);
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const int cnt = (int)min(4ll, n - i);
  float pv[4], gv[4], mv[4], vv[4];
  if (cnt == 4) {
    load4(p + i, pv); load4(g + i, gv); load4(m + i, mv); load4(v + i, vv);
  } else {
    for (int e = 0; e < cnt; ++e) { pv[e] = p[i + e]; gv[e] = g[i + e]; mv[e] = m[i + e]; vv[e] = v[i + e]; }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < cnt) {
      const float gg = gv[e] * gs;
      pv[e] *= 1.0f - lr * wd;
      mv[e] = beta1 * mv[e] + (1.0f - beta1) * gg;
      vv[e] = beta2 * vv[e] + (1.0f - beta2) * gg * gg;
      const float denom = sqrtf(vv[e]) / bc2s + eps;
      pv[e] -= (lr / bc1) * (mv[e] / denom);
    }
  }
  if (cnt == 4) {
    store4(p + i, pv); store4(m + i, mv); store4(v + i, vv);
  } else {
    for (int e = 0; e < cnt; ++e) { p[i + e] = pv[e]; m[i + e] = mv[e]; v[i + e] = vv[e]; }
  }
}

// Gradient accumulation over micro-batches: acc = first ? g : acc + g on a range of the flat buffers, one IEEE fp32 addition per
// element (nothing for the compiler to contract), so the sum equals torch.add bit for bit and inf / NaN travel on to eg_clip_coef.
// Streaming, 12 B/element (8 when FIRST: acc is not read, stale contents cannot leak): one f32x4 per lane and trip, two trips in
// flight, grid-stride over a grid the host sizes from the CU count.  NORM adds eg_grad_sqnorm's partials of the new acc to the same
// pass: block b writes sq_partial[b], block 0 clears the entries beyond the grid.
template <bool FIRST, bool NORM>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long long n4,
                                                              float* __restrict__ sq_partial, int nblk) {
  f32x4* __restrict__ a4 = (f32x4*)acc;
  const f32x4* __restrict__ g4 = (const f32x4*)g;
  const long long stride = (long long)gridDim.x * 256;
  float s = 0.f;
#pragma unroll 2
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 v = g4[i];
    if (!FIRST) v = a4[i] + v;
    a4[i] = v;
    if (NORM) s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (NORM) {
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sq_partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    if (blockIdx.x == 0)
      for (int b = (int)gridDim.x + threadIdx.x; b < nblk; b += 256) sq_partial[b] = 0.f;
  }
}

__global__ void fill_kernel(float* __restrict__ p, long long n, float val) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = val;
}

}  // namespace

extern "C" int eg_grad_sqnorm(const float* g, int64_t n, float* partial, int nblk, void* stream) {
  EG_CHECK(g && partial && n > 0 && nblk > 0 && nblk <= 4096, "eg_grad_sqnorm: bad arguments");
  EG_CHECK((uintptr_t)g % 16 == 0, "eg_grad_sqnorm: alignment");
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, g, (long long)n, partial);
  EG_LAUNCH_CHECK("grad_sqnorm");
  return 0;
}

extern "C" int eg_grad_sqnorm_clip(const float* g, int64_t n, float* partial, int nblk, float max_norm, eg_step_state* state,
                                   uint32_t* counter, void* stream) {
  EG_CHECK(g && partial && state && counter && n > 0 && nblk > 0 && nblk <= 4096, "eg_grad_sqnorm_clip: bad arguments");
  EG_CHECK((uintptr_t)g % 16 == 0 && (uintptr_t)counter % 4 == 0, "eg_grad_sqnorm_clip: alignment");
  hipLaunchKernelGGL(sqnorm_clip_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, g, (long long)n, partial, max_norm, state,
                     counter);
  EG_LAUNCH_CHECK("grad_sqnorm_clip");
  return 0;
}

extern "C" int eg_grad_accumulate(float* acc, const float* g, int64_t n, int first, float* sq_partial, int nblk, void* stream) {
  EG_CHECK(acc && g && n > 0 && n % 4 == 0, "eg_grad_accumulate: bad arguments (acc=%p g=%p n=%lld: n must be a positive multiple of 4)",
           (void*)acc, (const void*)g, (long long)n);
  EG_CHECK(((uintptr_t)acc | (uintptr_t)g) % 16 == 0, "eg_grad_accumulate: alignment (acc and g must be 16-B aligned)");
  EG_CHECK(!sq_partial || (nblk >= 1 && nblk <= 1024), "eg_grad_accumulate: bad arguments (nblk=%d outside [1, 1024])", nblk);
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    const bool ok = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess;
    cus = ok && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  // memory-bound: 8 blocks (32 waves) per CU cover the chip, the grid-stride loop takes the rest; the norm partials allow at
  // most one block per entry
  const long long n4 = n / 4;
  long long grid = std::min<long long>((n4 + 255) / 256, 8ll * cus);
  if (sq_partial) grid = std::min<long long>(grid, nblk);
  const dim3 gd((unsigned)grid), bd(256);
  hipStream_t s = (hipStream_t)stream;
  if (sq_partial) {
    if (first) hipLaunchKernelGGL((grad_accumulate_kernel<true, true>), gd, bd, 0, s, acc, g, n4, sq_partial, nblk);
    else hipLaunchKernelGGL((grad_accumulate_kernel<false, true>), gd, bd, 0, s, acc, g, n4, sq_partial, nblk);
  } else {
    if (first) hipLaunchKernelGGL((grad_accumulate_kernel<true, false>), gd, bd, 0, s, acc, g, n4, sq_partial, nblk);
    else hipLaunchKernelGGL((grad_accumulate_kernel<false, false>), gd, bd, 0, s, acc, g, n4, sq_partial, nblk);
  }
  EG_LAUNCH_CHECK("grad_accumulate");
  return 0;
}

extern "C" int eg_clip_coef(const float* partial, int nblk, float max_norm, eg_step_state* state, void* stream) {
  EG_CHECK(partial && state && nblk > 0, "eg_clip_coef: bad arguments");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblk, max_norm, state);
  EG_LAUNCH_CHECK("clip_coef");
  return 0;
}

extern "C" int eg_adamw_group(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                              float weight_decay, float lr_mult, const eg_step_state* state, void* stream) {
  EG_CHECK(p && g && m && v && state && n > 0, "eg_adamw: bad arguments");
  EG_CHECK(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0, "eg_adamw: alignment");
  const long long nt = (n + 3) / 4;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     (long long)n, beta1, beta2, eps, weight_decay, lr_mult, state);
  EG_LAUNCH_CHECK("adamw");
  return 0;
}

extern "C" int eg_adamw(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                        float weight_decay, const eg_step_state* state, void* stream) {
  return eg_adamw_group(p, g, m, v, n, beta1, beta2, eps, weight_decay, 1.0f, state, stream);
}

extern "C" int eg_set_step_state(eg_step_state* state, uint32_t seed_lo, uint32_t seed_hi, float lr, float bias_corr1,
                                 float bias_corr2, float grad_scale, int reset_scaler, float init_scale, int use_dev_t,
                                 void* stream) {
  EG_CHECK(state && (uintptr_t)state % 16 == 0, "eg_set_step_state: state must be a 16-B aligned device pointer");
  EG_CHECK(reset_scaler >= 0 && reset_scaler <= 2, "eg_set_step_state: reset_scaler %d", reset_scaler);
  EG_CHECK(reset_scaler != 1 || init_scale > 0.f, "eg_set_step_state: init_scale must be positive");
  hipLaunchKernelGGL(set_step_state_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, seed_lo, seed_hi, lr, bias_corr1,
                     bias_corr2, grad_scale, reset_scaler, init_scale, use_dev_t);
  EG_LAUNCH_CHECK("set_step_state");
  return 0;
}

extern "C" int eg_scaler_update(eg_step_state* state, float growth, float backoff, int growth_interval, void* stream) {
  EG_CHECK(state && growth >= 1.f && backoff > 0.f && backoff <= 1.f && growth_interval > 0, "eg_scaler_update: bad arguments");
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, growth, backoff, growth_interval);
  EG_LAUNCH_CHECK("scaler_update");
  return 0;
}

extern "C" int eg_fill_f32(float* p, int64_t n, float value, void* stream) {
  EG_CHECK(p && n > 0, "eg_fill_f32: bad arguments");
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, (long long)n,
                     value);
  EG_LAUNCH_CHECK("fill");
  return 0;
}
