// Exact t-SNE of model embeddings (sklearn.manifold.TSNE, method="exact", two components) in stages, each a deterministic function
// of its inputs: squared distances, the perplexity search, the joint probabilities, the KL gradient and the descent update.
// include/eyegaze_hip.h states the contracts; DESIGN.md §8p the stages, the numerics and the measurements.
//
// No atomics and no grid-wide waits.  Every sum that crosses lanes goes through one fixed-order block sum in fp64, every sum that
// crosses workgroups is written as per-workgroup partials and folded in ascending order by the launch that needs it, so two runs
// give the same bytes.  Nothing on the device iterates until converged: the perplexity search is a counted loop of 100 steps.
#include "common.h"

namespace {

constexpr int MAX_N = EG_TSNE_MAX_N;
constexpr int MAX_D = EG_TSNE_MAX_D;
constexpr double TINY = 2.220446049250313e-16;      // 2^-52, sklearn's MACHINE_EPSILON

// fixed order: the lanes of a wave by xor shuffles, then the NW waves in ascending order
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int k = 1; k < NW; ++k) s += red[k];
  return s;
}

// ---------------------------------------------------------------------------------------------
// squared distances: a 32 x 32 tile of dist per workgroup, 2 x 2 outputs per thread, 32 dimensions per round through LDS.
// (x_id - x_jd)^2 in fp64, added in ascending d: dist[i][j] and dist[j][i] are the same sum term by term, the diagonal is 0.
// ---------------------------------------------------------------------------------------------
constexpr int DT = 32;

__global__ __launch_bounds__(256) void sqdist_kernel(const float* __restrict__ X, const int N, const int D, float* __restrict__ dist) {
  __shared__ double A[DT][DT + 1], B[DT][DT + 1];          // widened once per element, not once per pair
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * DT, j0 = blockIdx.x * DT;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int d0 = 0; d0 < D; d0 += DT) {
    __syncthreads();
    for (int e = threadIdx.x; e < DT * DT; e += 256) {
      const int r = e >> 5, c = e & 31;
      const bool in = d0 + c < D;
      A[r][c] = (in && i0 + r < N) ? (double)X[(long long)(i0 + r) * D + d0 + c] : 0.0;
      B[r][c] = (in && j0 + r < N) ? (double)X[(long long)(j0 + r) * D + d0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int c = 0; c < DT; ++c) {                   // a dimension past D holds 0 on both sides and adds an exact 0
      const double a0 = A[ty][c], a1 = A[ty + 16][c], b0 = B[tx][c], b1 = B[tx + 16][c];
      const double d00 = a0 - b0, d01 = a0 - b1, d10 = a1 - b0, d11 = a1 - b1;
      acc[0][0] = fma(d00, d00, acc[0][0]);
      acc[0][1] = fma(d01, d01, acc[0][1]);
      acc[1][0] = fma(d10, d10, acc[1][0]);
      acc[1][1] = fma(d11, d11, acc[1][1]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < N && j < N) dist[(long long)i * N + j] = (float)acc[a][b];
    }
}

// ---------------------------------------------------------------------------------------------
// perplexity search (sklearn/manifold/_utils.pyx, _binary_search_perplexity): one workgroup per row
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void affinities_kernel(const float* __restrict__ dist, const int N, const double target,
                                                         float* __restrict__ cond, double* __restrict__ beta_out,
                                                         int* __restrict__ steps_out) {
  __shared__ double red[4];
  const int i = blockIdx.x, t = threadIdx.x;
  const float* __restrict__ drow = dist + (long long)i * N;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, S = 1e-8;
  int steps = 100;
  for (int l = 0; l < 100; ++l) {
    double s = 0.0, sd = 0.0;
    for (int j = t; j < N; j += 256) {
      if (j == i) continue;
      const double d = (double)drow[j], p = exp(-d * beta);
      s += p;
      sd = fma(d, p, sd);
    }
    s = block_sum<4>(s, red);
    sd = block_sum<4>(sd, red);
    S = s == 0.0 ? 1e-8 : s;
    const double diff = (log(S) + beta * (sd / S)) - target;
    if (fabs(diff) <= 1e-5) { steps = l; break; }              // every lane holds the same sums: the whole workgroup leaves together
    if (l == 99) break;                                         // beta stays the one the sums above belong to
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) * 0.5;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta * 0.5 : (beta + lo) * 0.5;
    }
  }
  float* __restrict__ crow = cond + (long long)i * N;
  for (int j = t; j < N; j += 256) crow[j] = j == i ? 0.f : (float)(exp(-(double)drow[j] * beta) / S);
  if (t == 0) beta_out[i] = beta, steps_out[i] = steps;
}

// ---------------------------------------------------------------------------------------------
// joint probabilities.  workspace doubles: [0, N) the row sums of cond, [N] the total
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void joint_rowsum_kernel(const float* __restrict__ cond, const int N, double* __restrict__ ws) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  const float* __restrict__ crow = cond + (long long)i * N;
  double s = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) s += (double)crow[j];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) ws[i] = s;
}

// sum over all of (c + c^T) = twice the sum over all of c: the rows in ascending order per lane, then the block sum
__global__ __launch_bounds__(256) void joint_total_kernel(const int N, double* __restrict__ ws) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) s += ws[i];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) ws[N] = fmax(2.0 * s, TINY);
}

__global__ __launch_bounds__(256) void joint_kernel(const float* __restrict__ cond, const int N, const double* __restrict__ ws,
                                                    float* __restrict__ P) {
  __shared__ float T[DT][DT + 1];
  const int i0 = blockIdx.y * DT, j0 = blockIdx.x * DT;
  for (int e = threadIdx.x; e < DT * DT; e += 256) {             // T[r][c] = cond[j0 + r][i0 + c]
    const int r = e >> 5, c = e & 31;
    T[r][c] = (j0 + r < N && i0 + c < N) ? cond[(long long)(j0 + r) * N + i0 + c] : 0.f;
  }
  __syncthreads();
  const double total = ws[N];
  for (int e = threadIdx.x; e < DT * DT; e += 256) {
    const int r = e >> 5, c = e & 31, i = i0 + r, j = j0 + c;
    if (i < N && j < N)
      P[(long long)i * N + j] = i == j ? 0.f : (float)fmax(((double)cond[(long long)i * N + j] + (double)T[c][r]) / total, TINY);
  }
}

// ---------------------------------------------------------------------------------------------
// gradient of the KL divergence (sklearn's _kl_divergence, one degree of freedom).  A workgroup of 8 waves owns GR = 16 rows, two
// per wave; the whole Y sits in LDS.  workspace doubles: [0, nblk) per-workgroup sums of w, [nblk, 2 nblk) per-workgroup KL sums.
//   launch 1 (z):     sum over the workgroup's rows and every j != i of w_ij
//   launch 2 (grad):  Z = the partials in ascending order (every workgroup folds them itself, in the same order), then P is
//                     streamed once: grad_i, and with KL the workgroup's share of the divergence
//   launch 3 (kl):    with KL only, one workgroup folds the shares in ascending order into stats[0]
// w = 1 / (1 + |y_i - y_j|^2) in fp64: the fp32 reciprocal as the seed of two Newton steps (relative error below 2^-50).
// ---------------------------------------------------------------------------------------------
constexpr int GT = 512, GW = GT / 64, GR = 2 * GW;

__device__ __forceinline__ double student_w(double dx, double dy) {
  const double t = fma(dx, dx, fma(dy, dy, 1.0));
  double r = (double)__frcp_rn((float)t);            // t >= 1; beyond the fp32 range the seed is 0 and so is w
  r = fma(r, fma(-t, r, 1.0), r);
  r = fma(r, fma(-t, r, 1.0), r);
  return r;
}

__device__ __forceinline__ void stage_y(const float* __restrict__ Y, const int N, float2* ys) {
  for (int j = threadIdx.x; j < N; j += GT) ys[j] = ((const float2*)Y)[j];
  __syncthreads();
}

__global__ __launch_bounds__(GT) void tsne_z_kernel(const float* __restrict__ Y, const int N, double* __restrict__ zpart) {
  extern __shared__ float2 ys[];
  __shared__ double red[GW];
  stage_y(Y, N, ys);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * GR + 2 * wave, i1 = i0 + 1;
  double z = 0.0;
  if (i0 < N) {
    const bool two = i1 < N;
    const float2 a = ys[i0], b = ys[two ? i1 : i0];
    for (int j = lane; j < N; j += 64) {
      const float2 y = ys[j];
      if (j != i0) z += student_w((double)a.x - (double)y.x, (double)a.y - (double)y.y);
      if (two && j != i1) z += student_w((double)b.x - (double)y.x, (double)b.y - (double)y.y);
    }
  }
  z = block_sum<GW>(z, red);
  if (threadIdx.x == 0) zpart[blockIdx.x] = z;
}

template <bool KL>
__global__ __launch_bounds__(GT) void tsne_grad_kernel(const float* __restrict__ Y, const float* __restrict__ P, const double ex,
                                                       const int N, const int nblk, const double* __restrict__ zpart,
                                                       double* __restrict__ klpart, float* __restrict__ grad) {
  extern __shared__ float2 ys[];
  __shared__ double red[GW];
  stage_y(Y, N, ys);
  double Z = 0.0;
  for (int k = threadIdx.x; k < nblk; k += GT) Z += zpart[k];
  Z = block_sum<GW>(Z, red);
  const double invZ = 1.0 / Z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * GR + 2 * wave, i1 = i0 + 1;
  double kl = 0.0;
  if (i0 < N) {
    const bool two = i1 < N;
    const float2 a = ys[i0], b = ys[two ? i1 : i0];
    const float* __restrict__ p0 = P + (long long)i0 * N;
    const float* __restrict__ p1 = P + (long long)(two ? i1 : i0) * N;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < N; j += 64) {
      const float2 y = ys[j];
      const double pa = ex * (double)p0[j], pb = ex * (double)p1[j];
      {
        const double dx = (double)a.x - (double)y.x, dy = (double)a.y - (double)y.y;
        const double w = student_w(dx, dy), q = fmax(w * invZ, TINY), m = (pa - q) * w;
        g[0] = fma(m, dx, g[0]), g[1] = fma(m, dy, g[1]);
        if (KL && j != i0) kl = fma(pa, log(fmax(pa, TINY) / q), kl);
      }
      {
        const double dx = (double)b.x - (double)y.x, dy = (double)b.y - (double)y.y;
        const double w = student_w(dx, dy), q = fmax(w * invZ, TINY), m = (pb - q) * w;
        g[2] = fma(m, dx, g[2]), g[3] = fma(m, dy, g[3]);
        if (KL && two && j != i1) kl = fma(pb, log(fmax(pb, TINY) / q), kl);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) g[c] += __shfl_xor(g[c], o, 64);
    }
    if (lane == 0) {
      grad[2 * (long long)i0] = (float)(4.0 * g[0]), grad[2 * (long long)i0 + 1] = (float)(4.0 * g[1]);
      if (two) grad[2 * (long long)i1] = (float)(4.0 * g[2]), grad[2 * (long long)i1 + 1] = (float)(4.0 * g[3]);
    }
  }
  if (KL) {
    kl = block_sum<GW>(kl, red);
    if (threadIdx.x == 0) klpart[blockIdx.x] = kl;
  }
}

__global__ __launch_bounds__(256) void tsne_kl_kernel(const int nblk, const double* __restrict__ klpart, double* __restrict__ stats) {
  __shared__ double red[4];
  double s = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) s += klpart[k];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) stats[0] = s;
}

// sklearn's _gradient_descent body in float32, one workgroup over the 2 N elements (at most 128 per lane)
__global__ __launch_bounds__(256) void tsne_update_kernel(float* __restrict__ Y, float* __restrict__ update, float* __restrict__ gains,
                                                          const float* __restrict__ grad, const int n, const float momentum,
                                                          const float lr, const float min_gain, double* __restrict__ stats) {
  __shared__ double red[4];
  double q = 0.0;
  for (int e = threadIdx.x; e < n; e += 256) {
    const float u = update[e], g0 = grad[e];
    float ga = gains[e];
    ga = __fmul_rn(u, g0) < 0.f ? __fadd_rn(ga, 0.2f) : __fmul_rn(ga, 0.8f);
    ga = fmaxf(ga, min_gain);
    const float g = __fmul_rn(g0, ga);
    const float un = __fsub_rn(__fmul_rn(momentum, u), __fmul_rn(lr, g));
    gains[e] = ga, update[e] = un, Y[e] = __fadd_rn(Y[e], un);
    q = fma((double)g, (double)g, q);
  }
  if (stats) {
    q = block_sum<4>(q, red);
    if (threadIdx.x == 0) stats[1] = q;
  }
}

inline int grad_blocks(int N) { return (N + GR - 1) / GR; }

}  // namespace

extern "C" int64_t eg_tsne_workspace_bytes(int N) {
  if (N < 2 || N > MAX_N) return -1;
  const int64_t joint = (int64_t)N + 1, grad = 2 * (int64_t)grad_blocks(N);
  return 8 * (joint > grad ? joint : grad);
}

#define TSNE_N_CHECK(who) EG_CHECK(N >= 2 && N <= MAX_N, who ": N=%d outside [2, %d]", N, MAX_N)
#define TSNE_WS_CHECK(who)                                                                                                    \
  EG_CHECK(workspace_bytes >= eg_tsne_workspace_bytes(N), who ": N=%d needs %lld workspace bytes, the workspace holds %lld", N, \
           (long long)eg_tsne_workspace_bytes(N), (long long)workspace_bytes)

extern "C" int eg_tsne_sqdist(const float* X, int N, int D, float* dist, void* stream) {
  EG_CHECK(X && dist, "eg_tsne_sqdist: null pointer");
  TSNE_N_CHECK("eg_tsne_sqdist");
  EG_CHECK(D >= 1 && D <= MAX_D, "eg_tsne_sqdist: D=%d outside [1, %d]", D, MAX_D);
  const int tiles = (N + DT - 1) / DT;
  hipLaunchKernelGGL(sqdist_kernel, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, X, N, D, dist);
  EG_LAUNCH_CHECK("tsne_sqdist");
  return 0;
}

extern "C" int eg_tsne_affinities(const float* dist, int N, double perplexity, float* cond, double* beta, int32_t* steps, void* stream) {
  EG_CHECK(dist && cond && beta && steps, "eg_tsne_affinities: null pointer");
  TSNE_N_CHECK("eg_tsne_affinities");
  EG_CHECK(perplexity > 0.0 && perplexity < (double)N, "eg_tsne_affinities: perplexity=%g outside (0, N=%d)", perplexity, N);
  EG_CHECK(dist != cond, "eg_tsne_affinities: cond may not be written over dist");
  hipLaunchKernelGGL(affinities_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, dist, N, log(perplexity), cond, beta, steps);
  EG_LAUNCH_CHECK("tsne_affinities");
  return 0;
}

extern "C" int eg_tsne_joint(const float* cond, int N, void* workspace, int64_t workspace_bytes, float* P, void* stream) {
  EG_CHECK(cond && workspace && P, "eg_tsne_joint: null pointer");
  TSNE_N_CHECK("eg_tsne_joint");
  TSNE_WS_CHECK("eg_tsne_joint");
  EG_CHECK(cond != P, "eg_tsne_joint: P may not be written over cond");
  hipStream_t s = (hipStream_t)stream;
  double* ws = (double*)workspace;
  const int tiles = (N + DT - 1) / DT;
  hipLaunchKernelGGL(joint_rowsum_kernel, dim3(N), dim3(256), 0, s, cond, N, ws);
  EG_LAUNCH_CHECK("tsne_joint_rowsum");
  hipLaunchKernelGGL(joint_total_kernel, dim3(1), dim3(256), 0, s, N, ws);
  EG_LAUNCH_CHECK("tsne_joint_total");
  hipLaunchKernelGGL(joint_kernel, dim3(tiles, tiles), dim3(256), 0, s, cond, N, (const double*)ws, P);
  EG_LAUNCH_CHECK("tsne_joint");
  return 0;
}

extern "C" int eg_tsne_gradient(const float* Y, const float* P, double exaggeration, int N, void* workspace, int64_t workspace_bytes,
                                float* grad, double* stats, void* stream) {
  EG_CHECK(Y && P && workspace && grad, "eg_tsne_gradient: null pointer");
  EG_CHECK(((uintptr_t)Y & 7) == 0, "eg_tsne_gradient: Y must lie on an 8-byte boundary");
  TSNE_N_CHECK("eg_tsne_gradient");
  TSNE_WS_CHECK("eg_tsne_gradient");
  EG_CHECK(exaggeration > 0.0, "eg_tsne_gradient: exaggeration=%g must be > 0", exaggeration);
  static const hipError_t attr[3] = {
      hipFuncSetAttribute((const void*)tsne_z_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * MAX_N),
      hipFuncSetAttribute((const void*)tsne_grad_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * MAX_N),
      hipFuncSetAttribute((const void*)tsne_grad_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * MAX_N)};
  (void)attr;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = grad_blocks(N), lds = 8 * N;
  double* zpart = (double*)workspace;
  double* klpart = zpart + nblk;
  hipLaunchKernelGGL(tsne_z_kernel, dim3(nblk), dim3(GT), lds, s, Y, N, zpart);
  EG_LAUNCH_CHECK("tsne_z");
  if (stats) {
    hipLaunchKernelGGL(tsne_grad_kernel<true>, dim3(nblk), dim3(GT), lds, s, Y, P, exaggeration, N, nblk, (const double*)zpart, klpart, grad);
    EG_LAUNCH_CHECK("tsne_grad");
    hipLaunchKernelGGL(tsne_kl_kernel, dim3(1), dim3(256), 0, s, nblk, (const double*)klpart, stats);
    EG_LAUNCH_CHECK("tsne_kl");
  } else {
    hipLaunchKernelGGL(tsne_grad_kernel<false>, dim3(nblk), dim3(GT), lds, s, Y, P, exaggeration, N, nblk, (const double*)zpart, klpart, grad);
    EG_LAUNCH_CHECK("tsne_grad");
  }
  return 0;
}

extern "C" int eg_tsne_update(float* Y, float* update, float* gains, const float* grad, int N, float momentum, float learning_rate,
                              float min_gain, double* stats, void* stream) {
  EG_CHECK(Y && update && gains && grad, "eg_tsne_update: null pointer");
  TSNE_N_CHECK("eg_tsne_update");
  EG_CHECK(learning_rate > 0.f && momentum >= 0.f && min_gain > 0.f, "eg_tsne_update: learning_rate=%g, momentum=%g, min_gain=%g",
           learning_rate, momentum, min_gain);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, Y, update, gains, grad, 2 * N, momentum,
                     learning_rate, min_gain, stats);
  EG_LAUNCH_CHECK("tsne_update");
  return 0;
}
