// Noisy linear layers, the dueling combination over atoms and the capturable PER weights of Rainbow (gfx950 only, fp32).
//
// Reference: deep_rl/network/network_utils.py:31-83 (NoisyLinear), network_heads.py:79-86 (RainbowNet.forward),
// deep_rl/agent/DQN_agent.py:121-127 (PER weights).
//
// A noisy layer is y = act(x W^T + b) with W = W_mu + W_sigma * (f(e_out) f(e_in)^T), b = b_mu + b_sigma * f(e_b), f(e) = sign(e) sqrt|e|.
// Neither W nor the outer product is ever written: the kernels use the factorised form
//     y = x W_mu^T + f(e_out) * ((x * f(e_in)) W_sigma^T) + b
// with two accumulators over ONE pass through W_mu and W_sigma, and the transposed form of it for the input gradient.  Every sum has
// a fixed order (K slices per wave, waves in LDS in wave order, slabs in slab order): two calls give the same bits, no atomics.
//
//   forward, rows >= 8 (update):  32x32x2 fp32 MFMA, one wave = 32 rows x 32 outputs x a K slice; split-K slabs + fold launch
//   forward, rows <  8 (actor):   one workgroup per output column, float4 streams, block reduction -- no slabs, one launch
//   weight gradient:              dW_mu = g^T x from VALU accumulators (8 outputs x 4 inputs per thread), dW_sigma = dW_mu * eps_W
//                                 stored from the same registers; the bias gradients ride in the first column of workgroups
//   input gradient:               32x32x2 fp32 MFMA over the outputs (4 column tiles per wave = float4 weight loads), split-N slabs + fold
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

__device__ __forceinline__ float noise_f(float e) { return copysignf(sqrtf(fabsf(e)), e); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 noise_f4(const float* e, int k) {   // (noise vectors are views at any 4-byte offset: scalar loads)
  return make_float4(noise_f(e[k]), noise_f(e[k + 1]), noise_f(e[k + 2]), noise_f(e[k + 3]));
}

constexpr int kWaves = 4;   // waves per workgroup of the MFMA kernels

// ------------------------------------------------------------------------------------------------ forward, MFMA
// grid (ceil(N / 32), KB, ceil(rows / (32 RT))).  Wave `w` of K-block `kb` owns the 32-wide K chunks [c0, c0 + cpw) with
// c0 = (kb * 4 + w) * cpw.  Per chunk a lane (j = lane & 31, h = lane >> 5) loads 16 consecutive k of weight row n0 + j
// (k = 32 c + 16 h ...): the two lane halves together consume one 128-byte line per row.  MFMA (u, e) contracts the k pair
// {32 c + 4 u + e, 32 c + 16 + 4 u + e}: A[i = j][k = h] = x, B[k = h][j] = W -- the same pairing on both operands.
// K % 4 == 0, 16-byte aligned x / W rows.  Slab [kb][rows][N] receives the four waves' sums (wave order).
template <int RT>
__global__ void __launch_bounds__(256)
noisy_fwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ wmu, const float* __restrict__ wsig,
                      const float* __restrict__ e_in, const float* __restrict__ e_out, int rows, int K, int N, int cpw,
                      float* __restrict__ slabs) {
  __shared__ float red[kWaves][RT][32 * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * 32, kb = blockIdx.y, r0 = blockIdx.z * (32 * RT);
  const int n = min(n0 + j, N - 1);
  const int c0 = (kb * kWaves + wave) * cpw;
  const float* wm_row = wmu + (size_t)n * K;
  const float* ws_row = wsig + (size_t)n * K;
  f32x16 am[RT], as[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { am[t][r] = 0.f; as[t][r] = 0.f; }
  for (int c = c0; c < c0 + cpw; ++c) {
    if (c * 32 >= K) break;                  // (wave-uniform)
    const int kbase = c * 32 + 16 * h;
    float4 wm[4], ws[4], fe[4];
    int kc[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kbase + 4 * u;
      ok[u] = k < K;
      kc[u] = ok[u] ? k : 0;
      wm[u] = ok[u] ? ld4(wm_row + kc[u]) : zero4();
      ws[u] = ok[u] ? ld4(ws_row + kc[u]) : zero4();
      fe[u] = noise_f4(e_in, kc[u]);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int row = min(r0 + 32 * t + j, rows - 1);
      const float* x_row = x + (size_t)row * K;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 xv = ok[u] ? ld4(x_row + kc[u]) : zero4();
        const float xa[4] = {xv.x, xv.y, xv.z, xv.w};
        const float fa[4] = {fe[u].x, fe[u].y, fe[u].z, fe[u].w};
        const float ma[4] = {wm[u].x, wm[u].y, wm[u].z, wm[u].w};
        const float sa[4] = {ws[u].x, ws[u].y, ws[u].z, ws[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          am[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e], ma[e], am[t], 0, 0, 0);
          as[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e] * fa[e], sa[e], as[t], 0, 0, 0);
        }
      }
    }
  }
  // D[row][col]: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const float fo = noise_f(e_out[n]);
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      red[wave][t][row * 32 + j] = am[t][r] + fo * as[t][r];
    }
  __syncthreads();
  float* slab = slabs + (size_t)kb * rows * N;
#pragma unroll
  for (int t = 0; t < RT; ++t)
    for (int i = threadIdx.x; i < 32 * 32; i += 256) {
      float s = red[0][t][i];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += red[w][t][i];
      const int row = r0 + 32 * t + (i >> 5), col = n0 + (i & 31);
      if (row < rows && col < N) slab[(size_t)row * N + col] = s;
    }
}

// out[r][c] = epilogue(sum of the slabs in slab order): + (b_mu[c] + b_sigma[c] f(e_b[c])) and act for a forward,
// + add (the input gradient of another head on the same features) and * [xact > 0] for an input gradient that hands the layer
// below a pre-activation gradient.
__global__ void __launch_bounds__(256)
noisy_fold_kernel(const float* __restrict__ slabs, int n_slabs, int64_t stride, int cols, const float* __restrict__ bmu,
                  const float* __restrict__ bsig, const float* __restrict__ e_b, int act, const float* __restrict__ add,
                  const float* __restrict__ xact, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= stride) return;
  float s = slabs[i];
  for (int q = 1; q < n_slabs; ++q) s += slabs[(size_t)q * stride + i];
  if (bmu) {
    const int c = (int)(i % cols);
    s += bmu[c] + bsig[c] * noise_f(e_b[c]);
  }
  if (act == DRA_ACT_RELU) s = fmaxf(s, 0.f);
  if (add) s += add[i];
  if (xact) s = xact[i] > 0.f ? s : 0.f;
  out[i] = s;
}

// ------------------------------------------------------------------------------------------------ forward, small batches / any shape
// One workgroup per output column; RB rows per pass over the column's two weight rows.  VEC: K % 4 == 0 and aligned rows.
template <int RB, bool VEC>
__global__ void __launch_bounds__(256)
noisy_fwd_col_kernel(const float* __restrict__ x, const float* __restrict__ wmu, const float* __restrict__ wsig,
                     const float* __restrict__ bmu, const float* __restrict__ bsig, const float* __restrict__ e_in,
                     const float* __restrict__ e_out, const float* __restrict__ e_b, int rows, int K, int N, int act,
                     float* __restrict__ y) {
  __shared__ float red[kWaves][RB][2];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* wm_row = wmu + (size_t)n * K;
  const float* ws_row = wsig + (size_t)n * K;
  const float fo = noise_f(e_out[n]);
  const float bias = bmu[n] + bsig[n] * noise_f(e_b[n]);
  for (int r0 = 0; r0 < rows; r0 += RB) {
    float am[RB], as[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) am[r] = as[r] = 0.f;
    if constexpr (VEC) {
      for (int k = 4 * threadIdx.x; k < K; k += 4 * 256) {
        const float4 wm = ld4(wm_row + k), ws = ld4(ws_row + k), fe = noise_f4(e_in, k);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          const float4 xv = ld4(x + (size_t)min(r0 + r, rows - 1) * K + k);
          am[r] += xv.x * wm.x; am[r] += xv.y * wm.y; am[r] += xv.z * wm.z; am[r] += xv.w * wm.w;
          as[r] += (xv.x * fe.x) * ws.x; as[r] += (xv.y * fe.y) * ws.y; as[r] += (xv.z * fe.z) * ws.z; as[r] += (xv.w * fe.w) * ws.w;
        }
      }
    } else {
      for (int k = threadIdx.x; k < K; k += 256) {
        const float wm = wm_row[k], ws = ws_row[k], fe = noise_f(e_in[k]);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          const float xv = x[(size_t)min(r0 + r, rows - 1) * K + k];
          am[r] += xv * wm;
          as[r] += (xv * fe) * ws;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const float m = wave_sum(am[r]), s = wave_sum(as[r]);
      if (lane == 0) { red[wave][r][0] = m; red[wave][r][1] = s; }
    }
    __syncthreads();
    if (threadIdx.x < RB && r0 + threadIdx.x < rows) {
      const int r = threadIdx.x;
      float m = red[0][r][0], s = red[0][r][1];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) { m += red[w][r][0]; s += red[w][r][1]; }
      float v = m + fo * s + bias;
      if (act == DRA_ACT_RELU) v = fmaxf(v, 0.f);
      y[(size_t)(r0 + r) * N + n] = v;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ forward, one noise draw per row
// noisy_fwd_col_kernel with row r of x under ITS OWN noise (e_in / e_out / e_b rows `noise_stride` floats apart): the transitions
// of one agent step see the same parameters and differ only in their draws (DQN_agent.py:28-29), so ONE pass over the column's
// two weight rows serves all of them.  Per row the arithmetic is the column kernel's, operation for operation (per-thread k order,
// wave butterfly, waves in LDS in wave order, m + fo * s + bias): row r has the bits of a rows = 1 launch with row r's noise.
template <int RB, bool VEC>
__global__ void __launch_bounds__(256)
noisy_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ wmu, const float* __restrict__ wsig,
                      const float* __restrict__ bmu, const float* __restrict__ bsig, const float* __restrict__ e_in,
                      const float* __restrict__ e_out, const float* __restrict__ e_b, int64_t stride_in, int64_t stride_out,
                      int rows, int K, int N, int act, float* __restrict__ y) {
  __shared__ float red[kWaves][RB][2];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* wm_row = wmu + (size_t)n * K;
  const float* ws_row = wsig + (size_t)n * K;
  float am[RB], as[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) am[r] = as[r] = 0.f;
  if constexpr (VEC) {
    for (int k = 4 * threadIdx.x; k < K; k += 4 * 256) {
      const float4 wm = ld4(wm_row + k), ws = ld4(ws_row + k);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int rr = min(r, rows - 1);
        const float4 xv = ld4(x + (size_t)rr * K + k), fe = noise_f4(e_in + (size_t)rr * stride_in, k);
        am[r] += xv.x * wm.x; am[r] += xv.y * wm.y; am[r] += xv.z * wm.z; am[r] += xv.w * wm.w;
        as[r] += (xv.x * fe.x) * ws.x; as[r] += (xv.y * fe.y) * ws.y; as[r] += (xv.z * fe.z) * ws.z; as[r] += (xv.w * fe.w) * ws.w;
      }
    }
  } else {
    for (int k = threadIdx.x; k < K; k += 256) {
      const float wm = wm_row[k], ws = ws_row[k];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int rr = min(r, rows - 1);
        const float xv = x[(size_t)rr * K + k], fe = noise_f(e_in[(size_t)rr * stride_in + k]);
        am[r] += xv * wm;
        as[r] += (xv * fe) * ws;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const float m = wave_sum(am[r]), s = wave_sum(as[r]);
    if (lane == 0) { red[wave][r][0] = m; red[wave][r][1] = s; }
  }
  __syncthreads();
  if (threadIdx.x < RB && threadIdx.x < rows) {
    const int r = threadIdx.x;
    float m = red[0][r][0], s = red[0][r][1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { m += red[w][r][0]; s += red[w][r][1]; }
    const float fo = noise_f(e_out[(size_t)r * stride_out + n]);
    const float bias = bmu[n] + bsig[n] * noise_f(e_b[(size_t)r * stride_out + n]);
    float v = m + fo * s + bias;
    if (act == DRA_ACT_RELU) v = fmaxf(v, 0.f);
    y[(size_t)r * N + n] = v;
  }
}

// ------------------------------------------------------------------------------------------------ Rainbow's greedy action per row
// One workgroup per row: logits[a][z] = value[z] + (adv[a][z] - mean_a adv[.][z]) (dueling_atoms_fwd_kernel's expression: ascending
// a, mean = sum / A) into LDS, then one thread per action: softmax over the atoms (max, sum of exp, both ascending z) and
// q[a] = sum_z p[a][z] atoms[z] in ascending z; thread 0 takes the FIRST maximum (np.argmax).  A, Z <= 64.
constexpr int kActMax = 64;
__global__ void __launch_bounds__(256)
rainbow_act_rows_kernel(const float* __restrict__ value, const float* __restrict__ adv, const float* __restrict__ atoms, int A, int Z,
                        int64_t* __restrict__ action, float* __restrict__ q_out) {
  __shared__ float logit[kActMax * kActMax];
  __shared__ float sq[kActMax];
  const int b = blockIdx.x;
  const float* ap = adv + (size_t)b * A * Z;
  for (int z = threadIdx.x; z < Z; z += 256) {
    float s = 0.f;
    for (int a = 0; a < A; ++a) s += ap[(size_t)a * Z + z];
    const float mean = s / (float)A, v = value[(size_t)b * Z + z];
    for (int a = 0; a < A; ++a) logit[a * Z + z] = v + (ap[(size_t)a * Z + z] - mean);
  }
  __syncthreads();
  if (threadIdx.x < A) {
    const float* l = logit + threadIdx.x * Z;
    float m = l[0];
    for (int z = 1; z < Z; ++z) m = fmaxf(m, l[z]);
    float se = 0.f;
    for (int z = 0; z < Z; ++z) se += expf(l[z] - m);
    float q = 0.f;
    for (int z = 0; z < Z; ++z) q += (expf(l[z] - m) / se) * atoms[z];
    sq[threadIdx.x] = q;
    if (q_out) q_out[(size_t)b * A + threadIdx.x] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    float bq = sq[0];
    for (int a = 1; a < A; ++a)
      if (sq[a] > bq) { bq = sq[a]; best = a; }
    action[b] = (int64_t)best;
  }
}

// ------------------------------------------------------------------------------------------------ weight / bias gradients
// grid (ceil(K / (V blockDim)), ceil(N / 8)).  A thread owns V consecutive inputs k of 8 outputs n: acc[i][e] = sum_b g[b][n0 + i]
// x[b][k + e] in ascending b; the rows of g are staged through LDS 32 at a time.  dW_mu and dW_sigma = dW_mu * (f(e_out) f(e_in))
// are stored from the same accumulators.  Workgroups of the first column also form db_mu = sum_b g and db_sigma = db_mu f(e_b).
constexpr int kWN = 8;
template <int V>
__global__ void __launch_bounds__(256)
noisy_bwd_w_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ e_in,
                   const float* __restrict__ e_out, const float* __restrict__ e_b, int rows, int K, int N,
                   float* __restrict__ dwmu, float* __restrict__ dwsig, float* __restrict__ dbmu, float* __restrict__ dbsig) {
  __shared__ float gs[32][kWN];
  const int n0 = blockIdx.y * kWN;
  const int k = (blockIdx.x * blockDim.x + threadIdx.x) * V;
  const bool kok = k < K;
  float acc[kWN][V];
#pragma unroll
  for (int i = 0; i < kWN; ++i)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[i][e] = 0.f;
  for (int b0 = 0; b0 < rows; b0 += 32) {
    __syncthreads();
    for (int q = threadIdx.x; q < 32 * kWN; q += blockDim.x) {
      const int bb = q / kWN, i = q % kWN;
      gs[bb][i] = (b0 + bb < rows && n0 + i < N) ? g[(size_t)(b0 + bb) * N + n0 + i] : 0.f;
    }
    __syncthreads();
    const int nb = min(32, rows - b0);
    if (kok) {
      for (int bb = 0; bb < nb; ++bb) {
        float xv[V];
        if constexpr (V == 4) {
          const float4 t = ld4(x + (size_t)(b0 + bb) * K + k);
          xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
        } else {
          xv[0] = x[(size_t)(b0 + bb) * K + k];
        }
#pragma unroll
        for (int i = 0; i < kWN; ++i) {
          const float gv = gs[bb][i];
#pragma unroll
          for (int e = 0; e < V; ++e) acc[i][e] += gv * xv[e];
        }
      }
    }
  }
  if (kok) {
    float fi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) fi[e] = noise_f(e_in[k + e]);
#pragma unroll
    for (int i = 0; i < kWN; ++i) {
      const int n = n0 + i;
      if (n >= N) break;
      const float fo = noise_f(e_out[n]);
      float sg[V];
#pragma unroll
      for (int e = 0; e < V; ++e) sg[e] = acc[i][e] * (fo * fi[e]);
      if constexpr (V == 4) {
        *reinterpret_cast<float4*>(dwmu + (size_t)n * K + k) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        *reinterpret_cast<float4*>(dwsig + (size_t)n * K + k) = make_float4(sg[0], sg[1], sg[2], sg[3]);
      } else {
        dwmu[(size_t)n * K + k] = acc[i][0];
        dwsig[(size_t)n * K + k] = sg[0];
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < kWN && n0 + threadIdx.x < N && dbmu) {
    const int n = n0 + threadIdx.x;
    float s = 0.f;
    for (int b = 0; b < rows; ++b) s += g[(size_t)b * N + n];
    dbmu[n] = s;
    dbsig[n] = s * noise_f(e_b[n]);
  }
}

// ------------------------------------------------------------------------------------------------ input gradient, MFMA
// dx[b][k] = sum_n g[b][n] W_mu[n][k] + f(e_in[k]) sum_n (g[b][n] f(e_out[n])) W_sigma[n][k].
// grid (ceil(K / 128), NB, ceil(rows / 32)).  A lane (j, h) loads the float4 W[n + h][k0 + 4 j ..]: component e belongs to column tile
// e (columns k0 + 4 j + e), so a wave keeps 4 tiles x 2 accumulators and every weight load is a full 512-byte run per lane half.
// MFMA: A[i = j][k = h] = g[r0 + j][n + h], B[k = h][j] = W[n + h][k0 + 4 j + e].  Wave w of N-block nb owns the outputs
// [(nb * 4 + w) * npw, + npw), npw even.  The four waves add up in LDS in wave order; slab [nb][rows][K].  K % 4 == 0.
__global__ void __launch_bounds__(256)
noisy_bwd_x_mfma_kernel(const float* __restrict__ g, const float* __restrict__ wmu, const float* __restrict__ wsig,
                        const float* __restrict__ e_in, const float* __restrict__ e_out, int rows, int K, int N, int npw,
                        float* __restrict__ slabs) {
  __shared__ float4 red[32 * 32];            // [row][4 j .. 4 j + 3]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int k0 = blockIdx.x * 128, nb = blockIdx.y, r0 = blockIdx.z * 32;
  const int kcol = k0 + 4 * j;
  const bool kok = kcol < K;
  const int kc = kok ? kcol : 0;
  const int row = min(r0 + j, rows - 1);
  const int n_begin = (nb * kWaves + wave) * npw, n_end = min(N, n_begin + npw);
  f32x16 am[4], as[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) { am[e][r] = 0.f; as[e][r] = 0.f; }
  for (int n = n_begin; n < n_end; n += 2) {
    const int nn = n + h;
    const bool ok = nn < N;
    const int nc = ok ? nn : 0;
    const float gv = ok ? g[(size_t)row * N + nc] : 0.f;
    const float gsv = gv * noise_f(e_out[nc]);
    const float4 wm = ok ? ld4(wmu + (size_t)nc * K + kc) : zero4();
    const float4 ws = ok ? ld4(wsig + (size_t)nc * K + kc) : zero4();
    am[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, wm.x, am[0], 0, 0, 0);
    as[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gsv, ws.x, as[0], 0, 0, 0);
    am[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, wm.y, am[1], 0, 0, 0);
    as[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gsv, ws.y, as[1], 0, 0, 0);
    am[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, wm.z, am[2], 0, 0, 0);
    as[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(gsv, ws.z, as[2], 0, 0, 0);
    am[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, wm.w, am[3], 0, 0, 0);
    as[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(gsv, ws.w, as[3], 0, 0, 0);
  }
  const float4 fi = noise_f4(e_in, kc);
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int orow = (r & 3) + 8 * (r >> 2) + 4 * h;
        float4 p = make_float4(am[0][r] + fi.x * as[0][r], am[1][r] + fi.y * as[1][r], am[2][r] + fi.z * as[2][r],
                               am[3][r] + fi.w * as[3][r]);
        if (w > 0) {
          const float4 q = red[orow * 32 + j];
          p = make_float4(q.x + p.x, q.y + p.y, q.z + p.z, q.w + p.w);
        }
        red[orow * 32 + j] = p;
      }
    }
    __syncthreads();
  }
  float* slab = slabs + (size_t)nb * rows * K;
  for (int i = threadIdx.x; i < 32 * 32; i += 256) {
    const int orow = r0 + (i >> 5), col = k0 + 4 * (i & 31);
    if (orow < rows && col < K) *reinterpret_cast<float4*>(slab + (size_t)orow * K + col) = red[i];
  }
}

// any shape: one thread per (row, input), ascending n
__global__ void __launch_bounds__(256)
noisy_bwd_x_any_kernel(const float* __restrict__ g, const float* __restrict__ wmu, const float* __restrict__ wsig,
                       const float* __restrict__ e_in, const float* __restrict__ e_out, const float* __restrict__ add,
                       const float* __restrict__ xact, int rows, int K, int N, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * K) return;
  const int b = (int)(i / K), k = (int)(i % K);
  float m = 0.f, s = 0.f;
  for (int n = 0; n < N; ++n) {
    const float gv = g[(size_t)b * N + n];
    m += gv * wmu[(size_t)n * K + k];
    s += (gv * noise_f(e_out[n])) * wsig[(size_t)n * K + k];
  }
  float v = m + noise_f(e_in[k]) * s;
  if (add) v += add[i];
  if (xact) v = xact[i] > 0.f ? v : 0.f;
  dx[i] = v;
}

// ------------------------------------------------------------------------------------------------ dueling over atoms
// logits[b][a][z] = value[b][z] + (adv[b][a][z] - mean_a adv[b][.][z]); one thread per (b, z), ascending a.
__global__ void __launch_bounds__(256)
dueling_atoms_fwd_kernel(const float* __restrict__ value, const float* __restrict__ adv, int B, int A, int Z,
                         float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * Z) return;
  const int b = i / Z, z = i % Z;
  const float* ap = adv + (size_t)b * A * Z + z;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += ap[(size_t)a * Z];
  const float mean = s / (float)A, v = value[i];
  float* op = out + (size_t)b * A * Z + z;
  for (int a = 0; a < A; ++a) op[(size_t)a * Z] = v + (ap[(size_t)a * Z] - mean);
}
// dvalue[b][z] = sum_a g[b][a][z]; dadv[b][a][z] = g[b][a][z] - dvalue[b][z] / A
__global__ void __launch_bounds__(256)
dueling_atoms_bwd_kernel(const float* __restrict__ g, int B, int A, int Z, float* __restrict__ dvalue, float* __restrict__ dadv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * Z) return;
  const int b = i / Z, z = i % Z;
  const float* gp = g + (size_t)b * A * Z + z;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += gp[(size_t)a * Z];
  dvalue[i] = s;
  const float m = s / (float)A;
  float* dp = dadv + (size_t)b * A * Z + z;
  for (int a = 0; a < A; ++a) dp[(size_t)a * Z] = gp[(size_t)a * Z] - m;
}

// ------------------------------------------------------------------------------------------------ PER weights, beta on the device
// losses.hip per_kernel with the importance exponent read from *beta_dev (same expressions, same bits)
__global__ void __launch_bounds__(1024)
per_dev_kernel(const float* __restrict__ loss_vec, const float* __restrict__ samp_prob, int B, const float* __restrict__ beta_dev,
               float eps, float alpha, float* __restrict__ out_prio, float* __restrict__ out_w) {
  __shared__ float s_red[16];
  const int b = threadIdx.x;
  const bool on = b < B;
  if (on && loss_vec && out_prio) {
    const float ad = fabsf(loss_vec[b]) + eps;
    out_prio[b] = (alpha == 0.5f) ? sqrtf(ad) : powf(ad, alpha);
  }
  if (samp_prob && out_w) {
    const float beta = *beta_dev;
    const float wraw = on ? powf(samp_prob[b] * (float)B + 1e-6f, -beta) : -INFINITY;
    const float wv = wave_max(wraw);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = wv;
    __syncthreads();
    float wmax = s_red[0];
    for (int w = 1; w < (int)((blockDim.x + 63) >> 6); ++w) wmax = fmaxf(wmax, s_red[w]);
    if (on) out_w[b] = wraw / wmax;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

}  // namespace

// split plans (shared by the launches and by dra_noisy_workspace_floats)
struct FwdPlan { int rt, col_tiles, row_groups, cpw, kb; };
static FwdPlan fwd_plan(int rows, int K, int N) {
  FwdPlan p;
  p.rt = rows > 32 ? 2 : 1;
  p.col_tiles = ceil_div(N, 32);
  p.row_groups = ceil_div(rows, 32 * p.rt);
  const int chunks = ceil_div(K, 32);
  const int kb_target = max(1, 512 / (p.col_tiles * p.row_groups));
  p.cpw = max(2, ceil_div(chunks, kWaves * kb_target));
  p.kb = ceil_div(ceil_div(chunks, p.cpw), kWaves);
  return p;
}
struct BwdPlan { int col_blocks, row_groups, npw, nb; };
static BwdPlan bwd_plan(int rows, int K, int N) {
  BwdPlan p;
  p.col_blocks = ceil_div(K, 128);
  p.row_groups = ceil_div(rows, 32);
  const int nb_target = max(1, 256 / (p.col_blocks * p.row_groups));
  int npw = ceil_div(N, kWaves * nb_target);
  p.npw = max(2, npw + (npw & 1));
  p.nb = ceil_div(N, kWaves * p.npw);
  return p;
}

// floats of workspace dra_noisy_linear_fwd / _bwd use for this shape (split-K / split-N slabs)
DRA_API int dra_noisy_workspace_floats(int rows, int in_features, int out_features, int64_t* fwd, int64_t* bwd) {
  if (rows < 1 || rows > 1024 || in_features < 1 || out_features < 1 || !fwd || !bwd) return DRA_EINVAL;
  *fwd = (int64_t)fwd_plan(rows, in_features, out_features).kb * rows * out_features;
  *bwd = (int64_t)bwd_plan(rows, in_features, out_features).nb * rows * in_features;
  return DRA_OK;
}

DRA_API int dra_noisy_linear_fwd(const float* x, const float* w_mu, const float* w_sigma, const float* b_mu, const float* b_sigma,
                                 const float* noise_in, const float* noise_out_weight, const float* noise_out_bias, float* y,
                                 int rows, int in_features, int out_features, int act, float* workspace, int64_t workspace_floats,
                                 void* stream) {
  if (!x || !w_mu || !w_sigma || !b_mu || !b_sigma || !noise_in || !noise_out_weight || !noise_out_bias || !y) return DRA_EINVAL;
  if (rows < 1 || rows > 1024 || in_features < 1 || out_features < 1 || (act != DRA_ACT_NONE && act != DRA_ACT_RELU)) return DRA_EINVAL;
  const int K = in_features, N = out_features;
  hipStream_t st = dra_stream(stream);
  const bool vec = K % 4 == 0 && aligned16(x) && aligned16(w_mu) && aligned16(w_sigma);
  if (rows >= 8 && vec) {
    const FwdPlan p = fwd_plan(rows, K, N);
    const int cpw = p.cpw, kb = p.kb;
    if (!workspace || workspace_floats < (int64_t)kb * rows * N) return DRA_EINVAL;
    dim3 grid(p.col_tiles, kb, p.row_groups);
    if (p.rt == 2)
      hipLaunchKernelGGL(noisy_fwd_mfma_kernel<2>, grid, dim3(256), 0, st, x, w_mu, w_sigma, noise_in, noise_out_weight, rows, K, N,
                         cpw, workspace);
    else
      hipLaunchKernelGGL(noisy_fwd_mfma_kernel<1>, grid, dim3(256), 0, st, x, w_mu, w_sigma, noise_in, noise_out_weight, rows, K, N,
                         cpw, workspace);
    DRA_LAUNCH_CHECK();
    const int64_t total = (int64_t)rows * N;
    hipLaunchKernelGGL(noisy_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, workspace, kb, total, N, b_mu,
                       b_sigma, noise_out_bias, act, (const float*)nullptr, (const float*)nullptr, y);
    DRA_LAUNCH_CHECK();
    return DRA_OK;
  }
#define DRA_NOISY_COL(RB, VEC)                                                                                                  \
  hipLaunchKernelGGL((noisy_fwd_col_kernel<RB, VEC>), dim3(N), dim3(256), 0, st, x, w_mu, w_sigma, b_mu, b_sigma, noise_in,     \
                     noise_out_weight, noise_out_bias, rows, K, N, act, y)
  if (rows == 1) { if (vec) DRA_NOISY_COL(1, true); else DRA_NOISY_COL(1, false); }
  else           { if (vec) DRA_NOISY_COL(4, true); else DRA_NOISY_COL(4, false); }
#undef DRA_NOISY_COL
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

DRA_API int dra_noisy_linear_fwd_rows(const float* x, const float* w_mu, const float* w_sigma, const float* b_mu, const float* b_sigma,
                                      const float* noise_in, const float* noise_out_weight, const float* noise_out_bias,
                                      int64_t noise_stride, float* y, int rows, int in_features, int out_features, int act,
                                      void* stream) {
  if (!x || !w_mu || !w_sigma || !b_mu || !b_sigma || !noise_in || !noise_out_weight || !noise_out_bias || !y) return DRA_EINVAL;
  if (rows < 1 || rows > 8 || in_features < 1 || out_features < 1 || (act != DRA_ACT_NONE && act != DRA_ACT_RELU)) return DRA_EINVAL;
  if (noise_stride < 0 || (noise_stride > 0 && (noise_stride < in_features || noise_stride < out_features))) return DRA_EINVAL;
  const int K = in_features, N = out_features;
  const int64_t s_in = noise_stride ? noise_stride : K, s_out = noise_stride ? noise_stride : N;
  hipStream_t st = dra_stream(stream);
  const bool vec = K % 4 == 0 && aligned16(x) && aligned16(w_mu) && aligned16(w_sigma);
#define DRA_NOISY_ROWS(RB, VEC)                                                                                                 \
  hipLaunchKernelGGL((noisy_fwd_rows_kernel<RB, VEC>), dim3(N), dim3(256), 0, st, x, w_mu, w_sigma, b_mu, b_sigma, noise_in,    \
                     noise_out_weight, noise_out_bias, s_in, s_out, rows, K, N, act, y)
  if (rows == 1)      { if (vec) DRA_NOISY_ROWS(1, true); else DRA_NOISY_ROWS(1, false); }
  else if (rows <= 4) { if (vec) DRA_NOISY_ROWS(4, true); else DRA_NOISY_ROWS(4, false); }
  else                { if (vec) DRA_NOISY_ROWS(8, true); else DRA_NOISY_ROWS(8, false); }
#undef DRA_NOISY_ROWS
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

DRA_API int dra_rainbow_act_rows(const float* value, const float* advantage, const float* atoms, int rows, int n_actions, int n_atoms,
                                 int64_t* action, float* q, void* stream) {
  if (!value || !advantage || !atoms || !action) return DRA_EINVAL;
  if (rows < 1 || rows > 8 || n_actions < 1 || n_actions > kActMax || n_atoms < 1 || n_atoms > kActMax) return DRA_EINVAL;
  hipLaunchKernelGGL(rainbow_act_rows_kernel, dim3(rows), dim3(256), 0, dra_stream(stream), value, advantage, atoms, n_actions,
                     n_atoms, action, q);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

DRA_API int dra_noisy_linear_bwd(const float* g, const float* x, const float* w_mu, const float* w_sigma, const float* noise_in,
                                 const float* noise_out_weight, const float* noise_out_bias, const float* x_relu, const float* dx_add,
                                 float* dw_mu, float* dw_sigma, float* db_mu, float* db_sigma, float* dx, int rows, int in_features,
                                 int out_features, float* workspace, int64_t workspace_floats, void* stream) {
  if (!g || !x || !w_mu || !w_sigma || !noise_in || !noise_out_weight || !noise_out_bias) return DRA_EINVAL;
  if (rows < 1 || rows > 1024 || in_features < 1 || out_features < 1) return DRA_EINVAL;
  if ((dw_mu == nullptr) != (dw_sigma == nullptr) || (db_mu == nullptr) != (db_sigma == nullptr)) return DRA_EINVAL;
  if (db_mu && !dw_mu) return DRA_EINVAL;
  const int K = in_features, N = out_features;
  hipStream_t st = dra_stream(stream);
  // (every check before the first launch: a refused call writes nothing)
  const bool dx_vec = dx && K % 4 == 0 && aligned16(w_mu) && aligned16(w_sigma) && aligned16(dx) && aligned16(workspace) && workspace;
  const BwdPlan p = bwd_plan(rows, K, N);
  const int64_t total = (int64_t)rows * K;
  if (dx_vec && workspace_floats < (int64_t)p.nb * total) return DRA_EINVAL;
  if (dw_mu) {
    const bool vec = K % 4 == 0 && aligned16(x) && aligned16(dw_mu) && aligned16(dw_sigma);
    const int units = vec ? K / 4 : K;       // threads along K
    int threads = 256, best = -1;
    for (int t = 256; t >= 64; t /= 2) {
      const int waste = ceil_div(units, t) * t - units;
      if (best < 0 || waste < best) { best = waste; threads = t; }
    }
    dim3 grid(ceil_div(units, threads), ceil_div(N, kWN));
    if (vec)
      hipLaunchKernelGGL(noisy_bwd_w_kernel<4>, grid, dim3(threads), 0, st, g, x, noise_in, noise_out_weight, noise_out_bias, rows, K,
                         N, dw_mu, dw_sigma, db_mu, db_sigma);
    else
      hipLaunchKernelGGL(noisy_bwd_w_kernel<1>, grid, dim3(threads), 0, st, g, x, noise_in, noise_out_weight, noise_out_bias, rows, K,
                         N, dw_mu, dw_sigma, db_mu, db_sigma);
    DRA_LAUNCH_CHECK();
  }
  if (dx) {
    if (dx_vec) {
      const int npw = p.npw, nb = p.nb;
      hipLaunchKernelGGL(noisy_bwd_x_mfma_kernel, dim3(p.col_blocks, nb, p.row_groups), dim3(256), 0, st, g, w_mu, w_sigma, noise_in,
                         noise_out_weight, rows, K, N, npw, workspace);
      DRA_LAUNCH_CHECK();
      hipLaunchKernelGGL(noisy_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, workspace, nb, total, K,
                         (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, DRA_ACT_NONE, dx_add, x_relu, dx);
      DRA_LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL(noisy_bwd_x_any_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, w_mu, w_sigma, noise_in,
                         noise_out_weight, dx_add, x_relu, rows, K, N, dx);
      DRA_LAUNCH_CHECK();
    }
  }
  return DRA_OK;
}

DRA_API int dra_dueling_atoms_fwd(const float* value, const float* advantage, int batch, int n_actions, int n_atoms, float* logits,
                                  void* stream) {
  if (!value || !advantage || !logits || batch < 1 || n_actions < 1 || n_atoms < 1) return DRA_EINVAL;
  hipLaunchKernelGGL(dueling_atoms_fwd_kernel, dim3(ceil_div(batch * n_atoms, 256)), dim3(256), 0, dra_stream(stream), value,
                     advantage, batch, n_actions, n_atoms, logits);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

DRA_API int dra_dueling_atoms_bwd(const float* g_logits, int batch, int n_actions, int n_atoms, float* d_value, float* d_advantage,
                                  void* stream) {
  if (!g_logits || !d_value || !d_advantage || batch < 1 || n_actions < 1 || n_atoms < 1) return DRA_EINVAL;
  hipLaunchKernelGGL(dueling_atoms_bwd_kernel, dim3(ceil_div(batch * n_atoms, 256)), dim3(256), 0, dra_stream(stream), g_logits,
                     batch, n_actions, n_atoms, d_value, d_advantage);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

DRA_API int dra_per_weights_dev(const float* loss_vec, const float* sampling_prob, int batch, const float* beta_dev, float replay_eps,
                                float replay_alpha, float* out_prio, float* out_weights, void* stream) {
  if (batch < 1 || batch > 1024 || (sampling_prob && out_weights && !beta_dev)) return DRA_EINVAL;
  const int threads = ((batch + 63) / 64) * 64;
  hipLaunchKernelGGL(per_dev_kernel, dim3(1), dim3(threads), 0, dra_stream(stream), loss_vec, sampling_prob, batch, beta_dev,
                     replay_eps, replay_alpha, out_prio, out_weights);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
