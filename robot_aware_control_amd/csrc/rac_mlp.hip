// The learned robot model's two 4-layer MLPs (reference src/prediction/models/dynamics.py:269-338): in -> 512 -> 512 ->
// 512 -> D with ReLU after the first three layers, in = D + A.  Forward, the T-step residual rollout of both models in
// one launch, and the parameter gradients.  Exact fp32 throughout: the two 512x512 layers on v_mfma_f32_16x16x4_f32 (a
// k-ordered fmaf chain per output element), the thin first (K <= 12) and last (N <= 7) layers on plain fmaf.
//
// A workgroup (8 waves) owns a tile of TM = 16 rows; a layer's activations of the tile live in one LDS buffer
// ([16][512] floats, rows padded to 516), wave w owns output columns [64 w, 64 w + 64) and keeps them in four 16x16
// accumulators across the K loop.  Weights stream from global memory (every tile reads the same 3 MB per model: L2).
// A row's result depends on nothing but the row: the K order of every output element is fixed, K is never split and no
// float atomic is used anywhere, so a row gives the same bits in any tile position, batch and entry point.
#include "rac_common.h"

namespace rac {
namespace {

constexpr int HID = 512;    // hidden width (dynamics.py:279,315)
constexpr int TM = 16;      // rows per workgroup
constexpr int LDH = 516;    // LDS row stride of the activation tile: 16-byte rows, float4 reads of 16 rows hit 64 banks
constexpr int NTHR = 512;   // 8 waves, 64 output columns each
constexpr int MAXD = 7, MAXA = 5, MAXIN = MAXD + MAXA;
constexpr int LDX = MAXIN;  // LDS row stride of the (x | a) input tile

struct MlpParams {
  const float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;
};

// state_dict order, torch's [out][in] Linear layout (include/rac_hip.h, rac_mlp4_fwd)
__host__ __device__ inline MlpParams carve(const float* p, int D, int A) {
  MlpParams P;
  const int IN = D + A;
  P.W1 = p;
  P.b1 = P.W1 + (long)HID * IN;
  P.W2 = P.b1 + HID;
  P.b2 = P.W2 + (long)HID * HID;
  P.W3 = P.b2 + HID;
  P.b3 = P.W3 + (long)HID * HID;
  P.W4 = P.b3 + HID;
  P.b4 = P.W4 + (long)D * HID;
  return P;
}
inline long param_count(int D, int A) { return (long)HID * (D + A) + HID + 2L * (HID * HID + HID) + (long)D * HID + D; }

// acc[nt] (rows 4 g + reg, column n0 + 16 nt + c of the tile's product) += buf[16][512] . B, K = 512 in 32 chunks of 16.
// TRANS = false: B[k][n] = W[n][k] (forward, y = h W^T); TRANS = true: B[k][n] = W[k][n] (dgrad, dh = dz W).
// Lane (c = l & 15, g = l >> 4) holds k = 16 j + 4 g + t of chunk j in element t of its fragments: MFMA t of the chunk
// sums k = 16 j + t, + 4, + 8, + 12 in that order -- a permutation of K, the same for every output element.
// (Keeping the B fragments of 4 chunks ahead in flight in a register ring, and the last layer's 128 weights per lane in
// flight at once, were both measured: no change of the rollout's 78 us per step, so the plain loops stayed.)
template <bool TRANS>
__device__ __forceinline__ void gemm512(const float* __restrict__ W, const float* buf, f32x4 acc[4], int n0, int c, int g) {
#pragma unroll 2
  for (int j = 0; j < HID / 16; ++j) {
    const int k = 16 * j + 4 * g;
    const f32x4 a = *reinterpret_cast<const f32x4*>(buf + c * LDH + k);
    f32x4 b[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = n0 + 16 * nt + c;
      if (!TRANS) {
        b[nt] = *reinterpret_cast<const f32x4*>(W + (long)n * HID + k);
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) b[nt][t] = W[(long)(k + t) * HID + n];
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[nt][t], acc[nt], 0, 0, 0);
  }
}

// One hidden 512 -> 512 layer with bias and ReLU, in place in `buf`; `save` (or null) receives the tile's valid rows.
__device__ __forceinline__ void hidden_layer(const float* __restrict__ W, const float* __restrict__ bias, float* buf,
                                             float* save, int valid) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, n0 = (threadIdx.x >> 6) * 64;
  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const float bv = bias[n0 + 16 * nt + c];
    acc[nt] = f32x4{bv, bv, bv, bv};
  }
  gemm512<false>(W, buf, acc, n0, c, g);
  __syncthreads();  // every wave has read the layer's input
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r, col = n0 + 16 * nt + c;
      const float h = fmaxf(acc[nt][r], 0.f);
      buf[row * LDH + col] = h;
      if (save && row < valid) save[(long)row * HID + col] = h;
    }
  __syncthreads();
}

// delta = MLP([x | a]) of the tile whose (x | a) rows stand in `xin` (rows >= valid zero).  The result of row o / D,
// output o % D (o = threadIdx.x >> 2 < TM * D) is returned on the lane with (threadIdx.x & 3) == 0.
// acts: null, or the tile's first row of the [3][M][512] post-ReLU activations (plane stride `plane`).
__device__ __forceinline__ float mlp_tile(const MlpParams& P, int D, int A, const float* xin, float* buf, float* acts,
                                          long plane, int valid) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, IN = D + A;
  {  // layer 1: thread = output column, K = IN <= 12
    float w[MAXIN];
#pragma unroll
    for (int k = 0; k < MAXIN; ++k) w[k] = k < IN ? P.W1[(long)tid * IN + k] : 0.f;
    const float bv = P.b1[tid];
    for (int r = 0; r < TM; ++r) {
      float s = bv;
#pragma unroll
      for (int k = 0; k < MAXIN; ++k)
        if (k < IN) s = fmaf(xin[r * LDX + k], w[k], s);
      const float h = fmaxf(s, 0.f);
      buf[r * LDH + tid] = h;
      if (acts && r < valid) acts[(long)r * HID + tid] = h;
    }
  }
  __syncthreads();
  hidden_layer(P.W2, P.b2, buf, acts ? acts + plane : nullptr, valid);
  hidden_layer(P.W3, P.b3, buf, acts ? acts + 2 * plane : nullptr, valid);
  // layer 4: 4 lanes per output, 128 consecutive k each, summed (p0 + p1) + (p2 + p3)
  const int o = tid >> 2, part = tid & 3;
  float p = 0.f;
  if (o < TM * D) {
    const int r = o / D, d = o - r * D;
    const float* h = buf + r * LDH + 128 * part;
    const float* w = P.W4 + (long)d * HID + 128 * part;
    for (int i = 0; i < 128; i += 4) {
      const f32x4 hv = *reinterpret_cast<const f32x4*>(h + i);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + i);
#pragma unroll
      for (int t = 0; t < 4; ++t) p = fmaf(hv[t], wv[t], p);
    }
  }
  p = p + __shfl_xor(p, 1);
  p = p + __shfl_xor(p, 2);
  if (o < TM * D) p = p + P.b4[o % D];
  return p;
}

// (x | a) rows of the tile into LDS; rows past the end and columns past D + A are zero.
__device__ __forceinline__ void load_inputs(float* xin, const float* x, const float* a, long row0, int valid, int D, int A) {
  const int tid = threadIdx.x;
  if (tid < TM * LDX) {
    const int r = tid / LDX, k = tid - r * LDX;
    float v = 0.f;
    if (r < valid) {
      if (k < D) v = x[(row0 + r) * D + k];
      else if (k < D + A && a) v = a[(row0 + r) * A + (k - D)];
    }
    xin[tid] = v;
  }
}

__global__ void __launch_bounds__(NTHR) mlp4_fwd_kernel(const float* params, const float* x, const float* a, float* y,
                                                        float* acts, long M, int D, int A, int residual) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float buf[TM * LDH];
  __shared__ float xin[TM * LDX];
  const long row0 = (long)blockIdx.x * TM;
  const int valid = (int)min((long)TM, M - row0);
  const MlpParams P = carve(params, D, A);
  load_inputs(xin, x, a, row0, valid, D, A);
  __syncthreads();
  const float delta = mlp_tile(P, D, A, xin, buf, acts ? acts + row0 * HID : nullptr, M * HID, valid);
  const int o = threadIdx.x >> 2;
  if ((threadIdx.x & 3) == 0 && o < TM * D) {
    const int r = o / D, d = o - r * D;
    if (r < valid) y[(row0 + r) * D + d] = residual ? xin[r * LDX + d] + delta : delta;
  }
}

// blockIdx.y = model (0: joints, 1: gripper state); state[t + 1] = state[t] + MLP(state[t] | actions[t]), t < T.
__global__ void __launch_bounds__(NTHR) robot_rollout_kernel(const float* jp, const float* gp, const float* q0,
                                                             const float* s0, const float* actions, float* q_out,
                                                             float* s_out, int T, long N, int J, int R, int A) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float buf[TM * LDH];
  __shared__ float xin[TM * LDX];
  const bool grip = blockIdx.y == 1;
  const float* params = grip ? gp : jp;
  if (!params) return;
  const int D = grip ? R : J;
  const float* start = grip ? s0 : q0;
  float* out = grip ? s_out : q_out;
  const long row0 = (long)blockIdx.x * TM;
  const int valid = (int)min((long)TM, N - row0);
  const MlpParams P = carve(params, D, A);
  const int o = threadIdx.x >> 2, r = o / D, d = o - r * D;
  const bool owner = (threadIdx.x & 3) == 0 && o < TM * D && r < valid;
  load_inputs(xin, start, actions, row0, valid, D, A);
  if (owner) out[(row0 + r) * D + d] = start[(row0 + r) * D + d];
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float delta = mlp_tile(P, D, A, xin, buf, nullptr, 0, valid);
    float nxt = 0.f;
    if (owner) {
      nxt = xin[r * LDX + d] + delta;
      out[((long)(t + 1) * N + row0 + r) * D + d] = nxt;
    }
    __syncthreads();  // layer 4 has read buf, every owner its old state
    if (owner) xin[r * LDX + d] = nxt;
    if (t + 1 < T && threadIdx.x < TM * A) {
      const int ar = threadIdx.x / A, ak = threadIdx.x - ar * A;
      if (ar < valid) xin[ar * LDX + D + ak] = actions[((long)(t + 1) * N + row0 + ar) * A + ak];
    }
    __syncthreads();
  }
}

// Backward, part one: per tile, dy -> dz3 -> dz2 -> dz1 (gradients of the three pre-activations), dz[k][M][512].
__global__ void __launch_bounds__(NTHR) mlp4_dgrad_kernel(const float* params, const float* dy, const float* acts,
                                                          float* dz, long M, int D, int A) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float buf[TM * LDH];
  __shared__ float dys[TM * 8];
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * TM, plane = M * HID;
  const int valid = (int)min((long)TM, M - row0);
  const MlpParams P = carve(params, D, A);
  if (tid < TM * 8) {
    const int r = tid >> 3, d = tid & 7;
    dys[tid] = (r < valid && d < D) ? dy[(row0 + r) * D + d] : 0.f;
  }
  __syncthreads();
  {  // dh3 = dy W4 (K = D <= 7), thread = column
    float w[MAXD];
#pragma unroll
    for (int d = 0; d < MAXD; ++d) w[d] = d < D ? P.W4[(long)d * HID + tid] : 0.f;
    for (int r = 0; r < TM; ++r) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < MAXD; ++d)
        if (d < D) s = fmaf(dys[r * 8 + d], w[d], s);
      float gz = 0.f;
      if (r < valid) {
        gz = acts[2 * plane + (row0 + r) * HID + tid] > 0.f ? s : 0.f;
        dz[2 * plane + (row0 + r) * HID + tid] = gz;
      }
      buf[r * LDH + tid] = gz;
    }
  }
  __syncthreads();
  const int lane = tid & 63, c = lane & 15, g = lane >> 4, n0 = (tid >> 6) * 64;
#pragma unroll 1
  for (int layer = 1; layer >= 0; --layer) {  // dh_{layer+1} = dz_{layer+2} W_{layer+2}, masked by h_{layer+1} > 0
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm512<true>(layer == 1 ? P.W3 : P.W2, buf, acc, n0, c, g);
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r, col = n0 + 16 * nt + c;
        float gz = 0.f;
        if (row < valid) {
          gz = acts[layer * plane + (row0 + row) * HID + col] > 0.f ? acc[nt][r] : 0.f;
          dz[layer * plane + (row0 + row) * HID + col] = gz;
        }
        if (layer == 1) buf[row * LDH + col] = gz;
      }
    __syncthreads();
  }
}

// Backward, parts two and three: dW[o][i] = sum_m G[m][o] H[m][i] and db[o] = sum_m G[m][o], m ascending, one job per
// layer (blockIdx.z).  H's columns may come from two arrays (the first layer's never-materialised x | a).
struct WgradJob {
  const float* G;   // [M][ldG], NO columns used
  const float* H0;  // columns [0, n0) from H0[m][ld0], columns [n0, NI) from H1[m][ld1]
  const float* H1;
  float* dW;        // [NO][NI]
  float* db;        // [NO]
  int ldG, NO, ld0, n0, ld1, NI;
};
struct WgradJobs {
  WgradJob job[4];
};

__global__ void __launch_bounds__(256) mlp4_wgrad_kernel(WgradJobs jobs, long M, int accumulate) {
#pragma clang fp contract(off)
  const WgradJob J = jobs.job[blockIdx.z];
  const int i0 = blockIdx.x * 64, o0 = blockIdx.y * 64;
  if (i0 >= J.NI || o0 >= J.NO) return;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4, wave = tid >> 6;
  const int ob = o0 + 32 * (wave >> 1), ib = i0 + 32 * (wave & 1);
  f32x4 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int oa[2] = {ob + c, ob + 16 + c}, ia[2] = {ib + c, ib + 16 + c};
  for (long m0 = 0; m0 < M; m0 += 4) {  // MFMA k slot g = row m0 + g: rows enter every sum in ascending order
    const long m = m0 + g;
    float a[2], b[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      a[q] = (m < M && oa[q] < J.NO) ? J.G[m * J.ldG + oa[q]] : 0.f;
      float v = 0.f;
      if (m < M && ia[q] < J.NI) v = ia[q] < J.n0 ? J.H0[m * J.ld0 + ia[q]] : J.H1[m * J.ld1 + (ia[q] - J.n0)];
      b[q] = v;
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = ob + 16 * mt + 4 * g + r, i = ib + 16 * nt + c;
        if (o < J.NO && i < J.NI) {
          float* dst = J.dW + (long)o * J.NI + i;
          *dst = accumulate ? *dst + acc[mt][nt][r] : acc[mt][nt][r];
        }
      }
  if (blockIdx.x == 0 && tid < 64 && o0 + tid < J.NO) {  // bias gradient: the column sum of G
    const int o = o0 + tid;
    float s = 0.f;
#pragma unroll 4
    for (long m = 0; m < M; ++m) s = s + J.G[m * J.ldG + o];
    J.db[o] = accumulate ? J.db[o] + s : s;
  }
}

// loss[0] = scale * sum (pred - target)^2, dy = 2 scale (pred - target); one workgroup, a fixed summation order.
__global__ void __launch_bounds__(256) mse_rows_kernel(const float* pred, const float* target, float scale, float* loss,
                                                       float* dy, long n) {
#pragma clang fp contract(off)
  __shared__ float part[256];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) {
    const float d = pred[i] - target[i];
    s = s + d * d;
    if (dy) dy[i] = (2.f * scale) * d;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] * scale;
}

bool dims_ok(int D, int A) { return D >= 1 && D <= MAXD && A >= 1 && A <= MAXA; }

}  // namespace
}  // namespace rac

using namespace rac;
#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

int64_t rac_mlp4_param_count(int32_t D, int32_t A) { return dims_ok(D, A) ? param_count(D, A) : -1; }

int rac_mlp4_fwd(const float* params, const float* x, const float* a, float* y, float* acts, int64_t M, int32_t D,
                 int32_t A, int32_t residual, void* stream) {
  RAC_REQUIRE(params && x && a && y && M > 0 && M < (1L << 34), "rac_mlp4_fwd: bad args");
  RAC_REQUIRE(dims_ok(D, A), "rac_mlp4_fwd: D in 1..%d and A in 1..%d (got %d, %d)", MAXD, MAXA, D, A);
  RAC_REQUIRE(aligned16(params), "rac_mlp4_fwd: the parameter block must be 16-B aligned");
  hipLaunchKernelGGL(mlp4_fwd_kernel, dim3(cdiv(M, TM)), dim3(NTHR), 0, ST(stream), params, x, a, y, acts, (long)M, D, A,
                     residual);
  return check_launch("rac_mlp4_fwd");
}

int rac_robot_rollout(const float* joint_params, const float* gripper_params, const float* q0, const float* s0,
                      const float* actions, float* q_out, float* s_out, int32_t T, int64_t N, int32_t J, int32_t R,
                      int32_t A, void* stream) {
  RAC_REQUIRE((joint_params || gripper_params) && T >= 0 && N > 0 && N < (1L << 34) && (T == 0 || actions),
              "rac_robot_rollout: bad args");
  RAC_REQUIRE(!joint_params || (q0 && q_out && dims_ok(J, A) && aligned16(joint_params)),
              "rac_robot_rollout: joint model needs q0, q_out, J in 1..%d, A in 1..%d, 16-B aligned parameters", MAXD, MAXA);
  RAC_REQUIRE(!gripper_params || (s0 && s_out && dims_ok(R, A) && aligned16(gripper_params)),
              "rac_robot_rollout: gripper model needs s0, s_out, R in 1..%d, A in 1..%d, 16-B aligned parameters", MAXD, MAXA);
  hipLaunchKernelGGL(robot_rollout_kernel, dim3(cdiv(N, TM), 2), dim3(NTHR), 0, ST(stream), joint_params, gripper_params,
                     q0, s0, actions, q_out, s_out, T, (long)N, J, R, A);
  return check_launch("rac_robot_rollout");
}

int rac_mlp4_bwd(const float* params, const float* x, const float* a, const float* acts, const float* dy, float* dz,
                 float* grads, int64_t M, int32_t D, int32_t A, int32_t accumulate, void* stream) {
  RAC_REQUIRE(params && x && a && acts && dy && dz && grads && M > 0 && M < (1L << 34), "rac_mlp4_bwd: bad args");
  RAC_REQUIRE(dims_ok(D, A), "rac_mlp4_bwd: D in 1..%d and A in 1..%d (got %d, %d)", MAXD, MAXA, D, A);
  RAC_REQUIRE(aligned16(params), "rac_mlp4_bwd: the parameter block must be 16-B aligned");
  hipLaunchKernelGGL(mlp4_dgrad_kernel, dim3(cdiv(M, TM)), dim3(NTHR), 0, ST(stream), params, dy, acts, dz, (long)M, D, A);
  if (int e = check_launch("rac_mlp4_bwd (dgrad chain)")) return e;
  const MlpParams G = carve(grads, D, A);  // the gradient block has the parameter block's layout
  const long plane = (long)M * HID;
  WgradJobs jobs;
  jobs.job[0] = {dz, x, a, const_cast<float*>(G.W1), const_cast<float*>(G.b1), HID, HID, D, D, A, D + A};
  jobs.job[1] = {dz + plane, acts, nullptr, const_cast<float*>(G.W2), const_cast<float*>(G.b2), HID, HID, HID, HID, 0, HID};
  jobs.job[2] = {dz + 2 * plane, acts + plane, nullptr, const_cast<float*>(G.W3), const_cast<float*>(G.b3), HID, HID, HID,
                 HID, 0, HID};
  jobs.job[3] = {dy, acts + 2 * plane, nullptr, const_cast<float*>(G.W4), const_cast<float*>(G.b4), D, D, HID, HID, 0, HID};
  hipLaunchKernelGGL(mlp4_wgrad_kernel, dim3(HID / 64, HID / 64, 4), dim3(256), 0, ST(stream), jobs, (long)M, accumulate);
  return check_launch("rac_mlp4_bwd (weight gradients)");
}

int rac_mse_rows(const float* pred, const float* target, float scale, float* loss, float* dy, int64_t n, void* stream) {
  RAC_REQUIRE(pred && target && loss && n > 0, "rac_mse_rows: bad args");
  hipLaunchKernelGGL(mse_rows_kernel, dim3(1), dim3(256), 0, ST(stream), pred, target, scale, loss, dy, (long)n);
  return check_launch("rac_mse_rows");
}

}  // extern "C"
RAC_DEVICE_CODE_END
