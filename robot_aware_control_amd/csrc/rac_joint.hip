// The learned robot model's data path and its plot (reference src/dataset/joint_pos_dataset.py and
// src/prediction/joint_pos_trainer.py `plot` / `_compute_iou`):
//   * joint_batch_kernel gathers one training batch from the device-resident split and applies the dataset's numeric
//     preprocessing -- the imputed gripper command, `state_infer` actions, the gripper-force normalisation -- in the
//     precision numpy / torch use on the host, so the batch has the bits of process_batch(collate(host items));
//   * mask_compare_kernel counts intersection and union of predicted and true masks per frame and writes the
//     [true | predicted | xor] comparison frames of the GIF;
//   * window_gather_kernel copies the windows of one batch out of up to 8 resident fp32 tables (the video path's
//     preprocessed numerics, data.py ResidentVideos) into time-first outputs: a pure copy, one writer per element.
// All are latency-sized: one thread per output element / one workgroup per frame, no atomics, fixed-order reductions.
#include <algorithm>

#include "rac_common.h"

namespace rac {
namespace {

constexpr int GRIP = 4;  // the gripper-force column of a state (joint_pos_dataset.py:139-140)

struct JointSplit {
  const double* states;  // [N][Tmax][R]  as stored (fp32 files widened: exact)
  const float* actions;  // [N][Tmax-1][A] `.astype(float32)`, the file's own columns first
  const float* qpos;     // [N][Tmax][J]   `.astype(float32)`
  const double* bounds;  // [N][2][R]      low, high (fp32 files widened: exact)
  const int* meta;       // [N][3]         length, action width, 1 when the bounds are stored as float64
  int N, Tmax, J, R, A;
};

// states[t][c] denormalised as `_denormalize` assigns it into the float32 window (joint_pos_dataset.py:150-153,187):
// float64 bounds promote the product and the sum to float64, rounded once by the assignment.
__device__ __forceinline__ float denorm(float s, double low, double high, bool f64) {
#pragma clang fp contract(off)
  if (f64) {
    double d = (double)s * (high - low);
    d = d + low;
    return (float)d;
  }
  float d = s * ((float)high - (float)low);
  d = d + (float)low;
  return d;
}

__global__ void __launch_bounds__(256) joint_batch_kernel(JointSplit S, const int* __restrict__ index,
                                                          const int* __restrict__ start, float* __restrict__ qpos_out,
                                                          float* __restrict__ states_out, float* __restrict__ actions_out,
                                                          int B, int L, int state_infer) {
#pragma clang fp contract(off)
  const long nq = (long)L * B * S.J, ns = (long)L * B * S.R, na = (long)(L - 1) * B * S.A;
  long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nq + ns + na) return;
  const int which = e < nq ? 0 : (e < nq + ns ? 1 : 2);
  if (which == 1) e -= nq;
  if (which == 2) e -= nq + ns;
  const int width = which == 0 ? S.J : (which == 1 ? S.R : S.A);
  const int c = (int)(e % width);
  const int b = (int)((e / width) % B);
  const int l = (int)(e / ((long)width * B));
  // the tables were checked on the host; the clamps keep any value inside the resident arrays regardless
  const int n = min(max(index[b], 0), S.N - 1);
  const int len = min(max(S.meta[3 * n], L), S.Tmax);
  const int t = min(max(start[b], 0), len - L) + l;
  const int adim = S.meta[3 * n + 1];
  const bool f64 = S.meta[3 * n + 2] != 0;
  const double* low = S.bounds + (long)n * 2 * S.R;
  const double* high = low + S.R;
  const double* st = S.states + ((long)n * S.Tmax + t) * S.R;
  if (which == 0) {
    qpos_out[e] = S.qpos[((long)n * S.Tmax + t) * S.J + c];
  } else if (which == 1) {
    float s = (float)st[c];
    if (c == GRIP) {  // torch on the float32 tensor: both scalars rounded to float32 first
      const float fmin = (float)low[GRIP];
      const float span = f64 ? (float)(high[GRIP] - low[GRIP]) : (float)high[GRIP] - (float)low[GRIP];
      s = (s - fmin) / span;
    }
    states_out[e] = s;
  } else {
    float a;
    if (state_infer && c < 3) {  // what happened between the states, not the recorded action
      a = denorm((float)st[S.R + c], low[c], high[c], f64) - denorm((float)st[c], low[c], high[c], f64);
    } else if (c < adim) {
      a = S.actions[((long)n * (S.Tmax - 1) + t) * S.A + c];
    } else {  // the imputed gripper command: the next STORED state's last column against the bounds' midpoint
      const double lo = low[S.R - 1], hi = high[S.R - 1];
      const double mid = f64 ? (hi + lo) / 2.0 : (double)(((float)hi + (float)lo) / 2.0f);
      a = (float)(st[S.R + S.R - 1] > mid ? hi : lo);
    }
    actions_out[e] = a;
  }
}

struct GatherTables {
  rac_gather_table t[RAC_GATHER_MAX_TABLES];
  long first[RAC_GATHER_MAX_TABLES + 1];  // element offsets of the tables in the launch's flat element range
  int n;
};

// dst[r][b][c] = src[v][s + r][c] per table, v = index[b], s = start[b] (0 for a per-video table).  index, start and
// length were checked on the host; the clamps keep any value inside the tables regardless.  Scalar 4-byte accesses:
// widths such as 5 and 7 leave no wider alignment.
__global__ void __launch_bounds__(256) window_gather_kernel(GatherTables G, const int* __restrict__ index,
                                                            const int* __restrict__ start, const int* __restrict__ length,
                                                            int V, int B, int L) {
  const long total = G.first[G.n];
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int k = 0;
    while (k + 1 < G.n && e >= G.first[k + 1]) ++k;
    const rac_gather_table T = G.t[k];
    const long i = e - G.first[k];
    const int c = (int)(i % T.width);
    const int b = (int)((i / T.width) % B);
    const int r = (int)(i / ((long)T.width * B));
    const int v = min(max(index[b], 0), V - 1);
    int s = 0;
    if (!T.per_video) {
      const int len = max(length[v], L);
      s = min(min(max(start[b], 0), len - L), T.rows_stored - T.rows);
    }
    T.dst[i] = T.src[((long)v * T.rows_stored + s + r) * T.width + c];
  }
}

// One workgroup per (video, time step) frame of H x W pixels.  counts[frame] = {|pred & true|, |pred | true|} (a mask is
// set where it is nonzero); frames[t][v H + y][x + {0, W, 2 W}] = true, predicted (clamped to [0, 1], times 255,
// truncated) and 255 where exactly one of them is set.
__global__ void __launch_bounds__(256) mask_compare_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                           int* __restrict__ counts, unsigned char* __restrict__ frames,
                                                           int V, int T, int H, int W) {
#pragma clang fp contract(off)
  __shared__ int part[2][256];
  const int v = blockIdx.x / T, t = blockIdx.x % T;
  const long px = (long)H * W;
  const float* p = pred + ((long)v * T + t) * px;
  const float* q = truth + ((long)v * T + t) * px;
  unsigned char* out = frames + ((long)t * V + v) * px * 3;
  int inter = 0, uni = 0;
  for (long i = threadIdx.x; i < px; i += 256) {
    const float pv = p[i], qv = q[i];
    const bool ps = pv != 0.f, qs = qv != 0.f;
    inter += ps && qs;
    uni += ps || qs;
    unsigned char* row = out + (i / W) * 3L * W + (i % W);
    row[0] = (unsigned char)(fminf(fmaxf(qv, 0.f), 1.f) * 255.f);
    row[W] = (unsigned char)(fminf(fmaxf(pv, 0.f), 1.f) * 255.f);
    row[2 * W] = ps != qs ? 255 : 0;
  }
  part[0][threadIdx.x] = inter;
  part[1][threadIdx.x] = uni;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      part[0][threadIdx.x] += part[0][threadIdx.x + w];
      part[1][threadIdx.x] += part[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[2 * blockIdx.x] = part[0][0];
    counts[2 * blockIdx.x + 1] = part[1][0];
  }
}

}  // namespace
}  // namespace rac

using namespace rac;
#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

int rac_joint_batch(const double* states, const float* actions, const float* qpos, const double* bounds,
                    const int32_t* meta, const int32_t* index, const int32_t* start, float* qpos_out, float* states_out,
                    float* actions_out, int32_t N, int32_t Tmax, int32_t B, int32_t L, int32_t J, int32_t R, int32_t A,
                    int32_t state_infer, void* stream) {
  RAC_REQUIRE(states && actions && qpos && bounds && meta && index && start && qpos_out && states_out && actions_out,
              "rac_joint_batch: NULL argument");
  RAC_REQUIRE(N >= 1 && B >= 1 && L >= 2 && L <= Tmax, "rac_joint_batch: N %d, B %d and a window 2 <= L (%d) <= Tmax (%d)",
              N, B, L, Tmax);
  RAC_REQUIRE(J >= 1 && R > GRIP && A >= 1 && (!state_infer || A >= 3),
              "rac_joint_batch: J %d >= 1, R %d >= 5, A %d >= 1 (>= 3 for state_infer)", J, R, A);
  const long total = (long)L * B * (J + R) + (long)(L - 1) * B * A;
  RAC_REQUIRE(total < (1L << 31), "rac_joint_batch: %ld output elements", total);
  const JointSplit S = {states, actions, qpos, bounds, meta, N, Tmax, J, R, A};
  hipLaunchKernelGGL(joint_batch_kernel, dim3(cdiv(total, 256)), dim3(256), 0, ST(stream), S, index, start, qpos_out,
                     states_out, actions_out, B, L, state_infer);
  return check_launch("rac_joint_batch");
}

int rac_window_gather(const rac_gather_table* tables, int32_t n_tables, const int32_t* index, const int32_t* start,
                      const int32_t* length, int32_t V, int32_t B, int32_t L, void* stream) {
  RAC_REQUIRE(tables && index && start && length, "rac_window_gather: NULL argument");
  RAC_REQUIRE(n_tables >= 1 && n_tables <= RAC_GATHER_MAX_TABLES, "rac_window_gather: %d tables, 1..%d in one launch",
              n_tables, RAC_GATHER_MAX_TABLES);
  RAC_REQUIRE(V >= 1 && B >= 1 && L >= 1, "rac_window_gather: V %d, B %d, L %d must be >= 1", V, B, L);
  GatherTables G = {};
  G.n = n_tables;
  G.first[0] = 0;
  for (int k = 0; k < n_tables; ++k) {
    const rac_gather_table& t = tables[k];
    RAC_REQUIRE(t.src && t.dst, "rac_window_gather: table %d has a NULL pointer", k);
    RAC_REQUIRE(t.width >= 1 && t.rows >= 1 && t.rows_stored >= t.rows,
                "rac_window_gather: table %d: width %d, %d rows of %d stored", k, t.width, t.rows, t.rows_stored);
    RAC_REQUIRE(t.per_video ? t.rows == 1 : (t.rows == L || t.rows == L - 1),
                "rac_window_gather: table %d: %d rows for a window of %d (L or L - 1; 1 for a per-video table)", k, t.rows,
                L);
    G.t[k] = t;
    G.first[k + 1] = G.first[k] + (long)t.rows * B * t.width;
    RAC_REQUIRE((long)V * t.rows_stored * t.width < (1L << 31) && G.first[k + 1] < (1L << 31),
                "rac_window_gather: table %d is too large (V %d x %d rows x %d)", k, V, t.rows_stored, t.width);
  }
  const int blocks = (int)std::min<long>(cdiv(G.first[n_tables], 256), 1024);
  hipLaunchKernelGGL(window_gather_kernel, dim3(blocks), dim3(256), 0, ST(stream), G, index, start, length, V, B, L);
  return check_launch("rac_window_gather");
}

int rac_mask_compare(const float* pred, const float* truth, int32_t* counts, uint8_t* frames, int32_t V, int32_t T,
                     int32_t H, int32_t W, void* stream) {
  RAC_REQUIRE(pred && truth && counts && frames, "rac_mask_compare: NULL argument");
  RAC_REQUIRE(V >= 1 && T >= 1 && H >= 1 && W >= 1 && (long)H * W < (1L << 31) && (long)V * T < (1L << 31),
              "rac_mask_compare: V %d, T %d, H %d, W %d", V, T, H, W);
  hipLaunchKernelGGL(mask_compare_kernel, dim3(V * T), dim3(256), 0, ST(stream), pred, truth, counts, frames, V, T, H, W);
  return check_launch("rac_mask_compare");
}

}  // extern "C"
RAC_DEVICE_CODE_END
