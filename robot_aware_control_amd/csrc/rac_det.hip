// The deterministic baselines' own kernels (reference dynamics.py:341-454): the ConvLSTM input of
// DeterministicConvModel -- [encoder map | action_encoder(a) | state_encoder(r) | zeros up to the padded width] -- written
// in one launch, its backward pass (encoder-map gradient + both Linears' weight / bias gradients, fixed summation order,
// no float atomics), and CopyModel's masked select.  All three are bandwidth- and latency-bound: 16 B per lane where the
// data is a map, grid-stride over at most 2048 workgroups of 256.
#include "rac_common.h"

namespace rac {

static inline int det_grid(long work_items, const void* amax) {
  long b = (work_items + 255) / 256;
  const long cap = amax ? 512 : 2048;  // (a kernel that commits a max |v| slot: one atomic per workgroup on ONE address)
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// y = bias[o] + sum_k w[o][k] * v[b][k], k ascending (fp32, at most one rounding per term)
__device__ __forceinline__ float det_linear(const float* w, const float* bias, const float* v, int n, long o, int b) {
  float acc = bias[o];
  for (int k = 0; k < n; ++k) acc = fmaf(w[o * n + k], v[(long)b * n + k], acc);
  return acc;
}

// out [B][HW][Gp] in 4-channel groups: groups below g/4 copy the encoder map, group g/4 holds the two action lanes and the
// two state lanes (Linear outputs viewed (B, 2, h, w): lane ch of pixel p is output ch*HW + p), the rest is zero
__global__ void det_pack_fwd_kernel(const f32x4* enc, int g4, const float* act, int A, const float* wa, const float* ba,
                                    const float* st, int R, const float* ws, const float* bs, f32x4* out, int Gp4, int B,
                                    int HW, unsigned* amax) {
  const long n = (long)B * HW * Gp4;
  unsigned mx = 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % Gp4);
    const long q = i / Gp4;  // b*HW + p
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c4 < g4) {
      v = enc[q * g4 + c4];
    } else if (c4 == g4) {
      const int b = (int)(q / HW);
      const long p = q % HW;
      v.x = det_linear(wa, ba, act, A, p, b);
      v.y = det_linear(wa, ba, act, A, HW + p, b);
      if (st) {
        v.z = det_linear(ws, bs, st, R, p, b);
        v.w = det_linear(ws, bs, st, R, HW + p, b);
      }
    }
    mx = max(mx, max(max(absbits(v.x), absbits(v.y)), max(absbits(v.z), absbits(v.w))));
    out[i] = v;
  }
  if (amax) amax_commit_block(mx, amax);
}

// work items [0, n_copy): denc[q][c4] = dout[q][c4] (the encoder lanes of the gradient, 16 B each);
// then one thread per Linear weight / bias element: dw[o][k] += sum_b d[b][o] * v[b][k], db[o] += sum_b d[b][o], b ascending
__global__ void det_pack_bwd_kernel(const float* dout, int Gp, int g, const float* act, int A, const float* st, int R,
                                    f32x4* denc, float* dwa, float* dba, float* dws, float* dbs, int B, int HW) {
  const int g4 = g / 4, Gp4 = Gp / 4;
  const long n_copy = denc ? (long)B * HW * g4 : 0;
  const long n_a = dwa ? (long)2 * HW * (A + 1) : 0;
  const long n_s = dws ? (long)2 * HW * (R + 1) : 0;
  const long n = n_copy + n_a + n_s;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (i < n_copy) {
      const long q = i / g4;
      denc[i] = reinterpret_cast<const f32x4*>(dout)[q * Gp4 + (i % g4)];
      continue;
    }
    long j = i - n_copy;
    const bool is_state = j >= n_a;
    if (is_state) j -= n_a;
    const int nk = is_state ? R : A;
    const float* v = is_state ? st : act;
    float* dw = is_state ? dws : dwa;
    float* db = is_state ? dbs : dba;
    const long o = j / (nk + 1);  // ch*HW + p
    const int k = (int)(j % (nk + 1));  // k == nk: the bias
    const long col = g + (is_state ? 2 : 0) + o / HW;
    const long p = o % HW;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      const float d = dout[((long)b * HW + p) * Gp + col];
      acc = k < nk ? fmaf(d, v[(long)b * nk + k], acc) : acc + d;
    }
    if (k < nk)
      dw[o * nk + k] += acc;
    else
      db[o] += acc;
  }
}

// out[b][c][p] = next_mask[b][p] != 0 ? next_image[b][c][p] : image[b][c][p]   (NCHW planes, 3 channels, 1 mask plane)
__global__ void copy_baseline_kernel(const float* image, const float* next_image, const float* next_mask, float* out,
                                     int B, int HW) {
  const long n = (long)B * 3 * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long b = i / (3L * HW);
    const long p = i % HW;
    out[i] = next_mask[b * HW + p] != 0.f ? next_image[i] : image[i];
  }
}

}  // namespace rac

using namespace rac;
#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

int rac_det_pack_fwd(const float* enc, int32_t g, const float* action, int32_t A, const float* wa, const float* ba,
                     const float* state, int32_t R, const float* ws, const float* bs, float* out, int32_t Gp, int32_t B,
                     int32_t HW, uint32_t* out_amax, void* stream) {
  RAC_REQUIRE(enc && action && wa && ba && out && B > 0 && HW > 0 && A > 0, "rac_det_pack_fwd: bad args");
  RAC_REQUIRE(g > 0 && g % 4 == 0 && Gp % 4 == 0 && Gp >= g + 4, "rac_det_pack_fwd: g %% 4 == 0, Gp %% 4 == 0, Gp >= g + 4");
  RAC_REQUIRE(state ? (ws && bs && R > 0) : true, "rac_det_pack_fwd: state without its Linear");
  RAC_REQUIRE(aligned16(enc) && aligned16(out), "rac_det_pack_fwd: 16-byte aligned maps");
  const long n = (long)B * HW * (Gp / 4);
  hipLaunchKernelGGL(det_pack_fwd_kernel, dim3(det_grid(n, out_amax)), dim3(256), 0, ST(stream), (const f32x4*)enc, g / 4,
                     action, A, wa, ba, state, R, ws, bs, (f32x4*)out, Gp / 4, B, HW, out_amax);
  return check_launch("rac_det_pack_fwd");
}

int rac_det_pack_bwd(const float* dout, int32_t Gp, int32_t g, const float* action, int32_t A, const float* state,
                     int32_t R, float* denc, float* dwa, float* dba, float* dws, float* dbs, int32_t B, int32_t HW,
                     void* stream) {
  RAC_REQUIRE(dout && B > 0 && HW > 0, "rac_det_pack_bwd: bad args");
  RAC_REQUIRE(g > 0 && g % 4 == 0 && Gp % 4 == 0 && Gp >= g + 4, "rac_det_pack_bwd: g %% 4 == 0, Gp %% 4 == 0, Gp >= g + 4");
  RAC_REQUIRE((dwa == nullptr) == (dba == nullptr) && (!dwa || (action && A > 0)),
              "rac_det_pack_bwd: dwa / dba come together, with the action");
  RAC_REQUIRE((dws == nullptr) == (dbs == nullptr) && (!dws || (state && R > 0)),
              "rac_det_pack_bwd: dws / dbs come together, with the state");
  RAC_REQUIRE(denc || dwa || dws, "rac_det_pack_bwd: nothing to write");
  RAC_REQUIRE(aligned16(dout) && (!denc || aligned16(denc)), "rac_det_pack_bwd: 16-byte aligned maps");
  const long n = (denc ? (long)B * HW * (g / 4) : 0) + (dwa ? 2L * HW * (A + 1) : 0) + (dws ? 2L * HW * (R + 1) : 0);
  hipLaunchKernelGGL(det_pack_bwd_kernel, dim3(det_grid(n, nullptr)), dim3(256), 0, ST(stream), dout, Gp, g, action, A,
                     state, R, (f32x4*)denc, dwa, dba, dws, dbs, B, HW);
  return check_launch("rac_det_pack_bwd");
}

int rac_copy_baseline(const float* image, const float* next_image, const float* next_mask, float* out, int32_t B,
                      int32_t HW, void* stream) {
  RAC_REQUIRE(image && next_image && next_mask && out && B > 0 && HW > 0, "rac_copy_baseline: bad args");
  hipLaunchKernelGGL(copy_baseline_kernel, dim3(det_grid((long)B * 3 * HW, nullptr)), dim3(256), 0, ST(stream), image,
                     next_image, next_mask, out, B, HW);
  return check_launch("rac_copy_baseline");
}

}  // extern "C"

RAC_DEVICE_CODE_END
