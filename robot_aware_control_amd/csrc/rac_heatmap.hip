// End-effector heatmaps of a whole batch in one launch (robonet_dataset.py:482-544 create_heatmaps, :420-431
// get_2d_eef_pos, src/utils/gaussian.py gaus2d): the `heatmaps` input of --model_use_heatmap.
#include "rac_common.h"

extern "C" int rac_heatmap_view_bytes(void) { return (int)sizeof(rac_heatmap_view); }

namespace rac {

constexpr int HM_THREADS = 256;
constexpr float HM_PEAK = 0.63661977236758134f;  // 100 / (2 pi 5 5): gaus2d's height / (2 pi sx sy)

// The centre of one frame.  The reference's order and precisions: the denormalisation and the z offset in fp32 with a
// separate multiply and add (torch), everything behind them in fp64 (numpy), nothing contracted into an fma.
// `valid` is 0 <= trunc(x) < W and 0 <= trunc(y) < H, tested on the fp64 coordinates (trunc(x) >= 0 is x > -1), so no
// value is ever cast out of range; a NaN fails every comparison.  mx / my of an invalid frame are the truncated
// coordinates saturated to int32, or 0 where they are not finite.
__device__ __forceinline__ void eef_centre(const float* s, const float* low, const float* high,
                                           const rac_heatmap_view& v, int H, int W, int& mx, int& my, int& valid) {
#pragma clang fp contract(off)
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = __fadd_rn(__fmul_rn(s[k], __fsub_rn(high[k], low[k])), low[k]);
  p[2] = __fadd_rn(p[2], v.z_offset);
  const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
  double pix[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    pix[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(v.proj[4 * r], X), __dmul_rn(v.proj[4 * r + 1], Y)),
                                 __dmul_rn(v.proj[4 * r + 2], Z)),
                       v.proj[4 * r + 3]);
  const double x = __dmul_rn(pix[0] / pix[2], v.scale_x), y = __dmul_rn(pix[1] / pix[2], v.scale_y);
  valid = (x > -1.0 && x < (double)W && y > -1.0 && y < (double)H) ? 1 : 0;
  const bool fin = isfinite(x) && isfinite(y);
  mx = fin ? (int)fmin(fmax(x, -2147483648.0), 2147483647.0) : 0;
  my = fin ? (int)fmin(fmax(y, -2147483648.0), 2147483647.0) : 0;
}

// grid T B, 256 threads: workgroup f = t B + b writes frame (t, b) and nothing else.  Every thread derives the centre
// itself (a few dozen flops on wave-uniform values; no LDS, no barrier), then the workgroup streams the frame out: VEC
// with one 16-byte store per four pixels of a row (W % 4 == 0, strides and base allow it), the other form pixel by
// pixel; a pixel's value is the same expression in both.  (x - mx)^2 + (y - my)^2 is an exact integer in fp32.
template <bool VEC>
__global__ void __launch_bounds__(HM_THREADS) eef_heatmaps_kernel(const float* states, long s_fs, long s_vs,
                                                                  const float* low, const float* high, long b_vs,
                                                                  const rac_heatmap_view* views, float* out, long o_fs,
                                                                  long o_vs, int* centres, int B, int H, int W) {
  const int f = blockIdx.x, t = f / B, b = f - t * B;
  int mx, my, valid;
  eef_centre(states + (long)t * s_fs + (long)b * s_vs, low + (long)b * b_vs, high + (long)b * b_vs, views[b], H, W, mx, my,
             valid);
  if (centres && threadIdx.x == 0) {
    int* c = centres + (long)f * 3;
    c[0] = mx, c[1] = my, c[2] = valid;
  }
  float* o = out + (long)t * o_fs + (long)b * o_vs;
  const int HW = H * W;
  if (VEC) {
    for (int q = threadIdx.x; q < (HW >> 2); q += HM_THREADS) {
      const int p0 = q * 4, y = p0 / W, x0 = p0 - y * W;
      f32x4 r = {0.f, 0.f, 0.f, 0.f};
      if (valid) {
        const int dy2 = (y - my) * (y - my);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int dx = x0 + j - mx;
          r[j] = HM_PEAK * expf(-(float)(dx * dx + dy2) / 50.f);
        }
      }
      *reinterpret_cast<f32x4*>(o + p0) = r;
    }
  } else {
    for (int p = threadIdx.x; p < HW; p += HM_THREADS) {
      const int y = p / W, dx = p - y * W - mx, dy = y - my;
      o[p] = valid ? HM_PEAK * expf(-(float)(dx * dx + dy * dy) / 50.f) : 0.f;
    }
  }
}

}  // namespace rac

extern "C" int rac_eef_heatmaps(const float* states, int64_t state_frame_stride, int64_t state_video_stride,
                                const float* low, const float* high, int64_t bound_stride,
                                const rac_heatmap_view* views, float* heatmaps, int64_t out_frame_stride,
                                int64_t out_video_stride, int32_t* centres, int32_t T, int32_t B, int32_t H, int32_t W,
                                void* stream) {
  using namespace rac;
  RAC_REQUIRE(states && low && high && views && heatmaps && T >= 1 && B >= 1 && H >= 1 && W >= 1 &&
                  state_frame_stride >= 0 && state_video_stride >= 0 && bound_stride >= 0 && out_frame_stride >= 0 &&
                  out_video_stride >= 0,
              "rac_eef_heatmaps: bad args");
  RAC_REQUIRE(H <= 2048 && W <= 2048 && (long)T * B < (1L << 31), "rac_eef_heatmaps: H, W <= 2048 and T B < 2^31");
  RAC_REQUIRE((reinterpret_cast<uintptr_t>(views) & 7u) == 0, "rac_eef_heatmaps: views must be 8-byte aligned");
  const bool vec = W % 4 == 0 && out_frame_stride % 4 == 0 && out_video_stride % 4 == 0 && aligned16(heatmaps);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(eef_heatmaps_kernel<true>, dim3(T * B), dim3(HM_THREADS), 0, st, states, state_frame_stride,
                       state_video_stride, low, high, bound_stride, views, heatmaps, out_frame_stride, out_video_stride,
                       centres, B, H, W);
  else
    hipLaunchKernelGGL(eef_heatmaps_kernel<false>, dim3(T * B), dim3(HM_THREADS), 0, st, states, state_frame_stride,
                       state_video_stride, low, high, bound_stride, views, heatmaps, out_frame_stride, out_video_stride,
                       centres, B, H, W);
  return check_launch("rac_eef_heatmaps");
}

RAC_DEVICE_CODE_END
