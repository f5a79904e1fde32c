// The image half of the data path on the device (data.py ImagePipeline, reference robonet_dataset.py:257-300,545-572):
// raw uint8 frames and 0 / 1 masks of a batch -> the time-first fp32 `images` (T, B, 3, h, w) / `masks` (T, B, 1, h, w)
// the trainer consumes, in ONE launch: u8 / 255, bilinear resize to the model size, the trajectory's crop + resize back
// and its colour jitter, with the parameters the dataset drew on the host (struct rac_image_job, one per video).
//
// A workgroup owns one frame (t, b); a thread owns pixel quads (4 consecutive pixels of one output row, w % 4 == 0:
// float4 stores).  Nothing but the output is written: the cropped resize evaluates the first resize in place at each of
// its four taps (<= 16 raw taps per pixel, every index clamped into the raw frame).  The contrast step needs the mean
// of the frame's gray values as the image stands when that step runs, so a jittered frame is walked twice by the SAME
// instructions: pass 0 stops at the contrast step and sums gray (per thread in quad order, butterfly over the wave, the
// four wave sums in wave order: a fixed order, no atomics), pass 1 recomputes the pixel, goes through all four steps and
// stores.  Every fp32 expression is the host pipeline's, one rounding per operation (contraction off), so the result
// differs from torch's only where torch's kernels order a sum differently.
#include "rac_common.h"

namespace rac {

// One axis of torch's bilinear rule, align_corners=False (area_pixel_compute_source_index + guard_index_and_lambda):
// src = max(scale * (o + 0.5) - 0.5, 0) with the product and the difference rounded separately, so that a weight is
// exactly zero where torch's is.
struct AxisTap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ AxisTap axis_tap(int o, float scale, int in) {
#pragma clang fp contract(off)
  const float src = fmaxf(__fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f), 0.f);
  AxisTap t;
  t.i0 = min((int)src, in - 1);
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(__fsub_rn(src, (float)t.i0), 0.f), 1.f);
  t.l0 = __fsub_rn(1.f, t.l1);
  return t;
}

__device__ __forceinline__ float lerp2(const AxisTap& ty, const AxisTap& tx, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
  return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

struct FrameSrc {
  const unsigned char* rgb;   // (Hs, Ws, 3) of this frame
  const unsigned char* mask;  // (Hs, Ws) 0 / 1 of this frame
  int Hs, Ws;
  int h, w;      // the model size: stage 1's output
  float sy, sx;  // (float)Hs / h, (float)Ws / w
  bool same;     // raw size == model size: stage 1 is the identity
};

__device__ __forceinline__ float unit_of(unsigned char v) { return __fdiv_rn((float)v, 255.f); }

// stage 1 at pixel (y, x) of the model-size image: u8 / 255 resized from (Hs, Ws)
__device__ __forceinline__ void stage1_rgb(const FrameSrc& s, int y, int x, float (&out)[3]) {
  y = min(max(y, 0), s.h - 1), x = min(max(x, 0), s.w - 1);  // into the model-size image (a crop window inside it never
                                                             // needs this; axis_tap keeps the raw taps inside the frame)
  if (s.same) {
    const unsigned char* p = s.rgb + ((long)y * s.Ws + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = unit_of(p[c]);
    return;
  }
  const AxisTap ty = axis_tap(y, s.sy, s.Hs), tx = axis_tap(x, s.sx, s.Ws);
  const unsigned char* r0 = s.rgb + (long)ty.i0 * s.Ws * 3;
  const unsigned char* r1 = s.rgb + (long)ty.i1 * s.Ws * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[c] = lerp2(ty, tx, unit_of(r0[tx.i0 * 3 + c]), unit_of(r0[tx.i1 * 3 + c]), unit_of(r1[tx.i0 * 3 + c]),
                   unit_of(r1[tx.i1 * 3 + c]));
}

__device__ __forceinline__ float stage1_mask(const FrameSrc& s, int y, int x) {
  y = min(max(y, 0), s.h - 1), x = min(max(x, 0), s.w - 1);
  if (s.same) return (float)s.mask[(long)y * s.Ws + x];
  const AxisTap ty = axis_tap(y, s.sy, s.Hs), tx = axis_tap(x, s.sx, s.Ws);
  const unsigned char* r0 = s.mask + (long)ty.i0 * s.Ws;
  const unsigned char* r1 = s.mask + (long)ty.i1 * s.Ws;
  return lerp2(ty, tx, (float)r0[tx.i0], (float)r0[tx.i1], (float)r1[tx.i0], (float)r1[tx.i1]);
}

struct Crop {
  int top, left, th, tw;
  float sy, sx;  // (float)th / h, (float)tw / w
  bool on;       // (th, tw) != (h, w)
};

__device__ __forceinline__ void geometry_rgb(const FrameSrc& s, const Crop& c, int y, int x, float (&out)[3]) {
  if (!c.on) {
    stage1_rgb(s, y, x, out);
    return;
  }
  const AxisTap ty = axis_tap(y, c.sy, c.th), tx = axis_tap(x, c.sx, c.tw);
  float v[4][3];
  stage1_rgb(s, c.top + ty.i0, c.left + tx.i0, v[0]);
  stage1_rgb(s, c.top + ty.i0, c.left + tx.i1, v[1]);
  stage1_rgb(s, c.top + ty.i1, c.left + tx.i0, v[2]);
  stage1_rgb(s, c.top + ty.i1, c.left + tx.i1, v[3]);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = lerp2(ty, tx, v[0][ch], v[1][ch], v[2][ch], v[3][ch]);
}

__device__ __forceinline__ float geometry_mask(const FrameSrc& s, const Crop& c, int y, int x) {
  float v;
  if (!c.on) {
    v = stage1_mask(s, y, x);
  } else {
    const AxisTap ty = axis_tap(y, c.sy, c.th), tx = axis_tap(x, c.sx, c.tw);
    v = lerp2(ty, tx, stage1_mask(s, c.top + ty.i0, c.left + tx.i0), stage1_mask(s, c.top + ty.i0, c.left + tx.i1),
              stage1_mask(s, c.top + ty.i1, c.left + tx.i0), stage1_mask(s, c.top + ty.i1, c.left + tx.i1));
  }
  return v != 0.f ? 1.f : 0.f;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float gray_of(const float (&p)[3]) {
#pragma clang fp contract(off)
  return 0.2989f * p[0] + 0.587f * p[1] + 0.114f * p[2];
}

// data.py _adjust_hue on one pixel: rgb -> hsv, h + factor (mod 1), hsv -> rgb, with its guards for gray pixels
__device__ __forceinline__ void adjust_hue(float (&px)[3], float factor) {
#pragma clang fp contract(off)
  const float r = px[0], g = px[1], b = px[2];
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float crd = eqc ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const float hr = (maxc == r ? 1.f : 0.f) * (bc - gc);
  const float hg = ((maxc == g) && (maxc != r) ? 1.f : 0.f) * (2.0f + rc - bc);
  const float hb = ((maxc != g) && (maxc != r) ? 1.f : 0.f) * (4.0f + gc - rc);
  float h = fmodf((hr + hg + hb) / 6.0f + 1.0f, 1.0f);
  h = fmodf(h + factor, 1.0f);  // torch's `%`: the sign of the divisor
  if (h < 0.f) h = h + 1.0f;
  const float v = maxc;
  const float h6 = h * 6.0f;
  const float fl = floorf(h6);
  const float f = h6 - fl;
  const int i = ((int)fl) % 6;
  const float p = clamp01(v * (1.0f - s));
  const float q = clamp01(v * (1.0f - s * f));
  const float t = clamp01(v * (1.0f - s * (1.0f - f)));
  px[0] = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  px[1] = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  px[2] = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

struct Jitter {
  int order;  // step k's operation in bits [2k, 2k + 2)
  float bf, cf, cf1, sf, sf1, hf;  // cf1 = (float)(1 - cf), sf1 = (float)(1 - sf), the differences taken in double
};

// The jitter steps [0, n_steps) in the job's order; `mean` is the contrast step's gray mean (unused before that step).
__device__ __forceinline__ void jitter_pixel(float (&px)[3], const Jitter& j, int n_steps, float mean) {
#pragma clang fp contract(off)
#pragma unroll 1
  for (int k = 0; k < n_steps; ++k) {
    const int op = (j.order >> (2 * k)) & 3;
    if (op == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = clamp01(px[c] * j.bf);
    } else if (op == 1) {
      const float m = j.cf1 * mean;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = clamp01(j.cf * px[c] + m);
    } else if (op == 2) {
      const float g = j.sf1 * gray_of(px);
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = clamp01(j.sf * px[c] + g);
    } else {
      adjust_hue(px, j.hf);
    }
  }
}

__global__ __launch_bounds__(256) void image_pipeline_kernel(const unsigned char* frames, const unsigned char* masks,
                                                             const rac_image_job* jobs, float* images, float* out_masks,
                                                             int B, int h, int w) {
  __shared__ float wave_part[4];
  const int t = blockIdx.x / B, b = blockIdx.x - t * B;
  const rac_image_job& job = jobs[b];  // workgroup-uniform
  FrameSrc src;
  src.Hs = job.Hs, src.Ws = job.Ws;
  src.h = h, src.w = w;
  const long raw = (long)src.Hs * src.Ws;
  src.rgb = frames + job.frame_offset + (long)t * raw * 3;
  src.mask = masks + job.mask_offset + (long)t * raw;
  src.sy = __fdiv_rn((float)src.Hs, (float)h), src.sx = __fdiv_rn((float)src.Ws, (float)w);
  src.same = src.Hs == h && src.Ws == w;
  Crop crop;
  crop.top = job.top, crop.left = job.left, crop.th = job.th, crop.tw = job.tw;
  crop.sy = __fdiv_rn((float)crop.th, (float)h), crop.sx = __fdiv_rn((float)crop.tw, (float)w);
  crop.on = crop.th != h || crop.tw != w;
  Jitter jit;
  jit.order = 0;
  int contrast_at = 4;  // the steps before the contrast step are all pass 0 runs
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = job.order[k] & 3;
    jit.order |= op << (2 * k);
    if (op == 1 && contrast_at == 4) contrast_at = k;
  }
  jit.bf = (float)job.factor[0];
  jit.cf = (float)job.factor[1], jit.cf1 = (float)(1.0 - job.factor[1]);
  jit.sf = (float)job.factor[2], jit.sf1 = (float)(1.0 - job.factor[2]);
  jit.hf = (float)job.factor[3];
  const bool jitter = job.jitter != 0;

  const int HW = h * w, quads = HW >> 2;
  float* img = images + (long)blockIdx.x * 3 * HW;
  float* msk = out_masks + (long)blockIdx.x * HW;
  float mean = 0.f;
#pragma unroll 1
  for (int pass = jitter ? 0 : 1; pass < 2; ++pass) {
    const bool summing = pass == 0;
    float gsum = 0.f;
    for (int q = threadIdx.x; q < quads; q += 256) {
      const int p = q << 2;
      const int y = p / w, x = p - y * w;
      f32x4 o[3], om;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float px[3];
        geometry_rgb(src, crop, y, x + e, px);
        if (jitter) jitter_pixel(px, jit, summing ? contrast_at : 4, mean);
        if (summing) {
          gsum = __fadd_rn(gsum, gray_of(px));
        } else {
          o[0][e] = px[0], o[1][e] = px[1], o[2][e] = px[2];
          om[e] = geometry_mask(src, crop, y, x + e);
        }
      }
      if (!summing) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(img + (long)c * HW + p) = o[c];
        *reinterpret_cast<f32x4*>(msk + p) = om;
      }
    }
    if (summing) {  // (workgroup-uniform)
      gsum = wave_sum(gsum);
      if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = gsum;
      __syncthreads();
      mean = __fdiv_rn(((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3], (float)HW);
    }
  }
}

}  // namespace rac

using namespace rac;

extern "C" {

int rac_image_job_bytes(void) { return (int)sizeof(rac_image_job); }

int rac_image_pipeline(const uint8_t* frames, const uint8_t* masks, const rac_image_job* jobs, float* images,
                       float* out_masks, int32_t B, int32_t T, int32_t h, int32_t w, void* stream) {
  RAC_REQUIRE(frames && masks && jobs && images && out_masks && B > 0 && T > 0 && h > 0 && w > 0,
              "rac_image_pipeline: bad args");
  RAC_REQUIRE(w % 4 == 0, "rac_image_pipeline: the model width must be a multiple of 4 (float4 stores), got %d", w);
  RAC_REQUIRE(h <= 128 && w <= 128 && (long)B * T < (1L << 31), "rac_image_pipeline: model size at most 128 x 128");
  RAC_REQUIRE(aligned16(images) && aligned16(out_masks) && (reinterpret_cast<uintptr_t>(jobs) & 7u) == 0,
              "rac_image_pipeline: 16-byte aligned outputs, 8-byte aligned jobs");
  hipLaunchKernelGGL(image_pipeline_kernel, dim3((unsigned)(B * T)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     frames, masks, jobs, images, out_masks, B, h, w);
  return check_launch("rac_image_pipeline");
}

}  // extern "C"

RAC_DEVICE_CODE_END
