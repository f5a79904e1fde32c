// Robot masks from joint positions in one launch: forward kinematics of a link tree + triangle rasterisation with a depth
// test, one workgroup per pose (the reference's MuJoCo mask environments, src/env/robotics/masks/base_mask_env.py:
// set the named joints, mj_forward, render a segmentation image from one fixed camera, mark the robot geoms' pixels).
// The semantics are those of include/rac_hip.h (rac_render_masks) and DESIGN.md 18.
#include "rac_common.h"

extern "C" int rac_render_link_bytes(void) { return (int)sizeof(rac_render_link); }

namespace rac {

constexpr int RD_THREADS = 256;
constexpr float RD_ZNEAR = 0.01f;
constexpr unsigned RD_FAR = 0x7F800000u;  // +inf: "nothing hit"; positive floats order as their bit patterns

struct RenderCam {
  float local[12];  // camera-to-link, MuJoCo's camera frame (looks along -z, +x right, +y up)
  int link;
  float focal;      // 0.5 H / tan(fovy / 2), pixels
};

// C = A B for affine 3x4 matrices (row-major, the fourth row 0 0 0 1 implied)
__device__ __forceinline__ void affine_mul(const float* A, const float* B, float* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c];
      C[4 * r + c] = (c == 3) ? v + A[4 * r + 3] : v;
    }
  }
}

// The joint's transform J of a link at joint position q: hinge T(anchor) R(axis, q) T(-anchor), slide T(axis q).
__device__ __forceinline__ void joint_transform(const rac_render_link& k, float q, float* Jm) {
  const float ax = k.axis[0], ay = k.axis[1], az = k.axis[2];
  if (k.joint == 1) {
    float s, c;
    sincosf(q, &s, &c);
    const float t = 1.f - c;
    Jm[0] = c + t * ax * ax, Jm[1] = t * ax * ay - s * az, Jm[2] = t * ax * az + s * ay;
    Jm[4] = t * ax * ay + s * az, Jm[5] = c + t * ay * ay, Jm[6] = t * ay * az - s * ax;
    Jm[8] = t * ax * az - s * ay, Jm[9] = t * ay * az + s * ax, Jm[10] = c + t * az * az;
    const float px = k.anchor[0], py = k.anchor[1], pz = k.anchor[2];
    Jm[3] = px - (Jm[0] * px + Jm[1] * py + Jm[2] * pz);
    Jm[7] = py - (Jm[4] * px + Jm[5] * py + Jm[6] * pz);
    Jm[11] = pz - (Jm[8] * px + Jm[9] * py + Jm[10] * pz);
  } else {
    Jm[0] = 1.f, Jm[1] = 0.f, Jm[2] = 0.f, Jm[4] = 0.f, Jm[5] = 1.f, Jm[6] = 0.f, Jm[8] = 0.f, Jm[9] = 0.f, Jm[10] = 1.f;
    const float d = (k.joint == 2) ? q : 0.f;
    Jm[3] = ax * d, Jm[7] = ay * d, Jm[11] = az * d;
  }
}

__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// One source index and its two tap weights of torch's bilinear resize (align_corners=False, no antialias) in fp32:
// src = max(0, in / out (o + 0.5) - 0.5), products and sums rounded separately.
__device__ __forceinline__ void resize_taps(int o, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  float src = __fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = __fsub_rn(src, (float)i0);
  l0 = __fsub_rn(1.f, l1);
}

// grid P, 256 threads: workgroup p renders pose p and writes nothing else.
//   1. links in table order (parents first): threads 0..11 of the first wave compute one element each of
//      X_link = X_parent (local J) into LDS, a workgroup barrier between a link and its children;
//   2. thread l < L turns link l's matrix into link-to-camera;
//   3. all threads stride over the shared triangle table (structure of arrays, coalesced), transform, project and walk
//      the clamped bounding box: an LDS integer atomic min on the depth's bits, one buffer for the robot and -- only for a
//      model with other geoms -- one for the rest;
//   4. robot = (robot depth is finite and <= other depth), then the resize rule, coalesced stores.
// No global atomic, no float atomic: a pose's bits depend on its own qpos row alone.
__global__ void __launch_bounds__(RD_THREADS) render_masks_kernel(
    const float* qpos, long qpos_stride, int J, const rac_render_link* links, int L, const float* tri, long tri_stride,
    const int* tri_meta, int N, int two, RenderCam cam, int H, int W, int h, int w, float* masks, float* native,
    float* link_xpos) {
  __shared__ float xw[RAC_RENDER_MAX_LINKS * 12];  // link-to-world
  __shared__ float xc[RAC_RENDER_MAX_LINKS * 12];  // link-to-camera
  extern __shared__ __attribute__((aligned(16))) unsigned depth[];  // [two ? 2 : 1][H W]
  const int tid = threadIdx.x, HW = H * W;
  const long p = blockIdx.x;
  const float* q = qpos + p * qpos_stride;

  for (int i = tid; i < (two ? 2 * HW : HW); i += RD_THREADS) depth[i] = RD_FAR;
  for (int l = 0; l < L; ++l) {
    if (tid < 12) {
      const rac_render_link k = links[l];
      float Jm[12], M[12];
      joint_transform(k, (k.qcol >= 0 && k.qcol < J) ? q[k.qcol] : 0.f, Jm);
      affine_mul(k.local, Jm, M);
      const int r = tid >> 2, c = tid & 3;
      const float m0 = c == 0 ? M[0] : c == 1 ? M[1] : c == 2 ? M[2] : M[3];
      const float m1 = c == 0 ? M[4] : c == 1 ? M[5] : c == 2 ? M[6] : M[7];
      const float m2 = c == 0 ? M[8] : c == 1 ? M[9] : c == 2 ? M[10] : M[11];
      float v;
      if (k.parent >= 0) {
        const float* Xp = xw + min(k.parent, L - 1) * 12 + 4 * r;
        v = Xp[0] * m0 + Xp[1] * m1 + Xp[2] * m2;
        if (c == 3) v += Xp[3];
      } else {
        v = r == 0 ? m0 : r == 1 ? m1 : m2;
      }
      xw[l * 12 + tid] = v;
    }
    __syncthreads();
  }
  if (tid < L) {
    float C[12], inv[12], out[12];
    affine_mul(xw + cam.link * 12, cam.local, C);  // camera-to-world
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      inv[4 * r] = C[r], inv[4 * r + 1] = C[4 + r], inv[4 * r + 2] = C[8 + r];
      inv[4 * r + 3] = -(C[r] * C[3] + C[4 + r] * C[7] + C[8 + r] * C[11]);
    }
    affine_mul(inv, xw + tid * 12, out);
#pragma unroll
    for (int e = 0; e < 12; ++e) xc[tid * 12 + e] = out[e];
    if (link_xpos) {
      float* o = link_xpos + (p * L + tid) * 3;
      o[0] = xw[tid * 12 + 3], o[1] = xw[tid * 12 + 7], o[2] = xw[tid * 12 + 11];
    }
  }
  __syncthreads();

  // MuJoCo's image of the camera (u = W/2 + f x/d, v = H/2 - f y/d, d = -z) read bottom-up and with its columns
  // reversed, as the reference environment hands it out: u' = W - u, v' = H - v.
  const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
  for (int t = tid; t < N; t += RD_THREADS) {
    const int meta = tri_meta[t];
    const int robot = (meta >> 8) & 1;
    if (!robot && !two) continue;
    const float* M = xc + min(meta & 0xFF, L - 1) * 12;
    float px[3], py[3], iz[3];
    bool ok = true;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const float x = tri[(3 * v) * tri_stride + t], y = tri[(3 * v + 1) * tri_stride + t],
                  z = tri[(3 * v + 2) * tri_stride + t];
      const float vx = M[0] * x + M[1] * y + M[2] * z + M[3];
      const float vy = M[4] * x + M[5] * y + M[6] * z + M[7];
      const float d = -(M[8] * x + M[9] * y + M[10] * z + M[11]);
      ok = ok && (d >= RD_ZNEAR);
      const float id = 1.f / d;
      px[v] = cx - cam.focal * vx * id;
      py[v] = cy + cam.focal * vy * id;
      iz[v] = id;
    }
    if (!ok) continue;  // a vertex nearer than znear (or not a number): the triangle is dropped whole
    const float area = edge_fn(px[0], py[0], px[1], py[1], px[2], py[2]);
    if (!(fabsf(area) > 0.f)) continue;
    const float sgn = area > 0.f ? 1.f : -1.f, inv_area = 1.f / area;
    const float xmin = fminf(px[0], fminf(px[1], px[2])), xmax = fmaxf(px[0], fmaxf(px[1], px[2]));
    const float ymin = fminf(py[0], fminf(py[1], py[2])), ymax = fmaxf(py[0], fmaxf(py[1], py[2]));
    // pixel centres c + 0.5 inside [xmin, xmax], clamped to the image in float before the cast
    const int c0 = (int)ceilf(fmaxf(xmin - 0.5f, 0.f)), c1 = (int)floorf(fminf(xmax - 0.5f, (float)(W - 1)));
    const int r0 = (int)ceilf(fmaxf(ymin - 0.5f, 0.f)), r1 = (int)floorf(fminf(ymax - 0.5f, (float)(H - 1)));
    unsigned* buf = depth + (robot ? 0 : HW);
    for (int r = r0; r <= r1; ++r) {
      const float sy = (float)r + 0.5f;
      for (int c = c0; c <= c1; ++c) {
        const float sx = (float)c + 0.5f;
        const float e0 = edge_fn(px[1], py[1], px[2], py[2], sx, sy), e1 = edge_fn(px[2], py[2], px[0], py[0], sx, sy),
                    e2 = edge_fn(px[0], py[0], px[1], py[1], sx, sy);
        if (e0 * sgn >= 0.f && e1 * sgn >= 0.f && e2 * sgn >= 0.f) {
          const float z = 1.f / ((e0 * iz[0] + e1 * iz[1] + e2 * iz[2]) * inv_area);
          if (z > 0.f) atomicMin(buf + r * W + c, __float_as_uint(z));
        }
      }
    }
  }
  __syncthreads();

  const bool same = (h == H && w == W);
  for (int i = tid; i < HW; i += RD_THREADS) {
    const unsigned dr = depth[i];
    const unsigned set = (dr != RD_FAR && (!two || dr <= depth[HW + i])) ? 1u : 0u;
    if (native) native[p * HW + i] = (float)set;
    if (same) masks[p * HW + i] = (float)set;
    else depth[i] = set;
  }
  if (same) return;
  __syncthreads();
  const float sh = (float)H / (float)h, sw = (float)W / (float)w;
  const int hw = h * w;
  for (int o = tid; o < hw; o += RD_THREADS) {
    const int oy = o / w, ox = o - oy * w;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    resize_taps(oy, sh, H, y0, y1, ly0, ly1);
    resize_taps(ox, sw, W, x0, x1, lx0, lx1);
    // a tap counts where its weight (the product of its row's and its column's) is not zero
    const unsigned a = (ly0 != 0.f && lx0 != 0.f) ? depth[y0 * W + x0] : 0u;
    const unsigned b = (ly0 != 0.f && lx1 != 0.f) ? depth[y0 * W + x1] : 0u;
    const unsigned c = (ly1 != 0.f && lx0 != 0.f) ? depth[y1 * W + x0] : 0u;
    const unsigned d = (ly1 != 0.f && lx1 != 0.f) ? depth[y1 * W + x1] : 0u;
    masks[p * hw + o] = (a | b | c | d) ? 1.f : 0.f;
  }
}

}  // namespace rac

extern "C" int rac_render_masks(const float* qpos, int64_t qpos_stride, int32_t P, int32_t J, const rac_render_link* links,
                                int32_t L, const float* tri, int64_t tri_stride, const int32_t* tri_meta, int32_t N,
                                int32_t other_geoms, const float* cam_local, int32_t cam_link, float fovy, int32_t H,
                                int32_t W, int32_t h, int32_t w, float* masks, float* native, float* link_xpos,
                                void* stream) {
  using namespace rac;
  RAC_REQUIRE(qpos && links && tri && tri_meta && cam_local && masks && P >= 1 && J >= 1 && N >= 1 &&
                  qpos_stride >= J && tri_stride >= N,
              "rac_render_masks: bad args");
  RAC_REQUIRE(L >= 1 && L <= RAC_RENDER_MAX_LINKS && cam_link >= 0 && cam_link < L,
              "rac_render_masks: 1 <= L <= %d links and a camera on one of them (L %d, camera link %d)",
              RAC_RENDER_MAX_LINKS, L, cam_link);
  RAC_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= RAC_RENDER_MAX_PIXELS,
              "rac_render_masks: the render size %d x %d is outside 1..%d pixels", H, W, RAC_RENDER_MAX_PIXELS);
  RAC_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "rac_render_masks: output size %d x %d outside 1..4096", h, w);
  RAC_REQUIRE(fovy > 0.f && fovy < 180.f, "rac_render_masks: fovy %g outside (0, 180) degrees", (double)fovy);
  RenderCam cam;
  for (int i = 0; i < 12; ++i) cam.local[i] = cam_local[i];
  cam.link = cam_link;
  cam.focal = (float)(0.5 * (double)H / tan(0.5 * (double)fovy * 3.14159265358979323846 / 180.0));
  const int two = other_geoms ? 1 : 0;
  const size_t lds = (size_t)(two ? 2 : 1) * H * W * sizeof(unsigned);
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(render_masks_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       2 * RAC_RENDER_MAX_PIXELS * (int)sizeof(unsigned));
    if (e != hipSuccess) {
      set_error("rac_render_masks: hipFuncSetAttribute: %s", hipGetErrorString(e));
      return RAC_ELAUNCH;
    }
    attr_done = true;
  }
  hipLaunchKernelGGL(render_masks_kernel, dim3(P), dim3(RD_THREADS), lds, reinterpret_cast<hipStream_t>(stream), qpos,
                     (long)qpos_stride, J, links, L, tri, (long)tri_stride, tri_meta, N, two, cam, H, W, h, w, masks, native,
                     link_xpos);
  return check_launch("rac_render_masks");
}

RAC_DEVICE_CODE_END
