// animate.hip — rigs posed on the device: blend shapes, then linear-blend skinning, written straight into the resident
// gVertices (sthip_scene_animate, api.hip), so that a moving rig costs the host a few bone matrices and four factors per
// frame instead of every deformed vertex. The gather, the refit and the top level of refit.hip follow unchanged.
//
// The reference has the two passes as separate dispatches over the vertex buffer in place (src/Shaders/kernels/anim.hlsl:
// `blend` at :53-86, `skin` at :27-51; nothing upstream calls them). Here they are one pass from a rest pose that stays
// resident: a pose is then a function of the rest pose alone and not of the poses before it. Per vertex, with rest record r,
// in binary32, unfused (sthip_detmath.h), left to right:
//   blend (target_count > 0):  f = max(0, 1 - (((|b0| + |b1|) + |b2|) + |b3|));  p = f * r.position;  p = p + bk * Tk.position
//                              for k = 0 .. target_count - 1;  n the same from the normals, then n = normalize3(n).
//                              Without targets p and n are bit copies of the rest.
//   skin (bone_count > 0):     M = +0;  M = M + bones[indices[j]] * weights[j] for j = 0 .. 3, elementwise;
//                              p' = M * (p, 1), n' = (3x3 of M) * n, rows dotted left to right; no renormalisation (as upstream).
//   u and v are bit copies of the rest. Upstream's tangent has no field in PackedVertexData and is not carried.
//
// One lane per vertex, grid-stride; a record is two 16-byte loads and two 16-byte stores, so consecutive lanes coalesce.
// The block first copies the rig's bones into LDS (at most 1024 x 48 B = 48 KB), 16 bytes per lane and step, in a loop that
// serves any bone_count against the block size; lanes then fetch their four matrices from LDS by index (validated on the
// host when the rig was set). No atomics, no ordering between blocks: every lane writes only its own record.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "animate.h"
#include "device_math.h"

namespace sthip {
namespace {

constexpr unsigned ANIMATE_BLOCK = 256;

struct AnimateArgs {
  float4* vertices;
  const float4* rest;
  const float4* targets[ANIMATE_MAX_TARGETS];
  const sthip_VertexWeight* weights;
  const float4* bones;
  uint32_t vertex_count, target_count, bone_count;
  float factors[ANIMATE_MAX_TARGETS];
};

__global__ void __launch_bounds__(ANIMATE_BLOCK) k_animate(const AnimateArgs a) {
  extern __shared__ float4 s_bones[];  // 3 rows per bone
  for (uint32_t k = threadIdx.x; k < 3u * a.bone_count; k += ANIMATE_BLOCK) s_bones[k] = a.bones[k];
  __syncthreads();
  const float b0 = a.factors[0], b1 = a.factors[1], b2 = a.factors[2], b3 = a.factors[3];
  const float f = fmaxf(0.0f, 1.0f - (((fabsf(b0) + fabsf(b1)) + fabsf(b2)) + fabsf(b3)));
  for (uint32_t i = blockIdx.x * ANIMATE_BLOCK + threadIdx.x; i < a.vertex_count; i += gridDim.x * ANIMATE_BLOCK) {
    const float4 r0 = a.rest[2 * (size_t)i], r1 = a.rest[2 * (size_t)i + 1];  // (position, u), (normal, v)
    f3 p = xyz(r0), n = xyz(r1);
    if (a.target_count) {
      p = f * p;
      n = f * n;
#pragma unroll
      for (uint32_t k = 0; k < ANIMATE_MAX_TARGETS; k++) {
        if (k >= a.target_count) break;
        const float4 t0 = a.targets[k][2 * (size_t)i], t1 = a.targets[k][2 * (size_t)i + 1];
        const float b = a.factors[k];
        p = p + b * xyz(t0);
        n = n + b * xyz(t1);
      }
      n = normalize3(n);
    }
    if (a.bone_count) {
      const uint4* wp = reinterpret_cast<const uint4*>(a.weights + i);
      const uint4 wbits = wp[0], idx = wp[1];
      const float w[4] = {__uint_as_float(wbits.x), __uint_as_float(wbits.y), __uint_as_float(wbits.z), __uint_as_float(wbits.w)};
      const uint32_t bone[4] = {idx.x, idx.y, idx.z, idx.w};
      float m[12];
      for (int e = 0; e < 12; e++) m[e] = 0.0f;
      for (int j = 0; j < 4; j++) {
        const float4 q0 = s_bones[3u * bone[j]], q1 = s_bones[3u * bone[j] + 1u], q2 = s_bones[3u * bone[j] + 2u];
        const float q[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        for (int e = 0; e < 12; e++) m[e] = m[e] + q[e] * w[j];
      }
      Xf M;
      M.r0 = make_float4(m[0], m[1], m[2], m[3]);
      M.r1 = make_float4(m[4], m[5], m[6], m[7]);
      M.r2 = make_float4(m[8], m[9], m[10], m[11]);
      p = xf_point(M, p);
      n = xf_vector(M, n);
    }
    a.vertices[2 * (size_t)i] = make_float4(p.x, p.y, p.z, r0.w);
    a.vertices[2 * (size_t)i + 1] = make_float4(n.x, n.y, n.z, r1.w);
  }
}

}  // namespace

bool animate_launch(const AnimateRig& rig, int cu_count, void* stream, std::string& err) {
  static_assert(sizeof(sthip_PackedVertexData) == 32 && sizeof(sthip_VertexWeight) == 32 && sizeof(sthip_TransformData) == 48, "two, two and three 16-byte words");
  if (!rig.vertex_count) return true;
  if (rig.target_count > ANIMATE_MAX_TARGETS || rig.bone_count > ANIMATE_MAX_BONES) {
    err = "animate: more targets or bones than the kernel serves";
    return false;
  }
  AnimateArgs a{};
  a.vertices = reinterpret_cast<float4*>(rig.vertices);
  a.rest = reinterpret_cast<const float4*>(rig.rest);
  for (uint32_t k = 0; k < ANIMATE_MAX_TARGETS; k++) {
    a.targets[k] = k < rig.target_count ? reinterpret_cast<const float4*>(rig.targets[k]) : nullptr;
    a.factors[k] = k < rig.target_count ? rig.factors[k] : 0.0f;
  }
  a.weights = rig.weights;
  a.bones = reinterpret_cast<const float4*>(rig.bones);
  a.vertex_count = rig.vertex_count;
  a.target_count = rig.target_count;
  a.bone_count = rig.bone_count;
  // every block fills its own copy of the bones: few enough blocks that the fill stays small beside the records (grid-stride)
  const uint32_t blocks = (rig.vertex_count + ANIMATE_BLOCK - 1) / ANIMATE_BLOCK;
  const uint32_t grid = std::max(1u, std::min(blocks, (uint32_t)std::max(1, cu_count) * 4u));
  hipLaunchKernelGGL(k_animate, dim3(grid), dim3(ANIMATE_BLOCK), (size_t)rig.bone_count * sizeof(sthip_TransformData), (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("k_animate: ") + hipGetErrorString(e);
    return false;
  }
  return true;
}

}  // namespace sthip
