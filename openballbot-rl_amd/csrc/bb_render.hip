// bb_render.hip -- robot-mounted depth cameras.
//
// The reference renders cam_0 / cam_1 (ballbot.xml:44-54, fovy 90, 64x64,
// depth only) through MuJoCo's OpenGL renderer every ceil((1/90 s)/2 ms) = 6
// physics steps (ballbot_env.py:389-411, 743-767) and clips depth at 1 m
// (sensors/rgbd.py:46-82).  Here every (env, camera) is one workgroup that
// ray-casts its image: the linear eye-space depth of the nearest front face
// among the hfield surface, the ball, the tower cylinder, the cam sticks and
// the wheel capsules, clipped to 1.  The geometry and conventions are those of
// oracle/bb_oracle.c:bbo_render_depth (fp64), the checker of this kernel.  The
// primitives and the ray tests live in bb_raycast.h, shared with bb_view.hip.
//
// Work: scene_kernel (one thread per env) runs the fixed-tree kinematics
// (bb_physics.h) and writes both cameras' frames and the 7 primitives (220 B
// per camera); depth_kernel stages one scene in LDS and its 256 threads cast
// H*W rays (16 each at 64x64).  Rays stop at z-depth 1 m, so the hfield
// DDA visits at most ~100 cells (cell 34 mm, ray <= sqrt(3) m); a typical ray
// hits the ground within ~10.  Only envs whose step counter is a multiple of
// the frame interval render (the others keep their last image), so on average
// 1/6 of the workgroups do work.  Output: depth f32[n][2][H][W] (obs rgbd_0 =
// [:, 0:1], rgbd_1 = [:, 1:2]) and relative_image_timestamp f32[n].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_raycast.h"
#include "bb_render.h"

namespace bb {
namespace {

struct Scene {
  float o[3], R[9];     // camera origin, camera->world rotation (columns: x right, y up, z back)
  float ball[3];
  float pa[6][3], pb[6][3];  // 0 tower (cylinder), 1-2 sticks, 3-5 wheels (capsules)
  float rad[6];
  float size_z;
  float ztop;  // max terrain height (hmax * size_z): rays above it skip the march
  int tid;
};

// one thread per env: camera frames and primitives of both cameras -> scenes[e][cam]
template <typename T>
__global__ __launch_bounds__(64) void scene_kernel(ModelT<float> m, CamRig rig, RenderDev d, int every, int force,
                                                   double dt, Scene* __restrict__ scenes, float* __restrict__ rel_ts) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.n) return;
  const int k6 = d.steps[e] % every;
  if (rel_ts) rel_ts[e] = float(double(k6) * dt);  // the reference subtracts two double times, then casts
  if (!force && k6 != 0) return;
  const T* Q = (const T*)d.qpos;
  float q[NQ];
#pragma unroll
  for (int i = 0; i < NQ; i++) q[i] = float(Q[size_t(i) * d.n + e]);
  Kin<float> k;
  kinematics(m, q, k);
  Scene S;
  BB_SCENE_PRIMITIVES(m, k, S);
  S.tid = d.terrain[e];
  S.size_z = d.size_z[S.tid];
  S.ztop = d.hmax[S.tid] * S.size_z;
  for (int cam = 0; cam < 2; cam++) {
    to_world(k, rig.p[cam], S.o);
    mm3(S.R, k.Rb, rig.R[cam]);
    scenes[2 * e + cam] = S;
  }
}

// one workgroup per (env, camera): H*W rays against the scene
__global__ __launch_bounds__(256) void depth_kernel(ModelT<float> m, RenderDev d, const Scene* __restrict__ scenes,
                                                    int H, int W, int every, int force, float* __restrict__ depth) {
  const int e = blockIdx.x >> 1, cam = blockIdx.x & 1;
  if (e >= d.n) return;
  if (!force && d.steps[e] % every != 0) return;
  __shared__ Scene S;
  constexpr int NW = sizeof(Scene) / sizeof(float);
  static_assert(sizeof(Scene) % sizeof(float) == 0, "Scene is copied as floats");
  if (threadIdx.x < NW)
    reinterpret_cast<float*>(&S)[threadIdx.x] = reinterpret_cast<const float*>(scenes + 2 * e + cam)[threadIdx.x];
  __syncthreads();
  const float* hf = d.bank + size_t(S.tid) * (HF_N * HF_N);
  float* out = depth + (size_t(e) * 2 + cam) * H * W;
  const float aspect = float(W) / float(H);
  for (int px = threadIdx.x; px < H * W; px += blockDim.x) {
    const int i = px / W, j = px - i * W;
    const float xc = (2.f * (j + 0.5f) / W - 1.f) * aspect, yc = 1.f - 2.f * (i + 0.5f) / H;  // tan(fovy/2) = 1
    float dr[3] = {S.R[0] * xc + S.R[1] * yc - S.R[2], S.R[3] * xc + S.R[4] * yc - S.R[5],
                   S.R[6] * xc + S.R[7] * yc - S.R[8]};
    const float len = sqrtf(dot3(dr, dr)), il = 1.f / len;
    dr[0] *= il; dr[1] *= il; dr[2] *= il;
    const float tmin = ZNEAR * len;
    float best = len;  // z-depth 1
    const float tb = ray_sphere(S.o, dr, S.ball, m.ball_r);
    if (tb > tmin && tb < best) best = tb;
    {
      const float t = ray_cylinder(S.o, dr, S.pa[0], S.pb[0], S.rad[0]);
      if (t > tmin && t < best) best = t;
    }
#pragma unroll 1
    for (int g = 1; g < 6; g++) {
      const float t = ray_capsule(S.o, dr, S.pa[g], S.pb[g], S.rad[g]);
      if (t > tmin && t < best) best = t;
    }
    const float tg = ray_hfield(S.o, dr, hf, S.size_z, S.ztop, m.hf_sx, m.hf_sy, tmin, best);
    if (tg > tmin && tg < best) best = tg;
    out[px] = fminf(best * il, 1.f);
  }
}

}  // namespace

size_t scene_bytes(int n) { return sizeof(Scene) * 2 * size_t(n); }

int launch_depth(bool fp64, const ModelT<float>& m, const CamRig& rig, const RenderDev& d, int H, int W, int every,
                 int force, double dt, void* scenes, float* depth, float* rel_ts, hipStream_t s) {
  if (d.n <= 0) return 0;
  Scene* sc = (Scene*)scenes;
  if (fp64)
    hipLaunchKernelGGL(scene_kernel<double>, dim3((d.n + 63) / 64), dim3(64), 0, s, m, rig, d, every, force, dt, sc,
                       rel_ts);
  else
    hipLaunchKernelGGL(scene_kernel<float>, dim3((d.n + 63) / 64), dim3(64), 0, s, m, rig, d, every, force, dt, sc,
                       rel_ts);
  hipLaunchKernelGGL(depth_kernel, dim3(2 * d.n), dim3(256), 0, s, m, d, sc, H, W, every, force, depth);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bb
