// bb_rgbd.hip -- robot-mounted RGB-D cameras: the observation for camera.disable_rgb: false.
//
// The reference renders cam_0 / cam_1 as RGB in [0, 1] plus depth clipped at 1 m
// (sensors/rgbd.py:46-82, a (4, H, W) frame) through MuJoCo's OpenGL renderer.  MuJoCo's colour
// image cannot be pinned here, so the colour is this project's own definition, the
// one bb_view.hip applies from the free camera: flat base colours, a 0.5 m ground checker, a
// two-tone ball and one shading rule, here seen along the depth cameras' rays (bb_render.hip) and
// stored as float32(int(255 c + 0.5)) / 255, the reference's render().astype(float32) / 255.
// Colour rays run to zfar (14.142 m); the D plane is min(t / len, 1), the depth camera's quantity.
// tests/rgbd_ref.py is the fp64 reference.
//
// Work: rgbd_scene_kernel (one thread per env) runs the fixed-tree kinematics and writes both
// cameras' frames, the primitives and the ball's rotation; rgbd_kernel gives one wave to each 8x8
// pixel tile of one (env, camera) image (four tiles per workgroup), so a wave's rays walk
// neighbouring cells of the field, and does work only for envs whose frame is due.  A tile's four
// planes are gathered in LDS and leave as 16-byte row halves where the address allows it.
//
// The colour and normal code restates bb_view.hip's: bb_render.hip, bb_view.hip and bb_raycast.h
// stay as they are, because sharing by refactoring would change the depth images' last bits
// (bb_raycast.h, BB_SCENE_PRIMITIVES).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_raycast.h"
#include "bb_rgbd.h"

namespace bb {
namespace {

constexpr float ZFAR = 14.142135623730951f;  // ballbot.xml:8 zfar * extent
constexpr int TILE = 8, WAVES = 4;           // pixels per tile side; tiles (waves) per workgroup

struct RgbdScene {
  float o[3], R[9];     // camera origin, camera->world rotation (columns: x right, y up, z back)
  float ball[3];
  float pa[6][3], pb[6][3];  // 0 tower (cylinder), 1-2 sticks, 3-5 wheels (capsules)
  float rad[6];
  float RB[9];          // ball body -> world
  float size_z;
  float ztop;           // max terrain height (hmax * size_z)
  int tid;
};

// one thread per env: camera frames, primitives and the ball's rotation -> scenes[e][cam]
template <typename T>
__global__ __launch_bounds__(64) void rgbd_scene_kernel(ModelT<float> m, CamRig rig, RenderDev d, int every, int force,
                                                        double dt, RgbdScene* __restrict__ scenes,
                                                        float* __restrict__ rel_ts) {
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
  RgbdScene S;
  BB_SCENE_PRIMITIVES(m, k, S);
#pragma unroll
  for (int i = 0; i < 9; i++) S.RB[i] = k.RB[i];
  S.tid = d.terrain[e];
  S.size_z = d.size_z[S.tid];
  S.ztop = d.hmax[S.tid] * S.size_z;
  for (int cam = 0; cam < 2; cam++) {
    to_world(k, rig.p[cam], S.o);
    mm3(S.R, k.Rb, rig.R[cam]);
    scenes[2 * e + cam] = S;
  }
}

__device__ __forceinline__ void unit3(float* n) {
  const float il = 1.f / sqrtf(dot3(n, n));
  n[0] *= il; n[1] *= il; n[2] *= il;
}

// a colour count 0..255 as the reference stores it: float32(q) / 255, correctly rounded
__device__ __forceinline__ float count_to_float(int q) { return __fdiv_rn(float(q), 255.f); }

// one wave per 8x8 tile of one (env, camera) image
__global__ __launch_bounds__(64 * WAVES) void rgbd_kernel(ModelT<float> m, RenderDev d,
                                                          const RgbdScene* __restrict__ scenes, int H, int W,
                                                          int every, int force, float* __restrict__ rgbd,
                                                          int8_t* __restrict__ ids) {
  const int tx = (W + TILE - 1) / TILE, ty = (H + TILE - 1) / TILE, ntiles = tx * ty;
  const int groups = (ntiles + WAVES - 1) / WAVES;  // workgroups per image
  const int v = blockIdx.x / groups, g = blockIdx.x - v * groups;  // v = 2 e + cam
  const int e = v >> 1;
  if (e >= d.n) return;
  if (!force && d.steps[e] % every != 0) return;  // the whole workgroup: no barrier is passed by a part of it
  __shared__ RgbdScene S;
  __shared__ float sh_px[WAVES][4][TILE * TILE];
  constexpr int NW = sizeof(RgbdScene) / sizeof(float);
  static_assert(sizeof(RgbdScene) % sizeof(float) == 0 && NW <= 64 * WAVES, "RgbdScene is copied as floats");
  if (threadIdx.x < NW)
    reinterpret_cast<float*>(&S)[threadIdx.x] = reinterpret_cast<const float*>(scenes + v)[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = g * WAVES + wave;
  const int ti = tile / tx, tj = tile - ti * tx;
  const int row = lane >> 3, col = lane & 7;
  const int i = ti * TILE + row, j = tj * TILE + col;
  float px[4] = {count_to_float(int(255.f * 0.55f + 0.5f)), count_to_float(int(255.f * 0.70f + 0.5f)),
                 count_to_float(int(255.f * 0.90f + 0.5f)), 1.f};  // background, unshaded; depth 1
  const bool live = tile < ntiles && i < H && j < W;
  if (live) {
    int id = 0;
    const float* hf = d.bank + size_t(S.tid) * (HF_N * HF_N);
    const float aspect = float(W) / float(H);
    const float xc = (2.f * (j + 0.5f) / W - 1.f) * aspect, yc = 1.f - 2.f * (i + 0.5f) / H;  // tan(fovy/2) = 1
    float dr[3] = {S.R[0] * xc + S.R[1] * yc - S.R[2], S.R[3] * xc + S.R[4] * yc - S.R[5],
                   S.R[6] * xc + S.R[7] * yc - S.R[8]};
    const float len = sqrtf(dot3(dr, dr)), il = 1.f / len;
    dr[0] *= il; dr[1] *= il; dr[2] *= il;
    const float tmin = ZNEAR * len;
    float best = ZFAR * len;
    int part = 0, tri = 0;
    const float tb = ray_sphere(S.o, dr, S.ball, m.ball_r);
    if (tb > tmin && tb < best) { best = tb; id = 2; }
    {
      int p = 0;
      const float t = ray_cylinder_face<true>(S.o, dr, S.pa[0], S.pb[0], S.rad[0], &p);
      if (t > tmin && t < best) { best = t; id = 3; part = p; }
    }
#pragma unroll 1
    for (int k = 1; k < 6; k++) {
      const float t = ray_capsule(S.o, dr, S.pa[k], S.pb[k], S.rad[k]);
      if (t > tmin && t < best) { best = t; id = 3 + k; }
    }
    const float tg = ray_hfield_tri<true>(S.o, dr, hf, S.size_z, S.ztop, m.hf_sx, m.hf_sy, tmin, best, &tri);
    if (tg > tmin && tg < best) { best = tg; id = 1; }
    if (id != 0) {
      const float p[3] = {S.o[0] + best * dr[0], S.o[1] + best * dr[1], S.o[2] + best * dr[2]};
      float n[3], base[3];
      if (id == 1) {  // the hit triangle's plane, turned to face the ray; world-xy checker of 0.5 m squares
        const int cell = tri >> 1, r = cell / HF_N, c = cell - r * HF_N;
        const float dx = 2.f * m.hf_sx / (HF_N - 1), dy = 2.f * m.hf_sy / (HF_N - 1);
        const float zA = hf[r * HF_N + c] * S.size_z, zB = hf[(r + 1) * HF_N + c] * S.size_z;
        const float zC = hf[r * HF_N + c + 1] * S.size_z, zD = hf[(r + 1) * HF_N + c + 1] * S.size_z;
        const float gx = ((tri & 1) ? zD - zB : zC - zA) / dx, gy = ((tri & 1) ? zD - zC : zB - zA) / dy;
        n[0] = -gx; n[1] = -gy; n[2] = 1.f;
        unit3(n);
        if (dot3(n, dr) > 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        const bool odd = (int(floorf(p[0] * 2.f)) + int(floorf(p[1] * 2.f))) & 1;
        base[0] = odd ? 0.30f : 0.42f; base[1] = odd ? 0.33f : 0.45f; base[2] = odd ? 0.36f : 0.48f;
      } else if (id == 2) {  // two-tone by the octant of the normal in the ball's own frame
        n[0] = p[0] - S.ball[0]; n[1] = p[1] - S.ball[1]; n[2] = p[2] - S.ball[2];
        unit3(n);
        const float nb[3] = {S.RB[0] * n[0] + S.RB[3] * n[1] + S.RB[6] * n[2],
                             S.RB[1] * n[0] + S.RB[4] * n[1] + S.RB[7] * n[2],
                             S.RB[2] * n[0] + S.RB[5] * n[1] + S.RB[8] * n[2]};
        const bool lit = nb[0] * nb[1] * nb[2] >= 0.f;
        base[0] = lit ? 0.90f : 0.20f; base[1] = lit ? 0.45f : 0.12f; base[2] = lit ? 0.10f : 0.08f;
      } else {
        const int k = id - 3;
        const float* pa = S.pa[k];
        const float ba[3] = {S.pb[k][0] - pa[0], S.pb[k][1] - pa[1], S.pb[k][2] - pa[2]};
        const float ap[3] = {p[0] - pa[0], p[1] - pa[1], p[2] - pa[2]};
        if (k == 0 && part != 0) {  // a disc of the tower
          const float sg = float(part);
          n[0] = sg * ba[0]; n[1] = sg * ba[1]; n[2] = sg * ba[2];
        } else {  // away from the nearest point of the segment (capsule caps included)
          float h = dot3(ap, ba) / dot3(ba, ba);
          if (k != 0) h = fminf(fmaxf(h, 0.f), 1.f);
          n[0] = ap[0] - h * ba[0]; n[1] = ap[1] - h * ba[1]; n[2] = ap[2] - h * ba[2];
        }
        unit3(n);
        if (k < 3) { base[0] = 0.18f; base[1] = 0.80f; base[2] = 0.44f; }
        else { base[0] = k == 3 ? 1.f : 0.f; base[1] = k == 4 ? 1.f : 0.f; base[2] = k == 5 ? 1.f : 0.f; }
      }
      // c = base (0.25 + 0.45 max(0, n_z) + 0.30 max(0, -n.d)) -> int(255 c + 0.5) / 255
      const float s = 0.25f + 0.45f * fmaxf(0.f, n[2]) + 0.30f * fmaxf(0.f, -dot3(n, dr));
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = count_to_float(int(255.f * (base[k] * s) + 0.5f));
      px[3] = fminf(best * il, 1.f);
    }
    if (ids) ids[(size_t(v) * H + i) * W + j] = int8_t(id);  // a tile row's lanes: consecutive bytes
  }
#pragma unroll
  for (int k = 0; k < 4; k++) sh_px[wave][k][lane] = px[k];
  __syncthreads();
  // 64 lanes = 4 planes x 8 rows x 2 halves of a row: four floats each, as one 16-byte store when
  // the half lies inside the image and its address is aligned (17x23 planes are not), else one by one
  const int pl = lane >> 4, r2 = (lane >> 1) & 7, c0 = (lane & 1) * 4;
  const int i2 = ti * TILE + r2, cols = min(TILE, W - tj * TILE);
  if (tile < ntiles && i2 < H && c0 < cols) {
    float* dst = rgbd + ((size_t(v) * 4 + pl) * H + i2) * W + size_t(tj) * TILE + c0;
    const float* src = &sh_px[wave][pl][r2 * TILE + c0];
    const int cnt = min(4, cols - c0);
    if (cnt == 4 && (uintptr_t(dst) & 15u) == 0) {
      *reinterpret_cast<float4*>(dst) = make_float4(src[0], src[1], src[2], src[3]);
    } else {
      for (int k = 0; k < cnt; k++) dst[k] = src[k];
    }
  }
}

}  // namespace

size_t rgbd_scene_bytes(int n) { return sizeof(RgbdScene) * 2 * size_t(n); }

int launch_rgbd(bool fp64, const ModelT<float>& m, const CamRig& rig, const RenderDev& d, int H, int W, int every,
                int force, double dt, void* scenes, float* rgbd, float* rel_ts, int8_t* ids, hipStream_t s) {
  if (d.n <= 0) return 0;
  RgbdScene* sc = (RgbdScene*)scenes;
  const int64_t ntiles = int64_t((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
  const int64_t blocks = (ntiles + WAVES - 1) / WAVES * 2 * d.n;
  if (blocks > 0x7fffffff) return -1;
  if (fp64)
    hipLaunchKernelGGL(rgbd_scene_kernel<double>, dim3((d.n + 63) / 64), dim3(64), 0, s, m, rig, d, every, force, dt,
                       sc, rel_ts);
  else
    hipLaunchKernelGGL(rgbd_scene_kernel<float>, dim3((d.n + 63) / 64), dim3(64), 0, s, m, rig, d, every, force, dt, sc,
                       rel_ts);
  hipLaunchKernelGGL(rgbd_kernel, dim3((unsigned)blocks), dim3(64 * WAVES), 0, s, m, d, sc, H, W, every, force, rgbd,
                     ids);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bb
