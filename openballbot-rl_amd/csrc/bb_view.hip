// bb_view.hip -- world-view RGB renderer: env.render() and the trainer's videos.
//
// The reference's render() (ballbot_env.py:1077-1135) returns a third-person frame of MuJoCo's
// OpenGL renderer from a free camera that tracks the robot.  MuJoCo's image cannot be pinned here,
// so the image is this project's own definition: the depth cameras' surfaces
// (bb_raycast.h: heightfield, ball, tower, sticks, wheels) seen from MuJoCo's free camera, flat
// base colours and one shading rule, uint8 RGB.  tests/view_ref.py is its fp64 reference.
//
// Work: view_scene_kernel (one thread per view = an entry of env_ids) runs the fixed-tree
// kinematics and writes the primitives, the ball's rotation, the env's bank slot and the camera;
// view_kernel gives one wave to each 8x8 pixel tile of one view (four tiles per workgroup), so a
// wave's rays walk neighbouring cells of the field.  A tile's bytes are gathered in LDS and leave
// as aligned dwords; only the ends of a row that do not fill a dword go out as bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_raycast.h"
#include "bb_view.h"

namespace bb {
namespace {

constexpr float ZFAR = 14.142135623730951f;  // ballbot.xml:8 zfar * extent
constexpr int TILE = 8, WAVES = 4;           // pixels per tile side; tiles (waves) per workgroup

struct ViewScene {
  float o[3], R[9];     // camera origin, camera->world rotation (columns: x right, y up, z back)
  float ball[3];
  float pa[6][3], pb[6][3];  // 0 tower (cylinder), 1-2 sticks, 3-5 wheels (capsules)
  float rad[6];
  float RB[9];          // ball body -> world
  float size_z;
  float ztop;           // max terrain height (hmax * size_z)
  int tid;              // bank slot; -1: the view's env id is out of range (background only)
};

// one thread per view
template <typename T>
__global__ __launch_bounds__(64) void view_scene_kernel(ModelT<float> m, RenderDev d, ViewCam cam,
                                                        const int32_t* __restrict__ env_ids, int n_views,
                                                        ViewScene* __restrict__ scenes) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_views) return;
  const int e = env_ids[v];
  ViewScene S = {};
  if (e < 0 || e >= d.n) {
    S.tid = -1;
    scenes[v] = S;
    return;
  }
  const T* Q = (const T*)d.qpos;
  float q[NQ];
#pragma unroll
  for (int i = 0; i < NQ; i++) q[i] = float(Q[size_t(i) * d.n + e]);
  Kin<float> k;
  kinematics(m, q, k);
  BB_SCENE_PRIMITIVES(m, k, S);
#pragma unroll
  for (int i = 0; i < 9; i++) { S.RB[i] = k.RB[i]; S.R[i] = cam.R[i]; }
  S.tid = d.terrain[e];
  S.size_z = d.size_z[S.tid];
  S.ztop = d.hmax[S.tid] * S.size_z;
#pragma unroll
  for (int i = 0; i < 3; i++) S.o[i] = float(Q[size_t(i) * d.n + e] + T(cam.rel[i]));  // the camera tracks the base
  scenes[v] = S;
}

__device__ __forceinline__ void unit3(float* n) {
  const float il = 1.f / sqrtf(dot3(n, n));
  n[0] *= il; n[1] *= il; n[2] *= il;
}

// c = base (0.25 + 0.45 max(0, n_z) + 0.30 max(0, -n.d)) -> uint8 int(255 c + 0.5)
__device__ __forceinline__ void shade(const float* base, const float* n, const float* d, uint8_t* out) {
  const float s = 0.25f + 0.45f * fmaxf(0.f, n[2]) + 0.30f * fmaxf(0.f, -dot3(n, d));
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = uint8_t(int(255.f * (base[k] * s) + 0.5f));
}

// nbytes <= 24 bytes of src (LDS) -> dst + off, by the 8 lanes l of a tile row: lane l owns the
// l-th aligned dword under the row and writes it whole when the row covers it, else byte by byte
__device__ __forceinline__ void store_row(uint8_t* dst, size_t off, int nbytes, const uint8_t* src, int l) {
  const uintptr_t a = uintptr_t(dst + off);
  const uintptr_t w = (a & ~uintptr_t(3)) + 4u * unsigned(l);
  const int s = int(intptr_t(w) - intptr_t(a));  // index in src of the dword's first byte, >= -3
  if (s >= nbytes) return;
  if (s >= 0 && s + 4 <= nbytes) {
    *reinterpret_cast<uint32_t*>(w) = uint32_t(src[s]) | (uint32_t(src[s + 1]) << 8) | (uint32_t(src[s + 2]) << 16) |
                                      (uint32_t(src[s + 3]) << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (s + k >= 0 && s + k < nbytes) reinterpret_cast<uint8_t*>(w)[k] = src[s + k];
  }
}

// one wave per 8x8 tile of one view
__global__ __launch_bounds__(64 * WAVES) void view_kernel(ModelT<float> m, RenderDev d,
                                                          const ViewScene* __restrict__ scenes, int H, int W,
                                                          float tan_half, uint8_t* __restrict__ rgb,
                                                          int8_t* __restrict__ ids) {
  const int tx = (W + TILE - 1) / TILE, ty = (H + TILE - 1) / TILE, ntiles = tx * ty;
  const int groups = (ntiles + WAVES - 1) / WAVES;  // workgroups per view
  const int v = blockIdx.x / groups, g = blockIdx.x - v * groups;
  __shared__ ViewScene S;
  __shared__ uint8_t sh_rgb[WAVES][TILE * TILE * 3];
  __shared__ uint8_t sh_id[WAVES][TILE * TILE];
  constexpr int NW = sizeof(ViewScene) / sizeof(float);
  static_assert(sizeof(ViewScene) % sizeof(float) == 0 && NW <= 64 * WAVES, "ViewScene is copied as floats");
  if (threadIdx.x < NW)
    reinterpret_cast<float*>(&S)[threadIdx.x] = reinterpret_cast<const float*>(scenes + v)[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = g * WAVES + wave;
  const int ti = tile / tx, tj = tile - ti * tx;
  const int row = lane >> 3, col = lane & 7;
  const int i = ti * TILE + row, j = tj * TILE + col;
  uint8_t px[3] = {uint8_t(int(255.f * 0.55f + 0.5f)), uint8_t(int(255.f * 0.70f + 0.5f)),
                   uint8_t(int(255.f * 0.90f + 0.5f))};  // background, unshaded
  int id = 0;
  if (tile < ntiles && i < H && j < W && S.tid >= 0) {
    const float* hf = d.bank + size_t(S.tid) * (HF_N * HF_N);
    const float xc = (2.f * (j + 0.5f) / W - 1.f) * (float(W) / float(H)) * tan_half;
    const float yc = (1.f - 2.f * (i + 0.5f) / H) * tan_half;
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
      shade(base, n, dr, px);
    }
  }
  sh_rgb[wave][lane * 3 + 0] = px[0];
  sh_rgb[wave][lane * 3 + 1] = px[1];
  sh_rgb[wave][lane * 3 + 2] = px[2];
  sh_id[wave][lane] = uint8_t(id);
  __syncthreads();
  if (tile < ntiles && i < H) {  // lanes 8 row .. 8 row + 7 write the tile's row
    const int cols = min(TILE, W - tj * TILE);
    const size_t first = size_t(i) * W + size_t(tj) * TILE;
    store_row(rgb + size_t(v) * H * W * 3, first * 3, cols * 3, &sh_rgb[wave][row * TILE * 3], col);
    if (ids) store_row(reinterpret_cast<uint8_t*>(ids) + size_t(v) * H * W, first, cols, &sh_id[wave][row * TILE], col);
  }
}

}  // namespace

size_t view_scene_bytes(int n_views) { return sizeof(ViewScene) * size_t(n_views); }

int launch_view(bool fp64, const ModelT<float>& m, const RenderDev& d, const ViewCam& cam, const int32_t* env_ids,
                int n_views, int H, int W, void* scenes, uint8_t* rgb, int8_t* ids, hipStream_t s) {
  if (n_views <= 0) return 0;
  ViewScene* sc = (ViewScene*)scenes;
  const int64_t ntiles = int64_t((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
  const int64_t blocks = (ntiles + WAVES - 1) / WAVES * n_views;
  if (blocks > 0x7fffffff) return -1;
  if (fp64)
    hipLaunchKernelGGL(view_scene_kernel<double>, dim3((n_views + 63) / 64), dim3(64), 0, s, m, d, cam, env_ids,
                       n_views, sc);
  else
    hipLaunchKernelGGL(view_scene_kernel<float>, dim3((n_views + 63) / 64), dim3(64), 0, s, m, d, cam, env_ids,
                       n_views, sc);
  hipLaunchKernelGGL(view_kernel, dim3((unsigned)blocks), dim3(64 * WAVES), 0, s, m, d, sc, H, W, cam.tan_half, rgb,
                     ids);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bb
