// bb_raycast.h -- the ray caster's surfaces, shared by the depth cameras (bb_render.hip) and the
// world-view renderer (bb_view.hip): the robot's seven primitives from the fixed-tree kinematics
// and the ray tests against them and against the heightfield.  Device code, internal linkage:
// each unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_physics.h"

namespace bb {
namespace {

constexpr float ZNEAR = 1e-4f * 14.142135623730951f;  // ballbot.xml:8 znear * extent

__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ float ray_sphere(const float* o, const float* d, const float* c, float r) {
  const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
  const float b = dot3(oc, d), cc = dot3(oc, oc) - r * r, h = b * b - cc;
  return h < 0.f ? -1.f : -b - sqrtf(h);
}

__device__ float ray_capsule(const float* o, const float* d, const float* pa, const float* pb, float r) {
  const float ba[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  const float oa[3] = {o[0] - pa[0], o[1] - pa[1], o[2] - pa[2]};
  const float baba = dot3(ba, ba), bard = dot3(ba, d), baoa = dot3(ba, oa), rdoa = dot3(d, oa), oaoa = dot3(oa, oa);
  const float a = baba - bard * bard, b = baba * rdoa - baoa * bard, c = baba * oaoa - baoa * baoa - r * r * baba;
  const float h = b * b - a * c;
  if (h < 0.f) return -1.f;
  const bool body = a > 1e-30f;
  const float t = body ? (-b - sqrtf(h)) / a : -1.f;
  const float y = baoa + t * bard;
  if (body && y > 0.f && y < baba) return t;
  float oc[3];
  if (y <= 0.f) { oc[0] = oa[0]; oc[1] = oa[1]; oc[2] = oa[2]; }
  else { oc[0] = o[0] - pb[0]; oc[1] = o[1] - pb[1]; oc[2] = o[2] - pb[2]; }
  const float bb = dot3(d, oc), cc = dot3(oc, oc) - r * r, hh = bb * bb - cc;
  return hh > 0.f ? -bb - sqrtf(hh) : -1.f;
}

// PART: *part receives the face of the entry point, 0 the side, -1 the disc at pa, +1 the disc at pb
template <bool PART>
__device__ float ray_cylinder_face(const float* o, const float* d, const float* pa, const float* pb, float r, int* part) {
  const float ba[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  const float oc[3] = {o[0] - pa[0], o[1] - pa[1], o[2] - pa[2]};
  const float baba = dot3(ba, ba), bard = dot3(ba, d), baoc = dot3(ba, oc);
  const float k2 = baba - bard * bard, k1 = baba * dot3(oc, d) - baoc * bard;
  const float k0 = baba * dot3(oc, oc) - baoc * baoc - r * r * baba;
  float h = k1 * k1 - k2 * k0;
  if (h < 0.f) return -1.f;
  h = sqrtf(h);
  if (k2 > 1e-30f) {
    float t = (-k1 - h) / k2;
    const float y = baoc + t * bard;
    if (y > 0.f && y < baba) {
      if (PART) *part = 0;
      return t;
    }
    if (fabsf(bard) < 1e-30f) return -1.f;
    t = (((y < 0.f) ? 0.f : baba) - baoc) / bard;
    if (PART) *part = y < 0.f ? -1 : 1;
    return fabsf(k1 + k2 * t) < h ? t : -1.f;
  }
  if (k0 > 0.f || fabsf(bard) < 1e-30f) return -1.f;
  const float t0 = -baoc / bard, t1 = (baba - baoc) / bard;
  if (PART) *part = t0 < t1 ? -1 : 1;
  return fminf(t0, t1);
}

__device__ float ray_cylinder(const float* o, const float* d, const float* pa, const float* pb, float r) {
  return ray_cylinder_face<false>(o, d, pa, pb, r, nullptr);
}

// Two-sided Moller-Trumbore.  The barycentric tests accept TRI_PAD (of a cell, 3.4 um) outside the
// triangle: in float u and v carry ~1e-5 of rounding (|o - a| / cell * 2^-24, the hit point's own
// rounding at |x| = 5), so with exact tests 4 rays in 10^6 slipped between the two triangles of a
// cell or two cells and came back as depth 1.  The overlap moves a hit by the change of slope across
// the edge times 3.4 um at most.
constexpr float TRI_PAD = 1e-4f;

__device__ float ray_tri(const float* o, const float* d, const float* a, const float* b, const float* c) {
  const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
  const float det = dot3(e1, p);
  if (fabsf(det) < 1e-30f) return -1.f;
  const float inv = 1.f / det;
  const float s[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
  const float u = dot3(s, p) * inv;
  if (u < -TRI_PAD || u > 1.f + TRI_PAD) return -1.f;
  const float q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
  const float v = dot3(d, q) * inv;
  if (v < -TRI_PAD || u + v > 1.f + TRI_PAD) return -1.f;
  return dot3(e2, q) * inv;
}

// nearest hfield hit in (tmin, tmax) by a 2-D DDA over the cells the ray crosses.  The bound of
// 4 HF_N steps covers any ray: one across the whole field crosses at most 2 (HF_N - 1) cells.
// TRI: *tri receives 2 * (r * HF_N + c) + (1 for the cell's upper triangle B C D) of the hit.
template <bool TRI>
__device__ float ray_hfield_tri(const float* o, const float* d, const float* hf, float size_z, float ztop, float sx,
                                float sy, float tmin, float tmax, int* tri) {
  const int N1 = HF_N - 1;
  const float dx = 2.f * sx / N1, dy = 2.f * sy / N1;
  float t0 = tmin, t1 = tmax;
  // no surface above ztop: start 1 mm before the ray descends through it (flat: the plane hit).
  // The margin is absolute: the start point rounds by up to 5e-7 m at |x| = 5, and a start cell
  // past the hit's cell is a hole.
  if (o[2] > ztop) {
    if (d[2] >= 0.f) return -1.f;
    t0 = fmaxf(t0, (ztop - o[2]) / d[2] - 1e-3f);
  }
  const float half[2] = {sx, sy};
#pragma unroll
  for (int ax = 0; ax < 2; ax++) {
    if (fabsf(d[ax]) < 1e-30f) {
      if (o[ax] < -half[ax] || o[ax] > half[ax]) return -1.f;
      continue;
    }
    float ta = (-half[ax] - o[ax]) / d[ax], tb = (half[ax] - o[ax]) / d[ax];
    if (ta > tb) { const float s = ta; ta = tb; tb = s; }
    t0 = fmaxf(t0, ta);
    t1 = fminf(t1, tb);
  }
  const float px = o[0] + t0 * d[0], py = o[1] + t0 * d[1];
  // negated: a NaN camera pose (diverged state) casts no ray into the field
  if (!(t0 <= t1) || !(fabsf(px) <= 2.f * sx && fabsf(py) <= 2.f * sy)) return -1.f;
  int c = (int)floorf((px + sx) / dx), r = (int)floorf((py + sy) / dy);
  c = c < 0 ? 0 : (c > N1 - 1 ? N1 - 1 : c);
  r = r < 0 ? 0 : (r > N1 - 1 ? N1 - 1 : r);
  const int stc = d[0] > 0.f ? 1 : -1, str = d[1] > 0.f ? 1 : -1;
  const float tdx = fabsf(d[0]) > 1e-30f ? dx / fabsf(d[0]) : 1e30f;
  const float tdy = fabsf(d[1]) > 1e-30f ? dy / fabsf(d[1]) : 1e30f;
  float tmx = fabsf(d[0]) > 1e-30f ? (-sx + (c + (stc > 0)) * dx - o[0]) / d[0] : 1e30f;
  float tmy = fabsf(d[1]) > 1e-30f ? (-sy + (r + (str > 0)) * dy - o[1]) / d[1] : 1e30f;
  for (int it = 0; it < 4 * HF_N; it++) {
    const float x0 = -sx + c * dx, x1 = -sx + (c + 1) * dx, y0 = -sy + r * dy, y1 = -sy + (r + 1) * dy;
    const float A[3] = {x0, y0, hf[r * HF_N + c] * size_z}, B[3] = {x0, y1, hf[(r + 1) * HF_N + c] * size_z};
    const float C[3] = {x1, y0, hf[r * HF_N + c + 1] * size_z}, D[3] = {x1, y1, hf[(r + 1) * HF_N + c + 1] * size_z};
    float best = -1.f;
    bool upper = false;
    const float ta = ray_tri(o, d, A, B, C), tb = ray_tri(o, d, B, C, D);
    if (ta > tmin && ta < tmax) best = ta;
    if (tb > tmin && tb < tmax && (best < 0.f || tb < best)) { best = tb; upper = true; }
    if (best > 0.f) {
      if (TRI) *tri = 2 * (r * HF_N + c) + (upper ? 1 : 0);
      return best;
    }
    if (fminf(tmx, tmy) > t1) break;
    if (tmx < tmy) {
      c += stc; tmx += tdx;
      if (c < 0 || c > N1 - 1) break;
    } else {
      r += str; tmy += tdy;
      if (r < 0 || r > N1 - 1) break;
    }
  }
  return -1.f;
}

__device__ float ray_hfield(const float* o, const float* d, const float* hf, float size_z, float ztop, float sx,
                            float sy, float tmin, float tmax) {
  return ray_hfield_tri<false>(o, d, hf, size_z, ztop, sx, sy, tmin, tmax, nullptr);
}

__device__ void to_world(const Kin<float>& k, const float* pl, float* pw) {
  float t[3];
  mv3(t, k.Rb, pl);
  pw[0] = k.pb[0] + t[0]; pw[1] = k.pb[1] + t[1]; pw[2] = k.pb[2] + t[2];
}

// The seven primitives in world coordinates -> S.ball, S.pa / S.pb / S.rad [6]: 0 tower (cylinder),
// 1-2 sticks, 3-5 wheels (capsules); m a ModelT<float>, k the Kin<float> of the state.  A macro, not
// a function: as a function, force-inlined too, the compiler unrolls these loops before it inlines
// them, contracts other products into FMAs, and the depth images change in their last bit.
#define BB_SCENE_PRIMITIVES(m, k, S)                                                          \
  do {                                                                                        \
    S.ball[0] = k.c[0]; S.ball[1] = k.c[1]; S.ball[2] = k.c[2];                               \
    float a[3], p[3];                                                                         \
    for (int s = -1; s <= 1; s += 2) { /* tower cylinder along the base z axis */             \
      p[0] = m.tower_c[0]; p[1] = m.tower_c[1]; p[2] = m.tower_c[2] + s * m.tower_hh;         \
      to_world(k, p, s < 0 ? S.pa[0] : S.pb[0]);                                              \
    }                                                                                         \
    S.rad[0] = m.tower_r;                                                                     \
    for (int c = 0; c < 2; c++) {                                                             \
      for (int s = -1; s <= 1; s += 2) {                                                      \
        for (int i = 0; i < 3; i++) p[i] = m.stick_c[c][i] + s * m.stick_hh * m.stick_a[c][i]; \
        to_world(k, p, s < 0 ? S.pa[1 + c] : S.pb[1 + c]);                                    \
      }                                                                                       \
      S.rad[1 + c] = m.stick_r;                                                               \
    }                                                                                         \
    for (int w = 0; w < 3; w++) {                                                             \
      mv3(a, k.Rw[w], m.gz);                                                                  \
      for (int s = -1; s <= 1; s += 2) {                                                      \
        for (int i = 0; i < 3; i++) p[i] = k.wc[w][i] + s * m.wheel_hh * a[i];                \
        to_world(k, p, s < 0 ? S.pa[3 + w] : S.pb[3 + w]);                                    \
      }                                                                                       \
      S.rad[3 + w] = m.wheel_r;                                                               \
    }                                                                                         \
  } while (0)

}  // namespace
}  // namespace bb
