// Test-only host program (tests/test_host_prism_window.py): prism_window (bb_physics.h), the cell
// window t16::collide_team walks, against brute force over the whole sub-grid under the ball's
// AABB, in float and double.  Per case:
//   * with no bound, and with a bound far above the ball, the window is the AABB's (a copy of
//     collide_ground's text below), and a rejected ball (off the field, NaN) is rejected;
//   * with a bound Z the window is a subset of the AABB's;
//   * every prism of the AABB's sub-grid that passes collide_ground's z cull and coarse test,
//     evaluated in T on the vertices collide_team forms, lies inside the window: zero misses;
//   * the contact list (sphere_prism on the survivors, in order, uncapped) over the window is the
//     list over the AABB's sub-grid, bit for bit.
// Z is taken both ways a caller may: the field's top T(max h) * size_z (what forward passes), and
// the exact maximum of T(h) * size_z over the sub-grid's vertices (the tightest valid bound).
// Fields: flat, ones, a sinusoid and Gaussian hills, size_z 0.3, 1 and 2.  Cases: penetrations
// from 1e-4 m to r, a ball 1 mm above the ground, a grazing ball (c[2] - Z = r within +-3 ulps),
// centres on grid lines and vertices within +-1 ulp, centres at the field's edge and outside it.
// Prints its counts and "ok" and returns 0, or says what differs.  Never shipped.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bb_model.h"
#include "bb_physics.h"

using namespace bb;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {  // xorshift64*, uniform in [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return double((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / double(1ull << 53);
}
static double uni(double a, double b) { return a + (b - a) * rnd(); }

struct Win {
  int cmin, cmax, rmin, rmax;
  bool operator==(const Win& o) const { return cmin == o.cmin && cmax == o.cmax && rmin == o.rmin && rmax == o.rmax; }
};

// collide_ground's AABB test and sub-grid, its text
template <typename T>
static bool aabb_window(const ModelT<T>& m, const T* c, T size_z, Win& w) {
  const T r = m.ball_r;
  const T sx = m.hf_sx, sy = m.hf_sy, zb = m.hf_bottom;
  T xmin = c[0] - r, xmax = c[0] + r, ymin = c[1] - r, ymax = c[1] + r, zmin = c[2] - r, zmax = c[2] + r;
  if (!(xmin <= sx && xmax >= -sx && ymin <= sy && ymax >= -sy && zmin <= size_z && zmax >= -zb)) return false;
  const int N1 = HF_N - 1;
  int cmin = (int)floor((xmin + sx) / (2 * sx) * N1);
  int cmax = (int)ceil((xmax + sx) / (2 * sx) * N1);
  int rmin = (int)floor((ymin + sy) / (2 * sy) * N1);
  int rmax = (int)ceil((ymax + sy) / (2 * sy) * N1);
  cmin = cmin < 0 ? 0 : cmin;
  cmax = cmax > N1 ? N1 : cmax;
  rmin = rmin < 0 ? 0 : rmin;
  rmax = rmax > N1 ? N1 : rmax;
  w = Win{cmin, cmax, rmin, rmax};
  return true;
}

struct Hit {
  int rr, cc, tri;  // cell row, cell column, triangle of the cell
  double n[3], dist;
};

// collide_team's enumeration of window w, one prism after the other: the prisms that pass the z
// cull and the coarse test (`coarse`), and of those the contacts (`hits`)
template <typename T>
static void walk(const ModelT<T>& m, const T* c, const float* hf, T size_z, const Win& w, std::vector<Hit>& coarse,
                 std::vector<Hit>& hits) {
  coarse.clear();
  hits.clear();
  const T r = m.ball_r, sx = m.hf_sx, sy = m.hf_sy, zb = m.hf_bottom, zmin = c[2] - r;
  const int ncol = w.cmax - w.cmin + 1, np = 2 * ncol - 2;
  const int total = (w.rmax - w.rmin) * (np > 0 ? np : 0);
  T dx, dy;
  once_pitch(m, dx, dy);
  for (int P = 0; P < total; P++) {
    const int rr = w.rmin + P / np, p = P % np;
    T V[3][3];
    for (int t = 0; t < 3; t++) {
      const int vt = p + t, cc = w.cmin + (vt >> 1), ri = rr + (vt & 1);
      V[t][0] = dx * cc - sx;
      V[t][1] = dy * ri - sy;
      V[t][2] = T(hf[ri * HF_N + cc]) * size_z;
    }
    if (V[0][2] < zmin && V[1][2] < zmin && V[2][2] < zmin) continue;
    const T bx0 = minT(V[0][0], minT(V[1][0], V[2][0])), bx1 = maxT(V[0][0], maxT(V[1][0], V[2][0]));
    const T by0 = minT(V[0][1], minT(V[1][1], V[2][1])), by1 = maxT(V[0][1], maxT(V[1][1], V[2][1]));
    const T ztop = maxT(V[0][2], maxT(V[1][2], V[2][2]));
    const T ex = maxT(T(0), maxT(bx0 - c[0], c[0] - bx1));
    const T ey = maxT(T(0), maxT(by0 - c[1], c[1] - by1));
    const T ez = maxT(T(0), c[2] - ztop);
    if (!(ex * ex + ey * ey + ez * ez <= r * r)) continue;
    Hit h{rr, w.cmin + (p >> 1), p & 1, {0, 0, 0}, 0};
    coarse.push_back(h);
    T nn[3] = {0, 0, 1}, dist = 0;
    if (!sphere_prism(c, r, V, -zb, nn, &dist)) continue;
    for (int i = 0; i < 3; i++) h.n[i] = double(nn[i]);
    h.dist = double(dist);
    hits.push_back(h);
  }
}

struct Field {
  const char* name;
  std::vector<float> h;
  float hmax;
};

static std::vector<Field> fields() {
  std::vector<Field> out(4);
  const int n = HF_N;
  out[0].name = "flat";
  out[0].h.assign(n * n, 0.f);
  out[1].name = "ones";
  out[1].h.assign(n * n, 1.f);
  out[2].name = "sinusoid";
  out[2].h.resize(n * n);
  out[3].name = "hills";
  out[3].h.resize(n * n);
  double hx[12], hy[12], hs[12], ha[12];
  for (int k = 0; k < 12; k++) { hx[k] = uni(0, n); hy[k] = uni(0, n); hs[k] = uni(4, 40); ha[k] = uni(0.3, 1); }
  double top = 0;
  std::vector<double> hill(n * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      out[2].h[i * n + j] = float(0.5 + 0.5 * sin(0.37 * j) * cos(0.23 * i));
      double s = 0;
      for (int k = 0; k < 12; k++)
        s += ha[k] * exp(-((j - hx[k]) * (j - hx[k]) + (i - hy[k]) * (i - hy[k])) / (2 * hs[k] * hs[k]));
      hill[i * n + j] = s;
      top = s > top ? s : top;
    }
  for (int i = 0; i < n * n; i++) out[3].h[i] = float(hill[i] / top);
  for (Field& f : out) {
    f.hmax = f.h[0];
    for (float x : f.h) f.hmax = x > f.hmax ? x : f.hmax;
  }
  return out;
}

template <typename T>
static T step_ulps(T x, int k) {
  for (int i = 0; i < (k < 0 ? -k : k); i++) x = T(nextafter(x, k < 0 ? T(-1e30) : T(1e30)));
  return x;
}

struct Counts {
  long cases = 0, rejected = 0, passing = 0, contacts = 0, misses = 0, flat_cases = 0, flat_parent = 0, flat_kept = 0;
};

static int fail(const char* what, const char* type, const char* field, double size_z, const double* c, double Z) {
  printf("%s (%s, %s, size_z %g, centre %.17g %.17g %.17g, Z %.17g)\n", what, type, field, size_z, c[0], c[1], c[2],
         Z);
  return 1;
}

// one centre, one bound: the checks of the header
template <typename T>
static int check(const ModelT<T>& m, const Field& f, double size_z_d, const double* cd, T Z, bool shallow,
                 Counts& n) {
  const char* type = sizeof(T) == 8 ? "double" : "float";
  const T size_z = T(size_z_d);
  const T c[3] = {T(cd[0]), T(cd[1]), T(cd[2])};
  Win pw{-1, -1, -1, -1}, w0{-2, -2, -2, -2}, wf{-3, -3, -3, -3}, w{-4, -4, -4, -4};
  const bool live = aabb_window(m, c, size_z, pw);
  n.cases++;
  if (prism_window(m, c, size_z, prism_no_bound<T>(), w0.cmin, w0.cmax, w0.rmin, w0.rmax) != live ||
      prism_window(m, c, size_z, T(cd[2] + 10.0), wf.cmin, wf.cmax, wf.rmin, wf.rmax) != live ||
      prism_window(m, c, size_z, Z, w.cmin, w.cmax, w.rmin, w.rmax) != live)
    return fail("the AABB test's answer differs", type, f.name, size_z_d, cd, double(Z));
  if (!live) {
    n.rejected++;
    return 0;
  }
  if (!(w0 == pw)) return fail("no bound: not the AABB's window", type, f.name, size_z_d, cd, double(Z));
  if (!(wf == pw)) return fail("bound far above the ball: not the AABB's window", type, f.name, size_z_d, cd, double(Z));
  if (w.cmin < pw.cmin || w.cmax > pw.cmax || w.rmin < pw.rmin || w.rmax > pw.rmax)
    return fail("the window is no subset of the AABB's", type, f.name, size_z_d, cd, double(Z));
  std::vector<Hit> pc, ph, wc, wh;
  walk(m, c, f.h.data(), size_z, pw, pc, ph);
  walk(m, c, f.h.data(), size_z, w, wc, wh);
  n.passing += long(pc.size());
  n.contacts += long(ph.size());
  for (const Hit& h : pc)
    if (h.rr < w.rmin || h.rr + 1 > w.rmax || h.cc < w.cmin || h.cc + 1 > w.cmax) {
      n.misses++;
      printf("prism row %d col %d tri %d passes outside window cols %d..%d rows %d..%d (AABB %d..%d, %d..%d)\n", h.rr,
             h.cc, h.tri, w.cmin, w.cmax, w.rmin, w.rmax, pw.cmin, pw.cmax, pw.rmin, pw.rmax);
      return fail("a passing prism is outside the window", type, f.name, size_z_d, cd, double(Z));
    }
  if (ph.size() != wh.size()) return fail("contact counts differ", type, f.name, size_z_d, cd, double(Z));
  for (size_t i = 0; i < ph.size(); i++)
    if (ph[i].rr != wh[i].rr || ph[i].cc != wh[i].cc || ph[i].tri != wh[i].tri ||
        memcmp(ph[i].n, wh[i].n, sizeof ph[i].n) != 0 || memcmp(&ph[i].dist, &wh[i].dist, sizeof(double)) != 0)
      return fail("contact lists differ", type, f.name, size_z_d, cd, double(Z));
  if (shallow) {
    const int npp = 2 * (pw.cmax - pw.cmin), npw = 2 * (w.cmax - w.cmin);
    n.flat_cases++;
    n.flat_parent += (pw.rmax - pw.rmin) * (npp > 0 ? npp : 0);
    n.flat_kept += (w.rmax > w.rmin ? w.rmax - w.rmin : 0) * (npw > 0 ? npw : 0);
  }
  return 0;
}

// the exact maximum of T(h) * size_z over the vertices of the AABB's sub-grid (the field's top off the field)
template <typename T>
static T patch_top(const ModelT<T>& m, const Field& f, double size_z, const double* cd) {
  const T c[3] = {T(cd[0]), T(cd[1]), T(cd[2])};
  Win pw;
  T top = T(f.hmax) * T(size_z);
  if (!aabb_window(m, c, T(size_z), pw)) return top;
  bool any = false;
  for (int ri = pw.rmin; ri <= pw.rmax; ri++)
    for (int cc = pw.cmin; cc <= pw.cmax; cc++) {
      const T z = T(f.h[ri * HF_N + cc]) * T(size_z);
      top = !any || z > top ? z : top;
      any = true;
    }
  return top;
}

template <typename T>
static int run(const std::vector<Field>& fs, Counts& n) {
  const ModelT<T> m = cast_model<T>(compile_model(default_solver(sizeof(T) == 8)));
  const double r = double(m.ball_r), sx = double(m.hf_sx), sy = double(m.hf_sy);
  const double dx = 2 * sx / (HF_N - 1), dy = 2 * sy / (HF_N - 1);
  const double size_zs[3] = {0.3, 1.0, 2.0};
  const double deltas[] = {1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 4e-3, 8e-3, 0.015, 0.03, 0.05, 0.07, 0.0899, 0.09};
  for (const Field& f : fs)
    for (double size_z : size_zs) {
      const bool flat = f.hmax == 0.f;
      // both bounds for one centre; on every failure the case is printed
      auto both = [&](const double* cd, bool shallow) {
        const T top = T(f.hmax) * T(size_z);
        if (check<T>(m, f, size_z, cd, top, shallow && flat, n)) return 1;
        return check<T>(m, f, size_z, cd, patch_top<T>(m, f, size_z, cd), false, n);
      };
      auto ground = [&](double x, double y) {  // the nearest vertex's height
        int cc = int(lrint((x + sx) / dx)), rr = int(lrint((y + sy) / dy));
        cc = cc < 0 ? 0 : (cc > HF_N - 1 ? HF_N - 1 : cc);
        rr = rr < 0 ? 0 : (rr > HF_N - 1 ? HF_N - 1 : rr);
        return double(f.h[rr * HF_N + cc]) * size_z;
      };
      for (int rep = 0; rep < 40; rep++) {
        const double x = uni(-4.8, 4.8), y = uni(-4.8, 4.8), z0 = ground(x, y);
        for (double d : deltas) {  // penetrations
          const double c[3] = {x, y, z0 + r - d};
          if (both(c, d >= 5e-4 && d <= 4e-3)) return 1;
        }
        const double above[3] = {x, y, z0 + r + 1e-3};  // 1 mm above the ground
        if (both(above, false)) return 1;
        // grazing: c[2] - Z = r within a few ulps, for both bounds
        for (int which = 0; which < 2; which++)
          for (int k = -3; k <= 3; k++) {
            double c[3] = {x, y, 0};
            const double Z = double(which ? patch_top<T>(m, f, size_z, above) : T(f.hmax) * T(size_z));
            c[2] = double(step_ulps<T>(T(Z + r), k));
            if (both(c, false)) return 1;
          }
        // a centre on a grid line, on a vertex, within +-1 ulp
        const int cc = 3 + int(rnd() * 286), rr = 3 + int(rnd() * 286);
        for (int kx = -1; kx <= 1; kx++)
          for (int ky = -1; ky <= 1; ky++)
            for (double d : {2e-4, 2e-3, 0.03}) {
              const double xv = double(step_ulps<T>(T(dx * cc - sx), kx)), yv = double(step_ulps<T>(T(dy * rr - sy), ky));
              const double onv[3] = {xv, yv, ground(xv, yv) + r - d};
              const double online[3] = {xv, y, ground(xv, y) + r - d};
              const double online2[3] = {x, yv, ground(x, yv) + r - d};
              if (both(onv, false) || both(online, false) || both(online2, false)) return 1;
            }
        // at the field's edge, inside and outside it, and off the field
        for (double d : {2e-4, 2e-3, 0.03}) {
          const double sg = rnd() < 0.5 ? -1.0 : 1.0, off = uni(-0.12, 0.12);
          const double e1[3] = {sg * sx + off, y, ground(sg * sx + off, y) + r - d};
          const double e2[3] = {x, sg * sy + off, ground(x, sg * sy + off) + r - d};
          const double e3[3] = {sg * sx + off, -sg * sy - off, ground(sg * sx + off, -sg * sy - off) + r - d};
          const double e4[3] = {sg * sx, y, ground(sg * sx, y) + r - d};  // on the edge itself
          const double e5[3] = {sg * (sx + r), y, ground(sg * sx, y) + r - d};  // the AABB touches the edge
          const double out[3] = {sg * (sx + 0.2), y, z0 + r - d};
          if (both(e1, false) || both(e2, false) || both(e3, false) || both(e4, false) || both(e5, false) ||
              both(out, false))
            return 1;
        }
      }
      const double bad[3] = {NAN, 0.3, r}, bad2[3] = {0.1, 0.3, NAN};
      if (both(bad, false) || both(bad2, false)) return 1;
      // a NaN bound leaves the AABB's window
      const double c[3] = {0.1, 0.3, r - 1e-3};
      Win pw, w;
      const T ct[3] = {T(c[0]), T(c[1]), T(c[2])};
      if (!aabb_window(m, ct, T(size_z), pw) || !prism_window(m, ct, T(size_z), T(NAN), w.cmin, w.cmax, w.rmin, w.rmax) ||
          !(w == pw))
        return fail("NaN bound: not the AABB's window", sizeof(T) == 8 ? "double" : "float", f.name, size_z, c, NAN);
    }
  return 0;
}

int main() {
  if (!kPrismWindow) {
    printf("built with -DBB_NO_PRISM_WINDOW: nothing to check\n");
    return 1;
  }
  const std::vector<Field> fs = fields();
  for (int pass = 0; pass < 2; pass++) {
    Counts n;
    if (pass ? run<float>(fs, n) : run<double>(fs, n)) return 1;
    printf("%s: %ld cases (%ld rejected by the AABB test), %ld passing prisms, %ld contacts, %ld misses; flat, "
           "0.5 to 4 mm deep: %.1f of %.1f prisms kept\n",
           pass ? "float" : "double", n.cases, n.rejected, n.passing, n.contacts, n.misses,
           n.flat_cases ? double(n.flat_kept) / n.flat_cases : 0.0,
           n.flat_cases ? double(n.flat_parent) / n.flat_cases : 0.0);
    if (n.misses || n.passing < 100000 || n.rejected < 100) {
      printf("too few cases of a kind, or a miss\n");
      return 1;
    }
  }
  printf("ok\n");
  return 0;
}
