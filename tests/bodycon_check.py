"""The checks that hold bb_bodycon.h's four primitives to tests/bodycon_ref.py, shared by the host
test (test_host_bodycon.py, the templates' host build) and the device test (test_gpu_bodycon.py).

tests/hostcheck/bodycon_check.hip is built like collide_check.hip (the same hipcc line, cached in
tests/_build); its host entries need no GPU.  Every check_* runs one primitive on the first n cases
at one precision, asserts, and returns the worst figures it measured.
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import bodycon_ref as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "hostcheck" / "bodycon_check.hip"
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SENTINEL = -12345.0  # what a no-hit must leave in all seven outputs
KIND = dict(capsule=0, cylinder=1, sphere_cylinder=2, sphere_capsule=3)
SIZES = (1, 63, 64, 65, None)  # None: the full set
MAX_DIST_ONLY = 0.10  # of the contacts: the normal's gap too small to hold it
MAX_RIM_EDGE = 0.15   # of the cylinder contacts


class Lib:
    def __init__(self):
        out = ROOT / "tests" / "_build" / "libbodycon_check.so"
        out.parent.mkdir(parents=True, exist_ok=True)
        srcs = [SRC] + sorted(CSRC.glob("*.h"))
        if not (out.exists() and all(out.stat().st_mtime >= s.stat().st_mtime for s in srcs)):
            subprocess.run(["hipcc", "-O2", "-fPIC", "-shared", "--offload-arch=gfx950", "-std=c++17", "-w",
                            f"-I{CSRC}", "-o", str(out), str(SRC)], check=True)
        self.L = C.CDLL(str(out))

    def run(self, kind, device, prec, inp):
        """-> hit[n] (int), out[n, 7] (dist, n, pos; the sentinel where the primitive reported no hit)."""
        inp = np.ascontiguousarray(R.rounded(inp, prec), np.float64)
        n = len(inp)
        dt, ct, fn = ((np.float64, C.c_double, self.L.bc_run_f64) if prec == "fp64" else
                      (np.float32, C.c_float, self.L.bc_run_f32))
        hit = np.full(n + 64, int(SENTINEL), np.int32)  # 64 rows past n, which no lane may write
        out = np.full((n + 64, 7), SENTINEL, dt)
        rc = fn(KIND[kind], int(device), inp.ctypes.data_as(C.POINTER(C.c_double)), n,
                hit.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(ct)))
        assert rc == 0, "the check program's launch failed"
        assert np.all(hit[n:] == int(SENTINEL)) and np.all(out[n:] == dt(SENTINEL)), "a lane past n wrote"
        hit, out = hit[:n], out[:n]
        assert set(np.unique(hit)) <= {0, 1}, "a lane did not run"
        miss = out[hit == 0]
        assert np.all(miss == dt(SENTINEL)), "a no-hit wrote an output"
        return hit, out.astype(np.float64)


def _cut(kind, prec, n):
    cs, ref = R.cases()[kind], R.references(prec)[kind]
    n = len(ref) if n is None else n
    return cs, R.rounded(cs["inp"][:n], prec), ref[:n], n


def _seg_dist(x, p0, p1):
    d = p1 - p0
    t = np.clip((x - p0) @ d / (d @ d), 0.0, 1.0)
    return np.linalg.norm(x - (p0 + t * d))


# ------------------------------------------------------------------ capsule x prism
def check_capsule(lib, device, prec, n=None):
    cs, x, ref, n = _cut("capsule", prec, n)
    hit, out = lib.run("capsule", device, prec, cs["inp"][:n])
    w = dict(dist=0.0, normal=0.0, pos=0.0, excess_a=0.0, n_excess_a=0, contacts=0, dist_only=0, undecided=0)
    for i, o in enumerate(ref):
        row = x[i]
        V = R.prism_vertices(row[:9].reshape(3, 3), row[9])
        c, a, hh, r = row[10:13], row[13:16], row[16], row[17]
        p0, p1 = c - hh * a, c + hh * a
        B = R.bound(prec, max(np.abs(V).max(), np.abs(p0).max(), np.abs(p1).max()))
        what = f"capsule case {i} ({cs['name'][i]}, route {cs['route'][i]}) [{prec}]"
        if abs(o["dist"]) > B:
            assert bool(hit[i]) == o["hit"], f"{what}: hit {hit[i]}, the reference's dist is {o['dist']:.3e}"
        else:
            w["undecided"] += 1
        if not (hit[i] and o["hit"]):
            continue
        w["contacts"] += 1
        dist, nk, pos = out[i, 0], out[i, 1:4], out[i, 4:7]
        class_a_sat = cs["class_a"][i] and o["inside"]
        if class_a_sat:  # a SAT over a subset of the axes can only overestimate the depth
            ex = (-dist - r) - o["depth"]
            assert ex >= -B, f"{what}: depth {-dist - r:.6e} below the reference's {o['depth']:.6e}"
            if ex > B:
                w["n_excess_a"] += 1
                w["excess_a"] = max(w["excess_a"], ex)
        else:
            e = abs(dist - o["dist"])
            assert e <= B, f"{what}: dist {dist:.9e}, reference {o['dist']:.9e}, off by {e:.2e} (bound {B:.2e})"
            w["dist"] = max(w["dist"], e)
        # pos by the header's convention, with the kernel's own normal: pos + n (r + dist / 2) is a point
        # of the segment; inside, one farthest along -n; apart, one whose step back along n by the
        # separation lands on the prism
        xk = pos + nk * (r + dist / 2)
        assert _seg_dist(xk, p0, p1) <= B, f"{what}: pos is {_seg_dist(xk, p0, p1):.2e} off the segment's line through n"
        short = nk @ xk - min(nk @ p0, nk @ p1)
        q = xk - nk * (dist + r)
        out_by = max(nn @ q - d for nn, d in R.prism_halfspaces(V))
        if -dist - r > B:
            assert short <= B, f"{what}: pos is {short:.2e} short of the deepest point along n"
        elif -dist - r < -B:
            assert out_by <= B, f"{what}: the prism-side point of pos is {out_by:.2e} outside the prism"
        else:  # the segment touches the prism: either reading
            assert short <= B or out_by <= B, f"{what}: pos fits neither reading ({short:.2e}, {out_by:.2e})"
        assert abs(np.linalg.norm(nk) - 1) <= 1e-3, f"{what}: |n| = {np.linalg.norm(nk)}"
        exact = not class_a_sat or abs((-dist - r) - o["depth"]) <= B
        if o["gap"] > 100 * B and exact:
            en = np.abs(nk - o["normal"]).max()
            assert en <= B / o["gap"], f"{what}: normal off by {en:.2e} (bound {B / o['gap']:.2e})"
            w["normal"] = max(w["normal"], en)
            d_hat = (p1 - p0) / np.linalg.norm(p1 - p0)
            if len(o["deep"]) == 1 and abs(o["normal"] @ d_hat) > 1e-3:  # the reference's deepest point is an end
                xr = p0 if o["deep"][0] == 0 else p1
                ep = np.abs(pos - (xr - o["normal"] * (r + o["dist"] / 2))).max()
                bp = 2 * B + B / o["gap"] * (r + abs(o["dist"]))
                assert ep <= bp, f"{what}: pos off the reference's by {ep:.2e} (bound {bp:.2e})"
                w["pos"] = max(w["pos"], ep)
        elif exact:
            w["dist_only"] += 1
    return w


# ------------------------------------------------------------------ cylinder x prism
def check_cylinder(lib, device, prec, n=None):
    cs, x, ref, n = _cut("cylinder", prec, n)
    hit, out = lib.run("cylinder", device, prec, cs["inp"][:n])
    w = dict(below=0.0, above=0.0, contacts=0, rim_edge=0, excess_b=[], separated_b=[], pos_checked=0, normal=0.0,
             pos=0.0)
    for i, o in enumerate(ref):
        row = x[i]
        V = R.prism_vertices(row[:9].reshape(3, 3), row[9])
        c, a, hh, r = row[10:13], row[13:16], row[16], row[17]
        B = R.bound(prec, max(np.abs(V).max(), np.abs(c).max() + hh + r))
        what = f"cylinder case {i} ({o['feature']}{', rim x edge' if o['rim_edge'] else ''}) [{prec}]"
        dist, nk, pos = out[i, 0], out[i, 1:4], out[i, 4:7]
        depth = -dist
        truly = not o["apart_inner"]  # the inscribed polygon intersects: the shapes do
        if truly:
            w["contacts"] += 1
            w["rim_edge"] += o["rim_edge"]
        if truly and o["lo"] > B:
            assert hit[i], f"{what}: no contact, the inscribed polygon is {o['lo']:.3e} deep"
        if not hit[i]:
            continue
        if o["rim_edge"]:  # class B: the axis set has no rim x edge axis, the depth can only be too large
            if o["apart_outer"]:
                w["separated_b"].append(depth)
            elif truly:
                assert depth >= o["lo"] - B, f"{what}: depth {depth:.6e} below the bracket's {o['lo']:.6e}"
                if depth > o["hi"] + B:
                    w["excess_b"].append(depth - o["hi"])
            continue
        assert not o["apart_outer"], (f"{what}: a contact of depth {depth:.3e} between shapes {o['sep']:.3e} apart "
                                      f"(n* = {o['normal']}, prism vertices in the feature {o['vertex']})")
        if not truly:
            continue  # between the two polygons: the answer is within 8.3e-6 of touching
        assert o["lo"] - B <= depth <= o["hi"] + B, (f"{what}: depth {depth:.9e} outside [{o['lo']:.9e}, {o['hi']:.9e}] "
                                                     f"by {max(o['lo'] - depth, depth - o['hi']):.2e} (B {B:.2e})")
        w["below"] = max(w["below"], o["lo"] - depth)
        w["above"] = max(w["above"], depth - o["hi"])
        if o["feature"] in ("cap", "side_vertex"):
            # pos + n dist / 2 is a point of the cylinder farthest along -n (the header's convention)
            xk = pos + nk * (dist / 2) - c
            z = xk @ a
            rho = np.linalg.norm(xk - z * a)
            assert abs(z) <= hh + B and rho <= r + B, f"{what}: pos's surface point is off the cylinder (z {z}, rho {rho})"
            na = nk @ a
            low = -(hh * abs(na) + r * np.linalg.norm(nk - na * a))  # (1 - na^2 cancels; the rejection does not)
            assert nk @ xk <= low + 2 * B, f"{what}: pos is {nk @ xk - low:.2e} short of the deepest point along n"
            # where that point is a whole disc or a whole line of the wall, the header takes the one
            # nearest the prism's centroid
            dc = V.mean(axis=0) - c
            if o["feature"] == "cap" and abs(abs(na) - 1) <= 4 * R.EPS[prec]:
                pr = dc - (dc @ a) * a
                want = -np.sign(na) * hh * a + pr * min(1.0, r / np.linalg.norm(pr))
            elif o["feature"] == "side_vertex" and abs(na) <= 4 * R.EPS[prec]:
                rad = nk - na * a
                want = np.clip(dc @ a, -hh, hh) * a - r * rad / np.linalg.norm(rad)
            else:
                want = None
            if want is not None:
                ep = np.abs(xk - want).max()
                assert ep <= 4 * B, f"{what}: pos's surface point is {ep:.2e} off the header's choice"
                w["pos"] = max(w["pos"], ep)
            w["pos_checked"] += 1
            if o["feature"] == "cap" and o["gap"] > 100 * B:
                en = np.abs(nk - o["normal"]).max()
                assert en <= B / o["gap"], f"{what}: normal off by {en:.2e}"
                w["normal"] = max(w["normal"], en)
    return w


# ------------------------------------------------------------------ sphere x cylinder, sphere x capsule
def check_sphere(lib, device, prec, kind, n=None):
    cs, x, ref, n = _cut(kind, prec, n)
    hit, out = lib.run(kind, device, prec, cs["inp"][:n])
    w = dict(dist=0.0, normal=0.0, pos=0.0, contacts=0, dist_only=0, undecided=0, tol=0.0)
    for i, o in enumerate(ref):
        row = x[i]
        sc, sr, c = row[:3], row[3], row[4:7]
        B = R.bound(prec, max(np.abs(sc).max(), np.abs(c).max()))
        what = f"{kind} case {i} ({cs['kind'][i]}) [{prec}]"
        lo, hi = (o["dist_lo"], o["dist_hi"]) if kind == "sphere_cylinder" else (o["dist"], o["dist"])
        tol = B + o["tol"]
        if min(abs(lo), abs(hi)) > tol and lo * hi > 0:
            assert bool(hit[i]) == o["hit"], f"{what}: hit {hit[i]}, the reference's dist is {hi:.3e}"
        else:
            w["undecided"] += 1
        if not (hit[i] and o["hit"]):
            continue
        w["contacts"] += 1
        w["tol"] = max(w["tol"], o["tol"])
        dist, nk, pos = out[i, 0], out[i, 1:4], out[i, 4:7]
        e = max(lo - dist, dist - hi)
        assert e <= tol, f"{what}: dist {dist:.9e} outside [{lo:.9e}, {hi:.9e}] by {e:.2e} (bound {tol:.2e})"
        w["dist"] = max(w["dist"], e)
        # pos = centre + n (r + dist / 2), with the kernel's own normal
        ec = np.abs(pos - (sc + nk * (sr + dist / 2))).max()
        assert ec <= B, f"{what}: pos is {ec:.2e} off the centre's line along n"
        assert abs(np.linalg.norm(nk) - 1) <= 1e-3, f"{what}: |n| = {np.linalg.norm(nk)}"
        if o["normal"] is not None and o["gap"] > 100 * tol:
            nb = (B + o.get("xerr", 0.0)) / o["gap"] + (np.pi / R.K_GON if o.get("side") else 0.0)
            en = np.abs(nk - o["normal"]).max()
            assert en <= nb, f"{what}: normal off by {en:.2e} (bound {nb:.2e})"
            if not o.get("side"):
                w["normal"] = max(w["normal"], en)
                ep = np.abs(pos - (sc + o["normal"] * (sr + (lo + hi) / 4))).max()
                bp = 2 * tol + nb * (sr + abs(lo)) + (hi - lo)
                assert ep <= bp, f"{what}: pos off the reference's by {ep:.2e} (bound {bp:.2e})"
                w["pos"] = max(w["pos"], ep)
        else:
            w["dist_only"] += 1
    return w


# ------------------------------------------------------------------ the case set's own conditions
def check_case_set(prec):
    """What keeps the cases from hiding failures, from the reference alone."""
    cs, ref = R.cases(), R.references(prec)
    cap = cs["capsule"]
    x = R.rounded(cap["inp"], prec)
    low = np.minimum(x[:, 12] - x[:, 16] * x[:, 15], x[:, 12] + x[:, 16] * x[:, 15]) - x[:, 9]
    assert cap["class_a"].sum() == 200 and np.all(np.abs(low[cap["class_a"]]) <= 0.02 + 1e-6)
    assert np.all(low[~cap["class_a"]] > 0.03), "a case outside class A has its lower end within 3 cm of the bottom"
    assert cap["degenerate"].sum() >= 40
    for s in range(0, len(x) - 63, 64):
        assert len(set(cap["route"][s:s + 64])) == 3, f"wave {s // 64} does not hold all three routes"
    L = np.abs(x[:, :13]).max(axis=1)
    hits = np.array([o["hit"] for o in ref["capsule"]])
    small = np.array([o["gap"] <= 100 * R.bound(prec, l) for o, l in zip(ref["capsule"], L)])
    assert (hits & small).sum() <= MAX_DIST_ONLY * hits.sum(), ((hits & small).sum(), hits.sum())
    only = dict(capsule=int((hits & small).sum()))
    for kind in ("sphere_cylinder", "sphere_capsule"):
        xs = R.rounded(cs[kind]["inp"], prec)
        Ls = np.abs(xs[:, [0, 1, 2, 4, 5, 6]]).max(axis=1)
        h = [o for o in ref[kind] if o["hit"]]
        ill = sum(o["normal"] is None or o["gap"] <= 100 * (R.bound(prec, l) + o["tol"])
                  for o, l in zip(ref[kind], Ls) if o["hit"])
        assert ill <= MAX_DIST_ONLY * len(h), (kind, ill, len(h))
        only[kind] = ill
    con = [o for o in ref["cylinder"] if not o["apart_inner"]]
    rim = sum(o["rim_edge"] for o in con)
    assert len(con) >= 40 and rim <= MAX_RIM_EDGE * len(con), (rim, len(con))
    return dict(capsule_hits=int(hits.sum()), dist_only=only,
                routes=np.bincount(cap["route"]).tolist(), cylinder_contacts=len(con), rim_edge=int(rim),
                cylinder_apart=sum(o["apart_outer"] for o in ref["cylinder"]))


def check_against(lib, prec, kind):
    """Device against host build: the same hit flags everywhere, dist within B."""
    cs = R.cases()[kind]
    x = R.rounded(cs["inp"], prec)
    hd, od = lib.run(kind, 1, prec, cs["inp"])
    hh, oh = lib.run(kind, 0, prec, cs["inp"])
    assert np.array_equal(hd, hh), f"{kind} [{prec}]: hit flags differ at cases {np.nonzero(hd != hh)[0][:8]}"
    cols = slice(0, 13) if kind in ("capsule", "cylinder") else [0, 1, 2, 4, 5, 6]
    B = R.bound(prec, np.abs(x[:, cols]).max(axis=1) + (0.25 if kind == "cylinder" else 0.0))
    m = hd == 1
    e = np.abs(od[m, 0] - oh[m, 0])
    assert np.all(e <= B[m]), f"{kind} [{prec}]: dist differs from the host build's by {e.max():.2e}"
    return float(e.max()) if m.any() else 0.0
