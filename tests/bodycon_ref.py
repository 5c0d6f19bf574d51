"""A reference for the base-tree contact primitives of bb_bodycon.h, written from the geometry alone.

Two convex bodies A (the prism, or a sphere's centre) and B (a capsule's axis segment, a cylinder)
intersect iff the origin lies in the Minkowski difference A - B, and then the penetration depth (the
shortest translation that separates them) is the origin's distance to the boundary of A - B; when
they are apart, their distance is the origin's distance to A - B.  For polytopes A - B is the convex
hull of the vertex differences, which Qhull builds (scipy.spatial.ConvexHull): facet equations
n.x + offset <= 0, so the depth is min(-offset) and its normal the minimising facet's.  No axis list
and no case split: the hull is the only construction.  A cylinder is bracketed between two prisms
over regular K-gons, inscribed and circumscribed: inner <= true <= outer, r (1 / cos(pi / K) - 1)
apart (8.3e-6 m for the tower at K = 256).

Signs.  A is the first body, B the second; a facet normal n of A - B is the direction that moves B
out of A, which is bb_bodycon.h's "normal from prism to capsule" and, for the sphere pairs (the
sphere first), "normal from sphere to cylinder".
"""
import numpy as np
from scipy.optimize import minimize
from scipy.spatial import ConvexHull

K_GON = 256
HF_N, HF_SX, HF_BOTTOM = 293, 5.0, -0.1           # the terrain grid: 292 cells over 10 m, bottom 0.1 below zero
CELL = 2 * HF_SX / (HF_N - 1)
TOWER = dict(r=0.11, hh=0.14)
STICK = dict(r=0.01, hh=0.1)
WHEEL = dict(r=0.025, hh=0.02)
BALL_R = 0.09
EPS = {"fp64": 2.220446049250313e-16, "fp32": 1.1920929e-7}
# The bound of every comparison is B = C eps(T) L, L the largest coordinate magnitude of the case.
# C counts the roundings that act at magnitude L on the way to dist (everything else is formed from
# differences of nearby points, whose roundings are relative to the small results): the segment end
# c -+ hh a (1), a three-term dot product of an axis with a vertex (3), one with a segment end or the
# cylinder's centre (3), the plane offset or the second support (3), the final difference (1): 11,
# taken as 16 as in collide_ref.BOUNDS.
C_BOUND = 16


def bound(prec, L):
    return C_BOUND * EPS[prec] * L


# ------------------------------------------------------------------ distance of the origin to triangles
def _origin_to_triangles(T):
    """T[m, 3, 3] -> (distance[m], closest point[m, 3]) of the origin to each triangle: the foot of the
    perpendicular when it falls inside, else the nearest point of the three sides."""
    A, B, C = T[:, 0], T[:, 1], T[:, 2]
    best = np.full(len(T), np.inf)
    q = np.zeros((len(T), 3))
    for P, Q in ((A, B), (B, C), (C, A)):  # the sides: clamp the foot on each line
        d = Q - P
        dd = np.einsum("ij,ij->i", d, d)
        t = np.clip(np.where(dd > 0, -np.einsum("ij,ij->i", P, d) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
        x = P + t[:, None] * d
        dist = np.linalg.norm(x, axis=1)
        take = dist < best
        best = np.where(take, dist, best)
        q[take] = x[take]
    n = np.cross(B - A, C - A)
    nn = np.einsum("ij,ij->i", n, n)
    ok = nn > 0
    nn = np.where(ok, nn, 1.0)
    foot = n * (np.einsum("ij,ij->i", A, n) / nn)[:, None]  # the origin's projection on the plane
    # inside iff the foot is on the inner side of all three sides
    s = [np.einsum("ij,ij->i", np.cross(Q - P, foot - P), n) for P, Q in ((A, B), (B, C), (C, A))]
    inside = ok & (s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)
    dist = np.linalg.norm(foot, axis=1)
    take = inside & (dist <= best)
    best = np.where(take, dist, best)
    q[take] = foot[take]
    return best, q


def hull_origin(pts):
    """The origin against the hull of pts[m, 3].  Inside (every facet offset <= 0): depth = min(-offset),
    normal = that facet's, gap = how much deeper the next facet of a distinct normal is.  Outside:
    dist = the distance to the hull, w = the hull's closest point, normal = -w / |w|, gap = dist (the
    normal divides by it).  `support` lists the indices of the points within 1e-9 of the hull's support
    along the normal -- the vertices of the contact feature."""
    h = ConvexHull(pts)
    nrm, off = h.equations[:, :3], h.equations[:, 3]
    if off.max() <= 0:
        k = int(np.argmin(-off))
        n, depth = nrm[k], -off[k]
        other = nrm @ n < 1 - 1e-9
        gap = float((-off[other]).min() - depth) if other.any() else np.inf
        out = dict(inside=True, depth=float(depth), normal=n.copy(), gap=gap)
    else:
        d, q = _origin_to_triangles(pts[h.simplices])
        k = int(np.argmin(d))
        n = -q[k] / d[k] if d[k] > 0 else nrm[int(np.argmax(off))]
        out = dict(inside=False, dist=float(d[k]), w=q[k].copy(), normal=n.copy(), gap=float(d[k]))
    out["eq"] = h.equations
    s = pts @ out["normal"]
    out["support"] = np.nonzero(s >= s.max() - 1e-9)[0]
    return out


# ------------------------------------------------------------------ segment x prism
def prism_vertices(tri, zb):
    """tri[3, 3] (the top triangle), zb -> V[6, 3]: the top vertices, then the same at the bottom."""
    tri = np.asarray(tri, float)
    low = tri.copy()
    low[:, 2] = zb
    return np.concatenate([tri, low])


def segment_prism(V, c, a, hh):
    """The axis segment c -+ hh a against the prism V[6, 3]: hull_origin of the 12 points V_i - p_j
    (formed as (V_i - c) +- hh a, so that no rounding acts at the coordinates' magnitude), with
    `deep`: the segment's end(s) farthest along -normal when inside, the ends the closest feature
    uses when outside (0: the lower parameter end c - hh a, 1: the other)."""
    V, c, a = np.asarray(V, float), np.asarray(c, float), np.asarray(a, float)
    rel = V - c
    pts = np.concatenate([rel + hh * a, rel - hh * a])  # V_i - p0, V_i - p1
    out = hull_origin(pts)
    out["deep"] = np.unique(out["support"] // 6)
    return out


def capsule_prism(V, c, a, hh, r):
    """-> dict(dist, hit, normal, gap, inside, deep): dist = -depth - r inside, distance - r outside."""
    o = segment_prism(V, c, a, hh)
    o["dist"] = -o["depth"] - r if o["inside"] else o["dist"] - r
    o["hit"] = o["dist"] < 0
    return o


def full_sat_depth(V, p0, p1):
    """Penetration depth of the segment into the prism by the separating-axis theorem over all 5 face
    normals and dir x all 9 edges (both signs): min over axes of max n.V - min n.p.  Holds
    hull_origin to a second construction; the test uses it once."""
    V, p0, p1 = np.asarray(V, float), np.asarray(p0, float), np.asarray(p1, float)
    E = [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 3), (1, 4), (2, 5)]
    F = [(0, 1, 2), (3, 5, 4), (0, 3, 4), (1, 4, 5), (2, 5, 3)]
    axes = []
    for i, j, k in F:
        axes.append(np.cross(V[j] - V[i], V[k] - V[i]))
    for i, j in E:
        axes.append(np.cross(p1 - p0, V[j] - V[i]))
    best = np.inf
    for ax in axes:
        l = np.linalg.norm(ax)
        if l < 1e-12 * 1e-2:
            continue
        ax = ax / l
        for s in (ax, -ax):
            best = min(best, (V @ s).max() - min(p0 @ s, p1 @ s))
    return best


# ------------------------------------------------------------------ cylinder x prism
def _frame(a):
    """Two unit vectors that complete a to an orthogonal frame."""
    a = np.asarray(a, float)
    k = int(np.argmin(np.abs(a)))
    u = np.cross(a, np.eye(3)[k])
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    return u, v / np.linalg.norm(v)


def _disc_points(a, hh, rho, K):
    """The 2K corners of the prism over a regular K-gon of circumradius rho, relative to its centre."""
    u, v = _frame(a)
    th = 2 * np.pi * np.arange(K) / K
    ring = rho * (np.cos(th)[:, None] * u + np.sin(th)[:, None] * v)
    return np.concatenate([ring + hh * a, ring - hh * a])


def _polytope_pair(A_rel, a, hh, r, K):
    """hull_origin of A - (K-gon prism) for the inscribed and the circumscribed polygon; A_rel are
    A's vertices relative to the cylinder's centre."""
    out = []
    for rho in (r, r / np.cos(np.pi / K)):
        Q = _disc_points(a, hh, rho, K)
        pts = (A_rel[:, None, :] - Q[None, :, :]).reshape(-1, 3)
        o = hull_origin(pts)
        o["vertex"] = np.unique(o["support"] // len(Q))  # A's vertices in the contact feature
        out.append(o)
    return out


def cylinder_prism(V, c, a, hh, r, K=K_GON):
    """-> dict(lo, hi: the bracket of the depth (None when that polygon is apart), apart_inner,
    apart_outer, normal: n* of the outer polygon (the closest-point direction when it is apart),
    rim_edge, feature: 'cap' / 'side_vertex' / 'other', gap, vertex)."""
    V, c, a = np.asarray(V, float), np.asarray(c, float), np.asarray(a, float)
    inner, outer = _polytope_pair(V - c, a, hh, r, K)
    n = outer["normal"]
    na = abs(n @ a) / np.linalg.norm(a)
    nv = len(outer["vertex"])
    feature = "cap" if na >= 1 - 1e-3 else "side_vertex" if (na <= 1e-3 and nv == 1) else "other"
    return dict(lo=inner["depth"] if inner["inside"] else None, hi=outer["depth"] if outer["inside"] else None,
                apart_inner=not inner["inside"], apart_outer=not outer["inside"], normal=n, gap=outer["gap"],
                rim_edge=bool(1e-3 < na < 1 - 1e-3 and nv >= 2), feature=feature, vertex=outer["vertex"],
                sep=None if outer["inside"] else outer["dist"])


# ------------------------------------------------------------------ sphere x capsule, sphere x cylinder
def sphere_capsule(sc, sr, c, a, hh, r):
    """Point-segment distance: dist = |sc - nearest point of the axis segment| - sr - r."""
    sc, c, a = np.asarray(sc, float), np.asarray(c, float), np.asarray(a, float)
    rel = sc - c
    t = np.clip(rel @ a / (a @ a), -hh, hh)
    w = t * a - rel                     # from the sphere's centre to the segment's nearest point
    d = float(np.linalg.norm(w))
    return dict(dist=d - sr - r, hit=d - sr - r < 0, normal=w / d if d > 0 else None, gap=d, tol=0.0)


def _polish_outside(rel, a, hh, r):
    """min |rel - x| over the cylinder x = z a + rho (cos phi u + sin phi v), |z| <= hh, 0 <= rho <= r,
    with rel the sphere's centre relative to the cylinder's: a grid of starts, L-BFGS-B from the
    best two, then projected Newton steps with the analytic Hessian.  -> (d, x, conv, xerr): xerr = sqrt(2 D) bounds |x - x*| (|.|^2 / 2 is 1-strongly convex), conv bounds
    what is left of d - d_min by the polish's own figure, the projected gradient of |.|^2 / 2 times
    the box's extent (f is convex over the cylinder), through d - d* <= min(sqrt(2 D), 2 D / d, d)."""
    u, v = _frame(a)
    lo = np.array([-hh, 0.0, -np.pi])
    hi = np.array([hh, r, 3 * np.pi])

    def parts(p):
        z, rho, ph = p
        w = np.cos(ph) * u + np.sin(ph) * v
        wp = -np.sin(ph) * u + np.cos(ph) * v
        e = z * a + rho * w - rel
        return e, w, wp

    def fg(p):
        e, w, wp = parts(p)
        return 0.5 * e @ e, np.array([e @ a, e @ w, p[1] * (e @ wp)])

    def pgrad(p, g):  # the gradient's part that the bounds do not hold back
        g = g.copy()
        g[(p <= lo) & (g > 0)] = 0
        g[(p >= hi) & (g < 0)] = 0
        return g

    zs, rs, ps = np.linspace(-hh, hh, 7), np.linspace(r / 3, r, 3), 2 * np.pi * np.arange(12) / 12
    grid = np.array(np.meshgrid(zs, rs, ps, indexing="ij")).reshape(3, -1).T
    x = grid[:, :1] * a + grid[:, 1:2] * (np.cos(grid[:, 2:]) * u + np.sin(grid[:, 2:]) * v) - rel
    vals = np.einsum("ij,ij->i", x, x)
    best = None
    for s in np.argsort(vals)[:2]:
        res = minimize(fg, grid[s], jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                       options=dict(ftol=0.0, gtol=1e-15, maxiter=200))
        p = res.x.copy()
        for _ in range(12):
            f, g = fg(p)
            free = ~(((p <= lo) & (g > 0)) | ((p >= hi) & (g < 0)))
            if not free.any() or np.abs(g[free]).max() < 1e-18:
                break
            e, w, wp = parts(p)
            H = np.array([[a @ a, 0.0, 0.0], [0.0, 1.0, e @ wp], [0.0, e @ wp, p[1] ** 2 - p[1] * (e @ w)]])
            idx = np.nonzero(free)[0]
            try:
                step = np.linalg.solve(H[np.ix_(idx, idx)], -g[idx])
            except np.linalg.LinAlgError:
                break
            q = p.copy()
            q[idx] += step
            q = np.clip(q, lo, hi)
            if np.linalg.norm(pgrad(q, fg(q)[1])) < np.linalg.norm(pgrad(p, g)):
                p = q
            else:
                break
        f, g = fg(p)
        if best is None or f < best[0]:
            best = (f, p, g)
    f, p, g = best
    if p[1] <= 1e-12:  # on the axis the angle's derivative vanishes: stationary only if no angle leads outward
        e = p[0] * a - rel
        assert min(e @ (np.cos(t) * u + np.sin(t) * v) for t in ps) >= -1e-12, "the polish stopped on the axis"
    D = float(np.linalg.norm(pgrad(p, g)) * (2 * hh + r + 2 * np.pi))
    d = float(np.sqrt(2 * f))
    conv = min(np.sqrt(2 * D), 2 * D / d if d > 0 else np.inf, d)  # and d* >= 0
    e, _, _ = parts(p)
    return d, e + rel, float(conv), float(np.sqrt(2 * D))


def sphere_cylinder(sc, sr, c, a, hh, r, K=K_GON):
    """Centre inside the cylinder: the hull bracket with a one-point polytope, -> lo <= depth <= hi and
    dist in [-hi - sr, -lo - sr].  Centre outside: the polished minimum distance d, dist = d - sr
    within tol.  -> dict(inside, dist_lo, dist_hi, hit, normal, gap, tol, side)."""
    sc, c, a = np.asarray(sc, float), np.asarray(c, float), np.asarray(a, float)
    rel = sc - c
    z = rel @ a / np.sqrt(a @ a)
    rho = np.linalg.norm(rel - (rel @ a) * a / (a @ a))
    if abs(z) <= hh and rho <= r:
        inner, outer = _polytope_pair(rel[None, :], a, hh, r, K)
        # the polygon's side normals are good to pi / K only; a cap's is exact
        side = abs(outer["normal"] @ a) < 0.5
        gap = outer["gap"]
        if outer["inside"]:  # wall against caps: the polygon's neighbouring sides are one wall
            eq = outer["eq"]
            wall = np.abs(eq[:, :3] @ a) < 0.5
            gap = abs((-eq[wall, 3]).min() - (-eq[~wall, 3]).min())
            if side:  # and the wall's normal divides by the centre's distance from the axis
                gap = min(gap, rho)
        # a centre within 8.3e-6 of the wall may lie outside the inscribed polygon: the depth is still >= 0
        lo = inner["depth"] if inner["inside"] else 0.0
        hi = outer["depth"] if outer["inside"] else 0.0
        return dict(inside=True, dist_lo=-hi - sr, dist_hi=-lo - sr, hit=True,
                    normal=outer["normal"], gap=float(gap), tol=0.0, xerr=0.0, side=bool(side))
    d, x, conv, xerr = _polish_outside(rel, a, hh, r)
    w = x - rel
    return dict(inside=False, dist_lo=d - sr, dist_hi=d - sr, hit=d - sr < 0, normal=w / d if d > 0 else None,
                gap=d, tol=conv, xerr=xerr, side=False)


# ------------------------------------------------------------------ the case set
def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _prism(rng, flat=None):
    """A prism of the terrain grid: a random cell (half of them from the central 5 m), either triangle
    of it, tops U(0, 0.3) or all 0."""
    ci, ri = rng.integers(0, HF_N - 1, size=2) if rng.random() < 0.5 else rng.integers(73, 219, size=2)
    x0, x1, y0, y1 = CELL * ci - HF_SX, CELL * (ci + 1) - HF_SX, CELL * ri - HF_SX, CELL * (ri + 1) - HF_SX
    xy = [(x0, y0), (x0, y1), (x1, y0)] if rng.random() < 0.5 else [(x0, y1), (x1, y0), (x1, y1)]
    if flat is None:
        flat = rng.random() < 0.3
    z = np.zeros(3) if flat else rng.uniform(0, 0.3, size=3)
    return np.array([[x, y, zz] for (x, y), zz in zip(xy, z)])


def _row(tri, c, a, hh, r):
    return np.concatenate([np.asarray(tri, float).ravel(), [HF_BOTTOM], c, a, [hh, r]])


def prism_halfspaces(V):
    """The prism V[6, 3] as five outward half-spaces [(n, d)]: n.x <= d (top, bottom, three sides)."""
    tri = V[:3]
    faces = []
    nt = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    nt = nt / np.linalg.norm(nt) * (1 if nt[2] > 0 else -1)
    faces.append((nt, nt @ tri[0]))
    faces.append((np.array([0.0, 0.0, -1.0]), -V[3, 2]))
    cen = tri[:, :2].mean(axis=0)
    for i in range(3):
        p, q = tri[i, :2], tri[(i + 1) % 3, :2]
        n2 = np.array([q[1] - p[1], p[0] - q[0]])
        n2 = n2 / np.linalg.norm(n2)
        if n2 @ (cen - p) > 0:
            n2 = -n2
        faces.append((np.array([n2[0], n2[1], 0.0]), n2 @ p))
    return faces


def _route(V, c, a, hh, r):
    """Which of capsule_prism's three regimes a case lies in, from the geometry: 0 a face plane has
    both ends at least r outside it, 1 the segment meets the prism, 2 neither."""
    faces = prism_halfspaces(V)
    p0, p1 = c - hh * a, c + hh * a
    if any(n @ p0 - d >= r and n @ p1 - d >= r for n, d in faces):
        return 0
    return 1 if segment_prism(V, c, a, hh)["inside"] else 2


def _spread(keys):
    """An order in which every key's cases are spread evenly over the whole list."""
    keys = np.asarray(keys)
    pos = np.zeros(len(keys))
    for k in np.unique(keys):
        idx = np.nonzero(keys == k)[0]
        pos[idx] = (np.arange(len(idx)) + 0.5) / len(idx)
    return np.argsort(pos, kind="stable")


_cases = {}


def cases(seed=5):
    """Deterministic inputs: dict of capsule (in[n, 18], route[n], class_a[n], degenerate[n], name[n]),
    cylinder (in[n, 18]), sphere_cylinder and sphere_capsule (in[n, 12], kind[n]).  Built once per
    process and never changed."""
    if seed in _cases:
        return _cases[seed]
    rng = np.random.default_rng(seed)

    # ---- capsules: 1250 plain cases over the three routes, 200 of class A, 48 degenerate
    rows, route, cls_a, degen, names = [], [], [], [], []

    def add(tri, c, a, g, name, A=False, D=False, rt=None):
        V = prism_vertices(tri, HF_BOTTOM)
        rows.append(_row(tri, c, a, g["hh"], g["r"]))
        route.append(_route(V, c, a, g["hh"], g["r"]) if rt is None else rt)
        cls_a.append(A); degen.append(D); names.append(name)

    quota = {0: 300, 1: 500, 2: 450}
    while any(quota.values()):
        tri = _prism(rng)
        g = STICK if rng.random() < 0.5 else WHEEL
        a = _unit(rng)
        cen = tri.mean(axis=0)
        c = cen + np.array([*rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.12, 0.12)])
        if min(c[2] - g["hh"] * a[2], c[2] + g["hh"] * a[2]) <= HF_BOTTOM + 0.03:
            continue  # outside class A: the lower end more than 3 cm above the bottom plane
        rt = _route(prism_vertices(tri, HF_BOTTOM), c, a, g["hh"], g["r"])
        if quota[rt]:
            quota[rt] -= 1
            add(tri, c, a, g, f"plain {'stick' if g is STICK else 'wheel'}", rt=rt)
    quota = {1: 160, 2: 40}
    while any(quota.values()):  # class A: the lower end within 2 cm of the bottom plane
        tri = _prism(rng)
        g = STICK if rng.random() < 0.5 else WHEEL
        a = _unit(rng)
        if a[2] < 0:
            a = -a
        low = np.array([*(tri[:, :2].mean(axis=0) + rng.uniform(-0.03, 0.03, 2)), HF_BOTTOM + rng.uniform(-0.02, 0.02)])
        c = low + g["hh"] * a
        rt = _route(prism_vertices(tri, HF_BOTTOM), c, a, g["hh"], g["r"])
        if quota.get(rt):
            quota[rt] -= 1
            add(tri, c, a, g, f"class A {'stick' if g is STICK else 'wheel'}", A=True, rt=rt)
    for k in range(48):  # degenerate directions and positions
        tri = _prism(rng, flat=(k % 8 >= 6))
        g = STICK if k % 2 else WHEEL
        cen = tri.mean(axis=0)
        kind = k % 4
        if kind == 0:    # parallel to a top edge
            e = tri[(k // 4 + 1) % 3] - tri[(k // 4) % 3]
            a = e / np.linalg.norm(e)
            c = cen + np.array([*rng.uniform(-0.03, 0.03, 2), rng.uniform(-0.03, 0.03)])
            name = "parallel to a top edge"
        elif kind == 1:  # parallel to z
            a = np.array([0.0, 0.0, 1.0])
            c = cen + np.array([*rng.uniform(-0.03, 0.03, 2), rng.uniform(0.0, 0.1)])
            name = "parallel to z"
        elif kind == 2:  # through a top vertex
            a = _unit(rng)
            c = tri[(k // 4) % 3] + rng.uniform(-0.8, 0.8) * g["hh"] * a
            name = "through a vertex"
        else:            # in the plane of the prism's axis-aligned side face
            xs = tri[:, 0]
            x_face = xs[0] if np.sum(xs == xs[0]) == 2 else xs[1]
            a = _unit(rng)
            a[0] = 0.0
            a /= np.linalg.norm(a)
            c = np.array([x_face, cen[1] + rng.uniform(-0.03, 0.03), cen[2] + rng.uniform(-0.05, 0.05)])
            name = "in a face plane"
        if min(c[2] - g["hh"] * a[2], c[2] + g["hh"] * a[2]) <= HF_BOTTOM + 0.03:
            c[2] += 0.1
        add(tri, c, a, g, "degenerate: " + name, D=True)
    order = _spread(route)
    cap = dict(inp=np.array(rows)[order], route=np.array(route)[order], class_a=np.array(cls_a)[order],
               degenerate=np.array(degen)[order], name=[names[i] for i in order])
    for s in range(0, len(order) - 63, 64):  # every wave holds all three routes
        assert len(set(cap["route"][s:s + 64])) == 3

    # ---- the tower cylinder: 80 poses at random axes, a third near-horizontal; the prism up to 0.15 m
    # off the centre line; the cylinder's lowest point between 5 mm above and 30 mm below the prism's
    # top (its mean height).  A generator of its own, so that the seed's choice (by the conditions
    # of bodycon_check.check_case_set, from the reference alone) leaves the other cases alone.
    # rim_edge classes a contact by 1e-3 < |n*.a| < 1 - 1e-3; a two-vertex feature whose normal is
    # oblique by less than that (a rim x edge contact within 2.6 degrees of a cap or of the wall)
    # is neither that class nor exact, and is drawn again: the set holds classified cases only.
    rc = np.random.default_rng([seed, 6])
    rows, refs = [], []
    hh, r = TOWER["hh"], TOWER["r"]
    while len(rows) < 80:
        k = len(rows)
        tri = _prism(rc, flat=k % 8 == 5)
        a = _unit(rc)
        if k % 3 == 0:
            a[2] = rc.uniform(-0.1, 0.1) * np.linalg.norm(a[:2])
            a /= np.linalg.norm(a)
        off = np.cross(a, _unit(rc))
        c = tri.mean(axis=0) - rc.uniform(-hh, hh) * a - off / np.linalg.norm(off) * 0.15 * rc.random()
        c[2] = tri[:, 2].mean() + rc.uniform(-0.03, 0.005) + hh * abs(a[2]) + r * np.sqrt(max(0.0, 1 - a[2] ** 2))
        o = cylinder_prism(prism_vertices(tri, HF_BOTTOM), c, a, hh, r)
        na = abs(o["normal"] @ a)
        if len(o["vertex"]) >= 2 and not o["rim_edge"] and 1e-9 < na < 1 - 1e-9:
            continue
        rows.append(_row(tri, c, a, hh, r))
        refs.append(o)
    cyl = dict(inp=np.array(rows), ref64=refs)

    # ---- the ball against the tower (140) and against a stick (60)
    rows, kinds = [], []
    K6 = ["inside", "beside the wall", "beyond a cap", "beyond the rim", "on the axis", "at the surface"]
    for k in range(140):
        gc, a = rng.uniform(-3, 3, 3), _unit(rng)
        u, v = _frame(a)
        kind = K6[k % 26 - 20] if k % 26 >= 24 else K6[k % 4]  # the two ill-posed kinds: 5 cases each
        hh, r = TOWER["hh"], TOWER["r"]
        ph = rng.uniform(0, 2 * np.pi)
        sg = 1.0 if rng.random() < 0.5 else -1.0
        if kind == "inside":
            z, rho = rng.uniform(-hh, hh), r * np.sqrt(rng.random())
        elif kind == "beside the wall":
            z, rho = rng.uniform(-hh, hh), r + rng.uniform(0, 0.12)
        elif kind == "beyond a cap":
            z, rho = sg * (hh + rng.uniform(0, 0.12)), r * np.sqrt(rng.random())
        elif kind == "beyond the rim":
            z, rho = sg * (hh + rng.uniform(0, 0.1)), r + rng.uniform(0, 0.1)
        elif kind == "on the axis":
            # every other one inside and nearer the wall than a cap: every direction across the axis is as deep
            z, rho = rng.uniform(-0.02, 0.02) if (k // 26) % 2 == 0 else rng.uniform(-hh - 0.12, hh + 0.12), 0.0
        else:  # within 1e-12 of the surface, either side of the wall or of a cap
            s = 1e-12 * (1 if (k // 26) % 2 else -1)
            if (k // 26) % 3:
                z, rho = rng.uniform(-0.8 * hh, 0.8 * hh), r + s
            else:
                z, rho = sg * (hh + s), 0.8 * r * np.sqrt(rng.random())
        sc = gc + z * a + rho * (np.cos(ph) * u + np.sin(ph) * v)
        rows.append(np.concatenate([sc, [BALL_R], gc, a, [hh, r]]))
        kinds.append(kind)
    sph_cyl = dict(inp=np.array(rows), kind=kinds)
    rows, kinds = [], []
    for k in range(60):
        gc, a = rng.uniform(-3, 3, 3), _unit(rng)
        u, v = _frame(a)
        hh, r = STICK["hh"], STICK["r"]
        ph = rng.uniform(0, 2 * np.pi)
        t = rng.uniform(-1.6 * hh, 1.6 * hh)
        if k % 15 == 13:
            rho, kind = 0.0, "on the axis"
        elif k % 15 == 14:
            t = rng.uniform(-hh, hh)
            rho, kind = BALL_R + r + 1e-12 * (1 if (k // 15) % 2 else -1), "at the surface"
        else:
            rho, kind = rng.uniform(0.0, 0.16), "around"
        sc = gc + t * a + rho * (np.cos(ph) * u + np.sin(ph) * v)
        rows.append(np.concatenate([sc, [BALL_R], gc, a, [hh, r]]))
        kinds.append(kind)
    sph_cap = dict(inp=np.array(rows), kind=kinds)
    _cases[seed] = dict(capsule=cap, cylinder=cyl, sphere_cylinder=sph_cyl, sphere_capsule=sph_cap)
    return _cases[seed]


def rounded(inp, prec):
    """The inputs as the precision holds them, as doubles: what the kernel sees and the reference gets."""
    return inp if prec == "fp64" else inp.astype(np.float32).astype(np.float64)


_refs = {}


def references(prec, seed=5):
    """The reference's answer for every case at a precision's inputs: computed once, shared, unchanged."""
    key = (prec, seed)
    if key in _refs:
        return _refs[key]
    cs = cases(seed)
    out = {}
    x = rounded(cs["capsule"]["inp"], prec)
    out["capsule"] = [capsule_prism(prism_vertices(r[:9].reshape(3, 3), r[9]), r[10:13], r[13:16], r[16], r[17]) for r in x]
    x = rounded(cs["cylinder"]["inp"], prec)
    out["cylinder"] = cs["cylinder"]["ref64"] if prec == "fp64" else [
        cylinder_prism(prism_vertices(r[:9].reshape(3, 3), r[9]), r[10:13], r[13:16], r[16], r[17]) for r in x]
    x = rounded(cs["sphere_cylinder"]["inp"], prec)
    out["sphere_cylinder"] = [sphere_cylinder(r[:3], r[3], r[4:7], r[7:10], r[10], r[11]) for r in x]
    x = rounded(cs["sphere_capsule"]["inp"], prec)
    out["sphere_capsule"] = [sphere_capsule(r[:3], r[3], r[4:7], r[7:10], r[10], r[11]) for r in x]
    _refs[key] = out
    return out
