"""Independent fp64 reference of the ball x heightfield contact list (numpy only).

A heightfield prism is convex: five half-spaces n.x <= d (the top plane through its three
vertices, the bottom plane z = zb, three vertical side planes).  The sphere's penetration into it
is written from that alone:

  centre inside all five   depth = the smallest plane depth, normal = that plane's,
                           dist = -depth - r
  centre outside           x = the Euclidean projection of the centre onto the polytope, found by
                           active-set enumeration (every subset of at most 3 of the 5 planes, the
                           nearest feasible stationary point); contact iff d = |c - x| <= r,
                           normal = (c - x) / d, dist = d - r

This is not the product's or the oracle's form (closest point over the prism's 8 boundary
triangles), which share one closed form from one hand; it pins both.

Geometry constants, stated once (ballbot.xml): the ball's sphere has radius 0.09 and sits at
(0, 0, -0.14) in the ball body's frame; the heightfield is 293 x 293 over a half-extent of
5 x 5 m with a base of 0.1 m below z = 0.
"""
from itertools import combinations

import numpy as np

BALL_R = 0.09
BALL_DZ = -0.14
HF_N = 293
HF_SX = HF_SY = 5.0
HF_BASE = 0.1
MAXG = 50  # contacts kept per geom pair (MuJoCo's mjMAXCONPAIR); the caller applies it

_SUBSETS = [s for k in (1, 2, 3) for s in combinations(range(5), k)]  # 5 + 10 + 10 = 25
_FEAS_TOL = 1e-12  # a stationary point this far outside an inactive plane still counts as feasible:
#                    it moves the distance by its square over 2 d, far below 1e-15


def prism_planes(V, zb):
    """V[..., 3, 3]: the top vertices, relative to any origin; zb: the bottom's z in the same frame.
    Returns the outward unit normals A[..., 5, 3] and offsets b[..., 5] of n.x <= b."""
    V = np.asarray(V, np.float64)
    A = np.zeros(V.shape[:-2] + (5, 3))
    b = np.zeros(V.shape[:-2] + (5,))
    nt = np.cross(V[..., 1, :] - V[..., 0, :], V[..., 2, :] - V[..., 0, :])
    nt = nt * np.where(nt[..., 2:3] < 0, -1.0, 1.0)
    nt = nt / np.linalg.norm(nt, axis=-1, keepdims=True)
    A[..., 0, :] = nt
    b[..., 0] = np.sum(nt * V[..., 0, :], axis=-1)
    A[..., 1, 2] = -1.0
    b[..., 1] = -np.asarray(zb, np.float64)
    for i in range(3):
        P, Q, O = V[..., i, :], V[..., (i + 1) % 3, :], V[..., (i + 2) % 3, :]
        n = np.stack([Q[..., 1] - P[..., 1], P[..., 0] - Q[..., 0]], axis=-1)  # perpendicular to the edge, in xy
        n = n / np.linalg.norm(n, axis=-1, keepdims=True)
        side = np.sum(n * (O[..., :2] - P[..., :2]), axis=-1)
        n = n * np.where(side > 0, -1.0, 1.0)[..., None]  # away from the opposite vertex
        A[..., 2 + i, :2] = n
        b[..., 2 + i] = np.sum(n * P[..., :2], axis=-1)
    return A, b


def _project_origin(A, b):
    """The point of {x : A x <= b} nearest to the origin, for a batch: A[N, 5, 3], b[N, 5] -> x[N, 3].
    The projection is the stationary point of its own active set, and every feasible stationary
    point is at least as far, so the nearest feasible one over all active sets is the projection."""
    N = A.shape[0]
    best = np.full(N, np.inf)
    xbest = np.zeros((N, 3))
    for S in _SUBSETS:
        As, bs = A[:, S, :], b[:, S]  # min |x|^2 with As x = bs: x = As' (As As')^-1 bs
        G = As @ np.swapaxes(As, 1, 2)
        ok = np.abs(np.linalg.det(G)) > 1e-12  # parallel or dependent planes share no stationary point
        G = np.where(ok[:, None, None], G, np.eye(len(S)))
        lam = np.linalg.solve(G, bs[:, :, None])
        x = (np.swapaxes(As, 1, 2) @ lam)[:, :, 0]
        feas = ok & np.all(np.einsum("nij,nj->ni", A, x) <= b + _FEAS_TOL, axis=1)
        d2 = np.sum(x * x, axis=1)
        take = feas & (d2 < best)
        best = np.where(take, d2, best)
        xbest = np.where(take[:, None], x, xbest)
    assert np.all(np.isfinite(best)), "a prism without a feasible stationary point"
    return xbest


def sphere_prisms_ref(c, V, zb, r):
    """Batched sphere_prism_ref: V[N, 3, 3], c[3] or c[N, 3].  Returns hit[N], dist[N], normal[N, 3],
    margin[N] and gap[N]: |d - r| for the prisms whose decision is a distance test (centre outside),
    inf inside."""
    V = np.asarray(V, np.float64).reshape(-1, 3, 3)
    N = V.shape[0]
    c = np.broadcast_to(np.asarray(c, np.float64), (N, 3))
    A, b = prism_planes(V - c[:, None, :], zb - c[:, 2])  # the centre is the origin: depths are b itself
    inside = np.all(b >= 0, axis=1)
    order = np.argsort(b, axis=1, kind="stable")
    rows = np.arange(N)
    d0, d1 = b[rows, order[:, 0]], b[rows, order[:, 1]]
    n_in = A[rows, order[:, 0], :]
    x = _project_origin(A, b)
    d = np.linalg.norm(x, axis=1)
    n_out = -x / np.where(d > 0, d, 1.0)[:, None]
    hit = inside | (d <= r)
    dist = np.where(inside, -d0 - r, d - r)
    normal = np.where(inside[:, None], n_in, n_out)
    margin = np.where(inside, np.minimum(d0, d1 - d0), d)
    gap = np.where(inside, np.inf, np.abs(d - r))
    return hit, dist, normal, margin, gap


def sphere_prism_ref(c, V, zb, r):
    """One prism: None (no contact) or (dist, normal, margin).  margin says how well-posed the
    normal is: outside, the distance d it is divided by; inside, the smaller of the minimum depth
    and the gap between the two smallest depths (the face choice flips when that gap closes)."""
    hit, dist, normal, margin, _ = sphere_prisms_ref(c, np.asarray(V)[None], zb, r)
    return (float(dist[0]), normal[0], float(margin[0])) if hit[0] else None


def _prisms_under(c, H, size_z, r):
    """Top vertices V[n, 3, 3] of the prisms MuJoCo's mjc_ConvexHField visits for a sphere at c, in its
    order: the sub-grid under the sphere's bounding box (same floor / ceil and clamping to
    [0, 292]), rows rmin..rmax-1, columns cmin..cmax, two prisms per cell in sliding-window order."""
    lo, hi = c - r, c + r
    if (lo[0] > HF_SX or hi[0] < -HF_SX or lo[1] > HF_SY or hi[1] < -HF_SY or lo[2] > size_z
            or hi[2] < -HF_BASE):
        return np.zeros((0, 3, 3))
    N1 = HF_N - 1
    cmin = max(int(np.floor((lo[0] + HF_SX) / (2 * HF_SX) * N1)), 0)
    cmax = min(int(np.ceil((hi[0] + HF_SX) / (2 * HF_SX) * N1)), N1)
    rmin = max(int(np.floor((lo[1] + HF_SY) / (2 * HF_SY) * N1)), 0)
    rmax = min(int(np.ceil((hi[1] + HF_SY) / (2 * HF_SY) * N1)), N1)
    npr = 2 * (cmax - cmin + 1) - 2
    if rmax <= rmin or npr <= 0:
        return np.zeros((0, 3, 3))
    dx, dy = 2 * HF_SX / N1, 2 * HF_SY / N1
    rr, p, t = np.meshgrid(np.arange(rmin, rmax), np.arange(npr), np.arange(3), indexing="ij")
    vt = p + t  # the window's vertex t of prism p: column cmin + vt // 2, row rr + vt % 2
    cc, ri = cmin + vt // 2, rr + vt % 2
    V = np.stack([dx * cc - HF_SX, dy * ri - HF_SY, H[ri, cc].astype(np.float64) * size_z], axis=-1)
    return V.reshape(-1, 3, 3)


def collide_ref_many(cs, hf, size_z, r=BALL_R):
    """collide_ref for every centre of cs[n, 3] on one field, the prisms of all cases in one batch."""
    cs = np.asarray(cs, np.float64).reshape(-1, 3)
    H = np.asarray(hf, np.float32).reshape(HF_N, HF_N)
    Vs = [_prisms_under(c, H, size_z, r) for c in cs]
    cnt = [len(V) for V in Vs]
    out = []
    if sum(cnt):
        call = np.repeat(cs, cnt, axis=0)
        hit, dist, normal, margin, gap = sphere_prisms_ref(call, np.concatenate(Vs), -HF_BASE, r)
    o = 0
    for n in cnt:
        if n == 0:
            out.append(dict(dist=np.zeros(0), normal=np.zeros((0, 3)), margin=np.zeros(0), flip=np.inf,
                            gaps=np.zeros(0)))
            continue
        s, h = slice(o, o + n), hit[o:o + n]
        out.append(dict(dist=dist[s][h], normal=normal[s][h], margin=margin[s][h], flip=float(gap[s].min()),
                        gaps=gap[s]))
        o += n
    return out


def collide_ref(c, hf, size_z, r=BALL_R):
    """The whole ball x heightfield contact list at sphere centre c, in MuJoCo's order and uncapped
    (the caller applies the cap of MAXG): one contact per penetrated prism.  MuJoCo's "all three
    vertices below the sphere" skip is left out: such a prism lies wholly below the sphere, so the
    skip is a geometric no-op.

    Returns dict(dist[n], normal[n, 3], margin[n], flip, gaps); gaps holds |d - r| of every prism and flip is the smallest |d - r| over the
    prisms whose centre test is a distance test: how near any contact decision is to flipping."""
    return collide_ref_many(np.asarray(c, np.float64)[None], hf, size_z, r)[0]


# ------------------------------------------------------------------ the case set of the tests
DZ = (0.0895, 0.089, 0.085, 0.08, 0.07, 0.06, 0.04, 0.02, -0.01, -0.05, -0.12)  # centre above the nearest vertex
PLACEMENTS = ("vertex", "edge", "diagonal", "interior", "field_edge", "corner")
_cases = None


def terrains():
    """(name, heights float32[293 * 293], size_z) of the five fields of the case set."""
    from ballbot_gym.terrain import generate_hills_terrain
    from ballbot_gym.terrain.stepped import generate_stepped_terrain
    from ballbot_gym.terrain.terraced import generate_terraced_terrain

    n = HF_N
    return [("flat", np.zeros(n * n, np.float32), 2.0),
            ("hills7", generate_hills_terrain(n, seed=7).astype(np.float32), 2.0),
            ("stepped3", generate_stepped_terrain(n, seed=3).astype(np.float32), 2.0),
            ("terraced3", generate_terraced_terrain(n, seed=3).astype(np.float32), 2.0),
            ("ones", np.ones(n * n, np.float32), 2.0)]  # the top of the field's range


def _place(rng, kind, rep):
    """Lateral position of one case.  The three "over a line" placements sit exactly on the line when
    rep is even and 1e-5 m off it when rep is odd, where their normals are well-posed."""
    dx, dy = 2 * HF_SX / (HF_N - 1), 2 * HF_SY / (HF_N - 1)
    cc, rr = rng.integers(3, 289, 2)
    x0, y0 = dx * cc - HF_SX, dy * rr - HF_SY
    u = rng.uniform(0.1, 0.9)
    off = 1e-5 * np.array([0.6, 0.8]) if rep % 2 else np.zeros(2)  # parallel to no edge and not to the diagonal
    if kind == "vertex":  # shared by six prisms
        return np.array([x0, y0]) + off
    if kind == "edge":
        return (np.array([x0 + u * dx, y0]) if rng.integers(2) else np.array([x0, y0 + u * dy])) + off
    if kind == "diagonal":  # from vertex (cc, rr + 1) to (cc + 1, rr)
        return np.array([x0 + u * dx, y0 + (1 - u) * dy]) + off
    if kind == "interior":
        return np.array([x0 + rng.uniform(0, dx), y0 + rng.uniform(0, dy)])
    sgn = rng.choice([-1.0, 1.0], 2)
    if kind == "field_edge":  # up to 0.12 m inside or outside one edge of the field
        p = np.array([sgn[0] * HF_SX + rng.uniform(-0.12, 0.12), rng.uniform(-4.8, 4.8)])
        return p if rng.integers(2) else p[::-1].copy()
    assert kind == "corner"
    return sgn * HF_SX + rng.uniform(-0.1, 0.1, 2)


def ball_qpos(c):
    """qpos[17] with the ball's sphere centred at c (identity orientation) and the base lifted clear
    of everything, so that only ball x heightfield contacts exist."""
    q = np.zeros(17)
    q[2], q[3], q[13] = 6.0, 1.0, 1.0
    q[10:13] = np.asarray(c, np.float64) - np.array([0.0, 0.0, BALL_DZ])
    return q


def ball_cases():
    """The case set, built once per process and never changed: per terrain a dict(name, hf, size_z,
    q[n, 17], c[n, 3], kind[n], ref[n]) of 132 cases (6 placements x 11 heights x 2)."""
    global _cases
    if _cases is None:
        out = []
        for ti, (name, hf, size_z) in enumerate(terrains()):
            rng = np.random.default_rng(1000 + ti)
            H = hf.reshape(HF_N, HF_N)
            qs, kinds = [], []
            for kind in PLACEMENTS:
                for dz in DZ:
                    for rep in range(2):
                        xy = _place(rng, kind, rep)
                        ij = np.clip(np.rint((xy + HF_SX) / (2 * HF_SX) * (HF_N - 1)).astype(int), 0, HF_N - 1)
                        z = float(H[ij[1], ij[0]]) * size_z + dz
                        qs.append(ball_qpos([xy[0], xy[1], z]))
                        kinds.append(kind)
            q = np.array(qs)
            c = q[:, 10:13] + np.array([0.0, 0.0, BALL_DZ])  # as the kinematics forms it
            out.append(dict(name=name, hf=hf, size_z=size_z, q=q, c=c, kind=kinds,
                            ref=collide_ref_many(c, hf, size_z)))
        _cases = out
    return _cases


# ------------------------------------------------------------------ comparing a list with the reference
# Bounds from the formats, not from any implementation (eps: the type's machine epsilon, 5.1 m: the
# largest coordinate magnitude): dist 16 eps 5.1; normal, where the reference's margin is at least
# the floor, 16 eps 5.1 / floor; a case is dropped for a precision when the reference puts any
# prism within `flip` of touching (the decision itself is then rounding).
BOUNDS = {"fp64": dict(dist=16 * 2.220446049250313e-16 * 5.1, floor=1e-6, flip=1e-9),
          "fp32": dict(dist=16 * 1.1920929e-7 * 5.1, floor=1e-3, flip=1e-5)}
for _b in BOUNDS.values():
    _b["normal"] = _b["dist"] / _b["floor"]
MAX_DROPPED = 0.05  # of the cases


class Tally:
    """Worst figures and counts of one run over the case set."""

    def __init__(self, prec):
        self.prec, self.b = prec, BOUNDS[prec]
        self.cases = self.contacts = self.dropped = self.dist_only = 0
        self.worst_dist = self.worst_normal = 0.0

    def check(self, ref, g, overflow, what):
        """g[ng, 4] (normal, dist per slot) and the overflow flag of one case against its reference
        list: count, order and flag exactly, dist on every contact, the normal where it is well-posed."""
        b = self.b
        self.cases += 1
        n = len(ref["dist"])
        near = int(np.sum(ref["gaps"] < b["flip"]))
        if near:  # some decision is rounding: the count may be off by that many, nothing else is held
            self.dropped += 1
            assert abs(len(g) - min(n, MAXG)) <= near, f"{what}: {len(g)} contacts, reference {n} (+-{near})"
            return
        assert len(g) == min(n, MAXG), f"{what}: {len(g)} contacts, reference {n}"
        assert bool(overflow) == (n > MAXG), f"{what}: overflow {overflow}, reference has {n} contacts"
        for s in range(len(g)):
            ed = abs(g[s, 3] - ref["dist"][s])
            self.worst_dist = max(self.worst_dist, ed)
            assert ed <= b["dist"], f"{what} slot {s}: dist {g[s, 3]!r} vs {ref['dist'][s]!r} ({ed:.2e})"
            if ref["margin"][s] >= b["floor"]:
                en = np.abs(g[s, :3] - ref["normal"][s]).max()
                self.worst_normal = max(self.worst_normal, en)
                assert en <= b["normal"], (f"{what} slot {s}: normal {g[s, :3]} vs {ref['normal'][s]} ({en:.2e}, "
                                           f"margin {ref['margin'][s]:.2e})")
            else:
                self.dist_only += 1
        self.contacts += len(g)

    def finish(self, what):
        print(f"\n{what} [{self.prec}]: {self.cases} cases, {self.contacts} contacts, worst dist "
              f"{self.worst_dist:.2e} (bound {self.b['dist']:.1e}), worst normal {self.worst_normal:.2e} "
              f"(bound {self.b['normal']:.1e}), {self.dist_only} contacts held to dist only, "
              f"{self.dropped} cases dropped")
        assert self.dropped <= MAX_DROPPED * self.cases, f"{self.dropped} of {self.cases} cases dropped"


def census(cases):
    """Counts of the case set by reference list length, and of centres outside the field with contacts."""
    n = np.array([len(r["dist"]) for t in cases for r in t["ref"]])
    c = np.concatenate([t["c"] for t in cases])
    outside = (np.abs(c[:, 0]) > HF_SX) | (np.abs(c[:, 1]) > HF_SY)
    return {"0": int((n == 0).sum()), "1-12": int(((n >= 1) & (n <= 12)).sum()),
            "13-49": int(((n >= 13) & (n < MAXG)).sum()), "capped": int((n >= MAXG).sum()),
            "overflow": int((n > MAXG).sum()), "outside with contacts": int((outside & (n > 0)).sum())}
