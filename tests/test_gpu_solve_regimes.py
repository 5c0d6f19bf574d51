"""The constraint solve of both step-kernel forms at qacc level, on directed states that cover the solver's regimes.

bb_forward launches the full kernel's solve16<BODY=true>; the fast kernels' solve16<false, FUSE> (Jacobians of the
first GC_LDS = 13 ground contacts in LDS, the jar0 shortcut of the line search, the DPP-fused sweeps) runs only
under bb_step, where the suite held it to qpos 1e-9 / qvel 1e-6 after RK4: with h = 0.002 that lets through a
qacc error of ~5e-4.  The warm start a step leaves behind is the last RK stage's solved qacc, so comparing it with
the oracle's holds the fast form to the forward tests' 1e-7 (relative to max(1, max|warm|)).

States: built here on the CPU with the oracle alone, from seeds; nothing is read from a file.  They start from
tests/test_gpu_solve_fused.py's fall / rest / slip states and vary: the whole robot moved +4 .. -35 mm vertically on
flat ground and on hills (seed 7) at random places (the depth scanned for exact ball-terrain contact counts);
velocity scales {0, 1e-5, 1e-3, 0.05, 0.5}; action scales {0, 0.01, 1}; the base raised off the ball; the base
leaving the ball or rocking on it (wheel contacts that carry no force); the ball alone pressed 45 .. 80 mm in (the cap
of 50 contacts); the ball turning under a slowly turning base (sticking wheels, searched with the oracle's forward:
a wheel sticks only where it needs under 0.001 of its load along its axis, ~1 near-rest state in 25).  Only states
without a base-tree contact are kept (the fast kernel's envs).  A state is dropped where the oracle's own stop is
ambiguous: its default solver and (100 iterations, tolerance 1e-12) leave warm starts more than 1e-8 apart after
one env step; at most 2% may go.

Census (oracle's forward at the state: cone zone of every contact at the solution, contact count, Newton
iterations) and, per cell, the worst warm-start error after one env step against the oracle, relative: the host
build of the solver templates (CPU) and the fast kernels on an MI355X.  307 states built, 1 dropped, 306 kept
(154 flat, 152 hills).  Every cell needs 4 states, the open ranges of counts 1.

  cell                                       states   host build   MI355X
  wheels: all three sliding                     176     3.8e-08    3.8e-08
  wheels: one or more sticking                   34     6.0e-09    6.0e-09
  wheels: inactive next to active                13     6.5e-10    6.5e-10
  wheels: all three inactive                     10     2.0e-08    2.0e-08
  wheels: no contact                             36     8.2e-09    8.2e-09
  ground: ng = 0                                 29     3.8e-08    3.8e-08
  ground: all active sticking                    47     6.2e-09    6.2e-09
  ground: one or more sliding                   230     2.0e-08    2.0e-08
  ground: inactive next to active               192     2.0e-08    2.0e-08
  ng = 1                                          7     4.5e-10    4.5e-10
  ng = 13                                        11     5.3e-09    5.3e-09
  ng = 14                                        12     1.6e-09    1.6e-09
  ng = 29                                        13     3.1e-11    3.1e-11
  ng = 30                                        25     1.6e-09    1.6e-09
  ng = 46                                        10     5.5e-11    5.5e-11
  ng = 50 (capped, ground_overflow set)          10     2.6e-10    2.6e-10
  ng 2..12                                       70     2.0e-08    2.0e-08
  ng 15..28                                      49     6.8e-10    6.8e-10
  ng 31..45                                      68     1.0e-09    1.0e-09
  ng 47..49                                       2     3.2e-14    2.8e-14
  crossed: wheel sticking, ground sliding        12     4.2e-10    4.2e-10
  crossed: ng >= 14, a wheel inactive             7     1.0e-09    1.0e-09
  niter 0                                        13     6.3e-16    2.3e-15
  niter 1                                        10     1.8e-10    1.8e-10
  niter >= 12                                    40     6.0e-09    6.0e-09

ng = 13 | 14, 29 | 30, 45 | 46 are where a lane of solve16's 16-lane team picks up its 2nd, 3rd and 4th contact
(c = tl, tl + 16, ... over 3 + ng), and 13 | 14 also where a contact's Jacobian is kept in LDS or rebuilt.  No cell
was out of the search's reach; ng = 45 itself never appeared (31..44 and 46 did), and 47..49 are two states, kept
at rest so that no RK stage reaches the cap.  Worst of the 306 fast-kernel steps on the MI355X: qpos 1.5e-12, qvel
2.6e-9, obs 1.9e-9, reward 0, warm 3.8e-8; none outside the bounds, slow_path unmoved.

The full kernel's forward on the same states (test B): qacc within 8.0e-8 on flat (one state, ng = 13, where the
oracle's own default and 1e-12 forwards are 8.0e-8 apart; the next is 9.1e-10) and 2.4e-8 on hills.  Before the
solver's improvement stop was guarded (IMPR_GRAD, bb_physics.h) one hills state of 152 missed the bound at 1.07e-7:
a cold-start forward of a pressed ball (wheels sliding, 6 ground contacts sticking, max|qacc| 55) whose Newton loop
left after 8 iterations on MuJoCo's improvement test (scaled cost decrease 1.7e-9 < 1e-8) from a point whose scaled
gradient was still 3e-2, 1.07e-7 from the minimiser; the host build gave the same figure.  With the one further
iteration the guard allows, it ends 4e-12 away.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

Q_TOL, V_TOL, OBS_TOL, R_TOL, QACC_TOL = 1e-9, 1e-6, 1e-6, 1e-7, 1e-7
AMBIG_TOL, MAX_DROP_FRAC = 1e-8, 0.02
MIN_PER_CELL = 4
V_SCALES = (0.0, 1e-5, 1e-3, 0.05, 0.5)
A_SCALES = (0.0, 0.01, 1.0)
NG_EXACT = (1, 13, 14, 29, 30, 46, 50)
NG_RANGES = ((2, 12), (15, 28), (31, 45), (47, 49))
TERRAINS = ("flat", "hills")
HILLS_SEED = 7
N_RANDOM = 80  # per terrain


def _relerr(a, ref):
    return np.abs(a - ref).max(axis=-1) / np.maximum(1.0, np.abs(ref).max(axis=-1))


def _hfield(O, terrain):
    if terrain == "flat":
        return O.flat_hfield()
    from ballbot_gym.terrain import generate_hills_terrain

    return generate_hills_terrain(293, seed=HILLS_SEED).astype(np.float32)


def _terrain_cfg(terrain):
    return {"type": "flat", "config": {}} if terrain == "flat" else {"type": "hills", "config": {"seed": HILLS_SEED}}


def _placed(q, hf, x, y, dz, ball_only=False):
    """q moved by (x, y) and set on the terrain there: the height of the vertex nearest the ball's
    centre, plus dz (negative: pressed in).  ball_only: the base goes 1 m up instead, off the ball."""
    q = q.copy()
    q[[0, 10]] += x
    q[[1, 11]] += y
    r, c = int(round((q[11] + 5) / 10 * 292)), int(round((q[10] + 5) / 10 * 292))
    top = float(hf.reshape(293, 293)[r, c]) * 2.0
    q[12] += top + dz
    q[2] += top + (1.0 if ball_only else dz)
    return q


def _rot(quat):
    w, x, y, z = quat
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _yaw(q, om_base, om_ball):
    """qvel of the base turning at om_base and the ball at om_ball (rad/s) about the vertical through the ball's
    centre (free joints: linear velocity in the world frame, angular velocity in the body's)."""
    v = np.zeros(15)
    v[0:3] = np.cross([0, 0, om_base], q[0:3] - q[10:13])
    v[3:6] = _rot(q[3:7]).T @ [0, 0, om_base]
    v[12:15] = _rot(q[13:17]).T @ [0, 0, om_ball]
    return v


def _ctrl(action):
    """The env step's ctrl of an action (float32 product and clip, negated)."""
    return -np.clip(np.asarray(action, np.float32) * np.float32(10.0), -10, 10).astype(np.float64)


def _candidates(O, terrain, seed):
    """(qpos, qvel, warm, action) candidates on one terrain, in a fixed order from the seed."""
    from test_gpu_solve_fused import build_states

    hf, cfg = _hfield(O, terrain), O.default_cfg()
    rng = np.random.default_rng(seed)
    base = {name: (q, v, w) for name, q, v, w in build_states(O)}
    rq, rv, rw = base["rest"]
    out = []

    def xy():
        return rng.uniform(-1, 1, 2)

    def action(scale=None):
        s = A_SCALES[rng.integers(len(A_SCALES))] if scale is None else scale
        return (rng.uniform(-1, 1, 3) * s).astype(np.float32)

    def vel(scale=None):
        s = V_SCALES[rng.integers(len(V_SCALES))] if scale is None else scale
        return rng.normal(0, 1, 15) * s

    # 1. exact ball-terrain contact counts: the resting robot pressed in at a random place, the depth scanned
    #    in 0.25 mm steps for the middle of each count's range of depths
    want = {k: MIN_PER_CELL + 1 for k in NG_EXACT[:-1]}
    want.update({k: 1 for k in range(47, 50)})
    dzs = np.arange(2.0, -35.01, -0.25) * 1e-3
    for i in range(80):
        if not any(want.values()):
            break
        if i == 16:  # what is still missing are the counts of the deepest 5 mm
            dzs = dzs[dzs < -30e-3 + 1e-9]
        x, y = xy()
        ng = np.array([O.forward(_placed(rq, hf, x, y, dz), rv, np.zeros(3), rw, hf).nground for dz in dzs])
        for k in want:
            hit = np.nonzero(ng == k)[0]
            if want[k] and len(hit):
                want[k] -= 1
                # 47..49 sit next to the cap: at rest, so that no RK stage reaches it
                v = np.zeros(15) if k >= 47 else vel()
                out.append((_placed(rq, hf, x, y, dzs[hit[len(hit) // 2]]), v, rw.copy(), action()))
    # 2. the cap: the ball alone pressed 45 to 80 mm in (more than 50 prisms), the base held 1 m above it
    for _ in range(MIN_PER_CELL + 1):
        x, y = xy()
        out.append((_placed(rq, hf, x, y, -rng.uniform(0.045, 0.08), ball_only=True), vel(0.05), np.zeros(15),
                    action()))
    # 3. no contact at all (no Newton iteration): the fall state with the base lifted 5 cm off the ball
    fq = base["fall"][0]
    for i in range(3):
        x, y = xy()
        q = _placed(fq, hf, x, y, 0.0)
        q[2] += 0.05
        out.append((q, vel(V_SCALES[i]), np.zeros(15), action()))
    # 4. a robot settled on this terrain going on from its own warm start (one Newton iteration)
    if terrain == "flat":
        q, v, w = rq.copy(), rv.copy(), rw.copy()
    else:
        q, v, w = O.reset_state(O.init_offset(hf))
        for _ in range(400):
            O.env_step(cfg, q, v, w, np.zeros(1, np.int32), np.zeros(3, np.float32), hf)
    for i in range(MIN_PER_CELL + 1):
        O.env_step(cfg, q, v, w, np.zeros(1, np.int32), np.zeros(3, np.float32), hf)
        out.append((q.copy(), v.copy(), w.copy(), np.zeros(3, np.float32)))
    # 5. wheel contacts that carry no force: the base leaving the ball (pull) or turning about a horizontal
    #    axis (rock), resting lightly and pressed deep (there the ball is thrown up against the wheels)
    for i in range(20):
        deep = i % 2 == 1
        x, y = xy()
        q = _placed(rq, hf, x, y, rng.uniform(-30e-3, -14e-3) if deep else rng.uniform(-2e-3, 4e-3))
        v = vel(V_SCALES[i % 4])
        if i % 4 < 2:
            v[2] += rng.uniform(0.8, 1.6) if deep else rng.uniform(0.3, 0.8)
        else:
            a = rng.uniform(0, 2 * np.pi)
            v[3:6] += rng.uniform(1.0, 4.0) * (4 if deep else 1) * np.array([np.cos(a), np.sin(a), 0.0])
        out.append((q, v, rw.copy() if i % 3 else np.zeros(15), action()))
    # 6. sticking wheels.  A wheel contact's friction is 1.0 along the wheel's rolling direction and 0.001 along
    #    its axis (the rollers), so it sticks only where the axial force it needs is under a thousandth of its
    #    load: about one near-rest state in twenty-five.  The settled robot turning slowly about the vertical
    #    through the ball's centre, the ball turning under it (fast: the ball slides on the ground), no action;
    #    searched with the oracle's forward for a sticking wheel, half of them with a sliding ground contact.
    found = {False: 0, True: 0}
    for _ in range(1500):
        if min(found.values()) >= MIN_PER_CELL + 2:
            break
        x, y = xy()
        q = _placed(rq, hf, x, y, rng.uniform(-1e-3, 0.5e-3))
        v = _yaw(q, rng.uniform(0, 3), rng.uniform(5, 30))
        fo = O.forward(q, v, np.zeros(3), rw, hf)
        zw = [fo.con_zone[k] for k in range(fo.ncon) if fo.con_body1[k] == 7]
        zg = [fo.con_zone[k] for k in range(fo.ncon) if fo.con_body1[k] == 0]
        if 2 in zw and found[1 in zg] < MIN_PER_CELL + 2:
            found[1 in zg] += 1
            out.append((q, v, rw.copy(), np.zeros(3, np.float32)))
    # 7. the mix
    for i in range(N_RANDOM):
        kind = rng.choice(["rest", "slip", "fall", "glide"], p=[0.55, 0.25, 0.05, 0.15])
        x, y = xy()
        dz = rng.uniform(-35e-3, 4e-3)
        q0, v0, w0 = base["rest" if kind == "glide" else kind]
        q = _placed(q0, hf, x, y, 0.0 if kind == "fall" else dz)
        v = vel()
        if kind == "slip":
            v[6:9] += v0[6:9] * rng.choice([0.0, 0.1, 1.0])
        if kind == "glide":  # the robot and its ball translating as one body: nothing moves against the wheels
            a = rng.uniform(0, 2 * np.pi)
            u = rng.choice([0.02, 0.1, 0.3, 1.0]) * np.array([np.cos(a), np.sin(a), 0])
            v = vel(rng.choice([0.0, 1e-5, 1e-3]))
            v[0:3] += u
            v[9:12] += u
        mod = rng.choice(["none", "raise", "off"], p=[0.7, 0.15, 0.15])
        if mod == "raise":  # the wheels' 2.3 mm of penetration partly or wholly taken away
            q[2] += rng.uniform(0.5e-3, 3e-3)
        elif mod == "off":
            q[2] += 0.05
        w = w0.copy() if rng.random() < 0.5 else np.zeros(15)
        out.append((q, v, w, action()))
    return out


def _evaluate(O, terrain, cands):
    """The oracle on every candidate: forward at the state (zones, counts, iterations), one env step with the
    default solver and one with (100 iterations, 1e-12).  Keeps the fast kernel's envs (no base-tree contact)."""
    hf, cfg = _hfield(O, terrain), O.default_cfg()
    keep = []
    for q, v, w, a in cands:
        fo = O.forward(q, v, _ctrl(a), w, hf)
        if fo.nbody:
            continue
        rec = dict(q=q, v=v, w=w, a=a, ng=fo.nground, niter=fo.niter, over=fo.ground_overflow & 1,
                   qacc=np.array(fo.qacc), ncon=fo.ncon,
                   zw=[fo.con_zone[k] for k in range(fo.ncon) if fo.con_body1[k] == 7],
                   zg=[fo.con_zone[k] for k in range(fo.ncon) if fo.con_body1[k] == 0])
        res = []
        try:
            for solver in (None, (100, 1e-12)):
                if solver:
                    O.set_solver(*solver)
                qe, ve, we, se = q.copy(), v.copy(), w.copy(), np.zeros(1, np.int32)
                obs, r, fl, _, _ = O.env_step(cfg, qe, ve, we, se, a, hf)
                res.append(dict(q1=qe, v1=ve, w1=we, obs=obs, r=r, flags=fl))
        finally:
            O.set_solver(100, 1e-8)
        rec.update(res[0])
        rec["ambig"] = float(_relerr(res[1]["w1"], res[0]["w1"]))
        keep.append(rec)
    return keep


def census_cells(s):
    """Names of the census cells one state is in."""
    zw, zg, ng, it = s["zw"], s["zg"], s["ng"], s["niter"]
    act_g = [z for z in zg if z > 0]
    c = []
    if len(zw) == 3 and all(z == 1 for z in zw):
        c.append("wheels: all three sliding")
    if 2 in zw:
        c.append("wheels: one or more sticking")
    if 0 in zw and any(z > 0 for z in zw):
        c.append("wheels: inactive next to active")
    if len(zw) == 3 and all(z == 0 for z in zw):
        c.append("wheels: all three inactive")
    if len(zw) == 0:
        c.append("wheels: no contact")
    if ng == 0:
        c.append("ground: ng = 0")
    if act_g and all(z == 2 for z in act_g):
        c.append("ground: all active sticking")
    if 1 in zg:
        c.append("ground: one or more sliding")
    if 0 in zg and act_g:
        c.append("ground: inactive next to active")
    for k in NG_EXACT:
        if ng == k and (k < 50 or s["over"]):
            c.append(f"ng = {k}")
    for lo, hi in NG_RANGES:
        if lo <= ng <= hi:
            c.append(f"ng {lo}..{hi}")
    if 2 in zw and 1 in zg:
        c.append("crossed: wheel sticking, ground sliding")
    if ng >= 14 and 0 in zw:
        c.append("crossed: ng >= 14, a wheel inactive")
    if it == 0:
        c.append("niter 0")
    if it == 1:
        c.append("niter 1")
    if it >= 12:
        c.append("niter >= 12")
    return c


CELL_MIN = {name: MIN_PER_CELL for name in (
    ["wheels: all three sliding", "wheels: one or more sticking", "wheels: inactive next to active",
     "wheels: all three inactive", "wheels: no contact", "ground: ng = 0", "ground: all active sticking",
     "ground: one or more sliding", "ground: inactive next to active"] + [f"ng = {k}" for k in NG_EXACT]
    + ["crossed: wheel sticking, ground sliding", "crossed: ng >= 14, a wheel inactive", "niter 0", "niter 1",
       "niter >= 12"])}
CELL_MIN.update({f"ng {lo}..{hi}": 1 for lo, hi in NG_RANGES})


def build(O):
    """{terrain: [state records]} after the ambiguity drop, and the number dropped."""
    out, dropped, total = {}, 0, 0
    for i, terrain in enumerate(TERRAINS):
        recs = _evaluate(O, terrain, _candidates(O, terrain, seed=100 + i))
        total += len(recs)
        good = [r for r in recs if r["ambig"] <= AMBIG_TOL]
        dropped += len(recs) - len(good)
        for r in good:
            r["cells"] = census_cells(r)
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        out[terrain] = good
    return out, dropped, total


@pytest.fixture(scope="module")
def regime_states(oracle):
    """The kept states per terrain (read-only records); at most 2% may be solver-ambiguous."""
    states, dropped, total = build(oracle)
    assert dropped <= MAX_DROP_FRAC * total, (dropped, total)
    print(f"\nregime states: {total} built, {dropped} dropped as solver-ambiguous, "
          f"kept {[(t, len(s)) for t, s in states.items()]}")
    return states


def _stack(recs, key):
    return np.array([r[key] for r in recs])


def _cell_table(title, recs, err):
    """Print count and worst err per census cell (the module docstring's table)."""
    print(f"\n{title}")
    for cell in CELL_MIN:
        e = [x for r, x in zip(recs, err) if cell in r["cells"]]
        print(f"  {cell:42s} {len(e):4d}  {max(e) if e else float('nan'):.1e}")


def test_census_and_host_bounds(oracle, regime_states):
    """CPU: every census cell is populated, and the host build of the kernel's solver templates steps every
    kept state within the bounds the GPU tests apply (no state is solver-ambiguous for the kernel's search)."""
    import hostcheck_lib as H

    allr = [r for t in TERRAINS for r in regime_states[t]]
    assert 250 <= len(allr) <= 400, len(allr)
    counts = {cell: sum(cell in r["cells"] for r in allr) for cell in CELL_MIN}
    short = {c: (n, CELL_MIN[c]) for c, n in counts.items() if n < CELL_MIN[c]}
    assert not short, f"census cells short of their minimum (have, need): {short}"
    errs = []
    cfg = H.default_cfg()
    for t in TERRAINS:
        hf = _hfield(oracle, t)
        for i, r in enumerate(regime_states[t]):
            qe, ve, we, se = r["q"].copy(), r["v"].copy(), r["w"].copy(), np.zeros(1, np.int32)
            H.env_step(cfg, qe, ve, we, se, r["a"], hf)
            eq, ev, ew = np.abs(qe - r["q1"]).max(), np.abs(ve - r["v1"]).max(), float(_relerr(we, r["w1"]))
            errs.append(ew)
            assert eq <= Q_TOL and ev <= V_TOL and ew <= QACC_TOL, (t, i, eq, ev, ew, r["cells"])
    _cell_table("host build vs oracle, warm start (count, worst relative error)", allr, errs)


def _step_on_gpu(terrain, recs, precision, monkeypatch):
    """One env.step of the states on the fast kernels (serial route: the fast kernel takes every env)."""
    from ballbot_gym.envs import BallbotVecEnv

    monkeypatch.setenv("BB_ROUTE", "1")
    n = len(recs)
    env = BallbotVecEnv(n, device="cuda:0", precision=precision, auto_reset=False,
                        terrain_config=_terrain_cfg(terrain))
    env.set_state(_stack(recs, "q"), _stack(recs, "v"), _stack(recs, "w"), np.zeros(n, np.int32))
    s0 = env.stats()
    obs, rew, term, trunc, info = env.step(torch.tensor(_stack(recs, "a"), device="cuda:0"))
    q1, v1, w1, _ = env.get_state()
    out = dict(q1=q1, v1=v1, w1=w1, obs=obs.cpu().numpy().copy(), r=rew.cpu().numpy().copy(),
               flags=info["done_flags"].cpu().numpy().copy())
    s1 = env.stats()
    env.close()
    assert s1["slow_path"] == s0["slow_path"], "an env left the fast kernel (solve16<BODY=false>)"
    assert s1["diverged"] == s0["diverged"]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("terrain", TERRAINS)
def test_fast_kernel_step_by_regime(regime_states, terrain, monkeypatch):
    """A: the fast instantiation at qacc level, every state, no outlier."""
    recs = regime_states[terrain]
    g = _step_on_gpu(terrain, recs, "fp64", monkeypatch)
    eq = np.abs(g["q1"] - _stack(recs, "q1")).max(axis=1)
    ev = np.abs(g["v1"] - _stack(recs, "v1")).max(axis=1)
    eo = np.abs(g["obs"] - _stack(recs, "obs")).max(axis=1)
    er = np.abs(g["r"] - _stack(recs, "r"))
    ew = _relerr(g["w1"], _stack(recs, "w1"))
    _cell_table(f"{terrain}: fast kernel vs oracle, warm start (count, worst relative error)", recs, ew)
    print(f"{terrain}: {len(recs)} states, worst qpos {eq.max():.2e} qvel {ev.max():.2e} obs {eo.max():.2e} "
          f"reward {er.max():.2e} warm {ew.max():.2e}")
    bad = np.nonzero((eq > Q_TOL) | (ev > V_TOL) | (eo > OBS_TOL) | (er > R_TOL) | (ew > QACC_TOL))[0]
    assert len(bad) == 0, [(int(i), eq[i], ev[i], eo[i], er[i], ew[i], recs[i]["cells"]) for i in bad]
    assert np.array_equal(g["flags"] & 7, _stack(recs, "flags") & 7)
    assert np.array_equal((g["flags"] & 8) != 0, _stack(recs, "over") != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("terrain", TERRAINS)
def test_full_kernel_forward_by_regime(regime_states, terrain):
    """B: the full instantiation (bb_forward, solve16<BODY=true>) on the same states; every state, no outlier."""
    from ballbot_gym.envs import BallbotVecEnv

    recs = regime_states[terrain]
    n = len(recs)
    env = BallbotVecEnv(n, device="cuda:0", precision="fp64", auto_reset=False, terrain_config=_terrain_cfg(terrain))
    env.set_state(_stack(recs, "q"), _stack(recs, "v"), _stack(recs, "w"))
    qacc, ncon = env.forward(np.array([_ctrl(r["a"]) for r in recs]))
    env.close()
    assert np.array_equal(ncon[:, 0], _stack(recs, "ng")) and not ncon[:, 1].any()
    err = _relerr(qacc, _stack(recs, "qacc"))
    _cell_table(f"{terrain}: full kernel's forward vs oracle, qacc (count, worst relative error)", recs, err)
    bad = np.nonzero(err > QACC_TOL)[0]
    assert len(bad) == 0, [(int(i), err[i], recs[i]["cells"]) for i in bad]


def _mixed_order(recs, seed):
    """A seeded order whose 4-env waves each take one state without ground contact, one with 30 or more, and
    one each from the lower and the upper half of the others' Newton iteration counts, while those last."""
    rng = np.random.default_rng(seed)
    ng, it = _stack(recs, "ng"), _stack(recs, "niter")
    idx = np.arange(len(recs))
    mid = idx[(ng > 0) & (ng < 30)]
    med = np.median(it[mid])
    queues = [list(rng.permutation(k)) for k in (idx[ng == 0], idx[ng >= 30], mid[it[mid] < med], mid[it[mid] >= med])]
    order = []
    while any(queues):
        for j in range(4):
            q = queues[j] if queues[j] else max(queues, key=len)
            if q:
                order.append(int(q.pop()))
    return np.array(order)


@pytest.mark.gpu
@pytest.mark.parametrize("terrain,ragged", [("flat", 3), ("hills", 1), ("hills", 2)])
def test_step_independent_of_wave_neighbours(regime_states, terrain, ragged, monkeypatch):
    """C: the same states as built, reversed and in the mixed order, in env counts that leave the last wave
    with 1, 2 or 3 teams: every state's result is bit-equal whatever shares its wave."""
    recs = regime_states[terrain]
    recs = recs[:len(recs) - (len(recs) - ragged) % 4]
    n = len(recs)
    assert n % 4 == ragged
    mixed = _mixed_order(recs, seed=5)
    assert sorted(mixed) == list(range(n))
    ng, it = _stack(recs, "ng")[mixed], _stack(recs, "niter")[mixed]
    waves = [slice(4 * k, 4 * k + 4) for k in range(n // 4)]
    full_mix = sum((ng[w] == 0).any() and (ng[w] >= 30).any() and len(set(it[w])) > 1 for w in waves)
    assert full_mix >= MIN_PER_CELL, full_mix
    ref = None
    for order in (np.arange(n), np.arange(n)[::-1], mixed):
        g = _step_on_gpu(terrain, [recs[i] for i in order], "fp64", monkeypatch)
        back = np.empty(n, np.int64)
        back[order] = np.arange(n)
        g = {k: v[back] for k, v in g.items()}
        if ref is None:
            ref = g
            continue
        for k in ("q1", "v1", "w1", "obs", "r", "flags"):
            diff = np.nonzero((g[k] != ref[k]).reshape(n, -1).any(axis=1))[0]
            assert len(diff) == 0, (k, [(int(i), recs[i]["cells"]) for i in diff])


@pytest.mark.gpu
@pytest.mark.parametrize("terrain", TERRAINS)
def test_fast_kernel_step_fp32(regime_states, terrain, monkeypatch):
    """fp32: finite outputs, the oracle's done flags, overflow on the capped states only."""
    recs = regime_states[terrain]
    g = _step_on_gpu(terrain, recs, "fp32", monkeypatch)
    for k in ("q1", "v1", "w1", "obs", "r"):
        assert np.isfinite(g[k]).all(), k
    assert np.array_equal(g["flags"] & 3, _stack(recs, "flags") & 3)
    assert np.array_equal((g["flags"] & 8) != 0, _stack(recs, "over") != 0)
