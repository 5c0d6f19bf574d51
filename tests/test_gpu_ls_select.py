"""The fast kernels' line search after its exec-mask branches were cut (bb_team16.h, bb_solve.h: one evaluation as
ls_exits / ls_next with the three exits folded into `done`, the sums of phi', phi'' and the magnitude bound
interleaved, the later rounds of contacts behind a wave-uniform test), on the shapes at which a change there can
go wrong.

States: tests/test_gpu_solve_regimes.py's flat-ground candidates (same seed), evaluated with the oracle and, for
what the line searches of the step did, with a host build of the kernels' solver templates (BB_SOLVE_STATS,
tests/hostcheck/ls_census.cpp); 65 of them, chosen so that every cell below is populated, the rest in the
builder's order.  The host build runs the same search on a team of one lane; its counts say which states take
the paths, the GPU's own evaluations agree to rounding.

  search of 1 | 2 | >= 6 evaluations   the first trial accepted, one more, and long searches (kinks, a bracket)
  kink snap                            a trial point shortened to a contact's kink
  ng 0 | 13 | 14                       no ball-terrain contact (idle lanes 3..15), every lane busy, and contact 16
                                       on lane 0: the later rounds' wave-uniform path
  niter 0 | >= 12                      a solve that never searches, and long ones

  The first four states share a wave and mix a step whose searches all end at the first evaluation with one
  that holds a search of six or more: teams leaving the loop at different evaluations is what the change touches.

  The fallback (an unconverged search) is not reachable from physical flat states: no candidate's step takes it
  (the census prints the count).  tests/hostcheck/ls_select_check.cpp covers it, with searches cut short.

  step vs oracle    one fast-kernel step of the first 1, 3, 17 and all 65 states: qpos 1e-9, qvel 1e-6, warm start
                    1e-7 relative, no outlier, the oracle's flags
  fp32              the same 65 states: finite, the oracle's done flags
  forms agree       bb_step x 20, bb_step_multi (20 steps) and the rollout kernel on 65 flat envs from these
                    states: observations, rewards, flags and final states bit for bit
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_solve_regimes as R  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
N_STATES = 65
ENV_COUNTS = (1, 3, 17, 65)
CELLS = {"ls >= 6": 2, "ls all 1": 2, "ls 1": 2, "ls 2": 2, "kink snap": 2, "ng 0": 2, "ng 13": 2, "ng 14": 2,
         "niter 0": 2, "niter >= 12": 2}
T_FORMS = 20


def _census_lib():
    import hostcheck_lib as H

    src, lib = ROOT / "tests" / "hostcheck" / "ls_census.cpp", ROOT / "tests" / "_build" / "libbb_ls_census.so"
    lib.parent.mkdir(parents=True, exist_ok=True)
    srcs = [src] + sorted(CSRC.glob("*.h"))
    if not lib.exists() or any(lib.stat().st_mtime < s.stat().st_mtime for s in srcs):
        subprocess.run(["hipcc", "-O2", "-fPIC", "-shared", "--offload-arch=gfx950", "-std=c++17", "-DBB_SOLVE_STATS",
                        f"-I{CSRC}", "-o", str(lib), str(src)], check=True, capture_output=True)
    L = C.CDLL(str(lib))
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    L.lc_step.argtypes = [C.POINTER(H.EnvCfg), dp, dp, dp, fp, fp, C.c_double, C.POINTER(C.c_long)]
    return L, H


def _ls_stats(L, H, rec, hf):
    """What the line searches of one host step of the state did (ls_census.cpp)."""
    out = np.zeros(20, np.int64)
    cfg = H.default_cfg()
    q, v, w = (np.ascontiguousarray(rec[k], np.float64) for k in ("q", "v", "w"))
    a, hfa = np.ascontiguousarray(rec["a"], np.float32), np.ascontiguousarray(hf, np.float32)
    L.lc_step(C.byref(cfg), H._d(q), H._d(v), H._d(w), H._f(a), H._f(hfa), 2.0, out.ctypes.data_as(C.POINTER(C.c_long)))
    return dict(hist=out[:16].copy(), evals=int(out[16]), snaps=int(out[17]), fallbacks=int(out[18]))


def _cells(r):
    c, h = [], r["ls"]["hist"]
    if h[6:].sum() > 0:
        c.append("ls >= 6")
    if h[1] > 0 and h[2:].sum() == 0 and r["ls"]["fallbacks"] == 0:
        c.append("ls all 1")
    if h[1] > 0:
        c.append("ls 1")
    if h[2] > 0:
        c.append("ls 2")
    if r["ls"]["snaps"] > 0:
        c.append("kink snap")
    if r["ls"]["fallbacks"] > 0:
        c.append("fallback")
    if r["ng"] in (0, 13, 14):
        c.append(f"ng {r['ng']}")
    if r["niter"] == 0:
        c.append("niter 0")
    if r["niter"] >= 12:
        c.append("niter >= 12")
    return c


@pytest.fixture(scope="module")
def ls_states(oracle):
    """65 read-only state records (test_gpu_solve_regimes._evaluate plus "ls" and "lcells"): first one state per
    cell, in CELLS' order, then a second of each, then the rest in the builder's order."""
    O = oracle
    hf = R._hfield(O, "flat")
    L, H = _census_lib()
    recs = [r for r in R._evaluate(O, "flat", R._candidates(O, "flat", seed=100)) if r["ambig"] <= R.AMBIG_TOL]
    for r in recs:
        r["ls"] = _ls_stats(L, H, r, hf)
        r["lcells"] = _cells(r)
    order = []

    def take(i):
        if i not in order and len(order) < N_STATES:
            order.append(i)

    for rounds in (1, 2):
        for cell, need in CELLS.items():
            have = [i for i, r in enumerate(recs) if cell in r["lcells"]]
            for i in have[:need if rounds == 2 else 1]:
                take(i)
    for i in range(len(recs)):
        take(i)
    out = [recs[i] for i in order]
    for r in out:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    out[0]["pool_fallbacks"] = sum(r["ls"]["fallbacks"] > 0 for r in recs)
    out[0]["pool_size"] = len(recs)
    return out


def test_census(ls_states):
    """CPU: 65 states, every cell populated, the first wave mixes searches that end at once with a long one, and
    the pool's count of states that take the fallback is printed (none: the host check covers it)."""
    recs = ls_states
    assert len(recs) == N_STATES
    counts = {c: sum(c in r["lcells"] for r in recs) for c in list(CELLS) + ["fallback"]}
    print(f"\ncensus {counts}; states of the pool ({recs[0]['pool_size']}) that take the fallback: "
          f"{recs[0]['pool_fallbacks']}; first four: {[(r['ng'], r['niter'], r['ls']['hist'].tolist()) for r in recs[:4]]}")
    short = {c: (counts[c], n) for c, n in CELLS.items() if counts[c] < n}
    assert not short, f"cells short of their minimum (have, need): {short}"
    assert "ls >= 6" in recs[0]["lcells"] and "ls all 1" in recs[1]["lcells"]


def test_select_forms_on_host():
    """CPU: tests/hostcheck/ls_select_check.cpp, the branch-free prep, crosses and evaluation against copies of
    the branching forms, bit for bit in floats and doubles."""
    src, exe = ROOT / "tests" / "hostcheck" / "ls_select_check.cpp", ROOT / "tests" / "_build" / "ls_select_check"
    exe.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", "-o", str(exe), str(src)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _against_oracle(recs, g):
    eq = np.abs(g["q1"] - R._stack(recs, "q1")).max(axis=1)
    ev = np.abs(g["v1"] - R._stack(recs, "v1")).max(axis=1)
    ew = R._relerr(g["w1"], R._stack(recs, "w1"))
    print(f"{len(recs)} envs: worst qpos {eq.max():.2e} qvel {ev.max():.2e} warm {ew.max():.2e}")
    bad = np.nonzero((eq > R.Q_TOL) | (ev > R.V_TOL) | (ew > R.QACC_TOL))[0]
    assert len(bad) == 0, [(int(i), eq[i], ev[i], ew[i], recs[i]["lcells"]) for i in bad]
    assert np.array_equal(g["flags"] & 7, R._stack(recs, "flags") & 7)
    assert np.array_equal((g["flags"] & 8) != 0, R._stack(recs, "over") != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_fast_step_vs_oracle(ls_states, n, monkeypatch):
    recs = ls_states[:n]
    _against_oracle(recs, R._step_on_gpu("flat", recs, "fp64", monkeypatch))


@pytest.mark.gpu
def test_fast_step_fp32_finite(ls_states, monkeypatch):
    recs = ls_states
    g = R._step_on_gpu("flat", recs, "fp32", monkeypatch)
    for k in ("q1", "v1", "w1", "obs", "r"):
        assert np.isfinite(g[k]).all(), k
    assert np.array_equal(g["flags"] & 3, R._stack(recs, "flags") & 3)
    assert np.array_equal((g["flags"] & 8) != 0, R._stack(recs, "over") != 0)


@pytest.mark.gpu
def test_launch_forms_bit_equal(ls_states, monkeypatch):
    """The rollout kernel's 20 steps from the directed states, its own clipped actions replayed through bb_step
    and through one bb_step_multi launch on twin envs.  A first bb_step with zero actions on all three gives the
    rollout its observations (set_state does not form them); the states are then one step on."""
    from ballbot_gym.envs import BallbotVecEnv
    from ballbot_rl.training.logger import CSVLogger
    from ballbot_rl.training.ppo import BatchedPPO, fused_mlp_slots

    recs, n, T = ls_states, N_STATES, T_FORMS
    monkeypatch.setenv("BB_ROUTE", "1")
    envs = [BallbotVecEnv(n, device="cuda:0", precision="fp64", seed=3, terrain_config=R._terrain_cfg("flat"))
            for _ in range(3)]
    zero = torch.zeros(n, 3, device="cuda:0")
    for e in envs:
        e.set_state(R._stack(recs, "q"), R._stack(recs, "v"), R._stack(recs, "w"), np.zeros(n, np.int32))
        e.step(zero)
    a, b, c = envs
    assert torch.equal(a.obs, b.obs) and torch.equal(a.obs, c.obs)
    m = BatchedPPO(a, n_steps=T, batch_size=n * T, n_epochs=1, seed=4, logger=CSVLogger(None, stdout=False))
    with torch.no_grad():
        for p in m.policy.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    slots = fused_mlp_slots(m, update=False)
    assert slots
    m._last_obs = a.obs
    m._last_starts.fill_(1)
    m._collect_rollout_kernel(slots)
    torch.cuda.synchronize()
    actions = m.buf.actions[:T].clamp(-1.0, 1.0).contiguous()
    obs = b.obs.clone()
    step_obs, step_rew, step_done = [], [], []
    for t in range(T):
        assert torch.equal(m.buf.obs[t], obs), t
        o, r, _, _, info = b.step(actions[t])
        assert torch.equal(m.buf.rewards[t], r), t
        step_obs.append(o.clone()), step_rew.append(r.clone()), step_done.append(info["done_flags"].clone())
        obs = o.clone()
    assert torch.equal(a.obs, obs)
    got = c.step_multi(actions)
    assert torch.equal(got["obs"], torch.stack(step_obs))
    assert torch.equal(got["reward"], torch.stack(step_rew))
    assert torch.equal(got["done"], torch.stack(step_done))
    sb = b.get_state()
    for other in (a, c):
        for x, y in zip(sb, other.get_state()):
            np.testing.assert_array_equal(x, y)
    for e in envs:
        e.close()
