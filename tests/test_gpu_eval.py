"""GPU: the device-side evaluator and its pieces.

* bb_eval_track against the numpy restatement of evaluate_policy's loop (tests/eval_track_ref.py), on the
  host test's streams, at sizes that cross a wave (64 / 65), the accounting workgroup's chunk of 1024 envs
  (1025) and two chunks (2049): everything exact.
* bb_depth_encoder's skip rule: rows with index >= 0 equal the gathered call of those rows bit for bit,
  skipped rows keep a sentinel, also where a conv2 workgroup walks several images (n = 321); train mode
  refuses a negative entry.
* evaluate_policy(fused=True) / DeviceEvaluator against a stepwise twin: this file's own loop over a twin
  env built with the same arguments, calling the same kernels eagerly (fused_encoder_forward on all rows
  every step, the features assembled with torch, bb_ppo_mlp_act without noise, env.step_flags) with
  evaluate_policy's host accounting.  Equality is exact (returns, lengths, env ids, steps, order; at
  poll = 1 also the env's obs, depth frames, timestamps, state and terrain draws): both sides run the same
  kernels on the same bits, and an eval-mode encoder is a fixed function of one image.
* The fused first step's clipped actions against policy.predict on the same observation, under
  tests/test_gpu_ppo_kernels.py's rule for bb_ppo_mlp_act: e_kernel <= 8 * e_torch + 1e-8 with a float64 MLP
  on the feature rows as the reference, e_torch the error of policy.predict.  Whole evaluations are not compared
  with the eager torch path: the two MLPs sum in different orders and a falling robot amplifies that.
* BatchedPPO.load_policy("x.zip") on the GPU optimiser's flat buffer (the path `resume:` takes).
"""
import copy
import ctypes as C
import io
import json
import os
import subprocess
import sys
import zipfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import eval_track_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
SENT = 12345.0


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ bb_eval_track alone
class DevState:
    """One bb_eval_track caller's device arrays, initialised as eval_track_ref.TrackRef (sentinels
    included); the table arrays hold `slack` rows more than cap says."""

    def __init__(self, n, targets, cap, slack=8):
        ref = R.TrackRef(n, targets, cap + slack)
        self.n, self.cap = n, cap
        for k in ("targets", "ep_ret", "ep_len", "counts", "tab_ret", "tab_len", "tab_env", "tab_step", "book"):
            setattr(self, k, _dev(getattr(ref, k)))
        self.feats = torch.full((n, 56), R.SENTINEL, device=DEV)
        self.fresh = torch.full((n,), -5, dtype=torch.int64, device=DEV)

    def call(self, reward, flags, obs, rel_ts, stage=True):
        from ballbot_gym import _native as N

        a = N.EvalArgs(self.n, self.cap, _ptr(reward), _ptr(flags), _ptr(obs), _ptr(rel_ts), _ptr(self.targets),
                       _ptr(self.ep_ret), _ptr(self.ep_len), _ptr(self.counts), _ptr(self.tab_ret), _ptr(self.tab_len),
                       _ptr(self.tab_env), _ptr(self.tab_step), _ptr(self.book), _ptr(self.feats) if stage else None,
                       _ptr(self.fresh) if stage else None)
        N.check(N.lib().bb_eval_track(C.byref(a), _stream()), "bb_eval_track")


def _assert_track_equal(got, ref, slack=8):
    for k in ("ep_ret", "ep_len", "counts", "book"):
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), getattr(ref, k), err_msg=k)
    for k in ("tab_ret", "tab_len", "tab_env", "tab_step"):
        g, r = getattr(got, k).cpu().numpy(), getattr(ref, k)
        np.testing.assert_array_equal(g[:len(r)], r, err_msg=k)
        assert (g[len(r):] == (R.SENTINEL if k == "tab_ret" else -7)).all(), f"{k}: rows past cap were written"


@pytest.mark.parametrize("n", [1, 64, 65, 1025, 2049])
def test_eval_track_equals_the_numpy_restatement(n):
    """50 steps, p(done) = 0.2, E = n + 2 (two envs owe two episodes) and E = n // 2 (half owe none);
    checked after steps 1, 2, 3, 10 and 50 (the state carries over, so a late check sees every step)."""
    reward, flags, obs, rel_ts = R.streams(n)
    T = reward.shape[0]
    d_reward, d_flags, d_obs, d_ts = _dev(reward), _dev(flags), _dev(obs), _dev(rel_ts)
    for E in sorted({n + 2, max(1, n // 2)}):
        tg = R.targets_for(E, n)
        ref, got = R.TrackRef(n, tg, E), DevState(n, tg, E)
        feats_ref = np.full((n, 56), R.SENTINEL, np.float32)
        fresh_ref = np.full(n, -5, np.int64)
        multi = 0
        for t in range(T):
            before = int(ref.book[0])
            ref.step(reward[t], flags[t])
            multi += int(ref.book[0]) - before >= 2
            R.stage_ref(obs[t], rel_ts[t], feats_ref, fresh_ref)
            got.call(d_reward[t], d_flags[t], d_obs[t], d_ts[t])
            if t in (0, 1, 2, 9, T - 1):
                _assert_track_equal(got, ref)
                np.testing.assert_array_equal(got.feats.cpu().numpy(), feats_ref)
                np.testing.assert_array_equal(got.fresh.cpu().numpy(), fresh_ref)
        listed = int(ref.book[0])
        print(f"n={n} E={E}: {listed} listed, {multi} steps listed two or more")
        assert listed >= 1 and ref.book[3] == 0 and (n < 3 or multi > 0)
        assert (got.feats[:, 13:53] == R.SENTINEL).all()
        assert (got.tab_ret[listed:] == R.SENTINEL).all() and (got.tab_env[listed:] == -7).all()


def test_eval_track_at_32768_envs():
    """The largest n the header promises: 32 chunks of the accounting workgroup, 32 staging workgroups;
    4 steps at p(done) = 0.2 with E = n + 2, everything exact."""
    n, E = 32768, 32770
    reward, flags, obs, rel_ts = R.streams(n, T=4, seed=5)
    tg = R.targets_for(E, n)
    ref, got = R.TrackRef(n, tg, E), DevState(n, tg, E)
    feats_ref, fresh_ref = np.full((n, 56), R.SENTINEL, np.float32), np.full(n, -5, np.int64)
    for t in range(reward.shape[0]):
        ref.step(reward[t], flags[t])
        R.stage_ref(obs[t], rel_ts[t], feats_ref, fresh_ref)
        got.call(_dev(reward[t]), _dev(flags[t]), _dev(obs[t]), _dev(rel_ts[t]))
    _assert_track_equal(got, ref)
    np.testing.assert_array_equal(got.feats.cpu().numpy(), feats_ref)
    np.testing.assert_array_equal(got.fresh.cpu().numpy(), fresh_ref)
    assert int(ref.book[0]) > 3 * 1024 and int(ref.tab_env[:int(ref.book[0])].max()) > 32000


def test_eval_track_overflow_and_priming():
    n, E, cap = 1025, 1030, 700
    reward, flags, obs, rel_ts = R.streams(n, T=12, seed=2)
    tg = R.targets_for(E, n)
    ref, got = R.TrackRef(n, tg, cap), DevState(n, tg, cap)
    d_reward, d_flags = _dev(reward), _dev(flags)
    for t in range(reward.shape[0]):
        ref.step(reward[t], flags[t])
        got.call(d_reward[t], d_flags[t], None, None, stage=False)
    _assert_track_equal(got, ref)
    assert int(got.book[3]) == 1 and int(got.book[0]) > cap
    assert (got.feats == R.SENTINEL).all() and (got.fresh == -5).all()  # staging was off
    # the priming call: staging only, the accounting state is not touched
    got2 = DevState(n, tg, cap)
    before = [getattr(got2, k).clone() for k in ("ep_ret", "ep_len", "counts", "tab_ret", "tab_env", "book")]
    got2.call(None, None, _dev(obs[0]), torch.zeros(n, device=DEV))
    for k, v in zip(("ep_ret", "ep_len", "counts", "tab_ret", "tab_env", "book"), before):
        assert torch.equal(getattr(got2, k), v), k
    assert torch.equal(got2.fresh, torch.arange(n, device=DEV))
    assert torch.equal(got2.feats[:, 0:12], _dev(obs[0])[:, 0:12]) and (got2.feats[:, 12] == 0).all()
    assert torch.equal(got2.feats[:, 53:56], _dev(obs[0])[:, 12:15]) and (got2.feats[:, 13:53] == R.SENTINEL).all()
    got2.feats[:, 12] = 5.0
    got2.call(None, None, _dev(obs[1]), None)  # no cameras: column 12 stays, nothing is fresh
    assert (got2.fresh == -1).all() and (got2.feats[:, 12] == 5.0).all()


def test_eval_track_argument_errors():
    from ballbot_gym import _native as N

    L = N.lib()
    assert L.bb_eval_track(None, None) < 0 and "NULL args" in N.last_error()
    a = N.EvalArgs(0, 4, *([None] * 15))
    assert L.bb_eval_track(C.byref(a), None) < 0 and "n must be >= 1" in N.last_error()
    x = torch.zeros(64, device=DEV)
    a = N.EvalArgs(4, 4, _ptr(x), _ptr(x), *([None] * 13))
    assert L.bb_eval_track(C.byref(a), None) < 0 and "must be non-NULL with flags" in N.last_error()
    a = N.EvalArgs(4, 4, *([None] * 13), _ptr(x), None)
    assert L.bb_eval_track(C.byref(a), None) < 0 and "need obs" in N.last_error()


# ------------------------------------------------------------------ the encoder's skip rule
def _encoder(seed):
    """A frozen encoder of the reference's layout with random weights and running statistics."""
    from ballbot_rl.encoders.models import TinyAutoencoder

    g = torch.Generator().manual_seed(seed)
    enc = TinyAutoencoder(64, 64).encoder
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            elif isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (0.3 if m.weight.dim() == 4 else 0.02))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    for p in enc.parameters():
        p.requires_grad = False
    return enc.to(DEV).eval()


@pytest.mark.parametrize("n", [1, 33, 65, 321])
def test_masked_encoder_equals_the_gathered_call(n):
    """n = 321 is past conv2_kernel's grid of 256 workgroups: workgroups 0..64 walk two images each, with every
    combination of a live and a skipped image (empty pipeline stages between live ones, the LDS buffer's
    parity, the accumulators restarted at an image's first item after a skip)."""
    from ballbot_rl.encoders.models import fused_encoder_forward

    enc = _encoder(3)
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, 2, 64, 64, generator=g).to(DEV)
    img = x[:, 1:2]  # a channel slice of the camera tensor, as the evaluator passes it
    keep = torch.rand(n, generator=g) < 0.5
    if n > 256:  # the four (first image, second image) combinations of a two-image workgroup occur
        pairs = {(bool(keep[b]), bool(keep[b + 256])) for b in range(n - 256)}
        assert pairs == {(True, True), (True, False), (False, True), (False, False)}
    for name, mask in (("random half", keep), ("all skipped", torch.zeros(n, dtype=torch.bool)),
                       ("identity", torch.ones(n, dtype=torch.bool))):
        index = torch.where(mask, torch.arange(n), torch.full((n,), -1)).to(DEV)
        feats = torch.full((n, 56), SENT, device=DEV)
        out = fused_encoder_forward(enc, img, index=index, out=feats[:, 33:53], out_stride=56)
        assert out.data_ptr() == feats[:, 33:53].data_ptr()
        rows = torch.nonzero(mask).view(-1).to(DEV)
        if rows.numel():
            want = fused_encoder_forward(enc, img, index=rows)  # today's gathered call of those rows
            assert torch.equal(feats[rows, 33:53], want), name
            assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        skipped = torch.nonzero(~mask).view(-1).to(DEV)
        assert (feats[skipped] == SENT).all(), f"{name}: a skipped row was written"
        assert (feats[:, :33] == SENT).all() and (feats[:, 53:] == SENT).all(), f"{name}: wrote outside its columns"
    # the whole batch through the plain call equals the identity index (no index, the evaluator's priming)
    plain = fused_encoder_forward(enc, img)
    assert torch.equal(plain, feats[:, 33:53])


def test_train_mode_refuses_a_negative_index():
    from ballbot_gym import _native as N
    from ballbot_rl.encoders.models import fused_encoder_forward

    enc = _encoder(4)
    x = torch.rand(8, 1, 64, 64, device=DEV)
    before = enc[1].running_mean.clone()
    enc.train()
    with pytest.raises(RuntimeError, match="negative in train mode"):
        fused_encoder_forward(enc, x, index=torch.tensor([0, 1, -1, 3], device=DEV))
    assert "index[2]" in N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(enc[1].running_mean, before), "a refused call moved the running statistics"
    out = fused_encoder_forward(enc, x, index=torch.tensor([0, 1, 2, 3], device=DEV))  # non-negative: as before
    assert out.shape == (4, 20) and not torch.equal(enc[1].running_mean, before)


# ------------------------------------------------------------------ fused evaluator against a stepwise twin
def _policy(cameras, seed=0, scale=150.0, biases=False):
    """A randomly initialised policy whose action head is scaled up (orthogonal gain 0.01 x scale), so the
    deterministic actions saturate and the robot falls.  biases: random trunk and head biases (N(0, 0.1)), so
    that the all-zero proprio observation after a reset does not give an exactly zero action."""
    from ballbot_rl.policies.mlp_policy import ActorCriticPolicy, obs_spaces

    torch.manual_seed(seed)
    enc = _encoder(seed + 1).cpu() if cameras else None
    pol = ActorCriticPolicy(obs_spaces(cameras=cameras), 3, frozen_encoder=enc)
    with torch.no_grad():
        pol.action_net.weight.mul_(scale)
        if biases:
            for m in list(pol.policy_net) + list(pol.value_net_trunk) + [pol.action_net, pol.value_net]:
                if isinstance(m, torch.nn.Linear):
                    m.bias.normal_(0.0, 0.1)
    return pol.to(DEV).eval()


def _env(n, cameras, terrain="flat", max_ep_steps=None, seed=5):
    from ballbot_gym.envs import BallbotVecEnv

    kw = {"n_terrains": None} if terrain == "perlin" else {}
    return BallbotVecEnv(n, device=DEV, seed=seed, terrain_config={"type": terrain, "config": {}},
                         max_ep_steps=max_ep_steps, disable_cameras=not cameras,
                         stream_seeds=[seed + 100 + i for i in range(n)], **kw)


class Twin:
    """evaluate_policy, stepwise: the same kernels as the fused graph, called one by one, no cache."""

    def __init__(self, policy, env):
        from ballbot_rl.training.ppo import pack_mlp_params, reference_mlp_tensors

        self.policy, self.env, self.cameras = policy, env, bool(env.cameras)
        self.flat, offs = pack_mlp_params(reference_mlp_tensors(policy, self.cameras), env.device)
        self.offs = (C.c_int32 * 21)(*offs)
        self.first_clipped = None
        self.first_feats = None
        self.first_inputs = None  # (obs, depth, rel_ts) the first policy step read
        self.partial_mask_steps = 0  # steps after which some, not all, cameras had just rendered

    def features(self):
        from ballbot_rl.encoders.models import fused_encoder_forward

        env = self.env
        if not self.cameras:
            return env.obs
        ext = self.policy.features_extractor.extractors
        return torch.cat([env.obs[:, 0:12], env.rel_ts.reshape(-1, 1),
                          fused_encoder_forward(ext["rgbd_0"], env.depth[:, 0:1]),
                          fused_encoder_forward(ext["rgbd_1"], env.depth[:, 1:2]), env.obs[:, 12:15]], dim=1).contiguous()

    def evaluate(self, E, max_steps=1_000_000):
        from ballbot_gym import _native as N

        env, n = self.env, int(self.env.num_envs)
        targets, counts = R.targets_for(E, n), np.zeros(n, np.int64)
        ret, length = np.zeros(n, np.float64), np.zeros(n, np.int64)
        rows = []  # (return rounded as evaluate_policy, length, env, step)
        acts, clipped = torch.zeros(n, 3, device=DEV), torch.zeros(n, 3, device=DEV)
        val, logp = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.policy.eval()
        env.reset()
        for step in range(1, max_steps + 1):
            f = self.features()
            N.check(N.lib().bb_ppo_mlp_act(_ptr(self.flat), self.offs, int(self.flat.numel()), _ptr(f),
                                           int(f.shape[1]), None, n, None, _ptr(acts), _ptr(clipped), _ptr(val),
                                           _ptr(logp), _stream()), "bb_ppo_mlp_act")
            if self.first_clipped is None:
                self.first_clipped, self.first_feats = clipped.clone(), f.clone()
                self.first_inputs = (env.obs.clone(), env.depth.clone() if self.cameras else None,
                                     env.rel_ts.clone() if self.cameras else None)
            _, reward, flags = env.step_flags(clipped)
            if self.cameras:
                k = int((env.rel_ts == 0).sum())
                self.partial_mask_steps += 0 < k < n
            ret += reward.cpu().numpy().astype(np.float64)
            length += 1
            for i in np.nonzero(flags.cpu().numpy() & 1)[0]:
                if counts[i] < targets[i]:
                    rows.append((round(float(ret[i]), 6), int(length[i]), int(i), step))
                    counts[i] += 1
                ret[i], length[i] = 0.0, 0
            if not (counts < targets).any():
                break
        self.steps = step
        return rows


def _rows(result):
    return list(zip(result["episode_rewards"], result["episode_lengths"], result["episode_envs"],
                    result["episode_steps"]))


def _snapshot(env):
    q, v, w, s = env.get_state()
    out = {"obs": env.obs.cpu().numpy().copy(), "qpos": q.copy(), "qvel": v.copy(), "warm": w.copy(),
           "steps": s.copy(), "terrain": np.asarray(env.env_terrain()[0]).copy(),
           "draws": np.asarray(env.env_terrain()[1]).copy()}
    if env.cameras:
        out["depth"] = env.depth.cpu().numpy().copy()
        out["rel_ts"] = env.rel_ts.cpu().numpy().copy()
    return out


def _assert_same_env(a, b):
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), f"env {k} differs after the evaluation"


# name: (n, E, terrain, max_ep_steps, cameras); the twin of a case is computed once and shared
CASES = {
    "n1_E3": (1, 3, "flat", None, True),
    "n3_E8": (3, 8, "flat", None, True),
    "n65_E8": (65, 8, "flat", None, True),      # 57 envs owe nothing and keep stepping
    "n64_E66": (64, 66, "flat", None, True),    # two envs owe two episodes
    "flat13": (33, 40, "flat", 13, True),       # every env truncates in the same step, out of phase with the
                                                # cameras' 6-step cadence
    "perlin200": (33, 40, "perlin", 200, True),
    "proprio": (64, 70, "flat", None, False),
}
_twins = {}


def _twin(name):
    if name not in _twins:
        n, E, terrain, mes, cams = CASES[name]
        pol = _policy(cams, seed=len(name))
        env = _env(n, cams, terrain, mes)
        tw = Twin(pol, env)
        rows = tw.evaluate(E)
        fails = sum(1 for r in rows if r[1] < env.max_ep_steps)
        steps = [r[3] for r in rows]
        print(f"twin {name}: {len(rows)} episodes in {tw.steps} steps, {fails} failures, "
              f"{len(rows) - fails} truncations, {len(steps) - len(set(steps))} shared steps")
        _twins[name] = (pol, tw, rows, env.max_ep_steps)
    return _twins[name]


def test_the_cases_cover_failure_truncation_and_shared_steps():
    """A condition on the inputs, asserted on the twin's own tables: over the cases at least one episode
    ended by failure and one by truncation, and in at least one step two or more envs finished."""
    fail = trunc = shared = 0
    for name in ("n65_E8", "flat13", "perlin200"):
        _, _, rows, mes = _twin(name)
        fail += sum(1 for r in rows if r[1] < mes)
        trunc += sum(1 for r in rows if r[1] == mes)
        steps = [r[3] for r in rows]
        shared += len(steps) - len(set(steps))
    assert fail >= 1 and trunc >= 1 and shared >= 1, (fail, trunc, shared)
    # flat resets are identical and the policy is deterministic, so every flat env finishes in the same step and
    # its cameras render together: envs out of step with each other come from the perlin case alone
    _, tw, rows, _ = _twin("perlin200")
    assert len({r[3] for r in rows}) >= 2, "perlin200: every episode finished in the same step"
    assert tw.partial_mask_steps >= 1, "perlin200: the encoder's mask was never partial (0 < fresh rows < n)"
    print(f"perlin200: {len({r[3] for r in rows})} distinct finishing steps, {tw.partial_mask_steps} steps with a "
          f"partial mask")


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_the_stepwise_twin(name):
    from ballbot_rl.evaluation import evaluate_policy

    n, E, terrain, mes, cams = CASES[name]
    pol, tw, rows, _ = _twin(name)
    env = _env(n, cams, terrain, mes)
    r = evaluate_policy(pol, env, n_eval_episodes=E, fused=True, poll=1)
    assert _rows(r) == rows
    assert len(rows) == E and r["mean_reward"] == float(np.mean([x[0] for x in rows]))
    assert r["mean_ep_length"] == float(np.mean([x[1] for x in rows])) and r["std_reward"] == float(np.std([x[0] for x in rows]))
    _assert_same_env(env, tw.env)  # poll = 1 stops where the eager loop stops: state, frames, terrain draws
    env.close()


def test_poll_7_gives_the_same_table():
    from ballbot_rl.evaluation import DeviceEvaluator

    n, E, terrain, mes, cams = CASES["n65_E8"]
    pol, tw, rows, _ = _twin("n65_E8")
    env = _env(n, cams, terrain, mes)
    ev = DeviceEvaluator(pol, env)
    r = ev.evaluate(E, poll=7)
    assert _rows(r) == rows
    assert tw.steps <= ev.steps < tw.steps + 7 and (ev.steps % 7 == 0)
    env.close()


def test_device_evaluator_reuse_carries_the_generators_over():
    """Two evaluations in a row on one DeviceEvaluator (one capture) equal two twin evaluations in a row:
    the second starts on the terrains the first one's resets left."""
    from ballbot_rl.evaluation import DeviceEvaluator

    n, E = 17, 20
    pol = _policy(True, seed=21)
    twin_env, env = _env(n, True, "perlin", 120), _env(n, True, "perlin", 120)
    tw = Twin(pol, twin_env)
    want = [tw.evaluate(E), tw.evaluate(E)]
    ev = DeviceEvaluator(pol, env)
    got = [_rows(ev.evaluate(E)), None]
    graph = ev.graph
    got[1] = _rows(ev.evaluate(E))
    assert ev.graph is graph, "the second evaluation captured a new graph"
    assert got == want and want[0] != want[1]
    _assert_same_env(env, twin_env)
    env.close()
    twin_env.close()


def test_eval_callback_fused_writes_the_twins_npz(tmp_path):
    from ballbot_rl.training.callbacks import EvalCallback
    from ballbot_rl.training.logger import CSVLogger

    n, E, terrain, mes, cams = CASES["n3_E8"]
    pol, tw, rows, _ = _twin("n3_E8")
    env = _env(n, cams, terrain, mes)
    model = SimpleNamespace(policy=pol, logger=CSVLogger(None, stdout=False), save=lambda path: None)
    cb = EvalCallback(env, n_eval_episodes=E, eval_freq=10, n_total_envs=4, log_path=tmp_path, fused=True)
    cb(model, 1, 10)
    z = np.load(tmp_path / "evaluations.npz", allow_pickle=False)
    np.testing.assert_array_equal(z["timesteps"], [40])
    np.testing.assert_array_equal(z["results"], np.array([[x[0] for x in rows]]))
    np.testing.assert_array_equal(z["ep_lengths"], np.array([[x[1] for x in rows]]))
    assert cb._evaluator is not None and cb.best_mean_reward == float(np.mean([x[0] for x in rows]))
    env.close()


@pytest.mark.parametrize("cams", [True, False], ids=["cameras_perlin", "proprio_flat"])
def test_fused_first_actions_against_policy_predict(cams):
    """The fused graph's first clipped actions against policy.predict on the same observation, under
    tests/test_gpu_ppo_kernels.py's rule for bb_ppo_mlp_act: with a float64 MLP on the feature rows as the
    reference, e_kernel <= 8 * e_torch + 1e-8, e_torch being the error of policy.predict (the torch Extractor and
    the policy's fp32 torch modules on the GPU).  The policy here has random biases and a mild action scale, so
    the actions are neither zero nor saturated, and on perlin the camera rows differ between envs; all three are
    asserted, as conditions on the inputs."""
    from ballbot_rl.evaluation import DeviceEvaluator
    from ballbot_rl.training.ppo import policy_obs

    n, terrain = (33, "perlin") if cams else (64, "flat")
    pol = _policy(cams, seed=31, scale=10.0, biases=True)
    twin_env, env = _env(n, cams, terrain, 200), _env(n, cams, terrain, 200)
    tw = Twin(pol, twin_env)
    tw.evaluate(n, max_steps=1)
    ev = DeviceEvaluator(pol, env)
    ev.evaluate(n, max_steps=1)  # one replay: ev.clipped holds the first step's actions
    assert torch.equal(ev.clipped, tw.first_clipped)
    obs, depth, rel_ts = tw.first_inputs
    feats = tw.first_feats
    with torch.no_grad():
        yard = pol.predict(policy_obs(obs, depth, rel_ts) if cams else obs, deterministic=True)
        p64, a64 = copy.deepcopy(pol.policy_net).double().cpu(), copy.deepcopy(pol.action_net).double().cpu()
        ref = a64(p64(feats.double().cpu())).clamp(-1.0, 1.0)
    ek = float((ev.clipped.double().cpu() - ref).abs().max())
    et = float((yard.double().cpu() - ref).abs().max())
    unclipped = int((ref.abs() < 1).all(1).sum())
    distinct = len({tuple(r) for r in ref.numpy().round(9).tolist()})
    print(f"RATIO fused first step cams={cams}: e_kernel={ek:.3e} e_torch={et:.3e} unclipped rows {unclipped}/{n} "
          f"distinct rows {distinct} max|a|={float(ref.abs().max()):.3f}")
    assert unclipped >= 1 and float(ref.abs().max()) > 1e-3 and et > 0, "the case does not exercise the comparison"
    assert not cams or distinct >= 2, "every env saw the same camera rows"
    assert ek <= 8.0 * et + 1e-8
    env.close()
    twin_env.close()


def test_resume_from_a_zip_on_the_gpu(tmp_path):
    """BatchedPPO.load_policy("x.zip") on FlatAdamW (the path `resume:` takes): the parameters stay views of the
    optimiser's flat buffer, and the buffer holds the zip's tensors."""
    from test_sb3_zip import sb3_state, write_zip

    from ballbot_rl.evaluation import load_sb3_policy
    from ballbot_rl.training.optim import FlatAdamW
    from ballbot_rl.training.ppo import BatchedPPO, fused_mlp_slots

    env = _env(4, False)
    ppo = BatchedPPO(env, n_steps=8, batch_size=16, seed=1)
    opt = ppo.optimizer
    assert isinstance(opt, FlatAdamW)
    flat_ptr = opt.flat.data_ptr()
    before = opt.flat.clone()
    path = write_zip(tmp_path / "best_model.zip", sb3_state(15, seed=9))
    ppo.load_policy(str(path))
    want, _ = load_sb3_policy(path, DEV)
    assert opt.flat.data_ptr() == flat_ptr and not torch.equal(opt.flat, before)
    named = dict(ppo.policy.named_parameters())
    for (k, w), p, off in zip(want.named_parameters(), opt.params, opt.offsets):
        assert named[k] is p, k
        assert p.data_ptr() == flat_ptr + 4 * off, f"{k} is no longer a view of the flat buffer"
        assert torch.equal(opt.flat[off:off + p.numel()], w.detach().reshape(-1)), k
    slots = fused_mlp_slots(ppo, update=False)  # the fused kernels still find every tensor in the buffer
    assert slots is not None and sorted(slots) == sorted(opt.offsets)
    env.close()


def test_refusals():
    from ballbot_gym.envs import BallbotVecEnv
    from ballbot_rl.evaluation import DeviceEvaluator, evaluate_policy
    from ballbot_rl.policies.mlp_policy import ActorCriticPolicy, obs_spaces

    cam_pol, pro_pol = _policy(True, seed=2), _policy(False, seed=2)
    env = _env(2, True)
    with pytest.raises(ValueError, match="15 features"):
        DeviceEvaluator(pro_pol, env)  # a proprio policy on a camera env
    wide = ActorCriticPolicy(obs_spaces(), 3, net_arch={"pi": [64] * 4, "vf": [64] * 4}).to(DEV)
    penv = _env(2, False)
    with pytest.raises(ValueError, match="reference's MLP"):
        evaluate_policy(wide, penv, 2, fused=True)
    trainable = ActorCriticPolicy(obs_spaces(cameras=True), 3).to(DEV)  # the Extractor's trainable CNNs
    with pytest.raises(ValueError, match="fusable_encoder"):
        DeviceEvaluator(trainable, env)
    with pytest.raises(ValueError, match="deterministic"):
        DeviceEvaluator(cam_pol, env).evaluate(2, deterministic=False)
    env.close()
    rgbd = BallbotVecEnv(2, device=DEV, disable_cameras=False, env_config={"camera": {"disable_rgb": False}})
    with pytest.raises(ValueError, match="RGB-D"):
        DeviceEvaluator(cam_pol, rgbd)
    rgbd.close()
    penv._host_reward = object()  # a host reward plugin: evaluated per step(), outside any graph
    with pytest.raises(ValueError, match="host plugin"):
        DeviceEvaluator(pro_pol, penv)
    penv._host_reward = None
    penv._log_on = True
    with pytest.raises(ValueError, match="per-episode logs"):
        DeviceEvaluator(pro_pol, penv)
    penv._log_on = False
    penv.close()


# ------------------------------------------------------------------ the command line
def test_cli_on_a_synthetic_zip(tmp_path):
    from ballbot_rl.evaluation import save_sb3_policy_pth

    pol = _policy(True, seed=9)
    save_sb3_policy_pth(pol, tmp_path / "policy.pth")
    data = {"num_timesteps": 4096, "n_envs": 3, "seed": 1, "terrain_type": "flat",
            "policy_kwargs": {":type:": "<class 'dict'>", ":serialized:": "!!! not base64 !!!",
                              "activation_fn": "<class 'torch.nn.modules.activation.LeakyReLU'>"}}
    path = tmp_path / "ppo_agent_4096_steps.zip"
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", json.dumps(data))
        z.write(tmp_path / "policy.pth", "policy.pth")
        z.writestr("_stable_baselines3_version", "2.6.0")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / "openballbot-rl_amd"),
                                                       os.environ.get("PYTHONPATH", "")]))
    results = []
    for extra in ([], ["--eager"]):
        out = tmp_path / f"result{len(extra)}.json"
        p = subprocess.run([sys.executable, "-m", "ballbot_rl.evaluation", "--model", str(path), "--terrain", "flat",
                            "--n-envs", "3", "--n-episodes", "5", "--seed", "4", "--out", str(out), *extra],
                           capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        r = json.loads(line)
        assert json.loads(out.read_text()) == r
        assert len(r["episode_rewards"]) == len(r["episode_lengths"]) == 5
        assert r["fused"] == (not extra) and r["num_timesteps"] == 4096 and r["n_envs"] == 3
        results.append(r)
    assert results[0]["episode_envs"] and "episode_envs" not in results[1]
