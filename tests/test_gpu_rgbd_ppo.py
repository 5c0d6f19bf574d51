"""GPU: the trainer and the pretraining on an RGB-D env (camera.disable_rgb: false) with frozen
4-channel encoders -- the twins of tests/test_gpu_ppo.py's depth-camera tests (same constructions and
tolerances) on 8 envs, 64x64 frames, with a random frozen 4-channel encoder (tests/rgbd_encoder_ref.py).

bb_ppo_mlp_step takes minibatches of a multiple of 256 rows, so the tests of the fused minibatch
run 8 envs x 64 (or 32) steps with batch_size 256.  The end-to-end case at n_steps 12, batch_size 48
runs the fused rollout and the captured autograd minibatch, whose frozen encoders are the fused
kernels too (the Extractor calls them); at 32 / 256 the minibatch is bb_ppo_mlp_step.

Snapshots of trainable parameters are taken with detach(): a plain clone() under grad keeps the
parameter's AccumulateGrad node alive, bound to the stream of the test body, and the update graph's
captured backward then runs that node on a stream outside the capture.  The first form of the
end-to-end test did that and the process ended in a segmentation fault at the end of the capture,
twice, whichever encoder path the update took.  There is no twin of
test_rollout_graph_matches_eager: the rollout graph holds the proprio rollout only."""
import copy

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rgbd_encoder_ref as G  # noqa: E402

DEV = "cuda:0"
RGBD = {"camera": {"disable_rgb": False}}


def _env(n=8, **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device=DEV, disable_cameras=False, env_config=RGBD, **kw)


def _ppo(env, **kw):
    from ballbot_rl.training.logger import CSVLogger
    from ballbot_rl.training.ppo import BatchedPPO

    return BatchedPPO(env, logger=CSVLogger(None, stdout=False), **kw)


def test_fused_encoder_in_extractor_rgbd(monkeypatch):
    """The camera policy's Extractor with a frozen 4-channel encoder: fused vs BB_FUSED_ENCODER=0."""
    from ballbot_rl.policies.mlp_policy import ActorCriticPolicy, obs_spaces

    pol = ActorCriticPolicy(obs_spaces(cameras=True, channels=4), frozen_encoder=G.random_frozen_encoder(4)).to(DEV)
    assert pol.features_extractor._frozen_keys == {"rgbd_0", "rgbd_1"}
    n = 256
    obs = {k: torch.randn(n, 3, device=DEV) for k in ("actions", "angular_vel", "motor_state", "orientation", "vel")}
    cams = torch.rand(n, 2, 4, 64, 64, device=DEV)
    obs["rgbd_0"], obs["rgbd_1"] = cams[:, 0], cams[:, 1]
    obs["relative_image_timestamp"] = torch.rand(n, 1, device=DEV) * 0.01
    pol.eval()
    with torch.no_grad():
        fused = pol.features_extractor(obs)
        monkeypatch.setenv("BB_FUSED_ENCODER", "0")
        plain = pol.features_extractor(obs)
    assert torch.allclose(fused, plain, rtol=1e-4, atol=2e-4), (fused - plain).abs().max()


def test_fused_camera_policy_matches_autograd_rgbd(monkeypatch):
    """The fused minibatch over the 56-d features (4-channel encoders in train mode, gathered through
    the permutation) vs the autograd minibatch on the same rollout, and the fused rollout step vs the
    torch one on the first env step."""
    enc = G.random_frozen_encoder(5)
    envs = [_env(8, seed=5) for _ in range(2)]
    models = []
    for fused, env in zip(("0", "1"), envs):
        monkeypatch.setenv("BB_PPO_FUSED", fused)
        m = _ppo(env, n_steps=64, batch_size=256, n_epochs=2, learning_rate=3e-4, seed=3,
                 frozen_encoder=copy.deepcopy(enc))
        m.collect_rollouts()
        models.append(m)
    assert models[0]._act_slots is False and models[1]._act_slots
    a, b = models[0].buf, models[1].buf
    assert a.depth.shape[2:] == (2, 4, 64, 64) and float(a.depth[0][:, :, :3].std()) > 0
    assert torch.equal(a.obs[0], b.obs[0]) and torch.equal(a.depth[0], b.depth[0])
    assert torch.allclose(a.actions[0], b.actions[0], rtol=1e-4, atol=1e-5), (a.actions[0] - b.actions[0]).abs().max()
    assert torch.allclose(a.values[0], b.values[0], rtol=1e-4, atol=1e-5)
    assert torch.allclose(a.log_probs[0], b.log_probs[0], rtol=1e-4, atol=1e-4)
    d0 = models[0].buf.flat()
    for fused, m in zip(("0", "1"), models):
        monkeypatch.setenv("BB_PPO_FUSED", fused)
        m.shuffle_gen.manual_seed(99)
        m._update({k: v.clone() for k, v in d0.items()})
    assert not models[0]._graphs.fused and models[1]._graphs.fused
    la, lb = models[0].logger.values, models[1].logger.values
    for k in ("train/policy_gradient_loss", "train/value_loss", "train/approx_kl"):
        assert la[k] == pytest.approx(lb[k], rel=5e-3, abs=1e-6), k
    for p, q in zip(models[0].policy.parameters(), models[1].policy.parameters()):
        diff = (p - q).abs()
        assert float((diff > 1e-5).float().mean()) < 1e-2, float(diff.max())
    for p, q in zip(models[0].policy.features_extractor.buffers(), models[1].policy.features_extractor.buffers()):
        assert torch.allclose(p.double(), q.double(), rtol=1e-4, atol=1e-5)
    for env in envs:
        env.close()


def test_camera_feature_cache_is_exact_rgbd(monkeypatch):
    """The camera rollout re-encodes only the envs whose cameras re-rendered this step; the rollout
    buffers equal a full re-encode every step."""
    enc = G.random_frozen_encoder(7)
    bufs = []
    for cache in ("1", "0"):
        monkeypatch.setenv("BB_ENC_CACHE", cache)
        env = _env(8, seed=9, max_ep_steps=5)
        m = _ppo(env, n_steps=14, batch_size=56, seed=3, frozen_encoder=copy.deepcopy(enc))
        m.collect_rollouts()
        assert m._act_slots
        bufs.append((m.buf.actions.clone(), m.buf.values.clone(), m.buf.rel_ts.clone()))
        env.close()
    (a0, v0, r0), (a1, v1, r1) = bufs
    assert float((r0 == 0).float().mean()) < 0.5  # most steps reuse cached features
    assert torch.equal(r0, r1) and torch.equal(a0, a1) and torch.equal(v0, v1)


def test_update_graph_build_keeps_encoder_statistics_rgbd():
    """Building the update graphs runs warm-up minibatches in train mode on a zero buffer: the frozen
    encoders' BatchNorm running statistics and num_batches_tracked must be exactly as before."""
    env = _env(8, seed=5)
    m = _ppo(env, n_steps=32, batch_size=256, n_epochs=1, seed=3, frozen_encoder=G.random_frozen_encoder(7))
    m.collect_rollouts()
    before = [b.clone() for b in m.policy.buffers()]
    assert len(before) > 0
    g = m._graphs_for(8 * 32)
    assert g.fused
    for b0, b1 in zip(before, m.policy.buffers()):
        assert torch.equal(b0, b1)
    env.close()


@pytest.mark.parametrize("n_steps,batch_size,fused_update", [(12, 48, False), (32, 256, True)])
def test_ppo_learns_one_iteration_on_rgbd(n_steps, batch_size, fused_update):
    """One PPO iteration on an RGB-D env with a frozen 4-channel encoder: the rollout is the fused one
    (both cameras' encoders and the policy step as HIP kernels); at 256 rows the minibatch is
    bb_ppo_mlp_step over features the encoders gathered in train mode; 48 rows are fewer than
    bb_ppo_mlp_step takes, so that update is the captured autograd minibatch, its frozen encoders
    still the fused kernels (BB_FUSED_ENCODER unset, no grad through them).  The conv weights stay,
    the BatchNorm running statistics move."""
    from ballbot_rl.training.ppo import fused_mlp_slots

    env = _env(8, seed=2)
    m = _ppo(env, n_steps=n_steps, batch_size=batch_size, n_epochs=1, seed=1, frozen_encoder=G.random_frozen_encoder(9))
    ext = m.policy.features_extractor
    assert ext._frozen_keys == {"rgbd_0", "rgbd_1"} and ext.extractors["rgbd_0"][0].in_channels == 4
    assert fused_mlp_slots(m, update=False) is not None
    enc0 = ext.extractors["rgbd_0"]
    w0 = [p.detach().clone() for p in enc0.parameters()]
    stats0 = [enc0[1].running_mean.clone(), enc0[4].running_var.clone(), enc0[8].running_mean.clone()]
    p0 = m.policy.action_net.weight.detach().clone()  # detach: see the module docstring
    m.learn(total_timesteps=8 * n_steps)
    assert m._act_slots                                  # the fused rollout
    assert m._graphs.fused == fused_update               # bb_ppo_mlp_step on the gathered features
    assert all(torch.equal(a, b) for a, b in zip(w0, enc0.parameters()))
    stats1 = [enc0[1].running_mean, enc0[4].running_var, enc0[8].running_mean]
    assert all(not torch.equal(a, b) for a, b in zip(stats0, stats1))
    assert int(enc0[1].num_batches_tracked) == 8 * n_steps // batch_size
    assert not torch.equal(p0, m.policy.action_net.weight)
    assert all(bool(torch.isfinite(p).all()) for p in m.policy.parameters())
    env.close()


def test_pretrain_on_rgbd_frames(tmp_path):
    from ballbot_rl.encoders import TinyAutoencoder, collect_camera_images, collect_depth_images, \
        load_frozen_encoder, train_autoencoder
    from ballbot_rl.encoders.models import fusable_encoder

    env = _env(16, seed=1, terrain_config={"type": "perlin", "config": {}}, n_terrains=4)
    imgs = collect_camera_images(env, 256, seed=1)
    assert imgs.shape == (256, 4, 64, 64) and float(imgs.min()) >= 0 and float(imgs[:, :3].max()) <= 1.0
    assert float(imgs[:, :3].std()) > 1e-3 and not torch.equal(imgs[:, 0], imgs[:, 2])  # colour, not grey
    depth = collect_depth_images(env, 64, seed=1)
    assert depth.shape == (64, 1, 64, 64)
    losses = []
    path = str(tmp_path / "enc.safetensors")
    train_autoencoder(TinyAutoencoder(64, 64, in_c=4), imgs, epochs=2, batch_size=64, save_path=path,
                      log=lambda s: losses.append(float(s.split("train_loss=")[1].split(",")[0]))
                      if "train_loss=" in s else None)
    assert len(losses) == 2 and losses[1] < losses[0]
    enc = load_frozen_encoder(path, device=DEV)
    assert enc[0].in_channels == 4 and fusable_encoder(enc)
    env.close()
