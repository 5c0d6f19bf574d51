"""Stable-Baselines3 checkpoints without a GPU (ballbot_rl/evaluation/sb3_zip.py).

The zips are written here in SB3's format: a state dict under SB3's key names whose three extractor
copies (features_extractor / pi_features_extractor / vf_features_extractor) share storage, saved
with torch.save as policy.pth; a `data` JSON whose objects carry ":serialized:" payloads that are
not valid base64 (so decoding one would raise: they must never be decoded); the version file.  One
extra test walks the reference's archived checkpoints where that directory exists."""
import io
import json
import os
import zipfile
from collections import OrderedDict
from pathlib import Path

import pytest
import torch
from torch import nn

from ballbot_rl.evaluation import load_sb3_policy, read_sb3_zip, save_sb3_policy_pth, sb3_state_dict

# where tools/compare_evals.py looks for the reference's archive too; BB_REFERENCE_ARCHIVE names another place
ARCHIVE = Path(os.environ.get("BB_REFERENCE_ARCHIVE", "/root/reference/outputs/experiments/archived_models"))
BAD_B64 = "!!! not base64 \x00 ???"


def _bn(t, n, g):
    return {f"{t}.weight": torch.rand(n, generator=g) + 0.5, f"{t}.bias": torch.randn(n, generator=g) * 0.1,
            f"{t}.running_mean": torch.randn(n, generator=g) * 0.1, f"{t}.running_var": torch.rand(n, generator=g) + 0.5,
            f"{t}.num_batches_tracked": torch.tensor(1234)}


def _encoder_tensors(g):
    d = {"0.weight": torch.randn(32, 1, 3, 3, generator=g) * 0.3, "0.bias": torch.randn(32, generator=g) * 0.1}
    d.update(_bn("1", 32, g))
    d.update({"3.weight": torch.randn(32, 32, 3, 3, generator=g) * 0.05, "3.bias": torch.randn(32, generator=g) * 0.1})
    d.update(_bn("4", 32, g))
    d.update({"7.weight": torch.randn(20, 8192, generator=g) * 0.01, "7.bias": torch.randn(20, generator=g) * 0.1})
    d.update(_bn("8", 20, g))
    return d


def sb3_state(width, seed=0):
    """A state dict as SB3's MultiInputPolicy saves it (reference train.py:39-56), random values."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    sd["log_std"] = torch.randn(3, generator=g) * 0.1
    if width == 56:
        enc = {f"extractors.rgbd_{c}.{k}": v for c in (0, 1) for k, v in _encoder_tensors(g).items()}
        for prefix in ("features_extractor.", "pi_features_extractor.", "vf_features_extractor."):
            for k, v in enc.items():
                sd[prefix + k] = v  # the same tensors: shared storage, as SB3 saves them
    for net in ("policy_net", "value_net"):
        for i, (o, k) in zip((0, 2, 4, 6), ((128, width), (128, 128), (128, 128), (128, 128))):
            sd[f"mlp_extractor.{net}.{i}.weight"] = torch.randn(o, k, generator=g) * 0.1
            sd[f"mlp_extractor.{net}.{i}.bias"] = torch.randn(o, generator=g) * 0.1
    sd["action_net.weight"] = torch.randn(3, 128, generator=g) * 0.1
    sd["action_net.bias"] = torch.randn(3, generator=g) * 0.1
    sd["value_net.weight"] = torch.randn(1, 128, generator=g) * 0.1
    sd["value_net.bias"] = torch.randn(1, generator=g) * 0.1
    return sd


def sb3_data(**over):
    d = {"policy_class": {":type:": "<class 'abc.ABCMeta'>", ":serialized:": BAD_B64, "__module__": "sb3"},
         "policy_kwargs": {":type:": "<class 'dict'>", ":serialized:": BAD_B64,
                           "activation_fn": "<class 'torch.nn.modules.activation.LeakyReLU'>",
                           "net_arch": "{'pi': [128, 128, 128, 128], 'vf': [128, 128, 128, 128]}"},
         "observation_space": {":type:": "<class 'gymnasium.spaces.dict.Dict'>", ":serialized:": BAD_B64},
         "learning_rate": {":type:": "<class 'function'>", ":serialized:": BAD_B64},
         "seed": {":type:": "<class 'int'>", ":serialized:": BAD_B64},  # a listed key, but not plain: dropped
         "num_timesteps": 800000, "_n_updates": 195, "n_steps": 2048, "batch_size": 256, "n_epochs": 5,
         "gamma": 0.99, "gae_lambda": 0.95, "ent_coef": 0.001, "vf_coef": 2.0, "max_grad_norm": 0.5, "target_kl": 0.3,
         "normalize_advantage": False, "n_envs": 10, "terrain_type": "flat", "verbose": 1}
    d.update(over)
    return d


def write_zip(path, sd, data=None, extra=()):
    buf = io.BytesIO()
    torch.save(sd, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", json.dumps(sb3_data() if data is None else data))
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("policy.optimizer.pth", b"not a torch file: never opened")
        z.writestr("pytorch_variables.pth", b"not a torch file: never opened")
        z.writestr("_stable_baselines3_version", "2.6.0")
        for name, body in extra:
            z.writestr(name, body)
    return path


class SB3Twin(nn.Module):
    """Torch modules under SB3's own attribute names, assembled from the same tensors."""

    def __init__(self, sd, width):
        super().__init__()
        from ballbot_rl.policies.mlp_policy import depth_cnn

        def mlp():
            return nn.Sequential(nn.Linear(width, 128), nn.LeakyReLU(), nn.Linear(128, 128), nn.LeakyReLU(),
                                 nn.Linear(128, 128), nn.LeakyReLU(), nn.Linear(128, 128), nn.LeakyReLU())

        self.mlp_extractor = nn.Module()
        self.mlp_extractor.policy_net, self.mlp_extractor.value_net = mlp(), mlp()
        self.action_net, self.value_net = nn.Linear(128, 3), nn.Linear(128, 1)
        self.log_std = nn.Parameter(torch.zeros(3))
        if width == 56:
            self.features_extractor = nn.Module()
            self.features_extractor.extractors = nn.ModuleDict({"rgbd_0": depth_cnn(1, 64, 64),
                                                                "rgbd_1": depth_cnn(1, 64, 64)})
        own = {k: v for k, v in sd.items() if not k.startswith(("pi_features", "vf_features"))}
        self.load_state_dict(own, strict=True)
        self.eval()

    def forward(self, obs15, depth=None, rel_ts=None):
        f = obs15
        if depth is not None:  # the Dict space's sorted key order
            ex = self.features_extractor.extractors
            f = torch.cat([obs15[:, 0:12], rel_ts.reshape(-1, 1), ex["rgbd_0"](depth[:, 0:1]),
                           ex["rgbd_1"](depth[:, 1:2]), obs15[:, 12:15]], dim=1)
        return (self.action_net(self.mlp_extractor.policy_net(f)),
                self.value_net(self.mlp_extractor.value_net(f)).squeeze(-1))


@pytest.mark.parametrize("width", [15, 56])
def test_loaded_policy_equals_modules_under_sb3_names(tmp_path, width):
    from ballbot_rl.encoders.models import fusable_encoder
    from ballbot_rl.training.ppo import policy_obs

    sd = sb3_state(width, seed=width)
    path = write_zip(tmp_path / "ppo_agent_800000_steps.zip", sd)
    policy, meta = load_sb3_policy(path, "cpu")
    assert meta["num_timesteps"] == 800000 and meta["_n_updates"] == 195 and meta["n_envs"] == 10
    assert meta["terrain_type"] == "flat" and meta["normalize_advantage"] is False and meta["target_kl"] == 0.3
    assert meta["_stable_baselines3_version"] == "2.6.0"
    assert "seed" not in meta and "policy_class" not in meta and "verbose" not in meta
    assert policy.features_extractor.features_dim == width
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(5, 15, generator=g)
    twin = SB3Twin(sd, width)
    policy.eval()
    with torch.no_grad():
        if width == 56:
            encs = [policy.features_extractor.extractors[k] for k in ("rgbd_0", "rgbd_1")]
            assert all(fusable_encoder(e) and not e.training for e in encs)
            depth, ts = torch.rand(5, 2, 64, 64, generator=g), torch.tensor([0.0, 0.002, 0.004, 0.0, 0.01])
            mean, value = policy._heads(policy_obs(obs, depth, ts))
            want = twin(obs, depth, ts)
        else:
            mean, value = policy._heads(obs)
            want = twin(obs)
    assert torch.equal(mean, want[0]) and torch.equal(value, want[1])
    assert mean.abs().max() > 0
    # the inverse map reproduces every tensor, the three extractor copies sharing storage
    back = sb3_state_dict(policy)
    assert list(back.keys()) == list(sd.keys())
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
    if width == 56:
        k = "extractors.rgbd_1.7.weight"
        assert back["features_extractor." + k].data_ptr() == back["pi_features_extractor." + k].data_ptr() \
            == back["vf_features_extractor." + k].data_ptr()


@pytest.mark.parametrize("width", [15, 56])
def test_saved_policy_pth_round_trips(tmp_path, width):
    policy, _ = load_sb3_policy(write_zip(tmp_path / "a.zip", sb3_state(width, seed=3)), "cpu")
    save_sb3_policy_pth(policy, tmp_path / "policy.pth")
    sd = torch.load(tmp_path / "policy.pth", map_location="cpu", weights_only=True)
    ref = sb3_state(width, seed=3)
    assert list(sd.keys()) == list(ref.keys())
    assert all(torch.equal(sd[k], ref[k]) for k in ref)
    SB3Twin(sd, width)  # model.policy.load_state_dict's strictness, minus the aliases
    if width == 56:  # the copies still share storage in the file
        k = "extractors.rgbd_0.3.weight"
        assert sd["features_extractor." + k].data_ptr() == sd["vf_features_extractor." + k].data_ptr()
    again, _ = load_sb3_policy(write_zip(tmp_path / "b.zip", sd), "cpu")
    for (k, v), (k2, v2) in zip(policy.state_dict().items(), again.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)


def test_read_never_opens_what_it_must_not(tmp_path):
    """The optimiser and variable files are garbage, every ":serialized:" payload is invalid base64:
    reading succeeds and returns plain values only."""
    sd, meta = read_sb3_zip(write_zip(tmp_path / "best_model.zip", sb3_state(15)))
    assert set(meta) <= {"num_timesteps", "_n_updates", "n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda",
                         "ent_coef", "vf_coef", "max_grad_norm", "target_kl", "normalize_advantage", "seed", "n_envs",
                         "terrain_type", "_stable_baselines3_version", "activation_fn"}
    assert all(not isinstance(v, (dict, list)) for v in meta.values())
    assert "LeakyReLU" in meta["activation_fn"]
    assert all(isinstance(v, torch.Tensor) and v.device.type == "cpu" for v in sd.values())


def test_documented_errors(tmp_path):
    sd = sb3_state(56, seed=5)
    # a pi_ copy that differs
    bad = OrderedDict(sd)
    k = "pi_features_extractor.extractors.rgbd_0.1.running_mean"
    bad[k] = sd[k].clone()
    bad[k][3] += 1e-3
    with pytest.raises(ValueError, match="pi_features_extractor.extractors.rgbd_0.1.running_mean"):
        load_sb3_policy(write_zip(tmp_path / "a.zip", bad))
    # a vf_ copy with another counter
    bad = OrderedDict(sd)
    k = "vf_features_extractor.extractors.rgbd_1.8.num_batches_tracked"
    bad[k] = torch.tensor(7)
    with pytest.raises(ValueError, match="vf_features_extractor.extractors.rgbd_1.8.num_batches_tracked"):
        load_sb3_policy(write_zip(tmp_path / "b.zip", bad))
    # a missing key, named by its SB3 name
    bad = OrderedDict((k, v) for k, v in sd.items() if k != "mlp_extractor.value_net.4.bias")
    with pytest.raises(ValueError, match="missing key 'mlp_extractor.value_net.4.bias'"):
        load_sb3_policy(write_zip(tmp_path / "c.zip", bad))
    bad = OrderedDict((k, v) for k, v in sd.items() if k != "features_extractor.extractors.rgbd_0.4.running_var")
    with pytest.raises(ValueError, match="rgbd_0.4.running_var"):
        load_sb3_policy(write_zip(tmp_path / "c2.zip", bad))
    # an extra key
    bad = OrderedDict(sd)
    bad["mlp_extractor.policy_net.8.weight"] = torch.zeros(128, 128)
    with pytest.raises(ValueError, match="unexpected key 'mlp_extractor.policy_net.8.weight'"):
        load_sb3_policy(write_zip(tmp_path / "d.zip", bad))
    # a 57-wide trunk
    bad = sb3_state(15)
    bad["mlp_extractor.policy_net.0.weight"] = torch.zeros(128, 57)
    with pytest.raises(ValueError, match="mlp_extractor.policy_net.0.weight"):
        load_sb3_policy(write_zip(tmp_path / "e.zip", bad))
    # a wrong shape further in
    bad = sb3_state(15)
    bad["action_net.weight"] = torch.zeros(4, 128)
    with pytest.raises(ValueError, match="action_net.weight"):
        load_sb3_policy(write_zip(tmp_path / "f.zip", bad))
    # an activation that cannot be LeakyReLU
    data = sb3_data()
    data["policy_kwargs"]["activation_fn"] = "<class 'torch.nn.modules.activation.Tanh'>"
    with pytest.raises(ValueError, match="policy_kwargs.activation_fn"):
        load_sb3_policy(write_zip(tmp_path / "g.zip", sb3_state(15), data=data))
    # not a zip at all
    (tmp_path / "h.zip").write_bytes(b"safetensors or anything else")
    with pytest.raises(ValueError, match="not an SB3 zip"):
        read_sb3_zip(tmp_path / "h.zip")
    # a policy.pth that is not a weights-only state dict: an object the restricted unpickler refuses, garbage bytes
    for tag, body in (("obj", {"log_std": torch.zeros(3), "hook": zipfile.ZipFile}), ("junk", None)):
        buf = io.BytesIO()
        if body is None:
            buf.write(b"not a torch file at all")
        else:
            torch.save(body, buf)
        with zipfile.ZipFile(tmp_path / f"j_{tag}.zip", "w") as z:
            z.writestr("data", json.dumps(sb3_data()))
            z.writestr("policy.pth", buf.getvalue())
        with pytest.raises(ValueError, match="policy.pth"):
            read_sb3_zip(tmp_path / f"j_{tag}.zip")
    # a zip without a policy
    with zipfile.ZipFile(tmp_path / "i.zip", "w") as z:
        z.writestr("data", "{}")
    with pytest.raises(ValueError, match="policy.pth"):
        read_sb3_zip(tmp_path / "i.zip")


def test_batched_ppo_resumes_from_a_zip(tmp_path):
    from fake_env import FakeEnv

    from ballbot_rl.training.ppo import BatchedPPO

    sd = sb3_state(15, seed=9)
    path = write_zip(tmp_path / "best_model.zip", sd)
    ppo = BatchedPPO(FakeEnv(4), n_steps=8, batch_size=16, seed=1)
    before = {k: v.clone() for k, v in ppo.policy.state_dict().items()}
    held = [p for g in ppo.optimizer.param_groups for p in g["params"]]
    ppo.load_policy(str(path))
    want, _ = load_sb3_policy(path, "cpu")
    got = ppo.policy.state_dict()
    assert any(not torch.equal(before[k], got[k]) for k in got)
    for k, v in want.state_dict().items():
        assert torch.equal(got[k], v), k
    # the optimiser still steps the very tensors that now hold the zip's values (a flat buffer's views on the GPU)
    now = [p for g in ppo.optimizer.param_groups for p in g["params"]]
    assert [id(p) for p in held] == [id(p) for p in now] == [id(p) for p in ppo.policy.parameters()]
    flat = getattr(ppo.optimizer, "flat", None)
    vec = nn.utils.parameters_to_vector(now).detach()
    assert torch.equal(vec, nn.utils.parameters_to_vector(list(want.parameters())).detach())
    if flat is not None:
        for p, off in zip(ppo.optimizer.params, ppo.optimizer.offsets):
            assert torch.equal(flat[off:off + p.numel()], p.detach().reshape(-1))
    # a camera zip does not fit a proprio trainer: named key, nothing half-loaded
    with pytest.raises(ValueError, match="mlp_extractor.policy_net.0.weight|features_extractor"):
        ppo.load_policy(str(write_zip(tmp_path / "cam.zip", sb3_state(56))))
    for k, v in want.state_dict().items():
        assert torch.equal(ppo.policy.state_dict()[k], v), k


_ZIPS = sorted(ARCHIVE.glob("**/*.zip")) if ARCHIVE.is_dir() else []  # twelve in the reference's archive


@pytest.mark.skipif(not _ZIPS, reason="the reference's archived checkpoints are not on this machine")
def test_the_archive_holds_twelve_zips():
    assert len(_ZIPS) == 12, [str(p.relative_to(ARCHIVE)) for p in _ZIPS]


@pytest.mark.skipif(not _ZIPS, reason="the reference's archived checkpoints are not on this machine")
@pytest.mark.parametrize("path", _ZIPS, ids=lambda p: "/".join(p.parts[-3:]) if isinstance(p, Path) else str(p))
def test_archived_reference_checkpoints_load(path):
    policy, meta = load_sb3_policy(path, "cpu")
    assert policy.features_extractor.features_dim == 56
    assert tuple(policy.policy_net[0].weight.shape) == (128, 56)
    with zipfile.ZipFile(path) as z:
        data = json.loads(z.read("data"))
    assert meta["num_timesteps"] == data["num_timesteps"] and meta["n_envs"] == data["n_envs"]
    assert meta["_stable_baselines3_version"] == "2.6.0"
    stem = path.stem
    if stem.startswith("ppo_agent_"):
        assert meta["num_timesteps"] == int(stem.split("_")[2])
    bn = policy.features_extractor.extractors["rgbd_0"][1]
    assert int(bn.num_batches_tracked) > 0 and not bn.training and not bn.weight.requires_grad
