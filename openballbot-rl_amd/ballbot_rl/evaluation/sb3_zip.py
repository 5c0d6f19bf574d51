"""Stable-Baselines3 checkpoints (`best_model.zip`, `ppo_agent_<N>_steps.zip`) as this project's policy.

An SB3 zip holds `data` (JSON whose objects are cloudpickled, base64, under ":serialized:"),
`policy.pth` (the policy's state dict), `policy.optimizer.pth`, `pytorch_variables.pth` and
`_stable_baselines3_version`.  Only what can be read without executing anything is read:
* `policy.pth` through torch.load(map_location="cpu", weights_only=True);
* `data` as JSON, keeping the plain values of PLAIN_KEYS (an entry with a ":serialized:" field is
  never decoded, let alone unpickled);
* the version file.
The optimiser state and `pytorch_variables.pth` are not opened.

Key map (SB3 MultiInputPolicy as the reference builds it, train.py:39-56 -> ActorCriticPolicy):
    mlp_extractor.policy_net.{0,2,4,6}.*             policy_net.{0,2,4,6}.*
    mlp_extractor.value_net.{0,2,4,6}.*              value_net_trunk.{0,2,4,6}.*
    action_net.*, value_net.*, log_std               unchanged
    features_extractor.extractors.rgbd_{0,1}.{0,1,3,4,7,8}.*   unchanged (the Extractor's per-camera
                                                     modules, depth_cnn's layout)
    pi_features_extractor.* / vf_features_extractor.*  SB3's aliases of features_extractor.* (one
                                                     shared extractor): must equal it bit for bit
The observation space follows from the first trunk layer's input width: 15 = the proprio keys,
56 = proprio + relative_image_timestamp + 2 x 20 camera features.  The encoders come from the zip
(their BatchNorm statistics moved during training), frozen and in eval mode.  Their input
channels follow from features_extractor.extractors.rgbd_0.0.weight: 1 (depth frames) or 4 (RGB-D
frames, camera.disable_rgb: false).
"""
from __future__ import annotations

import io
import json
import pickle
import zipfile
from collections import OrderedDict
from typing import Dict, Tuple

import torch

PLAIN_KEYS = ("num_timesteps", "_n_updates", "n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "ent_coef",
              "vf_coef", "max_grad_norm", "target_kl", "normalize_advantage", "seed", "n_envs", "terrain_type")
_PLAIN_TYPES = (bool, int, float, str, type(None))
_FE = "features_extractor."
_ALIASES = ("pi_features_extractor.", "vf_features_extractor.")
_TRUNKS = (("mlp_extractor.policy_net.", "policy_net."), ("mlp_extractor.value_net.", "value_net_trunk."))
_FIRST = "mlp_extractor.policy_net.0.weight"


def read_sb3_zip(path) -> Tuple[Dict[str, torch.Tensor], Dict[str, object]]:
    """-> (the state dict of policy.pth on the CPU, meta).  meta holds the plain values of
    PLAIN_KEYS found in `data`, "_stable_baselines3_version", and "activation_fn": the class name
    SB3 wrote beside policy_kwargs' payload (a plain string; None when absent)."""
    try:
        zf = zipfile.ZipFile(str(path))
    except (zipfile.BadZipFile, IsADirectoryError) as e:
        raise ValueError(f"{path}: not an SB3 zip ({e})") from e
    with zf:
        names = set(zf.namelist())
        for need in ("policy.pth", "data"):
            if need not in names:
                raise ValueError(f"{path}: not an SB3 zip (no {need!r} inside)")
        try:
            sd = torch.load(io.BytesIO(zf.read("policy.pth")), map_location="cpu", weights_only=True)
        except (pickle.UnpicklingError, RuntimeError, EOFError, KeyError, AttributeError) as e:
            # what the weights-only unpickler rejects (anything but tensors and plain containers) or cannot parse
            raise ValueError(f"{path}: policy.pth is not a weights-only state dict ({e})") from e
        try:
            data = json.loads(zf.read("data").decode())
        except (UnicodeDecodeError, json.JSONDecodeError) as e:
            raise ValueError(f"{path}: 'data' is not JSON ({e})") from e
        version = zf.read("_stable_baselines3_version").decode().strip() \
            if "_stable_baselines3_version" in names else None
    if not isinstance(sd, dict) or not isinstance(data, dict):
        raise ValueError(f"{path}: policy.pth / data do not hold dictionaries")
    bad = [k for k, v in sd.items() if not isinstance(v, torch.Tensor)]
    if bad:
        raise ValueError(f"{path}: policy.pth entry {bad[0]!r} is not a tensor")
    meta: Dict[str, object] = {}
    for k in PLAIN_KEYS:
        v = data.get(k)
        if k in data and isinstance(v, _PLAIN_TYPES):  # a dict (":serialized:" or not) is never kept
            meta[k] = v
    kw = data.get("policy_kwargs")
    act = kw.get("activation_fn") if isinstance(kw, dict) else None
    meta["activation_fn"] = act if isinstance(act, str) else None
    meta["_stable_baselines3_version"] = version
    return OrderedDict(sd), meta


def _to_project(sd: Dict[str, torch.Tensor], meta: Dict[str, object]) -> Tuple["OrderedDict", int]:
    """SB3's state dict under this project's names (aliases checked and dropped) -> (state, width)."""
    act = meta.get("activation_fn")
    if act is not None and "LeakyReLU" not in act:  # the trunks here are LeakyReLU(0.01), torch's default slope
        raise ValueError(f"policy_kwargs.activation_fn is {act!r}: the policy's trunks must be LeakyReLU(0.01)")
    if _FIRST not in sd:
        raise ValueError(f"missing key {_FIRST!r}")
    w0 = sd[_FIRST]
    width = int(w0.shape[1]) if w0.dim() == 2 else -1
    if width not in (15, 56):
        raise ValueError(f"{_FIRST!r} has shape {tuple(w0.shape)}: the trunk's input must be 15 (proprio) or 56 "
                         "(proprio + relative_image_timestamp + 2 x 20 camera features) wide")
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        alias = next((a for a in _ALIASES if k.startswith(a)), None)
        if alias is not None:
            base = _FE + k[len(alias):]
            if base not in sd:
                raise ValueError(f"unexpected key {k!r} (no {base!r} to be a copy of)")
            b = sd[base]
            if b.shape != v.shape or b.dtype != v.dtype or not torch.equal(b, v):
                raise ValueError(f"{k!r} differs from {base!r}: the extractor copies must be identical")
            continue
        trunk = next(((s, p) for s, p in _TRUNKS if k.startswith(s)), None)
        out[(trunk[1] + k[len(trunk[0]):]) if trunk else k] = v
    return out, width


_CONV1 = _FE + "extractors.rgbd_0.0.weight"


def encoder_channels(state: Dict[str, torch.Tensor]) -> int:
    """Input channels of a camera policy's encoders, from the first conv's weight [32, C, 3, 3] in a
    state dict (SB3's names or this project's: the key is the same): 1 or 4; 1 when the key is
    absent (the key check names it as missing afterwards)."""
    w = state.get(_CONV1)
    if w is None:
        return 1
    c = int(w.shape[1]) if w.dim() == 4 else -1
    if c not in (1, 4):
        raise ValueError(f"{_CONV1!r} has shape {tuple(w.shape)}: the encoders read 1 (depth) or 4 (RGB-D) channels")
    return c


def _empty_policy(width: int, channels: int = 1):
    from ballbot_rl.encoders.models import TinyAutoencoder
    from ballbot_rl.policies.mlp_policy import ActorCriticPolicy, obs_spaces

    if width == 15:
        return ActorCriticPolicy(obs_spaces(), 3, ortho_init=False)
    # depth_cnn's layout (4 input planes for RGB-D frames); the Extractor copies it per camera, frozen
    enc = TinyAutoencoder(64, 64, in_c=channels).encoder
    return ActorCriticPolicy(obs_spaces(cameras=True, channels=channels), 3, frozen_encoder=enc, ortho_init=False)


def _check_keys(state: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], back=lambda k: k) -> None:
    for k, t in want.items():
        if k not in state:
            raise ValueError(f"missing key {back(k)!r}")
        if tuple(state[k].shape) != tuple(t.shape) or state[k].dtype != t.dtype:
            raise ValueError(f"key {back(k)!r}: expected {t.dtype} {tuple(t.shape)}, got {state[k].dtype} "
                             f"{tuple(state[k].shape)}")
    for k in state:
        if k not in want:
            raise ValueError(f"unexpected key {back(k)!r}")


def _sb3_name(k: str) -> str:
    for s, p in _TRUNKS:
        if k.startswith(p):
            return s + k[len(p):]
    return k


def policy_state_from_sb3(sd: Dict[str, torch.Tensor], meta: Dict[str, object], policy=None):
    """The state dict `policy.load_state_dict` takes, checked key by key against `policy` (None: a
    fresh policy of the width the zip implies) -> (state, policy)."""
    state, width = _to_project(sd, meta)
    if policy is None:
        policy = _empty_policy(width, encoder_channels(state) if width == 56 else 1)
    _check_keys(state, policy.state_dict(), _sb3_name)
    return state, policy


def load_sb3_policy(path, device="cpu"):
    """-> (ActorCriticPolicy on `device` holding the zip's tensors, meta).  The camera policy's two
    encoders are the zip's, with requires_grad off and in eval mode (fusable_encoder accepts them)."""
    sd, meta = read_sb3_zip(path)
    state, policy = policy_state_from_sb3(sd, meta)
    policy.load_state_dict(state, strict=True)
    policy = policy.to(device)
    for m in policy.features_extractor.extractors.values():
        m.eval()
        for p in m.parameters():
            p.requires_grad = False
    return policy, meta


def sb3_state_dict(policy) -> "OrderedDict[str, torch.Tensor]":
    """The policy's tensors under SB3's names and in SB3's order, the pi_/vf_ extractor entries
    being the very tensors of features_extractor.* (shared storage, as SB3 saves them)."""
    own = policy.state_dict()
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    if "log_std" in own:
        out["log_std"] = own["log_std"]
    fe = [(k, v) for k, v in own.items() if k.startswith(_FE)]
    for prefix in (_FE,) + _ALIASES:
        for k, v in fe:
            out[prefix + k[len(_FE):]] = v
    for k, v in own.items():
        if k == "log_std" or k.startswith(_FE):
            continue
        out[_sb3_name(k)] = v
    return out


def save_sb3_policy_pth(policy, path) -> None:
    """Write the `policy.pth` of an SB3 zip (what model.policy.load_state_dict(torch.load(...))
    takes on the reference's side).  A whole zip is not written: its `data` needs pickled objects."""
    host: Dict[int, torch.Tensor] = {}  # one host copy per tensor, so that the aliases still share storage
    out = OrderedDict()
    for k, v in sb3_state_dict(policy).items():
        if id(v) not in host:
            host[id(v)] = v.detach().cpu()
        out[k] = host[id(v)]
    torch.save(out, str(path))
