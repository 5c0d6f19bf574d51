"""Host, no GPU: the RGB-D (4-channel) frozen encoder through the Python layers -- the autoencoder
module, the safetensors round trip, fusable_encoder, the Extractor and reference_mlp_tensors, the
checkpoint loaders' channel detection, and the C-ABI's declaration."""
import json

import pytest
import torch

from rgbd_encoder_ref import random_frozen_encoder

from ballbot_rl.encoders.models import TinyAutoencoder, fusable_encoder, load_frozen_encoder, save_encoder


def test_autoencoder_honours_in_c():
    m = TinyAutoencoder(64, 64, in_c=4)
    assert m.encoder[0].in_channels == 4 and tuple(m.encoder[0].weight.shape) == (32, 4, 3, 3)
    x = torch.rand(2, 4, 64, 64, generator=torch.Generator().manual_seed(0))
    y = m(x)
    assert tuple(y.shape) == (2, 4, 64, 64)
    torch.nn.functional.mse_loss(y, x).backward()
    g = m.encoder[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and all(float(g[:, c].abs().max()) > 0 for c in range(4))
    assert m.decoder[-2].out_channels == 4


def test_in_c_1_is_the_module_as_it_was():
    F, flat = 32, 32 * 16 * 16
    want = {"encoder.0.weight": (F, 1, 3, 3), "encoder.0.bias": (F,), "encoder.3.weight": (F, F, 3, 3),
            "encoder.3.bias": (F,), "encoder.7.weight": (20, flat), "encoder.7.bias": (20,),
            "decoder.0.weight": (flat, 20), "decoder.0.bias": (flat,), "decoder.4.weight": (F, F, 3, 3),
            "decoder.4.bias": (F,), "decoder.7.weight": (F, 1, 3, 3), "decoder.7.bias": (1,)}
    for name, nf in (("encoder.1", F), ("encoder.4", F), ("encoder.8", 20), ("decoder.1", flat), ("decoder.5", F)):
        want.update({f"{name}.weight": (nf,), f"{name}.bias": (nf,), f"{name}.running_mean": (nf,),
                     f"{name}.running_var": (nf,), f"{name}.num_batches_tracked": ()})
    for m in (TinyAutoencoder(64, 64), TinyAutoencoder(64, 64, in_c=1)):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want


def test_save_load_round_trip_keeps_in_c(tmp_path):
    m = TinyAutoencoder(64, 64, in_c=4)
    path = str(tmp_path / "enc4.safetensors")
    p_sum = save_encoder(m, path)
    meta = json.loads(open(path + ".json").read())
    assert meta["in_c"] == 4 and meta["p_sum"] == p_sum
    enc = load_frozen_encoder(path)  # raises when the p_sum check fails
    assert enc[0].in_channels == 4 and not enc.training and fusable_encoder(enc)
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), m.encoder.state_dict().values()))
    # a sidecar from before RGB-D encoders has no "in_c": a 1-channel encoder
    m1 = TinyAutoencoder(64, 64)
    path1 = str(tmp_path / "enc1.safetensors")
    p1 = save_encoder(m1, path1)
    with open(path1 + ".json", "w") as f:
        json.dump({"H": 64, "W": 64, "out_sz": 20, "p_sum": p1}, f)
    enc1 = load_frozen_encoder(path1)
    assert enc1[0].in_channels == 1 and fusable_encoder(enc1)


def test_fusable_encoder_takes_one_or_four_channels():
    assert fusable_encoder(random_frozen_encoder(0, in_c=4))
    assert fusable_encoder(random_frozen_encoder(0, in_c=1))
    assert not fusable_encoder(random_frozen_encoder(0, in_c=3))
    trainable = random_frozen_encoder(0, in_c=4)
    trainable[0].weight.requires_grad = True
    assert not fusable_encoder(trainable)
    mom = random_frozen_encoder(0, in_c=4)
    mom[4].momentum = 0.2
    assert not fusable_encoder(mom)


def test_extractor_and_mlp_tensors_on_rgbd_spaces():
    from ballbot_rl.policies import ActorCriticPolicy, obs_spaces
    from ballbot_rl.training.ppo import camera_images, reference_mlp_tensors

    pol = ActorCriticPolicy(obs_spaces(cameras=True, channels=4), 3, frozen_encoder=random_frozen_encoder(1, in_c=4))
    ext = pol.features_extractor
    assert ext._frozen_keys == {"rgbd_0", "rgbd_1"} and ext.features_dim == 56
    tensors = reference_mlp_tensors(pol, True)
    assert tensors is not None and len(tensors) == 21
    with pytest.raises(ValueError, match="Channel mismatch: Encoder expects 1 channels"):
        ActorCriticPolicy(obs_spaces(cameras=True, channels=4), 3, frozen_encoder=random_frozen_encoder(1, in_c=1))
    with pytest.raises(ValueError, match="Channel mismatch: Encoder expects 4 channels"):
        ActorCriticPolicy(obs_spaces(cameras=True, channels=1), 3, frozen_encoder=random_frozen_encoder(1, in_c=4))
    # the one helper the trainer's encoder call sites share
    rgbd, depth = torch.zeros(3, 2, 4, 64, 64), torch.zeros(3, 2, 64, 64)
    v = camera_images(rgbd, 1)
    assert tuple(v.shape) == (3, 4, 64, 64) and v.data_ptr() == rgbd[:, 1].data_ptr() and v.stride(0) == 2 * 4 * 4096
    v = camera_images(depth, 1)
    assert tuple(v.shape) == (3, 1, 64, 64) and v.data_ptr() == depth[:, 1].data_ptr()


def test_fused_forward_refuses_another_channel_count():
    from ballbot_rl.encoders.models import fused_encoder_forward

    with pytest.raises(ValueError, match="4-channel"):
        fused_encoder_forward(random_frozen_encoder(2, in_c=4), torch.zeros(2, 1, 64, 64))
    with pytest.raises(ValueError, match="1-channel"):
        fused_encoder_forward(random_frozen_encoder(2, in_c=1), torch.zeros(2, 4, 64, 64))


def _sb3_state_4ch(seed=0):
    from test_sb3_zip import sb3_state

    sd = sb3_state(56, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for c in (0, 1):
        w = torch.randn(32, 4, 3, 3, generator=g) * 0.3
        for prefix in ("features_extractor.", "pi_features_extractor.", "vf_features_extractor."):
            sd[f"{prefix}extractors.rgbd_{c}.0.weight"] = w
    return sd


def test_checkpoint_loaders_build_the_policy_for_four_channels(tmp_path):
    from safetensors.torch import save_file
    from test_sb3_zip import write_zip

    from ballbot_rl.evaluation import load_sb3_policy, sb3_state_dict
    from ballbot_rl.evaluation.__main__ import _load_policy
    from ballbot_rl.training.ppo import policy_obs

    sd = _sb3_state_4ch(3)
    policy, _ = load_sb3_policy(write_zip(tmp_path / "rgbd.zip", sd), "cpu")
    encs = [policy.features_extractor.extractors[k] for k in ("rgbd_0", "rgbd_1")]
    assert all(e[0].in_channels == 4 and fusable_encoder(e) and not e.training for e in encs)
    assert policy.features_extractor._frozen_keys == {"rgbd_0", "rgbd_1"}
    back = sb3_state_dict(policy)
    assert list(back.keys()) == list(sd.keys()) and all(torch.equal(back[k], v) for k, v in sd.items())
    # the same policy as this project's safetensors, through the CLI's loader
    path = str(tmp_path / "rgbd.safetensors")
    save_file({k: v.contiguous() for k, v in policy.state_dict().items()}, path)
    again, _ = _load_policy(path, torch.device("cpu"))
    assert again.features_extractor.extractors["rgbd_1"][0].in_channels == 4
    g = torch.Generator().manual_seed(5)
    obs, frames, ts = torch.randn(3, 15, generator=g), torch.rand(3, 2, 4, 64, 64, generator=g), torch.zeros(3)
    policy.eval()
    again.eval()
    with torch.no_grad():
        a, b = policy._heads(policy_obs(obs, frames, ts)), again._heads(policy_obs(obs, frames, ts))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0].abs().max()) > 0
    # a first conv of another width is named
    bad = _sb3_state_4ch(3)
    for k in [k for k in bad if k.endswith("rgbd_0.0.weight")]:
        bad[k] = torch.zeros(32, 3, 3, 3)
    with pytest.raises(ValueError, match="1 .depth. or 4 .RGB-D. channels"):
        load_sb3_policy(write_zip(tmp_path / "bad.zip", bad), "cpu")


def test_abi_declares_the_rgbd_encoder():
    from ballbot_gym import _native as native

    assert {"bb_rgbd_encoder", "bb_rgbd_encoder_workspace_bytes"} <= set(native.EXPORTS)
    assert "bb_encoder_rgbd.hip" in native.HIP_SOURCES and native.ABI_VERSION == 21
    header = (native.INCLUDE / "ballbot_mi355x.h").read_text()
    assert "int bb_rgbd_encoder(const bb_encoder_params* params" in header
