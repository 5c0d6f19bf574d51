"""Inputs and modules for the RGB-D encoder tests (tests/test_rgbd_encoder_host.py and the
tests/test_gpu_rgbd_*.py files): RGB-D-like images, a random frozen 4-channel encoder, and the
tensor list bb_encoder_params takes."""
import torch

import ppo_ref as R


def rgbd_like_images(n: int, seed: int) -> torch.Tensor:
    """[n][4][64][64] frames as an onboard RGB-D camera gives them.  D plane: ppo_ref's depth-like
    images (half the pixels exactly 1.0).  Colour planes: each image is cut into a few regions by
    two random lines, every region takes one of six flat colours, times one of four shading factors
    per region -- piecewise constant, so most neighbouring pixels are exactly equal, channel values
    in [0, 1], and no image is constant."""
    g = torch.Generator().manual_seed(seed)
    palette = torch.tensor([[0.20, 0.30, 0.40], [0.85, 0.85, 0.80], [0.55, 0.35, 0.20], [0.10, 0.60, 0.15],
                            [0.90, 0.20, 0.10], [0.30, 0.30, 0.90]])
    shades = torch.tensor([1.0, 0.75, 0.5, 0.25])
    lin = torch.linspace(-1, 1, 64)
    yy, xx = lin.view(1, 64, 1), lin.view(1, 1, 64)
    region = torch.zeros(n, 64, 64, dtype=torch.int64)
    for bit in range(2):
        ang = 2 * torch.pi * torch.rand(n, 1, 1, generator=g)
        off = 0.6 * torch.rand(n, 1, 1, generator=g) - 0.3
        region += ((torch.cos(ang) * xx + torch.sin(ang) * yy) > off).long() << bit
    first = torch.randint(0, 6, (n, 1), generator=g)
    colour = (first + torch.arange(4).view(1, 4)) % 6          # four different colours per image
    shade = torch.randint(0, 4, (n, 4), generator=g)
    rgb_of_region = palette[colour] * shades[shade].unsqueeze(-1)  # [n][4][3]
    rgb = torch.gather(rgb_of_region, 1, region.view(n, -1, 1).expand(-1, -1, 3)).view(n, 64, 64, 3).permute(0, 3, 1, 2)
    img = torch.cat([rgb, R.depth_like_images(n, seed + 1).unsqueeze(1)], 1).contiguous()
    same = (img[:, :3, :, 1:] == img[:, :3, :, :-1]).float().mean()
    assert float(same) > 0.9 and float(img.min()) >= 0 and float(img.max()) <= 1
    assert bool((img[:, :3].reshape(n, -1).std(1) > 1e-3).all())
    return img


def random_frozen_encoder(seed: int = 0, in_c: int = 4, device="cpu"):
    """The encoder of TinyAutoencoder(64, 64, in_c) with random weights (torch's global generator,
    seeded here and restored) and random BatchNorm tensors, frozen.  test_gpu_ppo.py's
    _random_frozen_encoder for a chosen channel count."""
    from ballbot_rl.encoders import TinyAutoencoder

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        enc = TinyAutoencoder(64, 64, in_c=in_c).encoder
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in enc:
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                nf = mod.num_features
                mod.weight.copy_(1 + 0.2 * torch.randn(nf, generator=g))
                mod.bias.copy_(0.1 * torch.randn(nf, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(nf, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(nf, generator=g))
    for p in enc.parameters():
        p.requires_grad = False
    return enc.to(device)


def encoder_tensors(enc):
    """The 21 tensors of bb_encoder_params, in its field order."""
    c1, b1, _, c2, b2, _, _, fc, b3, _ = list(enc)
    return [c1.weight, c1.bias, b1.weight, b1.bias, b1.running_mean, b1.running_var, b1.num_batches_tracked,
            c2.weight, c2.bias, b2.weight, b2.bias, b2.running_mean, b2.running_var, b2.num_batches_tracked,
            fc.weight, fc.bias, b3.weight, b3.bias, b3.running_mean, b3.running_var, b3.num_batches_tracked]
