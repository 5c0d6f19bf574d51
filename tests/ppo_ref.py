"""float64 references for the fused PPO kernels (tests/test_gpu_ppo_kernels.py).

Everything here runs on the CPU and needs no GPU: the policy with its flat
parameter buffer (bb_ppo_mlp_args' layout, with padding between the tensors),
the SB3 minibatch loss in whatever dtype its tensors have, the fp64 AdamW step
of csrc/bb_ppo.hip's comment, and the input conditioning that keeps every
branch a fp32 kernel and a fp64 reference could take differently away from its
edge, so that the comparison needs no "allowed outliers".
"""
from __future__ import annotations

import copy
import math
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LOG_2PI = math.log(2.0 * math.pi)
SLOT_NAMES = ([f"pi.W{l}" for l in range(4)] + [f"pi.b{l}" for l in range(4)] + [f"vf.W{l}" for l in range(4)]
              + [f"vf.b{l}" for l in range(4)] + ["action.W", "action.b", "value.W", "value.b", "log_std"])
Z_MARGIN = 1e-4      # |pre-activation| a LeakyReLU unit must keep (fp32 forward error <= 2e-6: 50-fold)
CLIP_MARGIN = 1e-3   # relative to the clip range: distance rho keeps from 1 - clip and 1 + clip


def policy_tensors(pol):
    """The 21 tensors in the order include/ballbot_mi355x.h documents for bb_ppo_mlp_args.offsets."""
    pi = [m for m in pol.policy_net if isinstance(m, torch.nn.Linear)]
    vf = [m for m in pol.value_net_trunk if isinstance(m, torch.nn.Linear)]
    return ([m.weight for m in pi] + [m.bias for m in pi] + [m.weight for m in vf] + [m.bias for m in vf]
            + [pol.action_net.weight, pol.action_net.bias, pol.value_net.weight, pol.value_net.bias, pol.log_std])


@lru_cache(maxsize=None)
def ref_policy(fd: int, seed: int):
    """ActorCriticPolicy over fd features (15 proprio, 56 camera) with perturbed parameters.

    -> namespace: module (fp32), module64 (its .double() copy), T32 / T64 (the 21 tensors),
    flat (fp32 [n_params], padding zero), offsets, sizes, pad (bool mask of the padding floats)."""
    from ballbot_rl.policies.mlp_policy import ActorCriticPolicy, obs_spaces

    assert fd in (15, 56)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        pol = ActorCriticPolicy(obs_spaces(cameras=fd == 56))
        with torch.no_grad():
            for t in policy_tensors(pol)[:-1]:
                t.add_(0.05 * torch.randn_like(t))
            pol.log_std.copy_(0.3 * torch.randn(3))
    assert pol.features_extractor.features_dim == fd
    pol64 = copy.deepcopy(pol).double()
    T32 = [t.detach() for t in policy_tensors(pol)]
    T64 = [t.detach() for t in policy_tensors(pol64)]
    offsets, sizes, off = [], [], 4  # padding in front, and 4..7 floats after every tensor
    for t in T32:
        offsets.append(off)
        sizes.append(t.numel())
        off = (off + t.numel() + 3) // 4 * 4 + 4
    n_params = off
    flat = torch.zeros(n_params)
    pad = torch.ones(n_params, dtype=torch.bool)
    for t, o, s in zip(T32, offsets, sizes):
        flat[o:o + s] = t.reshape(-1)
        pad[o:o + s] = False
    assert all(o % 4 == 0 for o in offsets) and int(pad.sum()) >= 4 * 22
    return SimpleNamespace(module=pol, module64=pol64, T32=T32, T64=T64, flat=flat, offsets=offsets, sizes=sizes,
                           pad=pad, n_params=n_params, fd=fd)


def flatten_like(ref, tensors, dtype):
    """21 tensors -> the flat layout of ref (padding zero)."""
    out = torch.zeros(ref.n_params, dtype=dtype, device=tensors[0].device)
    for t, o, s in zip(tensors, ref.offsets, ref.sizes):
        out[o:o + s] = t.reshape(-1).to(dtype)
    return out


def heads(T, x):
    """mean [n][3], value [n] and the 8 trunk pre-activations of the policy whose 21 tensors are T."""
    pre = []
    out = []
    for w0, b0 in ((0, 4), (8, 12)):
        h = x
        for l in range(4):
            z = F.linear(h, T[w0 + l], T[b0 + l])
            pre.append(z)
            h = F.leaky_relu(z, 0.01)
        out.append(h)
    mean = F.linear(out[0], T[16], T[17])
    value = F.linear(out[1], T[18], T[19]).squeeze(-1)
    return mean, value, pre


def log_prob(mean, actions, ls):
    z = (actions - mean) * torch.exp(-ls)
    return (-0.5 * z * z - ls - 0.5 * LOG_2PI).sum(-1)


def surrogate(logp, value, ls, old_logp, adv, ret, clip, ent_coef, vf_coef, normalize, adv_stats=None):
    """SB3 2.6.0 PPO.train's minibatch loss from the log-probabilities and values (the body of
    _sb3_minibatch_loss in tests/test_gpu_ppo.py): loss, pg, vf, entropy loss, approx_kl, clip_fraction."""
    if normalize and adv.shape[0] > 1:
        if adv_stats is not None:  # the data-parallel update: the global minibatch's mean, 1 / (std + 1e-8)
            adv = (adv - adv_stats[0]) * adv_stats[1]
        else:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    lr = logp - old_logp
    r = torch.exp(lr)
    pg = -torch.min(adv * r, adv * torch.clamp(r, 1 - clip, 1 + clip)).mean()
    vf = F.mse_loss(ret, value)
    ent = -(0.5 + 0.5 * LOG_2PI + ls).sum()
    with torch.no_grad():
        kl = torch.mean((r - 1) - lr)
        cf = torch.mean((torch.abs(r - 1) > clip).to(r.dtype))
    return pg + ent_coef * ent + vf_coef * vf, pg, vf, ent, kl, cf


def sb3_loss(T, obs, act, old_logp, adv, ret, clip, ent_coef, vf_coef, normalize, adv_stats=None):
    """The six log terms (a [6] tensor, detached) and the gradients of the loss w.r.t. the 21 tensors T,
    in the dtype and on the device of T."""
    T = [t.detach().clone().requires_grad_() for t in T]
    mean, value, _ = heads(T, obs)
    terms = surrogate(log_prob(mean, act, T[20]), value, T[20], old_logp, adv, ret, clip, ent_coef, vf_coef,
                      normalize, adv_stats)
    grads = torch.autograd.grad(terms[0], T)
    return torch.stack([t.detach() for t in terms]), list(grads)


def sb3_loss64(policy64, obs, act, old_logp, adv, ret, clip, ent_coef, vf_coef, normalize, adv_stats=None):
    """sb3_loss in float64 on the CPU: the fp32 inputs, widened exactly, through policy64's tensors."""
    d = lambda t: None if t is None else t.detach().cpu().double()  # noqa: E731
    return sb3_loss([t.detach() for t in policy_tensors(policy64)], d(obs), d(act), d(old_logp), d(adv), d(ret), clip,
                    ent_coef, vf_coef, normalize, d(adv_stats))


def rho_ambiguous(rho, clip):
    """Rows whose ratio sits within CLIP_MARGIN * clip of an edge of the clip range."""
    m = CLIP_MARGIN * clip
    return ((rho - (1 - clip)).abs() < m) | ((rho - (1 + clip)).abs() < m) | (((rho - 1).abs() - clip).abs() < m)


def conditioned_minibatch(ref, B: int, seed: int, clip: float, max_rounds: int = 40):
    """B minibatch rows (obs [B][fd], actions, old log-probs, advantages, returns; fp32) on which the
    fp64 reference shows no branch a fp32 kernel could take the other way: every one of the 2 x 4 x 128
    trunk pre-activations has |z| >= Z_MARGIN and the ratio rho keeps CLIP_MARGIN * clip from both clip
    edges.  A third of the rows has old_logp = the fp64 log-prob (rho ~ 1), a third is pushed well outside
    the clip range on both sides, the rest spreads over it; advantages take both signs everywhere.
    Ambiguous rows are redrawn whole (the weights are shared) until none is left; asserts the set is empty.
    -> namespace with the rows, `rounds` and `first_round` (ambiguous rows before any redraw)."""
    g = torch.Generator().manual_seed(seed)
    fd = ref.fd
    T = ref.T64
    std = torch.exp(T[20])
    kind = torch.arange(B) % 3
    obs = torch.empty(B, fd)
    act = torch.empty(B, 3)
    old = torch.empty(B)

    def draw(rows):
        k = rows.numel()
        obs[rows] = torch.randn(k, fd, generator=g)
        with torch.no_grad():
            mean, _, _ = heads(T, obs[rows].double())
            act[rows] = (mean + std * torch.randn(k, 3, generator=g).double()).float()
            lp = log_prob(mean, act[rows].double(), T[20])
        side = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
        far = side * (0.3 + 0.7 * torch.rand(k, generator=g))    # rho in [0.37, 0.74] or [1.35, 2.7]
        near = 1.5 * clip * torch.randn(k, generator=g)          # over and around the clip range
        kd = kind[rows]
        delta = torch.where(kd == 0, torch.zeros(k), torch.where(kd == 1, far, near))
        old[rows] = (lp + delta.double()).float()

    def ambiguous():
        with torch.no_grad():
            mean, _, pre = heads(T, obs.double())
            zmin = torch.stack([z.abs().min(1).values for z in pre]).min(0).values
            rho = torch.exp(log_prob(mean, act.double(), T[20]) - old.double())
        return (zmin < Z_MARGIN) | rho_ambiguous(rho, clip)

    draw(torch.arange(B))
    bad = ambiguous()
    first, rounds = int(bad.sum()), 0
    while bad.any() and rounds < max_rounds:
        draw(bad.nonzero().view(-1))
        bad = ambiguous()
        rounds += 1
    assert not bad.any(), f"{int(bad.sum())} ambiguous rows left after {rounds} redraws"
    adv = torch.randn(B, generator=g) * 1.5 + 0.3
    ret = torch.randn(B, generator=g)
    return SimpleNamespace(obs=obs, act=act, old=old, adv=adv, ret=ret, rounds=rounds, first_round=first, B=B)


def adamw64(p, g, m, v, step, lr, beta1, beta2, eps, wd, max_norm):
    """clip_grad_norm_ + AdamW in float64 (csrc/bb_ppo.hip's comment above adamw_prep_kernel);
    step is the counter BEFORE the call.  -> (p, m, v, step + 1, clip factor)."""
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    cf = min(1.0, max_norm / (float(g.norm()) + 1e-6))
    g = g * cf
    t = step + 1
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - lr / (1.0 - beta1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v, t, cf


def torch_adamw32(p, g, m, v, step, lr, beta1, beta2, eps, wd, max_norm):
    """torch's own fp32 clip_grad_norm_ + torch.optim.AdamW from the same seeded state, on the device
    of p (the yardstick test_flat_adamw_matches_torch trusts).  -> (p, m, v)."""
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    opt = torch.optim.AdamW([q], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step)), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
    torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def depth_like_images(n: int, seed: int) -> torch.Tensor:
    """[n][64][64] depth-camera-like images: a tilted plane plus small noise clipped to (0, 1], so that
    at least half of the pixels sit exactly at the 1.0 clip and no image is constant."""
    g = torch.Generator().manual_seed(seed)
    ang = 2 * math.pi * torch.rand(n, 1, 1, generator=g)
    lin = torch.linspace(-1, 1, 64)
    plane = 1.1 + 0.6 * (torch.cos(ang) * lin.view(1, 1, 64) + torch.sin(ang) * lin.view(1, 64, 1))
    img = (plane + 0.02 * torch.randn(n, 64, 64, generator=g)).clamp(0.05, 1.0)
    assert float((img == 1.0).float().mean()) >= 0.5 and float(img.min()) > 0
    assert bool((img.reshape(n, -1).std(1) > 1e-3).all())
    return img


def max_err(x, ref64) -> float:
    return float((x.detach().cpu().double() - ref64.detach().cpu().double()).abs().max())

