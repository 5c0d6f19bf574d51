"""GPU: the fused PPO kernels (bb_ppo_mlp_step, bb_ppo_mlp_act, bb_ppo_loss, bb_adamw_clip,
bb_depth_encoder) through the C ABI against float64 references on the CPU, at their edge shapes.

The tests own every buffer; the references and the input conditioning are in tests/ppo_ref.py.

Tolerance rule, for every compared tensor: e_kernel = max|kernel - ref64| and e_torch =
max|torch fp32 on the GPU - ref64| on the same inputs, and e_kernel <= 8 * e_torch + 1e-8.  Both are
fp32 with their own summation orders, so a factor of a few is honest; a mishandled row, slab or
tail moves a result by 1e-3 of its scale or more.  The project's earlier bounds stay as ceilings
(2e-4 * max|g| for gradients, rtol 1e-4 / atol 2e-4 for encoder features).  Every figure is printed
("RATIO ...") before a test asserts.

Measured on an MI355X, one run: the worst e_kernel / e_torch per kernel and shape, over the tensors
whose e_kernel is above the 1e-8 floor and over the normalize / image-family / step variants of the
shape (tensor, e_kernel / e_torch in brackets).  Nothing needed more than the factor 8; the largest
share of the bound 8 * e_torch + 1e-8 any tensor used was 0.81 (bb_ppo_loss B = 2: the loss term,
4.08, one ulp off where torch was 0.15 ulp off).

    kernel            shape              worst ratio
    bb_ppo_mlp_step   B=256,   obs 15    6.27  (log_std grad, 1.3e-07 / 2.0e-08)
    phase 1           B=768,   obs 15    4.22  (log row,      2.9e-07 / 6.9e-08)
                      B=768,   obs 56    4.46  (log_std grad, 6.3e-08 / 1.4e-08)
                      B=1280,  obs 56    4.43  (value.b grad, 1.5e-07 / 3.5e-08)
                      B=4096,  obs 15    5.39  (log row,      2.9e-07 / 5.4e-08)
                      B=16384, obs 15    5.39  (log row,      2.9e-07 / 5.4e-08)
    phases 0, 1+2     B=768,   obs 15    1.00  (params,       4.6e-08 / 4.6e-08)
    bb_ppo_mlp_act    n=1      15 / 56   1.00 / 1.41  (log_prob / mean)
                      n=31     15 / 56   1.14 / 0.78  (mean)
                      n=32     15 / 56   1.08 / 1.00  (value / mean)
                      n=33     15 / 56   1.14 / 0.80  (value / mean)
                      n=1000   15 / 56   1.07 / 1.39  (mean / log_prob)
    bb_ppo_loss       B=1                2.04  (terms, 3.2e-07 / 1.6e-07)
                      B=2                6.61  (terms, 4.6e-07 / 7.0e-08)
                      B=63               1.41  (d log_std, 1.4e-06 / 1.0e-06)
                      B=1025             1.00  (terms, 6.9e-08 / 6.9e-08)
                      B=8193             2.23  (terms, 3.4e-07 / 1.5e-07)
    bb_adamw_clip     n=1 ... 4099       1.00  (param; the kernel takes torch's AdamW roundings)
    bb_depth_encoder  eval,  n=1         0.90  (features, 1.0e-07 / 1.1e-07)
                      eval,  n=31        1.20  (features, 2.3e-07 / 2.0e-07)
                      eval,  n=33        1.30  (features, 1.9e-07 / 1.5e-07)
                      eval,  n=257       1.30  (features, 2.5e-07 / 1.9e-07)
                      train, n=2         1.94  (bn1 running_var, 1.3e-07 / 6.9e-08)
                      train, n=33        1.41  (bn2 running_var, 1.2e-07 / 8.2e-08)
                      train, n=257       1.53  (features, 6.2e-06 / 4.1e-06)

The ten weight-gradient tensors sit at ratios of 0.02 to 2.0 in every case (e_kernel at most 1.0e-06
of the tensor's largest entry); the ratios above 4 are all tensors of six or fewer elements (log_std,
value.b, the log row), where one lucky rounding on torch's side makes the ratio.  In train mode on the depth-like images torch's own fp32 BatchNorm path is the
less accurate side: its features are 3.8e-04 (n = 257) and 8.5e-04 (the gathered camera slice) from
fp64 where the kernel, whose batch statistics accumulate in fp64, is 6.6e-06 and 1.1e-05.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ppo_ref as R  # noqa: E402

DEV = "cuda:0"
CLIP, ENT_COEF, VF_COEF = 0.1, 0.01, 0.5
BETA1, BETA2, EPS, WD, MAX_NORM = 0.9, 0.999, 1e-8, 0.01, 0.5
LR = float(np.float32(1e-3))  # the kernels read a float32 learning rate from the device
SENT = 12345.0                # fills what a kernel must leave alone
FACTOR, FLOOR = 8.0, 1e-8


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Tally:
    """Collects (tensor, e_kernel, e_torch) of one test, prints each, asserts them together."""

    def __init__(self, kernel, case):
        self.kernel, self.case, self.bad = kernel, case, []

    def add(self, name, got, yard, ref64, ceiling=None):
        assert bool(torch.isfinite(got).all()), (self.kernel, self.case, name, "not finite")
        ek, et = R.max_err(got, ref64), R.max_err(yard, ref64)
        print(f"RATIO {self.kernel} {self.case} {name} e_kernel={ek:.3e} e_torch={et:.3e} "
              f"ratio={ek / max(et, 1e-300):.2f} scale={float(ref64.abs().max()):.3e}")
        if ek > FACTOR * et + FLOOR:
            self.bad.append((name, "e_kernel", ek, "> 8 * e_torch + 1e-8, e_torch", et))
        if ceiling is not None and ek > ceiling:
            self.bad.append((name, "e_kernel", ek, "> ceiling", ceiling))

    def finish(self):
        assert not self.bad, (self.kernel, self.case, self.bad)


# ------------------------------------------------------------------ bb_ppo_mlp_step
STEP_CASES = [(256, 15), (768, 15), (768, 56), (1280, 56), (4096, 15), (16384, 15)]
_cache = {}


def _minibatch(B, fd):
    """The conditioned minibatch of a case and its fp64 references, computed once and left unchanged."""
    key = (B, fd)
    if key not in _cache:
        ref = R.ref_policy(fd, 11)
        mb = R.conditioned_minibatch(ref, B, 100 + B + fd, CLIP)
        print(f"conditioning B={B} fd={fd}: {mb.first_round} ambiguous rows at first, {mb.rounds} redraws, 0 left")
        _cache[key] = (ref, mb, {})
    return _cache[key]


def _reference(B, fd, normalize, stats):
    ref, mb, done = _minibatch(B, fd)
    key = (normalize, stats is not None)
    if key not in done:
        done[key] = R.sb3_loss64(ref.module64, mb.obs, mb.act, mb.old, mb.adv, mb.ret, CLIP, ENT_COEF, VF_COEF,
                                 normalize, stats)
    return done[key]


class _StepRun:
    """Device buffers of one bb_ppo_mlp_step call: a rollout of 3 B rows whose minibatch `k` (a random
    permutation's rows) holds the conditioned rows; every other row holds large junk."""

    def __init__(self, ref, mb, k, normalize, stats=None, seeded_state=False):
        from ballbot_gym import _native as N

        self.N, self.L, self.ref = N, N.lib(), ref
        B, fd = mb.B, ref.fd
        n = 3 * B
        g = torch.Generator().manual_seed(7 * B + fd)
        perm = torch.randperm(n, generator=g).view(3, B)
        rows = perm[k]
        assert int(rows.max()) >= B  # the indices point outside the first B rows

        def scatter(x):
            full = 1e3 * torch.randn(n, *x.shape[1:], generator=g)
            full[rows] = x
            return full.to(DEV)

        self.obs = mb.obs.to(DEV) if fd == 56 else scatter(mb.obs)  # 56-d: the minibatch's features in order
        self.act, self.old, self.adv, self.ret = (scatter(x) for x in (mb.act, mb.old, mb.adv, mb.ret))
        self.perm = perm.to(DEV)
        self.k = torch.tensor([k], dtype=torch.int64, device=DEV)
        self.row = torch.tensor([1], dtype=torch.int64, device=DEV)
        self.log = torch.full((4, 6), SENT, device=DEV)
        self.params = ref.flat.to(DEV)
        self.grad = torch.where(ref.pad, 0.0, float("nan")).float().to(DEV)  # tensors: to be overwritten
        if seeded_state:
            self.m0 = 0.01 * torch.randn(ref.n_params, generator=g)
            self.v0 = 1e-4 * torch.rand(ref.n_params, generator=g) + 1e-6
            self.step0 = 5
        else:
            self.m0, self.v0, self.step0 = torch.zeros(ref.n_params), torch.zeros(ref.n_params), 0
        self.m, self.v = self.m0.to(DEV), self.v0.to(DEV)
        self.step = torch.tensor(float(self.step0), device=DEV)
        self.clip = torch.tensor(CLIP, device=DEV)
        self.lr = torch.tensor(LR, device=DEV)
        self.coef = torch.zeros(4, device=DEV)
        self.stats = None if stats is None else stats.to(DEV)
        nbytes = C.c_int64()
        N.check(self.L.bb_ppo_mlp_workspace_bytes(B, C.byref(nbytes)), "bb_ppo_mlp_workspace_bytes")
        self.ws = torch.empty(nbytes.value // 4, device=DEV)
        a = N.PPOMlpArgs()
        a.params, a.grad, a.exp_avg, a.exp_avg_sq = (t.data_ptr() for t in (self.params, self.grad, self.m, self.v))
        a.n_params = ref.n_params
        for i, o in enumerate(ref.offsets):
            a.offsets[i] = o
        a.obs, a.actions, a.old_logp = self.obs.data_ptr(), self.act.data_ptr(), self.old.data_ptr()
        a.advantages, a.returns, a.perm = self.adv.data_ptr(), self.ret.data_ptr(), self.perm.data_ptr()
        a.mb_counter, a.row_counter, a.log = self.k.data_ptr(), self.row.data_ptr(), self.log.data_ptr()
        a.clip, a.lr, a.step, a.coef = (t.data_ptr() for t in (self.clip, self.lr, self.step, self.coef))
        a.B, a.normalize_advantage, a.obs_dim, a.obs_direct = B, int(normalize), fd, int(fd == 56)
        a.ent_coef, a.vf_coef = ENT_COEF, VF_COEF
        a.beta1, a.beta2, a.eps, a.weight_decay, a.max_grad_norm = BETA1, BETA2, EPS, WD, MAX_NORM
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), nbytes.value
        a.adv_stats = None if stats is None else self.stats.data_ptr()
        self.args, self.k0 = a, k

    def run(self, phase):
        self.args.phase = phase
        self.N.check(self.L.bb_ppo_mlp_step(C.byref(self.args), _stream()), "bb_ppo_mlp_step")
        torch.cuda.synchronize()

    def grads(self):
        return [self.grad[o:o + s].view_as(t) for o, s, t in zip(self.ref.offsets, self.ref.sizes, self.ref.T32)]


def _torch32(ref, mb, normalize, stats):
    """torch's own fp32 autograd of the same loss on the GPU, from the same fp32 inputs (the yardstick)."""
    return R.sb3_loss([t.to(DEV) for t in ref.T32], mb.obs.to(DEV), mb.act.to(DEV), mb.old.to(DEV), mb.adv.to(DEV),
                      mb.ret.to(DEV), CLIP, ENT_COEF, VF_COEF, normalize, None if stats is None else stats.to(DEV))


def _outer_stats(B):
    """Advantage statistics of a different, larger set (the data-parallel global minibatch), as the
    float32 pair the kernel reads; the reference uses the same two numbers."""
    big = (1.5 * torch.randn(4 * B, generator=torch.Generator().manual_seed(B)) + 0.3).double()
    return torch.stack([big.mean(), 1.0 / (big.std() + 1e-8)]).float()


@pytest.mark.parametrize("B,fd,normalize,ext_stats",
                         [(B, fd, nz, False) for B, fd in STEP_CASES for nz in (0, 1)] + [(768, 15, 1, True)])
def test_mlp_step_gradient_matches_fp64(B, fd, normalize, ext_stats):
    """bb_ppo_mlp_step phase 1: the flat gradient (all 21 tensors) and the log row vs the fp64 SB3 loss,
    on inputs conditioned so that no LeakyReLU unit and no clip edge is ambiguous.  B / n_chunks(B) / 32
    slabs per weight-gradient chunk: 256 -> 1, 768 -> 3, 1280 -> 5, 4096 -> 2, 16384 -> 8."""
    stats = _outer_stats(B) if ext_stats else None
    ref, mb, _ = _minibatch(B, fd)
    terms64, grads64 = _reference(B, fd, normalize, stats)
    terms32, grads32 = _torch32(ref, mb, normalize, stats)
    k = 1 + (B // 256) % 2
    run = _StepRun(ref, mb, k, normalize, stats)
    run.run(1)
    tally = _Tally("mlp_step", f"B={B},fd={fd},norm={normalize},stats={int(ext_stats)}")
    tally.add("log_row", run.log[1], terms32, terms64)
    for name, got, yard, want in zip(R.SLOT_NAMES, run.grads(), grads32, grads64):
        tally.add(name, got, yard, want, ceiling=2e-4 * float(want.abs().max()) + 1e-8)
    assert int(run.k) == k + 1 and int(run.row) == 2                      # both counters advanced by one
    assert bool((run.log[[0, 2, 3]] == SENT).all())                      # the other log rows untouched
    assert bool((run.grad.cpu()[ref.pad] == 0).all())                    # padding of grad never written
    assert torch.equal(run.params.cpu(), ref.flat)                       # phase 1 takes no optimiser step
    assert torch.equal(run.m.cpu(), run.m0) and float(run.step) == 0.0
    tally.finish()


def test_mlp_step_optimiser_phases_match_fp64():
    """Phase 0 (whole minibatch) and phase 1 + 2 (gradient, then clip + AdamW) from a seeded AdamW state
    (step 5, so the update is smooth in the gradient) vs fp64 clip_grad_norm_ + AdamW on the fp64 gradient;
    the yardstick is torch's fp32 gradient through torch's clip_grad_norm_ + AdamW.  The two routes differ
    only in the summation of the clip norm: a few ulp of the operands."""
    B, fd = 768, 15
    ref, mb, _ = _minibatch(B, fd)
    _, grads64 = _reference(B, fd, 1, None)
    _, grads32 = _torch32(ref, mb, 1, None)
    g64 = R.flatten_like(ref, grads64, torch.float64)
    outs = {}
    for route, phases in (("phase0", (0,)), ("phase1+2", (1, 2))):
        run = _StepRun(ref, mb, 1, 1, seeded_state=True)
        for ph in phases:
            run.run(ph)
        assert float(run.step) == 6.0 and int(run.k) == 2 and int(run.row) == 2
        outs[route] = (run.params.cpu(), run.m.cpu(), run.v.cpu(), run.grad.cpu())
    p64, m64, v64, _, cf = R.adamw64(ref.flat, g64, run.m0, run.v0, 5, LR, BETA1, BETA2, EPS, WD, MAX_NORM)
    assert cf < 0.9  # the clip bites
    yard = R.torch_adamw32(ref.flat.to(DEV), R.flatten_like(ref, grads32, torch.float32), run.m0.to(DEV),
                           run.v0.to(DEV), 5, LR, BETA1, BETA2, EPS, WD, MAX_NORM)
    tally = _Tally("mlp_step_opt", f"B={B},fd={fd}")
    for route, (p, m, v, _) in outs.items():
        tally.add(f"{route}.params", p, yard[0], p64)
        tally.add(f"{route}.exp_avg", m, yard[1], m64)
        tally.add(f"{route}.exp_avg_sq", v, yard[2], v64)
    (pa, ma, va, ga), (pb, mb_, vb, gb) = outs["phase0"], outs["phase1+2"]
    assert torch.equal(ga, gb)  # the same gradient: the routes part at the clip norm
    e = 2.0 ** -23
    g = ga.double().abs()
    assert bool(((ma.double() - mb_.double()).abs() <= 4 * e * (run.m0.double().abs() + g)).all())
    assert bool(((va.double() - vb.double()).abs() <= 4 * e * va.double().abs()).all())
    moved = (pa.double() - ref.flat.double()).abs()
    assert bool(((pa.double() - pb.double()).abs() <= 4 * e * (pa.double().abs() + moved)).all())
    tally.finish()


# ------------------------------------------------------------------ bb_ppo_mlp_act
@pytest.mark.parametrize("fd", [15, 56])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_mlp_act_matches_fp64(n, fd):
    """bb_ppo_mlp_act with noise: mean (the deterministic call), value and log-prob vs fp64; the sampled
    action follows from the kernel's own mean; nothing is written past row n (partial tiles)."""
    from ballbot_gym import _native as N

    ref = R.ref_policy(fd, 11)
    g = torch.Generator().manual_seed(1000 * n + fd)
    rows = n + 32
    obs = torch.full((rows, fd), float("nan"))
    noise = torch.full((rows, 3), float("nan"))
    obs[:n] = torch.randn(n, fd, generator=g)
    noise[:n] = torch.randn(n, 3, generator=g)
    obs_d, noise_d, params = obs.to(DEV), noise.to(DEV), ref.flat.to(DEV)
    offs = (C.c_int32 * 21)(*ref.offsets)

    def call(noise_t):
        out = {k: torch.full(s, SENT, device=DEV) for k, s in (("obs_copy", (rows, fd)), ("act", (rows, 3)),
                                                               ("clipped", (rows, 3)), ("val", (rows,)),
                                                               ("lp", (rows,)))}
        N.check(N.lib().bb_ppo_mlp_act(_ptr(params), offs, ref.n_params, _ptr(obs_d), fd, _ptr(noise_t), n,
                                       _ptr(out["obs_copy"]) if fd == 15 else None, _ptr(out["act"]),
                                       _ptr(out["clipped"]), _ptr(out["val"]), _ptr(out["lp"]), _stream()),
                "bb_ppo_mlp_act")
        torch.cuda.synchronize()
        for k, t in out.items():  # rows >= n keep the sentinel
            assert bool((t[n:] == SENT).all()), k
        return out

    det, smp = call(None), call(noise_d)
    mean32 = det["act"][:n]
    x64, nz64, ls64 = obs[:n].double(), noise[:n].double(), ref.T64[20]
    with torch.no_grad():
        mean64, val64, _ = R.heads(ref.T64, x64)
        lp64 = R.log_prob(mean64, mean64 + nz64 * torch.exp(ls64), ls64)
        T = [t.to(DEV) for t in ref.T32]
        mean_t, val_t, _ = R.heads(T, obs_d[:n])
        act_t = mean_t + noise_d[:n] * torch.exp(T[20])
        lp_t = R.log_prob(mean_t, act_t, T[20])
    tally = _Tally("mlp_act", f"n={n},fd={fd}")
    tally.add("mean", mean32, mean_t, mean64)
    tally.add("value", smp["val"][:n], val_t, val64)
    tally.add("log_prob", smp["lp"][:n], lp_t, lp64)
    assert torch.equal(det["val"][:n], smp["val"][:n])
    # actions = fl(mean32 + fl(noise * fl(exp(log_std)))): three roundings of at most one ulp32 of their results
    step = nz64 * torch.exp(ls64)
    want = mean32.cpu().double() + step
    tol = 2.0 ** -23 * (want.abs() + 2 * step.abs())
    assert bool(((smp["act"][:n].cpu().double() - want).abs() <= tol).all())
    assert torch.equal(smp["clipped"][:n], smp["act"][:n].clamp(-1, 1))
    assert torch.equal(det["clipped"][:n], mean32.clamp(-1, 1))
    if fd == 15:
        assert torch.equal(smp["obs_copy"][:n], obs_d[:n])
    tally.finish()


# ------------------------------------------------------------------ bb_ppo_loss
def _loss_inputs(B):
    g = torch.Generator().manual_seed(31 * B + 5)
    mean, values, act = torch.randn(B, 3, generator=g), torch.randn(B, generator=g), torch.randn(B, 3, generator=g)
    ls = 0.3 * torch.randn(3, generator=g)
    adv, ret = 1.5 * torch.randn(B, generator=g) + 0.3, torch.randn(B, generator=g)
    lp = R.log_prob(mean.double(), act.double(), ls.double())
    kind = torch.arange(B) % 3  # ties (rho ~ 1), far outside the clip range on both sides, over the range
    old = torch.empty(B)

    def draw(rows):
        k = rows.numel()
        side = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
        far, near = side * (0.3 + 0.7 * torch.rand(k, generator=g)), 1.5 * CLIP * torch.randn(k, generator=g)
        kd = kind[rows]
        delta = torch.where(kd == 0, torch.zeros(k), torch.where(kd == 1, far, near))
        old[rows] = (lp[rows] + delta.double()).float()

    draw(torch.arange(B))
    for _ in range(40):  # no ratio within 1e-3 * clip of a clip edge (proved on the reference alone)
        bad = R.rho_ambiguous(torch.exp(lp - old.double()), CLIP)
        if not bad.any():
            break
        draw(bad.nonzero().view(-1))
    assert not R.rho_ambiguous(torch.exp(lp - old.double()), CLIP).any()
    return mean, values, ls, act, old, adv, ret


def _loss_ref(inp, normalize, dtype, device):
    mean, values, ls, act, old, adv, ret = (t.to(device=device, dtype=dtype) for t in inp)
    mean, values, ls = (t.requires_grad_() for t in (mean, values, ls))
    terms = R.surrogate(R.log_prob(mean, act, ls), values, ls, old, adv, ret, CLIP, ENT_COEF, VF_COEF, normalize)
    gm, gv, gl = torch.autograd.grad(terms[0], (mean, values, ls))
    return torch.stack([t.detach() for t in terms]), gl, gm, gv


def _loss_kernel(inp, normalize):
    from ballbot_gym import _native as N

    B = inp[0].shape[0]
    dev = [t.to(DEV) for t in inp] + [torch.tensor(CLIP, device=DEV)]
    terms, gm, gv = torch.full((9 + 4,), SENT, device=DEV), torch.full((B + 4, 3), SENT, device=DEV), \
        torch.full((B + 4,), SENT, device=DEV)
    N.check(N.lib().bb_ppo_loss(*[_ptr(t) for t in dev], B, int(normalize), ENT_COEF, VF_COEF, _ptr(terms), _ptr(gm),
                                _ptr(gv), _stream()), "bb_ppo_loss")
    torch.cuda.synchronize()
    assert bool((terms[9:] == SENT).all()) and bool((gm[B:] == SENT).all()) and bool((gv[B:] == SENT).all())
    return terms[:6], terms[6:9], gm[:B], gv[:B]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 63, 1025, 8193])
def test_ppo_loss_matches_fp64(B, normalize):
    """bb_ppo_loss at edge sizes: the six loss terms, d loss / d log_std, grad_mean and grad_values vs the
    fp64 SB3 loss; one sample with normalize_advantage is the un-normalised loss (SB3's len > 1 guard)."""
    inp = _loss_inputs(B)
    got = _loss_kernel(inp, normalize)
    want = _loss_ref(inp, normalize, torch.float64, "cpu")
    yard = _loss_ref(inp, normalize, torch.float32, DEV)
    tally = _Tally("ppo_loss", f"B={B},norm={normalize}")
    for name, a, b, c in zip(("terms", "dlog_std", "grad_mean", "grad_values"), got, yard, want):
        tally.add(name, a, b, c)
    if B == 1 and normalize:
        for a, b in zip(got, _loss_kernel(inp, 0)):
            assert torch.equal(a, b)
    tally.finish()


# ------------------------------------------------------------------ bb_adamw_clip
@pytest.mark.parametrize("grad_case", ["zero", "small", "large"])
@pytest.mark.parametrize("n", [1, 3, 5, 1023, 1025, 4099])
def test_adamw_clip_matches_fp64(n, grad_case):
    """bb_adamw_clip on sizes that reach the float4 body and the scalar tail of the norm pass and the last
    partial block of the update, from a seeded state at step 0 and 999: gradient all zero (clip factor 1,
    nothing NaN), norm far below max_norm, norm far above it.  grad is not modified."""
    from ballbot_gym import _native as N

    g = torch.Generator().manual_seed(17 * n + len(grad_case))
    scale = {"zero": 0.0, "small": 1e-3, "large": 1e3}[grad_case]
    for step0 in (0, 999):
        p0, m0 = torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g)
        v0 = 1e-4 * torch.rand(n, generator=g) + 1e-6
        g0 = scale * torch.randn(n, generator=g) / max(n, 1) ** 0.5
        if grad_case == "large":
            assert float(g0.norm()) > 10 * MAX_NORM or n <= 5
            g0 = g0 * (1e3 / float(g0.norm()))
        # n + 4 rows: what follows the n elements must stay as it was
        bufs = [torch.cat([t, torch.full((4,), SENT)]).to(DEV) for t in (p0, g0, m0, v0)]
        step, lr, coef = torch.tensor(float(step0), device=DEV), torch.tensor(LR, device=DEV), torch.zeros(4, device=DEV)
        N.check(N.lib().bb_adamw_clip(*[_ptr(t) for t in bufs], n, _ptr(lr), _ptr(step), _ptr(coef), BETA1, BETA2, EPS,
                                      WD, MAX_NORM, _stream()), "bb_adamw_clip")
        torch.cuda.synchronize()
        p, gg, m, v = (t.cpu() for t in bufs)
        assert all(bool((t[n:] == SENT).all()) for t in (p, gg, m, v)) and torch.equal(gg[:n], g0)
        assert float(step) == step0 + 1
        p64, m64, v64, _, cf = R.adamw64(p0, g0, m0, v0, step0, LR, BETA1, BETA2, EPS, WD, MAX_NORM)
        assert (cf == 1.0) == (grad_case != "large")
        assert abs(float(coef[0]) - cf) <= 4 * 2.0 ** -23 * cf
        yard = R.torch_adamw32(p0.to(DEV), g0.to(DEV), m0.to(DEV), v0.to(DEV), step0, LR, BETA1, BETA2, EPS, WD,
                               MAX_NORM)
        tally = _Tally("adamw_clip", f"n={n},grad={grad_case},step={step0}")
        tally.add("param", p[:n], yard[0], p64)
        tally.add("exp_avg", m[:n], yard[1], m64)
        tally.add("exp_avg_sq", v[:n], yard[2], v64)
        tally.finish()


# ------------------------------------------------------------------ bb_depth_encoder
def _encoder(seed):
    from test_gpu_ppo import _random_frozen_encoder

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)  # the conv and linear weights come from torch's global generator
        return _random_frozen_encoder(seed)


def _encode(enc, images, stride, index, n, train):
    """bb_depth_encoder through the C ABI on buffers of the test's own; -> features [n][20]."""
    from ballbot_gym import _native as N

    c1, b1, _, c2, b2, _, _, fc, b3, _ = list(enc)
    vals = [c1.weight, c1.bias, b1.weight, b1.bias, b1.running_mean, b1.running_var, b1.num_batches_tracked,
            c2.weight, c2.bias, b2.weight, b2.bias, b2.running_mean, b2.running_var, b2.num_batches_tracked,
            fc.weight, fc.bias, b3.weight, b3.bias, b3.running_mean, b3.running_var, b3.num_batches_tracked]
    p = N.EncoderParams(*[t.data_ptr() for t in vals])
    nbytes = C.c_int64()
    N.check(N.lib().bb_depth_encoder_workspace_bytes(n, C.byref(nbytes)), "bb_depth_encoder_workspace_bytes")
    ws = torch.empty(nbytes.value // 4 + 4, device=DEV)
    out = torch.full((n + 4, 20), SENT, device=DEV)
    N.check(N.lib().bb_depth_encoder(C.byref(p), _ptr(images), stride, _ptr(index), n, 64, 64, int(train),
                                     float(b1.momentum), float(b1.eps), _ptr(out), 20, _ptr(ws), nbytes.value,
                                     _stream()), "bb_depth_encoder")
    torch.cuda.synchronize()
    assert bool((out[n:] == SENT).all())
    return out[:n]


def _images(family, n, seed):
    if family == "depth":
        return R.depth_like_images(n, seed)
    return torch.rand(n, 64, 64, generator=torch.Generator().manual_seed(seed))


def _check_encoder(case, train, mine, images, stride, index, gathered):
    """mine: the module whose tensors the kernel reads (and, in train mode, updates); gathered: the
    [n][1][64][64] batch (CPU) the call encodes, for the fp64 module and torch's fp32 one."""
    import copy

    n = gathered.shape[0]
    ref64 = copy.deepcopy(mine).double().cpu()
    yard = copy.deepcopy(mine)
    for m in (mine, ref64, yard):
        m.train(train)
    with torch.no_grad():
        want = ref64(gathered.double())
        ygot = yard(gathered.to(DEV))
    got = _encode(mine, images, stride, index, n, train)
    tally = _Tally("depth_encoder", case)
    tally.add("features", got, ygot, want)
    # the project's earlier bound stays as a ceiling: rtol 1e-4 / atol 2e-4
    assert bool(((got.cpu().double() - want).abs() <= 2e-4 + 1e-4 * want.abs()).all())
    bns = lambda e: [m for m in e if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]  # noqa: E731
    for i, (a, b, c) in enumerate(zip(bns(mine), bns(yard), bns(ref64)), 1):
        if train:
            tally.add(f"bn{i}.running_mean", a.running_mean, b.running_mean, c.running_mean)
            tally.add(f"bn{i}.running_var", a.running_var, b.running_var, c.running_var)
        else:  # eval mode moves nothing
            assert torch.equal(a.running_mean.cpu().double(), c.running_mean)
            assert torch.equal(a.running_var.cpu().double(), c.running_var)
        assert int(a.num_batches_tracked) == int(c.num_batches_tracked) == (1 if train else 0)
    tally.finish()


@pytest.mark.parametrize("family", ["noise", "depth"])
@pytest.mark.parametrize("train,n", [(False, 1), (False, 31), (False, 33), (False, 257),
                                     (True, 2), (True, 33), (True, 257)])
def test_depth_encoder_matches_fp64(train, n, family):
    """bb_depth_encoder below one 32-image group, across it, and across the n < 256 / n >= 256 grid
    switch with a remainder, on uniform noise and on depth-like images (half the pixels exactly 1.0)."""
    img = _images(family, n, 10 * n + train)
    _check_encoder(f"train={int(train)},n={n},{family}", train, _encoder(3), img.to(DEV), 4096, None,
                   img.unsqueeze(1))


def test_depth_encoder_gathers_repeated_rows_of_a_camera_slice():
    """Train mode reading camera 1 of a [300][2][64][64] buffer (image_stride 8192, offset 4096 floats)
    through index_dev, with repeated indices, == the fp64 module on the gathered images."""
    cams = torch.stack([_images("noise", 300, 1), _images("depth", 300, 2)], 1)
    idx = torch.randint(0, 300, (257,), generator=torch.Generator().manual_seed(3))
    assert idx.unique().numel() < idx.numel()
    cams_d = cams.to(DEV)
    _check_encoder("train=1,n=257,index+stride", True, _encoder(4), cams_d[:, 1], 2 * 4096, idx.to(DEV),
                   cams[idx][:, 1:2])
