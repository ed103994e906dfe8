"""Restatement, for the tests, of the stochastic steps under Qwen-Image's norm-rescaled true CFG (advgrpo_sde_step_rescaled,
advgrpo_flow_sde_step_rescaled and their backward): the combine and the rescale are qwen_sampler_reference's ``pack`` / ``combine`` /
``rescale`` (PARITY UNPINNED, as there: written from the published pipeline), the Flow-SDE step is flow_sde_reference's, the Flow-CPS
step is restated here (sd3_sde_with_logprob.py:117-134 of the reference).

    v    = unpack( comb * ||pos|| / ||comb|| ) ,  comb = neg + s (pos - neg)                  per 2 x 2 x 16 token
    cps:   std = sigma_prev sin(noise_level pi / 2) ;  mu = (x - sigma v)(1 - sigma_prev) + (x + v (1 - sigma)) sqrt(sigma_prev^2 - std^2)
           x' = mu + std eps ;  lp = -mean_i (x'_i - mu_i)^2
    sde:   flow_sde_reference.flow_sde_step

``rescaled_step`` is that in float64 with no rounding point (or, with ``dtype=None``, in the tensors' own dtypes: one torch op per
rounding).  ``grad_analytic`` is the closed form the backward kernels evaluate, in float64; ``grad_emulated_f32`` runs the kernel's own
operation order -- roundings, fixed summation order, float32 throughout -- with torch on the CPU: the tolerance rule of
tests/test_gpu_cfg_rescale.py measures it against float64 autograd."""
import math
import os

import numpy as np
import torch

import flow_sde_reference as F
import qwen_sampler_reference as Q

SCALE, SHAPES, make_inputs = Q.SCALE, Q.SHAPES, Q.make_inputs
NOISE_LEVEL, STEP = 0.7, 3                      # step 3 of the 10-step SD3 table (the golden's own copy of it)
SIGMAS = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), "golden", "flow_sde.npz"))["s10_i5/sigmas"]).float()
bf16 = torch.bfloat16


def _col(t, x):
    return t.view((-1,) + (1,) * (x.dim() - 1))


def rescaled_v(v_neg, v_pos, scale=SCALE, dtype=torch.float64):
    """[B, C, H, W] predictions -> the rescaled prediction; dtype=None keeps the tensors' dtype (torch's own rounding points)."""
    B, C, H, W = v_neg.shape
    if dtype is not None:
        v_neg, v_pos = v_neg.to(dtype), v_pos.to(dtype)
    neg, pos = Q.pack(v_neg), Q.pack(v_pos)
    return Q.unpack(Q.rescale(Q.combine(neg, pos, scale), pos), C, H, W)


def cps_step(v, x, sigma, sigma_prev, noise_level, eps=None, prev_sample=None, dtype=torch.float64):
    """Flow-CPS; sigma / sigma_prev [B] float32 schedule entries.  -> (prev_sample, log_prob [B], mean, std [B]) in ``dtype``; with
    float32 the reference's operation sequence, one torch op per rounding."""
    v, x = v.to(dtype), x.to(dtype)
    sigma, sigma_prev = _col(sigma.to(dtype), x), _col(sigma_prev.to(dtype), x)
    sin = torch.tensor(math.sin(noise_level * math.pi / 2), dtype=torch.float32).to(dtype)   # the kernel takes the f32 coefficient
    std = sigma_prev * sin
    x0 = x - sigma * v
    x1 = x + v * (1 - sigma)
    mean = x0 * (1 - sigma_prev) + x1 * torch.sqrt(sigma_prev ** 2 - std ** 2)
    prev_sample = mean + std * eps.to(dtype) if prev_sample is None else prev_sample.to(dtype)
    log_prob = (-((prev_sample.detach() - mean) ** 2)).mean(dim=tuple(range(1, x.dim())))
    return prev_sample, log_prob, mean, std.reshape(-1)


def step(sde_type, v, x, sigma, sigma_prev, noise_level=NOISE_LEVEL, eps=None, prev_sample=None, dtype=torch.float64, sigma_max=None):
    """-> (prev_sample, log_prob, mean, std_dev_t) of either step on an already combined prediction."""
    if sde_type == "cps":
        return cps_step(v, x, sigma, sigma_prev, noise_level, eps, prev_sample, dtype)
    smax = float(SIGMAS[1]) if sigma_max is None else sigma_max
    nxt, lp, mean, std, _ = F.flow_sde_step(v, x, sigma, sigma_prev, smax, noise_level, eps=eps, prev_sample=prev_sample, dtype=dtype)
    return nxt, lp, mean, std


def rescaled_step(sde_type, v_neg, v_pos, x, sigma, sigma_prev, noise_level=NOISE_LEVEL, eps=None, prev_sample=None, scale=SCALE,
                  dtype=torch.float64):
    """The combined step.  dtype=float64: no rounding point.  dtype=None: the rescale in the predictions' dtype, the step in float32."""
    v = rescaled_v(v_neg, v_pos, scale, dtype)
    return step(sde_type, v, x, sigma, sigma_prev, noise_level, eps, prev_sample, torch.float32 if dtype is None else dtype)


def schedule_rows(B, step_index=STEP):
    return SIGMAS[step_index].repeat(B), SIGMAS[step_index + 1].repeat(B)


# ---------------------------------------------------------------------------------------------------------------- backward
def _dmu_dv(sde_type, sigma, sigma_prev, noise_level, dtype):
    """(d mean / d v [B], w^2 [B] or None): d log_prob / d mean = 2 (prev - mean) / n for Flow-CPS, (prev - mean) / (n w^2) for Flow-SDE."""
    s, sp = sigma.to(dtype), sigma_prev.to(dtype)
    if sde_type == "cps":
        std = sp * torch.tensor(math.sin(noise_level * math.pi / 2), dtype=torch.float32).to(dtype)
        return (1 - s) * torch.sqrt(sp ** 2 - std ** 2) - s * (1 - sp), None
    dt = sp - s
    sd = torch.sqrt(s / (1 - torch.where(s == 1, SIGMAS[1].to(dtype), s))) * noise_level
    w = sd * torch.sqrt(-1 * dt)
    return (1 + sd ** 2 * (1 - s) / (2 * s)) * dt, w * w


def loss(sde_type, v_neg, v_pos, x, sigma, sigma_prev, prev_sample, grad_log_prob, mean_ref=None, kl_weight=0.0, noise_level=NOISE_LEVEL,
         scale=SCALE):
    """sum_b glp_b log_prob_b [+ kl_weight mean_b mean_elem (mean - mean_ref)^2] of the float64 restatement, and the per-sample KL."""
    _, lp, mean, _ = rescaled_step(sde_type, v_neg, v_pos, x, sigma, sigma_prev, noise_level, prev_sample=prev_sample, scale=scale)
    total, kl = (lp * grad_log_prob.double()).sum(), None
    if mean_ref is not None:
        kl = ((mean - mean_ref.double()) ** 2).mean(dim=(1, 2, 3))
        total = total + kl_weight * kl.mean()
    return total, kl


def grad_autograd(sde_type, v_neg, v_pos, *args, **kw):
    """(d loss / d v_neg, d loss / d v_pos, kl) by float64 autograd of the restatement."""
    n_, p_ = v_neg.double().requires_grad_(True), v_pos.double().requires_grad_(True)
    total, kl = loss(sde_type, n_, p_, *args, **kw)
    total.backward()
    return n_.grad, p_.grad, None if kl is None else kl.detach()


def grad_analytic(sde_type, v_neg, v_pos, x, sigma, sigma_prev, prev_sample, grad_log_prob, mean_ref=None, kl_weight=0.0,
                  noise_level=NOISE_LEVEL, scale=SCALE):
    """The closed form, float64.  Per token with p = pos, n = neg, c = n + s (p - n), a = ||p||, b = ||c||, r = a / b and g = dL/dv:
    dL/dc = r (g - (c.g) / b^2 c) ;  dL/dp = s dL/dc + (c.g) / (a b) p ;  dL/dn = (1 - s) dL/dc."""
    d = torch.float64
    B, C, H, W = x.shape
    n = x[0].numel()
    _, _, mean, _ = rescaled_step(sde_type, v_neg, v_pos, x, sigma, sigma_prev, noise_level, prev_sample=prev_sample, scale=scale)
    dmu, w2 = _dmu_dv(sde_type, sigma, sigma_prev, noise_level, d)
    g = _col(grad_log_prob.double() * (2.0 if w2 is None else 1 / w2) / n * dmu, x) * (prev_sample.double() - mean)
    if mean_ref is not None:
        g = g + _col(kl_weight * 2 * dmu / (n * B), x) * (mean - mean_ref.double())
    ng, ps, g = Q.pack(v_neg.to(d)), Q.pack(v_pos.to(d)), Q.pack(g)
    c = ng + scale * (ps - ng)
    a, b = ps.pow(2).sum(-1, keepdim=True).sqrt(), c.pow(2).sum(-1, keepdim=True).sqrt()
    cg = (c * g).sum(-1, keepdim=True)
    dc = (a / b) * (g - cg / b ** 2 * c)
    return Q.unpack((1 - scale) * dc, C, H, W), Q.unpack(scale * dc + cg / (a * b) * ps, C, H, W)


def _token_sum_kernel_order(t):
    """Packed [B, N, 64] float32, values ordered (channel, row, pixel) -> [B, N, 1]: four partials of 16 values (one per wave of four
    channels), each added one value after the other, then added in wave order 0..3."""
    parts = t.reshape(*t.shape[:-1], 4, 16)
    acc = torch.zeros_like(parts[..., 0])
    for i in range(16):
        acc = acc + parts[..., i]
    tot = torch.zeros_like(acc[..., 0])
    for w in range(4):
        tot = tot + acc[..., w]
    return tot.unsqueeze(-1)


def kernel_order_norms(v_neg, v_pos, scale=SCALE):
    """(||pos||, ||comb||) per token as the kernels round them: the combine in the predictions' dtype, float32 sums of squares in the
    kernel's order, sqrt, and the cast to bf16 on bf16 predictions.  Packed [B, N, 1] in the predictions' dtype."""
    neg, pos = Q.pack(v_neg), Q.pack(v_pos)
    comb = Q.combine(neg, pos, scale)
    cn = torch.sqrt(_token_sum_kernel_order(pos.float() * pos.float())).to(v_neg.dtype)
    nn = torch.sqrt(_token_sum_kernel_order(comb.float() * comb.float())).to(v_neg.dtype)
    return cn, nn


def grad_emulated_f32(sde_type, v_neg, v_pos, x, sigma, sigma_prev, prev_sample, grad_log_prob, mean_ref=None, kl_weight=0.0,
                      noise_level=NOISE_LEVEL, scale=SCALE):
    """The backward kernel's arithmetic with torch on the CPU: (grad_v_neg, grad_v_pos) in the predictions' dtype."""
    f = torch.float32
    vd = v_neg.dtype
    B, C, H, W = x.shape
    n = x[0].numel()
    neg, pos = Q.pack(v_neg), Q.pack(v_pos)
    comb = Q.combine(neg, pos, scale)                                           # three roundings in the predictions' dtype
    cn, nn = kernel_order_norms(v_neg, v_pos, scale)
    ratio = cn / nn                                                             # ... and the ratio and the product one each
    v = Q.unpack(comb * ratio, C, H, W)
    _, _, mean, _ = step(sde_type, v, x, sigma, sigma_prev, noise_level, prev_sample=prev_sample, dtype=f)
    dmu, w2 = _dmu_dv(sde_type, sigma, sigma_prev, noise_level, f)
    glp = grad_log_prob.to(f)
    nf = torch.tensor(float(n), dtype=f)
    lp_scale = glp * 2.0 / nf * dmu if w2 is None else glp / (nf * w2) * dmu
    g = _col(lp_scale, x) * (prev_sample.to(f) - mean)
    if mean_ref is not None:
        kl_scale = torch.tensor(kl_weight, dtype=f) * 2.0 / (nf * torch.tensor(float(B), dtype=f)) * dmu
        g = g + _col(kl_scale, x) * (mean - mean_ref.to(f))
    g, c, p, r, cn, nn = Q.pack(g), comb.to(f), pos.to(f), ratio.to(f), cn.to(f), nn.to(f)
    cg = _token_sum_kernel_order(c * g)
    dc = r * (g - cg / (nn * nn) * c)
    s = torch.tensor(scale, dtype=f)
    return Q.unpack(((1.0 - s) * dc).to(vd), C, H, W), Q.unpack((s * dc + cg / (cn * nn) * p).to(vd), C, H, W)


# ---------------------------------------------------------------------------------------------------------------- backward cases
PROJECT_BOUND = {torch.float32: 1e-5, bf16: 2e-2}     # of the gradient scale: tests/test_gpu_flow_sde.py, tests/test_gpu_sde_step.py
KL_WEIGHT = 0.37


def bwd_case(shape, dt, sde_type, with_kl, seed=None):
    """Inputs of one backward case on the CPU: predictions, sample and prev_sample in ``dt``; grad_log_prob scaled so that the policy and
    the KL gradients are of one order (as tests/test_gpu_flow_sde.py does)."""
    si = SHAPES.index(tuple(shape))
    seed = 5000 + 10 * si + (1 if dt == bf16 else 0) if seed is None else seed
    v_neg, v_pos, x = make_inputs(shape, dt, dt, 1.0, seed)
    g = torch.Generator().manual_seed(seed + 5)
    r_neg, r_pos = (torch.randn(shape, generator=g).to(dt) for _ in range(2))
    prev = (x.float() + 0.1 * torch.randn(shape, generator=g)).to(dt)
    glp = torch.randn(shape[0], generator=g) * (1e-3 if with_kl else 1.0)
    sig, sigp = schedule_rows(shape[0])
    mean_ref = None
    if with_kl:
        mean_ref = rescaled_step(sde_type, r_neg, r_pos, x, sig, sigp, prev_sample=prev)[2].float()
    return dict(v_neg=v_neg, v_pos=v_pos, x=x, prev=prev, glp=glp, sig=sig, sigp=sigp, mean_ref=mean_ref,
                kl_weight=KL_WEIGHT if with_kl else 0.0)


def bwd_cases():
    return [(shape, dt, sde_type, with_kl) for shape in SHAPES for dt in (torch.float32, bf16) for sde_type in ("cps", "sde")
            for with_kl in (False, True)]


def rel_err(got_neg, got_pos, ref_neg, ref_pos):
    """max |diff| over both gradients, as a share of the gradient scale max |d loss / d v_pos| (the project's measure)."""
    scale = ref_pos.abs().max().item()
    return max((got_neg.double() - ref_neg).abs().max().item(), (got_pos.double() - ref_pos).abs().max().item()) / scale


def measure_emulation():
    """{dtype: max over the case list of the float32 emulation's error against float64 autograd} and the GPU bound that follows: the
    project bound, or four times the measured error where that exceeds a quarter of it (the factor allows for the device's sqrt,
    division and reduction order differing from the emulation's)."""
    worst = {torch.float32: 0.0, bf16: 0.0}
    for shape, dt, sde_type, with_kl in bwd_cases():
        c = bwd_case(shape, dt, sde_type, with_kl)
        args = (sde_type, c["v_neg"], c["v_pos"], c["x"], c["sig"], c["sigp"], c["prev"], c["glp"], c["mean_ref"], c["kl_weight"])
        ref_n, ref_p, _ = grad_autograd(*args)
        emu_n, emu_p = grad_emulated_f32(*args)
        worst[dt] = max(worst[dt], rel_err(emu_n, emu_p, ref_n, ref_p))
    bound = {dt: PROJECT_BOUND[dt] if worst[dt] <= PROJECT_BOUND[dt] / 4 else 4 * worst[dt] for dt in worst}
    return worst, bound
