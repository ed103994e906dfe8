"""Restatement of the Flow-SDE step (adv_grpo/diffusers_patch/sd3_sde_with_logprob.py:13-73, the reference's `sde_step_with_logprob`) for
the tests: float64 by default, parity-pinned by tests/golden/flow_sde.npz (tests/test_flow_sde_host.py).

With ``dtype=torch.float32`` the same lines are the reference's own float32 operation sequence (sigma a [B, 1, ...] tensor, sigma_max and
noise_level python floats, `**2`, one torch op per rounding): what the kernel's mean / next are compared with bit for bit.

    dt = sigma_prev - sigma
    s  = sqrt(sigma / (1 - (sigma == 1 ? sigma_max : sigma))) * noise_level          (std_dev_t)
    mu = x * (1 + s^2 / (2 sigma) * dt) + v * (1 + s^2 (1 - sigma) / (2 sigma)) * dt
    w  = s * sqrt(-dt)
    x' = mu + w * eps            (or the given prev_sample)
    lp = mean_i( -(x'_i - mu_i)^2 / (2 w^2) - log w - log sqrt(2 pi) )
"""
import math

import torch

LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)        # 0.9189385...


def cfg_combine(v_uncond, v_text, guidance_scale):
    """u + s * (t - u) in the tensors' own dtype: three roundings in bf16, one per torch op (sd3_pipeline_with_logprob_fast.py:640-642)."""
    return v_uncond + guidance_scale * (v_text - v_uncond)


def flow_sde_step(v, x, sigma, sigma_prev, sigma_max, noise_level, eps=None, prev_sample=None, dtype=torch.float64):
    """v, x: [B, ...]; sigma, sigma_prev: [B] float32 schedule entries; sigma_max: the schedule's sigmas[1] (a float).
    -> (prev_sample, log_prob [B], prev_sample_mean, std_dev_t [B], w [B]) in ``dtype``."""
    v, x = v.to(dtype), x.to(dtype)
    shape = (-1,) + (1,) * (x.dim() - 1)
    sigma, sigma_prev = sigma.to(dtype).view(shape), sigma_prev.to(dtype).view(shape)
    sigma_max = float(sigma_max)
    dt = sigma_prev - sigma                                                                   # :47
    std_dev_t = torch.sqrt(sigma / (1 - torch.where(sigma == 1, sigma_max, sigma))) * noise_level   # :49
    mean = x * (1 + std_dev_t ** 2 / (2 * sigma) * dt) + v * (1 + std_dev_t ** 2 * (1 - sigma) / (2 * sigma)) * dt   # :53
    w = std_dev_t * torch.sqrt(-1 * dt)
    if prev_sample is None:
        prev_sample = mean + std_dev_t * torch.sqrt(-1 * dt) * eps.to(dtype)                  # :62
    else:
        prev_sample = prev_sample.to(dtype)
    log_prob = (-((prev_sample.detach() - mean) ** 2) / (2 * (w ** 2)) - torch.log(w)
                - torch.log(torch.sqrt(2 * torch.as_tensor(math.pi, dtype=dtype))))          # :64-68
    log_prob = log_prob.mean(dim=tuple(range(1, log_prob.ndim)))                              # :71
    return prev_sample, log_prob, mean, std_dev_t.reshape(-1), w.reshape(-1)


def log_prob_bound(prev_sample, mean, w):
    """The project's 2e-6 relative bound for f32 sums of this length (tests/test_gpu_leaf_kernels.py), applied to the sum of the magnitudes of
    the three terms of the log-density -- q = sum d^2 / (2 n w^2), log w and log sqrt(2 pi) -- because they cancel near the end of a schedule."""
    d = prev_sample.double() - mean.double()
    w = w.double().reshape(-1)
    q = (d ** 2).flatten(1).mean(1) / (2 * w ** 2)
    return 2e-6 * (q.abs() + torch.log(w).abs() + 0.919)


def grad_v(v, x, sigma, sigma_prev, sigma_max, noise_level, prev_sample, grad_log_prob, mean_ref=None, kl_weight=0.0):
    """The closed forms the backward kernels evaluate, in float64: with c_v = (1 + s^2 (1 - sigma) / (2 sigma)) dt,
    g_v = grad_log_prob[b] (prev - mu) c_v / (n w^2)  [+ kl_weight 2 (mu - mu_ref) c_v / (n B)]."""
    _, _, mean, s, w = flow_sde_step(v, x, sigma, sigma_prev, sigma_max, noise_level, prev_sample=prev_sample)
    shape = (-1,) + (1,) * (x.dim() - 1)
    sg, dt = sigma.double().view(shape), (sigma_prev.double() - sigma.double()).view(shape)
    s, w = s.view(shape), w.view(shape)
    c_v = (1 + s ** 2 * (1 - sg) / (2 * sg)) * dt
    n, B = x[0].numel(), x.shape[0]
    g = grad_log_prob.double().view(shape) * (prev_sample.double() - mean) * c_v / (n * w ** 2)
    if mean_ref is not None:
        g = g + kl_weight * 2 * (mean - mean_ref.double()) * c_v / (n * B)
    return g
