"""Restatement, for the tests, of one Qwen-Image sampling step and of its sigma schedule: diffusers' ``QwenImagePipeline.__call__``
(the norm-rescaled "true CFG" combine on packed [B, N_img, 64] latents), ``FlowMatchEulerDiscreteScheduler.step`` and the
scheduler's ``set_timesteps`` under Qwen-Image's configuration (dynamic exponential shift, shift_terminal 0.02).  PARITY UNPINNED:
written from the published code, no diffusers is installed where the suite runs (scripts/verify_against_diffusers.py compares
where one is).

``cfg_euler_step`` is the pipeline's operation sequence in the tensors' own dtypes -- one torch op per rounding:

    comb = neg + scale * (pos - neg)                                   three bf16 roundings on bf16 predictions
    cn   = norm(pos, dim=-1) ; nn = norm(comb, dim=-1)                 f32 accumulation, result in the predictions' dtype
    out  = comb * (cn / nn)
    prev = (sample.float() + dt * out).to(sample.dtype)                dt a 0-dim f32 tensor: torch casts it to bf16 first, dt * bf16 stays bf16

``cfg_euler_step_f64`` is the same arithmetic in float64 with no rounding point.  ``CASES`` / ``make_inputs`` are the inputs of
tests/test_gpu_qwen_sampler.py, shared with tests/test_qwen_sampler_host.py (same seeds)."""
import math

import numpy as np
import torch

SCALE = 4.0
SHAPES = [(1, 16, 2, 2), (2, 16, 6, 10), (1, 16, 2, 258), (3, 16, 64, 64)]
MULTS = [1.0, 1e-3, 30.0]
MISMATCH_CAP = 0.01          # share of tokens whose bf16 norm may round the other way under another summation order


def pack(x):
    """QwenImagePipeline._pack_latents: [B, C, H, W] -> [B, (H/2)(W/2), C * 4], a token's values ordered (c, py, px)."""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), C * 4)


def unpack(x, C, H, W):
    B = x.shape[0]
    return x.reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def combine(v_neg, v_pos, scale=SCALE):
    return v_neg + scale * (v_pos - v_neg)


def rescale(comb, pos):
    """Packed [B, N, 64] tensors -> comb * (||pos|| / ||comb||), token by token."""
    cond_norm = torch.norm(pos, dim=-1, keepdim=True)
    noise_norm = torch.norm(comb, dim=-1, keepdim=True)
    return comb * (cond_norm / noise_norm)


def euler(sample, pred, sigma, sigma_next):
    """FlowMatchEulerDiscreteScheduler.step: sigma / sigma_next 0-dim f32 tensors (entries of the table)."""
    dt = sigma_next - sigma
    return (sample.to(torch.float32) + dt * pred).to(sample.dtype)


def cfg_euler_step(v_neg, v_pos, sample, sigma, sigma_next, scale=SCALE):
    B, C, H, W = sample.shape
    if v_pos is None:
        return euler(sample, v_neg, sigma, sigma_next)
    neg, pos = pack(v_neg), pack(v_pos)
    return euler(sample, unpack(rescale(combine(neg, pos, scale), pos), C, H, W), sigma, sigma_next)


def cfg_euler_step_f64(v_neg, v_pos, sample, sigma, sigma_next, scale=SCALE):
    d = torch.float64
    B, C, H, W = sample.shape
    pred = v_neg.to(d)
    if v_pos is not None:
        neg, pos = pack(v_neg.to(d)), pack(v_pos.to(d))
        comb = neg + scale * (pos - neg)
        pred = unpack(comb * (pos.pow(2).sum(-1, keepdim=True).sqrt() / comb.pow(2).sum(-1, keepdim=True).sqrt()), C, H, W)
    return sample.to(d) + (sigma_next.to(d) - sigma.to(d)) * pred


def token_norm_mismatch_share(x):
    """x packed [B, N, 64] bf16: the share of tokens whose torch bf16 norm differs from the float64 sum rounded to bf16."""
    a = torch.norm(x, dim=-1)
    b = x.double().pow(2).sum(-1).sqrt().to(torch.bfloat16)
    return (a != b).double().mean().item()


def make_inputs(shape, v_dtype, x_dtype, mult, seed):
    """(v_neg, v_pos, sample) on the CPU: N(0, 1) * mult drawn in f32, then cast."""
    g = torch.Generator().manual_seed(seed)
    v_neg, v_pos, sample = (torch.randn(shape, generator=g) * mult for _ in range(3))
    return v_neg.to(v_dtype), v_pos.to(v_dtype), sample.to(x_dtype)


def cases():
    """(id, shape, v_dtype, x_dtype, mult, seed) of every kernel-against-restatement case."""
    out = []
    for si, shape in enumerate(SHAPES):
        for vi, vd in enumerate((torch.bfloat16, torch.float32)):
            for xi, xd in enumerate((torch.bfloat16, torch.float32)):
                for mi, mult in enumerate(MULTS):
                    name = "x".join(map(str, shape)) + f"-v{'bf16' if vi == 0 else 'f32'}-x{'bf16' if xi == 0 else 'f32'}-m{mult:g}"
                    out.append((name, shape, vd, xd, mult, 1000 + 100 * si + 10 * (2 * vi + xi) + mi))
    return out


# ---------------------------------------------------------------------------------------------------------------- schedule
def calculate_shift(image_seq_len, base_seq_len=256, max_seq_len=8192, base_shift=0.5, max_shift=0.9):
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    b = base_shift - m * base_seq_len
    return image_seq_len * m + b


def schedule_f64(n, image_seq_len, shift_terminal=0.02):
    """-> (sigmas [n + 1], timesteps [n]) as python floats (float64), element by element."""
    mu = calculate_shift(image_seq_len)
    raw = [1.0 + (1.0 / n - 1.0) * i / (n - 1) if n > 1 else 1.0 for i in range(n)]          # linspace(1, 1/n, n)
    s = [math.exp(mu) / (math.exp(mu) + (1.0 / t - 1.0)) for t in raw]
    k = (1.0 - s[-1]) / (1.0 - shift_terminal)
    s = [1.0 - (1.0 - v) / k for v in s]
    return s + [0.0], [1000.0 * v for v in s]


def schedule(n, image_seq_len, shift_terminal=0.02):
    """The float32 table: the float64 restatement rounded once."""
    sig, _ = schedule_f64(n, image_seq_len, shift_terminal)
    sig = np.asarray(sig, dtype=np.float64).astype(np.float32)
    return sig, sig[:-1] * np.float32(1000.0)
