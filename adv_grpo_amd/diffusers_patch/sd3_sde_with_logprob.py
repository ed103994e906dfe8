"""Flow-CPS and Flow-SDE steps with per-sample log-prob on the fused gfx950 kernel.

Drop-in for adv_grpo/diffusers_patch/sd3_sde_with_logprob.py:77-139 (same name, argument
meaning and return tuple).  ``sde_step_cfg`` is the fused entry the rollout uses: it also
folds the CFG combine and the cast back to the latent dtype
(sd3_pipeline_with_logprob_fast.py:640-655) into the same HBM pass.

Names: ``sde_step_with_logprob`` and ``sde_step_with_logprob_new`` both mean Flow-CPS here (what the reference's rollouts import under
either name).  The reference's own ``sde_step_with_logprob`` (SDE:13-73, the original Flow-GRPO step with the full Gaussian log-density) is
``flow_sde_step_with_logprob``; ``sde_step_cfg(sde_type="sde")`` is its fused form.

``sde_step_cfg(cfg_rescale=True)`` replaces the SD3 combine by Qwen-Image's norm-rescaled true CFG (qwen_generate.py has the
deterministic sampler's form of it) in front of either step, still in one launch; ``rescaled_prediction`` is that combine as torch ops.
"""
import math

import torch

from .. import _lib


SDE_TYPES = ("cps", "sde")
_ENTRY = {"cps": "advgrpo_sde_step", "sde": "advgrpo_flow_sde_step"}   # + "", _branch, _bwd, _bwd_kl, _rescaled, _rescaled_bwd


def _sigma_tables(scheduler, timestep, B, device):
    """Per-sample (sigma, sigma_prev) device views + stride without a device sync."""
    ts = timestep.tolist() if isinstance(timestep, torch.Tensor) else list(timestep)
    idx = [scheduler.index_for_timestep(t) for t in ts]
    if len(set(idx)) == 1:
        i = idx[0]
        return scheduler.sigmas[i:i + 1], scheduler.sigmas[i + 1:i + 2], 0
    assert len(idx) == B
    ii = torch.tensor(idx, device=device)
    return scheduler.sigmas[ii].contiguous(), scheduler.sigmas[ii + 1].contiguous(), 1


def rescaled_prediction(v_uncond, v_text, guidance_scale):
    """Qwen-Image's true-CFG prediction as the torch ops of QwenImagePipeline.__call__, launch by launch, on unpacked [B, C, H, W]
    predictions: comb = neg + s (pos - neg), then comb * (||pos|| / ||comb||) over each 2 x 2 x C token, in the predictions' dtype."""
    from ..qwen_generate import _pack, _unpack
    B, C, H, W = v_uncond.shape
    neg, pos = _pack(v_uncond), _pack(v_text)
    comb = neg + guidance_scale * (pos - neg)
    cond_norm = torch.norm(pos, dim=-1, keepdim=True)
    noise_norm = torch.norm(comb, dim=-1, keepdim=True)
    return _unpack(comb * (cond_norm / noise_norm), C, H, W).contiguous()


def _step_head(v_uncond, v_text, guidance_scale, sample, sig, sigp, stride, sde_type, noise_level, tab, ptr=_lib.ptr):
    """What all twelve step entries start with: v_uncond .. sigma_stride, then the level -- sin(noise_level pi / 2) for Flow-CPS;
    noise_level and a device pointer to sigma_max = tab[1] (SDE:46) for Flow-SDE."""
    level = (float(noise_level), ptr(tab[1:2])) if sde_type == "sde" else (float(math.sin(noise_level * math.pi / 2)),)
    return (ptr(v_uncond), ptr(v_text), _lib.dtype_code(v_uncond.dtype), float(guidance_scale), ptr(sample),
            _lib.dtype_code(sample.dtype), ptr(sig), ptr(sigp), stride, *level)


def sde_step_cfg(scheduler, v_uncond, v_text, guidance_scale, timestep, sample, noise_level=0.7,
                 prev_sample=None, noise=None, seed=None, offset=0, out_dtype=None, want_mean=True,
                 step_index=None, sigmas=None, copies=None, sde_type="cps", cfg_rescale=False, sequenced=False):
    """Returns (prev_sample_f32_or_None, prev_sample_cast_or_None, log_prob, prev_sample_mean_or_None, std_dev_t).

    v_text=None => no CFG.  Exactly one of prev_sample (replay), noise (injected epsilon) or seed
    (in-kernel Philox) selects the mode.

    copies=G: the fan-out step of the branching rollouts (advgrpo_sde_step_branch).  v_uncond / v_text / sample hold P rows,
    noise / prev_sample and every output P * G rows; output row j continues input row j % P (``sample.repeat(G, 1, 1, 1)``)
    with its own epsilon -- the bits of this function on the repeated inputs, without the repeat and with one read of them.

    sde_type: "cps" (Flow-CPS, SDE:117-134: log_prob = -mean((x' - mean)^2)) or "sde" (Flow-SDE, SDE:44-71: the Gaussian log-density with
    its 1 / (2 w^2), log w and log sqrt(2 pi) terms; std_dev_t is returned without the sqrt(-dt)).  With "sde" and noise_level == 0 the
    step is the deterministic x + v * dt and log_prob is NaN, as in the reference.

    cfg_rescale=True (with v_text): Qwen-Image's norm-rescaled true CFG instead of the SD3 combine -- v = comb * ||v_text|| / ||comb|| over
    each 2 x 2 x 16 token -- fused with the step (advgrpo_sde_step_rescaled / advgrpo_flow_sde_step_rescaled); `sample` must be
    [B, 16, H, W] with even H, W.  Not with copies=.  With v_text=None it changes nothing.  sequenced=True runs the same rescaled step
    as separate operations (the torch combine and rescale, then this function's kernel with v_text=None): the check and the
    benchmark's baseline."""
    if sde_type not in SDE_TYPES:
        raise ValueError(f"sde_step_cfg: sde_type must be one of {SDE_TYPES}, got {sde_type!r}")
    rescale = bool(cfg_rescale) and v_text is not None
    if cfg_rescale and copies is not None:
        raise ValueError("sde_step_cfg(cfg_rescale=True): the fan-out step (copies=) has no rescaled form")
    if rescale and (sample.dim() != 4 or sample.shape[1] != 16 or v_uncond.shape != sample.shape or v_text.shape != sample.shape
                    or v_text.dtype != v_uncond.dtype):
        raise ValueError(f"sde_step_cfg(cfg_rescale=True): predictions and sample must be [B, 16, H, W] tensors of one shape, the "
                         f"predictions of one dtype; got {tuple(v_uncond.shape)}, {tuple(v_text.shape)}, {tuple(sample.shape)}")
    if rescale and sequenced:
        return sde_step_cfg(scheduler, rescaled_prediction(v_uncond, v_text, guidance_scale), None, 1.0, timestep, sample, noise_level,
                            prev_sample=prev_sample, noise=noise, seed=seed, offset=offset, out_dtype=out_dtype, want_mean=want_mean,
                            step_index=step_index, sigmas=sigmas, sde_type=sde_type)
    lib = _lib.load()
    P = sample.shape[0]
    B = P if copies is None else P * int(copies)
    out_shape = (B, *sample.shape[1:])
    n = sample[0].numel()
    dev = sample.device
    tab = scheduler.sigmas if sigmas is None else sigmas           # `sigmas`: the caller's rollout-local table
    if step_index is not None:
        sig, sigp, stride = tab[step_index:step_index + 1], tab[step_index + 1:step_index + 2], 0
    else:
        sig, sigp, stride = _sigma_tables(scheduler, timestep, P, dev)
    v_uncond = v_uncond.contiguous()
    v_text = v_text.contiguous() if v_text is not None else None
    sample = sample.contiguous()
    if prev_sample is not None:
        mode, prev_sample = _lib.SDE_REPLAY, prev_sample.contiguous()
    elif noise is not None:
        mode, noise = _lib.SDE_EPS, noise.contiguous().float()
    else:
        if seed is None:
            raise ValueError("sampling mode needs `noise` or `seed`")
        mode = _lib.SDE_PHILOX
    replay = mode == _lib.SDE_REPLAY
    for name, t in (("noise", noise if mode == _lib.SDE_EPS else None), ("prev_sample", prev_sample)):
        if copies is not None and t is not None and tuple(t.shape) != out_shape:
            raise ValueError(f"sde_step_cfg(copies={copies}): {name} must have the output's shape {out_shape}, got {tuple(t.shape)}")
    nxt = None if replay else torch.empty(out_shape, dtype=torch.float32, device=dev)
    cast = None
    if not replay and out_dtype is not None and out_dtype != torch.float32:
        cast = torch.empty(out_shape, dtype=out_dtype, device=dev)
    mean = torch.empty(out_shape, dtype=torch.float32, device=dev) if want_mean else None
    lp = torch.empty(B, dtype=torch.float32, device=dev)
    std = torch.empty(B, dtype=torch.float32, device=dev)
    if rescale:
        shape = (B, *sample.shape[1:], 2)                          # (B, C, H, W, patch_size) in place of (B, n)
        ws_bytes = lib.advgrpo_sde_step_rescaled_workspace_bytes(*shape)
    else:
        shape = ((B,) if copies is None else (P, int(copies))) + (n,)
        ws_bytes = lib.advgrpo_sde_step_workspace_bytes(B, n)
    ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device=dev)
    _lib.check(getattr(lib, _ENTRY[sde_type] + ("_rescaled" if rescale else "" if copies is None else "_branch"))(
        *_step_head(v_uncond, v_text, guidance_scale, sample, sig, sigp, stride, sde_type, noise_level, tab),
        mode, _lib.ptr(noise) if mode == _lib.SDE_EPS else None,
        int(seed or 0), int(offset), _lib.ptr(prev_sample) if replay else None,
        _lib.dtype_code(prev_sample.dtype) if replay else 0, _lib.ptr(nxt), _lib.ptr(cast),
        _lib.dtype_code(cast.dtype) if cast is not None else 0, _lib.ptr(mean), _lib.ptr(lp), _lib.ptr(std),
        _lib.ptr(ws), *shape, _lib.stream_ptr()))
    return nxt, cast, lp, mean, std.view(-1, *([1] * (sample.dim() - 1)))


def sde_step_cfg_bwd(scheduler, v_uncond, v_text, guidance_scale, sample, noise_level, prev_sample, grad_log_prob, step_index,
                     mean_ref=None, kl_weight=0.0, sde_type="cps", cfg_rescale=False):
    """Backward of the replay-mode ``sde_step_cfg`` at scheduler index `step_index`: d loss / d log_prob [B] in, (d loss / d v_uncond,
    d loss / d v_text, kl) out, the gradients in the predictions' dtype.  mean_ref (the same step's mean under the reference
    transformer) adds kl_weight * mean_b mean_elem (mean - mean_ref)^2 to the loss and returns its per-sample values in `kl` [B];
    without it kl is None.  The entry follows (sde_type, cfg_rescale, mean_ref is None): advgrpo_{,flow_}sde_step_bwd{,_kl}, or the one
    advgrpo_{,flow_}sde_step_rescaled_bwd whose mean_ref is nullable."""
    lib, tab, B, dev = _lib.load(), scheduler.sigmas, sample.shape[0], sample.device
    gu, gt = torch.empty_like(v_uncond), torch.empty_like(v_text)
    shape = (*sample.shape, 2) if cfg_rescale else (B, sample[0].numel())          # (B, C, H, W, patch_size) in place of (B, n)
    kl = ws = None
    if mean_ref is not None:
        query = lib.advgrpo_sde_step_rescaled_workspace_bytes if cfg_rescale else lib.advgrpo_sde_step_workspace_bytes
        kl = torch.empty(B, dtype=torch.float32, device=dev)
        ws = torch.empty(max(1, query(*shape) // 4), dtype=torch.float32, device=dev)
    suffix = "_rescaled_bwd" if cfg_rescale else "_bwd" if mean_ref is None else "_bwd_kl"
    ptr = lambda t: None if t is None else t.data_ptr()            # unchecked, as the G-step always passed its own fresh tensors
    kl_in, kl_out = ((), ()) if suffix == "_bwd" else ((ptr(mean_ref), float(kl_weight)), (ptr(kl), ptr(ws)))
    _lib.check(getattr(lib, _ENTRY[sde_type] + suffix)(
        *_step_head(v_uncond, v_text, guidance_scale, sample, tab[step_index:step_index + 1], tab[step_index + 1:step_index + 2], 0,
                    sde_type, noise_level, tab, ptr),
        ptr(prev_sample), _lib.dtype_code(prev_sample.dtype), ptr(grad_log_prob), *kl_in, ptr(gu), ptr(gt), *kl_out, *shape,
        _lib.stream_ptr()))
    return gu, gt, kl


def _step_with_logprob(sde_type, scheduler, model_output, timestep, sample, noise_level, prev_sample, generator, noise):
    seed = None
    if prev_sample is None and noise is None:
        if generator is not None:
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
        else:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    nxt, _, lp, mean, std = sde_step_cfg(scheduler, model_output, None, 1.0, timestep, sample, noise_level,
                                         prev_sample=prev_sample, noise=noise, seed=seed, sde_type=sde_type)
    if prev_sample is not None:
        nxt = prev_sample.float()
    return nxt, lp, mean, std


def sde_step_with_logprob(scheduler, model_output, timestep, sample, noise_level=0.7, prev_sample=None,
                          generator=None, noise=None):
    """Flow-CPS.  Reference signature (sd3_sde_with_logprob.py:77-85); returns
    (prev_sample, log_prob, prev_sample_mean, std_dev_t), all float32.
    ``generator``: a torch.Generator whose next int64 seeds the in-kernel Philox stream."""
    return _step_with_logprob("cps", scheduler, model_output, timestep, sample, noise_level, prev_sample, generator, noise)


sde_step_with_logprob_new = sde_step_with_logprob


def flow_sde_step_with_logprob(scheduler, model_output, timestep, sample, noise_level=0.7, prev_sample=None,
                               generator=None, noise=None):
    """Flow-SDE: the reference's ``sde_step_with_logprob`` (sd3_sde_with_logprob.py:13-73), its signature (plus ``noise=``) and its return
    tuple (prev_sample, log_prob, prev_sample_mean, std_dev_t), all float32; log_prob is the Gaussian log-density, mean over the elements."""
    return _step_with_logprob("sde", scheduler, model_output, timestep, sample, noise_level, prev_sample, generator, noise)
