"""SD3 VAE encoder on the gfx950 kernels (host orchestration only).

Stands in for ``pipe.vae.encode(img_tensor).latent_dist.sample() * pipe.vae.config.scaling_factor`` of the reference's
``image_to_latent`` (adv_grpo/diffusers_patch/sd3_pipeline_with_logprob_fast.py:686-705): diffusers' AutoencoderKL encoder in the SD3 /
SD3.5 configuration -- conv_in, four down blocks of two resnets (the first three followed by Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1))
+ a 3x3 convolution of stride 2), mid block (resnet, single-head attention, resnet), GroupNorm + SiLU, conv_out to 2 * latent_channels
moments, no quant_conv.  The other half of the model adv_grpo_amd/vae.py decodes with; it reuses that class's GroupNorm, split-operand
convolution, resnet and mid-block attention sequencing.

Arithmetic: the reference runs the VAE in fp32 (train_sd3_fast_pickscore.py:481), so the only mode is the decoder's default
fp32-equivalent ``mode="bf16x3"`` -- split-bf16 operands, three MFMA products per f32 product, f32 between two matrix products.  Every
convolution runs on the three-product form: the two-product f16x2 path of the decoder (fp16-exact checkpoints) and ``mode="bf16"`` have no
strided kernel and are refused.  Activations NHWC; the (0, 1, 0, 1) zero padding of the downsamplers is folded into the strided
convolution's tap addressing (csrc/conv_x3.hip), the 3 image channels are padded to one 64-channel slice for conv_in.

Sizes: H and W multiples of 8 (three halvings) with (H / 8) * (W / 8) a multiple of 64 (the mid attention's P . V product contracts over
3 x that many split columns in 64-wide k-tiles): 64 x 64, 64 x 128, 128 x 128, 512 x 512, 1024 x 1024, ...

DEVIATION kept from the reference: the latents are ``sample * scaling_factor`` WITHOUT ``- shift_factor`` (PF:704 does not subtract it,
although the decode at PF:1074 adds it back).
"""
import ctypes

import torch

from . import _lib, ops
from .vae import AutoencoderKLDecoder

SIZE_MULTIPLE = 8
TOKEN_MULTIPLE = 64


class AutoencoderKLEncoder(AutoencoderKLDecoder):
    _prefix = "encoder."
    c_encode = True                  # the chain through advgrpo_vae_encode (one C-ABI call per batch); False: launch by launch

    def __init__(self, state_dict, cfg, device="cuda", mode="bf16x3"):
        if mode != "bf16x3":
            raise ValueError(f"AutoencoderKLEncoder: only mode='bf16x3' (the reference's fp32 arithmetic on split-bf16 operands) is implemented, "
                             f"got {mode!r}; the decoder's 'bf16' mode and its f16x2 path have no strided convolution")
        if not any(k.startswith("encoder.") for k in state_dict):
            raise ValueError("AutoencoderKLEncoder: the state dict has no encoder.* tensors (hub.load_vae_encoder / synthetic.vae_encoder_weights)")
        if any(k.startswith("quant_conv.") for k in state_dict):
            raise ValueError("AutoencoderKLEncoder: a quant_conv behind the encoder (use_quant_conv) is not implemented")
        super().__init__(state_dict, cfg, device, mode="bf16x3", f16_weights=False)
        self._edesc = None           # (key, descriptor, host arrays): rebuilt when a weight tensor it points at has been replaced

    # ------------------------------------------------------------------ launch by launch (the check of the C entry)
    def _check_images(self, images):
        if images.dtype == torch.uint8:
            ok, (B, H, W) = images.dim() == 4 and images.shape[-1] == 3, (images.shape[0], images.shape[1], images.shape[2]) if images.dim() == 4 else (0, 0, 0)
        else:
            ok = images.dim() == 4 and images.shape[1] == 3 and images.dtype in (torch.float32, torch.bfloat16)
            B, H, W = (images.shape[0], images.shape[2], images.shape[3]) if images.dim() == 4 else (0, 0, 0)
        if not ok:
            raise ValueError(f"AutoencoderKLEncoder: images must be [B,3,H,W] f32 / bf16 in [0,1] or uint8 [B,H,W,3], got {tuple(images.shape)} {images.dtype}")
        if B < 1 or H < SIZE_MULTIPLE or W < SIZE_MULTIPLE or H % SIZE_MULTIPLE or W % SIZE_MULTIPLE or (H // 8) * (W // 8) % TOKEN_MULTIPLE:
            raise ValueError(f"AutoencoderKLEncoder: image height and width must be multiples of {SIZE_MULTIPLE} with (H / 8) * (W / 8) a multiple of "
                             f"{TOKEN_MULTIPLE} (64 x 64, 128 x 128, 512 x 512, 1024 x 1024, ...), got {H} x {W}")
        if not images.is_cuda:
            raise _lib.AdvGrpoError("AutoencoderKLEncoder takes device tensors; there is no CPU path")
        return B, H, W

    def _moments_chain(self, images):
        cfg = self.cfg
        x = self._conv3("encoder.conv_in", ops.image_to_nhwc_x3(images, 64))
        n = len(cfg.block_out_channels)
        for i in range(n):
            for j in range(cfg.layers_per_block):
                x = self._res3(f"encoder.down_blocks.{i}.resnets.{j}", x)
            if i < n - 1:
                p = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                x = ops.conv3x3_s2_x3(ops.split_x3(x, order=2), self.w[p + ".weight"], bias=self.w[p + ".bias"])
        x = self._res3("encoder.mid_block.resnets.0", x)
        x = self._attn3("encoder.mid_block.attentions.0", x)
        x = self._res3("encoder.mid_block.resnets.1", x)
        return self._conv3("encoder.conv_out", self._gn3("encoder.conv_norm_out", x, True))

    # ------------------------------------------------------------------ one C-ABI call
    def _e_desc(self):
        w, cfg = self.w, self.cfg
        key = tuple(t.data_ptr() for _, t in sorted(w.items()))
        with self._side_lock:
            if self._edesc is not None and self._edesc[0] == key:
                return self._edesc[1]

            def conv(name):
                c = _lib.VaeConv()
                t = w[name + ".weight"]
                c.w, c.cin, c.cout, c.form = t.data_ptr(), t.shape[1] // 27, t.shape[0], 0
                c.bias = w[name + ".bias"].data_ptr()
                return c

            def resnet(r, p):
                r.norm1_w, r.norm1_b = w[f"{p}.norm1.weight"].data_ptr(), w[f"{p}.norm1.bias"].data_ptr()
                r.norm2_w, r.norm2_b = w[f"{p}.norm2.weight"].data_ptr(), w[f"{p}.norm2.bias"].data_ptr()
                r.conv1, r.conv2 = conv(f"{p}.conv1"), conv(f"{p}.conv2")
                sc = w.get(f"{p}.conv_shortcut.weight")
                r.shortcut_w = sc.data_ptr() if sc is not None else None
            n, per = len(cfg.block_out_channels), cfg.layers_per_block
            d = _lib.VaeDecoderDesc()
            d.latent_channels, d.groups, d.n_up, d.resnets_per_up, d.f16_single = cfg.latent_channels, self.G, n, per, 0
            d.scaling_factor, d.shift_factor = cfg.scaling_factor, cfg.shift_factor
            d.conv_in, d.conv_out = conv("encoder.conv_in"), conv("encoder.conv_out")
            d.norm_out_w, d.norm_out_b = w["encoder.conv_norm_out.weight"].data_ptr(), w["encoder.conv_norm_out.bias"].data_ptr()
            resnet(d.mid[0], "encoder.mid_block.resnets.0")
            resnet(d.mid[1], "encoder.mid_block.resnets.1")
            a = "encoder.mid_block.attentions.0"
            d.attn_norm_w, d.attn_norm_b = w[f"{a}.group_norm.weight"].data_ptr(), w[f"{a}.group_norm.bias"].data_ptr()
            for k, nm in (("q", "to_q"), ("k", "to_k"), ("v", "to_v"), ("o", "to_out.0")):
                setattr(d, f"attn_{k}_w", w[f"{a}.{nm}.weight"].data_ptr())
                setattr(d, f"attn_{k}_b", w[f"{a}.{nm}.bias"].data_ptr())
            downs = (_lib.VaeResnet * (n * per))()
            for i in range(n):
                for j in range(per):
                    resnet(downs[i * per + j], f"encoder.down_blocks.{i}.resnets.{j}")
            samp = (_lib.VaeConv * max(1, n - 1))()
            for i in range(n - 1):
                samp[i] = conv(f"encoder.down_blocks.{i}.downsamplers.0.conv")
            d.up_resnets, d.upsamplers = ctypes.cast(downs, ctypes.POINTER(_lib.VaeResnet)), ctypes.cast(samp, ctypes.POINTER(_lib.VaeConv))
            zero = ops.zero_page(self.device)
            d.zero_page = zero.data_ptr()
            self._edesc = (key, d, (downs, samp, zero))
            return d

    def _moments_c(self, images):
        lib = _lib.load()
        images = images.contiguous()
        B, H, W = self._check_images(images)
        d = _lib.VaeDecoderDesc.from_buffer_copy(self._e_desc())
        d.B, d.h, d.w = B, H, W
        down = 2 ** (len(self.cfg.block_out_channels) - 1)
        mom = torch.empty(B, H // down, W // down, 2 * self.cfg.latent_channels, dtype=torch.float32, device=images.device)
        ws = torch.empty(int(lib.advgrpo_vae_encode_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8, device=images.device)
        code = _lib.U8 if images.dtype == torch.uint8 else _lib.dtype_code(images.dtype)
        _lib.check(lib.advgrpo_vae_encode(ctypes.byref(d), images.data_ptr(), code, mom.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return mom

    def _moments_nhwc(self, images):
        self._check_images(images)
        return self._moments_c(images) if self.c_encode else self._moments_chain(images)

    # ------------------------------------------------------------------ public surface
    @torch.no_grad()
    def moments(self, images):
        """images [B,3,H,W] in [0,1] (f32 / bf16) or uint8 [B,H,W,3] -> f32 [B, 2C, H/8, W/8]: mean | logvar of the latent distribution
        (what ``vae.encode(2 x - 1).latent_dist.parameters`` holds)."""
        return self._moments_nhwc(images).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def encode(self, images, seed=None, noise=None, sample=True, out_dtype=torch.bfloat16):
        """-> latents * scaling_factor [B,C,H/8,W/8] in out_dtype (PF:703-705; shift_factor is NOT subtracted, as there).
        sample=False: the distribution's mean.  Otherwise eps = `noise` ([B,C,h,w] f32, injected) or the in-kernel Philox stream of
        (seed, offset 0) -- element i is advgrpo_randn's element i for the same seed; seed None draws one from torch's generator."""
        mom = self._moments_nhwc(images)
        if not sample:
            return ops.vae_latent_tail(mom, self.cfg.scaling_factor, "mean", out_dtype=out_dtype)
        if noise is not None:
            return ops.vae_latent_tail(mom, self.cfg.scaling_factor, "eps", eps=noise.to(device=mom.device, dtype=torch.float32).contiguous(),
                                       out_dtype=out_dtype)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return ops.vae_latent_tail(mom, self.cfg.scaling_factor, "philox", seed=seed, offset=0, out_dtype=out_dtype)

    @torch.no_grad()
    def encode_and_noise(self, images, sigma, seed=None, noise=None, mix_noise=None, sample=True):
        """encode() to bf16 and, in the same launch, the forward noising of flux_to_sd3_denoise_random (PF:961-965) with the reference's
        rounding points: (1 - sigma) * z + sigma * noise in bf16 arithmetic.  sigma: device f32 scalar tensor (the scheduler's value; rounded
        to bf16 in the kernel).  mix_noise injected ([B,C,h,w]) or Philox of (seed, counters behind the sampling draw's).
        -> (latents bf16, noised latents bf16)."""
        mom = self._moments_nhwc(images)
        B, h, w, C2 = mom.shape
        ctr = (B * h * w * (C2 // 2) + 3) // 4 + 1
        if seed is None and (mix_noise is None or (sample and noise is None)):
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        mode = "mean" if not sample else ("eps" if noise is not None else "philox")
        eps = None if noise is None else noise.to(device=mom.device, dtype=torch.float32).contiguous()
        mn = None if mix_noise is None else mix_noise.to(mom.device).contiguous()
        sigma = sigma.to(device=mom.device, dtype=torch.float32).reshape(1)
        return ops.vae_latent_tail(mom, self.cfg.scaling_factor, mode, eps=eps, seed=seed or 0, offset=0, out_dtype=torch.bfloat16,
                                   sigma=sigma, mix_noise=mn, mix_seed=seed or 0, mix_offset=ctr)

    def decode_to_image(self, latents):
        raise TypeError("AutoencoderKLEncoder encodes; decode with AutoencoderKLDecoder")
