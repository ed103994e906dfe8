"""The SD3 VAE encoder (adv_grpo_amd/vae_encoder.py, mode bf16x3) next to the decoder in the same mode in the same process: ms per batch and per
image at 512^2 and 1024^2 on synthetic weights (plain f32: both on three-product convolutions; fp16-checkpoint: the decoder as it is deployed,
on its two-product f16x2 path, which the encoder does not have), and one img2img call end to end (encode, noise, 15 denoise steps of a 2-block
MMDiT, decode).  Derived from the layer list the encoder is 0.53 T multiply-adds per 512^2 image against the decoder's 1.22 T (0.44): the
expectation printed beside the measured ratio is 0.44 x 1.5.  Prints one JSON line per measurement."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adv_grpo_amd import synthetic  # noqa: E402
from adv_grpo_amd.model_configs import MMDiTConfig, VaeConfig  # noqa: E402
from adv_grpo_amd.vae import AutoencoderKLDecoder  # noqa: E402
from adv_grpo_amd.vae_encoder import AutoencoderKLEncoder  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bench(B, size, fp16_checkpoint, iters):
    cfg = VaeConfig()
    enc = AutoencoderKLEncoder(synthetic.vae_encoder_weights(cfg, 1, fp16_checkpoint=fp16_checkpoint), cfg, "cuda")
    dec = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 2, fp16_checkpoint=fp16_checkpoint), cfg, "cuda", mode="bf16x3")
    dec.two_streams = False                                   # one chain against one chain
    img = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(0)).cuda()
    lat = enc.encode(img, seed=1)
    e_ms = timed(lambda: enc.encode(img, seed=1), iters)
    d_ms = timed(lambda: dec.decode_to_image(lat), iters)
    print(json.dumps({"shape": [B, 3, size, size], "mode": "bf16x3", "fp16_checkpoint": fp16_checkpoint, "decoder_arithmetic": dec.arithmetic()["text"],
                      "encode_ms": round(e_ms, 3), "decode_ms": round(d_ms, 3), "encode_ms_per_image": round(e_ms / B, 3),
                      "decode_ms_per_image": round(d_ms / B, 3), "encode_over_decode": round(e_ms / d_ms, 3), "expected_at_most": 0.66}))
    return enc, dec


def bench_img2img(enc, dec, B=2, size=512):
    from adv_grpo_amd.diffusers_patch.sd3_img2img_with_logprob import flux_to_sd3_denoise_random
    from adv_grpo_amd.mmdit import SD3Transformer2DModel
    from adv_grpo_amd.pipeline import SD3Pipeline
    mcfg = MMDiTConfig(num_layers=2, dual_attention_layers=(0,))
    W = {k: v.to(torch.bfloat16) for k, v in synthetic.mmdit_weights(mcfg, 3).items()}
    pipe = SD3Pipeline(SD3Transformer2DModel(W, mcfg, "cuda"), dec, "cuda", vae_encoder=enc)
    pe, ppe, npe, nppe = (t.to(torch.bfloat16).cuda() for t in synthetic.prompt_embeddings())
    img = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(1)).cuda()
    call = lambda: flux_to_sd3_denoise_random(pipe, flux_images=img, num_inference_steps=20, guidance_scale=4.5, prompt_embeds=pe, negative_prompt_embeds=npe,
                                              pooled_prompt_embeds=ppe, negative_pooled_prompt_embeds=nppe, target_idx=5, seed=7)
    ms = timed(call, 3, warmup=1)
    print(json.dumps({"img2img": [B, 3, size, size], "mmdit_layers": mcfg.num_layers, "start_step": 5, "denoise_steps": 15, "ms_per_call": round(ms, 2)}))


if __name__ == "__main__":
    for fp16 in (False, True):
        enc, dec = bench(4, 512, fp16, 5)
        bench(1, 1024, fp16, 3)
    bench_img2img(enc, dec)
