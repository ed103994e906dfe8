"""Qwen-Image text-to-image sampling on the gfx950 kernels: what the reference's reference-image scripts run
(qwen_generate.py:69-77, reference_imgs_scripts/qwen_generate_multi.py:61-68: ``QwenImagePipeline(prompt, negative_prompt=" ",
width=512, height=512, num_inference_steps=50, true_cfg_scale=4.0)``), and the file / json contract of those scripts.

``QwenImageSampler`` is diffusers' ``QwenImagePipeline.__call__`` over this package's towers: both prompts through the Qwen2.5-VL
encoder (masks kept), context embedding and all modulation rows once, latents as ``prepare_latents`` draws them, then per step two
transformer calls -- positive and negative as separate batches, each with its own ``encoder_hidden_states_mask``, as the pipeline does --
and ONE ``advgrpo_qwen_cfg_euler_step`` launch: the norm-rescaled "true CFG" combine and the Euler update of
``FlowMatchEulerDiscreteScheduler.step`` (scheduler.QwenImageFlowMatchScheduler holds the dynamic-shift table).  Then the existing Qwen
decode.  ``sequenced=True`` runs the step as the torch ops of the restatement, launch by launch: the check.  PARITY UNPINNED: the step's
rounding points and the schedule are restated from the published pipeline; scripts/verify_against_diffusers.py pins them where diffusers is
installed.  The SD3-style stochastic rollouts of config 5 keep their own combine (diffusers_patch/).

The second half of the module is the host logic of scripts/qwen_generate.py (file names, prompt suffixes, resume, the merged
``prompt2img.json``) as plain functions over a ``generate(prompts) -> images`` callable, so that a CPU test can drive them."""
import json
import os

import torch

from . import _lib
from .qwen_text_encoder import DROP_IDX
from .scheduler import QwenImageFlowMatchScheduler

# QwenImagePipeline.prompt_template_encode / tokenizer_max_length
PROMPT_TEMPLATE = ("<|im_start|>system\nDescribe the image by detailing the color, shape, size, texture, quantity, text, spatial relationships of "
                   "the objects and background:<|im_end|>\n<|im_start|>user\n{}<|im_end|>\n<|im_start|>assistant\n")
TOKENIZER_MAX_LENGTH = 1024
VAE_SCALE_FACTOR = 8
PATCH = 2


# ---------------------------------------------------------------------------------------------------------------- the step
def cfg_euler_step(v_neg, v_pos, sample, sigmas, step_index, true_cfg_scale, out=None):
    """One advgrpo_qwen_cfg_euler_step launch.  v_neg / v_pos / sample: [B, C, H, W]; v_pos=None: the plain Euler step on v_neg.
    sigmas: the device table; the kernel reads sigmas[step_index] and sigmas[step_index + 1] itself (no host value enters the launch,
    so a captured graph follows the table).  out may be `sample`."""
    B, C, H, W = sample.shape
    v_neg = v_neg.contiguous()
    v_pos = v_pos.contiguous() if v_pos is not None else None
    sample = sample.contiguous()
    if v_neg.shape != sample.shape or (v_pos is not None and (v_pos.shape != sample.shape or v_pos.dtype != v_neg.dtype)):
        raise ValueError("cfg_euler_step: predictions and sample must share one shape, the predictions one dtype")
    if out is None:
        out = torch.empty_like(sample)
    sig, nxt = sigmas[step_index:step_index + 1], sigmas[step_index + 1:step_index + 2]
    _lib.check(_lib.load().advgrpo_qwen_cfg_euler_step(
        _lib.ptr(v_neg), _lib.ptr(v_pos), _lib.dtype_code(v_neg.dtype), float(true_cfg_scale), _lib.ptr(sample),
        _lib.dtype_code(sample.dtype), _lib.ptr(sig), _lib.ptr(nxt), 0, _lib.ptr(out), B, C, H, W, PATCH, _lib.stream_ptr()))
    return out


def _pack(x):
    """QwenImagePipeline._pack_latents on [B, C, H, W] -> [B, N_img, C * 4]."""
    B, C, H, W = x.shape
    return x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), C * 4)


def _unpack(x, C, H, W):
    B = x.shape[0]
    return x.view(B, H // 2, W // 2, C, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def cfg_euler_step_sequenced(v_neg, v_pos, sample, sigmas, step_index, true_cfg_scale, f32=False):
    """The same step as the torch ops of QwenImagePipeline.__call__ and FlowMatchEulerDiscreteScheduler.step, launch by launch.
    f32=True: the predictions are upcast first, so no bf16 rounding point is left (the arithmetic's own noise floor)."""
    B, C, H, W = sample.shape
    if f32:
        v_neg, v_pos = v_neg.float(), (v_pos.float() if v_pos is not None else None)
    if v_pos is not None:
        neg, pos = _pack(v_neg), _pack(v_pos)
        comb = neg + true_cfg_scale * (pos - neg)
        cond_norm = torch.norm(pos, dim=-1, keepdim=True)
        noise_norm = torch.norm(comb, dim=-1, keepdim=True)
        pred = _unpack(comb * (cond_norm / noise_norm), C, H, W)
    else:
        pred = v_neg
    dt = sigmas[step_index + 1] - sigmas[step_index]            # 0-dim f32: torch casts it to bf16, the product stays bf16
    return (sample.to(torch.float32) + dt * pred).to(sample.dtype)


# ---------------------------------------------------------------------------------------------------------------- the sampler
def tokenize_prompts(tokenizer, prompts):
    """Strings -> (input_ids, attention_mask) the way QwenImagePipeline._get_qwen_prompt_embeds calls its tokenizer: the chat template
    around every prompt, padded to the longest, truncated at 1024 + the 34 template tokens that encode_prompt drops."""
    if tokenizer is None:
        raise RuntimeError("string prompts need a tokenizer callable (no tokenizer files ship with this package); pass input_ids instead")
    txt = [PROMPT_TEMPLATE.format(p) for p in prompts]
    tok = tokenizer(txt, max_length=TOKENIZER_MAX_LENGTH + DROP_IDX, padding=True, truncation=True, return_tensors="pt")
    return tok.input_ids, tok.attention_mask


class QwenImageSampler:
    def __init__(self, text_encoder, transformer, vae, scheduler=None, tokenizer=None):
        self.text_encoder, self.transformer, self.vae = text_encoder, transformer, vae
        self.scheduler = scheduler if scheduler is not None else QwenImageFlowMatchScheduler()
        self.tokenizer = tokenizer
        self.device = transformer.device

    def _ids(self, ids, mask):
        if isinstance(ids, str):
            ids = [ids]
        if isinstance(ids, (list, tuple)) and ids and isinstance(ids[0], str):
            return tokenize_prompts(self.tokenizer, list(ids))
        if mask is None:
            raise ValueError("QwenImageSampler: token ids need their attention_mask")
        return ids, mask

    def _encode(self, ids, mask, B):
        ids, mask = self._ids(ids, mask)
        emb, msk = self.text_encoder.encode_prompt(ids.to(self.device), mask, drop_idx=DROP_IDX)
        if emb.shape[0] == 1 and B > 1:                       # one negative prompt for the batch (the pipeline repeats it)
            emb, msk = emb.expand(B, -1, -1).contiguous(), msk.expand(B, -1).contiguous()
        if emb.shape[0] != B:
            raise ValueError(f"QwenImageSampler: {emb.shape[0]} prompts for a batch of {B}")
        return {"emb": emb, "mask": msk.to(self.device), "context": self.transformer.embed_context(emb)}

    @torch.no_grad()
    def prepare(self, input_ids, attention_mask=None, neg_input_ids=None, neg_attention_mask=None, height=512, width=512,
                num_inference_steps=50, true_cfg_scale=4.0, seed=0, noises=None):
        """Everything in front of the denoising loop -> the state dict `step` advances."""
        ids, mask = self._ids(input_ids, attention_mask)
        B = ids.shape[0]
        h, w = PATCH * (int(height) // (VAE_SCALE_FACTOR * PATCH)), PATCH * (int(width) // (VAE_SCALE_FACTOR * PATCH))
        C = self.transformer.cfg.out_channels
        st = {"pos": self._encode(ids, mask, B), "neg": None, "scale": float(true_cfg_scale), "n": int(num_inference_steps)}
        if true_cfg_scale > 1 and neg_input_ids is not None:     # the pipeline's do_true_cfg
            st["neg"] = self._encode(neg_input_ids, neg_attention_mask, B)
        timesteps = self.scheduler.set_timesteps(st["n"], (h // PATCH) * (w // PATCH), device=self.device)
        st["timesteps"], st["sigmas"] = timesteps, self.scheduler.sigmas
        st["mods"] = self.transformer.precompute_mods(timesteps)
        if noises is not None:
            if tuple(noises.shape) != (B, C, h, w):
                raise ValueError(f"QwenImageSampler: noises must be {(B, C, h, w)}, got {tuple(noises.shape)}")
            lat = noises.to(device=self.device, dtype=torch.bfloat16).contiguous().clone()
        else:                                                     # prepare_latents: randn of [B, 1, C, h, w] in the embeddings' dtype
            gen = torch.Generator(device=self.device).manual_seed(int(seed))
            lat = torch.randn((B, 1, C, h, w), generator=gen, device=self.device, dtype=torch.bfloat16)[:, 0].contiguous()
        st["latents"] = lat
        return st

    def _predict(self, st, side, i):
        p = st[side]
        return self.transformer(st["latents"], st["timesteps"][i:i + 1], p["emb"], mods=st["mods"][i], context=p["context"],
                                encoder_hidden_states_mask=p["mask"])[0]

    @torch.no_grad()
    def step(self, st, i, sequenced=False, step_f32=False):
        """Denoising step i: two transformer calls and the fused combine + Euler launch, in place on st["latents"]."""
        v_pos = self._predict(st, "pos", i)
        v_neg = self._predict(st, "neg", i) if st["neg"] is not None else None
        v, vp = (v_neg, v_pos) if v_neg is not None else (v_pos, None)
        if sequenced:
            st["latents"].copy_(cfg_euler_step_sequenced(v, vp, st["latents"], st["sigmas"], i, st["scale"], f32=step_f32))
        else:
            cfg_euler_step(v, vp, st["latents"], st["sigmas"], i, st["scale"], out=st["latents"])
        return st["latents"]

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, neg_input_ids=None, neg_attention_mask=None, height=512, width=512,
                 num_inference_steps=50, true_cfg_scale=4.0, seed=0, noises=None, output_type="pt", sequenced=False, step_f32=False):
        """-> images [B, 3, height, width] f32 in [0, 1] ("pt"), a list of PIL images ("pil") or the final latents ("latent").
        input_ids / neg_input_ids: token ids after the chat template with their masks, or strings (through the injected tokenizer)."""
        if output_type not in ("pt", "pil", "latent"):
            raise ValueError(f"QwenImageSampler: output_type must be 'pt', 'pil' or 'latent', got {output_type!r}")
        if step_f32 and not sequenced:
            raise ValueError("QwenImageSampler: step_f32 is a mode of the sequenced check")
        st = self.prepare(input_ids, attention_mask, neg_input_ids, neg_attention_mask, height, width, num_inference_steps,
                          true_cfg_scale, seed, noises)
        for i in range(st["n"]):
            self.step(st, i, sequenced=sequenced, step_f32=step_f32)
        if output_type == "latent":
            return st["latents"]
        image = self.vae.decode_to_image(st["latents"])
        return to_pil(image) if output_type == "pil" else image


def to_pil(image):
    """[B, 3, H, W] in [0, 1] -> PIL images (diffusers' VaeImageProcessor: * 255, round, uint8)."""
    from PIL import Image
    arr = (image.float().clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    return [Image.fromarray(a) for a in arr]


# ---------------------------------------------------------------------------------------------------------------- the tool's host logic
POSITIVE_MAGIC = {"en": ", Ultra HD, 4K, cinematic composition.", "zh": ", 超清，4K，电影级构图."}     # qwen_generate.py:15-18
NEGATIVE_PROMPT = " "                                                                               # :19
JSON_NAME = "prompt2img.json"


def read_prompts(path):
    with open(path, "r", encoding="utf-8") as f:                  # :101-102
        return [line.strip() for line in f if line.strip()]


def final_prompt(p):
    return p + (POSITIVE_MAGIC["en"] if all(ord(c) < 128 for c in p) else POSITIVE_MAGIC["zh"])    # :62-66


def image_name(rank, index):
    return f"rank{rank}_{index:05d}.png"                          # :42


def split_prompts(prompts, n_ranks):
    """numpy.array_split's sizes (:106): the first len % n ranks take one prompt more."""
    q, r = divmod(len(prompts), n_ranks)
    out, at = [], 0
    for k in range(n_ranks):
        size = q + (1 if k < r else 0)
        out.append(list(prompts[at:at + size]))
        at += size
    return out


def generate_rank(generate, prompts, rank, out_dir, batch_size=4, log=None):
    """One rank's loop (:38-87) -> {prompt: file name}.  generate(list of final prompts) -> as many images, each with .save(path).
    A prompt whose file exists is recorded and skipped (resume); a batch with nothing left to do never reaches `generate`."""
    os.makedirs(out_dir, exist_ok=True)
    local = {}
    for i in range(0, len(prompts), batch_size):
        todo = []
        for j, p in enumerate(prompts[i:i + batch_size]):
            name = image_name(rank, i + j)
            path = os.path.join(out_dir, name)
            if os.path.exists(path):
                local[p] = name
                if log:
                    log(f"exists: {path}")
            else:
                todo.append((p, path, name))
        if not todo:
            continue
        images = generate([final_prompt(p) for p, _, _ in todo])
        if len(images) != len(todo):
            raise RuntimeError(f"generate returned {len(images)} images for {len(todo)} prompts")
        for (p, path, name), img in zip(todo, images):
            img.save(path)
            local[p] = name
    return local


def merge_maps(maps):
    """The ranks' maps in rank order -> one dict (:118-121: dict.update, a later rank's entry for a repeated prompt wins)."""
    out = {}
    for m in maps:
        out.update(m)
    return out


def write_json(out_dir, mapping):
    path = os.path.join(out_dir, JSON_NAME)
    with open(path, "w", encoding="utf-8") as f:                  # :127-129
        json.dump(mapping, f, ensure_ascii=False, indent=2)
    return path
