"""CLIP ViT-L/14 image-text score on the gfx950 kernels.

Mirror of adv_grpo/clip_scorer.py (``ClipScorer``, ``__call__(pixels, prompts) -> scores[N]``):
``exp(logit_scale) * <i / |i|, t / |t|> / 30`` per (image, prompt) pair, the diagonal of CLIPModel's ``logits_per_image``.
Differences that come with the platform:
  * the torchvision tensor transform (T.Resize(224) bilinear antialias -> T.CenterCrop(224) -> T.Normalize) runs as one kernel that
    writes the patch rows of the crop window (preprocess.tv_clip_patches, bit-equal to torch's GPU F.interpolate); pixels are a device
    tensor [N,3,H,W] f32 / bf16 (used as given, any H x W) or uint8 (divided by 255 in f32, the reference's ndarray path);
  * prompts are token ids: a rewards.PromptBatch carrying ``clip_ids`` (CLIP-L shares PickScore's OpenAI BPE vocabulary), an
    ``input_ids`` tensor [N,77], or strings with a ``tokenizer``; the text tower runs once per distinct prompt beside the image
    tower, as in PickScoreScorer;
  * weights come from a state dict + ClipConfig (hub.load_clip, ClipConfig.vit_l14()) or a built tower (``model``);
  * ``dtype`` selects the arithmetic: ``torch.float32`` (the reference's) runs vit_x3.CLIPModelX3, ``torch.bfloat16`` vit.CLIPModel;
    ``compute_dtype`` says which.  The score epilogue is f32 either way.
Scores stay on the device; nothing synchronises.
"""
import threading

import torch

from . import preprocess, vit, vit_x3
from .pickscore_scorer import PickScoreScorer


def clip_scores_f32(image_embs, text_embs, logit_scale, div=30.0):
    """CLIPModel.forward's logits_per_image diagonal / div in f32: exp(logit_scale) * <t / |t|, i / |i|> / div per pair."""
    i = image_embs.float()
    t = text_embs.float()
    i = i / i.norm(dim=-1, keepdim=True)
    t = t / t.norm(dim=-1, keepdim=True)
    return torch.as_tensor(logit_scale, device=i.device).exp() * (t * i).sum(-1) / div


class ClipScorer(PickScoreScorer):
    def __init__(self, device="cuda", dtype=torch.float32, model_sd=None, clip_cfg=None, tokenizer=None, model=None):
        torch.nn.Module.__init__(self)
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"ClipScorer: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        if model is None and (model_sd is None or clip_cfg is None):
            raise RuntimeError("ClipScorer needs model_sd + clip_cfg or a built tower (no checkpoint download on this platform)")
        tower = vit_x3.CLIPModelX3 if dtype == torch.float32 else vit.CLIPModel
        if model is None:
            model = tower(model_sd, clip_cfg, device)
        elif not isinstance(model, tower):
            raise ValueError(f"ClipScorer(dtype={dtype}) runs on a {tower.__name__}, got a {type(model).__name__}")
        self.model, self.dtype, self.tokenizer = model, dtype, tokenizer
        self.device = model.device
        self.compute_dtype = "bf16x3" if dtype == torch.float32 else "bf16"
        self._text_streams = {}
        self._text_streams_lock = threading.Lock()

    def _image_features(self, images):
        images = images.to(self.device)
        if images.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
            images = images.float()
        size = self.model.cfg.image_size
        if self.dtype == torch.float32:
            return self.model.get_image_features(pixel_patches3=preprocess.tv_clip_patches(images, size, x3=True))
        return self.model.get_image_features(pixel_patches=preprocess.tv_clip_patches(images, size))

    def _scores(self, image_embs, text_embs):
        return clip_scores_f32(image_embs, text_embs, self.model.logit_scale)

    @torch.no_grad()
    def __call__(self, pixels, prompts):
        """The reference's argument order (clip_scorer.py: pixels first)."""
        return PickScoreScorer.__call__(self, prompts, pixels)
