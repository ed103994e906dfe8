"""LAION aesthetic predictor on the gfx950 kernels.

Mirror of adv_grpo/aesthetic_scorer.py (``AestheticScorer(dtype)``, ``__call__(images) -> scores[N]``): CLIP ViT-L/14
``get_image_features`` on CLIPProcessor pixels, ``embed / ||embed||``, then the MLP 768 -> 1024 -> 128 -> 64 -> 16 -> 1.
Differences that come with the platform:
  * images are a device tensor [N,3,H,W]: f32 / bf16 in [0,1] (quantised on the device as (x*255).round().clamp(0,255) in that
    dtype, rewards.py:43) or uint8; the Pillow-exact CLIPProcessor resize runs on the device (preprocess.clip_patches), which
    needs square images (a non-square image raises ValueError);
  * weights come from state dicts or a built tower (no checkpoint download): ``model_sd`` + ``clip_cfg`` (hub.load_clip,
    ClipConfig.vit_l14()) or ``model``, a vit.CLIPModel / vit_x3.CLIPModelX3, and ``head_sd`` (hub.load_aesthetic_head);
  * ``dtype`` selects the arithmetic as in PickScoreScorer: ``torch.float32`` (the reference's and the reward factory's) runs the
    fp32-equivalent tower of vit_x3.py, ``torch.bfloat16`` the bf16 tower of vit.py; ``compute_dtype`` says which ("bf16x3" or
    "bf16").  The normalisation and the MLP are one f32 kernel launch either way (advgrpo_aesthetic_head).
Scores stay on the device; nothing synchronises.
"""
import torch

from . import _lib, preprocess, vit, vit_x3
from .synthetic import AESTHETIC_HEAD_DIMS, AESTHETIC_HEAD_LAYERS


def aesthetic_head(embeds, head):
    """embeds f32 / bf16 [N, 768] (device) -> f32 [N]: L2 normalisation + the five Linears in one launch.  ``head``: the state dict
    moved to the device (f32, contiguous), as AestheticScorer keeps it."""
    lib = _lib.load()
    N, D = embeds.shape
    if D != AESTHETIC_HEAD_DIMS[0]:
        raise ValueError(f"aesthetic_head: embeddings of width {D}; the head reads {AESTHETIC_HEAD_DIMS[0]}")
    embeds = embeds.contiguous()
    out = torch.empty(N, dtype=torch.float32, device=embeds.device)
    wb = []
    for i, (fi, fo) in zip(AESTHETIC_HEAD_LAYERS, zip(AESTHETIC_HEAD_DIMS[:-1], AESTHETIC_HEAD_DIMS[1:])):
        w, b = head[f"layers.{i}.weight"], head[f"layers.{i}.bias"]
        if tuple(w.shape) != (fo, fi) or tuple(b.shape) != (fo,) or w.dtype != torch.float32 or b.dtype != torch.float32:
            raise ValueError(f"aesthetic_head: layers.{i} must be f32 [{fo}, {fi}] + [{fo}]")
        wb += [_lib.ptr(w), _lib.ptr(b)]
    _lib.check(lib.advgrpo_aesthetic_head(embeds.data_ptr(), _lib.dtype_code(embeds.dtype), N, *wb, out.data_ptr(), _lib.stream_ptr()))
    return out


class AestheticScorer(torch.nn.Module):
    def __init__(self, dtype=torch.float32, device="cuda", model_sd=None, clip_cfg=None, head_sd=None, model=None):
        super().__init__()
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"AestheticScorer: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        if head_sd is None or (model is None and (model_sd is None or clip_cfg is None)):
            raise RuntimeError("AestheticScorer needs head_sd and model_sd + clip_cfg (or a built tower) (no checkpoint download)")
        tower = vit_x3.CLIPModelX3 if dtype == torch.float32 else vit.CLIPModel
        if model is None:
            model = tower(model_sd, clip_cfg, device)
        elif not isinstance(model, tower):
            raise ValueError(f"AestheticScorer(dtype={dtype}) runs on a {tower.__name__}, got a {type(model).__name__}")
        if model.cfg.proj != AESTHETIC_HEAD_DIMS[0]:
            raise ValueError(f"AestheticScorer: the tower projects to {model.cfg.proj}; the aesthetic head reads {AESTHETIC_HEAD_DIMS[0]}")
        self.model, self.dtype = model, dtype
        self.device = model.device
        self.compute_dtype = "bf16x3" if dtype == torch.float32 else "bf16"
        self.head = {k: v.to(device=self.device, dtype=torch.float32).contiguous() for k, v in head_sd.items()}

    @torch.no_grad()
    def __call__(self, images):
        """images: device tensor [N,3,H,W], square; f32 / bf16 in [0,1] or uint8."""
        if images.shape[-1] != images.shape[-2]:
            raise ValueError(f"aesthetic: images must be square (the Pillow-exact resize writes size x size), got "
                             f"{tuple(images.shape[-2:])}")
        images = images.to(self.device)
        if images.dtype == torch.uint8:
            images = images.float() / 255.0        # re-quantised exactly by the kernel's (x*255).round()
        elif images.dtype not in (torch.float32, torch.bfloat16):
            images = (images * 255).round().clamp(0, 255).float() / 255.0      # rewards.py:43 in the tensor's own dtype
        size = self.model.cfg.image_size
        if self.dtype == torch.float32:
            embeds = self.model.get_image_features(pixel_patches3=preprocess.clip_patches(images, size, x3=True))
        else:
            embeds = self.model.get_image_features(pixel_patches=preprocess.clip_patches(images, size))
        return aesthetic_head(embeds, self.head)
