#!/usr/bin/env python3
"""Reference images with Qwen-Image on the gfx950 kernels: the contract of the reference's qwen_generate.py.

    python scripts/qwen_generate.py PROMPTS.txt --out DIR [--weights SNAPSHOT] [--devices N] [--batch 4] [--steps 50]
                                    [--size 512] [--scale 4.0] [--seed 42]

PROMPTS.txt holds one prompt per line (blank lines skipped).  DIR receives ``rank{r}_{i:05d}.png`` and ``prompt2img.json``
({prompt: file name}), what ``config.json_path`` / ``config.reference_image_path`` of the trainers point to
(adv_grpo_amd/reference_images.py).  All-ASCII prompts get ", Ultra HD, 4K, cinematic composition.", the others the Chinese
suffix; the negative prompt is " "; a prompt whose file exists is recorded and skipped, so an interrupted run resumes.

--weights SNAPSHOT   a local Qwen/Qwen-Image snapshot (transformer/, vae/, text_encoder/, scheduler/, tokenizer/), read through
                     adv_grpo_amd.hub; the tokenizer needs `transformers`.  Without it: seeded synthetic weights at a small
                     configuration (2 transformer blocks, 2 text layers) and a byte-level stand-in tokenizer -- the images are noise,
                     the path and the files are real.
--devices N          N fresh child processes (multiprocessing "spawn"), one GPU each, at most 8; the prompts are split the way
                     numpy.array_split does.  This parent process never opens a GPU.
"""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class ByteTokenizer:
    """Stand-in for the synthetic mode (no tokenizer files exist without a snapshot): 34 template ids, the user text's UTF-8 bytes,
    5 closing ids; right-padded with 0.  Same call signature and outputs as the Hugging Face tokenizer the sampler expects."""

    def __init__(self, vocab):
        self.vocab = vocab

    def __call__(self, texts, max_length=None, **kw):
        import torch
        rows = []
        for t in texts:
            user = t.split("<|im_start|>user\n", 1)[-1].split("<|im_end|>", 1)[0]
            ids = list(range(1, 35)) + [40 + b % (self.vocab - 40) for b in user.encode("utf-8")] + list(range(35, 40))
            rows.append(ids[:max_length] if max_length else ids)
        L = max(len(r) for r in rows)
        ids = torch.zeros(len(rows), L, dtype=torch.long)
        mask = torch.zeros(len(rows), L, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return type("Encoding", (), {"input_ids": ids, "attention_mask": mask})()


def build_sampler(weights, device):
    import torch
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import QwenMMDiTConfig, QwenTextConfig, QwenVaeConfig
    from adv_grpo_amd.qwen_generate import QwenImageSampler
    from adv_grpo_amd.qwen_mmdit import QwenImageTransformer2DModel
    from adv_grpo_amd.qwen_text_encoder import Qwen25VLTextEncoder
    from adv_grpo_amd.qwen_vae import AutoencoderKLQwenImageDecoder
    from adv_grpo_amd.scheduler import QwenImageFlowMatchScheduler
    if weights:
        from adv_grpo_amd import hub
        snap = hub.load_pipeline(weights, text_encoders=True)
        if snap["kind"] != "qwen":
            raise SystemExit(f"--weights {weights} holds a {snap['kind']} pipeline, not Qwen-Image")
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(os.path.join(weights, "tokenizer"), local_files_only=True)
        (tw, mcfg), (vw, vcfg), (xw, tcfg), sched = snap["transformer"], snap["vae"], snap["text_encoder"], snap["scheduler"]
        attention = "fused"                                          # prompts of up to 1024 tokens
    else:
        mcfg, vcfg, tcfg, sched = QwenMMDiTConfig(num_layers=2), QwenVaeConfig(), QwenTextConfig(vocab_size=2000, num_layers=2), {}
        with synthetic.on_device(device):
            tw = synthetic.qwen_mmdit_weights(mcfg, 4242, dtype=torch.bfloat16)
            vw = synthetic.qwen_vae_decoder_weights(vcfg, 2468, dtype=torch.bfloat16)
            xw = synthetic.qwen_text_weights(tcfg, 1357, dtype=torch.bfloat16)
        tokenizer, attention = ByteTokenizer(tcfg.vocab_size), "materialised"
    enc = Qwen25VLTextEncoder(xw, tcfg, device, attention=attention)
    tr = QwenImageTransformer2DModel(tw, mcfg, device)
    vae = AutoencoderKLQwenImageDecoder(vw, vcfg, device)
    return QwenImageSampler(enc, tr, vae, QwenImageFlowMatchScheduler(**sched), tokenizer=tokenizer)


def worker(rank, prompts, opt, queue):
    """One child process = one GPU: everything that touches the device happens here."""
    try:
        import torch
        from adv_grpo_amd import qwen_generate as Q
        device = torch.device(f"cuda:{rank}")
        torch.cuda.set_device(device)
        sampler = build_sampler(opt["weights"], device)
        calls = [0]

        def generate(final_prompts):
            calls[0] += 1
            return sampler(list(final_prompts), neg_input_ids=[Q.NEGATIVE_PROMPT], height=opt["size"], width=opt["size"],
                           num_inference_steps=opt["steps"], true_cfg_scale=opt["scale"], seed=opt["seed"] + 1000 * rank + calls[0],
                           output_type="pil")
        local = Q.generate_rank(generate, prompts, rank, opt["out"], batch_size=opt["batch"], log=print)
        torch.cuda.synchronize()
        queue.put((rank, local, None))
    except BaseException as e:                                       # the parent reports it and exits non-zero
        import traceback
        queue.put((rank, {}, traceback.format_exc() or repr(e)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("prompts", help="text file, one prompt per line")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--weights", default=None, help="local Qwen-Image snapshot; default: seeded synthetic weights at a small config")
    ap.add_argument("--devices", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args()
    if not 1 <= a.devices <= 8:
        raise SystemExit("--devices must be between 1 and 8")
    from adv_grpo_amd import qwen_generate as Q
    prompts = Q.read_prompts(a.prompts)
    os.makedirs(a.out, exist_ok=True)
    opt = dict(weights=a.weights, out=a.out, batch=a.batch, steps=a.steps, size=a.size, scale=a.scale, seed=a.seed)
    ctx = multiprocessing.get_context("spawn")
    queue = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, part, opt, queue)) for r, part in enumerate(Q.split_prompts(prompts, a.devices))]
    for p in procs:
        p.start()
    results, failed = {}, None
    while len(results) < len(procs) and failed is None:
        try:
            rank, local, err = queue.get(timeout=5)
        except Exception:                                            # queue.Empty: is everyone still there?
            dead = [r for r, p in enumerate(procs) if not p.is_alive() and p.exitcode not in (0, None) and r not in results]
            if dead:
                failed = f"rank {dead[0]} ended with status {procs[dead[0]].exitcode}"
            continue
        if err:
            failed = f"rank {rank}:\n{err}"
        results[rank] = local
    if failed:                                                       # nothing more is started; the others are told to stop
        for p in procs:
            if p.is_alive():
                p.terminate()
    for p in procs:
        p.join()
    if failed:
        raise SystemExit(f"qwen_generate: {failed}")
    path = Q.write_json(a.out, Q.merge_maps([results[r] for r in sorted(results)]))
    print(f"{len(prompts)} prompts, {a.devices} device(s): {path}")


if __name__ == "__main__":
    main()
