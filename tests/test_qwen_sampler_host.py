"""CPU: the host side of Qwen-Image sampling -- the dynamic-shift sigma table, the restatement of the true-CFG Euler step
(tests/qwen_sampler_reference.py), the share of tokens whose bf16 norm depends on the summation order on the GPU test's own inputs,
the file / resume / json logic of scripts/qwen_generate.py under a fake sampler, and the binding's refusal of a missing symbol."""
import json
import os

import numpy as np
import pytest
import torch

import qwen_sampler_reference as R

bf16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("n,n_img", [(4, 16), (50, 1024), (50, 4096), (28, 256), (2, 1024)])
def test_schedule_properties(n, n_img):
    from adv_grpo_amd.scheduler import QwenImageFlowMatchScheduler
    sch = QwenImageFlowMatchScheduler()
    ts = sch.set_timesteps(n, n_img)
    sig = sch.sigmas.numpy()
    assert sig.dtype == np.float32 and sig.shape == (n + 1,) and ts.shape == (n,)
    assert np.all(np.diff(sig.astype(np.float64)) < 0)
    assert sig[0] == np.float32(1.0) and sig[n] == 0.0
    if n > 1:
        assert sig[n - 1] == np.float32(0.02)
    assert np.array_equal(ts.numpy(), np.float32(1000.0) * sig[:-1])
    # the f32 table against the float64 restatement: within one f32 ulp, element by element
    ref, ref_ts = R.schedule_f64(n, n_img)
    ref = np.asarray(ref)
    assert np.all(np.abs(sig.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    assert np.array_equal(sig, R.schedule(n, n_img)[0])


def test_mu_is_linear_in_the_token_count():
    from adv_grpo_amd.scheduler import QwenImageFlowMatchScheduler, calculate_shift
    sch = QwenImageFlowMatchScheduler()
    assert sch.mu(1024) == pytest.approx(0.5 + 0.4 * 768 / 7936, rel=1e-14)
    assert sch.mu(256) == pytest.approx(0.5, rel=1e-14) and sch.mu(8192) == pytest.approx(0.9, rel=1e-14)
    assert calculate_shift(1024) == pytest.approx(R.calculate_shift(1024), rel=1e-15)
    assert sch.mu(2048) - sch.mu(1024) == pytest.approx(sch.mu(3072) - sch.mu(2048), rel=1e-12)


def test_tables_are_built_once_and_the_sd3_class_is_untouched():
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler, QwenImageFlowMatchScheduler
    sch = QwenImageFlowMatchScheduler()
    sch.set_timesteps(50, 1024)
    a = sch.sigmas
    sch.set_timesteps(50, 4096)
    assert sch.sigmas is not a and not torch.equal(sch.sigmas, a)        # the table depends on the image size
    sch.set_timesteps(50, 1024)
    assert sch.sigmas is a
    sd3 = FlowMatchEulerDiscreteScheduler()
    sd3.set_timesteps(10)
    assert sd3.sigmas.shape == (11,) and abs(float(sd3.sigmas[0]) - 1.0) < 1e-6 and sd3.shift == 3.0


def test_hub_reads_the_snapshots_scheduler_config(tmp_path):
    from adv_grpo_amd import hub
    from adv_grpo_amd.scheduler import QwenImageFlowMatchScheduler
    assert hub.load_qwen_scheduler(str(tmp_path)) == {}                     # no file: the published defaults
    cfg = {"_class_name": "FlowMatchEulerDiscreteScheduler", "base_image_seq_len": 256, "base_shift": 0.5, "invert_sigmas": False,
           "max_image_seq_len": 8192, "max_shift": 0.9, "num_train_timesteps": 1000, "shift": 1.0, "shift_terminal": 0.02,
           "stochastic_sampling": False, "time_shift_type": "exponential", "use_beta_sigmas": False, "use_dynamic_shifting": True,
           "use_exponential_sigmas": False, "use_karras_sigmas": False}
    (tmp_path / "scheduler_config.json").write_text(json.dumps(cfg))
    kw = hub.load_qwen_scheduler(str(tmp_path))
    assert kw == dict(num_train_timesteps=1000, base_image_seq_len=256, max_image_seq_len=8192, base_shift=0.5, max_shift=0.9, shift_terminal=0.02)
    a, b = QwenImageFlowMatchScheduler(**kw), QwenImageFlowMatchScheduler()
    assert np.array_equal(a.table(50, 1024)[0], b.table(50, 1024)[0])
    (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(cfg, max_shift=1.15, shift_terminal=0.05)))
    c = QwenImageFlowMatchScheduler(**hub.load_qwen_scheduler(str(tmp_path)))
    assert c.table(50, 1024)[0][49] == np.float32(0.05) and c.mu(8192) == pytest.approx(1.15)
    for bad in (dict(use_dynamic_shifting=False), dict(time_shift_type="linear"), dict(use_karras_sigmas=True)):
        (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(cfg, **bad)))
        with pytest.raises(hub.HubError):
            hub.load_qwen_scheduler(str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- step restatement
def _ulp_bf16(x):
    """Spacing of bf16 at |x| (f32 tensor)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().float().clamp_min(2.0 ** -126))) - 7)


@pytest.mark.parametrize("dtype", [bf16, torch.float32])
def test_equal_predictions_leave_the_positive_one(dtype):
    """pos == neg: comb == pos, the norms are equal, the ratio is exactly 1 and out == pos (at most the ratio's rounding away)."""
    g = torch.Generator().manual_seed(3)
    pos = R.pack(torch.randn(2, 16, 6, 10, generator=g).to(dtype))
    comb = R.combine(pos.clone(), pos)
    assert torch.equal(comb, pos)
    out = R.rescale(comb, pos)
    tol = _ulp_bf16(pos) if dtype == bf16 else pos.abs() * 2.0 ** -23
    assert ((out.float() - pos.float()).abs() <= tol).all()


@pytest.mark.parametrize("dtype", [bf16, torch.float32])
def test_scale_one_gives_the_positive_prediction(dtype):
    """neg + 1 * (pos - neg) == pos exactly wherever pos - neg is exact: neg within [pos / 2, 2 pos] (Sterbenz).  (For unrelated
    pos and neg the difference rounds and no floating-point format gives pos back exactly; the inputs respect that.)"""
    g = torch.Generator().manual_seed(4)
    pos = torch.randn(2, 16, 6, 10, generator=g).to(dtype)
    neg = (pos.float() * (0.5 + 1.5 * torch.rand(pos.shape, generator=g))).to(dtype)
    lo, hi = torch.minimum(pos / 2, pos * 2), torch.maximum(pos / 2, pos * 2)
    neg = torch.maximum(torch.minimum(neg, hi), lo)
    assert torch.equal(R.combine(neg, pos, 1.0), pos)
    sample = torch.randn(2, 16, 6, 10, generator=g).to(dtype)
    s0, s1 = torch.tensor(0.9), torch.tensor(0.8)
    # ... and then the rescale's ratio is 1: the CFG step is the plain Euler step on pos
    assert torch.equal(R.cfg_euler_step(neg, pos, sample, s0, s1, 1.0), R.cfg_euler_step(pos, None, sample, s0, s1))


def test_restatement_tracks_its_float64_form():
    g = torch.Generator().manual_seed(5)
    neg, pos, x = (torch.randn(2, 16, 8, 8, generator=g) for _ in range(3))
    s0, s1 = torch.tensor(0.7), torch.tensor(0.65)
    ref = R.cfg_euler_step_f64(neg, pos, x, s0, s1)
    assert (R.cfg_euler_step(neg, pos, x, s0, s1).double() - ref).abs().max().item() < 1e-5
    got = R.cfg_euler_step(neg.to(bf16), pos.to(bf16), x.to(bf16), s0, s1).double()
    ref = R.cfg_euler_step_f64(neg.to(bf16), pos.to(bf16), x.to(bf16), s0, s1)
    assert (got - ref).abs().max().item() < 0.05 and ((got - ref).norm() / ref.norm()).item() < 4e-3
    assert torch.equal(R.unpack(R.pack(x), 16, 8, 8), x) and R.pack(x).shape == (2, 16, 64)
    assert torch.equal(R.pack(x)[0, 5].view(16, 2, 2), x[0, :, 2:4, 2:4])           # token (1, 1): c, py, px


def test_norm_rounding_depends_on_summation_order_in_under_one_percent_of_tokens():
    """The GPU test lets <= 1 % of tokens differ from the restatement because the kernel adds a token's 64 squares in another order
    than torch.norm.  On every bf16 input of that test: the share of tokens whose bf16 norm (of pos, and of comb) rounds differently
    between torch's f32 accumulation and the exact (float64) sum stays under that cap."""
    worst = 0.0
    for name, shape, vd, xd, mult, seed in R.cases():
        if vd != bf16:
            continue
        neg, pos, _ = R.make_inputs(shape, vd, xd, mult, seed)
        neg, pos = R.pack(neg), R.pack(pos)
        share = R.token_norm_mismatch_share(pos) + R.token_norm_mismatch_share(R.combine(neg, pos))
        print(f"{name}: tokens {pos.shape[0] * pos.shape[1]} norm mismatch share {share:.5f}")
        worst = max(worst, share)
        assert share <= R.MISMATCH_CAP, (name, share)
    print(f"worst share {worst:.5f} (cap {R.MISMATCH_CAP})")


# ---------------------------------------------------------------------------------------------------------------- tool logic
class _FakeImage:
    def __init__(self, prompt):
        self.prompt = prompt

    def save(self, path):
        with open(path, "w", encoding="utf-8") as f:
            f.write(self.prompt)


def test_names_suffixes_resume_and_merged_json(tmp_path):
    from adv_grpo_amd import qwen_generate as Q
    assert Q.image_name(0, 7) == "rank0_00007.png" and Q.image_name(3, 12345) == "rank3_12345.png"
    assert Q.final_prompt("a red cube") == "a red cube, Ultra HD, 4K, cinematic composition."
    assert Q.final_prompt("一只猫") == "一只猫, 超清，4K，电影级构图."
    assert Q.final_prompt("café") == "café, 超清，4K，电影级构图."                  # any non-ASCII character takes the second suffix
    assert Q.NEGATIVE_PROMPT == " "
    src = tmp_path / "prompts.txt"
    src.write_text("a red cube\n\n  一只猫  \nthree dogs\n   \nfour\nfive\n", encoding="utf-8")
    prompts = Q.read_prompts(str(src))
    assert prompts == ["a red cube", "一只猫", "three dogs", "four", "five"]
    parts = Q.split_prompts(prompts, 2)
    assert parts == [["a red cube", "一只猫", "three dogs"], ["four", "five"]]
    assert [len(p) for p in Q.split_prompts(list(range(10)), 4)] == [len(a) for a in np.array_split(np.arange(10), 4)]
    out = tmp_path / "out"
    calls = []

    def generate(ps):
        calls.append(list(ps))
        return [_FakeImage(p) for p in ps]
    os.makedirs(out)
    (out / "rank0_00001.png").write_text("kept")                           # an earlier run got this far
    maps = [Q.generate_rank(generate, part, r, str(out), batch_size=2) for r, part in enumerate(parts)]
    assert calls == [["a red cube, Ultra HD, 4K, cinematic composition."], ["three dogs, Ultra HD, 4K, cinematic composition."],
                     ["four, Ultra HD, 4K, cinematic composition.", "five, Ultra HD, 4K, cinematic composition."]]
    assert (out / "rank0_00001.png").read_text() == "kept"
    assert sorted(os.listdir(out)) == ["rank0_00000.png", "rank0_00001.png", "rank0_00002.png", "rank1_00000.png", "rank1_00001.png"]
    merged = Q.merge_maps(maps)
    # the reference's mapping: the ORIGINAL prompt (no suffix) -> the file its rank and index name
    assert merged == {"a red cube": "rank0_00000.png", "一只猫": "rank0_00001.png", "three dogs": "rank0_00002.png",
                      "four": "rank1_00000.png", "five": "rank1_00001.png"}
    path = Q.write_json(str(out), merged)
    assert os.path.basename(path) == "prompt2img.json"
    assert json.load(open(path, encoding="utf-8")) == merged and "一只猫" in open(path, encoding="utf-8").read()
    # a second run finds everything and never reaches the sampler
    calls.clear()
    again = [Q.generate_rank(generate, part, r, str(out), batch_size=2) for r, part in enumerate(parts)]
    assert calls == [] and Q.merge_maps(again) == merged
    with pytest.raises(RuntimeError):
        Q.generate_rank(lambda ps: [], ["x"], 5, str(out))


def test_reference_image_store_reads_the_tools_output(tmp_path):
    from PIL import Image
    from adv_grpo_amd import qwen_generate as Q
    from adv_grpo_amd.reference_images import ReferenceImageStore
    colours = {"a red cube, Ultra HD, 4K, cinematic composition.": (255, 0, 0), "一只猫, 超清，4K，电影级构图.": (0, 0, 255)}
    gen = lambda ps: [Image.new("RGB", (16, 16), colours[p]) for p in ps]
    m = Q.generate_rank(gen, ["a red cube", "一只猫"], 0, str(tmp_path))
    store = ReferenceImageStore(Q.write_json(str(tmp_path), m), str(tmp_path), resolution=16, device="cpu")
    img = store.get("一只猫")
    assert img.shape == (1, 3, 16, 16) and img[0, 2].min() == 1.0 and img[0, 0].max() == 0.0
    assert store.get("a red cube", n=1)[0, 0].min() == 1.0
    store.close()


def test_string_prompts_go_through_the_injected_tokenizer():
    from adv_grpo_amd import qwen_generate as Q
    seen = {}

    def tokenizer(txt, **kw):
        seen.update(txt=txt, kw=kw)
        return type("Tok", (), {"input_ids": torch.zeros(len(txt), 40, dtype=torch.long), "attention_mask": torch.ones(len(txt), 40, dtype=torch.long)})()
    ids, mask = Q.tokenize_prompts(tokenizer, ["a cat", " "])
    assert ids.shape == (2, 40) and mask.shape == (2, 40)
    assert seen["txt"][0].startswith("<|im_start|>system\nDescribe the image") and seen["txt"][0].endswith("<|im_start|>user\na cat<|im_end|>\n<|im_start|>assistant\n")
    assert seen["kw"] == dict(max_length=1024 + 34, padding=True, truncation=True, return_tensors="pt")
    with pytest.raises(RuntimeError, match="tokenizer"):
        Q.tokenize_prompts(None, ["a cat"])


# ---------------------------------------------------------------------------------------------------------------- binding
def test_binding_declares_the_step_and_refuses_a_missing_symbol(monkeypatch):
    from adv_grpo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    assert "advgrpo_qwen_cfg_euler_step" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "advgrpo_qwen_cfg_euler_step")
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "advgrpo_qwen_no_such_step", (_lib.c_int, []))
    with pytest.raises(AttributeError, match="advgrpo_qwen_no_such_step"):
        _lib.load()
    assert _lib._lib is None                                               # nothing half-loaded is kept


def test_tools_stand_in_tokenizer_keeps_the_template_contract():
    """scripts/qwen_generate.py without a snapshot: 34 template ids in front (what encode_prompt drops), the prompt's bytes, right padding."""
    import importlib.util
    from adv_grpo_amd import qwen_generate as Q
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("qwen_generate_tool", os.path.join(root, "scripts", "qwen_generate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ids, mask = Q.tokenize_prompts(tool.ByteTokenizer(2000), ["a cat", " ", "一只猫"])
    assert ids.shape == mask.shape == (3, 34 + 9 + 5)
    assert mask.sum(dim=1).tolist() == [34 + 5 + 5, 34 + 1 + 5, 34 + 9 + 5] and int(ids.max()) < 2000
    assert torch.equal(ids[:, :34], torch.arange(1, 35).expand(3, -1)) and (ids[mask == 0] == 0).all()
