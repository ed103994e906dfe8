"""CPU: what the twelve SDE step entries refuse, the exact text of each refusal, and the two workspace queries.

Every argument check of these entries runs on the host before anything is launched, and the library loads without a device, so the
"pointers" below are small aligned integers that are never dereferenced: EVERY call in this file is refused.  The return code must be
-1 (an argument check; a launch that failed would be -2) and advgrpo_last_error() must be the literal recorded here.  The texts were
recorded from the library as it was before the entries were put on one call block and one check path; the copies of the checks
differ from entry to entry and each entry keeps its own:
  - the dtype and B / n checks of the plain and fan-out entries say "sde_step:" under every one of the eight entries,
  - only the rescaled entries refuse a bad prev_dtype / out_cast_dtype, bound B by 65535 and look at sigma_stride,
  - the fan-out entries check P, G before the common checks, which then report P as "B=",
  - *_bwd_kl requires mean_ref; under *_rescaled_bwd a NULL mean_ref selects the policy-only backward.

Left out because the call reaches a launch: nothing from the list this file was written to.  Not refusals at all, so not here: a NULL
mean_ref under the rescaled backward, and a NULL kl_out / workspace there while mean_ref is NULL too."""
import pytest

from adv_grpo_amd import _lib

P = 0x10000          # a 16-byte aligned non-null "pointer"; never dereferenced
BF16, F32 = _lib.BF16, _lib.F32
EPS, PHILOX, REPLAY = _lib.SDE_EPS, _lib.SDE_PHILOX, _lib.SDE_REPLAY
BAD = 7              # no dtype code

HEAD = ["v_uncond", "v_text", "v_dtype", "guidance", "x", "x_dtype", "sigma", "sigma_prev", "sigma_stride", "level"]
FWD = ["mode", "eps", "seed", "offset", "prev_sample", "prev_dtype", "out_next", "out_cast", "out_cast_dtype", "out_mean", "out_log_prob",
       "out_std", "workspace"]
BWD = ["prev_sample", "prev_dtype", "grad_log_prob", "grad_v_uncond", "grad_v_text"]
BWD_KL = ["prev_sample", "prev_dtype", "grad_log_prob", "mean_ref", "kl_weight", "grad_v_uncond", "grad_v_text", "kl_out", "workspace"]
FLAT, FAN, TOKENS = ["B", "n"], ["P", "G", "n"], ["B", "C", "H", "W", "patch"]

# arguments that would pass every check (so no test may send them unchanged): PHILOX mode, CFG, bf16 predictions on an f32 sample
ARGS = dict(v_uncond=P, v_text=P, v_dtype=BF16, guidance=4.5, x=P, x_dtype=F32, sigma=P, sigma_prev=P, sigma_stride=0, level=0.7, sigma_max=P,
            mode=PHILOX, eps=None, seed=1, offset=0, prev_sample=None, prev_dtype=0, out_next=P, out_cast=None, out_cast_dtype=0, out_mean=P,
            out_log_prob=P, out_std=P, workspace=P, grad_log_prob=P, mean_ref=P, kl_weight=0.5, grad_v_uncond=P, grad_v_text=P, kl_out=P,
            B=2, n=16, P=2, G=3, C=16, H=4, W=8, patch=2)
BWD_ARGS = dict(prev_sample=P, prev_dtype=F32)

# entry -> (the name its own texts carry, argument order without the trailing stream, is it a Flow-SDE entry)
ENTRIES = {}
for _flow in (False, True):
    _pre, _head = ("flow_", HEAD + ["sigma_max"]) if _flow else ("", HEAD)
    for _suffix, _tail in (("", FWD + FLAT), ("_branch", FWD + FAN), ("_bwd", BWD + FLAT), ("_bwd_kl", BWD_KL + FLAT),
                           ("_rescaled", FWD + TOKENS), ("_rescaled_bwd", BWD_KL + TOKENS)):
        ENTRIES[f"{_pre}sde_step{_suffix}"] = (_head + _tail, _flow)
FORWARDS = [e for e in ENTRIES if "bwd" not in e]
BACKWARDS = [e for e in ENTRIES if "bwd" in e]
RESCALED = [e for e in ENTRIES if "rescaled" in e]
FLAT_OR_FAN = [e for e in ENTRIES if "rescaled" not in e]
FANS = [e for e in ENTRIES if "branch" in e]
FLOWS = [e for e in ENTRIES if e.startswith("flow_")]


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _call(lib, entry, **over):
    assert over, "every call in this file must be refused: the unchanged arguments would reach a launch"
    order, _ = ENTRIES[entry]
    a = dict(ARGS, **(BWD_ARGS if "bwd" in entry else {}))
    a.update(over)
    return getattr(lib, "advgrpo_" + entry)(*[a[k] for k in order], None)


def _refused(lib, entry, text, **over):
    rc = _call(lib, entry, **over)
    assert rc == -1, (entry, over, rc, lib.advgrpo_last_error())
    assert lib.advgrpo_last_error().decode() == text, (entry, over)


def _who(entry):
    """The prefix of the dtype and B / n checks: the rescaled entries say their own name, the other eight all say sde_step."""
    return entry if "rescaled" in entry else "sde_step"


def _null_list(entry):
    if "bwd" not in entry:
        return ["v_uncond", "x", "sigma", "sigma_prev", "out_log_prob", "workspace"]
    base = ["v_uncond", "x", "sigma", "sigma_prev", "prev_sample", "grad_log_prob", "grad_v_uncond"]
    if entry.endswith("rescaled_bwd"):
        return base + ["kl_out", "workspace"]            # (with mean_ref set; a NULL mean_ref is the policy-only backward, no refusal)
    return base + (["mean_ref", "kl_out", "workspace"] if entry.endswith("bwd_kl") else [])


# ----------------------------------------------------------------------------------------------------------------------- all twelve entries
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_bad_dtypes(lib, entry):
    _refused(lib, entry, f"{_who(entry)}: bad v_dtype 7", v_dtype=BAD)
    _refused(lib, entry, f"{_who(entry)}: bad x_dtype 7", x_dtype=BAD)
    _refused(lib, entry, f"{_who(entry)}: bad v_dtype -1", v_dtype=-1)
    _refused(lib, entry, f"{_who(entry)}: bad v_dtype 7", v_dtype=BAD, x_dtype=BAD)                    # order: v before x
    _refused(lib, entry, f"{_who(entry)}: bad x_dtype 2", x_dtype=_lib.F64, v_uncond=None, mode=3)     # order: dtypes before pointers


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_arguments_one_at_a_time(lib, entry):
    for name in _null_list(entry):
        _refused(lib, entry, f"{entry}: null argument", **{name: None})
    # order: the null list before sigma_max, the mode (forwards) and grad_v_text (backwards)
    _refused(lib, entry, f"{entry}: null argument", sigma=None, sigma_max=None, mode=3, grad_v_text=None)


@pytest.mark.parametrize("entry", FLOWS)
def test_flow_entries_need_sigma_max(lib, entry):
    _refused(lib, entry, f"{entry}: null sigma_max", sigma_max=None)
    # order: before the mode checks (forwards), prev_dtype (rescaled backward) and grad_v_text (backwards)
    _refused(lib, entry, f"{entry}: null sigma_max", sigma_max=None, mode=-1, prev_dtype=BAD, grad_v_text=None)


# ---------------------------------------------------------------------------------------------------------------------------- the forwards
@pytest.mark.parametrize("entry", FORWARDS)
def test_forward_mode_checks(lib, entry):
    _refused(lib, entry, f"{entry}: bad mode 3", mode=3)
    _refused(lib, entry, f"{entry}: bad mode -1", mode=-1)
    _refused(lib, entry, f"{entry}: mode EPS needs eps", mode=EPS, eps=None)
    _refused(lib, entry, f"{entry}: mode REPLAY needs prev_sample", mode=REPLAY, prev_sample=None)
    _refused(lib, entry, f"{entry}: bad mode 3", mode=3, eps=None, prev_sample=None, prev_dtype=BAD)   # order: the range first
    _refused(lib, entry, f"{entry}: mode REPLAY needs prev_sample", mode=REPLAY, prev_sample=None, prev_dtype=BAD, out_cast=P,
             out_cast_dtype=BAD, v_uncond=P + 2)            # order: before the rescaled entries' dtype and alignment checks


# --------------------------------------------------------------------------------------------------------------------------- the backwards
@pytest.mark.parametrize("entry", BACKWARDS)
def test_backward_cfg_needs_grad_v_text(lib, entry):
    _refused(lib, entry, f"{entry}: CFG needs grad_v_text", grad_v_text=None)
    _refused(lib, entry, f"{entry}: CFG needs grad_v_text", grad_v_text=None, x=P + 4)     # order: before the rescaled alignment check


# ----------------------------------------------------------------------------------------------------------------- plain and fan-out shapes
@pytest.mark.parametrize("entry", FLAT_OR_FAN)
def test_flat_shape(lib, entry):
    fan = "branch" in entry
    _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=2 n=12)", n=12)
    _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=2 n=0)", n=0)
    _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=3 n=12)", n=12, B=3, P=3)              # fan-out: P is reported as B
    _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=2 n=12)", n=12, x=None, mode=3)         # order: before the pointers
    if not fan:
        _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=0 n=16)", B=0)
        _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=-1 n=16)", B=-1)


@pytest.mark.parametrize("entry", FANS)
def test_fan_out_shape(lib, entry):
    _refused(lib, entry, f"{entry}: need P>0 and G>0 (P=0 G=3)", P=0)
    _refused(lib, entry, f"{entry}: need P>0 and G>0 (P=2 G=0)", G=0)
    _refused(lib, entry, f"{entry}: P=65536 G=3 too large", P=65536)
    _refused(lib, entry, f"{entry}: P=65535 G=32769 too large", P=65535, G=32769)                     # P * G > INT32_MAX
    _refused(lib, entry, f"{entry}: need P>0 and G>0 (P=0 G=3)", P=0, v_dtype=BAD, n=12)              # order: P, G first of all
    _refused(lib, entry, "sde_step: need B>0 and n % 8 == 0 (B=65536 n=12)", P=65536, n=12)           # ... then the common checks
    _refused(lib, entry, f"{entry}: P=65536 G=3 too large", P=65536, v_uncond=None)                    # ... then the size, then pointers


# ---------------------------------------------------------------------------------------------------------------------- the rescaled entries
@pytest.mark.parametrize("entry", RESCALED)
def test_rescaled_shape(lib, entry):
    _refused(lib, entry, f"{entry}: built for patch 2 and C = 16 (patch=1 C=16)", patch=1)
    _refused(lib, entry, f"{entry}: built for patch 2 and C = 16 (patch=2 C=8)", C=8)
    _refused(lib, entry, f"{entry}: need 0 < B <= 65535 and even H, W (B=2 H=5 W=8)", H=5)
    _refused(lib, entry, f"{entry}: need 0 < B <= 65535 and even H, W (B=2 H=4 W=7)", W=7)
    _refused(lib, entry, f"{entry}: need 0 < B <= 65535 and even H, W (B=65536 H=4 W=8)", B=65536)
    _refused(lib, entry, f"{entry}: need 0 < B <= 65535 and even H, W (B=0 H=4 W=8)", B=0)
    _refused(lib, entry, f"{entry}: need 0 < B <= 65535 and even H, W (B=2 H=4 W=8)", sigma_stride=-1)
    _refused(lib, entry, f"{entry}: too many tokens", B=65535, H=2898, W=2898)       # 32807 blocks of 64 tokens > INT32_MAX / 65535
    _refused(lib, entry, f"{entry}: built for patch 2 and C = 16 (patch=1 C=16)", patch=1, B=65536, x=None)        # order
    _refused(lib, entry, f"{entry}: need 0 < B <= 65535 and even H, W (B=65536 H=2898 W=2898)", B=65536, H=2898, W=2898, sigma=None)
    _refused(lib, entry, f"{entry}: too many tokens", B=65535, H=2898, W=2898, v_uncond=None)


@pytest.mark.parametrize("entry", RESCALED)
def test_rescaled_replay_and_cast_dtypes(lib, entry):
    if "bwd" in entry:
        _refused(lib, entry, f"{entry}: bad prev_dtype 7", prev_dtype=BAD)
        _refused(lib, entry, f"{entry}: bad prev_dtype 7", prev_dtype=BAD, grad_v_text=None, x=P + 4)          # order
        return
    _refused(lib, entry, f"{entry}: bad prev_dtype 7", mode=REPLAY, prev_sample=P, prev_dtype=BAD)
    _refused(lib, entry, f"{entry}: bad out_cast_dtype 7", out_cast=P, out_cast_dtype=BAD)
    _refused(lib, entry, f"{entry}: bad out_cast_dtype 7", mode=EPS, eps=P, out_cast=P, out_cast_dtype=BAD)
    _refused(lib, entry, f"{entry}: bad prev_dtype 7", mode=REPLAY, prev_sample=P, prev_dtype=BAD, x=P + 4)     # order: before alignment
    _refused(lib, entry, f"{entry}: bad out_cast_dtype 7", out_cast=P, out_cast_dtype=BAD, x=P + 4)


@pytest.mark.parametrize("entry", RESCALED)
def test_rescaled_alignment(lib, entry):
    """Each tensor the kernel reads or writes two elements at a time, off by one of its elements."""
    text = f"{entry}: tensors must be aligned to two of their elements"
    _refused(lib, entry, text, v_uncond=P + 2)
    _refused(lib, entry, text, v_text=P + 2)
    _refused(lib, entry, text, v_uncond=P + 4, v_dtype=F32)
    _refused(lib, entry, text, x=P + 4)
    _refused(lib, entry, text, x=P + 2, x_dtype=BF16)
    if "bwd" in entry:
        _refused(lib, entry, text, prev_sample=P + 4)
        _refused(lib, entry, text, prev_sample=P + 2, prev_dtype=BF16)
        _refused(lib, entry, text, mean_ref=P + 4)
        _refused(lib, entry, text, grad_v_uncond=P + 2)
        _refused(lib, entry, text, grad_v_text=P + 2)
    else:
        _refused(lib, entry, text, mode=EPS, eps=P + 4)
        _refused(lib, entry, text, mode=REPLAY, prev_sample=P + 2, prev_dtype=BF16)
        _refused(lib, entry, text, out_next=P + 4)
        _refused(lib, entry, text, out_cast=P + 2, out_cast_dtype=BF16)
        _refused(lib, entry, text, out_mean=P + 4)


# ---------------------------------------------------------------------------------------------------------------------- workspace queries
def test_workspace_queries(lib):
    flat = lib.advgrpo_sde_step_workspace_bytes
    assert flat(3, 8) == 3 * 1 * 4 and flat(3, 2048) == 3 * 1 * 4           # one block of 2048 elements per sample
    assert flat(3, 2048 + 8) == 3 * 2 * 4
    assert flat(3, 64 * 2048 + 8) == 3 * 64 * 4                             # 65 chunks: the cap of 64 blocks per sample
    tok = lib.advgrpo_sde_step_rescaled_workspace_bytes                     # one float per block of 64 tokens per sample
    assert tok(2, 16, 4, 6, 2) == 2 * 1 * 4
    assert tok(1, 16, 18, 16, 2) == 1 * 2 * 4                               # 72 tokens: a second block
    assert tok(3, 16, 64, 64, 2) == 3 * 16 * 4
    assert tok(0, 16, 4, 6, 2) == 0 and tok(-1, 16, 4, 6, 2) == 0 and tok(2, 16, 0, 6, 2) == 0
