"""CPU: what the GEMM, convolution and LayerNorm entries refuse, and the exact text of each refusal.

Every argument check of these entries runs on the host before anything is launched, and the library loads without a device, so the
"pointers" below are small integers that are never dereferenced: EVERY call in this file is refused.  The return code must be -1 (an
argument check; a launch that failed would be -2) and advgrpo_last_error() must be the literal recorded here.  The texts were recorded
from the library as it was before the entries' parameter blocks were built in one place; the three copies of the LayerNorm checks
differ from entry to entry (which pointers "null pointer" covers, where ldq < D is reported, the wording for a second output) and
each entry keeps its own.

Left out because the call reaches a launch: nothing from the list this file was written to; but note two refusals that carry another
check's text than one might expect -- advgrpo_conv3x3_nhwc with Cin % 64 != 0 is stopped by the GEMM's K % 64 check (K = 9 Cin), and
the flat advgrpo_layernorm_mod_fp8 reports ldq < D as a pitch that is no multiple of 8."""
import ctypes

import pytest

from adv_grpo_amd import _lib

P = 0x10000          # a 16-byte aligned non-null "pointer"; never dereferenced
BF16, F32 = _lib.BF16, _lib.F32


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _refused(lib, rc, text):
    assert rc == -1, (rc, lib.advgrpo_last_error())
    assert lib.advgrpo_last_error().decode() == text


# ------------------------------------------------------------------------------------------------------------------------ Linear entries
GEMM = dict(A=P, lda=64, W=P, ldw=64, C=P, ldc=128, out_dtype=BF16, M=16, N=128, K=64, bias=None, act=0, alpha=1.0, gate=None,
            gate_stride=0, gate_rows=0, residual=None, ldr=0)
TXT_NULL = "gemm: null operand"
TXT_K = "gemm: need M,N>0 and K % 64 == 0 (M=16 N=128 K=96)"
TXT_LD = "gemm: lda/ldw must be multiples of 8 elements (16 B rows)"
TXT_DT = "gemm: bad out dtype"
TXT_SPLITK = "gemm: split-K accumulates atomically into f32 and takes no other epilogue"
TXT_ACC = "gemm: accumulation into C is a plain f32 GEMM without other epilogue"
TXT_DACT = "gemm: d-activation epilogue needs aux_in"
TXT_AUX = "gemm: aux needs N, ld_aux % 4 == 0"
TXT_AUX_LDC = "gemm: aux / d-activation needs ldc % 4 == 0 (ldc=130)"
TXT_AUX_LDR = "gemm: aux / d-activation needs ldr % 4 == 0 (ldr=134)"
TXT_AUX_GATE = "gemm: aux / d-activation needs gate_stride % 4 == 0 (gate_stride=138)"
# aux_out / a d-activation on a pitch that would take the scalar form of the epilogue, which carries neither
AUX_PITCH = [(dict(aux_out=P, ld_aux=128, ldc=130), TXT_AUX_LDC), (dict(aux_in=P, ld_aux=128, act=5, ldc=130), TXT_AUX_LDC),
             (dict(aux_in=P, ld_aux=128, act=7, residual=P, ldr=134), TXT_AUX_LDR), (dict(aux_out=P, ld_aux=128, act=1, ldr=134), TXT_AUX_LDR),
             (dict(aux_in=P, ld_aux=128, act=6, gate=P, gate_stride=138, gate_rows=16), TXT_AUX_GATE),
             (dict(aux_out=P, ld_aux=128, ldc=130, ldr=134, gate_stride=138), TXT_AUX_LDC),          # the order of the three checks
             (dict(aux_out=P, ld_aux=126, ldc=130), TXT_AUX)]                                        # after the N / ld_aux check
TXT_RMS = "gemm: fused QK-norm needs a plain bf16 projection with N % 64 == 0 and 16-byte aligned rows"
COMMON = [(dict(A=None), TXT_NULL), (dict(W=None), TXT_NULL), (dict(C=None), TXT_NULL), (dict(K=96), TXT_K), (dict(lda=60), TXT_LD),
          (dict(ldw=60), TXT_LD)]


def _flat(lib, **over):
    a = dict(GEMM, **over)
    return lib.advgrpo_gemm_bf16(a["A"], a["lda"], a["W"], a["ldw"], a["C"], a["ldc"], a["out_dtype"], a["M"], a["N"], a["K"], a["bias"],
                                 a["act"], a["alpha"], a["gate"], a["gate_stride"], a["gate_rows"], a["residual"], a["ldr"],
                                 a.get("seg_rows", 0), 0, 0, 0, 0, 0, a.get("batch", 1), 0, 0, 0, None)


def _desc(**over):
    d = _lib.GemmDesc()
    for k, v in dict(GEMM, **over).items():
        setattr(d, k, v)
    return d


def _grouped(lib, *descs, count=None):
    arr = (_lib.GemmDesc * len(descs))(*descs)
    return lib.advgrpo_gemm_grouped(arr, len(descs) if count is None else count, None)


def _train(lib, **over):
    a = dict(GEMM, aux_out=None, aux_in=None, ld_aux=0, splitk=1)
    a.update(over)
    return lib.advgrpo_gemm_bf16_train(a["A"], a["lda"], a["W"], a["ldw"], a["C"], a["ldc"], a["out_dtype"], a["M"], a["N"], a["K"],
                                       a["bias"], a["act"], a["alpha"], a["gate"], a["gate_stride"], a["gate_rows"], a["residual"],
                                       a["ldr"], a["aux_out"], a["aux_in"], a["ld_aux"], a["splitk"], None)


def _acc(lib, **over):
    a = dict(GEMM, **over)
    return lib.advgrpo_gemm_bf16_acc_f32(a["A"], a["lda"], a["W"], a["ldw"], a["C"], a["ldc"], a["M"], a["N"], a["K"], a["alpha"], None)


@pytest.mark.parametrize("over,text", COMMON + [(dict(out_dtype=2), TXT_DT), (dict(act=5), TXT_DACT), (dict(act=7), TXT_DACT),
                                                (dict(batch=2, K=96), "gemm: need M,N>0 and K % 64 == 0 (M=16 N=128 K=96)")])
def test_gemm_bf16_refusals(lib, over, text):
    _refused(lib, _flat(lib, **over), text)


@pytest.mark.parametrize("over,text", COMMON + [
    (dict(out_dtype=2), TXT_DT), (dict(act=5), TXT_DACT), (dict(aux_out=P, ld_aux=128, N=126), TXT_AUX),
    (dict(aux_out=P, ld_aux=126), TXT_AUX), (dict(aux_in=P, ld_aux=128, act=5, N=126), TXT_AUX),
    (dict(rms_weight=P, rms_nheads=2, rms_heads_per_weight=1, gate=P, gate_stride=128, gate_rows=16), TXT_RMS),
    (dict(rms_weight=P, rms_nheads=2, rms_heads_per_weight=1, out_dtype=F32), TXT_RMS),
    (dict(rms_weight=P, rms_nheads=0, rms_heads_per_weight=1), TXT_RMS)] + AUX_PITCH)
def test_gemm_grouped_refusals(lib, over, text):
    _refused(lib, _grouped(lib, _desc(**over)), text)
    _refused(lib, _grouped(lib, _desc(**over), _desc()), text)          # as the first of a pair
    _refused(lib, _grouped(lib, _desc(), _desc(**over)), text)          # as the second: both are validated before the launch


def test_gemm_grouped_takes_one_or_two_descriptors(lib):
    d = _desc()
    for count in (0, 3):
        _refused(lib, _grouped(lib, d, d, d, count=count), "gemm_grouped: need 1 or 2 descriptors")
    _refused(lib, lib.advgrpo_gemm_grouped(None, 1, None), "gemm_grouped: need 1 or 2 descriptors")


def test_gemm_fp8_grouped_refusals(lib):
    sc = (_lib.Fp8Scales * 2)()
    sc[0].a_scale = sc[0].w_scale = sc[1].a_scale = sc[1].w_scale = P
    one = lambda d: lib.advgrpo_gemm_fp8_grouped((_lib.GemmDesc * 1)(d), sc, 1, None)
    _refused(lib, one(_desc(out_dtype=F32)), "gemm_fp8_grouped: bf16 output, no d-activation input")
    _refused(lib, one(_desc(aux_in=P, ld_aux=128, act=5)), "gemm_fp8_grouped: bf16 output, no d-activation input")
    two = (_lib.GemmDesc * 2)(_desc(), _desc(out_dtype=F32))
    _refused(lib, lib.advgrpo_gemm_fp8_grouped(two, sc, 2, None), "gemm_fp8_grouped: bf16 output, no d-activation input")
    _refused(lib, lib.advgrpo_gemm_fp8_grouped(two, None, 2, None), "gemm_fp8_grouped: need 1 or 2 descriptors with their scales")
    _refused(lib, lib.advgrpo_gemm_fp8_grouped(two, sc, 3, None), "gemm_fp8_grouped: need 1 or 2 descriptors with their scales")


@pytest.mark.parametrize("over,text", COMMON + [
    (dict(out_dtype=2), TXT_DT), (dict(splitk=2, out_dtype=F32, bias=P), TXT_SPLITK), (dict(splitk=2), TXT_SPLITK),
    (dict(splitk=2, out_dtype=F32, aux_out=P, ld_aux=128), TXT_SPLITK), (dict(act=5), TXT_DACT), (dict(act=6), TXT_DACT),
    (dict(aux_out=P, ld_aux=128, N=126), TXT_AUX), (dict(aux_in=P, ld_aux=130, act=5), TXT_AUX)] + AUX_PITCH)
def test_gemm_bf16_train_refusals(lib, over, text):
    _refused(lib, _train(lib, **over), text)


@pytest.mark.parametrize("over,text", COMMON)
def test_gemm_bf16_acc_f32_refusals(lib, over, text):
    _refused(lib, _acc(lib, **over), text)


# -------------------------------------------------------------------------------------------------------------------------- convolutions
def test_conv3x3_nhwc_refusals(lib):
    conv = lambda x=P, Cin=64, Cout=128: lib.advgrpo_conv3x3_nhwc(x, P, P, BF16, 1, 4, 4, Cin, Cout, 0, None, 0, None, P, None)
    _refused(lib, conv(Cin=32), "gemm: need M,N>0 and K % 64 == 0 (M=16 N=128 K=288)")     # (K = 9 Cin: the GEMM's check comes first)
    _refused(lib, conv(Cin=96, Cout=3), "gemm: need M,N>0 and K % 64 == 0 (M=16 N=3 K=864)")
    _refused(lib, conv(x=None), TXT_NULL)


def test_conv3x3_nhwc_x3_refusals(lib):
    conv = lambda Cin3, Cout: lib.advgrpo_conv3x3_nhwc_x3(P, P, P, 1, 4, 4, Cin3, Cout, 0, None, 0, None, P, None)
    for Cout in (3, 128):                                      # both routes out of the entry
        _refused(lib, conv(64, Cout), "conv3x3_x3: Cin3 must be 3 x (a multiple of 64) (Cin3=64)")
        _refused(lib, conv(96, Cout), "conv3x3_x3: Cin3 must be 3 x (a multiple of 64) (Cin3=96)")


@pytest.mark.parametrize("name", ["advgrpo_conv3x3_nhwc_f16x2", "advgrpo_conv3x3_nhwc_f16x1", "advgrpo_conv3x3_nhwc_bf16x2"])
def test_conv3x3_two_product_refusals(lib, name):
    fn = getattr(lib, name)
    conv = lambda x=P, Hout=4, Wout=4, Cin3=192, Cout=128, part=None: fn(x, P, P, 1, Hout, Wout, Cin3, Cout, 0, None, 0, None, P, 1.0, part, None)
    _refused(lib, conv(Cout=64), "conv3x3_f16x2: Cin3 must be 3 x (a multiple of 64), Cout >= 128 (Cin3=192 Cout=64)")
    _refused(lib, conv(Cin3=64), "conv3x3_f16x2: Cin3 must be 3 x (a multiple of 64), Cout >= 128 (Cin3=64 Cout=128)")
    _refused(lib, conv(x=None), "conv3x3_f16x2: null pointer")
    _refused(lib, conv(Hout=3, Wout=5, part=P), "conv3x3_f16x2: block sums need 16 | Hout Wout")
    _refused(lib, conv(Cout=130, part=P), "conv3x3_f16x2: block sums need 16 | Hout Wout")
    _refused(lib, conv(x=None, Hout=3, Wout=5, part=P), "conv3x3_f16x2: null pointer")           # the order of the checks


@pytest.mark.parametrize("name,who", [("advgrpo_conv3x3_nhwc_f16x2_pair", "conv3x3_f16x2_pair"), ("advgrpo_conv3x3_nhwc_f16x1_pair", "conv3x3_f16x1_pair")])
def test_conv3x3_pair_output_refusals(lib, name, who):
    fn = getattr(lib, name)
    conv = lambda out=P, x=P, Cin3=192, Cout=128: fn(x, P, out, 1.0, 1, 4, 4, Cin3, Cout, 0, None, 0, None, P, 1.0, None)
    _refused(lib, conv(out=None), who + ": null output")
    _refused(lib, conv(Cout=64), "conv3x3_f16x2: Cin3 must be 3 x (a multiple of 64), Cout >= 128 (Cin3=192 Cout=64)")
    _refused(lib, conv(Cout=130), "conv3x3_f16x2: pair output needs Cout % 4 == 0, 8-byte alignment and no block sums")
    _refused(lib, conv(out=P + 4), "conv3x3_f16x2: pair output needs Cout % 4 == 0, 8-byte alignment and no block sums")
    _refused(lib, conv(x=None), "conv3x3_f16x2: null pointer")


def test_conv3x3_s2_nhwc_x3_refusals(lib):
    conv = lambda x=P, B=1, Cin3=192, Cout=128: lib.advgrpo_conv3x3_s2_nhwc_x3(x, P, P, B, 4, 4, Cin3, Cout, None, P, None)
    _refused(lib, conv(Cout=130), "conv3x3_s2_x3: Cin3 must be 3 x (a multiple of 64), Cout >= 128 and a multiple of 4 (Cin3=192 Cout=130)")
    _refused(lib, conv(Cout=64), "conv3x3_s2_x3: Cin3 must be 3 x (a multiple of 64), Cout >= 128 and a multiple of 4 (Cin3=192 Cout=64)")
    _refused(lib, conv(Cin3=64), "conv3x3_s2_x3: Cin3 must be 3 x (a multiple of 64), Cout >= 128 and a multiple of 4 (Cin3=64 Cout=128)")
    _refused(lib, conv(x=None), "conv3x3_s2_x3: null pointer")
    _refused(lib, conv(B=0), "conv3x3_s2_x3: bad shape (B=0 Hout=4 Wout=4)")


# ----------------------------------------------------------------------------------------------------------------------------- LayerNorm
LN = dict(x=P, ldx=64, out0=P, out1=None, ldo=64, w=None, b=None, scale0=None, shift0=None, scale1=None, shift1=None, mod_stride=0,
          rows_per_batch=0, M=4, D=64, eps=1e-6)
LN8 = dict(LN, out0=None, q0=P, qs0=P, q1=None, qs1=None, ldq=64)
ORDER = ["x", "ldx", "out0", "out1", "ldo", "w", "b", "scale0", "shift0", "scale1", "shift1", "mod_stride", "rows_per_batch", "M", "D", "eps"]


def _ln(lib, **over):
    a = dict(LN, **over)
    return lib.advgrpo_layernorm_mod(*[a[k] for k in ORDER], None)


def _ln8(lib, **over):
    a = dict(LN8, **over)
    return lib.advgrpo_layernorm_mod_fp8(*[a[k] for k in ORDER], a["q0"], a["qs0"], a["q1"], a["qs1"], a["ldq"], None)


def _lnd(base=LN, **over):
    d = _lib.LnDesc()
    for k, v in dict(base, **over).items():
        setattr(d, k, v)
    return d


def _pair(lib, a, b):
    return lib.advgrpo_layernorm_mod_pair(ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None, None)


# the refusals all three forms make, as (arguments, text after "<entry>: ")
LN_SHARED = [(dict(x=None), "null pointer"), (dict(D=60), "need D % 8 == 0, D <= 4096 (D=60)"), (dict(D=4104, ldx=4104, ldo=4104, ldq=4104),
             "need D % 8 == 0, D <= 4096 (D=4104)"), (dict(M=0), "need D % 8 == 0, D <= 4096 (D=64)"),
             (dict(ldx=68), "pitches must be multiples of 8"), (dict(ldo=68), "pitches must be multiples of 8"),
             (dict(mod_stride=68), "pitches must be multiples of 8"), (dict(scale0=P), "scale0/shift0 come together"),
             (dict(shift0=P), "scale0/shift0 come together"), (dict(x=None, D=60, ldx=68, scale0=P), "null pointer"),
             (dict(D=60, ldx=68, scale0=P), "need D % 8 == 0, D <= 4096 (D=60)"), (dict(ldx=68, scale0=P), "pitches must be multiples of 8")]


@pytest.mark.parametrize("over,text", LN_SHARED + [
    (dict(out0=None), "null pointer"), (dict(out1=P), "out1 needs scale1/shift1"), (dict(out1=P, scale1=P), "out1 needs scale1/shift1"),
    (dict(out1=P, shift1=P, scale0=P), "scale0/shift0 come together")])
def test_layernorm_mod_refusals(lib, over, text):
    over = {k: v for k, v in over.items() if k != "ldq"}
    _refused(lib, _ln(lib, **over), "layernorm_mod: " + text)


@pytest.mark.parametrize("over,text", LN_SHARED + [
    (dict(q0=None), "null pointer"), (dict(q0=None, out0=P), "null pointer"), (dict(qs0=None), "null pointer"),
    (dict(ldq=68), "pitches must be multiples of 8"), (dict(ldq=56), "pitches must be multiples of 8"),
    (dict(ldq=56, scale0=P), "pitches must be multiples of 8"),
    (dict(q1=P, qs1=P), "a second output needs scale1/shift1"), (dict(out0=P, out1=P), "a second output needs scale1/shift1"),
    (dict(q1=P, qs1=P, scale1=P), "a second output needs scale1/shift1"), (dict(q1=P, scale1=P, shift1=P), "q1 needs qs1")])
def test_layernorm_mod_fp8_refusals(lib, over, text):
    _refused(lib, _ln8(lib, **over), "layernorm_mod_fp8: " + text)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("over,text", LN_SHARED + [
    (dict(out0=None, q0=None), "null pointer"), (dict(ldq=68), "pitches must be multiples of 8"),
    (dict(out1=P, out0=P), "a second output needs scale1/shift1"), (dict(out0=P, out1=P, scale1=P), "a second output needs scale1/shift1"),
    (dict(q0=P, qs0=None, ldq=64), "q0 needs qs0 and ldq >= D"), (dict(q0=P, qs0=P, ldq=56), "q0 needs qs0 and ldq >= D"),
    (dict(q0=P, qs0=P, ldq=56, scale0=P), "scale0/shift0 come together"),
    (dict(q0=None, out0=P, q1=P, qs1=P, scale1=P, shift1=P), "q1 needs q0 and qs1"),
    (dict(q0=P, qs0=P, ldq=64, q1=P, scale1=P, shift1=P), "q1 needs q0 and qs1"),
    (dict(q0=P, qs0=P, ldq=64, q1=P, qs1=P), "a second output needs scale1/shift1")])
def test_layernorm_mod_pair_refusals(lib, fp8, over, text):
    base = LN8 if fp8 else LN
    _refused(lib, _pair(lib, _lnd(base, **over), _lnd(base)), "layernorm_mod_pair: " + text)
    _refused(lib, _pair(lib, _lnd(base), _lnd(base, **over)), "layernorm_mod_pair: " + text)


def test_layernorm_mod_pair_wants_two_problems_of_one_kind(lib):
    _refused(lib, _pair(lib, _lnd(LN), _lnd(LN8)), "layernorm_mod_pair: both problems bf16 or both fp8")
    _refused(lib, _pair(lib, _lnd(LN8), _lnd(LN)), "layernorm_mod_pair: both problems bf16 or both fp8")
    _refused(lib, _pair(lib, _lnd(LN8, out0=P), _lnd(LN)), "layernorm_mod_pair: both problems bf16 or both fp8")
    _refused(lib, _pair(lib, None, _lnd(LN)), "layernorm_mod_pair: null pointer")
    _refused(lib, _pair(lib, _lnd(LN), None), "layernorm_mod_pair: null pointer")
    _refused(lib, _pair(lib, _lnd(LN, D=60), None), "layernorm_mod_pair: need D % 8 == 0, D <= 4096 (D=60)")     # a is looked at first


def test_rmsnorm_rows_refusals(lib):
    rms = lambda x=P, ldx=64, out=P, ldo=64, w=P, M=4, D=64: lib.advgrpo_rmsnorm_rows(x, ldx, out, ldo, w, M, D, 1e-6, None)
    _refused(lib, rms(w=None), "rmsnorm_rows: null pointer")
    _refused(lib, rms(x=None), "rmsnorm_rows: null pointer")
    _refused(lib, rms(out=None), "rmsnorm_rows: null pointer")
    _refused(lib, rms(D=60), "rmsnorm_rows: need D % 8 == 0, D <= 4096 (D=60)")
    _refused(lib, rms(D=4104, ldx=4104, ldo=4104), "rmsnorm_rows: need D % 8 == 0, D <= 4096 (D=4104)")
    _refused(lib, rms(ldx=68), "rmsnorm_rows: pitches must be multiples of 8")
    _refused(lib, rms(ldo=68), "rmsnorm_rows: pitches must be multiples of 8")
