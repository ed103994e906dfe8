"""scripts/probes/asm_compare.py on small synthetic assembly texts: the matching of kernel names, what counts as a difference, the
directory mode and the exit status.  No GPU, no compiler; the demangler is a table, so that the test needs no binutils either."""
import importlib.util
import pathlib
import re

import pytest

_PATH = pathlib.Path(__file__).resolve().parents[1] / "scripts" / "probes" / "asm_compare.py"

NAMES = {
    "_Z11norm_kernelILi4ELb0EEvPf": "void norm_kernel<4, false>(float*)",
    "_Z11norm_kernelILi4ELb1EEvPf": "void norm_kernel<4, true>(float*)",
    "_Z11attn_kernelPf": "attn_kernel(float*)",
    "_Z11attn_kernelILb0EEvPf": "void attn_kernel<false>(float*)",
    "_Z11attn_kernelILb1EEvPf": "void attn_kernel<true>(float*)",
    "_Z11copy_kernelPf": "(anonymous namespace)::copy_kernel(float*)",
}


@pytest.fixture()
def ac(monkeypatch):
    spec = importlib.util.spec_from_file_location("asm_compare_under_test", _PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "demangle", lambda name: NAMES[name])
    return mod


def kernel(sym, body, label=3, comment="note"):
    """one labelled kernel: its instructions, a branch to a local label, a descriptor line, the end marker"""
    lines = [f"\t.section\t.text.{sym},\"axG\",@progbits,{sym},comdat", f"{sym}:", f"; %bb.0: {comment}"]
    lines += [f"\t{ins}\t; {comment}" for ins in body]
    lines += [f"\ts_cbranch_scc1 .LBB{label}_2", f".LBB{label}_2:", "\ts_endpgm", "\t.amdhsa_next_free_vgpr 12",
              f".Lfunc_end{label}:", f"\t.size\t{sym}, .Lfunc_end{label}-{sym}"]
    return "\n".join(lines) + "\n"


BODY = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", "global_store_dword v1, v0, s[0:1]"]
CHANGED = [BODY[0], "v_mov_b32_e32 v1, 1", BODY[2]]


def status(lines, name):
    hit = [ln.split()[0] for ln in lines if re.fullmatch(r"(EQUAL  |DIFFERS) " + re.escape(name) + r" \(\d+ lines\)", ln.strip())]
    assert len(hit) == 1, (name, lines)
    return hit[0]


def test_trailing_false_on_both_sides_is_equal(ac):
    old = kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY) + kernel("_Z11attn_kernelILb0EEvPf", BODY)
    new = kernel("_Z11attn_kernelILb0EEvPf", BODY) + kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY)
    lines, bad, n = ac.compare(old, new)
    assert (bad, n) == (0, 2)
    assert status(lines, "norm_kernel<4, false>") == "EQUAL"
    assert status(lines, "attn_kernel<false>") == "EQUAL"
    assert lines[-1] == "only in the new build: []"


def test_exact_name_wins_over_the_stripped_one(ac):
    # the new build has both attn_kernel (unchanged) and attn_kernel<false> (different): the old attn_kernel is its exact namesake
    old = kernel("_Z11attn_kernelPf", BODY)
    new = kernel("_Z11attn_kernelILb0EEvPf", CHANGED) + kernel("_Z11attn_kernelPf", BODY)
    lines, bad, _ = ac.compare(old, new)
    assert bad == 0 and status(lines, "attn_kernel") == "EQUAL"
    assert lines[-1] == "only in the new build: ['attn_kernel<false>']"


def test_old_plain_kernel_matches_new_defaulted_false(ac):
    old = kernel("_Z11attn_kernelPf", BODY)
    new = kernel("_Z11attn_kernelILb0EEvPf", BODY, label=7) + kernel("_Z11attn_kernelILb1EEvPf", CHANGED, label=8)
    lines, bad, _ = ac.compare(old, new)
    assert bad == 0 and status(lines, "attn_kernel") == "EQUAL"
    assert lines[-1] == "only in the new build: ['attn_kernel<true>']"


def test_changed_instruction_differs_and_exits_1(ac, tmp_path, capsys):
    (tmp_path / "old.s").write_text(kernel("_Z11copy_kernelPf", BODY) + kernel("_Z11attn_kernelPf", BODY))
    (tmp_path / "new.s").write_text(kernel("_Z11copy_kernelPf", CHANGED) + kernel("_Z11attn_kernelPf", BODY))
    assert ac.main(str(tmp_path / "old.s"), str(tmp_path / "new.s")) == 1
    out = capsys.readouterr().out.splitlines()
    assert status(out, "copy_kernel") == "DIFFERS" and status(out, "attn_kernel") == "EQUAL"
    assert "-\tv_mov_b32_e32 v1, 0" in out and "+\tv_mov_b32_e32 v1, 1" in out
    assert ac.main(str(tmp_path / "old.s"), str(tmp_path / "old.s")) == 0


def test_changed_descriptor_differs(ac):
    old = kernel("_Z11copy_kernelPf", BODY)
    lines, bad, _ = ac.compare(old, old.replace(".amdhsa_next_free_vgpr 12", ".amdhsa_next_free_vgpr 13"))
    assert bad == 1 and status(lines, "copy_kernel") == "DIFFERS"


def test_absent_kernel_is_missing_and_exits_1(ac, tmp_path, capsys):
    (tmp_path / "old.s").write_text(kernel("_Z11copy_kernelPf", BODY) + kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY))
    (tmp_path / "new.s").write_text(kernel("_Z11copy_kernelPf", BODY) + kernel("_Z11norm_kernelILi4ELb1EEvPf", BODY))
    assert ac.main(str(tmp_path / "old.s"), str(tmp_path / "new.s")) == 1
    out = capsys.readouterr().out.splitlines()
    assert "MISSING norm_kernel<4, false>" in out and status(out, "copy_kernel") == "EQUAL"
    assert out[-1] == "only in the new build: ['norm_kernel<4, true>']"


def test_label_numbers_and_comments_are_normalised(ac):
    old = kernel("_Z11copy_kernelPf", BODY, label=3, comment="old note")
    new = "; a file-level comment\n" + kernel("_Z11copy_kernelPf", BODY, label=41, comment="another note")
    lines, bad, _ = ac.compare(old, new)
    assert bad == 0 and status(lines, "copy_kernel") == "EQUAL"


def test_directory_mode_reports_per_file(ac, tmp_path, capsys):
    old, new = tmp_path / "old", tmp_path / "new"
    old.mkdir()
    new.mkdir()
    same = kernel("_Z11copy_kernelPf", BODY) + kernel("_Z11attn_kernelPf", BODY)
    (old / "a.s").write_text(same)
    (new / "a.s").write_text(same)
    (old / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY))
    (new / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY, label=9))
    (new / "only_new.s").write_text(same)      # not in OLD_DIR: not compared
    (old / "notes.txt").write_text("not assembly")
    assert ac.main(str(old), str(new)) == 0
    assert capsys.readouterr().out.splitlines() == ["EQUAL   a.s (2 kernels)", "EQUAL   b.s (1 kernels)"]

    (new / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", CHANGED))
    assert ac.main(str(old), str(new)) == 1
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "EQUAL   a.s (2 kernels)"
    assert out[1] == "DIFFERS b.s (1 kernels, 1 missing or different)"
    assert out[2] == "    DIFFERS norm_kernel<4, false> (7 lines)"

    (new / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY))
    (new / "a.s").unlink()
    assert ac.main(str(old), str(new)) == 1
    assert capsys.readouterr().out.splitlines() == ["MISSING a.s", "EQUAL   b.s (1 kernels)"]
