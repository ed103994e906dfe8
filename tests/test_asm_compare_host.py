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


# ------------------------------------------------------------------------------------------------ RENAMED and REORDERED
RENAMED = ["s_load_dwordx2 s[2:3], s[4:5], 0x0", "v_mov_b32_e32 v3, 0", "global_store_dword v3, v0, s[2:3]"]      # other registers
LONG = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", "v_add_f32_e32 v2, v0, v0", "v_mul_f32_e32 v3, v0, v0",
        "global_store_dword v1, v2, s[0:1]", "global_store_dword v1, v3, s[0:1] offset:4"]
MOVED = [LONG[0], LONG[2], LONG[1], LONG[3], LONG[4], LONG[5]]                                                        # two slots swapped
OTHER_OPCODE = LONG[:3] + ["v_fma_f32 v3, v0, v0, v0"] + LONG[4:]


def verdict_of(lines, name):
    hit = [ln.split()[0] for ln in lines if re.fullmatch(r"\w+\s+" + re.escape(name) + r" \(\d+ lines\)", ln.strip())]
    assert len(hit) == 1, (name, lines)
    return hit[0]


def test_other_registers_are_renamed(ac):
    old, new = kernel("_Z11copy_kernelPf", BODY), kernel("_Z11copy_kernelPf", RENAMED)
    lines, bad, _ = ac.compare(old, new)
    assert bad == 1 and verdict_of(lines, "copy_kernel") == "RENAMED"
    lines, bad, _ = ac.compare(old, new, allow_reordered=True)
    assert bad == 0 and verdict_of(lines, "copy_kernel") == "RENAMED"
    # an immediate is no register: v1, 0 -> v1, 1 under other register numbers is still a difference
    lines, bad, _ = ac.compare(old, kernel("_Z11copy_kernelPf", [RENAMED[0], "v_mov_b32_e32 v3, 1", RENAMED[2]]), allow_reordered=True)
    assert bad == 1 and verdict_of(lines, "copy_kernel") == "DIFFERS"


def test_moved_instructions_are_reordered(ac):
    old, new = kernel("_Z11copy_kernelPf", LONG), kernel("_Z11copy_kernelPf", MOVED)
    lines, bad, _ = ac.compare(old, new)
    assert bad == 1 and verdict_of(lines, "copy_kernel") == "REORDERED"
    assert "+\tv_add_f32_e32 v2, v0, v0" in lines and "-\tv_add_f32_e32 v2, v0, v0" in lines   # the diff is printed: what moved
    lines, bad, _ = ac.compare(old, new, allow_reordered=True)
    assert bad == 0 and verdict_of(lines, "copy_kernel") == "REORDERED"
    lines, bad, _ = ac.compare(old, kernel("_Z11copy_kernelPf", OTHER_OPCODE), allow_reordered=True)     # another multiset of opcodes
    assert bad == 1 and verdict_of(lines, "copy_kernel") == "DIFFERS"


@pytest.mark.parametrize("body,new_body", [(BODY, RENAMED), (LONG, MOVED)])
def test_another_descriptor_stays_differs(ac, body, new_body):
    old = kernel("_Z11copy_kernelPf", body)
    new = kernel("_Z11copy_kernelPf", new_body).replace(".amdhsa_next_free_vgpr 12", ".amdhsa_next_free_vgpr 13")
    for allow in (False, True):
        lines, bad, _ = ac.compare(old, new, allow_reordered=allow)
        assert bad == 1 and verdict_of(lines, "copy_kernel") == "DIFFERS"


def test_allow_reordered_exit_status_and_directory_mode(ac, tmp_path, capsys):
    old, new = tmp_path / "old", tmp_path / "new"
    old.mkdir()
    new.mkdir()
    (old / "a.s").write_text(kernel("_Z11copy_kernelPf", BODY) + kernel("_Z11attn_kernelPf", LONG))
    (new / "a.s").write_text(kernel("_Z11copy_kernelPf", RENAMED) + kernel("_Z11attn_kernelPf", MOVED))
    (old / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY))
    (new / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", BODY))
    assert ac.main(str(old), str(new)) == 1                                   # as before: anything but EQUAL fails
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "DIFFERS a.s (2 kernels, 2 missing or different)" and out[-1] == "EQUAL   b.s (1 kernels)"
    assert ac.main(str(old), str(new), allow_reordered=True) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "REORDERED a.s (2 kernels)" and out[-1] == "EQUAL   b.s (1 kernels)"
    assert verdict_of(out, "copy_kernel") == "RENAMED" and verdict_of(out, "attn_kernel") == "REORDERED"
    (new / "b.s").write_text(kernel("_Z11norm_kernelILi4ELb0EEvPf", CHANGED))
    assert ac.main(str(old), str(new), allow_reordered=True) == 1             # a real difference still fails


def test_command_line_flag(tmp_path):
    import subprocess
    import sys
    # (kernel names c++filt leaves alone, so the tool's own demangler call works with or without binutils' table)
    (tmp_path / "old.s").write_text(kernel("_Z11copy_kernelPf", BODY))
    (tmp_path / "new.s").write_text(kernel("_Z11copy_kernelPf", RENAMED))
    run = lambda *flags: subprocess.run([sys.executable, str(_PATH), *flags], capture_output=True, text=True)
    assert run(str(tmp_path / "old.s"), str(tmp_path / "new.s")).returncode == 1
    for args in (("--allow-reordered", str(tmp_path / "old.s"), str(tmp_path / "new.s")), (str(tmp_path / "old.s"), str(tmp_path / "new.s"), "--allow-reordered")):
        r = run(*args)
        assert r.returncode == 0 and r.stdout.startswith("RENAMED"), r
