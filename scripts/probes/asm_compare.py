"""Kernel by kernel, is the device assembly of two builds the same?

    python scripts/probes/asm_compare.py old.s new.s        two builds of one .hip file
    python scripts/probes/asm_compare.py OLD_DIR NEW_DIR    every X.s of OLD_DIR against NEW_DIR/X.s
    python scripts/probes/asm_compare.py --allow-reordered OLD NEW      RENAMED and REORDERED (below) count as clean

`make -C adv_grpo_amd/csrc asm [EXPERIMENTS=1]` writes obj/asm/<name>.s (obj-exp/asm/ with EXPERIMENTS=1) for every .hip source with
that file's own flags; build it in a checkout of the old commit and in the new tree and hand the two directories to this tool.  By hand:
    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S x.hip -o x.s      (in the source's directory, so that the includes resolve)

Compared: every line between a kernel's label and its .Lfunc_end (instructions, the .amdhsa_ kernel descriptor with its register and
scratch counts).  Normalised: comments, debug directives, the numbers of local labels (they count the functions of the file) and mangled
symbol names (a kernel that became a template gets another name and a comdat section).  Kernels are matched by their exact demangled
name; an old kernel without such a match is also looked up with a trailing `false` template argument of the NEW build stripped (a
parameter the new build added with a default, such as VARLEN).  The directory mode prints one line per file, and the per-kernel lines
of the files that are not clean.

Verdicts per kernel, from the strictest: EQUAL (the normalised lines are the same); RENAMED (the same sequence of instructions once the
register operands v7, v[2:3], s4, s[0:1], a0, a[0:3] are masked: another register allocation of the same schedule); REORDERED (the same
multiset of opcodes, operands ignored, in another order -- whether the dependencies are the same is for a run to show; the same
opcodes in the SAME order with another immediate or offset are not a reordering); DIFFERS.  RENAMED and REORDERED also require an identical .amdhsa_ descriptor (register, scratch and LDS counts): with another
descriptor the kernel DIFFERS.  Exit status 1 unless every kernel (in the directory mode, every file) of the old build is there and
EQUAL; with --allow-reordered RENAMED and REORDERED pass as well."""
import collections
import difflib
import os
import re
import subprocess
import sys


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()


def kernels(text):
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None and "kernel" in m.group(1):
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        if re.match(r"^\s*(;|\.loc|\.file|\.cfi|\.text|\.section\s+\.text)", ln):
            continue
        ln = re.sub(r";.*$", "", ln.rstrip()).rstrip()
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        out[cur].append(re.sub(r"_Z\w+", "SYM", ln))
    return out


def key(name):
    d = demangle(name).replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", d).replace("void ", "")


def strip_false(k):
    return re.sub(r"<false>$", "", re.sub(r", false>$", ">", k))


_REG = re.compile(r"\b[vsa](\d+\b|\[\d+(:\d+)?\])")
VERDICTS = ("EQUAL", "RENAMED", "REORDERED", "DIFFERS")     # from the strictest


def verdict(old_body, new_body):
    if old_body == new_body:
        return "EQUAL"
    def split(body):
        return [ln for ln in body if ".amdhsa_" not in ln], [ln for ln in body if ".amdhsa_" in ln]
    (old_ins, old_desc), (new_ins, new_desc) = split(old_body), split(new_body)
    if old_desc != new_desc:
        return "DIFFERS"
    if [_REG.sub("REG", ln) for ln in old_ins] == [_REG.sub("REG", ln) for ln in new_ins]:
        return "RENAMED"
    def opcodes(ins):
        return [ln.split()[0] for ln in ins if ln.strip()]
    old_ops, new_ops = opcodes(old_ins), opcodes(new_ins)
    # (the same opcodes in the same order, yet not RENAMED: an immediate, an offset or a wait count changed -- nothing moved)
    return "REORDERED" if old_ops != new_ops and collections.Counter(old_ops) == collections.Counter(new_ops) else "DIFFERS"


def compare(old_text, new_text, allow_reordered=False):
    """-> (lines of the report, kernels of the old text that are missing or not clean, kernels compared)"""
    clean = VERDICTS[:3] if allow_reordered else VERDICTS[:1]
    old = {key(k): v for k, v in kernels(old_text).items()}
    new = {key(k): v for k, v in kernels(new_text).items()}
    stripped = {strip_false(k): k for k in new if strip_false(k) != k}
    lines, bad, used = [], 0, set()
    for k, body in old.items():
        nk = k if k in new else stripped.get(k)
        if nk is None:
            lines.append(f"MISSING {k}")
            bad += 1
            continue
        used.add(nk)
        v = verdict(body, new[nk])
        bad += v not in clean
        lines.append(f"{v:<7} {k} ({len(body)} lines)")
        if v in VERDICTS[2:]:
            lines += list(difflib.unified_diff(body, new[nk], lineterm="", n=0))[:40]
    lines.append(f"only in the new build: {sorted(k for k in new if k not in used)}")
    return lines, bad, len(old)


def compare_dirs(old_dir, new_dir, allow_reordered=False):
    lines, bad_files = [], 0
    for name in sorted(f for f in os.listdir(old_dir) if f.endswith(".s")):
        path = os.path.join(new_dir, name)
        if not os.path.exists(path):
            lines.append(f"MISSING {name}")
            bad_files += 1
            continue
        sub, bad, n = compare(open(os.path.join(old_dir, name)).read(), open(path).read(), allow_reordered)
        extra = not sub[-1].endswith("[]")
        # (a file that is clean only thanks to --allow-reordered is headed by its loosest verdict and lists its kernels)
        worst = max((VERDICTS.index(ln.split()[0]) for ln in sub if ln.split()[0] in VERDICTS), default=0)
        lines.append(f"{'DIFFERS' if bad else VERDICTS[worst]:<7} {name} ({n} kernels{', ' + str(bad) + ' missing or different' if bad else ''})")
        if bad or extra or worst:
            lines += ["    " + ln for ln in sub]
        bad_files += bad > 0
    return lines, bad_files


def main(old_path, new_path, allow_reordered=False):
    if os.path.isdir(old_path):
        lines, bad = compare_dirs(old_path, new_path, allow_reordered)
    else:
        lines, bad, _ = compare(open(old_path).read(), open(new_path).read(), allow_reordered)
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    paths = [a for a in sys.argv[1:] if a != "--allow-reordered"]
    sys.exit(main(paths[0], paths[1], allow_reordered=len(paths) != len(sys.argv) - 1))
