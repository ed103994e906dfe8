"""Kernel by kernel, is the device assembly of two builds the same?

    python scripts/probes/asm_compare.py old.s new.s        two builds of one .hip file
    python scripts/probes/asm_compare.py OLD_DIR NEW_DIR    every X.s of OLD_DIR against NEW_DIR/X.s

`make -C adv_grpo_amd/csrc asm [EXPERIMENTS=1]` writes obj/asm/<name>.s (obj-exp/asm/ with EXPERIMENTS=1) for every .hip source with
that file's own flags; build it in a checkout of the old commit and in the new tree and hand the two directories to this tool.  By hand:
    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S x.hip -o x.s      (in the source's directory, so that the includes resolve)

Compared: every line between a kernel's label and its .Lfunc_end (instructions, the .amdhsa_ kernel descriptor with its register and
scratch counts).  Normalised: comments, debug directives, the numbers of local labels (they count the functions of the file) and mangled
symbol names (a kernel that became a template gets another name and a comdat section).  Kernels are matched by their exact demangled
name; an old kernel without such a match is also looked up with a trailing `false` template argument of the NEW build stripped (a
parameter the new build added with a default, such as VARLEN).  The directory mode prints one line per file, and the per-kernel lines
of the files that are not clean.  Exit status 1 when a kernel (or, in the directory mode, a file) of the old build is missing or differs."""
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


def compare(old_text, new_text):
    """-> (lines of the report, kernels of the old text that are missing or differ, kernels compared)"""
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
        same = body == new[nk]
        bad += not same
        lines.append(f"{'EQUAL  ' if same else 'DIFFERS'} {k} ({len(body)} lines)")
        if not same:
            lines += list(difflib.unified_diff(body, new[nk], lineterm="", n=0))[:40]
    lines.append(f"only in the new build: {sorted(k for k in new if k not in used)}")
    return lines, bad, len(old)


def compare_dirs(old_dir, new_dir):
    lines, bad_files = [], 0
    for name in sorted(f for f in os.listdir(old_dir) if f.endswith(".s")):
        path = os.path.join(new_dir, name)
        if not os.path.exists(path):
            lines.append(f"MISSING {name}")
            bad_files += 1
            continue
        sub, bad, n = compare(open(os.path.join(old_dir, name)).read(), open(path).read())
        extra = not sub[-1].endswith("[]")
        lines.append(f"{'DIFFERS' if bad else 'EQUAL  '} {name} ({n} kernels{', ' + str(bad) + ' missing or different' if bad else ''})")
        if bad or extra:
            lines += ["    " + ln for ln in sub]
        bad_files += bad > 0
    return lines, bad_files


def main(old_path, new_path):
    if os.path.isdir(old_path):
        lines, bad = compare_dirs(old_path, new_path)
    else:
        lines, bad, _ = compare(open(old_path).read(), open(new_path).read())
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
