"""Kernel by kernel, is the device assembly of two builds of one .hip file the same?

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S old.hip -o old.s      (same directory, so that the includes resolve)
    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S new.hip -o new.s
    python scripts/probes/asm_compare.py old.s new.s

Compared: every line between a kernel's label and its .Lfunc_end (instructions, the .amdhsa_ kernel descriptor with its register and
scratch counts).  Normalised: comments, debug directives, the numbers of local labels (they count the functions of the file), mangled
symbol names (a kernel that became a template gets another name and a comdat section), and a trailing `false` template argument of the NEW
build (a defaulted parameter such as VARLEN).  Exit status 1 when a kernel of the old build is missing or differs."""
import difflib
import re
import subprocess
import sys


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
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


def key(name, new):
    d = demangle(name).replace("(anonymous namespace)::", "")
    d = re.sub(r"\(.*$", "", d).replace("void ", "")
    if new:
        d = re.sub(r"<false>$", "", re.sub(r", false>$", ">", d))
    return d


def main(old_path, new_path):
    old = {key(k, False): v for k, v in kernels(old_path).items()}
    new = {key(k, True): v for k, v in kernels(new_path).items()}
    bad = 0
    for k, body in old.items():
        if k not in new:
            print("MISSING", k)
            bad += 1
            continue
        same = body == new[k]
        bad += not same
        print("EQUAL  " if same else "DIFFERS", k, f"({len(body)} lines)")
        if not same:
            print("\n".join(list(difflib.unified_diff(body, new[k], lineterm="", n=0))[:40]))
    print("only in the new build:", sorted(k for k in new if k not in old))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
