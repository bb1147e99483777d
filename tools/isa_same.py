#!/usr/bin/env python3
"""Is the gfx950 code of one source the same as at an earlier revision?  The gate of a kernel refactor: identical instruction
streams have identical results and identical speed.  Needs hipcc and git, no GPU.

    isa_same.py <rev> <path.hip> [--kernel NAME ...] [--except NAME ...] [--was <old path.hip> [--was-kernel NAME ...]] [-DFOO ...]

Compiles `git show <rev>:<path>` (next to that revision's headers) and the working-tree file with build.FLAGS to device assembly,
drops the per-translation-unit __hip_cuid_* symbol and the source file name, and exits non-zero at the first difference.
With --kernel (repeatable) only the kernels whose mangled name contains NAME are compared -- their instruction streams and
their .amdhsa_kernel descriptors -- which is the question when a kernel has moved OUT of the file: did the ones that stayed change?
For the kernel that moved, --was names the file it had at <rev> (and --was-kernel the name it had there, if that changed too); the
kernels' own symbol names are then left out of the comparison.
With --except (repeatable) every kernel of the working-tree file whose mangled name does NOT contain NAME is compared, each on its
own and in name order: for a file that dropped a kernel or instantiates its kernels in another order.
"""
import os, re, subprocess, sys, tempfile
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bayer_low_light_image_enhancement_amd import build as B  # noqa: E402

rev, path, flags, kernels, was, was_kernels, excepted = sys.argv[1], os.path.relpath(os.path.abspath(sys.argv[2]), REPO), [], [], None, [], []
rest = sys.argv[3:]
while rest:
    a = rest.pop(0)
    if a == "--kernel":
        kernels.append(rest.pop(0))
    elif a == "--except":
        excepted.append(rest.pop(0))
    elif a == "--was":
        was = os.path.relpath(os.path.abspath(rest.pop(0)), REPO)
    elif a == "--was-kernel":
        was_kernels.append(rest.pop(0))
    else:
        flags.append(a)


def only_kernels(lines, kernels):
    """The bodies (label .. .Lfunc_end) and descriptors (.amdhsa_kernel .. .end_amdhsa_kernel) of the chosen kernels; the
    numbers of local labels and of .Lfunc_end belong to the whole file and are normalised per kernel."""
    out, keep, names = [], False, []
    for ln in lines:
        m = re.match(r"^(\w+):", ln) or re.match(r"^\s*\.amdhsa_kernel\s+(\w+)", ln)
        if m and any(k in m.group(1) for k in kernels):
            keep, first = True, None
            names.append(m.group(1))
        if keep:
            def renum(mm):
                nonlocal first
                first = int(mm.group(2)) if first is None else first
                return f"{mm.group(1)}{int(mm.group(2)) - first}_"
            ln = re.sub(r"(?<![.\w])BB\d+_", "BB_", ln)          # the function's number in the file, in the loop comments
            ln = re.sub(r":\s+;", ": ;", ln)                     # ... whose column moves with the width of the label's number
            out.append(re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin)(\d+)_?", renum, ln) if ".L" in ln else ln)
        if keep and (ln.startswith(".Lfunc_end") or ".end_amdhsa_kernel" in ln):
            keep = False
    if was:                                                  # another file, perhaps another namespace or name: compare the code alone
        for i, n in enumerate(sorted(set(names), key=len, reverse=True)):
            out = [ln.replace(n, f"<kernel {i}>") for ln in out]
    return out, sorted(set(names))


def listing(src, kernels):
    r = subprocess.run([B._hipcc(), *B.FLAGS, *flags, "--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if "__hip_cuid_" not in ln and not ln.lstrip().startswith(".file")]
    if excepted:      # every other kernel of the working-tree file (compiled second: `kernels` is filled by then), one at a time
        every = sorted(m.group(1) for ln in lines if (m := re.match(r"^\s*\.amdhsa_kernel\s+(\w+)", ln)))
        if not kernels:
            kernels.extend(k for k in every if not any(e in k for e in excepted))
        print(f"{src}: {len(kernels)} of {len(every)} kernel(s)")
        return [ln for k in kernels for ln in only_kernels(lines, [k])[0]]
    if kernels:
        lines, names = only_kernels(lines, kernels)
        if not names:
            sys.exit(f"no kernel of {src} matches {kernels}")
        print(f"{src}: {len(names)} kernel(s): " + " ".join(names))
    return lines


with tempfile.TemporaryDirectory(prefix="isa_same_") as tmp:
    tree = subprocess.check_output(["git", "ls-tree", "-r", "--name-only", rev], cwd=REPO, text=True).split("\n")
    for f in (f for f in tree if f == (was or path) or f.endswith((".h", ".hpp"))):       # the source and every header of that revision
        os.makedirs(os.path.dirname(os.path.join(tmp, f)), exist_ok=True)
        with open(os.path.join(tmp, f), "wb") as out:
            out.write(subprocess.check_output(["git", "show", f"{rev}:{f}"], cwd=REPO))
    new = listing(os.path.join(REPO, path), kernels)
    old = listing(os.path.join(tmp, was or path), was_kernels or kernels)
what = f"{path} {' '.join(flags)}".strip() + (f" [all but {', '.join(excepted)}]" if excepted else f" [{', '.join(kernels)}]" if kernels else "")
i = next((i for i, (a, b) in enumerate(zip(old, new)) if a != b), min(len(old), len(new)))
if i == len(old) == len(new):
    print(f"identical: {what}: {len(new)} lines of gfx950 assembly, {rev} and the working tree")
    sys.exit(0)
kernel = next((m.group(1) for ln in reversed(new[:i + 1]) if (m := re.match(r"^(\w+):", ln))), "(before the first function)")
print(f"DIFFERENT: {what}: line {i + 1}, in {kernel}")
for tag, text in ((f"--- {rev}", old), ("+++ working tree", new)):
    print(tag, *text[max(i - 3, 0):i + 12], sep="\n")
sys.exit(1)
