#!/usr/bin/env python3
"""Is the device code of two source trees the same, function by function?  ("Source-only changes to the engines")

    python tools/isa_diff.py BEFORE AFTER [--save DIR]

BEFORE / AFTER: a source tree (the directory that holds balatro_gym_amd/csrc/bg_lib.hip; e.g. `git worktree add ../parent HEAD~1`) or an assembly
file saved by an earlier run (`--save DIR` keeps before.s / after.s and the compiler's remarks beside them as before.remarks / after.remarks).
A tree is compiled, device code only, to assembly:

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Wno-unused-value --cuda-device-only -S -Rpass-analysis=kernel-resource-usage

(build.py's flags without the host half; minutes per tree, the two trees side by side).  The assembly is split per function -- a kernel's descriptor
travels with its code, what stands in front of the first function and behind the last one are two pieces of their own --, the function number in
`.LBB<n>_<m>` / `BB<n>_<m>` (loop comments) / `.Lfunc_begin<n>` / `.Lfunc_end<n>` and the random `__hip_cuid_<hex>` symbol are normalised, and the pieces are compared as text:
no instruction is looked for.  Printed: the line counts of every function whose text differs, or "identical"; then the compiler's per-kernel
resource table of the step engines in the format of profiles/above_cap_resources.txt (all kernels with --all-kernels).  Exit status 1 when
something differs."""
from __future__ import annotations

import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
FIELDS = ["VGPRs", "VGPRs Spill", "ScratchSize", "SGPRs Spill", "LDS Size", "Occupancy"]


def hipcc() -> str:
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def compile_tree(tree: str, out_s: str) -> str:
    """tree -> assembly at out_s; returns the compiler's stderr (the resource remarks)."""
    src = os.path.join(tree, "balatro_gym_amd", "csrc", "bg_lib.hip")
    if not os.path.exists(src):
        raise SystemExit(f"{tree}: no balatro_gym_amd/csrc/bg_lib.hip")
    r = subprocess.run([hipcc()] + FLAGS + ["-o", out_s, os.path.basename(src)], cwd=os.path.dirname(src), capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{tree}: hipcc failed\n{r.stderr[-4000:]}")
    return r.stderr


def load(arg: str, label: str, workdir: str) -> tuple[str, str | None]:
    """(assembly text, remarks or None) of a tree or a saved assembly file."""
    if os.path.isdir(arg):
        out_s = os.path.join(workdir, label + ".s")
        remarks = compile_tree(arg, out_s)
        with open(os.path.join(workdir, label + ".remarks"), "w") as f:
            f.write(remarks)
    else:
        out_s = arg
        rpath = os.path.splitext(arg)[0] + ".remarks"
        remarks = open(rpath).read() if os.path.exists(rpath) else None
    with open(out_s) as f:
        return f.read(), remarks


_START = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$")
# (`BB<n>_<m>` stands in the comments of the blocks of a loop -- `Header=`, `Parent Loop`, `Child Loop`: a function added in front of others renumbers it
# like the labels, and a number that gains a digit shifts the padding in front of a label's comment)
_NORM = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"), (re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_"),
         (re.compile(r"\bBB\d+_"), "BB_"), (re.compile(r"^(\.LBB_\d+:) +;"), r"\1 ;")]


def split(asm: str) -> tuple[dict[str, list[str]], set[str]]:
    """{function name: its normalised lines} in file order, with "(head)" and "(tail)" for what surrounds the functions, and the set of kernels.
    A function's piece starts at its `.globl` / `.type` preamble and ends where the next one's starts; the last one ends at the metadata."""
    lines = asm.split("\n")
    starts = []   # (first line of the preamble, name)
    for i, ln in enumerate(lines):
        m = _START.match(ln)
        if m:
            j = i
            while j > 0 and lines[j - 1].lstrip().startswith((".globl", ".p2align", ".type", ".protected", ".weak", ".hidden", ".section\t.text")):
                j -= 1
            starts.append((j, m.group(1)))
    tail = next((i for i, ln in enumerate(lines) if ln.startswith("\t.amdgpu_metadata") or ".AMDGPU.gpr_maximums" in ln), len(lines))
    if starts and tail < starts[-1][0]:
        tail = len(lines)
    # the module's end-of-text padding (`.text`, `.p2alignl`, `.fill`) stands behind whichever function is last: it belongs to the tail, not to that
    # function, or a kernel appended to the module would make the previously last one differ by three lines that are no instruction
    while starts and tail > starts[-1][0] and lines[tail - 1].strip().startswith((".text", ".p2alignl", ".fill")):
        tail -= 1
    pieces: dict[str, list[str]] = {"(head)": lines[:starts[0][0]] if starts else lines}
    for k, (j, name) in enumerate(starts):
        end = starts[k + 1][0] if k + 1 < len(starts) else tail
        pieces[name] = lines[j:end]
    pieces["(tail)"] = lines[tail:] if starts else []
    kernels = set(re.findall(r"^\t\.amdhsa_kernel (\S+)", asm, re.M))
    for name, body in pieces.items():
        out = []
        for ln in body:
            for rx, to in _NORM:
                ln = rx.sub(to, ln)
            out.append(ln)
        pieces[name] = out
    return pieces, kernels


def resources(remarks: str | None) -> dict[str, dict[str, str]]:
    """{mangled kernel name: {field: value}} from -Rpass-analysis=kernel-resource-usage."""
    res: dict[str, dict[str, str]] = {}
    cur = None
    for ln in (remarks or "").split("\n"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", ln)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(": ")
        if key == "Function Name":
            cur = res.setdefault(val, {})
        elif cur is not None:
            cur[key.split(" [")[0]] = val
    return res


def demangle(names: list[str]) -> dict[str, str]:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        out = names
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        depth = 0
        for i, ch in enumerate(d[1:], 1):   # cut the argument list: the first "(" outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                d = d[:i]
                break
        short[n] = d
    return short


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--save", metavar="DIR", help="keep before.s / after.s and their remarks here")
    ap.add_argument("--all-kernels", action="store_true", help="the resource table of every kernel, not of the step engines only")
    args = ap.parse_args()
    workdir = args.save or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(workdir, exist_ok=True)
    try:
        ver = subprocess.run([hipcc(), "--version"], capture_output=True, text=True).stdout.strip().split("\n")
        print("\n".join(l for l in ver if "version" in l.lower()))
        print(f"hipcc {' '.join(FLAGS)} bg_lib.hip")
        with concurrent.futures.ThreadPoolExecutor(2) as ex:
            fb, fa = ex.submit(load, args.before, "before", workdir), ex.submit(load, args.after, "after", workdir)
            (asm_b, rem_b), (asm_a, rem_a) = fb.result(), fa.result()
    finally:
        if not args.save:
            shutil.rmtree(workdir, ignore_errors=True)
    pb, kb = split(asm_b)
    pa, ka = split(asm_a)
    for label, asm, p, k in (("before", asm_b, pb, kb), ("after", asm_a, pa, ka)):
        print(f"{label}: {asm.count(chr(10))} lines, {len(p) - 2} functions, {len(k)} kernels")
    names = list(pb) + [n for n in pa if n not in pb]
    dm = demangle(names)
    differ = 0
    for n in names:
        b, a = pb.get(n), pa.get(n)
        if b != a:
            differ += 1
            print(f"differs: {dm[n]}: {len(b) if b is not None else 'absent'} -> {len(a) if a is not None else 'absent'} lines")
    print("identical" if not differ else f"{differ} of {len(names)} pieces differ (functions, and what stands in front of and behind them)")
    rb, ra = resources(rem_b), resources(rem_a)
    if rb or ra:
        rows = [n for n in names if (n in kb or n in ka) and (args.all_kernels or "bg_engine" in n)]
        print()
        print("kernel".ljust(90) + "".join(f.rjust(23) for f in FIELDS))
        changed = []
        for n in rows:
            cells = []
            for f in FIELDS:
                b, a = rb.get(n, {}).get(f, "?"), ra.get(n, {}).get(f, "?")
                star = " *" if b != a and "?" not in (b, a) else ""
                if star:
                    changed.append((dm[n], f))
                cells.append(f"{b} -> {a}{star}".rjust(23))
            print(dm[n].ljust(90) + "".join(cells))
        print("changed: " + (", ".join(f"{k} ({f})" for k, f in changed) if changed else "nothing"))
    else:
        print("(no resource table: an assembly file without its .remarks beside it)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
