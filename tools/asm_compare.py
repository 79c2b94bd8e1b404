#!/usr/bin/env python3
"""Compare two `make asm` outputs of csrc/zs_kernels.hip kernel by kernel.

    tools/asm_compare.py PARENT_DIR HEAD_DIR [--renames FILE] [--cxxfilt PROGRAM]

Each directory holds `zs_kernels.s` and `resource-usage.txt` as `make asm` leaves them in
build/asm.  Kernels are paired by demangled name (namespace, return type and parameter list
dropped); `--renames` is a file of `regex<TAB>replacement` lines applied to the parent's names
first, for kernels whose template arguments moved.  A kernel's text runs from its label to its
`.Lfunc_end`, kernel descriptor included, with comments dropped, the function number taken out of
`.LBB<function>_<block>` labels and mangled symbols replaced by their (renamed) names, so two
bodies compare equal exactly when their instruction streams and descriptors do.

Prints one tab-separated row per kernel: identical / differs / only-parent / only-head, the line
counts of both texts, and VGPRs, SGPRs, scratch and occupancy of both builds side by side.  Exits
non-zero if any kernel differs (text or any resource remark) or is unpaired.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

SHOWN = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")


def demangle(symbols, cxxfilt):
    out = subprocess.run([cxxfilt], input="\n".join(symbols), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return dict(zip(symbols, (short_name(n) for n in out)))


def short_name(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for k, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:k]
    return name


def kernel_texts(path):
    """{mangled symbol: [raw lines from the label to .Lfunc_end]} for every .amdhsa_kernel."""
    lines = open(path).read().split("\n")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    texts, cur = {}, None
    for ln in lines:
        m = re.match(r"^(\w+):", ln)
        if cur is None and m and m.group(1) in kernels:
            cur = m.group(1)
            texts[cur] = []
        elif cur is not None and re.match(r"^\.Lfunc_end\d+:", ln):
            cur = None
        elif cur is not None:
            texts[cur].append(ln)
    return texts


def normalise(lines, names):
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln:
            continue
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        ln = re.sub(r"\b_Z\w+", lambda m: names.get(m.group(0), m.group(0)), ln)
        out.append(re.sub(r"\s+", " ", ln))
    return out


def resources(path):
    """{mangled symbol: {remark key: value}} from -Rpass-analysis=kernel-resource-usage."""
    res, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark:\s+(.+?):\s+(\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def load(directory, cxxfilt, renames):
    texts = kernel_texts(os.path.join(directory, "zs_kernels.s"))
    res = resources(os.path.join(directory, "resource-usage.txt"))
    names = demangle(sorted(texts), cxxfilt)
    for sym, name in names.items():
        for pat, rep in renames:
            name = re.sub(pat, rep, name)
        names[sym] = name
    if len(set(names.values())) != len(names):
        sys.exit(f"{directory}: two kernels share one name after renaming")
    return {names[s]: (normalise(t, names), res.get(s, {})) for s, t in texts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--renames")
    ap.add_argument("--cxxfilt", default=shutil.which("llvm-cxxfilt") or shutil.which("c++filt"))
    a = ap.parse_args()
    if not a.cxxfilt:
        sys.exit("no llvm-cxxfilt or c++filt on PATH: pass --cxxfilt")
    renames = []
    if a.renames:
        for ln in open(a.renames):
            if ln.strip() and not ln.startswith("#"):
                renames.append(tuple(ln.rstrip("\n").split("\t")))
    old, new = load(a.parent, a.cxxfilt, renames), load(a.head, a.cxxfilt, [])
    bad = 0
    print("\t".join(["kernel", "text", "lines parent", "lines head"] +
                    [f"{k} {side}" for k in SHOWN for side in ("parent", "head")] + ["resources"]))
    for name in sorted(set(old) | set(new)):
        (t0, r0), (t1, r1) = old.get(name, ([], {})), new.get(name, ([], {}))
        text = ("only-head" if name not in old else "only-parent" if name not in new else
                "identical" if t0 == t1 else "differs")
        same_res = r0 == r1 and bool(r0)
        bad += text != "identical" or not same_res
        print("\t".join([name, text, str(len(t0)), str(len(t1))] +
                        [r.get(k, "-") for k in SHOWN for r in (r0, r1)] +
                        ["identical" if same_res else "differs"]))
    print(f"# {len(old)} kernels at the parent, {len(new)} at head, "
          f"{len(set(old) & set(new))} paired, {bad} unpaired or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
