#!/usr/bin/env python3
"""Which kernels of two BUILT libraries are the same instructions (no GPU needed)?

    python tools/kernel_diff.py OLD.so NEW.so [--rename 'OLD-REGEX=NEW' ...] [--only REGEX] [--census] [--md]

Kernels are matched by demangled name, after the renames (re.sub on the names of OLD) — for a refactor that merges or renames
kernel templates.  Per kernel one of
    identical   the same instruction text: mnemonics and operands of the disassembly, without addresses, and with the
                kernel's own symbol taken out of branch targets
    differs     with both instruction counts (--census: registers, scratch, spills, LDS and the hot loop of
                tools/kernel_census.py on both sides)
    only in OLD / only in NEW
Exit status 1 if anything differs or is on one side only (after --only).
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census as kc  # noqa: E402


def kernels(lib, tmp, tag):
    """{(mangled name, code object index): (code object path, metadata, [instruction text])} of every kernel in the library."""
    out = {}
    for i, co in enumerate(kc.code_objects(lib)):
        path = os.path.join(tmp, f"{tag}{i}.co")
        with open(path, "wb") as f:
            f.write(co)
        meta = kc.kernel_metadata(path)
        txt = subprocess.run([kc._tool("llvm-objdump"), "-d", "--no-show-raw-insn", path], check=True, capture_output=True, text=True).stdout
        sym = None
        for line in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                sym = (m.group(1), i) if m.group(1) in meta else None
                if sym:
                    out[sym] = (path, meta[sym[0]], [])
                continue
            if sym is None or not line.startswith("\t"):
                continue
            ins = re.sub(r"\s*//.*$", "", line.strip())        # the address, and a branch's target as <symbol+offset>
            if ins != "...":                                   # (a run of zero padding behind the kernel's last instruction)
                out[sym][2].append(re.sub(r"\s+", " ", ins))   # (a branch's operand is its relative offset: kept)
    return out


def short_name(name):
    """`void fa::kern<A, 1>(params)` -> `fa::kern<A, 1>`: a kernel template's parameter types follow from its arguments, and a
    refactor that computes them from the arguments changes how they are spelled in the mangled name, not what they are."""
    s = name.replace("(anonymous namespace)", "{anon}")
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            s = s[:i]
            break
    return s.split(" ", 1)[1] if s.startswith("void ") else s


def census_of(path, sym, meta):
    ins = kc.disassemble(path, sym)
    _h, _b, span = kc.hot_loop(ins)
    hist = collections.Counter(mn for _o, mn, _t in span)
    top = " ".join(f"{k}:{v}" for k, v in sorted(hist.items(), key=lambda kv: (-kv[1], kv[0]))[:6])
    return dict(meta, loop=len(span), loop_mfma=sum(v for k, v in hist.items() if k.startswith("v_mfma")), top=top)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=NEW", help="re.sub on the demangled kernel names of OLD")
    ap.add_argument("--only", default="", help="regex: report only kernels whose (new) name matches")
    ap.add_argument("--census", action="store_true", help="registers and hot loop of both sides for kernels that differ")
    ap.add_argument("--md", action="store_true", help="the differing kernels as a markdown table")
    ap.add_argument("--list", action="store_true", help="list the identical kernels too")
    args = ap.parse_args()
    renames = [r.split("=", 1) for r in args.rename]
    only = re.compile(args.only)
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(args.old, tmp, "a"), kernels(args.new, tmp, "b")
        names = kc.demangle(sorted({s for s, _c in list(old) + list(new)}))

        def keyed(lib, is_old):
            full = {}
            for ent in lib:
                n = names[ent[0]]
                for rx, to in (renames if is_old else []):
                    n = re.sub(rx, to, n)
                full[ent] = n
            short = collections.Counter(short_name(n) for n in full.values())
            out = {}
            for ent, n in full.items():
                k = short_name(n) if short[short_name(n)] == 1 else n    # overloads keep their parameter lists
                while k in out:
                    k += " (again)"                                       # one name in two code objects: in the library's order
                out[k] = ent
            return out
        ko, kn = keyed(old, True), keyed(new, False)
        same, diff, only_old, only_new = [], [], [], []
        for n in sorted(set(ko) | set(kn)):
            if not only.search(n):
                continue
            if n not in kn:
                only_old.append(n)
            elif n not in ko:
                only_new.append(n)
            elif old[ko[n]][2] == new[kn[n]][2]:
                same.append(n)
            else:
                diff.append(n)
        print(f"{len(same)} identical, {len(diff)} differ, {len(only_old)} only in OLD, {len(only_new)} only in NEW")
        if args.list:
            for n in same:
                print("identical  ", n)
        cols = ("vgpr", "agpr", "sgpr", "scratch", "sgpr_spills", "vgpr_spills", "lds", "loop", "loop_mfma")
        if args.md and diff:
            print("| kernel | instructions | " + " | ".join(cols) + " |\n|---|---|" + "---|" * len(cols))
        for n in diff:
            a, b = old[ko[n]], new[kn[n]]
            if not args.census:
                print(f"differs     {n}: {len(a[2])} -> {len(b[2])} instructions")
                continue
            ca, cb = census_of(a[0], ko[n][0], a[1]), census_of(b[0], kn[n][0], b[1])
            if args.md:
                print(f"| `{n}` | {len(a[2])} -> {len(b[2])} | " + " | ".join(str(ca[c]) if ca[c] == cb[c] else f"{ca[c]} -> {cb[c]}" for c in cols) + " |")
            else:
                print(f"differs     {n}: {len(a[2])} -> {len(b[2])} instructions")
                for side, c in (("old", ca), ("new", cb)):
                    print(f"    {side}  " + "  ".join(f"{k} {c[k]}" for k in cols) + f"  | {c['top']}")
        for n in only_old:
            print("only in OLD ", n)
        for n in only_new:
            print("only in NEW ", n)
    sys.exit(1 if diff or only_old or only_new else 0)


if __name__ == "__main__":
    main()
