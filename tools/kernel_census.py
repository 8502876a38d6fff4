#!/usr/bin/env python3
"""Instruction census of one kernel of the BUILT library (no GPU needed): registers, scratch and the mnemonic histogram of
its hot loop, read from the code object with the ROCm disassembler.

    python tools/kernel_census.py [--lib PATH] [--json] [--all] 'REGEX of the (demangled or mangled) kernel name'

The hot loop is the loop (in the control-flow graph of the disassembly) of the backward branch that holds the most MFMAs, the
smallest such loop on a tie: for the stream kernels that is the steady-state loop over key tiles / row blocks.  Every block of
the loop is counted, the rarely taken ones (mask, rescale) too: an upper bound of what a trip issues.
`lane_moves` = v_readlane_b32 + v_writelane_b32 in that loop: SGPRs spilled into VGPR lanes.
"""
import argparse
import collections
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "flashattention-pytorch_amd", "flashattention_lab_cuda", "libfa_mi355x.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# the default forward: bf16, d = 128, dense, 128-key tiles, ring depth 4, K-ahead schedule, production instantiation
# (mangled, so that it matches with or without a demangler: <bf16_tag, 128, false, 4, false, 4, false, true, false>)
DEFAULT_FWD = "fwd_mfma_stag_kernelINS_8bf16_tagELi128ELb0ELi4ELb0ELi4ELb0ELb1ELb0EEE"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if p is None:
        raise FileNotFoundError(f"{name} not found (ROCm's llvm/bin)")
    return p


def code_objects(lib, arch="gfx950"):
    """The device code objects for `arch` in the library's offload bundles, as bytes."""
    blob = open(lib, "rb").read()
    out = []
    for m in re.finditer(re.escape(MAGIC), blob):
        off = m.start()
        (n,) = struct.unpack_from("<Q", blob, off + len(MAGIC))
        p = off + len(MAGIC) + 8
        for _ in range(n):
            o, s, t = struct.unpack_from("<QQQ", blob, p)
            p += 24
            triple = blob[p:p + t].decode()
            p += t
            if arch in triple and s:
                out.append(blob[off + o:off + o + s])
    return out


def kernel_metadata(co_path):
    """{mangled name: {vgpr, agpr, sgpr, scratch, sgpr_spills, vgpr_spills, lds}} from the code object's notes."""
    txt = subprocess.run([_tool("llvm-readelf"), "--notes", co_path], check=True, capture_output=True, text=True).stdout
    res = {}
    for block in re.split(r"^  - (?=\.)", txt, flags=re.M)[1:]:
        def field(key, block=block):
            m = re.search(rf"^\s*\.{key}:\s+(\S+)", block, flags=re.M)
            return m.group(1) if m else None
        name = field("name")
        if name is None:
            continue
        res[name] = {"vgpr": int(field("vgpr_count")), "agpr": int(field("agpr_count") or 0), "sgpr": int(field("sgpr_count")),
                     "scratch": int(field("private_segment_fixed_size")), "sgpr_spills": int(field("sgpr_spill_count") or 0),
                     "vgpr_spills": int(field("vgpr_spill_count") or 0), "lds": int(field("group_segment_fixed_size"))}
    return res


def demangle(names):
    for filt in ("llvm-cxxfilt", "c++filt"):   # whichever the machine has; without one the names stay mangled
        try:
            out = subprocess.run([_tool(filt)], input="\n".join(names), check=True, capture_output=True, text=True).stdout
            return dict(zip(names, out.split("\n")))
        except (FileNotFoundError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def disassemble(co_path, symbol):
    """[(offset in the kernel, mnemonic, branch target offset or None)]"""
    txt = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={symbol}", co_path],
                         check=True, capture_output=True, text=True).stdout
    ins, base = [], None
    for line in txt.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            base = int(m.group(1), 16) if m.group(2) == symbol else None
            continue
        if base is None or not line.startswith("\t"):
            continue
        m = re.match(r"^\t(\S+).*//\s*([0-9A-Fa-f]+):", line)
        if not m:
            continue
        tgt = None
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            t = re.search(re.escape(symbol) + r"(?:\+0x([0-9a-f]+))?>\s*$", line)
            if t:
                tgt = int(t.group(1) or "0", 16)
        ins.append((int(m.group(2), 16) - base, m.group(1), tgt))
    return ins


def _sccs(nodes, succs):
    """Strongly connected components (Tarjan, iterative) of the graph restricted to `nodes`."""
    index, low, on, stack, out, n = {}, {}, set(), [], [], 0
    for root in nodes:
        if root in index:
            continue
        work = [(root, iter(succs[root]))]
        index[root] = low[root] = n; n += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in nodes:
                    continue
                if w not in index:
                    index[w] = low[w] = n; n += 1; stack.append(w); on.add(w)
                    work.append((w, iter(succs[w])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = set()
                    while True:
                        w = stack.pop(); on.discard(w); comp.add(w)
                        if w == v:
                            break
                    out.append(comp)
    return out


def hot_loop(ins):
    """(lowest offset, highest offset, instructions) of the loop that holds the most MFMAs.  Loops are the cycles of the
    control-flow graph (strongly connected components; hipcc lays rarely taken blocks out of line and enters rotated loops in
    the middle, so neither a branch's address span nor its dominator tree finds them); an inner loop (what stays a cycle with
    the entry blocks taken away) is preferred while it keeps every MFMA of the outer one."""
    offs = [i[0] for i in ins]
    leaders = {offs[0]} | {t for _o, _m, t in ins if t is not None}
    for k, (_o, mn, _t) in enumerate(ins[:-1]):
        if mn.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            leaders.add(offs[k + 1])
    blocks, cur = {}, None               # leader -> its instructions
    for i in ins:
        if i[0] in leaders:
            cur = blocks.setdefault(i[0], [])
        cur.append(i)
    order = sorted(blocks)
    succs = {b: set() for b in order}
    for k, b in enumerate(order):
        _o, mn, tgt = blocks[b][-1]
        if tgt in succs:
            succs[b].add(tgt)
        if not mn.startswith(("s_branch", "s_endpgm", "s_setpc")) and k + 1 < len(order):
            succs[b].add(order[k + 1])
    mfma = {b: sum(1 for i in blocks[b] if i[1].startswith("v_mfma")) for b in order}

    def cycles(nodes):
        return [c for c in _sccs(nodes, succs) if len(c) > 1 or next(iter(c)) in succs[next(iter(c))]]

    def pick(cs):
        return min(cs, key=lambda c: (-sum(mfma[b] for b in c), len(c), min(c))) if cs else None

    loop = pick(cycles(set(order)))
    if loop is None:
        return None, None, []
    while True:
        entries = {b for b in loop if any(b in succs[p] for p in order if p not in loop)}
        inner = pick(cycles(loop - entries))
        if inner is None or sum(mfma[b] for b in inner) < sum(mfma[b] for b in loop):
            break
        loop = inner
    body = [i for blk in sorted(loop) for i in blocks[blk]]
    return body[0][0], body[-1][0], body


def census(lib, pattern):
    """One dict per kernel of `lib` whose name matches the regex `pattern`."""
    rx, found = re.compile(pattern), []
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib)):
            path = os.path.join(tmp, f"{i}.co")
            open(path, "wb").write(co)
            meta = kernel_metadata(path)
            nice = demangle(list(meta))
            for sym, regs in meta.items():
                if not (rx.search(nice[sym]) or rx.search(sym)):
                    continue
                ins = disassemble(path, sym)
                head, back, span = hot_loop(ins)
                hist = collections.Counter(mn for _o, mn, _t in span)
                found.append({"kernel": nice[sym], "symbol": sym, **regs, "instructions": len(ins), "loop_first": head, "loop_last": back,
                              "loop_instructions": len(span), "loop_mfma": sum(v for k, v in hist.items() if k.startswith("v_mfma")),
                              "lane_moves": hist.get("v_readlane_b32", 0) + hist.get("v_writelane_b32", 0),
                              "loop_s_nop": hist.get("s_nop", 0),
                              "loop_branches": sum(v for k, v in hist.items() if k.startswith(("s_cbranch", "s_branch"))),
                              "kernel_lane_moves": sum(1 for i in ins if i[1] in ("v_readlane_b32", "v_writelane_b32")),
                              "histogram": dict(sorted(hist.items(), key=lambda kv: (-kv[1], kv[0])))})
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pattern", nargs="?", default=re.escape(DEFAULT_FWD), help="regex of the kernel name (default: the default forward)")
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--all", action="store_true", help="allow more than one matching kernel")
    args = ap.parse_args()
    found = census(args.lib, args.pattern)
    if not found or (len(found) > 1 and not args.all):
        sys.exit(f"{len(found)} kernels match {args.pattern!r}" + "".join("\n  " + f["kernel"] for f in found))
    if args.json:
        print(json.dumps(found if args.all else found[0]))
        return
    for f in found:
        print(f"kernel   {f['kernel']}")
        print(f"registers  vgpr {f['vgpr']}  agpr {f['agpr']}  sgpr {f['sgpr']}  scratch {f['scratch']} B  "
              f"sgpr spills {f['sgpr_spills']}  vgpr spills {f['vgpr_spills']}  static lds {f['lds']} B")
        print(f"kernel   {f['instructions']} instructions, {f['kernel_lane_moves']} lane moves")
        print(f"loop     +0x{f['loop_first']:x} .. +0x{f['loop_last']:x}: {f['loop_instructions']} instructions, {f['loop_mfma']} MFMA, "
              f"{f['lane_moves']} lane moves, {f['loop_s_nop']} s_nop, {f['loop_branches']} branches")
        print("histogram  " + "  ".join(f"{k} {v}" for k, v in f["histogram"].items()))
        print()


if __name__ == "__main__":
    main()
