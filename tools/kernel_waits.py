#!/usr/bin/env python3
"""List, for one kernel of the runtime, what stands between its entry and its first s_barrier: every scalar load, vector load,
LDS write, wait and branch, in program order, with the labels branches go to.  Scalar loads through the kernel-argument pointer
("argument load") are told apart from those that read the operator's arrays ("scalar load").  The order of loads and waits in a prologue is a
property of the compiled code, not of the source; this prints it, so DESIGN can quote a listing where it used to make a claim.

The device code of saena_amd/csrc/sgpu_runtime.hip is compiled to assembly with the Makefile's HIPFLAGS (hipcc only: no GPU, nothing
but the compiler), or an assembly file made that way is read with --asm.

    tools/kernel_waits.py 'k_vidxw<0, false, false>'                    # this tree
    tools/kernel_waits.py --tree ../parent 'k_vidxw<1, false, false>'   # another checkout
    tools/kernel_waits.py --asm runtime.s --list k_vidxw                # the kernels of an assembly file whose names hold k_vidxw
    tools/kernel_waits.py --counts 'k_vidxw<0, false, false>'           # instructions per class and basic block, the whole kernel

--counts is a STATIC count: what a launch executes is the sum over the blocks its waves pass through, once per pass.

A kernel is named as the demangler prints it; blanks are ignored and any unique part of the name will do."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

KINDS = (                                    # mnemonic prefix -> what the listing calls it
    ("s_load", "scalar load"), ("s_buffer_load", "scalar load"),
    ("global_load", "vector load"), ("flat_load", "vector load"), ("buffer_load", "vector load"), ("scratch_load", "vector load"),
    ("ds_write", "LDS write"), ("ds_store", "LDS write"),
    ("s_waitcnt", "wait"),
    ("s_cbranch", "branch"), ("s_branch", "branch"),
    ("s_barrier", "barrier"),
)


def makefile_flags(csrc):
    """HIPCC and HIPFLAGS as saena_amd/csrc/Makefile sets them (the environment overrides its ?= defaults, as in make)"""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {}
    for name, op, value in re.findall(r"^(\w+)\s*(\?=|:=)\s*(.*)$", text, re.M):
        var[name] = os.environ.get(name, value) if op == "?=" else value
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    return expand(var["HIPCC"]), expand(var["HIPFLAGS"]).split()


def compile_asm(tree, out):
    csrc = os.path.join(tree, "saena_amd", "csrc")
    hipcc, flags = makefile_flags(csrc)
    cmd = [hipcc, *flags, "--cuda-device-only", "-S", "-o", out, "sgpu_runtime.hip"]
    print("# " + " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, cwd=csrc, check=True)
    return hipcc


def demangle(names, hipcc):
    tool = None
    for cand in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), "llvm-cxxfilt") if hipcc else None,
                 os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt") if hipcc else None,
                 shutil.which("llvm-cxxfilt"), "/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("c++filt")):
        if cand and os.path.exists(cand):
            tool = cand
            break
    if tool is None:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def kernels(asm):
    """-> {symbol: [lines of its body]}, {symbol: the SGPR pair that holds the kernel-argument pointer at entry, or None} for every
    kernel (.amdhsa_kernel names) of the file"""
    lines = open(asm).read().splitlines()
    syms = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    bodies, argptr, cur, desc = {}, {}, None, None
    for ln in lines:
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", ln)
        if m and m.group(1) in syms:
            cur = bodies.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end", ln):
                cur = None
            else:
                cur.append(ln)
        # the kernel descriptor: the user SGPRs come in a fixed order, the argument pointer after buffer (4), dispatch (2) and queue (2)
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            desc = {"sym": m.group(1)}
        elif desc is not None:
            m = re.match(r"^\s*\.amdhsa_user_sgpr_(\w+)\s+(\d+)", ln)
            if m:
                desc[m.group(1)] = int(m.group(2))
            elif re.match(r"^\s*\.end_amdhsa_kernel", ln):
                at = 4 * desc.get("private_segment_buffer", 0) + 2 * desc.get("dispatch_ptr", 0) + 2 * desc.get("queue_ptr", 0)
                argptr[desc["sym"]] = f"s[{at}:{at + 1}]" if desc.get("kernarg_segment_ptr") else None
                desc = None
    return bodies, argptr


def listing(body, argptr=None):
    """the instructions of KINDS up to and including the first barrier, and every label on the way.  A scalar load through the
    kernel-argument pointer is an "argument load": it reads the dispatch's own block of arguments, not the operator's arrays (told by
    the base register, which holds while the kernel leaves that pair alone -- a prologue does)"""
    out, n = [], 0
    for ln in body:
        text = ln.split(";")[0].strip()
        if not text or text.startswith("."):
            m = re.match(r"^(\.LBB[\w.]*):", text)
            if m:
                out.append(f"      {m.group(1)}:")
            continue
        n += 1
        mnem = text.split()[0]
        for prefix, kind in KINDS:
            if mnem.startswith(prefix):
                if kind == "scalar load" and argptr and re.search(r",\s*" + re.escape(argptr) + r"\s*,", text):
                    kind = "argument load"
                out.append(f"{n:5d} {kind:<13s} {text}")
                break
        if mnem.startswith("s_barrier"):
            return out, n, True
    return out, n, False


CLASSES = ("VALU", "SALU", "s_nop", "SMEM", "LDS", "VMEM load", "VMEM store", "wait", "branch", "other")


def classify(mnem):
    if mnem.startswith("v_"):
        return "VALU"
    if mnem.startswith("ds_"):
        return "LDS"
    if mnem.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if mnem.startswith(("global_load", "flat_load", "buffer_load", "scratch_load")):
        return "VMEM load"
    if mnem.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM store"
    if mnem.startswith("s_waitcnt"):
        return "wait"
    if mnem.startswith("s_nop"):
        return "s_nop"
    if mnem.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
        return "branch"
    if mnem.startswith("s_barrier"):
        return "other"
    return "SALU" if mnem.startswith("s_") else "other"


def counts(body):
    """-> [(block label, {class: instructions})] in program order (the entry block is "entry"), over the whole kernel"""
    blocks = [("entry", dict.fromkeys(CLASSES, 0))]
    for ln in body:
        text = ln.split(";")[0].strip()
        if not text or text.startswith("."):
            m = re.match(r"^(\.LBB[\w.]*):", text)
            if m:
                blocks.append((m.group(1), dict.fromkeys(CLASSES, 0)))
            continue
        blocks[-1][1][classify(text.split()[0])] += 1
    return blocks


def counts_table(blocks):
    out = [f"   {'block':<12s}" + "".join(f"{c:>11s}" for c in CLASSES) + f"{'all':>8s}"]
    total = dict.fromkeys(CLASSES, 0)
    for label, n in blocks:
        out.append(f"   {label:<12s}" + "".join(f"{n[c]:11d}" for c in CLASSES) + f"{sum(n.values()):8d}")
        for c in CLASSES:
            total[c] += n[c]
    out.append(f"   {'all blocks':<12s}" + "".join(f"{total[c]:11d}" for c in CLASSES) + f"{sum(total.values()):8d}")
    return out


def summary(rows):
    """how many of each kind the listing holds -- on every path together: which blocks a launch runs is for the reader to follow"""
    kinds = [r[6:19].strip() for r in rows if not r.endswith(":")]
    return ["on all paths together: " + ", ".join(f"{kinds.count(k)} {k}{'es' if k == 'branch' else 's'}" for k in ("argument load", "scalar load", "vector load", "LDS write", "wait", "branch"))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="*", help="kernels to list, as the demangler prints them (any unique part, blanks ignored)")
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="the checkout to compile (default: this one)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep-asm", help="keep the compiled assembly here")
    ap.add_argument("--counts", action="store_true", help="print the static instruction counts per class and basic block of the whole kernel instead")
    ap.add_argument("--list", metavar="PART", help="print the demangled names that hold PART and stop")
    a = ap.parse_args()
    hipcc = None
    with tempfile.TemporaryDirectory() as tmp:
        asm = a.asm
        if asm is None:
            asm = a.keep_asm or os.path.join(tmp, "sgpu_runtime.s")
            hipcc = compile_asm(os.path.abspath(a.tree), os.path.abspath(asm))
        bodies, argptr = kernels(asm)
        names = demangle(sorted(bodies), hipcc or makefile_flags(os.path.join(os.path.abspath(a.tree), "saena_amd", "csrc"))[0])
        squeeze = lambda s: re.sub(r"\s+", "", s)
        if a.list is not None:
            print("\n".join(sorted(d for d in names.values() if squeeze(a.list) in squeeze(d))))
            return 0
        for want in a.kernel:
            hits = [s for s, d in names.items() if squeeze(want) in squeeze(d)]
            if len(hits) != 1:
                print(f"{want!r} names {len(hits)} kernels" + "".join("\n  " + names[h] for h in hits), file=sys.stderr)
                return 1
            print(f"== {names[hits[0]]}")
            if a.counts:
                print("\n".join(counts_table(counts(bodies[hits[0]]))))
                print()
                continue
            rows, n, found = listing(bodies[hits[0]], argptr.get(hits[0]))
            print(f"   entry to the first s_barrier: {n} instructions" if found else f"   no s_barrier: all {n} instructions")
            print("\n".join(rows))
            print("\n".join("   " + s for s in summary(rows)))
            print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
