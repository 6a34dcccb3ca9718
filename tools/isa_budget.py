"""Instruction budget of a kernel in device assembly (hipcc --cuda-device-only -S):
per basic block the VALU / SALU / vector-memory / LDS instruction counts, the
kernel's register use and spills, and the loop blocks of the traversal step.

    python tools/isa_budget.py <file.s> [kernel-substring] [--blocks] [--json]

Build the assembly with the library's own flags: tools/isa_budget.py --build UNIT [EXTRA...]
runs the Makefile's asm rule for the device unit UNIT (ddgi_kernels, ddgi_update, ...; `all`:
every unit) with EXTRA added to its flags, and prints the path of each .s written.

    python tools/isa_budget.py --inventory <file.s> [<file.s> ...]

One line per kernel of the files, sorted by demangled name: SGPRs, VGPRs, VGPR and SGPR
spills, LDS and scratch bytes, the instruction count and the SHA-256 of the normalised
instruction stream (instructions and local labels only; the function index of .LBB<i>_<n>,
.Ltmp<n> and .Lfunc_* becomes a placeholder, since it changes with a function's position in
its unit). Two builds generate the same code for a kernel iff its lines are equal: a pull
request proves "before = after" by diffing two inventories.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
from collections import Counter, OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = f"{ROOT}/arkoserenderer_amd/csrc"


def kind(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def parse(path, key):
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l]
    if not starts:
        raise SystemExit(f"no kernel matching {key}")
    i0 = starts[0]
    name = lines[i0].split(":")[0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks = OrderedDict()
    cur = "entry"
    blocks[cur] = []
    for l in lines[i0 + 1:i1]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            cur = m.group(1)
            blocks[cur] = []
            continue
        s = l.strip()
        if s and not s.startswith((".", ";")):
            blocks[cur].append(s.split()[0])
    meta = {}
    text = "\n".join(lines)
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\n", text)
    if m:
        # the entry's scalar fields follow its .name up to .wavefront_size
        tail = text[m.end():m.end() + 4000]
        tail = tail[:tail.find(".wavefront_size")] if ".wavefront_size" in tail else tail
        for k in ("sgpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size"):
            mm = re.search(r"\." + k + r":\s+(\d+)", tail)
            if mm:
                meta[k] = int(mm.group(1))
    return name, blocks, meta


META = ("sgpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def inventory(paths):
    """[(mangled name, {META...}, instruction count, digest)] of every kernel of the files."""
    rows = []
    for path in paths:
        lines = open(path).read().split("\n")
        # the kernels' metadata: the entries of amdhsa.kernels, each a run of "    .key: value"
        meta = {}
        k0 = lines.index("amdhsa.kernels:")
        for entry in re.split(r"\n  - ", "\n".join(lines[k0 + 1:lines.index("amdhsa.target:", k0) if "amdhsa.target:" in lines[k0:] else len(lines)])):
            fields = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
            if "name" in fields:
                meta[fields["name"]] = {k: int(fields[k]) for k in META}
        for name in meta:
            i0 = lines.index(next(l for l in lines if l.startswith(name + ":")))
            i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
            stream, count = [], 0
            for l in lines[i0 + 1:i1]:
                t = l.split(";")[0].strip()
                label = re.match(r"^\.L\w+:$", t)
                if not t or (t.startswith(".") and not label):
                    continue
                count += 0 if label else 1
                t = re.sub(r"\.LBB\d+_", ".LBB#_", t)
                t = re.sub(r"\.L(tmp|func_begin|func_end)\d+", r".L\1#", t)
                stream.append(" ".join(t.split()))
            rows.append((name, meta[name], count, hashlib.sha256("\n".join(stream).encode()).hexdigest()))
    names = [r[0] for r in rows]
    dup = {n for n in names if names.count(n) > 1}
    if dup:
        raise SystemExit(f"kernels emitted by more than one unit: {sorted(dup)}")
    filt = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n") if filt else names
    return sorted((plain[i],) + rows[i] for i in range(len(rows)))


def main():
    if sys.argv[1] == "--build":
        unit, extra = sys.argv[2], sys.argv[3:]
        goal = "asm" if unit == "all" else f"build/{unit}.s"
        # (-B: a changed EXTRA is not a changed prerequisite)
        subprocess.run(["make", "-B" if extra else "-s", goal, "EXTRA=" + " ".join(extra)], cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
        for s in sorted(os.listdir(f"{CSRC}/build")):
            if s.endswith(".s") and unit in ("all", s[:-2]):
                print(f"{CSRC}/build/{s}")
        return
    if sys.argv[1] == "--inventory":
        rows = inventory(sys.argv[2:])
        print("# sgpr vgpr vgpr_spill sgpr_spill lds_bytes scratch_bytes instructions sha256(normalised stream) kernel")
        for plain, _, m, count, digest in rows:
            print(" ".join(str(m[k]) for k in META), count, digest, plain)
        print(f"# {len(rows)} kernels")
        return
    path = sys.argv[1]
    key = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else "k_traceILb0ELi6ENS0_9ProbeRays"
    name, blocks, meta = parse(path, key)
    tot = Counter()
    rows = []
    for b, ops in blocks.items():
        c = Counter(kind(o) for o in ops)
        tot += c
        rows.append((b, len(ops), dict(c), Counter(ops).most_common(6)))
    out = {"kernel": name, "meta": meta, "total": dict(tot), "blocks": {b: c for b, _, c, _ in rows}}
    if "--json" in sys.argv:
        print(json.dumps(out))
        return
    print(name)
    print("registers:", meta)
    print("static totals:", dict(tot))
    if "--blocks" in sys.argv:
        for b, n, c, top in rows:
            print(f"{b:12s} {n:4d} {c} {top}")


if __name__ == "__main__":
    main()
