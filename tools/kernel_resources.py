#!/usr/bin/env python3
"""tools/kernel_resources.py -- registers, spills, scratch and LDS of every kernel in the library, from the compiler's own metadata, and a digest of each
kernel's instruction text (hipcc -S --cuda-device-only per source file; no GPU needed).  The files are the Makefile's SRCS that hold a kernel.
  python tools/kernel_resources.py > profiles/r05_resources.txt
Two trees compile to the same machine code where the tables of the two agree: diff the two outputs (the digest is of the text normalise() leaves)."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kvazzup_amd", "csrc")


def kernel_files():
    """SRCS of the Makefile, without the host-only units (no __global__ function in them)"""
    mk = open(os.path.join(SRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    return [f for f in srcs if "__global__" in open(os.path.join(SRC, f)).read()]


def normalise(lines):
    """a kernel's assembly lines (its label to its .Lfunc_end) as what two builds can be compared by: comments (from ';') go, blank and alignment lines
    go, and local labels lose the index of the function within its file (.LBB<i>_<n> -> .LBB_<n>), which moves when a kernel is added in front"""
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln or re.match(r"\.(p2align|balign|align)\b", ln):
            continue
        out.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln))
    return out


def digest(lines):
    return hashlib.sha256("\n".join(normalise(lines)).encode()).hexdigest()[:16]


def kernel_bodies(text):
    """{symbol: lines} of every function of an assembly file, the line after its label up to its .Lfunc_end (the kernel descriptor lies in between and names
    the kernel, as its section does: the symbol reads <self> in the lines, so that a kernel that was renamed compares equal)"""
    bodies, name, body = {}, None, []
    for ln in text.split("\n"):
        if name is None:
            m = re.match(r"([A-Za-z_][\w$.]*):", ln)
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
        elif re.match(r"\.Lfunc_end\d+:", ln):
            bodies[name], name = body, None
        else:
            body.append(ln.replace(name, "<self>"))
    return bodies


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def rows_of(f):
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", s, os.path.join(SRC, f)],
                       check=True, stderr=subprocess.DEVNULL, cwd=SRC)
        text = open(s).read()
    bodies = kernel_bodies(text)
    rows = []
    # the metadata block: one YAML-ish entry per kernel
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        e = m.group(0)
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, e) or [None, "?"])[1]
        rows.append((f, g("name"), g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("sgpr_spill_count"), g("vgpr_spill_count"), g("private_segment_fixed_size"),
                     g("group_segment_fixed_size"), digest(bodies[g("name")])))
    return rows


def main():
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        rows = [r for rs in pool.map(rows_of, kernel_files()) for r in rs]
    names = demangle([r[1] for r in rows])
    print("# registers, spills, scratch (private segment), LDS and instruction-text digest per kernel of libkvazzup_amd.so -- compiler output, hipcc -O3 --offload-arch=gfx950 (tools/kernel_resources.py)")
    print("%-18s %-78s %5s %5s %5s %10s %10s %8s %7s %-16s" % ("file", "kernel", "vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "lds", "digest"))
    for r in rows:
        n = names[r[1]].replace("(anonymous namespace)::", "").replace("kvzx::", "").split("(")[0].replace("void ", "")
        print("%-18s %-78s %5s %5s %5s %10s %10s %8s %7s %-16s" % (r[0], n[:78], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]))


if __name__ == "__main__":
    main()
