"""Per-kernel fingerprint of the gfx950 machine code, without a GPU.

Compiles every translation unit of ``build.SOURCES`` with the flags ``build.py`` uses plus ``--cuda-device-only -S`` and
prints one line per kernel: its register / spill / scratch / LDS metadata and a hash + length of its filtered instruction
stream -- in program order the mnemonics of every v_mfma*, ds_*, buffer_*, global_*, scratch_*, v_accvgpr_*, s_waitcnt
(with its operands), s_barrier, s_nop (with its operand), s_cbranch* and s_endpgm; register numbers are not part of it.
Scalar address set-up, which the compiler may order differently after a source-level refactor, is not in the stream.

    python tools/isa_fingerprint.py > profiles/isa_fingerprint_branch.txt       # all translation units, ~10 s each
    python tools/isa_fingerprint.py gemm_v5.hip --dump out/                     # also writes out/<kernel>.stream
    diff profiles/isa_fingerprint_parent.txt profiles/isa_fingerprint_branch.txt
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bind_your_avatar_implementation_amd import build  # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")
STREAM = re.compile(r"^(v_mfma|ds_|buffer_|global_|scratch_|v_accvgpr_|s_waitcnt|s_barrier|s_nop|s_cbranch|s_endpgm)")
WITH_OPERANDS = ("s_waitcnt", "s_nop")


def assemble(src, extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        cmd = [build._hipcc(), *build.compile_flags(src), *extra, "--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout.decode()}")
        with open(out) as f:
            return f.read()


def kernel_streams(asm):
    """{kernel symbol: [stream entries]} -- a kernel's text runs from its label to its .Lfunc_end."""
    streams, cur = {}, None
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if cur is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
            if m and not line.startswith(".L"):
                cur = m.group(1)
                streams[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        # (a line of inline asm may hold several instructions behind "\n\t": the assembly output has them on lines of their own)
        if STREAM.match(line):
            op = line.split(None, 1)
            keep = op[0] in WITH_OPERANDS and len(op) > 1
            streams[cur].append(op[0] + (" " + re.sub(r"\s+", " ", op[1]) if keep else ""))
    return streams


def kernel_metadata(asm):
    """{kernel symbol: {field: value}} from the amdhsa.kernels metadata (a kernel's own fields sit at the first indent level)."""
    kernels, in_md = [], False
    for raw in asm.splitlines():
        if raw.startswith("amdhsa.kernels:"):
            in_md = True
        elif in_md and (raw.startswith("amdhsa.") or raw.startswith("...")):
            break
        elif in_md:
            m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", raw)
            if not m:
                continue
            if m.group(1) == "  - ":
                kernels.append({})
            kernels[-1][m.group(2)] = m.group(3).strip()
    return {k[".name"]: k for k in kernels}


def fingerprint(src, extra=(), dump=None):
    asm = assemble(src, list(extra))
    streams, meta = kernel_streams(asm), kernel_metadata(asm)
    lines = []
    for name in sorted(meta):
        s = streams.get(name)
        if s is None:
            raise RuntimeError(f"{src}: no text found for kernel {name}")
        text = "\n".join(s) + "\n"
        if dump:
            os.makedirs(dump, exist_ok=True)
            with open(os.path.join(dump, name + ".stream"), "w") as f:
                f.write(text)
        fields = " ".join(f"{k[1:]}={meta[name].get(k, '?')}" for k in META)
        lines.append(f"{src} {name} {fields} stream_len={len(s)} stream_sha1={hashlib.sha1(text.encode()).hexdigest()[:16]}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="*", help="translation units (default: all of build.SOURCES)")
    ap.add_argument("--dump", help="directory for the filtered streams, one file per kernel")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra -D for probe / ablation builds")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    sources = a.sources or build.SOURCES
    extra = ["-D" + d for d in a.defines]
    with ThreadPoolExecutor(a.j) as ex:
        for lines in ex.map(lambda s: fingerprint(s, extra, a.dump), sources):
            print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
