"""Register-spill check for the hand-written GEMM kernels (profiles/gemm_spills_r04.md).

Emits the gfx950 device assembly of a kernel source (``hipcc --cuda-device-only -S``, ~4 min for
gemm_big.hip) or reads an existing ``.s`` and reports, per ``gemm_big_k`` instantiation and for ``gemm_wg_k``, the scratch
(spill) instructions in the whole body and inside its MFMA main loop (the span between the first and
last ``v_mfma`` of the densest cluster).  Exits 1 if any main loop holds more than ``--max-loop``.

    python scripts/check_spills.py                      # compile csrc/kernels/gemm_big.hip
    python scripts/check_spills.py --asm /tmp/gb.s      # scan an existing assembly file
    python scripts/check_spills.py --all-kernels --src csrc/kernels/llama.hip
                                                        # every kernel of a source: exits 1 on any scratch use
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = re.compile(r"\n(_ZN\w*gemm_(?:big|wg)_k\w*):[^\n]*\n(.*?)\.Lfunc_end", re.S)
TPL = re.compile(r"gemm_big_kILi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")


def emit(src: str, out: str, defines) -> None:
    sys.path.insert(0, os.path.join(ROOT, "csrc"))
    import build  # noqa: E402  (csrc/build.py: the library's flags for this source)
    cmd = [build.HIPCC, *build.flags_for(src), "-x", "hip", "--cuda-device-only", "-S", src, "-o", out] + \
        [f"-D{d}" for d in defines]
    subprocess.run(cmd, check=True)


def loop_spills(lines):
    """(MFMAs, scratch instructions, scratch instructions inside the MFMA main loop) of one kernel body."""
    mf = [i for i, ln in enumerate(lines) if "v_mfma" in ln]
    sc = [i for i, ln in enumerate(lines) if "scratch_" in ln]
    loop = 0
    if mf:
        # MFMA clusters: runs of v_mfma lines less than 400 lines apart; the main loop is the largest
        clusters, a, prev = [], mf[0], mf[0]
        for i in mf[1:]:
            if i - prev > 400:
                clusters.append((a, prev))
                a = i
            prev = i
        clusters.append((a, prev))
        lo, hi = max(clusters, key=lambda c: sum(1 for x in mf if c[0] <= x <= c[1]))
        loop = sum(1 for i in sc if lo <= i <= hi)
    return len(mf), len(sc), loop


def scan(text: str):
    rows = []
    for m in PAT.finditer(text):
        name, body = m.group(1), m.group(2)
        t = TPL.search(name)
        tag = "".join(t.groups()) if t else "wg" if "gemm_wg_k" in name else name[-40:]
        rows.append((tag, *loop_spills(body.split("\n"))))
    return rows


ANY = re.compile(r"\n(\w+):[^\n]*\n(.*?)\.Lfunc_end", re.S)
META = re.compile(r"\.name:\s+(\w+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)")


def scan_all(text: str):
    """(kernel, scratch instructions, private segment bytes) of every kernel in the assembly."""
    priv = {m.group(1): int(m.group(2)) for m in META.finditer(text)}
    return [(m.group(1), sum("scratch_" in ln for ln in m.group(2).split("\n")), priv[m.group(1)])
            for m in ANY.finditer(text) if m.group(1) in priv]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="")
    ap.add_argument("--src", default=os.path.join(ROOT, "csrc", "kernels", "gemm_big.hip"))
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--max-loop", type=int, default=16)
    ap.add_argument("--all-kernels", action="store_true")
    a = ap.parse_args()
    path = a.asm
    if not path:
        path = os.path.join(tempfile.mkdtemp(), "k.s")
        emit(a.src, path, a.defines)
    if a.all_kernels:
        with open(path) as f:
            rows = scan_all(f.read())
        print("kernel  scratch-instructions  private-segment-bytes")
        for name, nsc, nb in rows:
            print(f"{name} {nsc} {nb}{'  <-- scratch' if nsc or nb else ''}")
        return 1 if not rows or any(nsc or nb for _, nsc, nb in rows) else 0
    with open(path) as f:
        rows = scan(f.read())
    bad = 0
    print("instantiation <LA LB KTAIL DIRECT BNB N192>  mfma  scratch  scratch-in-main-loop")
    for tag, nmf, nsc, loop in rows:
        flag = "  <-- spills in the main loop" if loop > a.max_loop else ""
        bad += bool(flag)
        print(f"{tag:>10} {nmf:6d} {nsc:8d} {loop:8d}{flag}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
