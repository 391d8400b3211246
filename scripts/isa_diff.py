#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every kernel source between two revisions (no GPU needed).

    python scripts/isa_diff.py REV_A [REV_B] [-j N]

Each csrc/kernels/*.hip is compiled to assembly (isa_census.compile_asm: the library's flags) once
from REV_A's csrc/ and once from REV_B's (default: the working tree); revisions are unpacked with
`git archive` into a temporary directory.  Lines that differ between two compiles of the same
source (.file, .ident, comments, the per-compile __hip_cuid_ symbol) are dropped; the rest must be
equal line for line.  Prints one markdown table row per file and, for a file that differs, the
kernel holding the first difference and that hunk.  Exit status 1 if any file differs.

--per-kernel gives one row per kernel instead: its body after normalising block labels and symbol
suffixes (identical / differs / removed / added), and parent / new VGPRs, SGPRs, scratch bytes, LDS
bytes, the scripts/check_spills.py count of scratch instructions in the MFMA main loop, and the waves
per SIMD the registers and the LDS allow.  Exit status 1 if a kept kernel's figure got worse.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_spills import loop_spills  # noqa: E402
from isa_census import compile_asm  # noqa: E402


def csrc_of(rev, tmp):
    """The csrc/ directory of a revision (None: the working tree)."""
    if rev is None:
        return os.path.join(ROOT, "csrc")
    dst = os.path.join(tmp, re.sub(r"\W", "_", rev))
    os.makedirs(dst)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "csrc"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return os.path.join(dst, "csrc")


def asm_lines(csrc, name, tmp):
    src = os.path.join(csrc, "kernels", name)
    if not os.path.exists(src):
        return None
    out = tempfile.mktemp(suffix=".s", dir=tmp)
    compile_asm(src, out, include=os.path.join(csrc, "include"))
    keep = []
    for l in open(out):
        s = l.strip()
        if s and not s.startswith((".file", ".ident", ";")) and "__hip_cuid_" not in s:
            keep.append(l.rstrip())
    return keep


def first_hunk(a, b):
    for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag != "equal":
            kernel = next((m.group(1) for l in reversed(a[:i0 + 1]) if (m := re.match(r"^(_Z\S+):", l))), "(no kernel)")
            lines = [f"-{l}" for l in a[i0:i1][:20]] + [f"+{l}" for l in b[j0:j1][:20]]
            return kernel, lines
    return None, []


META = {"vgpr": "vgpr_count", "sgpr": "sgpr_count", "scratch": "private_segment_fixed_size",
        "lds": "group_segment_fixed_size", "wg": "max_flat_workgroup_size"}


def kernel_table(lines):
    """{demangled kernel name: (normalised body lines, figures)} of one file's assembly."""
    meta, name, cur = {}, None, {}
    for l in lines:     # a kernel's metadata entry: keys in alphabetical order, .vgpr_count the last one read
        if (m := re.match(r"\s+(?:- )?\.name:\s+(_Z\S+)", l)):
            name = m.group(1)
        for k, f in META.items():
            if (m := re.match(r"\s+(?:- )?\." + f + r":\s+(\d+)", l)):
                cur[k] = int(m.group(1))
                if k == "vgpr":
                    meta[name], cur = cur, {}
    out = {}
    for i, l in enumerate(lines):
        if not (m := re.match(r"^(_Z\S+):", l)) or m.group(1) not in meta:
            continue
        j = next(k for k in range(i, len(lines)) if lines[k].strip().startswith(".Lfunc_end"))
        # block labels carry the function's index in the file, symbols a per-compile hash
        # (also in the trailing "; in Loop: Header=BB126_15" comments, which go)
        body = [re.sub(r"\.L(BB|tmp|func_\w+?)\d+(_\d+)?", r".L\1\2", x.split(";")[0].rstrip()) for x in lines[i + 1:j]]
        f = dict(meta[m.group(1)])
        f["loop"] = loop_spills(body)[2] if any("v_mfma" in x for x in body) else None
        # gfx950: 512 unified registers per SIMD lane in granules of 8, 160 KB of LDS per CU, 4 SIMDs
        by_lds = (163840 // f["lds"]) * (f["wg"] // 64) // 4 if f.get("lds") else 8
        f["waves"] = max(0, min(8, 512 // (-(-max(f["vgpr"], 1) // 8) * 8), by_lds))
        short = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"\(anonymous namespace\)::", "", short).split("(")[0]] = (body, f)
    return out


def per_kernel(names, fa, fb) -> int:
    worse = 0
    print("| file | kernel | body | VGPR p/n | SGPR p/n | scratch B p/n | LDS p/n | loop spills p/n | waves/SIMD p/n |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in names:
        ka, kb = kernel_table(fa[n].result() or []), kernel_table(fb[n].result() or [])
        for k in sorted(set(ka) | set(kb)):
            (x, p), (y, q) = ka.get(k, (None, {})), kb.get(k, (None, {}))
            if x is None or y is None:
                body = "added" if x is None else "REMOVED"
            elif x == y:
                body = "identical"
            else:
                nd = sum(max(i1 - i0, j1 - j0) for t, i0, i1, j0, j1 in
                         difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes() if t != "equal")
                body = f"differs ({nd} of {len(x)} lines)"
            def show(key):
                return "/".join("-" if d.get(key) is None else str(d[key]) for d in (p, q) if d)
            if p and q:
                worse += any((q[f] or 0) > (p[f] or 0) for f in ("vgpr", "sgpr", "scratch", "lds", "loop"))
                worse += q["waves"] < p["waves"]
            print(f"| `{n}` | `{k}` | {body} | " + " | ".join(show(f) for f in
                  ("vgpr", "sgpr", "scratch", "lds", "loop", "waves")) + " |")
    return 1 if worse else 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("rev_a")
    ap.add_argument("rev_b", nargs="?", default=None)
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--only", default=".", metavar="REGEX", help="compare only the files whose name matches")
    ap.add_argument("--per-kernel", action="store_true", help="one row per kernel, with its resource figures")
    a = ap.parse_args()
    bad, hunks = 0, []
    with tempfile.TemporaryDirectory() as tmp:
        ca, cb = csrc_of(a.rev_a, tmp), csrc_of(a.rev_b, tmp)
        names = sorted({os.path.basename(p) for c in (ca, cb) for p in glob.glob(os.path.join(c, "kernels", "*.hip"))
                        if re.search(a.only, os.path.basename(p))})
        with cf.ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
            fa = {n: ex.submit(asm_lines, ca, n, tmp) for n in names}
            fb = {n: ex.submit(asm_lines, cb, n, tmp) for n in names}
            if a.per_kernel:
                return per_kernel(names, fa, fb)
            print(f"| file | asm lines {a.rev_a} | asm lines {a.rev_b or 'working tree'} | verdict |")
            print("|---|---:|---:|---|")
            for n in names:
                x, y = fa[n].result(), fb[n].result()
                if x is None or y is None:
                    verdict, hunk = "only in one revision", []
                elif x == y:
                    verdict, hunk = "identical", []
                else:
                    kernel, hunk = first_hunk(x, y)
                    verdict = f"DIFFERS, first in `{kernel}`"
                bad += verdict != "identical"
                print(f"| `{n}` | {len(x or [])} | {len(y or [])} | {verdict} |")
                hunks += [f"\n{n}: {verdict}"] + ["    " + l for l in hunk] if hunk else []
    print("\n".join(hunks))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
