#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every kernel source between two revisions (no GPU needed).

    python scripts/isa_diff.py REV_A [REV_B] [-j N]

Each csrc/kernels/*.hip is compiled to assembly (isa_census.compile_asm: the library's flags) once
from REV_A's csrc/ and once from REV_B's (default: the working tree); revisions are unpacked with
`git archive` into a temporary directory.  Lines that differ between two compiles of the same
source (.file, .ident, comments, the per-compile __hip_cuid_ symbol) are dropped; the rest must be
equal line for line.  Prints one markdown table row per file and, for a file that differs, the
kernel holding the first difference and that hunk.  Exit status 1 if any file differs.
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("rev_a")
    ap.add_argument("rev_b", nargs="?", default=None)
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--only", default=".", metavar="REGEX", help="compare only the files whose name matches")
    a = ap.parse_args()
    bad, hunks = 0, []
    with tempfile.TemporaryDirectory() as tmp:
        ca, cb = csrc_of(a.rev_a, tmp), csrc_of(a.rev_b, tmp)
        names = sorted({os.path.basename(p) for c in (ca, cb) for p in glob.glob(os.path.join(c, "kernels", "*.hip"))
                        if re.search(a.only, os.path.basename(p))})
        with cf.ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
            fa = {n: ex.submit(asm_lines, ca, n, tmp) for n in names}
            fb = {n: ex.submit(asm_lines, cb, n, tmp) for n in names}
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
