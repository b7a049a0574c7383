"""Builds oracle/_ref/libdcmt_ref.so from the reference's own sources (test infrastructure, never shipped).

The reference's three self-contained files are compiled in place and unmodified against the stand-in headers of this
directory.  Functions that live in files which cannot be compiled whole are cut out, at build time, by signature and
brace matching into oracle/_ref/*.inc and included by cuts.cpp.  Nothing this writes is tracked by git.

The reference checkout is looked for in $DCMT_REFERENCE_DIR, else in the directory `reference` next to this repository.

    python oracle/refbuild/build_ref.py          # build (fails loudly if a signature is not found exactly once)
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB_NAME = "libdcmt_ref.so"

WHOLE_FILES = ("src/DC_lidar_only/img_completion.cpp",
               "src/DC_lidar_camera/img_completion_lc.cpp",
               "src/DC_lidar_camera/slic.cpp")
# (source file, output .inc, definitions to cut: kind and name, in the order they are written out)
CUTS = (
    ("src/DC_lidar_only/main.cpp", "eval_lo.inc", (("void", "evaluate_performance"),)),
    ("src/DC_lidar_camera/main_lc.cpp", "eval_lc.inc", (("void", "evaluate_performance"),)),
    ("src/DC_stereo_lidar/main_sl.cpp", "stereo_sl.inc", (("struct", "EntryType"),
                                                         ("void", "calculateMeasuementDerivatives"),
                                                         ("bool", "calculateObservationDerivatives"),
                                                         ("void", "optimize_IG"),
                                                         ("void", "get_initial_disparity"),
                                                         ("void", "retrieve_optimized_depth"),
                                                         ("void", "evaluate_performances"))),
)
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w"]


class CutError(RuntimeError):
    pass


def reference_dir() -> str | None:
    """The reference checkout, or None where there is none."""
    d = os.environ.get("DCMT_REFERENCE_DIR") or os.path.join(os.path.dirname(ROOT), "reference")
    return d if os.path.isdir(os.path.join(d, "src")) else None


def lib_path() -> str:
    return os.path.join(OUT_DIR, LIB_NAME)


def code_mask(text: str) -> list[bool]:
    """True for every character that is program text proper: not in a comment, a string or a character literal."""
    mask = [True] * len(text)
    i, n = 0, len(text)
    while i < n:
        two = text[i:i + 2]
        if two == "//":
            j = text.find("\n", i)
            j = n if j < 0 else j
        elif two == "/*":
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
        elif text[i] in "\"'":
            quote, j = text[i], i + 1
            while j < n and text[j] != quote:
                j += 2 if text[j] == "\\" else 1
            j = min(j + 1, n)
        else:
            i += 1
            continue
        for k in range(i, j):
            mask[k] = False
        i = j
    return mask


def cut_definition(text: str, kind: str, name: str, where: str = "") -> str:
    """The one definition `kind name ... { ... }` of the file, found by its signature and matched braces."""
    mask = code_mask(text)
    tail = r"\s*\(" if kind != "struct" else r"\b"
    found = []
    for m in re.finditer(rf"^[ \t]*{re.escape(kind)}\s+{re.escape(name)}{tail}", text, flags=re.M):
        if not mask[m.end() - 1]:
            continue
        k = m.end()
        while k < len(text) and not (mask[k] and text[k] in "{;"):
            k += 1
        if k < len(text) and text[k] == "{":          # a definition, not a declaration
            found.append((m.start(), k))
    if len(found) != 1:
        raise CutError(f"{where}: expected exactly one definition of `{kind} {name}`, found {len(found)}")
    start, k = found[0]
    depth = 0
    while k < len(text):
        if mask[k]:
            if text[k] == "{":
                depth += 1
            elif text[k] == "}":
                depth -= 1
                if depth == 0:
                    break
        k += 1
    if depth != 0:
        raise CutError(f"{where}: braces of `{kind} {name}` do not close")
    end = k + 1
    if kind == "struct":
        while end < len(text) and text[end] in " \t\r\n":
            end += 1
        if end >= len(text) or text[end] != ";":
            raise CutError(f"{where}: `struct {name}` does not end in `;`")
        end += 1
    return text[start:end] + "\n"


def build(ref: str | None = None, out_dir: str = OUT_DIR, cxx: str | None = None) -> str:
    ref = ref or reference_dir()
    if ref is None:
        raise FileNotFoundError("no reference checkout (set DCMT_REFERENCE_DIR)")
    os.makedirs(out_dir, exist_ok=True)
    for rel, inc, defs in CUTS:
        with open(os.path.join(ref, rel), encoding="utf-8", errors="replace") as f:
            text = f.read()
        parts = [cut_definition(text, kind, name, rel) for kind, name in defs]
        with open(os.path.join(out_dir, inc), "w", encoding="utf-8") as f:
            f.write("\n".join(parts))
    so = os.path.join(out_dir, LIB_NAME)
    cmd = [cxx or os.environ.get("CXX", "g++"), *CXXFLAGS,
           "-I", HERE, "-I", out_dir, "-I", os.path.join(ref, "src", "DC_lidar_camera"),
           "-o", so, os.path.join(HERE, "driver.cpp"), os.path.join(HERE, "cuts.cpp"),
           *[os.path.join(ref, rel) for rel in WHOLE_FILES]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building the reference failed:\n" + " ".join(cmd) + "\n" + r.stderr[-4000:])
    return so


if __name__ == "__main__":
    print(build())
    sys.exit(0)
