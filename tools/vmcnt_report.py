"""Vector-memory operations and s_waitcnt vmcnt(N) of every loop of a kernel, in program order, from the -save-temps
assembly (csrc/build, `make asm`).

usage: python tools/vmcnt_report.py <mangled-name-substring> [listing.s] [--min-ops N]

A loop is a backward branch: the lines from the label it targets to the branch itself.  Per loop one line of tokens:
    L   a load  (buffer_load_* / global_load_* / flat_load_* / scratch_load_*)
    S   a store (the *_store_* forms)
    A   an atomic
    wN  s_waitcnt vmcnt(N)
    |   a basic-block label inside the loop
and, behind it, what the back edge carries: the waits between the last memory operation and the branch.  A small N there
means that the loop drains its own prefetch once per iteration -- the loads issued near the end of the body have to land
before the next iteration starts.  `steady` is the largest N in the loop (the lookahead the body was written for), `back edge`
the smallest N behind the last operation (None: no wait there).
"""
import os
import re
import sys

DEFAULT_LISTING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "depth_completion_mt_amd", "csrc", "build",
                               "dcmt-hip-amdgcn-amd-amdhsa-gfx950.s")

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_MEM = re.compile(r"^(buffer|global|flat|scratch)_(load|store|atomic)")


def function_body(text, key):
    """(mangled name, lines) of the first function whose mangled name contains key."""
    m = re.search(r"^(_Z\w*" + re.escape(key) + r"\w*):", text, re.M)
    if m is None:
        raise KeyError(f"no function matching {key!r}")
    end = text.find(".Lfunc_end", m.start())
    return m.group(1), text[m.start():end if end >= 0 else len(text)].split("\n")


def token(line):
    """The token of one instruction line, or None."""
    t = line.strip()
    if t.startswith("s_waitcnt"):
        m = _VMCNT.search(t)
        return f"w{m.group(1)}" if m else None
    m = _MEM.match(t)
    if m:
        return {"load": "L", "store": "S", "atomic": "A"}[m.group(2)]
    return None


def loops(lines):
    """Every backward branch of a function body as a dict: label, first / last line index, tokens, valu, branches, back_edge, steady, inner."""
    where = {}
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m:
            where[m.group(1)] = i
    spans = []
    for i, ln in enumerate(lines):
        m = _BRANCH.match(ln)
        if m and m.group(1) in where and where[m.group(1)] < i:
            spans.append((where[m.group(1)], i, m.group(1)))
    out = []
    for a, b, label in spans:
        toks, valu, branches = [], 0, 0
        for ln in lines[a + 1:b + 1]:
            if _LABEL.match(ln):
                toks.append("|")
                continue
            if not ln.startswith("\t"):
                continue
            t = ln.strip()
            if not t or t[0] in ".;":
                continue
            valu += t.startswith("v_")
            branches += t.startswith(("s_cbranch", "s_branch"))
            tk = token(ln)
            if tk:
                toks.append(tk)
        tail = []
        for tk in reversed(toks):
            if tk in ("L", "S", "A"):
                break
            if tk != "|":
                tail.append(int(tk[1:]))
        waits = [int(tk[1:]) for tk in toks if tk[0] == "w"]
        out.append({"label": label, "first": a, "last": b, "tokens": toks, "valu": valu, "branches": branches,
                    "back_edge": min(tail) if tail else None, "steady": max(waits) if waits else None,
                    "inner": sum(1 for a2, b2, _ in spans if a < a2 and b2 < b)})
    return out


def report(text, key, min_ops=1):
    name, lines = function_body(text, key)
    rows = [name]
    for lp in loops(lines):
        ops = sum(1 for tk in lp["tokens"] if tk in ("L", "S", "A"))
        if ops < min_ops:
            continue
        rows.append(f"loop {lp['label']}  lines {lp['first']}..{lp['last']}  VALU {lp['valu']}  branches {lp['branches']}  "
                    f"inner loops {lp['inner']}  ops {ops}  steady vmcnt {lp['steady']}  back edge vmcnt {lp['back_edge']}")
        rows.append("    " + " ".join(lp["tokens"]))
    return "\n".join(rows)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    min_ops = int(sys.argv[sys.argv.index("--min-ops") + 1]) if "--min-ops" in sys.argv else 1
    if "--min-ops" in sys.argv:
        args.remove(str(min_ops))
    if not args:
        sys.exit(__doc__)
    with open(args[1] if len(args) > 1 else DEFAULT_LISTING) as fh:
        print(report(fh.read(), args[0], min_ops))
