"""Compare the kernels of two gfx950 code objects instruction by instruction, mangled names aside: the check that a change to a shared
header left every existing kernel as it was.  Works without a GPU.
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -c dcmt.hip -o new.co          (and the same in the other tree: old.co)
    python tools/diff_kernels.py old.co new.co [--show NAME]
An object that is an offload bundle is unbundled first.  Kernels are matched by demangled name without the parameter list, after the
renamings in RENAMED (a template parameter that changed its type or gained a defaulted sibling).  Not compared: the padding behind
s_endpgm, and the literal of the s_add_u32 behind s_getpc_b64 (the distance to a constant table, which moves with the code in front).
Prints the kernels that differ, those that are new, and the counts; exit status 1 if an existing kernel differs or is missing."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
# (pattern, replacement) applied to the demangled names of BOTH objects
RENAMED = [
    (r"k_local<(\d+), (\d+), (\d+), (true|false)>", lambda m: f"k_local<{m[1]}, {m[2]}, {m[3]}, {1 if m[4] == 'true' else 0}>"),   # bool BLUR -> a kind
    (r"k_post_v1<(\d+), (\d+), false>", r"k_post_v1<\1, \2>"),                                                                    # + bool VALID = false
    (r"k_gauss5<false, false>", "k_gauss5"),                                                                                      # + <VALID, INVERT>
]


def elf_of(path, tmp):
    with open(path, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return path
    out = os.path.join(tmp, os.path.basename(path) + ".elf")
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={path}",
                    f"--output={out}"], check=True)
    return out


def kernels(path):
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    out, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name and line.strip():
            ins = re.sub(r"//.*$", "", line).strip()
            out[name].append(re.sub(r"<[^>]*>", "<sym>", ins))          # branch targets carry the kernel's own name
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"\bvoid ", "", d)
        for pat, rep in RENAMED:
            d = re.sub(pat, rep, d)
        d = re.sub(r"\(.*$", "", d)
        body = out[n]
        if "s_endpgm" in body:
            body = body[:len(body) - body[::-1].index("s_endpgm")]
        for i in range(1, len(body)):
            if body[i - 1].startswith("s_getpc_b64") and body[i].startswith("s_add_u32"):
                body[i] = re.sub(r"0x[0-9a-f]+$", "<pcrel>", body[i])
        res[d] = body
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show = sys.argv[sys.argv.index("--show") + 1] if "--show" in sys.argv else None
    if show:
        args.remove(show)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(elf_of(args[0], tmp)), kernels(elf_of(args[1], tmp))
    same = bad = 0
    for k, v in a.items():
        if k not in b:
            print("MISSING in the new object:", k)
            bad += 1
        elif v == b[k]:
            same += 1
        else:
            bad += 1
            print(f"DIFFERS: {k}: {len(v)} -> {len(b[k])} instructions")
        if show and show in k and k in b:
            print("\n".join(difflib.unified_diff(v, b[k], lineterm="", n=1)))
    new = [k for k in b if k not in a]
    print(f"{same} kernels identical, {bad} differ or are missing, {len(new)} new:")
    for k in new:
        print(f"    {k}: {len(b[k])} instructions")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
