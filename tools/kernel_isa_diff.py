"""Per-kernel gfx950 disassembly diff of two builds of libullava_hip.so.

    python tools/kernel_isa_diff.py OLD.so NEW.so

Extracts every gfx950 code object from each library's .hip_fatbin section (one offload bundle per translation unit), disassembles them with
llvm-objdump, and compares the instruction text of every kernel present in OLD against the same kernel in NEW.  Kernel names are compared
demangled, by code object (the libraries must link the same objects in the same order) and without the parameter list, with a trailing
template argument `, 0>` of the new build removed, so a kernel that gained a defaulted template parameter is matched with its old
instantiation.  Prints one line per kernel that differs or disappeared, and a summary; exit status 1 when
any old kernel changed.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
OBJCOPY = os.path.join(ROCM, "llvm", "bin", "llvm-objcopy")
CXXFILT = next((p for p in (os.path.join(ROCM, "llvm", "bin", "llvm-cxxfilt"), "/usr/bin/c++filt") if os.path.exists(p)), "c++filt")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib: str, tmp: str):
    fat = os.path.join(tmp, os.path.basename(lib) + ".fatbin")
    subprocess.run([OBJCOPY, "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "discard.o")], check=True)
    data = open(fat, "rb").read()
    out = []
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + 1)
    return out


def kernels(lib: str):
    """demangled kernel name -> instruction text (addresses and encodings stripped)."""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib, tmp)):
            path = os.path.join(tmp, f"co{i}.o")
            open(path, "wb").write(co)
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], check=True, capture_output=True, text=True).stdout
            name, body = None, []
            for line in dis.splitlines():
                m = re.match(r"^(\S+):$", line.strip()) if line and not line.startswith((" ", "\t")) else None
                if line.endswith(">:") or m:
                    if name:
                        res[(i, name)] = body
                    name = line.strip().rstrip(":").strip("<>")
                    body = []
                elif name and line.strip():
                    # the trailing `// address: encoding <symbol+offset>` comment differs with the kernel's place in the object; branch
                    # operands are relative, so the instruction text alone is compared
                    body.append(re.sub(r"\s+", " ", line.split("//")[0].strip()))
            if name:
                res[(i, name)] = body
    keys = list(res)
    dem = subprocess.run([CXXFILT], input="\n".join(n for _, n in keys), capture_output=True, text=True, check=True).stdout.splitlines()
    return {(k[0], strip_params(d)): res[k] for k, d in zip(keys, dem)}


def strip_params(name: str) -> str:
    """`void ns::f<1, 8>(int, ...)` -> `ns::f<1, 8>` (the kernels here are told apart by their template arguments)."""
    depth, i = 0, len(name)
    for j in range(len(name) - 1, -1, -1):
        c = name[j]
        if c == ")":
            depth += 1
        elif c == "(":
            depth -= 1
            if depth == 0:
                i = j
                break
    head = name[:i]
    return head.split(" ", 1)[1] if head.startswith("void ") else head


def norm(key):
    return (key[0], re.sub(r", (\(\w+\))?0>$", ">", key[1]))


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    new_n = {}
    for k, v in new.items():
        new_n.setdefault(norm(k), v)
        new_n[k] = v
    changed = missing = 0
    for k, v in sorted(old.items()):
        w = new_n.get(k, new_n.get(norm(k)))
        if w is None:
            missing += 1
            print("MISSING", *k)
        elif w != v:
            changed += 1
            print("CHANGED", *k)
    print(f"{len(old)} kernels in old, {len(new)} in new, {len(set(new) - set(old))} new names; {changed} changed, {missing} missing")
    sys.exit(1 if changed or missing else 0)


if __name__ == "__main__":
    main()
