"""Compare the gfx950 machine code of two library builds, function by function.  Offline, no GPU.

    python tools/kernel_code_diff.py OLD.so NEW.so [--rename REGEX REPL]...

Each library's code objects are extracted as tools/kernel_resources.sh does and disassembled with
llvm-objdump; addresses, encodings and symbol names are stripped (branch operands are relative), and
the instruction text of every function is compared under its mangled name.  --rename rewrites OLD's
names first (re.sub), for functions that changed name on purpose.  A plain textual comparison of
two listings: prints the functions that differ or exist on one side only; exit status 0 when none.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")


def code_objects(lib, d):
    """The gfx950 code objects of the fatbin: one offload bundle per translation unit, CCOB-compressed or plain."""
    subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={d}/fat.bin", lib], check=True)
    b = open(f"{d}/fat.bin", "rb").read()
    starts, i = [], 0
    while True:
        j = min([x for x in (b.find(b"CCOB", i), b.find(b"__CLANG_OFFLOAD_BUNDLE__", i)) if x >= 0], default=-1)
        if j < 0:
            break
        starts.append(j)
        i = j + 4
    for n, s in enumerate(starts):
        if b[s:s + 4] == b"CCOB":
            ver = struct.unpack("<H", b[s + 4:s + 6])[0]
            size = struct.unpack("<Q", b[s + 8:s + 16])[0] if ver >= 3 else struct.unpack("<I", b[s + 8:s + 12])[0]
        else:
            size = (starts[n + 1] if n + 1 < len(starts) else len(b)) - s
        f = f"{d}/b{n}.bin"
        open(f, "wb").write(b[s:s + size])
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={f}", f"--output={f}.co", "--unbundle", "--allow-missing-bundles"],
                       stderr=subprocess.DEVNULL)
        if os.path.exists(f + ".co") and os.path.getsize(f + ".co"):
            yield f + ".co"


def functions(lib):
    """{mangled name: instruction text without addresses, encodings or symbol references}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True,
                                 capture_output=True, text=True).stdout
            name = None
            for line in txt.splitlines():
                m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1)
                    assert name not in out, name
                    out[name] = []
                elif name and line.startswith("\t") and line.strip() != "...":  # "...": zero padding up to the next symbol
                    out[name].append(line.split("//")[0].strip())
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append((args[i + 1], args[i + 2]))
        del args[i:i + 3]
    old, new = functions(args[0]), functions(args[1])
    renamed = {}
    for k, v in old.items():
        k2 = k
        for pat, repl in renames:
            k2 = re.sub(pat, repl, k2)
        if k2 != k:
            print(f"renamed: {k}\n      -> {k2}")
        assert k2 not in renamed, k2
        renamed[k2] = v
    bad = 0
    for k in sorted(set(renamed) | set(new)):
        a, b = renamed.get(k), new.get(k)
        if a != b:
            bad += 1
            print(f"{'differs' if a and b else 'only in ' + ('old' if a else 'new')}: {k}")
    print(f"{len(old)} functions before, {len(new)} after, {sum(len(v) for v in new.values())} instructions after, "
          f"{bad} differ or are on one side only")
    sys.exit(1 if bad else 0)
