"""Compare two tools/kernel_resources.sh listings across the WP -> <Loop, N> renaming of the
vi_fused_kernel / vi_serve_kernel template arguments.

    tools/kernel_resources.sh OLD.so vi_ > old.txt; tools/kernel_resources.sh NEW.so vi_ > new.txt
    python tools/kernel_resources_diff.py old.txt new.txt

Kernel names are demangled (c++filt) and both spellings are rewritten to `<..., family, N>`;
prints the kernels whose vgpr / sgpr / scratch / lds line differs or that exist on one side only.
Exit status 0 when the two listings agree.
"""
import re
import subprocess
import sys

LOOPS = ["generic", "sa", "pair", "quad", "xyd_soa", "dk_soa", "wave", "xyd_x2", "xyd_x4", "xyd_pair2", "wave2", "band",
         "wave2n", "mix", "dk_1t", "dk_half", "dk_rows", "dk_rows16", "serve_ew", "serve_pair", "opts", "sweep",
         "sweep_pipe"]
CXXFILT = "c++filt"


def old_tag(wp: int, model: int):
    if wp == 0:
        return "generic", 0
    if wp > 0:
        return "wave", wp
    single = {-2: "xyd_x2", -4: "xyd_x4", -100: "dk_1t", -200: "dk_soa" if model else "xyd_soa", -600: "serve_ew",
              -601: "serve_pair", -800: "dk_rows", -801: "dk_rows16"}
    if wp in single:
        return single[wp], 0
    base = {3: "xyd_pair2", 4: "wave2", 5: "dk_half", 7: "wave2n", 9: "band", 10: "mix"}[-wp // 100]
    return base, -wp % 100


def canon(name: str) -> str:
    m = re.match(r"void mgdp::(vi_fused_kernel|vi_serve_kernel)<(\w+), (\d+), (\w+), (\d+), (.*)>\(", name)
    if not m:
        return name.split("(")[0]
    kern, t, model, slip, mapping, rest = m.groups()
    n = re.fullmatch(r"\(mgdp::Loop\)(\d+), (-?\d+)", rest)
    if n:
        fam, size = LOOPS[int(n.group(1))], int(n.group(2))
    else:
        fam, size = old_tag(int(rest), int(model))
    return f"{kern}<{t}, {model}, {slip}, {mapping}, {fam}, {size}>"


def load(path):
    rows = {}
    for line in open(path):
        res, mangled = line.rstrip("\n").rsplit("  ", 1)
        name = subprocess.run([CXXFILT, mangled.strip()], capture_output=True, text=True).stdout.strip()
        key = canon(name)
        assert key not in rows, key
        rows[key] = " ".join(res.split())
    return rows


if __name__ == "__main__":
    a, b = load(sys.argv[1]), load(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if a.get(k) != b.get(k):
            bad += 1
            print(f"{k}\n  old: {a.get(k)}\n  new: {b.get(k)}")
    print(f"{len(a)} kernels before, {len(b)} after, {bad} differ")
    sys.exit(1 if bad else 0)
