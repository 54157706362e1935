"""Compare two tools/kernel_resources.sh listings, kernel by kernel (keyed by the mangled name).

    tools/kernel_resources.sh OLD.so . > old.txt; tools/kernel_resources.sh NEW.so . > new.txt
    python tools/kernel_resources_diff.py old.txt new.txt

Prints the kernels whose vgpr / sgpr / scratch / lds line differs or that exist on one side only.
Exit status 0 when the two listings agree.
"""
import sys


def load(path):
    rows = {}
    for line in open(path):
        res, name = line.rstrip("\n").rsplit("  ", 1)
        assert name not in rows, name
        rows[name] = " ".join(res.split())
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
