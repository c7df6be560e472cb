"""Code-object resources of every kernel of two builds of libpinn_hip.so, side by side, from the builds' own logs.

    make -C pinn_elastodynamics_amd/csrc -j16 hip > new.log 2>&1          (in each tree; the Makefile passes -Rpass-analysis=kernel-resource-usage)
    python tools/kernel_resources.py parent.log new.log > profiles/stream_sets_kernel_resources.txt

Needs no GPU.  Prints one line per kernel symbol of the first build that differs in the second (none expected from an additive change),
the kernels only the second build has, and exits 1 if a kernel of the first build changed or disappeared."""
import re
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?:\[[^\]]+\])?):\s*(\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[key] = val
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    print(f"kernels: {len(a)} in {sys.argv[1]}, {len(b)} in {sys.argv[2]}")
    print("fields compared: " + ", ".join(FIELDS))
    bad = 0
    for name in sorted(a):
        if name not in b:
            print(f"MISSING  {name}")
            bad += 1
        elif a[name] != b[name]:
            diff = {k: (a[name].get(k), b[name].get(k)) for k in FIELDS if a[name].get(k) != b[name].get(k)}
            print(f"CHANGED  {name}  {diff}")
            bad += 1
    print(f"kernels of the first build with changed resources: {bad}")
    new = sorted(n for n in b if n not in a)
    print(f"kernels only in the second build: {len(new)}")
    for name in new:
        print("NEW      " + name + "  " + "  ".join(f"{k}={b[name].get(k)}" for k in FIELDS))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
