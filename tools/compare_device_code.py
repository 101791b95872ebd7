"""Compare the gfx950 device code of two builds of the kernel library, kernel by kernel.

    python tools/compare_device_code.py OLD/libneube_hip.so NEW/libneube_hip.so

Prints the symbols only one library has, the kernels whose instruction text differs and the kernels whose register / spill /
scratch / LDS figures differ; exit status 1 if there are any.  Instruction text = the disassembly (build.disassembly) without
addresses, without the encoding column and without the padding behind a kernel's last s_endpgm.  For changes that move or
regroup kernel source without meaning to change what the compiler makes of it."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from brushstroke_engine_amd import build  # noqa: E402


def kernels(lib):
    """{symbol: [instruction text, ...]} of every function in the library's code objects."""
    out = {}
    dis = build.disassembly(lib)
    for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <[^>]+>:\n|\Z)", dis, flags=re.M | re.S):
        ins = [re.sub(r"\s+", " ", line.split("//")[0].strip()) for line in m.group(2).split("\n")]
        ins = [i for i in ins if i]
        ends = [k for k, i in enumerate(ins) if i.startswith("s_endpgm")]
        if ends:
            ins = ins[:ends[-1] + 1]
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = ins
    return out


def main(old, new):
    ko, kn = kernels(old), kernels(new)
    ro, rn = build.kernel_resources(old), build.kernel_resources(new)
    bad = 0
    for name in sorted(set(ko) ^ set(kn)):
        print(("only in " + (old if name in ko else new)) + ": " + name)
        bad += 1
    for name in sorted(set(ko) & set(kn)):
        if ko[name] != kn[name]:
            first = next((k for k, (a, b) in enumerate(zip(ko[name], kn[name])) if a != b), min(len(ko[name]), len(kn[name])))
            print(f"code differs: {name}: {len(ko[name])} / {len(kn[name])} instructions, first difference at instruction {first}")
            bad += 1
    for name in sorted(set(ro) | set(rn)):
        if ro.get(name) != rn.get(name):
            print(f"resources differ: {name}: {ro.get(name)} / {rn.get(name)}")
            bad += 1
    print(f"{len(kn)} functions, {len(rn)} kernels with metadata compared; {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
