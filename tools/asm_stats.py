"""Per-kernel code statistics of a hipcc --cuda-device-only -S listing:
instruction count, VGPR/SGPR counts, LDS bytes (.group_segment_fixed_size)
and scratch bytes (.private_segment_fixed_size). Used to check that a source
change leaves a hot kernel's code unchanged (e.g. a new template instance
beside it).  Usage: python tools/asm_stats.py file.s [file.s ...]
"""
import re
import sys

# the fields of a kernel's entry in the listing's amdhsa.kernels metadata
META = {"lds": "group_segment_fixed_size", "scratch": "private_segment_fixed_size", "sgpr": "sgpr_count",
        "vgpr": "vgpr_count"}


def stats(path):
    text = open(path).read().splitlines()
    out, cur, n = {}, None, 0
    for line in text:
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur, n = m.group(1), 0
            continue
        if cur and line.startswith("\ts_endpgm"):
            out[cur] = {"insts": n + 1}
            cur = None
            continue
        if cur and line.startswith("\t") and not line.startswith("\t.") and not line.strip().startswith(";"):
            n += 1
    # amdhsa.kernels: one list item per kernel ("  - .agpr_count: ...", its own lists indented deeper)
    for entry in re.split(r"\n  - ", "\n".join(text)):
        name = re.search(r"\.name:\s+(_Z\S+)", entry)
        if not name or ".vgpr_count:" not in entry:
            continue
        for key, field in META.items():
            m = re.search(r"\.%s:\s+(\d+)" % field, entry)
            if m:
                out.setdefault(name.group(1), {})[key] = int(m.group(1))
    return out


if __name__ == "__main__":
    for p in sys.argv[1:]:
        for k, v in sorted(stats(p).items()):
            print(f"{p.split('/')[-1]:10s} {v.get('insts', 0):6d} insts  v{v.get('vgpr', 0):4d} s{v.get('sgpr', 0):4d}"
                  f"  lds{v.get('lds', 0):6d}  scratch{v.get('scratch', 0):4d}  {k}")
