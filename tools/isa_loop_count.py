#!/usr/bin/env python3
"""Static instruction classes of one kernel's loop in a hipcc -S listing: from a label to the end of the function.
usage: tools/isa_loop_count.py <listing.s> <kernel name substring> [label, e.g. .LBB0_43; default: the kernel's first
loop that has inner loops]"""
import re
import sys


def main():
    path, kernel = sys.argv[1:3]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and kernel in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    if len(sys.argv) > 3:
        first = next(i for i in range(start, end) if lines[i].startswith(sys.argv[3] + ":"))
    else:       # the first loop that has inner loops: k_find_sn's position loop
        first = next(i for i in range(start, end) if "=>This Loop Header: Depth=1" in lines[i])
    label = lines[first].split(":")[0]
    ops = [l.split()[0] for l in lines[first:end] if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
    dpp = [l for l in lines[first:end] if l.startswith("\t") and re.search(r"quad_perm|row_|wave_", l)]
    mem = sum(o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_", "s_load", "s_buffer_load")) for o in ops)
    n = lambda pre: sum(o.startswith(pre) for o in ops)
    print(f"{lines[start].split(':')[0]}  {label} .. end of function")
    print(f"  v_* {n('v_')}  s_* {n('s_') - sum(o.startswith(('s_load', 's_buffer_load')) for o in ops)}  memory {mem}")
    print(f"  v_cmp {n('v_cmp')}  v_cndmask {n('v_cndmask')}  v_min/v_max {n('v_min') + n('v_max')}  dpp {len(dpp)}"
          f"  of which row_ror {sum('row_ror' in l for l in dpp)}")


if __name__ == "__main__":
    main()
