"""Instruction census of one kernel in a hipcc -S listing: counts by class, and how many SGPR-spill lane ops / waits sit
between the first and the last MFMA.  usage: python tools/kasm.py file.s <substring of the mangled name>

Comparison of two listings of the same source (hipcc <product flags> -S --cuda-device-only), the gate of a refactor that
must not move device code:  python tools/kasm.py --diff parent.s change.s [parent2.s change2.s ...]
Per kernel (every symbol with an .amdhsa_kernel descriptor) it compares the instruction stream -- `;` comments dropped, local
labels renumbered in order of appearance, so the order of the symbols in the file does not matter -- and the .amdhsa_*
descriptor lines (registers, LDS, scratch).  Prints `identical N of M` per pair, the name and the two instruction counts of
every kernel that differs, and exits 1 when one differs or is missing on either side."""
import re
import sys


def kernel_body(path, sub):
    lines = open(path).read().split("\n")
    start = [i for i, l in enumerate(lines) if l.startswith("_Z") and sub in l and l.rstrip().split(":")[0].endswith(("i", "s", "l"))
             or (l.startswith("_Z") and sub in l and ": " in l)]
    if not start:
        raise SystemExit("no kernel matches %r" % sub)
    i = start[0]
    j = i
    while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
        j += 1
    return lines[i], lines[i + 1:j]


def kernels(path):
    """{kernel symbol: (normalised instruction stream, instruction count, descriptor lines)} of a listing"""
    lines = [l.split(";")[0].rstrip() for l in open(path).read().split("\n")]
    desc, i = {}, 0
    while i < len(lines):
        if lines[i].strip().startswith(".amdhsa_kernel "):
            name = lines[i].split()[1]
            j = i + 1
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[name] = [" ".join(l.split()) for l in lines[i + 1:j] if l.strip()]
            i = j
        i += 1
    starts = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":") and l[:-1] in desc}
    out = {}
    for name, d in desc.items():
        if name not in starts:
            raise SystemExit("%s: descriptor of %s without a body" % (path, name))
        labels, stream, count = {}, [], 0
        renumber = lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels))
        for l in lines[starts[name] + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            s = " ".join(l.split())
            is_label = s.startswith(".L") and s.endswith(":")
            if not s or (s.startswith(".") and not is_label):
                continue
            count += not is_label
            stream.append(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", renumber, s))
        out[name] = (stream, count, d)
    return out


def diff(parent, change):
    a, b = kernels(parent), kernels(change)
    names = sorted(set(a) | set(b))
    same = 0
    for n in names:
        if n not in a or n not in b:
            print("  missing in %s: %s" % ("parent" if n not in a else "change", n))
        elif a[n][0] == b[n][0] and a[n][2] == b[n][2]:
            same += 1
        else:
            what = "instructions" if a[n][0] != b[n][0] else "descriptor"
            print("  differs (%s): %s  %d -> %d instructions" % (what, n, a[n][1], b[n][1]))
    print("%s: identical %d of %d" % (change, same, len(names)))
    return same == len(names)


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        files = sys.argv[2:]
        if not files or len(files) % 2:
            raise SystemExit(__doc__)
        ok = [diff(files[k], files[k + 1]) for k in range(0, len(files), 2)]
        sys.exit(0 if all(ok) else 1)
    name, body = kernel_body(sys.argv[1], sys.argv[2])
    ins = [l.strip().split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    cnt = {}
    for k in ins:
        cnt[k] = cnt.get(k, 0) + 1
    mf = [i for i, l in enumerate(body) if "v_mfma" in l]
    inside = body[mf[0]:mf[-1]] if mf else []
    c = lambda ls, k: sum(1 for l in ls if k in l)
    print(name.split(":")[0][:100])
    print("instructions %d  mfma %d  ds_read %d  global_load %d  global_store %d  s_load %d  scratch %d" % (
        len(ins), c(body, "v_mfma"), c(body, "ds_read") + c(body, "ds_load"), c(body, "global_load"), c(body, "global_store"),
        c(body, "s_load"), c(body, "scratch_")))
    print("lane spill ops total %d, between first and last MFMA %d; s_waitcnt inside %d; valu inside %d" % (
        c(body, "v_readlane") + c(body, "v_writelane"), c(inside, "v_readlane") + c(inside, "v_writelane"),
        c(inside, "s_waitcnt"), sum(1 for l in inside if re.match(r"\s+v_(?!mfma)", l))))
