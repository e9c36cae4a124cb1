#!/usr/bin/env python3
"""Compare the device code of two builds of libafx.so (or libafx_dbg.so) kernel by kernel.

    python tools/kernel_diff.py OLD.so NEW.so [--exports]

For every kernel symbol of either library: the resource figures of the code-object metadata (VGPRs, AGPRs, SGPRs,
scratch bytes, static LDS) side by side, and whether the disassembled text is the same once addresses and encodings
are dropped.  A kernel that differs is listed with its instruction count in both.  --exports also compares the
exported afx_* symbols.  Exit status 0: same kernel set, same figures, same text everywhere.

Needs only the LLVM tools of the ROCm installation (ROCM_PATH, default /opt/rocm); runs without a GPU.
"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    """The gfx code objects of every translation unit linked into `lib`, as files."""
    fat = os.path.join(tmp, "fatbin")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "stripped"))
    data = open(fat, "rb").read()
    out = []
    for m in re.finditer(re.escape(MAGIC), data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        p = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "amdgcn" in triple and size:
                path = os.path.join(tmp, "co%d.elf" % len(out))
                open(path, "wb").write(data[base + off:base + off + size])
                out.append(path)
    return out


def kernels(lib):
    """{kernel symbol: (figures dict, [normalised instruction lines])}"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            figs = {}
            notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
            for item in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
                f = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)\s*$", item, flags=re.M))
                if "symbol" in f:
                    figs[f["symbol"].strip("'")[:-3]] = {k: int(f[k]) for k in FIELDS if k in f}
            text = {}
            sym = None
            for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
                if m:
                    sym = m.group(1)
                    text[sym] = []
                    continue
                if sym is None:
                    continue
                ins = line.split("//")[0].strip()
                if ins:
                    text[sym].append(re.sub(r"\s+", " ", ins))
            for lines in text.values():          # alignment padding behind a kernel's last instruction
                while lines and lines[-1].split()[0] in ("s_nop", "s_code_end"):
                    lines.pop()
            for name, f in figs.items():
                res[name] = (f, text.get(name, []))
    return res


def exports(lib):
    syms = set()
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", lib).splitlines():
        p = line.split()
        if len(p) >= 8 and p[6] != "UND" and p[7].startswith("afx_") and p[3] == "FUNC":
            syms.add(p[7])
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--exports", action="store_true")
    ap.add_argument("--table", action="store_true", help="print the figures of every kernel, not only of those that differ")
    a = ap.parse_args()
    bad = 0
    if a.exports:
        eo, en = exports(a.old), exports(a.new)
        print("exported afx_* functions: old %d, new %d, %s" % (len(eo), len(en), "identical" if eo == en else "DIFFERENT"))
        for s in sorted(eo ^ en):
            print("  only in %s: %s" % ("old" if s in eo else "new", s))
        bad += eo != en
    ko, kn = kernels(a.old), kernels(a.new)
    print("kernel symbols: old %d, new %d, %s" % (len(ko), len(kn), "same set" if set(ko) == set(kn) else "DIFFERENT sets"))
    for s in sorted(set(ko) ^ set(kn)):
        print("  only in %s: %s" % ("old" if s in ko else "new", s))
    bad += set(ko) != set(kn)
    nfig = ntext = 0
    if a.table:
        print("figures (vgpr agpr sgpr scratch lds), old | new, and instruction count:")
    for s in sorted(set(ko) & set(kn)):
        fo, to = ko[s]
        fn, tn = kn[s]
        vo, vn = [fo.get(k, -1) for k in FIELDS], [fn.get(k, -1) for k in FIELDS]
        same_t = to == tn
        if a.table:
            print("  %s | %s  %6d %s %s" % (" ".join("%4d" % v for v in vo), " ".join("%4d" % v for v in vn), len(tn),
                                            "identical" if same_t and vo == vn else "DIFFERS", s))
        if vo != vn:
            nfig += 1
            print("  FIGURES differ: %s: old %s new %s" % (s, vo, vn))
        if not same_t:
            ntext += 1
            print("  TEXT differs: %s: %d instructions old, %d new" % (s, len(to), len(tn)))
    n = len(set(ko) & set(kn))
    print("resource figures: %d of %d kernels equal" % (n - nfig, n))
    print("disassembly: %d of %d kernels identical" % (n - ntext, n))
    return 1 if (bad or nfig or ntext) else 0


if __name__ == "__main__":
    sys.exit(main())
