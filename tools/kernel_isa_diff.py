#!/usr/bin/env python3
"""Compare the compiled gfx950 code of two source trees, function by function (no GPU; for relocations that must not change a kernel).

    python tools/kernel_isa_diff.py <old tree> <new tree>

Every file of each tree's dyglib_amd/_build.py SOURCES is compiled with that tree's CXXFLAGS plus `--cuda-device-only -S`.  The assembly is
split by function symbol; comments and the function numbers of local labels are dropped; what is left of each function and its kernel
descriptor's .amdhsa_ directives (registers, LDS, scratch) must be equal.  A symbol that left one file and appeared in another is compared across the two, so code may move.
"""
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys

RENAMED = {      # old name -> new name of a symbol that moved namespace or file
    "_ZN5dygnn4attn8cos_libmEf": "_ZN5dygnn7timeenc8cos_libmEf",
    # the element kernels of dygformer_train.hip and graphmixer_train.hip -> train_elements.h (a static copy per including source)
    "_ZN5dygnn5train15k_gelu_drop_fwdEPKflNS0_4DropEjPf": "_ZN5dygnn5trainL11k_gelu_dropEPKflNS0_4DropEjPf",
    "_ZN5dygnn5train15k_gelu_drop_bwdEPfPKflNS0_4DropEj": "_ZN5dygnn5trainL15k_gelu_drop_bwdEPfPKflNS0_4DropEj",
    "_ZN5dygnn5train14k_drop_add_fwdEPKfS2_lNS0_4DropEjPf": "_ZN5dygnn5trainL10k_drop_addEPKfS2_lNS0_4DropEjPf",
    "_ZN5dygnn5train10k_drop_bwdEPKflNS0_4DropEjPf": "_ZN5dygnn5trainL10k_drop_bwdEPKflNS0_4DropEjPf",
    "_ZN5dygnn3gmt15k_gmt_gelu_dropEPKfPflNS_5train4DropEj": "_ZN5dygnn5trainL11k_gelu_dropEPKflNS0_4DropEjPf",
    "_ZN5dygnn3gmt13k_gmt_hid_bwdEPfPKflNS_5train4DropEj": "_ZN5dygnn5trainL15k_gelu_drop_bwdEPfPKflNS0_4DropEj",
    "_ZN5dygnn3gmt9k_gmt_resEPKfS2_PflNS_5train4DropEj": "_ZN5dygnn5trainL10k_drop_addEPKfS2_lNS0_4DropEjPf",
    "_ZN5dygnn3gmt14k_gmt_drop_bwdEPKfPflNS_5train4DropEj": "_ZN5dygnn5trainL10k_drop_bwdEPKflNS0_4DropEjPf",
    # dygformer_train.hip's table kernel -> dygformer_generic.hip's one (k_cooc_lut is gone)
    "_ZN5dygnn5train9k_lut_fwdEPKfS2_S2_S2_iiPfS3_": "_ZN5dygnn12k_cooc_tableEPKfS1_S1_S1_iPfS2_",
}


def functions(tree):
    """{(symbol, source): (source, instruction text, .amdhsa_ text or None for a device function)} of one tree."""
    spec = importlib.util.spec_from_file_location("_b", os.path.join(tree, "dyglib_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)

    def asm(src):
        cmd = [b._hipcc(), *b.CXXFLAGS, "-I", b.INCLUDE, "--cuda-device-only", "-S", "-x", "hip", os.path.join(b.CSRC, src), "-o", "-"]
        return src, subprocess.run(cmd, capture_output=True, text=True, check=True).stdout

    out = {}
    with cf.ThreadPoolExecutor(max_workers=6) as ex:
        for src, text in ex.map(asm, b.SOURCES):
            for old, new in RENAMED.items():
                text = text.replace(old, new)
            text = re.sub(r";.*", "", text)                                 # comments
            text = re.sub(r"\.L(BB|JTI|tmp|func_(?:begin|end))\d+", r".L\1", text)      # .LBB12_3 -> .LBB_3: 12 counts the file's functions
            text = "\n".join(ln.strip() for ln in text.splitlines() if ln.strip())
            for name, body in re.findall(r"^\.type\s+(\S+),@function\n\1:\n(.*?)\n\.Lfunc_end:", text, re.M | re.S):
                code, _, desc = body.partition("\n.amdhsa_kernel ")      # a kernel's descriptor stands at the end of its body
                out[name, src] = (src, code, desc or None)
    return out


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    gone, come = {k[0]: k for k in old if k not in new}, {k[0]: k for k in new if k not in old}
    for name in set(gone) & set(come):      # the symbol moved to another file
        new[gone[name]] = new.pop(come[name])
    rows, bad = [], 0
    for key in sorted(set(old) | set(new)):
        name, o, n = key[0], old.get(key), new.get(key)
        if o is None or n is None:
            verdict = "only in " + ("new" if o is None else "old")
        else:
            verdict = " and ".join(w for w, i in (("instructions", 1), ("directives", 2)) if o[i] != n[i]) or "identical"
            verdict = verdict if verdict == "identical" else verdict + " differ"
        bad += verdict != "identical"
        rows.append((name, "kernel" if (o or n)[2] is not None else "function", o[0] if o else "-", n[0] if n else "-", verdict))
    print("| symbol | kind | old file | new file | result |\n|---|---|---|---|---|")
    for r in rows:
        print("| `%s` | %s | %s | %s | %s |" % r)
    kernels = sum(r[1] == "kernel" for r in rows)
    print("\n%d symbols (%d kernels, %d device functions), %d not identical" % (len(rows), kernels, len(rows) - kernels, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
