"""Register budget of the kernels TCL, CAWN, TGAT and GraphMixer share (encoder_block.h, train_rows.h, colsum.h), as hipcc reports it
(-Rpass-analysis=kernel-resource-usage), on the pattern of test_dygformer_resources_cpu.py.

The inference block tail k_encoder_post<NT, MT> replaced k_tcl_post and k_cawn_post<NT, MT>.  Those had, compiled with the build's flags:

    k_tcl_post         95 VGPRs  2 waves/SIMD          k_cawn_post<5, 2>   76 VGPRs  3 waves/SIMD
    k_cawn_post<4, 4> 100 VGPRs  2 waves/SIMD          k_cawn_post<8, 2>  100 VGPRs  2 waves/SIMD

and no scratch and no spills; every shared instance is held to that, in both files that launch it.  The row-wise training kernels and the
wave-per-column column-sum finish replaced per-backbone copies that all ran at 8 waves/SIMD (22-38 VGPRs) without scratch; every file that
instantiates one is held to that too.  The device code is compiled with the build's own flags; no GPU is needed."""
import concurrent.futures as cf
import functools
import re
import subprocess
import tempfile

from dyglib_amd import _build

SOURCES = ["tcl.hip", "cawn.hip", "tcl_train.hip", "cawn_train.hip", "tgat_train.hip", "graphmixer_train.hip"]
FIELDS = r"VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]"


def _remarks(src, tmp):
    cmd = [_build._hipcc(), *_build.CXXFLAGS, "-I", _build.INCLUDE, "--cuda-device-only", "-c",
           f"{_build.CSRC}/{src}", "-o", f"{tmp}/{src}.o", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@functools.lru_cache(maxsize=None)
def _resource_usage():
    """{source: {mangled kernel name: {field: value}}}"""
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(len(SOURCES)) as ex:
        logs = list(ex.map(lambda s: _remarks(s, tmp), SOURCES))
    usage = {}
    for src, log in zip(SOURCES, logs):
        per, name = usage.setdefault(src, {}), None
        for line in log.splitlines():
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                per[name] = {}
                continue
            m = re.search(rf"remark:\s+({FIELDS}): (\d+)", line)
            if m and name:
                per[name][m.group(1)] = int(m.group(2))
    return usage


def _one(src, tag):
    hits = {k: v for k, v in _resource_usage()[src].items() if tag in k}
    assert len(hits) == 1, (src, tag, sorted(_resource_usage()[src]))
    return next(iter(hits.values()))


# (source, <NT, MT>) -> waves/SIMD of the kernel it replaced
POST_FLOOR = {("tcl.hip", (4, 4)): 2, ("cawn.hip", (4, 4)): 2, ("cawn.hip", (5, 2)): 3, ("cawn.hip", (8, 2)): 2}


def test_the_shared_post_kernel_keeps_the_occupancy_of_the_kernels_it_replaced():
    for (src, (nt, mt)), floor in POST_FLOOR.items():
        u = _one(src, f"k_encoder_postILi{nt}ELi{mt}EE")
        print(f"{src} k_encoder_post<{nt}, {mt}>:", u, "floor:", floor)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (src, nt, mt, u)
        assert u["Occupancy [waves/SIMD]"] >= floor, (src, nt, mt, u)
    # nothing else instantiates it: a new instance gets a line here with its own floor
    for src, per in _resource_usage().items():
        assert sum("k_encoder_post" in k for k in per) == sum(s == src for s, _ in POST_FLOOR), (src, sorted(per))


SHARED = ("k_res_ln", "k_res_ln_bwd", "k_row_drop", "k_hid_bwd", "k_time_part", "k_time_fin", "k_colsum_fin")
# the widths (columns per lane) each file instantiates the LayerNorm pair at: one per caller, so none gets wider loops than its own copy had
LN_WIDTHS = {"tcl_train.hip": {"k_res_lnILi4EE", "k_res_ln_bwdILi4EE"}, "cawn_train.hip": {"k_res_lnILi8EE", "k_res_ln_bwdILi8EE"},
             "tgat_train.hip": {"k_res_ln_bwdILi5EE"}, "graphmixer_train.hip": set()}


def test_the_shared_row_kernels_run_at_full_occupancy_without_scratch():
    for src, widths in LN_WIDTHS.items():
        # Itanium mangling is <length><name>: k_res_ln does not match k_res_ln_bwd, nor k_colsum_fin the one-thread-per-column k_tt_colsum_fin
        found = {k: v for k, v in _resource_usage()[src].items() if any(f"L{len(n)}{n}" in k for n in SHARED)}
        for k, u in found.items():
            print(src, k, u)
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (src, k, u)
            assert u["Occupancy [waves/SIMD]"] == 8, (src, k, u)
        assert found, src
        ln = {m.group(1) for m in (re.search(r"\d+(k_res_ln(?:_bwd)?ILi\d+EE)", k) for k in found) if m}
        assert ln == widths, (src, ln)
