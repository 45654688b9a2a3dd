"""Register budget of the fused DyGFormer kernels, as hipcc reports it (-Rpass-analysis=kernel-resource-usage).

DESIGN §4.3: the pooled product kernel of the headline shape, k_dygformer_fused3<4, false, 8, 1>, uses no scratch memory, and the
128-token shape <8, false, 8, 1> spills no more than the 2 VGPRs of the per-token form it replaces (outside the loops).  Both figures
lean on two values being formed where they are used instead of being kept alive through the layer loop (the empty `asm` statements in
the kernel), which a compiler update may undo: this test says so at build time.  The training forward and the two backward kernels are
held to the scratch and spill figures they had before the kernels were split into files of their own.  The device code is compiled with
the build's own flags; no GPU is needed."""
import concurrent.futures as cf
import functools
import re
import subprocess
import tempfile

from dyglib_amd import _build

SOURCES = ["dygformer_fused3.hip", "dygformer_fused3_train.hip", "dygformer_fused3_bwd.hip"]


def _remarks(src, tmp):
    cmd = [_build._hipcc(), *_build.CXXFLAGS, "-I", _build.INCLUDE, "--cuda-device-only", "-c",
           f"{_build.CSRC}/{src}", "-o", f"{tmp}/{src}.o", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@functools.lru_cache(maxsize=None)
def _resource_usage():
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(len(SOURCES)) as ex:
        logs = list(ex.map(lambda s: _remarks(s, tmp), SOURCES))
    usage, name = {}, None
    for line in "\n".join(logs).splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    return usage


def test_pooled_inference_kernels_keep_their_register_budget():
    usage = _resource_usage()
    # mangled template arguments: <TPW, TR, NW, PL> = ILi<TPW>ELb<TR>ELi<NW>ELi<PL>E
    kern = lambda tpw, nw, pl: next(v for k, v in usage.items() if f"k_dygformer_fused3ILi{tpw}ELb0ELi{nw}ELi{pl}E" in k)
    headline = kern(4, 8, 1)
    print("k_dygformer_fused3<4,false,8,1>:", headline, " <8,false,8,1>:", kern(8, 8, 1), " <4,false,4,1>:", kern(4, 4, 1))
    assert headline["ScratchSize [bytes/lane]"] == 0 and headline["VGPRs Spill"] == 0, headline
    assert kern(4, 4, 1)["ScratchSize [bytes/lane]"] == 0, kern(4, 4, 1)
    assert kern(8, 8, 1)["VGPRs Spill"] <= 2, kern(8, 8, 1)          # the per-token form's figure


# (ScratchSize [bytes/lane], VGPRs Spill) of commit c0e4020, the last one with all of these kernels in dygformer_fused3.hip, compiled
# with the same flags: the ceiling of each kernel here
PARENT_BUDGET = {
    "k_dygformer_fused3ILi4ELb1ELi4ELi0E": (0, 0),        # <4, true, 4>
    "k_dygformer_fused3ILi4ELb1ELi8ELi0E": (48, 17),      # <4, true, 8>
    "k_dygformer_fused3ILi8ELb1ELi8ELi0E": (304, 83),     # <8, true, 8>
    "k_ffn_bwdILi4E": (0, 0),
    "k_ffn_bwdILi8E": (0, 0),
    "k_attn_bwdILi4ELi4E": (0, 0),
    "k_attn_bwdILi4ELi8E": (12, 2),
    "k_attn_bwdILi8ELi8E": (192, 47),
}


def test_training_kernels_stay_within_the_scratch_and_spills_of_the_unsplit_file():
    usage = _resource_usage()
    for tag, (scratch, spill) in PARENT_BUDGET.items():
        hits = [v for k, v in usage.items() if tag in k]
        assert len(hits) == 1, (tag, sorted(usage))
        print(tag, hits[0], "ceiling:", scratch, spill)
        assert hits[0]["ScratchSize [bytes/lane]"] <= scratch and hits[0]["VGPRs Spill"] <= spill, (tag, hits[0])
