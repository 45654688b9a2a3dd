"""Register budget of the fused DyGFormer inference kernels, as hipcc reports it (-Rpass-analysis=kernel-resource-usage).

DESIGN §4.3: the pooled product kernel of the headline shape, k_dygformer_fused3<4, false, 8, 1>, uses no scratch memory, and the
128-token shape <8, false, 8, 1> spills no more than the 2 VGPRs of the per-token form it replaces (outside the loops).  Both figures
lean on two values being formed where they are used instead of being kept alive through the layer loop (the empty `asm` statements in
the kernel), which a compiler update may undo: this test says so at build time.  The device code is compiled with the build's own flags;
no GPU is needed."""
import re
import subprocess
import tempfile

from dyglib_amd import _build


def _resource_usage():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc(), *_build.CXXFLAGS, "-I", _build.INCLUDE, "--cuda-device-only", "-c",
               f"{_build.CSRC}/dygformer_fused3.hip", "-o", f"{tmp}/fused3.o", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
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
