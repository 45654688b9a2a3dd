"""Register budget of the link-predictor head's kernels (merge_layer.hip), as hipcc reports it (-Rpass-analysis=kernel-resource-usage), on the
pattern of test_encoder_block_resources_cpu.py.

The five kernels came out of dygformer_api.hip unchanged.  There, compiled with the build's flags, they had

    k_merge_sigmoid            26 VGPRs  8 waves/SIMD          k_merge_sigmoid_rows4<1>   40 VGPRs  8 waves/SIMD
    k_merge_sigmoid_mfma       48 VGPRs  8 waves/SIMD          k_merge_sigmoid_rows4<4>   58 VGPRs  8 waves/SIMD
    k_merge_bwd_rows          132 VGPRs  3 waves/SIMD  (13056 bytes of LDS: dh^T [192][17])

and no scratch and no spills; each is held to that occupancy in its new file, the file holds these five and no other kernel, and
dygformer_api.hip, which keeps the DyGFormer entry points, has no device code left.  The device code is compiled with the build's own
flags; no GPU is needed."""
import concurrent.futures as cf
import functools
import re
import subprocess
import tempfile

from dyglib_amd import _build

SOURCES = ["merge_layer.hip", "dygformer_api.hip"]
FIELDS = r"VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]"
# mangled name -> waves/SIMD in the parent's dygformer_api.hip
FLOOR = {"_ZN5dygnn15k_merge_sigmoidEPKfS1_iiS1_S1_S1_S1_Pfi": 8,
         "_ZN5dygnn20k_merge_sigmoid_mfmaEPKfS1_liiS1_S1_S1_S1_Pfi": 8,
         "_ZN5dygnn21k_merge_sigmoid_rows4ILi1EEEvPKfS2_liiS2_S2_S2_S2_Pfii": 8,
         "_ZN5dygnn21k_merge_sigmoid_rows4ILi4EEEvPKfS2_liiS2_S2_S2_S2_Pfii": 8,
         "_ZN5dygnn16k_merge_bwd_rowsEPKfS1_liiS1_S1_S1_S1_PfiS2_S2_S2_S2_": 3}


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


def test_merge_layer_holds_the_five_head_kernels_and_nothing_else():
    assert set(_resource_usage()["merge_layer.hip"]) == set(FLOOR), sorted(_resource_usage()["merge_layer.hip"])


def test_the_head_kernels_keep_their_occupancy_without_scratch_or_spills():
    for name, floor in FLOOR.items():
        u = _resource_usage()["merge_layer.hip"][name]
        print(name, u, "floor:", floor)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["Occupancy [waves/SIMD]"] >= floor, (name, u)


def test_the_dygformer_entry_points_have_no_device_code_left():
    assert _resource_usage()["dygformer_api.hip"] == {}, sorted(_resource_usage()["dygformer_api.hip"])
    assert "__global__" not in open(f"{_build.CSRC}/dygformer_api.hip").read()
