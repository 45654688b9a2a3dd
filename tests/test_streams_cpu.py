"""The stream tests' case list (tests/stream_cases.py) names everything dyglib_amd exports that launches on a stream, so a backbone or device
primitive added later cannot be left out of tests/test_streams_gpu.py silently; and its host-side pieces hold what the GPU test relies on."""
import numpy as np

import dyglib_amd
from tests import stream_cases as sc


def test_every_export_is_a_stream_case_or_host_only():
    covered = {name for c in sc.CASES for name in c.covers}
    exported = set(dyglib_amd.__all__)
    assert covered <= exported, covered - exported
    assert set(sc.HOST_ONLY) <= exported, set(sc.HOST_ONLY) - exported
    assert not covered & set(sc.HOST_ONLY)
    missing = exported - covered - set(sc.HOST_ONLY)
    assert not missing, f"exported by dyglib_amd but in no stream case (tests/stream_cases.py): {sorted(missing)}"
    assert all(reason for reason in sc.HOST_ONLY.values())


def test_every_trainable_backbone_has_a_training_step():
    by_name = {c.name: c for c in sc.CASES}
    for backbone, case in sc.TRAIN_BACKBONES.items():
        assert backbone in by_name[case].covers
    # a backbone that gains a training path (its module defines an autograd Function) needs a training step here too
    import importlib
    import torch
    for module, backbone in (("dygformer", "DyGFormer"), ("tgat", "TGAT"), ("memory_model", "MemoryModel"), ("tcl", "TCL"), ("cawn", "CAWN"),
                             ("graphmixer", "GraphMixer"), ("memory_variants", "JODIE")):
        m = importlib.import_module("dyglib_amd." + module)
        trains = any(isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == m.__name__ for v in vars(m).values())
        assert trains == (backbone in sc.TRAIN_BACKBONES), (module, trains)


def test_case_names_are_unique_and_the_other_batch_is_another_valid_batch():
    assert len(set(sc.CASE_NAMES)) == len(sc.CASE_NAMES)
    for c in sc.CASES:
        real, stale = c.inputs(), c.stale()
        assert list(real) == list(stale)
        for k in real:
            assert stale[k].shape == real[k].shape and stale[k].dtype == real[k].dtype, (c.name, k)
            assert (stale[k] != real[k]).any(), (c.name, k)                                   # a launch that reads it computes something else
            # a permutation of the real array along one axis: every id is an id of the same graph, every time one of its times
            assert np.array_equal(np.sort(stale[k], axis=c.roll_axis), np.sort(real[k], axis=c.roll_axis)), (c.name, k)


def test_hold_lengths():
    assert sc.hold_ms(0.1) == sc.MIN_HOLD_MS == 20.0
    assert sc.hold_ms(5.0) == 50.0
    assert sc.hold_ms(1e3) == sc.MAX_HOLD_MS == 250.0
