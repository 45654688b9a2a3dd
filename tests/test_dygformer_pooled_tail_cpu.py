"""Host arithmetic of the deferred pooled epilogue without a GPU: the fused path's workspace holds one row of 800 + 208 floats per
(pair, side) for k_pooled_tail, on top of the per-query search results (≈ 24 B per query + one CallDims per pair)."""
import ctypes as C

from dyglib_amd import _capi

ROW_BYTES = (800 + 208) * 4


def test_fused_workspace_holds_the_pooled_rows():
    lib = _capi.load()
    cfg = _capi.DygformerConfig(172, 172, 100, 50, 2, 2, 2, 64)
    size = lambda B, impl: lib.dygnn_dygformer_workspace_bytes_for(C.byref(cfg), B, impl)
    for B in (1, 9, 257, 12800):
        rows = 2 * B * ROW_BYTES
        search = 2 * B * (4 + 8) + B * 32           # hist_len, end_pos, CallDims
        assert rows + search <= size(B, 3) <= rows + search + 4 * 256, B          # four sections, each padded to 256 B
        assert size(B, 0) == size(B, 3) and size(B, 1) > size(B, 3)               # the generic path adds its activation buffers
        assert lib.dygnn_dygformer_workspace_bytes(C.byref(cfg), B) == size(B, 1)
