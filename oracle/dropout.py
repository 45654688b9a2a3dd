"""CPU ORACLE (test infrastructure) — host restatement of the training path's dropout generator, dyglib_amd/csrc/dropout.h (train::Drop):
a counter-based hash of (seed, site, element index), so a mask is a function of where the element sits, never of which kernel draws it.
All arithmetic is uint32 wrap-around, done here in uint64 and masked back to 32 bits."""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64) & _M32


def _mul(x: np.ndarray, c: int) -> np.ndarray:
    return (x * np.uint64(c)) & _M32          # both factors < 2^32: the product fits in uint64


def mix32(x) -> np.ndarray:
    """dropout.h mix32: 32-bit integer hash with full avalanche (uint32 in, uint32 out)."""
    x = _u32(x)
    x ^= x >> np.uint64(16)
    x = _mul(x, 0x7FEB352D)
    x ^= x >> np.uint64(15)
    x = _mul(x, 0x846CA68B)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


class Drop:
    """dropout.h make_drop: the keys, threshold and scale of dropout probability `p` (taken as float32: the C ABI passes a float) and a
    64-bit seed."""

    def __init__(self, p: float, seed: int):
        p32 = np.float32(p)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.p = p32
        self.key0 = seed & 0xFFFFFFFF
        self.key1 = ((seed >> 32) * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF
        self.thresh = 0 if p32 <= 0 else int(float(p32) * 4294967296.0)          # (uint32_t)((double)p * 2^32): truncation
        self.scale = np.float32(1.0) if p32 <= 0 else np.float32(1.0 / (1.0 - float(p32)))

    def site_key(self, site: int) -> int:
        return int(mix32((self.key0 + 0x9E3779B9 * (int(site) + 1)) & 0xFFFFFFFF)) ^ self.key1

    def mask(self, site: int, idx) -> np.ndarray:
        """float32 multipliers of elements `idx` (any shape, int64 / uint64) of site `site`: scale where kept, 0 where dropped."""
        h = mix32(_u32(fold_index(idx)) ^ np.uint64(self.site_key(site)))
        return np.where(h.astype(np.uint64) >= np.uint64(self.thresh), self.scale, np.float32(0.0)).astype(np.float32)


def make_drop(p: float, seed: int) -> Drop:
    return Drop(p, seed)


def fold_index(idx) -> np.ndarray:
    """The 64-bit element index folded to 32 bits: (uint32)idx + 0x27d4eb2f * (uint32)(idx >> 32).  The identity below 2^32."""
    i = np.asarray(idx).astype(np.uint64)
    return ((i & _M32) + _mul(i >> np.uint64(32), 0x27D4EB2F)) & _M32


def mask(p: float, seed: int, site: int, idx) -> np.ndarray:
    """Drop(p, seed).mask(site, idx)."""
    return Drop(p, seed).mask(site, idx)
