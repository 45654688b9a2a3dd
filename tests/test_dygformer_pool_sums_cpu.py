"""The reduce-scatter behind the pooled layer's per-side token sums (csrc/fused3_device.h: row_sums8), the part that needs no GPU.

The kernels sum eight values per lane — two register tiles; input k = 4 u + r is row 4 g + r of tile u, g = lane >> 4 — over the 16 lanes of
a lane group (the 16 tokens of the wave's tile).  The 64 lanes are simulated here in numpy, instruction for instruction: a DPP add writes
the banks its mask names (a bank = four lanes of a row of 16) and leaves the other banks of the destination as they were; row_ror:n gives
lane c the value of lane c - n (mod 16) of its row.  Where the sums end up is the library's own arithmetic (csrc/fused3_plan.h, through
dygnn_dygformer_pool_sum_slot_host), the one the kernels store by.

* Every (lane group, tile, row) sum is stored exactly once, at the word the epilogue reads: [tile][row] of the step's two tiles.
* Every sum is the same tree over its 16 tokens — ((c + c^8) + (c^4 + c^12)), then the quad's lanes ^1 and ^2 — whichever register and bank it
  ends in: a row's bits depend on its tokens alone.
* A tile of one side and a tile that straddles the sides give the same bits for the same tokens: the straddling form's other-side lanes and
  the one-side form's absent lanes both enter as +0, and the two are the same routine."""
import ctypes as C

import numpy as np

from dyglib_amd import _capi

# (destination, DPP source, control, argument, bank mask) of row_sums8's sixteen adds, in order; registers 0 .. 3 = tile 0's, 4 .. 7 = tile 1's
PROGRAM = (
    [(j, j, "ror", 8, 0x3) for j in range(4)] + [(j, j + 4, "ror", 8, 0xC) for j in range(4)]
    + [(j, j, "ror", 12, 0x5) for j in range(2)] + [(j, j + 2, "ror", 4, 0xA) for j in range(2)]
    + [(j, j, "quad", (1, 0, 3, 2), 0xF) for j in range(2)] + [(j, j, "quad", (2, 3, 0, 1), 0xF) for j in range(2)]
)


def simulate(v):
    """v: float32 [8 registers][64 lanes] -> the two result registers [2][64]"""
    v = v.astype(np.float32).copy()
    lane = np.arange(64)
    row, c = lane & ~15, lane & 15
    for dst, src, ctrl, arg, mask in PROGRAM:
        frm = row + (c - arg) % 16 if ctrl == "ror" else (lane & ~3) + np.asarray(arg)[lane & 3]
        s = (v[src][frm] + v[src]).astype(np.float32)             # v_add_f32_dpp dst, src (through DPP), src
        on = ((mask >> (c >> 2)) & 1).astype(bool)
        v[dst] = np.where(on, s, v[dst])
    return v[:2]


def slots():
    out = []
    for lane in range(64):
        o = (C.c_int32 * 5)()
        _capi.load().dygnn_dygformer_pool_sum_slot_host(lane, o)
        out.append(tuple(o))
    return out


def tree(x):
    """the one order of a row's sum; x: float32 [16 tokens]"""
    f = np.float32
    p = [f(f(x[c] + x[c ^ 8]) + f(x[c ^ 4] + x[c ^ 12])) for c in range(4)]
    return f(f(p[0] + p[1]) + f(p[2] + p[3]))


def test_every_sum_is_stored_once_where_the_epilogue_reads_it():
    # input k of lane group g holds the integer 1000 (8 g + k) + token: every sum names its row, and integer sums are exact
    lane = np.arange(64)
    v = np.stack([1000.0 * (8 * (lane >> 4) + k) + (lane & 15) for k in range(8)]).astype(np.float32)
    z = simulate(v)
    words = {}                                                    # word of the [2 tiles][16 rows] block -> value
    for ln, (stores, tile, row, in0, in1) in enumerate(slots()):
        g, bank = ln >> 4, (ln & 15) >> 2
        assert stores == (1 if ln % 4 == 0 else 0)
        assert row // 4 == g and 0 <= tile <= 1                   # rows 4 g .. 4 g + 3 belong to lane group g
        for j, k in enumerate((in0, in1)):
            assert z[j][ln] == 16 * 1000.0 * (8 * g + k) + 120.0, (ln, j)      # every lane of the bank holds the sum of input k
            assert k == 4 * tile + (row + j) % 4, (ln, j, k)      # ... and stores it at [tile k / 4][row 4 g + k % 4]
            if stores:
                w = 16 * tile + row + j
                assert w not in words, (ln, w)
                words[w] = z[j][ln]
        assert (in0, in1) == (4 * (bank >> 1) + 2 * (bank & 1), 4 * (bank >> 1) + 2 * (bank & 1) + 1)
    assert sorted(words) == list(range(32))                       # 2 tiles x 16 rows (4 per lane group), each exactly once
    for g in range(4):
        for u in range(2):
            for r in range(4):
                assert words[16 * u + 4 * g + r] == 16 * 1000.0 * (8 * g + 4 * u + r) + 120.0


def test_every_sum_takes_the_same_tree_whatever_register_and_bank_holds_it():
    rs = np.random.RandomState(5)
    v = (rs.standard_normal((8, 64)) * np.exp(rs.uniform(-6, 6, (8, 64)))).astype(np.float32)       # magnitudes apart: the order shows in the bits
    z = simulate(v)
    for ln, (stores, tile, row, in0, in1) in enumerate(slots()):
        for j, k in enumerate((in0, in1)):
            want = tree(v[k][(ln & ~15):(ln & ~15) + 16])
            assert z[j][ln].tobytes() == want.tobytes(), (ln, j, k)
    # the same sixteen tokens in another register and another tile: the same bits
    z2 = simulate(v[[5, 6, 7, 4, 1, 2, 3, 0]])
    sl = slots()
    for g in range(4):
        a = next(ln for ln in range(16 * g, 16 * g + 16) if sl[ln][3] == 0)      # input 0 of the second run is input 5 of the first
        b = next(ln for ln in range(16 * g, 16 * g + 16) if sl[ln][4] == 5)
        assert z2[0][a].tobytes() == z[1][b].tobytes()


def test_one_side_and_straddling_tiles_give_the_same_bits_for_the_same_tokens():
    rs = np.random.RandomState(6)
    h = rs.standard_normal((8, 64)).astype(np.float32)
    tok = np.arange(64) & 15
    for k in (1, 7, 15):                                          # source tokens [0, k); then destination tokens, or nothing
        one_side = np.where(tok < k, h, np.float32(0.0))           # the tile ends at token k: absent lanes are +0
        src_form = np.where(tok < k, h * np.float32(1.0), np.float32(0.0))      # the tile straddles: the weight 1, the other side's lanes +0
        dst_form = np.where(tok >= k, h * np.float32(1.0), np.float32(0.0))
        a, b, d = simulate(one_side), simulate(src_form), simulate(dst_form)
        assert a.tobytes() == b.tobytes(), k
        # and the destination side's sum does not see the source tokens: the same tokens alone in a tile of their own lanes
        assert d.tobytes() == simulate(np.where(tok >= k, h, np.float32(0.0))).tobytes(), k
