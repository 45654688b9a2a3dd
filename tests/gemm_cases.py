"""Case table, buffers and float64 references for the general GEMM (dygnn_mm: k_mm / k_mm_big / k_mm_dma behind train::mm) and the grouped
weight-gradient product (dygnn_dw_grouped).  numpy only: tests/test_gemm_cases_cpu.py checks the table without a GPU, tests/test_gemm_gpu.py
runs it.

Buffers.  Every operand lies inside a larger allocation.  A and B hold NaN wherever the product may not read: behind the logical width up to
the leading dimension, in guard blocks before and after, between batches (an a_kpad case holds zeros from K to round_up(K, 4), NaN beyond).
C and colsum_out are pre-filled with a sentinel bit pattern everywhere; the logical elements of C then get C0 where the call reads them
(beta != 0), zeros where the call says it zeroed them (c_is_zero) and keep the sentinel, a NaN, where the call must overwrite.  Row tables
are drawn with repeats from a taller A and every entry is a valid row, so no kernel, right or wrong, is sent out of range by the table.

Two value regimes.  "exact": A, B, bias, C0 integers in [-3, 3], alpha in {1, -2, 0.5}, beta in {0, 1, 0.5}, K <= 4608: every partial sum
is an integer or half-integer below 2^24, so any summation order (split-K atomics included) gives the same float32 and the bar is equality.
"rounded": standard normal A and B, bias and C0 of order 1; the bar is the forward bound of a K-term inner product in any order,
    |got - ref| <= 2 (K + 4) 2^-24 (|alpha| |op(A)| . |op(B)| + |bias| + |beta C0|),
(gamma_K ~ K u with u = 2^-24, four more operations in the epilogue, the factor 2 because the rounding inside the f32 MFMA accumulation is
not documented: it covers u = 2^-23).  Derived, not measured."""
import numpy as np

SMALL, BIG, DMA = 0, 1, 2                      # dygnn_mm_path: k_mm, k_mm_big, k_mm_dma
KERNEL_NAMES = {SMALL: "k_mm", BIG: "k_mm_big", DMA: "k_mm_dma"}
E_INVALID, E_UNSUPPORTED = -1, -3
SENTINEL_BITS = 0x7FC5A5A5                     # a quiet NaN with a payload no kernel produces
U = 2.0 ** -24
ALPHAS, BETAS = (1.0, -2.0, 0.5), (0.0, 1.0, 0.5)
SPLIT_K, KCHUNK = 2048, 256                    # mm splits batch == 1, K >= 2048, !relu into parts of 256 columns
DW_MAX_PROBLEMS = 36                           # kDwMaxProblems = 4 * DYGNN_MAX_LAYERS + 4
FAKE_BASE = 0x40000000                         # a 16-byte aligned non-null address for the host-only path queries


def r4(x):
    return (x + 3) // 4 * 4


def mk(name, kernel, M, N, K, tA=False, tB=False, alpha=1.0, beta=0.0, bias=False, relu=False, batch=1, H=1, lda=None, ldb=None, ldc=None,
       offA=0, offB=0, offC=0, c_is_zero=False, colsum=False, m_dev=None, a_kpad=False, a_rows=False, strides=None, dma_env=None, ksplit=1,
       f4=None, group="misc", zero_pad=False, data=None):
    """One call of dygnn_mm.  kernel / ksplit / f4: what the table INTENDS the dispatch to do (a negative kernel: the refusal's code).
    off*: floats by which the base pointer misses 16-byte alignment.  ld* default to the logical width rounded up to 4, plus 4.
    zero_pad: A's columns K .. round_up(K, 4) hold zeros although the call does not pass a_kpad.  data: the case whose values this one shares."""
    wA, wB = (M if tA else K), (K if tB else N)
    c = dict(name=name, kernel=kernel, M=M, N=N, K=K, tA=tA, tB=tB, alpha=alpha, beta=beta, bias=bias, relu=relu, batch=batch, H=H,
             zero_pad=zero_pad or a_kpad, data=data or name,
             lda=r4(wA) + 4 if lda is None else lda, ldb=r4(wB) + 4 if ldb is None else ldb, ldc=r4(N) + 4 if ldc is None else ldc,
             offA=offA, offB=offB, offC=offC, c_is_zero=c_is_zero, colsum=colsum, m_dev=m_dev, a_kpad=a_kpad, a_rows=a_rows,
             strides={**dict(sAb=0, sAh=0, sBb=0, sBh=0, sCb=0, sCh=0), **(strides or {})}, dma_env=dma_env, ksplit=ksplit,
             f4=(kernel == DMA) if f4 is None else f4, group=group)
    assert alpha in ALPHAS and beta in BETAS and c["lda"] >= wA and c["ldb"] >= wB and c["ldc"] >= N
    return c


def case_id(c):
    return c["name"]


ORIENT = [(False, False), (False, True), (True, False), (True, True)]
ON = {(False, False): "NN", (False, True): "NT", (True, False): "TN", (True, True): "TT"}


def _cycle(*lists):
    n = max(len(l) for l in lists)
    return [tuple(l[i % len(l)] for l in lists) for i in range(n)]


def _mm_cases():
    out = []
    # ---- orientations x sizes on each kernel.  Every M, N and K of the issue's lists appears on every kernel and orientation that can take it.
    for tA, tB in ORIENT:
        o = ON[(tA, tB)]
        # k_mm: M < 48 or N < 48
        small = [(1, 130), (47, 68), (1, 64), (47, 51), (1, 50), (47, 49), (1, 48), (47, 47), (1, 1), (47, 1), (48, 47), (50, 1), (64, 47), (65, 1), (132, 47)]
        for i, ((M, N), K) in enumerate(_cycle(small, [1, 4, 15, 16, 17, 20, 36, 172])):
            out.append(mk(f"small-{o}-m{M}n{N}k{K}", SMALL, M, N, K, tA, tB, alpha=ALPHAS[i % 3], bias=i % 2 == 0, group="sizes"))
        # k_mm_dma: K % 4 == 0, tA: M % 4 == 0, !tB: N % 4 == 0; aligned, default ld multiples of 4
        Ms = [48, 64, 132] if tA else [48, 50, 64, 65, 132]
        Ns = [48, 49, 50, 51, 64, 68, 130] if tB else [48, 64, 68]
        for i, (M, N, K) in enumerate(_cycle(Ms, Ns, [4, 16, 20, 36, 172])):
            out.append(mk(f"dma-{o}-m{M}n{N}k{K}", DMA, M, N, K, tA, tB, alpha=ALPHAS[i % 3], bias=i % 2 == 1, group="sizes"))
        # k_mm_big: the same size lists without the multiples-of-4 conditions, forced off the DMA path by an A base one float off alignment
        # (K % 4 != 0 would do for some, not for all)
        for i, (M, N, K) in enumerate(_cycle([48, 50, 64, 65, 132], [48, 49, 50, 51, 64, 68, 130], [1, 4, 15, 16, 17, 20, 36, 172])):
            out.append(mk(f"big-{o}-m{M}n{N}k{K}", BIG, M, N, K, tA, tB, alpha=ALPHAS[i % 3], bias=i % 2 == 0, offA=1, group="sizes"))
        # ---- k_mm_big on a DMA-eligible shape, one broken precondition at a time, and by the environment switch
        M, N, K = 64, 68, 36
        wA, wB = (M if tA else K), (K if tB else N)
        out.append(mk(f"route-{o}-eligible", DMA, M, N, K, tA, tB, bias=True, group="routes"))
        out.append(mk(f"route-{o}-A+1", BIG, M, N, K, tA, tB, bias=True, offA=1, group="routes"))
        out.append(mk(f"route-{o}-B+1", BIG, M, N, K, tA, tB, bias=True, offB=1, group="routes"))
        out.append(mk(f"route-{o}-lda-odd", BIG, M, N, K, tA, tB, bias=True, lda=wA + 1, group="routes"))
        out.append(mk(f"route-{o}-ldb-odd", BIG, M, N, K, tA, tB, bias=True, ldb=wB + 1, group="routes"))
        out.append(mk(f"route-{o}-k-mod4-2", BIG, M, N, K + 2, tA, tB, bias=True, group="routes"))
        if tA:
            out.append(mk(f"route-{o}-m-mod4-2", BIG, M + 2, N, K, tA, tB, bias=True, group="routes"))
        if not tB:
            out.append(mk(f"route-{o}-n-mod4-2", BIG, M, N + 2, K, tA, tB, bias=True, group="routes"))
        out.append(mk(f"route-{o}-env0", BIG, M, N, K, tA, tB, bias=True, dma_env="0", group="routes"))
    # ---- epilogues of k_mm_dma: float4 (aligned C, ldc % 4 == 0, beta == 0) and scalar (C one float off, ldc odd, beta == 1); relu with a bias
    # and mixed signs through both, and through k_mm and k_mm_big
    for tB, N in ((True, 51), (True, 130), (False, 68)):
        o, M, K = ON[(False, tB)], 65, 36
        for relu in (False, True):
            r = "-relu" if relu else ""
            out.append(mk(f"epi-{o}-n{N}{r}-f4", DMA, M, N, K, False, tB, bias=True, relu=relu, alpha=0.5, group="epilogues"))
            out.append(mk(f"epi-{o}-n{N}{r}-C+1", DMA, M, N, K, False, tB, bias=True, relu=relu, alpha=0.5, offC=1, f4=False, group="epilogues"))
            out.append(mk(f"epi-{o}-n{N}{r}-ldc-odd", DMA, M, N, K, False, tB, bias=True, relu=relu, alpha=0.5, ldc=N + 1 + N % 2, f4=False, group="epilogues"))
            out.append(mk(f"epi-{o}-n{N}{r}-beta1", DMA, M, N, K, False, tB, bias=True, relu=relu, alpha=-2.0, beta=1.0, f4=False, group="epilogues"))
            out.append(mk(f"epi-{o}-n{N}{r}-beta.5", DMA, M, N, K, False, tB, bias=True, relu=relu, beta=0.5, f4=False, group="epilogues"))
    for tA, tB in ORIENT:
        o = ON[(tA, tB)]
        out.append(mk(f"epi-small-{o}-relu", SMALL, 47, 50, 20, tA, tB, bias=True, relu=True, alpha=-2.0, beta=0.5, group="epilogues"))
        out.append(mk(f"epi-big-{o}-relu", BIG, 50, 50, 17, tA, tB, bias=True, relu=True, alpha=0.5, beta=1.0, group="epilogues"))
        out.append(mk(f"epi-big-{o}-ldc-odd", BIG, 65, 51, 15, tA, tB, ldc=53, offC=3, group="epilogues"))
        out.append(mk(f"epi-small-{o}-ldc-odd", SMALL, 20, 51, 15, tA, tB, ldc=51, offC=1, beta=1.0, group="epilogues"))
    # ---- split-K: K in {2048, 2052, 2304} and 2050 (off the DMA path); bias added once; beta 0 over garbage, beta 0 over a zeroed C with
    # c_is_zero, beta 1 over C0; relu at K = 2048 does not split
    def parts(K):
        return (K + KCHUNK - 1) // KCHUNK
    for kern, kn, M, N, off in ((SMALL, "small", 20, 52, 0), (BIG, "big", 52, 68, 1), (DMA, "dma", 52, 68, 0)):
        for i, (tA, tB) in enumerate(ORIENT):
            o, K = ON[(tA, tB)], (2048, 2052, 2304, 2052)[i]
            kw = dict(tA=tA, tB=tB, offA=off, ksplit=parts(K), f4=False, group="splitk")
            out.append(mk(f"split-{kn}-{o}-k{K}-garbage", kern, M, N, K, bias=True, alpha=ALPHAS[i % 3], **kw))
            out.append(mk(f"split-{kn}-{o}-k{K}-zeroed", kern, M, N, K, bias=True, c_is_zero=True, **kw))
            out.append(mk(f"split-{kn}-{o}-k{K}-beta1", kern, M, N, K, bias=True, beta=1.0, alpha=ALPHAS[(i + 1) % 3], **kw))
        out.append(mk(f"split-{kn}-NT-k2048-relu", kern, M, N, 2048, tB=True, bias=True, relu=True, beta=1.0, offA=off, f4=False, group="splitk"))
        out.append(mk(f"split-{kn}-NT-k2048-relu-beta0", kern, M, N, 2048, tB=True, bias=True, relu=True, offA=off, group="splitk"))
        # K = 2050: no float4 fits the K tail, so an aligned call falls to k_mm_big (k_mm stays k_mm)
        out.append(mk(f"split-{kn}-NT-k2050", SMALL if kern == SMALL else BIG, M, N, 2050, tB=True, bias=True, offA=off, ksplit=parts(2050), f4=False,
                      group="splitk"))
    # ---- a_kpad: !tA, !tB, K in {18, 171}, lda = round_up(K, 4) and larger; with the flag k_mm_dma, without it k_mm_big on the same buffers
    for K in (18, 171):
        for lda in (r4(K), r4(K) + 8):
            out.append(mk(f"kpad-k{K}-lda{lda}", DMA, 65, 68, K, lda=lda, a_kpad=True, bias=True, group="kpad"))
            out.append(mk(f"kpad-k{K}-lda{lda}-noflag", BIG, 65, 68, K, lda=lda, zero_pad=True, data=f"kpad-k{K}-lda{lda}", bias=True, group="kpad"))
    # ---- a_rows: on k_mm_dma, NT and NN, M in {48, 100}, without m_dev and with m_dev in {1, 64, 65, M}
    for tB in (True, False):
        for M in (48, 100):
            for md in (None, 1, 64, 65, M):
                if md is not None and md > M:
                    continue
                out.append(mk(f"rows-{ON[(False, tB)]}-m{M}-mdev{md}", DMA, M, 52, 20, False, tB, a_rows=True, m_dev=md, bias=True, group="rows"))
    out.append(mk("rows-NT-split", DMA, 100, 52, 2052, False, True, a_rows=True, beta=1.0, ksplit=parts(2052), f4=False, group="rows"))
    out.append(mk("rows-refused-A+1", E_UNSUPPORTED, 100, 52, 20, False, True, a_rows=True, offA=1, group="refusals"))
    out.append(mk("rows-refused-k-mod4", E_UNSUPPORTED, 100, 52, 18, False, True, a_rows=True, group="refusals"))
    out.append(mk("rows-refused-env0", E_UNSUPPORTED, 100, 52, 20, False, True, a_rows=True, dma_env="0", group="refusals"))
    out.append(mk("rows-refused-m20", E_UNSUPPORTED, 20, 52, 20, False, True, a_rows=True, group="refusals"))
    out.append(mk("rows-refused-tA", E_UNSUPPORTED, 100, 52, 20, True, False, a_rows=True, group="refusals"))
    # ---- the other refusals: beta outside {0, 1} on a split product; column sums with !tA, with batch > 1
    for kn, M, off in (("small", 20, 0), ("big", 52, 1), ("dma", 52, 0)):
        out.append(mk(f"refused-split-beta.5-{kn}", E_UNSUPPORTED, M, 68, 2048, beta=0.5, offA=off, group="refusals"))
        out.append(mk(f"refused-colsum-notA-{kn}", E_UNSUPPORTED, M, 68, 20, False, True, colsum=True, offA=off, group="refusals"))
        out.append(mk(f"refused-colsum-batch-{kn}", E_UNSUPPORTED, M, 68, 20, True, False, colsum=True, offA=off, batch=2, H=1,
                      strides=dict(sAb=4096, sCb=8192), group="refusals"))
    # ---- m_dev on all three kernels: {0, 1, 64, 65, M} at M = 132, and one split-K case (beta = 1: a split with beta = 0 zeroes all M rows)
    for kern, kn, N, off in ((SMALL, "small", 47, 0), (BIG, "big", 50, 1), (DMA, "dma", 50, 0)):
        for md in (0, 1, 64, 65, 132):
            out.append(mk(f"mdev-{kn}-{md}", kern, 132, N, 20, False, True, m_dev=md, bias=True, offA=off, group="mdev"))
            out.append(mk(f"mdev-{kn}-{md}-beta1", kern, 132, N, 20, True, True, m_dev=md, beta=1.0, offA=off, f4=False, group="mdev"))
    out.append(mk("mdev-dma-65-split", DMA, 132, 52, 2052, True, False, m_dev=65, beta=1.0, ksplit=parts(2052), f4=False, group="mdev"))
    # ---- batched, TGAT's per-head pattern: batch = 6, H = 3; A [n][H hd] (sAh = hd), weights [H hd][ldb] (sBh = hd ldb), C [n][H Dkv] (sCh = Dkv)
    def heads(name, kernel, n, hd, Dkv, two_copies, f4=None):
        H, lda, ldb, ldc = 3, 3 * hd, r4(Dkv) + 4, 3 * Dkv
        st = dict(sAh=hd, sBh=hd * ldb, sCh=Dkv, sCb=n * ldc)
        if two_copies:
            st.update(sAb=n * lda + 8, sBb=H * hd * ldb + 12)
        return mk(name, kernel, n, Dkv, hd, batch=6, H=H, lda=lda, ldb=ldb, ldc=ldc, strides=st, bias=True, f4=f4, group="batched")
    out.append(heads("heads-dma-shared-A", DMA, 50, 8, 48, False))
    out.append(heads("heads-big-hd6", BIG, 50, 6, 48, False))
    out.append(heads("heads-dma-all-strides", DMA, 50, 8, 52, True))
    out.append(heads("heads-big-all-strides", BIG, 65, 6, 50, True))
    out.append(heads("heads-small-n20", SMALL, 20, 8, 48, True))
    # ---- batched with all six strides in play, one case per kernel: batch = 4, H = 2, every stride non-zero and different from the other five
    # (a call that swaps two of them reads NaN or misses C); a guard block between the four products of each operand.  The smallest shapes that
    # select each kernel; k_mm_dma keeps its strides multiples of 4, the other two get odd ones
    def strided(name, kernel, M, N, K, tA, tB, step, **kw):
        c = mk(name, kernel, M, N, K, tA, tB, batch=4, H=2, bias=True, group="batched", **kw)
        st = {}
        for i, (X, rows, ld) in enumerate((("A", K if tA else M, c["lda"]), ("B", N if tB else K, c["ldb"]), ("C", M, c["ldc"]))):
            st[f"s{X}h"] = rows * ld + r4(4 * ld + 16) + step * i
            st[f"s{X}b"] = 2 * st[f"s{X}h"] + r4(4 * ld + 16) + step * (i + 1)
        assert all(st.values()) and len(set(st.values())) == 6
        c["strides"] = st
        return c
    out.append(strided("strides-small-TN", SMALL, 5, 7, 6, True, False, 1, alpha=-2.0))
    out.append(strided("strides-dma-NN", DMA, 64, 48, 8, False, False, 4, alpha=0.5))
    out.append(strided("strides-big-NT", BIG, 50, 49, 7, False, True, 1, offA=1, beta=1.0))
    # ---- column sums (tA), onto a pre-filled colsum_out: riding along in k_mm_dma and k_mm_big, stand-alone next to k_mm, and split at K = 2304
    for tB in (False, True):
        o = ON[(True, tB)]
        for M in (64, 100):
            out.append(mk(f"colsum-dma-{o}-m{M}", DMA, M, 48, 36, True, tB, colsum=True, group="colsum"))
            out.append(mk(f"colsum-big-{o}-m{M}", BIG, M, 48, 36, True, tB, colsum=True, offA=1, group="colsum"))
            out.append(mk(f"colsum-big-{o}-m{M}-k17", BIG, M, 48, 17, True, tB, colsum=True, offB=1, group="colsum"))
        out.append(mk(f"colsum-small-{o}-m20", SMALL, 20, 48, 36, True, tB, colsum=True, group="colsum"))
        out.append(mk(f"colsum-dma-{o}-split", DMA, 100, 48, 2304, True, tB, colsum=True, ksplit=9, f4=False, group="colsum"))
        out.append(mk(f"colsum-big-{o}-split", BIG, 100, 48, 2304, True, tB, colsum=True, offA=1, ksplit=9, f4=False, beta=1.0, group="colsum"))
        out.append(mk(f"colsum-small-{o}-split", SMALL, 20, 48, 2304, True, tB, colsum=True, ksplit=9, f4=False, group="colsum"))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


MM_CASES = _mm_cases()
MM_RUN = [c for c in MM_CASES if c["kernel"] >= 0]
MM_REFUSED = [c for c in MM_CASES if c["kernel"] < 0]
SPOT_CASES = ["dma-TN-m48n48k4", "heads-big-all-strides", "epi-NT-n51-relu-beta1", "strides-small-TN", "strides-dma-NN", "strides-big-NT"]


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------------
def _nan(n):
    return np.full(n, np.nan, dtype=np.float32)


def _sentinel(n):
    return np.full(n, SENTINEL_BITS, dtype=np.uint32).view(np.float32)


def _guard(ld):
    return r4(4 * ld + 16)


def _zoffs(c, X):
    z = np.arange(c["batch"])
    return (z // c["H"]) * c["strides"][f"s{X}b"] + (z % c["H"]) * c["strides"][f"s{X}h"]


def _index(base, zoffs, rows, width, ld):
    """Float index of element (z, r, col) inside the allocation."""
    return base + zoffs[:, None, None] + np.arange(rows)[None, :, None] * ld + np.arange(width)[None, None, :]


def _draw(rs, regime, shape):
    if regime == "exact":
        return rs.randint(-3, 4, size=shape).astype(np.float32)
    return rs.standard_normal(shape).astype(np.float32)


def live_rows(c):
    return c["M"] if c["m_dev"] is None else c["m_dev"]


def build(c, regime, seed=0):
    """Host arrays of a case: flat float32 allocations A, B, C (and bias, colsum, m_dev, a_rows where the case has them), the float offset of each
    base pointer inside its allocation (`base`), and the index arrays `idx` [batch, rows, width] of the logical elements."""
    rs = np.random.RandomState((seed * 1000003 + sum((i + 1) * ord(ch) for i, ch in enumerate(c["data"])) * 2 + (regime == "exact")) % (2 ** 31))
    M, N, K, b = c["M"], c["N"], c["K"], c["batch"]
    tall = M + 37 if c["a_rows"] else M
    rA, wA = (K, M) if c["tA"] else (tall, K)
    rB, wB = (N, K) if c["tB"] else (K, N)
    out, base, idx = {}, {}, {}
    for X, rows, width, ld, fill in (("A", rA, wA, c["lda"], _nan), ("B", rB, wB, c["ldb"], _nan), ("C", M, N, c["ldc"], _sentinel)):
        z = _zoffs(c, X)
        g = _guard(ld)
        base[X] = g + c[f"off{X}"]
        out[X] = fill(base[X] + int(z.max()) + rows * ld + g)
        idx[X] = _index(base[X], z, rows, width, ld)
    if c["zero_pad"]:                                                   # zeros behind K up to a multiple of 4, NaN beyond
        out["A"][_index(base["A"], _zoffs(c, "A"), rA, r4(K), c["lda"])] = 0.0
    out["A"][idx["A"]] = _draw(rs, regime, idx["A"].shape)
    out["B"][idx["B"]] = _draw(rs, regime, idx["B"].shape)
    if c["beta"] != 0.0:
        out["C"][idx["C"]] = _draw(rs, regime, idx["C"].shape)
    elif c["c_is_zero"]:
        out["C"][idx["C"]] = 0.0
    if c["bias"]:
        out["bias"] = np.concatenate([_nan(8), _draw(rs, regime, N), _nan(8)])
        base["bias"] = 8
    if c["colsum"]:
        out["colsum"] = _sentinel(16 + M + 16)
        out["colsum"][16:16 + M] = _draw(rs, regime, M)
        base["colsum"] = 16
    if c["a_rows"]:
        out["a_rows"] = rs.randint(0, tall, size=M + 8).astype(np.int32)   # repeats are likely; the 8 behind M are valid rows too
        out["a_rows"][:2] = out["a_rows"][2]                                # ... and certain
    if c["m_dev"] is not None:
        out["m_dev"] = np.array([c["m_dev"]], dtype=np.int32)
    out["base"], out["idx"] = base, idx
    return out


def mm_fields(c, ptrs, arrays):
    """Field values of dygnn_mm_args for allocations that start at the addresses `ptrs` (a dict like the arrays)."""
    base = arrays["base"]
    f = dict(A=ptrs["A"] + 4 * base["A"], B=ptrs["B"] + 4 * base["B"], C=ptrs["C"] + 4 * base["C"],
             bias=ptrs["bias"] + 4 * base["bias"] if c["bias"] else None, colsum_out=ptrs["colsum"] + 4 * base["colsum"] if c["colsum"] else None,
             m_dev=ptrs["m_dev"] if c["m_dev"] is not None else None, a_rows=ptrs["a_rows"] if c["a_rows"] else None,
             lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], M=c["M"], N=c["N"], K=c["K"], batch=c["batch"], H=c["H"], alpha=c["alpha"], beta=c["beta"],
             tA=int(c["tA"]), tB=int(c["tB"]), relu=int(c["relu"]), c_is_zero=int(c["c_is_zero"]), a_kpad=int(c["a_kpad"]))
    f.update(c["strides"])
    return f


def fake_fields(c):
    """The same fields with made-up, never followed addresses of the case's alignment (for the host-only path queries)."""
    arrays = dict(base=dict(A=c["offA"], B=c["offB"], C=c["offC"], bias=0, colsum=0))
    ptrs = {k: FAKE_BASE * (i + 1) for i, k in enumerate(("A", "B", "C", "bias", "colsum", "m_dev", "a_rows"))}
    return mm_fields(c, ptrs, arrays)


def operands(c, arrays):
    """op(A) [batch, M, K], op(B) [batch, K, N], C0 [batch, M, N] (zeros where the call does not read C), bias [N], colsum0 [M]: float64,
    read back from the buffers the device reads."""
    A = arrays["A"][arrays["idx"]["A"]].astype(np.float64)
    B = arrays["B"][arrays["idx"]["B"]].astype(np.float64)
    if c["a_rows"]:
        A = A[:, arrays["a_rows"][:c["M"]], :]
    opA = A.transpose(0, 2, 1) if c["tA"] else A
    opB = B.transpose(0, 2, 1) if c["tB"] else B
    C0 = arrays["C"][arrays["idx"]["C"]].astype(np.float64) if c["beta"] != 0.0 else np.zeros((c["batch"], c["M"], c["N"]))
    bias = arrays["bias"][8:8 + c["N"]].astype(np.float64) if c["bias"] else np.zeros(c["N"])
    cs0 = arrays["colsum"][16:16 + c["M"]].astype(np.float64) if c["colsum"] else None
    return opA, opB, C0, bias, cs0


def reference(c, arrays):
    """relu?(alpha op(A) @ op(B) + bias + beta C0) per batch in float64 and its elementwise bound; the column sums colsum0 + sum_k op(A)[m][k]
    and theirs (None without colsum_out).  Returns dict(C, C_bound, colsum, colsum_bound)."""
    opA, opB, C0, bias, cs0 = operands(c, arrays)
    ref = c["alpha"] * np.matmul(opA, opB) + bias[None, None, :] + c["beta"] * C0
    if c["relu"]:
        ref = np.maximum(ref, 0.0)
    mag = abs(c["alpha"]) * np.matmul(np.abs(opA), np.abs(opB)) + np.abs(bias)[None, None, :] + np.abs(c["beta"] * C0)
    g = 2.0 * (c["K"] + 4) * U
    r = dict(C=ref, C_bound=g * mag, colsum=None, colsum_bound=None)
    if cs0 is not None:
        r["colsum"] = cs0 + opA[0].sum(axis=1)
        r["colsum_bound"] = g * (np.abs(cs0) + np.abs(opA[0]).sum(axis=1))
    return r


# ---- dw_grouped ---------------------------------------------------------------------------------------------------------------------------------
def dw_problem(M, N, lda=None, ldb=None, ldc=None, colsum=True, offA=0):
    return dict(M=M, N=N, lda=r4(M) if lda is None else lda, ldb=N + 4 if ldb is None else ldb, ldc=N + 3 if ldc is None else ldc, colsum=colsum,
                offA=offA)


DW_SHAPES = [dict(M=4, N=4), dict(M=30, N=100, lda=32), dict(M=128, N=208), dict(M=132, N=212), dict(M=260, N=420)]
DW_KS = [1, 15, 16, 31, 32, 33, 200, 700]
DW_SINGLE = [dict(name=f"dw-k{K}-m{s['M']}n{s['N']}", K=K, problems=[dw_problem(**s)], regime="exact") for K in DW_KS for s in DW_SHAPES]
DW_FIVE = dict(name="dw-five", K=200, regime="exact",
               problems=[dw_problem(30, 100, lda=32, colsum=True), dw_problem(132, 212, colsum=False), dw_problem(4, 4, ldc=9, colsum=False),
                         dw_problem(260, 420, lda=264, colsum=True), dw_problem(128, 208, ldb=216, colsum=False)])
DW_ROUNDED = [dict(name=f"dw-rounded-k{K}-m{s['M']}n{s['N']}", K=K, problems=[dw_problem(**s)], regime="rounded")
              for K, s in ((33, DW_SHAPES[1]), (200, DW_SHAPES[3]), (700, DW_SHAPES[4]))]
DW_CASES = DW_SINGLE + [DW_FIVE] + DW_ROUNDED
DW_REFUSED = [dict(name="dw-refused-A+1", K=32, problems=[dw_problem(128, 208, offA=1)]),
              dict(name="dw-refused-ldb-mod4", K=32, problems=[dw_problem(128, 100, ldb=101)]),
              dict(name="dw-refused-n-mod4", K=32, problems=[dw_problem(128, 102, ldb=108)]),
              dict(name="dw-refused-m-mod4-unpadded", K=32, problems=[dw_problem(30, 100, lda=30)]),
              dict(name="dw-refused-too-many", K=32, problems=[dw_problem(4, 4)] * (DW_MAX_PROBLEMS + 1))]


def dw_build(case, seed=0):
    """Per problem: flat allocations A [K][lda], B [K][ldb] (NaN outside the logical columns -- for M % 4 != 0 the columns up to round_up(M, 4)
    are read into accumulator rows that are never written, NaN there too), C [M][ldc] and colsum pre-filled with values inside, the sentinel
    outside; base offsets and index arrays as in build()."""
    rs = np.random.RandomState((seed * 1000003 + sum(map(ord, case["name"])) * 31) % (2 ** 31))
    K, regime, out = case["K"], case.get("regime", "exact"), []
    z = np.zeros(1, dtype=np.int64)
    for p in case["problems"]:
        a, base, idx = {}, {}, {}
        for X, rows, width, ld, fill in (("A", K, p["M"], p["lda"], _nan), ("B", K, p["N"], p["ldb"], _nan), ("C", p["M"], p["N"], p["ldc"], _sentinel)):
            g = _guard(ld)
            base[X] = g + (p["offA"] if X == "A" else 0)
            a[X] = fill(base[X] + rows * ld + g)
            idx[X] = _index(base[X], z, rows, width, ld)[0]
            a[X][idx[X]] = _draw(rs, regime, idx[X].shape)
        if p["colsum"]:
            a["colsum"] = _sentinel(16 + p["M"] + 16)
            a["colsum"][16:16 + p["M"]] = _draw(rs, regime, p["M"])
            base["colsum"] = 16
        a["base"], a["idx"] = base, idx
        out.append(a)
    return out


def dw_reference(case, arrays):
    """Per problem: C0 + A^T B and colsum0 + column sums of A in float64, with the bounds of the rounded regime."""
    g, out = 2.0 * (case["K"] + 4) * U, []
    for p, a in zip(case["problems"], arrays):
        A, B, C0 = (a[X][a["idx"][X]].astype(np.float64) for X in "ABC")
        r = dict(C=C0 + A.T @ B, C_bound=g * (np.abs(C0) + np.abs(A).T @ np.abs(B)), colsum=None, colsum_bound=None)
        if p["colsum"]:
            cs0 = a["colsum"][16:16 + p["M"]].astype(np.float64)
            r["colsum"], r["colsum_bound"] = cs0 + A.sum(axis=0), g * (np.abs(cs0) + np.abs(A).sum(axis=0))
        out.append(r)
    return out
