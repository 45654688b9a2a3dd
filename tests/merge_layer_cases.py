"""Cases, seeded inputs and the float64 reference of the link-predictor head (MergeLayer: dyglib_amd/modules.py over
dygnn_merge_layer_sigmoid / _logits / _backward, dyglib_amd/csrc/merge_layer.hip).  Importable without a GPU.

The head picks one of four forward kernels by (n, dim, hidden): G = one workgroup per row, R1 = 4 rows per workgroup, R4 = 16 rows per
workgroup (both on the 4x4x1 MFMA, 16-wide k chunks through a four-deep register ring, one wave per 16 hidden units), M = one wave per 16 rows
(16x16x4 MFMA, passes of 64 hidden units).  Every width below is there for an edge of one of them; every row count is the smallest that reaches
a regime or one of its ragged ends.  The table states the path it INTENDS for each case; tests/test_merge_layer_gpu.py reads the path the
library takes from dygnn_merge_layer_forward_path and compares.

Reference: z = relu(cat(a, b) @ W1.T + b1) @ w2 + b2, p = sigmoid(z) in float64 (numpy); gradients by torch autograd through the same
expression in float64.  Parameters are drawn as nn.Linear's default initialisation draws them (weights and biases uniform within
1 / sqrt(fan_in)); (172, 172) also runs with synthetic.make_merge_layer_params(7), the set the older tests use."""
import functools

import numpy as np
import torch

from dyglib_amd import synthetic as syn

G, R1, R4, M = 0, 1, 2, 3
PATH_NAMES = {G: "G", R1: "R1", R4: "R4", M: "M"}

# ---- forward -------------------------------------------------------------------------------------------------------------------------------
ROW_BLOCK_WIDTHS = [            # dim % 4 == 0 and hidden <= 256: G below 64 rows, R1 below 2048, R4 from there
    (172, 172),                 # the workload
    (4, 4),                     # K = 8 < 16: one partly filled k chunk (lanes whose k slice lies beyond the row)
    (8, 16),                    # exactly one chunk and one hidden tile
    (12, 20),                   # 1.5 chunks (fewer than the ring is deep), 1.25 tiles
    (36, 100),                  # 5 chunks: the ring wraps once, with a tail
    (128, 256),                 # the ldx = k16 + 16 branch; 16 waves = a 1024-thread workgroup
    (172, 170),                 # hidden % 4 != 0
]
MFMA_WIDTHS = [                 # hidden > 256: G below 2048 rows, M from there
    (172, 260),                 # four full passes of 64 hidden units and one with 4 live
    (64, 320),                  # five exact passes, K = 128
]
N_OF_PATH = {
    G: (1, 63),
    R1: (64, 65, 67, 2047),                 # last workgroup with 1 and with 3 rows
    R4: (2048, 2049, 2063),                 # last workgroup with 1 and with 15 rows
    M: (2048, 2049, 2063, 2095, 2111),      # last wave with 1 / 15 rows, its workgroup's other waves leaving early; last workgroups with 3 and 4 live waves
}
RAGGED_N = {G: (63,), R1: (65, 67, 2047), R4: (2049, 2063), M: (2049, 2063, 2095, 2111)}


def _forward_table():
    rows = []
    for dim, hidden in ROW_BLOCK_WIDTHS:
        rows += [(dim, hidden, n, path, "nn") for path in (G, R1, R4) for n in N_OF_PATH[path]]
    rows += [(172, 172, n, path, "syn7") for path in (G, R1, R4) for n in N_OF_PATH[path]]
    rows += [(170, 172, n, G, "nn") for n in (1, 63, 2100)]                      # dim % 4 != 0: G at every n
    for dim, hidden in MFMA_WIDTHS:
        rows += [(dim, hidden, n, G, "nn") for n in N_OF_PATH[G] + (2047,)]      # (2047: the last n before M)
        rows += [(dim, hidden, n, M, "nn") for n in N_OF_PATH[M]]
    # rows too long for a row block's LDS stage: 16 rows of (516, 4) do not fit 64 KB, 4 do; 4 rows of (4100, 4) do not, one does, and from
    # 2048 rows on M (which stages nothing) takes them: M with hidden < 64, a partial first pass
    rows += [(516, 4, 2047, R1, "nn"), (516, 4, 2048, R1, "nn"), (4100, 4, 63, G, "nn"), (4100, 4, 64, G, "nn"), (4100, 4, 2048, M, "nn")]
    return rows


FORWARD_CASES = _forward_table()                    # (dim, hidden, n, intended path, parameter set)
LONG_ROW_PAIRS = [((516, 4), 2047, 2048), ((4100, 4), 63, 64), ((4100, 4), 64, 2048)]
ONE_PER_PATH = [(172, 172, 63, G), (172, 172, 67, R1), (172, 172, 2063, R4), (172, 260, 2063, M)]      # permutation and NaN tests


def case_id(c):
    dim, hidden, n, *rest = c
    tail = "".join(f"-{PATH_NAMES.get(r, r)}" for r in rest if r != "nn")
    return f"d{dim}h{hidden}n{n}{tail}"


# ---- backward (library contract: dim % 4 == 0, hidden % 4 == 0, hidden <= 192) --------------------------------------------------------------
BACKWARD_WIDTHS = [
    (172, 172),                 # the workload
    (4, 4), (8, 16), (12, 20), (36, 100),
    (128, 192),                 # the largest hidden; K = 256: exactly one 64-feature set per wave
    (160, 48),                  # K = 320: wave 0 gets two sets; only wave 0 owns hidden tiles
    (172, 52),                  # hidden tiles end inside wave 1
]
BACKWARD_N = (1, 16, 17, 33, 130)       # a ragged 16-row workgroup; the weight-gradient K-split with one chunk, a one-row tail, several chunks
BACKWARD_CASES = [(dim, hidden, n, "nn") for dim, hidden in BACKWARD_WIDTHS for n in BACKWARD_N] + [(172, 172, n, "syn7") for n in BACKWARD_N]
PRE_MARGIN = 1e-5                       # no float64 pre-activation of a backward case is closer to the ReLU kink than this
# input seeds are bumped for the cases whose first draw puts a pre-activation inside the margin (tests/test_merge_layer_cases_cpu.py asserts it)
BACKWARD_SALT = {(172, 172, 130, "nn"): 2, (12, 20, 130, "nn"): 1, (36, 100, 33, "nn"): 1, (36, 100, 130, "nn"): 1, (128, 192, 130, "nn"): 3,
                 (160, 48, 16, "nn"): 1, (172, 172, 130, "syn7"): 1}


# ---- parameters and inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params(dim, hidden, kind="nn"):
    """fc1 [hidden, 2 dim], fc2 [1, hidden] with their biases, float32, read-only."""
    if kind == "syn7":
        assert dim == hidden
        p = syn.make_merge_layer_params(7, dim)
    else:
        rs = np.random.RandomState([20241, dim, hidden])
        k1, k2 = 1.0 / np.sqrt(2 * dim), 1.0 / np.sqrt(hidden)
        p = {"fc1.weight": rs.uniform(-k1, k1, size=(hidden, 2 * dim)), "fc1.bias": rs.uniform(-k1, k1, size=(hidden,)),
             "fc2.weight": rs.uniform(-k2, k2, size=(1, hidden)), "fc2.bias": rs.uniform(-k2, k2, size=(1,))}
    p = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}
    for v in p.values():
        v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _forward_rows(dim, hidden):
    nmax = max(c[2] for c in FORWARD_CASES if c[:2] == (dim, hidden))
    rs = np.random.RandomState([777, dim, hidden])
    a, b = rs.standard_normal((nmax, dim)).astype(np.float32), rs.standard_normal((nmax, dim)).astype(np.float32)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def forward_inputs(dim, hidden, n):
    """a, b [n, dim] standard normal float32: the first n rows of the width's stream, so two n of one width share their common rows."""
    a, b = _forward_rows(dim, hidden)
    return a[:n], b[:n]


@functools.lru_cache(maxsize=None)
def backward_inputs(dim, hidden, n, kind="nn"):
    rs = np.random.RandomState([999, dim, hidden, n, BACKWARD_SALT.get((dim, hidden, n, kind), 0)])
    out = rs.standard_normal((n, dim)).astype(np.float32), rs.standard_normal((n, dim)).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    for v in out:
        v.setflags(write=False)
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def reference_pre(a, b, p):
    """Hidden pre-activations cat(a, b) @ W1.T + b1, float64 [n, hidden]."""
    x = np.concatenate([a, b], axis=1).astype(np.float64)
    return x @ p["fc1.weight"].astype(np.float64).T + p["fc1.bias"].astype(np.float64)


def reference_forward(a, b, p):
    """(logits, probabilities), float64 [n]."""
    h = np.maximum(reference_pre(a, b, p), 0.0)
    z = h @ p["fc2.weight"].astype(np.float64)[0] + float(p["fc2.bias"][0])
    return z, 1.0 / (1.0 + np.exp(-z))


@functools.lru_cache(maxsize=None)
def forward_reference(dim, hidden, n, kind="nn"):
    z, pr = reference_forward(*forward_inputs(dim, hidden, n), params(dim, hidden, kind))
    z.setflags(write=False), pr.setflags(write=False)
    return z, pr


@functools.lru_cache(maxsize=None)
def backward_reference(dim, hidden, n, kind="nn"):
    """d(sum(z * g)) / d(a, b, fc1.weight, fc1.bias, fc2.weight, fc2.bias) by torch autograd in float64, and the logits."""
    a, b, g = backward_inputs(dim, hidden, n, kind)
    p = params(dim, hidden, kind)
    t = {k: torch.from_numpy(np.array(v)).double().requires_grad_(True)
         for k, v in (("a", a), ("b", b), ("w1", p["fc1.weight"]), ("b1", p["fc1.bias"]), ("w2", p["fc2.weight"]), ("b2", p["fc2.bias"]))}
    z = torch.relu(torch.cat([t["a"], t["b"]], dim=1) @ t["w1"].T + t["b1"]) @ t["w2"].T + t["b2"]
    (z[:, 0] * torch.from_numpy(np.array(g)).double()).sum().backward()
    out = {k: v.grad.numpy() for k, v in t.items()}
    out["z"] = z.detach().numpy()[:, 0]
    for v in out.values():
        v.setflags(write=False)
    return out
