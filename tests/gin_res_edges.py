"""Shared by tests/test_gin_res_edges_cpu.py and tests/test_gin_res_edges_gpu.py: the shapes at the edges of what the run-time
instantiation of the single-launch GIN kernel (`k_gin_res`, csrc/mtfjsp_gin_resident.h) is eligible for, and an adjacency whose
in-edges are as far apart as an instance allows.  Test infrastructure only.

What each case reaches (T = J * M rows per instance; ipc instances per workgroup = ceil(B / 256), 576 rows = 18 row tiles of 32):
the 6-tile aggregation ring (sources up to T - 1 rows away: two tiles at T >= 33), the pooling over 16-row chunks split at instance
boundaries (two or three instances in a tile below T = 32), the pooled tail (five chunks per instance at T = 65), the prologue's
clamps and its f64 conversion (three passes only in a full workgroup), the candidate table [ipc][J]."""
import numpy as np

CUS = 256
GENERIC = "k_gin_res"

# (J, M, E, B, observation dtype) -> (T, instances per workgroup, workgroups, instances of the last workgroup) on 256 compute units
CASES = [
    ((4, 4, 2, 9216, "f32"), (16, 36, 256, 36)),     # minimum T, 576 rows exactly, two instances per tile, the most instances per workgroup
    ((4, 4, 2, 8965, "f64"), (16, 36, 250, 1)),      # ragged last workgroup; f64 conversion in full workgroups and in one of 16 rows
    ((6, 3, 2, 700, "f32"), (18, 3, 234, 1)),        # boundaries at 18 and 36: a tile with two boundaries, chunks cut off 16
    ((5, 6, 2, 4852, "f32"), (30, 19, 256, 7)),      # 570 of 576 rows used: 6 idle rows in every workgroup
    ((4, 8, 2, 512, "f32"), (32, 2, 256, 2)),        # instance = tile
    ((3, 11, 2, 1279, "f32"), (33, 5, 256, 4)),      # one row past a tile: every instance straddles
    ((7, 9, 2, 300, "f32"), (63, 2, 150, 2)),        # one short of two tiles
    ((8, 8, 2, 2304, "f64"), (64, 9, 256, 9)),       # 576 rows exactly, f64, instance = two tiles: sources up to 63 rows away, next tile only
    ((5, 13, 2, 2048, "f32"), (65, 8, 256, 8)),      # maximum T: five chunks per instance
    ((13, 5, 2, 2041, "f32"), (65, 8, 256, 1)),      # maximum T with 13 candidates per instance, ragged
]
ADJACENCIES = ("env", "far")
# the global critic's forward (no candidates) runs on these, `far` adjacency
CRITIC_CASES = [c for c in CASES if c[1][0] in (16, 65)]


def case_id(case):
    J, M, E, B, obs = case[0]
    return f"{J}x{M}x{E}x{B}:{obs}"


def case_name(size, adj, streaming=False):
    """the (case) key of tests/error_budget.py"""
    J, M, E, B, obs = size
    return f"gin_res_edges:{J}x{M}x{E}x{B}:{obs}:{adj}" + (":streaming" if streaming else "")


def shops(M, E):
    """Shops of the environment that supplies a case's observation.  The library takes only n_machine divisible by n_edge (the reference
    stacks the shop lists into an array), and the table has odd M beside E = 2: those cases run as ONE shop.  The shop count shapes the
    transport times and nothing the GIN encoder sees the shape of; the case keeps its name."""
    return E if M % E == 0 else 1


def perturb(weight_dicts, seed):
    """non-trivial BatchNorm affine parameters (the default initialiser has gamma 1 / beta 0), as tests/test_encoder_sizes_gpu.py::_perturb"""
    rs = np.random.RandomState(seed)
    for d in weight_dicts:
        for k in d:
            if "batch_norms" in k or k.startswith("bn."):
                d[k] = (rs.uniform(0.5, 1.5, d[k].shape) if k.endswith("weight") else rs.uniform(-0.5, 0.5, d[k].shape)).astype(np.float32)


def edge_weights(ell_col, ell_val):
    """the non-zero edge weights an observation holds, each as often as it occurs (durations and transport times as integers: a few
    hundred distinct values with a mean of 3 .. 15 and a tail to several hundred)"""
    v = np.asarray(ell_val, np.float32)[np.asarray(ell_col) >= 0]
    return v[v != 0]


def far_adjacency(B, T, seed, weights):
    """-> (col [B,T,2] int32, val [B,T,2] float32): a well-formed adjacency (every index in [-1, T), every weight one of `weights`,
    the non-zero edge weights of an observation) whose in-edges span the instance.  Row a gets source T-1-a (the mirror; none where that is
    a itself) in one entry and (a + T//2) % T in the other; odd instances hold them in the other order.  Rows a = 2 mod 5 keep the
    mirror edge only, rows a = 5 mod 7 keep none (rows 0 and T-1 keep theirs at every T of the table: the distance reaches T-1 both ways).
    A weight is drawn from `weights` as given, so a value that occurs often there occurs often here: the magnitudes AND their
    frequencies are the environment's.  (Drawn from the distinct values instead, every row carries the environment's rarest and
    largest weights, and at J5M13 the first Linear's outputs leave the range of the kernel's fixed-point statistics: the forward then
    repeats on the f32-instruction kernels, as designed, and a test of `k_gin_res` has not run it.)"""
    w = np.asarray(weights, np.float32).ravel()
    assert w.size and (w != 0).all() and np.isfinite(w).all()
    a = np.arange(T)
    mirror = T - 1 - a
    mirror[mirror == a] = -1
    src = np.stack([mirror, (a + T // 2) % T], 1)
    src[a % 5 == 2, 1] = -1
    src[a % 7 == 5] = -1
    col = np.broadcast_to(src, (B, T, 2)).copy()
    col[1::2] = col[1::2, :, ::-1]
    val = w[np.random.RandomState(seed).randint(w.size, size=(B, T, 2))]
    val[col < 0] = 0
    return col.astype(np.int32), val.astype(np.float32)


def tile_distance(col, T, ipc):
    """[B,T,2] |tile of the source - tile of the row| with workgroup-relative rows (instance b of the batch is instance b % ipc of its
    workgroup, row (b % ipc) * T + a, tile = row >> 5); -1 where there is no edge"""
    col = np.asarray(col)
    B = col.shape[0]
    base = (np.arange(B) % ipc * T)[:, None, None]
    row = base + np.arange(T)[None, :, None]
    return np.where(col >= 0, np.abs(((base + col) >> 5) - (row >> 5)), -1)
