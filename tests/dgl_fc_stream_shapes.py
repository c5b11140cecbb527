"""Shapes (N, T) of the streaming fc kernels' tests (step_amd/csrc/dgl_fc_stream.hip), shared by tests/test_gpu_dgl_fc_stream.py and the
host-side conditioning check tests/test_dgl_fc_stream_host.py.  The constants repeat the kernels' own constexprs:

  forward          FS_TM = 320 rows of a row tile, FS_KS = 64 bf16 of a k step (4 time steps of 16 channels), FS_RING = 3 stages,
                   FS_RANGES = 96 k ranges at most, and never more than the staged GEMM reserves workspace for:
                   min(ceil(768 / ceil(N / 128)), floor(ceil(K / 64) / 4)) partial results, K = 16 (T - 18)
  weight gradient  WG_TN = 320 resident nodes (graphs beyond stay on the staged GEMM: dgl_fc_stream_wgrad_ok, pinned on both sides in
                   the GPU test), WG_CT = 32 bf16 of a column tile (2 time steps), WG_RING = 4 stages, 256 workgroups at most
"""
FS_TM, FS_KS, FS_RING, FS_RANGES = 320, 64, 3, 96
WG_TN, WG_CT, WG_RING, WG_GROUPS = 320, 32, 4, 256
STEPS_PER_KS = FS_KS // 16          # time steps of a forward k step
STEPS_PER_CT = WG_CT // 16          # time steps of a weight-gradient column tile


def fwd_ranges(N, T2):
    """(k steps, k steps per range, ranges launched) of the forward kernel, as dgl_fc_stream_fwd chooses them"""
    ksteps = -(-16 * T2 // FS_KS)
    tiles = -(-N // 128)
    reserved = max(1, min(-(-768 // tiles), ksteps // 4))
    ranges = max(1, min(reserved, FS_RANGES, ksteps)) if reserved > 1 else 1
    per = -(-ksteps // ranges)
    return ksteps, per, -(-ksteps // per)


def wgrad_groups(T2):
    """(column tiles, tiles per workgroup, workgroups launched) of the weight-gradient kernel"""
    tiles = -(-16 * T2 // WG_CT)
    per = -(-tiles // min(tiles, WG_GROUPS))
    return tiles, per, -(-tiles // per)


def _around(x):
    return [x - 1, x, x + 1]


# T - 18 one below, at and one above: one forward k step (3, 4, 5); one weight-gradient column tile (1, 2, 3); a full weight-gradient
# ring (7, 8, 9) and a full forward ring (11, 12, 13); a forward k range -- 80 time steps are 20 k steps in 5 ranges of 4, 81 make the
# last step ragged and the last range a single step, 79 leave the last step one time step short; 770 time steps are 193 k steps,
# which 48 reserved ranges take in 5s: 39 ranges, the last ragged, nine never launched -- and the weight gradient's 256 workgroups
# (512 time steps are 256 tiles, 513 make 257 tiles in pairs).
T2_EDGES = sorted(set(_around(STEPS_PER_KS) + _around(STEPS_PER_CT) +_around(STEPS_PER_CT * WG_RING) + _around(STEPS_PER_KS * FS_RING)
                      + _around(80) + [770] + _around(STEPS_PER_CT * WG_GROUPS)))
SMALL_N = 13
# few nodes at every T - 18 edge (T - 18 = 1 with 33 nodes: 13 samples per BatchNorm2 channel are ill conditioned); every N edge at a
# ragged T - 18
N_EDGES = [SMALL_N, FS_TM - 1, FS_TM, FS_TM + 1]
EDGE_SHAPES = [(33 if t2 < 3 else SMALL_N, t2 + 18) for t2 in T2_EDGES] + [(n, 81 + 18) for n in N_EDGES[1:]] + [(307, 13 + 18)]
# the caller-visible scenarios: PEMS04's node count, two slices of 150 columns
SCENARIO = (307, 300 + 18)
SCENARIO_SLICES = ((0, 150), (150, 300))
AGREEMENT_SHAPES = [(SMALL_N, 81 + 18), (SMALL_N, 513 + 18), (FS_TM, 81 + 18), (FS_TM + 1, 81 + 18), SCENARIO]
ALL_SHAPES = sorted(set(EDGE_SHAPES + [SCENARIO] + AGREEMENT_SHAPES))
