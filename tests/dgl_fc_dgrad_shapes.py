"""Shapes of the tests of the graph learner's streaming fc input-gradient kernel (step_amd/csrc/dgl_fc_stream.hip,
fc_stream_dgrad_kernel), shared by tests/test_gpu_dgl_fc_dgrad.py and the host-side check tests/test_dgl_fc_dgrad_host.py.  The constants
repeat the kernel's constexprs:

  DG_TM = 320 nodes of a row tile (any number of row tiles), DG_CT = 64 bf16 of a column tile (4 time steps of 16 channels),
  DG_RING = 3 stages, DG_GROUPS = 256 workgroups at most: floor(256 / row tiles) column ranges per row tile, at least one;
  DG_MAX_RTILES = 3: graphs of more row tiles (N > 960) stay on the staged GEMM
  (dgl_fc_stream_dgrad_ok, pinned on both sides in tests/test_dgl_fc_dgrad_host.py)
"""
DG_TM, DG_CT, DG_RING, DG_GROUPS, DG_MAX_RTILES = 320, 64, 3, 256, 3
STEPS_PER_CT = DG_CT // 16          # time steps of a column tile


def dgrad_grid(N, T2):
    """(column tiles, tiles per workgroup, column ranges launched, row tiles) as dgl_fc_stream_dgrad chooses them"""
    tiles = -(-16 * T2 // DG_CT)
    rtiles = -(-N // DG_TM)
    ranges = max(1, min(DG_GROUPS // rtiles, tiles))
    per = -(-tiles // ranges)
    return tiles, per, -(-tiles // per), rtiles


def _around(x):
    return [x - 1, x, x + 1]


SMALL_N = 13
# T - 18 one below, at and one above one column tile (3, 4, 5: 5 leaves a last tile of one time step) and a full ring (11, 12, 13);
# 1024 time steps are 256 tiles, one per workgroup; 1025 are 257 tiles, which no longer divide: pairs, 129 workgroups, the last with one
# ragged tile of one time step -- the first shape at which a workgroup gets two tiles.  With three row tiles (641 nodes) 85 column ranges
# are left: 340 time steps are one tile each, 341 make 86 tiles in pairs.  The ring only turns inside a workgroup with more tiles than
# stages: 4100 time steps are 1025 tiles in fives (13 nodes), 1100 time steps on three row tiles 275 tiles in fours.
# The staged GEMM's side of the dispatch rule: 961 nodes (four row tiles).
T2_EDGES = sorted(set(_around(STEPS_PER_CT) + _around(STEPS_PER_CT * DG_RING) + [STEPS_PER_CT * DG_GROUPS, STEPS_PER_CT * DG_GROUPS + 1]))
# every N edge at a ragged T - 18 of more than a ring: 1 node, one below, at and one above a row tile, three row tiles the last with one
# row, PEMS04's 307
N_EDGES = [1, SMALL_N, DG_TM - 1, DG_TM, DG_TM + 1, 2 * DG_TM + 1, 307]
DIRECT_SHAPES = ([(SMALL_N, t2) for t2 in T2_EDGES] + [(n, 13) for n in N_EDGES if n != SMALL_N]
                 + [(2 * DG_TM + 1, 340), (2 * DG_TM + 1, 341), (SMALL_N, 4100), (2 * DG_TM + 1, 1100), (307, 300),
                    (DG_MAX_RTILES * DG_TM, 5), (DG_MAX_RTILES * DG_TM + 1, 5)])
# through the library: (N, T) with T - 18 = 81 (ragged: 21 tiles, the last of one time step), and the caller-visible scenario
LIBRARY_SHAPES = [(SMALL_N, 81 + 18), (DG_TM, 81 + 18), (DG_TM + 1, 81 + 18), (2 * DG_TM + 1, 81 + 18)]
SCENARIO = (307, 300 + 18)
SCENARIO_SLICES = ((0, 150), (150, 300))
ALL_LIBRARY_SHAPES = sorted(set(LIBRARY_SHAPES + [SCENARIO]))
