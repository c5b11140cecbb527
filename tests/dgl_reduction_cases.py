"""Shapes of tests/test_gpu_dgl_reductions.py (and of tests/test_dgl_reductions_host.py, which holds their inputs to the conditioning the
tolerance rule relies on): the tile edges of the channels-last kernels of step_amd/csrc/dgl_conv_mfma.hip / dgl.hip whose BatchNorm and
bias sums are reduced per workgroup through LDS and one in-register wave sum.

conv1_fwd_cl_kernel: a lane owns runs of RUN = 8 consecutive time steps, a wave 2 x 512, a workgroup SPAN = 4096 of the T - 9 conv1
outputs.  fc_unpermute_kernel: a workgroup covers FC_SPAN = 256 of the T - 18 conv2 outputs of one fc row."""
RUN, SPAN, FC_SPAN = 8, 4096, 256

# T - 9 at every edge of conv1's tiling: the smallest the entry point accepts (T = 19: T - 9 = 10; the entry points refuse T - 9 = 1), one
# short of / exactly / one past two runs, one short of / exactly / one past a workgroup, two workgroups and one step.
CONV1_T1 = (10, 15, 16, 17, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1)
EXACT_SHAPES = [(N, t1 + 9) for N in (3, 13) for t1 in CONV1_T1]
# the tolerance rule needs live BatchNorm3 features: no N below 13 (tests/direct_ref.py), 33 nodes where the series is a few steps long;
# 14 nodes at two workgroups and one step: with 13 the float32 oracle itself is 1.6e-3 off float64 on conv2_b (a cancelling sum)
EDGE_SHAPES = [(33 if t1 < 100 else (14 if t1 > 2 * SPAN else 13), t1 + 9) for t1 in CONV1_T1]
# T - 18 around multiples of fc_unpermute's span
FC_SHAPES = [(13, t2 + 18) for t2 in (FC_SPAN - 1, FC_SPAN, FC_SPAN + 1, 2 * FC_SPAN + 1)]
# time slices (bounds over the T - 18 conv2 columns; a slice's own conv1 columns are b - a, the 9 behind them are halo): no bound is a
# multiple of RUN, so every halo starts inside a lane's run -- 197 = 24 * 8 + 5 in the first wave, 4101 = SPAN + 5 in the second
# workgroup's first run
SLICED = [(13, 600, ((0, 197), (197, 390), (390, 582))), (13, 4500, ((0, 4101), (4101, 4482)))]
REUSE_SHAPES = [(13, SPAN + 1 + 9)]

TOLERANCE_SHAPES = sorted(set(EDGE_SHAPES + FC_SHAPES + [(N, T) for N, T, _ in SLICED] + REUSE_SHAPES))
