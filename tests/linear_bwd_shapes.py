"""Shapes of the Linear backward's small-row tests, with the slice counts worked out by hand from the slicing rules: data only, so
tests/test_gpu_linear_bwd.py (which reads S back off the scratch on a GPU) and tests/test_route_table.py (which reads it off the
host-only plan, without one) assert the same figures."""

# (M, N, K, S): S = the slices the straight (k_gemm_tn) path cuts M rows into.
# mdt_op_linear_bwd_scratch_exact cannot confirm them: at every shape here it returns the need of the transposed-copy path,
# (N + K) Mp + ..., which exceeds the straight path's S (N K + N) + 64.  The GPU test reads S off the scratch instead and asserts
# it, and the route table (tests/c_client/route_table.cpp: the lin_bwd/ keys) states the plan's S for the same shapes on a machine
# without a GPU, so a retuned split that moves a shape off its edge shows in both.
M_EDGES = [(1, 64, 128, 1), (31, 64, 128, 1), (32, 64, 128, 1), (33, 64, 128, 1),    # one ragged / exactly full 32-row chunk
           (127, 64, 128, 1), (128, 64, 128, 1), (129, 64, 128, 1),                  # the slice-count floor M / 128
           (130, 64, 128, 1)]                                                        # a last chunk of 2 rows
N_EDGES = [(300, 16, 128, 2), (300, 48, 128, 2), (300, 80, 128, 2), (300, 240, 128, 2)]   # a partly empty last 64-wide n-tile
K_EDGES = [(300, 64, 16, 2),                       # smallest accepted
           (300, 64, 80, 2), (300, 64, 208, 2),    # ragged last k-tile
           (300, 64, 192, 2), (300, 64, 576, 2)]   # KT = 3: one tile, three tiles
MANY_SLICES = [(1024, 16, 16, 8),      # 8 full slices of 128 rows
               (1000, 80, 208, 7),     # slices of 160 rows, the last of 40
               (300, 48, 80, 2),       # 160 + 140 rows
               (257, 64, 128, 2)]      # 160 + 97 rows
SMALL_SHAPES = M_EDGES + N_EDGES + K_EDGES + MANY_SLICES
