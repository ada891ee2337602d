"""The shapes and forms of tests/test_hip_gemm_f16s_tiled.py, stated once: the GPU test runs them, tests/gemm_f16s_tiled_shapes_check.cpp
(through tests/test_gemm_f16s_tiled_shapes_cpu.py) holds them against the planner -- every launch and tail on the persistent kernel, every
one of its five tiles reached.

M: the node rows of the bench batch (2560), the same with a ragged last tile (+ 33), the tail rows of the 8-phase launches (1536), two
tiles with one live row in the second (65).  (N, K): the Linears of the forward that run on the persistent kernel; (3328, 512) at
M >= 2560 is the one launch with a full round of 128 x 128 tiles (the node-side projection), (2048, 128) the one of 64 x 128 tiles plus a
64 x 64 tail, (512, 32) the 64 x 64 tile at one k-slice per step (K is no multiple of 64).  The 128 x 64 tile takes N <= 64 and at least a
round of tiles: 65 536 + 33 rows of 64 columns at K = 32.  N = 96 and N = 100 are no multiple of the tile's width: the last column tile is cut
by N, so the sibling reads plane rows past N (zeros through the buffer descriptor) and takes the element-wise epilogue."""
M_LIST = (2560, 2560 + 33, 1536, 65)
NK_LIST = ((512, 512), (1024, 512), (512, 1024), (3328, 512), (256, 128), (512, 32), (2048, 128))
EXTRA = ((65536 + 33, 64, 32), (2560 + 33, 96, 512), (65, 100, 128))
SHAPES = tuple((M, N, K) for N, K in NK_LIST for M in M_LIST) + EXTRA
FORMS = ((0, 0), (0, 1), (1, 0), (6, 0), (6, 1))            # (additive operands, ReLU-on-A)
